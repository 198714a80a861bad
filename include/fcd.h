/*
 * fcd.h -- C ABI of the MI355X-native batched CTC decoder (libfcd_hip.so).
 *
 * This is the drop-in boundary for fast-ctc-decode's hot path.  The reference exports no C ABI
 * of its own (only PyInit_fast_ctc_decode, /root/reference/src/lib.rs:617-628); its FFI seam is
 * the set of Rust search functions the PyO3 wrappers call with the GIL released.  Each entry
 * point below replaces one of those calls, batched over reads, and cites it:
 *
 *   fcd_viterbi_search_*      <- search::viterbi_search      src/search.rs:320-327 (call site src/lib.rs:199-208)
 *   fcd_beam_search_*         <- search::beam_search         src/search.rs:159-165 (call site src/lib.rs:353-361)
 *   fcd_crf_beam_search_*     <- search::crf_beam_search     src/search.rs:38-44   (call site src/lib.rs:274-282)
 *   fcd_crf_greedy_search_*   <- search::crf_greedy_search   src/search.rs:385-392 (call site src/lib.rs:237-246)
 *   fcd_beam_search_duplex_*  <- duplex::beam_search         src/duplex.rs:443-451 (call site src/lib.rs:474-484)
 *   fcd_crf_beam_search_duplex_* <- duplex::crf_beam_search  src/duplex.rs:652-661 (call site src/lib.rs:563-575)
 *   per-read status codes     <- enum SearchError            src/lib.rs:36-41
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / numpy / HIP types in any signature
 *     (a hipStream_t is passed as void*).
 *   - `*_dev` functions take DEVICE pointers (inputs already resident in HBM, outputs written to
 *     HBM) and only enqueue work on the handle's stream; `*_host` functions take HOST pointers,
 *     stage through the handle's workspace and return after synchronising.
 *   - strides are in ELEMENTS (the reference accepts arbitrarily strided ndarray views,
 *     src/lib.rs:198,352).
 *   - the device writes label INDICES into the caller's alphabet (1..N-1, 0 is the blank and is
 *     never emitted); strings are joined on the host (src/search.rs:293,358).
 *   - `path` values are the u32 row index at which the emitted label's tree node was created
 *     (src/search.rs:214,231,359); the reference's usize is narrowed, T must be < 2^28.
 *   - return value: FCD_OK or a negative FCD_E_* for API misuse / runtime failure;
 *     per-read search outcomes go to status[read] (FCD_ST_*).
 *   - one handle may be used by one host thread at a time (calls on a handle are serialised by
 *     an internal mutex); use one handle per thread / per stream for concurrency.
 */
#ifndef FCD_H
#define FCD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCD_VERSION_MAJOR 0
#define FCD_VERSION_MINOR 1

/* return codes */
enum {
    FCD_OK = 0,
    FCD_E_INVALID = -1,     /* bad argument (null pointer, negative size, unsupported shape) */
    FCD_E_HIP = -2,         /* a HIP runtime call failed; see fcd_last_error() */
    FCD_E_NOMEM = -3,       /* workspace allocation failed */
    FCD_E_UNSUPPORTED = -4, /* shape outside what the kernels implement */
    FCD_E_NODEVICE = -5     /* no usable gfx950 device */
};

/* per-read status, mirrors SearchError (src/lib.rs:36-41) */
enum {
    FCD_ST_OK = 0,
    FCD_ST_RAN_OUT_OF_BEAM = 1,   /* "Ran out of search space (beam_cut_threshold too high)" */
    FCD_ST_INCOMPARABLE = 2,      /* "Failed to compare values (NaNs in input?)" */
    FCD_ST_INVALID_ENVELOPE = 3,  /* "Invalid envelope values" */
    FCD_ST_BAD_STATE = 4,         /* the reference panics (aborts the process) here: a CRF state index outside [0,S),
                                     NaN / out-of-range init_state, or -- duplex -- an envelope whose upper bound moves
                                     back and then forward by less than a beam entry's window already covers
                                     (assert!(current_end < upper_bound), src/duplex.rs:363-366) */
    FCD_ST_INTERNAL = 5           /* tree arena exhausted -- a bug in workspace sizing */
};

/* duplex log-add flavour (SURVEY.md section 0 finding 3) */
enum {
    FCD_LOGADD_LOGSUMEXP = 0, /* reference built with --no-default-features */
    FCD_LOGADD_MAX = 1,       /* reference's default `fastexp` feature (exp() == 0.0) */
    /* FCD_LOGADD_LOGSUMEXP computes ln / exp / ln_1p correctly rounded -- a platform-independent definition.  The
     * reference computes them with whatever expf / logf / log1pf its process links (src/duplex.rs:17,25,50); this
     * flavour reproduces ONE such library bit for bit: glibc 2.35 on x86-64 with FMA (csrc/glibc235_math.h; verified
     * against that libm on every binary32 argument).  Strings then equal the reference's on such a host, not only on
     * >= 90 % of the pairs.  Slower: no fast paths. */
    FCD_LOGADD_LOGSUMEXP_GLIBC235 = 2
};

/* kernel selection for fcd_beam_search_* (0 = pick the fastest that supports the shape) */
enum {
    FCD_KERNEL_AUTO = 0,
    FCD_KERNEL_GENERIC = 1,  /* LDS-resident beam, any beam_size / alphabet */
    FCD_KERNEL_WAVE = 2,     /* register-resident beam: beam_size <= 8 with N <= 7, or beam_size <= 12
                                with N <= 5; packs two reads per wavefront when beam_size <= 5, N <= 5 */
    FCD_KERNEL_WAVE1 = 3,    /* the same kernel, always one read per wavefront */
    FCD_KERNEL_LANE = 4      /* one beam entry per lane: beam_size <= 64, N <= 8, plain (non-CRF) search */
};

/* Order of EQUAL probabilities in the prune of the beam searches (src/search.rs:122,262, src/duplex.rs:620,807:
 * sort_unstable_by on a list that is in ascending node order).  Up to 20 candidates Rust's sort is an insertion
 * sort and ties keep node order; above 20 it is the pattern-defeating quicksort of the pinned toolchain (Rust
 * 1.78.0, .github/workflows/test.yml:16), whose permutation of equal keys is a deterministic function of the list.
 *   FCD_TIE_PDQ178 (default)  on a step with more than 20 candidates in which a candidate that survives the
 *                  truncation ties with another one, that quicksort is replayed on the node-ordered list -- by the
 *                  whole wavefront in the register kernels (csrc/pdq178_wave.h, pdq178_reg.h), by one lane in the
 *                  LDS-resident ones (csrc/pdq178.h) -- and the search adopts its order; every other step is ranked
 *                  exactly on (probability desc, node asc), which is the same thing.  The quicksort was restated
 *                  from memory of library/core/src/slice/sort.rs (no Rust source or toolchain in the build image)
 *                  and then pinned, element for element, against a rustc-1.65 build of std found compiled in that
 *                  image (tools/verify/rust165_pdqsort.py) -- all of it but the two routines std changed in 2023,
 *                  whose LATER forms (Rust 1.78 as recalled) are the default.  The environment variable
 *                  FCD_PDQ178_STD_FORM (0 .. 3, read at load time; bit 0: break_patterns' generator as until 2022,
 *                  bit 1: partial_insertion_sort's shifting as until 2022) selects the earlier ones process-wide
 *                  for the 1-D searches (the duplex searches replay the default form only: csrc/pdq178.h says why;
 *                  none of 1024 BASELINE config-5 pairs decodes differently under another form);
 *                  tools/verify/pdq178_check.rs tells a holder of rustc 1.78.0 in one command which form it carries.
 *   FCD_TIE_STABLE ties always keep ascending node order (what rounds 1-3 shipped): one of the admissible answers
 *                  of an unstable sort, but not the one Rust 1.78 gives on about 0.05 % of BASELINE config-2 reads.
 * A handle follows the process default until fcd_set_tie_order names an order for it (FCD_TIE_DEFAULT: follow
 * again); the process default is FCD_TIE_PDQ178, or what the environment variable FCD_TIE_ORDER (pdq178 | stable)
 * says at load time, or what fcd_set_default_tie_order set last.  The lanes of a host job follow the handle the job
 * was begun on; a coalescer's own handles follow the process default. */
enum { FCD_TIE_DEFAULT = -1, FCD_TIE_PDQ178 = 0, FCD_TIE_STABLE = 1 };

typedef struct fcd_handle fcd_handle;

/* Shape/stride description of a batch of posterior matrices.
 *   1D searches: element (read r, row t, column j)        at base[r*stride_read + t*stride_t + j*stride_n]
 *   CRF searches: element (read r, row t, state s, col j) at base[r*stride_read + t*stride_t + s*stride_s + j*stride_n]
 * lengths (nullable): per-read row count T_r <= T (ragged batches); device pointer for *_dev,
 * host pointer for *_host.
 * Any non-negative strides are accepted.  Two layouts have kernels of their own in the HBM-bound searches
 * (viterbi_search, crf_greedy_search; 16-byte aligned base): READ-MAJOR, every read a contiguous (T, N) / (T, S, N) block
 * (stride_n = 1, stride_s = N, stride_t = S*N), and TIME-MAJOR, the (T, B, N) / (T, B, S, N) tensor a basecaller network
 * emits seen as a batch (stride_read = S*N, stride_t = B*S*N: no transposition needed).  The beam searches fetch one row
 * per step and read and run at the same speed on either. */
/* Element type of the posteriors.  Basecaller networks emit half precision; the reference only takes float32
 * (src/lib.rs:182,325: &PyArray<f32>), which costs its callers a host-side upcast.  f16 and bf16 convert to float32
 * EXACTLY, so a search on half-precision input IS the reference's search on the upcast matrix; the kernels convert
 * in registers while loading (no separate pass; the HBM-bound viterbi search streams half the bytes). */
enum { FCD_DTYPE_F32 = 0, FCD_DTYPE_F16 = 1, FCD_DTYPE_BF16 = 2 };

typedef struct fcd_batch {
    const void *post;   /* elements of type `dtype`: float (FCD_DTYPE_F32) or 16-bit words (F16 / BF16) */
    int64_t n_reads;
    int64_t T;          /* rows allocated per read */
    int64_t S;          /* CRF states; 1 for the plain searches */
    int64_t N;          /* alphabet size including the blank */
    int64_t stride_read;
    int64_t stride_t;
    int64_t stride_s;
    int64_t stride_n;
    const int64_t *lengths;
    int32_t dtype;      /* FCD_DTYPE_*; strides are in elements of that type (0 = float32: zero-initialised structs
                           keep their meaning) */
} fcd_batch;

/* Output of the 1D searches; every array has n_reads rows.
 *   labels : [n_reads * out_stride] u8   alphabet index of each emitted label, in sequence order
 *   path   : [n_reads * out_stride] u32  (nullable)
 *   qual   : [n_reads * out_stride] f32  (nullable; viterbi/crf_greedy only) the probability the
 *            reference feeds to phred() for each emitted label (src/search.rs:348-356,370-376)
 *   out_len: [n_reads] u32   number of emitted labels
 *   status : [n_reads] i32   FCD_ST_*  (nullable for viterbi)
 *   ambiguous: [n_reads][2] u32 (nullable; the beam searches -- fcd_beam_search_*, fcd_crf_beam_search_* and the
 *            two duplex searches, whose prune is the same sort_unstable_by, src/duplex.rs:620,807; device pointer
 *            for *_dev, host pointer for *_host) -- a TIE INSTRUMENT, not a reference output.  The reference
 *            orders candidates with sort_unstable_by (src/search.rs:122,262): a stable insertion sort up to
 *            20 elements, pdqsort -- implementation-defined tie order -- above.  Under FCD_TIE_STABLE the kernels
 *            break exact probability ties by ascending node index, which is what the stable path does; under
 *            FCD_TIE_PDQ178 (default) the steps counted in [r][0] are exactly the ones re-ranked by the restated
 *            quicksort.  The counters do not depend on the tie order within a step.
 *              [r][0] steps with MORE than 20 candidates in which a candidate that survives the truncation has
 *                     exactly the probability of another candidate.  0 for a read => its beam, set and order,
 *                     follows the reference step for step;
 *              [r][1] steps (any candidate count) with equal probabilities at ranks 0 / 1 or across the
 *                     truncation boundary.  0 for a read => no tie rule can change a kept set or the best entry.
 *            A read with either counter at 0 is pinned to the reference; the others can be settled with the
 *            oracle's exhaustive replay (oracle/fcd_oracle.h, fcdo_beam_search_all_tie_orders).
 *            Passing the array selects instrumented kernel instantiations (slower by a few percent).
 * out_stride must be >= the longest possible output (T is always enough). */
typedef struct fcd_result {
    uint8_t *labels;
    uint32_t *path;
    float *qual;
    uint32_t *out_len;
    int32_t *status;
    int64_t out_stride;
    uint32_t *ambiguous;
} fcd_result;

/* ---- library / handle ---- */
int fcd_version(void);                                   /* major*1000 + minor */
int fcd_device_count(void);                              /* number of visible HIP devices, 0 if none */
int fcd_create(int device, fcd_handle **out);            /* binds to a device, creates its own stream */
int fcd_destroy(fcd_handle *h);                         /* FCD_E_INVALID while a host job (fcd_*_host_begin) is open */
int fcd_set_stream(fcd_handle *h, void *hip_stream);     /* launch on this hipStream_t; NULL = the HIP null (legacy default) stream */
int fcd_reset_stream(fcd_handle *h);                     /* back to the handle's own non-blocking stream */
int fcd_synchronize(fcd_handle *h);                      /* waits for the handle's stream (and for overlapping calls, below) */
/* Overlapping calls (no counterpart in the reference, whose searches are synchronous: src/lib.rs:199).
 * A batch is as slow as its slowest read, and a batch of 4096 reads fills half of the chip's wavefront slots: under
 * FCD_TIE_PDQ178 a wide-beam read whose every step ties runs 2.3x as long as the rest of its batch, on
 * one wavefront, while the chip idles.  fcd_set_overlap(h, n), n in 2 .. 8: the *_dev beam searches (1-D and duplex)
 * are enqueued round-robin on n internal streams -- each behind the handle's stream AS IT STOOD WHEN THE CALL WAS
 * MADE, not behind one another, so the stragglers of a call run under the next calls.  Wide-beam jobs share ONE tree
 * arena whose slabs are handed out on the device, as many as the chip holds wavefronts (csrc/slab_pool.h); the other
 * kernels' calls get a region of the workspace per internal stream.  Results are complete once fcd_overlap_join(h) has
 * made the handle's stream wait for them (fcd_overlap_join_stream: any other hipStream_t), or after fcd_synchronize.
 * Every *_dev entry point of this handle that reads or writes arrays an overlapping call in flight writes (a search into
 * the same result arrays, fcd_result_offsets_dev / fcd_pack_results_dev / fcd_unpack_*_dev on its results) is ordered
 * behind that call by the library.  The caller's own kernels and copies that read such results need the join, and the
 * inputs of a call must stay untouched until it is joined.  n = 0 (default): every call is in stream order; changing n
 * joins what is in flight.  The internal streams are created in the high priority class, whose hardware queues the runtime hands out
 * separately from those of the process's normal streams. */
int fcd_set_overlap(fcd_handle *h, int streams);
int fcd_overlap_join(fcd_handle *h);
int fcd_overlap_join_stream(fcd_handle *h, void *hip_stream);
/* One call at a time: fcd_overlap_last_slot = the internal stream (0 .. n-1) the latest overlapping call went to, -1 if
 * none; fcd_overlap_join_slot makes `hip_stream` wait for what THAT internal stream has been given so far -- the call
 * itself as long as fewer than n further calls have been made since.  (A consumer that lags n - 1 calls behind -- a
 * gather of results on a communication stream -- waits for exactly the call it consumes.) */
int fcd_overlap_last_slot(fcd_handle *h);
int fcd_overlap_join_slot(fcd_handle *h, int slot, void *hip_stream);
const char *fcd_last_error(const fcd_handle *h);         /* text of the last failure on this handle */
const char *fcd_status_string(int status);               /* exact SearchError Display text, src/lib.rs:46-53 */
/* cap (bytes) on the per-call tree-arena workspace; batches needing more are decoded in chunks */
int fcd_set_workspace_limit(fcd_handle *h, int64_t bytes);
/* The handle's device workspace (tree arena, staging) only grows and is kept between calls; this waits for the
 * handle's stream and gives it all back (the next call allocates afresh).  For processes that share the GPU
 * with another allocator (PyTorch's caching allocator) after an unusually large job. */
int fcd_release_workspace(fcd_handle *h);
/* tie order of the beam searches' prune (FCD_TIE_*, above) */
int fcd_set_tie_order(fcd_handle *h, int order);         /* FCD_TIE_DEFAULT: follow the process default again */
int fcd_get_tie_order(const fcd_handle *h);              /* the order searches on this handle use right now */
int fcd_set_default_tie_order(int order);                /* FCD_TIE_PDQ178 or FCD_TIE_STABLE; process-wide */
/* (test hooks and developer instruments -- fcd_debug_*, the probes and sweeps -- are declared in fcd_debug.h: the
 * library exports them, but they are no part of the surface a binding generator should consume) */
/* duration (ms) of the decode kernel(s) of the last call on this handle, measured with HIP
 * events on the stream the kernels were launched on; <0 if unavailable */
double fcd_last_kernel_ms(fcd_handle *h);
/* Every search call brackets its kernel launches with a HIP event pair on the launch stream
 * (ring of 256).  fcd_timing_reset forgets them; fcd_timing_mean_ms synchronises on and averages
 * the pairs recorded since the reset (n_calls, nullable, receives how many). */
int fcd_timing_reset(fcd_handle *h);
double fcd_timing_mean_ms(fcd_handle *h, int64_t *n_calls);

/* ---- search::viterbi_search (src/search.rs:320-383) ---- */
int fcd_viterbi_search_dev(fcd_handle *h, const fcd_batch *in, int collapse_repeats,
                           const fcd_result *out);
int fcd_viterbi_search_host(fcd_handle *h, const fcd_batch *in, int collapse_repeats,
                            const fcd_result *out);

/* ---- search::beam_search (src/search.rs:159-301) ---- */
int fcd_beam_search_dev(fcd_handle *h, const fcd_batch *in, int64_t beam_size,
                        float beam_cut_threshold, int collapse_repeats, int kernel,
                        const fcd_result *out);
int fcd_beam_search_host(fcd_handle *h, const fcd_batch *in, int64_t beam_size,
                         float beam_cut_threshold, int collapse_repeats, int kernel,
                         const fcd_result *out);

/* ---- search::crf_beam_search (src/search.rs:38-157) ----
 * init: [n_reads * init_stride] f32, n_init entries used per read (src/search.rs:54-59). */
int fcd_crf_beam_search_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                            int64_t init_stride, int64_t beam_size, float beam_cut_threshold,
                            const fcd_result *out);
/* same as fcd_crf_beam_search_dev with an explicit FCD_KERNEL_* choice (tests / benchmarks) */
int fcd_crf_beam_search_dev_k(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                              int64_t init_stride, int64_t beam_size, float beam_cut_threshold,
                              int kernel, const fcd_result *out);
int fcd_crf_beam_search_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                             int64_t init_stride, int64_t beam_size, float beam_cut_threshold,
                             const fcd_result *out);
int fcd_crf_beam_search_host_k(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                               int64_t init_stride, int64_t beam_size, float beam_cut_threshold,
                               int kernel, const fcd_result *out);

/* ---- n best hypotheses of search::beam_search / search::crf_beam_search (src/search.rs:159-301, :38-157) ----
 * NOT a reference function: the reference returns beam[0] only (src/search.rs:165,300).  These run the same search
 * and, after the last row's truncation and division by the top probability (:278-282 / :125-131), trace back the
 * first n_hyp = min(n_best, beam length) entries of the final beam, in its rank order (the tie order in force,
 * FCD_TIE_*), each read off the suffix tree exactly as the reference reads beam[0] (:285-300 / :133-156).
 *   out   : n_reads * n_best rows of labels / path (nullable) / out_len; hypothesis i of read r is row r * n_best + i,
 *           and hypothesis 0 is, byte for byte, what fcd_beam_search_* / fcd_crf_beam_search_* return for the read.
 *           status and ambiguous (nullable) stay per read.  Rows i >= n_hyp[r] get out_len 0 and score 0.
 *   score : [n_reads * n_best] f32, entry i's label_prob + gap_prob (SearchPoint::probability(), src/search.rs:26-28):
 *           RELATIVE to the best entry of the last step (<= 1 up to rounding; hypothesis 0's need not be exactly 1),
 *           not a log-likelihood of the read.
 *   n_hyp : [n_reads] u32; 0 for a read whose search fails (its status says why).
 * Hypotheses are distinct labellings (the search merges by tree node).  Everything listed is written by the call:
 * uninitialised arrays are fine.  n_best outside 1 .. beam_size is FCD_E_INVALID.  The _dev forms share the kernel
 * choice, workspace chunking, wide-beam retry pass and fcd_set_overlap behaviour of fcd_beam_search_dev; the _host
 * forms stage the batch, decode and copy back in one piece (not through the chunk pipeline of the host jobs). */
typedef struct fcd_nbest {
    int64_t n_best;     /* 1 .. beam_size */
    float *score;       /* [n_reads * n_best] */
    uint32_t *n_hyp;    /* [n_reads] */
} fcd_nbest;
int fcd_beam_search_nbest_dev(fcd_handle *h, const fcd_batch *in, int64_t beam_size, float beam_cut_threshold,
                              int collapse_repeats, int kernel, const fcd_nbest *nb, const fcd_result *out);
int fcd_beam_search_nbest_host(fcd_handle *h, const fcd_batch *in, int64_t beam_size, float beam_cut_threshold,
                               int collapse_repeats, int kernel, const fcd_nbest *nb, const fcd_result *out);
int fcd_crf_beam_search_nbest_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                                  int64_t init_stride, int64_t beam_size, float beam_cut_threshold, int kernel,
                                  const fcd_nbest *nb, const fcd_result *out);
int fcd_crf_beam_search_nbest_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                                   int64_t init_stride, int64_t beam_size, float beam_cut_threshold, int kernel,
                                   const fcd_nbest *nb, const fcd_result *out);

/* ---- beam-search sessions: search::beam_search / search::crf_beam_search on rows as they arrive ----
 * (src/search.rs:159-301, :38-157.)  Both searches are causal: step t reads row t, the beam and the prefix tree, nothing
 * else.  A session is a fixed set of n_reads read SLOTS with a fixed search shape (N, S, beam_size, beam_cut_threshold,
 * collapse_repeats, max_steps = the most rows a slot takes between restarts; the tie order in force on the handle and the
 * kernel are frozen at create).  Each slot's search advances over the rows pushed to it and can be read back at any time.
 *   push   : chunk->n_reads == n_reads, T_c rows; slot r takes the first lengths[r] rows (all T_c if lengths is NULL, 0
 *            leaves it untouched).  chunk->lengths is a HOST pointer here (the one exception to the _dev convention: the
 *            session keeps a host-side step count per slot, and stages the lengths to the device in stream order from a
 *            page-locked buffer it does not reuse before the copy has completed).  Any strides and f32 / f16 / bf16,
 *            which may change from push to push.  A push that would take a slot past max_steps is FCD_E_INVALID before
 *            anything is enqueued, the session unchanged.  out (nullable): the result after the push, from the same launch.
 *   result : for every slot, exactly what fcd_beam_search_dev / fcd_crf_beam_search_dev return for the slot's PREFIX (all
 *            rows pushed since create or its restart, concatenated): labels, path (row indices into the prefix), out_len,
 *            status and -- count_ambiguous sessions only, out->ambiguous given -- the two tie counters over the prefix.
 *            out_stride >= max_steps.  Before the first push: a read of length 0.  The session does not change.
 *   A slot that fails (FCD_ST_INCOMPARABLE, FCD_ST_RAN_OUT_OF_BEAM, CRF FCD_ST_BAD_STATE -- a bad init row at its first
 *   non-empty push) stays failed: later pushes leave it alone, as the one-shot search fails every longer prefix.
 *   restart: slots[0 .. n) (host) go back to the root with 0 steps; CRF: init (host) holds n rows of n_init, row j for
 *            slots[j].  create: init (host) holds n_reads rows of n_init.
 * Kernel: FCD_KERNEL_AUTO takes the wave kernel where it holds the shape and (max_steps << id shift) + 16 < 2^25, else the
 * LDS-resident kernel; WAVE / WAVE1 / GENERIC force one; FCD_KERNEL_LANE is FCD_E_UNSUPPORTED (wide beams run on the
 * generic kernel).  Memory: ONE device allocation made at create (FCD_E_NOMEM if it fails), outside the handle's workspace
 * and its limit; fcd_beam_session_bytes says how large.  Per slot: wave kernel 2080 B of state + cap * (8 + 4 * row
 * words) B of tree, cap = (max_steps << s) + 8 rounded up to 4, s = 5 at beam <= 5 and N <= 5 (WAVE1: 6) else 6, row
 * words 4 (N <= 5) or 8; generic kernel (32 + 4 * beam_size * (N + 6)) B of state + (max_steps * beam_size * (N-1) + 8) *
 * (16 + 4 * (N-1)) B of tree; plus 16 B (lengths, slot list) and, CRF, 4 * n_init B.
 * Ordering: every enqueuing call runs on the handle's current stream (never on the fcd_set_overlap internal streams: a
 * session's pushes stay in order), behind overlapping calls in flight that write arrays it reads or writes.  The
 * session's state and staged lengths are ordered by that stream alone: a caller that changes the handle's stream between
 * two session calls must order the two streams itself.  fcd_destroy
 * is FCD_E_INVALID while the handle has live sessions.  The _host forms take host posteriors / results and return when
 * the results are in place.  Not covered: the lane kernel, n-best results, viterbi / greedy and the duplex searches. */
typedef struct fcd_beam_session fcd_beam_session;
int fcd_beam_session_create(fcd_handle *h, int64_t n_reads, int64_t N, int64_t max_steps, int64_t beam_size,
                            float beam_cut_threshold, int collapse_repeats, int kernel, int count_ambiguous,
                            fcd_beam_session **out);
int fcd_crf_beam_session_create(fcd_handle *h, int64_t n_reads, int64_t S, int64_t N, const float *init, int64_t n_init,
                                int64_t max_steps, int64_t beam_size, float beam_cut_threshold, int kernel,
                                int count_ambiguous, fcd_beam_session **out);
int fcd_beam_session_push_dev(fcd_beam_session *s, const fcd_batch *chunk, const fcd_result *out);
int fcd_beam_session_push_host(fcd_beam_session *s, const fcd_batch *chunk, const fcd_result *out);
int fcd_beam_session_result_dev(fcd_beam_session *s, const fcd_result *out);
int fcd_beam_session_result_host(fcd_beam_session *s, const fcd_result *out);
int fcd_beam_session_restart(fcd_beam_session *s, const int64_t *slots, int64_t n, const float *init);
int fcd_beam_session_steps(const fcd_beam_session *s, int64_t *steps);  /* [n_reads] rows taken since create / restart */
int64_t fcd_beam_session_bytes(const fcd_beam_session *s);
int fcd_beam_session_destroy(fcd_beam_session *s);

/* ---- CTC forward log-likelihood of given labellings (csrc/ctc_score.hip) ----
 * NOT a reference function.  logp[r * n_hyp + i] = ln P(y | x) = ln of the sum, over every alignment of labelling y
 * (hypothesis i of read r) to the T_r rows of the read, of the product of the posteriors along it: the unpruned, unmerged
 * sum of the recurrences search::beam_search walks (src/search.rs:186-241), float64, comparable between reads.
 * Extended sequence z of 2L + 1 states, z[2k] = blank, z[2k+1] = y[k]; rows converted to f32 exactly as the searches do:
 *   start   alpha_0[0] = p[0][0], alpha_0[1] = p[0][y_0], else 0
 *   blank   alpha_t[s] = (alpha_{t-1}[s] + alpha_{t-1}[s-1]) * p[t][0]
 *   label   collapse_repeats = 1: (alpha_{t-1}[s] + alpha_{t-1}[s-1] + [s >= 3, z[s] != z[s-2]] alpha_{t-1}[s-2]) * p[t][z[s]]
 *           collapse_repeats = 0: (alpha_{t-1}[s-1] + [s >= 3] alpha_{t-1}[s-2]) * p[t][z[s]]  (every non-blank row emits)
 *   result  ln(alpha_{T_r-1}[2L] + alpha_{T_r-1}[2L-1])
 * L = 0: ln prod p[t][0].  T_r = 0: 0.0 for L = 0, else -inf.  P = 0 (L > T_r, ...): -inf.  A label outside 1 .. N-1 (or
 * len > stride): NaN.  A NaN posterior in a cell that contributes: NaN.  Rows i >= n_valid[r]: not scored, NaN.
 * band = 0: the exact lattice.  band = W >= 1: with k(t) = #{k : path[k] <= t} (path ascending, as the searches return it),
 * only the states max(0, 2 (k(t) - W) - 2) <= s <= min(2L, 2 (k(t) + W)) are live at row t, every other state counts as 0
 * there: the sum over the alignments that stay inside the window, a lower bound that rises with W.
 * Numerics: alpha in f32 probability space, rescaled by exact powers of two every row with an integer exponent total,
 * ln(m) + E ln 2 formed in float64, no logarithm per step; |error| <= about 3 T_r 2^-24 nats.  A cell below 2^-246 of its
 * row's largest live cell may be dropped (the result is then a lower bound).  Posteriors outside [0, 1], infinities and
 * negative values give some value, nothing more.
 * in->S must be 1 (CRF models are scored on transitions: out of scope); in->lengths as everywhere (device / host pointer).
 * Limits (FCD_E_UNSUPPORTED): the widest possible window, min(4 band + 3, 2 min(T, stride) + 1) states, lives in
 * registers up to 510 states and double-buffered in LDS (160 KiB) beyond: about 18000 states, i.e. exact scoring of
 * labellings up to ~9000 labels -- use a band beyond that.
 * _dev: device pointers, enqueued on the handle's stream in stream order, behind overlapping searches in flight
 * (fcd_set_overlap) that still write the arrays it reads.  _host: host pointers; stages, runs and copies back in one piece.
 * FCD_E_INVALID before anything is enqueued: band < 0, band > 0 without path, n_hyp < 1, S != 1. */
typedef struct fcd_labellings {
    const uint8_t  *labels;   /* [n_reads * n_hyp * stride], row r * n_hyp + i: fcd_result.labels as the searches write it */
    const uint32_t *len;      /* [n_reads * n_hyp]: fcd_result.out_len */
    const uint32_t *n_valid;  /* [n_reads], nullable (fcd_nbest.n_hyp): rows i >= n_valid[r] are not scored, logp = NaN */
    const uint32_t *path;     /* same shape as labels; required when band > 0, else nullable */
    int64_t n_hyp;            /* rows per read: 1 for a plain result, n_best for an n-best one */
    int64_t stride;           /* out_stride */
} fcd_labellings;
int fcd_ctc_score_dev(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                      double *logp);
int fcd_ctc_score_host(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                       double *logp);

/* ---- CTC forced alignment of given labellings (csrc/ctc_align.hip) ----
 * NOT a reference function.  The BEST single alignment through the lattice fcd_ctc_score_* sums over -- same extended
 * sequence z, same transitions under collapse_repeats, same live window under `band`: the state sequence s_0 .. s_{T_r-1}
 * (s_0 in {0, 1}, s_t - s_{t-1} in {0, 1, 2}, 2 only where the score's s-2 term enters, 0 never on a label when
 * collapse_repeats = 0) that maximises prod_t p[t][z[s_t]] and ends in state 2L or 2L - 1.  It gives every label its rows,
 * and from them a quality defined as search::viterbi_search defines its own (src/search.rs:337-376): a beam result plus
 * this call is a FASTQ record.  Aligning viterbi_search's own labelling returns its path and its qualities bit for bit.
 * Arithmetic: f32 with an unbounded exponent; a cell is max(candidates) * p, ONE f32 rounding; rows are rescaled by powers
 * of two only (exact); a cell below 2^-160 of its row's maximum may be dropped.
 * Ties: candidates are taken in the order stay (s), s-1, s-2, and a later one replaces an earlier one only if it is
 * strictly greater; at the end state 2L is taken unless 2L - 1 is strictly greater.
 * Per labelling row (row = r * n_hyp + i), label k < len:
 *   start[row * stride + k]  the first row spent in state 2k + 1
 *   count[row * stride + k]  the rows spent in it (consecutive; exactly 1 when collapse_repeats = 0)
 *   qual [row * stride + k]  (p[start][y_k] + ... + p[start + count - 1][y_k]) / (float)count, summed in f32 in ascending row
 *                            order, no fused multiply-add: viterbi_search's label_prob_total / label_prob_count.  Nullable.
 *   logp [row]               ln of the alignment's probability, ln(m) + E ln 2 in float64.  Nullable.
 * Rows without an alignment, tested in this order: i >= n_valid[r], len > stride, a label outside 1 .. N-1: logp = NaN;
 * T_r = 0 < L or L > T_r: logp = -inf; a NaN, infinite or negative posterior ANYWHERE in the read's first T_r rows (found
 * while the rows are staged; a comparison-based search has no sensible order for them): logp = NaN; no alignment inside
 * the window or repeats that need more rows than there are: logp = -inf.  In all of them count = 0 for every
 * k < min(len, stride) and start / qual are left alone.  L = 0: logp = sum_t ln p[t][0], nothing else is written.
 * Entries k >= len are never written by _dev; _host returns them as 0.
 * band: as fcd_ctc_score_*; the best alignment among those that stay inside the window, so logp rises with W.
 * Shapes, limits, in->S, in->lengths, stream order and the FCD_E_INVALID / FCD_E_UNSUPPORTED cases are fcd_ctc_score_*'s;
 * start and count must not be null.  _dev is enqueue-only on the handle's stream, behind every overlapping search in
 * flight (fcd_set_overlap).  Its back-pointers (2 bits per row and slot for windows up to 510 states: 64 or 128 bytes a
 * row; a byte per row and state beyond) live in the handle's workspace: the labellings are launched in groups of whole
 * reads that fit 4 GiB of it, one after the other on the stream, no host wait in between. */
typedef struct fcd_alignment {
    uint32_t *start;  /* [n_reads * n_hyp * stride] */
    uint32_t *count;  /* [n_reads * n_hyp * stride] */
    float    *qual;   /* [n_reads * n_hyp * stride], nullable */
    double   *logp;   /* [n_reads * n_hyp], nullable */
} fcd_alignment;
int fcd_ctc_align_dev(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                      const fcd_alignment *out);
int fcd_ctc_align_host(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                       const fcd_alignment *out);

/* ---- CTC forward-backward substitution posteriors of given labellings (csrc/ctc_posterior.hip) ----
 * NOT a reference function.  For a labelling y of L labels (hypothesis i of read r, row = r * n_hyp + i), label position
 * k < L and label c in 1 .. N-1, let y[k:=c] be y with label k replaced by c.  With P as fcd_ctc_score_* defines it -- same
 * extended sequence, same transitions under collapse_repeats, and under `band` the live window derived from y's OWN path
 * for every variant --
 *   sub[k][c]  = P(y[k:=c] | x)
 *   post[k][c] = sub[k][c] / sum_{c' = 1 .. N-1} sub[k][c']      float32, entry ((row * stride + k) * (N-1) + c-1)
 *   conf[k]    = post[k][y_k]
 * post[k][.] is the posterior over what label stands at position k with the rest of the labelling held fixed, conf[k] the
 * called label's share of it, 1 - conf[k] a substitution error probability: the number a FASTQ quality, a variant caller
 * or a polisher wants, which fcd_ctc_align_*'s qual (the network's sharpness along ONE alignment) is not.  Deletions and
 * insertions are fcd_ctc_edits_*'s (below).
 * Computed without rescoring any variant, from one forward and one backward walk.  alpha: fcd_ctc_score_*'s forward values.
 * beta, on the same lattice and window: beta_{T_r-1}[2L] = beta_{T_r-1}[2L-1] = 1; beta_t[q] = sum over the successors s of
 * q that are live at row t+1 of p[t+1][z[s]] * beta_{t+1}[s].  For s = 2k + 1, over the rows t at which s is live:
 *   exit_t(c)  = [k = L-1 and t = T_r-1] + p[t+1][0] * beta_{t+1}[s+1]
 *              + [s+2 <= 2L and (no collapse or c != y_{k+1})] * p[t+1][y_{k+1}] * beta_{t+1}[s+2]
 *              + [collapse] * w_{t+1}(c)                                 (the stay; w = 0 where s is not live)
 *   w_t(c)     = p[t][c] * exit_t(c)
 *   entry_t(c) = t = 0: [k = 0];  else alpha_{t-1}[s-1] + [s >= 3 and (no collapse or c != y_{k-1})] * alpha_{t-1}[s-2]
 *   sub[k][c]  = sum_t entry_t(c) * w_t(c)                              (c = y_k gives P(y | x) for every k)
 * Numerics: f32 probability space; rows rescaled by exact powers of two with integer exponents (one per forward row, one
 * per backward row, one for the accumulators); every term non-negative, one rounding per product and per sum, no fused
 * multiply-add.  |post - exact| <= about 12 T_r 2^-24 * post.  A cell below 2^-160 of its row's maximum may be dropped.
 * logp (nullable): ln P(y | x), fcd_ctc_score_*'s value (the same forward recurrence).
 * Rows without a value: logp follows fcd_ctc_score_*'s rules for that row (NaN, -inf, 0.0); whenever P(y | x) is not a
 * positive finite number every post entry for k < min(len, stride) is NaN.  A position whose sum over c is 0 or NaN: NaN.
 * Entries k >= len are never written by _dev; _host returns them as 0.  L = 0 writes logp only.
 * Shapes, dtypes, strides, in->S = 1, in->lengths, n_valid, stream order and the FCD_E_INVALID cases are
 * fcd_ctc_score_*'s; a null out or out->post is one more.
 * Limits (FCD_E_UNSUPPORTED): register-resident windows only -- the widest possible window, min(4 band + 3,
 * 2 min(T, stride) + 1) states, must not exceed 510 (bands up to 126; exact mode up to min(T, stride) = 254: "use a band"
 * beyond) -- N - 1 <= 8 labels, and min(T, stride) <= 28480 (the labelling's copy shares 64 KiB of LDS with the tile).
 * _dev is enqueue-only on the handle's stream, behind every overlapping search in flight (fcd_set_overlap).  The forward
 * rows (4 bytes per slot, 128 / 256 / 384 / 512 slots a row for windows up to 126 / 254 / 382 / 510 states, plus an exponent
 * word; only the live cells are written) live in the handle's workspace: the labellings are launched in groups of whole
 * reads that fit 4 GiB of it (or fcd_set_workspace_limit), one after the other on the stream, no host wait in between. */
typedef struct fcd_posterior {
    float  *post;   /* [n_reads * n_hyp * stride * (N-1)], entry ((row * stride + k) * (N-1) + c-1) */
    double *logp;   /* [n_reads * n_hyp], nullable: ln P(y | x), fcd_ctc_score's value within its tolerance */
} fcd_posterior;
int fcd_ctc_posterior_dev(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                          const fcd_posterior *out);
int fcd_ctc_posterior_host(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                           const fcd_posterior *out);

/* ---- CTC deletion and insertion likelihoods of given labellings (csrc/ctc_posterior.hip) ----
 * NOT a reference function.  What fcd_ctc_posterior_* leaves out: with its substitutions, the full edit-distance-1
 * neighbourhood of a labelling, from one forward and one backward walk instead of L + (L+1)(N-1) rescorings.
 * y is a labelling of L labels (hypothesis i of read r, row = r * n_hyp + i), z its 2L + 1 extended states, alpha
 * fcd_ctc_score_*'s forward value, b_t[s] = p[t][z[s]] * beta_t[s] the backward value of fcd_ctc_posterior_* ("row T_r":
 * all of b on state 2L; b is 0 above state 2L); "collapse" stands for collapse_repeats = 1.
 * Deletion of label k, 0 <= k < L -- the carrying state is s = 2k + 1:
 *   entry_t  = t = 0: [k = 0];  else alpha_{t-1}[2k] + [k >= 1 and (no collapse or y_{k-1} != y_{k+1})] alpha_{t-1}[2k-1]
 *   D[k]     = sum_t entry_t * b_t[2k+3]                                 for k < L-1
 *   D[L-1]   = alpha_{T_r-1}[2L-2] + [L >= 2] alpha_{T_r-1}[2L-3]         (the shortened labelling's two final states)
 * Insertion of label c into gap g, 0 <= g <= L (before y_g; after the last label for g = L) -- the carrying state is the
 * blank s = 2g, and the blank that follows the inserted label behaves exactly as y's state 2g does:
 *   u_t(c)     = p[t][c] * ([collapse] u_{t+1}(c) + b_{t+1}[2g] + [g < L and (no collapse or c != y_g)] b_{t+1}[2g+1])
 *   entry_t(c) = t = 0: [g = 0];  else alpha_{t-1}[2g] + [g >= 1 and (no collapse or c != y_{g-1})] alpha_{t-1}[2g-1]
 *   I[g][c]    = sum_t entry_t(c) * u_t(c)
 * band = 0: D[k] = P(y without label k | x) and I[g][c] = P(y with c inserted at g | x), as fcd_ctc_score_* defines P.
 * band = W: alpha and b are y's own values on y's own window (fcd_ctc_score_*'s, from y's path); a state outside its row's
 * window counts 0; the sums run over the rows at which the carrying state is live (D[L-1]: 0 unless state 2L-1 is live at
 * row T_r-1); u is 0 where the carrying state is not live.  A lower bound that rises with W and equals the exact value once
 * the window holds the whole lattice.
 * Outputs, float32 log-ratios against the labelling itself -- a positive entry is an edit that explains the read better:
 *   deletion [row * stride + k]                     = ln D[k]    - ln P(y | x)
 *   insertion[(row * (stride+1) + g) * (N-1) + c-1] = ln I[g][c] - ln P(y | x)
 *   logp[row] (nullable, float64)                   = ln P(y | x), fcd_ctc_score_*'s value
 * Rows without a value: logp follows fcd_ctc_score_*'s rules; whenever P(y | x) is not a positive finite number every
 * entry for k < min(len, stride) and g <= min(len, stride) is NaN.  A variant of probability 0 (L + 1 > T_r, repeats that
 * need more rows than there are, ...): -inf.  A NaN posterior in a cell that only the variant reads: NaN -- in that
 * variant's entry alone: a cell no alignment of y passes through (row 0 of y's second label, the last row of its last but
 * one, ...) leaves logp and every entry whose variant has no alignment through it as they are.  L = 0 is a real
 * case: gap 0 is written (I[0][c] = P([c] | x)), nothing goes to deletion.  Entries beyond the labelling are never written
 * by _dev; _host returns them as 0.
 * Numerics: fcd_ctc_posterior_*'s -- f32 probability space, exact power-of-two rescaling with integer exponents, every
 * term non-negative, one rounding per product and per sum, no fused multiply-add; the log-ratio is formed in float64 from
 * the accumulator's mantissa and its integer exponent.  |error| <= about 12 T_r 2^-24 + 2^-23 |value| nats.  A cell below
 * 2^-160 of its row's maximum may be dropped: an entry below -100 ln 2 is a lower bound and may come back as -inf.
 * Limits, shapes, dtypes, in->S = 1, in->lengths, n_valid, stream order, the grouping by workspace size and the
 * FCD_E_INVALID / FCD_E_UNSUPPORTED cases are fcd_ctc_posterior_*'s (windows up to 510 states, N - 1 <= 8, min(T, stride)
 * <= 28480; the messages name ctc_edits and the way out: "use a band"); a null out, out->deletion or out->insertion is one
 * more FCD_E_INVALID. */
typedef struct fcd_edits {
    float  *deletion;   /* [n_reads * n_hyp * stride] */
    float  *insertion;  /* [n_reads * n_hyp * (stride+1) * (N-1)], entry ((row * (stride+1) + g) * (N-1) + c-1) */
    double *logp;       /* [n_reads * n_hyp], nullable: ln P(y | x), fcd_ctc_score's value within its tolerance */
} fcd_edits;
int fcd_ctc_edits_dev(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                      const fcd_edits *out);
int fcd_ctc_edits_host(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                       const fcd_edits *out);

/* ---- CRF scoring and forced alignment of given labellings (csrc/crf_lattice.hip) ----
 * NOT reference functions.  The lattice of a GIVEN labelling under a CRF model -- the recurrence search::crf_beam_search
 * walks (src/search.rs:62-100), unpruned and unmerged, for one labelling -- walked forward as a sum (score) and as a max with
 * traceback (align).  Batch (n_reads, T, S, N) as fcd_batch describes it: any strides, f32 / f16 / bf16 (converted to f32
 * exactly), ragged lengths.  init: [n_reads * init_stride] f32, n_init entries used per read, as fcd_crf_beam_search_*.
 * A labelling y of L labels in 1 .. N-1; nb = N - 1.
 * State trajectory: sigma_0 = the index of the FIRST maximum of the read's init row (src/search.rs:58,404; a NaN counts
 *   as -inf); sigma_{k+1} = (sigma_k * nb) mod S + (y_k - 1) (:97,414).  It depends on init and y only.
 * Reading rule: P(t, k, j) = p[t][sigma_k][j]; where sigma_k lies outside 0 .. S-1 (S = 5, N = 4 gets there) P reads as 0
 *   and nothing is read out of bounds: such a state is a dead end, except as the final state entered at the last row.
 * Lattice: states k = 0 .. L, the labels emitted so far; no repeat-collapsing (a CRF has none).
 *   alpha_{-1}[0] = 1;  alpha_t[k] = alpha_{t-1}[k] * P(t,k,0) + alpha_{t-1}[k-1] * P(t,k-1,y_{k-1})
 *   crf_score = ln alpha_{T_r-1}[L], float64.  The init probabilities do not enter: the search's start value
 *   max(init) + init[0] is a common factor of all hypotheses of a read.
 * Alignment: the strictly increasing emission rows e_0 < ... < e_{L-1} that maximise the product (max where the score has
 *   +).  Label k: start[k] = e_k, count[k] = 1, qual[k] = P(e_k, k, y_k) -- what crf_greedy_search feeds to phred (:412-413);
 *   logp = ln of the product, float64.  Ties: the stay candidate is kept unless the advance candidate is strictly greater.
 * Arithmetic: f32 with an unbounded exponent, rows rescaled by exact powers of two; each of the two candidates of a cell is
 *   ONE product with one rounding, the score's sum a third; no fused multiply-add; ln(m) + E ln 2 in float64.  |error| of
 *   the score <= about 3 T_r 2^-24 nats.  A cell below 2^-160 of its row's maximum may be dropped.
 * band = 0: the whole lattice.  band = W >= 1 (needs y->path, ascending): with k(t) = #{k : path[k] <= t}, only the states
 *   max(0, k(t) - W) <= k <= min(L, k(t) + W) are live at row t; the window is also cut to what can be reached (k <= t + 1)
 *   and can still reach the end (k >= L - (T_r - 1 - t)), which changes no result.  Score: a lower bound that rises with W;
 *   align: the best alignment inside the window.
 * Rows without a value, tested in this order: i >= n_valid[r], len > stride, a label outside 1 .. N-1: NaN; T_r = 0: 0.0 for
 *   L = 0, else -inf; L > T_r: -inf; score: a NaN in a contributing cell: NaN; align: a NaN, infinite or negative value among
 *   the values that enter a live cell (P(t,k,0) into cell k, P(t,k,y_k) into cell k + 1, both cells live at row t): NaN --
 *   not "anywhere in the read" as fcd_ctc_align_*: scanning S * N values a row would defeat the gather; no alignment: -inf.
 *   In all align cases without an alignment count = 0 is written for k < min(len, stride), start / qual are left alone.
 *   L = 0: logp = sum_t ln P(t,0,0), nothing else is written.  Entries k >= len: never written by _dev, 0 from _host.
 * Limits (FCD_E_UNSUPPORTED): the widest possible window, min(2 band + 1, min(T, stride) + 1) states, lives in registers:
 *   up to 512 states ("use a band" beyond: exact alignment up to 511 labels); S < 2^24 - 1; min(T, stride) <= 15263 (the
 *   labelling and its trajectory live in 64 KiB of LDS).  S = 1024 and 4096 are ordinary shapes: rows of more than 1024
 *   values are gathered from global memory instead of being staged.
 * FCD_E_INVALID before anything is enqueued or written: band < 0, band > 0 without path, n_hyp < 1, S < 1, null init or
 *   n_init < 1, null start / count, null out / logp.
 * _dev: device pointers, enqueue-only on the handle's stream (never on the fcd_set_overlap internal streams), behind
 *   overlapping searches in flight that still write the arrays it reads.  Align keeps one back-pointer bit per row and
 *   slot (8, 16, 32 or 64 bytes a row) in the handle's workspace and launches groups of whole reads that fit 4 GiB of it.
 * _host: host pointers; stages, runs and copies back in one piece. */
int fcd_crf_score_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                      const fcd_labellings *y, int64_t band, double *logp);
int fcd_crf_score_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                       const fcd_labellings *y, int64_t band, double *logp);
int fcd_crf_align_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                      const fcd_labellings *y, int64_t band, const fcd_alignment *out);
int fcd_crf_align_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                       const fcd_labellings *y, int64_t band, const fcd_alignment *out);

/* ---- CRF forward-backward substitution posteriors of given labellings (csrc/crf_posterior.hip) ----
 * NOT a reference function.  Everything is as fcd_crf_score_* defines it: batch (n_reads, T, S, N), init, nb = N - 1, the
 * trajectory sigma_0 = first maximum of the init row, sigma_{k+1} = (sigma_k * nb) mod S + (y_k - 1), the reading rule
 * P(t, k, j) = p[t][sigma_k][j], the lattice k = 0 .. L, under band = W the window from y->path.
 * For hypothesis i of read r (row = r * n_hyp + i), position k < L and label c in 1 .. N-1, y[k:=c] is y with label k
 * replaced by c:
 *   sub[k][c]  = exp(crf_score(y[k:=c])) -- the variant has ITS OWN trajectory, the same init row, and under a band the
 *                window derived from y's own path (windows are in label counts: a variant's window is the same set of cells)
 *   post[k][c] = sub[k][c] / sum_{c' = 1 .. N-1} sub[k][c']      float32, entry ((row * stride + k) * (N-1) + c-1)
 *   conf[k]    = post[k][y_k]
 *   logp       = ln P(y | x), fcd_crf_score_*'s value within its tolerance; float64, nullable
 * What fcd_crf_align_*'s qual is not: how much better the called label explains the read than another label would, with all
 * alignments counted.
 * Shapes: S = nb^m with nb >= 2 and m >= 1, or S = 1.  The model state is then the last m labels as base-nb digits, no sigma
 * ever leaves 0 .. S-1 after state 0, and the variant's trajectory is closed-form:
 *   sigma'_{k+j} = sigma_{k+j} + (c - y_k) * nb^(j-1) for j = 1 .. m; it rejoins y's trajectory at state k + m + 1.
 * S = 1 walks as m = 1: the trajectory rule gives sigma_{k+1} = y_k - 1 there -- the table's one row after label 1, outside
 * the table (a dead end, as fcd_crf_score_* has it) after any other label, for y and for its variants alike.
 * Computed without rescoring any variant.  Pass 1: fcd_crf_score_*'s forward recurrence, every row's cells stored.  Pass 2
 * walks the rows backwards: beta_{T_r-1}[L] = 1, beta_t[k] = P(t+1,k,0) beta_{t+1}[k] + P(t+1,k,y_k) beta_{t+1}[k+1], and per
 * state s the chain values V_s[j][c], j = 1 .. min(m, s) -- the backward value state s has in the variant that substituted c
 * at position s - j:
 *   V_s[j][c]_t = P'(t+1,s,0) V_s[j][c]_{t+1} + P'(t+1,s,y_s) V_{s+1}[j+1][c]_{t+1},  P' read from row
 *   sigma_s + (c - y_{s-j}) nb^(j-1),  V_{s+1}[m+1][c] = beta[s+1];  at the last row the value is [s = L].
 *   sub[k][c] = sum_t alpha_{t-1}[k] * P(t,k,c) * V_{k+1}[1][c]_t                 (c = y_k gives P(y | x) for every k)
 * A chain that would pass state L ends there.
 * Numerics: fcd_crf_score_*'s and fcd_ctc_posterior_*'s -- f32 probability space, exact power-of-two rescaling with integer
 * exponents (one per forward row; one per backward row shared by beta and every V; one per position for its accumulators,
 * counted from floor(log2 P(y | x)): it starts at 0, where the called label's sum is about 1, and rises with the largest
 * term, so a variant may outweigh y by any factor -- y's share is then the 0 it rounds to), every term non-negative, one
 * rounding per product and per sum, no fused multiply-add.  A cell below 2^-160 of its row's maximum may be dropped.  Error bound, by roundings along the longest chain: alpha_{t-1} carries 3 t (two products and a sum a row), V_t
 * 3 (T_r - 1 - t), a term two products, the sum over the rows at most T_r -- a sub[k][c] is within (4 T_r - 1) 2^-24 of its
 * value, relative; the ratio doubles that and adds the N - 2 sums of the denominator and the division:
 *   |post - exact| <= (8 T_r + 6) 2^-24 * post.
 * Rows without a value: logp follows fcd_crf_score_*'s order and values (i >= n_valid[r], len > stride, a bad label,
 * T_r = 0, L > T_r, a NaN in a contributing cell).  Whenever P(y | x) is not a positive finite number every post entry for
 * k < min(len, stride) is NaN.  A position whose sum over c is 0 or NaN is NaN; a NaN posterior that only a variant reads
 * makes that position NaN and leaves logp alone.  Entries k >= len are never written by _dev and are 0 from _host.  L = 0
 * writes logp only.
 * FCD_E_INVALID: fcd_crf_score_*'s cases, and a null out or out->post.
 * Limits (FCD_E_UNSUPPORTED; the message says which): fcd_crf_score_*'s, and
 *   S that is no power of N - 1 (S = 5, N = 4);  N - 1 > 8;
 *   the kernels are instantiated on (states per lane, m, nb) tiers -- a held state costs m nb registers --
 *     m <= 2 and nb <= 4,  m <= 4 and nb <= 2   (m nb <= 8):    windows up to 512 states (1, 2, 4, 8 states per lane)
 *     m <= 1 and 5 <= nb <= 8                   (m nb <= 8):    windows up to 256 states (band <= 127; 1, 2, 4 per lane:
 *                                                               eight states of eight labels do not fit 256 VGPRs)
 *     m <= 3 and nb <= 8,  m <= 6 and nb <= 4   (m nb <= 24):   windows up to 192 states (band <= 95; 1, 2, 3 per lane)
 *   (S = 4, 16 at N = 5: the first row; S = 64, 1024, 4096 at N = 5: the third.)  Any other (m, nb) is unsupported, a wider
 *   window too, with the band that fits in the message.
 * _dev: device pointers, enqueue-only on the handle's stream, behind overlapping searches in flight that still write the
 * arrays it reads.  The forward rows (4 bytes per slot, 64 / 128 / 256 / 512 slots a row for windows up to that many
 * states -- 64 / 128 / 192 in the last row of the table -- plus an exponent word) live in the handle's workspace: the
 * labellings are launched in groups of whole reads that fit 4 GiB of it (or fcd_set_workspace_limit), forward then backward
 * per group, one after the other on the stream, no host wait in between.
 * _host: host pointers; stages, runs and copies back in one piece. */
int fcd_crf_posterior_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                          const fcd_labellings *y, int64_t band, const fcd_posterior *out);
int fcd_crf_posterior_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                           const fcd_labellings *y, int64_t band, const fcd_posterior *out);

/* ---- CRF deletion and insertion likelihoods of given labellings (csrc/crf_posterior.hip) ----
 * NOT a reference function.  What fcd_crf_posterior_* leaves out: with its substitutions, the full edit-distance-1
 * neighbourhood of a labelling under a CRF model, from one forward and two backward walks instead of L + (L+1)(N-1)
 * rescorings.  Everything is as fcd_crf_posterior_* has it: batch, init, nb = N - 1, S = nb^m or S = 1 (walked as m = 1),
 * y's trajectory sigma_k, the reading rule P(u, sigma, j) = p[u][sigma][j] (0 for sigma outside 0 .. S-1), alpha and beta.
 * A variant labelling walks ITS OWN trajectory: the rule sigma'_{k+1} = (sigma'_k nb) mod S + (y'_k - 1) from the same
 * sigma_0.  It differs from y's only while the edit is inside the m-label history; the closed forms below are what the
 * kernel reads, the rule is the definition (tests/crf_edits_reference.py pins both to the enumeration of every alignment).
 * Deletion of label k, 0 <= k < L (y' = y without y_k).  y' has y's states 0 .. k; its state k emits y_{k+1} from row
 * sigma_k; its state k+1+j lives in y's slot s = k+2+j, j = 0 .. m-2, with
 *   sigma' = (sigma_k nb^(j+1)) mod S + (sigma_s mod nb^(j+1)),   and rejoins y's trajectory at slot k+m+1:
 *   W_s[j]_{u-1} = P(u,sigma',0) W_s[j]_u + P(u,sigma',y_s) W_{s+1}[j+1]_u,   W_{s+1}[m-1] = beta[s+1];  last row: [s = L]
 *   D[k]   = sum_u alpha_{u-1}[k] * P(u,sigma_k,y_{k+1}) * X_u[k+2]   for k < L-1,   X = W[0] (m = 1: X = beta)
 *   D[L-1] = alpha_{T_r-1}[L-1]
 * Insertion of label c before y_g, 0 <= g <= L (g = L: after the last label).  y' state g emits c from row sigma_g; its
 * state g+1+j lives in y's slot s = g+j, j = 0 .. m-1, with
 *   sigma' = (sigma_g nb^(j+1)) mod S + (c-1) nb^j + (sigma_s mod nb^j),   and rejoins at slot g+m:
 *   U_s[j][c]_{u-1} = P(u,sigma',0) U_s[j][c]_u + P(u,sigma',y_s) U_{s+1}[j+1][c]_u,   U_{s+1}[m][c] = beta[s+1];
 *   last row: [s = L];  a chain that would pass state L ends there
 *   I[g][c] = sum_u alpha_{u-1}[g] * P(u,sigma_g,c) * U_g[0][c]_u            ("row -1" is state 0 holding 1)
 * band = 0: D[k] = exp(crf_score(y without label k)) and I[g][c] = exp(crf_score(y with c at g)), exactly.  y's own cone
 * (k <= t + 1, k >= L - (T_r - 1 - t)) is one state too narrow for the shortened labelling on both sides: the forward pass of
 * this call keeps alpha for the state below it, the deletion walk keeps beta and W for the state above it.
 * band = W: the band's own bounds (k(t) +- W from y's path) stay y's, the cone's margins lie inside them, everything lives in
 * y's slots, and a slot outside its row's window counts 0.  The carrying state of D[k] is k + 1 (its accumulator rides there),
 * of I[g][.] it is g: the sums run over the rows u at which the carrying state is inside the window of row u - 1 (deletion:
 * the deletion walk's) and the value read -- X_u[k+2], U_g[0]_u -- inside that of row u.  A lower bound that rises with W and
 * equals the exact value once the window holds the lattice (fcd_ctc_edits_*'s rule).
 * Outputs: fcd_edits, float32 log-ratios against ln P(y | x); layout, never-written entries and _host's zeros as
 * fcd_ctc_edits_*.  logp: fcd_crf_score_*'s value within its tolerance -- the extra state below the cone can move a row's
 * shared exponent and with it the last bit of the float64 logarithm.
 * Rows without a value: logp follows fcd_crf_score_*; whenever P(y | x) is not a positive finite number every entry for
 * k < min(len, stride) and g <= min(len, stride) is NaN.  A variant of probability 0: -inf (every insertion at T_r = L).  A
 * NaN posterior that only a variant reads: NaN in that variant's entry alone, logp as it is.  L = 0 writes gap 0
 * (I[0][c] = P([c] | x)) and no deletion.
 * Numerics: fcd_crf_posterior_*'s -- f32 probability space, exact power-of-two scales with integer exponents (one per forward
 * row; one per backward row shared by beta and every chain value; one per slot for its accumulators, counted from
 * floor(log2 P(y | x)), rising with the largest term), every term non-negative, one rounding per product and per sum, no
 * fused multiply-add; the log-ratio is formed in float64 from the accumulator's mantissa (its logarithm in f32), its exponent
 * and logp.  A cell below 2^-160 of its row's maximum may be dropped: an entry below -100 ln 2 may come back as -inf.
 * Error bound, by roundings along the longest chain as fcd_crf_posterior_* counts them: alpha_{u-1} carries 3 u, a chain
 * value 3 (T_r - 1 - u), a term two products, the sum over the rows at most T_r: a numerator is within (4 T_r - 1) 2^-24,
 * relative; P(y | x) within 3 T_r 2^-24; the f32 logarithm and the store add 2^-23 |value|:
 *   |error| <= 7 T_r 2^-24 + 2^-23 |value| nats.
 * FCD_E_INVALID: fcd_crf_score_*'s cases, and a null out, out->deletion or out->insertion.
 * Limits (FCD_E_UNSUPPORTED), workspace, grouping, stream order: fcd_crf_posterior_*'s, tier for tier -- every instantiation
 * carries the two walks within its 256 registers; the messages name crf_edits and the band that fits.  The launches per
 * group: forward, insertion walk, deletion walk; both walks read the stored forward rows. */
int fcd_crf_edits_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                      const fcd_labellings *y, int64_t band, const fcd_edits *out);
int fcd_crf_edits_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                       const fcd_labellings *y, int64_t band, const fcd_edits *out);

/* ---- CRF edge occupancies of given labellings (csrc/crf_posterior.hip) ----
 * NOT a reference function.  The gradient half of a CRF-CTC loss's numerator, and a soft alignment of a called sequence:
 * the probability, over the alignments of labelling y, that the model leaves state s by symbol a at row t -- the labelled
 * counterpart of fcd_crf_marginals_*'s marg, with  d ln P(y, sigma_0 | x) / d x[t][s][a] = occ[t][s][a] - marg[t][s][a]
 * for raw scores x whose (posteriors, init) fcd_crf_transition_probs_* made.
 * Everything is as fcd_crf_score_* defines it: batch (n_reads, T, S, N), nb = N - 1, sigma_0 the first maximum of the init
 * row, sigma_{k+1} = (sigma_k nb) mod S + (y_k - 1), a sigma outside the table reads as 0, the lattice k = 0 .. L, under
 * band = W the window from y->path.  alpha is fcd_crf_score_*'s, beta fcd_crf_posterior_*'s: beta_{T_r-1}[L] = 1,
 * beta_{u-1}[k] = P(u,k,0) beta_u[k] + P(u,k,y_k) beta_u[k+1], and P = alpha_{T_r-1}[L].  For a row t < T_r:
 *   stay_t[k] = alpha_{t-1}[k] * p[t][sigma_k][0]   * beta_t[k]   / P
 *   adv_t[k]  = alpha_{t-1}[k] * p[t][sigma_k][y_k] * beta_t[k+1] / P          (k < L)
 *   occ[t][s][0] = sum_{k: sigma_k = s} stay_t[k]
 *   occ[t][s][a] = sum_{k: sigma_k = s, y_k = a} adv_t[k]                       (a >= 1)
 * over the cells live in both rows' windows ("row -1" is state 0 holding 1): exact at band = 0.  Several states of a row may
 * share an entry (S = 4: sigma_k = y_{k-1} - 1); their sum is taken in an unspecified order.  Every row of occ sums to 1.
 * Output: fcd_occupancy.  Labelling row = r * n_hyp + i has its own (T, S, N) block of f32, dense (S, N) rows, row t at
 * occ + row * stride_row + t * stride_t (64-bit offsets; with n_hyp = 1 a marg buffer of fcd_crf_marginals_*, time-major
 * included).  accumulate = 0: block[t][s][a] = scale * occ;  accumulate = 1: block[t][s][a] += scale * occ (one f32 product,
 * one f32 sum).  An entry whose occupancy is 0 is not read under accumulate = 1.  logp (nullable): fcd_crf_score_*'s value,
 * the same forward recurrence, bit for bit (NaN for a labelling the walk gives up, below).
 * Rows without a value: logp follows fcd_crf_score_*'s order and values.  Whenever P(y | x) is not a positive finite number
 * nothing of the labelling's block is written (accumulate = 0: not even the zeros); rows t >= T_r and the blocks of
 * i >= n_valid[r] are never touched.  L = 0 is a labelling like any other: occupancy 1 on (sigma_0, 0) in every row.
 * Arithmetic: pass 1 is fcd_crf_score_*'s forward recurrence with every row stored; pass 2 walks the rows backwards with
 * beta alone (f32, one integer exponent per row, exact power-of-two scales).  A term is two mantissa products, the exact
 * power of two 2^(Ea(t-1) + Eb(t) + e - floor(log2 P)) and the division by P's mantissa -- three roundings; no fused
 * multiply-add; every term non-negative.  Error bound, by roundings along the longest chain: alpha_{t-1} 3 t, beta_t
 * 3 (T_r - 1 - t), the term 3, P 3 T_r and its mantissa 1, the sum of an entry's terms at most W - 1 (W: the window's states):
 *   |occ - exact| <= (6 T_r + W + 1) 2^-24 * occ;   accumulate = 1 adds 2^-24 |block| for the final sum.
 * What the rows can hold.  alpha and beta keep one f32 exponent per row, and a cell below 2^-160 of its row's maximum may
 * be dropped, as in fcd_crf_posterior_*.  Where the read supports its labelling (the read it was decoded from does; so does
 * any band around its path) the two rows' maxima meet on the alignments that carry the probability and the dropped cells
 * carry less than 2^-100 of occupancy.  Where it does not -- near-uniform or random posteriors against a labelling with
 * many rows per label -- the maxima sit at opposite ends of the window and cells that carry probability fall out of
 * range.  The walk checks every row: its terms must sum to 1 within
 *   lost(T_r) = 2 (6 T_r + 64 K + 2 K + 8) 2^-24        (K = 1, 2, 4, 8: the states a lane holds; twice the roundings above)
 * and a labelling with a row that does not is given up: logp = NaN (not fcd_crf_score_*'s value) and NaN in every row
 * t < T_r of its block, accumulate = 1 included.  So for every labelling with a finite logp every row of occ sums to 1
 * within lost(T_r), and an entry is within the relative bound above plus, at worst, the mass its row may have lost, an
 * absolute lost(T_r) + (6 T_r + W + 1) 2^-24.  Measured range at S = 4, N = 5, exact lattice:
 * uniform random posteriors hold (T, L) = (330, 300), (600, 511), (1000, 511), (1500, 511) and are given up at (1500, 255),
 * (1500, 127), (4000, 127); past about 2000 rows fcd_crf_score_*'s own value is no longer right for such reads.
 * FCD_E_INVALID: fcd_crf_score_*'s cases; a null out or out->occ; stride_t < S N; stride_row < 0; accumulate not 0 or 1;
 * with more than one labelling, blocks that overlap: either stride_row >= (T - 1) stride_t + S N (whole blocks apart) or
 * stride_row >= S N and stride_t >= (n_reads n_hyp - 1) stride_row + S N (time-major: the blocks interleaved row by row).
 * Limits (FCD_E_UNSUPPORTED; the message says which): fcd_crf_score_*'s (windows up to 512 states, the band named beyond);
 *   N - 1 <= 8;  the labelling and an S * N float row live in the 160 KiB of LDS a workgroup is granted:
 *   4 (min(T, stride) + 1) + 4 S N + 4480 <= 163840 -- S = 1024 and S = 4096 at N = 5 fit (S N up to about 39800 for a short labelling).
 *   No S = nb^m is asked for: any S fcd_crf_score_* takes.
 * _dev: device pointers, enqueue-only on the handle's stream, behind every overlapping call in flight, as
 * fcd_crf_posterior_*; the stored forward rows live in the handle's workspace and the labellings are launched in groups
 * of whole reads that fit it, forward then backward per group.  _host: host pointers; stages (the block travels both ways),
 * runs and copies back in one piece. */
typedef struct fcd_occupancy {
    float *occ;          /* the first labelling's block */
    int64_t stride_row;  /* floats between the blocks of two labellings */
    int64_t stride_t;    /* floats between two rows of a block, >= S * N */
    float scale;
    int32_t accumulate;  /* 0: block = scale * occ; 1: block += scale * occ */
    double *logp;        /* [n_reads * n_hyp], nullable */
} fcd_occupancy;
int fcd_crf_occupancy_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                          const fcd_labellings *y, int64_t band, const fcd_occupancy *out);
int fcd_crf_occupancy_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                           const fcd_labellings *y, int64_t band, const fcd_occupancy *out);

/* ---- the CRF forward sum and the occupancies for windows beyond 512 states ----
 * fcd_set_crf_lattice_wide(h, 1) makes fcd_crf_score_dev / _host and fcd_crf_occupancy_dev / _host on this handle take them,
 * (h, 0) -- the state of a new handle -- restores the limits above; any other value is FCD_E_INVALID.  The switch is read
 * when a call is made, under the handle's lock.  No new entry point: arguments, outputs, rows without a value, the
 * FCD_E_INVALID cases and the give-up rule are unchanged.  Every other CRF lattice call (fcd_crf_align_*,
 * fcd_crf_posterior_*, fcd_crf_edits_*) ignores the switch and keeps its limit.  With W = min(T, stride) + 1 states
 * (band > 0: at most 2 band + 1) the widest window of the call:
 *   W <= 512   the call is what it is with the switch off: the same launches, the same bits, the same messages.
 *   W >  512   the window lives in LDS: J = ceil(W / 64) = 9 .. 64 states per lane, still one wavefront per labelling, walked
 *              by loop bodies inside the forward and the occupancy kernels of eight states per lane.  The arithmetic is
 *              that of the register-resident walks -- the same products, one exponent per row, exact powers of two, one
 *              rounding per product and per sum, no fused multiply-add -- so fcd_crf_occupancy_*'s logp is fcd_crf_score_*'s
 *              bit for bit (the same code), and the bounds above hold with J in K's place:
 *                |occ - exact| <= (6 T_r + W + 1) 2^-24 occ,   lost(T_r) = 2 (6 T_r + 64 J + 2 J + 8) 2^-24
 *              (an entry's colliding terms meet in the S * N row as before, W - 1 sums at most; a row's mass is summed
 *              lane-serially over the J cells, one sum per term pair and one per cell, then across the wavefront: 2 J + 6).
 * What the rows can hold is unchanged -- one f32 exponent per row -- and a wider window does not hold more: INTEGRATION.md
 * section 2p has the measured range.
 * Workspace (occupancy; the score takes none): the stored rows, T (64 J + 1) 4 bytes per labelling rounded up to 256, in
 * groups of whole reads under the 4 GiB cap and the handle's workspace limit.
 * Limits (FCD_E_UNSUPPORTED; the message starts with "crf_score_wide:" / "crf_occupancy_wide:" and says which): N - 1 <= 8;
 * W <= 4096 (64 cells per lane: exact lattices up to 4095 rows or labels, bands up to 2047); S < 2^24 - 1; the labelling's
 * copy, the tile, the window's three rows (cells, products, exponents) and -- occupancy -- the S * N row within the 160 KiB
 * of LDS: 4 (min(T, stride) + 1) + 4480 + 768 J [+ 4 S N] <= 163840.  S = 1024 and S = 4096 at N = 5 fit with 2048 states. */
int fcd_set_crf_lattice_wide(fcd_handle *h, int on);

/* ---- CTC label occupancies of given labellings (csrc/ctc_posterior.hip) ----
 * NOT a reference function.  The soft version of fcd_ctc_align_*'s spans and the gradient of the CTC loss: the probability,
 * over the alignments of labelling y, that row t emits symbol c.
 * Everything is as fcd_ctc_posterior_* defines it: batch (n_reads, T, N) with in->S = 1, y of L labels, z its 2L + 1
 * extended states, collapse_repeats, under band = W the window from y->path (the labelling's own, slack 0).  alpha is
 * fcd_ctc_score_*'s forward value, b fcd_ctc_posterior_*'s backward value, "row T_r" holding all of b on state 2L:
 *   beta_t[s]  = b_{t+1}[s] (a blank, or collapse_repeats) + b_{t+1}[s+1] + b_{t+1}[s+2] (where the step is allowed)
 *   b_t[s]     = beta_t[s] * p[t][z[s]]
 *   gamma_t[s] = alpha_t[s] * beta_t[s] / P(y | x)                       for s live at row t (alpha_t: the row of the same index)
 *   occ[t][c]  = sum over the s live at row t with z[s] = c of gamma_t[s]        c = 0 .. N-1, t < T_r
 * Every row of occ sums to 1.  d ln P / d ln p[t][c] = occ[t][c]; at the logits of a softmax d(-ln P)/dx = p - occ.
 * Output: fcd_occupancy as above with N for S * N.  Labelling row = r * n_hyp + i has its own (T, N) block of f32, row t at
 * occ + row * stride_row + t * stride_t (64-bit offsets), stride_t >= N; with n_hyp = 1 a buffer of the batch's own shape,
 * time-major included.  accumulate = 0: block[t][c] = scale * occ (a cell of occupancy 0 holds +0);  accumulate = 1:
 * block[t][c] += scale * occ (one f32 product, one f32 sum), and a cell whose occupancy is 0 is not read.  logp (nullable):
 * fcd_ctc_score_*'s value, bit for bit (NaN for a labelling the walk gives up, below).
 * Rows without a value: logp follows fcd_ctc_score_*'s order and values.  Whenever P(y | x) is not a positive finite number
 * nothing of the labelling's block is written; rows t >= T_r and the blocks of i >= n_valid[r] are never touched.  L = 0 is a
 * labelling like any other: occupancy 1 on the blank in every row.
 * Arithmetic: pass 1 is fcd_ctc_posterior_*'s forward launch with every row stored; pass 2 walks the rows backwards with b
 * alone (f32, one integer exponent per row, exact power-of-two scales).  A term gamma is one product, the exact power of two
 * 2^(Ea(t) + Eb(t+1) - floor(log2 P)) and the division by P's mantissa; no fused multiply-add; every term non-negative.  A
 * label's sum is taken in a fixed order -- a lane's own states, then the lanes of the wavefront, 6 sums deep -- so two calls
 * on the same input give the same bits.  Error bound, by roundings along the longest chain: alpha_t 3 (t + 1), beta_t
 * 3 (T_r - 1 - t) + 2, the term and the division 2, P 3 T_r + 1 and its mantissa 1, a label's sum K / 2 - 1 + 6 with
 * K = 2, 4, 6, 8 the states a lane holds (windows up to 126, 254, 382, 510 states):
 *   bound(T_r) = (6 T_r + K / 2 + 11) 2^-24,   |occ - exact| <= bound(T_r) * occ;
 *   accumulate = 1 adds 2^-24 |block| for the final sum.
 * What the rows can hold.  alpha and b keep one f32 exponent per row, and a cell below 2^-160 of its row's maximum may be
 * dropped, as in fcd_ctc_posterior_*.  Where the read supports its labelling the two rows' maxima meet on the alignments
 * that carry the probability.  Where it does not -- near-uniform posteriors against a labelling with many rows per label --
 * the maxima sit at opposite ends of the window and cells that carry probability fall out of range.  The walk sums every
 * row (the N label sums, N - 1 <= 8 more roundings); the sum must be 1 within
 *   lost(T_r) = 2 (6 T_r + K / 2 + 19) 2^-24
 * and a labelling with a row that is not is given up: logp = NaN (not fcd_ctc_score_*'s value) and NaN in every row
 * t < T_r of its block, accumulate = 1 included.  So for every labelling with a finite logp every row of occ sums to 1
 * within lost(T_r) and |occ - exact| <= bound(T_r) * occ + lost(T_r).  The measured range is in INTEGRATION.md section 2n.
 * FCD_E_INVALID: fcd_ctc_posterior_*'s cases; a null out or out->occ; stride_t < N; stride_row < 0; accumulate not 0 or 1;
 * with more than one labelling, blocks that overlap: either stride_row >= (T - 1) stride_t + N (whole blocks apart) or
 * stride_row >= N and stride_t >= (n_reads n_hyp - 1) stride_row + N (time-major: the blocks interleaved row by row).
 * Limits (FCD_E_UNSUPPORTED; the message names ctc_occupancy): fcd_ctc_posterior_*'s -- windows up to 510 states (use a
 * band), N - 1 <= 8, min(T, stride) <= 28480.
 * _dev: device pointers, enqueue-only on the handle's stream, behind every overlapping call in flight, as
 * fcd_ctc_posterior_*; the stored forward rows live in the handle's workspace and the labellings are launched in groups of
 * whole reads that fit it.  _host: host pointers; stages (the block travels both ways), runs and copies back in one piece. */
int fcd_ctc_occupancy_dev(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                          const fcd_occupancy *out);
int fcd_ctc_occupancy_host(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                           const fcd_occupancy *out);

/* ---- the same occupancies for every labelling fcd_ctc_score_* takes: windows beyond 510 states ----
 * fcd_set_ctc_occupancy_wide(h, 1) makes fcd_ctc_occupancy_dev / _host on this handle take them, (h, 0) -- the state of a
 * new handle -- restores the limits above; any other value is FCD_E_INVALID.  The switch is read when a call is made, under
 * the handle's lock.  No new entry point: arguments, outputs, rows without a value, FCD_E_INVALID and the give-up rule are
 * unchanged; while the switch is on, error messages name ctc_occupancy_wide.  With S = 2 min(T, stride) + 1 states (band = W > 0: at most 4 W + 3) the widest window of the call:
 *   S <= 510   the call is what it is with the switch off: the same launches, the same bits, bound(T_r) and lost(T_r) above.
 *   S >  510   the window lives in LDS (fcd_ctc_score_*'s kernel for such windows, 256 work-items up to S = 2048, 512 up to
 *              5120, 1024 beyond: nw = 4, 8, 16 wavefronts): its forward walk once more, storing every row, then a backward
 *              walk of the same arithmetic as above -- one product, the exact power of two, the division by P's mantissa; no
 *              fused multiply-add; every term non-negative.  logp is fcd_ctc_score_*'s value bit for bit.
 * A label's sum is taken in a fixed order, so two calls give the same bits: a work-item adds its up to 10 cells of the label
 * in increasing state order (9 sums), the 64 lanes of a wavefront (6 deep), the wavefronts in their order (nw - 1).  By the
 * chain of fcd_ctc_occupancy_* -- alpha_t 3 (t + 1), beta_t 3 (T_r - 1 - t) + 2, the term and the division 2, P 3 T_r + 1
 * and its mantissa 1: 6 T_r + 6 -- with this depth in place of K / 2 - 1 + 6 the roundings come to 6 T_r + nw + 20; the
 * contract keeps 6 more in hand:
 *   bound_w(T_r) = (6 T_r + 9 + 6 + (nw - 1) + 12) 2^-24 = (6 T_r + nw + 26) 2^-24,   |occ - exact| <= bound_w(T_r) * occ;
 *   lost_w(T_r)  = 2 (6 T_r + nw + 34) 2^-24       (twice the roundings of a row's sum: N - 1 <= 8 more)
 * and for every labelling with a finite logp every row sums to 1 within lost_w(T_r) and
 * |occ - exact| <= bound_w(T_r) * occ + lost_w(T_r); accumulate = 1 adds 2^-24 |block|.  A row further from 1 gives the
 * labelling up, as above.  What the rows can hold is unchanged: one f32 exponent per row.
 * Workspace: the stored rows, T (S + 1) 4 bytes per labelling rounded up to 256 (S <= 510: fcd_ctc_occupancy_*'s), in
 * groups of whole reads under the 4 GiB cap and the handle's workspace limit.
 * Limits (FCD_E_UNSUPPORTED; the message starts with "ctc_occupancy_wide:" and says which): N - 1 <= 8; S <= 10240 (1024
 * work-items of 10 cells: exact lattices up to 5119 rows or labels, bands up to 2559); 2 min(T, stride) + 8 S + 9152 bytes -- the labelling's copy, the tile, the two rows of the
 * window and the 16 x 9 reduction words -- within the 160 KiB of LDS; S <= 510: min(T, stride) <= 28480. */
int fcd_set_ctc_occupancy_wide(fcd_handle *h, int on);

/* ---- search::crf_greedy_search (src/search.rs:385-423) ---- */
int fcd_crf_greedy_search_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                              int64_t init_stride, const fcd_result *out);
int fcd_crf_greedy_search_host(fcd_handle *h, const fcd_batch *in, const float *init,
                               int64_t n_init, int64_t init_stride, const fcd_result *out);

/* ---- the Viterbi search under a CRF model: the single most probable path through the model's states ----
 * NOT a reference function.  The exact, unpruned decode over ALL labellings: fcd_crf_greedy_search_* follows the locally
 * best label (a lower bound), fcd_crf_beam_search_* is a pruned sum over alignments, fcd_crf_align_* finds the best
 * alignment of ONE labelling; this finds the best alignment over all of them -- no labelling's best alignment beats it.
 * Batch and reading rule: (n_reads, T, S, N) posteriors, init rows and nb = N - 1 as fcd_crf_greedy_search_* /
 * fcd_crf_align_* read them: f32 / f16 / bf16 converted exactly, any strides (time-major views included), in->lengths.
 * Start: sigma_0 = the first maximum of the read's init row (the init probabilities do not enter, as in
 * fcd_crf_score_*); v_{-1}[sigma_0] = 1, every other state 0.
 * Step, for every state s':   v_t[s'] = max( v_{t-1}[s'] p_t[s'][0] ,  max_i v_{t-1}[s_i] p_t[s_i][j+1] )
 *   j = s' mod nb,  q = S / nb,  s_i = s' div nb + i q,  i = 0 .. nb-1:  exactly the states with (s_i nb) mod S + j = s',
 *   the searches' transition (src/search.rs:97,414).  The formula needs S mod nb = 0 (every S = nb^m, and other multiples).
 * Ties: the stay candidate is kept unless an advance is strictly greater; among advances the lowest i unless a later one is
 * strictly greater; the end state is the first maximum of v_{T_r-1}.
 * Result, by traceback from the end state: path = the emitting rows in order, labels = their labels j + 1, qual[k] = the
 * posterior of that emission p_t[s_i][j+1] (what fcd_crf_greedy_search_* feeds to phred), logp[read] = ln v_{T_r-1}[end],
 * float64.  out->qual, out->path and logp are nullable; out->status is required; out->ambiguous is not written.  Entries
 * of labels / path / qual at and beyond out_len are unspecified (the traceback parks emissions there).
 * Edge cases: a NaN in the init row (or an init row no state follows from: sigma_0 >= S with T_r > 0): FCD_ST_BAD_STATE,
 * out_len 0, logp NaN, as greedy.  T_r = 0: out_len 0, logp 0.0, FCD_ST_OK.  A NaN anywhere in rows 0 .. T_r-1 of the read:
 * FCD_ST_INCOMPARABLE, out_len 0, logp NaN (every value of a read enters a live cell).  Infinite or negative posteriors:
 * the call terminates and writes some result, nothing more.
 * Arithmetic: fcd_crf_align_*'s -- f32 with an unbounded exponent (mantissa / exponent split, exact power-of-two rescaling
 * per row), each candidate ONE product with one rounding, no fused multiply-add, ln(m) + E ln 2 in float64; a cell below
 * 2^-160 of its row's maximum may be dropped.  Executable specification: tests/crf_viterbi_reference.py.
 * Limits (FCD_E_UNSUPPORTED; the message says which): 2 <= N <= 9; S a multiple of N - 1; S < 2^24; N S 4 bytes of LDS
 * per read (the states and their N - 1 advance candidates) within the 160 KiB of a CU (S = 4096 at N = 5: 80 KiB).
 * Workspace: one back-pointer byte per state and row, T S bytes per read (rounded up to 256), from the handle's workspace;
 * whole reads per launch, as many as min(4 GiB, the handle's workspace budget) holds, the launches one after the other in
 * the same memory (fcd_debug_set_align_workspace_cap sets the cap for tests).
 * _dev is enqueue-only on the handle's stream (never on fcd_set_overlap's internal streams) and ordered behind every
 * overlapping call in flight; _host stages host arrays and returns when the results are in them.
 * FCD_E_INVALID: null in / out / labels / out_len / status, out_stride < T, null init or n_init < 1, negative init_stride. */
int fcd_crf_viterbi_search_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                               const fcd_result *out, double *logp);
int fcd_crf_viterbi_search_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                                const fcd_result *out, double *logp);

/* ---- CRF transition probabilities: a network's raw scores -> the (posteriors, init) pair every CRF entry point reads ----
 * NOT a reference function.  A CRF basecaller network emits unnormalised log scores; this is the backward pass over all
 * labellings and the local softmax that turn them into transition posteriors and an init row, on the device.
 * Input: `scores`, a (n_reads, T, S, N) batch of log scores, f32 / f16 / bf16 converted exactly, any non-negative strides
 * (time-major views included), scores->lengths.  nb = N - 1.  Symbol 0 stays in state s; symbol j + 1 emits label j + 1 and
 * moves to d(s, j + 1) = (s nb) mod S + j (src/search.rs:97,414); d(s, 0) = s.  Per read, with x[t][s][a] its scores:
 *     beta_T[s]  = 0
 *     y_t[s][a]  = x[t][s][a] + beta_{t+1}[d(s, a)]
 *     beta_t[s]  = ln sum_a exp y_t[s][a]
 *     p[t][s][a] = exp(y_t[s][a] - beta_t[s])                       out->probs: every row over a sums to 1
 *     init[s]    = exp(beta_0[s] - logZ),  logZ = ln sum_s exp beta_0[s]     out->init, out->logz
 * Property: for every start state s0 and every symbol sequence a_0 .. a_{T-1} with the states s_t it passes,
 *     init[s0] prod_t p[t][s_t][a_t] = exp(sum_t x[t][s_t][a_t] - logZ):
 * the locally normalised outputs reproduce the globally normalised model exactly, which is what gives the searches'
 * products of posteriors their meaning.
 * Layout of the scores:
 *   FCD_LAYOUT_SOURCE  x[t][s][a] as above: indexed as the output is, by the state being LEFT.
 *   FCD_LAYOUT_DEST    xd[t][s'][.] indexed by the state being ENTERED: xd[t][s'][0] stays at s'; xd[t][s'][1 + i] enters s'
 *                      from s_i = s' div nb + i (S / nb), the s_i of fcd_crf_viterbi_search_*.  That is
 *                      x[t][s][j + 1] = xd[t][(s nb) mod S + j][1 + (s nb) div S] and x[t][s][0] = xd[t][s][0]; the layout is
 *                      defined by this formula alone.  A different offset per element at load time; no transposing pass.
 *   The output is always source-indexed.
 * Output (fcd_transitions):
 *   probs  f32 (FCD_DTYPE_F32) or f16 (FCD_DTYPE_F16: the f32 value rounded to nearest even), element (r, t, s, a) at
 *          probs[r stride_read + t stride_t + s N + a]: dense (S, N) rows, the caller's read and row strides in elements
 *          (stride_read = S N, stride_t = n_reads S N is the time-major (T, B, S, N) tensor).  Rows t >= T_r are not written.
 *   init   f32, [n_reads * init_stride], S per read;  logz  float64 per read, nullable;  status  FCD_ST_* per read.
 * Arithmetic (f32; executable specification: tests/crf_transitions_reference.py): beta is renormalised by its row maximum
 * at every step, beta~_t = beta_t - c_t with c_t = max_s beta_t[s] -- the outputs depend on differences only --, and
 * logZ = sum_t c_t + ln sum_s exp beta~_0[s], accumulated in float64.  Per state m = max_a y, e_a = exp(y_a - m), the sum in
 * the order a = 0 .. N - 1, p_a = e_a / sum, beta = m + ln sum.  init[s] = exp(beta~_0[s]) / sum_s exp(beta~_0[s]).  exp and ln
 * are the device's fast forms (a few ulp).
 * Edge cases: x = -inf is a forbidden transition, its p exactly 0.  A state whose N candidates are all -inf is dead: its p
 * row is all zeros, its beta -inf; dead at row 0, its init is 0.  A read FAILS -- FCD_ST_INCOMPARABLE, logz NaN, its probs
 * and init unspecified, the other reads unaffected -- if a row of beta~ has no live state (no path has positive weight) or
 * a row t < T_r holds a NaN or +inf.  T_r = 0: init = 1 / S, logz = ln S, FCD_ST_OK.
 * Limits (FCD_E_UNSUPPORTED; the message says which): 2 <= N <= 9; S a multiple of N - 1; S < 2^24; 8 S + 4608 bytes of LDS
 * per read (two rows of beta~ and the store staging) within the 160 KiB of a CU.  No workspace: beta~ is never stored.
 * _dev is enqueue-only on the handle's stream (never on fcd_set_overlap's internal streams) and ordered behind every
 * overlapping call in flight; _host stages host arrays (probs included: rows t >= T_r keep the caller's content) and
 * returns when the results are in them.
 * FCD_E_INVALID: null scores / out / probs / init / status, an unknown layout or dtype, stride_read or stride_t below S N,
 * init_stride below S. */
enum { FCD_LAYOUT_SOURCE = 0, FCD_LAYOUT_DEST = 1 };

typedef struct fcd_transitions {
    void *probs;
    int32_t dtype;       /* FCD_DTYPE_F32 or FCD_DTYPE_F16 */
    int64_t stride_read;
    int64_t stride_t;
    float *init;
    int64_t init_stride;
    double *logz;        /* nullable */
    int32_t *status;
} fcd_transitions;

int fcd_crf_transition_probs_dev(fcd_handle *h, const fcd_batch *scores, int layout, const fcd_transitions *out);
int fcd_crf_transition_probs_host(fcd_handle *h, const fcd_batch *scores, int layout, const fcd_transitions *out);

/* ---- CRF edge marginals over all labellings: the forward pass behind fcd_crf_transition_probs_*, logZ and its gradient ----
 * NOT a reference function.  How probable it is, over every labelling, that the model takes transition a out of state s at
 * row t: the true posterior of an emission (the searches' qualities are the local conditional p[t][s][a], which ignores how
 * likely the model is to be in s at all), summed over states a (T, N) matrix of label posteriors whose rows sum to 1, and
 * exactly d logZ / d x, the denominator gradient of CRF-CTC training.
 * Input: `scores` and `layout` as fcd_crf_transition_probs_* take them; x, nb, d(s, a), beta and logZ as defined there.  Every
 * start state is allowed.  Per read:
 *     alpha_0[s]      = 0
 *     alpha_{t+1}[s'] = ln sum_{(s, a): d(s, a) = s'} exp(alpha_t[s] + x[t][s][a])
 *     marg[t][s][a]   = exp(alpha_t[s] + x[t][s][a] + beta_{t+1}[d(s, a)] - logZ)      source-indexed, as probs is
 *     emit[t][a]      = sum_s marg[t][s][a]
 * Identities: sum_{s, a} marg[t] = 1 for every row t < T_r; sum_a marg[t][s][a] = exp(alpha_t[s] + beta_t[s] - logZ), the
 * state occupancy; marg = d logZ / d x.
 * Output (fcd_marginals):
 *   marg   f32, element (r, t, s, a) at marg[r stride_read + t stride_t + s N + a]: dense (S, N) rows, the caller's read and
 *          row strides in elements, as fcd_transitions.probs.  Required: it is the walk's own storage -- the backward pass
 *          writes p into it, the forward pass multiplies it in place; there is no workspace.  Rows t >= T_r are not written.
 *   emit   f32, nullable: element (r, t, a) at emit[r emit_stride + t N + a], emit_stride >= T N.  Rows t >= T_r are not
 *          written.
 *   logz   float64 per read, nullable: fcd_crf_transition_probs_*'s value, bit for bit;  status  FCD_ST_* per read.
 * Arithmetic (f32; executable specification: tests/crf_marginals_reference.py): (p, init) of fcd_crf_transition_probs_* is the
 * model restated as a Markov chain, so the forward pass propagates state occupancies and needs no exp or ln:
 *     pi_0 = init;  marg[t][s][a] = pi_t[s] p[t][s][a];  pi_{t+1}[s'] = marg[t][s'][0] + sum_{i = 0 .. nb-1} marg[t][s_i][j + 1]
 * with s_i = s' div nb + i (S / nb), j = s' mod nb, the sum taken left to right in that order from the stay term on.  emit is
 * summed in f32 in an unspecified order.
 * Edge cases: x = -inf gives marg exactly 0.  A failed read (fcd_crf_transition_probs_*'s rule) has FCD_ST_INCOMPARABLE, logz
 * NaN, marg and emit unspecified; the other reads are unaffected.  T_r = 0: FCD_ST_OK, logz = ln S, nothing else written.
 * Limits: those of fcd_crf_transition_probs_*, the LDS included (8 S + 4608 bytes per read).
 * _dev is enqueue-only on the handle's stream, one kernel launch, ordered behind every overlapping call in flight; _host
 * stages host arrays (marg and emit travel both ways: rows t >= T_r keep the caller's content).
 * FCD_E_INVALID: null scores / out / marg / status, an unknown layout, stride_read or stride_t below S N, emit_stride below
 * T N.  Out of scope: f16 marginals, marginals without the (T, S, N) buffer, the numerator of a training loss. */
typedef struct fcd_marginals {
    float *marg;
    int64_t stride_read;
    int64_t stride_t;
    float *emit;         /* nullable */
    int64_t emit_stride;
    double *logz;        /* nullable */
    int32_t *status;
} fcd_marginals;

int fcd_crf_marginals_dev(fcd_handle *h, const fcd_batch *scores, int layout, const fcd_marginals *out);
int fcd_crf_marginals_host(fcd_handle *h, const fcd_batch *scores, int layout, const fcd_marginals *out);

/* ---- duplex::beam_search (src/duplex.rs:443-650) ----
 * (Two kernels serve the duplex searches since round 6, with identical results: the slot-resident one --
 * csrc/duplex_slots.hip -- wherever beam_size * N <= 64 and the live nodes' windows fit the LDS, the any-shape one --
 * csrc/duplex.hip -- otherwise.  Nothing at this boundary depends on which runs; FCD_DUPLEX_KERNEL=legacy|slots and
 * fcd_debug_set_duplex_kernel (fcd_debug.h) force one for A/B runs and tests.)
 * in1/in2 describe the two reads of each pair (same n_reads and N); envelope is
 * [n_reads * env_stride] pairs of u64 (lo,hi), row t of pair r at envelope[(r*env_stride + t)*2].
 * Only labels/out_len/status (and the tie counters `ambiguous`, when given) of `out` are written (the reference
 * returns the string only). */
int fcd_beam_search_duplex_dev(fcd_handle *h, const fcd_batch *in1, const fcd_batch *in2,
                               const uint64_t *envelope, int64_t env_stride, int64_t beam_size,
                               float beam_cut_threshold, int collapse_repeats, int logadd_mode,
                               const fcd_result *out);
int fcd_beam_search_duplex_host(fcd_handle *h, const fcd_batch *in1, const fcd_batch *in2,
                                const uint64_t *envelope, int64_t env_stride, int64_t beam_size,
                                float beam_cut_threshold, int collapse_repeats, int logadd_mode,
                                const fcd_result *out);

/* ---- duplex::crf_beam_search (src/duplex.rs:652-834) ----
 * in1/in2 are (T,S,N) batches with the same S and N; init1/init2: [n_reads * initX_stride] f32 with
 * n_initX entries used per pair (the start state is their argmax, src/duplex.rs:679,691). */
int fcd_crf_beam_search_duplex_dev(fcd_handle *h, const fcd_batch *in1, const float *init1,
                                   int64_t n_init1, int64_t init1_stride, const fcd_batch *in2,
                                   const float *init2, int64_t n_init2, int64_t init2_stride,
                                   const uint64_t *envelope, int64_t env_stride, int64_t beam_size,
                                   float beam_cut_threshold, int logadd_mode, const fcd_result *out);
int fcd_crf_beam_search_duplex_host(fcd_handle *h, const fcd_batch *in1, const float *init1,
                                    int64_t n_init1, int64_t init1_stride, const fcd_batch *in2,
                                    const float *init2, int64_t n_init2, int64_t init2_stride,
                                    const uint64_t *envelope, int64_t env_stride, int64_t beam_size,
                                    float beam_cut_threshold, int logadd_mode, const fcd_result *out);

/* ---- alignment-band estimator for the duplex searches ----
 * NOT a reference function: duplex::beam_search takes the envelope as an argument, the PyO3 wrapper
 * defaults to the full matrix and its docstring only anticipates a better default
 * (/root/reference/src/lib.rs:376-378,459-468).  Input: per pair, the label sequences of the two
 * reads with their emission times (e.g. the labels / path / out_len arrays of fcd_viterbi_search_*).
 * The label sequences are aligned globally (unit-cost edit distance); matched labels anchor read-1
 * time to read-2 time; envelope row i = [centre(i) - band, centre(i) + band + 1) clipped to
 * [0, T2], with lo(0) = 0, hi(T1 - 1) = T2 and consecutive rows touching (src/duplex.rs:485-488).
 * T1 / T2: nullable per-pair row counts (else T1cap / T2cap).  Limits: at most 65535 labels per pair and
 * ~13000 labels in read 2 (the DP rows live in LDS as u16; FCD_E_UNSUPPORTED beyond).  Executable specification: tests/envelope_model.py. */
int fcd_duplex_envelope_dev(fcd_handle *h, int64_t n_pairs,
                            const uint8_t *labels1, const uint32_t *path1, const uint32_t *len1,
                            int64_t stride1, const int64_t *T1, int64_t T1cap,
                            const uint8_t *labels2, const uint32_t *path2, const uint32_t *len2,
                            int64_t stride2, const int64_t *T2, int64_t T2cap,
                            int64_t band, uint64_t *envelope, int64_t env_stride);
int fcd_duplex_envelope_host(fcd_handle *h, int64_t n_pairs,
                             const uint8_t *labels1, const uint32_t *path1, const uint32_t *len1,
                             int64_t stride1, const int64_t *T1, int64_t T1cap,
                             const uint8_t *labels2, const uint32_t *path2, const uint32_t *len2,
                             int64_t stride2, const int64_t *T2, int64_t T2cap,
                             int64_t band, uint64_t *envelope, int64_t env_stride);


/* ---- compact wire format of a shard's results, for the ONE gather of the multi-GPU path ----
 * The searches write fixed-stride rows; only out_len[r] entries of row r are meaningful (~48 % at BASELINE
 * config 2).  These three calls turn a result into one contiguous buffer holding just the used prefixes
 * (layout in csrc/pack.hip) and back.  All pointers are device memory; work is enqueued on the handle's stream.
 *   1. fcd_result_offsets_dev: offsets[i] = sum of out_len[0..i) (clamped to out_stride), offsets[n_reads] =
 *      total labels.  Read offsets[n_reads] back to size the buffer: fcd_packed_result_bytes().
 *   2. fcd_pack_results_dev: labels/path(u32 -> path_bytes = 2 or 4 wide)/out_len/status -> buf.
 *   3. fcd_unpack_results_dev: buf -> fixed-stride arrays of `out` (offsets: workspace of n_reads+1 u64). */
int64_t fcd_packed_result_bytes(int64_t n_reads, int64_t total_labels, int path_bytes);
int fcd_result_offsets_dev(fcd_handle *h, const uint32_t *out_len, int64_t n_reads, int64_t out_stride,
                           uint64_t *offsets);
int fcd_pack_results_dev(fcd_handle *h, const fcd_result *res, int64_t n_reads, int path_bytes,
                         const uint64_t *offsets, uint8_t *buf);
int fcd_unpack_results_dev(fcd_handle *h, const uint8_t *buf, int64_t n_reads, uint64_t *offsets,
                           const fcd_result *out);

/* ---- the multi-GPU step without Python (csrc/comm.hip) ----------------------------------------
 * One process per GPU; reads shard across the ranks with no exchange inside the searches; what is left is ONE
 * gather of every rank's decoded results on a destination rank over RCCL / xGMI.  RCCL is loaded at run time
 * (dlopen), so single-GPU users never need it.
 *   fcd_comm_unique_id   rank 0 makes the 128-byte id (ncclGetUniqueId); the host hands it to the other ranks
 *   fcd_comm_create      ncclCommInitRank on the handle's device (collective: every rank calls it)
 *   fcd_comm_wrap        use an ncclComm_t the host already owns (passed as void*); NULL is allowed for world = 1
 *   fcd_gather_results_dev  this rank's `res` (n_reads fixed-stride rows in device memory, e.g. what
 *                        fcd_beam_search_dev wrote) -> on rank `dst`, `out` receives all ranks' rows in global read
 *                        order (counts[k] = reads of rank k; out->out_stride >= res->out_stride).  Steps, all on
 *                        the handle's stream: prefix sums + pack of the used prefixes (u16 times below 65536 rows),
 *                        a 16-byte ncclAllReduce(MAX) of {label total, out_stride} so that all ranks send one size (the
 *                        ranks' out_stride should be equal; the destination's must not be narrower), ONE ncclGather, and on `dst`
 *                        the unpack of every shard with one pair of launches.  The call waits for the device once
 *                        (the agreed size: 16 bytes); the gather and the unpack are left in flight on the stream.  An error a
 *                        rank finds after the all-reduce is reported once its own ncclGather is enqueued: no rank is left hanging.
 *   fcd_comm_synchronize waits for the stream and reports a shard whose header contradicted `counts`
 *                        (FCD_E_INVALID; such a shard's rows are left empty, never read out of bounds). */
#define FCD_COMM_ID_BYTES 128
typedef struct fcd_comm fcd_comm;
int fcd_comm_unique_id(uint8_t id[FCD_COMM_ID_BYTES]);
int fcd_comm_create(fcd_handle *h, int world, int rank, const uint8_t id[FCD_COMM_ID_BYTES], fcd_comm **out);
int fcd_comm_wrap(fcd_handle *h, void *nccl_comm, int world, int rank, fcd_comm **out);
int fcd_comm_destroy(fcd_comm *c);
int fcd_gather_results_dev(fcd_comm *c, const fcd_result *res, int64_t n_reads, const int64_t *counts, int dst,
                           const fcd_result *out);
int fcd_comm_synchronize(fcd_comm *c);
/* The unpack step on its own (what fast_ctc_decode_amd/dist.py calls after torch.distributed's gather):
 * gathered = world packed shards of `stride` bytes each, back to back; first = DEVICE array [world + 1] of
 * prefix sums of the per-rank read counts; offsets = DEVICE workspace of first[world] + world u64; bad = DEVICE
 * int32 that receives 1 + shard for a shard whose header contradicts the counts or the buffer size. */
int fcd_unpack_gathered_dev(fcd_handle *h, const uint8_t *gathered, int64_t stride, int world, const int64_t *first,
                            int64_t n_total, uint64_t *offsets, const fcd_result *out, int32_t *bad);

/* ---- coalescing front door for per-read callers (csrc/coalesce.hip) --------------------------------------
 * The reference decodes ONE read per call and releases the GIL around the search so that callers can run it
 * from many threads (src/lib.rs:199 viterbi_search, :353 beam_search).  On a GPU a lone read is one wavefront;
 * a coalescer turns CONCURRENT per-read calls into batched launches without changing the callers: the first
 * thread to arrive decodes every compatible pending request (same search, alphabet size, beam size, threshold,
 * collapse flag) with one ragged batch on one of the coalescer's own handles; whatever arrives while that launch
 * is in flight forms the next batch.  max_wait_us = 0 (adaptive): before launching, a leader waits briefly for
 * the callers of the previous batches to come back (until as many requests are pending as recent batches held,
 * at most an eighth of the last launch's duration, <= 1 ms); a lone caller never waits.  max_wait_us > 0: every
 * leader waits up to that long for company (or until max_batch requests are pending).  A few
 * leaders run side by side while fewer than four reads are in flight, so a handful of callers overlap like
 * independent per-read calls.  Results are bit-identical to the per-read calls.
 * `read` must describe exactly one (T, N) matrix (n_reads = 1, S <= 1, non-negative strides, no lengths);
 * `out` is a one-read fcd_result with out_stride >= T.  Blocking; any number of threads.  On failure the text
 * is in fcd_coalescer_last_error() (per calling thread). */
typedef struct fcd_coalescer fcd_coalescer;
int fcd_coalescer_create(int device, int max_batch, int max_wait_us, fcd_coalescer **out);
int fcd_coalescer_destroy(fcd_coalescer *c);   /* FCD_E_INVALID while calls are in flight */
int fcd_coalescer_beam_search(fcd_coalescer *c, const fcd_batch *read, int64_t beam_size,
                              float beam_cut_threshold, int collapse_repeats, const fcd_result *out);
int fcd_coalescer_viterbi_search(fcd_coalescer *c, const fcd_batch *read, int collapse_repeats,
                                 const fcd_result *out);
/* r04: the CRF searches (src/search.rs:38-157, :385-423) through the same door: one (T, S, N) read and its init_state
 * (n_init contiguous floats) per call; calls with the same S, N, n_init, beam and threshold share a launch. */
int fcd_coalescer_crf_beam_search(fcd_coalescer *c, const fcd_batch *read, const float *init, int64_t n_init,
                                  int64_t beam_size, float beam_cut_threshold, const fcd_result *out);
int fcd_coalescer_crf_greedy_search(fcd_coalescer *c, const fcd_batch *read, const float *init, int64_t n_init,
                                    const fcd_result *out);
/* r05: the pair searches (src/duplex.rs:443-650, :652-834; the reference's beam_search_duplex /
 * crf_beam_search_duplex, src/lib.rs:401-578, decode ONE pair per call with the GIL released): read1 / read2 as above,
 * `envelope` = read1->T rows of {lo, hi} (u64), logadd_mode = FCD_LOGADD_*.  A lone pair is one wavefront walking a
 * 2000-step chain: per-pair callers get the latency of a whole batch per call -- through this door concurrent calls
 * with the same N (S, init sizes), beam, threshold, collapse flag and log-add flavour share ONE launch. */
int fcd_coalescer_beam_search_duplex(fcd_coalescer *c, const fcd_batch *read1, const fcd_batch *read2,
                                     const uint64_t *envelope, int64_t beam_size, float beam_cut_threshold,
                                     int collapse_repeats, int logadd_mode, const fcd_result *out);
int fcd_coalescer_crf_beam_search_duplex(fcd_coalescer *c, const fcd_batch *read1, const float *init1, int64_t n_init1,
                                         const fcd_batch *read2, const float *init2, int64_t n_init2,
                                         const uint64_t *envelope, int64_t beam_size, float beam_cut_threshold,
                                         int logadd_mode, const fcd_result *out);
int fcd_coalescer_stats(fcd_coalescer *c, int64_t *n_calls, int64_t *n_launches, int64_t *largest_batch);
const char *fcd_coalescer_last_error(void);

/* ---- large HOST batches as a stream of result chunks (csrc/hostjob.hip) -----------------------------------
 * The reference's callers hold posteriors in host memory (src/lib.rs:182,325: &PyArray2<f32>) and want strings
 * and paths back (src/lib.rs:208,361).  A job decodes a host batch chunk by chunk on a few internal lanes (own
 * stream, staging area and tree arena each): the upload of chunk c+1 overlaps the searches of the chunks before
 * it, only the USED prefix of every result row crosses PCIe (times as u16 when T < 65536), and the caller can
 * turn chunk c into its own objects while later chunks are still in flight.
 *   fcd_*_host_begin   same arguments and checks as fcd_*_host (host pointers; they must stay valid until
 *                      fcd_job_end) plus `want`, an OR of FCD_JOB_*; starts the pipeline and returns.
 *   fcd_job_next       blocks until the next chunk (in read order) is in host memory and describes it in *out;
 *                      the view stays valid until the next fcd_job_next / fcd_job_end on the job.  Returns
 *                      FCD_OK, FCD_JOB_DONE after the last chunk, or a negative FCD_E_*.
 *   fcd_job_end        always call: waits for / cancels outstanding work and frees the job.
 * One job at a time per handle; the handle's other entry points may be used again after fcd_job_end.
 * fcd_*_host on large batches (>= 128 reads and >= 16 MB) runs the same pipeline and expands the chunks into the
 * caller's fixed-stride arrays.  Environment: FCD_HOST_LANES (default 3; 1 = no pipelining), FCD_HOST_CHUNK
 * (reads per chunk; default = the batch split evenly over the lanes, at most 2048). */
enum { FCD_JOB_PATH = 1, FCD_JOB_QUAL = 2, FCD_JOB_AMBIGUOUS = 4 };
enum { FCD_JOB_DONE = 1 };
typedef struct fcd_job fcd_job;
typedef struct fcd_chunk {
    int64_t read_begin;        /* index of the chunk's first read in the batch */
    int64_t n_reads;
    const uint32_t *out_len;   /* [n_reads] */
    const int32_t *status;     /* [n_reads] FCD_ST_* */
    const uint64_t *offsets;   /* [n_reads + 1]: read i owns entries offsets[i] .. offsets[i+1] of the arrays below */
    const uint8_t *labels;     /* label indices of read 0, read 1, ... back to back */
    const void *path;          /* u16 (path_bytes == 2) or u32 (4) row indices, same order; NULL unless FCD_JOB_PATH */
    int path_bytes;
    const float *qual;         /* NULL unless FCD_JOB_QUAL (viterbi / crf_greedy) */
    const uint32_t *ambiguous; /* [n_reads][2] tie counters (fcd_result.ambiguous); NULL unless FCD_JOB_AMBIGUOUS */
} fcd_chunk;
int fcd_viterbi_search_host_begin(fcd_handle *h, const fcd_batch *in, int collapse_repeats, int want, fcd_job **job);
int fcd_beam_search_host_begin(fcd_handle *h, const fcd_batch *in, int64_t beam_size, float beam_cut_threshold,
                               int collapse_repeats, int kernel, int want, fcd_job **job);
int fcd_crf_beam_search_host_begin(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                                   int64_t init_stride, int64_t beam_size, float beam_cut_threshold, int kernel,
                                   int want, fcd_job **job);
int fcd_crf_greedy_search_host_begin(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                                     int64_t init_stride, int want, fcd_job **job);
/* The same jobs for a batch whose reads are SEPARATE host arrays -- a Python list of ragged matrices, which is how the
 * reference's callers hold them (src/lib.rs:325,352 take one read per call): reads[r] points at read r's contiguous
 * (rows[r], N) matrix of element type `dtype`.  Every chunk is gathered into page-locked memory by its lane (the lanes
 * gather side by side) and leaves as one DMA: no padded copy of the batch on the caller's side.  reads / rows must stay
 * valid until fcd_job_end.  Chunk views are the same (out_stride = the longest read). */
int fcd_viterbi_search_host_ptrs_begin(fcd_handle *h, const void *const *reads, const int64_t *rows, int64_t n_reads,
                                       int64_t N, int dtype, int collapse_repeats, int want, fcd_job **job);
int fcd_beam_search_host_ptrs_begin(fcd_handle *h, const void *const *reads, const int64_t *rows, int64_t n_reads,
                                    int64_t N, int dtype, int64_t beam_size, float beam_cut_threshold,
                                    int collapse_repeats, int kernel, int want, fcd_job **job);
/* Tuning / tests: lanes (0 = default 3 or FCD_HOST_LANES; 1 = never pipeline), reads per chunk (0 = automatic),
 * and the input size from which fcd_*_host takes the pipeline (-1 = default: >= 128 reads and >= 16 MB). */
int fcd_set_host_pipeline(fcd_handle *h, int lanes, int64_t chunk_reads, int64_t min_bytes);
int fcd_job_chunks(const fcd_job *job, int64_t *chunk_reads, int *n_lanes);  /* number of chunks; -1 for NULL */
int fcd_job_next(fcd_job *job, fcd_chunk *out);
int fcd_job_end(fcd_job *job);

/* ---- host-side helpers shared with the language bindings ---- */
/* phred quality character code point for a probability (src/search.rs:31-36) */
uint32_t fcd_phred(float prob, float qscale, float qbias);

#ifdef __cplusplus
}
#endif
#endif /* FCD_H */
