// fcd_internal.h -- shared declarations of libfcd_hip.so (host side + kernel launchers).
// gfx950 / CDNA4 only.  No CUDA compatibility paths by design.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fcd.h"
#include "../../include/fcd_debug.h"

namespace fcd {

// Everything a search kernel needs to know about the input batch (device pointers).
struct BatchDesc {
    const float *post;
    const int64_t *lengths;  // nullable
    int64_t n_reads;
    int64_t T;
    int64_t stride_read, stride_t, stride_s, stride_n;
    int S;
    int N;
    int dtype;  // element type of `post`: 0 f32, 1 f16, 2 bf16 (strides are in elements of that type)
};

// Device-side output arrays (see fcd_result in include/fcd.h).
struct ResultDesc {
    uint8_t *labels;
    uint32_t *path;
    float *qual;
    uint32_t *out_len;
    int32_t *status;
    int64_t out_stride;
    uint32_t *ambiguous;  // nullable: per-read count of unpinned tie steps (beam searches only)
};

// n-best layout of the beam searches (fcd_*_nbest_*), read by the kernels only after the time loop.  n_best = 0: one
// row per read (every other entry point).  n_best > 0: labels / path / out_len of the ResultDesc and score have
// n_reads * n_best rows, hypothesis i of read r in row r * n_best + i; n_hyp, status and ambiguous stay per read.
// (The LAST member of the beam kernels' parameter blocks: the fields before it keep their kernel-argument offsets.)
struct NBestDesc {
    float *score;
    uint32_t *n_hyp;
    int64_t n_best;
};

// Beam-search sessions (fcd_beam_session_*): the saved search of every slot, read by the SES instantiations of the wave
// and generic kernels only -- state == nullptr everywhere else.  (The LAST member of the beam kernels' parameter blocks,
// behind NBestDesc: the fields before it keep their kernel-argument offsets.)
// Slot r's block of block_words i32 starts at state + r * block_words; its first kSesHeader words are
//   [0] beam length B  [1] alive  [2] status once failed  [3] [4] the two tie counters  [5] steps taken (t0)
//   [6] wave kernel: a bad CRF init waits for the slot's first non-empty push / generic kernel: nodes in the tree
// followed by the kernel's own form of the beam (beam_wave.hip, beam_generic.hip).
constexpr int kSesHeader = 8;
constexpr int kSesWaveWords = kSesHeader + 8 * 64;  // eight registers of each of the 64 lanes, verbatim
struct SessionDesc {
    int32_t *state;
    int64_t block_words;
    int count_amb;  // the session counts ties (fcd_result.ambiguous), whether or not this launch reports them
};
inline int64_t ses_generic_words(int64_t beam_size, int64_t N) { return kSesHeader + beam_size * (7 + (N - 1)); }

// Parameters of the 1D beam searches (search::beam_search / search::crf_beam_search).
struct BeamArgs {
    int beam_size;
    float thr;
    int collapse;
    int crf;
    const float *init;  // CRF only: [n_reads * init_stride]
    int64_t n_init;
    int64_t init_stride;
    int force_one_read_per_wave;  // wave kernel: skip the two-reads-per-wavefront variant
    // developer instrument (fcd_beam_search_profile_dev): per wavefront, shader cycles spent in each block
    // of the step, summed over the read -- [n_wavefronts][8] u32, nullable
    uint32_t *prof;
    int tie_order;  // FCD_TIE_PDQ178 / FCD_TIE_STABLE (include/fcd.h): order of equal probabilities above 20 candidates
};

// Per-chunk tree arena of the LDS-resident ("generic") beam kernel: one slab per read.
//   rec  : int4 {parent, time, label, depth} per node            (tree.rs LabelNode)
//   rows : NL int32 per node, child index or -1                  (tree.rs children: Vec2D<i32>)
struct GenericArena {
    int4 *rec;
    int32_t *rows;
    int64_t cap_nodes;  // nodes per read
};

// Tree arena of the register-resident ("wave") beam kernel.
//   rec  : i32 (parent + 1) << 3 | label per node; the creation time -- what `path` reports -- is the upper part
//          of the node id (wave kernel) or looked up in `first` (lane kernel, dense ids)
//   jmp  : i32 per node, written for nodes at depth % 64 == 0: next such ancestor (traceback)
//   rows : int4 per node (NL <= 4) or 8 x int32 (NL <= 6..7); entry = child | EVER bit, or -1
struct WaveArena {
    int32_t *rec;
    int32_t *jmp;
    int32_t *rows;
    int32_t *first;        // lane kernel: first[slab][t] = the read's node count when step t began
    int64_t first_stride;  // words per slab of `first`
    int64_t cap_nodes;
    int row_words;  // 4 or 8
    // retry pass of the lane kernel (one read per wavefront): only reads whose first-pass slab overflowed
    // (status FCD_ST_INTERNAL) run, in worst-case slabs; the counter says how many did
    int32_t *retry_counter;  // nullable
    // lane kernel, large jobs: the slabs (pairs of slabs at two reads per wavefront) come from a device-side pool,
    // taken when a wavefront starts and handed back after its traceback (slab_pool.h); null = slab i belongs to read i
    unsigned long long *pool;
};

size_t beam_generic_lds_bytes(int beam_size, int N, int tie_order);  // (the quicksort's list and scratch only under FCD_TIE_PDQ178 above 20 candidates)
hipError_t launch_beam_generic(const BatchDesc &in, int64_t read_begin, int64_t n_reads,
                               const BeamArgs &a, const GenericArena &arena, const ResultDesc &out,
                               hipStream_t stream, const NBestDesc &nb = NBestDesc{}, const SessionDesc &ses = SessionDesc{});

int beam_lane_reads_per_wave(int beam_size);  // of a first pass (a retry pass: one)
// wavefronts of the instantiation the current device holds at once: the size of a slab pool nobody ever waits for
int beam_lane_resident_waves(int beam_size, int N, int crf, bool first_pass, bool ambiguous, int tie_order,
                             bool nbest = false);
hipError_t slab_pool_init(unsigned long long *pool, int slabs, hipStream_t stream);  // `pool`: slab_pool::bytes(slabs) of device memory
bool beam_wave_supported(int beam_size, int N, int crf, int S);
// node ids of the wave kernel are (time step << shift) | index among the step's new nodes: slots per step = 1 << shift
int beam_wave_id_shift(int beam_size, int N, int force_one_read_per_wave);
hipError_t launch_beam_wave(const BatchDesc &in, int64_t read_begin, int64_t n_reads,
                            const BeamArgs &a, const WaveArena &arena, const ResultDesc &out,
                            hipStream_t stream, const NBestDesc &nb = NBestDesc{});
// the session instantiations of the wave kernel (beam_wave_session.hip): n_reads = the session's slots, from slot 0
hipError_t launch_beam_wave_session(const BatchDesc &in, int64_t n_reads, const BeamArgs &a, const WaveArena &arena,
                                    const ResultDesc &out, const SessionDesc &ses, hipStream_t stream);
// sessions: the root state of the listed slots (session.hip).  CRF: from init rows [n_slots][n_init], row j for slots[j]
hipError_t launch_session_restart(const SessionDesc &ses, const int64_t *slots, int64_t n_slots, bool wave, int beam_size,
                                  int N, int crf, int S, const float *init, int64_t n_init, hipStream_t stream);

// one beam entry per lane: beam_size <= 64, N <= 8 (CRF: N = 5, S a power of two >= 4); uses the wave arena layout
bool beam_lane_supported(int beam_size, int N, int crf, int S);
hipError_t launch_beam_lane(const BatchDesc &in, int64_t read_begin, int64_t n_reads,
                            const BeamArgs &a, const WaveArena &arena, const ResultDesc &out,
                            hipStream_t stream, const NBestDesc &nb = NBestDesc{});

hipError_t launch_viterbi(const BatchDesc &in, int collapse, const ResultDesc &out,
                          hipStream_t stream);

hipError_t launch_crf_greedy(const BatchDesc &in, const float *init, int64_t n_init,
                             int64_t init_stride, const ResultDesc &out, hipStream_t stream);

// A kernel launched with more than 64 KiB of dynamic LDS has to be opted in first; below that there is nothing to do.
inline hipError_t allow_dynamic_lds(const void *kernel, int bytes) {
#ifndef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: the LDS is host memory)
    if (bytes > 64 * 1024) return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
#endif
    return hipSuccess;
}

// The Viterbi search under a CRF model (fcd_crf_viterbi_search_* in include/fcd.h; crf_viterbi_kernel,
// crf_viterbi.hip).  crf_viterbi_unsupported: 0 supported, 1 N outside 2 .. 9, 2 S no multiple of N - 1, 3 S beyond the
// state word, 4 the state and candidate arrays beyond the LDS of a CU.  bp: crf_viterbi_read_bytes(T, S) bytes per read.
int crf_viterbi_unsupported(int64_t S, int64_t N);
size_t crf_viterbi_read_bytes(int64_t T, int64_t S);
hipError_t launch_crf_viterbi(const BatchDesc &in, const float *init, int64_t n_init, int64_t init_stride,
                              const ResultDesc &out, double *logp, unsigned char *bp, hipStream_t stream);

// CRF transition probabilities from raw scores (fcd_crf_transition_probs_* in include/fcd.h; crf_transitions_kernel,
// crf_transitions.hip).  `in` holds the scores; everything here is device memory.  crf_transitions_unsupported:
// 0 supported, 1 N outside 2 .. 9, 2 S no multiple of N - 1, 3 S beyond the state word, 4 the two rows of the backward
// vector and the store staging beyond the LDS of a CU.
struct TransitionsDesc {
    void *probs;          // f32 or f16 (dtype: kF32 / kF16); row t of read r at r * stride_read + t * stride_t, (S, N) dense
    int dtype;
    int layout;           // of the scores: FCD_LAYOUT_SOURCE / FCD_LAYOUT_DEST
    int64_t stride_read, stride_t;
    float *init;          // [n_reads * init_stride]
    int64_t init_stride;
    double *logz;         // [n_reads], nullable
    int32_t *status;      // [n_reads]
};
int crf_transitions_unsupported(int64_t S, int64_t N);
hipError_t launch_crf_transitions(const BatchDesc &in, const TransitionsDesc &out, hipStream_t stream);
// CRF edge marginals (fcd_crf_marginals_* in include/fcd.h; crf_marginals_kernel, crf_transitions.hip): the transition walk
// with out.probs the marginals' f32 buffer and out.init null, then the forward pass over that buffer in the same launch.
// emit [n_reads * emit_stride] is nullable.  The limits are crf_transitions_unsupported's.
hipError_t launch_crf_marginals(const BatchDesc &in, const TransitionsDesc &out, float *emit, int64_t emit_stride,
                                hipStream_t stream);

// duplex::beam_search (src/duplex.rs:443-650) launch arguments; all pointers are device memory.
struct DuplexArgs {
    const float *ln1, *ln2;  // log-space posteriors [pair][Tcap][N]
    int64_t T1cap, T2cap;
    const int64_t *len1, *len2;
    const uint64_t *env;
    int64_t env_stride;
    int N, beam_size;
    float thr_ln;
    int collapse, mode;
    int S, crf;                  // CRF: S transition states, init scores per pair
    const float *init1, *init2;
    int64_t n_init1, n_init2, init1_stride, init2_stride;
    int4 *meta;
    float *nmax;
    int32_t *rlo;
    int32_t *rows;
    float *vec;
    float *rootgap;
    int64_t cap_nodes;
    int Wcap;
    int staged;
    ResultDesc out;
    uint32_t *prof;  // developer instrument: [pair][8] cycle account, nullable
    int tie_order;   // FCD_TIE_PDQ178 / FCD_TIE_STABLE
    // slot-resident kernel (duplex_slots.hip): `meta` is the base of the arena, ONE slab of `pair_stride` bytes per pair
    // (meta | aux | rings of Wcap floats | NLp child ids per node | the root's T2cap + 1 floats), below 4 GiB each
    int4 *aux;
    int NLp;
    int64_t pair_stride;
};

size_t duplex_lds_bytes(int beam_size, int N, int Wmax, int S, int tie_order);
// duplex_slots.hip: beam_size * N <= 64, N <= 8, and the rings of every live node + the read-2 tile fit 64 KiB of LDS
bool duplex_slots_supported(int beam_size, int N, int S, int width, int tie_order);
size_t duplex_slots_pair_bytes(int64_t cap_nodes, int N, int ring_rows, int64_t T2cap);  // one pair's slab
int duplex_slots_ring_rows(int width);  // ring capacity for a widest envelope row of `width`
size_t duplex_slots_lds_bytes(int beam_size, int N, int S, int ring_rows, int tie_order);
hipError_t launch_duplex_slots(const DuplexArgs &a, int64_t pair_begin, int64_t n_pairs, hipStream_t stream);
hipError_t launch_ln_convert(const float *x, int dtype, int64_t n_reads, int64_t T, int S, int N, int64_t s_read,
                             int64_t s_t, int64_t s_s, int64_t s_n, float *out, int glibc235, hipStream_t stream);
hipError_t launch_env_width(const uint64_t *env, int64_t n_pairs, int64_t env_stride, int64_t T1cap,
                            int64_t T2cap, const int64_t *len1, const int64_t *len2, int *out,
                            hipStream_t stream);
hipError_t launch_duplex(const DuplexArgs &a, int64_t pair_begin, int64_t n_pairs,
                         hipStream_t stream);
// alignment-band estimator (envelope.hip); all pointers are device memory
struct EnvelopeArgs {
    const uint8_t *labels1, *labels2;  // [pair][stride] label indices of the two reads
    const uint32_t *path1, *path2;     // [pair][stride] emission times of those labels
    const uint32_t *len1, *len2;       // labels per read
    int64_t stride1, stride2;
    const int64_t *T1, *T2;            // nullable per-pair row counts
    int64_t T1cap, T2cap;
    int64_t L2cap;                     // most labels any read 2 of the batch holds (sizes the LDS rows)
    int64_t band;
    uint64_t *env;                     // [pair][env_stride][2]
    int64_t env_stride;
    uint64_t *dirs;                    // workspace: [pair][dirs_stride] decision ballots
    int64_t dirs_stride;
    int nchunk;                        // 64-column chunks per DP row
    int32_t *anchor;                   // workspace: [pair][T1cap + 1]
};
size_t envelope_lds_bytes(int64_t L2cap);
hipError_t launch_max_u32(const uint32_t *a, const uint32_t *b, int64_t n, uint32_t *out2, hipStream_t stream);
hipError_t launch_envelope(const EnvelopeArgs &a, int64_t pair_begin, int64_t n_pairs, hipStream_t stream);

// compact wire format of decoded results (pack.hip)
hipError_t launch_result_offsets(const uint32_t *len, int64_t n, int64_t stride, uint64_t *offsets, hipStream_t stream);
// (res.qual non-null: an f32 region follows the path region, 4-byte aligned -- host result chunks only)
hipError_t launch_pack(const ResultDesc &res, int64_t n, int path_bytes, const uint64_t *offsets, uint8_t *buf,
                       hipStream_t stream);
hipError_t launch_unpack(const uint8_t *buf, int64_t n, const uint64_t *offsets, const ResultDesc &out,
                         hipStream_t stream);
// every shard of a gathered buffer (world x stride bytes) at once; first = [world + 1] prefix sums of the
// per-rank read counts (device), offsets = workspace of n_total + world u64, *bad = 1 + shard on a bad header
hipError_t launch_unpack_gathered(const uint8_t *gathered, int64_t stride, int world, const int64_t *first,
                                  int64_t n_total, uint64_t *offsets, const ResultDesc &out, int32_t *bad,
                                  hipStream_t stream);

// CTC forward scoring of given labellings (ctc_score.hip; fcd_labellings in include/fcd.h); all pointers device memory
struct ScoreDesc {
    const uint8_t *labels;
    const uint32_t *len;
    const uint32_t *n_valid;  // nullable
    const uint32_t *path;     // nullable when band == 0
    int64_t n_hyp;
    int64_t stride;
};
// the most states a live window of such a call can hold, and whether the kernels hold it (LDS: 160 KiB per workgroup)
int64_t ctc_score_window_states(int64_t T, int64_t stride, int64_t band);
bool ctc_score_supported(int64_t T, int64_t stride, int64_t band);
hipError_t launch_ctc_score(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, double *logp,
                            hipStream_t stream);
// CTC forced alignment of given labellings (ctc_align.hip; fcd_alignment in include/fcd.h): what ctc_score supports.
// bp: ctc_align_row_bytes() of device memory per labelling of the launch (the back-pointers); logp must not be null.
struct AlignOut {
    uint32_t *start;
    uint32_t *count;
    float *qual;  // nullable
    double *logp;
};
size_t ctc_align_row_bytes(int64_t T, int64_t stride, int64_t band);
hipError_t launch_ctc_align(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, const AlignOut &out,
                            unsigned char *bp, hipStream_t stream);
// CTC forward-backward substitution posteriors of given labellings (ctc_posterior.hip; fcd_posterior in include/fcd.h).
// ctc_posterior_unsupported: 0 = the kernels hold the call; 1 = the widest window exceeds the 510 register-resident states,
// 2 = more than 8 labels, 3 = min(T, stride) beyond the 28480 labels whose LDS copy fits 64 KiB next to the tile.  alpha: ctc_posterior_row_bytes() of device memory per labelling of the launch (the stored
// forward rows); post: [labellings * stride * (N - 1)]; logp must not be null.
int ctc_posterior_unsupported(int64_t T, int64_t stride, int64_t band, int64_t N);
size_t ctc_posterior_row_bytes(int64_t T, int64_t stride, int64_t band);
hipError_t launch_ctc_posterior(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, float *post,
                                double *logp, unsigned char *alpha, hipStream_t stream);
// CTC deletion and insertion likelihoods of given labellings (ctc_posterior.hip; fcd_edits in include/fcd.h): the limits,
// the workspace and the forward launch of launch_ctc_posterior.  deletion: [labellings * stride], insertion:
// [labellings * (stride + 1) * (N - 1)]; logp must not be null.
hipError_t launch_ctc_edits(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, float *deletion,
                            float *insertion, double *logp, unsigned char *alpha, hipStream_t stream);
// The lattice of given labellings under a CRF model (crf_lattice.hip; fcd_crf_score_* / fcd_crf_align_* in include/fcd.h).
// crf_lattice_unsupported: 0 = the kernels hold the call; 1 = the window exceeds the 512 register-resident states,
// 2 = S beyond the 24-bit state word, 3 = the labelling's LDS copy (4 bytes per state) exceeds 64 KiB.
// bp: crf_align_row_bytes() of device memory per labelling of the launch; out.logp must not be null.
int64_t crf_lattice_window_states(int64_t T, int64_t stride, int64_t band);
int crf_lattice_unsupported(int64_t T, int64_t S, int64_t stride, int64_t band);
size_t crf_align_row_bytes(int64_t T, int64_t stride, int64_t band);
hipError_t launch_crf_score(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                            int64_t band, double *logp, hipStream_t stream);
hipError_t launch_crf_align(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                            int64_t band, const AlignOut &out, unsigned char *bp, hipStream_t stream);
// CRF forward-backward substitution posteriors of given labellings (crf_posterior.hip; fcd_crf_posterior_* in include/fcd.h),
// on top of crf_lattice_unsupported.  crf_posterior_unsupported: 0 = the kernels hold the call; 1 = the window exceeds the
// *max_states register-resident states of the chain's tier, 2 = more than 8 labels, 4 = S is no power of N - 1, 5 = a
// history beyond the tiers (m > 6 or m (N - 1) > 24).  *max_states: 512 where m (N - 1) <= 8 and N - 1 <= 4, 256 where
// m = 1 and N - 1 > 4, else 192.  alpha: crf_posterior_row_bytes() of device memory per labelling of the launch (the stored
// forward rows); post: [labellings * stride * (N - 1)]; logp must not be null.
int crf_posterior_unsupported(int64_t T, int64_t S, int64_t N, int64_t stride, int64_t band, int64_t *max_states);
size_t crf_posterior_row_bytes(int64_t T, int64_t S, int64_t N, int64_t stride, int64_t band);
hipError_t launch_crf_posterior(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                                int64_t band, float *post, double *logp, unsigned char *alpha, hipStream_t stream);
// CRF deletion and insertion likelihoods of the same labellings (crf_posterior.hip; fcd_crf_edits_* in include/fcd.h): the
// same kernels and workspace (crf_posterior_row_bytes), and crf_posterior_unsupported's limits: every instantiation carries
// the two walks.
hipError_t launch_crf_edits(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                            int64_t band, float *deletion, float *insertion, double *logp, unsigned char *alpha,
                            hipStream_t stream);
// CRF edge occupancies of the same labellings' own lattices (crf_posterior.hip; fcd_crf_occupancy_* in include/fcd.h), on top
// of crf_lattice_unsupported: crfp_fwd_kernel<K> and a fourth walk inside crfp_back_kernel<K, 2, 4>, K = 1, 2, 4, 8 as the
// score's.  crf_occupancy_unsupported: 0 = the kernels hold the call; 2 = more than 8 labels, 6 = the labelling's LDS copy
// plus the S * N accumulation row exceed the 160 KiB of a workgroup.  alpha: crf_occupancy_row_bytes() per labelling of the
// launch; out.occ: the first labelling's block; logp must not be null.
struct OccupancyDesc {
    float *occ;
    int64_t stride_row, stride_t;
    float scale;
    int accumulate;
};
int crf_occupancy_unsupported(int64_t T, int64_t S, int64_t N, int64_t stride);
size_t crf_occupancy_row_bytes(int64_t T, int64_t stride, int64_t band);
hipError_t launch_crf_occupancy(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                                int64_t band, const OccupancyDesc &out, double *logp, unsigned char *alpha, hipStream_t stream);
// The CRF forward sum and the occupancies for windows beyond 512 states (crf_posterior.hip; fcd_set_crf_lattice_wide in
// include/fcd.h): the window lives in LDS, J = ceil(states / 64) = 9 .. 64 states per lane, walked by loop bodies inside
// crfp_fwd_kernel<8> (sum only when alpha is null: the score) and crfp_back_kernel<8, 2, 4>.  A window within 512 states
// (crf_lattice_is_wide false) goes to launch_crf_score / launch_crf_occupancy unchanged.
// crf_lattice_wide_unsupported: 0 = the kernels hold the call; 1 = the window exceeds 4096 states, 2 = more than 8 labels,
// 3 = S beyond the state word, 4 = the labelling's copy, the tile, the window's three rows and (occupancy) the S * N row
// exceed the 160 KiB of a workgroup; *lds_bytes: what the widest launch takes (0 where 1 .. 3 answered first).
// alpha: crf_lattice_wide_row_bytes() per labelling of the launch -- stored_rows_bytes(T, J); logp must not be null.
bool crf_lattice_is_wide(int64_t T, int64_t stride, int64_t band);
int crf_lattice_wide_unsupported(int64_t T, int64_t S, int64_t N, int64_t stride, int64_t band, bool occupancy, size_t *lds_bytes);
size_t crf_lattice_wide_row_bytes(int64_t T, int64_t stride, int64_t band);
hipError_t launch_crf_score_wide(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                                 int64_t band, double *logp, hipStream_t stream);
hipError_t launch_crf_occupancy_wide(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                                     int64_t band, const OccupancyDesc &out, double *logp, unsigned char *alpha, hipStream_t stream);
// CTC label occupancies of the same labellings (ctc_posterior.hip; fcd_ctc_occupancy_* in include/fcd.h): post_fwd_kernel<K>
// and a second walk inside post_back_kernel<K, 8>.  The limits and the workspace are launch_ctc_posterior's
// (ctc_posterior_unsupported, ctc_posterior_row_bytes); out.occ: the first labelling's (T, N) block; logp must not be null.
hipError_t launch_ctc_occupancy(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, const OccupancyDesc &out,
                                double *logp, unsigned char *alpha, hipStream_t stream);
// The same occupancies for every labelling ctc_score takes (ctc_score.hip; fcd_set_ctc_occupancy_wide in include/fcd.h).  A
// window the registers hold goes to launch_ctc_occupancy unchanged (the same launches, the same bits); a wider one is two
// launches of score_lds_kernel: its forward walk storing its rows, then the backward walk in LDS.
// ctc_occupancy_wide_unsupported: 0 = the kernels hold the call; 2 = more than 8 labels, 3 = (register-resident windows)
// ctc_posterior_unsupported's 3, 4 = the window exceeds the 10240 states of 1024 work-items, 5 = the labelling's copy, the
// tile, the two alpha buffers and the reduction words exceed the 160 KiB of LDS.  alpha: ctc_occupancy_wide_row_bytes() per
// labelling of the launch -- T * (states + 1) * 4 bytes rounded up to 256 beyond the registers; logp must not be null.
int ctc_occupancy_wide_unsupported(int64_t T, int64_t stride, int64_t band, int64_t N);
size_t ctc_occupancy_wide_row_bytes(int64_t T, int64_t stride, int64_t band);
hipError_t launch_ctc_occupancy_wide(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, const OccupancyDesc &out,
                                     double *logp, unsigned char *alpha, hipStream_t stream);

hipError_t launch_logspace_probe(const float *a, const float *b, float *out_add, float *out_ln,
                                 int64_t n, int mode, hipStream_t stream);
hipError_t launch_glibc235_apply(int which, const float *x, float *y, int64_t n, hipStream_t stream);
hipError_t launch_logadd_chain(int n_chain, int mode, uint64_t *cycles, float *sink, hipStream_t stream);
hipError_t launch_logadd_sweep(int which, uint32_t first, uint32_t last, unsigned long long *counts, hipStream_t stream);
hipError_t launch_pdq178_probe(uint64_t *lists, int64_t n_lists, int64_t stride, const int32_t *lens, hipStream_t stream);
hipError_t launch_pdq178_coop_probe(uint64_t *lists, int64_t n_lists, int64_t stride, const int32_t *lens, int planes,
                                    int keep, hipStream_t stream);
hipError_t coop_prof_read(unsigned long long *out16, bool reset);  // developer instrument of the probe kernels
// the replay's std-form word (pdq178.h g_std_form) of each translation unit that holds a replay, on the current device
hipError_t beam_wave_set_pdq178_std_form(int bits);
hipError_t beam_lane_set_pdq178_std_form(int bits);
hipError_t beam_generic_set_pdq178_std_form(int bits);
hipError_t beam_wave_session_set_pdq178_std_form(int bits);
hipError_t tieorder_set_pdq178_std_form(int bits);
hipError_t lane_tie_prof_read(unsigned long long *out16, bool reset);  // ... of a -DFCD_LANE_TIE_PROF build of beam_lane.hip
// the tie order searches on this handle use (capi.hip)
int effective_tie_order(const fcd_handle *h);

// ---- host side of the four 1D searches (capi.hip, hostjob.hip) ----
enum class HostOp { Viterbi, Beam, CrfBeam, CrfGreedy };

struct HostCall {
    HostOp op;
    int collapse = 1;
    int64_t beam_size = 5;
    float thr = 0.0f;
    int kernel = FCD_KERNEL_AUTO;
    const float *init = nullptr;  // host pointer
    int64_t n_init = 0, init_stride = 0;
    int64_t n_best = 0;  // Beam / CrfBeam: > 0 = the n-best layout (fcd_*_nbest_host; never through the chunk pipeline)
};

// where one staged host call lives inside fcd_handle::stage (byte offsets)
struct HostStage {
    size_t o_in, o_len, o_init, o_lab, o_path, o_qual, o_olen, o_stat, o_amb, o_score, o_nhyp, used;
    size_t n_in, n_out, n_init, n_rows;  // n_rows: result rows (n_reads, or n_reads * n_best)
    int64_t B;
    bool want_amb, mirror;
};

int host_check(fcd_handle *h, const fcd_batch *in, const fcd_result *out, const HostCall &c);
int host_upload(fcd_handle *h, const fcd_batch *in, const fcd_result *shape, const HostCall &c, bool allow_mirror,
                HostStage *st, fcd_batch *din, fcd_result *dout);
int host_search(fcd_handle *h, const HostStage &st, const fcd_batch *din, const HostCall &c, const fcd_result *dout);
// (nb: the caller's score / n_hyp arrays of an n-best call)
int host_download(fcd_handle *h, const HostStage &st, const fcd_result &dout, const fcd_result *out,
                  const fcd_nbest *nb = nullptr);
// large host batches: chunks on internal lanes, upload || search || packed download (hostjob.hip)
bool host_job_wanted(fcd_handle *h, const fcd_batch *in, const HostCall &c);
int host_job_run_fixed(fcd_handle *h, const fcd_batch *in, const fcd_result *out, const HostCall &c);
void host_job_release_lanes(fcd_handle *h, bool destroy);

}  // namespace fcd

struct fcd_host_lane;

struct fcd_handle {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // ring of (start, stop) event pairs, one per search call, recorded on the launch stream
    static constexpr int kTimingRing = 256;
    std::vector<hipEvent_t> ev0, ev1;
    int64_t n_timed = 0;  // calls recorded since the last fcd_timing_reset
    int64_t ws_limit = 0;  // 0 = auto (half of the free device memory)
    int first_pass_div = 2;  // lane kernel, two-pass sizing: first-pass slabs hold 1/div of the worst case
    bool first_pass_div_pinned = false;  // set by fcd_debug_set_first_pass_divisor: no adaptation
    // grow-only device workspace (tree arenas, staging for *_host calls)
    void *arena = nullptr;
    size_t arena_bytes = 0;
    size_t arena_region = 0;  // fcd_set_overlap: internal stream k's calls use the arena from k * arena_region on
    void *stage = nullptr;
    size_t stage_bytes = 0;
    void *pin = nullptr;  // page-locked host mirror of `stage` for small *_host calls (one DMA each way)
    size_t pin_bytes = 0;
    void *lnbuf = nullptr;  // duplex: log-space copies of both reads + scalars
    size_t lnbuf_bytes = 0;
    size_t lnbuf_region = 0;  // (fcd_set_overlap: as arena_region)
    // wide-beam kernel, large jobs: slabs handed out on the device (slab_pool.h).  An allocation of its own: calls in
    // flight on the overlap streams keep using it while other entry points size `arena` for themselves
    void *pool_arena = nullptr;
    size_t pool_arena_bytes = 0;
    void *pool_ctl = nullptr;  // the two rings: first-pass (pairs of) slabs, worst-case slabs of the retry pass
    size_t pool_ctl_bytes = 0;
    struct PoolGeom {
        int64_t cap_nodes = 0, cap_worst = 0, first_stride = 0;
        int rpw = 0, row_words = 0, p1 = 0, p2 = 0;
    } pool_geom;
    // fcd_set_overlap: the beam searches go round-robin to internal streams, ordered after the handle's stream as it stood
    // at the call and not after one another; what each stream still runs writes the output ranges listed here.  Only
    // capi.hip's CallScope and the handle-control entry points touch these (and `arena`, `lnbuf`).
    static constexpr int kMaxOverlap = 8;
    int overlap_n = 0;
    hipStream_t ov_stream[kMaxOverlap] = {};
    hipEvent_t ov_last[kMaxOverlap] = {};  // recorded behind the last call of the stream
    bool ov_used[kMaxOverlap] = {};
    hipEvent_t ov_fork = nullptr;
    uint64_t ov_seq = 0;
    int ov_last_slot = -1;  // the internal stream the latest overlapping call went to
    struct Range { uintptr_t lo, hi; };
    static constexpr int kMaxRanges = 10;  // arrays one call reads or writes (fcd_unpack_gathered_dev: 10)
    // the calls each internal stream has not finished yet, oldest first: what they write, and an event behind each (so that
    // a stream that never idles does not accumulate ranges: finished calls are dropped from the front)
    struct Flight {
        hipEvent_t done = nullptr;
        Range r[kMaxRanges];
        int n = 0;
    };
    std::deque<Flight> ov_flights[kMaxOverlap];
    std::vector<hipEvent_t> ov_event_pool;
    void *retry_counter = nullptr;  // lane kernel, two-pass sizing: overflow counters of the retry pass, one word per stream
    size_t retry_counter_bytes = 0;
    void *retry_host = nullptr;     // page-locked word the first retry round's overflow count is copied to, read one call late
    hipEvent_t retry_ev = nullptr;  // ... recorded behind that copy
    bool retry_pending = false;
    int64_t retry_n = 0;            // reads of the chunk the pending count belongs to
    // chunk lanes of the pipelined host path (hostjob.hip): sub-handles with their own stream and workspace
    std::vector<fcd_host_lane *> lanes;
    bool job_active = false;  // a host job owns the lanes from begin to end
    int live_sessions = 0;    // fcd_beam_session_create .. _destroy
    bool occ_wide = false;    // fcd_set_ctc_occupancy_wide: fcd_ctc_occupancy_* takes windows beyond 510 states
    bool crf_wide = false;    // fcd_set_crf_lattice_wide: fcd_crf_score_* and fcd_crf_occupancy_* take windows beyond 512 states
    int64_t align_ws_cap = 0; // fcd_debug_set_align_workspace_cap: back-pointer bytes one launch of fcd_ctc_align_* may take, 0 = default
    bool is_lane = false;
    uint32_t *duplex_prof = nullptr;  // fcd_debug_set_duplex_profile
    int duplex_kernel = 0;            // fcd_debug_set_duplex_kernel: 0 automatic, 1 the any-shape kernel (duplex.hip), 2 the slot-resident one
    int tie_order = FCD_TIE_DEFAULT;  // fcd_set_tie_order; FCD_TIE_DEFAULT = follow the process default
    int pipe_lanes = 0;          // fcd_set_host_pipeline: 0 = default (FCD_HOST_LANES or 4)
    int64_t pipe_chunk = 0;      // reads per chunk, 0 = automatic
    int64_t pipe_min_bytes = -1; // fcd_*_host batches of at least this many input bytes take the pipeline; -1 = default
    std::string err;
    std::recursive_mutex mu;  // a *_host call holds it from staging to copy-back, the *_dev call inside re-enters
};
