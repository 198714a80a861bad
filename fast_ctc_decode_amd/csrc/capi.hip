// capi.hip -- the C ABI of libfcd_hip.so (include/fcd.h): argument checking, workspace and
// chunking, stream/event plumbing, host staging for the *_host entry points.
#include <stdio.h>
#include <math.h>
#include <string.h>

#include <stdlib.h>

#include <algorithm>
#include <functional>
#include <atomic>
#include <vector>

#include "fcd_internal.h"
#include "glibc235_math.h"
#include "slab_pool.h"

using namespace fcd;

namespace {

// process default of the prune's tie order (include/fcd.h, FCD_TIE_*): the environment at load time, then
// fcd_set_default_tie_order
int tie_order_from_env() {
    const char *e = getenv("FCD_TIE_ORDER");
    if (!e || !*e) return FCD_TIE_PDQ178;
    if (!strcmp(e, "stable") || !strcmp(e, "STABLE") || !strcmp(e, "1")) return FCD_TIE_STABLE;
    if (!strcmp(e, "pdq178") || !strcmp(e, "PDQ178") || !strcmp(e, "2")) return FCD_TIE_PDQ178;
    // a typo must not silently select the other order
    fprintf(stderr, "fast_ctc_decode (fcd): FCD_TIE_ORDER=\"%s\" is neither \"pdq178\" nor \"stable\"; using pdq178\n", e);
    return FCD_TIE_PDQ178;
}
std::atomic<int> g_tie_order{tie_order_from_env()};

// FCD_PDQ178_STD_FORM (include/fcd.h): which form of the two routines std changed in 2023 the quicksort replay follows --
// a process-wide word, copied to every device a handle is created on (csrc/pdq178.h g_std_form)
int pdq178_std_form_from_env() {
    const char *e = getenv("FCD_PDQ178_STD_FORM");
    if (!e || !*e) return 0;
    if (e[0] >= '0' && e[0] <= '3' && !e[1]) {
        // (said once, so that nobody compares a 1-D search under form 3 with a duplex search and wonders)
        if (e[0] != '0')
            fprintf(stderr, "fast_ctc_decode (fcd): FCD_PDQ178_STD_FORM=%s applies to the 1-D searches; the duplex searches replay "
                            "form 0 only (csrc/pdq178.h)\n", e);
        return e[0] - '0';
    }
    fprintf(stderr, "fast_ctc_decode (fcd): FCD_PDQ178_STD_FORM=\"%s\" is not 0, 1, 2 or 3; using 0\n", e);
    return 0;
}
std::atomic<int> g_pdq178_std_form{pdq178_std_form_from_env()};

// (on the current device)
hipError_t apply_pdq178_std_form(int bits) {
    hipError_t e = beam_wave_set_pdq178_std_form(bits);
    if (e == hipSuccess) e = beam_lane_set_pdq178_std_form(bits);
    if (e == hipSuccess) e = beam_generic_set_pdq178_std_form(bits);
    if (e == hipSuccess) e = beam_wave_session_set_pdq178_std_form(bits);
    if (e == hipSuccess) e = tieorder_set_pdq178_std_form(bits);
    return e;
}

constexpr int kRetrySlabs = 256;  // lane kernel, two-pass sizing: worst-case slabs of the retry pass (its wavefronts wait for one)

#define FCD_HIP(h, expr)                                                          \
    do {                                                                          \
        hipError_t e__ = (expr);                                                  \
        if (e__ != hipSuccess) {                                                  \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e__);        \
            return FCD_E_HIP;                                                     \
        }                                                                         \
    } while (0)

// Binds the calling thread to the handle's device for the duration of an entry point and puts the previous
// device back afterwards: a caller that works on several GPUs (torch) must not find its current device changed.
struct DeviceGuard {
    int prev = -1;
    hipError_t err;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        err = prev == dev ? hipSuccess : hipSetDevice(dev);
        if (prev == dev) prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
#define FCD_DEVICE(h)                \
    DeviceGuard dev_guard__((h)->device); \
    FCD_HIP(h, dev_guard__.err)

int fail(fcd_handle *h, int code, const char *msg) {
    if (h) h->err = msg;
    return code;
}

int ensure(fcd_handle *h, void **buf, size_t *have, size_t need) {
    if (*have >= need) return FCD_OK;
    if (*buf) {
        // work enqueued earlier -- on the current stream or on one set before the last fcd_set_stream -- may
        // still use the buffer: hipFree waits for the whole device, but be explicit about both streams
        FCD_HIP(h, hipStreamSynchronize(h->stream));
        if (h->own_stream && h->own_stream != h->stream) FCD_HIP(h, hipStreamSynchronize(h->own_stream));
        FCD_HIP(h, hipFree(*buf));
        *buf = nullptr;
        *have = 0;
    }
    hipError_t e = hipMalloc(buf, need);
    if (e != hipSuccess) {
        *buf = nullptr;
        h->err = std::string("hipMalloc of workspace failed: ") + hipGetErrorString(e);
        return FCD_E_NOMEM;
    }
    *have = need;
    return FCD_OK;
}

int check_batch(fcd_handle *h, const fcd_batch *in, bool crf) {
    if (!h) return FCD_E_INVALID;
    if (!in) return fail(h, FCD_E_INVALID, "null batch");
    if (in->n_reads < 0 || in->T < 0 || in->N < 1) return fail(h, FCD_E_INVALID, "negative size");
    if (in->n_reads > 0 && in->T > 0 && !in->post) return fail(h, FCD_E_INVALID, "null post");
    if (in->N > 256) return fail(h, FCD_E_UNSUPPORTED, "alphabets above 256 labels are unsupported (u8 labels)");
    if (in->T >= (1ll << 28)) return fail(h, FCD_E_UNSUPPORTED, "T must be < 2^28");
    if (in->dtype != FCD_DTYPE_F32 && in->dtype != FCD_DTYPE_F16 && in->dtype != FCD_DTYPE_BF16)
        return fail(h, FCD_E_INVALID, "unknown posterior dtype");
    if (crf && in->S < 1) return fail(h, FCD_E_INVALID, "S must be >= 1");
    return FCD_OK;
}

int check_result(fcd_handle *h, const fcd_batch *in, const fcd_result *out, bool need_status) {
    if (!out) return fail(h, FCD_E_INVALID, "null result");
    if (in->n_reads == 0) return FCD_OK;
    if (!out->labels || !out->out_len) return fail(h, FCD_E_INVALID, "null labels/out_len");
    if (need_status && !out->status) return fail(h, FCD_E_INVALID, "null status");
    if (out->out_stride < in->T) return fail(h, FCD_E_INVALID, "out_stride must be >= T");
    return FCD_OK;
}

// the n-best form (fcd_*_nbest_*): `out` has n_reads * n_best rows, `nb` the scores and hypothesis counts
int check_result_nbest(fcd_handle *h, const fcd_batch *in, const fcd_result *out, const fcd_nbest *nb, int64_t beam_size) {
    if (!nb) return fail(h, FCD_E_INVALID, "null n-best description");
    if (nb->n_best < 1 || nb->n_best > beam_size) return fail(h, FCD_E_INVALID, "n_best must be in 1 .. beam_size");
    int rc = check_result(h, in, out, true);
    if (rc) return rc;
    if (in->n_reads > 0 && (!nb->score || !nb->n_hyp)) return fail(h, FCD_E_INVALID, "null score/n_hyp");
    return FCD_OK;
}

BatchDesc to_desc(const fcd_batch *in, bool crf) {
    BatchDesc d;
    d.post = static_cast<const float *>(in->post);  // (typed by `dtype`; the kernels convert on load)
    d.lengths = in->lengths;
    d.n_reads = in->n_reads;
    d.T = in->T;
    d.stride_read = in->stride_read;
    d.stride_t = in->stride_t;
    d.stride_s = crf ? in->stride_s : 0;
    d.stride_n = in->stride_n;
    d.S = crf ? (int)in->S : 1;
    d.N = (int)in->N;
    d.dtype = in->dtype;
    return d;
}

ResultDesc to_desc(const fcd_result *o) {
    return ResultDesc{o->labels, o->path, o->qual, o->out_len, o->status, o->out_stride, o->ambiguous};
}

int64_t workspace_budget(fcd_handle *h) {
    if (h->ws_limit > 0) return h->ws_limit;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 8ll << 30;
    return (int64_t)((free_b + h->arena_bytes + h->pool_arena_bytes) / 2);
}

// ---- fcd_set_overlap: wide-beam calls on internal streams ----
// every internal stream's work is finished (host wait)
int overlap_drain(fcd_handle *h) {
    for (int s = 0; s < fcd_handle::kMaxOverlap; ++s) {
        if (!h->ov_stream[s]) continue;
        FCD_HIP(h, hipStreamSynchronize(h->ov_stream[s]));
        for (fcd_handle::Flight &f : h->ov_flights[s]) h->ov_event_pool.push_back(f.done);
        h->ov_flights[s].clear();
        h->ov_used[s] = false;
    }
    return FCD_OK;
}

// `stream` waits for every call enqueued on the internal streams so far
int overlap_join(fcd_handle *h, hipStream_t stream) {
    for (int s = 0; s < fcd_handle::kMaxOverlap; ++s)
        if (h->ov_stream[s] && h->ov_used[s]) FCD_HIP(h, hipStreamWaitEvent(stream, h->ov_last[s], 0));
    return FCD_OK;
}

// The stream, ordering, workspace and timing of one *_dev entry point; every entry point that enqueues work goes through
// one, in this order:
//   add()     the arrays the call reads or writes (result arrays, offsets: what an overlapping call may be writing)
//   begin()   the stream: the handle's, or -- fcd_set_overlap, a call that may overlap -- the next internal stream, behind
//             the handle's stream as it stands now.  Then ONE ordering rule: the stream waits for every overlapping call in
//             flight that writes any of the add()ed arrays.  An exclusive call -- one that takes `arena` / `lnbuf` from
//             their start -- waits for every call in flight instead (they hold regions of both).
//   arena() / lnbuf()  workspace, only after begin(): an overlapping call's region of the buffer (one per internal
//             stream), or the whole buffer for an exclusive call.  Growing a buffer drains the internal streams first.
//   time()    starts the call's timing (fcd_last_kernel_ms) on its stream; finish() stops it.
//   finish()  an overlapping call counts as in flight from here on: its stream, the arrays it writes, an event behind it.
//             Every error return after begin() records it too (the destructor): whatever reached the internal stream.
class CallScope {
  public:
    hipStream_t stream;
    int slot = -1;  // internal stream of an overlapping call, -1: the handle's stream

    explicit CallScope(fcd_handle *h) : stream(h->stream), h_(h) {}
    CallScope(const CallScope &) = delete;
    CallScope &operator=(const CallScope &) = delete;
    ~CallScope() {
        if (slot < 0 || finished_) return;
        const std::string err = h_->err;  // (the error the call returns stays the one reported)
        (void)record();
        h_->err = err;
    }

    void add(const void *ptr, size_t bytes) {
        if (ptr && bytes && f_.n < fcd_handle::kMaxRanges)
            f_.r[f_.n++] = {reinterpret_cast<uintptr_t>(ptr), reinterpret_cast<uintptr_t>(ptr) + bytes};
    }
    void add(const ResultDesc &o, int64_t n_reads, const NBestDesc &nb = NBestDesc{}) {
        const size_t n_rows = (size_t)n_reads * (size_t)(nb.n_best > 0 ? nb.n_best : 1);  // (n-best: n_best rows per read)
        const size_t rows = n_rows * (size_t)o.out_stride;
        add(o.labels, rows);
        add(o.path, rows * 4);
        add(o.qual, rows * 4);
        add(o.out_len, n_rows * 4);
        add(o.status, (size_t)n_reads * 4);
        add(o.ambiguous, (size_t)n_reads * 8);
        add(nb.score, n_rows * 4);
        add(nb.n_hyp, (size_t)n_reads * 4);
    }

    int begin(bool may_overlap, bool exclusive) {
        fcd_handle *h = h_;
        if (may_overlap && h->overlap_n >= 2) {
            n_ = std::min(h->overlap_n, (int)fcd_handle::kMaxOverlap);
            if (!h->ov_fork) FCD_HIP(h, hipEventCreateWithFlags(&h->ov_fork, hipEventDisableTiming));
            for (int s = 0; s < n_; ++s) {
                if (h->ov_stream[s]) continue;
                // The internal streams are created in the HIGH priority class: the runtime hands out the hardware queues of
                // a class separately, so they get queues of their own whatever the process's other streams occupy (normal
                // streams beyond GPU_MAX_HW_QUEUES = 4 share queues, and kernels that share a queue run one after the other:
                // 262 k reads/s instead of 320 k on BASELINE config 3, profiles/r06v_*).  FCD_OVERLAP_PRIORITY=normal|low: A/B.
                const char *pr = getenv("FCD_OVERLAP_PRIORITY");
                int least = 0, greatest = 0;
                const bool ranged = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess;
                if (ranged && (!pr || !strcmp(pr, "high") || !strcmp(pr, "low")))
                    FCD_HIP(h, hipStreamCreateWithPriority(&h->ov_stream[s], hipStreamNonBlocking, (pr && !strcmp(pr, "low")) ? least : greatest));
                else
                    FCD_HIP(h, hipStreamCreateWithFlags(&h->ov_stream[s], hipStreamNonBlocking));
                FCD_HIP(h, hipEventCreateWithFlags(&h->ov_last[s], hipEventDisableTiming));
            }
            const int s = (int)(h->ov_seq % (uint64_t)n_);
            FCD_HIP(h, hipEventRecord(h->ov_fork, h->stream));
            FCD_HIP(h, hipStreamWaitEvent(h->ov_stream[s], h->ov_fork, 0));
            slot = s;
            stream = h->ov_stream[s];
        } else if (exclusive) {
            exclusive_ = true;
            return overlap_join(h, stream);
        }
        for (int s = 0; s < fcd_handle::kMaxOverlap; ++s) {
            if (!h->ov_stream[s] || !h->ov_used[s]) continue;
            std::deque<fcd_handle::Flight> &fl = h->ov_flights[s];
            while (!fl.empty() && hipEventQuery(fl.front().done) == hipSuccess) {  // finished calls go
                h->ov_event_pool.push_back(fl.front().done);
                fl.pop_front();
            }
            if (fl.empty()) {  // nothing in flight there any more
                h->ov_used[s] = false;
                continue;
            }
            if (s == slot) continue;  // (stream order)
            // the YOUNGEST call in flight there that writes any of these arrays: the stream runs them in order
            hipEvent_t wait_for = nullptr;
            for (const fcd_handle::Flight &f : fl) {
                bool clash = false;
                for (int i = 0; i < f.n && !clash; ++i)
                    for (int k = 0; k < f_.n && !clash; ++k) clash = f.r[i].lo < f_.r[k].hi && f_.r[k].lo < f.r[i].hi;
                if (clash) wait_for = f.done;
            }
            if (wait_for) FCD_HIP(h, hipStreamWaitEvent(stream, wait_for, 0));
        }
        return FCD_OK;
    }

    int regions() const { return slot >= 0 ? n_ : 1; }  // how many calls share a workspace buffer
    int arena(size_t need, char **out) { return region(&h_->arena, &h_->arena_bytes, &h_->arena_region, need, out); }
    int lnbuf(size_t need, char **out) { return region(&h_->lnbuf, &h_->lnbuf_bytes, &h_->lnbuf_region, need, out); }

    void time() {
        fcd_handle *h = h_;
        timer_ = (int)(h->n_timed % fcd_handle::kTimingRing);
        if ((int)h->ev0.size() <= timer_) {
            hipEvent_t a = nullptr, b = nullptr;
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            h->ev0.push_back(a);
            h->ev1.push_back(b);
        }
        (void)hipEventRecord(h->ev0[timer_], stream);
    }

    int finish() {
        finished_ = true;
        if (timer_ >= 0) {
            (void)hipEventRecord(h_->ev1[timer_], stream);
            h_->n_timed++;
        }
        return slot >= 0 ? record() : FCD_OK;
    }

  private:
    fcd_handle *h_;
    int n_ = 1;  // internal streams in use (an overlapping call)
    bool exclusive_ = false, finished_ = false;
    int timer_ = -1;
    fcd_handle::Flight f_;  // the add()ed arrays; `done` once recorded

    int region(void **buf, size_t *bytes, size_t *region_bytes, size_t need, char **out) {
        if (slot < 0) {
            if (!exclusive_) return fail(h_, FCD_E_INVALID, "internal error: workspace taken outside an exclusive call");
            int rc = ensure(h_, buf, bytes, need);
            if (rc) return rc;
            *out = static_cast<char *>(*buf);
            return FCD_OK;
        }
        need = (need + 255) & ~(size_t)255;
        if (need > *region_bytes || *bytes < (size_t)n_ * *region_bytes) {
            int rc = overlap_drain(h_);  // (calls in flight count on the old regions)
            if (rc) return rc;
            rc = ensure(h_, buf, bytes, (size_t)n_ * need);
            if (rc) return rc;
            *region_bytes = need;
        }
        *out = static_cast<char *>(*buf) + (size_t)slot * *region_bytes;
        return FCD_OK;
    }

    int record() {
        fcd_handle *h = h_;
        FCD_HIP(h, hipEventRecord(h->ov_last[slot], stream));
        if (!h->ov_event_pool.empty()) {
            f_.done = h->ov_event_pool.back();
            h->ov_event_pool.pop_back();
        } else {
            FCD_HIP(h, hipEventCreateWithFlags(&f_.done, hipEventDisableTiming));
        }
        FCD_HIP(h, hipEventRecord(f_.done, stream));
        h->ov_flights[slot].push_back(f_);
        h->ov_used[slot] = true;
        h->ov_last_slot = slot;
        h->ov_seq++;
        return FCD_OK;
    }
};

// Shared driver of search::beam_search and search::crf_beam_search on device buffers.  nb (nullable): the n-best
// layout of fcd_*_nbest_dev -- the same kernels, chunking and retry, with n_best result rows per read.
int beam_dev(fcd_handle *h, const fcd_batch *in, const BeamArgs &a, int kernel,
             const fcd_result *out, const fcd_nbest *nb = nullptr) {
    const bool crf = a.crf != 0;
    int rc = check_batch(h, in, crf);
    if (rc) return rc;
    rc = nb ? check_result_nbest(h, in, out, nb, a.beam_size) : check_result(h, in, out, true);
    if (rc) return rc;
    if (a.beam_size < 1) return fail(h, FCD_E_INVALID, "beam_size cannot be 0");
    if (in->N < 2) return fail(h, FCD_E_UNSUPPORTED, "alphabet needs at least one label besides the blank");
    if (in->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);

    const BatchDesc d = to_desc(in, crf);
    const ResultDesc o = to_desc(out);
    const NBestDesc nbd = nb ? NBestDesc{nb->score, nb->n_hyp, nb->n_best} : NBestDesc{};
    const int N = d.N, NL = N - 1;
    int64_t beam = a.beam_size;
    BeamArgs args = a;
    args.tie_order = effective_tie_order(h);

    bool use_wave = false;
    if (kernel == FCD_KERNEL_WAVE || kernel == FCD_KERNEL_WAVE1) {
        if (!beam_wave_supported((int)std::min<int64_t>(beam, 1 << 20), N, a.crf, d.S))
            return fail(h, FCD_E_UNSUPPORTED, "wave kernel: needs beam_size <= 8 and N <= 7, or beam_size <= 12 and N <= 5 (CRF: N = 5, S a power of two >= 4)");
        use_wave = true;
    } else if (kernel == FCD_KERNEL_AUTO) {
        use_wave = beam_wave_supported((int)std::min<int64_t>(beam, 1 << 20), N, a.crf, d.S);
    }
    // the wave kernel packs node ids -- (time step << shift) | index among the step's new nodes -- into 25 bits
    const int wave_shift = use_wave ? beam_wave_id_shift((int)std::min<int64_t>(beam, 1 << 20), N, kernel == FCD_KERNEL_WAVE1) : 0;
    if (use_wave && ((d.T << wave_shift) + 16 >= (1ll << 25))) {
        if (kernel != FCD_KERNEL_AUTO) return fail(h, FCD_E_UNSUPPORTED, "wave kernel: T too large");
        use_wave = false;
    }
    args.force_one_read_per_wave = kernel == FCD_KERNEL_WAVE1 ? 1 : 0;
    // wide beams: one beam entry per lane (node ids in 23 bits)
    bool use_lane = false;
    if (kernel == FCD_KERNEL_LANE || (kernel == FCD_KERNEL_AUTO && !use_wave)) {
        const bool ok = beam_lane_supported((int)std::min<int64_t>(beam, 1 << 20), N, a.crf, d.S) &&
                        d.T < (1ll << 26) && d.T * beam * NL + 16 < (1ll << 23);
        if (kernel == FCD_KERNEL_LANE && !ok)
            return fail(h, FCD_E_UNSUPPORTED, "lane kernel: needs beam_size <= 64, N <= 8 (CRF: N = 5, S a power of two >= 4), T * beam_size * (N-1) < 2^23");
        use_lane = ok;
    }

    // Worst-case tree size per read: every step every beam entry creates NL nodes
    // (tree.rs:125 add_node is only called from the expansion loop, search.rs:200-239).
    const int64_t T = std::max<int64_t>(d.T, 1);
    int64_t cap_nodes;
    size_t per_read;
    if (use_wave || use_lane) {
        // (wave kernel: one block of 1 << shift ids per time step, see beam_wave.hip; its records are 4 bytes)
        cap_nodes = use_wave ? ((T << wave_shift) + 8 + 3) & ~3ll
                             : (T * std::min<int64_t>(beam, 64) * NL + 8 + 3) & ~3ll;  // rows stay 16-B aligned
        const int row_words = NL <= 4 ? 4 : 8;
        per_read = (size_t)cap_nodes * (4 + 4 + row_words * 4);
    } else {
        if (beam > (1 << 16)) return fail(h, FCD_E_UNSUPPORTED, "beam_size above 65536");
        if (beam_generic_lds_bytes((int)beam, N, args.tie_order) > 64 * 1024)
            return fail(h, FCD_E_UNSUPPORTED, beam_generic_lds_bytes((int)beam, N, FCD_TIE_STABLE) > 64 * 1024
                                                  ? "beam_size * alphabet too large for the LDS-resident kernel"
                                                  : "beam_size * alphabet too large for the LDS-resident kernel under FCD_TIE_PDQ178 (the "
                                                    "quicksort's list needs LDS too: it fits under FCD_TIE_STABLE)");
        cap_nodes = T * beam * NL + 8;
        if (cap_nodes >= (1ll << 30)) return fail(h, FCD_E_UNSUPPORTED, "tree arena above 2^30 nodes per read");
        per_read = (size_t)cap_nodes * (sizeof(int4) + (size_t)NL * 4);
    }
    args.beam_size = (int)beam;
    const int64_t budget = workspace_budget(h);
    // Wide beams, large jobs: the worst case (every entry creates every child at every step) is about three
    // times what trees actually grow to (172 k of 512 k nodes per read at beam 32) and
    // would reserve 117 GB for BASELINE config 3's 8192 reads.  The lane kernel therefore runs in slabs of HALF
    // the worst case; a read that outgrows its slab is stopped (FCD_ST_INTERNAL) and decoded again by a retry
    // pass in worst-case slabs (stream order: the first pass has finished, results are already traced back).  The
    // retry pass is enqueued unconditionally (see below): the entry point never waits for the device.  Used only
    // when the worst-case arena would exceed 8 GiB (or the workspace limit) -- and then the slabs of both passes are
    // handed out on the device (slab_pool.h), as many as the chip holds wavefronts, whatever the size of the job.
    // A job in which more than a quarter of the reads overflow (dense posteriors: nearly every extension passes
    // the cut) makes this handle size later jobs for the worst case straight away -- one job late.
    // both register kernels keep 4-byte records (parent, label); the creation time is the upper part of the id
    // (wave kernel) or comes from the lane kernel's per-step table of first ids: T + 1 more words per slab
    const size_t rec_bytes = 4;
    const size_t node_bytes = (use_wave || use_lane) ? rec_bytes + 4 + (NL <= 4 ? 4 : 8) * 4 : 0;
    const int64_t first_stride = use_lane ? ((T + 1 + 3) & ~3ll) : 0;
    const size_t first_bytes = (size_t)first_stride * 4;
    if (use_lane) per_read += first_bytes;
    const size_t worst_total = ((size_t)cap_nodes * node_bytes + first_bytes) * (size_t)d.n_reads;
    const bool two_pass = use_lane && (worst_total > ((size_t)8 << 30) || (int64_t)worst_total > budget);
    const int64_t cap_worst = cap_nodes;
    const size_t worst_read = (size_t)cap_worst * node_bytes + first_bytes;
    auto wave_arena = [&](char *base, int64_t slabs, int64_t cap) {
        WaveArena ar{};
        ar.cap_nodes = cap;
        ar.row_words = NL <= 4 ? 4 : 8;
        ar.rec = reinterpret_cast<int32_t *>(base);
        ar.jmp = reinterpret_cast<int32_t *>(base + (size_t)slabs * cap * rec_bytes);
        ar.rows = reinterpret_cast<int32_t *>(base + (size_t)slabs * cap * (rec_bytes + 4));
        ar.first = reinterpret_cast<int32_t *>(base + (size_t)slabs * cap * node_bytes);
        ar.first_stride = first_stride;
        return ar;
    };
    CallScope sc(h);
    sc.add(o, d.n_reads, nbd);
    if (two_pass) {
        // ---- slabs from the device-side pool (slab_pool.h): the arena is sized by what the chip holds at once, one
        // launch takes the whole job, and calls on the overlap streams share it ----
        if (h->retry_pending && hipEventQuery(h->retry_ev) == hipSuccess) {
            // the overflow count of an earlier job has arrived: a job in which more than a quarter of the reads outgrew
            // their first-pass slabs makes this handle size later jobs for the worst case straight away
            const int64_t overflowed = *reinterpret_cast<volatile int32_t *>(h->retry_host);
            if (!h->first_pass_div_pinned && overflowed * 4 > h->retry_n) h->first_pass_div = 1;
            h->retry_pending = false;
        }
        cap_nodes = (cap_worst / std::max(h->first_pass_div, 1) + 63) & ~63ll;
        if (cap_nodes > cap_worst) cap_nodes = cap_worst;
        const bool retry_needed = cap_nodes < cap_worst;  // (divisor 1: the first pass IS the worst case)
        const int rpw = beam_lane_reads_per_wave((int)beam);
        const size_t wave_bytes = (size_t)rpw * ((size_t)cap_nodes * node_bytes + first_bytes);
        const int64_t waves = (d.n_reads + rpw - 1) / rpw;
        const bool amb = o.ambiguous != nullptr;
        int64_t p1_want = std::min<int64_t>(slab_pool::kMaxSlabs, beam_lane_resident_waves((int)beam, N, a.crf, true, amb, args.tie_order, nb != nullptr));
        if (h->overlap_n < 2) p1_want = std::min<int64_t>(p1_want, waves);  // (overlapping calls: whatever the chip holds)
        // the retry pass: a few worst-case slabs however small the job -- never less than one: a read that overflowed
        // must be decodable -- and no more than a quarter of the workspace limit
        int64_t p2 = 0;
        if (retry_needed) {
            p2 = std::min<int64_t>(std::min<int64_t>(d.n_reads, kRetrySlabs),
                                   beam_lane_resident_waves((int)beam, N, a.crf, false, amb, args.tie_order, nb != nullptr));
            p2 = std::max<int64_t>(1, std::min<int64_t>(p2, budget / 4 / (int64_t)worst_read));
        }
        const int64_t left = budget - p2 * (int64_t)worst_read;
        const int64_t p1 = std::max<int64_t>(1, std::min<int64_t>(p1_want, left / (int64_t)wave_bytes));
        fcd_handle::PoolGeom &g = h->pool_geom;
        const bool fits = h->pool_arena && g.cap_nodes == cap_nodes && g.cap_worst == cap_worst && g.first_stride == first_stride &&
                          g.rpw == rpw && g.row_words == (NL <= 4 ? 4 : 8) && g.p1 >= p1 && g.p2 >= p2 && (g.p2 > 0) == (p2 > 0);
        if (!fits) {
            rc = overlap_drain(h);  // calls in flight still use the old slabs
            if (rc) return rc;
            FCD_HIP(h, hipStreamSynchronize(h->stream));
            if (h->pool_arena) FCD_HIP(h, hipFree(h->pool_arena));
            if (h->pool_ctl) FCD_HIP(h, hipFree(h->pool_ctl));
            h->pool_arena = h->pool_ctl = nullptr;
            h->pool_arena_bytes = h->pool_ctl_bytes = 0;
            g = fcd_handle::PoolGeom();
            const size_t first_region = ((size_t)p1 * wave_bytes + 255) & ~(size_t)255;
            size_t dummy = 0;
            rc = ensure(h, &h->pool_arena, &h->pool_arena_bytes, first_region + (size_t)p2 * worst_read);
            if (rc) return rc;
            rc = ensure(h, &h->pool_ctl, &dummy, slab_pool::bytes((int)p1) + slab_pool::bytes((int)std::max<int64_t>(p2, 1)));
            if (rc) return rc;
            h->pool_ctl_bytes = dummy;
            unsigned long long *ring1 = reinterpret_cast<unsigned long long *>(h->pool_ctl);
            FCD_HIP(h, slab_pool_init(ring1, (int)p1, h->stream));
            if (p2 > 0) FCD_HIP(h, slab_pool_init(reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(h->pool_ctl) + slab_pool::bytes((int)p1)), (int)p2, h->stream));
            g.cap_nodes = cap_nodes;
            g.cap_worst = cap_worst;
            g.first_stride = first_stride;
            g.rpw = rpw;
            g.row_words = NL <= 4 ? 4 : 8;
            g.p1 = (int)p1;
            g.p2 = (int)p2;
        }
        if (retry_needed) {  // the overflow counters have their own small allocation: a word per stream (kMaxOverlap + 1 <= 64)
            rc = ensure(h, &h->retry_counter, &h->retry_counter_bytes, 256);
            if (rc) return rc;
            if (!h->retry_host) {  // (page-locked: the copy back is a DMA nobody waits for)
                if (hipHostMalloc(&h->retry_host, 64, hipHostMallocDefault) != hipSuccess) h->retry_host = nullptr;
                if (h->retry_host && hipEventCreateWithFlags(&h->retry_ev, hipEventDisableTiming) != hipSuccess) {
                    (void)hipHostFree(h->retry_host);
                    h->retry_host = nullptr;
                }
                if (!h->retry_host) {  // (not silently)
                    static std::atomic<bool> said{false};
                    if (!said.exchange(true))
                        fprintf(stderr, "fast_ctc_decode (fcd): no page-locked word for the overflow count of the wide-beam kernel's first "
                                        "pass: the first-pass slab size will not adapt (results are unaffected)\n");
                }
            }
        }
        char *const base = reinterpret_cast<char *>(h->pool_arena);
        const size_t first_region = ((size_t)g.p1 * wave_bytes + 255) & ~(size_t)255;
        unsigned long long *const ring1 = reinterpret_cast<unsigned long long *>(h->pool_ctl);
        unsigned long long *const ring2 = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(h->pool_ctl) + slab_pool::bytes(g.p1));
        // (the pool is not a region: calls on every stream share it, after its initialisation above on the handle's stream)
        rc = sc.begin(true, false);
        if (rc) return rc;
        const hipStream_t S = sc.stream;
        sc.time();
        WaveArena ar = wave_arena(base, (int64_t)g.p1 * rpw, cap_nodes);
        ar.pool = ring1;
        FCD_HIP(h, launch_beam_lane(d, 0, d.n_reads, args, ar, o, S, nbd));
        if (retry_needed) {
            // every read that overflowed is decoded again in a worst-case slab, where it cannot overflow; a wavefront of
            // this pass that finds no slab free waits for one (the pool is a queue), so ONE launch finishes the job
            // whatever happened in the first pass -- with nothing to do it is n wavefronts that read one status word and
            // leave.  Nobody waits for it: this entry point stays enqueue-only.
            // (overflow counter: word 0 for the handle's stream, slot + 1 for an internal one -- a stream's calls run in order)
            int32_t *const d_counter = reinterpret_cast<int32_t *>(h->retry_counter) + (sc.slot + 1);
            WaveArena rr = wave_arena(base + first_region, g.p2, cap_worst);
            rr.pool = ring2;
            rr.retry_counter = d_counter;
            FCD_HIP(h, hipMemsetAsync(d_counter, 0, sizeof(int32_t), S));
            FCD_HIP(h, launch_beam_lane(d, 0, d.n_reads, args, rr, o, S, nbd));
            // how many reads overflowed is read back ONE CALL LATE: it only steers the sizing of later jobs
            if (h->retry_host && !h->retry_pending) {
                FCD_HIP(h, hipMemcpyAsync(h->retry_host, d_counter, sizeof(int32_t), hipMemcpyDeviceToHost, S));
                FCD_HIP(h, hipEventRecord(h->retry_ev, S));
                h->retry_pending = true;
                h->retry_n = d.n_reads;
            }
        }
        return sc.finish();
    }
    // the arena: a region of it per internal stream (calls on the same internal stream follow one another, so do their
    // uses of its region), or all of it in stream order
    rc = sc.begin(true, true);
    if (rc) return rc;
    const hipStream_t S = sc.stream;
    const int64_t chunk = std::min<int64_t>(std::max<int64_t>(1, budget / sc.regions() / (int64_t)per_read), d.n_reads);
    char *abase = nullptr;
    rc = sc.arena((size_t)chunk * per_read, &abase);
    if (rc) return rc;
    sc.time();
    for (int64_t begin = 0; begin < d.n_reads; begin += chunk) {
        const int64_t n = std::min<int64_t>(chunk, d.n_reads - begin);
        if (use_wave || use_lane) {
            const WaveArena ar = wave_arena(abase, chunk, cap_nodes);
            FCD_HIP(h, use_lane ? launch_beam_lane(d, begin, n, args, ar, o, S, nbd) : launch_beam_wave(d, begin, n, args, ar, o, S, nbd));
        } else {
            GenericArena ar;
            ar.cap_nodes = cap_nodes;
            ar.rec = reinterpret_cast<int4 *>(abase);
            ar.rows = reinterpret_cast<int32_t *>(abase + (size_t)chunk * cap_nodes * sizeof(int4));
            FCD_HIP(h, launch_beam_generic(d, begin, n, args, ar, o, S, nbd));
        }
    }
    return sc.finish();
}

// ---- host staging -------------------------------------------------------------------------
// Element span of a strided batch, so that an arbitrarily strided host view can be shipped with
// one copy (non-negative strides only).
int64_t span_elems(const fcd_batch *in, bool crf) {
    if (in->n_reads == 0 || in->T == 0) return 0;
    int64_t s = 1;
    s += (in->n_reads - 1) * in->stride_read;
    s += (in->T - 1) * in->stride_t;
    if (crf) s += (in->S - 1) * in->stride_s;
    s += (in->N - 1) * in->stride_n;
    return s;
}

// The staging buffer of one *_host call: the host arrays the call ships to the device and back, each 256-byte aligned in
// h->stage, all on the handle's stream.  in() / out() name them, then commit() sizes the buffer and enqueues the uploads
// and the zero-fills; only then at() gives device addresses (ensure may move the buffer); fetch() after the device call
// copies the outputs back and waits.  A null host array takes no room and stays null on the device: the kernels branch
// on it.  An empty one keeps an address (the *_dev checks refuse null arrays) and is never copied.
class Staging {
  public:
    explicit Staging(fcd_handle *h) : h_(h) {}
    int in(const void *host, size_t bytes) { return put(const_cast<void *>(host), bytes, kIn); }
    int out(void *host, size_t bytes, bool zeroed = false) { return put(host, bytes, zeroed ? kOutZeroed : kOut); }
    int inout(void *host, size_t bytes) { return put(host, bytes, kInOut); }  // an output the call writes only parts of

    int commit() {
        fcd_handle *h = h_;
        int rc = ensure(h, &h->stage, &h->stage_bytes, used_);
        if (rc) return rc;
        char *base = static_cast<char *>(h->stage);
        for (const Array &a : a_)
            if ((a.kind == kIn || a.kind == kInOut) && a.bytes)
                FCD_HIP(h, hipMemcpyAsync(base + a.off, a.host, a.bytes, hipMemcpyHostToDevice, h->stream));
        // (outputs zeroed next to one another: one fill, padding included)
        for (size_t i = 0; i < a_.size(); ++i) {
            if (a_[i].kind != kOutZeroed) continue;
            size_t last = i;
            while (last + 1 < a_.size() && a_[last + 1].kind == kOutZeroed) ++last;
            const size_t n = a_[last].off + a_[last].bytes - a_[i].off;
            if (n) FCD_HIP(h, hipMemsetAsync(base + a_[i].off, 0, n, h->stream));
            i = last;
        }
        return FCD_OK;
    }

    template <class T>
    T *at(int id) const {
        return id < 0 ? nullptr : reinterpret_cast<T *>(static_cast<char *>(h_->stage) + a_[id].off);
    }

    int fetch() {
        fcd_handle *h = h_;
        char *base = static_cast<char *>(h->stage);
        for (const Array &a : a_)
            if (a.kind != kIn && a.bytes) FCD_HIP(h, hipMemcpyAsync(a.host, base + a.off, a.bytes, hipMemcpyDeviceToHost, h->stream));
        FCD_HIP(h, hipStreamSynchronize(h->stream));
        return FCD_OK;
    }

  private:
    enum Kind { kIn, kOut, kOutZeroed, kInOut };
    struct Array {
        void *host;
        size_t off, bytes;
        Kind kind;
    };
    fcd_handle *h_;
    std::vector<Array> a_;
    size_t used_ = 0;

    int put(void *host, size_t bytes, Kind kind) {  // -> what at() takes; -1: null
        if (!host) return -1;
        const size_t off = (used_ + 255) & ~(size_t)255;
        used_ = off + bytes;
        a_.push_back({host, off, bytes, kind});
        return (int)a_.size() - 1;
    }
};

}  // namespace

namespace fcd {
int effective_tie_order(const fcd_handle *h) {
    return (h && h->tie_order != FCD_TIE_DEFAULT) ? h->tie_order : g_tie_order.load();
}
}  // namespace fcd

// =============================================================================================
extern "C" {

int fcd_version(void) { return FCD_VERSION_MAJOR * 1000 + FCD_VERSION_MINOR; }

int fcd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int fcd_create(int device, fcd_handle **out) {
    if (!out) return FCD_E_INVALID;
    *out = nullptr;
    int n = fcd_device_count();
    if (n <= 0 || device < 0 || device >= n) return FCD_E_NODEVICE;
    DeviceGuard dev_guard(device);  // the caller's current device is put back on return
    if (dev_guard.err != hipSuccess) return FCD_E_HIP;
    fcd_handle *h = new fcd_handle();
    h->device = device;
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return FCD_E_HIP;
    }
    h->stream = h->own_stream;
    // the replay's std-form word lives on the device: every device a handle is created on gets the process's value
    if (apply_pdq178_std_form(g_pdq178_std_form.load()) != hipSuccess) {
        (void)hipStreamDestroy(h->own_stream);
        delete h;
        return FCD_E_HIP;
    }
    *out = h;
    return FCD_OK;
}

int fcd_destroy(fcd_handle *h) {
    if (!h) return FCD_OK;
    {
        std::lock_guard<std::recursive_mutex> g(h->mu);
        if (h->job_active) {  // its lane threads still write buffers this call would free: fcd_job_end comes first
            h->err = "a host job is running on this handle (fcd_job_end it first)";
            return FCD_E_INVALID;
        }
        if (h->live_sessions > 0) {  // their pushes run on this handle's stream
            h->err = "beam-search sessions are open on this handle (fcd_beam_session_destroy them first)";
            return FCD_E_INVALID;
        }
    }
    DeviceGuard dev_guard(h->device);
    host_job_release_lanes(h, true);
    (void)overlap_drain(h);
    (void)hipStreamSynchronize(h->stream);
    for (int s = 0; s < fcd_handle::kMaxOverlap; ++s) {
        if (h->ov_last[s]) (void)hipEventDestroy(h->ov_last[s]);
        if (h->ov_stream[s]) (void)hipStreamDestroy(h->ov_stream[s]);
    }
    if (h->ov_fork) (void)hipEventDestroy(h->ov_fork);
    for (hipEvent_t e : h->ov_event_pool) (void)hipEventDestroy(e);  // (overlap_drain above returned every flight's)
    if (h->pool_arena) (void)hipFree(h->pool_arena);
    if (h->pool_ctl) (void)hipFree(h->pool_ctl);
    if (h->arena) (void)hipFree(h->arena);
    if (h->stage) (void)hipFree(h->stage);
    if (h->pin) (void)hipHostFree(h->pin);
    if (h->lnbuf) (void)hipFree(h->lnbuf);
    if (h->retry_counter) (void)hipFree(h->retry_counter);
    if (h->retry_host) {
        (void)hipEventDestroy(h->retry_ev);
        (void)hipHostFree(h->retry_host);
        h->retry_host = nullptr;
        h->retry_pending = false;
    }
    for (hipEvent_t e : h->ev0) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->ev1) (void)hipEventDestroy(e);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
    return FCD_OK;
}

int fcd_set_stream(fcd_handle *h, void *hip_stream) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->stream = reinterpret_cast<hipStream_t>(hip_stream);  // nullptr is the HIP null stream
    return FCD_OK;
}

int fcd_reset_stream(fcd_handle *h) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->stream = h->own_stream;
    return FCD_OK;
}

int fcd_synchronize(fcd_handle *h) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    FCD_DEVICE(h);
    int rc = overlap_drain(h);  // (fcd_set_overlap: the internal streams first)
    if (rc) return rc;
    FCD_HIP(h, hipStreamSynchronize(h->stream));
    return FCD_OK;
}

int fcd_set_overlap(fcd_handle *h, int streams) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (streams < 0 || streams > fcd_handle::kMaxOverlap) return fail(h, FCD_E_INVALID, "fcd_set_overlap: 0 .. 8 streams");
    FCD_DEVICE(h);
    // what is in flight joins the handle's stream: from here on the stream order holds again (or a new round starts)
    int rc = overlap_join(h, h->stream);
    if (rc) return rc;
    h->overlap_n = streams < 2 ? 0 : streams;
    return FCD_OK;
}

int fcd_overlap_join(fcd_handle *h) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    FCD_DEVICE(h);
    return overlap_join(h, h->stream);
}

int fcd_overlap_last_slot(fcd_handle *h) {
    if (!h) return -1;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    return h->overlap_n >= 2 ? h->ov_last_slot : -1;
}

int fcd_overlap_join_slot(fcd_handle *h, int slot, void *hip_stream) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (slot < 0 || slot >= fcd_handle::kMaxOverlap) return fail(h, FCD_E_INVALID, "fcd_overlap_join_slot: no such internal stream");
    FCD_DEVICE(h);
    if (h->ov_stream[slot] && h->ov_used[slot]) FCD_HIP(h, hipStreamWaitEvent(reinterpret_cast<hipStream_t>(hip_stream), h->ov_last[slot], 0));
    return FCD_OK;
}

int fcd_overlap_join_stream(fcd_handle *h, void *hip_stream) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    FCD_DEVICE(h);
    return overlap_join(h, reinterpret_cast<hipStream_t>(hip_stream));
}

const char *fcd_last_error(const fcd_handle *h) { return h ? h->err.c_str() : "null handle"; }

const char *fcd_status_string(int status) {
    switch (status) {  // src/lib.rs:46-53, verbatim
        case FCD_ST_OK: return "";
        case FCD_ST_RAN_OUT_OF_BEAM: return "Ran out of search space (beam_cut_threshold too high)";
        case FCD_ST_INCOMPARABLE: return "Failed to compare values (NaNs in input?)";
        case FCD_ST_INVALID_ENVELOPE: return "Invalid envelope values";
        case FCD_ST_BAD_STATE:
            return "the reference would abort on this input (CRF state or init_state out of range, or an envelope whose "
                   "upper bound moves back below a beam entry's window)";
        case FCD_ST_INTERNAL: return "internal error: tree arena exhausted";
        default: return "unknown status";
    }
}

int fcd_set_workspace_limit(fcd_handle *h, int64_t bytes) {
    if (!h || bytes < 0) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->ws_limit = bytes;
    return FCD_OK;
}

int fcd_set_ctc_occupancy_wide(fcd_handle *h, int on) {
    if (!h || (on != 0 && on != 1)) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->occ_wide = on != 0;
    return FCD_OK;
}

int fcd_set_crf_lattice_wide(fcd_handle *h, int on) {
    if (!h || (on != 0 && on != 1)) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->crf_wide = on != 0;
    return FCD_OK;
}

int fcd_release_workspace(fcd_handle *h) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (h->job_active) return fail(h, FCD_E_INVALID, "a host job is running on this handle (fcd_job_end it first)");
    FCD_DEVICE(h);
    FCD_HIP(h, hipStreamSynchronize(h->stream));
    if (h->own_stream && h->own_stream != h->stream) FCD_HIP(h, hipStreamSynchronize(h->own_stream));
    host_job_release_lanes(h, false);
    {
        int rc = overlap_drain(h);
        if (rc) return rc;
    }
    if (h->pool_arena) (void)hipFree(h->pool_arena);
    if (h->pool_ctl) (void)hipFree(h->pool_ctl);
    h->pool_arena = h->pool_ctl = nullptr;
    h->pool_arena_bytes = h->pool_ctl_bytes = 0;
    h->pool_geom = fcd_handle::PoolGeom();
    if (h->arena) (void)hipFree(h->arena);
    if (h->stage) (void)hipFree(h->stage);
    if (h->lnbuf) (void)hipFree(h->lnbuf);
    if (h->pin) (void)hipHostFree(h->pin);
    if (h->retry_counter) (void)hipFree(h->retry_counter);
    if (h->retry_host) {
        (void)hipEventDestroy(h->retry_ev);
        (void)hipHostFree(h->retry_host);
        h->retry_host = nullptr;
        h->retry_pending = false;
    }
    h->arena = h->stage = h->lnbuf = h->pin = h->retry_counter = nullptr;
    h->arena_region = h->lnbuf_region = 0;
    h->arena_bytes = h->stage_bytes = h->lnbuf_bytes = h->pin_bytes = h->retry_counter_bytes = 0;
    return FCD_OK;
}

int64_t fcd_debug_workspace_bytes(fcd_handle *h) {
    if (!h) return -1;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    return (int64_t)(h->arena_bytes + h->pool_arena_bytes + h->pool_ctl_bytes + h->stage_bytes + h->lnbuf_bytes +
                     h->retry_counter_bytes);
}

int fcd_set_tie_order(fcd_handle *h, int order) {
    if (!h || (order != FCD_TIE_DEFAULT && order != FCD_TIE_PDQ178 && order != FCD_TIE_STABLE)) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->tie_order = order;
    return FCD_OK;
}

int fcd_get_tie_order(const fcd_handle *h) { return effective_tie_order(h); }

int fcd_set_default_tie_order(int order) {
    if (order != FCD_TIE_PDQ178 && order != FCD_TIE_STABLE) return FCD_E_INVALID;
    g_tie_order.store(order);
    return FCD_OK;
}

int fcd_debug_set_pdq178_std_form(fcd_handle *h, int bits) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (bits < 0 || bits > 3) return fail(h, FCD_E_INVALID, "the std form is 0, 1, 2 or 3");
    FCD_DEVICE(h);
    FCD_HIP(h, hipStreamSynchronize(h->stream));  // (no launch of this handle reads the word while it changes)
    FCD_HIP(h, apply_pdq178_std_form(bits));
    g_pdq178_std_form.store(bits);
    return FCD_OK;
}

int fcd_debug_get_pdq178_std_form(void) { return g_pdq178_std_form.load(); }

int fcd_debug_pdq178_sort_dev(fcd_handle *h, uint64_t *lists, int64_t n_lists, int64_t stride, const int32_t *lens) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (n_lists < 0 || stride < 0 || (n_lists > 0 && (!lists || !lens))) return fail(h, FCD_E_INVALID, "bad argument");
    FCD_DEVICE(h);
    FCD_HIP(h, launch_pdq178_probe(lists, n_lists, stride, lens, h->stream));
    return FCD_OK;
}

int fcd_debug_pdq178_coop_sort_dev(fcd_handle *h, uint64_t *lists, int64_t n_lists, int64_t stride, const int32_t *lens,
                                   int planes, int keep) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (n_lists < 0 || stride < 0 || (n_lists > 0 && (!lists || !lens)) || (planes != 1 && planes != 3 && planes != 5 && planes != 8) || keep < 1)
        return fail(h, FCD_E_INVALID, "bad argument");
    FCD_DEVICE(h);
    FCD_HIP(h, launch_pdq178_coop_probe(lists, n_lists, stride, lens, planes, keep, h->stream));
    return FCD_OK;
}

int fcd_debug_pdq178_coop_profile(fcd_handle *h, uint64_t cycles[16], int reset) {
    if (!h || !cycles) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    FCD_DEVICE(h);
    FCD_HIP(h, hipStreamSynchronize(h->stream));
    // bit 0: reset afterwards; bit 1: the wide-beam kernel's in-place counters (a -DFCD_LANE_TIE_PROF build) instead of the probe kernels'
    if (reset & 2) FCD_HIP(h, lane_tie_prof_read(reinterpret_cast<unsigned long long *>(cycles), (reset & 1) != 0));
    else FCD_HIP(h, coop_prof_read(reinterpret_cast<unsigned long long *>(cycles), (reset & 1) != 0));
    return FCD_OK;
}

int fcd_debug_set_first_pass_divisor(fcd_handle *h, int divisor) {
    if (!h || divisor < 0) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->first_pass_div = divisor ? divisor : 2;
    h->first_pass_div_pinned = divisor != 0;  // 0: back to the default, adaptive sizing
    return FCD_OK;
}

int fcd_debug_set_duplex_profile(fcd_handle *h, uint32_t *cycles) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->duplex_prof = cycles;
    return FCD_OK;
}

int fcd_debug_set_duplex_kernel(fcd_handle *h, int which) {
    if (!h || which < 0 || which > 2) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->duplex_kernel = which;
    return FCD_OK;
}

double fcd_last_kernel_ms(fcd_handle *h) {
    if (!h) return -1.0;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (h->n_timed == 0) return -1.0;
    const int slot = (int)((h->n_timed - 1) % fcd_handle::kTimingRing);
    if (hipEventSynchronize(h->ev1[slot]) != hipSuccess) return -1.0;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, h->ev0[slot], h->ev1[slot]) != hipSuccess) return -1.0;
    return (double)ms;
}

int fcd_timing_reset(fcd_handle *h) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->n_timed = 0;
    return FCD_OK;
}

double fcd_timing_mean_ms(fcd_handle *h, int64_t *n_calls) {
    if (!h) return -1.0;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    const int64_t n = std::min<int64_t>(h->n_timed, fcd_handle::kTimingRing);
    if (n_calls) *n_calls = n;
    if (n == 0) return -1.0;
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        float ms = 0.0f;
        if (hipEventSynchronize(h->ev1[i]) != hipSuccess) return -1.0;
        if (hipEventElapsedTime(&ms, h->ev0[i], h->ev1[i]) != hipSuccess) return -1.0;
        sum += ms;
    }
    return sum / (double)n;
}

// ---- viterbi -------------------------------------------------------------------------------
int fcd_viterbi_search_dev(fcd_handle *h, const fcd_batch *in, int collapse_repeats,
                           const fcd_result *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    int rc = check_batch(h, in, false);
    if (rc) return rc;
    rc = check_result(h, in, out, false);
    if (rc) return rc;
    if (in->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);
    CallScope sc(h);
    sc.add(to_desc(out), in->n_reads);
    rc = sc.begin(false, false);
    if (rc) return rc;
    sc.time();
    FCD_HIP(h, launch_viterbi(to_desc(in, false), collapse_repeats, to_desc(out), sc.stream));
    return sc.finish();
}

int fcd_beam_search_dev(fcd_handle *h, const fcd_batch *in, int64_t beam_size,
                        float beam_cut_threshold, int collapse_repeats, int kernel,
                        const fcd_result *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (beam_size < 1) return fail(h, FCD_E_INVALID, "beam_size cannot be 0");
    BeamArgs a{};
    a.beam_size = (int)std::min<int64_t>(beam_size, 1ll << 30);
    a.thr = beam_cut_threshold;
    a.collapse = collapse_repeats ? 1 : 0;
    a.crf = 0;
    return beam_dev(h, in, a, kernel, out);
}

int fcd_beam_search_profile_dev(fcd_handle *h, const fcd_batch *in, int64_t beam_size,
                                float beam_cut_threshold, int collapse_repeats, const fcd_result *out,
                                uint32_t *cycles) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (beam_size < 1 || beam_size > 5 || !in || in->N != 5 || !cycles)
        return fail(h, FCD_E_UNSUPPORTED, "profile: the instrumented instantiation is beam_size <= 5, N = 5");
    BeamArgs a{};
    a.beam_size = (int)beam_size;
    a.thr = beam_cut_threshold;
    a.collapse = collapse_repeats ? 1 : 0;
    a.crf = 0;
    a.prof = cycles;
    return beam_dev(h, in, a, FCD_KERNEL_WAVE, out);
}

int fcd_crf_beam_search_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                            int64_t init_stride, int64_t beam_size, float beam_cut_threshold,
                            const fcd_result *out) {
    return fcd_crf_beam_search_dev_k(h, in, init, n_init, init_stride, beam_size, beam_cut_threshold,
                                     FCD_KERNEL_AUTO, out);
}

int fcd_crf_beam_search_dev_k(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                              int64_t init_stride, int64_t beam_size, float beam_cut_threshold,
                              int kernel, const fcd_result *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (beam_size < 1) return fail(h, FCD_E_INVALID, "beam_size cannot be 0");
    if (!init || n_init < 1) return fail(h, FCD_E_INVALID, "init_state missing");
    BeamArgs a{};
    a.beam_size = (int)std::min<int64_t>(beam_size, 1ll << 30);
    a.thr = beam_cut_threshold;
    a.collapse = 0;
    a.crf = 1;
    a.init = init;
    a.n_init = n_init;
    a.init_stride = init_stride;
    return beam_dev(h, in, a, kernel, out);
}

int fcd_beam_search_nbest_dev(fcd_handle *h, const fcd_batch *in, int64_t beam_size, float beam_cut_threshold,
                              int collapse_repeats, int kernel, const fcd_nbest *nb, const fcd_result *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (beam_size < 1) return fail(h, FCD_E_INVALID, "beam_size cannot be 0");
    BeamArgs a{};
    a.beam_size = (int)std::min<int64_t>(beam_size, 1ll << 30);
    a.thr = beam_cut_threshold;
    a.collapse = collapse_repeats ? 1 : 0;
    a.crf = 0;
    return beam_dev(h, in, a, kernel, out, nb);
}

int fcd_crf_beam_search_nbest_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                                  int64_t init_stride, int64_t beam_size, float beam_cut_threshold, int kernel,
                                  const fcd_nbest *nb, const fcd_result *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (beam_size < 1) return fail(h, FCD_E_INVALID, "beam_size cannot be 0");
    if (!init || n_init < 1) return fail(h, FCD_E_INVALID, "init_state missing");
    BeamArgs a{};
    a.beam_size = (int)std::min<int64_t>(beam_size, 1ll << 30);
    a.thr = beam_cut_threshold;
    a.collapse = 0;
    a.crf = 1;
    a.init = init;
    a.n_init = n_init;
    a.init_stride = init_stride;
    return beam_dev(h, in, a, kernel, out, nb);
}

int fcd_crf_greedy_search_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                              int64_t init_stride, const fcd_result *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    int rc = check_batch(h, in, true);
    if (rc) return rc;
    rc = check_result(h, in, out, true);
    if (rc) return rc;
    if (!init || n_init < 1) return fail(h, FCD_E_INVALID, "init_state missing");
    if (in->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);
    CallScope sc(h);
    sc.add(to_desc(out), in->n_reads);
    rc = sc.begin(false, false);
    if (rc) return rc;
    sc.time();
    FCD_HIP(h, launch_crf_greedy(to_desc(in, true), init, n_init, init_stride, to_desc(out), sc.stream));
    return sc.finish();
}

// ---- the Viterbi search under a CRF model (crf_viterbi.hip): the best state path over all labellings ----
namespace {
int crf_viterbi_check(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                      const fcd_result *out) {
    int rc = check_batch(h, in, true);
    if (rc) return rc;
    rc = check_result(h, in, out, true);
    if (rc) return rc;
    if (!init || n_init < 1) return fail(h, FCD_E_INVALID, "init_state missing");
    if (init_stride < 0) return fail(h, FCD_E_INVALID, "negative stride");
    switch (crf_viterbi_unsupported(in->S, in->N)) {
    case 1: return fail(h, FCD_E_UNSUPPORTED, "crf_viterbi_search: N must be in 2 .. 9");
    case 2: return fail(h, FCD_E_UNSUPPORTED, "crf_viterbi_search: S must be a multiple of N - 1 (the states that reach a state are "
                                              "s div (N - 1) + i S / (N - 1))");
    case 3: return fail(h, FCD_E_UNSUPPORTED, "crf_viterbi_search: S must be below 2^24");
    case 4: return fail(h, FCD_E_UNSUPPORTED, "crf_viterbi_search: N S 4 bytes of states and candidates do not fit the 160 KiB of LDS");
    default: break;
    }
    return FCD_OK;
}

// Whole reads per launch, as many as the workspace cap holds back-pointers for (at least one), every launch in the same
// memory, one after the other on the handle's stream (lattice_grouped's rule; the cap is fcd_crf_align_*'s).
int crf_viterbi_run(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                    const fcd_result *out, double *logp) {
    const int64_t read_bytes = (int64_t)crf_viterbi_read_bytes(in->T, in->S);
    const int64_t cap = h->align_ws_cap > 0 ? h->align_ws_cap : std::min<int64_t>(4ll << 30, workspace_budget(h));
    const int64_t group = std::max<int64_t>(1, std::min<int64_t>(in->n_reads, cap / read_bytes));
    CallScope sc(h);
    sc.add(to_desc(out), in->n_reads);
    sc.add(logp, (size_t)in->n_reads * 8);
    int rc = sc.begin(false, true);  // (exclusive: the workspace from its start, behind every overlapping call in flight)
    if (rc) return rc;
    char *ws = nullptr;
    rc = sc.arena((size_t)group * (size_t)read_bytes, &ws);
    if (rc) return rc;
    const int64_t esz = in->dtype == FCD_DTYPE_F32 ? 4 : 2;
    sc.time();
    for (int64_t r0 = 0; r0 < in->n_reads; r0 += group) {
        BatchDesc d = to_desc(in, true);
        d.post = reinterpret_cast<const float *>(reinterpret_cast<const char *>(in->post) + r0 * in->stride_read * esz);
        d.lengths = in->lengths ? in->lengths + r0 : nullptr;
        d.n_reads = std::min(group, in->n_reads - r0);
        ResultDesc o = to_desc(out);
        o.labels = out->labels + r0 * out->out_stride;
        o.path = out->path ? out->path + r0 * out->out_stride : nullptr;
        o.qual = out->qual ? out->qual + r0 * out->out_stride : nullptr;
        o.out_len = out->out_len + r0;
        o.status = out->status + r0;
        FCD_HIP(h, launch_crf_viterbi(d, init + r0 * init_stride, n_init, init_stride, o, logp ? logp + r0 : nullptr,
                                      reinterpret_cast<unsigned char *>(ws), sc.stream));
    }
    return sc.finish();
}
}  // namespace

int fcd_crf_viterbi_search_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                               const fcd_result *out, double *logp) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    int rc = crf_viterbi_check(h, in, init, n_init, init_stride, out);
    if (rc) return rc;
    if (in->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);
    return crf_viterbi_run(h, in, init, n_init, init_stride, out, logp);
}

// host arrays: staged in the order post, init, lengths, the outputs; the device call runs on the handle's stream
int fcd_crf_viterbi_search_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                                const fcd_result *out, double *logp) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    int rc = crf_viterbi_check(h, in, init, n_init, init_stride, out);
    if (rc) return rc;
    if (in->n_reads == 0) return FCD_OK;
    if (in->stride_read < 0 || in->stride_t < 0 || in->stride_s < 0 || in->stride_n < 0)
        return fail(h, FCD_E_UNSUPPORTED, "negative strides: pass a contiguous copy");
    FCD_DEVICE(h);
    const size_t B = (size_t)in->n_reads, cells = B * (size_t)out->out_stride;
    Staging st(h);
    const int i_post = st.in(in->post, (size_t)span_elems(in, true) * (in->dtype == FCD_DTYPE_F32 ? 4 : 2));
    const int i_init = st.in(init, (size_t)((in->n_reads - 1) * init_stride + n_init) * 4);
    const int i_len = st.in(in->lengths, B * 8);
    const int i_lab = st.out(out->labels, cells);
    const int i_path = st.out(out->path, cells * 4);
    const int i_qual = st.out(out->qual, cells * 4);
    const int i_olen = st.out(out->out_len, B * 4);
    const int i_stat = st.out(out->status, B * 4);
    const int i_logp = st.out(logp, B * 8);
    rc = st.commit();
    if (rc) return rc;
    fcd_batch din = *in;
    din.post = st.at<char>(i_post);
    din.lengths = st.at<int64_t>(i_len);
    fcd_result dout = *out;
    dout.labels = st.at<uint8_t>(i_lab);
    dout.path = st.at<uint32_t>(i_path);
    dout.qual = st.at<float>(i_qual);
    dout.out_len = st.at<uint32_t>(i_olen);
    dout.status = st.at<int32_t>(i_stat);
    dout.ambiguous = nullptr;
    rc = crf_viterbi_run(h, &din, st.at<float>(i_init), n_init, init_stride, &dout, st.at<double>(i_logp));
    if (rc) return rc;
    return st.fetch();
}

// ---- CRF transition probabilities from raw scores (crf_transitions.hip): the (posteriors, init) pair of the CRF entry points ----
namespace {
int64_t transitions_span(const fcd_batch *in, const fcd_transitions *out) {  // elements of probs the call may write
    if (in->n_reads == 0 || in->T == 0) return 0;
    return (in->n_reads - 1) * out->stride_read + (in->T - 1) * out->stride_t + in->S * in->N;
}

int crf_transitions_check(fcd_handle *h, const fcd_batch *in, int layout, const fcd_transitions *out) {
    int rc = check_batch(h, in, true);
    if (rc) return rc;
    if (!out) return fail(h, FCD_E_INVALID, "null transitions");
    if (layout != FCD_LAYOUT_SOURCE && layout != FCD_LAYOUT_DEST) return fail(h, FCD_E_INVALID, "unknown score layout");
    if (out->dtype != FCD_DTYPE_F32 && out->dtype != FCD_DTYPE_F16)
        return fail(h, FCD_E_INVALID, "unknown dtype of the transition probabilities (float32 or float16)");
    if (in->stride_read < 0 || in->stride_t < 0 || in->stride_s < 0 || in->stride_n < 0)
        return fail(h, FCD_E_INVALID, "negative stride");
    switch (crf_transitions_unsupported(in->S, in->N)) {
    case 1: return fail(h, FCD_E_UNSUPPORTED, "crf_transition_probs: N must be in 2 .. 9");
    case 2: return fail(h, FCD_E_UNSUPPORTED, "crf_transition_probs: S must be a multiple of N - 1 (symbol j + 1 moves state s to "
                                              "(s (N - 1)) mod S + j)");
    case 3: return fail(h, FCD_E_UNSUPPORTED, "crf_transition_probs: S must be below 2^24");
    case 4: return fail(h, FCD_E_UNSUPPORTED, "crf_transition_probs: 8 S + 4608 bytes of backward rows and staging do not fit the 160 KiB of LDS");
    default: break;
    }
    if (in->n_reads == 0) return FCD_OK;
    if ((in->T > 0 && !out->probs) || !out->init || !out->status) return fail(h, FCD_E_INVALID, "null probs/init/status");
    if (out->stride_read < in->S * in->N || out->stride_t < in->S * in->N)
        return fail(h, FCD_E_INVALID, "stride_read and stride_t of the transition probabilities must be at least S N");
    if (out->init_stride < in->S) return fail(h, FCD_E_INVALID, "init_stride must be at least S");
    return FCD_OK;
}

int crf_transitions_run(fcd_handle *h, const fcd_batch *in, int layout, const fcd_transitions *out) {
    const size_t B = (size_t)in->n_reads;
    CallScope sc(h);
    sc.add(out->probs, (size_t)transitions_span(in, out) * (out->dtype == FCD_DTYPE_F32 ? 4 : 2));
    sc.add(out->init, ((B - 1) * (size_t)out->init_stride + (size_t)in->S) * 4);
    sc.add(out->logz, B * 8);
    sc.add(out->status, B * 4);
    int rc = sc.begin(false, true);  // (behind every overlapping call in flight: one of them may be writing the scores)
    if (rc) return rc;
    TransitionsDesc d;
    d.probs = out->probs;
    d.dtype = out->dtype;
    d.layout = layout;
    d.stride_read = out->stride_read;
    d.stride_t = out->stride_t;
    d.init = out->init;
    d.init_stride = out->init_stride;
    d.logz = out->logz;
    d.status = out->status;
    sc.time();
    FCD_HIP(h, launch_crf_transitions(to_desc(in, true), d, sc.stream));
    return sc.finish();
}
}  // namespace

int fcd_crf_transition_probs_dev(fcd_handle *h, const fcd_batch *scores, int layout, const fcd_transitions *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    int rc = crf_transitions_check(h, scores, layout, out);
    if (rc) return rc;
    if (scores->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);
    return crf_transitions_run(h, scores, layout, out);
}

// host arrays: staged in the order scores, lengths, the outputs; probs travels both ways (rows t >= T_r are not written)
int fcd_crf_transition_probs_host(fcd_handle *h, const fcd_batch *scores, int layout, const fcd_transitions *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    int rc = crf_transitions_check(h, scores, layout, out);
    if (rc) return rc;
    const fcd_batch *in = scores;
    if (in->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);
    const size_t B = (size_t)in->n_reads;
    Staging st(h);
    const int i_x = st.in(in->post, (size_t)span_elems(in, true) * (in->dtype == FCD_DTYPE_F32 ? 4 : 2));
    const int i_len = st.in(in->lengths, B * 8);
    const int i_probs = st.inout(out->probs, (size_t)transitions_span(in, out) * (out->dtype == FCD_DTYPE_F32 ? 4 : 2));
    const size_t init_bytes = ((B - 1) * (size_t)out->init_stride + (size_t)in->S) * 4;
    // (init rows with spare elements between them travel both ways too: the spare elements keep the caller's content)
    const int i_init = out->init_stride > in->S ? st.inout(out->init, init_bytes) : st.out(out->init, init_bytes);
    const int i_logz = st.out(out->logz, B * 8);
    const int i_stat = st.out(out->status, B * 4);
    rc = st.commit();
    if (rc) return rc;
    fcd_batch din = *in;
    din.post = st.at<char>(i_x);
    din.lengths = st.at<int64_t>(i_len);
    fcd_transitions dout = *out;
    dout.probs = st.at<char>(i_probs);
    dout.init = st.at<float>(i_init);
    dout.logz = st.at<double>(i_logz);
    dout.status = st.at<int32_t>(i_stat);
    rc = crf_transitions_run(h, &din, layout, &dout);
    if (rc) return rc;
    return st.fetch();
}

// ---- CRF edge marginals (crf_transitions.hip): the transition walk into the caller's buffer and the forward pass over it ----
namespace {
int64_t marginals_span(const fcd_batch *in, const fcd_marginals *out) {  // elements of marg the call may write
    if (in->n_reads == 0 || in->T == 0) return 0;
    return (in->n_reads - 1) * out->stride_read + (in->T - 1) * out->stride_t + in->S * in->N;
}

int64_t emit_span(const fcd_batch *in, const fcd_marginals *out) {
    if (in->n_reads == 0 || in->T == 0 || !out->emit) return 0;
    return (in->n_reads - 1) * out->emit_stride + in->T * in->N;
}

int crf_marginals_check(fcd_handle *h, const fcd_batch *in, int layout, const fcd_marginals *out) {
    int rc = check_batch(h, in, true);
    if (rc) return rc;
    if (!out) return fail(h, FCD_E_INVALID, "null marginals");
    if (layout != FCD_LAYOUT_SOURCE && layout != FCD_LAYOUT_DEST) return fail(h, FCD_E_INVALID, "unknown score layout");
    if (in->stride_read < 0 || in->stride_t < 0 || in->stride_s < 0 || in->stride_n < 0)
        return fail(h, FCD_E_INVALID, "negative stride");
    switch (crf_transitions_unsupported(in->S, in->N)) {
    case 1: return fail(h, FCD_E_UNSUPPORTED, "crf_marginals: N must be in 2 .. 9");
    case 2: return fail(h, FCD_E_UNSUPPORTED, "crf_marginals: S must be a multiple of N - 1 (symbol j + 1 moves state s to "
                                              "(s (N - 1)) mod S + j)");
    case 3: return fail(h, FCD_E_UNSUPPORTED, "crf_marginals: S must be below 2^24");
    case 4: return fail(h, FCD_E_UNSUPPORTED, "crf_marginals: 8 S + 4608 bytes of occupancy rows and staging do not fit the 160 KiB of LDS");
    default: break;
    }
    if (in->n_reads == 0) return FCD_OK;
    if ((in->T > 0 && !out->marg) || !out->status) return fail(h, FCD_E_INVALID, "null marg/status");
    if (out->stride_read < in->S * in->N || out->stride_t < in->S * in->N)
        return fail(h, FCD_E_INVALID, "stride_read and stride_t of the marginals must be at least S N");
    if (out->emit && out->emit_stride < in->T * in->N) return fail(h, FCD_E_INVALID, "emit_stride must be at least T N");
    return FCD_OK;
}

int crf_marginals_run(fcd_handle *h, const fcd_batch *in, int layout, const fcd_marginals *out) {
    const size_t B = (size_t)in->n_reads;
    CallScope sc(h);
    sc.add(out->marg, (size_t)marginals_span(in, out) * 4);
    sc.add(out->emit, (size_t)emit_span(in, out) * 4);
    sc.add(out->logz, B * 8);
    sc.add(out->status, B * 4);
    int rc = sc.begin(false, true);  // (behind every overlapping call in flight: one of them may be writing the scores)
    if (rc) return rc;
    TransitionsDesc d;
    d.probs = out->marg;
    d.dtype = FCD_DTYPE_F32;
    d.layout = layout;
    d.stride_read = out->stride_read;
    d.stride_t = out->stride_t;
    d.init = nullptr;  // (the init row stays in LDS)
    d.init_stride = 0;
    d.logz = out->logz;
    d.status = out->status;
    sc.time();
    FCD_HIP(h, launch_crf_marginals(to_desc(in, true), d, out->emit, out->emit_stride, sc.stream));
    return sc.finish();
}
}  // namespace

int fcd_crf_marginals_dev(fcd_handle *h, const fcd_batch *scores, int layout, const fcd_marginals *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    int rc = crf_marginals_check(h, scores, layout, out);
    if (rc) return rc;
    if (scores->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);
    return crf_marginals_run(h, scores, layout, out);
}

// host arrays: staged in the order scores, lengths, the outputs; marg and emit travel both ways (rows t >= T_r are not written)
int fcd_crf_marginals_host(fcd_handle *h, const fcd_batch *scores, int layout, const fcd_marginals *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    int rc = crf_marginals_check(h, scores, layout, out);
    if (rc) return rc;
    const fcd_batch *in = scores;
    if (in->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);
    const size_t B = (size_t)in->n_reads;
    Staging st(h);
    const int i_x = st.in(in->post, (size_t)span_elems(in, true) * (in->dtype == FCD_DTYPE_F32 ? 4 : 2));
    const int i_len = st.in(in->lengths, B * 8);
    const int i_marg = st.inout(out->marg, (size_t)marginals_span(in, out) * 4);
    const int i_emit = st.inout(out->emit, (size_t)emit_span(in, out) * 4);
    const int i_logz = st.out(out->logz, B * 8);
    const int i_stat = st.out(out->status, B * 4);
    rc = st.commit();
    if (rc) return rc;
    fcd_batch din = *in;
    din.post = st.at<char>(i_x);
    din.lengths = st.at<int64_t>(i_len);
    fcd_marginals dout = *out;
    dout.marg = st.at<float>(i_marg);
    dout.emit = st.at<float>(i_emit);
    dout.logz = st.at<double>(i_logz);
    dout.status = st.at<int32_t>(i_stat);
    rc = crf_marginals_run(h, &din, layout, &dout);
    if (rc) return rc;
    return st.fetch();
}

namespace {
struct CrfInit {
    const float *init1 = nullptr, *init2 = nullptr;
    int64_t n1 = 0, s1 = 0, n2 = 0, s2 = 0;
};

// Shared driver of duplex::beam_search (crf == nullptr) and duplex::crf_beam_search.
int duplex_dev(fcd_handle *h, const fcd_batch *in1, const fcd_batch *in2, const CrfInit *crf,
               const uint64_t *envelope, int64_t env_stride, int64_t beam_size,
               float beam_cut_threshold, int collapse_repeats, int logadd_mode,
               const fcd_result *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    const bool is_crf = crf != nullptr;
    int rc = check_batch(h, in1, is_crf);
    if (rc) return rc;
    rc = check_batch(h, in2, is_crf);
    if (rc) return rc;
    if (is_crf && in1->S != in2->S) return fail(h, FCD_E_INVALID, "state counts of the two network outputs differ");
    if (is_crf && (!crf->init1 || !crf->init2 || crf->n1 < 1 || crf->n2 < 1))
        return fail(h, FCD_E_INVALID, "init_state missing");
    const int S = is_crf ? (int)in1->S : 1;
    if (in1->n_reads != in2->n_reads) return fail(h, FCD_E_INVALID, "pair counts differ");
    if (in1->N != in2->N) return fail(h, FCD_E_INVALID, "inner axes of the network outputs do not match");
    if (in1->N < 2) return fail(h, FCD_E_UNSUPPORTED, "alphabet needs at least one label besides the blank");
    if (beam_size < 1) return fail(h, FCD_E_INVALID, "beam_size cannot be 0");
    if (logadd_mode != FCD_LOGADD_LOGSUMEXP && logadd_mode != FCD_LOGADD_MAX && logadd_mode != FCD_LOGADD_LOGSUMEXP_GLIBC235)
        return fail(h, FCD_E_INVALID, "unknown logadd_mode");
    if (!out) return fail(h, FCD_E_INVALID, "null result");
    const int64_t B = in1->n_reads;
    if (B == 0) return FCD_OK;
    if (!out->labels || !out->out_len || !out->status) return fail(h, FCD_E_INVALID, "null output array");
    if (out->out_stride < in1->T) return fail(h, FCD_E_INVALID, "out_stride must be >= T1");
    if (!envelope || env_stride < in1->T) return fail(h, FCD_E_INVALID, "envelope missing or shorter than read 1");
    if (beam_size > (1 << 12)) return fail(h, FCD_E_UNSUPPORTED, "beam_size above 4096");
    const int N = (int)in1->N, NL = N - 1;
    if (duplex_lds_bytes((int)beam_size, N, 0, S, effective_tie_order(h)) > 64 * 1024)
        return fail(h, FCD_E_UNSUPPORTED, "beam_size * alphabet too large for the LDS-resident kernel");
    FCD_DEVICE(h);

    // log-space copies + one int for the envelope width.  fcd_set_overlap: the call goes to the next internal stream, with
    // a region of the log-space buffer and of the arena to itself (beam_dev)
    const int64_t T1 = std::max<int64_t>(in1->T, 1), T2 = std::max<int64_t>(in2->T, 1);
    const size_t n1 = (size_t)B * T1 * S * N, n2 = (size_t)B * T2 * S * N;
    CallScope sc(h);
    sc.add(to_desc(out), B);
    rc = sc.begin(true, true);
    if (rc) return rc;
    const hipStream_t St = sc.stream;
    char *lnbase = nullptr;
    rc = sc.lnbuf((n1 + n2) * 4 + 256, &lnbase);
    if (rc) return rc;
    float *ln1 = reinterpret_cast<float *>(lnbase);
    float *ln2 = ln1 + n1;
    int *d_width = reinterpret_cast<int *>(ln2 + n2);
    sc.time();
    FCD_HIP(h, launch_ln_convert(static_cast<const float *>(in1->post), in1->dtype, B, in1->T, S, N, in1->stride_read, in1->stride_t,
                                 is_crf ? in1->stride_s : 0, in1->stride_n, ln1, logadd_mode == FCD_LOGADD_LOGSUMEXP_GLIBC235, St));
    FCD_HIP(h, launch_ln_convert(static_cast<const float *>(in2->post), in2->dtype, B, in2->T, S, N, in2->stride_read, in2->stride_t,
                                 is_crf ? in2->stride_s : 0, in2->stride_n, ln2, logadd_mode == FCD_LOGADD_LOGSUMEXP_GLIBC235, St));
    FCD_HIP(h, hipMemsetAsync(d_width, 0, sizeof(int), St));
    FCD_HIP(h, launch_env_width(envelope, B, env_stride, in1->T, in2->T, in1->lengths,
                                in2->lengths, d_width, St));
    int width = 0;
    FCD_HIP(h, hipMemcpyAsync(&width, d_width, sizeof(int), hipMemcpyDeviceToHost, St));
    FCD_HIP(h, hipStreamSynchronize(St));  // ring capacity is needed to size the arena
    // Which kernel: the slot-resident one (duplex_slots.hip) wherever it fits -- beam_size * N <= 64 and the live nodes'
    // rings next to the read-2 tile in 64 KiB of LDS -- the any-shape one (duplex.hip) otherwise.
    const int tie = effective_tie_order(h);
    static const int env_kernel = [] {
        const char *e = getenv("FCD_DUPLEX_KERNEL");  // "legacy" / "slots": A/B and test aid
        return e ? (!strcmp(e, "legacy") ? 1 : (!strcmp(e, "slots") ? 2 : 0)) : 0;
    }();
    const int want = h->duplex_kernel ? h->duplex_kernel : env_kernel;
    const bool fits = duplex_slots_supported((int)beam_size, N, S, std::max(width, 1), tie);
    if (want == 2 && !fits) return fail(h, FCD_E_UNSUPPORTED, "duplex kernel: the slot-resident kernel does not cover this shape");
    const int NLp = (NL + 3) & ~3;
    const int64_t cap_nodes = (std::max<int64_t>(in1->T, 1) * beam_size * NL + 8 + 3) & ~3ll;
    if (cap_nodes >= (1ll << 30)) return fail(h, FCD_E_UNSUPPORTED, "tree arena above 2^30 nodes per pair");
    // (the slot-resident kernel addresses a pair's slab and its log-space reads with 32-bit byte offsets)
    const bool small = fits && duplex_slots_pair_bytes(cap_nodes, N, duplex_slots_ring_rows(std::max(width, 1)), in2->T) < (1ull << 32) &&
                       (uint64_t)std::max(in1->T, in2->T) * S * N * 4 < (1ull << 31);
    if (want == 2 && fits && !small) return fail(h, FCD_E_UNSUPPORTED, "duplex kernel: a pair's arena above 4 GiB");
    const bool slots = small && want != 1;
    const int Wcap = slots ? duplex_slots_ring_rows(std::max(width, 1)) : std::max(width, 1) + 2;
    const size_t per_pair = slots ? duplex_slots_pair_bytes(cap_nodes, N, Wcap, in2->T)
                                  : (size_t)cap_nodes * (sizeof(int4) + 8 + (size_t)NL * 4 + (size_t)Wcap * 12) +
                                        (((size_t)(in2->T + 1) * 4 + 64 + 15) & ~(size_t)15);
    const int64_t budget = workspace_budget(h);
    const int64_t chunk = std::min<int64_t>(std::max<int64_t>(1, budget / sc.regions() / (int64_t)per_pair), B);
    char *abase = nullptr;
    rc = sc.arena((size_t)chunk * per_pair, &abase);
    if (rc) return rc;

    DuplexArgs a;
    a.ln1 = ln1; a.ln2 = ln2; a.T1cap = in1->T; a.T2cap = in2->T;
    a.len1 = in1->lengths; a.len2 = in2->lengths; a.env = envelope; a.env_stride = env_stride;
    a.N = N; a.beam_size = (int)beam_size;
    // ln(threshold) with the kernels' definition of ln: correctly rounded f32 (duplex.rs:454)
    a.thr_ln = logadd_mode == FCD_LOGADD_LOGSUMEXP_GLIBC235 ? g235::logf235(beam_cut_threshold)
                                                           : (float)log((double)beam_cut_threshold);
    a.collapse = collapse_repeats ? 1 : 0; a.mode = logadd_mode;
    a.S = S; a.crf = is_crf ? 1 : 0;
    a.init1 = is_crf ? crf->init1 : nullptr; a.init2 = is_crf ? crf->init2 : nullptr;
    a.n_init1 = is_crf ? crf->n1 : 0; a.n_init2 = is_crf ? crf->n2 : 0;
    a.init1_stride = is_crf ? crf->s1 : 0; a.init2_stride = is_crf ? crf->s2 : 0;
    char *base = abase;
    a.meta = reinterpret_cast<int4 *>(base); base += (size_t)chunk * cap_nodes * sizeof(int4);
    a.aux = nullptr; a.nmax = nullptr; a.rlo = nullptr; a.NLp = NLp; a.pair_stride = (int64_t)per_pair;
    if (slots) {
        a.meta = reinterpret_cast<int4 *>(abase);  // (one slab per pair: duplex_slots.hip)
        a.vec = nullptr; a.rows = nullptr;
    } else {
        a.nmax = reinterpret_cast<float *>(base); base += (size_t)chunk * cap_nodes * 4;
        a.rlo = reinterpret_cast<int32_t *>(base); base += (size_t)chunk * cap_nodes * 4;
        a.rows = reinterpret_cast<int32_t *>(base); base += (size_t)chunk * cap_nodes * NL * 4;
        a.vec = reinterpret_cast<float *>(base); base += (size_t)chunk * cap_nodes * (size_t)Wcap * 12;
    }
    a.rootgap = reinterpret_cast<float *>(base);
    a.cap_nodes = cap_nodes; a.Wcap = Wcap;
    // any-shape kernel: tile the envelope window through LDS when it fits next to the beam (48 KiB budget)
    // (and keep the beam entries' windows resident there: one LDS buffer per beam slot, handed over by lane votes)
    a.staged = !slots && duplex_lds_bytes((int)beam_size, N, Wcap - 2, S, tie) <= 48 * 1024 && beam_size <= 64 ? 1 : 0;
    a.out = to_desc(out);
    a.prof = h->duplex_prof;
    a.tie_order = tie;
    for (int64_t begin = 0; begin < B; begin += chunk) {
        const int64_t n = std::min<int64_t>(chunk, B - begin);
        FCD_HIP(h, slots ? launch_duplex_slots(a, begin, n, St) : launch_duplex(a, begin, n, St));
    }
    return sc.finish();
}
}  // namespace

int fcd_beam_search_duplex_dev(fcd_handle *h, const fcd_batch *in1, const fcd_batch *in2,
                               const uint64_t *envelope, int64_t env_stride, int64_t beam_size,
                               float beam_cut_threshold, int collapse_repeats, int logadd_mode,
                               const fcd_result *out) {
    return duplex_dev(h, in1, in2, nullptr, envelope, env_stride, beam_size, beam_cut_threshold,
                      collapse_repeats, logadd_mode, out);
}

int fcd_crf_beam_search_duplex_dev(fcd_handle *h, const fcd_batch *in1, const float *init1,
                                   int64_t n_init1, int64_t init1_stride, const fcd_batch *in2,
                                   const float *init2, int64_t n_init2, int64_t init2_stride,
                                   const uint64_t *envelope, int64_t env_stride, int64_t beam_size,
                                   float beam_cut_threshold, int logadd_mode, const fcd_result *out) {
    CrfInit c;
    c.init1 = init1; c.n1 = n_init1; c.s1 = init1_stride;
    c.init2 = init2; c.n2 = n_init2; c.s2 = init2_stride;
    return duplex_dev(h, in1, in2, &c, envelope, env_stride, beam_size, beam_cut_threshold, 0,
                      logadd_mode, out);
}

namespace {
// host staging shared by fcd_beam_search_duplex_host / fcd_crf_beam_search_duplex_host
int duplex_host(fcd_handle *h, const fcd_batch *in1, const fcd_batch *in2, const CrfInit *crf,
                const uint64_t *envelope, int64_t env_stride, int64_t beam_size,
                float beam_cut_threshold, int collapse_repeats, int logadd_mode,
                const fcd_result *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    const bool is_crf = crf != nullptr;
    int rc = check_batch(h, in1, is_crf);
    if (rc) return rc;
    rc = check_batch(h, in2, is_crf);
    if (rc) return rc;
    if (in1->n_reads != in2->n_reads) return fail(h, FCD_E_INVALID, "pair counts differ");
    if (!out || !envelope) return fail(h, FCD_E_INVALID, "null result/envelope");
    if (in1->stride_read < 0 || in1->stride_t < 0 || in1->stride_n < 0 || in2->stride_read < 0 ||
        in2->stride_t < 0 || in2->stride_n < 0 || (is_crf && (in1->stride_s < 0 || in2->stride_s < 0)))
        return fail(h, FCD_E_UNSUPPORTED, "negative strides: pass a contiguous copy");
    if (is_crf && (!crf->init1 || !crf->init2 || crf->n1 < 1 || crf->n2 < 1))
        return fail(h, FCD_E_INVALID, "init_state missing");
    const int64_t B = in1->n_reads;
    if (B == 0) return FCD_OK;
    if (!out->labels || !out->out_len || !out->status) return fail(h, FCD_E_INVALID, "null output array");
    FCD_DEVICE(h);  // staging, search and copy-back all run on the handle's device
    Staging st(h);
    const int i_post1 = st.in(in1->post, (size_t)span_elems(in1, is_crf) * (in1->dtype == FCD_DTYPE_F32 ? 4 : 2));
    const int i_post2 = st.in(in2->post, (size_t)span_elems(in2, is_crf) * (in2->dtype == FCD_DTYPE_F32 ? 4 : 2));
    const int i_env = st.in(envelope, (size_t)B * (size_t)env_stride * 16);
    const int i_len1 = st.in(in1->lengths, (size_t)B * 8);
    const int i_len2 = st.in(in2->lengths, (size_t)B * 8);
    const int i_init1 = is_crf ? st.in(crf->init1, (size_t)((B - 1) * crf->s1 + crf->n1) * 4) : -1;
    const int i_init2 = is_crf ? st.in(crf->init2, (size_t)((B - 1) * crf->s2 + crf->n2) * 4) : -1;
    const int i_lab = st.out(out->labels, (size_t)B * (size_t)out->out_stride);
    const int i_olen = st.out(out->out_len, (size_t)B * 4);
    const int i_stat = st.out(out->status, (size_t)B * 4);
    const int i_amb = st.out(out->ambiguous, (size_t)B * 8);
    rc = st.commit();
    if (rc) return rc;
    fcd_batch d1 = *in1, d2 = *in2;
    d1.post = st.at<char>(i_post1);
    d2.post = st.at<char>(i_post2);
    d1.lengths = st.at<int64_t>(i_len1);
    d2.lengths = st.at<int64_t>(i_len2);
    fcd_result dout{};
    dout.labels = st.at<uint8_t>(i_lab);
    dout.out_len = st.at<uint32_t>(i_olen);
    dout.status = st.at<int32_t>(i_stat);
    dout.out_stride = out->out_stride;
    dout.ambiguous = st.at<uint32_t>(i_amb);
    CrfInit dc;
    if (is_crf) {
        dc = *crf;
        dc.init1 = st.at<float>(i_init1);
        dc.init2 = st.at<float>(i_init2);
    }
    rc = duplex_dev(h, &d1, &d2, is_crf ? &dc : nullptr, st.at<uint64_t>(i_env), env_stride, beam_size,
                    beam_cut_threshold, collapse_repeats, logadd_mode, &dout);
    if (rc) return rc;
    if (h->overlap_n >= 2) {  // (fcd_set_overlap: the search may sit on an internal stream; the copies back are in the handle's)
        rc = overlap_join(h, h->stream);
        if (rc) return rc;
    }
    return st.fetch();
}
}  // namespace

int fcd_beam_search_duplex_host(fcd_handle *h, const fcd_batch *in1, const fcd_batch *in2,
                                const uint64_t *envelope, int64_t env_stride, int64_t beam_size,
                                float beam_cut_threshold, int collapse_repeats, int logadd_mode,
                                const fcd_result *out) {
    return duplex_host(h, in1, in2, nullptr, envelope, env_stride, beam_size, beam_cut_threshold,
                       collapse_repeats, logadd_mode, out);
}

int fcd_crf_beam_search_duplex_host(fcd_handle *h, const fcd_batch *in1, const float *init1,
                                    int64_t n_init1, int64_t init1_stride, const fcd_batch *in2,
                                    const float *init2, int64_t n_init2, int64_t init2_stride,
                                    const uint64_t *envelope, int64_t env_stride, int64_t beam_size,
                                    float beam_cut_threshold, int logadd_mode, const fcd_result *out) {
    CrfInit c;
    c.init1 = init1; c.n1 = n_init1; c.s1 = init1_stride;
    c.init2 = init2; c.n2 = n_init2; c.s2 = init2_stride;
    return duplex_host(h, in1, in2, &c, envelope, env_stride, beam_size, beam_cut_threshold, 0,
                       logadd_mode, out);
}

// ---- alignment-band estimator (envelope.hip) ----
int fcd_duplex_envelope_dev(fcd_handle *h, int64_t n_pairs,
                            const uint8_t *labels1, const uint32_t *path1, const uint32_t *len1,
                            int64_t stride1, const int64_t *T1, int64_t T1cap,
                            const uint8_t *labels2, const uint32_t *path2, const uint32_t *len2,
                            int64_t stride2, const int64_t *T2, int64_t T2cap,
                            int64_t band, uint64_t *envelope, int64_t env_stride) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (n_pairs < 0 || T1cap < 0 || T2cap < 0 || band < 0) return fail(h, FCD_E_INVALID, "negative size");
    if (n_pairs == 0 || T1cap == 0) return FCD_OK;
    if (!labels1 || !path1 || !len1 || !labels2 || !path2 || !len2 || !envelope)
        return fail(h, FCD_E_INVALID, "null array");
    if (stride1 < T1cap || stride2 < T2cap) return fail(h, FCD_E_INVALID, "label strides shorter than the reads");
    if (env_stride < T1cap) return fail(h, FCD_E_INVALID, "envelope shorter than read 1");
    band = std::min<int64_t>(band, 1 << 20);
    FCD_DEVICE(h);
    // the workspace from its start: behind every overlapping call in flight (the first bytes of `lnbuf` are scratch)
    CallScope sc(h);
    int rc = sc.begin(false, true);
    if (rc) return rc;
    // the DP is sized by the longest labellings actually present, not by the time axes
    char *scratch = nullptr;
    rc = sc.lnbuf(256, &scratch);
    if (rc) return rc;
    uint32_t *d_max = reinterpret_cast<uint32_t *>(scratch);
    uint32_t h_max[2] = {0, 0};
    FCD_HIP(h, hipMemsetAsync(d_max, 0, 8, sc.stream));
    FCD_HIP(h, launch_max_u32(len1, len2, n_pairs, d_max, sc.stream));
    FCD_HIP(h, hipMemcpyAsync(h_max, d_max, 8, hipMemcpyDeviceToHost, sc.stream));
    FCD_HIP(h, hipStreamSynchronize(sc.stream));
    const int64_t L1cap = std::max<int64_t>(1, std::min<int64_t>(h_max[0], T1cap));
    const int64_t L2cap = std::max<int64_t>(1, std::min<int64_t>(h_max[1], T2cap));
    if (L1cap + L2cap > 65535) return fail(h, FCD_E_UNSUPPORTED, "envelope estimator: more than 65535 labels in a pair");
    if (envelope_lds_bytes(L2cap) > 64 * 1024)
        return fail(h, FCD_E_UNSUPPORTED, "envelope estimator: read 2 holds too many labels for the LDS-resident rows");
    const int nchunk = (int)((L2cap + 63) / 64);
    const int64_t dirs_stride = std::max<int64_t>(L1cap * std::max(nchunk, 1) * 2, 2);
    const size_t anchor_bytes = ((size_t)(T1cap + 1) * 4 + 15) & ~(size_t)15;
    const size_t per_pair = (size_t)dirs_stride * 8 + anchor_bytes;
    int64_t chunk = std::max<int64_t>(1, workspace_budget(h) / (int64_t)per_pair);
    chunk = std::min<int64_t>(chunk, n_pairs);
    char *abase = nullptr;
    rc = sc.arena((size_t)chunk * per_pair, &abase);
    if (rc) return rc;
    EnvelopeArgs a;
    a.labels1 = labels1; a.labels2 = labels2; a.path1 = path1; a.path2 = path2;
    a.len1 = len1; a.len2 = len2; a.stride1 = stride1; a.stride2 = stride2;
    a.T1 = T1; a.T2 = T2; a.T1cap = T1cap; a.T2cap = T2cap; a.L2cap = L2cap; a.band = band;
    a.env = envelope; a.env_stride = env_stride;
    a.dirs = reinterpret_cast<uint64_t *>(abase);
    a.dirs_stride = dirs_stride;
    a.nchunk = std::max(nchunk, 1);
    a.anchor = reinterpret_cast<int32_t *>(abase + (size_t)chunk * dirs_stride * 8);
    // anchor slabs are (T1cap + 1) ints apart inside their region
    sc.time();
    for (int64_t b0 = 0; b0 < n_pairs; b0 += chunk)
        FCD_HIP(h, launch_envelope(a, b0, std::min<int64_t>(chunk, n_pairs - b0), sc.stream));
    return sc.finish();
}

int fcd_duplex_envelope_host(fcd_handle *h, int64_t n_pairs,
                             const uint8_t *labels1, const uint32_t *path1, const uint32_t *len1,
                             int64_t stride1, const int64_t *T1, int64_t T1cap,
                             const uint8_t *labels2, const uint32_t *path2, const uint32_t *len2,
                             int64_t stride2, const int64_t *T2, int64_t T2cap,
                             int64_t band, uint64_t *envelope, int64_t env_stride) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    if (n_pairs < 0 || T1cap < 0 || T2cap < 0) return fail(h, FCD_E_INVALID, "negative size");
    if (n_pairs == 0 || T1cap == 0) return FCD_OK;
    if (!labels1 || !path1 || !len1 || !labels2 || !path2 || !len2 || !envelope)
        return fail(h, FCD_E_INVALID, "null array");
    if (stride1 < T1cap || stride2 < T2cap || env_stride < T1cap) return fail(h, FCD_E_INVALID, "strides shorter than the reads");
    FCD_DEVICE(h);
    // one device slab: labels, paths, lengths, row counts of both reads, then the envelope
    Staging st(h);
    const int i_l1 = st.in(labels1, (size_t)n_pairs * stride1), i_l2 = st.in(labels2, (size_t)n_pairs * stride2);
    const int i_p1 = st.in(path1, (size_t)n_pairs * stride1 * 4), i_p2 = st.in(path2, (size_t)n_pairs * stride2 * 4);
    const int i_n1 = st.in(len1, (size_t)n_pairs * 4), i_n2 = st.in(len2, (size_t)n_pairs * 4);
    const int i_t1 = st.in(T1, (size_t)n_pairs * 8), i_t2 = st.in(T2, (size_t)n_pairs * 8);
    const int i_env = st.out(envelope, (size_t)n_pairs * env_stride * 16, true);
    int rc = st.commit();
    if (rc) return rc;
    rc = fcd_duplex_envelope_dev(h, n_pairs, st.at<uint8_t>(i_l1), st.at<uint32_t>(i_p1), st.at<uint32_t>(i_n1), stride1,
                                 st.at<int64_t>(i_t1), T1cap, st.at<uint8_t>(i_l2), st.at<uint32_t>(i_p2),
                                 st.at<uint32_t>(i_n2), stride2, st.at<int64_t>(i_t2), T2cap, band, st.at<uint64_t>(i_env),
                                 env_stride);
    if (rc) return rc;
    return st.fetch();
}

int fcd_logspace_probe_dev(fcd_handle *h, const float *a, const float *b, float *out_add,
                           float *out_ln, int64_t n, int logadd_mode) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (n < 0 || (n > 0 && (!a || !b || !out_add || !out_ln))) return fail(h, FCD_E_INVALID, "null array");
    FCD_DEVICE(h);
    FCD_HIP(h, launch_logspace_probe(a, b, out_add, out_ln, n, logadd_mode, h->stream));
    return FCD_OK;
}

int fcd_debug_glibc235_dev(fcd_handle *h, int which, const float *x, float *y, int64_t n) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (which < 0 || which > 2 || n < 0 || (n > 0 && (!x || !y))) return fail(h, FCD_E_INVALID, "bad argument");
    FCD_DEVICE(h);
    FCD_HIP(h, launch_glibc235_apply(which, x, y, n, h->stream));
    return FCD_OK;
}

int fcd_logadd_sweep_dev(fcd_handle *h, int which, uint32_t first_bits, uint32_t last_bits, uint64_t *counts) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if ((which != 0 && which != 1) || !counts || first_bits > last_bits) return fail(h, FCD_E_INVALID, "bad argument");
    FCD_DEVICE(h);
    FCD_HIP(h, hipMemsetAsync(counts, 0, 24, h->stream));
    FCD_HIP(h, launch_logadd_sweep(which, first_bits, last_bits, reinterpret_cast<unsigned long long *>(counts), h->stream));
    return FCD_OK;
}

int fcd_logadd_latency_probe_dev(fcd_handle *h, int n_chain, int logadd_mode, uint64_t *cycles, float *sink) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (n_chain < 1 || !cycles || !sink) return fail(h, FCD_E_INVALID, "bad argument");
    FCD_DEVICE(h);
    FCD_HIP(h, launch_logadd_chain(n_chain, logadd_mode, cycles, sink, h->stream));
    return FCD_OK;
}

// ---- compact wire format of a shard's results (pack.hip) ----
int64_t fcd_packed_result_bytes(int64_t n_reads, int64_t total_labels, int path_bytes) {
    if (n_reads < 0 || total_labels < 0 || (path_bytes != 2 && path_bytes != 4)) return -1;
    const int64_t b = 16 + 8 * n_reads + ((total_labels + 3) & ~3ll) + total_labels * path_bytes;
    return (b + 15) & ~15ll;
}

int fcd_result_offsets_dev(fcd_handle *h, const uint32_t *out_len, int64_t n_reads, int64_t out_stride,
                           uint64_t *offsets) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (n_reads < 0 || !offsets || (n_reads > 0 && !out_len) || out_stride < 0) return fail(h, FCD_E_INVALID, "bad argument");
    FCD_DEVICE(h);
    CallScope sc(h);
    sc.add(out_len, (size_t)n_reads * 4);
    sc.add(offsets, (size_t)(n_reads + 1) * 8);
    int rc = sc.begin(false, false);
    if (rc) return rc;
    FCD_HIP(h, launch_result_offsets(out_len, n_reads, out_stride, offsets, sc.stream));
    return sc.finish();
}

int fcd_pack_results_dev(fcd_handle *h, const fcd_result *res, int64_t n_reads, int path_bytes,
                         const uint64_t *offsets, uint8_t *buf) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (!res || n_reads < 0 || !offsets || !buf || (path_bytes != 2 && path_bytes != 4))
        return fail(h, FCD_E_INVALID, "bad argument");
    if (n_reads > 0 && (!res->labels || !res->path || !res->out_len)) return fail(h, FCD_E_INVALID, "null labels/path/out_len");
    FCD_DEVICE(h);
    ResultDesc wire = to_desc(res);
    wire.qual = nullptr;  // the wire format carries labels, path, out_len, status
    CallScope sc(h);
    sc.add(wire, n_reads);
    sc.add(offsets, (size_t)(n_reads + 1) * 8);
    int rc = sc.begin(false, false);
    if (rc) return rc;
    if (n_reads == 0) FCD_HIP(h, hipMemsetAsync(buf, 0, 16, sc.stream));
    else FCD_HIP(h, launch_pack(wire, n_reads, path_bytes, offsets, buf, sc.stream));
    return sc.finish();
}

int fcd_unpack_results_dev(fcd_handle *h, const uint8_t *buf, int64_t n_reads, uint64_t *offsets,
                           const fcd_result *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (!buf || n_reads < 0 || !offsets || !out) return fail(h, FCD_E_INVALID, "bad argument");
    if (n_reads == 0) return FCD_OK;
    if (!out->labels || !out->out_len) return fail(h, FCD_E_INVALID, "null labels/out_len");
    FCD_DEVICE(h);
    CallScope sc(h);
    sc.add(to_desc(out), n_reads);
    sc.add(buf, 16 + (size_t)n_reads * 8);
    sc.add(offsets, (size_t)(n_reads + 1) * 8);
    int rc = sc.begin(false, false);
    if (rc) return rc;
    // the buffer's own out_len array (offset 16) gives the read offsets
    FCD_HIP(h, launch_result_offsets(reinterpret_cast<const uint32_t *>(buf + 16), n_reads, out->out_stride, offsets,
                                     sc.stream));
    FCD_HIP(h, launch_unpack(buf, n_reads, offsets, to_desc(out), sc.stream));
    return sc.finish();
}

int fcd_unpack_gathered_dev(fcd_handle *h, const uint8_t *gathered, int64_t stride, int world, const int64_t *first,
                            int64_t n_total, uint64_t *offsets, const fcd_result *out, int32_t *bad) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (!gathered || stride < 16 || world < 1 || !first || n_total < 0 || !offsets || !out || !bad)
        return fail(h, FCD_E_INVALID, "bad argument");
    if (n_total == 0) return FCD_OK;
    if (!out->labels || !out->out_len) return fail(h, FCD_E_INVALID, "null labels/out_len");
    FCD_DEVICE(h);
    CallScope sc(h);
    sc.add(to_desc(out), n_total);
    sc.add(gathered, (size_t)stride * world);
    sc.add(offsets, (size_t)(n_total + world) * 8);
    int rc = sc.begin(false, false);
    if (rc) return rc;
    FCD_HIP(h, launch_unpack_gathered(gathered, stride, world, first, n_total, offsets, to_desc(out), bad, sc.stream));
    return sc.finish();
}

// ---- the lattice of given labellings: CTC forward score (ctc_score.hip), CTC forced alignment (ctc_align.hip), both
// under a CRF model (crf_lattice.hip), the CTC substitution posteriors and edit likelihoods (ctc_posterior.hip), and the
// substitution posteriors under a CRF model (crf_posterior.hip) ----
int fcd_debug_set_align_workspace_cap(fcd_handle *h, int64_t bytes) {
    if (!h || bytes < 0) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    h->align_ws_cap = bytes;
    return FCD_OK;
}

namespace {
// One fcd_{ctc,crf}_{score,align,posterior,edits}_{dev,host} call: the score
// writes `logp`, the alignment `out`, the posteriors `post`, the edit likelihoods `edits`.
struct LatticeCall {
    bool crf, align;
    const fcd_batch *in;
    const fcd_labellings *y;
    int64_t band;
    int collapse;  // (CTC; a CRF model emits at every label)
    const float *init;  // (CRF)
    int64_t n_init, init_stride;
    double *logp;
    const fcd_alignment *out;
    bool posterior = false;
    const fcd_posterior *post = nullptr;
    bool edit = false;
    const fcd_edits *edits = nullptr;
    bool occupancy = false;
    const fcd_occupancy *occ = nullptr;
    bool wide = false;  // (CTC occupancy) fcd_set_ctc_occupancy_wide: windows beyond the registers walk score_lds_kernel
    bool crf_wide = false;  // (CRF score, occupancy) fcd_set_crf_lattice_wide: windows beyond 512 states walk in LDS
};

// the call is one of those the CRF switch covers AND its window is beyond the registers: every other call is what it is
// with the switch off (in and y checked by then)
bool crf_wide_call(const LatticeCall &c) {
    return c.crf && c.crf_wide && !c.align && !c.posterior && !c.edit &&
           crf_lattice_is_wide(c.in->T, c.y->stride, std::min<int64_t>(c.band, 1ll << 28));
}

// floats from the first to the last element the call may address in out->occ (0: none)
size_t occupancy_span(const fcd_batch *in, const fcd_labellings *y, const fcd_occupancy *o) {
    if (in->n_reads <= 0 || in->T <= 0) return 0;
    return (size_t)((in->n_reads * y->n_hyp - 1) * o->stride_row + (in->T - 1) * o->stride_t + in->S * in->N);
}

int lattice_check(fcd_handle *h, const LatticeCall &c) {
    if (c.align && !c.out) return fail(h, FCD_E_INVALID, "null alignment");
    if (c.posterior && !c.post) return fail(h, FCD_E_INVALID, "null posterior");
    if (c.edit && !c.edits) return fail(h, FCD_E_INVALID, c.crf ? "crf_edits: null output" : "ctc_edits: null output");
    const std::string occ_who = c.crf ? "crf_occupancy" : (c.wide ? "ctc_occupancy_wide" : "ctc_occupancy");
    if (c.occupancy && !c.occ) return fail(h, FCD_E_INVALID, (occ_who + ": null output").c_str());
    const fcd_batch *in = c.in;
    const fcd_labellings *y = c.y;
    int rc = check_batch(h, in, c.crf);
    if (rc) return rc;
    if (c.crf) {
        if (!c.init || c.n_init < 1) return fail(h, FCD_E_INVALID, "init_state missing");
        if (c.init_stride < 0) return fail(h, FCD_E_INVALID, "negative stride");
    } else if (in->S != 1) {
        return fail(h, FCD_E_INVALID, "ctc_score: S must be 1 (CRF models are not scored)");
    }
    if (!y) return fail(h, FCD_E_INVALID, "null labellings");
    if (y->n_hyp < 1) return fail(h, FCD_E_INVALID, "n_hyp must be >= 1");
    if (c.band < 0) return fail(h, FCD_E_INVALID, "band must be >= 0");
    if (c.band > 0 && !y->path) return fail(h, FCD_E_INVALID, "a band needs the labellings' path");
    if (y->stride < 0) return fail(h, FCD_E_INVALID, "negative stride");
    if (in->n_reads > 0 && (!y->labels || !y->len ||
                            !(c.occupancy ? (const void *)c.occ->occ : c.edit ? (const void *)c.edits->deletion : c.posterior ? (const void *)c.post->post
                              : c.align ? (const void *)c.out->start : (const void *)c.logp)))
        return fail(h, FCD_E_INVALID, c.occupancy ? (c.crf ? "crf_occupancy: null labels/len/occ" : c.wide ? "ctc_occupancy_wide: null labels/len/occ" : "ctc_occupancy: null labels/len/occ") : c.edit ? (c.crf ? "crf_edits: null labels/len/deletion" : "ctc_edits: null labels/len/deletion") : c.posterior ? "null labels/len/post"
                                      : c.align ? "null labels/len/start" : "null labels/len/logp");
    if (c.edit && in->n_reads > 0 && !c.edits->insertion) return fail(h, FCD_E_INVALID, c.crf ? "crf_edits: null insertion" : "ctc_edits: null insertion");
    if (in->n_reads * y->n_hyp >= (1ll << 31)) return fail(h, FCD_E_UNSUPPORTED, "more than 2^31 labellings in one call");
    if (c.crf && crf_wide_call(c)) {
        const std::string who = c.occupancy ? "crf_occupancy_wide" : "crf_score_wide";
        size_t lds = 0;
        switch (crf_lattice_wide_unsupported(in->T, in->S, in->N, y->stride, std::min<int64_t>(c.band, 1ll << 28), c.occupancy, &lds)) {
        case 1: return fail(h, FCD_E_UNSUPPORTED, (who + (c.band > 0 ? ": the band's window exceeds the 4096 states of 64 cells per lane: use a narrower band"
                                                                     : ": the exact lattice exceeds the 4096 states of 64 cells per lane: use a band")).c_str());
        case 2: return fail(h, FCD_E_UNSUPPORTED, (who + ": more than 8 labels besides the blank").c_str());
        case 3: return fail(h, FCD_E_UNSUPPORTED, (who + ": S must be below 2^24 - 1").c_str());
        case 4: return fail(h, FCD_E_UNSUPPORTED, (who + ": the labelling, the tile, the window's three rows" + (c.occupancy ? " and the S * N accumulation row" : "") +
                                                   " do not fit the 160 KiB of LDS (4 (min(T, stride) + 1) + 4480 + 768 ceil(states / 64)" +
                                                   (c.occupancy ? " + 4 S N" : "") + " = " + std::to_string(lds) + " bytes): use a band or a smaller stride").c_str());
        default: break;
        }
    } else if (c.crf) {
        switch (crf_lattice_unsupported(in->T, in->S, y->stride, std::min<int64_t>(c.band, 1ll << 28))) {
        case 1: return fail(h, FCD_E_UNSUPPORTED, c.band > 0 ? "crf lattice: the band's window exceeds 512 states: use a narrower band"
                                                             : "crf lattice: the exact lattice exceeds 512 states: use a band");
        case 2: return fail(h, FCD_E_UNSUPPORTED, "crf lattice: S must be below 2^24 - 1");
        case 3: return fail(h, FCD_E_UNSUPPORTED, "crf lattice: labellings beyond 15263 labels do not fit the 64 KiB of LDS: use a smaller stride");
        default: break;
        }
    } else if (!c.wide && !ctc_score_supported(in->T, y->stride, c.band)) {  // (wide: its own limits below, no looser)
        return fail(h, FCD_E_UNSUPPORTED, c.band > 0 ? "ctc_score: the band's window does not fit the 160 KiB of LDS: use a narrower band"
                                                     : "ctc_score: the exact lattice does not fit the 160 KiB of LDS: use a band");
    }
    if (c.align && in->n_reads > 0 && !c.out->count) return fail(h, FCD_E_INVALID, "null count");
    if (c.occupancy) {  // (a CTC batch has S = 1: its rows are N floats)
        if (c.occ->stride_row < 0 || c.occ->stride_t < in->S * in->N)
            return fail(h, FCD_E_INVALID, (occ_who + (c.crf ? ": stride_t must hold a dense (S, N) row, stride_row must not be negative"
                                                            : ": stride_t must hold a dense row of N, stride_row must not be negative")).c_str());
        if (c.occ->accumulate != 0 && c.occ->accumulate != 1) return fail(h, FCD_E_INVALID, (occ_who + ": accumulate must be 0 or 1").c_str());
        {  // every labelling's block to itself: whole blocks apart (read-major), or rows apart with the blocks interleaved (time-major)
            const int64_t rows = in->n_reads * y->n_hyp, SN = in->S * in->N, sr = c.occ->stride_row, st = c.occ->stride_t;
            const bool apart = sr >= (in->T - 1) * st + SN, interleaved = sr >= SN && st >= (rows - 1) * sr + SN;
            if (rows > 1 && in->T > 0 && !apart && !interleaved)
                return fail(h, FCD_E_INVALID, (occ_who + ": the labellings' blocks overlap (stride_row, stride_t)").c_str());
        }
    }
    if (c.occupancy && c.crf && crf_wide_call(c)) {  // (its limits: above)
    } else if (c.occupancy && c.crf) {
        switch (crf_occupancy_unsupported(in->T, in->S, in->N, y->stride)) {
        case 2: return fail(h, FCD_E_UNSUPPORTED, "crf_occupancy: more than 8 labels besides the blank");
        case 6: return fail(h, FCD_E_UNSUPPORTED, "crf_occupancy: the labelling and the S * N accumulation row do not fit the 160 KiB "
                                                  "of LDS (4 (min(T, stride) + 1) + 4 S N + 4480 bytes)");
        default: break;
        }
    } else if (c.crf && (c.posterior || c.edit)) {
        int64_t fit = 0;
        const int64_t bnd = std::min<int64_t>(c.band, 1ll << 28);
        const std::string who = c.edit ? "crf_edits" : "crf_posterior";
        switch (crf_posterior_unsupported(in->T, in->S, in->N, y->stride, bnd, &fit)) {  // (one set of limits: the same kernels)
        case 1: return fail(h, FCD_E_UNSUPPORTED, (who + ": a model state of this depth holds windows of " +
                                                   std::to_string(fit) + " states: use a band of at most " +
                                                   std::to_string((fit - 1) / 2)).c_str());
        case 2: return fail(h, FCD_E_UNSUPPORTED, (who + ": more than 8 labels besides the blank").c_str());
        case 4: return fail(h, FCD_E_UNSUPPORTED, (who + ": S must be a power of N - 1 (the model state is the last labels)").c_str());
        case 5: return fail(h, FCD_E_UNSUPPORTED, (who + ": the model state holds more labels than the kernels carry "
                                                   "(S = (N - 1)^m with m <= 6 and m (N - 1) <= 24, or m <= 4 at N = 3)").c_str());
        default: break;
        }
    } else if (c.occupancy && c.wide) {
        switch (ctc_occupancy_wide_unsupported(in->T, y->stride, c.band, in->N)) {
        case 2: return fail(h, FCD_E_UNSUPPORTED, "ctc_occupancy_wide: more than 8 labels besides the blank");
        case 3: return fail(h, FCD_E_UNSUPPORTED, "ctc_occupancy_wide: labellings beyond 28480 labels do not fit the 64 KiB of LDS of a "
                                                  "register-resident window: use a smaller stride");
        case 4: return fail(h, FCD_E_UNSUPPORTED, c.band > 0 ? "ctc_occupancy_wide: the band's window exceeds the 10240 states of 1024 work-items: use a narrower band"
                                                             : "ctc_occupancy_wide: the exact lattice exceeds the 10240 states of 1024 work-items: use a band");
        case 5: return fail(h, FCD_E_UNSUPPORTED, "ctc_occupancy_wide: the labelling, the tile, the two rows of the window and the reduction "
                                                  "words do not fit the 160 KiB of LDS (2 min(T, stride) + 8 states + 9152 bytes): "
                                                  "use a band or a smaller stride");
        default: break;
        }
    } else if (c.edit || c.posterior || c.occupancy) {  // (one set of limits: all walk ctc_posterior.hip's register-resident window)
        const std::string who = c.occupancy ? occ_who : c.edit ? "ctc_edits" : "ctc_posterior";
        switch (ctc_posterior_unsupported(in->T, y->stride, c.band, in->N)) {
        case 1: return fail(h, FCD_E_UNSUPPORTED, (who + (c.band > 0 ? ": the band's window exceeds 510 states: use a narrower band"
                                                                     : ": the exact lattice exceeds 510 states: use a band")).c_str());
        case 2: return fail(h, FCD_E_UNSUPPORTED, (who + ": more than 8 labels besides the blank").c_str());
        case 3: return fail(h, FCD_E_UNSUPPORTED, (who + ": labellings beyond 28480 labels do not fit the 64 KiB of LDS: use a smaller stride").c_str());
        default: break;
        }
    }
    return FCD_OK;
}

void add_labellings(CallScope &sc, const LatticeCall &c, size_t n_rows) {
    sc.add(c.y->labels, n_rows * (size_t)c.y->stride);
    sc.add(c.y->len, n_rows * 4);
    sc.add(c.y->n_valid, (size_t)c.in->n_reads * 4);
    sc.add(c.y->path, n_rows * (size_t)c.y->stride * 4);
}

// (the drivers: a checked call with reads in it, on the handle's device)
int lattice_score(fcd_handle *h, const LatticeCall &c) {
    const fcd_batch *in = c.in;
    const fcd_labellings *y = c.y;
    const size_t n_rows = (size_t)in->n_reads * (size_t)y->n_hyp;
    CallScope sc(h);
    add_labellings(sc, c, n_rows);
    sc.add(c.logp, n_rows * 8);
    int rc = sc.begin(false, false);
    if (rc) return rc;
    const ScoreDesc yd{y->labels, y->len, y->n_valid, c.band > 0 ? y->path : nullptr, y->n_hyp, y->stride};
    const int64_t bnd = std::min<int64_t>(c.band, 1ll << 28);
    sc.time();
    if (c.crf && crf_wide_call(c))
        FCD_HIP(h, launch_crf_score_wide(to_desc(in, true), yd, c.init, c.n_init, c.init_stride, bnd, c.logp, sc.stream));
    else if (c.crf)
        FCD_HIP(h, launch_crf_score(to_desc(in, true), yd, c.init, c.n_init, c.init_stride, bnd, c.logp, sc.stream));
    else
        FCD_HIP(h, launch_ctc_score(to_desc(in, false), yd, c.collapse, bnd, c.logp, sc.stream));
    return sc.finish();
}

// What lattice_align and lattice_posterior share: per-labelling workspace (back-pointers, stored forward rows) of
// row_bytes each.  Whole reads per launch, as many as `cap` bytes hold (at least one), every launch in the same memory, one
// after the other on the stream; logp lent from the workspace when the caller wants none.  add_outputs(sc): the arrays the
// call writes; launch(d, yd, r0, row0, logp, ws, stream): one group -- reads r0 .., labellings row0 .., its slice of logp.
using GroupLaunch = std::function<hipError_t(const BatchDesc &, const ScoreDesc &, int64_t, int64_t, double *, unsigned char *, hipStream_t)>;
int lattice_grouped(fcd_handle *h, const LatticeCall &c, size_t row_bytes, int64_t cap, double *out_logp,
                    const std::function<void(CallScope &)> &add_outputs, const GroupLaunch &launch) {
    const fcd_batch *in = c.in;
    const fcd_labellings *y = c.y;
    const size_t n_rows = (size_t)in->n_reads * (size_t)y->n_hyp;
    const int64_t read_bytes = (int64_t)(row_bytes * (size_t)y->n_hyp);
    const int64_t group = std::max<int64_t>(1, std::min<int64_t>(in->n_reads, cap / read_bytes));
    const size_t o_logp = (size_t)group * (size_t)read_bytes;
    CallScope sc(h);
    add_labellings(sc, c, n_rows);
    add_outputs(sc);
    sc.add(out_logp, n_rows * 8);
    int rc = sc.begin(false, true);  // (exclusive: the workspace from its start, behind every overlapping call in flight)
    if (rc) return rc;
    char *ws = nullptr;
    rc = sc.arena(o_logp + (out_logp ? 0 : n_rows * 8), &ws);
    if (rc) return rc;
    double *logp = out_logp ? out_logp : reinterpret_cast<double *>(ws + o_logp);
    const int64_t esz = in->dtype == FCD_DTYPE_F32 ? 4 : 2;
    sc.time();
    for (int64_t r0 = 0; r0 < in->n_reads; r0 += group) {
        const int64_t row0 = r0 * y->n_hyp;
        BatchDesc d = to_desc(in, c.crf);
        d.post = reinterpret_cast<const float *>(reinterpret_cast<const char *>(in->post) + r0 * in->stride_read * esz);
        d.lengths = in->lengths ? in->lengths + r0 : nullptr;
        d.n_reads = std::min(group, in->n_reads - r0);
        const ScoreDesc yd{y->labels + row0 * y->stride, y->len + row0, y->n_valid ? y->n_valid + r0 : nullptr,
                           c.band > 0 ? y->path + row0 * y->stride : nullptr, y->n_hyp, y->stride};
        FCD_HIP(h, launch(d, yd, r0, row0, logp + row0, reinterpret_cast<unsigned char *>(ws), sc.stream));
    }
    return sc.finish();
}

int lattice_align(fcd_handle *h, const LatticeCall &c) {
    const fcd_batch *in = c.in;
    const fcd_labellings *y = c.y;
    const fcd_alignment *out = c.out;
    const size_t cells = (size_t)in->n_reads * (size_t)y->n_hyp * (size_t)y->stride;
    // (the CTC kernels size their rows by the band as given, the CRF kernels by the band the launch gets)
    const int64_t bnd = std::min<int64_t>(c.band, 1ll << 28);
    const size_t row_bytes = c.crf ? crf_align_row_bytes(in->T, y->stride, bnd) : ctc_align_row_bytes(in->T, y->stride, c.band);
    const int64_t cap = h->align_ws_cap > 0 ? h->align_ws_cap : std::min<int64_t>(4ll << 30, workspace_budget(h));
    return lattice_grouped(
        h, c, row_bytes, cap, out->logp,
        [&](CallScope &sc) {
            sc.add(out->start, cells * 4);
            sc.add(out->count, cells * 4);
            sc.add(out->qual, cells * 4);
        },
        [&](const BatchDesc &d, const ScoreDesc &yd, int64_t r0, int64_t row0, double *logp, unsigned char *bp, hipStream_t stream) {
            const AlignOut od{out->start + row0 * y->stride, out->count + row0 * y->stride,
                              out->qual ? out->qual + row0 * y->stride : nullptr, logp};
            return c.crf ? launch_crf_align(d, yd, c.init + r0 * c.init_stride, c.n_init, c.init_stride, bnd, od, bp, stream)
                         : launch_ctc_align(d, yd, c.collapse, bnd, od, bp, stream);
        });
}

int lattice_posterior(fcd_handle *h, const LatticeCall &c) {
    const fcd_batch *in = c.in;
    const fcd_labellings *y = c.y;
    const fcd_posterior *out = c.post;
    const size_t per_row = (size_t)y->stride * ((size_t)in->N - 1);  // post entries of one labelling
    const int64_t bnd = std::min<int64_t>(c.band, 1ll << 28);
    // (the CTC kernels size their rows by the band as given, the CRF kernels by the band the launch gets)
    const size_t row_bytes = c.crf ? crf_posterior_row_bytes(in->T, in->S, in->N, y->stride, bnd) : ctc_posterior_row_bytes(in->T, y->stride, c.band);
    return lattice_grouped(
        h, c, row_bytes, std::min<int64_t>(4ll << 30, workspace_budget(h)), out->logp,
        [&](CallScope &sc) { sc.add(out->post, (size_t)in->n_reads * (size_t)y->n_hyp * per_row * 4); },
        [&](const BatchDesc &d, const ScoreDesc &yd, int64_t r0, int64_t row0, double *logp, unsigned char *alpha, hipStream_t stream) {
            float *post = out->post + (size_t)row0 * per_row;
            return c.crf ? launch_crf_posterior(d, yd, c.init + r0 * c.init_stride, c.n_init, c.init_stride, bnd, post, logp, alpha, stream)
                         : launch_ctc_posterior(d, yd, c.collapse, bnd, post, logp, alpha, stream);
        });
}

int lattice_edits(fcd_handle *h, const LatticeCall &c) {
    const fcd_batch *in = c.in;
    const fcd_labellings *y = c.y;
    const fcd_edits *out = c.edits;
    const size_t nc = (size_t)in->N - 1, n_rows = (size_t)in->n_reads * (size_t)y->n_hyp;
    const size_t del_row = (size_t)y->stride, ins_row = ((size_t)y->stride + 1) * nc;  // entries of one labelling
    const int64_t bnd = std::min<int64_t>(c.band, 1ll << 28);
    // (the CTC kernels size their rows by the band as given, the CRF kernels by the band the launch gets)
    const size_t row_bytes = c.crf ? crf_posterior_row_bytes(in->T, in->S, in->N, y->stride, bnd) : ctc_posterior_row_bytes(in->T, y->stride, c.band);
    return lattice_grouped(
        h, c, row_bytes, std::min<int64_t>(4ll << 30, workspace_budget(h)), out->logp,
        [&](CallScope &sc) {
            sc.add(out->deletion, n_rows * del_row * 4);
            sc.add(out->insertion, n_rows * ins_row * 4);
        },
        [&](const BatchDesc &d, const ScoreDesc &yd, int64_t r0, int64_t row0, double *logp, unsigned char *alpha, hipStream_t stream) {
            float *del = out->deletion + (size_t)row0 * del_row, *ins = out->insertion + (size_t)row0 * ins_row;
            return c.crf ? launch_crf_edits(d, yd, c.init + r0 * c.init_stride, c.n_init, c.init_stride, bnd, del, ins, logp, alpha, stream)
                         : launch_ctc_edits(d, yd, c.collapse, bnd, del, ins, logp, alpha, stream);
        });
}

int lattice_occupancy(fcd_handle *h, const LatticeCall &c) {
    const fcd_batch *in = c.in;
    const fcd_labellings *y = c.y;
    const fcd_occupancy *out = c.occ;
    const int64_t bnd = std::min<int64_t>(c.band, 1ll << 28);
    // (the CTC kernels size their rows by the band as given, the CRF kernels by the band the launch gets)
    const bool crf_wide = crf_wide_call(c);
    const size_t row_bytes = crf_wide ? crf_lattice_wide_row_bytes(in->T, y->stride, bnd)
                             : c.crf  ? crf_occupancy_row_bytes(in->T, y->stride, bnd)
                             : c.wide ? ctc_occupancy_wide_row_bytes(in->T, y->stride, c.band)
                                      : ctc_posterior_row_bytes(in->T, y->stride, c.band);
    return lattice_grouped(
        h, c, row_bytes, std::min<int64_t>(4ll << 30, workspace_budget(h)), out->logp,
        [&](CallScope &sc) { sc.add(out->occ, occupancy_span(in, y, out) * 4); },
        [&](const BatchDesc &d, const ScoreDesc &yd, int64_t r0, int64_t row0, double *logp, unsigned char *alpha, hipStream_t stream) {
            const OccupancyDesc od{out->occ + row0 * out->stride_row, out->stride_row, out->stride_t, out->scale, out->accumulate};
            return crf_wide ? launch_crf_occupancy_wide(d, yd, c.init + r0 * c.init_stride, c.n_init, c.init_stride, bnd, od, logp, alpha, stream)
                   : c.crf  ? launch_crf_occupancy(d, yd, c.init + r0 * c.init_stride, c.n_init, c.init_stride, bnd, od, logp, alpha, stream)
                         : c.wide ? launch_ctc_occupancy_wide(d, yd, c.collapse, bnd, od, logp, alpha, stream)
                                  : launch_ctc_occupancy(d, yd, c.collapse, bnd, od, logp, alpha, stream);
        });
}

int lattice_run(fcd_handle *h, const LatticeCall &c) {
    if (c.occupancy) return lattice_occupancy(h, c);
    if (c.edit) return lattice_edits(h, c);
    return c.posterior ? lattice_posterior(h, c) : (c.align ? lattice_align(h, c) : lattice_score(h, c));
}

int lattice_dev(fcd_handle *h, const LatticeCall &c) {
    int rc = lattice_check(h, c);
    if (rc) return rc;
    if (c.in->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);
    return lattice_run(h, c);
}

// host arrays: staged in the order post, init, lengths, the labellings, the outputs; the device call runs on the handle's
// stream (no fcd_set_overlap), so the copy-back needs no join
int lattice_host(fcd_handle *h, const LatticeCall &c) {
    int rc = lattice_check(h, c);
    if (rc) return rc;
    const fcd_batch *in = c.in;
    const fcd_labellings *y = c.y;
    if (in->n_reads == 0) return FCD_OK;
    if (in->stride_read < 0 || in->stride_t < 0 || (c.crf && in->stride_s < 0) || in->stride_n < 0)
        return fail(h, FCD_E_INVALID, "negative stride");
    FCD_DEVICE(h);
    const size_t B = (size_t)in->n_reads, n_rows = B * (size_t)y->n_hyp, cells = n_rows * (size_t)y->stride;
    Staging st(h);
    // the posteriors keep their strides: the span from the first to the last addressed element is staged as it is
    const int i_post = st.in(in->post, (size_t)span_elems(in, c.crf) * (in->dtype == FCD_DTYPE_F32 ? 4 : 2));
    const int i_init = st.in(c.crf ? c.init : nullptr, (size_t)((in->n_reads - 1) * c.init_stride + c.n_init) * 4);
    const int i_len = st.in(in->lengths, B * 8);
    const int i_lab = st.in(y->labels, cells);
    const int i_ylen = st.in(y->len, n_rows * 4);
    const int i_nv = st.in(y->n_valid, B * 4);
    const int i_path = st.in(c.band > 0 ? y->path : nullptr, cells * 4);
    // (alignment entries the kernel does not write -- k >= len -- come back as 0)
    const int i_start = c.align ? st.out(c.out->start, cells * 4, true) : -1;
    const int i_count = c.align ? st.out(c.out->count, cells * 4, true) : -1;
    const int i_qual = c.align ? st.out(c.out->qual, cells * 4, true) : -1;
    // (posterior entries the kernel does not write -- k >= len -- come back as 0)
    const int i_sub = c.posterior ? st.out(c.post->post, cells * ((size_t)in->N - 1) * 4, true) : -1;
    // (edit entries the kernel does not write -- k >= len, g > len -- come back as 0)
    const int i_del = c.edit ? st.out(c.edits->deletion, cells * 4, true) : -1;
    const int i_ins = c.edit ? st.out(c.edits->insertion, (cells + n_rows) * ((size_t)in->N - 1) * 4, true) : -1;
    // (the occupancies are added to what the block holds, and most of it may stay untouched: it travels both ways)
    const int i_occ = c.occupancy ? st.inout(c.occ->occ, occupancy_span(in, y, c.occ) * 4) : -1;
    const int i_logp = st.out(c.occupancy ? c.occ->logp : c.edit ? c.edits->logp : c.posterior ? c.post->logp : (c.align ? c.out->logp : c.logp), n_rows * 8);
    rc = st.commit();
    if (rc) return rc;
    fcd_batch din = *in;
    din.post = st.at<char>(i_post);
    din.lengths = st.at<int64_t>(i_len);
    fcd_labellings dy = *y;
    dy.labels = st.at<uint8_t>(i_lab);
    dy.len = st.at<uint32_t>(i_ylen);
    dy.n_valid = st.at<uint32_t>(i_nv);
    dy.path = st.at<uint32_t>(i_path);
    const fcd_alignment dout{st.at<uint32_t>(i_start), st.at<uint32_t>(i_count), st.at<float>(i_qual), st.at<double>(i_logp)};
    LatticeCall d = c;
    d.in = &din;
    d.y = &dy;
    d.init = st.at<float>(i_init);
    d.logp = st.at<double>(i_logp);
    d.out = &dout;
    const fcd_posterior dpost{st.at<float>(i_sub), st.at<double>(i_logp)};
    d.post = &dpost;
    const fcd_edits dedits{st.at<float>(i_del), st.at<float>(i_ins), st.at<double>(i_logp)};
    d.edits = &dedits;
    fcd_occupancy docc{};
    if (c.occupancy) {
        docc = *c.occ;
        docc.occ = st.at<float>(i_occ);
        docc.logp = st.at<double>(i_logp);
        d.occ = &docc;
    }
    rc = lattice_run(h, d);
    if (rc) return rc;
    return st.fetch();
}
}  // namespace

int fcd_ctc_score_dev(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                      double *logp) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    return lattice_dev(h, LatticeCall{false, false, in, y, band, collapse_repeats != 0, nullptr, 0, 0, logp, nullptr});
}

int fcd_ctc_score_host(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                       double *logp) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    return lattice_host(h, LatticeCall{false, false, in, y, band, collapse_repeats != 0, nullptr, 0, 0, logp, nullptr});
}

int fcd_ctc_align_dev(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                      const fcd_alignment *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    return lattice_dev(h, LatticeCall{false, true, in, y, band, collapse_repeats != 0, nullptr, 0, 0, nullptr, out});
}

int fcd_ctc_align_host(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                       const fcd_alignment *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    return lattice_host(h, LatticeCall{false, true, in, y, band, collapse_repeats != 0, nullptr, 0, 0, nullptr, out});
}

int fcd_ctc_posterior_dev(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                          const fcd_posterior *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    return lattice_dev(h, LatticeCall{false, false, in, y, band, collapse_repeats != 0, nullptr, 0, 0, nullptr, nullptr, true, out});
}

int fcd_ctc_posterior_host(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                           const fcd_posterior *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    return lattice_host(h, LatticeCall{false, false, in, y, band, collapse_repeats != 0, nullptr, 0, 0, nullptr, nullptr, true, out});
}

int fcd_ctc_edits_dev(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                      const fcd_edits *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    return lattice_dev(h, LatticeCall{false, false, in, y, band, collapse_repeats != 0, nullptr, 0, 0, nullptr, nullptr, false, nullptr, true, out});
}

int fcd_ctc_edits_host(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                       const fcd_edits *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    return lattice_host(h, LatticeCall{false, false, in, y, band, collapse_repeats != 0, nullptr, 0, 0, nullptr, nullptr, false, nullptr, true, out});
}

int fcd_crf_score_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                      const fcd_labellings *y, int64_t band, double *logp) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    LatticeCall c{true, false, in, y, band, 0, init, n_init, init_stride, logp, nullptr};
    c.crf_wide = h->crf_wide;
    return lattice_dev(h, c);
}

int fcd_crf_score_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                       const fcd_labellings *y, int64_t band, double *logp) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    LatticeCall c{true, false, in, y, band, 0, init, n_init, init_stride, logp, nullptr};
    c.crf_wide = h->crf_wide;
    return lattice_host(h, c);
}

int fcd_crf_align_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                      const fcd_labellings *y, int64_t band, const fcd_alignment *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    return lattice_dev(h, LatticeCall{true, true, in, y, band, 0, init, n_init, init_stride, nullptr, out});
}

int fcd_crf_align_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                       const fcd_labellings *y, int64_t band, const fcd_alignment *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    return lattice_host(h, LatticeCall{true, true, in, y, band, 0, init, n_init, init_stride, nullptr, out});
}

int fcd_crf_posterior_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                          const fcd_labellings *y, int64_t band, const fcd_posterior *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    return lattice_dev(h, LatticeCall{true, false, in, y, band, 0, init, n_init, init_stride, nullptr, nullptr, true, out});
}

int fcd_crf_posterior_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                           const fcd_labellings *y, int64_t band, const fcd_posterior *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    return lattice_host(h, LatticeCall{true, false, in, y, band, 0, init, n_init, init_stride, nullptr, nullptr, true, out});
}

int fcd_crf_edits_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                      const fcd_labellings *y, int64_t band, const fcd_edits *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    return lattice_dev(h, LatticeCall{true, false, in, y, band, 0, init, n_init, init_stride, nullptr, nullptr, false, nullptr, true, out});
}

int fcd_crf_edits_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                       const fcd_labellings *y, int64_t band, const fcd_edits *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    return lattice_host(h, LatticeCall{true, false, in, y, band, 0, init, n_init, init_stride, nullptr, nullptr, false, nullptr, true, out});
}

int fcd_crf_occupancy_dev(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                          const fcd_labellings *y, int64_t band, const fcd_occupancy *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    LatticeCall c{true, false, in, y, band, 0, init, n_init, init_stride, nullptr, nullptr};
    c.occupancy = true;
    c.crf_wide = h->crf_wide;
    c.occ = out;
    return lattice_dev(h, c);
}

int fcd_crf_occupancy_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init, int64_t init_stride,
                           const fcd_labellings *y, int64_t band, const fcd_occupancy *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    LatticeCall c{true, false, in, y, band, 0, init, n_init, init_stride, nullptr, nullptr};
    c.occupancy = true;
    c.crf_wide = h->crf_wide;
    c.occ = out;
    return lattice_host(h, c);
}

int fcd_ctc_occupancy_dev(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                          const fcd_occupancy *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    LatticeCall c{false, false, in, y, band, collapse_repeats != 0, nullptr, 0, 0, nullptr, nullptr};
    c.occupancy = true;
    c.wide = h->occ_wide;
    c.occ = out;
    return lattice_dev(h, c);
}

int fcd_ctc_occupancy_host(fcd_handle *h, const fcd_batch *in, const fcd_labellings *y, int collapse_repeats, int64_t band,
                           const fcd_occupancy *out) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);  // staging .. copy-back, see run_host
    LatticeCall c{false, false, in, y, band, collapse_repeats != 0, nullptr, 0, 0, nullptr, nullptr};
    c.occupancy = true;
    c.wide = h->occ_wide;
    c.occ = out;
    return lattice_host(h, c);
}

}  // extern "C"

// ---- *_host: stage host buffers through device memory, run the *_dev path, copy back -------
namespace fcd {

// Checks shared by every host-side entry of the four 1D searches.
int host_check(fcd_handle *h, const fcd_batch *in, const fcd_result *out, const HostCall &c) {
    const bool crf = c.op == HostOp::CrfBeam || c.op == HostOp::CrfGreedy;
    int rc = check_batch(h, in, crf);
    if (rc) return rc;
    rc = check_result(h, in, out, c.op != HostOp::Viterbi);
    if (rc) return rc;
    if (in->stride_read < 0 || in->stride_t < 0 || in->stride_n < 0 || (crf && in->stride_s < 0))
        return fail(h, FCD_E_UNSUPPORTED, "negative strides: pass a contiguous copy");
    if (crf && (!c.init || c.n_init < 1)) return fail(h, FCD_E_INVALID, "init_state missing");
    return FCD_OK;
}

// Lays the call out in h->stage (inputs first, then the fixed-stride result arrays) and uploads the inputs on
// h->stream.  `shape` says which result arrays are wanted (non-null members) and their stride; *din / *dout
// receive the device-side batch and result.  Small calls (the per-read drop-in functions: a few hundred KB) go
// through a page-locked mirror of the staging area when allow_mirror: ONE DMA in (and ONE out in host_download)
// instead of a runtime-staged copy per array from pageable memory; large batches are copied straight from / to
// the caller's arrays (an extra host pass would cost more).
int host_upload(fcd_handle *h, const fcd_batch *in, const fcd_result *shape, const HostCall &c, bool allow_mirror,
                HostStage *st, fcd_batch *din, fcd_result *dout) {
    const bool crf = c.op == HostOp::CrfBeam || c.op == HostOp::CrfGreedy;
    const int64_t B = in->n_reads;
    st->B = B;
    st->n_in = (size_t)span_elems(in, crf);
    st->n_rows = (size_t)B * (size_t)(c.n_best > 0 ? c.n_best : 1);
    st->n_out = st->n_rows * (size_t)shape->out_stride;
    st->n_init = crf ? (size_t)((B - 1) * c.init_stride + c.n_init) : 0;
    size_t used = 0;
    auto reserve = [&](size_t bytes) {
        size_t off = (used + 255) & ~(size_t)255;
        used = off + std::max<size_t>(bytes, 4);
        return off;
    };
    const size_t esz = in->dtype == FCD_DTYPE_F32 ? 4 : 2;  // bytes per posterior element
    st->o_in = reserve(st->n_in * esz);
    st->o_len = reserve(in->lengths ? (size_t)B * 8 : 0);
    st->o_init = reserve(st->n_init * 4);
    st->o_lab = reserve(st->n_out);
    st->o_path = reserve(shape->path ? st->n_out * 4 : 0);
    st->o_qual = reserve(shape->qual ? st->n_out * 4 : 0);
    st->o_olen = reserve(st->n_rows * 4);
    st->o_stat = reserve((size_t)B * 4);
    st->want_amb = shape->ambiguous && (c.op == HostOp::Beam || c.op == HostOp::CrfBeam);
    st->o_amb = reserve(st->want_amb ? (size_t)B * 8 : 0);
    st->o_score = reserve(c.n_best > 0 ? st->n_rows * 4 : 0);
    st->o_nhyp = reserve(c.n_best > 0 ? (size_t)B * 4 : 0);
    st->used = used;
    const bool mirror = allow_mirror && used <= ((size_t)4 << 20);
    st->mirror = mirror;

    int rc = ensure(h, &h->stage, &h->stage_bytes, used);
    if (rc) return rc;
    char *base = reinterpret_cast<char *>(h->stage);
    if (mirror) {
        if (h->pin_bytes < used) {
            if (h->pin) (void)hipHostFree(h->pin);
            h->pin = nullptr;
            h->pin_bytes = 0;
            const size_t want = std::max<size_t>(used + used / 2, (size_t)256 << 10);
            if (hipHostMalloc(&h->pin, want, hipHostMallocDefault) != hipSuccess) {
                h->pin = nullptr;
                return fail(h, FCD_E_NOMEM, "hipHostMalloc failed (staging mirror)");
            }
            h->pin_bytes = want;
        }
        char *pin = reinterpret_cast<char *>(h->pin);
        if (st->n_in) memcpy(pin + st->o_in, in->post, st->n_in * esz);
        if (in->lengths) memcpy(pin + st->o_len, in->lengths, (size_t)B * 8);
        if (crf) memcpy(pin + st->o_init, c.init, st->n_init * 4);
        FCD_HIP(h, hipMemcpyAsync(base, pin, st->o_lab, hipMemcpyHostToDevice, h->stream));  // inputs lie before o_lab
    } else {
        if (st->n_in)
            FCD_HIP(h, hipMemcpyAsync(base + st->o_in, in->post, st->n_in * esz, hipMemcpyHostToDevice, h->stream));
        if (in->lengths)
            FCD_HIP(h, hipMemcpyAsync(base + st->o_len, in->lengths, (size_t)B * 8, hipMemcpyHostToDevice, h->stream));
        if (crf)
            FCD_HIP(h, hipMemcpyAsync(base + st->o_init, c.init, st->n_init * 4, hipMemcpyHostToDevice, h->stream));
    }
    *din = *in;
    din->post = reinterpret_cast<const float *>(base + st->o_in);
    din->lengths = in->lengths ? reinterpret_cast<const int64_t *>(base + st->o_len) : nullptr;
    dout->labels = reinterpret_cast<uint8_t *>(base + st->o_lab);
    dout->path = shape->path ? reinterpret_cast<uint32_t *>(base + st->o_path) : nullptr;
    dout->qual = shape->qual ? reinterpret_cast<float *>(base + st->o_qual) : nullptr;
    dout->out_len = reinterpret_cast<uint32_t *>(base + st->o_olen);
    dout->status = reinterpret_cast<int32_t *>(base + st->o_stat);
    dout->out_stride = shape->out_stride;
    dout->ambiguous = st->want_amb ? reinterpret_cast<uint32_t *>(base + st->o_amb) : nullptr;
    return FCD_OK;
}

// Runs the *_dev search of a staged call on h->stream.
int host_search(fcd_handle *h, const HostStage &st, const fcd_batch *din, const HostCall &c, const fcd_result *dout) {
    const float *dinit = reinterpret_cast<const float *>(reinterpret_cast<char *>(h->stage) + st.o_init);
    int rc = FCD_E_INVALID;
    if (c.n_best > 0 && (c.op == HostOp::Beam || c.op == HostOp::CrfBeam)) {
        char *base = reinterpret_cast<char *>(h->stage);
        const fcd_nbest dnb{c.n_best, reinterpret_cast<float *>(base + st.o_score), reinterpret_cast<uint32_t *>(base + st.o_nhyp)};
        rc = c.op == HostOp::Beam
                 ? fcd_beam_search_nbest_dev(h, din, c.beam_size, c.thr, c.collapse, c.kernel, &dnb, dout)
                 : fcd_crf_beam_search_nbest_dev(h, din, dinit, c.n_init, c.init_stride, c.beam_size, c.thr, c.kernel, &dnb, dout);
        if (rc == FCD_OK && h->overlap_n >= 2) rc = overlap_join(h, h->stream);
        return rc;
    }
    switch (c.op) {
        case HostOp::Viterbi: return fcd_viterbi_search_dev(h, din, c.collapse, dout);
        case HostOp::Beam: rc = fcd_beam_search_dev(h, din, c.beam_size, c.thr, c.collapse, c.kernel, dout); break;
        case HostOp::CrfBeam:
            rc = fcd_crf_beam_search_dev_k(h, din, dinit, c.n_init, c.init_stride, c.beam_size, c.thr, c.kernel, dout);
            break;
        case HostOp::CrfGreedy: return fcd_crf_greedy_search_dev(h, din, dinit, c.n_init, c.init_stride, dout);
    }
    // (fcd_set_overlap: the search may sit on an internal stream; the download that follows is in the handle's stream)
    if (rc == FCD_OK && h->overlap_n >= 2) rc = overlap_join(h, h->stream);
    return rc;
}

// Copies the fixed-stride device result of a staged call into the caller's arrays and waits.
int host_download(fcd_handle *h, const HostStage &st, const fcd_result &dout, const fcd_result *out, const fcd_nbest *nb) {
    const size_t B = (size_t)st.B;
    const size_t rows = st.n_rows;
    if (st.mirror) {
        char *pin = reinterpret_cast<char *>(h->pin);
        char *base = reinterpret_cast<char *>(h->stage);
        FCD_HIP(h, hipMemcpyAsync(pin + st.o_lab, base + st.o_lab, st.used - st.o_lab, hipMemcpyDeviceToHost, h->stream));
        FCD_HIP(h, hipStreamSynchronize(h->stream));
        memcpy(out->labels, pin + st.o_lab, st.n_out);
        if (out->path) memcpy(out->path, pin + st.o_path, st.n_out * 4);
        if (out->qual) memcpy(out->qual, pin + st.o_qual, st.n_out * 4);
        memcpy(out->out_len, pin + st.o_olen, rows * 4);
        if (out->status) memcpy(out->status, pin + st.o_stat, B * 4);
        if (st.want_amb) memcpy(out->ambiguous, pin + st.o_amb, B * 8);
        if (nb) {
            memcpy(nb->score, pin + st.o_score, rows * 4);
            memcpy(nb->n_hyp, pin + st.o_nhyp, B * 4);
        }
        return FCD_OK;
    }
    FCD_HIP(h, hipMemcpyAsync(out->labels, dout.labels, st.n_out, hipMemcpyDeviceToHost, h->stream));
    if (out->path) FCD_HIP(h, hipMemcpyAsync(out->path, dout.path, st.n_out * 4, hipMemcpyDeviceToHost, h->stream));
    if (out->qual) FCD_HIP(h, hipMemcpyAsync(out->qual, dout.qual, st.n_out * 4, hipMemcpyDeviceToHost, h->stream));
    FCD_HIP(h, hipMemcpyAsync(out->out_len, dout.out_len, rows * 4, hipMemcpyDeviceToHost, h->stream));
    if (out->status) FCD_HIP(h, hipMemcpyAsync(out->status, dout.status, B * 4, hipMemcpyDeviceToHost, h->stream));
    if (st.want_amb)
        FCD_HIP(h, hipMemcpyAsync(out->ambiguous, dout.ambiguous, B * 8, hipMemcpyDeviceToHost, h->stream));
    if (nb) {
        char *base = reinterpret_cast<char *>(h->stage);
        FCD_HIP(h, hipMemcpyAsync(nb->score, base + st.o_score, rows * 4, hipMemcpyDeviceToHost, h->stream));
        FCD_HIP(h, hipMemcpyAsync(nb->n_hyp, base + st.o_nhyp, B * 4, hipMemcpyDeviceToHost, h->stream));
    }
    FCD_HIP(h, hipStreamSynchronize(h->stream));
    return FCD_OK;
}

}  // namespace fcd

namespace {

int run_host(fcd_handle *h, const fcd_batch *in, const fcd_result *out, const HostCall &c) {
    if (!h) return FCD_E_INVALID;
    // held from staging to copy-back: two threads sharing a handle are serialised (fcd.h), they cannot
    // interleave on the staging buffer
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);
    int rc = host_check(h, in, out, c);
    if (rc) return rc;
    if (in->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);  // every HIP call of this entry point runs on the handle's device
    // Large batches: chunks on several internal lanes, upload || search || packed download (hostjob.hip)
    if (host_job_wanted(h, in, c)) return host_job_run_fixed(h, in, out, c);
    HostStage st;
    fcd_batch din{};
    fcd_result dout{};
    rc = host_upload(h, in, out, c, true, &st, &din, &dout);
    if (rc == FCD_OK) rc = host_search(h, st, &din, c, &dout);
    if (rc) return rc;
    return host_download(h, st, dout, out);
}

// the n-best forms: stage, decode, copy back -- never the chunk pipeline of hostjob.hip
int run_host_nbest(fcd_handle *h, const fcd_batch *in, const fcd_result *out, const fcd_nbest *nb, const HostCall &c) {
    if (!h) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> whole_call(h->mu);
    if (c.beam_size < 1) return fail(h, FCD_E_INVALID, "beam_size cannot be 0");
    int rc = host_check(h, in, out, c);
    if (rc) return rc;
    rc = check_result_nbest(h, in, out, nb, c.beam_size);
    if (rc) return rc;
    if (in->n_reads == 0) return FCD_OK;
    FCD_DEVICE(h);
    HostCall cn = c;
    cn.n_best = nb->n_best;
    HostStage st;
    fcd_batch din{};
    fcd_result dout{};
    rc = host_upload(h, in, out, cn, true, &st, &din, &dout);
    if (rc == FCD_OK) rc = host_search(h, st, &din, cn, &dout);
    if (rc) return rc;
    return host_download(h, st, dout, out, nb);
}

}  // namespace

extern "C" {

int fcd_viterbi_search_host(fcd_handle *h, const fcd_batch *in, int collapse_repeats,
                            const fcd_result *out) {
    HostCall c{HostOp::Viterbi};
    c.collapse = collapse_repeats;
    return run_host(h, in, out, c);
}

int fcd_beam_search_host(fcd_handle *h, const fcd_batch *in, int64_t beam_size,
                         float beam_cut_threshold, int collapse_repeats, int kernel,
                         const fcd_result *out) {
    HostCall c{HostOp::Beam};
    c.collapse = collapse_repeats;
    c.beam_size = beam_size;
    c.thr = beam_cut_threshold;
    c.kernel = kernel;
    return run_host(h, in, out, c);
}

int fcd_crf_beam_search_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                             int64_t init_stride, int64_t beam_size, float beam_cut_threshold,
                             const fcd_result *out) {
    return fcd_crf_beam_search_host_k(h, in, init, n_init, init_stride, beam_size, beam_cut_threshold,
                                      FCD_KERNEL_AUTO, out);
}

int fcd_crf_beam_search_host_k(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                               int64_t init_stride, int64_t beam_size, float beam_cut_threshold,
                               int kernel, const fcd_result *out) {
    HostCall c{HostOp::CrfBeam};
    c.beam_size = beam_size;
    c.thr = beam_cut_threshold;
    c.kernel = kernel;
    c.init = init;
    c.n_init = n_init;
    c.init_stride = init_stride;
    return run_host(h, in, out, c);
}

int fcd_beam_search_nbest_host(fcd_handle *h, const fcd_batch *in, int64_t beam_size, float beam_cut_threshold,
                               int collapse_repeats, int kernel, const fcd_nbest *nb, const fcd_result *out) {
    HostCall c{HostOp::Beam};
    c.collapse = collapse_repeats;
    c.beam_size = beam_size;
    c.thr = beam_cut_threshold;
    c.kernel = kernel;
    return run_host_nbest(h, in, out, nb, c);
}

int fcd_crf_beam_search_nbest_host(fcd_handle *h, const fcd_batch *in, const float *init, int64_t n_init,
                                   int64_t init_stride, int64_t beam_size, float beam_cut_threshold, int kernel,
                                   const fcd_nbest *nb, const fcd_result *out) {
    HostCall c{HostOp::CrfBeam};
    c.beam_size = beam_size;
    c.thr = beam_cut_threshold;
    c.kernel = kernel;
    c.init = init;
    c.n_init = n_init;
    c.init_stride = init_stride;
    return run_host_nbest(h, in, out, nb, c);
}

int fcd_crf_greedy_search_host(fcd_handle *h, const fcd_batch *in, const float *init,
                               int64_t n_init, int64_t init_stride, const fcd_result *out) {
    HostCall c{HostOp::CrfGreedy};
    c.init = init;
    c.n_init = n_init;
    c.init_stride = init_stride;
    return run_host(h, in, out, c);
}

// phred (src/search.rs:31-36), host side; log10f is libm's, as in the reference
uint32_t fcd_phred(float prob, float qscale, float qbias) {
    const float mx = 1e-4f;
    const float om = 1.0f - prob;
    const float p = (om < mx) ? mx : om;
    const float q = -10.0f * log10f(p) * qscale + qbias;
    const float rq = roundf(q);  // f32::round: half away from zero
    uint32_t u;                  // Rust `as u32`: saturating, NaN -> 0
    if (!(rq == rq) || rq <= 0.0f) u = 0;
    else if (rq >= 4294967296.0f) u = 4294967295u;
    else u = (uint32_t)rq;
    return u + 33u;
}

}  // extern "C"

// ---- beam-search sessions (include/fcd.h, fcd_beam_session_*) ------------------------------
struct fcd_beam_session {
    fcd_handle *h = nullptr;
    int64_t n = 0, N = 0, S = 1, max_steps = 0, beam = 0, n_init = 0;
    float thr = 0.0f;
    int collapse = 1, crf = 0, wave = 0, force1 = 0, tie_order = FCD_TIE_PDQ178;
    void *mem = nullptr;  // the one device allocation: state blocks | staged lengths | slot list | init rows | tree slabs
    size_t bytes = 0;
    SessionDesc ses{};
    int64_t *d_len = nullptr, *d_slots = nullptr;
    float *d_init = nullptr;
    WaveArena war{};
    GenericArena gar{};
    std::vector<int64_t> steps;  // rows taken by each slot since creation or its restart (host side: the max_steps check)
    char *pin = nullptr;         // page-locked staging of lengths / slot lists / init rows, reused only once its copy is done
    hipEvent_t pin_ev = nullptr;
    bool pin_busy = false;
};

namespace {

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// host bytes -> device, in stream order, through the session's page-locked buffer
int ses_stage(fcd_beam_session *s, hipStream_t stream, const void *src0, size_t n0, void *dst0, const void *src1 = nullptr,
              size_t n1 = 0, void *dst1 = nullptr) {
    fcd_handle *h = s->h;
    if (s->pin_busy) {
        FCD_HIP(h, hipEventSynchronize(s->pin_ev));
        s->pin_busy = false;
    }
    memcpy(s->pin, src0, n0);
    FCD_HIP(h, hipMemcpyAsync(dst0, s->pin, n0, hipMemcpyHostToDevice, stream));
    if (n1) {
        memcpy(s->pin + align256(n0), src1, n1);
        FCD_HIP(h, hipMemcpyAsync(dst1, s->pin + align256(n0), n1, hipMemcpyHostToDevice, stream));
    }
    FCD_HIP(h, hipEventRecord(s->pin_ev, stream));
    s->pin_busy = true;
    return FCD_OK;
}

int ses_check_out(fcd_beam_session *s, const fcd_result *out) {
    fcd_handle *h = s->h;
    if (!out->labels || !out->out_len || !out->status) return fail(h, FCD_E_INVALID, "null labels/out_len/status");
    if (out->out_stride < s->max_steps) return fail(h, FCD_E_INVALID, "out_stride must be >= max_steps");
    if (out->ambiguous && !s->ses.count_amb)
        return fail(h, FCD_E_INVALID, "the session was created without count_ambiguous: it has no tie counters to report");
    return FCD_OK;
}

// one launch of the session's kernel on `chunk` (device posteriors; nullptr: no rows, a result only)
int ses_launch(fcd_beam_session *s, const fcd_batch *chunk, const fcd_result *out) {
    fcd_handle *h = s->h;
    const int64_t Tc = chunk ? chunk->T : 0;
    std::vector<int64_t> take((size_t)s->n, 0);
    if (chunk) {
        for (int64_t r = 0; r < s->n; ++r) {
            int64_t t = chunk->lengths ? chunk->lengths[r] : Tc;
            t = t < 0 ? 0 : (t < Tc ? t : Tc);  // (as the kernels clamp lengths)
            if (s->steps[(size_t)r] + t > s->max_steps)
                return fail(h, FCD_E_INVALID, "the push would take a slot past max_steps (nothing was enqueued)");
            take[(size_t)r] = t;
        }
    }
    FCD_DEVICE(h);
    BatchDesc d{};
    if (chunk) {
        d = to_desc(chunk, s->crf != 0);
    } else {
        d.N = (int)s->N;
        d.S = (int)s->S;
        d.dtype = FCD_DTYPE_F32;
    }
    d.n_reads = s->n;
    const ResultDesc o = out ? to_desc(out) : ResultDesc{};
    CallScope sc(h);
    if (out) sc.add(o, s->n);
    if (chunk && Tc > 0) sc.add(chunk->post, (size_t)span_elems(chunk, s->crf != 0) * (chunk->dtype == FCD_DTYPE_F32 ? 4 : 2));
    sc.add(s->mem, s->bytes);
    int rc = sc.begin(false, false);  // the handle's stream: a session's pushes stay in order
    if (rc) return rc;
    sc.time();
    if (chunk && chunk->lengths) {
        rc = ses_stage(s, sc.stream, chunk->lengths, (size_t)s->n * 8, s->d_len);
        if (rc) return rc;
        d.lengths = s->d_len;
    }
    BeamArgs a{};
    a.beam_size = (int)s->beam;
    a.thr = s->thr;
    a.collapse = s->collapse;
    a.crf = s->crf;
    a.n_init = s->n_init;
    a.force_one_read_per_wave = s->force1;
    a.tie_order = s->tie_order;
    if (s->wave) FCD_HIP(h, launch_beam_wave_session(d, s->n, a, s->war, o, s->ses, sc.stream));
    else FCD_HIP(h, launch_beam_generic(d, 0, s->n, a, s->gar, o, sc.stream, NBestDesc{}, s->ses));
    rc = sc.finish();
    if (rc) return rc;
    for (int64_t r = 0; r < s->n; ++r) s->steps[(size_t)r] += take[(size_t)r];
    return FCD_OK;
}

int ses_restart(fcd_beam_session *s, const int64_t *slots, int64_t n, const float *init) {
    fcd_handle *h = s->h;
    if (n < 0 || n > s->n || (n > 0 && !slots)) return fail(h, FCD_E_INVALID, "bad slot list");
    if (s->crf && n > 0 && !init) return fail(h, FCD_E_INVALID, "a CRF restart needs an init row per slot");
    std::vector<char> seen((size_t)s->n, 0);  // (one restart block per entry: a slot listed twice would be written twice at once)
    for (int64_t j = 0; j < n; ++j) {
        if (slots[j] < 0 || slots[j] >= s->n) return fail(h, FCD_E_INVALID, "slot out of range");
        if (seen[(size_t)slots[j]]++) return fail(h, FCD_E_INVALID, "a slot is listed twice");
    }
    if (n == 0) return FCD_OK;
    FCD_DEVICE(h);
    CallScope sc(h);
    sc.add(s->mem, s->bytes);
    int rc = sc.begin(false, false);
    if (rc) return rc;
    const size_t n_init_bytes = s->crf ? (size_t)n * (size_t)s->n_init * 4 : 0;
    rc = ses_stage(s, sc.stream, slots, (size_t)n * 8, s->d_slots, init, n_init_bytes, s->d_init);
    if (rc) return rc;
    FCD_HIP(h, launch_session_restart(s->ses, s->d_slots, n, s->wave != 0, (int)s->beam, (int)s->N, s->crf, (int)s->S,
                                      s->d_init, s->n_init, sc.stream));
    rc = sc.finish();
    if (rc) return rc;
    for (int64_t j = 0; j < n; ++j) s->steps[(size_t)slots[j]] = 0;
    return FCD_OK;
}

void ses_free(fcd_beam_session *s) {
    if (s->mem) (void)hipFree(s->mem);
    if (s->pin) (void)hipHostFree(s->pin);
    if (s->pin_ev) (void)hipEventDestroy(s->pin_ev);
    delete s;
}

int ses_create(fcd_handle *h, int64_t n_reads, int64_t S, int64_t N, int crf, const float *init, int64_t n_init,
               int64_t max_steps, int64_t beam_size, float thr, int collapse, int kernel, int count_ambiguous,
               fcd_beam_session **out) {
    if (!h || !out) return FCD_E_INVALID;
    *out = nullptr;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    if (n_reads < 1 || max_steps < 1) return fail(h, FCD_E_INVALID, "n_reads and max_steps must be >= 1");
    if (beam_size < 1) return fail(h, FCD_E_INVALID, "beam_size cannot be 0");
    if (N < 2) return fail(h, FCD_E_UNSUPPORTED, "alphabet needs at least one label besides the blank");
    if (N > 256) return fail(h, FCD_E_UNSUPPORTED, "alphabets above 256 labels are unsupported (u8 labels)");
    if (max_steps >= (1ll << 28)) return fail(h, FCD_E_UNSUPPORTED, "max_steps must be < 2^28");
    if (crf && (S < 1 || !init || n_init < 1)) return fail(h, FCD_E_INVALID, "a CRF session needs S >= 1 and an init row per slot");
    if (kernel == FCD_KERNEL_LANE) return fail(h, FCD_E_UNSUPPORTED, "sessions do not run on the lane kernel (wide beams take the generic kernel)");
    if (kernel < FCD_KERNEL_AUTO || kernel > FCD_KERNEL_LANE) return fail(h, FCD_E_INVALID, "unknown kernel");
    const int beam = (int)std::min<int64_t>(beam_size, 1 << 20);
    const int NL = (int)N - 1;
    const int tie = effective_tie_order(h);
    // kernel choice (as beam_dev): the wave kernel where it holds the shape and node ids of max_steps rows fit 25 bits
    bool wave = false;
    int shift = 0;
    if (kernel != FCD_KERNEL_GENERIC) {
        const bool ok = beam_wave_supported(beam, (int)N, crf, (int)S);
        shift = beam_wave_id_shift(beam, (int)N, kernel == FCD_KERNEL_WAVE1);
        wave = ok && (max_steps << shift) + 16 < (1ll << 25);
        if (!wave && kernel != FCD_KERNEL_AUTO)
            return fail(h, FCD_E_UNSUPPORTED, ok ? "wave kernel: max_steps too large" : "wave kernel: needs beam_size <= 8 and N <= 7, or beam_size <= 12 and N <= 5 (CRF: N = 5, S a power of two >= 4)");
    }
    int64_t cap, block_words;
    size_t slab_bytes;
    if (wave) {
        cap = ((max_steps << shift) + 8 + 3) & ~3ll;
        slab_bytes = (size_t)cap * (4 + 4 + (NL <= 4 ? 4 : 8) * 4);
        block_words = kSesWaveWords;
    } else {
        if (beam > (1 << 16)) return fail(h, FCD_E_UNSUPPORTED, "beam_size above 65536");
        if (beam_generic_lds_bytes(beam, (int)N, tie) > 64 * 1024)
            return fail(h, FCD_E_UNSUPPORTED, "beam_size * alphabet too large for the LDS-resident kernel");
        cap = max_steps * beam * NL + 8;
        if (cap >= (1ll << 30)) return fail(h, FCD_E_UNSUPPORTED, "tree arena above 2^30 nodes per slot");
        slab_bytes = (size_t)cap * (sizeof(int4) + (size_t)NL * 4);
        block_words = ses_generic_words(beam, N);
    }
    const size_t o_len = align256((size_t)n_reads * block_words * 4);
    const size_t o_slots = o_len + align256((size_t)n_reads * 8);
    const size_t o_init = o_slots + align256((size_t)n_reads * 8);
    const size_t o_slab = o_init + align256(crf ? (size_t)n_reads * n_init * 4 : 0);
    const size_t bytes = o_slab + (size_t)n_reads * slab_bytes;
    DeviceGuard dev_guard(h->device);
    FCD_HIP(h, dev_guard.err);
    fcd_beam_session *s = new fcd_beam_session();
    s->h = h;
    s->n = n_reads;
    s->N = N;
    s->S = crf ? S : 1;
    s->max_steps = max_steps;
    s->beam = beam;
    s->n_init = crf ? n_init : 0;
    s->thr = thr;
    s->collapse = crf ? 0 : (collapse ? 1 : 0);
    s->crf = crf;
    s->wave = wave ? 1 : 0;
    s->force1 = kernel == FCD_KERNEL_WAVE1 ? 1 : 0;
    s->tie_order = tie;
    s->steps.assign((size_t)n_reads, 0);
    if (hipMalloc(&s->mem, bytes) != hipSuccess) {
        s->mem = nullptr;
        ses_free(s);
        return fail(h, FCD_E_NOMEM, "hipMalloc of the session's state and tree slabs failed");
    }
    s->bytes = bytes;
    const size_t pin_bytes = align256((size_t)n_reads * 8) + (size_t)n_reads * std::max<int64_t>(s->n_init, 1) * 4;
    if (hipHostMalloc(reinterpret_cast<void **>(&s->pin), pin_bytes, hipHostMallocDefault) != hipSuccess) {
        s->pin = nullptr;
        ses_free(s);
        return fail(h, FCD_E_NOMEM, "hipHostMalloc of the session's staging buffer failed");
    }
    if (hipEventCreateWithFlags(&s->pin_ev, hipEventDisableTiming) != hipSuccess) {
        s->pin_ev = nullptr;
        ses_free(s);
        return fail(h, FCD_E_HIP, "hipEventCreate failed");
    }
    char *base = static_cast<char *>(s->mem);
    s->ses.state = reinterpret_cast<int32_t *>(base);
    s->ses.block_words = block_words;
    s->ses.count_amb = count_ambiguous ? 1 : 0;
    s->d_len = reinterpret_cast<int64_t *>(base + o_len);
    s->d_slots = reinterpret_cast<int64_t *>(base + o_slots);
    s->d_init = reinterpret_cast<float *>(base + o_init);
    if (wave) {
        s->war.cap_nodes = cap;
        s->war.row_words = NL <= 4 ? 4 : 8;
        s->war.rec = reinterpret_cast<int32_t *>(base + o_slab);
        s->war.jmp = s->war.rec + (size_t)n_reads * cap;
        s->war.rows = s->war.jmp + (size_t)n_reads * cap;
    } else {
        s->gar.cap_nodes = cap;
        s->gar.rec = reinterpret_cast<int4 *>(base + o_slab);
        s->gar.rows = reinterpret_cast<int32_t *>(base + o_slab + (size_t)n_reads * cap * sizeof(int4));
    }
    // every slot starts at the root
    std::vector<int64_t> all((size_t)n_reads);
    for (int64_t r = 0; r < n_reads; ++r) all[(size_t)r] = r;
    int rc = ses_restart(s, all.data(), n_reads, init);
    if (rc == FCD_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(h, FCD_E_HIP, "session initialisation failed");
    if (rc) {
        ses_free(s);
        return rc;
    }
    h->live_sessions++;
    *out = s;
    return FCD_OK;
}

// the *_host forms: posteriors and results through the handle's staging buffer, synchronous
int ses_host(fcd_beam_session *s, const fcd_batch *chunk, const fcd_result *out) {
    fcd_handle *h = s->h;
    const size_t n = (size_t)s->n, w = (size_t)s->max_steps;
    const size_t in_bytes = chunk ? (size_t)span_elems(chunk, s->crf != 0) * (chunk->dtype == FCD_DTYPE_F32 ? 4 : 2) : 0;
    const size_t o_lab = align256(in_bytes), o_path = o_lab + align256(n * w), o_olen = o_path + align256(n * w * 4);
    const size_t o_stat = o_olen + align256(n * 4), o_amb = o_stat + align256(n * 4), used = o_amb + n * 8;
    FCD_DEVICE(h);
    int rc = ensure(h, &h->stage, &h->stage_bytes, used);
    if (rc) return rc;
    char *base = static_cast<char *>(h->stage);
    fcd_batch din{};
    if (chunk) {
        din = *chunk;
        din.post = base;
        if (in_bytes) FCD_HIP(h, hipMemcpyAsync(base, chunk->post, in_bytes, hipMemcpyHostToDevice, h->stream));
    }
    fcd_result dout{};
    if (out) {
        dout.labels = reinterpret_cast<uint8_t *>(base + o_lab);
        dout.path = out->path ? reinterpret_cast<uint32_t *>(base + o_path) : nullptr;
        dout.out_len = reinterpret_cast<uint32_t *>(base + o_olen);
        dout.status = reinterpret_cast<int32_t *>(base + o_stat);
        dout.ambiguous = out->ambiguous ? reinterpret_cast<uint32_t *>(base + o_amb) : nullptr;
        dout.out_stride = (int64_t)w;
    }
    rc = ses_launch(s, chunk ? &din : nullptr, out ? &dout : nullptr);
    if (rc) return rc;
    if (out) {
        const hipStream_t st = h->stream;
        auto rows = [&](void *dst, const char *src, size_t elem) -> hipError_t {
            if ((size_t)out->out_stride == w) return hipMemcpyAsync(dst, src, n * w * elem, hipMemcpyDeviceToHost, st);
            for (size_t r = 0; r < n; ++r) {
                hipError_t e = hipMemcpyAsync(static_cast<char *>(dst) + r * out->out_stride * elem, src + r * w * elem, w * elem,
                                              hipMemcpyDeviceToHost, st);
                if (e != hipSuccess) return e;
            }
            return hipSuccess;
        };
        FCD_HIP(h, rows(out->labels, base + o_lab, 1));
        if (out->path) FCD_HIP(h, rows(out->path, base + o_path, 4));
        FCD_HIP(h, hipMemcpyAsync(out->out_len, base + o_olen, n * 4, hipMemcpyDeviceToHost, st));
        FCD_HIP(h, hipMemcpyAsync(out->status, base + o_stat, n * 4, hipMemcpyDeviceToHost, st));
        if (out->ambiguous) FCD_HIP(h, hipMemcpyAsync(out->ambiguous, base + o_amb, n * 8, hipMemcpyDeviceToHost, st));
    }
    FCD_HIP(h, hipStreamSynchronize(h->stream));
    return FCD_OK;
}

int ses_check_chunk(fcd_beam_session *s, const fcd_batch *chunk) {
    fcd_handle *h = s->h;
    int rc = check_batch(h, chunk, s->crf != 0);
    if (rc) return rc;
    if (chunk->n_reads != s->n) return fail(h, FCD_E_INVALID, "chunk->n_reads must be the session's n_reads");
    if (chunk->N != s->N || (s->crf && chunk->S != s->S)) return fail(h, FCD_E_INVALID, "chunk shape differs from the session's");
    return FCD_OK;
}

}  // namespace

extern "C" {

int fcd_beam_session_create(fcd_handle *h, int64_t n_reads, int64_t N, int64_t max_steps, int64_t beam_size,
                            float beam_cut_threshold, int collapse_repeats, int kernel, int count_ambiguous,
                            fcd_beam_session **out) {
    return ses_create(h, n_reads, 1, N, 0, nullptr, 0, max_steps, beam_size, beam_cut_threshold, collapse_repeats, kernel,
                      count_ambiguous, out);
}

int fcd_crf_beam_session_create(fcd_handle *h, int64_t n_reads, int64_t S, int64_t N, const float *init, int64_t n_init,
                                int64_t max_steps, int64_t beam_size, float beam_cut_threshold, int kernel,
                                int count_ambiguous, fcd_beam_session **out) {
    return ses_create(h, n_reads, S, N, 1, init, n_init, max_steps, beam_size, beam_cut_threshold, 0, kernel,
                      count_ambiguous, out);
}

int fcd_beam_session_push_dev(fcd_beam_session *s, const fcd_batch *chunk, const fcd_result *out) {
    if (!s) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(s->h->mu);
    int rc = ses_check_chunk(s, chunk);
    if (rc) return rc;
    if (out && (rc = ses_check_out(s, out))) return rc;
    return ses_launch(s, chunk, out);
}

int fcd_beam_session_push_host(fcd_beam_session *s, const fcd_batch *chunk, const fcd_result *out) {
    if (!s) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(s->h->mu);
    int rc = ses_check_chunk(s, chunk);
    if (rc) return rc;
    if (out && (rc = ses_check_out(s, out))) return rc;
    return ses_host(s, chunk, out);
}

int fcd_beam_session_result_dev(fcd_beam_session *s, const fcd_result *out) {
    if (!s) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(s->h->mu);
    if (!out) return fail(s->h, FCD_E_INVALID, "null result");
    int rc = ses_check_out(s, out);
    if (rc) return rc;
    return ses_launch(s, nullptr, out);
}

int fcd_beam_session_result_host(fcd_beam_session *s, const fcd_result *out) {
    if (!s) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(s->h->mu);
    if (!out) return fail(s->h, FCD_E_INVALID, "null result");
    int rc = ses_check_out(s, out);
    if (rc) return rc;
    return ses_host(s, nullptr, out);
}

int fcd_beam_session_restart(fcd_beam_session *s, const int64_t *slots, int64_t n, const float *init) {
    if (!s) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(s->h->mu);
    return ses_restart(s, slots, n, init);
}

int fcd_beam_session_steps(const fcd_beam_session *s, int64_t *steps) {
    if (!s || !steps) return FCD_E_INVALID;
    std::lock_guard<std::recursive_mutex> g(s->h->mu);
    memcpy(steps, s->steps.data(), (size_t)s->n * 8);
    return FCD_OK;
}

int64_t fcd_beam_session_bytes(const fcd_beam_session *s) { return s ? (int64_t)s->bytes : 0; }

int fcd_beam_session_destroy(fcd_beam_session *s) {
    if (!s) return FCD_OK;
    fcd_handle *h = s->h;
    std::lock_guard<std::recursive_mutex> g(h->mu);
    DeviceGuard dev_guard(h->device);
    (void)hipStreamSynchronize(h->stream);  // (its last launches may still read the state)
    ses_free(s);
    h->live_sessions--;
    return FCD_OK;
}

}  // extern "C"
