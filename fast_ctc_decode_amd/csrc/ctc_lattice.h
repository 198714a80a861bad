// ctc_lattice.h -- what the walks of the CTC lattice of a GIVEN labelling share: ctc_score.hip (forward: the sum over
// the alignments), ctc_align.hip (Viterbi: the best alignment) and ctc_posterior.hip (forward and backward).  Parameter
// block, LDS layout, everything before the time loop, the staging of the posteriors (split into mantissa and exponent),
// the live window of a row, the integer row maximum and the wave rotations.  The pieces the CRF lattice (crf_lattice.h,
// which includes this file) has in common with it live here too:
// k(t) of a decoded path (labels_up_to, stage_krow_before), the ln P result (ln_p), the stored forward rows (kAlphaDown,
// stored_rows_bytes) and what the backward walks end in (store_post, log_ratio).
#pragma once

#include <math.h>

#include "device_utils.h"
#include "fcd_internal.h"

namespace fcd {
namespace {

// (kTarget and kNoExp: device_utils.h)
constexpr int kTileElems = 1024;      // posteriors staged per tile
constexpr int kTileRows = 64;         // ... at most this many rows (one lane per row finds k(t))
constexpr int kLdsCells = 20;         // LDS kernel: cells per work-item and step
constexpr int kMiscWords = 32;        // [0..15] per-wave maxima, [16] bad-label flag, [17] kBadPost, [18] [19] the two final cells,
                                      // [20] kKrowBefore
constexpr int kBadPost = 17;          // misc word of ctc_align.hip: the read holds a posterior no comparison can order
constexpr int kKrowBefore = 20;       // misc word of ctc_posterior.hip: k(t) of the row before the tile

struct ScoreParams {
    BatchDesc in;
    ScoreDesc y;
    int collapse;
    int band;
    double *logp;
    int cap;      // LDS kernel: states per alpha buffer
    int lab_cap;  // labels the LDS copy of a labelling holds
    int slack = 0;  // states by which window_k's two reachability cuts are relaxed (ctc_posterior.hip's edit walk: 2)
};

struct Lds {
    float *pm;
    int *pe;
    int *krow;
    int *misc;
    uint16_t *lab;
    float *alpha;
};

__device__ __forceinline__ Lds carve(unsigned char *smem, int lab_cap) {
    Lds l;
    l.pm = reinterpret_cast<float *>(smem);
    l.pe = reinterpret_cast<int *>(smem + kTileElems * 4);
    l.krow = reinterpret_cast<int *>(smem + kTileElems * 8);
    l.misc = l.krow + kTileRows;
    l.lab = reinterpret_cast<uint16_t *>(l.misc + kMiscWords);
    l.alpha = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(l.lab) + (((size_t)lab_cap * 2 + 15) & ~(size_t)15));
    return l;
}

inline size_t lds_bytes(int lab_cap, int cap) {
    return (size_t)kTileElems * 8 + (kTileRows + kMiscWords) * 4 + (((size_t)lab_cap * 2 + 15) & ~(size_t)15) + (size_t)cap * 8;
}

// what one row of the lattice needs to know about itself
struct Row {
    const float *post;  // the read's first element
    const uint8_t *labels;
    const uint32_t *path;
    int Tr, L, N, rows_per_tile;
};

// Everything before the time loop.  Returns false when the row's result is already written (every work-item agrees).
__device__ __forceinline__ bool prologue(const ScoreParams &p, const Lds &lds, Row *rw) {
    const int tid = threadIdx.x, bd = blockDim.x;
    const int64_t row = blockIdx.x;
    const int64_t read = row / p.y.n_hyp;
    const int64_t hyp = row - read * p.y.n_hyp;
    const double nan = (double)NAN;
    if (p.y.n_valid && hyp >= (int64_t)p.y.n_valid[read]) {  // not a hypothesis of this read
        if (tid == 0) p.logp[row] = nan;
        return false;
    }
    int64_t Tr = p.in.lengths ? p.in.lengths[read] : p.in.T;
    Tr = Tr < 0 ? 0 : (Tr > p.in.T ? p.in.T : Tr);
    const uint32_t len = p.y.len[row];
    if ((int64_t)len > p.y.stride) {  // longer than its row: not a labelling
        if (tid == 0) p.logp[row] = nan;
        return false;
    }
    const int L = (int)len;
    const uint8_t *labels = p.y.labels + row * p.y.stride;
    if (tid == 0) lds.misc[16] = 0;
    __syncthreads();
    bool bad = false;
    for (int k = tid; k < L; k += bd) {
        const int y = labels[k], yp = k ? labels[k - 1] : 0;
        bad |= y < 1 || y >= p.in.N;
        if (k < p.lab_cap) lds.lab[k] = (uint16_t)(y | ((k > 0 && y != yp) ? 0x100 : 0));
    }
    if (bad) lds.misc[16] = 1;
    __syncthreads();
    double early = 0.0;
    bool done = true;
    if (lds.misc[16]) early = nan;                             // a label outside 1 .. N-1
    else if (Tr == 0) early = L == 0 ? 0.0 : -(double)INFINITY;
    else if ((int64_t)L > Tr) early = -(double)INFINITY;      // more labels than rows: no alignment
    else done = false;
    if (done) {
        if (tid == 0) p.logp[row] = early;
        return false;
    }
    rw->post = post_at(p.in.post, read * p.in.stride_read, p.in.dtype);
    rw->labels = labels;
    rw->path = p.y.path ? p.y.path + row * p.y.stride : nullptr;
    rw->Tr = (int)Tr;
    rw->L = L;
    rw->N = p.in.N;
    rw->rows_per_tile = min(kTileRows, kTileElems / p.in.N);
    return true;
}

// k(t) = #{k : path[k] <= t}: the labels the decoded path has emitted up to row t
__device__ __forceinline__ int labels_up_to(const uint32_t *path, int L, uint32_t t) {
    int lo = 0, hi = L;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (path[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// A backward walk's row t0 reads the window of the row BEFORE its tile, which has no krow entry: k(t0 - 1) goes to
// misc[kKrowBefore] once per tile (after fill_tile) ...
__device__ __forceinline__ void stage_krow_before(int *misc, const uint32_t *path, int L, int band, int t0) {
    if (band > 0 && t0 > 0) {
        if (threadIdx.x == 0) misc[kKrowBefore] = labels_up_to(path, L, (uint32_t)(t0 - 1));
        __syncthreads();
    }
}

// ... and k(t - 1) of the tile's row i is read from there or from the row's predecessor in the tile (0 unbanded)
__device__ __forceinline__ int krow_before(const int *krow, const int *misc, int band, int i) {
    return band > 0 ? (i > 0 ? krow[i - 1] : misc[kKrowBefore]) : 0;
}

// rows t0 .. t0 + rc of the read into the tile, split into mantissa and exponent; banded: k(t) of each of them
__device__ __forceinline__ void fill_tile(const ScoreParams &p, const Lds &lds, const Row &rw, int t0, int rc) {
    const int tid = threadIdx.x, bd = blockDim.x;
    __syncthreads();  // the previous tile's readers are done
    for (int e = tid; e < rc * rw.N; e += bd) {
        const int i = e / rw.N, j = e - i * rw.N;
        const float v = load_post(rw.post, (int64_t)(t0 + i) * p.in.stride_t + (int64_t)j * p.in.stride_n, p.in.dtype);
        int ex = 0;
        float m = v;
        if (v - v == 0.0f) m = frexpf(v, &ex);  // (finite; an infinity or a NaN stays what it is, exponent 0)
        lds.pm[e] = m;
        lds.pe[e] = ex;
    }
    if (p.band > 0 && tid < rc) lds.krow[tid] = labels_up_to(rw.path, rw.L, (uint32_t)(t0 + tid));
    __syncthreads();
}

// live states of row t: the band around the path (k = k(t), read only when banded), cut to what can be reached and can
// still reach the end -- in the labelling itself; p.slack more states on either side for a walk that also follows
// labellings one label shorter (their alignments reach a state a row earlier and may leave it a row later)
__device__ __forceinline__ void window_k(const ScoreParams &p, const Row &rw, int t, int k, int *lo, int *hi) {
    int l = 0, h = 2 * rw.L;
    if (p.band > 0) {
        l = max(0, 2 * (k - p.band) - 2);
        h = min(h, 2 * (k + p.band));
    }
    *hi = min(h, 2 * t + 1 + p.slack);
    *lo = max(l, 2 * rw.L - 2 * (rw.Tr - 1 - t) - 2 - p.slack);
}

// ... of row t, the tile's row i
__device__ __forceinline__ void window(const ScoreParams &p, const Lds &lds, const Row &rw, int t, int i, int *lo, int *hi) {
    window_k(p, rw, t, p.band > 0 ? lds.krow[i] : 0, lo, hi);
}

// (finite_exp and wave_imax: device_utils.h, shared with the CRF Viterbi search of crf_viterbi.hip)

__device__ __forceinline__ float from_prev_lane(float x) {  // wave_ror:1 -- lane l receives lane (l - 1) & 63
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x13C, 0xf, 0xf, false));
}

__device__ __forceinline__ float from_next_lane(float x) {  // wave_rol:1 -- lane l receives lane (l + 1) & 63
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x134, 0xf, 0xf, false));
}

template <int K>
__device__ __forceinline__ int slot_state(int lane, int r, int lo) {  // the state >= lo that lives in slot lane * K + r
    constexpr int C = 64 * K;
    const int s = lo / C * C + lane * K + r;
    return s < lo ? s + C : s;
}

// ---- the register-resident window (K consecutive states per lane, state s in slot s mod 64K) ----
// What a lane needs for one row: read from LDS a row ahead of its use (nothing here depends on alpha).
template <int K>
struct StepIn {
    float pm0, pm[K / 2];
    int pe0, pe[K / 2];
    uint32_t in_mask;    // bit r: the lane's state r lies in the row's window
    uint32_t skip_mask;  // bit r (odd r): the s-2 term enters
    int lo, hi;
};

template <int K>
__device__ __forceinline__ StepIn<K> load_step(const ScoreParams &p, const Lds &lds, const Row &rw, int t, int i) {
    StepIn<K> in;
    const int lane = threadIdx.x;
    window(p, lds, rw, t, i, &in.lo, &in.hi);
    in.pm0 = lds.pm[i * rw.N];
    in.pe0 = lds.pe[i * rw.N];
    in.in_mask = 0;
    in.skip_mask = 0;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = slot_state<K>(lane, r, in.lo);
        const bool live = s <= in.hi;
        in.in_mask |= (live ? 1u : 0u) << r;
        if (r & 1) {
            const int info = lds.lab[live ? (s >> 1) : 0];  // (a dead slot reads a valid address and is masked below)
            const int y = live ? (info & 0xFF) : 0;
            in.pm[r / 2] = lds.pm[i * rw.N + y];
            in.pe[r / 2] = lds.pe[i * rw.N + y];
            const bool skip = live && s >= 3 && (!p.collapse || (info & 0x100));
            in.skip_mask |= (skip ? 1u : 0u) << r;
        }
    }
    return in;
}

// ---- what a forward walk leaves: ln P, and (stored) its rows for a backward walk ----
constexpr double kLn2 = 0.693147180559945309417232121458;

// ln(m * 2^eacc), in float64
__device__ __forceinline__ double ln_p(double m, int64_t eacc) { return log(m) + (double)eacc * kLn2; }

constexpr int kAlphaDown = 60;  // stored alpha: row maximum in [2^59, 2^60) -- times a backward value (below 2^60) stays finite

// stored forward rows of one labelling at k states per lane (every labelling of a call has T rows' worth): T * 64k cells
// by SLOT, scaled by 2^-kAlphaDown (exact), then T exponent words
inline size_t stored_rows_bytes(int64_t T, size_t k) {
    return ((size_t)(T > 1 ? T : 1) * (64 * k + 1) * 4 + 255) & ~(size_t)255;
}

// ---- what a backward walk ends in ----
// post[k][.] = acc / sum over the labels
template <int NC>
__device__ __forceinline__ void store_post(float *post, int k, int nc, const float (&acc)[NC]) {
    float sum = acc[0];
#pragma unroll
    for (int c = 1; c < NC; ++c)
        if (c < nc) sum += acc[c];
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (c < nc) post[(int64_t)k * nc + c] = acc[c] / sum;  // (0 / 0 and x / NaN: NaN, as the contract wants it)
}

// ln(v * 2^e) - lp, what the edit outputs hold: the logarithm of the mantissa in f32 (in [ln 0.5, 0): its rounding is below
// 2^-24), the exponents and the labelling's own ln P in float64.  v = 0: -inf; a NaN: NaN.
__device__ __forceinline__ float log_ratio(float v, int64_t e, double lp) {
    if (v == 0.0f) return -INFINITY;
    if (!(v > 0.0f) || v - v != 0.0f) return NAN;
    int ex;
    const float m = frexpf(v, &ex);
    return (float)((double)logf(m) + (double)(e + ex) * kLn2 - lp);
}

}  // namespace
}  // namespace fcd
