// crf_lattice.h -- what the walks of the lattice of a GIVEN labelling under a CRF model share: crf_lattice.hip (forward
// sum and best alignment) and crf_posterior.hip (forward and backward).  Parameter block, LDS layout, everything before
// the time loop (the rows without a value, the labelling and its state trajectory), the staging of the posteriors, the
// live window of a row, what a lane reads for one forward row -- and the FORWARD WALK itself (crf_forward_walk: sum, max
// with back-pointer ballots, sum with stored rows) and its twin for a window that lives in LDS (crf_forward_walk_lds: beyond
// 512 states, sum and stored rows).  What this lattice has in common with the CTC one (k(t), the rotations,
// ln P, the stored rows, the backward walks' stores) is ctc_lattice.h's.  Included by those translation units only.
#pragma once

#include <math.h>

#include <algorithm>

#include "ctc_lattice.h"

namespace fcd {
namespace {

constexpr uint32_t kNoState = 0xFFFFFFu;  // sigma outside 0 .. S-1: every posterior of the state reads as 0
struct CrfParams {
    BatchDesc in;
    ScoreDesc y;
    const float *init;
    int64_t n_init, init_stride;
    int band;
    int lab_cap;        // states (labels + 1) the LDS copy of a labelling holds
    int pow_m;          // S == nb^pow_m with nb >= 2, pow_m >= 1: sigma_k is a function of the last pow_m labels; 0: serial scan
    int staged;         // whole rows in LDS (S * N <= kTileElems)
    int rows_per_tile;  // rows between two fills (staged: what the tile holds; gather: kTileRows)
    // the cone's margins, in states: a labelling one label shorter reaches the end from one state lower (forward) and is
    // one state further at every row (backward).  0 everywhere but in the launches of fcd_crf_edits_* (crf_posterior.hip)
    int cone_lo, cone_hi;
    double *logp;
    // align only
    uint32_t *start;
    uint32_t *count;
    float *qual;
    unsigned char *bp;
    int64_t bp_row_bytes;
    // motif occurrence posteriors (fcd_crf_detect_*: crf_detect_walk below); null in every other launch
    const CrfDetectOut *det;
    // motif spotting (fcd_crf_spot_*: crf_spot_walk below); null in every other launch.  start / count / qual / bp above are
    // its spans, all null when none are asked for
    const CrfSpotOut *spot;
};

struct CrfLds {
    float *tile;     // kTileElems raw posteriors; the traceback's chunk afterwards
    int *krow;
    int *misc;       // [16] bad-label flag, [17] kBadPost, [18] the final cell
    uint32_t *info;  // per state k: sigma_k (kNoState: outside the table) | y_k << 24 (0 for state L)
};

__device__ __forceinline__ CrfLds crf_carve(unsigned char *smem) {
    CrfLds l;
    l.tile = reinterpret_cast<float *>(smem);
    l.krow = reinterpret_cast<int *>(smem + kTileElems * 4);
    l.misc = l.krow + kTileRows;
    l.info = reinterpret_cast<uint32_t *>(l.misc + kMiscWords);
    return l;
}

inline size_t crf_lds_bytes(int lab_cap) { return (size_t)kTileElems * 4 + (kTileRows + kMiscWords) * 4 + (size_t)lab_cap * 4; }

struct CrfRow {
    const float *post;
    const uint32_t *path;
    int Tr, L;
};

__device__ __forceinline__ int int_from_prev_lane(int x) {  // wave_ror:1
    return __builtin_amdgcn_update_dpp(0, x, 0x13C, 0xf, 0xf, false);
}

// Everything before the time loop: the rows without a value, the labelling and its state trajectory.  Returns false when
// the row's result is already written (every lane agrees).
__device__ __forceinline__ bool crf_prologue(const CrfParams &p, const CrfLds &lds, CrfRow *rw) {
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int64_t read = row / p.y.n_hyp;
    const int64_t hyp = row - read * p.y.n_hyp;
    const double nan = (double)NAN;
    if (p.y.n_valid && hyp >= (int64_t)p.y.n_valid[read]) {
        if (lane == 0) p.logp[row] = nan;
        return false;
    }
    int64_t Tr = p.in.lengths ? p.in.lengths[read] : p.in.T;
    Tr = Tr < 0 ? 0 : (Tr > p.in.T ? p.in.T : Tr);
    const uint32_t len = p.y.len[row];
    if ((int64_t)len > p.y.stride) {
        if (lane == 0) p.logp[row] = nan;
        return false;
    }
    const int L = (int)len;
    const uint8_t *labels = p.y.labels + row * p.y.stride;
    if (lane == 0) lds.misc[16] = 0;
    __syncthreads();
    bool bad = false;
    for (int k = lane; k < L; k += 64) {
        const int y = labels[k];
        bad |= y < 1 || y >= p.in.N;
    }
    if (bad) lds.misc[16] = 1;
    __syncthreads();
    double early = 0.0;
    bool done = true;
    if (lds.misc[16]) early = nan;
    else if (Tr == 0) early = L == 0 ? 0.0 : -(double)INFINITY;
    else if ((int64_t)L > Tr) early = -(double)INFINITY;
    else done = false;
    if (done) {
        if (lane == 0) p.logp[row] = early;
        return false;
    }
    // sigma_0: the first maximum of the init row (src/search.rs:58,404)
    const float *init = p.init + read * p.init_stride;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int64_t i = lane; i < p.n_init; i += 64) {
        float v = init[i];
        v = v != v ? -INFINITY : v;  // (a NaN counts as -inf)
        if (bi == 0x7fffffff || v > bv) {
            bv = v;
            bi = (int)i;
        }
    }
    for (int m = 1; m < 64; m <<= 1) {
        const float ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
        }
    }
    const int64_t S = p.in.S, nb = p.in.N - 1;
    // the trajectory sigma_{k+1} = (sigma_k * nb) mod S + (y_k - 1) (:97,414): serial up to where the closed form starts
    const int serial_end = p.pow_m > 0 ? min(p.pow_m - 1, L) : L;  // the last state of the serial scan
    if (lane == 0) {
        int64_t s = bi;
        for (int k = 0; k <= serial_end; ++k) {
            const uint32_t y = k < L ? labels[k] : 0u;
            lds.info[k] = ((s >= 0 && s < S) ? (uint32_t)s : kNoState) | (y << 24);
            if (k < L) s = (s * nb) % S + ((int64_t)y - 1);
        }
    }
    for (int k = serial_end + 1 + lane; k <= L; k += 64) {  // (pow_m labels behind state k exist: k >= pow_m)
        int64_t s = 0;
        for (int j = k - p.pow_m; j < k; ++j) s = s * nb + ((int64_t)labels[j] - 1);
        const uint32_t y = k < L ? labels[k] : 0u;
        lds.info[k] = (uint32_t)s | (y << 24);
    }
    if (lane == 0) lds.misc[kBadPost] = 0;
    __syncthreads();
    rw->post = post_at(p.in.post, read * p.in.stride_read, p.in.dtype);
    rw->path = p.y.path ? p.y.path + row * p.y.stride : nullptr;
    rw->Tr = (int)Tr;
    rw->L = L;
    return true;
}

// rows t0 .. t0 + rc of the read into the tile (staged shapes); banded: k(t) of each of them
__device__ __forceinline__ void crf_fill_tile(const CrfParams &p, const CrfLds &lds, const CrfRow &rw, int t0, int rc) {
    const int lane = threadIdx.x;
    __syncthreads();  // the previous tile's readers are done
    if (p.staged) {
        const int SN = p.in.S * p.in.N;
        for (int e = lane; e < rc * SN; e += 64) {
            const int i = e / SN, rem = e - i * SN;
            const int s = rem / p.in.N, j = rem - s * p.in.N;
            lds.tile[e] = load_post(rw.post, (int64_t)(t0 + i) * p.in.stride_t + (int64_t)s * p.in.stride_s + (int64_t)j * p.in.stride_n,
                                    p.in.dtype);
        }
    }
    if (p.band > 0 && lane < rc) lds.krow[lane] = labels_up_to(rw.path, rw.L, (uint32_t)(t0 + lane));
    __syncthreads();
}

// live states of row t, k = k(t): the band around the path, cut to what can be reached and can still reach the end -- the
// cone, widened by cone_hi states above and cone_lo below (never beyond the band's own bounds)
__device__ __forceinline__ void crf_window_of(const CrfParams &p, const CrfRow &rw, int t, int k, int cone_lo, int cone_hi,
                                              int *lo, int *hi) {
    int l = 0, h = rw.L;
    if (p.band > 0) {
        l = max(0, k - p.band);
        h = min(h, k + p.band);
    }
    *hi = min(h, t + 1 + cone_hi);
    *lo = max(l, rw.L - (rw.Tr - 1 - t) - cone_lo);
}

__device__ __forceinline__ void crf_window(const CrfParams &p, const CrfLds &lds, const CrfRow &rw, int t, int i, int *lo, int *hi) {
    crf_window_of(p, rw, t, p.band > 0 ? lds.krow[i] : 0, p.cone_lo, p.cone_hi, lo, hi);
}

// What a lane needs for one row, read a row ahead of its use (nothing here depends on alpha).  Per slot r: the two
// posteriors of the state the slot held in the PREVIOUS row, split, and whether their products enter a live cell.
template <int K>
struct CrfStep {
    float pm0[K], pmy[K];
    int pe0[K], pey[K];
    uint32_t stay_mask;  // bit r: the slot holds the same state in both rows, live in both
    uint32_t adv_mask;   // bit r: the state above the slot's previous one is live in this row
    uint32_t bad;        // a value that enters a live cell is NaN, infinite or negative
    int lo, hi;
};

// (crf_split: device_utils.h, shared with the CRF Viterbi search of crf_viterbi.hip)

template <int K>
__device__ __forceinline__ CrfStep<K> crf_load_step(const CrfParams &p, const CrfLds &lds, const CrfRow &rw, int t, int i,
                                                    int lo_prev, int hi_prev) {
    CrfStep<K> in;
    const int lane = threadIdx.x;
    crf_window(p, lds, rw, t, i, &in.lo, &in.hi);
    in.stay_mask = in.adv_mask = in.bad = 0;
    const int SN = p.in.S * p.in.N;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int kp = slot_state<K>(lane, r, lo_prev);
        const bool src = kp <= hi_prev;
        const uint32_t info = lds.info[src ? kp : 0];  // (a dead slot reads a valid address and is masked below)
        const uint32_t sig = info & 0xFFFFFFu, y = info >> 24;
        const bool stay = src && kp >= in.lo && kp <= in.hi;
        const bool adv = src && kp < rw.L && kp + 1 >= in.lo && kp + 1 <= in.hi;
        const bool table = sig != kNoState;
        float v0 = 0.0f, vy = 0.0f;
        if (p.staged) {
            const int base = i * SN + (int)(table ? sig : 0u) * p.in.N;
            if (stay && table) v0 = lds.tile[base];
            if (adv && table) vy = lds.tile[base + (int)y];
        } else {
            const int64_t base = (int64_t)t * p.in.stride_t + (int64_t)(table ? sig : 0u) * p.in.stride_s;
            if (stay && table) v0 = load_post(rw.post, base, p.in.dtype);
            if (adv && table) vy = load_post(rw.post, base + (int64_t)y * p.in.stride_n, p.in.dtype);
        }
        in.bad |= (!(v0 >= 0.0f && v0 - v0 == 0.0f) || !(vy >= 0.0f && vy - vy == 0.0f)) ? 1u : 0u;
        crf_split(v0, &in.pm0[r], &in.pe0[r]);
        crf_split(vy, &in.pmy[r], &in.pey[r]);
        in.stay_mask |= (stay ? 1u : 0u) << r;
        in.adv_mask |= (adv ? 1u : 0u) << r;
    }
    return in;
}

// The forward walk, from "row -1" to the final cell: the step and the numerics the head of crf_lattice.hip describes.
//   kCrfSum    the sum over the alignments (fcd_crf_score_*)
//   kCrfMax    the best alignment: max for +, and per row K 64-bit ballots "the advance won" in bp; a NaN, infinite or
//              negative posterior that entered a live cell is flagged in misc[kBadPost] (fcd_crf_align_*)
//   kCrfStore  the sum, and every row left for a backward walk (crf_posterior.hip): its cells in am by SLOT, scaled by
//              2^-kAlphaDown (a slot outside the row's window holds 0), its exponent in ae
// Returns the final cell alpha[L] of the last row (0 outside its window), the same in every lane, at the scale 2^*eacc_out:
// ln P = ln_p(m, eacc).
constexpr int kCrfSum = 0, kCrfMax = 1, kCrfStore = 2;

template <int MODE, int K>
__device__ __forceinline__ float crf_forward_walk(const CrfParams &p, const CrfLds &lds, const CrfRow &rw, uint64_t *bp, float *am,
                                                  int *ae, int64_t *eacc_out) {
    constexpr int C = 64 * K;
    constexpr bool MAX = MODE == kCrfMax;
    const int lane = threadIdx.x;
    float a[K];  // alpha of the state each of the lane's K slots holds, scaled by 2^-eacc
#pragma unroll
    for (int r = 0; r < K; ++r) a[r] = 0.0f;
    if (lane == 0) a[0] = 1.0f;  // "row -1": state 0, the one live state
    int64_t eacc = 0;
    int lo = 0, hi = 0;
    uint32_t bad = 0;
    for (int t0 = 0; t0 < rw.Tr; t0 += p.rows_per_tile) {
        const int rc = min(p.rows_per_tile, rw.Tr - t0);
        crf_fill_tile(p, lds, rw, t0, rc);
        CrfStep<K> in = crf_load_step<K>(p, lds, rw, t0, 0, lo, hi);
        for (int i = 0; i < rc; ++i) {
            CrfStep<K> nx = in;
            if (i + 1 < rc) nx = crf_load_step<K>(p, lds, rw, t0 + i + 1, i + 1, in.lo, in.hi);
            lo = in.lo;
            hi = in.hi;
            if constexpr (MAX) bad |= in.bad;
            float s[K], v[K];
#pragma unroll
            for (int r = 0; r < K; ++r) {
                s[r] = ((in.stay_mask >> r) & 1) ? a[r] * in.pm0[r] : 0.0f;
                v[r] = ((in.adv_mask >> r) & 1) ? a[r] * in.pmy[r] : 0.0f;
            }
            const float v_in = from_prev_lane(v[K - 1]);
            const int e_in = int_from_prev_lane(in.pey[K - 1]);
            float ua[K];
            int ea[K];
            int emax = kNoExp;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                ua[r] = r >= 1 ? v[r - 1] : v_in;
                ea[r] = r >= 1 ? in.pey[r - 1] : e_in;
                const int e0 = finite_exp(s[r]), e1 = finite_exp(ua[r]);
                emax = max(emax, e0 != kNoExp ? e0 + in.pe0[r] : kNoExp);
                emax = max(emax, e1 != kNoExp ? e1 + ea[r] : kNoExp);
            }
            emax = wave_imax(emax);
            const int sh = emax == kNoExp ? 0 : kTarget - emax;
            eacc -= sh;
            uint64_t mine = 0;
            float *row = MODE == kCrfStore ? am + (int64_t)(t0 + i) * C + lane * K : nullptr;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const float c0 = ldexpf(s[r], min(max(in.pe0[r] + sh, -512), 512));
                const float c1 = ldexpf(ua[r], min(max(ea[r] + sh, -512), 512));
                if constexpr (MAX) {
                    const bool up = c1 > c0;  // the stay candidate is kept unless the advance is strictly greater
                    a[r] = up ? c1 : c0;
                    const uint64_t word = __ballot(up);
                    if (lane == r) mine = word;
                } else {
                    a[r] = c0 + c1;
                }
                if constexpr (MODE == kCrfStore) row[r] = ldexpf(a[r], -kAlphaDown);
            }
            if constexpr (MAX) {
                if (lane < K) bp[(int64_t)(t0 + i) * K + lane] = mine;
            }
            if constexpr (MODE == kCrfStore) {
                if (lane == 0) ae[t0 + i] = (int)(eacc + kAlphaDown);
            }
            in = nx;
        }
    }
    if (lane == 0) lds.misc[18] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int k = slot_state<K>(lane, r, lo);
        if (k <= hi && k == rw.L) lds.misc[18] = __float_as_int(a[r]);
    }
    if (MAX && bad) lds.misc[kBadPost] = 1;
    __syncthreads();
    *eacc_out = eacc;
    return __int_as_float(lds.misc[18]);
}

// ---- kCrfDetect: motif occurrence posteriors, the expected number of occurrences under the CRF (fcd_crf_detect_*) ----
// A fourth forward walk, with a body of its own: it shares the tile, the slots and the source-lane products with the three
// above and none of their bookkeeping.  With h = min(L, m), cell k = h .. L - 1 ("k labels of the motif emitted") lives in
// slot k - h from the first row of the range to the last: the window never slides, so a slot's model state sigma_k and label
// y_k are loop invariants in one register (slot_state, the window of a row and its masks are not needed).
//   scale    every cell is a probability and an entry weight e_u is at most nb^(m-h+1) <= S < 2^24, so a cell stays below
//            T * S < 2^55 whatever the marginals add up to: the cells carry the FIXED factor 2^kDetScale = 2^64 (below 2^119,
//            no overflow) instead of a per-row exponent -- no wave_imax, no mantissa / exponent split, no reduction in the
//            row loop.  The price is a floor: a cell below 2^-190 as a probability is subnormal at that scale and loses
//            bits, one below 2^-213 counts as 0.
//   entry    e_u = the sum over the nb^(m-h+1) states whose last h - 1 labels are the motif's first of marg[u][sigma][y_(h-1)],
//            f32, in ascending order of the state: lane i sums row u0 + i of the next 64 rows into LDS (the k(t) words, which
//            a walk without a band does not use), and lane 0 reads one word a row into slot 0's advance.
//   step     s = a * p[u][sigma_k][0] and v = a * p[u][sigma_k][y_k] at the source lane, v one slot up (in the lane or by one
//            wave rotation), a = s + v: one rounding per product and per sum.  The posteriors come from the staged tile
//            or, S * N beyond it, from global memory a row ahead: crf_fill_tile's rule.
//   exit     c_u = the last cell's advance product (cell L is not walked): one readlane a row.  A slot above the last cell
//            reads its posteriors as 0; what travels into it never travels on.
//   result   c_u into a float64 sum in row order, into the running best (value, row) -- strictly greater only, so ties go
//            to the earliest row; both wave-uniform -- and, with a track, into lane u mod 64 until 64 rows are stored at
//            once: one logf and one store per lane.  L <= m: no cells, c_u = e_u straight from the LDS words.
// The range's first row takes the read's place: rows [b, e) are rows 0 .. e - b - 1 here.
constexpr int kCrfDetect = 3;
constexpr int kDetScale = 64;
constexpr uint32_t kCrfNoHit = 0xFFFFFFFFu;
constexpr float kCrfLn2f = 0.693147180559945309f;

// a row that does not walk
__device__ __forceinline__ void crf_detect_none(const CrfParams &p, double count, double logp) {
    if (threadIdx.x == 0) {
        p.det->count[blockIdx.x] = count;
        p.det->end[blockIdx.x] = kCrfNoHit;
        p.logp[blockIdx.x] = logp;
    }
}

struct CrfDetectAcc {
    double sum;  // c_b + .. so far, at the walk's scale
    float bv;    // the best c so far (0: none yet) ...
    int bt;      // ... and its row of the range
    float tv;    // lane j: c of row c0 + j of the 64 rows of `track` being staged
};

// The block's fields, a read's length and range come from global memory the kernel also writes: loaded once, ahead of the
// time loop, and pinned in scalar registers -- every loop bound derived from them stays scalar too.
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t wave_uniform(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
template <class T>
__device__ __forceinline__ T *wave_uniform(T *ptr) {
    return reinterpret_cast<T *>((uintptr_t)wave_uniform((int64_t)(uintptr_t)ptr));
}

// The track of a walk whose rows are complete one at a time: c (times 2^sc) of row t of the range, whose first row `track`
// points at, into lane t mod 64 (tv) until 64 rows -- or the range's last -- are stored at once, ln c in f32
__device__ __forceinline__ void crf_track_row(float *track, float &tv, float c, int sc, int t, int rows) {
    const int j = threadIdx.x;
    if (j == (t & 63)) tv = c;
    if ((t & 63) == 63 || t == rows - 1) {
        const int c0 = t & ~63;
        if (c0 + j <= t) {
            int ex = 0;
            const float m = frexpf(tv, &ex);
            track[c0 + j] = tv > 0.0f ? fmaf((float)(ex - sc), kCrfLn2f, logf(m)) : -INFINITY;
        }
    }
}

// c_t (times 2^sc) is complete; t: row of the range, whose first row `track` points at (null: no track)
__device__ __forceinline__ void crf_detect_row(float *track, CrfDetectAcc &acc, float c, int sc, int t, int rows) {
    acc.sum += (double)c;
    if (c > acc.bv) {
        acc.bv = c;
        acc.bt = t;
    }
    if (track) crf_track_row(track, acc.tv, c, sc, t, rows);
}

// What a lane reads for one row, a row ahead of its use: the two posteriors of the state each of its slots holds.  Where
// they sit in a row never changes, so a slot keeps two 32-bit offsets for the whole walk -- words into the staged tile's
// row, or bytes into the read's row in global memory (the launch's check: a row spans less than 2^31 bytes), which the
// load adds to a wave-uniform row address.  -1: a slot above the last cell, or a state outside the table: both read 0.
template <int K>
struct CrfDetectStep {
    float p0[K], py[K];
};

template <int K, bool STAGED>
__device__ __forceinline__ CrfDetectStep<K> crf_detect_load(const CrfParams &p, const CrfLds &lds, const float *post, const int (&off0)[K],
                                                            const int (&offy)[K], int t, int i, uint32_t *bad) {
    CrfDetectStep<K> in;
    const float *tile_row = lds.tile + i * (p.in.S * p.in.N);
    const uintptr_t post_row = (uintptr_t)post_at(post, (int64_t)t * p.in.stride_t, p.in.dtype);
#pragma unroll
    for (int r = 0; r < K; ++r) {
        float v0 = 0.0f, vy = 0.0f;
        if (off0[r] >= 0) {
            if (STAGED) {
                v0 = tile_row[off0[r]];
                vy = tile_row[offy[r]];
            } else {  // (opaque: the 64-bit sums are formed at the load, not kept in a register pair per value across rows)
                uint32_t o0 = (uint32_t)off0[r], oy = (uint32_t)offy[r];
                FCD_OPAQUE_VQ(o0);
                FCD_OPAQUE_VQ(oy);
                v0 = load_post_global(post_row + o0, p.in.dtype);
                vy = load_post_global(post_row + oy, p.in.dtype);
            }
        }
        *bad |= (!(v0 >= 0.0f && v0 - v0 == 0.0f) || !(vy >= 0.0f && vy - vy == 0.0f)) ? 1u : 0u;
        in.p0[r] = v0;
        in.py[r] = vy;
    }
    return in;
}

__device__ __forceinline__ float *crf_detect_etile(const CrfLds &lds) {  // (band 0: no k(t) in these 64 words)
    return reinterpret_cast<float *>(lds.krow);
}

// the entry weights of rows t0 .. t0 + 63 of the range: lane i sums row t0 + i, in ascending order of the state
__device__ __forceinline__ void crf_detect_entries(const CrfLds &lds, int t0, int rows, uint32_t *bad) {
    const int lane = threadIdx.x;
    __syncthreads();  // the previous 64 words' readers are done (and misc is written)
    if (t0 + lane < rows) {
        const int *w = lds.misc;
        const auto word = [w](int i) { return (int64_t)(((uint64_t)(uint32_t)w[2 * i + 1] << 32) | (uint32_t)w[2 * i]); };
        const int64_t stride_s = word(2);
        const float *at = reinterpret_cast<const float *>((uintptr_t)word(0)) + (int64_t)(t0 + lane) * word(1) + (int64_t)w[7] * stride_s;
        const int64_t step = (int64_t)w[6] * stride_s;
        float e = 0.0f;
        for (int d = 0; d < w[8]; ++d, at += step) {
            const float v = *at;
            *bad |= !(v >= 0.0f && v - v == 0.0f) ? 1u : 0u;
            e += v;
        }
        crf_detect_etile(lds)[lane] = e;
    }
}

// What crf_spot_walk does before its time loop, crf_detect_walk's statements: the rows without a value in
// fcd_crf_score_*'s order, the range of rows, the cells' trajectory in lds.info and the entry weights' parameters in
// lds.misc.  (Functions of their own, and crf_detect_walk keeps its text, so that the score kernels' detect copy compiles to
// what it was: sharing them moved crf_detect by 1.7 % on an MI355X at unchanged register counts.)
struct CrfMotif {
    int64_t read;
    int L, h, nc;  // labels; min(L, m); cells h .. L - 1
    int tb, rows;  // the range's first row and its length
};

// false: the row does not walk and *early is its logp (NaN; 0 for an empty motif; -inf for an empty range)
template <class OUT>
__device__ __forceinline__ bool crf_motif_prologue(const CrfParams &p, const CrfLds &lds, const OUT *out, CrfMotif *mo, double *early) {
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int64_t read = row / p.y.n_hyp;
    const int64_t hyp = row - read * p.y.n_hyp;
    *early = (double)NAN;
    if (p.y.n_valid && hyp >= (int64_t)p.y.n_valid[read]) return false;
    int64_t Tr = p.in.lengths ? wave_uniform(p.in.lengths[read]) : p.in.T;
    Tr = Tr < 0 ? 0 : (Tr > p.in.T ? p.in.T : Tr);
    const uint32_t len = (uint32_t)wave_uniform((int)p.y.len[row]);
    if ((int64_t)len > p.y.stride) return false;
    const int L = (int)len;
    const uint8_t *labels = p.y.labels + row * p.y.stride;
    if (lane == 0) lds.misc[16] = lds.misc[kBadPost] = 0;
    __syncthreads();
    bool bad_label = false;
    for (int k = lane; k < L; k += 64) {
        const int y = labels[k];
        bad_label |= y < 1 || y >= p.in.N;
    }
    if (bad_label) lds.misc[16] = 1;
    __syncthreads();
    if (lds.misc[16]) return false;
    *early = 0.0;
    if (L == 0) return false;
    const uint32_t *row_begin = wave_uniform(out->row_begin), *row_end = wave_uniform(out->row_end);
    const int tb = row_begin ? (int)min((int64_t)(uint32_t)wave_uniform((int)row_begin[read]), Tr) : 0;
    const int te = row_end ? (int)min((int64_t)(uint32_t)wave_uniform((int)row_end[read]), Tr) : (int)Tr;
    const int rows = te - tb;
    *early = -(double)INFINITY;
    if (rows <= 0) return false;
    // the entry states d * q + prefix, d = 0 .. ne - 1, and the label they emit; the cells' trajectory, from the motif alone
    const int S = p.in.S, nb = p.in.N - 1;
    const int m = p.pow_m > 0 ? p.pow_m : 1;  // (S = 1 walks as m = 1: a state outside the table reads 0)
    const int h = min(L, m), nc = L - h;
    int q = 1, prefix = 0;
    for (int j = 0; j < h - 1; ++j) {
        prefix = prefix * nb + ((int)labels[j] - 1);
        q *= nb;
    }
    for (int j = lane; j < nc; j += 64) {  // (nc > 0: h = m, so the m labels behind cell k = m + j exist)
        int64_t s = 0;
        for (int g = j; g < j + m; ++g) s = s * nb + ((int64_t)labels[g] - 1);
        lds.info[j] = (s < S ? (uint32_t)s : kNoState) | ((uint32_t)labels[j + m] << 24);
    }
    __syncthreads();
    // the entry weights' parameters wait in LDS (misc[0 .. 8], free in a CRF walk): read once per 64 rows, they take no
    // scalar registers from the row loop
    if (lane == 0) {
        const float *marg = out->marg + read * out->marg_stride_read + (int64_t)tb * out->marg_stride_t + labels[h - 1];
        const int64_t words[3] = {(int64_t)(uintptr_t)marg, out->marg_stride_t, out->marg_stride_s};
        for (int w = 0; w < 3; ++w) {
            lds.misc[2 * w] = (int)(uint32_t)words[w];
            lds.misc[2 * w + 1] = (int)(uint32_t)((uint64_t)words[w] >> 32);
        }
        lds.misc[6] = q;
        lds.misc[7] = prefix;
        lds.misc[8] = (S - prefix + q - 1) / q;  // the states below S among them: all nb^(m-h+1) where S = nb^m
    }
    *mo = CrfMotif{read, L, h, nc, tb, rows};
    return true;
}

// a slot's two constant offsets (crf_detect_load), from lds.info as the prologue left it
template <int K, bool STAGED>
__device__ __forceinline__ void crf_motif_offsets(const CrfParams &p, const CrfLds &lds, int nc, int (&off0)[K], int (&offy)[K]) {
    const int lane = threadIdx.x;
    const int esz = p.in.dtype == kF32 ? 4 : 2;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const uint32_t info = lane * K + r < nc ? lds.info[lane * K + r] : kNoState;
        const int sig = (int)(info & 0xFFFFFFu), y = (int)(info >> 24);
        off0[r] = STAGED ? sig * p.in.N : (int)(sig * p.in.stride_s) * esz;
        offy[r] = off0[r] + (STAGED ? y : (int)(y * p.in.stride_n) * esz);
        if ((uint32_t)sig == kNoState) off0[r] = offy[r] = -1;
    }
}

// STAGED: CrfParams::staged as a compile-time copy of the function (not of the kernel): each copy keeps one kind of offset
template <int K, bool STAGED>
__device__ __forceinline__ void crf_detect_walk(const CrfParams &p, const CrfLds &lds) {
    const CrfDetectOut *det = p.det;
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    const int64_t read = row / p.y.n_hyp;
    const int64_t hyp = row - read * p.y.n_hyp;
    const double nan = (double)NAN;
    // the rows without a value, in fcd_crf_score_*'s order
    if (p.y.n_valid && hyp >= (int64_t)p.y.n_valid[read]) return crf_detect_none(p, nan, nan);
    int64_t Tr = p.in.lengths ? wave_uniform(p.in.lengths[read]) : p.in.T;
    Tr = Tr < 0 ? 0 : (Tr > p.in.T ? p.in.T : Tr);
    const uint32_t len = (uint32_t)wave_uniform((int)p.y.len[row]);
    if ((int64_t)len > p.y.stride) return crf_detect_none(p, nan, nan);
    const int L = (int)len;
    const uint8_t *labels = p.y.labels + row * p.y.stride;
    if (lane == 0) lds.misc[16] = lds.misc[kBadPost] = 0;
    __syncthreads();
    bool bad_label = false;
    for (int k = lane; k < L; k += 64) {
        const int y = labels[k];
        bad_label |= y < 1 || y >= p.in.N;
    }
    if (bad_label) lds.misc[16] = 1;
    __syncthreads();
    if (lds.misc[16]) return crf_detect_none(p, nan, nan);
    if (L == 0) return crf_detect_none(p, 0.0, 0.0);
    const uint32_t *row_begin = wave_uniform(det->row_begin), *row_end = wave_uniform(det->row_end);
    const int tb = row_begin ? (int)min((int64_t)(uint32_t)wave_uniform((int)row_begin[read]), Tr) : 0;
    const int te = row_end ? (int)min((int64_t)(uint32_t)wave_uniform((int)row_end[read]), Tr) : (int)Tr;
    const int rows = te - tb;
    if (rows <= 0) return crf_detect_none(p, 0.0, -(double)INFINITY);
    // the entry states d * q + prefix, d = 0 .. ne - 1, and the label they emit; the cells' trajectory, from the motif alone
    const int S = p.in.S, nb = p.in.N - 1;
    const int m = p.pow_m > 0 ? p.pow_m : 1;  // (S = 1 walks as m = 1: a state outside the table reads 0)
    const int h = min(L, m), nc = L - h;
    int q = 1, prefix = 0;
    for (int j = 0; j < h - 1; ++j) {
        prefix = prefix * nb + ((int)labels[j] - 1);
        q *= nb;
    }
    for (int j = lane; j < nc; j += 64) {  // (nc > 0: h = m, so the m labels behind cell k = m + j exist)
        int64_t s = 0;
        for (int g = j; g < j + m; ++g) s = s * nb + ((int64_t)labels[g] - 1);
        lds.info[j] = (s < S ? (uint32_t)s : kNoState) | ((uint32_t)labels[j + m] << 24);
    }
    __syncthreads();
    int off0[K], offy[K];
    const int esz = p.in.dtype == kF32 ? 4 : 2;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const uint32_t info = lane * K + r < nc ? lds.info[lane * K + r] : kNoState;
        const int sig = (int)(info & 0xFFFFFFu), y = (int)(info >> 24);
        off0[r] = STAGED ? sig * p.in.N : (int)(sig * p.in.stride_s) * esz;
        offy[r] = off0[r] + (STAGED ? y : (int)(y * p.in.stride_n) * esz);
        if ((uint32_t)sig == kNoState) off0[r] = offy[r] = -1;
    }
    // the entry weights' parameters wait in LDS (misc[0 .. 8], free in a CRF walk): read once per 64 rows, they take no
    // scalar registers from the row loop
    if (lane == 0) {
        const float *marg = det->marg + read * det->marg_stride_read + (int64_t)tb * det->marg_stride_t + labels[h - 1];
        const int64_t words[3] = {(int64_t)(uintptr_t)marg, det->marg_stride_t, det->marg_stride_s};
        for (int w = 0; w < 3; ++w) {
            lds.misc[2 * w] = (int)(uint32_t)words[w];
            lds.misc[2 * w + 1] = (int)(uint32_t)((uint64_t)words[w] >> 32);
        }
        lds.misc[6] = q;
        lds.misc[7] = prefix;
        lds.misc[8] = (S - prefix + q - 1) / q;  // the states below S among them: all nb^(m-h+1) where S = nb^m
    }
    float *track = wave_uniform(det->track);
    if (track) track += row * wave_uniform(det->track_stride) + tb;
    CrfDetectAcc acc{0.0, 0.0f, -1, 0.0f};
    uint32_t bad = 0;
    int sc = 0;
    if (nc == 0) {  // L <= m: c_u = e_u, 64 rows at a time
        for (int t0 = 0; t0 < rows; t0 += 64) {
            crf_detect_entries(lds, t0, rows, &bad);
            __syncthreads();
            for (int i = 0; i < min(64, rows - t0); ++i) crf_detect_row(track, acc, crf_detect_etile(lds)[i], 0, t0 + i, rows);
        }
    } else {
        sc = kDetScale;
        CrfRow rw;
        rw.post = post_at(p.in.post, read * p.in.stride_read + (int64_t)tb * p.in.stride_t, p.in.dtype);
        rw.path = nullptr;
        rw.Tr = rows;
        rw.L = L;
        const int end_lane = (nc - 1) / K, end_r = (nc - 1) % K;
        float a[K];
#pragma unroll
        for (int r = 0; r < K; ++r) a[r] = 0.0f;
        for (int t0 = 0; t0 < rows;) {
            // a tile ends where the staged rows end and where the next 64 entry weights begin
            const int rc = min(min(p.rows_per_tile, rows - t0), 64 - (t0 & 63));
            if ((t0 & 63) == 0) crf_detect_entries(lds, t0, rows, &bad);
            crf_fill_tile(p, lds, rw, t0, rc);  // (its barriers order the 64 words too)
            CrfDetectStep<K> in = crf_detect_load<K, STAGED>(p, lds, rw.post, off0, offy, t0, 0, &bad);
            for (int i = 0; i < rc; ++i) {
                const float e = crf_detect_etile(lds)[(t0 + i) & 63];
                float s[K], v[K];
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    s[r] = a[r] * in.p0[r];
                    v[r] = a[r] * in.py[r];
                }
                // the next row's posteriors, into the registers the products have just freed: their latency is the rest of this row
                if (i + 1 < rc) in = crf_detect_load<K, STAGED>(p, lds, rw.post, off0, offy, t0 + i + 1, i + 1, &bad);
                float mine = 0.0f;
#pragma unroll
                for (int r = 0; r < K; ++r)
                    if (r == end_r) mine = v[r];
                const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), end_lane));
                float v_in = from_prev_lane(v[K - 1]);
                if (lane == 0) v_in = e * 0x1p64f;  // slot 0's advance is the entry weight, at the walk's scale (exact)
#pragma unroll
                for (int r = 0; r < K; ++r) a[r] = s[r] + (r >= 1 ? v[r - 1] : v_in);
                crf_detect_row(track, acc, c, kDetScale, t0 + i, rows);
            }
            t0 += rc;
        }
    }
    if (bad) lds.misc[kBadPost] = 1;
    __syncthreads();
    if (lane == 0) {
        const bool flagged = lds.misc[kBadPost] != 0, hit = acc.bt >= 0;
        det->count[row] = flagged ? nan : ldexp(acc.sum, -sc);
        det->end[row] = flagged || !hit ? kCrfNoHit : (uint32_t)(tb + acc.bt);
        p.logp[row] = flagged ? nan : (hit ? ln_p((double)acc.bv, -sc) : -(double)INFINITY);
    }
}

// ---- kCrfSpot: motif spotting, the best single occurrence and its rows under the CRF (fcd_crf_spot_*) ----
// crf_detect_walk's lattice with max in the place of +, compiled into the ALIGNMENT's kernels (crf_lattice_kernel<true, K>)
// and chosen once by CrfParams::spot.  Window, slots, offsets, scale, entry weights, source-lane products and the exit are
// the detect walk's, word for word; what is its own:
//   first    every cell carries, next to its value, the row at which its best path entered (u0, K more registers): the
//            compare that picks the max picks it too, and it travels one slot up with the advance product.  The lane that
//            owns cell L - 1 so knows the hit's first row at the exit: (first, end, logp, track) need no back-pointer and
//            no workspace.  The exit stays one readlane a row; the second one (u0) is read only where the row is a new best.
//   ballots  only where spans are asked for (bp, wave-uniform, tested outside the products): K 64-bit words a row, bit `lane`
//            of word r = "the advance or the entry won, strictly" in slot lane * K + r -- the kCrfMax walk's layout.
//   trace    after the walk, from cell L - 1 at row end - 1 down to the entry bit of cell h, 64 rows at a time through the
//            tile area: rows first .. end - 1 only.  A set bit in slot j at row t is the emission row of y_(h+j-1).
// Candidates in the order stay, then advance or entry: the later one only if strictly greater.
struct CrfSpotAcc {
    float bv;    // the best v so far (0: none yet) ...
    int bt, bf;  // ... its row of the range, and the row its path entered at
    float tv;    // crf_track_row's staging word
};

// a row that does not walk
__device__ __forceinline__ void crf_spot_none(const CrfParams &p, double logp) {
    const int64_t row = blockIdx.x;
    if (threadIdx.x == 0) {
        p.spot->end[row] = kCrfNoHit;
        p.spot->first[row] = kCrfNoHit;
        p.logp[row] = logp;
    }
    if (p.count) {
        const int64_t n = min((int64_t)p.y.len[row], p.y.stride);
        for (int64_t k = threadIdx.x; k < n; k += 64) p.count[row * p.y.stride + k] = 0u;
    }
}

template <int K, bool STAGED>
__device__ __forceinline__ void crf_spot_walk(const CrfParams &p, const CrfLds &lds) {
    const CrfSpotOut *sp = p.spot;
    const int lane = threadIdx.x;
    const int64_t row = blockIdx.x;
    CrfMotif mo;
    double early;
    if (!crf_motif_prologue(p, lds, sp, &mo, &early)) return crf_spot_none(p, early);
    const int L = mo.L, h = mo.h, nc = mo.nc, tb = mo.tb, rows = mo.rows;
    int off0[K], offy[K];
    crf_motif_offsets<K, STAGED>(p, lds, nc, off0, offy);
    float *track = wave_uniform(sp->track);
    if (track) track += row * wave_uniform(sp->track_stride) + tb;
    uint64_t *bp = p.start ? reinterpret_cast<uint64_t *>(p.bp + row * p.bp_row_bytes) : nullptr;
    CrfSpotAcc acc{0.0f, -1, -1, 0.0f};
    uint32_t bad = 0;
    int sc = 0;
    if (nc == 0) {  // L <= m: v_u = e_u, the hit is one row
        for (int t0 = 0; t0 < rows; t0 += 64) {
            crf_detect_entries(lds, t0, rows, &bad);
            __syncthreads();
            for (int i = 0; i < min(64, rows - t0); ++i) {
                const float c = crf_detect_etile(lds)[i];
                if (c > acc.bv) {
                    acc.bv = c;
                    acc.bt = acc.bf = t0 + i;
                }
                if (track) crf_track_row(track, acc.tv, c, 0, t0 + i, rows);
            }
        }
    } else {
        sc = kDetScale;
        CrfRow rw;
        rw.post = post_at(p.in.post, mo.read * p.in.stride_read + (int64_t)tb * p.in.stride_t, p.in.dtype);
        rw.path = nullptr;
        rw.Tr = rows;
        rw.L = L;
        const int end_lane = (nc - 1) / K, end_r = (nc - 1) % K;
        float a[K];
        int u0[K];
#pragma unroll
        for (int r = 0; r < K; ++r) {
            a[r] = 0.0f;
            u0[r] = 0;
        }
        for (int t0 = 0; t0 < rows;) {
            // a tile ends where the staged rows end and where the next 64 entry weights begin
            const int rc = min(min(p.rows_per_tile, rows - t0), 64 - (t0 & 63));
            if ((t0 & 63) == 0) crf_detect_entries(lds, t0, rows, &bad);
            crf_fill_tile(p, lds, rw, t0, rc);  // (its barriers order the 64 words too)
            CrfDetectStep<K> in = crf_detect_load<K, STAGED>(p, lds, rw.post, off0, offy, t0, 0, &bad);
            for (int i = 0; i < rc; ++i) {
                const int t = t0 + i;
                const float e = crf_detect_etile(lds)[t & 63];
                float s[K], v[K];
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    s[r] = a[r] * in.p0[r];
                    v[r] = a[r] * in.py[r];
                }
                if (i + 1 < rc) in = crf_detect_load<K, STAGED>(p, lds, rw.post, off0, offy, t + 1, i + 1, &bad);
                float mine = 0.0f;
                int mine_u = 0;
#pragma unroll
                for (int r = 0; r < K; ++r)
                    if (r == end_r) {
                        mine = v[r];
                        mine_u = u0[r];
                    }
                const float c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), end_lane));
                if (c > acc.bv) {  // (wave-uniform) strictly greater only: ties go to the earliest row
                    acc.bv = c;
                    acc.bt = t;
                    acc.bf = __builtin_amdgcn_readlane(mine_u, end_lane);
                }
                float v_in = from_prev_lane(v[K - 1]);
                int u_in = int_from_prev_lane(u0[K - 1]);
                if (lane == 0) {  // slot 0's advance is the entry, at the walk's scale (exact), and it enters here
                    v_in = e * 0x1p64f;
                    u_in = t;
                }
                bool up[K];
#pragma unroll
                for (int r = K - 1; r >= 0; --r) {  // (from the top: u0[r - 1] is still the previous row's)
                    const float adv = r >= 1 ? v[r - 1] : v_in;
                    up[r] = adv > s[r];
                    a[r] = up[r] ? adv : s[r];
                    u0[r] = up[r] ? (r >= 1 ? u0[r - 1] : u_in) : u0[r];
                }
                if (bp) {
                    uint64_t word = 0;
#pragma unroll
                    for (int r = 0; r < K; ++r) {
                        const uint64_t w = __ballot(up[r]);
                        if (lane == r) word = w;
                    }
                    if (lane < K) bp[(int64_t)t * K + lane] = word;
                }
                if (track) crf_track_row(track, acc.tv, c, kDetScale, t, rows);
            }
            t0 += rc;
        }
    }
    if (bad) lds.misc[kBadPost] = 1;
    __syncthreads();
    const bool flagged = lds.misc[kBadPost] != 0;
    if (flagged || acc.bt < 0) return crf_spot_none(p, flagged ? (double)NAN : -(double)INFINITY);
    if (lane == 0) {
        sp->end[row] = (uint32_t)(tb + acc.bt);
        sp->first[row] = (uint32_t)(tb + acc.bf);
        p.logp[row] = ln_p((double)acc.bv, -sc);
    }
    if (!p.start) return;
    // the spans: labels 0 .. h - 2 lie in the model's history and are not located; y_(h-1) is emitted at the entry, y_(L-1)
    // at the hit's last row, the others where the trace finds their cells entered
    uint32_t *start = p.start + row * p.y.stride, *count = p.count + row * p.y.stride;
    float *qual = p.qual + row * p.y.stride;
    for (int k = lane; k < L; k += 64) {
        const bool located = k >= h - 1;
        count[k] = located ? 1u : 0u;
        start[k] = located ? (uint32_t)(tb + acc.bt) : kCrfNoHit;  // (a row of the read, whatever the trace finds)
        if (!located) qual[k] = 0.0f;
    }
    __syncthreads();
    if (lane == 0) {
        start[h - 1] = (uint32_t)(tb + acc.bf);
        start[L - 1] = (uint32_t)(tb + acc.bt);
    }
    uint64_t *sbp = reinterpret_cast<uint64_t *>(lds.tile);
    int j = nc - 1;  // the cell the path is in at row t: (nc == 0: no walk, no trace)
    for (int c0 = (acc.bt - 1) & ~63; j >= 0 && c0 >= 0 && c0 + 63 >= acc.bf; c0 -= 64) {
        const int n = min(64, acc.bt - c0);  // rows c0 .. end - 1
        __syncthreads();
        for (int e = lane; e < n * K; e += 64) sbp[e] = bp[(int64_t)c0 * K + e];
        __syncthreads();
        for (int i = n - 1; i >= 0 && j >= 0 && c0 + i >= acc.bf; --i) {
            const uint64_t word = sbp[i * K + j % K];
            const int d = __builtin_amdgcn_readfirstlane((int)((word >> (j / K)) & 1u));
            if (d) {  // cell h + j was entered at this row: y_(h+j-1) is emitted here (j = 0: the entry, written above)
                if (lane == 0 && j > 0) start[h + j - 1] = (uint32_t)(tb + c0 + i);
                j -= 1;
            }
        }
    }
    // the qualities, as the alignment writes them: p[start_k][sigma_k][y_k] for k >= h, the entry weight for k = h - 1
    crf_detect_entries(lds, acc.bf & ~63, rows, &bad);
    __syncthreads();  // ... and start as the trace left it
    if (lane == 0) qual[h - 1] = crf_detect_etile(lds)[acc.bf & 63];
    const float *post = post_at(p.in.post, mo.read * p.in.stride_read, p.in.dtype);
    for (int k = h + lane; k < L; k += 64) {
        const uint32_t info = lds.info[k - h];
        const uint32_t sig = info & 0xFFFFFFu;
        const int64_t at = (int64_t)start[k] * p.in.stride_t + (int64_t)sig * p.in.stride_s + (int64_t)(info >> 24) * p.in.stride_n;
        qual[k] = sig != kNoState ? load_post(post, at, p.in.dtype) : 0.0f;
    }
}

// ---- the LDS-resident window: J = 9 .. 64 states per lane, state k in slot k mod 64J, lane l owns slots lJ .. lJ + J - 1 ----
// (fcd_set_crf_lattice_wide of include/fcd.h: windows beyond the 512 states eight registers per lane hold).  Three rows of
// 64J words behind what the launch's other users of LDS take: the cells, the advance products, the packed exponents.  A
// slot's word sits at (slot mod J) * 64 + slot / J in its row -- a lane's J cells are 64 words apart, so the 64 lanes of one
// access touch 64 consecutive words -- and the stored rows of the workspace keep that order.
struct CrfWideLds {
    float *cell;    // alpha (forward), beta (backward) of the state each slot holds; between a row's two passes the stay products
    float *up;      // the products that leave their slot: the advance products (forward), beta[s + 1] P(u, s, y_s) (backward)
    uint32_t *exp;  // per slot: both products' posterior exponents, and the occupancy walk's two "a term was added" bits
};

__device__ __forceinline__ CrfWideLds crf_wide_carve(void *behind, int J) {
    CrfWideLds w;
    w.cell = reinterpret_cast<float *>(behind);
    w.up = w.cell + 64 * J;
    w.exp = reinterpret_cast<uint32_t *>(w.up + 64 * J);
    return w;
}

inline size_t crf_wide_lds_bytes(int J) { return (size_t)3 * 64 * (size_t)J * 4; }

__device__ __forceinline__ int crf_wide_at(int lane, int j) { return j * 64 + lane; }

__device__ __forceinline__ int crf_wide_state(int slot, int lo, int C) {  // the state >= lo that lives in the slot
    const int s = lo / C * C + slot;
    return s < lo ? s + C : s;
}

// the exponents of a split posterior lie in -148 .. 128 (0 for a value that is not finite): nine bits each, biased by 256
__device__ __forceinline__ uint32_t crf_wide_pack(int e0, int ey) { return (uint32_t)(e0 + 256) | ((uint32_t)(ey + 256) << 9); }
__device__ __forceinline__ int crf_wide_e0(uint32_t w) { return (int)(w & 511u) - 256; }
__device__ __forceinline__ int crf_wide_ey(uint32_t w) { return (int)((w >> 9) & 511u) - 256; }

// crf_forward_walk for such a window, kCrfSum and kCrfStore: the same products, the same exponent and the same sum per cell,
// so the same numerics.  A row is two passes over the lane's J cells.  The first forms both products of the state each slot
// held in the previous row, leaves the stay product in the cell, the advance product in `up` and takes the row's largest
// exponent; the second rescales and adds its own stay product and the advance product of the slot below -- the alpha row is
// updated IN PLACE, and what a lane reads of its neighbour (the top slot's advance product) is in a row the second pass only
// reads.  Posteriors: from the staged tile, or (S * N beyond it) gathered from global memory as the first pass needs them.
// Stored rows: T * 64J cells, a slot's at crf_wide_at, scaled by 2^-kAlphaDown, then T exponent words -- stored_rows_bytes(T, J).
// kCrfStore with a null `am` stores nothing, decided at run time: crfp_fwd_kernel<8> compiles this one body for both of its
// uses (half the cold code next to its register walk); kCrfSum is the same decision at compile time.
template <int MODE>
__device__ __forceinline__ float crf_forward_walk_lds(const CrfParams &p, const CrfLds &lds, const CrfRow &rw, const CrfWideLds &w,
                                                      int J, float *am, int *ae, int64_t *eacc_out) {
    static_assert(MODE == kCrfSum || MODE == kCrfStore, "the best alignment keeps its 512 states");
    const int C = 64 * J;
    const int lane = threadIdx.x;
    const int SN = p.in.S * p.in.N;
    for (int j = 0; j < J; ++j) w.cell[crf_wide_at(lane, j)] = 0.0f;
    if (lane == 0) w.cell[0] = 1.0f;  // "row -1": state 0, the one live state
    int64_t eacc = 0;
    int lo = 0, hi = 0;  // the window of the previous row
    for (int t0 = 0; t0 < rw.Tr; t0 += p.rows_per_tile) {
        const int rc = min(p.rows_per_tile, rw.Tr - t0);
        crf_fill_tile(p, lds, rw, t0, rc);
        for (int i = 0; i < rc; ++i) {
            const int t = t0 + i;
            int lo_t, hi_t;
            crf_window(p, lds, rw, t, i, &lo_t, &hi_t);
            int emax = kNoExp;
            for (int j = 0; j < J; ++j) {
                const int at = crf_wide_at(lane, j);
                const int kp = crf_wide_state(lane * J + j, lo, C);
                const bool src = kp <= hi;
                const uint32_t info = lds.info[src ? kp : 0];  // (a dead slot reads a valid address and is masked below)
                const uint32_t sig = info & 0xFFFFFFu, y = info >> 24;
                const bool table = sig != kNoState;
                const bool stay = src && kp >= lo_t && kp <= hi_t;
                const bool adv = src && kp < rw.L && kp + 1 >= lo_t && kp + 1 <= hi_t;
                float v0 = 0.0f, vy = 0.0f;  // (a state outside the table reads 0, as in crf_load_step)
                if (p.staged) {
                    const int base = i * SN + (int)(table ? sig : 0u) * p.in.N;
                    if (stay && table) v0 = lds.tile[base];
                    if (adv && table) vy = lds.tile[base + (int)y];
                } else {
                    const int64_t base = (int64_t)t * p.in.stride_t + (int64_t)(table ? sig : 0u) * p.in.stride_s;
                    if (stay && table) v0 = load_post(rw.post, base, p.in.dtype);
                    if (adv && table) vy = load_post(rw.post, base + (int64_t)y * p.in.stride_n, p.in.dtype);
                }
                float m0, my;
                int e0, ey;
                crf_split(v0, &m0, &e0);
                crf_split(vy, &my, &ey);
                const float a = w.cell[at];
                const float s = stay ? a * m0 : 0.0f;
                const float v = adv ? a * my : 0.0f;
                const int x0 = finite_exp(s), x1 = finite_exp(v);
                emax = max(emax, x0 != kNoExp ? x0 + e0 : kNoExp);
                emax = max(emax, x1 != kNoExp ? x1 + ey : kNoExp);
                w.cell[at] = s;
                w.up[at] = v;
                w.exp[at] = crf_wide_pack(e0, ey);
            }
            emax = wave_imax(emax);
            const int sh = emax == kNoExp ? 0 : kTarget - emax;
            eacc -= sh;
            __syncthreads();  // every advance product is in its slot
            float *row = MODE == kCrfStore && am ? am + (int64_t)t * C : nullptr;
            // the slot below the lane's first: the previous lane's top (lane 0: the top slot of the window)
            int below = crf_wide_at((lane + 63) & 63, J - 1);
            for (int j = 0; j < J; ++j) {
                const int at = crf_wide_at(lane, j);
                const float c0 = ldexpf(w.cell[at], min(max(crf_wide_e0(w.exp[at]) + sh, -512), 512));
                const float c1 = ldexpf(w.up[below], min(max(crf_wide_ey(w.exp[below]) + sh, -512), 512));
                const float a = c0 + c1;
                w.cell[at] = a;
                if (MODE == kCrfStore && am) row[at] = ldexpf(a, -kAlphaDown);
                below = at;
            }
            if (MODE == kCrfStore && am) {
                if (lane == 0) ae[t] = (int)(eacc + kAlphaDown);
            }
            lo = lo_t;
            hi = hi_t;
            __syncthreads();  // ... and read before the next row writes over it
        }
    }
    const int slot = rw.L % C;
    const float last = (rw.L >= lo && rw.L <= hi) ? w.cell[crf_wide_at(slot / J, slot % J)] : 0.0f;  // (every lane reads the one word)
    *eacc_out = eacc;
    return last;
}

CrfParams crf_params(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                     int64_t band) {
    CrfParams p{};
    p.in = in;
    p.y = y;
    p.init = init;
    p.n_init = n_init;
    p.init_stride = init_stride;
    p.band = (int)band;
    p.lab_cap = (int)std::min(in.T, y.stride) + 1;
    const int64_t nb = in.N - 1, SN = (int64_t)in.S * in.N;
    p.pow_m = 0;
    if (nb >= 2) {
        int m = 0;
        int64_t v = 1;
        while (v < in.S) {
            v *= nb;
            ++m;
        }
        if (v == in.S && m >= 1) p.pow_m = m;
    }
    p.staged = SN <= kTileElems;
    p.rows_per_tile = p.staged ? (int)std::min<int64_t>(kTileRows, kTileElems / SN) : kTileRows;
    return p;
}

int crf_states_per_lane(int64_t T, int64_t stride, int64_t band) {
    const int64_t states = crf_lattice_window_states(T, stride, band);
    return states <= 64 ? 1 : (states <= 128 ? 2 : (states <= 256 ? 4 : 8));
}

}  // namespace
}  // namespace fcd
