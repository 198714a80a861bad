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
