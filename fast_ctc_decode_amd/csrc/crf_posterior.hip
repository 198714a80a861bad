// crf_posterior.hip -- forward-backward substitution posteriors of given labellings under a CRF model
// (fcd_crf_posterior_*; include/fcd.h): post[k][c] = P(y[k:=c] | x) / sum_c' P(y[k:=c'] | x) for every label position k
// and every label c, from ONE forward and ONE backward walk of the lattice crf_lattice.hip sums over.  NOT a reference
// function.
//
// In a CRF the model state sigma_k is the history of the last m labels (S == nb^m, nb = N - 1): the variant y[k:=c] reads
// other posterior rows than y in the states k + 1 .. k + m, sigma'_{k+j} = sigma_{k+j} + (c - y_k) nb^(j-1), and rejoins y's
// trajectory at state k + m + 1.  The backward walk carries that: next to beta[s], state s holds the chain values
// V_s[j][c], j = 1 .. min(m, s) -- the backward value state s has in the variant that substituted c at position s - j.
// S == 1 walks as m = 1: the trajectory rule gives sigma_{k+1} = y_k - 1 there, which is the table's one row for label 1 and
// outside the table (every posterior reads as 0) for any other label -- for y as for its variants.
//
// Two launches, one wavefront per labelling each, the register-resident window of crf_lattice.hip (K consecutive states
// per lane, state k in slot k mod 64K):
//   crfp_fwd_kernel<K>           crf_lattice.hip's forward sum, step for step (its logp is crf_score's bit for bit).
//                                    Every row's cells go to the workspace by SLOT, scaled by 2^-kAlphaDown (exact), and the
//                                    row's exponent next to them: T * 64K floats, then T exponent words, per labelling.
//                                    K = 1, 2, 4, 8 as crf_lattice.hip, and 3 for the backward pass's deeper tiers.
//   crfp_back_kernel<K, MM, NB>  m <= MM, nb <= NB.  Step u = T_r - 1 .. 0 consumes the posteriors of row u: with the
//                                    values of row u in the registers ("old"; row T_r - 1: 1 in state L and in its chains),
//                                      acc[k][c]    += alpha_{u-1}[k] * P(u,k,c) * V_{k+1}[1][c]_u
//                                      beta_{u-1}[s] = P(u,s,0) beta_u[s] + P(u,s,y_s) beta_u[s+1]
//                                      V_s[j][c]_{u-1} = P'(u,s,0) V_s[j][c]_u + P'(u,s,y_s) V_{s+1}[j+1][c]_u
//                                    with P' read from row sigma_s + (c - y_{s-j}) nb^(j-1) and V_{s+1}[m+1][c] = beta[s+1]:
//                                    the chain slots j = m + 1 .. MM hold a copy of beta[s], so no step asks where m ends.
//                                    Every old value a state reads is its own or the next slot's (one wave rotation), and the
//                                    slots are updated in ascending order, so the update is in place.  acc[k][c] summed over
//                                    the rows is P(y[k:=c] | x) up to a scale all c share; when state k leaves the window (or
//                                    after row 0) the lane divides by the sum over c and stores post[k][.].
// A value enters a cell only where both its source and the cell are live in their rows' windows (crf_window): the windows
// are in label counts, so every variant walks the cells y walks.
//
// Scales.  beta and every V share one integer exponent per row.  The step is two passes over the row's posteriors: the
// first takes only exponents -- the largest frexp(old) + frexp(posterior) over every product of the row, E, reduced as an
// integer (wave_imax); a product is below 2^E and the largest at least 2^(E-2), so with every product rescaled by the exact
// power of two 2^(kTargetB - E) the row's largest cell lands in [2^(kTargetB-2), 2^(kTargetB+1)) -- the second pass forms
// the products (one f32 rounding each) and their sum (one).  alpha has the forward pass's exponents.  A term of acc has the
// wave-uniform exponent X_u = Ea(u-1) + Eb(u) and its posterior's own, e.  The accumulators of a slot share one integer
// exponent Xa above Xp = floor(log2 P(y | x)), which the forward launch left in logp: a term is scaled by the exact power of
// two 2^(X_u + e - Xp - Xa).  Xa starts at 0 -- the called label's sum is about 1 at every position -- and rises, the slot's
// accumulators rescaled with it, whenever a term would reach 2^kAccTop: a variant may outweigh y by any factor, and y's own
// share then underflows to the 0 it is.  (The row maxima are no anchor: in a wide window alpha's largest cell and beta's lie
// at opposite ends, and their product exceeds every term an alignment passes through by as many bits as f32 has exponent.)
// Every term is non-negative; one rounding per product and per sum; no fused multiply-add (-ffp-contract=off).
#include <math.h>

#include <algorithm>

#include "crf_lattice.h"

namespace fcd {
namespace {

constexpr int kAlphaDown = 60;  // stored alpha: row maximum in [2^59, 2^60)
constexpr int kTargetB = 59;    // beta, V: row maximum in [2^57, 2^60)
constexpr int kAccTop = 64;     // a term enters its accumulator below 2^64: 2^46 rows sum below 2^110

struct CrfPostParams {
    CrfParams c;  // (c.logp is never null: the driver lends scratch when the caller wants none)
    float *post;  // [labellings of this launch * stride * (N - 1)]
    float *alpha;  // the stored forward rows, alpha_words per labelling of this launch
    int64_t alpha_words;
    int m;  // S == nb^m; S == 1: 1 (the one label sigma is made of, before the table cuts it)
};

// ---- pass 1: crf_lattice.hip's forward sum, storing what it computes ----
template <int K>
__global__ __launch_bounds__(64) void crfp_fwd_kernel(CrfPostParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int C = 64 * K;
    const CrfParams &p = q.c;
    const CrfLds lds = crf_carve(smem);
    CrfRow rw;
    if (!crf_prologue(p, lds, &rw)) return;
    const int lane = threadIdx.x;
    float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    int *ae = reinterpret_cast<int *>(am + (int64_t)p.in.T * C);
    float a[K];
#pragma unroll
    for (int r = 0; r < K; ++r) a[r] = 0.0f;
    if (lane == 0) a[0] = 1.0f;  // "row -1": state 0, the one live state
    int64_t eacc = 0;
    int lo = 0, hi = 0;
    for (int t0 = 0; t0 < rw.Tr; t0 += p.rows_per_tile) {
        const int rc = min(p.rows_per_tile, rw.Tr - t0);
        crf_fill_tile(p, lds, rw, t0, rc);
        CrfStep<K> in = crf_load_step<K>(p, lds, rw, t0, 0, lo, hi);
        for (int i = 0; i < rc; ++i) {
            CrfStep<K> nx = in;
            if (i + 1 < rc) nx = crf_load_step<K>(p, lds, rw, t0 + i + 1, i + 1, in.lo, in.hi);
            lo = in.lo;
            hi = in.hi;
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
            float *row = am + (int64_t)(t0 + i) * C + lane * K;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const float c0 = ldexpf(s[r], min(max(in.pe0[r] + sh, -512), 512));
                const float c1 = ldexpf(ua[r], min(max(ea[r] + sh, -512), 512));
                a[r] = c0 + c1;
                row[r] = ldexpf(a[r], -kAlphaDown);  // (a slot outside the row's window holds 0)
            }
            if (lane == 0) ae[t0 + i] = (int)(eacc + kAlphaDown);
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
    __syncthreads();
    const float m = __int_as_float(lds.misc[18]);
    if (lane == 0) p.logp[blockIdx.x] = log((double)m) + (double)eacc * 0.693147180559945309417232121458;
}

// ---- pass 2 ----
// NaN for the labels the row holds: a labelling without a positive finite P(y | x), and what the walk starts from
__device__ __forceinline__ void crf_no_posterior(const CrfPostParams &q) {
    const int64_t row = blockIdx.x, nc = q.c.in.N - 1;
    const int64_t n = min((int64_t)q.c.y.len[row], q.c.y.stride) * nc;
    for (int64_t e = threadIdx.x; e < n; e += 64) q.post[row * q.c.y.stride * nc + e] = NAN;
}

template <int NB>
__device__ __forceinline__ void crf_store_post(float *post, int k, int nb, const float (&acc)[NB]) {
    float sum = acc[0];
#pragma unroll
    for (int c = 1; c < NB; ++c)
        if (c < nb) sum += acc[c];
#pragma unroll
    for (int c = 0; c < NB; ++c)
        if (c < nb) post[(int64_t)k * nb + c] = acc[c] / sum;  // (0 / 0 and x / NaN: NaN, as the contract wants it)
}

__device__ __forceinline__ float crf_from_next_lane(float x) {  // wave_rol:1 -- lane l receives lane (l + 1) & 63
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x134, 0xf, 0xf, false));
}

// crf_window with k(t) handed in (the row before the tile has no krow entry)
__device__ __forceinline__ void crf_window_k(const CrfParams &p, const CrfRow &rw, int t, int k, int *lo, int *hi) {
    int l = 0, h = rw.L;
    if (p.band > 0) {
        l = max(0, k - p.band);
        h = min(h, k + p.band);
    }
    *hi = min(h, t + 1);
    *lo = max(l, rw.L - (rw.Tr - 1 - t));
}

// the posterior p[u][sig][col] of the tile's row i (staged shapes: from LDS; the others: from global memory)
__device__ __forceinline__ float crf_post_value(const CrfParams &p, const CrfLds &lds, const CrfRow &rw, int u, int i, int sig,
                                                int col) {
    if (p.staged) return lds.tile[(i * p.in.S + sig) * p.in.N + col];
    return load_post(rw.post, (int64_t)u * p.in.stride_t + (int64_t)sig * p.in.stride_s + (int64_t)col * p.in.stride_n, p.in.dtype);
}

// frexp(old) + frexp(v) of a product that takes part in the row maximum; kNoExp for every other one
__device__ __forceinline__ int crf_term_exp(float old, float v) {
    int eo, ev;
    (void)frexpf(old, &eo);
    (void)frexpf(v, &ev);
    return (old > 0.0f && old - old == 0.0f && v > 0.0f && v - v == 0.0f) ? eo + ev : kNoExp;
}

// old * v scaled by 2^sh: the mantissa product (one rounding), then the exact power of two
__device__ __forceinline__ float crf_term(float old, float v, int sh) {
    float m;
    int e;
    crf_split(v, &m, &e);
    return ldexpf(old * m, min(max(e + sh, -512), 512));
}

template <int K, int MM, int NB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void crfp_back_kernel(CrfPostParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int C = 64 * K;
    // the widest instantiations: a slot's posteriors are read when its turn comes, not all slots' ahead of the first --
    // what the scheduler would otherwise hoist does not fit the 256 registers
    constexpr bool kSlotFence = K * MM * NB > 48;
    const CrfParams &p = q.c;
    const CrfLds lds = crf_carve(smem);
    CrfRow rw;
    if (!crf_prologue(p, lds, &rw)) {  // (the forward launch wrote this row's logp already; the same value again)
        crf_no_posterior(q);
        return;
    }
    const double lp = p.logp[blockIdx.x];
    if (lp - lp != 0.0) {  // P = 0, or a NaN on the way
        crf_no_posterior(q);
        return;
    }
    if (rw.L == 0) return;
    crf_no_posterior(q);  // a position no row's window holds keeps this
    __syncthreads();      // the fill is in place before another lane's store writes over it
    const int lane = threadIdx.x, nb = p.in.N - 1, L = rw.L, m = q.m;
    const float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    const int *ae = reinterpret_cast<const int *>(am + (int64_t)p.in.T * C);
    float *post = q.post + (int64_t)blockIdx.x * p.y.stride * nb;
    float b[K], V[K][MM][NB], acc[K][NB];
    int xa[K];  // the exponent of a slot's accumulators, above Xp
#pragma unroll
    for (int r = 0; r < K; ++r) {
        b[r] = 0.0f;
        xa[r] = 0;
#pragma unroll
        for (int c = 0; c < NB; ++c) acc[r][c] = 0.0f;
#pragma unroll
        for (int j = 0; j < MM; ++j)
#pragma unroll
            for (int c = 0; c < NB; ++c) V[r][j][c] = 0.0f;
    }
    int64_t eb = 0;
    const int64_t xp = (int64_t)floor(lp * 1.44269504088896340735992468100189214);  // floor(log2 P(y | x))
    bool first = true;
    int lo_p = 0, hi_p = 0;
    for (int t0 = (rw.Tr - 1) / p.rows_per_tile * p.rows_per_tile; t0 >= 0; t0 -= p.rows_per_tile) {
        const int rc = min(p.rows_per_tile, rw.Tr - t0);
        crf_fill_tile(p, lds, rw, t0, rc);
        if (p.band > 0 && t0 > 0) {  // k(t0 - 1): the window of the row before the tile
            if (lane == 0) {
                int a0 = 0, a1 = L;
                while (a0 < a1) {
                    const int mid = (a0 + a1) >> 1;
                    if (rw.path[mid] <= (uint32_t)(t0 - 1)) a0 = mid + 1;
                    else a1 = mid;
                }
                lds.misc[kKrowBefore] = a0;
            }
            __syncthreads();
        }
        for (int i = rc - 1; i >= 0; --i) {
            const int u = t0 + i;
            int lo_u, hi_u;  // the window of row u: the states whose "old" values the registers hold
            crf_window(p, lds, rw, u, i, &lo_u, &hi_u);
            lo_p = hi_p = 0;  // the window of row u - 1 ("row -1": state 0): the states that get a value in this step
            int64_t x_u = 0;
            if (u > 0) {
                crf_window_k(p, rw, u - 1, p.band > 0 ? (i > 0 ? lds.krow[i - 1] : lds.misc[kKrowBefore]) : 0, &lo_p, &hi_p);
                x_u = ae[u - 1];
            }
            const float *arow = am + (int64_t)max(u - 1, 0) * C + lane * K;  // alpha_{u-1}, by slot
            if (first) {  // row T_r - 1: state L and the chains that end in it
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const bool last = slot_state<K>(lane, r, lo_u) == L;
                    b[r] = last ? 1.0f : 0.0f;
#pragma unroll
                    for (int j = 0; j < MM; ++j)
#pragma unroll
                        for (int c = 0; c < NB; ++c) V[r][j][c] = (last && (j >= m || j < L)) ? 1.0f : 0.0f;
                }
                first = false;
            } else {  // the states that were live at row u and are not at row u - 1: their positions are complete
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int s = slot_state<K>(lane, r, lo_u);
                    if (s > hi_p) {  // (b and V stay: this step still reads them as the values of row u)
                        if (s <= hi_u && s < L) crf_store_post<NB>(post, s, nb, acc[r]);
#pragma unroll
                        for (int c = 0; c < NB; ++c) acc[r][c] = 0.0f;
                        xa[r] = 0;
                    }
                }
            }
            // ---- the exponents: the largest frexp(old) + frexp(posterior) over the products of this step ----
            int emax = kNoExp;
            {
                // (the next lane's first slot, as it stands at row u; rotated once per pass, so that no copy lives across both)
                const float nb0 = crf_from_next_lane(b[0]);
                float nV[MM][NB];
#pragma unroll
                for (int j = 0; j < MM; ++j)
#pragma unroll
                    for (int c = 0; c < NB; ++c) nV[j][c] = crf_from_next_lane(V[0][j][c]);
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    int ln = lane;
                    if (kSlotFence) {  // (nothing of this slot -- its addresses least of all -- is worked out ahead of its turn)
                        __asm__ volatile("" ::: "memory");
                        FCD_OPAQUE_V(ln);
                    }
                    const int s = slot_state<K>(ln, r, lo_p);
                    const bool live = s <= hi_p;
                    const bool own = live && s >= lo_u && s <= hi_u;          // state s holds a value at row u
                    const bool nxt = live && s + 1 >= lo_u && s + 1 <= hi_u;  // state s + 1 does
                    const uint32_t info = lds.info[live ? s : 0];  // (a dead slot reads a valid address and is masked below)
                    const uint32_t sg = info & 0xFFFFFFu;
                    const int y = (int)(info >> 24);
                    const bool table = sg != kNoState;
                    const int sig = table ? (int)sg : 0;
                    const float bo = own ? b[r] : 0.0f;
                    const float bn = nxt ? (r + 1 < K ? b[r + 1 < K ? r + 1 : 0] : nb0) : 0.0f;
                    if (own && table) emax = max(emax, crf_term_exp(bo, crf_post_value(p, lds, rw, u, i, sig, 0)));
                    if (nxt && table) emax = max(emax, crf_term_exp(bn, crf_post_value(p, lds, rw, u, i, sig, y)));
                    int pw = 1;
#pragma unroll
                    for (int j = 0; j < MM; ++j) {
                        if (kSlotFence) __asm__ volatile("" ::: "memory");
                        const bool chain = live && j < m && j < s;  // the variant substituted position s - 1 - j
                        const int yk = (int)(lds.info[chain ? s - 1 - j : 0] >> 24);
#pragma unroll
                        for (int c = 0; c < NB; ++c) {
                            bool ok = chain && c < nb;
                            const int sv = ok ? (p.in.S == 1 ? yk - 1 : sig) + (c + 1 - yk) * pw : 0;  // (S == 1: below, then c)
                            ok = ok && sv < p.in.S;
                            const float vo = own ? V[r][j][c] : 0.0f;
                            const float up = j + 1 < MM ? (r + 1 < K ? V[r + 1 < K ? r + 1 : 0][j + 1 < MM ? j + 1 : 0][c]
                                                                     : nV[j + 1 < MM ? j + 1 : 0][c])
                                                        : (r + 1 < K ? b[r + 1 < K ? r + 1 : 0] : nb0);
                            const float vn = nxt ? up : 0.0f;
                            if (ok && own) emax = max(emax, crf_term_exp(vo, crf_post_value(p, lds, rw, u, i, sv, 0)));
                            if (ok && nxt) emax = max(emax, crf_term_exp(vn, crf_post_value(p, lds, rw, u, i, sv, y)));
                        }
                        pw *= nb;
                    }
                }
            }
            emax = wave_imax(emax);
            const int sh = emax == kNoExp ? 0 : kTargetB - emax;
            x_u += eb;  // the exponent of this step's terms: alpha of row u - 1 times a value of row u
            const int dt = (int)min(max(x_u - xp, (int64_t)-(1 << 20)), (int64_t)(1 << 20));
            eb -= sh;
            // (the posteriors are read again rather than kept: two values per product would not fit the registers)
            __asm__ volatile("" ::: "memory");
            // ---- the terms of acc, and the values of row u - 1, in place: slot r reads slots r and r + 1 only ----
            // the next lane's first slot, as it stands at row u
            const float nb0 = crf_from_next_lane(b[0]);
            float nV[MM][NB];
#pragma unroll
            for (int j = 0; j < MM; ++j)
#pragma unroll
                for (int c = 0; c < NB; ++c) nV[j][c] = crf_from_next_lane(V[0][j][c]);
#pragma unroll
            for (int r = 0; r < K; ++r) {
                int ln = lane;
                if (kSlotFence) {  // (nothing of this slot -- its addresses least of all -- is worked out ahead of its turn)
                    __asm__ volatile("" ::: "memory");
                    FCD_OPAQUE_V(ln);
                }
                const int s = slot_state<K>(ln, r, lo_p);
                const bool live = s <= hi_p;
                const bool own = live && s >= lo_u && s <= hi_u;
                const bool nxt = live && s + 1 >= lo_u && s + 1 <= hi_u;
                const uint32_t info = lds.info[live ? s : 0];
                const uint32_t sg = info & 0xFFFFFFu;
                const int y = (int)(info >> 24);
                const bool table = sg != kNoState;
                const int sig = table ? (int)sg : 0;
                const float bo = own ? b[r] : 0.0f;
                const float bn = nxt ? (r + 1 < K ? b[r + 1 < K ? r + 1 : 0] : nb0) : 0.0f;
                const float av = u > 0 ? (live ? arow[r] : 0.0f) : 1.0f;  // ("row -1": state 0, the one live state, holds 1)
                const float b0 = (own && table) ? crf_term(bo, crf_post_value(p, lds, rw, u, i, sig, 0), sh) : 0.0f;
                const float b1 = (nxt && table) ? crf_term(bn, crf_post_value(p, lds, rw, u, i, sig, y), sh) : 0.0f;
                const float b_new = b0 + b1;  // (b[r] itself is written last: the terms below read it as it stands at row u)
                // what position s gains at this row: state s emits c, the variant's state s + 1 takes over
                // (the slot's exponent rises, its accumulators rescaled with it, before a term of 2^kAccTop or more enters: a
                // variant that outweighs y by more than f32 holds takes the accumulators down with it instead of overflowing)
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    if (c < nb && nxt) {
                        const float vn = r + 1 < K ? V[r + 1 < K ? r + 1 : 0][0][c] : nV[0][c];
                        float pm;
                        int pe;
                        crf_split(table ? crf_post_value(p, lds, rw, u, i, sig, c + 1) : 0.0f, &pm, &pe);
                        const float term = (av * pm) * vn;
                        const int e = finite_exp(term);
                        if (e != kNoExp && e + dt + pe - kAccTop > xa[r]) {
                            const int up = e + dt + pe - kAccTop;
                            const int down = max(xa[r] - up, -512);
#pragma unroll
                            for (int c2 = 0; c2 < NB; ++c2) acc[r][c2] = ldexpf(acc[r][c2], down);
                            xa[r] = up;
                        }
                        acc[r][c] += ldexpf(term, min(max(dt + pe - xa[r], -512), 512));
                    }
                }
                int pw = 1;
#pragma unroll
                for (int j = 0; j < MM; ++j) {
                    if (kSlotFence) __asm__ volatile("" ::: "memory");
                    const bool chain = live && j < m && j < s;
                    const int yk = (int)(lds.info[chain ? s - 1 - j : 0] >> 24);
#pragma unroll
                    for (int c = 0; c < NB; ++c) {
                        bool ok = chain && c < nb;
                        const int sv = ok ? (p.in.S == 1 ? yk - 1 : sig) + (c + 1 - yk) * pw : 0;  // (S == 1: below, then c)
                        ok = ok && sv < p.in.S;
                        const float vo = own ? V[r][j][c] : 0.0f;
                        const float up = j + 1 < MM ? (r + 1 < K ? V[r + 1 < K ? r + 1 : 0][j + 1 < MM ? j + 1 : 0][c]
                                                                 : nV[j + 1 < MM ? j + 1 : 0][c])
                                                    : (r + 1 < K ? b[r + 1 < K ? r + 1 : 0] : nb0);
                        const float vn = nxt ? up : 0.0f;
                        const float c0 = (ok && own) ? crf_term(vo, crf_post_value(p, lds, rw, u, i, sv, 0), sh) : 0.0f;
                        const float c1 = (ok && nxt) ? crf_term(vn, crf_post_value(p, lds, rw, u, i, sv, y), sh) : 0.0f;
                        V[r][j][c] = j < m ? c0 + c1 : b_new;
                    }
                    pw *= nb;
                }
                b[r] = b_new;
            }
        }
    }
    // the positions whose state is live at "row -1": state 0
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = slot_state<K>(lane, r, lo_p);
        if (s <= hi_p && s < L) crf_store_post<NB>(post, s, nb, acc[r]);
    }
}

// the chain tier that holds (m, nb), the narrowest alphabet first: 2 = {4, 2}, 1 = {2, 4} (up to 8 states per lane),
// 0 = {1, 8} (up to 4), 3 = {3, 8}, 4 = {6, 4} (m nb <= 24: up to 3 states per lane); -1: none
int crf_post_tier(int m, int nb) {
    if (m <= 4 && nb <= 2) return 2;
    if (m <= 2 && nb <= 4) return 1;
    if (m <= 1 && nb <= 8) return 0;
    if (m <= 3 && nb <= 8) return 3;
    if (m <= 6 && nb <= 4) return 4;
    return -1;
}

// S == nb^m: m (S == 1: 1, see the head of the file); -1 where S is no power of nb
int crf_post_chain(int64_t S, int64_t nb) {
    if (S == 1) return 1;
    if (nb < 2) return -1;
    int m = 0;
    int64_t v = 1;
    while (v < S) {
        v *= nb;
        ++m;
    }
    return v == S ? m : -1;
}

template <int K, int MM, int NB>
void launch_pair(const CrfPostParams &q, dim3 grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL(crfp_fwd_kernel<K>, grid, dim3(64), lds, stream, q);
    hipLaunchKernelGGL((crfp_back_kernel<K, MM, NB>), grid, dim3(64), lds, stream, q);
}

// KMAX: the most states per lane the tier is instantiated at -- 8: 1, 2, 4, 8; 4: 1, 2, 4; 3: 1, 2, 3 (what fits 256 VGPRs
// without scratch: eight states of eight labels do not)
template <int MM, int NB, int KMAX>
hipError_t launch_tier(const CrfPostParams &q, int k, dim3 grid, size_t lds, hipStream_t stream) {
    if (k == 1) launch_pair<1, MM, NB>(q, grid, lds, stream);
    else if (k == 2) launch_pair<2, MM, NB>(q, grid, lds, stream);
    else if (KMAX == 3 && k == 3) launch_pair<KMAX == 3 ? 3 : 1, MM, NB>(q, grid, lds, stream);
    else if (KMAX >= 4 && k == 4) launch_pair<KMAX >= 4 ? 4 : 1, MM, NB>(q, grid, lds, stream);
    else if (KMAX >= 8 && k == 8) launch_pair<KMAX >= 8 ? 8 : 1, MM, NB>(q, grid, lds, stream);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// the widest window of a tier: 64 states per state a lane holds
int64_t crf_post_max_states(int tier) { return tier == 0 ? 256 : (tier <= 2 ? 512 : 192); }

// states per lane of both launches: crf_lattice.hip's 1, 2, 4, 8 in the first three tiers, else 1, 2, 3
int crf_post_states_per_lane(int tier, int64_t T, int64_t stride, int64_t band) {
    if (tier <= 2) return crf_states_per_lane(T, stride, band);
    const int64_t states = crf_lattice_window_states(T, stride, band);
    return states <= 64 ? 1 : (states <= 128 ? 2 : 3);
}

}  // namespace

// 0 = the kernels hold the call; 1 = the window exceeds the register-resident states of the chain's tier (*max_states),
// 2 = more than 8 labels, 4 = S is no power of N - 1, 5 = a chain beyond the tiers (m > 6, or m nb > 24)
int crf_posterior_unsupported(int64_t T, int64_t S, int64_t N, int64_t stride, int64_t band, int64_t *max_states) {
    if (N - 1 > 8) return 2;
    const int m = crf_post_chain(S, N - 1);
    if (m < 0) return 4;
    const int tier = crf_post_tier(m, (int)(N - 1));
    if (tier < 0) return 5;
    *max_states = crf_post_max_states(tier);
    return crf_lattice_window_states(T, stride, band) > *max_states ? 1 : 0;
}

// stored forward rows of one labelling (every one of a call has T rows' worth): T * 64K cells, then T exponent words
size_t crf_posterior_row_bytes(int64_t T, int64_t S, int64_t N, int64_t stride, int64_t band) {
    const size_t k = (size_t)crf_post_states_per_lane(crf_post_tier(crf_post_chain(S, N - 1), (int)(N - 1)), T, stride, band);
    return ((size_t)std::max<int64_t>(T, 1) * (64 * k + 1) * 4 + 255) & ~(size_t)255;
}

hipError_t launch_crf_posterior(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                                int64_t band, float *post, double *logp, unsigned char *alpha, hipStream_t stream) {
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    CrfPostParams q;
    q.c = crf_params(in, y, init, n_init, init_stride, band);
    q.c.logp = logp;
    q.post = post;
    q.alpha = reinterpret_cast<float *>(alpha);
    q.alpha_words = (int64_t)(crf_posterior_row_bytes(in.T, in.S, in.N, y.stride, band) / 4);
    q.m = crf_post_chain(in.S, in.N - 1);
    const dim3 grid((unsigned)rows);
    const size_t lds = crf_lds_bytes(q.c.lab_cap);
    const int tier = crf_post_tier(q.m, in.N - 1), k = crf_post_states_per_lane(tier, in.T, y.stride, band);
    switch (tier) {
    case 0: return launch_tier<1, 8, 4>(q, k, grid, lds, stream);
    case 1: return launch_tier<2, 4, 8>(q, k, grid, lds, stream);
    case 2: return launch_tier<4, 2, 8>(q, k, grid, lds, stream);
    case 3: return launch_tier<3, 8, 3>(q, k, grid, lds, stream);
    case 4: return launch_tier<6, 4, 3>(q, k, grid, lds, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace fcd
