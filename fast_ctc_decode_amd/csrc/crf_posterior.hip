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
// fcd_crf_edits_* (the deletion and insertion likelihoods of the same labellings) is the same forward launch -- with the cone
// kept one state wider below, CrfParams::cone_lo -- and two more walks compiled into crfp_back_kernel, selected by the
// wave-uniform q.walk: crfp_back_walk<K, MM, NB, WALK> below says where they differ from the substitution walk.  Their
// accumulators become float32 log-ratios against ln P(y | x) (log_ratio of ctc_lattice.h), as ctc_posterior.hip's edit walk forms them.
//
// fcd_crf_occupancy_* (the edge occupancies of the labelling's own lattice) is the forward launch at crf_lattice.hip's K and a
// fourth walk, crfp_occ_walk below, compiled into crfp_back_kernel<K, 2, 4> only: beta alone, no chains, any S.
//
// fcd_set_crf_lattice_wide (windows beyond 512 states, for the forward sum and the occupancies): the window lives in LDS, J =
// 9 .. 64 states per lane, and two more loop bodies walk it -- crf_forward_walk_lds of crf_lattice.h inside crfp_fwd_kernel<8>
// (alpha null: the sum alone, fcd_crf_score_*) and crfp_occ_walk_lds below inside crfp_back_kernel<8, 2, 4> -- selected by the
// wave-uniform q.wide_j.  No instantiation of their own; the other instantiations do not compile them.
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

// (kAlphaDown, the scale of the stored alpha: ctc_lattice.h)
constexpr int kTargetB = 59;    // beta, V: row maximum in [2^57, 2^60)
constexpr int kAccTop = 64;     // a term enters its accumulator below 2^64: 2^46 rows sum below 2^110

struct CrfPostParams {
    CrfParams c;  // (c.logp is never null: the driver lends scratch when the caller wants none)
    float *post;  // [labellings of this launch * stride * (N - 1)]
    float *alpha;  // the stored forward rows, alpha_words per labelling of this launch
    int64_t alpha_words;
    int m;  // S == nb^m; S == 1: 1 (the one label sigma is made of, before the table cuts it)
    int walk;  // what the backward launch walks (wave-uniform): kWalkSub, kWalkIns, kWalkDel
    float *del, *ins;  // [.. * stride], [.. * (stride + 1) * (N - 1)]                          (fcd_crf_edits_*)
    // (fcd_crf_occupancy_*) a (T, S, N) block per labelling of this launch, at row * occ_stride_row + t * occ_stride_t
    float *occ;
    int64_t occ_stride_row, occ_stride_t;
    float occ_scale;
    int occ_clear;  // accumulate = 0: rows t < T_r of a labelling with a value are zeroed before the walk adds to them
    // (fcd_set_crf_lattice_wide) states per lane of a window that lives in LDS, 9 .. 64; 0: the register-resident walks.
    // Read by crfp_fwd_kernel<8> and crfp_back_kernel<8, 2, 4> only.  With it a null alpha is "sum only": the wide crf_score
    int wide_j;
};
constexpr int kWalkSub = 0, kWalkIns = 1, kWalkDel = 2, kWalkOcc = 3;

// ---- the LDS-resident walks share nothing with the register walks of their kernels ----
// Inlined next to a register walk, a wide walk that reads the same parameter block keeps the block's scalar registers live
// across both, and the allocator then spills the register walk's own (4.2 % on the gathered
// occupancy call).  So a wide walk is entered by one wave-uniform branch ahead of everything the register walk computes, runs
// the prologue for itself, and reads the parameter block AGAIN, through the kernarg segment's pointer -- the block is the
// kernels' one argument -- with scalar loads of its own: no value is live in both paths.  (The emulator has no kernarg
// segment and no registers: there it is the block the kernel was handed.)
__device__ __forceinline__ const CrfPostParams &crfp_params_again(const CrfPostParams &q) {
#ifdef FCD_HIPEMU
    return q;
#else
    return *(const CrfPostParams *)__builtin_amdgcn_kernarg_segment_ptr();
#endif
}

// ---- pass 1: crf_lattice.hip's forward sum, storing what it computes (crf_forward_walk of crf_lattice.h) ----
template <int K>
__global__ __launch_bounds__(64) void crfp_fwd_kernel(CrfPostParams q0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int C = 64 * K;
    if constexpr (K == 8) {  // (the one instantiation that hosts the LDS-resident window: wave-uniform)
        if (q0.wide_j > 0) {
            const CrfPostParams &q = crfp_params_again(q0);
            const CrfParams &p = q.c;
            const CrfLds lds = crf_carve(smem);
            CrfRow rw;
            if (!crf_prologue(p, lds, &rw)) return;
            const int J = q.wide_j;
            const CrfWideLds w = crf_wide_carve(lds.info + p.lab_cap, J);
            int64_t eacc;
            float *am = q.alpha ? q.alpha + (int64_t)blockIdx.x * q.alpha_words : nullptr;  // (null: the sum alone)
            int *ae = am ? reinterpret_cast<int *>(am + (int64_t)p.in.T * 64 * J) : nullptr;
            const float m = crf_forward_walk_lds<kCrfStore>(p, lds, rw, w, J, am, ae, &eacc);
            if (threadIdx.x == 0) p.logp[blockIdx.x] = ln_p((double)m, eacc);
            return;
        }
    }
    const CrfPostParams &q = q0;
    const CrfParams &p = q.c;
    const CrfLds lds = crf_carve(smem);
    CrfRow rw;
    if (!crf_prologue(p, lds, &rw)) return;
    float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    int64_t eacc;
    const float m = crf_forward_walk<kCrfStore, K>(p, lds, rw, nullptr, am, reinterpret_cast<int *>(am + (int64_t)p.in.T * C), &eacc);
    if (threadIdx.x == 0) p.logp[blockIdx.x] = ln_p((double)m, eacc);
}

// ---- pass 2 ----
// NaN for the labels the row holds: a labelling without a positive finite P(y | x), and what the walk starts from
__device__ __forceinline__ void crf_no_posterior(const CrfPostParams &q) {
    const int64_t row = blockIdx.x, nc = q.c.in.N - 1;
    const int64_t n = min((int64_t)q.c.y.len[row], q.c.y.stride) * nc;
    for (int64_t e = threadIdx.x; e < n; e += 64) q.post[row * q.c.y.stride * nc + e] = NAN;
}

// (store_post, from_next_lane, log_ratio: ctc_lattice.h)

// crf_window with k(t) handed in (the row before the tile has no krow entry)
__device__ __forceinline__ void crf_window_k(const CrfParams &p, const CrfRow &rw, int t, int k, int *lo, int *hi) {
    crf_window_of(p, rw, t, k, p.cone_lo, p.cone_hi, lo, hi);
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

// ---- what the walks of fcd_crf_edits_* need next to the substitution walk's helpers ----
// every entry of the walk's output the row owns -- k < min(len, stride), g <= min(len, stride) -- set to v
template <int WALK>
__device__ __forceinline__ void crf_fill_edits(const CrfPostParams &q, float v) {
    const int64_t row = blockIdx.x, nc = q.c.in.N - 1;
    const int64_t n = min((int64_t)q.c.y.len[row], q.c.y.stride);
    if constexpr (WALK == kWalkDel) {
        for (int64_t e = threadIdx.x; e < n; e += 64) q.del[row * q.c.y.stride + e] = v;
    } else {
        for (int64_t e = threadIdx.x; e < (n + 1) * nc; e += 64) q.ins[row * (q.c.y.stride + 1) * nc + e] = v;
    }
}

// a complete position leaves the registers: the substitution posteriors of label s; the insertions into gap s; the
// deletion of label s - 1 (its accumulator rides in the slot of the state after it)
template <int WALK, int NB, int CN>
__device__ __forceinline__ void crf_store_position(const CrfPostParams &q, int s, int L, int nb, const float (&acc)[CN], int64_t e,
                                                   double lp) {
    const int64_t row = blockIdx.x;
    if constexpr (WALK == kWalkSub) {
        if (s < L) store_post<NB>(q.post + row * q.c.y.stride * nb, s, nb, acc);
    } else if constexpr (WALK == kWalkIns) {
        float *ins = q.ins + (row * (q.c.y.stride + 1) + s) * nb;
#pragma unroll
        for (int c = 0; c < CN; ++c)
            if (c < nb) ins[c] = log_ratio(acc[c], e, lp);
    } else {
        if (s >= 1 && s < L) q.del[row * q.c.y.stride + s - 1] = log_ratio(acc[0], e, lp);
    }
}

// chain slot j of state s is in use: the variant substituted position s - 1 - j; inserted into gap s - j; deleted label
// s - 2 - j (m: the labels of the model state)
template <int WALK>
__device__ __forceinline__ bool crf_chain_live(bool live, int j, int m, int s) {
    if constexpr (WALK == kWalkSub) return live && j < m && j < s;
    else if constexpr (WALK == kWalkIns) return live && j < m && j <= s;
    else return live && j < m - 1 && j + 2 <= s;
}

// what the chain's posterior row depends on besides sigma_s: the label the variant replaced (substitution); the model
// state the edit left from, sigma_{s-j} (insertion), sigma_{s-2-j} (deletion)
template <int WALK>
__device__ __forceinline__ int crf_chain_word(const CrfLds &lds, bool chain, int s, int j) {
    const uint32_t w = lds.info[chain ? s - (WALK == kWalkSub ? 1 : (WALK == kWalkIns ? 0 : 2)) - j : 0];
    return WALK == kWalkSub ? (int)(w >> 24) : (int)(w & 0xFFFFFFu);
}

// the part of an edit's posterior row that no label c changes (pw = nb^j): the digits of sigma_from that are still inside the
// history, moved up past the edit, and the labels of y since -- insertion: j of them, below the inserted one; deletion: j + 1
template <int WALK>
__device__ __forceinline__ int crf_edit_row_base(const CrfParams &p, bool chain, int from, int sig, int pw, int nb) {
    if (!chain || p.in.S == 1) return 0;  // (S == 1, insertion: the row is the label alone)
    const int pwn = pw * nb;              // (chain: j < m, so nb^(j+1) divides S)
    return (from % (p.in.S / pwn)) * pwn + (WALK == kWalkIns ? sig % pw : sig % pwn);
}

// One backward walk.  WALK = kWalkSub is the walk the head of the file describes.  The other two are fcd_crf_edits_*'s and
// differ from it where `if constexpr` says so:
//   kWalkIns  V[r][j][c] = U_s[j][c], the backward value state s has in the variant that inserted c into gap s - j, read
//             from row (sigma_{s-j} nb^(j+1)) mod S + (c - 1) nb^j + sigma_s mod nb^j; U_{s+1}[m][c] = beta[s+1].  Gap g gains
//             alpha_{u-1}[g] * P(u,g,c) * U_g[0][c]_u: its OWN slot's value.  Chains 0 <= s - j, positions 0 .. L; L = 0 walks.
//   kWalkDel  V[r][j][0] = W_s[j], the value state s has in the variant that deleted label s - 2 - j, read from row
//             (sigma_{s-2-j} nb^(j+1)) mod S + sigma_s mod nb^(j+1); W_{s+1}[m-1] = beta[s+1]: MM - 1 chain slots, one
//             accumulator.  D[k] rides in the slot of state k + 1 and gains alpha_{u-1}[k] * P(u,k,y_{k+1}) * X_u[k+2], X = W[0]
//             (m = 1: beta): alpha from the state below (the forward launch kept the cone one state wider below for it: the
//             forward window is computed here next to the walk's own, which is one state wider ABOVE -- q.c.cone_hi), X from the
//             slot above.  D[L-1] = alpha_{T_r-1}[L-1] comes off the last forward row.
// An entry no row's window holds keeps what the fill wrote: NaN (substitution), -inf (the edits: probability 0).
template <int K, int MM, int NB, int WALK>
__device__ __forceinline__ void crfp_back_walk(const CrfPostParams &q, unsigned char *smem) {
    constexpr int C = 64 * K;
    constexpr bool kSub = WALK == kWalkSub, kIns = WALK == kWalkIns, kDel = WALK == kWalkDel;
    constexpr int JN = kDel ? MM - 1 : MM;  // chain slots in use
    constexpr int J = JN > 0 ? JN : 1;
    constexpr int CN = kDel ? 1 : NB;       // variants per chain slot, and accumulators per state
    // the widest instantiations: a slot's posteriors are read when its turn comes, not all slots' ahead of the first --
    // what the scheduler would otherwise hoist does not fit the 256 registers
    constexpr bool kSlotFence = K * MM * NB > 48;
    const CrfParams &p = q.c;
    const CrfLds lds = crf_carve(smem);
    CrfRow rw;
    const bool walk = crf_prologue(p, lds, &rw);  // (the forward launch wrote this row's logp already; the same value again)
    if constexpr (kSub) {
        if (!walk) {
            crf_no_posterior(q);
            return;
        }
    }
    const double lp = p.logp[blockIdx.x];
    if (lp - lp != 0.0) {  // P = 0, or a NaN on the way (the edits: or not a labelling)
        if constexpr (kSub) crf_no_posterior(q);
        else crf_fill_edits<WALK>(q, NAN);
        return;
    }
    if constexpr (kSub) {
        if (rw.L == 0) return;
        crf_no_posterior(q);  // a position no row's window holds keeps this
    } else {
        crf_fill_edits<WALK>(q, -INFINITY);  // an edit no row carries has probability 0
        if (!walk) return;                   // (T_r = 0 and L = 0: P(y | x) = 1, and no insertion has an alignment)
        if (kDel && rw.L == 0) return;
    }
    __syncthreads();  // the fill is in place before another lane's store writes over it
    const int lane = threadIdx.x, nb = p.in.N - 1, L = rw.L, m = q.m;
    const float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    const int *ae = reinterpret_cast<const int *>(am + (int64_t)p.in.T * C);
    float b[K], V[K][J][CN], acc[K][CN];
    int xa[K];  // the exponent of a slot's accumulators, above Xp
#pragma unroll
    for (int r = 0; r < K; ++r) {
        b[r] = 0.0f;
        xa[r] = 0;
#pragma unroll
        for (int c = 0; c < CN; ++c) acc[r][c] = 0.0f;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int c = 0; c < CN; ++c) V[r][j][c] = 0.0f;
    }
    int64_t eb = 0;
    const int64_t xp = (int64_t)floor(lp * 1.44269504088896340735992468100189214);  // floor(log2 P(y | x))
    bool first = true;
    int lo_p = 0, hi_p = 0;
    for (int t0 = (rw.Tr - 1) / p.rows_per_tile * p.rows_per_tile; t0 >= 0; t0 -= p.rows_per_tile) {
        const int rc = min(p.rows_per_tile, rw.Tr - t0);
        crf_fill_tile(p, lds, rw, t0, rc);
        stage_krow_before(lds.misc, rw.path, L, p.band, t0);  // the window of the row before the tile
        for (int i = rc - 1; i >= 0; --i) {
            const int u = t0 + i;
            int lo_u, hi_u;  // the window of row u: the states whose "old" values the registers hold
            crf_window(p, lds, rw, u, i, &lo_u, &hi_u);
            lo_p = 0;  // the window of row u - 1 ("row -1": state 0): the states that get a value in this step
            hi_p = kDel ? min(L, 1) : 0;  // (the deletion walk's is a state wider above, at "row -1" too)
            int lo_a = 0, hi_a = 0;  // (deletion) the forward window of row u - 1: the states alpha_{u-1} holds
            int64_t x_u = 0;
            if (u > 0) {
                const int kp = krow_before(lds.krow, lds.misc, p.band, i);
                crf_window_k(p, rw, u - 1, kp, &lo_p, &hi_p);
                if constexpr (kDel) crf_window_of(p, rw, u - 1, kp, 1, 0, &lo_a, &hi_a);
                x_u = ae[u - 1];
            }
            const float *arow = am + (int64_t)max(u - 1, 0) * C + lane * K;  // alpha_{u-1}, by slot
            if (first) {  // row T_r - 1: state L and the chains that end in it
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const bool last = slot_state<K>(lane, r, lo_u) == L;
                    b[r] = last ? 1.0f : 0.0f;
#pragma unroll
                    for (int j = 0; j < JN; ++j)
#pragma unroll
                        for (int c = 0; c < CN; ++c)
                            V[r][j][c] = (last && (kSub ? (j >= m || j < L) : (kIns ? (j >= m || j <= L) : (j >= m - 1 || j + 2 <= L))))
                                             ? 1.0f : 0.0f;
                }
                first = false;
                if constexpr (kDel) {  // the last label's deletion: the shortened labelling's final state, off the last forward row
                    if (lane == 0) {
                        int la, ha;
                        crf_window_of(p, rw, u, p.band > 0 ? lds.krow[i] : 0, 1, 0, &la, &ha);
                        const float v = (L - 1 >= la && L - 1 <= ha) ? am[(int64_t)u * C + (L - 1) % C] : 0.0f;
                        q.del[(int64_t)blockIdx.x * p.y.stride + L - 1] = log_ratio(v, ae[u], lp);
                    }
                }
            } else {  // the states that were live at row u and are not at row u - 1: their positions are complete
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int s = slot_state<K>(lane, r, lo_u);
                    if (s > hi_p) {  // (b and V stay: this step still reads them as the values of row u)
                        if (s <= hi_u) crf_store_position<WALK, NB, CN>(q, s, L, nb, acc[r], xp + xa[r], lp);
#pragma unroll
                        for (int c = 0; c < CN; ++c) acc[r][c] = 0.0f;
                        xa[r] = 0;
                    }
                }
            }
            // ---- the exponents: the largest frexp(old) + frexp(posterior) over the products of this step ----
            int emax = kNoExp;
            {
                // (the next lane's first slot, as it stands at row u; rotated once per pass, so that no copy lives across both)
                const float nb0 = from_next_lane(b[0]);
                float nV[J][CN];
#pragma unroll
                for (int j = 0; j < JN; ++j)
#pragma unroll
                    for (int c = 0; c < CN; ++c) nV[j][c] = from_next_lane(V[0][j][c]);
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
                    for (int j = 0; j < JN; ++j) {
                        if (kSlotFence) __asm__ volatile("" ::: "memory");
                        const bool chain = crf_chain_live<WALK>(live, j, m, s);
                        const int yk = crf_chain_word<WALK>(lds, chain, s, j);
                        const int base = kSub ? 0 : crf_edit_row_base<WALK>(p, chain, yk, sig, pw, nb);
#pragma unroll
                        for (int c = 0; c < CN; ++c) {
                            bool ok = chain && c < nb;
                            int sv = 0;
                            if constexpr (kSub) sv = ok ? (p.in.S == 1 ? yk - 1 : sig) + (c + 1 - yk) * pw : 0;  // (S == 1: below, then c)
                            else sv = ok ? base + (kIns ? c * pw : 0) : 0;
                            ok = ok && sv < p.in.S;
                            const float vo = own ? V[r][j][c] : 0.0f;
                            const float up = j + 1 < JN ? (r + 1 < K ? V[r + 1 < K ? r + 1 : 0][j + 1 < JN ? j + 1 : 0][c]
                                                                     : nV[j + 1 < JN ? j + 1 : 0][c])
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
            const float nb0 = from_next_lane(b[0]);
            float nV[J][CN];
#pragma unroll
            for (int j = 0; j < JN; ++j)
#pragma unroll
                for (int c = 0; c < CN; ++c) nV[j][c] = from_next_lane(V[0][j][c]);
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
                float av;  // alpha_{u-1} of the state the term leaves from ("row -1": state 0, the one live state, holds 1)
                if constexpr (kDel) {  // state s - 1, where the forward window holds it
                    const bool below = live && s >= 1 && s - 1 >= lo_a && s - 1 <= hi_a;
                    av = u > 0 ? (below ? am[(int64_t)(u - 1) * C + (s - 1) % C] : 0.0f) : (s == 1 ? 1.0f : 0.0f);
                } else {
                    av = u > 0 ? (live ? arow[r] : 0.0f) : 1.0f;
                }
                const float b0 = (own && table) ? crf_term(bo, crf_post_value(p, lds, rw, u, i, sig, 0), sh) : 0.0f;
                const float b1 = (nxt && table) ? crf_term(bn, crf_post_value(p, lds, rw, u, i, sig, y), sh) : 0.0f;
                const float b_new = b0 + b1;  // (b[r] itself is written last: the terms below read it as it stands at row u)
                // what position s gains at this row: state s emits c, the variant's state s + 1 takes over (insertion: the
                // variant's state lives in slot s itself; deletion: state s - 1 emits y_s, the variant goes on in slot s + 1)
                // (the slot's exponent rises, its accumulators rescaled with it, before a term of 2^kAccTop or more enters: a
                // variant that outweighs y by more than f32 holds takes the accumulators down with it instead of overflowing)
                int sig_from = sig;
                bool from_table = table;
                if constexpr (kDel) {
                    const uint32_t sb = lds.info[(live && s >= 1) ? s - 1 : 0] & 0xFFFFFFu;
                    from_table = sb != kNoState;
                    sig_from = from_table ? (int)sb : 0;
                }
                const bool gains = kSub ? nxt : (kIns ? own : (nxt && s >= 1 && s < L));
#pragma unroll
                for (int c = 0; c < CN; ++c) {
                    if (c < nb && gains) {
                        float vn;
                        if constexpr (kIns) vn = V[r][0][c];
                        else if constexpr (kDel && JN == 0) vn = r + 1 < K ? b[r + 1 < K ? r + 1 : 0] : nb0;
                        else vn = r + 1 < K ? V[r + 1 < K ? r + 1 : 0][0][c] : nV[0][c];
                        float pm;
                        int pe;
                        crf_split(from_table ? crf_post_value(p, lds, rw, u, i, sig_from, kDel ? y : c + 1) : 0.0f, &pm, &pe);
                        const float term = (av * pm) * vn;
                        const int e = finite_exp(term);
                        if (e != kNoExp && e + dt + pe - kAccTop > xa[r]) {
                            const int up = e + dt + pe - kAccTop;
                            const int down = max(xa[r] - up, -512);
#pragma unroll
                            for (int c2 = 0; c2 < CN; ++c2) acc[r][c2] = ldexpf(acc[r][c2], down);
                            xa[r] = up;
                        }
                        acc[r][c] += ldexpf(term, min(max(dt + pe - xa[r], -512), 512));
                    }
                }
                int pw = 1;
#pragma unroll
                for (int j = 0; j < JN; ++j) {
                    if (kSlotFence) __asm__ volatile("" ::: "memory");
                    const bool chain = crf_chain_live<WALK>(live, j, m, s);
                    const int yk = crf_chain_word<WALK>(lds, chain, s, j);
                    const int base = kSub ? 0 : crf_edit_row_base<WALK>(p, chain, yk, sig, pw, nb);
#pragma unroll
                    for (int c = 0; c < CN; ++c) {
                        bool ok = chain && c < nb;
                        int sv = 0;
                        if constexpr (kSub) sv = ok ? (p.in.S == 1 ? yk - 1 : sig) + (c + 1 - yk) * pw : 0;  // (S == 1: below, then c)
                        else sv = ok ? base + (kIns ? c * pw : 0) : 0;
                        ok = ok && sv < p.in.S;
                        const float vo = own ? V[r][j][c] : 0.0f;
                        const float up = j + 1 < JN ? (r + 1 < K ? V[r + 1 < K ? r + 1 : 0][j + 1 < JN ? j + 1 : 0][c]
                                                                 : nV[j + 1 < JN ? j + 1 : 0][c])
                                                    : (r + 1 < K ? b[r + 1 < K ? r + 1 : 0] : nb0);
                        const float vn = nxt ? up : 0.0f;
                        const float c0 = (ok && own) ? crf_term(vo, crf_post_value(p, lds, rw, u, i, sv, 0), sh) : 0.0f;
                        const float c1 = (ok && nxt) ? crf_term(vn, crf_post_value(p, lds, rw, u, i, sv, y), sh) : 0.0f;
                        V[r][j][c] = j < (kDel ? m - 1 : m) ? c0 + c1 : b_new;
                    }
                    pw *= nb;
                }
                b[r] = b_new;
            }
        }
    }
    // the positions whose state is live at "row -1": state 0 (deletion: and state 1)
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = slot_state<K>(lane, r, lo_p);
        if (s <= hi_p) crf_store_position<WALK, NB, CN>(q, s, L, nb, acc[r], xp + xa[r], lp);
    }
}

// ---- the edge occupancies of the labelling's own lattice (fcd_crf_occupancy_*; include/fcd.h) ----
// The fourth walk, compiled into crfp_back_kernel<K, 2, 4> only: beta alone, no chain values, so it needs no S == nb^m.
// Step u = T_r - 1 .. 0, with beta_u in the registers and alpha_{u-1} in the stored rows:
//   stay[s] = alpha_{u-1}[s] * P(u,s,0)   * beta_u[s]     / P        into entry (sigma_s, 0)
//   adv[s]  = alpha_{u-1}[s] * P(u,s,y_s) * beta_u[s + 1] / P        into entry (sigma_s, y_s)
// each the mantissa products (two roundings), the exact power of two 2^(Ea(u-1) + Eb(u) + e - floor(log2 P)) and the division
// by P's mantissa (one rounding); then beta_{u-1} in place, as the substitution walk forms it.  Several states of a row may
// share an entry (sigma is the last m labels: a homopolymer run shares one): the row's terms are added up in an S * N float
// row of LDS behind the labelling's trajectory, and the first lane to exchange an entry for 0 holds its sum and adds
// scale * sum to the output -- one lane per touched entry, no global atomics; an entry nobody touches is never read or
// written.  The kernel always adds: with q.occ_clear the walk zeroes rows t < T_r of its block first (a labelling without a
// positive finite P(y | x) has returned by then: its block keeps what it held).
// The lattice the rows cannot hold.  alpha and beta keep one exponent per row; where a long read does not support its
// labelling their maxima sit at opposite ends of the window and the cells that carry the probability fall out of range.
// The terms of a row sum to 1 exactly, each is within (6 T_r + W + 1) 2^-24 of its value and the wave's sum adds 2 K + 6
// roundings, so a row whose computed terms are further than kOccLost(T_r) = 2 (6 T_r + 64 K + 2 K + 8) 2^-24 from 1 has lost
// cells (or P has, in the forward walk): the walk then gives up -- logp = NaN and NaN in every row t < T_r of the block --
// rather than hand out occupancies that do not add up.
// (wave_fsum, the sum of a non-negative value over the wavefront: device_utils.h)
template <int K>
__device__ __forceinline__ void crfp_occ_walk(const CrfPostParams &q, unsigned char *smem) {
    constexpr int C = 64 * K;
    const CrfParams &p = q.c;
    const CrfLds lds = crf_carve(smem);
    float *sum = reinterpret_cast<float *>(lds.info + p.lab_cap);  // [S * N], behind crf_lds_bytes(lab_cap)
    CrfRow rw;
    if (!crf_prologue(p, lds, &rw)) return;
    const double lp = p.logp[blockIdx.x];
    if (lp - lp != 0.0) return;  // P = 0, or a NaN on the way: nothing of the block is written
    const int lane = threadIdx.x, L = rw.L, N = p.in.N, SN = p.in.S * N;
    float *out = q.occ + (int64_t)blockIdx.x * q.occ_stride_row;
    for (int e = lane; e < SN; e += 64) sum[e] = 0.0f;
    if (q.occ_clear) {
        if (q.occ_stride_t == (int64_t)SN) {
            for (int64_t e = lane; e < (int64_t)rw.Tr * SN; e += 64) out[e] = 0.0f;
        } else {
            for (int t = 0; t < rw.Tr; ++t)
                for (int e = lane; e < SN; e += 64) out[(int64_t)t * q.occ_stride_t + e] = 0.0f;
        }
    }
    __syncthreads();  // the zeros are in place before another lane adds to them
    const float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    const int *ae = reinterpret_cast<const int *>(am + (int64_t)p.in.T * C);
    float b[K];
#pragma unroll
    for (int r = 0; r < K; ++r) b[r] = 0.0f;
    int64_t eb = 0;
    const int64_t xp = (int64_t)floor(lp * 1.44269504088896340735992468100189214);  // floor(log2 P(y | x))
    const float pman = (float)exp(lp - (double)xp * kLn2);                          // P / 2^xp, in [1, 2]
    const float lost = 2.0f * (6.0f * (float)rw.Tr + (float)(C + 2 * K + 8)) * 5.9604644775390625e-8f;  // kOccLost(T_r)
    bool first = true;
    for (int t0 = (rw.Tr - 1) / p.rows_per_tile * p.rows_per_tile; t0 >= 0; t0 -= p.rows_per_tile) {
        const int rc = min(p.rows_per_tile, rw.Tr - t0);
        crf_fill_tile(p, lds, rw, t0, rc);
        stage_krow_before(lds.misc, rw.path, L, p.band, t0);  // the window of the row before the tile
        for (int i = rc - 1; i >= 0; --i) {
            const int u = t0 + i;
            int lo_u, hi_u;  // the window of row u: the states whose beta the registers hold
            crf_window(p, lds, rw, u, i, &lo_u, &hi_u);
            int lo_p = 0, hi_p = 0;  // the window of row u - 1 ("row -1": state 0): the states the terms leave from
            int64_t x_u = 0;
            if (u > 0) {
                crf_window_k(p, rw, u - 1, krow_before(lds.krow, lds.misc, p.band, i), &lo_p, &hi_p);
                x_u = ae[u - 1];
            }
            const float *arow = am + (int64_t)max(u - 1, 0) * C + lane * K;  // alpha_{u-1}, by slot
            if (first) {  // row T_r - 1: state L
#pragma unroll
                for (int r = 0; r < K; ++r) b[r] = slot_state<K>(lane, r, lo_u) == L ? 1.0f : 0.0f;
                first = false;
            }
            // ---- the row's posteriors and the exponents: the largest frexp(beta) + frexp(posterior) over its products ----
            const float nb0 = from_next_lane(b[0]);  // the next lane's first slot, as it stands at row u
            float p0[K], py[K], bo[K], bn[K], av[K];
            int ent[K], ys[K];
            int emax = kNoExp;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int s = slot_state<K>(lane, r, lo_p);
                const bool live = s <= hi_p;
                const bool own = live && s >= lo_u && s <= hi_u;          // state s holds a value at row u
                const bool nxt = live && s + 1 >= lo_u && s + 1 <= hi_u;  // state s + 1 does (s < L: hi_u <= L)
                const uint32_t info = lds.info[live ? s : 0];  // (a dead slot reads a valid address and is masked below)
                const uint32_t sg = info & 0xFFFFFFu;
                const bool table = sg != kNoState;
                const int sig = table ? (int)sg : 0;
                ys[r] = (int)(info >> 24);
                ent[r] = sig * N;
                bo[r] = own ? b[r] : 0.0f;
                bn[r] = nxt ? (r + 1 < K ? b[r + 1 < K ? r + 1 : 0] : nb0) : 0.0f;
                p0[r] = (own && table) ? crf_post_value(p, lds, rw, u, i, sig, 0) : 0.0f;
                py[r] = (nxt && table) ? crf_post_value(p, lds, rw, u, i, sig, ys[r]) : 0.0f;
                av[r] = u > 0 ? (live ? arow[r] : 0.0f) : 1.0f;  // ("row -1": state 0, the one live state, holds 1)
                emax = max(emax, crf_term_exp(bo[r], p0[r]));
                emax = max(emax, crf_term_exp(bn[r], py[r]));
            }
            emax = wave_imax(emax);
            const int sh = emax == kNoExp ? 0 : kTargetB - emax;
            x_u += eb;  // the exponent of this step's terms: alpha of row u - 1 times beta of row u
            const int dt = (int)min(max(x_u - xp, (int64_t)-(1 << 20)), (int64_t)(1 << 20));
            eb -= sh;
            // ---- the occupancies of row u, then beta of row u - 1 in place ----
            float stay[K], adv[K];
            float mass = 0.0f;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                float m0, my;
                int e0, ey;
                crf_split(p0[r], &m0, &e0);
                crf_split(py[r], &my, &ey);
                stay[r] = ldexpf((av[r] * m0) * bo[r], min(max(dt + e0, -512), 512)) / pman;
                adv[r] = ldexpf((av[r] * my) * bn[r], min(max(dt + ey, -512), 512)) / pman;
                mass += stay[r] + adv[r];
                if (stay[r] > 0.0f) atomicAdd(&sum[ent[r]], stay[r]);
                if (adv[r] > 0.0f) atomicAdd(&sum[ent[r] + ys[r]], adv[r]);
                b[r] = crf_term(bo[r], p0[r], sh) + crf_term(bn[r], py[r], sh);
            }
            mass = wave_fsum(mass);
            if (!(fabsf(mass - 1.0f) <= lost)) {  // (wave-uniform) the rows cannot hold this lattice
                __syncthreads();
                for (int t = 0; t < rw.Tr; ++t)
                    for (int e = lane; e < SN; e += 64) out[(int64_t)t * q.occ_stride_t + e] = NAN;
                if (lane == 0) p.logp[blockIdx.x] = (double)NAN;
                return;
            }
            __syncthreads();  // every term of the row is in its entry
            float *orow = out + (int64_t)u * q.occ_stride_t;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                if (stay[r] > 0.0f) {
                    const float v = atomicExch(&sum[ent[r]], 0.0f);  // the first lane here takes the sum and leaves the entry clear
                    if (v != 0.0f) orow[ent[r]] = orow[ent[r]] + q.occ_scale * v;
                }
                if (adv[r] > 0.0f) {
                    const float v = atomicExch(&sum[ent[r] + ys[r]], 0.0f);
                    if (v != 0.0f) orow[ent[r] + ys[r]] = orow[ent[r] + ys[r]] + q.occ_scale * v;
                }
            }
            __syncthreads();  // ... and clear again before the next row adds
        }
    }
}

// The same walk for a window that lives in LDS (fcd_set_crf_lattice_wide; crf_lattice.h has the layout): J = q.wide_j states
// per lane, compiled into crfp_back_kernel<8, 2, 4> only.  The terms, their roundings, the S * N row and its add-then-exchange,
// the give-up rule and everything around the time loop are crfp_occ_walk's.  A step is two passes over the lane's J cells.
// The first reads beta_u -- the lane's own cells in ascending order, the slot above its last one (the next lane's first)
// ahead of the loop, before that lane writes over it --, adds the terms to their entries and to the row's mass (lane-serial,
// in slot order; then wave_fsum: 2 J + 6 roundings, lost(T_r) with J in K's place) and leaves both products of beta_{u-1} and
// their exponents where crf_forward_walk_lds leaves its own; the second rescales and adds them into the cell.  The bits "a
// term went into the entry" ride with the exponents to the exchange.
constexpr uint32_t kWideStay = 1u << 18, kWideAdv = 1u << 19;

__device__ __forceinline__ void crfp_occ_walk_lds(const CrfPostParams &q, unsigned char *smem) {
    const CrfParams &p = q.c;
    const int J = q.wide_j, C = 64 * J;
    const CrfLds lds = crf_carve(smem);
    float *sum = reinterpret_cast<float *>(lds.info + p.lab_cap);  // [S * N], behind crf_lds_bytes(lab_cap)
    CrfRow rw;
    if (!crf_prologue(p, lds, &rw)) return;
    const double lp = p.logp[blockIdx.x];
    if (lp - lp != 0.0) return;  // P = 0, or a NaN on the way: nothing of the block is written
    const int lane = threadIdx.x, L = rw.L, N = p.in.N, SN = p.in.S * N;
    const CrfWideLds w = crf_wide_carve(sum + SN, J);
    float *out = q.occ + (int64_t)blockIdx.x * q.occ_stride_row;
    for (int e = lane; e < SN; e += 64) sum[e] = 0.0f;
    if (q.occ_clear) {
        if (q.occ_stride_t == (int64_t)SN) {
            for (int64_t e = lane; e < (int64_t)rw.Tr * SN; e += 64) out[e] = 0.0f;
        } else {
            for (int t = 0; t < rw.Tr; ++t)
                for (int e = lane; e < SN; e += 64) out[(int64_t)t * q.occ_stride_t + e] = 0.0f;
        }
    }
    const float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    const int *ae = reinterpret_cast<const int *>(am + (int64_t)p.in.T * C);
    int64_t eb = 0;
    const int64_t xp = (int64_t)floor(lp * 1.44269504088896340735992468100189214);  // floor(log2 P(y | x))
    const float pman = (float)exp(lp - (double)xp * kLn2);                          // P / 2^xp, in [1, 2]
    const float lost = 2.0f * (6.0f * (float)rw.Tr + (float)(C + 2 * J + 8)) * 5.9604644775390625e-8f;  // kOccLost(T_r)
    bool first = true;
    for (int t0 = (rw.Tr - 1) / p.rows_per_tile * p.rows_per_tile; t0 >= 0; t0 -= p.rows_per_tile) {
        const int rc = min(p.rows_per_tile, rw.Tr - t0);
        crf_fill_tile(p, lds, rw, t0, rc);  // (its barriers: the zeros above are in place before a lane adds to them)
        stage_krow_before(lds.misc, rw.path, L, p.band, t0);  // the window of the row before the tile
        for (int i = rc - 1; i >= 0; --i) {
            const int u = t0 + i;
            int lo_u, hi_u;  // the window of row u: the states whose beta the cells hold
            crf_window(p, lds, rw, u, i, &lo_u, &hi_u);
            int lo_p = 0, hi_p = 0;  // the window of row u - 1 ("row -1": state 0): the states the terms leave from
            int64_t x_u = 0;
            if (u > 0) {
                crf_window_k(p, rw, u - 1, krow_before(lds.krow, lds.misc, p.band, i), &lo_p, &hi_p);
                x_u = ae[u - 1];
            }
            const float *arow = am + (int64_t)max(u - 1, 0) * C;  // alpha_{u-1}, a slot's at crf_wide_at
            if (first) {  // row T_r - 1: state L
                for (int j = 0; j < J; ++j) w.cell[crf_wide_at(lane, j)] = crf_wide_state(lane * J + j, lo_u, C) == L ? 1.0f : 0.0f;
                first = false;
                __syncthreads();
            }
            x_u += eb;  // the exponent of this step's terms: alpha of row u - 1 times beta of row u
            const int dt = (int)min(max(x_u - xp, (int64_t)-(1 << 20)), (int64_t)(1 << 20));
            // ---- the occupancies of row u, the products of beta of row u - 1 and the largest of their exponents ----
            const float nb0 = w.cell[crf_wide_at((lane + 1) & 63, 0)];  // the next lane's first slot, as it stands at row u
            __syncthreads();                                            // ... read before that lane's first pass writes it
            int emax = kNoExp;
            float mass = 0.0f;
            float b_own = w.cell[crf_wide_at(lane, 0)];
            for (int j = 0; j < J; ++j) {
                const int at = crf_wide_at(lane, j);
                const float b_up = j + 1 < J ? w.cell[crf_wide_at(lane, j + 1 < J ? j + 1 : 0)] : nb0;
                const int s = crf_wide_state(lane * J + j, lo_p, C);
                const bool live = s <= hi_p;
                const bool own = live && s >= lo_u && s <= hi_u;          // state s holds a value at row u
                const bool nxt = live && s + 1 >= lo_u && s + 1 <= hi_u;  // state s + 1 does (s < L: hi_u <= L)
                const uint32_t info = lds.info[live ? s : 0];  // (a dead slot reads a valid address and is masked below)
                const uint32_t sg = info & 0xFFFFFFu;
                const bool table = sg != kNoState;
                const int sig = table ? (int)sg : 0;
                const int ys = (int)(info >> 24), ent = sig * N;
                const float bo = own ? b_own : 0.0f;
                const float bn = nxt ? b_up : 0.0f;
                const float p0 = (own && table) ? crf_post_value(p, lds, rw, u, i, sig, 0) : 0.0f;
                const float py = (nxt && table) ? crf_post_value(p, lds, rw, u, i, sig, ys) : 0.0f;
                const float av = u > 0 ? (live ? arow[at] : 0.0f) : 1.0f;  // ("row -1": state 0, the one live state, holds 1)
                emax = max(emax, crf_term_exp(bo, p0));
                emax = max(emax, crf_term_exp(bn, py));
                float m0, my;
                int e0, ey;
                crf_split(p0, &m0, &e0);
                crf_split(py, &my, &ey);
                const float stay = ldexpf((av * m0) * bo, min(max(dt + e0, -512), 512)) / pman;
                const float adv = ldexpf((av * my) * bn, min(max(dt + ey, -512), 512)) / pman;
                mass += stay + adv;
                if (stay > 0.0f) atomicAdd(&sum[ent], stay);
                if (adv > 0.0f) atomicAdd(&sum[ent + ys], adv);
                w.cell[at] = bo * m0;  // (crf_term's mantissa products; the power of two waits for the row's exponent)
                w.up[at] = bn * my;
                w.exp[at] = crf_wide_pack(e0, ey) | (stay > 0.0f ? kWideStay : 0u) | (adv > 0.0f ? kWideAdv : 0u);
                b_own = b_up;
            }
            emax = wave_imax(emax);
            const int sh = emax == kNoExp ? 0 : kTargetB - emax;
            eb -= sh;
            mass = wave_fsum(mass);
            if (!(fabsf(mass - 1.0f) <= lost)) {  // (wave-uniform) the rows cannot hold this lattice
                __syncthreads();
                for (int t = 0; t < rw.Tr; ++t)
                    for (int e = lane; e < SN; e += 64) out[(int64_t)t * q.occ_stride_t + e] = NAN;
                if (lane == 0) p.logp[blockIdx.x] = (double)NAN;
                return;
            }
            __syncthreads();  // every term of the row is in its entry
            float *orow = out + (int64_t)u * q.occ_stride_t;
            for (int j = 0; j < J; ++j) {
                const int at = crf_wide_at(lane, j);
                const uint32_t word = w.exp[at];
                w.cell[at] = ldexpf(w.cell[at], min(max(crf_wide_e0(word) + sh, -512), 512)) +
                             ldexpf(w.up[at], min(max(crf_wide_ey(word) + sh, -512), 512));  // beta of row u - 1
                if (word & (kWideStay | kWideAdv)) {
                    const int s = crf_wide_state(lane * J + j, lo_p, C);
                    const uint32_t info = lds.info[s <= hi_p ? s : 0];
                    const uint32_t sg = info & 0xFFFFFFu;
                    const int ent = (sg != kNoState ? (int)sg : 0) * N, ys = (int)(info >> 24);
                    if (word & kWideStay) {
                        const float v = atomicExch(&sum[ent], 0.0f);  // the first lane here takes the sum and leaves the entry clear
                        if (v != 0.0f) orow[ent] = orow[ent] + q.occ_scale * v;
                    }
                    if (word & kWideAdv) {
                        const float v = atomicExch(&sum[ent + ys], 0.0f);
                        if (v != 0.0f) orow[ent + ys] = orow[ent + ys] + q.occ_scale * v;
                    }
                }
            }
            __syncthreads();  // ... and clear again before the next row adds; beta of row u - 1 in every cell
        }
    }
}

template <int K, int MM, int NB>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void crfp_back_kernel(CrfPostParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (K == 8 && MM == 2 && NB == 4) {  // (the LDS-resident window rides in this one only)
        if (q.walk == kWalkOcc && q.wide_j > 0) return crfp_occ_walk_lds(crfp_params_again(q), smem);
    }
    // (every instantiation carries these three walks within its 256 registers: a kernel's count is its widest walk's)
    if constexpr (MM == 2 && NB == 4) {  // (the occupancy walk rides in these four only)
        if (q.walk == kWalkOcc) return crfp_occ_walk<K>(q, smem);
    }
    if (q.walk == kWalkIns) return crfp_back_walk<K, MM, NB, kWalkIns>(q, smem);
    if (q.walk == kWalkDel) return crfp_back_walk<K, MM, NB, kWalkDel>(q, smem);
    crfp_back_walk<K, MM, NB, kWalkSub>(q, smem);
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

// forward, then the backward walks of q[1 .. n_back] (crf_posterior: one; crf_edits: insertion, deletion), all on the rows
// the forward launch stored
template <int K, int MM, int NB>
void launch_pair(const CrfPostParams *q, int n_back, dim3 grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL(crfp_fwd_kernel<K>, grid, dim3(64), lds, stream, q[0]);
    for (int w = 1; w <= n_back; ++w) hipLaunchKernelGGL((crfp_back_kernel<K, MM, NB>), grid, dim3(64), lds, stream, q[w]);
}

// KMAX: the most states per lane the tier is instantiated at -- 8: 1, 2, 4, 8; 4: 1, 2, 4; 3: 1, 2, 3 (what fits 256 VGPRs
// without scratch: eight states of eight labels do not)
template <int MM, int NB, int KMAX>
hipError_t launch_tier(const CrfPostParams *q, int n_back, int k, dim3 grid, size_t lds, hipStream_t stream) {
    if (k == 1) launch_pair<1, MM, NB>(q, n_back, grid, lds, stream);
    else if (k == 2) launch_pair<2, MM, NB>(q, n_back, grid, lds, stream);
    else if (KMAX == 3 && k == 3) launch_pair<KMAX == 3 ? 3 : 1, MM, NB>(q, n_back, grid, lds, stream);
    else if (KMAX >= 4 && k == 4) launch_pair<KMAX >= 4 ? 4 : 1, MM, NB>(q, n_back, grid, lds, stream);
    else if (KMAX >= 8 && k == 8) launch_pair<KMAX >= 8 ? 8 : 1, MM, NB>(q, n_back, grid, lds, stream);
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
    return stored_rows_bytes(T, k);
}

namespace {
// q[0]: the forward launch; q[1 .. n_back]: the backward walks
hipError_t launch_crf_walks(CrfPostParams *q, int n_back, const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init,
                            int64_t init_stride, int64_t band, double *logp, unsigned char *alpha, hipStream_t stream) {
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    const CrfParams c = crf_params(in, y, init, n_init, init_stride, band);
    for (int w = 0; w <= n_back; ++w) {
        const int lo = q[w].c.cone_lo, hi = q[w].c.cone_hi;
        q[w].c = c;
        q[w].c.cone_lo = lo;
        q[w].c.cone_hi = hi;
        q[w].c.logp = logp;
        q[w].alpha = reinterpret_cast<float *>(alpha);
        q[w].alpha_words = (int64_t)(crf_posterior_row_bytes(in.T, in.S, in.N, y.stride, band) / 4);
        q[w].m = crf_post_chain(in.S, in.N - 1);
    }
    const dim3 grid((unsigned)rows);
    const size_t lds = crf_lds_bytes(c.lab_cap);
    const int tier = crf_post_tier(q[0].m, in.N - 1), k = crf_post_states_per_lane(tier, in.T, y.stride, band);
    switch (tier) {
    case 0: return launch_tier<1, 8, 4>(q, n_back, k, grid, lds, stream);
    case 1: return launch_tier<2, 4, 8>(q, n_back, k, grid, lds, stream);
    case 2: return launch_tier<4, 2, 8>(q, n_back, k, grid, lds, stream);
    case 3: return launch_tier<3, 8, 3>(q, n_back, k, grid, lds, stream);
    case 4: return launch_tier<6, 4, 3>(q, n_back, k, grid, lds, stream);
    default: return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t launch_crf_posterior(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                                int64_t band, float *post, double *logp, unsigned char *alpha, hipStream_t stream) {
    CrfPostParams q[2] = {};
    q[0].walk = q[1].walk = kWalkSub;
    q[0].post = q[1].post = post;
    return launch_crf_walks(q, 1, in, y, init, n_init, init_stride, band, logp, alpha, stream);
}

// forward (the cone one state wider below, for the deletions), the insertion walk, the deletion walk (one state wider
// above): the stored forward rows are read by both walks
hipError_t launch_crf_edits(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                            int64_t band, float *deletion, float *insertion, double *logp, unsigned char *alpha,
                            hipStream_t stream) {
    CrfPostParams q[3] = {};
    q[0].walk = kWalkSub;
    q[0].c.cone_lo = 1;
    q[1].walk = kWalkIns;
    q[2].walk = kWalkDel;
    q[2].c.cone_hi = 1;
    q[1].ins = q[2].ins = insertion;
    q[1].del = q[2].del = deletion;
    return launch_crf_walks(q, 2, in, y, init, n_init, init_stride, band, logp, alpha, stream);
}

// ---- fcd_crf_occupancy_*: crfp_fwd_kernel<K>, then the occupancy walk in crfp_back_kernel<K, 2, 4> ----
namespace {
constexpr size_t kOccLdsLimit = 160 * 1024;  // what a workgroup is granted on gfx950

size_t crf_occupancy_lds_bytes(int64_t T, int64_t S, int64_t N, int64_t stride) {
    return crf_lds_bytes((int)std::min<int64_t>(std::min(T, stride) + 1, 1 << 24)) + (size_t)S * (size_t)N * 4;
}

template <int K>
hipError_t launch_occupancy_pair(const CrfPostParams *q, dim3 grid, size_t lds_fwd, size_t lds_back, hipStream_t stream) {
    const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(crfp_back_kernel<K, 2, 4>), (int)lds_back);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crfp_fwd_kernel<K>, grid, dim3(64), lds_fwd, stream, q[0]);
    hipLaunchKernelGGL((crfp_back_kernel<K, 2, 4>), grid, dim3(64), lds_back, stream, q[1]);
    return hipGetLastError();
}
}  // namespace

// 0 = the kernels hold the call; 2 = more than 8 labels, 6 = the labelling and the S * N row exceed the LDS of a workgroup
int crf_occupancy_unsupported(int64_t T, int64_t S, int64_t N, int64_t stride) {
    if (N - 1 > 8) return 2;
    if (S > (1 << 24) || crf_occupancy_lds_bytes(T, S, N, stride) > kOccLdsLimit) return 6;
    return 0;
}

size_t crf_occupancy_row_bytes(int64_t T, int64_t stride, int64_t band) {
    return stored_rows_bytes(T, (size_t)crf_states_per_lane(T, stride, band));
}

hipError_t launch_crf_occupancy(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                                int64_t band, const OccupancyDesc &out, double *logp, unsigned char *alpha, hipStream_t stream) {
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    CrfPostParams q[2] = {};
    for (int w = 0; w < 2; ++w) {
        q[w].c = crf_params(in, y, init, n_init, init_stride, band);
        q[w].c.logp = logp;
        q[w].alpha = reinterpret_cast<float *>(alpha);
        q[w].alpha_words = (int64_t)(crf_occupancy_row_bytes(in.T, y.stride, band) / 4);
        q[w].m = 1;  // (no chain values: the walk never asks)
        q[w].walk = w ? kWalkOcc : kWalkSub;
        q[w].occ = out.occ;
        q[w].occ_stride_row = out.stride_row;
        q[w].occ_stride_t = out.stride_t;
        q[w].occ_scale = out.scale;
        q[w].occ_clear = out.accumulate ? 0 : 1;
    }
    const dim3 grid((unsigned)rows);
    const size_t lds_fwd = crf_lds_bytes(q[0].c.lab_cap), lds_back = lds_fwd + (size_t)in.S * (size_t)in.N * 4;
    switch (crf_states_per_lane(in.T, y.stride, band)) {
    case 1: return launch_occupancy_pair<1>(q, grid, lds_fwd, lds_back, stream);
    case 2: return launch_occupancy_pair<2>(q, grid, lds_fwd, lds_back, stream);
    case 4: return launch_occupancy_pair<4>(q, grid, lds_fwd, lds_back, stream);
    case 8: return launch_occupancy_pair<8>(q, grid, lds_fwd, lds_back, stream);
    default: return hipErrorInvalidValue;
    }
}

// ---- fcd_set_crf_lattice_wide: windows beyond 512 states, walked in LDS inside crfp_fwd_kernel<8> / crfp_back_kernel<8, 2, 4> ----
namespace {
int crf_wide_states_per_lane(int64_t T, int64_t stride, int64_t band) {
    return (int)((crf_lattice_window_states(T, stride, band) + 63) / 64);
}

size_t crf_wide_launch_lds(int64_t T, int64_t S, int64_t N, int64_t stride, int64_t band, bool occupancy) {
    return crf_lds_bytes((int)std::min<int64_t>(std::min(T, stride) + 1, 1 << 24)) + (occupancy ? (size_t)S * (size_t)N * 4 : 0) +
           crf_wide_lds_bytes(crf_wide_states_per_lane(T, stride, band));
}
}  // namespace

bool crf_lattice_is_wide(int64_t T, int64_t stride, int64_t band) { return crf_lattice_window_states(T, stride, band) > 512; }

int crf_lattice_wide_unsupported(int64_t T, int64_t S, int64_t N, int64_t stride, int64_t band, bool occupancy, size_t *lds_bytes) {
    *lds_bytes = 0;
    if (N - 1 > 8) return 2;
    if (crf_lattice_window_states(T, stride, band) > 4096) return 1;
    if (S >= (int64_t)kNoState) return 3;
    *lds_bytes = crf_wide_launch_lds(T, S, N, stride, band, occupancy);
    return *lds_bytes > kOccLdsLimit ? 4 : 0;
}

size_t crf_lattice_wide_row_bytes(int64_t T, int64_t stride, int64_t band) {
    if (!crf_lattice_is_wide(T, stride, band)) return crf_occupancy_row_bytes(T, stride, band);
    return stored_rows_bytes(T, (size_t)crf_wide_states_per_lane(T, stride, band));
}

namespace {
CrfPostParams crf_wide_params(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                              int64_t band, double *logp) {
    CrfPostParams q = {};
    q.c = crf_params(in, y, init, n_init, init_stride, band);
    q.c.logp = logp;
    q.m = 1;  // (no chain values: neither walk asks)
    q.walk = kWalkSub;
    q.wide_j = crf_wide_states_per_lane(in.T, y.stride, band);
    return q;
}
}  // namespace

hipError_t launch_crf_score_wide(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                                 int64_t band, double *logp, hipStream_t stream) {
    if (!crf_lattice_is_wide(in.T, y.stride, band)) return launch_crf_score(in, y, init, n_init, init_stride, band, logp, stream);
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    const CrfPostParams q = crf_wide_params(in, y, init, n_init, init_stride, band, logp);  // (alpha null: the sum alone)
    const size_t lds = crf_wide_launch_lds(in.T, in.S, in.N, y.stride, band, false);
    const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(crfp_fwd_kernel<8>), (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crfp_fwd_kernel<8>, dim3((unsigned)rows), dim3(64), lds, stream, q);
    return hipGetLastError();
}

hipError_t launch_crf_occupancy_wide(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                                     int64_t band, const OccupancyDesc &out, double *logp, unsigned char *alpha, hipStream_t stream) {
    if (!crf_lattice_is_wide(in.T, y.stride, band))
        return launch_crf_occupancy(in, y, init, n_init, init_stride, band, out, logp, alpha, stream);
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    CrfPostParams q[2];
    for (int w = 0; w < 2; ++w) {
        q[w] = crf_wide_params(in, y, init, n_init, init_stride, band, logp);
        q[w].alpha = reinterpret_cast<float *>(alpha);
        q[w].alpha_words = (int64_t)(crf_lattice_wide_row_bytes(in.T, y.stride, band) / 4);
        q[w].walk = w ? kWalkOcc : kWalkSub;
        q[w].occ = out.occ;
        q[w].occ_stride_row = out.stride_row;
        q[w].occ_stride_t = out.stride_t;
        q[w].occ_scale = out.scale;
        q[w].occ_clear = out.accumulate ? 0 : 1;
    }
    const size_t lds_fwd = crf_wide_launch_lds(in.T, in.S, in.N, y.stride, band, false);
    const size_t lds_back = crf_wide_launch_lds(in.T, in.S, in.N, y.stride, band, true);
    hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(crfp_fwd_kernel<8>), (int)lds_fwd);
    if (e == hipSuccess) e = allow_dynamic_lds(reinterpret_cast<const void *>(crfp_back_kernel<8, 2, 4>), (int)lds_back);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)rows);
    hipLaunchKernelGGL(crfp_fwd_kernel<8>, grid, dim3(64), lds_fwd, stream, q[0]);
    hipLaunchKernelGGL((crfp_back_kernel<8, 2, 4>), grid, dim3(64), lds_back, stream, q[1]);
    return hipGetLastError();
}

}  // namespace fcd
