// ctc_posterior.hip -- CTC forward-backward substitution posteriors of given labellings (fcd_ctc_posterior_*;
// include/fcd.h): post[k][c] = P(y[k:=c] | x) / sum_c' P(y[k:=c'] | x) for every label position k and every label c, from
// ONE forward and ONE backward walk of the lattice ctc_score.hip sums over.  NOT a reference function.
//
// Two launches, one wavefront per labelling each, the register-resident window of ctc_score.hip (K consecutive states
// per lane, state s in slot s mod 64K):
//   post_fwd_kernel<K>       ctc_score's forward step (under fcd_ctc_posterior_* its logp is ctc_score's bit for bit; under
//                            fcd_ctc_edits_* the relaxed window can move a row's scale, and the value is ctc_score's within
//                            its tolerance -- that much is tested, not the bits).  Every row's live
//                            cells go to the workspace by SLOT, scaled by 2^-kAlphaDown (exact), and the row's exponent
//                            next to them: T * 64K floats, then T exponent words, per labelling.
//   post_back_kernel<K, NC>  walks the rows from T_r - 1 down.  b_t[s] = p[t][z[s]] * beta_t[s] obeys the mirror image of
//                            the forward step, b_t[s] = (b_{t+1}[s] + b_{t+1}[s+1] + b_{t+1}[s+2]) * p[t][z[s]] under the
//                            same transition rules ("row T_r": all mass on state 2L), so a cell is again at most two sums
//                            and one product.  A label state s = 2k + 1 also carries, for each label c <= NC,
//                              w_t(c)  = (w_{t+1}(c) [collapse] + b_{t+1}[s+1] + [c != y_{k+1} or no collapse] b_{t+1}[s+2]) * p[t][c]
//                                        the backward value of state s had its label been c, and
//                              acc(c) += (alpha_{t-1}[s-1] + [s >= 3, c != y_{k-1} or no collapse] alpha_{t-1}[s-2]) * w_t(c)
//                            summed over the rows s is live at: P(y[k:=c] | x) up to a scale all c share.  When s leaves the
//                            window (or after row 0) the lane divides by the sum over c and stores post[k][.].
// Scales.  b and w share one integer exponent per row (the row's largest b or w lands in [2^(kTargetB-1), 2^kTargetB));
// alpha has the forward pass's.  A term of acc therefore has the wave-uniform exponent X_t = Ea(t-1) + Eb(t); acc is kept
// at the largest X seen so far, kAccDown bits below it so that the sum over the rows cannot overflow: a term is scaled by
// the power of two 2^(X_t - Xmax - kAccDown), acc by 2^(Xmax_old - Xmax_new) when Xmax rises.  Both exact.
// Every term is non-negative; one rounding per product and per sum; no fused multiply-add (-ffp-contract=off).
//
// fcd_ctc_edits_* (the deletion and insertion likelihoods of the same labellings) is the same pair of launches with another
// second pass:
//   edit_back_kernel<K, NC>  the same walk, the same b.  A label state s = 2k + 1 carries ONE accumulator,
//                              accD += (alpha_{t-1}[s-1] + [k >= 1, y_{k-1} != y_{k+1} or no collapse] alpha_{t-1}[s-2]) * b_t[s+2]
//                            -- the alignments that step over label k --, a blank state s = 2g carries for each label c
//                              u_t(c)   = (u_{t+1}(c) [collapse] + b_{t+1}[s] + [c != y_g or no collapse] b_{t+1}[s+1]) * p[t][c]
//                                         the backward value of a label c standing in gap g, and
//                              accI(c) += (alpha_{t-1}[s] + [s >= 1, c != y_{g-1} or no collapse] alpha_{t-1}[s-1]) * u_t(c)
//                            When s leaves the window (or after row 0) the lane stores ln(acc) - ln P(y | x).
// A labelling one label shorter reaches a state a row earlier and may leave it a row later than y's own alignments do, so
// both launches relax window_k's two reachability cuts by two states (ScoreParams::slack); the band's window, and with it
// the number of slots, is what it was.  No alignment of y passes through such a cell, so a NaN or an infinity there must not
// reach y's own values: where nothing enters a cell outside the unrelaxed cuts (the sum is exactly 0) the posterior is not
// multiplied in (core_states); likewise u where nothing leaves the gap, and a term where nothing enters it.
//
// fcd_ctc_occupancy_* (the label occupancies of the labelling's own alignments, row by row) is post_fwd_kernel<K> at slack 0
// and a second walk, ctc_occ_walk below, compiled into post_back_kernel<K, 8> only and chosen by the wave-uniform
// PostParams::walk: b alone, no w, no accumulator that lives across rows.
#include <math.h>

#include <algorithm>

#include "ctc_lattice.h"

namespace fcd {
namespace {

// (kAlphaDown, the scale of the stored alpha: ctc_lattice.h)
constexpr int kTargetB = 60;     // b, w: row maximum in [2^59, 2^60)
constexpr int kAccDown = 40;     // a term (below 2^121) enters acc below 2^81: 2^46 rows sum below 2^127

struct PostParams {
    ScoreParams s;        // (s.logp is never null: the launcher lends scratch when the caller wants none)
    float *post;          // [labellings of this launch * stride * (N - 1)]                  (fcd_ctc_posterior_*)
    float *del, *ins;     // [.. * stride], [.. * (stride + 1) * (N - 1)]                     (fcd_ctc_edits_*)
    float *alpha;         // the stored forward rows, alpha_words per labelling of this launch
    int64_t alpha_words;
    int walk;             // what post_back_kernel<K, 8> walks (wave-uniform): kWalkSub, kWalkOcc
    // (fcd_ctc_occupancy_*) a (T, N) block per labelling of this launch, at row * occ_stride_row + t * occ_stride_t
    float *occ;
    int64_t occ_stride_row, occ_stride_t;
    float occ_scale;
    int occ_accumulate;
};
constexpr int kWalkSub = 0, kWalkOcc = 1;

// bit r: the lane's state r (the one >= lo) lies inside window_k's unrelaxed cuts -- a cell an alignment of y can pass
// through.  p.slack = 0: every live state.
template <int K>
__device__ __forceinline__ uint32_t core_states(const ScoreParams &p, const Row &rw, int lane, int t, int lo) {
    if (p.slack == 0) return ~0u;
    const int top = 2 * t + 1, bottom = 2 * rw.L - 2 * (rw.Tr - 1 - t) - 2;
    uint32_t m = 0;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = slot_state<K>(lane, r, lo);
        m |= (s <= top && s >= bottom ? 1u : 0u) << r;
    }
    return m;
}

// ---- pass 1: ctc_score's score_reg_kernel, storing what it computes ----
template <int K>
__global__ __launch_bounds__(64) void post_fwd_kernel(PostParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int C = 64 * K;
    const ScoreParams &p = q.s;
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    if (!prologue(p, lds, &rw)) return;
    const int lane = threadIdx.x;
    float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    int *ae = reinterpret_cast<int *>(am + (int64_t)p.in.T * C);
    float a[K];
#pragma unroll
    for (int r = 0; r < K; ++r) a[r] = 0.0f;
    if (lane == 0) a[0] = 1.0f;  // "row -1": all mass on state 0
    int64_t eacc = 0;
    int lo_prev = 0, lo = 0, hi = 0;
    for (int t0 = 0; t0 < rw.Tr; t0 += rw.rows_per_tile) {
        const int rc = min(rw.rows_per_tile, rw.Tr - t0);
        fill_tile(p, lds, rw, t0, rc);
        StepIn<K> in = load_step<K>(p, lds, rw, t0, 0);
        for (int i = 0; i < rc; ++i) {
            StepIn<K> nx = in;
            if (i + 1 < rc) nx = load_step<K>(p, lds, rw, t0 + i + 1, i + 1);
            lo = in.lo;
            hi = in.hi;
            if (hi - lo_prev >= C) {  // the window jumped: slots it re-enters start from 0
#pragma unroll
                for (int r = 0; r < K; ++r)
                    if (slot_state<K>(lane, r, lo_prev) <= hi - C) a[r] = 0.0f;
            }
            const float p1 = from_prev_lane(a[K - 1]), p2 = from_prev_lane(a[K - 2]);
            const uint32_t core = core_states<K>(p, rw, lane, t0 + i, lo);
            float u[K];
            int ex[K];
            int emax = kNoExp;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const float x1 = r >= 1 ? a[r - 1] : p1;
                const float x2 = r >= 2 ? a[r - 2] : (r == 1 ? p1 : p2);
                float sum;
                if (r & 1) {
                    sum = p.collapse ? a[r] + x1 : x1;
                    sum += ((in.skip_mask >> r) & 1) ? x2 : 0.0f;
                    u[r] = sum * in.pm[r / 2];
                    ex[r] = in.pe[r / 2];
                } else {
                    sum = a[r] + x1;
                    u[r] = sum * in.pm0;
                    ex[r] = in.pe0;
                }
                if (!((core >> r) & 1) && sum == 0.0f) u[r] = 0.0f;  // (nothing enters a cell y's alignments never see)
                const int e = finite_exp(u[r]);
                emax = max(emax, ((in.in_mask >> r) & 1) && e != kNoExp ? e + ex[r] : kNoExp);
            }
            emax = wave_imax(emax);
            const int sh = emax == kNoExp ? 0 : kTarget - emax;
            eacc -= sh;
            float *row = am + (int64_t)(t0 + i) * C + lane * K;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                a[r] = ((in.in_mask >> r) & 1) ? ldexpf(u[r], min(max(ex[r] + sh, -512), 512)) : 0.0f;
                if ((in.in_mask >> r) & 1) row[r] = ldexpf(a[r], -kAlphaDown);
            }
            if (lane == 0) ae[t0 + i] = (int)(eacc + kAlphaDown);
            lo_prev = lo;
            in = nx;
        }
    }
    if (lane == 0) lds.misc[18] = lds.misc[19] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = slot_state<K>(lane, r, lo);
        if (s <= hi && s == 2 * rw.L) lds.misc[18] = __float_as_int(a[r]);
        if (s <= hi && s == 2 * rw.L - 1) lds.misc[19] = __float_as_int(a[r]);
    }
    __syncthreads();
    if (lane == 0) {
        p.logp[blockIdx.x] = ln_p((double)__int_as_float(lds.misc[18]) + (double)__int_as_float(lds.misc[19]), eacc);
    }
}

// ---- pass 2 ----
// a labelling without a positive finite P(y | x): NaN for the labels the row holds
__device__ __forceinline__ void no_posterior(const PostParams &q) {
    const int64_t row = blockIdx.x, nc = q.s.in.N - 1;
    const int64_t n = min((int64_t)q.s.y.len[row], q.s.y.stride) * nc;
    for (int64_t e = threadIdx.x; e < n; e += blockDim.x) q.post[row * q.s.y.stride * nc + e] = NAN;
}

// every entry of the edit outputs the row owns -- k < min(len, stride), g <= min(len, stride) -- set to v
__device__ __forceinline__ void fill_edits(const PostParams &q, float v) {
    const int64_t row = blockIdx.x, nc = q.s.in.N - 1;
    const int64_t n = min((int64_t)q.s.y.len[row], q.s.y.stride);
    for (int64_t e = threadIdx.x; e < n; e += blockDim.x) q.del[row * q.s.y.stride + e] = v;
    for (int64_t e = threadIdx.x; e < (n + 1) * nc; e += blockDim.x) q.ins[row * (q.s.y.stride + 1) * nc + e] = v;
}

// ---- the backward walk's scaffolding: what post_back_kernel and edit_back_kernel do alike, written once.  The two kernels
// below keep their own loops and what a slot carries and flushes, so that their recurrences read side by side. ----
// the first row of the last tile: the tiles are walked from there down
__device__ __forceinline__ int last_tile(const Row &rw) { return (rw.Tr - 1) / rw.rows_per_tile * rw.rows_per_tile; }

// rows t0 .. t0 + rc staged, and k(t0 - 1) next to them: the window of the alpha row that row t0 reads
__device__ __forceinline__ void fill_back_tile(const ScoreParams &p, const Lds &lds, const Row &rw, int t0, int rc) {
    fill_tile(p, lds, rw, t0, rc);
    stage_krow_before(lds.misc, rw.path, rw.L, p.band, t0);
}

// "row T_r": all mass on state 2L
template <int K>
__device__ __forceinline__ void start_beyond_last_row(float (&b)[K], int lo, int L) {
#pragma unroll
    for (int r = 0; r < K; ++r) b[r] = slot_state<K>((int)threadIdx.x, r, lo) == 2 * L ? 1.0f : 0.0f;
}

// the posteriors of the labels 1 .. nc of the tile's row i, split (a label beyond nc reads the last one and is masked)
template <int NC>
__device__ __forceinline__ void label_posts(const Lds &lds, int at, int nc, float (&pmc)[NC], int (&pec)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        pmc[c] = lds.pm[at + min(c + 1, nc)];
        pec[c] = lds.pe[at + min(c + 1, nc)];
    }
}

// b_{t+1} of s, s + 1, s + 2, s the state of slot r: a state below row t + 1's window (lo_n) is not what its slot holds;
// n1, n2: the next lane's first two slots
struct Above {
    float y0, y1, y2;
};

template <int K>
__device__ __forceinline__ Above b_above(const float (&b)[K], int r, int s, int lo_n, float n1, float n2) {
    Above y;
    y.y0 = s >= lo_n ? b[r] : 0.0f;
    y.y1 = s + 1 >= lo_n ? (r + 1 < K ? b[r + 1 < K ? r + 1 : 0] : n1) : 0.0f;
    y.y2 = s + 2 >= lo_n ? (r + 2 < K ? b[r + 2 < K ? r + 2 : 0] : (r + 2 == K ? n1 : n2)) : 0.0f;
    return y;
}

// what the label state of label k passes down, before its posterior: b[s] [collapse] + b[s+1] + [y_{k+1} != y_k or no
// collapse] b[s+2]; inext: the labelling's word of label k + 1
__device__ __forceinline__ float label_state_sum(int collapse, const Above &y, int k, int L, int inext) {
    float sum = collapse ? y.y0 + y.y1 : y.y1;
    sum += (k + 1 < L && (!collapse || (inext & 0x100))) ? y.y2 : 0.0f;
    return sum;
}

// The row's scale: its largest b or w lands in [2^(kTargetB-1), 2^kTargetB).  Returns the shift; eb follows it, and x_t
// (alpha_{t-1}'s exponent on entry) becomes the exponent of this row's terms
__device__ __forceinline__ int back_row_shift(int emax, int64_t &eb, int64_t &x_t) {
    emax = wave_imax(emax);
    const int sh = emax == kNoExp ? 0 : kTargetB - emax;
    eb -= sh;
    x_t += eb;
    return sh;
}

// acc is kept at the largest X seen so far: where x_t exceeds it, rescale(d) brings the accumulators down by 2^d (d < 0)
template <class F>
__device__ __forceinline__ void raise_xmax(int64_t x_t, int64_t &xmax, bool &any, F rescale) {
    if (!any || x_t > xmax) {
        if (any) rescale((int)max(xmax - x_t, (int64_t)-512));
        xmax = x_t;
        any = true;
    }
}

// the power of two a term of this row enters acc by
__device__ __forceinline__ int term_shift(int64_t x_t, int64_t xmax) { return (int)max(x_t - xmax, (int64_t)-512) - kAccDown; }

// u * 2^(e + sh): a cell at the row's scale
__device__ __forceinline__ float at_row_scale(float u, int e, int sh) { return ldexpf(u, min(max(e + sh, -512), 512)); }

// ---- the label occupancies of the labelling's own alignments (fcd_ctc_occupancy_*; include/fcd.h) ----
// The second walk of post_back_kernel<K, 8>.  Row t = T_r - 1 .. 0, with b_{t+1} in the registers ("row T_r": all mass on
// state 2L) and alpha_t in the stored rows -- the row of the SAME index, so the window both are read by is row t's own and
// k(t - 1) is never asked for:
//   beta_t[s]  = b_{t+1}[s] [blank, or collapse] + b_{t+1}[s+1] + [allowed] b_{t+1}[s+2]     what the backward step sums
//   gamma_t[s] = alpha_t[s] * beta_t[s] / P                                                  before p[t][z[s]] enters
// one product, the exact power of two 2^(Ea(t) + Eb(t+1) - floor(log2 P)) and the division by P's mantissa -- two roundings;
// then b_t = beta_t * p[t][z[s]] in place at the row's own scale, as the substitution walk forms it.  A slot's parity is its
// state's (K is even): the even slots are the blank.  occ[t][c] is the sum of gamma_t over the states of label c: each lane
// adds up its own slots (at most K / 2 - 1 sums), wave_fsum the lanes (6 deep), once per label of the alphabet -- the same
// order in every call, so the same bits.  Every lane then holds the whole row; lane c stores cell c.  No LDS, no atomics.
// Where nothing leaves a cell (a dead end beside a band's jump: beta is exactly 0) neither the posterior nor alpha is
// multiplied in: no alignment of y reads them.
// The lattice the rows cannot hold.  alpha and b keep one exponent per row; where a long read does not support its
// labelling their maxima sit at opposite ends of the window and the cells that carry the probability fall out of range.
// The row's occupancies sum to 1 exactly; each is within (6 T_r + K / 2 + 11) 2^-24 of its value and the sum over the
// labels adds N - 1 <= 8 roundings, so a row whose sum is further than kOccLost(T_r) = 2 (6 T_r + K / 2 + 19) 2^-24 from 1
// has lost cells: the walk gives the labelling up -- logp = NaN and NaN in every row t < T_r of its block.
template <int K>
__device__ __forceinline__ void ctc_occ_walk(const PostParams &q, unsigned char *smem) {
    constexpr int C = 64 * K, NL = 9;  // (NL: the blank and the 8 labels)
    const ScoreParams &p = q.s;
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    if (!prologue(p, lds, &rw)) return;  // (the forward launch wrote this row's logp already; the same value again)
    const double lp = p.logp[blockIdx.x];
    if (lp - lp != 0.0) return;  // P = 0, or a NaN on the way: nothing of the block is written
    const int lane = threadIdx.x, N = rw.N, L = rw.L;
    const float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    const int *ae = reinterpret_cast<const int *>(am + (int64_t)p.in.T * C);
    float *out = q.occ + (int64_t)blockIdx.x * q.occ_stride_row;
    float b[K];
#pragma unroll
    for (int r = 0; r < K; ++r) b[r] = 0.0f;
    int64_t eb = 0;
    const int64_t xp = (int64_t)floor(lp * 1.44269504088896340735992468100189214);  // floor(log2 P(y | x))
    const float pman = (float)exp(lp - (double)xp * kLn2);                          // P / 2^xp, in [1, 2]
    const float lost = 2.0f * (6.0f * (float)rw.Tr + (float)(K / 2 + 19)) * 5.9604644775390625e-8f;  // kOccLost(T_r)
    bool first = true;
    int lo = 0, hi = 0, lo_n = 0;
    for (int t0 = last_tile(rw); t0 >= 0; t0 -= rw.rows_per_tile) {
        const int rc = min(rw.rows_per_tile, rw.Tr - t0);
        fill_tile(p, lds, rw, t0, rc);
        for (int i = rc - 1; i >= 0; --i) {
            const int t = t0 + i;
            window(p, lds, rw, t, i, &lo, &hi);
            if (first) {
                start_beyond_last_row<K>(b, lo, L);
                first = false;
                lo_n = lo;
            }
            const float *arow = am + (int64_t)t * C + lane * K;  // alpha_t, by slot (a slot outside the window is masked below)
            float av[K];
#pragma unroll
            for (int r = 0; r < K; ++r) av[r] = arow[r];
            // the exponent of this row's terms: alpha of row t times b of row t + 1, over 2^floor(log2 P)
            const int dt = (int)min(max((int64_t)ae[t] + eb - xp, (int64_t)-512), (int64_t)512);
            const float n1 = from_next_lane(b[0]), n2 = from_next_lane(b[1]);
            const float pm0 = lds.pm[i * N];
            const int pe0 = lds.pe[i * N];
            float u[K], g[K];
            int ex[K], yk[K / 2];
            uint32_t live = 0;
            int emax = kNoExp;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int s = slot_state<K>(lane, r, lo);
                const bool in = s <= hi;
                live |= (in ? 1u : 0u) << r;
                const Above y = b_above<K>(b, r, s, lo_n, n1, n2);
                float sum, pm;
                if (r & 1) {
                    const int k = in ? (s >> 1) : 0;  // (a dead slot reads valid addresses and is masked below)
                    const int info = lds.lab[k], inext = lds.lab[min(k + 1, max(L - 1, 0))];
                    yk[r / 2] = in ? (info & 0xFF) : 0;
                    sum = label_state_sum(p.collapse, y, k, L, inext);
                    pm = lds.pm[i * N + yk[r / 2]];
                    ex[r] = lds.pe[i * N + yk[r / 2]];
                } else {
                    sum = y.y0 + y.y1;
                    pm = pm0;
                    ex[r] = pe0;
                }
                const bool leaves = in && sum != 0.0f;
                u[r] = leaves ? sum * pm : 0.0f;
                g[r] = leaves ? ldexpf(av[r] * sum, dt) / pman : 0.0f;
                const int e = finite_exp(u[r]);
                emax = max(emax, e != kNoExp ? e + ex[r] : kNoExp);
            }
            int64_t unused = 0;
            const int sh = back_row_shift(emax, eb, unused);
#pragma unroll
            for (int r = 0; r < K; ++r) b[r] = ((live >> r) & 1) ? at_row_scale(u[r], ex[r], sh) : 0.0f;
            // ---- the row's N occupancies, the same in every lane ----
            float v[NL];
            {
                float x = g[0];
#pragma unroll
                for (int r = 2; r < K; r += 2) x += g[r];
                v[0] = wave_fsum(x);
            }
            float mass = v[0];
#pragma unroll
            for (int c = 1; c < NL; ++c) {
                v[c] = 0.0f;
                if (c < N) {  // (wave-uniform)
                    float x = yk[0] == c ? g[1] : 0.0f;
#pragma unroll
                    for (int r = 3; r < K; r += 2) x += yk[r / 2] == c ? g[r] : 0.0f;
                    v[c] = wave_fsum(x);
                    mass += v[c];
                }
            }
            if (!(fabsf(mass - 1.0f) <= lost)) {  // (wave-uniform) the rows cannot hold this lattice
                __syncthreads();  // the rows stored so far are behind the NaN that replaces them
                for (int tt = 0; tt < rw.Tr; ++tt)
                    if (lane < N) out[(int64_t)tt * q.occ_stride_t + lane] = NAN;
                if (lane == 0) p.logp[blockIdx.x] = (double)NAN;
                return;
            }
            float mine = v[0];
#pragma unroll
            for (int c = 1; c < NL; ++c) mine = lane == c ? v[c] : mine;
            if (lane < N) {
                float *cell = out + (int64_t)t * q.occ_stride_t + lane;
                if (!q.occ_accumulate) *cell = mine == 0.0f ? 0.0f : q.occ_scale * mine;
                else if (mine != 0.0f) *cell = *cell + q.occ_scale * mine;  // (a cell of occupancy 0 is not read)
            }
            lo_n = lo;
        }
    }
}

template <int K, int NC>
__global__ __launch_bounds__(64) void post_back_kernel(PostParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (NC == 8) {  // (the occupancy walk rides in these four only)
        if (q.walk == kWalkOcc) return ctc_occ_walk<K>(q, smem);
    }
    constexpr int C = 64 * K, H = K / 2;
    const ScoreParams &p = q.s;
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    if (!prologue(p, lds, &rw)) {  // (the forward launch wrote this row's logp already; the same value again)
        no_posterior(q);
        return;
    }
    const double lp = p.logp[blockIdx.x];
    if (lp - lp != 0.0) {  // P = 0, or a NaN on the way
        no_posterior(q);
        return;
    }
    if (rw.L == 0) return;
    const int lane = threadIdx.x, nc = rw.N - 1, L = rw.L;
    const float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    const int *ae = reinterpret_cast<const int *>(am + (int64_t)p.in.T * C);
    float *post = q.post + (int64_t)blockIdx.x * p.y.stride * nc;
    float b[K], w[H][NC], acc[H][NC];
#pragma unroll
    for (int r = 0; r < K; ++r) b[r] = 0.0f;
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
        for (int c = 0; c < NC; ++c) w[h][c] = acc[h][c] = 0.0f;
    int64_t eb = 0, xmax = 0;
    bool first = true, any = false;
    int lo = 0, hi = 0, lo_n = 0, hi_n = 0;
    for (int t0 = last_tile(rw); t0 >= 0; t0 -= rw.rows_per_tile) {
        const int rc = min(rw.rows_per_tile, rw.Tr - t0);
        fill_back_tile(p, lds, rw, t0, rc);
        for (int i = rc - 1; i >= 0; --i) {
            const int t = t0 + i;
            window(p, lds, rw, t, i, &lo, &hi);
            // alpha_{t-1}, by slot; row -1: all mass on state 0, exponent 0
            int lo_p = 0, hi_p = 0;
            float av[K];
            int64_t x_t = 0;
            if (t > 0) {
                window_k(p, rw, t - 1, krow_before(lds.krow, lds.misc, p.band, i), &lo_p, &hi_p);
                const float *row = am + (int64_t)(t - 1) * C + lane * K;
#pragma unroll
                for (int r = 0; r < K; ++r) av[r] = slot_state<K>(lane, r, lo_p) <= hi_p ? row[r] : 0.0f;
                x_t = ae[t - 1];
            } else {
#pragma unroll
                for (int r = 0; r < K; ++r) av[r] = (lane == 0 && r == 0) ? 1.0f : 0.0f;
            }
            const float av_prev = from_prev_lane(av[K - 1]);
            if (first) {
                start_beyond_last_row<K>(b, lo, L);
                first = false;
                lo_n = lo;
            } else {  // the label states that were live at row t + 1 and are not at row t: their labels are complete
#pragma unroll
                for (int r = 1; r < K; r += 2) {
                    const int s = slot_state<K>(lane, r, lo_n);
                    if (s > hi) {  // (b stays: row t still reads b_{t+1} of the states above its window)
                        if (s <= hi_n) store_post<NC>(post, s >> 1, nc, acc[r / 2]);
#pragma unroll
                        for (int c = 0; c < NC; ++c) w[r / 2][c] = acc[r / 2][c] = 0.0f;
                    }
                }
            }
            const float n1 = from_next_lane(b[0]), n2 = from_next_lane(b[1]);
            const float pm0 = lds.pm[i * rw.N];
            const int pe0 = lds.pe[i * rw.N];
            float pmc[NC];
            int pec[NC];
            label_posts<NC>(lds, i * rw.N, nc, pmc, pec);
            float u[K], uw[H][NC], e1[H], e2[H];
            int ex[K], yprev[H];
            uint32_t live = 0;
            int emax = kNoExp;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int s = slot_state<K>(lane, r, lo);
                const bool in = s <= hi;
                live |= (in ? 1u : 0u) << r;
                const Above y = b_above<K>(b, r, s, lo_n, n1, n2);
                if (r & 1) {
                    const int h = r / 2, k = in ? (s >> 1) : 0;  // (a dead slot reads valid addresses and is masked below)
                    const int info = lds.lab[k], inext = lds.lab[min(k + 1, L - 1)], iprev = lds.lab[max(k - 1, 0)];
                    const int yk = in ? (info & 0xFF) : 0;
                    const int ynext = k + 1 < L ? (inext & 0xFF) : 0;  // (0: no label c equals it)
                    yprev[h] = k > 0 ? (iprev & 0xFF) : 0;
                    u[r] = label_state_sum(p.collapse, y, k, L, inext) * lds.pm[i * rw.N + yk];
                    ex[r] = lds.pe[i * rw.N + yk];
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        float exit = p.collapse ? w[h][c] + y.y1 : y.y1;
                        exit += (p.collapse && c + 1 == ynext) ? 0.0f : y.y2;  // (b[s + 2] is 0 beyond state 2L)
                        uw[h][c] = exit * pmc[c];
                        const int e = finite_exp(uw[h][c]);
                        emax = max(emax, in && c < nc && e != kNoExp ? e + pec[c] : kNoExp);
                    }
                    // what enters state s from row t - 1 (a state above that row's window is not in its slot)
                    const float x1 = av[r >= 1 ? r - 1 : 0], x2 = r >= 2 ? av[r - 2] : av_prev;
                    e1[h] = (in && s - 1 <= hi_p) ? x1 : 0.0f;
                    e2[h] = (in && s >= 3 && s - 2 <= hi_p) ? x2 : 0.0f;
                } else {
                    u[r] = (y.y0 + y.y1) * pm0;
                    ex[r] = pe0;
                }
                const int e = finite_exp(u[r]);
                emax = max(emax, in && e != kNoExp ? e + ex[r] : kNoExp);
            }
            const int sh = back_row_shift(emax, eb, x_t);
            raise_xmax(x_t, xmax, any, [&](int d) {
#pragma unroll
                for (int h = 0; h < H; ++h)
#pragma unroll
                    for (int c = 0; c < NC; ++c) acc[h][c] = ldexpf(acc[h][c], d);
            });
            const int dt = term_shift(x_t, xmax);
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const bool in = (live >> r) & 1;
                b[r] = in ? at_row_scale(u[r], ex[r], sh) : 0.0f;
                if (r & 1) {
                    const int h = r / 2;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        w[h][c] = (in && c < nc) ? at_row_scale(uw[h][c], pec[c], sh) : 0.0f;
                        const float entry = e1[h] + ((p.collapse && c + 1 == yprev[h]) ? 0.0f : e2[h]);
                        const float term = entry * w[h][c];
                        acc[h][c] += ldexpf(term, dt);
                    }
                }
            }
            lo_n = lo;
            hi_n = hi;
        }
    }
    // the labels whose state is live at row 0
#pragma unroll
    for (int r = 1; r < K; r += 2) {
        const int s = slot_state<K>(lane, r, lo);
        if (s <= hi) store_post<NC>(post, s >> 1, nc, acc[r / 2]);
    }
}

// ---- pass 2 of fcd_ctc_edits_* ----
template <int NC>
__device__ __forceinline__ void store_ins(float *ins, int g, int nc, const float (&acc)[NC], int64_t e, double lp) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (c < nc) ins[(int64_t)g * nc + c] = log_ratio(acc[c], e, lp);
}

template <int K, int NC>
__global__ __launch_bounds__(64) void edit_back_kernel(PostParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int C = 64 * K, H = K / 2;
    const ScoreParams &p = q.s;
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    const bool walk = prologue(p, lds, &rw);  // (the forward launch wrote this row's logp already; the same value again)
    const double lp = p.logp[blockIdx.x];
    if (lp - lp != 0.0) {  // P = 0, a NaN on the way, or not a labelling
        fill_edits(q, NAN);
        return;
    }
    fill_edits(q, -INFINITY);  // an edit no row carries has probability 0
    if (!walk) return;         // (T_r = 0 and L = 0: P(y | x) = 1, and no insertion has an alignment)
    __syncthreads();           // the fill is in place before another lane's flush writes over it
    const int lane = threadIdx.x, nc = rw.N - 1, L = rw.L, Lm = max(L - 1, 0);
    const float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    const int *ae = reinterpret_cast<const int *>(am + (int64_t)p.in.T * C);
    float *del = q.del + (int64_t)blockIdx.x * p.y.stride;
    float *ins = q.ins + (int64_t)blockIdx.x * (p.y.stride + 1) * nc;
    float b[K], u[H][NC], accI[H][NC], accD[H];
#pragma unroll
    for (int r = 0; r < K; ++r) b[r] = 0.0f;
#pragma unroll
    for (int h = 0; h < H; ++h) {
        accD[h] = 0.0f;
#pragma unroll
        for (int c = 0; c < NC; ++c) u[h][c] = accI[h][c] = 0.0f;
    }
    int64_t eb = 0, xmax = 0;
    bool first = true, any = false;
    int lo = 0, hi = 0, lo_n = 0, hi_n = 0;
    for (int t0 = last_tile(rw); t0 >= 0; t0 -= rw.rows_per_tile) {
        const int rc = min(rw.rows_per_tile, rw.Tr - t0);
        fill_back_tile(p, lds, rw, t0, rc);
        for (int i = rc - 1; i >= 0; --i) {
            const int t = t0 + i;
            window(p, lds, rw, t, i, &lo, &hi);
            // alpha_{t-1}, by slot; row -1: all mass on state 0, exponent 0
            int lo_p = 0, hi_p = 0;
            float av[K];
            int64_t x_t = 0;
            if (t > 0) {
                window_k(p, rw, t - 1, krow_before(lds.krow, lds.misc, p.band, i), &lo_p, &hi_p);
                const float *row = am + (int64_t)(t - 1) * C + lane * K;
#pragma unroll
                for (int r = 0; r < K; ++r) av[r] = slot_state<K>(lane, r, lo_p) <= hi_p ? row[r] : 0.0f;
                x_t = ae[t - 1];
            } else {
#pragma unroll
                for (int r = 0; r < K; ++r) av[r] = (lane == 0 && r == 0) ? 1.0f : 0.0f;
            }
            const float av_prev = from_prev_lane(av[K - 1]);
            if (first) {
                start_beyond_last_row<K>(b, lo, L);
                first = false;
                lo_n = lo;
                // the last label's deletion: the two final states of the shortened labelling, off the last forward row
                if (lane == 0 && L >= 1) {
                    const float *row = am + (int64_t)t * C;
                    float v = 0.0f;
                    if (2 * L - 1 >= lo && 2 * L - 1 <= hi) {
                        if (2 * L - 2 >= lo) v = row[(2 * L - 2) % C];
                        if (L >= 2 && 2 * L - 3 >= lo) v += row[(2 * L - 3) % C];
                    }
                    del[L - 1] = log_ratio(v, ae[t], lp);
                }
            } else {  // the states that were live at row t + 1 and are not at row t: their edits are complete
#pragma unroll
                for (int r = 0; r < K; ++r) {
                    const int s = slot_state<K>(lane, r, lo_n), h = r / 2;
                    if (s > hi) {  // (b stays: row t still reads b_{t+1} of the states above its window)
                        if (r & 1) {
                            if (s <= hi_n && (s >> 1) != L - 1) del[s >> 1] = log_ratio(accD[h], xmax + kAccDown, lp);
                            accD[h] = 0.0f;
                        } else {
                            if (s <= hi_n) store_ins<NC>(ins, s >> 1, nc, accI[h], xmax + kAccDown, lp);
#pragma unroll
                            for (int c = 0; c < NC; ++c) u[h][c] = accI[h][c] = 0.0f;
                        }
                    }
                }
            }
            const float n1 = from_next_lane(b[0]), n2 = from_next_lane(b[1]);
            const float pm0 = lds.pm[i * rw.N];
            const int pe0 = lds.pe[i * rw.N];
            float pmc[NC];
            int pec[NC];
            label_posts<NC>(lds, i * rw.N, nc, pmc, pec);
            const uint32_t core = core_states<K>(p, rw, lane, t, lo);
            float ub[K], uu[H][NC], eD[H], e1[H], e2[H];
            int ex[K], yprev[H];
            uint32_t live = 0;
            int emax = kNoExp;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const int s = slot_state<K>(lane, r, lo), h = r / 2;
                const bool in = s <= hi;
                live |= (in ? 1u : 0u) << r;
                const Above y = b_above<K>(b, r, s, lo_n, n1, n2);
                if (r & 1) {
                    const int k = in ? (s >> 1) : 0;  // (a dead slot reads valid addresses and is masked below)
                    const int info = lds.lab[k], inext = lds.lab[min(k + 1, Lm)], iprev = lds.lab[max(k - 1, 0)];
                    const int yk = in ? (info & 0xFF) : 0;
                    const float sum = label_state_sum(p.collapse, y, k, L, inext);
                    ub[r] = (!((core >> r) & 1) && sum == 0.0f) ? 0.0f : sum * lds.pm[i * rw.N + yk];
                    ex[r] = lds.pe[i * rw.N + yk];
                    // what steps over label k from row t - 1 (a state above that row's window is not in its slot)
                    const float x1 = av[r >= 1 ? r - 1 : 0], x2 = r >= 2 ? av[r - 2] : av_prev;
                    const bool skip = k >= 1 && k + 1 < L && (!p.collapse || ((iprev ^ inext) & 0xFF));
                    eD[h] = ((in && s - 1 <= hi_p) ? x1 : 0.0f) + ((in && skip && s - 2 <= hi_p) ? x2 : 0.0f);
                } else {
                    ub[r] = (!((core >> r) & 1) && y.y0 + y.y1 == 0.0f) ? 0.0f : (y.y0 + y.y1) * pm0;
                    ex[r] = pe0;
                    const int g = in ? (s >> 1) : 0;
                    const int ynext = g < L ? (lds.lab[min(g, Lm)] & 0xFF) : 0;  // (0: no label c equals it)
                    yprev[h] = g > 0 ? (lds.lab[min(g - 1, Lm)] & 0xFF) : 0;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        float exit = p.collapse ? u[h][c] + y.y0 : y.y0;
                        exit += (p.collapse && c + 1 == ynext) ? 0.0f : y.y1;  // (b[s + 1] is 0 beyond state 2L)
                        uu[h][c] = exit == 0.0f ? 0.0f : exit * pmc[c];  // (nothing leaves the gap: no alignment reads p[t][c])
                        const int e = finite_exp(uu[h][c]);
                        emax = max(emax, in && c < nc && e != kNoExp ? e + pec[c] : kNoExp);
                    }
                    // what enters the gap from row t - 1
                    const float x0 = av[r], x1 = r >= 1 ? av[r - 1] : av_prev;
                    e1[h] = (in && s <= hi_p) ? x0 : 0.0f;
                    e2[h] = (in && s >= 1 && s - 1 <= hi_p) ? x1 : 0.0f;
                }
                const int e = finite_exp(ub[r]);
                emax = max(emax, in && e != kNoExp ? e + ex[r] : kNoExp);
            }
            const int sh = back_row_shift(emax, eb, x_t);
            raise_xmax(x_t, xmax, any, [&](int d) {
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    accD[h] = ldexpf(accD[h], d);
#pragma unroll
                    for (int c = 0; c < NC; ++c) accI[h][c] = ldexpf(accI[h][c], d);
                }
            });
            const int dt = term_shift(x_t, xmax);
#pragma unroll
            for (int r = 0; r < K; ++r) b[r] = ((live >> r) & 1) ? at_row_scale(ub[r], ex[r], sh) : 0.0f;
            const float m1 = from_next_lane(b[1]);  // b_t of the next lane's first label state
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const bool in = (live >> (2 * h)) & 1;
                const float above = 2 * h + 3 < K ? b[min(2 * h + 3, K - 1)] : m1;  // b_t[s + 2] of the pair's label state s
                accD[h] += eD[h] == 0.0f ? 0.0f : ldexpf(eD[h] * above, dt);  // (nothing enters: no alignment, whatever lies above)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    u[h][c] = (in && c < nc) ? at_row_scale(uu[h][c], pec[c], sh) : 0.0f;
                    const float entry = e1[h] + ((p.collapse && c + 1 == yprev[h]) ? 0.0f : e2[h]);
                    accI[h][c] += entry == 0.0f ? 0.0f : ldexpf(entry * u[h][c], dt);
                }
            }
            lo_n = lo;
            hi_n = hi;
        }
    }
    // the states that are live at row 0
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = slot_state<K>(lane, r, lo), h = r / 2;
        if (s > hi) continue;
        if (r & 1) {
            if ((s >> 1) != L - 1) del[s >> 1] = log_ratio(accD[h], xmax + kAccDown, lp);
        } else {
            store_ins<NC>(ins, s >> 1, nc, accI[h], xmax + kAccDown, lp);
        }
    }
}

int reg_states_per_lane(int64_t T, int64_t stride, int64_t band) {  // 0: the window does not fit the registers
    const int64_t states = ctc_score_window_states(T, stride, band);
    return states + 2 <= 128 ? 2 : (states + 2 <= 256 ? 4 : (states + 2 <= 384 ? 6 : (states + 2 <= 512 ? 8 : 0)));
}

}  // namespace

// 0 = the kernels hold the call; 1 = the widest window exceeds the 510 register-resident states; 2 = more than 8 labels;
// 3 = the labelling's LDS copy and the tile exceed the 64 KiB a launch gets without asking for more
int ctc_posterior_unsupported(int64_t T, int64_t stride, int64_t band, int64_t N) {
    if (reg_states_per_lane(T, stride, band) == 0) return 1;
    if (N - 1 > 8) return 2;
    return lds_bytes((int)std::max<int64_t>(std::min<int64_t>(std::min(T, stride), 1 << 20), 1), 0) > 64 * 1024 ? 3 : 0;
}

// stored forward rows of one labelling (every one of a call has T rows' worth): T * 64K cells, then T exponent words
size_t ctc_posterior_row_bytes(int64_t T, int64_t stride, int64_t band) {
    const size_t k = (size_t)reg_states_per_lane(T, stride, band);
    return stored_rows_bytes(T, k);
}

namespace {
PostParams post_params(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, double *logp, unsigned char *alpha) {
    PostParams q;
    q.s.in = in;
    q.s.y = y;
    q.s.collapse = collapse;
    q.s.band = (int)band;
    q.s.logp = logp;
    q.s.cap = 0;
    q.s.lab_cap = (int)std::max<int64_t>(std::min(in.T, y.stride), 1);
    q.post = q.del = q.ins = nullptr;
    q.walk = kWalkSub;
    q.occ = nullptr;
    q.occ_stride_row = q.occ_stride_t = 0;
    q.occ_scale = 0.0f;
    q.occ_accumulate = 0;
    q.alpha = reinterpret_cast<float *>(alpha);
    q.alpha_words = (int64_t)(ctc_posterior_row_bytes(in.T, y.stride, band) / 4);
    return q;
}

// the forward launch, then the backward one: EDIT picks the kernel, the window K, the alphabet NC
template <bool EDIT, int K>
void launch_pair(const PostParams &q, dim3 grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL(post_fwd_kernel<K>, grid, dim3(64), lds, stream, q);
    if constexpr (EDIT) {
        if (q.s.in.N - 1 <= 4) hipLaunchKernelGGL((edit_back_kernel<K, 4>), grid, dim3(64), lds, stream, q);
        else hipLaunchKernelGGL((edit_back_kernel<K, 8>), grid, dim3(64), lds, stream, q);
    } else {
        if (q.s.in.N - 1 <= 4) hipLaunchKernelGGL((post_back_kernel<K, 4>), grid, dim3(64), lds, stream, q);
        else hipLaunchKernelGGL((post_back_kernel<K, 8>), grid, dim3(64), lds, stream, q);
    }
}

// fcd_ctc_occupancy_*: the forward launch, then the occupancy walk in post_back_kernel<K, 8> whatever the alphabet
template <int K>
void launch_occupancy_pair(const PostParams &q, dim3 grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL(post_fwd_kernel<K>, grid, dim3(64), lds, stream, q);
    hipLaunchKernelGGL((post_back_kernel<K, 8>), grid, dim3(64), lds, stream, q);
}

template <bool EDIT>
hipError_t launch_walks(const PostParams &q, int64_t band, hipStream_t stream) {
    const dim3 grid((unsigned)(q.s.in.n_reads * q.s.y.n_hyp));
    const size_t lds = lds_bytes(q.s.lab_cap, 0);
    switch (reg_states_per_lane(q.s.in.T, q.s.y.stride, band)) {
    case 2: launch_pair<EDIT, 2>(q, grid, lds, stream); break;
    case 4: launch_pair<EDIT, 4>(q, grid, lds, stream); break;
    case 6: launch_pair<EDIT, 6>(q, grid, lds, stream); break;
    case 8: launch_pair<EDIT, 8>(q, grid, lds, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
}  // namespace

hipError_t launch_ctc_posterior(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, float *post,
                                double *logp, unsigned char *alpha, hipStream_t stream) {
    if (in.n_reads * y.n_hyp <= 0) return hipSuccess;
    PostParams q = post_params(in, y, collapse, band, logp, alpha);
    q.post = post;
    return launch_walks<false>(q, band, stream);
}

hipError_t launch_ctc_edits(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, float *deletion,
                            float *insertion, double *logp, unsigned char *alpha, hipStream_t stream) {
    if (in.n_reads * y.n_hyp <= 0) return hipSuccess;
    PostParams q = post_params(in, y, collapse, band, logp, alpha);
    q.s.slack = 2;  // (both launches: the stored forward rows hold the two states more that a deletion reads)
    q.del = deletion;
    q.ins = insertion;
    return launch_walks<true>(q, band, stream);
}

hipError_t launch_ctc_occupancy(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, const OccupancyDesc &out,
                                double *logp, unsigned char *alpha, hipStream_t stream) {
    if (in.n_reads * y.n_hyp <= 0) return hipSuccess;
    PostParams q = post_params(in, y, collapse, band, logp, alpha);
    q.walk = kWalkOcc;
    q.occ = out.occ;
    q.occ_stride_row = out.stride_row;
    q.occ_stride_t = out.stride_t;
    q.occ_scale = out.scale;
    q.occ_accumulate = out.accumulate;
    const dim3 grid((unsigned)(in.n_reads * y.n_hyp));
    const size_t lds = lds_bytes(q.s.lab_cap, 0);
    switch (reg_states_per_lane(in.T, y.stride, band)) {
    case 2: launch_occupancy_pair<2>(q, grid, lds, stream); break;
    case 4: launch_occupancy_pair<4>(q, grid, lds, stream); break;
    case 6: launch_occupancy_pair<6>(q, grid, lds, stream); break;
    case 8: launch_occupancy_pair<8>(q, grid, lds, stream); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace fcd
