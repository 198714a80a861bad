// ctc_score.hip -- CTC forward log-likelihood ln P(y | x) of given labellings (fcd_ctc_score_*; include/fcd.h).
// NOT a reference function: the unpruned, unmerged sum of the recurrences the beam search walks (src/search.rs:186-241).
//
// One workgroup per (read, hypothesis) row walks the T_r rows of the read over the LIVE WINDOW of the extended
// sequence z (blank, y0, blank, y1, ..., blank; 2L + 1 states): the band around the decoded path (band > 0), cut to the
// states that can be reached from the start and can still reach the end (which changes no result).
//
// Numerics.  alpha stays in f32 probability space and is kept as  alpha = a * 2^Eacc  with ONE integer exponent per row
// of the lattice.  A posterior p is split once, when its tile is staged, into mantissa pm in [0.5, 1) and exponent pe;
// a cell is  u = (a[s] + a[s-1] + a[s-2]) * pm  (at most three f32 roundings), its true exponent is exp(u) + pe, the
// row's largest such exponent Emax is reduced as an INTEGER, and the cell is stored as ldexp(u, pe - Emax + kTarget):
// powers of two only, exact; the row maximum lands in [2^(kTarget-1), 2^kTarget) every step, whatever the posteriors'
// magnitude.  A cell below 2^-(kTarget+126) = 2^-246 of its row's maximum leaves the normal range and may be rounded or
// dropped (the contract allows that below 2^-160).  The final value ln(m) + Eacc * ln 2 is formed in float64.  No
// logarithm per step.
//
// Two kernels, one step:
//   score_reg_kernel<K>  windows of up to 64 * K - 2 states: one wavefront, K consecutive states per lane in registers
//                        (state s lives in slot s mod 64K: the window slides through the slots), the s-1 / s-2
//                        neighbours of a lane's first two states by two wave rotations, Emax by a DPP reduction.
//   score_lds_kernel     wider windows: alpha double-buffered in LDS (circular), up to 1024 work-items.
// Both stage the posteriors kTileRows rows at a time in LDS (split into pm / pe), next to the labelling (u16 per label:
// label | "differs from its predecessor" << 8) and, banded, the label count k(t) of every row of the tile.
#include <math.h>

#include <algorithm>

#include "ctc_lattice.h"

namespace fcd {
namespace {

__device__ __forceinline__ void write_result(const ScoreParams &p, float c0, float c1, int64_t eacc) {
    p.logp[blockIdx.x] = ln_p((double)c0 + (double)c1, eacc);
}

// ---- the register-resident window ----
template <int K>
__global__ __launch_bounds__(64) void score_reg_kernel(ScoreParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int C = 64 * K;
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    if (!prologue(p, lds, &rw)) return;
    const int lane = threadIdx.x;
    float a[K];  // alpha of the lane's K states, scaled by 2^-eacc
#pragma unroll
    for (int r = 0; r < K; ++r) a[r] = 0.0f;
    if (lane == 0) a[0] = 1.0f;  // "row -1": all mass on state 0, so that row 0 comes out as p[0][0], p[0][y0]
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
            if (hi - lo_prev >= C) {  // the window jumped (several labels on one row): slots it re-enters start from 0
#pragma unroll
                for (int r = 0; r < K; ++r)
                    if (slot_state<K>(lane, r, lo_prev) <= hi - C) a[r] = 0.0f;
            }
            const float p1 = from_prev_lane(a[K - 1]), p2 = from_prev_lane(a[K - 2]);
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
                const int e = finite_exp(u[r]);
                emax = max(emax, ((in.in_mask >> r) & 1) && e != kNoExp ? e + ex[r] : kNoExp);
            }
            emax = wave_imax(emax);
            const int sh = emax == kNoExp ? 0 : kTarget - emax;
            eacc -= sh;
#pragma unroll
            for (int r = 0; r < K; ++r)
                a[r] = ((in.in_mask >> r) & 1) ? ldexpf(u[r], min(max(ex[r] + sh, -512), 512)) : 0.0f;
            lo_prev = lo;
            in = nx;
        }
    }
    // P = alpha[2L] + alpha[2L - 1] of the last row, where they lie in its window
    if (lane == 0) lds.misc[18] = lds.misc[19] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = slot_state<K>(lane, r, lo);
        if (s <= hi && s == 2 * rw.L) lds.misc[18] = __float_as_int(a[r]);
        if (s <= hi && s == 2 * rw.L - 1) lds.misc[19] = __float_as_int(a[r]);
    }
    __syncthreads();
    if (lane == 0) write_result(p, __int_as_float(lds.misc[18]), __int_as_float(lds.misc[19]), eacc);
}

// ---- the LDS-resident window ----
__global__ __launch_bounds__(1024) void score_lds_kernel(ScoreParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    if (!prologue(p, lds, &rw)) return;
    const int tid = threadIdx.x, bd = blockDim.x, cap = p.cap, nw = bd >> 6;
    for (int s = tid; s < 2 * cap; s += bd) lds.alpha[s] = 0.0f;
    __syncthreads();
    if (tid == 0) lds.alpha[0] = 1.0f;  // "row -1": all mass on state 0
    int64_t eacc = 0;
    int lo_prev = 0, hi_prev = 0, base = 0, which = 0;  // base: the multiple of cap at or below the window's start
    // alpha_{t-1}[n] as the previous row left it: 0 outside that row's window (state n lives at n mod cap)
    auto rd = [&](const float *buf, int n) -> float {
        if (n < lo_prev || n > hi_prev) return 0.0f;
        int idx = n - base;
        idx = idx < 0 ? idx + cap : (idx >= cap ? idx - cap : idx);
        return buf[idx];
    };
    for (int t0 = 0; t0 < rw.Tr; t0 += rw.rows_per_tile) {
        const int rc = min(rw.rows_per_tile, rw.Tr - t0);
        fill_tile(p, lds, rw, t0, rc);
        for (int i = 0; i < rc; ++i) {
            int lo, hi;
            window(p, lds, rw, t0 + i, i, &lo, &hi);
            const float *prev = lds.alpha + which * cap;
            float *next = lds.alpha + (which ^ 1) * cap;
            const float pm0 = lds.pm[i * rw.N];
            const int pe0 = lds.pe[i * rw.N];
            float u[kLdsCells];
            int ex[kLdsCells];
            int emax = kNoExp;
#pragma unroll
            for (int c = 0; c < kLdsCells; ++c) {
                const int s = lo + tid + c * bd;
                u[c] = 0.0f;
                ex[c] = 0;
                if (s <= hi) {
                    const float x0 = rd(prev, s), x1 = rd(prev, s - 1);
                    if (s & 1) {
                        const int info = lds.lab[s >> 1];
                        float sum = p.collapse ? x0 + x1 : x1;
                        if (s >= 3 && (!p.collapse || (info & 0x100))) sum += rd(prev, s - 2);
                        u[c] = sum * lds.pm[i * rw.N + (info & 0xFF)];
                        ex[c] = lds.pe[i * rw.N + (info & 0xFF)];
                    } else {
                        u[c] = (x0 + x1) * pm0;
                        ex[c] = pe0;
                    }
                    const int e = finite_exp(u[c]);
                    emax = max(emax, e != kNoExp ? e + ex[c] : kNoExp);
                }
            }
            emax = wave_imax(emax);
            if ((tid & 63) == 0) lds.misc[tid >> 6] = emax;
            __syncthreads();  // every read of `prev` is done, the waves' maxima are in place
            for (int w = 0; w < nw; ++w) emax = max(emax, lds.misc[w]);
            const int sh = emax == kNoExp ? 0 : kTarget - emax;
            eacc -= sh;
            while (lo >= base + cap) base += cap;
#pragma unroll
            for (int c = 0; c < kLdsCells; ++c) {
                const int s = lo + tid + c * bd;
                if (s <= hi) {
                    int idx = s - base;
                    idx = idx >= cap ? idx - cap : idx;
                    next[idx] = ldexpf(u[c], min(max(ex[c] + sh, -512), 512));
                }
            }
            lo_prev = lo;
            hi_prev = hi;
            which ^= 1;
            __syncthreads();
        }
    }
    if (tid == 0) {
        const float *last = lds.alpha + which * cap;
        write_result(p, rd(last, 2 * rw.L), rd(last, 2 * rw.L - 1), eacc);
    }
}

}  // namespace

// The most states a window of this call can hold: what the host knows without reading a labelling.
int64_t ctc_score_window_states(int64_t T, int64_t stride, int64_t band) {
    const int64_t exact = 2 * std::min(T, stride) + 1;
    return band > 0 ? std::min(exact, 4 * band + 3) : exact;
}

bool ctc_score_supported(int64_t T, int64_t stride, int64_t band) {
    const int64_t states = ctc_score_window_states(T, stride, band);
    const int64_t lab_cap = std::max<int64_t>(std::min(T, stride), 1);
    const int64_t cap = states + 2 <= 512 ? 0 : states;  // (register-resident windows keep no alpha in LDS)
    return lab_cap <= 80 * 1024 && cap <= 1024 * kLdsCells && lds_bytes((int)lab_cap, (int)cap) <= 160 * 1024;
}

hipError_t launch_ctc_score(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, double *logp,
                            hipStream_t stream) {
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    ScoreParams p;
    p.in = in;
    p.y = y;
    p.collapse = collapse;
    p.band = (int)band;
    p.logp = logp;
    p.lab_cap = (int)std::max<int64_t>(std::min(in.T, y.stride), 1);
    const int64_t states = ctc_score_window_states(in.T, y.stride, band);
    const dim3 grid((unsigned)rows);
    if (states + 2 <= 512) {  // the slots must exceed the widest window by two states (the s-1 / s-2 reads below it)
        p.cap = 0;
        const size_t lds = lds_bytes(p.lab_cap, 0);
        if (states + 2 <= 128) hipLaunchKernelGGL(score_reg_kernel<2>, grid, dim3(64), lds, stream, p);
        else if (states + 2 <= 256) hipLaunchKernelGGL(score_reg_kernel<4>, grid, dim3(64), lds, stream, p);
        else if (states + 2 <= 384) hipLaunchKernelGGL(score_reg_kernel<6>, grid, dim3(64), lds, stream, p);
        else hipLaunchKernelGGL(score_reg_kernel<8>, grid, dim3(64), lds, stream, p);
    } else {
        p.cap = (int)states;
        const size_t lds = lds_bytes(p.lab_cap, p.cap);
        const int threads = states <= 2048 ? 256 : (states <= 6144 ? 512 : 1024);
#ifndef FCD_HIPEMU
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(score_lds_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
#endif
        hipLaunchKernelGGL(score_lds_kernel, grid, dim3(threads), lds, stream, p);
    }
    return hipGetLastError();
}

}  // namespace fcd
