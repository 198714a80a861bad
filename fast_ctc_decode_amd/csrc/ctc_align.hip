// ctc_align.hip -- CTC forced alignment of given labellings (fcd_ctc_align_*; include/fcd.h): the best single alignment
// through the lattice ctc_score.hip sums over.  NOT a reference function.
//
// The step is ctc_score's with max where it has +: a cell is  u = max(a[s], a[s-1], a[s-2]) * pm  (ONE f32 rounding),
// candidates taken in the order stay, s-1, s-2, a later one only if strictly greater; which one won is the cell's 2-bit
// back-pointer.  Window, staging (ctc_lattice.h), the power-of-two rescaling of every row and the float64 tail are the
// score kernels'.  A read with a NaN, infinite or negative posterior is flagged while its tiles are staged (misc[17]).
//
// Back-pointers go to device memory (the caller's workspace), indexed by SLOT, so the traceback never needs to know where
// a row's window lay:
//   align_reg_kernel<K>  row t of a labelling is 64 words, one per lane: the 2K bits of the lane's K cells (a byte for
//                        K <= 4, a halfword above) -- 0.25 bytes per (row, slot), one coalesced 64 / 128-byte store per row.
//   align_lds_kernel     one byte per (row, slot), slot = s mod cap: cap bytes per row.
// The workgroup that ran the forward pass walks them back in the same launch, 64 rows at a time through LDS (the tile
// area, free by then): the register kernel's 64 x 64 words as they are; the LDS kernel the 64 x 128 cells the walk can
// reach from where it stands (it descends at most two states a row).  The walk itself is wave-uniform and leaves
// start / count of every label; the qualities are then one label per work-item, each a sequential f32 sum in row order.
#include <math.h>

#include <algorithm>

#include "ctc_lattice.h"

namespace fcd {
namespace {

constexpr int kTraceRows = 64;
constexpr int kTraceSpan = 128;  // LDS kernel: states of a row the walk can reach inside one chunk (2 * 63 + 1, rounded up)
static_assert(kTraceRows * kTraceSpan <= kTileElems * 8, "the traceback chunk lives in the tile area");
static_assert(2 * kLdsCells <= 64, "the LDS kernel keeps a step's back-pointers in one 64-bit word");

struct AlignParams {
    ScoreParams s;  // (s.logp is never null: the launcher lends scratch when the caller wants none)
    uint32_t *start;
    uint32_t *count;
    float *qual;          // nullable
    unsigned char *bp;    // back-pointers, bp_row_bytes per labelling of this launch
    int64_t bp_row_bytes;
};

template <int K> struct BpWord { typedef uint16_t type; };
template <> struct BpWord<2> { typedef uint8_t type; };
template <> struct BpWord<4> { typedef uint8_t type; };

// fill_tile of ctc_lattice.h, and the flag
__device__ __forceinline__ void fill_tile_checked(const ScoreParams &p, const Lds &lds, const Row &rw, int t0, int rc) {
    const int tid = threadIdx.x, bd = blockDim.x;
    __syncthreads();  // the previous tile's readers are done
    bool bad = false;
    for (int e = tid; e < rc * rw.N; e += bd) {
        const int i = e / rw.N, j = e - i * rw.N;
        const float v = load_post(rw.post, (int64_t)(t0 + i) * p.in.stride_t + (int64_t)j * p.in.stride_n, p.in.dtype);
        int ex = 0;
        float m = v;
        if (v - v == 0.0f) m = frexpf(v, &ex);
        bad |= !(v >= 0.0f && v - v == 0.0f);
        lds.pm[e] = m;
        lds.pe[e] = ex;
    }
    if (bad) lds.misc[kBadPost] = 1;
    if (p.band > 0 && tid < rc) lds.krow[tid] = labels_up_to(rw.path, rw.L, (uint32_t)(t0 + tid));
    __syncthreads();
}

// a row without an alignment: count = 0 for the labels the row holds (its logp is written already)
__device__ __forceinline__ void no_alignment(const AlignParams &q) {
    const int64_t row = blockIdx.x;
    const int64_t n = min((int64_t)q.s.y.len[row], q.s.y.stride);
    for (int64_t k = threadIdx.x; k < n; k += blockDim.x) q.count[row * q.s.y.stride + k] = 0u;
}

// the walk, last row first: the alignment is in state s at the row at hand, cnt rows of its label seen so far
struct Walk {
    int s, cnt;
};

__device__ __forceinline__ void walk_row(Walk &w, int t, int d, uint32_t *start, uint32_t *count, bool writer) {
    d = min(min(d, 2), w.s);  // (a back-pointer is 0, 1 or 2: the bound the parked chunk is sized for)
    if (w.s & 1) {
        w.cnt++;
        if (d != 0) {  // the label was entered at this row
            if (writer) {
                start[w.s >> 1] = (uint32_t)t;
                count[w.s >> 1] = (uint32_t)w.cnt;
            }
            w.cnt = 0;
        }
    }
    w.s -= d;
}

// logp of the row; returns the state the best alignment ends in, -1 when there is none (count zeroed by the caller)
__device__ __forceinline__ int finish(const AlignParams &q, const Lds &lds, const Row &rw, float c0, float c1, int64_t eacc) {
    const bool bad = lds.misc[kBadPost] != 0;
    const bool odd = c1 > c0;  // state 2L unless 2L - 1 is strictly greater
    const float m = odd ? c1 : c0;
    if (threadIdx.x == 0)
        q.s.logp[blockIdx.x] = bad ? (double)NAN : ln_p((double)m, eacc);
    if (bad || !(m > 0.0f) || m - m != 0.0f) return -1;
    return 2 * rw.L - (odd ? 1 : 0);
}

// one label per work-item: the mean posterior of its rows, summed in f32 in row order (search.rs:337-376)
__device__ __forceinline__ void qualities(const AlignParams &q, const Row &rw) {
    if (!q.qual) return;
    const ScoreParams &p = q.s;
    const int64_t base = (int64_t)blockIdx.x * p.y.stride;
    __syncthreads();  // start / count as the walk left them
    for (int k = threadIdx.x; k < rw.L; k += blockDim.x) {
        const int64_t t = q.start[base + k];
        const int c = (int)q.count[base + k];
        const int64_t col = (int64_t)rw.labels[k] * p.in.stride_n;
        float sum = load_post(rw.post, t * p.in.stride_t + col, p.in.dtype);
        for (int j = 1; j < c; ++j) sum += load_post(rw.post, (t + j) * p.in.stride_t + col, p.in.dtype);
        q.qual[base + k] = sum / (float)c;
    }
}

// ---- the register-resident window ----
template <int K>
__global__ __launch_bounds__(64) void align_reg_kernel(AlignParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    typedef typename BpWord<K>::type BpT;
    constexpr int C = 64 * K;
    const ScoreParams &p = q.s;
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    if (!prologue(p, lds, &rw)) {
        no_alignment(q);
        return;
    }
    const int lane = threadIdx.x;
    if (lane == 0) lds.misc[kBadPost] = 0;
    BpT *bp = reinterpret_cast<BpT *>(q.bp + (int64_t)blockIdx.x * q.bp_row_bytes);
    float a[K];  // the best alignment into each of the lane's K states, scaled by 2^-eacc
#pragma unroll
    for (int r = 0; r < K; ++r) a[r] = 0.0f;
    if (lane == 0) a[0] = 1.0f;  // "row -1": state 0
    int64_t eacc = 0;
    int lo_prev = 0, lo = 0, hi = 0;
    for (int t0 = 0; t0 < rw.Tr; t0 += rw.rows_per_tile) {
        const int rc = min(rw.rows_per_tile, rw.Tr - t0);
        fill_tile_checked(p, lds, rw, t0, rc);
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
            float u[K];
            int ex[K];
            int emax = kNoExp;
            uint32_t bits = 0;
#pragma unroll
            for (int r = 0; r < K; ++r) {
                const float x1 = r >= 1 ? a[r - 1] : p1;
                const float x2 = r >= 2 ? a[r - 2] : (r == 1 ? p1 : p2);
                float best;
                uint32_t arg;
                if (r & 1) {
                    best = p.collapse ? a[r] : x1;
                    arg = p.collapse ? 0u : 1u;
                    if (p.collapse && x1 > best) {
                        best = x1;
                        arg = 1u;
                    }
                    const float x2m = ((in.skip_mask >> r) & 1) ? x2 : 0.0f;
                    if (x2m > best) {
                        best = x2m;
                        arg = 2u;
                    }
                    u[r] = best * in.pm[r / 2];
                    ex[r] = in.pe[r / 2];
                } else {
                    best = a[r];
                    arg = 0u;
                    if (x1 > best) {
                        best = x1;
                        arg = 1u;
                    }
                    u[r] = best * in.pm0;
                    ex[r] = in.pe0;
                }
                bits |= arg << (2 * r);
                const int e = finite_exp(u[r]);
                emax = max(emax, ((in.in_mask >> r) & 1) && e != kNoExp ? e + ex[r] : kNoExp);
            }
            bp[(int64_t)(t0 + i) * 64 + lane] = (BpT)bits;
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
    if (lane == 0) lds.misc[18] = lds.misc[19] = 0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const int s = slot_state<K>(lane, r, lo);
        if (s <= hi && s == 2 * rw.L) lds.misc[18] = __float_as_int(a[r]);
        if (s <= hi && s == 2 * rw.L - 1) lds.misc[19] = __float_as_int(a[r]);
    }
    __syncthreads();
    const int end = finish(q, lds, rw, __int_as_float(lds.misc[18]), __int_as_float(lds.misc[19]), eacc);
    if (end < 0) {
        no_alignment(q);
        return;
    }
    // the walk: every lane parks its own column of 64 rows (the words it stored itself), then all of them follow the path
    uint32_t *start = q.start + (int64_t)blockIdx.x * p.y.stride, *count = q.count + (int64_t)blockIdx.x * p.y.stride;
    BpT *sbp = reinterpret_cast<BpT *>(smem);
    Walk w{end, 0};
    for (int c0 = (rw.Tr - 1) / kTraceRows * kTraceRows; c0 >= 0; c0 -= kTraceRows) {
        const int n = min(kTraceRows, rw.Tr - c0);
        __syncthreads();
        for (int i = 0; i < n; ++i) sbp[i * 64 + lane] = bp[(int64_t)(c0 + i) * 64 + lane];
        __syncthreads();
        for (int i = n - 1; i >= 0; --i) {
            const int slot = w.s % C;
            const int word = sbp[i * 64 + slot / K];
            const int d = __builtin_amdgcn_readfirstlane((word >> (2 * (slot % K))) & 3);
            walk_row(w, c0 + i, d, start, count, lane == 0);
        }
    }
    qualities(q, rw);
}

// ---- the LDS-resident window ----
__global__ __launch_bounds__(1024) void align_lds_kernel(AlignParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const ScoreParams &p = q.s;
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    if (!prologue(p, lds, &rw)) {
        no_alignment(q);
        return;
    }
    const int tid = threadIdx.x, bd = blockDim.x, cap = p.cap, nw = bd >> 6;
    if (tid == 0) lds.misc[kBadPost] = 0;
    unsigned char *bp = q.bp + (int64_t)blockIdx.x * q.bp_row_bytes;
    for (int s = tid; s < 2 * cap; s += bd) lds.alpha[s] = 0.0f;
    __syncthreads();
    if (tid == 0) lds.alpha[0] = 1.0f;  // "row -1": state 0
    int64_t eacc = 0;
    int lo_prev = 0, hi_prev = 0, base = 0, which = 0;
    auto rd = [&](const float *buf, int n) -> float {
        if (n < lo_prev || n > hi_prev) return 0.0f;
        int idx = n - base;
        idx = idx < 0 ? idx + cap : (idx >= cap ? idx - cap : idx);
        return buf[idx];
    };
    for (int t0 = 0; t0 < rw.Tr; t0 += rw.rows_per_tile) {
        const int rc = min(rw.rows_per_tile, rw.Tr - t0);
        fill_tile_checked(p, lds, rw, t0, rc);
        for (int i = 0; i < rc; ++i) {
            int lo, hi;
            window(p, lds, rw, t0 + i, i, &lo, &hi);
            const float *prev = lds.alpha + which * cap;
            float *next = lds.alpha + (which ^ 1) * cap;
            const float pm0 = lds.pm[i * rw.N];
            const int pe0 = lds.pe[i * rw.N];
            float u[kLdsCells];
            int ex[kLdsCells];
            uint64_t args = 0;  // 2 bits a cell: kLdsCells = 20 of them
            int emax = kNoExp;
#pragma unroll
            for (int c = 0; c < kLdsCells; ++c) {
                const int s = lo + tid + c * bd;
                u[c] = 0.0f;
                ex[c] = 0;
                if (s <= hi) {
                    const float x0 = rd(prev, s), x1 = rd(prev, s - 1);
                    float best;
                    uint32_t arg;
                    if (s & 1) {
                        const int info = lds.lab[s >> 1];
                        best = p.collapse ? x0 : x1;
                        arg = p.collapse ? 0u : 1u;
                        if (p.collapse && x1 > best) {
                            best = x1;
                            arg = 1u;
                        }
                        if (s >= 3 && (!p.collapse || (info & 0x100))) {
                            const float x2 = rd(prev, s - 2);
                            if (x2 > best) {
                                best = x2;
                                arg = 2u;
                            }
                        }
                        u[c] = best * lds.pm[i * rw.N + (info & 0xFF)];
                        ex[c] = lds.pe[i * rw.N + (info & 0xFF)];
                    } else {
                        best = x0;
                        arg = 0u;
                        if (x1 > best) {
                            best = x1;
                            arg = 1u;
                        }
                        u[c] = best * pm0;
                        ex[c] = pe0;
                    }
                    args |= (uint64_t)arg << (2 * c);
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
            unsigned char *bp_row = bp + (int64_t)(t0 + i) * cap;
#pragma unroll
            for (int c = 0; c < kLdsCells; ++c) {
                const int s = lo + tid + c * bd;
                if (s <= hi) {
                    int idx = s - base;
                    idx = idx >= cap ? idx - cap : idx;
                    next[idx] = ldexpf(u[c], min(max(ex[c] + sh, -512), 512));
                    bp_row[idx] = (unsigned char)((args >> (2 * c)) & 3u);
                }
            }
            lo_prev = lo;
            hi_prev = hi;
            which ^= 1;
            __syncthreads();
        }
    }
    const float *last = lds.alpha + which * cap;
    const int end = finish(q, lds, rw, rd(last, 2 * rw.L), rd(last, 2 * rw.L - 1), eacc);
    if (end < 0) {
        no_alignment(q);
        return;
    }
    // the walk: of every row of a chunk, the kTraceSpan states at and below the state the chunk is entered in
    uint32_t *start = q.start + (int64_t)blockIdx.x * p.y.stride, *count = q.count + (int64_t)blockIdx.x * p.y.stride;
    unsigned char *sbp = smem;
    Walk w{end, 0};
    for (int c0 = (rw.Tr - 1) / kTraceRows * kTraceRows; c0 >= 0; c0 -= kTraceRows) {
        const int n = min(kTraceRows, rw.Tr - c0);
        const int s0 = w.s - (kTraceSpan - 1);  // the state in column 0
        __syncthreads();
        for (int e = tid; e < n * kTraceSpan; e += bd) {
            const int i = e / kTraceSpan, s = s0 + (e - i * kTraceSpan);
            sbp[e] = s >= 0 ? bp[(int64_t)(c0 + i) * cap + s % cap] : (unsigned char)0;
        }
        __syncthreads();
        for (int i = n - 1; i >= 0; --i) {
            const int d = __builtin_amdgcn_readfirstlane((int)sbp[i * kTraceSpan + (w.s - s0)] & 3);
            walk_row(w, c0 + i, d, start, count, tid == 0);
        }
    }
    qualities(q, rw);
}

// the shape of a call's kernel: states per lane of the register kernel (0: the LDS kernel) and the LDS kernel's states
void align_shape(int64_t T, int64_t stride, int64_t band, int *k, int64_t *cap) {
    const int64_t states = ctc_score_window_states(T, stride, band);
    *cap = 0;
    if (states + 2 <= 128) *k = 2;
    else if (states + 2 <= 256) *k = 4;
    else if (states + 2 <= 384) *k = 6;
    else if (states + 2 <= 512) *k = 8;
    else {
        *k = 0;
        *cap = states;
    }
}

}  // namespace

// back-pointer bytes of one labelling (every one of a call has T rows' worth)
size_t ctc_align_row_bytes(int64_t T, int64_t stride, int64_t band) {
    int k;
    int64_t cap;
    align_shape(T, stride, band, &k, &cap);
    const size_t per_row = k == 0 ? (size_t)cap : (k <= 4 ? 64 : 128);
    return ((size_t)std::max<int64_t>(T, 1) * per_row + 255) & ~(size_t)255;
}

hipError_t launch_ctc_align(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, const AlignOut &out,
                            unsigned char *bp, hipStream_t stream) {
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    AlignParams q;
    q.s.in = in;
    q.s.y = y;
    q.s.collapse = collapse;
    q.s.band = (int)band;
    q.s.logp = out.logp;
    q.s.lab_cap = (int)std::max<int64_t>(std::min(in.T, y.stride), 1);
    q.start = out.start;
    q.count = out.count;
    q.qual = out.qual;
    q.bp = bp;
    q.bp_row_bytes = (int64_t)ctc_align_row_bytes(in.T, y.stride, band);
    int k;
    int64_t cap;
    align_shape(in.T, y.stride, band, &k, &cap);
    q.s.cap = (int)cap;
    const dim3 grid((unsigned)rows);
    const size_t lds = lds_bytes(q.s.lab_cap, q.s.cap);
    if (k == 2) hipLaunchKernelGGL(align_reg_kernel<2>, grid, dim3(64), lds, stream, q);
    else if (k == 4) hipLaunchKernelGGL(align_reg_kernel<4>, grid, dim3(64), lds, stream, q);
    else if (k == 6) hipLaunchKernelGGL(align_reg_kernel<6>, grid, dim3(64), lds, stream, q);
    else if (k == 8) hipLaunchKernelGGL(align_reg_kernel<8>, grid, dim3(64), lds, stream, q);
    else {
        const int threads = cap <= 2048 ? 256 : (cap <= 6144 ? 512 : 1024);
#ifndef FCD_HIPEMU
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(align_lds_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
#endif
        hipLaunchKernelGGL(align_lds_kernel, grid, dim3(threads), lds, stream, q);
    }
    return hipGetLastError();
}

}  // namespace fcd
