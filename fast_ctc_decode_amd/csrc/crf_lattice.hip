// crf_lattice.hip -- the lattice of a GIVEN labelling under a CRF model (fcd_crf_score_* / fcd_crf_align_*; include/fcd.h):
// walked forward as a sum (the likelihood of the labelling) and as a max with back-pointers (its best alignment).
// NOT a reference function: the unpruned, unmerged form of the recurrence search::crf_beam_search walks
// (src/search.rs:62-100), for one labelling.
//
// States k = 0 .. L count the labels emitted so far; the model state sigma_k they read their row from depends on the
// init row and the labelling only (src/search.rs:58,97) and is computed once, before the time loop, next to the label in
// LDS.  A cell has two sources:  stay  a[k] * p[t][sigma_k][0]  and  advance  a[k-1] * p[t][sigma_{k-1}][y_{k-1}].
// Both products are formed AT THE SOURCE (one f32 rounding each): a lane reads the two posteriors of every state it
// holds, and the advance product travels one slot up -- inside the lane, or by one wave rotation (from_prev_lane).
//
// One wavefront per labelling, K in {1, 2, 4, 8} consecutive states per lane in registers; state k lives in slot
// k mod 64K (slot_state of ctc_lattice.h), so the window slides through the slots.  Every slot knows which state it
// held in the previous row and which it holds now: a product enters a cell only if both agree, so a window may fill
// all 64K slots.  Numerics are ctc_score.hip's: posteriors split into mantissa and exponent, the row's largest
// exponent reduced as an integer (wave_imax), every cell rescaled by an exact power of two, ln(m) + E ln 2 in float64.
//
// Posteriors: a row is S * N values of which the window reads two per live state.  While S * N fits the tile, whole
// rows are staged in LDS (raw f32, rows_per_tile at a time); beyond it every lane gathers its own values from global
// memory, a row ahead of their use (the addresses depend on sigma, y and t only, never on alpha).
//
// Align: one back-pointer BIT per row and slot (advance won, strictly), a row is K 64-bit ballots = 8K bytes in the
// caller's workspace; the workgroup walks them back in the same launch, 64 rows at a time through LDS.
#include <math.h>

#include <algorithm>

#include "crf_lattice.h"

namespace fcd {
namespace {

constexpr int kCrfTraceRows = 64;
static_assert(kCrfTraceRows * 8 * 8 <= kTileElems * 4, "the traceback chunk lives in the tile area");

// a row without an alignment: count = 0 for the labels the row holds (its logp is written already)
__device__ __forceinline__ void crf_no_alignment(const CrfParams &p) {
    const int64_t row = blockIdx.x;
    const int64_t n = min((int64_t)p.y.len[row], p.y.stride);
    for (int64_t k = threadIdx.x; k < n; k += 64) p.count[row * p.y.stride + k] = 0u;
}

// MAX = false: the forward sum (fcd_crf_score_*); MAX = true: the best alignment with back-pointers (fcd_crf_align_*).
// The time loop is crf_forward_walk of crf_lattice.h (crf_posterior.hip's forward launch runs its third mode); the
// traceback and the qualities are here.
template <bool MAX, int K>
__global__ __launch_bounds__(64) void crf_lattice_kernel(CrfParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int C = 64 * K;
    const CrfLds lds = crf_carve(smem);
    CrfRow rw;
    if (!crf_prologue(p, lds, &rw)) {
        if (MAX) crf_no_alignment(p);
        return;
    }
    const int lane = threadIdx.x;
    uint64_t *bp = MAX ? reinterpret_cast<uint64_t *>(p.bp + (int64_t)blockIdx.x * p.bp_row_bytes) : nullptr;
    int64_t eacc;
    const float m = crf_forward_walk<MAX ? kCrfMax : kCrfSum, K>(p, lds, rw, bp, nullptr, nullptr, &eacc);
    const double ln = ln_p((double)m, eacc);
    if (!MAX) {
        if (lane == 0) p.logp[blockIdx.x] = ln;
        return;
    }
    const bool flagged = lds.misc[kBadPost] != 0;
    if (lane == 0) p.logp[blockIdx.x] = flagged ? (double)NAN : ln;
    if (flagged || !(m > 0.0f) || m - m != 0.0f) {
        crf_no_alignment(p);
        return;
    }
    // the walk, last row first: a set bit means the state was entered at that row -- its label's emission row
    uint32_t *start = p.start + (int64_t)blockIdx.x * p.y.stride, *count = p.count + (int64_t)blockIdx.x * p.y.stride;
    uint64_t *sbp = reinterpret_cast<uint64_t *>(smem);
    int k = rw.L;
    for (int c0 = (rw.Tr - 1) / kCrfTraceRows * kCrfTraceRows; c0 >= 0; c0 -= kCrfTraceRows) {
        const int n = min(kCrfTraceRows, rw.Tr - c0);
        __syncthreads();
        for (int e = lane; e < n * K; e += 64) sbp[e] = bp[(int64_t)c0 * K + e];
        __syncthreads();
        for (int i = n - 1; i >= 0; --i) {
            const int slot = k % C;
            const uint64_t word = sbp[i * K + slot % K];
            const int d = __builtin_amdgcn_readfirstlane((int)((word >> (slot / K)) & 1u));
            if (d && k > 0) {
                if (lane == 0) {
                    start[k - 1] = (uint32_t)(c0 + i);
                    count[k - 1] = 1u;
                }
                k -= 1;
            }
        }
    }
    if (!p.qual) return;
    float *qual = p.qual + (int64_t)blockIdx.x * p.y.stride;
    __syncthreads();  // start as the walk left it
    for (int j = lane; j < rw.L; j += 64) {
        const uint32_t info = lds.info[j];
        const uint32_t sig = info & 0xFFFFFFu;
        const int64_t at = (int64_t)start[j] * p.in.stride_t + (int64_t)sig * p.in.stride_s + (int64_t)(info >> 24) * p.in.stride_n;
        qual[j] = sig != kNoState ? load_post(rw.post, at, p.in.dtype) : 0.0f;
    }
}

template <bool MAX>
hipError_t launch_crf(const CrfParams &p, int k, int64_t rows, hipStream_t stream) {
    const dim3 grid((unsigned)rows);
    const size_t lds = crf_lds_bytes(p.lab_cap);
    if (k == 1) hipLaunchKernelGGL((crf_lattice_kernel<MAX, 1>), grid, dim3(64), lds, stream, p);
    else if (k == 2) hipLaunchKernelGGL((crf_lattice_kernel<MAX, 2>), grid, dim3(64), lds, stream, p);
    else if (k == 4) hipLaunchKernelGGL((crf_lattice_kernel<MAX, 4>), grid, dim3(64), lds, stream, p);
    else hipLaunchKernelGGL((crf_lattice_kernel<MAX, 8>), grid, dim3(64), lds, stream, p);
    return hipGetLastError();
}

}  // namespace

// The most states a window of this call can hold: what the host knows without reading a labelling.
int64_t crf_lattice_window_states(int64_t T, int64_t stride, int64_t band) {
    const int64_t exact = std::min(T, stride) + 1;
    return band > 0 ? std::min(exact, 2 * band + 1) : exact;
}

// 0: supported; 1: the window exceeds the 512 register-resident states; 2: S beyond the state word; 3: the labelling's LDS copy
int crf_lattice_unsupported(int64_t T, int64_t S, int64_t stride, int64_t band) {
    if (crf_lattice_window_states(T, stride, band) > 512) return 1;
    if (S >= (int64_t)kNoState) return 2;
    if (crf_lds_bytes((int)std::min<int64_t>(std::min(T, stride) + 1, 1 << 24)) > 64 * 1024) return 3;
    return 0;
}

size_t crf_align_row_bytes(int64_t T, int64_t stride, int64_t band) {
    const size_t per_row = 8 * (size_t)crf_states_per_lane(T, stride, band);
    return ((size_t)std::max<int64_t>(T, 1) * per_row + 255) & ~(size_t)255;
}

hipError_t launch_crf_score(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                            int64_t band, double *logp, hipStream_t stream) {
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    CrfParams p = crf_params(in, y, init, n_init, init_stride, band);
    p.logp = logp;
    return launch_crf<false>(p, crf_states_per_lane(in.T, y.stride, band), rows, stream);
}

hipError_t launch_crf_align(const BatchDesc &in, const ScoreDesc &y, const float *init, int64_t n_init, int64_t init_stride,
                            int64_t band, const AlignOut &out, unsigned char *bp, hipStream_t stream) {
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    CrfParams p = crf_params(in, y, init, n_init, init_stride, band);
    p.logp = out.logp;
    p.start = out.start;
    p.count = out.count;
    p.qual = out.qual;
    p.bp = bp;
    p.bp_row_bytes = (int64_t)crf_align_row_bytes(in.T, y.stride, band);
    return launch_crf<true>(p, crf_states_per_lane(in.T, y.stride, band), rows, stream);
}

}  // namespace fcd
