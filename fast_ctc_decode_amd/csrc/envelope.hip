// envelope.hip -- alignment-band estimator for the duplex searches.
//
// The reference has no such function: beam_search_duplex defaults to the full envelope and its
// docstring only anticipates "a non-trivial default" (/root/reference/src/lib.rs:376-378).  The
// algorithm is therefore specified by tests/envelope_model.py (numpy), which this kernel reproduces
// exactly (integer work):
//   1. global alignment of the two label sequences of a pair under unit-cost edit distance -- one
//      wavefront per pair, one DP row at a time: the in-row dependency D[i][j-1] + 1 is a min-plus
//      prefix scan (D[i][j] = j + min_{j' <= j} (E[j'] - j')), done with DPP row shifts across the 64
//      lanes and a carry between 64-column chunks; the previous row lives in LDS as u16, the
//      "came from diagonal / from above" decisions leave the kernel as two 64-bit ballots per chunk;
//   2. traceback (diagonal, then up, then left) turns matches of equal labels into anchors
//      (time in read 1 -> time in read 2) through the two paths;
//   3. row i of the envelope is the anchors' piecewise-linear interpolation +- band, clipped, with
//      lo(0) = 0, hi(T1 - 1) = T2 and lo(i) <= hi(i - 1) (src/duplex.rs:485-488).
#include <limits.h>

#include <algorithm>

#include "device_utils.h"
#include "fcd_internal.h"

namespace fcd {

namespace {

struct EnvParams {
    EnvelopeArgs a;
    int64_t pair_begin;
    EditArgs ed;  // fcd_edit_distance_*: read where `edit` is set, and nothing else is
    int edit;
};

constexpr int kBig = INT_MAX / 2;

// DPP controls (gfx9 family): row_shr:n = 0x110 + n, row_bcast:15 = 0x142, row_bcast:31 = 0x143
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ int dpp_or_big(int x) {
    return __builtin_amdgcn_update_dpp(kBig, x, CTRL, ROW_MASK, BANK_MASK, false);
}

// inclusive prefix minimum over the 64 lanes (the classic GCN scan: three shifts of the input,
// then shifts by 4 and 8 inside each row of 16, then the two row broadcasts)
__device__ __forceinline__ int wave_prefix_min(int x) {
    int t = min(x, dpp_or_big<0x111, 0xf, 0xf>(x));
    t = min(t, dpp_or_big<0x112, 0xf, 0xf>(x));
    t = min(t, dpp_or_big<0x113, 0xf, 0xf>(x));
    t = min(t, dpp_or_big<0x114, 0xf, 0xe>(t));
    t = min(t, dpp_or_big<0x118, 0xf, 0xc>(t));
    t = min(t, dpp_or_big<0x142, 0xa, 0xf>(t));
    t = min(t, dpp_or_big<0x143, 0xc, 0xf>(t));
    return t;
}

__device__ __forceinline__ uint64_t load_u64_l2(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- batched edit distance (fcd_edit_distance_*): the kernel's second body ----
// Myers' bit-parallel recurrence in Hyyro's global-distance form, one PAIR per lane (or per group of lanes), no DP row in
// memory.  Sequence 2 is the vertical pattern: a lane holds W blocks of 64 labels as four bit-planes each (labels are below
// 16), and the vertical deltas Pv / Mv of those blocks; everything is statically indexed and lives in registers.  One step
// takes one label of sequence 1 (the text): Eq of a block is the AND over the planes of ~(plane ^ broadcast of the
// label's bit), then Xv / Xh / Ph / Mh per block with the horizontal carry (hp, hm) handed from block b to block b + 1;
// the carry into block 0 is +1 (global: D[0][j] = j) or 0 (infix: free start in the text).  The block holding bit
// len2 - 1 reads the score's change off Ph / Mh at that bit; bits above it never reach down, so lanes of one wavefront hold
// patterns of any lengths up to the tier.
// Patterns beyond 512 labels spread over g = 2 .. 64 adjacent lanes (W = 8 each) that run as a systolic array skewed by one
// text label per lane: at step k lane i of a group takes label k - i, with (label, hp, hm) as lane i - 1 left them one step
// earlier -- one full-wave DPP shift (wave_shr:1, which crosses the 16-lane rows) of one packed word per step.
// Text labels reach the lanes through a 64 x 64 byte LDS tile (rows 68 bytes apart: word reads of 64 rows hit 64 banks):
// the wavefront reads 64 consecutive labels of one pair per load.  The pattern's planes are ballots of the label bits while
// 64 labels of a pair sit one per lane; the owning lane keeps the four words.
constexpr int kEditTilePitch = 68;

__device__ __forceinline__ int edit_from_lane_below(int x) {  // wave_shr:1; lane 0 keeps 0
    return __builtin_amdgcn_update_dpp(0, x, 0x138, 0xf, 0xf, false);
}

template <int W>
__device__ __forceinline__ void edit_walk(const EditArgs &a, unsigned char *smem) {
    constexpr int U = 8 / W;  // pairs whose pattern loads are in flight together: eight loads either way
    const int lane = threadIdx.x;
    const int gs = a.gshift, g = 1 << gs;
    const int npw = kWave >> gs;    // pairs per wavefront
    const int gi = lane & (g - 1);  // this lane's place in its group
    const int slot = lane >> gs;    // its pair's place in the wavefront
    const int64_t pair0 = (int64_t)blockIdx.x * npw;
    const int64_t r = pair0 + slot;
    const bool have = r < a.n_pairs;
    int L1 = 0, L2 = 0;
    if (have) {
        const uint32_t v1 = a.len1[r], v2 = a.len2[r];
        L1 = v1 < (uint32_t)a.cap1 ? (int)v1 : a.cap1;
        L2 = v2 < (uint32_t)a.cap2 ? (int)v2 : a.cap2;
    }
    const int maxL1 = wave_imax(L1), maxL2 = wave_imax(L2);
    bool bad = false;  // a label of 16 or more inside the pair's lengths

    // ---- the pattern: ballots of the label bits, 64 labels of one pair at a time ----
    uint64_t plane[W][4], Pv[W], Mv[W];
#pragma unroll
    for (int b = 0; b < W; ++b) {
        plane[b][0] = plane[b][1] = plane[b][2] = plane[b][3] = 0;
        Pv[b] = ~0ull;
        Mv[b] = 0;
    }
    for (int q0 = 0; q0 < npw; q0 += U) {
        int Lq[U], Lmax = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            Lq[u] = __shfl(L2, ((q0 + u) << gs) & 63);  // (q0 + u < npw: U > 1 only where npw = 64)
            Lmax = Lq[u] > Lmax ? Lq[u] : Lmax;
        }
        for (int i = 0; i < g && i * (W * 64) < Lmax; ++i) {
            uint32_t v[U][W];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint8_t *row = a.labels2 + (pair0 + q0 + u) * a.stride2;
#pragma unroll
                for (int b = 0; b < W; ++b) {
                    const int j = (i * W + b) * 64 + lane;
                    v[u][b] = j < Lq[u] ? row[j] : 0u;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool owner = lane == ((q0 + u) << gs) + i;
#pragma unroll
                for (int b = 0; b < W; ++b) {
                    if ((i * W + b) * 64 >= Lq[u]) continue;  // (wave-uniform)
                    const uint32_t x = v[u][b];
                    const uint64_t m16 = ballot(x >= 16u);
                    const uint64_t m0 = ballot((x & 1u) != 0u), m1 = ballot((x & 2u) != 0u);
                    const uint64_t m2 = ballot((x & 4u) != 0u), m3 = ballot((x & 8u) != 0u);
                    if (owner) {
                        plane[b][0] = m0;
                        plane[b][1] = m1;
                        plane[b][2] = m2;
                        plane[b][3] = m3;
                    }
                    if (slot == q0 + u && m16 != 0ull) bad = true;
                }
            }
        }
    }

    // ---- the walk ----
    uint8_t *tile = smem;
    const uint32_t *tile32 = reinterpret_cast<const uint32_t *>(smem);
    const int last = L2 > 0 ? L2 - 1 : 0;
    const int owner_gi = (last >> 6) / W, bs = (last >> 6) % W, bit = last & 63;
    const bool pass = (gi + 1) * (W * 64) < L2;    // the pattern goes on in the next lane
    const int nb = g > 1 ? W : (maxL2 + 63) >> 6;  // blocks any lane of the wavefront needs (wave-uniform)
    const int carry_in = a.mode == FCD_EDIT_GLOBAL ? 1 : 0;
    int score = L2, best = L2, best_end = 0;
    int out = 0;
    uint32_t word = 0;
    const int64_t nsteps = maxL1 > 0 ? (int64_t)maxL1 + g - 1 : 0;
    for (int64_t k = 0; k < nsteps; ++k) {
        if ((k & 63) == 0 && k < maxL1) {  // the next 64 text labels of every pair of the wavefront
            wave_sync();
            for (int q0 = 0; q0 < npw; q0 += 8) {
                uint32_t v[8];
                int Lq[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = q0 + u;
                    Lq[u] = __shfl(L1, (q << gs) & 63);
                    if (q >= npw) Lq[u] = 0;
                    const int64_t j = k + lane;
                    v[u] = j < Lq[u] ? a.labels1[(pair0 + q) * a.stride1 + j] : 0u;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int q = q0 + u;
                    if (k >= Lq[u]) continue;  // (wave-uniform: nobody reads this row any more)
                    const uint64_t m16 = ballot(v[u] >= 16u);
                    if (slot == q && m16 != 0ull) bad = true;
                    tile[q * kEditTilePitch + lane] = (uint8_t)v[u];
                }
            }
            wave_sync();
        }
        int x = gs > 0 ? edit_from_lane_below(out) : 0;
        if (gi == 0) {
            if ((k & 3) == 0) word = tile32[slot * (kEditTilePitch / 4) + (int)((k & 63) >> 2)];
            const int label = (int)(word >> (8 * (int)(k & 3))) & 15;
            x = k < L1 ? (label | carry_in << 4 | 64) : 0;
        }
        out = 0;
        if (x & 64) {  // (label, hp, hm) of text label k - gi
            const int label = x & 15;
            int hp = (x >> 4) & 1, hm = (x >> 5) & 1;
            const uint64_t t0 = 0ull - (uint64_t)(label & 1), t1 = 0ull - (uint64_t)((label >> 1) & 1);
            const uint64_t t2 = 0ull - (uint64_t)((label >> 2) & 1), t3 = 0ull - (uint64_t)((label >> 3) & 1);
            uint64_t selP = 0, selM = 0;
#pragma unroll
            for (int b = 0; b < W; ++b) {
                if (b >= nb) continue;
                uint64_t Eq = ~((plane[b][0] ^ t0) | (plane[b][1] ^ t1) | (plane[b][2] ^ t2) | (plane[b][3] ^ t3));
                const uint64_t pv = Pv[b], mv = Mv[b];
                const uint64_t Xv = Eq | mv;
                Eq |= (uint64_t)hm;
                const uint64_t Xh = (((Eq & pv) + pv) ^ pv) | Eq;
                uint64_t Ph = mv | ~(Xh | pv);
                uint64_t Mh = pv & Xh;
                selP = b == bs ? Ph : selP;
                selM = b == bs ? Mh : selM;
                const int hpo = (int)(Ph >> 63), hmo = (int)(Mh >> 63);
                Ph = (Ph << 1) | (uint64_t)hp;
                Mh = (Mh << 1) | (uint64_t)hm;
                Pv[b] = Mh | ~(Xv | Ph);
                Mv[b] = Ph & Xv;
                hp = hpo;
                hm = hmo;
            }
            if (pass) out = label | hp << 4 | hm << 5 | 64;
            if (gi == owner_gi) {
                score += (int)((selP >> bit) & 1ull) - (int)((selM >> bit) & 1ull);
                if (score < best) {  // (strictly: the smallest end among equals)
                    best = score;
                    best_end = (int)(k - gi) + 1;
                }
            }
        }
    }
    if (have && gi == owner_gi) {
        uint32_t d, e;
        if (bad) d = e = 0xFFFFFFFFu;
        else if (a.mode == FCD_EDIT_GLOBAL) d = L2 > 0 ? (uint32_t)score : (uint32_t)L1, e = (uint32_t)L1;
        else d = L2 > 0 ? (uint32_t)best : 0u, e = L2 > 0 ? (uint32_t)best_end : 0u;
        a.distance[r] = d;
        if (a.end) a.end[r] = e;
    }
}

__global__ __launch_bounds__(64) void envelope_kernel(EnvParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (p.edit) {  // fcd_edit_distance_*: blocks are wavefronts of pairs, not pairs
        switch (p.ed.W) {
            case 1: edit_walk<1>(p.ed, smem); break;
            case 2: edit_walk<2>(p.ed, smem); break;
            case 4: edit_walk<4>(p.ed, smem); break;
            default: edit_walk<8>(p.ed, smem); break;
        }
        return;
    }
    const EnvelopeArgs &a = p.a;
    const int lane = threadIdx.x;
    const int64_t local = blockIdx.x;
    const int64_t r = p.pair_begin + local;

    int64_t T1 = a.T1cap, T2 = a.T2cap;
    if (a.T1) { const int64_t v = a.T1[r]; T1 = v < 0 ? 0 : (v < T1 ? v : T1); }
    if (a.T2) { const int64_t v = a.T2[r]; T2 = v < 0 ? 0 : (v < T2 ? v : T2); }
    int L1 = (int)a.len1[r], L2 = (int)a.len2[r];
    L1 = L1 < 0 ? 0 : (L1 < T1 ? L1 : (int)T1);
    L2 = L2 < 0 ? 0 : (L2 < T2 ? L2 : (int)T2);
    L2 = L2 < a.L2cap ? L2 : (int)a.L2cap;
    const uint8_t *lab1 = a.labels1 + r * a.stride1;
    const uint8_t *lab2 = a.labels2 + r * a.stride2;
    const uint32_t *pth1 = a.path1 + r * a.stride1;
    const uint32_t *pth2 = a.path2 + r * a.stride2;
    uint64_t *dirs = a.dirs + local * a.dirs_stride;
    int32_t *anchor = a.anchor + local * (a.T1cap + 1);
    uint64_t *env = a.env + r * a.env_stride * 2;
    const int nchunk = a.nchunk;

    // LDS: two u16 DP rows of L2cap + 1 entries (L2cap = the batch's longest read-2 labelling), then
    // the labels of read 2
    const int rowlen = (int)a.L2cap + 1;
    uint16_t *prev = reinterpret_cast<uint16_t *>(smem);
    uint16_t *cur = prev + rowlen;
    uint8_t *s2 = reinterpret_cast<uint8_t *>(cur + rowlen);

    for (int64_t t = lane; t <= T1; t += kWave) anchor[t] = -1;
    for (int j = lane; j <= L2; j += kWave) prev[j] = (uint16_t)j;
    for (int j = lane; j < L2; j += kWave) s2[j] = lab2[j];
    wave_sync();

    // ---- 1. edit-distance rows ----
    int lab_reg = 0;
    for (int i = 1; i <= L1; ++i) {
        if (((i - 1) & 63) == 0) lab_reg = (i - 1 + lane < L1) ? lab1[i - 1 + lane] : 0;
        const int la = __shfl(lab_reg, (i - 1) & 63);
        int carry = i;  // D[i][0] - 0
        if (lane == 0) cur[0] = (uint16_t)i;
        const int nact = (L2 + 63) >> 6;
        for (int c = 0; c < nact; ++c) {
            const int j = c * 64 + lane + 1;
            const bool act = j <= L2;
            const int jj = act ? j : 1;
            const int up = (int)prev[jj] + 1;
            const int dg = (int)prev[jj - 1] + ((int)s2[jj - 1] != la ? 1 : 0);
            const int e = up < dg ? up : dg;
            int f = act ? e - j : kBig;
            f = wave_prefix_min(f);
            f = f < carry ? f : carry;
            const int d = f + j;
            carry = __shfl(f, 63);
            const uint64_t m_diag = ballot(act && d == dg);
            const uint64_t m_up = ballot(act && d == up);
            if (lane == 0) {
                uint64_t *q = dirs + ((int64_t)(i - 1) * nchunk + c) * 2;
                q[0] = m_diag;
                q[1] = m_up;
            }
            if (act) cur[j] = (uint16_t)d;
        }
        wave_sync();
        uint16_t *tmp = prev;
        prev = cur;
        cur = tmp;
    }

    // ---- 2. traceback: one lane chases the decisions; matches of equal labels become anchors ----
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0) {
        int i = L1, j = L2;
        while (i > 0 && j > 0) {
            const uint64_t *q = dirs + ((int64_t)(i - 1) * nchunk + ((j - 1) >> 6)) * 2;
            const uint64_t md = load_u64_l2(q), mu = load_u64_l2(q + 1);
            const int bit = (j - 1) & 63;
            if ((md >> bit) & 1ull) {
                if (lab1[i - 1] == s2[j - 1]) {
                    const uint32_t t1 = pth1[i - 1];
                    if (t1 > 0 && (int64_t)t1 <= T1) anchor[t1] = (int32_t)pth2[j - 1];
                }
                --i;
                --j;
            } else if ((mu >> bit) & 1ull) {
                --i;
            } else {
                --j;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (T1 <= 0) return;

    // ---- 3a. next anchor time for every row (suffix minimum), parked in env[i].hi ----
    const int band = (int)a.band;
    {
        int carry = (int)T1;  // the closing anchor (T1, T2)
        const int nrow = (int)((T1 + 63) >> 6);
        for (int c = nrow - 1; c >= 0; --c) {
            // lane k handles row c*64 + 63 - k so that a prefix scan over lanes is a suffix scan over rows
            const int i = c * 64 + 63 - lane;
            const bool act = i < T1;
            // "next" = smallest anchored time strictly greater than i
            int v = kBig;
            if (act && i + 1 < T1 && load_i32_l2(&anchor[i + 1]) >= 0) v = i + 1;
            v = wave_prefix_min(v);
            // exclusive over rows > i already, because row i looked at time i + 1
            v = v < carry ? v : carry;
            carry = __shfl(v, 63);
            if (act) env[(int64_t)i * 2 + 1] = (uint64_t)v;
        }
    }
    wave_sync();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // ---- 3b. previous anchor (prefix maximum), interpolation, band, row contiguity ----
    {
        int carry_t = 0;        // the opening anchor (0, 0)
        int carry_hi = 0;       // hi of the last row of the previous chunk
        const int nrow = (int)((T1 + 63) >> 6);
        for (int c = 0; c < nrow; ++c) {
            const int i = c * 64 + lane;
            const bool act = i < T1;
            int v = -kBig;  // "previous" = largest anchored time <= i (time 0 is never anchored)
            if (act && i > 0 && load_i32_l2(&anchor[i]) >= 0) v = i;
            v = -wave_prefix_min(-v);
            v = v > carry_t ? v : carry_t;
            carry_t = __shfl(v, 63);
            const int ta = v;
            const int ua = ta > 0 ? load_i32_l2(&anchor[act ? ta : 0]) : 0;
            const int tb = act ? (int)load_u64_l2(&env[(int64_t)i * 2 + 1]) : (int)T1;
            const int ub = tb < T1 ? load_i32_l2(&anchor[tb]) : (int)T2;
            const int64_t num = (int64_t)(i - ta) * (int64_t)(ub - ua);
            const int den = tb - ta > 0 ? tb - ta : 1;
            const int cc = ua + (int)(num / den);  // num >= 0: floor
            int lo = cc - band;
            lo = lo < 0 ? 0 : lo;
            int hi = cc + band + 1;
            hi = hi > T2 ? (int)T2 : hi;
            if (i == 0) lo = 0;
            if (i == T1 - 1) hi = (int)T2;
            int hprev = __shfl_up(hi, 1);
            if (lane == 0) hprev = carry_hi;
            if (i > 0 && lo > hprev) lo = hprev;
            carry_hi = __shfl(hi, 63);
            if (act) {
                env[(int64_t)i * 2] = (uint64_t)lo;
                env[(int64_t)i * 2 + 1] = (uint64_t)hi;
            }
        }
    }
}

}  // namespace

size_t envelope_lds_bytes(int64_t L2cap) { return (size_t)(2 * (L2cap + 1) * 2 + L2cap + 16); }

namespace {
__global__ void max_u32_kernel(const uint32_t *a, const uint32_t *b, int64_t n, uint32_t *out2) {
    uint32_t ma = 0, mb = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        ma = max(ma, a[i]);
        mb = max(mb, b[i]);
    }
    atomicMax(&out2[0], ma);
    atomicMax(&out2[1], mb);
}
}  // namespace

// out2[0] = max(a), out2[1] = max(b); out2 must be zeroed by the caller
hipError_t launch_max_u32(const uint32_t *a, const uint32_t *b, int64_t n, uint32_t *out2, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 256);
    hipLaunchKernelGGL(max_u32_kernel, dim3(blocks), dim3(256), 0, stream, a, b, n, out2);
    return hipGetLastError();
}

hipError_t launch_envelope(const EnvelopeArgs &a, int64_t pair_begin, int64_t n_pairs, hipStream_t stream) {
    if (n_pairs <= 0) return hipSuccess;
    EnvParams p{a, pair_begin, EditArgs{}, 0};
    hipLaunchKernelGGL(envelope_kernel, dim3((unsigned)n_pairs), dim3(64), envelope_lds_bytes(a.L2cap), stream, p);
    return hipGetLastError();
}

// the tier of a cap on sequence 2: W blocks per lane up to 512 labels, then groups of 2, 4, .. 64 lanes of eight blocks
void edit_tier(int64_t cap2, int *W, int *gshift) {
    int w = 1, gs = 0;
    while (w < 8 && (int64_t)w * 64 < cap2) w *= 2;
    while (gs < 6 && ((int64_t)512 << gs) < cap2) ++gs;
    *W = w;
    *gshift = gs;
}

// one wavefront per block, 64 >> gshift pairs in each; LDS: the text tile
hipError_t launch_edit_distance(const EditArgs &a, hipStream_t stream) {
    if (a.n_pairs <= 0) return hipSuccess;
    const int npw = kWave >> a.gshift;
    const int64_t blocks = (a.n_pairs + npw - 1) / npw;
    if (blocks > INT_MAX) return hipErrorInvalidValue;
    EnvParams p{EnvelopeArgs{}, 0, a, 1};
    hipLaunchKernelGGL(envelope_kernel, dim3((unsigned)blocks), dim3(64), 64 * kEditTilePitch, stream, p);
    return hipGetLastError();
}

}  // namespace fcd
