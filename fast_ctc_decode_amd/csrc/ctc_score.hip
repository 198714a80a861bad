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
//   score_lds_kernel     wider windows: alpha double-buffered in LDS (circular), up to 1024 work-items.  The same
//                        instantiation carries the two walks of fcd_set_ctc_occupancy_wide (the forward step storing its
//                        rows, and the backward walk that turns them into occupancies), chosen per launch: see below.
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

// ---- motif occurrence posteriors: the forward sum free at both ends (fcd_ctc_detect_*, include/fcd.h) ----
// The walk is the score's over the rows [b, e) of the read and the states 1 .. 2L - 1 (window_k<true>), with
//   entry  state 0 is no cell: its slot holds g_t * 2^-eacc, g_b = 1 and g_t = max(0, 1 - p[t-1][y_0]) under collapse (1
//          without), written after row t - 1's rescale from the tile that row was read from.  Like ctc_align.hip's pinned
//          state a TRUE 1 (not g) takes part in the row maximum: with posteriors <= 1 the cells are probabilities of disjoint
//          events, eacc stays at 1 - kTarget, and a cell below 2^-245 as a probability is below f32's range and counts as 0.
//   exit   v_t = a_t[2L - 1] is read with one readlane; c_t = v_t * h_t, h_t = max(0, 1 - p[t+1][y_{L-1}]) under collapse,
//          needs the NEXT row: (v_t, eacc) wait in two registers (across a tile boundary too) and c_t is completed at row
//          t + 1, the range's last row at once with h = 1.
// Every c_t, in row order: added to a float64 sum (ldexp by the row's exponent: exact), compared with the running best as
// (exponent, mantissa) -- a later row only if strictly greater, no logarithm -- and, with a track, kept as a pair by
// work-item t mod 64 until 64 rows are stored at once (ctc_align.hip's spot_row).  Wave-uniform but for that pair.
constexpr uint32_t kNoHit = 0xFFFFFFFFu;
constexpr float kLn2f = 0.693147180559945309f;

struct Detect {
    double sum;  // c_b + .. so far
    float bm;    // the best c so far, normalised: mantissa in [0.5, 1) ...
    int be;      // ... its exponent in true scale ...
    int bt;      // ... and its row (of the range); -1: none yet
    float vp;    // v of the row before, in that row's units ...
    int ep;      // ... 2^ep
    float tm;    // lane j: the pair of row c0 + j of the 64 rows of `track` being staged
    int te;
};

// max(0, 1 - p) of a staged posterior (one f32 rounding)
__device__ __forceinline__ float one_minus(const Lds &lds, int at) {
    return fmaxf(0.0f, 1.0f - ldexpf(lds.pm[at], lds.pe[at]));
}

// state 0's slot in the walk's units (eacc is at least 1 - kTarget in a free-ended walk, and an int)
__device__ __forceinline__ float entry_cell(float g, int64_t eacc) {
    const int e = (int)eacc;
    return ldexpf(g, e > 512 ? -512 : -e);
}

// c_t = c * 2^e is complete (t: row of the range)
__device__ __forceinline__ void detect_cell(const DetectOut *det, Detect &dt, float c, int e, int t, int Tr, int tb) {
    float m = 0.0f;
    int ex = 0;
    if (c > 0.0f && c - c == 0.0f) {
        dt.sum += ldexp((double)c, e);
        m = frexpf(c, &ex);
        ex += e;
        if (dt.bt < 0 || ex > dt.be || (ex == dt.be && m > dt.bm)) {
            dt.bm = m;
            dt.be = ex;
            dt.bt = t;
        }
    }
    float *track = det->track;
    if (track) {
        const int j = threadIdx.x;
        if (j == (t & 63)) {
            dt.tm = m;
            dt.te = ex;
        }
        if ((t & 63) == 63 || t == Tr - 1) {
            const int c0 = t & ~63;
            if (j < 64 && c0 + j <= t)
                track[(int64_t)blockIdx.x * det->track_stride + tb + c0 + j] =
                    dt.tm > 0.0f ? fmaf((float)dt.te, kLn2f, logf(dt.tm)) : -INFINITY;
        }
    }
}

// row t of the range is done: v, its cell of state 2L - 1 in units 2^eacc; h, the exit weight of the row BEFORE, which
// is completed now (the range's last row: by detect_finish)
__device__ __forceinline__ void detect_row(const DetectOut *det, Detect &dt, float v, int64_t eacc, float h, int t, int Tr, int tb) {
    if (t > 0) detect_cell(det, dt, dt.vp * h, dt.ep, t - 1, Tr, tb);
    dt.vp = v;
    dt.ep = (int)eacc;
}

// a row that does not walk: its logp is written already (NaN, -inf, or 0 for an empty motif)
__device__ __forceinline__ void no_detect(const ScoreParams &p, const DetectOut *det) {
    if (threadIdx.x == 0) {
        const double lp = p.logp[blockIdx.x];
        det->count[blockIdx.x] = lp != lp ? lp : 0.0;
        det->end[blockIdx.x] = kNoHit;
    }
}

__device__ __forceinline__ void detect_finish(const ScoreParams &p, const DetectOut *det, const Lds &lds, Detect &dt, int Tr, int tb) {
    detect_cell(det, dt, dt.vp, dt.ep, Tr - 1, Tr, tb);  // the last row: h = 1
    if (threadIdx.x == 0) {
        const bool bad = lds.misc[kBadPost] != 0;
        p.logp[blockIdx.x] = bad ? (double)NAN : (dt.bt < 0 ? -(double)INFINITY : ln_p((double)dt.bm, dt.be));
        det->count[blockIdx.x] = bad ? (double)NAN : dt.sum;
        det->end[blockIdx.x] = bad || dt.bt < 0 ? kNoHit : (uint32_t)(tb + dt.bt);
    }
}

// ---- the register-resident window ----
// DETECT: `det` non-null as a compile-time copy -- the kernel branches on it ONCE, so that a score's rows run the
// instructions they ran before the detecting walk existed
template <int K, bool DETECT>
__device__ __forceinline__ void score_reg_walk(const ScoreParams &p, const DetectOut *det, unsigned char *smem) {
    constexpr int C = 64 * K;
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    int tb = 0;  // (detecting: the first row of the range)
    if (DETECT) {
        if (!prologue(p, lds, &rw) || !row_range(p, det->row_begin, det->row_end, &rw, &tb)) return no_detect(p, det);
    } else {
        if (!prologue(p, lds, &rw)) return;
    }
    const int lane = threadIdx.x;
    float a[K];  // alpha of the lane's K states, scaled by 2^-eacc
#pragma unroll
    for (int r = 0; r < K; ++r) a[r] = 0.0f;
    if (lane == 0) a[0] = 1.0f;  // "row -1": all mass on state 0, so that row 0 comes out as p[0][0], p[0][y0]
    int64_t eacc = 0;
    int lo_prev = 0, lo = 0, hi = 0;
    Detect dt{0.0, 0.0f, 0, -1, 0.0f, 0, 0.0f, 0};
    // (detecting: lo stays 1) the first and the last label, and where state 2L - 1 lives
    const int y_first = DETECT ? lds.lab[0] & 0xFF : 0, y_last = DETECT ? lds.lab[rw.L - 1] & 0xFF : 0;
    const int end_lane = DETECT ? (2 * rw.L - 1) / K : 0, end_r = DETECT ? (2 * rw.L - 1) % K : 0;
    if (DETECT && lane == 0) lds.misc[kBadPost] = 0;
    for (int t0 = 0; t0 < rw.Tr; t0 += rw.rows_per_tile) {
        const int rc = min(rw.rows_per_tile, rw.Tr - t0);
        if (DETECT) fill_tile_checked(p, lds, rw, t0, rc);
        else fill_tile(p, lds, rw, t0, rc);
        StepIn<K> in = load_step<K, DETECT>(p, lds, rw, t0, 0);
        for (int i = 0; i < rc; ++i) {
            StepIn<K> nx = in;
            if (i + 1 < rc) nx = load_step<K, DETECT>(p, lds, rw, t0 + i + 1, i + 1);
            float g = 1.0f, h = 1.0f;  // (detecting) the entry weight of the NEXT row, the exit weight of the row BEFORE
            if (DETECT && p.collapse) {
                g = one_minus(lds, i * rw.N + y_first);
                h = one_minus(lds, i * rw.N + y_last);
            }
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
                if (DETECT) FCD_OPAQUE_VQ(u[r]);  // (the detecting copy's cells stay scalar f32 operations: see score_reg_kernel)
                const int e = finite_exp(u[r]);
                emax = max(emax, ((in.in_mask >> r) & 1) && e != kNoExp ? e + ex[r] : kNoExp);
            }
            if (DETECT) emax = max(emax, 1 - (int)eacc);  // state 0's 1: 2^-eacc in the units the row was computed in
            emax = wave_imax(emax);
            const int sh = emax == kNoExp ? 0 : kTarget - emax;
            eacc -= sh;
#pragma unroll
            for (int r = 0; r < K; ++r)
                a[r] = ((in.in_mask >> r) & 1) ? ldexpf(u[r], min(max(ex[r] + sh, -512), 512)) : 0.0f;
            if (DETECT) {
                if (lane == 0) a[0] = entry_cell(g, eacc);  // the slot of state 0 (outside the window: no cell), after the rescale
                float mine = 0.0f;
#pragma unroll
                for (int r = 1; r < K; r += 2)
                    if (r == end_r) mine = a[r];
                const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), end_lane));
                detect_row(det, dt, v, eacc, h, t0 + i, rw.Tr, tb);
            }
            lo_prev = lo;
            in = nx;
        }
    }
    if (DETECT) return detect_finish(p, det, lds, dt, rw.Tr, tb);
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

// ---- the packed detecting walk: one (read, motif) pair per LANE (fcd_set_ctc_detect_packed, include/fcd.h) ----
// M short motifs shared by all reads.  Lane q * Mp + m of a wavefront walks motif m of the wavefront's read slot q (Mp: M
// rounded up to a power of two, R = 64 / Mp slots; beyond 32 motifs one read and a block of 64 motifs), every cell of its
// lattice in a register of its own: a[0] is state 0's pinned g * 2^-E, a[s] state s <= 2L - 1, updated in place from the
// highest state down -- no value crosses a lane in the row loop.  States above 2L - 1 hold garbage nothing reads: a state
// only feeds the states above it, v_t is picked by a select on L, the maximum is masked.
//   rows   relative: row i of every lane is row b_r + i of its own read's range.  The wavefront stages, per slot, the next
//          rows of that slot's range as plain f32 (load_post: exact f16 / bf16, 64-bit offsets, any strides) at
//          tile[q * S + i * N + j], S = 31 * 64 / R words: the N values of a row lie in N consecutive banks, the rows of
//          the slots start 64 / R banks apart (-q * 64 / R mod 64; R = 64: 31 q mod 64, a permutation).  A NaN, infinite or
//          negative value sets the SLOT's word: a bad read leaves the reads next to it alone.  A lane whose range is over
//          sits out the rest under its predicate; the pending c of its last row is completed behind the loop with h = 1.
//   scale  a cell is value * 2^-E with a per-lane integer E; state 0's 1 starts as 2^64 (E = -64), so a cell stays a normal
//          f32 down to 2^-190 as a probability.  With posteriors <= 1 a row grows max(cells, 2^-E) at most threefold, so the
//          lane looks at that maximum every kPackCheck = 32 rows only (3^32 < 2^51: below 2^116 from [2^64, 2^65)) and
//          multiplies cells, pinned value and 2^-E by the power of two that puts it back: exact.  Where rows that do not
//          sum to 1 outgrow f32, E carries them; once 2^-E leaves f32 (values beyond 2^213) a fresh start counts as 0.
//   result detect_cell's arithmetic per lane: count a float64 sum in row order, the best c as (mantissa, exponent, row),
//          a later row only if strictly greater, one ln at the end; each lane stores its own three values.
// The cell arithmetic is the wave-wide walk's -- (a[s] + a[s-1] + a[s-2]) * p, one rounding each -- so its bound holds.
constexpr int kPackLabels = 24;   // 47 cells: the K = 2 instantiation stays under its 96 VGPRs (the resource report)
constexpr int kPackCheck = 32;    // rows between two looks at a lane's maximum
constexpr int kPackUnit = 65;     // frexp exponent the maximum is put back to: [2^64, 2^65)
constexpr int kPackTileWords = 31 * 64;  // of the 2048 words of pm / pe; the 64 behind them: the slots' bad-posterior words

constexpr int kPackGroup = 4;     // labels whose posteriors are read from the tile at a time
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: plain C++)
#define FCD_PACK_FENCE(x, y) ((void)0)
#else
#define FCD_PACK_FENCE(x, y) asm("" : "+v"(x), "+v"(y))
#endif

struct PackBest {
    double sum;
    float bm;
    int be, bt;
};

__device__ __forceinline__ void pack_cell(PackBest &r, float c, int e, int t) {
    if (c > 0.0f && c - c == 0.0f) {
        r.sum += ldexp((double)c, e);
        int ex;
        const float m = frexpf(c, &ex);
        ex += e;
        if (r.bt < 0 || ex > r.be || (ex == r.be && m > r.bm)) {
            r.bm = m;
            r.be = ex;
            r.bt = t;
        }
    }
}

// the rows [b, b + rows) of `read` that its motifs are looked for in (row_range's clamping); rows = 0 beyond the batch
__device__ __forceinline__ void pack_range(const ScoreParams &p, const DetectOut *det, int64_t read, int *b, int *rows) {
    *b = *rows = 0;
    if (read >= p.in.n_reads) return;
    int64_t Tr = p.in.lengths ? p.in.lengths[read] : p.in.T;
    Tr = Tr < 0 ? 0 : (Tr > p.in.T ? p.in.T : Tr);
    const int lo = det->row_begin ? (int)min((int64_t)det->row_begin[read], Tr) : 0;
    const int hi = det->row_end ? (int)min((int64_t)det->row_end[read], Tr) : (int)Tr;
    *b = lo;
    *rows = max(hi - lo, 0);
}

template <bool COLLAPSE>
__device__ __forceinline__ void pack_walk(const ScoreParams &p, const DetectOut *det, unsigned char *smem) {
    constexpr int NL = kPackLabels, NW = (NL + 3) / 4, GS = kPackGroup;
    static_assert(NL % GS == 0 && NL <= 32, "whole groups; the select tree has five levels");
    float *tile = reinterpret_cast<float *>(smem);
    int *badw = reinterpret_cast<int *>(smem) + kPackTileWords;
    int *slot_rows = reinterpret_cast<int *>(smem + kTileElems * 8);  // (krow's 64 words)
    const int lane = threadIdx.x, N = p.in.N, M = det->pack_m, R = det->pack_reads;
    const int G = 64 / R, S = 31 * G, rpt = min(kTileRows, S / N);  // lanes and words of a slot, rows of a tile
    const int Mp = M > 32 ? 64 : G;                                 // (the host takes fewer slots where N wants longer rows)
    const int nblk = (M + 63) >> 6;
    const int64_t group = blockIdx.x / nblk;
    {  // ---- the slot this lane stages (lane / G: its G lanes write the same value)
        int b_s, rows_s;
        pack_range(p, det, group * R + lane / G, &b_s, &rows_s);
        slot_rows[lane / G] = rows_s;
        badw[lane / G] = 0;
    }
    // ---- the pair this lane walks
    const int q = lane / Mp, m = (int)(blockIdx.x - group * nblk) * 64 + (lane - q * Mp);
    const int64_t read = group * R + q;
    const bool mine = q < R && m < M && read < p.in.n_reads;
    int b = 0, rows = 0, L = 0;
    uint32_t w[NW], dmask = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = 0;
    double early = (double)NAN;
    if (mine) {
        pack_range(p, det, read, &b, &rows);
        const uint32_t len = det->pack_len[m];
        const uint8_t *lab = det->pack_labels + (int64_t)m * p.y.stride;
        bool bad = (int64_t)len > p.y.stride || len > (uint32_t)NL;
        L = bad ? 0 : (int)len;
        int yp = 0;
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            if (k < L) {
                const int y = lab[k];
                bad |= y < 1 || y >= N;
                w[k >> 2] |= (uint32_t)y << (8 * (k & 3));
                dmask |= (k > 0 && (!COLLAPSE || y != yp) ? 1u : 0u) << k;
                yp = y;
            }
        }
        if (!bad) early = L == 0 ? 0.0 : -(double)INFINITY;
        if (bad) L = 0;
    }
    const bool walks = mine && L > 0 && L <= rows;
    if (mine && !walks) {
        const int64_t out = read * M + m;  // a pair without a value: NaN; no motif: 0; more labels than rows: -inf
        p.logp[out] = early;
        det->count[out] = early != early ? early : 0.0;
        det->end[out] = kNoHit;
    }
    const int nrows = walks ? rows : 0;
    if (!walks) {
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = 0;
    }
    // L, the first and the last label in one register (unpacked again in every row: three registers fewer across the loop)
    uint32_t meta = (uint32_t)L | (w[0] & 0xFF) << 8;
#pragma unroll
    for (int k = 0; k < NL; ++k)
        if (walks && k == L - 1) meta |= ((w[k >> 2] >> (8 * (k & 3))) & 0xFF) << 16;
    __syncthreads();
    int most = 0;
    for (int s = 0; s < R; ++s) most = max(most, slot_rows[s]);
    most = __builtin_amdgcn_readfirstlane(most);  // (the same in every lane)
    float a[2 * NL];
#pragma unroll
    for (int s = 0; s < 2 * NL; ++s) a[s] = 0.0f;
    int E = 1 - kPackUnit;
    a[0] = ldexpf(1.0f, -E);  // state 0's 1
    PackBest best{0.0, 0.0f, 0, -1};
    float vp = 0.0f;
    const float *slot = tile + (walks ? q : 0) * S;
    // (from here to the results the lane keeps its cells, labels, meta, nrows, slot and the running result: nothing else)
    for (int i0 = 0; i0 < most; i0 += rpt) {
        __syncthreads();  // the tile's readers are done
        {  // (what staging needs is worked out again for every tile: it holds no register while the rows are walked)
            int ln = lane;
            FCD_OPAQUE_VQ(ln);
            const int qs = ln / G, sub = ln - qs * G;
            int b_s, rows_s;
            pack_range(p, det, group * R + qs, &b_s, &rows_s);
            const float *post_s = post_at(p.in.post, (group * R + qs) * p.in.stride_read + (int64_t)b_s * p.in.stride_t, p.in.dtype);
            const int di = G / N, dj = G - di * N;
            const int cnt = min(rpt, rows_s - i0) * N;
            bool bad = false;
            int i = sub / N, j = sub - i * N;
            for (int e = sub; e < cnt; e += G) {
                const float v = load_post(post_s, (int64_t)(i0 + i) * p.in.stride_t + (int64_t)j * p.in.stride_n, p.in.dtype);
                bad |= !(v >= 0.0f && v - v == 0.0f);
                tile[qs * S + e] = v;
                i += di;
                j += dj;
                if (j >= N) {
                    j -= N;
                    ++i;
                }
            }
            if (bad) badw[qs] = 1;
        }
        __syncthreads();
        const int rc = min(rpt, most - i0);
        for (int i = 0; i < rc; ++i) {
            const int t = i0 + i;
            if (t < nrows) {
                const float *row = slot + i * N;
                const float p0 = row[0];
                FCD_OPAQUE_VQ(meta);
                const int L = meta & 0xFF, last = 2 * L - 1, y_first = (meta >> 8) & 0xFF, y_last = meta >> 16;
                if (t > 0) pack_cell(best, COLLAPSE ? vp * fmaxf(0.0f, 1.0f - row[y_last]) : vp, E, t - 1);  // c of the row before
                if (t > 0 && (t & (kPackCheck - 1)) == 0) {  // (behind it: the cells, v among them, share ONE exponent)
                    float mx = ldexpf(1.0f, max(-E, -200));
#pragma unroll
                    for (int s = 1; s < 2 * NL; ++s) mx = fmaxf(mx, s <= last ? a[s] : 0.0f);
                    int ex;
                    (void)frexpf(mx, &ex);
                    const int sh = mx > 0.0f && mx - mx == 0.0f ? min(max(kPackUnit - ex, -100), 100) : 0;
                    if (sh != 0) {
                        const float f = ldexpf(1.0f, sh);
#pragma unroll
                        for (int s = 0; s < 2 * NL; ++s) a[s] *= f;
                        E -= sh;
                    }
                }
                const float g = COLLAPSE ? fmaxf(0.0f, 1.0f - row[y_first]) : 1.0f;  // the entry weight of the NEXT row
                // (kept from hoisting 24 LDS offsets out of the time loop, into registers the cells need)
#pragma unroll
                for (int k = 0; k < NW; ++k) FCD_OPAQUE_VQ(w[k]);
                FCD_OPAQUE_VQ(dmask);
                // the labels' posteriors kPackGroup at a time, a group ahead of its use: the reads of group n + 1 wait for
                // the cells of group n - 1 (the fence), so that two groups' values are live, not 24
                int at = i * N;
                float pn[GS], pc[GS];
#pragma unroll
                for (int c = 0; c < GS; ++c) pn[c] = slot[at + ((w[(NL - 1 - c) >> 2] >> (8 * ((NL - 1 - c) & 3))) & 0xFF)];
#pragma unroll
                for (int k1 = NL - 1; k1 >= 0; k1 -= GS) {
#pragma unroll
                    for (int c = 0; c < GS; ++c) pc[c] = pn[c];
                    if (k1 - GS >= 0) {
                        if (k1 + 1 < NL) FCD_PACK_FENCE(at, a[2 * k1 + 2]);
#pragma unroll
                        for (int c = 0; c < GS; ++c) pn[c] = slot[at + ((w[(k1 - GS - c) >> 2] >> (8 * ((k1 - GS - c) & 3))) & 0xFF)];
                    }
                    // (every sum reads cells of the row before only: unfenced, all 47 are formed ahead of the first write)
                    if (k1 + 1 < NL) FCD_PACK_FENCE(a[2 * k1 + 1], a[2 * k1 + 2]);
#pragma unroll
                    for (int c = 0; c < GS; ++c) {
                        const int k = k1 - c, s = 2 * k + 1;
                        float sum = COLLAPSE ? a[s] + a[s - 1] : a[s - 1];
                        if (k > 0) sum += ((dmask >> k) & 1) ? a[s - 2] : 0.0f;
                        a[s] = sum * pc[c];
                        FCD_OPAQUE_VQ(a[s]);  // (scalar f32 operations: packed ones want register pairs the cells cannot spare)
                        if (k > 0) {
                            a[s - 1] = (a[s - 1] + a[s - 2]) * p0;
                            FCD_OPAQUE_VQ(a[s - 1]);
                        }
                    }
                }
                // v = a[2L - 1]: a tree of selects on the five bits of L - 1
                float v;
                {
                    float x[32];
#pragma unroll
                    for (int k = 0; k < 32; ++k) x[k] = k < NL ? a[2 * k + 1] : 0.0f;
#pragma unroll
                    for (int bit = 0; bit < 5; ++bit) {
                        const bool up = ((L - 1) >> bit) & 1;
#pragma unroll
                        for (int k = 0; k < (16 >> bit); ++k) x[k] = up ? x[2 * k + 1] : x[2 * k];
                    }
                    v = x[0];
                }
                vp = v;
                a[0] = ldexpf(g, max(-E, -200));
            }
        }
    }
    if (nrows > 0) {  // (the lane walked: who it is, worked out again)
        pack_cell(best, vp, E, nrows - 1);  // the last row: h = 1
        int ln = lane;
        FCD_OPAQUE_VQ(ln);
        const int q = ln / Mp, m = (int)(blockIdx.x - group * nblk) * 64 + (ln - q * Mp);
        const int64_t read = group * R + q, out = read * M + m;
        int b, rows;
        pack_range(p, det, read, &b, &rows);
        const bool bad = badw[q] != 0;
        p.logp[out] = bad ? (double)NAN : (best.bt < 0 ? -(double)INFINITY : ln_p((double)best.bm, best.be));
        det->count[out] = bad ? (double)NAN : best.sum;
        det->end[out] = bad || best.bt < 0 ? kNoHit : (uint32_t)(b + best.bt);
    }
}

// Both copies live in one kernel, so every launch, scores included, reserves the detecting copy's registers (63 / 73 /
// 83 / 94 VGPRs at K = 2 / 4 / 6 / 8 against the score copy's 28 / 40 / 50 / 60).  8.6 KiB of LDS a one-wavefront
// workgroup hold the kernel at 18 workgroups a CU, 4.5 wavefronts a SIMD, so five wavefronts a SIMD are all a score can
// use: amdgpu_waves_per_eu(5) makes the compiler keep both copies within the 96 VGPRs that allow them (it spills, and
// the resource report shows scratch, before a later change can take wavefronts from a score unnoticed).
// The detecting copy's cells go through FCD_OPAQUE_VQ: the compiler forms no packed f32 operations (v_pk_add_f32,
// v_pk_mul_f32) in that copy; the score copy keeps the 3 / 6 / 9 / 12 it had.
// K = 2 also carries the packed detecting walk (pack_walk): 91 VGPRs, no scratch, chosen once at the kernel's top by the
// parameter block's pack_reads; the other three instantiations do not compile it.
template <int K>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5))) void score_reg_kernel(ScoreParams p, const DetectOut *det) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if constexpr (K == 2) {  // (the packed walk: in the instantiation short motifs launch anyway, the one with the most registers to spare)
        if (det && det->pack_reads) return p.collapse ? pack_walk<true>(p, det, smem) : pack_walk<false>(p, det, smem);
    }
    if (det) score_reg_walk<K, true>(p, det, smem);
    else score_reg_walk<K, false>(p, det, smem);
}

// ---- the LDS-resident window ----
// One kernel, four walks, chosen once per block by LdsWalkParams::walk before any time loop (the instantiation ledger
// admits no new kernel symbol, as PostParams::walk of ctc_posterior.hip):
//   kLdsScore  fcd_ctc_score_*: the forward sum.
//   kLdsStore  the same forward step; every live cell of row t also goes to the workspace by slot (s mod cap, as in LDS),
//              scaled by 2^-kAlphaDown (exact), and the row's exponent word behind the T * cap cells, as post_fwd_kernel
//              stores the register window's rows.  logp is kLdsScore's bit for bit.
//   kLdsOcc    fcd_ctc_occupancy_* under fcd_set_ctc_occupancy_wide: rows T_r - 1 .. 0 (lds_occ_walk below).
//   kLdsDetect fcd_ctc_detect_* of motifs beyond 254 labels: the forward step free-ended (the detecting walk above: state 0's
//              slot is alpha[0] of the buffer a row writes, v_t is read back from that buffer behind the row's barrier).
struct LdsWalkParams {
    ScoreParams s;
    int walk;
    float *alpha;  // (kLdsStore, kLdsOcc) the stored forward rows, alpha_words per labelling of this launch
    int64_t alpha_words;
    // (kLdsOcc) a (T, N) block per labelling of this launch, at row * occ_stride_row + t * occ_stride_t
    float *occ;
    int64_t occ_stride_row, occ_stride_t;
    float occ_scale;
    int occ_accumulate;
    const DetectOut *detect;  // (kLdsDetect) null in every other walk
};
constexpr int kLdsScore = 0, kLdsStore = 1, kLdsOcc = 2, kLdsDetect = 3;
constexpr int kWideCells = 10;  // cells per work-item and step of kLdsOcc: 20 would take the kernel from 77 to 117 VGPRs and
                                // ctc_score's walk from 6 to 4 wavefronts per SIMD; at 10 it stays at 6
constexpr int kWideLabels = 9;         // the blank and the 8 labels
constexpr int kRedWords = 16 * kWideLabels;  // kLdsOcc: a word per wavefront and label behind the two alpha buffers
constexpr int kTargetBack = 60;        // b: row maximum in [2^59, 2^60), as ctc_posterior.hip's kTargetB

template <bool STORE, bool DETECT = false>
__device__ __forceinline__ void lds_forward(const LdsWalkParams &q, unsigned char *smem) {
    // (the detecting copy at the occupancy walks' cells per work-item: at 20 its bookkeeping takes the kernel past 80 VGPRs)
    constexpr int kCells = DETECT ? kWideCells : kLdsCells;
    const ScoreParams &p = q.s;
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    int tb = 0;  // (detecting: the first row of the range)
    if (DETECT) {
        if (!prologue(p, lds, &rw) || !row_range(p, q.detect->row_begin, q.detect->row_end, &rw, &tb)) return no_detect(p, q.detect);
    } else {
        if (!prologue(p, lds, &rw)) return;
    }
    const int tid = threadIdx.x, bd = blockDim.x, cap = p.cap, nw = bd >> 6;
    for (int s = tid; s < 2 * cap; s += bd) lds.alpha[s] = 0.0f;
    __syncthreads();
    if (tid == 0) lds.alpha[0] = 1.0f;  // "row -1": all mass on state 0
    if (DETECT && tid == 0) lds.misc[kBadPost] = 0;
    Detect dt{0.0, 0.0f, 0, -1, 0.0f, 0, 0.0f, 0};
    const int y_first = DETECT ? lds.lab[0] & 0xFF : 0, y_last = DETECT ? lds.lab[rw.L - 1] & 0xFF : 0;
    int64_t eacc = 0;
    int lo_prev = 0, hi_prev = 0, base = 0, which = 0;  // base: the multiple of cap at or below the window's start
    // alpha_{t-1}[n] as the previous row left it: 0 outside that row's window (state n lives at n mod cap)
    auto rd = [&](const float *buf, int n) -> float {
        if (n < lo_prev || n > hi_prev) return 0.0f;
        int idx = n - base;
        idx = idx < 0 ? idx + cap : (idx >= cap ? idx - cap : idx);
        return buf[idx];
    };
    float *am = nullptr;
    int *ae = nullptr;
    if constexpr (STORE) {
        am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
        ae = reinterpret_cast<int *>(am + (int64_t)p.in.T * cap);
    }
    for (int t0 = 0; t0 < rw.Tr; t0 += rw.rows_per_tile) {
        const int rc = min(rw.rows_per_tile, rw.Tr - t0);
        if (DETECT) fill_tile_checked(p, lds, rw, t0, rc);
        else fill_tile(p, lds, rw, t0, rc);
        for (int i = 0; i < rc; ++i) {
            int lo, hi;
            window<DETECT>(p, lds, rw, t0 + i, i, &lo, &hi);
            if (DETECT) FCD_OPAQUE_S(lo);  // (a constant 1: kept from hoisting every cell's label and addresses out of the time loop)
            const float *prev = lds.alpha + which * cap;
            float *next = lds.alpha + (which ^ 1) * cap;
            const float pm0 = lds.pm[i * rw.N];
            const int pe0 = lds.pe[i * rw.N];
            float g = 1.0f, h = 1.0f;  // (detecting) the entry weight of the NEXT row, the exit weight of the row BEFORE
            if (DETECT && p.collapse) {
                g = one_minus(lds, i * rw.N + y_first);
                h = one_minus(lds, i * rw.N + y_last);
            }
            float u[kCells];
            int ex[kCells];
            int emax = kNoExp;
#pragma unroll
            for (int c = 0; c < kCells; ++c) {
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
            if (DETECT) emax = max(emax, 1 - (int)eacc);  // state 0's 1: 2^-eacc in the units the row was computed in
            emax = wave_imax(emax);
            if ((tid & 63) == 0) lds.misc[tid >> 6] = emax;
            __syncthreads();  // every read of `prev` is done, the waves' maxima are in place
            for (int w = 0; w < nw; ++w) emax = max(emax, lds.misc[w]);
            const int sh = emax == kNoExp ? 0 : kTarget - emax;
            eacc -= sh;
            while (lo >= base + cap) base += cap;
            float *row = nullptr;
            if constexpr (STORE) row = am + (int64_t)(t0 + i) * cap;
#pragma unroll
            for (int c = 0; c < kCells; ++c) {
                const int s = lo + tid + c * bd;
                if (s <= hi) {
                    int idx = s - base;
                    idx = idx >= cap ? idx - cap : idx;
                    const float a = ldexpf(u[c], min(max(ex[c] + sh, -512), 512));
                    next[idx] = a;
                    if constexpr (STORE) row[idx] = ldexpf(a, -kAlphaDown);
                }
            }
            if constexpr (STORE) {
                if (tid == 0) ae[t0 + i] = (int)(eacc + kAlphaDown);
            }
            if (DETECT && tid == 0) next[0] = entry_cell(g, eacc);  // state 0 (below the window, base stays 0: no cell), after the rescale
            lo_prev = lo;
            hi_prev = hi;
            which ^= 1;
            __syncthreads();
            if (DETECT) {  // (the next step writes the other buffer: `next` stands until the barrier inside it)
                lo_prev = 0;  // state 0 is read like a cell
                const float mine = 2 * rw.L - 1 <= hi ? next[2 * rw.L - 1] : 0.0f;
                const float v = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mine)));
                detect_row(q.detect, dt, v, eacc, h, t0 + i, rw.Tr, tb);
            }
        }
    }
    if (DETECT) return detect_finish(p, q.detect, lds, dt, rw.Tr, tb);
    if (tid == 0) {
        const float *last = lds.alpha + which * cap;
        write_result(p, rd(last, 2 * rw.L), rd(last, 2 * rw.L - 1), eacc);
    }
}

// The label occupancies of a labelling whose window the registers cannot hold (fcd_set_ctc_occupancy_wide; include/fcd.h):
// ctc_occ_walk of ctc_posterior.hip with the window in LDS.  Row t = T_r - 1 .. 0; b_{t+1} is double-buffered in lds.alpha
// ("row T_r": all mass on state 2L), state n at n mod cap with `base` -- the multiple of cap at or below the stored row's
// first state -- running downward; alpha_t is the stored row of the SAME index, read through row t's own window.  A cell:
//   beta_t[s]  = b_{t+1}[s] [blank, or collapse] + b_{t+1}[s+1] + [allowed] b_{t+1}[s+2]
//   gamma_t[s] = ldexp(alpha_t[s] * beta_t[s], Ea(t) + Eb(t+1) - floor(log2 P)) / mantissa(P)       two roundings
//   b_t[s]     = beta_t[s] * p[t][z[s]]  at the row's own scale
// no fused multiply-add, every term non-negative; where beta is exactly 0 neither the posterior nor alpha is multiplied in.
// occ[t][c] in a fixed order, so that two calls return the same bits: a work-item adds its cells of label c in increasing
// cell order (its cells are kWideCells states blockDim apart -- all of one parity: all blank or all labels), wave_fsum the
// lanes, then the wavefronts' sums -- each in an LDS word of its own -- in wavefront order, by every work-item alike.
// Work-item c < N stores cell c.  No atomics, no clearing pass.  The row-sum check and the give-up rule are ctc_occ_walk's,
// block-uniform, with this walk's depth: lost_w(T_r) = 2 (6 T_r + nw + 34) 2^-24, nw the block's wavefronts.
__device__ __forceinline__ void lds_occ_walk(const LdsWalkParams &q, unsigned char *smem) {
    constexpr int NL = kWideLabels;
    const ScoreParams &p = q.s;
    const Lds lds = carve(smem, p.lab_cap);
    Row rw;
    if (!prologue(p, lds, &rw)) return;  // (the forward launch wrote this row's logp already; the same value again)
    const double lp = p.logp[blockIdx.x];
    if (lp - lp != 0.0) return;  // P = 0, or a NaN on the way: nothing of the block is written
    const int tid = threadIdx.x, bd = blockDim.x, cap = p.cap, nw = bd >> 6, N = rw.N, L = rw.L;
    float *red = lds.alpha + 2 * cap;  // [nw][NL]
    const float *am = q.alpha + (int64_t)blockIdx.x * q.alpha_words;
    const int *ae = reinterpret_cast<const int *>(am + (int64_t)p.in.T * cap);
    float *out = q.occ + (int64_t)blockIdx.x * q.occ_stride_row;
    for (int s = tid; s < 2 * cap; s += bd) lds.alpha[s] = 0.0f;
    __syncthreads();
    int base = 2 * L / cap * cap;
    if (tid == 0) lds.alpha[2 * L - base] = 1.0f;  // "row T_r": all mass on state 2L
    int lo_n = 2 * L, hi_n = 2 * L, which = 0;
    int64_t eb = 0;
    const int64_t xp = (int64_t)floor(lp * 1.44269504088896340735992468100189214);  // floor(log2 P(y | x))
    const float pman = (float)exp(lp - (double)xp * kLn2);                          // P / 2^xp, in [1, 2]
    const float lost = 2.0f * (6.0f * (float)rw.Tr + (float)(nw + 34)) * 5.9604644775390625e-8f;  // lost_w(T_r)
    // b_{t+1}[n] as the row above left it: 0 outside that row's window
    auto rd = [&](const float *buf, int n) -> float {
        if (n < lo_n || n > hi_n) return 0.0f;
        int idx = n - base;
        idx = idx >= cap ? idx - cap : idx;
        return buf[idx];
    };
    for (int t0 = (rw.Tr - 1) / rw.rows_per_tile * rw.rows_per_tile; t0 >= 0; t0 -= rw.rows_per_tile) {
        const int rc = min(rw.rows_per_tile, rw.Tr - t0);
        fill_tile(p, lds, rw, t0, rc);
        for (int i = rc - 1; i >= 0; --i) {
            const int t = t0 + i;
            int lo, hi;
            window(p, lds, rw, t, i, &lo, &hi);
            const float *above = lds.alpha + which * cap;
            float *mine = lds.alpha + (which ^ 1) * cap;
            const float *arow = am + (int64_t)t * cap;
            // the exponent of this row's terms: alpha of row t times b of row t + 1, over 2^floor(log2 P)
            const int dt = (int)min(max((int64_t)ae[t] + eb - xp, (int64_t)-512), (int64_t)512);
            int nbase = base;  // this row's: at or below lo
            while (lo < nbase) nbase -= cap;
            const float pm0 = lds.pm[i * N];
            const int pe0 = lds.pe[i * N];
            float u[kWideCells], acc[NL];
            int ex[kWideCells];
            int emax = kNoExp;
#pragma unroll
            for (int c = 0; c < NL; ++c) acc[c] = 0.0f;
#pragma unroll
            for (int c = 0; c < kWideCells; ++c) {
                const int s = lo + tid + c * bd;
                u[c] = 0.0f;
                ex[c] = 0;
                if (s <= hi) {
                    const float y0 = rd(above, s), y1 = rd(above, s + 1);
                    float sum, pm;
                    int z = 0;
                    if (s & 1) {
                        const int k = s >> 1;
                        const int info = lds.lab[k], inext = lds.lab[min(k + 1, max(L - 1, 0))];
                        z = info & 0xFF;
                        sum = p.collapse ? y0 + y1 : y1;
                        if (k + 1 < L && (!p.collapse || (inext & 0x100))) sum += rd(above, s + 2);
                        pm = lds.pm[i * N + z];
                        ex[c] = lds.pe[i * N + z];
                    } else {
                        sum = y0 + y1;
                        pm = pm0;
                        ex[c] = pe0;
                    }
                    if (sum != 0.0f) {  // (something leaves the cell)
                        u[c] = sum * pm;
                        int idx = s - nbase;
                        idx = idx >= cap ? idx - cap : idx;
                        const float g = ldexpf(arow[idx] * sum, dt) / pman;
                        if (s & 1) {
#pragma unroll
                            for (int l = 1; l < NL; ++l) acc[l] += z == l ? g : 0.0f;
                        } else {
                            acc[0] += g;
                        }
                        const int e = finite_exp(u[c]);
                        emax = max(emax, e != kNoExp ? e + ex[c] : kNoExp);
                    }
                }
            }
            emax = wave_imax(emax);
            if ((tid & 63) == 0) lds.misc[tid >> 6] = emax;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                if (l < N) {  // (block-uniform)
                    const float v = wave_fsum(acc[l]);
                    if ((tid & 63) == 0) red[(tid >> 6) * NL + l] = v;
                }
            }
            __syncthreads();  // every read of `above` is done, the waves' maxima and sums are in place
            for (int w = 0; w < nw; ++w) emax = max(emax, lds.misc[w]);
            const int sh = emax == kNoExp ? 0 : kTargetBack - emax;
            eb -= sh;
            // ---- the row's N occupancies, the same in every work-item ----
            float mass = 0.0f, cell = 0.0f;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                if (l < N) {
                    float v = red[l];
                    for (int w = 1; w < nw; ++w) v += red[w * NL + l];
                    mass = l == 0 ? v : mass + v;
                    cell = tid == l ? v : cell;
                }
            }
            if (!(fabsf(mass - 1.0f) <= lost)) {  // (block-uniform) the rows cannot hold this lattice
                // (work-item c wrote column c of the rows above: its own NaN follows its own stores)
                for (int tt = 0; tt < rw.Tr; ++tt)
                    if (tid < N) out[(int64_t)tt * q.occ_stride_t + tid] = NAN;
                if (tid == 0) p.logp[blockIdx.x] = (double)NAN;
                return;
            }
            if (tid < N) {
                float *o = out + (int64_t)t * q.occ_stride_t + tid;
                if (!q.occ_accumulate) *o = cell == 0.0f ? 0.0f : q.occ_scale * cell;
                else if (cell != 0.0f) *o = *o + q.occ_scale * cell;  // (a cell of occupancy 0 is not read)
            }
#pragma unroll
            for (int c = 0; c < kWideCells; ++c) {
                const int s = lo + tid + c * bd;
                if (s <= hi) {
                    int idx = s - nbase;
                    idx = idx >= cap ? idx - cap : idx;
                    mine[idx] = ldexpf(u[c], min(max(ex[c] + sh, -512), 512));
                }
            }
            base = nbase;
            lo_n = lo;
            hi_n = hi;
            which ^= 1;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(1024) void score_lds_kernel(LdsWalkParams q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (q.walk == kLdsOcc) return lds_occ_walk(q, smem);
    if (q.walk == kLdsStore) return lds_forward<true>(q, smem);
    if (q.walk == kLdsDetect) return lds_forward<false, true>(q, smem);
    lds_forward<false>(q, smem);
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

// fcd_ctc_detect_*'s LDS walk holds kWideCells cells per work-item
bool ctc_detect_supported(int64_t T, int64_t stride) {
    const int64_t states = ctc_score_window_states(T, stride, 0);
    return states + 2 <= 512 || states <= 1024 * kWideCells;
}

namespace {
// a launch of score_lds_kernel; lds: the dynamic LDS the walk needs.  Work-items: ctc_score's choice for its own walk; the
// occupancy pair steps from 512 to 1024 at 512 * kWideCells states
hipError_t launch_lds_walk(const LdsWalkParams &q, int64_t rows, size_t lds, hipStream_t stream) {
    const int64_t states = q.s.cap;
    const int64_t two = q.walk == kLdsScore ? 6144 : 512 * kWideCells;
    const int threads = states <= 2048 ? 256 : (states <= two ? 512 : 1024);
#ifndef FCD_HIPEMU
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(score_lds_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
#endif
    hipLaunchKernelGGL(score_lds_kernel, dim3((unsigned)rows), dim3(threads), lds, stream, q);
    return hipGetLastError();
}

// the LDS of the two occupancy walks: ctc_score's, and kLdsOcc's reduction words behind the alpha buffers
size_t wide_lds_bytes(int64_t lab_cap, int64_t cap) { return lds_bytes((int)lab_cap, (int)cap) + (size_t)kRedWords * 4; }

bool wide_delegates(int64_t T, int64_t stride, int64_t band) {  // the window fits the registers: fcd_ctc_occupancy_*'s walk
    return ctc_score_window_states(T, stride, band) + 2 <= 512;
}
}  // namespace

// 0 = the kernels hold the call; 2 = more than 8 labels; 3 = (register-resident windows) the labelling's LDS copy and the
// tile exceed 64 KiB; 4 = the window exceeds 1024 * kWideCells states; 5 = the labelling's copy, the tile, the two alpha
// buffers and the reduction words exceed 160 KiB
int ctc_occupancy_wide_unsupported(int64_t T, int64_t stride, int64_t band, int64_t N) {
    if (wide_delegates(T, stride, band)) return ctc_posterior_unsupported(T, stride, band, N);
    if (N - 1 > 8) return 2;
    const int64_t cap = ctc_score_window_states(T, stride, band);
    if (cap > 1024 * kWideCells) return 4;
    const int64_t lab_cap = std::max<int64_t>(std::min<int64_t>(std::min(T, stride), 1 << 20), 1);
    return wide_lds_bytes(lab_cap, cap) > 160 * 1024 ? 5 : 0;
}

// stored forward rows of one labelling: T * cap cells by slot, then T exponent words (a register-resident window:
// ctc_posterior_row_bytes)
size_t ctc_occupancy_wide_row_bytes(int64_t T, int64_t stride, int64_t band) {
    if (wide_delegates(T, stride, band)) return ctc_posterior_row_bytes(T, stride, band);
    const size_t cap = (size_t)ctc_score_window_states(T, stride, band);
    return ((size_t)(T > 1 ? T : 1) * (cap + 1) * 4 + 255) & ~(size_t)255;
}

hipError_t launch_ctc_occupancy_wide(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, const OccupancyDesc &out,
                                     double *logp, unsigned char *alpha, hipStream_t stream) {
    if (wide_delegates(in.T, y.stride, band)) return launch_ctc_occupancy(in, y, collapse, band, out, logp, alpha, stream);
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    LdsWalkParams q;
    q.s.in = in;
    q.s.y = y;
    q.s.collapse = collapse;
    q.s.band = (int)band;
    q.s.logp = logp;
    q.s.lab_cap = (int)std::max<int64_t>(std::min(in.T, y.stride), 1);
    q.s.cap = (int)ctc_score_window_states(in.T, y.stride, band);
    q.alpha = reinterpret_cast<float *>(alpha);
    q.alpha_words = (int64_t)(ctc_occupancy_wide_row_bytes(in.T, y.stride, band) / 4);
    q.occ = out.occ;
    q.occ_stride_row = out.stride_row;
    q.occ_stride_t = out.stride_t;
    q.occ_scale = out.scale;
    q.occ_accumulate = out.accumulate;
    q.detect = nullptr;
    const size_t lds = wide_lds_bytes(q.s.lab_cap, q.s.cap);
    q.walk = kLdsStore;
    hipError_t e = launch_lds_walk(q, rows, lds, stream);
    if (e != hipSuccess) return e;
    q.walk = kLdsOcc;
    return launch_lds_walk(q, rows, lds, stream);
}

// The packed detecting walk (pack_walk above): y describes y.n_hyp motifs shared by all reads; *detect (device memory) holds
// them again with pack_reads = ctc_detect_packed_reads(): one wavefront per pack_reads reads, or per read and 64 motifs.
int ctc_detect_packed_labels() { return kPackLabels; }

int ctc_detect_packed_reads(int64_t n_motifs, int64_t N) {
    if (n_motifs > 32) return 1;
    int mp = 1;
    while (mp < n_motifs) mp *= 2;
    int reads = 64 / mp;
    while (reads > 1 && 31 * (64 / reads) / N < 2) reads /= 2;  // (a slot's 31 * 64 / reads words hold two rows at least)
    return reads;
}

hipError_t launch_ctc_detect_packed(const BatchDesc &in, const ScoreDesc &y, int collapse, double *logp, hipStream_t stream,
                                    const DetectOut *detect) {
    const int64_t reads = ctc_detect_packed_reads(y.n_hyp, in.N);
    const int64_t blocks = (in.n_reads + reads - 1) / reads * ((y.n_hyp + 63) / 64);
    if (blocks <= 0) return hipSuccess;
    if (y.stride > kPackLabels || in.N > kPackTileWords || blocks >= (1ll << 31)) return hipErrorInvalidValue;
    ScoreParams p;
    p.in = in;
    p.y = y;
    p.collapse = collapse;
    p.band = 0;
    p.logp = logp;
    p.lab_cap = 1;
    p.cap = 0;
    hipLaunchKernelGGL(score_reg_kernel<2>, dim3((unsigned)blocks), dim3(64), lds_bytes(1, 0), stream, p, detect);
    return hipGetLastError();
}

hipError_t launch_ctc_score(const BatchDesc &in, const ScoreDesc &y, int collapse, int64_t band, double *logp,
                            hipStream_t stream, const DetectOut *detect) {
    const int64_t rows = in.n_reads * y.n_hyp;
    if (rows <= 0) return hipSuccess;
    LdsWalkParams q;
    q.walk = detect ? kLdsDetect : kLdsScore;  // (detecting: band is 0, the caller's check)
    q.detect = detect;
    q.alpha = q.occ = nullptr;
    q.alpha_words = q.occ_stride_row = q.occ_stride_t = 0;
    q.occ_scale = 0.0f;
    q.occ_accumulate = 0;
    ScoreParams &p = q.s;
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
        if (states + 2 <= 128) hipLaunchKernelGGL(score_reg_kernel<2>, grid, dim3(64), lds, stream, p, detect);
        else if (states + 2 <= 256) hipLaunchKernelGGL(score_reg_kernel<4>, grid, dim3(64), lds, stream, p, detect);
        else if (states + 2 <= 384) hipLaunchKernelGGL(score_reg_kernel<6>, grid, dim3(64), lds, stream, p, detect);
        else hipLaunchKernelGGL(score_reg_kernel<8>, grid, dim3(64), lds, stream, p, detect);
    } else {
        p.cap = (int)states;
        return launch_lds_walk(q, rows, lds_bytes(p.lab_cap, p.cap), stream);
    }
    return hipGetLastError();
}

}  // namespace fcd
