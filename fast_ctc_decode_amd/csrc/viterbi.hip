// viterbi.hip -- greedy decoders: search::viterbi_search (/root/reference/src/search.rs:303-383)
// and search::crf_greedy_search (:385-423), one read per wavefront.
//
// viterbi: the wave walks the read in tiles of 64 rows, one row per lane.  Per row: first-maximum
// argmax with the reference's strict '>' fold (:303-318); emission test against the previous
// row's label (lane-1 via a wave shuffle, lane 0 from the carry); wave-level stream compaction of
// the emissions with ballot + prefix popcount, so labels / path are written coalesced.  The
// optional quality output reproduces the reference's per-run f32 running sum IN ROW ORDER
// (:348-376) -- a tree reduction would round differently -- by letting every run head absorb one
// following row per iteration.
#include <math.h>

#include <algorithm>

#include "device_utils.h"
#include "fcd_internal.h"

namespace fcd {

namespace {

constexpr int kWavesPerBlock = 4;

// Running state of one read's scan, carried across 64-row sub-tiles.
struct ScanState {
    int n_out = 0;          // emissions so far (wave-uniform)
    int carry_label = -1;   // label of the last row of the previous sub-tile (None)
    float run_total = 0.0f; // open quality run carried across sub-tiles (:337-339)
    int run_count = 0;
};

// One sub-tile: lane holds (label, prob) of row base+lane; emits, compacts, accumulates quality.
__device__ __forceinline__ void scan_subtile(ScanState &st, int label, float prob, bool act,
                                             int64_t base, int64_t T, int collapse, uint8_t *lab,
                                             uint32_t *pth, float *qual) {
    const int lane = threadIdx.x & 63;
    const int64_t row = base + lane;
    int prev = __shfl_up(label, 1);
    if (lane == 0) prev = st.carry_label;
    const bool emit = act && label != 0 && (!collapse || prev != label);  // :347
    const uint64_t m_emit = ballot(emit);
    const int my_out = st.n_out + popc64(m_emit & lanemask_lt());
    if (emit) {
        lab[my_out] = (uint8_t)label;
        if (pth) pth[my_out] = (uint32_t)row;
    }
    if (qual) {
        // Each emission opens a run that owns every following non-blank row up to the next
        // emission; its mean probability is what the reference feeds to phred().
        const bool nonblank = act && label != 0;
        const float contrib = nonblank ? prob : 0.0f;  // adding +0.0 is exact
        const int cnt1 = nonblank ? 1 : 0;
        // (a) the run carried in from the previous sub-tile absorbs rows [0, first emission)
        const int first_emit = m_emit ? __builtin_ctzll(m_emit) : kWave;
        const int tile_rows = (int)((T - base) < kWave ? (T - base) : kWave);
        const int lim = first_emit < tile_rows ? first_emit : tile_rows;
        for (int j = 0; j < lim; ++j) {
            st.run_total += __shfl(contrib, j);
            st.run_count += __shfl(cnt1, j);
        }
        if (m_emit && st.run_count > 0) {
            if (lane == 0) qual[st.n_out - 1] = st.run_total / (float)st.run_count;
            st.run_total = 0.0f;
            st.run_count = 0;
        }
        // (b) runs that start in this sub-tile: every head absorbs one more row per iteration
        float acc = contrib;  // the emission row itself (:362-365)
        int cnt = cnt1;
        bool alive = emit;
        float sh_c = contrib;
        int sh_n = cnt1;
        bool sh_e = emit;
        bool sh_a = act;
        for (int d = 1; d < kWave; ++d) {
            sh_c = __shfl_down(sh_c, 1);
            sh_n = __shfl_down(sh_n, 1);
            sh_e = __shfl_down((int)sh_e, 1) != 0;
            sh_a = __shfl_down((int)sh_a, 1) != 0;
            const bool in_tile = lane + d < kWave && sh_a;
            if (alive && (!in_tile || sh_e)) alive = false;
            if (alive) {
                acc += sh_c;
                cnt += sh_n;
            }
            if (ballot(alive) == 0ull) break;
        }
        // a head whose run is closed by a later emission in this sub-tile writes its mean now;
        // the last head's run stays open and becomes the carry
        const uint64_t later = m_emit & ~(lanemask_lt() | (1ull << lane));
        if (emit && later) qual[my_out] = acc / (float)cnt;
        if (m_emit) {
            const int last = 63 - __builtin_clzll(m_emit);
            st.run_total = __shfl(acc, last);
            st.run_count = __shfl(cnt, last);
        }
    }
    st.n_out += popc64(m_emit);
    const int last_lane = (int)((T - base) < kWave ? (T - base - 1) : (kWave - 1));
    st.carry_label = __shfl(label, last_lane);
}

// The same for a sub-tile whose 64 rows all exist, without quality values: the neighbour's label through a DPP
// wave shift (no LDS round trip), 32-bit output offsets against wave-uniform bases -- a third of the instructions.
__device__ __forceinline__ void scan_subtile_full(ScanState &st, int label, uint32_t row, int collapse, uint8_t *lab,
                                                  uint32_t *pth) {
    // wave_shr:1 -- lane 0 has no source lane and keeps `old`, the label carried over from the previous sub-tile
    const int prev = __builtin_amdgcn_update_dpp(st.carry_label, label, 0x138, 0xf, 0xf, false);
    const bool emit = label != 0 && (!collapse || prev != label);  // :347
    const uint64_t m_emit = ballot(emit);
    const uint32_t my_out = (uint32_t)st.n_out + (uint32_t)popc64(m_emit & lanemask_lt());
    if (emit) {
        lab[my_out] = (uint8_t)label;
        if (pth) pth[my_out] = row;
    }
    st.n_out += popc64(m_emit);
    st.carry_label = __builtin_amdgcn_readlane(label, 63);
}

__device__ __forceinline__ void scan_finish(ScanState &st, int64_t r, float *qual,
                                            const ResultDesc &out) {
    const int lane = threadIdx.x & 63;
    if (qual && st.run_count > 0 && lane == 0)
        qual[st.n_out - 1] = st.run_total / (float)st.run_count;  // :370-376
    if (lane == 0) {
        out.out_len[r] = (uint32_t)st.n_out;
        if (out.status) out.status[r] = FCD_ST_OK;
    }
}

// Generic path: any N, any strides; one row per lane, strided 4-byte loads.
__global__ __launch_bounds__(64 * kWavesPerBlock) void viterbi_kernel(BatchDesc in, int collapse,
                                                                    ResultDesc out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (r >= in.n_reads) return;
    int64_t T = in.T;
    if (in.lengths) {
        int64_t t = in.lengths[r];
        T = t < 0 ? 0 : (t < T ? t : T);
    }
    const int N = in.N;
    const int dt = in.dtype;
    const float *post = post_at(in.post, r * in.stride_read, dt);
    uint8_t *lab = out.labels + r * out.out_stride;
    uint32_t *pth = out.path ? out.path + r * out.out_stride : nullptr;
    float *qual = out.qual ? out.qual + r * out.out_stride : nullptr;
    ScanState st;
    for (int64_t base = 0; base < T; base += kWave) {
        const int64_t row = base + lane;
        const bool act = row < T;
        int label = 0;
        float prob = 0.0f;
        if (act) {
            const float *pr = post_at(post, row * in.stride_t, dt);
            prob = load_post(pr, 0, dt);
            for (int j = 1; j < N; ++j) {  // find_max: strict '>' keeps the first maximum
                const float v = load_post(pr, j * in.stride_n, dt);
                if (v > prob) {
                    prob = v;
                    label = j;
                }
            }
        }
        scan_subtile(st, label, prob, act, base, T, collapse, lab, pth, qual);
    }
    scan_finish(st, r, qual, out);
}

// Streaming path for C-contiguous reads (stride_n == 1, stride_t == N, 16-byte aligned reads):
// the wave pulls a 256-row tile with N fully coalesced 16-byte loads per lane (1 KiB per wave
// instruction), parks it in LDS and reads it back one row per lane (row stride N dwords: conflict
// free for odd N), so HBM sees only wide contiguous requests.  The next tile's loads are issued
// before the current tile is scanned.
constexpr int kTileRows = 256;

// DT: the posteriors' element type.  Half-precision reads (what basecaller networks emit; the reference forces a
// host float32 copy, src/lib.rs:182) stream at HALF the bytes: a 16-byte load brings eight elements, which are
// converted in registers -- exactly -- and parked in the same f32 tile, so everything after the tile is shared.
template <int N, int DT>
__global__ __launch_bounds__(64 * kWavesPerBlock) void viterbi_stream_kernel(BatchDesc in,
                                                                           int collapse,
                                                                           ResultDesc out) {
    constexpr int EPL = DT == kF32 ? 4 : 8;                             // elements per 16-byte load
    constexpr int NLOAD = (kTileRows * N + 64 * EPL - 1) / (64 * EPL);  // 16-byte loads per lane and tile
    // (f32: NLOAD = N and the tile is covered exactly; 16-bit, odd N: the last load is half used)
    __shared__ __attribute__((aligned(16))) float s_tile[kWavesPerBlock][NLOAD * 64 * EPL];
    const int lane = threadIdx.x & 63;
    // (wave-uniform, and said so: the read's index, its length and every pointer derived from them live in scalar registers)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (r >= in.n_reads) return;
    int64_t T = in.T;
    if (in.lengths) {
        int64_t t = in.lengths[r];
        T = t < 0 ? 0 : (t < T ? t : T);
    }
    const float *post = post_at(in.post, r * in.stride_read, DT);
    uint8_t *lab = out.labels + r * out.out_stride;
    uint32_t *pth = out.path ? out.path + r * out.out_stride : nullptr;
    float *qual = out.qual ? out.qual + r * out.out_stride : nullptr;
    float *tile = s_tile[wave];
    const int64_t total = T * N;  // elements in this read

    auto fetch = [&](int64_t tile_row0, uint4 (&v)[NLOAD]) {
        const int64_t f0 = tile_row0 * N;
#pragma unroll
        for (int m = 0; m < NLOAD; ++m) {
            const int64_t f = f0 + (int64_t)(lane + 64 * m) * EPL;
            const bool in_tile = (lane + 64 * m) * EPL < kTileRows * N;
            if (in_tile && f + EPL - 1 < total) {
                v[m] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(post) + f * (DT == kF32 ? 4 : 2));
            } else {  // the ragged end of the read: element by element, zeros beyond it
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                if (in_tile) {
                    if (DT == kF32) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (f + e < total) w[e] = __float_as_uint(post[f + e]);
                    } else {
                        const uint16_t *ph = reinterpret_cast<const uint16_t *>(post);
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (f + e < total) w[e >> 1] |= (uint32_t)ph[f + e] << (16 * (e & 1));
                    }
                }
                v[m] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    };
    auto park = [&](const uint4 (&v)[NLOAD]) {
#pragma unroll
        for (int m = 0; m < NLOAD; ++m) {
            float *dst = tile + (lane + 64 * m) * EPL;
            if (DT == kF32) {
                *reinterpret_cast<uint4 *>(dst) = v[m];
            } else {
                const uint32_t w[4] = {v[m].x, v[m].y, v[m].z, v[m].w};
                float4 lo4, hi4;
                if (DT == kF16) {
                    lo4 = make_float4(f16_bits_to_f32((uint16_t)w[0]), f16_bits_to_f32((uint16_t)(w[0] >> 16)),
                                      f16_bits_to_f32((uint16_t)w[1]), f16_bits_to_f32((uint16_t)(w[1] >> 16)));
                    hi4 = make_float4(f16_bits_to_f32((uint16_t)w[2]), f16_bits_to_f32((uint16_t)(w[2] >> 16)),
                                      f16_bits_to_f32((uint16_t)w[3]), f16_bits_to_f32((uint16_t)(w[3] >> 16)));
                } else {
                    lo4 = make_float4(__uint_as_float(w[0] << 16), __uint_as_float(w[0] & 0xFFFF0000u),
                                      __uint_as_float(w[1] << 16), __uint_as_float(w[1] & 0xFFFF0000u));
                    hi4 = make_float4(__uint_as_float(w[2] << 16), __uint_as_float(w[2] & 0xFFFF0000u),
                                      __uint_as_float(w[3] << 16), __uint_as_float(w[3] & 0xFFFF0000u));
                }
                *reinterpret_cast<float4 *>(dst) = lo4;
                *reinterpret_cast<float4 *>(dst + 4) = hi4;
            }
        }
    };

    // a tile that lies inside the read entirely: no bounds to check (256 * N elements are a whole number of loads'
    // in-tile lanes for every element type)
    auto fetch_full = [&](int64_t tile_row0, uint4 (&v)[NLOAD]) {
        const char *src = reinterpret_cast<const char *>(post) + tile_row0 * N * (DT == kF32 ? 4 : 2) + lane * 16;
#pragma unroll
        for (int m = 0; m < NLOAD; ++m) {
            if ((lane + 64 * m) * EPL < kTileRows * N) v[m] = *reinterpret_cast<const uint4 *>(src + m * 1024);
            else v[m] = make_uint4(0u, 0u, 0u, 0u);
        }
    };

    ScanState st;
    uint4 cur[NLOAD], nxt[NLOAD];
    if (T >= kTileRows) fetch_full(0, cur);
    else if (T > 0) fetch(0, cur);
    int64_t base = 0;
    // ---- whole tiles: nothing to test per row ----
    for (; base + kTileRows <= T; base += kTileRows) {
        const int64_t nb = base + kTileRows;
        if (nb + kTileRows <= T) fetch_full(nb, nxt);
        else if (nb < T) fetch(nb, nxt);
        park(cur);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < kTileRows / 64; ++u) {
            const float *pr = tile + (64 * u + lane) * N;
            float prob = pr[0];
            int label = 0;
#pragma unroll
            for (int j = 1; j < N; ++j) {  // find_max: strict '>' keeps the first maximum
                const float v = pr[j];
                if (v > prob) {
                    prob = v;
                    label = j;
                }
            }
            if (qual) scan_subtile(st, label, prob, true, base + 64 * u, T, collapse, lab, pth, qual);
            else scan_subtile_full(st, label, (uint32_t)(base + 64 * u) + (uint32_t)lane, collapse, lab, pth);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int m = 0; m < NLOAD; ++m) cur[m] = nxt[m];
    }
    // ---- the ragged last tile ----
    for (; base < T; base += kTileRows) {
        if (base + kTileRows < T) fetch(base + kTileRows, nxt);
        park(cur);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < kTileRows / 64; ++u) {
            const int64_t sub = base + 64 * u;
            if (sub >= T) break;
            const bool act = sub + lane < T;
            const float *pr = tile + (64 * u + lane) * N;
            float prob = pr[0];
            int label = 0;
#pragma unroll
            for (int j = 1; j < N; ++j) {  // find_max: strict '>' keeps the first maximum
                const float v = pr[j];
                if (v > prob) {
                    prob = v;
                    label = j;
                }
            }
            if (!act) {
                label = 0;
                prob = 0.0f;
            }
            scan_subtile(st, label, prob, act, sub, T, collapse, lab, pth, qual);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int m = 0; m < NLOAD; ++m) cur[m] = nxt[m];
    }
    scan_finish(st, r, qual, out);
}

// Time-major storage: element (read r, row t, column c) at post[t * stride_t + r * N + c] -- the (T, B, N) tensor a
// basecaller network emits, handed over as a (B, T, N) batch by its strides, no transposition.  A row of one read is
// N elements, but a row of EIGHT neighbouring reads is 8 * N contiguous elements: a workgroup of four wavefronts takes
// 8 reads, pulls 64-row tiles of them with 16-byte loads (each time step of the group is one contiguous run), parks the
// tile in LDS as [step][read][column] with a pitch of 8 * N + 1 words -- so that the row-per-lane read back, lanes one
// time step apart, hits all banks -- and every wavefront scans two of the reads exactly as the read-major kernel does.
constexpr int kTmReads = 8;
constexpr int kTmSteps = 64;

template <int N, int DT>
__global__ __launch_bounds__(256) void viterbi_tm_kernel(BatchDesc in, int collapse, ResultDesc out) {
    constexpr int EPL = DT == kF32 ? 4 : 8;      // elements per 16-byte load
    constexpr int ESZ = DT == kF32 ? 4 : 2;
    constexpr int G = kTmReads * N;               // elements of one time step of the group (a whole number of 16-byte units)
    constexpr int U = G / EPL;                    // 16-byte units per time step
    constexpr int UNITS = kTmSteps * U;           // per tile
    constexpr int NLD = (UNITS + 255) / 256;      // loads per thread and tile
    constexpr int PITCH = G + 1;
    __shared__ float s_tile[kTmSteps * PITCH];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // Neighbouring groups share cache lines (a group's run of 8 * N elements is not a whole number of 128-byte lines),
    // and consecutive workgroup ids go round the eight XCDs, each with its own L2: hand every XCD a CONTIGUOUS range of
    // groups, so that a shared line is fetched into one L2, not two.
    const unsigned n_groups = gridDim.x, per_xcd = (n_groups + 7) / 8;
    unsigned gidx = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (n_groups < 64 || gidx >= n_groups || (n_groups & 7)) gidx = blockIdx.x;  // (small or ragged launches: as they come)
    const int64_t r0 = (int64_t)gidx * kTmReads;  // (the launch covers whole groups only)
    const int64_t T = in.T;
    const char *base = reinterpret_cast<const char *>(in.post) + r0 * in.stride_read * ESZ;
    const int64_t pitch_b = in.stride_t * ESZ;

    auto fetch = [&](int64_t t0, uint4 (&v)[NLD]) {
#pragma unroll
        for (int m = 0; m < NLD; ++m) {
            const int u = tid + 256 * m;
            const int sidx = u / U, o = u - sidx * U;
            v[m] = make_uint4(0u, 0u, 0u, 0u);
            if (u < UNITS && t0 + sidx < T)
                v[m] = *reinterpret_cast<const uint4 *>(base + (t0 + sidx) * pitch_b + o * 16);
        }
    };
    auto park = [&](const uint4 (&v)[NLD]) {
#pragma unroll
        for (int m = 0; m < NLD; ++m) {
            const int u = tid + 256 * m;
            if (u >= UNITS) continue;
            const int sidx = u / U, o = u - sidx * U;
            float *dst = s_tile + sidx * PITCH + o * EPL;  // (the odd pitch leaves only 4-byte alignment)
            const uint32_t w[4] = {v[m].x, v[m].y, v[m].z, v[m].w};
            if (DT == kF32) {
#pragma unroll
                for (int e = 0; e < 4; ++e) dst[e] = __uint_as_float(w[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint16_t h = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
                    dst[e] = DT == kF16 ? f16_bits_to_f32(h) : bf16_bits_to_f32(h);
                }
            }
        }
    };

    constexpr int RPW = kTmReads / 4;  // reads per wavefront
    ScanState st[RPW];
    int64_t Tr[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int64_t r = r0 + wave * RPW + i;
        int64_t t = T;
        if (in.lengths) {
            const int64_t tl = in.lengths[r];
            t = tl < 0 ? 0 : (tl < T ? tl : T);
        }
        Tr[i] = t;
    }
    uint4 cur[NLD], nxt[NLD];
    if (T > 0) fetch(0, cur);
    for (int64_t t0 = 0; t0 < T; t0 += kTmSteps) {
        if (t0 + kTmSteps < T) fetch(t0 + kTmSteps, nxt);
        park(cur);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            if (t0 >= Tr[i]) continue;  // (wave-uniform)
            const int rr = wave * RPW + i;
            const int64_t r = r0 + rr;
            const float *pr = s_tile + lane * PITCH + rr * N;
            float prob = pr[0];
            int label = 0;
#pragma unroll
            for (int j = 1; j < N; ++j) {  // find_max: strict '>' keeps the first maximum
                const float v = pr[j];
                if (v > prob) {
                    prob = v;
                    label = j;
                }
            }
            uint8_t *lab = out.labels + r * out.out_stride;
            uint32_t *pth = out.path ? out.path + r * out.out_stride : nullptr;
            float *qual = out.qual ? out.qual + r * out.out_stride : nullptr;
            if (!qual && t0 + kTmSteps <= Tr[i]) {
                scan_subtile_full(st[i], label, (uint32_t)t0 + (uint32_t)lane, collapse, lab, pth);
            } else {
                const bool act = t0 + lane < Tr[i];
                if (!act) {
                    label = 0;
                    prob = 0.0f;
                }
                scan_subtile(st[i], label, prob, act, t0, Tr[i], collapse, lab, pth, qual);
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < NLD; ++m) cur[m] = nxt[m];
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int64_t r = r0 + wave * RPW + i;
        scan_finish(st[i], r, out.qual ? out.qual + r * out.out_stride : nullptr, out);
    }
}

// ---- the Viterbi search under a CRF model (fcd_crf_viterbi_search_*; include/fcd.h has the definition) ----
// NOT a reference function: the exact, unpruned decode over all labellings -- the single most probable path through the
// model's states, of which crf_greedy_search (:385-423) follows the locally best one.
//
// One wavefront per read, all S states live: v[s] is the best probability of any path that leaves state s behind after
// the row, in LDS.  Per row the wavefront reads the S * N posteriors (S * N <= 64: a lane per element; beyond: lane l the
// N posteriors of states l, l + 64, ..., consecutive lanes consecutive states), forms each product with its state's v, and
// leaves the stay products in v[s] and writes the nb = N - 1 advance products to c[s * nb + j]; then lane l settles states
// l, l + 64, ...  (v[s] is overwritten only once its readers are done: with a lane per element every lane reads v[s] before
// the wave maximum and stores after it; with a lane per state a state's v[s] is read and written by its own lane only.)  The state s' that source s reaches with label j + 1 is (s nb) mod S + j
// (:97,414), so c[s nb + j] = c[s' + i S] with i = (s nb) div S: destination s' reads c[s' + i S], i = 0 .. nb-1 -- both
// sides contiguous across lanes, no cross-lane shuffle.  The LDS is the wavefront's own: a wait on its counter orders it.
// Arithmetic: crf_lattice.hip's -- posteriors split into mantissa and exponent, ONE f32 product per candidate, every
// cell rescaled by an exact power of two per row (the row's largest exponent is known to within one from the operands'
// exponents, before any product is formed), ln(m) + E ln 2 in float64.
// Back-pointers: one byte per state and row in the caller's workspace (0 stay, i + 1 advance i); the wavefront walks them
// back after the last row, 64 emissions at a time in registers, written to the END of the read's output rows and moved
// to the front once their number is known -- no second pass over the posteriors.
struct VitArgs {
    int mode;               // 0: crf_greedy_search's walk (every launch of launch_crf_greedy); 1: the Viterbi walk;
                            // 2: the transition-probability walk (crf_transitions_walk); 3: that walk, then the forward
                            // pass over what it stored (crf_marginals_forward)
    int lds_bytes;          // dynamic LDS of the launch (modes 1, 2 and 3)
    double *logp;           // [n_reads], nullable
    unsigned char *bp;      // back-pointers: bp_read_bytes per read, row t and state s at [t * S + s]
    int64_t bp_read_bytes;
    TransitionsDesc tr;     // modes 2 and 3: the outputs and the input's layout (mode 3: probs is the marginals' buffer,
                            // f32, and init is null -- the init row stays in LDS)
    float *emit;            // mode 3: [n_reads * emit_stride], (T, N) dense per read, nullable
    int64_t emit_stride;
};

constexpr int kVitMaxN = 9;
constexpr int kVitMinLds = 4096;  // the traceback's chunk of back-pointers reuses the LDS: at least this much of it
constexpr int kVitAhead = 4;      // S * N <= 64: rows whose loads are in flight

__device__ __forceinline__ void vit_lds_sync() {  // LDS written by one lane, read by another, same wavefront
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void vit_global_sync() {  // global memory written by one lane, read by another
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

__device__ __forceinline__ void crf_viterbi_walk(const BatchDesc &in, const float *init_all, int64_t n_init,
                                                 int64_t init_stride, const ResultDesc &out, const VitArgs &va,
                                                 float *lds) {
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    int64_t T = in.T;
    if (in.lengths) {
        int64_t t = in.lengths[r];
        T = t < 0 ? 0 : (t < T ? t : T);
    }
    const int Tr = (int)T;
    const int N = in.N, S = in.S, nb = N - 1;
    const int dt = in.dtype;
    const float *post = post_at(in.post, r * in.stride_read, dt);
    uint8_t *lab = out.labels + r * out.out_stride;
    uint32_t *pth = out.path ? out.path + r * out.out_stride : nullptr;
    float *qual = out.qual ? out.qual + r * out.out_stride : nullptr;

    // sigma_0: the first maximum of the init row, as crf_greedy_search takes it (:399)
    const float *init = init_all + r * init_stride;
    int state = 0;
    bool bad = n_init <= 0;
    if (!bad) {
        float m = init[0];
        bad = m != m;
        for (int64_t j = 1; j < n_init && !bad; ++j) {
            const float e = init[j];
            if (e != e) bad = true;
            if (e > m) {
                m = e;
                state = (int)j;
            }
        }
    }
    if (bad || Tr == 0 || state >= S) {  // (an init row no state follows from; no rows: the empty path, probability 1)
        const bool ok = !bad && Tr == 0;
        if (lane == 0) {
            out.out_len[r] = 0u;
            out.status[r] = ok ? FCD_ST_OK : FCD_ST_BAD_STATE;
            if (va.logp) va.logp[r] = ok ? 0.0 : (double)NAN;
        }
        return;
    }

    float *v = lds, *c = lds + S;
    for (int s = lane; s < S; s += kWave) v[s] = s == state ? 1.0f : 0.0f;  // "row -1"
    vit_lds_sync();
    unsigned char *bp = va.bp + r * va.bp_read_bytes;
    int64_t eacc = 0;  // the cells are v * 2^eacc
    bool nan = false;
    // A row of at most 64 elements is walked by ELEMENT: lane e takes element e = s N + j of the S * N row, so a small table
    // still fills its lanes (S = 4, N = 5: 20 lanes with one product each, not 4 lanes with five).
    const int E = S * N;
    const uint32_t recip_n = 0xFFFFFFFFu / (uint32_t)N + 1u;  // e div N = (e * recip_n) >> 32 for e < 2^24
    auto load_elem = [&](int t, int e) {
        const int s = (int)(((uint64_t)(uint32_t)e * recip_n) >> 32), j = e - s * N;
        return load_post(post, (int64_t)t * in.stride_t + (int64_t)s * in.stride_s + (int64_t)j * in.stride_n, dt);
    };
    // the largest exponent the product can have (it has that or one less); a NaN anywhere in the row is remembered
    auto bound_of = [&](float a, float p) {
        nan = nan || (p != p);
        const int ea = finite_exp(a), ep = finite_exp(p);
        return (ea != kNoExp && ep != kNoExp) ? ea + ep : kNoExp;
    };
    // the product, rescaled: the stay candidate of state s, or advance j - 1 at c[s * nb + j - 1]
    auto spread = [&](int e, float a, float p, int sh) {
        const int s = (int)(((uint64_t)(uint32_t)e * recip_n) >> 32), j = e - s * N;
        float m;
        int ex;
        crf_split(p, &m, &ex);
        const float val = ldexpf(a * m, min(max(ex + sh, -512), 512));
        if (j == 0) v[s] = val;  // (the stay candidate takes v[s]'s place: its readers are done, see above)
        else c[s * nb + (j - 1)] = val;
    };
    auto state_of = [&](int e) { return (int)(((uint64_t)(uint32_t)e * recip_n) >> 32); };
    // destination s: the stay candidate is kept unless an advance is strictly greater, the lowest i among equals
    auto settle = [&](int t) {
        for (int s = lane; s < S; s += kWave) {
            float best = v[s];
            int b = 0;
            for (int i = 0; i < nb; ++i) {
                const float cand = c[s + i * S];
                if (cand > best) {
                    best = cand;
                    b = i + 1;
                }
            }
            v[s] = best;
            bp[(int64_t)t * S + s] = (unsigned char)b;
        }
    };
    auto shift_of = [&](int eb) {  // the row's power of two from its largest exponent bound
        const int sh = eb == kNoExp ? 0 : kTarget - eb;
        eacc -= sh;
        return sh;
    };

    if (E <= kWave) {  // one element per lane, its posteriors of the next kVitAhead rows in flight
        const bool act = lane < E;
        const int e = act ? lane : 0, s = state_of(e);
        float ring[kVitAhead];
#pragma unroll
        for (int u = 0; u < kVitAhead; ++u) ring[u] = (act && u < Tr) ? load_elem(u, e) : 0.0f;
        for (int t0 = 0; t0 < Tr; t0 += kVitAhead) {
#pragma unroll
            for (int u = 0; u < kVitAhead; ++u) {
                const int t = t0 + u;
                if (t >= Tr) break;
                const float p = ring[u];
                if (act && t + kVitAhead < Tr) ring[u] = load_elem(t + kVitAhead, e);
                const float a = act ? v[s] : 0.0f;
                const int sh = shift_of(wave_imax(act ? bound_of(a, p) : kNoExp));
                if (act) spread(e, a, p, sh);
                vit_lds_sync();
                settle(t);
                vit_lds_sync();
            }
        }
    } else {
        // Larger rows are walked by STATE: lane l takes states l, l + 64, ... and forms a state's N products from one read
        // of v[s], the label a compile-time index (consecutive lanes still read consecutive states of the row).
        auto load_row = [&](int t, int s, float (&p)[kVitMaxN]) {
            const float *pr = post_at(post, (int64_t)t * in.stride_t + (int64_t)s * in.stride_s, dt);
#pragma unroll
            for (int j = 0; j < kVitMaxN; ++j) p[j] = j < N ? load_post(pr, (int64_t)j * in.stride_n, dt) : 0.0f;
        };
        auto bound_row = [&](float a, const float (&p)[kVitMaxN]) {
            float pm = p[0];
            bool n = p[0] != p[0];
#pragma unroll
            for (int j = 1; j < kVitMaxN; ++j) {
                n = n || (p[j] != p[j]);
                pm = fmaxf(pm, p[j]);  // (the padding is 0.0: it moves no maximum that matters)
            }
            nan = nan || n;
            const int ea = finite_exp(a), ep = finite_exp(pm);
            return (ea != kNoExp && ep != kNoExp) ? ea + ep : kNoExp;
        };
        auto spread_row = [&](int s, float a, const float (&p)[kVitMaxN], int sh) {
#pragma unroll
            for (int j = 0; j < kVitMaxN; ++j) {
                if (j >= N) break;
                float m;
                int ex;
                crf_split(p[j], &m, &ex);
                const float val = ldexpf(a * m, min(max(ex + sh, -512), 512));
                if (j == 0) v[s] = val;  // (the stay candidate takes v[s]'s place: its readers are done, see above)
                else c[s * nb + (j - 1)] = val;
            }
        };
        if (S <= kWave) {  // one state per lane: its row in registers, the next row's loads in flight
            const bool act = lane < S;
            const int s = act ? lane : 0;
            float cur[kVitMaxN], nxt[kVitMaxN];
#pragma unroll
            for (int j = 0; j < kVitMaxN; ++j) cur[j] = nxt[j] = 0.0f;
            if (act) load_row(0, s, cur);
            for (int t = 0; t < Tr; ++t) {
                if (act && t + 1 < Tr) load_row(t + 1, s, nxt);
                const float a = act ? v[s] : 0.0f;
                const int sh = shift_of(wave_imax(act ? bound_row(a, cur) : kNoExp));
                if (act) spread_row(s, a, cur, sh);
                vit_lds_sync();
                settle(t);
                vit_lds_sync();
#pragma unroll
                for (int j = 0; j < kVitMaxN; ++j) cur[j] = nxt[j];
            }
        } else {  // S / 64 states per lane: the row is read twice (the second time from the cache), once per pass
            for (int t = 0; t < Tr; ++t) {
                int eb = kNoExp;
                for (int s = lane; s < S; s += kWave) {
                    float p[kVitMaxN];
                    load_row(t, s, p);
                    eb = max(eb, bound_row(v[s], p));
                }
                const int sh = shift_of(wave_imax(eb));
                for (int s = lane; s < S; s += kWave) {
                    float p[kVitMaxN];
                    load_row(t, s, p);
                    spread_row(s, v[s], p, sh);
                }
                vit_lds_sync();
                settle(t);
                vit_lds_sync();
            }
        }
    }

    // the end state: the first maximum of the last row
    float bv = 0.0f;
    int bi = 0x7fffffff;
    for (int s = lane; s < S; s += kWave) {
        const float x = v[s];
        if (bi == 0x7fffffff || x > bv) {
            bv = x;
            bi = s;
        }
    }
    for (int m = 1; m < kWave; m <<= 1) {
        const float ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) {
            bv = ov;
            bi = oi;
        }
    }
    if (ballot(nan) != 0ull) {  // every value of a read enters a live cell: no comparison orders a NaN
        if (lane == 0) {
            out.out_len[r] = 0u;
            out.status[r] = FCD_ST_INCOMPARABLE;
            if (va.logp) va.logp[r] = (double)NAN;
        }
        return;
    }
    int be = 0;
    const double bm = frexp((double)bv, &be);  // ln(m) + E ln 2 with m in [0.5, 1)
    const double logp = log(bm) + (double)(eacc + be) * 0.693147180559945309417232121458;

    // ---- the walk back: chunks of whole rows of back-pointers through the LDS, every lane follows the one path ----
    vit_global_sync();  // the back-pointers other lanes stored
    unsigned char *sb = reinterpret_cast<unsigned char *>(lds);
    uint32_t *sw = reinterpret_cast<uint32_t *>(lds);
    const int rows_per_chunk = max(1, (va.lds_bytes - 8) / S);
    const uint32_t recip = nb > 1 ? 0xFFFFFFFFu / (uint32_t)nb + 1u : 0u;  // s div nb = (s * recip) >> 32 for s < 2^24
    const int q = S / nb;
    int s = bi, k = 0;  // k: emissions found so far, the last one first; lane k mod 64 holds emission k
    uint8_t my_lab = 0;
    uint32_t my_row = 0;
    float my_q = 0.0f;
    auto flush = [&](int k0, int n) {  // emissions k0 .. k0 + n - 1 to the end of the rows: k lands at Tr - 1 - k
        if (lane < n) {
            const int at = Tr - 1 - (k0 + lane);
            lab[at] = my_lab;
            if (pth) pth[at] = my_row;
            if (qual) qual[at] = my_q;
        }
    };
    for (int c0 = (Tr - 1) / rows_per_chunk * rows_per_chunk; c0 >= 0; c0 -= rows_per_chunk) {
        const int n = min(rows_per_chunk, Tr - c0);
        const int64_t b0 = (int64_t)c0 * S, w0 = b0 & ~(int64_t)3;  // (whole words: a read's rows start 256-byte aligned)
        const int n_words = (int)((b0 + (int64_t)n * S - w0 + 3) >> 2);
        vit_lds_sync();  // the LDS's previous readers are done
        for (int e = lane; e < n_words; e += kWave) sw[e] = reinterpret_cast<const uint32_t *>(bp + w0)[e];
        vit_lds_sync();
        const int skew = (int)(b0 - w0);
        for (int i = n - 1; i >= 0; --i) {
            const int b = __builtin_amdgcn_readfirstlane((int)sb[skew + i * S + s]);
            if (b == 0) continue;
            const int sd = nb > 1 ? (int)(((uint64_t)(uint32_t)s * recip) >> 32) : s;
            const int j = s - sd * nb, src = sd + (b - 1) * q;
            if ((k & 63) == lane) {
                my_lab = (uint8_t)(j + 1);
                my_row = (uint32_t)(c0 + i);
                if (qual)
                    my_q = load_post(post, (int64_t)(c0 + i) * in.stride_t + (int64_t)src * in.stride_s + (int64_t)(j + 1) * in.stride_n, dt);
            }
            s = src;
            if ((++k & 63) == 0) flush(k - 64, 64);
        }
    }
    if (k & 63) flush(k & ~63, k & 63);
    // to the front, 64 at a time: every lane's load before any lane's store (the ranges overlap)
    const int shift = Tr - k;
    if (shift > 0 && k > 0) {
        vit_global_sync();
        for (int base = 0; base < k; base += kWave) {
            const int i = base + lane;
            const bool mine = i < k;
            const uint8_t l = mine ? lab[i + shift] : (uint8_t)0;
            const uint32_t p = (mine && pth) ? pth[i + shift] : 0u;
            const float g = (mine && qual) ? qual[i + shift] : 0.0f;
            __builtin_amdgcn_wave_barrier();
            if (mine) {
                lab[i] = l;
                if (pth) pth[i] = p;
                if (qual) qual[i] = g;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    if (lane == 0) {
        out.out_len[r] = (uint32_t)k;
        out.status[r] = FCD_ST_OK;
        if (va.logp) va.logp[r] = logp;
    }
}

// ---- CRF transition probabilities from raw scores (fcd_crf_transition_probs_*; include/fcd.h has the definition) ----
// NOT a reference function: the step in front of every CRF entry point -- a backward pass over all labellings and a local
// softmax, which turns a network's unnormalised log scores x into the (posteriors, init) pair the searches read.
//
// One wavefront per read, back to front.  The backward vector lives in LDS, two rows of S floats (row t is written while
// row t + 1 is read) and is never stored.  A row is kept UNNORMALISED as it is written; its maximum c_t, a wave reduction,
// is subtracted where the next row reads it (beta~[d] = beta[d] - c_t, the same f32 subtraction either way), and summed
// in float64 for logZ.  Per state: y_a = x_a + beta~[d(s, a)], d(s, 0) = s, d(s, j + 1) = (s nb) mod S + j -- the nb advance
// destinations are nb consecutive states --, m = max y, e_a = exp(y_a - m), the sum in the order a = 0 .. N - 1,
// p_a = e_a / sum, beta = m + ln sum; a state whose candidates are all -inf is dead (p = 0, beta = -inf).
// A row of at most 64 elements takes a lane per element (the candidates of a state meet through LDS; the store is one
// contiguous run); larger rows a lane per state, 64 states at a time, whose 64 N probabilities are parked in LDS and
// stored as contiguous runs across lanes.  Loads run ahead of the dependent chain: kTrAhead rows with a lane per element,
// kTrRows chunks of 64 states with a lane per state (a chunk is N registers per lane).
// Scores indexed by the state being ENTERED (FCD_LAYOUT_DEST) are a different offset per element at load time, nothing more.
constexpr int kTrAhead = 4;
constexpr int kTrRows = 2;
constexpr int kTrStage = kWave * kVitMaxN;  // floats of one staging buffer: the probabilities of 64 states

#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: the plain libm forms)
#define FCD_TR_EXP(x) expf(x)
#define FCD_TR_LOG(x) logf(x)
#else
#define FCD_TR_EXP(x) __expf(x)
#define FCD_TR_LOG(x) __logf(x)
#endif

__device__ __forceinline__ float wave_fmax(float x) {  // of values that are not NaN: through the order-preserving integer
    int b = __float_as_int(x);
    b ^= (b >> 31) & 0x7fffffff;
    b = wave_imax(b);
    b ^= (b >> 31) & 0x7fffffff;
    return __int_as_float(b);
}

// -> whether the read failed (wave-uniform).  A null o.init (the marginals, mode 3) leaves the init row in LDS instead, over
// beta~_0 at lds[0 .. S): every lane overwrites only the states it has just read.
__device__ __forceinline__ bool crf_transitions_walk(const BatchDesc &in, const VitArgs &va, float *lds) {
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    int64_t T = in.T;
    if (in.lengths) {
        int64_t t = in.lengths[r];
        T = t < 0 ? 0 : (t < T ? t : T);
    }
    const int Tr = (int)T;
    const int N = in.N, S = in.S, nb = N - 1, q = S / nb;
    const int dt = in.dtype;
    const TransitionsDesc &o = va.tr;
    const bool dest = o.layout != 0, half_out = o.dtype == kF16;
    const float *x = post_at(in.post, r * in.stride_read, dt);
    float *pf = reinterpret_cast<float *>(o.probs) + (half_out ? 0 : r * o.stride_read);
    uint16_t *ph = reinterpret_cast<uint16_t *>(o.probs) + (half_out ? r * o.stride_read : 0);
    auto store_p = [&](int64_t off, float v) {
        if (half_out) ph[off] = f32_to_f16_bits(v);
        else pf[off] = v;
    };
    float *beta = lds, *stage = lds + 2 * (size_t)S;

    for (int s = lane; s < S; s += kWave) beta[(size_t)(Tr & 1) * S + s] = 0.0f;  // beta~_T = 0
    vit_lds_sync();
    float cprev = 0.0f;     // the maximum of the row being read, not yet subtracted from it
    double csum = 0.0;      // of the row maxima
    bool badx = false;      // this lane met a NaN or +inf
    bool no_path = false;   // a row without a live state (wave-uniform)
    const int E = S * N;

    if (E <= kWave) {  // ---- a lane per element e = s N + a ----
        const bool act = lane < E;
        const int e = act ? lane : 0, s = e / N, a = e - s * N;
        const int sq = s / q, d = a == 0 ? s : (s - sq * q) * nb + a - 1;
        const int64_t xoff = a == 0 ? (int64_t)s * in.stride_s
                             : dest ? (int64_t)d * in.stride_s + (int64_t)(1 + sq) * in.stride_n
                                    : (int64_t)s * in.stride_s + (int64_t)a * in.stride_n;
        float ring[kTrAhead];
#pragma unroll
        for (int u = 0; u < kTrAhead; ++u)
            ring[u] = (act && u < Tr) ? load_post(x, (int64_t)(Tr - 1 - u) * in.stride_t + xoff, dt) : 0.0f;
        for (int k0 = 0; k0 < Tr; k0 += kTrAhead) {
#pragma unroll
            for (int u = 0; u < kTrAhead; ++u) {
                const int t = Tr - 1 - (k0 + u);
                if (t < 0) break;
                const float xv = ring[u];
                if (act && t - kTrAhead >= 0) ring[u] = load_post(x, (int64_t)(t - kTrAhead) * in.stride_t + xoff, dt);
                badx = badx || !(xv < INFINITY);
                const float *bn = beta + (size_t)((t + 1) & 1) * S;
                const float y = xv + (bn[d] - cprev);
                if (act) stage[e] = y;
                vit_lds_sync();
                const float *ys = stage + s * N;
                float m = ys[0];
                for (int j = 1; j < N; ++j) m = fmaxf(m, ys[j]);
                const bool live = m > -INFINITY;
                float sum = 0.0f;
                for (int j = 0; j < N; ++j) sum += live ? FCD_TR_EXP(ys[j] - m) : 0.0f;
                const float p = live ? FCD_TR_EXP(y - m) / sum : 0.0f;
                const float b = live ? m + FCD_TR_LOG(sum) : -INFINITY;
                if (act) store_p((int64_t)t * o.stride_t + e, p);
                if (act && a == 0) beta[(size_t)(t & 1) * S + s] = b;
                const float c = wave_fmax(act ? b : -INFINITY);
                no_path = no_path || !(c > -INFINITY);
                csum += (double)c;
                cprev = c;
                vit_lds_sync();
            }
        }
    } else {  // ---- a lane per state, 64 states (a chunk) at a time; the items (row, chunk) in the order they are walked ----
        const int nchunk = (S + kWave - 1) / kWave;
        // state s = sq q + rq: its advances enter rq nb .. rq nb + nb - 1, and a `dest` input holds them in column 1 + sq
        const int sq0 = lane / q, rq0 = lane - sq0 * q, stepq = kWave / q, stepr = kWave - stepq * q;
        struct Cur {
            int t, c, s, rq, sq;
        };
        auto cur_next = [&](Cur &k) {
            if (++k.c == nchunk) {
                k.c = 0;
                --k.t;
                k.s = lane;
                k.rq = rq0;
                k.sq = sq0;
            } else {
                k.s += kWave;
                k.rq += stepr;
                k.sq += stepq;
                if (k.rq >= q) {
                    k.rq -= q;
                    ++k.sq;
                }
            }
        };
        auto load_row = [&](const Cur &k, float (&p)[kVitMaxN]) {
#pragma unroll
            for (int j = 0; j < kVitMaxN; ++j) p[j] = 0.0f;
            if (k.t < 0 || k.s >= S) return;
            const int64_t row = (int64_t)k.t * in.stride_t, o0 = row + (int64_t)k.s * in.stride_s;
            const int64_t o1 = dest ? row + (int64_t)(k.rq * nb) * in.stride_s + (int64_t)(1 + k.sq) * in.stride_n : o0 + in.stride_n;
            const int64_t da = dest ? in.stride_s : in.stride_n;
            p[0] = load_post(x, o0, dt);
#pragma unroll
            for (int j = 1; j < kVitMaxN; ++j)
                if (j < N) p[j] = load_post(x, o1 + (int64_t)(j - 1) * da, dt);
        };
        Cur lc{Tr - 1, 0, lane, rq0, sq0}, cc = lc;
        float ring[kTrRows][kVitMaxN];
#pragma unroll
        for (int u = 0; u < kTrRows; ++u) {
            load_row(lc, ring[u]);
            cur_next(lc);
        }
        const int64_t items = (int64_t)Tr * nchunk;
        float lmax = -INFINITY;  // this lane's largest beta of the row so far
        int par = 0;             // staging buffer of the item
        for (int64_t k0 = 0; k0 < items; k0 += kTrRows) {
#pragma unroll
            for (int u = 0; u < kTrRows; ++u) {
                if (k0 + u >= items) break;
                float y[kVitMaxN];
#pragma unroll
                for (int j = 0; j < kVitMaxN; ++j) y[j] = ring[u][j];
                load_row(lc, ring[u]);
                cur_next(lc);
                const bool act = cc.s < S;
                const int s = act ? cc.s : 0, base = act ? cc.rq * nb : 0;
                const float *bn = beta + (size_t)((cc.t + 1) & 1) * S;
                float *st = stage + par * kTrStage + lane * N;
#pragma unroll
                for (int j = 0; j < kVitMaxN; ++j) {
                    if (j >= N) break;
                    badx = badx || !(y[j] < INFINITY);
                    y[j] += bn[j == 0 ? s : base + j - 1] - cprev;
                }
                float m = y[0];
#pragma unroll
                for (int j = 1; j < kVitMaxN; ++j) {
                    if (j >= N) break;
                    m = fmaxf(m, y[j]);
                }
                const bool live = m > -INFINITY;
                float sum = 0.0f;
#pragma unroll
                for (int j = 0; j < kVitMaxN; ++j) {
                    if (j >= N) break;
                    y[j] = live ? FCD_TR_EXP(y[j] - m) : 0.0f;
                    sum += y[j];
                }
                const float b = live ? m + FCD_TR_LOG(sum) : -INFINITY;
                if (act) {
                    beta[(size_t)(cc.t & 1) * S + s] = b;
                    lmax = fmaxf(lmax, b);
#pragma unroll
                    for (int j = 0; j < kVitMaxN; ++j) {
                        if (j >= N) break;
                        st[j] = live ? y[j] / sum : 0.0f;
                    }
                }
                if (cc.c == nchunk - 1) {  // the row is complete: its maximum
                    const float c = wave_fmax(lmax);
                    no_path = no_path || !(c > -INFINITY);
                    csum += (double)c;
                    cprev = c;
                    lmax = -INFINITY;
                }
                vit_lds_sync();
                // the chunk's probabilities, contiguous across lanes
                const int s0 = cc.c * kWave, n_el = min(kWave, S - s0) * N;
                const int64_t o0 = (int64_t)cc.t * o.stride_t + (int64_t)s0 * N;
                const float *sp = stage + par * kTrStage;
                for (int el = lane; el < n_el; el += kWave) store_p(o0 + el, sp[el]);
                par ^= 1;
                cur_next(cc);
            }
        }
    }

    // init[s] = exp(beta~_0[s]) / sum_s exp(beta~_0[s]); logZ = sum_t c_t + ln of that sum
    const float *b0 = beta;
    float zs = 0.0f;
    for (int s = lane; s < S; s += kWave) zs += FCD_TR_EXP(b0[s] - cprev);
    for (int m = 1; m < kWave; m <<= 1) zs += __shfl_xor(zs, m);
    const bool failed = ballot(badx) != 0ull || no_path;
    float *init = o.init ? o.init + r * o.init_stride : lds;
    for (int s = lane; s < S; s += kWave) init[s] = FCD_TR_EXP(b0[s] - cprev) / zs;
    if (lane == 0) {
        o.status[r] = failed ? FCD_ST_INCOMPARABLE : FCD_ST_OK;
        if (o.logz) o.logz[r] = failed ? (double)NAN : csum + log((double)zs);
    }
    return failed;
}

// ---- CRF edge marginals over all labellings (fcd_crf_marginals_*; include/fcd.h has the definition) ----
// NOT a reference function.  The forward half behind crf_transitions_walk, which has left p[t][s][a] in the marginals' buffer
// (f32, the walk's own storage) and the init row in LDS.  (p, init) is the model restated as a Markov chain, so the forward
// pass is a propagation of state occupancies without exp or ln:
//     pi_0 = init;  marg[t][s][a] = pi_t[s] p[t][s][a];  pi_{t+1}[s'] = marg[t][s'][0] + sum_i marg[t][s_i][j + 1]
// with s_i = s' div nb + i (S / nb), j = s' mod nb, the sum taken in that order, left to right, from the stay term on.
// One wavefront per read, front to back, every row multiplied in place.  Rows of at most 64 elements: a lane per element,
// pi_t[s] in a register of every lane of state s, the products meeting through a double-buffered LDS row.  Larger rows: a
// lane per DESTINATION state s', 64 at a time, which gathers p[t][s'][0] and the nb elements p[t][s_i][j + 1] (s_i N + j + 1
// = (s' div nb) N + j + 1 + i (S / nb) N: for consecutive s' the advances of one i are consecutive elements but for the
// stay column), pi in two LDS rows of S floats.  (s', i) -> element is a bijection onto the row, so every element is loaded,
// multiplied and stored exactly once, BY THE SAME LANE: a lane's store follows its own load of that element in program
// order, and no other lane touches it, so a row's loads are consumed before it is overwritten without any further fence;
// the loads running ahead (kTrAhead rows, kTrRows chunks) are of other elements.  That leaves the stores scattered rather
// than staged: N runs per chunk, the advance runs dense but for every N-th element.
// emit[t][a] = sum_s marg[t][s][a]: through the LDS row with a lane per element; with a lane per state, lane-private LDS
// accumulators per advance column (the column a lane serves changes from chunk to chunk) and one shuffle reduction a row.
__device__ __forceinline__ void crf_marginals_forward(const BatchDesc &in, const VitArgs &va, float *lds) {
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    int64_t T = in.T;
    if (in.lengths) {
        int64_t t = in.lengths[r];
        T = t < 0 ? 0 : (t < T ? t : T);
    }
    const int Tr = (int)T;
    const int N = in.N, S = in.S, nb = N - 1, q = S / nb;
    const TransitionsDesc &o = va.tr;
    float *mg = reinterpret_cast<float *>(o.probs) + r * o.stride_read;
    float *em = va.emit ? va.emit + r * va.emit_stride : nullptr;
    float *pi = lds, *stage = lds + 2 * (size_t)S;
    const int E = S * N;

    if (E <= kWave) {  // ---- a lane per element e = s N + a ----
        const bool act = lane < E;
        const int e = act ? lane : 0, s = e / N;
        const int hi = s / nb, j = s - hi * nb;
        float pv = pi[s];  // pi_t[s]
        float ring[kTrAhead];
#pragma unroll
        for (int u = 0; u < kTrAhead; ++u) ring[u] = (act && u < Tr) ? mg[(int64_t)u * o.stride_t + e] : 0.0f;
        int par = 0;
        for (int k0 = 0; k0 < Tr; k0 += kTrAhead) {
#pragma unroll
            for (int u = 0; u < kTrAhead; ++u) {
                const int t = k0 + u;
                if (t >= Tr) break;
                const float m = pv * ring[u];
                if (act && t + kTrAhead < Tr) ring[u] = mg[(int64_t)(t + kTrAhead) * o.stride_t + e];
                float *sg = stage + par * kTrStage;
                if (act) {
                    mg[(int64_t)t * o.stride_t + e] = m;
                    sg[e] = m;
                }
                vit_lds_sync();
                float nx = sg[s * N];
                for (int i = 0; i < nb; ++i) nx += sg[(hi + i * q) * N + j + 1];
                pv = nx;
                if (em && lane < N) {
                    float z = 0.0f;
                    for (int k = 0; k < S; ++k) z += sg[k * N + lane];
                    em[(int64_t)t * N + lane] = z;
                }
                par ^= 1;  // (row t + 2 writes this buffer again behind row t + 1's barrier: every lane has read it by then)
            }
        }
        return;
    }

    // ---- a lane per destination state, 64 states (a chunk) at a time; the items (row, chunk) in the order they are walked ----
    const int nchunk = (S + kWave - 1) / kWave;
    // state s' = h nb + j: it is entered from h + i q by symbol j + 1
    const int h0 = lane / nb, j0 = lane - h0 * nb, steph = kWave / nb, stepj = kWave - steph * nb;
    const int qn = q * N;
    struct Cur {
        int t, c, s, h, j;
    };
    auto cur_next = [&](Cur &k) {
        if (++k.c == nchunk) {
            k.c = 0;
            ++k.t;
            k.s = lane;
            k.h = h0;
            k.j = j0;
        } else {
            k.s += kWave;
            k.h += steph;
            k.j += stepj;
            if (k.j >= nb) {
                k.j -= nb;
                ++k.h;
            }
        }
    };
    auto load_row = [&](const Cur &k, float (&p)[kVitMaxN]) {
#pragma unroll
        for (int i = 0; i < kVitMaxN; ++i) p[i] = 0.0f;
        if (k.t >= Tr || k.s >= S) return;
        const float *row = mg + (int64_t)k.t * o.stride_t;
        const float *adv = row + (k.h * N + k.j + 1);
        p[0] = row[k.s * N];
#pragma unroll
        for (int i = 1; i < kVitMaxN; ++i)
            if (i < N) p[i] = adv[(i - 1) * qn];
    };
    Cur lc{0, 0, lane, h0, j0}, cc = lc;
    float ring[kTrRows][kVitMaxN];
#pragma unroll
    for (int u = 0; u < kTrRows; ++u) {
        load_row(lc, ring[u]);
        cur_next(lc);
    }
    float *acc = stage + lane;  // advance column j + 1 of the row so far: acc[j * kWave], this lane's own
    if (em)
        for (int i = 0; i < nb; ++i) acc[i * kWave] = 0.0f;
    float e0 = 0.0f;  // the stay column
    const int64_t items = (int64_t)Tr * nchunk;
    for (int64_t k0 = 0; k0 < items; k0 += kTrRows) {
#pragma unroll
        for (int u = 0; u < kTrRows; ++u) {
            if (k0 + u >= items) break;
            float m[kVitMaxN];
#pragma unroll
            for (int i = 0; i < kVitMaxN; ++i) m[i] = ring[u][i];
            load_row(lc, ring[u]);
            cur_next(lc);
            if (cc.s < S) {
                const float *pt = pi + (size_t)(cc.t & 1) * S;
                float *row = mg + (int64_t)cc.t * o.stride_t;
                float *adv = row + (cc.h * N + cc.j + 1);
                m[0] *= pt[cc.s];
                row[cc.s * N] = m[0];
                float nx = m[0], sa = 0.0f;
#pragma unroll
                for (int i = 1; i < kVitMaxN; ++i) {
                    if (i >= N) break;
                    m[i] *= pt[cc.h + (i - 1) * q];
                    adv[(i - 1) * qn] = m[i];
                    nx += m[i];
                    sa += m[i];
                }
                pi[(size_t)((cc.t + 1) & 1) * S + cc.s] = nx;
                if (em) {
                    e0 += m[0];
                    acc[cc.j * kWave] += sa;
                }
            }
            if (cc.c == nchunk - 1) {  // the row is complete
                if (em) {
                    float mine = 0.0f;  // lane a ends up with column a
                    for (int m2 = 1; m2 < kWave; m2 <<= 1) e0 += __shfl_xor(e0, m2);
                    if (lane == 0) mine = e0;
                    e0 = 0.0f;
                    for (int i = 0; i < nb; ++i) {
                        float v = acc[i * kWave];
                        acc[i * kWave] = 0.0f;
                        for (int m2 = 1; m2 < kWave; m2 <<= 1) v += __shfl_xor(v, m2);
                        if (lane == i + 1) mine = v;
                    }
                    if (lane < N) em[(int64_t)cc.t * N + lane] = mine;
                }
                vit_lds_sync();  // pi_{t+1} is in place before row t + 1 reads it; its other row is free to be written
            }
            cur_next(cc);
        }
    }
}

// crf_greedy_search (:385-423): the state walk is a serial dependency; one wave per read,
// lanes 0..N-1 hold the current state's row and reduce it with a first-maximum argmax.
// va.mode (wave-uniform) = 1: the Viterbi walk above instead, 2: the transition-probability walk, 3: that walk and the
// marginals' forward pass behind it -- the launches with dynamic LDS.
__global__ __launch_bounds__(64) void crf_greedy_kernel(BatchDesc in, const float *init_all,
                                                      int64_t n_init, int64_t init_stride,
                                                      ResultDesc out, VitArgs va) {
    extern __shared__ __attribute__((aligned(16))) float s_vit[];
    if (va.mode >= 2) {
        const bool failed = crf_transitions_walk(in, va, s_vit);
        if (va.mode == 3 && !failed) {
            // The forward pass reads p back from the marginals' buffer: global memory that OTHER lanes of this wavefront
            // stored (the backward pass stores a chunk's elements as contiguous runs across lanes, the forward pass gathers
            // them by destination state).  The release fence at device scope makes every lane's stores visible beyond the
            // lane before any lane passes the wave barrier, the acquire fence behind it keeps the loads below from being
            // served by anything older.  The init row in LDS needs the same between lanes at wavefront scope.
            vit_global_sync();
            vit_lds_sync();
            crf_marginals_forward(in, va, s_vit);
        }
        return;
    }
    if (va.mode) {
        crf_viterbi_walk(in, init_all, n_init, init_stride, out, va, s_vit);
        return;
    }
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    int64_t T = in.T;
    if (in.lengths) {
        int64_t t = in.lengths[r];
        T = t < 0 ? 0 : (t < T ? t : T);
    }
    const int N = in.N, S = in.S, n_base = N - 1;
    const int dt = in.dtype;
    const float *post = post_at(in.post, r * in.stride_read, dt);
    uint8_t *lab = out.labels + r * out.out_stride;
    uint32_t *pth = out.path ? out.path + r * out.out_stride : nullptr;
    float *qual = out.qual ? out.qual + r * out.out_stride : nullptr;

    // init_state.argmax() :399 (first maximum; NaN -> the reference panics)
    const float *init = init_all + r * init_stride;
    int state = 0;
    bool bad = n_init <= 0;
    if (!bad) {
        float m = init[0];
        bad = m != m;
        for (int64_t j = 1; j < n_init && !bad; ++j) {
            const float e = init[j];
            if (e != e) bad = true;
            if (e > m) {
                m = e;
                state = (int)j;
            }
        }
    }
    int n_out = 0;
    for (int64_t t = 0; t < T && !bad; ++t) {
        if (state < 0 || state >= S) {
            bad = true;
            break;
        }
        const float *pr = post_at(post, t * in.stride_t + (int64_t)state * in.stride_s, dt);
        // argmax over N columns, N may exceed 64: strided per-lane first-max, then wave reduce
        float best = 0.0f;
        int arg = 1 << 30;
        bool nan = false;
        for (int j = lane; j < N; j += kWave) {
            const float v = load_post(pr, j * in.stride_n, dt);
            nan = nan || (v != v);
            if (arg == (1 << 30) || v > best) {
                best = v;
                arg = j;
            }
        }
        if (__ballot(nan) != 0ull) {
            bad = true;
            break;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const int oa = __shfl_xor(arg, off);
            if (oa != (1 << 30) && (arg == (1 << 30) || ob > best || (ob == best && oa < arg))) {
                best = ob;
                arg = oa;
            }
        }
        if (arg > 0) {  // :409-416
            if (lane == 0) {
                lab[n_out] = (uint8_t)arg;
                if (pth) pth[n_out] = (uint32_t)t;
                if (qual) qual[n_out] = best;
            }
            n_out++;
            state = (int)(((int64_t)state * n_base) % S) + (arg - 1);
        }
    }
    if (lane == 0) {
        out.out_len[r] = bad ? 0u : (uint32_t)n_out;
        if (out.status) out.status[r] = bad ? FCD_ST_BAD_STATE : FCD_ST_OK;
    }
}


// crf_greedy_search for small state counts (S <= 8), streamed at HBM rate.
//
// The state walk looks serial -- row t is read at the state row t-1 left behind -- but over S states
// row t is just a function f_t : state -> state (with one extra absorbing value for "out of range",
// where the reference aborts).  So: every lane takes one row of a 64-row tile, evaluates the
// first-maximum argmax for ALL S states of its row, packs f_t into 4-bit entries of a 64-bit word,
// and an inclusive wave scan of function COMPOSITION (six shuffle steps) yields the state every row is
// entered with.  The visited state then selects each row's label / probability / NaN flag, and the
// emissions are compacted with ballot + prefix popcount like viterbi_search's.  Tiles arrive through
// LDS with 16-byte coalesced loads; the next tile is in flight while the current one is scanned.
// A state -> state function over S + 1 <= 16 values, as 4-bit entries of a 64-bit word; for S <= 7
// the entries are whole BYTES instead (8 of them), because then composing two functions is exactly
// what v_perm_b32 does -- pick bytes of one operand pair by the selector bytes of another: two
// instructions per composition instead of ~30 shift/mask operations.
template <int S>
struct FnTable {
    static constexpr bool kBytes = S <= 7;
    static constexpr int kBits = kBytes ? 8 : 4;
    __device__ static __forceinline__ uint64_t compose(uint64_t first, uint64_t then) {
        // (then o first)[s] = then[first[s]]
        if (kBytes) {
            const uint32_t tl = (uint32_t)then, th = (uint32_t)(then >> 32);
            const uint32_t lo = __builtin_amdgcn_perm(th, tl, (uint32_t)first);
            const uint32_t hi = __builtin_amdgcn_perm(th, tl, (uint32_t)(first >> 32));
            return ((uint64_t)hi << 32) | lo;
        }
        uint64_t out = 0;
#pragma unroll
        for (int s = 0; s <= S; ++s) {
            const int mid = (int)((first >> (4 * s)) & 15ull);
            out |= ((then >> (4 * mid)) & 15ull) << (4 * s);
        }
        return out;
    }
    __device__ static __forceinline__ uint64_t identity() {
        if (kBytes) return 0x0706050403020100ull;
        uint64_t id = 0;
#pragma unroll
        for (int s = 0; s <= S; ++s) id |= (uint64_t)s << (4 * s);
        return id;
    }
    __device__ static __forceinline__ uint64_t entry(int s, int value) { return (uint64_t)value << (kBits * s); }
    __device__ static __forceinline__ int at(uint64_t f, int s) {
        return (int)((f >> (kBits * s)) & (kBytes ? 255ull : 15ull));
    }
};

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int o) {
    const int lo = __shfl_up((int)(uint32_t)v, o), hi = __shfl_up((int)(uint32_t)(v >> 32), o);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

constexpr int kCrfTileRows = 64;

// TM: time-major storage, (T, B, S, N) seen as a batch (stride_read = S * N): the four wavefronts of a workgroup take four
// NEIGHBOURING reads, whose rows of one time step are one contiguous run of 4 * S * N floats; the workgroup pulls 64-step
// tiles of the four together (coalesced 16-byte loads), parks them as [step][read][S * N] with an odd pitch, and every
// wavefront scans its read exactly as below.  (viterbi_tm_kernel is the same idea for the plain search.)
template <int S, bool TM>
__global__ __launch_bounds__(64 * kWavesPerBlock) void crf_greedy_stream_kernel(
    BatchDesc in, const float *init_all, int64_t n_init, int64_t init_stride, ResultDesc out) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    const int lane = threadIdx.x & 63;
    // (wave-uniform, and said so: the read's index, its length and every pointer derived from them live in scalar registers)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (TM) {  // every XCD takes a contiguous range of read groups: neighbouring groups share cache lines
        const unsigned n_groups = gridDim.x, per_xcd = (n_groups + 7) / 8;
        unsigned gidx = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
        if (n_groups < 64 || gidx >= n_groups || (n_groups & 7)) gidx = blockIdx.x;
        r = (int64_t)gidx * kWavesPerBlock + wave;  // (the launch covers whole groups only: every read exists)
    } else if (r >= in.n_reads) {
        return;
    }
    int64_t T = in.T;
    if (in.lengths) {
        int64_t t = in.lengths[r];
        T = t < 0 ? 0 : (t < T ? t : T);
    }
    const int N = in.N, n_base = N - 1;
    const int E = S * N;                      // floats per row
    const int tile_f = kCrfTileRows * E;      // floats per tile
    const int nload = TM ? (E + 3) / 4 : (tile_f / 4 + 63) / 64;  // float4 loads per lane and tile
    const int pitch = TM ? kWavesPerBlock * E + 1 : E;            // floats between consecutive rows of a read in the tile
    float *tile = TM ? s_dyn + wave * E : s_dyn + (size_t)wave * tile_f;
    const float *post = in.post + r * in.stride_read;
    const int64_t total = T * E;
    const int64_t T_loop = TM ? in.T : T;     // (TM: the workgroup's tiles cover the longest read of the batch)
    const int tm_step = (int)(threadIdx.x >> 2), tm_sub = (int)(threadIdx.x & 3);  // TM: four threads per time step
    const float *tm_base = in.post + (r - wave) * in.stride_read;                  // TM: the group's first read
    uint8_t *lab = out.labels + r * out.out_stride;
    uint32_t *pth = out.path ? out.path + r * out.out_stride : nullptr;
    float *qual = out.qual ? out.qual + r * out.out_stride : nullptr;

    // init_state.argmax() :399 (first maximum; NaN -> the reference panics)
    const float *init = init_all + r * init_stride;
    int state = 0;
    bool bad = n_init <= 0;
    if (!bad) {
        float m = init[0];
        bad = m != m;
        for (int64_t j = 1; j < n_init && !bad; ++j) {
            const float e = init[j];
            if (e != e) bad = true;
            if (e > m) {
                m = e;
                state = (int)j;
            }
        }
    }
    if (state >= S) state = S;  // out of range: the first row would abort

    constexpr int kMaxLoads = 8;  // S * N <= 32 floats per row (the launcher checks)
    float4 cur[kMaxLoads], nxt[kMaxLoads];
    auto fetch = [&](int64_t row0, float4 (&v)[kMaxLoads]) {
        if (TM) {
            // thread (step, sub) takes the 16-byte units sub, sub + 4, ... of its time step's run of 4 * E floats
            const float *src = tm_base + (row0 + tm_step) * in.stride_t;
#pragma unroll
            for (int m = 0; m < kMaxLoads; ++m) {
                if (m >= nload) break;
                const int o = tm_sub + 4 * m;
                v[m] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (o < E && row0 + tm_step < in.T) v[m] = *reinterpret_cast<const float4 *>(src + o * 4);
            }
            return;
        }
        const int64_t f0 = row0 * E;
#pragma unroll
        for (int m = 0; m < kMaxLoads; ++m) {
            if (m >= nload) break;
            const int64_t fl = (int64_t)(lane + 64 * m) * 4;  // float offset inside the tile
            const int64_t f = f0 + fl;
            if (fl + 3 < tile_f && f + 3 < total) {
                v[m] = *reinterpret_cast<const float4 *>(post + f);
            } else {
                v[m].x = (fl < tile_f && f < total) ? post[f] : 0.0f;
                v[m].y = (fl + 1 < tile_f && f + 1 < total) ? post[f + 1] : 0.0f;
                v[m].z = (fl + 2 < tile_f && f + 2 < total) ? post[f + 2] : 0.0f;
                v[m].w = (fl + 3 < tile_f && f + 3 < total) ? post[f + 3] : 0.0f;
            }
        }
    };

    int n_out = 0;
    if (T_loop > 0) fetch(0, cur);
    for (int64_t base = 0; base < T_loop; base += kCrfTileRows) {
        if (base + kCrfTileRows < T_loop) fetch(base + kCrfTileRows, nxt);
        if (TM) {
#pragma unroll
            for (int m = 0; m < kMaxLoads; ++m) {
                if (m >= nload) break;
                const int o = tm_sub + 4 * m;
                if (o < E) {
                    float *dst = s_dyn + tm_step * pitch + o * 4;  // (odd pitch: 4-byte alignment only)
                    dst[0] = cur[m].x;
                    dst[1] = cur[m].y;
                    dst[2] = cur[m].z;
                    dst[3] = cur[m].w;
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int m = 0; m < kMaxLoads; ++m) {
            if (TM || m >= nload) break;
            const int fl = (lane + 64 * m) * 4;
            if (fl + 3 < tile_f) {
                *reinterpret_cast<float4 *>(tile + fl) = cur[m];
            } else {
                if (fl < tile_f) tile[fl] = cur[m].x;
                if (fl + 1 < tile_f) tile[fl + 1] = cur[m].y;
                if (fl + 2 < tile_f) tile[fl + 2] = cur[m].z;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        const int64_t row = base + lane;
        const bool act = row < T;
        if (!TM || base < T) {  // (TM: a wavefront whose read has ended still takes part in the tile loads)
        // this row, for every state: first-maximum argmax (:405), its probability, NaN anywhere in the row
        const float *pr = tile + lane * pitch;
        float prob_s[S];
        uint32_t labels_packed = 0, nan_mask = 0;
        uint64_t f = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            float best = pr[s * N];
            int arg = 0;
            bool nan = best != best;
            for (int j = 1; j < N; ++j) {
                const float v = pr[s * N + j];
                nan = nan || (v != v);
                if (v > best) {
                    best = v;
                    arg = j;
                }
            }
            prob_s[s] = best;
            labels_packed |= (uint32_t)arg << (4 * s);
            nan_mask |= nan ? (1u << s) : 0u;
            int next = arg > 0 ? (s * n_base) % S + (arg - 1) : s;  // :415
            if (next >= S) next = S;
            f |= FnTable<S>::entry(s, next);
        }
        // out of range stays out of range (byte tables: the unused upper entries map to themselves)
        if (FnTable<S>::kBytes) {
#pragma unroll
            for (int s2 = S; s2 < 8; ++s2) f |= FnTable<S>::entry(s2, s2 == S ? S : s2);
        } else {
            f |= FnTable<S>::entry(S, S);
        }
        if (!act) f = FnTable<S>::identity();  // rows past the end change nothing

        // inclusive scan of composition: F_k = f_k o ... o f_0
        uint64_t F = f;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint64_t g = shfl_up_u64(F, o);
            if (lane >= o) F = FnTable<S>::compose(g, F);
        }
        // the state this row is entered with
        uint64_t Fprev = shfl_up_u64(F, 1);
        if (lane == 0) Fprev = FnTable<S>::identity();
        const int st = FnTable<S>::at(Fprev, state);
        // the state the tile leaves behind (wave-uniform)
        const uint64_t Flast = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(F >> 32), 63) << 32) |
                               (uint32_t)__shfl((int)(uint32_t)F, 63);
        const int state_out = FnTable<S>::at(Flast, state);

        // a row entered out of range, or a NaN in the visited state's row: the reference aborts
        const bool row_bad = act && (st >= S || ((nan_mask >> (st < S ? st : 0)) & 1u));
        if (ballot(row_bad) != 0ull) bad = true;
        int label = 0;
        float prob = 0.0f;
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (st == s) {
                label = (int)((labels_packed >> (4 * s)) & 15u);
                prob = prob_s[s];
            }
        const bool emit = act && !row_bad && label > 0;
        const uint64_t m_emit = ballot(emit);
        const int my_out = n_out + popc64(m_emit & lanemask_lt());
        if (emit) {
            lab[my_out] = (uint8_t)label;
            if (pth) pth[my_out] = (uint32_t)row;
            if (qual) qual[my_out] = prob;
        }
        n_out += popc64(m_emit);
        state = state_out;
        }
        if (TM) __syncthreads();
        else __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int m = 0; m < kMaxLoads; ++m) cur[m] = nxt[m];
    }
    if (lane == 0) {
        out.out_len[r] = bad ? 0u : (uint32_t)n_out;
        if (out.status) out.status[r] = bad ? FCD_ST_BAD_STATE : FCD_ST_OK;
    }
}

}  // namespace

hipError_t launch_viterbi(const BatchDesc &in, int collapse, const ResultDesc &out,
                          hipStream_t stream) {
    if (in.n_reads <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((in.n_reads + kWavesPerBlock - 1) / kWavesPerBlock);
    const dim3 grid(blocks), block(64 * kWavesPerBlock);
    // 16-byte loads: every read must start on a 16-byte boundary (4 f32 / 8 half elements)
    const bool stream_ok = in.stride_n == 1 && in.stride_t == in.N && (in.stride_read % (in.dtype == kF32 ? 4 : 8)) == 0 &&
                           (reinterpret_cast<uintptr_t>(in.post) % 16) == 0;
    // time-major storage ((T, B, N) seen as a batch): neighbouring reads are N elements apart
    const int64_t esz = in.dtype == kF32 ? 4 : 2;
    const bool tm_ok = in.stride_n == 1 && in.stride_read == in.N && in.N >= 2 && in.N <= 8 && in.n_reads >= kTmReads &&
                       in.stride_t >= in.n_reads * in.N && (in.stride_t * esz) % 16 == 0 &&
                       (reinterpret_cast<uintptr_t>(in.post) % 16) == 0;
    if (tm_ok) {
        const int64_t groups = in.n_reads / kTmReads, done = groups * kTmReads;
        switch (in.N) {
#define FCD_VTM(NN)                                                                                                 \
    case NN:                                                                                                        \
        if (in.dtype == kF32)                                                                                       \
            hipLaunchKernelGGL((viterbi_tm_kernel<NN, kF32>), dim3((unsigned)groups), dim3(256), 0, stream, in, collapse, out);  \
        else if (in.dtype == kF16)                                                                                  \
            hipLaunchKernelGGL((viterbi_tm_kernel<NN, kF16>), dim3((unsigned)groups), dim3(256), 0, stream, in, collapse, out);  \
        else                                                                                                        \
            hipLaunchKernelGGL((viterbi_tm_kernel<NN, kBF16>), dim3((unsigned)groups), dim3(256), 0, stream, in, collapse, out); \
        break;
            FCD_VTM(2) FCD_VTM(3) FCD_VTM(4) FCD_VTM(5) FCD_VTM(6) FCD_VTM(7) FCD_VTM(8)
#undef FCD_VTM
            default: break;
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess || done == in.n_reads) return e;
        // the last n_reads mod 8 reads: the strided kernel on the tail of the batch
        BatchDesc in2 = in;
        in2.post = reinterpret_cast<const float *>(reinterpret_cast<const char *>(in.post) + done * in.stride_read * esz);
        in2.lengths = in.lengths ? in.lengths + done : nullptr;
        in2.n_reads = in.n_reads - done;
        ResultDesc out2 = out;
        out2.labels = out.labels + done * out.out_stride;
        out2.path = out.path ? out.path + done * out.out_stride : nullptr;
        out2.qual = out.qual ? out.qual + done * out.out_stride : nullptr;
        out2.out_len = out.out_len + done;
        out2.status = out.status ? out.status + done : nullptr;
        const unsigned blocks2 = (unsigned)((in2.n_reads + kWavesPerBlock - 1) / kWavesPerBlock);
        hipLaunchKernelGGL(viterbi_kernel, dim3(blocks2), block, 0, stream, in2, collapse, out2);
        return hipGetLastError();
    }
    if (stream_ok) {
        switch (in.N) {
#define FCD_VSTREAM(NN)                                                                                         \
    case NN:                                                                                                    \
        if (in.dtype == kF32)                                                                                   \
            hipLaunchKernelGGL((viterbi_stream_kernel<NN, kF32>), grid, block, 0, stream, in, collapse, out);   \
        else if (in.dtype == kF16)                                                                              \
            hipLaunchKernelGGL((viterbi_stream_kernel<NN, kF16>), grid, block, 0, stream, in, collapse, out);   \
        else                                                                                                    \
            hipLaunchKernelGGL((viterbi_stream_kernel<NN, kBF16>), grid, block, 0, stream, in, collapse, out);  \
        return hipGetLastError();
            FCD_VSTREAM(2) FCD_VSTREAM(3) FCD_VSTREAM(4) FCD_VSTREAM(5) FCD_VSTREAM(6) FCD_VSTREAM(7)
            FCD_VSTREAM(8)
#undef FCD_VSTREAM
            default: break;
        }
    }
    hipLaunchKernelGGL(viterbi_kernel, grid, block, 0, stream, in, collapse, out);
    return hipGetLastError();
}

hipError_t launch_crf_greedy(const BatchDesc &in, const float *init, int64_t n_init,
                             int64_t init_stride, const ResultDesc &out, hipStream_t stream) {
    if (in.n_reads <= 0) return hipSuccess;
    // small state counts, C-contiguous rows: the streaming kernel (function-composition scan)
    const int64_t E = (int64_t)in.S * in.N;
    // (half-precision input takes the serial kernel below: the function-composition scan reads f32 tiles)
    const bool stream_ok = in.dtype == kF32 && in.S >= 1 && in.S <= 8 && in.N >= 1 && in.N <= 15 && E <= 32 && in.stride_n == 1 &&
                           in.stride_s == in.N && in.stride_t == E && (in.stride_read % 4) == 0 &&
                           (reinterpret_cast<uintptr_t>(in.post) % 16) == 0;
    if (stream_ok) {
        const unsigned blocks = (unsigned)((in.n_reads + kWavesPerBlock - 1) / kWavesPerBlock);
        const size_t lds = (size_t)kWavesPerBlock * kCrfTileRows * E * sizeof(float);
        switch (in.S) {
#define FCD_GSTREAM(SS)                                                                                   \
    case SS:                                                                                              \
        hipLaunchKernelGGL((crf_greedy_stream_kernel<SS, false>), dim3(blocks), dim3(64 * kWavesPerBlock), lds, stream, \
                           in, init, n_init, init_stride, out);                                           \
        return hipGetLastError();
            FCD_GSTREAM(1) FCD_GSTREAM(2) FCD_GSTREAM(3) FCD_GSTREAM(4) FCD_GSTREAM(5) FCD_GSTREAM(6)
            FCD_GSTREAM(7) FCD_GSTREAM(8)
#undef FCD_GSTREAM
            default: break;
        }
    }
    // time-major storage ((T, B, S, N) seen as a batch): neighbouring reads are S * N floats apart
    const bool tm_ok = in.dtype == kF32 && in.S >= 1 && in.S <= 8 && in.N >= 1 && in.N <= 15 && E <= 32 && in.stride_n == 1 &&
                       in.stride_s == in.N && in.stride_read == E && in.n_reads >= kWavesPerBlock &&
                       in.stride_t >= in.n_reads * E && (in.stride_t % 4) == 0 &&
                       (reinterpret_cast<uintptr_t>(in.post) % 16) == 0;
    int64_t done = 0;
    if (tm_ok) {
        const int64_t groups = in.n_reads / kWavesPerBlock;
        const size_t lds = (size_t)kCrfTileRows * (kWavesPerBlock * E + 1) * sizeof(float);
        switch (in.S) {
#define FCD_GTM(SS)                                                                                              \
    case SS:                                                                                                     \
        hipLaunchKernelGGL((crf_greedy_stream_kernel<SS, true>), dim3((unsigned)groups), dim3(64 * kWavesPerBlock), lds, \
                           stream, in, init, n_init, init_stride, out);                                          \
        done = groups * kWavesPerBlock;                                                                          \
        break;
            FCD_GTM(1) FCD_GTM(2) FCD_GTM(3) FCD_GTM(4) FCD_GTM(5) FCD_GTM(6) FCD_GTM(7) FCD_GTM(8)
#undef FCD_GTM
            default: break;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess || done == in.n_reads) return e;
    }
    // (everything else, and the last n_reads mod 4 reads of a time-major batch: the serial walk)
    BatchDesc in2 = in;
    in2.post = in.post + done * in.stride_read;  // (done > 0 only for float32 input: plain element arithmetic)
    in2.lengths = in.lengths ? in.lengths + done : nullptr;
    in2.n_reads = in.n_reads - done;
    ResultDesc out2 = out;
    out2.labels = out.labels + done * out.out_stride;
    out2.path = out.path ? out.path + done * out.out_stride : nullptr;
    out2.qual = out.qual ? out.qual + done * out.out_stride : nullptr;
    out2.out_len = out.out_len + done;
    out2.status = out.status ? out.status + done : nullptr;
    hipLaunchKernelGGL(crf_greedy_kernel, dim3((unsigned)in2.n_reads), dim3(64), 0, stream, in2, init + done * init_stride,
                       n_init, init_stride, out2, VitArgs{});
    return hipGetLastError();
}

namespace {
size_t crf_viterbi_lds_bytes(int64_t S, int64_t N) {  // v and c, and never less than the traceback's chunk wants
    return std::max<size_t>((size_t)N * (size_t)S * 4, kVitMinLds);
}
}  // namespace

int crf_viterbi_unsupported(int64_t S, int64_t N) {
    if (N < 2 || N > kVitMaxN) return 1;
    if (S % (N - 1) != 0) return 2;
    if (S >= (1ll << 24)) return 3;
    if (crf_viterbi_lds_bytes(S, N) > 160 * 1024) return 4;
    return 0;
}

size_t crf_viterbi_read_bytes(int64_t T, int64_t S) {
    return ((size_t)std::max<int64_t>(T, 1) * (size_t)S + 255) & ~(size_t)255;
}

hipError_t launch_crf_viterbi(const BatchDesc &in, const float *init, int64_t n_init, int64_t init_stride,
                              const ResultDesc &out, double *logp, unsigned char *bp, hipStream_t stream) {
    if (in.n_reads <= 0) return hipSuccess;
    VitArgs va{};
    va.mode = 1;
    va.lds_bytes = (int)crf_viterbi_lds_bytes(in.S, in.N);
    va.logp = logp;
    va.bp = bp;
    va.bp_read_bytes = (int64_t)crf_viterbi_read_bytes(in.T, in.S);
#ifndef FCD_HIPEMU
    if (va.lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(crf_greedy_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, va.lds_bytes);
        if (e != hipSuccess) return e;
    }
#endif
    hipLaunchKernelGGL(crf_greedy_kernel, dim3((unsigned)in.n_reads), dim3(64), (size_t)va.lds_bytes, stream, in, init, n_init,
                       init_stride, out, va);
    return hipGetLastError();
}

namespace {
size_t crf_transitions_lds_bytes(int64_t S) {  // two rows of the backward vector, two staging buffers
    return ((size_t)2 * (size_t)S + 2 * kTrStage) * 4;
}
}  // namespace

int crf_transitions_unsupported(int64_t S, int64_t N) {
    if (N < 2 || N > kVitMaxN) return 1;
    if (S % (N - 1) != 0) return 2;
    if (S >= (1ll << 24)) return 3;
    if (crf_transitions_lds_bytes(S) > 160 * 1024) return 4;
    return 0;
}

hipError_t launch_crf_transitions(const BatchDesc &in, const TransitionsDesc &out, hipStream_t stream) {
    return launch_crf_marginals(in, out, nullptr, 0, stream, 2);
}

// mode 3: out.probs is the marginals' buffer (f32), out.init null; mode 2 (launch_crf_transitions): emit unused
hipError_t launch_crf_marginals(const BatchDesc &in, const TransitionsDesc &out, float *emit, int64_t emit_stride,
                                hipStream_t stream, int mode) {
    if (in.n_reads <= 0) return hipSuccess;
    VitArgs va{};
    va.mode = mode;
    va.lds_bytes = (int)crf_transitions_lds_bytes(in.S);
    va.tr = out;
    va.emit = emit;
    va.emit_stride = emit_stride;
#ifndef FCD_HIPEMU
    if (va.lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(crf_greedy_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, va.lds_bytes);
        if (e != hipSuccess) return e;
    }
#endif
    hipLaunchKernelGGL(crf_greedy_kernel, dim3((unsigned)in.n_reads), dim3(64), (size_t)va.lds_bytes, stream, in,
                       static_cast<const float *>(nullptr), (int64_t)0, (int64_t)0, ResultDesc{}, va);
    return hipGetLastError();
}

}  // namespace fcd
