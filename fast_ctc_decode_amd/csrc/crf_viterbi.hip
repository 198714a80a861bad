// crf_viterbi.hip -- the Viterbi search under a CRF model (fcd_crf_viterbi_search_*; include/fcd.h has the definition).
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
#include <math.h>

#include <algorithm>

#include "device_utils.h"
#include "fcd_internal.h"

namespace fcd {

namespace {

constexpr int kVitMinLds = 4096;  // the traceback's chunk of back-pointers reuses the LDS: at least this much of it
constexpr int kVitAhead = 4;      // S * N <= 64: rows whose loads are in flight

// logp_all [n_reads], nullable; bp_all: the back-pointers, bp_read_bytes per read, row t and state s at [t * S + s];
// lds_bytes: the dynamic LDS of the launch, at lds
// (A function behind crf_viterbi_kernel, not the kernel's own body: written as the body, the same text was allocated
// differently -- the lane-per-state row loads reused the 16-bit load's register for an address and so each waited for the
// one before -- and the search ran 22 % longer at S = 64, float32)
__device__ __forceinline__ void crf_viterbi_walk(const BatchDesc &in, const float *init_all, int64_t n_init,
                                                 int64_t init_stride, const ResultDesc &out, double *logp_all,
                                                 unsigned char *bp_all, int64_t bp_read_bytes, int lds_bytes, float *lds) {
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int Tr = (int)read_rows(in.T, in.lengths, r);
    const int N = in.N, S = in.S, nb = N - 1;
    const int dt = in.dtype;
    const float *post = post_at(in.post, r * in.stride_read, dt);
    uint8_t *lab = out.labels + r * out.out_stride;
    uint32_t *pth = out.path ? out.path + r * out.out_stride : nullptr;
    float *qual = out.qual ? out.qual + r * out.out_stride : nullptr;

    // sigma_0: the first maximum of the init row, as crf_greedy_search takes it (:399)
    bool bad;
    const int state = init_first_max(init_all + r * init_stride, n_init, &bad);
    if (bad || Tr == 0 || state >= S) {  // (an init row no state follows from; no rows: the empty path, probability 1)
        const bool ok = !bad && Tr == 0;
        if (lane == 0) {
            out.out_len[r] = 0u;
            out.status[r] = ok ? FCD_ST_OK : FCD_ST_BAD_STATE;
            if (logp_all) logp_all[r] = ok ? 0.0 : (double)NAN;
        }
        return;
    }

    float *v = lds, *c = lds + S;
    for (int s = lane; s < S; s += kWave) v[s] = s == state ? 1.0f : 0.0f;  // "row -1"
    vit_lds_sync();
    unsigned char *bp = bp_all + r * bp_read_bytes;
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
            if (logp_all) logp_all[r] = (double)NAN;
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
    const int rows_per_chunk = max(1, (lds_bytes - 8) / S);
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
        if (logp_all) logp_all[r] = logp;
    }
}

__global__ __launch_bounds__(64) void crf_viterbi_kernel(BatchDesc in, const float *init_all, int64_t n_init,
                                                       int64_t init_stride, ResultDesc out, double *logp_all,
                                                       unsigned char *bp_all, int64_t bp_read_bytes, int lds_bytes) {
    extern __shared__ __attribute__((aligned(16))) float s_vit[];
    crf_viterbi_walk(in, init_all, n_init, init_stride, out, logp_all, bp_all, bp_read_bytes, lds_bytes, s_vit);
}

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
    const int lds_bytes = (int)crf_viterbi_lds_bytes(in.S, in.N);
    const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(crf_viterbi_kernel), lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crf_viterbi_kernel, dim3((unsigned)in.n_reads), dim3(64), (size_t)lds_bytes, stream, in, init, n_init,
                       init_stride, out, logp, bp, (int64_t)crf_viterbi_read_bytes(in.T, in.S), lds_bytes);
    return hipGetLastError();
}

}  // namespace fcd
