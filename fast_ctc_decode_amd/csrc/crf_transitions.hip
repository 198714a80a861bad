// crf_transitions.hip -- CRF transition probabilities from raw scores (fcd_crf_transition_probs_*) and the edge marginals
// that continue from them (fcd_crf_marginals_*, further down); include/fcd.h has the definitions.
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
#include <math.h>

#include "device_utils.h"
#include "fcd_internal.h"

namespace fcd {

namespace {

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

// -> whether the read failed (wave-uniform).  A null o.init (the marginals) leaves the init row in LDS instead, over
// beta~_0 at lds[0 .. S): every lane overwrites only the states it has just read.
__device__ __forceinline__ bool crf_transitions_walk(const BatchDesc &in, const TransitionsDesc &o, float *lds) {
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int Tr = (int)read_rows(in.T, in.lengths, r);
    const int N = in.N, S = in.S, nb = N - 1, q = S / nb;
    const int dt = in.dtype;
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
__device__ __forceinline__ void crf_marginals_forward(const BatchDesc &in, const TransitionsDesc &o, float *emit,
                                                      int64_t emit_stride, float *lds) {
    const int lane = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int Tr = (int)read_rows(in.T, in.lengths, r);
    const int N = in.N, S = in.S, nb = N - 1, q = S / nb;
    float *mg = reinterpret_cast<float *>(o.probs) + r * o.stride_read;
    float *em = emit ? emit + r * emit_stride : nullptr;
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

__global__ __launch_bounds__(64) void crf_transitions_kernel(BatchDesc in, TransitionsDesc o) {
    extern __shared__ __attribute__((aligned(16))) float s_tr[];
    (void)crf_transitions_walk(in, o, s_tr);
}

// o.probs is the marginals' buffer (f32), o.init null; emit [n_reads * emit_stride], (T, N) dense per read, nullable
__global__ __launch_bounds__(64) void crf_marginals_kernel(BatchDesc in, TransitionsDesc o, float *emit,
                                                         int64_t emit_stride) {
    extern __shared__ __attribute__((aligned(16))) float s_tr[];
    if (crf_transitions_walk(in, o, s_tr)) return;
    // The forward pass reads p back from the marginals' buffer: global memory that OTHER lanes of this wavefront
    // stored (the backward pass stores a chunk's elements as contiguous runs across lanes, the forward pass gathers
    // them by destination state).  The release fence at device scope makes every lane's stores visible beyond the
    // lane before any lane passes the wave barrier, the acquire fence behind it keeps the loads below from being
    // served by anything older.  The init row in LDS needs the same between lanes at wavefront scope.
    vit_global_sync();
    vit_lds_sync();
    crf_marginals_forward(in, o, emit, emit_stride, s_tr);
}

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
    if (in.n_reads <= 0) return hipSuccess;
    const int lds_bytes = (int)crf_transitions_lds_bytes(in.S);
    const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(crf_transitions_kernel), lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crf_transitions_kernel, dim3((unsigned)in.n_reads), dim3(64), (size_t)lds_bytes, stream, in, out);
    return hipGetLastError();
}

hipError_t launch_crf_marginals(const BatchDesc &in, const TransitionsDesc &out, float *emit, int64_t emit_stride,
                                hipStream_t stream) {
    if (in.n_reads <= 0) return hipSuccess;
    const int lds_bytes = (int)crf_transitions_lds_bytes(in.S);
    const hipError_t e = allow_dynamic_lds(reinterpret_cast<const void *>(crf_marginals_kernel), lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(crf_marginals_kernel, dim3((unsigned)in.n_reads), dim3(64), (size_t)lds_bytes, stream, in, out, emit,
                       emit_stride);
    return hipGetLastError();
}

}  // namespace fcd
