// device_utils.h -- wave64 helpers for the gfx950 search kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fcd {

constexpr int kWave = 64;  // CDNA wavefront width; hard-coded on purpose

__device__ __forceinline__ uint64_t lanemask_lt() {
    return (1ull << (threadIdx.x & 63)) - 1ull;
}

__device__ __forceinline__ int popc64(uint64_t m) { return __builtin_popcountll(m); }

// wave-wide vote straight from an i1 (no 0/1 materialisation + compare as __ballot(int) does)
__device__ __forceinline__ uint64_t ballot(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }

// Posterior element types (include/fcd.h: fcd_batch.dtype).  Basecaller networks emit half precision; the
// reference forces a host float32 copy (src/lib.rs:182,325).  Both 16-bit formats convert to binary32 EXACTLY, so
// a search on half-precision input is the reference's search on the upcast matrix, without a separate upcast pass.
enum { kF32 = 0, kF16 = 1, kBF16 = 2 };

#ifndef FCD_F16_TO_F32  // (tests/hipemu predefines a software conversion: its host compiler has no _Float16)
#define FCD_F16_TO_F32(h) ((float)__builtin_bit_cast(_Float16, (uint16_t)(h)))  // v_cvt_f32_f16: exact, subnormals included
#endif
__device__ __forceinline__ float f16_bits_to_f32(uint16_t h) { return FCD_F16_TO_F32(h); }
__device__ __forceinline__ float bf16_bits_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// binary32 -> binary16 bits, round to nearest even (v_cvt_f16_f32 under the default rounding mode)
__device__ __forceinline__ uint16_t f32_to_f16_bits(float v) {
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: its host compiler has no _Float16)
    const uint32_t u = __float_as_uint(v), sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return (uint16_t)(sign | (a > 0x7F800000u ? 0x7E00u : 0x7C00u));  // NaN, infinity
    if (a >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                                // rounds to 2^16 or beyond
    if (a < 0x33000000u) return (uint16_t)sign;                                             // at most 2^-25: to zero
    const int e = (int)(a >> 23) - 127;
    const uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
    const int shift = e >= -14 ? 13 : 13 + (-14 - e);  // (subnormal results lose -14 - e more bits)
    uint32_t q = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (q & 1u))) ++q;
    // normal: q holds the implicit bit at 2^10, so adding (e + 14) << 10 gives exponent field e + 15 (a carry out of the
    // mantissa lands in the exponent, as it should); subnormal: q is the field itself (a carry makes the least normal)
    return (uint16_t)(sign | (e >= -14 ? ((uint32_t)(e + 14) << 10) + q : q));
#else
    return __builtin_bit_cast(uint16_t, (_Float16)v);
#endif
}

// the address of element `offset` of a posterior array (a read's first element), still typed as float *
__device__ __forceinline__ const float *post_at(const float *base, int64_t offset, int dtype) {
    return reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + offset * (dtype == kF32 ? 4 : 2));
}

// element `idx` of a posterior array of type `dtype` (wave-uniform: a scalar branch), as binary32
__device__ __forceinline__ float load_post(const float *base, int64_t idx, int dtype) {
    if (dtype == kF32) return base[idx];
    const uint16_t h = reinterpret_cast<const uint16_t *>(base)[idx];
    return dtype == kF16 ? f16_bits_to_f32(h) : bf16_bits_to_f32(h);
}

// The float at a device address held as an integer (a lane's running address into the posteriors).  A GLOBAL load: through a
// generic pointer it is a flat load, which counts on the LDS counter as well and turns every LDS wait behind it into a full one.
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: plain C++)
#define FCD_GLOBAL_F32(addr) (*reinterpret_cast<const float *>(addr))
#else
#define FCD_GLOBAL_F32(addr) (*(const __attribute__((address_space(1))) float *)(addr))
#endif

// Sort key for the prune step: descending probability, ties -> ascending node index
// (src/search.rs:245 stable sort by node followed by :262-269 sort by probability; see
// SURVEY.md 8a A4).  Larger key == earlier in the beam.  prob must not be NaN.
// (p: the probability with -0.0 already taken to +0.0, prob + 0.0f)
__device__ __forceinline__ uint64_t make_key_canonical(float p, int node) {
    uint32_t u = __float_as_uint(p);
    u ^= (u & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u;  // total order on non-NaN floats
    uint32_t lo = 0x7FFFFFFFu - (uint32_t)node;           // node >= -1; smaller node -> larger lo
    return ((uint64_t)u << 32) | lo;
}
__device__ __forceinline__ uint64_t make_key(float prob, int node) {
    return make_key_canonical(prob + 0.0f, node);  // -0.0 -> +0.0 so that equal floats give equal keys
}

// Loads that must observe this wave's own earlier global stores made from other lanes:
// served from L2 (sc1), bypassing the per-CU L1 (MI355X_MICROARCH.md, visibility table).
__device__ __forceinline__ int32_t load_i32_l2(const int32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Exact-rank building block: r_j += (k_j > key) for four comparands at once.  The compiler's own code for
// `rank += (k > key)` funnels every compare through VCC (v_cmp -> s_nop -> v_cndmask / v_addc), one long
// dependent chain; here the four compares land in four SGPR pairs and feed four independent accumulators,
// so consecutive instructions never wait on each other (each consumer sits three instructions behind its
// producer, which also covers the VALU-writes-SGPR -> VALU-reads-it wait states).
// (tests/hipemu predefines FCD_RANK4 in plain C++.)
#ifndef FCD_RANK4
#define FCD_RANK4(key, ka, kb, kc, kd, r0, r1, r2, r3)                                         \
    do {                                                                                       \
        uint64_t m0__, m1__, m2__, m3__;                                                       \
        asm("v_cmp_gt_u64_e64 %4, %9, %8\n\t"                                                  \
            "v_cmp_gt_u64_e64 %5, %10, %8\n\t"                                                 \
            "v_cmp_gt_u64_e64 %6, %11, %8\n\t"                                                 \
            "v_cmp_gt_u64_e64 %7, %12, %8\n\t"                                                 \
            "v_addc_co_u32_e64 %0, vcc, 0, %0, %4\n\t"                                         \
            "v_addc_co_u32_e64 %1, vcc, 0, %1, %5\n\t"                                         \
            "v_addc_co_u32_e64 %2, vcc, 0, %2, %6\n\t"                                         \
            "v_addc_co_u32_e64 %3, vcc, 0, %3, %7"                                              \
            : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "=&s"(m0__), "=&s"(m1__), "=&s"(m2__), "=&s"(m3__) \
            : "v"(key), "v"(ka), "v"(kb), "v"(kc), "v"(kd)                                     \
            : "vcc");                                                                          \
    } while (0)
#endif

// First block of a rank: the four accumulators START here (r_j = (k_j > key)), read off a shared zero register
// instead of being cleared one by one.
#ifndef FCD_RANK4_FIRST
#define FCD_RANK4_FIRST(key, ka, kb, kc, kd, r0, r1, r2, r3)                                   \
    do {                                                                                       \
        uint64_t m0__, m1__, m2__, m3__;                                                       \
        const int zero__ = 0;                                                                  \
        asm("v_cmp_gt_u64_e64 %4, %9, %8\n\t"                                                  \
            "v_cmp_gt_u64_e64 %5, %10, %8\n\t"                                                 \
            "v_cmp_gt_u64_e64 %6, %11, %8\n\t"                                                 \
            "v_cmp_gt_u64_e64 %7, %12, %8\n\t"                                                 \
            "v_addc_co_u32_e64 %0, vcc, 0, %13, %4\n\t"                                        \
            "v_addc_co_u32_e64 %1, vcc, 0, %13, %5\n\t"                                        \
            "v_addc_co_u32_e64 %2, vcc, 0, %13, %6\n\t"                                        \
            "v_addc_co_u32_e64 %3, vcc, 0, %13, %7"                                             \
            : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&s"(m0__), "=&s"(m1__), "=&s"(m2__), "=&s"(m3__) \
            : "v"(key), "v"(ka), "v"(kb), "v"(kc), "v"(kd), "v"(zero__)                        \
            : "vcc");                                                                          \
    } while (0)
#endif

// The same two blocks on 32-bit words: r_j += (w_j > word).  The two-reads-per-wavefront kernels rank on the probability
// word of the key alone (beam_wave_step.inc, R32) -- half the comparand bytes, and the node word only where two kept
// candidates share a probability.
// ..._ONE: all four compares feed ONE accumulator (the headline family, whose step is bound by the number of vector
// instructions: four chains end in three adds, one chain in none; a consumer still sits four instructions behind its
// producer, and with six wavefronts per SIMD the chain's own latency is covered by the other wavefronts).
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: plain C++)
#define FCD_RANK4_32_ONE(word, wa, wb, wc, wd, r) \
    do { (r) += ((wa) > (word)) + ((wb) > (word)) + ((wc) > (word)) + ((wd) > (word)); } while (0)
#define FCD_RANK4_32_ONE_FIRST(word, wa, wb, wc, wd, r) \
    do { (r) = ((wa) > (word)) + ((wb) > (word)) + ((wc) > (word)) + ((wd) > (word)); } while (0)
#define FCD_RANK4_32(word, wa, wb, wc, wd, r0, r1, r2, r3) \
    do { (r0) += (wa) > (word); (r1) += (wb) > (word); (r2) += (wc) > (word); (r3) += (wd) > (word); } while (0)
#define FCD_RANK4_32_FIRST(word, wa, wb, wc, wd, r0, r1, r2, r3) \
    do { (r0) = (wa) > (word); (r1) = (wb) > (word); (r2) = (wc) > (word); (r3) = (wd) > (word); } while (0)
#else
#define FCD_RANK4_32(word, wa, wb, wc, wd, r0, r1, r2, r3)                                     \
    do {                                                                                       \
        uint64_t m0__, m1__, m2__, m3__;                                                       \
        asm("v_cmp_gt_u32_e64 %4, %9, %8\n\t"                                                  \
            "v_cmp_gt_u32_e64 %5, %10, %8\n\t"                                                 \
            "v_cmp_gt_u32_e64 %6, %11, %8\n\t"                                                 \
            "v_cmp_gt_u32_e64 %7, %12, %8\n\t"                                                 \
            "v_addc_co_u32_e64 %0, vcc, 0, %0, %4\n\t"                                         \
            "v_addc_co_u32_e64 %1, vcc, 0, %1, %5\n\t"                                         \
            "v_addc_co_u32_e64 %2, vcc, 0, %2, %6\n\t"                                         \
            "v_addc_co_u32_e64 %3, vcc, 0, %3, %7"                                              \
            : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "=&s"(m0__), "=&s"(m1__), "=&s"(m2__), "=&s"(m3__) \
            : "v"(word), "v"(wa), "v"(wb), "v"(wc), "v"(wd)                                    \
            : "vcc");                                                                          \
    } while (0)
#define FCD_RANK4_32_FIRST(word, wa, wb, wc, wd, r0, r1, r2, r3)                               \
    do {                                                                                       \
        uint64_t m0__, m1__, m2__, m3__;                                                       \
        const int zero__ = 0;                                                                  \
        asm("v_cmp_gt_u32_e64 %4, %9, %8\n\t"                                                  \
            "v_cmp_gt_u32_e64 %5, %10, %8\n\t"                                                 \
            "v_cmp_gt_u32_e64 %6, %11, %8\n\t"                                                 \
            "v_cmp_gt_u32_e64 %7, %12, %8\n\t"                                                 \
            "v_addc_co_u32_e64 %0, vcc, 0, %13, %4\n\t"                                        \
            "v_addc_co_u32_e64 %1, vcc, 0, %13, %5\n\t"                                        \
            "v_addc_co_u32_e64 %2, vcc, 0, %13, %6\n\t"                                        \
            "v_addc_co_u32_e64 %3, vcc, 0, %13, %7"                                             \
            : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&s"(m0__), "=&s"(m1__), "=&s"(m2__), "=&s"(m3__) \
            : "v"(word), "v"(wa), "v"(wb), "v"(wc), "v"(wd), "v"(zero__)                       \
            : "vcc");                                                                          \
    } while (0)
#define FCD_RANK4_32_ONE(word, wa, wb, wc, wd, r)                                              \
    do {                                                                                       \
        uint64_t m0__, m1__, m2__, m3__;                                                       \
        asm("v_cmp_gt_u32_e64 %1, %6, %5\n\t"                                                  \
            "v_cmp_gt_u32_e64 %2, %7, %5\n\t"                                                  \
            "v_cmp_gt_u32_e64 %3, %8, %5\n\t"                                                  \
            "v_cmp_gt_u32_e64 %4, %9, %5\n\t"                                                  \
            "v_addc_co_u32_e64 %0, vcc, 0, %0, %1\n\t"                                         \
            "v_addc_co_u32_e64 %0, vcc, 0, %0, %2\n\t"                                         \
            "v_addc_co_u32_e64 %0, vcc, 0, %0, %3\n\t"                                         \
            "v_addc_co_u32_e64 %0, vcc, 0, %0, %4"                                              \
            : "+v"(r), "=&s"(m0__), "=&s"(m1__), "=&s"(m2__), "=&s"(m3__)                      \
            : "v"(word), "v"(wa), "v"(wb), "v"(wc), "v"(wd)                                    \
            : "vcc");                                                                          \
    } while (0)
#define FCD_RANK4_32_ONE_FIRST(word, wa, wb, wc, wd, r)                                        \
    do {                                                                                       \
        uint64_t m0__, m1__, m2__, m3__;                                                       \
        const int zero__ = 0;                                                                  \
        asm("v_cmp_gt_u32_e64 %1, %6, %5\n\t"                                                  \
            "v_cmp_gt_u32_e64 %2, %7, %5\n\t"                                                  \
            "v_cmp_gt_u32_e64 %3, %8, %5\n\t"                                                  \
            "v_cmp_gt_u32_e64 %4, %9, %5\n\t"                                                  \
            "v_addc_co_u32_e64 %0, vcc, 0, %10, %1\n\t"                                        \
            "v_addc_co_u32_e64 %0, vcc, 0, %0, %2\n\t"                                         \
            "v_addc_co_u32_e64 %0, vcc, 0, %0, %3\n\t"                                         \
            "v_addc_co_u32_e64 %0, vcc, 0, %0, %4"                                              \
            : "=&v"(r), "=&s"(m0__), "=&s"(m1__), "=&s"(m2__), "=&s"(m3__)                     \
            : "v"(word), "v"(wa), "v"(wb), "v"(wc), "v"(wd), "v"(zero__)                       \
            : "vcc");                                                                          \
    } while (0)
#endif

// The same count as FCD_RANK4_32_ONE in the cheapest instruction class (the KEYED form of r12 - r16 first; the form the kernel
// runs, FCD_RANKP4 on raw words, is stated against it below) (tools/microbench/issue_cost.hip,
// profiles/r12a_issue_cost.txt: at six wavefronts per SIMD a compare into a scalar register pair and the add that reads it
// as its carry hold the SIMD for 4.9 cycles each, v_fma_f32 and v_add_f32 for 2.6 - 2.8).  The word of a non-negative probability
// p is bits(p) | 0x80000000: read as a float it is -p, an empty slot's word 0 is +0.0.  With A = as_float(own word) * 2^100,
// t = clamp(fma(as_float(w), -2^100, A)) = clamp((p_w - p_own) * 2^100) is exactly 1 where w > own and exactly 0 elsewhere
// WHILE every candidate word of the half is that of +0 or of a finite p in [2^-76, 2^27]: the smallest gap there is an ulp of 2^-76,
// 2^-99, so a positive difference scales to >= 2 and nothing overflows, is subnormal or a NaN; an empty slot gives A <= 0.
// The sum of the 25 t's is then the rank, an integer below 2^24.  fcd_rankf_outside() is the guard: a lane whose own word
// leaves that range sends the step to the exact recount (beam_wave_step.inc, m_clash).  Outside it t is still in [0, 1]
// (the clamp takes a NaN to 0), so the rank of a guarded step's first pass stays within the survivor table.  A candidate
// of probability exactly 0 (word 0x80000000, -0.0: it differs from every positive p by at least 2^-76) is inside -- a slot
// whose label probability is 0 and whose blank falls under the threshold leaves one, on ordinary
// rows too.  (A lane without a candidate holds word 0 and is taken out of the vote by the mask of valid candidates.)
constexpr uint32_t kRankfLo = 0x80000000u | (uint32_t)(127 - 76) << 23;  // word of 2^-76
constexpr uint32_t kRankfHi = 0x80000000u | (uint32_t)(127 + 27) << 23;  // word of 2^27
__device__ __forceinline__ float fcd_rankf_own(uint32_t word) { return __uint_as_float(word) * 0x1p100f; }
// The count on RAW words (the headline family's table since r17: bits(p + 0.0f) of a candidate, 0 otherwise).  Own term
// A = as_float(word) * -2^100, comparand term t = clamp(fma(as_float(w), +2^100, A)) = clamp((p_w - p_own) * 2^100): for
// every p >= 0 the very floats the keyed form multiplies out (its word read as a float is -p, its two factors have the
// opposite signs), so everything said above holds word for word, and:
//  - a lane without a candidate holds word 0, A = -0.0: its count is a sum of 25 values in [0, 1] like any other, and nobody
//    reads it (m_val);
//  - an empty slot and a candidate of probability 0 both hold word 0 (keyed: 0 and 0x80000000, +0.0 and -0.0 as floats):
//    neither is "greater" than anything, t = clamp(0 * 2^100 + A) with A <= 0 -- the same outcome as the keyed pair;
//  - the guard is fed A = -p * 2^100 for EVERY p now, not only for p >= 0, and fcd_rankf_outside_a / _m still say of p what
//    fcd_rankf_outside() says of p's keyed word, for all 2^32 patterns (tests/test_headline_rawword_emu.py walks them):
//    a negative p (-0.0 is not one: its word is that of +0.0, and the third vote, p != 0, takes it out) gives A > 0 and the second vote
//    fires; a NaN of either sign gives a NaN A and the first vote fires; +inf, p > 2^27 and 0 < p < 2^-76 give the A they
//    gave.  Raw order and keyed order differ exactly on negative words, and a step that holds one is recounted on keyed tables.
__device__ __forceinline__ float fcd_rankp_own(uint32_t raw) { return __uint_as_float(raw) * -0x1p100f; }
__device__ __forceinline__ bool fcd_rankf_outside(uint32_t word) {
    return word - kRankfLo > kRankfHi - kRankfLo && word != 0x80000000u;
}
// The same predicate as a wave-wide vote, on what the step holds anyway -- the candidate's probability p (make_key: its
// word is that of p + 0.0) and A = fcd_rankf_own(word) -- as three votes on bare compares joined in scalar registers, no
// arithmetic.  A = -p * 2^100 exactly for p >= 0 (a subnormal p scales to a normal A, p >= 2^28 to -inf), so
//   word > kRankfHi (p > 2^27, +inf, a NaN of positive sign)         <=>  A < -2^127, -inf or a NaN:  !(A >= -2^127);
//   word < kRankfLo with bit 31 set (0 <= p < 2^-76)                  <=>  -2^24 < A <= -0.0;
//   word with bit 31 clear (p < 0, a NaN of negative sign)             =>  A >= +0.0 (its word read as a float is positive):
// the second vote, A > -2^24, takes both of the last two and with them the word of +0, which the third, p != 0 (true of a
// NaN), takes out again.  For every one of the 2^32 values of p it says what fcd_rankf_outside() says of p's word
// (tests/test_headline_votes_emu.py walks them all; every word but 0x7FFFFFFF, which no p makes, is among them).  The two
// bounds are parameters: the kernel keeps them in scalar registers across its time loop (FCD_OPAQUE_S) instead of
// rebuilding two literals in every step.
constexpr float kRankfALo = -0x1p24f;   // A of p = 2^-76
constexpr float kRankfAHi = -0x1p127f;  // A of p = 2^27
__device__ __forceinline__ bool fcd_rankf_outside_a(float p, float a, float a_lo, float a_hi) {  // (one lane)
    return !(a >= a_hi) || (a > a_lo && p != 0.0f);
}
__device__ __forceinline__ uint64_t fcd_rankf_outside_m(float p, float a, float a_lo, float a_hi) {
    return ballot(!(a >= a_hi)) | (ballot(a > a_lo) & ballot(p != 0.0f));
}
// Makes a wave-uniform value opaque to the optimiser and pins it in a scalar register: a constant the time loop reads in
// every step stays there instead of being rebuilt from a literal.
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: plain C++)
#define FCD_OPAQUE_S(x) ((void)(x))
#else
#define FCD_OPAQUE_S(x) asm volatile("" : "+s"(x))
#endif
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: plain C++)
static inline float fcd_rankp_t(float a, uint32_t w) {
    const float t = fmaf(__uint_as_float(w), 0x1p100f, a);
    return t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;  // v_fma_f32 ... clamp: [0, 1], a NaN -> 0
}
#define FCD_RANKP4(a, wa, wb, wc, wd, acc) \
    do { (acc) += fcd_rankp_t(a, wa); (acc) += fcd_rankp_t(a, wb); (acc) += fcd_rankp_t(a, wc); (acc) += fcd_rankp_t(a, wd); } while (0)
#define FCD_RANKP4_FIRST(a, wa, wb, wc, wd, acc) \
    do { (acc) = fcd_rankp_t(a, wa) + fcd_rankp_t(a, wb); (acc) += fcd_rankp_t(a, wc); (acc) += fcd_rankp_t(a, wd); } while (0)
#define FCD_RANKP1(a, w, acc) do { (acc) += fcd_rankp_t(a, w); } while (0)
#else
#define FCD_RANKP4(a, wa, wb, wc, wd, acc)                                                     \
    do {                                                                                       \
        float t0__, t1__, t2__, t3__;                                                          \
        asm("v_fma_f32 %1, %6, %10, %5 clamp\n\t"                                              \
            "v_fma_f32 %2, %7, %10, %5 clamp\n\t"                                              \
            "v_fma_f32 %3, %8, %10, %5 clamp\n\t"                                              \
            "v_fma_f32 %4, %9, %10, %5 clamp\n\t"                                              \
            "v_add_f32 %0, %0, %1\n\t"                                                         \
            "v_add_f32 %0, %0, %2\n\t"                                                         \
            "v_add_f32 %0, %0, %3\n\t"                                                         \
            "v_add_f32 %0, %0, %4"                                                             \
            : "+v"(acc), "=&v"(t0__), "=&v"(t1__), "=&v"(t2__), "=&v"(t3__)                    \
            : "v"(a), "v"(wa), "v"(wb), "v"(wc), "v"(wd), "s"(0x1p100f));                      \
    } while (0)
// (the first block: the accumulator STARTS as the sum of two of its four -- one add fewer, nothing to clear)
#define FCD_RANKP4_FIRST(a, wa, wb, wc, wd, acc)                                               \
    do {                                                                                       \
        float t0__, t1__, t2__, t3__;                                                          \
        asm("v_fma_f32 %1, %6, %10, %5 clamp\n\t"                                              \
            "v_fma_f32 %2, %7, %10, %5 clamp\n\t"                                              \
            "v_fma_f32 %3, %8, %10, %5 clamp\n\t"                                              \
            "v_fma_f32 %4, %9, %10, %5 clamp\n\t"                                              \
            "v_add_f32 %0, %1, %2\n\t"                                                         \
            "v_add_f32 %0, %0, %3\n\t"                                                         \
            "v_add_f32 %0, %0, %4"                                                             \
            : "=&v"(acc), "=&v"(t0__), "=&v"(t1__), "=&v"(t2__), "=&v"(t3__)                   \
            : "v"(a), "v"(wa), "v"(wb), "v"(wc), "v"(wd), "s"(0x1p100f));                      \
    } while (0)
#define FCD_RANKP1(a, w, acc)                                                                  \
    do {                                                                                       \
        float t0__;                                                                            \
        asm("v_fma_f32 %1, %3, %4, %2 clamp\n\t"                                               \
            "v_add_f32 %0, %0, %1"                                                             \
            : "+v"(acc), "=&v"(t0__)                                                           \
            : "v"(a), "v"(w), "s"(0x1p100f));                                                  \
    } while (0)
#endif

// Set bits of a half's word of a wave-wide vote below this lane's place in its half, counted onto `base`: the lower half
// counts in the low word (v_mbcnt_lo), the upper half in the high word (v_mbcnt_hi adds nothing for a lane below 32).
// `low_half` is lane-constant, all ones on a lane below 32 and 0 above: the caller keeps it in a register, and "the low word,
// or 0 for the upper half" is one v_and_b32 with the mask word as its scalar operand instead of a move and a select.
__device__ __forceinline__ int half_prefix_count(uint64_t m, int lane, uint32_t low_half, int base) {
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: plain C++)
    const uint32_t w = lane >= 32 ? (uint32_t)(m >> 32) : (low_half & (uint32_t)m);
    return base + __builtin_popcount(w & ((1u << (lane & 31)) - 1u));
#else
    const uint32_t lo = low_half & (uint32_t)m;
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo(lo, (uint32_t)base));
#endif
}

// A wave-uniform mask (one bit per lane, as ballot() returns it) read as this lane's flag: the scalar register pair IS
// the condition, nothing is computed.
__device__ __forceinline__ bool lane_in(uint64_t m, int lane) {
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: plain C++)
    return ((m >> lane) & 1ull) != 0ull;
#else
    return __builtin_amdgcn_inverse_ballot_w64(m);
#endif
}

// `yes` on the lanes of mask m, `no` elsewhere, as ONE v_cndmask_b32 whose mask is an SGPR pair.  Written out: left to the
// register allocator, a mask that an s_and_b64 has just formed may land in VCC and the select take its VCC form, which
// tools/microbench/issue_cost.hip prices apart from the SGPR-pair form.
__device__ __forceinline__ int select_on_pair(uint64_t m, int lane, int yes, int no) {
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: plain C++)
    return ((m >> lane) & 1ull) != 0ull ? yes : no;
#else
    int r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(no), "v"(yes), "s"(m));
    return r;
#endif
}

// Makes a value opaque to the optimiser and pins it in vector registers (the duplex kernel's coefficient table).
// (tests/hipemu predefines FCD_OPAQUE_V as a no-op.)
#ifndef FCD_OPAQUE_V
#define FCD_OPAQUE_V(x) asm volatile("" : "+v"(x))
#endif

// The same without `volatile`: the value is opaque, but the statement is no barrier -- an `asm volatile` has unmodelled side
// effects, and LDS reads on its two sides are not merged into one wider read.
#ifdef FCD_HIPEMU  // (lockstep emulation, tests/hipemu: plain C++)
#define FCD_OPAQUE_VQ(x) ((void)(x))
#else
#define FCD_OPAQUE_VQ(x) asm("" : "+v"(x))
#endif

// Cycle stamp for the instrumented (PROF) kernel instantiations: reads the shader clock once every input
// the stamped block produced (`dep`) has arrived, and makes `dep` opaque so that nothing consuming it is
// scheduled above the stamp.  (tests/hipemu predefines FCD_STAMP as a no-op: there is no clock to read.)
#ifndef FCD_STAMP
#define FCD_STAMP(t64, dep) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t64), "+v"(dep) : : "memory")
#endif

// ---- f32 with an unbounded exponent: what the lattice walks (ctc_lattice.h, crf_lattice.h) and the CRF Viterbi search
// (crf_viterbi.hip) share.  A row's cells are f32 values times one power of two per row; the row's largest exponent is reduced
// as an integer and every cell rescaled exactly.
constexpr int kTarget = 120;          // the row maximum is kept in [2^119, 2^120): three of them sum below 2^127
constexpr int kNoExp = -(1 << 24);    // "exponent" of a cell that takes no part in the row maximum (0, inf, NaN)

__device__ __forceinline__ int finite_exp(float u) {  // exponent of a positive finite value, kNoExp for anything else
    int e;
    (void)frexpf(u, &e);
    return (u > 0.0f && u - u == 0.0f) ? e : kNoExp;
}

__device__ __forceinline__ int wave_imax(int x) {
    int t = x;
#define FCD_DPP_IMAX(CTRL, RM) t = max(t, __builtin_amdgcn_update_dpp(t, t, CTRL, RM, 0xf, false));
    FCD_DPP_IMAX(0x111, 0xf)  // row_shr:1
    FCD_DPP_IMAX(0x112, 0xf)  // row_shr:2
    FCD_DPP_IMAX(0x114, 0xf)  // row_shr:4
    FCD_DPP_IMAX(0x118, 0xf)  // row_shr:8   -> lane 15 of every row holds the row's maximum
    FCD_DPP_IMAX(0x142, 0xa)  // row_bcast:15 into rows 1 and 3
    FCD_DPP_IMAX(0x143, 0xc)  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the maximum
#undef FCD_DPP_IMAX
    return __builtin_amdgcn_readlane(t, 63);
}

// the sum of a non-negative value over the wavefront, the same in every lane (wave_imax's network with + for max)
__device__ __forceinline__ float wave_fsum(float x) {
    float t = x;
#define FCD_DPP_FSUM(CTRL, RM) t = t + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), CTRL, RM, 0xf, false));
    FCD_DPP_FSUM(0x111, 0xf)  // row_shr:1
    FCD_DPP_FSUM(0x112, 0xf)  // row_shr:2
    FCD_DPP_FSUM(0x114, 0xf)  // row_shr:4
    FCD_DPP_FSUM(0x118, 0xf)  // row_shr:8   -> lane 15 of every row holds the row's sum
    FCD_DPP_FSUM(0x142, 0xa)  // row_bcast:15 into rows 1 and 3
    FCD_DPP_FSUM(0x143, 0xc)  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the sum
#undef FCD_DPP_FSUM
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), 63));
}

__device__ __forceinline__ void crf_split(float v, float *m, int *e) {
    int ex = 0;
    float mm = v;
    if (v - v == 0.0f) mm = frexpf(v, &ex);  // (finite; an infinity or a NaN stays what it is, exponent 0)
    *m = mm;
    *e = ex;
}

__device__ __forceinline__ float wave_fmax(float x) {  // of values that are not NaN: through the order-preserving integer
    int b = __float_as_int(x);
    b ^= (b >> 31) & 0x7fffffff;
    b = wave_imax(b);
    b ^= (b >> 31) & 0x7fffffff;
    return __int_as_float(b);
}

// ---- what the one-wavefront-per-read CRF walks share (viterbi.hip's crf_greedy_kernel, crf_viterbi.hip, crf_transitions.hip)
constexpr int kVitMaxN = 9;  // labels of a state that the Viterbi, transition and marginal walks hold in registers

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

// rows of read r: the batch's T, clamped by the read's own length where the batch has lengths
__device__ __forceinline__ int64_t read_rows(int64_t T, const int64_t *lengths, int64_t r) {
    if (lengths) {
        int64_t t = lengths[r];
        T = t < 0 ? 0 : (t < T ? t : T);
    }
    return T;
}

// init_state.argmax() (src/search.rs:399): the first maximum of an init row; *bad: the row is empty or holds a NaN (the
// reference panics)
__device__ __forceinline__ int init_first_max(const float *init, int64_t n_init, bool *bad_out) {
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
    *bad_out = bad;
    return state;
}

}  // namespace fcd
