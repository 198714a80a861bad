// tools/microbench/issue_cost.hip -- what one wave64 instruction of each class costs a SIMD when 1, 2, 4, 6, 7 or 8
// wavefronts share it and every CU is filled: cycles per instruction per SIMD = elapsed cycles / (wavefronts per SIMD x
// instructions per wavefront).  branchlat.hip and f64lat.hip time a lone wavefront; the headline beam step
// (csrc/beam_wave_step.inc) runs at six, and which class its rank count is written in depends on this table.
// Every stream is a bounded loop of inline-asm instructions of ONE class, as four independent chains (ind4, the arrangement
// of FCD_RANK4) and as one dependent chain (dep).  The last rows are whole rank counts on 25 comparands held in registers:
// the present FCD_RANK4_32_ONE form and its exact equivalents in other classes.
// A workgroup is four wavefronts, one per SIMD; a dummy dynamic LDS array lets exactly W workgroups share a CU.
// The only store is one word per wavefront (its s_memtime interval).  HIP events around the launch give the wall time of the
// same work, and with one wavefront per SIMD the shader clock.
// About 700 launches (two per class, form and W) of 50 us to 2.4 ms: two thirds of a second of GPU time in all.
//   hipcc --offload-arch=gfx950 -O3 issue_cost.hip -o issue_cost      ./issue_cost [trips, default 1024]
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>

#define CHECK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e__)); exit(1); } } while (0)

// operands of every stream: %0-%3 four VGPR accumulators, %4-%7 four SGPR pairs, %8-%11 four 32-bit SGPRs,
// %12 %13 two VGPR inputs, %14 %15 two 64-bit VGPR inputs
#define OPS : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+s"(m0), "+s"(m1), "+s"(m2), "+s"(m3), "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) \
            : "v"(y0), "v"(y1), "v"(z0), "v"(z1) : "vcc", "scc"
// M(d, m, s): the instruction(s) of one chain -- VGPR accumulator %d, SGPR pair %m, SGPR %s
#define IND4(M) M(0, 4, 8) M(1, 5, 9) M(2, 6, 10) M(3, 7, 11)
#define IND16(M) IND4(M) IND4(M) IND4(M) IND4(M)
#define DEP4(M) M(0, 4, 8) M(0, 4, 8) M(0, 4, 8) M(0, 4, 8)
#define DEP16(M) DEP4(M) DEP4(M) DEP4(M) DEP4(M)

#define I_FMA(d, m, s)       "v_fma_f32 %" #d ", %" #d ", %12, %13\n\t"
#define I_FMA_CLAMP(d, m, s) "v_fma_f32 %" #d ", %" #d ", %12, %13 clamp\n\t"
#define I_ADD_F32(d, m, s)   "v_add_f32 %" #d ", %12, %" #d "\n\t"
#define I_MUL_F32(d, m, s)   "v_mul_f32 %" #d ", %12, %" #d "\n\t"
#define I_CVT_U32(d, m, s)   "v_cvt_u32_f32 %" #d ", %" #d "\n\t"
#define I_ADD_U32(d, m, s)   "v_add_u32 %" #d ", %12, %" #d "\n\t"
#define I_SUB_U32(d, m, s)   "v_sub_u32 %" #d ", %12, %" #d "\n\t"
#define I_AND(d, m, s)       "v_and_b32 %" #d ", %12, %" #d "\n\t"
#define I_LSHL(d, m, s)      "v_lshlrev_b32 %" #d ", 1, %" #d "\n\t"
#define I_ALIGNBIT(d, m, s)  "v_alignbit_b32 %" #d ", %" #d ", %12, 31\n\t"
#define I_BFE(d, m, s)       "v_bfe_u32 %" #d ", %" #d ", 1, 31\n\t"
#define I_LSHL_ADD(d, m, s)  "v_lshl_add_u32 %" #d ", %" #d ", 1, %12\n\t"
#define I_AND_OR(d, m, s)    "v_and_or_b32 %" #d ", %" #d ", %12, %13\n\t"
#define I_BCNT(d, m, s)      "v_bcnt_u32_b32 %" #d ", %12, %" #d "\n\t"
#define I_MIN3(d, m, s)      "v_min3_u32 %" #d ", %" #d ", %12, %13\n\t"
#define I_CMP_VCC(d, m, s)   "v_cmp_gt_u32 vcc, %12, %" #d "\n\t"
#define I_CMP_U32(d, m, s)   "v_cmp_gt_u32_e64 %" #m ", %12, %" #d "\n\t"
#define I_CMP_F32(d, m, s)   "v_cmp_gt_f32_e64 %" #m ", %12, %" #d "\n\t"
#define I_CMP_U64(d, m, s)   "v_cmp_gt_u64_e64 %" #m ", %14, %15\n\t"
#define I_ADDC(d, m, s)      "v_addc_co_u32_e64 %" #d ", vcc, 0, %" #d ", %" #m "\n\t"
#define I_CND_VCC(d, m, s)   "v_cndmask_b32_e32 %" #d ", %12, %" #d ", vcc\n\t"
#define I_CND_SGPR(d, m, s)  "v_cndmask_b32_e64 %" #d ", %12, %" #d ", %" #m "\n\t"
#define I_MBCNT(d, m, s)     "v_mbcnt_lo_u32_b32 %" #d ", %12, %" #d "\n\tv_mbcnt_hi_u32_b32 %" #d ", %13, %" #d "\n\t"  // 2
#define I_READLANE(d, m, s)  "v_readlane_b32 %" #s ", %" #d ", 3\n\t"
#define I_DPP(d, m, s)       "v_mov_b32_dpp %" #d ", %" #d " row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
#define I_SALU(d, m, s)      "s_and_b64 %" #m ", %" #m ", exec\n\ts_xor_b64 %" #m ", %" #m ", exec\n\t"  // 2
#define I_SALU_VALU(d, m, s) "s_and_b64 %" #m ", %" #m ", exec\n\tv_add_u32 %" #d ", %12, %" #d "\n\t" \
                             "s_xor_b64 %" #m ", %" #m ", exec\n\tv_add_u32 %" #d ", %13, %" #d "\n\t"  // 2 + 2
// r14: the classes the vote, guard and child-fate forms of the headline step rest on
#define I_MIN_U32(d, m, s)   "v_min_u32 %" #d ", %12, %" #d "\n\t"
#define I_MAX_U32(d, m, s)   "v_max_u32 %" #d ", %12, %" #d "\n\t"
#define I_CMP_CLASS(d, m, s) "v_cmp_class_f32_e64 %" #m ", %" #d ", 32\n\t"
#define I_BFI(d, m, s)       "v_bfi_b32 %" #d ", %" #d ", %12, %13\n\t"
#define I_BCNT1_CSEL(d, m, s) "s_bcnt1_i32_b64 %" #s ", %" #m "\n\tv_add_u32 %" #d ", %12, %" #d "\n\t" \
                              "s_cselect_b32 %" #s ", %" #s ", 0\n\tv_add_u32 %" #d ", %13, %" #d "\n\t"  // 2 + 2
// an exec region around one vector instruction whose s_cbranch_execz is not taken (the mask is exec itself)
#define I_SAVEEXEC(d, m, s)  "s_and_saveexec_b64 %" #m ", exec\n\ts_cbranch_execz 1f\n\tv_add_u32 %" #d ", %12, %" #d "\n\t" \
                             "1:\n\ts_or_b64 exec, exec, %" #m "\n\t"
// r15: forms on the headline step's hot path that the rows above do not price.  The VCC select is priced three ways: behind a
// vector compare that writes VCC, behind a scalar instruction that writes VCC (both as the kernel has them; the plain row above
// never writes VCC inside its loop), and in the e64 encoding with VCC spelled as its pair operand.
#define I_CMP_CND_VCC(d, m, s)  "v_cmp_gt_u32 vcc, %12, %" #d "\n\tv_cndmask_b32_e32 %" #d ", %12, %" #d ", vcc\n\t"  // 2
#define I_SAND_CND_VCC(d, m, s) "s_and_b64 vcc, %" #m ", exec\n\tv_cndmask_b32_e32 %" #d ", %12, %" #d ", vcc\n\t"  // 2
#define I_CMP_CND_SGPR(d, m, s) "v_cmp_gt_u32_e64 %" #m ", %12, %" #d "\n\tv_cndmask_b32_e64 %" #d ", %12, %" #d ", %" #m "\n\t"  // 2 (the pair to set the VCC pair against)
#define I_CND_E64_VCC(d, m, s)  "v_cndmask_b32_e64 %" #d ", %12, %" #d ", vcc\n\t"
#define I_MUL_LO(d, m, s)       "v_mul_lo_u32 %" #d ", %12, %" #d "\n\t"
#define I_DIV_SCALE(d, m, s)    "v_div_scale_f32 %" #d ", vcc, %12, %12, %" #d "\n\t"
#define I_RCP(d, m, s)          "v_rcp_f32 %" #d ", %" #d "\n\t"
#define I_DIV_FMAS(d, m, s)     "v_div_fmas_f32 %" #d ", %" #d ", %12, %13\n\t"
#define I_DIV_FIXUP(d, m, s)    "v_div_fixup_f32 %" #d ", %" #d ", %12, %13\n\t"
// r18: the scalar forms that replace wave-uniform vector work in the headline step (a half's candidate count, beam width and
// group mask; "own candidate dropped" as a multiple of the kept own-lane bits), each 1:1 beside a v_add_u32 stream as the rows
// of s_and/s_xor and s_bcnt1/s_cselect above; v_and_b32 with the mask word as its scalar operand (half_prefix_count); and the
// LDS look-up the multiple replaces -- ds_bpermute_b32, its wait and the compare that reads it -- against the three scalar
// instructions, both beside two v_add_u32.
#define I_SMUL_VALU(d, m, s) "s_mul_i32 %" #s ", %" #s ", 30\n\tv_add_u32 %" #d ", %12, %" #d "\n\t" \
                             "s_mul_i32 %" #s ", %" #s ", 30\n\tv_add_u32 %" #d ", %13, %" #d "\n\t"  // 2 + 2
#define I_SBFM_VALU(d, m, s) "s_bfm_b32 %" #s ", %" #s ", 0\n\tv_add_u32 %" #d ", %12, %" #d "\n\t" \
                             "s_bfm_b32 %" #s ", %" #s ", 0\n\tv_add_u32 %" #d ", %13, %" #d "\n\t"  // 2 + 2
#define I_SBCNT_MIN_VALU(d, m, s) "s_bcnt1_i32_b32 %" #s ", %" #s "\n\tv_add_u32 %" #d ", %12, %" #d "\n\t" \
                                  "s_min_i32 %" #s ", %" #s ", 5\n\tv_add_u32 %" #d ", %13, %" #d "\n\t"  // 2 + 2
#define I_AND_SGPR(d, m, s)  "v_and_b32 %" #d ", %" #s ", %" #d "\n\t"
#define I_BPERM_CMP(d, m, s) "ds_bpermute_b32 %" #d ", %12, %" #d "\n\tv_add_u32 %" #d ", %12, %" #d "\n\ts_waitcnt lgkmcnt(0)\n\t" \
                             "v_cmp_eq_u32_e64 %" #m ", 0, %" #d "\n\tv_add_u32 %" #d ", %13, %" #d "\n\t"  // (1 LDS + 1 compare) + 2
#define I_SMUL2_ANDN2(d, m, s) "s_mul_i32 %" #s ", %" #s ", 30\n\tv_add_u32 %" #d ", %12, %" #d "\n\ts_mul_i32 %" #s ", %" #s ", 30\n\t" \
                               "s_andn2_b64 %" #m ", exec, %" #m "\n\tv_add_u32 %" #d ", %13, %" #d "\n\t"  // 3 scalar + 2
// a scalar compare and its branch to the next instruction: taken (the compare holds) against not taken
#define I_BR_TAKEN(d, m, s)     "s_cmp_eq_u32 %" #s ", %" #s "\n\ts_cbranch_scc1 1f\n\t1:\n\t"  // 2
#define I_BR_NOT(d, m, s)       "s_cmp_lg_u32 %" #s ", %" #s "\n\ts_cbranch_scc1 1f\n\t1:\n\t"  // 2
// 64-bit forms: %0-%3 four 64-bit VGPR accumulators, %4-%7 four SGPR pairs, %8 %9 two 32-bit VGPR inputs, %10 a 64-bit VGPR input
#define OPS64 : "+v"(w0), "+v"(w1), "+v"(w2), "+v"(w3), "+s"(m0), "+s"(m1), "+s"(m2), "+s"(m3) : "v"(y0), "v"(y1), "v"(z0) : "vcc", "scc"
#define IND4_64(M) M(0, 4) M(1, 5) M(2, 6) M(3, 7)
#define IND16_64(M) IND4_64(M) IND4_64(M) IND4_64(M) IND4_64(M)
#define DEP16_64(M) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4) M(0, 4)
#define J_LSHR_B64_S(d, m)  "v_lshrrev_b64 %" #d ", %8, %" #m "\n\t"   // scalar pair source, as the step has it (no chain through it)
#define J_LSHR_B64_V(d, m)  "v_lshrrev_b64 %" #d ", 1, %" #d "\n\t"
#define J_MOV_B64(d, m)     "v_mov_b64 %" #d ", %" #m "\n\t"
#define J_MAD_U64(d, m)     "v_mad_u64_u32 %" #d ", %" #m ", %8, %9, %" #d "\n\t"
#define J_LSHL_ADD_U64(d, m) "v_lshl_add_u64 %" #d ", %" #d ", 2, %10\n\t"
// the pair the rank count is made of today, consumer four instructions behind its producer
#define I_CMP_ADDC_PAIR "v_cmp_gt_u32_e64 %4, %12, %0\n\tv_cmp_gt_u32_e64 %5, %12, %1\n\tv_cmp_gt_u32_e64 %6, %12, %2\n\tv_cmp_gt_u32_e64 %7, %12, %3\n\t" \
                        "v_addc_co_u32_e64 %0, vcc, 0, %0, %4\n\tv_addc_co_u32_e64 %1, vcc, 0, %1, %5\n\t"                                                   \
                        "v_addc_co_u32_e64 %2, vcc, 0, %2, %6\n\tv_addc_co_u32_e64 %3, vcc, 0, %3, %7\n\t"

enum {
    C_FMA, C_FMA_CLAMP, C_ADD_F32, C_MUL_F32, C_CVT_U32, C_ADD_U32, C_SUB_U32, C_AND, C_LSHL, C_ALIGNBIT, C_BFE, C_LSHL_ADD,
    C_AND_OR, C_BCNT, C_MIN3, C_CMP_VCC, C_CMP_U32, C_CMP_F32, C_CMP_U64, C_ADDC, C_CND_VCC, C_CND_SGPR, C_MBCNT, C_READLANE,
    C_DPP, C_SALU, C_SALU_VALU, C_MIN_U32, C_MAX_U32, C_CMP_CLASS, C_BFI, C_BCNT1_CSEL, C_SAVEEXEC, C_CMP_ADDC, C_FDIV, C_RANK_NOW,
    C_RANK_F, C_RANK_I, C_RANK_S, C_RANK_P,
    C_CMP_CND_VCC, C_SAND_CND_VCC, C_CMP_CND_SGPR, C_CND_E64_VCC, C_MUL_LO, C_DIV_SCALE, C_RCP, C_DIV_FMAS, C_DIV_FIXUP, C_BR_TAKEN, C_BR_NOT,
    C_LSHR_B64_S, C_LSHR_B64_V, C_MOV_B64, C_MAD_U64, C_LSHL_ADD_U64,
    C_SMUL_VALU, C_SBFM_VALU, C_SBCNT_MIN_VALU, C_AND_SGPR, C_BPERM_CMP, C_SMUL2_ANDN2, C_COUNT
};
struct Cls { const char *name; int per_trip_ind, per_trip_dep; const char *unit; };
// instructions (or units) one loop trip issues per wavefront
static const Cls kCls[C_COUNT] = {
    {"v_fma_f32", 16, 16, "inst"}, {"v_fma_f32 clamp", 16, 16, "inst"}, {"v_add_f32", 16, 16, "inst"}, {"v_mul_f32", 16, 16, "inst"},
    {"v_cvt_u32_f32", 16, 16, "inst"}, {"v_add_u32", 16, 16, "inst"}, {"v_sub_u32", 16, 16, "inst"}, {"v_and_b32", 16, 16, "inst"},
    {"v_lshlrev_b32", 16, 16, "inst"}, {"v_alignbit_b32", 16, 16, "inst"}, {"v_bfe_u32", 16, 16, "inst"}, {"v_lshl_add_u32", 16, 16, "inst"},
    {"v_and_or_b32", 16, 16, "inst"}, {"v_bcnt_u32_b32", 16, 16, "inst"}, {"v_min3_u32", 16, 16, "inst"},
    {"v_cmp_gt_u32 -> vcc", 16, 16, "inst"}, {"v_cmp_gt_u32_e64 -> sgpr pair", 16, 16, "inst"}, {"v_cmp_gt_f32_e64 -> sgpr pair", 16, 16, "inst"},
    {"v_cmp_gt_u64_e64 -> sgpr pair", 16, 16, "inst"}, {"v_addc_co_u32_e64 <- sgpr carry", 16, 16, "inst"},
    {"v_cndmask_b32 on vcc", 16, 16, "inst"}, {"v_cndmask_b32_e64 on sgpr pair", 16, 16, "inst"},
    {"v_mbcnt_lo + v_mbcnt_hi", 32, 32, "inst"}, {"v_readlane_b32", 16, 0, "inst"}, {"v_mov_b32 dpp row_shr:1", 16, 0, "inst"},
    {"s_and_b64 + s_xor_b64 alone", 32, 32, "inst"}, {"s_and/s_xor 1:1 with v_add_u32 (per v_add_u32)", 32, 32, "v_add"},
    {"v_min_u32", 16, 16, "inst"}, {"v_max_u32", 16, 16, "inst"}, {"v_cmp_class_f32_e64 -> sgpr pair", 16, 16, "inst"},
    {"v_bfi_b32", 16, 16, "inst"}, {"s_bcnt1_i32_b64/s_cselect_b32 1:1 with v_add_u32 (per v_add_u32)", 32, 32, "v_add"},
    {"saveexec region, execz not taken, around one v_add_u32", 16, 16, "region"},
    {"v_cmp_gt_u32_e64 + v_addc pair (4 chains)", 16, 0, "inst"}, {"f32 IEEE division (compiler's sequence)", 16, 16, "division"},
    {"RANK now: 25 x (v_cmp_e64 + v_addc)", 1, 0, "block"}, {"RANK F: 25 x (v_fma clamp + v_add_f32) + cvt", 1, 0, "block"},
    {"RANK I: 25 x (v_sub + v_alignbit) + bcnt + sub", 1, 0, "block"}, {"RANK S: scalar full adder, 3 cmp + 2 addc + 5 salu", 1, 0, "block"},
    {"RANK P: 12 x (v_pk_fma_f32 clamp + v_pk_add_f32) + 1 + halves + cvt", 1, 0, "block"},
    {"v_cmp_gt_u32 -> vcc + v_cndmask_b32_e32 on vcc (per pair)", 16, 16, "pair"},
    {"s_and_b64 vcc + v_cndmask_b32_e32 on vcc (per pair)", 16, 16, "pair"},
    {"v_cmp_gt_u32_e64 -> sgpr pair + v_cndmask_b32_e64 on it (per pair)", 16, 16, "pair"},
    {"v_cndmask_b32_e64 with vcc as its pair operand", 16, 16, "inst"}, {"v_mul_lo_u32", 16, 16, "inst"},
    {"v_div_scale_f32", 16, 16, "inst"}, {"v_rcp_f32", 16, 16, "inst"}, {"v_div_fmas_f32", 16, 16, "inst"}, {"v_div_fixup_f32", 16, 16, "inst"},
    {"s_cmp + s_cbranch_scc1 taken (per pair)", 16, 0, "pair"}, {"s_cmp + s_cbranch_scc1 not taken (per pair)", 16, 0, "pair"},
    {"v_lshrrev_b64 <- sgpr pair", 16, 0, "inst"}, {"v_lshrrev_b64 <- vgpr pair", 16, 16, "inst"}, {"v_mov_b64 <- sgpr pair", 16, 0, "inst"},
    {"v_mad_u64_u32", 16, 16, "inst"}, {"v_lshl_add_u64", 16, 16, "inst"},
    {"s_mul_i32 by 30 1:1 with v_add_u32 (per v_add_u32)", 32, 32, "v_add"}, {"s_bfm_b32 1:1 with v_add_u32 (per v_add_u32)", 32, 32, "v_add"},
    {"s_bcnt1_i32_b32/s_min_i32 1:1 with v_add_u32 (per v_add_u32)", 32, 32, "v_add"}, {"v_and_b32 <- sgpr operand", 16, 16, "inst"},
    {"ds_bpermute_b32 + wait + v_cmp_eq_u32_e64 beside 2 v_add_u32 (per group)", 16, 0, "group"},
    {"2 s_mul_i32 + s_andn2_b64 beside 2 v_add_u32 (per group)", 16, 0, "group"},
};

#define T0 asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0) : : "memory")
#define T1 asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1) : : "memory")
#define STREAM_CASE(ID, M)                                                                          \
    if (C == ID) {                                                                                  \
        if (!DEP) { for (int i = 0; i < trips; ++i) asm volatile(IND16(M) OPS); }                   \
        else { for (int i = 0; i < trips; ++i) asm volatile(DEP16(M) OPS); }                        \
    }

#define STREAM_CASE64(ID, M)                                                                        \
    if (C == ID) {                                                                                  \
        if (!DEP) { for (int i = 0; i < trips; ++i) asm volatile(IND16_64(M) OPS64); }              \
        else { for (int i = 0; i < trips; ++i) asm volatile(DEP16_64(M) OPS64); }                   \
    }

template <int C, bool DEP>
__global__ __launch_bounds__(256) void k(uint32_t *cyc, int trips, uint32_t a, float fa) {
    extern __shared__ uint32_t dummy_lds[];
    uint64_t t0, t1;
    uint32_t x0 = threadIdx.x + a, x1 = x0 * 3u, x2 = x0 * 5u, x3 = x0 * 7u, y0 = a * 11u + threadIdx.x, y1 = a ^ 0x5555u;
    uint64_t m0 = a, m1 = a + 1, m2 = a + 2, m3 = a + 3;
    uint32_t s0 = a, s1 = a + 1, s2 = a + 2, s3 = a + 3;
    uint64_t z0 = ((uint64_t)x1 << 32) | x0, z1 = ((uint64_t)x3 << 32) | x2;
    if (trips < 0) dummy_lds[threadIdx.x] = a;  // (never: the array only has to exist)
    T0;
    STREAM_CASE(C_FMA, I_FMA) STREAM_CASE(C_FMA_CLAMP, I_FMA_CLAMP) STREAM_CASE(C_ADD_F32, I_ADD_F32) STREAM_CASE(C_MUL_F32, I_MUL_F32)
    STREAM_CASE(C_CVT_U32, I_CVT_U32) STREAM_CASE(C_ADD_U32, I_ADD_U32) STREAM_CASE(C_SUB_U32, I_SUB_U32) STREAM_CASE(C_AND, I_AND)
    STREAM_CASE(C_LSHL, I_LSHL) STREAM_CASE(C_ALIGNBIT, I_ALIGNBIT) STREAM_CASE(C_BFE, I_BFE) STREAM_CASE(C_LSHL_ADD, I_LSHL_ADD)
    STREAM_CASE(C_AND_OR, I_AND_OR) STREAM_CASE(C_BCNT, I_BCNT) STREAM_CASE(C_MIN3, I_MIN3) STREAM_CASE(C_CMP_VCC, I_CMP_VCC)
    STREAM_CASE(C_CMP_U32, I_CMP_U32) STREAM_CASE(C_CMP_F32, I_CMP_F32) STREAM_CASE(C_CMP_U64, I_CMP_U64) STREAM_CASE(C_ADDC, I_ADDC)
    STREAM_CASE(C_CND_VCC, I_CND_VCC) STREAM_CASE(C_CND_SGPR, I_CND_SGPR) STREAM_CASE(C_MBCNT, I_MBCNT) STREAM_CASE(C_READLANE, I_READLANE)
    STREAM_CASE(C_DPP, I_DPP) STREAM_CASE(C_SALU, I_SALU) STREAM_CASE(C_SALU_VALU, I_SALU_VALU)
    STREAM_CASE(C_MIN_U32, I_MIN_U32) STREAM_CASE(C_MAX_U32, I_MAX_U32) STREAM_CASE(C_CMP_CLASS, I_CMP_CLASS) STREAM_CASE(C_BFI, I_BFI)
    STREAM_CASE(C_BCNT1_CSEL, I_BCNT1_CSEL) STREAM_CASE(C_SAVEEXEC, I_SAVEEXEC)
    STREAM_CASE(C_CMP_CND_VCC, I_CMP_CND_VCC) STREAM_CASE(C_SAND_CND_VCC, I_SAND_CND_VCC) STREAM_CASE(C_CMP_CND_SGPR, I_CMP_CND_SGPR)
    STREAM_CASE(C_CND_E64_VCC, I_CND_E64_VCC) STREAM_CASE(C_MUL_LO, I_MUL_LO) STREAM_CASE(C_DIV_SCALE, I_DIV_SCALE) STREAM_CASE(C_RCP, I_RCP)
    STREAM_CASE(C_DIV_FMAS, I_DIV_FMAS) STREAM_CASE(C_DIV_FIXUP, I_DIV_FIXUP) STREAM_CASE(C_BR_TAKEN, I_BR_TAKEN) STREAM_CASE(C_BR_NOT, I_BR_NOT)
    STREAM_CASE(C_SMUL_VALU, I_SMUL_VALU) STREAM_CASE(C_SBFM_VALU, I_SBFM_VALU) STREAM_CASE(C_SBCNT_MIN_VALU, I_SBCNT_MIN_VALU)
    STREAM_CASE(C_AND_SGPR, I_AND_SGPR) STREAM_CASE(C_BPERM_CMP, I_BPERM_CMP) STREAM_CASE(C_SMUL2_ANDN2, I_SMUL2_ANDN2)
    if (C >= C_LSHR_B64_S && C <= C_LSHL_ADD_U64) {
        uint64_t w0 = z0, w1 = z1, w2 = z0 + 5, w3 = z1 + 7;
        STREAM_CASE64(C_LSHR_B64_S, J_LSHR_B64_S) STREAM_CASE64(C_LSHR_B64_V, J_LSHR_B64_V) STREAM_CASE64(C_MOV_B64, J_MOV_B64)
        STREAM_CASE64(C_MAD_U64, J_MAD_U64) STREAM_CASE64(C_LSHL_ADD_U64, J_LSHL_ADD_U64)
        asm volatile("" : : "v"(w0), "v"(w1), "v"(w2), "v"(w3));
    }
    if (C == C_CMP_ADDC) {
        for (int i = 0; i < trips; ++i) asm volatile(I_CMP_ADDC_PAIR I_CMP_ADDC_PAIR OPS);
    }
    if (C == C_FDIV) {
        float f0 = fa + (float)threadIdx.x, f1 = f0 + 1.0f, f2 = f0 + 2.0f, f3 = f0 + 3.0f;
        for (int i = 0; i < trips; ++i) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (!DEP) {
                    f0 = fa / f0; f1 = fa / f1; f2 = fa / f2; f3 = fa / f3;
                    asm volatile("" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3));
                } else {
#pragma unroll
                    for (int v = 0; v < 4; ++v) { f0 = fa / f0; asm volatile("" : "+v"(f0)); }
                }
            }
        }
        asm volatile("" : : "v"(f0), "v"(f1), "v"(f2), "v"(f3));
    }
    if (C >= C_RANK_NOW && C <= C_RANK_P) {
        // 25 comparand words in registers (in the domain of every form: words of positive finite probabilities) and the lane's own
        uint32_t kw[25];
#pragma unroll
        for (int u = 0; u < 25; ++u) { kw[u] = 0xBF000000u + (a + u * 977u + threadIdx.x * 31u) % 4096u; asm volatile("" : "+v"(kw[u])); }
        uint32_t kp = 0xBF000000u + x0 % 4096u, r = 0;
        uint64_t kw2[12];  // RANK P: the same comparands as register pairs
#pragma unroll
        for (int u = 0; u < 12; ++u) { kw2[u] = ((uint64_t)kw[2 * u + 1] << 32) | kw[2 * u]; if (C == C_RANK_P) asm volatile("" : "+v"(kw2[u])); }
        for (int i = 0; i < trips; ++i) {
            asm volatile("" : "+v"(kp));
            if (C == C_RANK_NOW) {  // FCD_RANK4_32_ONE_FIRST, 5 x FCD_RANK4_32_ONE, the 25th: compare into vcc, add with carry
                const uint32_t zero = 0;
#define RANK4_NOW(ACC_IN, wa, wb, wc, wd)                                                                              \
    asm volatile("v_cmp_gt_u32_e64 %1, %6, %5\n\tv_cmp_gt_u32_e64 %2, %7, %5\n\tv_cmp_gt_u32_e64 %3, %8, %5\n\tv_cmp_gt_u32_e64 %4, %9, %5\n\t" \
                 "v_addc_co_u32_e64 %0, vcc, 0, %10, %1\n\tv_addc_co_u32_e64 %0, vcc, 0, %0, %2\n\t"                 \
                 "v_addc_co_u32_e64 %0, vcc, 0, %0, %3\n\tv_addc_co_u32_e64 %0, vcc, 0, %0, %4"                        \
                 : "=&v"(r), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3) : "v"(kp), "v"(wa), "v"(wb), "v"(wc), "v"(wd), "v"(ACC_IN) : "vcc")
                RANK4_NOW(zero, kw[0], kw[1], kw[2], kw[3]);
#pragma unroll
                for (int j = 1; j < 6; ++j) RANK4_NOW(r, kw[4 * j], kw[4 * j + 1], kw[4 * j + 2], kw[4 * j + 3]);
                asm volatile("v_cmp_gt_u32 vcc, %1, %2\n\tv_addc_co_u32_e32 %0, vcc, 0, %0, vcc" : "+v"(r) : "v"(kw[24]), "v"(kp) : "vcc");
            } else if (C == C_RANK_F) {  // t = clamp(fma(w, -2^100, A)) is 1 where w > kp (as floats: -p_w < -p_kp), else 0
                float A, acc = 0.0f;
                const float scale = -0x1p100f;
                asm volatile("v_mul_f32 %0, 0x71800000, %1" : "=v"(A) : "v"(kp));  // A = as_float(kp) * 2^100
#pragma unroll
                for (int u = 0; u < 25; u += 5) {
                    float ta, tb, tc, td, te;
                    asm volatile("v_fma_f32 %1, %7, %12, %6 clamp\n\tv_fma_f32 %2, %8, %12, %6 clamp\n\tv_fma_f32 %3, %9, %12, %6 clamp\n\t"
                                 "v_fma_f32 %4, %10, %12, %6 clamp\n\tv_fma_f32 %5, %11, %12, %6 clamp\n\t"
                                 "v_add_f32 %0, %0, %1\n\tv_add_f32 %0, %0, %2\n\tv_add_f32 %0, %0, %3\n\tv_add_f32 %0, %0, %4\n\tv_add_f32 %0, %0, %5"
                                 : "+v"(acc), "=&v"(ta), "=&v"(tb), "=&v"(tc), "=&v"(td), "=&v"(te)
                                 : "v"(A), "v"(kw[u]), "v"(kw[u + 1]), "v"(kw[u + 2]), "v"(kw[u + 3]), "v"(kw[u + 4]), "v"(scale));
                }
                asm volatile("v_cvt_u32_f32 %0, %1" : "=v"(r) : "v"(acc));
            } else if (C == C_RANK_I) {  // bit 31 of kp - w is (w > kp) while both words are >= 0x80000000
                uint32_t acc = 0;
#pragma unroll
                for (int u = 0; u < 25; u += 5) {
                    uint32_t da, db, dc, dd, de;
                    asm volatile("v_sub_u32 %1, %6, %7\n\tv_sub_u32 %2, %6, %8\n\tv_sub_u32 %3, %6, %9\n\tv_sub_u32 %4, %6, %10\n\tv_sub_u32 %5, %6, %11\n\t"
                                 "v_alignbit_b32 %0, %0, %1, 31\n\tv_alignbit_b32 %0, %0, %2, 31\n\tv_alignbit_b32 %0, %0, %3, 31\n\t"
                                 "v_alignbit_b32 %0, %0, %4, 31\n\tv_alignbit_b32 %0, %0, %5, 31"
                                 : "+v"(acc), "=&v"(da), "=&v"(db), "=&v"(dc), "=&v"(dd), "=&v"(de)
                                 : "v"(kp), "v"(kw[u]), "v"(kw[u + 1]), "v"(kw[u + 2]), "v"(kw[u + 3]), "v"(kw[u + 4]));
                }
                asm volatile("v_bcnt_u32_b32 %0, %1, 0\n\tv_sub_u32 %0, %0, %2" : "=&v"(r) : "v"(acc), "v"(y1));
            } else if (C == C_RANK_P) {  // RANK F two comparands per instruction: packed f32 fma with clamp, packed add, the halves summed
                float A, single, s_lo;
                const float scale = -0x1p100f;
                uint64_t acc2 = 0, A2, sc2;
                asm volatile("v_mul_f32 %0, 0x71800000, %1" : "=v"(A) : "v"(kp));
                A2 = ((uint64_t)__float_as_uint(A) << 32) | __float_as_uint(A);
                sc2 = ((uint64_t)__float_as_uint(scale) << 32) | __float_as_uint(scale);
                asm volatile("" : "+v"(A2), "+s"(sc2));
#pragma unroll
                for (int u = 0; u < 12; u += 4) {
                    uint64_t ta, tb, tc, td;
                    asm volatile("v_pk_fma_f32 %1, %6, %10, %5 clamp\n\tv_pk_fma_f32 %2, %7, %10, %5 clamp\n\t"
                                 "v_pk_fma_f32 %3, %8, %10, %5 clamp\n\tv_pk_fma_f32 %4, %9, %10, %5 clamp\n\t"
                                 "v_pk_add_f32 %0, %0, %1\n\tv_pk_add_f32 %0, %0, %2\n\tv_pk_add_f32 %0, %0, %3\n\tv_pk_add_f32 %0, %0, %4"
                                 : "+v"(acc2), "=&v"(ta), "=&v"(tb), "=&v"(tc), "=&v"(td)
                                 : "v"(A2), "v"(kw2[u]), "v"(kw2[u + 1]), "v"(kw2[u + 2]), "v"(kw2[u + 3]), "s"(sc2));
                }
                asm volatile("v_fma_f32 %0, %3, %4, %2 clamp\n\tv_add_f32 %1, %5, %6\n\tv_add_f32 %1, %1, %0"
                             : "=&v"(single), "=&v"(s_lo)
                             : "v"(A), "v"(kw[24]), "s"(scale), "v"((uint32_t)acc2), "v"((uint32_t)(acc2 >> 32)));
                asm volatile("v_cvt_u32_f32 %0, %1" : "=v"(r) : "v"(s_lo));
            } else {  // C_RANK_S: three compare masks through a scalar full adder into carry-adds of weight 1 and 2
                uint32_t r1 = 0, r2 = 0;
#pragma unroll
                for (int u = 0; u < 24; u += 3) {
                    asm volatile("v_cmp_gt_u32_e64 %2, %6, %5\n\tv_cmp_gt_u32_e64 %3, %7, %5\n\tv_cmp_gt_u32_e64 %4, %8, %5\n\t"
                                 "s_xor_b64 vcc, %2, %3\n\ts_and_b64 %2, %2, %3\n\ts_and_b64 %3, %4, vcc\n\ts_xor_b64 %4, %4, vcc\n\ts_or_b64 %2, %2, %3\n\t"
                                 "v_addc_co_u32_e64 %0, vcc, 0, %0, %4\n\tv_addc_co_u32_e64 %1, vcc, 0, %1, %2"
                                 : "+v"(r1), "+v"(r2), "=&s"(m0), "=&s"(m1), "=&s"(m2)
                                 : "v"(kp), "v"(kw[u]), "v"(kw[u + 1]), "v"(kw[u + 2]) : "vcc", "scc");
                }
                asm volatile("v_cmp_gt_u32 vcc, %2, %3\n\tv_addc_co_u32_e32 %0, vcc, 0, %0, vcc\n\tv_lshl_add_u32 %0, %1, 1, %0"
                             : "+v"(r1) : "v"(r2), "v"(kw[24]), "v"(kp) : "vcc");
                r = r1;
            }
            kp += r & 1u;  // (the next count waits for this one, as the step's consumer does)
        }
        x0 = r;
    }
    T1;
    asm volatile("" : : "v"(x0), "v"(x1), "v"(x2), "v"(x3), "s"(m0), "s"(m1), "s"(m2), "s"(m3), "s"(s0), "s"(s1), "s"(s2), "s"(s3));
    // one word per wavefront, an ordinary vector store
    if ((threadIdx.x & 63) == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = (uint32_t)(t1 - t0);
}

typedef void (*kern_t)(uint32_t *, int, uint32_t, float);
template <int C>
struct Table {
    static void fill(kern_t (*t)[2]) {
        t[C][0] = k<C, false>;
        t[C][1] = k<C, true>;
        Table<C + 1>::fill(t);
    }
};
template <>
struct Table<C_COUNT> {
    static void fill(kern_t (*)[2]) {}
};

int main(int argc, char **argv) {
    const int trips = argc > 1 ? atoi(argv[1]) : 1024;
    if (trips < 1 || trips > (1 << 16)) { printf("trips must be 1 .. 65536\n"); return 1; }
    static kern_t tab[C_COUNT][2];
    Table<0>::fill(tab);
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const int lds_cu = 160 * 1024;  // gfx950: LDS per CU
    const int Ws[6] = {1, 2, 4, 6, 7, 8};
    const int max_waves = cus * 8 * 4;
    uint32_t *cyc;
    CHECK(hipMalloc(&cyc, max_waves * sizeof(uint32_t)));
    std::vector<uint32_t> h(max_waves);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    printf("# %s, %d CUs x 4 SIMDs, %d loop trips per wavefront; cycles per unit per SIMD = wavefront's s_memtime interval / (W x units per wavefront)\n",
           prop.gcnArchName, cus, trips);
    printf("# class | chains | W | blocks per CU the code object allows | units per wavefront | cycles per unit per SIMD: mean (min .. max over wavefronts) | launch by HIP events, us | ns per unit per SIMD by events | mean interval / launch, GHz\n");
    printf("# The SIMD issues the oldest wavefront first, so the wavefronts of a launch finish one after the other: the LONGEST interval (max) and the\n"
           "# launch by HIP events are what the SIMD needed, the mean is not; the last column is the shader clock only in the rows of one wavefront.\n");
    for (int c = 0; c < C_COUNT; ++c) {
        for (int dep = 0; dep < 2; ++dep) {
            const int per_trip = dep ? kCls[c].per_trip_dep : kCls[c].per_trip_ind;
            if (per_trip == 0) continue;
            for (int wi = 0; wi < 6; ++wi) {
                const int W = Ws[wi];
                // exactly W workgroups of this much LDS fit a CU (a lone one: more than half of it)
                const int lds = W == 1 ? 96 * 1024 : (lds_cu / W) / 2048 * 2048;
                const kern_t fn = tab[c][dep];
                CHECK(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
                int occ = 0;
                CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)fn, 256, lds));
                const int grid = cus * W;
                for (int rep = 0; rep < 2; ++rep) {  // (the first launch loads the code)
                    CHECK(hipEventRecord(e0, 0));
                    hipLaunchKernelGGL(fn, dim3(grid), dim3(256), lds, 0, cyc, trips, 1u + rep, 3.0f);
                    CHECK(hipEventRecord(e1, 0));
                    CHECK(hipDeviceSynchronize());
                }
                float ms = 0.0f;
                CHECK(hipEventElapsedTime(&ms, e0, e1));
                CHECK(hipMemcpy(h.data(), cyc, grid * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
                double sum = 0.0;
                uint32_t lo = ~0u, hi = 0;
                for (int i = 0; i < grid * 4; ++i) { sum += h[i]; lo = std::min(lo, h[i]); hi = std::max(hi, h[i]); }
                const double units = (double)trips * per_trip, den = units * W, mean = sum / (grid * 4);
                printf("%-50s | %s | %d | %d | %.0f %s | %6.2f (%6.2f .. %6.2f) | %8.1f | %7.3f | %.2f\n", kCls[c].name, dep ? "dep " : "ind4", W, occ, units,
                       kCls[c].unit, mean / den, lo / den, hi / den, ms * 1e3, ms * 1e6 / den, mean / (ms * 1e6));
            }
        }
    }
    CHECK(hipFree(cyc));
    return 0;
}
