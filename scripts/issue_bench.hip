// Issue-rate and clock microbenchmark for the RDF hot loop's instruction mix (round 2).
//   * real engine clock under each load: s_memtime (clock64) against s_memrealtime (wall_clock64, 100 MHz)
//     inside the kernel, printed next to the HIP-event time; run under
//     `rocprofv3 --pmc GRBM_GUI_ACTIVE --kernel-trace` to get the counter-based clock as well;
//   * SALU issue rate (independent s_add_u32 / s_and_b32 / s_lshr_b32), alone and beside VALU;
//   * the hot step's mix: 10 plain VALU + v_sqrt_f32 + 2 v_cmp + 10 SALU per 13 VALU;
//   * the same 13 VALU with v_cmpx + s_cbranch_execz around the seven behind the candidate test (round 7), at
//     0, 5 of 32 and all steps empty — the price of the branch alone and what a skipped tail gives back — after a
//     check that a skipped step leaves the mask register zero and its temporaries untouched;
//   * the price of what a trip issues AROUND the step (round 8), at the pair kernel's seven waves per SIMD: the
//     skip step with no empty step, then with 1, 2, 4 and 8 independent s_add_i32 spread through it, with a
//     compare and a not-taken s_cbranch_scc0 behind it, and with one and two more VALU instructions.
//   * the skip step with the bin position in 16.16 fixed point (round 17): v_cvt_flr_i32_f32, a 16-bit compare on
//     the low half and v_mad_u32_u16 on the high half instead of v_fract_f32, v_cmp_f32, v_cvt_i32_f32 and the
//     shift — 12 VALU where there were 13 — after a check that the fixed-point value, the mask and the address
//     come out as the C++ restatement says.
//   * the fixed-point skip step fed from an LDS slab (round 18, `--rot`): a broadcast row as in the row loops against
//     the rotated row of a diagonal tile's steps (lane l reads row (l + k) & 63, by index and by a running byte
//     offset) — after a check that every lane got that row.
//   * the same step fed from registers (round 19, `--rotreg`): the wave's own row moved one lane per step by
//     v_mov_b32_dpp with a whole-wave rotate — three registers, and four with the tag — after a check that after k
//     rotations every lane of every wave holds row (lane - k) & 63 (wave_ror:1) or (lane + k) & 63 (wave_rol:1) in
//     every register; and the rotated step as a LOOP, the way the pair kernel runs it: one step per turn, two steps
//     per turn with both reads in front, and the register forms.  Outcome (ns per step): three registers 24.3 - 24.6
//     against 24.6 - 25.0 of the LDS read, inside its scatter in one pass of three; four registers 26.3 - 26.6,
//     above it: not built.  Two steps per turn 23.6 - 23.8 against 25.2 - 25.4 of one per turn: below in every
//     pass — and in the pair kernel 0.3 ms per step SLOWER than the loop it has (NOTES.md, round 19): not built.
//   * orders of the skipping step's tail (round 19, `--tail`): v_sqrt_f32 in front of the v_cmpx (no s_nop),
//     v_mad_u32_u16 in front of the s_andn2_b64 of EXEC, and both — up to the address, as the rows of round 17 are,
//     and with the ds_add_u32 behind it (the whole tail; there also with the v_sqrt_f32 between the v_cmpx and the
//     branch).  Outcome at 5 of 32 steps empty: the moved root is above its yardstick in every form; the moved
//     v_mad_u32_u16 is within the yardstick's scatter up to the address and 0.2 - 0.4 ns ABOVE it in the whole tail
//     — and in the pair kernel 2.7 ms per step (1.4 %) FASTER, in five builds and five series.  These rows do not
//     predict the pair kernel; why is not known (one difference: a row's steps chain through a0 .. a2, the
//     kernel's steps are independent of each other).
// hipcc -O2 --offload-arch=gfx950 scripts/issue_bench.hip -o /tmp/issue_bench
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define REP16(x) x x x x x x x x x x x x x x x x
typedef float v2f __attribute__((ext_vector_type(2)));
// One step with the skip, as cell_step<..., SKIP> writes it: lanes whose r2 is below `hi` are candidates.
__global__ void skip_check(const float *r2_in, float hi, unsigned long long *mask, float *pos)
{
    const float r2 = r2_in[threadIdx.x];
    unsigned long long m;
    float tmp = -7.f, t = 0.f;
    asm volatile("v_cmpx_gt_f32_e64 %[mt], %[hi], %[r2]\n\ts_cbranch_execz .Lskip_check%=\n\t"
                 "v_sqrt_f32_e32 %[tmp], %[r2]\n\ts_nop 0\n\tv_fma_f32 %[tmp], %[tmp], 1.0, 0\n\tv_fract_f32_e32 %[t], %[tmp]\n\t"
                 "v_cmp_le_f32_e64 %[mt], 0.5, %[t]\n"
                 ".Lskip_check%=:\n\ts_mov_b64 exec, -1"
                 : [mt] "=&s"(m), [tmp] "+v"(tmp), [t] "+v"(t) : [hi] "s"(hi), [r2] "v"(r2) : "memory");
    pos[threadIdx.x] = tmp;
    if (threadIdx.x == 0) *mask = m;
}
// One step with the fixed-point tail, as cell_step<..., SKIP> writes it from round 17 on (without the narrowing of
// EXEC to the sure lanes, so that the address of every candidate lane can be looked at).
__global__ void fixed_check(const float *r2_in, float hi, float iwq, float p0q, unsigned tq, unsigned stride,
                            unsigned hb, unsigned long long *mask, float *root, unsigned *q_out, unsigned *ad_out)
{
    const float r2 = r2_in[threadIdx.x];
    unsigned long long m;
    float s = -7.f;
    unsigned q = 0xdeadbeefu, ad = 0xdeadbeefu;
    asm volatile("v_cmpx_gt_f32_e64 %[mt], %[hi], %[r2]\n\ts_cbranch_execz .Lfixed_check%=\n\t"
                 "v_sqrt_f32_e32 %[s], %[r2]\n\ts_nop 0\n\tv_fma_f32 %[q], %[s], %[iw], %[p0]\n\t"
                 "v_cvt_flr_i32_f32_e32 %[q], %[q]\n\t"
                 "v_cmp_le_u16_e64 %[mt], %[tq], %[q]\n\t"
                 "v_mad_u32_u16 %[ad], %[q], %[st], %[hb] op_sel:[1,0,0,0]\n"
                 ".Lfixed_check%=:\n\ts_mov_b64 exec, -1"
                 : [mt] "=&s"(m), [s] "+v"(s), [q] "+v"(q), [ad] "+v"(ad)
                 : [hi] "s"(hi), [r2] "v"(r2), [iw] "s"(iwq), [p0] "v"(p0q), [tq] "s"(tq), [st] "s"(stride), [hb] "v"(hb)
                 : "memory");
    root[threadIdx.x] = s;
    q_out[threadIdx.x] = q;
    ad_out[threadIdx.x] = ad;
    if (threadIdx.x == 0) *mask = m;
}
// The rows the rotated steps of a diagonal tile read (round 18): in step k lane l takes row (l + k) & 63 of its wave's
// slab — by the index the pair kernel forms (way 0) and by the running byte offset of MODE 18 (way 1).  Row r of wave
// v holds 64 v + r.
__global__ void rot_check(unsigned *rows, int way)
{
    __shared__ float4 slab[256];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    slab[threadIdx.x] = make_float4(0.f, 0.f, 0.f, float(threadIdx.x));
    __syncthreads();
    const float4 *sw = slab + wave * 64;
    unsigned off = lane * 16u;
    for (unsigned k = 0; k < 33u; ++k) {
        const float4 q = way == 0 ? sw[(lane + k) & 63u]
                                  : *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(sw) + off);
        off = (off + 16u) & 1023u;
        rows[(wave * 33u + k) * 64u + lane] = unsigned(q.w);
    }
}
// The rows the register form holds (round 19): every lane starts with its own row in four registers and moves them
// one lane per step with the whole-wave rotate CTRL (0x13C wave_ror:1, 0x134 wave_rol:1).  Register c of row r of
// wave v holds 4 (64 v + r) + c.
#define MDX_WAVE_ROT(x, CTRL) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false))
template <int CTRL>
__global__ void rotreg_check(unsigned *rows)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    float4 q = make_float4(float(4u * threadIdx.x), float(4u * threadIdx.x + 1u), float(4u * threadIdx.x + 2u),
                           float(4u * threadIdx.x + 3u));
#pragma unroll 1
    for (unsigned k = 0; k < 33u; ++k) {
        reinterpret_cast<uint4 *>(rows)[(wave * 33u + k) * 64u + lane] =
            make_uint4(unsigned(q.x), unsigned(q.y), unsigned(q.z), unsigned(q.w));
        q.x = MDX_WAVE_ROT(q.x, CTRL);
        q.y = MDX_WAVE_ROT(q.y, CTRL);
        q.z = MDX_WAVE_ROT(q.z, CTRL);
        q.w = MDX_WAVE_ROT(q.w, CTRL);
    }
}
// MODE 9: the skip step of MODE 8 with EMPTY reused as the extra scalar work per step: 0, 1, 2, 4 = that many
// s_add_i32 (8 as well, for a longer lever); 100 = s_cmp_eq_u32 (SCC = 1) + s_cbranch_scc0 that is never taken;
// 201, 202 = one, two extra VALU instructions (v_max_f32 of a register with itself), the other yardstick.
// MODE 10: the skip step of MODE 8 (bit k of EMPTY = step k has no candidate) with the fixed-point tail: 12 VALU.
template <int MODE, unsigned EMPTY = 0u>
__global__ void kern(float *out, long long *clk, int iters)
{
    float a0 = threadIdx.x, a1 = 1.f, a2 = 2.f, a3 = 3.f, a4 = 4.f, a5 = 5.f, a6 = 6.f, a7 = 7.f;
    float b = 1.0001f, c = 0.5f;
    v2f p0 = {a0, a1}, p1 = {a2, a3}, p2 = {a4, a5}, p3 = {a6, a7}, p4 = p0 + 1.f, p5 = p1 + 1.f, p6 = p2 + 1.f, p7 = p3 + 1.f;
    v2f pb = {b, b}, pc = {c, c};
    unsigned s0 = blockIdx.x, s1 = 1, s2 = 2, s3 = 3;
    // MODEs 16 - 18: a slab of 64 rows per wave of a 256-thread block (run7)
    __shared__ float4 rot_slab[((MODE >= 16 && MODE <= 18) || (MODE >= 25 && MODE <= 32)) ? 256 : 1];
    if ((MODE >= 16 && MODE <= 18) || (MODE >= 25 && MODE <= 32)) {
        if (threadIdx.x < 256)
            rot_slab[threadIdx.x] = make_float4(1.f + float(threadIdx.x & 63u), 2.f, 3.f, float(threadIdx.x & 63u));
        __syncthreads();
    }
    const long long t0 = clock64(), w0 = wall_clock64();
    for (int i = 0; i < iters; ++i) {
        if (MODE == 0) {   // 8 independent v_fma_f32
            REP16(asm volatile("v_fma_f32 %0, %0, %8, %9\n v_fma_f32 %1, %1, %8, %9\n v_fma_f32 %2, %2, %8, %9\n v_fma_f32 %3, %3, %8, %9\n"
                               "v_fma_f32 %4, %4, %8, %9\n v_fma_f32 %5, %5, %8, %9\n v_fma_f32 %6, %6, %8, %9\n v_fma_f32 %7, %7, %8, %9\n"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c));)
        } else if (MODE == 1) {   // 8 independent SALU
            REP16(asm volatile("s_add_u32 %0, %0, 3\n s_and_b32 %1, %1, 0xffff\n s_lshr_b32 %2, %2, 1\n s_add_u32 %3, %3, 5\n"
                               "s_add_u32 %0, %0, 7\n s_xor_b32 %1, %1, 0x55\n s_lshl_b32 %2, %2, 1\n s_sub_u32 %3, %3, 2\n"
                               : "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3) :: "scc");)
        } else if (MODE == 2) {   // 8 VALU + 8 SALU interleaved
            REP16(asm volatile("v_fma_f32 %0, %0, %12, %13\n s_add_u32 %8, %8, 3\n v_fma_f32 %1, %1, %12, %13\n s_and_b32 %9, %9, 0xffff\n"
                               "v_fma_f32 %2, %2, %12, %13\n s_lshr_b32 %10, %10, 1\n v_fma_f32 %3, %3, %12, %13\n s_add_u32 %11, %11, 5\n"
                               "v_fma_f32 %4, %4, %12, %13\n s_add_u32 %8, %8, 7\n v_fma_f32 %5, %5, %12, %13\n s_xor_b32 %9, %9, 0x55\n"
                               "v_fma_f32 %6, %6, %12, %13\n s_lshl_b32 %10, %10, 1\n v_fma_f32 %7, %7, %12, %13\n s_sub_u32 %11, %11, 2\n"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7),
                                 "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3)
                               : "v"(b), "v"(c) : "scc");)
        } else if (MODE == 3) {   // the hot step: 10 plain VALU + sqrt + 2 cmp (13 VALU), no SALU
            REP16(asm volatile("v_sub_f32 %0, %0, %8\n v_sub_f32 %1, %1, %8\n v_sub_f32 %2, %2, %8\n v_mul_f32 %3, %0, %0\n"
                               "v_fma_f32 %3, %1, %1, %3\n v_fma_f32 %3, %2, %2, %3\n v_sqrt_f32 %4, %3\n v_fma_f32 %4, %4, %8, %9\n"
                               "v_fract_f32 %5, %4\n v_cmp_gt_f32 vcc, %3, %9\n v_cmp_gt_f32 vcc, %5, %9\n v_cvt_i32_f32 %6, %4\n v_lshlrev_b32 %7, 2, %6\n"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c) : "vcc");)
        } else if (MODE == 4) {   // the same with 10 SALU spread through it
            REP16(asm volatile("v_sub_f32 %0, %0, %12\n s_add_u32 %8, %8, 3\n v_sub_f32 %1, %1, %12\n s_and_b32 %9, %9, 0xffff\n v_sub_f32 %2, %2, %12\n s_lshr_b32 %10, %10, 1\n v_mul_f32 %3, %0, %0\n"
                               "s_add_u32 %11, %11, 5\n v_fma_f32 %3, %1, %1, %3\n s_add_u32 %8, %8, 7\n v_fma_f32 %3, %2, %2, %3\n s_xor_b32 %9, %9, 0x55\n v_sqrt_f32 %4, %3\n s_lshl_b32 %10, %10, 1\n v_fma_f32 %4, %4, %12, %13\n"
                               "s_sub_u32 %11, %11, 2\n v_fract_f32 %5, %4\n s_add_u32 %8, %8, 1\n v_cmp_gt_f32 vcc, %3, %13\n s_add_u32 %9, %9, 1\n v_cmp_gt_f32 vcc, %5, %13\n v_cvt_i32_f32 %6, %4\n v_lshlrev_b32 %7, 2, %6\n"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7),
                                 "+s"(s0), "+s"(s1), "+s"(s2), "+s"(s3)
                               : "v"(b), "v"(c) : "vcc", "scc");)
        } else if (MODE == 5) {   // 8 independent v_pk_fma_f32 (two f32 per lane each)
            REP16(asm volatile("v_pk_fma_f32 %0, %0, %8, %9\n v_pk_fma_f32 %1, %1, %8, %9\n v_pk_fma_f32 %2, %2, %8, %9\n v_pk_fma_f32 %3, %3, %8, %9\n"
                               "v_pk_fma_f32 %4, %4, %8, %9\n v_pk_fma_f32 %5, %5, %8, %9\n v_pk_fma_f32 %6, %6, %8, %9\n v_pk_fma_f32 %7, %7, %8, %9\n"
                               : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7) : "v"(pb), "v"(pc));)
        } else if (MODE == 6) {   // 4 v_pk_add_f32 + 4 v_pk_mul_f32
            REP16(asm volatile("v_pk_add_f32 %0, %0, %8\n v_pk_mul_f32 %1, %1, %9\n v_pk_add_f32 %2, %2, %8\n v_pk_mul_f32 %3, %3, %9\n"
                               "v_pk_add_f32 %4, %4, %8\n v_pk_mul_f32 %5, %5, %9\n v_pk_add_f32 %6, %6, %8\n v_pk_mul_f32 %7, %7, %9\n"
                               : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3), "+v"(p4), "+v"(p5), "+v"(p6), "+v"(p7) : "v"(pb), "v"(pc));)
        } else if (MODE == 7) {   // 4 v_sub_u32 + 4 v_cvt_f32_i32 (fixed-point minimum image)
            REP16(asm volatile("v_sub_u32 %0, %0, %8\n v_cvt_f32_i32 %1, %0\n v_sub_u32 %2, %2, %8\n v_cvt_f32_i32 %3, %2\n"
                               "v_sub_u32 %4, %4, %8\n v_cvt_f32_i32 %5, %4\n v_sub_u32 %6, %6, %8\n v_cvt_f32_i32 %7, %6\n"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(b), "v"(c));)
        } else if (MODE == 8) {   // the hot step with the skip: 32 steps per turn, bit k of EMPTY = step k has no candidate
            const float pass = 3e38f, fail = -1.f;   // r2 stays finite and positive: every lane passes or none
#pragma unroll
            for (int k = 0; k < 32; ++k)
                asm volatile("v_sub_f32 %0, %0, %8\n v_sub_f32 %1, %1, %8\n v_sub_f32 %2, %2, %8\n v_mul_f32 %3, %0, %0\n"
                             "v_fma_f32 %3, %1, %1, %3\n v_fma_f32 %3, %2, %2, %3\n v_cmpx_gt_f32_e64 vcc, %10, %3\n"
                             "s_cbranch_execz .Lbench_skip%=\n v_sqrt_f32 %4, %3\n s_nop 0\n v_fma_f32 %4, %4, %8, %9\n"
                             "v_fract_f32 %5, %4\n v_cmp_gt_f32 vcc, %5, %9\n v_cvt_i32_f32 %6, %4\n v_lshlrev_b32 %7, 2, %6\n"
                             ".Lbench_skip%=:\n s_mov_b64 exec, -1\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                             : "v"(b), "v"(c), "s"(((EMPTY >> k) & 1u) ? fail : pass) : "vcc");
        } else if (MODE == 10 || MODE == 14 || MODE == 15) {
            // 10: the fixed-point tail (12 VALU).  Its two yardsticks: 14, the bare tail of MODE 9 without its
            // v_fract_f32 (12 plain VALU: what a removed instruction is worth), and 15, the bare tail with the pair
            // kernel's own three-operand v_lshl_add_u32 where MODE 9 has v_lshlrev_b32 (13 VALU: what the kernel
            // issued, the row the fixed-point tail has to beat).
            const float pass = 3e38f, fail = -1.f;
#define MDX_B10_STEP(TAIL)                                                                                           \
    asm volatile("v_sub_f32 %0, %0, %8\n v_sub_f32 %1, %1, %8\n v_sub_f32 %2, %2, %8\n v_mul_f32 %3, %0, %0\n"           \
                 "v_fma_f32 %3, %1, %1, %3\n v_fma_f32 %3, %2, %2, %3\n v_cmpx_gt_f32_e64 vcc, %10, %3\n"                 \
                 "s_cbranch_execz .Lbench10_skip%=\n v_sqrt_f32 %4, %3\n s_nop 0\n v_fma_f32 %4, %4, %8, %9\n" TAIL       \
                 ".Lbench10_skip%=:\n s_mov_b64 exec, -1\n"                                                            \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)                       \
                 : "v"(b), "v"(c), "s"(((EMPTY >> k) & 1u) ? fail : pass), "s"(s1), "s"(s2)                             \
                 : "vcc")
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                if (MODE == 10) MDX_B10_STEP("v_cvt_flr_i32_f32 %5, %4\n v_cmp_le_u16_e64 vcc, %11, %5\n v_mad_u32_u16 %7, %5, %12, %6 op_sel:[1,0,0,0]\n");
                else if (MODE == 14) MDX_B10_STEP("v_cmp_gt_f32 vcc, %4, %9\n v_cvt_i32_f32 %6, %4\n v_lshlrev_b32 %7, 2, %6\n");
                else MDX_B10_STEP("v_fract_f32 %5, %4\n v_cmp_gt_f32 vcc, %5, %9\n v_cvt_i32_f32 %6, %4\n v_lshl_add_u32 %7, %6, %12, %0\n");
            }
#undef MDX_B10_STEP
        } else if (MODE == 16 || MODE == 17 || MODE == 18) {
            // The fixed-point skipping step of MODE 10 fed from a wave-private LDS slab of 64 rows, as the pair kernel
            // feeds it (round 18).  16: the row loops' read — every lane the same row (a broadcast), the address a
            // scalar moved into a vector register; the yardstick.  17: the rotated step of a diagonal tile — lane l
            // reads row (l + k) & 63: v_add_u32, v_and_b32, v_lshl_add_u32 in front of the read.  18: the same rows
            // through a running byte offset, off = (off + 16) & 1023, added to the slab's base.
            const float pass = 3e38f;
            const unsigned lane = threadIdx.x & 63u;
            float4 *sw = rot_slab + (threadIdx.x >> 6) * 64;
            unsigned kbase = (unsigned(i) * 32u) & 63u;
            asm volatile("" : "+s"(kbase));
            unsigned off = (lane * 16u + kbase * 16u) & 1023u;
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                float4 q;
                if (MODE == 16) {
                    q = sw[(kbase + unsigned(k)) & 63u];
                } else if (MODE == 17) {
                    q = sw[(lane + kbase + unsigned(k)) & 63u];
                } else {
                    q = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(sw) + off);
                    off = (off + 16u) & 1023u;
                }
                asm volatile("" ::"v"(q.w));   // whole 16-byte read
                asm volatile("v_sub_f32 %0, %13, %8\n v_sub_f32 %1, %14, %8\n v_sub_f32 %2, %15, %8\n v_mul_f32 %3, %0, %0\n"
                             "v_fma_f32 %3, %1, %1, %3\n v_fma_f32 %3, %2, %2, %3\n v_cmpx_gt_f32_e64 vcc, %10, %3\n"
                             "s_cbranch_execz .Lbench16_skip%=\n v_sqrt_f32 %4, %3\n s_nop 0\n v_fma_f32 %4, %4, %8, %9\n"
                             "v_cvt_flr_i32_f32 %5, %4\n v_cmp_le_u16_e64 vcc, %11, %5\n v_mad_u32_u16 %7, %5, %12, %6 op_sel:[1,0,0,0]\n"
                             ".Lbench16_skip%=:\n s_mov_b64 exec, -1\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                             : "v"(b), "v"(c), "s"(pass), "s"(s1), "s"(s2), "v"(q.x), "v"(q.y), "v"(q.z)
                             : "vcc");
            }
        } else if (MODE == 19 || MODE == 20) {
            // The step of MODEs 16 - 18 fed from registers (round 19): the lane's own row, moved one lane per step by
            // three v_mov_b32_dpp wave_ror:1 (19), four with the tag (20).  No address, no LDS read.
            const float pass = 3e38f;
            float4 q = make_float4(1.f + float(threadIdx.x & 63u), 2.f, 3.f, float(threadIdx.x & 63u));
            asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w));
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                asm volatile("v_sub_f32 %0, %13, %8\n v_sub_f32 %1, %14, %8\n v_sub_f32 %2, %15, %8\n v_mul_f32 %3, %0, %0\n"
                             "v_fma_f32 %3, %1, %1, %3\n v_fma_f32 %3, %2, %2, %3\n v_cmpx_gt_f32_e64 vcc, %10, %3\n"
                             "s_cbranch_execz .Lbench19_skip%=\n v_sqrt_f32 %4, %3\n s_nop 0\n v_fma_f32 %4, %4, %8, %9\n"
                             "v_cvt_flr_i32_f32 %5, %4\n v_cmp_le_u16_e64 vcc, %11, %5\n v_mad_u32_u16 %7, %5, %12, %6 op_sel:[1,0,0,0]\n"
                             ".Lbench19_skip%=:\n s_mov_b64 exec, -1\n"
                             : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                             : "v"(b), "v"(c), "s"(pass), "s"(s1), "s"(s2), "v"(q.x), "v"(q.y), "v"(q.z)
                             : "vcc");
                q.x = MDX_WAVE_ROT(q.x, 0x13C);
                q.y = MDX_WAVE_ROT(q.y, 0x13C);
                q.z = MDX_WAVE_ROT(q.z, 0x13C);
                if (MODE == 20) {
                    q.w = MDX_WAVE_ROT(q.w, 0x13C);
                    asm volatile("" ::"v"(q.w));
                }
            }
            a7 += q.x + q.w;
        } else if (MODE >= 25 && MODE <= 28) {
            // The rotated step as a LOOP, which is how the pair kernel runs it (MODEs 16 - 20 unroll 32 steps, and the
            // compiler issues their reads well ahead).  25: one step per turn — index, read, wait, step — the
            // kernel's loop of round 18.  26: two steps per turn, both reads issued before the first wait, the rows
            // through the running byte offset of MODE 18.  27, 28: one step per turn on registers, four and three
            // v_mov_b32_dpp wave_ror:1.
            const float pass = 3e38f;
            const unsigned lane = threadIdx.x & 63u;
            float4 *sw = rot_slab + (threadIdx.x >> 6) * 64;
#define MDX_B25_STEP(Q)                                                                                              \
    asm volatile("v_sub_f32 %0, %13, %8\n v_sub_f32 %1, %14, %8\n v_sub_f32 %2, %15, %8\n v_mul_f32 %3, %0, %0\n"        \
                 "v_fma_f32 %3, %1, %1, %3\n v_fma_f32 %3, %2, %2, %3\n v_cmpx_gt_f32_e64 vcc, %10, %3\n"                 \
                 "s_cbranch_execz .Lbench25_skip%=\n v_sqrt_f32 %4, %3\n s_nop 0\n v_fma_f32 %4, %4, %8, %9\n"            \
                 "v_cvt_flr_i32_f32 %5, %4\n v_cmp_le_u16_e64 vcc, %11, %5\n v_mad_u32_u16 %7, %5, %12, %6 op_sel:[1,0,0,0]\n" \
                 ".Lbench25_skip%=:\n s_mov_b64 exec, -1\n"                                                            \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)                       \
                 : "v"(b), "v"(c), "s"(pass), "s"(s1), "s"(s2), "v"(Q.x), "v"(Q.y), "v"(Q.z)                            \
                 : "vcc")
            if (MODE == 25) {
                unsigned kbase = (unsigned(i) * 32u) & 63u;
                asm volatile("" : "+s"(kbase));
#pragma unroll 1
                for (unsigned k = 0; k < 32u; ++k) {
                    const float4 q = sw[(lane + kbase + k) & 63u];
                    asm volatile("" ::"v"(q.w));   // whole 16-byte read
                    MDX_B25_STEP(q);
                }
            } else if (MODE == 26) {
                unsigned off = (lane * 16u + unsigned(i) * 512u) & 1023u;
#pragma unroll 1
                for (unsigned t = 0; t < 16u; ++t) {
                    const float4 q0 = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(sw) + off);
                    off = (off + 16u) & 1023u;
                    const float4 q1 = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(sw) + off);
                    off = (off + 16u) & 1023u;
                    asm volatile("" ::"v"(q0.w), "v"(q1.w));   // both reads in front of the first step
                    MDX_B25_STEP(q0);
                    MDX_B25_STEP(q1);
                }
            } else {
                float4 q = sw[lane];
                asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w));
#pragma unroll 1
                for (unsigned k = 0; k < 32u; ++k) {
                    MDX_B25_STEP(q);
                    q.x = MDX_WAVE_ROT(q.x, 0x13C);
                    q.y = MDX_WAVE_ROT(q.y, 0x13C);
                    q.z = MDX_WAVE_ROT(q.z, 0x13C);
                    if (MODE == 27) {
                        q.w = MDX_WAVE_ROT(q.w, 0x13C);
                        asm volatile("" ::"v"(q.w));
                    }
                }
                a7 += q.x + q.w;
            }
#undef MDX_B25_STEP
        } else if ((MODE >= 21 && MODE <= 24) || (MODE >= 29 && MODE <= 32)) {
            // Orders of the tail of the fixed-point skipping step of MODE 10 (round 19), with the s_andn2_b64 of EXEC
            // that the pair kernel's tail has between the undecided test and the address.  21 - 24 end at the address,
            // as MODE 10 does; 29 - 32 are the WHOLE tail: the ds_add_u32 that reads the address follows, every lane
            // adding to a word of its own in the wave's slab (the stride operand is zero, the base the lane's word:
            // no conflicts, nothing out of bounds).
            //   22, 29: the kernel's order of round 17 — s_andn2_b64, v_mad_u32_u16 — the yardsticks.
            //   23, 30: (b) v_mad_u32_u16 in front of the s_andn2_b64.
            //   21: (a) v_sqrt_f32 in front of the v_cmpx, no s_nop (the compare and the branch stand between the root
            //       and the v_fma_f32 that reads it).  24: (c) = (a) and (b).
            //   31: v_sqrt_f32 between the v_cmpx and s_cbranch_execz, no s_nop (the root of the candidate lanes
            //       alone).  32: 31 and (b).
            const float pass = 3e38f, fail = -1.f;
            constexpr bool WHOLE = MODE >= 29;
            unsigned word = (unsigned)(size_t)(__attribute__((address_space(3))) float4 *)rot_slab + threadIdx.x * 4u;
            unsigned stride = WHOLE ? 0u : s2, one = 1u;
            asm volatile("" : "+v"(word), "+s"(stride), "+v"(one));
// (ROOT0, ROOTX, ROOT1: the square root in front of the v_cmpx, between it and the branch, or behind the branch)
#define MDX_B21_STEP(ROOT0, ROOTX, ROOT1, TAIL)                                                                       \
    asm volatile("v_sub_f32 %0, %0, %8\n v_sub_f32 %1, %1, %8\n v_sub_f32 %2, %2, %8\n v_mul_f32 %3, %0, %0\n"           \
                 "v_fma_f32 %3, %1, %1, %3\n v_fma_f32 %3, %2, %2, %3\n" ROOT0 "v_cmpx_gt_f32_e64 vcc, %10, %3\n" ROOTX  \
                 "s_cbranch_execz .Lbench21_skip%=\n" ROOT1 "v_fma_f32 %4, %4, %8, %9\n"                                \
                 "v_cvt_flr_i32_f32 %5, %4\n v_cmp_le_u16_e64 vcc, %11, %5\n" TAIL                                     \
                 ".Lbench21_skip%=:\n s_mov_b64 exec, -1\n"                                                            \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)                       \
                 : "v"(b), "v"(c), "s"(((EMPTY >> k) & 1u) ? fail : pass), "s"(s1), "s"(stride), "v"(word), "v"(one)    \
                 : "vcc", "scc", "memory")   /* (s_andn2_b64 writes SCC) */
#define MDX_B21_ROOT "v_sqrt_f32 %4, %3\n"
#define MDX_B21_ROOT_NOP "v_sqrt_f32 %4, %3\n s_nop 0\n"
#define MDX_B21_NARROW_FIRST(BASE) "s_andn2_b64 exec, exec, vcc\n v_mad_u32_u16 %7, %5, %12, " BASE " op_sel:[1,0,0,0]\n"
#define MDX_B21_MAD_FIRST(BASE) "v_mad_u32_u16 %7, %5, %12, " BASE " op_sel:[1,0,0,0]\n s_andn2_b64 exec, exec, vcc\n"
#define MDX_B21_ADD "ds_add_u32 %7, %14\n"
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                if (MODE == 22) MDX_B21_STEP("", "", MDX_B21_ROOT_NOP, MDX_B21_NARROW_FIRST("%6"));
                else if (MODE == 21) MDX_B21_STEP(MDX_B21_ROOT, "", "", MDX_B21_NARROW_FIRST("%6"));
                else if (MODE == 23) MDX_B21_STEP("", "", MDX_B21_ROOT_NOP, MDX_B21_MAD_FIRST("%6"));
                else if (MODE == 24) MDX_B21_STEP(MDX_B21_ROOT, "", "", MDX_B21_MAD_FIRST("%6"));
                else if (MODE == 29) MDX_B21_STEP("", "", MDX_B21_ROOT_NOP, MDX_B21_NARROW_FIRST("%13") MDX_B21_ADD);
                else if (MODE == 30) MDX_B21_STEP("", "", MDX_B21_ROOT_NOP, MDX_B21_MAD_FIRST("%13") MDX_B21_ADD);
                else if (MODE == 31) MDX_B21_STEP("", MDX_B21_ROOT, "", MDX_B21_NARROW_FIRST("%13") MDX_B21_ADD);
                else MDX_B21_STEP("", MDX_B21_ROOT, "", MDX_B21_MAD_FIRST("%13") MDX_B21_ADD);
            }
#undef MDX_B21_STEP
#undef MDX_B21_ROOT
#undef MDX_B21_ROOT_NOP
#undef MDX_B21_NARROW_FIRST
#undef MDX_B21_MAD_FIRST
#undef MDX_B21_ADD
        } else if (MODE == 9) {
            // (operands %8 and %9 are b and c in MODE 8; here the four scalar counters sit at %8..%11, so the
            // strings below are written with their own numbering: b = %12, c = %13, pass = %14)
            const float pass = 3e38f;
#pragma unroll
            for (int k = 0; k < 32; ++k) {
#define MDX_B9_STEP(S1, S2, S3)                                                                                      \
    asm volatile("v_sub_f32 %0, %0, %12\n v_sub_f32 %1, %1, %12\n" S1 "v_sub_f32 %2, %2, %12\n v_mul_f32 %3, %0, %0\n"      \
                 "v_fma_f32 %3, %1, %1, %3\n" S2 "v_fma_f32 %3, %2, %2, %3\n v_cmpx_gt_f32_e64 vcc, %14, %3\n"               \
                 "s_cbranch_execz .Lbench9_skip%=\n v_sqrt_f32 %4, %3\n s_nop 0\n v_fma_f32 %4, %4, %12, %13\n"              \
                 "v_fract_f32 %5, %4\n v_cmp_gt_f32 vcc, %5, %13\n v_cvt_i32_f32 %6, %4\n v_lshlrev_b32 %7, 2, %6\n"          \
                 ".Lbench9_skip%=:\n s_mov_b64 exec, -1\n" S3                                                            \
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7), "+s"(s0), "+s"(s1),  \
                   "+s"(s2), "+s"(s3)                                                                                \
                 : "v"(b), "v"(c), "s"(pass)                                                                         \
                 : "vcc", "scc")
                if (EMPTY == 0u) MDX_B9_STEP("", "", "");
                else if (EMPTY == 1u) MDX_B9_STEP("", "s_add_i32 %8, %8, 3\n", "");
                else if (EMPTY == 2u) MDX_B9_STEP("s_add_i32 %8, %8, 3\n", "", "s_add_i32 %9, %9, 5\n");
                else if (EMPTY == 4u) MDX_B9_STEP("s_add_i32 %8, %8, 3\n s_add_i32 %10, %10, 1\n", "s_add_i32 %11, %11, 7\n", "s_add_i32 %9, %9, 5\n");
                else if (EMPTY == 8u) MDX_B9_STEP("s_add_i32 %8, %8, 3\n s_add_i32 %10, %10, 1\n s_add_i32 %9, %9, 1\n", "s_add_i32 %11, %11, 7\n s_add_i32 %8, %8, 1\n s_add_i32 %10, %10, 3\n", "s_add_i32 %9, %9, 5\n s_add_i32 %11, %11, 5\n");
                else if (EMPTY == 201u) MDX_B9_STEP("", "v_max_f32 %7, %7, %7\n", "");
                else if (EMPTY == 202u) MDX_B9_STEP("v_max_f32 %7, %7, %7\n", "", "v_max_f32 %6, %6, %6\n");
                else MDX_B9_STEP("", "", "s_cmp_eq_u32 %8, %8\n s_cbranch_scc0 .Lbench9_skip%=\n");
#undef MDX_B9_STEP
            }
        }
    }
    const long long t1 = clock64(), w1 = wall_clock64();
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        clk[0] = t1 - t0;
        clk[1] = w1 - w0;
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + float(s0 + s1 + s2 + s3) +
        (p0 + p1 + p2 + p3 + p4 + p5 + p6 + p7).x + (p0 + p1 + p2 + p3 + p4 + p5 + p6 + p7).y;
}
template <int MODE, unsigned EMPTY = 0u> void run(const char *name, int n_valu, int n_salu, int groups = 16)
{
    float *d; hipMalloc(&d, 256 * 64 * 64 * 4 * 8);
    long long *clk; hipMalloc(&clk, 16);
    for (int waves = 1; waves <= 8; waves *= 2) {
        if (waves == 8) waves = 6;
        dim3 grid(256), block(64 * 4 * (waves > 4 ? 4 : waves));
        if (waves == 6) { grid = dim3(512); block = dim3(64 * 4 * 3); }   // 2 blocks of 12 waves per CU
        const int iters = 4000;
        kern<MODE, EMPTY><<<grid, block>>>(d, clk, 10);
        hipDeviceSynchronize();
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        hipEventRecord(e0);
        kern<MODE, EMPTY><<<grid, block>>>(d, clk, iters);
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        long long h[2]; hipMemcpy(h, clk, 16, hipMemcpyDeviceToHost);
        const double mhz_memtime = double(h[0]) / double(h[1]) * 100.0;
        const double steps_per_simd = double(iters) * groups * waves;
        printf("%-22s waves/SIMD=%d  %.3f ms  per 16-instr group and SIMD: %.1f ns = %.1f cycles at 2.4 GHz  "
               "(VALU %d SALU %d per group; s_memtime/s_memrealtime -> %.0f MHz)\n",
               name, waves, ms, ms * 1e6 / steps_per_simd, ms * 1e-3 * 2.4e9 / steps_per_simd, n_valu, n_salu, mhz_memtime);
        if (waves == 6) break;
    }
    hipFree(d); hipFree(clk);
}
// The pair kernel's occupancy: seven blocks of 256 threads per CU = seven waves per SIMD.
template <int MODE, unsigned EXTRA> void run7(const char *name, int n_valu, int n_salu)
{
    float *d; hipMalloc(&d, size_t(256) * 7 * 256 * 4);
    long long *clk; hipMalloc(&clk, 16);
    const int waves = 7, groups = 32, iters = 4000;
    dim3 grid(256 * 7), block(256);
    kern<MODE, EXTRA><<<grid, block>>>(d, clk, 10);
    hipDeviceSynchronize();
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0);
    kern<MODE, EXTRA><<<grid, block>>>(d, clk, iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    long long h[2]; hipMemcpy(h, clk, 16, hipMemcpyDeviceToHost);
    const double mhz = double(h[0]) / double(h[1]) * 100.0;
    const double steps_per_simd = double(iters) * groups * waves;
    printf("%-30s waves/SIMD=%d  %.3f ms  per step and SIMD: %.2f ns = %.2f cycles at the measured %.0f MHz  "
           "(VALU %d, scalar/branch %d per step)\n",
           name, waves, ms, ms * 1e6 / steps_per_simd, ms * 1e-3 * mhz * 1e6 / steps_per_simd, mhz, n_valu, n_salu);
    hipFree(d); hipFree(clk);
}
// Every lane a candidate, none, the odd lanes: the mask must hold the undecided candidates (fract >= 0.5) — zero
// after a skipped step, whose temporaries stay untouched.
static bool check_skip()
{
    float *r2, *pos, h_r2[64], h_pos[64], h_want[64];
    unsigned long long *mask, h_mask;
    hipMalloc(&r2, 256); hipMalloc(&pos, 256); hipMalloc(&mask, 8);
    bool ok = true;
    const char *names[3] = {"every lane a candidate", "no candidate (step skipped)", "odd lanes candidates"};
    for (int variant = 0; variant < 3; ++variant) {
        unsigned long long want = 0;
        for (int l = 0; l < 64; ++l) {
            const bool cand = variant == 0 || (variant == 2 && (l & 1));
            const float r = (l & 2) ? 2.75f : 2.f;      // fract 0.75: undecided; fract 0: decided
            h_r2[l] = cand ? r * r : 100.f;             // the candidate test is r2 < 50
            h_want[l] = cand ? r : -7.f;
            if (cand && (l & 2)) want |= 1ull << l;
        }
        hipMemcpy(r2, h_r2, 256, hipMemcpyHostToDevice);
        skip_check<<<1, 64>>>(r2, 50.f, mask, pos);
        hipMemcpy(&h_mask, mask, 8, hipMemcpyDeviceToHost);
        hipMemcpy(h_pos, pos, 256, hipMemcpyDeviceToHost);
        bool good = h_mask == want;
        for (int l = 0; l < 64; ++l)
            good = good && h_pos[l] == h_want[l];
        printf("skip check, %s: mask %016llx (want %016llx) %s\n", names[variant], h_mask, want, good ? "ok" : "WRONG");
        ok = ok && good;
    }
    hipFree(r2); hipFree(pos); hipFree(mask);
    return ok;
}
// The fixed-point tail against its C++ restatement: q = floor(sqrt(r2) * IWQ + P0Q) as a 32-bit integer, undecided
// <=> low16(q) >= TQ, address = high16(q) * stride + base (all modulo 2^32).  inv_w = 1, pos0 = -0.25, sure_w = 0.5.
static bool check_fixed()
{
    float *r2, *root, h_r2[64], h_root[64];
    unsigned *q, *ad, h_q[64], h_ad[64];
    unsigned long long *mask, h_mask;
    hipMalloc(&r2, 256); hipMalloc(&root, 256); hipMalloc(&q, 256); hipMalloc(&ad, 256); hipMalloc(&mask, 8);
    const float iwq = 65536.f, p0q = -0.25f * 65536.f;
    const unsigned tq = 32768u, stride = 12u, hb = 0x1230u;
    bool ok = true;
    const char *names[5] = {"every lane sure", "every lane undecided", "no candidate (step skipped)",
                            "odd lanes candidates", "negative positions"};
    for (int variant = 0; variant < 5; ++variant) {
        for (int l = 0; l < 64; ++l) {
            float r = 2.5f + float(l);                          // position l + 2.25: sure, bin l + 2
            if (variant == 1) r = 2.f + float(l);               // position l + 1.75: undecided
            if (variant == 3) r = (l & 2) ? 2.f + float(l) : 2.5f + float(l);
            if (variant == 4) r = float(l) * (1.f / 256.f);     // positions -0.25 ... -0.004: undecided, high half all ones
            h_r2[l] = r * r;                                    // the candidate test is r2 < 5000
            if (variant == 2 || (variant == 3 && !(l & 1))) h_r2[l] = 1e4f;
        }
        hipMemcpy(r2, h_r2, 256, hipMemcpyHostToDevice);
        fixed_check<<<1, 64>>>(r2, 5000.f, iwq, p0q, tq, stride, hb, mask, root, q, ad);
        hipMemcpy(&h_mask, mask, 8, hipMemcpyDeviceToHost);
        hipMemcpy(h_root, root, 256, hipMemcpyDeviceToHost);
        hipMemcpy(h_q, q, 256, hipMemcpyDeviceToHost);
        hipMemcpy(h_ad, ad, 256, hipMemcpyDeviceToHost);
        unsigned long long want = 0;
        bool good = true;
        for (int l = 0; l < 64; ++l) {
            if (!(h_r2[l] < 5000.f)) {   // not a candidate: nothing written
                good = good && h_root[l] == -7.f && h_q[l] == 0xdeadbeefu && h_ad[l] == 0xdeadbeefu;
                continue;
            }
            const unsigned wq = unsigned(int(floorf(fmaf(h_root[l], iwq, p0q))));
            if ((wq & 0xffffu) >= tq) want |= 1ull << l;
            good = good && h_q[l] == wq && h_ad[l] == (wq >> 16) * stride + hb && h_root[l] >= 0.f;
            if (variant == 4) good = good && (wq >> 16) == 0xffffu;
            if (variant == 0) good = good && (wq >> 16) == unsigned(l + 2);
        }
        good = good && h_mask == want;
        if (variant == 0) good = good && want == 0ull;
        if (variant == 1 || variant == 4) good = good && want == ~0ull;
        printf("fixed-point check, %s: mask %016llx (want %016llx) %s\n", names[variant], h_mask, want, good ? "ok" : "WRONG");
        ok = ok && good;
    }
    hipFree(r2); hipFree(root); hipFree(q); hipFree(ad); hipFree(mask);
    return ok;
}
// Every lane of every wave got row (lane + k) & 63 of its own slab in step k = 0 .. 32, either way.
static bool check_rot()
{
    unsigned *rows, h[4 * 33 * 64];
    hipMalloc(&rows, sizeof h);
    bool ok = true;
    for (int way = 0; way < 2; ++way) {
        hipMemset(rows, 0xff, sizeof h);
        rot_check<<<1, 256>>>(rows, way);
        hipMemcpy(h, rows, sizeof h, hipMemcpyDeviceToHost);
        int wrong = 0;
        for (unsigned wave = 0; wave < 4; ++wave)
            for (unsigned k = 0; k < 33; ++k)
                for (unsigned lane = 0; lane < 64; ++lane)
                    wrong += h[(wave * 33 + k) * 64 + lane] != 64 * wave + ((lane + k) & 63u);
        printf("rotation check, %s: %d of %d rows wrong %s\n", way ? "running byte offset" : "index (lane + k) & 63", wrong,
               4 * 33 * 64, wrong ? "WRONG" : "ok");
        ok = ok && !wrong;
    }
    hipFree(rows);
    return ok;
}
// After k one-lane rotations (k = 0 .. 32) every lane of every wave holds, in all four registers, row (lane - k) & 63
// (sign -1) or (lane + k) & 63 (sign +1) of its own wave.  Returns the sign found, 0 if a lane is wrong.
template <int CTRL> static int check_rotreg(const char *name)
{
    static unsigned h[4 * 33 * 64 * 4];
    unsigned *rows;
    hipMalloc(&rows, sizeof h);
    hipMemset(rows, 0xff, sizeof h);
    rotreg_check<CTRL><<<1, 256>>>(rows);
    hipMemcpy(h, rows, sizeof h, hipMemcpyDeviceToHost);
    hipFree(rows);
    const unsigned first = h[(0 * 33 + 1) * 64 * 4 + 4 * 1] / 4u;   // wave 0, k = 1, lane 1, register 0
    const int sign = first == 0u ? -1 : first == 2u ? 1 : 0;
    int wrong = 0;
    for (unsigned wave = 0; wave < 4 && sign; ++wave)
        for (unsigned k = 0; k < 33; ++k)
            for (unsigned lane = 0; lane < 64; ++lane)
                for (unsigned c = 0; c < 4; ++c) {
                    const unsigned got = h[((wave * 33 + k) * 64 + lane) * 4 + c];
                    const unsigned want = 4u * (64u * wave + ((lane + unsigned(sign * int(k))) & 63u)) + c;
                    if (got != want && wrong++ < 8)
                        printf("  wave %u step %u lane %u register %u holds %u, not %u\n", wave, k, lane, c, got, want);
                }
    if (!sign)
        printf("register rotation check, %s: lane 1 holds row %u after one rotation — neither neighbour WRONG\n", name, first);
    else
        printf("register rotation check, %s: after k rotations lane l holds row (l %c k) & 63; %d of %d values wrong %s\n",
               name, sign > 0 ? '+' : '-', wrong, 4 * 33 * 64 * 4, wrong ? "WRONG" : "ok");
    return wrong ? 0 : sign;
}
int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "--rotreg")) {   // the round-19 register rows
        const int ror = check_rotreg<0x13C>("wave_ror:1"), rol = check_rotreg<0x134>("wave_rol:1");
        if (!ror || !rol) return 1;   // not timed
        const int passes = argc > 2 ? atoi(argv[2]) : 3;
        for (int pass = 0; pass < passes; ++pass) {
            run7<10, 0u>("skip step fixed-point", 12, 2);
            run7<16, 0u>("fixed-point, broadcast row", 13, 2);
            run7<17, 0u>("fixed-point, rotated row", 15, 2);
            run7<18, 0u>("fixed-point, rotated, offset", 15, 2);
            run7<19, 0u>("fixed-point, 3 registers dpp", 15, 2);
            run7<20, 0u>("fixed-point, 4 registers dpp", 16, 2);
            run7<25, 0u>("loop, rotated row, 1 per turn", 15, 5);
            run7<26, 0u>("loop, rotated rows, 2 per turn", 15, 4);
            run7<28, 0u>("loop, 3 registers dpp", 15, 5);
            run7<27, 0u>("loop, 4 registers dpp", 16, 5);
        }
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "--tail")) {   // the round-19 tail orders
        if (!check_fixed()) return 1;
        const int passes = argc > 2 ? atoi(argv[2]) : 3;
        for (int pass = 0; pass < passes; ++pass) {
            run7<10, 0u>("skip step fixed-point", 12, 2);
            run7<22, 0u>("fixed-point + s_andn2 exec", 12, 3);
            run7<21, 0u>("(a) sqrt before cmpx", 12, 2);
            run7<23, 0u>("(b) mad before s_andn2", 12, 3);
            run7<24, 0u>("(c) both", 12, 2);
            run7<10, 0x04082082u>("skip step fixed-point, 5/32", 12, 2);
            run7<22, 0x04082082u>("fixed-point + s_andn2, 5/32", 12, 3);
            run7<21, 0x04082082u>("(a) sqrt before cmpx, 5/32", 12, 2);
            run7<23, 0x04082082u>("(b) mad before s_andn2, 5/32", 12, 3);
            run7<24, 0x04082082u>("(c) both, 5/32", 12, 2);
            run7<29, 0u>("whole tail, kernel's order", 12, 3);
            run7<30, 0u>("whole tail, (b) mad first", 12, 3);
            run7<31, 0u>("whole tail, sqrt behind cmpx", 12, 2);
            run7<32, 0u>("whole tail, both", 12, 2);
            run7<29, 0x04082082u>("whole tail, kernel's, 5/32", 12, 3);
            run7<30, 0x04082082u>("whole tail, (b), 5/32", 12, 3);
            run7<31, 0x04082082u>("whole tail, sqrt behind, 5/32", 12, 2);
            run7<32, 0x04082082u>("whole tail, both, 5/32", 12, 2);
        }
        return 0;
    }
    const bool fixed_only = argc > 1 && !strcmp(argv[1], "--fixed");   // the round-17 rows alone
    if (argc > 1 && !strcmp(argv[1], "--rot")) {   // the round-18 rows alone
        if (!check_rot()) return 1;
        const int passes = argc > 2 ? atoi(argv[2]) : 3;
        for (int pass = 0; pass < passes; ++pass) {
            run7<9, 0u>("skip step bare", 13, 2);
            run7<10, 0u>("skip step fixed-point", 12, 2);
            run7<16, 0u>("fixed-point, broadcast row", 13, 2);
            run7<17, 0u>("fixed-point, rotated row", 15, 2);
            run7<18, 0u>("fixed-point, rotated, offset", 15, 2);
        }
        return 0;
    }
    if (fixed_only) {
        if (!check_fixed()) return 1;
        const int passes = argc > 2 ? atoi(argv[2]) : 3;
        for (int pass = 0; pass < passes; ++pass) {
            run7<9, 0u>("skip step bare", 13, 2);
            run7<10, 0u>("skip step fixed-point", 12, 2);
            run7<8, 0x04082082u>("skip step, 5/32 empty", 13, 2);
            run7<10, 0x04082082u>("skip step fixed-point, 5/32", 12, 2);
            run7<14, 0u>("bare without v_fract_f32", 12, 2);
            run7<15, 0u>("bare, v_lshl_add_u32", 13, 2);
            run7<15, 0x04082082u>("bare, v_lshl_add_u32, 5/32", 13, 2);
        }
        return 0;
    }
    run<0>("8 v_fma_f32", 8, 0);
    run<1>("8 SALU", 0, 8);
    run<2>("8 v_fma_f32 + 8 SALU", 8, 8);
    run<3>("hot step 13 VALU", 13, 0);
    run<4>("hot step 13 VALU+10 SALU", 13, 10);
    run<5>("8 v_pk_fma_f32", 8, 0);
    run<6>("4 pk_add + 4 pk_mul f32", 8, 0);
    run<7>("4 v_sub_u32+4 cvt_f32_i32", 8, 0);
    if (!check_skip()) return 1;
    if (!check_fixed()) return 1;
    run<8, 0u>("skip step, 0/32 empty", 13, 1, 32);
    run<8, 0x04082082u>("skip step, 5/32 empty", 13, 1, 32);
    run<8, ~0u>("skip step, 32/32 empty", 13, 1, 32);
    // three passes: they show how far two runs of one row differ
    for (int pass = 0; pass < 3; ++pass) {
        run7<9, 0u>("skip step bare", 13, 2);
        run7<9, 1u>("skip step + 1 s_add_i32", 13, 3);
        run7<9, 2u>("skip step + 2 s_add_i32", 13, 4);
        run7<9, 4u>("skip step + 4 s_add_i32", 13, 6);
        run7<9, 8u>("skip step + 8 s_add_i32", 13, 10);
        run7<9, 100u>("skip step + s_cmp + s_cbranch", 13, 4);
        run7<9, 201u>("skip step + 1 VALU", 14, 2);
        run7<9, 202u>("skip step + 2 VALU", 15, 2);
        run7<10, 0u>("skip step fixed-point", 12, 2);
        run7<8, 0x04082082u>("skip step, 5/32 empty", 13, 2);
        run7<10, 0x04082082u>("skip step fixed-point, 5/32", 12, 2);
    }
    return 0;
}
