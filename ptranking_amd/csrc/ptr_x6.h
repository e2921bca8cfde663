// The "bf16 x 6" arithmetic, in one place: every fp32 product on the hot path is six bf16 matrix products on operands split EXACTLY into three
// bf16 planes.  The split, the order of the six products and the transpose-read that feeds them are the numeric contract between the kernels
// (scorer_x6.hip, scorer_bwd_x6.hip, scorer_dw_x6.hip, linear_x6.hip, linear_bw_x6.hip, the image hand-over x6_img_put in ptr_mlp.h): the float64
// gates, "the image the optimiser refreshes is bit-identical to a fresh prep" and the bit-stability tests all rest on every kernel doing these steps
// the same way, so they are written here once.  Plain inline functions; layouts, tilings and schedules stay with the kernels.
//
// Arithmetic.  An fp32 number is EXACTLY the sum of three bf16 pieces (8 + 8 + 8 mantissa bits), so
//     a * b = a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a2 b2 + a3 b1) + terms below 2^-24 |a b|:
// six v_mfma_f32_16x16x32_bf16 (fp32 accumulation inside the instruction) do the work of eight v_mfma_f32_16x16x4_f32 at 6 x 16 instead of 8 x 32
// issue cycles, with an error against float64 equal to or below the fp32 MFMA's (scratch/bf16x6, tests/test_x6_gpu.py).
#pragma once
#include "ptr_device.h"
#include "ptr_dropout.h"          // f32x4

namespace ptr {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;
using i16x4 = __attribute__((ext_vector_type(4))) short;
using lds_u32x4 = __attribute__((address_space(3))) u32x4;
using lds_u32x2 = __attribute__((address_space(3))) u32x2;
using lds_f32x4 = __attribute__((address_space(3))) f32x4;
using lds_i16x4 = __attribute__((address_space(3))) i16x4;
// one MFMA operand of one plane: 8 bf16 per lane (the 16-deep instruction takes the first two dwords)
union Frag { bf16x8 v; u32x4 q; uint32_t u[4]; };

// ---- the split
// Split by ROUNDING (v_cvt_pk_bf16_f32, round to nearest even): a = p1 + p2 + p3 exactly (|p2| <= 2^-9 |a|, |p3| <= 2^-18 |a|), and the
// pieces below the first carry either sign — the dropped products a2 b3 + a3 b2 + a3 b3 (<= 2^-26 |a b|) average out.  A split by
// truncation (two AND / SUB pairs, r3 probe) has all pieces of one sign: on all-positive data every dropped product pulls the same way
// and the median relative error was 1.6e-7 against 5e-8 for the fp32 MFMA (tests/test_x6_gpu.py all_positive); same instruction count.
__device__ __forceinline__ uint32_t cvt_pk_bf16(float x0, float x1) {                // {bf16(x0), bf16(x1)} in one dword, element 0 in the low half
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
}
// two fp32 values -> one dword of each of the three planes
__device__ __forceinline__ void split_pack2(float x0, float x1, uint32_t &p1, uint32_t &p2, uint32_t &p3) {
    p1 = cvt_pk_bf16(x0, x1);
    const float r0 = x0 - __uint_as_float(p1 << 16), r1 = x1 - __uint_as_float(p1 & 0xffff0000u);
    p2 = cvt_pk_bf16(r0, r1);
    const float s0 = r0 - __uint_as_float(p2 << 16), s1 = r1 - __uint_as_float(p2 & 0xffff0000u);
    p3 = cvt_pk_bf16(s0, s1);
}
// ONE fp32 value -> its bf16 of each plane: the low half of split_pack2(x, 0), bit for bit (x6_img_put refreshes the forward's weight image one
// parameter at a time).  Kept beside the pair form instead of calling it: the unused high half's subtractions would have to be removed by the
// compiler, and the image hand-over must not depend on that.
__device__ __forceinline__ void split_pack1(float x, uint16_t &p1, uint16_t &p2, uint16_t &p3) {
    p1 = (uint16_t)(cvt_pk_bf16(x, 0.0f) & 0xffffu);
    const float r = x - __uint_as_float((uint32_t)p1 << 16);
    p2 = (uint16_t)(cvt_pk_bf16(r, 0.0f) & 0xffffu);
    const float s = r - __uint_as_float((uint32_t)p2 << 16);
    p3 = (uint16_t)(cvt_pk_bf16(s, 0.0f) & 0xffffu);
}
// four consecutive fp32 values -> dwords d, d + 1 of the three plane fragments
__device__ __forceinline__ void split_pack4(const f32x4 v, Frag (&f)[3], int d) {
    split_pack2(v[0], v[1], f[0].u[d], f[1].u[d], f[2].u[d]);
    split_pack2(v[2], v[3], f[0].u[d + 1], f[1].u[d + 1], f[2].u[d + 1]);
}
// four consecutive fp32 values -> 8 bytes of each of the three plane images, `plane_bytes` apart, at the LDS byte address `addr`
__device__ __forceinline__ void split_write4(uint32_t addr, int plane_bytes, const f32x4 v) {
    uint32_t a[3], b[3];
    split_pack2(v[0], v[1], a[0], a[1], a[2]);
    split_pack2(v[2], v[3], b[0], b[1], b[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<lds_u32x2 *>((uintptr_t)(addr + (uint32_t)(p * plane_bytes))) = u32x2{a[p], b[p]};
}
// the same through a generic pointer (linear_x6.hip's weight staging computes its destinations as pointers into the shared array; the compiler
// proves the address space itself, and rewriting the caller onto byte addresses changes its instruction stream)
__device__ __forceinline__ void split_put4(uint8_t *dst, int plane_bytes, const f32x4 v) {
    uint32_t a[3], b[3];
    split_pack2(v[0], v[1], a[0], a[1], a[2]);
    split_pack2(v[2], v[3], b[0], b[1], b[2]);
#pragma unroll
    for (int p = 0; p < 3; ++p) *reinterpret_cast<u32x2 *>(dst + (size_t)p * plane_bytes) = u32x2{a[p], b[p]};
}

// ---- the transpose-read: the fragment of tile t (16 features x 32 rows) of a [row][feature] bf16 plane image (planes `plane_bytes`, rows
// `row_bytes` apart).  img_lane = the image's LDS byte address + this lane's chunk (row 4 g + (j >> 2), 8 bytes (j & 3), whatever swizzle the
// image uses); lane (j, g) receives feature 16 t + j, k slot (g, e): e < 4 row 4 g + e, e >= 4 row 16 + 4 g + e - 4 (ds_read_b64_tr_b16 twice per plane)
__device__ __forceinline__ void read_tr(Frag (&f)[3], uint32_t img_lane, int plane_bytes, int row_bytes, int t) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_i16x4 *>((uintptr_t)(img_lane + (uint32_t)(p * plane_bytes + 32 * t))));
        const i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<lds_i16x4 *>((uintptr_t)(img_lane + (uint32_t)(p * plane_bytes + 32 * t + 16 * row_bytes))));
        const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
        f[p].u[0] = l2[0]; f[p].u[1] = l2[1]; f[p].u[2] = h2[0]; f[p].u[3] = h2[1];
    }
}

// ---- the six products of one fp32 product, SMALL TERMS FIRST: product q multiplies plane kSixA[q] of A by plane kSixB[q] of B
// (a1 b3, a2 b2, a3 b1 | a1 b2, a2 b1 | a1 b1).  Kernels that interleave the products of several accumulators (scorer_x6.hip, linear_x6.hip)
// and the 16-deep tails walk the table themselves; everything else calls mma6.
constexpr int kSixA[6] = {0, 1, 2, 0, 1, 0}, kSixB[6] = {2, 1, 0, 1, 0, 0};
// c += A * B for one 16 x 16 tile and one 32-deep contraction slice
__device__ __forceinline__ void mma6(f32x4 &c, const Frag (&a)[3], const Frag (&b)[3]) {
#pragma unroll
    for (int q = 0; q < 6; ++q) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kSixA[q]].v, b[kSixB[q]].v, c, 0, 0, 0);
}

}  // namespace ptr
