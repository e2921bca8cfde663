// What the two families of attention kernels of the listwise scorer share: the narrow forms (listsf.hip, head dimension <= 128, the
// whole head in registers) and the wide forms (listsf_wide.hip, 128 < head dimension <= PTR_MHSA_MAX_HEAD_DIM).  Layouts and the MFMA
// formulation are described at the top of listsf.hip.
#pragma once
#include "ptr_device.h"
#include "ptr_dropout.h"

namespace ptr {

constexpr int kAttnNarrowMaxHeadDim = 128;   // widest head of the narrow forms (dispatch_dt: D = ceil(dh / 16) <= 8)
constexpr int kDsPadLd = 20;           // row stride (floats) of the dS transpose pad: 16-byte aligned rows, 80 B = 20 banks apart

struct AttnArgs {
    int B, L, H, dh, F;
    int ld;                            // row stride (floats) of Q / K / V and dQ / dK / dV: F, or 3F for a packed [B][L][3F] projection
    float inv_scale;                   // 1 / sqrt(dh)
    float p_drop;
    uint32_t seed_lo, seed_hi;
    int site;
};

// LDS leading dimension for a [rows][dh] tile: covers the 16*DT columns the d-tiles touch, ld/4 odd (conflict-free b128)
__host__ __device__ constexpr int attn_ld(int DT) { return ((16 * DT / 4) & 1) ? 16 * DT : 16 * DT + 4; }

// Workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  The row (key) blocks of one (query, head) re-read the
// same K / V (Q / dO) rows, so consecutive LOGICAL block ids are placed on the same XCD: logical = xcd * (n / 8) + slot.
__device__ __forceinline__ int xcd_major_block_id() {
    const int n = gridDim.x, b = blockIdx.x;
    return (n & 7) == 0 ? (b & 7) * (n >> 3) + (b >> 3) : b;
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ float xor_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float xor_sum(float v) {
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

// The kernel form of ptr_mhsa_forward / ptr_mhsa_backward.  Narrow (dh <= 128): D = ceil(dh / 16) column tiles, the whole head in registers;
// two row tiles per forward wave (every K / V operand read feeds two MFMAs) when the rows exist and the registers allow it; 4 waves per
// workgroup (two workgroups share a CU, one's barrier / staging phases covered by the other's MFMA work) except the dK / dV kernel of the
// widest heads, whose 4-wave form spills more.  Wide: D = column tiles rounded up to even, one form per 32 columns of head dimension (10 .. 22).
// store_ds: a dS scratch was passed, so dK / dV stores dS and dQ is one GEMM from it; else dQ and dK / dV both recompute.
struct AttnForm { int wide; int D; int fwd_row_tiles; int dkv_waves; int store_ds; };
inline AttnForm attn_form(int dh, int L, bool store_ds) {
    if (dh > kAttnNarrowMaxHeadDim) return {1, 2 * ((dh + 31) / 32), 1, 4, store_ds};
    const int D = (dh + 15) / 16;
    return {0, D, D <= 5 && L > 64 ? 2 : 1, D >= 7 && L > 64 ? 8 : 4, store_ds};
}

// Floats per global access of a head's rows, which each kernel picks for each array it touches.  Narrow: 4 when the head dimension and the
// row stride are multiples of 4 and the array is 16-byte aligned, else 1 (a macro: the narrow kernels come out of the compiler with another
// register allocation when this is a function).  Wide: the same, and 2 when they are even and the array is 8-byte aligned.
#define ATTN_FLOAT4_ROWS(dh, stride, p) (((dh & 3) == 0) && ((stride & 3) == 0) && ((reinterpret_cast<uintptr_t>(p) & 15) == 0))
__host__ __device__ inline int wide_access_width(int dh, int stride, uintptr_t address) {
    if (((dh | stride) & 3) == 0 && (address & 15) == 0) return 4;
    if (((dh | stride) & 1) == 0 && (address & 7) == 0) return 2;
    return 1;
}

// LayerNorm: NI = ceil(F / 64) values per lane in registers (1 .. 4; 0 = the generic form), one row per wave and four per workgroup, which
// walk the rows with a grid stride; the backward keeps one partial of d a_2, d b_2 per workgroup (ptr_layernorm_backward_ws_floats).
constexpr int kLnBlocks = 1024;
struct LnForm { int NI; int fwd_blocks; int bwd_blocks; };
inline LnForm layernorm_form(int64_t R, int F) {
    const int64_t want = (R + 3) / 4 > 0 ? (R + 3) / 4 : 1;
    const int ni = (F + 63) / 64;
    return {ni <= 4 ? ni : 0, (int)(want < 8192 ? want : 8192), (int)(want < kLnBlocks ? want : kLnBlocks)};
}

// The wide forms (listsf_wide.hip), entered by ptr_mhsa_forward / ptr_mhsa_backward for attn_form(..).wide with its D.  The backward expects
// Dv = rowdot(O, dO) already queued on `st`.
int mhsa_wide_forward(int DT, const float *Q, const float *K, const float *V, const int32_t *lens, const AttnArgs &a, float *O, float *LSE,
                      hipStream_t st, const char *who);
int mhsa_wide_backward(int DT, const float *Q, const float *K, const float *V, const float *dO, const float *LSE, const float *Dv,
                       const int32_t *lens, const AttnArgs &a, float *dQ, float *dK, float *dV, float *ds_ws, hipStream_t st, const char *who);

}  // namespace ptr
