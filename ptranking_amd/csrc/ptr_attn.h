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

// The wide forms (listsf_wide.hip), entered by ptr_mhsa_forward / ptr_mhsa_backward for dh > kAttnNarrowMaxHeadDim.  The backward expects
// Dv = rowdot(O, dO) already queued on `st`.
int mhsa_wide_forward(const float *Q, const float *K, const float *V, const int32_t *lens, const AttnArgs &a, float *O, float *LSE,
                      hipStream_t st, const char *who);
int mhsa_wide_backward(const float *Q, const float *K, const float *V, const float *dO, const float *LSE, const float *Dv,
                       const int32_t *lens, const AttnArgs &a, float *dQ, float *dK, float *dV, float *ds_ws, hipStream_t st, const char *who);

}  // namespace ptr
