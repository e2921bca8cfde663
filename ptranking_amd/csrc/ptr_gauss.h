// The Gaussian pair of two documents with independent normal scores (ptranking/ltr_diversification/util/prob_utils.py:5-26, :62-80) —
// shared by DivProbRanker's objectives (divprob.hip) and by the expected-rank metric objectives (gaussmetric.hip):
//   a = 1 / sqrt(2 (v_i + v_j))     x = (m_i - m_j) a     Phi = erfc(x) / 2     phi = exp(-x^2) / sqrt(pi)
#pragma once
#include "ptr_device.h"

namespace ptr {
#if defined(__HIPCC__)

// 1 / sqrt(z): v_rsq_f32 and one Newton step (the pair argument x carries its error into erfc at relative weight ~ 2 x^2)
__device__ __forceinline__ float inv_sqrt(float z) {
    const float r = __builtin_amdgcn_rsqf(z);
    return fmaf(0.5f * r, fmaf(-z * r, r, 1.0f), r);
}
// a / b from v_rcp_f32 and one Newton step
__device__ __forceinline__ float quot(float a, float b) { return a * rcp_nr(b); }

// The pair (i, j) seen from document i.  x is clamped to +-1e18 so that x^2 stays finite (beyond |x| ~ 13 every quantity below is at
// its limit anyway).  sq_hi + sq_lo = x^2 exactly; e2 = exp(-x^2) with the rounding of x^2 taken out.
struct PairGeo { float a, x, sq_hi, sq_lo, e2; };
__device__ __forceinline__ PairGeo pair_geo(float mi, float vi, float mj, float vj) {
    PairGeo g;
    g.a = inv_sqrt(2.0f * (vi + vj));
    g.x = __builtin_amdgcn_fmed3f((mi - mj) * g.a, -1e18f, 1e18f);
    g.sq_hi = g.x * g.x;
    g.sq_lo = fmaf(g.x, g.x, -g.sq_hi);
    const float e = expf(-g.sq_hi);
    g.e2 = fmaf(-g.sq_lo, e, e);
    return g;
}
// Phi = erfc(x) / 2 through the scaled complementary error function: the tail exp(-x^2) erfcx(|x|) / 2 keeps its relative precision
__device__ __forceinline__ float pair_phi(const PairGeo &g) {
    const float tail = 0.5f * g.e2 * erfcxf(fabsf(g.x));
    return g.x >= 0.0f ? tail : 1.0f - tail;
}

constexpr float kInvSqrtPi = 0.5641895835477563f;

#endif  // __HIPCC__
}  // namespace ptr
