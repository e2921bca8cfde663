// Robust_Sigmoid (ptranking/base/utils.py:57-95) of an unordered pair — shared by the smooth-rank pair loops of ApproxNDCG
// (approxndcg.hip) and of the alpha-DCG loss (diversity.hip).
#pragma once
#include "ptr_device.h"

namespace ptr {
#if defined(__HIPCC__)

// Both Robust_Sigmoid values of an unordered pair from one exponential.
// delta = s_b - s_a.  ya = rs(alpha*delta) (contribution of b to pi_hat_a), yb = rs(-alpha*delta).
__device__ __forceinline__ void robust_pair(float delta, float alpha, float &ya, float &yb) {
    const float x = alpha * fabsf(delta);
    const float e = __expf(-x);
    const float dd = 1.0f + e;
    float r = __builtin_amdgcn_rcpf(dd);
    r = fmaf(r, fmaf(-dd, r, 1.0f), r);          // 1/(1+e)      (base/utils.py:71)
    const float sm = e * r;                       // e/(1+e)      (base/utils.py:73-74)
    const bool pos = delta > 0.0f, neg = delta < 0.0f;
    ya = pos ? r : (neg ? sm : 0.5f);
    yb = pos ? sm : (neg ? r : 0.5f);
}

#endif  // __HIPCC__
}  // namespace ptr
