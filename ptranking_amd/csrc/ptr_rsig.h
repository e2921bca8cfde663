// Robust_Sigmoid (ptranking/base/utils.py:57-95) of an unordered pair — shared by the smooth-rank pair loops of ApproxNDCG
// (approxndcg.hip), of the smooth-rank metric objectives (smoothmetric.hip) and of the alpha-DCG loss (diversity.hip): the scalar pair
// (robust_pair) and the one-wavefront register ring over all pairs of a query (approx_ring).
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
    const float r = rcp_nr(dd);                   // 1/(1+e)      (base/utils.py:71)
    const float sm = e * r;                       // e/(1+e)      (base/utils.py:73-74)
    const bool pos = delta > 0.0f, neg = delta < 0.0f;
    ya = pos ? r : (neg ? sm : 0.5f);
    yb = pos ? sm : (neg ? r : 0.5f);
}

// The register ring of approxndcg_ring_kernel (approxndcg.hip) and smooth_ring_kernel (smoothmetric.hip), list lengths up to 512: ONE
// wavefront per query, both O(L^2) passes out of registers — the scheme of lambdarank_ring_kernel (pairwise.hip).  PASS 1: out = sum_{j != i}
// y_ij; PASS 2: out = the gradient from the coefficients c.  Lane a owns documents a, a+64, ... in INPUT order (nothing in the loss depends on the ideal
// ORDER, only the IDCG does: a value-only sort of the labels, or the labels as they are under `presort`); every own record {s} / {s, c}
// stays put, every slot has two travelling copies {s, acc} / {s, c, acc} (the records 1..16 and 17..32 lanes ahead, one packed
// instruction stream for both), rotated one lane per step with v_mov_b32_dpp wave_rol:1.  The partner's share of a pair accumulates in the
// travelling record instead of an LDS read-modify-write, and the partner's score / coefficient arrive by rotation instead of LDS reads:
// per pair and pass ~10 / ~15 VALU slots against ~23 / ~30 of approxndcg_kernel.  Padding slots carry s = -1e30, c = 0: e = 0, y in
// {0, 1}, y(1-y) = 0 — every pair with a padding record contributes exactly 0 to real documents (scores are assumed far above -1e30).
template <int DPT, int PASS>
__device__ __forceinline__ void approx_ring(const float (&s)[DPT], const float (&c)[DPT], float c2, float alpha, int lane, float (&out)[DPT]) {
    f32x2 so2[DPT], co2[DPT], acc2[DPT];                          // own records {v, v}; own accumulators of the two copies
    f32x2 Ts[DPT], Tc[DPT], Ta[DPT];                              // travelling {copy A, copy B}
    const int ahead16 = (lane + 16) & 63;
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
        so2[k] = f32x2{s[k], s[k]};
        Ts[k] = f32x2{s[k], __shfl(s[k], ahead16, 64)};
        acc2[k] = f32x2{0.f, 0.f}; Ta[k] = f32x2{0.f, 0.f};
        if constexpr (PASS == 2) { co2[k] = f32x2{c[k], c[k]}; Tc[k] = f32x2{c[k], __shfl(c[k], ahead16, 64)}; }
    }
    const f32x2 c22 = {c2, c2}, one2 = {1.0f, 1.0f}, al2 = {alpha, alpha};
    auto pair2 = [&](int k, int t, f32x2 mask, bool use_mask) __attribute__((always_inline)) {
        // Robust_Sigmoid (base/utils.py:57-95) of +-alpha*delta from ONE exponential, as robust_pair(): r = 1/(1+e), sm = e/(1+e)
        const f32x2 dl = pk_sub(Ts[t], so2[k]);                   // delta = s_b - s_a
        const f32x2 x = dl * c22;                                 // alpha*log2(e) folded
        const f32x2 e = {__builtin_amdgcn_exp2f(-fabsf(x.x)), __builtin_amdgcn_exp2f(-fabsf(x.y))};
        const f32x2 dd = one2 + e;      // compiler-emitted: an inline-asm reader right behind v_exp_f32 would miss the trans-use wait state
        f32x2 r = {__builtin_amdgcn_rcpf(dd.x), __builtin_amdgcn_rcpf(dd.y)};
        r = __builtin_elementwise_fma(r, __builtin_elementwise_fma(-dd, r, one2), r);
        const f32x2 sm = e * r;
        f32x2 ya, yb;                                             // delta == 0: e = 1, r = sm = 0.5 on its own
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool pos = dl[h] > 0.0f;
            ya[h] = pos ? r[h] : sm[h];
            yb[h] = pos ? sm[h] : r[h];
        }
        if constexpr (PASS == 1) {
            if (use_mask) { ya = ya * mask; yb = yb * mask; }
            acc2[k] = pk_add(acc2[k], ya);                        // b's contribution to pi_hat_a
            Ta[t] = pk_add(Ta[t], yb);                            // a's contribution to pi_hat_b
        } else {
            const f32x2 dab = (ya * al2) * pk_sub(one2, ya), dba = (yb * al2) * pk_sub(one2, yb);      // base/utils.py:78
            f32x2 flow = __builtin_elementwise_fma(-co2[k], dab, Tc[t] * dba);                         // d loss / d s_a from this pair
            if (use_mask) flow = flow * mask;
            acc2[k] = pk_add(acc2[k], flow);
            Ta[t] = pk_sub(Ta[t], flow);
        }
    };
    auto rotate = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < DPT; ++t)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                Ts[t][h] = dpp_rol1(Ts[t][h]); Ta[t][h] = dpp_rol1(Ta[t][h]);
                if constexpr (PASS == 2) Tc[t][h] = dpp_rol1(Tc[t][h]);
            }
    };
    // offset 0: pairs inside a lane (travelling slot t > own slot k), copy A only
#pragma unroll
    for (int k = 0; k < DPT; ++k)
#pragma unroll
        for (int t = k + 1; t < DPT; ++t) pair2(k, t, f32x2{1.0f, 0.0f}, true);
    // steps 1..15: lane offsets r (copy A) and r + 16 (copy B)
    for (int r = 1; r < 16; ++r) {
        rotate();
#pragma unroll
        for (int k = 0; k < DPT; ++k)
#pragma unroll
            for (int t = 0; t < DPT; ++t) pair2(k, t, one2, false);
    }
    // step 16: offset 16 (A) and the half step 32 (B), where lanes a and a+32 see each other from both ends — the lower half keeps them
    {
        rotate();
        const float lm = lane < 32 ? 1.0f : 0.0f;
#pragma unroll
        for (int k = 0; k < DPT; ++k)
#pragma unroll
            for (int t = 0; t < DPT; ++t) pair2(k, t, f32x2{1.0f, lm}, true);
    }
    // the travelling accumulators sit 16 (copy A) / 32 (copy B) lanes behind their owners
    const int behind16 = (lane - 16) & 63;
#pragma unroll
    for (int k = 0; k < DPT; ++k) out[k] = (acc2[k].x + acc2[k].y) + (__shfl(Ta[k].x, behind16, 64) + __shfl(Ta[k].y, lane ^ 32, 64));
}

#endif  // __HIPCC__
}  // namespace ptr
