// What the adversarial frame's kernels share (irgan.hip, irfgan.hip, adlist.hip): the stable softplus family, the f-divergences' a(v) and
// c(v) in closed form, the group helpers of the samplers (any, arg-max, the V largest keys, prefix sums into LDS, the inverse-CDF search)
// and the argument checks.  The header of irgan.hip states the
// sampling rules these helpers implement.
#pragma once
#include <limits.h>

#include "ptr_device.h"

namespace ptr {

inline int ig_check_shape(const char *who, int B, int L, float temperature) {
    if (B < 0 || L <= 0) { set_error("%s: bad shape B=%d L=%d", who, B, L); return PTR_ERR_INVALID_ARG; }
    if (L > PTR_MAX_LIST_LEN) { set_error("%s: list length %d exceeds PTR_MAX_LIST_LEN=%d", who, L, PTR_MAX_LIST_LEN); return PTR_ERR_INVALID_ARG; }
    if (!(temperature > 0.0f) || !(temperature < INFINITY)) { set_error("%s: temperature must be a finite number > 0 (got %g)", who, (double)temperature); return PTR_ERR_INVALID_ARG; }
    return 0;
}
inline int ig_check_samples(const char *who, int S) {
    if (S < 1 || S > PTR_IRGAN_MAX_SAMPLES) { set_error("%s: samples per query must be in 1 .. %d (got %d)", who, PTR_IRGAN_MAX_SAMPLES, S); return PTR_ERR_INVALID_ARG; }
    return 0;
}

#if defined(__HIPCC__)

__device__ __forceinline__ float ig_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float ig_logsigmoid(float x) { return -ig_softplus(-x); }
__device__ __forceinline__ float ig_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// a(v) = activation_f(v) and its derivative (util/f_divergence.py)
__device__ __forceinline__ void fg_act(int f, float v, float &a, float &da) {
    switch (f) {
        case PTR_FDIV_TVAR: {
            const float e = expf(-2.0f * fabsf(v)), d = 1.0f + e;
            a = 0.5f * tanhf(v);
            da = 2.0f * e / (d * d);                                         // 0.5 sech^2 v without the cancellation of 1 - tanh^2
            break;
        }
        case PTR_FDIV_KL: case PTR_FDIV_PC: a = v; da = 1.0f; break;
        case PTR_FDIV_RKL: da = expf(-v); a = -da; break;
        case PTR_FDIV_NC: case PTR_FDIV_SH: a = -expm1f(-v); da = expf(-v); break;
        case PTR_FDIV_JS: a = 0.69314718055994531f - ig_softplus(-v); da = ig_sigmoid(-v); break;
        default: a = -ig_softplus(-v); da = ig_sigmoid(-v); break;           // PTR_FDIV_GAN
    }
}
// c(v) = conjugate_f(activation_f(v)) in closed form and its derivative; the composition cancels or overflows in fp32 long before these do
// (GAN: -log(1 - exp(-softplus(-v))) is inf from v = 17 on, where softplus(v) is v)
__device__ __forceinline__ void fg_conj(int f, float v, float &c, float &dc) {
    switch (f) {
        case PTR_FDIV_TVAR: {
            const float e = expf(-2.0f * fabsf(v)), d = 1.0f + e;
            c = 0.5f * tanhf(v);
            dc = 2.0f * e / (d * d);
            break;
        }
        case PTR_FDIV_KL: c = expf(v - 1.0f); dc = c; break;
        case PTR_FDIV_RKL: c = v - 1.0f; dc = 1.0f; break;
        case PTR_FDIV_PC: c = 0.25f * v * v + v; dc = 0.5f * v + 1.0f; break;
        case PTR_FDIV_NC: c = -2.0f * expm1f(-0.5f * v); dc = expf(-0.5f * v); break;
        case PTR_FDIV_SH: c = expm1f(v); dc = expf(v); break;
        case PTR_FDIV_JS: c = ig_softplus(v) - 0.69314718055994531f; dc = ig_sigmoid(v); break;
        default: c = ig_softplus(v); dc = ig_sigmoid(v); break;              // PTR_FDIV_GAN
    }
}

template <int G> __device__ __forceinline__ bool group_any(bool v, int *red, int t) {
    if constexpr (G == kWave) {
        (void)red; (void)t;
        return __any(v) != 0;
    } else {
        return __syncthreads_or(v) != 0;
    }
}

// (key descending, index ascending) over the G threads; every thread gets the winner.  `red`: 8 words of LDS (G == 256).
template <int G> __device__ __forceinline__ void group_argmax(float &key, int &idx, float *red, int t) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ok = __shfl_xor(key, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        if (ok > key || (ok == key && oi < idx)) { key = ok; idx = oi; }
    }
    if constexpr (G != kWave) {
        int *redi = reinterpret_cast<int *>(red) + 4;
        __syncthreads();
        if ((t & 63) == 0) { red[t >> 6] = key; redi[t >> 6] = idx; }
        __syncthreads();
        key = red[0];
        idx = redi[0];
#pragma unroll
        for (int w = 1; w < G / kWave; ++w) {
            const float ok = red[w];
            const int oi = redi[w];
            if (ok > key || (ok == key && oi < idx)) { key = ok; idx = oi; }
        }
    }
}

// V rounds of arg-max over K[0..n): out[k] = the k-th document in (key descending, index ascending); a taken key becomes -inf.
// A round without a finite key left (scores of -inf) names document 0.
template <int G> __device__ __forceinline__ void take_largest(float *K, int n, int V, int64_t *out, float *red, int t) {
    for (int k = 0; k < V; ++k) {
        float best = -INFINITY;
        int bi = INT_MAX;
        for (int i = t; i < n; i += G) {
            const float v = K[i];
            if (v > best) { best = v; bi = i; }                              // ascending walk: the first of equal keys stays
        }
        group_argmax<G>(best, bi, red, t);
        if (t == 0) {
            out[k] = bi < n ? (int64_t)bi : 0;
            if (bi < n) K[bi] = -INFINITY;
        }
        group_sync<G>();
    }
}

// C[i] = inclusive prefix sum of w(i) over the documents 0..n), tile by tile in thread order; returns C[n - 1] (0 for n == 0).
template <int G, class W> __device__ __forceinline__ float prefix_into(float *C, int n, float *red, int t, W &&w) {
    float carry = 0.0f;
    for (int base = 0; base < n; base += G) {
        const int i = base + t;
        const float v = i < n ? w(i) : 0.0f;
        const float ex = grp_excl_prefix<G>(v, red, t);
        if (i < n) C[i] = carry + (ex + v);
        carry += group_sum<G>(v, red, t);
    }
    group_sync<G>();
    return n > 0 ? C[n - 1] : 0.0f;
}

// the with-replacement rule of irgan.hip's header: C the prefix sums, x = u * C[n - 1], `zero(i)` true where w_i == 0
template <class Z> __device__ __forceinline__ int inverse_cdf(const float *C, int n, float x, Z &&zero) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x < C[mid]) hi = mid; else lo = mid + 1;
    }
    while (lo > 0 && zero(lo)) --lo;
    return lo;
}

#endif  // __HIPCC__

}  // namespace ptr
