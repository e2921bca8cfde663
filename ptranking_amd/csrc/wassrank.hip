// WassRank (ptranking/ltr_adhoc/listwise/wassrank/wassRank.py:43-88, mode 'SinkhornOT', smooth_type 'ST', norm_type 'BothST'): the
// entropic Wasserstein distance between a = softmax(m * preds) and b = softmax(labels) under a label/position cost C, evaluated with
// log-domain Sinkhorn iterations (pytorch_wasserstein.py:323-393), and its gradient pushed through the softmax — one workgroup per query,
// every iteration and the backward inside one launch.
//
// Numerics.  The reference shifts each K-matvec by ONE maximum per query (log_u_max / log_v_max) and takes log(K @ exp(v - max v)); when
// every term of a row lies far below that shift, the row sum underflows to 0 and log(0) turns the loss and gradient into NaN in fp32.  Here
// every log-sum-exp takes the maximum of ITS OWN row (two passes over the row: max, then sum of exp2(t - max) >= 1), which is the same
// mathematics and finite whenever the inputs are.  The iteration runs in base-2 units (every log quantity times log2(e), C/lam folded into
// s = log2(e)/lam) so that each term is one fma and one v_exp_f32.
//
// Cost C_ij (wasserstein_cost_mat.py:47-139) is recomputed from a per-document key in LDS, never loaded: C is symmetric for every cost type,
// so the v-step (LSE over i of u_i - C_ij/lam) and the u-step (LSE over j of v_j - C_ij/lam) are the same row operation.
//
// Work: (2 sh_itr + 1) passes of n^2 terms per query; each LSE pass reads the row twice (max, sum), each term one v_exp_f32.  Every reduction
// has a fixed order and there are no atomics: run-to-run bit-stable.
#include <math.h>

#include "ptr_device.h"

namespace ptr {

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// C_ij from the keys of documents i and j (ki, di: document i; kj, dj: document j).  K holds |position| (p1, p2), the gap-adjusted gain
// (eg) or 2^y - 1 (dg, ddg); D holds 1/log2(position + 2) (ddg only).
template <int COST>
__device__ __forceinline__ float wass_cost(float ki, float kj, float di, float dj, int i, int j, float vp) {
    const float d = fabsf(ki - kj);
    if constexpr (COST == PTR_WASS_COST_P1) {
        return d;
    } else if constexpr (COST == PTR_WASS_COST_P2) {
        return d * d;
    } else if constexpr (COST == PTR_WASS_COST_EG) {
        const float c = d < 1.0f ? vp : d;          // any pair closer than 1 (not only equal labels) costs var_penalty
        return i == j ? 0.0f : c;                   // ... except the diagonal
    } else if constexpr (COST == PTR_WASS_COST_DG) {
        return d;
    } else {
        return d * fabsf(di - dj);
    }
}

// out[j] = base[j] - LSE2_i(in[i] - s * C_ij) for every real document j (< n).  `in` is padded with -inf up to n4 = round_up(n, 4), K and D
// with 0, so the padded terms are exp2(-inf) = 0.  Thread t owns the columns j = j0 + d*G + t of each tile of G*DPT columns.
template <int COST, int G, int DPT>
__device__ __forceinline__ void lse_rows(const float *in, const float *base, float *out, const float *K, const float *D, int n, int n4, int t,
                                         float s, float vp) {
    for (int j0 = 0; j0 < n; j0 += G * DPT) {
        if (j0 + (t & ~63) >= n) continue;          // wave-uniform: every column of this wave is padding
        int jj[DPT];
        float kj[DPT], dj[DPT], mx[DPT];
#pragma unroll
        for (int d = 0; d < DPT; ++d) {
            const int j = j0 + d * G + t;
            jj[d] = j < n ? j : n - 1;
            kj[d] = K[jj[d]];
            dj[d] = COST == PTR_WASS_COST_DDG ? D[jj[d]] : 0.0f;
            mx[d] = -INFINITY;
        }
        for (int i = 0; i < n4; i += 4) {
            const float4 x = *reinterpret_cast<const float4 *>(in + i);
            const float4 k = *reinterpret_cast<const float4 *>(K + i);
            float4 dd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if constexpr (COST == PTR_WASS_COST_DDG) dd = *reinterpret_cast<const float4 *>(D + i);
            const float xs[4] = {x.x, x.y, x.z, x.w}, ks[4] = {k.x, k.y, k.z, k.w}, ds[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int d = 0; d < DPT; ++d)
                    mx[d] = fmaxf(mx[d], fmaf(-wass_cost<COST>(ks[u], kj[d], ds[u], dj[d], i + u, jj[d], vp), s, xs[u]));
        }
        float acc[DPT][4];
#pragma unroll
        for (int d = 0; d < DPT; ++d)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[d][u] = 0.0f;
        for (int i = 0; i < n4; i += 4) {
            const float4 x = *reinterpret_cast<const float4 *>(in + i);
            const float4 k = *reinterpret_cast<const float4 *>(K + i);
            float4 dd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if constexpr (COST == PTR_WASS_COST_DDG) dd = *reinterpret_cast<const float4 *>(D + i);
            const float xs[4] = {x.x, x.y, x.z, x.w}, ks[4] = {k.x, k.y, k.z, k.w}, ds[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int d = 0; d < DPT; ++d)
                    acc[d][u] += fast_exp2(fmaf(-wass_cost<COST>(ks[u], kj[d], ds[u], dj[d], i + u, jj[d], vp), s, xs[u]) - mx[d]);
        }
#pragma unroll
        for (int d = 0; d < DPT; ++d) {
            const int j = j0 + d * G + t;
            const float sum = (acc[d][0] + acc[d][1]) + (acc[d][2] + acc[d][3]);     // >= 1: the maximum's own term is exp2(0)
            if (j < n) out[j] = base[j] - (mx[d] + fast_log2(sum));
        }
    }
}

// log2 of softmax(x) over the n real entries of `v` (already in LDS), written in place; returns nothing, ends with a barrier.
template <int G>
__device__ __forceinline__ void log2_softmax_inplace(float *v, int n, int t, float *red) {
    float m = -INFINITY;
    for (int i = t; i < n; i += G) m = fmaxf(m, v[i]);
    m = group_max<G>(m, red, t);
    float s = 0.0f;
    for (int i = t; i < n; i += G) s += fast_exp2((v[i] - m) * kLog2e);
    s = group_sum<G>(s, red + 4, t);
    const float ls = fast_log2(s);
    for (int i = t; i < n; i += G) v[i] = (v[i] - m) * kLog2e - ls;
    __syncthreads();
}

// One workgroup of G threads per query.  LDS (floats, Lp = round_up(L, 4)): A = log2 a, Bh = log2 b, U = log2 u, V = log2 v, K = cost key,
// D = ddg discount, each Lp long, then 8 reduction slots.
template <int COST, int G, int DPT>
__global__ void __launch_bounds__(G)
wassrank_kernel(const float *__restrict__ preds, const float *__restrict__ labels, const int32_t *__restrict__ lens, int L, int Lp,
                float gain_base, float non_rele_gap, float var_penalty, float lam, int sh_itr, int scale_by_max_label, float inv_b,
                float *__restrict__ loss_q, float *__restrict__ grad) {
    extern __shared__ float lds[];
    float *A = lds, *Bh = A + Lp, *U = Bh + Lp, *V = U + Lp, *K = V + Lp, *D = K + Lp, *red = D + Lp;
    const int q = blockIdx.x, t = threadIdx.x;
    const int n = query_len(lens, q, L);
    const float *ps = preds + (size_t)q * L, *ys = labels + (size_t)q * L;
    float *g = grad + (size_t)q * L;
    if (n <= 1) {                                   // one document (or none): a = b = 1, C = 0, loss 0, gradient 0
        for (int i = t; i < L; i += G) g[i] = 0.0f;
        if (t == 0) loss_q[q] = 0.0f;
        return;
    }
    const int n4 = (n + 3) & ~3;

    // labels -> b (in Bh), the per-query maximum label, the cost keys
    float ymax = -INFINITY;
    for (int i = t; i < n4; i += G) {
        const float y = i < n ? ys[i] : 0.0f;
        if (i < n) ymax = fmaxf(ymax, y);
        float k;
        if constexpr (COST == PTR_WASS_COST_P1 || COST == PTR_WASS_COST_P2) {
            k = (float)i;
        } else if constexpr (COST == PTR_WASS_COST_EG) {
            const float gn = powf(gain_base, y) - 1.0f;
            k = gn < 1.0f ? -non_rele_gap : gn;
        } else {
            k = exp2f(y) - 1.0f;
        }
        K[i] = i < n ? k : 0.0f;
        D[i] = (COST == PTR_WASS_COST_DDG && i < n) ? 1.0f / log2f((float)i + 2.0f) : 0.0f;
        Bh[i] = y;
    }
    ymax = group_max<G>(ymax, red, t);
    const float m = scale_by_max_label ? ymax : 1.0f;
    for (int i = t; i < n; i += G) A[i] = m * ps[i];
    __syncthreads();
    log2_softmax_inplace<G>(Bh, n, t, red);
    log2_softmax_inplace<G>(A, n, t, red);

    // Sinkhorn: log u = log v = -log n; then sh_itr times the v-step and the u-step
    const float init = -fast_log2((float)n);
    for (int i = t; i < n4; i += G) {
        U[i] = i < n ? init : -INFINITY;
        V[i] = i < n ? init : -INFINITY;
    }
    __syncthreads();
    const float s = kLog2e / lam;
    for (int it = 0; it < sh_itr; ++it) {
        lse_rows<COST, G, DPT>(U, Bh, V, K, D, n, n4, t, s, var_penalty);
        __syncthreads();
        lse_rows<COST, G, DPT>(V, A, U, K, D, n, n4, t, s, var_penalty);
        __syncthreads();
    }

    // loss_q = sum_ij C_ij exp(log u_i - C_ij / lam + log v_j): thread t owns the columns j, fixed order over i, then the group sum
    float part = 0.0f;
    for (int j = t; j < n; j += G) {
        const float kj = K[j], dj = D[j], vj = V[j];
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int i = 0; i < n4; i += 4) {
            const float4 x = *reinterpret_cast<const float4 *>(U + i);
            const float4 k = *reinterpret_cast<const float4 *>(K + i);
            float4 dd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if constexpr (COST == PTR_WASS_COST_DDG) dd = *reinterpret_cast<const float4 *>(D + i);
            const float xs[4] = {x.x, x.y, x.z, x.w}, ks[4] = {k.x, k.y, k.z, k.w}, ds[4] = {dd.x, dd.y, dd.z, dd.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float c = wass_cost<COST>(ks[u], kj, ds[u], dj, i + u, j, var_penalty);
                acc[u] = fmaf(c, fast_exp2(fmaf(-c, s, xs[u]) + vj), acc[u]);
            }
        }
        part += (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
    const float loss = group_sum<G>(part, red, t);

    // gradient: dL/da = lam log u centred, / B (the reference centres twice; once is the same in exact arithmetic); through the softmax
    // a = softmax(m * preds): dL/dpreds_i = m a_i (g_i - sum_j a_j g_j)
    const float glam = lam * kLn2;                  // lam * log u = lam * ln2 * log2 u
    float su = 0.0f;
    for (int i = t; i < n; i += G) su += U[i];
    const float mean_u = group_sum<G>(su, red + 4, t) / (float)n;
    float sag = 0.0f;
    for (int i = t; i < n; i += G) sag = fmaf(fast_exp2(A[i]), glam * (U[i] - mean_u), sag);
    sag = group_sum<G>(sag, red, t);
    const float scale = m * inv_b;
    for (int i = t; i < L; i += G) {
        float gi = 0.0f;
        if (i < n) {
            const float gc = glam * (U[i] - mean_u);
            gi = scale * fast_exp2(A[i]) * (gc - sag);
        }
        g[i] = gi;
    }
    if (t == 0) loss_q[q] = loss;
}

template <int G, int DPT, class F> int dispatch_cost(int cost_type, F &&f) {
    switch (cost_type) {
        case PTR_WASS_COST_P1: return f(wassrank_kernel<PTR_WASS_COST_P1, G, DPT>);
        case PTR_WASS_COST_P2: return f(wassrank_kernel<PTR_WASS_COST_P2, G, DPT>);
        case PTR_WASS_COST_EG: return f(wassrank_kernel<PTR_WASS_COST_EG, G, DPT>);
        case PTR_WASS_COST_DG: return f(wassrank_kernel<PTR_WASS_COST_DG, G, DPT>);
        default: return f(wassrank_kernel<PTR_WASS_COST_DDG, G, DPT>);
    }
}

}  // namespace

// One workgroup of G threads per query, each thread DPT columns of a column tile.
Tiling wassrank_form(int L) {
    if (L <= 64) return {64, 1};
    if (L <= 128) return {64, 2};
    if (L <= 256) return {128, 2};
    return {256, 2};
}

}  // namespace ptr

extern "C" int ptr_wassrank_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, int cost_type,
                                    float gain_base, float non_rele_gap, float var_penalty, float lam, int sh_itr,
                                    int scale_by_max_label, float *loss_out, float *loss_q, float *grad, void *stream) {
    using namespace ptr;
    const char *who = "ptr_wassrank_fwd_bwd";
    if (int rc = check_loss_args(preds, labels, B, L, loss_q && grad, who)) return rc;
    if (cost_type < PTR_WASS_COST_P1 || cost_type > PTR_WASS_COST_DDG) {
        set_error("%s: unknown cost_type %d (PTR_WASS_COST_*)", who, cost_type);
        return PTR_ERR_INVALID_ARG;
    }
    if (!(lam > 0.0f)) { set_error("%s: lam must be > 0 (got %g)", who, (double)lam); return PTR_ERR_INVALID_ARG; }
    if (sh_itr < 0) { set_error("%s: sh_itr must be >= 0 (got %d)", who, sh_itr); return PTR_ERR_INVALID_ARG; }
    if (B > 0) {
        const int Lp = round_up(L, 4);
        const size_t lds = (6 * (size_t)Lp + 8) * sizeof(float);
        const float inv_b = 1.0f / (float)B;
        auto launch = [&]<int G>(auto kern) -> int {
            return launch_queries(kern, B, 1, G, lds, stream, who, preds, labels, lens, L, Lp, gain_base, non_rele_gap, var_penalty, lam, sh_itr,
                                  scale_by_max_label, inv_b, loss_q, grad);
        };
        const Tiling f = wassrank_form(L);
        int rc;
        if (f.DPT == 1) rc = dispatch_cost<64, 1>(cost_type, [&](auto k) { return launch.template operator()<64>(k); });
        else if (f.G == 64) rc = dispatch_cost<64, 2>(cost_type, [&](auto k) { return launch.template operator()<64>(k); });
        else if (f.G == 128) rc = dispatch_cost<128, 2>(cost_type, [&](auto k) { return launch.template operator()<128>(k); });
        else rc = dispatch_cost<256, 2>(cost_type, [&](auto k) { return launch.template operator()<256>(k); });
        if (rc) return rc;
    }
    return finish_loss(loss_q, B, B > 0 ? 1.0f / (float)B : 0.0f, loss_out, stream);
}
