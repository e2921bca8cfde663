// Search-result diversification (the reference's ltr_diversification frame): DALETOR's alpha-DCG loss and the three diversity metrics.
//
// Reference: ptranking/ltr_diversification/score_and_sort/daletor.py:9-38 (get_approx_ranks, alphaDCG_as_a_loss; the reference runs ONE
//            query per call on [T, L] tensors and materialises [T, L, L]), Robust_Sigmoid ptranking/base/utils.py:57-95,
//            ptranking/metric/srd/diversity_metric.py:43-82 (alpha-nDCG@ks), :189-245 (ERR-IA@ks), :265-291 (nERR-IA@ks),
//            ptranking/base/ranker.py:269-475 (the Evaluator's sort -> gather -> metric prologue).
//
// Loss, per query (R = subtopic-by-document relevance [T][L], rs = Robust_Sigmoid, c = 1 - alpha):
//   ind[i][j]   = rs(rt (s_j - s_i))                         pi[i] = 0.5 + sum_j ind[i][j]
//   cover[t][i] = sum_j ind[i][j] R[t][j] - R[t][i] / 2      (the j = i term cancels: both sums run over j != i here)
//   g[t][i]     = R[t][i] c^cover[t][i] / log2(1 + pi[i])    loss = - sum_{(t,i) kept by top_k} g[t][i]
// Gradient, with d[i][j] = ind[i][j] (1 - ind[i][j]) = d[j][i] (the two indicators of a pair sum to 1):
//   A[i] = sum_t g / (log2(1 + pi) ln2 (1 + pi)),  Bc[t][i] = -g ln c,  G[i][j] = A[i] + sum_t Bc[t][i] R[t][j]
//   grad[j] = rt sum_i d[i][j] (G[i][j] - G[j][i])
//
// Kernel form: ONE thread owns document i.  Pass 1 keeps pi[i] and cover[0..T)[i] in registers and walks j with s_j and the column
// R[:, j] broadcast from LDS; A and Bc go to LDS; pass 2 walks the partners once more and, because d is symmetric, takes both
// directions of a pair from the same exponential.  No atomics, nothing of size L x L anywhere, fixed summation order.
// LDS per query: S[Lp] | A[Lp] | R[Lp][TP] | Bc[Lp][TP] (TP = T rounded up to 4, 8, 16 or 32: float4 broadcast reads of a column).
#include "ptr_div.h"
#include "ptr_rsig.h"

namespace ptr {

__host__ __device__ constexpr size_t adcg_group_floats(int Lp, int TP) { return (size_t)Lp * (2 + 2 * TP) + 4; }

template <int G, int TP>
__global__ void __launch_bounds__(kBlock)
alphadcg_kernel(const float *__restrict__ preds, const float *__restrict__ rele, const int32_t *__restrict__ lens,
                const int32_t *__restrict__ ntopics, int B, int T, int L, int Lp, float rt, float log2_c, float ln_c, int top_k,
                int top_k_axis, float *__restrict__ loss_q, float *__restrict__ grad) {
    constexpr int QPB = kBlock / G;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, grp = tid / G, t = tid % G;
    const int q = blockIdx.x * QPB + grp;
    const bool valid = q < B;
    const int n = __builtin_amdgcn_readfirstlane(valid ? query_len(lens, q, L) : 0);
    int nt = valid ? (ntopics ? ntopics[q] : T) : 0;
    nt = __builtin_amdgcn_readfirstlane(nt < 0 ? 0 : (nt > T ? T : nt));

    float *S = smem + (size_t)grp * adcg_group_floats(Lp, TP);
    float *A = S + Lp, *R = A + Lp, *Bc = R + (size_t)Lp * TP, *red = Bc + (size_t)Lp * TP;

    // ---- stage the scores and the relevance columns (padded documents / subtopics: 0, never read from memory)
    for (int i = t; i < Lp; i += G) { S[i] = i < n ? preds[(size_t)q * L + i] : 0.0f; A[i] = 0.0f; }
#pragma unroll 1
    for (int tt = 0; tt < TP; ++tt) {
        const bool real = tt < nt;
        const float *row = rele + ((size_t)q * T + (real ? tt : 0)) * L;
        for (int i = t; i < Lp; i += G) {
            R[(size_t)i * TP + tt] = (real && i < n) ? row[i] : 0.0f;
            Bc[(size_t)i * TP + tt] = 0.0f;
        }
    }
    __syncthreads();

    // ---- pass 1: smooth ranks, prior cover counts, per-document gains
    const float ln2 = 0.6931471805599453f;
    float lpart = 0.0f;
    for (int i = t; i < n; i += G) {
        const float si = S[i];
        float ri[TP], cov[TP];
        lds_row<TP>(R + (size_t)i * TP, ri);
#pragma unroll
        for (int u = 0; u < TP; ++u) cov[u] = 0.0f;
        float pi = 1.0f;                                       // 0.5 (the j = i indicator, utils.py:57-95 at 0) + 0.5 (daletor.py:15)
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            float ya, yb;
            robust_pair(S[j] - si, rt, ya, yb);                // ind[i][j]                                   daletor.py:11-13
            ya = j == i ? 0.0f : ya;
            float rj[TP];
            lds_row<TP>(R + (size_t)j * TP, rj);
            pi += ya;
#pragma unroll
            for (int u = 0; u < TP; ++u) cov[u] = fmaf(ya, rj[u], cov[u]);   //                              daletor.py:17-19
        }
        const float lg = log2f(1.0f + pi);
        const bool doc_kept = top_k_axis == 0 || top_k <= 0 || i < top_k;
        float gsum = 0.0f;
#pragma unroll
        for (int u = 0; u < TP; ++u) {
            const bool kept = doc_kept && (top_k_axis != 0 || top_k <= 0 || u < top_k);     // daletor.py:30-35 slices SUBTOPIC rows
            const float g = kept ? ri[u] * exp2f(cov[u] * log2_c) / lg : 0.0f;              // daletor.py:29
            gsum += g;
            cov[u] = -g * ln_c;                                // dloss / dcover[t][i]
        }
#pragma unroll
        for (int u = 0; u < TP; u += 4) *reinterpret_cast<float4 *>(Bc + (size_t)i * TP + u) = float4{cov[u], cov[u + 1], cov[u + 2], cov[u + 3]};
        A[i] = gsum / (lg * ln2 * (1.0f + pi));                // dloss / dpi[i]
        lpart += gsum;
    }
    const float tot = group_sum<G>(lpart, red, t);
    __syncthreads();

    // ---- pass 2: gradient; both directions of a pair from one exponential
    for (int i = t; i < n; i += G) {
        const float si = S[i], ai = A[i];
        float ri[TP], bi[TP];
        lds_row<TP>(R + (size_t)i * TP, ri);
        lds_row<TP>(Bc + (size_t)i * TP, bi);
        float acc = 0.0f;
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            float ya, yb;
            robust_pair(S[j] - si, rt, ya, yb);
            const float d = j == i ? 0.0f : ya * yb;           // ind (1 - ind): the tensor Robust_Sigmoid saves, utils.py:76
            float rj[TP], bj[TP];
            lds_row<TP>(R + (size_t)j * TP, rj);
            lds_row<TP>(Bc + (size_t)j * TP, bj);
            float dot = A[j] - ai;
#pragma unroll
            for (int u = 0; u < TP; ++u) dot = fmaf(bj[u], ri[u], dot);
#pragma unroll
            for (int u = 0; u < TP; ++u) dot = fmaf(-bi[u], rj[u], dot);
            acc = fmaf(d, dot, acc);
        }
        grad[(size_t)q * L + i] = rt * acc;
    }
    if (valid) {
        for (int i = n + t; i < L; i += G) grad[(size_t)q * L + i] = 0.0f;
        if (t == 0) loss_q[q] = -tot;
    }
}

// ---------------------------------------------------------------------------------------------------------------- metrics
struct DivCutoffs { int nk; int kmax; int k[PTR_MAX_CUTOFFS]; };

// One group per query ranks the scores exactly as ptr_sort_desc does (count_ranks: value descending, NaN first, original index ascending) and
// scatters the top documents into `order`; then ONE wavefront walks the ranks 0 .. min(max(ks), n) - 1 with lane = subtopic: the
// system ranking and the ideal one (the input order, ranker.py:296) side by side, every running quantity per lane, a cross-lane sum
// only at the cut-offs.  LDS per group: keys[Lp] | order[Lp] | red[4].
template <int G, int DPT>
__global__ void __launch_bounds__(kBlock)
div_metrics_kernel(const float *__restrict__ preds, const float *__restrict__ rele, const int32_t *__restrict__ lens,
                   const int32_t *__restrict__ ntopics, int B, int T, int L, int Lp, DivCutoffs ck, float log2_c, float inv_2ml,
                   float *__restrict__ o_andcg, float *__restrict__ o_err, float *__restrict__ o_nerr, int32_t *__restrict__ o_valid) {
    constexpr int QPB = kBlock / G;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, grp = tid / G, t = tid % G;
    const int q = blockIdx.x * QPB + grp;
    const bool valid = q < B;
    const int n = __builtin_amdgcn_readfirstlane(valid ? query_len(lens, q, L) : 0);
    int nt = valid ? (ntopics ? ntopics[q] : T) : 0;
    nt = __builtin_amdgcn_readfirstlane(nt < 0 ? 0 : (nt > T ? T : nt));

    float *keys = smem + (size_t)grp * (2 * (size_t)Lp + 4);
    int *order = reinterpret_cast<int *>(keys + Lp);
    float *red = keys + 2 * (size_t)Lp;

    float own[DPT];
    int rk[DPT];
    bool isnan = false;
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        own[m] = i < n ? preds[(size_t)q * L + i] : -INFINITY;
        isnan |= own[m] != own[m];
        if (i < Lp) { keys[i] = own[m]; order[i] = 0; }
    }
    // A NaN score ranks first, as in ptr_sort_desc and torch.sort; the float compares of the plain count would give it rank 0 beside the
    // true maximum (two documents in order[0], none in order[n - 1]).  The vote rides on the barrier the staging needs anyway: each
    // wavefront leaves its own in red[] ahead of it (group_sum() below opens with a barrier before it reuses red).
    static_assert(G == kWave || G == 4 * kWave, "red[] holds one vote per wavefront of a four-wave group");
    bool anynan = __any(isnan);
    if constexpr (G != kWave) {
        if ((t & 63) == 0) red[t >> 6] = anynan ? 1.0f : 0.0f;
    }
    __syncthreads();
    if constexpr (G != kWave) anynan = (red[0] + red[1]) + (red[2] + red[3]) != 0.0f;
    if (anynan) count_ranks<G, DPT, false, true>(keys, n, t, own, rk);
    else count_ranks<G, DPT>(keys, n, t, own, rk);
#pragma unroll
    for (int m = 0; m < DPT; ++m)
        if (t + m * G < n && rk[m] >= 0 && rk[m] < n) order[rk[m]] = t + m * G;
    // total relevance of the query: the evaluator skips a query whose R sums to less than 1 (ranker.py:282, :319, :430)
    float rsum = 0.0f;
    for (int idx = t; idx < nt * n; idx += G) rsum += rele[((size_t)q * T + idx / n) * L + idx % n];
    const float rtot = group_sum<G>(rsum, red, t);
    __syncthreads();
    const bool ok = valid && rtot >= 1.0f;

    if (t < kWave) {
        const bool act = t < nt;
        const float *row = rele + ((size_t)q * T + (act ? t : 0)) * L;
        const int kwalk = ck.kmax < n ? ck.kmax : n;
        float cov_s = 0.0f, cov_i = 0.0f, dcg_s = 0.0f, dcg_i = 0.0f;       // this subtopic's cover count and cumulated gain
        float uns_s = 1.0f, uns_i = 1.0f, err_s = 0.0f, err_i = 0.0f;       // cascade of 1 - satisfaction, cumulated ERR
        float my_a = 0.0f, my_e = 0.0f, my_n = 0.0f;                        // lane c keeps the outputs of cut-off c
        for (int r = 0; r < kwalk; ++r) {
            const float xs = act ? row[order[r]] : 0.0f, xi = act ? row[r] : 0.0f;
            const float den = log2f((float)r + 2.0f), rr = 1.0f / ((float)r + 1.0f);
            dcg_s += exp2f(cov_s * log2_c) * xs / den;                       // diversity_metric.py:52
            dcg_i += exp2f(cov_i * log2_c) * xi / den;
            cov_s += xs; cov_i += xi;
            const float sat_s = (exp2f(xs) - 1.0f) * inv_2ml, sat_i = (exp2f(xi) - 1.0f) * inv_2ml;   // :198
            err_s += sat_s * uns_s * rr;                                     // :213
            err_i += sat_i * uns_i * rr;
            uns_s *= 1.0f - sat_s; uns_i *= 1.0f - sat_i;                    // :199-202
            bool hit = false;
            for (int c = 0; c < ck.nk; ++c) hit |= ck.k[c] == r + 1;
            if (hit) {
                const float Ds = wave_sum(dcg_s), Di = wave_sum(dcg_i);
                const float Es = wave_sum(err_s) / (float)nt, Ei = wave_sum(err_i) / (float)nt;   // :217, :221: all subtopics count
                const float a = Di > 0.0f ? Ds / Di : 0.0f;                  // :73-75
                const float ne = Ei > 0.0f ? Es / Ei : 0.0f;                 // :281-283
                if (t < ck.nk && ck.k[t & (PTR_MAX_CUTOFFS - 1)] == r + 1) { my_a = a; my_e = Es; my_n = ne; }
            }
        }
        if (valid && t < ck.nk) {                                            // k > n (or an invalid query): 0, the reference's padding
            const size_t o = (size_t)q * ck.nk + t;
            if (o_andcg) o_andcg[o] = ok ? my_a : 0.0f;
            if (o_err) o_err[o] = ok ? my_e : 0.0f;
            if (o_nerr) o_nerr[o] = ok ? my_n : 0.0f;
        }
        if (valid && t == 0 && o_valid) o_valid[q] = ok ? 1 : 0;
    }
}

}  // namespace ptr

extern "C" int ptr_alphadcg_fwd_bwd(const float *preds, const float *rele, const int32_t *lens, const int32_t *ntopics, int B, int T,
                                    int L, float rt, float alpha, int top_k, int top_k_axis, float *loss_out, float *loss_q,
                                    float *grad, void *stream) {
    using namespace ptr;
    const char *who = "ptr_alphadcg_fwd_bwd";
    if (int rc = check_div(preds, rele, B, T, L, alpha, who)) return rc;
    if (!(rt > 0.0f)) { set_error("%s: rt must be > 0 (got %g)", who, (double)rt); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_top_k_axis(top_k_axis, who)) return rc;
    if (int rc = check_pointers(B, loss_q && grad, who)) return rc;
    const DivForm f = div_form(T, L);
    const int Lp = round_up(L, 4), TP = f.TP, QPB = kBlock / f.G;
    const size_t lds = (size_t)QPB * adcg_group_floats(Lp, TP) * sizeof(float);
    if (lds > kLdsPerWorkgroup) {
        set_error("%s: T=%d, L=%d need %zu bytes of LDS per workgroup (limit %zu): 8 * round_up(L, 4) * (1 + %d) + 16 bytes per query", who, T, L,
                  lds, kLdsPerWorkgroup, TP);
        return PTR_ERR_UNSUPPORTED;
    }
    if (B > 0) {
        const double c = 1.0 - (double)alpha;
        auto go = [&](auto kern) -> int {
            return launch_queries(kern, B, QPB, kBlock, lds, stream, who, preds, rele, lens, ntopics, B, T, L, Lp, rt, (float)log2(c), (float)log(c), top_k,
                                  top_k_axis, loss_q, grad);
        };
        if (int rc = dispatch_tp(TP, [&]<int TP_>() { return f.G == kWave ? go(alphadcg_kernel<64, TP_>) : go(alphadcg_kernel<256, TP_>); })) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}

extern "C" int ptr_div_metrics_at_ks(const float *preds, const float *rele, const int32_t *lens, const int32_t *ntopics, int B, int T,
                                     int L, const int32_t *ks, int nk, float alpha, float max_label, float *andcg, float *err_ia,
                                     float *nerr_ia, int32_t *valid, void *stream) {
    using namespace ptr;
    const char *who = "ptr_div_metrics_at_ks";
    if (int rc = check_div(preds, rele, B, T, L, alpha, who)) return rc;
    if (nk < 0 || (nk > 0 && !ks)) { set_error("%s: bad cut-off list", who); return PTR_ERR_INVALID_ARG; }
    if (nk > PTR_MAX_CUTOFFS) { set_error("%s: %d cut-offs exceed PTR_MAX_CUTOFFS=%d", who, nk, PTR_MAX_CUTOFFS); return PTR_ERR_UNSUPPORTED; }
    if ((err_ia || nerr_ia) && !(max_label >= 0.0f)) {      // diversity_metric.py:190 asserts a maximum label; none is guessed here
        set_error("%s: ERR-IA needs max_label >= 0 (got %g)", who, (double)max_label);
        return PTR_ERR_INVALID_ARG;
    }
    if (B == 0) return 0;
    DivCutoffs ck;
    ck.nk = nk; ck.kmax = 0;
    for (int c = 0; c < PTR_MAX_CUTOFFS; ++c) {
        ck.k[c] = c < nk ? ks[c] : 0;
        if (ck.k[c] > ck.kmax) ck.kmax = ck.k[c];
    }
    const float inv_2ml = (err_ia || nerr_ia) ? exp2f(-max_label) : 0.0f;
    return dispatch_tiling(L, [&]<int G, int DPT>() -> int {
        constexpr int QPB = kBlock / G;
        const int Lp = round_up(L, 4);
        const size_t lds = (size_t)QPB * (2 * (size_t)Lp + 4) * sizeof(float);
        return launch_queries(div_metrics_kernel<G, DPT>, B, QPB, kBlock, lds, stream, who, preds, rele, lens, ntopics, B, T, L, Lp, ck,
                              (float)log2(1.0 - (double)alpha), inv_2ml, andcg, err_ia, nerr_ia, valid);
    });
}
