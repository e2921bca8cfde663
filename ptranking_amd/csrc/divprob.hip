// DivProbRanker's objectives (the reference's ltr_diversification frame, the Gaussian half): every loss it optimises is built from the
// probability that document j outscores document i when both scores are independent normal variables.
//
// Reference: ptranking/ltr_diversification/score_and_sort/div_prob_ranker.py:29-79 (alpha_dcg_as_a_loss), :81-165 (err_ia_as_a_loss),
//            :167-202 (prob_lambda_loss 'PairCLS' / 'LambdaPairCLS', opt_ideal), ptranking/ltr_diversification/util/prob_utils.py:5-26,
//            :62-80 (get_diff_normal, get_expected_rank), util/div_lambda_utils.py:26-43 (get_prob_pairwise_comp_probs),
//            ptranking/metric/srd/diversity_metric.py:13-30, :143-183 (torch_alpha_dcg_at_k, get_delta_alpha_dcg).  The reference runs ONE
//            query per call and materialises [1, L, L] and [T, L, L] tensors.
//
// Per query (m = means, v = variances, r = subtopic-by-document relevance [T][L], c = 1 - beta):
//   a[i][j] = 1 / sqrt(2 (v_i + v_j))     x[i][j] = (m_i - m_j) a[i][j]     Phi[i][j] = erfc(x[i][j]) / 2   (j != i)
//   R[i] = 1 + sum_j Phi[i][j]                                                                      the expected rank
//   ANDCG          cov[t][i] = sum_j Phi[i][j] r[t][j];  loss = - sum_kept r[t][i] c^cov[t][i] / log2(1 + R[i])
//   ERRIA          s = (2^r - 1) / 2^max_label, E[i] = sum_t s[t][i] prod_{k<i} (1 - s[t][k]) (0 beyond top_k); loss = - sum_i E[i] / R[i]
//   PAIRCLS        over pairs i < j: - [ tb log P + (1 - tb) log Q ], Q = Phi[i][j], P = 1 - Q, tb = mean_t (1 + clamp(r_ti - r_tj, -1, 1)) / 2,
//                  each logarithm clamped at -100 (F.binary_cross_entropy)
//   LAMBDAPAIRCLS  the same term times | sum_t (g_ti - g_tj)(d_i f_ti - d_j f_tj) | (/ the input order's alpha-DCG when norm), g = 2^r - 1,
//                  d_i = 1 / log2(i + 2), f_ti = c^(sum_{k<i} r_tk)
// With phi = exp(-x^2) / sqrt(pi): dPhi/dx = -phi, dx[i][j]/dm_i = a, dx[i][j]/dv_i = -x a^2, and x[j][i] = -x[i][j]; so with
// D[i][j] = dLoss/dPhi[i][j] - dLoss/dPhi[j][i]:   dLoss/dm_i = - sum_j phi a D[i][j],   dLoss/dv_i = sum_j phi a (x a) D[i][j].
// The pairwise term is symmetric in (i, j) (tb[j][i] = 1 - tb[i][j], P[j][i] = Q[i][j]), so document i walks ALL its partners, takes
// half of the terms for the loss and the whole derivative for its own gradient.
//
// log Q and log P never go through 1 - Q: with e = erfcx(|x|) the small tail is exp(-x^2) e / 2, its logarithm -x^2 + log(e / 2), its
// derivative ratio phi / tail = 2 / (sqrt(pi) e); the large side is log1p(-tail) and phi / (1 - tail).  A logarithm at the -100 clamp
// passes no gradient.
//
// Kernel form: ONE thread owns document i (strided for long lists); means, variances and the relevance tile(s) live in LDS and the j
// side is read as an LDS broadcast; forward and backward in one launch, no atomics, nothing of size L x L anywhere, fixed summation order.
// LDS per query: M[Lp] | V[Lp] | A[Lp] | K tiles [Lp][TP] | red[4]; K = 1 (ERRIA: s; PAIRCLS: r), 2 (ANDCG: r, dLoss/dcov),
// 3 (LAMBDAPAIRCLS: r, d f, g); TP = T rounded up to 4, 8, 16 or 32.
#include "ptr_div.h"
#include "ptr_gauss.h"      // inv_sqrt, quot, pair_geo, pair_phi, kInvSqrtPi

namespace ptr {

__host__ __device__ constexpr int divprob_tiles(int obj) {
    return obj == PTR_DIVPROB_ANDCG ? 2 : obj == PTR_DIVPROB_LAMBDAPAIRCLS ? 3 : 1;
}
__host__ __device__ constexpr size_t divprob_group_floats(int Lp, int TP, int K) { return (size_t)Lp * (3 + K * TP) + 4; }

constexpr float kLogClamp = -100.0f;                   // F.binary_cross_entropy clamps each logarithm at -100

// expected ranks of the documents t, t + G, ... into LDS row `out` (prob_utils.py:62-80)
template <int G>
__device__ __forceinline__ void expected_ranks_pass(const float *M, const float *V, int n, int t, float *out) {
    for (int i = t; i < n; i += G) {
        const float mi = M[i], vi = V[i];
        float Ri = 1.0f;
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            const float p = pair_phi(pair_geo(mi, vi, M[j], V[j]));
            Ri += j == i ? 0.0f : p;
        }
        out[i] = Ri;
    }
}

template <int G, int TP, int OBJ>
__global__ void __launch_bounds__(kBlock)
divprob_kernel(const float *__restrict__ mus, const float *__restrict__ vars, const float *__restrict__ rele,
               const int32_t *__restrict__ lens, const int32_t *__restrict__ ntopics, int B, int T, int L, int Lp, float log2_c, float ln_c,
               int top_k, int top_k_axis, float inv_2ml, int norm, float *__restrict__ loss_q, float *__restrict__ grad_mu,
               float *__restrict__ grad_var) {
    constexpr int QPB = kBlock / G;
    constexpr int K = divprob_tiles(OBJ);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, grp = tid / G, t = tid % G;
    const int q = blockIdx.x * QPB + grp;
    const bool valid = q < B;
    int nt = valid ? (ntopics ? ntopics[q] : T) : 0;
    nt = __builtin_amdgcn_readfirstlane(nt < 0 ? 0 : (nt > T ? T : nt));
    // a query without a subtopic has no objective (the mean over subtopics of PAIRCLS is empty): it contributes exactly 0
    const int n = __builtin_amdgcn_readfirstlane(valid && nt > 0 ? query_len(lens, q, L) : 0);

    float *M = smem + (size_t)grp * divprob_group_floats(Lp, TP, K);
    float *V = M + Lp, *A = V + Lp, *R = A + Lp;
    float *T1 = R + (size_t)Lp * TP * (K > 1 ? 1 : 0), *T2 = R + (size_t)Lp * TP * (K > 2 ? 2 : 0);
    float *red = R + (size_t)Lp * TP * K;

    // ---- stage the means, the variances and the relevance columns (padded documents / subtopics: never read from memory)
    for (int i = t; i < Lp; i += G) {
        M[i] = i < n ? mus[(size_t)q * L + i] : 0.0f;
        V[i] = i < n ? vars[(size_t)q * L + i] : 1.0f;
        A[i] = 0.0f;
    }
#pragma unroll 1
    for (int tt = 0; tt < TP; ++tt) {
        const bool real = tt < nt;
        const float *row = rele + ((size_t)q * T + (real ? tt : 0)) * L;
        for (int i = t; i < Lp; i += G) {
            R[(size_t)i * TP + tt] = (real && i < n) ? row[i] : 0.0f;
            if constexpr (K > 1) T1[(size_t)i * TP + tt] = 0.0f;
            if constexpr (K > 2) T2[(size_t)i * TP + tt] = 0.0f;
        }
    }
    __syncthreads();

    float lpart = 0.0f;
    if constexpr (OBJ == PTR_DIVPROB_ANDCG || OBJ == PTR_DIVPROB_ERRIA) {
        const float ln2 = 0.6931471805599453f;
        if constexpr (OBJ == PTR_DIVPROB_ERRIA) {
            // satisfaction probabilities in place of the relevance (each thread rewrites its own rows)   div_prob_ranker.py:125
            for (int i = t; i < n; i += G) {
                float ri[TP];
                lds_row<TP>(R + (size_t)i * TP, ri);
#pragma unroll
                for (int u = 0; u < TP; ++u) ri[u] = (exp2f(ri[u]) - 1.0f) * inv_2ml;
                lds_put<TP>(R + (size_t)i * TP, ri);
            }
            __syncthreads();
        }
        // ---- pass 1: expected ranks, prior cover counts / cascades, per-document gains
        for (int i = t; i < n; i += G) {
            const float mi = M[i], vi = V[i];
            float ri[TP], cov[TP];
            lds_row<TP>(R + (size_t)i * TP, ri);
            float E = 0.0f;
            if constexpr (OBJ == PTR_DIVPROB_ERRIA) {
                if (top_k <= 0 || i < top_k) {                 // :140-158: the first top_k documents of the given order
#pragma unroll
                    for (int u = 0; u < TP; ++u) cov[u] = 1.0f;
                    for (int j = 0; j < i; ++j) {              // exclusive running product of 1 - s, in document order    :126-129
                        float sj[TP];
                        lds_row<TP>(R + (size_t)j * TP, sj);
#pragma unroll
                        for (int u = 0; u < TP; ++u) cov[u] *= 1.0f - sj[u];
                    }
#pragma unroll
                    for (int u = 0; u < TP; ++u) E = fmaf(ri[u], cov[u], E);
                }
            } else {
#pragma unroll
                for (int u = 0; u < TP; ++u) cov[u] = 0.0f;
            }
            float Ri = 1.0f;
#pragma unroll 2
            for (int j = 0; j < n; ++j) {
                float p = pair_phi(pair_geo(mi, vi, M[j], V[j]));            // prob_utils.py:70
                p = j == i ? 0.0f : p;                                       // :72
                Ri += p;
                if constexpr (OBJ == PTR_DIVPROB_ANDCG) {
                    float rj[TP];
                    lds_row<TP>(R + (size_t)j * TP, rj);
#pragma unroll
                    for (int u = 0; u < TP; ++u) cov[u] = fmaf(p, rj[u], cov[u]);   // div_prob_ranker.py:66
                }
            }
            if constexpr (OBJ == PTR_DIVPROB_ANDCG) {
                const float lg = log2f(1.0f + Ri);
                const bool doc_kept = top_k_axis == 0 || top_k <= 0 || i < top_k;
                float gsum = 0.0f;
#pragma unroll
                for (int u = 0; u < TP; ++u) {
                    const bool kept = doc_kept && (top_k_axis != 0 || top_k <= 0 || u < top_k);     // :70-75 slices SUBTOPIC rows
                    const float g = kept ? ri[u] * exp2f(cov[u] * log2_c) / lg : 0.0f;              // :68-69
                    gsum += g;
                    cov[u] = -g * ln_c;                        // dloss / dcov[t][i]
                }
                lds_put<TP>(T1 + (size_t)i * TP, cov);
                A[i] = gsum / (lg * ln2 * (1.0f + Ri));        // dloss / dR[i]
                lpart += gsum;
            } else {
                A[i] = E / (Ri * Ri);                          // dloss / dR[i]
                lpart += E / Ri;                               // :124, :131
            }
        }
        lpart = -lpart;
        __syncthreads();

        // ---- pass 2: both gradients; Phi[i][j] and Phi[j][i] share one exponential
        for (int i = t; i < n; i += G) {
            const float mi = M[i], vi = V[i], ai = A[i];
            float gm = 0.0f, gv = 0.0f;
            float ri[TP], bi[TP];
            if constexpr (OBJ == PTR_DIVPROB_ANDCG) {
                lds_row<TP>(R + (size_t)i * TP, ri);
                lds_row<TP>(T1 + (size_t)i * TP, bi);
            }
#pragma unroll 2
            for (int j = 0; j < n; ++j) {
                const PairGeo g = pair_geo(mi, vi, M[j], V[j]);
                const float w = j == i ? 0.0f : g.e2 * kInvSqrtPi * g.a;     // phi a
                float dot = ai - A[j];
                if constexpr (OBJ == PTR_DIVPROB_ANDCG) {
                    float rj[TP], bj[TP];
                    lds_row<TP>(R + (size_t)j * TP, rj);
                    lds_row<TP>(T1 + (size_t)j * TP, bj);
#pragma unroll
                    for (int u = 0; u < TP; ++u) dot = fmaf(bi[u], rj[u], dot);
#pragma unroll
                    for (int u = 0; u < TP; ++u) dot = fmaf(-bj[u], ri[u], dot);
                }
                gm = fmaf(-w, dot, gm);
                gv = fmaf(w * (g.x * g.a), dot, gv);
            }
            grad_mu[(size_t)q * L + i] = gm;
            grad_var[(size_t)q * L + i] = gv;
        }
    } else {
        float winv = 1.0f;
        if constexpr (OBJ == PTR_DIVPROB_LAMBDAPAIRCLS) {
            // ---- per-(t, i) user focus times the rank discount, gains, and the input order's alpha-DCG   diversity_metric.py:152-167, :13-30
            float ipart = 0.0f;
            for (int i = t; i < n; i += G) {
                float cov[TP], ri[TP];
#pragma unroll
                for (int u = 0; u < TP; ++u) cov[u] = 0.0f;
                for (int j = 0; j < i; ++j) {                  // exclusive cumulative cover count, in document order
                    float rj[TP];
                    lds_row<TP>(R + (size_t)j * TP, rj);
#pragma unroll
                    for (int u = 0; u < TP; ++u) cov[u] += rj[u];
                }
                lds_row<TP>(R + (size_t)i * TP, ri);
                const float d = 1.0f / log2f((float)i + 2.0f);
#pragma unroll
                for (int u = 0; u < TP; ++u) {
                    cov[u] = exp2f(cov[u] * log2_c) * d;
                    ipart = fmaf(ri[u], cov[u], ipart);
                }
                lds_put<TP>(T1 + (size_t)i * TP, cov);
#pragma unroll
                for (int u = 0; u < TP; ++u) cov[u] = exp2f(ri[u]) - 1.0f;
                lds_put<TP>(T2 + (size_t)i * TP, cov);
            }
            const float ideal = group_sum<G>(ipart, red, t);
            if (norm) winv = ideal > 0.0f ? 1.0f / ideal : 0.0f;             // :180-181; an ideal value <= 0: weight 0, not 0 / 0
            __syncthreads();
        }
        const float half_inv_nt = nt > 0 ? 0.5f / (float)nt : 0.0f;
        for (int i = t; i < n; i += G) {
            const float mi = M[i], vi = V[i];
            float ri[TP], gi[TP], hi[TP];
            lds_row<TP>(R + (size_t)i * TP, ri);
            if constexpr (OBJ == PTR_DIVPROB_LAMBDAPAIRCLS) {
                lds_row<TP>(T1 + (size_t)i * TP, hi);
                lds_row<TP>(T2 + (size_t)i * TP, gi);
            }
            float lp = 0.0f, gm = 0.0f, gv = 0.0f;
#pragma unroll 2
            for (int j = 0; j < n; ++j) {
                const PairGeo g = pair_geo(mi, vi, M[j], V[j]);
                const float ex = erfcxf(fabsf(g.x));
                const float tail = 0.5f * g.e2 * ex;
                const float log_small = (logf(0.5f * ex) - g.sq_lo) - g.sq_hi, log_big = log1pf(-tail);
                const float rat_small = quot(2.0f * kInvSqrtPi, ex), rat_big = quot(g.e2 * kInvSqrtPi, 1.0f - tail);
                const bool pos = g.x > 0.0f;                                 // Q = erfc(x) / 2 is the small side
                const float logQ = pos ? log_small : log_big, logP = pos ? log_big : log_small;
                const float ratQ = pos ? rat_small : rat_big, ratP = pos ? rat_big : rat_small;
                float rj[TP];
                lds_row<TP>(R + (size_t)j * TP, rj);
                float sd = 0.0f;
#pragma unroll
                for (int u = 0; u < TP; ++u) sd += __builtin_amdgcn_fmed3f(ri[u] - rj[u], -1.0f, 1.0f);   // div_lambda_utils.py:36-38
                const float tb = fmaf(sd, half_inv_nt, 0.5f);                //                                    :39
                float w = j == i ? 0.0f : 1.0f;
                if constexpr (OBJ == PTR_DIVPROB_LAMBDAPAIRCLS) {
                    float gj[TP], hj[TP];
                    lds_row<TP>(T1 + (size_t)j * TP, hj);
                    lds_row<TP>(T2 + (size_t)j * TP, gj);
                    float dd = 0.0f;
#pragma unroll
                    for (int u = 0; u < TP; ++u) dd = fmaf(gi[u] - gj[u], hi[u] - hj[u], dd);             // diversity_metric.py:164-178
                    w *= fabsf(dd) * winv;
                }
                const float term = -(tb * fmaxf(logP, kLogClamp) + (1.0f - tb) * fmaxf(logQ, kLogClamp));
                const float dx = (1.0f - tb) * (logQ > kLogClamp ? ratQ : 0.0f) - tb * (logP > kLogClamp ? ratP : 0.0f);
                lp = fmaf(w, term, lp);
                const float wd = w * dx * g.a;
                gm += wd;
                gv = fmaf(-wd, g.x * g.a, gv);
            }
            lpart = fmaf(0.5f, lp, lpart);
            grad_mu[(size_t)q * L + i] = gm;
            grad_var[(size_t)q * L + i] = gv;
        }
    }
    const float tot = group_sum<G>(lpart, red, t);
    if (valid) {
        for (int i = n + t; i < L; i += G) { grad_mu[(size_t)q * L + i] = 0.0f; grad_var[(size_t)q * L + i] = 0.0f; }
        if (t == 0) loss_q[q] = tot;
    }
}

// The first pass alone: R[i] = 1 + sum_{j != i} Phi[i][j].  LDS per query: M[Lp] | V[Lp] | R[Lp].
template <int G>
__global__ void __launch_bounds__(kBlock)
divprob_ranks_kernel(const float *__restrict__ mus, const float *__restrict__ vars, const int32_t *__restrict__ lens, int B, int L, int Lp,
                     float *__restrict__ ranks) {
    constexpr int QPB = kBlock / G;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, grp = tid / G, t = tid % G;
    const int q = blockIdx.x * QPB + grp;
    const bool valid = q < B;
    const int n = __builtin_amdgcn_readfirstlane(valid ? query_len(lens, q, L) : 0);
    float *M = smem + (size_t)grp * 3 * Lp, *V = M + Lp, *out = V + Lp;
    for (int i = t; i < Lp; i += G) {
        M[i] = i < n ? mus[(size_t)q * L + i] : 0.0f;
        V[i] = i < n ? vars[(size_t)q * L + i] : 1.0f;
        out[i] = 0.0f;
    }
    __syncthreads();
    expected_ranks_pass<G>(M, V, n, t, out);
    if (valid)
        for (int i = t; i < L; i += G) ranks[(size_t)q * L + i] = i < n ? out[i] : 0.0f;     // thread t reads what it wrote
}

template <int G, int TP> static auto divprob_kernel_of(int objective) {
    return objective == PTR_DIVPROB_ANDCG ? divprob_kernel<G, TP, PTR_DIVPROB_ANDCG>
         : objective == PTR_DIVPROB_ERRIA ? divprob_kernel<G, TP, PTR_DIVPROB_ERRIA>
         : objective == PTR_DIVPROB_PAIRCLS ? divprob_kernel<G, TP, PTR_DIVPROB_PAIRCLS>
                                            : divprob_kernel<G, TP, PTR_DIVPROB_LAMBDAPAIRCLS>;
}

static size_t divprob_query_bytes(int objective, int T, int L) {
    return divprob_group_floats(round_up(L, 4), tp_of(T), divprob_tiles(objective)) * sizeof(float);
}
DivForm divprob_form(int objective, int T, int L) {
    return div_form(T, L, (kBlock / kWave) * divprob_query_bytes(objective, T, L) <= kLdsPerWorkgroup);
}

}  // namespace ptr

extern "C" int ptr_divprob_fwd_bwd(const float *mus, const float *vars, const float *rele, const int32_t *lens, const int32_t *ntopics, int B,
                                   int T, int L, int objective, float beta, int top_k, int top_k_axis, float max_label, int norm,
                                   float *loss_out, float *loss_q, float *grad_mu, float *grad_var, void *stream) {
    using namespace ptr;
    const char *who = "ptr_divprob_fwd_bwd";
    if (int rc = check_batch(mus, vars, B, L, who)) return rc;
    if (int rc = check_pointers(B, rele != nullptr, who, "NULL input pointer (rele)")) return rc;
    if (int rc = check_subtopics_given(T, who)) return rc;
    if (objective < PTR_DIVPROB_ANDCG || objective > PTR_DIVPROB_LAMBDAPAIRCLS) {
        set_error("%s: objective must be one of PTR_DIVPROB_* (0 .. 3), got %d", who, objective);
        return PTR_ERR_INVALID_ARG;
    }
    if (!(beta > 0.0f && beta < 1.0f)) { set_error("%s: beta must be in (0, 1) (got %g)", who, (double)beta); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_top_k_axis(top_k_axis, who)) return rc;
    if (objective == PTR_DIVPROB_ERRIA && !(max_label >= 0.0f)) {
        set_error("%s: ERR-IA needs max_label >= 0 (got %g)", who, (double)max_label);
        return PTR_ERR_INVALID_ARG;
    }
    if (int rc = check_subtopics_fit(T, who)) return rc;
    if (int rc = check_pointers(B, loss_q && grad_mu && grad_var, who)) return rc;
    const int Lp = round_up(L, 4), TP = tp_of(T), K = divprob_tiles(objective);
    const size_t per_query = divprob_query_bytes(objective, T, L);
    if (per_query > kLdsPerWorkgroup) {
        set_error("%s: T=%d, L=%d need %zu bytes of LDS per workgroup (limit %zu): 4 * round_up(L, 4) * (3 + %d * %d) + 16 bytes per query", who, T,
                  L, per_query, kLdsPerWorkgroup, K, TP);
        return PTR_ERR_UNSUPPORTED;
    }
    const DivForm f = divprob_form(objective, T, L);
    const int QPB = kBlock / f.G;
    const size_t lds = (size_t)QPB * per_query;
    if (B > 0) {
        const double c = 1.0 - (double)beta;
        auto go = [&](auto kern) -> int {
            return launch_queries(kern, B, QPB, kBlock, lds, stream, who, mus, vars, rele, lens, ntopics, B, T, L, Lp, (float)log2(c), (float)log(c), top_k,
                                  top_k_axis, objective == PTR_DIVPROB_ERRIA ? exp2f(-max_label) : 0.0f, norm, loss_q, grad_mu, grad_var);
        };
        if (int rc = dispatch_tp(TP, [&]<int TP_>() {
                return f.G == kWave ? go(divprob_kernel_of<64, TP_>(objective)) : go(divprob_kernel_of<256, TP_>(objective));
            })) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}

extern "C" int ptr_divprob_expected_ranks(const float *mus, const float *vars, const int32_t *lens, int B, int L, float *ranks, void *stream) {
    using namespace ptr;
    const char *who = "ptr_divprob_expected_ranks";
    if (int rc = check_loss_args(mus, vars, B, L, ranks != nullptr, who, "NULL output pointer (ranks)")) return rc;
    if (B == 0) return 0;
    const int Lp = round_up(L, 4);
    const int QPB = L <= 128 ? kBlock / kWave : 1;
    const size_t lds = (size_t)QPB * 3 * Lp * sizeof(float);          // <= 48 KiB at L = PTR_MAX_LIST_LEN
    return QPB > 1 ? launch_queries(divprob_ranks_kernel<64>, B, QPB, kBlock, lds, stream, who, mus, vars, lens, B, L, Lp, ranks)
                   : launch_queries(divprob_ranks_kernel<256>, B, 1, kBlock, lds, stream, who, mus, vars, lens, B, L, Lp, ranks);
}
