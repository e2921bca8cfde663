// Gaussian expected-rank metric objectives: P, AP, nERR and nDCG as optimisation objectives on the expected ranks of documents whose scores
// are independent normal variables — a variance-aware ad hoc ranker; with a constant variance, SoftRank's rank model under all four metrics.
//
// Reference: ptranking/ltr_diversification/util/prob_utils.py:62-80 (get_expected_rank), :82-101 (get_expected_rank_const) feeding
//            ptranking/metric/smooth_metric/metric_as_opt_objective.py:12-257 (precision_ / AP_ / nERR_ / nDCG_as_opt_objective: the line
//            `#batch_expt_ranks = get_expected_rank(batch_mus=..., batch_vars=...)` each of them carries), and their autograd backward.
//
// Per query of n documents (means m, variances v, labels presorted: the input order is the ideal order):
//   a_ij = 1 / sqrt(2 (v_i + v_j))    x_ij = (m_i - m_j) a_ij    Phi_ij = erfc(x_ij) / 2    phi_ij = exp(-x_ij^2) / sqrt(pi)
//   r_i    = 1 + sum_{j != i} Phi_ij
//   loss   = - sum_i W_i f(r_i),      f(r) = 1 / r (P, AP, nERR)  or  1 / log2(1 + r) (nDCG);      u_i = -W_i f'(r_i)
//   dloss/dm_i = sum_j phi_ij a_ij (u_j - u_i)          dloss/dv_i = sum_j phi_ij a_ij (x_ij a_ij) (u_i - u_j)
// (the D-form of divprob.hip's header with D_ij = u_i - u_j).  The weights W_i are those of smoothmetric.hip (ptr_smooth.h; listed per form
// in include/ptranking_amd.h): constants of the backward that depend on the labels and on the HARD position pos_i — the input index under
// opt_ideal, else the 0-based rank of the kernel's own fp32 r_i ascending with ties by index, the reference's torch.sort of the ranks.
// Expected ranks are NOT monotone in the mean (a wide document sits nearer the middle than a narrow one of the same mean), so the
// order is counted from the computed ranks (count_ranks_fast on the keys -r_i), never from the means.
//
// Kernel forms: the pair primitives of divprob.hip (ptr_gauss.h) around the O(n) weight step of smoothmetric.hip (ptr_smooth.h).  Nothing
// of size n x n exists, there are no atomics, and every sum has a fixed order given (n, L): a query's bits do not depend on the rest of the
// batch or on the run.  Every sum over the partners (the rank and both gradients) is compensated (Kahan): a plain fp32 chain that grows to
// r ~ n would lose more than the erfc terms' own error, and the gradient terms are signed.
//   L <= 512   one wavefront per query, four queries per workgroup, both passes out of registers (gauss_ring): lane a owns documents a,
//              a + 64, ... (1, 2, 3, 4, 6 or 8 per lane) and a set of travelling records {m, v, u, accumulators} that moves one lane per
//              step (v_mov_b32_dpp wave_rol:1), the circulant half ring of approx_ring (ptr_rsig.h): every UNORDERED pair is evaluated
//              once — x_ji = -x_ij exactly, so Phi_ji = 1 - tail or tail from the same erfcx, g a is symmetric and (x a) antisymmetric —
//              and the partner's share rides in the travelling accumulators.  Padding records carry m = -1e30, v = 1, u = 0: a real
//              document gets Phi = 0 and g = 0 from them exactly.  LDS per wavefront: 128 x documents per lane floats (the rank
//              count's keys and marks, then the scan row of the weight step).
//   L <= 4096  one workgroup per query, 4, 8 or 16 documents per thread; means, variances and u in LDS, document i walks ALL its partners
//              j (an LDS broadcast read per partner), so nothing is accumulated into a partner's row.  LDS per query (floats),
//              Lp = 256 x documents per thread: M[Lp] | V[Lp] | A[Lp] | S[Lp] | red[4] — A: the ranks, then the sort keys, then u; S: the
//              rank count's marks, then the scan row of the weight step.  64 KiB + 16 bytes at L = 4096.
#include "ptr_device.h"
#include "ptr_gauss.h"
#include "ptr_smooth.h"

namespace ptr {

__host__ __device__ constexpr size_t gauss_group_floats(int Lp) { return (size_t)Lp * 4 + 4; }

// s + c += x, compensated
__device__ __forceinline__ void kahan_add(float &s, float &c, float x) {
    const float y = x - c, t = s + y;
    c = (t - s) - y;
    s = t;
}

// The register ring over all unordered pairs of one query (one wavefront).  PASS 1: o1[k] = 1 + sum_{j != i} Phi_ij of document lane + 64 k.
// PASS 2: o1[k] = dloss/dm, o2[k] = dloss/dv from the coefficients u.  Own records stay put; the travelling records meet the lanes 1 .. 32
// ahead (at 32 both ends see each other: the lower half keeps the pair), slot pairs inside a lane are taken once (t > k).
template <int DPT, int PASS>
__device__ __forceinline__ void gauss_ring(const float (&m)[DPT], const float (&v)[DPT], const float (&u)[DPT], int lane, float (&o1)[DPT],
                                           float (&o2)[DPT]) {
    float Tm[DPT], Tv[DPT], Tu[DPT];
    float as1[DPT], ac1[DPT], as2[DPT], ac2[DPT], Ts1[DPT], Tc1[DPT], Ts2[DPT], Tc2[DPT];
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
        Tm[k] = m[k]; Tv[k] = v[k]; Tu[k] = u[k];
        as1[k] = PASS == 1 ? 1.0f : 0.0f;
        ac1[k] = as2[k] = ac2[k] = Ts1[k] = Tc1[k] = Ts2[k] = Tc2[k] = 0.0f;
    }
    auto pair = [&](int k, int t, bool keep) __attribute__((always_inline)) {
        const PairGeo g = pair_geo(m[k], v[k], Tm[t], Tv[t]);
        if constexpr (PASS == 1) {
            const float tail = 0.5f * g.e2 * erfcxf(fabsf(g.x));          // pair_phi, both directions from one erfcx
            const bool pos = g.x >= 0.0f;
            const float pa = pos ? tail : 1.0f - tail, pb = pos ? 1.0f - tail : tail;
            kahan_add(as1[k], ac1[k], keep ? pa : 0.0f);
            kahan_add(Ts1[t], Tc1[t], keep ? pb : 0.0f);
        } else {
            const float w = g.e2 * kInvSqrtPi * g.a;                       // phi a
            const float d = Tu[t] - u[k];
            const float tm = keep ? w * d : 0.0f, tv = keep ? (w * (g.x * g.a)) * (0.0f - d) : 0.0f;
            kahan_add(as1[k], ac1[k], tm);
            kahan_add(Ts1[t], Tc1[t], 0.0f - tm);
            kahan_add(as2[k], ac2[k], tv);
            kahan_add(Ts2[t], Tc2[t], tv);                                 // x and d both change sign
        }
    };
    auto rotate = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < DPT; ++t) {
            Tm[t] = dpp_rol1(Tm[t]); Tv[t] = dpp_rol1(Tv[t]); Ts1[t] = dpp_rol1(Ts1[t]); Tc1[t] = dpp_rol1(Tc1[t]);
            if constexpr (PASS == 2) { Tu[t] = dpp_rol1(Tu[t]); Ts2[t] = dpp_rol1(Ts2[t]); Tc2[t] = dpp_rol1(Tc2[t]); }
        }
    };
#pragma unroll
    for (int k = 0; k < DPT; ++k)
#pragma unroll
        for (int t = k + 1; t < DPT; ++t) pair(k, t, true);
    for (int r = 1; r < 32; ++r) {
        rotate();
#pragma unroll
        for (int k = 0; k < DPT; ++k)
#pragma unroll
            for (int t = 0; t < DPT; ++t) pair(k, t, true);
    }
    rotate();
    const bool low = lane < 32;
#pragma unroll
    for (int k = 0; k < DPT; ++k)
#pragma unroll
        for (int t = 0; t < DPT; ++t) pair(k, t, low);
    // the travelling accumulators sit half a ring away from their owners
#pragma unroll
    for (int k = 0; k < DPT; ++k) {
        kahan_add(as1[k], ac1[k], __shfl_xor(Ts1[k], 32, 64));
        kahan_add(as1[k], ac1[k], 0.0f - __shfl_xor(Tc1[k], 32, 64));
        o1[k] = as1[k];
        if constexpr (PASS == 2) {
            kahan_add(as2[k], ac2[k], __shfl_xor(Ts2[k], 32, 64));
            kahan_add(as2[k], ac2[k], 0.0f - __shfl_xor(Tc2[k], 32, 64));
            o2[k] = as2[k];
        }
    }
}

// One wavefront per query, lists of up to 64 DPT <= 512 documents.  LDS per wavefront: 128 DPT floats (keys | marks, then the scan row).
template <int DPT>
__global__ void __launch_bounds__(kBlock)
gauss_ring_kernel(const float *__restrict__ mus, const float *__restrict__ vars, const float *__restrict__ labels,
                  const int32_t *__restrict__ lens, int B, int L, int metric, int opt_ideal, int top_k, float const_var, float max_label,
                  const float *__restrict__ max_label_dev, float *__restrict__ loss_q, float *__restrict__ valid_q, float *__restrict__ ranks,
                  int32_t *__restrict__ pos_out, float *__restrict__ grad_mu, float *__restrict__ grad_var) {
    constexpr int RS = 64 * DPT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int q = blockIdx.x * (kBlock / kWave) + wv;
    const bool valid = q < B;
    const int n = __builtin_amdgcn_readfirstlane(valid ? query_len(lens, q, L) : 0);
    float *A = smem + (size_t)wv * (2 * RS), *S = A + RS;
    const size_t base = (size_t)q * L;

    float mi[DPT], vi[DPT], yi[DPT], r[DPT], none[DPT];
    int pos[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = lane + 64 * m;
        const bool in = i < n;
        mi[m] = in ? mus[base + i] : -1e30f;                      // padding: Phi = 0 and g = 0 against every real document
        vi[m] = in ? (vars ? vars[base + i] : const_var) : 1.0f;
        yi[m] = in ? labels[base + i] : 0.0f;
        pos[m] = i;
    }
    // ---- pass 1: expected ranks (prob_utils.py:70-73)
    gauss_ring<DPT, 1>(mi, vi, vi, lane, r, none);
#pragma unroll
    for (int m = 0; m < DPT; ++m) r[m] = lane + 64 * m < n ? r[m] : 0.0f;      // r_i; 0 on padding
    if (!opt_ideal) {                                             // hard positions: rank by (r ascending, index ascending)
        float key[DPT];
#pragma unroll
        for (int m = 0; m < DPT; ++m) {
            key[m] = lane + 64 * m < n ? -r[m] : -INFINITY;
            A[lane + 64 * m] = key[m];
        }
        wave_lds_sync();
        count_ranks_fast<kWave, DPT>(A, reinterpret_cast<int *>(S), n, lane, key, pos);
        const int last = n > 0 ? n - 1 : 0;
#pragma unroll
        for (int m = 0; m < DPT; ++m) pos[m] = min(max(pos[m], 0), last);     // NaN ranks (a variance <= 0): any order, but inside the rows
        wave_lds_sync();
    }
    // ---- the O(n) step: weights, loss, coefficients
    float W[DPT], u[DPT], gm[DPT], gv[DPT];
    const bool keep = smooth_weights<kWave, DPT>(S, nullptr, n, lane, metric, opt_ideal != 0, top_k,
                                                 metric == PTR_SMOOTH_NERR ? smooth_pow_max(max_label, max_label_dev) : 1.0f, yi, pos, W);
    float part = 0.0f;
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        float term = 0.0f;
        u[m] = 0.0f;
        if (lane + 64 * m < n) smooth_phi(metric, W[m], r[m], term, u[m]);
        part += term;
        gm[m] = 0.0f; gv[m] = 0.0f;
    }
    const float loss = 0.0f - wave_sum_dpp(part);
    // ---- pass 2: both gradients.  A list of one document has no pair: gradient 0 whatever its weight, as the reference's triu + tril
    // mask gives (tests/golden/gauss_metric.npz, edge/n1_norel)
    if (keep && n > 1) gauss_ring<DPT, 2>(mi, vi, u, lane, gm, gv);
    if (valid) {
#pragma unroll
        for (int m = 0; m < DPT; ++m) {
            const int i = lane + 64 * m;
            if (i < L) {
                const bool in = i < n;
                grad_mu[base + i] = in ? gm[m] : 0.0f;
                if (grad_var) grad_var[base + i] = in ? gv[m] : 0.0f;
                if (ranks) ranks[base + i] = r[m];
                if (pos_out) pos_out[base + i] = in ? pos[m] : -1;
            }
        }
        if (lane == 0) {
            loss_q[q] = keep ? loss : 0.0f;
            if (valid_q) valid_q[q] = keep ? 1.0f : 0.0f;
        }
    }
}

// One workgroup per query (G = 256), lists of up to 256 DPT documents: the one-sided walk.
template <int G, int DPT>
__global__ void __launch_bounds__(kBlock)
gauss_metric_kernel(const float *__restrict__ mus, const float *__restrict__ vars, const float *__restrict__ labels,
                    const int32_t *__restrict__ lens, int B, int L, int metric, int opt_ideal, int top_k, float const_var, float max_label,
                    const float *__restrict__ max_label_dev, float *__restrict__ loss_q, float *__restrict__ valid_q, float *__restrict__ ranks,
                    int32_t *__restrict__ pos_out, float *__restrict__ grad_mu, float *__restrict__ grad_var) {
    constexpr int QPB = kBlock / G, Lp = G * DPT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, grp = tid / G, t = tid % G;
    const int q = blockIdx.x * QPB + grp;
    const bool valid = q < B;
    const int n = __builtin_amdgcn_readfirstlane(valid ? query_len(lens, q, L) : 0);
    float *M = smem + (size_t)grp * gauss_group_floats(Lp), *V = M + Lp, *A = V + Lp, *S = A + Lp, *red = S + Lp;
    const size_t base = (size_t)q * L;

    float yi[DPT];
    int pos[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        const bool in = i < smooth_step_len<DPT>(n);
        M[i] = in ? mus[base + i] : 0.0f;
        V[i] = in ? (vars ? vars[base + i] : const_var) : 1.0f;
        yi[m] = in ? labels[base + i] : 0.0f;
        pos[m] = i;
    }
    group_sync<G>();

    // ---- pass 1: expected ranks (prob_utils.py:70-73)
#pragma unroll 1
    for (int i = t; i < n; i += G) {
        const float mi = M[i], vi = V[i];
        float s = 1.0f, c = 0.0f;
#pragma unroll 2
        for (int j = 0; j < n; ++j) {
            const float p = pair_phi(pair_geo(mi, vi, M[j], V[j]));
            kahan_add(s, c, j == i ? 0.0f : p);
        }
        A[i] = s;
    }
    group_sync<G>();
    float r[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        r[m] = i < smooth_step_len<DPT>(n) ? A[i] : 0.0f;         // r_i; 0 on padding
    }
    if (!opt_ideal) {                                             // hard positions: rank by (r ascending, index ascending)
        float key[DPT];
        group_sync<G>();
#pragma unroll
        for (int m = 0; m < DPT; ++m) {
            const int i = t + m * G;
            key[m] = i < smooth_step_len<DPT>(n) ? -r[m] : -INFINITY;
            A[i] = key[m];
        }
        group_sync<G>();
        count_ranks_fast<G, DPT>(A, reinterpret_cast<int *>(S), n, t, key, pos);
        const int last = n > 0 ? n - 1 : 0;
#pragma unroll
        for (int m = 0; m < DPT; ++m) pos[m] = min(max(pos[m], 0), last);     // NaN ranks (a variance <= 0): any order, but inside the rows
        group_sync<G>();
    }

    // ---- the O(n) step: weights, loss, coefficients
    float W[DPT], u[DPT];
    const bool keep = smooth_weights<G, DPT>(S, red, n, t, metric, opt_ideal != 0, top_k,
                                             metric == PTR_SMOOTH_NERR ? smooth_pow_max(max_label, max_label_dev) : 1.0f, yi, pos, W);
    float part = 0.0f;
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        float term = 0.0f;
        u[m] = 0.0f;
        if (t + m * G < smooth_step_len<DPT>(n)) smooth_phi(metric, W[m], r[m], term, u[m]);
        part += term;
    }
    const float loss = 0.0f - group_sum<G>(part, red, t);
    group_sync<G>();
#pragma unroll
    for (int m = 0; m < DPT; ++m) A[t + m * G] = u[m];
    group_sync<G>();

    // ---- pass 2: both gradients.  A document is no partner of itself: a list of one document has gradient 0 whatever its weight, as the
    // reference's triu + tril mask gives (tests/golden/gauss_metric.npz, edge/n1_norel)
    if (valid) {
#pragma unroll 1
        for (int i = t; i < n; i += G) {
            float gm = 0.0f, cm = 0.0f, gv = 0.0f, cv = 0.0f;
            if (keep) {
                const float mi = M[i], vi = V[i], ui = A[i];
#pragma unroll 2
                for (int j = 0; j < n; ++j) {
                    const PairGeo g = pair_geo(mi, vi, M[j], V[j]);
                    const float w = g.e2 * kInvSqrtPi * g.a;                   // phi a
                    const float d = A[j] - ui;
                    const float tm = w * d, tv = (w * (g.x * g.a)) * (0.0f - d);
                    kahan_add(gm, cm, j == i ? 0.0f : tm);
                    kahan_add(gv, cv, j == i ? 0.0f : tv);
                }
            }
            grad_mu[base + i] = gm;
            if (grad_var) grad_var[base + i] = gv;
        }
        for (int i = n + t; i < L; i += G) {
            grad_mu[base + i] = 0.0f;
            if (grad_var) grad_var[base + i] = 0.0f;
        }
#pragma unroll
        for (int m = 0; m < DPT; ++m) {
            const int i = t + m * G;
            if (i < L) {
                const bool in = i < smooth_step_len<DPT>(n);
                if (ranks) ranks[base + i] = r[m];
                if (pos_out) pos_out[base + i] = in ? pos[m] : -1;
            }
        }
        if (t == 0) {
            loss_q[q] = keep ? loss : 0.0f;
            if (valid_q) valid_q[q] = keep ? 1.0f : 0.0f;
        }
    }
}

}  // namespace ptr

extern "C" int ptr_gaussmetric_fwd_bwd(const float *mus, const float *vars, const float *labels, const int32_t *lens, int B, int L, int metric,
                                       int opt_ideal, int top_k, float const_std, float max_label, float *loss_out, float *loss_q, float *valid_q,
                                       float *ranks, int32_t *pos, float *max_label_ws, float *grad_mu, float *grad_var, void *stream) {
    using namespace ptr;
    const char *who = "ptr_gaussmetric_fwd_bwd";
    if (L > PTR_MAX_LIST_LEN) { set_error("%s: list length %d exceeds PTR_MAX_LIST_LEN=%d", who, L, PTR_MAX_LIST_LEN); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_loss_args(mus, labels, B, L, loss_q && grad_mu, who)) return rc;
    if (metric < PTR_SMOOTH_P || metric > PTR_SMOOTH_NDCG) { set_error("%s: metric %d (PTR_SMOOTH_P .. PTR_SMOOTH_NDCG)", who, metric); return PTR_ERR_INVALID_ARG; }
    if (!vars && !(const_std > 0.0f)) { set_error("%s: without vars, const_std must be > 0 (got %g)", who, (double)const_std); return PTR_ERR_INVALID_ARG; }
    if (vars && !grad_var) { set_error("%s: vars given without grad_var", who); return PTR_ERR_INVALID_ARG; }
    const bool dev_max = metric == PTR_SMOOTH_NERR && !(max_label >= 0.0f);
    if (dev_max && B > 0 && !max_label_ws) { set_error("%s: nERR with max_label < 0 needs the max_label_ws device scalar", who); return PTR_ERR_INVALID_ARG; }
    if (B > 0) {
        const float *ml_dev = nullptr;
        if (dev_max) {
            if (int rc = smooth_max_label_launch(labels, lens, B, L, max_label_ws, stream, who)) return rc;
            ml_dev = max_label_ws;
        }
        const float const_var = vars ? 0.0f : (float)((double)const_std * (double)const_std);     // the variance every document gets
        const RingForm f = ring_form(L);
        auto go = [&](auto kern, int QPB, size_t lds_floats) -> int {
            return launch_queries(kern, B, QPB, kBlock, lds_floats * sizeof(float), stream, who, mus, vars, labels, lens, B, L, metric, opt_ideal, top_k,
                                  const_var, max_label, ml_dev, loss_q, valid_q, ranks, pos, grad_mu, grad_var);
        };
        auto walk = [&]<int DPT>() { return go(gauss_metric_kernel<256, DPT>, 1, gauss_group_floats(kBlock * DPT)); };
        const int rc = f.ring     ? dispatch_ring_dpt(f.DPT, [&]<int DPT>() { return go(gauss_ring_kernel<DPT>, kBlock / kWave, (size_t)kBlock / kWave * 128 * DPT); })
                     : f.DPT == 4 ? walk.template operator()<4>()
                     : f.DPT == 8 ? walk.template operator()<8>()
                                  : walk.template operator()<16>();
        if (rc) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}
