// Smooth-rank metric objectives: P, AP, nERR and nDCG as optimisation objectives on the smooth ranks of ApproxNDCG.
//
// Reference: ptranking/metric/smooth_metric/metric_as_opt_objective.py:12-72 (precision_as_opt_objective), :75-145 (AP_as_opt_objective),
//            :148-210 (nERR_as_opt_objective), :213-257 (nDCG_as_opt_objective), fed with batch_smooth_ranks = get_approx_ranks
//            (ptranking/ltr_adhoc/listwise/approxNDCG.py:19-27), Robust_Sigmoid ptranking/base/utils.py:57-95, the ideal ERR
//            ptranking/metric/adhoc/adhoc_metric.py:127-148, the IDCG ptranking/metric/metric_utils.py (torch_dcg_at_k), and their autograd backward.
//
// Per query of n documents (labels presorted: the input order is the ideal order), all 16 forms (4 metrics x opt_ideal x top_k) collapse to
//   r_i    = 1 + sum_{j != i} rs(alpha (s_j - s_i))
//   loss   = - sum_i W_i phi(r_i),      phi(r) = 1 / r (P, AP, nERR)  or  1 / log2(1 + r) (nDCG)
//   grad_k = sum_i c_i d_ik - c_k sum_j d_kj,      c_i = -W_i phi'(r_i),   d_ij = alpha y_ij (1 - y_ij)
// with weights W_i that are constants of the backward: they depend on the labels and on the HARD position pos_i of document i only (the input
// index under opt_ideal, else the rank by score descending with index tie-break — the order of the reference's torch.sort of the smooth ranks,
// which decrease strictly with the score).  include/ptranking_amd.h lists W per form.
//
// The kernels are ApproxNDCG's two O(n^2) passes (approxndcg.hip) with an O(n) step between them:
//   pass 1   smooth ranks (and, for the re-sorted forms, the hard positions: a rank count before it);
//   O(n)     labels scattered to their positions in LDS, one scan by ONE wavefront (suffix sum for AP, prefix count for the full-list re-sorted
//            AP, exclusive prefix product for nERR), W_i, the loss and c_i;
//   pass 2   the gradient from the pair derivatives.
// Lists of up to 512 documents: one wavefront per query, both passes out of registers (approx_ring, ptr_rsig.h: the ring of
// approxndcg_ring_kernel; padding records carry s = -1e30, c = 0).  Up to PTR_MAX_LIST_LEN: one workgroup per query, scores in LDS, the partner's share
// of a pair accumulated in one LDS row per wavefront, the rank indicators in fixed point (exact integer additions: see pass 1 there).  Nothing
// of size n x n exists and there are no atomics; every sum has a fixed order given (n, L): a query's outputs do not depend on the rest of the
// batch or on the run.
#include "ptr_device.h"
#include "ptr_rsig.h"
#include "ptr_smooth.h"     // wave_scan_row, smooth_weights, smooth_phi, smooth_pow_max

namespace ptr {

// One wavefront per query, lists of up to 64 DPT <= 512 documents.  LDS per wavefront: 128 DPT floats (the scan row | the rank count's marks).
template <int DPT>
__global__ void __launch_bounds__(kBlock)
smooth_ring_kernel(const float *__restrict__ preds, const float *__restrict__ labels, const int32_t *__restrict__ lens, int B, int L, int metric,
                   int opt_ideal, int top_k, float alpha, float max_label, const float *__restrict__ max_label_dev,
                   float *__restrict__ loss_q, float *__restrict__ valid_q, float *__restrict__ ranks, float *__restrict__ grad) {
    constexpr int RS = 64 * DPT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int q = blockIdx.x * (kBlock / kWave) + wv;
    const bool valid = q < B;
    const int n = __builtin_amdgcn_readfirstlane(valid ? query_len(lens, q, L) : 0);
    float *row = smem + (size_t)wv * (2 * RS);
    int *mark = reinterpret_cast<int *>(row + RS);

    float si[DPT], yi[DPT];
    int pos[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = lane + 64 * m;
        const bool in = i < n;
        si[m] = in ? preds[(size_t)q * L + i] : -INFINITY;
        yi[m] = in ? labels[(size_t)q * L + i] : 0.0f;
        pos[m] = i;
    }
    if (!opt_ideal) {                                             // hard positions: rank by (score descending, index ascending)
#pragma unroll
        for (int m = 0; m < DPT; ++m) row[lane + 64 * m] = si[m];
        wave_lds_sync();
        count_ranks_fast<kWave, DPT>(row, mark, n, lane, si, pos);
        wave_lds_sync();
    }
#pragma unroll
    for (int m = 0; m < DPT; ++m) si[m] = lane + 64 * m < n ? si[m] : -1e30f;

    const float c2 = alpha * 1.4426950408889634f;
    float pia[DPT], W[DPT], ca[DPT], tot[DPT];
    approx_ring<DPT, 1>(si, si, c2, alpha, lane, pia);
    const bool keep = smooth_weights<kWave, DPT>(row, nullptr, n, lane, metric, opt_ideal != 0, top_k,
                                                 metric == PTR_SMOOTH_NERR ? smooth_pow_max(max_label, max_label_dev) : 1.0f, yi, pos, W);
    float part = 0.0f;
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const bool in = lane + 64 * m < n;
        pia[m] = in ? pia[m] + 1.0f : 0.0f;                       // r_i; 0 on padding
        float term = 0.0f;
        ca[m] = 0.0f;
        if (in) smooth_phi(metric, W[m], pia[m], term, ca[m]);
        part += term;
        tot[m] = 0.0f;
    }
    const float loss = 0.0f - wave_sum_dpp(part);
    if (keep && n > 1) approx_ring<DPT, 2>(si, ca, c2, alpha, lane, tot);
    // n == 1: no pair.  The reference's backward still passes +c and -c through the diagonal of its difference matrix: exactly 0 for a finite
    // c, NaN where the only document is irrelevant and W = 0 / 0 (tests/golden/smooth_metric.npz, edge/n1_norel)
    if (n == 1) tot[0] = ca[0] - ca[0];
    if (valid) {
#pragma unroll
        for (int m = 0; m < DPT; ++m) {
            const int i = lane + 64 * m;
            if (i < L) {
                grad[(size_t)q * L + i] = i < n ? tot[m] : 0.0f;
                if (ranks) ranks[(size_t)q * L + i] = pia[m];
            }
        }
        if (lane == 0) {
            loss_q[q] = keep ? loss : 0.0f;
            if (valid_q) valid_q[q] = keep ? 1.0f : 0.0f;
        }
    }
}

// One workgroup per query, lists of up to 256 DPT documents (DPT = 4, 8, 16: 513 .. PTR_MAX_LIST_LEN).
// LDS (floats), Lp = 256 DPT: S[Lp] | C[Lp] | acc[4][Lp] | red[4] (24, 48, 96 KiB); C is the scan row of the O(n) step, then the coefficients; acc row 0 is the rank count's
// mark row before pass 1.
__host__ __device__ constexpr size_t smooth_lds_floats(int Lp) { return (size_t)Lp * 6 + 4; }

template <int DPT>
__global__ void __launch_bounds__(kBlock)
smooth_lds_kernel(const float *__restrict__ preds, const float *__restrict__ labels, const int32_t *__restrict__ lens, int B, int L,
                  int metric, int opt_ideal, int top_k, float alpha, float max_label, const float *__restrict__ max_label_dev,
                  float *__restrict__ loss_q, float *__restrict__ valid_q, float *__restrict__ ranks, float *__restrict__ grad) {
    constexpr int G = kBlock, NW = G / kWave, Lp = G * DPT;       // rows of the full tile: every thread's slots exist, no `i < Lp` lane masks
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int t = threadIdx.x, wv = t >> 6;
    const int q = blockIdx.x;
    const int n = query_len(lens, q, L);
    float *S = smem, *Cc = smem + Lp, *acc = smem + 2 * (size_t)Lp, *red = acc + (size_t)NW * Lp;

    float si[DPT], yi[DPT];
    int pos[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        const bool in = i < smooth_step_len<DPT>(n);
        si[m] = in ? preds[(size_t)q * L + i] : -INFINITY;
        yi[m] = in ? labels[(size_t)q * L + i] : 0.0f;
        pos[m] = i;
        if (i < Lp) S[i] = si[m];
    }
    __syncthreads();
    if (!opt_ideal) {
        count_ranks_fast<G, DPT>(S, reinterpret_cast<int *>(acc), n, t, si, pos);
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        if (i < Lp) {
#pragma unroll
            for (int w = 0; w < NW; ++w) acc[(size_t)w * Lp + i] = 0.0f;
        }
    }
    __syncthreads();

    float *aw = acc + (size_t)wv * Lp;
    const int half = (n - 1) >> 1;
    // ---- pass 1: every unordered pair once (circulant half matrix), both indicators from one exponential.
    // The indicators are summed in FIXED POINT: an fp32 chain of n / 2 additions that grows to r ~ n loses ~sqrt(n / 2) ulp(r) / 2 (1.3e-3 at
    // n = 2048, more than the sigmoids' own error); integer additions are exact, so a rank carries one rounding per indicator (half a
    // quantum, 2^-26 for n <= 64 up to 2^-21 at n = 4096, against an fp32 sigmoid's 2^-25 near 1) and one at the end, in any order.
    // scale = 2^(32 - ceil(log2 n)) <= 2^25: the n - 1 indicators of a document, each <= 1, sum below 2^32.
    int lgn = 1;
    while ((1 << lgn) < n) ++lgn;
    const float scale = __builtin_amdgcn_exp2f((float)min(32 - lgn, 25)), inv_scale = __builtin_amdgcn_exp2f(-(float)min(32 - lgn, 25));
    uint32_t *awu = reinterpret_cast<uint32_t *>(aw);
    const uint32_t *accu = reinterpret_cast<const uint32_t *>(acc);
    uint32_t piu[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) piu[m] = 0u;
    for (int d = 1; d <= half; ++d) {
        const int nv = smooth_step_len<DPT>(n);
#pragma unroll
        for (int m = 0; m < DPT; ++m) {
            const int a = t + m * G;
            if (a < nv) {
                int b = a + d; if (b >= n) b -= n;
                float ya, yb;
                robust_pair(S[b] - si[m], alpha, ya, yb);
                piu[m] += __float2uint_rn(ya * scale);
                awu[b] += __float2uint_rn(yb * scale);            // per-wave row, distinct b per lane
            }
        }
    }
    if (n > 0 && (n & 1) == 0) {
        const int d = n >> 1;
#pragma unroll
        for (int m = 0; m < DPT; ++m) {
            const int a = t + m * G;
            if (a < d) {
                float ya, yb;
                robust_pair(S[a + d] - si[m], alpha, ya, yb);
                piu[m] += __float2uint_rn(ya * scale);
                awu[a + d] += __float2uint_rn(yb * scale);
            }
        }
    }
    __syncthreads();
    float pia[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int a = t + m * G;
        pia[m] = 0.0f;
        if (a < smooth_step_len<DPT>(n)) {
            uint64_t tot = (uint64_t)piu[m] + (uint64_t)scale;    // + 1: the rank itself, still exact
#pragma unroll
            for (int w = 0; w < NW; ++w) tot += accu[(size_t)w * Lp + a];
            pia[m] = (float)tot * inv_scale;                      // r_i
        }
    }
    float W[DPT], ca[DPT];
    const bool keep = smooth_weights<G, DPT>(Cc, red, n, t, metric, opt_ideal != 0, top_k,
                                             metric == PTR_SMOOTH_NERR ? smooth_pow_max(max_label, max_label_dev) : 1.0f, yi, pos, W);
    float part = 0.0f;
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int a = t + m * G;
        float term = 0.0f;
        ca[m] = 0.0f;
        if (a < smooth_step_len<DPT>(n)) smooth_phi(metric, W[m], pia[m], term, ca[m]);
        part += term;
    }
    const float loss = 0.0f - group_sum<G>(part, red, t);     // (its barriers fence the reuse of `acc` and `Cc`)
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int a = t + m * G;
        if (a < Lp) {
            Cc[a] = ca[m];
#pragma unroll
            for (int w = 0; w < NW; ++w) acc[(size_t)w * Lp + a] = 0.0f;
        }
    }
    __syncthreads();

    // ---- pass 2: entry (a, b): r_a depends on s_b with +d_ab and on s_a with -d_ab
    float ga[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) ga[m] = 0.0f;
    auto gpair = [&](int m, int b) {
        float ya, yb;
        robust_pair(S[b] - si[m], alpha, ya, yb);
        const float dab = (alpha * ya) * (1.0f - ya);             // base/utils.py:78
        const float dba = (alpha * yb) * (1.0f - yb);
        const float flow = Cc[b] * dba - ca[m] * dab;
        ga[m] += flow;
        aw[b] -= flow;
    };
    if (keep) {                                                   // uniform over the workgroup
        for (int d = 1; d <= half; ++d) {
            const int nv = smooth_step_len<DPT>(n);
#pragma unroll
            for (int m = 0; m < DPT; ++m) {
                const int a = t + m * G;
                if (a < nv) { int b = a + d; if (b >= n) b -= n; gpair(m, b); }
            }
        }
        if (n > 0 && (n & 1) == 0) {
            const int d = n >> 1;
#pragma unroll
            for (int m = 0; m < DPT; ++m) {
                const int a = t + m * G;
                if (a < d) gpair(m, a + d);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        if (i < L) {
            float tot = ga[m];
            if (i < smooth_step_len<DPT>(n)) {
#pragma unroll
                for (int w = 0; w < NW; ++w) tot += acc[(size_t)w * Lp + i];
                if (n == 1) tot = ca[m] - ca[m];                  // as the ring kernel: 0, or NaN with c
            }
            grad[(size_t)q * L + i] = i < smooth_step_len<DPT>(n) ? tot : 0.0f;
            if (ranks) ranks[(size_t)q * L + i] = pia[m];
        }
    }
    if (t == 0) {
        loss_q[q] = keep ? loss : 0.0f;
        if (valid_q) valid_q[q] = keep ? 1.0f : 0.0f;
    }
}

// max over the valid documents' labels -> out[0], ONE workgroup (no atomics, one float of workspace): nERR's batch-wide max_label (:151).
// Wavefront w takes the rows w, w + 16, ...; its lanes stride over the row's valid documents (coalesced, no index division).
__global__ void __launch_bounds__(1024)
smooth_max_label_kernel(const float *__restrict__ labels, const int32_t *__restrict__ lens, int B, int L, float *__restrict__ out) {
    __shared__ float red[16];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float v = -INFINITY;
    for (int q = wv; q < B; q += 16) {
        const int n = query_len(lens, q, L);
        const float *row = labels + (size_t)q * L;
        for (int i = lane; i < n; i += 64) v = fmaxf(v, row[i]);
    }
    v = wave_max(v);
    if (lane == 0) red[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float r = red[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) r = fmaxf(r, red[w]);
        out[0] = r;
    }
}

int smooth_max_label_launch(const float *labels, const int32_t *lens, int B, int L, float *out, void *stream, const char *who) {
    hipLaunchKernelGGL(smooth_max_label_kernel, dim3(1), dim3(1024), 0, as_stream(stream), labels, lens, B, L, out);
    return check_hip(hipGetLastError(), who);
}

}  // namespace ptr

extern "C" int ptr_smoothmetric_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, int metric, int opt_ideal,
                                        int top_k, float alpha, float max_label, float *loss_out, float *loss_q, float *valid_q, float *ranks,
                                        float *max_label_ws, float *grad, void *stream) {
    using namespace ptr;
    const char *who = "ptr_smoothmetric_fwd_bwd";
    if (L > PTR_MAX_LIST_LEN) { set_error("%s: list length %d exceeds PTR_MAX_LIST_LEN=%d", who, L, PTR_MAX_LIST_LEN); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_loss_args(preds, labels, B, L, loss_q && grad, who)) return rc;
    if (metric < PTR_SMOOTH_P || metric > PTR_SMOOTH_NDCG) { set_error("%s: metric %d (PTR_SMOOTH_P .. PTR_SMOOTH_NDCG)", who, metric); return PTR_ERR_INVALID_ARG; }
    if (!(alpha > 0.0f)) { set_error("%s: alpha must be > 0 (got %g)", who, (double)alpha); return PTR_ERR_INVALID_ARG; }
    const bool dev_max = metric == PTR_SMOOTH_NERR && !(max_label >= 0.0f);
    if (dev_max && B > 0 && !max_label_ws) { set_error("%s: nERR with max_label < 0 needs the max_label_ws device scalar", who); return PTR_ERR_INVALID_ARG; }
    if (B > 0) {
        const float *ml_dev = nullptr;
        if (dev_max) {
            if (int rc = smooth_max_label_launch(labels, lens, B, L, max_label_ws, stream, who)) return rc;
            ml_dev = max_label_ws;
        }
        const RingForm f = ring_form(L);
        auto go = [&](auto kern, int QPB, size_t lds_floats) -> int {
            return launch_queries(kern, B, QPB, kBlock, lds_floats * sizeof(float), stream, who, preds, labels, lens, B, L, metric, opt_ideal, top_k,
                                  alpha, max_label, ml_dev, loss_q, valid_q, ranks, grad);
        };
        auto walk = [&]<int DPT>() { return go(smooth_lds_kernel<DPT>, 1, smooth_lds_floats(kBlock * DPT)); };
        const int rc = f.ring     ? dispatch_ring_dpt(f.DPT, [&]<int DPT>() { return go(smooth_ring_kernel<DPT>, kBlock / kWave, (size_t)kBlock / kWave * 128 * DPT); })
                     : f.DPT == 4 ? walk.template operator()<4>()
                     : f.DPT == 8 ? walk.template operator()<8>()
                                  : walk.template operator()<16>();
        if (rc) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}
