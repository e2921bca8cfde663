// The O(n) step of the metric objectives (ptranking/metric/smooth_metric/metric_as_opt_objective.py): the weights W_i of P, AP, nERR and nDCG
// from the labels and the hard positions, phi(r) and its derivative, nERR's batch-wide maximum label — shared by the objectives on the
// sigmoid ranks (smoothmetric.hip) and on the Gaussian expected ranks (gaussmetric.hip).
#pragma once
#include "ptr_device.h"

namespace ptr {

// max over the valid documents' labels -> out[0], one launch of ONE workgroup (smoothmetric.hip)
int smooth_max_label_launch(const float *labels, const int32_t *lens, int B, int L, float *out, void *stream, const char *who);

#if defined(__HIPCC__)

enum { kScanPrefixSum = 0, kScanSuffixSum = 1, kScanPrefixProdExcl = 2 };

// In-place scan of row[0..n) (LDS) by ONE full wavefront: lane l owns the chunk [l ch, (l + 1) ch), ch = ceil(n / 64); a serial walk inside the
// chunk, the chunk totals scanned across the lanes, a second walk.  Inclusive sums, EXCLUSIVE product.  The order depends on n alone.
template <int MODE> __device__ __forceinline__ void wave_scan_row(float *row, int n, int lane) {
    const int ch = (n + 63) >> 6, lo = min(lane * ch, n), hi = min(lo + ch, n);
    float tot = MODE == kScanPrefixProdExcl ? 1.0f : 0.0f;
    for (int p = lo; p < hi; ++p) tot = MODE == kScanPrefixProdExcl ? tot * row[p] : tot + row[p];
    if constexpr (MODE == kScanPrefixSum) {
        float run = dpp_wave_shr1(wave_incl_sum(tot, lane));                       // lane 0 <- 0
        for (int p = lo; p < hi; ++p) { run += row[p]; row[p] = run; }
    } else if constexpr (MODE == kScanSuffixSum) {
        float run = dpp_wave_shl1(wave_incl_suffix_sum(tot, lane));                // lane 63 <- 0
        for (int p = hi - 1; p >= lo; --p) { run += row[p]; row[p] = run; }
    } else {
        const float before = dpp_wave_shr1(wave_incl_prod(tot, lane));
        float run = lane == 0 ? 1.0f : before;
        for (int p = lo; p < hi; ++p) { const float v = row[p]; row[p] = run; run *= v; }
    }
}

// The list length as one phase of the 16-documents-per-thread kernel compares against it.  The 16 lane masks `i < n` of an unrolled loop are
// invariants that the compiler computes once and keeps in 32 scalar registers for every later loop — more than that kernel has, so they were
// kept in VGPR lanes (v_writelane / v_readlane).  An opaque copy per phase (per step in the pair loops) makes each mask one v_cmp where it is
// used, and nothing has to stay live.
template <int DPT> __device__ __forceinline__ int smooth_step_len(int n) {
    if constexpr (DPT >= 16) asm volatile("" : "+v"(n));
    return n;
}

// The O(n) step: W[m] of document i = t + m G from its label y[m] and hard position pos[m]; returns whether the query contributes (the
// reference's pos_inds filter of the re-sorted top-k forms).  `row`: n floats of LDS owned by the group; red: 4 floats (G == 256).  Every
// thread of the group must call it.  pow_max = 2^max_label (nERR).
template <int G, int DPT>
__device__ __forceinline__ bool smooth_weights(float *row, float *red, int n, int t, int metric, bool ideal, int top_k, float pow_max,
                                               const float (&y)[DPT], const int (&pos)[DPT], float (&W)[DPT]) {
    const int K = top_k <= 0 ? n : min(top_k, n);
    const float kdiv = (float)(top_k <= 0 ? n : top_k);
    const bool filter = !ideal && top_k > 0;
    float b[DPT], gn[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        b[m] = fminf(fmaxf(y[m], 0.0f), 1.0f);
        gn[m] = gain_of(y[m]);
    }
    auto in = [&](int m) { return t + m * G < smooth_step_len<DPT>(n); };
    auto top = [&](int m) { return in(m) && pos[m] < K; };
    auto total = [&](auto f) {                                                     // sum over the group's documents, fixed order
        float part = 0.0f;
#pragma unroll
        for (int m = 0; m < DPT; ++m) part += f(m);
        return group_sum<G>(part, red, t);
    };
    auto scatter_scan = [&](auto f, auto mode, bool by_pos) {                      // row[position] = f(document), scanned; returns row[own]
        group_sync<G>();
#pragma unroll
        for (int m = 0; m < DPT; ++m)
            if (in(m)) row[by_pos ? pos[m] : t + m * G] = f(m);
        group_sync<G>();
        if (t < kWave) wave_scan_row<decltype(mode)::value>(row, n, t);
        group_sync<G>();
    };
    using std::integral_constant;
    float crit = 1.0f;
    if (metric == PTR_SMOOTH_P) {
        crit = total([&](int m) { return top(m) ? b[m] : 0.0f; });
#pragma unroll
        for (int m = 0; m < DPT; ++m) W[m] = top(m) ? (float)(pos[m] + 1) * b[m] / kdiv : 0.0f;
    } else if (metric == PTR_SMOOTH_AP) {
        if (!ideal && top_k <= 0) {                                                // :118-123: cumulative count of relevant documents
            scatter_scan([&](int m) { return b[m]; }, integral_constant<int, kScanPrefixSum>{}, true);
            const float S = total([&](int m) { return in(m) ? b[m] : 0.0f; });
#pragma unroll
            for (int m = 0; m < DPT; ++m) W[m] = top(m) ? b[m] * row[pos[m]] / S : 0.0f;
        } else {                                                                   // :92-94, :104-106, :140-143
            scatter_scan([&](int m) { return top(m) ? b[m] / (float)(pos[m] + 1) : 0.0f; }, integral_constant<int, kScanSuffixSum>{}, true);
            const float S = total([&](int m) { return top(m) ? b[m] : 0.0f; });
            crit = S;
#pragma unroll
            for (int m = 0; m < DPT; ++m) W[m] = top(m) ? (float)(pos[m] + 1) * row[pos[m]] / S : 0.0f;
        }
    } else if (metric == PTR_SMOOTH_NERR) {
        float sat[DPT], num[DPT];
#pragma unroll
        for (int m = 0; m < DPT; ++m) sat[m] = gn[m] / pow_max;                    // :176, :200
        scatter_scan([&](int m) { return 1.0f - sat[m]; }, integral_constant<int, kScanPrefixProdExcl>{}, true);
#pragma unroll
        for (int m = 0; m < DPT; ++m) num[m] = top(m) ? sat[m] * row[pos[m]] : 0.0f;
        if (!ideal) scatter_scan([&](int m) { return 1.0f - sat[m]; }, integral_constant<int, kScanPrefixProdExcl>{}, false);
        const float ideal_err = total([&](int m) {                                 // adhoc_metric.py:127-148 over the input (ideal) order
            const int i = t + m * G;
            return i < K ? sat[m] * row[i] / (float)(i + 1) : 0.0f;
        });
        crit = total([&](int m) { return top(m) ? y[m] : 0.0f; });
#pragma unroll
        for (int m = 0; m < DPT; ++m) W[m] = top(m) ? num[m] / ideal_err : 0.0f;
    } else {
        const float idcg = total([&](int m) { return in(m) ? gn[m] * inv_log2_pos(t + m * G) : 0.0f; });   // the WHOLE list, :216
        crit = total([&](int m) { return top(m) ? gn[m] : 0.0f; });
#pragma unroll
        for (int m = 0; m < DPT; ++m) W[m] = top(m) ? gn[m] / idcg : 0.0f;
    }
    group_sync<G>();                                                               // the caller may reuse `row`
    const bool keep = n > 0 && !(filter && crit == 0.0f);
    if (!keep) {
#pragma unroll
        for (int m = 0; m < DPT; ++m) W[m] = 0.0f;
    }
    return keep;
}

// phi(r) and c = -W phi'(r) of one document
__device__ __forceinline__ void smooth_phi(int metric, float W, float r, float &term, float &c) {
    if (metric == PTR_SMOOTH_NDCG) {
        const float lg = log2f(r + 1.0f);
        term = W / lg;                                                              // :221, :231
        c = W / (0.6931471805599453f * (1.0f + r) * lg * lg);
    } else {
        const float ri = 1.0f / r;
        term = W * ri;
        c = term * ri;
    }
}

__device__ __forceinline__ float smooth_pow_max(float max_label, const float *max_label_dev) {
    return exp2f(max_label_dev ? max_label_dev[0] : max_label);
}

#endif  // __HIPCC__
}  // namespace ptr
