// The tree frame's custom objectives (the reference's ltr_tree frame): the gradient AND the Hessian per document that LightGBM asks a custom
// objective for every boosting round, over LightGBM's ragged layout (flat arrays + group sizes).  The boosting itself stays in LightGBM.
//
// Reference: ptranking/ltr_tree/util/lightgbm_util.py:120-183 (per_query_gradient_hessian_lambda: a Python loop over document pairs),
//            :17-60 (triu_indice: the four pair masks), :82-118 (ideal_dcg, get_delta_gains, get_delta_ndcg), :308-330
//            (per_query_gradient_hessian_listnet), :185-389 (the six wrappers that walk `group`).
//
// What reading the reference turned up (include/ptranking_amd.h states which entry point each concerns; DESIGN.md has the whole list):
//   1. the lambdarank wrappers pass weighting=True, which the per-query function never recognises ('True in [DeltaNDCG, DeltaGain]' is
//      false): the weights are a separate argument here (PTR_TREE_W_*), and the drop-in passes PTR_TREE_W_NONE;
//   2. the Hessian is signed by rank order: for a pair at sorted positions r < c, hess[r] += h and hess[c] -= h (PTR_TREE_HESS_REFERENCE);
//      PTR_TREE_HESS_SUM adds h to both, as LightGBM and XGBoost do;
//   3. the Hessian's sigmoid ignores epsilon: epsilon^2 s(d)(1 - s(d)) with s at epsilon 1, floored at 1e-16 BEFORE the weight;
//   5. the reference's sort is not stable; here a higher score ranks first and equal scores rank by original index, the rule
//      ptr_lambdarank_fwd_bwd documents.
//
// Closed form per document i, over the partners j != i of its query that pass the pair mask (d = s_i - s_j, s() the logistic function):
//   grad_i = sum_j w_ij epsilon (s(epsilon d) - (1 + clip(y_i - y_j, -1, 1)) / 2)
//   h_ij   = max(epsilon^2 s(d) (1 - s(d)), 1e-16) w_ij
//   hess_i = sum_j h_ij [j ranks below i] - sum_j h_ij [j ranks above i]     (REFERENCE)         hess_i = sum_j h_ij     (SUM)
//   w_ij   = 1 | |G_i - G_j| |D_i - D_j| (G = (2^y - 1) / IDCG, D = 1 / log2(rank + 2), rank 0-based in predicted order) | |g_i - g_j| (g = 2^y - 1)
// Both sums are symmetric in (i, j), so ONE thread owns document i (strided where the list is longer than the group), walks all its partners
// in index order and writes its own two results: no atomics, nothing of size n x n, and the order of every floating-point addition depends
// on the query alone — not on the form that runs it, the batch around it or the launch.  The group-wide sums (IDCG, the softmax
// normalisers) are a halving tree over LDS whose shape depends on n alone, for the same reason.
//
// Forms (G threads per query, 256 / G queries per workgroup), chosen by the longest list of the launch:
//   G = 16   n <= 16      sixteen short queries per workgroup
//   G = 64   n <= 128     one wavefront per query, four per workgroup
//   G = 256  n <= 4096    one workgroup per query (PTR_MAX_LIST_LEN)
// The host buckets its queries by length class once and launches each class through the `queries` index list (ptranking_amd/tree.py).
// LDS per query: K rows of round_up(max_len, 4) floats — scores | labels | (normalised) gains | discounts; K = 2 (no weights), 3 (DeltaGain),
// 4 (DeltaNDCG): at most 16 round_up(n, 4) bytes.  ListNet: scores | gains | the tree's row.  XE-nDCG: scores | the tree's row.
#include "ptr_device.h"
#include "ptr_plhash.h"

namespace ptr {

__host__ __device__ constexpr int tree_rows(int W) { return W == PTR_TREE_W_DELTA_NDCG ? 4 : W == PTR_TREE_W_DELTA_GAIN ? 3 : 2; }

// Does any thread of the group hold `pred`?  (G == 256: a workgroup barrier as well: every thread of the block must call it.)
template <int G> __device__ __forceinline__ bool group_any(bool pred, int tid) {
    if constexpr (G == kBlock) return __syncthreads_or(pred) != 0;
    else if constexpr (G == kWave) return __any(pred) != 0;
    else return ((__ballot(pred) >> ((tid & (kWave - 1)) & ~(G - 1))) & ((1ull << G) - 1)) != 0;
}
// x[0] = op over x[0 .. n), in place: halves of ceil(m / 2) folded onto each other.  The tree's shape depends on n alone, so the result does
// not depend on G.  Within a level the entries written ([0, m - h)) and read ([h, m)) do not overlap.  Starts and ends with a group barrier;
// the caller reads x[0] and passes another barrier before it reuses the row.
template <int G, class Op> __device__ __forceinline__ void group_tree(float *x, int n, int t, Op op) {
    group_sync<G>();
    for (int m = n; m > 1;) {
        const int h = (m + 1) >> 1;
        for (int i = t; i + h < m; i += G) x[i] = op(x[i], x[i + h]);
        m = h;
        group_sync<G>();
    }
}

// Max and normaliser of the softmax of row[0 .. n) (_softmax, lightgbm_util.py:5-11), both by the tree over the scratch row T; every thread of
// the group gets the same two values.  Starts with a group barrier; the caller passes another before it writes T again.
template <int G> __device__ __forceinline__ void softmax_parts(const float *row, float *T, int n, int t, float &mx, float &z) {
    group_sync<G>();
    for (int i = t; i < n; i += G) T[i] = row[i];
    group_tree<G>(T, n, t, [](float a, float b) { return fmaxf(a, b); });
    mx = n > 0 ? T[0] : 0.0f;
    group_sync<G>();
    for (int i = t; i < n; i += G) T[i] = expf(row[i] - mx);
    group_tree<G>(T, n, t, [](float a, float b) { return a + b; });
    z = n > 0 ? T[0] : 1.0f;
}

// The query of this group: its first document and its length.  A query longer than the launch's max_len (the caller's error: the LDS rows
// are sized by max_len) is not evaluated: its documents receive NaN.
struct TreeQuery { int64_t base; int n; };
template <int G>
__device__ __forceinline__ TreeQuery tree_query(const int64_t *__restrict__ offsets, int B, const int32_t *__restrict__ queries, int nq, int max_len, int t,
                                                float *__restrict__ grad, float *__restrict__ hess) {
    constexpr int QPB = kBlock / G;
    const int gq = blockIdx.x * QPB + (int)threadIdx.x / G;
    TreeQuery r{0, 0};
    if (gq >= nq) return r;
    const int q = queries ? queries[gq] : gq;
    if (q < 0 || q >= B) return r;
    r.base = offsets[q];
    const int64_t len = offsets[q + 1] - r.base;
    if (len > (int64_t)max_len) {
        for (int64_t i = t; i < len; i += G) { grad[r.base + i] = NAN; hess[r.base + i] = NAN; }
        return r;
    }
    r.n = len < 0 ? 0 : (int)len;
    return r;
}

// 1 / (1 + e) (the LambdaRank kernels' form, pairwise.hip)
__device__ __forceinline__ float rcp1p(float e) { return rcp_nr(1.0f + e); }

// pmask: bit (2 [y_i == y_j] + [y_i == y_j == 0]) set where the pair type keeps the pair (triu_indice, lightgbm_util.py:17-60)
template <int G, int W, int H>
__global__ void __launch_bounds__(kBlock)
tree_pair_kernel(const float *__restrict__ preds, const float *__restrict__ labels, const int64_t *__restrict__ offsets, int B,
                 const int32_t *__restrict__ queries, int nq, int Lp, int max_len, int pmask, float eps, float *__restrict__ grad,
                 float *__restrict__ hess) {
    constexpr int K = tree_rows(W);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, grp = tid / G, t = tid % G;
    const TreeQuery qu = tree_query<G>(offsets, B, queries, nq, max_len, t, grad, hess);
    const int64_t base = qu.base;
    const int n = G >= kWave ? __builtin_amdgcn_readfirstlane(qu.n) : qu.n;

    float *S = smem + (size_t)grp * K * Lp, *Y = S + Lp;
    float *A = S + (size_t)Lp * (K > 2 ? 2 : 0), *D = S + (size_t)Lp * (K > 3 ? 3 : 0);

    // ---- stage the scores and the labels; both rows are padded with -inf up to a multiple of 4 (count_ranks reads float4)
    bool bad = false;
    const int np = (n + 3) & ~3;
    for (int i = t; i < np; i += G) {
        const float s = i < n ? preds[base + i] : -INFINITY, y = i < n ? labels[base + i] : -INFINITY;
        S[i] = s; Y[i] = y;
        bad |= s != s || y != y;
    }
    // a NaN score or label gives the list no ranking: NaN on every document of this list, and of no other (COVERAGE a9)
    const bool nanq = group_any<G>(bad, tid);
    group_sync<G>();

    if constexpr (W == PTR_TREE_W_DELTA_NDCG) {
        // IDCG from the exact label ranks (ideal_dcg, lightgbm_util.py:82-94), summed by the tree
        for (int i = t; i < n; i += G) {
            const float own[1] = {Y[i]};
            int rk[1];
            count_ranks<G, 1>(Y, n, i, own, rk);
            D[i] = gain_of(own[0]) * inv_log2_pos(rk[0]);
        }
        group_tree<G>(D, n, t, [](float a, float b) { return a + b; });
        const float idcg = n > 0 ? D[0] : 1.0f;
        group_sync<G>();
        for (int i = t; i < n; i += G) {
            const float own[1] = {S[i]};
            int rk[1];
            count_ranks<G, 1>(S, n, i, own, rk);
            A[i] = gain_of(Y[i]) / idcg;                       // 0 / 0 without a relevant document: NaN wherever a pair reads it, as the reference
            D[i] = inv_log2_pos(rk[0]);                        // get_delta_ndcg, :103-118
        }
        group_sync<G>();
    } else if constexpr (W == PTR_TREE_W_DELTA_GAIN) {
        for (int i = t; i < n; i += G) A[i] = gain_of(Y[i]);   // get_delta_gains, :96-101
        group_sync<G>();
    }

    const bool eps_one = eps == 1.0f;
    const float eps2 = eps * eps;
    for (int i = t; i < n; i += G) {
        const float si = S[i], yi = Y[i];
        const float ai = K > 2 ? A[i] : 0.0f, di = K > 3 ? D[i] : 0.0f;
        const bool yi0 = yi == 0.0f;
        float g = 0.0f, h = 0.0f;
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const float sj = S[j], yj = Y[j];
            const float ds = si - sj;                          // the difference first, epsilon after: rounds relative to |ds|, not to |s|
            const bool tie = yi == yj;
            const bool pass = ((pmask >> ((tie ? 2 : 0) + (tie && yi0 ? 1 : 0))) & 1) != 0 && j != i;
            // e / (1 + e)^2 = s(d)(1 - s(d)) without the cancellation of 1 - s; at epsilon 1 the gradient's sigmoid shares e and r
            const float e1 = __expf(-fabsf(ds));
            const float r1 = rcp1p(e1);
            float p;
            if (eps_one) {
                p = ds >= 0.0f ? r1 : e1 * r1;
            } else {
                const float x = eps * ds;
                const float e = __expf(-fabsf(x));
                const float r = rcp1p(e);
                p = x >= 0.0f ? r : e * r;
            }
            const float tt = 0.5f * (1.0f + __builtin_amdgcn_fmed3f(yi - yj, -1.0f, 1.0f));
            float w = 1.0f;
            if constexpr (W == PTR_TREE_W_DELTA_NDCG) w = fabsf(ai - A[j]) * fabsf(di - D[j]);
            if constexpr (W == PTR_TREE_W_DELTA_GAIN) w = fabsf(ai - A[j]);
            const float lam = w * (eps * (p - tt));            // :162-163
            g += pass ? lam : 0.0f;
            if constexpr (H != PTR_TREE_HESS_CONSTANT) {
                float hv = fmaxf(eps2 * (e1 * r1 * r1), 1e-16f) * w;                  // :171-173
                if constexpr (H == PTR_TREE_HESS_REFERENCE) {
                    const bool below = ds > 0.0f || (ds == 0.0f && j > i);            // j ranks below i: +h to i (:177-178)
                    hv = below ? hv : -hv;
                }
                h += pass ? hv : 0.0f;
            }
        }
        grad[base + i] = nanq ? NAN : g;
        hess[base + i] = H == PTR_TREE_HESS_CONSTANT ? 1.0f : (nanq ? NAN : h);
    }
}

// ListNet: grad = softmax(s) - softmax(gain), hess = p (1 - p) (per_query_gradient_hessian_listnet, lightgbm_util.py:308-330).
// LDS per query: scores | gains | the tree's row.
template <int G>
__global__ void __launch_bounds__(kBlock)
tree_listnet_kernel(const float *__restrict__ preds, const float *__restrict__ labels, const int64_t *__restrict__ offsets, int B,
                    const int32_t *__restrict__ queries, int nq, int Lp, int max_len, int power_gain, int const_hess, float *__restrict__ grad,
                    float *__restrict__ hess) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, grp = tid / G, t = tid % G;
    const TreeQuery qu = tree_query<G>(offsets, B, queries, nq, max_len, t, grad, hess);
    const int64_t base = qu.base;
    const int n = G >= kWave ? __builtin_amdgcn_readfirstlane(qu.n) : qu.n;
    float *S = smem + (size_t)grp * 3 * Lp, *Y = S + Lp, *T = Y + Lp;

    bool bad = false;
    for (int i = t; i < n; i += G) {
        const float s = preds[base + i], y = labels[base + i];
        S[i] = s; Y[i] = power_gain ? gain_of(y) : y;
        bad |= s != s || y != y;
    }
    const bool nanq = group_any<G>(bad, tid);

    float ms, zs, my, zy;
    softmax_parts<G>(S, T, n, t, ms, zs);
    softmax_parts<G>(Y, T, n, t, my, zy);
    for (int i = t; i < n; i += G) {
        const float pp = expf(S[i] - ms) / zs, pt = expf(Y[i] - my) / zy;
        grad[base + i] = nanq ? NAN : pp - pt;
        hess[base + i] = const_hess ? 1.0f : (nanq ? NAN : pp * (1.0f - pp));
    }
}

// ---- Cross-entropy nDCG, LightGBM's rank_xendcg (ptr_tree_xendcg_grad_hess; include/ptranking_amd.h states the rule).  The rule is this
// project's own, written after LightGBM's RankXENDCG; nothing here is compared with LightGBM.  O(n) per query: a softmax and three more
// tree sums (P, A, Bs).  LDS per query: 2 rows of Lp words (scores | the tree's row): 32 KiB at 4096 documents.  A thread owns the documents
// t, t + G, ... (at most K of them: tree_form gives the launch the smallest K in 1, 2, 4, 8, 16 that covers its longest list, so the
// length classes of the host each get a kernel without idle slots) and keeps rho, q and the running terms of each in registers across
// the three passes.  Neither G nor K touches a result: every sum is a tree over n.
constexpr float kXeFloor = 0x1p-20f;               // the floor of 1 - rho

// sum of v over the documents of the group, by the tree over T; every thread gets the same value
template <int G, int K> __device__ __forceinline__ float owned_sum(float *T, const float (&v)[K], int n, int t) {
    group_sync<G>();                                // the readers of the previous T[0] are done
#pragma unroll
    for (int k = 0; k < K; ++k)
        if (t + k * G < n) T[t + k * G] = v[k];
    group_tree<G>(T, n, t, [](float a, float b) { return a + b; });
    return n > 0 ? T[0] : 0.0f;
}

template <int G, int K>
__global__ void __launch_bounds__(kBlock)
tree_xendcg_kernel(const float *__restrict__ preds, const float *__restrict__ labels, const int64_t *__restrict__ offsets, int B,
                   const int32_t *__restrict__ queries, int nq, int Lp, int max_len, const float *__restrict__ unif, uint64_t seed,
                   int64_t draw, float *__restrict__ grad, float *__restrict__ hess) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, grp = tid / G, t = tid % G;
    const TreeQuery qu = tree_query<G>(offsets, B, queries, nq, max_len, t, grad, hess);
    const int64_t base = qu.base;
    const int n = G >= kWave ? __builtin_amdgcn_readfirstlane(qu.n) : qu.n;
    float *S = smem + (size_t)grp * 2 * Lp, *T = S + Lp;

    // ---- stage the scores; phi = 2^y - u from the label and the document's uniform (its global index keys the stream)
    const PlKeys round_keys = pl_query_keys(seed, draw);
    float rho[K], q[K], g[K], v[K];
    bool bad = false;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = t + k * G;
        v[k] = 0.0f;
        if (i < n) {
            const uint64_t d = (uint64_t)(base + i);
            const float s = preds[base + i], y = labels[base + i];
            const float u = unif ? unif[base + i] : pl_uniform(pl_sample_keys(round_keys, (uint32_t)(d >> 32)), (uint32_t)d);
            S[i] = s;
            v[k] = exp2f(y) - u;
            bad |= s != s || !(y >= 0.0f) || !(u >= 0.0f && u < 1.0f);
        }
    }
    // a NaN score or label, a negative label or a uniform outside [0, 1): NaN on every document of this list, and of no other
    const bool nanq = group_any<G>(bad, tid);

    float ms, zs;
    softmax_parts<G>(S, T, n, t, ms, zs);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = t + k * G;
        rho[k] = i < n ? expf(S[i] - ms) / zs : 0.0f;
        q[k] = fmaxf(1.0f - rho[k], kXeFloor);
    }
    const float P = owned_sum<G, K>(T, v, n, t);
#pragma unroll
    for (int k = 0; k < K; ++k) {                   // first order
        g[k] = rho[k] - v[k] / P;
        v[k] = g[k] / q[k];
    }
    const float A = owned_sum<G, K>(T, v, n, t);
#pragma unroll
    for (int k = 0; k < K; ++k) {                   // second order
        const float b = rho[k] * (A - v[k]);
        g[k] += b;
        v[k] = b / q[k];
    }
    const float Bs = owned_sum<G, K>(T, v, n, t);
    const bool one = n <= 1;                        // exactly 0
#pragma unroll
    for (int k = 0; k < K; ++k) {                   // third order
        const int i = t + k * G;
        if (i < n) {
            const float c = rho[k] * (Bs - v[k]);
            grad[base + i] = nanq ? NAN : one ? 0.0f : g[k] + c;
            hess[base + i] = nanq ? NAN : one ? 0.0f : rho[k] * (1.0f - rho[k]);
        }
    }
}

// ---- LightGBM-style truncated, normalised lambdarank (ptr_tree_lambdarank_ndcg_grad_hess; include/ptranking_amd.h states the rule).
// The rule is this project's own, written after LightGBM's LambdarankNDCG; nothing here is compared with LightGBM.
// LDS per query: 7 rows of Lp = round_up(max_len, 4) words (28 Lp bytes, 112 KiB at 4096 documents):
//   S   scores by document (float4 reads of the rank count)     -> after the scatter: sum_j lam per rank, the row of the S tree
//   Y   labels by document (likewise)                           -> after the scatter: grad per rank
//   Rs | Rg | Rd   score and gain of the document AT rank r, and the discount table 1 / log2(r + 2): a partner read is a broadcast
//   H   the terms of maxDCG by document, summed by the tree     -> hess per rank
//   Ix  the document at rank r
// Work split: the thread that owns rank r (strided where the list is longer than the group) walks EVERY rank when r < T and only the ranks
// below min(T, n) otherwise, in rank order (four interleaved chains per sum), and writes its own document's two results; a pair of two
// top-T documents is evaluated from both ends.  The first T ranks sit in the first lanes of the first pass, so one wavefront carries the
// n-step walks and the rest T-step ones.
constexpr int kLrnRows = 7;

// Descending rank of document i among keys[0 .. n) in ONE pass: #{j : k_j > k_i} + #{j < i : k_j == k_i} (count_ranks' rule).  Label rows and
// the first boosting round's scores are all ties, where count_ranks' second pass costs i steps per document; this costs n / 4 either way.
__device__ __forceinline__ int rank_indexed(const float *keys, int n, int i, float own) {
    const float4 *k4 = reinterpret_cast<const float4 *>(keys);
    const int n4 = (n + 3) >> 2;
    int rk = 0;
    for (int j4 = 0; j4 < n4; ++j4) {
        const float4 v = k4[j4];
        const int j = 4 * j4;
        rk += (v.x > own || (v.x == own && j < i)) + (v.y > own || (v.y == own && j + 1 < i)) + (v.z > own || (v.z == own && j + 2 < i)) +
              (v.w > own || (v.w == own && j + 3 < i));
    }
    return rk;
}

template <int G>
__global__ void __launch_bounds__(kBlock)
tree_lambdarank_ndcg_kernel(const float *__restrict__ preds, const float *__restrict__ labels, const int64_t *__restrict__ offsets, int B,
                            const int32_t *__restrict__ queries, int nq, int Lp, int max_len, int T, float sigma, int norm,
                            float *__restrict__ grad, float *__restrict__ hess) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, grp = tid / G, t = tid % G;
    const TreeQuery qu = tree_query<G>(offsets, B, queries, nq, max_len, t, grad, hess);
    const int64_t base = qu.base;
    const int n = G >= kWave ? __builtin_amdgcn_readfirstlane(qu.n) : qu.n;

    float *S = smem + (size_t)grp * kLrnRows * Lp, *Y = S + Lp, *Rs = Y + Lp, *Rg = Rs + Lp, *Rd = Rg + Lp, *H = Rd + Lp;
    int *Ix = reinterpret_cast<int *>(H + Lp);

    // ---- stage the scores and the labels; both rows are padded with -inf up to a multiple of 4 (rank_indexed reads float4)
    bool bad = false;
    const int np = (n + 3) & ~3;
    for (int i = t; i < np; i += G) {
        const float s = i < n ? preds[base + i] : -INFINITY, y = i < n ? labels[base + i] : -INFINITY;
        S[i] = s; Y[i] = y;
        bad |= s != s || y != y;
    }
    // a NaN score or label gives the list no ranking (the ranks below would not be a permutation): NaN on every document of this list
    const bool nanq = group_any<G>(bad, tid);
    group_sync<G>();

    // ---- ranks by score and by label; scatter into rank order; the terms of maxDCG (the IDCG cut at T)
    if (!nanq) {
        for (int i = t; i < n; i += G) {
            const float s = S[i], y = Y[i];
            const int r = rank_indexed(S, n, i, s), ry = rank_indexed(Y, n, i, y);
            const float g = gain_of(y);
            Rs[r] = s; Rg[r] = g; Ix[r] = i;
            Rd[i] = inv_log2_pos(i);
            H[i] = ry < T ? g * inv_log2_pos(ry) : 0.0f;
        }
    }
    group_tree<G>(H, n, t, [](float a, float b) { return a + b; });
    const float maxdcg = n > 0 ? H[0] : 0.0f;
    const float inv = maxdcg > 0.0f ? 1.0f / maxdcg : 0.0f;
    // the score-distance division applies where the list's largest and smallest scores differ
    const bool spread = norm != 0 && n > 0 && !nanq && Rs[0] != Rs[n - 1];
    group_sync<G>();

    const int Tn = T < n ? T : n;
    const float sigma2 = sigma * sigma;
    if (!nanq) {
        for (int r = t; r < n; r += G) {
            const float sr = Rs[r], gr = Rg[r], dr = Rd[r];
            const int kend = r < T ? n : Tn;
            // four interleaved chains per sum (partner k adds into chain k mod 4), joined as (0 + 1) + (2 + 3): a fixed order that depends on
            // the query alone, a quarter of the in-order rounding of one chain, and four independent dependency chains for the adder
            float g[4] = {0.0f, 0.0f, 0.0f, 0.0f}, h[4] = {0.0f, 0.0f, 0.0f, 0.0f}, l[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            auto partner = [&](int k, float &ga, float &ha, float &la) {
                const float dg = gr - Rg[k];                       // > 0: this document is the pair's `hi`
                const float d0 = sr - Rs[k];
                const float ds = dg > 0.0f ? d0 : -d0;             // s_hi - s_lo: the difference first, sigma after
                float delta = fabsf(dg) * fabsf(dr - Rd[k]) * inv;
                if (spread) delta *= rcp_nr(0.01f + fabsf(ds));
                const float x = sigma * ds;
                const float e = __expf(-fabsf(x));
                const float r1 = rcp1p(e);
                const float p = x >= 0.0f ? e * r1 : r1;           // 1 / (1 + exp(x))
                const float lam = sigma * delta * p;
                const float hv = sigma2 * delta * (e * r1 * r1);   // p (1 - p) without the cancellation of 1 - p
                const bool on = dg != 0.0f;                        // equal gains: equal labels (k == r among them), or delta = 0
                ga += on ? (dg > 0.0f ? -lam : lam) : 0.0f;
                ha += on ? hv : 0.0f;
                la += on ? lam : 0.0f;
            };
            int k = 0;
            for (; k + 4 <= kend; k += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) partner(k + u, g[u], h[u], l[u]);
            }
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (k + u < kend) partner(k + u, g[u], h[u], l[u]);
            Y[r] = (g[0] + g[1]) + (g[2] + g[3]);
            H[r] = (h[0] + h[1]) + (h[2] + h[3]);
            S[r] = (l[0] + l[1]) + (l[2] + l[3]);
        }
    }
    // S = 2 sum lam: every pair was seen once from each end
    group_tree<G>(S, n, t, [](float a, float b) { return a + b; });
    const float total = n > 0 ? S[0] : 0.0f;
    if (nanq) {
        for (int i = t; i < n; i += G) { grad[base + i] = NAN; hess[base + i] = NAN; }
        return;
    }
    const float scale = norm != 0 && total > 0.0f ? log1pf(total) * 1.4426950408889634f / total : 1.0f;    // log2(1 + S) / S
    for (int r = t; r < n; r += G) {
        const int i = Ix[r];
        grad[base + i] = Y[r] * scale;
        hess[base + i] = H[r] * scale;
    }
}

// ---- host side
static int tree_check(const void *preds, const void *labels, const void *offsets, int B, const void *queries, int nq, int max_len, int hessian,
                      const void *grad, const void *hess, const char *who) {
    if (B < 0 || nq < 0 || max_len < 0) {
        set_error("%s: negative size (B=%d, nq=%d, max_len=%d)", who, B, nq, max_len);
        return PTR_ERR_INVALID_ARG;
    }
    if (!queries && nq != B) { set_error("%s: queries is NULL (all queries), so nq must equal B (nq=%d, B=%d)", who, nq, B); return PTR_ERR_INVALID_ARG; }
    if (hessian < PTR_TREE_HESS_REFERENCE || hessian > PTR_TREE_HESS_CONSTANT) {
        set_error("%s: hessian must be one of PTR_TREE_HESS_* (0 .. 2), got %d", who, hessian);
        return PTR_ERR_INVALID_ARG;
    }
    if (int rc = check_pointers(nq, preds && labels && offsets, who, "NULL input pointer (preds, labels or offsets)")) return rc;
    return check_pointers(nq, grad && hess, who, "NULL output pointer (grad or hess)");
}

static int tree_check_len(int max_len, const char *who) {
    if (max_len > PTR_MAX_LIST_LEN) {
        set_error("%s: max_len=%d exceeds PTR_MAX_LIST_LEN=%d", who, max_len, PTR_MAX_LIST_LEN);
        return PTR_ERR_UNSUPPORTED;
    }
    return 0;
}

// Calls f.template operator()<G>() for the form of max_len.
template <class F> static int dispatch_tree_form(int max_len, F &&f) {
    if (max_len <= 16) return f.template operator()<16>();
    if (max_len <= 128) return f.template operator()<64>();
    return f.template operator()<256>();
}
template <int G, int W> static auto tree_pair_kernel_of(int hessian) {
    return hessian == PTR_TREE_HESS_REFERENCE ? tree_pair_kernel<G, W, PTR_TREE_HESS_REFERENCE>
         : hessian == PTR_TREE_HESS_SUM ? tree_pair_kernel<G, W, PTR_TREE_HESS_SUM>
                                        : tree_pair_kernel<G, W, PTR_TREE_HESS_CONSTANT>;
}

}  // namespace ptr

extern "C" int ptr_tree_pair_grad_hess(const float *preds, const float *labels, const int64_t *offsets, int B, const int32_t *queries, int nq,
                                       int max_len, int pair_type, int weighting, float epsilon, int hessian, float *grad, float *hess,
                                       void *stream) {
    using namespace ptr;
    const char *who = "ptr_tree_pair_grad_hess";
    if (int rc = tree_check(preds, labels, offsets, B, queries, nq, max_len, hessian, grad, hess, who)) return rc;
    if (pair_type < PTR_TREE_PAIRS_ALL || pair_type > PTR_TREE_PAIRS_00) {
        set_error("%s: pair_type must be one of PTR_TREE_PAIRS_* (0 .. 3), got %d", who, pair_type);
        return PTR_ERR_INVALID_ARG;
    }
    if (weighting < PTR_TREE_W_NONE || weighting > PTR_TREE_W_DELTA_GAIN) {
        set_error("%s: weighting must be one of PTR_TREE_W_* (0 .. 2), got %d", who, weighting);
        return PTR_ERR_INVALID_ARG;
    }
    if (!(epsilon >= 0.0f)) { set_error("%s: epsilon must be >= 0 (got %g)", who, (double)epsilon); return PTR_ERR_INVALID_ARG; }
    if (int rc = tree_check_len(max_len, who)) return rc;
    if (nq == 0 || max_len == 0) return 0;
    // bit 0: labels differ; bit 2: equal labels, not both 0; bit 3: both 0
    const int pmask = pair_type == PTR_TREE_PAIRS_ALL ? 0xD : pair_type == PTR_TREE_PAIRS_NOTIES ? 0x1 : pair_type == PTR_TREE_PAIRS_NO00 ? 0x5 : 0x8;
    const int Lp = round_up(max_len, 4);
    return dispatch_tree_form(max_len, [&]<int G>() {
        auto go = [&](auto kern, int K) -> int {
            const size_t lds = (size_t)(kBlock / G) * K * Lp * sizeof(float);
            return launch_queries(kern, nq, kBlock / G, kBlock, lds, stream, who, preds, labels, offsets, B, queries, nq, Lp, max_len, pmask, epsilon,
                                  grad, hess);
        };
        return weighting == PTR_TREE_W_NONE ? go(tree_pair_kernel_of<G, PTR_TREE_W_NONE>(hessian), tree_rows(PTR_TREE_W_NONE))
             : weighting == PTR_TREE_W_DELTA_NDCG ? go(tree_pair_kernel_of<G, PTR_TREE_W_DELTA_NDCG>(hessian), tree_rows(PTR_TREE_W_DELTA_NDCG))
                                                  : go(tree_pair_kernel_of<G, PTR_TREE_W_DELTA_GAIN>(hessian), tree_rows(PTR_TREE_W_DELTA_GAIN));
    });
}

extern "C" int ptr_tree_listnet_grad_hess(const float *preds, const float *labels, const int64_t *offsets, int B, const int32_t *queries, int nq,
                                          int max_len, int gain_type, int hessian, float *grad, float *hess, void *stream) {
    using namespace ptr;
    const char *who = "ptr_tree_listnet_grad_hess";
    if (int rc = tree_check(preds, labels, offsets, B, queries, nq, max_len, hessian, grad, hess, who)) return rc;
    if (gain_type < PTR_TREE_GAIN_POWER || gain_type > PTR_TREE_GAIN_LABEL) {
        set_error("%s: gain_type must be one of PTR_TREE_GAIN_* (0 .. 1), got %d", who, gain_type);
        return PTR_ERR_INVALID_ARG;
    }
    if (int rc = tree_check_len(max_len, who)) return rc;
    if (nq == 0 || max_len == 0) return 0;
    const int Lp = round_up(max_len, 4);
    return dispatch_tree_form(max_len, [&]<int G>() {
        const size_t lds = (size_t)(kBlock / G) * 3 * Lp * sizeof(float);
        return launch_queries(tree_listnet_kernel<G>, nq, kBlock / G, kBlock, lds, stream, who, preds, labels, offsets, B, queries, nq, Lp, max_len,
                              gain_type == PTR_TREE_GAIN_POWER ? 1 : 0, hessian == PTR_TREE_HESS_CONSTANT ? 1 : 0, grad, hess);
    });
}

extern "C" int ptr_tree_lambdarank_ndcg_grad_hess(const float *preds, const float *labels, const int64_t *offsets, int B, const int32_t *queries,
                                                  int nq, int max_len, int truncation_level, float sigmoid, int norm, float *grad, float *hess,
                                                  void *stream) {
    using namespace ptr;
    const char *who = "ptr_tree_lambdarank_ndcg_grad_hess";
    if (int rc = tree_check(preds, labels, offsets, B, queries, nq, max_len, PTR_TREE_HESS_SUM, grad, hess, who)) return rc;
    if (truncation_level < 1) { set_error("%s: truncation_level must be >= 1 (got %d)", who, truncation_level); return PTR_ERR_INVALID_ARG; }
    if (!(sigmoid > 0.0f)) { set_error("%s: sigmoid must be > 0 (got %g)", who, (double)sigmoid); return PTR_ERR_INVALID_ARG; }
    if (int rc = tree_check_len(max_len, who)) return rc;
    if (nq == 0 || max_len == 0) return 0;
    const int Lp = round_up(max_len, 4);
    return dispatch_tree_form(max_len, [&]<int G>() {
        const size_t lds = (size_t)(kBlock / G) * kLrnRows * Lp * sizeof(float);
        return launch_queries(tree_lambdarank_ndcg_kernel<G>, nq, kBlock / G, kBlock, lds, stream, who, preds, labels, offsets, B, queries, nq, Lp,
                              max_len, truncation_level, sigmoid, norm, grad, hess);
    });
}

extern "C" int ptr_tree_xendcg_grad_hess(const float *preds, const float *labels, const int64_t *offsets, int B, const int32_t *queries, int nq,
                                         int max_len, const float *unif, uint64_t seed, int64_t draw, float *grad, float *hess, void *stream) {
    using namespace ptr;
    const char *who = "ptr_tree_xendcg_grad_hess";
    if (int rc = tree_check(preds, labels, offsets, B, queries, nq, max_len, PTR_TREE_HESS_SUM, grad, hess, who)) return rc;
    if (draw < 0) { set_error("%s: draw must be >= 0 (got %lld)", who, (long long)draw); return PTR_ERR_INVALID_ARG; }
    if (int rc = tree_check_len(max_len, who)) return rc;
    if (nq == 0 || max_len == 0) return 0;
    const int Lp = round_up(max_len, 4);
    auto go = [&]<int G, int K>() {
        static_assert(G * K <= PTR_MAX_LIST_LEN);
        const size_t lds = (size_t)(kBlock / G) * 2 * Lp * sizeof(float);
        return launch_queries(tree_xendcg_kernel<G, K>, nq, kBlock / G, kBlock, lds, stream, who, preds, labels, offsets, B, queries, nq, Lp, max_len,
                              unif, seed, draw, grad, hess);
    };
    // tree_form: sixteen queries per workgroup up to 16 documents, pick_tiling's (G, documents per thread) beyond
    return max_len <= 16 ? go.template operator()<16, 1>() : dispatch_tiling(max_len, go);
}
