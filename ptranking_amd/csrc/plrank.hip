// PL-Rank: the policy-gradient estimator of the expected top-K reward under a Plackett-Luce ranking policy, sampling included, in one launch.
//
// The rule is stated in include/ptranking_amd.h (the estimator is PL-Rank-3: Oosterhuis, SIGIR 2021 and SIGIR 2022).  Per sampled ranking y it
// needs the suffix sums D (of e = exp(s - max)) and PR (of theta * rho) and the prefix sums RI (of PR / D) and DR (of theta / D) along y:
// one sort and O(L) per sample, the shape of work plsample.hip does.  The draw is that of ptr_pl_sample(PTR_PL_DIST_PL, temperature 1): the
// same uniforms, key s + gumbel, (key descending, index ascending) — the perm rows are equal bit for bit.
//
// Shape: one workgroup per query, W = min(S, 4) wavefronts; wave w takes the samples w, w + W, w + 2W, ...  A wave holds a whole ranking in
// registers, lane t owning positions t*DPT .. t*DPT + DPT-1 (DPT 1 .. 16 by pick_wave_tiling: lists of up to 1024 documents), sorted by the
// register sort of pl_wave_kernel (sort_scores_packed, else rank_blocked_wave).  The four scans run in position order in registers: inside the
// lane, then across the lanes (grp_excl_suffix, the DPP prefix scan); the two prefix values at position K-1 are broadcast from their lane
// for the documents a top-K ranking leaves unplaced.  Each sample's gradient is added into the wave's own LDS row by document (a document
// occurs once per sample: plain read-modify-write); the W rows and value sums are combined in wave order after one barrier.  No atomics,
// nothing of size [B,S,L] in global memory but the optional perm: a query's bits depend on (its data, L, S, seed, q0 + q) alone.
//
// LDS (N = 64 DPT floats a row): SR scores | E exp(s - max) | GN gains, by document, shared; per wave K keys / sorted row | X2 scratch of the
// float sort | GA gradient sums by document; + 4 value sums: (3 + 3 W) N + 4 floats, 60 KiB + 16 at N = 1024 and W = 4.
#include "ptr_device.h"
#include "ptr_plhash.h"

namespace ptr {

PlrankForm plrank_form(int L, int S) {
    const int dpt = pick_wave_tiling(L).DPT, waves = S < kPlrankMaxWaves ? (S < 1 ? 1 : S) : kPlrankMaxWaves;
    return {dpt, waves, (int)(((size_t)(3 + 3 * waves) * kWave * dpt + 4) * sizeof(float))};
}

struct PlrankArgs {
    const float *preds, *labels;
    const int32_t *lens;
    int B, L, S, top_k, normalize;
    uint64_t seed;
    int64_t q0;
    const float *unif;
    int64_t *perm;
    float *value_q, *grad;
    int aligned;
};

template <int DPT>
__global__ void __launch_bounds__(kBlock) plrank_kernel(const PlrankArgs A) {
    constexpr int N = kWave * DPT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int W = blockDim.x >> 6, w = threadIdx.x >> 6, t = threadIdx.x & 63;
    const int q = blockIdx.x, L = A.L, S = A.S;
    const int n = query_len(A.lens, q, L);
    float *SR = smem, *E = SR + N, *GN = E + N;
    float *K = GN + N + (size_t)w * 3 * N, *X2 = K + N, *GA = X2 + N;          // K doubles as the float sort's sorted row
    float *red = smem + (size_t)(3 + 3 * W) * N;
    const int top = (A.top_k <= 0 || A.top_k > n) ? n : A.top_k;
    bool bad = false;
    float th[DPT];                                                           // theta by position, 0 from position K on
    {
        // every wave reads the list (it needs the maximum and the ideal DCG in its own registers); wave 0 stages the shared rows
        float s[DPT], y[DPT], e[DPT];
        load_blocked<DPT>(A.preds + (size_t)q * L, n, L, t, -INFINITY, s, A.aligned != 0);
        load_blocked<DPT>(A.labels + (size_t)q * L, n, L, t, 0.0f, y, A.aligned != 0);
        float m = -INFINITY;
#pragma unroll
        for (int r = 0; r < DPT; ++r) { bad |= s[r] != s[r]; m = fmaxf(m, s[r]); }
        m = wave_max(m);
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            e[r] = p < n ? expf(s[r] - m) : 0.0f;
            y[r] = p < n ? gain_of(y[r]) : 0.0f;
            th[r] = p < top ? 1.0f / log2f(2.0f + (float)p) : 0.0f;
        }
        if (w == 0) {
            lds_store_blocked<DPT>(SR, t, s);
            lds_store_blocked<DPT>(E, t, e);
            lds_store_blocked<DPT>(GN, t, y);
        }
#pragma unroll
        for (int r = 0; r < DPT; ++r) e[r] = 0.0f;
        lds_store_blocked<DPT>(GA, t, e);
        if (A.normalize) {                                                   // theta / ideal DCG@K; an ideal DCG of 0 gives value 0, gradient 0
#pragma unroll
            for (int r = 0; r < DPT; ++r) y[r] = t * DPT + r < n ? y[r] : -INFINITY;
            wave_sort_desc<DPT>(y, t);
            float part = 0.0f;
#pragma unroll
            for (int r = 0; r < DPT; ++r) part += t * DPT + r < top ? th[r] * y[r] : 0.0f;
            const float idcg = wave_sum(part);
            const float norm = idcg > 0.0f ? 1.0f / idcg : 0.0f;
#pragma unroll
            for (int r = 0; r < DPT; ++r) th[r] *= norm;
        }
    }
    const bool nanq = __any(bad);                                            // the same in every wave: each read the whole list
    __syncthreads();
    const PlKeys qk = pl_query_keys(A.seed, A.q0 + (int64_t)q);
    float vsum = 0.0f;
    for (int smp = w; smp < S; smp += W) {
        const size_t row = ((size_t)q * S + smp) * L;
        int64_t *prow = A.perm ? A.perm + row : nullptr;
        int id[DPT];
        if (nanq || n == 0) {                                                // no ranking: the identity, as ptr_pl_sample
            if (prow) {
#pragma unroll
                for (int r = 0; r < DPT; ++r)
                    if (t * DPT + r < L) prow[t * DPT + r] = (int64_t)(t * DPT + r);
            }
            continue;
        }
        // ---- draw and sort: pl_wave_kernel's steps at PTR_PL_DIST_PL, temperature 1 (key = s + gumbel)
        const PlKeys sk = pl_sample_keys(qk, (uint32_t)smp);
        float key[DPT], kv[DPT];
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int i = t * DPT + r;
            key[r] = -INFINITY;
            if (i < n) key[r] = SR[i] + pl_gumbel(A.unif ? A.unif[row + i] : pl_uniform(sk, (uint32_t)i));
        }
        bool sorted = false;
        if constexpr (DPT >= 2) {
            sorted = sort_scores_packed<DPT, false>(K, n, t, key, kv, id);
            if (!sorted) wave_lds_sync();
        }
        if (!sorted) {                                                       // 64 documents at most, or keys the packed order cannot tell apart
            int rk[DPT];
            rank_blocked_wave<DPT>(K, X2, n, t, key, rk, kv);
            int *PD = reinterpret_cast<int *>(X2);
#pragma unroll
            for (int r = 0; r < DPT; ++r)
                if (t * DPT + r < n) PD[rk[r]] = t * DPT + r;
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < DPT; ++r) id[r] = t * DPT + r < n ? PD[t * DPT + r] : N - 1;
            wave_lds_sync();
        }
        if (prow) {
#pragma unroll
            for (int r = 0; r < DPT; ++r) {
                const int p = t * DPT + r;
                if (p < L) prow[p] = p < n ? (int64_t)id[r] : (int64_t)p;
            }
        }
        // ---- the suffix scans D and PR: inside the lane from its last position down, then the lanes behind it
        float ev[DPT], rho[DPT], a[DPT], D[DPT], PRn[DPT];                   // PRn[r] = PR at position p + 1
        float es = 0.0f, as = 0.0f;
#pragma unroll
        for (int r = DPT - 1; r >= 0; --r) {
            const bool live = t * DPT + r < n;
            ev[r] = live ? E[id[r]] : 0.0f;
            rho[r] = live ? GN[id[r]] : 0.0f;
            a[r] = th[r] * rho[r];
            PRn[r] = as;
            as += a[r];
            es += ev[r];
            D[r] = es;
        }
        const float ex_e = grp_excl_suffix<kWave>(es, nullptr, t), ex_a = grp_excl_suffix<kWave>(as, nullptr, t);
        // ---- the prefix scans RI and DR over the placed positions (their terms are 0 from position K on)
        float RI[DPT], DR[DPT];
        float ri = 0.0f, dr = 0.0f;
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            if (t * DPT + r < top) {
                const float rd = 1.0f / (D[r] + ex_e);
                PRn[r] += ex_a;
                ri += (a[r] + PRn[r]) * rd;
                dr += th[r] * rd;
            }
            RI[r] = ri;
            DR[r] = dr;
        }
        wave_incl_sum2(ri, dr);
        const float px_ri = dpp_wave_shr1(ri), px_dr = dpp_wave_shr1(dr);
        float riK = 0.0f, drK = 0.0f;                                        // RI and DR at position K - 1, for the unplaced documents
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            RI[r] += px_ri;
            DR[r] += px_dr;
            if (t * DPT + r == top - 1) { riK = RI[r]; drK = DR[r]; }
        }
        riK = __shfl(riK, (top - 1) / DPT, 64);
        drK = __shfl(drK, (top - 1) / DPT, 64);
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            if (p < n) GA[id[r]] += PRn[r] + ev[r] * (rho[r] * (p < top ? DR[r] : drK) - (p < top ? RI[r] : riK));
        }
        vsum += __shfl(as + ex_a, 0, 64);                                    // PR at position 0: the sample's reward
        wave_lds_sync();
    }
    if (t == 0) red[w] = vsum;
    __syncthreads();
    // ---- the W rows and value sums in wave order; the gradient of the loss -reward
    const float inv_s = 1.0f / (float)S;
    const float *G0 = GN + 3 * N;                                            // wave 0's GA row
    float *g = A.grad + (size_t)q * L;
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        float v = 0.0f;
        if (i < n) {
            v = G0[i];
            for (int u = 1; u < W; ++u) v += G0[(size_t)u * 3 * N + i];
            v = nanq ? __builtin_nanf("") : 0.0f - v * inv_s;
        }
        g[i] = v;
    }
    if (threadIdx.x == 0) {
        float v = red[0];
        for (int u = 1; u < W; ++u) v += red[u];
        A.value_q[q] = (nanq && n > 0) ? __builtin_nanf("") : v * inv_s;
    }
}

}  // namespace ptr

extern "C" int ptr_plrank_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, int S, int top_k, int normalize,
                                  uint64_t seed, int64_t q0, const float *unif, float *loss_out, float *value_q, float *grad, int64_t *perm_out,
                                  void *stream) {
    using namespace ptr;
    const char *who = "ptr_plrank_fwd_bwd";
    if (B < 0 || L <= 0) { set_error("%s: bad shape B=%d L=%d", who, B, L); return PTR_ERR_INVALID_ARG; }
    if (L > kPlrankMaxLen) { set_error("%s: list length %d exceeds PLRANK_MAX_LEN=%d", who, L, kPlrankMaxLen); return PTR_ERR_INVALID_ARG; }
    if (S < 1) { set_error("%s: samples per query must be >= 1 (got %d)", who, S); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_pointers(B, preds && labels, who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, value_q && grad, who)) return rc;
    if (B == 0) return 0;
    PlrankArgs A{preds, labels, lens, B, L, S, top_k, normalize, seed, q0, unif, perm_out, value_q, grad, 0};
    A.aligned = ((reinterpret_cast<uintptr_t>(preds) | reinterpret_cast<uintptr_t>(labels)) & 15) == 0;
    const PlrankForm f = plrank_form(L, S);
    const int rc = dispatch_wave_tiling(L, [&]<int G, int DPT>() -> int {
        if constexpr (G == kWave) return launch_queries(plrank_kernel<DPT>, B, 1, kWave * f.waves, (size_t)f.lds_bytes, stream, who, A);
        else return PTR_ERR_INVALID_ARG;                                     // not reached: L <= 1024 is one wavefront per ranking
    });
    if (rc) return rc;
    return finish_loss(value_q, B, -1.0f, loss_out, stream);
}
