// Device Plackett-Luce sampling of rankings and the fused multi-sample MDPRank loss.
//
// Reference: ptranking/ltr_adhoc/util/sampling_utils.py:31-81 (sample_ranking_PL, sample_ranking_PL_gumbel_softmax),
//            ptranking/ltr_adversarial/util/list_sampling.py:38-67 (the same sampler with num_sample_ranking > 1),
//            ptranking/ltr_adhoc/listwise/mdprank.py:36-71 (sample, then the return-weighted ListMLE of the episode).
// A ranking drawn from the Plackett-Luce model with weights exp(s_i / T) is the descending order of s_i / T + g_i with g_i i.i.d. standard
// Gumbel (the reference's own STPL branch at T = 1), so ONE construction serves both distributions: counter-based uniforms -> the
// reference's Gumbel transform -> the (key descending, index ascending) order of ptr_sort_desc.  Nothing here needs a non-zero weight per
// draw: where torch.multinomial(replacement=False) fails once exp() underflows, the key s_i / T + g_i is as finite as the score.
//
// Uniforms: u(seed, q0 + q, s, i) = 24 random bits * 2^-24.  Two 32-bit keys per (query, sample) come from lowbias32 finalisers on the
// seed words and the GLOBAL query index q0 + q; per document one finaliser on ka + i * odd, then one multiply on its xor with kb (three
// 32-bit multiplies per document, no 64-bit arithmetic per document).  With ONE key two of 2^18 streams would be shifted copies of each
// other (a 32-bit counter space holds 2^30 draws of such a batch only just); the second key decouples them.
//
// Shape: lists of up to 1024 documents take one wavefront per query, lane t owning documents / positions t*DPT .. t*DPT+DPT-1 in
// registers: packed (key, index) register sort (ptr_device.h sort_scores_packed; the float sort + exact count where two keys agree in the
// packed bits or tie), DPT 1 .. 16.  Up to 4096: one workgroup per query, keys in LDS, count_ranks_fast.  The S samples of a query are taken
// in order by the same wave / workgroup; the loss and the gradient are accumulated per query in a register and one LDS row, in that
// order, without atomics: a query's bits depend on (its data, L, S, seed, q0 + q) alone.  Nothing of size L x L.
#include "ptr_device.h"
#include "ptr_plhash.h"

namespace ptr {

// key of a document: 'PL' s / T + g (s itself at T == 1, sampling_utils.py:41-44), 'STPL' s + g (:71, :76-78: T never enters the order)
__device__ __forceinline__ float pl_key(float s, float u, float temperature, int dist) {
    const float g = pl_gumbel(u);
    return (dist == PTR_PL_DIST_PL && temperature != 1.0f ? s / temperature : s) + g;
}

// mdprank.py:45-71 on ONE sampled ranking held by position (thread t: positions t*DPT ..): a = action value, id = document.  Adds
// gscale * d loss / d a to GA[document] and returns the episode's loss (every thread).  GN = 2^label - 1 by document.
template <int G, int DPT>
__device__ __forceinline__ float pl_episode(const float (&a)[DPT], const int (&id)[DPT], const float *GN, float *GA, float *red, int n, int top,
                                            int t, float gamma, float gscale) {
    float m = -INFINITY, lo = -INFINITY;
#pragma unroll
    for (int r = 0; r < DPT; ++r) {
        m = t * DPT + r < n ? fmaxf(m, a[r]) : m;
        lo = t * DPT + r < n ? fmaxf(lo, -a[r]) : lo;
    }
    m = group_max<G>(m, red, t);                                                             // mdprank.py:65
    lo = group_max<G>(lo, red, t);
    float w[DPT];
    float rs = 0.0f;
#pragma unroll
    for (int r = DPT - 1; r >= 0; --r) {                                                     // tail sums of the rewards inside the thread
        const int p = t * DPT + r;
        rs += p < top ? GN[id[r]] / log2f(2.0f + (float)p) : 0.0f;                           // :53-56
        w[r] = rs;
    }
    const float rx = grp_excl_suffix<G>(rs, red, t);                                         // :59
#pragma unroll
    for (int r = 0; r < DPT; ++r)
        w[r] = t * DPT + r < top ? (w[r] + rx) * (gamma == 1.0f ? 1.0f : powf(gamma, (float)(t * DPT + r + 1))) : 0.0f;   // :61-63
    float loss = 0.0f;
    if (m + lo > 80.0f) {
        // a spread beyond e^-80: exp(a - m) underflows, the reference's log(cumsum) is -inf (:68-69).  Both scans in the log domain:
        // with b = a - m:  lse_t = log sum_{j >= t} e^{b_j},  d loss / d a_j = sum_{t <= min(j, top - 1)} w_t e^{b_j - lse_t} - w_j, every
        // exponent <= log w_t; m is taken off first so that the roundings stay relative to |a - m|, as on the other path
        float ls[DPT];
        float run = -INFINITY;
#pragma unroll
        for (int r = DPT - 1; r >= 0; --r) {
            if (t * DPT + r < n) run = lse2(a[r] - m, run);
            ls[r] = run;
        }
        const float lx = grp_excl_suffix_lse<G>(run, red, t);
        run = -INFINITY;
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            ls[r] = lse2(ls[r], lx);
            if (t * DPT + r < top) {
                loss += w[r] * ((ls[r] + m) - a[r]);
                if (w[r] > 0.0f) run = lse2(run, logf(w[r]) - ls[r]);
            }
            ls[r] = run;                                                                     // ls now holds the prefix of log(w / T)
        }
        const float qx = grp_excl_prefix_lse<G>(run, red, t);
#pragma unroll
        for (int r = 0; r < DPT; ++r)
            if (t * DPT + r < n) GA[id[r]] += (expf((a[r] - m) + lse2(ls[r], qx)) - w[r]) * gscale;
        return group_sum<G>(loss, red, t);
    }
    float e[DPT], T[DPT];
    float ts = 0.0f;
#pragma unroll
    for (int r = DPT - 1; r >= 0; --r) {                                                     // tail sums inside the thread
        e[r] = t * DPT + r < n ? expf(a[r] - m) : 0.0f;
        ts += e[r];
        T[r] = ts;
    }
    const float tx = grp_excl_suffix<G>(ts, red, t);                                         // :68
    float ps = 0.0f;
#pragma unroll
    for (int r = 0; r < DPT; ++r) {
        T[r] += tx;
        if (t * DPT + r < top) {
            loss += w[r] * ((logf(T[r]) + m) - a[r]);                                        // :69-71
            ps += w[r] / T[r];
        }
        T[r] = ps;                                                                           // T now holds the prefix of w / T
    }
    const float px = grp_excl_prefix<G>(ps, red, t);
#pragma unroll
    for (int r = 0; r < DPT; ++r)
        if (t * DPT + r < n) GA[id[r]] += (e[r] * (T[r] + px) - w[r]) * gscale;
    return group_sum<G>(loss, red, t);
}

// perm / action rows of one sample, held by position: 16-byte stores where the row allows it
template <int DPT>
__device__ __forceinline__ void pl_store_rows(int64_t *__restrict__ prow, float *__restrict__ arow, int n, int L, int t, const int (&id)[DPT],
                                              const float (&a)[DPT], bool vec) {
    typedef long i64x2_t __attribute__((ext_vector_type(2)));
    if (DPT % 4 == 0 && vec) {
#pragma unroll
        for (int r = 0; r < DPT; r += 4) {
            const int p = t * DPT + r;
            if (p < L) {
                if (prow) {
                    *reinterpret_cast<i64x2_t *>(prow + p) = i64x2_t{p < n ? (long)id[r] : (long)p, p + 1 < n ? (long)id[r + 1] : (long)(p + 1)};
                    *reinterpret_cast<i64x2_t *>(prow + p + 2) = i64x2_t{p + 2 < n ? (long)id[r + 2] : (long)(p + 2), p + 3 < n ? (long)id[r + 3] : (long)(p + 3)};
                }
                if (arow)
                    *reinterpret_cast<float4 *>(arow + p) = float4{p < n ? a[r] : 0.0f, p + 1 < n ? a[r + 1] : 0.0f, p + 2 < n ? a[r + 2] : 0.0f, p + 3 < n ? a[r + 3] : 0.0f};
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            if (p < L) {
                if (prow) prow[p] = p < n ? (int64_t)id[r] : (int64_t)p;
                if (arow) arow[p] = p < n ? a[r] : 0.0f;
            }
        }
    }
}

struct PlArgs {
    const float *preds, *labels;
    const int32_t *lens;
    int B, L, S, top_k;
    float gamma, temperature;
    int dist;
    uint64_t seed;
    int64_t q0;
    const float *unif;
    int64_t *perm;
    float *action, *loss_q, *grad;
    int aligned;
};

// ---- one wavefront per query, lists of up to 64 DPT <= 1024 documents.  LDS per query (N = 64 DPT floats each): K keys by document | SR
// scores by document | X1, X2 scratch of the float sort | LOSS: GN gains by document | GA gradient sums by document
template <int DPT, bool LOSS>
__global__ void __launch_bounds__(kBlock) pl_wave_kernel(const PlArgs A) {
    constexpr int N = kWave * DPT, QPB = kBlock / kWave, ROWS = LOSS ? 6 : 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int grp = threadIdx.x >> 6, t = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * QPB + grp);
    if (q >= A.B) return;                                                    // wave-level synchronisation only below
    const int L = A.L, S = A.S;
    const int n = query_len(A.lens, q, L);
    float *K = smem + (size_t)grp * ROWS * N, *SR = K + N, *X1 = SR + N, *X2 = X1 + N;
    float *GN = X2 + N, *GA = GN + N;                                        // LOSS only
    bool bad = false;
    {
        float s[DPT];
        load_blocked<DPT>(A.preds + (size_t)q * L, n, L, t, -INFINITY, s, A.aligned != 0);
#pragma unroll
        for (int r = 0; r < DPT; ++r) bad |= s[r] != s[r];
        lds_store_blocked<DPT>(SR, t, s);
        if constexpr (LOSS) {
            float y[DPT];
            load_blocked<DPT>(A.labels + (size_t)q * L, n, L, t, 0.0f, y, A.aligned != 0);
#pragma unroll
            for (int r = 0; r < DPT; ++r) { y[r] = gain_of(y[r]); s[r] = 0.0f; }
            lds_store_blocked<DPT>(GN, t, y);
            lds_store_blocked<DPT>(GA, t, s);
        }
    }
    const bool nanq = __any(bad);
    wave_lds_sync();
    const int top = (A.top_k <= 0 || A.top_k > n) ? n : A.top_k;              // top_k=None -> the whole list (mdprank.py:45)
    const bool stpl = A.dist == PTR_PL_DIST_STPL, t1 = A.temperature == 1.0f;
    const float gscale = (stpl && !t1) ? 1.0f / A.temperature : 1.0f;
    const PlKeys qk = pl_query_keys(A.seed, A.q0 + (int64_t)q);
    float lsum = 0.0f;
    for (int smp = 0; smp < S; ++smp) {
        const size_t row = ((size_t)q * S + smp) * L;
        int64_t *prow = A.perm ? A.perm + row : nullptr;
        float *arow = A.action ? A.action + row : nullptr;
        float a[DPT];
        int id[DPT];
        if (nanq || n == 0) {                                                // no ranking: the identity, NaN actions on the real positions
#pragma unroll
            for (int r = 0; r < DPT; ++r) { id[r] = t * DPT + r; a[r] = __builtin_nanf(""); }
            pl_store_rows<DPT>(prow, arow, n, L, t, id, a, A.aligned != 0 && (L & 3) == 0);
            continue;
        }
        const PlKeys sk = pl_sample_keys(qk, (uint32_t)smp);
        float key[DPT], kv[DPT];
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int i = t * DPT + r;
            key[r] = -INFINITY;
            if (i < n) key[r] = pl_key(SR[i], A.unif ? A.unif[row + i] : pl_uniform(sk, (uint32_t)i), A.temperature, A.dist);
        }
        bool sorted = false;
        if constexpr (DPT >= 2) {
            sorted = sort_scores_packed<DPT, true>(K, n, t, key, kv, id);
            if (!sorted) wave_lds_sync();
        }
        if (!sorted) {                                                       // 64 documents at most, or keys the packed order cannot tell apart
            int rk[DPT];
            rank_blocked_wave<DPT>(X1, X2, n, t, key, rk, kv);               // kv: the keys in descending order, by position
            int *PD = reinterpret_cast<int *>(X2);
#pragma unroll
            for (int r = 0; r < DPT; ++r)
                if (t * DPT + r < n) PD[rk[r]] = t * DPT + r;
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < DPT; ++r) id[r] = t * DPT + r < n ? PD[t * DPT + r] : N - 1;
            wave_lds_sync();
        }
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            // 'PL': the raw scores in sampled order (sampling_utils.py:56); 'STPL': (s + g) / T, no division at T == 1 (:75-80)
            if (t * DPT + r < n) a[r] = stpl ? (t1 ? kv[r] : kv[r] / A.temperature) : SR[id[r]];
            else a[r] = 0.0f;
        }
        pl_store_rows<DPT>(prow, arow, n, L, t, id, a, A.aligned != 0 && (L & 3) == 0);
        if constexpr (LOSS) lsum += pl_episode<kWave, DPT>(a, id, GN, GA, nullptr, n, top, t, A.gamma, gscale);
        wave_lds_sync();
    }
    if constexpr (LOSS) {
        const float inv_s = 1.0f / (float)S;
        float *g = A.grad + (size_t)q * L;
        for (int i = t; i < L; i += kWave) g[i] = i < n ? (nanq ? __builtin_nanf("") : GA[i] * inv_s) : 0.0f;
        if (t == 0) A.loss_q[q] = (nanq && n > 0) ? __builtin_nanf("") : lsum * inv_s;
    }
}

// ---- one workgroup per query, lists of up to 256 DPT <= 4096 documents: documents t + 256 m per thread for the rank count, positions
// t*DPT .. per thread for the episode.  LDS (Lp floats each): K keys by document | PD document by position | SR | LOSS: GN | GA; + 4.
template <int DPT, bool LOSS>
__global__ void __launch_bounds__(kBlock) pl_block_kernel(const PlArgs A, int Lp) {
    constexpr int G = kBlock;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int t = threadIdx.x, q = blockIdx.x;
    const int L = A.L, S = A.S;
    const int n = query_len(A.lens, q, L);
    float *K = smem, *SR = K + 2 * Lp, *GN = SR + Lp, *GA = LOSS ? GN + Lp : GN;
    int *PD = reinterpret_cast<int *>(K + Lp);
    float *red = (LOSS ? GA + Lp : SR + Lp);
    bool bad = false;
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        if (i < Lp) {
            const float s = i < n ? A.preds[(size_t)q * L + i] : -INFINITY;
            bad |= s != s;
            SR[i] = s;
            if constexpr (LOSS) { GN[i] = i < n ? gain_of(A.labels[(size_t)q * L + i]) : 0.0f; GA[i] = 0.0f; }
        }
    }
    const bool nanq = __syncthreads_or(bad);
    const int top = (A.top_k <= 0 || A.top_k > n) ? n : A.top_k;
    const bool stpl = A.dist == PTR_PL_DIST_STPL, t1 = A.temperature == 1.0f;
    const float gscale = (stpl && !t1) ? 1.0f / A.temperature : 1.0f;
    const PlKeys qk = pl_query_keys(A.seed, A.q0 + (int64_t)q);
    float lsum = 0.0f;
    for (int smp = 0; smp < S; ++smp) {
        const size_t row = ((size_t)q * S + smp) * L;
        int64_t *prow = A.perm ? A.perm + row : nullptr;
        float *arow = A.action ? A.action + row : nullptr;
        float a[DPT];
        int id[DPT];
        if (nanq || n == 0) {                                                // uniform over the workgroup
#pragma unroll
            for (int r = 0; r < DPT; ++r) { id[r] = t * DPT + r; a[r] = __builtin_nanf(""); }
            pl_store_rows<DPT>(prow, arow, n, L, t, id, a, A.aligned != 0 && (L & 3) == 0);
            continue;
        }
        const PlKeys sk = pl_sample_keys(qk, (uint32_t)smp);
        float own[DPT];
        int rk[DPT];
#pragma unroll
        for (int m = 0; m < DPT; ++m) {
            const int i = t + m * G;
            own[m] = -INFINITY;
            if (i < n) own[m] = pl_key(SR[i], A.unif ? A.unif[row + i] : pl_uniform(sk, (uint32_t)i), A.temperature, A.dist);
            if (i < Lp) K[i] = own[m];
        }
        __syncthreads();
        count_ranks_fast<G, DPT>(K, PD, n, t, own, rk);                      // PD doubles as its permutation-check scratch
        __syncthreads();
#pragma unroll
        for (int m = 0; m < DPT; ++m)
            if (t + m * G < n) PD[rk[m]] = t + m * G;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            id[r] = p < n ? PD[p] : 0;
            a[r] = 0.0f;
            if (p < n) { const float kv = K[id[r]]; a[r] = stpl ? (t1 ? kv : kv / A.temperature) : SR[id[r]]; }
        }
        pl_store_rows<DPT>(prow, arow, n, L, t, id, a, A.aligned != 0 && (L & 3) == 0);
        if constexpr (LOSS) lsum += pl_episode<G, DPT>(a, id, GN, GA, red, n, top, t, A.gamma, gscale);
        __syncthreads();
    }
    if constexpr (LOSS) {
        const float inv_s = 1.0f / (float)S;
        float *g = A.grad + (size_t)q * L;
        for (int i = t; i < L; i += G) g[i] = i < n ? (nanq ? __builtin_nanf("") : GA[i] * inv_s) : 0.0f;
        if (t == 0) A.loss_q[q] = (nanq && n > 0) ? __builtin_nanf("") : lsum * inv_s;
    }
}

// the uniforms of the two kernels above, one wavefront per (query, sample) row
__global__ void __launch_bounds__(kBlock) pl_uniforms_kernel(long rows, int L, int S, uint64_t seed, int64_t q0, float *__restrict__ unif) {
    const long row = (long)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const PlKeys sk = pl_sample_keys(pl_query_keys(seed, q0 + row / S), (uint32_t)(row % S));
    for (int i = threadIdx.x & 63; i < L; i += kWave) unif[(size_t)row * L + i] = pl_uniform(sk, (uint32_t)i);
}

static int pl_check(const char *who, int B, int L, int S, float temperature, int distribution) {
    if (B < 0 || L <= 0) { set_error("%s: bad shape B=%d L=%d", who, B, L); return PTR_ERR_INVALID_ARG; }
    if (L > PTR_MAX_LIST_LEN) { set_error("%s: list length %d exceeds PTR_MAX_LIST_LEN=%d", who, L, PTR_MAX_LIST_LEN); return PTR_ERR_INVALID_ARG; }
    if (S < 1) { set_error("%s: samples per query must be >= 1 (got %d)", who, S); return PTR_ERR_INVALID_ARG; }
    if (!(temperature > 0.0f)) { set_error("%s: temperature must be > 0 (got %g)", who, (double)temperature); return PTR_ERR_INVALID_ARG; }
    if (distribution != PTR_PL_DIST_PL && distribution != PTR_PL_DIST_STPL) {
        set_error("%s: distribution %d (PTR_PL_DIST_PL, PTR_PL_DIST_STPL)", who, distribution);
        return PTR_ERR_INVALID_ARG;
    }
    return 0;
}

template <bool LOSS> static int pl_launch(PlArgs A, void *stream, const char *who) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(A.preds) | reinterpret_cast<uintptr_t>(A.labels) | reinterpret_cast<uintptr_t>(A.unif) |
                           reinterpret_cast<uintptr_t>(A.perm) | reinterpret_cast<uintptr_t>(A.action);
    A.aligned = (bits & 15) == 0;
    return dispatch_wave_tiling(A.L, [&]<int G, int DPT>() -> int {
        if constexpr (G == kWave) {
            constexpr int QPB = kBlock / kWave;
            const size_t lds = (size_t)QPB * (LOSS ? 6 : 4) * kWave * DPT * sizeof(float);
            return launch_queries(pl_wave_kernel<DPT, LOSS>, A.B, QPB, kBlock, lds, stream, who, A);
        } else {
            const int Lp = round_up(A.L, 4);
            const size_t lds = ((size_t)(LOSS ? 5 : 3) * Lp + 4) * sizeof(float);
            return launch_queries(pl_block_kernel<DPT, LOSS>, A.B, 1, kBlock, lds, stream, who, A, Lp);
        }
    });
}

}  // namespace ptr

extern "C" int ptr_pl_uniforms(int B, int L, int S, uint64_t seed, int64_t q0, float *unif, void *stream) {
    using namespace ptr;
    const char *who = "ptr_pl_uniforms";
    if (int rc = pl_check(who, B, L, S, 1.0f, PTR_PL_DIST_PL)) return rc;
    if (int rc = check_pointers(B, unif != nullptr, who)) return rc;
    if (B == 0) return 0;
    const long rows = (long)B * S;
    hipLaunchKernelGGL(pl_uniforms_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(kBlock), 0, as_stream(stream), rows, L, S, seed, q0, unif);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_pl_sample(const float *preds, const int32_t *lens, int B, int L, int S, float temperature, int distribution, uint64_t seed,
                             int64_t q0, const float *unif, int64_t *perm, float *action, void *stream) {
    using namespace ptr;
    const char *who = "ptr_pl_sample";
    if (int rc = pl_check(who, B, L, S, temperature, distribution)) return rc;
    if (int rc = check_pointers(B, preds != nullptr, who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, perm != nullptr, who)) return rc;
    if (B == 0) return 0;
    PlArgs A{preds, nullptr, lens, B, L, S, 0, 1.0f, temperature, distribution, seed, q0, unif, perm, action, nullptr, nullptr, 0};
    return pl_launch<false>(A, stream, who);
}

extern "C" int ptr_mdprank_sample_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, int S, int top_k,
                                          float gamma, float temperature, int distribution, uint64_t seed, int64_t q0, const float *unif,
                                          float *loss_out, float *loss_q, float *grad, int64_t *perm_out, void *stream) {
    using namespace ptr;
    const char *who = "ptr_mdprank_sample_fwd_bwd";
    if (int rc = pl_check(who, B, L, S, temperature, distribution)) return rc;
    if (!(gamma > 0.0f)) { set_error("%s: gamma must be > 0 (got %g)", who, (double)gamma); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_pointers(B, preds && labels, who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, loss_q && grad, who)) return rc;
    if (B > 0) {
        PlArgs A{preds, labels, lens, B, L, S, top_k, gamma, temperature, distribution, seed, q0, unif, perm_out, nullptr, loss_q, grad, 0};
        if (int rc = pl_launch<true>(A, stream, who)) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}
