// The adversarial frame's list machines, IRGAN_List and IRFGAN_List: sampling the rankings the discriminator trains on, and both players'
// ranking-probability losses with their gradients.
//
// Reference: ptranking/ltr_adversarial/listwise/irgan_list.py:230-291 (per_query_generation), :294-312 (get_reward), :315-341 (the
//            discriminator's loss), :344-395 (the generator's step); listwise/irfgan_list.py:295, :322, :375 (the f-divergence forms);
//            util/list_probability.py:24-62 (log_ranking_prob_Plackett_Luce, _Bradley_Terry); util/list_sampling.py:16-36 (gumbel_softmax),
//            :70-87 (arg_shuffle_ties).
// The reference walks one query per optimiser step: S Gumbel-softmax rankings, a Python loop of fancy-indexing gathers, one torch.randperm
// per sample for the label ties, an [S, K, K] Bradley-Terry matrix, and autograd through softmax, sort and LogCumsumExp.  Here a padded
// batch [B, L] with lens takes one sampling launch and one fused loss launch per player; nothing of size K x K or [B, S, L] is stored.
//
// Orders.  A ranking is the rank of every document among its list, counted exactly: document i goes to position
// #{j : j before i}, "before" being (key descending, index ascending) for the generated rankings, key_i = preds_i + gumbel(u(s, i)) — the
// STPL keys of plsample.hip, so the first Kq positions are the prefix of ptr_pl_sample's perm — and (label descending, u(S + s, i)
// descending, index ascending) for the standard rankings: uniform among label ties, the law of arg_shuffle_ties.  Counting is integer
// work on exact comparisons: the rankings do not depend on the launch form.  Cost n^2 / G comparisons per thread and sample, keys read
// from LDS 16 bytes at a time as broadcasts.
//
// Ranking probabilities of v[0 .. K) held by position in LDS (al_lp_pl, al_lp_bt):
//   PL   lp = sum_p (v_p - L_p), L_p = log sum_{r >= p} e^{v_r}; thread t owns the positions t dpt .. t dpt + dpt - 1 (dpt = ceil(K / G)):
//        a suffix scan of e^{v - max} and a prefix scan of 1 / (suffix sum), both in DOUBLE, d lp / d v_r = 1 - e^{v_r} sum_{p <= r} e^{-L_p};
//        a ranking whose scores spread over more than 600 takes both scans in the LOG domain (fp32, lse2, grp_excl_*_lse), where no
//        exponent is ever positive, so neither scan can overflow or lose the tail.
//   BT   lp = sum_{p < r} log sigmoid(v_p - v_r), a pair loop (thread t owns positions t, t + G, ...), one exp per visited pair,
//        d lp / d v_p = sum_{r > p} sigmoid(v_r - v_p) - sum_{r < p} sigmoid(v_p - v_r).  K^2 / G pair visits per thread: the whole list of
//        a long query under BT is as quadratic as the reference's K x K matrix, just without storing it.
// Gradients are put together per document in one LDS row: a ranking names a document at most once, so the positions of ONE ranking add
// into distinct words, and the rankings are taken one after the other with a group barrier between them — a fixed order, no atomics.
// (ptr_adlist_fwd_bwd's discriminator mode relies on that: rankings that name a document twice are the caller's error; an index outside
// the list makes its query invalid.)
//
// exp(1 - lp) (the reward of repTrick = False, dropLog = True) overflows fp32 once lp < -87.7, i.e. for long rankings, as it does in the
// reference; non-finite values propagate as in IEEE arithmetic.
//
// Shape: as irgan.hip — a list of up to 256 documents takes one wavefront, four queries per workgroup; a longer one a workgroup of 256
// threads.  LDS per query: 2 rows of round_up(L, 4) words and 6 of round_up(min(K, L), 4) (sampler: 2 rows of round_up(L, 4)), + 8 words
// per workgroup.  A query's bits depend on (its data, L, S, K, the parameters, seed, q0 + q) alone.
#include "ptr_irgan.h"
#include "ptr_plhash.h"

namespace ptr {

// i's rank among the n documents of a list.  ONE key: (A descending, index ascending); TWO: (A descending, B descending, index
// ascending).  The rows hold round_up(n, 4) words, the padding after n ranks behind every document.  place(rank, i) per document.
template <int G, bool TWO, class P>
__device__ __forceinline__ void al_rank(const float *A, const float *Bk, int n, int t, P &&place) {
    const int n4 = (n + 3) & ~3;
    for (int base = t; base < n; base += 4 * G) {
        float a[4], b[4];
        int id[4], r[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            id[c] = base + c * G;
            const int i = min(id[c], n - 1);
            a[c] = A[i];
            b[c] = TWO ? Bk[i] : 0.0f;
            r[c] = 0;
        }
        for (int j = 0; j < n4; j += 4) {
            const float4 ka = *reinterpret_cast<const float4 *>(A + j);
            const float4 kb = TWO ? *reinterpret_cast<const float4 *>(Bk + j) : float4{0.0f, 0.0f, 0.0f, 0.0f};
            const float kaj[4] = {ka.x, ka.y, ka.z, ka.w}, kbj[4] = {kb.x, kb.y, kb.z, kb.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const bool tie = TWO ? (kbj[e] > b[c] || (kbj[e] == b[c] && j + e < id[c])) : j + e < id[c];
                    r[c] += (kaj[e] > a[c] || (kaj[e] == a[c] && tie)) ? 1 : 0;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (id[c] < n) place(r[c], id[c]);
    }
}

// exclusive scans and the sum over the G threads of a group in double (thread order, fixed order); `red`: 4 doubles of LDS (G == 256)
template <int G> __device__ __forceinline__ double al_excl_suffix_d(double v, double *red, int t) {
    const int lane = t & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_down(v, d, 64);
        if (lane + d < 64) v += o;
    }
    const double nx = __shfl_down(v, 1, 64);
    double ex = lane < 63 ? nx : 0.0;
    if constexpr (G != kWave) {
        __syncthreads();
        if (lane == 0) red[t >> 6] = v;
        __syncthreads();
        for (int w = G / kWave - 1; w > (t >> 6); --w) ex += red[w];
    }
    return ex;
}
template <int G> __device__ __forceinline__ double al_excl_prefix_d(double v, double *red, int t) {
    const int lane = t & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    const double pv = __shfl_up(v, 1, 64);
    double ex = lane > 0 ? pv : 0.0;
    if constexpr (G != kWave) {
        __syncthreads();
        if (lane == 63) red[t >> 6] = v;
        __syncthreads();
        for (int w = 0; w < (t >> 6); ++w) ex += red[w];
    }
    return ex;
}
template <int G> __device__ __forceinline__ double al_sum_d(double v, double *red, int t) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if constexpr (G != kWave) {
        __syncthreads();
        if ((t & 63) == 0) red[t >> 6] = v;
        __syncthreads();
        v = red[0];
#pragma unroll
        for (int w = 1; w < G / kWave; ++w) v += red[w];
    }
    return v;
}

constexpr float kAlSpread = 600.0f;      // exp(-600) is a normal double: below this spread of a ranking's scores no term of a sum is lost

// Plackett-Luce log-probability of the ranking V[0 .. K); GRAD: D[p] = d lp / d v_p, otherwise D is scratch.  Every thread gets lp.
// The sums run in DOUBLE, for two consumers.  The generator's gradient is c y_j (h_j - sum_i y_i h_i), a difference of numbers of order 1:
// h must be good to about 1e-8 absolute for the gradient to be good to 1e-5 relative, and an fp32 scan of sums that reach log K carries a
// few 1e-6.  The exponential rewards turn an ABSOLUTE error of lp into a RELATIVE error of every output, so lp leaves as a double.
// A spread beyond kAlSpread takes both scans in the LOG domain instead (fp32, lse2): no exponent is ever positive, nothing underflows.
template <int G, bool GRAD, class TV> __device__ __forceinline__ double al_lp_pl(const TV *V, double *D, int K, float *red, int t) {
    const int dpt = (K + G - 1) / G, lo = min(t * dpt, K), hi = min(lo + dpt, K);
    float m = -INFINITY, mn = -INFINITY;
    for (int p = lo; p < hi; ++p) {
        m = fmaxf(m, (float)V[p]);
        mn = fmaxf(mn, -(float)V[p]);
    }
    m = group_max<G>(m, red, t);
    mn = group_max<G>(mn, red, t);
    double *redd = reinterpret_cast<double *>(red);
    if (m + mn <= kAlSpread) {
        double run = 0.0;
        for (int p = hi - 1; p >= lo; --p) {
            run += exp((double)V[p] - (double)m);
            D[p] = run;
        }
        const double ex = al_excl_suffix_d<G>(run, redd, t);
        double lp = 0.0, pr = 0.0;
        for (int p = lo; p < hi; ++p) {
            const double T = D[p] + ex;                                      // sum_{r >= p} e^{v_r - m}
            lp += ((double)V[p] - (double)m) - log(T);
            if constexpr (GRAD) {
                pr += 1.0 / T;
                D[p] = pr;
            }
        }
        if constexpr (GRAD) {
            const double px = al_excl_prefix_d<G>(pr, redd, t);
            for (int p = lo; p < hi; ++p) D[p] = 1.0 - exp((double)V[p] - (double)m) * (D[p] + px);
        }
        return al_sum_d<G>(lp, redd, t);
    }
    float run = -INFINITY;
    for (int p = hi - 1; p >= lo; --p) {
        run = lse2((float)V[p] - m, run);
        D[p] = (double)run;
    }
    const float ex = grp_excl_suffix_lse<G>(run, red, t);
    float lp = 0.0f, pr = -INFINITY;
    for (int p = lo; p < hi; ++p) {
        const float lam = lse2((float)D[p], ex);                             // L_p - m
        lp += ((float)V[p] - m) - lam;
        if constexpr (GRAD) {
            pr = lse2(pr, -lam);
            D[p] = (double)pr;
        }
    }
    if constexpr (GRAD) {
        const float px = grp_excl_prefix_lse<G>(pr, red, t);
        for (int p = lo; p < hi; ++p) D[p] = (double)(1.0f - expf(((float)V[p] - m) + lse2((float)D[p], px)));
    }
    return (double)group_sum<G>(lp, red, t);
}

// Bradley-Terry log-probability of the ranking V[0 .. K) (list_probability.py:44-62: e_p / (e_p + e_r) is sigmoid(v_p - v_r))
// The pair terms are fp32 (one exp and one log1p each); their sum, up to K^2 / 2 of them, is kept in double.
template <int G, bool GRAD> __device__ __forceinline__ double al_lp_bt(const float *V, double *D, int K, float *red, int t) {
    double lp = 0.0;
    for (int p = t; p < K; p += G) {
        const float vp = V[p];
        float d = 0.0f;
        for (int r = 0; r < K; ++r) {
            if (r == p) continue;
            const float z = vp - V[r], e = expf(-fabsf(z)), inv = 1.0f / (1.0f + e);
            if (r > p) {
                lp += (double)(fminf(z, 0.0f) - log1pf(e));                  // log sigmoid(z)
                d += z >= 0.0f ? e * inv : inv;                              // sigmoid(-z)
            } else {
                d -= z >= 0.0f ? inv : e * inv;                              // sigmoid(z)
            }
        }
        if constexpr (GRAD) D[p] = (double)d;
    }
    return al_sum_d<G>(lp, reinterpret_cast<double *>(red), t);
}

template <int G, bool GRAD> __device__ __forceinline__ double al_lp(int prob, const float *V, double *D, int K, float *red, int t) {
    return prob == PTR_ADLIST_PL ? al_lp_pl<G, GRAD, float>(V, D, K, red, t) : al_lp_bt<G, GRAD>(V, D, K, red, t);
}

__device__ __forceinline__ int al_kq(int top_k, int n) { return top_k <= 0 ? n : min(top_k, n); }

// ---------------------------------------------------------------------------------------------------------------- the sampler
struct AlSampleArgs {
    const float *preds, *labels;
    const int32_t *lens;
    int B, L, S, top_k, Kw;
    uint64_t seed;
    int64_t q0;
    const float *unif;
    int64_t *std_idx, *gen_idx;
    int32_t *kq;
};

// LDS per query: KA | KB (round_up(L, 4) floats each), + 8 words per workgroup
template <int G> __global__ void __launch_bounds__(kBlock) adlist_sample_kernel(const AlSampleArgs A, int Lp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int QPB = kBlock / G;
    const int grp = G == kWave ? threadIdx.x >> 6 : 0, t = G == kWave ? threadIdx.x & 63 : threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * QPB + grp);
    if (q >= A.B) return;                                                    // G == 64: wave-level synchronisation only below
    float *KA = smem + (size_t)grp * 2 * Lp, *KB = KA + Lp, *red = smem + (size_t)QPB * 2 * Lp;
    const int L = A.L, S = A.S, Kw = A.Kw;
    const int n = query_len(A.lens, q, L);
    const float *s = A.preds + (size_t)q * L, *y = A.labels + (size_t)q * L;
    bool bad = false;
    for (int i = t; i < n; i += G) bad |= s[i] != s[i];
    const bool nanq = group_any<G>(bad, reinterpret_cast<int *>(red), t);
    const int Kq = nanq ? 0 : al_kq(A.top_k, n);
    if (t == 0) A.kq[q] = Kq;
    const PlKeys qk = pl_query_keys(A.seed, A.q0 + (int64_t)q);
    for (int smp = 0; smp < S; ++smp) {
        int64_t *gen = A.gen_idx + ((size_t)q * S + smp) * Kw, *std_ = A.std_idx + ((size_t)q * S + smp) * Kw;
        for (int p = Kq + t; p < Kw; p += G) { gen[p] = 0; std_[p] = 0; }
        if (Kq == 0) continue;                                               // uniform over the group
        const float *ug = A.unif ? A.unif + ((size_t)q * 2 * S + smp) * L : nullptr;
        const float *us = A.unif ? A.unif + ((size_t)q * 2 * S + S + smp) * L : nullptr;
        const PlKeys kg = pl_sample_keys(qk, (uint32_t)smp), ks = pl_sample_keys(qk, (uint32_t)(S + smp));
        for (int i = t; i < Lp; i += G) KA[i] = i < n ? s[i] + pl_gumbel(ug ? ug[i] : pl_uniform(kg, (uint32_t)i)) : -INFINITY;
        group_sync<G>();
        al_rank<G, false>(KA, nullptr, n, t, [&](int r, int i) { if (r < Kq) gen[r] = (int64_t)i; });
        group_sync<G>();
        for (int i = t; i < Lp; i += G) {
            KA[i] = i < n ? y[i] : -INFINITY;
            KB[i] = i < n ? (us ? us[i] : pl_uniform(ks, (uint32_t)i)) : -1.0f;
        }
        group_sync<G>();
        al_rank<G, true>(KA, KB, n, t, [&](int r, int i) { if (r < Kq) std_[r] = (int64_t)i; });
        group_sync<G>();
    }
}

// ---------------------------------------------------------------------------------------------------------------- the losses
struct AlLossArgs {
    const float *x, *d_preds;
    const int64_t *std_idx, *gen_idx;
    const int32_t *kq, *lens;
    int B, L, S, top_k, Kw, mode, prob, family, reward, f_div;
    float temperature;
    uint64_t seed;
    int64_t q0;
    const float *unif;
    float *loss_q, *valid_q, *grad;
    int64_t *gen_idx_out;
};

// the generator's reward from the discriminator's log-probability of a ranking (irgan_list.py:301-310; irfgan_list.py:295)
// (the exponentials in double: a rounding of lp to fp32, 2^-24 |lp|, would reach every output as a relative error)
__device__ __forceinline__ double al_reward(int family, int reward, int f_div, double lp) {
    if (family == PTR_ADLIST_IRFGAN) {
        float c, dc;
        fg_conj(f_div, (float)lp, c, dc);
        return (double)c;
    }
    switch (reward) {
        case PTR_ADLIST_REWARD_NEG_EXP: return -exp(lp);
        case PTR_ADLIST_REWARD_NEG_LP: return -lp;
        case PTR_ADLIST_REWARD_EXP_1M: return exp(1.0 - lp);
        default: return log1p(-lp);                                          // PTR_ADLIST_REWARD_LOG_1M: log(1 - lp), lp <= 0
    }
}

// LDS per query: XK | GA (Lp floats each) | V | D (Kp doubles each; V floats in the D mode) | W | IDX (Kp words each), + 8 words per workgroup.
//   D mode: XK the scores by document, V a ranking's scores by position, D its d lp / d v, IDX its documents.
//   G mode: XK the keys x + gumbel, then the probabilities y by document; V the top probabilities in double, W the discriminator's scores,
//           by position.
template <int G> __global__ void __launch_bounds__(kBlock) adlist_loss_kernel(const AlLossArgs A, int Lp, int Kp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int QPB = kBlock / G;
    const int grp = G == kWave ? threadIdx.x >> 6 : 0, t = G == kWave ? threadIdx.x & 63 : threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * QPB + grp);
    if (q >= A.B) return;
    const size_t per = (size_t)2 * Lp + 6 * Kp;
    float *XK = smem + grp * per, *GA = XK + Lp, *V = GA + Lp, *W = V + 4 * Kp, *red = smem + QPB * per;
    double *Vd = reinterpret_cast<double *>(V), *D = Vd + Kp;                // 8-byte aligned: Lp and Kp are multiples of 4
    int *IDX = reinterpret_cast<int *>(W + Kp);
    const int L = A.L, S = A.S, Kw = A.Kw;
    const int n = query_len(A.lens, q, L);
    const float *x = A.x + (size_t)q * L;
    float *g = A.grad + (size_t)q * L;
    const bool fgan = A.family == PTR_ADLIST_IRFGAN;
    const float invS = 1.0f / (float)S;
    auto nothing = [&]() {
        for (int i = t; i < L; i += G) g[i] = 0.0f;
        if (t == 0) { A.loss_q[q] = 0.0f; A.valid_q[q] = 0.0f; }
    };
    float loss = 0.0f;
    if (A.mode == PTR_ADLIST_D) {
        const int Kq = min(min(max(A.kq[q], 0), n), Kw);
        const int64_t *sq = A.std_idx + (size_t)q * S * Kw, *gq = A.gen_idx + (size_t)q * S * Kw;
        bool bad = false;
        for (int k = t; k < S * Kq; k += G) {
            const size_t o = (size_t)(k / Kq) * Kw + k % Kq;
            const int64_t a = sq[o], b = gq[o];
            bad |= a < 0 || a >= (int64_t)n || b < 0 || b >= (int64_t)n;
        }
        const bool out = group_any<G>(bad, reinterpret_cast<int *>(red), t);
        if (Kq == 0 || out) { nothing(); return; }
        for (int i = t; i < n; i += G) { XK[i] = x[i]; GA[i] = 0.0f; }
        group_sync<G>();
        for (int smp = 0; smp < S; ++smp) {
            for (int which = 0; which < 2; ++which) {                        // 0: the standard ranking, 1: the generated one
                const int64_t *row = (which ? gq : sq) + (size_t)smp * Kw;
                for (int p = t; p < Kq; p += G) {
                    const int d = (int)row[p];
                    IDX[p] = d;
                    V[p] = XK[d];
                }
                group_sync<G>();
                const float lp = (float)al_lp<G, true>(A.prob, V, D, Kq, red, t);
                float coef;
                if (fgan) {                                                  // irfgan_list.py:322
                    float a, da;
                    if (which) fg_conj(A.f_div, lp, a, da); else fg_act(A.f_div, lp, a, da);
                    loss += which ? a * invS : -a * invS;
                    coef = which ? da * invS : -da * invS;
                } else if (which) {                                          // irgan_list.py:336-337
                    loss -= log1pf(-lp);
                    coef = 1.0f / (1.0f - lp);
                } else {
                    loss -= lp;
                    coef = -1.0f;
                }
                group_sync<G>();
                for (int p = t; p < Kq; p += G) GA[IDX[p]] += coef * (float)D[p];
                group_sync<G>();
            }
        }
        for (int i = t; i < L; i += G) g[i] = i < n ? GA[i] : 0.0f;
        if (t == 0) { A.loss_q[q] = loss; A.valid_q[q] = 1.0f; }
        return;
    }
    // ---- the generator (irgan_list.py:344-395): S rankings drawn here, A_s = lp_PL of the top probabilities, R_s from the discriminator
    const float *dp = A.d_preds + (size_t)q * L;
    bool bad = false;
    for (int i = t; i < n; i += G) bad |= x[i] != x[i];
    const bool nanq = group_any<G>(bad, reinterpret_cast<int *>(red), t);
    const int Kq = nanq ? 0 : al_kq(A.top_k, n);
    if (A.gen_idx_out)
        for (int smp = 0; smp < S; ++smp)
            for (int p = Kq + t; p < Kw; p += G) A.gen_idx_out[((size_t)q * S + smp) * Kw + p] = 0;
    if (Kq == 0) { nothing(); return; }
    for (int i = t; i < n; i += G) GA[i] = 0.0f;
    const PlKeys qk = pl_query_keys(A.seed, A.q0 + (int64_t)q);
    const float T = A.temperature;
    for (int smp = 0; smp < S; ++smp) {
        const float *ug = A.unif ? A.unif + ((size_t)q * S + smp) * L : nullptr;
        const PlKeys kg = pl_sample_keys(qk, (uint32_t)smp);
        float m = -INFINITY;
        for (int i = t; i < Lp; i += G) {
            const float k = i < n ? x[i] + pl_gumbel(ug ? ug[i] : pl_uniform(kg, (uint32_t)i)) : -INFINITY;
            XK[i] = k;
            m = fmaxf(m, k);
        }
        m = group_max<G>(m, red, t);                                        // its barriers publish XK (G == 256)
        group_sync<G>();
        int64_t *gout = A.gen_idx_out ? A.gen_idx_out + ((size_t)q * S + smp) * Kw : nullptr;
        al_rank<G, false>(XK, nullptr, n, t, [&](int r, int i) {
            if (r < Kq) {
                IDX[r] = i;
                W[r] = dp[i];
                if (gout) gout[r] = (int64_t)i;
            }
        });
        group_sync<G>();
        const double lpd = al_lp<G, false>(A.prob, W, D, Kq, red, t);        // the discriminator's lp of the ranking; D is its scratch here
        // y = softmax((x + gumbel) / T) through the log-softmax.  The normaliser and the top probabilities in DOUBLE: a top probability
        // near 1 meets sum_i y_i h_i in the gradient as 1 - y, which an fp32 Z (one rounding of a number just above 1) leaves 1e-5 off.
        double zs = 0.0;
        for (int i = t; i < n; i += G) zs += exp(((double)XK[i] - (double)m) / (double)T);
        const double logZ = log(al_sum_d<G>(zs, reinterpret_cast<double *>(red), t));
        group_sync<G>();
        for (int p = t; p < Kq; p += G) Vd[p] = exp(((double)XK[IDX[p]] - (double)m) / (double)T - logZ);
        group_sync<G>();                                                     // every thread is past its reads of the keys
        for (int i = t; i < n; i += G) XK[i] = expf((XK[i] - m) / T - (float)logZ);
        group_sync<G>();
        const double As = al_lp_pl<G, true, double>(Vd, D, Kq, red, t);      // the PL of the PROBABILITIES, as the reference takes it (:379)
        group_sync<G>();
        double hs = 0.0;
        for (int p = t; p < Kq; p += G) hs += Vd[p] * D[p];
        const double H = al_sum_d<G>(hs, reinterpret_cast<double *>(red), t);    // sum_i y_i h_i
        const double R = al_reward(A.family, A.reward, A.f_div, lpd);
        const double sgn = fgan ? -(double)invS : (double)invS;                              // irgan_list.py:391, irfgan_list.py:375
        loss += (float)(sgn * As * R);
        const double c = sgn * R / (double)T;
        group_sync<G>();
        for (int p = t; p < Kq; p += G) {                                    // a top document: c y (h - H), the difference taken in double
            const int i = IDX[p];
            GA[i] += (float)(c * Vd[p] * (D[p] - H));
            XK[i] = 0.0f;                                                    // the loop below is for the others
        }
        group_sync<G>();
        for (int i = t; i < n; i += G) GA[i] -= (float)(c * (double)XK[i] * H);
        group_sync<G>();
    }
    for (int i = t; i < L; i += G) g[i] = i < n ? GA[i] : 0.0f;
    if (t == 0) { A.loss_q[q] = loss; A.valid_q[q] = 1.0f; }
}

IrganForm adlist_form(int L) { return irgan_form(L); }

static int al_check(const char *who, int B, int L, int S, int top_k) {
    if (int rc = ig_check_shape(who, B, L, 1.0f)) return rc;
    if (int rc = ig_check_samples(who, S)) return rc;
    if (top_k > PTR_MAX_LIST_LEN) { set_error("%s: top_k %d exceeds PTR_MAX_LIST_LEN=%d (top_k <= 0: the whole list)", who, top_k, PTR_MAX_LIST_LEN); return PTR_ERR_INVALID_ARG; }
    return 0;
}

}  // namespace ptr

extern "C" int ptr_adlist_sample(const float *preds, const float *labels, const int32_t *lens, int B, int L, int S, int top_k, uint64_t seed,
                                 int64_t q0, const float *unif, int64_t *std_idx, int64_t *gen_idx, int32_t *kq, void *stream) {
    using namespace ptr;
    const char *who = "ptr_adlist_sample";
    if (int rc = al_check(who, B, L, S, top_k)) return rc;
    if (int rc = check_pointers(B, preds && labels, who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, std_idx && gen_idx && kq, who)) return rc;
    if (B == 0) return 0;
    const AlSampleArgs A{preds, labels, lens, B, L, S, top_k, top_k <= 0 ? L : top_k, seed, q0, unif, std_idx, gen_idx, kq};
    const int Lp = round_up(L, 4);
    if (adlist_form(L).G == kWave)
        return launch_queries(adlist_sample_kernel<kWave>, B, kBlock / kWave, kBlock, ((size_t)(kBlock / kWave) * 2 * Lp + 8) * sizeof(float), stream, who, A, Lp);
    return launch_queries(adlist_sample_kernel<kBlock>, B, 1, kBlock, ((size_t)2 * Lp + 8) * sizeof(float), stream, who, A, Lp);
}

extern "C" int ptr_adlist_fwd_bwd(const float *x, const float *d_preds, const int64_t *std_idx, const int64_t *gen_idx, const int32_t *kq,
                                  const int32_t *lens, int B, int L, int S, int top_k, int mode, int prob, int family, int reward, int f_div,
                                  float temperature, uint64_t seed, int64_t q0, const float *unif, float *loss_out, float *loss_q,
                                  float *valid_q, float *grad, int64_t *gen_idx_out, void *stream) {
    using namespace ptr;
    const char *who = "ptr_adlist_fwd_bwd";
    if (int rc = ig_check_shape(who, B, L, temperature)) return rc;
    if (int rc = al_check(who, B, L, S, top_k)) return rc;
    if (mode != PTR_ADLIST_D && mode != PTR_ADLIST_G) { set_error("%s: mode %d (PTR_ADLIST_D, PTR_ADLIST_G)", who, mode); return PTR_ERR_INVALID_ARG; }
    if (prob != PTR_ADLIST_PL && prob != PTR_ADLIST_BT) { set_error("%s: prob %d (PTR_ADLIST_PL, PTR_ADLIST_BT)", who, prob); return PTR_ERR_INVALID_ARG; }
    if (family != PTR_ADLIST_IRGAN && family != PTR_ADLIST_IRFGAN) { set_error("%s: family %d (PTR_ADLIST_IRGAN, PTR_ADLIST_IRFGAN)", who, family); return PTR_ERR_INVALID_ARG; }
    if (reward < PTR_ADLIST_REWARD_NEG_EXP || reward > PTR_ADLIST_REWARD_LOG_1M) { set_error("%s: reward %d (PTR_ADLIST_REWARD_*)", who, reward); return PTR_ERR_INVALID_ARG; }
    if (f_div < PTR_FDIV_TVAR || f_div > PTR_FDIV_GAN) { set_error("%s: f_div %d (PTR_FDIV_*)", who, f_div); return PTR_ERR_INVALID_ARG; }
    const bool gen = mode == PTR_ADLIST_G;
    if (int rc = check_pointers(B, x && (gen ? d_preds != nullptr : (std_idx && gen_idx && kq)), who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, loss_q && valid_q && grad, who)) return rc;
    if (B > 0) {
        const int Kw = top_k <= 0 ? L : top_k;
        const AlLossArgs A{x, d_preds, std_idx, gen_idx, kq, lens, B, L, S, top_k, Kw, mode, prob, family, reward, f_div, temperature, seed, q0, unif,
                           loss_q, valid_q, grad, gen ? gen_idx_out : nullptr};
        const int Lp = round_up(L, 4), Kp = round_up(Kw < L ? Kw : L, 4);
        const size_t per = (size_t)2 * Lp + 6 * Kp;
        int rc;
        if (adlist_form(L).G == kWave)
            rc = launch_queries(adlist_loss_kernel<kWave>, B, kBlock / kWave, kBlock, ((size_t)(kBlock / kWave) * per + 8) * sizeof(float), stream, who, A, Lp, Kp);
        else
            rc = launch_queries(adlist_loss_kernel<kBlock>, B, 1, kBlock, (per + 8) * sizeof(float), stream, who, A, Lp, Kp);
        if (rc) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}
