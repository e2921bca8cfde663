// The adversarial frame's IRGAN point and pair machines: sampling documents from the generator's distribution and the two players' losses.
//
// Reference: ptranking/ltr_adversarial/pointwise/irgan_point.py:130-146 (per_query_generation), :161-169 (the discriminator's loss),
//            :184-217 (the generator's step); ptranking/ltr_adversarial/pairwise/irgan_pair.py:140-161, :180-184, :39-42, :207-218.
// The reference runs one query per step through torch.multinomial, torch.randperm, fancy indexing and autograd; here a padded batch
// [B, L] with lens and num_pos (the relevant documents sit at the front of a list, train_presort) takes one launch per piece.
//
// Sampling rules (include/ptranking_amd.h states them for callers):
//   with replacement     inverse CDF on the inclusive prefix sum C of the unnormalised weights w_i: draw k names the smallest i with
//                        u_k * C_{n-1} < C_i, the last document when there is none, and from there the nearest document at or below with
//                        w_i > 0 (in exact arithmetic the first rule never names a document of zero weight; a prefix sum built as a tree
//                        of fp32 additions can move by an ulp between two neighbours that differ by a zero term).  The same holds
//                        at a tile boundary of a list longer than one tile (prefix_into): inside a tile C_i is the carry plus the
//                        tile's scan, while the carry moves on by the tile's butterfly sum, another order of the same additions, so
//                        the first C of a tile can lie an ulp or so BELOW the last C of the tile before it, whatever the weights.
//                        Only a draw x inside that gap of an ulp or so sees it, and the binary search then ends within one document
//                        of the boundary (the last of the earlier tile, or the second of the later one if it probes the first):
//                        fp32 rounding of C moves draws that close to any boundary to a neighbour as well, and the law moves by
//                        that much (tests keep supplied uniforms 2^-12 of the total away from every boundary).
//   without replacement  V rounds of arg-max over key_i = log-weight_i + gumbel(u_i), (key descending, index ascending): the law of
//                        torch.multinomial(replacement=False) with no weight that can underflow (plsample.hip).
//   positives            the V largest of P uniform keys, (key descending, index ascending): the law of randperm(P)[:V].
// Uniforms: pl_uniform (plsample.hip's counter hash) keyed by (seed, q0 + q, stream, index).  ptr_irgan_sample: stream 0 index i = the
// key of positive i, stream 1 index k = draw k (with replacement) or index i = document i (without).  ptr_irgan_point_gen_fwd_bwd: draw k
// is stream k / L, index k % L.  A caller's `unif` array replaces the hash with the same layout, [B, streams, L]: ptr_pl_uniforms writes it.
//
// Shape: a list of up to 256 documents takes one wavefront, four queries per workgroup; a longer one a workgroup of 256 threads.  Scores,
// weights and prefix sums live in LDS rows of round_up(L, 4) floats, thread t walks documents t, t + G, ...  (a wavefront reads 64
// consecutive floats: no bank conflict).  Below 256 documents a lane walks at most four documents per pass and the arg-max rounds and
// scans need no workgroup barrier; above, four waves share the walk and a round costs two barriers.  No floating-point atomics: sums are
// butterflies and fixed-order scans; the draw counts are integer LDS atomics, exact in any order.  A query's bits depend on (its data, L,
// the parameters, seed, q0 + q) alone.  Nothing of size L x L.
// The stable softplus family, the group helpers (group_any, group_argmax, take_largest, prefix_into, inverse_cdf) and the argument checks
// live in ptr_irgan.h, which irfgan.hip shares.
#include "ptr_irgan.h"
#include "ptr_plhash.h"

namespace ptr {

struct IgSampleArgs {
    const float *preds;
    const int32_t *lens, *num_pos;
    int B, L, S, mode;
    float temperature;
    uint64_t seed;
    int64_t q0;
    const float *unif;
    int64_t *pos_idx, *neg_idx;
    int32_t *nsel;
};

// LDS per query: K | E (round_up(L, 4) floats each), + 8 words per workgroup (G == 256)
template <int G> __global__ void __launch_bounds__(kBlock) irgan_sample_kernel(const IgSampleArgs A, int Lp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int QPB = kBlock / G;
    const int grp = G == kWave ? threadIdx.x >> 6 : 0, t = G == kWave ? threadIdx.x & 63 : threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * QPB + grp);
    if (q >= A.B) return;                                                    // G == 64: wave-level synchronisation only below
    float *K = smem + (size_t)grp * 2 * Lp, *E = K + Lp, *red = smem + (size_t)QPB * 2 * Lp;
    const int L = A.L, S = A.S;
    const int n = query_len(A.lens, q, L);
    const int P = min(max(A.num_pos[q], 0), n);
    const float *s = A.preds + (size_t)q * L;
    bool bad = false;
    for (int i = t; i < n; i += G) bad |= s[i] != s[i];
    const bool nanq = group_any<G>(bad, reinterpret_cast<int *>(red), t);
    int V = A.mode == PTR_IRGAN_POINT_D ? min(P, S) : min(min(P, n - P), S);
    if (nanq) V = 0;                                                         // a list with a NaN score is not sampled
    int64_t *pos = A.pos_idx + (size_t)q * S, *neg = A.neg_idx + (size_t)q * S;
    for (int k = V + t; k < S; k += G) { pos[k] = 0; neg[k] = 0; }
    if (t == 0) A.nsel[q] = V;
    if (V == 0) return;
    const PlKeys qk = pl_query_keys(A.seed, A.q0 + (int64_t)q);
    const PlKeys k0 = pl_sample_keys(qk, 0u), k1 = pl_sample_keys(qk, 1u);
    const float *u0 = A.unif ? A.unif + (size_t)q * 2 * L : nullptr, *u1 = u0 ? u0 + L : nullptr;
    // positives: the V largest of P uniform keys
    for (int i = t; i < P; i += G) K[i] = u0 ? u0[i] : pl_uniform(k0, (uint32_t)i);
    group_sync<G>();
    take_largest<G>(K, P, V, pos, red, t);
    const bool t1 = A.temperature == 1.0f;
    if (A.mode == PTR_IRGAN_POINT_D) {
        float m = -INFINITY;
        for (int i = t; i < n; i += G) m = fmaxf(m, t1 ? s[i] : s[i] / A.temperature);
        m = group_max<G>(m, red, t);
        for (int i = t; i < n; i += G) E[i] = expf((t1 ? s[i] : s[i] / A.temperature) - m);
        group_sync<G>();
        const float total = prefix_into<G>(K, n, red, t, [&](int i) { return E[i]; });
        if (t < V) {
            const float u = u1 ? u1[t] : pl_uniform(k1, (uint32_t)t);
            neg[t] = (int64_t)inverse_cdf(K, n, u * total, [&](int i) { return E[i] == 0.0f; });
        }
        return;
    }
    const int first = A.mode == PTR_IRGAN_PAIR_D ? P : 0;
    for (int i = t; i < n; i += G) {
        const float z = t1 ? s[i] : s[i] / A.temperature;
        const float lw = A.mode == PTR_IRGAN_PAIR_D ? z : ig_logsigmoid(z);
        K[i] = i >= first ? lw + pl_gumbel(u1 ? u1[i] : pl_uniform(k1, (uint32_t)i)) : -INFINITY;
    }
    group_sync<G>();
    take_largest<G>(K, n, V, neg, red, t);
}

struct IgGenArgs {
    const float *g_preds, *d_preds;
    const int32_t *lens, *num_pos;
    int B, L;
    float temperature, lambda;
    int draws_per_pos;
    uint64_t seed;
    int64_t q0;
    const float *unif;
    float *loss_q, *valid_q, *grad;
    int32_t *counts;
};

// LDS per query: E | C | CNT (round_up(L, 4) words each), + 8 words per workgroup
template <int G> __global__ void __launch_bounds__(kBlock) irgan_point_gen_kernel(const IgGenArgs A, int Lp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int QPB = kBlock / G;
    const int grp = G == kWave ? threadIdx.x >> 6 : 0, t = G == kWave ? threadIdx.x & 63 : threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * QPB + grp);
    if (q >= A.B) return;
    float *E = smem + (size_t)grp * 3 * Lp, *C = E + Lp, *red = smem + (size_t)QPB * 3 * Lp;
    int *CNT = reinterpret_cast<int *>(C + Lp);
    const int L = A.L;
    const int n = query_len(A.lens, q, L);
    const int P = min(max(A.num_pos[q], 0), n);
    const float *s = A.g_preds + (size_t)q * L, *d = A.d_preds + (size_t)q * L;
    float *g = A.grad + (size_t)q * L;
    int32_t *cnt_out = A.counts ? A.counts + (size_t)q * L : nullptr;
    bool bad = false;
    for (int i = t; i < n; i += G) bad |= s[i] != s[i];
    const bool nanq = group_any<G>(bad, reinterpret_cast<int *>(red), t);
    if (P == 0 || nanq) {                                                    // irgan_point.py:185 `continue`, then :191-195 a NaN prediction
        const bool nanl = nanq && P > 0;
        const float fill = nanl ? __builtin_nanf("") : 0.0f;
        for (int i = t; i < L; i += G) {
            g[i] = i < n ? fill : 0.0f;
            if (cnt_out) cnt_out[i] = 0;
        }
        if (t == 0) { A.loss_q[q] = fill; A.valid_q[q] = nanl ? 1.0f : 0.0f; }
        return;
    }
    const bool t1 = A.temperature == 1.0f;
    const float lam = A.lambda;
    float m = -INFINITY;
    for (int i = t; i < n; i += G) m = fmaxf(m, t1 ? s[i] : s[i] / A.temperature);
    m = group_max<G>(m, red, t);
    float zs = 0.0f;
    for (int i = t; i < n; i += G) {
        const float e = expf((t1 ? s[i] : s[i] / A.temperature) - m);
        E[i] = e;
        CNT[i] = 0;
        zs += e;
    }
    const float Z = group_sum<G>(zs, red, t);
    const float boost = lam * Z / (float)P;                                  // q_i Z = (1 - lambda) e_i + [i < P] lambda Z / P  (:199-201)
    group_sync<G>();
    const float total = prefix_into<G>(C, n, red, t, [&](int i) { return (1.0f - lam) * E[i] + (i < P ? boost : 0.0f); });
    const int K = A.draws_per_pos * P;                                       // :203
    const PlKeys qk = pl_query_keys(A.seed, A.q0 + (int64_t)q);
    const float *uq = A.unif ? A.unif + (size_t)q * A.draws_per_pos * L : nullptr;
    for (int k = t; k < K; k += G) {
        const float u = uq ? uq[k] : pl_uniform(pl_sample_keys(qk, (uint32_t)(k / L)), (uint32_t)(k % L));
        const int i = inverse_cdf(C, n, u * total, [&](int j) { return (1.0f - lam) * E[j] + (j < P ? boost : 0.0f) == 0.0f; });
        atomicAdd(&CNT[i], 1);
    }
    group_sync<G>();
    // loss = -(1/K) sum_i c_i r_i log p_i rho_i, rho = p / q (:205-210); with a_i = [i < P] lambda / P:
    //   h_i = -(1/K) c_i r_i rho_i (1 + log p_i a_i / q_i),   d loss / d z_j = h_j - p_j sum_i h_i,   z = g_preds / T
    const float logZ = logf(Z), invK = 1.0f / (float)K;
    float ls = 0.0f, hs = 0.0f;
    for (int i = t; i < n; i += G) {
        const int c = CNT[i];
        float h = 0.0f;
        if (c > 0) {
            const float e = E[i], wq = (1.0f - lam) * e + (i < P ? boost : 0.0f);
            const float logp = ((t1 ? s[i] : s[i] / A.temperature) - m) - logZ;
            const float rho = e / wq, r = 2.0f * (d[i] - 0.5f);              // :42 the reward
            const float cr = -invK * (float)c * r * rho;
            ls += cr * logp;
            h = cr * (1.0f + logp * (i < P ? boost : 0.0f) / wq);
        }
        C[i] = h;                                                            // the prefix sums are spent
        hs += h;
    }
    const float loss = group_sum<G>(ls, red, t);
    const float H = group_sum<G>(hs, red, t);
    group_sync<G>();
    const float invT = t1 ? 1.0f : 1.0f / A.temperature;
    for (int i = t; i < L; i += G) {
        g[i] = i < n ? (C[i] - (E[i] / Z) * H) * invT : 0.0f;
        if (cnt_out) cnt_out[i] = i < n ? CNT[i] : 0;
    }
    if (t == 0) { A.loss_q[q] = loss; A.valid_q[q] = 1.0f; }
}

struct IgSelArgs {
    const float *x, *d_sel;
    const int64_t *neg_idx;
    const int32_t *nsel, *lens;
    int B, L, S, mode;
    float temperature;
    float *loss_q, *valid_q, *grad;
};

// One group per query; the first wavefront holds the V <= 64 samples, one per lane.  The gradient row is put together in LDS (W words per
// query: zeros, then the V or 2 V entries) and leaves with one coalesced store per element.
template <int G> __global__ void __launch_bounds__(kBlock) irgan_sel_kernel(const IgSelArgs A, int Wp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int QPB = kBlock / G;
    const int grp = G == kWave ? threadIdx.x >> 6 : 0, t = G == kWave ? threadIdx.x & 63 : threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * QPB + grp);
    if (q >= A.B) return;
    const int S = A.S, V = min(max(A.nsel[q], 0), S);
    const bool gen = A.mode >= PTR_IRGAN_SEL_PAIR_G_SVM;
    const int W = gen ? A.L : 2 * S;
    float *R = smem + (size_t)grp * Wp;
    float *g = A.grad + (size_t)q * W;
    for (int i = t; i < W; i += G) R[i] = 0.0f;
    group_sync<G>();
    if (t < kWave) {                                                         // G == 256: the first wave does the arithmetic
        float term = 0.0f;
        const float invV = 1.0f / (float)max(V, 1);
        if (t < V) {
            const float *ds = (gen ? A.d_sel : A.x) + (size_t)q * 2 * S;
            const float dp = ds[t], dn = ds[V + t];
            if (A.mode == PTR_IRGAN_SEL_POINT_D) {                           // irgan_point.py:161-169, labels 1 | 0, mean over 2 V
                term = (ig_softplus(-dp) + ig_softplus(dn)) * (0.5f * invV);
                R[t] = -ig_sigmoid(-dp) * (0.5f * invV);
                R[V + t] = ig_sigmoid(dn) * (0.5f * invV);
            } else if (A.mode == PTR_IRGAN_SEL_PAIR_D_SVM) {                 // irgan_pair.py:182
                const float x = 1.0f - (dp - dn);
                const float sub = x > 0.0f ? 1.0f : x == 0.0f ? 0.5f : x != x ? x : 0.0f;   // torch.max of two tensors halves the gradient at a tie
                term = (x != x ? x : fmaxf(0.0f, x)) * invV;
                R[t] = -sub * invV;
                R[V + t] = sub * invV;
            } else if (A.mode == PTR_IRGAN_SEL_PAIR_D_LOG) {                 // :184
                const float x = dp - dn;
                term = -ig_logsigmoid(x) * invV;
                R[t] = -ig_sigmoid(-x) * invV;
                R[V + t] = ig_sigmoid(-x) * invV;
            } else {                                                         // :39-42 the reward, :216-218 the generator's loss
                const float reward = A.mode == PTR_IRGAN_SEL_PAIR_G_SVM ? ig_sigmoid(fmaxf(0.0f, 1.0f - (dp - dn))) : ig_logsigmoid(dn - dp);
                const int64_t doc = A.neg_idx[(size_t)q * S + t];
                if (doc >= 0 && doc < (int64_t)query_len(A.lens, q, A.L)) {   // an index outside the list names nothing
                    const float sc = A.x[(size_t)q * A.L + doc];
                    const float z = A.temperature == 1.0f ? sc : sc / A.temperature;
                    term = -ig_logsigmoid(z) * reward * invV;
                    R[doc] = -ig_sigmoid(-z) * reward * invV / A.temperature;
                }
            }
        }
        term = wave_sum(term);
        if (t == 0) { A.loss_q[q] = term; A.valid_q[q] = V > 0 ? 1.0f : 0.0f; }
    }
    group_sync<G>();
    for (int i = t; i < W; i += G) g[i] = R[i];
}

IrganForm irgan_form(int L) { return L <= 256 ? IrganForm{kWave, kBlock / kWave} : IrganForm{kBlock, 1}; }
IrganForm irgan_sel_form(int mode, int L) { return mode >= PTR_IRGAN_SEL_PAIR_G_SVM ? irgan_form(L) : IrganForm{kWave, kBlock / kWave}; }

}  // namespace ptr

extern "C" int ptr_irgan_sample(const float *preds, const int32_t *lens, const int32_t *num_pos, int B, int L, int S, int mode, float temperature,
                                uint64_t seed, int64_t q0, const float *unif, int64_t *pos_idx, int64_t *neg_idx, int32_t *nsel, void *stream) {
    using namespace ptr;
    const char *who = "ptr_irgan_sample";
    if (int rc = ig_check_shape(who, B, L, temperature)) return rc;
    if (int rc = ig_check_samples(who, S)) return rc;
    if (mode < PTR_IRGAN_POINT_D || mode > PTR_IRGAN_PAIR_G) { set_error("%s: mode %d (PTR_IRGAN_POINT_D, _PAIR_D, _PAIR_G)", who, mode); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_pointers(B, preds && num_pos, who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, pos_idx && neg_idx && nsel, who)) return rc;
    if (B == 0) return 0;
    const IgSampleArgs A{preds, lens, num_pos, B, L, S, mode, temperature, seed, q0, unif, pos_idx, neg_idx, nsel};
    const int Lp = round_up(L, 4);
    if (irgan_form(L).G == kWave)
        return launch_queries(irgan_sample_kernel<kWave>, B, kBlock / kWave, kBlock, ((size_t)(kBlock / kWave) * 2 * Lp + 8) * sizeof(float), stream, who, A, Lp);
    return launch_queries(irgan_sample_kernel<kBlock>, B, 1, kBlock, ((size_t)2 * Lp + 8) * sizeof(float), stream, who, A, Lp);
}

extern "C" int ptr_irgan_point_gen_fwd_bwd(const float *g_preds, const float *d_preds, const int32_t *lens, const int32_t *num_pos, int B, int L,
                                           float temperature, float lambda, int draws_per_pos, uint64_t seed, int64_t q0, const float *unif,
                                           float *loss_out, float *loss_q, float *valid_q, float *grad, int32_t *counts, void *stream) {
    using namespace ptr;
    const char *who = "ptr_irgan_point_gen_fwd_bwd";
    if (int rc = ig_check_shape(who, B, L, temperature)) return rc;
    if (!(lambda >= 0.0f && lambda < 1.0f)) { set_error("%s: lambda must be in [0, 1) (got %g)", who, (double)lambda); return PTR_ERR_INVALID_ARG; }
    if (draws_per_pos < 1 || draws_per_pos > PTR_IRGAN_MAX_DRAWS_PER_POS) {
        set_error("%s: draws_per_pos must be in 1 .. %d (got %d)", who, PTR_IRGAN_MAX_DRAWS_PER_POS, draws_per_pos);
        return PTR_ERR_INVALID_ARG;
    }
    if (int rc = check_pointers(B, g_preds && d_preds && num_pos, who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, loss_q && valid_q && grad, who)) return rc;
    if (B > 0) {
        const IgGenArgs A{g_preds, d_preds, lens, num_pos, B, L, temperature, lambda, draws_per_pos, seed, q0, unif, loss_q, valid_q, grad, counts};
        const int Lp = round_up(L, 4);
        int rc;
        if (irgan_form(L).G == kWave)
            rc = launch_queries(irgan_point_gen_kernel<kWave>, B, kBlock / kWave, kBlock, ((size_t)(kBlock / kWave) * 3 * Lp + 8) * sizeof(float), stream, who, A, Lp);
        else
            rc = launch_queries(irgan_point_gen_kernel<kBlock>, B, 1, kBlock, ((size_t)3 * Lp + 8) * sizeof(float), stream, who, A, Lp);
        if (rc) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}

extern "C" int ptr_irgan_sel_fwd_bwd(const float *x, const float *d_sel, const int64_t *neg_idx, const int32_t *nsel, const int32_t *lens, int B,
                                     int L, int S, int mode, float temperature, float *loss_out, float *loss_q, float *valid_q, float *grad,
                                     void *stream) {
    using namespace ptr;
    const char *who = "ptr_irgan_sel_fwd_bwd";
    if (int rc = ig_check_shape(who, B, L, temperature)) return rc;
    if (int rc = ig_check_samples(who, S)) return rc;
    if (mode < PTR_IRGAN_SEL_POINT_D || mode > PTR_IRGAN_SEL_PAIR_G_LOG) { set_error("%s: mode %d (PTR_IRGAN_SEL_*)", who, mode); return PTR_ERR_INVALID_ARG; }
    const bool gen = mode >= PTR_IRGAN_SEL_PAIR_G_SVM;
    if (int rc = check_pointers(B, x && nsel && (!gen || (d_sel && neg_idx)), who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, loss_q && valid_q && grad, who)) return rc;
    if (B > 0) {
        const IgSelArgs A{x, d_sel, neg_idx, nsel, lens, B, L, S, mode, temperature, loss_q, valid_q, grad};
        int rc;
        const int Wp = round_up(gen ? L : 2 * S, 4);
        if (irgan_sel_form(mode, L).G == kWave)
            rc = launch_queries(irgan_sel_kernel<kWave>, B, kBlock / kWave, kBlock, (size_t)(kBlock / kWave) * Wp * sizeof(float), stream, who, A, Wp);
        else
            rc = launch_queries(irgan_sel_kernel<kBlock>, B, 1, kBlock, (size_t)Wp * sizeof(float), stream, who, A, Wp);
        if (rc) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}
