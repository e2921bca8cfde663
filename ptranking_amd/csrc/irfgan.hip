// The adversarial frame's IRFGAN point and pair machines: the f-divergence generalisation of irgan.hip — sampling the documents and the
// document pairs both players train on, and the two players' losses under the eight f-divergences of the reference.
//
// Reference: ptranking/ltr_adversarial/pointwise/irfgan_point.py:179-192 (the draws), :200-220 (the losses);
//            ptranking/ltr_adversarial/pairwise/irfgan_pair.py:112-130, :141-170; ptranking/ltr_adversarial/util/pair_sampling.py:26-77
//            (the true pairs), :111-122 (the Bernoulli mask and the multinomial over it); util/f_divergence.py (activation_f, conjugate_f).
// The reference runs one query per step, holds an n x n matrix of Bradley-Terry probabilities, an n x n Bernoulli mask and a P x n weight
// matrix, and composes conjugate_f(activation_f(v)) literally in fp32.  Here a padded batch [B, L] with lens and num_pos takes one launch
// per piece, nothing of size n x n is stored, and the composition is evaluated in closed form (fg_conj, ptr_irgan.h).
//
// The pair sampler (irfgan_pair_sample_kernel), n = lens[q], P = num_pos[q], thread t owns rows t, t + G, ...:
//   true pairs   w_ij = max(0, y_i - y_j) / (log2(2 + i) log2(2 + j)), i < P, j < n.  Pass 1: every thread sums its own rows over all
//                partners, j ascending (R_i).  Pass 2: the FIRST wavefront builds the inclusive prefix C over the rows in tiles of 64 (both
//                forms run the same additions in the same order).  Draw k: x = u(0, k) C_{P-1}; the head is the inverse-CDF row of x
//                (ptr_irgan.h), the tail the first column with w > 0 whose in-row prefix (the additions of pass 1, so it ends at R_i
//                exactly) exceeds x - C_{head-1}, the last column with w > 0 when there is none.
//   fake pairs   b_ij = [u(2 + i, j) < sigmoid(s_i - s_j)], all n x n, the diagonal included.  Pass 1: every thread counts the bits of its own
//                rows by recomputing the hash.  Pass 2: an integer inclusive prefix over the row counts, M its last entry.  Draw k:
//                r = min(M - 1, floor(floor(u(1, k) 2^24) M / 2^24)) in 64-bit integers; the row is the first whose prefix exceeds r; one
//                wavefront rescans that row 64 columns at a time and finds the column by ballot prefix counts.  From the comparison
//                outcomes on everything is integer arithmetic: the draws are a function of the bits b_ij alone, whatever the form.
// Shape: a list of up to 256 documents takes one wavefront, four queries per workgroup; a longer one a workgroup of 256 threads (its four
// waves share the rows, and each takes every fourth fake draw).  LDS per query: 4 rows of round_up(L, 4) words — labels then scores,
// discounts, row sums then row counts, the prefix — + 16 words per workgroup.  No floating-point atomics, no atomics at all.  A query's bits
// depend on (its data, L, S, seed, q0 + q) alone.
#include "ptr_irgan.h"
#include "ptr_plhash.h"

namespace ptr {

// ---------------------------------------------------------------------------------------------------------------- the point sampler
struct FgPointArgs {
    const float *preds;
    const int32_t *lens, *num_pos;
    int B, L, S;
    uint64_t seed;
    int64_t q0;
    const float *unif;
    int64_t *pos_idx, *neg_idx;
    int32_t *nsel;
};

// LDS per query: K (round_up(L, 4) floats), + 8 words per workgroup
template <int G> __global__ void __launch_bounds__(kBlock) irfgan_point_sample_kernel(const FgPointArgs A, int Lp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int QPB = kBlock / G;
    const int grp = G == kWave ? threadIdx.x >> 6 : 0, t = G == kWave ? threadIdx.x & 63 : threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * QPB + grp);
    if (q >= A.B) return;                                                    // G == 64: wave-level synchronisation only below
    float *K = smem + (size_t)grp * Lp, *red = smem + (size_t)QPB * Lp;
    const int L = A.L, S = A.S;
    const int n = query_len(A.lens, q, L);
    const int P = min(max(A.num_pos[q], 0), n);
    const float *s = A.preds + (size_t)q * L;
    bool bad = false;
    for (int i = t; i < n; i += G) bad |= s[i] != s[i];
    const bool nanq = group_any<G>(bad, reinterpret_cast<int *>(red), t);
    const int V = nanq ? 0 : min(P, S);                                      // irfgan_point.py:180-182, :188-190
    int64_t *pos = A.pos_idx + (size_t)q * S, *neg = A.neg_idx + (size_t)q * S;
    for (int k = V + t; k < S; k += G) { pos[k] = 0; neg[k] = 0; }
    if (t == 0) A.nsel[q] = V;
    if (V == 0) return;
    const PlKeys qk = pl_query_keys(A.seed, A.q0 + (int64_t)q);
    const PlKeys k0 = pl_sample_keys(qk, 0u), k1 = pl_sample_keys(qk, 1u);
    const float *u0 = A.unif ? A.unif + (size_t)q * 2 * L : nullptr, *u1 = u0 ? u0 + L : nullptr;
    for (int i = t; i < P; i += G) K[i] = u0 ? u0[i] : pl_uniform(k0, (uint32_t)i);     // :183 randperm(P)[:V]
    group_sync<G>();
    take_largest<G>(K, P, V, pos, red, t);
    for (int i = t; i < n; i += G) K[i] = s[i] + pl_gumbel(u1 ? u1[i] : pl_uniform(k1, (uint32_t)i));   // :186, :192 softmax, no replacement
    group_sync<G>();
    take_largest<G>(K, n, V, neg, red, t);
}

// ---------------------------------------------------------------------------------------------------------------- the pair sampler
struct FgPairArgs {
    const float *preds, *labels;
    const int32_t *lens, *num_pos;
    int B, L, S;
    uint64_t seed;
    int64_t q0;
    const float *unif_draw, *unif_bern;
    int64_t *true_head, *true_tail, *fake_head, *fake_tail;
    int32_t *nsel, *bern_count;
};

// one term of the true pairs' weight matrix; passes 1 and the tail search evaluate exactly this expression
__device__ __forceinline__ float fg_pair_weight(float yi, float di, float yj, float dj) { return (fmaxf(0.0f, yi - yj) * dj) * di; }

template <int G> __global__ void __launch_bounds__(kBlock) irfgan_pair_sample_kernel(const FgPairArgs A, int Lp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int QPB = kBlock / G;
    const int grp = G == kWave ? threadIdx.x >> 6 : 0, t = G == kWave ? threadIdx.x & 63 : threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * QPB + grp);
    if (q >= A.B) return;                                                    // every early return below is uniform over the group
    float *Y = smem + (size_t)grp * 4 * Lp, *D = Y + Lp, *R = D + Lp, *C = R + Lp, *red = smem + (size_t)QPB * 4 * Lp;
    float *Sc = Y;                                                           // the scores take the labels' row once the true pairs are drawn
    int *CNT = reinterpret_cast<int *>(R);                                   // and the row counts the row sums'
    const int L = A.L, S = A.S, lane = t & 63, wave = t >> 6;
    const int n = query_len(A.lens, q, L);
    const int P = min(max(A.num_pos[q], 0), n);
    const float *s = A.preds + (size_t)q * L, *y = A.labels + (size_t)q * L;
    int64_t *th = A.true_head + (size_t)q * S, *tt = A.true_tail + (size_t)q * S, *fh = A.fake_head + (size_t)q * S, *ft = A.fake_tail + (size_t)q * S;
    auto nothing = [&]() {                                                   // nsel = 0: no pair is named, no bit counted
        for (int k = t; k < S; k += G) { th[k] = 0; tt[k] = 0; fh[k] = 0; ft[k] = 0; }
        if (t == 0) { A.nsel[q] = 0; if (A.bern_count) A.bern_count[q] = 0; }
    };
    bool bad = false;
    for (int i = t; i < n; i += G) bad |= s[i] != s[i];
    const bool nanq = group_any<G>(bad, reinterpret_cast<int *>(red), t);
    if (n == 0 || nanq) { nothing(); return; }                              // irfgan_pair.py:120-123
    for (int i = t; i < n; i += G) { Y[i] = y[i]; D[i] = 1.0f / log2f((float)(i + 2)); }
    group_sync<G>();
    if (Y[0] == Y[n - 1]) { nothing(); return; }                            // :109 num_unique_labels < 2 on a presorted list
    // ---- true pairs (pair_sampling.py:26-77): row sums, their prefix, S inverse-CDF draws
    for (int i = t; i < P; i += G) {
        const float yi = Y[i], di = D[i];
        float acc = 0.0f;
        for (int j = 0; j < n; ++j) acc += fg_pair_weight(yi, di, Y[j], D[j]);
        R[i] = acc;
    }
    group_sync<G>();
    if (t < kWave) prefix_into<kWave>(C, P, red, t, [&](int i) { return R[i]; });   // one order of additions in both forms
    group_sync<G>();
    const float W = P > 0 ? C[P - 1] : 0.0f;
    if (!(W > 0.0f)) { nothing(); return; }
    const PlKeys qk = pl_query_keys(A.seed, A.q0 + (int64_t)q);
    const float *ud = A.unif_draw ? A.unif_draw + (size_t)q * 2 * S : nullptr;
    int head = 0, tail = 0;
    if (t < S) {
        const float u = ud ? ud[t] : pl_uniform(pl_sample_keys(qk, 0u), (uint32_t)t);
        const float x = u * W;
        head = inverse_cdf(C, P, x, [&](int i) { return R[i] == 0.0f; });
        const float rem = x - (head > 0 ? C[head - 1] : 0.0f);
        const float yi = Y[head], di = D[head];
        float acc = 0.0f;
        int last = 0;
        tail = -1;
        for (int j = 0; j < n; ++j) {
            const float w = fg_pair_weight(yi, di, Y[j], D[j]);
            if (w > 0.0f) {
                acc += w;
                last = j;
                if (acc > rem) { tail = j; break; }
            }
        }
        if (tail < 0) tail = last;
    }
    group_sync<G>();                                                         // the labels and the row sums are spent
    // ---- fake pairs (pair_sampling.py:111-122 on irfgan_pair.py:127-130): the bits of every row, counted, never stored
    for (int i = t; i < n; i += G) Sc[i] = s[i];
    group_sync<G>();
    const float *ubq = A.unif_bern ? A.unif_bern + (size_t)q * L * L : nullptr;
    auto bit = [&](float si, const PlKeys &rk, const float *ub, int j) {
        const float u = ub ? ub[j] : pl_uniform(rk, (uint32_t)j);
        return u < ig_sigmoid(si - Sc[j]);
    };
    for (int i = t; i < n; i += G) {
        const float si = Sc[i];
        const PlKeys rk = pl_sample_keys(qk, 2u + (uint32_t)i);
        const float *ub = ubq ? ubq + (size_t)i * L : nullptr;
        int c = 0;
        for (int j = 0; j < n; ++j) c += bit(si, rk, ub, j) ? 1 : 0;
        CNT[i] = c;
    }
    group_sync<G>();
    if (t < kWave) {                                                         // integer inclusive prefix over the rows, exact in any order
        int carry = 0;
        for (int base = 0; base < n; base += kWave) {
            const int i = base + t;
            int v = i < n ? CNT[i] : 0;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const int o = __shfl_up(v, d, 64);
                if (t >= d) v += o;
            }
            if (i < n) CNT[i] = carry + v;
            carry += __shfl(v, 63, 64);
        }
    }
    group_sync<G>();
    const int M = CNT[n - 1];
    if (M == 0) { nothing(); return; }                                      // torch.multinomial would raise on an all-zero mask
    if (t < S) { th[t] = head; tt[t] = tail; }
    if (t == 0) { A.nsel[q] = S; if (A.bern_count) A.bern_count[q] = M; }
    const PlKeys k1 = pl_sample_keys(qk, 1u);
    for (int k = wave; k < S; k += G / kWave) {                              // one wavefront per draw; nothing below differs between its lanes
        const float u = ud ? ud[S + k] : pl_uniform(k1, (uint32_t)k);
        const uint64_t k24 = (uint64_t)(fminf(fmaxf(u, 0.0f), 1.0f) * 16777216.0f);
        const int r = (int)min((uint64_t)(M - 1), (k24 * (uint64_t)M) >> 24);
        int lo = 0, hi = n - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (r < CNT[mid]) hi = mid; else lo = mid + 1;
        }
        const int row = lo;
        int rem = r - (row > 0 ? CNT[row - 1] : 0);
        const float si = Sc[row];
        const PlKeys rk = pl_sample_keys(qk, 2u + (uint32_t)row);
        const float *ub = ubq ? ubq + (size_t)row * L : nullptr;
        int col = 0;
        for (int base = 0; base < n; base += kWave) {
            const int j = base + lane;
            const bool b = j < n && bit(si, rk, ub, j);
            const uint64_t mask = __ballot(b);
            const int c = __popcll(mask);
            if (rem < c) {
                const int before = __popcll(mask & ((1ull << lane) - 1ull));
                const uint64_t hit = __ballot(b && before == rem);
                col = base + __ffsll((unsigned long long)hit) - 1;
                break;
            }
            rem -= c;
        }
        if (lane == 0) { fh[k] = row; ft[k] = col; }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the losses
// fg_act (a(v) = activation_f(v)) and fg_conj (c(v) = conjugate_f(activation_f(v)) in closed form) live in ptr_irgan.h: adlist.hip shares them
struct FgLossArgs {
    const float *x, *d_fake;
    const int64_t *idx_a, *idx_b;
    const int32_t *nsel, *lens;
    int B, L, S, mode, f_div;
    float *loss_q, *valid_q, *grad;
};

// One group per query; the first wavefront holds the V <= 64 samples, one per lane.  The discriminator's modes put the gradient row together
// in LDS (Wq words per query) and store it coalesced; the generator's modes stage (c_k or g_k, the two indices) in 3 x 64 words, and every
// document's thread walks the V samples in k order and sums its own shares: no atomics, a fixed order.
template <int G> __global__ void __launch_bounds__(kBlock) irfgan_loss_kernel(const FgLossArgs A, int Wq) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int QPB = kBlock / G;
    const int grp = G == kWave ? threadIdx.x >> 6 : 0, t = G == kWave ? threadIdx.x & 63 : threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(blockIdx.x * QPB + grp);
    if (q >= A.B) return;
    const int S = A.S, V = min(max(A.nsel[q], 0), S), f = A.f_div;
    const float invV = 1.0f / (float)max(V, 1);
    float *R = smem + (size_t)grp * Wq, *red = smem + (size_t)QPB * Wq;
    if (A.mode < PTR_IRFGAN_POINT_G) {                                       // the discriminator's modes: G == 64
        const bool pair = A.mode == PTR_IRFGAN_PAIR_D;
        const int W = (pair ? 4 : 2) * S;
        const float *x = A.x + (size_t)q * W;
        float *g = A.grad + (size_t)q * W;
        for (int i = t; i < W; i += G) R[i] = 0.0f;
        group_sync<G>();
        float term = 0.0f;
        if (t < V) {
            float a, da, c, dc;
            if (pair) {                                                      // irfgan_pair.py:143-150
                fg_act(f, x[t] - x[V + t], a, da);
                fg_conj(f, x[2 * V + t] - x[3 * V + t], c, dc);
                R[t] = -da * invV;
                R[V + t] = da * invV;
                R[2 * V + t] = dc * invV;
                R[3 * V + t] = -dc * invV;
            } else {                                                         // irfgan_point.py:202-205
                fg_act(f, x[t], a, da);
                fg_conj(f, x[V + t], c, dc);
                R[t] = -da * invV;
                R[V + t] = dc * invV;
            }
            term = (c - a) * invV;
        }
        term = wave_sum(term);
        if (t == 0) { A.loss_q[q] = term; A.valid_q[q] = V > 0 ? 1.0f : 0.0f; }
        group_sync<G>();
        for (int i = t; i < W; i += G) g[i] = R[i];
        return;
    }
    const int L = A.L, n = query_len(A.lens, q, L);
    const float *x = A.x + (size_t)q * L;
    float *g = A.grad + (size_t)q * L;
    if (V == 0) {
        for (int i = t; i < L; i += G) g[i] = 0.0f;
        if (t == 0) { A.loss_q[q] = 0.0f; A.valid_q[q] = 0.0f; }
        return;
    }
    float *CK = R;
    int *IA = reinterpret_cast<int *>(R + kWave), *IB = IA + kWave;
    const bool pair = A.mode == PTR_IRFGAN_PAIR_G;
    auto named = [&](int64_t d) { return d >= 0 && d < (int64_t)n ? (int)d : -1; };   // an index outside the list names nothing
    float m = 0.0f, logZ = 0.0f, Z = 1.0f;
    if (!pair) {                                                             // the log-softmax over the n real documents
        m = -INFINITY;
        for (int i = t; i < n; i += G) m = fmaxf(m, x[i]);
        m = group_max<G>(m, red, t);
        float zs = 0.0f;
        for (int i = t; i < n; i += G) zs += expf(x[i] - m);
        Z = group_sum<G>(zs, red, t);
        logZ = logf(Z);
    }
    if (t < kWave) {
        float term = 0.0f, ck = 0.0f;
        int ia = -1, ib = -1;
        if (t < V) {
            float c, dc;
            if (pair) {                                                      // irfgan_pair.py:157-166
                const float *d = A.d_fake + (size_t)q * 2 * S;
                fg_conj(f, d[t] - d[V + t], c, dc);
                ia = named(A.idx_a[(size_t)q * S + t]);
                ib = named(A.idx_b[(size_t)q * S + t]);
                if (ia < 0 || ib < 0) { ia = -1; ib = -1; }
                else {
                    const float z = x[ia] - x[ib];
                    term = -ig_logsigmoid(z) * c * invV;
                    ck = -ig_sigmoid(-z) * c * invV;                         // d loss / d z_k: + at the head, - at the tail
                }
            } else {                                                         // irfgan_point.py:213-216
                fg_conj(f, A.d_fake[(size_t)q * S + t], c, dc);
                ia = named(A.idx_a[(size_t)q * S + t]);
                if (ia >= 0) {
                    ck = c;
                    term = -(((x[ia] - m) - logZ) * c) * invV;
                }
            }
        }
        CK[t] = ck; IA[t] = ia; IB[t] = ib;
        term = wave_sum(term);
        if (t == 0) { A.loss_q[q] = term; A.valid_q[q] = 1.0f; }
    }
    group_sync<G>();
    float csum = 0.0f;
    if (!pair) for (int k = 0; k < V; ++k) csum += IA[k] >= 0 ? CK[k] : 0.0f;
    for (int i = t; i < L; i += G) {
        float acc = 0.0f;
        if (i < n) {
            if (pair) {
                for (int k = 0; k < V; ++k) {
                    if (IA[k] == i) acc += CK[k];
                    if (IB[k] == i) acc -= CK[k];
                }
            } else {
                for (int k = 0; k < V; ++k) acc += IA[k] == i ? CK[k] : 0.0f;
                acc = -invV * (acc - (expf(x[i] - m) / Z) * csum);
            }
        }
        g[i] = acc;
    }
}

IrganForm irfgan_loss_form(int mode, int L) { return mode >= PTR_IRFGAN_POINT_G ? irgan_form(L) : IrganForm{kWave, kBlock / kWave}; }

static int fg_check(const char *who, int B, int L, int S) {
    if (int rc = ig_check_shape(who, B, L, 1.0f)) return rc;
    return ig_check_samples(who, S);
}

}  // namespace ptr

extern "C" int ptr_irfgan_point_sample(const float *preds, const int32_t *lens, const int32_t *num_pos, int B, int L, int S, uint64_t seed, int64_t q0,
                                       const float *unif, int64_t *pos_idx, int64_t *neg_idx, int32_t *nsel, void *stream) {
    using namespace ptr;
    const char *who = "ptr_irfgan_point_sample";
    if (int rc = fg_check(who, B, L, S)) return rc;
    if (int rc = check_pointers(B, preds && num_pos, who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, pos_idx && neg_idx && nsel, who)) return rc;
    if (B == 0) return 0;
    const FgPointArgs A{preds, lens, num_pos, B, L, S, seed, q0, unif, pos_idx, neg_idx, nsel};
    const int Lp = round_up(L, 4);
    if (irgan_form(L).G == kWave)
        return launch_queries(irfgan_point_sample_kernel<kWave>, B, kBlock / kWave, kBlock, ((size_t)(kBlock / kWave) * Lp + 8) * sizeof(float), stream, who, A, Lp);
    return launch_queries(irfgan_point_sample_kernel<kBlock>, B, 1, kBlock, ((size_t)Lp + 8) * sizeof(float), stream, who, A, Lp);
}

extern "C" int ptr_irfgan_pair_sample(const float *preds, const float *labels, const int32_t *lens, const int32_t *num_pos, int B, int L, int S,
                                      uint64_t seed, int64_t q0, const float *unif_draw, const float *unif_bern, int64_t *true_head,
                                      int64_t *true_tail, int64_t *fake_head, int64_t *fake_tail, int32_t *nsel, int32_t *bern_count, void *stream) {
    using namespace ptr;
    const char *who = "ptr_irfgan_pair_sample";
    if (int rc = fg_check(who, B, L, S)) return rc;
    if (int rc = check_pointers(B, preds && labels && num_pos, who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, true_head && true_tail && fake_head && fake_tail && nsel, who)) return rc;
    if (B == 0) return 0;
    const FgPairArgs A{preds, labels, lens, num_pos, B, L, S, seed, q0, unif_draw, unif_bern, true_head, true_tail, fake_head, fake_tail, nsel, bern_count};
    const int Lp = round_up(L, 4);
    if (irgan_form(L).G == kWave)
        return launch_queries(irfgan_pair_sample_kernel<kWave>, B, kBlock / kWave, kBlock, ((size_t)(kBlock / kWave) * 4 * Lp + 16) * sizeof(float), stream, who, A, Lp);
    return launch_queries(irfgan_pair_sample_kernel<kBlock>, B, 1, kBlock, ((size_t)4 * Lp + 16) * sizeof(float), stream, who, A, Lp);
}

extern "C" int ptr_irfgan_fwd_bwd(const float *x, const float *d_fake, const int64_t *idx_a, const int64_t *idx_b, const int32_t *nsel,
                                  const int32_t *lens, int B, int L, int S, int mode, int f_div, float *loss_out, float *loss_q, float *valid_q,
                                  float *grad, void *stream) {
    using namespace ptr;
    const char *who = "ptr_irfgan_fwd_bwd";
    if (int rc = fg_check(who, B, L, S)) return rc;
    if (mode < PTR_IRFGAN_POINT_D || mode > PTR_IRFGAN_PAIR_G) { set_error("%s: mode %d (PTR_IRFGAN_*)", who, mode); return PTR_ERR_INVALID_ARG; }
    if (f_div < PTR_FDIV_TVAR || f_div > PTR_FDIV_GAN) { set_error("%s: f_div %d (PTR_FDIV_*)", who, f_div); return PTR_ERR_INVALID_ARG; }
    const bool gen = mode >= PTR_IRFGAN_POINT_G;
    if (int rc = check_pointers(B, x && nsel && (!gen || (d_fake && idx_a)) && (mode != PTR_IRFGAN_PAIR_G || idx_b), who, "NULL input pointer")) return rc;
    if (int rc = check_pointers(B, loss_q && valid_q && grad, who)) return rc;
    if (B > 0) {
        const FgLossArgs A{x, d_fake, idx_a, idx_b, nsel, lens, B, L, S, mode, f_div, loss_q, valid_q, grad};
        const int Wq = gen ? 3 * kWave : round_up((mode == PTR_IRFGAN_PAIR_D ? 4 : 2) * S, 4);
        int rc;
        if (irfgan_loss_form(mode, L).G == kWave)
            rc = launch_queries(irfgan_loss_kernel<kWave>, B, kBlock / kWave, kBlock, ((size_t)(kBlock / kWave) * Wq + 8) * sizeof(float), stream, who, A, Wq);
        else
            rc = launch_queries(irfgan_loss_kernel<kBlock>, B, 1, kBlock, ((size_t)Wq + 8) * sizeof(float), stream, who, A, Wq);
        if (rc) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}
