// NeuralNDCG: nDCG on the NeuralSort relaxation of the sort operator, made doubly stochastic by Sinkhorn scaling (the rule is this project's
// own, modelled on allRank's neuralNDCG; include/ptranking_amd.h states it) — one workgroup per query, the softmax, every scaling iteration,
// the objective and the exact backward through all of them inside one launch.
//
// Scale-vector form.  With a_ij = (c_i s_j - B_j) / tau, c_i = n - 1 - 2 i, B_j = sum_k |s_j - s_k| and m_i = max_j a_ij,
//   K_ij = exp(a_ij - m_i)                                   is FIXED across the iterations, and every iterate is
//   P_t  = diag(u_t) K diag(v_t),     u_0 = 1 / (K 1)  (the softmax),  v_0 = 1,
//   v_t  = v_{t-1} / max(v_{t-1} * (K^T u_{t-1}), eps),      u_t = u_{t-1} / max(u_{t-1} * (K v_t), eps),      eps = 1e-10.
// P is never formed: a half-iteration is one matvec over K (a column pass: thread t owns column j and walks the rows; or a row pass: thread t
// owns row i and walks the columns) and a division.  loss_q = sum_i w_i u_T,i (K (v_T * g))_i with w_i = -[i < k] d_i / idcg.
//
// Two forms behind one template (as wass_cost does it): K resident in LDS in fp32 (row-major with an ODD leading dimension, so that both the
// column pass — lanes along a row — and the row pass — lanes along a column — touch 64 distinct banks) while L (L | 1) floats and the
// vectors fit the 160 KiB of a compute unit; above that, up to kNeuralMaxLen, K_ij is recomputed from (s_j, B_j) and (c_i, m_i) in every pass.
//
// Exponent in fp64.  |a_ij| reaches 1e5 and more (scores of scale 30, tau = 0.1, 65 documents) while K only matters where a_ij - m_i is
// small: in fp32 the cancellation would leave an absolute error of 1e-2 in the exponent.  s_j / tau, B_j / tau and m_i are therefore kept as
// doubles (in base-2 units), the exponent is one v_fma_f64 and one v_add_f64, and only the difference is rounded to fp32 for v_exp_f32: the
// row maximum's own entry is exactly 1.  The resident form pays this once per entry, the recomputed form in every pass.
//
// Backward without an L x L accumulator.  The adjoint of K is a sum of 2 T + 2 rank-one terms a b^T (the objective, every half-iteration,
// the softmax), and the gradient needs of G = K o dK only M_j = sum_i G_ij and W_j = sum_i c_i G_ij: for a term a b^T these are b_j (K^T a)_j and
// b_j (K^T (c a))_j.  The reverse sweep over t = T .. 1 needs the history u_t, v_t (2 T + 1 vectors: in LDS where they fit, else in the
// caller's workspace; the forward is fp32, the sweep fp64) and, per iteration, ONE column pass with four accumulators (alpha, c alpha, u_{t-1}, c u_{t-1}) and ONE row pass (beta):
//   alpha = -ubar u_t^2              (u_t = 1 / (K v_t) where the sum is not clamped: d u_t / d u_{t-1} = 0 exactly)
//   vbar += K^T alpha;   M += v_t (K^T alpha) + beta (K^T u_{t-1});   W likewise with c alpha, c u_{t-1}
//   beta  = -vbar v_t^2;             ubar' = K beta;   vbar' = 0
// (a clamped sum passes ubar / eps or vbar / eps straight through and has alpha or beta = 0; the history marks it by its sign).  Then
//   d loss / d s_l = W_l / tau + sum_j (Bbar_l + Bbar_j) sign(s_l - s_j),     Bbar = -M / tau     (sign(0) = 0: ties are legal).
// DESIGN.md derives this.
//
// Every reduction has a fixed order and there are no atomics: the outputs of a query depend on (its documents, L, the parameters) alone.
// The passes are matvecs and row / column sums over a matrix whose entries are exponentials: nothing here is a matrix product, so there is
// no MFMA.
#include <math.h>

#include "ptr_device.h"

namespace ptr {

namespace {

constexpr double kLog2eD = 1.4426950408889634074;
constexpr float kSinkEps = 1e-10f;
constexpr int kNeuralVecFloats = 29;                 // per padded document: SB (4) MD (2) UB VB CA Mv Wv (2 each) R4 (8): doubles; S G Wt U V
constexpr int kNeuralRedFloats = 16;

template <bool RES> struct KMat {
    const float *Kl;                                 // RES: K[i * ld + j]
    int ld;
    const double2 *SB;                               // (s_j, B_j) log2(e) / tau
    const double *MD;                                // m_i in the same units
    int n;
};

template <bool RES> __device__ __forceinline__ float k_entry(const KMat<RES> &k, int i, int j, double ci, double2 sb, double md) {
    if constexpr (RES) return k.Kl[(size_t)i * k.ld + j];
    else return fast_exp2((float)(fma(ci, sb.x, -sb.y) - md));
}

// out[a] = sum_i K_ij x_a[i] for column j; x_a[i] = x[i] (NA == 1) or x[4 i + a].  Four interleaved partial sums, fixed order.
template <bool RES, int NA, class T>
__device__ __forceinline__ void col_dot(const KMat<RES> &k, int j, const T *x, T (&out)[NA]) {
    const int n = k.n;
    const double2 sb = k.SB[j];
    T acc[NA][4];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[a][u] = T(0);
    auto step = [&](int i, int u) {
        const T kv = (T)k_entry<RES>(k, i, j, (double)(n - 1 - 2 * i), sb, RES ? 0.0 : k.MD[i]);
        if constexpr (NA == 1) {
            acc[0][u] = fma(kv, x[i], acc[0][u]);
        } else {
#pragma unroll
            for (int a = 0; a < NA; ++a) acc[a][u] = fma(kv, x[4 * i + a], acc[a][u]);
        }
    };
    int i = 0;
    for (; i + 4 <= n; i += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) step(i + u, u);
    }
    for (int u = 0; i < n; ++i, ++u) step(i, u);
#pragma unroll
    for (int a = 0; a < NA; ++a) out[a] = (acc[a][0] + acc[a][1]) + (acc[a][2] + acc[a][3]);
}

// sum_j K_ij y[j] for row i.
template <bool RES, class T>
__device__ __forceinline__ T row_dot(const KMat<RES> &k, int i, const T *y) {
    const int n = k.n;
    const double ci = (double)(n - 1 - 2 * i), md = k.MD[i];
    T acc[4] = {T(0), T(0), T(0), T(0)};
    auto step = [&](int j, int u) {
        double2 sb = {0.0, 0.0};
        if constexpr (!RES) sb = k.SB[j];
        acc[u] = fma((T)k_entry<RES>(k, i, j, ci, sb, md), y[j], acc[u]);
    };
    int j = 0;
    for (; j + 4 <= n; j += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) step(j + u, u);
    }
    for (int u = 0; j < n; ++j, ++u) step(j, u);
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

template <int G> __device__ __forceinline__ double group_sum_f64(double v, double *red, int t) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if constexpr (G == kWave) {
        return v;
    } else {
        __syncthreads();
        if ((t & 63) == 0) red[t >> 6] = v;
        __syncthreads();
        double r = red[0];
#pragma unroll
        for (int w = 1; w < G / kWave; ++w) r += red[w];
        return r;
    }
}

// One workgroup of G threads per query.  LDS (floats, Lp = round_up(L, 4)): SB[2 Lp] double2 | MD UB VB CA Mv Wv [Lp] double each | R4[4 Lp] double | S G Wt U V
// [Lp] float each | red[16] | RES: K[L (L | 1)] | hist_lds: H[(2 T + 1) Lp].  History rows: u_0 .. u_T, then v_1 .. v_T; a negative
// entry marks a half-iteration whose sum was clamped.
template <bool RES, int G>
__global__ void __launch_bounds__(G)
neuralndcg_kernel(const float *__restrict__ preds, const float *__restrict__ labels, const int32_t *__restrict__ lens, int L, int Lp, float tau,
                  int T, int top_k, int powered, int hist_lds, float *__restrict__ ws, float *__restrict__ loss_q, float *__restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    double2 *SB = reinterpret_cast<double2 *>(smem);
    double *MD = reinterpret_cast<double *>(smem + 4 * (size_t)Lp);
    double *UB = MD + Lp, *VB = UB + Lp, *CA = VB + Lp, *Mv = CA + Lp, *Wv = Mv + Lp, *R4 = Wv + Lp;
    float *S = smem + 24 * (size_t)Lp, *Gn = S + Lp, *Wt = Gn + Lp, *U = Wt + Lp, *V = U + Lp;
    float *red = V + Lp;
    double *redd = reinterpret_cast<double *>(red + 8);
    float *Kl = red + kNeuralRedFloats;
    const int ld = L | 1;
    const int q = blockIdx.x, t = threadIdx.x;
    const int n = query_len(lens, q, L);
    float *H = hist_lds ? Kl + (RES ? (size_t)L * ld : 0) : ws + (size_t)q * (2 * (size_t)T + 1) * Lp;
    float *HU = H, *HV = H + (size_t)(T + 1) * Lp - Lp;          // HV + t * Lp = v_t, t = 1 .. T
    const float *ps = preds + (size_t)q * L, *ys = labels + (size_t)q * L;
    float *g = grad + (size_t)q * L;
    auto zero_out = [&]() {
        for (int i = t; i < L; i += G) g[i] = 0.0f;
        if (t == 0) loss_q[q] = 0.0f;
    };
    if (n == 0) { zero_out(); return; }

    // ---- gains, scores, the ideal DCG at the cut-off (labels ranked by counting: gain descending, index on ties)
    for (int j = t; j < n; j += G) {
        const float y = ys[j];
        S[j] = ps[j];
        Gn[j] = powered ? exp2f(y) - 1.0f : y;
    }
    __syncthreads();
    const int kk = top_k > 0 && top_k < n ? top_k : n;
    const double kappa = kLog2eD / (double)tau;
    double part = 0.0;
    for (int j = t; j < n; j += G) {
        const float gj = Gn[j], sj = S[j];
        int rank = 0;
        double bj = 0.0;
        for (int l = 0; l < n; ++l) {
            const float gl = Gn[l];
            rank += (gl > gj) || (gl == gj && l < j);
            bj += fabs((double)sj - (double)S[l]);
        }
        if (rank < kk) part += (double)gj / log2((double)(rank + 2));
        SB[j] = double2{(double)sj * kappa, bj * kappa};
    }
    const double idcg = group_sum_f64<G>(part, redd, t);
    if (!(idcg > 0.0)) { zero_out(); return; }                  // uniform over the workgroup
    __syncthreads();

    // ---- m_i, the weights, K (resident form), the softmax as u_0
    KMat<RES> km{Kl, ld, SB, MD, n};
    for (int i = t; i < n; i += G) {
        const double ci = (double)(n - 1 - 2 * i);
        double mx = -INFINITY;
        for (int j = 0; j < n; ++j) { const double2 sb = SB[j]; mx = fmax(mx, fma(ci, sb.x, -sb.y)); }
        MD[i] = mx;
        if constexpr (RES) {
            for (int j = 0; j < n; ++j) { const double2 sb = SB[j]; Kl[(size_t)i * ld + j] = fast_exp2((float)(fma(ci, sb.x, -sb.y) - mx)); }
        }
        Wt[i] = i < kk ? (float)(-1.0 / (log2((double)(i + 2)) * idcg)) : 0.0f;
        V[i] = 1.0f;
    }
    __syncthreads();
    for (int i = t; i < n; i += G) {
        const float u = 1.0f / row_dot<RES, float>(km, i, V);           // the row sum is >= 1: the maximum's own entry
        U[i] = u;
        HU[i] = u;
    }
    __syncthreads();

    // ---- T scaling iterations
    for (int it = 1; it <= T; ++it) {
        for (int j = t; j < n; j += G) {
            float qj[1];
            col_dot<RES, 1, float>(km, j, U, qj);
            const float v0 = V[j], x = v0 * qj[0];
            const bool clamp = !(x >= kSinkEps);
            const float v = v0 / (clamp ? kSinkEps : x);
            V[j] = v;
            HV[(size_t)it * Lp + j] = clamp ? -v : v;
        }
        __syncthreads();
        for (int i = t; i < n; i += G) {
            const float u0 = U[i], y = u0 * row_dot<RES, float>(km, i, V);
            const bool clamp = !(y >= kSinkEps);
            const float u = u0 / (clamp ? kSinkEps : y);
            HU[(size_t)it * Lp + i] = clamp ? -u : u;
            U[i] = u;                                            // (the row pass reads V alone)
        }
        __syncthreads();
    }

    // ---- objective: loss = sum_i u_i ubar_i, ubar_i = w_i (K (v g))_i, vbar_j = g_j (K^T (w u))_j, and its rank-one term (w u)(v g)^T.
    // From here on every sum is fp64: the adjoint of K is a sum of large rank-one terms that cancel (the softmax removes each row's mean, a
    // scaling step each row's or column's), and in fp32 that cancellation costs 50 times the error of the forward (DESIGN.md has the figures).
    for (int j = t; j < n; j += G) CA[j] = (double)V[j] * (double)Gn[j];
    __syncthreads();
    double lpart = 0.0;
    for (int i = t; i < n; i += G) {
        const double ub = (double)Wt[i] * row_dot<RES, double>(km, i, CA);
        const double a = (double)Wt[i] * (double)U[i], ci = (double)(n - 1 - 2 * i);
        UB[i] = ub;
        lpart = fma((double)U[i], ub, lpart);
        R4[4 * i] = a; R4[4 * i + 1] = ci * a; R4[4 * i + 2] = 0.0; R4[4 * i + 3] = 0.0;
    }
    const float loss = (float)group_sum_f64<G>(lpart, redd, t);
    __syncthreads();
    for (int j = t; j < n; j += G) {
        double A[2];
        col_dot<RES, 2, double>(km, j, R4, A);
        VB[j] = (double)Gn[j] * A[0];
        Mv[j] = CA[j] * A[0];
        Wv[j] = CA[j] * A[1];
    }
    __syncthreads();

    // ---- reverse sweep
    const double inv_eps = 1.0 / (double)kSinkEps;
    for (int it = T; it >= 1; --it) {
        for (int i = t; i < n; i += G) {
            const double hu = (double)HU[(size_t)it * Lp + i], up = fabs((double)HU[(size_t)(it - 1) * Lp + i]);
            const double ub = UB[i], ci = (double)(n - 1 - 2 * i);
            const bool clamp = hu < 0.0;
            const double al = clamp ? 0.0 : -(ub * hu) * hu;
            UB[i] = clamp ? ub * inv_eps : 0.0;
            R4[4 * i] = al; R4[4 * i + 1] = ci * al; R4[4 * i + 2] = up; R4[4 * i + 3] = ci * up;
        }
        __syncthreads();
        for (int j = t; j < n; j += G) {
            double A[4];
            col_dot<RES, 4, double>(km, j, R4, A);
            const double hv = (double)HV[(size_t)it * Lp + j], vt = fabs(hv);
            const double vb = VB[j] + A[0];
            const bool clamp = hv < 0.0;
            const double be = clamp ? 0.0 : -(vb * vt) * vt;
            Mv[j] = fma(be, A[2], fma(vt, A[0], Mv[j]));
            Wv[j] = fma(be, A[3], fma(vt, A[1], Wv[j]));
            CA[j] = be;
            VB[j] = clamp ? vb * inv_eps : 0.0;
        }
        __syncthreads();
        for (int i = t; i < n; i += G) UB[i] += row_dot<RES, double>(km, i, CA);
        __syncthreads();
    }
    // the softmax: u_0 = 1 / (K 1)
    for (int i = t; i < n; i += G) {
        const double u0 = (double)HU[i], rb = -(UB[i] * u0) * u0;
        R4[4 * i] = rb; R4[4 * i + 1] = (double)(n - 1 - 2 * i) * rb; R4[4 * i + 2] = 0.0; R4[4 * i + 3] = 0.0;
    }
    __syncthreads();
    const double inv_tau = 1.0 / (double)tau;
    for (int j = t; j < n; j += G) {
        double A[2];
        col_dot<RES, 2, double>(km, j, R4, A);
        Mv[j] = -(Mv[j] + A[0]) * inv_tau;                       // Bbar_j
        Wv[j] = (Wv[j] + A[1]) * inv_tau;
    }
    __syncthreads();
    for (int l = t; l < L; l += G) {
        float gl = 0.0f;
        if (l < n) {
            const float sl = S[l];
            const double bl = Mv[l];
            double acc[2] = {0.0, 0.0};
            for (int j = 0; j < n; ++j) {
                const float sj = S[j];
                const double sg = (double)((sl > sj) - (sl < sj));
                acc[j & 1] = fma(sg, bl + Mv[j], acc[j & 1]);
            }
            gl = (float)(Wv[l] + (acc[0] + acc[1]));
        }
        g[l] = gl;
    }
    if (t == 0) loss_q[q] = loss;
}

}  // namespace

// resident: K in LDS; G: threads per workgroup; hist_lds: the history in LDS (else in the workspace); lds_bytes per query (= per workgroup);
// ws_bytes per query (0 when the history is in LDS); cutover: the longest list of the resident form.
NeuralForm neuralndcg_form(int L, int iters) {
    auto fixed = [](int l) { return (size_t)kNeuralVecFloats * round_up(l, 4) + kNeuralRedFloats; };
    auto res_bytes = [&](int l) { return (fixed(l) + (size_t)l * (l | 1)) * sizeof(float); };
    static const int cutover = [&] {
        int c = 1;
        while (c < kNeuralMaxLen && res_bytes(c + 1) <= kNeuralLdsBytes) ++c;
        return c;
    }();
    NeuralForm f;
    f.resident = L <= cutover;
    f.G = !f.resident || L > 128 ? 256 : L > 64 ? 128 : 64;
    const size_t base = f.resident ? res_bytes(L) : fixed(L) * sizeof(float);
    const size_t hist = (2 * (size_t)iters + 1) * round_up(L, 4) * sizeof(float);
    // the history stays in LDS only where it costs no resident workgroup of the compute unit (counted up to 8): its traffic is O(n) per
    // pass against the O(n^2) of K, while a workgroup more hides the latency of the LDS walks
    auto per_cu = [](size_t bytes) { return (int)(kNeuralLdsBytes / bytes < 8 ? kNeuralLdsBytes / bytes : 8); };
    f.hist_lds = base + hist <= kNeuralLdsBytes && per_cu(base + hist) == per_cu(base);
    f.lds_bytes = (int)(base + (f.hist_lds ? hist : 0));
    f.ws_bytes = f.hist_lds ? 0 : (int)hist;
    f.cutover = cutover;
    return f;
}

}  // namespace ptr

extern "C" int ptr_neuralndcg_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, float tau, int iters, int k,
                                      int powered, float *loss_out, float *loss_q, float *grad, float *ws, void *stream) {
    using namespace ptr;
    const char *who = "ptr_neuralndcg_fwd_bwd";
    if (L > kNeuralMaxLen) { set_error("%s: list length %d exceeds the supported maximum %d", who, L, kNeuralMaxLen); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_loss_args(preds, labels, B, L, loss_q && grad, who)) return rc;
    if (!(tau > 0.0f) || !(tau < INFINITY)) { set_error("%s: tau must be a finite number > 0 (got %g)", who, (double)tau); return PTR_ERR_INVALID_ARG; }
    if (iters < 0 || iters > kNeuralMaxIters) { set_error("%s: iters must be in [0, %d] (got %d)", who, kNeuralMaxIters, iters); return PTR_ERR_INVALID_ARG; }
    if (B > 0) {
        const NeuralForm f = neuralndcg_form(L, iters);
        if (!f.hist_lds && !ws) { set_error("%s: L=%d iters=%d needs a workspace of %d bytes per query", who, L, iters, f.ws_bytes); return PTR_ERR_INVALID_ARG; }
        auto go = [&](auto kern) -> int {
            return launch_queries(kern, B, 1, f.G, (size_t)f.lds_bytes, stream, who, preds, labels, lens, L, round_up(L, 4), tau, iters, k, powered,
                                  f.hist_lds, ws, loss_q, grad);
        };
        const int rc = !f.resident ? go(neuralndcg_kernel<false, 256>)
                     : f.G == 256  ? go(neuralndcg_kernel<true, 256>)
                     : f.G == 128  ? go(neuralndcg_kernel<true, 128>)
                                   : go(neuralndcg_kernel<true, 64>);
        if (rc) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}
