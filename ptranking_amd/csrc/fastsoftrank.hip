// FastSoftRank: soft ranks as the Euclidean projection onto the permutahedron (Blondel, Teboul, Berthet, Djolonga, ICML 2020; L2 regulariser),
// a Spearman or soft-nDCG objective on them and its exact gradient, in one launch.  The rule is stated in include/ptranking_amd.h.
//
// Per query the state is O(L): one sort, one isotonic regression, one block-mean pass.  Nothing of size L x L exists anywhere.
//
// The isotonic regression is NOT run as pool-adjacent-violators (a serial stack) but in its cumulative-sum form, which is exactly parallel:
//     S_k = sum_{i <= k} u_i (fp64, S_0 = 0),   g(j) = max_{k > j} (S_k - S_j) / (k - j),   v_i = min_{j < i} g(j),
// a block starting at position j + 1 exactly where g(j) is strictly below the running minimum of g(0 .. j-1).  The rho = (n, n-1, .., 1) part of
// S has the closed form k n - k (k-1) / 2 and stays out of the sum: only the fp32 keys are added, in fp64.
//
// Shape: G threads serve a query, G = 64 (one wavefront, four queries per workgroup, wave-level hand-overs only) up to kFsrWaveMaxLen
// documents, G = 256 (the workgroup) up to 4096.  A thread OWNS the documents i = t, t + G, ... (DPT of them, in registers: key, label, position,
// target, dloss/drank); everything indexed by POSITION lives in LDS.  Steps:
//   1. z = -theta / eps (one IEEE division), keys and labels to LDS by document; count_ranks gives every document its position
//      (key descending, index ascending); the label counts (ideal position, or #greater / #equal for the fractional hard rank) the same way.
//   2. the keys go back to LDS by position; a blocked fp64 scan (in-thread, DPP-free shuffles across lanes, wave totals through LDS) writes S.
//   3. the g pass, O(n^2 / 2): a thread takes the rows j and n-1-j (n + 1 pairs together, so the triangle balances); S_k is an LDS
//      broadcast, 1 / (k - j) comes from a reciprocal table whose reads are consecutive across the lanes; v_max_f64 keeps the row maximum.
//   4. a blocked prefix-min scan turns g into v in place and flags the block starts; a prefix-max scan of the flagged positions gives every
//      position its block's start, a scatter at the block boundaries every start its block's end.
//   5. by document again: r = z - v[position]; the objective's dloss/dr goes to LDS by position, a blocked fp64 prefix sum of it gives every
//      block mean as ONE difference at the block's boundaries; the gradient is -(a - mean) / eps.  No atomics: the bits depend on the
//      query's data, L and the form alone.
//
// LDS per query (Lp = round_up(L, 4), N1 = Lp + 4): S | G | RD fp64 [N1] each, 8 fp64 of scan scratch, Z fp32 [Lp]: 28 Lp + 160 bytes, 114 848
// at L = 4096.  The label row aliases G (dead before the g pass), the block starts / ends alias RD (dead after it), dloss/dr by position
// aliases S and its prefix sum G (both dead after step 5's rank read); S then takes the prefix count of its non-zero values.
#include "ptr_device.h"

namespace ptr {

__host__ __device__ static inline size_t fsr_query_bytes(int Lp) { return (size_t)3 * (Lp + 4) * sizeof(double) + 8 * sizeof(double) + (size_t)Lp * sizeof(float); }

FsrForm fastsoftrank_form(int L) {
    const int G = L <= kFsrWaveMaxLen ? kWave : kBlock;
    int dpt = 1;
    while (G * dpt < L) dpt *= 2;
    return {G, dpt, kBlock / G, (int)(kBlock / G * fsr_query_bytes(round_up(L, 4))), kFsrWaveMaxLen};
}

struct FsrArgs {
    const float *preds, *labels;
    const int32_t *lens;
    int B, L;
    float eps;
    int objective;
    float *loss_q, *ranks, *grad;
};

// Exclusive scan of one fp64 value per thread over the G threads of a group, thread order, `op` associative with identity `ident`.
// G == 256: workgroup barriers inside (every thread of the block calls it); red = 4 doubles of LDS.
template <int G, class Op> __device__ __forceinline__ double fsr_excl_scan(double v, Op op, double ident, double *red, int t) {
    const int lane = t & 63;
    double inc = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const double o = __shfl_up(inc, d, kWave);
        if (lane >= d) inc = op(o, inc);
    }
    double ex = __shfl_up(inc, 1, kWave);
    if (lane == 0) ex = ident;
    if constexpr (G == kBlock) {
        __syncthreads();
        if (lane == 63) red[t >> 6] = inc;
        __syncthreads();
        double carry = ident;
        for (int w = 0; w < (t >> 6); ++w) carry = op(carry, red[w]);
        ex = op(carry, ex);
    }
    return ex;
}

// Sum of one fp64 value per thread over the group, fixed order; every thread gets it.  red as above.
template <int G> __device__ __forceinline__ double fsr_sum(double v, double *red, int t) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    if constexpr (G == kBlock) {
        __syncthreads();
        if ((t & 63) == 0) red[t >> 6] = v;
        __syncthreads();
        v = ((red[0] + red[1]) + red[2]) + red[3];
    }
    return v;
}

template <int G> __device__ __forceinline__ bool fsr_any(bool x) {
    if constexpr (G == kBlock) return __syncthreads_or(x) != 0;
    else return __any(x) != 0;
}

template <int G, int DPT>
__global__ void __launch_bounds__(kBlock) fsr_kernel(const FsrArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char fsr_smem[];
    constexpr int QPB = kBlock / G;
    const int t = threadIdx.x % G, q = blockIdx.x * QPB + threadIdx.x / G;
    if (q >= A.B) return;                                                    // G == 64 only: a whole wavefront leaves, nothing block-wide follows
    const int L = A.L, Lp = (L + 3) & ~3, N1 = Lp + 4;
    const int n = query_len(A.lens, q, L);
    double *S = reinterpret_cast<double *>(fsr_smem + (size_t)(threadIdx.x / G) * fsr_query_bytes(Lp));
    double *Gd = S + N1, *RD = Gd + N1, *red = RD + N1;
    float *Z = reinterpret_cast<float *>(red + 8);
    float *Y = reinterpret_cast<float *>(Gd);                                // labels by document, until the g pass
    int *ST = reinterpret_cast<int *>(RD), *EN = ST + Lp;                    // block start by position, block end by start, after the g pass
    const size_t row = (size_t)q * L;
    const double INF = (double)INFINITY, eps = (double)A.eps;

    // ---- 1. keys and labels, by document
    float z[DPT], y[DPT];
    bool bad = false;
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        z[m] = i < n ? __fdiv_rn(-A.preds[row + i], A.eps) : -INFINITY;
        y[m] = i < n ? A.labels[row + i] : -INFINITY;
        bad |= i < n && !(fabsf(z[m]) < INFINITY);                           // NaN, or a key beyond fp32
        if (i < Lp) { Z[i] = z[m]; Y[i] = y[m]; }
    }
    if (fsr_any<G>(bad) || n == 0) {                                         // a NaN score poisons its own query; an empty one gives zeros
        const float v = n > 0 ? __builtin_nanf("") : 0.0f;
        for (int i = t; i < L; i += G) {
            if (A.ranks) A.ranks[row + i] = i < n ? v : 0.0f;
            if (A.grad) A.grad[row + i] = i < n ? v : 0.0f;
        }
        if (t == 0) A.loss_q[q] = v;
        return;
    }
    for (int d = t + 1; d <= n; d += G) RD[d] = 1.0 / (double)d;
    group_sync<G>();
    int rk[DPT];
    count_ranks<G, DPT>(Z, n, t, z, rk);
    // the labels: the target rank (Spearman: fractional hard rank, ties share the mean of their positions) or the gain over the ideal DCG
    double tgt[DPT];
    const bool ndcg = A.objective == PTR_FSR_NDCG;
    if (ndcg) {
        int ipos[DPT];
        count_ranks<G, DPT>(Y, n, t, y, ipos);
        double part = 0.0;
#pragma unroll
        for (int m = 0; m < DPT; ++m) {
            tgt[m] = t + m * G < n ? exp2((double)y[m]) - 1.0 : 0.0;
            if (t + m * G < n) part += tgt[m] / log2(2.0 + (double)ipos[m]);
        }
        const double idcg = fsr_sum<G>(part, red, t);
        const double inv = idcg > 0.0 ? 1.0 / idcg : 0.0;                    // no relevant document: loss 0, gradient 0
#pragma unroll
        for (int m = 0; m < DPT; ++m) tgt[m] *= inv;
    } else {
        int gt[DPT], ge[DPT];
#pragma unroll
        for (int m = 0; m < DPT; ++m) { gt[m] = 0; ge[m] = 0; }
        const float4 *y4 = reinterpret_cast<const float4 *>(Y);
        for (int j4 = 0; j4 < (n + 3) >> 2; ++j4) {
            const float4 v = y4[j4];
#pragma unroll
            for (int m = 0; m < DPT; ++m) {
                gt[m] += (v.x > y[m]) + (v.y > y[m]) + (v.z > y[m]) + (v.w > y[m]);
                ge[m] += (v.x >= y[m]) + (v.y >= y[m]) + (v.z >= y[m]) + (v.w >= y[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < DPT; ++m) tgt[m] = 0.5 * (double)(gt[m] + ge[m] + 1);         // gt + (eq + 1) / 2, eq = ge - gt counts the document
    }
    group_sync<G>();

    // ---- 2. keys by position, S by a blocked scan
#pragma unroll
    for (int m = 0; m < DPT; ++m)
        if (t + m * G < n) Z[rk[m]] = z[m];
    group_sync<G>();
    {
        float zs[DPT];
        double loc = 0.0;
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            zs[r] = p < n ? Z[p] : 0.0f;
            loc += (double)zs[r];
        }
        double run = fsr_excl_scan<G>(loc, [](double a, double b) { return a + b; }, 0.0, red, t);
        if (t == 0) S[0] = 0.0;
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            run += (double)zs[r];
            if (p < n) S[p + 1] = run - ((double)(p + 1) * (double)n - 0.5 * (double)(p + 1) * (double)p);
        }
    }
    group_sync<G>();

    // ---- 3. g(j) = max_{k > j} (S_k - S_j) / (k - j): rows j and n-1-j on one thread
    for (int j = t; j < (n + 1) / 2; j += G) {
        const int j2 = n - 1 - j;
        const double s1 = S[j], s2 = S[j2];
        double b1 = -INF, b2 = -INF;
#pragma unroll 4
        for (int k = j + 1; k <= j2; ++k) b1 = fmax(b1, (S[k] - s1) * RD[k - j]);
#pragma unroll 4
        for (int k = j2 + 1; k <= n; ++k) {
            const double sk = S[k];
            b1 = fmax(b1, (sk - s1) * RD[k - j]);
            b2 = fmax(b2, (sk - s2) * RD[k - j2]);
        }
        Gd[j] = b1;
        Gd[j2] = b2;
    }
    group_sync<G>();

    // ---- 4. v = prefix minimum of g, in place; block starts where g is strictly below the minimum so far; starts and ends by position
    {
        double gv[DPT], lmin = INF;
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            gv[r] = p < n ? Gd[p] : INF;
            lmin = fmin(lmin, gv[r]);
        }
        double prev = fsr_excl_scan<G>(lmin, [](double a, double b) { return fmin(a, b); }, INF, red, t);
        int stv[DPT], last = -1;
        unsigned flags = 0;
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            if (p < n) {
                if (p == 0 || gv[r] < prev) { last = p; flags |= 1u << r; }
                prev = fmin(prev, gv[r]);
                Gd[p] = prev;
            }
            stv[r] = last;
        }
        const int before = (int)fsr_excl_scan<G>((double)last, [](double a, double b) { return fmax(a, b); }, -1.0, red, t);
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            if (p < n) ST[p] = stv[r] >= 0 ? stv[r] : before;
        }
        group_sync<G>();
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            if (p < n && p > 0 && (flags >> r & 1u)) EN[ST[p - 1]] = p - 1;
            if (p == n - 1) EN[ST[p]] = p;
        }
    }
    group_sync<G>();

    // ---- 5. by document: rank, objective, dloss/drank
    double a[DPT], lsum = 0.0;
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        a[m] = 0.0;
        float rank = 0.0f;
        if (i < n) {
            const double r = (double)z[m] - Gd[rk[m]];
            rank = (float)r;
            if (ndcg) {
                const double lg = log2(1.0 + r);
                lsum -= tgt[m] / lg;
                a[m] = tgt[m] / (lg * lg * (1.0 + r) * 0.6931471805599453);
            } else {
                a[m] = r - tgt[m];
                lsum += 0.5 * a[m] * a[m];
            }
        }
        if (A.ranks && i < L) A.ranks[row + i] = rank;
    }
    lsum = fsr_sum<G>(lsum, red, t);
    if (t == 0) A.loss_q[q] = (float)lsum;
    if (!A.grad) return;
    group_sync<G>();                                                         // every read of v is done: S takes a by position
#pragma unroll
    for (int m = 0; m < DPT; ++m)
        if (t + m * G < n) S[rk[m]] = a[m];
    group_sync<G>();
    {
        double av[DPT], loc = 0.0, cnt = 0.0;
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            av[r] = p < n ? S[p] : 0.0;
            loc += av[r];
            cnt += av[r] != 0.0 ? 1.0 : 0.0;
        }
        double run = fsr_excl_scan<G>(loc, [](double x, double w) { return x + w; }, 0.0, red, t);
        // the same scan over the COUNT of non-zero values, into S (every thread has read its part): a rounded prefix sum need not return an
        // exact 0 over a run of zeros that crosses threads, and a block whose documents all have dloss/drank = 0 must give gradient 0
        double seen = fsr_excl_scan<G>(cnt, [](double x, double w) { return x + w; }, 0.0, red, t);
        if (t == 0) { Gd[0] = 0.0; S[0] = 0.0; }
#pragma unroll
        for (int r = 0; r < DPT; ++r) {
            const int p = t * DPT + r;
            run += av[r];
            seen += av[r] != 0.0 ? 1.0 : 0.0;
            if (p < n) { Gd[p + 1] = run; S[p + 1] = seen; }
        }
    }
    group_sync<G>();
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        float g = 0.0f;
        if (i < n) {
            const int st = ST[rk[m]], en = EN[st];
            const double mean = st == en ? a[m] : S[en + 1] == S[st] ? 0.0 : (Gd[en + 1] - Gd[st]) / (double)(en - st + 1);
            g = (float)(-(a[m] - mean) / eps);
        }
        if (i < L) A.grad[row + i] = g;
    }
}

}  // namespace ptr

extern "C" int ptr_fastsoftrank_fwd_bwd(const float *preds, const float *labels, const int32_t *lens, int B, int L, float eps, int objective,
                                        float *loss_out, float *loss_q, float *ranks, float *grad, void *stream) {
    using namespace ptr;
    const char *who = "ptr_fastsoftrank_fwd_bwd";
    if (int rc = check_loss_args(preds, labels, B, L, loss_q != nullptr, who)) return rc;
    if (!(eps > 0.0f) || !(eps < INFINITY)) { set_error("%s: eps must be a finite number > 0 (got %g)", who, (double)eps); return PTR_ERR_INVALID_ARG; }
    if (objective != PTR_FSR_SPEARMAN && objective != PTR_FSR_NDCG) {
        set_error("%s: unknown objective %d (PTR_FSR_SPEARMAN 0, PTR_FSR_NDCG 1)", who, objective);
        return PTR_ERR_INVALID_ARG;
    }
    if (B > 0) {
        const FsrArgs A{preds, labels, lens, B, L, eps, objective, loss_q, ranks, grad};
        const FsrForm f = fastsoftrank_form(L);
        auto go = [&](auto kern) -> int { return launch_queries(kern, B, f.QPB, kBlock, (size_t)f.lds_bytes, stream, who, A); };
        int rc;
        static_assert(kFsrWaveMaxLen == 2 * kWave, "the wavefront form is instantiated for one and two documents per lane");
        if (f.G == kWave) rc = f.DPT == 1 ? go(fsr_kernel<kWave, 1>) : go(fsr_kernel<kWave, 2>);
        else rc = f.DPT == 1 ? go(fsr_kernel<kBlock, 1>) : f.DPT == 2 ? go(fsr_kernel<kBlock, 2>) : f.DPT == 4 ? go(fsr_kernel<kBlock, 4>)
                : f.DPT == 8 ? go(fsr_kernel<kBlock, 8>) : go(fsr_kernel<kBlock, 16>);
        if (rc) return rc;
    }
    return finish_loss(loss_q, B, 1.0f, loss_out, stream);
}
