// Linear trees for the tree trainer (linear_tree / linear_lambda of ptranking_amd/gbdt.py, LightGBM's names): a tree grows as it always
// did, then every leaf is fitted with a small linear model over the distinct features on its root-to-leaf path.  The rule is this
// project's own, modelled on LightGBM's LinearTreeLearner; include/ptranking_amd.h states it and tests/gbdt_linear_ref.py restates it.
// Three kernel families, none with a float atomic: two runs give the same bits.
//
// gbdt_linear_moments_kernel: [A | b] = sum over a leaf's usable rows of z^T [h z | g], z = (x_P1 .. x_Pk, 1), in float64 on
//   v_mfma_f64_16x16x4_f64.
//
//   Work split.  An item is (leaf, kLinChunkRows consecutive entries of the leaf's segment of the row list); the host lists the items.  A
//   workgroup of four waves takes one item, wave w the fixed quarter w of its entries, four entries per MFMA step as the K dimension.
//
//   Operands.  Lane l stands for entry r = l / 16 of the step and column c = l % 16.  The A operand is z^T: lane l holds z[r][16 rb + c]
//   for row block rb.  The B operand is [h z | g]: lane l holds h_r z[r][16 cb + c], or g_r in column k + 1, for column block cb.  D then
//   accumulates [A | b] at once: (k + 1) x (k + 2) <= 31 x 32, which is why a leaf takes at most 30 regressors.  A is symmetric, so of the
//   2 x 2 blocks of 16 x 16 the three (0,0), (0,1), (1,1) are computed (b sits in column block 1 whenever row block 1 is not empty), and a
//   leaf of k + 2 <= 16 columns computes (0,0) alone behind a workgroup-uniform branch.  Per step a lane gathers ONE fp32 of the raw
//   matrix per column block, widens it and forms h z in float64 (fp32 x fp32 is exact there).  A lane beyond column k + 1, an entry beyond
//   the wave's range and an unusable row feed ZERO operands by selection, never by a multiplication (NaN x 0 is NaN).  A row is usable iff
//   none of its regressors is NaN: a ballot across the 16 lanes that hold the row.
//
//   Pipeline.  The row index of step s + 2 and the gather of step s + 1 are issued before the MFMAs of step s: two dependent global
//   latencies (index, then value) stay in flight under the matrix work.
//
//   Reduction.  Every wave stores its three D blocks to LDS (4 x 3 x 2 KiB = 24 KiB); the workgroup adds them in wave order 0, 1, 2, 3 and
//   writes the item's partial [32][32] float64 (the blocks it computed; (1,0) is never written or read) and the integer count of usable
//   rows to the item's own workspace slot.
//
//   R = kLinChunkRows = 1024 and four waves, reasoned from the code: the kernel is a gather, k + 1 scattered fp32 out of a
//   row of 4 F bytes per entry, so what hides its latency is waves in flight.  A wave needs 3 x 4 accumulator VGPR pairs and two steps of
//   operands, far below the 128-register line; the 24 KiB of LDS let six workgroups (24 waves) share the 160 KiB of a compute unit.  At
//   1M rows and 31 leaves R = 1024 gives about 1000 items, four per compute unit, 64 steps per wave; a partial is 8 KiB, so the workspace
//   stays under 9 MB and the solve reads about 32 partials per leaf.  A smaller R multiplies the workspace traffic, a larger one leaves
//   compute units idle at the row counts people train on.  Measured on an MI355X (profiles/mi355x_gbdt_linear.json: 795 428 rows x 136
//   features, 31 leaves of 3.6 regressors on average): 0.083 ms per tree beside 3.8 ms of growth kernels, 251 GB/s of the gather's own
//   bytes (4 k + 12 per entry), 3 % of the HBM peak: the kernel moves few bytes per row and is bound by the latency of scattered
//   4-byte reads, as reasoned, not by bandwidth; other values of R were not measured.
//
// gbdt_linear_solve_kernel: one wavefront per leaf, all leaves of a tree in one launch.  The leaf's partials are added in item order, the
//   ridge term goes on the k feature diagonals, and the (k + 1) x (k + 1) system is factorised in LDS by a right-looking Cholesky without
//   pivoting, lane i owning row i.  A pivot must be finite and exceed 2^-40 times its original diagonal entry (the relative floor is part
//   of the rule: a regressor that is constant over the leaf is collinear with the intercept and must fall back).  Forward and back
//   substitution, the learning rate, then leaf_coeff, leaf_const and the status.
//
// gbdt_linear_walk_kernel: a row's walk through gbdt_walk under the raw predictor's predicate (ptr_gbdt.h), so it lands where predict puts
//   it, and gbdt_linear_leaf_output, the ONE device function of a leaf's output: both training (one tree added to the resident scores
//   over all rows of the resident raw matrix) and prediction (the trees first_tree .. stop - 1) run it.  fp32 adds in tree order.
#include <math.h>

#include "ptr_gbdt.h"

namespace ptr {

constexpr int kLinMaxFeatures = 30;      // regressors of a leaf at the most: k + 2 columns fill two 16-column blocks
constexpr int kLinDim = 32;              // the partial [A | b] is stored [kLinDim][kLinDim]
constexpr int kLinChunkRows = 1024;      // entries of the row list per item
constexpr int kLinWaves = kBlock / kWave;
static_assert(kLinChunkRows % (4 * kLinWaves) == 0, "every wave takes whole MFMA steps of four entries");

typedef double double4_t __attribute__((ext_vector_type(4)));

// What a lane feeds one step: z of its two columns (A operands), [h z | g] of them (B operands), already zero where masked.
struct LinOperands { double a0, a1, b0, b1; int usable; };

// The gather of a step, issued ahead of its use: the raw values of the lane's two columns and the row's (g, h).
struct LinGather { float x0, x1, g, h; int row; };

__device__ __forceinline__ LinGather lin_gather(const float *__restrict__ X, int F, const float *__restrict__ g, const float *__restrict__ h, int row, int f0,
                                                int f1, bool wide) {
    LinGather q{0.0f, 0.0f, 0.0f, 0.0f, row};
    if (row < 0) return q;
    const float *x = X + (int64_t)row * F;
    if (f0 >= 0) q.x0 = x[f0];
    if (wide && f1 >= 0) q.x1 = x[f1];
    q.g = g[row];
    q.h = h[row];
    return q;
}

// c: the lane's column in block 0; k: the regressors.  Column j < k is a feature, column k the intercept, column k + 1 the gradient (B only).
__device__ __forceinline__ LinOperands lin_operands(const LinGather &q, int c, int k, int f0, int f1, bool wide) {
    const int r = (threadIdx.x & 63) >> 4;
    const bool nan = q.row >= 0 && ((f0 >= 0 && q.x0 != q.x0) || (wide && f1 >= 0 && q.x1 != q.x1));
    const unsigned long long vote = __ballot(nan);
    const bool usable = q.row >= 0 && ((vote >> (16 * r)) & 0xFFFFull) == 0ull;
    LinOperands o{0.0, 0.0, 0.0, 0.0, usable ? 1 : 0};
    if (!usable) return o;
    const double hd = (double)q.h, gd = (double)q.g;
    const double z0 = c < k ? (double)q.x0 : (c == k ? 1.0 : 0.0);
    o.a0 = z0;
    o.b0 = c <= k ? hd * z0 : (c == k + 1 ? gd : 0.0);
    if (wide) {
        const int c1 = c + 16;
        const double z1 = c1 < k ? (double)q.x1 : (c1 == k ? 1.0 : 0.0);
        o.a1 = z1;
        o.b1 = c1 <= k ? hd * z1 : (c1 == k + 1 ? gd : 0.0);
    }
    return o;
}

// items int32 [nitems][3]: (leaf, first entry, entries <= kLinChunkRows); feats int32 [leaves][kLinMaxFeatures] padded with -1; nfeat
// int32 [leaves].  ws float64 [nitems][32][32], usable int32 [nitems].
__global__ void __launch_bounds__(kBlock)
gbdt_linear_moments_kernel(const float *__restrict__ X, int64_t n, int F, const int32_t *__restrict__ rows, int64_t m, const int32_t *__restrict__ items,
                           const int32_t *__restrict__ feats, const int32_t *__restrict__ nfeat, int leaves, const float *__restrict__ g,
                           const float *__restrict__ h, double *__restrict__ ws, int32_t *__restrict__ usable_out) {
    __shared__ double part[kLinWaves][3][256];
    __shared__ int32_t cnt[kLinWaves];
    const int item = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int leaf = items[item * 3];
    int64_t first = items[item * 3 + 1];
    int count = items[item * 3 + 2];
    double *slot = ws + (int64_t)item * kLinDim * kLinDim;
    int k = leaf >= 0 && leaf < leaves ? nfeat[leaf] : 0;
    if (k < 1 || k > kLinMaxFeatures || first < 0 || count < 0 || count > kLinChunkRows || first + count > m) { k = 0; count = 0; }   // a malformed item sums nothing
    const bool wide = k + 2 > 16;                                          // workgroup-uniform
    const int c = lane & 15, r = lane >> 4;
    int f0 = -1, f1 = -1;
    if (c < k) f0 = feats[leaf * kLinMaxFeatures + c];
    if (c + 16 < k) f1 = feats[leaf * kLinMaxFeatures + c + 16];
    if (f0 >= F) f0 = -1;                                                  // a feature outside the matrix reads nothing (its column is then zero)
    if (f1 >= F) f1 = -1;
    // the wave's fixed quarter of the item
    const int per = kLinChunkRows / kLinWaves;
    const int lo = wave * per, hi = lo + per < count ? lo + per : count;
    const int steps = hi > lo ? (hi - lo + 3) >> 2 : 0;
    auto entry = [&](int s) -> int {                                       // the row of this lane's entry in step s, -1 beyond the range or outside X
        const int e = lo + 4 * s + r;
        if (s >= steps || e >= hi) return -1;
        const int row = rows[first + e];
        return row >= 0 && row < n ? row : -1;
    };
    double4_t d00 = {0.0, 0.0, 0.0, 0.0}, d01 = d00, d11 = d00;
    int used = 0;
    LinGather cur = lin_gather(X, F, g, h, entry(0), f0, f1, wide);
    int next_row = entry(1);
    for (int s = 0; s < steps; ++s) {
        const int after = entry(s + 2);                                    // the index two steps ahead
        const LinGather nxt = lin_gather(X, F, g, h, next_row, f0, f1, wide);   // the gather one step ahead, in flight under the MFMAs
        const LinOperands o = lin_operands(cur, c, k, f0, f1, wide);
        d00 = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a0, o.b0, d00, 0, 0, 0);
        if (wide) {
            d01 = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a0, o.b1, d01, 0, 0, 0);
            d11 = __builtin_amdgcn_mfma_f64_16x16x4f64(o.a1, o.b1, d11, 0, 0, 0);
        }
        used += c == 0 ? o.usable : 0;                                     // one lane per entry counts it
        cur = nxt;
        next_row = after;
    }
    // D of v_mfma_f64_16x16x4_f64: register v of lane l holds D[4 v + l / 16][l % 16]
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int e = (4 * v + r) * 16 + c;
        part[wave][0][e] = d00[v];
        part[wave][1][e] = d01[v];
        part[wave][2][e] = d11[v];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) used += __shfl_xor(used, off);
    if (lane == 0) cnt[wave] = used;
    __syncthreads();
    for (int e = tid; e < 3 * 256; e += kBlock) {
        const int b = e >> 8, i = (e >> 4) & 15, j = e & 15;
        if (b > 0 && !wide) break;
        double sum = part[0][b][e & 255];
#pragma unroll
        for (int w = 1; w < kLinWaves; ++w) sum += part[w][b][e & 255];    // wave order: fixed
        const int row = i + (b == 2 ? 16 : 0), col = j + (b >= 1 ? 16 : 0);
        slot[row * kLinDim + col] = sum;
    }
    if (tid == 0) usable_out[item] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// status of a leaf
enum { kLinFitted = 0, kLinNoFeature = 1, kLinTooMany = 2, kLinFewRows = 3, kLinPivot = 4, kLinNotFinite = 5 };

// item_offsets int32 [leaves + 1]: leaf l owns the partials item_offsets[l] .. item_offsets[l + 1] - 1.  coeff float64 [leaves][30], cst
// float64 [leaves], status int32 [leaves], usable int32 [leaves] (m_u).  A leaf that falls back writes zeros.
__global__ void __launch_bounds__(kWave)
gbdt_linear_solve_kernel(const double *__restrict__ ws, const int32_t *__restrict__ usable, int64_t nitems, const int32_t *__restrict__ item_offsets,
                         const int32_t *__restrict__ nfeat, double lambda, double lr, double *__restrict__ coeff, double *__restrict__ cst,
                         int32_t *__restrict__ status, int32_t *__restrict__ usable_out) {
    __shared__ double M[kLinDim][kLinDim + 1];                             // the system, then its factor L in the lower triangle
    __shared__ double rhs[kLinDim], diag0[kLinDim];
    __shared__ int fail;
    const int leaf = blockIdx.x, lane = threadIdx.x;
    const int k = nfeat[leaf], d = k + 1;
    int64_t i0 = item_offsets[leaf], i1 = item_offsets[leaf + 1];
    if (i0 < 0 || i1 < i0 || i1 > nitems) i0 = i1 = 0;
    int st = k < 1 ? kLinNoFeature : k > kLinMaxFeatures ? kLinTooMany : kLinFitted;
    int mu = 0;
    if (st == kLinFitted) {
        for (int64_t it = i0; it < i1; ++it) mu += usable[it];
        if (mu < k + 1) st = kLinFewRows;
    }
    if (lane == 0) fail = 0;
    if (st == kLinFitted) {
        // the upper triangle and the b column (column d), summed in item order
        for (int e = lane; e < kLinDim * kLinDim; e += kWave) {
            const int i = e >> 5, j = e & 31;
            if (i > j || i >= d || j > d) continue;
            double sum = 0.0;
            for (int64_t it = i0; it < i1; ++it) sum += ws[it * kLinDim * kLinDim + e];
            if (j == d) rhs[i] = sum;
            else {
                if (i == j) { if (i < k) sum += lambda; diag0[i] = sum; }
                M[i][j] = sum;
                M[j][i] = sum;
            }
        }
        __syncthreads();
        for (int j = 0; j < d; ++j) {                                       // right-looking Cholesky, lane i owns row i
            const double p = M[j][j];
            const bool good = p > 0x1p-40 * diag0[j] && p < INFINITY;     // a NaN fails both comparisons
            if (!good) { if (lane == 0) fail = 1; break; }                // uniform: every lane read the same p
            const double ljj = sqrt(p);
            __syncthreads();
            if (lane == j) M[j][j] = ljj;
            if (lane > j && lane < d) M[lane][j] = M[lane][j] / ljj;
            __syncthreads();
            if (lane > j && lane < d) {
                const double lij = M[lane][j];
                for (int cc = j + 1; cc <= lane; ++cc) M[lane][cc] -= lij * M[cc][j];
            }
            __syncthreads();
        }
        __syncthreads();
        if (fail) st = kLinPivot;
    }
    if (st == kLinFitted) {
        for (int j = 0; j < d; ++j) {                                       // L y = b
            const double yj = rhs[j] / M[j][j];
            __syncthreads();
            if (lane == j) rhs[j] = yj;
            if (lane > j && lane < d) rhs[lane] -= M[lane][j] * yj;
            __syncthreads();
        }
        for (int j = d - 1; j >= 0; --j) {                                  // L^T w = y
            const double wj = rhs[j] / M[j][j];
            __syncthreads();
            if (lane == j) rhs[j] = wj;
            if (lane < j) rhs[lane] -= M[j][lane] * wj;
            __syncthreads();
        }
        const bool bad = lane < d && !(fabs(rhs[lane]) < INFINITY);
        if (__any(bad)) st = kLinNotFinite;
    }
    if (lane < kLinMaxFeatures) coeff[leaf * kLinMaxFeatures + lane] = st == kLinFitted && lane < k ? -rhs[lane] * lr : 0.0;
    if (lane == 0) {
        cst[leaf] = st == kLinFitted ? -rhs[k] * lr : 0.0;
        status[leaf] = st;
        usable_out[leaf] = mu;
    }
}

// A leaf's output for a raw row (rule 7 of include/ptranking_amd.h): the ONE function of training and prediction.  A constant leaf
// (features[0] < 0) or a NaN regressor gives `value`; otherwise float(const + sum_j coeff_j * double(x_Pj)), float64, in path order.  A
// feature outside the matrix gives NaN.
__device__ __forceinline__ float gbdt_linear_leaf_output(const float *__restrict__ x, int F, float value, const int32_t *__restrict__ features,
                                                         const double *__restrict__ coeff, double cst) {
    double acc = cst;
    for (int j = 0; j < kLinMaxFeatures; ++j) {
        const int f = features[j];
        if (f < 0) { if (j == 0) return value; break; }
        if (f >= F) return NAN;
        const float xv = x[f];
        if (xv != xv) return value;
        acc = acc + coeff[j] * (double)xv;
    }
    return (float)acc;
}

// out[i] = (in ? in[i] : 0) + the outputs of the trees first .. stop - 1 for raw row i, fp32 adds in tree order.  The leaf arrays follow
// the layout of the leaf values: tree t owns the leaves tree_offsets[t] + t ...
__global__ void __launch_bounds__(kBlock)
gbdt_linear_walk_kernel(const float *__restrict__ X, int64_t n, int F, const int32_t *__restrict__ feature, const float *__restrict__ threshold,
                        const int32_t *__restrict__ left, const int32_t *__restrict__ right, const float *__restrict__ value,
                        const int32_t *__restrict__ tree_offsets, const uint8_t *__restrict__ default_left, const int32_t *__restrict__ leaf_features,
                        const double *__restrict__ leaf_coeff, const double *__restrict__ leaf_const, int first, int stop, const float *in,
                        float *out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *x = X + i * F;
    const GbdtCatWalk nocat{nullptr, nullptr, nullptr, 0};
    float s = in ? in[i] : 0.0f;
    for (int t = first; t < stop; ++t) {
        const int base = tree_offsets[t], nn = tree_offsets[t + 1] - base;
        bool bad = false;
        const int node = gbdt_walk(nn, F, feature + base, left + base, right + base,
                                   [&](int at, int f) { return gbdt_raw_goes_left<false>(x[f], base + at, f, threshold, default_left, nocat, bad); });
        float v = NAN;                                                     // a malformed tree gives NaN
        if (gbdt_is_leaf(node, nn)) {
            const int64_t l = (int64_t)base + t + ~node;
            v = gbdt_linear_leaf_output(x, F, value[l], leaf_features + l * kLinMaxFeatures, leaf_coeff + l * kLinMaxFeatures, leaf_const[l]);
        }
        s = __fadd_rn(s, v);
    }
    out[i] = s;
}

}  // namespace ptr

using namespace ptr;

extern "C" int ptr_gbdt_linear_moments(const float *X, int64_t n, int F, const int32_t *rows, int64_t m, const int32_t *items, int64_t nitems,
                                       const int32_t *feats, const int32_t *nfeat, int leaves, const float *g, const float *h, double *ws,
                                       int32_t *usable, void *stream) {
    const char *who = "ptr_gbdt_linear_moments";
    if (n < 0 || F < 0 || m < 0 || nitems < 0 || leaves < 0 || n > INT32_MAX || nitems > INT32_MAX) {
        set_error("%s: bad size (n=%lld, F=%d, m=%lld, nitems=%lld, leaves=%d)", who, (long long)n, F, (long long)m, (long long)nitems, leaves);
        return PTR_ERR_INVALID_ARG;
    }
    if (nitems == 0) return 0;
    if (!X || !rows || !items || !feats || !nfeat || !g || !h || !ws || !usable) { set_error("%s: NULL pointer", who); return PTR_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(gbdt_linear_moments_kernel, dim3((unsigned)nitems), dim3(kBlock), 0, as_stream(stream), X, n, F, rows, m, items, feats, nfeat, leaves, g,
                       h, ws, usable);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_linear_solve(const double *ws, const int32_t *usable, int64_t nitems, const int32_t *item_offsets, const int32_t *nfeat,
                                     int leaves, double lambda, double lr, double *coeff, double *cst, int32_t *status, int32_t *usable_out,
                                     void *stream) {
    const char *who = "ptr_gbdt_linear_solve";
    if (nitems < 0 || leaves < 0) { set_error("%s: negative size (nitems=%lld, leaves=%d)", who, (long long)nitems, leaves); return PTR_ERR_INVALID_ARG; }
    if (!(lambda >= 0.0 && lambda < INFINITY) || !(lr == lr)) { set_error("%s: lambda must be finite and >= 0, lr no NaN", who); return PTR_ERR_INVALID_ARG; }
    if (leaves == 0) return 0;
    if ((nitems > 0 && (!ws || !usable)) || !item_offsets || !nfeat || !coeff || !cst || !status || !usable_out) {
        set_error("%s: NULL pointer", who);
        return PTR_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(gbdt_linear_solve_kernel, dim3(leaves), dim3(kWave), 0, as_stream(stream), ws, usable, nitems, item_offsets, nfeat, lambda, lr, coeff,
                       cst, status, usable_out);
    return check_hip(hipGetLastError(), who);
}

static int linear_walk(const char *who, const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                       const int32_t *right, const float *value, const int32_t *tree_offsets, const uint8_t *default_left, const int32_t *leaf_features,
                       const double *leaf_coeff, const double *leaf_const, int first, int stop, const float *in, float *out, void *stream) {
    if (n < 0 || F < 0 || first < 0 || stop < first) { set_error("%s: bad size (n=%lld, F=%d, trees %d .. %d)", who, (long long)n, F, first, stop); return PTR_ERR_INVALID_ARG; }
    if (n == 0) return 0;
    if (!out || (F > 0 && !X)) { set_error("%s: NULL pointer (X or out)", who); return PTR_ERR_INVALID_ARG; }
    if (stop > first && (!value || !tree_offsets || !leaf_features || !leaf_coeff || !leaf_const)) { set_error("%s: NULL tree array", who); return PTR_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(gbdt_linear_walk_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream), X, n, F, feature, threshold,
                       left, right, value, tree_offsets, default_left, leaf_features, leaf_coeff, leaf_const, first, stop, in, out);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_predict_linear(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                       const int32_t *right, const float *value, const int32_t *tree_offsets, const uint8_t *default_left,
                                       const int32_t *leaf_features, const double *leaf_coeff, const double *leaf_const, int first_tree, int stop,
                                       float *out, void *stream) {
    return linear_walk("ptr_gbdt_predict_linear", X, n, F, feature, threshold, left, right, value, tree_offsets, default_left, leaf_features, leaf_coeff,
                       leaf_const, first_tree, stop, nullptr, out, stream);
}

extern "C" int ptr_gbdt_add_tree_linear(float *scores, const float *X, int64_t n, int F, const int32_t *feature, const float *threshold,
                                        const int32_t *left, const int32_t *right, const float *value, const int32_t *tree_offsets,
                                        const uint8_t *default_left, const int32_t *leaf_features, const double *leaf_coeff, const double *leaf_const,
                                        void *stream) {
    const char *who = "ptr_gbdt_add_tree_linear";
    if (!scores && n > 0) { set_error("%s: NULL pointer (scores)", who); return PTR_ERR_INVALID_ARG; }
    return linear_walk(who, X, n, F, feature, threshold, left, right, value, tree_offsets, default_left, leaf_features, leaf_coeff, leaf_const, 0, 1, scores,
                       scores, stream);
}
