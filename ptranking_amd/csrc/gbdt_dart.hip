// DART boosting for the tree trainer (boosting='dart' of ptranking_amd/gbdt.py; Rashmi & Gilad-Bachrach, "DART: Dropouts meet
// Multiple Additive Regression Trees"): every round takes a SET of earlier trees out of the resident scores, grows a tree on the gradients
// taken there and puts the dropped trees back, rescaled.  Three kernels; include/ptranking_amd.h states their contracts and
// tests/gbdt_dart_ref.py restates them.
//
// ptr_gbdt_dart_walk: out[i] = in[i] + sign * (the leaf values the listed trees give binned row i, summed in list order).  One launch for
// the whole set, where ptr_gbdt_add_tree_binned is one launch per tree and reads a row's bins from global memory at random offsets, once
// per node and tree.
//
//   The forest is resident in bin space.  A node is two 32-bit words: word 0 = feature | split bin << 16 | also-left bin << 24, word 1 =
//   left | right << 16 as int16 (a child c < 0 is the leaf ~c).  A node without an also-left bin stores its split bin there, so the test
//   b <= bin || b == also needs no flag.  The leaf values are an fp32 array beside the nodes; tree t owns the nodes tree_offsets[t] ..
//   tree_offsets[t + 1] - 1 and the values from tree_offsets[t] + t on, as GBDT.flat() lays trees out.
//
//   The row tile.  A workgroup of 256 threads takes 256 consecutive rows; their bins are ONE contiguous block of 256 * stride bytes.  It is
//   copied with coalesced 16-byte loads into LDS at a row pitch of stride + 4 bytes (four 4-byte LDS stores per load: the pitch is a
//   multiple of 4, not of 16).  stride is a multiple of 16, so pitch / 4 is odd, and the 64 lanes of a wave that read the same feature of 64
//   consecutive rows address 64 different banks.  A row's bins are read from global memory once for all listed trees.
//
//   The trees go through LDS, double-buffered: every thread loads its share of listed tree j + 1 (two nodes, two values) into registers
//   before it walks tree j out of the other buffer, and stores the share behind the walk: the global latency of the fetch hides behind the
//   walk, and ONE barrier per tree orders both buffers.  A node is one 8-byte LDS read; node 0 is a broadcast.  A tree of more than
//   kDartLdsNodes nodes is walked from global memory behind a workgroup-uniform branch.  The direct form (a matrix too wide for the tile,
//   gbdt_dart_walk_form in ptr_gbdt.h) reads the bins from global memory and still stages the trees.
//
//   fp32 adds only (__fadd_rn), in list order: numpy float32 restates a row bit for bit.  A malformed tree (a cycle, a node or a feature
//   out of range) or a list entry outside the forest gives the row NaN; the walk takes at most nn steps.
//
// ptr_gbdt_dart_select: which trees a round drops, from the counter stream bagging draws from.  ptr_gbdt_dart_scale: the dropped trees'
// leaf values times a float64 factor.
#include <math.h>

#include "ptr_gbdt.h"
#include "ptr_plhash.h"

namespace ptr {

static_assert(2 * (kBlock - 1) + 1 == kDartLdsNodes && kDartLdsNodes * 8 + (kDartLdsNodes + 1) * 4 <= kDartTreeBytes / 2,
              "a thread stages two nodes and two values of a tree, and a buffer holds them all");

struct DartForest { const uint2 *nodes; const float *values; const int32_t *tree_offsets; int ntrees; };

// Listed tree j of the forest -> (first node, nodes, first value); nn = -1 for a list entry outside the forest or offsets that do not ascend.
struct DartTree { int base, nn, vbase; };
__device__ __forceinline__ DartTree dart_tree(const DartForest &fo, const int32_t *__restrict__ list, int j) {
    const int t = list[j];
    if (t < 0 || t >= fo.ntrees) return {0, -1, 0};
    const int base = fo.tree_offsets[t], nn = fo.tree_offsets[t + 1] - base;
    if (base < 0 || nn < 0 || nn > kDartMaxNodes) return {0, -1, 0};
    return {base, nn, base + t};
}

// A thread's share of a tree that fits the LDS buffer: the nodes and the values 2 tid, 2 tid + 1.
struct DartShare { uint2 n0, n1; float v0, v1; };
__device__ __forceinline__ DartShare dart_fetch(const DartForest &fo, const DartTree &tr) {
    DartShare s{{0u, 0u}, {0u, 0u}, 0.0f, 0.0f};
    if (tr.nn < 0 || tr.nn > kDartLdsNodes) return s;
    const int i = 2 * threadIdx.x;
    if (i < tr.nn) s.n0 = fo.nodes[tr.base + i];
    if (i + 1 < tr.nn) s.n1 = fo.nodes[tr.base + i + 1];
    if (i <= tr.nn) s.v0 = fo.values[tr.vbase + i];
    if (i + 1 <= tr.nn) s.v1 = fo.values[tr.vbase + i + 1];
    return s;
}
__device__ __forceinline__ void dart_store(const DartShare &s, uint2 *__restrict__ nodes, float *__restrict__ values) {
    const int i = 2 * threadIdx.x;                                         // 2 * 255 + 1 = kDartLdsNodes: every index is inside the buffers
    if (i < kDartLdsNodes) nodes[i] = s.n0;
    if (i + 1 < kDartLdsNodes) nodes[i + 1] = s.n1;
    values[i] = s.v0;
    values[i + 1] = s.v1;
}

// One row down one tree: x its bins (LDS or global), nodes / values the tree's (LDS or global) -> the leaf value, NaN for a malformed tree.
__device__ __forceinline__ float dart_leaf_value(const uint8_t *x, int F, const uint2 *nodes, const float *values, int nn) {
    int node = nn > 0 ? 0 : ~0;
    for (int step = 0; step < nn && node >= 0; ++step) {
        if (node >= nn) break;
        const uint2 w = nodes[node];
        const int f = (int)(w.x & 0xFFFFu);
        if (f >= F) break;
        const int b = x[f], bin = (int)((w.x >> 16) & 0xFFu), also = (int)(w.x >> 24);
        node = (b <= bin || b == also) ? (int)(int16_t)(w.y & 0xFFFFu) : (int)(int16_t)(w.y >> 16);
    }
    return node < 0 && ~node <= nn ? values[~node] : NAN;
}

template <bool kTile> __global__ void __launch_bounds__(kBlock)
gbdt_dart_walk_kernel(const float *in, float *out, const uint8_t *__restrict__ bins, int stride, int n, int F, const DartForest fo,
                      const int32_t *__restrict__ list, int k, float sign) {
    extern __shared__ __align__(16) uint8_t dart_lds[];
    // buffer b: kDartLdsNodes nodes at b * kDartTreeBytes / 2, the values behind them
    auto lnodes = [&](int b) { return reinterpret_cast<uint2 *>(dart_lds + b * (kDartTreeBytes / 2)); };
    auto lvalues = [&](int b) { return reinterpret_cast<float *>(dart_lds + b * (kDartTreeBytes / 2) + kDartLdsNodes * 8); };
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kBlock;
    const int64_t row = row0 + tid;
    const uint8_t *x;
    if constexpr (kTile) {
        uint8_t *tile = dart_lds + kDartTreeBytes;
        const int pitch = stride + 4, per_row = stride >> 4;
        const int rows_here = (int)(n - row0 < kBlock ? n - row0 : kBlock);
        const uint4 *src = reinterpret_cast<const uint4 *>(bins + row0 * stride);
        for (int c = tid; c < rows_here * per_row; c += kBlock) {          // the block is contiguous: chunk c is the next 16 bytes
            const uint4 v = src[c];
            uint32_t *dst = reinterpret_cast<uint32_t *>(tile + (c / per_row) * pitch + (c % per_row) * 16);
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
        x = tile + tid * pitch;
    } else {
        x = bins + (row < n ? row : 0) * stride;
    }
    DartTree cur = k > 0 ? dart_tree(fo, list, 0) : DartTree{0, -1, 0};
    dart_store(dart_fetch(fo, cur), lnodes(0), lvalues(0));
    __syncthreads();                                                       // the tile and the first tree
    float acc = 0.0f;
    for (int j = 0; j < k; ++j) {
        const bool more = j + 1 < k;
        DartTree nxt{0, -1, 0};
        DartShare share;
        if (more) {
            nxt = dart_tree(fo, list, j + 1);
            share = dart_fetch(fo, nxt);                                   // in flight while this tree is walked
        }
        if (row < n) {
            float v = NAN;
            if (cur.nn >= 0 && cur.nn <= kDartLdsNodes) v = dart_leaf_value(x, F, lnodes(j & 1), lvalues(j & 1), cur.nn);
            else if (cur.nn >= 0) v = dart_leaf_value(x, F, fo.nodes + cur.base, fo.values + cur.vbase, cur.nn);      // workgroup-uniform
            acc = __fadd_rn(acc, v);
        }
        if (more) dart_store(share, lnodes((j + 1) & 1), lvalues((j + 1) & 1));      // that buffer was last read a barrier ago
        __syncthreads();
        cur = nxt;
    }
    if (row < n) out[row] = __fadd_rn(in[row], sign < 0.0f ? -acc : acc);
}

// One workgroup.  Tree t < T is dropped iff u(seed, draw, t) < p[t]; sel[0] = the count, sel[1 ..] = the dropped trees, ascending.
__global__ void __launch_bounds__(kBlock)
gbdt_dart_select_kernel(const float *__restrict__ p, int T, uint64_t seed, int64_t draw, float skip_drop, int32_t *__restrict__ sel) {
    __shared__ int32_t scan[kBlock];
    const PlKeys keys = pl_query_keys(seed, draw);
    if (pl_uniform(keys, 0xFFFFFFFFu) < skip_drop) {                        // the whole round is skipped
        if (threadIdx.x == 0) sel[0] = 0;
        return;
    }
    int before = 0;
    for (int t0 = 0; t0 < T; t0 += kBlock) {
        const int t = t0 + threadIdx.x;
        const int32_t drop = t < T && pl_uniform(keys, (uint32_t)t) < p[t] ? 1 : 0;
        const int32_t upto = block_scan_add(scan, drop);
        if (drop) sel[1 + before + upto - 1] = t;
        before += scan[kBlock - 1];
        __syncthreads();                                                   // every thread has read the total before the next scan writes
    }
    if (threadIdx.x == 0) sel[0] = before;
}

// grid = the listed trees: value = (float)((double)value * factor) over the leaf values of listed tree blockIdx.x.
__global__ void __launch_bounds__(kBlock)
gbdt_dart_scale_kernel(float *__restrict__ values, const int32_t *__restrict__ tree_offsets, int ntrees, const int32_t *__restrict__ list, double factor) {
    const int t = list[blockIdx.x];
    if (t < 0 || t >= ntrees) return;
    const int base = tree_offsets[t], nn = tree_offsets[t + 1] - base;
    if (base < 0 || nn < 0) return;
    float *v = values + base + t;
    for (int i = threadIdx.x; i <= nn; i += kBlock) v[i] = (float)((double)v[i] * factor);
}

}  // namespace ptr

using namespace ptr;

extern "C" int ptr_gbdt_dart_walk(const float *in, float *out, const uint8_t *bins, int stride, int64_t n, int F, const uint32_t *nodes,
                                  const float *values, const int32_t *tree_offsets, int ntrees, const int32_t *list, int k, int sign,
                                  void *stream) {
    const char *who = "ptr_gbdt_dart_walk";
    if (n < 0 || F < 0 || n > INT32_MAX) { set_error("%s: bad size (n=%lld, F=%d; n must fit an int32 row index)", who, (long long)n, F); return PTR_ERR_INVALID_ARG; }
    if (stride < F || stride % kGbdtTile != 0) {
        set_error("%s: stride must be a multiple of %d and at least F (stride=%d, F=%d)", who, kGbdtTile, stride, F);
        return PTR_ERR_INVALID_ARG;
    }
    if (F > kDartMaxFeatures) { set_error("%s: a packed node keeps its feature in 16 bits: F must be <= %d, got %d", who, kDartMaxFeatures, F); return PTR_ERR_UNSUPPORTED; }
    if (ntrees < 0 || k < 0) { set_error("%s: bad size (ntrees=%d, k=%d)", who, ntrees, k); return PTR_ERR_INVALID_ARG; }
    if (sign != 1 && sign != -1) { set_error("%s: sign must be +1 or -1, got %d", who, sign); return PTR_ERR_INVALID_ARG; }
    if (n == 0) return 0;
    if (!in || !out || !bins || (k > 0 && (!list || !tree_offsets || !values))) { set_error("%s: NULL pointer (in, out, bins, list, tree_offsets or values)", who); return PTR_ERR_INVALID_ARG; }
    if (reinterpret_cast<uintptr_t>(bins) & 15) { set_error("%s: bins must be 16-byte aligned", who); return PTR_ERR_INVALID_ARG; }
    const GbdtDartForm form = gbdt_dart_walk_form_of_stride(n, stride, 0);             // the LDS tile is sized by the stride the kernel copies
    const DartForest fo{reinterpret_cast<const uint2 *>(nodes), values, tree_offsets, ntrees};
    if (form.kind == 1)
        hipLaunchKernelGGL(gbdt_dart_walk_kernel<true>, dim3(form.groups), dim3(kBlock), form.lds_bytes, as_stream(stream), in, out, bins, stride, (int)n, F, fo,
                           list, k, (float)sign);
    else
        hipLaunchKernelGGL(gbdt_dart_walk_kernel<false>, dim3(form.groups), dim3(kBlock), form.lds_bytes, as_stream(stream), in, out, bins, stride, (int)n, F, fo,
                           list, k, (float)sign);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_dart_select(const float *p, int T, uint64_t seed, int64_t draw, float skip_drop, int32_t *sel, void *stream) {
    const char *who = "ptr_gbdt_dart_select";
    if (T < 0) { set_error("%s: negative tree count (T=%d)", who, T); return PTR_ERR_INVALID_ARG; }
    if (draw < 0) { set_error("%s: negative draw (%lld)", who, (long long)draw); return PTR_ERR_INVALID_ARG; }
    if (!(skip_drop >= 0.0f && skip_drop <= 1.0f)) { set_error("%s: skip_drop must be in [0, 1], got %g", who, (double)skip_drop); return PTR_ERR_INVALID_ARG; }
    if (!sel || (T > 0 && !p)) { set_error("%s: NULL pointer (p or sel)", who); return PTR_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(gbdt_dart_select_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), p, T, seed, draw, skip_drop, sel);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_dart_scale(float *values, const int32_t *tree_offsets, int ntrees, const int32_t *list, int k, double factor, void *stream) {
    const char *who = "ptr_gbdt_dart_scale";
    if (ntrees < 0 || k < 0) { set_error("%s: bad size (ntrees=%d, k=%d)", who, ntrees, k); return PTR_ERR_INVALID_ARG; }
    if (!(factor == factor)) { set_error("%s: factor is NaN", who); return PTR_ERR_INVALID_ARG; }
    if (k == 0) return 0;
    if (!values || !tree_offsets || !list) { set_error("%s: NULL pointer (values, tree_offsets or list)", who); return PTR_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(gbdt_dart_scale_kernel, dim3(k), dim3(kBlock), 0, as_stream(stream), values, tree_offsets, ntrees, list, factor);
    return check_hip(hipGetLastError(), who);
}
