// The histogram launch form of the gradient-boosted tree kernels (csrc/gbdt.hip), shared with ptr_launch_form (csrc/abi.hip).
#pragma once
#include "ptr_device.h"

namespace ptr {

constexpr int kGbdtTile = 16;            // features per tile: one 16-byte load of a row's bins
constexpr int kGbdtDirectRows = 256;     // row lists up to this length add straight into global memory
constexpr int kGbdtChunkRows = 2048;     // least rows per workgroup of the LDS form (amortises zeroing and flushing the tile)
constexpr int kGbdtMaxGroups = 1024;     // workgroups of one LDS-form launch, about

// kind 0: nothing to launch (m == 0); 1: direct (one thread per (row, feature), integer atomics in global memory); 2: LDS tile
// (grid = chunks x tiles, a workgroup sums its rows' 16 features in LDS and flushes the bins it touched).
struct GbdtHistForm { int kind; int tile; int tiles; int chunks; int lds_bytes; };
inline GbdtHistForm gbdt_hist_form(int64_t m, int F, int max_bin) {
    const int tiles = (F + kGbdtTile - 1) / kGbdtTile;
    if (m <= 0 || F <= 0) return {0, kGbdtTile, tiles, 0, 0};
    if (m <= kGbdtDirectRows) return {1, kGbdtTile, tiles, 0, 0};
    const int64_t want = (m + kGbdtChunkRows - 1) / kGbdtChunkRows;
    const int64_t cap = kGbdtMaxGroups / tiles > 1 ? kGbdtMaxGroups / tiles : 1;
    return {2, kGbdtTile, tiles, (int)(want < cap ? want : cap), kGbdtTile * max_bin * 20};
}

// The batched histogram (ptr_gbdt_histogram_segments): a segment of m rows inside a call whose LDS-form segments hold `total` rows together.
// kind as above, by m alone; an LDS-form segment is cut into row chunks of chunk_rows, which grows with `total` so that a call stays at about
// kGbdtMaxGroups workgroups.  launches: the most launches one call makes (one per form), however many segments it holds.
struct GbdtSegForm { int kind; int tile; int tiles; int chunks; int lds_bytes; int chunk_rows; int direct_rows; int launches; };
inline GbdtSegForm gbdt_hist_segments_form(int64_t m, int F, int max_bin, int64_t total) {
    const int tiles = (F + kGbdtTile - 1) / kGbdtTile;
    const int64_t cap = kGbdtMaxGroups / (tiles > 0 ? tiles : 1) > 1 ? kGbdtMaxGroups / (tiles > 0 ? tiles : 1) : 1;
    int64_t per = ((total > 0 ? total : 0) + cap - 1) / cap;
    per = (per + kBlock - 1) / kBlock * kBlock;
    if (per < kGbdtChunkRows) per = kGbdtChunkRows;
    if (per > (1 << 30)) per = 1 << 30;
    GbdtSegForm f{0, kGbdtTile, tiles, 0, 0, (int)per, kGbdtDirectRows, 2};
    if (m <= 0 || F <= 0) return f;
    if (m <= kGbdtDirectRows) { f.kind = 1; f.chunks = 1; return f; }
    f.kind = 2;
    f.chunks = (int)((m + per - 1) / per);
    f.lds_bytes = kGbdtTile * max_bin * 20;
    return f;
}

// The packed histogram (ptr_gbdt_histogram_packed, ptr_gbdt_histogram_segments_packed): low-bit gradients, |qg| <= bound_g <= 128 and
// |qh| <= bound_h <= 256.  One LDS cell per (feature, bin) is ONE 64-bit word of three fields, from the low end: sum qg in 21 bits, sum qh
// in 21 bits (both two's complement), the count in 22 bits.  A row adds qg + (qh << 21) + (1 << 42) with one 64-bit LDS atomic.  The fields
// are exact while at most R = floor((2^20 - 1) / max(2 bound_g, bound_h)) rows went into a tile since it was last flushed; a workgroup
// flushes and re-zeroes its tile every R rows.  The grid, the row chunks and the direct form are those of the int64 kernels.
constexpr int kGbdtPackedBits = 21;      // bits of the two sum fields
constexpr int kGbdtPackedCell = 8;       // bytes per (feature, bin) in LDS: [16][256] cells are 32 KiB, five workgroups per compute unit
inline int gbdt_packed_flush_rows(int bound_g, int bound_h) {
    const int b = 2 * bound_g > bound_h ? 2 * bound_g : bound_h;
    return ((1 << (kGbdtPackedBits - 1)) - 1) / (b > 0 ? b : 1);
}
// the form of ptr_gbdt_histogram with the packed tile's LDS bytes, and rows per flush R
struct GbdtPackedForm { int kind; int tile; int tiles; int chunks; int lds_bytes; int flush_rows; };
inline GbdtPackedForm gbdt_hist_packed_form(int64_t m, int F, int max_bin, int bound_g, int bound_h) {
    const GbdtHistForm f = gbdt_hist_form(m, F, max_bin);
    return {f.kind, f.tile, f.tiles, f.chunks, f.kind == 2 ? kGbdtTile * max_bin * kGbdtPackedCell : 0, gbdt_packed_flush_rows(bound_g, bound_h)};
}
// the form of ptr_gbdt_histogram_segments likewise (at most two launches per call, as there)
struct GbdtSegPackedForm { int kind; int tile; int tiles; int chunks; int lds_bytes; int chunk_rows; int direct_rows; int flush_rows; };
inline GbdtSegPackedForm gbdt_hist_segments_packed_form(int64_t m, int F, int max_bin, int64_t total, int bound_g, int bound_h) {
    const GbdtSegForm f = gbdt_hist_segments_form(m, F, max_bin, total);
    return {f.kind, f.tile, f.tiles, f.chunks, f.kind == 2 ? kGbdtTile * max_bin * kGbdtPackedCell : 0, f.chunk_rows, f.direct_rows,
            gbdt_packed_flush_rows(bound_g, bound_h)};
}

// The per-leaf sums over the grower's row list (ptr_gbdt_leaf_sums_rows): grid = (nleaves, parts).  The workgroup (l, p) sums the entries
// offsets[l] + p * kLeafRowsChunk .. of leaf l, striding by parts * kLeafRowsChunk, in registers, reduces over its wavefronts and adds the
// three totals with one global integer atomic each; a workgroup without an entry leaves at once.  parts grows with the list so that a
// leaf of every row is still spread over kLeafRowsMaxParts workgroups.
constexpr int kLeafRowsChunk = 2048;     // consecutive entries of a leaf that one workgroup takes per step
constexpr int kLeafRowsMaxParts = 64;    // workgroups per leaf at the most
struct GbdtLeafRowsForm { int block; int parts; int chunk_rows; };
inline GbdtLeafRowsForm gbdt_leaf_sums_rows_form(int64_t total, int64_t nleaves) {
    if (total <= 0 || nleaves <= 0) return {kBlock, 0, kLeafRowsChunk};
    const int64_t want = (total + kLeafRowsChunk - 1) / kLeafRowsChunk;
    return {kBlock, (int)(want < kLeafRowsMaxParts ? want : kLeafRowsMaxParts), kLeafRowsChunk};
}

constexpr int kGbdtPartRows = 1024;      // consecutive entries of a row list that one workgroup of the partition owns

// The exact k-th largest |g h| of GOSS (ptr_gbdt_goss): a radix select over the keys' uint32 bit patterns, most significant digit first.
constexpr int kGossPasses = 3;           // digits of 11, 11 and 10 bits (shifts 21, 10, 0)
constexpr int kGossDigits = 2048;        // counters per pass: 8 KiB of LDS per workgroup, one global table per pass
constexpr int kGossRowsPerGroup = 4096;  // least rows per workgroup of a counting pass
constexpr int kGossMaxGroups = 2048;     // workgroups of one counting pass at the most (256 compute units x 8)
constexpr int kGossState = 4;            // int32 after the three tables: reserved for the select

// passes, digits per pass, workgroups of one counting pass (and of the apply pass), launches of one call (a memset, 3 counts, the apply)
struct GbdtGossForm { int passes; int digits; int groups; int launches; };
inline GbdtGossForm gbdt_goss_form(int64_t n) {
    if (n <= 0) return {kGossPasses, kGossDigits, 0, 0};
    const int64_t want = (n + kGossRowsPerGroup - 1) / kGossRowsPerGroup;
    return {kGossPasses, kGossDigits, (int)(want < kGossMaxGroups ? want : kGossMaxGroups), 2 + kGossPasses};
}

// The per-leaf sums of refit (ptr_gbdt_leaf_sums): one tree, n rows, nleaves cells of (sum qg, sum qh, count).
// LDS budget: a cell is (int64, int64, uint32) = 20 bytes, as in the histogram tile, and a workgroup keeps at most kLeafSumsLdsLeaves of them:
// 20 KiB.  Eight workgroups of 256 threads are the 32 waves a compute unit holds, and 8 x 20 KiB = 160 KiB is its whole LDS, so the budget
// never costs a wave; it is 4 to 30 times the leaves of a tree people train (31 .. 255).  The walk is a chain of dependent loads, so waves in
// flight are what hide its latency: 256 threads, one row each per step, and a workgroup takes at least kLeafSumsRows rows so that zeroing
// and flushing nleaves cells is paid once per 1024 walks.  The grid stops at kLeafSumsMaxGroups = 256 compute units x 4 and strides beyond.
constexpr int kLeafSumsLdsLeaves = 1024; // most leaves a workgroup sums in LDS; a tree of more adds straight into global memory
constexpr int kLeafSumsRows = 1024;      // least rows per workgroup
constexpr int kLeafSumsMaxGroups = 1024; // workgroups of one launch at the most

// kind 0: nothing to launch (n == 0); 1: LDS cells, the non-zero ones flushed with one global atomic per value; 2: global integer atomics
// per row (nleaves == 0 too: every row is lost and nothing is added).  groups: the workgroups of the launch; lds_bytes: what one of them
// declares; lds_leaves: the budget.
struct GbdtLeafSumsForm { int kind; int block; int groups; int lds_bytes; int lds_leaves; };
inline GbdtLeafSumsForm gbdt_leaf_sums_form(int64_t n, int64_t nleaves) {
    if (n <= 0) return {0, kBlock, 0, 0, kLeafSumsLdsLeaves};
    const int64_t want = (n + kLeafSumsRows - 1) / kLeafSumsRows;
    const int groups = (int)(want < kLeafSumsMaxGroups ? want : kLeafSumsMaxGroups);
    if (nleaves > 0 && nleaves <= kLeafSumsLdsLeaves) return {1, kBlock, groups, (int)nleaves * 20, kLeafSumsLdsLeaves};
    return {2, kBlock, groups, 0, kLeafSumsLdsLeaves};
}

// The forest walk of DART (ptr_gbdt_dart_walk, csrc/gbdt_dart.hip): a workgroup of 256 threads takes 256 consecutive rows through every
// listed tree.  LDS budget, per workgroup:
//   trees   two buffers (the tree walked and the next one, fetched meanwhile) of kDartLdsNodes packed nodes of 8 bytes and
//           kDartLdsNodes + 1 leaf values of 4 bytes: 2 x (4088 + 2048) = 12 272 bytes, declared as kDartTreeBytes = 2 x 6144 = 12 KiB.  511
//           nodes are the 512 leaves above everything people train with (31 .. 255) and above the reference's own grid (400);
//   rows    the tile form keeps the 256 rows' bins at a pitch of stride + 4 bytes: 256 x 148 = 37 888 bytes at the 136 features of MSLR.
// A compute unit has 160 KiB: at 136 features a workgroup declares 37 888 + 12 288 = 50 176 bytes, so three fit (150 528 bytes): 12 of the
// 32 waves a compute unit holds.  The walk is a chain of dependent LDS reads (node, bin, node, ...), which those waves hide among
// themselves; at 64 features (17 408 + 12 288 bytes) five fit.  kDartTileBytes = 40 KiB caps the tile where a third workgroup still fits
// (3 x (40 960 + 12 288) = 159 744 <= 163 840): stride <= 144.  Beyond it the direct form reads the bins from global memory, one byte
// per node at a random offset, and declares the trees' 12 KiB alone.  This arithmetic is a design estimate, not a measurement: what was
// measured is in profiles/mi355x_gbdt_dart.json.
constexpr int kDartLdsNodes = 511;       // most nodes of a tree that is walked from LDS; a larger tree is walked from global memory
constexpr int kDartTreeBytes = 2 * 6144; // the two tree buffers
constexpr int kDartTileBytes = 40 * 1024;   // most bytes of the row tile; a wider matrix takes the direct form
constexpr int kDartMaxFeatures = 65535;  // a packed node keeps its feature in 16 bits
constexpr int kDartMaxNodes = 32767;     // and its children in int16: at most 32 768 leaves

// kind 0: nothing to launch (n == 0); 1: tile (the rows' bins in LDS); 2: direct (bins from global memory).  groups: the workgroups;
// lds_bytes: what one declares; lds_nodes: kDartLdsNodes; staged: 1 where a tree of max_nodes nodes is walked from LDS, 0 from global memory.
struct GbdtDartForm { int kind; int block; int groups; int lds_bytes; int lds_nodes; int staged; };
inline GbdtDartForm gbdt_dart_walk_form_of_stride(int64_t n, int64_t stride, int64_t max_nodes) {      // what the launcher asks, with the matrix's own stride
    const int staged = max_nodes <= kDartLdsNodes ? 1 : 0;
    if (n <= 0) return {0, kBlock, 0, 0, kDartLdsNodes, staged};
    const int groups = (int)((n + kBlock - 1) / kBlock);
    const int64_t tile = (int64_t)kBlock * (stride + 4);
    if (tile <= kDartTileBytes) return {1, kBlock, groups, (int)tile + kDartTreeBytes, kDartLdsNodes, staged};
    return {2, kBlock, groups, kDartTreeBytes, kDartLdsNodes, staged};
}
inline GbdtDartForm gbdt_dart_walk_form(int64_t n, int F, int64_t max_nodes) {                      // for the stride ptr_gbdt_bin gives F features
    return gbdt_dart_walk_form_of_stride(n, (int64_t)(F + kGbdtTile - 1) / kGbdtTile * kGbdtTile, max_nodes);
}

#if defined(__HIPCC__)
// Inclusive sums of one value per thread over the workgroup's kBlock threads, through buf [kBlock] in LDS.  A thread's last access to buf
// is to its own entry, behind a barrier: the next call may use the same buf at once.
template <class T> __device__ __forceinline__ T block_scan_add(T *buf, T v) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const T o = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += o;
        __syncthreads();
    }
    return buf[t];
}

constexpr int kSetWords = 4;             // a left set: 256 bits, bit b in word b / 64

// One row's walk down a tree of nn nodes (nn + 1 leaves; a child c < 0 is the leaf ~c) -> the node it ends in.  goes_left(node, f) decides at
// a node that splits on feature f, which the walk has checked against F.  The walk takes nn steps at the most and stops at an index out of
// range, so a malformed tree (a cycle, a node or feature out of range) ends it on something gbdt_is_leaf rejects.
template <class GoesLeft> __device__ __forceinline__ int gbdt_walk(int nn, int F, const int32_t *__restrict__ feature, const int32_t *__restrict__ left,
                                                                   const int32_t *__restrict__ right, const GoesLeft &goes_left) {
    int node = nn > 0 ? 0 : ~0;
    for (int step = 0; step < nn && node >= 0; ++step) {
        if (node >= nn) break;
        const int f = feature[node];
        if (f < 0 || f >= F) break;
        node = goes_left(node, f) ? left[node] : right[node];
    }
    return node;
}
__device__ __forceinline__ bool gbdt_is_leaf(int node, int nn) { return node < 0 && ~node <= nn; }

// The categorical nodes of a walk (the *_cat entry points): cat_index [nodes] is -1 at a numeric node, else the node's left set
// cat_sets[cat_index] (kSetWords int64 each, ncat of them).  The tables are device memory and read as untrusted: an index at or past ncat,
// or a node whose kind is not its feature's (is_cat [F]), is a malformed tree: -2, which the walks turn into NaN.
struct GbdtCatWalk { const uint8_t *is_cat; const int32_t *cat_index; const int64_t *cat_sets; int ncat; };
__device__ __forceinline__ int gbdt_cat_node(const GbdtCatWalk &c, int node, int f) {
    const int ci = c.cat_index[node];
    const bool isc = c.is_cat[f] != 0;
    if (ci < 0) return isc ? -2 : -1;
    return isc && ci < c.ncat ? ci : -2;
}
__device__ __forceinline__ bool gbdt_in_set(const int64_t *__restrict__ set, int b) { return (((unsigned long long)set[b >> 6]) >> (b & 63)) & 1ull; }     // b in 0 .. 255

// How a raw value decides at node `at` (an index over the nodes of ALL trees) that splits on feature f: the one predicate of every walk over
// raw rows (prediction, the leaf counts and the one fractions of TreeSHAP).  bad: a malformed categorical table.
template <bool kCat> __device__ __forceinline__ bool gbdt_raw_goes_left(float xv, int at, int f, const float *__restrict__ threshold,
                                                                        const uint8_t *__restrict__ default_left, const GbdtCatWalk &cat, bool &bad) {
    if constexpr (kCat) {
        const int ci = gbdt_cat_node(cat, at, f);
        if (ci == -2) { bad = true; return false; }
        if (ci >= 0) {                                                  // a NaN follows the node's direction; what is no code 0 .. 255 is in no set
            if (xv != xv) return default_left && default_left[at] != 0;
            if (!(xv >= 0.0f && xv <= 255.0f)) return false;
            const int c = (int)xv;
            return (float)c == xv && gbdt_in_set(cat.cat_sets + (int64_t)ci * kSetWords, c);
        }
    }
    return (default_left && xv != xv) ? default_left[at] != 0 : xv <= threshold[at];       // a NaN follows the node's direction
}
#endif

}  // namespace ptr
