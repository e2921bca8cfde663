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

}  // namespace ptr
