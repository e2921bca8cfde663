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

}  // namespace ptr
