// A histogram gradient-boosted tree trainer on the device: binning, fixed-point gradients, per-leaf histograms, the split scan, the stable
// row partition, the leaf-value update and prediction, and the batched forms of one level of a depth-wise tree (histograms, subtraction,
// split scan and partition over many leaves per call).  ptranking_amd/gbdt.py grows the trees leaf-wise or depth-wise on these entry points; the
// reference's tree frame (ptranking/ltr_tree/lambdamart/lightgbm_lambdaMART.py) hands this work to LightGBM.
//
// Why fixed point.  ptr_gbdt_quantize scales a round's gradients and Hessians by a power of two so that the largest magnitude lies just
// below 2^30 and rounds them to int32.  Every histogram sum is then an int64 sum of int32 terms, and integer addition is associative: the
// bits of a histogram do not depend on the row order, the number of workgroups, how a leaf's rows are chunked, or whether the histogram
// was built from rows or by subtracting a sibling from its parent.  The kernels use integer atomics only (LDS and global); there is no
// float atomic in this file.  An int64 sum holds 2^33 rows at the extreme; the split scan turns sums into float64 exactly up to 2^53,
// that is 2^23 rows with every gradient at the extreme.
//
// Layouts.  bins [n][stride] uint8, row-major, stride = round_up(F, 16), pad bytes 0: the 16 features of a tile are one 16-byte load of
// a row.  hist [F][max_bin][3] int64: sum qg, sum qh, count.  Split records: 9 int64 (include/ptranking_amd.h).
//
// Histogram forms (gbdt_hist_form, ptr_gbdt.h):
//   direct   m <= 256 rows: one thread per (row, feature) adds into global memory; a small leaf touches few bins, zeroing and flushing a
//            tile would cost more than the adds;
//   LDS      grid = row chunks x feature tiles of 16.  A workgroup keeps [16][max_bin] of (int64, int64, int32) in LDS (20 bytes per
//            entry, 80 KiB at 256 bins: two workgroups per compute unit), each lane loads one row's 16 bins as a uint4 and its qg, qh once,
//            and walks the 16 features ROTATED by its lane number: in one step the 64 lanes address 16 different features, so a constant
//            feature (every row in one bin) meets 4 lanes per address and step, not 64.  The flush adds only the bins the chunk touched.
//
// One body per step.  The single-list and the batched (segment) kernels of a step differ only in how a workgroup finds its rows and its
// destination; the work is a device function both call: gbdt_hist_tile (the LDS tile: zero, rotated walk, flush), hist_add_direct,
// part_count and part_scatter under a predicate (PartByBin, PartByMask; a batched workgroup builds a PartByBin over its segment), one scan
// kernel for both partitions on block_scan_add (goss_pick scans with it too), and gbdt_walk, to which the raw predictor and the binned walk
// pass their comparison.
//
// Row sampling (bagging by row or by query, GOSS): a keep mask of one byte per row, the stable partition under the predicate mask[row], and
// a walk of the finished tree over the binned rows outside the bag.  GOSS's threshold is the exact K-th largest |g h|: the keys are
// non-negative floats, their uint32 bit patterns order as integers, and a radix select of three counting passes (digits of 11, 11 and 10
// bits; LDS counters flushed with one integer atomic per touched digit) finds it without sorting and without a float atomic.  Each pass
// starts by reading the finished table of the pass before, in every workgroup alike, so no launch exists only to pick a digit.
//
// Missing values (the *_missing entry points; use_missing=True of gbdt.py): a feature's NaNs sit in one more bin behind its value bins, so
// the histogram layout and the histogram kernels are the same.  The split scan is a template on "missing" (one prefix pass, the second
// direction behind a wave-uniform test), both stable partitions and the binned walk take one more bin that goes left (also_left, -1: none)
// and the raw predictor a default_left byte per node; each older entry point passes "no missing" and computes what it computed.
//
// Monotone and interaction constraints (the *_cst entry points; monotone_constraints, interaction_constraints of gbdt.py): training-time
// rules that live in the split scan alone.  The scan is a template on "constrained" as well: such a wavefront first reads its leaf's
// (lo, hi, v), its feature's sign and its permission from three small device tables (scalar loads: the item is wave-uniform), and every
// candidate then takes the bounded gain; the grower computes the children's rows of the tables on the host from the record it reads anyway.
//
// A trained model on new data (ptr_gbdt_predict_leaf, ptr_gbdt_leaf_sums, ptr_gbdt_add_by_leaf; predict(pred_leaf=True), refit and
// fit_bins(init_model=...) of gbdt.py): walks of raw rows through gbdt_walk under the predicate of the raw predictor, so every row lands where
// prediction puts it.  The leaf index per (row, tree) with nothing summed; for one tree the leaf per row and the integer sums (qg, qh, 1) per
// leaf, in LDS cells per workgroup up to kLeafSumsLdsLeaves leaves and straight into global memory beyond (gbdt_leaf_sums_form, ptr_gbdt.h,
// gives the budget and why); and scores[r] += values[leaf[r]].  Integer atomics only, as everywhere in this file.
#include <math.h>

#include "ptr_gbdt.h"
#include "ptr_plhash.h"

namespace ptr {

using u64 = unsigned long long;
constexpr int kRec = 9;                  // int64 values of a split record

// ---------------------------------------------------------------- binning
__global__ void __launch_bounds__(kBlock)
gbdt_bin_kernel(const float *__restrict__ X, int64_t n, int F, const float *__restrict__ edges, const int32_t *__restrict__ nbins,
                const int32_t *__restrict__ nan_bin, int max_bin, int stride, uint8_t *__restrict__ bins) {
    const int64_t total = n * stride;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t row = e / stride;
        const int f = (int)(e - row * stride);
        int b = 0;
        if (f < F) {
            const float x = X[row * F + f];
            const float *ed = edges + (size_t)f * (max_bin - 1);
            int lo = 0, hi = min(max(nbins[f], 1), max_bin) - 1;          // the number of edges < x, by bisection over [0, nbins - 1)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (ed[mid] < x) lo = mid + 1; else hi = mid;
            }
            b = lo;
            if (nan_bin && x != x) {                                    // a missing value: the feature's NaN bin, where it has one (else 0, as the bisection gives)
                const int nb = nan_bin[f];
                if (nb >= 0 && nb < max_bin) b = nb;
            }
        }
        bins[e] = (uint8_t)b;
    }
}

// ---------------------------------------------------------------- quantization
// state[0], state[1]: the bit patterns of max|g| and max|h| (non-negative floats order as unsigned integers): an integer atomic max.
__global__ void __launch_bounds__(kBlock)
gbdt_absmax_kernel(const float *__restrict__ g, const float *__restrict__ h, int64_t n, uint32_t *__restrict__ state, int32_t *__restrict__ flag) {
    __shared__ uint32_t red[2];
    if (threadIdx.x < 2) red[threadIdx.x] = 0;
    __syncthreads();
    uint32_t mg = 0, mh = 0;
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const uint32_t a = __float_as_uint(g[i]) & 0x7fffffffu, b = __float_as_uint(h[i]) & 0x7fffffffu;
        if (a >= 0x7f800000u || b >= 0x7f800000u) bad = true;           // inf or NaN
        else { mg = max(mg, a); mh = max(mh, b); }
    }
    atomicMax(&red[0], mg);
    atomicMax(&red[1], mh);
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, 1);
    if (threadIdx.x == 0) { atomicMax(&state[0], red[0]); atomicMax(&state[1], red[1]); }
}

// the largest e with m 2^e < 2^30: m = fr 2^ex with fr in [0.5, 1), so e = 30 - ex; 0 for m == 0
__device__ __forceinline__ int gbdt_exponent(uint32_t bits) {
    if (bits == 0) return 0;
    int ex;
    (void)frexpf(__uint_as_float(bits), &ex);
    return 30 - ex;
}

__global__ void __launch_bounds__(kBlock)
gbdt_quantize_kernel(const float *__restrict__ g, const float *__restrict__ h, int64_t n, const uint32_t *__restrict__ state,
                     int32_t *__restrict__ qg, int32_t *__restrict__ qh, int32_t *__restrict__ expo) {
    const int eg = gbdt_exponent(state[0]), eh = gbdt_exponent(state[1]);
    if (blockIdx.x == 0 && threadIdx.x == 0) { expo[0] = eg; expo[1] = eh; }
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const float a = g[i], b = h[i];
        const bool fin = (__float_as_uint(a) & 0x7fffffffu) < 0x7f800000u && (__float_as_uint(b) & 0x7fffffffu) < 0x7f800000u;
        qg[i] = fin ? (int32_t)rintf(ldexpf(a, eg)) : 0;                // a non-finite entry raised the flag; its row carries nothing
        qh[i] = fin ? (int32_t)rintf(ldexpf(b, eh)) : 0;
    }
}

// ---------------------------------------------------------------- histograms
__device__ __forceinline__ void hist_add_global(int64_t *__restrict__ cell, int64_t g, int64_t h, int64_t c) {
    atomicAdd(reinterpret_cast<u64 *>(cell), (u64)g);
    atomicAdd(reinterpret_cast<u64 *>(cell + 1), (u64)h);
    atomicAdd(reinterpret_cast<u64 *>(cell + 2), (u64)c);
}

// The direct form's add of one (row, feature): a feature in the stride's padding, a row outside the matrix or a bin outside the histogram adds nothing.
__device__ __forceinline__ void hist_add_direct(const uint8_t *__restrict__ bins, int stride, int n, const int32_t *__restrict__ qg,
                                                const int32_t *__restrict__ qh, int row, int f, int F, int max_bin, int64_t *__restrict__ hist) {
    if (f >= F || row < 0 || row >= n) return;
    const int b = bins[(size_t)row * stride + f];
    if (b >= max_bin) return;
    hist_add_global(hist + ((size_t)f * max_bin + b) * 3, qg[row], qh[row], 1);
}

__global__ void __launch_bounds__(kBlock)
gbdt_hist_direct_kernel(const uint8_t *__restrict__ bins, int stride, int n, const int32_t *__restrict__ qg, const int32_t *__restrict__ qh,
                        const int32_t *__restrict__ rows, int m, int F, int max_bin, int64_t *__restrict__ hist) {
    const int e = blockIdx.x * kBlock + threadIdx.x;                    // m <= kGbdtDirectRows: m * stride fits an int
    if (e >= m * stride) return;
    const int i = e / stride, f = e - i * stride;
    hist_add_direct(bins, stride, n, qg, qh, rows ? rows[i] : i, f, F, max_bin, hist);
}

// The LDS form of one workgroup: zeroes its tile [kGbdtTile][max_bin] of (int64, int64, int32) at `smem`, adds the entries [r0, r1) of the row
// list (rows == NULL: the rows r0 .. r1 - 1 themselves) for the feature tile blockIdx.y, and flushes the bins it touched into hist
// [F][max_bin][3].  Every thread of the workgroup calls it.
__device__ __forceinline__ void gbdt_hist_tile(unsigned char *smem, const uint8_t *__restrict__ bins, int stride, int n, const int32_t *__restrict__ qg,
                                               const int32_t *__restrict__ qh, const int32_t *__restrict__ rows, int64_t r0, int64_t r1, int F,
                                               int max_bin, int64_t *__restrict__ hist) {
    const int cells = kGbdtTile * max_bin;
    u64 *lg = reinterpret_cast<u64 *>(smem), *lh = lg + cells;
    uint32_t *lc = reinterpret_cast<uint32_t *>(lh + cells);
    const int tid = threadIdx.x, f0 = blockIdx.y * kGbdtTile;
    for (int e = tid; e < cells; e += kBlock) { lg[e] = 0; lh[e] = 0; lc[e] = 0; }
    __syncthreads();
    const int nf = min(kGbdtTile, F - f0);
    for (int64_t i = r0 + tid; i < r1; i += kBlock) {
        const int row = rows ? rows[i] : (int)i;
        if (row < 0 || row >= n) continue;
        const uint4 bv = *reinterpret_cast<const uint4 *>(bins + (size_t)row * stride + f0);
        const u64 g = (u64)(int64_t)qg[row], h = (u64)(int64_t)qh[row];
#pragma unroll
        for (int k = 0; k < kGbdtTile; ++k) {
            const int f = (k + tid) & (kGbdtTile - 1);
            const uint32_t w = (f >> 2) == 0 ? bv.x : (f >> 2) == 1 ? bv.y : (f >> 2) == 2 ? bv.z : bv.w;
            const int b = (w >> ((f & 3) * 8)) & 0xff;
            if (f < nf && b < max_bin) {
                const int c = f * max_bin + b;
                atomicAdd(&lg[c], g);
                atomicAdd(&lh[c], h);
                atomicAdd(&lc[c], 1u);
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < nf * max_bin; e += kBlock) {
        const uint32_t c = lc[e];
        if (c) hist_add_global(hist + ((size_t)f0 * max_bin + e) * 3, (int64_t)lg[e], (int64_t)lh[e], (int64_t)c);
    }
}

__global__ void __launch_bounds__(kBlock)
gbdt_hist_lds_kernel(const uint8_t *__restrict__ bins, int stride, int n, const int32_t *__restrict__ qg, const int32_t *__restrict__ qh,
                     const int32_t *__restrict__ rows, int m, int F, int max_bin, int64_t *__restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gbdt_smem[];
    // this workgroup's rows: chunk c of gridDim.x, whole multiples of the block except the last
    const int per = (int)((((int64_t)m + gridDim.x - 1) / gridDim.x + kBlock - 1) / kBlock) * kBlock;
    const int64_t r0 = (int64_t)blockIdx.x * per;
    const int64_t r1 = r0 + per < (int64_t)m ? r0 + per : (int64_t)m;
    gbdt_hist_tile(gbdt_smem, bins, stride, n, qg, qh, rows, r0, r1, F, max_bin, hist);
}

__global__ void __launch_bounds__(kBlock)
gbdt_hist_sub_kernel(const int64_t *__restrict__ parent, const int64_t *__restrict__ child, int64_t count, int64_t *__restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < count; e += (int64_t)gridDim.x * kBlock) out[e] = parent[e] - child[e];
}

// ---------------------------------------------------------------- the split scan
template <class T> __device__ __forceinline__ T wave_scan_add(T v, int lane) {       // inclusive, over the 64 lanes
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

struct SplitCand { double gain; int bin; int64_t gl, hl, cl; };

// field 0 .. kRec - 1 of the record of a leaf without a split: gain -inf, feature and bin -1, no sums
__device__ __forceinline__ int64_t gbdt_no_split(int field) { return field == 0 ? __double_as_longlong(-INFINITY) : field <= 2 ? -1 : 0; }

// ---- monotone and interaction constraints (the *_cst entry points; monotone_constraints and interaction_constraints of gbdt.py).
// Three device tables, read as untrusted: mono [F] int8 (anything outside -1 .. 1 reads as 0), cst [leaves][3] float64 (lo, hi, v) or NULL
// (interaction constraints alone: today's gain), allowed [leaves][F] uint8 or NULL (every feature allowed).
struct GbdtCstArgs { const int8_t *mono; const double *cst; const uint8_t *allowed; };
// What one wavefront keeps of them: on (the bounded gain applies), the feature's sign, the leaf's bounds and its value v.  Under `on` the
// scan hands gbdt_split_gain the node's loss G * v where the unbounded gain takes the parent's term (one value live, not two).
struct GbdtBound { bool on; int sign; double lo, hi, v; };

// The gain of one candidate's left sums against the node's totals, or false where a validity rule rejects it.  kCst with bd.on: the
// bounded gain of include/ptranking_amd.h, vL = clamp(-GL / (HL + l2), lo, hi) and vR likewise, rejected where they break the feature's
// order, gain = ((G * v) - (GL * vL)) - (GR * vR).
template <bool kCst>
__device__ __forceinline__ bool gbdt_split_gain(int64_t gl, int64_t hl, int64_t cl, int64_t TG, int64_t TH, int64_t TC, int eg, int eh, double l2,
                                                int64_t min_data, double floor_h, double min_gain, double parent, double &gain, const GbdtBound &bd) {
    const int64_t cr = TC - cl;
    if (cl < min_data || cr < min_data) return false;
    const double GL = ldexp((double)gl, -eg), HL = ldexp((double)hl, -eh);
    const double GR = ldexp((double)(TG - gl), -eg), HR = ldexp((double)(TH - hl), -eh);
    if (!(HL >= floor_h) || !(HR >= floor_h)) return false;
    if (kCst && bd.on) {
        const double vl = fmin(fmax(-GL / (HL + l2), bd.lo), bd.hi), vr = fmin(fmax(-GR / (HR + l2), bd.lo), bd.hi);
        if ((bd.sign > 0 && vl > vr) || (bd.sign < 0 && vl < vr)) return false;
        gain = ((parent - (GL * vl)) - (GR * vr));
    } else {
        gain = ((GL * GL) / (HL + l2) + (GR * GR) / (HR + l2)) - parent;
    }
    return gain >= min_gain;
}

// One wavefront per (leaf, feature): lane t owns the bins 4 t .. 4 t + 3, one prefix pass.  Writes the feature's best candidate to ws.
// All arithmetic is float64 and nothing is contracted (the library is built with -ffp-contract=off):
//   gain = ((GL * GL) / (HL + l2) + (GR * GR) / (HR + l2)) - (G * G) / (H + l2),   G = (double)qsum * 2^-e_g, H likewise (both exact).
// (the scan itself is gbdt_split_scan, shared with the slot-list form of the batched level pass)
//
// kMissing (the *_missing entry points): the feature's NaN bin nan_bin[f] (a bin at or behind the value bins; anything else reads as "none")
// holds the node's missing rows (MG, MH, MC), which the totals include.  The candidates b < nb - 1 send the missing rows right; where
// MC > 0 the candidate b = nb - 1 (every value left, the NaNs right) joins them, and every b < nb - 1 is evaluated a second time with the
// missing rows on the left, behind the wave-uniform test MC > 0.  A candidate's order key is b with the missing rows right and 511 - b
// with them left, and the lowest key wins a tie: missing-right before missing-left, then the lowest bin among the missing-right candidates
// and the HIGHEST among the missing-left ones (scikit-learn scans those from the top bin down and keeps the first of equal gains; bins
// that are empty in a node make such ties bit-exact and common).  Field 2 of the record is bin + 256 * default_left; with MC == 0
// default_left = (left count > right count).
template <bool kMissing, bool kCst>
__device__ __forceinline__ void gbdt_split_scan(const int64_t *__restrict__ hp, int f, int lane, int max_bin, const int32_t *__restrict__ nbins,
                                                const int32_t *__restrict__ nan_bin, const int32_t *__restrict__ expo, double l2, int64_t min_data,
                                                double min_hess, double min_gain, int64_t *__restrict__ r, GbdtBound bd) {
    const int nb = min(max(nbins[f], 1), max_bin);
    int64_t MG = 0, MH = 0, MC = 0;
    if (kMissing) {
        const int mbin = nan_bin[f];
        if (mbin >= nb && mbin < max_bin) { MG = hp[mbin * 3]; MH = hp[mbin * 3 + 1]; MC = hp[mbin * 3 + 2]; }
    }
    int64_t pg[4], ph[4], pc[4], sg = 0, sh = 0, sc = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = lane * 4 + k;
        if (b < nb) { sg += hp[b * 3]; sh += hp[b * 3 + 1]; sc += hp[b * 3 + 2]; }
        pg[k] = sg; ph[k] = sh; pc[k] = sc;
    }
    const int64_t ig = wave_scan_add(sg, lane) - sg, ih = wave_scan_add(sh, lane) - sh, ic = wave_scan_add(sc, lane) - sc;
    const int64_t TG = __shfl(ig + sg, kWave - 1) + MG, TH = __shfl(ih + sh, kWave - 1) + MH, TC = __shfl(ic + sc, kWave - 1) + MC;
    const int eg = expo[0], eh = expo[1];
    const double G = ldexp((double)TG, -eg), H = ldexp((double)TH, -eh);
    const double parent = (kCst && bd.on) ? G * bd.v : (G * G) / (H + l2);
    const double floor_h = fmax(min_hess, 0x1p-40);
    SplitCand best{-INFINITY, -1, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = lane * 4 + k;
        if (b >= nb - 1 && !(kMissing && MC > 0 && b == nb - 1)) continue;   // the last bin leaves nothing on the right, unless the NaNs are there
        const int64_t gl = ig + pg[k], hl = ih + ph[k], cl = ic + pc[k];
        double gain;
        if (gbdt_split_gain<kCst>(gl, hl, cl, TG, TH, TC, eg, eh, l2, min_data, floor_h, min_gain, parent, gain, bd) &&
            (gain > best.gain || (kMissing && gain == best.gain && b < best.bin)))
            best = SplitCand{gain, b, gl, hl, cl};                       // ascending bins: a tie keeps the lowest (and beats any missing-left key)
        if (kMissing && MC > 0 && b < nb - 1 &&
            gbdt_split_gain<kCst>(gl + MG, hl + MH, cl + MC, TG, TH, TC, eg, eh, l2, min_data, floor_h, min_gain, parent, gain, bd) &&
            (gain > best.gain || (gain == best.gain && 511 - b < best.bin)))
            best = SplitCand{gain, 511 - b, gl + MG, hl + MH, cl + MC};   // a tie among missing-left candidates keeps the highest bin
    }
    // the wave's best: highest gain, then lowest bin
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const double og = __shfl_xor(best.gain, d);
        const int ob = __shfl_xor(best.bin, d);
        const int64_t o1 = __shfl_xor(best.gl, d), o2 = __shfl_xor(best.hl, d), o3 = __shfl_xor(best.cl, d);
        if (ob >= 0 && (best.bin < 0 || og > best.gain || (og == best.gain && ob < best.bin))) best = SplitCand{og, ob, o1, o2, o3};
    }
    if (lane == 0) {
        const bool ok = best.bin >= 0;
        r[0] = __double_as_longlong(ok ? best.gain : -INFINITY);
        r[1] = ok ? f : -1;
        if (kMissing && ok) {
            const bool mleft = best.bin >= 256;
            const int64_t dl = MC > 0 ? (mleft ? 1 : 0) : (best.cl > TC - best.cl ? 1 : 0);
            r[2] = (mleft ? 511 - best.bin : best.bin) + 256 * dl;
        } else {
            r[2] = best.bin;
        }
        r[3] = best.gl; r[4] = best.hl; r[5] = best.cl;
        r[6] = ok ? TG - best.gl : 0; r[7] = ok ? TH - best.hl : 0; r[8] = ok ? TC - best.cl : 0;
    }
}

// ---- categorical features (the *_cat entry points; categorical_feature of gbdt.py): a split sends a SET of bins left.
constexpr int kSetWords = 4;             // a left set: 256 bits, bit b in word b / 64
constexpr int kCatSorted = 3 * PTR_GBDT_MAX_BIN;   // int64 of LDS per wavefront: (G, H, C) of up to 256 categories in sorted order (6 KiB)

// lane `src` (wave-uniform) of a double, through two v_readlane
__device__ __forceinline__ double wave_read(double v, int src) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, src), hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
    return __longlong_as_double((long long)(((u64)(uint32_t)hi << 32) | (uint32_t)lo));
}

struct GbdtCatArgs { const uint8_t *is_cat; double cat_smooth; int64_t *sets; };      // sets [items][kSetWords], beside the records

// The scan of one categorical feature (include/ptranking_amd.h states the rule, tests/gbdt_cat_ref.py restates it).  Lane t owns the bins
// 4 t .. 4 t + 3 as categories: the value bins below nbins[f] and, where nan_bin names one, the NaN bin.  A category is used iff it holds
// rows, H_c (TC / TH) >= cat_smooth and its key v_c = G_c / (H_c + cat_smooth) is a number; an unused one carries the key NaN, which no
// comparison counts.  The rank of a used category is the number of used ones ahead of it under (key, bin): every lane's four keys are
// broadcast in turn (v_readlane; up to 256 rounds of 4 comparisons) — no sort network, and the order is total, so the ranks are a
// permutation of 0 .. u - 1 whatever the keys.  The sums go to LDS at their rank and come back by position, lane t owning the sorted
// positions 4 t .. 4 t + 3; one wave_scan_add pass then serves both directions: the left sums of "the first p + 1" are the prefix P[p], those
// of "the last i + 1" the used total minus P[u - 2 - i].  A candidate's order key is i left to right and 256 + i right to left (i + 1
// categories go left): the lowest key wins a tie, as in the numeric scan.  The winner's set is built from the ranks: a nibble per lane,
// OR-ed over each group of 16 lanes into one 64-bit word, stored by the lanes 0, 16, 32 and 48.
template <bool kCst>
__device__ __forceinline__ void gbdt_split_scan_cat(const int64_t *__restrict__ hp, int f, int lane, int max_bin, const int32_t *__restrict__ nbins,
                                                    const int32_t *__restrict__ nan_bin, const int32_t *__restrict__ expo, double l2, int64_t min_data,
                                                    double min_hess, double min_gain, double cat_smooth, int64_t *sorted, int64_t *__restrict__ r,
                                                    int64_t *__restrict__ set, GbdtBound bd) {
    const int nb = min(max(nbins[f], 1), max_bin);
    int mbin = nan_bin ? nan_bin[f] : -1;
    if (mbin < nb || mbin >= max_bin) mbin = -1;
    const int span = mbin >= 0 ? mbin + 1 : nb;                         // no category at or behind this bin
    int64_t cg[4], ch[4], cc[4], sg = 0, sh = 0, sc = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int b = lane * 4 + k;
        const bool is = b < nb || b == mbin;
        cg[k] = is ? hp[b * 3] : 0; ch[k] = is ? hp[b * 3 + 1] : 0; cc[k] = is ? hp[b * 3 + 2] : 0;
        sg += cg[k]; sh += ch[k]; sc += cc[k];
    }
    const int64_t TG = __shfl(wave_scan_add(sg, lane), kWave - 1), TH = __shfl(wave_scan_add(sh, lane), kWave - 1),
                  TC = __shfl(wave_scan_add(sc, lane), kWave - 1);
    const int eg = expo[0], eh = expo[1];
    const double G = ldexp((double)TG, -eg), H = ldexp((double)TH, -eh);
    const double parent = (kCst && bd.on) ? G * bd.v : (G * G) / (H + l2);
    const double floor_h = fmax(min_hess, 0x1p-40);
    if (kCst) bd.sign = 0;                                              // a set split has no order to keep
    const double factor = (double)TC / H;
    double key[4];
    int u = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double Gc = ldexp((double)cg[k], -eg), Hc = ldexp((double)ch[k], -eh);
        const double v = Gc / (Hc + cat_smooth);
        const bool used = cc[k] > 0 && Hc * factor >= cat_smooth && v == v;
        key[k] = used ? v : (double)NAN;
        u += __popcll(__ballot(used));
    }
    int rank[4] = {0, 0, 0, 0};
    const int nl = (span + 3) >> 2;                                     // the lanes that own a category: at most 64
    for (int s = 0; s < nl; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double ov = wave_read(key[j], s);
            const int ob = s * 4 + j;
#pragma unroll
            for (int k = 0; k < 4; ++k) rank[k] += (ov < key[k] || (ov == key[k] && ob < lane * 4 + k)) ? 1 : 0;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (key[k] == key[k]) {                                         // rank < the number of used categories <= 256: inside the wave's LDS
            sorted[rank[k]] = cg[k]; sorted[PTR_GBDT_MAX_BIN + rank[k]] = ch[k]; sorted[2 * PTR_GBDT_MAX_BIN + rank[k]] = cc[k];
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");              // the wave's own stores, read back by other lanes of the same wave
    __builtin_amdgcn_wave_barrier();
    int64_t pg[4], ph[4], pc[4];
    sg = sh = sc = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = lane * 4 + k;
        if (p < u) { sg += sorted[p]; sh += sorted[PTR_GBDT_MAX_BIN + p]; sc += sorted[2 * PTR_GBDT_MAX_BIN + p]; }
        pg[k] = sg; ph[k] = sh; pc[k] = sc;
    }
    const int64_t ig = wave_scan_add(sg, lane) - sg, ih = wave_scan_add(sh, lane) - sh, ic = wave_scan_add(sc, lane) - sc;
    const int64_t UG = __shfl(ig + sg, kWave - 1), UH = __shfl(ih + sh, kWave - 1), UC = __shfl(ic + sc, kWave - 1);
    const int mid = (u + 1) >> 1;
    SplitCand best{-INFINITY, -1, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = lane * 4 + k;
        if (u <= 1 || p >= u) continue;
        const int64_t gl = ig + pg[k], hl = ih + ph[k], cl = ic + pc[k];
        double gain;
        if (p < mid && gbdt_split_gain<kCst>(gl, hl, cl, TG, TH, TC, eg, eh, l2, min_data, floor_h, min_gain, parent, gain, bd) &&
            (gain > best.gain || (gain == best.gain && p < best.bin)))
            best = SplitCand{gain, p, gl, hl, cl};                       // left to right: the first p + 1 sorted categories
        const int i = u - 2 - p;                                        // right to left: the last i + 1, for i = 0 .. mid - 2
        if (i >= 0 && i <= mid - 2 &&
            gbdt_split_gain<kCst>(UG - gl, UH - hl, UC - cl, TG, TH, TC, eg, eh, l2, min_data, floor_h, min_gain, parent, gain, bd) &&
            (gain > best.gain || (gain == best.gain && 256 + i < best.bin)))
            best = SplitCand{gain, 256 + i, UG - gl, UH - hl, UC - cl};
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const double og = __shfl_xor(best.gain, d);
        const int ob = __shfl_xor(best.bin, d);
        const int64_t o1 = __shfl_xor(best.gl, d), o2 = __shfl_xor(best.hl, d), o3 = __shfl_xor(best.cl, d);
        if (ob >= 0 && (best.bin < 0 || og > best.gain || (og == best.gain && ob < best.bin))) best = SplitCand{og, ob, o1, o2, o3};
    }
    const bool ok = best.bin >= 0;                                      // the same in every lane: the order of the candidates is total
    const int rtl = best.bin >> 8, i = best.bin & 255;
    uint32_t nib = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool in = ok && key[k] == key[k] && (rtl ? rank[k] >= u - 1 - i : rank[k] <= i);
        nib |= (in ? 1u : 0u) << k;
    }
    u64 word = (u64)nib << ((lane & 15) * 4);
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) word |= __shfl_xor(word, d);
    if ((lane & 15) == 0) set[lane >> 4] = (int64_t)word;
    const int dl = mbin >= 0 ? (int)((__shfl(nib, mbin >> 2) >> (mbin & 3)) & 1u) : 0;      // the NaN bin's bit
    if (lane == 0) {
        r[0] = __double_as_longlong(ok ? best.gain : -INFINITY);
        r[1] = ok ? f : -1;
        r[2] = ok ? (i + 1) + 256 * dl : -1;
        r[3] = best.gl; r[4] = best.hl; r[5] = best.cl;
        r[6] = ok ? TG - best.gl : 0; r[7] = ok ? TH - best.hl : 0; r[8] = ok ? TC - best.cl : 0;
    }
}

// What the constrained scan reads for the wavefront of (leaf, f), all of it wave-uniform -> false where the wavefront has nothing to
// search: the feature is not allowed at the leaf, or the leaf's bounds are no interval (a NaN among lo, hi, v, or lo > hi).
// The wavefront's leaf and feature pass through v_readfirstlane, so the table reads are scalar loads and the bounds stay out of the VGPRs.
__device__ __forceinline__ bool gbdt_cst_bound(const GbdtCstArgs &cs, int64_t leaf_v, int f_v, int F, GbdtBound &bd) {
    const int64_t leaf = __builtin_amdgcn_readfirstlane((int)leaf_v);     // below nleaf (K), an int
    const int f = __builtin_amdgcn_readfirstlane(f_v);
    bd = GbdtBound{false, 0, 0.0, 0.0, 0.0};
    if (cs.allowed && !cs.allowed[leaf * F + f]) return false;
    if (!cs.cst) return true;
    const double lo = cs.cst[leaf * 3], hi = cs.cst[leaf * 3 + 1], v = cs.cst[leaf * 3 + 2];
    if (!(lo <= hi) || v != v) return false;
    const int m = cs.mono[f];
    bd = GbdtBound{true, m == 1 ? 1 : m == -1 ? -1 : 0, lo, hi, v};
    return true;
}

// kCat (the *_cat entry points): a feature with is_cat[f] != 0 takes the categorical scan, any other the numeric one and a zero set; the
// branch is uniform for the wavefront.  Without kCat the kernel holds neither the branch nor the LDS.  kCst (the *_cst entry points): the
// wavefront first reads its leaf's bounds and its feature's sign and permission; without kCst the kernel reads none of the three tables.
template <bool kMissing, bool kCat, bool kCst> __global__ void __launch_bounds__(kBlock)
gbdt_split_feature_kernel(const int64_t *__restrict__ hist, int nleaf, int F, int max_bin, const int32_t *__restrict__ nbins,
                          const int32_t *__restrict__ nan_bin, const int32_t *__restrict__ expo, double l2, int64_t min_data, double min_hess,
                          double min_gain, int64_t *__restrict__ ws, const GbdtCatArgs cat, const GbdtCstArgs cs) {
    const int lane = threadIdx.x & (kWave - 1);
    int wave = threadIdx.x >> 6;
    if constexpr (kCst) wave = __builtin_amdgcn_readfirstlane(wave);     // the item is wave-uniform: its addresses stay in scalar registers
    const int64_t item = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
    if (item >= (int64_t)nleaf * F) return;
    const int f = (int)(item % F);
    GbdtBound bd{false, 0, 0.0, 0.0, 0.0};
    if constexpr (kCst) {
        if (!gbdt_cst_bound(cs, item / F, f, F, bd)) {
            if (lane < kRec) ws[item * kRec + lane] = gbdt_no_split(lane);
            if (kCat && lane < kSetWords) cat.sets[item * kSetWords + lane] = 0;
            return;
        }
    }
    if constexpr (kCat) {
        __shared__ int64_t cat_sorted[kBlock / kWave][kCatSorted];
        if (cat.is_cat[f]) {
            gbdt_split_scan_cat<kCst>(hist + item * max_bin * 3, f, lane, max_bin, nbins, kMissing ? nan_bin : nullptr, expo, l2, min_data, min_hess,
                                      min_gain, cat.cat_smooth, cat_sorted[threadIdx.x >> 6], ws + item * kRec, cat.sets + item * kSetWords, bd);
            return;
        }
        if (lane < kSetWords) cat.sets[item * kSetWords + lane] = 0;
    }
    gbdt_split_scan<kMissing, kCst>(hist + item * max_bin * 3, f, lane, max_bin, nbins, nan_bin, expo, l2, min_data, min_hess, min_gain, ws + item * kRec,
                                    bd);
}

// The same scan over a list of K slots of a histogram pool [nslots][F][max_bin][3]: item = (k, feature).  A slot outside the pool gives the
// record of a leaf without a split, and is never read.  The tables of kCst are indexed by k, the place in the list.
template <bool kMissing, bool kCat, bool kCst> __global__ void __launch_bounds__(kBlock)
gbdt_split_feature_slots_kernel(const int64_t *__restrict__ pool, int nslots, const int32_t *__restrict__ slots, int K, int F, int max_bin,
                                const int32_t *__restrict__ nbins, const int32_t *__restrict__ nan_bin, const int32_t *__restrict__ expo, double l2,
                                int64_t min_data, double min_hess, double min_gain, int64_t *__restrict__ ws, const GbdtCatArgs cat,
                                const GbdtCstArgs cs) {
    const int lane = threadIdx.x & (kWave - 1);
    int wave = threadIdx.x >> 6;
    if constexpr (kCst) wave = __builtin_amdgcn_readfirstlane(wave);
    const int64_t item = (int64_t)blockIdx.x * (kBlock / kWave) + wave;
    if (item >= (int64_t)K * F) return;
    const int f = (int)(item % F);
    const int slot = slots[item / F];
    int64_t *r = ws + item * kRec;
    GbdtBound bd{false, 0, 0.0, 0.0, 0.0};
    bool live = slot >= 0 && slot < nslots;
    if constexpr (kCst) live = live && gbdt_cst_bound(cs, item / F, f, F, bd);
    if (!live) {
        if (lane < kRec) r[lane] = gbdt_no_split(lane);
        if (kCat && lane < kSetWords) cat.sets[item * kSetWords + lane] = 0;
        return;
    }
    const int64_t *hp = pool + ((int64_t)slot * F + f) * max_bin * 3;
    if constexpr (kCat) {
        __shared__ int64_t cat_sorted[kBlock / kWave][kCatSorted];
        if (cat.is_cat[f]) {
            gbdt_split_scan_cat<kCst>(hp, f, lane, max_bin, nbins, kMissing ? nan_bin : nullptr, expo, l2, min_data, min_hess, min_gain, cat.cat_smooth,
                                      cat_sorted[threadIdx.x >> 6], r, cat.sets + item * kSetWords, bd);
            return;
        }
        if (lane < kSetWords) cat.sets[item * kSetWords + lane] = 0;
    }
    gbdt_split_scan<kMissing, kCst>(hp, f, lane, max_bin, nbins, nan_bin, expo, l2, min_data, min_hess, min_gain, r, bd);
}

// One wavefront per leaf: the best of its F feature records, ties to the lowest feature.  sets (NULL: none): the winner's left set, from
// ws_sets [leaves][F][kSetWords], zero for a leaf without a split.
__global__ void __launch_bounds__(kWave)
gbdt_split_leaf_kernel(const int64_t *__restrict__ ws, int F, int64_t *__restrict__ rec, const int64_t *__restrict__ ws_sets, int64_t *__restrict__ sets) {
    const int lane = threadIdx.x;
    const int64_t *w = ws + (int64_t)blockIdx.x * F * kRec;
    double bg = -INFINITY;
    int bf = -1;
    for (int f = lane; f < F; f += kWave) {
        const double g = __longlong_as_double(w[(int64_t)f * kRec]);
        if (w[(int64_t)f * kRec + 1] >= 0 && (bf < 0 || g > bg)) { bg = g; bf = f; }
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        const double og = __shfl_xor(bg, d);
        const int of = __shfl_xor(bf, d);
        if (of >= 0 && (bf < 0 || og > bg || (og == bg && of < bf))) { bg = og; bf = of; }
    }
    if (lane < kRec) {
        rec[(int64_t)blockIdx.x * kRec + lane] = bf >= 0 ? w[(int64_t)bf * kRec + lane] : gbdt_no_split(lane);
    }
    if (sets && lane >= 16 && lane < 16 + kSetWords)
        sets[(int64_t)blockIdx.x * kSetWords + lane - 16] = bf >= 0 ? ws_sets[((int64_t)blockIdx.x * F + bf) * kSetWords + lane - 16] : 0;
}

// ---------------------------------------------------------------- the stable partition
// A list is cut into pieces of kGbdtPartRows consecutive entries, one per workgroup, which walks its piece in kPartSteps steps of the block.
constexpr int kPartSteps = kGbdtPartRows / kBlock;
static_assert(kPartSteps * kBlock == kGbdtPartRows, "a workgroup of the partition owns whole steps of the block");

// The predicates of the stable partition: pred(i, row) gives entry i's row (-1 past the list of pred.m entries) and whether it goes to the front.
struct PartByBin {                                                      // bins[row][feature] <= bin, or == also_left
    const uint8_t *bins; int stride, n; const int32_t *rows; int m, feature, bin, also_left;
    __device__ __forceinline__ bool operator()(int64_t i, int &row) const {
        row = i < m ? rows[i] : -1;
        if (row < 0 || row >= n) return false;
        const int b = bins[(size_t)row * stride + feature];
        return b <= bin || b == also_left;                              // also_left: the NaN bin of a split whose missing rows go left, or -1
    }
};
// the *_cat partitions: at a categorical feature (is_cat[feature] != 0) bit bins[row][feature] of the node's set (4 int64 in device
// memory); at any other one PartByBin's rule, the NaN bin nan_bin[feature] going left under default_left.  The three tables are read as
// they are found: every load is uniform for the workgroup, and a bin indexes the 256 bits of a set whatever it is.
struct PartBySet {
    const uint8_t *bins; int stride, n; const int32_t *rows; int m, feature, bin, default_left;
    const uint8_t *is_cat; const int32_t *nan_bin; const int64_t *set;
    __device__ __forceinline__ bool operator()(int64_t i, int &row) const {
        row = i < m ? rows[i] : -1;
        if (row < 0 || row >= n) return false;
        const int b = bins[(size_t)row * stride + feature];
        if (is_cat[feature]) return (((u64)set[b >> 6]) >> (b & 63)) & 1ull;
        return b <= bin || (default_left && nan_bin && b == nan_bin[feature]);
    }
};
struct PartByMask {                                                     // ptr_gbdt_partition_mask: mask[row] != 0; rows == NULL: the list 0 .. m - 1
    const uint8_t *mask; int n; const int32_t *rows; int m;
    __device__ __forceinline__ bool operator()(int64_t i, int &row) const {
        row = i < m ? (rows ? rows[i] : (int)i) : -1;
        return row >= 0 && row < n && mask[row] != 0;
    }
};

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

// *count = the entries of piece j of pred's list that go to the front.  Every thread of the workgroup calls it.
template <class Pred> __device__ __forceinline__ void part_count(const Pred &pred, int j, int32_t *__restrict__ count) {
    __shared__ int32_t tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    int c = 0, row;
    for (int s = 0; s < kPartSteps; ++s)
        c += pred(((int64_t)j * kPartSteps + s) * kBlock + threadIdx.x, row) ? 1 : 0;
    atomicAdd(&tot, c);
    __syncthreads();
    if (threadIdx.x == 0) *count = tot;
}

// Piece j of pred's list into out [pred.m]: left_before entries of the pieces ahead of it and total_left of the whole list go to the front.
// An entry that goes to the front lands behind the front entries ahead of it, any other behind the front and the other entries ahead of
// it: both orders are kept.  A position outside the list is not written (counts that do not belong to this list cannot leave it).
template <class Pred> __device__ __forceinline__ void part_scatter(const Pred &pred, int j, int left_before, int total_left, int32_t *__restrict__ out) {
    __shared__ int32_t wave_left[kBlock / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    for (int s = 0; s < kPartSteps; ++s) {
        const int64_t i = ((int64_t)j * kPartSteps + s) * kBlock + threadIdx.x;
        int row;
        const bool left = pred(i, row);
        const unsigned long long mask = __ballot(left);
        if (lane == 0) wave_left[wave] = __popcll(mask);
        __syncthreads();
        int before = left_before + __popcll(mask & ((1ull << lane) - 1));
        int step_left = 0;
        for (int w = 0; w < kBlock / kWave; ++w) { if (w < wave) before += wave_left[w]; step_left += wave_left[w]; }
        const int64_t pos = left ? before : total_left + (i - before);                // `before` = the lefts ahead of entry i
        if (i < pred.m && pos >= 0 && pos < pred.m) out[pos] = row;
        left_before += step_left;
        __syncthreads();
    }
}

template <class Pred> __global__ void __launch_bounds__(kBlock)
gbdt_part_count_kernel(const Pred pred, int32_t *__restrict__ counts) { part_count(pred, blockIdx.x, counts + blockIdx.x); }

// counts [nb] -> their exclusive prefix, in place; counts[nb], and left_count[0] where it is not NULL, = the total.  One workgroup.  The
// batched partition scans the counts of all its segments at once and takes differences within a segment.
__global__ void __launch_bounds__(kBlock)
gbdt_part_scan_kernel(int32_t *__restrict__ counts, int nb, int32_t *__restrict__ left_count) {
    __shared__ int32_t seg[kBlock];
    const int t = threadIdx.x, per = (nb + kBlock - 1) / kBlock;
    const int lo = min(t * per, nb), hi = min(lo + per, nb);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += counts[i];
    const int upto = block_scan_add(seg, s);
    int run = upto - s;
    for (int i = lo; i < hi; ++i) { const int c = counts[i]; counts[i] = run; run += c; }
    if (t == kBlock - 1) {
        counts[nb] = upto;
        if (left_count) left_count[0] = upto;
    }
}

template <class Pred> __global__ void __launch_bounds__(kBlock)
gbdt_part_scatter_kernel(const Pred pred, const int32_t *__restrict__ counts, int nb, int32_t *__restrict__ out) {
    part_scatter(pred, blockIdx.x, counts[blockIdx.x], counts[nb], out);
}

// ---------------------------------------------------------------- one level of a depth-wise tree: the batched forms
// Every table below comes from the host and is read as untrusted: an entry that points outside rows, outside the pool's slots or at a
// feature or bin out of range is skipped (the whole item, uniformly for its workgroup, before any barrier), never followed.
struct GbdtSeg { int start, count, slot; bool ok; };

// segment `seg` of segs [K][3] = (start, count, slot) over rows [nrows], and the rows [r0, r1) of it that the item (seg, begin, len) names
__device__ __forceinline__ GbdtSeg gbdt_hist_item(const int32_t *__restrict__ segs, int K, const int32_t *__restrict__ item, int64_t nrows, int nslots,
                                                  int64_t &r0, int64_t &r1) {
    GbdtSeg s{0, 0, 0, false};
    const int k = item[0], begin = item[1], len = item[2];
    if (k < 0 || k >= K) return s;
    s.start = segs[k * 3]; s.count = segs[k * 3 + 1]; s.slot = segs[k * 3 + 2];
    if (s.start < 0 || s.count < 0 || (int64_t)s.start + s.count > nrows || s.slot < 0 || s.slot >= nslots) return s;
    if (begin < 0 || len < 0 || (int64_t)begin + len > s.count) return s;
    r0 = (int64_t)s.start + begin;
    r1 = r0 + len;
    s.ok = true;
    return s;
}

// direct form: grid = (items, feature tiles); an item is a whole segment of at most kGbdtDirectRows rows
__global__ void __launch_bounds__(kBlock)
gbdt_hist_seg_direct_kernel(const uint8_t *__restrict__ bins, int stride, int n, const int32_t *__restrict__ qg, const int32_t *__restrict__ qh,
                            const int32_t *__restrict__ rows, int64_t nrows, const int32_t *__restrict__ segs, int K,
                            const int32_t *__restrict__ items, int F, int max_bin, int64_t *__restrict__ pool, int nslots) {
    int64_t r0 = 0, r1 = 0;
    const GbdtSeg s = gbdt_hist_item(segs, K, items + (int64_t)blockIdx.x * 3, nrows, nslots, r0, r1);
    if (!s.ok || r1 - r0 > kGbdtDirectRows) return;
    int64_t *hist = pool + (int64_t)s.slot * F * max_bin * 3;
    const int f0 = blockIdx.y * kGbdtTile, cnt = (int)(r1 - r0) * kGbdtTile;
    for (int e = threadIdx.x; e < cnt; e += kBlock)
        hist_add_direct(bins, stride, n, qg, qh, rows[r0 + (e >> 4)], f0 + (e & (kGbdtTile - 1)), F, max_bin, hist);
}

// LDS form: grid = (items, feature tiles); an item is one row chunk of a segment
__global__ void __launch_bounds__(kBlock)
gbdt_hist_seg_lds_kernel(const uint8_t *__restrict__ bins, int stride, int n, const int32_t *__restrict__ qg, const int32_t *__restrict__ qh,
                         const int32_t *__restrict__ rows, int64_t nrows, const int32_t *__restrict__ segs, int K,
                         const int32_t *__restrict__ items, int F, int max_bin, int64_t *__restrict__ pool, int nslots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gbdt_smem[];
    int64_t r0 = 0, r1 = 0;
    const GbdtSeg s = gbdt_hist_item(segs, K, items + (int64_t)blockIdx.x * 3, nrows, nslots, r0, r1);
    if (!s.ok || r1 == r0) return;
    gbdt_hist_tile(gbdt_smem, bins, stride, n, qg, qh, rows, r0, r1, F, max_bin, pool + (int64_t)s.slot * F * max_bin * 3);
}

// trips [K][3] = (parent slot, child slot, out slot): grid = (K, chunks of one histogram)
__global__ void __launch_bounds__(kBlock)
gbdt_hist_sub_seg_kernel(int64_t *__restrict__ pool, int nslots, int64_t slot_elems, const int32_t *__restrict__ trips) {
    const int p = trips[blockIdx.x * 3], c = trips[blockIdx.x * 3 + 1], o = trips[blockIdx.x * 3 + 2];
    if (p < 0 || p >= nslots || c < 0 || c >= nslots || o < 0 || o >= nslots) return;
    const int64_t *pp = pool + p * slot_elems, *cp = pool + c * slot_elems;
    int64_t *op = pool + o * slot_elems;
    for (int64_t e = (int64_t)blockIdx.y * kBlock + threadIdx.x; e < slot_elems; e += (int64_t)gridDim.y * kBlock) op[e] = pp[e] - cp[e];
}

// The batched stable partition.  segs [K][cols] = (start, count, feature, bin[, also_left]) over rows [nrows], cols 4 or 5; blocks [NB][2] = (segment, j): workgroup b owns
// the entries j * 1024 .. of its segment, and a segment's blocks stand together in ascending j, so block b - j is the segment's first.
struct GbdtPartSeg { int start, count, feature, bin, also_left, nblk; bool ok; };
__device__ __forceinline__ GbdtPartSeg gbdt_part_block(const int32_t *__restrict__ segs, int cols, int K, const int32_t *__restrict__ blocks, int b, int NB,
                                                       int64_t nrows, int F, int &j) {
    GbdtPartSeg s{0, 0, 0, 0, -1, 0, false};
    const int k = blocks[b * 2];
    j = blocks[b * 2 + 1];
    if (k < 0 || k >= K) return s;
    segs += (int64_t)k * cols;
    s.start = segs[0]; s.count = segs[1]; s.feature = segs[2]; s.bin = segs[3];
    if (cols > 4) s.also_left = segs[4];
    if (s.also_left < -1 || s.also_left > 255) return s;
    if (s.start < 0 || s.count < 0 || (int64_t)s.start + s.count > nrows || s.feature < 0 || s.feature >= F || s.bin < 0 || s.bin > 255) return s;
    s.nblk = (int)(((int64_t)s.count + kGbdtPartRows - 1) / kGbdtPartRows);
    if (j < 0 || j >= s.nblk || b - j < 0 || (int64_t)b - j + s.nblk > NB) return s;
    s.ok = true;
    return s;
}

// kCat (ptr_gbdt_partition_segments_cat): the fifth column of a segment is default_left, and segment k splits under PartBySet with the set
// cat.sets[k]; without it the kernels are the ones they were.
struct GbdtCatSegs { const uint8_t *is_cat; const int32_t *nan_bin; const int64_t *sets; };
__device__ __forceinline__ PartBySet gbdt_part_by_set(const uint8_t *__restrict__ bins, int stride, int n, const int32_t *__restrict__ rows,
                                                      const GbdtPartSeg &s, int k, const GbdtCatSegs &cat) {
    return PartBySet{bins, stride, n, rows + s.start, s.count, s.feature, s.bin, s.also_left > 0 ? 1 : 0, cat.is_cat, cat.nan_bin, cat.sets + (int64_t)k * kSetWords};
}

template <bool kCat> __global__ void __launch_bounds__(kBlock)
gbdt_part_seg_count_kernel(const uint8_t *__restrict__ bins, int stride, int n, int F, const int32_t *__restrict__ rows, int64_t nrows,
                           const int32_t *__restrict__ segs, int cols, int K, const int32_t *__restrict__ blocks, int NB, int32_t *__restrict__ counts,
                           const GbdtCatSegs cat) {
    int j;
    const GbdtPartSeg s = gbdt_part_block(segs, cols, K, blocks, blockIdx.x, NB, nrows, F, j);
    if (!s.ok) { if (threadIdx.x == 0) counts[blockIdx.x] = 0; return; }
    if constexpr (kCat) part_count(gbdt_part_by_set(bins, stride, n, rows, s, blocks[blockIdx.x * 2], cat), j, counts + blockIdx.x);
    else part_count(PartByBin{bins, stride, n, rows + s.start, s.count, s.feature, s.bin, s.also_left}, j, counts + blockIdx.x);
}

// counts: the exclusive prefix over the blocks of all segments (gbdt_part_scan_kernel); the lefts ahead of block b in its segment are
// prefix[b] - prefix[b - j], which is the segmented scan.  A table that lies about its blocks cannot leave the segment (part_scatter).
template <bool kCat> __global__ void __launch_bounds__(kBlock)
gbdt_part_seg_scatter_kernel(const uint8_t *__restrict__ bins, int stride, int n, int F, const int32_t *__restrict__ rows, int64_t nrows,
                             const int32_t *__restrict__ segs, int cols, int K, const int32_t *__restrict__ blocks, int NB,
                             const int32_t *__restrict__ counts, int32_t *__restrict__ out, int32_t *__restrict__ left_counts, const GbdtCatSegs cat) {
    int j;
    const GbdtPartSeg s = gbdt_part_block(segs, cols, K, blocks, blockIdx.x, NB, nrows, F, j);
    if (!s.ok) return;
    const int first = blockIdx.x - j;
    const int total_left = counts[first + s.nblk] - counts[first];
    if (j == 0 && threadIdx.x == 0) left_counts[blocks[blockIdx.x * 2]] = total_left;
    if constexpr (kCat) part_scatter(gbdt_part_by_set(bins, stride, n, rows, s, blocks[blockIdx.x * 2], cat), j, counts[blockIdx.x] - counts[first], total_left, out + s.start);
    else part_scatter(PartByBin{bins, stride, n, rows + s.start, s.count, s.feature, s.bin, s.also_left}, j, counts[blockIdx.x] - counts[first], total_left,
                      out + s.start);
}

// ---------------------------------------------------------------- leaf values and prediction
__global__ void __launch_bounds__(kBlock)
gbdt_add_leaf_values_kernel(float *__restrict__ scores, int n, const int32_t *__restrict__ rows, const int32_t *__restrict__ offsets,
                            const float *__restrict__ values, int nleaves, int total) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    int lo = 0, hi = nleaves;                                           // the leaf whose [offsets[l], offsets[l + 1]) holds i
    while (lo + 1 < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const int row = rows[i];
    if (i < offsets[nleaves] && i >= offsets[0] && row >= 0 && row < n) scores[row] += values[lo];
}

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
__device__ __forceinline__ bool gbdt_in_set(const int64_t *__restrict__ set, int b) { return (((u64)set[b >> 6]) >> (b & 63)) & 1ull; }     // b in 0 .. 255

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

template <bool kCat> __global__ void __launch_bounds__(kBlock)
gbdt_predict_kernel(const float *__restrict__ X, int64_t n, int F, const int32_t *__restrict__ feature, const float *__restrict__ threshold,
                    const int32_t *__restrict__ left, const int32_t *__restrict__ right, const float *__restrict__ value,
                    const int32_t *__restrict__ tree_offsets, const uint8_t *__restrict__ default_left, int ntrees, float *__restrict__ out,
                    const GbdtCatWalk cat) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *x = X + i * F;
    float s = 0.0f;
    for (int t = 0; t < ntrees; ++t) {
        const int base = tree_offsets[t], nn = tree_offsets[t + 1] - base, leaves = base + t;      // a tree of nn nodes has nn + 1 leaves
        bool bad = false;
        const int node = gbdt_walk(nn, F, feature + base, left + base, right + base,
                                   [&](int at, int f) { return gbdt_raw_goes_left<kCat>(x[f], base + at, f, threshold, default_left, cat, bad); });
        s += gbdt_is_leaf(node, nn) && !bad ? value[leaves + ~node] : NAN;      // a malformed tree gives NaN
    }
    out[i] = s;
}

// The rows of a background matrix per LEAF of every tree (the covers of TreeSHAP): the walk of gbdt_predict_kernel, one integer atomic per
// (row, tree).  counts [nodes + ntrees] int64 in the layout of the leaf values.  A row a malformed tree loses counts nowhere.  The node arrays
// may be NULL where nodes == 0 (leaf-only trees).
template <bool kCat> __global__ void __launch_bounds__(kBlock)
gbdt_leaf_counts_kernel(const float *__restrict__ X, int64_t n, int F, const int32_t *__restrict__ feature, const float *__restrict__ threshold,
                        const int32_t *__restrict__ left, const int32_t *__restrict__ right, const int32_t *__restrict__ tree_offsets,
                        const uint8_t *__restrict__ default_left, int ntrees, int64_t nodes, int64_t nleaves, int64_t *__restrict__ counts, const GbdtCatWalk cat) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *x = X + i * F;
    for (int t = 0; t < ntrees; ++t) {
        const int base = tree_offsets[t], nn = tree_offsets[t + 1] - base;
        if (base < 0 || nn < 0 || (int64_t)base + nn > nodes) continue;   // a tree outside the node arrays (a tree of no node reads none of them)
        bool bad = false;
        const int node = gbdt_walk(nn, F, feature + base, left + base, right + base,
                                   [&](int at, int f) { return gbdt_raw_goes_left<kCat>(x[f], base + at, f, threshold, default_left, cat, bad); });
        const int64_t cell = (int64_t)base + t + ~node;
        if (gbdt_is_leaf(node, nn) && !bad && cell >= 0 && cell < nleaves) atomicAdd(reinterpret_cast<u64 *>(counts + cell), 1ull);
    }
}

// ---------------------------------------------------------------- a trained model on new data: leaf indices, per-leaf sums, add by leaf
// The leaf index of every (row, tree): the walk of gbdt_predict_kernel with nothing summed.  One thread per cell of leaf [n][stop - first],
// the tree fastest: a wavefront's stores are consecutive and its rows few.  A tree outside the node arrays or a malformed one gives -1.
template <bool kCat> __global__ void __launch_bounds__(kBlock)
gbdt_predict_leaf_kernel(const float *__restrict__ X, int64_t n, int F, const int32_t *__restrict__ feature, const float *__restrict__ threshold,
                         const int32_t *__restrict__ left, const int32_t *__restrict__ right, const int32_t *__restrict__ tree_offsets,
                         const uint8_t *__restrict__ default_left, int first, int ntrees, int64_t nodes, int32_t *__restrict__ leaf, const GbdtCatWalk cat) {
    const int64_t total = n * ntrees;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t i = e / ntrees;
        const int t = first + (int)(e - i * ntrees);
        const int base = tree_offsets[t], nn = tree_offsets[t + 1] - base;
        int out = -1;
        if (base >= 0 && nn >= 0 && (int64_t)base + nn <= nodes) {       // a tree of no node reads none of the node arrays
            const float *x = X + i * F;
            bool bad = false;
            const int node = gbdt_walk(nn, F, feature + base, left + base, right + base,
                                       [&](int at, int f) { return gbdt_raw_goes_left<kCat>(x[f], base + at, f, threshold, default_left, cat, bad); });
            if (gbdt_is_leaf(node, nn) && !bad) out = ~node;
        }
        leaf[e] = out;
    }
}

// One row of ONE tree (nn nodes, the arrays start at the tree) -> its leaf index, or -1 where the tree loses the row or the leaf is past nleaves.
template <bool kCat> __device__ __forceinline__ int gbdt_leaf_of(const float *__restrict__ x, int F, const int32_t *__restrict__ feature,
                                                                 const float *__restrict__ threshold, const int32_t *__restrict__ left,
                                                                 const int32_t *__restrict__ right, const uint8_t *__restrict__ default_left, int nn,
                                                                 int nleaves, const GbdtCatWalk &cat) {
    bool bad = false;
    const int node = gbdt_walk(nn, F, feature, left, right,
                               [&](int at, int f) { return gbdt_raw_goes_left<kCat>(x[f], at, f, threshold, default_left, cat, bad); });
    return gbdt_is_leaf(node, nn) && !bad && ~node < nleaves ? ~node : -1;
}

// The per-leaf sums of refit, both forms.  A workgroup owns the rows [r0, r1), whole multiples of the block except the last.  kLds: it zeroes
// nleaves cells of (int64, int64, uint32) in LDS, adds its rows there and flushes the cells a row reached, one global atomic per value;
// otherwise every row adds into global memory.  Integer atomics either way: the sums are those of any other launch shape.
template <bool kCat, bool kLds> __global__ void __launch_bounds__(kBlock)
gbdt_leaf_sums_kernel(const float *__restrict__ X, int64_t n, int F, const int32_t *__restrict__ feature, const float *__restrict__ threshold,
                      const int32_t *__restrict__ left, const int32_t *__restrict__ right, const uint8_t *__restrict__ default_left, int nn,
                      const int32_t *__restrict__ qg, const int32_t *__restrict__ qh, int nleaves, int32_t *__restrict__ leaf,
                      int64_t *__restrict__ sums, const GbdtCatWalk cat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gbdt_smem[];
    const int64_t per = (((n + gridDim.x - 1) / gridDim.x + kBlock - 1) / kBlock) * kBlock;
    const int64_t r0 = (int64_t)blockIdx.x * per;
    const int64_t r1 = r0 + per < n ? r0 + per : n;
    const int tid = threadIdx.x;
    u64 *lg = reinterpret_cast<u64 *>(gbdt_smem), *lh = lg + (kLds ? nleaves : 0);
    uint32_t *lc = reinterpret_cast<uint32_t *>(lh + (kLds ? nleaves : 0));
    if constexpr (kLds) {
        for (int e = tid; e < nleaves; e += kBlock) { lg[e] = 0; lh[e] = 0; lc[e] = 0; }
        __syncthreads();
    }
    for (int64_t i = r0 + tid; i < r1; i += kBlock) {
        const int l = gbdt_leaf_of<kCat>(X + i * F, F, feature, threshold, left, right, default_left, nn, nleaves, cat);
        leaf[i] = l;
        if (l < 0) continue;
        if constexpr (kLds) {
            atomicAdd(&lg[l], (u64)(int64_t)qg[i]);
            atomicAdd(&lh[l], (u64)(int64_t)qh[i]);
            atomicAdd(&lc[l], 1u);
        } else {
            hist_add_global(sums + (size_t)l * 3, qg[i], qh[i], 1);
        }
    }
    if constexpr (kLds) {
        __syncthreads();
        for (int e = tid; e < nleaves; e += kBlock) {
            const uint32_t c = lc[e];
            if (!c) continue;
            int64_t *cell = sums + (size_t)e * 3;
            if (lg[e]) atomicAdd(reinterpret_cast<u64 *>(cell), lg[e]);
            if (lh[e]) atomicAdd(reinterpret_cast<u64 *>(cell + 1), lh[e]);
            atomicAdd(reinterpret_cast<u64 *>(cell + 2), (u64)c);
        }
    }
}

// scores[r] += values[leaf[r]] for the rows whose leaf index is one: what refit adds after it has re-estimated a tree's values.
__global__ void __launch_bounds__(kBlock)
gbdt_add_by_leaf_kernel(float *__restrict__ scores, int64_t n, const int32_t *__restrict__ leaf, const float *__restrict__ values, int nleaves) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int l = leaf[i];
    if (l >= 0 && l < nleaves) scores[i] += values[l];
}

// ---------------------------------------------------------------- TreeSHAP
// Path-dependent TreeSHAP in its per-leaf form (include/ptranking_amd.h states the rule, tests/gbdt_shap_ref.py restates it operation by
// operation).  A workgroup is ONE wavefront and owns a row: it walks the leaf table in order and keeps the row's [F + 1] float64 sums in
// LDS, so a row's bits depend on the row and the tables alone.  Per leaf: lane p evaluates the path's node p (the predicate of
// gbdt_raw_goes_left against the node's direction bit) and a disagreement marks the node's element in LDS; lane e then holds element e's
// (z, o).  The sum over subsets is a Gauss-Legendre quadrature (below): lane q multiplies the path's factors up at node t_q, one broadcast of
// z per element, then lane e divides its own factor out of every P(t_q), read by broadcast, and adds v (o - z) sum to its feature's
// cell; the elements of a path carry distinct features, so the adds need no atomic.  (Lundberg's EXTEND / UNWIND recurrences, one
// subset-size weight per lane with a neighbour exchange per step, were built first and are bit-equal to their numpy restatement, but
// UNWIND is a polynomial deflation: on a chain of 63 features it lost local accuracy down to 8e-4.  The quadrature holds 2e-15 there.)
constexpr int kShapWave = 64;            // lanes: the elements of a path, kShapWave - 1 at the most (the rules of up to 32 nodes are exact for them)
constexpr int kShapMaxGroups = 8192;     // workgroups of a launch at the most (256 compute units x 32 wavefronts); the rows beyond stride
constexpr int kShapQuad = 528;           // the Gauss-Legendre rules of 1 .. 32 nodes on [0, 1], one after the other
constexpr int kShapMaxF = 8000;          // (F + 1) float64 of LDS per wavefront: 64 KiB less the element marks

struct GbdtShapTables {
    const int32_t *path_offsets, *elem_offsets; const float *leaf_value; int64_t nleaves;
    const int32_t *path_node; const uint8_t *path_dir, *path_elem; int64_t npath;
    const int32_t *elem_feature; const double *elem_z; int64_t nelem;
    const double *quad_t, *quad_w;       // kShapQuad nodes and weights: the rule of Q nodes at Q (Q - 1) / 2
};

template <bool kCat> __global__ void __launch_bounds__(kShapWave)
gbdt_shap_kernel(const float *__restrict__ X, int64_t n, int F, const int32_t *__restrict__ feature, const float *__restrict__ threshold,
                 int64_t nodes, const uint8_t *__restrict__ default_left, const GbdtCatWalk cat, const GbdtShapTables tb, double *__restrict__ phi) {
    extern __shared__ double shap_acc[];                                 // [F + 1] sums, then kShapWave marks
    uint32_t *marks = reinterpret_cast<uint32_t *>(shap_acc + F + 1);
    const int lane = threadIdx.x;
    marks[lane] = 0;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        const float *x = X + row * F;
        for (int k = lane; k <= F; k += kShapWave) shap_acc[k] = 0.0;
        bool bad = false;
        for (int64_t l = 0; l < tb.nleaves; ++l) {
            const int p0 = tb.path_offsets[l], p1 = tb.path_offsets[l + 1], e0 = tb.elem_offsets[l], e1 = tb.elem_offsets[l + 1];
            const int d = e1 - e0;
            if (p0 < 0 || p1 < p0 || p1 > tb.npath || e0 < 0 || d < 0 || e1 > tb.nelem || d >= kShapWave) { bad = true; continue; }    // wave-uniform
            __syncthreads();                                            // the marks are clear and the sums of the leaf before are written
            for (int p = p0 + lane; p < p1; p += kShapWave) {
                const int at = tb.path_node[p], e = tb.path_elem[p];
                if (at < 0 || at >= nodes || e >= d) { bad = true; continue; }
                const int f = feature[at];
                if (f < 0 || f >= F) { bad = true; continue; }
                if (gbdt_raw_goes_left<kCat>(x[f], at, f, threshold, default_left, cat, bad) != (tb.path_dir[p] != 0)) marks[e] = 1;
            }
            __syncthreads();
            double z = 1.0;
            bool o = false;
            int f = F;
            if (lane < d) {
                o = marks[lane] == 0;
                marks[lane] = 0;
                z = tb.elem_z[e0 + lane];
                f = tb.elem_feature[e0 + lane];
                if (f < 0 || f >= F) { bad = true; f = F; }
            }
            const u64 ones = __ballot(o);
            // The Shapley weight of a subset size is a Beta integral, so element k's sum over subsets is the integral over t in [0, 1] of
            // prod_{j != k} (z_j (1 - t) + o_j t): a polynomial of degree d - 1, which the Gauss-Legendre rule of Q = ceil(d / 2) nodes
            // integrates exactly.  Every factor and weight is positive: nothing cancels, at 63 elements as at 3.
            const int Q = (d + 1) >> 1, rule = Q * (Q - 1) / 2;
            // lane q: P(t_q) = prod_j (z_j (1 - t_q) + o_j t_q) in element order, one broadcast of z per element (o comes from the ballot)
            const double t = lane < Q ? tb.quad_t[rule + lane] : 0.5, u = 1.0 - t;
            double P = 1.0, pz = 1.0;
            for (int j = 0; j < d; ++j) {
                const double zj = __shfl(z, j, kShapWave);
                P = P * (zj * u + (((ones >> j) & 1ull) ? t : 0.0));
                pz = pz * zj;
            }
            // lane e: sum_q w_q P(t_q) / (z_e (1 - t_q) + o_e t_q), its own factor divided out again
            double sum = 0.0;
            for (int q = 0; q < Q; ++q) {
                const double tq = tb.quad_t[rule + q], wq = tb.quad_w[rule + q];
                const double mine = z * (1.0 - tq) + (o ? tq : 0.0);
                sum = sum + wq * (__shfl(P, q, kShapWave) / mine);
            }
            const double v = (double)tb.leaf_value[l];
            if (lane < d) shap_acc[f] = shap_acc[f] + sum * ((o ? 1.0 : 0.0) - z) * v;
            if (lane == 0) shap_acc[F] = shap_acc[F] + v * pz;
        }
        __syncthreads();
        const bool nan = __ballot(bad) != 0;
        for (int k = lane; k <= F; k += kShapWave) phi[row * (F + 1) + k] = nan ? (double)NAN : shap_acc[k];
        __syncthreads();
    }
}

// One finished tree over the BINNED rows of a row list: x <= edges[f][b] is bin <= b, so the walk lands in the leaf ptr_gbdt_predict finds on
// the raw row, and the same fp32 value is added.  The rows a sampled tree was not grown on get their leaf value here.
// kCat: also_left is NULL, and a numeric node sends the NaN bin nan_bin[f] left where default_left[node] is set (both may be NULL).
template <bool kCat> __global__ void __launch_bounds__(kBlock)
gbdt_add_tree_binned_kernel(float *__restrict__ scores, const uint8_t *__restrict__ bins, int stride, int n, int F, const int32_t *__restrict__ rows,
                            int m, const int32_t *__restrict__ feature, const int32_t *__restrict__ bin, const int32_t *__restrict__ left,
                            const int32_t *__restrict__ right, const float *__restrict__ value, const int32_t *__restrict__ also_left, int nn,
                            const uint8_t *__restrict__ default_left, const int32_t *__restrict__ nan_bin, const GbdtCatWalk cat) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int row = rows ? rows[i] : i;
    if (row < 0 || row >= n) return;
    const uint8_t *x = bins + (size_t)row * stride;
    bool bad = false;
    const int node = gbdt_walk(nn, F, feature, left, right, [&](int at, int f) {
        const int b = x[f];
        if constexpr (kCat) {
            const int ci = gbdt_cat_node(cat, at, f);
            if (ci == -2) { bad = true; return false; }
            if (ci >= 0) return gbdt_in_set(cat.cat_sets + (int64_t)ci * kSetWords, b);
            return b <= bin[at] || (default_left && nan_bin && default_left[at] != 0 && b == nan_bin[f]);
        }
        return b <= bin[at] || (also_left && b == also_left[at]);
    });
    scores[row] += gbdt_is_leaf(node, nn) && !bad ? value[~node] : NAN;         // a malformed tree gives NaN
}

// ---------------------------------------------------------------- row sampling: the bag and GOSS
// u(draw, unit) = pl_uniform(pl_query_keys(seed, draw), unit) of ptr_plhash.h: a multiple of 2^-24 in [0, 1), a function of its three
// arguments alone.  include/ptranking_amd.h states the rules; tests/gbdt_sample_ref.py restates them.
__global__ void __launch_bounds__(kBlock)
gbdt_bag_mask_kernel(int64_t n, const int32_t *__restrict__ qid, uint64_t seed, int64_t draw, float fraction, uint8_t *__restrict__ mask) {
    const PlKeys keys = pl_query_keys(seed, draw);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        mask[i] = pl_uniform(keys, qid ? (uint32_t)qid[i] : (uint32_t)i) < fraction ? 1 : 0;
}

// The digit that holds the K-th largest of the keys a table of kGossDigits counters counted (K >= 1, at most their number), and K less the
// keys in the digits above it.  Thread t sums the 8 digits below the top - 8 t; one scan over the 256 sums.  Every thread of every workgroup
// gets the same answer: it depends on the finished table alone.
__device__ __forceinline__ void goss_pick(const uint32_t *__restrict__ table, uint32_t K, uint32_t &digit, uint32_t &krem) {
    __shared__ uint32_t scan[kBlock];
    __shared__ uint32_t res[2];
    constexpr int per = kGossDigits / kBlock;
    const int t = threadIdx.x;
    uint32_t c[per], s = 0;
#pragma unroll
    for (int k = 0; k < per; ++k) { c[k] = table[kGossDigits - 1 - (t * per + k)]; s += c[k]; }
    if (t == 0) { res[0] = 0; res[1] = 1; }
    uint32_t run = block_scan_add(scan, s) - s;
    if (run < K && K <= run + s) {                                      // one thread: the sums ahead of it fall short of K, with its own they reach it
#pragma unroll
        for (int k = 0; k < per; ++k) {
            if (run < K && K <= run + c[k]) { res[0] = (uint32_t)(kGossDigits - 1 - (t * per + k)); res[1] = K - run; }
            run += c[k];
        }
    }
    __syncthreads();
    digit = res[0];
    krem = res[1];
    __syncthreads();
}

constexpr uint32_t kGossNan = 0x7f800000u;                              // |g h| bit patterns above this one are NaNs
__device__ __forceinline__ uint32_t goss_bits(float g, float h) { return __float_as_uint(g * h) & 0x7fffffffu; }      // one fp32 product

// Counting pass P of the select: the keys whose digits above pass P's equal the digits chosen so far, counted by pass P's digit.  LDS
// counters, flushed with one global integer atomic per digit the workgroup touched.  A NaN key counts as 0, the smallest.
template <int P> __global__ void __launch_bounds__(kBlock)
gbdt_goss_count_kernel(const float *__restrict__ g, const float *__restrict__ h, int64_t n, uint32_t K, uint32_t *__restrict__ tables,
                       int32_t *__restrict__ info) {
    __shared__ uint32_t cnt[kGossDigits];
    constexpr int shift = P == 0 ? 21 : P == 1 ? 10 : 0;
    constexpr uint32_t digits = P == 2 ? 1023u : 2047u, above = P == 0 ? 0u : P == 1 ? 0xffe00000u : 0xfffffc00u;
    for (int e = threadIdx.x; e < kGossDigits; e += kBlock) cnt[e] = 0;
    if (P == 0 && blockIdx.x == 0 && threadIdx.x < 3) info[threadIdx.x] = 0;
    uint32_t prefix = 0, k = K, d;
    if (P >= 1) { goss_pick(tables, k, d, k); prefix = d << 21; }
    if (P >= 2) { goss_pick(tables + kGossDigits, k, d, k); prefix |= d << 10; }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        uint32_t key = goss_bits(g[i], h[i]);
        if (key > kGossNan) key = 0;
        if ((key & above) == prefix) atomicAdd(&cnt[(key >> shift) & digits], 1u);
    }
    __syncthreads();
    uint32_t *out = tables + P * kGossDigits;
    for (int e = threadIdx.x; e < kGossDigits; e += kBlock) {
        const uint32_t c = cnt[e];
        if (c) atomicAdd(&out[e], c);
    }
}

// tau from the three tables; then per row: top (key >= tau, a NaN never), kept (top, or u(draw, row) < p_other), g and h of a kept row
// outside the top times w_other.  g_out / h_out may be g / h: a thread reads its row before it writes it.
__global__ void __launch_bounds__(kBlock)
gbdt_goss_apply_kernel(const float *g, const float *h, int64_t n, uint32_t K, const uint32_t *__restrict__ tables, uint64_t seed, int64_t draw,
                       float p_other, float w_other, float *g_out, float *h_out, uint8_t *__restrict__ mask, int32_t *__restrict__ info) {
    __shared__ uint32_t tot[2];
    uint32_t k = K, d0, d1, d2;
    goss_pick(tables, k, d0, k);
    goss_pick(tables + kGossDigits, k, d1, k);
    goss_pick(tables + 2 * kGossDigits, k, d2, k);
    const uint32_t tau = d0 << 21 | d1 << 10 | d2;
    if (threadIdx.x < 2) tot[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) info[0] = (int32_t)tau;
    __syncthreads();
    const PlKeys keys = pl_query_keys(seed, draw);
    uint32_t ntop = 0, nkeep = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        float a = g[i], b = h[i];
        const uint32_t key = goss_bits(a, b);
        const bool top = key <= kGossNan && key >= tau;
        const bool keep = top || pl_uniform(keys, (uint32_t)i) < p_other;
        if (keep && !top) { a *= w_other; b *= w_other; }
        g_out[i] = a;
        h_out[i] = b;
        mask[i] = keep ? 1 : 0;
        ntop += top ? 1 : 0;
        nkeep += keep ? 1 : 0;
    }
    atomicAdd(&tot[0], ntop);
    atomicAdd(&tot[1], nkeep);
    __syncthreads();
    if (threadIdx.x < 2 && tot[threadIdx.x]) atomicAdd(&info[1 + threadIdx.x], (int32_t)tot[threadIdx.x]);
}

// count, scan, scatter: the three launches of a stable partition under either predicate
template <class Pred> static int launch_partition(const Pred &pred, int nb, int32_t *out, int32_t *left_count, int32_t *ws, hipStream_t s, const char *who) {
    hipLaunchKernelGGL(gbdt_part_count_kernel<Pred>, dim3(nb), dim3(kBlock), 0, s, pred, ws);
    hipLaunchKernelGGL(gbdt_part_scan_kernel, dim3(1), dim3(kBlock), 0, s, ws, nb, left_count);
    hipLaunchKernelGGL(gbdt_part_scatter_kernel<Pred>, dim3(nb), dim3(kBlock), 0, s, pred, ws, nb, out);
    return check_hip(hipGetLastError(), who);
}

static int grid_for(int64_t elems, int cap = 1 << 16) {
    const int64_t b = (elems + kBlock - 1) / kBlock;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}
static int check_max_bin(int max_bin, const char *who) {
    if (max_bin < 2 || max_bin > PTR_GBDT_MAX_BIN) {
        set_error("%s: max_bin must be in 2 .. %d, got %d", who, PTR_GBDT_MAX_BIN, max_bin);
        return max_bin > PTR_GBDT_MAX_BIN ? PTR_ERR_UNSUPPORTED : PTR_ERR_INVALID_ARG;
    }
    return 0;
}
static int check_split_thresholds(double lambda_l2, double min_hess, double min_gain, const char *who) {
    if (!(lambda_l2 >= 0.0) || !(min_hess == min_hess) || !(min_gain == min_gain)) {
        set_error("%s: lambda_l2 must be >= 0 and no threshold may be NaN", who);
        return PTR_ERR_INVALID_ARG;
    }
    return 0;
}
static int check_bins_layout(int64_t n, int F, int stride, const char *who) {
    if (n < 0 || F < 0 || n > INT32_MAX) { set_error("%s: bad size (n=%lld, F=%d; n must fit an int32 row index)", who, (long long)n, F); return PTR_ERR_INVALID_ARG; }
    if (stride < F || stride % kGbdtTile != 0) {
        set_error("%s: stride must be a multiple of %d and at least F (stride=%d, F=%d)", who, kGbdtTile, stride, F);
        return PTR_ERR_INVALID_ARG;
    }
    return 0;
}

}  // namespace ptr

using namespace ptr;

// nan_bin == NULL: no missing values (ptr_gbdt_bin)
static int gbdt_bin_impl(const char *who, const float *X, int64_t n, int F, const float *edges, const int32_t *nbins, const int32_t *nan_bin, bool missing,
                         int max_bin, int stride, uint8_t *bins, void *stream) {
    if (int rc = check_bins_layout(n, F, stride, who)) return rc;
    if (int rc = check_max_bin(max_bin, who)) return rc;
    if (n == 0 || F == 0) return 0;
    if (!X || !edges || !nbins || !bins || (missing && !nan_bin)) { set_error("%s: NULL pointer (X, edges, nbins%s or bins)", who, missing ? ", nan_bin" : ""); return PTR_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(gbdt_bin_kernel, dim3(grid_for(n * stride)), dim3(kBlock), 0, as_stream(stream), X, n, F, edges, nbins, nan_bin, max_bin, stride, bins);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_bin(const float *X, int64_t n, int F, const float *edges, const int32_t *nbins, int max_bin, int stride, uint8_t *bins,
                            void *stream) {
    return gbdt_bin_impl("ptr_gbdt_bin", X, n, F, edges, nbins, nullptr, false, max_bin, stride, bins, stream);
}

extern "C" int ptr_gbdt_bin_missing(const float *X, int64_t n, int F, const float *edges, const int32_t *nbins, const int32_t *nan_bin, int max_bin,
                                    int stride, uint8_t *bins, void *stream) {
    return gbdt_bin_impl("ptr_gbdt_bin_missing", X, n, F, edges, nbins, nan_bin, true, max_bin, stride, bins, stream);
}

extern "C" int ptr_gbdt_quantize(const float *g, const float *h, int64_t n, int32_t *qg, int32_t *qh, int32_t *expo, int32_t *flag, uint32_t *state,
                                 void *stream) {
    const char *who = "ptr_gbdt_quantize";
    if (n < 0) { set_error("%s: negative size (n=%lld)", who, (long long)n); return PTR_ERR_INVALID_ARG; }
    if (n == 0) return 0;
    if (!g || !h || !qg || !qh || !expo || !flag || !state) { set_error("%s: NULL pointer", who); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_hip(hipMemsetAsync(state, 0, 2 * sizeof(uint32_t), as_stream(stream)), who)) return rc;
    hipLaunchKernelGGL(gbdt_absmax_kernel, dim3(grid_for(n, 1024)), dim3(kBlock), 0, as_stream(stream), g, h, n, state, flag);
    hipLaunchKernelGGL(gbdt_quantize_kernel, dim3(grid_for(n, 4096)), dim3(kBlock), 0, as_stream(stream), g, h, n, state, qg, qh, expo);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_histogram(const uint8_t *bins, int stride, int64_t n, const int32_t *qg, const int32_t *qh, const int32_t *rows, int64_t m,
                                  int F, int max_bin, int64_t *hist, void *stream) {
    const char *who = "ptr_gbdt_histogram";
    if (int rc = check_bins_layout(n, F, stride, who)) return rc;
    if (int rc = check_max_bin(max_bin, who)) return rc;
    if (m < 0 || m > INT32_MAX) { set_error("%s: bad row count m=%lld", who, (long long)m); return PTR_ERR_INVALID_ARG; }
    if (!rows && m > n) { set_error("%s: rows is NULL (the first m rows), so m must not exceed n (m=%lld, n=%lld)", who, (long long)m, (long long)n); return PTR_ERR_INVALID_ARG; }
    const GbdtHistForm form = gbdt_hist_form(m, F, max_bin);
    if (form.kind == 0) return 0;
    if (!bins || !qg || !qh || !hist) { set_error("%s: NULL pointer (bins, qg, qh or hist)", who); return PTR_ERR_INVALID_ARG; }
    if (reinterpret_cast<uintptr_t>(bins) & 15) { set_error("%s: bins must be 16-byte aligned", who); return PTR_ERR_INVALID_ARG; }
    if (form.kind == 1) {
        hipLaunchKernelGGL(gbdt_hist_direct_kernel, dim3((unsigned)((m * stride + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream), bins, stride, (int)n, qg, qh, rows,
                           (int)m, F, max_bin, hist);
    } else {
        if (int rc = allow_lds(gbdt_hist_lds_kernel, (size_t)form.lds_bytes)) return rc;
        hipLaunchKernelGGL(gbdt_hist_lds_kernel, dim3(form.chunks, form.tiles), dim3(kBlock), (size_t)form.lds_bytes, as_stream(stream), bins, stride,
                           (int)n, qg, qh, rows, (int)m, F, max_bin, hist);
    }
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_hist_sub(const int64_t *parent, const int64_t *child, int F, int max_bin, int64_t *out, void *stream) {
    const char *who = "ptr_gbdt_hist_sub";
    if (F < 0) { set_error("%s: negative size (F=%d)", who, F); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_max_bin(max_bin, who)) return rc;
    if (F == 0) return 0;
    if (!parent || !child || !out) { set_error("%s: NULL pointer", who); return PTR_ERR_INVALID_ARG; }
    const int64_t count = (int64_t)F * max_bin * 3;
    hipLaunchKernelGGL(gbdt_hist_sub_kernel, dim3(grid_for(count)), dim3(kBlock), 0, as_stream(stream), parent, child, count, out);
    return check_hip(hipGetLastError(), who);
}

// The categorical form of a split search (the *_cat entry points): is_cat == NULL is "no categorical".  ws then holds the items' records
// and, behind them, their sets: items * (kRec + kSetWords) int64.
struct GbdtCatSearch { const uint8_t *is_cat; double cat_smooth; int64_t *sets; };
static int check_cat_search(const GbdtCatSearch &cat, bool on, int F, const char *who) {
    if (!on) return 0;
    if (!(cat.cat_smooth >= 0.0) || cat.cat_smooth > 1.79769313486231570e308) { set_error("%s: cat_smooth must be a finite number >= 0, got %g", who, cat.cat_smooth); return PTR_ERR_INVALID_ARG; }
    if (!cat.sets || (F > 0 && !cat.is_cat)) { set_error("%s: NULL pointer (is_cat or sets)", who); return PTR_ERR_INVALID_ARG; }
    return 0;
}

// The constrained form of a split search (the *_cst entry points): cst == NULL is "interaction constraints alone", allowed == NULL "monotone
// constraints alone"; one of the two must be there, and cst needs mono.
static int check_cst_search(const GbdtCstArgs &cs, bool on, int F, const char *who) {
    if (!on) return 0;
    if (!cs.cst && !cs.allowed) { set_error("%s: neither cst nor allowed: the unconstrained entry point serves that", who); return PTR_ERR_INVALID_ARG; }
    if (cs.cst && F > 0 && !cs.mono) { set_error("%s: NULL pointer (mono, with cst)", who); return PTR_ERR_INVALID_ARG; }
    return 0;
}

static int gbdt_best_split_impl(const char *who, const int64_t *hist, int nleaf, int F, int max_bin, const int32_t *nbins, const int32_t *nan_bin,
                                bool missing, const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf, double min_sum_hessian_in_leaf,
                                double min_gain_to_split, int64_t *ws, int64_t *rec, void *stream, bool cat_on = false, GbdtCatSearch cat = {nullptr, 0.0, nullptr},
                                bool cst_on = false, GbdtCstArgs cs = {nullptr, nullptr, nullptr}) {
    if (nleaf < 0 || F < 0) { set_error("%s: negative size (nleaf=%d, F=%d)", who, nleaf, F); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_max_bin(max_bin, who)) return rc;
    if (int rc = check_split_thresholds(lambda_l2, min_sum_hessian_in_leaf, min_gain_to_split, who)) return rc;
    if (int rc = check_cat_search(cat, cat_on && nleaf > 0, F, who)) return rc;
    if (int rc = check_cst_search(cs, cst_on && nleaf > 0, F, who)) return rc;
    if (nleaf == 0) return 0;
    if (!rec || (F > 0 && (!hist || !nbins || !expo || !ws || (missing && !nan_bin)))) {
        set_error("%s: NULL pointer (hist, nbins%s, expo, ws or rec)", who, missing ? ", nan_bin" : "");
        return PTR_ERR_INVALID_ARG;
    }
    const int64_t items = (int64_t)nleaf * F;
    const dim3 grid((unsigned)((items + 3) / 4));
    int64_t *ws_sets = cat_on ? ws + items * kRec : nullptr;
    const GbdtCatArgs ca{cat.is_cat, cat.cat_smooth, ws_sets};
#define PTR_LAUNCH_SPLIT(M, C, S)                                                                                                                     \
    hipLaunchKernelGGL((gbdt_split_feature_kernel<M, C, S>), grid, dim3(kBlock), 0, as_stream(stream), hist, nleaf, F, max_bin, nbins, nan_bin, expo,     \
                       lambda_l2, min_data_in_leaf, min_sum_hessian_in_leaf, min_gain_to_split, ws, ca, cs)
#define PTR_LAUNCH_SPLIT_MC(S)                                                                                                                        \
    do {                                                                                                                                              \
        if (cat_on) { if (missing) PTR_LAUNCH_SPLIT(true, true, S); else PTR_LAUNCH_SPLIT(false, true, S); }                                          \
        else if (missing) PTR_LAUNCH_SPLIT(true, false, S);                                                                                           \
        else PTR_LAUNCH_SPLIT(false, false, S);                                                                                                       \
    } while (0)
    if (items > 0 && cst_on) PTR_LAUNCH_SPLIT_MC(true);
    else if (items > 0) PTR_LAUNCH_SPLIT_MC(false);
#undef PTR_LAUNCH_SPLIT_MC
#undef PTR_LAUNCH_SPLIT
    hipLaunchKernelGGL(gbdt_split_leaf_kernel, dim3(nleaf), dim3(kWave), 0, as_stream(stream), ws, F, rec, ws_sets, cat_on ? cat.sets : nullptr);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_best_split(const int64_t *hist, int nleaf, int F, int max_bin, const int32_t *nbins, const int32_t *expo, double lambda_l2,
                                   int64_t min_data_in_leaf, double min_sum_hessian_in_leaf, double min_gain_to_split, int64_t *ws, int64_t *rec,
                                   void *stream) {
    return gbdt_best_split_impl("ptr_gbdt_best_split", hist, nleaf, F, max_bin, nbins, nullptr, false, expo, lambda_l2, min_data_in_leaf,
                                min_sum_hessian_in_leaf, min_gain_to_split, ws, rec, stream);
}

extern "C" int ptr_gbdt_best_split_missing(const int64_t *hist, int nleaf, int F, int max_bin, const int32_t *nbins, const int32_t *nan_bin,
                                           const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf, double min_sum_hessian_in_leaf,
                                           double min_gain_to_split, int64_t *ws, int64_t *rec, void *stream) {
    return gbdt_best_split_impl("ptr_gbdt_best_split_missing", hist, nleaf, F, max_bin, nbins, nan_bin, true, expo, lambda_l2, min_data_in_leaf,
                                min_sum_hessian_in_leaf, min_gain_to_split, ws, rec, stream);
}

extern "C" int ptr_gbdt_best_split_cat(const int64_t *hist, int nleaf, int F, int max_bin, const int32_t *nbins, const int32_t *nan_bin,
                                       const uint8_t *is_cat, const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf,
                                       double min_sum_hessian_in_leaf, double min_gain_to_split, double cat_smooth, int64_t *ws, int64_t *rec,
                                       int64_t *sets, void *stream) {
    return gbdt_best_split_impl("ptr_gbdt_best_split_cat", hist, nleaf, F, max_bin, nbins, nan_bin, nan_bin != nullptr, expo, lambda_l2, min_data_in_leaf,
                                min_sum_hessian_in_leaf, min_gain_to_split, ws, rec, stream, true, GbdtCatSearch{is_cat, cat_smooth, sets});
}

extern "C" int ptr_gbdt_best_split_cst(const int64_t *hist, int nleaf, int F, int max_bin, const int32_t *nbins, const int32_t *nan_bin,
                                       const uint8_t *is_cat, const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf,
                                       double min_sum_hessian_in_leaf, double min_gain_to_split, double cat_smooth, int64_t *ws, int64_t *rec,
                                       int64_t *sets, const int8_t *mono, const double *cst, const uint8_t *allowed, void *stream) {
    return gbdt_best_split_impl("ptr_gbdt_best_split_cst", hist, nleaf, F, max_bin, nbins, nan_bin, nan_bin != nullptr, expo, lambda_l2, min_data_in_leaf,
                                min_sum_hessian_in_leaf, min_gain_to_split, ws, rec, stream, is_cat != nullptr, GbdtCatSearch{is_cat, cat_smooth, sets}, true,
                                GbdtCstArgs{mono, cst, allowed});
}

extern "C" size_t ptr_gbdt_partition_ws_ints(int64_t m) {
    return m <= 0 ? 1 : (size_t)((m + kGbdtPartRows - 1) / kGbdtPartRows) + 1;
}

static int gbdt_partition_impl(const char *who, const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m, int feature, int bin,
                               int also_left, int32_t *out, int32_t *left_count, int32_t *ws, void *stream) {
    if (int rc = check_bins_layout(n, F, stride, who)) return rc;
    if (m < 0 || m > INT32_MAX) { set_error("%s: bad row count m=%lld", who, (long long)m); return PTR_ERR_INVALID_ARG; }
    if (feature < 0 || feature >= F || bin < 0 || bin > 255) {
        set_error("%s: feature must be in 0 .. F - 1 and bin in 0 .. 255 (feature=%d, F=%d, bin=%d)", who, feature, F, bin);
        return PTR_ERR_INVALID_ARG;
    }
    if (also_left < -1 || also_left > 255) { set_error("%s: also_left must be -1 (none) or a bin in 0 .. 255, got %d", who, also_left); return PTR_ERR_INVALID_ARG; }
    if (!left_count) { set_error("%s: NULL left_count", who); return PTR_ERR_INVALID_ARG; }
    if (m == 0) return check_hip(hipMemsetAsync(left_count, 0, sizeof(int32_t), as_stream(stream)), who);
    if (!bins || !rows || !out || !ws) { set_error("%s: NULL pointer (bins, rows, out or ws)", who); return PTR_ERR_INVALID_ARG; }
    const int nb = (int)ptr_gbdt_partition_ws_ints(m) - 1;
    return launch_partition(PartByBin{bins, stride, (int)n, rows, (int)m, feature, bin, also_left}, nb, out, left_count, ws, as_stream(stream), who);
}

extern "C" int ptr_gbdt_partition_cat(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m, int feature, int bin,
                                      int default_left, const uint8_t *is_cat, const int32_t *nan_bin, const int64_t *set, int32_t *out,
                                      int32_t *left_count, int32_t *ws, void *stream) {
    const char *who = "ptr_gbdt_partition_cat";
    if (int rc = check_bins_layout(n, F, stride, who)) return rc;
    if (m < 0 || m > INT32_MAX) { set_error("%s: bad row count m=%lld", who, (long long)m); return PTR_ERR_INVALID_ARG; }
    if (feature < 0 || feature >= F || bin < 0 || bin > 255) {
        set_error("%s: feature must be in 0 .. F - 1 and bin in 0 .. 255 (feature=%d, F=%d, bin=%d)", who, feature, F, bin);
        return PTR_ERR_INVALID_ARG;
    }
    if (default_left != 0 && default_left != 1) { set_error("%s: default_left must be 0 or 1, got %d", who, default_left); return PTR_ERR_INVALID_ARG; }
    if (!left_count || !is_cat || !set) { set_error("%s: NULL pointer (left_count, is_cat or set)", who); return PTR_ERR_INVALID_ARG; }
    if (m == 0) return check_hip(hipMemsetAsync(left_count, 0, sizeof(int32_t), as_stream(stream)), who);
    if (!bins || !rows || !out || !ws) { set_error("%s: NULL pointer (bins, rows, out or ws)", who); return PTR_ERR_INVALID_ARG; }
    const int nb = (int)ptr_gbdt_partition_ws_ints(m) - 1;
    return launch_partition(PartBySet{bins, stride, (int)n, rows, (int)m, feature, bin, default_left, is_cat, nan_bin, set}, nb, out, left_count, ws,
                            as_stream(stream), who);
}

extern "C" int ptr_gbdt_partition(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m, int feature, int bin,
                                  int32_t *out, int32_t *left_count, int32_t *ws, void *stream) {
    return gbdt_partition_impl("ptr_gbdt_partition", bins, stride, n, F, rows, m, feature, bin, -1, out, left_count, ws, stream);
}

extern "C" int ptr_gbdt_partition_missing(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m, int feature, int bin,
                                          int also_left, int32_t *out, int32_t *left_count, int32_t *ws, void *stream) {
    return gbdt_partition_impl("ptr_gbdt_partition_missing", bins, stride, n, F, rows, m, feature, bin, also_left, out, left_count, ws, stream);
}

extern "C" int ptr_gbdt_add_leaf_values(float *scores, int64_t n, const int32_t *rows, const int32_t *offsets, const float *values, int nleaves,
                                        int64_t total, void *stream) {
    const char *who = "ptr_gbdt_add_leaf_values";
    if (n < 0 || n > INT32_MAX || nleaves < 0 || total < 0 || total > INT32_MAX) {
        set_error("%s: bad size (n=%lld, nleaves=%d, total=%lld)", who, (long long)n, nleaves, (long long)total);
        return PTR_ERR_INVALID_ARG;
    }
    if (nleaves == 0 || total == 0) return 0;
    if (!scores || !rows || !offsets || !values) { set_error("%s: NULL pointer (scores, rows, offsets or values)", who); return PTR_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(gbdt_add_leaf_values_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream), scores, (int)n, rows,
                       offsets, values, nleaves, (int)total);
    return check_hip(hipGetLastError(), who);
}

static int gbdt_predict_impl(const char *who, const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                             const int32_t *right, const float *value, const int32_t *tree_offsets, const uint8_t *default_left, bool missing, int ntrees,
                             float *out, void *stream, bool cat_on = false, GbdtCatWalk cat = {nullptr, nullptr, nullptr, 0}) {
    if (n < 0 || F < 0 || ntrees < 0) { set_error("%s: negative size (n=%lld, F=%d, ntrees=%d)", who, (long long)n, F, ntrees); return PTR_ERR_INVALID_ARG; }
    if (n == 0) return 0;
    if (!out || (F > 0 && !X)) { set_error("%s: NULL pointer (X or out)", who); return PTR_ERR_INVALID_ARG; }
    if (ntrees > 0 && (!feature || !threshold || !left || !right || !value || !tree_offsets || (missing && !default_left))) {
        set_error("%s: NULL tree array", who);
        return PTR_ERR_INVALID_ARG;
    }
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (cat_on)
        hipLaunchKernelGGL(gbdt_predict_kernel<true>, grid, dim3(kBlock), 0, as_stream(stream), X, n, F, feature, threshold, left, right, value, tree_offsets,
                           default_left, ntrees, out, cat);
    else
        hipLaunchKernelGGL(gbdt_predict_kernel<false>, grid, dim3(kBlock), 0, as_stream(stream), X, n, F, feature, threshold, left, right, value, tree_offsets,
                           default_left, ntrees, out, cat);
    return check_hip(hipGetLastError(), who);
}

// what the two walks ask of their categorical tables before a launch
static int check_cat_walk(const GbdtCatWalk &cat, bool any_nodes, int F, const char *who) {
    if (cat.ncat < 0) { set_error("%s: negative size (ncat=%d)", who, cat.ncat); return PTR_ERR_INVALID_ARG; }
    if (any_nodes && ((F > 0 && !cat.is_cat) || !cat.cat_index || (cat.ncat > 0 && !cat.cat_sets))) {
        set_error("%s: NULL pointer (is_cat, cat_index or cat_sets)", who);
        return PTR_ERR_INVALID_ARG;
    }
    return 0;
}

extern "C" int ptr_gbdt_predict_cat(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                    const int32_t *right, const float *value, const int32_t *tree_offsets, const uint8_t *default_left,
                                    const uint8_t *is_cat, const int32_t *cat_index, const int64_t *cat_sets, int ncat, int ntrees, float *out,
                                    void *stream) {
    const char *who = "ptr_gbdt_predict_cat";
    const GbdtCatWalk cat{is_cat, cat_index, cat_sets, ncat};
    if (int rc = check_cat_walk(cat, n > 0 && ntrees > 0, F, who)) return rc;
    return gbdt_predict_impl(who, X, n, F, feature, threshold, left, right, value, tree_offsets, default_left, false, ntrees, out, stream, true, cat);
}

extern "C" int ptr_gbdt_predict(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                const int32_t *right, const float *value, const int32_t *tree_offsets, int ntrees, float *out, void *stream) {
    return gbdt_predict_impl("ptr_gbdt_predict", X, n, F, feature, threshold, left, right, value, tree_offsets, nullptr, false, ntrees, out, stream);
}

extern "C" int ptr_gbdt_predict_missing(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                        const int32_t *right, const float *value, const int32_t *tree_offsets, const uint8_t *default_left, int ntrees,
                                        float *out, void *stream) {
    return gbdt_predict_impl("ptr_gbdt_predict_missing", X, n, F, feature, threshold, left, right, value, tree_offsets, default_left, true, ntrees, out,
                             stream);
}

// ---------------------------------------------------------------- the entry points of TreeSHAP
static int gbdt_leaf_counts_impl(const char *who, const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                 const int32_t *right, const int32_t *tree_offsets, const uint8_t *default_left, bool missing, int ntrees, int64_t nodes,
                                 int64_t nleaves, int64_t *counts, void *stream, bool cat_on = false, GbdtCatWalk cat = {nullptr, nullptr, nullptr, 0}) {
    if (n < 0 || F < 0 || ntrees < 0 || nodes < 0 || nleaves < 0) {
        set_error("%s: negative size (n=%lld, F=%d, ntrees=%d, nodes=%lld, nleaves=%lld)", who, (long long)n, F, ntrees, (long long)nodes,
                  (long long)nleaves);
        return PTR_ERR_INVALID_ARG;
    }
    if (nleaves == 0) return 0;
    if (!counts) { set_error("%s: NULL pointer (counts)", who); return PTR_ERR_INVALID_ARG; }
    const bool walk = n > 0 && ntrees > 0;
    if (walk && F > 0 && !X) { set_error("%s: NULL pointer (X)", who); return PTR_ERR_INVALID_ARG; }
    if (walk && (!tree_offsets || (nodes > 0 && (!feature || !threshold || !left || !right || (missing && !default_left))))) {
        set_error("%s: NULL tree array", who);
        return PTR_ERR_INVALID_ARG;
    }
    if (int rc = check_hip(hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)nleaves, as_stream(stream)), who)) return rc;
    if (!walk) return 0;
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (cat_on)
        hipLaunchKernelGGL(gbdt_leaf_counts_kernel<true>, grid, dim3(kBlock), 0, as_stream(stream), X, n, F, feature, threshold, left, right, tree_offsets,
                           default_left, ntrees, nodes, nleaves, counts, cat);
    else
        hipLaunchKernelGGL(gbdt_leaf_counts_kernel<false>, grid, dim3(kBlock), 0, as_stream(stream), X, n, F, feature, threshold, left, right, tree_offsets,
                           default_left, ntrees, nodes, nleaves, counts, cat);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_leaf_counts(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                    const int32_t *right, const int32_t *tree_offsets, int ntrees, int64_t nodes, int64_t nleaves, int64_t *counts,
                                    void *stream) {
    return gbdt_leaf_counts_impl("ptr_gbdt_leaf_counts", X, n, F, feature, threshold, left, right, tree_offsets, nullptr, false, ntrees, nodes, nleaves, counts,
                                 stream);
}

extern "C" int ptr_gbdt_leaf_counts_missing(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                            const int32_t *right, const int32_t *tree_offsets, const uint8_t *default_left, int ntrees,
                                            int64_t nodes, int64_t nleaves, int64_t *counts, void *stream) {
    return gbdt_leaf_counts_impl("ptr_gbdt_leaf_counts_missing", X, n, F, feature, threshold, left, right, tree_offsets, default_left, true, ntrees,
                                 nodes, nleaves, counts, stream);
}

extern "C" int ptr_gbdt_leaf_counts_cat(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                        const int32_t *right, const int32_t *tree_offsets, const uint8_t *default_left, const uint8_t *is_cat,
                                        const int32_t *cat_index, const int64_t *cat_sets, int ncat, int ntrees, int64_t nodes, int64_t nleaves,
                                        int64_t *counts, void *stream) {
    const char *who = "ptr_gbdt_leaf_counts_cat";
    const GbdtCatWalk cat{is_cat, cat_index, cat_sets, ncat};
    if (int rc = check_cat_walk(cat, n > 0 && ntrees > 0 && nleaves > 0 && nodes > 0, F, who)) return rc;
    return gbdt_leaf_counts_impl(who, X, n, F, feature, threshold, left, right, tree_offsets, default_left, false, ntrees, nodes, nleaves, counts, stream, true,
                                 cat);
}

// ---------------------------------------------------------------- the entry points of a trained model on new data
static int gbdt_predict_leaf_impl(const char *who, const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                  const int32_t *right, const int32_t *tree_offsets, const uint8_t *default_left, bool missing, int first, int ntrees,
                                  int64_t nodes, int32_t *leaf, void *stream, bool cat_on = false, GbdtCatWalk cat = {nullptr, nullptr, nullptr, 0}) {
    if (n < 0 || F < 0 || first < 0 || ntrees < 0 || nodes < 0) {
        set_error("%s: negative size (n=%lld, F=%d, first=%d, ntrees=%d, nodes=%lld)", who, (long long)n, F, first, ntrees, (long long)nodes);
        return PTR_ERR_INVALID_ARG;
    }
    if (n == 0 || ntrees == 0) return 0;
    if (!leaf || (F > 0 && !X)) { set_error("%s: NULL pointer (X or leaf)", who); return PTR_ERR_INVALID_ARG; }
    if (!tree_offsets || (nodes > 0 && (!feature || !threshold || !left || !right || (missing && !default_left)))) {
        set_error("%s: NULL tree array", who);
        return PTR_ERR_INVALID_ARG;
    }
    const int64_t blocks = (n * ntrees + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)));  // the kernel strides beyond
    if (cat_on)
        hipLaunchKernelGGL(gbdt_predict_leaf_kernel<true>, grid, dim3(kBlock), 0, as_stream(stream), X, n, F, feature, threshold, left, right, tree_offsets,
                           default_left, first, ntrees, nodes, leaf, cat);
    else
        hipLaunchKernelGGL(gbdt_predict_leaf_kernel<false>, grid, dim3(kBlock), 0, as_stream(stream), X, n, F, feature, threshold, left, right, tree_offsets,
                           default_left, first, ntrees, nodes, leaf, cat);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_predict_leaf(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                     const int32_t *right, const int32_t *tree_offsets, int first, int ntrees, int64_t nodes, int32_t *leaf,
                                     void *stream) {
    return gbdt_predict_leaf_impl("ptr_gbdt_predict_leaf", X, n, F, feature, threshold, left, right, tree_offsets, nullptr, false, first, ntrees, nodes, leaf,
                                  stream);
}

extern "C" int ptr_gbdt_predict_leaf_missing(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                             const int32_t *right, const int32_t *tree_offsets, const uint8_t *default_left, int first, int ntrees,
                                             int64_t nodes, int32_t *leaf, void *stream) {
    return gbdt_predict_leaf_impl("ptr_gbdt_predict_leaf_missing", X, n, F, feature, threshold, left, right, tree_offsets, default_left, true, first, ntrees,
                                  nodes, leaf, stream);
}

extern "C" int ptr_gbdt_predict_leaf_cat(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                         const int32_t *right, const int32_t *tree_offsets, const uint8_t *default_left, const uint8_t *is_cat,
                                         const int32_t *cat_index, const int64_t *cat_sets, int ncat, int first, int ntrees, int64_t nodes,
                                         int32_t *leaf, void *stream) {
    const char *who = "ptr_gbdt_predict_leaf_cat";
    const GbdtCatWalk cat{is_cat, cat_index, cat_sets, ncat};
    if (int rc = check_cat_walk(cat, n > 0 && ntrees > 0 && nodes > 0, F, who)) return rc;
    return gbdt_predict_leaf_impl(who, X, n, F, feature, threshold, left, right, tree_offsets, default_left, false, first, ntrees, nodes, leaf, stream, true,
                                  cat);
}

static int gbdt_leaf_sums_impl(const char *who, const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                               const int32_t *right, const uint8_t *default_left, bool missing, int nodes, const int32_t *qg, const int32_t *qh,
                               int nleaves, int32_t *leaf, int64_t *sums, void *stream, bool cat_on = false,
                               GbdtCatWalk cat = {nullptr, nullptr, nullptr, 0}) {
    if (n < 0 || F < 0 || nodes < 0 || nleaves < 0) {
        set_error("%s: negative size (n=%lld, F=%d, nodes=%d, nleaves=%d)", who, (long long)n, F, nodes, nleaves);
        return PTR_ERR_INVALID_ARG;
    }
    const GbdtLeafSumsForm form = gbdt_leaf_sums_form(n, nleaves);
    if (n == 0) return 0;
    if (!leaf || !qg || !qh || (F > 0 && !X) || (nleaves > 0 && !sums)) { set_error("%s: NULL pointer (X, qg, qh, leaf or sums)", who); return PTR_ERR_INVALID_ARG; }
    if (nodes > 0 && (!feature || !threshold || !left || !right || (missing && !default_left))) {
        set_error("%s: NULL tree array", who);
        return PTR_ERR_INVALID_ARG;
    }
    const bool lds = form.kind == 1;                                    // nleaves == 0: the global form writes leaf = -1 and adds nothing
    const dim3 grid((unsigned)form.groups);
    const size_t smem = lds ? (size_t)form.lds_bytes : 0;
#define PTR_LEAF_SUMS(CAT, LDS)                                                                                                                     \
    hipLaunchKernelGGL((gbdt_leaf_sums_kernel<CAT, LDS>), grid, dim3(kBlock), smem, as_stream(stream), X, n, F, feature, threshold, left, right,  \
                       default_left, nodes, qg, qh, nleaves, leaf, sums, cat)
    if (cat_on) { if (lds) PTR_LEAF_SUMS(true, true); else PTR_LEAF_SUMS(true, false); }
    else { if (lds) PTR_LEAF_SUMS(false, true); else PTR_LEAF_SUMS(false, false); }
#undef PTR_LEAF_SUMS
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_leaf_sums(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                  const int32_t *right, int nodes, const int32_t *qg, const int32_t *qh, int nleaves, int32_t *leaf, int64_t *sums,
                                  void *stream) {
    return gbdt_leaf_sums_impl("ptr_gbdt_leaf_sums", X, n, F, feature, threshold, left, right, nullptr, false, nodes, qg, qh, nleaves, leaf, sums, stream);
}

extern "C" int ptr_gbdt_leaf_sums_missing(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                          const int32_t *right, const uint8_t *default_left, int nodes, const int32_t *qg, const int32_t *qh,
                                          int nleaves, int32_t *leaf, int64_t *sums, void *stream) {
    return gbdt_leaf_sums_impl("ptr_gbdt_leaf_sums_missing", X, n, F, feature, threshold, left, right, default_left, true, nodes, qg, qh, nleaves, leaf,
                               sums, stream);
}

extern "C" int ptr_gbdt_leaf_sums_cat(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, const int32_t *left,
                                      const int32_t *right, const uint8_t *default_left, const uint8_t *is_cat, const int32_t *cat_index,
                                      const int64_t *cat_sets, int ncat, int nodes, const int32_t *qg, const int32_t *qh, int nleaves,
                                      int32_t *leaf, int64_t *sums, void *stream) {
    const char *who = "ptr_gbdt_leaf_sums_cat";
    const GbdtCatWalk cat{is_cat, cat_index, cat_sets, ncat};
    if (int rc = check_cat_walk(cat, n > 0 && nodes > 0, F, who)) return rc;
    return gbdt_leaf_sums_impl(who, X, n, F, feature, threshold, left, right, default_left, false, nodes, qg, qh, nleaves, leaf, sums, stream, true, cat);
}

extern "C" int ptr_gbdt_add_by_leaf(float *scores, int64_t n, const int32_t *leaf, const float *values, int nleaves, void *stream) {
    const char *who = "ptr_gbdt_add_by_leaf";
    if (n < 0 || nleaves < 0) { set_error("%s: negative size (n=%lld, nleaves=%d)", who, (long long)n, nleaves); return PTR_ERR_INVALID_ARG; }
    if (n == 0 || nleaves == 0) return 0;
    if (!scores || !leaf || !values) { set_error("%s: NULL pointer (scores, leaf or values)", who); return PTR_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(gbdt_add_by_leaf_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, as_stream(stream), scores, n, leaf, values,
                       nleaves);
    return check_hip(hipGetLastError(), who);
}

static int gbdt_shap_impl(const char *who, const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, int64_t nodes,
                          const GbdtShapTables &tb, const uint8_t *default_left, bool missing, double *phi, void *stream, bool cat_on = false,
                          GbdtCatWalk cat = {nullptr, nullptr, nullptr, 0}) {
    if (n < 0 || F < 0 || nodes < 0 || tb.nleaves < 0 || tb.npath < 0 || tb.nelem < 0) {
        set_error("%s: negative size (n=%lld, F=%d, nodes=%lld, nleaves=%lld, npath=%lld, nelem=%lld)", who, (long long)n, F, (long long)nodes,
                  (long long)tb.nleaves, (long long)tb.npath, (long long)tb.nelem);
        return PTR_ERR_INVALID_ARG;
    }
    if (nodes > INT32_MAX || tb.npath > INT32_MAX || tb.nelem > INT32_MAX) {
        set_error("%s: nodes, npath and nelem must fit an int32 index", who);
        return PTR_ERR_INVALID_ARG;
    }
    if (F > kShapMaxF) { set_error("%s: F=%d, at most %d (a row's sums live in LDS)", who, F, kShapMaxF); return PTR_ERR_UNSUPPORTED; }
    if (n == 0) return 0;
    if (!phi || (F > 0 && !X)) { set_error("%s: NULL pointer (X or phi)", who); return PTR_ERR_INVALID_ARG; }
    if (tb.nleaves > 0 && (!tb.path_offsets || !tb.elem_offsets || !tb.leaf_value)) { set_error("%s: NULL leaf table", who); return PTR_ERR_INVALID_ARG; }
    if (tb.npath > 0 && (!tb.path_node || !tb.path_dir || !tb.path_elem || !feature || !threshold || (missing && !default_left))) {
        set_error("%s: NULL path table or tree array", who);
        return PTR_ERR_INVALID_ARG;
    }
    if (tb.nelem > 0 && (!tb.elem_feature || !tb.elem_z || !tb.quad_t || !tb.quad_w)) {
        set_error("%s: NULL element table or quadrature table", who);
        return PTR_ERR_INVALID_ARG;
    }
    const dim3 grid((unsigned)(n < kShapMaxGroups ? n : kShapMaxGroups));
    const size_t lds = sizeof(double) * (size_t)(F + 1) + sizeof(uint32_t) * kShapWave;
    if (cat_on)
        hipLaunchKernelGGL(gbdt_shap_kernel<true>, grid, dim3(kShapWave), lds, as_stream(stream), X, n, F, feature, threshold, nodes, default_left, cat, tb, phi);
    else
        hipLaunchKernelGGL(gbdt_shap_kernel<false>, grid, dim3(kShapWave), lds, as_stream(stream), X, n, F, feature, threshold, nodes, default_left, cat, tb, phi);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_shap(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, int64_t nodes,
                             const int32_t *path_offsets, const int32_t *elem_offsets, const float *leaf_value, int64_t nleaves,
                             const int32_t *path_node, const uint8_t *path_dir, const uint8_t *path_elem, int64_t npath,
                             const int32_t *elem_feature, const double *elem_z, int64_t nelem, const double *quad_t, const double *quad_w,
        double *phi, void *stream) {
    const GbdtShapTables tb{path_offsets, elem_offsets, leaf_value, nleaves, path_node, path_dir, path_elem, npath, elem_feature, elem_z, nelem, quad_t, quad_w};
    return gbdt_shap_impl("ptr_gbdt_shap", X, n, F, feature, threshold, nodes, tb, nullptr, false, phi, stream);
}

extern "C" int ptr_gbdt_shap_missing(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, int64_t nodes,
                                     const int32_t *path_offsets, const int32_t *elem_offsets, const float *leaf_value, int64_t nleaves,
                                     const int32_t *path_node, const uint8_t *path_dir, const uint8_t *path_elem, int64_t npath,
                                     const int32_t *elem_feature, const double *elem_z, int64_t nelem, const double *quad_t, const double *quad_w,
        const uint8_t *default_left, double *phi,
                                     void *stream) {
    const GbdtShapTables tb{path_offsets, elem_offsets, leaf_value, nleaves, path_node, path_dir, path_elem, npath, elem_feature, elem_z, nelem, quad_t, quad_w};
    return gbdt_shap_impl("ptr_gbdt_shap_missing", X, n, F, feature, threshold, nodes, tb, default_left, true, phi, stream);
}

extern "C" int ptr_gbdt_shap_cat(const float *X, int64_t n, int F, const int32_t *feature, const float *threshold, int64_t nodes,
                                 const int32_t *path_offsets, const int32_t *elem_offsets, const float *leaf_value, int64_t nleaves,
                                 const int32_t *path_node, const uint8_t *path_dir, const uint8_t *path_elem, int64_t npath,
                                 const int32_t *elem_feature, const double *elem_z, int64_t nelem, const double *quad_t, const double *quad_w,
        const uint8_t *default_left,
                                 const uint8_t *is_cat, const int32_t *cat_index, const int64_t *cat_sets, int ncat, double *phi, void *stream) {
    const char *who = "ptr_gbdt_shap_cat";
    const GbdtShapTables tb{path_offsets, elem_offsets, leaf_value, nleaves, path_node, path_dir, path_elem, npath, elem_feature, elem_z, nelem, quad_t, quad_w};
    const GbdtCatWalk cat{is_cat, cat_index, cat_sets, ncat};
    if (int rc = check_cat_walk(cat, n > 0 && npath > 0, F, who)) return rc;
    return gbdt_shap_impl(who, X, n, F, feature, threshold, nodes, tb, default_left, false, phi, stream, true, cat);
}

// ---------------------------------------------------------------- the entry points of row sampling
static int check_rows(int64_t n, const char *who) {
    if (n < 0 || n > INT32_MAX) { set_error("%s: bad size (n=%lld; n must fit an int32 row index)", who, (long long)n); return PTR_ERR_INVALID_ARG; }
    return 0;
}

extern "C" int ptr_gbdt_bag_mask(int64_t n, const int32_t *qid, uint64_t seed, int64_t draw, float fraction, uint8_t *mask, void *stream) {
    const char *who = "ptr_gbdt_bag_mask";
    if (int rc = check_rows(n, who)) return rc;
    if (!(fraction > 0.0f && fraction <= 1.0f)) { set_error("%s: fraction must be in (0, 1], got %g", who, (double)fraction); return PTR_ERR_INVALID_ARG; }
    if (draw < 0) { set_error("%s: negative draw (%lld)", who, (long long)draw); return PTR_ERR_INVALID_ARG; }
    if (n == 0) return 0;
    if (!mask) { set_error("%s: NULL pointer (mask)", who); return PTR_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(gbdt_bag_mask_kernel, dim3(grid_for(n, 4096)), dim3(kBlock), 0, as_stream(stream), n, qid, seed, draw, fraction, mask);
    return check_hip(hipGetLastError(), who);
}

extern "C" size_t ptr_gbdt_goss_ws_ints(int64_t n) { (void)n; return (size_t)kGossPasses * kGossDigits + kGossState; }

extern "C" int ptr_gbdt_goss(const float *g, const float *h, int64_t n, double top_rate, double other_rate, uint64_t seed, int64_t draw,
                             float *g_out, float *h_out, uint8_t *mask, int32_t *info, int32_t *ws, void *stream) {
    const char *who = "ptr_gbdt_goss";
    if (int rc = check_rows(n, who)) return rc;
    if (!(top_rate > 0.0) || !(other_rate > 0.0) || !(top_rate + other_rate <= 1.0)) {
        set_error("%s: top_rate and other_rate must be > 0 and sum to at most 1 (got %g, %g)", who, top_rate, other_rate);
        return PTR_ERR_INVALID_ARG;
    }
    if (draw < 0) { set_error("%s: negative draw (%lld)", who, (long long)draw); return PTR_ERR_INVALID_ARG; }
    if (n == 0) return 0;
    if (!g || !h || !g_out || !h_out || !mask || !info || !ws) { set_error("%s: NULL pointer (g, h, g_out, h_out, mask, info or ws)", who); return PTR_ERR_INVALID_ARG; }
    int64_t K = (int64_t)floor((double)n * top_rate);
    K = K < 1 ? 1 : K > n ? n : K;
    const float p_other = (float)(other_rate / (1.0 - top_rate)), w_other = (float)((1.0 - top_rate) / other_rate);
    const GbdtGossForm form = gbdt_goss_form(n);
    hipStream_t s = as_stream(stream);
    uint32_t *tables = reinterpret_cast<uint32_t *>(ws);
    if (int rc = check_hip(hipMemsetAsync(ws, 0, ptr_gbdt_goss_ws_ints(n) * sizeof(int32_t), s), who)) return rc;
    hipLaunchKernelGGL(gbdt_goss_count_kernel<0>, dim3(form.groups), dim3(kBlock), 0, s, g, h, n, (uint32_t)K, tables, info);
    hipLaunchKernelGGL(gbdt_goss_count_kernel<1>, dim3(form.groups), dim3(kBlock), 0, s, g, h, n, (uint32_t)K, tables, info);
    hipLaunchKernelGGL(gbdt_goss_count_kernel<2>, dim3(form.groups), dim3(kBlock), 0, s, g, h, n, (uint32_t)K, tables, info);
    hipLaunchKernelGGL(gbdt_goss_apply_kernel, dim3(form.groups), dim3(kBlock), 0, s, g, h, n, (uint32_t)K, tables, seed, draw, p_other, w_other, g_out,
                       h_out, mask, info);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_partition_mask(const uint8_t *mask, int64_t n, const int32_t *rows, int64_t m, int32_t *out, int32_t *left_count,
                                       int32_t *ws, void *stream) {
    const char *who = "ptr_gbdt_partition_mask";
    if (int rc = check_rows(n, who)) return rc;
    if (m < 0 || m > INT32_MAX) { set_error("%s: bad row count m=%lld", who, (long long)m); return PTR_ERR_INVALID_ARG; }
    if (!left_count) { set_error("%s: NULL left_count", who); return PTR_ERR_INVALID_ARG; }
    if (m == 0) return check_hip(hipMemsetAsync(left_count, 0, sizeof(int32_t), as_stream(stream)), who);
    if (!out || !ws || (n > 0 && !mask)) { set_error("%s: NULL pointer (mask, out or ws)", who); return PTR_ERR_INVALID_ARG; }
    if (rows == out) { set_error("%s: out must not be rows (the partition is not done in place)", who); return PTR_ERR_INVALID_ARG; }
    const int nb = (int)ptr_gbdt_partition_ws_ints(m) - 1;
    return launch_partition(PartByMask{mask, (int)n, rows, (int)m}, nb, out, left_count, ws, as_stream(stream), who);
}

static int gbdt_add_tree_binned_impl(const char *who, float *scores, const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m,
                                     const int32_t *feature, const int32_t *bin, const int32_t *left, const int32_t *right, const float *value,
                                     const int32_t *also_left, bool missing, int nnodes, void *stream, bool cat_on = false,
                                     const uint8_t *default_left = nullptr, const int32_t *nan_bin = nullptr, GbdtCatWalk cat = {nullptr, nullptr, nullptr, 0}) {
    if (int rc = check_bins_layout(n, F, stride, who)) return rc;
    if (m < 0 || m > INT32_MAX || nnodes < 0) { set_error("%s: bad size (m=%lld, nnodes=%d)", who, (long long)m, nnodes); return PTR_ERR_INVALID_ARG; }
    if (!rows && m > n) { set_error("%s: rows is NULL (the first m rows), so m must not exceed n (m=%lld, n=%lld)", who, (long long)m, (long long)n); return PTR_ERR_INVALID_ARG; }
    if (m == 0 || n == 0) return 0;
    if (!scores || !value || (nnodes > 0 && (!bins || !feature || !bin || !left || !right || (missing && !also_left)))) {
        set_error("%s: NULL pointer (scores, bins, value or a tree array)", who);
        return PTR_ERR_INVALID_ARG;
    }
    const dim3 grid((unsigned)((m + kBlock - 1) / kBlock));
    if (cat_on)
        hipLaunchKernelGGL(gbdt_add_tree_binned_kernel<true>, grid, dim3(kBlock), 0, as_stream(stream), scores, bins, stride, (int)n, F, rows, (int)m, feature, bin,
                           left, right, value, also_left, nnodes, default_left, nan_bin, cat);
    else
        hipLaunchKernelGGL(gbdt_add_tree_binned_kernel<false>, grid, dim3(kBlock), 0, as_stream(stream), scores, bins, stride, (int)n, F, rows, (int)m, feature, bin,
                           left, right, value, also_left, nnodes, default_left, nan_bin, cat);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_add_tree_binned_cat(float *scores, const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m,
                                            const int32_t *feature, const int32_t *bin, const int32_t *left, const int32_t *right, const float *value,
                                            const uint8_t *default_left, const uint8_t *is_cat, const int32_t *nan_bin, const int32_t *cat_index,
                                            const int64_t *cat_sets, int ncat, int nnodes, void *stream) {
    const char *who = "ptr_gbdt_add_tree_binned_cat";
    const GbdtCatWalk cat{is_cat, cat_index, cat_sets, ncat};
    if (int rc = check_cat_walk(cat, m > 0 && n > 0 && nnodes > 0, F, who)) return rc;
    return gbdt_add_tree_binned_impl(who, scores, bins, stride, n, F, rows, m, feature, bin, left, right, value, nullptr, false, nnodes, stream, true,
                                     default_left, nan_bin, cat);
}

extern "C" int ptr_gbdt_add_tree_binned(float *scores, const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m,
                                        const int32_t *feature, const int32_t *bin, const int32_t *left, const int32_t *right, const float *value,
                                        int nnodes, void *stream) {
    return gbdt_add_tree_binned_impl("ptr_gbdt_add_tree_binned", scores, bins, stride, n, F, rows, m, feature, bin, left, right, value, nullptr, false,
                                     nnodes, stream);
}

extern "C" int ptr_gbdt_add_tree_binned_missing(float *scores, const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t m,
                                                const int32_t *feature, const int32_t *bin, const int32_t *left, const int32_t *right,
                                                const float *value, const int32_t *also_left, int nnodes, void *stream) {
    return gbdt_add_tree_binned_impl("ptr_gbdt_add_tree_binned_missing", scores, bins, stride, n, F, rows, m, feature, bin, left, right, value, also_left,
                                     true, nnodes, stream);
}

// ---------------------------------------------------------------- the batched entry points of a depth-wise level
enum { kCheckMaxBin = 1, kCheckBins = 2 };
static int check_level_common(const char *who, int64_t n, int F, int stride, int max_bin, int K, int what) {
    if (K < 0) { set_error("%s: negative table length (K=%d)", who, K); return PTR_ERR_INVALID_ARG; }
    if (F < 1) { set_error("%s: F must be >= 1, got %d", who, F); return PTR_ERR_INVALID_ARG; }
    if (what & kCheckMaxBin) if (int rc = check_max_bin(max_bin, who)) return rc;
    if (what & kCheckBins) if (int rc = check_bins_layout(n, F, stride, who)) return rc;
    return 0;
}

extern "C" int ptr_gbdt_histogram_segments(const uint8_t *bins, int stride, int64_t n, const int32_t *qg, const int32_t *qh, const int32_t *rows,
                                           int64_t nrows, const int32_t *segs, int K, const int32_t *items, int n_direct, int n_lds, int F,
                                           int max_bin, int64_t *pool, int nslots, void *stream) {
    const char *who = "ptr_gbdt_histogram_segments";
    if (int rc = check_level_common(who, n, F, stride, max_bin, K, kCheckMaxBin | kCheckBins)) return rc;
    if (n_direct < 0 || n_lds < 0 || nrows < 0 || nrows > INT32_MAX || nslots < 0) {
        set_error("%s: bad size (n_direct=%d, n_lds=%d, nrows=%lld, nslots=%d)", who, n_direct, n_lds, (long long)nrows, nslots);
        return PTR_ERR_INVALID_ARG;
    }
    if (K == 0 || n_direct + (int64_t)n_lds == 0) return 0;
    if (!bins || !qg || !qh || !rows || !segs || !items || !pool) { set_error("%s: NULL pointer (bins, qg, qh, rows, segs, items or pool)", who); return PTR_ERR_INVALID_ARG; }
    if (reinterpret_cast<uintptr_t>(bins) & 15) { set_error("%s: bins must be 16-byte aligned", who); return PTR_ERR_INVALID_ARG; }
    const GbdtSegForm form = gbdt_hist_segments_form(kGbdtDirectRows + 1, F, max_bin, 0);
    if (n_direct > 0)
        hipLaunchKernelGGL(gbdt_hist_seg_direct_kernel, dim3(n_direct, form.tiles), dim3(kBlock), 0, as_stream(stream), bins, stride, (int)n, qg, qh, rows,
                           nrows, segs, K, items, F, max_bin, pool, nslots);
    if (n_lds > 0) {
        if (int rc = allow_lds(gbdt_hist_seg_lds_kernel, (size_t)form.lds_bytes)) return rc;
        hipLaunchKernelGGL(gbdt_hist_seg_lds_kernel, dim3(n_lds, form.tiles), dim3(kBlock), (size_t)form.lds_bytes, as_stream(stream), bins, stride, (int)n,
                           qg, qh, rows, nrows, segs, K, items + (int64_t)n_direct * 3, F, max_bin, pool, nslots);
    }
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_hist_sub_segments(int64_t *pool, int nslots, int F, int max_bin, const int32_t *trips, int K, void *stream) {
    const char *who = "ptr_gbdt_hist_sub_segments";
    if (int rc = check_level_common(who, 0, F, 0, max_bin, K, kCheckMaxBin)) return rc;
    if (nslots < 0) { set_error("%s: negative size (nslots=%d)", who, nslots); return PTR_ERR_INVALID_ARG; }
    if (K == 0) return 0;
    if (!pool || !trips) { set_error("%s: NULL pointer (pool or trips)", who); return PTR_ERR_INVALID_ARG; }
    const int64_t elems = (int64_t)F * max_bin * 3;
    hipLaunchKernelGGL(gbdt_hist_sub_seg_kernel, dim3(K, grid_for(elems, 64)), dim3(kBlock), 0, as_stream(stream), pool, nslots, elems, trips);
    return check_hip(hipGetLastError(), who);
}

static int gbdt_best_split_slots_impl(const char *who, const int64_t *pool, int nslots, const int32_t *slots, int K, int F, int max_bin,
                                      const int32_t *nbins, const int32_t *nan_bin, bool missing, const int32_t *expo, double lambda_l2,
                                      int64_t min_data_in_leaf, double min_sum_hessian_in_leaf, double min_gain_to_split, int64_t *ws, int64_t *rec,
                                      void *stream, bool cat_on = false, GbdtCatSearch cat = {nullptr, 0.0, nullptr}, bool cst_on = false,
                                      GbdtCstArgs cs = {nullptr, nullptr, nullptr}) {
    if (int rc = check_level_common(who, 0, F, 0, max_bin, K, kCheckMaxBin)) return rc;
    if (nslots < 0) { set_error("%s: negative size (nslots=%d)", who, nslots); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_split_thresholds(lambda_l2, min_sum_hessian_in_leaf, min_gain_to_split, who)) return rc;
    if (int rc = check_cat_search(cat, cat_on && K > 0, F, who)) return rc;
    if (int rc = check_cst_search(cs, cst_on && K > 0, F, who)) return rc;
    if (K == 0) return 0;
    if (!pool || !slots || !nbins || !expo || !ws || !rec || (missing && !nan_bin)) {
        set_error("%s: NULL pointer (pool, slots, nbins%s, expo, ws or rec)", who, missing ? ", nan_bin" : "");
        return PTR_ERR_INVALID_ARG;
    }
    const int64_t items = (int64_t)K * F;
    const dim3 grid((unsigned)((items + 3) / 4));
    int64_t *ws_sets = cat_on ? ws + items * kRec : nullptr;
    const GbdtCatArgs ca{cat.is_cat, cat.cat_smooth, ws_sets};
#define PTR_LAUNCH_SPLIT(M, C, S)                                                                                                                       \
    hipLaunchKernelGGL((gbdt_split_feature_slots_kernel<M, C, S>), grid, dim3(kBlock), 0, as_stream(stream), pool, nslots, slots, K, F, max_bin, nbins,     \
                       nan_bin, expo, lambda_l2, min_data_in_leaf, min_sum_hessian_in_leaf, min_gain_to_split, ws, ca, cs)
#define PTR_LAUNCH_SPLIT_MC(S)                                                                                                                          \
    do {                                                                                                                                                \
        if (cat_on) { if (missing) PTR_LAUNCH_SPLIT(true, true, S); else PTR_LAUNCH_SPLIT(false, true, S); }                                            \
        else if (missing) PTR_LAUNCH_SPLIT(true, false, S);                                                                                             \
        else PTR_LAUNCH_SPLIT(false, false, S);                                                                                                         \
    } while (0)
    if (items > 0 && cst_on) PTR_LAUNCH_SPLIT_MC(true);
    else if (items > 0) PTR_LAUNCH_SPLIT_MC(false);
#undef PTR_LAUNCH_SPLIT_MC
#undef PTR_LAUNCH_SPLIT
    hipLaunchKernelGGL(gbdt_split_leaf_kernel, dim3(K), dim3(kWave), 0, as_stream(stream), ws, F, rec, ws_sets, cat_on ? cat.sets : nullptr);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_best_split_slots_cat(const int64_t *pool, int nslots, const int32_t *slots, int K, int F, int max_bin, const int32_t *nbins,
                                             const int32_t *nan_bin, const uint8_t *is_cat, const int32_t *expo, double lambda_l2,
                                             int64_t min_data_in_leaf, double min_sum_hessian_in_leaf, double min_gain_to_split, double cat_smooth,
                                             int64_t *ws, int64_t *rec, int64_t *sets, void *stream) {
    return gbdt_best_split_slots_impl("ptr_gbdt_best_split_slots_cat", pool, nslots, slots, K, F, max_bin, nbins, nan_bin, nan_bin != nullptr, expo, lambda_l2,
                                      min_data_in_leaf, min_sum_hessian_in_leaf, min_gain_to_split, ws, rec, stream, true,
                                      GbdtCatSearch{is_cat, cat_smooth, sets});
}

extern "C" int ptr_gbdt_best_split_slots_cst(const int64_t *pool, int nslots, const int32_t *slots, int K, int F, int max_bin, const int32_t *nbins,
                                             const int32_t *nan_bin, const uint8_t *is_cat, const int32_t *expo, double lambda_l2,
                                             int64_t min_data_in_leaf, double min_sum_hessian_in_leaf, double min_gain_to_split, double cat_smooth,
                                             int64_t *ws, int64_t *rec, int64_t *sets, const int8_t *mono, const double *cst, const uint8_t *allowed,
                                             void *stream) {
    return gbdt_best_split_slots_impl("ptr_gbdt_best_split_slots_cst", pool, nslots, slots, K, F, max_bin, nbins, nan_bin, nan_bin != nullptr, expo, lambda_l2,
                                      min_data_in_leaf, min_sum_hessian_in_leaf, min_gain_to_split, ws, rec, stream, is_cat != nullptr,
                                      GbdtCatSearch{is_cat, cat_smooth, sets}, true, GbdtCstArgs{mono, cst, allowed});
}

extern "C" int ptr_gbdt_best_split_slots(const int64_t *pool, int nslots, const int32_t *slots, int K, int F, int max_bin, const int32_t *nbins,
                                         const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf, double min_sum_hessian_in_leaf,
                                         double min_gain_to_split, int64_t *ws, int64_t *rec, void *stream) {
    return gbdt_best_split_slots_impl("ptr_gbdt_best_split_slots", pool, nslots, slots, K, F, max_bin, nbins, nullptr, false, expo, lambda_l2,
                                      min_data_in_leaf, min_sum_hessian_in_leaf, min_gain_to_split, ws, rec, stream);
}

extern "C" int ptr_gbdt_best_split_slots_missing(const int64_t *pool, int nslots, const int32_t *slots, int K, int F, int max_bin, const int32_t *nbins,
                                                 const int32_t *nan_bin, const int32_t *expo, double lambda_l2, int64_t min_data_in_leaf,
                                                 double min_sum_hessian_in_leaf, double min_gain_to_split, int64_t *ws, int64_t *rec, void *stream) {
    return gbdt_best_split_slots_impl("ptr_gbdt_best_split_slots_missing", pool, nslots, slots, K, F, max_bin, nbins, nan_bin, true, expo, lambda_l2,
                                      min_data_in_leaf, min_sum_hessian_in_leaf, min_gain_to_split, ws, rec, stream);
}

extern "C" size_t ptr_gbdt_partition_segments_ws_ints(int64_t nblocks) { return nblocks <= 0 ? 1 : (size_t)nblocks + 1; }

// cols: the width of a segs entry, 4 (start, count, feature, bin) or 5 (with also_left)
static int gbdt_partition_segments_impl(const char *who, const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t nrows,
                                        const int32_t *segs, int cols, int K, const int32_t *blocks, int nblocks, int32_t *out, int32_t *left_counts,
                                        int32_t *ws, int64_t ws_ints, void *stream, bool cat_on = false, GbdtCatSegs cat = {nullptr, nullptr, nullptr}) {
    if (int rc = check_level_common(who, n, F, stride, 0, K, kCheckBins)) return rc;
    if (cat_on && K > 0 && (!cat.is_cat || !cat.sets)) { set_error("%s: NULL pointer (is_cat or sets)", who); return PTR_ERR_INVALID_ARG; }
    if (nblocks < 0 || nrows < 0 || nrows > INT32_MAX) { set_error("%s: bad size (nblocks=%d, nrows=%lld)", who, nblocks, (long long)nrows); return PTR_ERR_INVALID_ARG; }
    if (nrows > 0 && (!rows || !out)) { set_error("%s: NULL pointer (rows or out)", who); return PTR_ERR_INVALID_ARG; }
    if (nrows > 0 && rows == out) { set_error("%s: out must not be rows (the partition is not done in place)", who); return PTR_ERR_INVALID_ARG; }
    if (K > 0 && (!segs || !left_counts)) { set_error("%s: NULL pointer (segs or left_counts)", who); return PTR_ERR_INVALID_ARG; }
    if (K > 0 && nblocks > 0 && (!bins || !blocks || !ws)) { set_error("%s: NULL pointer (bins, blocks or ws)", who); return PTR_ERR_INVALID_ARG; }
    if (K > 0 && nblocks > 0 && ws_ints < (int64_t)ptr_gbdt_partition_segments_ws_ints(nblocks)) {
        set_error("%s: workspace too small (%lld int32, %lld needed)", who, (long long)ws_ints, (long long)ptr_gbdt_partition_segments_ws_ints(nblocks));
        return PTR_ERR_INVALID_ARG;
    }
    hipStream_t s = as_stream(stream);
    if (nrows > 0)                                                       // the positions outside every segment; the scatter overwrites the rest
        if (int rc = check_hip(hipMemcpyAsync(out, rows, (size_t)nrows * sizeof(int32_t), hipMemcpyDeviceToDevice, s), who)) return rc;
    if (K == 0) return 0;
    if (int rc = check_hip(hipMemsetAsync(left_counts, 0, (size_t)K * sizeof(int32_t), s), who)) return rc;
    if (nblocks == 0) return 0;
    if (cat_on)
        hipLaunchKernelGGL(gbdt_part_seg_count_kernel<true>, dim3(nblocks), dim3(kBlock), 0, s, bins, stride, (int)n, F, rows, nrows, segs, cols, K, blocks, nblocks, ws, cat);
    else
        hipLaunchKernelGGL(gbdt_part_seg_count_kernel<false>, dim3(nblocks), dim3(kBlock), 0, s, bins, stride, (int)n, F, rows, nrows, segs, cols, K, blocks, nblocks, ws, cat);
    hipLaunchKernelGGL(gbdt_part_scan_kernel, dim3(1), dim3(kBlock), 0, s, ws, nblocks, (int32_t *)nullptr);
    if (cat_on)
        hipLaunchKernelGGL(gbdt_part_seg_scatter_kernel<true>, dim3(nblocks), dim3(kBlock), 0, s, bins, stride, (int)n, F, rows, nrows, segs, cols, K, blocks, nblocks, ws,
                           out, left_counts, cat);
    else
        hipLaunchKernelGGL(gbdt_part_seg_scatter_kernel<false>, dim3(nblocks), dim3(kBlock), 0, s, bins, stride, (int)n, F, rows, nrows, segs, cols, K, blocks, nblocks, ws,
                           out, left_counts, cat);
    return check_hip(hipGetLastError(), who);
}

extern "C" int ptr_gbdt_partition_segments_cat(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t nrows, const int32_t *segs,
                                               const int64_t *sets, int K, const uint8_t *is_cat, const int32_t *nan_bin, const int32_t *blocks,
                                               int nblocks, int32_t *out, int32_t *left_counts, int32_t *ws, int64_t ws_ints, void *stream) {
    return gbdt_partition_segments_impl("ptr_gbdt_partition_segments_cat", bins, stride, n, F, rows, nrows, segs, 5, K, blocks, nblocks, out, left_counts, ws,
                                        ws_ints, stream, true, GbdtCatSegs{is_cat, nan_bin, sets});
}

extern "C" int ptr_gbdt_partition_segments(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t nrows, const int32_t *segs,
                                           int K, const int32_t *blocks, int nblocks, int32_t *out, int32_t *left_counts, int32_t *ws,
                                           int64_t ws_ints, void *stream) {
    return gbdt_partition_segments_impl("ptr_gbdt_partition_segments", bins, stride, n, F, rows, nrows, segs, 4, K, blocks, nblocks, out, left_counts, ws,
                                        ws_ints, stream);
}

extern "C" int ptr_gbdt_partition_segments_missing(const uint8_t *bins, int stride, int64_t n, int F, const int32_t *rows, int64_t nrows,
                                                   const int32_t *segs, int K, const int32_t *blocks, int nblocks, int32_t *out, int32_t *left_counts,
                                                   int32_t *ws, int64_t ws_ints, void *stream) {
    return gbdt_partition_segments_impl("ptr_gbdt_partition_segments_missing", bins, stride, n, F, rows, nrows, segs, 5, K, blocks, nblocks, out,
                                        left_counts, ws, ws_ints, stream);
}
