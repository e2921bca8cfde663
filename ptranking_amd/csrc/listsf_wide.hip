// Wide-head forms of the listsf attention kernels: 128 < head dimension <= PTR_MHSA_MAX_HEAD_DIM = 352 (the reference's stock listsf
// scorer has 2 heads: 350 on the 700 Yahoo! features; one head gives 136 on MSLR-WEB30K, 220 on Istella).
//
// Same formulation, fragment layouts, dropout addressing, `lens` handling and bit-stability rules as the narrow forms (listsf.hip, whose
// header describes them; the shared pieces are in ptr_attn.h), and the same launches per direction: one forward; backward = the row dot
// (listsf.hip), dQ, dK / dV.  What differs is where the head lives.  The narrow forms keep every operand and every accumulator of the
// whole head in registers, staged through index arithmetic that costs registers of its own; at 22 column tiles one operand or one
// accumulator is 88 registers, and the dK / dV kernel would want two operands and two accumulators next to 96 staging registers: that
// spills.  Here every kernel is compiled for one workgroup of 4 waves per CU (the unified 512-entry VGPR + AGPR file) and holds ONE
// operand of head width per wave in registers next to its accumulators (one; dK and dV in the dK / dV kernel):
//   * the streamed operand comes from LDS in chunks of 16 rows (keys forward and in dQ, query rows in dK / dV), prefetched into
//     registers one chunk ahead; the staging is wave-per-row (WideStage), so a chunk is 32 registers per tensor and its addresses and
//     masks a handful;
//   * a SECOND contraction operand, where one is needed, is read from an LDS tile staged once per workgroup: the block's 64 dO rows in
//     the recomputing dQ kernel (dP = dO V^T), the block's 64 V rows in the dK / dV kernel.  LDS: 2 x 16 + 64 rows of up to 1424 bytes
//     (+ 5 KB of dS transpose pads) = 142 KB at the widest head.
// The head dimension is a template parameter DT = column tiles of 16 rounded up to EVEN (10, 12, .. 22: dh <= 160, 192, .. 352).  LDS
// tiles and register operands are zero beyond dh, so the contraction simply runs over all 16 DT columns, as two interleaved MFMA
// chains (even / odd 16-column blocks, each in ascending steps of 4, the two sums added at the end), and the outputs' surplus columns
// are computed and not stored.  Keys / rows are accumulated in ascending order: fixed order, no atomics, repeats are bit-identical.
// Global accesses are 16 bytes wide when dh, the row stride and the pointers allow, 8 bytes when they are even (350: the Yahoo! head),
// 4 otherwise (wide_access_mode).
#include "ptr_attn.h"

namespace ptr {

constexpr int kWideNW = 4, kWideNT = kWideNW * 64;
constexpr int kWideRows = 16 * kWideNW;            // query rows (key rows in dK / dV) per workgroup: one 16-row tile per wave
constexpr int kWideChunk = 16;                     // streamed rows per LDS chunk: one tile

// Widest access the column block of a head allows: 4 floats (dh, the row stride and the pointer multiples of 16 bytes), 2 (of 8 bytes: the
// Yahoo! head of 350 starts 1400 bytes into its row), else 1.  Columns at and beyond dh are never touched: a group of `mode` columns is
// inside or outside the head as a whole.
__device__ __forceinline__ int wide_access_mode(int dh, int stride, const void *p) {
    return wide_access_width(dh, stride, reinterpret_cast<uintptr_t>(p));       // ptr_attn.h
}
using f32x2v = __attribute__((ext_vector_type(2))) float;
// Columns c .. c + 3 of a row, raw: columns at and beyond dh read (a valid) column 0 instead and are zeroed by the caller.
__device__ __forceinline__ f32x4 wide_load4(const float *row, int c, int dh, int mode) {
    f32x4 x;
    if (mode == 4) x = *reinterpret_cast<const f32x4 *>(row + (c < dh ? c : 0));
    else if (mode == 2) {
        const f32x2v lo = *reinterpret_cast<const f32x2v *>(row + (c < dh ? c : 0)), hi = *reinterpret_cast<const f32x2v *>(row + (c + 2 < dh ? c + 2 : 0));
        x = f32x4{lo[0], lo[1], hi[0], hi[1]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = row[c + e < dh ? c + e : 0];
    }
    return x;
}
__device__ __forceinline__ void wide_store4(float *row, int c, int dh, int mode, f32x4 o) {
    if (mode == 4) { if (c < dh) *reinterpret_cast<f32x4 *>(row + c) = o; }
    else if (mode == 2) {
        if (c < dh) *reinterpret_cast<f32x2v *>(row + c) = f32x2v{o[0], o[1]};
        if (c + 2 < dh) *reinterpret_cast<f32x2v *>(row + c + 2) = f32x2v{o[2], o[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (c + e < dh) row[c + e] = o[e];
    }
}

// One operand of head width in registers: lane (j, g) holds columns 16 blk + 4 g .. + 3 of ITS row (zero at and beyond dh, and for a
// row that does not exist: `row` is then a valid clamped pointer and ok = false).
template <int DT>
struct WideOperand {
    f32x4 v[DT];
    __device__ __forceinline__ void load_global(const float *row, bool ok, int dh, int g, int mode) {
#pragma unroll
        for (int blk = 0; blk < DT; ++blk) {
            const int c = 16 * blk + 4 * g;
            f32x4 x = wide_load4(row, c, dh, mode);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] *= (ok && c + e < dh) ? 1.0f : 0.0f;
            v[blk] = x;
        }
    }
    __device__ __forceinline__ f32x4 blk(int b) const { return v[b]; }
};
// The same operand read from a zero-padded LDS tile row (p = row + 4 g).
struct WideLdsOperand {
    const float *p;
    __device__ __forceinline__ f32x4 blk(int b) const { return *reinterpret_cast<const f32x4 *>(p + 16 * b); }
};

// Staging of 16 rows [row0, row0 + 16) of a head's column block into an LDS tile dst[16][LD] (rows >= row_lim and columns >= dh zero).
// Wave w owns rows w, w + 4, w + 8, w + 12, lane l the float4 columns l and l + 64: the row is wave-uniform (scalar address and
// validity), the column masks are the same for every row.  load() issues raw loads only (clamped, always-valid addresses) so that the
// next chunk's loads fly during the MFMAs of the current one; store() applies the zero padding.
template <int LD>
struct WideStage {
    static constexpr int LD4 = LD / 4, NQ = LD4 > 64 ? 2 : 1;
    static_assert(LD4 <= 128, "two float4 columns per lane");
    f32x4 v[4][NQ];
    __device__ __forceinline__ void load(const float *src, int stride, int dh, int row0, int row_lim, int wave, int lane) {
        const int mode = wide_access_mode(dh, stride, src);
        const int last = row_lim > 0 ? row_lim - 1 : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = row0 + wave + 4 * i;
            const float *p = src + (size_t)(r < row_lim ? r : last) * stride;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                v[i][q] = wide_load4(p, 4 * (lane + 64 * q), dh, mode);
            }
        }
    }
    __device__ __forceinline__ void store(float *dst, int dh, int row0, int row_lim, int wave, int lane) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int lr = wave + 4 * i;
            const bool rok = row0 + lr < row_lim;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = 4 * (lane + 64 * q);
                if (c < LD) {
                    f32x4 t = v[i][q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] *= (rok && c + e < dh) ? 1.0f : 0.0f;
                    *reinterpret_cast<f32x4 *>(dst + (size_t)lr * LD + c) = t;
                }
            }
        }
    }
};

// out[r] = sum_d A[4 g + r][d] * B[j][d] over the 16 DT (zero-padded) columns: A = the 16-row LDS tile As, B = this lane's operand row.
template <int DT, class BOp>
__device__ __forceinline__ f32x4 wide_dot(const float *As, int ld, int j, int g, const BOp &b) {
    static_assert(DT % 2 == 0, "two chains of 16-column blocks");
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
    const float *ap = As + (size_t)j * ld + 4 * g;
#pragma unroll
    for (int bp = 0; bp < DT / 2; ++bp) {
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(ap + 32 * bp), a1 = *reinterpret_cast<const f32x4 *>(ap + 32 * bp + 16);
        const f32x4 b0 = b.blk(2 * bp), b1 = b.blk(2 * bp + 1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            c0 = mfma4(a0[c], b0[c], c0);
            c1 = mfma4(a1[c], b1[c], c1);
        }
    }
    return c0 + c1;
}

// acc[dt]^T[d = 16 dt + j][n] += sum over the 16 tile rows of A[row][d] * b[row][n]: row 4 g + r of the LDS tile As is k-slot g of step r,
// where lane (j, g) holds b[r] for it.
template <int DT>
__device__ __forceinline__ void wide_accum(const float *As, int ld, int j, int g, const f32x4 &b, f32x4 (&acc)[DT]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float *arow = As + (size_t)(4 * g + r) * ld + j;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[dt] = mfma4(arow[16 * dt], b[r], acc[dt]);
    }
}

// One output row per lane j: columns 16 dt + 4 g .. + 3 of acc[dt] * scale, for the columns that exist.
template <int DT>
__device__ __forceinline__ void wide_store_row(float *dst, const f32x4 (&acc)[DT], float scale, int dh, int g, int mode) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) wide_store4(dst, 16 * dt + 4 * g, dh, mode, acc[dt] * scale);
}

// The indices every kernel derives from its block id: (query, head) bh, block rb of 64 rows (or keys), the list's length n.
struct WideBlock {
    int rb, bh, b, h, n;
    size_t base, obase;                // first element of the head's column block in Q / K / V (stride a.ld) and in O / dO (stride F)
};
__device__ __forceinline__ WideBlock wide_block(const AttnArgs &a, const int32_t *lens) {
    WideBlock w;
    const int nrb = (a.L + kWideRows - 1) / kWideRows;
    const int lid = xcd_major_block_id();
    w.rb = lid % nrb; w.bh = lid / nrb; w.b = w.bh / a.H; w.h = w.bh - w.b * a.H;
    const int n = lens ? lens[w.b] : a.L;
    w.n = n < 0 ? 0 : (n > a.L ? a.L : n);
    w.base = (size_t)w.b * a.L * a.ld + (size_t)w.h * a.dh;
    w.obase = (size_t)w.b * a.L * a.F + (size_t)w.h * a.dh;
    return w;
}

// ============================================================================================ forward
template <int DT>
__global__ void __launch_bounds__(kWideNT, 1)
mhsa_wide_fwd_kernel(const float *__restrict__ Q, const float *__restrict__ K, const float *__restrict__ V,
                     const int32_t *__restrict__ lens, AttnArgs a, float *__restrict__ O, float *__restrict__ LSE) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ld = attn_ld(DT), KC = kWideChunk;
    float *Ks = smem, *Vs = Ks + (size_t)KC * ld;
    const int L = a.L, F = a.F, dh = a.dh, ldi = a.ld;
    const WideBlock w = wide_block(a, lens);
    const int n = w.n, bh = w.bh;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int row = w.rb * kWideRows + wave * 16 + j;
    const bool rok = row < L;

    const uint32_t thr = drop_thr(a.p_drop);
    float m = -INFINITY, l = 0.0f;
    f32x4 acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    WideOperand<DT> qr;
    qr.load_global(Q + w.base + (size_t)(rok ? row : L - 1) * ldi, rok, dh, g, wide_access_mode(dh, ldi, Q + w.base));

    WideStage<ld> kst, vst;
    kst.load(K + w.base, ldi, dh, 0, n, wave, lane);
    vst.load(V + w.base, ldi, dh, 0, n, wave, lane);
    for (int kc = 0; kc < n; kc += KC) {
        __syncthreads();                                   // every wave is done with the previous chunk
        kst.store(Ks, dh, kc, n, wave, lane);
        vst.store(Vs, dh, kc, n, wave, lane);
        __syncthreads();
        if (kc + KC < n) {                                // prefetch the next chunk while this one is consumed
            kst.load(K + w.base, ldi, dh, kc + KC, n, wave, lane);
            vst.load(V + w.base, ldi, dh, kc + KC, n, wave, lane);
        }
        f32x4 p = wide_dot<DT>(Ks, ld, j, g, qr);          // p[r] = S[row j][key kc + 4 g + r]
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = kc + 4 * g + r < n ? p[r] * a.inv_scale : -INFINITY;                     // list_ranker.py:223
            mx = fmaxf(mx, p[r]);
        }
        mx = xor_max(mx);
        const float m_new = fmaxf(m, mx);
        const float corr = __expf(m - m_new);
        float rs = 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { p[r] = __expf(p[r] - m_new); rs += p[r]; }
        if (thr != 0) {                                                                     // list_ranker.py:229
            uint32_t w0, w1;
            drop_bits(a.seed_lo, a.seed_hi, a.site, bh * L + row, (kc + 4 * g) >> 2, w0, w1);
            p = drop4(p, w0, w1, thr, 1.0f);
        }
        rs = xor_sum(rs);
        l = l * corr + rs;
        m = m_new;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[dt] *= corr;
        wide_accum<DT>(Vs, ld, j, g, p, acc);              // O^T[d][row] += V^T[d][key] * P^T[key][row]      (list_ranker.py:236)
    }
    if (!rok) return;
    const float keep_inv = thr != 0 ? 1.0f / (1.0f - a.p_drop) : 1.0f;
    wide_store_row<DT>(O + w.obase + (size_t)row * F, acc, l > 0.0f ? keep_inv / l : 0.0f, dh, g, wide_access_mode(dh, F, O + w.obase));
    if (g == 0) LSE[(size_t)bh * L + row] = l > 0.0f ? m + __logf(l) : 0.0f;
}

// ============================================================================================ backward: dQ (recomputing S and dP)
template <int DT>
__global__ void __launch_bounds__(kWideNT, 1)
mhsa_wide_bwd_dq_kernel(const float *__restrict__ Q, const float *__restrict__ K, const float *__restrict__ V,
                        const float *__restrict__ dO, const float *__restrict__ LSE, const float *__restrict__ Dv,
                        const int32_t *__restrict__ lens, AttnArgs a, float *__restrict__ dQ) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ld = attn_ld(DT), KC = kWideChunk;
    float *Gs = smem, *Ks = Gs + (size_t)kWideRows * ld, *Vs = Ks + (size_t)KC * ld;       // Gs: the block's 64 dO rows, for the whole kernel
    const int L = a.L, F = a.F, dh = a.dh, ldi = a.ld;
    const WideBlock w = wide_block(a, lens);
    const int n = w.n, bh = w.bh;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int row0 = w.rb * kWideRows, row = row0 + wave * 16 + j;
    const bool rok = row < L;
    const float lse = rok ? LSE[(size_t)bh * L + row] : 0.0f;
    const float Dr = rok ? Dv[(size_t)bh * L + row] : 0.0f;
    const uint32_t thr = drop_thr(a.p_drop);
    const float keep_inv = thr != 0 ? 1.0f / (1.0f - a.p_drop) : 1.0f;
    f32x4 dq[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    WideOperand<DT> qr;
    qr.load_global(Q + w.base + (size_t)(rok ? row : L - 1) * ldi, rok, dh, g, wide_access_mode(dh, ldi, Q + w.base));
    WideStage<ld> kst, vst;
#pragma unroll 1
    for (int t = 0; t < kWideRows / 16; ++t) {             // the barrier of the first chunk below publishes Gs
        kst.load(dO + w.obase, F, dh, row0 + 16 * t, L, wave, lane);
        kst.store(Gs + (size_t)16 * t * ld, dh, row0 + 16 * t, L, wave, lane);
    }
    const WideLdsOperand gr = {Gs + (size_t)(wave * 16 + j) * ld + 4 * g};

    kst.load(K + w.base, ldi, dh, 0, n, wave, lane);
    vst.load(V + w.base, ldi, dh, 0, n, wave, lane);
    for (int kc = 0; kc < n; kc += KC) {
        __syncthreads();
        kst.store(Ks, dh, kc, n, wave, lane);
        vst.store(Vs, dh, kc, n, wave, lane);
        __syncthreads();
        if (kc + KC < n) {
            kst.load(K + w.base, ldi, dh, kc + KC, n, wave, lane);
            vst.load(V + w.base, ldi, dh, kc + KC, n, wave, lane);
        }
        const f32x4 s = wide_dot<DT>(Ks, ld, j, g, qr), dp = wide_dot<DT>(Vs, ld, j, g, gr);
        f32x4 keep = {keep_inv, keep_inv, keep_inv, keep_inv}, ds;
        if (thr != 0) {
            uint32_t w0, w1;
            drop_bits(a.seed_lo, a.seed_hi, a.site, bh * L + row, (kc + 4 * g) >> 2, w0, w1);
            keep = drop4(keep, w0, w1, thr, 1.0f);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pr = (kc + 4 * g + r < n && rok) ? __expf(s[r] * a.inv_scale - lse) : 0.0f;
            ds[r] = pr * (dp[r] * keep[r] - Dr) * a.inv_scale;
        }
        wide_accum<DT>(Ks, ld, j, g, ds, dq);               // dQ^T[d][row] += K^T[d][key] * dS^T[key][row]
    }
    if (!rok) return;
    wide_store_row<DT>(dQ + w.base + (size_t)row * ldi, dq, 1.0f, dh, g, wide_access_mode(dh, ldi, dQ + w.base));
}

// ============================================================================================ backward: dQ from the stored dS
// One GEMM unit, dQ^T[d][row] = sum_key K^T[d][key] * dS^T[key][row]; keys >= n are SELECTED to zero (listsf.hip mhsa_bwd_dq_ds_kernel).
template <int DT>
__global__ void __launch_bounds__(kWideNT, 1)
mhsa_wide_bwd_dq_ds_kernel(const float *__restrict__ K, const float *__restrict__ dS_ws, const int32_t *__restrict__ lens, AttnArgs a,
                           float *__restrict__ dQ) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ld = attn_ld(DT), KC = kWideChunk;
    float *Ks = smem;
    const int L = a.L, dh = a.dh, ldi = a.ld;
    const WideBlock w = wide_block(a, lens);
    const int n = w.n;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int row = w.rb * kWideRows + wave * 16 + j;
    const bool rok = row < L;
    const float *dsrow = dS_ws + ((size_t)w.bh * L + (rok ? row : L - 1)) * L;
    const bool vds = (L & 3) == 0 && (reinterpret_cast<uintptr_t>(dS_ws) & 15) == 0;
    f32x4 dq[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    WideStage<ld> kst;
    kst.load(K + w.base, ldi, dh, 0, n, wave, lane);
    auto load_ds = [&](int kc) {
        const int k0 = kc + 4 * g;
        f32x4 d;
        if (vds) d = *reinterpret_cast<const f32x4 *>(dsrow + (k0 + 3 < L ? k0 : 0));
        else {
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = dsrow[k0 + r < L ? k0 + r : 0];
        }
        return d;
    };
    f32x4 dsn = load_ds(0);
    for (int kc = 0; kc < n; kc += KC) {
        __syncthreads();
        kst.store(Ks, dh, kc, n, wave, lane);
        __syncthreads();
        f32x4 ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) ds[r] = (rok && kc + 4 * g + r < n) ? dsn[r] : 0.0f;
        if (kc + KC < n) { kst.load(K + w.base, ldi, dh, kc + KC, n, wave, lane); dsn = load_ds(kc + KC); }
        wide_accum<DT>(Ks, ld, j, g, ds, dq);
    }
    if (!rok) return;
    wide_store_row<DT>(dQ + w.base + (size_t)row * ldi, dq, 1.0f, dh, g, wide_access_mode(dh, ldi, dQ + w.base));
}

// ============================================================================================ backward: dK, dV
// One workgroup per (query, head, block of 64 keys), a wave per key tile; Q and dO rows stream through LDS in chunks of 16.
//   S[row][key] from the wave's K rows (registers) and the staged Q rows, dP = dO V^T against the block's V rows in LDS;
//   Pdrop = P * keep                          dV^T[d][key] += dO^T[d][row] * Pdrop[row][key]
//   dS = P * (dP * keep - D) / sqrt(dh)       dK^T[d][key] += Q^T[d][row]  * dS[row][key]
// STORE_DS also hands dS to mhsa_wide_bwd_dq_ds_kernel (transposed through a wave-private LDS pad so that every lane stores one float4
// of 4 consecutive keys of its row, as in listsf.hip).
template <int DT, bool STORE_DS>
__global__ void __launch_bounds__(kWideNT, 1)
mhsa_wide_bwd_dkv_kernel(const float *__restrict__ Q, const float *__restrict__ K, const float *__restrict__ V,
                         const float *__restrict__ dO, const float *__restrict__ LSE, const float *__restrict__ Dv,
                         const int32_t *__restrict__ lens, AttnArgs a, float *__restrict__ dK, float *__restrict__ dV,
                         float *__restrict__ dS_ws /* STORE_DS: [B*H][L][L] */) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ld = attn_ld(DT), RC = kWideChunk;
    float *Qs = smem, *Gs = Qs + (size_t)RC * ld;
    float *Vt = Gs + (size_t)RC * ld;                     // the block's 64 V rows, for the whole kernel
    float *lse_s = Vt + (size_t)kWideRows * ld, *D_s = lse_s + RC;
    float *ds_pad = D_s + RC;                             // [NW][16][kDsPadLd] wave-private transpose pads of the dS tiles
    const int L = a.L, F = a.F, dh = a.dh, ldi = a.ld;
    const WideBlock w = wide_block(a, lens);
    const int n = w.n, bh = w.bh;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    const int key0 = w.rb * kWideRows, wkey = wave * 16;
    const int key = key0 + wkey + j;
    const uint32_t thr = drop_thr(a.p_drop);
    const float keep_inv = thr != 0 ? 1.0f / (1.0f - a.p_drop) : 1.0f;
    f32x4 dk[DT], dv[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const bool live = key0 < n;                            // a block of padded keys only writes zeros

    WideStage<ld> qst, gst;
    float lse_pf = 0.0f, d_pf = 0.0f;
    auto prefetch = [&](int rc) {
        qst.load(Q + w.base, ldi, dh, rc, L, wave, lane);
        gst.load(dO + w.obase, F, dh, rc, L, wave, lane);
        if (tid < RC) {
            const int row = rc + tid, rcl = row < L ? row : L - 1;     // raw loads; rows >= L are masked where they are used
            lse_pf = LSE[(size_t)bh * L + rcl];
            d_pf = Dv[(size_t)bh * L + rcl];
        }
    };
    WideOperand<DT> kr;                                    // this wave's 16 keys as the B operand of S, for the whole kernel
    kr.load_global(K + w.base + (size_t)(key < L ? key : L - 1) * ldi, key < n, dh, g, wide_access_mode(dh, ldi, K + w.base));
    if (live) {
#pragma unroll 1
        for (int t = 0; t < kWideRows / 16; ++t) {         // keys >= n are zero rows; the barrier of the first chunk below publishes Vt
            qst.load(V + w.base, ldi, dh, key0 + 16 * t, n, wave, lane);
            qst.store(Vt + (size_t)16 * t * ld, dh, key0 + 16 * t, n, wave, lane);
        }
        prefetch(0);
    }
    const WideLdsOperand vr = {Vt + (size_t)(wkey + j) * ld + 4 * g};
    for (int rc = 0; live && rc < L; rc += RC) {
        __syncthreads();
        qst.store(Qs, dh, rc, L, wave, lane);
        gst.store(Gs, dh, rc, L, wave, lane);
        if (tid < RC) { lse_s[tid] = lse_pf; D_s[tid] = d_pf; }
        __syncthreads();
        if (rc + RC < L) prefetch(rc + RC);
        // S[row][key], dP[row][key] for the chunk's row tile: lane (j, g), reg r = row rc + 4 g + r, key j
        const f32x4 s = wide_dot<DT>(Qs, ld, j, g, kr), dp = wide_dot<DT>(Gs, ld, j, g, vr);
        f32x4 pd, ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lr = 4 * g + r, row = rc + lr;
            const float pr = (key < n && row < L) ? __expf(s[r] * a.inv_scale - lse_s[lr]) : 0.0f;
            float keep = keep_inv;
            if (thr != 0) keep = drop_keep1(a.seed_lo, a.seed_hi, a.site, bh * L + row, key, thr) ? keep_inv : 0.0f;
            pd[r] = pr * keep;
            ds[r] = pr * (dp[r] * keep - D_s[lr]) * a.inv_scale;
        }
        if constexpr (STORE_DS) {
            float *T = ds_pad + wave * (16 * kDsPadLd);
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 4; ++r) T[(4 * g + r) * kDsPadLd + j] = ds[r];
            wave_lds_sync();
            const f32x4 t4 = *reinterpret_cast<const f32x4 *>(T + j * kDsPadLd + 4 * g);           // row rc + j, keys 4 g .. 4 g + 3 of the tile
            const int srow = rc + j, skey = key0 + wkey + 4 * g;
            if (srow < L) {
                float *dst = dS_ws + ((size_t)bh * L + srow) * L + skey;
                if (skey + 3 < L && ((L & 3) == 0)) *reinterpret_cast<f32x4 *>(dst) = t4;
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (skey + e < L) dst[e] = t4[e];
                }
            }
        }
        wide_accum<DT>(Gs, ld, j, g, pd, dv);
        wide_accum<DT>(Qs, ld, j, g, ds, dk);
    }
    if (key >= L) return;
    wide_store_row<DT>(dK + w.base + (size_t)key * ldi, dk, 1.0f, dh, g, wide_access_mode(dh, ldi, dK + w.base));
    wide_store_row<DT>(dV + w.base + (size_t)key * ldi, dv, 1.0f, dh, g, wide_access_mode(dh, ldi, dV + w.base));
}

// ============================================================================================ host
constexpr int kWideMaxDT = 22;
static_assert(PTR_MHSA_MAX_HEAD_DIM == 16 * kWideMaxDT, "the widest form is the public limit");

// Calls f.template operator()<DT>() for the D of a wide attn_form (ptr_attn.h): head dimensions 129 .. 352.
template <class Fn> inline int dispatch_wide_dt(int DT, Fn &&f) {
    switch (DT) {
        case 10: return f.template operator()<10>();
        case 12: return f.template operator()<12>();
        case 14: return f.template operator()<14>();
        case 16: return f.template operator()<16>();
        case 18: return f.template operator()<18>();
        case 20: return f.template operator()<20>();
        default: return f.template operator()<kWideMaxDT>();
    }
}

template <class K, class... Args>
static int wide_launch(K kern, const AttnArgs &a, int lds_rows, int DT, size_t lds_extra, hipStream_t st, const char *who, Args... args) {
    const size_t lds = ((size_t)lds_rows * attn_ld(DT) + lds_extra) * sizeof(float);
    if (int e = allow_lds(kern, lds)) return e;
    const size_t nblk = (size_t)a.B * a.H * ((a.L + kWideRows - 1) / kWideRows);       // row blocks and key blocks are both 64 wide
    hipLaunchKernelGGL(kern, dim3((unsigned)nblk), dim3(kWideNT), lds, st, args...);
    return check_hip(hipGetLastError(), who);
}

int mhsa_wide_forward(int DT, const float *Q, const float *K, const float *V, const int32_t *lens, const AttnArgs &a, float *O, float *LSE,
                      hipStream_t st, const char *who) {
    return dispatch_wide_dt(DT, [&]<int D>() -> int {
        return wide_launch(mhsa_wide_fwd_kernel<D>, a, 2 * kWideChunk, D, 0, st, who, Q, K, V, lens, a, O, LSE);
    });
}

int mhsa_wide_backward(int DT, const float *Q, const float *K, const float *V, const float *dO, const float *LSE, const float *Dv,
                       const int32_t *lens, const AttnArgs &a, float *dQ, float *dK, float *dV, float *ds_ws, hipStream_t st, const char *who) {
    return dispatch_wide_dt(DT, [&]<int D>() -> int {
        constexpr size_t extra = 2 * kWideChunk + kWideNW * 16 * kDsPadLd;                // lse_s, D_s, the dS transpose pads
        auto dkv = [&](auto kern) -> int {
            return wide_launch(kern, a, 2 * kWideChunk + kWideRows, D, extra, st, who, Q, K, V, dO, LSE, Dv, lens, a, dK, dV, ds_ws);
        };
        if (ds_ws) {   // dK / dV first (it writes dS), then dQ as ONE GEMM unit from the stored dS
            if (int rc = dkv(mhsa_wide_bwd_dkv_kernel<D, true>)) return rc;
            return wide_launch(mhsa_wide_bwd_dq_ds_kernel<D>, a, kWideChunk, D, 0, st, who, K, ds_ws, lens, a, dQ);
        }
        if (int rc = wide_launch(mhsa_wide_bwd_dq_kernel<D>, a, kWideRows + 2 * kWideChunk, D, 0, st, who, Q, K, V, dO, LSE, Dv, lens, a, dQ))
            return rc;
        return dkv(mhsa_wide_bwd_dkv_kernel<D, false>);
    });
}

}  // namespace ptr
