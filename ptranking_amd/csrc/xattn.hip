// Rectangular attention (Lq != Lk) with one SHORT side, for SetRank's induced self-attention blocks (setrank.py): documents attend to M
// inducing points (short keys) and the inducing points attend to the documents (short queries), M = min(Lq, Lk) <= 64, head <= 128.
//
//   O[b, i, h] = softmax_j( Q[b, i, h] . K[b, j, h] / sqrt(d_h) ) V[b, j, h],   i < Lq, j < Lk,   lse [B][H][Lq]
//
// Work split: ONE workgroup of four waves per (query b, head h).  The short side's head slice (two operands of at most 64 x 128 fp32) is
// staged into LDS once, zero-padded to 16-row and 16-column tiles; the waves stride over 16-row tiles of the long side, which is read from
// HBM once per kernel straight into MFMA operand registers (OperandRegs, ptr_attn.h) — there is no L^2 and no L x M tensor anywhere.
// All products are v_mfma_f32_16x16x4_f32 in the operand layouts of listsf.hip ("transposed world"): with lane (j = l & 15, g = l >> 4),
//   multi_dot(LDS, regs)   -> C[short row 16 kt + 4 g + r][long row j]     (lane = a long-side row, registers = short-side rows)
//   dot_swapped(regs, LDS) -> C[long row 4 g + r][short row 16 kt + j]     (lane = a short-side row, registers = long-side rows)
// and whichever has lane = QUERY row puts the softmax statistics of a row into one lane group (in-lane over r, two shuffles over g).
//   short keys, forward     S^T = multi_dot(K_lds, q): the whole 16 x M score tile in at most 4 f32x4 per lane -> one-pass softmax in registers,
//                           O^T += V_lds^T P^T with P as the B operand as it stands.  No rescaling.
//   short queries, forward  S^T = dot_swapped(k, Q_lds): lane = query row; every wave keeps (max, sum, O^T accumulators) for the M query rows over
//                           ITS key tiles (online softmax; V rows come from global in A-operand layout, each element read by one lane), then the
//                           four partial states are merged through LDS in wave order 0, 1, 2, 3.
//   backward (both)         P = exp(S - lse), dS = P (dP - D) / sqrt(d_h) in the multi_dot layout.  The long side's gradient is one more product
//                           against the LDS-resident operand and is stored tile by tile.  The short side's gradient is a reduction over the long
//                           side: P / dS tiles are transposed through a wave-private LDS pad (so that lane = short row), multiplied with the
//                           tile's rows read from global as A operands into per-wave MFMA accumulators, and the four waves' accumulators are
//                           summed through LDS in wave order.
// Determinism: no atomics; every output element has one owner and every cross-wave sum a fixed order, so a query's bits depend only on its own
// data and on (Lq, Lk, F, H).  Masking is by selection: keys >= lens_k[b] get P = 0, query rows >= lens_q[b] give O = 0, lse = 0 exactly and
// add nothing to dK / dV; their dQ rows are exact zeros.
#include <stdlib.h>

#include "ptr_attn.h"
#include "ptr_device.h"

namespace ptr {

constexpr int kXW = 4, kXNT = kXW * 64;          // waves and threads of a workgroup

struct XArgs {
    int B, Lq, Lk, H, dh, F;
    int ld_q, ld_kv;                   // row strides (floats) of Q and of K / V (and dK / dV); O, dO, dQ are [B][Lq][F]
    long long qbs;                     // batch stride of Q in floats; 0: one [Lq][ld_q] Q shared by every query
    float inv_scale;                   // 1 / sqrt(dh)
};

struct XBlock {                        // what every kernel derives from its block index
    int b, h, bh, nq, nk, tid, wave, j, g, nb, rem;
};
__device__ __forceinline__ XBlock xblock(const XArgs &a, const int32_t *lens_q, const int32_t *lens_k) {
    XBlock x;
    x.bh = blockIdx.x; x.b = x.bh / a.H; x.h = x.bh - x.b * a.H;
    int nq = lens_q ? lens_q[x.b] : a.Lq, nk = lens_k ? lens_k[x.b] : a.Lk;
    x.nq = nq < 0 ? 0 : (nq > a.Lq ? a.Lq : nq);
    x.nk = nk < 0 ? 0 : (nk > a.Lk ? a.Lk : nk);
    x.tid = threadIdx.x; x.wave = x.tid >> 6; x.j = x.tid & 15; x.g = (x.tid & 63) >> 4;
    const int dh4 = (a.dh + 3) & ~3;
    x.nb = dh4 >> 4; x.rem = (dh4 & 15) >> 2;
    return x;
}

// rows [0, nvalid) of a head slice -> dst[rows][ld], everything else (rows up to `rows`, columns >= dh) zero
__device__ __forceinline__ void stage_short(float *dst, int ld, int rows, const float *src, int stride, int dh, int nvalid, int tid) {
    for (int idx = tid; idx < rows * ld; idx += kXNT) {
        const int r = idx / ld, c = idx - r * ld;
        dst[idx] = (r < nvalid && c < dh) ? src[(size_t)r * stride + c] : 0.0f;
    }
}

// acc[ia][r] = sum_d A[4 g + r][d] * B[16 ia + j][d]: the tile's rows (registers) as the A operand, NA LDS tiles as B.
template <int DT, int NA>
__device__ __forceinline__ void dot_swapped(const float *Bs, int ld, int nb, int rem, int j, int g, const OperandRegs<DT> &a, f32x4 (&acc)[NA]) {
#pragma unroll
    for (int ia = 0; ia < NA; ++ia) acc[ia] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float *bp = Bs + (size_t)j * ld;
#pragma unroll
    for (int blk = 0; blk < DT; ++blk) {
        if (blk < nb) {
            f32x4 b[NA];
#pragma unroll
            for (int ia = 0; ia < NA; ++ia) b[ia] = *reinterpret_cast<const f32x4 *>(bp + (size_t)16 * ia * ld + 16 * blk + 4 * g);
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int ia = 0; ia < NA; ++ia) acc[ia] = mfma4(a.v[blk][c], b[ia][c], acc[ia]);
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (i < rem) {
            const int d = 16 * nb + 4 * i + g;
#pragma unroll
            for (int ia = 0; ia < NA; ++ia) acc[ia] = mfma4(a.t[i], bp[(size_t)16 * ia * ld + d], acc[ia]);
        }
    }
}

// A 16 x 16 tile in C layout, x[r] = T[4 g + r][j]  ->  T[j][4 g .. 4 g + 3], through the wave's own pad (kDsPadLd floats per row).
__device__ __forceinline__ f32x4 tile_transpose(float *pad, int j, int g, f32x4 x) {
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) pad[(4 * g + r) * kDsPadLd + j] = x[r];
    wave_lds_sync();
    return *reinterpret_cast<const f32x4 *>(pad + j * kDsPadLd + 4 * g);
}

__device__ __forceinline__ void store4(float *dst, int d, int dh, bool vec, f32x4 v) {
    if (vec) { if (d < dh) *reinterpret_cast<f32x4 *>(dst) = v; }
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (d + e < dh) dst[e] = v[e];
    }
}

// The waves' accumulators acc[kt][dt] (lane = short row 16 kt + j, columns 16 dt + 4 g ..) summed into dst[16 MT][ld] in wave order.
template <int DT, int MT>
__device__ __forceinline__ void reduce_waves(float *dst, int ld, int wave, int j, int g, const f32x4 (&acc)[MT][DT]) {
    __syncthreads();                                       // every wave is done with what dst held
    for (int w = 0; w < kXW; ++w) {
        if (wave == w) {
#pragma unroll
            for (int kt = 0; kt < MT; ++kt)
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    f32x4 *p = reinterpret_cast<f32x4 *>(dst + (size_t)(16 * kt + j) * ld + 16 * dt + 4 * g);
                    *p = w == 0 ? acc[kt][dt] : *p + acc[kt][dt];
                }
        }
        __syncthreads();
    }
}

// ============================================================================================ forward, short keys
template <int DT, int MT>
__global__ void __launch_bounds__(kXNT)
xattn_fwd_sk_kernel(const float *__restrict__ Q, const float *__restrict__ K, const float *__restrict__ V, const int32_t *__restrict__ lens_q,
                    const int32_t *__restrict__ lens_k, XArgs a, float *__restrict__ O, float *__restrict__ LSE) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ld = attn_ld(DT);
    float *Ks = smem, *Vs = Ks + 16 * MT * ld;
    const XBlock x = xblock(a, lens_q, lens_k);
    const int j = x.j, g = x.g, dh = a.dh, Lq = a.Lq;
    const float *Qb = Q + (size_t)x.b * a.qbs + (size_t)x.h * dh;
    const size_t kvbase = (size_t)x.b * a.Lk * a.ld_kv + (size_t)x.h * dh;
    float *Ob = O + (size_t)x.b * Lq * a.F + (size_t)x.h * dh;
    stage_short(Ks, ld, 16 * MT, K + kvbase, a.ld_kv, dh, x.nk, x.tid);
    stage_short(Vs, ld, 16 * MT, V + kvbase, a.ld_kv, dh, x.nk, x.tid);
    __syncthreads();
    const bool vecq = ATTN_FLOAT4_ROWS(dh, a.ld_q, Qb), veco = ATTN_FLOAT4_ROWS(dh, a.F, Ob);
    for (int t = x.wave; 16 * t < Lq; t += kXW) {
        const int row = 16 * t + j;
        const bool rok = row < x.nq;
        OperandRegs<DT> qr[1];
        qr[0].load_global(Qb + (size_t)(row < Lq ? row : Lq - 1) * a.ld_q, rok, dh, x.nb, x.rem, g, vecq);
        f32x4 s[1][MT];
        multi_dot<DT, MT, 1>(Ks, 0, ld, x.nb, x.rem, j, g, qr, s);
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < MT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = 16 * kt + 4 * g + r < x.nk ? s[0][kt][r] * a.inv_scale : -INFINITY;
                s[0][kt][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = xor_max(mx);
        const float m = mx == -INFINITY ? 0.0f : mx;       // no key at all: every exp below is 0
        float l = 0.0f;
#pragma unroll
        for (int kt = 0; kt < MT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { s[0][kt][r] = __expf(s[0][kt][r] - m); l += s[0][kt][r]; }
        l = xor_sum(l);
        f32x4 acc[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // O^T[d][row] += V^T[d][key] * P^T[key][row]
#pragma unroll
        for (int kt = 0; kt < MT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *vrow = Vs + (size_t)(16 * kt + 4 * g + r) * ld + j;
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) acc[dt] = mfma4(vrow[16 * dt], s[0][kt][r], acc[dt]);
            }
        if (row >= Lq) continue;
        const bool live = rok && l > 0.0f;
        const float inv = live ? 1.0f / l : 0.0f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const f32x4 o = live ? acc[dt] * inv : f32x4{0.f, 0.f, 0.f, 0.f};
            store4(Ob + (size_t)row * a.F + 16 * dt + 4 * g, 16 * dt + 4 * g, dh, veco, o);
        }
        if (g == 0) LSE[(size_t)x.bh * Lq + row] = live ? m + __logf(l) : 0.0f;
    }
}

// ============================================================================================ forward, short queries
template <int DT, int MT>
__global__ void __launch_bounds__(kXNT)
xattn_fwd_sq_kernel(const float *__restrict__ Q, const float *__restrict__ K, const float *__restrict__ V, const int32_t *__restrict__ lens_q,
                    const int32_t *__restrict__ lens_k, XArgs a, float *__restrict__ O, float *__restrict__ LSE) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ld = attn_ld(DT);
    float *Qs = smem, *m_s = Qs + 16 * MT * ld, *l_s = m_s + 16 * MT;     // Qs becomes the merged O^T accumulators after the key loop
    const XBlock x = xblock(a, lens_q, lens_k);
    const int j = x.j, g = x.g, dh = a.dh, Lq = a.Lq, Lk = a.Lk;
    const float *Qb = Q + (size_t)x.b * a.qbs + (size_t)x.h * dh;
    const float *Kb = K + (size_t)x.b * Lk * a.ld_kv + (size_t)x.h * dh, *Vb = V + (size_t)x.b * Lk * a.ld_kv + (size_t)x.h * dh;
    float *Ob = O + (size_t)x.b * Lq * a.F + (size_t)x.h * dh;
    stage_short(Qs, ld, 16 * MT, Qb, a.ld_q, dh, x.nq, x.tid);
    __syncthreads();
    const bool veck = ATTN_FLOAT4_ROWS(dh, a.ld_kv, Kb);
    float m[MT], l[MT];
    f32x4 acc[MT][DT];
#pragma unroll
    for (int kt = 0; kt < MT; ++kt) {
        m[kt] = -INFINITY; l[kt] = 0.0f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int t = x.wave; 16 * t < x.nk; t += kXW) {        // key 16 t exists, so every query row sees a finite score in this tile
        const int key = 16 * t + j;
        OperandRegs<DT> kr;
        kr.load_global(Kb + (size_t)(key < Lk ? key : Lk - 1) * a.ld_kv, key < x.nk, dh, x.nb, x.rem, g, veck);
        f32x4 p[MT];                                       // S^T[key 16 t + 4 g + r][query row 16 kt + j]
        dot_swapped<DT, MT>(Qs, ld, x.nb, x.rem, j, g, kr, p);
#pragma unroll
        for (int kt = 0; kt < MT; ++kt) {
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = 16 * t + 4 * g + r < x.nk ? p[kt][r] * a.inv_scale : -INFINITY;
                p[kt][r] = v;
                mx = fmaxf(mx, v);
            }
            const float m_new = fmaxf(m[kt], xor_max(mx));
            const float corr = __expf(m[kt] - m_new);
            float rs = 0.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) { p[kt][r] = __expf(p[kt][r] - m_new); rs += p[kt][r]; }
            l[kt] = l[kt] * corr + xor_sum(rs);
            m[kt] = m_new;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) acc[kt][dt] *= corr;
        }
        // O^T[d][query row] += V^T[d][key] * P^T[key][query row]: V[key 16 t + 4 g + r][16 dt + j] straight from global, one lane per element
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int vk = 16 * t + 4 * g + r;
            const float *vrow = Vb + (size_t)(vk < Lk ? vk : Lk - 1) * a.ld_kv;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int d = 16 * dt + j;
                const float raw = vrow[d < dh ? d : 0];
                const float va = (d < dh && vk < x.nk) ? raw : 0.0f;
#pragma unroll
                for (int kt = 0; kt < MT; ++kt) acc[kt][dt] = mfma4(va, p[kt][r], acc[kt][dt]);
            }
        }
    }
    // merge the four waves' (m, l, O^T) in wave order
    __syncthreads();
    for (int w = 0; w < kXW; ++w) {
        if (x.wave == w) {
#pragma unroll
            for (int kt = 0; kt < MT; ++kt) {
                const int q = 16 * kt + j;
                float co = 0.0f, cw = 1.0f, mn = m[kt], ln = l[kt];
                if (w > 0) {
                    const float mo = m_s[q], lo = l_s[q];
                    mn = fmaxf(mo, m[kt]);
                    co = mo == -INFINITY ? 0.0f : __expf(mo - mn);
                    cw = m[kt] == -INFINITY ? 0.0f : __expf(m[kt] - mn);
                    ln = lo * co + l[kt] * cw;
                }
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    f32x4 *po = reinterpret_cast<f32x4 *>(Qs + (size_t)q * ld + 16 * dt + 4 * g);
                    *po = w == 0 ? acc[kt][dt] : *po * co + acc[kt][dt] * cw;
                }
                wave_lds_sync();                           // every lane group has read m_s / l_s before g == 0 replaces them
                if (g == 0) { m_s[q] = mn; l_s[q] = ln; }
            }
        }
        __syncthreads();
    }
    for (int idx = x.tid; idx < Lq * dh; idx += kXNT) {
        const int q = idx / dh, d = idx - q * dh;
        const bool live = q < x.nq && l_s[q] > 0.0f;
        Ob[(size_t)q * a.F + d] = live ? Qs[(size_t)q * ld + d] * (1.0f / l_s[q]) : 0.0f;
    }
    for (int q = x.tid; q < Lq; q += kXNT) LSE[(size_t)x.bh * Lq + q] = (q < x.nq && l_s[q] > 0.0f) ? m_s[q] + __logf(l_s[q]) : 0.0f;
}

// D[bh][row] = sum_d dO[row][d] * O[row][d], 16 lanes per row (the dvec scratch of the backward)
__global__ void __launch_bounds__(256) xattn_rowdot_kernel(const float *__restrict__ O, const float *__restrict__ dO, XArgs a, float *__restrict__ Dv) {
    const int lane = threadIdx.x & 15, slot = threadIdx.x >> 4;
    const size_t nrows = (size_t)a.B * a.H * a.Lq;
    for (size_t r = (size_t)blockIdx.x * 16 + slot; r < nrows; r += (size_t)gridDim.x * 16) {
        const int bh = (int)(r / a.Lq), row = (int)(r - (size_t)bh * a.Lq), b = bh / a.H, h = bh - b * a.H;
        const size_t off = ((size_t)b * a.Lq + row) * a.F + (size_t)h * a.dh;
        float s = 0.0f;
        for (int d = lane; d < a.dh; d += 16) s += O[off + d] * dO[off + d];
        s += __shfl_xor(s, 8); s += __shfl_xor(s, 4); s += __shfl_xor(s, 2); s += __shfl_xor(s, 1);
        if (lane == 0) Dv[r] = s;
    }
}

// ============================================================================================ backward, both forms
// SQ = false (short keys):    LDS holds K, V; tiles are query rows (operands Q, dO); tile gradient dQ; reduced gradients dK, dV.
// SQ = true  (short queries): LDS holds Q, dO, lse, D; tiles are keys (operands K, V); tile gradients dK, dV; reduced gradient dQ.
template <int DT, int MT, bool SQ>
__global__ void __launch_bounds__(kXNT)
xattn_bwd_kernel(const float *__restrict__ Q, const float *__restrict__ K, const float *__restrict__ V, const float *__restrict__ dO,
                 const float *__restrict__ LSE, const float *__restrict__ Dv, const int32_t *__restrict__ lens_q,
                 const int32_t *__restrict__ lens_k, XArgs a, float *__restrict__ dQ, float *__restrict__ dK, float *__restrict__ dV) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ld = attn_ld(DT), NR = SQ ? 1 : 2;       // NR: short-side gradients reduced over the long side
    float *R1 = smem, *R2 = R1 + 16 * MT * ld;             // short keys: K, V;  short queries: Q, dO
    float *lse_s = R2 + 16 * MT * ld, *D_s = lse_s + 16 * MT;
    const XBlock x = xblock(a, lens_q, lens_k);
    float *pad = D_s + 16 * MT + x.wave * (16 * kDsPadLd);
    const int j = x.j, g = x.g, dh = a.dh, Lq = a.Lq, Lk = a.Lk;
    const float *Qb = Q + (size_t)x.b * a.qbs + (size_t)x.h * dh;
    const size_t kvbase = (size_t)x.b * Lk * a.ld_kv + (size_t)x.h * dh, obase = (size_t)x.b * Lq * a.F + (size_t)x.h * dh;
    const float *Kb = K + kvbase, *Vb = V + kvbase, *Gb = dO + obase;
    float *dQb = dQ + obase, *dKb = dK + kvbase, *dVb = dV + kvbase;
    const size_t sbase = (size_t)x.bh * Lq;
    if constexpr (SQ) {
        stage_short(R1, ld, 16 * MT, Qb, a.ld_q, dh, x.nq, x.tid);
        stage_short(R2, ld, 16 * MT, Gb, a.F, dh, x.nq, x.tid);
        for (int q = x.tid; q < 16 * MT; q += kXNT) { lse_s[q] = q < x.nq ? LSE[sbase + q] : 0.0f; D_s[q] = q < x.nq ? Dv[sbase + q] : 0.0f; }
    } else {
        stage_short(R1, ld, 16 * MT, Kb, a.ld_kv, dh, x.nk, x.tid);
        stage_short(R2, ld, 16 * MT, Vb, a.ld_kv, dh, x.nk, x.tid);
    }
    __syncthreads();
    // the tile's two operands: (Q, dO) rows or (K, V) rows
    const float *T1 = SQ ? Kb : Qb, *T2 = SQ ? Vb : Gb;
    const int st1 = SQ ? a.ld_kv : a.ld_q, st2 = SQ ? a.ld_kv : a.F;
    const int Lt = SQ ? Lk : Lq, nt = SQ ? x.nk : x.nq, ns = SQ ? x.nq : x.nk;      // long-side rows, live long-side rows, live short-side rows
    const bool vec1 = ATTN_FLOAT4_ROWS(dh, st1, T1), vec2 = ATTN_FLOAT4_ROWS(dh, st2, T2);
    const bool vecq = ATTN_FLOAT4_ROWS(dh, a.F, dQb), veckv = ATTN_FLOAT4_ROWS(dh, a.ld_kv, dKb) && ((reinterpret_cast<uintptr_t>(dVb) & 15) == 0);
    f32x4 racc[NR][MT][DT];
#pragma unroll
    for (int n = 0; n < NR; ++n)
#pragma unroll
        for (int kt = 0; kt < MT; ++kt)
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) racc[n][kt][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = x.wave; 16 * t < Lt; t += kXW) {
        const int row = 16 * t + j;                        // this lane's long-side row
        const bool rok = row < nt;
        f32x4 tg1[DT], tg2[DT];                            // the tile's gradient(s): dQ, or dK and dV
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) { tg1[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; tg2[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        if (16 * t < nt) {                                 // a tile of padded rows only writes zeros
            OperandRegs<DT> o1[1], o2[1];
            const size_t rr = (size_t)(row < Lt ? row : Lt - 1);
            o1[0].load_global(T1 + rr * st1, rok, dh, x.nb, x.rem, g, vec1);
            o2[0].load_global(T2 + rr * st2, rok, dh, x.nb, x.rem, g, vec2);
            float lse_r = 0.0f, D_r = 0.0f;
            if constexpr (!SQ) { lse_r = rok ? LSE[sbase + row] : 0.0f; D_r = rok ? Dv[sbase + row] : 0.0f; }
            f32x4 p[1][MT], ds[1][MT];                     // [short row 16 kt + 4 g + r][long row j]: S then P, dP then dS
            multi_dot<DT, MT, 1>(R1, 0, ld, x.nb, x.rem, j, g, o1, p);
            multi_dot<DT, MT, 1>(R2, 0, ld, x.nb, x.rem, j, g, o2, ds);
#pragma unroll
            for (int kt = 0; kt < MT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int sr = 16 * kt + 4 * g + r;
                    const float lse = SQ ? lse_s[sr] : lse_r, Dq = SQ ? D_s[sr] : D_r;
                    const float pr = (rok && sr < ns) ? __expf(p[0][kt][r] * a.inv_scale - lse) : 0.0f;
                    p[0][kt][r] = pr;
                    ds[0][kt][r] = pr * (ds[0][kt][r] - Dq) * a.inv_scale;
                }
            // the tile's gradient: X^T[d][long row j] += R^T[d][short row] * (dS or P)[short row][long row j]
#pragma unroll
            for (int kt = 0; kt < MT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float *r1 = R1 + (size_t)(16 * kt + 4 * g + r) * ld + j, *r2 = R2 + (size_t)(16 * kt + 4 * g + r) * ld + j;
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt) {
                        tg1[dt] = mfma4(r1[16 * dt], ds[0][kt][r], tg1[dt]);                   // dQ += K^T dS^T,  or dK += Q^T dS
                        if constexpr (SQ) tg2[dt] = mfma4(r2[16 * dt], p[0][kt][r], tg2[dt]);   // dV += dO^T P
                    }
                }
            // the short side's gradient: lane = short row 16 kt + j, registers = the tile's rows 16 t + 4 g + e
#pragma unroll
            for (int kt = 0; kt < MT; ++kt) {
                ds[0][kt] = tile_transpose(pad, j, g, ds[0][kt]);
                if constexpr (!SQ) p[0][kt] = tile_transpose(pad, j, g, p[0][kt]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int tr = 16 * t + 4 * g + e;
                const size_t trc = (size_t)(tr < Lt ? tr : Lt - 1);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    const int d = 16 * dt + j, dc = d < dh ? d : 0;
                    const bool ok = d < dh && tr < nt;
                    const float raw1 = T1[trc * st1 + dc];
                    const float a1 = ok ? raw1 : 0.0f;                                        // Q (short keys) or K (short queries)
#pragma unroll
                    for (int kt = 0; kt < MT; ++kt) racc[0][kt][dt] = mfma4(a1, ds[0][kt][e], racc[0][kt][dt]);     // dK += Q^T dS, or dQ += K^T dS^T
                    if constexpr (!SQ) {
                        const float raw2 = T2[trc * st2 + dc];
                        const float a2 = ok ? raw2 : 0.0f;                                    // dO
#pragma unroll
                        for (int kt = 0; kt < MT; ++kt) racc[1][kt][dt] = mfma4(a2, p[0][kt][e], racc[1][kt][dt]); // dV += dO^T P
                    }
                }
            }
        }
        if (row < Lt) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int d = 16 * dt + 4 * g;
                if constexpr (SQ) {
                    store4(dKb + (size_t)row * a.ld_kv + d, d, dh, veckv, tg1[dt]);
                    store4(dVb + (size_t)row * a.ld_kv + d, d, dh, veckv, tg2[dt]);
                } else {
                    store4(dQb + (size_t)row * a.F + d, d, dh, vecq, tg1[dt]);
                }
            }
        }
    }
    reduce_waves<DT, MT>(R1, ld, x.wave, j, g, racc[0]);
    if constexpr (!SQ) reduce_waves<DT, MT>(R2, ld, x.wave, j, g, racc[1]);
    const int Ls = SQ ? Lq : Lk;
    for (int idx = x.tid; idx < Ls * dh; idx += kXNT) {
        const int r = idx / dh, d = idx - r * dh;
        if constexpr (SQ) dQb[(size_t)r * a.F + d] = R1[(size_t)r * ld + d];
        else { dKb[(size_t)r * a.ld_kv + d] = R1[(size_t)r * ld + d]; dVb[(size_t)r * a.ld_kv + d] = R2[(size_t)r * ld + d]; }
    }
}

template <class Fn> static int dispatch_xattn(const XattnForm &f, Fn &&fn) {
    auto mt = [&]<int D>() -> int {
        switch (f.MT) {
            case 1: return fn.template operator()<D, 1>();
            case 2: return fn.template operator()<D, 2>();
            default: return fn.template operator()<D, 4>();
        }
    };
    switch (f.D) {
        case 1: return mt.template operator()<1>();
        case 2: return mt.template operator()<2>();
        case 3: return mt.template operator()<3>();
        case 4: return mt.template operator()<4>();
        case 5: return mt.template operator()<5>();
        case 6: return mt.template operator()<6>();
        case 7: return mt.template operator()<7>();
        default: return mt.template operator()<8>();
    }
}

static int xattn_args(const char *who, int B, int Lq, int Lk, int F, int H, int ld_q, int64_t qbs, int ld_kv, XArgs &a) {
    if (B < 0 || Lq <= 0 || Lk <= 0 || F <= 0 || H <= 0 || F % H != 0) {
        set_error("%s: bad shape B=%d Lq=%d Lk=%d F=%d heads=%d", who, B, Lq, Lk, F, H);
        return PTR_ERR_INVALID_ARG;
    }
    if (ld_q < F || ld_kv < F || qbs < 0) { set_error("%s: row strides %d, %d < F = %d, or a negative batch stride", who, ld_q, ld_kv, F); return PTR_ERR_INVALID_ARG; }
    const int dh = F / H;
    if (dh > kAttnNarrowMaxHeadDim) { set_error("%s: head dimension %d exceeds %d", who, dh, kAttnNarrowMaxHeadDim); return PTR_ERR_UNSUPPORTED; }
    if ((Lq < Lk ? Lq : Lk) > kXattnMaxShort) {
        set_error("%s: min(Lq, Lk) = %d exceeds %d: one side must be short", who, Lq < Lk ? Lq : Lk, kXattnMaxShort);
        return PTR_ERR_UNSUPPORTED;
    }
    if ((size_t)B * H * Lq >= (1u << 31) || (size_t)B * H * Lk >= (1u << 31)) { set_error("%s: B*H*L too large", who); return PTR_ERR_UNSUPPORTED; }
    a = XArgs{B, Lq, Lk, H, dh, F, ld_q, ld_kv, (long long)qbs, 1.0f / sqrtf((float)dh)};
    return 0;
}

}  // namespace ptr

extern "C" int ptr_xattn_forward(const float *Q, int ld_q, int64_t q_batch_stride, const float *K, const float *V, int ld_kv,
                                 const int32_t *lens_q, const int32_t *lens_k, int B, int Lq, int Lk, int F, int n_heads, float *O,
                                 float *lse, void *stream) {
    using namespace ptr;
    const char *who = "ptr_xattn_forward";
    XArgs a;
    if (int rc = xattn_args(who, B, Lq, Lk, F, n_heads, ld_q, q_batch_stride, ld_kv, a)) return rc;
    if (!Q || !K || !V || !O || !lse) { set_error("%s: NULL pointer", who); return PTR_ERR_INVALID_ARG; }
    if (B == 0) return 0;
    hipStream_t st = as_stream(stream);
    const XattnForm f = xattn_form(Lq, Lk, a.dh);
    return dispatch_xattn(f, [&]<int D, int MT>() -> int {
        auto go = [&](auto kern, size_t lds) -> int {
            if (int e = allow_lds(kern, lds)) return e;
            hipLaunchKernelGGL(kern, dim3((unsigned)(B * n_heads)), dim3(kXNT), lds, st, Q, K, V, lens_q, lens_k, a, O, lse);
            return check_hip(hipGetLastError(), who);
        };
        const size_t tile = (size_t)16 * MT * attn_ld(D) * sizeof(float);
        if (f.short_q) return go(xattn_fwd_sq_kernel<D, MT>, tile + (size_t)2 * 16 * MT * sizeof(float));
        return go(xattn_fwd_sk_kernel<D, MT>, 2 * tile);
    });
}

extern "C" int ptr_xattn_backward(const float *Q, int ld_q, int64_t q_batch_stride, const float *K, const float *V, int ld_kv,
                                  const int32_t *lens_q, const int32_t *lens_k, int B, int Lq, int Lk, int F, int n_heads, const float *O,
                                  const float *dO, const float *lse, float *dvec, float *dQ, float *dK, float *dV, void *stream) {
    using namespace ptr;
    const char *who = "ptr_xattn_backward";
    XArgs a;
    if (int rc = xattn_args(who, B, Lq, Lk, F, n_heads, ld_q, q_batch_stride, ld_kv, a)) return rc;
    if (!Q || !K || !V || !O || !dO || !lse || !dvec || !dQ || !dK || !dV) { set_error("%s: NULL pointer", who); return PTR_ERR_INVALID_ARG; }
    if (B == 0) return 0;
    hipStream_t st = as_stream(stream);
    const size_t nrows = (size_t)B * n_heads * Lq;
    const int rblocks = (int)((nrows + 15) / 16 < 4096 ? (nrows + 15) / 16 : 4096);
    hipLaunchKernelGGL(xattn_rowdot_kernel, dim3(rblocks), dim3(256), 0, st, O, dO, a, dvec);
    if (int rc = check_hip(hipGetLastError(), who)) return rc;
    const XattnForm f = xattn_form(Lq, Lk, a.dh);
    return dispatch_xattn(f, [&]<int D, int MT>() -> int {
        auto go = [&](auto kern) -> int {
            const size_t lds = ((size_t)2 * 16 * MT * attn_ld(D) + 2 * 16 * MT + (size_t)kXW * 16 * kDsPadLd) * sizeof(float);
            if (int e = allow_lds(kern, lds)) return e;
            hipLaunchKernelGGL(kern, dim3((unsigned)(B * n_heads)), dim3(kXNT), lds, st, Q, K, V, dO, lse, dvec, lens_q, lens_k, a, dQ, dK, dV);
            return check_hip(hipGetLastError(), who);
        };
        if (f.short_q) return go(xattn_bwd_kernel<D, MT, true>);
        return go(xattn_bwd_kernel<D, MT, false>);
    });
}
