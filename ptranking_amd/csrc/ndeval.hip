// TREC ndeval 4.4's diversity measures and its greedy ideal ranking, bit for bit in float64.
//
// Reference: ptranking/metric/srd/ndeval.c — idealResult :351-400, computeMAP :484-525, computeNRBP :531-562, discount :567-590,
//            computeERR :597-643, computeDCG :651-698, computeSTRecall :704-730, computePrecision :736-759, the binarisation :908, the -M
//            cut-off :1000-1020, renormalize :1143-1156.  The greedy is also ptranking/metric/srd/diversity_metric.py:113-141.
//
// Per query (c = 1 - alpha, every judgment binarised to `rele > 0`, one uint32 subtopic mask per document):
//   pool     the first lens[q] documents; nrelSub[j] = #documents relevant to subtopic j, S = #{j : nrelSub[j] > 0}
//   run      the pool ranked as ptr_sort_desc ranks it (preds == NULL: the input order), cut to depth_m documents when depth_m > 0
//   ideal    lens[q] greedy rounds: score(d) = sum over d's subtopics j ASCENDING of gain[j]; the largest score wins, ties to the larger
//            index; gain[j] *= c for the winner's subtopics
//   score_p  along a ranking = sum over the subtopics j of position p, ascending, of c^(number of earlier positions covering j)
//   alpha-DCG / ERR-IA [0..20)  cumulative score_p * discount_p (log 2 / log(p + 2), resp. score_p / (p + 1)), divided FROM INDEX 1 ON by
//            the cumulative "ideal ideal" array that starts from gain S; index 0 stays undivided (ndeval.c:641, :696)
//   NRBP     (sum_p score_p beta^p) (1 - c beta) / S, MAP-IA, P-IA@k, strec@k as ndeval.c writes them; S == 0: everything 0, nNRBP = 0/0
//
// Kernel form: one group of G threads per query on pick_tiling (G = 64: four queries per workgroup, L <= 128; G = 256: one query per
// workgroup up to PTR_MAX_LIST_LEN).  What is parallel: the masks, the rank counting (count_ranks, NaN first), the candidates' scores in
// the greedy (each lane rescans only its candidates that share a subtopic with the last pick), the group-wide arg-max, the per-position
// scores of a ranking (the prior cover counts come from ballots: an exact integer prefix scan; the gain is read from powtab[count]).
// What is serial, in ndeval's order, because a float64 sum is not associative: powtab (repeated multiplication), each position's sum
// over its subtopics (ascending, in its own lane), the 20-deep cumulative arrays, the NRBP sum, MAP-IA's per-subtopic sums (lane =
// subtopic).  No atomics, nothing of size L x L; a query's bits depend on its own data and L alone.  The library is built with
// -ffp-contract=off: no multiply-add is fused, so these are ndeval's IEEE operations.  log() is NOT evaluated on the device: the 20
// discounts arrive from the host.
// LDS per query: 32 * round_up(L, 4) + kNdFixedBytes bytes (kNdFixedBytes = 1664; 129.6 KiB at L = 4096 <= 160 KiB: every supported L fits).
#include <math.h>

#include "ptr_div.h"

namespace ptr {

constexpr int kNdDepth = PTR_NDEVAL_DEPTH;
constexpr int kNdFixedDoubles = 32 /* gain */ + 4 * kNdDepth /* arr */ + kNdDepth /* disc */ + 32 /* mapsub */ + 4 /* redv */ + 4 /* misc */;
constexpr int kNdFixedInts = 4 /* redi */ + 32 /* nrel */ + 32 /* ks */ + 4 /* pad */;
constexpr size_t kNdFixedBytes = (size_t)kNdFixedDoubles * 8 + (size_t)kNdFixedInts * 4;
__host__ __device__ constexpr size_t nd_group_bytes(int Lp) { return (size_t)Lp * 32 + kNdFixedBytes; }

struct NdevalArgs {
    int nk, depth_m;
    int k[PTR_MAX_CUTOFFS];
    double disc[kNdDepth];
    double alpha, beta;
};

// (score, index) order of the greedy: the larger score, then the larger index (ndeval.c:380-387 with zero-padded docnos)
__device__ __forceinline__ bool nd_better(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia > ib); }

// sc[p] = score of position p of the ranking whose masks are mseq[0..len): ONE wavefront, 64 positions at a time.  Lane j keeps the running
// cover count of subtopic j; position p's lane adds powtab[prior count] over its subtopics in ascending j.
__device__ __forceinline__ void nd_score_ranking(const uint32_t *mseq, int len, int nt, const double *powtab, double *sc, int t) {
    int cnt = 0;
    const unsigned long long lt = t == 0 ? 0ull : (~0ull >> (64 - t));
    for (int base = 0; base < len; base += kWave) {
        const int p = base + t;
        const uint32_t mm = p < len ? mseq[p] : 0u;
        double s = 0.0;
        for (int j = 0; j < nt; ++j) {
            const bool bit = (mm >> j) & 1u;
            const unsigned long long b = __ballot(bit);
            const int cj = __shfl(cnt, j, kWave);
            if (bit) s += powtab[cj + __popcll(b & lt)];
            if (t == j) cnt += __popcll(b);
        }
        if (p < len) sc[p] = s;
    }
}

// The two cumulative arrays of one ranking (lane 0: alpha-DCG, lane 1: ERR-IA) and its NRBP (lane 2); computeDCG / computeERR / computeNRBP.
__device__ __forceinline__ void nd_serial_sums(const double *sc, int len, int S, double c1, double beta, const double *disc, double *arr2,
                                               double *nrbp_out, int t) {
    if (t < 2) {
        const bool is_err = t == 1;
        double *out = arr2 + t * kNdDepth;
        double ig = (double)S, cum = 0.0, icum = 0.0;
        for (int i = 0; i < kNdDepth; ++i) {
            const double s = i < len ? sc[i] : 0.0;
            const double v = is_err ? s / (double)(i + 1) : s * disc[i];
            const double iv = is_err ? ig / (double)(i + 1) : ig * disc[i];
            ig *= c1;
            cum = i == 0 ? v : v + cum;
            icum = i == 0 ? iv : iv + icum;
            out[i] = i == 0 ? cum : cum / icum;
        }
    } else if (t == 2) {
        double x = 0.0, decay = 1.0;
        for (int p = 0; p < len; ++p) {
            x += sc[p] * decay;
            decay *= beta;
        }
        x *= (1.0 - c1 * beta) / (double)S;
        *nrbp_out = x;
    }
}

template <int G, int DPT>
__global__ void __launch_bounds__(kBlock)
ndeval_kernel(const float *__restrict__ preds, const float *__restrict__ rele, const int32_t *__restrict__ lens,
              const int32_t *__restrict__ ntopics, int B, int T, int L, int Lp, NdevalArgs a, double *__restrict__ per_k,
              double *__restrict__ per_q, int32_t *__restrict__ o_S, int32_t *__restrict__ ideal_order) {
    constexpr int QPB = kBlock / G;
    extern __shared__ __attribute__((aligned(16))) unsigned char nd_smem[];
    const int tid = threadIdx.x, grp = tid / G, t = tid % G;
    const int q = blockIdx.x * QPB + grp;
    const bool valid = q < B;
    const int n = __builtin_amdgcn_readfirstlane(valid ? query_len(lens, q, L) : 0);
    int nt = valid ? (ntopics ? ntopics[q] : T) : 0;
    nt = __builtin_amdgcn_readfirstlane(nt < 0 ? 0 : (nt > T ? T : nt));
    const size_t qb = valid ? (size_t)q : 0;

    double *powtab = reinterpret_cast<double *>(nd_smem + (size_t)grp * nd_group_bytes(Lp));
    double *sc = powtab + Lp, *gain = sc + Lp, *arr = gain + 32, *disc = arr + 4 * kNdDepth, *mapsub = disc + kNdDepth, *redv = mapsub + 32;
    double *misc = redv + 4;
    float *keys = reinterpret_cast<float *>(misc + 4);
    uint32_t *mask = reinterpret_cast<uint32_t *>(keys + Lp), *rmask = mask + Lp, *imask = rmask + Lp;
    int *redi = reinterpret_cast<int *>(imask + Lp), *nrel = redi + 4, *ksl = nrel + 32;
    int *untaken = reinterpret_cast<int *>(keys);              // keys[] is free once the run order stands

    const double c1 = 1.0 - a.alpha, beta = a.beta;

    // ---- stage: scores, one subtopic mask per document (ndeval.c:908: any positive judgment is 1), the small tables
    float own[DPT];
    uint32_t mk[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) {
        const int i = t + m * G;
        own[m] = (i < n && preds) ? preds[qb * L + i] : -INFINITY;
        uint32_t mm = 0;
        if (i < n)
            for (int tt = 0; tt < nt; ++tt) mm |= (rele[(qb * T + tt) * L + i] > 0.0f ? 1u : 0u) << tt;
        mk[m] = mm;
        if (i < Lp) { keys[i] = own[m]; mask[i] = mm; rmask[i] = preds ? 0u : mm; imask[i] = 0u; }
    }
    if (t < 32) { gain[t] = 1.0; nrel[t] = 0; }
    if (t == 0) {
#pragma unroll
        for (int c = 0; c < PTR_MAX_CUTOFFS; ++c) ksl[c] = a.k[c];
#pragma unroll
        for (int i = 0; i < kNdDepth; ++i) disc[i] = a.disc[i];
    }
    group_sync<G>();

    // ---- the run order: ptr_sort_desc's (value descending, NaN first, original index ascending); the masks go into rank order
    if (preds) {
        int rk[DPT];
        count_ranks<G, DPT, false, true>(keys, n, t, own, rk);
#pragma unroll
        for (int m = 0; m < DPT; ++m)
            if (t + m * G < n && rk[m] >= 0 && rk[m] < n) rmask[rk[m]] = mk[m];
    }

    // ---- nrelSub, S and the gain table (wave 0): powtab[c] = (1 - alpha)^c by repeated multiplication, up to the largest cover count
    int S = 0;
    if (t < kWave) {
        int cnt = 0;
        for (int base = 0; base < n; base += kWave) {
            const uint32_t mm = base + t < n ? mask[base + t] : 0u;
            for (int j = 0; j < nt; ++j) {
                const unsigned long long b = __ballot((mm >> j) & 1u);
                if (t == j) cnt += __popcll(b);
            }
        }
        if (t < 32) nrel[t] = cnt;
        S = __popcll(__ballot(cnt > 0));
        int maxc = cnt;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(maxc, off, kWave); maxc = o > maxc ? o : maxc; }
        if (t == 0) {
            double g = 1.0;
            powtab[0] = 1.0;
            for (int c = 1; c < maxc; ++c) { g *= c1; powtab[c] = g; }
        }
    }

    // ---- greedy ideal ranking (ndeval.c:351-400): rounds of a group-wide arg-max until the best remaining score is 0
    double cs[DPT];
#pragma unroll
    for (int m = 0; m < DPT; ++m) cs[m] = t + m * G < n ? (double)__popc(mk[m]) : -1.0;       // every gain starts at 1; -1: taken or padding
    int pos = 0;
    for (; pos < n; ++pos) {
        double bs = -1.0;
        int bi = -1;
#pragma unroll
        for (int m = 0; m < DPT; ++m)
            if (cs[m] >= 0.0 && cs[m] >= bs) { bs = cs[m]; bi = t + m * G; }                  // the later (larger) index takes a tie
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double os = __shfl_xor(bs, off, kWave);
            const int oi = __shfl_xor(bi, off, kWave);
            if (nd_better(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if constexpr (G != kWave) {
            if ((t & 63) == 0) { redv[t >> 6] = bs; redi[t >> 6] = bi; }
            __syncthreads();
            bs = redv[0]; bi = redi[0];
#pragma unroll
            for (int w = 1; w < G / kWave; ++w) {
                const double os = redv[w];
                const int oi = redi[w];
                if (nd_better(os, oi, bs, bi)) { bs = os; bi = oi; }
            }
        }
        if (!(bs > 0.0)) break;                   // what is left scores 0 and stays there: ndeval takes it by descending index (below)
        const int w = bi;
        const uint32_t wm = mask[w];
        if (t == 0) {
            imask[pos] = wm;
            if (valid && ideal_order) ideal_order[qb * L + pos] = w;
        }
        if (t < 32 && ((wm >> t) & 1u)) gain[t] *= c1;                                        // ndeval.c:396-398
        group_sync<G>();
        // rescore the candidates that share a subtopic with the pick: each sum runs over its subtopics in ascending order (ndeval.c:375-377);
        // the sums of a lane's DPT candidates advance together, one term each per trip, so their LDS reads are in flight at once
        uint32_t mm[DPT];
        uint32_t left = 0u;
#pragma unroll
        for (int m = 0; m < DPT; ++m) {
            if (t + m * G == w) { cs[m] = -1.0; mk[m] = 0u; }
            mm[m] = (mk[m] & wm) ? mk[m] : 0u;
            if (mm[m]) cs[m] = 0.0;
            left |= mm[m];
        }
        while (left) {
            left = 0u;
#pragma unroll
            for (int m = 0; m < DPT; ++m) {
                const uint32_t x = mm[m];
                const double g = gain[x ? __builtin_ctz(x) : 0];
                cs[m] += x ? g : 0.0;                                                         // + 0.0 leaves a finished (or taken) sum as it is
                mm[m] = x & (x - 1u);
                left |= mm[m];
            }
        }
    }
    group_sync<G>();
#pragma unroll
    for (int m = 0; m < DPT; ++m)
        if (t + m * G < n) untaken[t + m * G] = cs[m] >= 0.0 ? 1 : 0;
    if (valid && ideal_order)
        for (int i = n + t; i < L; i += G) ideal_order[qb * L + i] = -1;
    group_sync<G>();

    if (t >= kWave) return;                       // the rest is one wavefront's work (no workgroup barrier below)

    // ---- the tail of the ideal ranking: the documents that score 0, by descending index
    {
        int p0 = pos;
        for (int base = n > 0 ? ((n - 1) / kWave) * kWave : 0; base >= 0; base -= kWave) {
            const int i = base + t;
            const bool u = i < n && untaken[i] != 0;
            const unsigned long long b = __ballot(u);
            const int higher = __popcll((b >> t) >> 1);
            if (u) {
                imask[p0 + higher] = mask[i];
                if (valid && ideal_order) ideal_order[qb * L + p0 + higher] = i;
            }
            p0 += __popcll(b);
        }
    }
    if (valid && t == 0 && o_S) o_S[q] = S;
    if (!valid || (!per_k && !per_q)) return;
    const int nk = a.nk;
    if (S == 0) {                                 // ndeval: every compute* returns early, renormalize() divides 0 by 0
        if (per_k)
            for (int idx = t; idx < 6 * nk; idx += kWave) per_k[qb * 6 * nk + idx] = 0.0;
        if (per_q && t == 0) { per_q[qb * 3 + 0] = 0.0; per_q[qb * 3 + 1] = __builtin_nan(""); per_q[qb * 3 + 2] = 0.0; }
        return;
    }
    wave_lds_sync();

    // ---- the run, then the ideal ranking, through the same code
    const int rlen = a.depth_m > 0 && a.depth_m < n ? a.depth_m : n;
    nd_score_ranking(rmask, rlen, nt, powtab, sc, t);
    wave_lds_sync();
    nd_serial_sums(sc, rlen, S, c1, beta, disc, arr, misc + 0, t);
    wave_lds_sync();
    nd_score_ranking(imask, n, nt, powtab, sc, t);
    wave_lds_sync();
    nd_serial_sums(sc, n, S, c1, beta, disc, arr + 2 * kNdDepth, misc + 1, t);

    // ---- MAP-IA (ndeval.c:484-525): lane = subtopic, the run top down
    if (t < nt) {
        int cnt = 0;
        double tot = 0.0;
        for (int p = 0; p < rlen; ++p)
            if ((rmask[p] >> t) & 1u) { ++cnt; tot += (double)cnt / (double)(p + 1); }
        mapsub[t] = nrel[t] > 0 ? tot / (double)nrel[t] : 0.0;
    }
    wave_lds_sync();
    if (per_q && t == 0) {
        double mapia = 0.0;
        for (int j = 0; j < nt; ++j)
            if (nrel[j] > 0) mapia += mapsub[j];
        mapia /= (double)S;
        per_q[qb * 3 + 0] = misc[0];
        per_q[qb * 3 + 1] = misc[0] / misc[1];
        per_q[qb * 3 + 2] = mapia;
    }
    if (per_k && t < nk) {
        const int k = ksl[t & (PTR_MAX_CUTOFFS - 1)], kk = k < rlen ? k : rlen;
        int count = 0;
        uint32_t seen = 0u;
        for (int p = 0; p < kk; ++p) { count += __popc(rmask[p]); seen |= rmask[p]; }
        const double rdcg = arr[k - 1], rerr = arr[kNdDepth + k - 1], idcg = arr[2 * kNdDepth + k - 1], ierr = arr[3 * kNdDepth + k - 1];
        double *o = per_k + qb * 6 * nk + t;
        o[0 * nk] = rerr;
        o[1 * nk] = rdcg != 0.0 ? rerr / ierr : 0.0;                                          // ndeval.c:1149-1153
        o[2 * nk] = rdcg;
        o[3 * nk] = rdcg != 0.0 ? rdcg / idcg : 0.0;
        o[4 * nk] = (double)count / (double)(k * S);                                          // ndeval.c:754, :758
        o[5 * nk] = (double)__popc(seen) / (double)S;                                         // ndeval.c:725, :729
    }
}

}  // namespace ptr

extern "C" int ptr_ndeval_measures(const float *preds, const float *rele, const int32_t *lens, const int32_t *ntopics, int B, int T, int L,
                                   const int32_t *ks, int nk, double alpha, double beta, int depth_m, double *per_k, double *per_q,
                                   int32_t *actual_subtopics, int32_t *ideal_order, void *stream) {
    using namespace ptr;
    const char *who = "ptr_ndeval_measures";
    if (int rc = check_batch(rele, rele, B, L, who)) return rc;
    if (int rc = check_subtopics_given(T, who)) return rc;
    if (!(alpha > 0.0 && alpha < 1.0)) { set_error("%s: alpha must be in (0, 1) (got %g)", who, alpha); return PTR_ERR_INVALID_ARG; }
    if (!(beta >= 0.0 && beta <= 1.0)) { set_error("%s: beta must be in [0, 1] (got %g)", who, beta); return PTR_ERR_INVALID_ARG; }
    if (depth_m < 0) { set_error("%s: depth_m must be >= 0 (got %d)", who, depth_m); return PTR_ERR_INVALID_ARG; }
    if (nk < 0 || (nk > 0 && !ks)) { set_error("%s: bad cut-off list", who); return PTR_ERR_INVALID_ARG; }
    if (int rc = check_subtopics_fit(T, who)) return rc;
    if (nk > PTR_MAX_CUTOFFS) { set_error("%s: %d cut-offs exceed PTR_MAX_CUTOFFS=%d", who, nk, PTR_MAX_CUTOFFS); return PTR_ERR_UNSUPPORTED; }
    NdevalArgs a;
    a.nk = nk; a.depth_m = depth_m; a.alpha = alpha; a.beta = beta;
    for (int c = 0; c < PTR_MAX_CUTOFFS; ++c) {
        a.k[c] = c < nk ? ks[c] : 1;
        if (a.k[c] < 1 || a.k[c] > PTR_NDEVAL_DEPTH) {
            set_error("%s: cut-off %d outside 1..PTR_NDEVAL_DEPTH=%d", who, a.k[c], PTR_NDEVAL_DEPTH);
            return PTR_ERR_INVALID_ARG;
        }
    }
    if (nk > 0 && !per_k) nk = a.nk = 0;
    for (int i = 0; i < kNdDepth; ++i) a.disc[i] = i == 0 ? 1.0 : log(2.0) / log(i + 2.0);    // discount(), ndeval.c:567-590
    const Tiling tl = pick_tiling(L);
    const int Lp = round_up(L, 4), QPB = kBlock / tl.G;
    const size_t lds = (size_t)QPB * nd_group_bytes(Lp);
    if (lds > kLdsPerWorkgroup) {
        set_error("%s: L=%d needs %zu bytes of LDS per workgroup (limit %zu): 32 * round_up(L, 4) + %zu bytes per query", who, L, lds,
                  kLdsPerWorkgroup, kNdFixedBytes);
        return PTR_ERR_UNSUPPORTED;
    }
    if (B == 0) return 0;
    return dispatch_tiling(L, [&]<int G, int DPT>() -> int {
        return launch_queries(ndeval_kernel<G, DPT>, B, kBlock / G, kBlock, lds, stream, who, preds, rele, lens, ntopics, B, T, L, Lp, a, per_k,
                              per_q, actual_subtopics, ideal_order);
    });
}
