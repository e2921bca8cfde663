// What the two diversification kernel families share (diversity.hip: DALETOR's alpha-DCG loss and the diversity metrics; divprob.hip:
// DivProbRanker's objectives): the subtopic tile [Lp][TP] in LDS with TP = T rounded up to 4, 8, 16 or 32 (float4 rows), the dispatch on
// TP and the host-side subtopic checks.  The kernels' own prologue, tile staging and alpha-DCG gain loops stay written out in each kernel:
// moved into inline functions they compute the same bits but come out of the compiler scheduled differently, and alphadcg_kernel<64, 32>
// ran a quarter slower (4096 x 128 documents, 32 subtopics: 0.54 -> 0.69 ms).
#pragma once
#include "ptr_device.h"

namespace ptr {

constexpr size_t kLdsPerWorkgroup = 160 * 1024;       // gfx950: 160 KiB per CU, all of it available to one workgroup

// ---------------------------------------------------------------- host side
inline int tp_of(int T) { return T <= 4 ? 4 : T <= 8 ? 8 : T <= 16 ? 16 : 32; }

// The form of the loss kernels: G threads per query (one wavefront and four queries per workgroup up to 128 documents, when the four tiles
// fit the LDS; else the whole workgroup on one query) and the subtopic tile TP.
struct DivForm { int G; int TP; };
inline DivForm div_form(int T, int L, bool four_tiles_fit = true) { return {L <= 128 && four_tiles_fit ? kWave : kBlock, tp_of(T)}; }
DivForm divprob_form(int objective, int T, int L);                                        // divprob.hip: by its objective's LDS need

// Calls f.template operator()<TP>() for a subtopic tile.
template <class F> inline int dispatch_tp(int TP, F &&f) {
    if (TP == 4) return f.template operator()<4>();
    if (TP == 8) return f.template operator()<8>();
    if (TP == 16) return f.template operator()<16>();
    return f.template operator()<32>();
}

inline int check_subtopics_given(int T, const char *who) {
    if (T <= 0) { set_error("%s: bad number of subtopics T=%d", who, T); return PTR_ERR_INVALID_ARG; }
    return 0;
}
inline int check_subtopics_fit(int T, const char *who) {
    if (T > PTR_MAX_SUBTOPICS) { set_error("%s: %d subtopics exceed PTR_MAX_SUBTOPICS=%d", who, T, PTR_MAX_SUBTOPICS); return PTR_ERR_UNSUPPORTED; }
    return 0;
}
inline int check_top_k_axis(int top_k_axis, const char *who) {
    if (top_k_axis != 0 && top_k_axis != 1) { set_error("%s: top_k_axis must be 0 (subtopics) or 1 (documents), got %d", who, top_k_axis); return PTR_ERR_INVALID_ARG; }
    return 0;
}

inline int check_div(const void *preds, const void *rele, int B, int T, int L, float alpha, const char *who) {
    if (int rc = check_batch(preds, rele, B, L, who)) return rc;
    if (int rc = check_subtopics_given(T, who)) return rc;
    if (!(alpha > 0.0f && alpha < 1.0f)) { set_error("%s: alpha must be in (0, 1) (got %g)", who, (double)alpha); return PTR_ERR_INVALID_ARG; }
    return check_subtopics_fit(T, who);
}

// ---------------------------------------------------------------- device side
#if defined(__HIPCC__)

template <int TP> __device__ __forceinline__ void lds_row(const float *row, float (&v)[TP]) {
#pragma unroll
    for (int u = 0; u < TP; u += 4) {
        const float4 x = *reinterpret_cast<const float4 *>(row + u);
        v[u] = x.x; v[u + 1] = x.y; v[u + 2] = x.z; v[u + 3] = x.w;
    }
}
template <int TP> __device__ __forceinline__ void lds_put(float *row, const float (&v)[TP]) {
#pragma unroll
    for (int u = 0; u < TP; u += 4) *reinterpret_cast<float4 *>(row + u) = float4{v[u], v[u + 1], v[u + 2], v[u + 3]};
}

#endif  // __HIPCC__
}  // namespace ptr
