// The counter-based uniform stream of the device samplers (plsample.hip, irgan.hip) and the reference's Gumbel transform: the header of
// plsample.hip describes the construction, tests/plsample_ref.py restates it on the host.
#pragma once
#include "ptr_dropout.h"

namespace ptr {

struct PlKeys { uint32_t a, b; };

__device__ __forceinline__ PlKeys pl_query_keys(uint64_t seed, int64_t qg) {
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
    const uint32_t qlo = (uint32_t)(uint64_t)qg, qhi = (uint32_t)((uint64_t)qg >> 32);
    PlKeys k;
    k.a = lowbias32(lo ^ lowbias32(hi + qlo * 0x9E3779B1u + qhi * 0xC2B2AE3Du));
    k.b = lowbias32(hi ^ lowbias32(lo + qlo * 0x85EBCA77u + qhi * 0x27D4EB2Fu + 0x68E31DA4u));
    return k;
}
__device__ __forceinline__ PlKeys pl_sample_keys(PlKeys q, uint32_t s) {
    return PlKeys{lowbias32(q.a + s * 0xC2B2AE3Du), lowbias32(q.b + s * 0x9E3779B1u)};
}
__device__ __forceinline__ float pl_uniform(PlKeys k, uint32_t i) {
    const uint32_t h = lowbias32(k.a + i * 0x85EBCA77u);
    return (float)(((h ^ k.b) * 0x2C1B3C6Du) >> 8) * 0x1p-24f;
}
// sampling_utils.py:68 as written (libm logarithms: supplied uniforms reproduce the reference's noise)
__device__ __forceinline__ float pl_gumbel(float u) { return -logf(-logf(u + 1e-20f) + 1e-20f); }

}  // namespace ptr
