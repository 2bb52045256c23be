// pt_chain.hpp — the chain signature of rt_render_features_chain: the ONE place a followed vertex enters it.
// h = 0; for each followed vertex in path order h = (h ^ object) * 0x9E3779B1 (mod 2^32), `object` the id an rt_feature
// record holds (kind in bits 31..30, index below).  pt_features_chain (pt_kernels.hip) and the host's
// rt_feature_chain_signature call this very function.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pt {

__host__ __device__ inline uint32_t chain_signature_step(uint32_t h, uint32_t object) { return (h ^ object) * 0x9E3779B1u; }

}  // namespace pt
