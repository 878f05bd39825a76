// Block-level sum and exclusive scan of one 32-bit word per thread, for kernels whose blocks are whole 64-wide wavefronts: the
// line-index kernels (dev_prims.hip) and the ingest's counting kernels (ingest_gpu.hip).  Device code only.
#ifndef BLU_WAVE_SCAN_H
#define BLU_WAVE_SCAN_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace blu {

// ---- block-level sum and exclusive scan: 64-wide wavefronts reduce / scan in registers (DPP), the wave totals meet in LDS ----
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true); }
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {   // inclusive prefix sum over the 64 lanes
    v += dpp_u32<0x111>(v);                                        // row_shr:1, :2, :4, :8 (zero shifted in): prefix inside each 16-lane row
    v += dpp_u32<0x112>(v);
    v += dpp_u32<0x114>(v);
    v += dpp_u32<0x118>(v);
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 15), t1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 31),
                   t2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 47);
    const uint32_t r = lane >> 4;
    return v + (r == 0 ? 0u : (r == 1 ? t0 : (r == 2 ? t0 + t1 : t0 + t1 + t2)));
}
// sum over the block in every thread's return value; `wave_sums` = LDS, one word per wave
template <int THREADS>
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* wave_sums) {
    const uint32_t incl = wave_incl_scan(v);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) total += wave_sums[w];
    __syncthreads();
    return total;
}
// exclusive prefix of v over the block
template <int THREADS>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wave_sums) {
    const uint32_t incl = wave_incl_scan(v);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) before += (uint32_t)w < wave ? wave_sums[w] : 0u;
    __syncthreads();
    return before + incl - v;
}
}  // namespace blu
#endif
