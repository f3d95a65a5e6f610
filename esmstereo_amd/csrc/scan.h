// The wave and workgroup scans of the two codecs (png.hip, jpeg.hip): 64-lane waves, 32-bit values.
#pragma once

#include "common.h"

namespace esm {

// sum of v over the wave, in every lane
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// inclusive prefix of v over the wave's lanes
__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t n = __shfl_up(v, d);
        if (lane >= d) v += n;
    }
    return v;
}

// exclusive prefix of v over the workgroup's THREADS lanes and the total; wsum: THREADS / 64 words of LDS, free again
// on return
template <int THREADS>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive(v);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < THREADS / 64; ++k) {
        const uint32_t s = wsum[k];
        base += k < wave ? s : 0;
        total += s;
    }
    __syncthreads();
    return base + inc - v;
}

}  // namespace esm
