// __device__ helpers, vector types and small predicates shared by the HIP units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < (int)(blockDim.x >> 6); ++k) r += sh[k];
    __syncthreads();
    return r;   // valid on thread 0
}

__device__ __forceinline__ void unrank_pair(long r, int& x, int& y) {   // r = x(x+1)/2 + y, x >= y
    long xx = (long)((sqrt(8.0 * (double)r + 1.0) - 1.0) * 0.5);
    while (xx * (xx + 1) / 2 > r) --xx;
    while ((xx + 1) * (xx + 2) / 2 <= r) ++xx;
    x = (int)xx;
    y = (int)(r - xx * (xx + 1) / 2);
}

inline bool even(long x) { return (x & 1) == 0; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
