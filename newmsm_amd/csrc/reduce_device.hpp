// reduce_device.hpp -- the fixed-shape sums of a 256-lane workgroup over LDS, shared by the statistics kernels (dedrift_kernels.hip, cohort_kernels.hip):
// a floating-point sum that goes through them has the same shape in every run and in every kernel, so it gives the same bits.
#pragma once

#include <hip/hip_runtime.h>

namespace msm {

constexpr int kSumBlock = 256;  // the workgroup's width: the tree's leaves

// the sum of one value per lane of a kSumBlock-wide workgroup, as a fixed binary tree over LDS (every lane gets it)
__device__ __forceinline__ double block_sum(double v, double *lds) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int s = kSumBlock / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] += lds[t + s];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

// N sums of one value per lane each, side by side over block_sum's tree; lane b < N returns sum b (the other lanes' value is not used)
template <class T, int N>
__device__ __forceinline__ T tile_sums(const T (&v)[N], T (*lds)[kSumBlock]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int b = 0; b < N; ++b) lds[b][t] = v[b];
    __syncthreads();
    for (int s = kSumBlock / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int b = 0; b < N; ++b) lds[b][t] += lds[b][t + s];
        }
        __syncthreads();
    }
    const T r = lds[t < N ? t : 0][0];
    __syncthreads();
    return r;
}

}  // namespace msm
