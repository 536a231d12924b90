// iaf_common.hpp -- what more than one translation unit of the engine uses (iaf_engine.hip, iaf_model_ops.hip, iaf_train_services.hip):
// the grid of the elementwise launches, HIP_TRY and two device helpers of the reductions.  No __global__ function lives here: a kernel
// header is included by exactly one unit (the kernels are not static, a second inclusion is a duplicate symbol at link time).
#pragma once
#include <hip/hip_runtime.h>

#define HIP_TRY(expr)                               \
    do {                                            \
        hipError_t _e = (expr);                     \
        if (_e != hipSuccess) return (int)_e;       \
    } while (0)

static dim3 ew_grid(size_t n) {
    size_t g = (n + 255) / 256;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return dim3((unsigned)g);
}
// non-finite = exponent field all ones, tested on the bits so that no fast-math setting can fold it away
__device__ __forceinline__ bool iaf_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// the sum of v over a workgroup of 256 lanes in a fixed order: shuffles inside the waves, one LDS round (red[4]) across them
__device__ __forceinline__ double iaf_block_sum_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
