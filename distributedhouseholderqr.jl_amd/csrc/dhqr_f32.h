// dhqr_f32.h -- the element-wise kernels that carry every Float32 shape beyond the wave tier through the Float64 library.
// (The native Float32 kernels are the T = float instantiations of the wave-per-matrix kernels: dhqr_wave.h, dhqr_batched.h.)
#pragma once
#include "dhqr_batched.h"

// ---- the promoted tier: Float32 arrays through the Float64 library ------------------------------------------------------
// dst_k[i + j ldd] = (double)src_k[i + j lds] for i < rows, j < cols, k < batch (block k at src + k sstride / dst + k dstride):
// exact.  Consecutive threads take consecutive rows of a column (coalesced for column-major blocks); grid-stride.
__global__ __launch_bounds__(256) void k_widen_f32(const float *__restrict__ src, int64_t lds, int64_t sstride, double *__restrict__ dst,
                                                   int64_t ldd, int64_t dstride, int64_t rows, int64_t cols, int64_t batch) {
  const int64_t per = rows * cols, total = per * batch;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = idx / per, r = idx - k * per, j = r / rows, i = r - j * rows;
    dst[k * dstride + j * ldd + i] = (double)src[k * sstride + j * lds + i];
  }
}
// the way back: round to nearest-even; a value outside Float32's range becomes +-inf, NaN stays NaN
__global__ __launch_bounds__(256) void k_round_f32(const double *__restrict__ src, int64_t lds, int64_t sstride, float *__restrict__ dst,
                                                   int64_t ldd, int64_t dstride, int64_t rows, int64_t cols, int64_t batch) {
  const int64_t per = rows * cols, total = per * batch;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = idx / per, r = idx - k * per, j = r / rows, i = r - j * rows;
    dst[k * dstride + j * ldd + i] = (float)src[k * sstride + j * lds + i];
  }
}
