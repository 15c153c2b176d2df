// dhqr_f32.h -- Float32 qr!(A_k) and H_k \ b_k for tiny matrices (one WAVE per matrix), and the element-wise kernels that
// carry every other Float32 shape through the Float64 library.
//
// k_batched_qr_wave_s / k_batched_ldiv_wave_s are the Float32 methods of k_batched_qr_wave / k_batched_ldiv_wave
// (dhqr_batched.h; the reference's qr! and `\` are generic over the element type, src:306-321): same shapes (m <= 64,
// n <= NC = 8, 16 or 32), same structure -- lane l holds row l of every column, the reflector loop runs over a runtime j,
// column j leaves and re-enters the register array through compile-time selects, the trailing update walks unrolled groups
// of four columns, branch-free loads, no LDS, no barrier, no wait of any kind, the same stride arguments.
//
// Arithmetic: the matrix is STORED in float (float a[NC]: NC registers, half of the Float64 kernel's), every SUM is taken in
// double.  The product of two floats is exact in double, so the column norm sum x_i^2 and each v_j' a_c (partialdot,
// src:42-49) lose nothing before the DPP tree, whose six double additions sit 29 bits below the stored precision -- that
// is why no double-double is needed here, where the Float64 kernel needs one for the norm.  alpha, f and the pivot are
// formed in double by the expressions of the Float64 kernel (sign(0) = 0 and the overflow branch included); every stored
// entry is rounded to float ONCE per column step: v_j when it is formed (the trailing update then uses the stored, rounded
// v_j -- the reflector the solve will apply), a_c after fma(-v, d, a_c) in double.  The solve carries b in plain double
// through Q'b and the back substitution and rounds each entry once at the end.
#pragma once
#include "dhqr_batched.h"

// waves per SIMD the register allocation must leave room for (profiles/batched_kernel_resources.txt: measured counts)
#define BQS_MIN_WAVES(NC_) ((NC_) <= 16 ? 8 : 6)

// householder!(A_k, alpha_k) for k < batch: A_k = A + k strideA (m x n, m <= 64, n <= NC, m >= n >= 1), in place.
template <int NC>
__global__ __launch_bounds__(64 * BQW_WAVES, BQS_MIN_WAVES(NC)) void k_batched_qr_wave_s(float *__restrict__ A, int64_t lda, int64_t strideA,
                                                                                         int m, int n, float *__restrict__ alpha,
                                                                                         int64_t stride_alpha, int64_t batch) {
  static_assert(NC % 4 == 0 && NC <= BQW_MAX_N, "columns in groups of four");
  const int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + (threadIdx.x >> 6);
  if (k >= batch) return;  // (the whole wave)
  float *Ak = A + k * strideA;
  float a[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool in = c < n && l < m;  // (no branch: every load of the matrix is in flight before the first use)
    const float t = Ak[in ? (int64_t)l + (int64_t)c * lda : 0];
    a[c] = in ? t : 0.0f;
  }
  float alv = 0.0f;  // lane j keeps alpha_j
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    float xf = 0.0f;
#pragma unroll
    for (int c = 0; c < NC; ++c) xf = (c == j) ? a[c] : xf;
    const double x = (double)xf;
    // reflector j (src:129-140): rows >= m hold zeros; x_i^2 is exact in double
    const double xs = l >= j ? x : 0.0;
    const double s2 = wave_sum_dpp(xs * xs);
    const double h = smq_readlane(x, j);
    double sn, f;
    if (s2 > 0.0 && s2 < 1e300) {
      double rinv, sq;
      dhqr_sqrt_rsqrt(s2, sn, rinv);                 // src:129
      dhqr_sqrt_rsqrt(fma(sn, fabs(h), s2), sq, f);  // src:131: s (s + |h|) = s^2 + s |h|
    } else {
      sn = sqrt(s2);
      f = 1.0 / sqrt(sn * (sn + fabs(h)));
    }
    const double al = sn * dhqr_alphafactor(h);  // src:130
    const double piv = (h - al) * f;             // src:132
    const float vf = (float)(l > j ? x * f : (l == j ? piv : 0.0));  // src:133-140, rounded once
    const double v = (double)vf;
    if (l == j) alv = (float)al;
    const float xv = l >= j ? vf : xf;  // rows < j keep R
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = (c == j) ? xv : a[c];
    // trailing update (src:198-213): columns >= n hold zeros and stay zeros
#pragma unroll
    for (int g = 0; g < NC / 4; ++g) {
      if (4 * g + 3 > j && 4 * g < n) {
        double d[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) d[cc] = wave_sum_dpp(v * (double)a[4 * g + cc]);  // src:42-49: exact products
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)  // src:156-160, src:209: rows >= j of the columns behind j, nothing else (a reflector of a
          a[4 * g + cc] =               // zero column is NaN: 0 * NaN); rounded once
              (4 * g + cc > j && l >= j) ? (float)fma(-v, d[cc], (double)a[4 * g + cc]) : a[4 * g + cc];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < n && l < m) Ak[(int64_t)l + (int64_t)c * lda] = a[c];
  if (l < n) alpha[k * stride_alpha + l] = alv;
}

// solve_householder!(b_k, H_k, alpha_k) (src:284-294) for k < batch: b_k = b + k strideb (m) <- [x_k; tail of Q'b_k].
template <int NC>
__global__ __launch_bounds__(64 * BQW_WAVES, BQS_MIN_WAVES(NC)) void k_batched_ldiv_wave_s(const float *__restrict__ A, int64_t lda,
                                                                                           int64_t strideA, int m, int n,
                                                                                           const float *__restrict__ alpha,
                                                                                           int64_t stride_alpha, float *__restrict__ b,
                                                                                           int64_t strideb, int64_t batch) {
  const int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + (threadIdx.x >> 6);
  if (k >= batch) return;  // (the whole wave)
  const float *Ak = A + k * strideA;
  float *bk = b + k * strideb;
  float a[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool in = c < n && l < m;  // (no branch: every load of the matrix is in flight before the first use)
    const float t = Ak[in ? (int64_t)l + (int64_t)c * lda : 0];
    a[c] = in ? t : 0.0f;
  }
  const double al = l < n ? (double)alpha[k * stride_alpha + l] : 1.0;  // lane j: alpha_j
  double bb = l < m ? (double)bk[l] : 0.0;
  // ---- b <- Q'b: reflectors left to right (src:215-224)
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c < n) {  // (wave-uniform)
      const double v = l >= c ? (double)a[c] : 0.0;  // rows < c of a factored column hold R
      const double s = wave_sum_dpp(v * bb);         // src:217
      bb = fma(-s, v, bb);                           // src:218-220
    }
  }
  // ---- back substitution, columns right to left (src:244-254): x_j = b_j / alpha_j, b[0:j] -= R[0:j, j] x_j
  const double rinv = dhqr_rcp(al);
#pragma unroll
  for (int c = NC - 1; c >= 0; --c) {
    if (c < n) {
      // b_j / alpha_j as k_batched_ldiv_wave forms it: reciprocal (off the chain) times b_j and one correction step
      const double bq = smq_readlane(bb, c), aj = smq_readlane(al, c), ri = smq_readlane(rinv, c);
      double xj = bq * ri;
      xj = fma(fma(-aj, xj, bq), ri, xj);
      if (l == c)
        bb = xj;
      else if (l < c)
        bb = fma(-(double)a[c], xj, bb);  // src:248-250
    }
  }
  if (l < m) bk[l] = (float)bb;  // rounded once
}

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
