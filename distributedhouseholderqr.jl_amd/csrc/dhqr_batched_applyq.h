// dhqr_batched_applyq.h -- B_k <- Q_k' B_k, B_k <- Q_k B_k, the explicit thin Q_k and R_k for a BATCH of tiny factored
// matrices: one WAVE per matrix.
//
// k_batched_applyq_wave / k_batched_applyq_wave_s are k_batched_ldiv_wave_nrhs / _s (dhqr_batched_nrhs.h) without the back
// substitution, under the same launch geometry and launch bounds, and like them the written-out form of the steps of
// dhqr_wave.h: built from bqw_reflect_group the Float64 kernel moved the SIGN of the NaNs a NaN reflector leaves in its matrix
// (profiles/wave_tier_refactor.txt), and a byte is a byte.  Whoever changes a step there changes it here.  The factor is loaded
// ONCE into registers -- no alpha: Q is made of the reflectors alone --, and the columns of B_k walk past it in groups of RG
// (bqa_rg).
//
//   TRANS = 1   B <- Q'B: reflectors left to right (src:215-224).  Per column the reflector step of the solve in the same
//               order, so rows n .. m-1 of the result have the BITS of the same rows of what the solve leaves in B (the tail
//               of Q'B, which back substitution never touches).
//   TRANS = 0   B <- QB: the same step, reflectors right to left, c = n-1 .. 0.
//   FORMQ       TRANS = 0 on columns e_r generated in registers: B is the m x n Q_k, of which nothing is read and all m rows
//               of the n columns are written.  Column r is H_0 ... H_r e_r: the reflectors c > r act as the identity on e_r
//               (v_c is zero above row c, e_r below row r: the dot product is an exact zero), so a group skips the
//               reflectors behind its last column under one wave-uniform branch.  For a finite factor the result compares
//               equal to TRANS = 0 applied to [I; 0].
//
// Float64 renormalises a column after every eighth reflector and once at the end.  TRANS = 1: after c = 7, 15, 23, as the
// solve does.  TRANS = 0: after c = 24, 16, 8 -- by the reflector's INDEX, not by how many this column has seen, so at most
// eight reflectors lie between two renormalisations wherever the walk starts (n - 1, or the group's last column under FORMQ)
// and FORMQ renormalises exactly where TRANS = 0 on [I; 0] does.  Column r of the result depends neither on nrhs nor on its
// place in its group nor on the batch.
//
// k_batched_form_r: R_k (n x n) = the strict upper part of H_k, alpha_k on the diagonal, zeros written below (src:296-309);
// k_batched_eye: [I; 0], the input of the explicit Q beyond the wave tier.  Plain element-wise kernels for every shape and
// every element type (ComplexF64: T = double2).
#pragma once
#include <type_traits>
#include "dhqr_batched_nrhs.h"

template <int NC, int TRANS, int FORMQ = 0, int RG = bqa_rg<double>(NC)>
__global__ __launch_bounds__(64 * BQW_WAVES, BQW_MIN_WAVES(NC)) void k_batched_applyq_wave(
    const double *__restrict__ A, int64_t lda, int64_t strideA, int m, int n, double *__restrict__ B, int nrhs, int64_t ldb,
    int64_t strideB, int64_t batch) {
  static_assert(!FORMQ || !TRANS, "the explicit Q is Q [I; 0]");
  int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + (threadIdx.x >> 6);
  if (k >= batch) return;  // (the whole wave)
  const double *Ak = A + k * strideA;
  double *Bk = B + k * strideB;
  double a[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool in = c < n && l < m;  // (no branch: every load of the matrix is in flight before the first use)
    const double t = Ak[in ? (int64_t)l + (int64_t)c * lda : 0];
    a[c] = in ? t : 0.0;
  }
#pragma unroll 1
  for (int r0 = 0; r0 < nrhs; r0 += RG) {
#pragma unroll
    for (int c = 0; c < NC; ++c) BQN_KEEP_IN_LOOP(a[c]);
    BQN_KEEP_IN_LOOP(l);  // (the lane masks l >= c: 2 NC scalar registers otherwise)
    dhqr_dd bb[RG];
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      if (FORMQ) {
        bb[q].hi = l == r0 + q ? 1.0 : 0.0;  // e_r (r >= nrhs = n: never stored)
      } else {
        const bool in = r0 + q < nrhs && l < m;  // (no branch; B_k[0] exists: m, nrhs >= 1)
        const double t = Bk[in ? (int64_t)l + (int64_t)(r0 + q) * ldb : 0];
        bb[q].hi = in ? t : 0.0;
      }
      bb[q].lo = 0.0;
    }
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
      const int c = TRANS ? cc : NC - 1 - cc;
      if (c < n && (!FORMQ || c < r0 + RG)) {  // (wave-uniform)
        const double v = l >= c ? a[c] : 0.0;  // rows < c of a factored column hold R
        dhqr_dd p[RG], sd[RG];
#pragma unroll
        for (int q = 0; q < RG; ++q) {
          p[q].hi = 0.0;
          p[q].lo = 0.0;
          dd_add_prod(p[q], v, bb[q].hi);  // src:217: v_i b_i, b_i = hi + lo
          p[q].lo = fma(v, bb[q].lo, p[q].lo);
        }
#pragma unroll
        for (int q = 0; q < RG; ++q) sd[q] = wave_sum_dd_plain(p[q]);
#pragma unroll
        for (int q = 0; q < RG; ++q) {
          const double s = sd[q].hi + sd[q].lo;
          dd_add_prod(bb[q], -s, v);  // src:218-220: b_i -= v_i s
          if (TRANS ? (c & 7) == 7 : (c & 7) == 0) dd_renorm(bb[q]);  // the low part stays small against the high one
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RG; ++q) dd_renorm(bb[q]);
#pragma unroll
    for (int q = 0; q < RG; ++q)
      if (r0 + q < nrhs && l < m) Bk[(int64_t)l + (int64_t)(r0 + q) * ldb] = bb[q].hi + bb[q].lo;
  }
}

// the Float32 method: the matrix in float, a column in plain double, rounded once at the end
template <int NC, int TRANS, int FORMQ = 0, int RG = bqa_rg<float>(NC)>
__global__ __launch_bounds__(64 * BQW_WAVES, BQS_MIN_WAVES(NC)) void k_batched_applyq_wave_s(
    const float *__restrict__ A, int64_t lda, int64_t strideA, int m, int n, float *__restrict__ B, int nrhs, int64_t ldb,
    int64_t strideB, int64_t batch) {
  static_assert(!FORMQ || !TRANS, "the explicit Q is Q [I; 0]");
  int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + (threadIdx.x >> 6);
  if (k >= batch) return;  // (the whole wave)
  const float *Ak = A + k * strideA;
  float *Bk = B + k * strideB;
  float a[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool in = c < n && l < m;  // (no branch: every load of the matrix is in flight before the first use)
    const float t = Ak[in ? (int64_t)l + (int64_t)c * lda : 0];
    a[c] = in ? t : 0.0f;
  }
#pragma unroll 1
  for (int r0 = 0; r0 < nrhs; r0 += RG) {
#pragma unroll
    for (int c = 0; c < NC; ++c) BQN_KEEP_IN_LOOP(a[c]);
    BQN_KEEP_IN_LOOP(l);  // (the lane masks l >= c: 2 NC scalar registers otherwise)
    double bb[RG];
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      if (FORMQ) {
        bb[q] = l == r0 + q ? 1.0 : 0.0;  // e_r (r >= nrhs = n: never stored)
      } else {
        const bool in = r0 + q < nrhs && l < m;  // (no branch; B_k[0] exists: m, nrhs >= 1)
        const float t = Bk[in ? (int64_t)l + (int64_t)(r0 + q) * ldb : 0];
        bb[q] = in ? (double)t : 0.0;
      }
    }
#pragma unroll
    for (int cc = 0; cc < NC; ++cc) {
      const int c = TRANS ? cc : NC - 1 - cc;
      if (c < n && (!FORMQ || c < r0 + RG)) {  // (wave-uniform)
        const double v = l >= c ? (double)a[c] : 0.0;  // rows < c of a factored column hold R
        double s[RG];
#pragma unroll
        for (int q = 0; q < RG; ++q) s[q] = wave_sum_dpp(v * bb[q]);  // src:217
#pragma unroll
        for (int q = 0; q < RG; ++q) bb[q] = fma(-s[q], v, bb[q]);  // src:218-220
      }
    }
#pragma unroll
    for (int q = 0; q < RG; ++q)
      if (r0 + q < nrhs && l < m) Bk[(int64_t)l + (int64_t)(r0 + q) * ldb] = (float)bb[q];  // rounded once
  }
}

// the zero and the one of an element type (T = double, float; double2: a ComplexF64 element, re and im)
template <typename T>
__device__ __forceinline__ T bq_elem(double re) {
  if constexpr (std::is_same_v<T, double2>) return make_double2(re, 0.0);
  else return (T)re;
}

// R_k[i, j] = H_k[i, j] (i < j) | alpha_k[j] (i == j) | 0 (i > j) for i, j < n, k < batch: R_k at R + k strideR (leading
// dimension ldr).  Consecutive threads take consecutive rows of a column; grid-stride.  T = double, float, double2.
template <typename T>
__global__ __launch_bounds__(256) void k_batched_form_r(const T *__restrict__ A, int64_t lda, int64_t strideA, int64_t n,
                                                        const T *__restrict__ alpha, int64_t stride_alpha, T *__restrict__ R,
                                                        int64_t ldr, int64_t strideR, int64_t batch) {
  const int64_t per = n * n, total = per * batch;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = idx / per, r = idx - k * per, j = r / n, i = r - j * n;
    T x = bq_elem<T>(0.0);
    if (i < j) x = A[k * strideA + j * lda + i];
    else if (i == j) x = alpha[k * stride_alpha + j];
    R[k * strideR + j * ldr + i] = x;
  }
}

// Q_k <- [I; 0] (rows x cols) for k < batch: what the blocked route turns into the explicit Q
template <typename T>
__global__ __launch_bounds__(256) void k_batched_eye(T *__restrict__ Q, int64_t ldq, int64_t strideQ, int64_t rows, int64_t cols,
                                                     int64_t batch) {
  const int64_t per = rows * cols, total = per * batch;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k = idx / per, r = idx - k * per, j = r / rows, i = r - j * rows;
    Q[k * strideQ + j * ldq + i] = bq_elem<T>(i == j ? 1.0 : 0.0);
  }
}
