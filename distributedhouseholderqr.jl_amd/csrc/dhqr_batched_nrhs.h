// dhqr_batched_nrhs.h -- H_k \ B_k for a BATCH of tiny matrices with SEVERAL right-hand sides each, Float64 and Float32: one
// WAVE per matrix (dhqr_wave.h), the launch geometry and launch bounds of k_batched_ldiv_wave (dhqr_batched.h).
//
// Local fits and per-pixel regressions solve several channels against one small design matrix; looping the single-column
// kernel over the channels re-reads every matrix once per channel.  Here the factor and alpha are loaded ONCE into registers,
// and the right-hand sides walk past them: a runtime loop over groups of RG columns of B_k (bqn_rg), the body unrolled over
// the group.  Column r of matrix k lives at B + k strideB + r ldb and is read and written in place ([X_k; tail of Q'B_k]).
//
// Per column these are the expressions of k_batched_ldiv_wave in the same order, so column r of the result is BIT-IDENTICAL
// to what the single-column kernel returns for that column alone: it depends neither on nrhs nor on the column's position in
// its group nor on the batch.
//
// These two kernels are NOT built from the steps of dhqr_wave.h (bqw_load, bqw_reflect_group, bqw_backsub_group), of which
// they are the written-out form: built from them they compute the same bits but
// allocate other registers (profiles/wave_tier_refactor.txt: Float64 NC = 8 two scalar registers fewer; Float32 34 / 43 / 61
// vector registers instead of 40 / 45 / 62).  Whoever changes a step there changes it here.
#pragma once
#include "dhqr_f32.h"

// solve_householder!(B_k[:, r], H_k, alpha_k) (src:284-294) for r < nrhs, k < batch: B_k = B + k strideB (m x nrhs, ldb).
template <int NC, int RG = bqn_rg<double>(NC)>
__global__ __launch_bounds__(64 * BQW_WAVES, BQW_MIN_WAVES(NC)) void k_batched_ldiv_wave_nrhs(
    const double *__restrict__ A, int64_t lda, int64_t strideA, int m, int n, const double *__restrict__ alpha, int64_t stride_alpha,
    double *__restrict__ B, int nrhs, int64_t ldb, int64_t strideB, int64_t batch) {
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
  double al = l < n ? alpha[k * stride_alpha + l] : 1.0;  // lane j: alpha_j
  double rinv = dhqr_rcp(al);
#pragma unroll 1
  for (int r0 = 0; r0 < nrhs; r0 += RG) {
#pragma unroll
    for (int c = 0; c < NC; ++c) BQN_KEEP_IN_LOOP(a[c]);
    BQN_KEEP_IN_LOOP(al);
    BQN_KEEP_IN_LOOP(rinv);
    BQN_KEEP_IN_LOOP(l);  // (the lane masks l >= c, l == c, l < c: 6 NC scalar registers otherwise)
    dhqr_dd bb[RG];
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      const bool in = r0 + q < nrhs && l < m;  // (no branch; B_k[0] exists: m, nrhs >= 1)
      const double t = Bk[in ? (int64_t)l + (int64_t)(r0 + q) * ldb : 0];
      bb[q].hi = in ? t : 0.0;
      bb[q].lo = 0.0;
    }
    // ---- B <- Q'B: reflectors left to right (src:215-224), the group's chains side by side
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < n) {  // (wave-uniform)
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
          if ((c & 7) == 7) dd_renorm(bb[q]);  // the low part stays small against the high one
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RG; ++q) dd_renorm(bb[q]);
    // ---- back substitution, columns right to left (src:244-254): x_j = b_j / alpha_j, b[0:j] -= R[0:j, j] x_j
#pragma unroll
    for (int c = NC - 1; c >= 0; --c) {
      if (c < n) {
        const double aj = smq_readlane(al, c), ri = smq_readlane(rinv, c);
#pragma unroll
        for (int q = 0; q < RG; ++q) {
          // b_j / alpha_j as k_small_ldiv forms it: reciprocal (off the chain) times b_j and one correction step
          const double bq = smq_readlane(bb[q].hi + bb[q].lo, c);
          double xj = bq * ri;
          xj = fma(fma(-aj, xj, bq), ri, xj);
          if (l == c) {
            bb[q].hi = xj;
            bb[q].lo = 0.0;
          } else if (l < c) {
            dd_add_prod(bb[q], -a[c], xj);  // src:248-250
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RG; ++q)
      if (r0 + q < nrhs && l < m) Bk[(int64_t)l + (int64_t)(r0 + q) * ldb] = bb[q].hi + bb[q].lo;
  }
}

// the Float32 method: the matrix in float, b in plain double, rounded once at the end (k_batched_ldiv_wave<NC, float>)
template <int NC, int RG = bqn_rg<float>(NC)>
__global__ __launch_bounds__(64 * BQW_WAVES, BQS_MIN_WAVES(NC)) void k_batched_ldiv_wave_nrhs_s(
    const float *__restrict__ A, int64_t lda, int64_t strideA, int m, int n, const float *__restrict__ alpha, int64_t stride_alpha,
    float *__restrict__ B, int nrhs, int64_t ldb, int64_t strideB, int64_t batch) {
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
  double al = l < n ? (double)alpha[k * stride_alpha + l] : 1.0;  // lane j: alpha_j
  double rinv = dhqr_rcp(al);
#pragma unroll 1
  for (int r0 = 0; r0 < nrhs; r0 += RG) {
#pragma unroll
    for (int c = 0; c < NC; ++c) BQN_KEEP_IN_LOOP(a[c]);
    BQN_KEEP_IN_LOOP(al);
    BQN_KEEP_IN_LOOP(rinv);
    BQN_KEEP_IN_LOOP(l);  // (the lane masks l >= c, l == c, l < c: 6 NC scalar registers otherwise)
    double bb[RG];
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      const bool in = r0 + q < nrhs && l < m;  // (no branch; B_k[0] exists: m, nrhs >= 1)
      const float t = Bk[in ? (int64_t)l + (int64_t)(r0 + q) * ldb : 0];
      bb[q] = in ? (double)t : 0.0;
    }
    // ---- B <- Q'B: reflectors left to right (src:215-224), the group's chains side by side
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c < n) {  // (wave-uniform)
        const double v = l >= c ? (double)a[c] : 0.0;  // rows < c of a factored column hold R
        double s[RG];
#pragma unroll
        for (int q = 0; q < RG; ++q) s[q] = wave_sum_dpp(v * bb[q]);  // src:217
#pragma unroll
        for (int q = 0; q < RG; ++q) bb[q] = fma(-s[q], v, bb[q]);  // src:218-220
      }
    }
    // ---- back substitution, columns right to left (src:244-254): x_j = b_j / alpha_j, b[0:j] -= R[0:j, j] x_j
#pragma unroll
    for (int c = NC - 1; c >= 0; --c) {
      if (c < n) {
        const double aj = smq_readlane(al, c), ri = smq_readlane(rinv, c);
#pragma unroll
        for (int q = 0; q < RG; ++q) {
          // b_j / alpha_j as k_batched_ldiv_wave forms it: reciprocal (off the chain) times b_j and one correction step
          const double bq = smq_readlane(bb[q], c);
          double xj = bq * ri;
          xj = fma(fma(-aj, xj, bq), ri, xj);
          if (l == c)
            bb[q] = xj;
          else if (l < c)
            bb[q] = fma(-(double)a[c], xj, bb[q]);  // src:248-250
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RG; ++q)
      if (r0 + q < nrhs && l < m) Bk[(int64_t)l + (int64_t)(r0 + q) * ldb] = (float)bb[q];  // rounded once
  }
}
