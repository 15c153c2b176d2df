// dhqr_batched.h -- qr!(A_k) and H_k \ b_k for a BATCH of tiny matrices, Float64 and Float32 (T = double, float; the
// reference's qr! and `\` are generic over the element type, src:306-321): one WAVE per matrix.  Geometry, arithmetic and
// every step: dhqr_wave.h.
//
// The fully unrolled factorisation of 32 columns is 500 column updates of straight-line code, so the reflector loop runs over
// a RUNTIME j: column j is taken out of (and put back into) the register array by a chain of selects, and the trailing update
// walks the columns in unrolled groups of four.
#pragma once
#include "dhqr_wave.h"

// householder!(A_k, alpha_k) for k < batch: A_k = A + k strideA (m x n, m <= 64, n <= NC, m >= n >= 1), in place.
template <int NC, typename T>
__global__ __launch_bounds__(64 * BQW_WAVES, bqw_min_waves<T>(NC)) void k_batched_qr_wave(T *__restrict__ A, int64_t lda, int64_t strideA, int m,
                                                                                         int n, T *__restrict__ alpha, int64_t stride_alpha,
                                                                                         int64_t batch) {
  const int l = bqw_lane();
  const int64_t k = bqw_matrix();
  if (k >= batch) return;  // (the whole wave)
  T *Ak = A + k * strideA;
  T a[NC];
  bqw_load(a, Ak, lda, m, n, l);
  T alv = (T)0;  // lane j keeps alpha_j
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    const T xt = bqw_take(a, j);
    const double x = (double)xt;
    // reflector j (src:129-140): rows >= m hold zeros
    const double s2 = bqw_norm2<T>(l >= j ? x : 0.0);
    const double h = smq_readlane(x, j);
    double sn, f, al;
    dhqr_reflector_scalars(s2, h, dhqr_alphafactor, sn, f, al);
    const double piv = (h - al) * f;  // src:132
    const T vt = (T)(l > j ? x * f : (l == j ? piv : 0.0));  // src:133-140 (Float32: rounded once; the trailing update uses the
    const double v = (double)vt;                              // stored, rounded v_j -- the reflector the solve will apply)
    if (l == j) alv = (T)al;
    bqw_put(a, j, l >= j ? vt : xt);  // rows < j keep R
    bqw_trailing_update(a, v, j, n, l);
  }
  bqw_store(a, Ak, lda, m, n, l);
  if (l < n) alpha[k * stride_alpha + l] = alv;
}

// solve_householder!(b_k, H_k, alpha_k) (src:284-294) for k < batch: b_k = b + k strideb (m) <- [x_k; tail of Q'b_k].
template <int NC, typename T>
__global__ __launch_bounds__(64 * BQW_WAVES, bqw_min_waves<T>(NC)) void k_batched_ldiv_wave(const T *__restrict__ A, int64_t lda, int64_t strideA,
                                                                                           int m, int n, const T *__restrict__ alpha,
                                                                                           int64_t stride_alpha, T *__restrict__ b,
                                                                                           int64_t strideb, int64_t batch) {
  const int l = bqw_lane();
  const int64_t k = bqw_matrix();
  if (k >= batch) return;  // (the whole wave)
  const T *Ak = A + k * strideA;
  T a[NC];
  bqw_load(a, Ak, lda, m, n, l);
  T *bk = b + k * strideb;
  const double al = l < n ? (double)alpha[k * stride_alpha + l] : 1.0;  // lane j: alpha_j
  bqw_col<T> bb[1];
  bqw_col_set(bb[0], l < m ? (double)bk[l] : 0.0);
  // ---- b <- Q'b: reflectors left to right (src:215-224)
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < n) bqw_reflect_group(bqw_reflector(a, c, l), bb, (c & 7) == 7);  // (wave-uniform)
  bqw_col_renorm(bb);
  // ---- back substitution, columns right to left (src:244-254)
  const double rinv = dhqr_rcp(al);
#pragma unroll
  for (int c = NC - 1; c >= 0; --c)
    if (c < n) bqw_backsub_group(c, l, a[c], al, rinv, bb);
  if (l < m) bk[l] = (T)bqw_col_value(bb[0]);
}
