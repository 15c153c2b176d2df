// dhqr_batched.h -- qr!(A_k) and H_k \ b_k for a BATCH of tiny matrices: one WAVE per matrix.
//
// The single-workgroup kernels of dhqr_small.h give a whole compute unit to one matrix; their smallest instantiation
// occupies 576 threads for a 16 x 8 matrix that fills 1/128 of its registers.  A batch of matrices of at most 64 rows and
// 32 columns (local fits, per-pixel regressions) runs here with ONE WAVE per matrix and BQW_WAVES matrices per workgroup:
//
//   lane l holds row l of every column (a[c], c < NC; NC = 8, 16 or 32, the smallest that holds n), so a column is one
//   coalesced access, a dot product v_j' a_c (partialdot, src:42-49) is one multiplication and a DPP wave reduction, the
//   update (hotloop!, src:156-160) one fma.  Nothing is shared between the waves of a workgroup: no LDS, no barrier, no
//   flag and no wait of any kind; a wave without a matrix leaves at once.
//
// The arithmetic is the reference's, column by column (src:122-148, 198-213), with the pieces of dhqr_small.h: the norm in
// double-double (dd_add_sq + wave_sum_dd_plain), alpha / f / pivot as k_small_qr_d's builder forms them (sign(0) = 0 and the
// overflow branch included); the solve carries b in double-double through Q'b and the back substitution and rounds once per
// entry, for the reason written at k_small_ldiv.
//
// A register array indexed by a runtime column goes to scratch memory, and the fully unrolled factorisation of 32 columns
// is 500 column updates of straight-line code.  So the reflector loop runs over a RUNTIME j: column j is taken out of (and
// put back into) the register array by a chain of selects over the compile-time index, and the trailing update walks the
// columns in unrolled groups of four under one uniform branch per group (finished groups are skipped; inside a group the
// four reductions are independent and interleave).
#pragma once
#include "dhqr_small.h"

#define BQW_WAVES 4  // matrices per workgroup (256 threads)
#define BQW_MAX_M 64
#define BQW_MAX_N 32
// waves per SIMD the register allocation must leave room for: the matrix takes 2 NC registers of a lane's 512 / waves
#define BQW_MIN_WAVES(NC_) ((NC_) <= 8 ? 8 : ((NC_) <= 16 ? 6 : 4))

// householder!(A_k, alpha_k) for k < batch: A_k = A + k strideA (m x n, m <= 64, n <= NC, m >= n >= 1), in place.
template <int NC>
__global__ __launch_bounds__(64 * BQW_WAVES, BQW_MIN_WAVES(NC)) void k_batched_qr_wave(double *__restrict__ A, int64_t lda, int64_t strideA, int m,
                                                                    int n, double *__restrict__ alpha, int64_t stride_alpha,
                                                                    int64_t batch) {
  static_assert(NC % 4 == 0 && NC <= BQW_MAX_N, "columns in groups of four");
  const int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + (threadIdx.x >> 6);
  if (k >= batch) return;  // (the whole wave)
  double *Ak = A + k * strideA;
  double a[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool in = c < n && l < m;  // (no branch: every load of the matrix is in flight before the first use)
    const double t = Ak[in ? (int64_t)l + (int64_t)c * lda : 0];
    a[c] = in ? t : 0.0;
  }
  double alv = 0.0;  // lane j keeps alpha_j
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    double x = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) x = (c == j) ? a[c] : x;
    // reflector j (src:129-140): rows >= m hold zeros
    dhqr_dd acc = {0.0, 0.0};
    dd_add_sq(acc, l >= j ? x : 0.0);
    const dhqr_dd ss = wave_sum_dd_plain(acc);
    const double s2 = ss.hi + ss.lo;
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
    const double v = l > j ? x * f : (l == j ? piv : 0.0);  // src:133-140
    if (l == j) alv = al;
    const double xv = l >= j ? v : x;  // rows < j keep R
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = (c == j) ? xv : a[c];
    // trailing update (src:198-213): columns >= n hold zeros and stay zeros
#pragma unroll
    for (int g = 0; g < NC / 4; ++g) {
      if (4 * g + 3 > j && 4 * g < n) {
        double d[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) d[cc] = wave_sum_dpp(v * a[4 * g + cc]);  // src:42-49
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)  // src:156-160, src:209: rows >= j of the columns behind j, nothing else (a reflector of a
          a[4 * g + cc] = (4 * g + cc > j && l >= j) ? fma(-v, d[cc], a[4 * g + cc]) : a[4 * g + cc];  // zero column is NaN: 0 * NaN)
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
__global__ __launch_bounds__(64 * BQW_WAVES, BQW_MIN_WAVES(NC)) void k_batched_ldiv_wave(const double *__restrict__ A, int64_t lda, int64_t strideA,
                                                                      int m, int n, const double *__restrict__ alpha,
                                                                      int64_t stride_alpha, double *__restrict__ b,
                                                                      int64_t strideb, int64_t batch) {
  const int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + (threadIdx.x >> 6);
  if (k >= batch) return;  // (the whole wave)
  const double *Ak = A + k * strideA;
  double *bk = b + k * strideb;
  double a[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool in = c < n && l < m;  // (no branch: every load of the matrix is in flight before the first use)
    const double t = Ak[in ? (int64_t)l + (int64_t)c * lda : 0];
    a[c] = in ? t : 0.0;
  }
  const double al = l < n ? alpha[k * stride_alpha + l] : 1.0;  // lane j: alpha_j
  dhqr_dd bb;
  bb.hi = l < m ? bk[l] : 0.0;
  bb.lo = 0.0;
  // ---- b <- Q'b: reflectors left to right (src:215-224)
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c < n) {  // (wave-uniform)
      const double v = l >= c ? a[c] : 0.0;  // rows < c of a factored column hold R
      dhqr_dd p = {0.0, 0.0};
      dd_add_prod(p, v, bb.hi);  // src:217: v_i b_i, b_i = hi + lo
      p.lo = fma(v, bb.lo, p.lo);
      const dhqr_dd sd = wave_sum_dd_plain(p);
      const double s = sd.hi + sd.lo;
      dd_add_prod(bb, -s, v);  // src:218-220: b_i -= v_i s
      if ((c & 7) == 7) dd_renorm(bb);  // the low part stays small against the high one
    }
  }
  dd_renorm(bb);
  // ---- back substitution, columns right to left (src:244-254): x_j = b_j / alpha_j, b[0:j] -= R[0:j, j] x_j
  const double rinv = dhqr_rcp(al);
#pragma unroll
  for (int c = NC - 1; c >= 0; --c) {
    if (c < n) {
      // b_j / alpha_j as k_small_ldiv forms it: reciprocal (off the chain) times b_j and one correction step
      const double bq = smq_readlane(bb.hi + bb.lo, c), aj = smq_readlane(al, c), ri = smq_readlane(rinv, c);
      double xj = bq * ri;
      xj = fma(fma(-aj, xj, bq), ri, xj);
      if (l == c) {
        bb.hi = xj;
        bb.lo = 0.0;
      } else if (l < c) {
        dd_add_prod(bb, -a[c], xj);  // src:248-250
      }
    }
  }
  if (l < m) bk[l] = bb.hi + bb.lo;
}
