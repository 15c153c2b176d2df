// dhqr_batched_complex.h -- qr!(A_k) and H_k \ b_k for a BATCH of tiny ComplexF64 matrices: one WAVE per matrix.
//
// The complex twins of k_batched_qr_wave / k_batched_ldiv_wave (dhqr_batched.h), for the same shapes -- at most 64 rows and
// 32 columns -- and with the same layout: BQW_WAVES matrices per workgroup, nothing shared between its waves (no LDS, no
// barrier, no flag and no wait of any kind), a wave without a matrix leaves at once.
//
//   lane l holds row l of every column as (re, im) (a[c], c < NC; NC = 8, 16 or 32, the smallest that holds n): 4 NC
//   registers for the matrix, a column is one coalesced 16-byte-per-lane access, the conj-dot v_j^H a_c (partialdot,
//   src:51-59) four fma and two DPP wave reductions, the update (hotloop!, src:171-196) four fma.
//
// The arithmetic is the reference's, column by column, with the pieces of dhqr_complex.h: the norm in double-double
// (dd_add_sq on both parts + wave_sum_dd_plain), alpha / f / pivot as k_zreflector forms them (zalphafactor: angle(0) = 0, so
// a zero pivot gives the factor -1, not the real type's sign(0) = 0), zcdot_acc and zsubmul for the trailing update; the
// solve carries b in double-double per component through Q'b (the per-lane expressions of k_zqtb_col_dd) and the back
// substitution (k_zbacksub_diag_dd: Smith's division by alpha_j) and rounds once per entry.
//
// The loop shape is that of k_batched_qr_wave, for the reasons written there: a RUNTIME column j, taken out of and put back
// into the register array by select chains, the trailing update in unrolled groups of four columns under one uniform branch
// per group.  The select chains, too, run inside j's own group of four under a uniform branch: four selects per part
// instead of NC, and four scalar masks instead of NC.
// Registers (profiles/batched_c64_kernel_resources.txt): no instantiation has scratch memory or a spilled register.
#pragma once
#include "dhqr_batched.h"
#include "dhqr_complex.h"

// waves per SIMD the register allocation must leave room for: the matrix takes 4 NC registers of a lane's 512 / waves
#define BQZ_MIN_WAVES(NC_) ((NC_) <= 8 ? 8 : ((NC_) <= 16 ? 4 : 2))
// the solve keeps b and its double-double sums beside the matrix: at NC = 8 they do not fit 64 registers, so six waves there
#define BQZ_MIN_WAVES_LDIV(NC_) ((NC_) <= 8 ? 6 : BQZ_MIN_WAVES(NC_))

__device__ __forceinline__ double2 bqz_readlane(const double2 v, int lane) {  // lane: wave-uniform
  return zmake(smq_readlane(v.x, lane), smq_readlane(v.y, lane));
}
// The matrix of wave k into registers, in the guarded-index form of k_batched_qr_wave: every load is in flight before the
// first use and no lane touches memory outside its matrix (a lane without a row, or a column >= n, reads element 0 and
// drops it).  The row mask and the uniform column test are applied one after the other: their 32 products, one scalar
// register pair each, alive while the loads are in flight, do not fit the scalar registers.
template <int NC>
__device__ __forceinline__ void bqz_load(double2 (&a)[NC], const double2 *__restrict__ Ak, int64_t lda, int m, int n, int l) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int64_t col = c < n ? (int64_t)c * lda : 0;  // (uniform)
    const double2 t = Ak[l < m ? (int64_t)l + col : 0];  // (no branch)
    a[c] = zmake(l < m ? t.x : 0.0, l < m ? t.y : 0.0);
    if (c >= n) a[c] = zmake(0.0, 0.0);
  }
}

// householder!(A_k, alpha_k) for k < batch: A_k = A + k strideA (m x n, m <= 64, n <= NC, m >= n >= 1), in place.
// lda and the strides count complex elements.
template <int NC>
__global__ __launch_bounds__(64 * BQW_WAVES, BQZ_MIN_WAVES(NC)) void k_batched_zqr_wave(double2 *__restrict__ A, int64_t lda, int64_t strideA,
                                                                     int m, int n, double2 *__restrict__ alpha,
                                                                     int64_t stride_alpha, int64_t batch) {
  static_assert(NC % 4 == 0 && NC <= BQW_MAX_N, "columns in groups of four");
  const int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + (threadIdx.x >> 6);
  if (k >= batch) return;  // (the whole wave)
  double2 *Ak = A + k * strideA;
  double2 a[NC];
  bqz_load<NC>(a, Ak, lda, m, n, l);
  double2 alv = zmake(0.0, 0.0);  // lane j keeps alpha_j
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    double2 x = zmake(0.0, 0.0);
#pragma unroll
    for (int g = 0; g < NC / 4; ++g)
      if ((j >> 2) == g) {  // (uniform: the select chain of j's own group of four)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          x.x = (cc == (j & 3)) ? a[4 * g + cc].x : x.x;
          x.y = (cc == (j & 3)) ? a[4 * g + cc].y : x.y;
        }
      }
    // reflector j (src:129-140, k_zreflector): rows >= m hold zeros
    dhqr_dd acc = {0.0, 0.0};
    dd_add_sq(acc, l >= j ? x.x : 0.0);
    dd_add_sq(acc, l >= j ? x.y : 0.0);
    const dhqr_dd ss = wave_sum_dd_plain(acc);
    const double sn = sqrt(ss.hi + ss.lo);  // src:129
    const double2 h = bqz_readlane(x, j);
    double ah;
    const double2 af = zalphafactor(h, &ah);
    const double2 al = zmake(sn * af.x, sn * af.y);  // src:130
    const double f = 1.0 / sqrt(sn * (sn + ah));     // src:131
    const double2 piv = zmake((h.x - al.x) * f, (h.y - al.y) * f);  // src:132
    double2 v;                                                      // src:133-140
    v.x = l > j ? x.x * f : (l == j ? piv.x : 0.0);
    v.y = l > j ? x.y * f : (l == j ? piv.y : 0.0);
    if (l == j) alv = al;
    const double2 xv = zmake(l >= j ? v.x : x.x, l >= j ? v.y : x.y);  // rows < j keep R
#pragma unroll
    for (int g = 0; g < NC / 4; ++g)
      if ((j >> 2) == g) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          a[4 * g + cc].x = (cc == (j & 3)) ? xv.x : a[4 * g + cc].x;
          a[4 * g + cc].y = (cc == (j & 3)) ? xv.y : a[4 * g + cc].y;
        }
      }
    // trailing update (src:198-213): columns >= n hold zeros and stay zeros
#pragma unroll
    for (int g = 0; g < NC / 4; ++g) {
      if (4 * g + 3 > j && 4 * g < n) {
        double dr[4], di[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {  // src:51-59: conj(v) . a_c (v is zero above row j)
          double sr = 0.0, si = 0.0;
          zcdot_acc(v, a[4 * g + cc], sr, si);
          dr[cc] = wave_sum_dpp(sr);
          di[cc] = wave_sum_dpp(si);
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {  // src:171-196, src:209: rows >= j of the columns behind j, nothing else
          const double2 u = zsubmul(a[4 * g + cc], v, dr[cc], di[cc]);
          const bool upd = 4 * g + cc > j && l >= j;
          a[4 * g + cc].x = upd ? u.x : a[4 * g + cc].x;
          a[4 * g + cc].y = upd ? u.y : a[4 * g + cc].y;
        }
      }
    }
  }
  // The lane index and n once more, as values of their own: derived from `l` and `n`, the row and column masks and the
  // addresses of these stores are formed ahead of the column loop and carried through it in scalar registers that spill.
  int ls = l, ns = n;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(ls), "+s"(ns));
#endif
  double2 *q = Ak + ls;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c < ns && ls < m) *q = a[c];
    q += lda;
  }
  if (l < n) alpha[k * stride_alpha + l] = alv;
}

// solve_householder!(b_k, H_k, alpha_k) (src:284-294) for k < batch: b_k = b + k strideb (m) <- [x_k; tail of Q'b_k].
template <int NC>
__global__ __launch_bounds__(64 * BQW_WAVES, BQZ_MIN_WAVES_LDIV(NC)) void k_batched_zldiv_wave(const double2 *__restrict__ A, int64_t lda,
                                                                       int64_t strideA, int m, int n,
                                                                       const double2 *__restrict__ alpha, int64_t stride_alpha,
                                                                       double2 *__restrict__ b, int64_t strideb, int64_t batch) {
  const int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + (threadIdx.x >> 6);
  if (k >= batch) return;  // (the whole wave)
  const double2 *Ak = A + k * strideA;
  double2 *bk = b + k * strideb;
  double2 a[NC];
  bqz_load<NC>(a, Ak, lda, m, n, l);
  const double2 alt = alpha[k * stride_alpha + (l < n ? l : 0)];
  const double2 al = zmake(l < n ? alt.x : 1.0, l < n ? alt.y : 0.0);  // lane j: alpha_j
  const double2 bt = bk[l < m ? l : 0];
  dhqr_dd br = {l < m ? bt.x : 0.0, 0.0}, bi = {l < m ? bt.y : 0.0, 0.0};  // b = (br, bi), each hi + lo
  // ---- b <- Q'b: reflectors left to right (src:215-224, k_zqtb_col_dd)
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c < n) {  // (wave-uniform)
      const double2 v = zmake(l >= c ? a[c].x : 0.0, l >= c ? a[c].y : 0.0);  // rows < c of a factored column hold R
      dhqr_dd sr = {0.0, 0.0}, si = {0.0, 0.0};
      dd_add_prod(sr, v.x, br.hi);  // src:217: conj(v_i) b_i
      dd_add_prod(sr, v.y, bi.hi);
      dd_add_prod(si, v.x, bi.hi);
      dd_add_prod(si, -v.y, br.hi);
      sr.lo += v.x * br.lo + v.y * bi.lo;
      si.lo += v.x * bi.lo - v.y * br.lo;
      const dhqr_dd tr = wave_sum_dd_plain(sr), ti = wave_sum_dd_plain(si);
      const double s_r = tr.hi + tr.lo, s_i = ti.hi + ti.lo;
      dd_add_prod(br, -s_r, v.x);  // src:218-220: b_i -= v_i s
      dd_add_prod(br, s_i, v.y);
      dd_add_prod(bi, -s_i, v.x);
      dd_add_prod(bi, -s_r, v.y);
      if ((c & 7) == 7) {  // the low parts stay small against the high ones
        dd_renorm(br);
        dd_renorm(bi);
      }
    }
  }
  dd_renorm(br);
  dd_renorm(bi);
  // ---- back substitution, columns right to left (src:244-254, k_zbacksub_diag_dd): x_j = b_j / alpha_j, b[0:j] -= R[0:j, j] x_j
#pragma unroll
  for (int c = NC - 1; c >= 0; --c) {
    if (c < n) {
      const double2 xj = zdiv(bqz_readlane(zmake(br.hi + br.lo, bi.hi + bi.lo), c), bqz_readlane(al, c));  // src:251
      if (l == c) {
        br.hi = xj.x;
        br.lo = 0.0;
        bi.hi = xj.y;
        bi.lo = 0.0;
      } else if (l < c) {  // src:248-250: b_l -= R_lc x_c
        const double2 r = a[c];
        dd_add_prod(br, -r.x, xj.x);
        dd_add_prod(br, r.y, xj.y);
        dd_add_prod(bi, -r.x, xj.y);
        dd_add_prod(bi, -r.y, xj.x);
      }
    }
  }
  if (l < m) bk[l] = zmake(br.hi + br.lo, bi.hi + bi.lo);
}
