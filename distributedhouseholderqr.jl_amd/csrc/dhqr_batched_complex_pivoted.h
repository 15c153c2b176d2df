// dhqr_batched_complex_pivoted.h -- qr!(A_k) with COLUMN PIVOTING and the rank-truncated least-squares solve for a batch of
// small ComplexF64 matrices (dhqr.h: dhqr_factor_batched_pivoted_c64, dhqr_solve_batched_pivoted_c64): the complex twins of
// the kernels of dhqr_batched_pivoted.h, under the rule written there.  What is complex about it:
//   pivot search   the squared norm of an entry is re^2 + im^2, in plain double, unscaled; first maximum, compared with `>`
//   zero tail      alpha_c = 0 and v_c = sqrt(2) e_c -- REAL -- for every remaining column
//   reflector      exactly the expressions of k_batched_zqr_wave (zalphafactor gives -1 at 0: nothing is special-cased)
//   solve          both parts of b in double-double, renormalised after every eighth reflector, Smith's division
//
// Wave tier (m <= 64, n <= 32): k_batched_zqr_wave with the pivot step / k_batched_zldiv_wave_nrhs's arithmetic with the
// wave's own rank in place of n, the columns of B one after the other.  One wave per matrix, BQW_WAVES matrices per
// workgroup, no LDS, no barrier, no flag, no wait.  A column's arithmetic does not depend on the position it sits in, so the
// pivoted factor of A has the BITS of dhqr_factor_batched_c64 on A[:, jpvt], and the solve with rank r those of
// dhqr_solve_batched_nrhs_c64 called with n = r.
//
// General tier (every other shape, and every shape with the small route off): one workgroup per matrix (factor) or per
// (matrix, column of B) (solve), in place in device memory, in plain double but for the reflector's norm.  BARRIER FORM ONLY:
// every loop around a __syncthreads() is bounded by values every thread reads alike (j, n, r, the candidates in LDS).  For
// completeness, not for speed, like the Float64 one.
// Registers (profiles/batched_kernel_resources.txt): no instantiation has scratch memory or a spilled register.
#pragma once
#include "dhqr_batched_complex_nrhs.h"
#include "dhqr_batched_pivoted.h"

// Waves per SIMD the register allocation must leave room for.  The factor keeps the chosen column AND the one that makes
// room for it, the lane's jpvt entry and a group's four norms beside the 4 NC registers of the matrix: k_batched_zqr_wave<8>
// fills its 64 registers already (BQZ_MIN_WAVES(8) = 8), so NC = 8 takes the solve's bound of six here; NC = 16 and 32 keep
// BQZ_MIN_WAVES.
#define BQZP_MIN_WAVES(NC_) ((NC_) <= 8 ? 6 : BQZ_MIN_WAVES(NC_))

// bqz_load with the column's address carried from column to column instead of formed as c * lda: the NC 64-bit products, alive
// as scalar register pairs while the loads are in flight, do not fit beside these kernels' longer argument lists (NC = 32:
// 40 - 46 scalar registers spilled).  The same guards: a lane without a row reads row 0, a column >= n reads column n - 1
// again, and both drop what they read.
template <int NC>
__device__ __forceinline__ void bqzp_load(double2 (&a)[NC], const double2 *__restrict__ Ak, int64_t lda, int m, int n, int l) {
  const double2 *q = Ak + (l < m ? l : 0);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    a[c] = *q;  // (no branch: every load of the matrix is in flight before the first use)
    q += c + 1 < n ? lda : 0;  // (uniform)
  }
  // the guards, with n as a value of its own: the NC tests c < n above would otherwise wait here as scalar register pairs
  int ns = n;
  BQZ_KEEP_SCALAR_IN_LOOP(ns);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool in = l < m && c < ns;
    a[c] = zmake(in ? a[c].x : 0.0, in ? a[c].y : 0.0);
  }
}

// householder!(A_k P_k, alpha_k) for k < batch, in place; jpvt_k = jpvt + k stride_jpvt receives the n 0-based original
// indices of the columns.  m <= 64, n <= NC, m >= n >= 1.  lda and the strides of A and alpha count complex elements.
template <int NC>
__global__ __launch_bounds__(64 * BQW_WAVES, BQZP_MIN_WAVES(NC)) void k_batched_zqrp_wave(double2 *__restrict__ A, int64_t lda, int64_t strideA,
                                                                       int m, int n, double2 *__restrict__ alpha,
                                                                       int64_t stride_alpha, int32_t *__restrict__ jpvt,
                                                                       int64_t stride_jpvt, int64_t batch) {
  static_assert(NC % 4 == 0 && NC <= BQW_MAX_N, "columns in groups of four");
  const int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + (threadIdx.x >> 6);
  if (k >= batch) return;  // (the whole wave)
  double2 *Ak = A + k * strideA;
  double2 a[NC];
  bqzp_load<NC>(a, Ak, lda, m, n, l);
  double2 alv = zmake(0.0, 0.0);  // lane j keeps alpha_j
  int jp = l;                     // lane c keeps jpvt[c]
  int jz = n;                     // the first column of the zero tail
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    // pivot search: the squared norms of rows >= j of the columns j .. n-1, afresh; the first maximum
    // (n as a value of this step's own: the NC tests c < n of the load would otherwise be carried into the loop, spilled)
    int nj = n;
    BQZ_KEEP_SCALAR_IN_LOOP(nj);
    double bestv = -1.0;
    int p = j;
#pragma unroll
    for (int g = 0; g < NC / 4; ++g) {
      if (4 * g + 3 >= j && 4 * g < nj) {
        double d[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          const double tr = l >= j ? a[4 * g + cc].x : 0.0, ti = l >= j ? a[4 * g + cc].y : 0.0;
          d[cc] = wave_sum_dpp(tr * tr + ti * ti);
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          const bool take = 4 * g + cc >= j && 4 * g + cc < nj && d[cc] > bestv;  // (wave-uniform)
          bestv = take ? d[cc] : bestv;
          p = take ? 4 * g + cc : p;
        }
      }
    }
    if (bestv == 0.0) {  // the rest of the matrix is zero: no more swaps (the tail is written behind the loop)
      jz = j;
      break;
    }
    // the chosen column, and the one that makes room for it: select chains inside the columns' own groups of four
    double2 x = zmake(0.0, 0.0), xj = zmake(0.0, 0.0);
#pragma unroll
    for (int g = 0; g < NC / 4; ++g) {
      if (g == (p >> 2)) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          x.x = (cc == (p & 3)) ? a[4 * g + cc].x : x.x;
          x.y = (cc == (p & 3)) ? a[4 * g + cc].y : x.y;
        }
      }
      if (g == (j >> 2)) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          xj.x = (cc == (j & 3)) ? a[4 * g + cc].x : xj.x;
          xj.y = (cc == (j & 3)) ? a[4 * g + cc].y : xj.y;
        }
      }
    }
    {
      const int pj = __builtin_amdgcn_readlane(jp, j), pp = __builtin_amdgcn_readlane(jp, p);
      jp = l == j ? pp : (l == p ? pj : jp);
    }
    // reflector j (src:129-140, k_zreflector): the expressions of k_batched_zqr_wave; rows >= m hold zeros
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
    for (int g = 0; g < NC / 4; ++g) {  // the swap, then the reflector in its place (p == j: the reflector alone)
      if (g == (p >> 2)) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          a[4 * g + cc].x = (cc == (p & 3)) ? xj.x : a[4 * g + cc].x;
          a[4 * g + cc].y = (cc == (p & 3)) ? xj.y : a[4 * g + cc].y;
        }
      }
      if (g == (j >> 2)) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          a[4 * g + cc].x = (cc == (j & 3)) ? xv.x : a[4 * g + cc].x;
          a[4 * g + cc].y = (cc == (j & 3)) ? xv.y : a[4 * g + cc].y;
        }
      }
    }
    // trailing update (src:198-213): columns >= n hold zeros and stay zeros
#pragma unroll
    for (int g = 0; g < NC / 4; ++g) {
      if (4 * g + 3 > j && 4 * g < nj) {
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
  // The lane index and n once more, as values of their own (k_batched_zqr_wave says why), for the zero tail and the stores.
  // The zero tail: alpha_c = 0 (alv is 0 in the lanes >= jz), v_c = sqrt(2) e_c for c >= jz.
  int ls = l, ns = n;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(ls), "+s"(ns), "+s"(jz));
#endif
  double2 *q = Ak + ls;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c >= jz) {  // (uniform)
      a[c].x = ls >= c ? (ls == c ? BQP_SQRT2 : 0.0) : a[c].x;
      a[c].y = ls >= c ? 0.0 : a[c].y;
    }
    if (c < ns && ls < m) *q = a[c];
    q += lda;
  }
  if (l < n) {
    alpha[k * stride_alpha + l] = alv;
    jpvt[k * stride_jpvt + l] = jp;
  }
}

// The rank-truncated solve for k < batch and every column q < nrhs of B_k: with r = clamp(rank[k], 0, n) the column
// b <- [z; tail] as k_batched_zldiv_wave_nrhs leaves it on the first r columns of the factor, and column q of X_k (n) <- the
// basic solution x[jpvt[i]] = z_i (i < r), exact zeros (+0 + 0i) elsewhere.  r = 0: b stays untouched.  The columns are
// taken one after the other: a column's bits depend neither on nrhs nor on its place nor on the batch.
template <int NC>
__global__ __launch_bounds__(64 * BQW_WAVES, BQZ_MIN_WAVES_LDIV(NC)) void k_batched_zldivp_wave(
    const double2 *__restrict__ A, int64_t lda, int64_t strideA, int m, int n, const double2 *__restrict__ alpha, int64_t stride_alpha,
    const int32_t *__restrict__ jpvt, int64_t stride_jpvt, const int32_t *__restrict__ rank, double2 *__restrict__ B, int nrhs,
    int64_t ldb, int64_t strideB, double2 *__restrict__ X, int64_t ldx, int64_t strideX, int64_t batch) {
  int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (a scalar)
  if (k >= batch) return;  // (the whole wave)
  double2 a[NC];
  bqzp_load<NC>(a, A + k * strideA, lda, m, n, l);
  const int rk = __builtin_amdgcn_readfirstlane(rank[k]);
  int r = rk < 0 ? 0 : (rk > n ? n : rk);  // wave-uniform
  const double2 alt = alpha[k * stride_alpha + (l < r ? l : 0)];  // (alpha_k[0] exists: n >= 1)
  double2 al = zmake(l < r ? alt.x : 1.0, l < r ? alt.y : 0.0);  // lane j: alpha_j
  const int jp = l < n ? jpvt[k * stride_jpvt + l] : -1;
  double2 *Bk = B + k * strideB, *Xk = X + k * strideX;
#pragma unroll 1
  for (int q = 0; q < nrhs; ++q) {
    bqz_keep_in_loop<NC>(a, l);
    BQZ_KEEP_SCALAR_IN_LOOP(r);
    BQN_KEEP_IN_LOOP(al.x);
    BQN_KEEP_IN_LOOP(al.y);
    double2 *bk = Bk + (int64_t)q * ldb;
    dhqr_dd br[1], bi[1];  // b = (br, bi), each hi + lo
    {
      const double2 t = bk[l < m ? l : 0];  // (no branch; B_k[0] exists: m, nrhs >= 1)
      br[0].hi = l < m ? t.x : 0.0;
      br[0].lo = 0.0;
      bi[0].hi = l < m ? t.y : 0.0;
      bi[0].lo = 0.0;
    }
    // ---- b <- Q_r^H b: reflectors left to right (src:215-224, k_zqtb_col_dd)
    zstatic_for(
        [&](auto cc) {
          constexpr int c = decltype(cc)::value;
          if (c < r) {  // (wave-uniform)
            const double2 v = zmake(l >= c ? a[c].x : 0.0, l >= c ? a[c].y : 0.0);  // rows < c of a factored column hold R
            bqz_reflect_group<1>(v, br, bi, (c & 7) == 7);
          }
        },
        std::make_integer_sequence<int, NC>{});
    dd_renorm(br[0]);
    dd_renorm(bi[0]);
    // ---- back substitution on R11, columns right to left (src:244-254, k_zbacksub_diag_dd)
    BQN_KEEP_IN_LOOP(l);
    BQZ_KEEP_SCALAR_IN_LOOP(r);
    zstatic_for(
        [&](auto cc) {
          constexpr int c = NC - 1 - decltype(cc)::value;
          if (c < r) {
            const double2 xc = zdiv(bqz_readlane(zmake(br[0].hi + br[0].lo, bi[0].hi + bi[0].lo), c), bqz_readlane(al, c));  // src:251
            if (l == c) {
              br[0].hi = xc.x;
              br[0].lo = 0.0;
              bi[0].hi = xc.y;
              bi[0].lo = 0.0;
            } else if (l < c) {  // src:248-250: b_l -= R_lc x_c
              const double2 rr = a[c];
              dd_add_prod(br[0], -rr.x, xc.x);
              dd_add_prod(br[0], rr.y, xc.y);
              dd_add_prod(bi[0], -rr.x, xc.y);
              dd_add_prod(bi[0], -rr.y, xc.x);
            }
          }
        },
        std::make_integer_sequence<int, NC>{});
    const double2 z = zmake(br[0].hi + br[0].lo, bi[0].hi + bi[0].lo);
    if (r > 0 && l < m) bk[l] = z;
    // jpvt is a permutation: every entry of the column is written once (an index out of range is not written at all)
    if (l < n && jp >= 0 && jp < n) Xk[(int64_t)q * ldx + jp] = l < r ? z : zmake(0.0, 0.0);
  }
}

// ---- the general tier ----------------------------------------------------------------------------------------------------
// Workgroup k factors matrix k (any m >= n >= 1) in place in device memory: k_batched_qrp_general's steps and barriers with
// complex elements.  All control flow around the barriers depends on j, n and values every thread reads from LDS alike.
__global__ __launch_bounds__(BQPG_THREADS) void k_batched_zqrp_general(double2 *__restrict__ A, int64_t lda, int64_t strideA, int64_t m,
                                                                        int64_t n, double2 *__restrict__ alpha, int64_t stride_alpha,
                                                                        int32_t *__restrict__ jpvt, int64_t stride_jpvt) {
  constexpr int NW = BQPG_THREADS / 64;
  __shared__ double red[2 * NW];
  __shared__ double candv[NW];
  __shared__ int64_t candc[NW];
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  double2 *Ak = A + (int64_t)blockIdx.x * strideA;
  double2 *alk = alpha + (int64_t)blockIdx.x * stride_alpha;
  int32_t *jk = jpvt + (int64_t)blockIdx.x * stride_jpvt;  // (thread 0 alone reads and writes it)
  if (t == 0)
    for (int64_t c = 0; c < n; ++c) jk[c] = (int32_t)c;
  for (int64_t j = 0; j < n; ++j) {
    double bestv = -1.0;
    int64_t p = j;
    for (int64_t c = j + w; c < n; c += NW) {
      const double2 *col = Ak + c * lda;
      double s = 0.0;
      for (int64_t i = j + l; i < m; i += 64) {
        const double2 e = col[i];
        s = fma(e.x, e.x, s);
        s = fma(e.y, e.y, s);
      }
      s = wave_sum_dpp(s);
      if (s > bestv) {  // (wave-uniform)
        bestv = s;
        p = c;
      }
    }
    if (l == 0) {
      candv[w] = bestv;
      candc[w] = p;
    }
    __syncthreads();
    bestv = -1.0;
    p = j;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const double cv = candv[i];
      const int64_t cc = candc[i];
      if (cv > bestv || (cv == bestv && cv >= 0.0 && cc < p)) {
        bestv = cv;
        p = cc;
      }
    }
    if (bestv == 0.0) {  // the rest of the matrix is zero (the same decision in every thread)
      for (int64_t c = j; c < n; ++c) {
        for (int64_t i = c + t; i < m; i += BQPG_THREADS) Ak[i + c * lda] = zmake(i == c ? BQP_SQRT2 : 0.0, 0.0);
        if (t == 0) alk[c] = zmake(0.0, 0.0);
      }
      break;
    }
    if (p != j) {
      for (int64_t i = t; i < m; i += BQPG_THREADS) {
        const double2 u = Ak[i + j * lda];
        Ak[i + j * lda] = Ak[i + p * lda];
        Ak[i + p * lda] = u;
      }
      if (t == 0) {
        const int32_t u = jk[j];
        jk[j] = jk[p];
        jk[p] = u;
      }
    }
    __syncthreads();  // column j is in place (and candv / candc have been read)
    double2 *vj = Ak + j * lda;
    dhqr_dd acc = {0.0, 0.0};
    for (int64_t i = j + t; i < m; i += BQPG_THREADS) {
      const double2 e = vj[i];
      dd_add_sq(acc, e.x);
      dd_add_sq(acc, e.y);
    }
    const double sn = sqrt(dd_block_sum<BQPG_THREADS>(acc, red));  // src:129
    const double2 h = vj[j];
    double ah;
    const double2 af = zalphafactor(h, &ah);
    const double2 al = zmake(sn * af.x, sn * af.y);  // src:130
    const double f = 1.0 / sqrt(sn * (sn + ah));     // src:131
    const double2 piv = zmake((h.x - al.x) * f, (h.y - al.y) * f);  // src:132
    __syncthreads();  // every thread has read h
    for (int64_t i = j + t; i < m; i += BQPG_THREADS) {  // src:133-140
      const double2 e = vj[i];
      vj[i] = i == j ? piv : zmake(e.x * f, e.y * f);
    }
    if (t == 0) alk[j] = al;
    __syncthreads();  // the reflector is in memory
    for (int64_t c = j + 1 + w; c < n; c += NW) {  // src:198-213
      double2 *col = Ak + c * lda;
      double sr = 0.0, si = 0.0;
      for (int64_t i = j + l; i < m; i += 64) zcdot_acc(vj[i], col[i], sr, si);
      sr = wave_sum_dpp(sr);
      si = wave_sum_dpp(si);
      for (int64_t i = j + l; i < m; i += 64) col[i] = zsubmul(col[i], vj[i], sr, si);
    }
    __syncthreads();  // the trailing matrix is in memory for the next step's norms
  }
}

// Workgroup w of a 1-D grid of batch * nrhs solves column q = w % nrhs of matrix k = w / nrhs with r = clamp(rank[k], 0, n):
// Q_r^H b as k_batched_zapplyq_general applies it, the back substitution on R11 with two barriers per column (x_c formed by
// every thread | b_c overwritten by its owner), the scatter through jpvt.
__global__ __launch_bounds__(BQPG_THREADS) void k_batched_zldivp_general(const double2 *__restrict__ A, int64_t lda, int64_t strideA, int64_t m,
                                                                          int64_t n, const double2 *__restrict__ alpha, int64_t stride_alpha,
                                                                          const int32_t *__restrict__ jpvt, int64_t stride_jpvt,
                                                                          const int32_t *__restrict__ rank, double2 *__restrict__ B,
                                                                          int64_t nrhs, int64_t ldb, int64_t strideB, double2 *__restrict__ X,
                                                                          int64_t ldx, int64_t strideX) {
  constexpr int NW = BQPG_THREADS / 64;
  __shared__ double red[2 * NW];
  const int t = threadIdx.x;
  const int64_t k = (int64_t)blockIdx.x / nrhs, q = (int64_t)blockIdx.x - k * nrhs;
  const double2 *Ak = A + k * strideA, *alk = alpha + k * stride_alpha;
  const int32_t *jk = jpvt + k * stride_jpvt;
  double2 *bcol = B + k * strideB + q * ldb, *xcol = X + k * strideX + q * ldx;
  const int64_t rk = rank[k];
  const int64_t r = rk < 0 ? 0 : (rk > n ? n : rk);  // (the same in every thread)
  for (int64_t c = 0; c < r; ++c) {
    const double2 *vc = Ak + c * lda;  // rows < c of a factored column hold R
    double sr = 0.0, si = 0.0;
    for (int64_t i = t; i < m; i += BQPG_THREADS)
      if (i >= c) zcdot_acc(vc[i], bcol[i], sr, si);  // src:217: conj(v_i) b_i
    sr = wave_sum_dpp(sr);
    si = wave_sum_dpp(si);
    if ((t & 63) == 0) {
      red[2 * (t >> 6)] = sr;
      red[2 * (t >> 6) + 1] = si;
    }
    __syncthreads();
    double s_r = 0.0, s_i = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      s_r += red[2 * i];
      s_i += red[2 * i + 1];
    }
    __syncthreads();
    for (int64_t i = t; i < m; i += BQPG_THREADS)
      if (i >= c) bcol[i] = zsubmul(bcol[i], vc[i], s_r, s_i);  // src:218-220: b_i -= v_i s
  }
  for (int64_t cc = 0; cc < r; ++cc) {  // src:244-254
    const int64_t c = r - 1 - cc;
    __syncthreads();  // b_c has all its updates
    const double2 xc = zdiv(bcol[c], alk[c]);
    __syncthreads();  // every thread has read b_c
    for (int64_t i = t; i <= c; i += BQPG_THREADS) bcol[i] = i == c ? xc : zsubmul(bcol[i], Ak[i + c * lda], xc.x, xc.y);
  }
  __syncthreads();
  for (int64_t i = t; i < n; i += BQPG_THREADS) {
    const int64_t pi = jk[i];
    if (pi >= 0 && pi < n) xcol[pi] = i < r ? bcol[i] : zmake(0.0, 0.0);
  }
}
