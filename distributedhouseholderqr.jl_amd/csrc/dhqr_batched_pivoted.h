// dhqr_batched_pivoted.h -- qr!(A_k) with COLUMN PIVOTING, the numerical rank and the rank-truncated least-squares solve
// for a batch of small Float64 or Float32 matrices (dhqr.h: dhqr_factor_batched_pivoted_f64 / _f32, dhqr_rank_batched_*,
// dhqr_solve_batched_pivoted_*; the ComplexF64 kernels: dhqr_batched_complex_pivoted.h): A_k P_k = Q_k R_k as LAPACK's geqp3 orders it, min ||A_k x - b|| with the columns behind
// the rank dropped as gelsy's basic solution drops them.  The reference has no counterpart; the factor keeps its format
// (reflectors below the diagonal, R above, alpha on it) and adds one int32 permutation per matrix, so every routine that
// takes a factor (apply-Q, explicit Q and R) takes a pivoted one unchanged.
//
// The pivot rule, the same on both tiers: at step j the squared 2-norms of the trailing columns (rows >= j) are computed
// AFRESH from the working matrix in plain double -- no downdating, so no cancellation safeguard --, the smallest column
// index that attains the maximum is taken (compared with `>`: a NaN never wins), columns j and p are swapped in whole (the R
// rows above the diagonal included) and so are their entries of jpvt.  The pivot search is NOT scaled: entries are 0 or of
// magnitude within [1e-150, 1e150].  A maximum of exactly 0 means the rest of the matrix is zero: every remaining column c
// gets alpha_c = 0 and the reflector v_c = sqrt(2) e_c (H_c = I - v v' flips e_c: a valid reflector, a finite factor) and
// there are no more swaps.  The reflector of the chosen column is formed by the expressions of k_batched_qr_wave, except
// that alphafactor(0) = -1 (as the ComplexF64 routes take it, src:9): a pivot entry that is exactly zero must give a valid
// reflector here, not alpha = 0.
//
// Float32 (T = float, the wave tier alone; every other shape is promoted on the host side): the matrix stored in float, the
// pivot norms from the stored values widened -- a product of two floats is exact in double --, every sum in double, every
// stored entry rounded once, as dhqr_wave.h has it for the unpivoted kernels; the zero tail's sqrt(2) is rounded to float.
// The double instantiations are the kernels as they were before T: the same instructions.
//
// Wave tier (m <= 64, n <= 32): k_batched_qr_wave / k_batched_ldiv_wave (dhqr_batched.h) with the pivot step / with the
// wave's own rank in place of n.  One wave per matrix, BQW_WAVES matrices per workgroup, no LDS, no barrier, no flag, no
// wait.  A column's arithmetic does not depend on the position it sits in, so the pivoted factor of A has the BITS of
// dhqr_factor_batched_f64 on A[:, jpvt], and the solve with rank r those of dhqr_solve_batched_f64 called with n = r.
//
// General tier (every other shape, and every shape with the small route off): one workgroup per matrix (factor) or per
// (matrix, column of B) (solve), in place in device memory, in plain double but for the reflector's norm, in the manner of
// k_batched_zapplyq_general.  BARRIER FORM ONLY: every loop is bounded by n and every wave reaches every __syncthreads().
// This tier exists for completeness -- any shape gets an answer --, not for speed: a step reads the trailing matrix from
// memory twice (the norms, the update) and costs seven barriers.
#pragma once
#include "dhqr_batched.h"
#include "dhqr_batched_nrhs.h"

// alphafactor for the pivoted routes: -sign(x) with sign(0) taken as +1 (src:9 does so for complex x); NaN stays NaN
__device__ __forceinline__ double dhqr_alphafactor_p(double x) { return x > 0.0 ? -1.0 : (x < 0.0 ? 1.0 : (x == 0.0 ? -1.0 : x)); }

#define BQP_SQRT2 1.4142135623730951
// an empty statement that claims to modify a scalar register: what is derived from it is formed where it is used
// (BQN_KEEP_IN_LOOP's scalar twin, dhqr_wave.h)
#if defined(__HIP_DEVICE_COMPILE__)
#define BQP_KEEP_SCALAR(x_) asm volatile("" : "+s"(x_))
#else
#define BQP_KEEP_SCALAR(x_) ((void)0)
#endif

// householder!(A_k P_k, alpha_k) for k < batch, in place; jpvt_k = jpvt + k stride_jpvt receives the n 0-based original
// indices of the columns.  m <= 64, n <= NC, m >= n >= 1.
template <int NC, typename T>
__global__ __launch_bounds__(64 * BQW_WAVES, bqw_min_waves<T>(NC)) void k_batched_qrp_wave(T *__restrict__ A, int64_t lda, int64_t strideA, int m,
                                                                                          int n, T *__restrict__ alpha, int64_t stride_alpha,
                                                                                          int32_t *__restrict__ jpvt, int64_t stride_jpvt,
                                                                                          int64_t batch) {
  const int l = bqw_lane();
  const int64_t k = bqw_matrix();
  if (k >= batch) return;  // (the whole wave)
  T *Ak = A + k * strideA;
  T a[NC];
  bqw_load(a, Ak, lda, m, n, l);
  T alv = (T)0;  // lane j keeps alpha_j
  int jp = l;        // lane c keeps jpvt[c]
  int jz = n;        // the first column of the zero tail
#pragma unroll 1
  for (int j = 0; j < n; ++j) {
    // pivot search: the squared norms of rows >= j of the columns j .. n-1, afresh; the first maximum
    // (Float32: n as a value of this step's own -- the NC tests c < n of the load would otherwise be carried through the loop
    // as scalar register pairs and spilled; the Float64 instantiations keep the code they had)
    int nj = n;
    if constexpr (!std::is_same_v<T, double>) BQP_KEEP_SCALAR(nj);
    double bestv = -1.0;
    int p = j;
#pragma unroll
    for (int g = 0; g < NC / 4; ++g) {
      if (4 * g + 3 >= j && 4 * g < nj) {
        double d[4];
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          const double t = l >= j ? (double)a[4 * g + cc] : 0.0;  // (Float32: the stored value widened, its square exact)
          d[cc] = wave_sum_dpp(t * t);
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
    // the chosen column, and the one that makes room for it: select chains inside the columns' own groups of four (a chain
    // over all NC columns keeps NC scalar masks alive)
    T xt = (T)0, xj = (T)0;
#pragma unroll
    for (int g = 0; g < NC / 4; ++g) {
      if (g == (p >> 2)) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) xt = (cc == (p & 3)) ? a[4 * g + cc] : xt;
      }
      if (g == (j >> 2)) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) xj = (cc == (j & 3)) ? a[4 * g + cc] : xj;
      }
    }
    const double x = (double)xt;
    {
      const int pj = __builtin_amdgcn_readlane(jp, j), pp = __builtin_amdgcn_readlane(jp, p);
      jp = l == j ? pp : (l == p ? pj : jp);
    }
    // reflector j (src:129-140): rows >= m hold zeros
    const double s2 = bqw_norm2<T>(l >= j ? x : 0.0);
    const double h = smq_readlane(x, j);
    double sn, f, al;
    dhqr_reflector_scalars(s2, h, dhqr_alphafactor_p, sn, f, al);
    const double piv = (h - al) * f;  // src:132
    const T vt = (T)(l > j ? x * f : (l == j ? piv : 0.0));  // src:133-140 (Float32: rounded once, as k_batched_qr_wave rounds
    const double v = (double)vt;                              // it; the trailing update uses the stored reflector)
    if (l == j) alv = (T)al;
    const T xv = l >= j ? vt : xt;  // rows < j keep R
#pragma unroll
    for (int g = 0; g < NC / 4; ++g) {  // the swap, then the reflector in its place (p == j: the reflector alone)
      if (g == (p >> 2)) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) a[4 * g + cc] = (cc == (p & 3)) ? xj : a[4 * g + cc];
      }
      if (g == (j >> 2)) {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) a[4 * g + cc] = (cc == (j & 3)) ? xv : a[4 * g + cc];
      }
    }
    bqw_trailing_update(a, v, j, nj, l);
  }
  // the zero tail: alpha_c = 0 (alv is 0 in the lanes >= jz), v_c = sqrt(2) e_c for c >= jz
  int ns = n;
  if constexpr (!std::is_same_v<T, double>) BQP_KEEP_SCALAR(ns);
#pragma unroll
  for (int c = 0; c < NC; ++c) a[c] = (c >= jz && c < ns && l >= c) ? (l == c ? (T)BQP_SQRT2 : (T)0) : a[c];
  bqw_store(a, Ak, lda, m, ns, l);
  if (l < n) {
    alpha[k * stride_alpha + l] = alv;
    jpvt[k * stride_jpvt + l] = jp;
  }
}

// The rank-truncated solve for k < batch and every column q < nrhs of B_k: with r = clamp(rank[k], 0, n) the column
// b <- [z; tail] as solve_householder! (k_batched_ldiv_wave's arithmetic) leaves it on the first r columns of the factor,
// and column q of X_k (n) <- the basic solution x[jpvt[i]] = z_i (i < r), exact zeros elsewhere.  r = 0: b stays untouched.
// A column's bits do not depend on nrhs, its place or the batch: the columns are taken one after the other.
template <int NC, typename T>
__global__ __launch_bounds__(64 * BQW_WAVES, bqw_min_waves<T>(NC)) void k_batched_ldivp_wave(
    const T *__restrict__ A, int64_t lda, int64_t strideA, int m, int n, const T *__restrict__ alpha, int64_t stride_alpha,
    const int32_t *__restrict__ jpvt, int64_t stride_jpvt, const int32_t *__restrict__ rank, T *__restrict__ B, int nrhs, int64_t ldb,
    int64_t strideB, T *__restrict__ X, int64_t ldx, int64_t strideX, int64_t batch) {
  int l = bqw_lane();
  const int64_t k = bqw_matrix();
  if (k >= batch) return;  // (the whole wave)
  T a[NC];
  bqw_load(a, A + k * strideA, lda, m, n, l);
  const int rk = __builtin_amdgcn_readfirstlane(rank[k]);
  int r = rk < 0 ? 0 : (rk > n ? n : rk);  // wave-uniform
  double al = l < r ? (double)alpha[k * stride_alpha + l] : 1.0;  // lane j: alpha_j
  const int jp = l < n ? jpvt[k * stride_jpvt + l] : -1;
  double rinv = dhqr_rcp(al);
#pragma unroll 1
  for (int q = 0; q < nrhs; ++q) {
    bqw_keep_in_loop(a);  // (BQN_KEEP_IN_LOOP, dhqr_wave.h)
    BQN_KEEP_IN_LOOP(al);
    BQN_KEEP_IN_LOOP(rinv);
    BQN_KEEP_IN_LOOP(l);
    if constexpr (!std::is_same_v<T, double>) BQP_KEEP_SCALAR(r);  // (Float32: the NC tests c < r formed where they are used)
    T *bk = B + k * strideB + (int64_t)q * ldb;
    bqw_col<T> bb[1];
    bqw_col_set(bb[0], l < m ? (double)bk[l] : 0.0);
    // ---- b <- Q_r'b: reflectors left to right (src:215-224)
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < r) bqw_reflect_group(bqw_reflector(a, c, l), bb, (c & 7) == 7);  // (wave-uniform)
    bqw_col_renorm(bb);
    // ---- back substitution on R11, columns right to left (src:244-254)
#pragma unroll
    for (int c = NC - 1; c >= 0; --c)
      if (c < r) bqw_backsub_group(c, l, a[c], al, rinv, bb);
    const double z = bqw_col_value(bb[0]);
    if (r > 0 && l < m) bk[l] = (T)z;  // (Float32: rounded once)
    // jpvt is a permutation: every entry of the column is written once (an index out of range is not written at all)
    if (l < n && jp >= 0 && jp < n) X[k * strideX + (int64_t)q * ldx + jp] = l < r ? (T)z : (T)0;
  }
}

// rank[k] = the number of leading j with |alpha_j| > rc |alpha_0| (counting stops at the first failure; a NaN fails):
// element-wise, one thread per matrix.  T: the type of an alpha -- double, float (widened: the comparison is in double) or
// double2 (ComplexF64: |alpha| = hypot(re, im))
__device__ __forceinline__ double bqp_abs(double x) { return fabs(x); }
__device__ __forceinline__ double bqp_abs(float x) { return fabs((double)x); }
__device__ __forceinline__ double bqp_abs(double2 x) { return hypot(x.x, x.y); }
template <typename T>
__global__ __launch_bounds__(256) void k_batched_rank(const T *__restrict__ alpha, int64_t n, int64_t stride_alpha, double rc,
                                                      int32_t *__restrict__ rank, int64_t batch) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < batch; k += (int64_t)gridDim.x * blockDim.x) {
    const T *al = alpha + k * stride_alpha;
    const double bound = rc * bqp_abs(al[0]);
    int64_t r = 0;
    while (r < n && bqp_abs(al[r]) > bound) ++r;
    rank[k] = (int32_t)r;
  }
}

// ---- the general tier ----------------------------------------------------------------------------------------------------
#define BQPG_THREADS 256
// Workgroup k factors matrix k (any m >= n >= 1) in place in device memory.  Per step: the norms of the trailing columns,
// column c to wave (c - j) % NW, each wave keeping its first maximum | the waves' candidates meet in LDS (largest norm,
// then smallest column) | the swap, rows spread over the threads | the reflector by the whole workgroup, its norm in
// double-double (dd_block_sum) | the trailing columns, column c to wave (c - j - 1) % NW.  All control flow around the
// barriers depends on j, n and values every thread reads from LDS alike.
__global__ __launch_bounds__(BQPG_THREADS) void k_batched_qrp_general(double *__restrict__ A, int64_t lda, int64_t strideA, int64_t m, int64_t n,
                                                                       double *__restrict__ alpha, int64_t stride_alpha,
                                                                       int32_t *__restrict__ jpvt, int64_t stride_jpvt) {
  constexpr int NW = BQPG_THREADS / 64;
  __shared__ double red[2 * NW];
  __shared__ double candv[NW];
  __shared__ int64_t candc[NW];
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  double *Ak = A + (int64_t)blockIdx.x * strideA;
  double *alk = alpha + (int64_t)blockIdx.x * stride_alpha;
  int32_t *jk = jpvt + (int64_t)blockIdx.x * stride_jpvt;  // (thread 0 alone reads and writes it)
  if (t == 0)
    for (int64_t c = 0; c < n; ++c) jk[c] = (int32_t)c;
  for (int64_t j = 0; j < n; ++j) {
    double bestv = -1.0;
    int64_t p = j;
    for (int64_t c = j + w; c < n; c += NW) {
      const double *col = Ak + c * lda;
      double s = 0.0;
      for (int64_t i = j + l; i < m; i += 64) s = fma(col[i], col[i], s);
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
        for (int64_t i = c + t; i < m; i += BQPG_THREADS) Ak[i + c * lda] = i == c ? BQP_SQRT2 : 0.0;
        if (t == 0) alk[c] = 0.0;
      }
      break;
    }
    if (p != j) {
      for (int64_t i = t; i < m; i += BQPG_THREADS) {
        const double u = Ak[i + j * lda];
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
    double *vj = Ak + j * lda;
    dhqr_dd acc = {0.0, 0.0};
    for (int64_t i = j + t; i < m; i += BQPG_THREADS) dd_add_sq(acc, vj[i]);
    const double s2 = dd_block_sum<BQPG_THREADS>(acc, red);
    const double h = vj[j];
    double sn, f, al;
    dhqr_reflector_scalars(s2, h, dhqr_alphafactor_p, sn, f, al);
    const double piv = (h - al) * f;  // src:132
    __syncthreads();  // every thread has read h
    for (int64_t i = j + t; i < m; i += BQPG_THREADS) vj[i] = i == j ? piv : vj[i] * f;  // src:133-140
    if (t == 0) alk[j] = al;
    __syncthreads();  // the reflector is in memory
    for (int64_t c = j + 1 + w; c < n; c += NW) {  // src:198-213
      double *col = Ak + c * lda;
      double s = 0.0;
      for (int64_t i = j + l; i < m; i += 64) s = fma(vj[i], col[i], s);
      s = wave_sum_dpp(s);
      for (int64_t i = j + l; i < m; i += 64) col[i] = fma(-vj[i], s, col[i]);
    }
    __syncthreads();  // the trailing matrix is in memory for the next step's norms
  }
}

// Workgroup w of a 1-D grid of batch * nrhs solves column q = w % nrhs of matrix k = w / nrhs with r = clamp(rank[k], 0, n):
// Q_r'b as k_batched_zapplyq_general applies it (thread t owns the rows t, t + BQPG_THREADS, ...), the back substitution on
// R11 with two barriers per column (x_c formed by every thread | b_c overwritten by its owner), the scatter through jpvt.
__global__ __launch_bounds__(BQPG_THREADS) void k_batched_ldivp_general(const double *__restrict__ A, int64_t lda, int64_t strideA, int64_t m,
                                                                         int64_t n, const double *__restrict__ alpha, int64_t stride_alpha,
                                                                         const int32_t *__restrict__ jpvt, int64_t stride_jpvt,
                                                                         const int32_t *__restrict__ rank, double *__restrict__ B, int64_t nrhs,
                                                                         int64_t ldb, int64_t strideB, double *__restrict__ X, int64_t ldx,
                                                                         int64_t strideX) {
  constexpr int NW = BQPG_THREADS / 64;
  __shared__ double red[NW];
  const int t = threadIdx.x;
  const int64_t k = (int64_t)blockIdx.x / nrhs, q = (int64_t)blockIdx.x - k * nrhs;
  const double *Ak = A + k * strideA, *alk = alpha + k * stride_alpha;
  const int32_t *jk = jpvt + k * stride_jpvt;
  double *bcol = B + k * strideB + q * ldb, *xcol = X + k * strideX + q * ldx;
  const int64_t rk = rank[k];
  const int64_t r = rk < 0 ? 0 : (rk > n ? n : rk);  // (the same in every thread)
  for (int64_t c = 0; c < r; ++c) {
    const double *vc = Ak + c * lda;  // rows < c of a factored column hold R
    double s = 0.0;
    for (int64_t i = t; i < m; i += BQPG_THREADS)
      if (i >= c) s = fma(vc[i], bcol[i], s);  // src:217
    s = wave_sum_dpp(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) tot += red[i];
    __syncthreads();
    for (int64_t i = t; i < m; i += BQPG_THREADS)
      if (i >= c) bcol[i] = fma(-vc[i], tot, bcol[i]);  // src:218-220
  }
  for (int64_t cc = 0; cc < r; ++cc) {  // src:244-254
    const int64_t c = r - 1 - cc;
    __syncthreads();  // b_c has all its updates
    const double xc = bcol[c] / alk[c];
    __syncthreads();  // every thread has read b_c
    for (int64_t i = t; i <= c; i += BQPG_THREADS) bcol[i] = i == c ? xc : fma(-Ak[i + c * lda], xc, bcol[i]);
  }
  __syncthreads();
  for (int64_t i = t; i < n; i += BQPG_THREADS) {
    const int64_t pi = jk[i];
    if (pi >= 0 && pi < n) xcol[pi] = i < r ? bcol[i] : 0.0;
  }
}
