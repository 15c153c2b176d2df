// dhqr_wave.h -- the steps of the wave-per-matrix kernels for Float64 and Float32, each written ONCE: dhqr_batched.h (qr!
// and `\`) and dhqr_batched_pivoted.h (column pivoting) are these pieces in the order of their algorithms.  The pivoted solve
// has the bytes of the solve with n = rank because both call the SAME step.  (The kernels that walk groups of columns past
// the factor -- dhqr_batched_nrhs.h, dhqr_batched_applyq.h -- are the written-out form of these steps, for the reasons given
// there: the compiler does not make the same code of a step and of its written-out form.)
//
// Geometry.  The single-workgroup kernels of dhqr_small.h give a whole compute unit to one matrix; their smallest
// instantiation occupies 576 threads for a 16 x 8 matrix that fills 1/128 of its registers.  A batch of matrices of at most
// 64 rows and 32 columns (local fits, per-pixel regressions) runs here with ONE WAVE per matrix and BQW_WAVES matrices per
// workgroup:
//
//   lane l holds row l of every column (a[c], c < NC; NC = 8, 16 or 32, the smallest that holds n), so a column is one
//   coalesced access, a dot product v_j' a_c (partialdot, src:42-49) is one multiplication and a DPP wave reduction, the
//   update (hotloop!, src:156-160) one fma.  Nothing is shared between the waves of a workgroup: no LDS, no barrier, no
//   flag and no wait of any kind; a wave without a matrix leaves at once.
//
// A register array indexed by a runtime column goes to scratch memory, so every loop over the columns of the factor is
// unrolled over the compile-time index, and a runtime column leaves and enters the array through a chain of selects.
//
// Arithmetic: the reference's, column by column (src:122-148, 198-213, 284-294), with the pieces of dhqr_small.h.
//   Float64  the matrix in double.  The reflector's norm in double-double (dd_add_sq + wave_sum_dd_plain); alpha, f and the
//            pivot as k_small_qr_d's builder forms them (dhqr_reflector_scalars).  A column of B is CARRIED in double-double
//            (dhqr_dd) through Q'b and the back substitution and rounded once per entry, for the reason written at
//            k_small_ldiv; the low part is folded into the high one (dd_renorm) after every eighth reflector and at the end.
//   Float32  the matrix STORED in float (NC registers, half of Float64's), every SUM taken in double.  The product of two
//            floats is exact in double, so the column norm and each v_j' a_c lose nothing before the DPP tree, whose six
//            double additions sit 29 bits below the stored precision -- no double-double is needed.  alpha, f and the pivot
//            are formed in double by the same expressions; every stored entry is rounded to float ONCE per column step.  A
//            column of B is carried in plain double and rounded once at the end.
// The carrier of a column of B -- dhqr_dd or double -- selects the Float64 or the Float32 step by overload.
#pragma once
#include <type_traits>
#include "dhqr_small.h"

#define BQW_WAVES 4  // matrices per workgroup (256 threads)
#define BQW_MAX_M 64
#define BQW_MAX_N 32
// waves per SIMD the register allocation must leave room for.  Float64: the matrix takes 2 NC registers of a lane's 512 /
// waves; Float32: from the measured counts (profiles/batched_kernel_resources.txt)
#define BQW_MIN_WAVES(NC_) ((NC_) <= 8 ? 8 : ((NC_) <= 16 ? 6 : 4))
#define BQS_MIN_WAVES(NC_) ((NC_) <= 16 ? 8 : 6)
template <typename T>
constexpr int bqw_min_waves(int NC) {
  return std::is_same_v<T, double> ? BQW_MIN_WAVES(NC) : BQS_MIN_WAVES(NC);
}

// Columns of B per group in the kernels that walk groups of columns past the resident factor.
#define BQN_RG 4
// The solve (dhqr_batched_nrhs.h).  Float64, NC = 16 and 32: three.  A group of four double-double chains beside 2 NC
// registers of matrix does not fit under the launch bound there (NC = 16: 2 registers spilled at 80; NC = 32: the matrix
// itself in scratch memory, 272 bytes), a group of three does without scratch (profiles/batched_kernel_resources.txt).
template <typename T>
constexpr int bqn_rg(int NC) {
  return std::is_same_v<T, double> && NC > 8 ? 3 : BQN_RG;
}
// Q application (dhqr_batched_applyq.h).  Without alpha and 1 / alpha beside the matrix, Float64 NC = 16 holds four chains
// under the launch bound where the solve holds three; NC = 32 stays at three.
template <typename T>
constexpr int bqa_rg(int NC) {
  return std::is_same_v<T, double> && NC > 16 ? 3 : BQN_RG;
}
// The factor, alpha and 1 / alpha do not change from group to group, so the compiler would move everything derived from them
// and from the lane number -- the masked reflectors v_c, the negated and widened R columns, 4 NC scalar registers of broadcast
// alphas, 6 NC of lane masks -- in front of the group loop: a second and third copy of the matrix in registers, and scratch
// memory.  An empty statement that claims to modify the register keeps each derivation inside the loop body, where it lives
// for one reflector.  (No instruction.  What the compiler does with it depends on its version: after a ROCm upgrade re-read
// the kernels' scratch sizes, profiles/batched_kernel_resources.txt says how; they must stay 0.)
#if defined(__HIP_DEVICE_COMPILE__)
#define BQN_KEEP_IN_LOOP(x_) asm volatile("" : "+v"(x_))
#else
#define BQN_KEEP_IN_LOOP(x_) ((void)0)
#endif
template <int NC, typename T>
__device__ __forceinline__ void bqw_keep_in_loop(T (&a)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) BQN_KEEP_IN_LOOP(a[c]);
}

// ---- the wave and its matrix ---------------------------------------------------------------------------------------------
// the lane (its row of the matrix) and the matrix of its wave; a wave with bqw_matrix() >= batch has none and leaves at once
__device__ __forceinline__ int bqw_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ int64_t bqw_matrix() { return (int64_t)blockIdx.x * BQW_WAVES + (threadIdx.x >> 6); }

// a <- rows and columns of the m x n matrix at Ak, zeros beyond them
template <int NC, typename T>
__device__ __forceinline__ void bqw_load(T (&a)[NC], const T *Ak, int64_t lda, int m, int n, int l) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool in = c < n && l < m;  // (no branch: every load of the matrix is in flight before the first use)
    const T t = Ak[in ? (int64_t)l + (int64_t)c * lda : 0];
    a[c] = in ? t : (T)0;
  }
}
template <int NC, typename T>
__device__ __forceinline__ void bqw_store(const T (&a)[NC], T *Ak, int64_t lda, int m, int n, int l) {
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c < n && l < m) Ak[(int64_t)l + (int64_t)c * lda] = a[c];
}
// column j (runtime) out of / into the register array
template <int NC, typename T>
__device__ __forceinline__ T bqw_take(const T (&a)[NC], int j) {
  T x = (T)0;
#pragma unroll
  for (int c = 0; c < NC; ++c) x = (c == j) ? a[c] : x;
  return x;
}
template <int NC, typename T>
__device__ __forceinline__ void bqw_put(T (&a)[NC], int j, T x) {
#pragma unroll
  for (int c = 0; c < NC; ++c) a[c] = (c == j) ? x : a[c];
}

// ---- the factorisation's steps -------------------------------------------------------------------------------------------
// sum over the lanes of xs^2 (src:129).  Float64: in double-double; Float32: xs^2 is exact in double
template <typename T>
__device__ __forceinline__ double bqw_norm2(double xs) {
  if constexpr (std::is_same_v<T, double>) {
    dhqr_dd acc = {0.0, 0.0};
    dd_add_sq(acc, xs);
    const dhqr_dd ss = wave_sum_dd_plain(acc);
    return ss.hi + ss.lo;
  } else {
    return wave_sum_dpp(xs * xs);
  }
}
// trailing update with reflector j in v (src:198-213): unrolled groups of four columns under one uniform branch per group
// (finished groups are skipped; inside a group the four reductions are independent and interleave).  Columns >= n hold zeros
// and stay zeros.  Float32: exact products, the entry rounded once.
template <int NC, typename T>
__device__ __forceinline__ void bqw_trailing_update(T (&a)[NC], double v, int j, int n, int l) {
  static_assert(NC % 4 == 0 && NC <= BQW_MAX_N, "columns in groups of four");
#pragma unroll
  for (int g = 0; g < NC / 4; ++g) {
    if (4 * g + 3 > j && 4 * g < n) {
      double d[4];
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) d[cc] = wave_sum_dpp(v * (double)a[4 * g + cc]);  // src:42-49
#pragma unroll
      for (int cc = 0; cc < 4; ++cc)  // src:156-160, src:209: rows >= j of the columns behind j, nothing else (a reflector of a
        a[4 * g + cc] =               // zero column is NaN: 0 * NaN)
            (4 * g + cc > j && l >= j) ? (T)fma(-v, d[cc], (double)a[4 * g + cc]) : a[4 * g + cc];
    }
  }
}

// ---- a column of B between load and store: dhqr_dd (Float64) or double (Float32) -------------------------------------------
template <typename T>
using bqw_col = std::conditional_t<std::is_same_v<T, double>, dhqr_dd, double>;
__device__ __forceinline__ void bqw_col_set(dhqr_dd &b, double x) {
  b.hi = x;
  b.lo = 0.0;
}
__device__ __forceinline__ void bqw_col_set(double &b, double x) { b = x; }
__device__ __forceinline__ double bqw_col_value(const dhqr_dd &b) { return b.hi + b.lo; }
__device__ __forceinline__ double bqw_col_value(double b) { return b; }  // (the caller rounds it to float: once)
template <int RG>
__device__ __forceinline__ void bqw_col_renorm(dhqr_dd (&bb)[RG]) {
#pragma unroll
  for (int q = 0; q < RG; ++q) dd_renorm(bb[q]);
}
template <int RG>
__device__ __forceinline__ void bqw_col_renorm(double (&)[RG]) {}

// reflector c of a factored column: rows < c hold R
template <int NC, typename T>
__device__ __forceinline__ double bqw_reflector(const T (&a)[NC], int c, int l) {
  return l >= c ? (double)a[c] : 0.0;
}
// b <- (I - v v') b for the RG columns of a group (src:215-220): their chains -- each a serial DPP reduction -- are
// independent and interleave, the way the four column dots of a trailing-update group do.
// Float64; renorm: fold the low part into the high one afterwards (it stays small against the high one)
template <int RG>
__device__ __forceinline__ void bqw_reflect_group(double v, dhqr_dd (&bb)[RG], bool renorm) {
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
    if (renorm) dd_renorm(bb[q]);
  }
}
// Float32 (nothing to renormalise)
template <int RG>
__device__ __forceinline__ void bqw_reflect_group(double v, double (&bb)[RG], bool /*renorm*/) {
  double s[RG];
#pragma unroll
  for (int q = 0; q < RG; ++q) s[q] = wave_sum_dpp(v * bb[q]);  // src:217
#pragma unroll
  for (int q = 0; q < RG; ++q) bb[q] = fma(-s[q], v, bb[q]);  // src:218-220
}

// Column c of the back substitution (src:244-254) for the RG columns of a group: x_c = b_c / alpha_c, b[0:c] -= R[0:c, c] x_c.
// ac: this lane's entry of column c of the factor; al, rinv: lane j holds alpha_j and 1 / alpha_j.  b_c / alpha_c as
// k_small_ldiv forms it: reciprocal (off the chain) times b_c and one correction step.
__device__ __forceinline__ double bqw_quotient(double bq, double aj, double ri) {
  const double xj = bq * ri;
  return fma(fma(-aj, xj, bq), ri, xj);
}
template <int RG>
__device__ __forceinline__ void bqw_backsub_group(int c, int l, double ac, double al, double rinv, dhqr_dd (&bb)[RG]) {
  const double aj = smq_readlane(al, c), ri = smq_readlane(rinv, c);
#pragma unroll
  for (int q = 0; q < RG; ++q) {
    const double xj = bqw_quotient(smq_readlane(bb[q].hi + bb[q].lo, c), aj, ri);
    if (l == c) {
      bb[q].hi = xj;
      bb[q].lo = 0.0;
    } else if (l < c) {
      dd_add_prod(bb[q], -ac, xj);  // src:248-250
    }
  }
}
template <int RG>
__device__ __forceinline__ void bqw_backsub_group(int c, int l, float ac, double al, double rinv, double (&bb)[RG]) {
  const double aj = smq_readlane(al, c), ri = smq_readlane(rinv, c);
#pragma unroll
  for (int q = 0; q < RG; ++q) {
    const double xj = bqw_quotient(smq_readlane(bb[q], c), aj, ri);
    if (l == c)
      bb[q] = xj;
    else if (l < c)
      bb[q] = fma(-(double)ac, xj, bb[q]);  // src:248-250
  }
}
