// dhqr_batched_complex_nrhs.h -- H_k \ B_k with SEVERAL right-hand sides, B_k <- Q_k^H B_k, B_k <- Q_k B_k and the explicit
// thin Q_k for a BATCH of tiny ComplexF64 factors: one WAVE per matrix; and the plain kernel that applies Q beyond that tier.
//
// k_batched_zldiv_wave_nrhs / k_batched_zapplyq_wave are to k_batched_zldiv_wave (dhqr_batched_complex.h) what
// k_batched_ldiv_wave_nrhs / k_batched_applyq_wave (dhqr_batched_nrhs.h, dhqr_batched_applyq.h) are to k_batched_ldiv_wave:
// same shapes (m <= 64, n <= NC = 8, 16 or 32), same launch geometry (BQW_WAVES matrices per workgroup, lane l on row l),
// the launch bounds of the single-column complex kernels, no LDS, no barrier, no flag and no wait of any kind, a wave
// without a matrix leaves at once.  The factor (bqz_load), alpha and nothing else are loaded ONCE into registers, and the
// columns of B_k walk past them: a runtime loop over groups of RG columns (BQZN_RG, BQZA_RG), the body unrolled over the
// group, the group's chains -- each two serial DPP reductions per reflector -- side by side.
//
// Column r of matrix k lives at B + k strideB + r ldb (complex elements) and is read and written in place, one coalesced
// 16-byte-per-lane access per column.  A tail group of 1 .. RG-1 columns loads zeros for the missing columns and stores
// nothing for them.
//
// Arithmetic: per column, the expressions of k_batched_zldiv_wave in the same order -- both parts of b in double-double
// (dd_add_prod, wave_sum_dd_plain), dd_renorm after every eighth reflector and once at the end, Smith's division (zdiv) in
// the back substitution.  So column r of the solve is BIT-IDENTICAL to what the single-column kernel returns for that column
// alone: it depends neither on nrhs nor on the column's place in its group nor on the batch.
//
//   TRANS = 1   B <- Q^H B: reflectors c = 0 .. n-1, renormalised after c = 7, 15, 23: rows n .. m-1 have the BITS of what
//               the solve leaves there (the tail of Q^H B, which back substitution never touches).
//   TRANS = 0   B <- Q B: reflectors c = n-1 .. 0, renormalised after c = 24, 16, 8 (and 0) -- by the reflector's INDEX, as
//               in the real kernel.  A reflector I - v v^H is Hermitian: both directions use the same expressions.
//   FORMQ       TRANS = 0 on columns e_r generated in registers: nothing of Q is read, all m x n is written.  The
//               reflectors c > r act as the identity on e_r (the dot product is an exact zero), so a group skips the
//               reflectors behind its last column under one wave-uniform branch.  For a finite factor the result compares
//               equal to TRANS = 0 applied to [I; 0].
//
// k_batched_zapplyq_general: any m and n, one workgroup per (matrix, column of B), in place in global memory -- the tier of
// apply-Q and explicit Q beyond 64 x 32 and with the small route off.  It re-reads the factor once per column of B.
// Registers (profiles/batched_c64_kernel_resources.txt): no instantiation has scratch memory or a spilled register.
#pragma once
#include "dhqr_batched_applyq.h"
#include "dhqr_batched_complex.h"

// Columns per group: the largest RG <= 4 for which the gfx950 code object has neither scratch memory nor a spilled register
// under the launch bound of the single-column kernel (profiles/batched_c64_kernel_resources.txt).  A complex double-double
// chain is 8 registers of b and 8 of partial sums beside the 4 NC of the matrix.
// Solve (BQZ_MIN_WAVES_LDIV): NC = 8 spills 8 registers with two chains, NC = 16 8 with three; NC = 32 holds four.
// Apply-Q and explicit Q (BQZ_MIN_WAVES): NC = 8 spills 22 - 30 with two chains, NC = 16 22 - 30 with four; NC = 32 holds four.
#define BQZN_RG(NC_) ((NC_) <= 8 ? 1 : ((NC_) <= 16 ? 2 : 4))
#define BQZA_RG(NC_) ((NC_) <= 8 ? 1 : ((NC_) <= 16 ? 3 : 4))

// conj(v) . b per lane, b = (br, bi) each hi + lo: the expressions of k_batched_zldiv_wave (src:217)
__device__ __forceinline__ void bqz_cdot_dd(const double2 v, const dhqr_dd &br, const dhqr_dd &bi, dhqr_dd &sr, dhqr_dd &si) {
  sr.hi = 0.0;
  sr.lo = 0.0;
  si.hi = 0.0;
  si.lo = 0.0;
  dd_add_prod(sr, v.x, br.hi);
  dd_add_prod(sr, v.y, bi.hi);
  dd_add_prod(si, v.x, bi.hi);
  dd_add_prod(si, -v.y, br.hi);
  sr.lo += v.x * br.lo + v.y * bi.lo;
  si.lo += v.x * bi.lo - v.y * br.lo;
}
// b -= v s (src:218-220)
__device__ __forceinline__ void bqz_submul_dd(dhqr_dd &br, dhqr_dd &bi, const double2 v, const double s_r, const double s_i) {
  dd_add_prod(br, -s_r, v.x);
  dd_add_prod(br, s_i, v.y);
  dd_add_prod(bi, -s_i, v.x);
  dd_add_prod(bi, -s_r, v.y);
}
// one reflector on the RG chains of a group: the dots, their wave sums side by side, the updates
template <int RG>
__device__ __forceinline__ void bqz_reflect_group(const double2 v, dhqr_dd (&br)[RG], dhqr_dd (&bi)[RG], bool renorm) {
  dhqr_dd sr[RG], si[RG], tr[RG], ti[RG];
#pragma unroll
  for (int q = 0; q < RG; ++q) bqz_cdot_dd(v, br[q], bi[q], sr[q], si[q]);
#pragma unroll
  for (int q = 0; q < RG; ++q) {
    tr[q] = wave_sum_dd_plain(sr[q]);
    ti[q] = wave_sum_dd_plain(si[q]);
  }
#pragma unroll
  for (int q = 0; q < RG; ++q) {
    const double s_r = tr[q].hi + tr[q].lo, s_i = ti[q].hi + ti[q].lo;
    bqz_submul_dd(br[q], bi[q], v, s_r, s_i);
    if (renorm) {  // (compile-time per reflector) the low parts stay small against the high ones
      dd_renorm(br[q]);
      dd_renorm(bi[q]);
    }
  }
}
// (the scalar twin of BQN_KEEP_IN_LOOP: bqz_load forms the NC uniform tests c < n as scalar register pairs; a loop that tests
// c < n again would carry all of them from the load to its last reflector -- 2 NC scalar registers, spilled at NC = 32)
#if defined(__HIP_DEVICE_COMPILE__)
#define BQZ_KEEP_SCALAR_IN_LOOP(x_) asm volatile("" : "+s"(x_))
#else
#define BQZ_KEEP_SCALAR_IN_LOOP(x_) ((void)0)
#endif
template <int NC>
__device__ __forceinline__ void bqz_keep_in_loop(double2 (&a)[NC], int &l) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    BQN_KEEP_IN_LOOP(a[c].x);
    BQN_KEEP_IN_LOOP(a[c].y);
  }
  BQN_KEEP_IN_LOOP(l);  // (the lane masks l >= c, l == c, l < c)
}

// solve_householder!(B_k[:, r], H_k, alpha_k) (src:284-294) for r < nrhs, k < batch: B_k = B + k strideB (m x nrhs, ldb)
// <- [X_k; tail of Q^H B_k].  lda, ldb and the strides count complex elements.
template <int NC, int RG = BQZN_RG(NC)>
__global__ __launch_bounds__(64 * BQW_WAVES, BQZ_MIN_WAVES_LDIV(NC)) void k_batched_zldiv_wave_nrhs(
    const double2 *__restrict__ A, int64_t lda, int64_t strideA, int m, int n, const double2 *__restrict__ alpha, int64_t stride_alpha,
    double2 *__restrict__ B, int nrhs, int64_t ldb, int64_t strideB, int64_t batch) {
  int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (a scalar)
  if (k >= batch) return;  // (the whole wave)
  const double2 *Ak = A + k * strideA;
  double2 *Bk = B + k * strideB;
  double2 a[NC];
  bqz_load<NC>(a, Ak, lda, m, n, l);
  const double2 alt = alpha[k * stride_alpha + (l < n ? l : 0)];
  double2 al = zmake(l < n ? alt.x : 1.0, l < n ? alt.y : 0.0);  // lane j: alpha_j
#pragma unroll 1
  for (int r0 = 0; r0 < nrhs; r0 += RG) {
    bqz_keep_in_loop<NC>(a, l);
    BQZ_KEEP_SCALAR_IN_LOOP(n);
    BQN_KEEP_IN_LOOP(al.x);
    BQN_KEEP_IN_LOOP(al.y);
    dhqr_dd br[RG], bi[RG];  // b = (br, bi), each hi + lo
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      const bool in = r0 + q < nrhs && l < m;  // (no branch; B_k[0] exists: m, nrhs >= 1)
      const double2 t = Bk[in ? (int64_t)l + (int64_t)(r0 + q) * ldb : 0];
      br[q].hi = in ? t.x : 0.0;
      br[q].lo = 0.0;
      bi[q].hi = in ? t.y : 0.0;
      bi[q].lo = 0.0;
    }
    // ---- B <- Q^H B: reflectors left to right (src:215-224, k_zqtb_col_dd), the group's chains side by side
    zstatic_for(
        [&](auto cc) {
          constexpr int c = decltype(cc)::value;
          if (c < n) {  // (wave-uniform)
            const double2 v = zmake(l >= c ? a[c].x : 0.0, l >= c ? a[c].y : 0.0);  // rows < c of a factored column hold R
            bqz_reflect_group<RG>(v, br, bi, (c & 7) == 7);
          }
        },
        std::make_integer_sequence<int, NC>{});
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      dd_renorm(br[q]);
      dd_renorm(bi[q]);
    }
    // ---- back substitution, columns right to left (src:244-254, k_zbacksub_diag_dd): x_j = b_j / alpha_j, b[0:j] -= R[0:j, j] x_j
    BQN_KEEP_IN_LOOP(l);  // (its masks l == c, l < c are formed here, not carried as the l >= c of the phase above: 2 NC scalars)
    BQZ_KEEP_SCALAR_IN_LOOP(n);
    zstatic_for(
        [&](auto cc) {
          constexpr int c = NC - 1 - decltype(cc)::value;
          if (c < n) {
            const double2 aj = bqz_readlane(al, c);
#pragma unroll
            for (int q = 0; q < RG; ++q) {
              const double2 xj = zdiv(bqz_readlane(zmake(br[q].hi + br[q].lo, bi[q].hi + bi[q].lo), c), aj);  // src:251
              if (l == c) {
                br[q].hi = xj.x;
                br[q].lo = 0.0;
                bi[q].hi = xj.y;
                bi[q].lo = 0.0;
              } else if (l < c) {  // src:248-250: b_l -= R_lc x_c
                const double2 r = a[c];
                dd_add_prod(br[q], -r.x, xj.x);
                dd_add_prod(br[q], r.y, xj.y);
                dd_add_prod(bi[q], -r.x, xj.y);
                dd_add_prod(bi[q], -r.y, xj.x);
              }
            }
          }
        },
        std::make_integer_sequence<int, NC>{});
#pragma unroll
    for (int q = 0; q < RG; ++q)
      if (r0 + q < nrhs && l < m) Bk[(int64_t)l + (int64_t)(r0 + q) * ldb] = zmake(br[q].hi + br[q].lo, bi[q].hi + bi[q].lo);
  }
}

// B_k <- Q_k^H B_k (TRANS) | Q_k B_k | Q_k [I; 0] (FORMQ: nrhs = n, B is the m x n Q_k) for k < batch
// Launch bound: that of the single-column factor kernel, BQZ_MIN_WAVES.  One exception: FORMQ at NC = 8 carries the lane
// number, which it needs for e_r and for the stores, past every reflector, and came to 64 registers + 2 spilled (12 bytes
// of scratch) under the bound of 8; it takes the solve's bound there, BQZ_MIN_WAVES_LDIV (6 at NC = 8, the same elsewhere).
template <int NC, int TRANS, int FORMQ = 0, int RG = BQZA_RG(NC)>
__global__ __launch_bounds__(64 * BQW_WAVES, FORMQ ? BQZ_MIN_WAVES_LDIV(NC) : BQZ_MIN_WAVES(NC)) void k_batched_zapplyq_wave(
    const double2 *__restrict__ A, int64_t lda, int64_t strideA, int m, int n, double2 *__restrict__ B, int nrhs, int64_t ldb,
    int64_t strideB, int64_t batch) {
  static_assert(!FORMQ || !TRANS, "the explicit Q is Q [I; 0]");
  int l = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * BQW_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (a scalar)
  if (k >= batch) return;  // (the whole wave)
  const double2 *Ak = A + k * strideA;
  double2 *Bk = B + k * strideB;
  double2 a[NC];
  bqz_load<NC>(a, Ak, lda, m, n, l);
  // Q is made of the reflectors alone: R, in the rows < c of column c, goes once, here, and no reflector needs a lane mask
#pragma unroll
  for (int c = 0; c < NC; ++c) a[c] = zmake(l >= c ? a[c].x : 0.0, l >= c ? a[c].y : 0.0);
#pragma unroll 1
  for (int r0 = 0; r0 < nrhs; r0 += RG) {
    bqz_keep_in_loop<NC>(a, l);
    BQZ_KEEP_SCALAR_IN_LOOP(n);
    dhqr_dd br[RG], bi[RG];
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      if (FORMQ) {
        br[q].hi = l == r0 + q ? 1.0 : 0.0;  // e_r (r >= nrhs = n: never stored)
        bi[q].hi = 0.0;
      } else {
        const bool in = r0 + q < nrhs && l < m;  // (no branch; B_k[0] exists: m, nrhs >= 1)
        const double2 t = Bk[in ? (int64_t)l + (int64_t)(r0 + q) * ldb : 0];
        br[q].hi = in ? t.x : 0.0;
        bi[q].hi = in ? t.y : 0.0;
      }
      br[q].lo = 0.0;
      bi[q].lo = 0.0;
    }
    zstatic_for(
        [&](auto cc) {
          constexpr int c = TRANS ? decltype(cc)::value : NC - 1 - decltype(cc)::value;
          if (c < n && (!FORMQ || c < r0 + RG))  // (wave-uniform)
            bqz_reflect_group<RG>(a[c], br, bi, TRANS ? (c & 7) == 7 : (c & 7) == 0);
        },
        std::make_integer_sequence<int, NC>{});
#pragma unroll
    for (int q = 0; q < RG; ++q) {
      dd_renorm(br[q]);
      dd_renorm(bi[q]);
    }
#pragma unroll
    for (int q = 0; q < RG; ++q)
      if (r0 + q < nrhs && l < m) Bk[(int64_t)l + (int64_t)(r0 + q) * ldb] = zmake(br[q].hi + br[q].lo, bi[q].hi + bi[q].lo);
  }
}

// The general tier: column r of B_k <- Q_k^H (TRANS) or Q_k times it, for any m >= n >= 1, in place in global memory.
// Workgroup w of a 1-D grid of batch * nrhs takes matrix k = w / nrhs and column r = w % nrhs.  Thread t owns the rows t,
// t + BQZG_THREADS, ... of the column from the first reflector to the last, so no row passes from thread to thread and the
// only exchange is the conj-dot: per reflector each thread sums its rows in row order (plain double, fma), a wave sums its
// lanes (wave_sum_dpp), the waves' sums meet in LDS and every thread adds them in wave order -- a fixed order, no atomics.
// Two barriers per reflector (the partial sums written | read before the next reflector overwrites them), both in uniform
// control flow: c, m and n are the same for the whole workgroup.
#define BQZG_THREADS 256
template <int TRANS>
__global__ __launch_bounds__(BQZG_THREADS) void k_batched_zapplyq_general(const double2 *__restrict__ A, int64_t lda, int64_t strideA,
                                                                           int64_t m, int64_t n, double2 *__restrict__ B, int64_t nrhs,
                                                                           int64_t ldb, int64_t strideB) {
  constexpr int NW = BQZG_THREADS / 64;
  __shared__ double red[2 * NW];
  const int t = threadIdx.x;
  const int64_t k = (int64_t)blockIdx.x / nrhs, r = (int64_t)blockIdx.x - k * nrhs;
  const double2 *Ak = A + k * strideA;
  double2 *bcol = B + k * strideB + r * ldb;
  for (int64_t cc = 0; cc < n; ++cc) {
    const int64_t c = TRANS ? cc : n - 1 - cc;
    const double2 *vc = Ak + c * lda;  // rows < c of a factored column hold R
    double sr = 0.0, si = 0.0;
    for (int64_t i = t; i < m; i += BQZG_THREADS)
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
    for (int w = 0; w < NW; ++w) {
      s_r += red[2 * w];
      s_i += red[2 * w + 1];
    }
    __syncthreads();
    for (int64_t i = t; i < m; i += BQZG_THREADS)
      if (i >= c) bcol[i] = zsubmul(bcol[i], vc[i], s_r, s_i);  // src:218-220: b_i -= v_i s
  }
}
