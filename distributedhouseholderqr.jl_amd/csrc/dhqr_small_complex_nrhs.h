// dhqr_small_complex_nrhs.h -- H_k \ B_k with SEVERAL right-hand sides, B_k <- Q_k^H B_k, B_k <- Q_k B_k and the explicit thin
// Q_k for SMALL ComplexF64 factors beyond the wave tier (1 <= n <= m <= 128): ONE launch, one workgroup per (matrix, group
// of SMZA_CW columns of B).
//
// k_small_zapply<MODE> is the multi-column sibling of k_small_zldiv (dhqr_small_complex.h).  512 threads = 8 waves:
//   waves 0 .. CW-1   CONSUMERS.  Wave w owns column CW g + w of B_k in registers, in the layout of wave 0 of k_small_zldiv:
//                     rows l and l + 64, both parts in double-double (8 doubles), and walks the reflectors past it.
//   waves CW .. 7     PRODUCERS.  They stream the factor in 8-column chunks (16 KB) into the double-buffered LDS stage
//                     buf[2][SMZL_CH][SMZ_MAX] (32 KB, plus the alphas of a chunk) one chunk ahead of the consumers.
// So a workgroup reads the factor ONCE for CW columns, where the column loop over k_small_zldiv reads it once per column
// and the general kernel (k_batched_zapplyq_general) once per column from global memory with two barriers per reflector.
// A 1-D grid of batch * groups, groups = ceil(nrhs / CW): workgroup b takes matrix b / groups and group b % groups.
//
// BARRIER FORM ONLY: the kernel waits on nothing but __syncthreads() -- no flag, no poll, no bounded wait.  One barrier per
// chunk; the chunk sequence depends on m, n, nrhs and the group alone, so it is the same for every wave of the workgroup
// and every wave executes the same number of barriers.  A consumer wave whose column is >= nrhs (the tail of the last
// group) does no arithmetic and no store, but reaches every barrier.
//
// Arithmetic, per column: the expressions of k_small_zldiv in the same order (the dot product of two rows per lane in
// double-double, wave_sum_dd_plain, the update by dd_add_prod, Smith's division zdiv), so a column's bits depend neither on
// nrhs nor on its place in a group nor on the batch, and:
//   SMZA_SOLVE  Q^H b left to right, dd_renorm once per chunk, then the back substitution right to left on chunks of which
//               only the rows above the chunk's last column are staged: column r has the BITS of k_small_zldiv on it alone.
//   SMZA_QH     the first phase alone: rows n .. m-1 have the bits of what the solve leaves there.
//   SMZA_QN     chunks nch-1 .. 0, columns 7 .. 0 inside a chunk, full rows staged, dd_renorm at the end of each chunk (by
//               the reflector's INDEX, as on the wave tier).  A reflector I - v v^H is Hermitian: the same expressions.
//   SMZA_FORMQ  SMZA_QN on columns e_r generated in registers: nothing of Q is read, all m x n is written.  The reflectors
//               c > r act as the identity on e_r (every product of the dot is an exact zero), so a workgroup starts at the
//               chunk that holds its group's last column -- one start for the whole workgroup.  For a finite factor the
//               result compares equal to SMZA_QN applied to [I; 0].
// Columns >= n of a chunk are staged as zeros and are no-ops.  Every consumer reads its whole column before anything is
// stored and stores it once at the end; rows >= m of a leading dimension and everything between matrices are never written.
// The pointers are plain device pointers (the host form stages in device memory).  Runs unchanged on the CPU emulator.
//
// Launch bound: 512 threads at SIX waves per SIMD, i.e. at most 80 registers per lane, so that three workgroups (3 x 33 KB
// of the 160 KB of LDS) share a compute unit: 18 double-double chains per compute unit.  Without the second bound the
// compiler spends all 128 registers a lane may have (two workgroups per compute unit); at eight waves per SIMD (64
// registers) every instantiation spills 9 - 23 registers.
// Compiler's resource report (gfx950, -O3, ROCm 7; profiles/batched_c64_kernel_resources.txt):
//   k_small_zapply<SMZA_SOLVE>   VGPRs 78, AGPRs 0, SGPRs 57, LDS 33024 B, scratch 0 B / lane, no spill, 6 waves / SIMD
//   k_small_zapply<SMZA_QH>      VGPRs 75, AGPRs 0, SGPRs 49, LDS 32768 B, scratch 0 B / lane, no spill, 6 waves / SIMD
//   k_small_zapply<SMZA_QN>      VGPRs 75, AGPRs 0, SGPRs 47, LDS 32768 B, scratch 0 B / lane, no spill, 6 waves / SIMD
//   k_small_zapply<SMZA_FORMQ>   VGPRs 75, AGPRs 0, SGPRs 54, LDS 32768 B, scratch 0 B / lane, no spill, 6 waves / SIMD
#pragma once
#include "dhqr_small_complex.h"

#define SMZA_THREADS 512  // 8 waves
#define SMZA_CW 6         // consumer waves = columns of B per workgroup; the other two waves stage the factor
#define SMZA_SOLVE 0
#define SMZA_QH 1
#define SMZA_QN 2
#define SMZA_FORMQ 3
#define SMZA_MIN_WAVES 6  // per SIMD: three workgroups per compute unit

// One reflector v (its rows l and l + 64; zeros above its first row) on the column b = (br, bi), each hi + lo: the
// expressions of the first phase of k_small_zldiv (src:217-220).
__device__ __forceinline__ void smza_reflect(const double2 (&v)[2], dhqr_dd (&br)[2], dhqr_dd (&bi)[2]) {
  dhqr_dd sr = {0.0, 0.0}, si = {0.0, 0.0};
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    dd_add_prod(sr, v[r].x, br[r].hi);  // src:217: conj(v_i) b_i
    dd_add_prod(sr, v[r].y, bi[r].hi);
    dd_add_prod(si, v[r].x, bi[r].hi);
    dd_add_prod(si, -v[r].y, br[r].hi);
    sr.lo += v[r].x * br[r].lo + v[r].y * bi[r].lo;
    si.lo += v[r].x * bi[r].lo - v[r].y * br[r].lo;
  }
  const dhqr_dd tr = wave_sum_dd_plain(sr), ti = wave_sum_dd_plain(si);
  const double s_r = tr.hi + tr.lo, s_i = ti.hi + ti.lo;
#pragma unroll
  for (int r = 0; r < 2; ++r) {  // src:218-220: b_i -= v_i s
    dd_add_prod(br[r], -s_r, v[r].x);
    dd_add_prod(br[r], s_i, v[r].y);
    dd_add_prod(bi[r], -s_i, v[r].x);
    dd_add_prod(bi[r], -s_r, v[r].y);
  }
}

// MODE: SMZA_SOLVE (B_k <- [X_k; tail of Q^H B_k], src:284-294) | SMZA_QH (B_k <- Q_k^H B_k) | SMZA_QN (B_k <- Q_k B_k) |
// SMZA_FORMQ (B_k <- Q_k [I; 0]: nrhs = n) for 1 <= n <= m <= 128.  B_k = B + k strideB (m x nrhs, ldb); lda, ldb and the
// strides count complex elements.  alpha is read by SMZA_SOLVE alone (else it may be nullptr).  groups = ceil(nrhs / SMZA_CW);
// the grid is batch * groups.
template <int MODE>
__global__ __launch_bounds__(SMZA_THREADS, SMZA_MIN_WAVES) void k_small_zapply(const double2 *__restrict__ A, int64_t lda, int64_t strideA,
                                                                               int m, int n, const double2 *__restrict__ alpha,
                                                                               int64_t stride_alpha, double2 *__restrict__ B, int nrhs,
                                                                               int64_t ldb, int64_t strideB, int groups) {
  constexpr int CH = SMZL_CH, LDR = SMZ_MAX, CW = SMZA_CW;
  constexpr bool FORWARD = MODE == SMZA_SOLVE || MODE == SMZA_QH;
  const int64_t k = (int64_t)blockIdx.x / groups;
  const int g = (int)((int64_t)blockIdx.x - k * groups);
  A += k * strideA;
  if (MODE == SMZA_SOLVE) alpha += k * stride_alpha;
  __shared__ double2 buf[2][CH][LDR];
  __shared__ double2 als[MODE == SMZA_SOLVE ? 2 : 1][CH];
  const int t = threadIdx.x, l = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);  // (a scalar: every test on it is a branch of the whole wave)
  const int nch = (n + CH - 1) / CH;
  const bool consumer = w < CW;
  const int col = CW * g + w;                // a consumer's column of B_k
  const bool active = consumer && col < nrhs;
  double2 *bcol = B + k * strideB + (int64_t)(active ? col : 0) * ldb;
  // the first chunk of a right-to-left pass: the last one, or (explicit Q) the one that holds the group's last column
  int clast = nch - 1;
  if (MODE == SMZA_FORMQ) {
    const int last = CW * g + CW - 1 < n ? CW * g + CW - 1 : n - 1;
    clast = last / CH;
  }
  // producers: columns [CH c, CH c + CH) rows [0, rtop) -> buf[c & 1] (zeros beyond the matrix); every load of a thread is
  // issued before its first LDS store
  auto stage = [&](int c, int rtop) {
    double2(*S)[LDR] = buf[c & 1];
    constexpr int NS = SMZA_THREADS - 64 * CW, PER = (CH * LDR + NS - 1) / NS;
    const int t0 = t - 64 * CW;
    double2 x[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = t0 + u * NS;
      const int jj = e / LDR, row = e % LDR, cj = CH * c + jj;
      x[u] = zmake(0.0, 0.0);
      if (jj < CH && cj < n && row < rtop && row < m) x[u] = A[(int64_t)row + (int64_t)cj * lda];
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = t0 + u * NS;
      if (e / LDR < CH) S[e / LDR][e % LDR] = x[u];
    }
    if (MODE == SMZA_SOLVE && t0 < CH) als[c & 1][t0] = (CH * c + t0 < n) ? alpha[CH * c + t0] : zmake(1.0, 0.0);
  };
  // consumers: the reflectors of chunk c (FWD: columns 0 .. 7, else 7 .. 0) on the column, then once per chunk the
  // renormalisation that keeps the low parts small against the high ones
  dhqr_dd br[2], bi[2];  // rows l and l + 64 of the column = (br, bi), each hi + lo
  auto reflect_chunk = [&](int c, auto fwd) {
    constexpr bool FWD = decltype(fwd)::value;
    const double2(*S)[LDR] = buf[c & 1];
#pragma unroll 2
    for (int q = 0; q < CH; ++q) {
      const int jj = FWD ? q : CH - 1 - q;
      const int j = CH * c + jj;  // (columns >= n are staged as zeros: no-ops)
      double2 v[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int row = l + 64 * r;
        const double2 x = S[jj][row];
        v[r] = zmake(row >= j ? x.x : 0.0, row >= j ? x.y : 0.0);  // rows < j of a factored column hold R
      }
      smza_reflect(v, br, bi);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      dd_renorm(br[r]);
      dd_renorm(bi[r]);
    }
  };
  if (consumer) {
    if (active) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int row = l + 64 * r;
        if (MODE == SMZA_FORMQ) {
          br[r].hi = row == col ? 1.0 : 0.0;  // e_col
          bi[r].hi = 0.0;
        } else {
          const double2 bt = bcol[row < m ? row : 0];
          br[r].hi = row < m ? bt.x : 0.0;
          bi[r].hi = row < m ? bt.y : 0.0;
        }
        br[r].lo = bi[r].lo = 0.0;
      }
    }
  } else {
    stage(FORWARD ? 0 : clast, m);
  }
  __syncthreads();
  if (FORWARD) {
    // ---- b <- Q^H b: reflectors left to right (src:215-224, k_zqtb_col_dd)
    for (int c = 0; c < nch; ++c) {
      if (consumer) {
        if (active) reflect_chunk(c, std::true_type{});
      } else if (c + 1 < nch) {
        stage(c + 1, m);
      }
      __syncthreads();
    }
  } else {
    // ---- b <- Q b: reflectors right to left
    for (int c = clast; c >= 0; --c) {
      if (consumer) {
        if (active) reflect_chunk(c, std::false_type{});
      } else if (c > 0) {
        stage(c - 1, m);
      }
      __syncthreads();
    }
  }
  if (MODE == SMZA_SOLVE) {
    // ---- back substitution, columns right to left (src:244-254, k_zbacksub_diag_dd): x_j = b_j / alpha_j, b[0:j] -= R[0:j, j] x_j
    // chunk nch - 1 is staged first; its parity may collide with the buffer the consumers read last, which the barrier above
    // released
    if (!consumer) stage(nch - 1, n);
    __syncthreads();
    for (int c = nch - 1; c >= 0; --c) {
      if (consumer) {
        if (active) {
          const double2(*S)[LDR] = buf[c & 1];
#pragma unroll 2
          for (int jj = CH - 1; jj >= 0; --jj) {
            const int j = CH * c + jj;
            if (j < n) {  // wave-uniform
              const int rj = j >> 6;
              const double2 bj = zmake(rj ? br[1].hi + br[1].lo : br[0].hi + br[0].lo, rj ? bi[1].hi + bi[1].lo : bi[0].hi + bi[0].lo);
              const double2 xj = zdiv(bqz_readlane(bj, j & 63), als[c & 1][jj]);  // src:251
#pragma unroll
              for (int r = 0; r < 2; ++r) {
                const int row = l + 64 * r;
                if (row == j) {
                  br[r].hi = xj.x;
                  br[r].lo = 0.0;
                  bi[r].hi = xj.y;
                  bi[r].lo = 0.0;
                } else if (row < j) {  // src:248-250: b_i -= R_ij x_j
                  const double2 rr = S[jj][row];
                  dd_add_prod(br[r], -rr.x, xj.x);
                  dd_add_prod(br[r], rr.y, xj.y);
                  dd_add_prod(bi[r], -rr.x, xj.y);
                  dd_add_prod(bi[r], -rr.y, xj.x);
                }
              }
            }
          }
        }
      } else if (c > 0) {
        stage(c - 1, CH * c);  // only rows above the chunk's last column are needed
      }
      __syncthreads();
    }
  }
  if (active) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int row = l + 64 * r;
      if (row < m) bcol[row] = zmake(br[r].hi + br[r].lo, bi[r].hi + bi[r].lo);
    }
  }
}
