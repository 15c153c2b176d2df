// dhqr_small_complex.h -- qr!(A) and H \ b of a SMALL ComplexF64 matrix, each in ONE single-workgroup launch.
//
// The complex twins of k_small_qr_d / k_small_ldiv (dhqr_small.h) for 1 <= n <= m <= 128: a 128 x 128 complex matrix is
// 256 KB, half of one compute unit's 512 KB of registers, so the reference's column-by-column algorithm (src:122-148,
// 171-213) runs with the whole matrix resident in VGPRs as (re, im) and ONE workgroup barrier per column.  A batch
// (dhqr_factor_batched_c64 / dhqr_solve_batched_c64) is the same kernel with grid = batch, workgroup k on matrix k.
//
//   k_small_zqr    512 threads = 8 waves, two per SIMD (256 registers per lane).  The layout is that of k_small_qr_d<8, 4>:
//                  lane (rg, cs) of wave w holds rows rg + 16 r (r < 8) of the columns 32 q + 4 w + cs (q < 4) -- a 16-lane
//                  DPP row spans 16 consecutive matrix rows of one column, the four rows of a wave are four adjacent
//                  columns: 32 complex = 128 VGPRs of matrix per lane.  The conj-dot v_j^H a_c (src:51-59) is 4 fma per
//                  row and two 4-step DPP reductions inside the 16-lane row, the update (src:171-196) 4 fma per row.
//                  BARRIER FORM ONLY: the kernel waits on nothing but __syncthreads() -- no flag, no poll, no bounded wait.
//                  A step: the owner of column j + 1 writes it to LDS as it updates it (inside its pass of reflector j);
//                  barrier; EVERY wave builds reflector j + 1 from that copy by the same instructions on the same numbers
//                  (two rows per lane, norm in double-double: dd_add_sq + wave_sum_dd_plain, alpha / f / pivot as
//                  k_batched_zqr_wave forms them), each lane scales the rows it holds itself.  So there is no builder wave,
//                  no second barrier and no second copy of a column that could differ in a rounding: the owner's lanes
//                  overwrite rows >= j of column j with the very values every wave applies (the "take-back" of
//                  k_small_qr_d without a hand-back), and what is stored is bit for bit the reflector that was applied.
//                  The price is the construction (one sqrt, one hypot, three divisions and one more sqrt behind two wave
//                  reductions) on every wave's chain once per column.
//   k_small_zldiv  256 threads: wave 0 keeps b in registers (two rows per lane, both parts in double-double: 8 doubles) and
//                  walks the columns, waves 1-3 stream the factor in 8-column chunks (16 KB) into a double-buffered LDS stage
//                  ahead of it -- once left to right for Q^H b (src:215-224), once right to left, upper triangle only, for
//                  the back substitution (src:244-254: Smith's division by alpha_j, as k_zbacksub_diag_dd).
//
// A column whose reflector is not finite (a zero column, a NaN, an infinity) ends the factorisation: what the reference
// leaves behind such a column j0 is known without computing it (see `dead_from` in dhqr_small.h) -- columns < j0 and rows
// < j0 as they stand, alpha[j0] as formed, NaN in alpha behind it and in rows >= j0 of the columns >= j0 -- and no product
// 0 * NaN can reach a finished column or R.  Every wave takes that decision from the same numbers, so it is uniform.
//
// Both kernels take plain pointers that may be device memory or pinned host memory (dhqr_qr_c64 / dhqr_ldiv_c64 hand them
// the context's pinned staging buffer and poll the word of small_signal_done), and both run unchanged on the CPU emulator.
//
// Register budget, k_small_zqr: 128 (matrix) + 16 (reflector rows) + 8 (two dot products in flight) + addresses and masks,
// of the 256 a lane has at two waves per SIMD.  Compiler's resource report (gfx950, -O3, ROCm 7):
//   k_small_zqr     VGPRs 199, AGPRs 0, SGPRs 106 (6 of them kept in vector lanes, none in memory), LDS 6144 B,
//                   scratch 0 B / lane, no dynamic stack, 2 waves / SIMD
//   k_small_zldiv   VGPRs  82, AGPRs 0, SGPRs 67, LDS 33024 B, scratch 0 B / lane, no spill
#pragma once
#include "dhqr_batched_complex.h"
#include "dhqr_small.h"

#define SMZ_THREADS 512  // k_small_zqr: 8 waves
#define SMZ_NR 8         // rows rg + 16 r of a column per lane
#define SMZ_NQ 4         // column groups of SMQ_GW = 32
#define SMZ_MAX 128      // most rows and columns (16 SMZ_NR, SMQ_GW SMZ_NQ)
#define SMZL_CH 8        // k_small_zldiv: columns per LDS chunk

// One pass of reflector j (vr: its rows rg + 16 r, zeros above row j and for r < R0) over the column groups of this wave.
// Inside the update of a group, as in smq_pass_d: the lanes of column j itself take the reflector (rows >= j), the lanes of
// column j + 1 hand their updated column to LDS (xo) for the next construction.
template <int R0>
__device__ __forceinline__ void smz_pass(double2 (&a)[SMZ_NQ][SMZ_NR], const double2 (&vr)[SMZ_NR], int j, int cbase, double2 *xo) {
  const int rg = threadIdx.x & 15;
#pragma unroll
  for (int q = 0; q < SMZ_NQ; ++q) {
    if (SMQ_GW * (q + 1) - 1 >= j) {  // (uniform; >=: the group of column j itself still takes its reflector)
      const int col = SMQ_GW * q + cbase;
      if (q == j / SMQ_GW) {  // (uniform) src:133-140
#pragma unroll
        for (int r = R0; r < SMZ_NR; ++r) {
          const bool take = col == j && rg + 16 * r >= j;
          a[q][r].x = take ? vr[r].x : a[q][r].x;
          a[q][r].y = take ? vr[r].y : a[q][r].y;
        }
      }
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int r = R0; r < SMZ_NR; ++r) zcdot_acc(vr[r], a[q][r], sr, si);  // src:51-59
      sr = row16_sum(sr);
      si = row16_sum(si);
      const bool behind = col > j;  // columns <= j are finished, columns >= n hold zeros
      const double dr = behind ? sr : 0.0, di = behind ? si : 0.0;
#pragma unroll
      for (int r = R0; r < SMZ_NR; ++r) a[q][r] = zsubmul(a[q][r], vr[r], dr, di);  // src:171-196, src:209
      if (q == (j + 1) / SMQ_GW) {  // (uniform)
#pragma unroll
        for (int r = 0; r < SMZ_NR; ++r)
          if (col == j + 1) xo[rg + 16 * r] = a[q][r];
      }
    }
  }
}

// householder!(A, alpha) (src:113, 122-148, 171-213) for 1 <= n <= m <= 128.  Asrc / Adst may alias; leading dimensions
// and strides count complex elements.
__global__ __launch_bounds__(SMZ_THREADS) void k_small_zqr(const double2 *Asrc, int64_t lds, double2 *Adst, int64_t ldd, int m, int n,
                                                           double2 *__restrict__ alpha, unsigned long long *done,
                                                           unsigned long long epoch, int64_t strideS, int64_t strideD,
                                                           int64_t stride_alpha) {
  Asrc += (int64_t)blockIdx.x * strideS;
  Adst += (int64_t)blockIdx.x * strideD;
  alpha += (int64_t)blockIdx.x * stride_alpha;
  __shared__ double2 xcol[2][SMZ_MAX];  // column j, updated through reflector j - 1 (by column parity)
  __shared__ double2 als[SMZ_MAX];
  const int t = threadIdx.x, w = t >> 6, l = t & 63, rg = l & 15, cs = l >> 4;
  const int cbase = 4 * w + cs;  // this lane's column of group q: 32 q + cbase
  double2 a[SMZ_NQ][SMZ_NR];
#pragma unroll
  for (int q = 0; q < SMZ_NQ; ++q)
#pragma unroll
    for (int r = 0; r < SMZ_NR; ++r) {
      const int row = rg + 16 * r, col = SMQ_GW * q + cbase;
      a[q][r] = zmake(0.0, 0.0);
      if (row < m && col < n) a[q][r] = Asrc[(int64_t)row + (int64_t)col * lds];
    }
  if (cbase == 0) {
#pragma unroll
    for (int r = 0; r < SMZ_NR; ++r) xcol[0][rg + 16 * r] = a[0][r];  // column 0 as it came
  }
  __syncthreads();
  int dead_from = 0x7fffffff;  // the first column whose reflector is not finite (the same value in every thread)
  // reflector j (src:129-140) from xcol -- every wave, the same instructions on the same numbers -- then its pass
  auto step = [&](auto r0c, int j) __attribute__((always_inline)) -> bool {
    constexpr int R0 = decltype(r0c)::value;
    const double2 *xi = xcol[j & 1];
    const double2 x0 = xi[l], x1 = xi[l + 64];  // rows >= m hold zeros
    dhqr_dd acc = {0.0, 0.0};
    dd_add_sq(acc, l >= j ? x0.x : 0.0);
    dd_add_sq(acc, l >= j ? x0.y : 0.0);
    dd_add_sq(acc, l + 64 >= j ? x1.x : 0.0);
    dd_add_sq(acc, l + 64 >= j ? x1.y : 0.0);
    const dhqr_dd ss = wave_sum_dd_plain(acc);
    const double sn = sqrt(ss.hi + ss.lo);  // src:129
    const double2 h = bqz_readlane((j >> 6) ? x1 : x0, j & 63);  // (uniform, like sn: the test below is a scalar branch)
    double ah;
    const double2 af = zalphafactor(h, &ah);
    const double2 al = zmake(sn * af.x, sn * af.y);  // src:130
    const double f = 1.0 / sqrt(sn * (sn + ah));     // src:131
    const double2 piv = zmake((h.x - al.x) * f, (h.y - al.y) * f);  // src:132
    if (t == 0) als[j] = al;
    // a zero column (f = 1 / 0), a NaN or an infinity in it, a norm beyond the range: the pivot entry or the norm tells
    const double big = 1.7976931348623157e308;
    if (!(sn > 0.0 && sn <= big && fabs(piv.x) <= big && fabs(piv.y) <= big)) return false;
    double2 vr[SMZ_NR];
#pragma unroll
    for (int r = 0; r < SMZ_NR; ++r) {
      const int row = rg + 16 * r;
      vr[r] = zmake(0.0, 0.0);
      if (r >= R0) {
        const double2 x = xi[row];
        vr[r].x = row > j ? x.x * f : (row == j ? piv.x : 0.0);  // src:133-140
        vr[r].y = row > j ? x.y * f : (row == j ? piv.y : 0.0);
      }
    }
    smz_pass<R0>(a, vr, j, cbase, xcol[(j + 1) & 1]);
    __syncthreads();  // column j + 1 is in xcol, every wave is done with column j's copy
    return true;
  };
  {
    int j = 0;  // (the last step, j = n - 1, only puts reflector n - 1 into its column: nothing lies behind it)
    bool ok = true;
    for (; ok && j < n && j < 32; ++j) ok = step(std::integral_constant<int, 0>{}, j);
    for (; ok && j < n && j < 64; ++j) ok = step(std::integral_constant<int, 2>{}, j);
    for (; ok && j < n && j < 96; ++j) ok = step(std::integral_constant<int, 4>{}, j);
    for (; ok && j < n; ++j) ok = step(std::integral_constant<int, 6>{}, j);
    if (!ok) dead_from = j - 1;
  }
  __syncthreads();  // als
#pragma unroll
  for (int q = 0; q < SMZ_NQ; ++q) {
    const int col = SMQ_GW * q + cbase;
#pragma unroll
    for (int r = 0; r < SMZ_NR; ++r) {
      const int row = rg + 16 * r;
      if (row < m && col < n) {
        const bool lost = row >= dead_from && col >= dead_from;
        Adst[(int64_t)row + (int64_t)col * ldd] = lost ? zmake(__builtin_nan(""), __builtin_nan("")) : a[q][r];
      }
    }
  }
  for (int i = t; i < n; i += SMZ_THREADS) alpha[i] = i > dead_from ? zmake(__builtin_nan(""), __builtin_nan("")) : als[i];
  small_signal_done(done, epoch);
}

// solve_householder!(b, H, alpha) (src:284-294) for 1 <= n <= m <= 128: bout (m) <- [x; tail of Q^H b], xout (n, may be
// nullptr) <- x; bin / bout may alias.  b is carried in double-double per component through Q^H b (the per-lane expressions
// of k_batched_zldiv_wave) and the back substitution, x rounded once per entry: the reference's acceptance statistic sees
// the solve's rounding (dhqr_solve_c64).  Awork != nullptr: A is pinned HOST memory and is first copied there (m x n,
// leading dimension m; device memory) with every load in flight at once, as k_small_ldiv does.
__global__ __launch_bounds__(SML_THREADS) void k_small_zldiv(const double2 *__restrict__ A, int64_t lda, int m, int n,
                                                             const double2 *__restrict__ alpha, const double2 *bin, double2 *bout,
                                                             double2 *xout, double2 *__restrict__ Awork, unsigned long long *done,
                                                             unsigned long long epoch, int64_t strideA, int64_t stride_alpha,
                                                             int64_t strideb) {
  A += (int64_t)blockIdx.x * strideA;
  alpha += (int64_t)blockIdx.x * stride_alpha;
  bin += (int64_t)blockIdx.x * strideb;
  bout += (int64_t)blockIdx.x * strideb;
  constexpr int CH = SMZL_CH, LDR = SMZ_MAX;
  __shared__ double2 buf[2][CH][LDR];
  __shared__ double2 als[2][CH];
  const int t = threadIdx.x, w = t >> 6, l = t & 63;
  const int nch = (n + CH - 1) / CH;
  if (Awork) {
    const int total = m * n;
    for (int base = 0; base < total; base += 8 * SML_THREADS) {
      double2 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = base + u * SML_THREADS + t;
        x[u] = zmake(0.0, 0.0);
        if (idx < total) x[u] = A[(int64_t)(idx % m) + (int64_t)(idx / m) * lda];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = base + u * SML_THREADS + t;
        if (idx < total) Awork[idx] = x[u];
      }
    }
    __threadfence_block();
    __syncthreads();
    A = Awork;
    lda = m;
  }
  // waves 1..3: columns [CH c, CH c + CH) rows [0, rtop) -> buf[c & 1] (zeros beyond the matrix); every load of a thread is
  // issued before its first LDS store
  auto stage = [&](int c, int rtop) {
    double2(*B)[LDR] = buf[c & 1];
    constexpr int NS = SML_THREADS - 64, PER = (CH * LDR + NS - 1) / NS;
    double2 x[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = t - 64 + u * NS;
      const int jj = e / LDR, row = e % LDR, col = CH * c + jj;
      x[u] = zmake(0.0, 0.0);
      if (jj < CH && col < n && row < rtop && row < m) x[u] = A[(int64_t)row + (int64_t)col * lda];
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = t - 64 + u * NS;
      if (e / LDR < CH) B[e / LDR][e % LDR] = x[u];
    }
    if (t >= 64 && t < 64 + CH) als[c & 1][t - 64] = (CH * c + t - 64 < n) ? alpha[CH * c + t - 64] : zmake(1.0, 0.0);
  };
  dhqr_dd br[2], bi[2];  // rows l and l + 64 of b = (br, bi), each hi + lo
  if (w == 0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int row = l + 64 * r;
      const double2 bt = bin[row < m ? row : 0];
      br[r].hi = row < m ? bt.x : 0.0;
      bi[r].hi = row < m ? bt.y : 0.0;
      br[r].lo = bi[r].lo = 0.0;
    }
  } else {
    stage(0, m);
  }
  __syncthreads();
  // ---- b <- Q^H b: reflectors left to right (src:215-224, k_zqtb_col_dd)
  for (int c = 0; c < nch; ++c) {
    if (w == 0) {
      const double2(*B)[LDR] = buf[c & 1];
#pragma unroll 2
      for (int jj = 0; jj < CH; ++jj) {
        const int j = CH * c + jj;  // (columns >= n are staged as zeros: no-ops)
        double2 v[2];
        dhqr_dd sr = {0.0, 0.0}, si = {0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const int row = l + 64 * r;
          const double2 x = B[jj][row];
          v[r] = zmake(row >= j ? x.x : 0.0, row >= j ? x.y : 0.0);  // rows < j of a factored column hold R
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
#pragma unroll
      for (int r = 0; r < 2; ++r) {  // once per chunk: the low parts stay small against the high ones
        dd_renorm(br[r]);
        dd_renorm(bi[r]);
      }
    } else if (c + 1 < nch) {
      stage(c + 1, m);
    }
    __syncthreads();
  }
  // ---- back substitution, columns right to left (src:244-254, k_zbacksub_diag_dd): x_j = b_j / alpha_j, b[0:j] -= R[0:j, j] x_j
  // chunk nch - 1 is staged first; its parity may collide with the buffer wave 0 read last, which the barrier above released
  if (w != 0) stage(nch - 1, n);
  __syncthreads();
  for (int c = nch - 1; c >= 0; --c) {
    if (w == 0) {
      const double2(*B)[LDR] = buf[c & 1];
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
              const double2 rr = B[jj][row];
              dd_add_prod(br[r], -rr.x, xj.x);
              dd_add_prod(br[r], rr.y, xj.y);
              dd_add_prod(bi[r], -rr.x, xj.y);
              dd_add_prod(bi[r], -rr.y, xj.x);
            }
          }
        }
      }
    } else if (c > 0) {
      stage(c - 1, CH * c);  // only rows above the chunk's last column are needed
    }
    __syncthreads();
  }
  if (w == 0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int row = l + 64 * r;
      const double2 val = zmake(br[r].hi + br[r].lo, bi[r].hi + bi[r].lo);
      if (row < m) bout[row] = val;
      if (xout && row < n) xout[row] = val;
    }
  }
  small_signal_done(done, epoch);
}
