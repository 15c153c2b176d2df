// dhqr_batched_host.h -- the host side of the small-matrix entry points (dhqr.h: dhqr_factor_batched_f64 ...
// dhqr_ldiv_batched_nrhs_f32, dhqr_apply_q_batched_f64 ... dhqr_form_r_batched_f32, and the Float32 single-matrix forms),
// written once for T = double and T = float.  Host code
// only; included by dhqr_api.hip ahead of its extern "C" block (templates need C++ linkage), which keeps the exported
// functions themselves: ENTER, the argument check, one call into this file.
// Tiers by shape.  Float64: one wave per matrix (dhqr_batched.h) | the single-workgroup kernels of dhqr_small.h with grid =
// batch, in their barrier form | a host loop over the single-matrix drivers.  Float32: m <= 64 and n <= 32 with the small
// route on -- one launch of the same wave-per-matrix kernels with T = float (a single matrix is a batch of 1) --, everything else
// PROMOTED: widened into a Float64 workspace of the context, the Float64 route with the caller's nb, rounded back.
// ComplexF64 (dhqr_factor_batched_c64 ... dhqr_ldiv_batched_c64): the wave tier -- one launch of the kernels of
// dhqr_batched_complex.h -- | up to 128 rows one launch of the single-workgroup kernels of dhqr_small_complex.h with grid =
// batch | a host loop over dhqr_factor_c64_nb / dhqr_solve_c64; the host forms are those of the real types with T = double2.  Several right-hand sides, Q application, explicit Q and R (dhqr_solve_batched_nrhs_c64 ...
// dhqr_form_r_batched_c64): the wave tier -- one launch of the kernels of dhqr_batched_complex_nrhs.h -- | up to 128 rows
// one launch of k_small_zapply (dhqr_small_complex_nrhs.h), a workgroup per (matrix, group of SMZA_CW columns of B): Q and
// the explicit Q for every nrhs, the solve where that was measured to pay (zsmall_nrhs_pays: one or three groups of columns)
// | the solve column by column on the single-column route (the same bits), Q on k_batched_zapplyq_general.
// The host forms (qr_host, ldiv_host) end alike: after a failure of any step they still reach the final
// hipStreamSynchronize -- nothing is left in flight on the caller's arrays -- and return the FIRST error.  (Before, the
// single-column ldiv forms returned from a failed enqueue of the copy of X without it.)
#pragma once
#include <type_traits>
#include "dhqr_batched_complex_nrhs.h"
#include "dhqr_small_complex.h"
#include "dhqr_small_complex_nrhs.h"

static int32_t pipe_error_check(dhqr_ctx *c);  // (dhqr_api.hip, below this file's inclusion)

// ---- argument checks -----------------------------------------------------------------------------------------------------
static int32_t check_nb(int32_t nb) {
  if (nb != 0 && nb != DHQR_NB) return set_err(DHQR_EINVAL, "nb must be 0 (unblocked) or %d (blocked); got %d", DHQR_NB, nb);
  return DHQR_OK;
}
// (with_alpha = false: a call that takes the factor alone -- Q is made of the reflectors)
static int32_t check_batch(const void *A, int64_t m, int64_t n, int64_t lda, int64_t strideA, const void *alpha,
                           int64_t stride_alpha, int64_t batch, bool with_alpha = true) {
  CHECK(check_mat(A, m, n, lda, true));
  if (with_alpha && !alpha) return set_err(DHQR_EINVAL, "null alpha pointer");
  if (strideA < lda * (n - 1) + m)
    return set_err(DHQR_EINVAL, "strideA %lld < lda*(n-1)+m = %lld", (long long)strideA, (long long)(lda * (n - 1) + m));
  if (with_alpha && stride_alpha < n) return set_err(DHQR_EINVAL, "stride_alpha %lld < n=%lld", (long long)stride_alpha, (long long)n);
  if (batch > 0x7fffffffLL) return set_err(DHQR_EINVAL, "batch %lld too large", (long long)batch);
  return DHQR_OK;
}
static int32_t check_nrhs(const void *B, const char *name, int64_t rows, int64_t nrhs, int64_t ldb, int64_t strideB) {
  if (!B) return set_err(DHQR_EINVAL, "null %s pointer", name);
  if (nrhs > 0x7fffffffLL) return set_err(DHQR_EINVAL, "nrhs %lld too large", (long long)nrhs);
  if (ldb < rows) return set_err(DHQR_EINVAL, "leading dimension of %s %lld < %lld", name, (long long)ldb, (long long)rows);
  if (strideB < ldb * (nrhs - 1) + rows)
    return set_err(DHQR_EINVAL, "stride of %s %lld < ld*(nrhs-1)+rows = %lld", name, (long long)strideB,
                   (long long)(ldb * (nrhs - 1) + rows));
  return DHQR_OK;
}
// The right-hand sides (or solutions) of a batched call as its checker sees them: rows x nrhs elements per matrix, leading
// dimension ld, matrix k at p + k stride.  column: one per matrix (b / x of the single-column forms: nrhs = 1, ld = rows).
struct RhsArg {
  const void *p = nullptr;
  int64_t nrhs = 1, ld = 0, stride = 0;
  bool block = false, given = false;
};
static inline RhsArg rhs_column(const void *p, int64_t rows, int64_t stride) { return RhsArg{p, 1, rows, stride, false, true}; }
static inline RhsArg rhs_block(const void *p, int64_t nrhs, int64_t ld, int64_t stride) { return RhsArg{p, nrhs, ld, stride, true, true}; }
// The preamble of every batched entry point.  What the call has beside A and alpha: nb (qr!) | B (a solve on the device) |
// B and X (a solve on the host), both columns or both blocks | nothing (form_r).
// *empty: nothing to do (batch, n or nrhs is 0) -- and then no pointer, leading dimension or stride has been looked at.
static int32_t check_batched(bool *empty, const void *A, int64_t m, int64_t n, int64_t lda, int64_t strideA, const void *alpha,
                             int64_t stride_alpha, int64_t batch, const int32_t *nb, RhsArg B = RhsArg(), RhsArg X = RhsArg()) {
  if (B.block && B.nrhs < 0) return set_err(DHQR_EINVAL, "negative nrhs %lld", (long long)B.nrhs);
  if (batch < 0) return set_err(DHQR_EINVAL, "negative batch %lld", (long long)batch);
  *empty = (B.block && B.nrhs == 0) || batch == 0 || no_columns(m, n);
  if (*empty) return DHQR_OK;
  CHECK(check_batch(A, m, n, lda, strideA, alpha, stride_alpha, batch));
  if (nb) return check_nb(*nb);
  if (!B.given) return DHQR_OK;  // (the factor and alpha alone: form_r, which checks its R itself)
  if (B.block) {
    CHECK(check_nrhs(B.p, "B", m, B.nrhs, B.ld, B.stride));
    return X.given ? check_nrhs(X.p, "X", n, X.nrhs, X.ld, X.stride) : DHQR_OK;
  }
  if (X.given ? !B.p || !X.p : !B.p) return set_err(DHQR_EINVAL, X.given ? "null pointer argument" : "null b pointer");
  if (B.stride < m) return set_err(DHQR_EINVAL, "strideb %lld < m=%lld", (long long)B.stride, (long long)m);
  if (X.given && X.stride < n) return set_err(DHQR_EINVAL, "stridex %lld < n=%lld", (long long)X.stride, (long long)n);
  return DHQR_OK;
}
#define CHECK_BATCHED(...)                       \
  do {                                           \
    bool empty_ = false;                         \
    CHECK(check_batched(&empty_, __VA_ARGS__));  \
    if (empty_) return DHQR_OK;                  \
  } while (0)
// The preamble of the entry points that take a factor WITHOUT alpha and a block of m rows (apply_q: B; form_q: Q, nrhs = n).
static int32_t check_batched_q(bool *empty, const void *A, int64_t m, int64_t n, int64_t lda, int64_t strideA, int64_t batch, RhsArg B,
                               const char *name, int32_t trans) {
  if (B.nrhs < 0) return set_err(DHQR_EINVAL, "negative nrhs %lld", (long long)B.nrhs);
  if (batch < 0) return set_err(DHQR_EINVAL, "negative batch %lld", (long long)batch);
  if (trans != 0 && trans != 1) return set_err(DHQR_EINVAL, "trans must be 0 (Q B) or 1 (Q'B); got %d", (int)trans);
  *empty = B.nrhs == 0 || batch == 0 || no_columns(m, n);
  if (*empty) return DHQR_OK;
  CHECK(check_batch(A, m, n, lda, strideA, nullptr, 0, batch, false));
  return check_nrhs(B.p, name, m, B.nrhs, B.ld, B.stride);
}
#define CHECK_BATCHED_Q(...)                       \
  do {                                             \
    bool empty_ = false;                           \
    CHECK(check_batched_q(&empty_, __VA_ARGS__));  \
    if (empty_) return DHQR_OK;                    \
  } while (0)

// ---- the wave tier: one wave per matrix, BQW_WAVES matrices per workgroup -------------------------------------------------
static inline bool batched_wave_fit(const dhqr_ctx *c, int64_t m, int64_t n) {
  return c->small_route && c->batched_wave && m <= BQW_MAX_M && n <= BQW_MAX_N && n >= 1 && m >= n;
}
// the instantiation (columns held per wave) that serves n columns
static inline int wave_nc(int64_t n) { return n <= 8 ? 8 : n <= 16 ? 16 : 32; }
// one launch of kernel_<NC targs_> for `batch_` matrices of n_ columns on c->stream (returns from the caller on a launch
// error); targs_: nothing, or WAVE_TARGS(further template arguments)
#define WAVE_TARGS(...) , __VA_ARGS__
#define WAVE_LAUNCH_T(kernel_, targs_, n_, batch_, ...)                                                         \
  do {                                                                                                          \
    const dim3 grid_((unsigned)(((batch_) + BQW_WAVES - 1) / BQW_WAVES)), block_(64 * BQW_WAVES);               \
    switch (wave_nc(n_)) {                                                                                      \
      case 8: hipLaunchKernelGGL((kernel_<8 targs_>), grid_, block_, 0, c->stream, __VA_ARGS__); break;         \
      case 16: hipLaunchKernelGGL((kernel_<16 targs_>), grid_, block_, 0, c->stream, __VA_ARGS__); break;       \
      default: hipLaunchKernelGGL((kernel_<32 targs_>), grid_, block_, 0, c->stream, __VA_ARGS__);              \
    }                                                                                                           \
    LAUNCHCHECK();                                                                                              \
  } while (0)
#define WAVE_LAUNCH(kernel_, n_, batch_, ...) WAVE_LAUNCH_T(kernel_, , n_, batch_, __VA_ARGS__)
// right-hand sides per group of the multi-column kernels (dhqr_batched_nrhs.h) in the instantiation NC
template <typename T>
static inline int wave_rg(int NC) {
  return bqn_rg<T>(NC);
}

template <typename T>
static int32_t wave_factor(dhqr_ctx *c, T *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, T *dalpha, int64_t stride_alpha,
                           int64_t batch) {
  CHECK(prof_begin(c, CAT_RANK1));  // ONE launch, one group
  WAVE_LAUNCH_T(k_batched_qr_wave, WAVE_TARGS(T), n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, batch);
  if (c->profiling)  // (an element update reads and writes one T)
    for (int64_t j = 0; j + 1 < n; ++j)
      c->st.bytes_rank1 += (double)batch * (double)(2 * sizeof(T)) * (double)(m - j) * (double)(n - j - 1);
  return prof_end(c);
}
template <typename T>
static int32_t wave_solve(dhqr_ctx *c, const T *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const T *dalpha,
                          int64_t stride_alpha, T *db, int64_t strideb, int64_t batch) {
  CHECK(prof_begin(c, CAT_SOLVE));
  WAVE_LAUNCH_T(k_batched_ldiv_wave, WAVE_TARGS(T), n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, db, strideb, batch);
  return prof_end(c);
}
// several right-hand sides per matrix: ONE launch of the multi-column kernels of dhqr_batched_nrhs.h
template <typename T>
static int32_t wave_solve_nrhs(dhqr_ctx *c, const T *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const T *dalpha,
                               int64_t stride_alpha, T *dB, int64_t nrhs, int64_t ldb, int64_t strideB, int64_t batch) {
  CHECK(prof_begin(c, CAT_SOLVE));  // ONE launch, one group, whatever nrhs and batch
  // (the real kernels are two: dhqr_batched_nrhs.h says why they are not one template over T)
  if constexpr (std::is_same_v<T, double>)
    WAVE_LAUNCH(k_batched_ldiv_wave_nrhs, n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, dB, (int)nrhs, ldb, strideB, batch);
  else if constexpr (std::is_same_v<T, double2>)
    WAVE_LAUNCH(k_batched_zldiv_wave_nrhs, n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, dB, (int)nrhs, ldb, strideB, batch);
  else
    WAVE_LAUNCH(k_batched_ldiv_wave_nrhs_s, n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, dB, (int)nrhs, ldb, strideB, batch);
  return prof_end(c);
}
// B_k <- Q_k'B_k | Q_k B_k | Q_k [I; 0]: ONE launch of the kernels of dhqr_batched_applyq.h
constexpr bool FORM_Q = true, APPLY_Q = false;  // `formq` of wave_apply_q / apply_q_batched
template <typename T>
static int32_t wave_apply_q(dhqr_ctx *c, const T *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, T *dB, int64_t nrhs, int64_t ldb,
                            int64_t strideB, int64_t batch, int trans, bool formq) {
  CHECK(prof_begin(c, CAT_SOLVE));  // ONE launch, one group, whatever nrhs and batch
#define APPLYQ_LAUNCH(kernel_)                                                                                                 \
  do {                                                                                                                         \
    if (formq)                                                                                                                 \
      WAVE_LAUNCH_T(kernel_, WAVE_TARGS(0, 1), n, batch, dA, lda, strideA, (int)m, (int)n, dB, (int)nrhs, ldb, strideB, batch); \
    else if (trans)                                                                                                            \
      WAVE_LAUNCH_T(kernel_, WAVE_TARGS(1), n, batch, dA, lda, strideA, (int)m, (int)n, dB, (int)nrhs, ldb, strideB, batch);    \
    else                                                                                                                       \
      WAVE_LAUNCH_T(kernel_, WAVE_TARGS(0), n, batch, dA, lda, strideA, (int)m, (int)n, dB, (int)nrhs, ldb, strideB, batch);    \
  } while (0)
  if constexpr (std::is_same_v<T, double>) APPLYQ_LAUNCH(k_batched_applyq_wave);
  else if constexpr (std::is_same_v<T, double2>) APPLYQ_LAUNCH(k_batched_zapplyq_wave);
  else APPLYQ_LAUNCH(k_batched_applyq_wave_s);
#undef APPLYQ_LAUNCH
  return prof_end(c);
}
// Does the multi-column kernel pay?  Measured (profiles/batched_nrhs_throughput.txt, batch 16384): the kernel is bound by
// instruction issue, not by re-reading the matrix, and its time goes by GROUPS -- a group of rg chains costs 2.5 to 3.0
// single-column solves whether its columns are real or the zeros of a tail.  nrhs = 2 loses everywhere (0.62 - 0.81 x the
// column loop), nrhs = 4 in groups of three (Float64, n > 8) loses (0.77 - 0.80 x); nrhs = 4 in groups of four, 8 and 16 win
// (1.01 - 1.23 x).  So: the kernel where the groups carry at least 2.6 real columns on average, the column loop -- the
// same bits -- elsewhere.
template <typename T>
static inline bool nrhs_wave_pays(int64_t nrhs, int64_t n) {
  const int rg = wave_rg<T>(wave_nc(n));
  const int64_t groups = (nrhs + rg - 1) / rg;
  return 5 * nrhs >= 13 * groups;
}

// ---- Float64 on the device ---------------------------------------------------------------------------------------------
// (`single` belongs to the Float32 forms below; the Float64 single-matrix entry points are not in this file)
static int32_t factor_batched(dhqr_ctx *c, double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, double *dalpha,
                              int64_t stride_alpha, int64_t batch, int32_t nb, bool /*single*/ = false) {
  const bool wave = batched_wave_fit(c, m, n);
  const int fit = small_qr_fit(c, m, n);
  if (!wave && fit < 0) {  // serial: one single-matrix factorisation after the other
    // (and synchronised after each: the error word of the drivers' bounded waits belongs to one call at a time, dhqr.h)
    for (int64_t k = 0; k < batch; ++k) {
      CHECK(dhqr_factor_f64(c, dA + k * strideA, m, n, lda, dalpha + k * stride_alpha, nb));
      HIPCHECK(hipStreamSynchronize(c->stream));
      CHECK(pipe_error_check(c));
    }
    return DHQR_OK;
  }
  c->tc_valid = false;  // whatever was kept for one of these matrices is gone
  c->retry.valid = false;
  if (wave) return wave_factor(c, dA, m, n, lda, strideA, dalpha, stride_alpha, batch);
  CHECK(prof_begin(c, CAT_RANK1));  // ONE launch, one group
  // the barrier form for every fit: with a batch in flight the compute units are full either way, and the barrier form
  // has no bounded wait that could give up (same bits as the flag form)
  const SmallBatch sb{batch, strideA, stride_alpha};
  const int keep = c->small_flags;
  c->small_flags = 0;
  const int32_t rc = small_qr_launch_strided(c, fit, dA, lda, dA, lda, m, n, dalpha, nullptr, 0, sb);
  c->small_flags = keep;
  CHECK(rc);
  if (c->profiling)
    for (int64_t j = 0; j + 1 < n; ++j) c->st.bytes_rank1 += (double)batch * 16.0 * (double)(m - j) * (double)(n - j - 1);
  return prof_end(c);
}

static int32_t solve_batched(dhqr_ctx *c, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const double *dalpha,
                             int64_t stride_alpha, double *db, int64_t strideb, int64_t batch, bool /*single*/ = false) {
  if (batched_wave_fit(c, m, n)) return wave_solve(c, dA, m, n, lda, strideA, dalpha, stride_alpha, db, strideb, batch);
  if (!small_ldiv_fit(c, m, n)) {
    for (int64_t k = 0; k < batch; ++k) {  // (a solve's repetition, pipe_error_check, knows the last solve only)
      CHECK(dhqr_solve_f64(c, dA + k * strideA, m, n, lda, dalpha + k * stride_alpha, db + k * strideb));
      HIPCHECK(hipStreamSynchronize(c->stream));
      CHECK(pipe_error_check(c));
    }
    return DHQR_OK;
  }
  CHECK(prof_begin(c, CAT_SOLVE));
  const SmallBatch sb{batch, strideA, stride_alpha, strideb};
  CHECK(small_ldiv_launch(c, dA, lda, m, n, dalpha, db, db, nullptr, nullptr, nullptr, 0, sb));  // (the factor is in HBM: no Awork)
  return prof_end(c);
}

// The wave tier where it pays: the multi-column kernel.  Every other shape: the single-column route, column by column --
// its tiers, its synchronisation, its profiling counts, its bits.
static int32_t solve_batched_nrhs(dhqr_ctx *c, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                  const double *dalpha, int64_t stride_alpha, double *dB, int64_t nrhs, int64_t ldb, int64_t strideB,
                                  int64_t batch) {
  if (batched_wave_fit(c, m, n) && nrhs_wave_pays<double>(nrhs, n))
    return wave_solve_nrhs(c, dA, m, n, lda, strideA, dalpha, stride_alpha, dB, nrhs, ldb, strideB, batch);
  for (int64_t r = 0; r < nrhs; ++r)
    CHECK(solve_batched(c, dA, m, n, lda, strideA, dalpha, stride_alpha, dB + r * ldb, strideB, batch));
  return DHQR_OK;
}

// ---- Float32 on the device: the native wave tier, else promoted ---------------------------------------------------------
static int32_t f32_convert_launch(dhqr_ctx *c, bool widen, const void *src, int64_t lds, int64_t sstride, void *dst, int64_t ldd,
                                  int64_t dstride, int64_t rows, int64_t cols, int64_t batch) {
  const int64_t total = rows * cols * batch;
  if (total <= 0) return DHQR_OK;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32);
  if (widen)
    hipLaunchKernelGGL(k_widen_f32, dim3(grid), dim3(256), 0, c->stream, (const float *)src, lds, sstride, (double *)dst, ldd, dstride,
                       rows, cols, batch);
  else
    hipLaunchKernelGGL(k_round_f32, dim3(grid), dim3(256), 0, c->stream, (const double *)src, lds, sstride, (float *)dst, ldd, dstride,
                       rows, cols, batch);
  LAUNCHCHECK();
  return DHQR_OK;
}

static inline size_t f32_even(size_t n) { return (n + 1) & ~(size_t)1; }
// The Float64 workspace of the promoted tier (c->f32_ws), packed: matrices (lda = m, matrix k at k m n) | alphas (n per
// matrix) | right-hand sides (an m x nrhs block per matrix; nrhs = 0: none), each section starting on an even element
// (16-byte boundaries, like separately allocated arrays).
struct F32Ws {
  double *A, *alpha, *B;
};
static int32_t f32_ws_get(dhqr_ctx *c, int64_t m, int64_t n, int64_t nrhs, int64_t batch, F32Ws &w) {
  const size_t na = (size_t)m * (size_t)n * (size_t)batch, nal = (size_t)n * (size_t)batch;
  const size_t nB = (size_t)m * (size_t)nrhs * (size_t)batch;
  CHECK(ensure(c, c->f32_ws, f32_even(na) + (nB ? f32_even(nal) + nB : nal)));
  w.A = c->f32_ws.p;
  w.alpha = w.A + f32_even(na);
  w.B = w.alpha + f32_even(nal);
  return DHQR_OK;
}
// The promoted tier: widen, call(w) -- the Float64 route on the workspace --, round back, synchronise where `sync` says.
// dB == nullptr: a factorisation (A in; A and alpha out).  Else a solve (A, alpha and the m x nrhs blocks of B in; B out);
// dalpha == nullptr: an application of Q (no alpha: A and B in, B out); b_in = false: the explicit Q (A in, B out).
template <typename Call>
static int32_t f32_promoted(dhqr_ctx *c, const float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const float *dalpha,
                            int64_t stride_alpha, float *dB, int64_t nrhs, int64_t ldb, int64_t strideB, int64_t batch, bool sync,
                            Call call, bool b_in = true) {
  F32Ws w;
  CHECK(f32_ws_get(c, m, n, dB ? nrhs : 0, batch, w));
  if (dB && c->tc_A == w.A) c->tc_valid = false;  // the caller's factor is widened afresh: nothing kept applies to it
  CHECK(f32_convert_launch(c, true, dA, lda, strideA, w.A, m, m * n, m, n, batch));
  if (dB) {
    if (dalpha) CHECK(f32_convert_launch(c, true, dalpha, n, stride_alpha, w.alpha, n, n, n, 1, batch));
    if (b_in) CHECK(f32_convert_launch(c, true, dB, ldb, strideB, w.B, m, m * nrhs, m, nrhs, batch));
  }
  CHECK(call(w));
  if (dB) {
    CHECK(f32_convert_launch(c, false, w.B, m, m * nrhs, dB, ldb, strideB, m, nrhs, batch));
  } else {  // (a factorisation's A and alpha are the caller's own, writable arrays)
    CHECK(f32_convert_launch(c, false, w.A, m, m * n, const_cast<float *>(dA), lda, strideA, m, n, batch));
    CHECK(f32_convert_launch(c, false, w.alpha, n, n, const_cast<float *>(dalpha), n, stride_alpha, n, 1, batch));
  }
  if (sync) HIPCHECK(hipStreamSynchronize(c->stream));
  return DHQR_OK;
}

// `single`: the promoted tier calls dhqr_factor_f64 / dhqr_solve_f64 (else the batched routes above)
static int32_t factor_batched(dhqr_ctx *c, float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, float *dalpha,
                              int64_t stride_alpha, int64_t batch, int32_t nb, bool single) {
  // (tc_valid / retry stay: what they remember are Float64 buffers, which a Float32 factorisation cannot overwrite -- the
  // promoted tier's workspace goes through dhqr_factor_f64, which resets them itself)
  if (batched_wave_fit(c, m, n)) return wave_factor(c, dA, m, n, lda, strideA, dalpha, stride_alpha, batch);
  // synchronous where the Float64 route is: the blocked driver of a single matrix, the serial tier of a batch
  const bool sync = small_qr_fit(c, m, n) < 0 && (!single || nb != 0);
  return f32_promoted(c, dA, m, n, lda, strideA, dalpha, stride_alpha, nullptr, 0, 0, 0, batch, sync, [&](const F32Ws &w) {
    return single ? dhqr_factor_f64(c, w.A, m, n, m, w.alpha, nb) : factor_batched(c, w.A, m, n, m, m * n, w.alpha, n, batch, nb);
  });
}

static int32_t solve_batched(dhqr_ctx *c, const float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const float *dalpha,
                             int64_t stride_alpha, float *db, int64_t strideb, int64_t batch, bool single) {
  if (batched_wave_fit(c, m, n)) return wave_solve(c, dA, m, n, lda, strideA, dalpha, stride_alpha, db, strideb, batch);
  const bool sync = !single && !small_ldiv_fit(c, m, n);  // (the serial tier of a batch)
  return f32_promoted(c, dA, m, n, lda, strideA, dalpha, stride_alpha, db, 1, m, strideb, batch, sync, [&](const F32Ws &w) -> int32_t {
    CHECK(single ? dhqr_solve_f64(c, w.A, m, n, m, w.alpha, w.B) : solve_batched(c, w.A, m, n, m, m * n, w.alpha, n, w.B, m, batch));
    if (single && c->retry.valid && c->retry.b == w.B) {  // (a flag left by an earlier Float64 solve names another b)
      // THIS solve took the persistent Q'b kernel and may be REPEATED by the next synchronising entry point (dhqr.h:
      // dhqr_get_solve_retries) -- into the workspace, behind the rounding enqueued next.  Settle it first; afterwards nothing
      // may come back to the remembered pointers: they lie in a workspace that a later call may reallocate.
      HIPCHECK(hipStreamSynchronize(c->stream));
      const int32_t rc = pipe_error_check(c);
      c->retry.valid = false;
      CHECK(rc);
    }
    return DHQR_OK;
  });
}

// The native multi-column kernel on the wave tier where it pays, the native single-column kernel column by column where
// it does not; everything else PROMOTED once -- factor, alpha and all of B widened into the Float64 workspace, the Float64
// route above, B rounded back.
static int32_t solve_batched_nrhs(dhqr_ctx *c, const float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const float *dalpha,
                                  int64_t stride_alpha, float *dB, int64_t nrhs, int64_t ldb, int64_t strideB, int64_t batch) {
  if (batched_wave_fit(c, m, n)) {
    if (nrhs_wave_pays<float>(nrhs, n))
      return wave_solve_nrhs(c, dA, m, n, lda, strideA, dalpha, stride_alpha, dB, nrhs, ldb, strideB, batch);
    for (int64_t r = 0; r < nrhs; ++r)
      CHECK(wave_solve(c, dA, m, n, lda, strideA, dalpha, stride_alpha, dB + r * ldb, strideB, batch));
    return DHQR_OK;
  }
  const bool sync = !small_ldiv_fit(c, m, n);  // (the serial tier)
  return f32_promoted(c, dA, m, n, lda, strideA, dalpha, stride_alpha, dB, nrhs, ldb, strideB, batch, sync, [&](const F32Ws &w) {
    return solve_batched_nrhs(c, w.A, m, n, m, m * n, w.alpha, n, w.B, nrhs, m, m * nrhs, batch);
  });
}

// ---- ComplexF64 beyond the wave tier, up to 128 rows: one workgroup per (matrix, group of columns of B) --------------------
static inline bool small_zfit(const dhqr_ctx *c, int64_t m, int64_t n);  // (the one-workgroup tier's shape rule, below)
static inline bool small_znrhs_fit(const dhqr_ctx *c, int64_t m, int64_t n) { return !batched_wave_fit(c, m, n) && small_zfit(c, m, n); }
static inline int64_t small_zapply_groups(int64_t nrhs) { return (nrhs + SMZA_CW - 1) / SMZA_CW; }
// ONE launch of k_small_zapply<mode> on a 1-D grid of batch * groups (the caller has checked that it fits), one n_solve
// group whatever nrhs and batch.  dalpha: SMZA_SOLVE alone (else nullptr).
static int32_t small_zapply(dhqr_ctx *c, int mode, const double2 *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                            const double2 *dalpha, int64_t stride_alpha, double2 *dB, int64_t nrhs, int64_t ldb, int64_t strideB,
                            int64_t batch) {
  CHECK(prof_begin(c, CAT_SOLVE));
  const int64_t groups = small_zapply_groups(nrhs);
  const dim3 grid((unsigned)(batch * groups)), block(SMZA_THREADS);
#define SMZA_LAUNCH(mode_)                                                                                                        \
  hipLaunchKernelGGL(k_small_zapply<mode_>, grid, block, 0, c->stream, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, dB, \
                     (int)nrhs, ldb, strideB, (int)groups)
  switch (mode) {
    case SMZA_SOLVE: SMZA_LAUNCH(SMZA_SOLVE); break;
    case SMZA_QH: SMZA_LAUNCH(SMZA_QH); break;
    case SMZA_QN: SMZA_LAUNCH(SMZA_QN); break;
    default: SMZA_LAUNCH(SMZA_FORMQ);
  }
#undef SMZA_LAUNCH
  LAUNCHCHECK();
  return prof_end(c);
}

// ---- Q application, explicit Q and R (dhqr.h: dhqr_apply_q_batched_f64 ...) -----------------------------------------------
// The wave tier: one launch.  Every other shape, Float64: matrix after matrix on apply_q_impl, the blocked route of
// dhqr_apply_q_f64 (its bits) -- the explicit Q from [I; 0] --, all of it enqueued on the stream; Float32: PROMOTED.
template <typename T>
static int32_t apply_q_batched(dhqr_ctx *c, const T *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, T *dB, int64_t nrhs,
                               int64_t ldb, int64_t strideB, int64_t batch, int trans, bool formq) {
  if (batched_wave_fit(c, m, n)) return wave_apply_q(c, dA, m, n, lda, strideA, dB, nrhs, ldb, strideB, batch, trans, formq);
  if constexpr (std::is_same_v<T, double2>) {
    // ComplexF64 has no blocked apply-Q.  Beyond 128 rows and with the small route off: [I; 0] for the explicit Q, then ONE
    // launch of the plain kernel, a workgroup per (matrix, column of B) on a 1-D grid (batch * nrhs may exceed a y dimension)
    if (batch * nrhs > 0x7fffffffLL) return set_err(DHQR_EINVAL, "batch * nrhs = %lld too large", (long long)(batch * nrhs));
    // Up to 128 rows: the one-workgroup kernel, which reads the factor once per SMZA_CW columns and carries a column in
    // double-double as every other ComplexF64 kernel of the family does.  By SHAPE alone, never by nrhs or batch: the two
    // kernels round differently, and a column's bits may not depend on its neighbours.  Measured, batch 16384
    // (profiles/small_c64_nrhs_throughput.txt): the explicit Q is 1.46 - 1.71 x the general kernel; Q^H B and Q B are NOT
    // faster -- 0.81 - 0.91 x at 66 x 33 in every round, 0.97 - 1.02 x at 110 x 100 and 128 x 128 -- and take this kernel for
    // the contracts above, which the general kernel cannot give.  (DHQR_TUNE zsmall_nrhs=0: the general kernel.)
    if (small_znrhs_fit(c, m, n) && c->zsmall_nrhs != 0)
      return small_zapply(c, formq ? SMZA_FORMQ : trans ? SMZA_QH : SMZA_QN, dA, m, n, lda, strideA, nullptr, 0, dB, nrhs, ldb, strideB,
                          batch);
    if (formq) {
      const int64_t total = m * nrhs * batch;
      hipLaunchKernelGGL(k_batched_eye<double2>, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32)), dim3(256), 0, c->stream,
                         dB, ldb, strideB, m, nrhs, batch);
      LAUNCHCHECK();
    }
    CHECK(prof_begin(c, CAT_SOLVE));
    const dim3 grid((unsigned)(batch * nrhs)), block(BQZG_THREADS);
    if (trans)
      hipLaunchKernelGGL(k_batched_zapplyq_general<1>, grid, block, 0, c->stream, dA, lda, strideA, m, n, dB, nrhs, ldb, strideB);
    else
      hipLaunchKernelGGL(k_batched_zapplyq_general<0>, grid, block, 0, c->stream, dA, lda, strideA, m, n, dB, nrhs, ldb, strideB);
    LAUNCHCHECK();
    return prof_end(c);
  } else if constexpr (std::is_same_v<T, double>) {
    CHECK(check_mat(dB, m, nrhs, ldb, false));  // (the blocked route's limit on a leading dimension; dA: check_batch)
    if (formq) {
      const int64_t total = m * nrhs * batch;
      hipLaunchKernelGGL(k_batched_eye<double>, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32)), dim3(256), 0, c->stream, dB,
                         ldb, strideB, m, nrhs, batch);
      LAUNCHCHECK();
    }
    for (int64_t k = 0; k < batch; ++k)
      CHECK(apply_q_impl(c, dA + k * strideA, m, n, lda, nullptr, dB + k * strideB, nrhs, ldb, trans, false));
    return DHQR_OK;
  } else {
    return f32_promoted(
        c, dA, m, n, lda, strideA, nullptr, 0, dB, nrhs, ldb, strideB, batch, false,
        [&](const F32Ws &w) { return apply_q_batched(c, w.A, m, n, m, m * n, w.B, nrhs, m, m * nrhs, batch, trans, formq); }, !formq);
  }
}

// one element-wise launch for every shape and every element type (copies: nothing to promote)
template <typename T>
static int32_t form_r_batched(dhqr_ctx *c, const T *dA, int64_t n, int64_t lda, int64_t strideA, const T *dalpha, int64_t stride_alpha,
                              T *dR, int64_t ldr, int64_t strideR, int64_t batch) {
  const int64_t total = n * n * batch;
  hipLaunchKernelGGL(k_batched_form_r<T>, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32)), dim3(256), 0, c->stream, dA,
                     lda, strideA, n, dalpha, stride_alpha, dR, ldr, strideR, batch);
  LAUNCHCHECK();
  return DHQR_OK;
}

// ---- ComplexF64 on the device: the wave tier | one workgroup per matrix | matrix after matrix ------------------------------
// The one-workgroup tier (dhqr_small_complex.h): ONE shape rule for single and batched calls alike.  The single-matrix
// entry points (dhqr_factor_c64 ... dhqr_ldiv_c64) call factor_batched / solve_batched below with a batch of one whenever
// it holds, so a single call and a batch of one are the same launch.
static inline bool small_zfit(const dhqr_ctx *c, int64_t m, int64_t n) { return c->small_route && n >= 1 && n <= m && m <= SMZ_MAX; }
// One launch of k_small_zqr, one n_rank1 group whatever the batch.  done != nullptr: a host-array call on the pinned
// staging buffer (small_signal_done).
static int32_t small_zqr(dhqr_ctx *c, const double2 *Asrc, int64_t lds, double2 *Adst, int64_t ldd, int64_t m, int64_t n, double2 *alpha,
                         unsigned long long *done, unsigned long long epoch, const SmallBatch &sb) {
  CHECK(prof_begin(c, CAT_RANK1));
  hipLaunchKernelGGL(k_small_zqr, dim3((unsigned)sb.batch), dim3(SMZ_THREADS), 0, c->stream, Asrc, lds, Adst, ldd, (int)m, (int)n, alpha,
                     done, epoch, sb.strideA, sb.strideA, sb.stride_alpha);
  LAUNCHCHECK();
  if (c->profiling)  // (as the wave tier counts: an element update reads and writes one complex element)
    for (int64_t j = 0; j + 1 < n; ++j) c->st.bytes_rank1 += (double)sb.batch * 32.0 * (double)(m - j) * (double)(n - j - 1);
  return prof_end(c);
}
// One launch of k_small_zldiv, one n_solve whatever the batch.  Awork: device memory for a factor that lies in pinned host
// memory (else nullptr).
static int32_t small_zldiv(dhqr_ctx *c, const double2 *A, int64_t lda, int64_t m, int64_t n, const double2 *alpha, const double2 *bin,
                           double2 *bout, double2 *xout, double2 *Awork, unsigned long long *done, unsigned long long epoch,
                           const SmallBatch &sb) {
  CHECK(prof_begin(c, CAT_SOLVE));
  hipLaunchKernelGGL(k_small_zldiv, dim3((unsigned)sb.batch), dim3(SML_THREADS), 0, c->stream, A, lda, (int)m, (int)n, alpha, bin, bout,
                     xout, Awork, done, epoch, sb.strideA, sb.stride_alpha, sb.strideb);
  LAUNCHCHECK();
  return prof_end(c);
}

// (lda and the strides count complex elements; nb was checked by the caller: 0 or DHQR_ZNB, ignored on the first two tiers)
static int32_t factor_batched(dhqr_ctx *c, double2 *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, double2 *dalpha,
                              int64_t stride_alpha, int64_t batch, int32_t nb, bool /*single*/ = false) {
  const bool wave = batched_wave_fit(c, m, n);
  if (!wave && small_zfit(c, m, n))  // workgroup k on matrix k: asynchronous, one launch
    return small_zqr(c, dA, lda, dA, lda, m, n, dalpha, nullptr, 0, SmallBatch{batch, strideA, stride_alpha});
  if (!wave) {  // serial: that call's bits and profiling counts, synchronised after each (see Float64)
    for (int64_t k = 0; k < batch; ++k) {
      CHECK(dhqr_factor_c64_nb(c, reinterpret_cast<double *>(dA + k * strideA), m, n, lda,
                               reinterpret_cast<double *>(dalpha + k * stride_alpha), nb));
      HIPCHECK(hipStreamSynchronize(c->stream));
      CHECK(pipe_error_check(c));
    }
    return DHQR_OK;
  }
  // (tc_valid / retry stay, as in dhqr_factor_c64: what they remember are Float64 factors and solves)
  CHECK(prof_begin(c, CAT_RANK1));  // ONE launch, one group
  WAVE_LAUNCH(k_batched_zqr_wave, n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, batch);
  if (c->profiling)  // (an element update reads and writes one complex element)
    for (int64_t j = 0; j + 1 < n; ++j) c->st.bytes_rank1 += (double)batch * 32.0 * (double)(m - j) * (double)(n - j - 1);
  return prof_end(c);
}

static int32_t solve_batched(dhqr_ctx *c, const double2 *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const double2 *dalpha,
                             int64_t stride_alpha, double2 *db, int64_t strideb, int64_t batch, bool /*single*/ = false) {
  const bool wave = batched_wave_fit(c, m, n);
  if (!wave && small_zfit(c, m, n))  // (the factor is in device memory: no Awork)
    return small_zldiv(c, dA, lda, m, n, dalpha, db, db, nullptr, nullptr, nullptr, 0, SmallBatch{batch, strideA, stride_alpha, strideb});
  if (!wave) {
    for (int64_t k = 0; k < batch; ++k) {
      CHECK(dhqr_solve_c64(c, reinterpret_cast<const double *>(dA + k * strideA), m, n, lda,
                           reinterpret_cast<const double *>(dalpha + k * stride_alpha), reinterpret_cast<double *>(db + k * strideb)));
      HIPCHECK(hipStreamSynchronize(c->stream));
      CHECK(pipe_error_check(c));
    }
    return DHQR_OK;
  }
  CHECK(prof_begin(c, CAT_SOLVE));
  WAVE_LAUNCH(k_batched_zldiv_wave, n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, db, strideb, batch);
  return prof_end(c);
}

// Does the complex multi-column kernel pay?  Measured on the MI355X (profiles/batched_c64_nrhs_throughput.txt: batch 16384,
// resident factor, 16 x 8 / 40 x 17 / 64 x 32, groups of BQZN_RG = 1 / 2 / 4, K = 2, 4, 8, 16 columns, five rounds of ten
// repetitions; the kernel over the loop of K dhqr_solve_batched_c64 calls, round by round).  Its time goes by GROUPS, like
// the real kernel's: a group costs 0.92 / 1.8 / 3.5 single-column solves, whether its columns are real or the zeros of a
// tail.  K = 2 is 1.01 - 1.04 x at 16 x 8 -- inside the 3 % the ratio moves from round to round -- and 0.55 - 0.56 x at
// the other two shapes; K = 4, 8 and 16, all of them full groups, win at every shape and in every round: 1.04 - 1.08 x,
// 1.07 - 1.12 x, 1.09 - 1.15 x (the first round of a process at the two smaller shapes, 1.01 - 1.06 x, aside).  No call with a tail group was measured.
// So: the kernel for at least four columns in full groups, the column loop -- the same bits -- for every other call.
// (DHQR_TUNE znrhs_wave=1 / 0: always the kernel / the loop, for measurements and for the tests of the tail groups.)
static inline bool znrhs_wave_pays(int64_t nrhs, int64_t n) { return nrhs >= 4 && nrhs % BQZN_RG(wave_nc(n)) == 0; }

// Does the one-workgroup multi-column kernel (k_small_zapply<SMZA_SOLVE>) pay against the loop of nrhs k_small_zldiv launches?
// Measured on the MI355X (profiles/small_c64_nrhs_throughput.txt: batch 16384, resident factor, 66 x 33 / 110 x 100 /
// 128 x 128, K = 2, 4, 8, 16 columns, one process per arm -- DHQR_TUNE zsmall_nrhs=1 against zsmall_nrhs=0 --, five rounds
// of ten repetitions, round by round; ratios move by up to 3 % from round to round).  ONE group of SMZA_CW = 6 columns wins
// in every round: K = 2 1.05 - 1.09 x, K = 4 1.56 - 1.67 x.  THREE groups (K = 16: 6 + 6 + 4) win in every round: 1.34 -
// 1.47 x; a batch of one at 110 x 100 with 16 columns takes 202 us instead of 1815 us.  TWO groups (K = 8: 6 + 2) LOSE in
// every round at every shape, 0.81 - 0.92 x: the second launch-worth of workgroups costs more than its columns' share,
// which the measurement shows and does not explain.  No other number of groups was measured.  So: the kernel for 2 .. 6 and
// for 13 .. 18 columns, the column loop -- the same bits -- for every other call.
// (DHQR_TUNE zsmall_nrhs=1 / 0: always the kernel / always the routes without it, for measurements and tests.)
static inline bool zsmall_nrhs_pays(int64_t nrhs) {
  const int64_t groups = small_zapply_groups(nrhs);
  return nrhs >= 2 && (groups == 1 || groups == 3);
}

// The wave tier and the one-workgroup tier where they pay: their multi-column kernels.  Every other call: the single-column
// route, column by column -- its tiers, its synchronisation, its profiling counts, its bits (a column of complex elements
// stays 16-byte aligned).
static int32_t solve_batched_nrhs(dhqr_ctx *c, const double2 *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                  const double2 *dalpha, int64_t stride_alpha, double2 *dB, int64_t nrhs, int64_t ldb, int64_t strideB,
                                  int64_t batch) {
  if (batched_wave_fit(c, m, n) && (c->znrhs_wave < 0 ? znrhs_wave_pays(nrhs, n) : c->znrhs_wave != 0))
    return wave_solve_nrhs(c, dA, m, n, lda, strideA, dalpha, stride_alpha, dB, nrhs, ldb, strideB, batch);
  // (a grid of batch * groups workgroups that does not fit a launch: the column loop, the same bits)
  if (small_znrhs_fit(c, m, n) && (c->zsmall_nrhs < 0 ? zsmall_nrhs_pays(nrhs) : c->zsmall_nrhs != 0) &&
      batch * small_zapply_groups(nrhs) <= 0x7fffffffLL)
    return small_zapply(c, SMZA_SOLVE, dA, m, n, lda, strideA, dalpha, stride_alpha, dB, nrhs, ldb, strideB, batch);
  for (int64_t r = 0; r < nrhs; ++r)
    CHECK(solve_batched(c, dA, m, n, lda, strideA, dalpha, stride_alpha, dB + r * ldb, strideB, batch));
  return DHQR_OK;
}

// ---- the host forms ------------------------------------------------------------------------------------------------------
// the packed device staging area of the host forms, `count` elements of T: matrices | alphas | right-hand sides
template <typename T>
static int32_t staging(dhqr_ctx *c, size_t count, T *&d) {
  Buf &buf = std::is_same_v<T, float> ? c->f32_dev : c->batch_dev;  // (both buffers count doubles; double2: batch_dev)
  CHECK(ensure(c, buf, (count * sizeof(T) + sizeof(double) - 1) / sizeof(double)));
  d = reinterpret_cast<T *>(buf.p);
  return DHQR_OK;
}
// host <-> device copies of `batch` blocks of rows x cols elements: block k at h + k hstride (leading dimension hld) and at
// d + k dstride (leading dimension dld)
template <typename T>
static int32_t batch_copy(dhqr_ctx *c, T *d, int64_t dld, int64_t dstride, const T *h, int64_t hld, int64_t hstride, int64_t rows,
                          int64_t cols, int64_t batch, bool up) {
  auto copy2d = [&](T *dp, const T *hp, int64_t dpitch, int64_t hpitch, int64_t width, int64_t height) -> int32_t {
    if (up)
      HIPCHECK(hipMemcpy2DAsync(dp, dpitch * sizeof(T), hp, hpitch * sizeof(T), width * sizeof(T), height, hipMemcpyHostToDevice,
                                c->stream));
    else
      HIPCHECK(hipMemcpy2DAsync(const_cast<T *>(hp), hpitch * sizeof(T), dp, dpitch * sizeof(T), width * sizeof(T), height,
                                hipMemcpyDeviceToHost, c->stream));
    return DHQR_OK;
  };
  // (for X the first path also takes nrhs = 1, and m = n with ldx = n, which the parent's two X paths -- the next two lines --
  // sent through a column-pitch copy or the per-matrix loop: the same bytes in one copy)
  if (cols == 1 || (hld == rows && dld == rows))  // every block contiguous
    return copy2d(d, h, dstride, hstride, rows * cols, batch);
  if ((hstride == hld * cols && dstride == dld * cols) || batch == 1)  // one column pitch throughout
    return copy2d(d, h, dld, hld, rows, cols * batch);
  for (int64_t k = 0; k < batch; ++k) CHECK(copy2d(d + k * dstride, h + k * hstride, dld, hld, rows, cols));
  return DHQR_OK;
}
// the packed form of the staging area: leading dimension = rows, block k at k rows cols
template <typename T>
static int32_t batch_copy(dhqr_ctx *c, T *d, const T *h, int64_t rows, int64_t cols, int64_t hld, int64_t hstride, int64_t batch,
                          bool up) {
  return batch_copy(c, d, rows, rows * cols, h, hld, hstride, rows, cols, batch, up);
}
// what every host form ends with: the stream drained whatever happened (rc: the first error so far), then the bounded waits'
// error word (a synchronous entry point reports it itself, after repeating a solve that has to be: dhqr.h)
static int32_t host_finish(dhqr_ctx *c, int32_t rc, bool pipe_check) {
  if (hipStreamSynchronize(c->stream) != hipSuccess && rc == DHQR_OK) rc = set_err(DHQR_EHIP, "hipStreamSynchronize failed");
  if (pipe_check && rc == DHQR_OK) rc = pipe_error_check(c);
  return rc;
}

template <typename T>
static int32_t qr_host(dhqr_ctx *c, T *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, T *halpha, int64_t stride_alpha,
                       int64_t batch, int32_t nb, bool single) {
  const size_t na = (size_t)m * (size_t)n * (size_t)batch, nal = (size_t)n * (size_t)batch;
  T *dA;
  CHECK(staging(c, na + nal, dA));
  T *dal = dA + na;
  int32_t rc = batch_copy(c, dA, hA, m, n, lda, strideA, batch, true);
  if (rc == DHQR_OK) rc = factor_batched(c, dA, m, n, m, m * n, dal, n, batch, nb, single);
  if (rc == DHQR_OK) rc = batch_copy(c, dA, hA, m, n, lda, strideA, batch, false);
  if (rc == DHQR_OK) rc = batch_copy(c, dal, halpha, n, 1, n, stride_alpha, batch, false);
  return host_finish(c, rc, true);
}

// nrhs columns per matrix: B_k at hB + k strideB (leading dimension ldb), X_k likewise.  `multi`: the _nrhs entry points,
// through the multi-column solve; else nrhs = 1, ldb = m, ldx = n, through the single-column solve.
constexpr bool SINGLE = true, BATCH = false;              // `single` of qr_host / ldiv_host / factor_batched / solve_batched
constexpr bool MULTI_COLUMN = true, ONE_COLUMN = false;   // `multi` of ldiv_host
template <typename T>
static int32_t ldiv_host(dhqr_ctx *c, const T *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const T *halpha,
                         int64_t stride_alpha, const T *hB, int64_t nrhs, int64_t ldb, int64_t strideB, T *hX, int64_t ldx,
                         int64_t strideX, int64_t batch, bool single, bool multi) {
  const size_t na = (size_t)m * (size_t)n * (size_t)batch, nal = (size_t)n * (size_t)batch;
  T *dA;
  CHECK(staging(c, na + nal + (size_t)m * (size_t)nrhs * (size_t)batch, dA));
  T *dal = dA + na, *dB = dal + nal;
  int32_t rc = batch_copy(c, dA, hA, m, n, lda, strideA, batch, true);
  if (rc == DHQR_OK) rc = batch_copy(c, dal, halpha, n, 1, n, stride_alpha, batch, true);
  if (rc == DHQR_OK) rc = batch_copy(c, dB, hB, m, nrhs, ldb, strideB, batch, true);  // src:318 copy of B
  if (rc == DHQR_OK)
    rc = multi ? solve_batched_nrhs(c, dA, m, n, m, m * n, dal, n, dB, nrhs, m, m * nrhs, batch)
               : solve_batched(c, dA, m, n, m, m * n, dal, n, dB, m, batch, single);
  if (rc == DHQR_OK) rc = host_finish(c, rc, true);  // (the serial tier's solves may have been repeated: dhqr.h)
  if (rc == DHQR_OK)  // src:320: X_k = the first n rows of B_k
    rc = batch_copy(c, dB, m, m * nrhs, hX, ldx, strideX, n, nrhs, batch, false);
  return host_finish(c, rc, false);
}

// ---- column-pivoted QR, the rank, the rank-truncated solve (dhqr.h: dhqr_factor_batched_pivoted_f64 ...), written once for
// T = double, float and double2 (ComplexF64; lda and the strides count complex elements) -------------------------------------
// Float64, ComplexF64.  Wave tier: ONE launch of the kernels of dhqr_batched_pivoted.h / dhqr_batched_complex_pivoted.h; every
// other shape, and every shape with the small route off: ONE launch of their general forms, a workgroup per matrix / per
// (matrix, column of B).  Float32: the wave tier natively (the same kernels with T = float); everything else PROMOTED --
// widened into the Float64 workspace, the Float64 route (its jpvt, written straight into the caller's), rounded back.
static int32_t check_pivoted(const void *jpvt, int64_t n, int64_t stride_jpvt) {
  if (!jpvt) return set_err(DHQR_EINVAL, "null jpvt pointer");
  if (stride_jpvt < n) return set_err(DHQR_EINVAL, "stride_jpvt %lld < n=%lld", (long long)stride_jpvt, (long long)n);
  return DHQR_OK;
}
template <typename T>
static int32_t factor_batched_pivoted(dhqr_ctx *c, T *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, T *dalpha,
                                      int64_t stride_alpha, int32_t *djpvt, int64_t stride_jpvt, int64_t batch) {
  const bool wave = batched_wave_fit(c, m, n);
  if constexpr (std::is_same_v<T, float>) {
    if (!wave)
      return f32_promoted(c, dA, m, n, lda, strideA, dalpha, stride_alpha, nullptr, 0, 0, 0, batch, false, [&](const F32Ws &w) {
        return factor_batched_pivoted(c, w.A, m, n, m, m * n, w.alpha, n, djpvt, stride_jpvt, batch);
      });
  }
  if constexpr (std::is_same_v<T, double>) {
    c->tc_valid = false;  // whatever was kept for one of these matrices is gone
    c->retry.valid = false;
  }
  CHECK(prof_begin(c, CAT_RANK1));  // ONE launch, one group
  if (wave) {
    if constexpr (std::is_same_v<T, double2>)
      WAVE_LAUNCH(k_batched_zqrp_wave, n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, djpvt, stride_jpvt, batch);
    else
      WAVE_LAUNCH_T(k_batched_qrp_wave, WAVE_TARGS(T), n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, djpvt,
                    stride_jpvt, batch);
  } else if constexpr (std::is_same_v<T, double2>) {
    hipLaunchKernelGGL(k_batched_zqrp_general, dim3((unsigned)batch), dim3(BQPG_THREADS), 0, c->stream, dA, lda, strideA, m, n, dalpha,
                       stride_alpha, djpvt, stride_jpvt);
    LAUNCHCHECK();
  } else if constexpr (std::is_same_v<T, double>) {
    hipLaunchKernelGGL(k_batched_qrp_general, dim3((unsigned)batch), dim3(BQPG_THREADS), 0, c->stream, dA, lda, strideA, m, n, dalpha,
                       stride_alpha, djpvt, stride_jpvt);
    LAUNCHCHECK();
  }
  if (c->profiling)  // (the update's traffic, as the unpivoted factor counts it; the pivot search reads as much again)
    for (int64_t j = 0; j + 1 < n; ++j)
      c->st.bytes_rank1 += (double)batch * (double)(2 * sizeof(T)) * (double)(m - j) * (double)(n - j - 1);
  return prof_end(c);
}
// one element-wise launch, not counted.  rcond < 0: max(m, n) eps(T) -- 2^-52 for Float64 and ComplexF64, 2^-23 for Float32
template <typename T>
static int32_t rank_batched(dhqr_ctx *c, const T *dalpha, int64_t m, int64_t n, int64_t stride_alpha, double rcond, int32_t *drank,
                            int64_t batch) {
  const double rc = rcond >= 0.0 ? rcond : (double)std::max(m, n) * (std::is_same_v<T, float> ? 0x1p-23 : 0x1p-52);
  hipLaunchKernelGGL(k_batched_rank<T>, dim3((unsigned)std::min<int64_t>((batch + 255) / 256, 256 * 32)), dim3(256), 0, c->stream, dalpha,
                     n, stride_alpha, rc, drank, batch);
  LAUNCHCHECK();
  return DHQR_OK;
}
template <typename T>
static int32_t solve_batched_pivoted(dhqr_ctx *c, const T *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const T *dalpha,
                                     int64_t stride_alpha, const int32_t *djpvt, int64_t stride_jpvt, const int32_t *drank, T *dB,
                                     int64_t nrhs, int64_t ldb, int64_t strideB, T *dX, int64_t ldx, int64_t strideX, int64_t batch) {
  const bool wave = batched_wave_fit(c, m, n);
  if (!wave && batch * nrhs > 0x7fffffffLL) return set_err(DHQR_EINVAL, "batch * nrhs = %lld too large", (long long)(batch * nrhs));
  if constexpr (std::is_same_v<T, float>) {
    if (!wave) {
      // PROMOTED.  The workspace: matrices | alphas | B | X, packed, each section on an even element.  X is widened too: the
      // entries the Float64 route does not write (a jpvt entry out of range) keep the caller's values through the rounding.
      const size_t na = (size_t)m * (size_t)n * (size_t)batch, nal = (size_t)n * (size_t)batch;
      const size_t nB = (size_t)m * (size_t)nrhs * (size_t)batch, nX = (size_t)n * (size_t)nrhs * (size_t)batch;
      CHECK(ensure(c, c->f32_ws, f32_even(na) + f32_even(nal) + f32_even(nB) + nX));
      double *wA = c->f32_ws.p, *wal = wA + f32_even(na), *wB = wal + f32_even(nal), *wX = wB + f32_even(nB);
      if (c->tc_A == wA) c->tc_valid = false;  // the caller's factor is widened afresh: nothing kept applies to it
      CHECK(f32_convert_launch(c, true, dA, lda, strideA, wA, m, m * n, m, n, batch));
      CHECK(f32_convert_launch(c, true, dalpha, n, stride_alpha, wal, n, n, n, 1, batch));
      CHECK(f32_convert_launch(c, true, dB, ldb, strideB, wB, m, m * nrhs, m, nrhs, batch));
      CHECK(f32_convert_launch(c, true, dX, ldx, strideX, wX, n, n * nrhs, n, nrhs, batch));
      CHECK(solve_batched_pivoted(c, (const double *)wA, m, n, m, m * n, (const double *)wal, n, djpvt, stride_jpvt, drank, wB, nrhs, m,
                                  m * nrhs, wX, n, n * nrhs, batch));
      CHECK(f32_convert_launch(c, false, wB, m, m * nrhs, dB, ldb, strideB, m, nrhs, batch));
      return f32_convert_launch(c, false, wX, n, n * nrhs, dX, ldx, strideX, n, nrhs, batch);
    }
  }
  CHECK(prof_begin(c, CAT_SOLVE));  // ONE launch, one group, whatever nrhs and batch
  if (wave) {
    if constexpr (std::is_same_v<T, double2>)
      WAVE_LAUNCH(k_batched_zldivp_wave, n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, djpvt, stride_jpvt, drank, dB,
                  (int)nrhs, ldb, strideB, dX, ldx, strideX, batch);
    else
      WAVE_LAUNCH_T(k_batched_ldivp_wave, WAVE_TARGS(T), n, batch, dA, lda, strideA, (int)m, (int)n, dalpha, stride_alpha, djpvt,
                    stride_jpvt, drank, dB, (int)nrhs, ldb, strideB, dX, ldx, strideX, batch);
  } else if constexpr (std::is_same_v<T, double2>) {
    hipLaunchKernelGGL(k_batched_zldivp_general, dim3((unsigned)(batch * nrhs)), dim3(BQPG_THREADS), 0, c->stream, dA, lda, strideA, m, n,
                       dalpha, stride_alpha, djpvt, stride_jpvt, drank, dB, nrhs, ldb, strideB, dX, ldx, strideX);
    LAUNCHCHECK();
  } else if constexpr (std::is_same_v<T, double>) {
    hipLaunchKernelGGL(k_batched_ldivp_general, dim3((unsigned)(batch * nrhs)), dim3(BQPG_THREADS), 0, c->stream, dA, lda, strideA, m, n,
                       dalpha, stride_alpha, djpvt, stride_jpvt, drank, dB, nrhs, ldb, strideB, dX, ldx, strideX);
    LAUNCHCHECK();
  }
  return prof_end(c);
}

// The host forms.  The staging area (the buffer of dhqr_qr_batched_f64 / _f32; dhqr_trim releases it), in elements of T:
// matrices | alphas | B | X | then the int32 sections jpvt and rank (each padded to a whole element).
static int32_t batch_copy_i32(dhqr_ctx *c, int32_t *d, int32_t *h, int64_t count, int64_t hstride, int64_t batch) {
  HIPCHECK(hipMemcpy2DAsync(h, hstride * sizeof(int32_t), d, count * sizeof(int32_t), count * sizeof(int32_t), batch, hipMemcpyDeviceToHost,
                            c->stream));
  return DHQR_OK;
}
template <typename T>
static inline size_t i32_elems(size_t count) {  // elements of T that hold `count` int32
  return (count * sizeof(int32_t) + sizeof(T) - 1) / sizeof(T);
}
template <typename T>
static int32_t qr_pivoted_host(dhqr_ctx *c, T *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, T *halpha, int64_t stride_alpha,
                               int32_t *hjpvt, int64_t stride_jpvt, int64_t batch) {
  const size_t na = (size_t)m * (size_t)n * (size_t)batch, nal = (size_t)n * (size_t)batch;
  T *dA;
  CHECK(staging(c, na + nal + i32_elems<T>(nal), dA));
  T *dal = dA + na;
  int32_t *djp = reinterpret_cast<int32_t *>(dal + nal);
  int32_t rc = batch_copy(c, dA, hA, m, n, lda, strideA, batch, true);
  if (rc == DHQR_OK) rc = factor_batched_pivoted(c, dA, m, n, m, m * n, dal, n, djp, n, batch);
  if (rc == DHQR_OK) rc = batch_copy(c, dA, hA, m, n, lda, strideA, batch, false);
  if (rc == DHQR_OK) rc = batch_copy(c, dal, halpha, n, 1, n, stride_alpha, batch, false);
  if (rc == DHQR_OK) rc = batch_copy_i32(c, djp, hjpvt, n, stride_jpvt, batch);
  return host_finish(c, rc, false);
}
// factor a staged copy, the ranks, the solve; X and the ranks out.  hA and hB are read only.
template <typename T>
static int32_t lstsq_host(dhqr_ctx *c, const T *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const T *hB, int64_t nrhs,
                          int64_t ldb, int64_t strideB, double rcond, T *hX, int64_t ldx, int64_t strideX, int32_t *hrank, int64_t batch) {
  const size_t na = (size_t)m * (size_t)n * (size_t)batch, nal = (size_t)n * (size_t)batch;
  const size_t nB = (size_t)m * (size_t)nrhs * (size_t)batch, nX = (size_t)n * (size_t)nrhs * (size_t)batch;
  T *dA;
  CHECK(staging(c, na + nal + nB + nX + i32_elems<T>(nal) + i32_elems<T>((size_t)batch), dA));
  T *dal = dA + na, *dB = dal + nal, *dX = dB + nB;
  int32_t *djp = reinterpret_cast<int32_t *>(dX + nX);
  int32_t *drk = reinterpret_cast<int32_t *>(dX + nX + i32_elems<T>(nal));
  int32_t rc = batch_copy(c, dA, hA, m, n, lda, strideA, batch, true);
  if (rc == DHQR_OK) rc = batch_copy(c, dB, hB, m, nrhs, ldb, strideB, batch, true);
  if (rc == DHQR_OK) rc = factor_batched_pivoted(c, dA, m, n, m, m * n, dal, n, djp, n, batch);
  if (rc == DHQR_OK) rc = rank_batched(c, (const T *)dal, m, n, n, rcond, drk, batch);
  if (rc == DHQR_OK)
    rc = solve_batched_pivoted(c, (const T *)dA, m, n, m, m * n, (const T *)dal, n, (const int32_t *)djp, n, (const int32_t *)drk, dB, nrhs,
                               m, m * nrhs, dX, n, n * nrhs, batch);
  if (rc == DHQR_OK) rc = batch_copy(c, dX, n, n * nrhs, hX, ldx, strideX, n, nrhs, batch, false);
  if (rc == DHQR_OK) rc = batch_copy_i32(c, drk, hrank, 1, 1, batch);
  return host_finish(c, rc, false);
}
