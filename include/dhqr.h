/*
 * dhqr.h -- C ABI of libdhqr.so: MI355X (gfx950) Householder QR hot path, drop-in for the
 * Julia functions of jwscook/DistributedHouseholderQR.jl (src/DistributedHouseholderQR.jl).
 *
 * The reference has no FFI layer; its boundary is the Julia function API.  Each entry point
 * below names the reference function (file:line) it replaces.  A Julia `ccall` wrapper with the
 * reference's names (`qr!`, `\`, `householder!`, `solve_householder!`, `partialdot`) is in
 * distributedhouseholderqr.jl_amd/julia/src/DistributedHouseholderQR.jl; the same ABI is bound from
 * Python (ctypes) by distributedhouseholderqr.jl_amd/_lib.py.  INTEGRATION.md shows both stubs.
 *
 * Conventions
 *   - plain C, no C++/torch types; every function returns int32 status (0 = DHQR_OK, <0 error),
 *     message via dhqr_last_error() (thread-local); nothing throws across the boundary.
 *   - sizes are int64 (Julia Int); matrices are column-major Float64 with leading dimension ld*.
 *   - "d"-prefixed pointers are DEVICE pointers owned by the caller (hipMalloc, torch tensor
 *     .data_ptr(), AMDGPU.jl ROCArray pointer ...); "h"-prefixed pointers are HOST pointers,
 *     borrowed for the duration of the call.
 *   - device-resident entry points enqueue work on the context's stream and return without
 *     synchronising unless they hand a host scalar back (documented per function).
 *   - one dhqr_ctx per (host thread, GPU); a ctx is not re-entrant.
 *   - a matrix without columns (n == 0, m >= 0) is a no-op for the factor / solve entry points, like the
 *     reference's empty loops (src:127, src:217); m < n, negative sizes and ld < m are DHQR_EINVAL.
 *   - factor format (identical to the reference, src:296-309): after factorisation
 *       A[j:m, j] = v_j  (diagonal INCLUDED, ||v_j||^2 = 2, H_j = I - v_j v_j'),
 *       A[i, j]  = R[i,j] for i < j,   alpha[j] = R[j,j].
 */
#ifndef DHQR_H
#define DHQR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DHQR_VERSION 500 /* 0.5.0: round 6 (dhqr_set_small_route added; nothing else changed); since then added, nothing changed:
                          * dhqr_factor_batched_f64, dhqr_solve_batched_f64, dhqr_qr_batched_f64, dhqr_ldiv_batched_f64;
                          * dhqr_factor_f32, dhqr_solve_f32, dhqr_qr_f32, dhqr_ldiv_f32, dhqr_factor_batched_f32, dhqr_solve_batched_f32,
                          * dhqr_qr_batched_f32, dhqr_ldiv_batched_f32;
                          * dhqr_solve_batched_nrhs_f64, dhqr_ldiv_batched_nrhs_f64, dhqr_solve_batched_nrhs_f32,
                          * dhqr_ldiv_batched_nrhs_f32;
                          * dhqr_factor_batched_c64, dhqr_solve_batched_c64, dhqr_qr_batched_c64, dhqr_ldiv_batched_c64;
                          * the one-workgroup ComplexF64 route up to 128 rows behind the existing dhqr_*_c64 names (no new symbol);
                          * dhqr_factor_batched_pivoted_f64, dhqr_rank_batched_f64, dhqr_solve_batched_pivoted_f64,
                          * dhqr_qr_batched_pivoted_f64, dhqr_lstsq_batched_f64;
                          * the same five for Float32 and ComplexF64: dhqr_factor_batched_pivoted_f32 / _c64, dhqr_rank_batched_f32 / _c64,
                          * dhqr_solve_batched_pivoted_f32 / _c64, dhqr_qr_batched_pivoted_f32 / _c64, dhqr_lstsq_batched_f32 / _c64 */

#define DHQR_OK 0
#define DHQR_EINVAL (-1)   /* bad argument (null pointer, m < n, ld < m, unsupported nb ...) */
#define DHQR_EHIP (-2)     /* a HIP runtime call failed; text in dhqr_last_error() */
#define DHQR_ENOMEM (-3)   /* workspace allocation failed */
#define DHQR_ENODEVICE (-4) /* no gfx950 device visible */
#define DHQR_ECOMM (-5)    /* rank-to-rank transport failed (RCCL error, peer rank failed, callback error) */

/* Panel (block-reflector) width of the blocked path.  BASELINE.json configs 3/4 fix it at 128. */
#define DHQR_NB 128
/* Cyclic block of the 1-D block-cyclic column split (dhqr_cs_*, dhqr_mg_*): TWO panels.  Global column j lives on rank
 * (j / DHQR_CS_BLOCK) % P at local column ((j / DHQR_CS_BLOCK) / P) * DHQR_CS_BLOCK + j % DHQR_CS_BLOCK. */
#define DHQR_CS_BLOCK 256

typedef struct dhqr_ctx dhqr_ctx; /* opaque: device id, stream, workspaces, event pools */

/* Per-phase device timings (ms, hipEvent on the ctx stream) and launch counts accumulated since
 * the last dhqr_reset_stats(); only filled while profiling is enabled (dhqr_set_profiling).
 * Replaces the reference's inline @elapsed accumulators t1a/t1b/t2 (src:126-146, src:291). */
typedef struct dhqr_stats {
  double ms_panel;      /* reflector construction + in-panel rank-1 updates   (src:122-148)  */
  double ms_tbuild;     /* pack V, V'V, T recurrence                           (new)          */
  double ms_gemm_vta;   /* W = V' * A     trailing GEMM 1 (MFMA)               (src:208)      */
  double ms_gemm_tw;    /* W = T' * W     small GEMM (MFMA)                    (new)          */
  double ms_gemm_avw;   /* A -= V * W     trailing GEMM 2 (MFMA)               (src:209)      */
  double ms_rank1;      /* unblocked fused reflector-apply kernel (nb = 0)     (src:198-213)  */
  double ms_solve;      /* Q'b + back substitution                             (src:215-294)  */
  int64_t n_panel, n_tbuild, n_gemm_vta, n_gemm_tw, n_gemm_avw, n_rank1, n_solve; /* launches */
  double flops_gemm_vta, flops_gemm_avw; /* algorithmic flops issued by the two trailing GEMMs */
  double bytes_rank1;                    /* HBM bytes of the nb = 0 launches AS IMPLEMENTED: 16 B per element of every column a
                                          * pass loads and stores once; a pass applies K reflectors (K = 5 where a column
                                          * fits 8192 rows), i.e. 16/K B per trailing element and reflector */
  double bytes_panel;                    /* algorithmic bytes of the panel-lane launches (16 B per element touched) */
} dhqr_stats;

/* ------------------------------------------------------------------ library / context */
int32_t dhqr_version(void);
const char *dhqr_last_error(void);
int32_t dhqr_device_count(int32_t *count);

/* Create a context on HIP device `device` (fails with DHQR_ENODEVICE when no GPU is visible:
 * there is NO CPU fallback).  Owns a stream and lazily grown workspaces. */
int32_t dhqr_create(dhqr_ctx **ctx, int32_t device);
int32_t dhqr_destroy(dhqr_ctx *ctx);
/* Run on the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream).  NULL means the
 * device's default (null) stream -- that IS torch's default stream.  dhqr_use_own_stream switches
 * back to the ctx-owned non-blocking stream (the state after dhqr_create). */
int32_t dhqr_set_stream(dhqr_ctx *ctx, void *hip_stream);
int32_t dhqr_use_own_stream(dhqr_ctx *ctx);
/* Waits for the ctx stream AND reports what only the device knows: the library's inter-workgroup pipelines (the ComplexF64
 * panel pipeline, the lead pipeline of the unblocked path, the flag-pipelined back substitution and the persistent Q'b
 * kernel of dhqr_solve_f64) bound their waits; a wait that expires lets its kernel finish with wrong numbers and records
 * the fact in an error word.  RESULTS OF AN ASYNCHRONOUS ENTRY POINT (dhqr_factor_f64 with nb == 0, dhqr_factor_c64*,
 * dhqr_solve_f64 / _c64, dhqr_cs_factor_c64) ARE VALID ONLY AFTER dhqr_synchronize RETURNED DHQR_OK.  The synchronous
 * entry points and every blocked driver (one status read per pass) check the word themselves. */
int32_t dhqr_synchronize(dhqr_ctx *ctx);
/* Release what the context keeps between calls for speed: the device copy and staging buffers of the host-in / host-out
 * entry points, the solve's workspaces and kept T factors, the blocked driver's group buffers.  Synchronises; the next call
 * that needs them allocates again. */
int32_t dhqr_trim(dhqr_ctx *ctx);
int32_t dhqr_set_profiling(dhqr_ctx *ctx, int32_t on);
int32_t dhqr_reset_stats(dhqr_ctx *ctx);
int32_t dhqr_get_stats(dhqr_ctx *ctx, dhqr_stats *out); /* synchronises the ctx stream */

/* Panels factored since the last dhqr_reset_stats() by the R-first fast path (csrc/dhqr_recon.h)
 * and panels whose verification failed and were redone by the column-by-column path. */
int32_t dhqr_get_panel_counters(dhqr_ctx *ctx, int64_t *n_fast, int64_t *n_fallback);
/* Where the R-first panel path takes its factors from (all drivers): 1 = Gram matrix + Cholesky, reflectors from the
 * panel itself (default), 2 = CholeskyQR2, 3 = TSQR-HR (csrc/dhqr_tsqr.h: 256-row leaves, pairwise reduction of the
 * 128 x 128 R factors -- across the ranks in the row-split driver --, explicit orthonormal Q back down the tree,
 * reflectors from Q: accuracy independent of the panel's condition number).  A panel rejected by the on-device
 * verification climbs the ladder 1 -> 2 (-> 3, see dhqr_set_tsqr_rung; row split: 1 -> 3) before it is redone column
 * by column.  Environment: DHQR_CHOLQR_PASSES=2, DHQR_TSQR=1, DHQR_TSQR_RUNG=0/1.
 * dhqr_get_tsqr_count: accepted panels that went through the tree since the last dhqr_reset_stats(). */
int32_t dhqr_set_r_source(dhqr_ctx *ctx, int32_t source);
/* The TSQR-HR rung of the ladder: on = 1 always, on = 0 never.  Default (neither called nor DHQR_TSQR_RUNG set): only in
 * the row-split driver on more than one rank, where the column-by-column rung costs two collectives per column; on a
 * single GPU the column kernels redo a panel faster than the tree. */
int32_t dhqr_set_tsqr_rung(dhqr_ctx *ctx, int32_t on);
/* The tree alone: R (128 x 128, column-major, upper triangular, zeros below) of a device-resident rows x 128 panel
 * (leading dimension ldp), unique up to the sign of each row (the replay of csrc/dhqr_recon.h fixes the reference's
 * signs R_jj = alpha_j when the tree feeds a factorisation).  Async on the ctx stream. */
int32_t dhqr_tsqr_r_f64(dhqr_ctx *ctx, const double *dP, int64_t rows, int64_t ldp, double *dR);
int32_t dhqr_get_tsqr_count(dhqr_ctx *ctx, int64_t *n_tsqr);
/* Small matrices -- the reference's own test shapes start at 110 x 100, test/runtests.jl:42 -- take ONE single-workgroup
 * launch per qr! (m <= 128 and n <= 128, m <= 224 and n <= 224, or m <= 256 and n <= 192: the matrix lives in the
 * registers of one compute unit, the reference's column-by-column algorithm src:122-148,198-213 as written) and per `\`
 * (m <= 256), whatever `nb` says; the host-array entry points dhqr_qr_f64 / dhqr_ldiv_f64 then run the kernel directly
 * on a pinned staging buffer (csrc/dhqr_small.h).  on = 0: the general drivers for every shape (also DHQR_SMALL=0).
 * Above 128 rows the kernel's waves hand columns and reflectors to each other through LDS flags instead of a barrier per
 * column; those waits are bounded, and a kernel that gave up on one answers NaN in every alpha (never a hung device):
 * dhqr_qr_f64 then factors once more with the barrier form by itself; a caller of the device-resident, asynchronous
 * dhqr_factor_f64 sees the NaN (DHQR_TUNE small_flags=0 selects the barrier form from the start).
 * ComplexF64: 1 <= n <= m <= 128 take ONE launch per qr! and per `\` too (dhqr_factor_c64, dhqr_factor_c64_nb, dhqr_solve_c64,
 * and dhqr_qr_c64 / dhqr_qr_c64_nb / dhqr_ldiv_c64 on the pinned staging buffer; csrc/dhqr_small_complex.h), in the barrier
 * form only: that kernel waits on nothing but a workgroup barrier and has no NaN answer of this kind.  on = 0: today's general
 * ComplexF64 routes for every shape. */
int32_t dhqr_set_small_route(dhqr_ctx *ctx, int32_t on);
/* Solves this context REPEATED with one launch per panel step because a wait of the persistent Q'b kernel (all of whose
 * workgroups must be resident at once) expired -- another process or stream held compute units.  The repetition happens
 * inside the first synchronising entry point after the solve (dhqr_synchronize, dhqr_ldiv_f64, ...), from a copy of b
 * taken before the persistent launch; the caller sees a correct x and DHQR_OK. */
int32_t dhqr_get_solve_retries(dhqr_ctx *ctx, int64_t *n_retries);

/* ------------------------------------------------------------------ synthetic inputs
 * Replaces rand(T,m,n) / rand(T,m) of test/runtests.jl:45-46 with the portable counter-based
 * generator shared with oracle/ :  value(gi, gj) = u01(seed, gi + gj*global_m).
 * The local block holds `rows` x `cols`; local row il is global row row0+il; local column jl is
 * global column ((jl / colblock) * nranks + rank) * colblock + jl % colblock  (block-cyclic 1-D
 * column layout; nranks = 1, rank = 0 gives the identity map). Async. */
int32_t dhqr_fill_uniform_f64(dhqr_ctx *ctx, double *dA, int64_t rows, int64_t cols, int64_t lda,
                              uint64_t seed, int64_t global_m, int64_t row0, int64_t colblock,
                              int32_t nranks, int32_t rank);

/* ------------------------------------------------------------------ factorisation
 * dhqr_factor_f64: device-resident replacement of householder!(A, alpha) (src:113, src:122-148,
 * src:198-213) for one GPU.  In place on dA (m x n, m >= n), writes dalpha[0:n].
 *   nb == 0      : unblocked path (BASELINE configs[1]) -- the reference's operations in the reference's order
 *                  (src:129-143, 208-209: each dot product over the column as updated so far); a launch applies K
 *                  consecutive reflectors to every trailing column it loads once (K = 5 ... 8 for columns of up to
 *                  8192 rows, 5 up to 32768 rows, one reflector per launch above) and builds the next K reflectors
 *                  in its lead workgroup(s).
 *   nb == DHQR_NB: blocked path -- panel factorisation + compact-WY trailing update
 *                  A -= V * (T' * (V' * A)) on FP64 MFMA (BASELINE configs[2]).
 * nb == 0 is asynchronous on the ctx stream.  nb == DHQR_NB enqueues the whole factorisation without host
 * synchronisation and then waits ONCE for the device-side panel verification word (a rejected panel is redone by the
 * robust ladder before returning): synchronous on return. */
int32_t dhqr_factor_f64(dhqr_ctx *ctx, double *dA, int64_t m, int64_t n, int64_t lda,
                        double *dalpha, int32_t nb);

/* dhqr_qr_f64: host-in / host-out drop-in for qr!(A::Matrix{Float64}) (src:311-315): uploads hA,
 * factors, downloads hA and halpha.  Synchronous.  Column blocks travel back while later panels are still being
 * factored, so ON AN ERROR RETURN hA IS UNDEFINED (a mix of original and factored columns) and halpha is not written.
 * The device copy of the matrix (and the pinned staging buffers) stay in the context between calls -- 8 GiB at 32768^2;
 * dhqr_trim releases them. */
int32_t dhqr_qr_f64(dhqr_ctx *ctx, double *hA, int64_t m, int64_t n, int64_t lda, double *halpha,
                    int32_t nb);

/* ------------------------------------------------------------------ solve
 * dhqr_solve_f64: device-resident replacement of solve_householder!(b, H, alpha) (src:284-294):
 * db (length m) <- Q' db (src:215-242), then back substitution with strict-upper dA and the
 * diagonal dalpha (src:244-282); the solution is db[0:n].  Mutates db like the reference.  Asynchronous (see
 * dhqr_synchronize).  csrc/dhqr_qtb.h: per 128-column panel the compact-WY form I - V T' V' with V read in place, GEMV-class
 * kernels (every element of V and of R crosses the memory system once), one persistent launch for Q'b and one
 * flag-pipelined launch for the back substitution.  T' of every panel comes from a batched pre-pass over the factor --
 * or, when this context's last blocked dhqr_factor_f64 was of this very matrix (same dA, m, n, lda) and dalpha still
 * holds that factorisation's values (compared on the device), from what the factorisation kept (DHQR_KEEP_T). */
int32_t dhqr_solve_f64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda,
                       const double *dalpha, double *db);

/* One block step of the back substitution (src:244-282) for rows/columns [lo, hi):
 *   do_diag  : solve the diagonal block in place in db[lo:hi] (divide by dalpha[lo:hi]);
 *   do_update: db[0:lo] -= R[0:lo, lo:hi] * db[lo:hi].
 * dAcols is addressed by GLOBAL column index: column j of R is read at dAcols + j*lda (a
 * column-split caller passes its local block shifted accordingly).  dhqr_solve_f64 is this call
 * looped over blocks; the distributed solve interleaves it with the all-reduce of the partial
 * dots (replacing sum(fetch.(futures)), src:262-266).  Async. */
int32_t dhqr_backsub_block_f64(dhqr_ctx *ctx, const double *dAcols, int64_t lda, const double *dalpha,
                               double *db, int64_t lo, int64_t hi, int32_t do_diag, int32_t do_update);

/* dhqr_ldiv_f64: host-in / host-out drop-in for `H \ b` (src:317-321): does NOT modify hb (the
 * reference copies b into a SharedArray first); writes hx[0:n].  Synchronous. */
int32_t dhqr_ldiv_f64(dhqr_ctx *ctx, const double *hA, int64_t m, int64_t n, int64_t lda,
                      const double *halpha, const double *hb, double *hx);

/* ------------------------------------------------------------------ batches of small matrices
 * `batch` independent problems in one call: the reference's `qr!(A_k)` and `qr!(A_k) \ b_k` repeated for k = 0 .. batch-1,
 * every matrix with its own factor and its own single right-hand side.  Strided layout: matrix k (m x n, column-major,
 * leading dimension lda) starts at A + k*strideA, its alpha at alpha + k*stride_alpha, its b at b + k*strideb, its x at
 * x + k*stridex (strides in elements).  The factor format of every matrix is the single-matrix one (top of this file).
 * Float64 only.
 *   dhqr_factor_batched_f64  device-resident, in place, asynchronous on the ctx stream (first two tiers).
 *   dhqr_solve_batched_f64   device-resident: db_k (m) <- [x_k; tail of Q'b_k]; asynchronous (first two tiers).
 *   dhqr_qr_batched_f64      host in / host out; synchronous.  The device copy of the batch stays in the context between
 *                            calls; dhqr_trim releases it.  On an error return hA is undefined.
 *   dhqr_ldiv_batched_f64    host in / host out `H_k \ b_k`; hb is not modified; synchronous.
 * Routes by shape, in this order:
 *   m <= 64 and n <= 32      ONE launch, one WAVE per matrix and four matrices per workgroup (csrc/dhqr_batched.h): the
 *                            reference's column-by-column algorithm with row l of the matrix in lane l; the solve carries b
 *                            in double-double.
 *   the shapes of dhqr_set_small_route (factor: m <= 128 and n <= 128, m <= 224 and n <= 224, m <= 256 and n <= 192;
 *   solve: m <= 256)         ONE launch of the single-workgroup kernels with grid = batch, workgroup k on matrix k, always in
 *                            their barrier form: results BIT-IDENTICAL to dhqr_factor_f64 / dhqr_solve_f64 of matrix k alone
 *                            with the small route on.
 *   everything else          a host loop over dhqr_factor_f64 / dhqr_solve_f64 with the caller's nb: serial, and
 *                            synchronised after every matrix; the results of the single calls.
 * dhqr_set_small_route(ctx, 0) (or DHQR_SMALL=0) sends every shape to the loop.  nb (0 or DHQR_NB) is ignored on the first
 * two routes.  With profiling on, a batched factor on the first two routes counts ONE n_rank1 group (time in ms_rank1) and
 * a batched solve one n_solve (ms_solve), whatever the batch.
 * batch == 0 or n == 0: no-op, DHQR_OK.  DHQR_EINVAL: batch < 0, m < n, lda < m, strideA < lda*(n-1) + m (the last column
 * of a matrix may be short of lda), stride_alpha < n, strideb < m, stridex < n, null pointers. */
int32_t dhqr_factor_batched_f64(dhqr_ctx *ctx, double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                double *dalpha, int64_t stride_alpha, int64_t batch, int32_t nb);
int32_t dhqr_solve_batched_f64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                               const double *dalpha, int64_t stride_alpha, double *db, int64_t strideb, int64_t batch);
int32_t dhqr_qr_batched_f64(dhqr_ctx *ctx, double *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                            double *halpha, int64_t stride_alpha, int64_t batch, int32_t nb);
int32_t dhqr_ldiv_batched_f64(dhqr_ctx *ctx, const double *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                              const double *halpha, int64_t stride_alpha, const double *hb, int64_t strideb, double *hx,
                              int64_t stridex, int64_t batch);

/* ------------------------------------------------------------------ Float32 methods
 * The reference's qr! and `\` are generic over the element type (partialdot(a, b, is, ::Type{<:Real}) src:42-49, qr!(A)
 * src:306-315): `qr!(rand(Float32, m, n)) \ b` works there.  These are the Float32 counterparts of the four single-matrix and
 * the four batched Float64 entry points above: the same arguments with `float *` in place of `double *`, the same
 * conventions, error codes (DHQR_EINVAL conditions, the n == 0 and batch == 0 no-ops) and factor format, in Float32.  Device
 * pointers need 4-byte alignment only.
 * Routes by shape, in this order:
 *   m <= 64 and n <= 32      NATIVE: one launch, one WAVE per matrix (csrc/dhqr_batched.h with T = float; a single matrix is a batch of 1).  The
 *                            matrix is stored in float, every sum (column norm, v_j' a_c) is taken in double -- the product of
 *                            two floats is exact there --, alpha / f / pivot are formed in double, every stored entry is
 *                            rounded to float once per column step; the solve carries b in double and rounds each entry once.
 *                            With profiling on a factor counts ONE n_rank1 group and a solve one n_solve, whatever the batch.
 *   everything else, and every shape when the small route is off (dhqr_set_small_route(ctx, 0), DHQR_SMALL=0)
 *                            PROMOTED: a kernel widens the matrix (for a solve: the factor, alpha and b) into a Float64
 *                            workspace of the context (packed, lda = m), the Float64 entry point of the same name runs on it
 *                            with the caller's nb (so its small route, one-CU batched tier, unblocked and blocked paths are all
 *                            reachable), a second kernel rounds the result to the caller's arrays, to nearest-even:
 *                                result = float32(f64_entry_point(float64(input)))   by definition.
 *                            A value outside Float32's range rounds to +-inf.  The workspace stays in the context; dhqr_trim
 *                            releases it; a failed allocation is DHQR_ENOMEM.
 *                            A native Float32 path for large matrices (FP32 MFMA trailing updates) does not exist.
 * Synchronisation follows the Float64 route taken:
 *   dhqr_factor_f32          asynchronous on the native tier, on the Float64 small route and with nb == 0; synchronous with
 *                            nb == DHQR_NB beyond the small route (the blocked driver).
 *   dhqr_solve_f32           asynchronous on the native tier and on the Float64 small route; beyond it the call waits for the
 *                            Float64 solve whenever that took the persistent Q'b kernel (a repetition, dhqr_get_solve_retries,
 *                            must land before the result is rounded); the rounding itself is enqueued.  Like every asynchronous
 *                            entry point: results are valid after dhqr_synchronize returned DHQR_OK.
 *   dhqr_factor_batched_f32 / dhqr_solve_batched_f32
 *                            asynchronous on the native tier and on the one-workgroup-per-matrix tier; synchronous on the
 *                            serial tier.
 *   dhqr_qr_f32, dhqr_ldiv_f32, dhqr_qr_batched_f32, dhqr_ldiv_batched_f32
 *                            host in / host out, synchronous: Float32 crosses PCIe (half the bytes of the Float64 forms), the
 *                            conversion happens on the device.  The device copy stays in the context (dhqr_trim).  On an error
 *                            return hA is undefined; hb is not modified. */
int32_t dhqr_factor_f32(dhqr_ctx *ctx, float *dA, int64_t m, int64_t n, int64_t lda, float *dalpha, int32_t nb);
int32_t dhqr_solve_f32(dhqr_ctx *ctx, const float *dA, int64_t m, int64_t n, int64_t lda, const float *dalpha, float *db);
int32_t dhqr_qr_f32(dhqr_ctx *ctx, float *hA, int64_t m, int64_t n, int64_t lda, float *halpha, int32_t nb);
int32_t dhqr_ldiv_f32(dhqr_ctx *ctx, const float *hA, int64_t m, int64_t n, int64_t lda, const float *halpha, const float *hb,
                      float *hx);
int32_t dhqr_factor_batched_f32(dhqr_ctx *ctx, float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, float *dalpha,
                                int64_t stride_alpha, int64_t batch, int32_t nb);
int32_t dhqr_solve_batched_f32(dhqr_ctx *ctx, const float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                               const float *dalpha, int64_t stride_alpha, float *db, int64_t strideb, int64_t batch);
int32_t dhqr_qr_batched_f32(dhqr_ctx *ctx, float *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, float *halpha,
                            int64_t stride_alpha, int64_t batch, int32_t nb);
int32_t dhqr_ldiv_batched_f32(dhqr_ctx *ctx, const float *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                              const float *halpha, int64_t stride_alpha, const float *hb, int64_t strideb, float *hx,
                              int64_t stridex, int64_t batch);

/* ------------------------------------------------------------------ several right-hand sides per matrix
 * `H_k \ B_k` for k = 0 .. batch-1 with a MATRIX B_k of nrhs right-hand sides (several channels fitted against the same
 * small design matrix): what torch.linalg.lstsq or LAPACK's ormqr + trtrs do with a matrix B.  A single matrix is
 * batch = 1.  Strided like the batched family above: B_k (m x nrhs, column-major, leading dimension ldb) starts at
 * B + k*strideB, X_k (n x nrhs, leading dimension ldx) at X + k*strideX; column r of B_k is B + k*strideB + r*ldb.  The
 * factor and alpha arguments are those of dhqr_solve_batched_f64 / _f32.
 *   dhqr_solve_batched_nrhs_f64 / _f32  device-resident: dB_k (m x nrhs) <- [X_k; tail of Q'B_k], in place; asynchronous
 *                                       wherever the single-column entry point of the same type is.
 *   dhqr_ldiv_batched_nrhs_f64 / _f32   host in / host out; hB is not modified (src:318), hX_k (n x nrhs) is written;
 *                                       synchronous; staged through the buffers of dhqr_ldiv_batched_f64 / _f32 (dhqr_trim).
 * Column r of the result is BIT-IDENTICAL to what dhqr_solve_batched_f64 / _f32 returns for b_k = B_k[:, r] alone, on every
 * route: it depends neither on nrhs nor on the column's position nor on the batch.
 * That is the BATCHED single-column entry point, also for batch = 1.  dhqr_solve_f64 (one matrix, one vector) is another
 * route for m <= 64 and n <= 32 -- the single-workgroup kernel of dhqr_set_small_route instead of the wave kernel --, and
 * its result may differ from these in the last bits, exactly as it differs from dhqr_solve_batched_f64 with batch = 1.
 * Beyond those shapes, and in Float32 everywhere, the single-matrix entry points give the same bits as these.
 * Routes, in this order:
 *   m <= 64 and n <= 32      ONE launch, one WAVE per matrix (csrc/dhqr_batched_nrhs.h): the factor and alpha are loaded into
 *                            registers once, the columns of B_k walk past them in groups of up to four (three for Float64
 *                            with n > 8, where four do not fit the registers) whose Q'b chains interleave.
 *                            With profiling on: ONE n_solve group, whatever nrhs and batch.  MEASURED (batch 16384,
 *                            profiles/batched_nrhs_throughput.txt): the kernel's time goes by groups -- a group costs 2.5 to
 *                            3.0 single-column solves, a tail's zero columns included -- so against the column loop below
 *                            nrhs = 2 lost (0.62 - 0.81 x), nrhs = 4 in groups of three lost (0.77 - 0.80 x), nrhs = 4 in
 *                            groups of four, 8 and 16 won (1.01 - 1.23 x).  The boundary: the kernel runs where its groups
 *                            carry at least 2.6 real columns on average (5 nrhs >= 13 ceil(nrhs / group)); every other nrhs,
 *                            nrhs == 1 among them, takes the column loop on the wave-per-matrix single-column kernel: the
 *                            same bits, nrhs n_solve groups.
 *   every other shape        (and every shape when the small route is off) ONE EXISTING SOLVE PER COLUMN: a loop r = 0 ..
 *                            nrhs-1 over dhqr_solve_batched_f64 with b = B + r*ldb and strideb = strideB -- its
 *                            one-workgroup tier, its serial tier with the synchronisation after every matrix, the profiling
 *                            counts of nrhs single calls.  Float32: factor, alpha and B are widened ONCE into the Float64
 *                            workspace, the Float64 entry point of this block runs on them, B is rounded back.
 *                            A blocked multi-column route for large matrices (Q'B by block reflectors and a triangular
 *                            solve with a matrix right-hand side) does not exist yet.
 * nrhs == 0, batch == 0 or n == 0: no-op, DHQR_OK, nothing is touched.  DHQR_EINVAL (nothing is written): everything the
 * batched family rejects, nrhs < 0, null B or X, ldb < m, strideB < ldb*(nrhs-1) + m, ldx < n, strideX < ldx*(nrhs-1) + n. */
int32_t dhqr_solve_batched_nrhs_f64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                    const double *dalpha, int64_t stride_alpha, double *dB, int64_t nrhs, int64_t ldb,
                                    int64_t strideB, int64_t batch);
int32_t dhqr_ldiv_batched_nrhs_f64(dhqr_ctx *ctx, const double *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                   const double *halpha, int64_t stride_alpha, const double *hB, int64_t nrhs, int64_t ldb,
                                   int64_t strideB, double *hX, int64_t ldx, int64_t strideX, int64_t batch);
int32_t dhqr_solve_batched_nrhs_f32(dhqr_ctx *ctx, const float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                    const float *dalpha, int64_t stride_alpha, float *dB, int64_t nrhs, int64_t ldb,
                                    int64_t strideB, int64_t batch);
int32_t dhqr_ldiv_batched_nrhs_f32(dhqr_ctx *ctx, const float *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                   const float *halpha, int64_t stride_alpha, const float *hB, int64_t nrhs, int64_t ldb,
                                   int64_t strideB, float *hX, int64_t ldx, int64_t strideX, int64_t batch);

/* ------------------------------------------------------------------ Q application, explicit Q and R: batches and Float32
 * What dhqr_apply_q_f64 and dhqr_form_r0_f64 (below) do for one Float64 matrix, for every factorisation of the small-matrix
 * family: k = 0 .. batch-1, Float64 and Float32; a single matrix is batch = 1.  Strided like the blocks above: H_k at
 * dA + k*strideA (the factor dhqr_factor_batched_* left), B_k (m x nrhs, leading dimension ldb) at dB + k*strideB, Q_k (m x n,
 * ldq) at dQ + k*strideQ, R_k (n x n, ldr) at dR + k*strideR.  All pointers are device-resident; every call is asynchronous
 * on the context's stream.
 *   dhqr_apply_q_batched_f64 / _f32  dB_k <- Q_k' dB_k (trans = 1) or Q_k dB_k (trans = 0), in place.  Q_k = H_0 ... H_{n-1} is
 *                                    made of the reflectors alone: no alpha is taken.
 *   dhqr_form_q_batched_f64 / _f32   dQ_k <- the explicit thin Q_k = Q_k [I; 0] (m x n).  dQ is written only: nothing of it
 *                                    is read, all m rows of its n columns are written.
 *   dhqr_form_r_batched_f64 / _f32   dR_k <- R_k: the strict upper part of H_k, alpha_k on the diagonal, zeros below
 *                                    (src:296-309).  One element-wise launch for every shape and both types; copies only.
 * Routes of apply_q and form_q, in this order:
 *   m <= 64 and n <= 32      (small route on) ONE launch, one WAVE per matrix (csrc/dhqr_batched_applyq.h), whatever nrhs and
 *                            batch: the factor is loaded into registers once, the columns walk past it in groups of up to four
 *                            (three for Float64 with n > 16).  trans = 1 evaluates, per column, exactly the expressions of the
 *                            Q'B phase of dhqr_solve_batched_nrhs_*: rows n .. m-1 of the result are BIT-IDENTICAL to the
 *                            same rows of what that solve leaves in dB (the tail of Q'B).  trans = 0 applies the same
 *                            expressions with the reflectors right to left.  form_q is trans = 0 on columns e_r made in
 *                            registers, skipping the reflectors behind a group's last column (they act as the identity);
 *                            for a finite factor it compares equal to trans = 0 applied to [I; 0].  Column r of a result
 *                            depends neither on nrhs nor on its place nor on the batch.
 *                            With profiling on: ONE n_solve group per call (the category of the solve whose first phase
 *                            this is).  dhqr_form_r_batched_* is not counted.
 *   every other shape, f64   a loop over the matrices on the blocked compact-WY route of dhqr_apply_q_f64: the bits of that
 *                            call on matrix k alone, its profiling counts.  form_q: dQ_k <- [I; 0] by one small launch, then
 *                            that loop with trans = 0.
 *   every other shape, f32   PROMOTED: the factor and B are widened once into the Float64 workspace of the context
 *                            (dhqr_trim), the Float64 entry point of this block runs on them (packed: leading dimension m),
 *                            the result is rounded back: result = float32(f64 entry point(float64(input))) by definition.
 * batch == 0, n == 0 or nrhs == 0: no-op, DHQR_OK, no pointer is looked at.  DHQR_EINVAL (nothing is written): batch < 0,
 * nrhs < 0, m < n, a null pointer, lda < m, strideA < lda*(n-1) + m, ldb or ldq < m, ldr < n, a stride of B, Q or R shorter
 * than its last column needs (ld*(cols-1) + rows), stride_alpha < n, trans outside {0, 1}. */
int32_t dhqr_apply_q_batched_f64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, double *dB,
                                 int64_t nrhs, int64_t ldb, int64_t strideB, int64_t batch, int32_t trans);
int32_t dhqr_apply_q_batched_f32(dhqr_ctx *ctx, const float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, float *dB,
                                 int64_t nrhs, int64_t ldb, int64_t strideB, int64_t batch, int32_t trans);
int32_t dhqr_form_q_batched_f64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, double *dQ,
                                int64_t ldq, int64_t strideQ, int64_t batch);
int32_t dhqr_form_q_batched_f32(dhqr_ctx *ctx, const float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA, float *dQ,
                                int64_t ldq, int64_t strideQ, int64_t batch);
int32_t dhqr_form_r_batched_f64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                const double *dalpha, int64_t stride_alpha, double *dR, int64_t ldr, int64_t strideR,
                                int64_t batch);
int32_t dhqr_form_r_batched_f32(dhqr_ctx *ctx, const float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                const float *dalpha, int64_t stride_alpha, float *dR, int64_t ldr, int64_t strideR,
                                int64_t batch);

/* ------------------------------------------------------- column-pivoted QR and rank-revealing least squares: batches, Float64
 * The entry points above assume full column rank: a zero column gives a NaN reflector, a nearly collinear design matrix a
 * huge, meaningless x.  These factor with COLUMN PIVOTING, A_k P_k = Q_k R_k (LAPACK geqp3's ordering), estimate the rank from
 * the diagonal of R and solve min ||A_k x - b|| with the columns behind the rank dropped (gelsy's basic solution).  The
 * reference has no counterpart.  Strided like the batched blocks above; jpvt_k (n int32) at djpvt + k*stride_jpvt.  The
 * factor format is the one at the top of this file plus the permutation, so a pivoted factor is a valid argument of
 * dhqr_apply_q_batched_f64, dhqr_form_q_batched_f64 and dhqr_form_r_batched_f64: they give Q_k, R_k with
 * A_k[:, jpvt_k] = Q_k R_k.  Device-resident and asynchronous on the context's stream unless stated otherwise.
 *   dhqr_factor_batched_pivoted_f64  in place; jpvt_k[j] (0-based) is the original column now in position j.  Step j: the
 *                            squared 2-norms of rows >= j of the columns j .. n-1 are computed afresh from the working matrix
 *                            in double (no downdating); the smallest column that attains the maximum is taken (compared with
 *                            `>`: a NaN never wins) and swapped with column j in whole, R rows included.  The reflector is
 *                            formed as dhqr_factor_batched_f64 forms it, except that a pivot entry of exactly 0 takes
 *                            alpha = -norm (alphafactor(0) = -1) and so a valid reflector.  A maximum of exactly 0: the rest
 *                            is zero, every remaining column c gets alpha_c = 0 and v_c = sqrt(2) e_c, no more swaps.  A
 *                            finite matrix in range therefore always gets a finite factor, and |alpha_j| does not increase
 *                            with j; a non-finite matrix keeps its trouble to itself and jpvt stays a permutation.
 *                            RANGE: the pivot search is NOT scaled -- entries must be 0 or of magnitude within
 *                            [1e-150, 1e150].
 *   dhqr_rank_batched_f64    drank[k] (int32) <- the number of leading j with |alpha_j| > rc |alpha_0|, counting stops at
 *                            the first failure (a NaN stops it; a zero matrix has rank 0); rc = rcond if rcond >= 0, else
 *                            max(m, n) 2^-52.  One element-wise launch; not counted by the profile.
 *   dhqr_solve_batched_pivoted_f64  with r = clamp(drank[k], 0, n): dB_k (m x nrhs) <- [z; tail], what solve_householder!
 *                            leaves when run with the first r columns of the factor: z = R11^-1 (Q_r' B_k)[0:r], and rows
 *                            r .. m-1 hold the part of B_k outside the range of A_k -- the 2-norm of those rows of a column is
 *                            its residual ||A_k x - b||.  dX_k (n x nrhs, ldx) <- the basic solution: x[jpvt[i]] = z_i for
 *                            i < r, exact zeros elsewhere.  r = 0: dB_k is left untouched, X_k = 0.
 *   dhqr_qr_batched_pivoted_f64  host in / host out form of the factorisation; synchronous.
 *   dhqr_lstsq_batched_f64   host in / host out: factors a staged copy, computes the ranks, solves, copies hX_k (n x nrhs) and
 *                            hrank[k] out; hA and hB are not modified; synchronous.  Both host forms stage through the buffer
 *                            of dhqr_qr_batched_f64 (dhqr_trim releases it).
 * Routes:
 *   m <= 64 and n <= 32      (small route on) ONE launch per call, one WAVE per matrix (csrc/dhqr_batched_pivoted.h): the
 *                            kernels of dhqr_factor_batched_f64 / dhqr_solve_batched_f64 with the pivot step / with the
 *                            wave's own rank in place of n.  The pivoted factor of A has the BITS of dhqr_factor_batched_f64
 *                            on A[:, jpvt] (where no pivot entry is exactly 0); dB after the solve has the bits of
 *                            dhqr_solve_batched_f64 called with n = r on that factor, column by column, whatever nrhs, the
 *                            column's place and the batch.
 *   every other shape        (and every shape with the small route off) ONE launch per call, one workgroup per matrix
 *                            (factor) or per (matrix, column of B) (solve), in place in device memory, in plain double but
 *                            for the reflector's norm.  This tier exists for completeness -- any shape gets an answer --,
 *                            not for speed.
 * With profiling on a factor counts ONE n_rank1 group and a solve ONE n_solve group per launch.
 * batch == 0, n == 0 or nrhs == 0: no-op, DHQR_OK.  DHQR_EINVAL (nothing is written): what the batched family rejects, a null
 * jpvt, rank or X, stride_jpvt < n, ldx < n, strideX < ldx*(nrhs-1) + n; off the wave tier batch * nrhs > 2^31 - 1. */
int32_t dhqr_factor_batched_pivoted_f64(dhqr_ctx *ctx, double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                        double *dalpha, int64_t stride_alpha, int32_t *djpvt, int64_t stride_jpvt, int64_t batch);
int32_t dhqr_rank_batched_f64(dhqr_ctx *ctx, const double *dalpha, int64_t m, int64_t n, int64_t stride_alpha, double rcond,
                              int32_t *drank, int64_t batch);
int32_t dhqr_solve_batched_pivoted_f64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                       const double *dalpha, int64_t stride_alpha, const int32_t *djpvt, int64_t stride_jpvt,
                                       const int32_t *drank, double *dB, int64_t nrhs, int64_t ldb, int64_t strideB, double *dX,
                                       int64_t ldx, int64_t strideX, int64_t batch);
int32_t dhqr_qr_batched_pivoted_f64(dhqr_ctx *ctx, double *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, double *halpha,
                                    int64_t stride_alpha, int32_t *hjpvt, int64_t stride_jpvt, int64_t batch);
int32_t dhqr_lstsq_batched_f64(dhqr_ctx *ctx, const double *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const double *hB,
                               int64_t nrhs, int64_t ldb, int64_t strideB, double rcond, double *hX, int64_t ldx, int64_t strideX,
                               int32_t *hrank, int64_t batch);

/* The same five for Float32 and ComplexF64 -- the argument lists of the _f64 forms with the element type changed; ComplexF64
 * is passed as every _c64 entry point passes it: `double *`, interleaved (re, im), lda and the strides of A, alpha, B and X
 * counted in COMPLEX elements, device pointers 16-byte aligned.  jpvt and rank stay int32.  Argument rules, the empty calls,
 * DHQR_EINVAL (nothing is written) and the profiling counts are those of the _f64 forms.  The rule above, per type:
 *   pivot search   the squared 2-norms of rows >= j of the trailing columns, afresh, in plain double, unscaled: Float32 from
 *                  the stored float values widened (products and sums in double), ComplexF64 as re^2 + im^2; the smallest
 *                  column index that attains the maximum, compared with `>`; whole columns and their jpvt entries swap.
 *   zero tail      a maximum of exactly 0: alpha_c = 0 and v_c = sqrt(2) e_c (real, also for ComplexF64; Float32: sqrt(2)
 *                  rounded to float) for every remaining column, no more swaps.
 *   reflector      Float32: the expressions of dhqr_factor_batched_f32's wave kernel (float storage, double sums, every
 *                  stored entry rounded once), a pivot entry of exactly 0 taking alpha = -norm.  ComplexF64: exactly the
 *                  expressions of dhqr_factor_batched_c64's wave kernel, whose alphafactor already gives -1 at 0.
 *   rank           the number of leading j with |alpha_j| > rc |alpha_0|, compared in double; ComplexF64: |alpha| =
 *                  hypot(re, im); rcond < 0: rc = max(m, n) eps -- 2^-52 for ComplexF64, 2^-23 for Float32.
 *   solve          r = clamp(drank[k], 0, n); dB_k <- [z; tail] as the type's own unpivoted solve leaves it on the first r
 *                  columns; dX_k[jpvt[i]] = z_i for i < r, exact zeros (+0, +0 + 0i) elsewhere; r = 0 leaves dB_k untouched;
 *                  an out-of-range jpvt entry is not written.
 * Routes:
 *   m <= 64 and n <= 32      (small route on) ONE launch per call, one WAVE per matrix.  Float32: the kernels of
 *                            csrc/dhqr_batched_pivoted.h with T = float.  ComplexF64: csrc/dhqr_batched_complex_pivoted.h.  The
 *                            pivoted factor of A has the BITS of dhqr_factor_batched_f32 / _c64 on A[:, jpvt] (Float32: where
 *                            no pivot entry is exactly 0); dB after the solve has the bits of dhqr_solve_batched_nrhs_f32 /
 *                            _c64 called with n = r, column by column, whatever nrhs, the column's place and the batch.
 *   every other shape        (and every shape with the small route off) ComplexF64: ONE launch per call of the general
 *                            kernels of csrc/dhqr_batched_complex_pivoted.h, a workgroup per matrix / per (matrix, column of
 *                            B).  Float32: PROMOTED as everywhere -- float32(Float64 route(float64(.))): A (or the factor,
 *                            alpha, B and X) widened, the Float64 pivoted route, the results rounded; jpvt is the Float64
 *                            route's.
 * The host forms stage through the buffers of dhqr_qr_batched_f32 / dhqr_qr_batched_c64 (dhqr_trim releases them). */
int32_t dhqr_factor_batched_pivoted_f32(dhqr_ctx *ctx, float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                        float *dalpha, int64_t stride_alpha, int32_t *djpvt, int64_t stride_jpvt, int64_t batch);
int32_t dhqr_rank_batched_f32(dhqr_ctx *ctx, const float *dalpha, int64_t m, int64_t n, int64_t stride_alpha, double rcond,
                              int32_t *drank, int64_t batch);
int32_t dhqr_solve_batched_pivoted_f32(dhqr_ctx *ctx, const float *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                       const float *dalpha, int64_t stride_alpha, const int32_t *djpvt, int64_t stride_jpvt,
                                       const int32_t *drank, float *dB, int64_t nrhs, int64_t ldb, int64_t strideB, float *dX,
                                       int64_t ldx, int64_t strideX, int64_t batch);
int32_t dhqr_qr_batched_pivoted_f32(dhqr_ctx *ctx, float *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, float *halpha,
                                    int64_t stride_alpha, int32_t *hjpvt, int64_t stride_jpvt, int64_t batch);
int32_t dhqr_lstsq_batched_f32(dhqr_ctx *ctx, const float *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const float *hB,
                               int64_t nrhs, int64_t ldb, int64_t strideB, double rcond, float *hX, int64_t ldx, int64_t strideX,
                               int32_t *hrank, int64_t batch);
int32_t dhqr_factor_batched_pivoted_c64(dhqr_ctx *ctx, double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                        double *dalpha, int64_t stride_alpha, int32_t *djpvt, int64_t stride_jpvt, int64_t batch);
int32_t dhqr_rank_batched_c64(dhqr_ctx *ctx, const double *dalpha, int64_t m, int64_t n, int64_t stride_alpha, double rcond,
                              int32_t *drank, int64_t batch);
int32_t dhqr_solve_batched_pivoted_c64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                       const double *dalpha, int64_t stride_alpha, const int32_t *djpvt, int64_t stride_jpvt,
                                       const int32_t *drank, double *dB, int64_t nrhs, int64_t ldb, int64_t strideB, double *dX,
                                       int64_t ldx, int64_t strideX, int64_t batch);
int32_t dhqr_qr_batched_pivoted_c64(dhqr_ctx *ctx, double *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, double *halpha,
                                    int64_t stride_alpha, int32_t *hjpvt, int64_t stride_jpvt, int64_t batch);
int32_t dhqr_lstsq_batched_c64(dhqr_ctx *ctx, const double *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA, const double *hB,
                               int64_t nrhs, int64_t ldb, int64_t strideB, double rcond, double *hX, int64_t ldx, int64_t strideX,
                               int32_t *hrank, int64_t batch);

/* KAT hook mirroring partialdot(a, b, lo:hi, Float64) (src:42-49; test/partialdot.jl:18):
 * sum_{i=lo}^{hi-1} da[i]*db[i] (0-based, hi exclusive) reduced on the device with the same
 * wavefront-shuffle + LDS tree the factor kernels use.  Synchronous (returns a host scalar). */
int32_t dhqr_partialdot_f64(dhqr_ctx *ctx, const double *da, const double *db, int64_t lo,
                            int64_t hi, double *hout);
/* Same with HOST vectors (uploads ha[lo:hi], hb[lo:hi]); what the Julia module's partialdot binds. */
int32_t dhqr_partialdot_host_f64(dhqr_ctx *ctx, const double *ha, const double *hb, int64_t lo,
                                 int64_t hi, double *hout);

/* ------------------------------------------------------------------ ComplexF64 methods
 * The reference's qr!/`\` are generic over the element type and its tests run every shape for
 * ComplexF64 too (test/runtests.jl:43); these are the ComplexF64 counterparts of the Float64 entry
 * points above (unblocked path).  A complex element is an interleaved
 * (re, im) pair of doubles == Julia's ComplexF64, so a `Ptr{ComplexF64}` is passed as `double *`;
 * m, n, lda and the lo/hi ranges count ELEMENTS.  Device pointers must be 16-byte aligned.
 * Factor format as for Float64 with H_j = I - v_j v_j^H and complex alpha (the reference does not
 * phase-normalise R: alpha_j = -exp(i arg a_jj) ||a_j||, src:9,130; a zero pivot gives -||a_j||).
 *
 * dhqr_factor_c64   householder!(A, alpha) for ComplexF64 (src:113, 122-148, 171-213). Async.
 * dhqr_qr_c64       host-in / host-out qr!(A) (src:311-315). Synchronous.
 * dhqr_solve_c64    solve_householder!(b, H, alpha) (src:284-294 with the conj-dot of src:51-59):
 *                   db (m elements) is overwritten, x = db[0:n]. Async.
 * dhqr_ldiv_c64     host-in / host-out `H \ b` (src:317-321); hb is not modified. Synchronous.
 * dhqr_partialdot_c64 / _host_c64
 *                   partialdot(a, b, lo:hi, ComplexF64) = sum conj(a[i]) b[i] (src:51-59) -- the
 *                   function the reference's only known-answer test exercises
 *                   (test/partialdot.jl:12-20); hout[0] = re, hout[1] = im. Synchronous.
 *
 * dhqr_factor_c64_nb / dhqr_qr_c64_nb: the same with a panel width: nb = 0 unblocked, nb = DHQR_ZNB (64 complex columns)
 *                   BLOCKED: the panel's block reflector I - V T V^H is applied to the trailing matrix by the Float64
 *                   MFMA kernels through the real 2 x 2 embedding of the 64 complex reflectors (= 128 real columns);
 *                   identical factor format and values (to rounding).
 *
 * The one-workgroup route (small route on, 1 <= n <= m <= 128; csrc/dhqr_small_complex.h): the matrix -- at most 256 KB --
 * lives in the registers of one compute unit as (re, im) and the reference's column-by-column algorithm runs as written, one
 * workgroup barrier per column; the solve carries both parts of b in double-double and divides by alpha_j as the general
 * solve does.  dhqr_factor_c64, dhqr_factor_c64_nb (whatever nb says; another nb than 0 or DHQR_ZNB is still DHQR_EINVAL) and
 * dhqr_solve_c64 make ONE asynchronous launch on the ctx stream: the batched tiers below on a batch of one (the wave kernel
 * up to 64 x 32, the workgroup kernel beyond), so a single call has the bits of dhqr_factor_batched_c64 /
 * dhqr_solve_batched_c64 with batch = 1, whatever lda.  dhqr_qr_c64, dhqr_qr_c64_nb and dhqr_ldiv_c64 copy into the context's
 * pinned staging buffer, make that one launch on it and copy out: no hipMalloc, hipFree or hipMemcpy, the bits of the
 * device-resident call; dhqr_trim releases the buffer.  Only these entry points: the panels of the blocked driver and of the
 * column-split and multi-GPU drivers keep their kernels whatever their size.  With profiling on a factor counts ONE n_rank1
 * group and a solve one n_solve.  A column whose reflector is not finite leaves what the reference leaves (finite columns
 * in front, alpha as formed there, NaN from that row on in the columns from there on).
 * Measured boundary: profiles/small_c64.txt. */
#define DHQR_ZNB 64
int32_t dhqr_factor_c64_nb(dhqr_ctx *ctx, double *dA, int64_t m, int64_t n, int64_t lda, double *dalpha, int32_t nb);
int32_t dhqr_qr_c64_nb(dhqr_ctx *ctx, double *hA, int64_t m, int64_t n, int64_t lda, double *halpha, int32_t nb);
int32_t dhqr_factor_c64(dhqr_ctx *ctx, double *dA, int64_t m, int64_t n, int64_t lda, double *dalpha);
int32_t dhqr_qr_c64(dhqr_ctx *ctx, double *hA, int64_t m, int64_t n, int64_t lda, double *halpha);
int32_t dhqr_solve_c64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda,
                       const double *dalpha, double *db);
int32_t dhqr_ldiv_c64(dhqr_ctx *ctx, const double *hA, int64_t m, int64_t n, int64_t lda,
                      const double *halpha, const double *hb, double *hx);
int32_t dhqr_partialdot_c64(dhqr_ctx *ctx, const double *da, const double *db, int64_t lo, int64_t hi,
                            double *hout);
int32_t dhqr_partialdot_host_c64(dhqr_ctx *ctx, const double *ha, const double *hb, int64_t lo,
                                 int64_t hi, double *hout);

/* ------------------------------------------------------------------ batches of small ComplexF64 matrices
 * The ComplexF64 counterparts of the four batched Float64 entry points (dhqr_factor_batched_f64 ...): `qr!(A_k)` and
 * `qr!(A_k) \ b_k` for k = 0 .. batch-1, every matrix with its own factor and its own single right-hand side.  The same
 * arguments and the same strided layout, with the conventions of the ComplexF64 section: pointers are interleaved (re, im)
 * doubles, lda and EVERY stride count complex elements, device pointers are 16-byte aligned.  nb is 0 or DHQR_ZNB.  The
 * factor format of every matrix is the single-matrix one (alpha_k complex: n complex elements per matrix).
 * Routes by shape, in this order:
 *   m <= 64 and n <= 32      (small route on) ONE launch, one WAVE per matrix and four matrices per workgroup
 *                            (csrc/dhqr_batched_complex.h): the reference's column-by-column algorithm with row l of the
 *                            matrix, as (re, im), in lane l; column norms in double-double, alphafactor(0) = -1 (src:9); the
 *                            solve carries both parts of b in double-double and divides by alpha_j as dhqr_solve_c64 does.
 *                            Asynchronous on the ctx stream.  nb is ignored.  With profiling on a factor counts ONE n_rank1
 *                            group and a solve one n_solve, whatever the batch.
 *   otherwise m <= 128       (small route on) ONE launch of the single-workgroup kernels of the ComplexF64 section above
 *                            (csrc/dhqr_small_complex.h) with grid = batch, workgroup k on matrix k: the bits of
 *                            dhqr_factor_c64 / dhqr_solve_c64 on matrix k alone, independent of lda, the strides, the batch
 *                            and the position in it.  Asynchronous on the ctx stream.  nb is ignored.  ONE n_rank1 group
 *                            per factor and one n_solve per solve, whatever the batch.
 *   everything else, and every shape when the small route is off (dhqr_set_small_route(ctx, 0), DHQR_SMALL=0)
 *                            a host loop over dhqr_factor_c64_nb (with the caller's nb) / dhqr_solve_c64 on matrix k alone:
 *                            serial, synchronised after every matrix; that call's bits and its profiling counts.
 *                            Synchronous.
 *   dhqr_qr_batched_c64, dhqr_ldiv_batched_c64
 *                            host in / host out, synchronous; staged through the context's device copy of a batch (the one
 *                            dhqr_qr_batched_f64 uses; dhqr_trim releases it).  On an error return hA is undefined; hb is not
 *                            modified (src:318).
 * batch == 0 or n == 0: no-op that looks at no pointer, DHQR_OK.  DHQR_EINVAL, and nothing is written: batch < 0, m < n,
 * lda < m, strideA < lda*(n-1) + m, stride_alpha < n, strideb < m, stridex < n, null pointers, another nb, a device pointer
 * that is not 16-byte aligned.  Several right-hand sides per matrix, Q application and explicit Q / R: the next section. */
int32_t dhqr_factor_batched_c64(dhqr_ctx *ctx, double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                double *dalpha, int64_t stride_alpha, int64_t batch, int32_t nb);
int32_t dhqr_solve_batched_c64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                               const double *dalpha, int64_t stride_alpha, double *db, int64_t strideb, int64_t batch);
int32_t dhqr_qr_batched_c64(dhqr_ctx *ctx, double *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                            double *halpha, int64_t stride_alpha, int64_t batch, int32_t nb);
int32_t dhqr_ldiv_batched_c64(dhqr_ctx *ctx, const double *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                              const double *halpha, int64_t stride_alpha, const double *hb, int64_t strideb, double *hx,
                              int64_t stridex, int64_t batch);

/* ------------------------------------------------------------------ batches of small ComplexF64 factors: several
 * right-hand sides, Q application, explicit Q and R
 * The ComplexF64 counterparts of dhqr_solve_batched_nrhs_f64, dhqr_ldiv_batched_nrhs_f64, dhqr_apply_q_batched_f64,
 * dhqr_form_q_batched_f64 and dhqr_form_r_batched_f64: the same argument lists, the same layouts (B_k, Q_k, R_k, X_k at
 * p + k stride with their own leading dimension), the same argument rules and empty cases, with the conventions of the
 * ComplexF64 section -- pointers are interleaved (re, im) doubles, EVERY leading dimension and stride counts complex
 * elements, device pointers are 16-byte aligned.  A single matrix is a batch of one.  Q = H_1 ... H_n with the Hermitian
 * reflectors H_c = I - v_c v_c^H of the factor; trans = 1 applies Q^H.
 *   dhqr_solve_batched_nrhs_c64  dB_k (m x nrhs) <- [X_k; tail of Q^H B_k], in place.  Column r has the BITS of
 *                            dhqr_solve_batched_c64 on that column alone, whatever nrhs and batch.  m <= 64 and n <= 32
 *                            (small route on): ONE launch of the multi-column kernel (csrc/dhqr_batched_complex_nrhs.h: the
 *                            factor and alpha in registers once, the columns in groups of 1 / 2 / 4 for n <= 8 / 16 / 32)
 *                            where that was measured to beat the column loop -- nrhs >= 4 in full groups: 1.04 - 1.15 x,
 *                            profiles/batched_c64_nrhs_throughput.txt --, else dhqr_solve_batched_c64 column by column.
 *                            Beyond that, up to 128 rows (small route on): ONE launch of the one-workgroup multi-column
 *                            kernel (csrc/dhqr_small_complex_nrhs.h: a workgroup per matrix and group of 6 columns, which
 *                            reads the factor once for the group), one n_solve group whatever nrhs and batch, where that
 *                            was measured to beat the column loop -- 2 .. 6 columns 1.05 - 1.67 x, 13 .. 18 columns 1.34 -
 *                            1.47 x; two groups (7 .. 12 columns) lose: profiles/small_c64_nrhs_throughput.txt; DHQR_TUNE
 *                            zsmall_nrhs=1 / 0: always / never.
 *                            Every other call: dhqr_solve_batched_c64 column by column: its tiers, synchronisation and
 *                            counts.
 *   dhqr_ldiv_batched_nrhs_c64   host in / host out through the staging area of dhqr_ldiv_batched_c64; hB is not modified
 *                            (src:318); X_k (n x nrhs) has the device form's bits (and its tiers: the staged copy is device
 *                            memory).  Synchronous.
 *   dhqr_apply_q_batched_c64 dB_k <- Q_k^H dB_k (trans = 1) or Q_k dB_k (trans = 0), in place; needs no alpha.
 *   dhqr_form_q_batched_c64  dQ_k (m x n, ldq) <- the explicit thin Q_k; nothing of dQ is read.
 *                            Both: m <= 64 and n <= 32 (small route on) ONE launch, one wave per matrix, a column carried in
 *                            double-double per component; rows n .. m-1 of trans = 1 have the bits of what the solve leaves
 *                            there; form_q compares equal to trans = 0 on [I; 0] for a finite factor.  Beyond that, up to
 *                            128 rows (small route on): ONE launch of the one-workgroup multi-column kernel
 *                            (csrc/dhqr_small_complex_nrhs.h) for every nrhs and batch, with the same three properties and
 *                            every column's bits independent of nrhs, of its place and of the batch (DHQR_TUNE
 *                            zsmall_nrhs=0: the plain kernel below).  More than 128 rows, and every shape with the small
 *                            route off: ONE launch of a plain kernel, a workgroup per (matrix, column), in place in device
 *                            memory in plain double (form_q: [I; 0] first); it re-reads the factor once per column -- a
 *                            blocked ComplexF64 apply-Q for large matrices does not exist yet.
 *                            Asynchronous on the ctx stream; with profiling on each launch counts one n_solve group.
 *   dhqr_form_r_batched_c64  dR_k (n x n, ldr) <- the strict upper part of H_k, alpha_k on the diagonal, zeros below: one
 *                            element-wise launch for every shape.  Asynchronous.
 * nrhs == 0, batch == 0 or n == 0: no-op that looks at no pointer.  DHQR_EINVAL, and nothing is written: what the Float64
 * namesakes reject (negative nrhs or batch, trans not 0 or 1, m < n, short leading dimensions or strides, null pointers) and
 * a device pointer that is not 16-byte aligned. */
int32_t dhqr_solve_batched_nrhs_c64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                    const double *dalpha, int64_t stride_alpha, double *dB, int64_t nrhs, int64_t ldb,
                                    int64_t strideB, int64_t batch);
int32_t dhqr_ldiv_batched_nrhs_c64(dhqr_ctx *ctx, const double *hA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                   const double *halpha, int64_t stride_alpha, const double *hB, int64_t nrhs, int64_t ldb,
                                   int64_t strideB, double *hX, int64_t ldx, int64_t strideX, int64_t batch);
int32_t dhqr_apply_q_batched_c64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                 double *dB, int64_t nrhs, int64_t ldb, int64_t strideB, int64_t batch, int32_t trans);
int32_t dhqr_form_q_batched_c64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                double *dQ, int64_t ldq, int64_t strideQ, int64_t batch);
int32_t dhqr_form_r_batched_c64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda, int64_t strideA,
                                const double *dalpha, int64_t stride_alpha, double *dR, int64_t ldr, int64_t strideR,
                                int64_t batch);

/* ------------------------------------------------------------------ Q application / metric
 * dB (m x nrhs) <- Q' dB (trans = 1) or Q dB (trans = 0), Q = H_1 ... H_n from a factored dA.
 * Blocked compact-WY on MFMA (T is rebuilt per panel from V). No reference analogue beyond
 * src:215-242 (single vector); needed for the north-star metric ||A - QR|| / ||A||. Async.
 * One Float64 matrix; batches and Float32: dhqr_apply_q_batched_f64 / _f32 above. */
int32_t dhqr_apply_q_f64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t n, int64_t lda,
                         double *dB, int64_t nrhs, int64_t ldb, int32_t trans);

/* rel = ||dAorig - Q R||_F / ||dAorig||_F with Q,R taken from (dAfact, dalpha). dwork is an
 * m x n scratch matrix (leading dimension m) that receives Q*R.  Synchronous (host scalar). */
int32_t dhqr_residual_f64(dhqr_ctx *ctx, const double *dAfact, int64_t m, int64_t n, int64_t lda,
                          const double *dalpha, const double *dAorig, int64_t ldo, double *dwork,
                          double *hrel);

/* Building blocks of the residual for a column-split matrix (same maps as dhqr_fill_uniform_f64):
 * dW[:, jl] = [R; 0] column of local column jl (global index via the block-cyclic map; dalpha is
 * the GLOBAL alpha vector).  Async. */
int32_t dhqr_form_r0_f64(dhqr_ctx *ctx, const double *dA, int64_t m, int64_t cols, int64_t lda,
                         const double *dalpha, double *dW, int64_t ldw, int64_t colblock,
                         int32_t nranks, int32_t rank);
/* hout2[0] = sum (X-Y)^2, hout2[1] = sum X^2 over an m x n block. Synchronous (host scalars). */
int32_t dhqr_diff_norms_f64(dhqr_ctx *ctx, const double *dX, int64_t ldx, const double *dY, int64_t ldy,
                            int64_t m, int64_t n, double *hout2);

/* ------------------------------------------------------------------ panel level (multi-GPU)
 * The 1-D column-split driver (one process per GPU, torch.distributed/RCCL broadcast of the panel,
 * replacing the per-column @spawnat fan-out of src:141-143) is built from these two calls.
 *
 * Packed panel buffer ("VT"), doubles:  [ V : ldv x DHQR_NB | T : NB x NB | T' : NB x NB | alpha : NB | status : 16 ]
 *   ldv = dhqr_panel_ldv(rows); V is the panel's reflectors with the R part above the diagonal
 *   zeroed and columns >= ncols zero; T is the upper-triangular compact-WY factor
 *   (H_1...H_nb = I - V T V').  dhqr_panel_buffer_elems gives the total length. */
int64_t dhqr_panel_ldv(int64_t rows);
int64_t dhqr_panel_buffer_elems(int64_t rows);

/* Factor the rows x ncols panel dP in place (ncols <= DHQR_NB, rows >= ncols; row 0 of dP is the
 * panel's diagonal row) exactly like src:122-148 restricted to these columns, and emit dVT. Async. */
int32_t dhqr_panel_factor_f64(dhqr_ctx *ctx, double *dP, int64_t rows, int64_t ncols, int64_t ldp,
                              double *dVT);
/* Pack + T only, for a panel that is ALREADY factored (used when Q is re-applied, e.g. to form
 * Q*R for the residual on a column-split matrix). Async. */
int32_t dhqr_panel_pack_f64(dhqr_ctx *ctx, const double *dP, int64_t rows, int64_t ncols, int64_t ldp,
                            double *dVT);
/* dC (rows x ncols) <- (I - V T' V') dC  (trans = 1, the factorisation's trailing update,
 * src:198-213 blocked) or (I - V T V') dC (trans = 0). Async. */
int32_t dhqr_panel_apply_f64(dhqr_ctx *ctx, const double *dVT, int64_t rows, double *dC,
                             int64_t ncols, int64_t ldc, int32_t trans);

/* ------------------------------------------------------------------ multi-GPU: communicators
 * The multi-GPU drivers are SPMD programs: every rank (one per GPU) makes the same sequence of collective calls.
 * A communicator binds a rank to a context and to one of three transports (csrc/dhqr_comm.h):
 *   RCCL      ncclBroadcast / ncclAllReduce over xGMI (librccl.so is dlopen()ed on first use);
 *   LOCAL     peer copies + HIP events between the rank threads of ONE process (dhqr_mg_* when several ranks share
 *             a device, or DHQR_TRANSPORT=local);
 *   CALLBACK  the host layer supplies broadcast / all-reduce (MPI.jl, Distributed.jl, torch.distributed ...).
 * Multi-process use (one Julia worker / one torchrun rank per GPU; replaces the `@spawnat` fan-out of src:141-143
 * and the SharedArray alpha of src:301-304): rank 0 calls dhqr_comm_unique_id, the host layer ships the 128
 * bytes to the other processes, every process calls dhqr_comm_create_rank (collective: ncclCommInitRank). */
#define DHQR_UNIQUE_ID_BYTES 128
#define DHQR_COMM_SELF 0
#define DHQR_COMM_RCCL 1
#define DHQR_COMM_LOCAL 2
#define DHQR_COMM_CALLBACK 3
typedef struct dhqr_comm dhqr_comm;
/* dbuf: device pointer; must return 0 on success.  The library synchronises hip_stream before calling; the
 * callback must have completed (data visible to the device) when it returns. */
typedef int32_t (*dhqr_bcast_fn)(void *user, void *dbuf, int64_t bytes, int32_t root, void *hip_stream);
typedef int32_t (*dhqr_allreduce_fn)(void *user, void *dbuf, int64_t count_f64, void *hip_stream); /* in-place sum */
int32_t dhqr_comm_unique_id(void *id128);
int32_t dhqr_comm_create_rank(dhqr_comm **comm, dhqr_ctx *ctx, int32_t nranks, int32_t rank, const void *id128);
int32_t dhqr_comm_create_callbacks(dhqr_comm **comm, dhqr_ctx *ctx, int32_t nranks, int32_t rank,
                                   dhqr_bcast_fn bcast, dhqr_allreduce_fn allreduce, void *user);
int32_t dhqr_comm_destroy(dhqr_comm *comm);
int32_t dhqr_comm_info(dhqr_comm *comm, int32_t *kind, int32_t *nranks, int32_t *rank, int64_t *bytes_bcast);
/* Collectives this communicator has carried since it was created: out4 = {broadcasts, broadcast bytes, all-reduces, all-reduce
 * bytes} (the row-split lane's channel included).  All-reduces are counted as the drivers ISSUE them -- also at one rank,
 * where they move nothing -- so a single-GPU run reports the count and volume BASELINE.md section 2 asks for. */
int32_t dhqr_comm_counters(dhqr_comm *comm, int64_t *out4);
/* Device time this rank spent in its collectives (one hipEvent pair around every broadcast / all-reduce on the stream that
 * carries it, the wait for the peers included): out4 = {broadcast ms, broadcasts timed, all-reduce ms, all-reduces timed}
 * since the last call; on = 1 / 0 starts / stops collecting, -1 leaves it.  Synchronises the device.  What tells "the
 * broadcast is slow" from "the panel chain is slow" in a multi-GPU run (bench.py prints it per rank). */
int32_t dhqr_comm_timing(dhqr_comm *comm, int32_t on, double *out4);
/* RCCL transport: which algorithm large panel broadcasts use -- 0 ncclBroadcast (rings), 1 scatter + all-gather (the root
 * sends 1/P of the panel to each peer over its own xGMI link, then ncclAllGather) -- and what the timed trial at
 * communicator creation measured for a 16 MiB broadcast with each (ms; 0 when no trial ran: other transports, or
 * DHQR_BCAST=ring|sag set).  dhqr_mg_get_bcast_tuning: the same for rank 0 of a single-process handle. */
int32_t dhqr_comm_get_bcast_tuning(dhqr_comm *comm, int32_t *algo, double *ms_ring, double *ms_scatter_allgather);
/* Rank count RCCL itself reports (ncclCommCount) for the communicator's main channel and for the row-split lane's second
 * channel; 0 = that channel is not an RCCL communicator (other transport, single rank, DHQR_LANE_CHANNEL=0). */
int32_t dhqr_comm_rccl_nranks(dhqr_comm *comm, int32_t *main_channel, int32_t *lane_channel);

/* ------------------------------------------------------------------ multi-GPU: 1-D column split (SPMD, collective)
 * householder!(A::DArray, alpha) (src:115-120).  Layout: BLOCK-CYCLIC columns, block = DHQR_CS_BLOCK (a pair of
 * panels): rank r holds the global column blocks r, r+P, r+2P, ... contiguously (dA: m x dhqr_cs_local_cols(n,P,r), leading dimension lda);
 * dalpha (n) is replicated.  Per panel ONE broadcast of its (V, T, T', alpha) operands replaces the reference's
 * per-column fan-out; trailing updates apply two panels per pass (K = 256 MFMA update) under look-ahead.
 * Every rank of the communicator must make the call.  Synchronous on return.
 *   dhqr_cs_factor_f64     in-place factorisation of the local blocks, alpha on every rank.
 *   dhqr_cs_residual_f64   ||A - QR||_F / ||A||_F with A regenerated from `seed` (dhqr_cs_fill_uniform_f64);
 *                          dW, dA0: m x local_cols scratch matrices (leading dimension m).
 *   dhqr_cs_solve_f64      solve_householder!(b, H, alpha) (src:226-282): db (m, identical on every rank) is
 *                          overwritten, x = db[0:n] on every rank; dwork: m + 128 doubles.  One all-reduce of the
 *                          partial dots per block replaces sum(fetch.(futures)) (src:262-266).
 *   dhqr_cs_load/store_contiguous_f64   convert between the reference's DArray layout (ONE contiguous column
 *                          block per process, dhqr_cs_contiguous_range = DistributedArrays' default split) and the
 *                          block-cyclic layout; dstage: m x max(n/P + 1, 128) doubles.
 *   dhqr_cs_qr_darray_f64  qr!(A::DArray) for one process: host block in, factored host block + alpha out.
 *   dhqr_cs_ldiv_darray_f64  `qrA \ b` for a DArray factorisation (src:317-321 -> src:226-230, 256-270; the call
 *                          test/runtests.jl:77-78 makes): this process's FACTORED contiguous host block, the replicated
 *                          alpha and b (m, the same on every process) in, x (n) out on every process; nothing on the
 *                          host is modified (the reference copies b into a SharedArray, src:318). */
int64_t dhqr_cs_local_cols(int64_t n, int32_t nranks, int32_t rank);
void dhqr_cs_contiguous_range(int64_t n, int32_t nranks, int32_t rank, int64_t *lo, int64_t *hi);
int32_t dhqr_cs_fill_uniform_f64(dhqr_comm *comm, double *dA, int64_t m, int64_t n, int64_t lda, uint64_t seed);
int32_t dhqr_cs_factor_f64(dhqr_comm *comm, double *dA, int64_t m, int64_t n, int64_t lda, double *dalpha);
int32_t dhqr_cs_residual_f64(dhqr_comm *comm, const double *dA, int64_t m, int64_t n, int64_t lda,
                             const double *dalpha, uint64_t seed, double *dW, double *dA0, double *hrel);
int32_t dhqr_cs_solve_f64(dhqr_comm *comm, const double *dA, int64_t m, int64_t n, int64_t lda,
                          const double *dalpha, double *db, double *dwork);
int32_t dhqr_cs_load_contiguous_f64(dhqr_comm *comm, double *dA, int64_t m, int64_t n, int64_t lda,
                                    const double *dBlock, int64_t ldb, double *dstage);
int32_t dhqr_cs_store_contiguous_f64(dhqr_comm *comm, const double *dA, int64_t m, int64_t n, int64_t lda,
                                     double *dBlock, int64_t ldb, double *dstage);
int32_t dhqr_cs_qr_darray_f64(dhqr_comm *comm, double *hBlock, int64_t m, int64_t n, int64_t ldb, double *halpha);
int32_t dhqr_cs_ldiv_darray_f64(dhqr_comm *comm, const double *hBlock, int64_t m, int64_t n, int64_t ldb,
                                const double *halpha, const double *hb, double *hx);

/* ------------------------------------------------------------------ multi-GPU: ComplexF64 column split
 * The reference's householder! is generic over the element type (src:215-294; test/runtests.jl:42-63 runs ComplexF64).
 * Layout: cyclic blocks of 64 complex columns (one panel): rank r holds the global panels r, r+P, r+2P, ...
 * contiguously (dA: m x dhqr_cs_local_cols_c64(n,P,r) complex, interleaved re/im, leading dimension lda complex
 * elements); dalpha (n complex) is replicated.  Per panel ONE broadcast of (alpha, T, T', the factored panel as
 * rows x 64 complex) replaces the per-column fan-out (src:141-143); every rank forms the real 2 x 2 embedding of the 64
 * reflectors itself (twice the bytes, which therefore do not travel); the owner of the next panel looks ahead on a
 * high-priority stream.
 * Every rank of the communicator must make the call.  Asynchronous on the context's stream like dhqr_factor_c64_nb.
 *   dhqr_cs_solve_c64      solve_householder!(b, H, alpha) (src:226-282) on the cyclic layout: db (m complex, identical on
 *                          every rank) is overwritten, x = db[0:n] on every rank; dwork: dhqr_cs_solve_work_c64(m, P)
 *                          complex.  b is carried in double-double (the reference's acceptance statistic sees the
 *                          solve's rounding).  Q'b: two broadcasts of b's tail (high / low parts) per panel; back
 *                          substitution: one all-reduce that gathers the ranks' 64 partial dots
 *                          (sum(fetch.(futures)), src:262-266) + one broadcast of the solved block per panel.
 *   dhqr_cs_qr_darray_c64  qr!(A::DArray{ComplexF64}) for one process: its CONTIGUOUS host column block
 *                          (dhqr_cs_contiguous_range) in, factored block + alpha out; synchronous.
 *   dhqr_cs_ldiv_darray_c64  `qrA \ b` for a DArray{ComplexF64} factorisation (test/runtests.jl:77-78 with T = ComplexF64):
 *                          factored contiguous host block + alpha + b in, x (n complex) out on every process; synchronous.
 *   dhqr_mg_qr_c64   qr!(A; ndev) for a ComplexF64 host matrix (host in / host out).
 *   dhqr_mg_ldiv_c64 `H \ b` for the host-format result over the same devices (dhqr_cs_solve_c64 inside). */
int64_t dhqr_cs_local_cols_c64(int64_t n, int32_t nranks, int32_t rank);
int32_t dhqr_cs_factor_c64(dhqr_comm *comm, double *dA, int64_t m, int64_t n, int64_t lda, double *dalpha);
int64_t dhqr_cs_solve_work_c64(int64_t m, int32_t nranks);
int32_t dhqr_cs_solve_c64(dhqr_comm *comm, const double *dA, int64_t m, int64_t n, int64_t lda,
                          const double *dalpha, double *db, double *dwork);
int32_t dhqr_cs_qr_darray_c64(dhqr_comm *comm, double *hBlock, int64_t m, int64_t n, int64_t ldb, double *halpha);
int32_t dhqr_cs_ldiv_darray_c64(dhqr_comm *comm, const double *hBlock, int64_t m, int64_t n, int64_t ldb,
                                const double *halpha, const double *hb, double *hx);

/* ------------------------------------------------------------------ multi-GPU: single-process handle
 * One host process drives `ndev` GPUs (devices[i] = HIP device of rank i; NULL = 0..ndev-1): one context, one
 * communicator rank and one host thread per device run the SPMD drivers above.  Transport: RCCL
 * (ncclCommInitAll) when the devices are distinct, peer copies otherwise or on DHQR_TRANSPORT=local.
 * What `qr!(A; ndev = 8)` of the Julia module and `python bench.py --gpus N` bind.
 *   dhqr_mg_qr_f64 / dhqr_mg_ldiv_f64    host-in / host-out drop-ins for qr!(A) and `H \ b` (src:311-321).
 *   dhqr_mg_alloc/fill/factor/residual   device-resident path (inputs generated in HBM; what bench.py times).
 *   dhqr_mg_solve_f64                    `\` with the factored matrix resident in the handle. */
typedef struct dhqr_mg dhqr_mg;
int32_t dhqr_mg_create(dhqr_mg **mg, const int32_t *devices, int32_t ndev);
int32_t dhqr_mg_destroy(dhqr_mg *mg);
int32_t dhqr_mg_info(dhqr_mg *mg, int32_t *ndev, int32_t *transport, int64_t *m, int64_t *n);
int32_t dhqr_mg_get_bcast_tuning(dhqr_mg *mg, int32_t *algo, double *ms_ring, double *ms_scatter_allgather);
int32_t dhqr_mg_rccl_nranks(dhqr_mg *mg, int32_t *main_channel, int32_t *lane_channel); /* dhqr_comm_rccl_nranks of rank 0 */
int32_t dhqr_mg_comm_counters(dhqr_mg *mg, int32_t rank, int64_t *out4);                 /* dhqr_comm_counters of one rank */
int32_t dhqr_mg_comm_timing(dhqr_mg *mg, int32_t rank, int32_t on, double *out4);          /* dhqr_comm_timing of one rank */
int32_t dhqr_mg_alloc_f64(dhqr_mg *mg, int64_t m, int64_t n);
int32_t dhqr_mg_fill_uniform_f64(dhqr_mg *mg, uint64_t seed);
int32_t dhqr_mg_factor_f64(dhqr_mg *mg);
int32_t dhqr_mg_residual_f64(dhqr_mg *mg, uint64_t seed, double *hrel);
int32_t dhqr_mg_upload_f64(dhqr_mg *mg, const double *hA, int64_t lda, const double *halpha);
int32_t dhqr_mg_download_f64(dhqr_mg *mg, double *hA, int64_t lda, double *halpha);
int32_t dhqr_mg_qr_f64(dhqr_mg *mg, double *hA, int64_t m, int64_t n, int64_t lda, double *halpha);
int32_t dhqr_mg_qr_c64(dhqr_mg *mg, double *hA, int64_t m, int64_t n, int64_t lda, double *halpha);
int32_t dhqr_mg_ldiv_c64(dhqr_mg *mg, const double *hA, int64_t m, int64_t n, int64_t lda, const double *halpha,
                         const double *hb, double *hx);
int32_t dhqr_mg_solve_f64(dhqr_mg *mg, const double *hb, double *hx);
int32_t dhqr_mg_ldiv_f64(dhqr_mg *mg, const double *hA, int64_t m, int64_t n, int64_t lda, const double *halpha,
                         const double *hb, double *hx);
int32_t dhqr_mg_set_profiling(dhqr_mg *mg, int32_t on);
int32_t dhqr_mg_reset_stats(dhqr_mg *mg);
int32_t dhqr_mg_get_stats(dhqr_mg *mg, int32_t rank, dhqr_stats *out, int64_t *n_fast, int64_t *n_fallback,
                          int64_t *bytes_bcast);

/* ------------------------------------------------------------------ multi-GPU: row split (BASELINE configs[4])
 * Tall-skinny matrices with the ROWS distributed (the reference cannot: `@assert rowrange == 1:size(A,1)`, src:33;
 * its per-column norm / partial dots, src:129,208, would need one cross-rank reduction per column).  SPMD and
 * collective like the column split.  Layout: rank r holds the rows [row0, row0 + mloc) of dhqr_rs_row_range
 * (128-row aligned slabs, so a panel's diagonal block lives on exactly one rank) as an mloc x n column-major
 * block; alpha (n) replicated.  Per 128-column panel: all-reduce of the 128 x 128 Gram matrices, broadcast of the
 * top-block result from the rank holding the diagonal rows, all-reduce of the V'C partial dots (128 x ncols) --
 * the "RCCL all-reduce of the cross-partition partial dots".  Panels are verified on the device; a rejected or
 * partial panel is redone column by column across the ranks (reference algorithm, one small all-reduce + broadcast
 * per column).  Same factor format, distributed by rows.  Synchronous on return.
 *   dhqr_rs_solve_f64: db = this rank's rows of b (overwritten), dx (n) <- x on every rank (src:215-254). */
void dhqr_rs_row_range(int64_t m, int32_t nranks, int32_t rank, int64_t *row0, int64_t *mloc);
int32_t dhqr_rs_fill_uniform_f64(dhqr_comm *comm, double *dA, int64_t m, int64_t n, int64_t lda, uint64_t seed);
int32_t dhqr_rs_factor_f64(dhqr_comm *comm, double *dA, int64_t m, int64_t n, int64_t lda, double *dalpha);
int32_t dhqr_rs_residual_f64(dhqr_comm *comm, const double *dA, int64_t m, int64_t n, int64_t lda,
                             const double *dalpha, uint64_t seed, double *dB, double *dA0, double *hrel);
int32_t dhqr_rs_solve_f64(dhqr_comm *comm, const double *dA, int64_t m, int64_t n, int64_t lda,
                          const double *dalpha, double *db, double *dx);
/* the same through the single-process handle (one host thread per device) */
int32_t dhqr_mg_rs_alloc_f64(dhqr_mg *mg, int64_t m, int64_t n);
int32_t dhqr_mg_rs_fill_uniform_f64(dhqr_mg *mg, uint64_t seed);
int32_t dhqr_mg_rs_factor_f64(dhqr_mg *mg);
int32_t dhqr_mg_rs_residual_f64(dhqr_mg *mg, uint64_t seed, double *hrel);
int32_t dhqr_mg_rs_transfer_f64(dhqr_mg *mg, double *hA, int64_t lda, double *halpha, int32_t upload);
int32_t dhqr_mg_rs_solve_f64(dhqr_mg *mg, const double *hb, double *hx);

/* Micro-benchmarks and the MFMA layout probe are NOT part of this library: include/dhqr_bench.h, libdhqr_bench.so. */

#ifdef __cplusplus
}
#endif
#endif /* DHQR_H */
