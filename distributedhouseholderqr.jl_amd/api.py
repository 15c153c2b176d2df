"""Host-side mirror of the reference's Julia API on top of libdhqr.so.

Reference (src/DistributedHouseholderQR.jl)        here
  qr!(A)                         :311-315          qr_(A, nb=...)             ('!' -> trailing '_')
  DistributedHouseholderQRStruct :296-309          DistributedHouseholderQRStruct(A, α)
  H \\ b                          :317-321          ldiv(H, b)  /  H.solve(b)   (b a vector, or a matrix of right-hand sides)
  householder!(A, α)             :113-120          householder_(A, α, nb=...)
  solve_householder!(b, H, α)    :284-294          solve_householder_(b, H, α)
  partialdot(a, b, is, T)        :42-49, :51-59    partialdot(a, b, lo, hi)

The reference's functions are generic over the element type (its tests run Float64 and ComplexF64,
test/runtests.jl:43); here the dtype of the argument selects the method the same way: float64 ->
the *_f64 entry points (blocked MFMA path by default), complex128 -> the *_c64 entry points
(unblocked path; nb must be None or 0).

Inputs are either host numpy arrays (column-major float64; goes through the host-in/host-out
C entry points, like qr!(::Matrix)) or CUDA/HIP torch tensors in column-major layout
(stride(0) == 1; device-resident entry points).  PyTorch is only plumbing here (device memory and
streams); every FLOP runs in the HIP library.  No CPU fallback exists.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional

import numpy as np

from . import _lib
from ._lib import NB, DHQRError, Stats, check

try:  # torch is only needed for device-resident tensors
    import torch
except Exception:  # pragma: no cover
    torch = None


class Context:
    """One dhqr_ctx per (process, GPU)."""

    def __init__(self, device: int = 0):
        self._h = ctypes.c_void_p()
        self.device = device
        check(_lib.lib().dhqr_create(ctypes.byref(self._h), device))

    @property
    def handle(self):
        return self._h

    def use_torch_stream(self):
        """run on torch's current stream of this device (so torch ops and dhqr kernels order).  DHQR_OWN_STREAM=1
        (experiments): keep the context's own stream; the caller then orders with torch by synchronising."""
        if os.environ.get("DHQR_OWN_STREAM") == "1":
            check(_lib.lib().dhqr_use_own_stream(self._h))
            return
        s = torch.cuda.current_stream(self.device).cuda_stream
        check(_lib.lib().dhqr_set_stream(self._h, ctypes.c_void_p(s)))

    def synchronize(self):
        check(_lib.lib().dhqr_synchronize(self._h))

    def trim(self):
        """release the device copy / staging buffers / solve workspaces the context keeps between calls (dhqr_trim)"""
        check(_lib.lib().dhqr_trim(self._h))

    def set_profiling(self, on: bool):
        check(_lib.lib().dhqr_set_profiling(self._h, 1 if on else 0))

    def reset_stats(self):
        check(_lib.lib().dhqr_reset_stats(self._h))

    def stats(self) -> dict:
        st = Stats()
        check(_lib.lib().dhqr_get_stats(self._h, ctypes.byref(st)))
        return st.asdict()

    def panel_counters(self):
        """(panels done by the R-first fast path, panels that fell back to the step kernels)"""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(_lib.lib().dhqr_get_panel_counters(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_r_source(self, source: int):
        """1 Gram/Cholesky (default), 2 CholeskyQR2, 3 TSQR-HR (csrc/dhqr_tsqr.h) for the R-first panel path"""
        check(_lib.lib().dhqr_set_r_source(self._h, int(source)))

    def set_tsqr_rung(self, on: bool):
        """False: rejected panels skip the TSQR-HR rung (straight to the column-by-column kernels)"""
        check(_lib.lib().dhqr_set_tsqr_rung(self._h, 1 if on else 0))

    def set_small_route(self, on: bool):
        """False: matrices that fit one compute unit's registers go through the general drivers too (csrc/dhqr_small.h)"""
        check(_lib.lib().dhqr_set_small_route(self._h, 1 if on else 0))

    def solve_retries(self) -> int:
        """solves repeated with the per-step kernels after a wait of the persistent Q'b kernel expired (dhqr.h)"""
        a = ctypes.c_int64()
        check(_lib.lib().dhqr_get_solve_retries(self._h, ctypes.byref(a)))
        return a.value

    def tsqr_count(self) -> int:
        a = ctypes.c_int64()
        check(_lib.lib().dhqr_get_tsqr_count(self._h, ctypes.byref(a)))
        return a.value

    def close(self):
        if self._h:
            _lib.lib().dhqr_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


_contexts: Dict[int, Context] = {}


def get_context(device: Optional[int] = None) -> Context:
    if device is None:
        device = torch.cuda.current_device() if (torch is not None and torch.cuda.is_available()) else 0
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]


# ------------------------------------------------------------------------------- helpers
def _is_tensor(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def _is_complex(x) -> bool:
    if _is_tensor(x):
        return x.dtype == torch.complex128
    return isinstance(x, np.ndarray) and x.dtype == np.complex128


def _is_f32(x) -> bool:
    if _is_tensor(x):
        return x.dtype == torch.float32
    return isinstance(x, np.ndarray) and x.dtype == np.float32


def _same_dtype(A, v, name):
    """Float32 and Float64 methods are separate (the reference dispatches on the element type): a float32 matrix with a
    float64 vector, or the reverse, is a TypeError, never a silent conversion -- also on the Float64 paths, which used to
    convert a float32 host `b` quietly"""
    dt = getattr(v, "dtype", None)
    real = (np.float32, np.float64) if torch is None else (torch.float32, torch.float64, np.float32, np.float64)
    if dt is not None and any(dt == t for t in real) and _is_f32(A) != _is_f32(v):
        raise TypeError(f"{name} is {dt} but the matrix is {A.dtype}: convert one of them explicitly")


def _same_field(A, v, name):
    """the ComplexF64 methods are separate from the real ones: a real vector with a complex matrix, or the reverse, is a
    TypeError, never a silent conversion (of a real b) or a dropped imaginary part (of a complex one)"""
    dt = getattr(v, "dtype", None)
    if dt is not None and _is_complex(A) != (dt == np.complex128 or (torch is not None and dt == torch.complex128)):
        raise TypeError(f"{name} is {dt} but the matrix is {A.dtype}: convert one of them explicitly")


def _resolve_dtype(dtype):
    """torch dtype of a `dtype` argument (None = float64, today's behaviour); float32 and float64 in torch's or numpy's spelling"""
    if dtype is None or dtype in (torch.float64, np.float64, "float64"):
        return torch.float64
    if dtype in (torch.float32, np.float32, "float32"):
        return torch.float32
    raise TypeError(f"dtype must be float64 or float32, got {dtype!r}")


def _host_ld(F) -> int:
    """leading dimension (in elements) of a column-major host matrix; numpy's relaxed strides report an
    arbitrary stride for a single column, where the reference's Matrix simply has ld = m"""
    m, n = F.shape
    return F.strides[1] // F.itemsize if n > 1 else max(m, 1)


DEFAULT_UNBLOCKED_MAX_ROWS = 480  # Float64: at most this many rows -> nb = 0 by default (tools/mid_bench.py)


def _resolve_nb(A, nb):
    """nb=None: the default of the element type (Float64: 128 blocked, but the reference's unblocked order up to 480 rows,
    where the K-reflector passes finish before the blocked driver's panel chains do: 440 x 400 1.46 ms against 1.53,
    300 x 260 0.97 against 1.00, 520 x 512 1.86 against 1.49 the other way, profiles/r06_mid_sizes.txt; ComplexF64: 64
    blocked -- the trailing update runs on the FP64 MFMA kernels through the real embedding -- for n >= 256, unblocked
    below)"""
    if _is_complex(A):
        if nb not in (None, 0, _lib.ZNB):
            raise ValueError(f"ComplexF64: nb must be None, 0 (unblocked) or {_lib.ZNB} (blocked)")
        if nb is None:
            return _lib.ZNB if A.shape[-1] >= 256 else 0  # (a batch (batch, m, n): the shape of its matrices)
        return nb
    if nb is None:
        return 0 if A.shape[-2] <= DEFAULT_UNBLOCKED_MAX_ROWS else NB
    return nb


def _dev_matrix(A, dtype=None):
    """(ptr, m, n, lda, device) of a column-major CUDA tensor (float64 unless `dtype` is given);
    lda counts elements."""
    dtype = torch.float64 if dtype is None else dtype
    if A.dtype != dtype or not A.is_cuda:
        raise TypeError(f"device path needs a {dtype} CUDA tensor")
    if A.dim() != 2:
        raise ValueError("matrix expected")
    m, n = A.shape
    if m > 1 and A.stride(0) != 1:
        raise ValueError("column-major layout required (stride(0) == 1); build it with "
                         "empty_colmajor(m, n) or X.t() of a contiguous (n, m) tensor")
    lda = A.stride(1) if n > 1 else max(m, 1)
    return ctypes.c_void_p(A.data_ptr()), m, n, lda, A.device.index


def _dev_vector(v, length=None, dtype=None):
    dtype = torch.float64 if dtype is None else dtype
    if v.dtype != dtype or not v.is_cuda or v.dim() != 1 or (v.numel() > 1 and v.stride(0) != 1):
        raise TypeError(f"contiguous {dtype} CUDA vector expected")
    if length is not None and v.numel() < length:
        raise ValueError(f"vector shorter than {length}")
    return ctypes.c_void_p(v.data_ptr())


def empty_colmajor(m: int, n: int, device="cuda", dtype=None):
    """uninitialised m x n float64 (or dtype=float32) device matrix in column-major layout (lda = m)."""
    return torch.empty((n, m), dtype=_resolve_dtype(dtype), device=device).t()


def rand_colmajor(m: int, n: int, seed: int, device="cuda", *, global_m=None, row0=0, colblock=NB,
                  nranks=1, rank=0, dtype=None):
    """Device-side synthetic input: A[i,j] = u01(seed, gi + gj*global_m), the generator shared with
    oracle/ (stands in for rand(T,m,n), test/runtests.jl:45).  With nranks > 1 fills the LOCAL
    block of a block-cyclic column layout.  dtype=float32: the same Float64 values, rounded."""
    if _resolve_dtype(dtype) == torch.float32:
        A64 = rand_colmajor(m, n, seed, device, global_m=global_m, row0=row0, colblock=colblock, nranks=nranks, rank=rank)
        A = empty_colmajor(m, n, device, torch.float32)
        A.copy_(A64)
        return A
    A = empty_colmajor(m, n, device)
    ctx = get_context(A.device.index)
    ctx.use_torch_stream()
    ptr, m_, n_, lda, _ = _dev_matrix(A)
    check(_lib.lib().dhqr_fill_uniform_f64(ctx.handle, ptr, m_, n_, lda, seed,
                                           global_m if global_m is not None else m, row0, colblock,
                                           nranks, rank))
    return A


def rand_vector_device(m: int, seed: int, device="cuda"):
    return rand_colmajor(m, 1, seed, device).reshape(-1)


def rand_colmajor_c(m: int, n: int, seed: int, device="cuda"):
    """rand(ComplexF64, m, n) stand-in on the device: the Float64 generator run over the
    interleaved 2m x n real view, A[i,j] = u01(seed, 2(i + j m)) + im*u01(seed, 2(i + j m) + 1)
    (identical to oracle rand_matrix_c)."""
    A = torch.empty((n, m), dtype=torch.complex128, device=device).t()
    ctx = get_context(A.device.index)
    ctx.use_torch_stream()
    check(_lib.lib().dhqr_fill_uniform_f64(ctx.handle, ctypes.c_void_p(A.data_ptr()), 2 * m, n, 2 * m, seed,
                                           2 * m, 0, NB, 1, 0))
    return A


# ------------------------------------------------------------------------------- API mirror
class DistributedHouseholderQRStruct:
    """src:296-309: the factored matrix `A` (V on/below the diagonal, R strictly above) and
    `α` = diag(R).  `alpha` is an ASCII alias of `α`.  `jpvt`: None, or the (batch, n) int32 column permutation of a
    pivoted factorisation (qr_pivoted_batched_): A[k][:, jpvt[k]] = Q[k] R[k]."""

    def __init__(self, A, α=None, jpvt=None):
        self.A = A
        self.jpvt = jpvt
        if α is None:  # src:306-309  α = zeros(eltype(A), size(A, 2)); a batch (batch, m, n) has one α per matrix: (batch, n)
            shape = tuple(A.shape[:-2]) + (A.shape[-1],)
            α = torch.zeros(shape, dtype=A.dtype, device=A.device) if _is_tensor(A) else np.zeros(shape, dtype=A.dtype)
        self.α = α

    @property
    def alpha(self):
        return self.α

    def solve(self, b):
        return ldiv(self, b)

    def __repr__(self):
        return f"DistributedHouseholderQRStruct(A={tuple(self.A.shape)}, α={tuple(self.α.shape)})"


def _householder_c64(A, α, nb=0):
    """ComplexF64 method of householder! (src:9, 51-59, 122-148, 171-213): nb = 0 unblocked, 64 blocked.  Up to 128 rows with
    the small route on, whatever nb: ONE launch (the batched tiers on a batch of one; host arrays through the context's
    pinned staging buffer)."""
    L = _lib.lib()
    if _is_tensor(A):
        ptr, m, n, lda, dev = _dev_matrix(A, torch.complex128)
        ctx = get_context(dev)
        ctx.use_torch_stream()
        check(L.dhqr_factor_c64_nb(ctx.handle, ptr, m, n, lda, _dev_vector(α, n, torch.complex128), nb))
        ctx.synchronize()  # qr! is synchronous in the reference; this also collects a pipeline hand-over error (dhqr.h)
        return A, α
    if not isinstance(α, np.ndarray) or α.dtype != np.complex128 or α.size < A.shape[1] or not α.flags.c_contiguous:
        raise TypeError("α must be a contiguous complex128 numpy vector of length n")
    m, n = A.shape
    F = A if A.flags.f_contiguous else np.asfortranarray(A)
    check(L.dhqr_qr_c64_nb(get_context().handle, F.ctypes.data_as(ctypes.c_void_p), m, n,
                           _host_ld(F), α.ctypes.data_as(ctypes.c_void_p), nb))
    if F is not A:
        A[...] = F
    return A, α


def _householder_f32(A, α, nb):
    """Float32 method of householder! (dhqr_factor_f32 / dhqr_qr_f32): native kernels up to 64 x 32, promoted beyond"""
    L = _lib.lib()
    _same_dtype(A, α, "α")
    if _is_tensor(A):
        ptr, m, n, lda, dev = _dev_matrix(A, torch.float32)
        ctx = get_context(dev)
        ctx.use_torch_stream()
        check(L.dhqr_factor_f32(ctx.handle, ptr, m, n, lda, _dev_vector(α, n, torch.float32), nb))
        ctx.synchronize()
        return A, α
    if A.ndim != 2:
        raise TypeError("float32 numpy matrix or CUDA tensor expected")
    if not isinstance(α, np.ndarray) or α.dtype != np.float32 or α.size < A.shape[1] or not α.flags.c_contiguous:
        raise TypeError("α must be a contiguous float32 numpy vector of length n")
    m, n = A.shape
    F = A if A.flags.f_contiguous else np.asfortranarray(A)
    check(L.dhqr_qr_f32(get_context().handle, F.ctypes.data_as(ctypes.c_void_p), m, n, _host_ld(F),
                        α.ctypes.data_as(ctypes.c_void_p), nb))
    if F is not A:
        A[...] = F
    return A, α


def householder_(A, α, nb: Optional[int] = None):
    """householder!(A, α) (src:113): factor A in place, fill α. nb=0 -> unblocked rank-1 path
    (the reference's algorithm verbatim), nb=128 -> blocked MFMA path (the Float64 default).
    complex128 input selects the ComplexF64 method (unblocked). Returns (A, α)."""
    L = _lib.lib()
    nb = _resolve_nb(A, nb)
    if _is_complex(A):
        return _householder_c64(A, α, nb)
    if _is_f32(A):
        return _householder_f32(A, α, nb)
    if _is_tensor(A):
        _same_dtype(A, α, "α")
        ptr, m, n, lda, dev = _dev_matrix(A)
        ctx = get_context(dev)
        ctx.use_torch_stream()
        check(L.dhqr_factor_f64(ctx.handle, ptr, m, n, lda, _dev_vector(α, n), nb))
        if nb == 0:  # the unblocked path is fully asynchronous and uses the inter-workgroup lead pipeline: its error word
            ctx.synchronize()  # is only reported by a synchronising entry point (the blocked driver reads it itself)
        return A, α
    if not isinstance(A, np.ndarray) or A.dtype != np.float64 or A.ndim != 2:
        raise TypeError("float64 numpy matrix or CUDA tensor expected")
    if not isinstance(α, np.ndarray) or α.dtype != np.float64 or α.size < A.shape[1] or not α.flags.c_contiguous:
        raise TypeError("α must be a contiguous float64 numpy vector of length n")
    m, n = A.shape
    ctx = get_context()
    F = A if A.flags.f_contiguous else np.asfortranarray(A)
    check(L.dhqr_qr_f64(ctx.handle, F.ctypes.data_as(ctypes.c_void_p), m, n, _host_ld(F),
                        α.ctypes.data_as(ctypes.c_void_p), nb))
    if F is not A:
        A[...] = F  # in-place semantics of qr! for row-major callers
    return A, α


def qr_(A, nb: Optional[int] = None) -> DistributedHouseholderQRStruct:
    """qr!(A) (src:311-315): mutates A, returns the struct."""
    H = DistributedHouseholderQRStruct(A)
    householder_(H.A, H.α, nb=nb)
    return H


def _solve_nrhs(B, H, α):
    """solve_householder!(B, H, α) for a MATRIX B (m, nrhs) of right-hand sides and one real factor (a batch of 1 of
    dhqr_solve_batched_nrhs_* / dhqr_ldiv_batched_nrhs_*): returns X (n, nrhs), column-major.  A device B (column-major) is
    overwritten with [X; tail of Q'B]; a host B in any layout is left untouched."""
    L = _lib.lib()
    f32 = _is_f32(H)
    if _is_tensor(H):
        dt = torch.float32 if f32 else torch.float64
        ptr, m, n, lda, dev = _dev_matrix(H, dt)
        if not _is_tensor(B):
            raise TypeError(f"column-major {dt} CUDA tensor of shape ({m}, nrhs) expected")
        bptr, mb, nrhs, ldb, _ = _dev_matrix(B, dt)
        if mb != m:
            raise ValueError(f"B has {mb} rows, the factor {m}")
        solve = L.dhqr_solve_batched_nrhs_f32 if f32 else L.dhqr_solve_batched_nrhs_f64
        ctx = get_context(dev)
        ctx.use_torch_stream()
        check(solve(ctx.handle, ptr, m, n, lda, max(lda * (n - 1) + m, 1), _dev_vector(α, n, dt), max(n, 1),
                    bptr, nrhs, ldb, max(ldb * (nrhs - 1) + m, 1), 1))
        ctx.synchronize()
        X = empty_colmajor(n, nrhs, B.device, dt)
        X.copy_(B[:n])
        return X
    dt = np.float32 if f32 else np.float64
    m, n = H.shape
    F = H if H.flags.f_contiguous else np.asfortranarray(H)
    Bf = np.asfortranarray(B, dtype=dt)  # (a copy only where the layout asks for one; never written)
    if Bf.ndim != 2 or Bf.shape[0] != m:
        raise ValueError(f"B must have shape ({m}, nrhs)")
    nrhs = Bf.shape[1]
    X = np.empty((n, nrhs), dtype=dt, order="F")
    ldiv_ = L.dhqr_ldiv_batched_nrhs_f32 if f32 else L.dhqr_ldiv_batched_nrhs_f64
    check(ldiv_(get_context().handle, F.ctypes.data_as(ctypes.c_void_p), m, n, _host_ld(F), max(_host_ld(F) * (n - 1) + m, 1),
                np.ascontiguousarray(α, dtype=dt).ctypes.data_as(ctypes.c_void_p), max(n, 1),
                Bf.ctypes.data_as(ctypes.c_void_p), nrhs, max(m, 1), max(m * nrhs, 1),
                X.ctypes.data_as(ctypes.c_void_p), max(n, 1), max(n * nrhs, 1), 1))
    return X


def solve_householder_(b, H, α):
    """solve_householder!(b, H, α) (src:284-294): returns x = b[1:n] (a copy, like Julia's b[1:n]).  A device
    tensor b is overwritten like the reference's b (b <- Q'b, then back substitution in place); a HOST b is
    uploaded and left untouched (the solve happens in device memory).  A matrix b (m, nrhs) -- column-major on the
    device, any layout on the host -- solves all its columns in one call and returns X (n, nrhs), column-major;
    Float64 and Float32.  Column r of X has the bits of ldiv_batched on a batch of one with the vector b[:, r].  For a
    Float64 factor of at most 64 x 32 that is NOT the route a vector b takes here (dhqr_solve_f64: the one-workgroup
    kernel, against the wave kernel of the batched entry points), so X[:, r] and solve_householder_(b[:, r], H, α) may
    differ in the last bits there; beyond those shapes, and in Float32, they are identical."""
    L = _lib.lib()
    if getattr(b, "ndim", 1) == 2 and H.ndim == 2:
        if _is_complex(H):
            raise TypeError("ComplexF64: vector right-hand side only")
        _same_dtype(H, α, "α")
        _same_dtype(H, b, "b")
        return _solve_nrhs(b, H, α)
    if _is_complex(H):
        if _is_tensor(H):
            ptr, m, n, lda, dev = _dev_matrix(H, torch.complex128)
            ctx = get_context(dev)
            ctx.use_torch_stream()
            check(L.dhqr_solve_c64(ctx.handle, ptr, m, n, lda, _dev_vector(α, n, torch.complex128),
                                   _dev_vector(b, m, torch.complex128)))
            x = b[:n].clone()
            ctx.synchronize()
            return x
        m, n = H.shape
        F = H if H.flags.f_contiguous else np.asfortranarray(H)
        x = np.empty(n, dtype=np.complex128)
        bb = np.ascontiguousarray(b, dtype=np.complex128)
        check(L.dhqr_ldiv_c64(get_context().handle, F.ctypes.data_as(ctypes.c_void_p), m, n,
                              _host_ld(F),
                              np.ascontiguousarray(α, dtype=np.complex128).ctypes.data_as(ctypes.c_void_p),
                              bb.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p)))
        return x
    _same_dtype(H, α, "α")
    _same_dtype(H, b, "b")
    if _is_f32(H):
        if _is_tensor(H):
            ptr, m, n, lda, dev = _dev_matrix(H, torch.float32)
            ctx = get_context(dev)
            ctx.use_torch_stream()
            check(L.dhqr_solve_f32(ctx.handle, ptr, m, n, lda, _dev_vector(α, n, torch.float32), _dev_vector(b, m, torch.float32)))
            ctx.synchronize()
            return b[:n].clone()
        m, n = H.shape
        F = H if H.flags.f_contiguous else np.asfortranarray(H)
        x = np.empty(n, dtype=np.float32)
        bb = np.ascontiguousarray(b, dtype=np.float32)
        check(L.dhqr_ldiv_f32(get_context().handle, F.ctypes.data_as(ctypes.c_void_p), m, n, _host_ld(F),
                              np.ascontiguousarray(α, dtype=np.float32).ctypes.data_as(ctypes.c_void_p),
                              bb.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p)))
        return x
    if _is_tensor(H):
        ptr, m, n, lda, dev = _dev_matrix(H)
        ctx = get_context(dev)
        ctx.use_torch_stream()
        check(L.dhqr_solve_f64(ctx.handle, ptr, m, n, lda, _dev_vector(α, n), _dev_vector(b, m)))
        ctx.synchronize()  # an expired hand-over wait is reported here -- or the solve repeated without the persistent kernel (dhqr.h)
        return b[:n].clone()
    m, n = H.shape
    F = H if H.flags.f_contiguous else np.asfortranarray(H)
    x = np.empty(n)
    bb = np.ascontiguousarray(b, dtype=np.float64)
    ctx = get_context()
    check(L.dhqr_ldiv_f64(ctx.handle, F.ctypes.data_as(ctypes.c_void_p), m, n, _host_ld(F),
                          np.ascontiguousarray(α).ctypes.data_as(ctypes.c_void_p),
                          bb.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p)))
    return x


def ldiv(H: DistributedHouseholderQRStruct, b):
    """`H \\ b` (src:317-321): least-squares solution of length n; the caller's b is NOT modified
    (the reference copies it into a SharedArray first, src:318).  `H \\ B` with a matrix B of as many dimensions as H.A
    -- (m, nrhs), or (batch, m, nrhs) for a batch -- solves every column: X (n, nrhs) / (batch, n, nrhs), column-major.
    X[..., r] has the bits of ldiv_batched on the vectors B[..., r] (a single matrix: a batch of one).  ldiv(H, B[:, r]) of one
    Float64 factor of at most 64 x 32 runs another kernel and may differ from X[:, r] in the last bits (solve_householder_)."""
    if H.A.ndim == 3:
        return ldiv_batched(H, b)
    if _is_tensor(H.A) and _is_tensor(b) and b.dim() == 2 and not _is_complex(H.A):
        _same_dtype(H.A, b, "b")
        _dev_matrix(b, H.A.dtype)  # (the dtype and layout rules, before the copy hides them)
        W = empty_colmajor(b.shape[0], b.shape[1], b.device, H.A.dtype)
        W.copy_(b)  # src:318 copy of B
        return solve_householder_(W, H.A, H.α)
    if _is_tensor(H.A):
        return solve_householder_(b.clone(), H.A, H.α)
    return solve_householder_(b, H.A, H.α)


# ------------------------------------------------------------------------------- batches of small matrices
def empty_colmajor_batched(batch: int, m: int, n: int, device="cuda", dtype=None):
    """uninitialised (batch, m, n) float64 (or dtype=float32) device tensor whose matrices are column-major (stride(1) == 1, lda = m)."""
    return torch.empty((batch, n, m), dtype=_resolve_dtype(dtype), device=device).transpose(1, 2)


def rand_colmajor_batched(batch: int, m: int, n: int, seed: int, device="cuda", dtype=None):
    """matrix k = rand_colmajor(m, n, seed + k): the shared generator, so the oracle's rand_matrix(m, n, seed + k) is its twin.
    dtype=float32: the same Float64 values, rounded."""
    if _resolve_dtype(dtype) == torch.float32:
        A = empty_colmajor_batched(batch, m, n, device, torch.float32)
        A.copy_(rand_colmajor_batched(batch, m, n, seed, device))
        return A
    A = empty_colmajor_batched(batch, m, n, device)
    ctx = get_context(A.device.index)
    ctx.use_torch_stream()
    L = _lib.lib()
    for k in range(batch):
        check(L.dhqr_fill_uniform_f64(ctx.handle, ctypes.c_void_p(A[k].data_ptr()), m, n, m, seed + k, m, 0, NB, 1, 0))
    return A


def empty_colmajor_batched_c(batch: int, m: int, n: int, device="cuda"):
    """uninitialised (batch, m, n) complex128 device tensor whose matrices are column-major (stride(1) == 1, lda = m)."""
    return torch.empty((batch, n, m), dtype=torch.complex128, device=device).transpose(1, 2)


def rand_colmajor_batched_c(batch: int, m: int, n: int, seed: int, device="cuda"):
    """matrix k = rand_colmajor_c(m, n, seed + k): the shared generator over the interleaved real view, so the oracle's
    rand_matrix_c(m, n, seed + k) is its twin."""
    A = empty_colmajor_batched_c(batch, m, n, device)
    ctx = get_context(A.device.index)
    ctx.use_torch_stream()
    L = _lib.lib()
    for k in range(batch):
        check(L.dhqr_fill_uniform_f64(ctx.handle, ctypes.c_void_p(A[k].data_ptr()), 2 * m, n, 2 * m, seed + k, 2 * m, 0, NB, 1, 0))
    return A


def _batch_layout(shape, strides):
    """(lda, strideA) in elements of a (batch, m, n) array whose matrices are column-major, else None"""
    batch, m, n = shape
    s0, s1, s2 = strides
    if m > 1 and s1 != 1:
        return None
    lda = s2 if n > 1 else max(m, 1)
    if lda < max(m, 1):
        return None
    need = lda * (n - 1) + m
    strideA = s0 if batch > 1 else max(need, 1)
    return (lda, strideA) if strideA >= need else None


def _host_rows(v, batch, length, name, dtype=np.float64):
    """(array, row stride in elements) of a (batch, length) float64 (or `dtype`) host array with contiguous rows"""
    v = np.asarray(v, dtype=dtype)
    if v.shape != (batch, length):
        raise ValueError(f"{name} must have shape ({batch}, {length})")
    if (length > 1 and v.strides[1] != v.itemsize) or (batch > 1 and (v.strides[0] % v.itemsize or v.strides[0] < length * v.itemsize)):
        v = np.ascontiguousarray(v)
    return v, (v.strides[0] // v.itemsize if batch > 1 else max(length, 1))


def qr_batched_(A, nb: Optional[int] = None) -> DistributedHouseholderQRStruct:
    """qr!(A[k]) for every matrix of a (batch, m, n) float64 batch in ONE call (dhqr_factor_batched_f64 /
    dhqr_qr_batched_f64): one wave per matrix up to 64 x 32, one workgroup per matrix up to the small route's shapes, a
    serial loop beyond.  A is a CUDA tensor whose matrices are column-major (empty_colmajor_batched) or a numpy array; a
    host array in another layout is copied to that layout and back.  Mutates A; returns the struct with α of shape (batch, n).
    float32: dhqr_*_batched_f32.  complex128 (empty_colmajor_batched_c): dhqr_factor_batched_c64 / dhqr_qr_batched_c64 -- one
    wave per matrix up to 64 x 32, one workgroup per matrix up to 128 rows (both one asynchronous launch, nb ignored), a
    serial loop of single factorisations beyond; nb is None, 0 or ZNB (_resolve_nb)."""
    L = _lib.lib()
    if A.ndim != 3:
        raise ValueError("(batch, m, n) array expected")
    batch, m, n = A.shape
    cplx = _is_complex(A)
    if cplx:
        nb = _resolve_nb(A, nb)
    elif nb is None:
        nb = 0 if m <= DEFAULT_UNBLOCKED_MAX_ROWS else NB
    f32 = _is_f32(A)
    factor, qr = ((L.dhqr_factor_batched_c64, L.dhqr_qr_batched_c64) if cplx else
                  (L.dhqr_factor_batched_f32, L.dhqr_qr_batched_f32) if f32 else (L.dhqr_factor_batched_f64, L.dhqr_qr_batched_f64))
    if _is_tensor(A):
        if A.dtype not in (torch.float64, torch.float32, torch.complex128) or not A.is_cuda:
            raise TypeError("device path needs a float64, float32 or complex128 CUDA tensor")
        lay = _batch_layout(A.shape, A.stride())
        if lay is None:
            raise ValueError("matrices of the batch must be column-major (stride(1) == 1); build it with empty_colmajor_batched")
        H = DistributedHouseholderQRStruct(A)
        ctx = get_context(A.device.index)
        ctx.use_torch_stream()
        check(factor(ctx.handle, ctypes.c_void_p(A.data_ptr()), m, n, lay[0], lay[1],
                                        ctypes.c_void_p(H.α.data_ptr()), max(n, 1), batch, nb))
        ctx.synchronize()
        return H
    if not isinstance(A, np.ndarray) or A.dtype not in (np.float64, np.float32, np.complex128):
        raise TypeError("float64, float32 or complex128 numpy array or CUDA tensor expected")
    F, lda, strideA = _host_batch(A)
    H = DistributedHouseholderQRStruct(A)
    check(qr(get_context().handle, F.ctypes.data_as(ctypes.c_void_p), m, n, lda, strideA,
                                H.α.ctypes.data_as(ctypes.c_void_p), max(n, 1), batch, nb))
    if F is not A:
        A[...] = F
    return H


def _host_batch(A):
    """(array, lda, strideA) of a (batch, rows, cols) host array with column-major matrices: A itself where its layout
    allows, else a copy in that layout"""
    batch, rows, cols = A.shape
    lay = None
    if all(st % A.itemsize == 0 and st >= 0 for st in A.strides):
        lay = _batch_layout(A.shape, tuple(st // A.itemsize for st in A.strides))
    if lay is not None:
        return A, lay[0], lay[1]
    F = np.empty((batch, cols, rows), dtype=A.dtype).transpose(0, 2, 1)
    F[...] = A
    return F, max(rows, 1), max(rows * cols, 1)


def _ldiv_batched_nrhs(H: DistributedHouseholderQRStruct, B):
    """ldiv_batched for B (batch, m, nrhs): dhqr_solve_batched_nrhs_* on a copy of a device B, dhqr_ldiv_batched_nrhs_*
    on a host B; X (batch, n, nrhs) with column-major matrices"""
    L = _lib.lib()
    A, α = H.A, H.α
    batch, m, n = A.shape
    f32 = _is_f32(A)
    solve, ldiv_ = ((L.dhqr_solve_batched_nrhs_f32, L.dhqr_ldiv_batched_nrhs_f32) if f32
                    else (L.dhqr_solve_batched_nrhs_f64, L.dhqr_ldiv_batched_nrhs_f64))
    if _is_tensor(A):
        lay = _batch_layout(A.shape, A.stride())
        if lay is None:
            raise ValueError("matrices of the batch must be column-major (stride(1) == 1)")
        if not _is_tensor(B) or B.dtype != A.dtype or not B.is_cuda or tuple(B.shape[:2]) != (batch, m):
            raise TypeError(f"{A.dtype} CUDA tensor of shape ({batch}, {m}, nrhs) expected")
        if _batch_layout(B.shape, B.stride()) is None:
            raise ValueError("matrices of B must be column-major (stride(1) == 1); build it with empty_colmajor_batched")
        if α.dtype != A.dtype or tuple(α.shape) != (batch, n) or not α.is_contiguous():
            raise TypeError(f"α must be a contiguous {A.dtype} tensor of shape ({batch}, {n})")
        nrhs = B.shape[2]
        W = empty_colmajor_batched(batch, m, nrhs, B.device, A.dtype)
        W.copy_(B)  # src:318 copy of B
        ctx = get_context(A.device.index)
        ctx.use_torch_stream()
        check(solve(ctx.handle, ctypes.c_void_p(A.data_ptr()), m, n, lay[0], lay[1], ctypes.c_void_p(α.data_ptr()), max(n, 1),
                    ctypes.c_void_p(W.data_ptr()), nrhs, max(m, 1), max(m * nrhs, 1), batch))
        ctx.synchronize()
        X = empty_colmajor_batched(batch, n, nrhs, B.device, A.dtype)
        X.copy_(W[:, :n, :])
        return X
    B = np.asarray(B, dtype=A.dtype)
    if B.shape[:2] != (batch, m):
        raise ValueError(f"B must have shape ({batch}, {m}, nrhs)")
    nrhs = B.shape[2]
    F, lda, strideA = _host_batch(A)
    Bf, ldb, strideB = _host_batch(B)
    al, sal = _host_rows(α, batch, n, "α", A.dtype)
    X = np.empty((batch, nrhs, n), dtype=A.dtype).transpose(0, 2, 1)
    check(ldiv_(get_context().handle, F.ctypes.data_as(ctypes.c_void_p), m, n, lda, strideA,
                al.ctypes.data_as(ctypes.c_void_p), sal, Bf.ctypes.data_as(ctypes.c_void_p), nrhs, ldb, strideB,
                X.ctypes.data_as(ctypes.c_void_p), max(n, 1), max(n * nrhs, 1), batch))
    return X


def ldiv_batched(H: DistributedHouseholderQRStruct, b):
    """`H[k] \\ b[k]` for every matrix of a batched factorisation: b (batch, m) -> x (batch, n); b is NOT modified.
    b (batch, m, nrhs), its matrices column-major like A's: every column of every b[k] -> X (batch, n, nrhs); real factors
    only -- a complex128 factor takes b (batch, m) complex128 (dhqr_solve_batched_c64 / dhqr_ldiv_batched_c64)."""
    L = _lib.lib()
    A, α = H.A, H.α
    if A.ndim != 3:
        raise ValueError("batched factorisation expected")
    batch, m, n = A.shape
    f32 = _is_f32(A)
    cplx = _is_complex(A)
    _same_dtype(A, α, "α")
    _same_dtype(A, b, "b")
    _same_field(A, α, "α")
    _same_field(A, b, "b")
    if getattr(b, "ndim", 2) == 3:
        if cplx:
            raise TypeError("ComplexF64: vector right-hand side only")
        return _ldiv_batched_nrhs(H, b)
    solve, ldiv_ = ((L.dhqr_solve_batched_c64, L.dhqr_ldiv_batched_c64) if cplx else
                    (L.dhqr_solve_batched_f32, L.dhqr_ldiv_batched_f32) if f32 else (L.dhqr_solve_batched_f64, L.dhqr_ldiv_batched_f64))
    if _is_tensor(A):
        lay = _batch_layout(A.shape, A.stride())
        if lay is None:
            raise ValueError("matrices of the batch must be column-major (stride(1) == 1)")
        if not _is_tensor(b) or b.dtype != A.dtype or not b.is_cuda or tuple(b.shape) != (batch, m):
            raise TypeError(f"{A.dtype} CUDA tensor of shape ({batch}, {m}) expected")
        if α.dtype != A.dtype or tuple(α.shape) != (batch, n) or not α.is_contiguous():
            raise TypeError(f"α must be a contiguous {A.dtype} tensor of shape ({batch}, {n})")
        w = b.clone(memory_format=torch.contiguous_format)  # src:318 copy of b
        ctx = get_context(A.device.index)
        ctx.use_torch_stream()
        check(solve(ctx.handle, ctypes.c_void_p(A.data_ptr()), m, n, lay[0], lay[1],
                                       ctypes.c_void_p(α.data_ptr()), max(n, 1), ctypes.c_void_p(w.data_ptr()), max(m, 1), batch))
        ctx.synchronize()
        return w[:, :n].clone()
    F, lda, strideA = _host_batch(A)
    al, sal = _host_rows(α, batch, n, "α", A.dtype)
    bb, sb = _host_rows(b, batch, m, "b", A.dtype)
    x = np.empty((batch, n), dtype=A.dtype)
    check(ldiv_(get_context().handle, F.ctypes.data_as(ctypes.c_void_p), m, n, lda, strideA,
                                  al.ctypes.data_as(ctypes.c_void_p), sal, bb.ctypes.data_as(ctypes.c_void_p), sb,
                                  x.ctypes.data_as(ctypes.c_void_p), max(n, 1), batch))
    return x


# ------------------------------------------------------------------------------- column pivoting, rank, truncated solve
def _is_f64(x) -> bool:
    return x.dtype == (torch.float64 if _is_tensor(x) else np.float64)


def _vp(x):
    return ctypes.c_void_p(x.data_ptr()) if _is_tensor(x) else x.ctypes.data_as(ctypes.c_void_p)


def _pivoted_input(A, what):
    """the (batch, m, n) float64 view of the argument of the pivoted functions (a 2-D A is a batch of one) and whether it
    lives on the device; float32 and complex input is a TypeError (dhqr.h: Float64 only)"""
    if not (_is_tensor(A) or isinstance(A, np.ndarray)):
        raise TypeError(f"{what}: float64 numpy array or CUDA tensor expected")
    if not _is_f64(A):
        raise TypeError(f"{what}: the pivoted routes are float64 only, got {A.dtype}")
    if A.ndim == 2:
        A = A[None]
    if A.ndim != 3:
        raise ValueError(f"{what}: (batch, m, n) or (m, n) array expected")
    if _is_tensor(A) and not A.is_cuda:
        raise TypeError(f"{what}: device path needs a float64 CUDA tensor")
    return A, _is_tensor(A)


def _rcond(rcond) -> float:
    return -1.0 if rcond is None else float(rcond)


def qr_pivoted_batched_(A) -> DistributedHouseholderQRStruct:
    """qr!(A[k]) with COLUMN PIVOTING for every matrix of a (batch, m, n) float64 batch (a 2-D A is a batch of one) in one
    call (dhqr_factor_batched_pivoted_f64 on a CUDA tensor with column-major matrices, dhqr_qr_batched_pivoted_f64 on a
    numpy array): A[k][:, jpvt[k]] = Q[k] R[k].  Mutates A; returns the struct with α (batch, n) and jpvt (batch, n) int32.
    get_q, get_r and apply_q_ take the struct unchanged."""
    L = _lib.lib()
    A, dev = _pivoted_input(A, "A")
    batch, m, n = A.shape
    if dev:
        lay = _batch_layout(A.shape, A.stride())
        if lay is None:
            raise ValueError("matrices of the batch must be column-major (stride(1) == 1); build it with empty_colmajor_batched")
        H = DistributedHouseholderQRStruct(A, jpvt=torch.zeros((batch, n), dtype=torch.int32, device=A.device))
        ctx = get_context(A.device.index)
        ctx.use_torch_stream()
        check(L.dhqr_factor_batched_pivoted_f64(ctx.handle, _vp(A), m, n, lay[0], lay[1], _vp(H.α), max(n, 1), _vp(H.jpvt), max(n, 1),
                                                batch))
        ctx.synchronize()
        return H
    F, lda, strideA = _host_batch(A)
    H = DistributedHouseholderQRStruct(A, jpvt=np.zeros((batch, n), dtype=np.int32))
    check(L.dhqr_qr_batched_pivoted_f64(get_context().handle, _vp(F), m, n, lda, strideA, _vp(H.α), max(n, 1), _vp(H.jpvt), max(n, 1),
                                        batch))
    if F is not A:
        A[...] = F
    return H


def _pivoted_struct(H):
    """(A (batch, m, n), α, jpvt, on the device?) of a struct qr_pivoted_batched_ returned"""
    if getattr(H, "jpvt", None) is None:
        raise TypeError("a pivoted factorisation (qr_pivoted_batched_) expected: the struct has no jpvt")
    A, dev = _pivoted_input(H.A, "H.A")
    batch, m, n = A.shape
    _same_dtype(A, H.α, "α")
    xp = torch if dev else np
    for v, dt, name in ((H.α, xp.float64, "α"), (H.jpvt, xp.int32, "jpvt")):
        if _is_tensor(v) != dev or v.dtype != dt or tuple(v.shape) != (batch, n) or (dev and not (v.is_cuda and v.is_contiguous())):
            raise TypeError(f"{name} must be a contiguous {dt} {'CUDA tensor' if dev else 'numpy array'} of shape ({batch}, {n})")
    if dev:
        return A, H.α, H.jpvt, True
    return A, np.ascontiguousarray(H.α), np.ascontiguousarray(H.jpvt), False


def rank_batched(H: DistributedHouseholderQRStruct, rcond=None):
    """the numerical rank of every matrix of a pivoted factorisation (dhqr_rank_batched_f64): the number of leading j with
    |α_j| > rc |α_0|, rc = rcond, or max(m, n) eps when rcond is None or negative; (batch,) int32, where the factor is."""
    L = _lib.lib()
    A, α, _, dev = _pivoted_struct(H)
    batch, m, n = A.shape
    if dev:
        rank = torch.zeros((batch,), dtype=torch.int32, device=A.device)
        _call_small_family(A, L.dhqr_rank_batched_f64, _vp(α), m, n, max(n, 1), _rcond(rcond), _vp(rank), batch)
        return rank
    if batch == 0 or n == 0:
        return np.zeros((batch,), dtype=np.int32)
    ctx = get_context()
    ctx.use_torch_stream()
    d = torch.from_numpy(α).to(f"cuda:{ctx.device}")
    rank = torch.zeros((batch,), dtype=torch.int32, device=d.device)
    check(L.dhqr_rank_batched_f64(ctx.handle, _vp(d), m, n, n, _rcond(rcond), _vp(rank), batch))
    ctx.synchronize()
    return rank.cpu().numpy()


def _rhs_block(b, batch, m, dev, what="b"):
    """(B (batch, m, nrhs), was it (batch, m)?) of the right-hand sides of the pivoted solves"""
    if _is_tensor(b) != dev or (dev and not b.is_cuda):
        raise TypeError(f"{what}: a {'float64 CUDA tensor' if dev else 'float64 numpy array'} like the matrices expected")
    if not _is_f64(b):
        raise TypeError(f"{what} is {b.dtype} but the pivoted routes are float64 only: convert it explicitly")
    vec = b.ndim == 2
    if vec:
        b = b[:, :, None]
    if b.ndim != 3 or tuple(b.shape[:2]) != (batch, m):
        raise ValueError(f"{what} must have shape ({batch}, {m}) or ({batch}, {m}, nrhs)")
    return b, vec


def ldiv_pivoted_batched(H: DistributedHouseholderQRStruct, B, rcond=None):
    """the rank-truncated least-squares solution of every matrix of a pivoted factorisation: rank_batched(H, rcond), then
    dhqr_solve_batched_pivoted_f64 on a copy of B.  B (batch, m) -> X (batch, n); B (batch, m, nrhs) -> X (batch, n, nrhs),
    column-major matrices.  X[k][jpvt[k][i]] = z_i for i < rank, exact zeros elsewhere; B is not modified."""
    L = _lib.lib()
    A, α, jpvt, dev = _pivoted_struct(H)
    batch, m, n = A.shape
    B, vec = _rhs_block(B, batch, m, dev, "B")
    nrhs = B.shape[2]
    ctx = get_context(A.device.index if dev else None)
    ctx.use_torch_stream()
    device = A.device if dev else f"cuda:{ctx.device}"
    if dev:
        dA, dal, djp = A, α, jpvt
    else:  # (the C ABI has no host form of the solve alone: stage with torch)
        dA = empty_colmajor_batched(batch, m, n, device)
        dA.copy_(torch.from_numpy(np.ascontiguousarray(A)))
        dal, djp = torch.from_numpy(α).to(device), torch.from_numpy(jpvt).to(device)
    lay = _batch_layout(dA.shape, dA.stride())
    if lay is None:
        raise ValueError("matrices of the batch must be column-major (stride(1) == 1)")
    rank = torch.zeros((batch,), dtype=torch.int32, device=device)
    W = empty_colmajor_batched(batch, m, nrhs, device)
    W.copy_(B if dev else torch.from_numpy(np.ascontiguousarray(B)))
    X = empty_colmajor_batched(batch, n, nrhs, device)
    check(L.dhqr_rank_batched_f64(ctx.handle, _vp(dal), m, n, max(n, 1), _rcond(rcond), _vp(rank), batch))
    check(L.dhqr_solve_batched_pivoted_f64(ctx.handle, _vp(dA), m, n, lay[0], lay[1], _vp(dal), max(n, 1), _vp(djp), max(n, 1), _vp(rank),
                                           _vp(W), nrhs, max(m, 1), max(m * nrhs, 1), _vp(X), max(n, 1), max(n * nrhs, 1), batch))
    ctx.synchronize()
    if not dev:
        X = X.cpu().numpy()
    return X[:, :, 0] if vec else X


def lstsq_batched(A, B, rcond=None):
    """min ||A[k] x - B[k]|| for every matrix of a (batch, m, n) float64 batch, rank-deficient matrices included: column-pivoted
    QR of a copy, the rank at rcond (rank_batched), the truncated solve.  Returns (X, rank); A and B are not modified.  numpy
    arrays: dhqr_lstsq_batched_f64; CUDA tensors: the three device entry points on copies."""
    L = _lib.lib()
    A, dev = _pivoted_input(A, "A")
    batch, m, n = A.shape
    B, vec = _rhs_block(B, batch, m, dev, "B")
    nrhs = B.shape[2]
    if dev:
        W = empty_colmajor_batched(batch, m, n, A.device)
        W.copy_(A)
        H = qr_pivoted_batched_(W)
        X = ldiv_pivoted_batched(H, B, rcond)
        return (X[:, :, 0] if vec else X), rank_batched(H, rcond)
    F, lda, strideA = _host_batch(A)
    Bf, ldb, strideB = _host_batch(B)
    X = np.zeros((batch, nrhs, n), dtype=np.float64).transpose(0, 2, 1)
    rank = np.zeros((batch,), dtype=np.int32)
    check(L.dhqr_lstsq_batched_f64(get_context().handle, _vp(F), m, n, lda, strideA, _vp(Bf), nrhs, ldb, strideB, _rcond(rcond), _vp(X),
                                   max(n, 1), max(n * nrhs, 1), _vp(rank), batch))
    return (X[:, :, 0] if vec else X), rank


# ---- the same four for every element type (float64: the functions above, their bytes; float32 and complex128: dhqr_*_f32 / _c64)
def _pivoted_sfx(A, what):
    """"f64", "f32" or "c64" for the element type of a numpy array or tensor; anything else is a TypeError"""
    if not (_is_tensor(A) or isinstance(A, np.ndarray)):
        raise TypeError(f"{what}: numpy array or CUDA tensor expected")
    xp = torch if _is_tensor(A) else np
    sfx = {xp.float64: "f64", xp.float32: "f32", xp.complex128: "c64"}.get(A.dtype if _is_tensor(A) else A.dtype.type)
    if sfx is None:
        raise TypeError(f"{what}: float64, float32 or complex128 expected, got {A.dtype}")
    return sfx


def _pivoted_any(A, what):
    """(A (batch, m, n), on the device?, suffix) of an argument of the typed pivoted functions (a 2-D A is a batch of one)"""
    sfx = _pivoted_sfx(A, what)
    if A.ndim == 2:
        A = A[None]
    if A.ndim != 3:
        raise ValueError(f"{what}: (batch, m, n) or (m, n) array expected")
    if _is_tensor(A) and not A.is_cuda:
        raise TypeError(f"{what}: device path needs a CUDA tensor")
    return A, _is_tensor(A), sfx


def _pivoted_rhs(b, A, batch, m, dev, what="B"):
    """(B (batch, m, nrhs), was it (batch, m)?); a dtype or residence other than the factor's is a TypeError"""
    if not (_is_tensor(b) or isinstance(b, np.ndarray)) or _is_tensor(b) != dev:
        raise TypeError(f"{what}: a {'CUDA tensor' if dev else 'numpy array'} like the matrices expected")
    if b.dtype != A.dtype:
        raise TypeError(f"{what} is {b.dtype} but the factor is {A.dtype}: convert it explicitly")
    if dev and not b.is_cuda:
        raise TypeError(f"{what}: a CUDA tensor like the matrices expected")
    vec = b.ndim == 2
    if vec:
        b = b[:, :, None]
    if b.ndim != 3 or tuple(b.shape[:2]) != (batch, m):
        raise ValueError(f"{what} must have shape ({batch}, {m}) or ({batch}, {m}, nrhs)")
    return b, vec


def _empty_colmajor_like(A, batch, m, n, device):
    return torch.empty((batch, n, m), dtype=A.dtype, device=device).transpose(1, 2)


def factor_pivoted_batched_(A) -> DistributedHouseholderQRStruct:
    """qr_pivoted_batched_ for every element type: qr!(A[k]) with COLUMN PIVOTING for every matrix of a (batch, m, n) float64,
    float32 or complex128 batch (a 2-D A is a batch of one): dhqr_factor_batched_pivoted_* on a CUDA tensor with column-major
    matrices, dhqr_qr_batched_pivoted_* on a numpy array.  Mutates A; returns the struct with α (batch, n) and jpvt (batch, n)
    int32.  form_q_batched, form_r_batched and apply_q_batched_ take the struct unchanged: A[k][:, jpvt[k]] = Q[k] R[k]."""
    A, dev, sfx = _pivoted_any(A, "A")
    if sfx == "f64":
        return qr_pivoted_batched_(A)
    L = _lib.lib()
    batch, m, n = A.shape
    if dev:
        lay = _batch_layout(A.shape, A.stride())
        if lay is None:
            raise ValueError("matrices of the batch must be column-major (stride(1) == 1); build it with empty_colmajor_batched")
        H = DistributedHouseholderQRStruct(A, jpvt=torch.zeros((batch, n), dtype=torch.int32, device=A.device))
        ctx = get_context(A.device.index)
        ctx.use_torch_stream()
        check(getattr(L, f"dhqr_factor_batched_pivoted_{sfx}")(ctx.handle, _vp(A), m, n, lay[0], lay[1], _vp(H.α), max(n, 1),
                                                               _vp(H.jpvt), max(n, 1), batch))
        ctx.synchronize()
        return H
    F, lda, strideA = _host_batch(A)
    H = DistributedHouseholderQRStruct(A, jpvt=np.zeros((batch, n), dtype=np.int32))
    check(getattr(L, f"dhqr_qr_batched_pivoted_{sfx}")(get_context().handle, _vp(F), m, n, lda, strideA, _vp(H.α), max(n, 1),
                                                       _vp(H.jpvt), max(n, 1), batch))
    if F is not A:
        A[...] = F
    return H


def _pivoted_struct_any(H):
    """(A (batch, m, n), α, jpvt, on the device?, suffix) of a struct factor_pivoted_batched_ returned"""
    if getattr(H, "jpvt", None) is None:
        raise TypeError("a pivoted factorisation (factor_pivoted_batched_) expected: the struct has no jpvt")
    A, dev, sfx = _pivoted_any(H.A, "H.A")
    batch, m, n = A.shape
    if not (_is_tensor(H.α) or isinstance(H.α, np.ndarray)) or H.α.dtype != A.dtype:
        raise TypeError(f"α is {getattr(H.α, 'dtype', type(H.α))} but the factor is {A.dtype}")
    xp = torch if dev else np
    for v, dt, name in ((H.α, A.dtype, "α"), (H.jpvt, xp.int32, "jpvt")):
        if _is_tensor(v) != dev or v.dtype != dt or tuple(v.shape) != (batch, n) or (dev and not (v.is_cuda and v.is_contiguous())):
            raise TypeError(f"{name} must be a contiguous {dt} {'CUDA tensor' if dev else 'numpy array'} of shape ({batch}, {n})")
    if dev:
        return A, H.α, H.jpvt, True, sfx
    return A, np.ascontiguousarray(H.α), np.ascontiguousarray(H.jpvt), False, sfx


def rank_pivoted_batched(H: DistributedHouseholderQRStruct, rcond=None):
    """rank_batched for every element type (dhqr_rank_batched_*): the number of leading j with |α_j| > rc |α_0|, rc = rcond, or
    max(m, n) eps of the element type when rcond is None or negative; (batch,) int32, where the factor is."""
    A, α, _, dev, sfx = _pivoted_struct_any(H)
    if sfx == "f64":
        return rank_batched(H, rcond)
    L = _lib.lib()
    batch, m, n = A.shape
    if batch == 0 or n == 0:
        return torch.zeros((batch,), dtype=torch.int32, device=A.device) if dev else np.zeros((batch,), dtype=np.int32)
    ctx = get_context(A.device.index if dev else None)
    ctx.use_torch_stream()
    d = α if dev else torch.from_numpy(α).to(f"cuda:{ctx.device}")
    rank = torch.zeros((batch,), dtype=torch.int32, device=d.device)
    check(getattr(L, f"dhqr_rank_batched_{sfx}")(ctx.handle, _vp(d), m, n, max(n, 1), _rcond(rcond), _vp(rank), batch))
    ctx.synchronize()
    return rank if dev else rank.cpu().numpy()


def solve_pivoted_batched(H: DistributedHouseholderQRStruct, B, rcond=None):
    """ldiv_pivoted_batched for every element type: rank_pivoted_batched(H, rcond), then dhqr_solve_batched_pivoted_* on a copy
    of B.  B (batch, m) -> X (batch, n); B (batch, m, nrhs) -> X (batch, n, nrhs), column-major matrices.  X[k][jpvt[k][i]] = z_i
    for i < rank, exact zeros elsewhere; B is not modified.  A B of another dtype than the factor's is a TypeError."""
    A, α, jpvt, dev, sfx = _pivoted_struct_any(H)
    batch, m, n = A.shape
    B, vec = _pivoted_rhs(B, A, batch, m, dev)
    if sfx == "f64":
        return ldiv_pivoted_batched(H, B[:, :, 0] if vec else B, rcond)
    L = _lib.lib()
    nrhs = B.shape[2]
    ctx = get_context(A.device.index if dev else None)
    ctx.use_torch_stream()
    device = A.device if dev else f"cuda:{ctx.device}"
    if dev:
        dA, dal, djp = A, α, jpvt
    else:  # (the C ABI has no host form of the solve alone: stage with torch)
        tA = torch.from_numpy(np.ascontiguousarray(A))
        dA = _empty_colmajor_like(tA, batch, m, n, device)
        dA.copy_(tA)
        dal, djp = torch.from_numpy(α).to(device), torch.from_numpy(jpvt).to(device)
    lay = _batch_layout(dA.shape, dA.stride())
    if lay is None:
        raise ValueError("matrices of the batch must be column-major (stride(1) == 1)")
    rank = torch.zeros((batch,), dtype=torch.int32, device=device)
    W = _empty_colmajor_like(dA, batch, m, nrhs, device)
    W.copy_(B if dev else torch.from_numpy(np.ascontiguousarray(B)))
    X = _empty_colmajor_like(dA, batch, n, nrhs, device)
    if batch and n and nrhs:
        check(getattr(L, f"dhqr_rank_batched_{sfx}")(ctx.handle, _vp(dal), m, n, max(n, 1), _rcond(rcond), _vp(rank), batch))
        check(getattr(L, f"dhqr_solve_batched_pivoted_{sfx}")(ctx.handle, _vp(dA), m, n, lay[0], lay[1], _vp(dal), max(n, 1), _vp(djp),
                                                              max(n, 1), _vp(rank), _vp(W), nrhs, max(m, 1), max(m * nrhs, 1), _vp(X),
                                                              max(n, 1), max(n * nrhs, 1), batch))
    ctx.synchronize()
    if not dev:
        X = X.cpu().numpy()
    return X[:, :, 0] if vec else X


def lstsq_pivoted_batched(A, B, rcond=None):
    """lstsq_batched for every element type: min ||A[k] x - B[k]|| for every matrix of a (batch, m, n) batch, rank-deficient
    matrices included.  Returns (X, rank); A and B are not modified.  numpy arrays: dhqr_lstsq_batched_*; CUDA tensors: the
    three device entry points on copies.  A B of another dtype than A's is a TypeError."""
    A, dev, sfx = _pivoted_any(A, "A")
    batch, m, n = A.shape
    B, vec = _pivoted_rhs(B, A, batch, m, dev)
    if sfx == "f64":
        return lstsq_batched(A, B[:, :, 0] if vec else B, rcond)
    L = _lib.lib()
    nrhs = B.shape[2]
    if dev:
        W = _empty_colmajor_like(A, batch, m, n, A.device)
        W.copy_(A)
        H = factor_pivoted_batched_(W)
        X = solve_pivoted_batched(H, B, rcond)
        return (X[:, :, 0] if vec else X), rank_pivoted_batched(H, rcond)
    F, lda, strideA = _host_batch(A)
    Bf, ldb, strideB = _host_batch(B)
    X = np.zeros((batch, nrhs, n), dtype=A.dtype).transpose(0, 2, 1)
    rank = np.zeros((batch,), dtype=np.int32)
    check(getattr(L, f"dhqr_lstsq_batched_{sfx}")(get_context().handle, _vp(F), m, n, lda, strideA, _vp(Bf), nrhs, ldb, strideB,
                                                  _rcond(rcond), _vp(X), max(n, 1), max(n * nrhs, 1), _vp(rank), batch))
    return (X[:, :, 0] if vec else X), rank


def _partialdot_c64(a, b, lo: int, hi: int) -> complex:
    """partialdot(a, b, lo:hi-1, ComplexF64) (src:51-59): sum conj(a[i]) b[i]"""
    L = _lib.lib()
    out = (ctypes.c_double * 2)()
    if not _is_tensor(a):
        a = np.ascontiguousarray(a, dtype=np.complex128)
        b = np.ascontiguousarray(b, dtype=np.complex128)
        check(L.dhqr_partialdot_host_c64(get_context().handle, a.ctypes.data_as(ctypes.c_void_p),
                                         b.ctypes.data_as(ctypes.c_void_p), lo, hi, out))
        return complex(out[0], out[1])
    ctx = get_context(a.device.index)
    ctx.use_torch_stream()
    check(L.dhqr_partialdot_c64(ctx.handle, _dev_vector(a, hi, torch.complex128),
                                _dev_vector(b, hi, torch.complex128), lo, hi, out))
    return complex(out[0], out[1])


def partialdot(a, b, lo: int, hi: int):
    """partialdot(a, b, lo:hi-1, T) (src:42-49 Float64, src:51-59 ComplexF64 = conj(a).b), 0-based
    with hi exclusive, reduced on the GPU."""
    L = _lib.lib()
    if _is_complex(a) or _is_complex(b):
        return _partialdot_c64(a, b, lo, hi)
    if not _is_tensor(a):  # host vectors: the entry point the Julia module binds
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        out = ctypes.c_double()
        check(L.dhqr_partialdot_host_f64(get_context().handle, a.ctypes.data_as(ctypes.c_void_p),
                                         b.ctypes.data_as(ctypes.c_void_p), lo, hi, ctypes.byref(out)))
        return out.value
    ctx = get_context(a.device.index)
    ctx.use_torch_stream()
    out = ctypes.c_double()
    check(L.dhqr_partialdot_f64(ctx.handle, _dev_vector(a, hi), _dev_vector(b, hi), lo, hi, ctypes.byref(out)))
    return out.value


# ------------------------------------------------------------------------------- metric helpers
def _small_family(A) -> bool:
    """does the factor belong to the entry points of the small-matrix family (dhqr_apply_q_batched_* ...): a (batch, m, n)
    batch of either real type, or one float32 matrix (a batch of one)?  A 2-D float64 tensor keeps the blocked route."""
    if not _is_tensor(A):
        raise TypeError("device tensors only: the factor is a host array (apply_q_, get_q and get_r have no host form)")
    if A.dtype not in (torch.float64, torch.float32):
        raise TypeError("device path needs a float64 or float32 CUDA tensor")
    return A.dim() == 3 or A.dtype == torch.float32


def _colmajor_batch(A, what):
    """(pointer, batch, rows, cols, ld, stride) of a device tensor of the small-matrix family: (batch, rows, cols) with
    column-major matrices, or one column-major (rows, cols) matrix -- a batch of one.  Layouts are judged before residency
    (_need_cuda), which needs no device."""
    shape, strides = (tuple(A.shape), tuple(A.stride())) if A.dim() == 3 else ((1,) + tuple(A.shape), (0,) + tuple(A.stride()))
    lay = _batch_layout(shape, strides) if len(shape) == 3 else None
    if lay is None:
        raise ValueError(f"{what}: column-major matrices required (unit stride down a column); build them with "
                         "empty_colmajor or empty_colmajor_batched")
    return (ctypes.c_void_p(A.data_ptr()),) + shape + lay


def _need_cuda(*tensors):
    if not all(x.is_cuda for x in tensors):
        raise TypeError("device tensors only: the device path needs CUDA tensors")


def _call_small_family(A, fn, *args):
    ctx = get_context(A.device.index)
    ctx.use_torch_stream()
    check(fn(ctx.handle, *args))
    ctx.synchronize()


def apply_q_(H: DistributedHouseholderQRStruct, B, trans: bool):
    """B <- Q' B (trans) or Q B, in place, device tensors only.  One float64 matrix: the blocked route (dhqr_apply_q_f64).
    A (batch, m, n) float64 or float32 batch with B (batch, m, nrhs), its matrices column-major like the factor's, and one
    float32 matrix with B (m, nrhs): dhqr_apply_q_batched_f64 / _f32 -- one launch up to 64 x 32."""
    _same_dtype(H.A, B, "B")
    if not _small_family(H.A):
        ptr, m, n, lda, dev = _dev_matrix(H.A)
        bptr, mb, nrhs, ldb, _ = _dev_matrix(B)
        if mb != m:
            raise ValueError("row mismatch")
        ctx = get_context(dev)
        ctx.use_torch_stream()
        check(_lib.lib().dhqr_apply_q_f64(ctx.handle, ptr, m, n, lda, bptr, nrhs, ldb, 1 if trans else 0))
        return B
    A = H.A
    ptr, batch, m, n, lda, strideA = _colmajor_batch(A, "H.A")
    if not _is_tensor(B) or B.dtype != A.dtype or B.dim() != A.dim() or tuple(B.shape[:-1]) != tuple(A.shape[:-2]) + (m,):
        raise TypeError(f"B: {A.dtype} CUDA tensor of shape {tuple(A.shape[:-2]) + (m, 'nrhs')} expected")
    bptr, _, _, nrhs, ldb, strideB = _colmajor_batch(B, "B")
    _need_cuda(A, B)
    L = _lib.lib()
    fn = L.dhqr_apply_q_batched_f32 if _is_f32(A) else L.dhqr_apply_q_batched_f64
    _call_small_family(A, fn, ptr, m, n, lda, strideA, bptr, nrhs, ldb, strideB, batch, 1 if trans else 0)
    return B


def get_r(H: DistributedHouseholderQRStruct):
    r"""n x n upper-triangular R of a device factorisation (strict upper part of H.A + α on the
    diagonal, src:296-309), as a new column-major device tensor; (batch, n, n) for a batch.  The reference exposes R only
    implicitly through `\`; SURVEY.md section 8f rank 2 asks for the explicit extraction."""
    _same_dtype(H.A, H.α, "α")
    if not _small_family(H.A):
        ptr, m, n, lda, dev = _dev_matrix(H.A)
        W = empty_colmajor(m, n, H.A.device)
        wptr, _, _, ldw, _ = _dev_matrix(W)
        ctx = get_context(dev)
        ctx.use_torch_stream()
        check(_lib.lib().dhqr_form_r0_f64(ctx.handle, ptr, m, n, lda, _dev_vector(H.α, n), wptr, ldw, NB, 1, 0))
        return W[:n, :]
    A, α = H.A, H.α
    ptr, batch, m, n, lda, strideA = _colmajor_batch(A, "H.A")
    _need_cuda(A)
    if not _is_tensor(α) or α.dtype != A.dtype or not α.is_cuda or tuple(α.shape) != tuple(A.shape[:-2]) + (n,) or not α.is_contiguous():
        raise TypeError(f"α must be a contiguous {A.dtype} CUDA tensor of shape {tuple(A.shape[:-2]) + (n,)}")
    R = empty_colmajor_batched(batch, n, n, A.device, A.dtype)
    L = _lib.lib()
    fn = L.dhqr_form_r_batched_f32 if _is_f32(A) else L.dhqr_form_r_batched_f64
    _call_small_family(A, fn, ptr, m, n, lda, strideA, ctypes.c_void_p(α.data_ptr()), max(n, 1), ctypes.c_void_p(R.data_ptr()),
                       max(n, 1), max(n * n, 1), batch)
    return R if A.dim() == 3 else R[0]


def get_q(H: DistributedHouseholderQRStruct):
    """explicit thin Q (m x n, column-major device tensor; (batch, m, n) for a batch): Q = H_1 ... H_n applied to [I; 0]."""
    if not _small_family(H.A):
        m, n = H.A.shape
        Q = empty_colmajor(m, n, H.A.device)
        Q.zero_()
        Q.diagonal().fill_(1.0)
        return apply_q_(H, Q, trans=False)
    A = H.A
    ptr, batch, m, n, lda, strideA = _colmajor_batch(A, "H.A")
    _need_cuda(A)
    Q = empty_colmajor_batched(batch, m, n, A.device, A.dtype)
    L = _lib.lib()
    fn = L.dhqr_form_q_batched_f32 if _is_f32(A) else L.dhqr_form_q_batched_f64
    _call_small_family(A, fn, ptr, m, n, lda, strideA, ctypes.c_void_p(Q.data_ptr()), max(m, 1), max(m * n, 1), batch)
    return Q if A.dim() == 3 else Q[0]


# ------------------------------------------------------------------------------- the batched names, complex128 included
# ldiv / ldiv_batched with a block of right-hand sides, apply_q_, get_q and get_r keep refusing a complex128 factor.  The four
# functions below are named after the C entry points (dhqr_solve_batched_nrhs_* ... dhqr_form_r_batched_*) and take every
# element type: complex128 goes to the _c64 entry points, float64 / float32 return exactly what the generic names return.
def _c64_factor(H, what):
    """(pointer, batch, m, n, lda, strideA) of a complex128 DEVICE factor: (batch, m, n) with column-major matrices, or one
    column-major (m, n) matrix -- a batch of one"""
    A = H.A
    if not _is_tensor(A):
        raise TypeError(f"device tensors only: the factor is a host array ({what} has no host form)")
    if A.dim() not in (2, 3):
        raise ValueError("(m, n) or (batch, m, n) factor expected")
    return _colmajor_batch(A, "H.A")


def _c64_alpha(H, batch, n):
    A, α = H.A, H.α
    if not _is_tensor(α) or α.dtype != A.dtype or not α.is_cuda or tuple(α.shape) != tuple(A.shape[:-2]) + (n,) or not α.is_contiguous():
        raise TypeError(f"α must be a contiguous {A.dtype} CUDA tensor of shape {tuple(A.shape[:-2]) + (n,)}")
    return ctypes.c_void_p(α.data_ptr())


def solve_batched_nrhs(H: DistributedHouseholderQRStruct, B):
    """`H \\ B` for a block of right-hand sides and every element type: B (batch, m, nrhs) with a batched factor, (m, nrhs)
    with a single one -> X (batch, n, nrhs) / (n, nrhs), column-major.  B is NOT modified.  complex128:
    dhqr_solve_batched_nrhs_c64 on a copy of a device B (its matrices column-major like the factor's),
    dhqr_ldiv_batched_nrhs_c64 on numpy arrays (any layout; copied where the layout asks for it); column r of X has the bits
    of ldiv_batched on the vectors B[..., r].  Up to 64 x 32 one wave per matrix; beyond that, up to 128 rows, one launch of the
    one-workgroup multi-column kernel (a workgroup per matrix and group of 6 columns) where that was measured to beat the column
    loop (2 .. 6 and 13 .. 18 columns; the same bits either way).  float64 / float32:
    ldiv(H, B)."""
    A, α = H.A, H.α
    _same_field(A, B, "B")
    _same_field(A, α, "α")
    if not _is_complex(A):
        return ldiv(H, B)
    if A.ndim not in (2, 3) or getattr(B, "ndim", 0) != A.ndim:
        raise ValueError("B must have as many dimensions as the factor: (batch, m, nrhs) or (m, nrhs)")
    L = _lib.lib()
    single = A.ndim == 2
    if _is_tensor(A):
        ptr, batch, m, n, lda, strideA = _c64_factor(H, "a device solve")
        if not _is_tensor(B) or B.dtype != A.dtype or tuple(B.shape[:-1]) != tuple(A.shape[:-2]) + (m,):
            raise TypeError(f"B: {A.dtype} CUDA tensor of shape {tuple(A.shape[:-2]) + (m, 'nrhs')} expected")
        _colmajor_batch(B, "B")  # (the layout rule, before the copy hides it)
        _need_cuda(A, B)
        nrhs = B.shape[-1]
        W = empty_colmajor_batched_c(batch, m, nrhs, B.device)
        W.copy_(B if not single else B.unsqueeze(0))  # src:318 copy of B
        _call_small_family(A, L.dhqr_solve_batched_nrhs_c64, ptr, m, n, lda, strideA, _c64_alpha(H, batch, n), max(n, 1),
                           ctypes.c_void_p(W.data_ptr()), nrhs, max(m, 1), max(m * nrhs, 1), batch)
        X = empty_colmajor_batched_c(batch, n, nrhs, B.device)
        X.copy_(W[:, :n, :])
        return X[0] if single else X
    if not isinstance(A, np.ndarray):
        raise TypeError("complex128 numpy array or CUDA tensor expected")
    A3 = A[None] if single else A
    batch, m, n = A3.shape
    B3 = np.asarray(B, dtype=np.complex128)
    B3 = B3[None] if single else B3
    if B3.shape[:2] != (batch, m):
        raise ValueError(f"B must have shape {tuple(A.shape[:-2]) + (m, 'nrhs')}")
    nrhs = B3.shape[2]
    F, lda, strideA = _host_batch(A3)
    Bf, ldb, strideB = _host_batch(B3)
    al, sal = _host_rows(np.asarray(α).reshape(batch, n), batch, n, "α", np.complex128)
    X = np.empty((batch, nrhs, n), dtype=np.complex128).transpose(0, 2, 1)
    check(L.dhqr_ldiv_batched_nrhs_c64(get_context().handle, F.ctypes.data_as(ctypes.c_void_p), m, n, lda, strideA,
                                       al.ctypes.data_as(ctypes.c_void_p), sal, Bf.ctypes.data_as(ctypes.c_void_p), nrhs, ldb, strideB,
                                       X.ctypes.data_as(ctypes.c_void_p), max(n, 1), max(n * nrhs, 1), batch))
    return X[0] if single else X


def apply_q_batched_(H: DistributedHouseholderQRStruct, B, trans: bool):
    """B <- Q^H B (trans) or Q B, in place, device tensors only, every element type: complex128 through
    dhqr_apply_q_batched_c64 (a (batch, m, n) factor with B (batch, m, nrhs), or one matrix with B (m, nrhs), matrices
    column-major) -- up to 128 rows one launch that carries every column in double-double, so rows n .. m-1 of Q^H B have the
    bits of what solve_batched_nrhs leaves there and a column's bits do not depend on its neighbours; float64 / float32:
    apply_q_(H, B, trans)."""
    A = H.A
    _same_field(A, B, "B")
    if not _is_complex(A):
        return apply_q_(H, B, trans)
    ptr, batch, m, n, lda, strideA = _c64_factor(H, "apply_q_batched_")
    if not _is_tensor(B) or B.dtype != A.dtype or B.dim() != A.dim() or tuple(B.shape[:-1]) != tuple(A.shape[:-2]) + (m,):
        raise TypeError(f"B: {A.dtype} CUDA tensor of shape {tuple(A.shape[:-2]) + (m, 'nrhs')} expected")
    bptr, _, _, nrhs, ldb, strideB = _colmajor_batch(B, "B")
    _need_cuda(A, B)
    _call_small_family(A, _lib.lib().dhqr_apply_q_batched_c64, ptr, m, n, lda, strideA, bptr, nrhs, ldb, strideB, batch, 1 if trans else 0)
    return B


def form_q_batched(H: DistributedHouseholderQRStruct):
    """explicit thin Q of a device factorisation of every element type: (batch, m, n) for a batch, (m, n) for one matrix,
    column-major.  complex128: dhqr_form_q_batched_c64 (up to 128 rows one launch, equal to apply_q_batched_(H, [I; 0], False) for
    a finite factor); float64 / float32: get_q(H)."""
    A = H.A
    if not _is_complex(A):
        return get_q(H)
    ptr, batch, m, n, lda, strideA = _c64_factor(H, "form_q_batched")
    _need_cuda(A)
    Q = empty_colmajor_batched_c(batch, m, n, A.device)
    _call_small_family(A, _lib.lib().dhqr_form_q_batched_c64, ptr, m, n, lda, strideA, ctypes.c_void_p(Q.data_ptr()), max(m, 1),
                       max(m * n, 1), batch)
    return Q if A.dim() == 3 else Q[0]


def form_r_batched(H: DistributedHouseholderQRStruct):
    """n x n upper-triangular R of a device factorisation of every element type (strict upper part of H.A, α on the diagonal,
    zeros below): (batch, n, n) or (n, n), column-major.  complex128: dhqr_form_r_batched_c64; float64 / float32: get_r(H)."""
    A = H.A
    _same_field(A, H.α, "α")
    if not _is_complex(A):
        return get_r(H)
    ptr, batch, m, n, lda, strideA = _c64_factor(H, "form_r_batched")
    _need_cuda(A)
    R = empty_colmajor_batched_c(batch, n, n, A.device)
    _call_small_family(A, _lib.lib().dhqr_form_r_batched_c64, ptr, m, n, lda, strideA, _c64_alpha(H, batch, n), max(n, 1),
                       ctypes.c_void_p(R.data_ptr()), max(n, 1), max(n * n, 1), batch)
    return R if A.dim() == 3 else R[0]


def residual(H: DistributedHouseholderQRStruct, Aorig, work=None) -> float:
    """||Aorig - Q R||_F / ||Aorig||_F on the device (north-star metric)."""
    ptr, m, n, lda, dev = _dev_matrix(H.A)
    optr, mo, no, ldo, _ = _dev_matrix(Aorig)
    if (mo, no) != (m, n):
        raise ValueError("shape mismatch")
    if work is None:
        work = empty_colmajor(m, n, H.A.device)
    wptr, _, _, ldw, _ = _dev_matrix(work)
    if ldw != m:
        raise ValueError("work must have leading dimension m")
    ctx = get_context(dev)
    ctx.use_torch_stream()
    out = ctypes.c_double()
    check(_lib.lib().dhqr_residual_f64(ctx.handle, ptr, m, n, lda, _dev_vector(H.α, n), optr, ldo, wptr,
                                       ctypes.byref(out)))
    return out.value


_bench_ctx = {}


def bench_context(device: Optional[int] = None):
    """(libdhqr_bench.so, context handle created by it) for the micro-benchmarks of include/dhqr_bench.h -- they are not
    in the product library, and contexts are per library."""
    import torch as _t
    dev = _t.cuda.current_device() if device is None else int(device)
    if dev not in _bench_ctx:
        B = _lib.lib_bench()
        h = ctypes.c_void_p()
        rc = B.dhqr_create(ctypes.byref(h), dev)
        if rc != 0:
            raise DHQRError(rc, B.dhqr_last_error().decode(errors="replace"))
        _bench_ctx[dev] = (B, h)
    return _bench_ctx[dev]


def bench_check(B, rc):
    if rc != 0:
        raise DHQRError(rc, B.dhqr_last_error().decode(errors="replace"))


def bench_mfma_tflops(device: Optional[int] = None) -> float:
    B, h = bench_context(device)
    out = ctypes.c_double()
    bench_check(B, B.dhqr_bench_mfma_f64(h, ctypes.byref(out)))
    return out.value


def bench_stream_gbps(nbytes: int = 1 << 30, device: Optional[int] = None) -> float:
    B, h = bench_context(device)
    out = ctypes.c_double()
    bench_check(B, B.dhqr_bench_stream_f64(h, nbytes, ctypes.byref(out)))
    return out.value
