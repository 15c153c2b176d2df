"""Test-only helpers of the tests of the batched ComplexF64 `H \\ B`, Q application, explicit Q and R
(test_emulated_zapplyq.py, test_gpu_zapplyq.py): the shapes and counts both files share, the seeded right-hand sides, a
strided sentinel-guarded complex batch with a block B_k per matrix (ZNBatch, in the style of zbatched_helpers.ZBatch) and
result matrices (ZOut, in the style of applyq_helpers.OutBatch) driven through the C ABI, the reflectors applied in
np.clongdouble (the reference of the accuracy criteria), the bounds.  The product never imports this file.

BOUNDS (the project's): |result - reference| <= 1e-12 max|result| for Q^H B, Q B and Q (applyq_helpers.tol("f64")); x within
1e-9 max|x| of orc.solve_c on the oracle's own factor; max|A - QR| and max|Q^H Q - I| at most zh.T(n) max|A|.  Measured on
the emulated library over every test of test_emulated_zapplyq.py (worst case): 3.4e-15 max|result| against the clongdouble
reflectors and in the round trip Q (Q^H B) = B, 6.0e-15 max|x|, 0.16 T(n) max|A| for A - QR and 0.23 T(n) max|A| for Q^H Q - I."""
import ctypes

import numpy as np

import zbatched_helpers as zh
from zbatched_helpers import SENT, cptr

P = ctypes.c_void_p
EINVAL = -1
TOL_Q = 1e-12  # applyq_helpers.tol("f64")
TOL_X = 1e-9
WAVE_SHAPES = [(1, 1), (5, 3), (16, 8), (33, 9), (40, 17), (64, 32), (32, 32)]
GPU_SHAPES = [(5, 3), (16, 8), (40, 17), (64, 32), (32, 32)]
BEYOND = [(66, 33, 1), (130, 20, 1), (16, 8, 0)]  # (m, n, small route): the general tier
SEED = 100


def nc(n):
    """columns held per wave by the instantiation that serves n columns"""
    return 8 if n <= 8 else 16 if n <= 16 else 32


def rg_solve(n):
    """right-hand sides per group of k_batched_zldiv_wave_nrhs (BQZN_RG)"""
    return {8: 1, 16: 2, 32: 4}[nc(n)]


def rg_apply(n):
    """columns per group of k_batched_zapplyq_wave (BQZA_RG)"""
    return {8: 1, 16: 3, 32: 4}[nc(n)]


def nrhs_list(n, rg):
    """1, a full group, a group and a tail of one, several groups (7), two full groups and a tail of one"""
    g = rg(n)
    return sorted({1, g, g + 1, 7, 2 * g + 1})


# The library sends a solve to the multi-column kernel only where that was measured to pay (dhqr.h: nrhs >= 4 in full
# groups) and to the column loop elsewhere -- the same bits.  A context created under TUNE_KERNEL takes the kernel for every
# call, tail groups included; the default context is tested at RULE_NRHS: 4 (the kernel at every shape) and 7 (the kernel for
# n <= 8, the loop beyond).
TUNE_KERNEL = "znrhs_wave=1"
RULE_NRHS = [4, 7]


def rule_takes_kernel(n, nrhs):
    return nrhs >= 4 and nrhs % rg_solve(n) == 0


def inputs(orc, m, n, nrhs, batch, seed=SEED):
    """(mats[k] (m, n), Bs[k] (m, nrhs)): A_k = rand_matrix_c(m, n, seed + k), column r of B_k = rand_vector_c(m, seed + 5000 +
    1000 r + k)"""
    mats = [orc.rand_matrix_c(m, n, seed + k) for k in range(batch)]
    Bs = [np.asfortranarray(np.stack([orc.rand_vector_c(m, seed + 5000 + 1000 * r + k) for r in range(nrhs)], axis=1))
          for k in range(batch)]
    return mats, Bs


def _flat(count, off):
    """SENT-filled complex buffer of `count` elements behind `off` leading ones (numpy buffers are 16-byte aligned)"""
    return np.full(off + count + 7, SENT)


class ZNBatch:
    """a strided batch in flat SENT-filled host buffers (for the EMULATED library, whose "device" memory is host memory):
    matrix k at A[off + k*sA:] (leading dimension lda), alpha_k at al[off + k*sal:], B_k (m x nrhs) at B[off + k*sB:] (ldb), X_k
    (n x nrhs, the host form's result) at X[off + k*sX:] (ldx); everything counts complex elements"""

    def __init__(self, mats, Bs, als=None, pad_ld=1, pad=5, pad_ldb=1, pad_ldx=2, off=1):
        self.batch, (self.m, self.n), self.nrhs = len(mats), mats[0].shape, Bs[0].shape[1]
        m, n, nrhs, batch = self.m, self.n, self.nrhs, self.batch
        self.off = off
        self.lda, self.ldb, self.ldx = m + pad_ld, m + pad_ldb, n + pad_ldx
        self.sA, self.sal = self.lda * n + pad, n + (3 if pad else 0)
        self.sB, self.sX = self.ldb * nrhs + pad, self.ldx * nrhs + pad
        self.A, self.al = _flat(batch * self.sA, off), _flat(batch * self.sal, off)
        self.B, self.X = _flat(batch * self.sB, off), _flat(batch * self.sX, off)
        self.maskA, self.maskal, self.maskB, self.maskX = (np.zeros(v.size, bool) for v in (self.A, self.al, self.B, self.X))
        for k in range(batch):
            self.mat(k)[...] = mats[k]
            self.bmat(k)[...] = Bs[k]
            if als is not None:
                self.alpha(k)[...] = als[k]
            self.maskal[off + k * self.sal: off + k * self.sal + n] = True
            for j in range(n):
                self.maskA[off + k * self.sA + j * self.lda: off + k * self.sA + j * self.lda + m] = True
            for r in range(nrhs):
                self.maskB[off + k * self.sB + r * self.ldb: off + k * self.sB + r * self.ldb + m] = True
                self.maskX[off + k * self.sX + r * self.ldx: off + k * self.sX + r * self.ldx + n] = True

    def _win(self, buf, k, stride, ld, rows, cols):
        o = self.off + k * stride
        return buf[o: o + ld * cols].reshape((ld, cols), order="F")[:rows]

    def mat(self, k):
        return self._win(self.A, k, self.sA, self.lda, self.m, self.n)

    def alpha(self, k):
        return self.al[self.off + k * self.sal: self.off + k * self.sal + self.n]

    def bmat(self, k):
        return self._win(self.B, k, self.sB, self.ldb, self.m, self.nrhs)

    def xmat(self, k):
        return self._win(self.X, k, self.sX, self.ldx, self.n, self.nrhs)

    def padding_intact(self):
        return all(bool(np.all(buf[~mask] == SENT)) for buf, mask in
                   ((self.A, self.maskA), (self.al, self.maskal), (self.B, self.maskB), (self.X, self.maskX)))

    def x_untouched(self):
        return bool(np.all(self.X == SENT))

    def pA(self):
        return cptr(self.A[self.off:])

    def pal(self):
        return cptr(self.al[self.off:])

    def pB(self):
        return cptr(self.B[self.off:])

    def pX(self):
        return cptr(self.X[self.off:])

    def _args(self, kw, **extra):
        a = dict(A=self.pA(), m=self.m, n=self.n, lda=self.lda, sA=self.sA, al=self.pal(), sal=self.sal, B=self.pB(),
                 nrhs=self.nrhs, ldb=self.ldb, sB=self.sB, batch=self.batch, **extra)
        a.update(kw)
        return a

    def factor(self, L, h, nb=0):
        return L.dhqr_factor_batched_c64(h, self.pA(), self.m, self.n, self.lda, self.sA, self.pal(), self.sal, self.batch, nb)

    def solve_nrhs(self, L, h, **kw):
        """dhqr_solve_batched_nrhs_c64, in place on B; keyword arguments replace single arguments"""
        a = self._args(kw)
        return L.dhqr_solve_batched_nrhs_c64(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["al"], a["sal"], a["B"], a["nrhs"],
                                             a["ldb"], a["sB"], a["batch"])

    def ldiv_nrhs(self, L, h, **kw):
        """dhqr_ldiv_batched_nrhs_c64: B is read, X written"""
        a = self._args(kw, X=self.pX(), ldx=self.ldx, sX=self.sX)
        return L.dhqr_ldiv_batched_nrhs_c64(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["al"], a["sal"], a["B"], a["nrhs"],
                                            a["ldb"], a["sB"], a["X"], a["ldx"], a["sX"], a["batch"])

    def apply_q(self, L, h, trans, **kw):
        a = self._args(kw, trans=trans)
        return L.dhqr_apply_q_batched_c64(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["B"], a["nrhs"], a["ldb"], a["sB"],
                                          a["batch"], a["trans"])

    def form_q(self, L, h, out, **kw):
        a = self._args(kw, Q=out.p(), ldq=out.ld, sQ=out.stride)
        return L.dhqr_form_q_batched_c64(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["Q"], a["ldq"], a["sQ"], a["batch"])

    def form_r(self, L, h, out, **kw):
        a = self._args(kw, R=out.p(), ldr=out.ld, sR=out.stride)
        return L.dhqr_form_r_batched_c64(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["al"], a["sal"], a["R"], a["ldr"],
                                         a["sR"], a["batch"])

    def single_column(self, L, h, r, B0):
        """the parent's call on column r alone: dhqr_solve_batched_c64 on a packed copy of the columns r of B0[k] -> (batch, m)"""
        b = np.ascontiguousarray(np.stack([B0[k][:, r] for k in range(self.batch)]))
        rc = L.dhqr_solve_batched_c64(h, self.pA(), self.m, self.n, self.lda, self.sA, self.pal(), self.sal, cptr(b), self.m, self.batch)
        assert rc == 0, L.dhqr_last_error()
        assert L.dhqr_synchronize(h) == 0
        return b


class ZOut:
    """`batch` complex result matrices (rows x cols, leading dimension rows + pad_ld, matrix k at off + k stride) in one flat
    SENT-filled buffer: the Q_k or R_k of a call"""

    def __init__(self, batch, rows, cols, pad_ld=2, pad=3, off=1):
        self.batch, self.rows, self.cols, self.off = batch, rows, cols, off
        self.ld, self.stride = rows + pad_ld, (rows + pad_ld) * cols + pad
        self.buf = _flat(batch * self.stride, off)
        self.mask = np.zeros(self.buf.size, bool)
        for k in range(batch):
            for j in range(cols):
                o = off + k * self.stride + j * self.ld
                self.mask[o: o + rows] = True

    def p(self):
        return cptr(self.buf[self.off:])

    def mat(self, k):
        o = self.off + k * self.stride
        return self.buf[o: o + self.ld * self.cols].reshape((self.ld, self.cols), order="F")[:self.rows]

    def padding_intact(self):
        return bool(np.all(self.buf[~self.mask] == SENT))

    def untouched(self):
        return bool(np.all(self.buf == SENT))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def eye_columns(m, n):
    """[I; 0] (m x n), complex"""
    E = np.zeros((m, n), dtype=np.complex128, order="F")
    E[np.arange(n), np.arange(n)] = 1
    return E


def reflect_clongdouble(H, B, trans):
    """Q^H B (trans) or Q B in np.clongdouble with the reflectors of the factor H (column c on and below the diagonal; the rows
    above hold R): H_c = I - v_c v_c^H (Hermitian), left to right for Q^H, right to left for Q"""
    Hl = np.asarray(H, dtype=np.clongdouble)
    X = np.array(B, dtype=np.clongdouble)
    n = Hl.shape[1]
    for c in (range(n) if trans else range(n - 1, -1, -1)):
        v = Hl[c:, c]
        X[c:] -= np.outer(v, np.conj(v) @ X[c:])
    return X


def check_close(got, want, what):
    """|got - want| <= TOL_Q max|want|; prints the figure first"""
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{what}: |d| / max|result| = {err / scale:.2e} (tol {TOL_Q:.0e})")
    assert err <= TOL_Q * scale, what


def check_x(orc, A, B, X, what):
    """every column of X within TOL_X max|x| of orc.solve_c on the oracle's own factor of A"""
    Ho, ao = orc.householder_c(A)
    worst = 0.0
    for r in range(B.shape[1]):
        xo = orc.solve_c(Ho, ao, np.ascontiguousarray(B[:, r]))
        worst = max(worst, float(np.abs(X[:, r] - xo).max() / np.abs(xo).max()))
    print(f"{what}: worst |dx| / max|x| = {worst:.2e} (tol {TOL_X:.0e})")
    assert worst <= TOL_X, what


def check_r(R, H, alpha):
    """R strictly upper = the bytes of H, diag(R) = the bytes of alpha, exact zeros below"""
    n = R.shape[0]
    assert R.shape == (n, n) and R.dtype == np.complex128
    assert not np.tril(R, -1).any(), "R is not upper triangular"
    assert np.ascontiguousarray(np.diagonal(R)).tobytes() == np.ascontiguousarray(alpha).tobytes(), "diag(R) != alpha"
    iu = np.triu_indices(n, 1)
    assert R[iu].tobytes() == np.asarray(H)[:n][iu].tobytes(), "strict upper part of R != H"


def check_qr(Q, R, A, what):
    """max|A - QR| and max|Q^H Q - I| at most zh.T(n) max|A|; prints the figures first"""
    n = Q.shape[1]
    scale = float(np.abs(A).max())
    res = float(np.abs(Q @ R - A).max())
    orth = float(np.abs(np.conj(Q.T) @ Q - np.eye(n)).max())
    bound = zh.T(n) * scale
    print(f"{what}: max|A - QR| = {res / bound:.3f}, max|Q^H Q - I| = {orth / bound:.3f} (in units of T(n) max|A| = {bound:.2e})")
    assert res <= bound and orth <= bound, what
