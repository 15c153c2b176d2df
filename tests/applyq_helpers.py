"""Test-only helpers of the tests of the batched / Float32 Q application, explicit Q and R (test_emulated_applyq.py,
test_gpu_applyq.py): the entry points dhqr_apply_q_batched_* / dhqr_form_q_batched_* / dhqr_form_r_batched_* driven through
the C ABI on the sentinel-filled strided batches of nrhs_helpers (factor and B in an NBatch, Q and R in an OutBatch), the
reflectors applied in np.longdouble (the reference of the accuracy criteria), the bounds.  The product never imports this
file."""
import numpy as np

import f32_helpers as F
from nrhs_helpers import NP, SENT, _flat, ptr

GPU_SHAPES = [(5, 3), (16, 8), (40, 17), (64, 32), (32, 32)]  # NC = 8 full, 16 and 32 barely entered and full, square


def tol(t):
    """|result - reference| <= tol(t) max|result|: Float64 the project's bound for Q'B (test_emulated_batched,
    test_gpu_nrhs), Float32 F.check_solve's (a column is carried in double and every entry rounded once: eps32 / 2)"""
    return 1e-12 if t == "f64" else 4 * F.EPS32


class OutBatch:
    """`batch` result matrices (rows x cols, leading dimension rows + pad_ld, matrix k at k stride) in one flat
    sentinel-filled buffer: the Q_k or R_k of a call"""

    def __init__(self, batch, rows, cols, t, pad_ld=2, pad=3, off=0):
        self.batch, self.rows, self.cols = batch, rows, cols
        self.ld, self.stride = rows + pad_ld, (rows + pad_ld) * cols + pad
        self.buf = _flat(batch * self.stride + 7, NP[t], off)
        self.mask = np.zeros(self.buf.size, bool)
        for k in range(batch):
            for j in range(cols):
                self.mask[k * self.stride + j * self.ld: k * self.stride + j * self.ld + rows] = True

    def mat(self, k):
        return self.buf[k * self.stride: k * self.stride + self.ld * self.cols].reshape((self.ld, self.cols), order="F")[:self.rows]

    def padding_intact(self):
        return bool(np.all(self.buf[~self.mask] == SENT))

    def untouched(self):
        return bool(np.all(self.buf == SENT))


def apply_q(L, h, D, trans, **kw):
    """dhqr_apply_q_batched_* in place on the B of the NBatch D; keyword arguments replace single arguments"""
    a = dict(A=ptr(D.A), m=D.m, n=D.n, lda=D.lda, sA=D.sA, B=ptr(D.B), nrhs=D.nrhs, ldb=D.ldb, sB=D.sB, batch=D.batch, trans=trans)
    a.update(kw)
    return getattr(L, f"dhqr_apply_q_batched_{D.t}")(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["B"], a["nrhs"], a["ldb"],
                                                     a["sB"], a["batch"], a["trans"])


def form_q(L, h, D, out, **kw):
    """dhqr_form_q_batched_* into the OutBatch `out`"""
    a = dict(A=ptr(D.A), m=D.m, n=D.n, lda=D.lda, sA=D.sA, Q=ptr(out.buf), ldq=out.ld, sQ=out.stride, batch=D.batch)
    a.update(kw)
    return getattr(L, f"dhqr_form_q_batched_{D.t}")(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["Q"], a["ldq"], a["sQ"], a["batch"])


def form_r(L, h, D, out, **kw):
    """dhqr_form_r_batched_* into the OutBatch `out`"""
    a = dict(A=ptr(D.A), m=D.m, n=D.n, lda=D.lda, sA=D.sA, al=ptr(D.al), sal=D.sal, R=ptr(out.buf), ldr=out.ld, sR=out.stride, batch=D.batch)
    a.update(kw)
    return getattr(L, f"dhqr_form_r_batched_{D.t}")(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["al"], a["sal"], a["R"], a["ldr"],
                                                    a["sR"], a["batch"])


def eye_columns(m, n, t):
    """[I; 0] (m x n)"""
    E = np.zeros((m, n), dtype=NP[t])
    E[np.arange(n), np.arange(n)] = 1
    return E


def reflect_longdouble(H, B, trans):
    """Q'B (trans) or QB in np.longdouble with the reflectors of the factor H (column c below and on the diagonal; the rows
    above hold R): H_c = I - v_c v_c', left to right for Q', right to left for Q"""
    Hl = np.asarray(H, dtype=np.longdouble)
    X = np.array(B, dtype=np.longdouble)
    n = Hl.shape[1]
    for c in (range(n) if trans else range(n - 1, -1, -1)):
        v = Hl[c:, c]
        X[c:] -= np.outer(v, v @ X[c:])
    return X


def check_r(R, H, alpha):
    """criterion 3 for one matrix: R upper triangular, diag(R) the bytes of alpha, the strict upper part the bytes of H"""
    n = R.shape[0]
    assert R.shape == (n, n) and R.dtype == H.dtype == alpha.dtype
    assert not np.tril(R, -1).any(), "R is not upper triangular"
    assert np.diagonal(R).tobytes() == np.ascontiguousarray(alpha).tobytes(), "diag(R) != alpha"
    iu = np.triu_indices(n, 1)
    assert R[iu].tobytes() == np.asarray(H)[:n][iu].tobytes(), "strict upper part of R != H"


def check_qr(Q, R, A, t, what=""):
    """criterion 3: Float64 |Q'Q - I|max < 1e-12 and ||QR - A|| / ||A|| < 1e-12 (test_explicit_q_and_r's bounds); Float32
    |Q'Q - I|max and max|QR - A| / max|A| at most F.tol_factor(n)"""
    n = Q.shape[1]
    Qd, Rd, Ad = (np.asarray(x, dtype=np.float64) for x in (Q, R, A))
    orth = np.abs(Qd.T @ Qd - np.eye(n)).max()
    if t == "f64":
        res = np.linalg.norm(Qd @ Rd - Ad) / np.linalg.norm(Ad)
        print(f"{what}: |Q'Q - I| = {orth:.2e}, ||QR - A||/||A|| = {res:.2e} (tol 1e-12)")
        assert orth < 1e-12 and res < 1e-12
    else:
        res = np.abs(Qd @ Rd - Ad).max() / np.abs(Ad).max()
        print(f"{what}: |Q'Q - I| = {orth / F.EPS32:.2f} eps32, max|QR - A|/max|A| = {res / F.EPS32:.2f} eps32 (tol {F.tol_factor(n) / F.EPS32:.0f})")
        assert orth <= F.tol_factor(n) and res <= F.tol_factor(n)
