"""Test-only helpers of the batched ComplexF64 tests (test_gpu_batched_complex.py, test_emulated_batched_complex.py): the
inputs, the tolerance rule against the oracle, and a strided sentinel-guarded batch for calls through the C ABI.
The product never imports this file.

THE RULE.  T = 8 max(n, 8) eps relative to max|H| (TOL of test_gpu_complex.py), element-wise on H and alpha.  Two correct
restatements of the reference that differ only in summation order (the oracle and its numpy twin) agree to a median of
0.04 T, but rare matrices of ordinary condition number land above T: of 300 matrices (seeds 100 .. 399, right-hand sides
5100 + k) none at (1,1) (5,3) (12,6) (16,8) (40,17) (64,32) (32,32) (worst 0.93 T), one at (33,9) (1.12 T), two at (66,33)
(3.43 T), one at (130,20) (1.22 T).  So: NO matrix above 8 T, and at most 1 % of a batch of 300 above T; a small batch
(nine matrices, or the seven special ones) may have ONE above T -- the worst the reference pair does at any shape is one
in 150.  x: within 1e-9 max|x| (test_gpu_batched.py); the reference pair stays below 4e-14.  A dropped term, a wrong sign
or a float accumulator is orders of magnitude outside 8 T."""
import ctypes

import numpy as np

EPS = np.finfo(np.float64).eps
SEED, BSEED = 100, 5100  # matrix k: rand_matrix_c(m, n, SEED + k); right-hand side k: rand_vector_c(m, BSEED + k)
WAVE_SHAPES = [(1, 1), (5, 3), (12, 6), (16, 8), (33, 9), (40, 17), (64, 32), (32, 32)]
SENT = complex(-7.25, 3.5)  # fills every element between and behind the matrices / vectors of a guarded batch
P = ctypes.c_void_p


def T(n):
    return 8.0 * max(int(n), 8) * EPS


def inputs(orc, m, n, ks, seed=SEED, bseed=BSEED):
    return [orc.rand_matrix_c(m, n, seed + k) for k in ks], [orc.rand_vector_c(m, bseed + k) for k in ks]


def reference(orc, A0, b0=None):
    Ho, ao = orc.householder_c(A0)
    return Ho, ao, (orc.solve_c(Ho, ao, b0) if b0 is not None else None)


def ratio_H(Ho, ao, H, al):
    """max(|dH|, |dalpha|) / (T max|H|) of one matrix"""
    scale = np.abs(Ho).max()
    return max(np.abs(H - Ho).max(), np.abs(al - ao).max()) / (T(Ho.shape[1]) * scale)


def check_rule(label, ratios, dxs, above_allowed):
    """the rule of this module's docstring on the per-matrix ratios (in units of T) and |dx| / max|x|; prints what it measured"""
    ratios, dxs = np.asarray(ratios, dtype=float), np.asarray(dxs, dtype=float)
    above = int((ratios > 1.0).sum())
    print(f"{label}: {len(ratios)} matrices vs oracle: worst {ratios.max():.3f} T, median {np.median(ratios):.3f} T, "
          f"{above} above T (allowed {above_allowed}); worst |dx|/max|x| {dxs.max() if len(dxs) else 0.0:.2e} (tol 1e-9)")
    assert np.isfinite(ratios).all() and np.isfinite(dxs).all()
    assert ratios.max() <= 8.0, f"{label}: a matrix is {ratios.max():.2f} T from the oracle (cap 8 T)"
    assert above <= above_allowed, f"{label}: {above} matrices above T (allowed {above_allowed})"
    if len(dxs):
        assert dxs.max() <= 1e-9


def special_matrices(orc, m, n, seed=900):
    """seven matrices: ordinary ones, an imaginary part identically zero, a real part identically zero, a first column whose
    pivot is exactly 0 above a nonzero rest (alphafactor(0) = -1, src:9) -- alone and together with a zero imaginary part"""
    mats = [orc.rand_matrix_c(m, n, seed + k) for k in range(7)]
    mats[1] = np.asfortranarray(mats[1].real + 0j)
    mats[2] = np.asfortranarray(1j * mats[2].imag)
    mats[3][0, 0] = 0.0
    mats[5] = np.asfortranarray(mats[5].real + 0j)
    mats[5][0, 0] = 0.0
    return mats


def poison_column(A, col=3):
    """a copy of A whose column `col` is identically zero: the oracle (like the reference) leaves columns < col finite, alpha_col
    = -0 and everything from row `col` on of the columns >= col non-finite"""
    B = A.copy(order="F")
    B[:, col] = 0.0
    return B


def cptr(a):
    return a.ctypes.data_as(P)


class ZBatch:
    """a strided batch of complex matrices in flat SENT-filled host buffers (for the EMULATED library, whose "device" memory
    is host memory): matrix k at A[off + k*sA:], leading dimension lda; everything counts complex elements; `off` complex
    elements in front of every array (numpy buffers are 16-byte aligned and stay so)"""

    def __init__(self, mats, bs, pad_ld=1, pad=5, off=1):
        self.batch, (self.m, self.n) = len(mats), mats[0].shape
        m, n = self.m, self.n
        self.off = off
        self.lda = m + pad_ld
        self.sA = self.lda * n + pad
        self.sal = n + (3 if pad else 0)
        self.sb = m + pad
        self.A = np.full(off + self.batch * self.sA + 7, SENT)
        self.al = np.full(off + self.batch * self.sal + 7, SENT)
        self.b = np.full(off + self.batch * self.sb + 7, SENT)
        self.maskA, self.maskal, self.maskb = (np.zeros(v.size, bool) for v in (self.A, self.al, self.b))
        for k in range(self.batch):
            self.mat(k)[...] = mats[k]
            for j in range(n):
                self.maskA[off + k * self.sA + j * self.lda: off + k * self.sA + j * self.lda + m] = True
            self.maskal[off + k * self.sal: off + k * self.sal + n] = True
            self.rhs(k)[...] = bs[k]
            self.maskb[off + k * self.sb: off + k * self.sb + m] = True

    def mat(self, k):
        o = self.off + k * self.sA
        return self.A[o: o + self.lda * self.n].reshape((self.lda, self.n), order="F")[:self.m]

    def alpha(self, k):
        return self.al[self.off + k * self.sal: self.off + k * self.sal + self.n]

    def rhs(self, k):
        return self.b[self.off + k * self.sb: self.off + k * self.sb + self.m]

    def padding_intact(self):
        return bool(np.all(self.A[~self.maskA] == SENT) and np.all(self.al[~self.maskal] == SENT) and np.all(self.b[~self.maskb] == SENT))

    def pA(self):
        return cptr(self.A[self.off:])

    def pal(self):
        return cptr(self.al[self.off:])

    def pb(self):
        return cptr(self.b[self.off:])

    def factor(self, L, h, nb=0):
        return L.dhqr_factor_batched_c64(h, self.pA(), self.m, self.n, self.lda, self.sA, self.pal(), self.sal, self.batch, nb)

    def solve(self, L, h):
        return L.dhqr_solve_batched_c64(h, self.pA(), self.m, self.n, self.lda, self.sA, self.pal(), self.sal, self.pb(), self.sb,
                                        self.batch)
