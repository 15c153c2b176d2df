"""Test-only helpers of the tests of `H \\ B` with several right-hand sides (test_emulated_nrhs.py, test_gpu_nrhs.py): the
shapes and seeds both files share, the seeded inputs, a strided batch (A_k, alpha_k, B_k, X_k) in flat sentinel-filled
buffers driven through the C ABI, a plain-double numpy twin of the solve (used to choose seeds on the CPU: the twin must
stay inside the oracle bound at the seeds the tests use).  The product never imports this file."""
import ctypes

import numpy as np

P = ctypes.c_void_p
SENT = -7.25  # fills every element between and behind the matrices of a batch (exact in float32)
EINVAL = -1

# NC = 8 full, NC = 16 barely entered, NC = 32 barely entered and full, the square case
WAVE_SHAPES = [(1, 1), (5, 3), (16, 8), (33, 9), (40, 17), (64, 32), (32, 32)]
NRHS = [1, 3, 4, 5, 9]       # below, at and above a group of four, a tail of one (Float64 NC >= 16 groups by three: 9 = 3 full)
# The library sends a call to the multi-column kernel only where it pays (dhqr.h: 5 nrhs >= 13 groups), to the column loop
# elsewhere -- the same bits.  Of the list above the kernel runs 3, 4 and 9 in groups of four (a tail of three, a full group,
# a tail of one) and 3 and 9 in groups of three (full groups only); 8 and 13 add the tails of two and of one there
# (groups of four: 8 two full groups, 13 a tail of one).
NRHS_KERNEL_TAILS = [8, 13]
NRHS_ALL = NRHS + NRHS_KERNEL_TAILS
NRHS_MAX = max(NRHS_ALL)
BATCHES = [1, 5, 300]        # 5 is no multiple of the four matrices of a workgroup
BEYOND = [(66, 33, 3), (130, 20, 3), (300, 40, 2)]  # (m, n, batch): one-workgroup tier twice, serial tier; nrhs = 3
SEED = 100                   # (test_gpu_batched.py's; twin_worst() below stays inside 1e-9 at it for every wave shape)
DTYPES = ["f64", "f32"]
NP = {"f64": np.float64, "f32": np.float32}


def ptr(a):
    return a.ctypes.data_as(P)


def inputs(orc, m, n, nrhs, batch, seed, t="f64", ks=None):
    """(mats[k] (m, n), Bs[k] (m, nrhs)) for k in ks (default: every k < batch): A_k = rand_matrix(m, n, seed + k), column r
    of B_k = rand_vector(m, seed + 5000 + 1000 r + k); float32: the same values, rounded"""
    ks = range(batch) if ks is None else ks
    mats = [np.asarray(orc.rand_matrix(m, n, seed + k), dtype=NP[t]) for k in ks]
    Bs = [np.stack([orc.rand_vector(m, seed + 5000 + 1000 * r + k) for r in range(nrhs)], axis=1).astype(NP[t]) for k in ks]
    return mats, Bs


def twin_solve64(H, al, b):
    """solve_householder!(b, H, alpha) in plain double (numpy)"""
    m, n = H.shape
    b = np.array(b, dtype=np.float64)
    for j in range(n):
        b[j:] -= H[j:, j] * (H[j:, j] @ b[j:])
    for j in range(n - 1, -1, -1):
        b[j] /= al[j]
        b[:j] -= H[:j, j] * b[j]
    return b[:n]


def twin_factor64(A):
    """householder!(A, alpha) in plain double (numpy): the reference's column-by-column order"""
    a = np.array(A, dtype=np.float64, order="F")
    m, n = a.shape
    alpha = np.zeros(n)
    for j in range(n):
        s = np.sqrt(float(a[j:, j] @ a[j:, j]))
        h = a[j, j]
        f = 1.0 / np.sqrt(s * (s + abs(h)))
        alpha[j] = -np.sign(h) * s
        a[j, j] = h - alpha[j]
        a[j:, j] *= f
        if j + 1 < n:
            a[j:, j + 1:] -= np.outer(a[j:, j], a[j:, j] @ a[j:, j + 1:])
    return a, alpha


def oracle_errors(orc, mats, Bs, X):
    """(worst |X_k[:, r] - oracle| / |oracle| over k and r, the same for the plain-double twin); X[k]: (n, nrhs) float64"""
    worst = twin = 0.0
    for k, (A, B) in enumerate(zip(mats, Bs)):
        Ho, ao = orc.householder(np.asfortranarray(A, dtype=np.float64))
        Ht, at = twin_factor64(A)
        for r in range(B.shape[1]):
            xo = orc.solve(Ho, ao, np.ascontiguousarray(B[:, r], dtype=np.float64))
            s = np.abs(xo).max()
            worst = max(worst, float(np.abs(X[k][:, r] - xo).max() / s))
            twin = max(twin, float(np.abs(twin_solve64(Ht, at, B[:, r]) - xo).max() / s))
    return worst, twin


def _flat(count, dtype, off=0):
    """1-D sentinel-filled buffer of `count` elements whose first element lies `off` elements behind a 256-byte boundary"""
    isz = np.dtype(dtype).itemsize
    raw = np.empty(count + off + 256 // isz, dtype=dtype)
    s = (-raw.ctypes.data % 256) // isz + off
    buf = raw[s:s + count]
    buf[:] = SENT
    assert buf.ctypes.data % 256 == off * isz
    return buf


class NBatch:
    """a strided batch in flat sentinel-filled buffers: matrix k at A[k*sA:] (leading dimension lda), alpha_k at al[k*sal:],
    B_k (m x nrhs) at B[k*sB:] (ldb), X_k (n x nrhs, the host forms' result) at X[k*sX:] (ldx)"""

    def __init__(self, mats, Bs, t="f64", pad_ld=3, pad=5, pad_ldb=1, pad_ldx=2, off=0):
        self.t, dt = t, NP[t]
        self.batch, (self.m, self.n), self.nrhs = len(mats), mats[0].shape, Bs[0].shape[1]
        m, n, nrhs, batch = self.m, self.n, self.nrhs, self.batch
        self.lda, self.ldb, self.ldx = m + pad_ld, m + pad_ldb, n + pad_ldx
        self.sA, self.sal = self.lda * n + pad, n + pad
        self.sB, self.sX = self.ldb * nrhs + pad, self.ldx * nrhs + pad
        self.A, self.al = _flat(batch * self.sA + 7, dt, off), _flat(batch * self.sal + 7, dt, off)
        self.B, self.X = _flat(batch * self.sB + 7, dt, off), _flat(batch * self.sX + 7, dt, off)
        self.maskA, self.maskal = np.zeros(self.A.size, bool), np.zeros(self.al.size, bool)
        self.maskB, self.maskX = np.zeros(self.B.size, bool), np.zeros(self.X.size, bool)
        for k in range(batch):
            self.mat(k)[...] = mats[k]
            self.bmat(k)[...] = Bs[k]
            self.maskal[k * self.sal: k * self.sal + n] = True
            for j in range(n):
                self.maskA[k * self.sA + j * self.lda: k * self.sA + j * self.lda + m] = True
            for r in range(nrhs):
                self.maskB[k * self.sB + r * self.ldb: k * self.sB + r * self.ldb + m] = True
                self.maskX[k * self.sX + r * self.ldx: k * self.sX + r * self.ldx + n] = True

    def _win(self, buf, k, stride, ld, rows, cols):
        return buf[k * stride: k * stride + ld * cols].reshape((ld, cols), order="F")[:rows]

    def mat(self, k):
        return self._win(self.A, k, self.sA, self.lda, self.m, self.n)

    def alpha(self, k):
        return self.al[k * self.sal: k * self.sal + self.n]

    def bmat(self, k):
        return self._win(self.B, k, self.sB, self.ldb, self.m, self.nrhs)

    def xmat(self, k):
        return self._win(self.X, k, self.sX, self.ldx, self.n, self.nrhs)

    def padding_intact(self):
        return all(np.all(buf[~mask] == SENT) for buf, mask in
                   ((self.A, self.maskA), (self.al, self.maskal), (self.B, self.maskB), (self.X, self.maskX)))

    def x_untouched(self):
        return bool(np.all(self.X == SENT))

    def factor(self, L, h):
        return getattr(L, f"dhqr_factor_batched_{self.t}")(h, ptr(self.A), self.m, self.n, self.lda, self.sA, ptr(self.al),
                                                           self.sal, self.batch, 0)

    def solve_nrhs(self, L, h, **kw):
        """the device form, in place on B; keyword arguments replace single arguments (the argument tests)"""
        a = dict(A=ptr(self.A), m=self.m, n=self.n, lda=self.lda, sA=self.sA, al=ptr(self.al), sal=self.sal, B=ptr(self.B),
                 nrhs=self.nrhs, ldb=self.ldb, sB=self.sB, batch=self.batch)
        a.update(kw)
        return getattr(L, f"dhqr_solve_batched_nrhs_{self.t}")(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["al"], a["sal"],
                                                               a["B"], a["nrhs"], a["ldb"], a["sB"], a["batch"])

    def ldiv_nrhs(self, L, h, **kw):
        """the host form: B is read, X written"""
        a = dict(A=ptr(self.A), m=self.m, n=self.n, lda=self.lda, sA=self.sA, al=ptr(self.al), sal=self.sal, B=ptr(self.B),
                 nrhs=self.nrhs, ldb=self.ldb, sB=self.sB, X=ptr(self.X), ldx=self.ldx, sX=self.sX, batch=self.batch)
        a.update(kw)
        return getattr(L, f"dhqr_ldiv_batched_nrhs_{self.t}")(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["al"], a["sal"],
                                                              a["B"], a["nrhs"], a["ldb"], a["sB"], a["X"], a["ldx"], a["sX"],
                                                              a["batch"])

    def single_column(self, L, h, r, B0):
        """today's call on column r alone: dhqr_solve_batched_* on a packed copy of the columns r of B0[k] -> (batch, m)"""
        b = np.ascontiguousarray(np.stack([B0[k][:, r] for k in range(self.batch)]), dtype=NP[self.t])
        rc = getattr(L, f"dhqr_solve_batched_{self.t}")(h, ptr(self.A), self.m, self.n, self.lda, self.sA, ptr(self.al), self.sal,
                                                        ptr(b), self.m, self.batch)
        assert rc == 0, L.dhqr_last_error()
        assert L.dhqr_synchronize(h) == 0
        return b


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
