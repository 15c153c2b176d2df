"""Test-only helpers of the tests of the column-pivoted batched QR and the rank-revealing least squares for Float32 and
ComplexF64 (test_emulated_pivoted_types.py, test_gpu_pivoted_types.py), modelled on pivoted_helpers.py: a numpy twin of the
rule of include/dhqr.h per type, the shapes and inputs both files share, a strided batch with jpvt and rank in
sentinel-filled buffers driven through the C ABI of the ten symbols dhqr_*_f32 / dhqr_*_c64 -- on the emulated library,
where a numpy buffer IS device memory, or on the GPU, where every buffer is copied to the device, guards and all, and back
-- and the checks themselves, written once for both files and both types ("f32", "c64").  The product never imports this file.

THE TWIN.  Float32: float32 storage, every sum in double, every stored entry rounded once (f32_helpers.twin_factor with
the pivot step and alphafactor(0) = -1).  ComplexF64: plain complex double, alpha = -h / |h| ||x|| (-||x|| at h = 0).
The twin asserts a GAP precondition at every step: the two largest remaining squared norms differ, relatively, by more
than 1e-10 (ComplexF64) or 1e-5 (Float32); a seed that misses it is changed, the bound is not.

MEASURED on the seeds used here, on the CPU, with the twin alone (`python pivoted_types_helpers.py` prints it again): the
smallest gap at a step where a pivot is compared is 1.4e-4 (f32) and 1.8e-4 (c64).  On the low-rank sets the twin's
|alpha_j / alpha_0| are: Float32 kept >= 3.7e-3, dropped <= 5.7e-8 (rcond 1e-5); ComplexF64 kept >= 6.0e-2, dropped <=
6.2e-16 (rcond 1e-10).

THE SOLUTION CHECK (pivoted_helpers.check_solution's): ||A^H (A x - b)|| at most 8 x the statistic of numpy.linalg.lstsq on
the widened inputs plus a floor -- 1e-13 ||A||^2 ||b|| for ComplexF64 (the project's figure), that figure scaled by
eps32 / eps64 = 2^29 for Float32 --, and the norm of the tail rows equal to ||A x - b|| within 1e-11 ||b|| (c64) or
1e-11 2^29 ||b|| (f32).  The twin's own solution (Float32: rounded to float32) was run through the same check on the CPU
on every set used here and passes everywhere with the floors as stated, so no floor is replaced: its worst statistic /
bound is 1.4e-3 for both types (f32: 32 x 32; c64: 5 x 3), its worst tail figure / tolerance 2.3e-3 (f32) and 4.6e-4 (c64),
both at 32 x 32."""
import ctypes

import numpy as np

import applyq_helpers as Q
import f32_helpers as F
import pivoted_helpers as PV
import zapplyq_helpers as ZQ
import zbatched_helpers as zh
from nrhs_helpers import EINVAL, P, SENT, _flat, ptr, same_bytes

TYPES = ["f32", "c64"]
NP = {"f32": np.float32, "c64": np.complex128}
WIDE = {"f32": np.float64, "c64": np.complex128}  # what the references compute in
WAVE_SHAPES = [(5, 3), (16, 8), (40, 17), (64, 32), (32, 32)]  # NC = 8 full, 16 and 32 barely entered and full, square
GENERAL_SHAPES = [(66, 33), (130, 20)]
LOW_RANK = [(16, 8, 3), (40, 17, 9), (64, 32, 1), (64, 32, 31), (66, 33, 10)]  # (m, n, r0)
BATCH, NRHS = 4, 3
SEED = PV.SEED
RCOND = {"f32": 1e-5, "c64": 1e-10}
GAP = {"f32": 1e-5, "c64": 1e-10}
EPSRATIO = {"f32": 2.0 ** 29, "c64": 1.0}  # eps32 / eps64: the Float32 floors are the Float64 figures scaled by it
MONO = {"f32": 1 + 4 * F.EPS32, "c64": 1 + 1e-12}  # |alpha_j| does not increase, within
ISENT = PV.ISENT


# ---- inputs ----------------------------------------------------------------------------------------------------------
def inputs(orc, t, m, n, nrhs=NRHS, batch=BATCH, seed=SEED):
    """the project's generator with column c scaled by 1 + 0.25 c: full rank, well separated column norms.  Float32:
    pivoted_helpers.inputs, rounded; ComplexF64: zbatched_helpers.inputs for the matrices, zapplyq_helpers' right-hand sides"""
    scale = 1.0 + 0.25 * np.arange(n)
    if t == "f32":
        mats, Bs = PV.inputs(orc, m, n, nrhs, batch, seed)
        return [np.asfortranarray(A, dtype=np.float32) for A in mats], [np.asfortranarray(B, dtype=np.float32) for B in Bs]
    mats = [np.asfortranarray(A * scale) for A in zh.inputs(orc, m, n, range(batch), seed=seed)[0]]
    Bs = [np.asfortranarray(np.stack([orc.rand_vector_c(m, seed + 5000 + 1000 * r + k) for r in range(nrhs)], axis=1)) for k in range(batch)]
    return mats, Bs


def low_rank_inputs(t, m, n, r0, nrhs=NRHS, batch=BATCH, seed=SEED):
    """A_k = X_k Y_k with uniform factors: rank r0 up to rounding.  Float32: pivoted_helpers.low_rank_inputs (the product
    formed in double), rounded; ComplexF64: real and imaginary parts uniform in (-1, 1)"""
    if t == "f32":
        mats, Bs = PV.low_rank_inputs(m, n, r0, nrhs, batch, seed)
        return [np.asfortranarray(A, dtype=np.float32) for A in mats], [np.asfortranarray(B, dtype=np.float32) for B in Bs]
    rng = np.random.default_rng(seed + 7 * m + n + r0)

    def u(*shape):
        return rng.uniform(-1, 1, size=shape) + 1j * rng.uniform(-1, 1, size=shape)
    mats = [np.asfortranarray(u(m, r0) @ u(r0, n)) for _ in range(batch)]
    Bs = [np.asfortranarray(u(m, nrhs)) for _ in range(batch)]
    return mats, Bs


# ---- the numpy twin --------------------------------------------------------------------------------------------------
def twin_factor(t, A, check_gap=False, gaps=None):
    """(H, alpha, jpvt) of the pivoted factorisation by the rule of include/dhqr.h for the type t.  check_gap: assert the
    precondition GAP[t] at every step; gaps: a list that receives every step's relative gap"""
    a = np.array(A, dtype=NP[t], order="F")
    m, n = a.shape
    alpha, jpvt = np.zeros(n, dtype=NP[t]), np.arange(n, dtype=np.int32)
    for j in range(n):
        w = a[j:, j:].astype(WIDE[t])
        nrm = (w.real ** 2 + w.imag ** 2).sum(axis=0)  # afresh from the working matrix, in double
        p = j + int(np.argmax(nrm))                    # the first maximum
        if nrm[p - j] == 0.0:                          # the rest is zero: alpha_c = 0, v_c = sqrt(2) e_c (real)
            for c in range(j, n):
                a[c:, c] = 0.0
                a[c, c] = NP[t](np.sqrt(2.0))
            break
        if n - j > 1:
            s = np.sort(nrm)
            gap = (s[-1] - s[-2]) / s[-1]
            if gaps is not None:
                gaps.append(gap)
            assert not check_gap or gap > GAP[t], f"step {j}: the two largest norms are closer than {GAP[t]} relative ({gap:.1e})"
        a[:, [j, p]] = a[:, [p, j]]
        jpvt[[j, p]] = jpvt[[p, j]]
        x = a[:, j].astype(WIDE[t])
        s = np.sqrt(float((x[j:].real ** 2 + x[j:].imag ** 2).sum()))
        h = x[j]
        ah = abs(h)
        al = s * ((-h / ah) if ah != 0 else -1.0) if t == "c64" else s * (-1.0 if h >= 0 else 1.0)
        f = 1.0 / np.sqrt(s * (s + ah))
        v = np.zeros(m, dtype=WIDE[t])
        v[j] = (h - al) * f
        v[j + 1:] = x[j + 1:] * f
        vs = v.astype(NP[t])  # (Float32: rounded once; the trailing update uses the stored reflector)
        a[j:, j] = vs[j:]
        alpha[j] = NP[t](al)
        if j + 1 < n:
            vd = vs[j:].astype(WIDE[t])
            T = a[j:, j + 1:].astype(WIDE[t])
            a[j:, j + 1:] = (T - np.outer(vd, np.conj(vd) @ T)).astype(NP[t])
    return a, alpha, jpvt


def twin_rank(t, alpha, rcond, m):
    n = len(alpha)
    rc = rcond if rcond >= 0 else max(m, n) * (2.0 ** -23 if t == "f32" else 2.0 ** -52)
    a = np.abs(np.asarray(alpha, dtype=WIDE[t]))  # (compared in double)
    r = 0
    while r < n and a[r] > rc * a[0]:
        r += 1
    return r


def twin_solve(t, H, alpha, jpvt, r, b):
    """(b <- [z; tail], x) of the truncated solve carried in double, rounded to the type once at the end"""
    Hw, aw = np.asarray(H, dtype=WIDE[t]), np.asarray(alpha, dtype=WIDE[t])
    n = Hw.shape[1]
    b = np.array(b, dtype=WIDE[t])
    for j in range(r):
        b[j:] -= Hw[j:, j] * (np.conj(Hw[j:, j]) @ b[j:])
    for j in range(r - 1, -1, -1):
        b[j] /= aw[j]
        b[:j] -= Hw[:j, j] * b[j]
    b = b.astype(NP[t])
    x = np.zeros(n, dtype=NP[t])
    x[jpvt[:r]] = b[:r]
    return b, x


# ---- a strided batch with jpvt and rank ------------------------------------------------------------------------------
class TBatch:
    """a strided batch of the type t in flat sentinel-filled buffers: matrix k at A[k*sA:] (leading dimension lda), alpha_k at
    al[k*sal:], B_k (m x nrhs) at B[k*sB:] (ldb), X_k (n x nrhs) at X[k*sX:] (ldx), jpvt_k (n int32) at jp[k*sjp:], rank[k] at
    rk[k]; ComplexF64 counts complex elements.  off: every base `off` elements behind a 256-byte boundary"""
    BUFS = ("A", "al", "B", "X", "jp", "rk")

    def __init__(self, t, mats, Bs, pad_ld=3, pad=5, pad_ldb=1, pad_ldx=2, pad_jp=3, off=0):
        self.t, dt = t, NP[t]
        self.batch, (self.m, self.n), self.nrhs = len(mats), mats[0].shape, Bs[0].shape[1]
        m, n, nrhs, batch = self.m, self.n, self.nrhs, self.batch
        self.off = off
        self.lda, self.ldb, self.ldx = m + pad_ld, m + pad_ldb, n + pad_ldx
        self.sA, self.sal, self.sjp = self.lda * n + pad, n + pad, n + pad_jp
        self.sB, self.sX = self.ldb * nrhs + pad, self.ldx * nrhs + pad
        self.A, self.al = _flat(batch * self.sA + 7, dt, off), _flat(batch * self.sal + 7, dt, off)
        self.B, self.X = _flat(batch * self.sB + 7, dt, off), _flat(batch * self.sX + 7, dt, off)
        self.jp, self.rk = _flat(batch * self.sjp + 7, np.int32, off), _flat(batch + 7, np.int32, off)
        self.mask = {nm: np.zeros(getattr(self, nm).size, bool) for nm in self.BUFS}
        self.mask["rk"][:batch] = True
        for k in range(batch):
            self.mat(k)[...] = mats[k]
            self.bmat(k)[...] = Bs[k]
            self.mask["al"][k * self.sal: k * self.sal + n] = True
            self.mask["jp"][k * self.sjp: k * self.sjp + n] = True
            for j in range(n):
                self.mask["A"][k * self.sA + j * self.lda: k * self.sA + j * self.lda + m] = True
            for r in range(nrhs):
                self.mask["B"][k * self.sB + r * self.ldb: k * self.sB + r * self.ldb + m] = True
                self.mask["X"][k * self.sX + r * self.ldx: k * self.sX + r * self.ldx + n] = True

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

    def jpvt(self, k):
        return self.jp[k * self.sjp: k * self.sjp + self.n]

    def ranks(self):
        return self.rk[:self.batch]

    def padding_intact(self):
        return all(bool(np.all(getattr(self, nm)[~self.mask[nm]] == (ISENT if nm in ("jp", "rk") else SENT))) for nm in self.BUFS)

    def untouched(self, *names):
        return all(bool(np.all(getattr(self, nm) == (ISENT if nm in ("jp", "rk") else SENT))) for nm in names)

    def set_factor(self, Hs, als, jps, ranks=None):
        for k in range(self.batch):
            self.mat(k)[...] = Hs[k]
            self.alpha(k)[...] = als[k]
            self.jpvt(k)[...] = jps[k]
        if ranks is not None:
            self.ranks()[...] = ranks
        return self


class Runner:
    """calls the C ABI of the type t on the buffers of a batch.  torch = None: the emulated library, numpy memory is device
    memory.  Else: every buffer goes to the GPU (at the same offset from an aligned base), the call runs there, every buffer
    comes back."""

    def __init__(self, L, h, t, torch=None):
        self.L, self.h, self.t, self.torch = L, h, t, torch

    def sync(self):
        assert self.L.dhqr_synchronize(self.h) == 0, self.L.dhqr_last_error()

    def call(self, name, D, args, host=False, null=()):
        """fn(h, *args(p)) with p(buffer name) -> pointer (a name in `null`: a null pointer); returns rc, synchronised"""
        fn = getattr(self.L, f"{name}_{self.t}")
        if self.torch is None or host:
            rc = fn(self.h, *args(lambda nm: P(None) if nm in null else ptr(getattr(D, nm))))
            self.sync()
            return rc
        torch, dev = self.torch, {}
        for nm in D.BUFS:
            buf = getattr(D, nm)
            t = torch.empty(buf.size + D.off, dtype=torch.from_numpy(buf[:1]).dtype, device="cuda:0")[D.off:]
            t.copy_(torch.from_numpy(buf))
            dev[nm] = t
        torch.cuda.synchronize()
        rc = fn(self.h, *args(lambda nm: P(None) if nm in null else P(dev[nm].data_ptr())))
        self.sync()
        for nm in D.BUFS:
            getattr(D, nm)[...] = dev[nm].cpu().numpy()
        return rc

    def ok(self, rc):
        assert rc == 0, self.L.dhqr_last_error()

    # keyword arguments replace single arguments (the argument tests)
    def factor(self, D, null=(), **kw):
        a = dict(m=D.m, n=D.n, lda=D.lda, sA=D.sA, sal=D.sal, sjp=D.sjp, batch=D.batch)
        a.update(kw)
        return self.call("dhqr_factor_batched_pivoted", D, lambda p: (p("A"), a["m"], a["n"], a["lda"], a["sA"], p("al"), a["sal"],
                                                                     p("jp"), a["sjp"], a["batch"]), null=null)

    def factor_unpivoted(self, D):
        return self.call("dhqr_factor_batched", D, lambda p: (p("A"), D.m, D.n, D.lda, D.sA, p("al"), D.sal, D.batch, 0))

    def rank(self, D, rcond, null=(), **kw):
        a = dict(m=D.m, n=D.n, sal=D.sal, batch=D.batch)
        a.update(kw)
        return self.call("dhqr_rank_batched", D, lambda p: (p("al"), a["m"], a["n"], a["sal"], rcond, p("rk"), a["batch"]), null=null)

    def solve(self, D, null=(), **kw):
        a = dict(m=D.m, n=D.n, lda=D.lda, sA=D.sA, sal=D.sal, sjp=D.sjp, nrhs=D.nrhs, ldb=D.ldb, sB=D.sB, ldx=D.ldx, sX=D.sX, batch=D.batch)
        a.update(kw)
        return self.call("dhqr_solve_batched_pivoted", D, lambda p: (
            p("A"), a["m"], a["n"], a["lda"], a["sA"], p("al"), a["sal"], p("jp"), a["sjp"], p("rk"), p("B"), a["nrhs"], a["ldb"], a["sB"],
            p("X"), a["ldx"], a["sX"], a["batch"]), null=null)

    def solve_unpivoted(self, D, n=None):
        """the type's unpivoted multi-column solve, dhqr_solve_batched_nrhs_*, with the first n columns of the factor"""
        n = D.n if n is None else n
        return self.call("dhqr_solve_batched_nrhs", D, lambda p: (p("A"), D.m, n, D.lda, D.sA, p("al"), D.sal, p("B"), D.nrhs, D.ldb,
                                                                 D.sB, D.batch))

    def qr_host(self, D, null=(), **kw):
        a = dict(m=D.m, n=D.n, lda=D.lda, sA=D.sA, sal=D.sal, sjp=D.sjp, batch=D.batch)
        a.update(kw)
        return self.call("dhqr_qr_batched_pivoted", D, lambda p: (p("A"), a["m"], a["n"], a["lda"], a["sA"], p("al"), a["sal"], p("jp"),
                                                                 a["sjp"], a["batch"]), host=True, null=null)

    def lstsq(self, D, rcond, null=(), **kw):
        a = dict(m=D.m, n=D.n, lda=D.lda, sA=D.sA, nrhs=D.nrhs, ldb=D.ldb, sB=D.sB, ldx=D.ldx, sX=D.sX, batch=D.batch)
        a.update(kw)
        return self.call("dhqr_lstsq_batched", D, lambda p: (p("A"), a["m"], a["n"], a["lda"], a["sA"], p("B"), a["nrhs"], a["ldb"],
                                                            a["sB"], rcond, p("X"), a["ldx"], a["sX"], p("rk"), a["batch"]),
                         host=True, null=null)

    def q_and_r(self, D):
        """(Q_k, R_k) of the factors in D by the EXISTING dhqr_form_q_batched_* / dhqr_form_r_batched_*"""
        dt, m, n = NP[self.t], D.m, D.n
        fq, fr = getattr(self.L, f"dhqr_form_q_batched_{self.t}"), getattr(self.L, f"dhqr_form_r_batched_{self.t}")
        out = []
        for k in range(D.batch):
            H, al = np.array(D.mat(k), order="F"), D.alpha(k).copy()
            if self.torch is None:
                Qm, Rm = np.full((m, n), SENT, dtype=dt, order="F"), np.full((n, n), SENT, dtype=dt, order="F")
                self.ok(fq(self.h, ptr(H), m, n, m, m * n, ptr(Qm), m, m * n, 1))
                self.ok(fr(self.h, ptr(H), m, n, m, m * n, ptr(al), n, ptr(Rm), n, n * n, 1))
                self.sync()
            else:
                tc = self.torch
                dH, dal = tc.from_numpy(H.T.copy()).cuda(), tc.from_numpy(al).cuda()  # (n, m) row-major = (m, n) column-major
                dQ, dR = tc.empty((n, m), dtype=dH.dtype, device="cuda:0"), tc.empty((n, n), dtype=dH.dtype, device="cuda:0")
                tc.cuda.synchronize()
                self.ok(fq(self.h, P(dH.data_ptr()), m, n, m, m * n, P(dQ.data_ptr()), m, m * n, 1))
                self.ok(fr(self.h, P(dH.data_ptr()), m, n, m, m * n, P(dal.data_ptr()), n, P(dR.data_ptr()), n, n * n, 1))
                self.sync()
                Qm, Rm = dQ.cpu().numpy().T, dR.cpu().numpy().T
            out.append((Qm, Rm))
        return out


def factored(R, mats, Bs, **layout):
    """a TBatch holding the pivoted factors of `mats` (device form), checked for its guards"""
    D = TBatch(R.t, mats, Bs, **layout)
    R.ok(R.factor(D))
    assert D.padding_intact() and D.untouched("X", "rk")
    return D


def snapshot(D):
    """(H_k, alpha_k, jpvt_k) copies"""
    return ([np.array(D.mat(k), order="F") for k in range(D.batch)], [D.alpha(k).copy() for k in range(D.batch)],
            [D.jpvt(k).copy() for k in range(D.batch)])


def check_qr(t, Qm, Rm, H, al, A, what):
    """the existing bounds of the type: R by check_r, Q and R on A by check_qr"""
    if t == "f32":
        Q.check_r(Rm, H, al)
        Q.check_qr(Qm, Rm, A, "f32", what)
    else:
        ZQ.check_r(Rm, H, al)
        ZQ.check_qr(Qm, Rm, A, what)


# ---- the checks, written once ----------------------------------------------------------------------------------------
def check_pivots_and_factor(R, mats, Bs, scipy_qr=None):
    """case 1: jpvt is a permutation and the twin's (precondition GAP asserted on the twin; ComplexF64: scipy's too where it
    imports), |alpha_j| does not increase, the factor is finite, Q and R from the existing form_q / form_r pass the existing
    bounds on A[:, jpvt]"""
    t = R.t
    D = factored(R, mats, Bs)
    m, n = D.m, D.n
    QR = R.q_and_r(D)
    for k, A in enumerate(mats):
        jp, al = D.jpvt(k), D.alpha(k)
        assert sorted(jp.tolist()) == list(range(n)), f"matrix {k}: jpvt is no permutation: {jp}"
        _, _, want = twin_factor(t, A, check_gap=True)
        assert np.array_equal(jp, want), f"matrix {k}: jpvt {jp} != twin {want}"
        if scipy_qr is not None and t == "c64":
            assert np.array_equal(jp, scipy_qr(A, pivoting=True, mode="r")[1]), f"matrix {k}: jpvt != scipy"
        assert np.all(np.isfinite(D.mat(k))) and np.all(np.isfinite(al))
        aa = np.abs(al.astype(WIDE[t]))
        assert np.all(aa[1:] <= aa[:-1] * MONO[t]), f"matrix {k}: |alpha| increases: {al}"
        Qm, Rm = QR[k]
        check_qr(t, Qm, Rm, np.array(D.mat(k)), al, A[:, jp], f"{t} {m}x{n} matrix {k}")
    return D


def check_wave_bits(R, mats, Bs):
    """case 2, the wave tier: the pivoted factor has the bytes of dhqr_factor_batched_* on A[:, jpvt]; the pivoted factor of
    A[:, jpvt] has the identity permutation and the same bytes; the solve with rank r has the bytes of the type's unpivoted
    multi-column solve called with n = r (r = n, mixed ranks with 0, out-of-range ranks clamped); X is z scattered through
    jpvt with exact zeros elsewhere; matrix k has the bytes of its batch-of-one call; a column's bytes depend neither on nrhs
    nor on its place; a guarded layout gives the packed call's bytes with every sentinel intact"""
    t = R.t
    D = factored(R, mats, Bs)
    m, n, batch = D.m, D.n, D.batch
    Hs, als, jps = snapshot(D)
    perm = [np.asfortranarray(A[:, jp]) for A, jp in zip(mats, jps)]
    U = TBatch(t, perm, Bs)
    R.ok(R.factor_unpivoted(U))
    D2 = factored(R, perm, Bs)
    for k in range(batch):
        assert same_bytes(D.mat(k), U.mat(k)) and same_bytes(D.alpha(k), U.alpha(k)), f"matrix {k}: != unpivoted factor of A[:, jpvt]"
        assert np.array_equal(D2.jpvt(k), np.arange(n)), f"matrix {k}: A[:, jpvt] is pivoted again: {D2.jpvt(k)}"
        assert same_bytes(D2.mat(k), D.mat(k)) and same_bytes(D2.alpha(k), D.alpha(k))
    for ranks in ([n] * batch, [(n - 1 - k) % (n + 1) if k else 0 for k in range(batch)], [n + 5, -3] + [max(n // 2, 1)] * (batch - 2)):
        S = TBatch(t, mats, Bs).set_factor(Hs, als, jps, ranks)
        R.ok(R.solve(S))
        assert S.padding_intact()
        for k in range(batch):
            r = min(max(ranks[k], 0), n)
            if r == 0:
                assert same_bytes(S.bmat(k), Bs[k]) and not S.xmat(k).any(), f"matrix {k}: rank 0"
                assert not np.signbit(S.xmat(k).real).any() and not np.signbit(S.xmat(k).imag).any(), f"matrix {k}: rank 0: a -0 in X"
                continue
            V = TBatch(t, [mats[k]], [Bs[k]]).set_factor([Hs[k]], [als[k]], [jps[k]])
            R.ok(R.solve_unpivoted(V, n=r))
            assert same_bytes(S.bmat(k), V.bmat(0)), f"matrix {k}, rank {r}: dB != dhqr_solve_batched_nrhs_{t} with n = r"
            X = np.zeros((n, D.nrhs), dtype=NP[t])
            X[jps[k][:r]] = V.bmat(0)[:r]
            assert same_bytes(S.xmat(k), X), f"matrix {k}, rank {r}: X is not z scattered through jpvt with exact zeros elsewhere"
    # the batch of one, and a single column: the bytes do not depend on the batch, nrhs or the column's place
    S = TBatch(t, mats, Bs).set_factor(Hs, als, jps, [max(n - 1, 1)] * batch)
    R.ok(R.solve(S))
    for k in range(batch):
        O = factored(R, [mats[k]], [np.asfortranarray(Bs[k][:, -1:])])
        assert same_bytes(O.mat(0), D.mat(k)) and same_bytes(O.alpha(0), D.alpha(k)) and np.array_equal(O.jpvt(0), D.jpvt(k)), k
        O.ranks()[...] = max(n - 1, 1)
        R.ok(R.solve(O))
        assert same_bytes(O.bmat(0)[:, 0], S.bmat(k)[:, -1]) and same_bytes(O.xmat(0)[:, 0], S.xmat(k)[:, -1]), k
    # guarded layout: lda = m + 1, padded strides, bases one element in
    G = factored(R, mats, Bs, pad_ld=1, pad=5, pad_ldb=1, pad_ldx=1, off=1)
    G.ranks()[...] = max(n - 1, 1)
    R.ok(R.solve(G))
    assert G.padding_intact()
    for k in range(batch):
        assert same_bytes(G.mat(k), D.mat(k)) and same_bytes(G.alpha(k), D.alpha(k)) and np.array_equal(G.jpvt(k), D.jpvt(k)), k
        assert same_bytes(G.bmat(k), S.bmat(k)) and same_bytes(G.xmat(k), S.xmat(k)), k


def check_rank(R, mats, Bs, r0, rcond=None):
    """case 3: prints the kept and dropped ratios, then rank == the twin's rank on the result's alpha == r0 for every matrix;
    returns the factored batch with the ranks in it"""
    t = R.t
    rcond = RCOND[t] if rcond is None else rcond
    D = factored(R, mats, Bs)
    R.ok(R.rank(D, rcond))
    assert D.padding_intact() and D.untouched("X")
    for k in range(D.batch):
        al = np.abs(D.alpha(k).astype(WIDE[t]))
        print(f"{t} {D.m}x{D.n} r0 {r0} matrix {k}: |alpha/alpha_0| kept >= {(al[:r0] / al[0]).min():.1e}, "
              f"dropped <= {(al[r0:] / al[0]).max() if r0 < D.n else 0.0:.1e}")
        assert D.ranks()[k] == twin_rank(t, D.alpha(k), rcond, D.m)
        assert twin_rank(t, twin_factor(t, mats[k])[1], rcond, D.m) == r0, f"matrix {k}: the twin's rank is not {r0}"
    assert D.ranks().tolist() == [r0] * D.batch, D.ranks()
    return D


def stat(A, x, b):
    """the reference's statistic ||A^H (A x - b)|| (test/runtests.jl:51,62)"""
    return float(np.linalg.norm(np.conj(A.T) @ (A @ x - b)))


def solution_figures(t, A, b, x, tail):
    """(statistic / bound, tail figure / tolerance, a line to print) of one column by the rule of this module's docstring"""
    Aw, bw, xw = (np.asarray(v, dtype=WIDE[t]) for v in (A, b, x))
    xn = np.linalg.lstsq(Aw, bw, rcond=RCOND[t])[0]
    got, ref = stat(Aw, xw, bw), stat(Aw, xn, bw)
    nb = float(np.linalg.norm(bw))
    floor = 1e-13 * EPSRATIO[t] * np.linalg.norm(Aw, 2) ** 2 * nb
    res, tl = float(np.linalg.norm(Aw @ xw - bw)), float(np.linalg.norm(np.asarray(tail, dtype=WIDE[t])))
    ttol = 1e-11 * EPSRATIO[t] * nb
    line = (f"||A^H(Ax-b)|| = {got:.2e} (numpy {ref:.2e}, floor {floor:.2e}); | ||tail|| - ||Ax-b|| | = {abs(tl - res):.2e} (tol {ttol:.2e})")
    return got / (8 * ref + floor), abs(tl - res) / ttol, line


def check_solution(t, A, b, x, tail, what):
    s, tf, line = solution_figures(t, A, b, x, tail)
    print(f"{what}: {line}")
    assert s <= 1.0, f"{what}: the statistic is {s:.2f} x its bound"
    assert tf <= 1.0, f"{what}: the tail rows miss the residual by {tf:.2f} x the tolerance"


def check_solve(R, mats, Bs, r0, rcond=None):
    """cases 3 and 4 on one set: factor, rank (== r0), device solve, exact zeros at the dropped columns, every column by
    check_solution; then the host form dhqr_lstsq_batched_*: the same X and ranks, hA and hB untouched"""
    t = R.t
    D = check_rank(R, mats, Bs, r0, rcond)
    R.ok(R.solve(D))
    assert D.padding_intact()
    for k in range(D.batch):
        jp = D.jpvt(k)
        for q in range(D.nrhs):
            x = D.xmat(k)[:, q]
            assert not x[jp[r0:]].any(), f"matrix {k} column {q}: rows of dropped columns are not exact zeros"
            check_solution(t, mats[k], Bs[k][:, q], x, D.bmat(k)[r0:, q], f"{t} {D.m}x{D.n} rank {r0} matrix {k} column {q}")
    Hst = TBatch(t, mats, Bs)
    R.ok(R.lstsq(Hst, RCOND[t] if rcond is None else rcond))
    assert Hst.padding_intact() and Hst.untouched("al", "jp")
    assert Hst.ranks().tolist() == [r0] * D.batch
    for k in range(D.batch):
        assert same_bytes(Hst.mat(k), mats[k]) and same_bytes(Hst.bmat(k), Bs[k]), f"matrix {k}: the host form changed A or B"
        assert same_bytes(Hst.xmat(k), D.xmat(k)), f"matrix {k}: the host form's X != the device form's"


def check_full_rank(R, mats, Bs):
    """case 4: rcond < 0 (max(m, n) eps of the type) gives rank n on a full-rank set, then case 3's solution check"""
    n = mats[0].shape[1]
    D = check_rank(R, mats, Bs, n, rcond=-1.0)
    assert D.ranks().tolist() == [n] * D.batch
    check_solve(R, mats, Bs, n)


def check_degenerate(R, orc):
    """case 5 at (16, 8): a zero matrix; a zero column in matrix 2 of 5; a zero first row"""
    t, dt = R.t, NP[R.t]
    m, n = 16, 8
    mats, Bs = inputs(orc, t, m, n, batch=5)
    clean = factored(R, mats, Bs)
    # a zero matrix: rank 0, alpha = 0, v_c = sqrt(2) e_c, identity jpvt, the solve leaves B alone and X = 0, Q orthonormal
    Z = factored(R, [np.zeros((m, n), dtype=dt, order="F")] * 2, Bs[:2])
    R.ok(R.rank(Z, RCOND[t]))
    R.ok(R.solve(Z))
    want = np.zeros((m, n), dtype=dt)
    want[np.arange(n), np.arange(n)] = dt(np.sqrt(2.0))
    for k in range(2):
        assert same_bytes(Z.mat(k), want) and not Z.alpha(k).any() and np.array_equal(Z.jpvt(k), np.arange(n))
        assert Z.ranks()[k] == 0 and same_bytes(Z.bmat(k), Bs[k]) and not Z.xmat(k).any()
    Qz, Rz = R.q_and_r(Z)[0]
    Qw = Qz.astype(WIDE[t])
    assert not Rz.any() and np.abs(np.conj(Qw.T) @ Qw - np.eye(n)).max() < (F.tol_factor(n) if t == "f32" else 1e-12)
    # a zero column in matrix 2 of 5
    dirty = [A.copy(order="F") for A in mats]
    dirty[2][:, 3] = 0.0
    Dd = factored(R, dirty, Bs)
    R.ok(R.rank(Dd, RCOND[t]))
    assert Dd.ranks().tolist() == [n, n, n - 1, n, n]
    assert np.all(np.isfinite(Dd.mat(2))) and np.all(np.isfinite(Dd.alpha(2))) and Dd.jpvt(2)[-1] == 3 and Dd.alpha(2)[-1] == 0.0
    assert sorted(Dd.jpvt(2).tolist()) == list(range(n))
    Qm, Rm = R.q_and_r(Dd)[2]
    check_qr(t, Qm, Rm, np.array(Dd.mat(2)), Dd.alpha(2), dirty[2][:, Dd.jpvt(2)], f"{t} zero column")
    for k in (0, 1, 3, 4):
        assert same_bytes(Dd.mat(k), clean.mat(k)) and same_bytes(Dd.alpha(k), clean.alpha(k)) and np.array_equal(Dd.jpvt(k), clean.jpvt(k)), k
    R.ok(R.solve(Dd))
    for q in range(Dd.nrhs):
        assert Dd.xmat(2)[3, q] == 0.0
        check_solution(t, dirty[2], Bs[2][:, q], Dd.xmat(2)[:, q], Dd.bmat(2)[n - 1:, q], f"{t} zero column, column {q}")
    # a zero first row: every pivot entry of step 0 is exactly 0 -- alphafactor(0) = -1 keeps the factor valid
    row = [A.copy(order="F") for A in mats]
    for A in row:
        A[0, :] = 0.0
    Dr = factored(R, row, Bs)
    R.ok(R.rank(Dr, -1.0))
    assert Dr.ranks().tolist() == [n] * 5
    for k, (Qm, Rm) in enumerate(R.q_and_r(Dr)):
        assert np.all(np.isfinite(Dr.mat(k))) and np.all(np.isfinite(Dr.alpha(k)))
        if t == "f32":
            assert Dr.alpha(k)[0] < 0
        else:  # (zalphafactor(0) = -1 + 0i)
            assert Dr.alpha(k)[0].real < 0 and Dr.alpha(k)[0].imag == 0
        check_qr(t, Qm, Rm, np.array(Dr.mat(k)), Dr.alpha(k), row[k][:, Dr.jpvt(k)], f"{t} zero first row, matrix {k}")


def check_arguments(R, orc):
    """case 6: the DHQR_EINVAL and empty-call tables of pivoted_helpers.check_arguments on the five symbols of the type: every
    DHQR_EINVAL case writes nothing; the empty cases are no-ops"""
    t = R.t
    m, n = 16, 8
    mats, Bs = inputs(orc, t, m, n)
    Fd = factored(R, mats, Bs)
    R.ok(R.rank(Fd, RCOND[t]))
    Hs, als, jps = snapshot(Fd)

    def fresh(with_factor):
        D = TBatch(t, mats, Bs)
        return D.set_factor(Hs, als, jps, Fd.ranks().copy()) if with_factor else D

    def same_as(D, E):
        return all(same_bytes(getattr(D, nm), getattr(E, nm)) for nm in D.BUFS)

    bad = [("factor", False, dict(null=("jp",))), ("factor", False, dict(sjp=n - 1)), ("factor", False, dict(null=("al",))),
           ("factor", False, dict(null=("A",))), ("factor", False, dict(lda=m - 1)), ("factor", False, dict(batch=-1)),
           ("factor", False, dict(m=n - 1)), ("factor", False, dict(sA=Fd.lda * (n - 1) + m - 1)), ("factor", False, dict(sal=n - 1)),
           ("qr_host", False, dict(null=("jp",))), ("qr_host", False, dict(sjp=n - 1)),
           ("solve", True, dict(null=("jp",))), ("solve", True, dict(null=("rk",))), ("solve", True, dict(null=("X",))),
           ("solve", True, dict(null=("B",))), ("solve", True, dict(sjp=n - 1)), ("solve", True, dict(ldx=n - 1)),
           ("solve", True, dict(sX=Fd.ldx * (Fd.nrhs - 1) + n - 1)), ("solve", True, dict(ldb=m - 1)), ("solve", True, dict(nrhs=-1)),
           ("solve", True, dict(batch=-1)),
           ("lstsq", False, dict(null=("rk",))), ("lstsq", False, dict(null=("X",))), ("lstsq", False, dict(null=("B",))),
           ("lstsq", False, dict(ldx=n - 1)), ("lstsq", False, dict(lda=m - 1)),
           ("rank", True, dict(null=("rk",))), ("rank", True, dict(null=("al",))), ("rank", True, dict(sal=n - 1)),
           ("rank", True, dict(batch=-1)), ("rank", True, dict(m=n - 1))]
    empty = [("factor", False, dict(batch=0)), ("factor", False, dict(n=0)), ("qr_host", False, dict(batch=0)),
             ("solve", True, dict(batch=0)), ("solve", True, dict(n=0)), ("solve", True, dict(nrhs=0)),
             ("lstsq", False, dict(batch=0)), ("lstsq", False, dict(nrhs=0)), ("lstsq", False, dict(n=0)),
             ("rank", True, dict(batch=0)), ("rank", True, dict(n=0))]
    for cases, want in ((bad, EINVAL), (empty, 0)):
        for name, with_factor, kw in cases:
            D, E = fresh(with_factor), fresh(with_factor)
            extra = (RCOND[t],) if name in ("rank", "lstsq") else ()
            rc = getattr(R, name)(D, *extra, **kw)
            assert rc == want, f"{t} {name} {kw}: rc {rc}, {R.L.dhqr_last_error()}"
            assert same_as(D, E), f"{t} {name} {kw}: something was written"


def check_profile_counts(R, orc, m, n, Stats=None):
    """a factor counts ONE n_rank1 group, a solve ONE n_solve group per launch, whatever nrhs and batch; rank is not counted.
    Stats: the dhqr_stats structure class the library's prototypes were declared with (default: the emulated loader's L.Stats)"""
    L, h, t = R.L, R.h, R.t
    mats, Bs = inputs(orc, t, m, n)
    D = TBatch(t, mats, Bs)
    st = (Stats or L.Stats)()
    assert L.dhqr_set_profiling(h, 1) == 0 and L.dhqr_reset_stats(h) == 0
    R.ok(R.factor(D))
    R.ok(R.rank(D, RCOND[t]))
    assert L.dhqr_get_stats(h, ctypes.byref(st)) == 0 and (st.n_rank1, st.n_solve) == (1, 0), (st.n_rank1, st.n_solve)
    R.ok(R.solve(D))
    assert L.dhqr_get_stats(h, ctypes.byref(st)) == 0 and (st.n_rank1, st.n_solve) == (1, 1), (st.n_rank1, st.n_solve)
    assert L.dhqr_set_profiling(h, 0) == 0


def twin_report(orc):
    """the CPU trial of this module's docstring: the twin alone on every set the tests use -- smallest gap, kept and dropped
    ratios, and the twin's own solution through solution_figures"""
    for t in TYPES:
        gaps, kept, dropped, ws, wt = [], [], [], (0.0, ""), (0.0, "")
        sets = [(m, n, n, inputs(orc, t, m, n)) for m, n in WAVE_SHAPES + GENERAL_SHAPES]
        sets += [(m, n, r0, low_rank_inputs(t, m, n, r0)) for m, n, r0 in LOW_RANK]
        for m, n, r0, (mats, Bs) in sets:
            for k, A in enumerate(mats):
                g = []
                H, al, jp = twin_factor(t, A, check_gap=r0 == n, gaps=g)
                gaps += g[:max(r0 - 1, 0)]  # (behind the rank the remaining norms are rounding noise: no pivot is compared there)
                a = np.abs(al.astype(WIDE[t]))
                if r0 < n:
                    kept.append((a[:r0] / a[0]).min())
                    dropped.append((a[r0:] / a[0]).max())
                assert twin_rank(t, al, RCOND[t], m) == r0, (t, m, n, r0, k)
                for q in range(Bs[k].shape[1]):
                    b, x = twin_solve(t, H, al, jp, r0, Bs[k][:, q])
                    s, tf, _ = solution_figures(t, A, Bs[k][:, q], x, b[r0:])
                    ws, wt = max(ws, (s, f"{m}x{n} rank {r0}")), max(wt, (tf, f"{m}x{n} rank {r0}"))
        print(f"{t}: smallest gap {min(gaps):.1e} (bound {GAP[t]:.0e}); kept >= {min(kept):.1e}, dropped <= {max(dropped):.1e}; "
              f"twin statistic / bound <= {ws[0]:.1e} ({ws[1]}), tail figure / tolerance <= {wt[0]:.1e} ({wt[1]})")


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import dhqr_oracle
    twin_report(dhqr_oracle)
