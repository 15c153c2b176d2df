"""Test-only helpers of the tests of the column-pivoted batched QR and the rank-revealing least squares
(test_emulated_pivoted.py, test_gpu_pivoted.py): a numpy twin of the rule of include/dhqr.h (norms afresh, first maximum,
alphafactor(0) = -1, the zero tail, the rank rule, the truncated solve), the shapes and inputs both files share, a strided
batch with jpvt and rank in sentinel-filled buffers driven through the C ABI -- on the emulated library, where a numpy
buffer IS device memory, or on the GPU, where every buffer is copied to the device, guards and all, and back -- and the
checks themselves, written once for both files.  The product never imports this file."""
import ctypes

import numpy as np

import applyq_helpers as Q
import nrhs_helpers as N
from nrhs_helpers import NBatch, P, SENT, _flat, ptr, same_bytes

WAVE_SHAPES = [(5, 3), (16, 8), (40, 17), (64, 32), (32, 32)]
GENERAL_SHAPES = [(66, 33), (130, 20), (300, 40)]
LOW_RANK = [(16, 8, 3), (40, 17, 9), (64, 32, 1), (64, 32, 31), (66, 33, 10), (130, 20, 7)]  # (m, n, r0)
BATCH, NRHS = 4, 3
SEED = N.SEED
RCOND = 1e-10
ISENT = int(SENT)  # what the sentinel becomes in an int32 buffer
EINVAL = N.EINVAL
GAP = 1e-10        # the precondition of the pivot comparison: the two largest remaining norms differ by more, relatively


# ---- inputs ----------------------------------------------------------------------------------------------------------
def inputs(orc, m, n, nrhs=NRHS, batch=BATCH, seed=SEED):
    """the project's generator (N.inputs) with column c scaled by 1 + 0.25 c: full rank, well separated column norms"""
    mats, Bs = N.inputs(orc, m, n, nrhs, batch, seed)
    scale = 1.0 + 0.25 * np.arange(n)
    return [np.asfortranarray(A * scale) for A in mats], Bs


def low_rank_inputs(m, n, r0, nrhs=NRHS, batch=BATCH, seed=SEED):
    """A_k = X_k Y_k with X (m x r0) and Y (r0 x n) uniform: rank r0 up to rounding; B uniform"""
    rng = np.random.default_rng(seed + 7 * m + n + r0)
    mats = [np.asfortranarray(rng.uniform(size=(m, r0)) @ rng.uniform(size=(r0, n))) for _ in range(batch)]
    Bs = [rng.uniform(-1, 1, size=(m, nrhs)) for _ in range(batch)]
    return mats, Bs


# ---- the numpy twin --------------------------------------------------------------------------------------------------
def twin_factor(A, check_gap=False):
    """(H, alpha, jpvt) of the pivoted factorisation in plain double.  check_gap: assert the precondition GAP at every step"""
    a = np.array(A, dtype=np.float64, order="F")
    m, n = a.shape
    alpha, jpvt = np.zeros(n), np.arange(n, dtype=np.int32)
    for j in range(n):
        nrm = (a[j:, j:] ** 2).sum(axis=0)  # afresh from the working matrix
        p = j + int(np.argmax(nrm))         # the first maximum
        if nrm[p - j] == 0.0:               # the rest is zero: alpha_c = 0, v_c = sqrt(2) e_c
            for c in range(j, n):
                a[c:, c] = 0.0
                a[c, c] = np.sqrt(2.0)
            break
        if check_gap and n - j > 1:
            s = np.sort(nrm)
            assert (s[-1] - s[-2]) > GAP * s[-1], f"step {j}: the two largest norms are closer than {GAP} relative"
        a[:, [j, p]] = a[:, [p, j]]
        jpvt[[j, p]] = jpvt[[p, j]]
        s = np.sqrt(float(a[j:, j] @ a[j:, j]))
        h = a[j, j]
        alpha[j] = (-1.0 if h >= 0 else 1.0) * s  # alphafactor(0) = -1
        f = 1.0 / np.sqrt(s * (s + abs(h)))
        a[j, j] = h - alpha[j]
        a[j:, j] *= f
        if j + 1 < n:
            a[j:, j + 1:] -= np.outer(a[j:, j], a[j:, j] @ a[j:, j + 1:])
    return a, alpha, jpvt


def twin_rank(alpha, rcond, m):
    n = len(alpha)
    rc = rcond if rcond >= 0 else max(m, n) * 2.0 ** -52
    r = 0
    while r < n and abs(alpha[r]) > rc * abs(alpha[0]):
        r += 1
    return r


def twin_solve(H, alpha, jpvt, r, b):
    """(b <- [z; tail], x) of the truncated solve in plain double"""
    n = H.shape[1]
    b = np.array(b, dtype=np.float64)
    for j in range(r):
        b[j:] -= H[j:, j] * (H[j:, j] @ b[j:])
    for j in range(r - 1, -1, -1):
        b[j] /= alpha[j]
        b[:j] -= H[:j, j] * b[j]
    x = np.zeros(n)
    x[jpvt[:r]] = b[:r]
    return b, x


# ---- a strided batch with jpvt and rank ------------------------------------------------------------------------------
class PBatch(NBatch):
    """NBatch (Float64) + jpvt_k (n int32) at jp[k*sjp:] and rank[k] at rk[k], sentinel-filled like the rest"""
    BUFS = ("A", "al", "B", "X", "jp", "rk")

    def __init__(self, mats, Bs, pad_jp=3, **layout):
        super().__init__(mats, Bs, "f64", **layout)
        off = layout.get("off", 0)
        self.off = off
        self.sjp = self.n + pad_jp
        self.jp, self.rk = _flat(self.batch * self.sjp + 7, np.int32, off), _flat(self.batch + 7, np.int32, off)
        self.maskjp, self.maskrk = np.zeros(self.jp.size, bool), np.zeros(self.rk.size, bool)
        self.maskrk[:self.batch] = True
        for k in range(self.batch):
            self.maskjp[k * self.sjp: k * self.sjp + self.n] = True

    def jpvt(self, k):
        return self.jp[k * self.sjp: k * self.sjp + self.n]

    def ranks(self):
        return self.rk[:self.batch]

    def padding_intact(self):
        return (super().padding_intact() and bool(np.all(self.jp[~self.maskjp] == ISENT)) and bool(np.all(self.rk[~self.maskrk] == ISENT)))

    def untouched(self, *names):
        """do the named buffers still hold nothing but what the constructor put there (the argument tests: sentinels and
        inputs, compared with a fresh copy by the caller) -- here: all sentinel"""
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
    """calls the C ABI on the buffers of a batch.  torch = None: the emulated library, numpy memory is device memory.  Else:
    every buffer goes to the GPU (at the same offset from an aligned base), the call runs there, every buffer comes back."""

    def __init__(self, L, h, torch=None):
        self.L, self.h, self.torch = L, h, torch

    def sync(self):
        assert self.L.dhqr_synchronize(self.h) == 0, self.L.dhqr_last_error()

    def call(self, name, D, args, host=False, null=()):
        """fn(h, *args(p)) with p(buffer name) -> pointer (a name in `null`: a null pointer); returns rc, synchronised"""
        fn = getattr(self.L, name)
        if self.torch is None or host:
            rc = fn(self.h, *args(lambda nm: P(None) if nm in null else ptr(getattr(D, nm))))
            self.sync()
            return rc
        torch, dev = self.torch, {}
        for nm in D.BUFS:
            buf = getattr(D, nm)
            t = torch.empty(buf.size + D.off, dtype=torch.int32 if buf.dtype == np.int32 else torch.float64, device="cuda:0")[D.off:]
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
        return self.call("dhqr_factor_batched_pivoted_f64", D, lambda p: (p("A"), a["m"], a["n"], a["lda"], a["sA"], p("al"), a["sal"],
                                                                         p("jp"), a["sjp"], a["batch"]), null=null)

    def factor_unpivoted(self, D):
        return self.call("dhqr_factor_batched_f64", D, lambda p: (p("A"), D.m, D.n, D.lda, D.sA, p("al"), D.sal, D.batch, 0))

    def rank(self, D, rcond, null=(), **kw):
        a = dict(m=D.m, n=D.n, sal=D.sal, batch=D.batch)
        a.update(kw)
        return self.call("dhqr_rank_batched_f64", D, lambda p: (p("al"), a["m"], a["n"], a["sal"], rcond, p("rk"), a["batch"]), null=null)

    def solve(self, D, null=(), **kw):
        a = dict(m=D.m, n=D.n, lda=D.lda, sA=D.sA, sal=D.sal, sjp=D.sjp, nrhs=D.nrhs, ldb=D.ldb, sB=D.sB, ldx=D.ldx, sX=D.sX, batch=D.batch)
        a.update(kw)
        return self.call("dhqr_solve_batched_pivoted_f64", D, lambda p: (
            p("A"), a["m"], a["n"], a["lda"], a["sA"], p("al"), a["sal"], p("jp"), a["sjp"], p("rk"), p("B"), a["nrhs"], a["ldb"], a["sB"],
            p("X"), a["ldx"], a["sX"], a["batch"]), null=null)

    def solve_unpivoted(self, D, n=None):
        """dhqr_solve_batched_nrhs_f64 with the first n columns of the factor (default: all)"""
        n = D.n if n is None else n
        return self.call("dhqr_solve_batched_nrhs_f64", D, lambda p: (p("A"), D.m, n, D.lda, D.sA, p("al"), D.sal, p("B"), D.nrhs, D.ldb,
                                                                     D.sB, D.batch))

    def qr_host(self, D, null=(), **kw):
        a = dict(m=D.m, n=D.n, lda=D.lda, sA=D.sA, sal=D.sal, sjp=D.sjp, batch=D.batch)
        a.update(kw)
        return self.call("dhqr_qr_batched_pivoted_f64", D, lambda p: (p("A"), a["m"], a["n"], a["lda"], a["sA"], p("al"), a["sal"], p("jp"),
                                                                     a["sjp"], a["batch"]), host=True, null=null)

    def lstsq(self, D, rcond, null=(), **kw):
        a = dict(m=D.m, n=D.n, lda=D.lda, sA=D.sA, nrhs=D.nrhs, ldb=D.ldb, sB=D.sB, ldx=D.ldx, sX=D.sX, batch=D.batch)
        a.update(kw)
        return self.call("dhqr_lstsq_batched_f64", D, lambda p: (p("A"), a["m"], a["n"], a["lda"], a["sA"], p("B"), a["nrhs"], a["ldb"],
                                                                a["sB"], rcond, p("X"), a["ldx"], a["sX"], p("rk"), a["batch"]),
                         host=True, null=null)

    def q_and_r(self, D):
        """(Q_k, R_k) of the factors in D by the EXISTING dhqr_form_q_batched_f64 / dhqr_form_r_batched_f64"""
        out = []
        for k in range(D.batch):
            H, al = np.array(D.mat(k), order="F"), D.alpha(k).copy()
            Qm, Rm = np.full((D.m, D.n), SENT, order="F"), np.full((D.n, D.n), SENT, order="F")
            if self.torch is None:
                self.ok(self.L.dhqr_form_q_batched_f64(self.h, ptr(H), D.m, D.n, D.m, D.m * D.n, ptr(Qm), D.m, D.m * D.n, 1))
                self.ok(self.L.dhqr_form_r_batched_f64(self.h, ptr(H), D.m, D.n, D.m, D.m * D.n, ptr(al), D.n, ptr(Rm), D.n, D.n * D.n, 1))
                self.sync()
            else:
                t = self.torch
                dH, dal = t.from_numpy(H.T.copy()).cuda(), t.from_numpy(al).cuda()  # (n, m) row-major = (m, n) column-major
                dQ, dR = t.empty((D.n, D.m), dtype=t.float64, device="cuda:0"), t.empty((D.n, D.n), dtype=t.float64, device="cuda:0")
                t.cuda.synchronize()
                self.ok(self.L.dhqr_form_q_batched_f64(self.h, P(dH.data_ptr()), D.m, D.n, D.m, D.m * D.n, P(dQ.data_ptr()), D.m, D.m * D.n, 1))
                self.ok(self.L.dhqr_form_r_batched_f64(self.h, P(dH.data_ptr()), D.m, D.n, D.m, D.m * D.n, P(dal.data_ptr()), D.n,
                                                       P(dR.data_ptr()), D.n, D.n * D.n, 1))
                self.sync()
                Qm, Rm = dQ.cpu().numpy().T, dR.cpu().numpy().T
            out.append((Qm, Rm))
        return out


def factored(R, mats, Bs, **layout):
    """a PBatch holding the pivoted factors of `mats` (device form), checked for its guards"""
    D = PBatch(mats, Bs, **layout)
    R.ok(R.factor(D))
    assert D.padding_intact() and D.untouched("X", "rk")
    return D


def snapshot(D):
    """(H_k, alpha_k, jpvt_k) copies"""
    return ([np.array(D.mat(k), order="F") for k in range(D.batch)], [D.alpha(k).copy() for k in range(D.batch)],
            [D.jpvt(k).copy() for k in range(D.batch)])


# ---- the checks, written once ----------------------------------------------------------------------------------------
def check_pivots_and_factor(R, mats, Bs, scipy_qr=None):
    """cases 1 and 2: jpvt is a permutation and the twin's (precondition GAP asserted on the twin), |alpha_j| does not
    increase (within 1 + 1e-12), Q and R from the existing form_q / form_r pass check_qr's Float64 bounds on A[:, jpvt]"""
    D = factored(R, mats, Bs)
    m, n = D.m, D.n
    QR = R.q_and_r(D)
    for k, A in enumerate(mats):
        jp, al = D.jpvt(k), D.alpha(k)
        assert sorted(jp.tolist()) == list(range(n)), f"matrix {k}: jpvt is no permutation: {jp}"
        _, _, want = twin_factor(A, check_gap=True)
        assert np.array_equal(jp, want), f"matrix {k}: jpvt {jp} != twin {want}"
        if scipy_qr is not None:
            assert np.array_equal(jp, scipy_qr(A, pivoting=True, mode="r")[1]), f"matrix {k}: jpvt != scipy"
        assert np.all(np.isfinite(D.mat(k))) and np.all(np.isfinite(al))
        assert np.all(np.abs(al[1:]) <= np.abs(al[:-1]) * (1 + 1e-12)), f"matrix {k}: |alpha| increases: {al}"
        Qm, Rm = QR[k]
        Q.check_r(Rm, np.array(D.mat(k)), al)
        Q.check_qr(Qm, Rm, A[:, jp], "f64", f"{m}x{n} matrix {k}")
    return D


def check_wave_bits(R, mats, Bs):
    """case 3, the wave tier: the pivoted factor has the bytes of dhqr_factor_batched_f64 on A[:, jpvt]; the pivoted factor of
    A[:, jpvt] has the identity permutation and the same bytes; the solve with r = n has the bytes of the unpivoted solve,
    with r < n those of that solve called with n = r; matrix k has the bytes of its batch-of-one call; a guarded layout
    (lda = m + 1, padded strides, bases one element in) gives the packed call's bytes with every sentinel intact"""
    D = factored(R, mats, Bs)
    m, n, batch = D.m, D.n, D.batch
    Hs, als, jps = snapshot(D)
    perm = [np.asfortranarray(A[:, jp]) for A, jp in zip(mats, jps)]
    U = PBatch(perm, Bs)
    R.ok(R.factor_unpivoted(U))
    D2 = factored(R, perm, Bs)
    for k in range(batch):
        assert same_bytes(D.mat(k), U.mat(k)) and same_bytes(D.alpha(k), U.alpha(k)), f"matrix {k}: != unpivoted factor of A[:, jpvt]"
        assert np.array_equal(D2.jpvt(k), np.arange(n)), f"matrix {k}: A[:, jpvt] is pivoted again: {D2.jpvt(k)}"
        assert same_bytes(D2.mat(k), D.mat(k)) and same_bytes(D2.alpha(k), D.alpha(k))
    # the solve: r = n, and ranks below n (0 included) matrix by matrix
    for ranks in ([n] * batch, [(n - 1 - k) % (n + 1) if k else 0 for k in range(batch)], [n + 5, -3] + [max(n // 2, 1)] * (batch - 2)):
        S = PBatch(mats, Bs).set_factor(Hs, als, jps, ranks)
        R.ok(R.solve(S))
        assert S.padding_intact()
        for k in range(batch):
            r = min(max(ranks[k], 0), n)
            if r == 0:
                assert same_bytes(S.bmat(k), Bs[k]) and not S.xmat(k).any() and not np.signbit(S.xmat(k)).any(), f"matrix {k}: rank 0"
                continue
            V = PBatch([mats[k]], [Bs[k]]).set_factor([Hs[k]], [als[k]], [jps[k]])
            R.ok(R.solve_unpivoted(V, n=r))
            assert same_bytes(S.bmat(k), V.bmat(0)), f"matrix {k}, rank {r}: dB != dhqr_solve_batched_nrhs_f64 with n = r"
            X = np.zeros((n, D.nrhs))
            X[jps[k][:r]] = V.bmat(0)[:r]
            assert same_bytes(S.xmat(k), X), f"matrix {k}, rank {r}: X is not z scattered through jpvt with exact zeros elsewhere"
    # the batch of one, and a single column: the bytes do not depend on the batch, nrhs or the column's place
    S = PBatch(mats, Bs).set_factor(Hs, als, jps, [max(n - 1, 1)] * batch)
    R.ok(R.solve(S))
    for k in range(batch):
        O = factored(R, [mats[k]], [Bs[k][:, -1:]])
        assert same_bytes(O.mat(0), D.mat(k)) and same_bytes(O.alpha(0), D.alpha(k)) and np.array_equal(O.jpvt(0), D.jpvt(k)), k
        O.ranks()[...] = max(n - 1, 1)
        R.ok(R.solve(O))
        assert same_bytes(O.bmat(0)[:, 0], S.bmat(k)[:, -1]) and same_bytes(O.xmat(0)[:, 0], S.xmat(k)[:, -1]), k
    # guarded layout
    G = factored(R, mats, Bs, pad_ld=1, pad=5, pad_ldb=1, pad_ldx=1, off=1)
    G.ranks()[...] = max(n - 1, 1)
    R.ok(R.solve(G))
    assert G.padding_intact()
    for k in range(batch):
        assert same_bytes(G.mat(k), D.mat(k)) and same_bytes(G.alpha(k), D.alpha(k)) and np.array_equal(G.jpvt(k), D.jpvt(k)), k
        assert same_bytes(G.bmat(k), S.bmat(k)) and same_bytes(G.xmat(k), S.xmat(k)), k


def check_rank(R, mats, Bs, r0, rcond=RCOND):
    """case 4: rank == r0 for every matrix; returns the factored batch with the ranks in it"""
    D = factored(R, mats, Bs)
    R.ok(R.rank(D, rcond))
    assert D.padding_intact() and D.untouched("X")
    for k in range(D.batch):
        al = D.alpha(k)
        print(f"{D.m}x{D.n} r0 {r0} matrix {k}: |alpha/alpha_0| kept >= {np.abs(al[:r0] / al[0]).min():.1e}, "
              f"dropped <= {np.abs(al[r0:] / al[0]).max() if r0 < D.n else 0.0:.1e}")
        assert D.ranks()[k] == twin_rank(al, rcond, D.m)
    assert D.ranks().tolist() == [r0] * D.batch, D.ranks()
    return D


def stat(A, x, b):
    """the reference's statistic ||A'(A x - b)|| (test/runtests.jl:51,62)"""
    return float(np.linalg.norm(A.T @ (A @ x - b)))


def check_solution(A, b, x, tail, what):
    """case 5 for one column: at most 8 x numpy.linalg.lstsq's statistic + 1e-13 ||A||^2 ||b||; the norm of the tail rows is
    the residual within 1e-11 ||b||"""
    xn = np.linalg.lstsq(A, b, rcond=RCOND)[0]
    got, ref = stat(A, x, b), stat(A, xn, b)
    floor = 1e-13 * np.linalg.norm(A, 2) ** 2 * np.linalg.norm(b)
    res, tl = float(np.linalg.norm(A @ x - b)), float(np.linalg.norm(tail))
    print(f"{what}: ||A'(Ax-b)|| = {got:.2e} (numpy {ref:.2e}, floor {floor:.2e}); | ||tail|| - ||Ax-b|| | / ||b|| = "
          f"{abs(tl - res) / np.linalg.norm(b):.2e} (tol 1e-11)")
    assert got <= 8 * ref + floor
    assert abs(tl - res) <= 1e-11 * np.linalg.norm(b)


def check_solve(R, mats, Bs, r0):
    """case 5 on one set: factor, rank (== r0), device solve; then the host form dhqr_lstsq_batched_f64: the same X and
    ranks, hA and hB untouched"""
    D = check_rank(R, mats, Bs, r0)
    R.ok(R.solve(D))
    assert D.padding_intact()
    for k in range(D.batch):
        jp = D.jpvt(k)
        for q in range(D.nrhs):
            x = D.xmat(k)[:, q]
            assert not x[jp[r0:]].any(), f"matrix {k} column {q}: rows of dropped columns are not exact zeros"
            check_solution(mats[k], Bs[k][:, q], x, D.bmat(k)[r0:, q], f"{D.m}x{D.n} rank {r0} matrix {k} column {q}")
    Hst = PBatch(mats, Bs)
    R.ok(R.lstsq(Hst, RCOND))
    assert Hst.padding_intact() and Hst.untouched("al", "jp")
    assert Hst.ranks().tolist() == [r0] * D.batch
    for k in range(D.batch):
        assert same_bytes(Hst.mat(k), mats[k]) and same_bytes(Hst.bmat(k), Bs[k]), f"matrix {k}: the host form changed A or B"
        assert same_bytes(Hst.xmat(k), D.xmat(k)), f"matrix {k}: the host form's X != the device form's"


def check_degenerate(R, orc):
    """case 4's exact zeros at (16, 8): a zero matrix; a zero column in matrix 2 of 5; a zero first row"""
    m, n = 16, 8
    mats, Bs = inputs(orc, m, n, batch=5)
    clean = factored(R, mats, Bs)
    # a zero matrix: rank 0, alpha = 0, v_c = sqrt(2) e_c, the solve leaves B alone and X = 0
    Z = factored(R, [np.zeros((m, n), order="F")] * 2, Bs[:2])
    R.ok(R.rank(Z, RCOND))
    R.ok(R.solve(Z))
    want = np.zeros((m, n))
    want[np.arange(n), np.arange(n)] = np.sqrt(2.0)
    for k in range(2):
        assert same_bytes(Z.mat(k), want) and not Z.alpha(k).any() and np.array_equal(Z.jpvt(k), np.arange(n))
        assert Z.ranks()[k] == 0 and same_bytes(Z.bmat(k), Bs[k]) and not Z.xmat(k).any()
    Qz, Rz = R.q_and_r(Z)[0]
    assert not Rz.any() and np.abs(Qz.T @ Qz - np.eye(n)).max() < 1e-12  # (R = 0; Q is still orthonormal)
    # a zero column in matrix 2 of 5
    dirty = [A.copy(order="F") for A in mats]
    dirty[2][:, 3] = 0.0
    Dd = factored(R, dirty, Bs)
    R.ok(R.rank(Dd, RCOND))
    assert Dd.ranks().tolist() == [n, n, n - 1, n, n]
    assert np.all(np.isfinite(Dd.mat(2))) and np.all(np.isfinite(Dd.alpha(2))) and Dd.jpvt(2)[-1] == 3 and Dd.alpha(2)[-1] == 0.0
    assert sorted(Dd.jpvt(2).tolist()) == list(range(n))
    Qm, Rm = R.q_and_r(Dd)[2]
    Q.check_qr(Qm, Rm, dirty[2][:, Dd.jpvt(2)], "f64", "zero column")
    for k in (0, 1, 3, 4):
        assert same_bytes(Dd.mat(k), clean.mat(k)) and same_bytes(Dd.alpha(k), clean.alpha(k)) and np.array_equal(Dd.jpvt(k), clean.jpvt(k)), k
    R.ok(R.solve(Dd))
    for q in range(Dd.nrhs):
        assert Dd.xmat(2)[3, q] == 0.0
        check_solution(dirty[2], Bs[2][:, q], Dd.xmat(2)[:, q], Dd.bmat(2)[n - 1:, q], f"zero column, column {q}")
    # a zero first row: every pivot entry of step 0 is exactly 0 -- alphafactor(0) = -1 keeps the factor valid
    row = [A.copy(order="F") for A in mats]
    for A in row:
        A[0, :] = 0.0
    Dr = factored(R, row, Bs)
    R.ok(R.rank(Dr, -1.0))
    assert Dr.ranks().tolist() == [n] * 5
    for k, (Qm, Rm) in enumerate(R.q_and_r(Dr)):
        assert np.all(np.isfinite(Dr.mat(k))) and np.all(np.isfinite(Dr.alpha(k))) and Dr.alpha(k)[0] < 0
        Q.check_qr(Qm, Rm, row[k][:, Dr.jpvt(k)], "f64", f"zero first row, matrix {k}")


def check_arguments(R, orc):
    """case 6: every DHQR_EINVAL case writes nothing; the empty cases are no-ops"""
    m, n = 16, 8
    mats, Bs = inputs(orc, m, n)
    F = factored(R, mats, Bs)
    R.ok(R.rank(F, RCOND))
    Hs, als, jps = snapshot(F)

    def fresh(with_factor):
        D = PBatch(mats, Bs)
        return D.set_factor(Hs, als, jps, F.ranks().copy()) if with_factor else D

    def same_as(D, E):
        return all(same_bytes(getattr(D, nm), getattr(E, nm)) for nm in D.BUFS)

    bad = [("factor", False, dict(null=("jp",))), ("factor", False, dict(sjp=n - 1)), ("factor", False, dict(null=("al",))),
           ("factor", False, dict(null=("A",))), ("factor", False, dict(lda=m - 1)), ("factor", False, dict(batch=-1)),
           ("factor", False, dict(m=n - 1)), ("factor", False, dict(sA=F.lda * (n - 1) + m - 1)), ("factor", False, dict(sal=n - 1)),
           ("qr_host", False, dict(null=("jp",))), ("qr_host", False, dict(sjp=n - 1)),
           ("solve", True, dict(null=("jp",))), ("solve", True, dict(null=("rk",))), ("solve", True, dict(null=("X",))),
           ("solve", True, dict(null=("B",))), ("solve", True, dict(sjp=n - 1)), ("solve", True, dict(ldx=n - 1)),
           ("solve", True, dict(sX=F.ldx * (F.nrhs - 1) + n - 1)), ("solve", True, dict(ldb=m - 1)), ("solve", True, dict(nrhs=-1)),
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
            extra = (RCOND,) if name in ("rank", "lstsq") else ()
            rc = getattr(R, name)(D, *extra, **kw)
            assert rc == want, f"{name} {kw}: rc {rc}, {R.L.dhqr_last_error()}"
            assert same_as(D, E), f"{name} {kw}: something was written"


def check_profile_counts(R, orc, m, n):
    """a factor counts ONE n_rank1 group, a solve ONE n_solve group per launch, whatever nrhs and batch; rank is not counted"""
    L, h = R.L, R.h
    mats, Bs = inputs(orc, m, n)
    D = PBatch(mats, Bs)
    st = L.Stats()
    assert L.dhqr_set_profiling(h, 1) == 0 and L.dhqr_reset_stats(h) == 0
    R.ok(R.factor(D))
    R.ok(R.rank(D, RCOND))
    assert L.dhqr_get_stats(h, ctypes.byref(st)) == 0 and (st.n_rank1, st.n_solve) == (1, 0), (st.n_rank1, st.n_solve)
    R.ok(R.solve(D))
    assert L.dhqr_get_stats(h, ctypes.byref(st)) == 0 and (st.n_rank1, st.n_solve) == (1, 1), (st.n_rank1, st.n_solve)
    assert L.dhqr_set_profiling(h, 0) == 0
