"""Test-only helpers of the tests of the one-workgroup ComplexF64 multi-column tier (csrc/dhqr_small_complex_nrhs.h:
k_small_zapply) -- test_emulated_small_znrhs.py on the emulated library, test_gpu_small_znrhs.py on the MI355X.  Both files
run the SAME checks, written here once against a `Rig`: the library, three contexts (the default rule | DHQR_TUNE
zsmall_nrhs=1, always the kernel | zsmall_nrhs=0, the routes without it) and the buffers the C ABI is driven on (flat
sentinel-guarded host buffers for the emulated library, device twins of them on the GPU).  The product never imports this
file.

BOUNDS: those of zapplyq_helpers (TOL_Q = 1e-12 max|result| against reflectors applied in np.clongdouble, TOL_X = 1e-9
max|x| against orc.solve_c, zh.T(n) max|A| for A - QR and Q^H Q - I); everything else is byte equality."""
import ctypes

import numpy as np

import zapplyq_helpers as Z
import zbatched_helpers as zh
from zapplyq_helpers import P, ZNBatch, ZOut, same_bytes
from zbatched_helpers import SENT

CW = 6  # SMZA_CW: columns of B per workgroup (consumer waves)
# the smallest shapes at which the kernel can go wrong: one row in the second row slot and one column | exactly one chunk |
# four chunks and a tail of one column | second row slot empty, n > 32 | pivot lane at the 64 boundary | full
SHAPES = [(65, 1), (70, 8), (66, 33), (48, 40), (97, 64), (128, 128)]
NRHS = [1, CW, CW + 1, 2 * CW + 1]  # one column | a full group | a group and a tail of one | two groups and a tail of one
NRHS_MAX = 2 * CW + 1
BATCHES = [1, 3]
TUNE_KERNEL, TUNE_PARENT = "zsmall_nrhs=1", "zsmall_nrhs=0"
SEED = 100


class _Dev:
    """device twins of the flat host buffers of a ZNBatch / ZOut: push() uploads, pull() downloads into the host buffers, so
    the views and sentinel checks of the host class judge what the device wrote"""

    def _twins(self, torch, names):
        self._torch, self._names = torch, names
        self._dev = {}
        for nm in names:
            self._dev[nm] = torch.from_numpy(getattr(self, nm)).to("cuda:0")
        torch.cuda.synchronize()

    def pull(self):
        self._torch.cuda.synchronize()
        for nm in self._names:
            getattr(self, nm)[...] = self._dev[nm].cpu().numpy()
        return self

    def _ptr(self, nm):
        return P(self._dev[nm].data_ptr() + 16 * self.off)


class DevBatch(ZNBatch, _Dev):
    def __init__(self, torch, mats, Bs, als=None, **layout):
        ZNBatch.__init__(self, mats, Bs, als, **layout)
        self._twins(torch, ("A", "al", "B", "X"))

    def pA(self):
        return self._ptr("A")

    def pal(self):
        return self._ptr("al")

    def pB(self):
        return self._ptr("B")

    def pX(self):
        return self._ptr("X")


class DevOut(ZOut, _Dev):
    def __init__(self, torch, batch, rows, cols, **layout):
        ZOut.__init__(self, batch, rows, cols, **layout)
        self._twins(torch, ("buf",))

    def p(self):
        return self._ptr("buf")


class Rig:
    """L: the library through ctypes; Stats: its dhqr_stats class; ctx: {"rule" | "kernel" | "parent": context handle}, all with
    the small route on; torch: None (the emulated library, whose "device" memory is host memory) or the torch module (GPU)"""

    def __init__(self, L, Stats, ctx, orc, torch=None, fbatch=None):
        self.L, self.Stats, self.ctx, self.orc, self.torch = L, Stats, ctx, orc, torch
        self.fbatch = fbatch or {}  # (m, n) -> matrices factored for that shape (3 where not listed)
        self._factors, self._results = {}, {}

    def batch(self, Hs, Bs, als, **layout):
        return ZNBatch(Hs, Bs, als, **layout) if self.torch is None else DevBatch(self.torch, Hs, Bs, als, **layout)

    def out(self, batch, rows, cols):
        return ZOut(batch, rows, cols) if self.torch is None else DevOut(self.torch, batch, rows, cols)

    def ok(self, h, rc, *objs):
        assert rc == 0, self.L.dhqr_last_error()
        assert self.L.dhqr_synchronize(h) == 0, self.L.dhqr_last_error()
        if self.torch is not None:
            for o in objs:
                o.pull()

    def factors(self, m, n, batch=None, seed=SEED, mats=None):
        """computed once per key, shared and left unchanged: (A_k, H_k, alpha_k of dhqr_factor_batched_c64, NRHS_MAX columns B_k)"""
        batch = batch or self.fbatch.get((m, n), 3)
        key = (m, n, batch, seed) if mats is None else None
        if key is None or key not in self._factors:
            ms, Bs = Z.inputs(self.orc, m, n, NRHS_MAX, batch, seed)
            if mats is not None:
                ms = mats
            h = self.ctx["rule"]
            D = self.batch(ms, Bs, None)
            self.ok(h, D.factor(self.L, h), D)
            assert D.padding_intact()
            Hs, als = [np.array(D.mat(k), order="F") for k in range(batch)], [D.alpha(k).copy() for k in range(batch)]
            for a in list(ms) + Bs + Hs + als:
                a.setflags(write=False)
            if key is None:
                return ms, Hs, als, Bs
            self._factors[key] = (ms, Hs, als, Bs)
        return self._factors[key]

    def solved(self, h, Hs, als, Bs, **layout):
        D = self.batch(Hs, Bs, als, **layout)
        A0, al0 = D.A.copy(), D.al.copy()
        self.ok(h, D.solve_nrhs(self.L, h), D)
        assert D.padding_intact() and D.x_untouched()
        assert same_bytes(D.A, A0) and same_bytes(D.al, al0), "the factor and alpha must stay untouched"
        return D

    def applied(self, h, Hs, als, Bs, trans, **layout):
        D = self.batch(Hs, Bs, als, **layout)
        A0, al0 = D.A.copy(), D.al.copy()
        self.ok(h, D.apply_q(self.L, h, trans), D)
        assert D.padding_intact() and D.x_untouched()
        assert same_bytes(D.A, A0) and same_bytes(D.al, al0), "the factor and alpha must stay untouched"
        return D

    def formed_q(self, h, Hs, als, **layout):
        m, n = Hs[0].shape
        D = self.batch(Hs, [Z.eye_columns(m, 1)] * len(Hs), als, **layout)
        A0 = D.A.copy()
        Qb = self.out(len(Hs), m, n)
        self.ok(h, D.form_q(self.L, h, Qb), D, Qb)
        assert Qb.padding_intact() and D.padding_intact() and same_bytes(D.A, A0)
        return Qb

    def formed_r(self, h, Hs, als):
        n = Hs[0].shape[1]
        D = self.batch(Hs, [Z.eye_columns(Hs[0].shape[0], 1)] * len(Hs), als)
        Rb = self.out(len(Hs), n, n)
        self.ok(h, D.form_r(self.L, h, Rb), Rb)
        return Rb

    def single_column(self, h, Hs, als, Bs, r):
        """dhqr_solve_batched_c64 on the columns r of Bs alone -> (batch, m)"""
        D = self.batch(Hs, [np.asfortranarray(B[:, r:r + 1]) for B in Bs], als, pad_ldb=0)
        rc = self.L.dhqr_solve_batched_c64(h, D.pA(), D.m, D.n, D.lda, D.sA, D.pal(), D.sal, D.pB(), D.sB, D.batch)
        self.ok(h, rc, D)
        assert D.padding_intact()
        return np.stack([D.bmat(k)[:, 0] for k in range(D.batch)])

    def result(self, which, op, m, n, r0, nrhs, batch):
        """computed once per key, shared and left unchanged: columns r0 .. r0 + nrhs - 1 of the first `batch` matrices of
        factors(m, n) through op = "solve" | 1 (Q^H B) | 0 (Q B) on the context `which` -> list of (m, nrhs) matrices"""
        key = (which, op, m, n, r0, nrhs, batch)
        if key not in self._results:
            mats, Hs, als, Bs = self.factors(m, n)
            c = [np.asfortranarray(B[:, r0:r0 + nrhs]) for B in Bs[:batch]]
            h = self.ctx[which]
            D = self.solved(h, Hs[:batch], als[:batch], c) if op == "solve" else self.applied(h, Hs[:batch], als[:batch], c, op)
            res = [np.array(D.bmat(k)) for k in range(batch)]
            for a in res:
                a.setflags(write=False)
            self._results[key] = res
        return self._results[key]

    def all_results(self, h, Hs, als, Bs, **layout):
        """(X and tail, Q^H B, Q B, Q) of a batch, each a list of matrices"""
        batch = len(Hs)
        out = [[np.array(self.solved(h, Hs, als, Bs, **layout).bmat(k)) for k in range(batch)]]
        for tr in (1, 0):
            D = self.applied(h, Hs, als, Bs, tr, **layout)
            out.append([np.array(D.bmat(k)) for k in range(batch)])
        Qb = self.formed_q(h, Hs, als, **layout)
        return out + [[np.array(Qb.mat(k)) for k in range(batch)]]

    def n_solve(self, h, call):
        """the n_solve groups that call() adds, profiling on"""
        st = self.Stats()
        assert self.L.dhqr_set_profiling(h, 1) == 0
        try:
            assert self.L.dhqr_reset_stats(h) == 0
            call()
            assert self.L.dhqr_get_stats(h, ctypes.byref(st)) == 0
        finally:
            assert self.L.dhqr_set_profiling(h, 0) == 0
        return st.n_solve


def cut(Bs, nrhs, batch=None):
    return [np.asfortranarray(B[:, :nrhs]) for B in (Bs if batch is None else Bs[:batch])]


def column(Bs, r):
    return [np.asfortranarray(B[:, r:r + 1]) for B in Bs]


# ---- the checks (the letters are those of the contract list in the module docstrings of the two test files) -------------------
def _clip(rig, m, n, cases):
    """the cases [(nrhs, batch)] with batch cut to the matrices factored for the shape"""
    have = len(rig.factors(m, n)[1])
    return sorted({(nrhs, min(batch, have)) for nrhs, batch in cases})


def check_solve_column_bits(rig, m, n, cases):
    """a: column r of dhqr_solve_batched_nrhs_c64 is byte-identical to dhqr_solve_batched_c64 on that column alone, with
    zsmall_nrhs=1 and under the default rule; cases: [(nrhs, batch)]"""
    mats, Hs, als, Bs = rig.factors(m, n)
    cases = _clip(rig, m, n, cases)
    rmax = max(nrhs for nrhs, _ in cases)
    alone = [rig.single_column(rig.ctx["rule"], Hs, als, Bs, r) for r in range(rmax)]
    for which in ("kernel", "rule"):
        for nrhs, batch in cases:
            S = rig.result(which, "solve", m, n, 0, nrhs, batch)
            for k in range(batch):
                for r in range(nrhs):
                    assert same_bytes(S[k][:, r], alone[r][k]), f"{which}, nrhs {nrhs} batch {batch}: matrix {k} column {r}"


def check_tail_bits(rig, m, n, cases):
    """b: rows n .. m-1 of apply-Q with trans = 1 have the bytes of what the solve leaves there"""
    for nrhs, batch in _clip(rig, m, n, cases):
        S, D = rig.result("rule", "solve", m, n, 0, nrhs, batch), rig.result("rule", 1, m, n, 0, nrhs, batch)
        for k in range(batch):
            assert same_bytes(D[k][n:], S[k][n:]), f"nrhs {nrhs} batch {batch}: tail of matrix {k}"


def check_column_independence(rig, m, n, cases):
    """c: every column of apply-Q in both directions has the bytes of its own nrhs = 1 call"""
    cases = _clip(rig, m, n, cases)
    have = len(rig.factors(m, n)[1])
    for tr in (1, 0):
        for nrhs, batch in cases:
            D = rig.result("rule", tr, m, n, 0, nrhs, batch)
            for k in range(batch):
                for r in range(nrhs):
                    alone = rig.result("rule", tr, m, n, r, 1, have)
                    assert same_bytes(D[k][:, r], alone[k][:, 0]), f"trans {tr} nrhs {nrhs} batch {batch}: matrix {k} column {r}"


def check_launch_groups(rig):
    """d: profiling on, (66, 33), batch 3, nrhs = 8: with zsmall_nrhs=1 each of solve, apply-Q (both directions) and form-Q adds
    exactly ONE n_solve; with zsmall_nrhs=0 the solve adds 8"""
    m, n, nrhs = 66, 33, 8
    mats, Hs, als, Bs = rig.factors(m, n, batch=3)
    c = cut(Bs, nrhs)
    h = rig.ctx["kernel"]
    D = rig.batch(Hs, c, als)
    Qb = rig.out(3, m, n)
    L = rig.L
    for name, call in (("solve", lambda: D.solve_nrhs(L, h)), ("Q^H B", lambda: D.apply_q(L, h, 1)), ("Q B", lambda: D.apply_q(L, h, 0)),
                       ("form_q", lambda: D.form_q(L, h, Qb))):
        got = rig.n_solve(h, lambda: rig.ok(h, call()))
        assert got == 1, f"{name}: {got} n_solve groups with {TUNE_KERNEL}"
    h0 = rig.ctx["parent"]
    got = rig.n_solve(h0, lambda: rig.ok(h0, D.solve_nrhs(L, h0)))
    assert got == nrhs, f"solve: {got} n_solve groups with {TUNE_PARENT}"


def check_accuracy(rig, m, n, nrhs=CW + 1, batch=None):
    """e: both directions against reflect_clongdouble, Q (Q^H B) = B, x against orc.solve_c, form_q equal (np.array_equal) to
    apply-Q with trans = 0 on [I; 0], A = QR and Q^H Q = I within zh.T(n)"""
    mats, Hs, als, Bs = (v[:batch] for v in rig.factors(m, n))
    batch = len(Hs)
    c = cut(Bs, nrhs)
    h = rig.ctx["rule"]
    L = rig.L
    X, QhB, QB, Qs = rig.all_results(h, Hs, als, c)
    D = rig.batch(Hs, QhB, als)
    rig.ok(h, D.apply_q(L, h, 0), D)  # Q (Q^H B)
    E = rig.applied(h, Hs, als, [Z.eye_columns(m, n)] * batch, 0)
    Rb = rig.formed_r(h, Hs, als)
    for k in range(batch):
        Z.check_close(QhB[k], Z.reflect_clongdouble(Hs[k], c[k], 1), f"{m}x{n} Q^H B matrix {k}")
        Z.check_close(QB[k], Z.reflect_clongdouble(Hs[k], c[k], 0), f"{m}x{n} Q B matrix {k}")
        Z.check_close(D.bmat(k), c[k], f"{m}x{n} Q (Q^H B) matrix {k}")
        Z.check_x(rig.orc, mats[k], c[k], X[k][:n], f"{m}x{n} matrix {k}")
        assert not (Qs[k] == SENT).any()
        assert np.array_equal(Qs[k], E.bmat(k)), f"form_q != Q [I; 0] for matrix {k}"
        Z.check_qr(Qs[k], Rb.mat(k), mats[k], f"{m}x{n} matrix {k}")


def check_switch(rig, m, n, nrhs=CW + 1):
    """f: with zsmall_nrhs=0 the solve's bytes are unchanged; apply-Q and the explicit Q agree with the kernel's within TOL_Q"""
    mats, Hs, als, Bs = rig.factors(m, n)
    c = cut(Bs, nrhs)
    new, old = (rig.all_results(rig.ctx[w], Hs, als, c) for w in ("kernel", "parent"))
    for k in range(len(Hs)):
        assert same_bytes(new[0][k], old[0][k]), f"solve of matrix {k}: {TUNE_PARENT} changed the bytes"
        for i, what in ((1, "Q^H B"), (2, "Q B"), (3, "Q")):
            Z.check_close(old[i][k], new[i][k], f"{m}x{n} {what} matrix {k}, {TUNE_PARENT} against the kernel")


def check_layout(rig, m, n, nrhs=CW + 1, host_rig=None):
    """g: lda = m + 1, padded strides, base one element in: the packed call's bytes, every sentinel intact, the factor and
    alpha untouched (inside the Rig's calls); the host form dhqr_ldiv_batched_nrhs_c64 on the same layout leaves B untouched"""
    mats, Hs, als, Bs = rig.factors(m, n)
    c = cut(Bs, nrhs)
    h = rig.ctx["kernel"]
    G = ZNBatch(Hs, c, als)  # (host arrays: the host form)
    assert (G.lda, G.sal, G.off, G.ldb) == (m + 1, n + 3, 1, m + 1)
    want = rig.all_results(h, Hs, als, c, pad_ld=0, pad=0, pad_ldb=0, pad_ldx=0, off=0)
    got = rig.all_results(h, Hs, als, c)
    for w, g in zip(want, got):
        for k in range(len(Hs)):
            assert same_bytes(w[k], g[k]), k
    before = [b.copy() for b in (G.A, G.al, G.B)]
    rc = G.ldiv_nrhs(rig.L, h)
    assert rc == 0, rig.L.dhqr_last_error()
    assert G.padding_intact()
    for b, b0 in zip((G.A, G.al, G.B), before):
        assert same_bytes(b, b0), "the host form must leave the factor, alpha and B untouched"
    for k in range(len(Hs)):
        assert same_bytes(G.xmat(k), want[0][k][:n]), k


def check_isolation(rig, m, n, nrhs=CW + 1):
    """h: a zero column in matrix 1 of 3 gives a non-finite factor there; matrices 0 and 2 keep their bytes in all four
    operations"""
    clean = rig.factors(m, n, seed=700)
    bad = [zh.poison_column(A, min(3, n - 1)) if k == 1 else A for k, A in enumerate(clean[0])]
    dirty = rig.factors(m, n, seed=700, mats=bad)
    assert not np.isfinite(dirty[1][1]).all(), "the zero column was meant to give a non-finite factor"
    h = rig.ctx["kernel"]
    runs = [rig.all_results(h, Hs, als, cut(Bs, nrhs)) for _, Hs, als, Bs in (clean, dirty)]
    for c, d in zip(*runs):
        for k in (0, 2):
            assert same_bytes(c[k], d[k]), k


def check_repeatable(rig, m, n, nrhs=CW + 1):
    """i: three calls give the same bytes"""
    mats, Hs, als, Bs = rig.factors(m, n)
    c = cut(Bs, nrhs)
    runs = [rig.all_results(rig.ctx["kernel"], Hs, als, c) for _ in range(3)]
    for again in runs[1:]:
        for a, b in zip(runs[0], again):
            for k in range(len(Hs)):
                assert same_bytes(a[k], b[k]), k
