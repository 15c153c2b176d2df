"""`H \\ B` with several right-hand sides, Q application, explicit Q and R for batches of small ComplexF64 factors on the
MI355X: dhqr_solve_batched_nrhs_c64 / dhqr_apply_q_batched_c64 / dhqr_form_q_batched_c64 / dhqr_form_r_batched_c64 through the
C ABI on guarded device buffers -- the wave-per-matrix kernels of csrc/dhqr_batched_complex_nrhs.h bit for bit against the
single-column solve, against reflectors applied in np.clongdouble and against the oracle (bounds: zapplyq_helpers.py) --,
the general tier, and solve_batched_nrhs / apply_q_batched_ / form_q_batched / form_r_batched on device tensors."""
import ctypes

import numpy as np
import pytest

import zapplyq_helpers as Z
import zbatched_helpers as zh
from zapplyq_helpers import P, ZNBatch, ZOut, same_bytes
from zbatched_helpers import SENT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NRHS_MAX = 9


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture
def abi(pkg, torch_cuda):
    """(library, context) with the small route on for one test (conftest.py switches it off for the suite)"""
    L = pkg._lib.lib()
    for name in ("dhqr_solve_batched_nrhs_c64", "dhqr_ldiv_batched_nrhs_c64", "dhqr_apply_q_batched_c64", "dhqr_form_q_batched_c64",
                 "dhqr_form_r_batched_c64"):
        assert hasattr(L, name), f"the library does not export {name}"
    ctx = pkg.get_context(0)
    ctx.use_torch_stream()
    ctx.set_small_route(True)
    yield L, ctx
    ctx.set_small_route(False)


@pytest.fixture
def abi_kernel(pkg, torch_cuda, abi):
    """(library, a context of its own that sends EVERY wave-tier solve to the multi-column kernel, tail groups included: the
    default context's rule sends only nrhs >= 4 in full groups there)"""
    import os
    old = os.environ.get("DHQR_TUNE")
    os.environ["DHQR_TUNE"] = Z.TUNE_KERNEL
    try:
        ctx = pkg.Context(0)
    finally:
        if old is None:
            os.environ.pop("DHQR_TUNE", None)
        else:
            os.environ["DHQR_TUNE"] = old
    ctx.use_torch_stream()
    ctx.set_small_route(True)
    yield abi[0], ctx
    ctx.close()


class _Dev:
    """device twins of the flat host buffers of a ZNBatch / ZOut: push() uploads, pull() downloads into the host buffers, so
    the views and sentinel checks of the host class judge what the device wrote"""

    def _twins(self, torch, names):
        self._torch, self._names = torch, names
        self._dev = {}
        self.push()

    def push(self):
        for nm in self._names:
            self._dev[nm] = self._torch.from_numpy(getattr(self, nm)).to(DEV)
        self._torch.cuda.synchronize()

    def pull(self):
        self._torch.cuda.synchronize()
        for nm in self._names:
            getattr(self, nm)[...] = self._dev[nm].cpu().numpy()
        return self

    def _ptr(self, nm):
        return P(self._dev[nm].data_ptr() + 16 * self.off)


class GBatch(ZNBatch, _Dev):
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

    def single_column(self, L, h, r, B0):
        b = self._torch.from_numpy(np.ascontiguousarray(np.stack([B0[k][:, r] for k in range(self.batch)]))).to(DEV)
        rc = L.dhqr_solve_batched_c64(h, self.pA(), self.m, self.n, self.lda, self.sA, self.pal(), self.sal, P(b.data_ptr()), self.m, self.batch)
        assert rc == 0, L.dhqr_last_error()
        self._torch.cuda.synchronize()
        return b.cpu().numpy()


class GOut(ZOut, _Dev):
    def __init__(self, torch, batch, rows, cols, **layout):
        ZOut.__init__(self, batch, rows, cols, **layout)
        self._twins(torch, ("buf",))

    def p(self):
        return self._ptr("buf")


def _ok(abi, rc):
    L, ctx = abi
    assert rc == 0, L.dhqr_last_error()
    ctx.synchronize()


_FACTORS = {}


def _factors(abi, torch, orc, m, n, batch=9, seed=Z.SEED, mats=None, small=True):
    """computed once per key on the device, shared and left unchanged: (A_k, H_k, alpha_k, B_k with NRHS_MAX columns)"""
    L, ctx = abi
    key = (m, n, batch, seed, small) if mats is None else None
    if key is None or key not in _FACTORS:
        ms, Bs = Z.inputs(orc, m, n, NRHS_MAX, batch, seed)
        if mats is not None:
            ms = mats
        ctx.set_small_route(small)
        D = GBatch(torch, ms, Bs)
        _ok(abi, D.factor(L, ctx.handle))
        D.pull()
        assert D.padding_intact()
        Hs, als = [np.array(D.mat(k), order="F") for k in range(batch)], [D.alpha(k).copy() for k in range(batch)]
        for a in list(ms) + Bs + Hs + als:
            a.setflags(write=False)
        if key is None:
            return ms, Hs, als, Bs
        _FACTORS[key] = (ms, Hs, als, Bs)
    return _FACTORS[key]


def _cut(Bs, nrhs, batch=None):
    return [np.asfortranarray(B[:, :nrhs]) for B in (Bs if batch is None else Bs[:batch])]


def _applied(abi, torch, Hs, als, Bs, trans, **layout):
    L, ctx = abi
    D = GBatch(torch, Hs, Bs, als, **layout)
    _ok(abi, D.apply_q(L, ctx.handle, trans))
    D.pull()
    assert D.padding_intact() and D.x_untouched()
    return D


def _solved(abi, torch, Hs, als, Bs, **layout):
    L, ctx = abi
    D = GBatch(torch, Hs, Bs, als, **layout)
    _ok(abi, D.solve_nrhs(L, ctx.handle))
    D.pull()
    assert D.padding_intact() and D.x_untouched()
    return D


def _q_and_r(abi, torch, Hs, als, **layout):
    L, ctx = abi
    m, n = Hs[0].shape
    batch = len(Hs)
    D = GBatch(torch, Hs, [Z.eye_columns(m, n)] * batch, als, **layout)
    Qb, Rb = GOut(torch, batch, m, n), GOut(torch, batch, n, n)
    _ok(abi, D.form_q(L, ctx.handle, Qb))
    _ok(abi, D.form_r(L, ctx.handle, Rb))
    _ok(abi, D.apply_q(L, ctx.handle, 0))
    Qb.pull(), Rb.pull(), D.pull()
    assert Qb.padding_intact() and Rb.padding_intact() and D.padding_intact()
    for k in range(batch):
        assert not (Qb.mat(k) == SENT).any() and not (Rb.mat(k) == SENT).any()
    return Qb, Rb, D


def _all_results(abi, torch, Hs, als, Bs, **layout):
    """(X and tail, Q^H B, Q B, Q, R) of a batch, each a list of matrices"""
    batch = len(Hs)
    out = [[np.array(_solved(abi, torch, Hs, als, Bs, **layout).bmat(k)) for k in range(batch)]]
    for tr in (1, 0):
        D = _applied(abi, torch, Hs, als, Bs, tr, **layout)
        out.append([np.array(D.bmat(k)) for k in range(batch)])
    Qb, Rb, _ = _q_and_r(abi, torch, Hs, als, **layout)
    return out + [[np.array(Qb.mat(k)) for k in range(batch)], [np.array(Rb.mat(k)) for k in range(batch)]]


@pytest.mark.parametrize("m,n", Z.GPU_SHAPES)
def test_bits_at_the_wave_tier(abi, abi_kernel, torch_cuda, orc, m, n):
    """item 1: column r of the multi-column solve has the bytes of dhqr_solve_batched_c64 on it alone -- on the kernel (a context
    that always takes it) and under the default context's rule; rows n .. m-1 of apply_q(trans = 1) the bytes of the solve's;
    every column of both directions the bytes of its nrhs = 1 call; batches of 9 (a partial workgroup) and 1"""
    torch = torch_cuda
    L, ctx = abi
    mats, Hs, als, Bs = _factors(abi, torch, orc, m, n)
    F = GBatch(torch, Hs, _cut(Bs, 1), als)
    alone = [F.single_column(L, ctx.handle, r, Bs) for r in range(NRHS_MAX)]
    alone_q = {tr: _applied(abi, torch, Hs, als, Bs, tr) for tr in (0, 1)}  # (column independence is checked against nrhs = 1 below)
    one = {tr: [_applied(abi, torch, Hs, als, [np.asfortranarray(B[:, r:r + 1]) for B in Bs], tr) for r in (0, 6)] for tr in (0, 1)}
    for tr in (0, 1):
        for k in range(9):
            for i, r in enumerate((0, 6)):
                assert same_bytes(alone_q[tr].bmat(k)[:, r], one[tr][i].bmat(k)[:, 0]), f"trans {tr}: matrix {k} column {r} != its nrhs = 1 call"
    for nrhs in sorted({1, Z.rg_solve(n) + 1, Z.rg_apply(n) + 1, 7, 2 * Z.rg_solve(n) + 1}):
        for batch in (9, 1):
            cut = _cut(Bs, nrhs, batch)
            S = _solved(abi_kernel, torch, Hs[:batch], als[:batch], cut)
            for k in range(batch):
                for r in range(nrhs):
                    assert same_bytes(S.bmat(k)[:, r], alone[r][k]), f"nrhs {nrhs} batch {batch}: matrix {k} column {r}"
            for tr in (1, 0):
                D = _applied(abi, torch, Hs[:batch], als[:batch], cut, tr)
                for k in range(batch):
                    if tr == 1:
                        assert same_bytes(D.bmat(k)[n:], S.bmat(k)[n:]), f"nrhs {nrhs} batch {batch}: tail of matrix {k}"
                    assert same_bytes(D.bmat(k), alone_q[tr].bmat(k)[:, :nrhs]), f"trans {tr} nrhs {nrhs} batch {batch}: matrix {k}"
    ctx.reset_stats()
    ctx.set_profiling(True)
    try:
        for nrhs in Z.RULE_NRHS:  # the default context: one launch where its rule takes the kernel, nrhs in the column loop
            ctx.reset_stats()
            S = _solved(abi, torch, Hs, als, _cut(Bs, nrhs))
            assert ctx.stats()["n_solve"] == (1 if Z.rule_takes_kernel(n, nrhs) else nrhs), nrhs
            for k in range(9):
                for r in range(nrhs):
                    assert same_bytes(S.bmat(k)[:, r], alone[r][k]), f"rule, nrhs {nrhs}: matrix {k} column {r}"
    finally:
        ctx.set_profiling(False)


def _check_accuracy(orc, mats, Hs, als, cut, res, what):
    X, QhB, QB, Qs, Rs = res
    m, n = Hs[0].shape
    for k in range(len(Hs)):
        Z.check_close(QhB[k], Z.reflect_clongdouble(Hs[k], cut[k], 1), f"{what} Q^H B matrix {k}")
        Z.check_close(QB[k], Z.reflect_clongdouble(Hs[k], cut[k], 0), f"{what} Q B matrix {k}")
        Z.check_x(orc, mats[k], cut[k], X[k][:n], f"{what} matrix {k}")
        Z.check_close(Qs[k], Z.reflect_clongdouble(Hs[k], Z.eye_columns(m, n), 0), f"{what} Q matrix {k}")
        Z.check_r(Rs[k], Hs[k], als[k])
        Z.check_qr(Qs[k], Rs[k], mats[k], f"{what} matrix {k}")


@pytest.mark.parametrize("m,n", Z.GPU_SHAPES)
def test_accuracy_and_explicit_q_and_r(abi, torch_cuda, orc, m, n):
    """item 2: both directions against the clongdouble reflectors, Q (Q^H B) = B, x against orc.solve_c, form_q equal to
    apply_q(trans = 0) on [I; 0], R strictly upper + alpha, A = QR and Q^H Q = I"""
    torch = torch_cuda
    L, ctx = abi
    mats, Hs, als, Bs = _factors(abi, torch, orc, m, n)
    cut = _cut(Bs, 7)
    _check_accuracy(orc, mats, Hs, als, cut, _all_results(abi, torch, Hs, als, cut), f"{m}x{n}")
    D = _applied(abi, torch, Hs, als, cut, 1)
    _ok(abi, D.apply_q(L, ctx.handle, 0))
    D.pull()
    Qb, Rb, E = _q_and_r(abi, torch, Hs, als)
    for k in range(9):
        Z.check_close(D.bmat(k), cut[k], f"{m}x{n} Q (Q^H B) matrix {k}")
        assert np.array_equal(Qb.mat(k), E.bmat(k)), f"form_q != Q [I; 0] for matrix {k}"


@pytest.mark.parametrize("m,n", [(16, 8), (64, 32)])
def test_special_matrices(abi, torch_cuda, orc, m, n):
    """item 3: imaginary part zero, real part zero, a pivot of exactly zero"""
    torch = torch_cuda
    mats, Hs, als, Bs = _factors(abi, torch, orc, m, n, batch=7, seed=900, mats=zh.special_matrices(orc, m, n))
    cut = _cut(Bs, 5)
    res = _all_results(abi, torch, Hs, als, cut)
    _check_accuracy(orc, mats, Hs, als, cut, res, f"special {m}x{n}")
    for k in (1, 5):  # a real factor gives a real Q and R
        assert (res[3][k].imag == 0).all() and (res[4][k].imag == 0).all()


def test_a_zero_column_stays_in_its_matrix(abi, torch_cuda, orc):
    """item 4: matrix 2 of five has a zero column: the other four keep their bits in all four operations"""
    torch = torch_cuda
    m, n, nrhs = 16, 8, 5
    clean = _factors(abi, torch, orc, m, n, batch=5, seed=700)
    bad = [zh.poison_column(A) if k == 2 else A for k, A in enumerate(clean[0])]
    dirty = _factors(abi, torch, orc, m, n, batch=5, seed=700, mats=bad)
    assert not np.isfinite(dirty[1][2]).all(), "the zero column was meant to give a non-finite factor"
    runs = [_all_results(abi, torch, Hs, als, _cut(Bs, nrhs)) for _, Hs, als, Bs in (clean, dirty)]
    for c, d in zip(*runs):
        for k in (0, 1, 3, 4):
            assert same_bytes(c[k], d[k]), k


def test_guarded_layout_gives_the_packed_bits(abi, torch_cuda, orc):
    """item 6: (40, 17), nrhs 5: lda = m + 1, padded strides, base one element in -- the packed call's bits, every sentinel
    intact (checked inside the helpers), for the four device entry points; the host form on the same layout"""
    torch = torch_cuda
    L, ctx = abi
    m, n, nrhs = 40, 17, 5
    mats, Hs, als, Bs = _factors(abi, torch, orc, m, n)
    cut = _cut(Bs, nrhs)
    want = _all_results(abi, torch, Hs, als, cut, pad_ld=0, pad=0, pad_ldb=0, pad_ldx=0, off=0)
    got = _all_results(abi, torch, Hs, als, cut)
    for w, g in zip(want, got):
        for k in range(9):
            assert same_bytes(w[k], g[k]), k
    G = ZNBatch(Hs, cut, als)  # host arrays: dhqr_ldiv_batched_nrhs_c64
    assert (G.lda, G.sal, G.off, G.ldb) == (m + 1, n + 3, 1, m + 1)
    B0 = G.B.copy()
    _ok(abi, G.ldiv_nrhs(L, ctx.handle))
    assert G.padding_intact() and same_bytes(G.B, B0)
    for k in range(9):
        assert same_bytes(G.xmat(k), want[0][k][:n])


def test_the_general_tier(abi, torch_cuda, orc):
    """item 5 at (66, 33), batch 2: the accuracy of item 2, the solve byte-identical to the column loop, repeatable bit for bit"""
    torch = torch_cuda
    L, ctx = abi
    m, n, batch, nrhs = 66, 33, 2, 3
    mats, Hs, als, Bs = _factors(abi, torch, orc, m, n, batch=batch, seed=200)
    cut = _cut(Bs, nrhs)
    runs = [_all_results(abi, torch, Hs, als, cut) for _ in range(3)]
    for again in runs[1:]:
        for a, b in zip(runs[0], again):
            for k in range(batch):
                assert same_bytes(a[k], b[k]), "the general tier must be repeatable bit for bit"
    F = GBatch(torch, Hs, _cut(Bs, 1), als)
    for r in range(nrhs):
        col = F.single_column(L, ctx.handle, r, Bs)
        for k in range(batch):
            assert same_bytes(runs[0][0][k][:, r], col[k]), f"solve column {r} of matrix {k} != the column loop"
    _check_accuracy(orc, mats, Hs, als, cut, runs[0], f"{m}x{n} general")


def _to_dev(torch, mats):
    """(batch, rows, cols) device tensor with column-major matrices holding the host matrices"""
    batch, (rows, cols) = len(mats), mats[0].shape
    A = torch.empty((batch, cols, rows), dtype=torch.complex128, device=DEV).transpose(1, 2)
    A.copy_(torch.from_numpy(np.stack(mats)))
    return A


@pytest.mark.parametrize("m,n", [(16, 8), (66, 33)])
def test_python_functions_equal_the_c_abi(pkg, abi, torch_cuda, orc, m, n):
    """solve_batched_nrhs / apply_q_batched_ / form_q_batched / form_r_batched on device tensors and numpy arrays: the C ABI's
    results; B is not modified; a single matrix is a batch of one; float64 goes to the generic names"""
    torch = torch_cuda
    batch, nrhs = 3, 5
    mats, Hs, als, Bs = _factors(abi, torch, orc, m, n, batch=batch, seed=300)
    cut = _cut(Bs, nrhs)
    X, QhB, QB, Qs, Rs = _all_results(abi, torch, Hs, als, cut)
    H = pkg.DistributedHouseholderQRStruct(_to_dev(torch, Hs), torch.from_numpy(np.stack(als)).to(DEV))
    B = _to_dev(torch, cut)
    B0 = B.clone()
    Xd = pkg.solve_batched_nrhs(H, B)
    assert torch.equal(B, B0), "B must not be modified"
    assert tuple(Xd.shape) == (batch, n, nrhs) and Xd.dtype == torch.complex128
    Xh = pkg.solve_batched_nrhs(pkg.DistributedHouseholderQRStruct(np.stack(Hs), np.stack(als)), np.stack(cut))
    Qd, Rd = pkg.form_q_batched(H), pkg.form_r_batched(H)
    W1, W0 = pkg.apply_q_batched_(H, B.clone().transpose(1, 2).contiguous().transpose(1, 2), True), None
    W0 = pkg.apply_q_batched_(H, B.clone().transpose(1, 2).contiguous().transpose(1, 2), False)
    for k in range(batch):
        assert same_bytes(Xd[k].cpu().numpy(), X[k][:n]) and same_bytes(np.asarray(Xh[k]), X[k][:n]), k
        assert same_bytes(W1[k].cpu().numpy(), QhB[k]) and same_bytes(W0[k].cpu().numpy(), QB[k]), k
        assert same_bytes(Qd[k].cpu().numpy(), Qs[k]) and same_bytes(Rd[k].cpu().numpy(), Rs[k]), k
    H1 = pkg.DistributedHouseholderQRStruct(H.A[0], H.α[0].contiguous())  # a single matrix
    assert same_bytes(pkg.solve_batched_nrhs(H1, B[0]).cpu().numpy(), X[0][:n])
    assert same_bytes(pkg.form_q_batched(H1).cpu().numpy(), Qs[0]) and same_bytes(pkg.form_r_batched(H1).cpu().numpy(), Rs[0])
    assert same_bytes(pkg.apply_q_batched_(H1, B[0].clone().t().contiguous().t(), True).cpu().numpy(), QhB[0])
    if m <= 64:  # float64: exactly what the generic names return
        Ar = pkg.rand_colmajor_batched(batch, m, n, 7, DEV)
        Br = pkg.rand_colmajor_batched(batch, m, nrhs, 8, DEV)
        Hr = pkg.qr_batched_(Ar)
        assert torch.equal(pkg.solve_batched_nrhs(Hr, Br), pkg.ldiv(Hr, Br))
        assert torch.equal(pkg.form_q_batched(Hr), pkg.get_q(Hr)) and torch.equal(pkg.form_r_batched(Hr), pkg.get_r(Hr))
        assert torch.equal(pkg.apply_q_batched_(Hr, Br.clone().transpose(1, 2).contiguous().transpose(1, 2), True),
                           pkg.apply_q_(Hr, Br.clone().transpose(1, 2).contiguous().transpose(1, 2), True))


def test_batch_300(abi, torch_cuda, orc):
    """75 workgroups at (40, 17), nrhs = 5: every matrix within the accuracy bounds, in all four operations"""
    torch = torch_cuda
    m, n, nrhs, batch = 40, 17, 5, 300
    mats, Hs, als, Bs = _factors(abi, torch, orc, m, n, batch=batch)
    cut = _cut(Bs, nrhs)
    _check_accuracy(orc, mats, Hs, als, cut, _all_results(abi, torch, Hs, als, cut), f"{m}x{n} batch 300")
