"""Every route on the matrix layouts a caller may pass: a leading dimension above m (even, odd, wide), a base 8 bytes off a
16-byte boundary, and both (layout_helpers.LAYOUTS).  The host picks the 16-byte operand path or the scalar one from
exactly these properties (lda % 2, rows % 2, the alignment of each pointer); the rest of the suite only ever runs
lda == m at an aligned base.

Each matrix and vector sits in a buffer poisoned with a quiet NaN outside its window (layout_helpers): a store outside the
window shows up bit for bit, a load from there that reaches the arithmetic turns the result into NaN.  Results against the
oracle element by element (TOL of test_gpu_parity.py for H and alpha, 1e-9 relative for x), ||A - QR|| / ||A|| < 1e-12,
then the guards.  The matrix content is the same in every layout: one oracle factorisation per shape, every layout of the
shape in one test (a failure message names every layout that failed)."""
import ctypes

import numpy as np
import pytest

from layout_helpers import assert_guards_intact, each_layout, guarded_matrix, guarded_vector
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
DEV = "cuda:0"


_ORC = {}


def _oracle(orc, m, n, seed):
    """(A0, H, alpha) of the oracle; the last two shapes are kept (the solve tests visit a shape once per mode)"""
    key = (m, n, seed)
    if key not in _ORC:
        while len(_ORC) >= 2:
            _ORC.pop(next(iter(_ORC)))
        A0 = orc.rand_matrix(m, n, seed)
        _ORC[key] = (A0,) + tuple(orc.householder(A0))
    return _ORC[key]


def _qtb(Ho, b):
    """Q'b from the oracle's reflectors (H_n ... H_1 b, src:215-242)"""
    y = np.array(b, dtype=np.float64)
    for j in range(Ho.shape[1]):
        y[j:] -= Ho[j:, j] * (Ho[j:, j] @ y[j:])
    return y


def _dev(X):
    """column-major device copy of a host matrix (lda == m)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(X).T)).to(DEV).T


def _check_factor(G, al, Ho, ao):
    scale = np.abs(Ho).max()
    eH = np.abs(G.host() - Ho).max()
    ea = np.abs(al.host() - ao).max()
    assert eH <= TOL(Ho) * scale and ea <= TOL(Ho) * scale, f"|dH| = {eH / scale:.2e}, |dalpha| = {ea / scale:.2e} (max|H|)"


def _factor(pkg, ctx, G, al, nb):
    L = pkg._lib.lib()
    m, n = G.view.shape
    ctx.use_torch_stream()
    pkg._lib.check(L.dhqr_factor_f64(ctx.handle, P(G.ptr), m, n, G.ld, P(al.ptr), nb))
    ctx.synchronize()


def _factor_layouts(pkg, orc, m, n, nb, seed, ctx=None, layouts=None):
    ctx = ctx or pkg.get_context(0)
    A0, Ho, ao = _oracle(orc, m, n, seed)
    A0d = _dev(A0)

    def run(lda, off):
        G = guarded_matrix(m, n, lda, off, device=DEV, content=A0)
        al = guarded_vector(n, off, device=DEV)
        _factor(pkg, ctx, G, al, nb)
        _check_factor(G, al, Ho, ao)
        res = pkg.residual(pkg.DistributedHouseholderQRStruct(G.view, al.view), A0d)
        assert res < 1e-12, f"||A - QR|| / ||A|| = {res:.2e}"
        assert_guards_intact(G, "A")
        assert_guards_intact(al, "alpha")

    each_layout(m, run, layouts)


# one shape from each rung of the unblocked kernel ladder of test_unblocked_vs_oracle: register-resident columns, the
# K-reflector passes (k_rankk_fused), k_rankk_tall (8192 < rows <= 16384), k_rankk_xtall (<= 32768), one reflector per
# launch above; even m is the case that matters (odd stride / offset base must leave the 16-byte path)
@pytest.mark.parametrize("m,n", [(1000, 64), (2000, 48), (8192, 24), (9001, 16), (1030, 600), (12288, 64), (20000, 64),
                                 (40000, 24)])
def test_unblocked_on_guarded_layouts(pkg, orc, m, n):
    _factor_layouts(pkg, orc, m, n, 0, 3)


@pytest.mark.parametrize("m,n", [(300, 200), (1000, 999), (2050, 1030), (1281, 896), (3000, 1152), (2048, 2048)])
def test_blocked_on_guarded_layouts(pkg, orc, m, n):
    _factor_layouts(pkg, orc, m, n, 128, 4)


def test_blocked_quads_and_stream_k_on_guarded_layouts(pkg, orc, monkeypatch):
    """4096^2 with the K = 512 quad steps (DHQR_QUAD_MIN_COLS=0) and the stream-K decomposition of the wide k_gemm_tn2
    launches (tn_min_tiles=3): on the 16-byte layouts the quads run, on the others the host must fall back to pairs
    (dhqr_dist.h: quads need even m and lda and an aligned base)"""
    monkeypatch.setenv("DHQR_QUAD_MIN_COLS", "0")  # read by dhqr_create
    monkeypatch.setenv("DHQR_TUNE", "tn_min_tiles=3")
    ctx = pkg.Context(0)
    try:
        _factor_layouts(pkg, orc, 4096, 4096, 128, 4, ctx=ctx)
    finally:
        ctx.close()


@pytest.mark.parametrize("m,n", [(110, 100), (220, 200), (256, 192), (129, 129)])
def test_small_route_device_pointers_on_guarded_layouts(pkg, orc, m, n):
    """dhqr_factor_f64 / dhqr_solve_f64 on the single-workgroup route (csrc/dhqr_small.h): the device-resident entry points
    launch k_small_qr_d / k_small_ldiv on the caller's own lda (the host-array path copies into a buffer of its own)"""
    import torch
    L = pkg._lib.lib()
    A0, Ho, ao = _oracle(orc, m, n, 41)
    b = orc.rand_vector(m, 42)
    xo = orc.solve(Ho, ao, b)
    qtb = _qtb(Ho, b)
    ctx = pkg.Context(0)
    ctx.set_small_route(True)

    def run(lda, off):
        G = guarded_matrix(m, n, lda, off, device=DEV, content=A0)
        al = guarded_vector(n, off, device=DEV)
        ctx.reset_stats()
        ctx.set_profiling(True)
        _factor(pkg, ctx, G, al, 128)
        st = ctx.stats()
        ctx.set_profiling(False)
        assert (st["n_rank1"], st["n_panel"]) == (1, 0), f"not the single-workgroup route: {st}"
        _check_factor(G, al, Ho, ao)
        bits = (G.bits().copy(), al.bits().copy())
        for boff in (0, 1):
            bg = guarded_vector(m, boff, device=DEV, content=b)
            ctx.use_torch_stream()
            pkg._lib.check(L.dhqr_solve_f64(ctx.handle, P(G.ptr), m, n, lda, P(al.ptr), P(bg.ptr)))
            ctx.synchronize()
            got = bg.host()
            assert np.abs(got[:n] - xo).max() <= 1e-9 * np.abs(xo).max(), f"b off {boff}: |dx| = {np.abs(got[:n] - xo).max():.2e}"
            if m > n:
                assert np.abs(got[n:] - qtb[n:]).max() <= 1e-12 * max(1.0, np.abs(qtb).max()), f"b off {boff}: Q'b tail"
            assert_guards_intact(bg, f"b (off {boff})")
        assert np.array_equal(G.bits(), bits[0]) and np.array_equal(al.bits(), bits[1]), "the solve wrote into A or alpha"
        assert_guards_intact(G, "A")
        assert_guards_intact(al, "alpha")
        torch.cuda.synchronize()

    try:
        each_layout(m, run)
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["kept_t", "gram", "persistent"])
@pytest.mark.parametrize("m,n", [(1100, 1000), (777, 130), (16400, 256)])
def test_solve_on_guarded_layouts(pkg, orc, monkeypatch, m, n, mode):
    """dhqr_solve_f64 with A padded / offset and b aligned or 8 bytes off (the 16-byte path depends on both):
    kept_t -- right after a blocked factorisation of the same buffer (T' kept by the factorisation, DHQR_KEEP_T);
    gram -- DHQR_KEEP_T=0 on the oracle's factor (the batched Gram / T' pre-pass); persistent -- DHQR_SOLVE_PIPE=3 (the
    persistent Q'b kernel).  db[0:n] = x, db[n:m] = (Q'b)[n:m] (include/dhqr.h), nothing outside db[0:m] changes, and
    A / alpha are read only."""
    L = pkg._lib.lib()
    A0, Ho, ao = _oracle(orc, m, n, 31)
    b = orc.rand_vector(m, 32)
    xo = orc.solve(Ho, ao, b)
    qtb = _qtb(Ho, b)
    if mode == "gram":
        monkeypatch.setenv("DHQR_KEEP_T", "0")  # read by dhqr_create
    elif mode == "persistent":
        monkeypatch.setenv("DHQR_SOLVE_PIPE", "3")
    ctx = pkg.Context(0)

    def run(lda, off):
        if mode == "kept_t":
            G = guarded_matrix(m, n, lda, off, device=DEV, content=A0)
            al = guarded_vector(n, off, device=DEV)
            _factor(pkg, ctx, G, al, 128)
            _check_factor(G, al, Ho, ao)
        else:
            G = guarded_matrix(m, n, lda, off, device=DEV, content=Ho)
            al = guarded_vector(n, off, device=DEV, content=ao)
        bits = (G.bits().copy(), al.bits().copy())
        for boff in (0, 1):
            bg = guarded_vector(m, boff, device=DEV, content=b)
            ctx.use_torch_stream()
            pkg._lib.check(L.dhqr_solve_f64(ctx.handle, P(G.ptr), m, n, lda, P(al.ptr), P(bg.ptr)))
            ctx.synchronize()
            got = bg.host()
            ex = np.abs(got[:n] - xo).max()
            assert ex <= 1e-9 * np.abs(xo).max(), f"b off {boff}: |dx| = {ex / np.abs(xo).max():.2e} relative"
            et = np.abs(got[n:] - qtb[n:]).max() if m > n else 0.0
            assert et <= 1e-12 * max(1.0, np.abs(qtb).max()), f"b off {boff}: |d(Q'b)[n:m]| = {et:.2e}"
            assert_guards_intact(bg, f"b (off {boff})")
        assert np.array_equal(G.bits(), bits[0]) and np.array_equal(al.bits(), bits[1]), "the solve wrote into A or alpha"

    try:
        each_layout(m, run)
    finally:
        ctx.close()


def test_apply_q_form_r0_and_residual_on_guarded_layouts(pkg, orc):
    """dhqr_apply_q_f64 (both directions), dhqr_form_r0_f64 and dhqr_residual_f64 on a padded / offset factor with a
    right-hand side, an R buffer and an original matrix whose leading dimensions are not m either"""
    L = pkg._lib.lib()
    ctx = pkg.get_context(0)
    m, n, nrhs = 1000, 333, 5
    A0, Ho, ao = _oracle(orc, m, n, 9)
    B0 = orc.rand_matrix(m, nrhs, 10)
    QtB = np.stack([_qtb(Ho, B0[:, k]) for k in range(nrhs)], axis=1)
    R0 = np.zeros((m, n))
    R0[:n] = np.triu(Ho[:n], 1) + np.diag(ao)

    def run(lda, off):
        G = guarded_matrix(m, n, lda, off, device=DEV, content=Ho)
        al = guarded_vector(n, off, device=DEV, content=ao)
        bits = (G.bits().copy(), al.bits().copy())
        B = guarded_matrix(m, nrhs, lda + 3, off, device=DEV, content=B0)
        ctx.use_torch_stream()
        pkg._lib.check(L.dhqr_apply_q_f64(ctx.handle, P(G.ptr), m, n, lda, P(B.ptr), nrhs, B.ld, 1))
        ctx.synchronize()
        e = np.abs(B.host() - QtB).max()
        assert e <= 1e-12 * np.abs(QtB).max(), f"Q'B: {e:.2e}"
        pkg._lib.check(L.dhqr_apply_q_f64(ctx.handle, P(G.ptr), m, n, lda, P(B.ptr), nrhs, B.ld, 0))
        ctx.synchronize()
        e = np.abs(B.host() - B0).max()
        assert e <= 1e-12 * np.abs(B0).max(), f"Q(Q'B) - B: {e:.2e}"
        assert_guards_intact(B, "B")
        W = guarded_matrix(m, n, lda + 1, off, device=DEV)
        pkg._lib.check(L.dhqr_form_r0_f64(ctx.handle, P(G.ptr), m, n, lda, P(al.ptr), P(W.ptr), W.ld, 128, 1, 0))
        ctx.synchronize()
        assert np.array_equal(W.host(), R0), "[R; 0] differs"
        assert_guards_intact(W, "[R; 0]")
        Ao = guarded_matrix(m, n, lda + 5, off, device=DEV, content=A0)
        work = guarded_matrix(m, n, m, 0, device=DEV)  # the work matrix has leading dimension m (include/dhqr.h)
        rel = ctypes.c_double()
        pkg._lib.check(L.dhqr_residual_f64(ctx.handle, P(G.ptr), m, n, lda, P(al.ptr), P(Ao.ptr), Ao.ld, P(work.ptr),
                                           ctypes.byref(rel)))
        assert rel.value < 1e-12, f"||A - QR|| / ||A|| = {rel.value:.2e}"
        assert_guards_intact(Ao, "original A")
        assert_guards_intact(work, "residual work")
        assert np.array_equal(G.bits(), bits[0]) and np.array_equal(al.bits(), bits[1]), "the factor was written"

    each_layout(m, run)


@pytest.mark.parametrize("m,n", [(8192, 1024), (4097, 300)])
def test_row_split_single_rank_on_guarded_layouts(pkg, orc, m, n):
    """dhqr_rs_* at world size 1 on a padded / offset local block (the Q'b pass chooses its operand width from lda, the
    block's rows, its first global row and both pointers, csrc/dhqr_rowsplit.h), with b and x offset too"""
    import torch
    L = pkg._lib.lib()
    A0, Ho, ao = _oracle(orc, m, n, 41)
    b = orc.rand_vector(m, 42)
    xo = orc.solve(Ho, ao, b)
    comm = pkg.Communicator.from_torch(pkg.get_context(0))

    def run(lda, off):
        G = guarded_matrix(m, n, lda, off, device=DEV, content=A0)
        al = guarded_vector(n, off, device=DEV)
        torch.cuda.synchronize()
        pkg._lib.check(L.dhqr_rs_factor_f64(comm.handle, P(G.ptr), m, n, lda, P(al.ptr)))
        torch.cuda.synchronize()
        _check_factor(G, al, Ho, ao)
        Bw, A0w = pkg.empty_colmajor(m, n, DEV), pkg.empty_colmajor(m, n, DEV)
        rel = ctypes.c_double()
        pkg._lib.check(L.dhqr_rs_residual_f64(comm.handle, P(G.ptr), m, n, lda, P(al.ptr), 41, P(Bw.data_ptr()),
                                              P(A0w.data_ptr()), ctypes.byref(rel)))
        assert rel.value < 1e-12, f"||A - QR|| / ||A|| = {rel.value:.2e}"
        del Bw, A0w
        bg = guarded_vector(m, off, device=DEV, content=b)
        xg = guarded_vector(n, off, device=DEV)
        torch.cuda.synchronize()
        pkg._lib.check(L.dhqr_rs_solve_f64(comm.handle, P(G.ptr), m, n, lda, P(al.ptr), P(bg.ptr), P(xg.ptr)))
        torch.cuda.synchronize()
        ex = np.abs(xg.host() - xo).max()
        assert ex <= 1e-9 * np.abs(xo).max(), f"|dx| = {ex / np.abs(xo).max():.2e} relative"
        for g, what in ((G, "A"), (al, "alpha"), (bg, "b"), (xg, "x")):
            assert_guards_intact(g, what)

    try:
        each_layout(m, run)
    finally:
        comm.close()


@pytest.mark.parametrize("nb", [0, 64])
@pytest.mark.parametrize("m,n", [(300, 200), (1100, 1000)])
def test_complex_on_guarded_layouts(pkg, orc, m, n, nb):
    """ComplexF64 with lda = m + 1 complex elements and a base one complex element in: both 16-byte aligned, so they must
    work (unblocked and blocked through the real embedding, and the solve).  A base 8 bytes off is DHQR_EINVAL, leaves
    the buffer bit for bit as it was, and the next call on the same context succeeds."""
    L = pkg._lib.lib()
    ctx = pkg.get_context(0)
    A0 = orc.rand_matrix_c(m, n, 8)
    Ho, ao = orc.householder_c(A0)
    b = orc.rand_vector_c(m, 9)
    xo = orc.solve_c(Ho, ao, b)
    c128 = np.complex128

    def run(lda, off):
        G = guarded_matrix(m, n, lda, off, dtype=c128, device=DEV, content=A0)
        al = guarded_vector(n, off, dtype=c128, device=DEV)
        bits = G.bits().copy()
        ctx.use_torch_stream()
        assert L.dhqr_factor_c64_nb(ctx.handle, P(G.ptr + 8), m, n, lda, P(al.ptr), nb) == pkg._lib.EINVAL
        assert b"16-byte" in L.dhqr_last_error()
        ctx.synchronize()
        assert np.array_equal(G.bits(), bits), "a rejected call changed the matrix"
        pkg._lib.check(L.dhqr_factor_c64_nb(ctx.handle, P(G.ptr), m, n, lda, P(al.ptr), nb))
        ctx.synchronize()
        _check_factor(G, al, Ho, ao)
        bg = guarded_vector(m, off, dtype=c128, device=DEV, content=b)
        pkg._lib.check(L.dhqr_solve_c64(ctx.handle, P(G.ptr), m, n, lda, P(al.ptr), P(bg.ptr)))
        ctx.synchronize()
        ex = np.abs(bg.host()[:n] - xo).max()
        assert ex <= 1e-9 * np.abs(xo).max(), f"|dx| = {ex / np.abs(xo).max():.2e} relative"
        for g, what in ((G, "A"), (al, "alpha"), (bg, "b")):
            assert_guards_intact(g, what)

    each_layout(m, run, [("control", (0, 0)), ("lda+1_off1", (1, 1))])


@pytest.mark.parametrize("nb", [0, 128])
@pytest.mark.parametrize("m,n", [(1100, 1000), (2207, 2000)])
def test_host_entry_points_on_guarded_layouts(pkg, orc, m, n, nb):
    """dhqr_qr_f64 / dhqr_ldiv_f64 (general route) on host arrays with lda = m + 5, aligned or 8 bytes off: in place
    within the window, hb untouched, x against the oracle, every host guard intact"""
    L = pkg._lib.lib()
    ctx = pkg.get_context(0)
    A0, Ho, ao = _oracle(orc, m, n, 12)
    b = orc.rand_vector(m, 13)
    xo = orc.solve(Ho, ao, b)

    def run(lda, off):
        G = guarded_matrix(m, n, lda, off, content=A0)
        al = guarded_vector(n, off)
        pkg._lib.check(L.dhqr_qr_f64(ctx.handle, P(G.ptr), m, n, lda, P(al.ptr), nb))
        _check_factor(G, al, Ho, ao)
        bg = guarded_vector(m, off, content=b)
        xg = guarded_vector(n, off)
        pkg._lib.check(L.dhqr_ldiv_f64(ctx.handle, P(G.ptr), m, n, lda, P(al.ptr), P(bg.ptr), P(xg.ptr)))
        assert np.array_equal(bg.view, b), "H \\ b modified b"
        ex = np.abs(xg.view - xo).max()
        assert ex <= 1e-9 * np.abs(xo).max(), f"|dx| = {ex / np.abs(xo).max():.2e} relative"
        for g, what in ((G, "A"), (al, "alpha"), (bg, "b"), (xg, "x")):
            assert_guards_intact(g, what)

    each_layout(m, run, [("lda+5", (5, 0)), ("lda+5_off1", (5, 1))])
