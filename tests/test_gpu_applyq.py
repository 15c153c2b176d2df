"""Q application, explicit Q and R for batches and Float32 on the MI355X through api.py (apply_q_, get_q, get_r on a
(batch, m, n) factor of either real type and on one float32 matrix): the tail of Q'B bit for bit against the multi-column
solve, every column independent of nrhs, place and batch, both directions against reflectors applied in np.longdouble, Q
and R, a NaN reflector that stays in its matrix, batch 300 against the single-matrix calls, the blocked route beyond the
wave tier, one guarded layout through the C ABI."""
import ctypes

import numpy as np
import pytest

import applyq_helpers as Q
import f32_helpers as F
import layout_helpers as LH
import nrhs_helpers as N

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
NRHS_MAX = max(N.NRHS_KERNEL_TAILS + [9])
CASES = [(b, k) for b in N.BATCHES for k in (4, 9)] + [(5, k) for k in N.NRHS_KERNEL_TAILS]  # (batch, nrhs)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture
def small_route(pkg):
    """the product default on the shared context for one test (conftest.py switches it off for the suite)"""
    ctx = pkg.get_context(0)
    ctx.set_small_route(True)
    yield ctx
    ctx.set_small_route(False)


def _tdt(torch, t):
    return torch.float32 if t == "f32" else torch.float64


def _dev_inputs(pkg, torch, m, n, nrhs, batch, t):
    """(A (batch, m, n), B (batch, m, nrhs)), matrices column-major: N.inputs' values from the device generator"""
    A = pkg.rand_colmajor_batched(batch, m, n, N.SEED, "cuda:0", dtype=_tdt(torch, t))
    B = pkg.empty_colmajor_batched(batch, m, nrhs, "cuda:0", dtype=_tdt(torch, t))
    for r in range(nrhs):
        B[:, :, r] = pkg.rand_colmajor_batched(batch, m, 1, N.SEED + 5000 + 1000 * r, "cuda:0", dtype=_tdt(torch, t)).reshape(batch, m)
    return A, B


def _colmajor_copy(pkg, X):
    W = pkg.empty_colmajor_batched(X.shape[0], X.shape[1], X.shape[2], X.device, X.dtype)
    W.copy_(X)
    return W


def _sub(pkg, H, batch):
    return pkg.DistributedHouseholderQRStruct(H.A[:batch], H.α[:batch])


def _eye(pkg, torch, batch, m, n, t):
    E = pkg.empty_colmajor_batched(batch, m, n, "cuda:0", _tdt(torch, t))
    E.zero_()
    E.diagonal(dim1=1, dim2=2).fill_(1.0)
    return E


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n", Q.GPU_SHAPES)
def test_wave_tier(pkg, torch_cuda, small_route, m, n, t):
    """criteria 1, 2 and 3 on the wave tier.  Batch 1, 5, 300 x nrhs 4, 9 (and 8, 13 at batch 5): every column of Q'B and QB
    has the bytes of the nrhs = 1 call on that column (taken once, at batch 300); rows n .. m-1 of Q'B have the bytes of the
    same rows after dhqr_solve_batched_nrhs_* on a copy.  Both directions against np.longdouble reflectors on the kernel's own
    factor, Q'(QB) = B, R with the bytes of alpha and H, Q'Q = I, QR = A, get_q equal to Q [I; 0]; a single float32 matrix
    is a batch of one."""
    torch = torch_cuda
    ctx, L = small_route, pkg._lib.lib()
    batch = max(N.BATCHES)
    A, B = _dev_inputs(pkg, torch, m, n, NRHS_MAX, batch, t)
    A0 = A.clone()
    H = pkg.qr_batched_(A)
    alone = {tr: torch.cat([pkg.apply_q_(H, _colmajor_copy(pkg, B[:, :, r:r + 1]), bool(tr)) for r in range(NRHS_MAX)], dim=2)
             for tr in (1, 0)}
    solve = getattr(L, f"dhqr_solve_batched_nrhs_{t}")
    for b, nrhs in CASES:
        Hb = _sub(pkg, H, b)
        for tr in (1, 0):
            W = pkg.apply_q_(Hb, _colmajor_copy(pkg, B[:b, :, :nrhs]), bool(tr))
            assert torch.equal(W, alone[tr][:b, :, :nrhs]), f"batch {b} nrhs {nrhs} trans {tr}"
        S = _colmajor_copy(pkg, B[:b, :, :nrhs])
        pkg._lib.check(solve(ctx.handle, P(H.A.data_ptr()), m, n, m, m * n, P(H.α.data_ptr()), n, P(S.data_ptr()), nrhs, m, m * nrhs, b))
        ctx.synchronize()
        assert torch.equal(S[:, n:], alone[1][:b, n:, :nrhs]), f"batch {b} nrhs {nrhs}: the tail of Q'B"
    # accuracy, on the host, for the first five matrices
    Hh, alh, Bh, A0h = H.A[:5].cpu().numpy(), H.α[:5].cpu().numpy(), B[:5, :, :9].cpu().numpy(), A0[:5].cpu().numpy()
    got = {tr: alone[tr][:5, :, :9].cpu().numpy() for tr in (1, 0)}
    for k in range(5):
        for tr in (1, 0):
            want = Q.reflect_longdouble(Hh[k], Bh[k], tr)
            err, scale = float(np.abs(got[tr][k] - want).max()), float(np.abs(want).max())
            print(f"{m}x{n} {t} trans {tr} matrix {k}: |d| / max|result| = {err / scale:.2e} (tol {Q.tol(t):.2e})")
            assert err <= Q.tol(t) * scale
    back = pkg.apply_q_(_sub(pkg, H, 5), _colmajor_copy(pkg, alone[0][:5, :, :9]), True).cpu().numpy()
    for k in range(5):
        assert np.abs(back[k].astype(np.float64) - Bh[k]).max() <= Q.tol(t) * np.abs(Bh[k]).max()
    # Q and R
    Qd, Rd = pkg.get_q(H), pkg.get_r(H)
    assert tuple(Qd.shape) == (batch, m, n) and tuple(Rd.shape) == (batch, n, n) and Qd.stride(1) == 1 and Rd.stride(1) == 1
    assert torch.equal(Qd, pkg.apply_q_(H, _eye(pkg, torch, batch, m, n, t), False)), "get_q != Q [I; 0]"
    Qh, Rh = Qd[:5].cpu().numpy(), Rd[:5].cpu().numpy()
    for k in range(5):
        Q.check_r(Rh[k], Hh[k], alh[k])
        Q.check_qr(Qh[k], Rh[k], A0h[k], t, f"{m}x{n} {t} matrix {k}")
    if t == "f32":
        H1 = pkg.DistributedHouseholderQRStruct(H.A[0], H.α[0])
        W = pkg.empty_colmajor(m, 9, "cuda:0", dtype=torch.float32)
        W.copy_(B[0, :, :9])
        assert torch.equal(pkg.apply_q_(H1, W, True), alone[1][0, :, :9])
        assert torch.equal(pkg.get_q(H1), Qd[0]) and torch.equal(pkg.get_r(H1), Rd[0])


def _all_results(pkg, torch, H, B, t):
    batch, m, n = H.A.shape
    return [pkg.apply_q_(H, _colmajor_copy(pkg, B), True), pkg.apply_q_(H, _colmajor_copy(pkg, B), False), pkg.get_q(H), pkg.get_r(H)]


@pytest.mark.parametrize("t", N.DTYPES)
def test_matrices_are_independent(pkg, torch_cuda, small_route, t):
    """criterion 5: a NaN reflector (a zero column in matrix 2 of a batch of 5, (16, 8)) stays in its matrix; at (5, 3) every
    matrix of a batch of 300 has the bytes of its single-matrix call -- in Q'B, QB, Q and R"""
    torch = torch_cuda
    m, n, nrhs = 16, 8, 4
    A, B = _dev_inputs(pkg, torch, m, n, nrhs, 5, t)
    Ad = A.clone()
    Ad[2, :, 3] = 0
    clean, Hd = _all_results(pkg, torch, pkg.qr_batched_(A), B, t), pkg.qr_batched_(Ad)
    assert torch.isnan(Hd.A[2]).any(), "the zero column was meant to give a NaN reflector"
    for c, d in zip(clean, _all_results(pkg, torch, Hd, B, t)):
        for k in (0, 1, 3, 4):
            assert torch.equal(c[k], d[k]), k
    m, n, batch = 5, 3, max(N.BATCHES)
    A, B = _dev_inputs(pkg, torch, m, n, nrhs, batch, t)
    H = pkg.qr_batched_(A)
    whole = _all_results(pkg, torch, H, B, t)
    for k in range(batch):
        Hk = pkg.DistributedHouseholderQRStruct(H.A[k:k + 1], H.α[k:k + 1])
        for w, o in zip(whole, _all_results(pkg, torch, Hk, B[k:k + 1], t)):
            assert torch.equal(w[k], o[0]), k


@pytest.mark.parametrize("m,n,batch", N.BEYOND)
def test_beyond_the_wave_tier_f64(pkg, torch_cuda, small_route, m, n, batch):
    """criterion 6, Float64: matrix k has the bytes of the single-matrix blocked route (apply_q_ / get_q on the 2-D factor:
    dhqr_apply_q_f64) on it alone, in both directions; R as on the wave tier"""
    torch = torch_cuda
    A, B = _dev_inputs(pkg, torch, m, n, 3, batch, "f64")
    A0 = A.clone()
    H = pkg.qr_batched_(A)
    Wt, Wn, Qd, Rd = _all_results(pkg, torch, H, B, "f64")
    for k in range(batch):
        Hk = pkg.DistributedHouseholderQRStruct(H.A[k], H.α[k])
        for W, tr in ((Wt, True), (Wn, False)):
            S = pkg.empty_colmajor(m, 3, "cuda:0")
            S.copy_(B[k])
            assert torch.equal(pkg.apply_q_(Hk, S, tr), W[k]), (k, tr)
        assert torch.equal(pkg.get_q(Hk), Qd[k]), k
        Q.check_r(Rd[k].cpu().numpy(), H.A[k].cpu().numpy(), H.α[k].cpu().numpy())
        Q.check_qr(Qd[k].cpu().numpy(), Rd[k].cpu().numpy(), A0[k].cpu().numpy(), "f64", f"{m}x{n} matrix {k}")


@pytest.mark.parametrize("t", N.DTYPES)
def test_guarded_layout(pkg, torch_cuda, small_route, t):
    """one guarded case through the C ABI, (40, 17), nrhs 9, a single matrix: lda = m + 1 and ldb = ldq = m + 3, ldr = n + 1,
    every base one element off an aligned boundary -- the packed call's bytes, the poison before, between (the padding rows)
    and behind the matrices intact"""
    torch = torch_cuda
    ctx, L = small_route, pkg._lib.lib()
    m, n, nrhs = 40, 17, 9
    A, B = _dev_inputs(pkg, torch, m, n, nrhs, 1, t)
    H = pkg.qr_batched_(A)
    want = _all_results(pkg, torch, H, B, t)
    if t == "f64":
        guarded, intact = (lambda r, c, ld, content=None: LH.guarded_matrix(r, c, ld, 1, content=content, device="cuda:0")), LH.assert_guards_intact
    else:
        guarded, intact = (lambda r, c, ld, content=None: F.guarded_f32(r, c, ld, 1, device="cuda:0", content=content)), F.assert_f32_guards_intact
    Hh, alh, Bh = H.A[0].cpu().numpy(), H.α[0].cpu().numpy(), B[0].cpu().numpy()
    gA, gal = guarded(m, n, m + 1, Hh), guarded(n, 1, n, alh.reshape(n, 1))
    sA = (m + 1) * (n - 1) + m
    apply_q, form_q, form_r = (getattr(L, f"dhqr_{k}_batched_{t}") for k in ("apply_q", "form_q", "form_r"))
    for tr in (1, 0):
        gB = guarded(m, nrhs, m + 3, Bh)
        pkg._lib.check(apply_q(ctx.handle, P(gA.ptr), m, n, m + 1, sA, P(gB.ptr), nrhs, m + 3, (m + 3) * (nrhs - 1) + m, 1, tr))
        ctx.synchronize()
        assert torch.equal(gB.view, want[1 - tr][0])
        intact(gB, f"B (trans {tr})")
    gQ, gR = guarded(m, n, m + 3), guarded(n, n, n + 1)
    pkg._lib.check(form_q(ctx.handle, P(gA.ptr), m, n, m + 1, sA, P(gQ.ptr), m + 3, (m + 3) * (n - 1) + m, 1))
    pkg._lib.check(form_r(ctx.handle, P(gA.ptr), m, n, m + 1, sA, P(gal.ptr), n, P(gR.ptr), n + 1, (n + 1) * (n - 1) + n, 1))
    ctx.synchronize()
    assert torch.equal(gQ.view, want[2][0]) and torch.equal(gR.view, want[3][0])
    for g, what in ((gA, "A"), (gal, "alpha"), (gQ, "Q"), (gR, "R")):
        intact(g, what)
