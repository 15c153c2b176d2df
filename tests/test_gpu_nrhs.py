"""`H \\ B` with several right-hand sides on the MI355X through api.py (ldiv, H.solve, solve_householder_ with a matrix B) and
the C ABI (dhqr_solve_batched_nrhs_* / dhqr_ldiv_batched_nrhs_*): every column bit for bit against today's single-column
call on every route, against the oracle, B untouched, padded / strided / guarded layouts, launch groups, arguments, host
against device, repeatability."""
import ctypes

import numpy as np
import pytest

import f32_helpers as F
import layout_helpers as LH
import nrhs_helpers as N
from nrhs_helpers import NBatch, same_bytes

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p


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


def _dev_inputs(pkg, torch, m, n, nrhs, batch, seed, t):
    """(A (batch, m, n), B (batch, m, nrhs)), matrices column-major: N.inputs' values from the device generator.  Column r of
    B_k is the vector of seed + 5000 + 1000 r + k, i.e. column 0 of matrix k + 1000 r: one fill serves every column of a large batch"""
    A = pkg.rand_colmajor_batched(batch, m, n, seed, "cuda:0", dtype=_tdt(torch, t))
    B = pkg.empty_colmajor_batched(batch, m, nrhs, "cuda:0", dtype=_tdt(torch, t))
    if batch >= 1000:
        V = pkg.rand_colmajor_batched(batch + 1000 * (nrhs - 1), m, 1, seed + 5000, "cuda:0", dtype=_tdt(torch, t)).reshape(-1, m)
    for r in range(nrhs):
        if batch >= 1000:
            B[:, :, r] = V[1000 * r: 1000 * r + batch]
        else:
            B[:, :, r] = pkg.rand_colmajor_batched(batch, m, 1, seed + 5000 + 1000 * r, "cuda:0", dtype=_tdt(torch, t)).reshape(batch, m)
    return A, B


def _single_columns(pkg, H, B):
    """today's call, column by column: ldiv_batched on the vectors B[:, :, r] -> list of (batch, n)"""
    return [pkg.ldiv_batched(H, B[:, :, r].contiguous()) for r in range(B.shape[2])]


def _check_oracle(orc, t, m, n, mats, Bs, Hh, alh, Xh, what):
    """criterion 2 for the matrices given: Float64 against the oracle's own factor and solve (1e-9, the twin first), Float32
    F.check_solve on the kernel's own factor"""
    if t == "f64":
        worst, twin = N.oracle_errors(orc, mats, Bs, [x.astype(np.float64) for x in Xh])
        print(f"{what} {m}x{n}: {len(mats)} matrices x {Bs[0].shape[1]} columns vs oracle: |dx|/|x| = {worst:.2e}, twin {twin:.2e} (tol 1e-9)")
        assert twin <= 1e-9, "the numpy twin misses the bound at these seeds: change the seed"
        assert worst <= 1e-9
    else:
        for r in range(Bs[0].shape[1]):
            F.check_solve(orc, Hh, alh, np.stack([B[:, r] for B in Bs]), np.stack([x[:, r] for x in Xh]), range(len(mats)),
                          f"{what} column {r}")


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n", N.WAVE_SHAPES)
def test_wave_tier(pkg, orc, torch_cuda, small_route, m, n, t):
    """criteria 1, 2, 3 and the result's form on the wave tier: batch 1, 5, 300 x nrhs 1, 3, 4, 5, 9 (and 8, 13: N.NRHS_KERNEL_TAILS) -- the same column has
    the same bytes in every call, those of ldiv_batched on that column alone; a single matrix (2-D B) is a batch of 1"""
    torch = torch_cuda
    batch, nrhs = 300, N.NRHS_MAX
    A, B = _dev_inputs(pkg, torch, m, n, nrhs, batch, N.SEED, t)
    B0 = B.clone()
    H = pkg.qr_batched_(A)
    cols = _single_columns(pkg, H, B)
    for nb in N.BATCHES:
        Hs = pkg.DistributedHouseholderQRStruct(H.A[:nb], H.α[:nb])
        for k in N.NRHS_ALL:
            X = pkg.ldiv(Hs, B[:nb, :, :k])
            assert tuple(X.shape) == (nb, n, k) and X.dtype == A.dtype
            assert X.stride(1) == 1 and (k == 1 or X.stride(2) == n)
            for r in range(k):
                assert torch.equal(X[:, :, r], cols[r][:nb]), f"batch {nb} nrhs {k} column {r}"
    H1 = pkg.DistributedHouseholderQRStruct(H.A[7], H.α[7])
    for k in N.NRHS_ALL:
        X1 = H1.solve(B[7][:, :k])
        assert tuple(X1.shape) == (n, k) and X1.dtype == A.dtype and X1.stride(0) == 1 and (k == 1 or X1.stride(1) == n)
        for r in range(k):
            assert torch.equal(X1[:, r], cols[r][7]), f"single matrix, nrhs {k} column {r}"
    assert torch.equal(B, B0), "H \\ B must not modify B (src:318)"
    mats, Bs = N.inputs(orc, m, n, nrhs, batch, N.SEED, t)
    assert same_bytes(B[:3].cpu().numpy(), np.stack(Bs[:3])), "the device generator, column by column"
    Xh = pkg.ldiv(H, B).cpu().numpy()
    _check_oracle(orc, t, m, n, mats, Bs, H.A.cpu().numpy(), H.α.cpu().numpy(), list(Xh), "wave tier")


@pytest.mark.parametrize("nrhs", [5, 9])
@pytest.mark.parametrize("t", N.DTYPES)
def test_wave_tier_large_batch(pkg, orc, torch_cuda, small_route, t, nrhs):
    """(16, 8), nrhs = 5, batch 20000: more workgroups than fit at once; every column of every matrix against the single-column
    call, the oracle at every 97th matrix.  (nrhs = 5 takes the column loop, dhqr.h; nrhs = 9 is the multi-column kernel.)"""
    torch = torch_cuda
    m, n, batch = 16, 8, 20000
    A, B = _dev_inputs(pkg, torch, m, n, nrhs, batch, N.SEED, t)
    H = pkg.qr_batched_(A)
    X = pkg.ldiv(H, B)
    for r, c in enumerate(_single_columns(pkg, H, B)):
        assert torch.equal(X[:, :, r], c), r
    ks = list(range(0, batch, 97))
    mats, Bs = N.inputs(orc, m, n, nrhs, batch, N.SEED, t, ks=ks)
    assert same_bytes(B[ks].cpu().numpy(), np.stack(Bs))
    _check_oracle(orc, t, m, n, mats, Bs, H.A[ks].cpu().numpy(), H.α[ks].cpu().numpy(), list(X[ks].cpu().numpy()), "large batch")


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n,batch", N.BEYOND)
def test_beyond_the_wave_tier(pkg, orc, torch_cuda, small_route, m, n, batch, t):
    """criteria 1, 2, 5 on the one-workgroup tier and the serial tier, nrhs = 3: the bytes of ldiv_batched on each column (and
    of ldiv on the vector, for a single matrix), the profiling counts of three single calls"""
    torch = torch_cuda
    ctx = small_route
    nrhs = 3
    A, B = _dev_inputs(pkg, torch, m, n, nrhs, batch, N.SEED, t)
    B0 = B.clone()
    H = pkg.qr_batched_(A, nb=0)
    ctx.reset_stats()
    ctx.set_profiling(True)
    try:
        cols = _single_columns(pkg, H, B)
        singles = ctx.stats()["n_solve"]
        ctx.reset_stats()
        X = pkg.ldiv(H, B)
        assert ctx.stats()["n_solve"] == singles
        if m <= 256:
            assert singles == 3
    finally:
        ctx.set_profiling(False)
    assert tuple(X.shape) == (batch, n, nrhs)
    for r in range(nrhs):
        assert torch.equal(X[:, :, r], cols[r]), r
    H1 = pkg.DistributedHouseholderQRStruct(H.A[1], H.α[1])
    X1 = pkg.ldiv(H1, B[1])
    for r in range(nrhs):
        assert torch.equal(X1[:, r], pkg.ldiv(H1, B[1][:, r].contiguous())), f"single matrix column {r}"
        assert torch.equal(X1[:, r], cols[r][1])
    assert torch.equal(B, B0)
    mats, Bs = N.inputs(orc, m, n, nrhs, batch, N.SEED, t)
    _check_oracle(orc, t, m, n, mats, Bs, H.A.cpu().numpy(), H.α.cpu().numpy(), list(X.cpu().numpy()), "beyond the wave tier")


@pytest.mark.parametrize("t", N.DTYPES)
def test_small_route_off(pkg, orc, torch_cuda, t):
    """(the suite's default context: DHQR_SMALL=0) every shape is the column loop over the serial tier"""
    torch = torch_cuda
    A, B = _dev_inputs(pkg, torch, 16, 8, 3, 2, N.SEED, t)
    H = pkg.qr_batched_(A)
    X = pkg.ldiv(H, B)
    for r, c in enumerate(_single_columns(pkg, H, B)):
        assert torch.equal(X[:, :, r], c)


@pytest.mark.parametrize("t", N.DTYPES)
def test_launch_groups(pkg, orc, torch_cuda, small_route, t):
    """criterion 5: wave tier, nrhs = 9, batch 7: exactly one n_solve; one-workgroup tier, nrhs = 3: three"""
    torch = torch_cuda
    ctx = small_route
    for (m, n, nrhs, want) in ((16, 8, 9, 1), (66, 33, 3, 3)):
        A, B = _dev_inputs(pkg, torch, m, n, nrhs, 7, 1, t)
        H = pkg.qr_batched_(A)
        ctx.reset_stats()
        ctx.set_profiling(True)
        try:
            pkg.ldiv(H, B)
            assert ctx.stats()["n_solve"] == want, (m, n)
        finally:
            ctx.set_profiling(False)


def _upload(torch, D):
    return {k: torch.from_numpy(getattr(D, k).copy()).to("cuda:0") for k in ("A", "al", "B")}


def _dev_ptrs(dev):
    return dict(A=P(dev["A"].data_ptr()), al=P(dev["al"].data_ptr()), B=P(dev["B"].data_ptr()))


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n", [(16, 8), (40, 17), (66, 33)])
def test_strided_batches_through_the_c_abi(pkg, orc, torch_cuda, small_route, m, n, t):
    """criteria 3, 4, 7: a batch in sentinel-filled buffers (ldb = m + 1 and m + 3, strideB > ldb nrhs, ldx > n): the device
    form writes the windows of B and nothing else, the host form leaves hB bit-identical and returns the device form's X"""
    torch = torch_cuda
    ctx = small_route
    L = pkg._lib.lib()
    nrhs, batch = 9, 5  # (the multi-column kernel on the wave tier: N.NRHS_KERNEL_TAILS)
    mats, Bs = N.inputs(orc, m, n, nrhs, batch, N.SEED, t)
    Ad, Bd = _dev_inputs(pkg, torch, m, n, nrhs, batch, N.SEED, t)
    H = pkg.qr_batched_(Ad)
    want = pkg.ldiv(H, Bd).cpu().numpy()
    Hh, alh = H.A.cpu().numpy(), H.α.cpu().numpy()
    for pad_ldb in (1, 3):
        D = NBatch(list(Hh), Bs, t, pad_ldb=pad_ldb)
        for k in range(batch):
            D.alpha(k)[...] = alh[k]
        A0, B0 = D.A.copy(), D.B.copy()
        pkg._lib.check(D.ldiv_nrhs(L, ctx.handle))
        assert same_bytes(D.B, B0) and same_bytes(D.A, A0), "the host form must not modify its inputs"
        for k in range(batch):
            assert same_bytes(D.xmat(k), want[k]), k
        assert D.padding_intact()
        dev = _upload(torch, D)
        torch.cuda.synchronize()
        pkg._lib.check(D.solve_nrhs(L, ctx.handle, **_dev_ptrs(dev)))
        ctx.synchronize()
        assert same_bytes(dev["A"].cpu().numpy(), A0)
        D.B[...] = dev["B"].cpu().numpy()
        for k in range(batch):
            assert same_bytes(D.bmat(k)[:n], want[k]), k
        assert D.padding_intact()


@pytest.mark.parametrize("t", N.DTYPES)
def test_guarded_layouts(pkg, orc, torch_cuda, small_route, t):
    """criterion 4 on NaN-guarded device and host buffers, one matrix: ldb = m + 1 and m + 3, ldx > n, a base one element off
    (Float32: 4 bytes off an 8-byte boundary).  Every guard word intact; the device form leaves the tail of Q'B below X
    (Float64: against apply_q_, 1e-12 of max|Q'B| as in test_emulated_batched)"""
    torch = torch_cuda
    ctx = small_route
    L = pkg._lib.lib()
    m, n, nrhs = 33, 9, 9
    A, B = _dev_inputs(pkg, torch, m, n, nrhs, 1, N.SEED, t)
    H = pkg.qr_batched_(A)
    H1 = pkg.DistributedHouseholderQRStruct(H.A[0], H.α[0])
    want = pkg.ldiv(H1, B[0])
    Bh, Hh, alh = B[0].cpu().numpy(), H.A[0].cpu().numpy(), H.α[0].cpu().numpy()
    if t == "f64":
        guarded, intact = (lambda r, c, ld, off, content, device=None: LH.guarded_matrix(r, c, ld, off, content=content, device=device)), LH.assert_guards_intact
    else:
        guarded, intact = (lambda r, c, ld, off, content, device=None: F.guarded_f32(r, c, ld, off, device=device, content=content)), F.assert_f32_guards_intact
    solve, ldiv = getattr(L, f"dhqr_solve_batched_nrhs_{t}"), getattr(L, f"dhqr_ldiv_batched_nrhs_{t}")
    for pad, off in ((1, 0), (3, 0), (1, 1), (3, 1)):
        sB, sX = (m + pad) * (nrhs - 1) + m, (n + pad) * (nrhs - 1) + n
        gB = guarded(m, nrhs, m + pad, off, Bh, "cuda:0")
        W = gB.view
        assert W.stride() == (1, m + pad)
        X = pkg.solve_householder_(W, H1.A, H1.α)  # overwrites the device B
        assert torch.equal(X, want) and torch.equal(W[:n], want)
        intact(gB, f"device B (pad {pad}, off {off})")
        if t == "f64" and m > n:
            Q = pkg.empty_colmajor(m, nrhs, "cuda:0")
            Q.copy_(B[0])
            pkg.apply_q_(H1, Q, trans=True)
            assert (W[n:] - Q[n:]).abs().max().item() <= 1e-12 * max(1.0, Q.abs().max().item())
        gB2 = guarded(m, nrhs, m + pad, off, Bh, "cuda:0")
        pkg._lib.check(solve(ctx.handle, P(H.A.data_ptr()), m, n, m, m * n, P(H.α.data_ptr()), n, P(gB2.ptr), nrhs, m + pad, sB, 1))
        ctx.synchronize()
        assert torch.equal(gB2.view, W)
        intact(gB2, f"device B through the C ABI (pad {pad}, off {off})")
        hA, hal = guarded(m, n, m + pad, off, Hh), guarded(n, 1, n, off, alh.reshape(n, 1))
        hB, hX = guarded(m, nrhs, m + pad, off, Bh), guarded(n, nrhs, n + pad, off, None)
        pkg._lib.check(ldiv(ctx.handle, P(hA.ptr), m, n, m + pad, (m + pad) * (n - 1) + m, P(hal.ptr), n, P(hB.ptr), nrhs, m + pad,
                            sB, P(hX.ptr), n + pad, sX, 1))
        assert same_bytes(hB.host(), Bh) and same_bytes(hX.host(), want.cpu().numpy())
        for g, what in ((hA, "hA"), (hal, "halpha"), (hB, "hB"), (hX, "hX")):
            intact(g, f"{what} (pad {pad}, off {off})")


@pytest.mark.parametrize("t", N.DTYPES)
def test_host_equals_device(pkg, orc, torch_cuda, small_route, t):
    """criteria 3 and 7: numpy inputs, B column-major and row-major, single and batched, give the device call's bytes; the
    caller's B is left as it was"""
    torch = torch_cuda
    for (m, n, batch) in ((16, 8, 5), (40, 17, 5), (66, 33, 3)):
        nrhs = 9
        A, B = _dev_inputs(pkg, torch, m, n, nrhs, batch, N.SEED, t)
        H = pkg.qr_batched_(A)
        want = pkg.ldiv(H, B).cpu().numpy()
        Hh = pkg.DistributedHouseholderQRStruct(H.A.cpu().numpy(), H.α.cpu().numpy())
        Bn = B.cpu().numpy()
        for Bx in (Bn, np.ascontiguousarray(Bn)):  # matrices column-major | row-major (C order)
            keep = Bx.copy()
            X = pkg.ldiv(Hh, Bx)
            assert isinstance(X, np.ndarray) and X.shape == (batch, n, nrhs) and X.dtype == Bn.dtype
            assert X.strides[1] == X.itemsize and same_bytes(X, want) and same_bytes(Bx, keep)
        H1 = pkg.DistributedHouseholderQRStruct(np.asfortranarray(Hh.A[2]), Hh.α[2].copy())
        for Bx in (np.asfortranarray(Bn[2]), np.ascontiguousarray(Bn[2])):
            keep = Bx.copy()
            X = H1.solve(Bx)
            assert X.shape == (n, nrhs) and X.dtype == Bn.dtype and X.flags.f_contiguous
            assert same_bytes(X, want[2]) and same_bytes(Bx, keep)
            assert same_bytes(pkg.solve_householder_(Bx, H1.A, H1.α), want[2]) and same_bytes(Bx, keep), "a host B is never written"


def test_python_arguments(pkg, orc, torch_cuda, small_route):
    """criterion 6 at the Python front end: dtype and layout rules, the ComplexF64 refusal, empty right-hand sides"""
    torch = torch_cuda
    m, n = 16, 8
    A, B = _dev_inputs(pkg, torch, m, n, 3, 4, N.SEED, "f64")
    H = pkg.qr_batched_(A)
    H1 = pkg.DistributedHouseholderQRStruct(H.A[0], H.α[0])
    A32, B32 = _dev_inputs(pkg, torch, m, n, 3, 4, N.SEED, "f32")
    H32 = pkg.qr_batched_(A32)
    with pytest.raises(TypeError):
        pkg.ldiv(H, B32)
    with pytest.raises(TypeError):
        pkg.ldiv(H32, B)
    with pytest.raises(TypeError):
        pkg.ldiv(H1, B32[0])
    with pytest.raises(TypeError):
        pkg.ldiv(pkg.DistributedHouseholderQRStruct(H32.A[0], H32.α[0]), B[0])
    with pytest.raises(ValueError):
        pkg.ldiv(H, B.contiguous())  # row-major matrices
    with pytest.raises(ValueError):
        pkg.ldiv(H1, B[0].contiguous())
    with pytest.raises((TypeError, ValueError)):
        pkg.ldiv(H, B[:, :m - 1, :])  # row mismatch
    with pytest.raises(ValueError):
        pkg.ldiv(H1, B[0][:m - 1])
    Hc = pkg.qr_(pkg.rand_colmajor_c(m, n, 3, "cuda:0"))
    with pytest.raises(TypeError, match="ComplexF64: vector right-hand side only"):
        pkg.ldiv(Hc, torch.zeros((m, 2), dtype=torch.complex128, device="cuda:0"))
    X = pkg.ldiv(H, B[:, :, :0])
    assert tuple(X.shape) == (4, n, 0)
    X = pkg.ldiv(H1, B[0][:, :0])
    assert tuple(X.shape) == (n, 0)
    # a vector goes where it went: (batch, m) and (m,)
    assert tuple(pkg.ldiv(H, B[:, :, 0].contiguous()).shape) == (4, n) and tuple(pkg.ldiv(H1, B[0][:, 0].contiguous()).shape) == (n,)


@pytest.mark.parametrize("t", N.DTYPES)
def test_c_abi_arguments_on_device_pointers(pkg, orc, torch_cuda, small_route, t):
    """criterion 6 at the C ABI with real device and host memory: every DHQR_EINVAL case and every no-op on the device and
    the host form, nothing touched"""
    torch = torch_cuda
    ctx = small_route
    L = pkg._lib.lib()
    m, n, nrhs, batch = 12, 6, 3, 3
    mats, Bs = N.inputs(orc, m, n, nrhs, batch, N.SEED, t)
    D = NBatch(mats, Bs, t)
    dev = _upload(torch, D)
    torch.cuda.synchronize()
    dp = _dev_ptrs(dev)
    before = [b.copy() for b in (D.A, D.al, D.B, D.X)]

    def both(**kw):
        host = D.ldiv_nrhs(L, ctx.handle, **kw)
        d = dict(dp)
        d.update({k: v for k, v in kw.items() if k not in ("X", "ldx", "sX")})
        return D.solve_nrhs(L, ctx.handle, **d), host

    for noop in (dict(nrhs=0), dict(batch=0), dict(n=0), dict(nrhs=0, B=None, X=None), dict(batch=0, A=None, al=None, B=None, X=None)):
        assert both(**noop) == (0, 0), noop
    bad = [dict(nrhs=-1), dict(batch=-1), dict(m=5, n=6), dict(lda=m - 1), dict(sA=D.lda * (n - 1) + m - 1), dict(sal=n - 1),
           dict(A=None), dict(al=None), dict(B=None), dict(ldb=m - 1), dict(sB=D.ldb * (nrhs - 1) + m - 1)]
    for kw in bad:
        assert both(**kw) == (N.EINVAL, N.EINVAL), kw
    for kw in (dict(X=None), dict(ldx=n - 1), dict(sX=D.ldx * (nrhs - 1) + n - 1)):
        assert D.ldiv_nrhs(L, ctx.handle, **kw) == N.EINVAL, kw
    ctx.synchronize()
    for got, want in zip((D.A, D.al, D.B, D.X), before):
        assert same_bytes(got, want), "a rejected or empty call must not touch anything"
    for k, want in zip(("A", "al", "B"), before):
        assert same_bytes(dev[k].cpu().numpy(), want), "a rejected or empty call must not touch device memory"


@pytest.mark.parametrize("t", N.DTYPES)
def test_repeatability(pkg, orc, torch_cuda, small_route, monkeypatch, t):
    """criterion 8: five calls on (40, 17), nrhs = 5 give identical bytes, the fifth on a fresh Context"""
    torch = torch_cuda
    m, n, nrhs, batch = 40, 17, 5, 300
    A, B = _dev_inputs(pkg, torch, m, n, nrhs, batch, N.SEED, t)
    H = pkg.qr_batched_(A)
    first = pkg.ldiv(H, B)
    for i in range(3):
        assert torch.equal(pkg.ldiv(H, B), first), i
    monkeypatch.setenv("DHQR_SMALL", "1")
    ctx = pkg.Context(0)
    try:
        W = B.clone(memory_format=torch.preserve_format)
        assert W.stride() == B.stride()
        torch.cuda.synchronize()
        solve = getattr(pkg._lib.lib(), f"dhqr_solve_batched_nrhs_{t}")
        pkg._lib.check(solve(ctx.handle, P(H.A.data_ptr()), m, n, m, m * n, P(H.α.data_ptr()), n, P(W.data_ptr()), nrhs, m,
                             m * nrhs, batch))
        ctx.synchronize()
        assert torch.equal(W[:, :n, :], first)
    finally:
        ctx.close()
