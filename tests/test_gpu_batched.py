"""Batches of small matrices on the MI355X through api.py: qr_batched_ / ldiv_batched on device tensors and host arrays --
the wave-per-matrix kernels (csrc/dhqr_batched.h) and the one-workgroup-per-matrix tier against the oracle, the latter bit
for bit against the single-matrix small route, launch counts, invariants of the factor format over large batches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
WAVE_SHAPES = [(1, 1), (5, 3), (12, 6), (16, 8), (33, 9), (40, 17), (64, 32), (32, 32)]
ONE_CU_SHAPES = [(66, 33), (70, 40), (130, 20), (110, 100), (128, 128), (220, 200), (256, 192)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture
def small_route(pkg):
    """the product default (csrc/dhqr_small.h) on the shared context for one test (conftest.py switches it off for the suite)"""
    ctx = pkg.get_context(0)
    ctx.set_small_route(True)
    yield ctx
    ctx.set_small_route(False)


def _rand_b(pkg, batch, m, seed):
    """(batch, m) device tensor, row k = the shared generator's vector of seed + k"""
    return pkg.rand_colmajor_batched(batch, m, 1, seed, "cuda:0").reshape(batch, m).contiguous()


def _invariants(torch, H, A0, n):
    """every matrix of the batch: finite, ||v_kj||^2 = 2 for every stored reflector, ||R_k||_F = ||A_k||_F"""
    tol = 8.0 * max(n, 8) * EPS
    A, al = H.A, H.α
    assert torch.isfinite(A).all() and torch.isfinite(al).all()
    v2 = torch.tril(A).pow(2).sum(dim=1)  # rows j..m-1 of column j
    assert (v2 - 2.0).abs().max().item() <= tol * 2.0
    r2 = torch.triu(A[:, :n, :], diagonal=1).pow(2).sum(dim=(1, 2)) + al.pow(2).sum(dim=1)
    a2 = A0.pow(2).sum(dim=(1, 2))
    assert ((r2.sqrt() - a2.sqrt()).abs() / a2.sqrt()).max().item() <= tol


def _against_oracle(orc, H, x, m, n, seed, ks):
    tol = 8.0 * max(n, 8) * EPS
    Ah, alh, xh = H.A.cpu().numpy(), H.α.cpu().numpy(), x.cpu().numpy()
    worst = [0.0, 0.0, 0.0]
    for k in ks:
        Ho, ao = orc.householder(orc.rand_matrix(m, n, seed + k))
        xo = orc.solve(Ho, ao, orc.rand_vector(m, seed + 5000 + k))
        scale = np.abs(Ho).max()
        e = (np.abs(Ah[k] - Ho).max() / scale, np.abs(alh[k] - ao).max() / scale, np.abs(xh[k] - xo).max() / np.abs(xo).max())
        worst = [max(a, b) for a, b in zip(worst, e)]
    print(f"{m}x{n}: {len(ks)} matrices vs oracle: |dH|={worst[0]:.2e} |dalpha|={worst[1]:.2e} (tol {tol:.2e}) |dx|={worst[2]:.2e} (tol 1e-9)")
    assert worst[0] <= tol and worst[1] <= tol
    assert worst[2] <= 1e-9


@pytest.mark.parametrize("m,n,batch", [(m, n, 300) for m, n in WAVE_SHAPES + ONE_CU_SHAPES] + [(16, 8, 20000)])
def test_batched_vs_oracle(pkg, orc, torch_cuda, small_route, m, n, batch):
    """more matrices than compute units (workgroups queue); tolerances of test_small_route_vs_oracle; the large batch is
    checked against the oracle at every 97th matrix and everywhere through the invariants of the factor format"""
    torch = torch_cuda
    seed = 100
    A = pkg.rand_colmajor_batched(batch, m, n, seed, "cuda:0")
    A0 = A.clone()
    b = _rand_b(pkg, batch, m, seed + 5000)
    b0 = b.clone()
    H = pkg.qr_batched_(A)
    assert H.A is A and tuple(H.α.shape) == (batch, n)
    x = H.solve(b)
    torch.cuda.synchronize()
    assert tuple(x.shape) == (batch, n)
    assert torch.equal(b, b0), "H \\ b must not modify b (src:318)"
    _invariants(torch, H, A0, n)
    _against_oracle(orc, H, x, m, n, seed, range(batch) if batch <= 300 else range(0, batch, 97))
    for k in (0, batch // 2, batch - 1):  # a matrix sliced out of the batch is a single-matrix factorisation
        Hk = pkg.DistributedHouseholderQRStruct(H.A[k], H.α[k])
        assert pkg.residual(Hk, A0[k]) < 1e-12


@pytest.mark.parametrize("m,n", ONE_CU_SHAPES)
def test_one_cu_tier_bit_identical_to_single_calls(pkg, torch_cuda, small_route, m, n):
    torch = torch_cuda
    batch, seed = 300, 300
    A = pkg.rand_colmajor_batched(batch, m, n, seed, "cuda:0")
    b = _rand_b(pkg, batch, m, seed + 5000)
    H = pkg.qr_batched_(A, nb=128)
    x = pkg.ldiv_batched(H, b)
    for k in (0, 1, 150, 299):
        Hk = pkg.qr_(pkg.rand_colmajor(m, n, seed + k, "cuda:0"))
        xk = pkg.ldiv(Hk, b[k])
        assert torch.equal(Hk.A, H.A[k]) and torch.equal(Hk.α, H.α[k]) and torch.equal(xk, x[k])


@pytest.mark.parametrize("m,n", [(16, 8), (64, 32), (110, 100), (220, 200)])
def test_batch_is_one_launch(pkg, torch_cuda, small_route, m, n):
    ctx = small_route
    A = pkg.rand_colmajor_batched(7, m, n, 1, "cuda:0")
    b = _rand_b(pkg, 7, m, 2)
    ctx.reset_stats()
    ctx.set_profiling(True)
    try:
        H = pkg.qr_batched_(A)
        st = ctx.stats()
        assert (st["n_rank1"], st["n_panel"], st["n_solve"]) == (1, 0, 0)
        pkg.ldiv_batched(H, b)
        st = ctx.stats()
        assert (st["n_rank1"], st["n_panel"], st["n_solve"]) == (1, 0, 1)
        # the small route off: the serial tier, as many groups as single calls make
        ctx.set_small_route(False)
        ctx.reset_stats()
        pkg.qr_batched_(pkg.rand_colmajor_batched(2, m, n, 1, "cuda:0"), nb=0)
        two = ctx.stats()
        ctx.reset_stats()
        for k in range(2):
            pkg.qr_(pkg.rand_colmajor(m, n, 1 + k, "cuda:0"), nb=0)
        one = ctx.stats()
        assert (two["n_rank1"], two["n_panel"]) == (one["n_rank1"], one["n_panel"])
    finally:
        ctx.set_profiling(False)
        ctx.set_small_route(True)


@pytest.mark.parametrize("m,n", [(16, 8), (40, 17), (110, 100)])
def test_host_arrays(pkg, orc, torch_cuda, small_route, m, n):
    """numpy batches: column-major matrices in place, any other layout copied there and back; the device pair's bits"""
    batch, seed = 9, 400
    mats = np.stack([orc.rand_matrix(m, n, seed + k) for k in range(batch)])
    bs = np.stack([orc.rand_vector(m, seed + 5000 + k) for k in range(batch)])
    Ad = pkg.rand_colmajor_batched(batch, m, n, seed, "cuda:0")
    assert np.array_equal(Ad.cpu().numpy(), mats), "device fill differs from the oracle generator"
    Hd = pkg.qr_batched_(Ad)
    xd = pkg.ldiv_batched(Hd, torch_cuda.tensor(bs, device="cuda:0"))
    F = np.empty((batch, n, m)).transpose(0, 2, 1)  # matrices column-major
    F[...] = mats
    C = mats.copy()                                  # C order: matrices row-major
    for X in (F, C):
        H = pkg.qr_batched_(X)
        assert H.A is X
        assert np.array_equal(X, Hd.A.cpu().numpy()) and np.array_equal(H.α, Hd.α.cpu().numpy())
        b0 = bs.copy()
        x = H.solve(bs)
        assert np.array_equal(bs, b0) and np.array_equal(x, xd.cpu().numpy())


def test_wave_tier_switch_and_errors(pkg, torch_cuda, small_route, monkeypatch):
    """DHQR_TUNE batched_wave=0 sends the tiny shapes to the one-workgroup kernels (what tools/batched_bench.py compares):
    the single-matrix small route's bits; argument errors surface as DHQRError"""
    torch = torch_cuda
    monkeypatch.setenv("DHQR_TUNE", "batched_wave=0")
    monkeypatch.setenv("DHQR_SMALL", "1")
    ctx = pkg.Context(0)
    try:
        L = pkg._lib.lib()
        import ctypes
        A = pkg.rand_colmajor_batched(5, 16, 8, 9, "cuda:0")
        al = torch.zeros((5, 8), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        pkg._lib.check(L.dhqr_factor_batched_f64(ctx.handle, ctypes.c_void_p(A.data_ptr()), 16, 8, 16, 128,
                                                 ctypes.c_void_p(al.data_ptr()), 8, 5, 0))
        ctx.synchronize()
        for k in range(5):
            Hk = pkg.qr_(pkg.rand_colmajor(16, 8, 9 + k, "cuda:0"))
            assert torch.equal(Hk.A, A[k]) and torch.equal(Hk.α, al[k])
    finally:
        ctx.close()
    with pytest.raises(pkg.DHQRError) as e:
        pkg.qr_batched_(pkg.empty_colmajor_batched(3, 4, 8, "cuda:0"))  # m < n
    assert e.value.code == pkg._lib.EINVAL
    with pytest.raises(ValueError):
        pkg.qr_batched_(torch.zeros((3, 16, 8), dtype=torch.float64, device="cuda:0"))  # row-major matrices
    H = pkg.qr_batched_(pkg.empty_colmajor_batched(0, 16, 8, "cuda:0"))  # an empty batch is a no-op
    assert tuple(H.α.shape) == (0, 8)
