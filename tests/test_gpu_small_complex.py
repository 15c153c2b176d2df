"""The one-workgroup ComplexF64 tier on the MI355X (csrc/dhqr_small_complex.h: k_small_zqr / k_small_zldiv, up to 128 x 128):
qr_batched_ / ldiv_batched and qr_ / ldiv on complex128 device tensors and host arrays against the oracle under the rule of
zbatched_helpers.py (T = 8 max(n, 8) eps of max|H|: no matrix above 8 T, at most 1 % of 300 or one of nine above T; x within
1e-9), single = batch of one bit for bit, independence of the matrices of a batch, repeatability, ONE launch per call,
guarded layouts through the C ABI, host arrays, stream order."""
import ctypes

import numpy as np
import pytest

import zbatched_helpers as zh

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
DEV = "cuda:0"


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


_REF = {}


def _reference(orc, m, n, k):
    """oracle factor and solution of matrix k of the shared inputs (seeds SEED + k, BSEED + k): computed once per session"""
    key = (m, n, k)
    if key not in _REF:
        _REF[key] = zh.reference(orc, orc.rand_matrix_c(m, n, zh.SEED + k), orc.rand_vector_c(m, zh.BSEED + k))
    return _REF[key]


def _rand_b(pkg, batch, m, seed):
    return pkg.rand_colmajor_batched_c(batch, m, 1, seed, DEV).reshape(batch, m).contiguous()


def _clone_cm(pkg, X):
    W = pkg.empty_colmajor_batched_c(X.shape[0], X.shape[1], X.shape[2], DEV)
    W.copy_(X)
    return W


@pytest.mark.parametrize("m,n,batch", [(66, 33, 300), (110, 100, 9), (128, 128, 9)])
def test_batched_vs_oracle(pkg, orc, torch_cuda, small_route, m, n, batch):
    """every matrix checked; 300 matrices are more than the compute units"""
    torch = torch_cuda
    A = pkg.rand_colmajor_batched_c(batch, m, n, zh.SEED, DEV)
    b = _rand_b(pkg, batch, m, zh.BSEED)
    A0, b0 = A.clone(), b.clone()
    assert np.array_equal(A0[batch - 1].cpu().numpy(), orc.rand_matrix_c(m, n, zh.SEED + batch - 1)), "device fill differs from the oracle generator"
    H = pkg.qr_batched_(A)
    x = pkg.ldiv_batched(H, b)
    torch.cuda.synchronize()
    assert torch.equal(b, b0), "H \\ b must not modify b (src:318)"
    Ah, alh, xh = H.A.cpu().numpy(), H.α.cpu().numpy(), x.cpu().numpy()
    ratios, dxs = [], []
    for k in range(batch):
        Ho, ao, xo = _reference(orc, m, n, k)
        ratios.append(zh.ratio_H(Ho, ao, Ah[k], alh[k]))
        dxs.append(np.abs(xh[k] - xo).max() / np.abs(xo).max())
    zh.check_rule(f"{m}x{n} batch {batch}", ratios, dxs, above_allowed=batch // 100 if batch >= 100 else 1)
    A0h = A0.cpu().numpy()
    for k in (0, batch // 2, batch - 1):
        QR = orc.form_qr_c(np.asfortranarray(Ah[k]), alh[k])
        assert np.linalg.norm(A0h[k] - QR) / np.linalg.norm(A0h[k]) < 1e-12


@pytest.mark.parametrize("m,n", [(66, 33), (128, 128)])
def test_single_is_a_batch_of_one(pkg, torch_cuda, small_route, m, n):
    """qr_ / ldiv against qr_batched_ / ldiv_batched on the same matrix, with nb = 0 and nb = 64"""
    torch = torch_cuda
    A = pkg.rand_colmajor_batched_c(1, m, n, 210, DEV)
    b = _rand_b(pkg, 1, m, 5210)
    Hb = pkg.qr_batched_(_clone_cm(pkg, A))
    xb = pkg.ldiv_batched(Hb, b)
    for nb in (0, 64):
        H1 = pkg.qr_(pkg.rand_colmajor_c(m, n, 210, DEV), nb=nb)
        x1 = pkg.ldiv(H1, b[0].clone())
        assert torch.equal(H1.A, Hb.A[0]) and torch.equal(H1.α, Hb.α[0]) and torch.equal(x1, xb[0])


def test_independent_and_repeatable(pkg, torch_cuda, small_route):
    """(66, 33): matrix k of a batch of 300 has the bits of a batch of one holding it alone; three runs give the same bits"""
    torch = torch_cuda
    m, n, batch = 66, 33, 300
    A0 = pkg.rand_colmajor_batched_c(batch, m, n, zh.SEED, DEV)
    b = _rand_b(pkg, batch, m, zh.BSEED)
    runs = []
    for _ in range(3):
        H = pkg.qr_batched_(_clone_cm(pkg, A0))
        runs.append((H.A.clone(), H.α.clone(), pkg.ldiv_batched(H, b)))
    for r in runs[1:]:
        assert all(torch.equal(u, v) for u, v in zip(r, runs[0]))
    HA, Hal, x = runs[0]
    for k in (0, 1, 150, 255, 256, 299):
        Hk = pkg.qr_batched_(_clone_cm(pkg, A0[k:k + 1]))
        xk = pkg.ldiv_batched(Hk, b[k:k + 1])
        assert torch.equal(Hk.A[0], HA[k]) and torch.equal(Hk.α[0], Hal[k]) and torch.equal(xk[0], x[k])


def test_batch_is_one_launch(pkg, torch_cuda, small_route):
    """(66, 33), batch 300: ONE n_rank1 group for the factor, ONE n_solve for the solve (the serial tier this shape had
    before counted 300 of each)"""
    ctx = small_route
    A = pkg.rand_colmajor_batched_c(300, 66, 33, 1, DEV)
    b = _rand_b(pkg, 300, 66, 2)
    ctx.reset_stats()
    ctx.set_profiling(True)
    try:
        H = pkg.qr_batched_(A)
        st = ctx.stats()
        assert (st["n_rank1"], st["n_panel"], st["n_solve"]) == (1, 0, 0)
        pkg.ldiv_batched(H, b)
        st = ctx.stats()
        assert (st["n_rank1"], st["n_panel"], st["n_solve"]) == (1, 0, 1)
    finally:
        ctx.set_profiling(False)


def _c_abi(pkg):
    ctx = pkg.get_context(0)
    ctx.use_torch_stream()
    return pkg._lib.lib(), ctx


def _guarded(torch, mats, bs, pad_ld, pad, pad_al, off):
    """flat sentinel-filled device buffers holding a strided batch (the layout of zbatched_helpers.ZBatch)"""
    batch, (m, n) = len(mats), mats[0].shape
    lda, sal, sb = m + pad_ld, n + pad_al, m + pad
    sA = lda * n + pad
    A = torch.full((off + batch * sA + 7,), zh.SENT, dtype=torch.complex128, device=DEV)
    al = torch.full((off + batch * sal + 7,), zh.SENT, dtype=torch.complex128, device=DEV)
    b = torch.full((off + batch * sb + 7,), zh.SENT, dtype=torch.complex128, device=DEV)
    mA, mal, mb = (torch.zeros(v.numel(), dtype=torch.bool, device=DEV) for v in (A, al, b))

    def mat(k):
        return A[off + k * sA: off + k * sA + lda * n].view(n, lda).t()[:m]

    for k in range(batch):
        mat(k).copy_(torch.from_numpy(mats[k]))
        for j in range(n):
            mA[off + k * sA + j * lda: off + k * sA + j * lda + m] = True
        mal[off + k * sal: off + k * sal + n] = True
        b[off + k * sb: off + k * sb + m] = torch.from_numpy(bs[k]).to(DEV)
        mb[off + k * sb: off + k * sb + m] = True

    def intact():
        return bool((A[~mA] == zh.SENT).all() and (al[~mal] == zh.SENT).all() and (b[~mb] == zh.SENT).all())

    def ptrs():
        return P(A.data_ptr() + 16 * off), P(al.data_ptr() + 16 * off), P(b.data_ptr() + 16 * off)

    return dict(A=A, al=al, b=b, lda=lda, sA=sA, sal=sal, sb=sb, mat=mat, intact=intact, ptrs=ptrs,
                alpha=lambda k: al[off + k * sal: off + k * sal + n], rhs=lambda k: b[off + k * sb: off + k * sb + m])


def _run_c_abi(pkg, torch, G, m, n, batch):
    L, ctx = _c_abi(pkg)
    pA, pal, pb = G["ptrs"]()
    torch.cuda.synchronize()
    pkg._lib.check(L.dhqr_factor_batched_c64(ctx.handle, pA, m, n, G["lda"], G["sA"], pal, G["sal"], batch, 0))
    pkg._lib.check(L.dhqr_solve_batched_c64(ctx.handle, pA, m, n, G["lda"], G["sA"], pal, G["sal"], pb, G["sb"], batch))
    ctx.synchronize()


@pytest.mark.parametrize("m,n", [(66, 33), (97, 64)])
def test_guarded_layout_through_the_c_abi(pkg, orc, torch_cuda, small_route, m, n):
    """lda = m + 1, strideA and strideb padded, stride_alpha = n + 3, base one complex element in, sentinel-filled: the packed
    call's bits, every sentinel intact; a base 8 bytes in is DHQR_EINVAL and writes nothing"""
    torch = torch_cuda
    batch = 5
    mats, bs = zh.inputs(orc, m, n, range(batch), seed=300, bseed=5300)
    G = _guarded(torch, mats, bs, 1, 5, 3, 1)
    Pk = _guarded(torch, mats, bs, 0, 0, 0, 0)
    L, ctx = _c_abi(pkg)
    pA, pal, pb = G["ptrs"]()
    before = [G[k].clone() for k in ("A", "al", "b")]
    EINVAL = pkg._lib.EINVAL
    assert L.dhqr_factor_batched_c64(ctx.handle, P(pA.value + 8), m, n, G["lda"], G["sA"], pal, G["sal"], batch, 0) == EINVAL
    assert L.dhqr_solve_batched_c64(ctx.handle, pA, m, n, G["lda"], G["sA"], pal, G["sal"], P(pb.value + 8), G["sb"], batch) == EINVAL
    assert L.dhqr_factor_c64(ctx.handle, P(pA.value + 8), m, n, G["lda"], pal) == EINVAL
    ctx.synchronize()
    for got, want in zip((G["A"], G["al"], G["b"]), before):
        assert torch.equal(got, want), "a rejected call must not touch anything"
    for X in (G, Pk):
        _run_c_abi(pkg, torch, X, m, n, batch)
    assert G["intact"]() and Pk["intact"]()
    for k in range(batch):
        assert torch.equal(G["mat"](k), Pk["mat"](k)) and torch.equal(G["alpha"](k), Pk["alpha"](k))
        assert torch.equal(G["rhs"](k), Pk["rhs"](k))


def test_host_arrays(pkg, orc, torch_cuda, small_route):
    """(110, 100) numpy arrays through qr_ / ldiv: the bits of the device-tensor calls, b untouched; and the reference's own
    statistic (test/runtests.jl:49-62) for draw seed 0: ||A'A x - A'b|| below 8 x that of numpy.linalg.lstsq's solution"""
    m, n, seed = 110, 100, 0
    A0, b0 = orc.rand_matrix_c(m, n, seed), orc.rand_vector_c(m, seed + 1)
    Ad = pkg.rand_colmajor_c(m, n, seed, DEV)
    assert np.array_equal(Ad.cpu().numpy(), A0), "device fill differs from the oracle generator"
    Hd = pkg.qr_(Ad)
    xd = pkg.ldiv(Hd, torch_cuda.from_numpy(b0.copy()).to(DEV))
    for nb in (0, 64):
        F = A0.copy(order="F")
        H = pkg.qr_(F, nb=nb)
        assert np.array_equal(np.asarray(H.A), Hd.A.cpu().numpy()) and np.array_equal(np.asarray(H.α), Hd.α.cpu().numpy())
        bb = b0.copy()
        x = np.asarray(pkg.ldiv(H, bb))
        assert np.array_equal(bb, b0) and np.array_equal(x, xd.cpu().numpy())
    Ah = A0.conj().T
    stat = np.linalg.norm(Ah @ (A0 @ x) - Ah @ b0)
    xl = np.linalg.lstsq(A0, b0, rcond=None)[0]
    stat_l = np.linalg.norm(Ah @ (A0 @ xl) - Ah @ b0)
    print(f"110x100 seed 0: ||A'Ax - A'b|| = {stat:.3e}, lstsq {stat_l:.3e}, ratio {stat / stat_l:.2f}")
    assert stat < 8.0 * stat_l


def test_stream_ordered(pkg, orc, torch_cuda, small_route):
    """dhqr_factor_c64 + dhqr_solve_c64 on the torch stream, followed only by torch.cuda.synchronize(): the bits of qr_ / ldiv"""
    torch = torch_cuda
    m, n = 110, 100
    L, ctx = _c_abi(pkg)
    A = pkg.rand_colmajor_c(m, n, 77, DEV)
    b = _rand_b(pkg, 1, m, 78)[0].contiguous()
    H = pkg.qr_(pkg.rand_colmajor_c(m, n, 77, DEV))
    x = pkg.ldiv(H, b.clone())
    al = torch.zeros(n, dtype=torch.complex128, device=DEV)
    lda = A.stride(1)
    pkg._lib.check(L.dhqr_factor_c64(ctx.handle, P(A.data_ptr()), m, n, lda, P(al.data_ptr())))
    pkg._lib.check(L.dhqr_solve_c64(ctx.handle, P(A.data_ptr()), m, n, lda, P(al.data_ptr()), P(b.data_ptr())))
    x2 = b[:n] * 1  # (enqueued on the torch stream behind the solve)
    torch.cuda.synchronize()
    assert torch.equal(A, H.A) and torch.equal(al, H.α) and torch.equal(x2, x)
