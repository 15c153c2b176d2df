"""Batches of small ComplexF64 matrices on the MI355X: qr_batched_ / ldiv_batched on complex128 device tensors and host arrays,
and dhqr_*_batched_c64 through the C ABI -- the wave-per-matrix kernels of csrc/dhqr_batched_complex.h against the oracle
under the rule of zbatched_helpers.py (T = 8 max(n, 8) eps of max|H|: no matrix above 8 T, at most 1 % of 300 above T; x
within 1e-9), the serial tier bit for bit against the single-matrix calls, independence of the matrices of a batch, launch
counts, guarded layouts, special inputs, host arrays, errors."""
import ctypes

import numpy as np
import pytest

import zbatched_helpers as zh

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
ZNB = 64
DEV = "cuda:0"


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


_REF = {}


def _reference(orc, m, n, k):
    """oracle factor and solution of matrix k of the shared inputs (seeds SEED + k, BSEED + k): computed once per session"""
    key = (m, n, k)
    if key not in _REF:
        _REF[key] = zh.reference(orc, orc.rand_matrix_c(m, n, zh.SEED + k), orc.rand_vector_c(m, zh.BSEED + k))
    return _REF[key]


def _rand_b(pkg, batch, m, seed):
    """(batch, m) complex device tensor, row k = the shared generator's complex vector of seed + k (rand_vector_c)"""
    return pkg.rand_colmajor_batched_c(batch, m, 1, seed, DEV).reshape(batch, m).contiguous()


def _clone_cm(pkg, X):
    """a copy of a (batch, m, n) device batch, its matrices column-major"""
    W = pkg.empty_colmajor_batched_c(X.shape[0], X.shape[1], X.shape[2], DEV)
    W.copy_(X)
    return W


def _to_dev(torch, mats):
    """(batch, m, n) device tensor with column-major matrices holding the host matrices"""
    batch, (m, n) = len(mats), mats[0].shape
    A = torch.empty((batch, n, m), dtype=torch.complex128, device=DEV).transpose(1, 2)
    A.copy_(torch.from_numpy(np.stack(mats)))
    return A


@pytest.mark.parametrize("m,n,batch", [(m, n, 300) for m, n in zh.WAVE_SHAPES] + [(16, 8, 20000)])
def test_batched_vs_oracle(pkg, orc, torch_cuda, small_route, m, n, batch):
    """more matrices than compute units; the large batch is checked at every 97th matrix"""
    torch = torch_cuda
    A = pkg.rand_colmajor_batched_c(batch, m, n, zh.SEED, DEV)
    b = _rand_b(pkg, batch, m, zh.BSEED)
    A0 = A.clone()
    b0 = b.clone()
    assert np.array_equal(A0[batch - 1].cpu().numpy(), orc.rand_matrix_c(m, n, zh.SEED + batch - 1)), "device fill differs from the oracle generator"
    assert np.array_equal(b0[batch - 1].cpu().numpy(), orc.rand_vector_c(m, zh.BSEED + batch - 1))
    H = pkg.qr_batched_(A)
    assert H.A is A and tuple(H.α.shape) == (batch, n) and H.α.dtype == torch.complex128
    x = H.solve(b)
    torch.cuda.synchronize()
    assert tuple(x.shape) == (batch, n) and x.dtype == torch.complex128
    assert torch.equal(b, b0), "H \\ b must not modify b (src:318)"
    Ah, alh, xh = H.A.cpu().numpy(), H.α.cpu().numpy(), x.cpu().numpy()
    ks = list(range(batch) if batch <= 300 else range(0, batch, 97))
    ratios, dxs = [], []
    for k in ks:
        Ho, ao, xo = _reference(orc, m, n, k)
        ratios.append(zh.ratio_H(Ho, ao, Ah[k], alh[k]))
        dxs.append(np.abs(xh[k] - xo).max() / np.abs(xo).max())
    zh.check_rule(f"{m}x{n} batch {batch}", ratios, dxs, above_allowed=len(ks) // 100)
    A0h = A0.cpu().numpy()
    for k in (0, batch // 2, batch - 1):
        QR = orc.form_qr_c(np.asfortranarray(Ah[k]), alh[k])
        assert np.linalg.norm(A0h[k] - QR) / np.linalg.norm(A0h[k]) < 1e-12


def _serial_tier(pkg, torch, m, n, nb):
    batch, seed = 3, 200
    A = pkg.rand_colmajor_batched_c(batch, m, n, seed, DEV)
    b = _rand_b(pkg, batch, m, seed + 5000)
    H = pkg.qr_batched_(A, nb=nb)
    x = pkg.ldiv_batched(H, b)
    for k in range(batch):
        Hk = pkg.qr_(pkg.rand_colmajor_c(m, n, seed + k, DEV), nb=nb)
        xk = pkg.ldiv(Hk, b[k])
        assert torch.equal(Hk.A, H.A[k]) and torch.equal(Hk.α, H.α[k]) and torch.equal(xk, x[k])


@pytest.mark.parametrize("nb", [0, ZNB])
@pytest.mark.parametrize("m,n", [(66, 33), (130, 20)])
def test_serial_tier_bit_identical_to_single_calls(pkg, torch_cuda, small_route, m, n, nb):
    """beyond 64 x 32: H, alpha and x of matrix k are those of qr_ / ldiv on that matrix alone"""
    _serial_tier(pkg, torch_cuda, m, n, nb)


@pytest.mark.parametrize("nb", [0, ZNB])
def test_serial_tier_with_the_small_route_off(pkg, torch_cuda, nb):
    """(16, 8) with the suite's default (small route off): the loop of single calls, their bits"""
    _serial_tier(pkg, torch_cuda, 16, 8, nb)


def test_matrices_of_a_batch_are_independent(pkg, torch_cuda, small_route):
    """matrix k of a batch of 300 has the bits of a batch of one holding it alone"""
    torch = torch_cuda
    m, n, batch = 16, 8, 300
    A = pkg.rand_colmajor_batched_c(batch, m, n, zh.SEED, DEV)
    b = _rand_b(pkg, batch, m, zh.BSEED)
    A0 = A.clone()
    H = pkg.qr_batched_(A)
    x = pkg.ldiv_batched(H, b)
    for k in (0, 1, 2, 3, 150, 297, 298, 299):
        Hk = pkg.qr_batched_(_clone_cm(pkg, A0[k:k + 1]))
        xk = pkg.ldiv_batched(Hk, b[k:k + 1])
        assert torch.equal(Hk.A[0], H.A[k]) and torch.equal(Hk.α[0], H.α[k]) and torch.equal(xk[0], x[k])


def _c_abi(pkg):
    ctx = pkg.get_context(0)
    ctx.use_torch_stream()
    return pkg._lib.lib(), ctx


def _guarded(torch, mats, bs, pad_ld, pad, pad_al, off):
    """flat sentinel-filled device buffers holding a strided batch; returns (A, al, b, lda, sA, sal, sb, views)"""
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


@pytest.mark.parametrize("batch", [1, 3, 4, 5])
def test_partial_workgroups_leave_the_bytes_behind_the_batch(pkg, orc, torch_cuda, small_route, batch):
    """four matrices per workgroup: a workgroup's last waves without a matrix write nothing"""
    torch = torch_cuda
    m, n = 16, 8
    mats, bs = zh.inputs(orc, m, n, range(batch), seed=350, bseed=5350)
    G = _guarded(torch, mats, bs, 0, 0, 0, 0)  # packed, seven sentinels behind the last matrix / alpha / b
    _run_c_abi(pkg, torch, G, m, n, batch)
    assert G["intact"]()
    H = pkg.qr_batched_(_to_dev(torch, mats))
    for k in range(batch):
        assert torch.equal(G["mat"](k), H.A[k]) and torch.equal(G["alpha"](k), H.α[k])


def test_batch_is_one_launch(pkg, torch_cuda, small_route):
    ctx = small_route
    A = pkg.rand_colmajor_batched_c(7, 16, 8, 1, DEV)
    b = _rand_b(pkg, 7, 16, 2)
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


def test_guarded_layout_through_the_c_abi(pkg, orc, torch_cuda, small_route):
    """(40, 17): lda = m + 1, strideA and strideb padded, stride_alpha = n + 3, base one complex element in, sentinel-filled:
    the packed call's bits, every sentinel intact"""
    torch = torch_cuda
    m, n, batch = 40, 17, 6
    mats, bs = zh.inputs(orc, m, n, range(batch), seed=300, bseed=5300)
    G = _guarded(torch, mats, bs, 1, 5, 3, 1)
    Pk = _guarded(torch, mats, bs, 0, 0, 0, 0)
    for X in (G, Pk):
        _run_c_abi(pkg, torch, X, m, n, batch)
    assert G["intact"]()
    for k in range(batch):
        assert torch.equal(G["mat"](k), Pk["mat"](k)) and torch.equal(G["alpha"](k), Pk["alpha"](k))
        assert torch.equal(G["rhs"](k), Pk["rhs"](k))


@pytest.mark.parametrize("m,n", [(16, 8), (64, 32)])
def test_special_matrices(pkg, orc, torch_cuda, small_route, m, n):
    """seven matrices: an imaginary part identically zero, a real part identically zero, a pivot exactly 0 above a nonzero
    rest (the factor -1 of zalphafactor), ordinary ones: every one within 8 T, at most one above T (zbatched_helpers.py)"""
    torch = torch_cuda
    mats = zh.special_matrices(orc, m, n)
    bs = [orc.rand_vector_c(m, 5900 + k) for k in range(7)]
    H = pkg.qr_batched_(_to_dev(torch, mats))
    x = pkg.ldiv_batched(H, torch.from_numpy(np.stack(bs)).to(DEV))
    Ah, alh, xh = H.A.cpu().numpy(), H.α.cpu().numpy(), x.cpu().numpy()
    ratios, dxs = [], []
    for k in range(7):
        Ho, ao, xo = zh.reference(orc, mats[k], bs[k])
        ratios.append(zh.ratio_H(Ho, ao, Ah[k], alh[k]))
        dxs.append(np.abs(xh[k] - xo).max() / np.abs(xo).max())
    for k in (1, 5):
        assert (Ah[k].imag == 0).all() and (alh[k].imag == 0).all(), "a real matrix stays real"
    for k in (3, 5):  # alphafactor(0) = -1: alpha_0 = -||a_0||
        assert alh[k][0].real < 0 and alh[k][0].imag == 0
    zh.check_rule(f"special {m}x{n}", ratios, dxs, above_allowed=1)


def test_zero_column_inside_a_batch(pkg, orc, torch_cuda, small_route):
    """matrix 2 of five has a zero column 3: its isfinite masks of H and alpha are the oracle's; every other matrix of the
    batch has the bits it has without the poisoned neighbour"""
    torch = torch_cuda
    m, n = 16, 8
    mats, _ = zh.inputs(orc, m, n, range(5), seed=700, bseed=5700)
    bad = [zh.poison_column(A) if k == 2 else A for k, A in enumerate(mats)]
    Hg = pkg.qr_batched_(_to_dev(torch, mats))
    Hb = pkg.qr_batched_(_to_dev(torch, bad))
    Ho, ao = orc.householder_c(bad[2])
    assert np.isfinite(Ho[:, :3]).all() and np.isfinite(Ho[:3]).all() and not np.isfinite(Ho[3:, 3:]).any()
    assert ao[3] == 0 and np.isfinite(ao[:4]).all() and not np.isfinite(ao[4:]).any()
    Hd, ad = Hb.A[2].cpu().numpy(), Hb.α[2].cpu().numpy()
    assert np.array_equal(np.isfinite(Hd), np.isfinite(Ho)) and np.array_equal(np.isfinite(ad), np.isfinite(ao))
    assert ad[3] == 0
    for k in (0, 1, 3, 4):
        assert torch.equal(Hb.A[k], Hg.A[k]) and torch.equal(Hb.α[k], Hg.α[k])


def test_one_by_one_matrices(pkg, orc, torch_cuda, small_route):
    """3 - 4i, 0, -2, i: alpha and H as the oracle's (3 - 4i: alpha = -3 + 4i; 0: alpha = -0 and a NaN H)"""
    torch = torch_cuda
    vals = [3 - 4j, 0j, -2 + 0j, 1j]
    mats = [np.asfortranarray(np.array([[v]], dtype=np.complex128)) for v in vals]
    H = pkg.qr_batched_(_to_dev(torch, mats))
    Ah, alh = H.A.cpu().numpy(), H.α.cpu().numpy()
    for k, v in enumerate(vals):
        Ho, ao = orc.householder_c(mats[k])
        assert np.array_equal(np.isfinite(Ah[k]), np.isfinite(Ho)) and np.array_equal(np.isfinite(alh[k]), np.isfinite(ao))
        assert abs(alh[k][0] - ao[0]) <= zh.T(1) * max(abs(v), 1.0)
        if v != 0:
            assert abs(Ah[k][0, 0] - Ho[0, 0]) <= zh.T(1) * abs(Ho[0, 0])
    assert abs(alh[0][0] - (-3 + 4j)) <= zh.T(1) * 5.0
    assert alh[1][0] == 0 and np.isnan(Ah[1][0, 0])


@pytest.mark.parametrize("m,n", [(16, 8), (40, 17)])
def test_host_arrays(pkg, orc, torch_cuda, small_route, m, n):
    """numpy batches: column-major matrices in place, a C-ordered batch copied there and back; the device pair's bits"""
    batch, seed = 9, 400
    mats = np.stack([orc.rand_matrix_c(m, n, seed + k) for k in range(batch)])
    bs = np.stack([orc.rand_vector_c(m, seed + 5000 + k) for k in range(batch)])
    Ad = pkg.rand_colmajor_batched_c(batch, m, n, seed, DEV)
    assert np.array_equal(Ad.cpu().numpy(), mats), "device fill differs from the oracle generator"
    Hd = pkg.qr_batched_(Ad)
    xd = pkg.ldiv_batched(Hd, torch_cuda.tensor(bs, device=DEV))
    F = np.empty((batch, n, m), dtype=np.complex128).transpose(0, 2, 1)  # matrices column-major
    F[...] = mats
    C = mats.copy()                                                      # C order: matrices row-major
    for X in (F, C):
        H = pkg.qr_batched_(X)
        assert H.A is X and H.α.dtype == np.complex128 and H.α.shape == (batch, n)
        assert np.array_equal(X, Hd.A.cpu().numpy()) and np.array_equal(H.α, Hd.α.cpu().numpy())
        b0 = bs.copy()
        x = H.solve(bs)
        assert np.array_equal(bs, b0) and np.array_equal(x, xd.cpu().numpy())


def test_errors(pkg, orc, torch_cuda, small_route):
    torch = torch_cuda
    m, n, batch = 12, 6, 3
    A = pkg.rand_colmajor_batched_c(batch, m, n, 9, DEV)
    H = pkg.qr_batched_(_clone_cm(pkg, A))
    with pytest.raises(TypeError):
        pkg.ldiv_batched(H, torch.zeros((batch, m), dtype=torch.float64, device=DEV))  # real b, complex factor
    with pytest.raises(TypeError):
        pkg.ldiv_batched(H, np.zeros((batch, m)))
    Hr = pkg.qr_batched_(pkg.rand_colmajor_batched(batch, m, n, 9, DEV))
    with pytest.raises(TypeError):
        pkg.ldiv_batched(Hr, torch.zeros((batch, m), dtype=torch.complex128, device=DEV))  # complex b, real factor
    with pytest.raises(TypeError):
        pkg.ldiv_batched(H, torch.zeros((batch, m, 2), dtype=torch.complex128, device=DEV))  # several right-hand sides
    with pytest.raises(ValueError):
        pkg.qr_batched_(_clone_cm(pkg, A), nb=128)
    with pytest.raises(ValueError):
        pkg.qr_batched_(torch.zeros((batch, m, n), dtype=torch.complex128, device=DEV))  # row-major matrices
    for fn in (pkg.get_q, pkg.get_r):
        with pytest.raises(TypeError):
            fn(H)
    with pytest.raises(TypeError):
        pkg.apply_q_(H, torch.zeros((batch, m, 2), dtype=torch.complex128, device=DEV).transpose(1, 2), True)
    with pytest.raises((TypeError, ValueError)):
        pkg.residual(H, A)
    with pytest.raises(pkg.DHQRError) as e:
        pkg.qr_batched_(pkg.empty_colmajor_batched_c(3, 4, 8, DEV))  # m < n
    assert e.value.code == pkg._lib.EINVAL
    H0 = pkg.qr_batched_(pkg.empty_colmajor_batched_c(0, 16, 8, DEV))  # an empty batch is a no-op
    assert tuple(H0.α.shape) == (0, 8) and H0.α.dtype == torch.complex128
    # the DHQR_EINVAL cases through the C ABI write nothing
    L, ctx = _c_abi(pkg)
    mats, bs = zh.inputs(orc, m, n, range(batch), seed=600, bseed=5600)
    G = _guarded(torch, mats, bs, 1, 5, 3, 1)
    before = [G[k].clone() for k in ("A", "al", "b")]
    pA, pal, pb = G["ptrs"]()
    h, lda, sA, sal, sb = ctx.handle, G["lda"], G["sA"], G["sal"], G["sb"]
    EINVAL = pkg._lib.EINVAL
    torch.cuda.synchronize()
    f, s = L.dhqr_factor_batched_c64, L.dhqr_solve_batched_c64
    assert f(h, pA, m, n, lda, sA, pal, sal, -1, 0) == EINVAL
    assert f(h, pA, n - 1, n, lda, sA, pal, sal, batch, 0) == EINVAL
    assert f(h, pA, m, n, lda, lda * (n - 1) + m - 1, pal, sal, batch, 0) == EINVAL
    assert f(h, pA, m, n, lda, sA, pal, n - 1, batch, 0) == EINVAL
    assert f(h, None, m, n, lda, sA, pal, sal, batch, 0) == EINVAL
    assert f(h, pA, m, n, lda, sA, None, sal, batch, 0) == EINVAL
    assert f(h, pA, m, n, lda, sA, pal, sal, batch, 128) == EINVAL
    assert f(h, P(pA.value + 8), m, n, lda, sA, pal, sal, batch, 0) == EINVAL
    assert s(h, pA, m, n, lda, sA, pal, sal, pb, m - 1, batch) == EINVAL
    assert s(h, pA, m, n, lda, sA, pal, sal, None, sb, batch) == EINVAL
    assert s(h, pA, m, n, lda, sA, pal, sal, pb, sb, -1) == EINVAL
    assert f(h, None, m, n, lda, sA, None, sal, 0, 7) == 0 and s(h, None, m, 0, lda, sA, None, sal, None, sb, batch) == 0  # empty
    ctx.synchronize()
    for got, want in zip((G["A"], G["al"], G["b"]), before):
        assert torch.equal(got, want), "a rejected or empty call must not touch anything"
