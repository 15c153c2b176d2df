"""Column-pivoted batched QR, the numerical rank and the rank-truncated least squares on the MI355X: the checks of
pivoted_helpers.py (shared with test_emulated_pivoted.py) through the C ABI on device memory -- every buffer of a batch goes
to the GPU guards and all and comes back --, one batch larger than the GPU holds at once, and the Python front end
(qr_pivoted_batched_, rank_batched, ldiv_pivoted_batched, lstsq_batched) against the C ABI's bytes on tensors and on numpy
arrays."""
import numpy as np
import pytest

import pivoted_helpers as PV
from nrhs_helpers import same_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture
def run(pkg, torch_cuda):
    """the product default (small route on) on the shared context for one test (conftest.py switches it off for the suite)"""
    ctx = pkg.get_context(0)
    ctx.use_torch_stream()
    ctx.set_small_route(True)
    yield PV.Runner(pkg._lib.lib(), ctx.handle, torch_cuda)
    ctx.set_small_route(False)


@pytest.fixture
def run_general(pkg, torch_cuda):
    """the small route off: every shape on the general tier"""
    ctx = pkg.get_context(0)
    ctx.use_torch_stream()
    ctx.set_small_route(False)
    return PV.Runner(pkg._lib.lib(), ctx.handle, torch_cuda)


@pytest.fixture(scope="module")
def data(orc):
    """the inputs, computed once per shape and left unchanged"""
    cache = {}

    def get(m, n):
        if (m, n) not in cache:
            mats, Bs = PV.inputs(orc, m, n)
            for a in mats + Bs:
                a.setflags(write=False)
            cache[(m, n)] = (mats, Bs)
        return cache[(m, n)]
    return get


@pytest.mark.parametrize("m,n", PV.WAVE_SHAPES + PV.GENERAL_SHAPES)
def test_pivots_and_factor(run, data, m, n):
    PV.check_pivots_and_factor(run, *data(m, n))


def test_pivots_and_factor_small_route_off(run_general, data):
    PV.check_pivots_and_factor(run_general, *data(16, 8))


@pytest.mark.parametrize("m,n", [(16, 8), (64, 32), (130, 20)])
def test_pivots_against_scipy(run, data, m, n):
    scipy_linalg = pytest.importorskip("scipy.linalg")
    PV.check_pivots_and_factor(run, *data(m, n), scipy_qr=scipy_linalg.qr)


@pytest.mark.parametrize("m,n", PV.WAVE_SHAPES)
def test_wave_tier_bits(run, data, m, n):
    PV.check_wave_bits(run, *data(m, n))


@pytest.mark.parametrize("m,n,r0", PV.LOW_RANK)
def test_rank_and_solve_of_rank_deficient_matrices(run, m, n, r0):
    PV.check_solve(run, *PV.low_rank_inputs(m, n, r0), r0)


@pytest.mark.parametrize("m,n", PV.WAVE_SHAPES + PV.GENERAL_SHAPES)
def test_solve_full_rank(run, data, m, n):
    """rcond < 0 (the default bound max(m, n) eps) gives rank n on the full-rank inputs"""
    mats, Bs = data(m, n)
    D = PV.check_rank(run, mats, Bs, n, rcond=-1.0)
    assert D.ranks().tolist() == [n] * D.batch
    PV.check_solve(run, mats, Bs, n)


def test_solve_small_route_off(run_general, data):
    PV.check_solve(run_general, *data(16, 8), 8)
    PV.check_solve(run_general, *PV.low_rank_inputs(16, 8, 3), 3)


def test_degenerate(run, orc):
    PV.check_degenerate(run, orc)


def test_degenerate_general_tier(run_general, orc):
    PV.check_degenerate(run_general, orc)


def test_arguments(run, orc):
    PV.check_arguments(run, orc)


def _tile(pkg, torch, mats, batch):
    """(batch, m, n) device tensor with column-major matrices: the given matrices, repeated"""
    m, n = mats[0].shape
    A = pkg.empty_colmajor_batched(batch, m, n, "cuda:0")
    A.copy_(torch.from_numpy(np.stack(mats)).cuda().repeat((batch + len(mats) - 1) // len(mats), 1, 1)[:batch])
    return A


def test_more_matrices_than_fit_at_once(pkg, torch_cuda, run, data):
    """(16, 8) at batch 20000 -- 5000 workgroups --, nrhs 3: matrix k has the bytes of matrix k % 4 of the small batch, in the
    factor, alpha, jpvt, the rank, dB and X; a low-rank matrix among them keeps its own rank"""
    torch = torch_cuda
    m, n, batch = 16, 8, 20000
    mats, Bs = data(m, n)
    mats, Bs = list(mats), list(Bs)
    mats[1] = PV.low_rank_inputs(m, n, 3)[0][0]
    D = PV.factored(run, mats, Bs)
    run.ok(run.rank(D, PV.RCOND))
    run.ok(run.solve(D))
    assert D.ranks().tolist() == [n, 3, n, n]
    H = pkg.qr_pivoted_batched_(_tile(pkg, torch, mats, batch))
    rank = pkg.rank_batched(H, PV.RCOND)
    B = _tile(pkg, torch, Bs, batch)
    B0 = B.clone()
    X = pkg.ldiv_pivoted_batched(H, B, PV.RCOND)
    assert torch.equal(B, B0)
    for k in range(len(mats)):
        for got, want in ((H.A, D.mat(k)), (H.α, D.alpha(k)), (H.jpvt, D.jpvt(k)), (rank, D.ranks()[k]), (X, D.xmat(k))):
            w = torch.from_numpy(np.ascontiguousarray(want)).cuda()
            assert torch.equal(got[k::len(mats)], w.expand_as(got[k::len(mats)])), k


def test_python_front_end(pkg, torch_cuda, run, data):
    """case 7: the four functions give the C ABI's bytes on tensors and on numpy input, for B (batch, m) and (batch, m, nrhs)
    and for a 2-D A (a batch of one); get_q / get_r / apply_q_ take the pivoted struct; arguments stay as they were"""
    torch = torch_cuda
    m, n = 40, 17
    mats, Bs = data(m, n)
    mats = list(mats)
    mats[2] = PV.low_rank_inputs(m, n, 9)[0][0]
    D = PV.factored(run, mats, Bs)
    run.ok(run.rank(D, PV.RCOND))
    run.ok(run.solve(D))
    batch = D.batch
    A_np, B_np = np.stack(mats), np.stack(Bs)
    want_X = np.stack([D.xmat(k) for k in range(batch)])
    for device in (True, False):
        if device:
            A, B = _tile(pkg, torch, mats, batch), _tile(pkg, torch, Bs, batch)
            host = lambda x: x.cpu().numpy()
        else:
            A, B = A_np.copy(), B_np.copy()
            host = lambda x: np.asarray(x)
        A0, B0 = host(A).copy(), host(B).copy()
        X, rank = pkg.lstsq_batched(A, B, PV.RCOND)
        assert same_bytes(host(A), A0) and same_bytes(host(B), B0), "lstsq_batched modified its arguments"
        assert same_bytes(host(X), want_X) and host(rank).tolist() == D.ranks().tolist() and host(rank).dtype == np.int32
        x1, _ = pkg.lstsq_batched(A, B[:, :, 1], PV.RCOND)
        assert same_bytes(host(x1), want_X[:, :, 1])
        H = pkg.qr_pivoted_batched_(A)
        assert H.jpvt is not None and host(H.jpvt).dtype == np.int32
        for k in range(batch):
            assert same_bytes(host(H.A)[k], D.mat(k)) and same_bytes(host(H.α)[k], D.alpha(k)) and same_bytes(host(H.jpvt)[k], D.jpvt(k))
        assert host(pkg.rank_batched(H, PV.RCOND)).tolist() == D.ranks().tolist()
        assert host(pkg.rank_batched(H)).tolist() == [PV.twin_rank(D.alpha(k), -1.0, m) for k in range(batch)]
        assert same_bytes(host(pkg.ldiv_pivoted_batched(H, B, PV.RCOND)), want_X)
        assert same_bytes(host(pkg.ldiv_pivoted_batched(H, B[:, :, 0], PV.RCOND)), want_X[:, :, 0])
        assert same_bytes(host(B), B0)
        one = (_tile(pkg, torch, mats[:1], 1)[0] if device else A_np[0].copy(order="F"))
        H1 = pkg.qr_pivoted_batched_(one)
        assert tuple(H1.A.shape) == (1, m, n) and same_bytes(host(H1.A)[0], D.mat(0)) and same_bytes(host(H1.jpvt)[0], D.jpvt(0))
        if device:
            Qd, Rd = pkg.get_q(H), pkg.get_r(H)
            for k in range(batch):
                jp = D.jpvt(k)
                PV.Q.check_qr(host(Qd)[k], host(Rd)[k], mats[k][:, jp], "f64", f"get_q / get_r, matrix {k}")
            E = pkg.empty_colmajor_batched(batch, m, n, "cuda:0")
            E.zero_()
            E.diagonal(dim1=1, dim2=2).fill_(1.0)
            assert torch.equal(pkg.apply_q_(H, E, False), Qd)
    for dt in (torch.float32, torch.complex128):
        with pytest.raises(TypeError):
            pkg.qr_pivoted_batched_(torch.ones((2, 3, 5), dtype=dt, device="cuda:0").transpose(1, 2))
        with pytest.raises(TypeError):
            pkg.lstsq_batched(torch.ones((2, 3, 5), dtype=dt, device="cuda:0").transpose(1, 2), torch.ones((2, 5), dtype=dt, device="cuda:0"))
