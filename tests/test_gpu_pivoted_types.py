"""Column-pivoted batched QR, the numerical rank and the rank-truncated least squares for Float32 and ComplexF64 on the
MI355X: the checks of pivoted_types_helpers.py (shared with test_emulated_pivoted_types.py) through the C ABI on device
memory -- every buffer of a batch goes to the GPU guards and all and comes back --, one ComplexF64 batch larger than the GPU
holds at once, and the Python front end (factor_pivoted_batched_, rank_pivoted_batched, solve_pivoted_batched,
lstsq_pivoted_batched) against the C ABI's bytes on tensors and on numpy arrays, float64 input against the Float64-only four."""
import numpy as np
import pytest

import pivoted_helpers as PV
import pivoted_types_helpers as PT
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
    yield lambda t: PT.Runner(pkg._lib.lib(), ctx.handle, t, torch_cuda)
    ctx.set_small_route(False)


@pytest.fixture
def run_general(pkg, torch_cuda):
    """the small route off: every shape on the general tier (Float32: promoted)"""
    ctx = pkg.get_context(0)
    ctx.use_torch_stream()
    ctx.set_small_route(False)
    return lambda t: PT.Runner(pkg._lib.lib(), ctx.handle, t, torch_cuda)


@pytest.fixture(scope="module")
def data(orc):
    """the inputs, computed once per type and shape and left unchanged"""
    cache = {}

    def get(t, m, n):
        if (t, m, n) not in cache:
            mats, Bs = PT.inputs(orc, t, m, n)
            for a in mats + Bs:
                a.setflags(write=False)
            cache[(t, m, n)] = (mats, Bs)
        return cache[(t, m, n)]
    return get


def _scipy_qr():
    try:
        import scipy.linalg
        return scipy.linalg.qr
    except ImportError:
        return None


@pytest.mark.parametrize("t", PT.TYPES)
@pytest.mark.parametrize("m,n", PT.WAVE_SHAPES + PT.GENERAL_SHAPES)
def test_pivots_and_factor(run, data, t, m, n):
    PT.check_pivots_and_factor(run(t), *data(t, m, n), scipy_qr=_scipy_qr())


@pytest.mark.parametrize("t", PT.TYPES)
def test_pivots_and_factor_small_route_off(run_general, data, t):
    PT.check_pivots_and_factor(run_general(t), *data(t, 16, 8))


@pytest.mark.parametrize("t", PT.TYPES)
@pytest.mark.parametrize("m,n", PT.WAVE_SHAPES)
def test_wave_tier_bits(run, data, t, m, n):
    PT.check_wave_bits(run(t), *data(t, m, n))


@pytest.mark.parametrize("t", PT.TYPES)
@pytest.mark.parametrize("m,n,r0", PT.LOW_RANK)
def test_rank_and_solve_of_rank_deficient_matrices(run, t, m, n, r0):
    PT.check_solve(run(t), *PT.low_rank_inputs(t, m, n, r0), r0)


@pytest.mark.parametrize("t", PT.TYPES)
@pytest.mark.parametrize("m,n", PT.WAVE_SHAPES + PT.GENERAL_SHAPES)
def test_solve_full_rank(run, data, t, m, n):
    """rcond < 0 (the default bound max(m, n) eps of the type) gives rank n on the full-rank inputs"""
    PT.check_full_rank(run(t), *data(t, m, n))


@pytest.mark.parametrize("t", PT.TYPES)
def test_solve_small_route_off(run_general, data, t):
    PT.check_solve(run_general(t), *data(t, 16, 8), 8)
    PT.check_solve(run_general(t), *PT.low_rank_inputs(t, 16, 8, 3), 3)


@pytest.mark.parametrize("t", PT.TYPES)
def test_degenerate(run, orc, t):
    PT.check_degenerate(run(t), orc)


@pytest.mark.parametrize("t", PT.TYPES)
def test_degenerate_general_tier(run_general, orc, t):
    PT.check_degenerate(run_general(t), orc)


@pytest.mark.parametrize("t", PT.TYPES)
def test_arguments(run, orc, t):
    PT.check_arguments(run(t), orc)


@pytest.mark.parametrize("t", PT.TYPES)
@pytest.mark.parametrize("m,n", [(16, 8), (66, 33)])
def test_profile_counts(pkg, run, orc, t, m, n):
    R = run(t)
    try:
        PT.check_profile_counts(R, orc, m, n, Stats=pkg._lib.Stats)
    finally:
        R.L.dhqr_set_profiling(R.h, 0)


def _tile(torch, mats, batch):
    """(batch, m, n) device tensor with column-major matrices: the given matrices, repeated"""
    m, n = mats[0].shape
    src = torch.from_numpy(np.stack(mats)).cuda()
    A = torch.empty((batch, n, m), dtype=src.dtype, device="cuda:0").transpose(1, 2)
    A.copy_(src.repeat((batch + len(mats) - 1) // len(mats), 1, 1)[:batch])
    return A


def test_more_matrices_than_fit_at_once(pkg, torch_cuda, run, data):
    """(16, 8) ComplexF64 at batch 20000 -- 5000 workgroups --, nrhs 3: matrix k has the bytes of matrix k % 4 of the small
    batch, in the factor, alpha, jpvt, the rank, dB and X; a low-rank matrix among them keeps its own rank"""
    torch, t = torch_cuda, "c64"
    R = run(t)
    m, n, batch = 16, 8, 20000
    mats, Bs = data(t, m, n)
    mats, Bs = list(mats), list(Bs)
    mats[1] = PT.low_rank_inputs(t, m, n, 3)[0][0]
    D = PT.factored(R, mats, Bs)
    R.ok(R.rank(D, PT.RCOND[t]))
    R.ok(R.solve(D))
    assert D.ranks().tolist() == [n, 3, n, n]
    L, h, P = R.L, R.h, PT.P
    A, B = _tile(torch, mats, batch), _tile(torch, Bs, batch)
    al = torch.zeros((batch, n), dtype=A.dtype, device="cuda:0")
    jp = torch.full((batch, n), -9, dtype=torch.int32, device="cuda:0")
    rk = torch.full((batch,), -9, dtype=torch.int32, device="cuda:0")
    X = torch.empty((batch, D.nrhs, n), dtype=A.dtype, device="cuda:0").transpose(1, 2)
    torch.cuda.synchronize()
    p = lambda x: P(x.data_ptr())
    R.ok(L.dhqr_factor_batched_pivoted_c64(h, p(A), m, n, m, m * n, p(al), n, p(jp), n, batch))
    R.ok(L.dhqr_rank_batched_c64(h, p(al), m, n, n, PT.RCOND[t], p(rk), batch))
    R.ok(L.dhqr_solve_batched_pivoted_c64(h, p(A), m, n, m, m * n, p(al), n, p(jp), n, p(rk), p(B), D.nrhs, m, m * D.nrhs, p(X), n,
                                          n * D.nrhs, batch))
    R.sync()
    for k in range(len(mats)):
        for got, want in ((A, D.mat(k)), (al, D.alpha(k)), (jp, D.jpvt(k)), (rk, D.ranks()[k]), (B, D.bmat(k)), (X, D.xmat(k))):
            w = torch.from_numpy(np.ascontiguousarray(want)).cuda()
            assert torch.equal(got[k::len(mats)], w.expand_as(got[k::len(mats)])), k


def _eq(a, b):
    """byte equality of two host arrays that may differ in memory layout"""
    return same_bytes(np.ascontiguousarray(a), np.ascontiguousarray(b))


@pytest.mark.parametrize("t", PT.TYPES)
def test_python_front_end(pkg, torch_cuda, run, data, t):
    """the four typed functions give the C ABI's bytes on tensors and on numpy input, for B (batch, m) and (batch, m, nrhs) and
    for a 2-D A (a batch of one); form_q_batched / form_r_batched / apply_q_batched_ take the pivoted struct unchanged;
    arguments stay as they were"""
    torch = torch_cuda
    R = run(t)
    m, n = 40, 17
    mats, Bs = data(t, m, n)
    mats = list(mats)
    mats[2] = PT.low_rank_inputs(t, m, n, 9)[0][0]
    rc = PT.RCOND[t]
    D = PT.factored(R, mats, Bs)
    R.ok(R.rank(D, rc))
    R.ok(R.solve(D))
    batch = D.batch
    assert D.ranks().tolist() == [n, n, 9, n]
    A_np, B_np = np.stack(mats), np.stack(Bs)
    want_X = np.stack([D.xmat(k) for k in range(batch)])
    for device in (True, False):
        if device:
            A, B = _tile(torch, mats, batch), _tile(torch, Bs, batch)
            host = lambda x: x.cpu().numpy()
        else:
            A, B = A_np.copy(), B_np.copy()
            host = lambda x: np.asarray(x)
        A0, B0 = host(A).copy(), host(B).copy()
        X, rank = pkg.lstsq_pivoted_batched(A, B, rc)
        assert _eq(host(A), A0) and _eq(host(B), B0), "lstsq_pivoted_batched modified its arguments"
        assert _eq(host(X), want_X) and host(rank).tolist() == D.ranks().tolist() and host(rank).dtype == np.int32
        x1, _ = pkg.lstsq_pivoted_batched(A, B[:, :, 1], rc)
        assert _eq(host(x1), want_X[:, :, 1])
        H = pkg.factor_pivoted_batched_(A)
        assert H.jpvt is not None and host(H.jpvt).dtype == np.int32 and host(H.α).dtype == PT.NP[t]
        for k in range(batch):
            assert _eq(host(H.A)[k], D.mat(k)) and _eq(host(H.α)[k], D.alpha(k)) and _eq(host(H.jpvt)[k], D.jpvt(k)), k
        assert host(pkg.rank_pivoted_batched(H, rc)).tolist() == D.ranks().tolist()
        assert host(pkg.rank_pivoted_batched(H)).tolist() == [PT.twin_rank(t, D.alpha(k), -1.0, m) for k in range(batch)]
        HA0 = host(H.A).copy()
        assert _eq(host(pkg.solve_pivoted_batched(H, B, rc)), want_X)
        assert _eq(host(pkg.solve_pivoted_batched(H, B[:, :, 0], rc)), want_X[:, :, 0])
        assert _eq(host(B), B0) and _eq(host(H.A), HA0)
        one = (_tile(torch, mats[:1], 1)[0] if device else A_np[0].copy(order="F"))
        H1 = pkg.factor_pivoted_batched_(one)
        assert tuple(H1.A.shape) == (1, m, n) and _eq(host(H1.A)[0], D.mat(0)) and _eq(host(H1.jpvt)[0], D.jpvt(0))
        if device:
            Qd, Rd = pkg.form_q_batched(H), pkg.form_r_batched(H)
            for k in range(batch):
                jp = D.jpvt(k)
                PT.check_qr(t, host(Qd)[k], host(Rd)[k], D.mat(k), D.alpha(k), mats[k][:, jp], f"{t} form_q / form_r, matrix {k}")
            E = torch.zeros((batch, n, m), dtype=A.dtype, device="cuda:0").transpose(1, 2)
            E.diagonal(dim1=1, dim2=2).fill_(1.0)
            QE = pkg.apply_q_batched_(H, E, False)
            assert torch.equal(QE, Qd)


def test_python_front_end_float64_is_the_old_four(pkg, torch_cuda, run, orc):
    """on float64 input the four typed functions return the bytes of qr_pivoted_batched_, rank_batched, ldiv_pivoted_batched
    and lstsq_batched"""
    torch = torch_cuda
    run("f32")  # (the small route on, as for the other tests)
    m, n = 40, 17
    mats, Bs = PV.inputs(orc, m, n)
    mats[2] = PV.low_rank_inputs(m, n, 9)[0][0]
    for device in (True, False):
        if device:
            mk = lambda: (_tile(torch, mats, len(mats)), _tile(torch, Bs, len(mats)))
            host = lambda x: x.cpu().numpy()
        else:
            mk = lambda: (np.stack(mats), np.stack(Bs))
            host = lambda x: np.asarray(x)
        (A1, B1), (A2, B2) = mk(), mk()
        Xn, rn = pkg.lstsq_pivoted_batched(A1, B1, PV.RCOND)
        Xo, ro = pkg.lstsq_batched(A2, B2, PV.RCOND)
        assert _eq(host(Xn), host(Xo)) and host(rn).tolist() == host(ro).tolist() == [n, n, 9, n]
        Hn, Ho = pkg.factor_pivoted_batched_(A1), pkg.qr_pivoted_batched_(A2)
        assert _eq(host(Hn.A), host(Ho.A)) and _eq(host(Hn.α), host(Ho.α)) and _eq(host(Hn.jpvt), host(Ho.jpvt))
        assert host(pkg.rank_pivoted_batched(Hn)).tolist() == host(pkg.rank_batched(Ho)).tolist()
        assert _eq(host(pkg.solve_pivoted_batched(Hn, B1, PV.RCOND)), host(pkg.ldiv_pivoted_batched(Ho, B2, PV.RCOND)))
        assert _eq(host(pkg.solve_pivoted_batched(Hn, B1[:, :, 0])), host(pkg.ldiv_pivoted_batched(Ho, B2[:, :, 0])))
