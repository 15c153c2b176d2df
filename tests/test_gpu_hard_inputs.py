"""The small-matrix kernels on the MI355X on inputs the seeded generator never produces (hard_inputs.py): signed, scaled to
2^+-500 (Float32: 2^+-100), graded by column and by row, nearly of rank one, triangular, with a zero pivot and a zero column.
The wave-per-matrix kernels (csrc/dhqr_batched.h, dhqr_f32.h, dhqr_batched_nrhs.h) and the one-workgroup tier
(csrc/dhqr_small.h) through qr_batched_ / ldiv_batched on device tensors, under the criteria C1-C6 of hard_inputs.py -- each
evaluated on the reference first -- and a sweep of 1 x 1 matrices over the exponent range: what the refinement of the
hardware's reciprocal and reciprocal-square-root estimates gives there is seen by no other test (the CPU emulator defines the
estimates as exact quotients).  One small case each of the general drivers at 2^+-400.

Measured on the MI355X when the file was written (worst ratio to the bound, reference | kernel): wave tier Float64 C1 0 | 0.09,
C2 0.16 | 0.16, C3 0.016 | 0.015; wave tier Float32 0.31 | 0.31, 0.05 | 0.05, 0.12 | 0.12; one-workgroup tier 0 | 0.07,
0.04 | 0.03, 0.003 | 0.001; C4 and C6 bit for bit everywhere.  The sweep: alpha = -a exactly in all 20000 entries of both types;
x within 9.9 ulp (Float64) and 1.6 ulp (Float32) of b / a, which is the rounding of v = sqrt 2 (v^2 enters Q'b), not the division.
One narrowing: the zero-pivot matrix of a SQUARE shape is compared with the oracle on its first n - 1 columns, because the
reference's reflector for h = 0 is a projector and the last pivot of a square matrix is then rounding noise in the oracle too
(hard_inputs.check_class).
What the file can and cannot see (each tried on a scratch copy of csrc/): dhqr_alphafactor(0) = -1 fails the `degenerate`
class (C5, alpha[0] of the zero-pivot matrix) on every tier and type; dropping the final NaN store of k_small_qr_d fails the
same class on the one-workgroup tier (the NaN pattern of the zero-column matrix).  dhqr_rcp without its second Newton step
fails nothing: the correction step behind it (x += (b - a x) / a) hides it, and the batch, column and mixed-batch identities
change alike.  `s2 < 1e300` replaced by `true` fails nothing either: dhqr_sqrt_rsqrt stays accurate until 2 s2 overflows
(max|a| about 2^511), beyond the tested range."""
import numpy as np
import pytest

import hard_inputs as HI

pytestmark = pytest.mark.gpu

WAVE_SHAPES = [(5, 3), (16, 8), (40, 17), (64, 32), (32, 32)]  # all three NC instantiations, m = 64 filling the wave, m = n
NRHS_SHAPES = [(16, 8), (40, 17), (64, 32)]
ONE_WG_SHAPES = [(66, 33), (128, 128), (256, 192)]
WAVE_BATCH, ONE_WG_BATCH = 64, 8


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


class Device:
    """hard_inputs' backend on api.py: host arrays up, qr_batched_ / ldiv_batched on device tensors, results down"""

    def __init__(self, pkg, torch):
        self.pkg, self.torch = pkg, torch

    def up(self, A):
        """(batch, m, n) numpy -> a device tensor (its own memory) whose matrices are column-major"""
        return self.torch.from_numpy(np.ascontiguousarray(A.transpose(0, 2, 1))).to("cuda:0").transpose(1, 2)

    def struct(self, H, al):
        return self.pkg.DistributedHouseholderQRStruct(self.up(H), self.torch.from_numpy(np.ascontiguousarray(al)).to("cuda:0"))

    def factor(self, A):
        H = self.pkg.qr_batched_(self.up(A))
        return np.ascontiguousarray(H.A.cpu().numpy()), H.α.cpu().numpy()

    def solve(self, H, al, b):
        bd = self.torch.from_numpy(np.ascontiguousarray(b)).to("cuda:0") if b.ndim == 2 else self.up(b)
        return np.ascontiguousarray(self.pkg.ldiv_batched(self.struct(H, al), bd).cpu().numpy())


def _class_case(pkg, orc, torch, tier, m, n, batch, t, cls):
    be = Device(pkg, torch)
    r = HI.check_class(be, orc, cls, m, n, batch, t, tier)
    if cls == "degenerate":
        HI.check_degenerate_neighbours(be, orc, m, n, batch, t, tier, r)
    return be, r


def _mixed_case(pkg, orc, torch, tier, m, n, batch, t):
    be = Device(pkg, torch)
    results = {cls: HI.run(be, *HI.make(orc, cls, m, n, batch, t)) for cls in HI.CLASSES}  # (each class in a batch of its own)
    HI.check_mixed(be, orc, m, n, t, tier, results)


@pytest.mark.parametrize("cls", HI.CLASSES)
@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("m,n", WAVE_SHAPES)
def test_wave_tier(pkg, orc, torch_cuda, small_route, m, n, t, cls):
    """C1-C5 on 64 matrices of one class, one wave per matrix"""
    _class_case(pkg, orc, torch_cuda, "wave", m, n, WAVE_BATCH, t, cls)


@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("m,n", WAVE_SHAPES)
def test_wave_tier_mixed_batch(pkg, orc, torch_cuda, small_route, m, n, t):
    """C6: 2^500 and 2^-500 (Float32: 2^+-100), NaN and graded matrices in neighbouring waves of one launch"""
    _mixed_case(pkg, orc, torch_cuda, "wave", m, n, WAVE_BATCH, t)


@pytest.mark.parametrize("t", ["f64", "f32"])
def test_one_by_one_sweep(pkg, orc, torch_cuda, small_route, t):
    """20000 1 x 1 matrices a = +-(1 + u) 2^e, e through [-500, 500] (Float32 [-120, 120]): alpha = -a, v^2 = 2, x = b / a"""
    HI.check_sweep(Device(pkg, torch_cuda), orc, 20000, t, "wave")


@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("m,n", NRHS_SHAPES)
def test_several_right_hand_sides(pkg, orc, torch_cuda, small_route, m, n, t):
    """column r of ldiv_batched(H, B) has the bits of ldiv_batched(H, B[..., r]), and H \\ B is odd in B, on hard classes.
    K = 5: one full group and a remainder for both group widths (the library answers it with the column loop, dhqr.h);
    K = 9 is the smallest of the existing tests' counts that the multi-column kernels of dhqr_batched_nrhs.h themselves run."""
    be = Device(pkg, torch_cuda)
    for cls in ("big", "tiny", "lowrank", "degenerate"):
        for K in (5, 9):
            HI.check_nrhs(be, orc, cls, m, n, WAVE_BATCH, K, t, "wave")


@pytest.mark.parametrize("cls", HI.CLASSES)
@pytest.mark.parametrize("m,n", ONE_WG_SHAPES)
def test_one_workgroup_tier(pkg, orc, torch_cuda, small_route, m, n, cls):
    """C1-C5 on 8 matrices of one class, one workgroup per matrix; matrix 0 alone through qr_ / ldiv has the batch's bits"""
    torch = torch_cuda
    be, r = _class_case(pkg, orc, torch, "one-workgroup", m, n, ONE_WG_BATCH, "f64", cls)
    H1 = pkg.qr_(be.up(r.A[:1])[0])
    x1 = pkg.ldiv(H1, torch.from_numpy(r.b[0]).to("cuda:0"))
    assert HI.same(H1.A.cpu().numpy(), r.H[0]) and HI.same(H1.α.cpu().numpy(), r.al[0]) and HI.same(x1.cpu().numpy(), r.x[0])


@pytest.mark.parametrize("m,n", ONE_WG_SHAPES)
def test_one_workgroup_tier_mixed_batch(pkg, orc, torch_cuda, small_route, m, n):
    _mixed_case(pkg, orc, torch_cuda, "one-workgroup", m, n, ONE_WG_BATCH, "f64")


@pytest.mark.parametrize("e", [0, 400, -400])
@pytest.mark.parametrize("m,n,nb", [(300, 40, 0), (300, 200, 128)])
def test_general_drivers(pkg, orc, torch_cuda, m, n, nb, e):
    """(the suite's default: small route off) the unblocked and the blocked driver on S and S 2^+-400: the factor against the
    oracle's with test_gpu_parity.py's TOL, the solve at its 1e-8"""
    torch = torch_cuda
    A = np.ldexp(HI.signed_matrix(orc, m, n, HI.SEED), e)
    b = 2.0 * orc.rand_vector(m, HI.SEED + 5000) - 1.0
    Ho, ao = orc.householder(np.asfortranarray(A))
    xo = orc.solve(Ho, ao, b)
    H = pkg.qr_(torch.from_numpy(np.ascontiguousarray(A.T)).to("cuda:0").t(), nb=nb)
    x = pkg.ldiv(H, torch.from_numpy(b).to("cuda:0")).cpu().numpy()
    tol, scale = 8.0 * max(n, 8) * np.finfo(np.float64).eps, np.abs(Ho).max()
    eH, ea = np.abs(H.A.cpu().numpy() - Ho).max() / scale, np.abs(H.α.cpu().numpy() - ao).max() / scale
    ex = np.abs(x - xo).max() / np.abs(xo).max()
    print(f"general nb={nb} {m}x{n} S 2^{e}: |dH|={eH:.2e} |dalpha|={ea:.2e} (tol {tol:.2e}) |dx|={ex:.2e} (tol 1e-8)")
    assert np.isfinite(Ho).all() and np.isfinite(xo).all(), "the reference is not finite here: change the input"
    assert eH <= tol and ea <= tol
    assert ex <= 1e-8
