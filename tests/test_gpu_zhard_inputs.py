"""The ComplexF64 small-matrix kernels on the MI355X on inputs the seeded generator never produces (zhard_inputs.py): signed
parts, 2^+-500, parts 2^60 apart, a part identically zero away from magnitude one, graded by column and by row, nearly of rank
one, triangular, with a zero pivot and a zero column.  The wave-per-matrix kernels (csrc/dhqr_batched_complex.h,
dhqr_batched_complex_nrhs.h), the one-workgroup tier (csrc/dhqr_small_complex.h, dhqr_small_complex_nrhs.h) and the complex
half of dhqr_batched_applyq.h through qr_batched_ / ldiv_batched / solve_batched_nrhs / apply_q_batched_ / form_q_batched /
form_r_batched on device tensors, under the criteria Z1-Z6 of zhard_inputs.py -- each evaluated on the reference first -- and
a sweep of 1 x 1 matrices over the exponent range and over parts up to 2^60 apart.  What the GPU build makes of zalphafactor
(hypot, the phase), zdiv (Smith's division), f = 1 / sqrt(sn (sn + |h|)), the four-fma conj-dot and the double-double carry of
the solve -- DPP reductions, register select chains, the compiler's contraction of the fma chains, the hardware's hypot, sqrt
and division -- is seen by no other test: every other complex test draws both parts from [0, 1).

Measured on the MI355X when the file was written (worst ratio to the bound, reference | kernel; 157 tests in 21 to 24 s).  Wave tier,
64 matrices per class: Z1 against the oracle in the classes of magnitude one, 2^+-500 and triangular 1.87 | 0.80; Z2 0.18 | 0.18
(QR) and 0.05 | 0.05 (|v|^2); Z3 x below 0.001 of 1e-9 on both sides, residual 0.017 | 0.012, tail 0.69 | 0.69
against the oracle's factor and 0.001 | below 0.001 against the factor's own (rowgraded_up, lowrank).  One-workgroup tier, 8
matrices: Z1 1.66 | 1.33 (one matrix of eight above T on either side), Z2 0.04 | 0.04 and 0.011 | 0.012, residual 0.003 | 0.001,
tail 0.35 | 0.35.  Z4 and Z6 bit for bit everywhere; factor(iA) against i factor(A) in the classes of magnitude one, 2^+-500 and
triangular 2.00 | 0.97 (wave) and 1.01 | 0.95 (one-workgroup): every matrix of the kernels' inside T, none needed the long-double
restatement.  The sweep: alpha 0.69 | 0.53 of 2 eps, |v|^2 0.05 | 0.06, x 0.10 | 0.11.  Apply-Q: Q (Q^H B) - B 0.16 | 0.15
of T max|B|, A - QR and Q^H Q - I 0.27 | 0.30 and 0.20 | 0.28 of T.
THE FINDING of this file is the reference's, not the kernels'.  The reference forms the phase of alpha as -exp(i angle(h)); the
rounded angle leaves an absolute error of 1e-16 in the small part of the phase, and with parts 2^60 apart (re_heavy, im_heavy,
real_only, imag_only) that error grows with every column: the oracle, and its numpy restatement with it, is up to 800 T (wave
tier) and 185 000 T (128 x 128) from a restatement that forms -h / |h| as the kernels do, its factor of iA up to 239 000 T from i
times its factor of A -- where the kernels' is bit for bit i times theirs (0 | 0 T).  In 25 of the 36 (shape, class) pairs of
those classes the kernel misses Z1 against the oracle with the oracle's own restatements, and is judged under the same rule
against the restatement in np.clongdouble instead: 0.07 | 0.07 T (wave), 0.04 | 0.03 T (one-workgroup).  So is the tail of Q^H
b in four of those pairs.  The classes of magnitude one, 2^+-500 and triangular were judged against the oracle at every shape on
this seed; zhard_inputs.py tells how the seed was chosen.
What the file can and cannot see (each tried on a scratch copy of csrc/ under emulation, test_emulated_zhard_inputs.py):
zalphafactor(0) returning 0 fails the `degenerate` class on both tiers (the zero-pivot matrix is not finite); the sign of the
imaginary part of zalphafactor flipped fails Z1 of `signed` (1e14 T) on both tiers, the sweep (alpha) and the apply-Q check; zdiv
without its second branch fails `imag_only` on both tiers (x not finite: the first branch divides by the zero real part) and
no other class -- zbatched_helpers.special_matrices sends zdiv a zero real part at magnitude one only; the final NaN store
of k_small_zqr dropped fails `degenerate` on the one-workgroup tier (the non-finite pattern of the zero-column matrix);
zcdot_acc without its conjugate fails Z1 of `signed` (1e14 T) on both tiers and the apply-Q check.  hypot
replaced by sqrt(x^2 + y^2) fails nothing, as expected: inside 2^+-500 no square overflows or underflows to a denormal that
matters, and beyond it the column norm itself does.
"""
import numpy as np
import pytest

import zhard_inputs as ZH

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WAVE_SHAPES = [(5, 3), (16, 8), (33, 9), (40, 17), (64, 32), (32, 32)]  # all three NC instantiations, m = 64 filling the wave, m = n
ONE_WG_SHAPES = [(66, 33), (97, 64), (128, 128)]
WAVE_BATCH, ONE_WG_BATCH = 64, 8
# (m, n, K of the column loop, K of the multi-column kernel): see test_several_right_hand_sides
NRHS_CASES = [(16, 8, 3, 4, WAVE_BATCH), (33, 9, 7, 4, WAVE_BATCH), (64, 32, 7, 4, WAVE_BATCH), (66, 33, 7, 6, ONE_WG_BATCH),
              (128, 128, 7, 6, ONE_WG_BATCH)]
APPLY_CASES = [(16, 8, WAVE_BATCH), (33, 9, WAVE_BATCH), (64, 32, WAVE_BATCH), (66, 33, ONE_WG_BATCH), (128, 128, ONE_WG_BATCH)]


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
    """zhard_inputs' backend on api.py: host arrays up, the api on device tensors, results down"""

    def __init__(self, pkg, torch):
        self.pkg, self.torch = pkg, torch

    def up(self, A):
        """(batch, rows, cols) numpy -> a device tensor (its own memory, an empty_colmajor_batched_c layout)"""
        W = self.pkg.empty_colmajor_batched_c(A.shape[0], A.shape[1], A.shape[2], DEV)
        W.copy_(self.torch.from_numpy(np.ascontiguousarray(A)))
        return W

    def down(self, X):
        return np.ascontiguousarray(X.cpu().numpy())

    def struct(self, H, al):
        return self.pkg.DistributedHouseholderQRStruct(self.up(H), self.torch.from_numpy(np.ascontiguousarray(al)).to(DEV))

    def factor(self, A):
        H = self.pkg.qr_batched_(self.up(A))
        return self.down(H.A), self.down(H.α)

    def solve(self, H, al, b):
        if b.ndim == 2:
            return self.down(self.pkg.ldiv_batched(self.struct(H, al), self.torch.from_numpy(np.ascontiguousarray(b)).to(DEV)))
        return self.down(self.pkg.solve_batched_nrhs(self.struct(H, al), self.up(b)))

    def solve_full(self, H, al, b):
        """x from ldiv_batched; rows n .. m-1 of Q^H b from apply_q_batched_, which the api promises to have the bits of what the
        solve leaves there (test_gpu_zapplyq.py, test_gpu_small_znrhs.py assert it)"""
        n = H.shape[2]
        return self.solve(H, al, b), np.ascontiguousarray(self.apply_q(H, al, b[:, :, None], True)[:, n:, 0])

    def apply_q(self, H, al, B, trans):
        return self.down(self.pkg.apply_q_batched_(self.struct(H, al), self.up(B), trans))

    def form_q(self, H, al):
        return self.down(self.pkg.form_q_batched(self.struct(H, al)))

    def form_r(self, H, al):
        return self.down(self.pkg.form_r_batched(self.struct(H, al)))


def _class_case(pkg, orc, torch, tier, m, n, batch, cls):
    be = Device(pkg, torch)
    r = ZH.check_class(be, orc, cls, m, n, batch, tier)
    if cls == "degenerate":
        ZH.check_degenerate_neighbours(be, orc, m, n, batch, tier, r)
    return be, r


def _mixed_case(pkg, orc, torch, tier, m, n, batch):
    be = Device(pkg, torch)
    results = {cls: ZH.run(be, *ZH.make(orc, cls, m, n, batch)) for cls in ZH.CLASSES}  # (each class in a batch of its own)
    ZH.check_mixed(be, orc, m, n, tier, results)


@pytest.mark.parametrize("cls", ZH.CLASSES)
@pytest.mark.parametrize("m,n", WAVE_SHAPES)
def test_wave_tier(pkg, orc, torch_cuda, small_route, m, n, cls):
    """Z1-Z5 on 64 matrices of one class, one wave per matrix"""
    _class_case(pkg, orc, torch_cuda, "wave", m, n, WAVE_BATCH, cls)


@pytest.mark.parametrize("m,n", WAVE_SHAPES)
def test_wave_tier_mixed_batch(pkg, orc, torch_cuda, small_route, m, n):
    """Z6: 2^500 and 2^-500, non-finite and graded matrices in neighbouring waves of one launch"""
    _mixed_case(pkg, orc, torch_cuda, "wave", m, n, WAVE_BATCH)


def test_one_by_one_sweep(pkg, orc, torch_cuda, small_route):
    """20000 1 x 1 matrices, e through [-500, 500], the parts up to 2^60 apart either way: alpha = -a, |v|^2 = 2, x = b / a"""
    ZH.check_sweep(Device(pkg, torch_cuda), orc, 20000, "wave")


@pytest.mark.parametrize("cls", ZH.CLASSES)
@pytest.mark.parametrize("m,n", ONE_WG_SHAPES)
def test_one_workgroup_tier(pkg, orc, torch_cuda, small_route, m, n, cls):
    """Z1-Z5 on 8 matrices of one class, one workgroup per matrix; matrix 0 alone through qr_ / ldiv has the batch's bits"""
    torch = torch_cuda
    be, r = _class_case(pkg, orc, torch, "one-workgroup", m, n, ONE_WG_BATCH, cls)
    H1 = pkg.qr_(be.up(r.A[:1])[0])
    x1 = pkg.ldiv(H1, torch.from_numpy(r.b[0]).to(DEV))
    assert ZH.same(be.down(H1.A), r.H[0]) and ZH.same(be.down(H1.α), r.al[0]) and ZH.same(be.down(x1), r.x[0])


@pytest.mark.parametrize("m,n", ONE_WG_SHAPES)
def test_one_workgroup_tier_mixed_batch(pkg, orc, torch_cuda, small_route, m, n):
    _mixed_case(pkg, orc, torch_cuda, "one-workgroup", m, n, ONE_WG_BATCH)


@pytest.mark.parametrize("m,n,loop,kernel,batch", NRHS_CASES)
def test_several_right_hand_sides(pkg, orc, torch_cuda, small_route, m, n, loop, kernel, batch):
    """column r of solve_batched_nrhs(H, B) has the bits of ldiv_batched(H, B[..., r]), and H \\ B is odd in B, on hard classes.
    Wave tier: the library's rule (znrhs_wave_pays: at least four columns in full groups of 1 | 2 | 4 for n <= 8 | 16 | 32) sends
    K = 4 to k_batched_zldiv_wave_nrhs at every shape (zapplyq_helpers.RULE_NRHS) and K = 7 -- K = 3 for n <= 8, where every
    K >= 4 is full groups (zapplyq_helpers.nrhs_list) -- to the column loop over k_batched_zldiv_wave.  One-workgroup tier
    (zsmall_nrhs_pays: one or three groups of six): K = 6 to k_small_zapply, K = 7 to the column loop over k_small_zldiv
    (zsmall_nrhs_helpers.NRHS: CW and CW + 1)."""
    be = Device(pkg, torch_cuda)
    for cls in ("big", "tiny", "lowrank", "degenerate"):
        ZH.check_nrhs(be, orc, cls, m, n, batch, (loop, kernel), "nrhs")


@pytest.mark.parametrize("cls", ["big", "tiny", "re_heavy", "rowgraded_up", "lowrank"])
@pytest.mark.parametrize("m,n,batch", APPLY_CASES)
def test_apply_q_and_explicit_q_and_r(pkg, orc, torch_cuda, small_route, m, n, batch, cls):
    """A = QR and Q^H Q = I with Q and R each judged against its own magnitude, R the bytes of the factor, Q (Q^H B) = B,
    form_q = apply_q on [I; 0] bit for bit"""
    ZH.check_apply(Device(pkg, torch_cuda), orc, cls, m, n, batch, 5, "apply-Q")
