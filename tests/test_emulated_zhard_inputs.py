"""The CPU twin of test_gpu_zhard_inputs.py: the input classes and criteria of zhard_inputs.py through the C ABI of the EMULATED
library (csrc/ host-compiled against tests/simt/fake, fiber mode) -- the wave-per-matrix ComplexF64 kernels
(csrc/dhqr_batched_complex.h, dhqr_batched_complex_nrhs.h) at all three NC instantiations, the one-workgroup tier
(csrc/dhqr_small_complex.h, dhqr_small_complex_nrhs.h), the complex half of dhqr_batched_applyq.h.  It proves the inputs, the
reference's preconditions and every piece of arithmetic that is not the hardware's; what the MI355X build makes of the same
code -- DPP reductions, register select chains, the compiler's contraction of the complex fma chains, the hardware's hypot,
sqrt and division -- is seen by the GPU file alone."""
import numpy as np
import pytest

import zapplyq_helpers as Z
import zhard_inputs as ZH
from test_emulated_batched_complex import _ctx, emu  # noqa: F401  (emu: the module fixture)
from zapplyq_helpers import ZNBatch, ZOut
from zbatched_helpers import ZBatch

# Six matrices per class everywhere.  Z1-Z3 and Z5 judge all six; Z4 -- three more factorisations and solves -- takes the first
# two, and in `degenerate` the first three (an ordinary matrix, the zero pivot, the zero column); the mixed batch of Z6
# interleaves matrices 1 and 2 of every class.  The emulator pays half a second for a one-workgroup factorisation (every
# barrier switches fibers through the kernel's threads); the batches of 64 and 8 with all of Z4 and Z6 are the GPU file's.
BATCH = 6
WAVE = [(16, 8), (33, 9), (64, 32)]  # NC = 8, 16, 32
ONE_WG = (66, 33)
ONE_WG_RHS = (70, 8)  # (exactly one chunk of columns, zsmall_nrhs_helpers.SHAPES; at 66 x 33 the emulator takes minutes over these launches)
PACKED = dict(pad_ld=0, pad=0, off=0)
NPACKED = dict(pad_ld=0, pad=0, pad_ldb=0, pad_ldx=0, off=0)


@pytest.fixture(scope="module")
def backend(emu):  # noqa: F811
    h = _ctx(emu)
    yield Emulated(emu, h)
    emu.dhqr_destroy(h)


class Emulated:
    """zhard_inputs' backend on the emulated library: packed ZBatch / ZNBatch / ZOut (lda = m, strideA = m n)"""

    def __init__(self, L, h):
        self.L, self.h = L, h

    def _ok(self, rc):
        assert rc == 0, self.L.dhqr_last_error()
        assert self.L.dhqr_synchronize(self.h) == 0

    def factor(self, A):
        batch, m, n = A.shape
        B = ZBatch(list(A), [np.zeros(m, dtype=np.complex128)] * batch, **PACKED)
        self._ok(B.factor(self.L, self.h))
        return np.stack([B.mat(k) for k in range(batch)]), np.stack([B.alpha(k) for k in range(batch)])

    def solve_full(self, H, al, b):
        batch, m, n = H.shape
        B = ZBatch(list(H), list(b), **PACKED)
        for k in range(batch):
            B.alpha(k)[...] = al[k]
        self._ok(B.solve(self.L, self.h))
        out = np.stack([B.rhs(k) for k in range(batch)])
        return np.ascontiguousarray(out[:, :n]), np.ascontiguousarray(out[:, n:])

    def _nbatch(self, H, al, B):
        return ZNBatch([np.asfortranarray(x) for x in H], [np.asfortranarray(x) for x in B], list(al), **NPACKED)

    def solve(self, H, al, b):
        if b.ndim == 2:
            return self.solve_full(H, al, b)[0]
        D = self._nbatch(H, al, b)
        self._ok(D.solve_nrhs(self.L, self.h))
        return np.stack([D.bmat(k)[:H.shape[2]] for k in range(len(H))])

    def apply_q(self, H, al, B, trans):
        D = self._nbatch(H, al, B)
        self._ok(D.apply_q(self.L, self.h, 1 if trans else 0))
        return np.stack([D.bmat(k) for k in range(len(H))])

    def _formed(self, H, al, rows, call):
        batch, m, n = H.shape
        D = self._nbatch(H, al, [Z.eye_columns(m, 1)] * batch)
        out = ZOut(batch, rows, n, pad_ld=0, pad=0, off=0)
        self._ok(call(D, out))
        return np.stack([out.mat(k) for k in range(batch)])

    def form_q(self, H, al):
        return self._formed(H, al, H.shape[1], lambda D, out: D.form_q(self.L, self.h, out))

    def form_r(self, H, al):
        return self._formed(H, al, H.shape[2], lambda D, out: D.form_r(self.L, self.h, out))


def _what(m, n):
    return "emulated one-workgroup" if (m, n) == ONE_WG else "emulated wave"


@pytest.fixture(scope="module")
def classes(backend, orc):
    """the Result of a (shape, class), computed on first use and left unchanged: judged=True runs check_class (the class
    test), judged=False only needs the numbers (the mixed batch, the neighbours) and runs the kernels where nothing is there"""
    done = {}

    def get(m, n, cls, judged):
        if judged:
            done[m, n, cls] = ZH.check_class(backend, orc, cls, m, n, BATCH, _what(m, n), z4=3 if cls == "degenerate" else 2)
        elif (m, n, cls) not in done:
            done[m, n, cls] = ZH.run(backend, *ZH.make(orc, cls, m, n, BATCH))
        return done[m, n, cls]
    return get


@pytest.mark.parametrize("cls", ZH.CLASSES)
@pytest.mark.parametrize("m,n", WAVE + [ONE_WG])
def test_classes(backend, orc, classes, m, n, cls):
    """Z1-Z5 on one class"""
    r = classes(m, n, cls, True)
    if cls == "degenerate":
        ZH.check_degenerate_neighbours(backend, orc, m, n, BATCH, _what(m, n), r, signed_result=classes(m, n, "signed", False))


@pytest.mark.parametrize("m,n", WAVE + [ONE_WG])
def test_mixed_batch(backend, orc, classes, m, n):
    """Z6: one batch interleaves matrices 1 and 2 of every class, the zero pivot and the zero column among them"""
    ZH.check_mixed(backend, orc, m, n, _what(m, n), {cls: classes(m, n, cls, False) for cls in ZH.CLASSES}, which=[1, 2])


def test_one_by_one_sweep(backend, orc):
    ZH.check_sweep(backend, orc, 512, "emulated")


@pytest.mark.parametrize("m,n,loop,kernel", [(33, 9, 7, 4), ONE_WG_RHS + (7, 6)])
def test_several_right_hand_sides(backend, orc, m, n, loop, kernel):
    """wave tier, n = 9 (groups of two columns): the library's rule sends K = 7 to the column loop over k_batched_zldiv_wave and
    K = 4 to k_batched_zldiv_wave_nrhs (zapplyq_helpers.RULE_NRHS); one-workgroup tier: K = 7 (two groups of six) to the
    column loop over k_small_zldiv, K = 6 (one group) to k_small_zapply (zsmall_nrhs_helpers.NRHS: CW + 1 and CW)"""
    for cls in ("big", "tiny", "lowrank", "degenerate"):
        ZH.check_nrhs(backend, orc, cls, m, n, BATCH, (loop, kernel), "emulated nrhs")


@pytest.mark.parametrize("m,n", [(33, 9), ONE_WG_RHS])
def test_apply_q_and_explicit_q_and_r(backend, orc, m, n):
    for cls in ("big", "tiny", "re_heavy", "rowgraded_up", "lowrank"):
        ZH.check_apply(backend, orc, cls, m, n, BATCH, 5, "emulated apply-Q")
