"""The CPU twin of test_gpu_hard_inputs.py: the input classes and criteria of hard_inputs.py through the C ABI of the EMULATED
library (csrc/ host-compiled against tests/simt/fake, fiber mode) -- the wave-per-matrix kernels in Float64 and Float32, the
several-right-hand-sides kernels, the one-workgroup tier.  It proves the inputs, the reference's preconditions and every piece
of arithmetic that is not the hardware's: the emulator defines the reciprocal and reciprocal-square-root estimates as exact
quotients, so what the refinement makes of the real estimates is seen by the GPU file alone."""
import ctypes

import numpy as np
import pytest

import hard_inputs as HI
from test_emulated_batched import _ctx

P = ctypes.c_void_p
BATCH = 6
WAVE = [(16, 8), (40, 17), (64, 32)]


def _ptr(a):
    return a.ctypes.data_as(P)


@pytest.fixture(scope="module")
def emu(emulated_so):
    from dist_helpers import load_emulated_library
    return load_emulated_library(emulated_so)


@pytest.fixture(scope="module")
def backend(emu):
    h = _ctx(emu)
    yield Emulated(emu, h)
    emu.dhqr_destroy(h)


def _packed(A):
    """(batch, m, n) -> flat buffer with matrix k column-major at k m n"""
    return np.array(A.transpose(0, 2, 1), order="C", copy=True).reshape(-1)  # (always a copy: the calls work in place)


def _unpacked(flat, batch, m, n):
    return np.ascontiguousarray(flat.reshape(batch, n, m).transpose(0, 2, 1))


class Emulated:
    """hard_inputs' backend on the emulated library: packed batches (lda = m, strideA = m n)"""

    def __init__(self, L, h):
        self.L, self.h = L, h

    def _fn(self, name, a):
        return getattr(self.L, f"{name}_{'f32' if a.dtype == np.float32 else 'f64'}")

    def _ok(self, rc):
        assert rc == 0, self.L.dhqr_last_error()
        assert self.L.dhqr_synchronize(self.h) == 0

    def factor(self, A):
        batch, m, n = A.shape
        fa, al = _packed(A), np.zeros(batch * n, dtype=A.dtype)
        self._ok(self._fn("dhqr_factor_batched", A)(self.h, _ptr(fa), m, n, m, m * n, _ptr(al), n, batch, 0))
        return _unpacked(fa, batch, m, n), al.reshape(batch, n)

    def solve(self, H, al, b):
        batch, m, n = H.shape
        fa, fal = _packed(H), np.ascontiguousarray(al)
        if b.ndim == 2:
            fb = np.array(b, order="C")
            self._ok(self._fn("dhqr_solve_batched", H)(self.h, _ptr(fa), m, n, m, m * n, _ptr(fal), n, _ptr(fb), m, batch))
            return np.ascontiguousarray(fb[:, :n])
        K = b.shape[2]
        fb = _packed(b)
        self._ok(self._fn("dhqr_solve_batched_nrhs", H)(self.h, _ptr(fa), m, n, m, m * n, _ptr(fal), n, _ptr(fb), K, m, m * K, batch))
        return np.ascontiguousarray(_unpacked(fb, batch, m, K)[:, :n, :])


@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("m,n", WAVE)
def test_wave_tier_classes(backend, orc, m, n, t):
    """C1-C6 on every class, six matrices each, and one mixed batch of all of them"""
    results = {cls: HI.check_class(backend, orc, cls, m, n, BATCH, t, "emulated wave") for cls in HI.CLASSES}
    HI.check_degenerate_neighbours(backend, orc, m, n, BATCH, t, "emulated wave", results["degenerate"])
    HI.check_mixed(backend, orc, m, n, t, "emulated wave", results)


@pytest.mark.parametrize("t", ["f64", "f32"])
@pytest.mark.parametrize("m,n", WAVE)
def test_several_right_hand_sides(backend, orc, m, n, t):
    """K = 5 is answered by the column loop (dhqr.h), K = 9 by the multi-column kernels of dhqr_batched_nrhs.h"""
    for cls in ("big", "tiny", "lowrank", "degenerate"):
        for K in (5, 9):
            HI.check_nrhs(backend, orc, cls, m, n, BATCH, K, t, "emulated nrhs")


def test_one_workgroup_tier_classes(backend, orc):
    m, n = 66, 33
    results = {cls: HI.check_class(backend, orc, cls, m, n, BATCH, "f64", "emulated one-workgroup") for cls in HI.CLASSES}
    HI.check_degenerate_neighbours(backend, orc, m, n, BATCH, "f64", "emulated one-workgroup", results["degenerate"])
    HI.check_mixed(backend, orc, m, n, "f64", "emulated one-workgroup", results)


@pytest.mark.parametrize("t", ["f64", "f32"])
def test_one_by_one_sweep(backend, orc, t):
    HI.check_sweep(backend, orc, 512, t, "emulated")
