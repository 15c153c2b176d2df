"""The one-workgroup ComplexF64 multi-column tier (csrc/dhqr_small_complex_nrhs.h: k_small_zapply -- H \\ B with several
right-hand sides, Q^H B, Q B and the explicit Q for factors beyond the wave tier up to 128 x 128) through the C ABI of the
EMULATED library (csrc/ host-compiled against tests/simt/fake, fiber mode).  The contracts (zsmall_nrhs_helpers.py):
  a  column r of the multi-column solve has the bytes of the single-column solve on it alone (kernel forced, and the rule)
  b  rows n .. m-1 of Q^H B have the bytes of what the solve leaves there
  c  every column of Q^H B and Q B has the bytes of its own nrhs = 1 call, whatever nrhs, its place in a group, the batch
  d  one call is ONE n_solve group; with DHQR_TUNE zsmall_nrhs=0 the solve is nrhs groups
  e  accuracy: clongdouble reflectors, Q (Q^H B) = B, x against the oracle, form_q == Q [I; 0], A = QR, Q^H Q = I
  f  zsmall_nrhs=0: the solve's bytes unchanged, Q within TOL_Q of the kernel's
  g  guarded layout = packed bytes, sentinels, factor and alpha untouched, the host form leaves B untouched
  h  a non-finite factor stays in its matrix      i  three calls, the same bytes
Shapes: zsmall_nrhs_helpers.SHAPES; nrhs 1, CW, CW + 1, 2 CW + 1; batches 1 and 3.  The emulator is slow (about 2 ms per
reflector and column of B), so this is the subset that keeps the file to a couple of minutes: the full nrhs x batch grid at
the two one-chunk shapes, one matrix and nrhs = CW + 1 at the four larger ones (item d: three matrices at (66, 33)); (97, 64)
and (128, 128) for the byte contracts a, b and c only; the layout, isolation and repeatability items at (70, 8).
test_gpu_small_znrhs.py runs every item at (66, 33), (97, 64) and (128, 128)."""
import ctypes
import os

import pytest

import zsmall_nrhs_helpers as S
from zapplyq_helpers import P

CW = S.CW
# (nrhs, batch): every nrhs at batch 3, the group-and-tail at batch 1 too | the subset of the larger shapes
FULL = [(nrhs, 3) for nrhs in S.NRHS] + [(1, 1), (CW + 1, 1)]
ONE = [(CW + 1, 1)]
CASES = {(65, 1): FULL, (70, 8): FULL, (66, 33): ONE, (48, 40): ONE, (97, 64): ONE, (128, 128): ONE}
FBATCH = {(66, 33): 1, (48, 40): 1, (97, 64): 1, (128, 128): 1}  # matrices factored per shape (3 elsewhere)


def _ctx(L, tune=None):
    """a context with the small route on; tune: DHQR_TUNE while it is created"""
    env = {"DHQR_SMALL": "1", "DHQR_TUNE": tune}
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        h = P()
        assert L.dhqr_create(ctypes.byref(h), 0) == 0, L.dhqr_last_error()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return h


@pytest.fixture(scope="module")
def rig(emulated_so, orc):
    from dist_helpers import load_emulated_library
    L = load_emulated_library(emulated_so)
    ctx = {"rule": _ctx(L), "kernel": _ctx(L, S.TUNE_KERNEL), "parent": _ctx(L, S.TUNE_PARENT)}
    yield S.Rig(L, L.Stats, ctx, orc, fbatch=FBATCH)
    for h in ctx.values():
        L.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", S.SHAPES)
def test_solve_columns_have_the_bits_of_the_single_column_solve(rig, m, n):
    S.check_solve_column_bits(rig, m, n, CASES[(m, n)])


@pytest.mark.parametrize("m,n", S.SHAPES)
def test_trans1_tail_has_the_bits_of_the_solve(rig, m, n):
    """b.  Without k_small_zapply this fails: k_batched_zapplyq_general sums in plain double."""
    S.check_tail_bits(rig, m, n, CASES[(m, n)])


@pytest.mark.parametrize("m,n", S.SHAPES)
def test_columns_are_independent(rig, m, n):
    S.check_column_independence(rig, m, n, CASES[(m, n)])


def test_launch_groups(rig):
    """d.  Without k_small_zapply this fails: the solve is nrhs launches of k_small_zldiv."""
    S.check_launch_groups(rig)


@pytest.mark.parametrize("m,n", S.SHAPES[:4])
def test_accuracy_and_explicit_q(rig, m, n):
    S.check_accuracy(rig, m, n)


def test_switch_off_keeps_the_solve_and_agrees_on_q(rig):
    S.check_switch(rig, 48, 40)


def test_guarded_layout_gives_the_packed_bits(rig):
    S.check_layout(rig, 70, 8)


def test_a_zero_column_stays_in_its_matrix(rig):
    S.check_isolation(rig, 70, 8)


def test_three_calls_give_the_same_bytes(rig):
    S.check_repeatable(rig, 70, 8)
