"""The one-workgroup ComplexF64 multi-column tier (csrc/dhqr_small_complex_nrhs.h: k_small_zapply -- H \\ B with several
right-hand sides, Q^H B, Q B and the explicit Q for factors beyond the wave tier up to 128 x 128) on the MI355X, through the
C ABI on guarded device buffers and through the Python front end.  The contracts (zsmall_nrhs_helpers.py):
  a  column r of the multi-column solve has the bytes of the single-column solve on it alone (kernel forced, and the rule)
  b  rows n .. m-1 of Q^H B have the bytes of what the solve leaves there
  c  every column of Q^H B and Q B has the bytes of its own nrhs = 1 call, whatever nrhs, its place in a group, the batch
  d  one call is ONE n_solve group; with DHQR_TUNE zsmall_nrhs=0 the solve is nrhs groups
  e  accuracy: clongdouble reflectors, Q (Q^H B) = B, x against the oracle, form_q == Q [I; 0], A = QR, Q^H Q = I
  f  zsmall_nrhs=0: the solve's bytes unchanged, Q within TOL_Q of the kernel's
  g  guarded layout = packed bytes, sentinels, factor and alpha untouched, the host form leaves B untouched
  h  a non-finite factor stays in its matrix      i  three calls, the same bytes
  j  solve_batched_nrhs, apply_q_batched_ and form_q_batched at (110, 100) equal the C ABI's bytes
at (66, 33), (97, 64) and (128, 128), nrhs 1, CW, CW + 1 and 2 CW + 1, batches 1 and 3, and a batch of 300 at (66, 33)."""
import os

import numpy as np
import pytest

import zapplyq_helpers as Z
import zsmall_nrhs_helpers as S
from zapplyq_helpers import same_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(66, 33), (97, 64), (128, 128)]
CASES = [(nrhs, batch) for nrhs in S.NRHS for batch in S.BATCHES]


@pytest.fixture(scope="module")
def rig(pkg, orc):
    import torch
    assert torch.cuda.is_available()
    L = pkg._lib.lib()
    made = {}
    old = os.environ.get("DHQR_TUNE")
    try:
        for which, tune in (("rule", None), ("kernel", S.TUNE_KERNEL), ("parent", S.TUNE_PARENT)):
            if tune is None:
                os.environ.pop("DHQR_TUNE", None)
            else:
                os.environ["DHQR_TUNE"] = tune
            made[which] = pkg.Context(0)
    finally:
        if old is None:
            os.environ.pop("DHQR_TUNE", None)
        else:
            os.environ["DHQR_TUNE"] = old
    for c in made.values():
        c.use_torch_stream()
        c.set_small_route(True)
    yield S.Rig(L, pkg._lib.Stats, {k: c.handle for k, c in made.items()}, orc, torch=torch)
    for c in made.values():
        c.close()


@pytest.mark.parametrize("m,n", SHAPES)
def test_solve_columns_have_the_bits_of_the_single_column_solve(rig, m, n):
    S.check_solve_column_bits(rig, m, n, CASES)


@pytest.mark.parametrize("m,n", SHAPES)
def test_trans1_tail_has_the_bits_of_the_solve(rig, m, n):
    """b.  Without k_small_zapply this fails: k_batched_zapplyq_general sums in plain double."""
    S.check_tail_bits(rig, m, n, CASES)


@pytest.mark.parametrize("m,n", SHAPES)
def test_columns_are_independent(rig, m, n):
    S.check_column_independence(rig, m, n, CASES)


def test_launch_groups(rig):
    """d.  Without k_small_zapply this fails: the solve is nrhs launches of k_small_zldiv."""
    S.check_launch_groups(rig)


@pytest.mark.parametrize("m,n", SHAPES)
def test_accuracy_and_explicit_q(rig, m, n):
    S.check_accuracy(rig, m, n)


@pytest.mark.parametrize("m,n", SHAPES)
def test_switch_off_keeps_the_solve_and_agrees_on_q(rig, m, n):
    S.check_switch(rig, m, n)


@pytest.mark.parametrize("m,n", SHAPES)
def test_guarded_layout_gives_the_packed_bits(rig, m, n):
    S.check_layout(rig, m, n)


@pytest.mark.parametrize("m,n", SHAPES)
def test_a_zero_column_stays_in_its_matrix(rig, m, n):
    S.check_isolation(rig, m, n)


@pytest.mark.parametrize("m,n", SHAPES)
def test_three_calls_give_the_same_bytes(rig, m, n):
    S.check_repeatable(rig, m, n)


def test_batch_300(rig):
    """(66, 33), nrhs = CW + 1, 600 workgroups per call: every column of the solve has the bytes of the single-column solve,
    the tail of Q^H B the solve's; Q (Q^H B) = B and the clongdouble reflectors on every tenth matrix"""
    m, n, nrhs, batch = 66, 33, S.CW + 1, 300
    mats, Hs, als, Bs = rig.factors(m, n, batch=batch)
    c = S.cut(Bs, nrhs)
    h = rig.ctx["kernel"]
    X = rig.solved(h, Hs, als, c)
    W = rig.applied(h, Hs, als, c, 1)
    alone = [rig.single_column(h, Hs, als, Bs, r) for r in range(nrhs)]
    back = rig.batch(Hs, [np.array(W.bmat(k)) for k in range(batch)], als)
    rig.ok(h, back.apply_q(rig.L, h, 0), back)
    for k in range(batch):
        assert same_bytes(W.bmat(k)[n:], X.bmat(k)[n:]), f"tail of matrix {k}"
        for r in range(nrhs):
            assert same_bytes(X.bmat(k)[:, r], alone[r][k]), f"matrix {k} column {r}"
    for k in range(0, batch, 10):
        Z.check_close(W.bmat(k), Z.reflect_clongdouble(Hs[k], c[k], 1), f"batch 300 Q^H B matrix {k}")
        Z.check_close(back.bmat(k), c[k], f"batch 300 Q (Q^H B) matrix {k}")


def _to_dev(torch, mats):
    """(batch, rows, cols) device tensor with column-major matrices holding the host matrices"""
    batch, (rows, cols) = len(mats), mats[0].shape
    A = torch.empty((batch, cols, rows), dtype=torch.complex128, device=DEV).transpose(1, 2)
    A.copy_(torch.from_numpy(np.stack(mats)))
    return A


def test_python_functions_equal_the_c_abi(pkg, rig):
    """j: solve_batched_nrhs, apply_q_batched_ and form_q_batched on device tensors at (110, 100): the C ABI's bytes"""
    torch = rig.torch
    m, n, nrhs = 110, 100, S.CW + 1
    mats, Hs, als, Bs = rig.factors(m, n)
    c = S.cut(Bs, nrhs)
    X, QhB, QB, Qs = rig.all_results(rig.ctx["rule"], Hs, als, c)
    ctx = pkg.get_context(0)
    ctx.use_torch_stream()
    ctx.set_small_route(True)
    try:
        H = pkg.DistributedHouseholderQRStruct(_to_dev(torch, Hs), torch.from_numpy(np.stack(als)).to(DEV))
        B = _to_dev(torch, c)
        B0 = B.clone()
        Xd = pkg.solve_batched_nrhs(H, B)
        assert torch.equal(B, B0), "B must not be modified"
        Qd = pkg.form_q_batched(H)
        W1 = pkg.apply_q_batched_(H, B.clone().transpose(1, 2).contiguous().transpose(1, 2), True)
        W0 = pkg.apply_q_batched_(H, B.clone().transpose(1, 2).contiguous().transpose(1, 2), False)
        for k in range(len(Hs)):
            assert same_bytes(Xd[k].cpu().numpy(), X[k][:n]), k
            assert same_bytes(W1[k].cpu().numpy(), QhB[k]) and same_bytes(W0[k].cpu().numpy(), QB[k]), k
            assert same_bytes(Qd[k].cpu().numpy(), Qs[k]), k
    finally:
        ctx.set_small_route(False)
