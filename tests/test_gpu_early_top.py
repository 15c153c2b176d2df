"""The early top of the panel chain (DHQR_TUNE early_top, csrc/dhqr_dist.h) on the GPU: panels after the first of a step
take their Gram matrix from a downdate and start k_panel_top behind the top rows of the narrow update, the rest of the
rows follows on the side stream.  Against the oracle, against the old chain (early_top=0), twice for bit-identical results
(a missing event wait shows as a difference), and on an input whose downdate is destroyed by cancellation.
Every launch is bounds-checked by construction; no case provokes a fault."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = np.finfo(np.float64).eps
SEED = 9


@contextlib.contextmanager
def _context(pkg, monkeypatch, early):
    """a context of its own with the schedule tests' settings (read by dhqr_create), installed as device 0's for api.py"""
    monkeypatch.setenv("DHQR_PAIR_MIN_N", "0")
    monkeypatch.setenv("DHQR_QUAD_MIN_COLS", "0")
    monkeypatch.setenv("DHQR_TUNE", f"tn_min_tiles=3,early_top={early}")
    ctx = pkg.Context(0)
    ctx.set_small_route(False)
    api = pkg.api
    old = api._contexts.get(0)
    api._contexts[0] = ctx
    try:
        yield ctx
    finally:
        api._contexts.pop(0, None)
        if old is not None:
            api._contexts[0] = old
        ctx.close()


def _factor(pkg, ctx, A0):
    import torch
    ctx.reset_stats()
    H = pkg.qr_(A0.clone(), nb=128)
    torch.cuda.synchronize()
    return H, ctx.panel_counters()


@pytest.mark.parametrize("m,n", [(2048, 2048), (2304, 1536)])
def test_early_top_main(pkg, orc, monkeypatch, m, n):
    """H and alpha against the oracle at 8 n eps (relative to max|H|), the residual at the 1e-12 of the panel-path tests, two
    runs bit-identical, early_top=0 within 8 n eps of early_top=1, no panel redone"""
    A0 = pkg.rand_colmajor(m, n, SEED, DEV)
    Ho, ao = orc.householder(orc.rand_matrix(m, n, SEED))
    scale, tol = np.abs(Ho).max(), 8.0 * n * EPS
    with _context(pkg, monkeypatch, 1) as ctx:
        H1, cnt1 = _factor(pkg, ctx, A0)
        res1 = pkg.residual(H1, A0)
        A1, al1 = H1.A.cpu().numpy(), H1.α.cpu().numpy()
        H1b, _ = _factor(pkg, ctx, A0)
        A1b, al1b = H1b.A.cpu().numpy(), H1b.α.cpu().numpy()
    with _context(pkg, monkeypatch, 0) as ctx:
        H0, cnt0 = _factor(pkg, ctx, A0)
        res0 = pkg.residual(H0, A0)
        A0_, al0 = H0.A.cpu().numpy(), H0.α.cpu().numpy()
    eH, ea = np.abs(A1 - Ho).max() / scale, np.abs(al1 - ao).max() / scale
    d01 = max(np.abs(A1 - A0_).max(), np.abs(al1 - al0).max()) / scale
    print(f"{m} x {n}: |dH| = {eH:.2e}, |dalpha| = {ea:.2e}, |early_top 1 - 0| = {d01:.2e} (bound {tol:.2e}); "
          f"residual {res1:.2e} (early_top=0: {res0:.2e}); counters {cnt1} / {cnt0}")
    assert eH <= tol and ea <= tol
    assert res1 < 1e-12 and res0 < 1e-12
    assert A1.tobytes() == A1b.tobytes() and al1.tobytes() == al1b.tobytes(), "two runs of early_top=1 differ"
    assert d01 <= tol
    assert A1.tobytes() != A0_.tobytes(), "early_top=1 took the old chain"
    assert cnt1 == cnt0 and cnt1[1] == 0


def test_early_top_hard_input(pkg, orc, monkeypatch):
    """1024 x 512 whose columns 128..255 are columns 0..127 times a fixed random matrix plus 1e-9 x noise (the matrix of
    tests/test_early_top_cpu.py: the oracle and early_top=0 pass it on the emulator).  The downdate of the second panel is
    destroyed by cancellation: the call must return OK with the residual bound early_top=0 meets; the bad Gram matrix may
    cost that one panel its first attempt, nothing else"""
    import torch
    from test_early_top_cpu import hard_matrix
    Ah = hard_matrix(orc)
    A0 = torch.from_numpy(np.ascontiguousarray(Ah.T)).to(DEV).T  # column-major on the device
    assert A0.stride() == (1, Ah.shape[0])
    out = {}
    for early in (0, 1):
        with _context(pkg, monkeypatch, early) as ctx:
            H, (fast, fb) = _factor(pkg, ctx, A0)
            out[early] = (pkg.residual(H, A0), fast, fb)
        print(f"early_top={early}: residual {out[early][0]:.2e}, fast {fast}, fallback {fb}")
    for early in (0, 1):
        res, fast, fb = out[early]
        assert res < 1e-12
        assert fb <= 1 and fast + fb == 4
