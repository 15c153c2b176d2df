"""`H_k \\ B_k` with several right-hand sides (dhqr_solve_batched_nrhs_f64 / _f32, dhqr_ldiv_batched_nrhs_f64 / _f32) through
the C ABI of the EMULATED library (csrc/ host-compiled against tests/simt/fake, fiber mode): every column bit for bit
against today's single-column call on every route, against the oracle, on padded / strided / guarded layouts, the launch-group
counts, the host forms, the argument rules, repeatability; the Python front end's argument errors that need no device."""
import ctypes
import os

import numpy as np
import pytest

import f32_helpers as F
import layout_helpers as LH
import nrhs_helpers as N
from nrhs_helpers import NBatch, P, ptr, same_bytes


@pytest.fixture(scope="module")
def emu(emulated_so):
    from dist_helpers import load_emulated_library
    return load_emulated_library(emulated_so)


def _ctx(L, small=1):
    old = os.environ.get("DHQR_SMALL")
    os.environ["DHQR_SMALL"] = str(small)
    try:
        h = P()
        assert L.dhqr_create(ctypes.byref(h), 0) == 0, L.dhqr_last_error()
    finally:
        if old is None:
            os.environ.pop("DHQR_SMALL", None)
        else:
            os.environ["DHQR_SMALL"] = old
    return h


def _n_solve(L, h):
    st = L.Stats()
    assert L.dhqr_get_stats(h, ctypes.byref(st)) == 0
    return st.n_solve


def _factored(emu, h, orc, m, n, nrhs, batch, t, seed=N.SEED, **layout):
    mats, Bs = N.inputs(orc, m, n, nrhs, batch, seed, t)
    D = NBatch(mats, Bs, t, **layout)
    assert D.factor(emu, h) == 0, emu.dhqr_last_error()
    assert emu.dhqr_synchronize(h) == 0
    return D, mats, Bs


@pytest.fixture(scope="module")
def wave_reference(emu, orc):
    """computed once per (shape, dtype), shared and left unchanged: the factors (H_k, alpha_k) of a batch of 5, its B_k and,
    for each of N.NRHS_MAX columns, what today's single-column call returns for that column alone ((5, m) arrays)"""
    cache = {}

    def get(m, n, t):
        if (m, n, t) not in cache:
            h = _ctx(emu)
            D, mats, Bs = _factored(emu, h, orc, m, n, N.NRHS_MAX, 5, t, pad_ld=0, pad=0, pad_ldb=0)
            cols = [D.single_column(emu, h, r, Bs) for r in range(N.NRHS_MAX)]
            Hs, als = [np.array(D.mat(k)) for k in range(5)], [D.alpha(k).copy() for k in range(5)]
            for c in cols + Hs + als + Bs:
                c.setflags(write=False)
            emu.dhqr_destroy(h)
            cache[(m, n, t)] = (Hs, als, Bs, cols)
        return cache[(m, n, t)]
    return get


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n", N.WAVE_SHAPES)
def test_wave_tier_columns_bit_for_bit(emu, orc, wave_reference, m, n, t):
    """criterion 1 on the wave tier: column r of an nrhs = 1, 3, 4, 5, 9 (and 8, 13: N.NRHS_KERNEL_TAILS) call -- all m rows, x and the tail of Q'b -- has the
    bytes of k_batched_ldiv_wave(_s) on that column alone, whatever nrhs, the column's place in its group and the batch
    (5, and its first matrix alone); B padded (ldb = m + 3, strideB > ldb nrhs), the padding untouched"""
    Hs, als, Bs, cols = wave_reference(m, n, t)
    h = _ctx(emu)
    for nrhs in N.NRHS_ALL:
        for batch in ((5, 1) if nrhs in N.NRHS else (5,)):
            D = NBatch(Hs[:batch], [B[:, :nrhs] for B in Bs[:batch]], t, pad_ldb=3)
            for k in range(batch):
                D.alpha(k)[...] = als[k]
            assert D.solve_nrhs(emu, h) == 0, emu.dhqr_last_error()
            assert emu.dhqr_synchronize(h) == 0
            for k in range(batch):
                for r in range(nrhs):
                    assert same_bytes(D.bmat(k)[:, r], cols[r][k]), f"nrhs {nrhs} batch {batch}: matrix {k} column {r}"
            assert D.padding_intact() and D.x_untouched()
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
def test_wave_tier_batch_300(emu, orc, t):
    """75 workgroups: nrhs = 4 (one full group: the multi-column kernel), every column of every matrix ((5, 3): the emulator steps every lane through every cross-lane
    operation, and the larger shapes at this batch are test_gpu_nrhs.py's)"""
    m, n, nrhs, batch = 5, 3, 4, 300
    h = _ctx(emu)
    D, mats, Bs = _factored(emu, h, orc, m, n, nrhs, batch, t)
    cols = [D.single_column(emu, h, r, Bs) for r in range(nrhs)]
    assert D.solve_nrhs(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    for k in range(batch):
        assert same_bytes(D.bmat(k), np.stack([cols[r][k] for r in range(nrhs)], axis=1)), k
    assert D.padding_intact()
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n", N.WAVE_SHAPES)
def test_wave_tier_against_the_oracle(emu, orc, m, n, t):
    """criterion 2, independent of criterion 1.  Float64: |X[:, r] - orc.solve(H, alpha, B[:, r])| / |x| <= 1e-9 with the
    oracle's own factor (the bound of test_gpu_batched._against_oracle); the plain-double numpy twin stays inside it at these
    seeds.  Float32: F.check_solve's 4 EPS32 on the kernel's own factor, widened.  The device form leaves the tail of Q'B
    below X (numpy reflectors on the kernel's factor: 1e-12 like test_emulated_batched, 4 EPS32 of max|Q'b| in Float32)."""
    nrhs, batch = 9, 5  # (the multi-column kernel: N.NRHS_KERNEL_TAILS)
    h = _ctx(emu)
    D, mats, Bs = _factored(emu, h, orc, m, n, nrhs, batch, t)
    Hk = [np.array(D.mat(k), order="F") for k in range(batch)]
    alk = [D.alpha(k).copy() for k in range(batch)]
    assert D.solve_nrhs(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    X = [np.array(D.bmat(k)[:n], dtype=np.float64) for k in range(batch)]
    if t == "f64":
        worst, twin = N.oracle_errors(orc, mats, Bs, X)
        print(f"{m}x{n} nrhs {nrhs}: |dx|/|x| = {worst:.2e}, twin {twin:.2e} (tol 1e-9)")
        assert twin <= 1e-9, "the numpy twin misses the bound at these seeds: change the seed"
        assert worst <= 1e-9
    else:
        for r in range(nrhs):
            F.check_solve(orc, np.stack(Hk), np.stack(alk), np.stack([B[:, r] for B in Bs]),
                          np.stack([D.bmat(k)[:n, r] for k in range(batch)]), range(batch), f"column {r}")
    if m > n:
        for k in range(batch):
            q = Bs[k].astype(np.float64)
            Hd = Hk[k].astype(np.float64)
            for j in range(n):
                q[j:] -= np.outer(Hd[j:, j], Hd[j:, j] @ q[j:])
            tol = (1e-12 if t == "f64" else 4 * F.EPS32) * max(1.0, np.abs(q).max())
            assert np.abs(D.bmat(k)[n:] - q[n:]).max() <= tol
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n,batch", N.BEYOND)
def test_beyond_the_wave_tier_is_one_existing_solve_per_column(emu, orc, m, n, batch, t):
    """criteria 1 and 5 beyond the wave tier (one-workgroup tier, serial tier): the bytes of today's call on each column and
    the profiling counts of nrhs such calls -- (66, 33), nrhs = 3 adds three n_solve"""
    nrhs = 3
    h = _ctx(emu)
    D, mats, Bs = _factored(emu, h, orc, m, n, nrhs, batch, t)
    assert emu.dhqr_set_profiling(h, 1) == 0 and emu.dhqr_reset_stats(h) == 0
    cols = [D.single_column(emu, h, r, Bs) for r in range(nrhs)]
    singles = _n_solve(emu, h)
    assert emu.dhqr_reset_stats(h) == 0
    assert D.solve_nrhs(emu, h) == 0, emu.dhqr_last_error()
    assert emu.dhqr_synchronize(h) == 0
    assert _n_solve(emu, h) == singles
    if m <= 256:
        assert singles == nrhs  # one launch per column, whatever the batch
    for k in range(batch):
        for r in range(nrhs):
            assert same_bytes(D.bmat(k)[:, r], cols[r][k]), (k, r)
    assert D.padding_intact()
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
def test_small_route_off_everything_is_looped(emu, orc, t):
    """with the small route off a wave-tier shape takes the column loop too: the bytes and counts of the single-column calls"""
    m, n, nrhs, batch = 16, 8, 3, 2
    h = _ctx(emu, small=0)
    D, mats, Bs = _factored(emu, h, orc, m, n, nrhs, batch, t)
    assert emu.dhqr_set_profiling(h, 1) == 0 and emu.dhqr_reset_stats(h) == 0
    cols = [D.single_column(emu, h, r, Bs) for r in range(nrhs)]
    singles = _n_solve(emu, h)
    assert emu.dhqr_reset_stats(h) == 0
    assert D.solve_nrhs(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    assert _n_solve(emu, h) == singles == nrhs * batch
    for k in range(batch):
        for r in range(nrhs):
            assert same_bytes(D.bmat(k)[:, r], cols[r][k])
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
def test_launch_groups(emu, orc, t):
    """criterion 5: a wave-tier call with nrhs = 9, batch 7 adds exactly ONE n_solve"""
    h = _ctx(emu)
    D, mats, Bs = _factored(emu, h, orc, 16, 8, 9, 7, t)
    assert emu.dhqr_set_profiling(h, 1) == 0 and emu.dhqr_reset_stats(h) == 0
    assert D.solve_nrhs(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    assert _n_solve(emu, h) == 1
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n", [(16, 8), (40, 17), (66, 33)])
def test_host_forms(emu, orc, m, n, t):
    """criteria 3, 4, 7 at the C ABI: the host form returns the device form's X, leaves hB bit-identical, writes nothing
    outside the n x nrhs windows of X (ldx > n; strideX with and without a gap) or anywhere else"""
    nrhs, batch = 9, (4 if m <= 64 else 2)
    h = _ctx(emu)
    D, mats, Bs = _factored(emu, h, orc, m, n, nrhs, batch, t)
    Hf = D.A.copy()
    assert D.solve_nrhs(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    layouts = (dict(), dict(pad=0, pad_ld=0, pad_ldb=0), dict(pad=0, pad_ldx=3), dict(pad_ldb=3, pad_ldx=0))
    for lay in (layouts if m <= 64 else layouts[:2]):
        Hb = NBatch(mats, Bs, t, **lay)
        for k in range(batch):  # the factor computed above
            Hb.mat(k)[...] = D.mat(k)
            Hb.alpha(k)[...] = D.alpha(k)
        A0, B0 = Hb.A.copy(), Hb.B.copy()
        assert Hb.ldiv_nrhs(emu, h) == 0, emu.dhqr_last_error()
        assert same_bytes(Hb.B, B0), "hB must not be modified"
        assert same_bytes(Hb.A, A0)
        for k in range(batch):
            assert same_bytes(Hb.xmat(k), D.bmat(k)[:n]), (lay, k)
        assert Hb.padding_intact()
    assert same_bytes(D.A, Hf)
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
def test_guarded_layouts(emu, orc, t):
    """criterion 4 on NaN-guarded buffers, a single matrix (batch = 1): ldb = m + 1 and m + 3, ldx > n, a base 8 bytes off a
    16-byte boundary (Float32: 4 bytes off an 8-byte boundary); the packed layout's bytes, every guard word intact"""
    m, n, nrhs = 33, 9, 9
    h = _ctx(emu)
    D, mats, Bs = _factored(emu, h, orc, m, n, nrhs, 1, t, pad_ld=0, pad=0, pad_ldb=0)
    H0, a0 = np.array(D.mat(0), order="F"), D.alpha(0).copy()
    assert D.solve_nrhs(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    want = np.array(D.bmat(0))
    if t == "f64":
        guarded = lambda r, c, ld, off, content=None: LH.guarded_matrix(r, c, ld, off, content=content)
        intact = LH.assert_guards_intact
    else:
        guarded = lambda r, c, ld, off, content=None: F.guarded_f32(r, c, ld, off, content=content)
        intact = F.assert_f32_guards_intact
    solve, ldiv = getattr(emu, f"dhqr_solve_batched_nrhs_{t}"), getattr(emu, f"dhqr_ldiv_batched_nrhs_{t}")
    for pad, off in ((1, 0), (3, 0), (1, 1), (3, 1)):
        gA, gal = guarded(m, n, m + pad, off, H0), guarded(n, 1, n, off, a0.reshape(n, 1))
        gB, gX = guarded(m, nrhs, m + pad, off, Bs[0]), guarded(n, nrhs, n + pad, off)
        sB, sX = (m + pad) * (nrhs - 1) + m, (n + pad) * (nrhs - 1) + n  # (the last column may be short of the leading dimension)
        assert ldiv(h, P(gA.ptr), m, n, m + pad, (m + pad) * (n - 1) + m, P(gal.ptr), n, P(gB.ptr), nrhs, m + pad, sB,
                    P(gX.ptr), n + pad, sX, 1) == 0, emu.dhqr_last_error()
        assert same_bytes(gB.host(), Bs[0]) and same_bytes(gX.host(), want[:n])
        assert solve(h, P(gA.ptr), m, n, m + pad, (m + pad) * (n - 1) + m, P(gal.ptr), n, P(gB.ptr), nrhs, m + pad, sB, 1) == 0
        assert emu.dhqr_synchronize(h) == 0
        assert same_bytes(gB.host(), want)
        for g, what in ((gA, "A"), (gal, "alpha"), (gB, "B"), (gX, "X")):
            intact(g, f"{what} (pad {pad}, off {off})")
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
def test_argument_rules(emu, orc, t):
    """criterion 6: every DHQR_EINVAL case and every no-op on the device and the host form; nothing is touched"""
    m, n, nrhs, batch = 12, 6, 3, 3
    h = _ctx(emu)
    D, mats, Bs = _factored(emu, h, orc, m, n, nrhs, batch, t)
    before = [b.copy() for b in (D.A, D.al, D.B, D.X)]

    def both(**kw):
        dev = {k: v for k, v in kw.items() if k not in ("X", "ldx", "sX")}
        return D.solve_nrhs(emu, h, **dev), D.ldiv_nrhs(emu, h, **kw)

    for noop in (dict(nrhs=0), dict(batch=0), dict(n=0), dict(nrhs=0, B=None, X=None), dict(batch=0, A=None, al=None, B=None, X=None)):
        assert both(**noop) == (0, 0), noop
    bad = [dict(nrhs=-1), dict(batch=-1), dict(m=5, n=6), dict(lda=m - 1), dict(sA=D.lda * (n - 1) + m - 1), dict(sal=n - 1),
           dict(A=None), dict(al=None), dict(B=None), dict(ldb=m - 1), dict(sB=D.ldb * (nrhs - 1) + m - 1)]
    for kw in bad:
        assert both(**kw) == (N.EINVAL, N.EINVAL), kw
    for kw in (dict(X=None), dict(ldx=n - 1), dict(sX=D.ldx * (nrhs - 1) + n - 1)):
        assert D.ldiv_nrhs(emu, h, **kw) == N.EINVAL, kw
    for got, want in zip((D.A, D.al, D.B, D.X), before):
        assert same_bytes(got, want), "a rejected or empty call must not touch anything"
    # the smallest strides are accepted: the last column of B_k and X_k may be short of the leading dimension
    assert D.ldiv_nrhs(emu, h, sB=D.sB, sX=D.sX) == 0
    T = NBatch(mats, Bs, t, pad=0)
    for k in range(batch):
        T.mat(k)[...] = D.mat(k)
        T.alpha(k)[...] = D.alpha(k)
    sB, sX = T.ldb * (nrhs - 1) + m, T.ldx * (nrhs - 1) + n
    Bt, Xt = np.full(batch * sB, N.SENT, dtype=N.NP[t]), np.full(batch * sX, N.SENT, dtype=N.NP[t])
    for k in range(batch):
        for r in range(nrhs):
            Bt[k * sB + r * T.ldb: k * sB + r * T.ldb + m] = Bs[k][:, r]
    assert T.ldiv_nrhs(emu, h, B=ptr(Bt), sB=sB, X=ptr(Xt), sX=sX) == 0, emu.dhqr_last_error()
    for k in range(batch):
        for r in range(nrhs):
            assert same_bytes(Xt[k * sX + r * T.ldx: k * sX + r * T.ldx + n], D.xmat(k)[:, r])
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
def test_repeatability(emu, orc, t):
    """criterion 8: five calls on (40, 17), nrhs = 5 give identical bytes, the fifth on a fresh context"""
    m, n, nrhs, batch = 40, 17, 5, 5
    h = _ctx(emu)
    D, mats, Bs = _factored(emu, h, orc, m, n, nrhs, batch, t)
    B0 = D.B.copy()
    first = None
    for i in range(5):
        if i == 4:
            emu.dhqr_destroy(h)
            h = _ctx(emu)
        D.B[...] = B0
        assert D.solve_nrhs(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
        if first is None:
            first = D.B.copy()
        assert same_bytes(D.B, first), i
    emu.dhqr_destroy(h)


def test_python_front_end_type_errors(pkg):
    """criterion 6, the errors raised before any device is needed: a ComplexF64 factor takes a vector only; Float32 and
    Float64 do not mix"""
    rng = np.random.default_rng(0)
    Hc = pkg.DistributedHouseholderQRStruct(np.asfortranarray(rng.random((6, 3)) + 1j * rng.random((6, 3))))
    with pytest.raises(TypeError, match="ComplexF64: vector right-hand side only"):
        pkg.ldiv(Hc, np.zeros((6, 2), dtype=np.complex128))
    with pytest.raises(TypeError, match="ComplexF64: vector right-hand side only"):
        pkg.solve_householder_(np.zeros((6, 2), dtype=np.complex128), Hc.A, Hc.α)
    H32 = pkg.DistributedHouseholderQRStruct(np.asfortranarray(rng.random((6, 3)), dtype=np.float32))
    H64 = pkg.DistributedHouseholderQRStruct(np.asfortranarray(rng.random((6, 3))))
    with pytest.raises(TypeError, match="convert one of them explicitly"):
        pkg.ldiv(H32, np.zeros((6, 2)))
    with pytest.raises(TypeError, match="convert one of them explicitly"):
        pkg.ldiv(H64, np.zeros((6, 2), dtype=np.float32))
    Hb32 = pkg.DistributedHouseholderQRStruct(np.zeros((4, 6, 3), dtype=np.float32))
    with pytest.raises(TypeError, match="convert one of them explicitly"):
        pkg.ldiv(Hb32, np.zeros((4, 6, 2)))
