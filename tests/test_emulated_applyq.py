"""Q application, explicit Q and R for batches and Float32 (dhqr_apply_q_batched_* / dhqr_form_q_batched_* /
dhqr_form_r_batched_*) through the C ABI of the EMULATED library (csrc/ host-compiled against tests/simt/fake, fiber mode):
the tail of Q'B bit for bit against the multi-column solve, every column independent of nrhs, place and batch, both
directions against reflectors applied in np.longdouble, Q and R, padded / strided / offset layouts, the independence of the
matrices of a batch, the routes beyond the wave tier, the argument rules, the launch-group count; the Python front end's
argument errors that need no device."""
import ctypes
import os

import numpy as np
import pytest

import applyq_helpers as Q
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


def _ok(emu, h, rc):
    assert rc == 0, emu.dhqr_last_error()
    assert emu.dhqr_synchronize(h) == 0


def _with_factor(Hs, als, Bs, t, **layout):
    """an NBatch that holds the given factors, alphas and right-hand sides"""
    D = NBatch(Hs, Bs, t, **layout)
    for k in range(len(Hs)):
        D.alpha(k)[...] = als[k]
    return D


@pytest.fixture(scope="module")
def factors(emu, orc):
    """computed once per (shape, dtype, batch), shared and left unchanged: the inputs A_k, the factors (H_k, alpha_k) of
    dhqr_factor_batched_* and N.NRHS_MAX columns of B_k"""
    cache = {}

    def get(m, n, t, batch=5, seed=N.SEED):
        key = (m, n, t, batch, seed)
        if key not in cache:
            h = _ctx(emu)
            mats, Bs = N.inputs(orc, m, n, N.NRHS_MAX, batch, seed, t)
            D = NBatch(mats, Bs, t)
            _ok(emu, h, D.factor(emu, h))
            Hs, als = [np.array(D.mat(k), order="F") for k in range(batch)], [D.alpha(k).copy() for k in range(batch)]
            for a in mats + Bs + Hs + als:
                a.setflags(write=False)
            emu.dhqr_destroy(h)
            cache[key] = (mats, Hs, als, Bs)
        return cache[key]
    return get


def _applied(emu, h, Hs, als, Bs, t, trans, **layout):
    D = _with_factor(Hs, als, Bs, t, **layout)
    _ok(emu, h, Q.apply_q(emu, h, D, trans))
    assert D.padding_intact() and D.x_untouched()
    return D


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n", N.WAVE_SHAPES)
def test_trans1_has_the_bits_of_the_solve(emu, factors, m, n, t):
    """criterion 1: trans = 1 with nrhs = 1, 3, 4, 5, 9, 8, 13 at batch 5 (and batch 1 for N.NRHS) -- rows n .. m-1 of every
    column have the bytes of the same rows after dhqr_solve_batched_nrhs_* on a copy; the whole column has the bytes of the
    nrhs = 1 call on that column, whatever nrhs, its place in its group and the batch"""
    mats, Hs, als, Bs = factors(m, n, t)
    h = _ctx(emu)
    alone = [_applied(emu, h, Hs, als, [B[:, r:r + 1] for B in Bs], t, 1) for r in range(N.NRHS_MAX)]
    for nrhs in N.NRHS_ALL:
        for batch in ((5, 1) if nrhs in N.NRHS else (5,)):
            cut = [B[:, :nrhs] for B in Bs[:batch]]
            D = _applied(emu, h, Hs[:batch], als[:batch], cut, t, 1)
            S = _with_factor(Hs[:batch], als[:batch], cut, t)
            _ok(emu, h, S.solve_nrhs(emu, h))
            for k in range(batch):
                assert same_bytes(D.bmat(k)[n:], S.bmat(k)[n:]), f"nrhs {nrhs} batch {batch}: tail of matrix {k}"
                for r in range(nrhs):
                    assert same_bytes(D.bmat(k)[:, r], alone[r].bmat(k)[:, 0]), f"nrhs {nrhs} batch {batch}: matrix {k} column {r}"
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n", N.WAVE_SHAPES)
def test_trans0_columns_do_not_depend_on_nrhs_place_or_batch(emu, factors, m, n, t):
    """criterion 1's independence for trans = 0: the bytes of the nrhs = 1 call on the column"""
    mats, Hs, als, Bs = factors(m, n, t)
    h = _ctx(emu)
    alone = [_applied(emu, h, Hs, als, [B[:, r:r + 1] for B in Bs], t, 0) for r in range(N.NRHS_MAX)]
    for nrhs, batch in ((3, 1), (4, 5), (9, 5), (13, 5)):  # a tail of three, full groups of four / three, tails of one
        D = _applied(emu, h, Hs[:batch], als[:batch], [B[:, :nrhs] for B in Bs[:batch]], t, 0)
        for k in range(batch):
            for r in range(nrhs):
                assert same_bytes(D.bmat(k)[:, r], alone[r].bmat(k)[:, 0]), f"nrhs {nrhs} batch {batch}: matrix {k} column {r}"
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n", N.WAVE_SHAPES)
def test_accuracy_against_longdouble_reflectors(emu, factors, m, n, t):
    """criterion 2, independent of criterion 1: both directions against the reflectors of the kernel's own factor applied in
    np.longdouble, |d| <= 1e-12 max|result| (Float64) / 4 EPS32 max|result| (Float32); and Q'(QB) returns B within the same
    bound (criterion 3)"""
    mats, Hs, als, Bs = factors(m, n, t)
    nrhs = 9
    cut = [B[:, :nrhs] for B in Bs]
    h = _ctx(emu)
    for trans in (1, 0):
        D = _applied(emu, h, Hs, als, cut, t, trans)
        for k in range(5):
            want = Q.reflect_longdouble(Hs[k], cut[k], trans)
            err, scale = float(np.abs(D.bmat(k) - want).max()), float(np.abs(want).max())
            print(f"{m}x{n} {t} trans {trans} matrix {k}: |d| / max|result| = {err / scale:.2e} (tol {Q.tol(t):.2e})")
            assert err <= Q.tol(t) * scale
    _ok(emu, h, Q.apply_q(emu, h, D, 1))  # D holds Q B
    for k in range(5):
        err, scale = float(np.abs(D.bmat(k).astype(np.float64) - cut[k]).max()), float(np.abs(cut[k]).max())
        print(f"{m}x{n} {t} Q'(QB) matrix {k}: |d| / max|B| = {err / scale:.2e}")
        assert err <= Q.tol(t) * scale
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n", N.WAVE_SHAPES)
def test_explicit_q_and_r(emu, factors, m, n, t):
    """criterion 3: R upper triangular with the bytes of alpha and of H; Q'Q = I and QR = A within the bounds of
    Q.check_qr; form_q compares equal to trans = 0 on [I; 0]; the sentinel-filled Q and R buffers are fully overwritten
    inside and untouched outside"""
    mats, Hs, als, Bs = factors(m, n, t)
    h = _ctx(emu)
    D = _with_factor(Hs, als, [Q.eye_columns(m, n, t)] * 5, t)
    Qb, Rb = Q.OutBatch(5, m, n, t), Q.OutBatch(5, n, n, t)
    _ok(emu, h, Q.form_q(emu, h, D, Qb))
    _ok(emu, h, Q.form_r(emu, h, D, Rb))
    _ok(emu, h, Q.apply_q(emu, h, D, 0))
    assert Qb.padding_intact() and Rb.padding_intact() and D.padding_intact()
    for k in range(5):
        assert not (Qb.mat(k) == N.SENT).any() and not (Rb.mat(k) == N.SENT).any()
        assert np.array_equal(Qb.mat(k), D.bmat(k)), f"form_q != Q [I; 0] for matrix {k}"
        Q.check_r(Rb.mat(k), Hs[k], als[k])
        Q.check_qr(Qb.mat(k), Rb.mat(k), mats[k], t, f"{m}x{n} {t} matrix {k}")
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
def test_layouts(emu, factors, t):
    """criterion 4: the packed layout's bytes on padded lda / ldb / ldq / ldr, strides with gaps and a base one element off a
    256-byte boundary; every element outside the matrices keeps the sentinel"""
    m, n, nrhs = 33, 9, 5
    mats, Hs, als, Bs = factors(m, n, t)
    cut = [B[:, :nrhs] for B in Bs]
    h = _ctx(emu)
    packed = dict(pad_ld=0, pad=0, pad_ldb=0)
    want = {tr: _applied(emu, h, Hs, als, cut, t, tr, **packed) for tr in (0, 1)}
    Qw, Rw = Q.OutBatch(5, m, n, t, 0, 0), Q.OutBatch(5, n, n, t, 0, 0)
    _ok(emu, h, Q.form_q(emu, h, want[0], Qw))
    _ok(emu, h, Q.form_r(emu, h, want[0], Rw))
    for lay, out in ((dict(pad_ld=1, pad=0, pad_ldb=3), (3, 0, 0)), (dict(pad_ld=3, pad=5, pad_ldb=1, off=1), (1, 7, 1)),
                     (dict(pad_ld=0, pad=2, pad_ldb=0, off=1), (0, 1, 1))):
        for tr in (0, 1):
            D = _applied(emu, h, Hs, als, cut, t, tr, **lay)
            for k in range(5):
                assert same_bytes(D.bmat(k), want[tr].bmat(k)), (lay, tr, k)
        Qb, Rb = Q.OutBatch(5, m, n, t, *out), Q.OutBatch(5, n, n, t, *out)
        _ok(emu, h, Q.form_q(emu, h, D, Qb))
        _ok(emu, h, Q.form_r(emu, h, D, Rb))
        for k in range(5):
            assert same_bytes(Qb.mat(k), Qw.mat(k)) and same_bytes(Rb.mat(k), Rw.mat(k)), (lay, k)
        assert Qb.padding_intact() and Rb.padding_intact() and D.padding_intact()
    emu.dhqr_destroy(h)


def _all_results(emu, h, Hs, als, Bs, t):
    """(Q'B, QB, Q, R) of a batch, each a list of matrices"""
    m, n = Hs[0].shape
    batch = len(Hs)
    out = []
    for tr in (1, 0):
        D = _applied(emu, h, Hs, als, Bs, t, tr)
        out.append([np.array(D.bmat(k)) for k in range(batch)])
    Qb, Rb = Q.OutBatch(batch, m, n, t), Q.OutBatch(batch, n, n, t)
    _ok(emu, h, Q.form_q(emu, h, D, Qb))
    _ok(emu, h, Q.form_r(emu, h, D, Rb))
    assert Qb.padding_intact() and Rb.padding_intact()
    return out + [[np.array(Qb.mat(k)) for k in range(batch)], [np.array(Rb.mat(k)) for k in range(batch)]]


@pytest.mark.parametrize("t", N.DTYPES)
def test_a_nan_reflector_stays_in_its_matrix(emu, orc, t):
    """criterion 5: matrix 2 of a batch of 5 has a zero column -- its reflector is NaN (dhqr_batched.h: 0 * NaN) --; matrices
    0, 1, 3 and 4 have the bytes of the clean run, in Q'B, QB, Q and R"""
    m, n, nrhs = 16, 8, 5
    mats, Bs = N.inputs(orc, m, n, nrhs, 5, N.SEED, t)
    h = _ctx(emu)
    runs = []
    for dirty in (False, True):
        ms = [a.copy() for a in mats]
        if dirty:
            ms[2][:, 3] = 0
        D = NBatch(ms, Bs, t)
        _ok(emu, h, D.factor(emu, h))
        Hs, als = [np.array(D.mat(k), order="F") for k in range(5)], [D.alpha(k).copy() for k in range(5)]
        if dirty:
            assert np.isnan(Hs[2]).any(), "the zero column was meant to give a NaN reflector"
        runs.append(_all_results(emu, h, Hs, als, Bs, t))
    for clean, dirty in zip(*runs):
        for k in (0, 1, 3, 4):
            assert same_bytes(clean[k], dirty[k]), k
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
def test_batch_300(emu, factors, t):
    """criterion 5: 75 workgroups at (5, 3) -- every matrix has the bytes of its single-matrix call, in Q'B, QB, Q and R"""
    m, n, nrhs, batch = 5, 3, 4, 300
    mats, Hs, als, Bs = factors(m, n, t, batch)
    cut = [B[:, :nrhs] for B in Bs]
    h = _ctx(emu)
    whole = _all_results(emu, h, Hs, als, cut, t)
    for k in range(batch):
        one = _all_results(emu, h, Hs[k:k + 1], als[k:k + 1], cut[k:k + 1], t)
        for w, o in zip(whole, one):
            assert same_bytes(w[k], o[0]), k
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
@pytest.mark.parametrize("m,n,batch", N.BEYOND)
def test_beyond_the_wave_tier(emu, factors, m, n, batch, t):
    """criterion 6.  Float64: matrix k has the bytes of dhqr_apply_q_f64 on it alone, in both directions, and form_q those of
    that call on [I; 0].  Float32: the rounded result of the Float64 entry point on the widened inputs (packed, as the
    promoted tier holds them), bit for bit.  form_r as on the wave tier."""
    nrhs = 3
    mats, Hs, als, Bs = factors(m, n, t, batch)
    cut = [B[:, :nrhs] for B in Bs]
    h = _ctx(emu)
    wide = lambda xs: [np.asarray(x, dtype=np.float64) for x in xs]
    packed = dict(pad_ld=0, pad=0, pad_ldb=0)
    for tr in (1, 0):
        D = _applied(emu, h, Hs, als, cut, t, tr)
        if t == "f64":
            S = _with_factor(Hs, als, cut, t)
            for k in range(batch):
                assert emu.dhqr_apply_q_f64(h, ptr(S.mat(k)), m, n, S.lda, ptr(S.bmat(k)), nrhs, S.ldb, tr) == 0, emu.dhqr_last_error()
            assert emu.dhqr_synchronize(h) == 0 and S.padding_intact()
            want = [S.bmat(k) for k in range(batch)]
        else:
            S = _applied(emu, h, wide(Hs), wide(als), wide(cut), "f64", tr, **packed)
            want = [S.bmat(k).astype(np.float32) for k in range(batch)]
        for k in range(batch):
            assert same_bytes(D.bmat(k), want[k]), (tr, k)
    Qb, Rb = Q.OutBatch(batch, m, n, t), Q.OutBatch(batch, n, n, t)
    _ok(emu, h, Q.form_q(emu, h, D, Qb))
    _ok(emu, h, Q.form_r(emu, h, D, Rb))
    eye = [Q.eye_columns(m, n, "f64")] * batch
    if t == "f64":
        S = _with_factor(Hs, als, eye, t, pad_ldb=2, pad=3)  # (the layout of Qb: the blocked route vectorises by alignment)
        for k in range(batch):
            assert emu.dhqr_apply_q_f64(h, ptr(S.mat(k)), m, n, S.lda, ptr(S.bmat(k)), n, S.ldb, 0) == 0, emu.dhqr_last_error()
        assert emu.dhqr_synchronize(h) == 0
        want = [S.bmat(k) for k in range(batch)]
    else:
        S = _with_factor(wide(Hs), wide(als), eye, "f64", **packed)
        Q64 = Q.OutBatch(batch, m, n, "f64", 0, 0)
        _ok(emu, h, Q.form_q(emu, h, S, Q64))
        want = [Q64.mat(k).astype(np.float32) for k in range(batch)]
    assert Qb.padding_intact() and Rb.padding_intact()
    for k in range(batch):
        assert same_bytes(Qb.mat(k), want[k]), k
        Q.check_r(Rb.mat(k), Hs[k], als[k])
        Q.check_qr(Qb.mat(k), Rb.mat(k), mats[k], t, f"{m}x{n} {t} matrix {k}")
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
def test_argument_rules(emu, factors, t):
    """criterion 7: every DHQR_EINVAL case writes nothing; the no-ops look at no pointer (null is passed); the smallest
    strides are accepted"""
    m, n, nrhs, batch = 16, 8, 3, 3
    mats, Hs, als, Bs = factors(m, n, t)
    h = _ctx(emu)
    D = _with_factor(Hs[:batch], als[:batch], [B[:, :nrhs] for B in Bs[:batch]], t)
    Qb, Rb = Q.OutBatch(batch, m, n, t), Q.OutBatch(batch, n, n, t)
    before = [b.copy() for b in (D.A, D.al, D.B)]
    null = dict(A=None, B=None)
    for noop in (dict(nrhs=0, **null), dict(batch=0, **null), dict(n=0, **null)):
        for tr in (0, 1):
            assert Q.apply_q(emu, h, D, tr, **noop) == 0, noop
    for noop in (dict(batch=0), dict(n=0)):
        assert Q.form_q(emu, h, D, Qb, A=None, Q=None, **noop) == 0, noop
        assert Q.form_r(emu, h, D, Rb, A=None, al=None, R=None, **noop) == 0, noop
    matrix = [dict(batch=-1), dict(m=7, n=8), dict(lda=m - 1), dict(sA=D.lda * (n - 1) + m - 1), dict(A=None)]
    for kw in matrix + [dict(nrhs=-1), dict(B=None), dict(ldb=m - 1), dict(sB=D.ldb * (nrhs - 1) + m - 1), dict(trans=2), dict(trans=-1)]:
        assert Q.apply_q(emu, h, D, kw.pop("trans", 1), **kw) == N.EINVAL, kw
    for kw in matrix + [dict(Q=None), dict(ldq=m - 1), dict(sQ=Qb.ld * (n - 1) + m - 1)]:
        assert Q.form_q(emu, h, D, Qb, **kw) == N.EINVAL, kw
    for kw in matrix + [dict(al=None), dict(sal=n - 1), dict(R=None), dict(ldr=n - 1), dict(sR=Rb.ld * (n - 1) + n - 1)]:
        assert Q.form_r(emu, h, D, Rb, **kw) == N.EINVAL, kw
    assert emu.dhqr_synchronize(h) == 0
    for got, want in zip((D.A, D.al, D.B), before):
        assert same_bytes(got, want), "a rejected or empty call must not touch anything"
    assert Qb.untouched() and Rb.untouched()
    # the last column of a matrix may be short of its leading dimension: a batch of one with the smallest strides
    one = _with_factor(Hs[:1], als[:1], [Bs[0][:, :nrhs]], t)
    want = _applied(emu, h, Hs[:1], als[:1], [Bs[0][:, :nrhs]], t, 1)
    _ok(emu, h, Q.apply_q(emu, h, one, 1, sA=one.lda * (n - 1) + m, sB=one.ldb * (nrhs - 1) + m))
    assert same_bytes(one.bmat(0), want.bmat(0))
    Q1, R1 = Q.OutBatch(1, m, n, t), Q.OutBatch(1, n, n, t)
    _ok(emu, h, Q.form_q(emu, h, one, Q1, sQ=Q1.ld * (n - 1) + m))
    _ok(emu, h, Q.form_r(emu, h, one, R1, sR=R1.ld * (n - 1) + n, sal=n))
    assert Q1.padding_intact() and R1.padding_intact()
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("t", N.DTYPES)
def test_launch_groups(emu, factors, t):
    """criterion 7: with profiling on, a wave-tier call adds exactly ONE n_solve, whatever nrhs and batch"""
    m, n = 16, 8
    mats, Hs, als, Bs = factors(m, n, t)
    h = _ctx(emu)
    D = _with_factor(Hs, als, [B[:, :9] for B in Bs], t)
    Qb = Q.OutBatch(5, m, n, t)
    assert emu.dhqr_set_profiling(h, 1) == 0
    for call in (lambda: Q.apply_q(emu, h, D, 1), lambda: Q.apply_q(emu, h, D, 0), lambda: Q.form_q(emu, h, D, Qb)):
        assert emu.dhqr_reset_stats(h) == 0
        _ok(emu, h, call())
        assert _n_solve(emu, h) == 1
    emu.dhqr_destroy(h)


def test_python_front_end_errors(pkg):
    """criterion 7, the errors raised before any device is needed: a numpy factor (device tensors only), Float32 and
    Float64 do not mix, matrices that are not column-major"""
    import torch
    rng = np.random.default_rng(0)
    Hn = pkg.DistributedHouseholderQRStruct(np.asfortranarray(rng.random((6, 3))))
    for call in (lambda: pkg.apply_q_(Hn, np.zeros((6, 2)), True), lambda: pkg.get_q(Hn), lambda: pkg.get_r(Hn)):
        with pytest.raises(TypeError, match="device tensors only"):
            call()
    H32 = pkg.DistributedHouseholderQRStruct(torch.zeros((4, 3, 6), dtype=torch.float32).transpose(1, 2))
    H64 = pkg.DistributedHouseholderQRStruct(torch.zeros((4, 3, 6), dtype=torch.float64).transpose(1, 2))
    with pytest.raises(TypeError, match="convert one of them explicitly"):
        pkg.apply_q_(H32, torch.zeros((4, 2, 6), dtype=torch.float64).transpose(1, 2), True)
    with pytest.raises(TypeError, match="convert one of them explicitly"):
        pkg.apply_q_(H64, torch.zeros((4, 2, 6), dtype=torch.float32).transpose(1, 2), False)
    Hrow = pkg.DistributedHouseholderQRStruct(torch.zeros((4, 6, 3), dtype=torch.float32))  # row-major matrices
    for call in (lambda: pkg.get_q(Hrow), lambda: pkg.apply_q_(Hrow, torch.zeros((4, 2, 6), dtype=torch.float32).transpose(1, 2), True)):
        with pytest.raises(ValueError, match="column-major"):
            call()
    with pytest.raises(ValueError, match="column-major"):
        pkg.apply_q_(H32, torch.zeros((4, 6, 2), dtype=torch.float32), True)  # B row-major
    with pytest.raises(TypeError, match="shape"):
        pkg.apply_q_(H32, torch.zeros((4, 2, 5), dtype=torch.float32).transpose(1, 2), True)  # 5 rows against 6
