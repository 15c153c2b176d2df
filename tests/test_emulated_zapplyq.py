"""`H \\ B` with several right-hand sides, Q application, explicit Q and R for batches of small ComplexF64 factors
(dhqr_solve_batched_nrhs_c64 / dhqr_ldiv_batched_nrhs_c64 / dhqr_apply_q_batched_c64 / dhqr_form_q_batched_c64 /
dhqr_form_r_batched_c64) through the C ABI of the EMULATED library (csrc/ host-compiled against tests/simt/fake, fiber mode):
every column of the solve bit for bit against the single-column entry point, the tail of Q^H B against the solve, form_q
against Q [I; 0], both directions against reflectors applied in np.clongdouble, A = QR and Q^H Q = I, special inputs, a
poisoned neighbour, the general tier, guarded layouts, the argument rules, the host form; the Python front end's errors
that need no device."""
import ctypes
import os

import numpy as np
import pytest

import zapplyq_helpers as Z
import zbatched_helpers as zh
from zapplyq_helpers import EINVAL, P, ZNBatch, ZOut, same_bytes
from zbatched_helpers import SENT, cptr

NRHS_MAX = 9


@pytest.fixture(scope="module")
def emu(emulated_so):
    from dist_helpers import load_emulated_library
    L = load_emulated_library(emulated_so)
    for name in ("dhqr_solve_batched_nrhs_c64", "dhqr_ldiv_batched_nrhs_c64", "dhqr_apply_q_batched_c64", "dhqr_form_q_batched_c64",
                 "dhqr_form_r_batched_c64"):
        assert hasattr(L, name), f"the library does not export {name}"
    return L


def _ctx(L, small=1, tune=None):
    """a context with the small route on (or off); tune: DHQR_TUNE while it is created"""
    env = {"DHQR_SMALL": str(small), "DHQR_TUNE": tune}
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


def _ok(emu, h, rc):
    assert rc == 0, emu.dhqr_last_error()
    assert emu.dhqr_synchronize(h) == 0


@pytest.fixture(scope="module")
def factors(emu, orc):
    """computed once per (shape, batch, seed, small route), shared and left unchanged: the inputs A_k, the factors (H_k, alpha_k)
    of dhqr_factor_batched_c64 and NRHS_MAX columns of B_k"""
    cache = {}

    def get(m, n, batch=5, seed=Z.SEED, small=1, mats=None):
        key = (m, n, batch, seed, small) if mats is None else None
        if key is None or key not in cache:
            h = _ctx(emu, small)
            ms, Bs = Z.inputs(orc, m, n, NRHS_MAX, batch, seed)
            if mats is not None:
                ms = mats
            D = ZNBatch(ms, Bs)
            _ok(emu, h, D.factor(emu, h))
            Hs, als = [np.array(D.mat(k), order="F") for k in range(batch)], [D.alpha(k).copy() for k in range(batch)]
            for a in list(ms) + Bs + Hs + als:
                a.setflags(write=False)
            emu.dhqr_destroy(h)
            if key is None:
                return ms, Hs, als, Bs
            cache[key] = (ms, Hs, als, Bs)
        return cache[key]
    return get


def _cut(Bs, nrhs, batch=None):
    return [np.asfortranarray(B[:, :nrhs]) for B in (Bs if batch is None else Bs[:batch])]


def _applied(emu, h, Hs, als, Bs, trans, **layout):
    D = ZNBatch(Hs, Bs, als, **layout)
    _ok(emu, h, D.apply_q(emu, h, trans))
    assert D.padding_intact() and D.x_untouched()
    return D


def _solved(emu, h, Hs, als, Bs, **layout):
    D = ZNBatch(Hs, Bs, als, **layout)
    _ok(emu, h, D.solve_nrhs(emu, h))
    assert D.padding_intact() and D.x_untouched()
    return D


@pytest.mark.parametrize("m,n", Z.WAVE_SHAPES)
def test_solve_columns_have_the_bits_of_the_single_column_solve(emu, factors, m, n):
    """item 1: column r of dhqr_solve_batched_nrhs_c64 is byte-identical to dhqr_solve_batched_c64 on that column alone -- on the
    multi-column kernel (a context that always takes it) for nrhs = 1, RG, RG + 1, 7 and 2 RG + 1 and batches of 1, 3, 4 and
    5, and on the default context, whose rule sends nrhs = 4 to the kernel and, beyond n = 8, nrhs = 7 to the column loop"""
    mats, Hs, als, Bs = factors(m, n)
    h, hk = _ctx(emu), _ctx(emu, tune=Z.TUNE_KERNEL)
    F = ZNBatch(Hs, _cut(Bs, 1), als)
    alone = [F.single_column(emu, h, r, Bs) for r in range(NRHS_MAX)]  # (5, m) per column
    st = emu.Stats()
    tail = Z.rg_solve(n) + 1  # (batches of 3 and 4 at one nrhs: the emulator is slow)
    for ctx, cases in ((hk, [(nrhs, batch) for nrhs in Z.nrhs_list(n, Z.rg_solve) for batch in (5, 1, 3, 4) if batch in (5, 1) or nrhs == tail]),
                       (h, [(nrhs, 5) for nrhs in Z.RULE_NRHS])):
        assert emu.dhqr_set_profiling(ctx, 1) == 0
        for nrhs, batch in cases:
            assert emu.dhqr_reset_stats(ctx) == 0
            D = _solved(emu, ctx, Hs[:batch], als[:batch], _cut(Bs, nrhs, batch))
            assert emu.dhqr_get_stats(ctx, ctypes.byref(st)) == 0
            kernel = ctx is hk or Z.rule_takes_kernel(n, nrhs)
            assert st.n_solve == (1 if kernel else nrhs), f"nrhs {nrhs}: {st.n_solve} launch groups"
            for k in range(batch):
                for r in range(nrhs):
                    assert same_bytes(D.bmat(k)[:, r], alone[r][k]), f"nrhs {nrhs} batch {batch}: matrix {k} column {r}"
        emu.dhqr_destroy(ctx)


@pytest.mark.parametrize("m,n", Z.WAVE_SHAPES)
def test_trans1_tail_has_the_bits_of_the_solve_and_columns_are_independent(emu, factors, m, n):
    """item 1: rows n .. m-1 of apply_q(trans = 1) are byte-identical to the solve's; every column of both directions has the
    bytes of the nrhs = 1 call on it, whatever nrhs, its place in its group and the batch"""
    mats, Hs, als, Bs = factors(m, n)
    h = _ctx(emu, tune=Z.TUNE_KERNEL)  # (the solve on its multi-column kernel)
    alone = {tr: [_applied(emu, h, Hs, als, [np.asfortranarray(B[:, r:r + 1]) for B in Bs], tr) for r in range(NRHS_MAX)] for tr in (0, 1)}
    for nrhs in Z.nrhs_list(n, Z.rg_apply):
        for batch in ((5, 1, 3, 4) if nrhs == Z.rg_apply(n) + 1 else (5, 1)):  # (batches of 3 and 4 at one nrhs: the emulator is slow)
            cut = _cut(Bs, nrhs, batch)
            S = _solved(emu, h, Hs[:batch], als[:batch], cut)
            for tr in (1, 0):
                D = _applied(emu, h, Hs[:batch], als[:batch], cut, tr)
                for k in range(batch):
                    if tr == 1:
                        assert same_bytes(D.bmat(k)[n:], S.bmat(k)[n:]), f"nrhs {nrhs} batch {batch}: tail of matrix {k}"
                    for r in range(nrhs):
                        assert same_bytes(D.bmat(k)[:, r], alone[tr][r].bmat(k)[:, 0]), f"trans {tr} nrhs {nrhs} batch {batch}: matrix {k} column {r}"
    emu.dhqr_destroy(h)


def _q_and_r(emu, h, Hs, als, **layout):
    """(ZOut Q, ZOut R, Q [I; 0] from apply_q) of a batch"""
    m, n = Hs[0].shape
    batch = len(Hs)
    D = ZNBatch(Hs, [Z.eye_columns(m, n)] * batch, als, **layout)
    Qb, Rb = ZOut(batch, m, n), ZOut(batch, n, n)
    _ok(emu, h, D.form_q(emu, h, Qb))
    _ok(emu, h, D.form_r(emu, h, Rb))
    _ok(emu, h, D.apply_q(emu, h, 0))
    assert Qb.padding_intact() and Rb.padding_intact() and D.padding_intact()
    for k in range(batch):
        assert not (Qb.mat(k) == SENT).any() and not (Rb.mat(k) == SENT).any()
    return Qb, Rb, D


@pytest.mark.parametrize("m,n", Z.WAVE_SHAPES)
def test_accuracy_and_explicit_q_and_r(emu, orc, factors, m, n):
    """item 2: both directions against the clongdouble reflectors of the device's own factor, Q (Q^H B) = B, x against
    orc.solve_c, form_q equal to apply_q(trans = 0) on [I; 0], R strictly upper + alpha with exact zeros below, A = QR and
    Q^H Q = I"""
    mats, Hs, als, Bs = factors(m, n)
    nrhs = 7
    cut = _cut(Bs, nrhs)
    h = _ctx(emu)
    for tr in (1, 0):
        D = _applied(emu, h, Hs, als, cut, tr)
        for k in range(5):
            Z.check_close(D.bmat(k), Z.reflect_clongdouble(Hs[k], cut[k], tr), f"{m}x{n} trans {tr} matrix {k}")
    D = _applied(emu, h, Hs, als, cut, 1)
    _ok(emu, h, D.apply_q(emu, h, 0))  # Q (Q^H B)
    S = _solved(emu, h, Hs, als, cut)
    for k in range(5):
        Z.check_close(D.bmat(k), cut[k], f"{m}x{n} Q (Q^H B) matrix {k}")
        Z.check_x(orc, mats[k], cut[k], S.bmat(k)[:n], f"{m}x{n} matrix {k}")
    Qb, Rb, E = _q_and_r(emu, h, Hs, als)
    for k in range(5):
        assert np.array_equal(Qb.mat(k), E.bmat(k)), f"form_q != Q [I; 0] for matrix {k}"
        Z.check_close(Qb.mat(k), Z.reflect_clongdouble(Hs[k], Z.eye_columns(m, n), 0), f"{m}x{n} Q matrix {k}")
        Z.check_r(Rb.mat(k), Hs[k], als[k])
        Z.check_qr(Qb.mat(k), Rb.mat(k), mats[k], f"{m}x{n} matrix {k}")
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", [(16, 8), (64, 32)])
def test_special_matrices(emu, orc, factors, m, n):
    """item 3: an imaginary part identically zero, a real part identically zero, a pivot of exactly zero (alone and with a zero
    imaginary part): a wrong conjugate or sign shows here"""
    mats = zh.special_matrices(orc, m, n)
    mats, Hs, als, Bs = factors(m, n, batch=7, seed=900, mats=mats)
    cut = _cut(Bs, 5)
    h = _ctx(emu)
    for tr in (1, 0):
        D = _applied(emu, h, Hs, als, cut, tr)
        for k in range(7):
            Z.check_close(D.bmat(k), Z.reflect_clongdouble(Hs[k], cut[k], tr), f"special {m}x{n} trans {tr} matrix {k}")
    S = _solved(emu, h, Hs, als, cut)
    Qb, Rb, E = _q_and_r(emu, h, Hs, als)
    for k in range(7):
        Z.check_x(orc, mats[k], cut[k], S.bmat(k)[:n], f"special {m}x{n} matrix {k}")
        assert np.array_equal(Qb.mat(k), E.bmat(k))
        Z.check_r(Rb.mat(k), Hs[k], als[k])
        Z.check_qr(Qb.mat(k), Rb.mat(k), mats[k], f"special {m}x{n} matrix {k}")
    for k in (1, 5):  # a real factor gives a real Q and R
        assert (Qb.mat(k).imag == 0).all() and (Rb.mat(k).imag == 0).all()
    emu.dhqr_destroy(h)


def _all_results(emu, h, Hs, als, Bs, **layout):
    """(X and tail, Q^H B, Q B, Q, R) of a batch, each a list of matrices"""
    m, n = Hs[0].shape
    batch = len(Hs)
    out = [[np.array(_solved(emu, h, Hs, als, Bs, **layout).bmat(k)) for k in range(batch)]]
    for tr in (1, 0):
        D = _applied(emu, h, Hs, als, Bs, tr, **layout)
        out.append([np.array(D.bmat(k)) for k in range(batch)])
    Qb, Rb = ZOut(batch, m, n), ZOut(batch, n, n)
    _ok(emu, h, D.form_q(emu, h, Qb))
    _ok(emu, h, D.form_r(emu, h, Rb))
    assert Qb.padding_intact() and Rb.padding_intact()
    return out + [[np.array(Qb.mat(k)) for k in range(batch)], [np.array(Rb.mat(k)) for k in range(batch)]]


def test_a_zero_column_stays_in_its_matrix(emu, orc, factors):
    """item 4: matrix 2 of five has a zero column (zh.poison_column): the other four keep their bits in all four operations"""
    m, n, nrhs = 16, 8, 5
    clean = factors(m, n, seed=700)
    bad = [zh.poison_column(A) if k == 2 else A for k, A in enumerate(clean[0])]
    dirty = factors(m, n, seed=700, mats=bad)
    assert not np.isfinite(dirty[1][2]).all(), "the zero column was meant to give a non-finite factor"
    h = _ctx(emu)
    runs = [_all_results(emu, h, Hs, als, _cut(Bs, nrhs)) for _, Hs, als, Bs in (clean, dirty)]
    for c, d in zip(*runs):
        for k in (0, 1, 3, 4):
            assert same_bytes(c[k], d[k]), k
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n,small", Z.BEYOND)
def test_the_general_tier(emu, orc, factors, m, n, small):
    """item 5: beyond 64 x 32, and (16, 8) with the small route off: the accuracy of item 2, the solve byte-identical to the
    column loop, every result repeatable byte for byte over three calls"""
    batch, nrhs = 2, 3
    mats, Hs, als, Bs = factors(m, n, batch=batch, seed=200, small=small)
    cut = _cut(Bs, nrhs)
    h = _ctx(emu, small)
    runs = [_all_results(emu, h, Hs, als, cut) for _ in range(3)]
    for again in runs[1:]:
        for a, b in zip(runs[0], again):
            for k in range(batch):
                assert same_bytes(a[k], b[k]), "the general tier must be repeatable bit for bit"
    X, QhB, QB, Qs, Rs = runs[0]
    F = ZNBatch(Hs, _cut(Bs, 1), als)
    for r in range(nrhs):
        col = F.single_column(emu, h, r, Bs)
        for k in range(batch):
            assert same_bytes(X[k][:, r], col[k]), f"solve column {r} of matrix {k} != the column loop"
    D = ZNBatch(Hs, QhB, als)
    _ok(emu, h, D.apply_q(emu, h, 0))
    for k in range(batch):
        Z.check_close(QhB[k], Z.reflect_clongdouble(Hs[k], cut[k], 1), f"{m}x{n} general Q^H B matrix {k}")
        Z.check_close(QB[k], Z.reflect_clongdouble(Hs[k], cut[k], 0), f"{m}x{n} general Q B matrix {k}")
        Z.check_close(D.bmat(k), cut[k], f"{m}x{n} general Q (Q^H B) matrix {k}")
        Z.check_x(orc, mats[k], cut[k], X[k][:n], f"{m}x{n} general matrix {k}")
        Z.check_close(Qs[k], Z.reflect_clongdouble(Hs[k], Z.eye_columns(m, n), 0), f"{m}x{n} general Q matrix {k}")
        Z.check_r(Rs[k], Hs[k], als[k])
        Z.check_qr(Qs[k], Rs[k], mats[k], f"{m}x{n} general matrix {k}")
    emu.dhqr_destroy(h)


def test_guarded_layout_gives_the_packed_bits(emu, factors):
    """item 6: (40, 17), nrhs 5: lda = m + 1, padded strides, base one element in -- the packed call's bits, every sentinel
    intact, for all five entry points"""
    m, n, nrhs = 40, 17, 5
    mats, Hs, als, Bs = factors(m, n)
    cut = _cut(Bs, nrhs)
    h = _ctx(emu)
    packed = dict(pad_ld=0, pad=0, pad_ldb=0, pad_ldx=0, off=0)
    G = ZNBatch(Hs, cut, als)
    assert (G.lda, G.sal, G.off, G.ldb) == (m + 1, n + 3, 1, m + 1)
    want = _all_results(emu, h, Hs, als, cut, **packed)
    got = _all_results(emu, h, Hs, als, cut)  # (guarded; ZOut is guarded in both)
    for w, g in zip(want, got):
        for k in range(5):
            assert same_bytes(w[k], g[k]), k
    _ok(emu, h, G.ldiv_nrhs(emu, h))
    assert G.padding_intact()
    for k in range(5):
        assert same_bytes(G.xmat(k), want[0][k][:n]) and same_bytes(G.bmat(k), cut[k])
    emu.dhqr_destroy(h)


def test_argument_rules_and_empty_cases(emu, factors):
    """item 7: every DHQR_EINVAL case writes nothing; the no-ops look at no pointer (null is passed)"""
    m, n, nrhs, batch = 16, 8, 3, 3
    mats, Hs, als, Bs = factors(m, n)
    h = _ctx(emu)
    D = ZNBatch(Hs[:batch], _cut(Bs, nrhs, batch), als[:batch])
    Qb, Rb = ZOut(batch, m, n), ZOut(batch, n, n)
    before = [b.copy() for b in (D.A, D.al, D.B, D.X)]
    null = dict(A=None, al=None, B=None)
    for noop in (dict(nrhs=0, **null), dict(batch=0, **null), dict(n=0, **null)):
        assert D.solve_nrhs(emu, h, **noop) == 0, noop
        assert D.ldiv_nrhs(emu, h, X=None, **noop) == 0, noop
        for tr in (0, 1):
            assert D.apply_q(emu, h, tr, **noop) == 0, noop
    for noop in (dict(batch=0), dict(n=0)):
        assert D.form_q(emu, h, Qb, A=None, Q=None, **noop) == 0, noop
        assert D.form_r(emu, h, Rb, A=None, al=None, R=None, **noop) == 0, noop
    odd = lambda buf, off: P(buf.ctypes.data + 16 * off + 8)  # off a 16-byte boundary
    matrix = [dict(batch=-1), dict(m=7, n=8), dict(lda=m - 1), dict(sA=D.lda * (n - 1) + m - 1), dict(A=None)]
    withal = [dict(al=None), dict(sal=n - 1)]
    block = [dict(nrhs=-1), dict(B=None), dict(ldb=m - 1), dict(sB=D.ldb * (nrhs - 1) + m - 1)]
    for kw in matrix + withal + block + [dict(A=odd(D.A, D.off)), dict(al=odd(D.al, D.off)), dict(B=odd(D.B, D.off))]:
        assert D.solve_nrhs(emu, h, **kw) == EINVAL, kw
    for kw in matrix + withal + block + [dict(X=None), dict(ldx=n - 1), dict(sX=D.ldx * (nrhs - 1) + n - 1)]:
        assert D.ldiv_nrhs(emu, h, **kw) == EINVAL, kw
    for kw in matrix + block + [dict(trans=2), dict(trans=-1), dict(A=odd(D.A, D.off)), dict(B=odd(D.B, D.off))]:
        assert D.apply_q(emu, h, kw.pop("trans", 1), **kw) == EINVAL, kw
    for kw in matrix + [dict(Q=None), dict(ldq=m - 1), dict(sQ=Qb.ld * (n - 1) + m - 1), dict(A=odd(D.A, D.off)), dict(Q=odd(Qb.buf, Qb.off))]:
        assert D.form_q(emu, h, Qb, **kw) == EINVAL, kw
    for kw in matrix + withal + [dict(R=None), dict(ldr=n - 1), dict(sR=Rb.ld * (n - 1) + n - 1), dict(A=odd(D.A, D.off)),
                                 dict(al=odd(D.al, D.off)), dict(R=odd(Rb.buf, Rb.off))]:
        assert D.form_r(emu, h, Rb, **kw) == EINVAL, kw
    assert emu.dhqr_synchronize(h) == 0
    for got, want in zip((D.A, D.al, D.B, D.X), before):
        assert same_bytes(got, want), "a rejected or empty call must not touch anything"
    assert Qb.untouched() and Rb.untouched()
    # the last column of the last matrix may be short of its leading dimension: a batch of one with the smallest strides
    one = ZNBatch(Hs[:1], _cut(Bs, nrhs, 1), als[:1])
    want = _applied(emu, h, Hs[:1], als[:1], _cut(Bs, nrhs, 1), 1)
    _ok(emu, h, one.apply_q(emu, h, 1, sA=one.lda * (n - 1) + m, sB=one.ldb * (nrhs - 1) + m))
    assert same_bytes(one.bmat(0), want.bmat(0))
    emu.dhqr_destroy(h)


def test_launch_groups(emu, factors):
    """profiling on: a wave-tier call of apply_q or form_q adds exactly ONE n_solve group whatever nrhs and batch; the solve
    one where the rule takes the multi-column kernel, nrhs (one single-column launch each) where it takes the column loop"""
    m, n = 40, 17
    mats, Hs, als, Bs = factors(m, n)
    h = _ctx(emu)
    Qb = ZOut(5, m, n)
    st = emu.Stats()
    assert emu.dhqr_set_profiling(h, 1) == 0
    for nrhs, solve_groups in ((4, 1), (8, 1), (2, 2), (5, 5)):
        D = ZNBatch(Hs, _cut(Bs, nrhs), als)
        for call, want in ((lambda: D.apply_q(emu, h, 1), 1), (lambda: D.apply_q(emu, h, 0), 1), (lambda: D.form_q(emu, h, Qb), 1),
                           (lambda: D.solve_nrhs(emu, h), solve_groups)):
            assert emu.dhqr_reset_stats(h) == 0
            _ok(emu, h, call())
            assert emu.dhqr_get_stats(h, ctypes.byref(st)) == 0
            assert st.n_solve == want, (nrhs, st.n_solve, want)
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", [(16, 8), (40, 17)])
def test_host_form_equals_the_device_form(emu, factors, m, n):
    """item 8: dhqr_ldiv_batched_nrhs_c64 on the three copy paths of batch_copy (looped | one block per matrix | one column
    pitch): the device call's bits, hB untouched, X guarded"""
    nrhs = 5
    mats, Hs, als, Bs = factors(m, n)
    cut = _cut(Bs, nrhs)
    h = _ctx(emu)
    S = _solved(emu, h, Hs, als, cut)
    for lay in (dict(pad_ld=1, pad=5, pad_ldb=1, pad_ldx=2), dict(pad_ld=0, pad=0, pad_ldb=0, pad_ldx=0), dict(pad_ld=2, pad=0, pad_ldb=2, pad_ldx=2)):
        D = ZNBatch(Hs, cut, als, **lay)
        B0 = D.B.copy()
        _ok(emu, h, D.ldiv_nrhs(emu, h))
        assert same_bytes(D.B, B0), "hB must not be modified (src:318)"
        assert D.padding_intact()
        for k in range(5):
            assert same_bytes(D.xmat(k), S.bmat(k)[:n]), (lay, k)
    emu.dhqr_destroy(h)


def test_python_front_end_errors(pkg):
    """item 9, what needs no device: a real / complex mix is a TypeError, row-major matrices are a ValueError, a host factor
    is refused by the three device-only functions; the five generic names still refuse a complex factor"""
    import torch
    c = lambda *shape: torch.zeros(shape, dtype=torch.complex128).transpose(-1, -2)  # column-major matrices
    r = lambda *shape: torch.zeros(shape, dtype=torch.float64).transpose(-1, -2)
    Hc, Hr = pkg.DistributedHouseholderQRStruct(c(4, 3, 6)), pkg.DistributedHouseholderQRStruct(r(4, 3, 6))
    for H, B in ((Hc, r(4, 2, 6)), (Hr, c(4, 2, 6))):
        for call in (lambda: pkg.solve_batched_nrhs(H, B), lambda: pkg.apply_q_batched_(H, B, True)):
            with pytest.raises(TypeError, match="convert one of them explicitly"):
                call()
    with pytest.raises(TypeError, match="convert one of them explicitly"):
        pkg.form_r_batched(pkg.DistributedHouseholderQRStruct(c(4, 3, 6), torch.zeros((4, 3), dtype=torch.float64)))
    Hrow = pkg.DistributedHouseholderQRStruct(torch.zeros((4, 6, 3), dtype=torch.complex128))  # row-major matrices
    for call in (lambda: pkg.form_q_batched(Hrow), lambda: pkg.form_r_batched(Hrow), lambda: pkg.apply_q_batched_(Hrow, c(4, 2, 6), True),
                 lambda: pkg.solve_batched_nrhs(Hrow, c(4, 2, 6)),
                 lambda: pkg.apply_q_batched_(Hc, torch.zeros((4, 6, 2), dtype=torch.complex128), False),
                 lambda: pkg.solve_batched_nrhs(Hc, torch.zeros((4, 6, 2), dtype=torch.complex128))):
        with pytest.raises(ValueError, match="column-major"):
            call()
    Hn = pkg.DistributedHouseholderQRStruct(np.zeros((4, 6, 3), dtype=np.complex128))
    for call in (lambda: pkg.apply_q_batched_(Hn, np.zeros((4, 6, 2), dtype=np.complex128), True), lambda: pkg.form_q_batched(Hn),
                 lambda: pkg.form_r_batched(Hn)):
        with pytest.raises(TypeError, match="device tensors only"):
            call()
    # the pinned behaviour of the generic names beside the new one
    H2 = pkg.DistributedHouseholderQRStruct(c(3, 6))
    with pytest.raises(TypeError):
        pkg.ldiv(H2, c(2, 6))
    with pytest.raises(TypeError):
        pkg.solve_householder_(c(2, 6), H2.A, H2.α)
    with pytest.raises(TypeError):
        pkg.ldiv_batched(Hc, c(4, 2, 6))
    with pytest.raises(TypeError):
        pkg.get_q(Hc)
    with pytest.raises(TypeError):
        pkg.get_r(Hc)
