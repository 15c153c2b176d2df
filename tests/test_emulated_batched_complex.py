"""Batches of small ComplexF64 matrices (dhqr_factor_batched_c64 / dhqr_solve_batched_c64 / dhqr_qr_batched_c64 /
dhqr_ldiv_batched_c64) through the C ABI of the EMULATED library (csrc/ host-compiled against tests/simt/fake, fiber mode):
the wave-per-matrix kernels of csrc/dhqr_batched_complex.h against the oracle under the rule of zbatched_helpers.py, the
serial tier bit for bit against the single-matrix calls, guarded strides, launch-group counts, the argument rules and the
empty cases, the host pair, a zero column inside a batch."""
import ctypes
import os

import numpy as np
import pytest

import zbatched_helpers as zh
from zbatched_helpers import SENT, ZBatch, cptr

P = ctypes.c_void_p
EINVAL = -1
ZNB = 64


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


def _stats(L, h):
    st = L.Stats()
    assert L.dhqr_get_stats(h, ctypes.byref(st)) == 0
    return st


def _single(L, h, A0, b0, nb=0):
    """dhqr_factor_c64_nb + dhqr_solve_c64 on one packed matrix"""
    m, n = A0.shape
    A = A0.copy(order="F")
    al = np.zeros(n, dtype=np.complex128)
    bb = b0.copy()
    assert L.dhqr_factor_c64_nb(h, cptr(A), m, n, m, cptr(al), nb) == 0, L.dhqr_last_error()
    assert L.dhqr_solve_c64(h, cptr(A), m, n, m, cptr(al), cptr(bb)) == 0, L.dhqr_last_error()
    assert L.dhqr_synchronize(h) == 0
    return A, al, bb


@pytest.mark.parametrize("m,n", zh.WAVE_SHAPES)
def test_wave_tier_vs_oracle(emu, orc, m, n):
    """one wave per matrix (k_batched_zqr_wave / k_batched_zldiv_wave) on a padded, offset, sentinel-guarded layout: nine
    matrices, every one within 8 T of the oracle and at most one above T; x within 1e-9; the tail of Q'b; padding untouched"""
    mats, bs = zh.inputs(orc, m, n, range(9))
    h = _ctx(emu)
    B = ZBatch(mats, bs)
    assert B.factor(emu, h) == 0, emu.dhqr_last_error()
    assert emu.dhqr_synchronize(h) == 0
    assert B.padding_intact()
    Hd = [B.mat(k).copy() for k in range(9)]
    ad = [B.alpha(k).copy() for k in range(9)]
    assert B.solve(emu, h) == 0, emu.dhqr_last_error()
    assert emu.dhqr_synchronize(h) == 0
    assert B.padding_intact()
    ratios, dxs = [], []
    for k in range(9):
        Ho, ao, xo = zh.reference(orc, mats[k], bs[k])
        ratios.append(zh.ratio_H(Ho, ao, Hd[k], ad[k]))
        dxs.append(np.abs(B.rhs(k)[:n] - xo).max() / np.abs(xo).max())
        assert np.array_equal(B.mat(k), Hd[k]) and np.array_equal(B.alpha(k), ad[k]), "the solve must not touch the factor"
        if m > n:  # the reference leaves Q'b below the triangle (src:284-294)
            qtb = bs[k].copy()
            for j in range(n):
                qtb[j:] -= Ho[j:, j] * np.vdot(Ho[j:, j], qtb[j:])
            assert np.abs(B.rhs(k)[n:] - qtb[n:]).max() <= 1e-12 * max(1.0, np.abs(qtb).max())
    zh.check_rule(f"emulated {m}x{n}", ratios, dxs, above_allowed=1)
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n,small", [(66, 33, 1), (130, 20, 1), (16, 8, 0)])
@pytest.mark.parametrize("nb", [0, ZNB])
def test_serial_tier_is_the_single_call_bit_for_bit(emu, orc, m, n, small, nb):
    """beyond 64 x 32, and at every shape with the small route off: dhqr_factor_c64_nb(nb) / dhqr_solve_c64 on matrix k alone"""
    mats, bs = zh.inputs(orc, m, n, range(3), seed=200, bseed=5200)
    h = _ctx(emu, small=small)
    B = ZBatch(mats, bs, pad_ld=0, pad=0, off=0)  # (the layout of the single calls below)
    assert B.factor(emu, h, nb=nb) == 0, emu.dhqr_last_error()
    assert B.solve(emu, h) == 0, emu.dhqr_last_error()
    for k in range(3):
        A, al, bb = _single(emu, h, mats[k], bs[k], nb)
        assert np.array_equal(B.mat(k), A) and np.array_equal(B.alpha(k), al) and np.array_equal(B.rhs(k), bb)
    G = ZBatch(mats, bs)  # padded and offset: the same numbers within the rule, nothing written outside
    assert G.factor(emu, h, nb=nb) == 0 and G.solve(emu, h) == 0, emu.dhqr_last_error()
    assert G.padding_intact()
    for k in range(3):
        scale = np.abs(B.mat(k)).max()
        assert np.abs(G.mat(k) - B.mat(k)).max() <= zh.T(n) * scale
    emu.dhqr_destroy(h)


def test_guarded_strides_give_the_packed_bits(emu, orc):
    """(40, 17): lda = m + 1, strideA / strideb padded, stride_alpha = n + 3, base one complex element in -- the packed
    call's bits, every sentinel intact"""
    m, n = 40, 17
    mats, bs = zh.inputs(orc, m, n, range(5), seed=300, bseed=5300)
    h = _ctx(emu)
    G, Pk = ZBatch(mats, bs), ZBatch(mats, bs, pad_ld=0, pad=0, off=0)
    assert (G.lda, G.sal, G.off) == (m + 1, n + 3, 1)
    for B in (G, Pk):
        assert B.factor(emu, h) == 0 and B.solve(emu, h) == 0, emu.dhqr_last_error()
    assert emu.dhqr_synchronize(h) == 0
    assert G.padding_intact()
    for k in range(5):
        assert np.array_equal(G.mat(k), Pk.mat(k)) and np.array_equal(G.alpha(k), Pk.alpha(k)) and np.array_equal(G.rhs(k), Pk.rhs(k))
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("batch", [1, 3, 4, 5])
def test_independence_and_partial_workgroups(emu, orc, batch):
    """matrix k has the bits of a batch of one holding it alone; a workgroup's last waves without a matrix write nothing"""
    m, n = 16, 8
    mats, bs = zh.inputs(orc, m, n, range(batch), seed=350, bseed=5350)
    h = _ctx(emu)
    B = ZBatch(mats, bs)
    assert B.factor(emu, h) == 0 and B.solve(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    assert B.padding_intact()
    for k in range(batch):
        O = ZBatch(mats[k:k + 1], bs[k:k + 1], pad_ld=0, pad=0, off=0)
        assert O.factor(emu, h) == 0 and O.solve(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
        assert np.array_equal(B.mat(k), O.mat(0)) and np.array_equal(B.alpha(k), O.alpha(0)) and np.array_equal(B.rhs(k), O.rhs(0))
    emu.dhqr_destroy(h)


def test_launch_group_counts(emu, orc):
    """profiling on: the wave tier counts ONE n_rank1 group per factor call and ONE n_solve per solve call; the serial tier
    counts what the single calls count"""
    m, n = 16, 8
    mats, bs = zh.inputs(orc, m, n, range(7), seed=400, bseed=5400)
    h = _ctx(emu)
    assert emu.dhqr_set_profiling(h, 1) == 0 and emu.dhqr_reset_stats(h) == 0
    B = ZBatch(mats, bs)
    assert B.factor(emu, h, nb=ZNB) == 0  # (nb is ignored on this tier)
    st = _stats(emu, h)
    assert (st.n_rank1, st.n_panel, st.n_solve) == (1, 0, 0)
    assert B.solve(emu, h) == 0
    st = _stats(emu, h)
    assert (st.n_rank1, st.n_panel, st.n_solve) == (1, 0, 1)
    assert emu.dhqr_set_small_route(h, 0) == 0  # the serial tier: two matrices, against two single calls
    B2 = ZBatch(mats[:2], bs[:2], pad_ld=0, pad=0, off=0)
    assert emu.dhqr_reset_stats(h) == 0
    assert B2.factor(emu, h) == 0 and B2.solve(emu, h) == 0
    st = _stats(emu, h)
    batched = (st.n_rank1, st.n_panel, st.n_solve)
    assert emu.dhqr_reset_stats(h) == 0
    for k in range(2):
        A, al, bb = _single(emu, h, mats[k], bs[k])
        assert np.array_equal(B2.mat(k), A) and np.array_equal(B2.alpha(k), al) and np.array_equal(B2.rhs(k), bb)
    st = _stats(emu, h)
    assert batched == (st.n_rank1, st.n_panel, st.n_solve) and st.n_solve == 2
    emu.dhqr_destroy(h)


def test_argument_rules_and_empty_cases(emu, orc):
    m, n, batch = 12, 6, 3
    mats, bs = zh.inputs(orc, m, n, range(batch), seed=600, bseed=5600)
    h = _ctx(emu)
    B = ZBatch(mats, bs)
    A, al, b = B.pA(), B.pal(), B.pb()
    x = np.full(batch * n, SENT)
    before = (B.A.copy(), B.al.copy(), B.b.copy(), x.copy())

    def solves(m=m, n=n, lda=B.lda, sA=B.sA, sal=B.sal, sb=B.sb, sx=n, batch=batch, A=A, al=al, b=b, xp=cptr(x)):
        return (emu.dhqr_solve_batched_c64(h, A, m, n, lda, sA, al, sal, b, sb, batch),
                emu.dhqr_ldiv_batched_c64(h, A, m, n, lda, sA, al, sal, b, sb, xp, sx, batch))

    def all_four(nb=0, **kw):
        a = dict(m=m, n=n, lda=B.lda, sA=B.sA, sal=B.sal, batch=batch, A=A, al=al)
        a.update({k: v for k, v in kw.items() if k in a})
        return (emu.dhqr_factor_batched_c64(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["al"], a["sal"], a["batch"], nb),
                emu.dhqr_qr_batched_c64(h, a["A"], a["m"], a["n"], a["lda"], a["sA"], a["al"], a["sal"], a["batch"], nb)) + solves(**kw)

    assert all_four(batch=0) == (0, 0, 0, 0)
    assert all_four(n=0) == (0, 0, 0, 0)
    assert all_four(batch=0, A=None, al=None, b=None, xp=None) == (0, 0, 0, 0)  # an empty call looks at no pointer
    assert all_four(batch=0, nb=7)[:2] == (0, 0)
    assert all_four(batch=-1) == (EINVAL,) * 4
    assert all_four(m=5, n=6) == (EINVAL,) * 4                # m < n
    assert all_four(lda=m - 1) == (EINVAL,) * 4
    assert all_four(sA=B.lda * (n - 1) + m - 1) == (EINVAL,) * 4
    assert all_four(sal=n - 1) == (EINVAL,) * 4
    assert all_four(A=None) == (EINVAL,) * 4
    assert all_four(al=None) == (EINVAL,) * 4
    assert solves(sb=m - 1) == (EINVAL, EINVAL)
    assert solves(b=None) == (EINVAL, EINVAL)
    assert emu.dhqr_ldiv_batched_c64(h, A, m, n, B.lda, B.sA, al, B.sal, b, B.sb, cptr(x), n - 1, batch) == EINVAL
    assert emu.dhqr_ldiv_batched_c64(h, A, m, n, B.lda, B.sA, al, B.sal, b, B.sb, None, n, batch) == EINVAL
    for nb in (128, 1):                                       # nb: 0 or DHQR_ZNB = 64
        assert emu.dhqr_factor_batched_c64(h, A, m, n, B.lda, B.sA, al, B.sal, batch, nb) == EINVAL
        assert emu.dhqr_qr_batched_c64(h, A, m, n, B.lda, B.sA, al, B.sal, batch, nb) == EINVAL
    odd = P(B.A.ctypes.data + 8)                              # device pointers: 16-byte aligned
    assert emu.dhqr_factor_batched_c64(h, odd, m, n, B.lda, B.sA, al, B.sal, batch, 0) == EINVAL
    assert emu.dhqr_solve_batched_c64(h, A, m, n, B.lda, B.sA, al, B.sal, P(B.b.ctypes.data + 8), B.sb, batch) == EINVAL
    for got, want in zip((B.A, B.al, B.b, x), before):
        assert np.array_equal(got, want), "a rejected or empty call must not touch anything"
    # the last column of the last matrix may be short of lda: strideA = lda*(n-1) + m is accepted
    sA = B.lda * (n - 1) + m
    Tt = np.full(batch * sA, SENT)
    for k in range(batch):
        for j in range(n):
            Tt[k * sA + j * B.lda: k * sA + j * B.lda + m] = mats[k][:, j]
    assert emu.dhqr_factor_batched_c64(h, cptr(Tt), m, n, B.lda, sA, al, B.sal, batch, 0) == 0
    assert B.factor(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    for k in range(batch):
        for j in range(n):
            assert np.array_equal(Tt[k * sA + j * B.lda: k * sA + j * B.lda + m], B.mat(k)[:, j])
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", [(16, 8), (40, 17), (66, 33)])
def test_host_pair_equals_device_pair(emu, orc, m, n):
    """dhqr_qr_batched_c64 / dhqr_ldiv_batched_c64 on every copy path of the staging (looped | one block per matrix | one
    column pitch): the device pair's bits; hb untouched; x guarded; dhqr_trim releases the staging buffer"""
    mats, bs = zh.inputs(orc, m, n, range(4), seed=500, bseed=5500)
    h = _ctx(emu)
    D = ZBatch(mats, bs)
    assert D.factor(emu, h) == 0 and D.solve(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    for pad_ld, pad in ((1, 5), (0, 0), (2, 0)) if m <= 64 else ((1, 5),):  # (the serial tier is slow on the emulator: one path)
        Hb = ZBatch(mats, bs, pad_ld=pad_ld, pad=pad)
        assert emu.dhqr_qr_batched_c64(h, Hb.pA(), m, n, Hb.lda, Hb.sA, Hb.pal(), Hb.sal, 4, 0) == 0, emu.dhqr_last_error()
        b0 = Hb.b.copy()
        sx = n + 2
        x = np.full(4 * sx + 3, SENT)
        assert emu.dhqr_ldiv_batched_c64(h, Hb.pA(), m, n, Hb.lda, Hb.sA, Hb.pal(), Hb.sal, Hb.pb(), Hb.sb, cptr(x), sx, 4) == 0
        assert np.array_equal(Hb.b, b0), "hb must not be modified (src:318)"
        for k in range(4):
            assert np.array_equal(Hb.mat(k), D.mat(k)) and np.array_equal(Hb.alpha(k), D.alpha(k))
            assert np.array_equal(x[k * sx: k * sx + n], D.rhs(k)[:n])
            assert np.all(x[k * sx + n: (k + 1) * sx] == SENT)
        assert Hb.padding_intact()
    if m <= 64:
        assert emu.dhqr_trim(h) == 0  # releases the device copy of the batch; the next call allocates again
        Hb = ZBatch(mats, bs)
        assert emu.dhqr_qr_batched_c64(h, Hb.pA(), m, n, Hb.lda, Hb.sA, Hb.pal(), Hb.sal, 4, 0) == 0
        assert all(np.array_equal(Hb.mat(k), D.mat(k)) for k in range(4))
    emu.dhqr_destroy(h)


def test_zero_column_inside_a_batch(emu, orc):
    """matrix 2 of five has a zero column 3: its isfinite masks of H and alpha are the oracle's (columns 0-2 finite, alpha_3 =
    -0, everything from row 3 on of the columns >= 3 non-finite); every other matrix has the bits it has without that
    neighbour"""
    m, n = 16, 8
    mats, bs = zh.inputs(orc, m, n, range(5), seed=700, bseed=5700)
    bad = [zh.poison_column(A) if k == 2 else A for k, A in enumerate(mats)]
    h = _ctx(emu)
    G, B = ZBatch(mats, bs), ZBatch(bad, bs)
    for X in (G, B):
        assert X.factor(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    Ho, ao = orc.householder_c(bad[2])
    assert np.isfinite(Ho[:, :3]).all() and np.isfinite(Ho[:3]).all() and not np.isfinite(Ho[3:, 3:]).any()
    assert ao[3] == 0 and np.isfinite(ao[:4]).all() and not np.isfinite(ao[4:]).any()
    assert np.array_equal(np.isfinite(B.mat(2)), np.isfinite(Ho)) and np.array_equal(np.isfinite(B.alpha(2)), np.isfinite(ao))
    assert B.alpha(2)[3] == 0
    scale = np.abs(Ho[:, :3]).max()
    assert np.abs(B.mat(2)[:, :3] - Ho[:, :3]).max() <= zh.T(n) * scale and np.abs(B.alpha(2)[:3] - ao[:3]).max() <= zh.T(n) * scale
    for k in (0, 1, 3, 4):
        assert np.array_equal(B.mat(k), G.mat(k)) and np.array_equal(B.alpha(k), G.alpha(k))
    assert B.padding_intact()
    emu.dhqr_destroy(h)
