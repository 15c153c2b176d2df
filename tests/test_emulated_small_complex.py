"""The one-workgroup ComplexF64 tier (csrc/dhqr_small_complex.h: k_small_zqr / k_small_zldiv, 1 <= n <= m <= 128) through the C
ABI of the EMULATED library (csrc/ host-compiled against tests/simt/fake, fiber mode), small route on: the single-matrix
calls against the oracle under the rule of zbatched_helpers.py, single = batch of one bit for bit, guarded strides, the
host-array forms, launch-group counts, special inputs and a zero column inside a batch."""
import ctypes
import os

import numpy as np
import pytest

import zbatched_helpers as zh
from zbatched_helpers import SENT, ZBatch, cptr

P = ctypes.c_void_p
EINVAL = -1
ZNB = 64
ORACLE_SHAPES = [(65, 1), (66, 33), (65, 65), (97, 64), (110, 100), (128, 128)]


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
    return (st.n_rank1, st.n_panel, st.n_solve)


def _factor(L, h, A0, nb=None):
    """dhqr_factor_c64 (nb = None) or dhqr_factor_c64_nb on one packed matrix -> (rc, H, alpha)"""
    m, n = A0.shape
    A = A0.copy(order="F")
    al = np.zeros(n, dtype=np.complex128)
    if nb is None:
        rc = L.dhqr_factor_c64(h, cptr(A), m, n, m, cptr(al))
    else:
        rc = L.dhqr_factor_c64_nb(h, cptr(A), m, n, m, cptr(al), nb)
    assert L.dhqr_synchronize(h) == 0
    return rc, A, al


def _solve(L, h, H, al, b0):
    m, n = H.shape
    bb = b0.copy()
    assert L.dhqr_solve_c64(h, cptr(H), m, n, m, cptr(al), cptr(bb)) == 0, L.dhqr_last_error()
    assert L.dhqr_synchronize(h) == 0
    return bb


def _single(L, h, A0, b0):
    rc, H, al = _factor(L, h, A0)
    assert rc == 0, L.dhqr_last_error()
    return H, al, _solve(L, h, H, al, b0)


@pytest.mark.parametrize("m,n", ORACLE_SHAPES)
def test_single_calls_vs_oracle(emu, orc, m, n):
    """dhqr_factor_c64 + dhqr_solve_c64 on nine matrices: every one within 8 T of the oracle, at most one above T, x within
    1e-9, A = QR to 1e-12, the tail of Q^H b; the solve leaves the factor alone; nb = 64 gives nb = 0's bits, nb = 32 is
    DHQR_EINVAL"""
    mats, bs = zh.inputs(orc, m, n, range(9))
    h = _ctx(emu)
    ratios, dxs = [], []
    for k in range(9):
        rc, H, al = _factor(emu, h, mats[k])
        assert rc == 0, emu.dhqr_last_error()
        H0, al0 = H.copy(), al.copy()
        bb = _solve(emu, h, H, al, bs[k])
        assert np.array_equal(H, H0) and np.array_equal(al, al0), "the solve must not touch the factor"
        Ho, ao, xo = zh.reference(orc, mats[k], bs[k])
        ratios.append(zh.ratio_H(Ho, ao, H, al))
        dxs.append(np.abs(bb[:n] - xo).max() / np.abs(xo).max())
        if m > n:  # the reference leaves Q^H b below the triangle (src:284-294)
            qtb = bs[k].copy()
            for j in range(n):
                qtb[j:] -= Ho[j:, j] * np.vdot(Ho[j:, j], qtb[j:])
            assert np.abs(bb[n:] - qtb[n:]).max() <= 1e-12 * max(1.0, np.abs(qtb).max())
        if k == 0:
            QR = orc.form_qr_c(np.asfortranarray(H), al)
            assert np.linalg.norm(mats[k] - QR) / np.linalg.norm(mats[k]) < 1e-12
            rc, Hb, alb = _factor(emu, h, mats[k], nb=ZNB)
            assert rc == 0 and np.array_equal(Hb, H) and np.array_equal(alb, al), "the route is taken whatever nb says"
            rc, Hc, _ = _factor(emu, h, mats[k], nb=32)
            assert rc == EINVAL and np.array_equal(Hc, mats[k])
    zh.check_rule(f"emulated single {m}x{n}", ratios, dxs, above_allowed=1)
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", [(16, 8), (64, 32), (66, 33), (128, 128)])
def test_single_is_a_batch_of_one(emu, orc, m, n):
    mats, bs = zh.inputs(orc, m, n, range(1), seed=210, bseed=5210)
    h = _ctx(emu)
    H, al, bb = _single(emu, h, mats[0], bs[0])
    B = ZBatch(mats, bs, pad_ld=0, pad=0, off=0)
    assert B.factor(emu, h) == 0 and B.solve(emu, h) == 0 and emu.dhqr_synchronize(h) == 0, emu.dhqr_last_error()
    assert np.array_equal(B.mat(0), H) and np.array_equal(B.alpha(0), al) and np.array_equal(B.rhs(0), bb)
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", [(66, 33), (70, 40)])
def test_guarded_batch_gives_the_single_calls_bits(emu, orc, m, n):
    """a batch of three with lda = m + 1, padded strides, stride_alpha = n + 3 and the base one complex element in: the bits
    of the three packed single calls, every sentinel intact"""
    mats, bs = zh.inputs(orc, m, n, range(3), seed=220, bseed=5220)
    h = _ctx(emu)
    G = ZBatch(mats, bs)
    assert (G.lda, G.sal, G.off) == (m + 1, n + 3, 1)
    assert G.factor(emu, h, nb=ZNB) == 0 and emu.dhqr_synchronize(h) == 0, emu.dhqr_last_error()  # (nb is ignored on this tier)
    assert G.padding_intact()
    assert G.solve(emu, h) == 0 and emu.dhqr_synchronize(h) == 0, emu.dhqr_last_error()
    assert G.padding_intact()
    for k in range(3):
        H, al, bb = _single(emu, h, mats[k], bs[k])
        assert np.array_equal(G.mat(k), H) and np.array_equal(G.alpha(k), al) and np.array_equal(G.rhs(k), bb)
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", [(16, 8), (66, 33), (110, 100)])
def test_host_arrays_equal_the_device_calls(emu, orc, m, n):
    """dhqr_qr_c64 / dhqr_qr_c64_nb / dhqr_ldiv_c64 on a host lda = m + 3: the bits of the device-resident calls, rows beyond
    m untouched, hb unmodified, x guarded; once more after dhqr_trim"""
    mats, bs = zh.inputs(orc, m, n, range(1), seed=230, bseed=5230)
    h = _ctx(emu)
    H, al, bb = _single(emu, h, mats[0], bs[0])
    lda = m + 3
    for nb in (None, 0, ZNB, None):
        F = np.full((lda, n), SENT, order="F")
        F[:m] = mats[0]
        alh = np.full(n + 2, SENT)
        if nb is None:
            assert emu.dhqr_qr_c64(h, cptr(F), m, n, lda, cptr(alh)) == 0, emu.dhqr_last_error()
        else:
            assert emu.dhqr_qr_c64_nb(h, cptr(F), m, n, lda, cptr(alh), nb) == 0, emu.dhqr_last_error()
        assert np.array_equal(F[:m], H) and np.all(F[m:] == SENT)
        assert np.array_equal(alh[:n], al) and np.all(alh[n:] == SENT)
        b0 = bs[0].copy()
        x = np.full(n + 2, SENT)
        assert emu.dhqr_ldiv_c64(h, cptr(F), m, n, lda, cptr(alh), cptr(b0), cptr(x)) == 0, emu.dhqr_last_error()
        assert np.array_equal(b0, bs[0]), "hb must not be modified (src:318)"
        assert np.array_equal(x[:n], bb[:n]) and np.all(x[n:] == SENT)
        assert np.array_equal(F[:m], H) and np.all(F[m:] == SENT) and np.array_equal(alh[:n], al)
        assert emu.dhqr_trim(h) == 0  # releases the pinned staging buffer; the next call allocates again
    assert emu.dhqr_qr_c64_nb(h, cptr(F), m, n, lda, cptr(alh), 32) == EINVAL
    emu.dhqr_destroy(h)


def test_launch_group_counts(emu, orc):
    """profiling on.  (66, 33), batch 3: ONE n_rank1 group for the factor call and ONE n_solve for the solve call (the serial
    tier this shape had before counted three of each); (129, 20): the serial tier, what three single calls count; the small
    route off: (66, 33) counts what three single calls count with the route off"""
    h = _ctx(emu)
    assert emu.dhqr_set_profiling(h, 1) == 0

    def batched(m, n, seed):
        mats, bs = zh.inputs(orc, m, n, range(3), seed=seed, bseed=seed + 5000)
        B = ZBatch(mats, bs, pad_ld=0, pad=0, off=0)
        assert emu.dhqr_reset_stats(h) == 0
        assert B.factor(emu, h) == 0, emu.dhqr_last_error()
        after_factor = _stats(emu, h)
        assert B.solve(emu, h) == 0 and emu.dhqr_synchronize(h) == 0, emu.dhqr_last_error()
        both = _stats(emu, h)
        assert emu.dhqr_reset_stats(h) == 0
        for k in range(3):
            H, al, bb = _single(emu, h, mats[k], bs[k])
            assert np.array_equal(B.mat(k), H) and np.array_equal(B.alpha(k), al) and np.array_equal(B.rhs(k), bb)
        return after_factor, both, _stats(emu, h)

    after_factor, both, singles = batched(66, 33, 240)
    assert after_factor == (1, 0, 0) and both == (1, 0, 1)
    assert singles == (3, 0, 3)  # a single call on the route: one group each
    _, both, singles = batched(129, 20, 250)
    assert both == singles and both[2] == 3
    assert emu.dhqr_set_small_route(h, 0) == 0
    _, both, singles = batched(66, 33, 240)
    assert both == singles and both[2] == 3
    emu.dhqr_destroy(h)


def test_special_matrices_in_one_batch(emu, orc):
    """(66, 33): an imaginary part identically zero, a real part identically zero, a pivot exactly 0 above a nonzero rest,
    ordinary ones -- ONE batch, every matrix within 8 T, at most one above T"""
    m, n = 66, 33
    mats = zh.special_matrices(orc, m, n)
    bs = [orc.rand_vector_c(m, 5900 + k) for k in range(7)]
    h = _ctx(emu)
    B = ZBatch(mats, bs)
    assert B.factor(emu, h) == 0 and emu.dhqr_synchronize(h) == 0, emu.dhqr_last_error()
    Hd = [B.mat(k).copy() for k in range(7)]
    ad = [B.alpha(k).copy() for k in range(7)]
    assert B.solve(emu, h) == 0 and emu.dhqr_synchronize(h) == 0, emu.dhqr_last_error()
    assert B.padding_intact()
    ratios, dxs = [], []
    for k in range(7):
        Ho, ao, xo = zh.reference(orc, mats[k], bs[k])
        ratios.append(zh.ratio_H(Ho, ao, Hd[k], ad[k]))
        dxs.append(np.abs(B.rhs(k)[:n] - xo).max() / np.abs(xo).max())
    for k in (1, 5):
        assert (Hd[k].imag == 0).all() and (ad[k].imag == 0).all(), "a real matrix stays real"
    for k in (3, 5):  # alphafactor(0) = -1: alpha_0 = -||a_0||
        assert ad[k][0].real < 0 and ad[k][0].imag == 0
    zh.check_rule(f"emulated special {m}x{n}", ratios, dxs, above_allowed=1)
    emu.dhqr_destroy(h)


def test_zero_column_inside_a_batch(emu, orc):
    """matrix 1 of three at (66, 33) has a zero column 3: its isfinite masks of H and alpha are the oracle's (columns 0-2
    and rows 0-2 finite, alpha_3 = -0, everything from row 3 on of the columns >= 3 non-finite); its neighbours have the
    bits they have without it"""
    m, n = 66, 33
    mats, bs = zh.inputs(orc, m, n, range(3), seed=700, bseed=5700)
    bad = [zh.poison_column(A, 3) if k == 1 else A for k, A in enumerate(mats)]
    h = _ctx(emu)
    G, B = ZBatch(mats, bs), ZBatch(bad, bs)
    for X in (G, B):
        assert X.factor(emu, h) == 0 and emu.dhqr_synchronize(h) == 0, emu.dhqr_last_error()
    Ho, ao = orc.householder_c(bad[1])
    assert np.isfinite(Ho[:, :3]).all() and np.isfinite(Ho[:3]).all() and not np.isfinite(Ho[3:, 3:]).any()
    assert ao[3] == 0 and np.isfinite(ao[:4]).all() and not np.isfinite(ao[4:]).any()
    assert np.array_equal(np.isfinite(B.mat(1)), np.isfinite(Ho)) and np.array_equal(np.isfinite(B.alpha(1)), np.isfinite(ao))
    assert B.alpha(1)[3] == 0
    scale = np.abs(Ho[:, :3]).max()
    assert np.abs(B.mat(1)[:, :3] - Ho[:, :3]).max() <= zh.T(n) * scale and np.abs(B.alpha(1)[:3] - ao[:3]).max() <= zh.T(n) * scale
    assert np.abs(B.mat(1)[:3, 3:] - Ho[:3, 3:]).max() <= zh.T(n) * scale, "R above the zero column's row stays"
    for k in (0, 2):
        assert np.array_equal(B.mat(k), G.mat(k)) and np.array_equal(B.alpha(k), G.alpha(k))
    assert B.padding_intact()
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("row", [0, 40, 64])
def test_one_column_with_a_single_entry(emu, orc, row):
    """65 x 1, one nonzero entry: at the pivot (alpha = -entry, v = sqrt(2) e_0 up to phase) or below it (pivot 0: the factor
    -1 of alphafactor)"""
    m, n = 65, 1
    A0 = np.zeros((m, n), dtype=np.complex128, order="F")
    A0[row, 0] = 3 - 4j
    b0 = orc.rand_vector_c(m, 5800)
    h = _ctx(emu)
    H, al, bb = _single(emu, h, A0, b0)
    Ho, ao, xo = zh.reference(orc, A0, b0)
    assert np.isfinite(H).all() and np.isfinite(al).all()
    zh.check_rule(f"emulated e_{row}", [zh.ratio_H(Ho, ao, H, al)], [np.abs(bb[:n] - xo).max() / np.abs(xo).max()], above_allowed=0)
    assert abs(abs(al[0]) - 5.0) <= zh.T(n) * 5.0
    emu.dhqr_destroy(h)
