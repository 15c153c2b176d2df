"""Batches of small matrices (dhqr_factor_batched_f64 / dhqr_solve_batched_f64 / dhqr_qr_batched_f64 /
dhqr_ldiv_batched_f64) through the C ABI of the EMULATED library (csrc/ host-compiled against tests/simt/fake, fiber
mode): the wave-per-matrix kernels of csrc/dhqr_batched.h against the oracle, the one-workgroup-per-matrix tier bit for bit
against the single-matrix calls, the launch-group counts, the host pair, the argument rules."""
import ctypes

import numpy as np
import pytest

P = ctypes.c_void_p
SENT = -7.25  # fills every element between and behind the matrices / vectors of a batch


def _ptr(a):
    return a.ctypes.data_as(P)


@pytest.fixture(scope="module")
def emu(emulated_so):
    from dist_helpers import load_emulated_library
    return load_emulated_library(emulated_so)


def _ctx(L, monkeypatch=None, small=1, tune=None):
    import os
    old = {k: os.environ.get(k) for k in ("DHQR_SMALL", "DHQR_TUNE")}
    os.environ["DHQR_SMALL"] = str(small)
    if tune is not None:
        os.environ["DHQR_TUNE"] = tune
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


class Batch:
    """a strided batch in flat sentinel-filled buffers: matrix k at A[k*sA:], leading dimension lda"""

    def __init__(self, mats, bs, pad_ld=3, pad=5):
        self.batch, (self.m, self.n) = len(mats), mats[0].shape
        m, n = self.m, self.n
        self.lda = m + pad_ld
        self.sA = self.lda * n + pad
        self.sal = n + pad
        self.sb = m + pad
        self.A = np.full(self.batch * self.sA + 7, SENT)
        self.al = np.full(self.batch * self.sal + 7, SENT)
        self.b = np.full(self.batch * self.sb + 7, SENT)
        self.maskA = np.zeros(self.A.size, bool)
        self.maskb = np.zeros(self.b.size, bool)
        for k in range(self.batch):
            self.mat(k)[...] = mats[k]
            for j in range(n):
                self.maskA[k * self.sA + j * self.lda: k * self.sA + j * self.lda + m] = True
            self.b[k * self.sb: k * self.sb + m] = bs[k]
            self.maskb[k * self.sb: k * self.sb + m] = True

    def mat(self, k):
        return self.A[k * self.sA: k * self.sA + self.lda * self.n].reshape((self.lda, self.n), order="F")[:self.m]

    def alpha(self, k):
        return self.al[k * self.sal: k * self.sal + self.n]

    def rhs(self, k):
        return self.b[k * self.sb: k * self.sb + self.m]

    def padding_intact(self):
        maskal = np.zeros(self.al.size, bool)
        for k in range(self.batch):
            maskal[k * self.sal: k * self.sal + self.n] = True
        return (np.all(self.A[~self.maskA] == SENT) and np.all(self.al[~maskal] == SENT)
                and np.all(self.b[~self.maskb] == SENT))

    def factor(self, L, h, nb=0):
        return L.dhqr_factor_batched_f64(h, _ptr(self.A), self.m, self.n, self.lda, self.sA, _ptr(self.al), self.sal,
                                         self.batch, nb)

    def solve(self, L, h):
        return L.dhqr_solve_batched_f64(h, _ptr(self.A), self.m, self.n, self.lda, self.sA, _ptr(self.al), self.sal,
                                        _ptr(self.b), self.sb, self.batch)


def _inputs(orc, m, n, batch, seed):
    return ([orc.rand_matrix(m, n, seed + k) for k in range(batch)],
            [orc.rand_vector(m, seed + 1000 + k) for k in range(batch)])


def _stats(L, h):
    st = L.Stats()
    assert L.dhqr_get_stats(h, ctypes.byref(st)) == 0
    return st


WAVE_SHAPES = [(1, 1), (5, 3), (12, 6), (16, 8), (33, 9), (40, 17), (64, 32), (32, 32)]


@pytest.mark.parametrize("m,n", WAVE_SHAPES)
def test_wave_tier_vs_oracle(emu, orc, m, n):
    """one wave per matrix (k_batched_qr_wave / k_batched_ldiv_wave): factor, alpha, x and the tail of Q'b against the
    oracle on a padded strided layout whose padding stays untouched.  Tolerances: those of test_emulated_library.py
    (_check: 1e-12 of max|H|; the small route's solve: 1e-10 of max|x|, 1e-12 for the tail)."""
    mats, bs = _inputs(orc, m, n, 5, 100)
    for A0 in mats:  # the x tolerance is about the kernel, not the matrix
        assert np.linalg.cond(A0, 2) <= 1e4
    h = _ctx(emu)
    B = Batch(mats, bs)
    assert B.factor(emu, h) == 0, emu.dhqr_last_error()
    assert emu.dhqr_synchronize(h) == 0
    ref = []
    for k, A0 in enumerate(mats):
        Ho, ao = orc.householder(A0)
        ref.append((Ho, ao))
        scale = np.abs(Ho).max()
        eH, ea = np.abs(B.mat(k) - Ho).max(), np.abs(B.alpha(k) - ao).max()
        print(f"{m}x{n} k={k}: |dH|={eH / scale:.2e} |dalpha|={ea / scale:.2e}")
        assert eH <= 1e-12 * scale
        assert ea <= 1e-12 * scale
    assert B.padding_intact()
    assert B.solve(emu, h) == 0, emu.dhqr_last_error()
    assert emu.dhqr_synchronize(h) == 0
    for k, (Ho, ao) in enumerate(ref):
        xo = orc.solve(Ho, ao, bs[k])
        ex = np.abs(B.rhs(k)[:n] - xo).max()
        print(f"{m}x{n} k={k}: |dx|={ex / np.abs(xo).max():.2e}")
        assert ex <= 1e-10 * np.abs(xo).max()
        if m > n:  # the reference leaves Q'b below the triangle (src:284-294)
            qtb = bs[k].copy()
            for j in range(n):
                qtb[j:] -= Ho[j:, j] * (Ho[j:, j] @ qtb[j:])
            assert np.abs(B.rhs(k)[n:] - qtb[n:]).max() <= 1e-12 * max(1.0, np.abs(qtb).max())
    assert B.padding_intact()
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", [(66, 33), (70, 40), (130, 20)])
def test_one_cu_tier_is_the_single_call_bit_for_bit(emu, orc, m, n):
    """grid = batch of the single-workgroup kernels, barrier form: the bits of dhqr_factor_f64 / dhqr_solve_f64 of matrix k
    alone with the small route on ((130, 20): the single call runs the flag form)"""
    mats, bs = _inputs(orc, m, n, 3, 200)
    h = _ctx(emu)
    B = Batch(mats, bs)
    assert B.factor(emu, h, nb=128) == 0, emu.dhqr_last_error()
    assert B.solve(emu, h) == 0, emu.dhqr_last_error()
    assert emu.dhqr_synchronize(h) == 0
    assert B.padding_intact()
    for k in range(3):
        A = mats[k].copy(order="F")
        al = np.zeros(n)
        bb = bs[k].copy()
        assert emu.dhqr_factor_f64(h, _ptr(A), m, n, m, _ptr(al), 0) == 0
        assert emu.dhqr_solve_f64(h, _ptr(A), m, n, m, _ptr(al), _ptr(bb)) == 0
        assert emu.dhqr_synchronize(h) == 0
        assert np.array_equal(B.mat(k), A) and np.array_equal(B.alpha(k), al) and np.array_equal(B.rhs(k), bb)
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", [(16, 8), (66, 33)])
def test_a_batch_is_one_launch_group(emu, orc, m, n):
    """with profiling on, a batched factor is ONE reflector-apply group and a batched solve ONE solve group on both
    tiers -- the batch is not looped; with the small route off the serial tier answers what single calls answer"""
    mats, bs = _inputs(orc, m, n, 7, 300)
    h = _ctx(emu)
    assert emu.dhqr_set_profiling(h, 1) == 0 and emu.dhqr_reset_stats(h) == 0
    B = Batch(mats, bs)
    assert B.factor(emu, h) == 0
    st = _stats(emu, h)
    assert (st.n_rank1, st.n_panel, st.n_solve) == (1, 0, 0)
    assert B.solve(emu, h) == 0
    st = _stats(emu, h)
    assert (st.n_rank1, st.n_panel, st.n_solve) == (1, 0, 1)
    # the serial tier: two matrices, against two single calls
    assert emu.dhqr_set_small_route(h, 0) == 0
    B2 = Batch(mats[:2], bs[:2], pad_ld=0, pad=0)  # (the layout of the single calls below: the general drivers pick kernels by it)
    assert emu.dhqr_reset_stats(h) == 0
    assert B2.factor(emu, h, nb=0) == 0 and B2.solve(emu, h) == 0
    st = _stats(emu, h)
    batched = (st.n_rank1, st.n_panel, st.n_solve)
    assert emu.dhqr_reset_stats(h) == 0
    for k in range(2):
        A = mats[k].copy(order="F")
        al = np.zeros(n)
        bb = bs[k].copy()
        assert emu.dhqr_factor_f64(h, _ptr(A), m, n, m, _ptr(al), 0) == 0
        assert emu.dhqr_solve_f64(h, _ptr(A), m, n, m, _ptr(al), _ptr(bb)) == 0
        assert emu.dhqr_synchronize(h) == 0
        assert np.array_equal(B2.mat(k), A) and np.array_equal(B2.alpha(k), al) and np.array_equal(B2.rhs(k), bb)
    st = _stats(emu, h)
    assert batched == (st.n_rank1, st.n_panel, st.n_solve) and st.n_solve == 2
    emu.dhqr_destroy(h)


def test_shapes_beyond_the_small_route_are_looped(emu, orc):
    """(300, 225) fits no instantiation: two single-matrix factorisations with the caller's nb, same numbers, same counts"""
    m, n = 300, 225
    mats, bs = _inputs(orc, m, n, 2, 400)
    h = _ctx(emu)
    assert emu.dhqr_set_profiling(h, 1) == 0 and emu.dhqr_reset_stats(h) == 0
    B = Batch(mats, bs, pad_ld=2, pad=4)
    assert B.factor(emu, h, nb=128) == 0, emu.dhqr_last_error()
    st = _stats(emu, h)
    batched = (st.n_rank1, st.n_panel)
    assert st.n_rank1 == 0 and st.n_panel >= 4
    assert emu.dhqr_reset_stats(h) == 0
    for k in range(2):
        A = np.full((m + 2, n), SENT, order="F")
        A[:m] = mats[k]
        al = np.zeros(n)
        assert emu.dhqr_factor_f64(h, _ptr(A), m, n, m + 2, _ptr(al), 128) == 0
        assert np.array_equal(B.mat(k), A[:m]) and np.array_equal(B.alpha(k), al)
    st = _stats(emu, h)
    assert batched == (st.n_rank1, st.n_panel)
    assert B.padding_intact()
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", [(16, 8), (40, 17), (66, 33)])
def test_host_pair_equals_device_pair(emu, orc, m, n):
    mats, bs = _inputs(orc, m, n, 4, 500)
    h = _ctx(emu)
    D = Batch(mats, bs)
    assert D.factor(emu, h) == 0 and D.solve(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    for pad_ld, pad in ((3, 5), (0, 0), (2, 0)):  # looped copies | one block per matrix | one column pitch throughout
        Hb = Batch(mats, bs, pad_ld=pad_ld, pad=pad)
        assert emu.dhqr_qr_batched_f64(h, _ptr(Hb.A), m, n, Hb.lda, Hb.sA, _ptr(Hb.al), Hb.sal, 4, 0) == 0, emu.dhqr_last_error()
        b0 = Hb.b.copy()
        sx = n + 2
        x = np.full(4 * sx + 3, SENT)
        assert emu.dhqr_ldiv_batched_f64(h, _ptr(Hb.A), m, n, Hb.lda, Hb.sA, _ptr(Hb.al), Hb.sal, _ptr(Hb.b), Hb.sb, _ptr(x), sx, 4) == 0
        assert np.array_equal(Hb.b, b0), "hb must not be modified"
        for k in range(4):
            assert np.array_equal(Hb.mat(k), D.mat(k)) and np.array_equal(Hb.alpha(k), D.alpha(k))
            assert np.array_equal(x[k * sx: k * sx + n], D.rhs(k)[:n])
            assert np.all(x[k * sx + n: (k + 1) * sx] == SENT)
        assert Hb.padding_intact()
    assert emu.dhqr_trim(h) == 0  # releases the device copy of the batch; the next call allocates again
    Hb = Batch(mats, bs)
    assert emu.dhqr_qr_batched_f64(h, _ptr(Hb.A), m, n, Hb.lda, Hb.sA, _ptr(Hb.al), Hb.sal, 4, 0) == 0
    assert all(np.array_equal(Hb.mat(k), D.mat(k)) for k in range(4))
    emu.dhqr_destroy(h)


def test_argument_rules(emu, orc):
    EINVAL = -1
    m, n, batch = 12, 6, 3
    mats, bs = _inputs(orc, m, n, batch, 600)
    h = _ctx(emu)
    B = Batch(mats, bs)
    A, al, b = _ptr(B.A), _ptr(B.al), _ptr(B.b)
    x = np.zeros(batch * n)
    before = (B.A.copy(), B.al.copy(), B.b.copy())

    def all_four(m=m, n=n, lda=B.lda, sA=B.sA, sal=B.sal, sb=B.sb, sx=n, batch=batch, A=A, al=al, b=b, xp=_ptr(x)):
        return (emu.dhqr_factor_batched_f64(h, A, m, n, lda, sA, al, sal, batch, 0),
                emu.dhqr_qr_batched_f64(h, A, m, n, lda, sA, al, sal, batch, 0)) + solves(m, n, lda, sA, sal, sb, sx, batch, A, al, b, xp)

    def solves(m=m, n=n, lda=B.lda, sA=B.sA, sal=B.sal, sb=B.sb, sx=n, batch=batch, A=A, al=al, b=b, xp=_ptr(x)):
        return (emu.dhqr_solve_batched_f64(h, A, m, n, lda, sA, al, sal, b, sb, batch),
                emu.dhqr_ldiv_batched_f64(h, A, m, n, lda, sA, al, sal, b, sb, xp, sx, batch))

    assert all_four(batch=0) == (0, 0, 0, 0)
    assert all_four(n=0) == (0, 0, 0, 0)
    assert all_four(batch=0, A=None, al=None, b=None, xp=None) == (0, 0, 0, 0)
    assert all_four(batch=-1) == (EINVAL,) * 4
    assert all_four(m=5, n=6) == (EINVAL,) * 4                # m < n
    assert all_four(lda=m - 1) == (EINVAL,) * 4
    assert all_four(sA=B.lda * (n - 1) + m - 1) == (EINVAL,) * 4
    assert all_four(sal=n - 1) == (EINVAL,) * 4
    assert all_four(A=None) == (EINVAL,) * 4
    assert all_four(al=None) == (EINVAL,) * 4
    assert solves(sb=m - 1) == (EINVAL, EINVAL)
    assert solves(b=None) == (EINVAL, EINVAL)
    assert emu.dhqr_ldiv_batched_f64(h, A, m, n, B.lda, B.sA, al, B.sal, b, B.sb, _ptr(x), n - 1, batch) == EINVAL
    assert emu.dhqr_ldiv_batched_f64(h, A, m, n, B.lda, B.sA, al, B.sal, b, B.sb, None, n, batch) == EINVAL
    assert emu.dhqr_factor_batched_f64(h, A, m, n, B.lda, B.sA, al, B.sal, batch, 64) == EINVAL  # nb: 0 or 128
    for got, want in zip((B.A, B.al, B.b), before):
        assert np.array_equal(got, want), "a rejected or empty call must not touch anything"
    # the last column of the last matrix may be short of lda: strideA = lda*(n-1) + m is accepted
    sA = B.lda * (n - 1) + m
    T = np.full(batch * sA, SENT)
    for k in range(batch):
        for j in range(n):
            T[k * sA + j * B.lda: k * sA + j * B.lda + m] = mats[k][:, j]
    assert emu.dhqr_factor_batched_f64(h, _ptr(T), m, n, B.lda, sA, al, B.sal, batch, 0) == 0
    assert emu.dhqr_synchronize(h) == 0
    assert B.factor(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    for k in range(batch):
        for j in range(n):
            assert np.array_equal(T[k * sA + j * B.lda: k * sA + j * B.lda + m], B.mat(k)[:, j])
    emu.dhqr_destroy(h)


def test_zero_pivot_and_zero_column_inside_a_batch(emu, orc):
    """alphafactor(0) = -sign(0) = 0 (src:8): a zero pivot gives the oracle's factor; an all-zero column gives its alpha
    (-0.0, and like the reference NaN in the columns behind it) without disturbing the neighbours in the batch"""
    m, n = 12, 6
    mats, bs = _inputs(orc, m, n, 4, 700)
    mats[1][0, 0] = 0.0       # zero pivot, non-zero column
    mats[2][:, 2] = 0.0       # all-zero column
    h = _ctx(emu)
    B = Batch(mats, bs)
    assert B.factor(emu, h) == 0 and emu.dhqr_synchronize(h) == 0
    for k in range(4):
        Ho, ao = orc.householder(mats[k])
        if k == 2:
            assert ao[2] == 0.0 and np.isnan(ao[3:]).all()
            assert B.alpha(k)[2] == 0.0 and np.isnan(B.alpha(k)[3:]).all()
            assert np.allclose(B.alpha(k)[:2], ao[:2], rtol=0, atol=1e-12 * np.abs(ao[:2]).max())
            assert np.allclose(B.mat(k)[:, :2], Ho[:, :2], rtol=0, atol=1e-12)
        else:
            scale = np.abs(Ho).max()
            assert np.abs(B.mat(k) - Ho).max() <= 1e-12 * scale and np.abs(B.alpha(k) - ao).max() <= 1e-12 * scale
    assert B.padding_intact()
    emu.dhqr_destroy(h)
