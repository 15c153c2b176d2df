"""Float32 entry points (dhqr_factor_f32 / dhqr_solve_f32 / dhqr_qr_f32 / dhqr_ldiv_f32 and their batched forms) through the
C ABI of the EMULATED library (csrc/ host-compiled against tests/simt/fake, fiber mode): the native wave-per-matrix kernels
of csrc/dhqr_f32.h against the Float64 oracle and against LAPACK in Float32, the promoted tier bit for bit against
float32(f64_entry_point(float64(input))), batched against single, guarded layouts, the host forms, the argument rules."""
import ctypes

import numpy as np
import pytest

import f32_helpers as F
from test_emulated_batched import _ctx, _stats

P = ctypes.c_void_p


def _ptr(a):
    return a.ctypes.data_as(P) if a is not None else None


@pytest.fixture(scope="module")
def emu(emulated_so):
    from dist_helpers import load_emulated_library
    return load_emulated_library(emulated_so)


def _packed(A):
    """(batch, m, n) -> flat buffer with matrix k column-major at k m n"""
    return np.ascontiguousarray(A.transpose(0, 2, 1)).reshape(-1)


def _unpacked(flat, batch, m, n):
    return flat.reshape(batch, n, m).transpose(0, 2, 1)


def _factor_batched(L, h, A, nb=0, dtype=np.float32):
    batch, m, n = A.shape
    fa = _packed(A).astype(dtype)
    al = np.zeros(batch * n, dtype=dtype)
    fn = L.dhqr_factor_batched_f32 if dtype == np.float32 else L.dhqr_factor_batched_f64
    assert fn(h, _ptr(fa), m, n, m, m * n, _ptr(al), n, batch, nb) == 0, L.dhqr_last_error()
    assert L.dhqr_synchronize(h) == 0
    return _unpacked(fa, batch, m, n), al.reshape(batch, n)


def _solve_batched(L, h, H, al, b, dtype=np.float32):
    batch, m, n = H.shape
    fa, fal, fb = _packed(H).astype(dtype), np.ascontiguousarray(al, dtype=dtype), np.array(b, dtype=dtype, order="C")
    fn = L.dhqr_solve_batched_f32 if dtype == np.float32 else L.dhqr_solve_batched_f64
    assert fn(h, _ptr(fa), m, n, m, m * n, _ptr(fal), n, _ptr(fb), m, batch) == 0, L.dhqr_last_error()
    assert L.dhqr_synchronize(h) == 0
    return fb  # (batch, m): [x_k; tail of Q'b_k]


@pytest.mark.parametrize("i,m,n", [(i, m, n) for i, (m, n) in enumerate(F.NATIVE_SHAPES)])
def test_native_tier(emu, orc, i, m, n):
    """criteria 1-3 and 5 of the native tier on batches of 5 .. 9 matrices: one launch group per call"""
    batch = 5 + i % 5
    A, b = F.inputs(orc, m, n, batch, 100)
    h = _ctx(emu)
    assert emu.dhqr_set_profiling(h, 1) == 0 and emu.dhqr_reset_stats(h) == 0
    H, al = _factor_batched(emu, h, A)
    st = _stats(emu, h)
    assert (st.n_rank1, st.n_panel, st.n_solve) == (1, 0, 0)
    y = _solve_batched(emu, h, H, al, b)
    st = _stats(emu, h)
    assert (st.n_rank1, st.n_panel, st.n_solve) == (1, 0, 1)
    ks = range(batch)
    F.check_factor(orc, A, H, al, ks, "emulated native")
    F.check_solve(orc, H, al, b, y[:, :n], ks, "emulated native")
    if (m, n) in F.OVERDETERMINED:
        F.check_vs_lapack(orc, A, b, y[:, :n], ks, "emulated native")
    for k in range(batch):  # the twin is the kernel's arithmetic up to the order of the double sums
        Ht, at = F.twin_factor(A[k])
        assert np.abs(Ht.astype(np.float64) - H[k]).max() <= F.tol_factor(n)
    # criterion 5: matrix k of the batch has the bytes of the single call on matrix k
    for k in (0, batch - 1):
        a1 = np.array(A[k], order="F")
        al1 = np.zeros(n, dtype=np.float32)
        b1 = b[k].copy()
        assert emu.dhqr_factor_f32(h, _ptr(a1), m, n, m, _ptr(al1), 0) == 0
        assert emu.dhqr_solve_f32(h, _ptr(a1), m, n, m, _ptr(al1), _ptr(b1)) == 0
        assert emu.dhqr_synchronize(h) == 0
        assert a1.tobytes() == np.asfortranarray(H[k]).tobytes() and al1.tobytes() == al[k].tobytes() and b1.tobytes() == y[k].tobytes()
    emu.dhqr_destroy(h)


def _promoted_case(emu, orc, m, n, batch, small, nb, seed):
    """criterion 4 on one context: the Float32 entry points' bytes equal float32(Float64 entry point on float64(input))"""
    A, b = F.inputs(orc, m, n, batch, seed)
    h = _ctx(emu, small=small)
    H32, al32 = _factor_batched(emu, h, A, nb)
    H64, al64 = _factor_batched(emu, h, A, nb, np.float64)
    assert H32.tobytes() == H64.astype(np.float32).tobytes() and al32.tobytes() == al64.astype(np.float32).tobytes()
    y32 = _solve_batched(emu, h, H32, al32, b)
    y64 = _solve_batched(emu, h, H32, al32, b, np.float64)
    assert y32.tobytes() == y64.astype(np.float32).tobytes()
    # the single-matrix entry points, matrix 0
    a1, al1, b1 = np.array(A[0], order="F"), np.zeros(n, dtype=np.float32), b[0].copy()
    a2, al2 = a1.astype(np.float64), np.zeros(n)
    assert emu.dhqr_factor_f32(h, _ptr(a1), m, n, m, _ptr(al1), nb) == 0 and emu.dhqr_synchronize(h) == 0
    assert emu.dhqr_factor_f64(h, _ptr(a2), m, n, m, _ptr(al2), nb) == 0 and emu.dhqr_synchronize(h) == 0
    assert a1.tobytes() == a2.astype(np.float32).tobytes() and al1.tobytes() == al2.astype(np.float32).tobytes()
    a2, al2, b2 = a1.astype(np.float64), al1.astype(np.float64), b1.astype(np.float64)
    assert emu.dhqr_solve_f32(h, _ptr(a1), m, n, m, _ptr(al1), _ptr(b1)) == 0 and emu.dhqr_synchronize(h) == 0
    assert emu.dhqr_solve_f64(h, _ptr(a2), m, n, m, _ptr(al2), _ptr(b2)) == 0 and emu.dhqr_synchronize(h) == 0
    assert b1.tobytes() == b2.astype(np.float32).tobytes()
    assert emu.dhqr_trim(h) == 0  # releases the workspace; the next call allocates again
    H32b, _ = _factor_batched(emu, h, A, nb)
    assert H32b.tobytes() == H32.tobytes()
    emu.dhqr_destroy(h)
    return A, b, H32, al32, y32


@pytest.mark.parametrize("m,n", [(66, 33), (130, 20)])
def test_promoted_tier_bit_for_bit(emu, orc, m, n):
    """beyond 64 x 32: the Float64 small route (one-workgroup tier for the batch) under the two element-wise passes; the
    result also meets the native tier's bound against the oracle"""
    A, b, H, al, y = _promoted_case(emu, orc, m, n, 3, 1, 0, 200)
    F.check_factor(orc, A, H, al, range(3), "emulated promoted")
    F.check_solve(orc, H, al, b, y[:, :n], range(3), "emulated promoted")


@pytest.mark.parametrize("m,n", [(5, 3), (40, 17), (32, 32)])
def test_native_shapes_are_promoted_with_the_small_route_off(emu, orc, m, n):
    _promoted_case(emu, orc, m, n, 2, 0, 0, 300)


@pytest.mark.parametrize("m,n,small", [(33, 9, 1), (64, 32, 1), (66, 33, 1)])
def test_guarded_layouts(emu, orc, m, n, small):
    """criterion 6: lda = m + 1, m + 3 and a base 4 bytes off an 8-byte boundary; matrix, alpha, b and x in float32
    NaN-guarded buffers; criterion 1, then every guard word bit for bit.  Device-resident and host forms."""
    A, b = F.inputs(orc, m, n, 1, 400)
    h = _ctx(emu, small=small)
    for pad, off in ((1, 0), (3, 0), (0, 1), (3, 1)):
        for host in (False, True):
            gA = F.guarded_f32(m, n, m + pad, off, content=A[0])
            gal = F.guarded_f32(n, 1, n, off, content=np.zeros(n, dtype=np.float32))
            gb = F.guarded_f32(m, 1, m, off, content=b[0])
            gx = F.guarded_f32(n, 1, n, off, content=np.zeros(n, dtype=np.float32))
            if host:
                assert emu.dhqr_qr_f32(h, P(gA.ptr), m, n, m + pad, P(gal.ptr), 0) == 0, emu.dhqr_last_error()
                assert emu.dhqr_ldiv_f32(h, P(gA.ptr), m, n, m + pad, P(gal.ptr), P(gb.ptr), P(gx.ptr)) == 0
                x = gx.view.copy()
                assert gb.view.tobytes() == b[0].tobytes(), "hb must not be modified"
            else:
                assert emu.dhqr_factor_f32(h, P(gA.ptr), m, n, m + pad, P(gal.ptr), 0) == 0, emu.dhqr_last_error()
                assert emu.dhqr_solve_f32(h, P(gA.ptr), m, n, m + pad, P(gal.ptr), P(gb.ptr)) == 0
                assert emu.dhqr_synchronize(h) == 0
                x = gb.view[:n].copy()
            H, al = np.array(gA.view)[None], gal.view.copy()[None]
            F.check_factor(orc, A, H, al, [0], f"emulated layout lda=m+{pad} off={off} host={host}")
            F.check_solve(orc, H, al, b, x[None], [0], f"emulated layout lda=m+{pad} off={off} host={host}")
            for g, name in ((gA, "A"), (gal, "alpha"), (gb, "b"), (gx, "x")):
                F.assert_f32_guards_intact(g, name)
    emu.dhqr_destroy(h)


@pytest.mark.parametrize("m,n", [(16, 8), (40, 17), (66, 33)])
def test_host_pair_equals_device_pair(emu, orc, m, n):
    batch = 4
    A, b = F.inputs(orc, m, n, batch, 500)
    h = _ctx(emu)
    H, al = _factor_batched(emu, h, A)
    y = _solve_batched(emu, h, H, al, b)
    for pad_ld, pad in ((3, 5), (0, 0), (2, 0)):  # looped copies | one block per matrix | one column pitch throughout
        lda, sA, sal, sb, sx = m + pad_ld, (m + pad_ld) * n + pad, n + pad, m + pad, n + 2
        fa = np.full(batch * sA + 7, -7.25, dtype=np.float32)
        fal = np.full(batch * sal + 7, -7.25, dtype=np.float32)
        fb = np.full(batch * sb + 7, -7.25, dtype=np.float32)
        fx = np.full(batch * sx + 3, -7.25, dtype=np.float32)
        mats = [fa[k * sA: k * sA + lda * n].reshape((lda, n), order="F")[:m] for k in range(batch)]
        for k in range(batch):
            mats[k][...] = A[k]
            fb[k * sb: k * sb + m] = b[k]
        b0 = fb.copy()
        assert emu.dhqr_qr_batched_f32(h, _ptr(fa), m, n, lda, sA, _ptr(fal), sal, batch, 0) == 0, emu.dhqr_last_error()
        assert emu.dhqr_ldiv_batched_f32(h, _ptr(fa), m, n, lda, sA, _ptr(fal), sal, _ptr(fb), sb, _ptr(fx), sx, batch) == 0
        assert np.array_equal(fb, b0), "hb must not be modified"
        for k in range(batch):
            assert np.array_equal(mats[k], H[k]) and np.array_equal(fal[k * sal: k * sal + n], al[k])
            assert np.array_equal(fx[k * sx: k * sx + n], y[k, :n]) and np.all(fx[k * sx + n: (k + 1) * sx] == -7.25)
            assert np.all(fa[k * sA + lda * n: (k + 1) * sA] == -7.25) and np.all(fal[k * sal + n: (k + 1) * sal] == -7.25)
            if pad_ld:
                assert np.all(fa[k * sA: k * sA + lda * n].reshape((lda, n), order="F")[m:] == -7.25)
    emu.dhqr_destroy(h)


def test_argument_rules(emu, orc):
    """every DHQR_EINVAL case and no-op of the Float64 batched family (test_emulated_batched.py), and of the single calls"""
    EINVAL = -1
    m, n, batch = 12, 6, 3
    A32, b32 = F.inputs(orc, m, n, batch, 600)
    h = _ctx(emu)
    lda, sA, sal, sb = m + 3, (m + 3) * n + 5, n + 5, m + 5
    fa = np.zeros(batch * sA, dtype=np.float32)
    for k in range(batch):
        fa[k * sA: k * sA + lda * n].reshape((lda, n), order="F")[:m] = A32[k]
    fal, fb, x = np.zeros(batch * sal, dtype=np.float32), np.zeros(batch * sb, dtype=np.float32), np.zeros(batch * n, dtype=np.float32)
    before = (fa.copy(), fal.copy(), fb.copy())
    A, al, b = _ptr(fa), _ptr(fal), _ptr(fb)

    def all_four(m=m, n=n, lda=lda, sA=sA, sal=sal, sb=sb, sx=n, batch=batch, A=A, al=al, b=b, xp=_ptr(x)):
        return (emu.dhqr_factor_batched_f32(h, A, m, n, lda, sA, al, sal, batch, 0),
                emu.dhqr_qr_batched_f32(h, A, m, n, lda, sA, al, sal, batch, 0)) + solves(m, n, lda, sA, sal, sb, sx, batch, A, al, b, xp)

    def solves(m=m, n=n, lda=lda, sA=sA, sal=sal, sb=sb, sx=n, batch=batch, A=A, al=al, b=b, xp=_ptr(x)):
        return (emu.dhqr_solve_batched_f32(h, A, m, n, lda, sA, al, sal, b, sb, batch),
                emu.dhqr_ldiv_batched_f32(h, A, m, n, lda, sA, al, sal, b, sb, xp, sx, batch))

    def singles(m=m, n=n, lda=lda, A=A, al=al, b=b, xp=_ptr(x), nb=0, which=(0, 1, 2, 3)):
        calls = (lambda: emu.dhqr_factor_f32(h, A, m, n, lda, al, nb), lambda: emu.dhqr_qr_f32(h, A, m, n, lda, al, nb),
                 lambda: emu.dhqr_solve_f32(h, A, m, n, lda, al, b), lambda: emu.dhqr_ldiv_f32(h, A, m, n, lda, al, b, xp))
        return tuple(calls[i]() for i in which)

    assert all_four(batch=0) == (0, 0, 0, 0)
    assert all_four(n=0) == (0, 0, 0, 0)
    assert all_four(batch=0, A=None, al=None, b=None, xp=None) == (0, 0, 0, 0)
    assert all_four(batch=-1) == (EINVAL,) * 4
    assert all_four(m=5, n=6) == (EINVAL,) * 4                # m < n
    assert all_four(lda=m - 1) == (EINVAL,) * 4
    assert all_four(sA=lda * (n - 1) + m - 1) == (EINVAL,) * 4
    assert all_four(sal=n - 1) == (EINVAL,) * 4
    assert all_four(A=None) == (EINVAL,) * 4
    assert all_four(al=None) == (EINVAL,) * 4
    assert solves(sb=m - 1) == (EINVAL, EINVAL)
    assert solves(b=None) == (EINVAL, EINVAL)
    assert emu.dhqr_ldiv_batched_f32(h, A, m, n, lda, sA, al, sal, b, sb, _ptr(x), n - 1, batch) == EINVAL
    assert emu.dhqr_ldiv_batched_f32(h, A, m, n, lda, sA, al, sal, b, sb, None, n, batch) == EINVAL
    assert emu.dhqr_factor_batched_f32(h, A, m, n, lda, sA, al, sal, batch, 64) == EINVAL  # nb: 0 or 128
    assert emu.dhqr_qr_batched_f32(h, A, m, n, lda, sA, al, sal, batch, 64) == EINVAL
    assert singles(n=0) == (0, 0, 0, 0)
    assert singles(m=5, n=6) == (EINVAL,) * 4
    assert singles(m=-1) == (EINVAL,) * 4
    assert singles(lda=m - 1) == (EINVAL,) * 4
    assert singles(A=None) == (EINVAL,) * 4
    assert singles(al=None) == (EINVAL,) * 4
    assert singles(b=None, which=(2, 3)) == (EINVAL, EINVAL)
    assert singles(xp=None, which=(3,)) == (EINVAL,)
    assert singles(nb=64, which=(0, 1)) == (EINVAL, EINVAL)
    for got, want in zip((fa, fal, fb), before):
        assert np.array_equal(got, want), "a rejected or empty call must not touch anything"
    # the last column of the last matrix may be short of lda: strideA = lda*(n-1) + m is accepted
    s2 = lda * (n - 1) + m
    T = np.zeros(batch * s2, dtype=np.float32)
    for k in range(batch):
        for j in range(n):
            T[k * s2 + j * lda: k * s2 + j * lda + m] = A32[k][:, j]
    assert emu.dhqr_factor_batched_f32(h, _ptr(T), m, n, lda, s2, al, sal, batch, 0) == 0
    assert emu.dhqr_synchronize(h) == 0
    H, _ = _factor_batched(emu, h, A32)
    for k in range(batch):
        for j in range(n):
            assert np.array_equal(T[k * s2 + j * lda: k * s2 + j * lda + m], H[k][:, j])
    emu.dhqr_destroy(h)


def test_zero_pivot_zero_column_and_overflow(emu, orc):
    """sign(0) = 0 (src:8): a zero pivot gives the oracle's factor; an all-zero column gives alpha = 0 and, like the reference,
    NaN behind it, without disturbing its neighbours; a promoted result beyond Float32's range rounds to inf"""
    m, n = 12, 6
    A, b = F.inputs(orc, m, n, 4, 700)
    A[1][0, 0] = 0.0
    A[2][:, 2] = 0.0
    h = _ctx(emu)
    H, al = _factor_batched(emu, h, A)
    F.check_factor(orc, A, H, al, [0, 3], "emulated zero pivot: the neighbours")
    eH, ea, ev = F.factor_errors(orc, A[1], H[1], al[1])  # (v_0 of a zero pivot has norm 1, in the reference as here)
    assert eH <= F.tol_factor(n) and ea <= F.tol_factor(n) and al[1][0] == 0.0
    assert al[2][2] == 0.0 and np.isnan(al[2][3:]).all()
    Ho, ao = orc.householder(A[2].astype(np.float64))
    assert np.abs(H[2][:, :2] - Ho[:, :2]).max() <= F.tol_factor(n)
    big = np.full((1, 66, 33), 0.0, dtype=np.float32)
    big[0] = A[0][:1, :1] * 0 + (orc.rand_matrix(66, 33, 9) * 3e38).astype(np.float32)
    Hb, alb = _factor_batched(emu, h, big)  # |alpha_0| = ||a_0|| ~ 1.4e39
    assert np.isinf(alb[0][0]) and np.isfinite(Hb[0][:, 0]).all()
    emu.dhqr_destroy(h)
