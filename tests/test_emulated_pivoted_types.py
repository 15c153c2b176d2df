"""Column-pivoted batched QR, the numerical rank and the rank-truncated least squares for Float32 and ComplexF64
(dhqr_factor_batched_pivoted_*, dhqr_rank_batched_*, dhqr_solve_batched_pivoted_*, dhqr_qr_batched_pivoted_*,
dhqr_lstsq_batched_* with * = f32, c64) through the C ABI of the EMULATED library (csrc/ host-compiled against tests/simt/fake,
fiber mode): the pivots against a numpy twin per type (ComplexF64: and scipy where it imports), the factor through the
existing form_q / form_r, the bits of the wave tier against the type's unpivoted entry points, the rank on products of given
rank, exact zeros, the solve against numpy.linalg.lstsq by the reference's statistic, the argument rules, the launch-group
counts; the Python front end's type errors, which need no device.
The checks themselves are in pivoted_types_helpers.py, shared with test_gpu_pivoted_types.py.  The wave shapes, ONE general
shape and THREE low-rank sets per type: the emulated library runs a thread per lane."""
import ctypes
import os

import numpy as np
import pytest

import pivoted_types_helpers as PT
from nrhs_helpers import P

GENERAL_SHAPE = (66, 33)
LOW_RANK = [(16, 8, 3), (40, 17, 9), (66, 33, 10)]  # NC = 8, NC = 32 barely entered, the general tier


@pytest.fixture(scope="module")
def emu(emulated_so):
    from dist_helpers import load_emulated_library
    return load_emulated_library(emulated_so)


def _handle(L, small=1):
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


@pytest.fixture(scope="module")
def run(emu):
    h = _handle(emu)
    yield lambda t: PT.Runner(emu, h, t)
    emu.dhqr_destroy(h)


@pytest.fixture(scope="module")
def run_general(emu):
    """the small route off: every shape on the general tier (Float32: promoted)"""
    h = _handle(emu, small=0)
    yield lambda t: PT.Runner(emu, h, t)
    emu.dhqr_destroy(h)


@pytest.fixture(scope="module")
def data(orc):
    """the inputs, computed once per type and shape and left unchanged"""
    cache = {}

    def get(t, m, n):
        if (t, m, n) not in cache:
            mats, Bs = PT.inputs(orc, t, m, n)
            for a in mats + Bs:
                a.setflags(write=False)
            cache[(t, m, n)] = (mats, Bs)
        return cache[(t, m, n)]
    return get


def _scipy_qr():
    try:
        import scipy.linalg
        return scipy.linalg.qr
    except ImportError:
        return None


@pytest.mark.parametrize("t", PT.TYPES)
@pytest.mark.parametrize("m,n", PT.WAVE_SHAPES + [GENERAL_SHAPE])
def test_pivots_and_factor(run, data, t, m, n):
    PT.check_pivots_and_factor(run(t), *data(t, m, n), scipy_qr=_scipy_qr())


@pytest.mark.parametrize("t", PT.TYPES)
def test_pivots_and_factor_small_route_off(run_general, data, t):
    PT.check_pivots_and_factor(run_general(t), *data(t, 16, 8))


@pytest.mark.parametrize("t", PT.TYPES)
@pytest.mark.parametrize("m,n", PT.WAVE_SHAPES)
def test_wave_tier_bits(run, data, t, m, n):
    PT.check_wave_bits(run(t), *data(t, m, n))


@pytest.mark.parametrize("t", PT.TYPES)
@pytest.mark.parametrize("m,n,r0", LOW_RANK)
def test_rank_and_solve_of_rank_deficient_matrices(run, t, m, n, r0):
    PT.check_solve(run(t), *PT.low_rank_inputs(t, m, n, r0), r0)


@pytest.mark.parametrize("t", PT.TYPES)
@pytest.mark.parametrize("m,n", PT.WAVE_SHAPES + [GENERAL_SHAPE])
def test_solve_full_rank(run, data, t, m, n):
    """rcond < 0 (the default bound max(m, n) eps of the type) gives rank n on the full-rank inputs"""
    PT.check_full_rank(run(t), *data(t, m, n))


@pytest.mark.parametrize("t", PT.TYPES)
def test_solve_small_route_off(run_general, data, t):
    PT.check_solve(run_general(t), *data(t, 16, 8), 8)
    PT.check_solve(run_general(t), *PT.low_rank_inputs(t, 16, 8, 3), 3)


@pytest.mark.parametrize("t", PT.TYPES)
def test_degenerate(run, orc, t):
    PT.check_degenerate(run(t), orc)


@pytest.mark.parametrize("t", PT.TYPES)
def test_degenerate_general_tier(run_general, orc, t):
    PT.check_degenerate(run_general(t), orc)


@pytest.mark.parametrize("t", PT.TYPES)
def test_arguments(run, orc, t):
    PT.check_arguments(run(t), orc)


@pytest.mark.parametrize("t", PT.TYPES)
@pytest.mark.parametrize("m,n", [(16, 8), (66, 33)])
def test_profile_counts(emu, orc, t, m, n):
    h = _handle(emu)
    PT.check_profile_counts(PT.Runner(emu, h, t), orc, m, n)
    emu.dhqr_destroy(h)


def test_python_type_errors():
    """the four typed functions reject a B of another dtype than the factor's before any device is touched; the four
    Float64-only functions still reject float32 and complex128"""
    import __graft_entry__ as g
    pkg = g.import_package()
    for dt, other in ((np.float32, np.float64), (np.complex128, np.float64), (np.float64, np.float32), (np.float64, np.complex128)):
        A, B = np.ones((2, 5, 3), dtype=dt), np.ones((2, 5), dtype=other)
        with pytest.raises(TypeError):
            pkg.lstsq_pivoted_batched(A, B)
        H = pkg.DistributedHouseholderQRStruct(A, np.zeros((2, 3), dtype=dt), jpvt=np.zeros((2, 3), dtype=np.int32))
        with pytest.raises(TypeError):
            pkg.solve_pivoted_batched(H, B)
        with pytest.raises(TypeError):
            pkg.solve_pivoted_batched(H, np.ones((2, 5, 2), dtype=other))
        with pytest.raises(TypeError):
            pkg.rank_pivoted_batched(pkg.DistributedHouseholderQRStruct(A, np.zeros((2, 3), dtype=other),
                                                                        jpvt=np.zeros((2, 3), dtype=np.int32)))
    with pytest.raises(TypeError):
        pkg.factor_pivoted_batched_(np.ones((2, 5, 3), dtype=np.int32))
    with pytest.raises(TypeError):
        pkg.rank_pivoted_batched(pkg.DistributedHouseholderQRStruct(np.ones((2, 5, 3), dtype=np.float32)))  # (no jpvt)
    for dt in (np.float32, np.complex128):  # the old four, exactly as they were
        A, B = np.ones((2, 5, 3), dtype=dt), np.ones((2, 5), dtype=dt)
        with pytest.raises(TypeError):
            pkg.qr_pivoted_batched_(A)
        with pytest.raises(TypeError):
            pkg.lstsq_batched(A, B)
        H = pkg.DistributedHouseholderQRStruct(A, np.zeros((2, 3), dtype=dt), jpvt=np.zeros((2, 3), dtype=np.int32))
        with pytest.raises(TypeError):
            pkg.rank_batched(H)
        with pytest.raises(TypeError):
            pkg.ldiv_pivoted_batched(H, B)
