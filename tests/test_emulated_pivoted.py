"""Column-pivoted batched QR, the numerical rank and the rank-truncated least squares (dhqr_factor_batched_pivoted_f64,
dhqr_rank_batched_f64, dhqr_solve_batched_pivoted_f64, dhqr_qr_batched_pivoted_f64, dhqr_lstsq_batched_f64) through the C
ABI of the EMULATED library (csrc/ host-compiled against tests/simt/fake, fiber mode): the pivots against a numpy twin (and
scipy where it imports), the factor through the existing form_q / form_r, the bits of the wave tier against the unpivoted
entry points, the rank on products of given rank, exact zeros, the solve against numpy.linalg.lstsq by the reference's
statistic, the argument rules, the launch-group counts; the Python front end's type errors, which need no device.
The checks themselves are in pivoted_helpers.py, shared with test_gpu_pivoted.py."""
import ctypes
import os

import numpy as np
import pytest

import pivoted_helpers as PV
from nrhs_helpers import P


@pytest.fixture(scope="module")
def emu(emulated_so):
    from dist_helpers import load_emulated_library
    return load_emulated_library(emulated_so)


def _runner(L, small=1):
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
    return PV.Runner(L, h)


@pytest.fixture(scope="module")
def run(emu):
    R = _runner(emu)
    yield R
    emu.dhqr_destroy(R.h)


@pytest.fixture(scope="module")
def run_general(emu):
    """the small route off: every shape on the general tier"""
    R = _runner(emu, small=0)
    yield R
    emu.dhqr_destroy(R.h)


@pytest.fixture(scope="module")
def data(orc):
    """the inputs, computed once per shape and left unchanged"""
    cache = {}

    def get(m, n):
        if (m, n) not in cache:
            mats, Bs = PV.inputs(orc, m, n)
            for a in mats + Bs:
                a.setflags(write=False)
            cache[(m, n)] = (mats, Bs)
        return cache[(m, n)]
    return get


@pytest.mark.parametrize("m,n", PV.WAVE_SHAPES + PV.GENERAL_SHAPES)
def test_pivots_and_factor(run, data, m, n):
    PV.check_pivots_and_factor(run, *data(m, n))


def test_pivots_and_factor_small_route_off(run_general, data):
    PV.check_pivots_and_factor(run_general, *data(16, 8))


@pytest.mark.parametrize("m,n", [(16, 8), (64, 32), (130, 20)])
def test_pivots_against_scipy(run, data, m, n):
    scipy_linalg = pytest.importorskip("scipy.linalg")
    PV.check_pivots_and_factor(run, *data(m, n), scipy_qr=scipy_linalg.qr)


@pytest.mark.parametrize("m,n", PV.WAVE_SHAPES)
def test_wave_tier_bits(run, data, m, n):
    PV.check_wave_bits(run, *data(m, n))


@pytest.mark.parametrize("m,n,r0", PV.LOW_RANK)
def test_rank_and_solve_of_rank_deficient_matrices(run, m, n, r0):
    PV.check_solve(run, *PV.low_rank_inputs(m, n, r0), r0)


@pytest.mark.parametrize("m,n", PV.WAVE_SHAPES + PV.GENERAL_SHAPES)
def test_solve_full_rank(run, data, m, n):
    """rcond < 0 (the default bound max(m, n) eps) gives rank n on the full-rank inputs"""
    mats, Bs = data(m, n)
    D = PV.check_rank(run, mats, Bs, n, rcond=-1.0)
    assert D.ranks().tolist() == [n] * D.batch
    PV.check_solve(run, mats, Bs, n)


def test_solve_small_route_off(run_general, data):
    PV.check_solve(run_general, *data(16, 8), 8)
    PV.check_solve(run_general, *PV.low_rank_inputs(16, 8, 3), 3)


def test_degenerate(run, orc):
    PV.check_degenerate(run, orc)


def test_degenerate_general_tier(run_general, orc):
    PV.check_degenerate(run_general, orc)


def test_arguments(run, orc):
    PV.check_arguments(run, orc)


@pytest.mark.parametrize("m,n", [(16, 8), (66, 33)])
def test_profile_counts(emu, orc, m, n):
    R = _runner(emu)
    PV.check_profile_counts(R, orc, m, n)
    emu.dhqr_destroy(R.h)


def test_python_rejects_float32_and_complex():
    """the four Python functions are Float64 only: a TypeError before any device is touched"""
    import __graft_entry__ as g
    pkg = g.import_package()
    for dt in (np.float32, np.complex128):
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
    with pytest.raises(TypeError):
        pkg.lstsq_batched(np.ones((2, 5, 3)), np.ones((2, 5), dtype=np.float32))
    assert pkg.DistributedHouseholderQRStruct(np.ones((5, 3))).jpvt is None  # (additive: the old constructor)
    with pytest.raises(TypeError):
        pkg.rank_batched(pkg.DistributedHouseholderQRStruct(np.ones((2, 5, 3))))
