"""The early top of the panel chain (DHQR_TUNE early_top, csrc/dhqr_dist.h) on the CPU emulator: the whole library,
unmodified, host-compiled as in tests/test_emulated_library.py.

A pair's second panel takes its Gram matrix from a downdate (Gold - R'R, k_gram_downdate) of the early Gram of its block,
and its narrow update is split by rows: the top 256 rows in front of k_panel_top, the rest behind it.  Checked here:
the factorisation against the oracle, the downdate kernel alone, and that the split update subtracts every row tile
exactly once (early_top=2 = the split with the true Gram matrices must reproduce early_top=0 to the bit: a tile left out or
subtracted twice changes bits)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMT = os.path.join(ROOT, "tests", "simt")
CSRC = os.path.join(ROOT, "distributedhouseholderqr.jl_amd", "csrc")
EPS = np.finfo(np.float64).eps
P = ctypes.c_void_p

# the schedule tests' settings: pairs and quads at every size, stream-K from three column tiles on
ENV = {"DHQR_PAIR_MIN_N": "0", "DHQR_QUAD_MIN_COLS": "0"}
# 1280 x 1280: quad, quad, pair -- in-pair panels, pair-boundary panels, a last pair; 1408 x 1280 and 1152 x 640: row counts
# below the top rows that are no multiple of 256, a step that ends in a partial group
SHAPES = [(1280, 1280), (1408, 1280), (1152, 640)]
SEED = 5


@pytest.fixture(scope="module")
def emu(emulated_so):
    from dist_helpers import load_emulated_library
    return load_emulated_library(emulated_so)


def _factor(L, A0, early):
    env = dict(ENV, DHQR_TUNE=f"tn_min_tiles=3,early_top={early}")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h = P()
        assert L.dhqr_create(ctypes.byref(h), 0) == 0, L.dhqr_last_error()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    m, n = A0.shape
    A = A0.copy(order="F")
    al = np.zeros(n)
    rc = L.dhqr_factor_f64(h, A.ctypes.data_as(P), m, n, m, al.ctypes.data_as(P), 128)
    assert rc == 0, L.dhqr_last_error()
    fast, fb = ctypes.c_int64(), ctypes.c_int64()
    assert L.dhqr_get_panel_counters(h, ctypes.byref(fast), ctypes.byref(fb)) == 0
    assert L.dhqr_destroy(h) == 0
    return A, al, (fast.value, fb.value)


_RUNS = {}


def _run(L, orc, m, n, early):
    """one emulated factorisation per (shape, setting) for the whole file; never modified"""
    key = (m, n, early)
    if key not in _RUNS:
        _RUNS[key] = _factor(L, orc.rand_matrix(m, n, SEED), early)
    return _RUNS[key]


_ORACLE = {}


def _oracle(orc, m, n):
    if (m, n) not in _ORACLE:
        _ORACLE[(m, n)] = orc.householder(orc.rand_matrix(m, n, SEED))
    return _ORACLE[(m, n)]


def _residual(orc, A0, A, al):
    return np.linalg.norm(A0 - orc.form_qr(np.asfortranarray(A), al)) / np.linalg.norm(A0)


@pytest.mark.parametrize("m,n", SHAPES)
def test_early_top_against_the_oracle(emu, orc, m, n):
    """H and alpha at the project's 8 n eps (relative to max|H|); residual and panel counters as with early_top=0"""
    A0 = orc.rand_matrix(m, n, SEED)
    Ho, ao = _oracle(orc, m, n)
    scale = np.abs(Ho).max()
    tol = 8.0 * n * EPS
    A1, al1, cnt1 = _run(emu, orc, m, n, 1)
    A0_, al0, cnt0 = _run(emu, orc, m, n, 0)
    eH, ea = np.abs(A1 - Ho).max() / scale, np.abs(al1 - ao).max() / scale
    r1, r0 = _residual(orc, A0, A1, al1), _residual(orc, A0, A0_, al0)
    print(f"{m} x {n}: |dH| = {eH:.2e}, |dalpha| = {ea:.2e} (bound {tol:.2e}); residual {r1:.2e} (early_top=0: {r0:.2e}); "
          f"counters {cnt1} (early_top=0: {cnt0})")
    assert eH <= tol and ea <= tol
    assert np.abs(A0_ - Ho).max() / scale <= tol  # the switch is the old path: it passes the same bound
    # 1e-12: the bound on ||A - QR|| / ||A|| of the existing panel-path tests
    assert r1 < 1e-12 and r0 < 1e-12
    assert cnt1 == cnt0 and cnt1[1] == 0


@pytest.mark.parametrize("m,n", [(1408, 1280), (1152, 640)])
def test_split_update_subtracts_every_row_tile_exactly_once(emu, orc, m, n):
    """early_top=2 runs the two launches of the split narrow update (rows [0, 256) on the lane, the rest on the side stream)
    with the true Gram matrices, i.e. the arithmetic of early_top=0: the factorisation is the same to the BIT only if the two
    launches partition the row tiles of the one full-height k_gemm_nn_sub -- an overlap or a tile left out changes bits"""
    A2, al2, cnt2 = _run(emu, orc, m, n, 2)
    A0_, al0, cnt0 = _run(emu, orc, m, n, 0)
    assert A2.tobytes() == A0_.tobytes() and al2.tobytes() == al0.tobytes()
    assert cnt2 == cnt0
    # and the downdate path is a different computation: were it bit-identical too, the switch would not reach it
    A1, _, _ = _run(emu, orc, m, n, 1)
    assert A1.tobytes() != A0_.tobytes()


@pytest.fixture(scope="module")
def emu_downdate(tmp_path_factory):
    from dist_helpers import CLANG
    if not os.path.exists(CLANG):
        pytest.skip("host clang++ (ROCm llvm) not found")
    exe = str(tmp_path_factory.mktemp("emu_early_top") / "emu_early_top")
    subprocess.check_call([CLANG, "-std=c++20", "-O1", "-g", "-fsanitize=thread", "-Wno-unknown-attributes", "-Wno-psabi",
                           "-I", os.path.join(SIMT, "fake"), "-I", CSRC, os.path.join(SIMT, "emu_early_top.cpp"),
                           "-o", exe, "-lpthread"])
    return exe


@pytest.mark.parametrize("nrows", [384, 256, 128])
def test_gram_downdate_kernel(emu_downdate, tmp_path, nrows):
    """k_gram_downdate alone against float64 numpy Gold - R'R at 4 nrows eps max|Gold|; symmetric to the bit; R read with a
    leading dimension larger than nrows (it is a pointer into the matrix); a launch of a rejected run writes nothing"""
    rng = np.random.default_rng(100 + nrows)
    ldr = nrows + 24
    X = rng.standard_normal((ldr + 300, 128))
    Gold = X.T @ X  # the Gram matrix of a block whose first rows are R
    Rfull = np.asfortranarray(X[:ldr])  # rows >= nrows must not be read: they are part of Gold but not of R
    f = {k: str(tmp_path / k) for k in ("gold", "r", "g", "g2")}
    Gold.T.tofile(f["gold"])
    Rfull.T.tofile(f["r"])  # column-major
    r = subprocess.run([emu_downdate, "downdate", str(nrows), str(ldr), f["gold"], f["r"], f["g"]], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "ThreadSanitizer" not in r.stderr, r.stderr[-3000:]
    G = np.fromfile(f["g"]).reshape(128, 128).T
    want = Gold - X[:nrows].T @ X[:nrows]
    err, bound = np.abs(G - want).max(), 4.0 * nrows * EPS * np.abs(Gold).max()
    print(f"nrows = {nrows}: |G - (Gold - R'R)| = {err:.2e}, bound {bound:.2e}")
    assert err <= bound
    assert np.array_equal(G, G.T)
    r = subprocess.run([emu_downdate, "downdate_stopped", str(nrows), str(ldr), f["gold"], f["r"], f["g2"]], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert np.all(np.fromfile(f["g2"]) == -7.0)


def hard_matrix(orc):
    """1024 x 512 whose columns 128..255 are columns 0..127 times a fixed random matrix plus 1e-9 x noise: the second panel
    lies in the span of the first up to 1e-9, and its downdated Gram matrix is destroyed by cancellation"""
    A = orc.rand_matrix(1024, 512, 77)
    rng = np.random.default_rng(78)
    A[:, 128:256] = A[:, :128] @ rng.standard_normal((128, 128)) + 1e-9 * rng.standard_normal((1024, 128))
    return np.asfortranarray(A)


def test_hard_input_on_the_emulator(emu, orc):
    """the input of tests/test_gpu_early_top.py's hard case: the oracle and early_top=0 factor it backward stably, so a failure
    of early_top=1 points at the new path; with early_top=1 the bad Gram matrix ends in the device-side rejection and the
    panel is redone from a true Gram matrix"""
    A0 = hard_matrix(orc)
    Ho, ao = orc.householder(A0)
    assert _residual(orc, A0, Ho, ao) < 1e-12
    res = {}
    for early in (0, 1):
        A, al, (fast, fb) = _factor(emu, A0, early)
        res[early] = _residual(orc, A0, A, al)
        print(f"early_top={early}: residual {res[early]:.2e}, fast {fast}, fallback {fb}")
        assert res[early] < 1e-12
        assert fb <= 1 and fast + fb == 4
