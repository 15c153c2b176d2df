"""Child process of the staged-host-path tests (test_gpu_schedule.py, test_emulated_hostio.py).

    python schedule_child.py LIBRARY CASESET        CASESET: "gpu" or "emu"

DHQR_HOSTIO is read once per process, so the parent starts one child per setting and compares what they print: one JSON
line per case with a SHA-256 of every output of dhqr_qr_f64 / dhqr_ldiv_f64 (the factor also per 128-column block, so
that a difference names its columns), the panel counters, and whether the NaN guards around a padded host matrix
survived.  Plain Python + numpy + ctypes on the library's C ABI: no torch, nothing else opens the GPU."""
import ctypes
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from layout_helpers import assert_guards_intact, guarded_matrix  # noqa: E402
from oracle import dhqr_oracle as orc  # noqa: E402

P = ctypes.c_void_p
NB = 128

# name -> list of calls on ONE context; a call is (m, n, nb, lda - m, kind); kind "near": columns 199 / 200 nearly dependent
# (the matrix of test_fast_panel_path_is_used_and_falls_back), "guard": the matrix sits in a NaN-guarded buffer
CASES = {
    "gpu": [
        ("1100x1000_nb128", [(1100, 1000, 128, 0, "")]),
        ("2207x2000_nb128", [(2207, 2000, 128, 0, "")]),
        ("1100x1000_nb0", [(1100, 1000, 0, 0, "")]),
        ("300x200_simple_driver", [(300, 200, 128, 0, "")]),
        ("1031x777_odd_m", [(1031, 777, 128, 0, "")]),
        ("1100x1000_lda_m+3_guarded", [(1100, 1000, 128, 3, "guard")]),
        ("1500x640_rejected_panel", [(1500, 640, 128, 0, "near")]),
        ("2207x2000_then_1031x777", [(2207, 2000, 128, 0, ""), (1031, 777, 128, 0, "")]),
    ],
    # the emulator's sizes: the same paths (more than four 128-column chunks with a one-column last block, nb = 0, the
    # simple driver, odd m, a guarded lda = m + 3, a rejected panel, large then small on one context)
    "emu": [
        ("200x150_nb0", [(200, 150, 0, 0, "")]),
        ("300x200_simple_driver", [(300, 200, 128, 0, "")]),
        ("333x300_odd_m", [(333, 300, 128, 0, "")]),
        ("390x300_lda_m+3_guarded", [(390, 300, 128, 3, "guard")]),
        ("520x384_rejected_panel", [(520, 384, 128, 0, "near")]),
        ("660x641_then_333x260", [(660, 641, 128, 0, ""), (333, 260, 128, 0, "")]),
    ],
}


def load(so):
    spec = importlib.util.spec_from_file_location(
        "dhqr_lib_signatures", os.path.join(ROOT, "distributedhouseholderqr.jl_amd", "_lib.py"))
    sig = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sig)
    L = ctypes.CDLL(so)
    for name, (res, args) in sig.SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def one_call(L, h, m, n, nb, pad, kind, seed):
    A0 = orc.rand_matrix(m, n, seed)
    if kind == "near":
        A0[:, 200] = A0[:, 199] * (1.0 + 1e-9)
    b = orc.rand_vector(m, seed + 1)
    G = guarded_matrix(m, n, m + pad, 0, content=A0)
    al = np.zeros(n)
    f0, r0 = ctypes.c_int64(), ctypes.c_int64()
    assert L.dhqr_get_panel_counters(h, ctypes.byref(f0), ctypes.byref(r0)) == 0
    rc = L.dhqr_qr_f64(h, P(G.ptr), m, n, G.ld, P(al.ctypes.data), nb)
    assert rc == 0, f"dhqr_qr_f64: {rc} {L.dhqr_last_error()}"
    f1, r1 = ctypes.c_int64(), ctypes.c_int64()
    assert L.dhqr_get_panel_counters(h, ctypes.byref(f1), ctypes.byref(r1)) == 0
    guards = "intact"
    try:
        assert_guards_intact(G, "hA")
    except AssertionError as e:
        guards = str(e)
    hb, x = b.copy(), np.zeros(n)
    rc = L.dhqr_ldiv_f64(h, P(G.ptr), m, n, G.ld, P(al.ctypes.data), P(hb.ctypes.data), P(x.ctypes.data))
    assert rc == 0, f"dhqr_ldiv_f64: {rc} {L.dhqr_last_error()}"
    H = G.host()
    # keeps an answer that is wrong in BOTH settings from passing: ||A - QR|| / ||A|| of the factor (every case, also the
    # near-dependent columns) and x against a least-squares solution of the input (where that is well determined)
    xo = np.linalg.lstsq(A0, b, rcond=None)[0] if kind != "near" else None
    QR = orc.form_qr(np.asfortranarray(H), al)
    return {"m": m, "n": n, "nb": nb, "lda": G.ld, "kind": kind,
            "residual": float(np.linalg.norm(A0 - QR) / np.linalg.norm(A0)),
            "sha": {"hA": sha(H), "halpha": sha(al), "hx": sha(x), "hA_buffer": sha(G.bits())},
            "hA_blocks": [sha(H[:, c:c + NB]) for c in range(0, n, NB)],
            "hb_unchanged": bool(np.array_equal(hb, b)), "guards": guards,
            "n_fast": f1.value - f0.value, "n_fallback": r1.value - r0.value,
            "x_err": None if xo is None else float(np.abs(x - xo).max() / np.abs(xo).max())}


def main():
    so, which = sys.argv[1], sys.argv[2]
    L = load(so)
    for i, (name, calls) in enumerate(CASES[which]):
        h = P()
        assert L.dhqr_create(ctypes.byref(h), 0) == 0, L.dhqr_last_error()
        out = [one_call(L, h, *call, seed=50 + 2 * i) for call in calls]
        assert L.dhqr_destroy(h) == 0
        print(json.dumps({"case": name, "hostio": os.environ.get("DHQR_HOSTIO", ""), "calls": out}), flush=True)


if __name__ == "__main__":
    main()
