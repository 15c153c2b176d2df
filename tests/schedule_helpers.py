"""Test-only helpers of the schedule tests: bitwise comparison with a message that names the first difference, and the
parent side of tests/helpers/schedule_child.py (staged host path, DHQR_HOSTIO=1, against the plain one).
The product never imports this file."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "helpers", "schedule_child.py")
NB = 128


def first_difference(a: dict, b: dict, dtypes: dict):
    """None if the two {name: bytes} sets are equal; else a message naming the first differing output, the element index
    and the two values (dtypes: name -> numpy dtype the bytes are shown as)"""
    if list(a) != list(b):
        return f"different outputs: {list(a)} against {list(b)}"
    for name in a:
        if a[name] == b[name]:
            continue
        if len(a[name]) != len(b[name]):
            return f"{name}: {len(a[name])} bytes against {len(b[name])}"
        dt = np.dtype(dtypes.get(name, np.float64))
        x, y = np.frombuffer(a[name], dtype=dt), np.frombuffer(b[name], dtype=dt)
        w = dt.itemsize // 8
        ne = (np.frombuffer(a[name], dtype=np.uint64).reshape(-1, w) != np.frombuffer(b[name], dtype=np.uint64).reshape(-1, w)).any(axis=1)
        i = int(np.flatnonzero(ne)[0])
        return f"{name}: {int(ne.sum())} of {x.size} elements differ, first at element {i}: {x[i]!r} against {y[i]!r}"
    return None


def run_hostio_child(so, caseset, hostio, timeout):
    """one child process with DHQR_HOSTIO = hostio; {case: record}.  A non-zero exit raises with the child's stderr tail."""
    env = dict(os.environ)
    env["DHQR_HOSTIO"] = hostio
    r = subprocess.run([sys.executable, CHILD, so, caseset], env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"child with DHQR_HOSTIO={hostio} exited with {r.returncode}:\n{r.stderr[-3000:]}"
    recs = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert all(rec["hostio"] == hostio for rec in recs)
    return {rec["case"]: rec for rec in recs}


def hostio_case_names(caseset):
    """the case names of one list of tests/helpers/schedule_child.py, for parametrised ids"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("schedule_child_cases", CHILD)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [name for name, _ in mod.CASES[caseset]]


def run_hostio_children(so, caseset, timeout):
    """(plain, staged): one child per setting, one after the other; a failed first child raises before the second starts"""
    plain = run_hostio_child(so, caseset, "0", timeout)
    staged = run_hostio_child(so, caseset, "1", timeout)
    assert list(plain) == list(staged) == hostio_case_names(caseset), (list(plain), list(staged))
    return plain, staged


def compare_hostio(plain: dict, staged: dict, x_tol: float, only=None):
    """the staged form factors the same device copy with the same dhqr_factor_f64: hA, halpha and hx bit-identical to the
    plain form's, hb unchanged, guards intact, and (so that an answer that is wrong in both forms does not pass) the
    factor's ||A - QR|| / ||A|| and x against a least-squares solution of the input within x_tol.  only: one case name"""
    assert list(plain) == list(staged) and plain, (list(plain), list(staged))
    fails = []
    for name, p in plain.items():
        if only is not None and name != only:
            continue
        s = staged[name]
        for k, (pc, sc) in enumerate(zip(p["calls"], s["calls"])):
            where = f"{name} call {k} ({pc['m']} x {pc['n']}, nb {pc['nb']}, lda {pc['lda']})"
            bad = [c for c, (u, v) in enumerate(zip(pc["hA_blocks"], sc["hA_blocks"])) if u != v]
            if bad:
                cols = ", ".join(f"[{c * NB}, {min((c + 1) * NB, pc['n'])})" for c in bad)
                fails.append(f"{where}: hA differs in columns {cols}")
            for out in ("hA", "halpha", "hx", "hA_buffer"):
                if pc["sha"][out] != sc["sha"][out] and not (out == "hA" and bad):
                    fails.append(f"{where}: {out} differs between the staged and the plain form")
            for rec, form in ((pc, "plain"), (sc, "staged")):
                if not rec["hb_unchanged"]:
                    fails.append(f"{where}: {form} form changed hb")
                if rec["guards"] != "intact":
                    fails.append(f"{where}: {form} form: {rec['guards']}")
                if rec["x_err"] is not None and not rec["x_err"] <= x_tol:
                    fails.append(f"{where}: {form} form: |dx| = {rec['x_err']:.2e} relative")
                # 1e-12: the bound on ||A - QR|| / ||A|| of test_fast_panel_path_is_used_and_falls_back (NaN fails it too)
                if not rec["residual"] < 1e-12:
                    fails.append(f"{where}: {form} form: ||A - QR|| / ||A|| = {rec['residual']:.2e}")
                if rec["kind"] == "near" and not rec["n_fallback"] >= 1:
                    fails.append(f"{where}: {form} form: no panel was rejected (n_fallback = {rec['n_fallback']})")
    assert not fails, "\n".join(fails)
