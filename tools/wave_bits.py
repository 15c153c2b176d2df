#!/usr/bin/env python3
"""Every output byte of the real-valued wave tier (m <= 64, n <= 32) on fixed inputs, for comparing two builds of the library.

  wave_bits.py run LIB OUT.npz [--cuda]   run the entry points below through the C ABI of LIB and save every output array
  wave_bits.py cmp A.npz B.npz            compare two such files byte for byte (exit status 1 on any difference)

LIB is a libdhqr.so (with --cuda: torch device tensors) or the emulated library of tests/dist_helpers.py (host arrays).
Entry points: dhqr_factor_batched_{f64,f32}, dhqr_solve_batched_{f64,f32}, dhqr_solve_batched_nrhs_{f64,f32},
dhqr_apply_q_batched_{f64,f32} (trans 0 and 1), dhqr_form_q_batched_{f64,f32}, dhqr_factor_batched_pivoted_f64 +
dhqr_rank_batched_f64 + dhqr_solve_batched_pivoted_f64.  Shapes: every instantiation and every edge -- (m, n) below, batch 5
(the last workgroup has waves without a matrix), nrhs 1, 4, 7, 8, 9 (full and tail groups of 4 and of 3; 1 takes the column
loop), one padded layout (lda > m, strides larger than the matrix), one batch with a zero column in matrix 2 (a NaN reflector
that must stay inside its matrix) and, for the pivoted calls, a matrix of rank n - 2."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 8), (13, 5), (16, 9), (33, 16), (40, 17), (64, 32)]
BATCH = 5
NRHS = [1, 4, 7, 8, 9]


def load(so):
    spec = importlib.util.spec_from_file_location("dhqr_lib_signatures", os.path.join(ROOT, "distributedhouseholderqr.jl_amd", "_lib.py"))
    sig = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sig)
    L = ctypes.CDLL(so)
    for name, (res, args) in sig.SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def run(so, out, cuda):
    L = load(so)
    dev = "cuda:0" if cuda else "cpu"
    h = ctypes.c_void_p()
    assert L.dhqr_create(ctypes.byref(h), 0) == 0
    res = {}

    def ok(rc):
        assert rc == 0, L.dhqr_last_error()

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def block(rng, k, rows, cols, ld, stride, dt):  # k blocks of rows x cols, column-major, padding filled with a marker
        a = np.full((k, stride), 7.0, dtype=dt)
        for i in range(k):
            a[i, : ld * cols].reshape(cols, ld)[:, :rows] = rng.standard_normal((cols, rows))
        return a

    for dt, sfx in ((np.float64, "f64"), (np.float32, "f32")):
        for (m, n) in SHAPES:
            for padded in (False, True):
                for special in ((None,) if padded else (None, "zerocol", "rankdef")):
                    if special == "rankdef" and sfx == "f32":
                        continue
                    lda = m + 3 if padded else m
                    sA = lda * n + 5 if padded else m * n
                    sal = n + 2 if padded else n
                    rng = np.random.default_rng(1000 * m + n)
                    A0 = block(rng, BATCH, m, n, lda, sA, dt)
                    if special == "zerocol":
                        A0[2, : lda * n].reshape(n, lda)[min(2, n - 1), :] = 0.0
                    if special == "rankdef" and n >= 3:
                        v = A0[1, : lda * n].reshape(n, lda)
                        v[n - 1, :m] = v[0, :m] + v[1, :m]
                        v[n - 2, :m] = 2.0 * v[0, :m] - v[1, :m]
                    key = f"{sfx}_{m}x{n}_{'pad' if padded else 'packed'}_{special}"
                    dA = torch.from_numpy(A0.copy()).to(dev)
                    dal = torch.full((BATCH, sal), 3.0, dtype=dA.dtype, device=dev)
                    if special != "rankdef":
                        ok(getattr(L, f"dhqr_factor_batched_{sfx}")(h, p(dA), m, n, lda, sA, p(dal), sal, BATCH, 0))
                        ok(L.dhqr_synchronize(h))
                        res[key + "_H"], res[key + "_alpha"] = dA.cpu().numpy(), dal.cpu().numpy()
                        sb = m + 4 if padded else m
                        b0 = block(rng, BATCH, m, 1, m, sb, dt)
                        db = torch.from_numpy(b0.copy()).to(dev)
                        ok(getattr(L, f"dhqr_solve_batched_{sfx}")(h, p(dA), m, n, lda, sA, p(dal), sal, p(db), sb, BATCH))
                        ok(L.dhqr_synchronize(h))
                        res[key + "_x"] = db.cpu().numpy()
                        for nrhs in NRHS:
                            ldb = m + 2 if padded else m
                            sB = ldb * nrhs + 3 if padded else m * nrhs
                            B0 = block(rng, BATCH, m, nrhs, ldb, sB, dt)
                            dB = torch.from_numpy(B0.copy()).to(dev)
                            ok(getattr(L, f"dhqr_solve_batched_nrhs_{sfx}")(h, p(dA), m, n, lda, sA, p(dal), sal, p(dB), nrhs, ldb, sB, BATCH))
                            ok(L.dhqr_synchronize(h))
                            res[f"{key}_X{nrhs}"] = dB.cpu().numpy()
                            for trans in (0, 1):
                                dB = torch.from_numpy(B0.copy()).to(dev)
                                ok(getattr(L, f"dhqr_apply_q_batched_{sfx}")(h, p(dA), m, n, lda, sA, p(dB), nrhs, ldb, sB, BATCH, trans))
                                ok(L.dhqr_synchronize(h))
                                res[f"{key}_Q{trans}B{nrhs}"] = dB.cpu().numpy()
                        ldq = m + 1 if padded else m
                        sQ = ldq * n + 2 if padded else m * n
                        dQ = torch.full((BATCH, sQ), 5.0, dtype=dA.dtype, device=dev)
                        ok(getattr(L, f"dhqr_form_q_batched_{sfx}")(h, p(dA), m, n, lda, sA, p(dQ), ldq, sQ, BATCH))
                        ok(L.dhqr_synchronize(h))
                        res[key + "_Q"] = dQ.cpu().numpy()
                    if sfx == "f64":
                        dA = torch.from_numpy(A0.copy()).to(dev)
                        sj = n + 1 if padded else n
                        djp = torch.full((BATCH, sj), -9, dtype=torch.int32, device=dev)
                        drk = torch.full((BATCH,), -9, dtype=torch.int32, device=dev)
                        ok(L.dhqr_factor_batched_pivoted_f64(h, p(dA), m, n, lda, sA, p(dal), sal, p(djp), sj, BATCH))
                        ok(L.dhqr_rank_batched_f64(h, p(dal), m, n, sal, -1.0, p(drk), BATCH))
                        ok(L.dhqr_synchronize(h))
                        res[key + "_pH"], res[key + "_palpha"] = dA.cpu().numpy(), dal.cpu().numpy()
                        res[key + "_jpvt"], res[key + "_rank"] = djp.cpu().numpy(), drk.cpu().numpy()
                        for nrhs in NRHS:
                            ldb = m + 2 if padded else m
                            sB = ldb * nrhs + 3 if padded else m * nrhs
                            ldx = n + 1 if padded else n
                            sX = ldx * nrhs + 2 if padded else n * nrhs
                            dB = torch.from_numpy(block(rng, BATCH, m, nrhs, ldb, sB, dt)).to(dev)
                            dX = torch.full((BATCH, sX), 5.0, dtype=dA.dtype, device=dev)
                            ok(L.dhqr_solve_batched_pivoted_f64(h, p(dA), m, n, lda, sA, p(dal), sal, p(djp), sj, p(drk), p(dB), nrhs, ldb, sB,
                                                                p(dX), ldx, sX, BATCH))
                            ok(L.dhqr_synchronize(h))
                            res[f"{key}_pB{nrhs}"], res[f"{key}_pX{nrhs}"] = dB.cpu().numpy(), dX.cpu().numpy()
    assert L.dhqr_destroy(h) == 0
    np.savez(out, **res)
    print(f"{len(res)} arrays, {sum(v.nbytes for v in res.values())} bytes -> {out}")


def cmp(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "different sets of arrays"
    bad = [k for k in A.files if A[k].tobytes() != B[k].tobytes()]
    nbytes = sum(A[k].nbytes for k in A.files)
    print(f"{len(A.files)} arrays, {nbytes} bytes: {'IDENTICAL' if not bad else 'DIFFERENT in ' + ', '.join(bad[:20])}")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], "--cuda" in sys.argv)
    else:
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
