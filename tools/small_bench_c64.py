"""ComplexF64 qr!(A) \\ b on HOST arrays at the reference's test shapes (test/runtests.jl:42-43,87-89) beside LAPACK on the host
cores (zgeqrf + zunmqr('L','C') + ztrtrs, 16 threads): microseconds per call (best of N), the ratio the reference prints, and
the two calls separately.  The ComplexF64 twin of small_bench.py.
usage: small_bench_c64.py [reps]   (DHQR_SMALL=0: the general drivers, i.e. the routes every shape took before the one-workgroup
tier of csrc/dhqr_small_complex.h)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.import_package()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
from scipy.linalg import lapack  # noqa: E402
from threadpoolctl import threadpool_limits  # noqa: E402

for m, n in ((110, 100), (220, 200), (440, 400), (880, 800), (1100, 1000)):
    A0 = np.asfortranarray(pkg.rand_colmajor_c(m, n, 0, "cuda:0").cpu().numpy())
    b0 = pkg.rand_colmajor_batched_c(1, m, 1, 1, "cuda:0").reshape(m).cpu().numpy()
    tq, tl, tt = [], [], []
    for _ in range(reps):
        A = A0.copy(order="F")
        t0 = time.perf_counter()
        H = pkg.qr_(A)
        t1 = time.perf_counter()
        x = np.asarray(pkg.ldiv(H, b0))
        t2 = time.perf_counter()
        tq.append(t1 - t0), tl.append(t2 - t1), tt.append(t2 - t0)
    tp = []
    with threadpool_limits(limits=16):
        for _ in range(reps):
            A = A0.copy(order="F")
            bl = b0.copy()
            t0 = time.perf_counter()
            qr_, tau, _, _ = lapack.zgeqrf(A, overwrite_a=True)
            cq, _, _ = lapack.zunmqr("L", "C", qr_, tau, bl.reshape(m, 1), lwork=64 * n)
            xl, _ = lapack.ztrtrs(qr_[:n, :n], cq[:n], lower=0)
            tp.append(time.perf_counter() - t0)
    xl = xl[:, 0]
    Ah = A0.conj().T
    ne = float(np.linalg.norm(Ah @ (A0 @ x - b0)))
    nel = float(np.linalg.norm(Ah @ (A0 @ xl - b0)))
    print(json.dumps({"m": m, "n": n, "dtype": "c64", "us_total": round(min(tt) * 1e6, 1), "us_qr": round(min(tq) * 1e6, 1),
                      "us_ldiv": round(min(tl) * 1e6, 1), "us_lapack": round(min(tp) * 1e6, 1),
                      "times_longer_than_lapack": round(min(tt) / min(tp), 3), "normal_eq": ne, "lapack_normal_eq": nel}), flush=True)
