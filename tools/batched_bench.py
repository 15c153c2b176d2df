"""Throughput of the batched qr! + `\\` (dhqr_factor_batched_f64 + dhqr_solve_batched_f64) against what a caller had before:
a loop of `batch` single calls (dhqr_factor_f64 with the small route on, then dhqr_solve_f64) on the same resident data.

usage: python tools/batched_bench.py [--out FILE]          every point, each in a child process under `timeout -k 10`
       python tools/batched_bench.py --point M N BATCH     one point (what the children run)
       --dtype f32                                         the Float32 entry points (dhqr_*_f32: native kernels up to 64 x 32,
                                                           the promoted tier beyond), same points, same columns
       --dtype c64                                         the ComplexF64 entry points (dhqr_factor_batched_c64 +
                                                           dhqr_solve_batched_c64 against the loop of dhqr_factor_c64 +
                                                           dhqr_solve_c64), at C64_SHAPES with batch 16384 unless --shapes /
                                                           --batches say otherwise; no one-CU column: ComplexF64 has no
                                                           one-workgroup tier.  With --nrhs K: the multi-column KERNEL
                                                           (DHQR_TUNE znrhs_wave=1) against the loop of K
                                                           dhqr_solve_batched_c64 calls, and the library's own rule, ROUNDS
                                                           rounds each.  With --applyq: as for the real types
                                                           Shapes beyond the wave tier up to 128 rows (e.g. --shapes
                                                           66x33,110x100,128x128) with --nrhs K or --applyq: the one-workgroup
                                                           multi-column kernel (DHQR_TUNE zsmall_nrhs=1) against the routes
                                                           without it (zsmall_nrhs=0: the column loop, the general apply-Q
                                                           kernel), one child process per arm in the same environment, ROUNDS
                                                           rounds each, kernel / parent round by round
       --shapes 16x8,32x16                                 only these shapes (default: every shape of SHAPES)
       --nrhs K [--batches 16384]                          `H_k \\ B_k` with K right-hand sides per matrix instead: ONE
                                                           dhqr_solve_batched_nrhs_* call against the loop of K
                                                           dhqr_solve_batched_* calls on the columns (the same resident factor;
                                                           the same bits, asserted); matrices/s and right-hand sides/s
       --applyq {t,n,q} [--nrhs 16] [--batches 16384]      Q_k'B_k (t), Q_k B_k (n) or the explicit thin Q_k (q) of a resident
                                                           batched factor: ONE dhqr_apply_q_batched_* / dhqr_form_q_batched_*
                                                           call, against dhqr_solve_batched_nrhs_* at the same shape and nrhs
                                                           (t does a strict subset of its work) and, Float64, against what a
                                                           caller had before: a loop of dhqr_apply_q_f64, one call per matrix
                                                           (on the first LOOP_BATCH matrices, scaled per matrix); ROUNDS
                                                           rounds of 10 repetitions each, every round's median listed
       --pivot [--dtype f64|f32|c64] [--shapes ...] [--batches 16384]
                                                           what column pivoting costs: dhqr_factor_batched_pivoted_* +
                                                           dhqr_rank_batched_* + dhqr_solve_batched_pivoted_* (one
                                                           right-hand side) against dhqr_factor_batched_* +
                                                           dhqr_solve_batched_* on the same resident data, at PIVOT_SHAPES
                                                           with batch 16384 unless told otherwise; ROUNDS rounds of 10
                                                           repetitions, every round's median, and the factors alone

Per point: 3 warm-up and 10 timed repetitions of (restore the inputs, synchronise, START, calls, synchronise, STOP) on the
host clock -- a caller's view, launch costs included; median and min-max of matrices per second; the ratio batched / looped
of the medians.  Shapes of at most 64 x 32 are also run with DHQR_TUNE batched_wave=0 (one workgroup per matrix instead of
one wave per matrix), which is what the wave kernels have to beat.  The run stops at the first point that fails."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(12, 6), (16, 8), (32, 16), (64, 32), (110, 100), (220, 200)]
BATCHES = [64, 1024, 16384]
WARMUP, REPS = 3, 10
ROUNDS, LOOP_BATCH = 5, 256  # --applyq
C64_SHAPES, C64_BATCHES = [(16, 8), (40, 17), (64, 32)], [16384]  # --dtype c64


def point(m, n, batch, dtype="f64"):
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    pkg = g.import_package()
    batch = min(batch, (4 << 30) // (m * n * 8) - 1)  # the batch stays under 4 GiB
    if dtype == "c64":
        return point_c64(pkg, torch, m, n, batch)
    tdt, esz = (torch.float32, 4) if dtype == "f32" else (torch.float64, 8)
    A0 = pkg.rand_colmajor_batched(batch, m, n, 1, "cuda:0", dtype=tdt)
    b0 = pkg.rand_colmajor_batched(batch, m, 1, 7, "cuda:0", dtype=tdt).reshape(batch, m).contiguous()
    A, b = A0.clone(), b0.clone()
    al = torch.zeros((batch, n), dtype=tdt, device="cuda:0")
    torch.cuda.synchronize()
    L = pkg._lib.lib()
    P = ctypes.c_void_p
    pa, pal, pb = A.data_ptr(), al.data_ptr(), b.data_ptr()
    factor_b, solve_b, factor_1, solve_1 = (getattr(L, f"dhqr_{k}_{dtype}") for k in ("factor_batched", "solve_batched", "factor", "solve"))
    os.environ["DHQR_SMALL"] = "1"

    def measure(ctx, fn):
        rates = []
        for r in range(WARMUP + REPS):
            A.copy_(A0)
            b.copy_(b0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(ctx.handle)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            if r >= WARMUP:
                rates.append(batch / dt)
        return {"median": statistics.median(rates), "min": min(rates), "max": max(rates)}

    def batched(h):
        pkg._lib.check(factor_b(h, P(pa), m, n, m, m * n, P(pal), n, batch, 0))
        pkg._lib.check(solve_b(h, P(pa), m, n, m, m * n, P(pal), n, P(pb), m, batch))

    def looped(h):
        for k in range(batch):
            ak, alk = P(pa + esz * k * m * n), P(pal + esz * k * n)
            pkg._lib.check(factor_1(h, ak, m, n, m, alk, 0))
            pkg._lib.check(solve_1(h, ak, m, n, m, alk, P(pb + esz * k * m)))

    out = {"m": m, "n": n, "batch": batch, "dtype": dtype}
    ctx = pkg.Context(0)
    out["batched"] = measure(ctx, batched)
    x = b[:, :n].clone()
    out["looped"] = measure(ctx, looped)
    ctx.close()
    if m <= 64 and n <= 32:
        if dtype == "f32":
            assert torch.equal(x, b[:, :n]), "a single Float32 matrix is a batch of 1: the same bits"
        assert ((x - b[:, :n]).abs().amax(dim=1) <= 1e-9 * x.abs().amax(dim=1)).all(), "batched and looped solutions differ"
        os.environ["DHQR_TUNE"] = "batched_wave=0"
        ctx = pkg.Context(0)
        out["batched_one_cu"] = measure(ctx, batched)
        ctx.close()
    else:
        assert torch.equal(x, b[:, :n]), "the one-workgroup tier must give the single calls' bits"
    print("POINT " + json.dumps(out), flush=True)


def point_c64(pkg, torch, m, n, batch):
    """ComplexF64: one dhqr_factor_batched_c64 + one dhqr_solve_batched_c64 against dhqr_factor_c64 + dhqr_solve_c64 per
    matrix on the same resident data"""
    A0 = pkg.rand_colmajor_batched_c(batch, m, n, 1, "cuda:0")
    b0 = pkg.rand_colmajor_batched_c(batch, m, 1, 7, "cuda:0").reshape(batch, m).contiguous()
    A, b = A0.clone(), b0.clone()
    al = torch.zeros((batch, n), dtype=torch.complex128, device="cuda:0")
    torch.cuda.synchronize()
    L = pkg._lib.lib()
    P = ctypes.c_void_p
    pa, pal, pb, esz = A.data_ptr(), al.data_ptr(), b.data_ptr(), 16
    os.environ["DHQR_SMALL"] = "1"

    def measure(ctx, fn):
        rates = []
        for r in range(WARMUP + REPS):
            A.copy_(A0)
            b.copy_(b0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(ctx.handle)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            if r >= WARMUP:
                rates.append(batch / dt)
        return {"median": statistics.median(rates), "min": min(rates), "max": max(rates)}

    def batched(h):
        pkg._lib.check(L.dhqr_factor_batched_c64(h, P(pa), m, n, m, m * n, P(pal), n, batch, 0))
        pkg._lib.check(L.dhqr_solve_batched_c64(h, P(pa), m, n, m, m * n, P(pal), n, P(pb), m, batch))

    def looped(h):
        for k in range(batch):
            ak, alk = P(pa + esz * k * m * n), P(pal + esz * k * n)
            pkg._lib.check(L.dhqr_factor_c64(h, ak, m, n, m, alk))
            pkg._lib.check(L.dhqr_solve_c64(h, ak, m, n, m, alk, P(pb + esz * k * m)))

    out = {"m": m, "n": n, "batch": batch, "dtype": "c64"}
    ctx = pkg.Context(0)
    out["batched"] = measure(ctx, batched)
    x = b[:, :n].clone()
    out["looped"] = measure(ctx, looped)
    ctx.close()
    assert ((x - b[:, :n]).abs().amax(dim=1) <= 1e-9 * x.abs().amax(dim=1)).all(), "batched and looped solutions differ"
    print("POINT " + json.dumps(out), flush=True)


def _makers(pkg, torch, dtype):
    """(random batch, empty batch, element size) of a dtype: (batch, rows, cols) device tensors with column-major matrices"""
    if dtype == "c64":
        return pkg.rand_colmajor_batched_c, pkg.empty_colmajor_batched_c, 16
    tdt, esz = (torch.float32, 4) if dtype == "f32" else (torch.float64, 8)
    return (lambda b, r, c, seed, dev: pkg.rand_colmajor_batched(b, r, c, seed, dev, dtype=tdt),
            lambda b, r, c, dev: pkg.empty_colmajor_batched(b, r, c, dev, dtype=tdt), esz)


def point_nrhs(m, n, batch, nrhs, dtype="f64"):
    """solve only: the factor stays resident; per repetition B is restored, then ONE multi-column call or K single-column ones"""
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    pkg = g.import_package()
    rand, empty, esz = _makers(pkg, torch, dtype)
    os.environ["DHQR_SMALL"] = "1"
    A = rand(batch, m, n, 1, "cuda:0")
    B0 = empty(batch, m, nrhs, "cuda:0")
    for r in range(nrhs):
        B0[:, :, r] = rand(batch, m, 1, 7 + 1000 * r, "cuda:0").reshape(batch, m)
    B = B0.clone(memory_format=torch.preserve_format)
    assert B.stride() == B0.stride() == (m * nrhs, 1, m)
    H = pkg.qr_batched_(A)
    al = H.α
    torch.cuda.synchronize()
    L = pkg._lib.lib()
    P = ctypes.c_void_p
    pa, pal, pb = A.data_ptr(), al.data_ptr(), B.data_ptr()
    solve_n, solve_1 = getattr(L, f"dhqr_solve_batched_nrhs_{dtype}"), getattr(L, f"dhqr_solve_batched_{dtype}")

    def measure(ctx, fn):
        rates = []
        for r in range(WARMUP + REPS):
            B.copy_(B0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(ctx.handle)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            if r >= WARMUP:
                rates.append(batch / dt)
        return {"median": statistics.median(rates), "min": min(rates), "max": max(rates)}

    def multi(h):
        pkg._lib.check(solve_n(h, P(pa), m, n, m, m * n, P(pal), n, P(pb), nrhs, m, m * nrhs, batch))

    def columns(h):
        for r in range(nrhs):
            pkg._lib.check(solve_1(h, P(pa), m, n, m, m * n, P(pal), n, P(pb + esz * r * m), m * nrhs, batch))

    out = {"m": m, "n": n, "batch": batch, "nrhs": nrhs, "dtype": dtype}
    if dtype == "c64":
        # the library sends a ComplexF64 call to the multi-column kernel or to the column loop by a speed rule; what the rule
        # is derived from is the KERNEL against the loop, so the kernel is forced here (DHQR_TUNE znrhs_wave=1, read when a
        # context is created) and the rule's own choice measured beside it; ROUNDS rounds each, for the spread
        os.environ["DHQR_TUNE"] = "znrhs_wave=1"
        forced = pkg.Context(0)
        del os.environ["DHQR_TUNE"]
        ctx = pkg.Context(0)
        out["kernel"], out["column_loop_rounds"], out["rule"] = [], [], []
        for _ in range(ROUNDS):
            out["kernel"].append(measure(forced, multi))
            X = B.clone()
            out["column_loop_rounds"].append(measure(ctx, columns))
            assert torch.equal(X, B), "the multi-column kernel and the loop over the columns must give the same bits"
            out["rule"].append(measure(ctx, multi))
            assert torch.equal(X, B)
        forced.close()
        ctx.close()
        print("POINT " + json.dumps(out), flush=True)
        return
    ctx = pkg.Context(0)
    out["nrhs_call"] = measure(ctx, multi)
    X = B.clone()
    out["column_loop"] = measure(ctx, columns)
    ctx.close()
    assert torch.equal(X, B), "the multi-column call and the loop over the columns must give the same bits"
    print("POINT " + json.dumps(out), flush=True)


def point_applyq(m, n, batch, nrhs, op, dtype="f64"):
    """the factor stays resident; per repetition B is restored (t, n; q writes only), then ONE call"""
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    pkg = g.import_package()
    rand, empty, esz = _makers(pkg, torch, dtype)
    os.environ["DHQR_SMALL"] = "1"
    cols = n if op == "q" else nrhs
    A = rand(batch, m, n, 1, "cuda:0")
    B0 = empty(batch, m, cols, "cuda:0")
    if op == "q":
        B0.zero_()
        B0.diagonal(dim1=1, dim2=2).fill_(1.0)  # [I; 0]: what the loop of single calls starts from
    else:
        for r in range(cols):
            B0[:, :, r] = rand(batch, m, 1, 7 + 1000 * r, "cuda:0").reshape(batch, m)
    B = B0.clone(memory_format=torch.preserve_format)
    assert B.stride() == B0.stride() == (m * cols, 1, m)
    H = pkg.qr_batched_(A)
    torch.cuda.synchronize()
    L = pkg._lib.lib()
    P = ctypes.c_void_p
    pa, pal, pb = A.data_ptr(), H.α.data_ptr(), B.data_ptr()
    apply_b, form_q, solve_n = (getattr(L, f"dhqr_{k}_{dtype}") for k in ("apply_q_batched", "form_q_batched", "solve_batched_nrhs"))
    trans = 1 if op == "t" else 0

    def measure(ctx, fn, count):
        rates = []
        for r in range(WARMUP + REPS):
            B.copy_(B0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(ctx.handle)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            if r >= WARMUP:
                rates.append(count / dt)
        return {"median": statistics.median(rates), "min": min(rates), "max": max(rates)}

    def new(h):
        if op == "q":
            pkg._lib.check(form_q(h, P(pa), m, n, m, m * n, P(pb), m, m * cols, batch))
        else:
            pkg._lib.check(apply_b(h, P(pa), m, n, m, m * n, P(pb), cols, m, m * cols, batch, trans))

    def solve(h):
        pkg._lib.check(solve_n(h, P(pa), m, n, m, m * n, P(pal), n, P(pb), cols, m, m * cols, batch))

    lb = min(batch, LOOP_BATCH)

    def looped(h):
        for k in range(lb):
            pkg._lib.check(L.dhqr_apply_q_f64(h, P(pa + esz * k * m * n), m, n, m, P(pb + esz * k * m * cols), cols, m, trans))

    out = {"m": m, "n": n, "batch": batch, "nrhs": cols, "op": op, "dtype": dtype, "loop_batch": lb, "new": [], "solve": [], "looped": []}
    ctx = pkg.Context(0)
    for _ in range(ROUNDS):
        out["new"].append(measure(ctx, new, batch))
        out["solve"].append(measure(ctx, solve, batch))
        if dtype == "f64":  # (dhqr_apply_q_f64: Float64 alone has a single-matrix apply-Q to loop over)
            out["looped"].append(measure(ctx, looped, lb))
    ctx.close()
    print("POINT " + json.dumps(out), flush=True)


def small_tier(m, n):
    """a ComplexF64 shape of the one-workgroup tier: beyond one wave per matrix, up to 128 rows"""
    return (m > 64 or n > 32) and n <= m <= 128


def point_arm(m, n, batch, nrhs, op):
    """one arm of the one-workgroup ComplexF64 comparison (the parent process has set DHQR_TUNE zsmall_nrhs=1 or 0): op = s
    (dhqr_solve_batched_nrhs_c64), t, n (dhqr_apply_q_batched_c64) or q (dhqr_form_q_batched_c64) on a resident factor, ROUNDS
    rounds; `sum`: a checksum of the result's bits (the solve's two arms must agree on it)"""
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    pkg = g.import_package()
    os.environ["DHQR_SMALL"] = "1"
    cols = n if op == "q" else nrhs
    A = pkg.rand_colmajor_batched_c(batch, m, n, 1, "cuda:0")
    B0 = pkg.empty_colmajor_batched_c(batch, m, cols, "cuda:0")
    if op == "q":
        B0.zero_()
    else:
        for r in range(cols):
            B0[:, :, r] = pkg.rand_colmajor_batched_c(batch, m, 1, 7 + 1000 * r, "cuda:0").reshape(batch, m)
    B = B0.clone(memory_format=torch.preserve_format)
    assert B.stride() == B0.stride() == (m * cols, 1, m)
    H = pkg.qr_batched_(A)
    torch.cuda.synchronize()
    L = pkg._lib.lib()
    P = ctypes.c_void_p
    pa, pal, pb = A.data_ptr(), H.α.data_ptr(), B.data_ptr()

    def call(h):
        if op == "s":
            pkg._lib.check(L.dhqr_solve_batched_nrhs_c64(h, P(pa), m, n, m, m * n, P(pal), n, P(pb), cols, m, m * cols, batch))
        elif op == "q":
            pkg._lib.check(L.dhqr_form_q_batched_c64(h, P(pa), m, n, m, m * n, P(pb), m, m * cols, batch))
        else:
            pkg._lib.check(L.dhqr_apply_q_batched_c64(h, P(pa), m, n, m, m * n, P(pb), cols, m, m * cols, batch, 1 if op == "t" else 0))

    ctx = pkg.Context(0)
    out = {"m": m, "n": n, "batch": batch, "nrhs": cols, "op": op, "tune": os.environ.get("DHQR_TUNE", ""), "rounds": []}
    for _ in range(ROUNDS):
        rates = []
        for r in range(WARMUP + REPS):
            B.copy_(B0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(ctx.handle)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            if r >= WARMUP:
                rates.append(batch / dt)
        out["rounds"].append({"median": statistics.median(rates), "min": min(rates), "max": max(rates)})
    ctx.close()
    out["sum"] = int(torch.view_as_real(B).contiguous().view(torch.int64).sum().item())
    print("POINT " + json.dumps(out), flush=True)


def main_arms(a, shapes, batches):
    op, K = (a.applyq or "s"), (a.nrhs or 16)
    what = {"s": f"H_k \\ B_k (dhqr_solve_batched_nrhs_c64), {K} right-hand sides", "t": f"B_k <- Q_k^H B_k (dhqr_apply_q_batched_c64), {K} columns",
            "n": f"B_k <- Q_k B_k (dhqr_apply_q_batched_c64), {K} columns", "q": "explicit thin Q_k (dhqr_form_q_batched_c64, nrhs = n)"}[op]
    lines = [f"# tools/batched_bench.py --dtype c64 {'--applyq ' + op if a.applyq else ''} --nrhs {K}: {what}, resident factor; matrices per second",
             f"# kernel = DHQR_TUNE zsmall_nrhs=1 (k_small_zapply), parent = zsmall_nrhs=0 (" +
             ("the loop of k_small_zldiv launches; the same bits, checked" if op == "s" else "k_batched_zapplyq_general") +
             f"); one child process per arm; {ROUNDS} rounds of {REPS} repetitions each: every round's median, then min .. max over all repetitions"]
    print("\n".join(lines), flush=True)
    rounds = lambda rs: " ".join(f"{x['median']:.0f}" for x in rs) + f" ({min(x['min'] for x in rs):.0f} .. {max(x['max'] for x in rs):.0f})"
    rc = 0
    for (m, n) in shapes:
        for batch in batches:
            arms = {}
            for arm in ("1", "0"):
                env = dict(os.environ, DHQR_TUNE=f"zsmall_nrhs={arm}")
                p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--point", str(m), str(n),
                                    str(batch), "--dtype", "c64", "--nrhs", str(K), "--arm", op], capture_output=True, text=True, env=env)
                row = [ln for ln in p.stdout.splitlines() if ln.startswith("POINT ")]
                if p.returncode != 0 or not row:
                    lines.append(f"{m}x{n} batch {batch} {op} zsmall_nrhs={arm}: FAILED (exit {p.returncode}); stopping\n{p.stderr[-2000:]}")
                    print(lines[-1], flush=True)
                    rc = 1
                    break
                arms[arm] = json.loads(row[0][6:])
            if rc:
                break
            k, o = arms["1"], arms["0"]
            if op == "s" and k["sum"] != o["sum"]:
                lines.append(f"{m}x{n} batch {batch}: the two arms of the solve differ in a bit; stopping")
                print(lines[-1], flush=True)
                rc = 1
                break
            ratios = [x["median"] / y["median"] for x, y in zip(k["rounds"], o["rounds"])]
            med = lambda rs: statistics.median(x["median"] for x in rs)
            txt = (f"{m:4d} x {n:<4d} batch {k['batch']:6d} nrhs {k['nrhs']:3d} c64 {op} | kernel {rounds(k['rounds'])} | parent {rounds(o['rounds'])} | "
                   f"kernel/parent per round {' '.join(f'{x:.3f}' for x in ratios)} | median {med(k['rounds']) / med(o['rounds']):5.2f}x")
            lines.append(txt)
            print(txt, flush=True)
        if rc:
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


def main_applyq(a, shapes, batches):
    t, K, op = a.dtype, (a.nrhs or 16), a.applyq
    what = {"t": "B_k <- Q_k'B_k", "n": "B_k <- Q_k B_k", "q": "explicit thin Q_k (nrhs = n)"}[op]
    call = f"dhqr_form_q_batched_{t}" if op == "q" else f"dhqr_apply_q_batched_{t} (trans = {1 if op == 't' else 0})"
    lines = [f"# tools/batched_bench.py --applyq {op} --nrhs {K} --dtype {t}: {what}, resident factor; matrices per second",
             f"# {ROUNDS} rounds of {REPS} timed repetitions in one process: every round's median, then min .. max over all repetitions",
             f"# new = one {call}; solve = one dhqr_solve_batched_nrhs_{t}, same shape and columns; looped (Float64) = "
             f"dhqr_apply_q_f64 per matrix on the first {LOOP_BATCH} matrices, per matrix"]
    print("\n".join(lines), flush=True)

    def rounds(rs):
        return (" ".join(f"{r['median']:.0f}" for r in rs) + f" ({min(r['min'] for r in rs):.0f} .. {max(r['max'] for r in rs):.0f})")

    rc = 0
    for (m, n) in shapes:
        for batch in batches:
            p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--point",
                                str(m), str(n), str(batch), "--dtype", t, "--nrhs", str(K), "--applyq", op], capture_output=True, text=True)
            row = [ln for ln in p.stdout.splitlines() if ln.startswith("POINT ")]
            if p.returncode != 0 or not row:
                lines.append(f"{m}x{n} batch {batch} applyq {op}: FAILED (exit {p.returncode}); stopping\n{p.stderr[-2000:]}")
                print(lines[-1], flush=True)
                rc = 1
                break
            r = json.loads(row[0][6:])
            med = lambda rs: statistics.median(x["median"] for x in rs)
            txt = (f"{m:4d} x {n:<4d} batch {r['batch']:6d} nrhs {r['nrhs']:3d} {t} {op} | new {rounds(r['new'])} | solve {rounds(r['solve'])} | "
                   f"new/solve {med(r['new']) / med(r['solve']):5.2f}x")
            if r["looped"]:
                txt += f" | looped {rounds(r['looped'])} | new/looped {med(r['new']) / med(r['looped']):8.0f}x"
            lines.append(txt)
            print(txt, flush=True)
        if rc:
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


PIVOT_SHAPES = [(16, 8), (40, 17), (64, 32)]


def point_pivot(m, n, batch, t="f64"):
    """one point of --pivot: pivoted (factor + rank + truncated solve) and unpivoted (factor + solve) of the element type t on
    the same inputs -- the project's generator with column c scaled by 1 + 0.25 c, full rank (f32: rounded) --, and each
    factor alone"""
    sys.path.insert(0, ROOT)
    import torch
    import __graft_entry__ as g
    pkg = g.import_package()
    os.environ["DHQR_SMALL"] = "1"
    if t == "c64":
        A0 = pkg.rand_colmajor_batched_c(batch, m, n, 1, "cuda:0")
        b0 = pkg.rand_colmajor_batched_c(batch, m, 1, 7, "cuda:0").reshape(batch, m).contiguous()
    else:
        dt = torch.float32 if t == "f32" else torch.float64
        A0 = pkg.rand_colmajor_batched(batch, m, n, 1, "cuda:0", dt)
        b0 = pkg.rand_colmajor_batched(batch, m, 1, 7, "cuda:0", dt).reshape(batch, m).contiguous()
    A0 *= (1.0 + 0.25 * torch.arange(n, dtype=torch.float64, device="cuda:0")).to(A0.dtype)
    A, b = A0.clone(), b0.clone()
    al = torch.zeros((batch, n), dtype=A0.dtype, device="cuda:0")
    jp = torch.zeros((batch, n), dtype=torch.int32, device="cuda:0")
    rk = torch.zeros((batch,), dtype=torch.int32, device="cuda:0")
    x = torch.zeros((batch, n), dtype=A0.dtype, device="cuda:0")
    torch.cuda.synchronize()
    L, P, chk = pkg._lib.lib(), ctypes.c_void_p, pkg._lib.check
    pa, pal, pb, pjp, prk, px = (P(t.data_ptr()) for t in (A, al, b, jp, rk, x))
    ctx = pkg.Context(0)
    h = ctx.handle

    def f_piv():
        chk(getattr(L, f"dhqr_factor_batched_pivoted_{t}")(h, pa, m, n, m, m * n, pal, n, pjp, n, batch))

    def f_plain():
        chk(getattr(L, f"dhqr_factor_batched_{t}")(h, pa, m, n, m, m * n, pal, n, batch, 0))

    def pivoted():
        f_piv()
        chk(getattr(L, f"dhqr_rank_batched_{t}")(h, pal, m, n, n, -1.0, prk, batch))
        chk(getattr(L, f"dhqr_solve_batched_pivoted_{t}")(h, pa, m, n, m, m * n, pal, n, pjp, n, prk, pb, 1, m, m, px, n, n, batch))

    def plain():
        f_plain()
        chk(getattr(L, f"dhqr_solve_batched_{t}")(h, pa, m, n, m, m * n, pal, n, pb, m, batch))

    def measure(fn):
        rates = []
        for r in range(WARMUP + REPS):
            A.copy_(A0)
            b.copy_(b0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            dt = time.perf_counter() - t0
            if r >= WARMUP:
                rates.append(batch / dt)
        return {"median": statistics.median(rates), "min": min(rates), "max": max(rates)}

    out = {"m": m, "n": n, "batch": batch, "dtype": t, "pivoted": [], "plain": [], "factor_pivoted": [], "factor_plain": []}
    for _ in range(ROUNDS):
        out["pivoted"].append(measure(pivoted))
        xp = x.clone()
        out["plain"].append(measure(plain))
        xu = b[:, :n].clone()
        out["factor_pivoted"].append(measure(f_piv))
        out["factor_plain"].append(measure(f_plain))
    assert int(rk.min()) == n, "the inputs were meant to have full rank"
    tol = 1e-3 if t == "f32" else 1e-9  # (two orders of the columns: the results differ by rounding times the condition number)
    assert ((xp - xu).abs().amax(dim=1) <= tol * xp.abs().amax(dim=1)).all(), "pivoted and unpivoted solutions differ"
    ctx.close()
    print("POINT " + json.dumps(out), flush=True)


def main_pivot(a, shapes, batches):
    t = a.dtype
    lines = [f"# tools/batched_bench.py --pivot --dtype {t}: matrices per second, {ROUNDS} rounds of {REPS} repetitions in one process, every round's median, then min .. max over all repetitions",
             f"# pivoted = dhqr_factor_batched_pivoted_{t} + dhqr_rank_batched_{t} + dhqr_solve_batched_pivoted_{t} (one right-hand side, X written);",
             f"# unpivoted = dhqr_factor_batched_{t} + dhqr_solve_batched_{t}; the same resident full-rank inputs; `factors` = the two factor calls alone"]
    print("\n".join(lines), flush=True)
    rc = 0
    for (m, n) in shapes:
        for batch in batches:
            p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--point",
                                str(m), str(n), str(batch), "--pivot", "--dtype", t], capture_output=True, text=True)
            row = [ln for ln in p.stdout.splitlines() if ln.startswith("POINT ")]
            if p.returncode != 0 or not row:
                lines.append(f"{m}x{n} batch {batch}: FAILED (exit {p.returncode}); stopping\n{p.stderr[-2000:]}")
                print(lines[-1], flush=True)
                rc = 1
                break
            r = json.loads(row[0][6:])
            med = lambda rs: statistics.median(v["median"] for v in rs)
            rounds = lambda rs: " ".join(f"{v['median']:.0f}" for v in rs) + f" ({min(v['min'] for v in rs):.0f} .. {max(v['max'] for v in rs):.0f})"
            ratios = " ".join("%.3f" % (x["median"] / y["median"]) for x, y in zip(r["pivoted"], r["plain"]))
            txt = (f"{m:4d} x {n:<4d} batch {r['batch']:6d} {t} | pivoted {rounds(r['pivoted'])} | unpivoted {rounds(r['plain'])} | "
                   f"pivoted/unpivoted per round {ratios} | "
                   f"median {med(r['pivoted']) / med(r['plain']):5.2f}x | factors: pivoted {med(r['factor_pivoted']):.0f} unpivoted "
                   f"{med(r['factor_plain']):.0f} ratio {med(r['factor_pivoted']) / med(r['factor_plain']):5.2f}x")
            lines.append(txt)
            print(txt, flush=True)
        if rc:
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


def fmt(r):
    return f"{r['median']:12.0f} ({r['min']:.0f} .. {r['max']:.0f})"


def main_nrhs(a, shapes, batches):
    t, K = a.dtype, a.nrhs
    lines = [f"# tools/batched_bench.py --nrhs {K} --dtype {t}: H_k \\ B_k, {K} right-hand sides per matrix, resident factor; median (min .. max) of 10 repetitions",
             f"# nrhs call = one dhqr_solve_batched_nrhs_{t}; column loop = {K} x dhqr_solve_batched_{t} on the columns of the same B (the same bits, asserted)"]
    if t == "c64":
        lines[0] = (f"# tools/batched_bench.py --nrhs {K} --dtype c64: H_k \\ B_k, {K} right-hand sides per matrix, resident factor; matrices per second; "
                    f"{ROUNDS} rounds of {REPS} repetitions in one process, every round's median, then min .. max over all repetitions")
        lines[1] = (f"# kernel = one dhqr_solve_batched_nrhs_c64 with DHQR_TUNE znrhs_wave=1 (always the multi-column kernel); column loop = {K} x "
                    "dhqr_solve_batched_c64 on the columns of the same B (the same bits, asserted); the library's rule = the same call, default context")
    print("\n".join(lines), flush=True)
    for (m, n) in shapes:
        for batch in batches:
            p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--point",
                                str(m), str(n), str(batch), "--dtype", t, "--nrhs", str(K)], capture_output=True, text=True)
            row = [ln for ln in p.stdout.splitlines() if ln.startswith("POINT ")]
            if p.returncode != 0 or not row:
                lines.append(f"{m}x{n} batch {batch} nrhs {K}: FAILED (exit {p.returncode}); stopping\n{p.stderr[-2000:]}")
                print(lines[-1], flush=True)
                if a.out:
                    with open(a.out, "w") as f:
                        f.write("\n".join(lines) + "\n")
                return 1
            r = json.loads(row[0][6:])
            if t == "c64":
                med = lambda rs: statistics.median(x["median"] for x in rs)
                rounds = lambda rs: " ".join(f"{x['median']:.0f}" for x in rs) + f" ({min(x['min'] for x in rs):.0f} .. {max(x['max'] for x in rs):.0f})"
                ratios = [k["median"] / c["median"] for k, c in zip(r["kernel"], r["column_loop_rounds"])]
                txt = (f"{m:4d} x {n:<4d} batch {r['batch']:6d} nrhs {K:3d} c64 | kernel {rounds(r['kernel'])} | column loop {rounds(r['column_loop_rounds'])} | "
                       f"kernel/loop per round {' '.join(f'{x:.3f}' for x in ratios)} | median {med(r['kernel']) / med(r['column_loop_rounds']):5.2f}x | "
                       f"the library's rule {rounds(r['rule'])}")
                lines.append(txt)
                print(txt, flush=True)
                continue
            new, old = r["nrhs_call"], r["column_loop"]
            txt = (f"{m:4d} x {n:<4d} batch {r['batch']:6d} nrhs {K:3d} {t} | nrhs call {fmt(new)} matrices/s {new['median'] * K:13.0f} rhs/s | "
                   f"column loop {fmt(old)} matrices/s {old['median'] * K:13.0f} rhs/s | nrhs/loop {new['median'] / old['median']:6.2f}x")
            lines.append(txt)
            print(txt, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", nargs=3, type=int)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dtype", choices=("f64", "f32", "c64"), default="f64")
    ap.add_argument("--shapes", default=None, help="e.g. 16x8,32x16 (default: every shape)")
    ap.add_argument("--nrhs", type=int, default=None, help="right-hand sides per matrix: the multi-column solve against the column loop")
    ap.add_argument("--applyq", choices=("t", "n", "q"), default=None, help="Q'B, QB or the explicit Q of a resident batched factor")
    ap.add_argument("--batches", default=None, help="e.g. 16384 or 64,1024 (default: every batch of BATCHES)")
    ap.add_argument("--arm", choices=("s", "t", "n", "q"), default=None, help="(what main_arms runs in a child: one arm of one point)")
    ap.add_argument("--pivot", action="store_true", help="column-pivoted factor + rank + truncated solve against the unpivoted factor + solve")
    ap.add_argument("--limit", type=int, default=300, help="seconds per point (timeout -k 10)")
    a = ap.parse_args()
    if a.point:
        if a.pivot:
            point_pivot(*a.point, a.dtype)
        elif a.arm is not None:
            point_arm(*a.point, a.nrhs or 16, a.arm)
        elif a.applyq is not None:
            point_applyq(*a.point, a.nrhs or 16, a.applyq, a.dtype)
        elif a.nrhs is not None:
            point_nrhs(*a.point, a.nrhs, a.dtype)
        else:
            point(*a.point, a.dtype)
        return 0
    t = a.dtype
    shapes = (C64_SHAPES if t == "c64" else SHAPES) if a.shapes is None else [tuple(int(v) for v in sh.split("x")) for sh in a.shapes.split(",")]
    batches = (C64_BATCHES if t == "c64" else BATCHES) if a.batches is None else [int(v) for v in a.batches.split(",")]
    if a.pivot:
        return main_pivot(a, PIVOT_SHAPES if a.shapes is None else shapes, batches if a.batches is not None else [16384])
    if t == "c64" and (a.applyq is not None or a.nrhs is not None) and all(small_tier(m, n) for m, n in shapes):
        return main_arms(a, shapes, batches if a.batches is not None else [16384])
    if a.applyq is not None:
        return main_applyq(a, shapes, batches if a.batches is not None else [16384])
    if a.nrhs is not None:
        return main_nrhs(a, shapes, batches)
    lines = ["# tools/batched_bench.py: qr! + \\ of `batch` matrices, matrices per second, median (min .. max) of 10 repetitions",
             f"# batched = one dhqr_factor_batched_{t} + one dhqr_solve_batched_{t}; looped = batch x (dhqr_factor_{t} + dhqr_solve_{t}), small route on",
             "# one-CU = the batched calls with DHQR_TUNE batched_wave=0 (one workgroup per matrix) on the wave tier's shapes"]
    if t == "c64":
        lines[2] = "# (ComplexF64: one wave per matrix up to 64 x 32, one workgroup per matrix up to 128 rows; no one-CU column is measured)"
    print("\n".join(lines), flush=True)
    for (m, n) in shapes:
        for batch in batches:
            p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--point",
                                str(m), str(n), str(batch), "--dtype", t], capture_output=True, text=True)
            row = [ln for ln in p.stdout.splitlines() if ln.startswith("POINT ")]
            if p.returncode != 0 or not row:
                lines.append(f"{m}x{n} batch {batch}: FAILED (exit {p.returncode}); stopping\n{p.stderr[-2000:]}")
                print(lines[-1], flush=True)
                break
            r = json.loads(row[0][6:])
            txt = (f"{m:4d} x {n:<4d} batch {r['batch']:6d} | batched {fmt(r['batched'])} | looped {fmt(r['looped'])} | "
                   f"batched/looped {r['batched']['median'] / r['looped']['median']:8.1f}x")
            if "batched_one_cu" in r:
                txt += (f" | one-CU {fmt(r['batched_one_cu'])} | wave/one-CU "
                        f"{r['batched']['median'] / r['batched_one_cu']['median']:6.1f}x")
            lines.append(txt)
            print(txt, flush=True)
        else:
            continue
        break
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
