"""Results must not depend on timing.  The rest of the suite judges every route once, against the oracle, at a tolerance:
that finds a kernel that is wrong, not a missing event wait or a buffer reused while a copy is in flight.  Here every route
runs repeatedly from the same input and the raw BYTES of its outputs are compared (the library has no floating-point
atomics and no dynamic work split that changes a sum's order), once more beside a busy second stream, under the serial
schedule (DHQR_LOOKAHEAD=0), and -- in child processes -- through the staged host path (DHQR_HOSTIO=1) against the plain
one.  Every bitwise assertion is an equality of bytes; the only tolerances are those of the route's existing test, named
where they are used."""
import contextlib
import time

import numpy as np
import pytest

from schedule_helpers import compare_hostio, first_difference, hostio_case_names, run_hostio_children
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class GaveUp(Exception):
    """a documented outcome of a route with bounded inter-workgroup waits (include/dhqr.h): NaN in every alpha of the
    device-resident small route, the pipeline error of dhqr_synchronize, or a solve repeated by the library itself"""


@contextlib.contextmanager
def _as_default(pkg, ctx):
    """api.py's calls take the context of device 0 from api._contexts: put `ctx` there for the duration"""
    api = pkg.api
    old = api._contexts.get(0)
    api._contexts[0] = ctx
    try:
        yield
    finally:
        api._contexts.pop(0, None)
        if old is not None:
            api._contexts[0] = old


_ORACLE = {}


def _oracle(orc, m, n, seed, complex_=False):
    """(H, alpha) of the oracle, computed once per shape for the whole file and never modified"""
    key = (m, n, seed, complex_)
    if key not in _ORACLE:
        A0 = orc.rand_matrix_c(m, n, seed) if complex_ else orc.rand_matrix(m, n, seed)
        _ORACLE[key] = orc.householder_c(A0) if complex_ else orc.householder(A0)
    return _ORACLE[key]


def _judge_factor(orc, out, m, n, seed, complex_=False, key="factor", akey="alpha"):
    """TOL of test_gpu_parity.py relative to max|H|: the bound of test_blocked_vs_oracle and of every route's own test"""
    Ho, ao = _oracle(orc, m, n, seed, complex_)
    scale = np.abs(Ho).max()
    eH, ea = np.abs(out[key].reshape(Ho.shape) - Ho).max(), np.abs(out[akey] - ao).max()
    assert eH <= TOL(Ho) * scale and ea <= TOL(Ho) * scale, f"|dH| = {eH / scale:.2e}, |dalpha| = {ea / scale:.2e} (max|H|)"


def _judge_x(x, xo, what="x"):
    """1e-9 relative: the bound on x of every existing solve test"""
    e = np.abs(x - xo).max()
    assert e <= 1e-9 * np.abs(xo).max(), f"|d{what}| = {e / np.abs(xo).max():.2e} relative"


def _np(t):
    """host copy of a device tensor in its logical (row, column) index order"""
    return np.ascontiguousarray(t.cpu().numpy())


def _raise_if_gave_up(e):
    if "gave up waiting" in str(e):
        raise GaveUp(str(e)) from e
    raise e


class Route:
    """one row of the table: `env` is read by dhqr_create (set before a context or handle is made); `call(pkg, ctx, inp)`
    returns {name: numpy array}; `judge(orc, out)` compares one result with the oracle; handle: 'ctx' (a pkg.Context) or
    'mg' (a pkg.MultiGpuQR of `ranks` logical ranks on cuda:0)"""

    def __init__(self, id, prepare, call, judge, env=None, bounded=False, busy=False, ranks=0, small=False):
        self.id, self.prepare, self.call, self.judge = id, prepare, call, judge
        self.env, self.bounded, self.busy, self.ranks, self.small = env or {}, bounded, busy, ranks, small
        self.meta = {}

    def open(self, pkg):
        if self.ranks:
            return pkg.MultiGpuQR(devices=[0] * self.ranks)
        ctx = pkg.Context(0)
        ctx.set_small_route(self.small)
        return ctx


def _run(route, ctx, inp=None, pkg=None):
    """raw bytes of every output of ONE call of the route on the context / handle `ctx`"""
    out = route.call(pkg, ctx, inp)
    route.meta = {k: (v.dtype, v.shape) for k, v in out.items()}
    return {k: np.ascontiguousarray(v).tobytes() for k, v in out.items()}


def _arrays(route, raw):
    return {k: np.frombuffer(b, dtype=route.meta[k][0]).reshape(route.meta[k][1]) for k, b in raw.items()}


def _diff(route, a, b):
    msg = first_difference(a, b, {k: v[0] for k, v in route.meta.items()})
    if msg is None:
        return None
    name = msg.split(":")[0]
    el = int(msg.split("first at element ")[1].split(":")[0]) if "first at element" in msg else None
    if el is not None and len(route.meta[name][1]) > 1:
        msg += f" (index {tuple(int(i) for i in np.unravel_index(el, route.meta[name][1]))} of shape {route.meta[name][1]})"
    return msg


# --------------------------------------------------------------------------------------------------- the routes
def _factor_f64(m, n, nb, seed, id, env=None, bounded=False, busy=False):
    def prepare(pkg, orc):
        return {"A": pkg.rand_colmajor(m, n, seed, DEV)}

    def call(pkg, ctx, inp):
        import torch
        A = inp["A"].clone()
        with _as_default(pkg, ctx):
            try:
                H = pkg.qr_(A, nb=nb)  # nb = 0: synchronises the context and reports the lead pipeline's error word
            except pkg._lib.DHQRError as e:
                _raise_if_gave_up(e)
        torch.cuda.synchronize()
        return {"factor": _np(H.A), "alpha": _np(H.α)}

    return Route(id, prepare, call, lambda orc, out: _judge_factor(orc, out, m, n, seed), env=env, bounded=bounded, busy=busy)


def _small_route(m, n, id):
    """device-resident dhqr_factor_f64 + dhqr_solve_f64 on the single-workgroup route (test_small_route_vs_oracle: seeds 41 /
    42, TOL, 1e-9 on x); (220, 200) runs the LDS-flag form, (110, 100) the barrier form"""
    def prepare(pkg, orc):
        import torch
        return {"A": pkg.rand_colmajor(m, n, 41, DEV), "b": torch.tensor(orc.rand_vector(m, 42), device=DEV)}

    def call(pkg, ctx, inp):
        import torch
        with _as_default(pkg, ctx):
            H = pkg.qr_(inp["A"].clone(), nb=128)
            torch.cuda.synchronize()
            al = _np(H.α)
            if np.isnan(al).all():
                raise GaveUp("NaN in every alpha (the flag form of the small route gave up on a wait)")
            x = pkg.ldiv(H, inp["b"])
        torch.cuda.synchronize()
        return {"factor": _np(H.A), "alpha": al, "x": _np(x)}

    def judge(orc, out):
        _judge_factor(orc, out, m, n, 41)
        Ho, ao = _oracle(orc, m, n, 41)
        _judge_x(out["x"], orc.solve(Ho, ao, orc.rand_vector(m, 42)))

    return Route(id, prepare, call, judge, bounded=True, small=True)


def _batched(m, n, batch, id, busy):
    """qr_batched_ / ldiv_batched (test_batched_vs_oracle: seed 100, b from seed 5100, tolerances of the small route); the
    batch sizes are no multiples of 4 (the wave tier packs four matrices into a workgroup)"""
    seed = 100

    def prepare(pkg, orc):
        with _as_default(pkg, pkg.get_context(0)):
            return {"A": pkg.rand_colmajor_batched(batch, m, n, seed, DEV),
                    "b": pkg.rand_colmajor_batched(batch, m, 1, seed + 5000, DEV).reshape(batch, m).contiguous()}

    def call(pkg, ctx, inp):
        import torch
        with _as_default(pkg, ctx):
            H = pkg.qr_batched_(inp["A"].clone())
            x = pkg.ldiv_batched(H, inp["b"])
        torch.cuda.synchronize()
        return {"factor": _np(H.A), "alpha": _np(H.α), "x": _np(x)}

    def judge(orc, out):
        tol = 8.0 * max(n, 8) * np.finfo(np.float64).eps  # test_batched_vs_oracle
        for k in sorted({0, 1, 2, 3, batch // 2, batch - 3, batch - 2, batch - 1}):
            Ho, ao = orc.householder(orc.rand_matrix(m, n, seed + k))
            xo = orc.solve(Ho, ao, orc.rand_vector(m, seed + 5000 + k))
            scale = np.abs(Ho).max()
            assert np.abs(out["factor"][k] - Ho).max() <= tol * scale and np.abs(out["alpha"][k] - ao).max() <= tol * scale, k
            _judge_x(out["x"][k], xo, f"x[{k}]")

    return Route(id, prepare, call, judge, busy=busy, small=True)


def _spmd_one_rank(kind, m, n, seed, id):
    """dhqr_cs_* / dhqr_rs_* at world size 1 (test_column_cyclic_driver_single_rank: seed 8, test_row_split_driver_single_rank:
    seed 41; TOL)"""
    def call(pkg, ctx, inp):
        import torch
        q = (pkg.ColumnCyclicQR if kind == "cs" else pkg.RowSplitQR)(m, n, ctx=ctx)
        try:
            q.fill(seed)
            q.factor()
            torch.cuda.synchronize()
            H, al = q.local_numpy()
            return {"factor": np.ascontiguousarray(H), "alpha": np.ascontiguousarray(al)}
        finally:
            q.comm.close()

    return Route(id, lambda pkg, orc: None, call, lambda orc, out: _judge_factor(orc, out, m, n, seed), busy=True)


def _solve(m, n, mode, id):
    """dhqr_solve_f64 on a resident factor in the three modes of test_solve_on_guarded_layouts (seeds 31 / 32): db[0:n] = x
    within 1e-9 relative, db[n:m] = (Q'b)[n:m] within 1e-12 max(1, |Q'b|)"""
    import ctypes
    P = ctypes.c_void_p
    env = {"gram": {"DHQR_KEEP_T": "0"}, "persistent": {"DHQR_SOLVE_PIPE": "3"}}.get(mode, {})

    def prepare(pkg, orc):
        import torch
        Ho, ao = _oracle(orc, m, n, 31)
        cm = lambda X: torch.from_numpy(np.ascontiguousarray(X.T)).to(DEV).T  # noqa: E731  (column-major device copy)
        return {"A0": pkg.rand_colmajor(m, n, 31, DEV), "Ho": cm(Ho), "ao": torch.from_numpy(ao.copy()).to(DEV),
                "b": torch.tensor(orc.rand_vector(m, 32), device=DEV)}

    def call(pkg, ctx, inp):
        import torch
        L = pkg._lib.lib()
        ctx.use_torch_stream()
        if mode == "kept_t":  # right after a blocked factorisation of the same buffer: T' kept by the factorisation
            A, al = inp["A0"].clone(), torch.empty(n, dtype=torch.float64, device=DEV)
            pkg._lib.check(L.dhqr_factor_f64(ctx.handle, P(A.data_ptr()), m, n, m, P(al.data_ptr()), 128))
        else:
            A, al = inp["Ho"].clone(), inp["ao"].clone()
        b = inp["b"].clone()
        r0 = ctx.solve_retries()
        pkg._lib.check(L.dhqr_solve_f64(ctx.handle, P(A.data_ptr()), m, n, m, P(al.data_ptr()), P(b.data_ptr())))
        try:
            ctx.synchronize()
        except pkg._lib.DHQRError as e:
            _raise_if_gave_up(e)
        if ctx.solve_retries() != r0:
            raise GaveUp("the library repeated the solve (dhqr_get_solve_retries advanced)")
        return {"x": _np(b)}

    def judge(orc, out):
        Ho, ao = _oracle(orc, m, n, 31)
        b = orc.rand_vector(m, 32)
        _judge_x(out["x"][:n], orc.solve(Ho, ao, b))
        y = b.copy()
        for j in range(n):
            y[j:] -= Ho[j:, j] * (Ho[j:, j] @ y[j:])
        et = np.abs(out["x"][n:] - y[n:]).max()
        assert et <= 1e-12 * max(1.0, np.abs(y).max()), f"|d(Q'b)[n:m]| = {et:.2e}"

    return Route(id, prepare, call, judge, env=env, bounded=True)


def _complex(m, n, nb, id):
    """dhqr_factor_c64_nb + dhqr_solve_c64 (test_complex_on_guarded_layouts: seeds 8 / 9, TOL, 1e-9 on x)"""
    def prepare(pkg, orc):
        import torch
        A0 = orc.rand_matrix_c(m, n, 8)
        return {"A": torch.from_numpy(np.ascontiguousarray(A0.T)).to(DEV).T, "b": torch.from_numpy(orc.rand_vector_c(m, 9)).to(DEV)}

    def call(pkg, ctx, inp):
        import torch
        with _as_default(pkg, ctx):
            try:
                H = pkg.qr_(inp["A"].clone(), nb=nb)
                x = pkg.ldiv(H, inp["b"])
            except pkg._lib.DHQRError as e:
                _raise_if_gave_up(e)
        torch.cuda.synchronize()
        return {"factor": _np(H.A), "alpha": _np(H.α), "x": _np(x)}

    def judge(orc, out):
        _judge_factor(orc, out, m, n, 8, complex_=True)
        Ho, ao = _oracle(orc, m, n, 8, True)
        _judge_x(out["x"], orc.solve_c(Ho, ao, orc.rand_vector_c(m, 9)))

    return Route(id, prepare, call, judge, bounded=True)


def _mg(kind, ranks, m, n, id, busy=False):
    """logical ranks on one GPU: dhqr_mg_* column split (test_multi_device_handle_logical_ranks_one_gpu: seeds 11 / 12),
    dhqr_mg_rs_* row split (test_row_split_logical_ranks_one_gpu: seeds 43 / 44); whatever download returns, and x"""
    seed = 11 if kind == "cs" else 43

    def call(pkg, mg, inp):
        if kind == "cs":
            mg.alloc(m, n).fill(seed).factor()
            H, al = mg.download()
            x = mg.solve(inp["b"])
        else:
            mg.rs_alloc(m, n).rs_fill(seed).rs_factor()
            H, al = mg.rs_download()
            x = mg.rs_solve(inp["b"])
        return {"factor": H, "alpha": al, "x": x}

    def judge(orc, out):
        _judge_factor(orc, out, m, n, seed)
        Ho, ao = _oracle(orc, m, n, seed)
        _judge_x(out["x"], orc.solve(Ho, ao, orc.rand_vector(m, seed + 1)))

    return Route(id, lambda pkg, orc: {"b": orc.rand_vector(m, seed + 1)}, call, judge, ranks=ranks, busy=busy)


def _mg_complex(ranks, m, n, id):
    """dhqr_mg_qr_c64 / dhqr_mg_ldiv_c64 (test_complex_column_split_logical_ranks_one_gpu: seeds 3 / 4; its tolerance is
    max(TOL, 64 kappa eps) with kappa = 1 below 1000 columns, i.e. TOL)"""
    def prepare(pkg, orc):
        return {"A": orc.rand_matrix_c(m, n, 3), "b": orc.rand_vector_c(m, 4)}

    def call(pkg, mg, inp):
        try:
            H, al = mg.qr_(np.asfortranarray(inp["A"].copy()))
            x = mg.ldiv(H, al, inp["b"])
        except pkg._lib.DHQRError as e:
            _raise_if_gave_up(e)
        return {"factor": H, "alpha": al, "x": x}

    def judge(orc, out):
        _judge_factor(orc, out, m, n, 3, complex_=True)
        Ho, ao = _oracle(orc, m, n, 3, True)
        _judge_x(out["x"], orc.solve_c(Ho, ao, orc.rand_vector_c(m, 4)))

    return Route(id, prepare, call, judge, ranks=ranks, bounded=True)


def _host(m, n, nb, id):
    """dhqr_qr_f64 + dhqr_ldiv_f64 on host arrays (test_host_entry_points_on_guarded_layouts: seeds 12 / 13, TOL, 1e-9)"""
    def prepare(pkg, orc):
        return {"A": orc.rand_matrix(m, n, 12), "b": orc.rand_vector(m, 13)}

    def call(pkg, ctx, inp):
        with _as_default(pkg, ctx):
            try:
                H = pkg.qr_(np.asfortranarray(inp["A"].copy()), nb=nb)
                x = pkg.ldiv(H, inp["b"])
            except pkg._lib.DHQRError as e:
                _raise_if_gave_up(e)
        return {"factor": H.A, "alpha": H.α, "x": x}

    def judge(orc, out):
        _judge_factor(orc, out, m, n, 12)
        Ho, ao = _oracle(orc, m, n, 12)
        _judge_x(out["x"], orc.solve(Ho, ao, orc.rand_vector(m, 13)))

    return Route(id, prepare, call, judge, bounded=True)  # nb = 0: the lead pipeline; the solve's Q'b and back substitution


_QUADS = {"DHQR_QUAD_MIN_COLS": "0", "DHQR_TUNE": "tn_min_tiles=3"}  # test_blocked_quads_and_stream_k_on_guarded_layouts
ROUTES = [
    # blocked Float64: the pair driver (conftest.py: DHQR_PAIR_MIN_N=512) with the look-ahead lane; seed 4 of test_blocked_vs_oracle
    _factor_f64(2050, 1030, 128, 4, "blocked_2050x1030", busy=True),
    _factor_f64(1281, 896, 128, 4, "blocked_1281x896", busy=True),
    _factor_f64(4096, 4096, 128, 4, "blocked_quads_stream_k_4096", env=_QUADS, busy=True),
    _spmd_one_rank("cs", 1300, 1290, 8, "column_cyclic_1300x1290"),
    _spmd_one_rank("rs", 4097, 300, 41, "row_split_4097x300"),
    # unblocked: the lead pipeline on flags (seed 7 of test_unblocked_lead_one_workgroup_or_pipelined)
    _factor_f64(8192, 40, 0, 7, "unblocked_8192x40", bounded=True),
    _factor_f64(2100, 300, 0, 7, "unblocked_2100x300", bounded=True),
    _factor_f64(8192, 40, 0, 7, "unblocked_8192x40_pipe0", env={"DHQR_RANKK_PIPE": "0"}, bounded=True),
    _factor_f64(2100, 300, 0, 7, "unblocked_2100x300_pipe0", env={"DHQR_RANKK_PIPE": "0"}, bounded=True),
    _small_route(220, 200, "small_flags_220x200"),
    _small_route(110, 100, "small_barrier_110x100"),
    _batched(16, 8, 1001, "batched_16x8x1001", busy=True),
    _batched(64, 32, 301, "batched_64x32x301", busy=True),
    _batched(110, 100, 37, "batched_110x100x37", busy=False),
] + [_solve(m, n, mode, f"solve_{mode}_{m}x{n}") for m, n in ((1100, 1000), (777, 130)) for mode in ("kept_t", "gram", "persistent")] + [
    _complex(1100, 1000, 0, "complex_1100x1000_nb0"),
    _complex(1100, 1000, 64, "complex_1100x1000_nb64"),
    _mg("cs", 2, 1500, 1300, "mg_column_2x1500x1300", busy=True),
    _mg("cs", 3, 2000, 1700, "mg_column_3x2000x1700", busy=True),
    _mg("rs", 2, 6000, 512, "mg_row_2x6000x512"),
    _mg("rs", 3, 3000, 1100, "mg_row_3x3000x1100"),
    _mg_complex(2, 300, 200, "mg_complex_column_2x300x200"),
] + [_host(m, n, nb, f"host_{m}x{n}_nb{nb}") for m, n in ((1100, 1000), (2207, 2000)) for nb in (0, 128)]
BY_ID = {r.id: r for r in ROUTES}


def _close(h):
    h.close()


def _setenv(monkeypatch, route, **extra):
    for k, v in {**route.env, **extra}.items():
        monkeypatch.setenv(k, v)


# --------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("route", ROUTES, ids=[r.id for r in ROUTES])
def test_repeat_is_bit_identical(pkg, orc, monkeypatch, route):
    """four calls from the same input on one context (or handle) and one on a fresh one: five equal byte sets; the first
    is judged against the oracle with the tolerance of the route's own test, so that a reproducible wrong answer does
    not pass.  Routes with bounded inter-workgroup waits may report the outcome include/dhqr.h documents (NaN in every
    alpha, the pipeline error of dhqr_synchronize, a solve repeated by the library): such a repetition is printed and set
    aside, two of them in one case fail it; nothing else is excused."""
    _setenv(monkeypatch, route)
    inp = route.prepare(pkg, orc)
    runs, aside = [], []
    handles = [route.open(pkg)]
    try:
        for rep in range(5):
            if rep == 4:
                handles.append(route.open(pkg))
            try:
                runs.append((rep, _run(route, handles[-1], inp, pkg)))
            except GaveUp as e:
                if not route.bounded:
                    raise
                print(f"[{route.id}] repetition {rep} set aside: {e}")
                aside.append(rep)
    finally:
        for h in handles:
            _close(h)
    print(f"[{route.id}] repetitions set aside: {len(aside)}")
    assert len(aside) <= 1, f"{len(aside)} of 5 repetitions gave up on a bounded wait: {aside}"
    route.judge(orc, _arrays(route, runs[0][1]))
    for rep, raw in runs[1:]:
        msg = _diff(route, runs[0][1], raw)
        assert msg is None, f"repetition {runs[0][0]} against repetition {rep}{' (fresh context)' if rep == 4 else ''}: {msg}"


_BUSY = [r for r in ROUTES if r.busy]


@pytest.mark.parametrize("route", _BUSY, ids=[r.id for r in _BUSY])
def test_result_does_not_depend_on_a_busy_device(pkg, orc, monkeypatch, route):
    """routes without a bounded inter-workgroup wait: the same bytes on an idle device and while a second torch stream
    works through a queue of 1024 x 1024 float64 matrix products enqueued before the call (twice the call's idle time worth
    of them, between 8 and 2000)"""
    import torch
    _setenv(monkeypatch, route)
    inp = route.prepare(pkg, orc)
    h = route.open(pkg)
    try:
        _run(route, h, inp, pkg)  # allocations, module loading
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        idle = _run(route, h, inp, pkg)
        e1.record()
        torch.cuda.synchronize()
        t_call = e0.elapsed_time(e1)
        X = torch.rand(1024, 1024, dtype=torch.float64, device=DEV)
        Y, Z = X.clone(), torch.empty_like(X)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.mm(X, Y, out=Z)
            e0.record()
            torch.mm(X, Y, out=Z)
            e1.record()
        torch.cuda.synchronize()
        t_mm = e0.elapsed_time(e1)
        count = int(min(2000, max(8, 2.0 * t_call / max(t_mm, 1e-3))))
        print(f"[{route.id}] idle call {t_call:.3f} ms, one 1024^3 float64 product {t_mm:.3f} ms -> {count} products queued")
        with torch.cuda.stream(side):
            for _ in range(count):
                torch.mm(X, Y, out=Z)
        loaded = _run(route, h, inp, pkg)
        torch.cuda.synchronize()
    finally:
        _close(h)
    msg = _diff(route, idle, loaded)
    assert msg is None, f"idle device against busy device: {msg}"


# does the serial schedule run the same kernels in the same order as the concurrent one?
#   blocked Float64: NO.  Without look-ahead dhqr_factor_f64 takes factor_blocked_simple (one 128-column panel per step, K =
#     128 updates) instead of cs_factor's pairs (K = 256 updates, cross term): another grouping of the same sums.
#   row split: dhqr_rowsplit.h runs "both roles on the caller's stream and one channel, in the same order".
#   ComplexF64 nb = 64: NO.  The lane applies panel k to the 64 columns of panel k + 1 in a launch of its own and the caller's
#     stream to the rest, where the serial loop issues ONE panel_apply over all trailing columns; the split of the V'C
#     sums over row slabs is picked per launch from its column count (pick_split), so the same sums are grouped differently.
_SERIAL = [("blocked_2050x1030", False), ("blocked_1281x896", False), ("row_split_4097x300", True), ("complex_1100x1000_nb64", False)]


@pytest.mark.parametrize("rid,same_bits", _SERIAL, ids=[r for r, _ in _SERIAL])
def test_serial_schedule(pkg, orc, monkeypatch, rid, same_bits):
    """DHQR_LOOKAHEAD=0 (read by dhqr_create): the serial schedule is the control of the concurrent one.  Against the oracle
    at the route's tolerance; bit for bit against the look-ahead result where both run the same kernels in the same order
    (the row split).  The blocked Float64 driver legitimately differs: without look-ahead it is factor_blocked_simple,
    single panels with K = 128 trailing updates, where the look-ahead driver groups panels in pairs (K = 256 updates and
    a cross term).  The blocked ComplexF64 driver differs too: its lane updates the next panel's 64 columns in a launch
    of its own, and the row-slab split of the V'C sums is picked per launch from the column count.  The same sums in
    another grouping: there the oracle is the assertion and the bit comparison is printed."""
    route = BY_ID[rid]
    _setenv(monkeypatch, route)
    inp = route.prepare(pkg, orc)
    res = {}
    for la in ("1", "0"):
        monkeypatch.setenv("DHQR_LOOKAHEAD", la)
        h = route.open(pkg)
        try:
            res[la] = _run(route, h, inp, pkg)
        finally:
            _close(h)
    route.judge(orc, _arrays(route, res["0"]))
    msg = _diff(route, res["1"], res["0"])
    print(f"[{rid}] look-ahead against serial: {'bit-identical' if msg is None else msg}")
    if same_bits:
        assert msg is None, f"look-ahead against serial schedule: {msg}"


@pytest.fixture(scope="module")
def hostio_children(pkg):
    """the two children of test_staged_host_io_equals_plain, run once: DHQR_HOSTIO is read once per process, so one child per
    setting (tests/helpers/schedule_child.py, case list "gpu"), one after the other, nothing started after a failed one"""
    t0 = time.time()
    res = run_hostio_children(pkg._lib.SO_PATH, "gpu", timeout=300)
    print(f"two children: {time.time() - t0:.1f} s for {sum(len(r['calls']) for r in res[0].values())} calls each")
    return res


@pytest.mark.parametrize("case", hostio_case_names("gpu"))
def test_staged_host_io_equals_plain(hostio_children, case):
    """DHQR_HOSTIO=1 (csrc/dhqr_hostio.h: column blocks downloaded behind their panel's commit event through four rotating
    pinned buffers on two copy streams) against the plain three-phase form.  The staged form factors the same device copy
    with the same dhqr_factor_f64, so hA, halpha and hx are bit-identical, hb is unchanged, the guards around a padded host
    matrix survive, and a rejected panel (n_fallback >= 1 in both children) takes everything again."""
    # 1e-9 relative: the bound on x of test_host_entry_points_on_guarded_layouts
    compare_hostio(*hostio_children, x_tol=1e-9, only=case)
