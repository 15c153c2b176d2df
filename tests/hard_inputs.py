"""Test-only helpers of the hard-input tests of the small-matrix kernels (test_gpu_hard_inputs.py on the MI355X,
test_emulated_hard_inputs.py on the CPU): matrices that are signed, scaled towards the ends of the exponent range, graded by
column and by row, nearly of rank one, triangular, and with a zero pivot / a zero column -- all built on the host from the
oracle's generator, so the kernel under test and the oracle see identical bits -- and the criteria C1-C6 both files apply.

A test hands over a `backend`: three functions on host arrays, however it runs them (api.py on device tensors, the C ABI of
the emulated library):
    backend.factor(A)         A (batch, m, n)            -> (H (batch, m, n), alpha (batch, n)), A untouched
    backend.solve(H, al, b)   b (batch, m)               -> x (batch, n)
    backend.solve(H, al, B)   B (batch, m, nrhs)         -> X (batch, n, nrhs)
Every criterion is evaluated on the reference first (Float64: the oracle's own factor and solve; Float32: the numpy twin of
f32_helpers), then on the kernel's result.  The product never imports this file."""
import numpy as np

import f32_helpers as F

LD = np.longdouble
# 32 x 32 in Float32: alpha's error is driven by the condition number of a square matrix (its last pivot), and over 64 matrices
# the numpy twin itself misses C1 at most seeds (4100: 1.74 of the bound; test_gpu_f32.py tells the same of its seed).  5700
# was chosen with the twin alone, on the CPU (0.31 of the bound over 64 matrices); every shape and class uses it.
SEED = 5700
WELL = ("signed", "big", "tiny", "triangular")                         # forward error of the solve is judged (C1, C3)
RESIDUAL = ("colgraded", "rowgraded_down", "rowgraded_up", "lowrank")  # kappa governs the forward error: the residual is judged
CLASSES = WELL + RESIDUAL + ("degenerate",)
NP = {"f64": np.float64, "f32": np.float32}
EXP = {"f64": 500, "f32": 100}      # big / tiny: S 2^(+-e)
LOWRANK_P = {"f64": 40, "f32": 12}  # lowrank: outer(u1, u2) + 2^-p S
GRADE_BUDGET = {"f64": 380, "f32": 90}


def eps(t):
    return float(np.finfo(NP[t]).eps)


def tol(n, t):
    """8 max(n, 8) eps: the expression of the batched and the Float32 tests"""
    return 8.0 * max(n, 8) * eps(t)


def signed_matrix(orc, m, n, seed):
    return 2.0 * orc.rand_matrix(m, n, seed) - 1.0  # exact in Float64


def grade(n, t):
    return min(3, GRADE_BUDGET[t] // n)


def make(orc, cls, m, n, batch, t, seed=SEED):
    """(A (batch, m, n), b (batch, m)) of class `cls` in dtype t: Float64 values, rounded once for Float32"""
    A = np.empty((batch, m, n))
    b = np.empty((batch, m))
    e = EXP[t]
    for k in range(batch):
        S = signed_matrix(orc, m, n, seed + k)
        b[k] = 2.0 * orc.rand_vector(m, seed + 5000 + k) - 1.0
        if cls in ("signed", "degenerate"):
            M = S
        elif cls == "big":
            M = np.ldexp(S, e)
        elif cls == "tiny":
            M = np.ldexp(S, -e)
        elif cls == "colgraded":
            M = S * np.ldexp(1.0, -grade(n, t) * np.arange(n))[None, :]
        elif cls in ("rowgraded_down", "rowgraded_up"):
            sc = np.ldexp(1.0, -((40 * np.arange(m)) // m))
            M = S * (sc if cls == "rowgraded_down" else sc[::-1])[:, None]
        elif cls == "lowrank":
            u1, u2 = orc.rand_vector(m, seed + 9000 + k), orc.rand_vector(n, seed + 13000 + k)
            M = np.outer(u1, u2) + np.ldexp(S, -LOWRANK_P[t])
        elif cls == "triangular":  # triu(S_k); the last matrix of the batch is the m x n identity
            M = np.eye(m, n) if k == batch - 1 else np.triu(S)
        else:
            raise ValueError(cls)
        A[k] = M
    if cls == "degenerate":
        assert batch >= 4
        A[1, 0, 0] = 0.0       # zero pivot, non-zero column
        if n >= 4:
            A[2, :, 2] = 0.0   # all-zero column: alpha[2] = 0, NaN behind it, as the reference does
    return A.astype(NP[t]), b.astype(NP[t])


# ---------------------------------------------------------------------------------------------- the reference
def ref_factor(orc, A, t):
    """Float64: the oracle; Float32: the numpy twin (float storage, double sums)"""
    if t == "f64":
        return orc.householder(np.asfortranarray(A))
    with np.errstate(all="ignore"):
        return F.twin_factor(A)


def ref_solve(orc, H, al, b, t):
    if t == "f64":
        return orc.solve(np.asfortranarray(H), np.ascontiguousarray(al), b)
    with np.errstate(all="ignore"):
        return F.twin_solve(H, al, b)[:H.shape[1]]


def oracle64(orc, A):
    """the Float64 oracle's factor of the (widened) input: what C1 compares with"""
    with np.errstate(all="ignore"):
        return orc.householder(np.asfortranarray(A, dtype=np.float64))


# ---------------------------------------------------------------------------------------------- criteria, one matrix
def c1(Ho, ao, H, al, t, ncols=None):
    """element-wise against the oracle, as ratios to tol: |H - Ho| / max|Ho| and (Float64) |alpha - alphao| / max|Ho| or
    (Float32) |alpha - alphao| / |alphao|; and, because V does not scale with the matrix while R does, the same with V judged
    against max|Vo| and R against max|Ro| (for a matrix of magnitude one the two forms agree up to a small factor)"""
    n = Ho.shape[1]
    nc = n if ncols is None else ncols
    H, al, Ho, ao = H[:, :nc].astype(np.float64), al[:nc].astype(np.float64), Ho[:, :nc], ao[:nc]
    T = tol(n, t)
    scale = np.abs(Ho).max()
    eH = np.abs(H - Ho).max() / scale
    if t == "f64":
        ea = np.abs(al - ao).max() / scale
    else:
        ea = (np.abs(al - ao) / np.where(ao == 0.0, 1.0, np.abs(ao))).max()
    low = np.tril(np.ones(Ho.shape, bool))
    Rs = max(np.abs(np.where(low, 0.0, Ho)).max(), np.abs(ao).max())
    eV = np.abs(np.where(low, H - Ho, 0.0)).max() / np.abs(np.where(low, Ho, 0.0)).max()
    eR = max(np.abs(np.where(low, 0.0, H - Ho)).max(), np.abs(al - ao).max()) / Rs
    return max(eH, ea, eV, eR) / T


def form_qr_ld(H, al):
    """Q R in long double from a factor (H, alpha): Q = H_0 ... H_{n-1}, H_j = I - v_j v_j'"""
    m, n = H.shape
    V = H.astype(LD)
    B = np.zeros((m, n), dtype=LD)
    B[:n] = np.triu(V[:n], 1)
    B[np.arange(n), np.arange(n)] = al.astype(LD)
    for j in range(n - 1, -1, -1):  # rows >= j, columns >= j: the rest is still zero / untouched
        v = V[j:, j]
        B[j:, j:] -= np.outer(v, v @ B[j:, j:])
    return B


def c2(A, H, al, t):
    """column-wise backward error max_j ||(QR - A)[:, j]|| / ||A[:, j]|| against tol and max_j | ||v_j||^2 - 2 | against 2 tol"""
    n = A.shape[1]
    T = tol(n, t)
    Al = A.astype(LD)
    D = form_qr_ld(H, al) - Al
    cn = np.sqrt((Al * Al).sum(axis=0))
    be = float((np.sqrt((D * D).sum(axis=0)) / cn).max())
    V = np.tril(H.astype(LD))
    ev = float(np.abs((V * V).sum(axis=0) - 2).max())
    return max(be / T, ev / (2 * T))


def c3_forward(xo, x, t):
    """Float64: |x - xo|_inf / |xo|_inf against 1e-9 (the existing bound)"""
    return float(np.abs(x.astype(np.float64) - xo).max() / np.abs(xo).max()) / 1e-9


def c3_f32(orc, H, al, b, x):
    """Float32 (f32_helpers.check_solve): x against the Float64 oracle's solve applied to the kernel's OWN factor, 4 eps32"""
    xo = orc.solve(np.asfortranarray(H.astype(np.float64)), al.astype(np.float64), b.astype(np.float64))
    return float(np.abs(x.astype(np.float64) - xo).max() / np.abs(xo).max()) / (4 * F.EPS32)


def c3_residual(H, al, b, x, t):
    """component-wise residual of the triangular system the factor defines: y = Q'b in long double from the factor itself,
    max_i |R x - y[:n]|_i / ((|R||x|)_i + ||b||_2) against tol"""
    m, n = H.shape
    V = H.astype(LD)
    y = b.astype(LD)
    for j in range(n):
        v = V[j:, j]
        y[j:] -= v * (v @ y[j:])
    R = np.triu(V[:n], 1)
    R[np.arange(n), np.arange(n)] = al.astype(LD)
    xl = x.astype(LD)
    num = np.abs(R @ xl - y[:n])
    den = np.abs(R) @ np.abs(xl) + np.sqrt((b.astype(LD) ** 2).sum())
    return float((num / den).max()) / tol(n, t)


def same(a, b):
    """bit for bit, a NaN equal to a NaN (the columns behind a zero column), -0 equal to 0"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=True))


# ---------------------------------------------------------------------------------------------- a whole class
class Result:
    def __init__(self, A, b, H, al, x):
        self.A, self.b, self.H, self.al, self.x = A, b, H, al, x


def run(backend, A, b):
    H, al = backend.factor(A)
    return Result(A, b, H, al, backend.solve(H, al, b))


def check_class(backend, orc, cls, m, n, batch, t, what, seed=SEED):
    """C1-C5 as they apply to `cls` on every matrix of a batch.  Returns the Result (C6 compares it with a mixed batch)."""
    A, b = make(orc, cls, m, n, batch, t, seed)
    r = run(backend, A, b)
    assert r.H.dtype == A.dtype and r.H.shape == A.shape and r.al.shape == (batch, n) and r.x.shape == (batch, n)
    ks = range(batch)
    zero_col = cls == "degenerate" and n >= 4
    ref = {"C1": 0.0, "C2": 0.0, "C3": 0.0}
    ker = dict(ref)

    def worse(d, key, v):
        d[key] = max(d[key], v) if np.isfinite(v) and np.isfinite(d[key]) else np.inf

    for k in ks:
        Ho, ao = oracle64(orc, A[k])
        Hr, ar = ref_factor(orc, A[k], t)
        if zero_col and k == 2:
            # C5: alpha[2] = 0 and NaN behind it; NaN exactly where the reference has it -- rows >= 2 of the columns >= 2 -- and
            # everything else (the columns before the zero column, the rows of R above it) under C1; x non-finite
            nan = np.isnan(Ho)
            assert ao[2] == 0.0 and np.isnan(ao[3:]).all() and nan[2:, 2:].all() and not nan[:, :2].any() and not nan[:2].any(), "the oracle"
            assert r.al[k][2] == 0.0 and np.isnan(r.al[k][3:]).all(), f"{what}: alpha behind the zero column {r.al[k]}"
            assert np.array_equal(np.isnan(Hr), nan), "the reference's own NaN pattern: change the input"
            assert np.array_equal(np.isnan(r.H[k]), nan), \
                f"{what} {m}x{n} {t}: behind a zero column the NaN differ from the reference's (rows >= 2 of columns >= 2, nothing else) at (row, column) {np.argwhere(np.isnan(r.H[k]) != nan)[:6].tolist()}"
            z = lambda a: np.where(np.isnan(a), 0.0, a).astype(a.dtype)  # (the finite entries: NaN -> 0 on both sides)
            worse(ref, "C1", c1(z(Ho), z(ao), z(Hr), z(ar), t))
            worse(ker, "C1", c1(z(Ho), z(ao), z(r.H[k]), z(r.al[k]), t))
            assert not np.isfinite(r.x[k]).all(), f"{what}: x of the zero-column matrix is finite"
            continue
        if cls == "degenerate" and k == 1:
            # C5: alpha[0] = -0 s = 0 as in the reference: its factor under C1, x[0] = b[0] / 0.  With h = 0 the reference's v_0 =
            # a_0 / s has norm 1, not sqrt 2: I - v v' is a projector, the columns behind lose one dimension, and for m = n the
            # LAST pivot is the rounding noise of a singular block -- in the oracle too (a plain-double twin differs from it by
            # O(1) there).  So a square matrix is judged on its first n - 1 columns, and x -- the solution of a system with
            # that pivot -- on its pattern: x[0] is not finite, the rest is.
            nc = n - 1 if m == n else n
            assert ao[0] == 0.0, "the oracle"
            assert r.al[k][0] == 0.0 and np.isfinite(r.H[k]).all() and np.isfinite(r.al[k]).all(), \
                f"{what} {m}x{n} {t}: zero pivot: alpha[0] = {r.al[k][0]!r}, the reference's -sign(0) s = 0"
            worse(ref, "C1", c1(Ho, ao, Hr, ar, t, ncols=nc))
            worse(ker, "C1", c1(Ho, ao, r.H[k], r.al[k], t, ncols=nc))
            assert not np.isfinite(r.x[k][0]) and np.isfinite(r.x[k][1:]).all(), f"{what}: x of the zero-pivot matrix {r.x[k]}"
            continue
        assert np.isfinite(Ho).all() and np.isfinite(ao).all(), "the reference is not finite here: change the input"
        assert np.isfinite(r.H[k]).all() and np.isfinite(r.al[k]).all() and np.isfinite(r.x[k]).all(), f"{what}: matrix {k} not finite"
        if cls in WELL or cls == "degenerate":
            worse(ref, "C1", c1(Ho, ao, Hr, ar, t))
            worse(ker, "C1", c1(Ho, ao, r.H[k], r.al[k], t))
        worse(ref, "C2", c2(A[k], Hr, ar, t))
        worse(ker, "C2", c2(A[k], r.H[k], r.al[k], t))
        xr = ref_solve(orc, Hr, ar, b[k], t)
        if cls in RESIDUAL:
            worse(ref, "C3", c3_residual(Hr, ar, b[k], xr, t))
            worse(ker, "C3", c3_residual(r.H[k], r.al[k], b[k], r.x[k], t))
        elif t == "f64":
            worse(ref, "C3", 0.0)  # (the oracle against itself)
            worse(ker, "C3", c3_forward(xr, r.x[k], t))
        else:
            worse(ref, "C3", c3_f32(orc, Hr, ar, b[k], xr))
            worse(ker, "C3", c3_f32(orc, r.H[k], r.al[k], b[k], r.x[k]))
    # C4: odd symmetry, bit for bit, on the whole batch
    rn = run(backend, -A, b)
    odd = {"factor(-A) H": same(rn.H, -r.H), "factor(-A) alpha": same(rn.al, -r.al), "solve(-A, b)": same(rn.x, -r.x),
           "solve(A, -b)": same(backend.solve(r.H, r.al, -b), -r.x)}
    print(f"{what} {t} {m}x{n} {cls}: {len(ks)} of {batch} matrices, worst ratio to the bound, reference | kernel: "
          + " ".join(f"{c} {ref[c]:.3f} | {ker[c]:.3f}" for c in ("C1", "C2", "C3")) + f" C4 {'odd' if all(odd.values()) else 'NOT ODD'}")
    for c in ("C1", "C2", "C3"):
        assert ref[c] <= 1.0, f"{c}: the reference misses the bound here: change the input ({ref[c]:.3f})"
    for c in ("C1", "C2", "C3"):
        assert ker[c] <= 1.0, f"{what} {cls} {m}x{n} {t}: {c} at {ker[c]:.3f} of its bound (reference {ref[c]:.3f})"
    assert all(odd.values()), f"{what} {cls} {m}x{n} {t}: not odd in its data: {[k for k, v in odd.items() if not v]}"
    return r


def check_degenerate_neighbours(backend, orc, m, n, batch, t, what, r, seed=SEED):
    """C5: every matrix but 1 and 2 of the degenerate batch has the bits of the `signed` batch (the same matrices without the
    degenerate ones); matrices 0 and 3 share the workgroup of 1 and 2 on the wave tier"""
    A, b = make(orc, "signed", m, n, batch, t, seed)
    s = run(backend, A, b)
    keep = [k for k in range(batch) if k not in (1, 2)]
    assert same(r.H[keep], s.H[keep]) and same(r.al[keep], s.al[keep]) and same(r.x[keep], s.x[keep]), \
        f"{what}: a degenerate matrix disturbed a neighbour in its batch"
    if n < 4:  # (no zero column at this shape: matrix 2 is untouched too)
        assert same(r.H[2], s.H[2]) and same(r.x[2], s.x[2])


def check_mixed(backend, orc, m, n, t, what, results, seed=SEED):
    """C6: one batch interleaves all classes (matrix i of the mixed batch = matrix i // len(classes) of class i % len(classes)),
    so scales 2^e and 2^-e sit in neighbouring waves: H, alpha, x bit-identical to the batch of the matrix's own class"""
    classes = list(results)
    per = min(len(results[c].A) for c in classes)
    idx = [(c, i) for i in range(per) for c in classes]
    A = np.stack([results[c].A[i] for c, i in idx])
    b = np.stack([results[c].b[i] for c, i in idx])
    r = run(backend, A, b)
    bad = [(c, i) for q, (c, i) in enumerate(idx)
           if not (same(r.H[q], results[c].H[i]) and same(r.al[q], results[c].al[i]) and same(r.x[q], results[c].x[i]))]
    print(f"{what} {t} {m}x{n} mixed batch of {len(idx)}: {len(bad)} matrices differ from their own class's batch")
    assert not bad, f"{what}: (class, matrix) that depend on their neighbours in the batch: {bad[:8]}"


def check_nrhs(backend, orc, cls, m, n, batch, K, t, what, seed=SEED):
    """several right-hand sides on a hard class: column r of solve(H, B) has the bits of solve(H, B[..., r]); odd in B"""
    A, b = make(orc, cls, m, n, batch, t, seed)
    B = np.stack([make(orc, "signed", m, 1, batch, t, seed + 1000 * r)[1] for r in range(K)], axis=2)  # column r: b of seed + 1000 r
    assert same(np.ascontiguousarray(B[:, :, 0]), b)
    H, al = backend.factor(A)
    X = backend.solve(H, al, B)
    assert X.shape == (batch, n, K)
    for r in range(K):
        xr = backend.solve(H, al, np.ascontiguousarray(B[:, :, r]))
        assert same(np.ascontiguousarray(X[:, :, r]), xr), f"{what} {cls} {m}x{n} {t}: column {r} differs from the single-column call"
    assert same(backend.solve(H, al, -B), -X), f"{what} {cls} {m}x{n} {t}: H \\ B is not odd in B"
    print(f"{what} {t} {m}x{n} {cls}: {K} columns x {batch} matrices: every column the single-column call's bits, odd in B")


# ---------------------------------------------------------------------------------------------- the 1 x 1 sweep
def sweep_inputs(orc, count, t, seed=SEED):
    """a_k = +-(1 + u_k) 2^e_k, e_k stepping evenly through [-E, E] (E = 500, Float32 120); b_k = +-(1 + u'_k), so that
    x = b / a is a normal number of the type throughout (Float32: 2^-122 < |x| < 2^122)"""
    E = 500 if t == "f64" else 120
    u, w = orc.rand_vector(count, seed), orc.rand_vector(count, seed + 1)
    sa = np.where(orc.rand_vector(count, seed + 2) < 0.5, -1.0, 1.0)
    sb = np.where(orc.rand_vector(count, seed + 3) < 0.5, -1.0, 1.0)
    e = np.round(np.linspace(-E, E, count)).astype(np.int64)
    a = (np.ldexp(sa * (1.0 + u), e)).astype(NP[t])
    b = (sb * (1.0 + w)).astype(NP[t])
    assert e[0] == -E and e[-1] == E and np.isfinite(a).all()
    return a.reshape(count, 1, 1), b.reshape(count, 1)


def check_sweep(backend, orc, count, t, what):
    """a batch of 1 x 1 matrices: s2 = a^2, alpha = -a, v = +-sqrt(2), x = b / a -- the square root / reciprocal square root
    and the reciprocal-and-correct division swept over the exponent range in one launch"""
    A, b = sweep_inputs(orc, count, t)
    r = run(backend, A, b)
    a, al, v, x = A[:, 0, 0].astype(LD), r.al[:, 0].astype(LD), r.H[:, 0, 0].astype(LD), r.x[:, 0].astype(LD)
    q = b[:, 0].astype(LD) / a
    E, T = eps(t), tol(1, t)
    assert np.isfinite(r.al).all() and np.isfinite(r.H).all() and np.isfinite(r.x).all()
    ea = np.abs(al + a) / np.abs(a)
    ev = np.abs(v * v - 2)
    ex = np.abs(x - q) / np.abs(q)
    ulp_a = float((np.abs(al + a) / np.spacing(np.abs(A[:, 0, 0])).astype(LD)).max())
    ulp_x = float((np.abs(x - q) / np.spacing(np.abs(r.x[:, 0])).astype(LD)).max())
    inexact = int((r.al[:, 0] != -A[:, 0, 0]).sum())
    print(f"{what} {t} 1x1 sweep of {count}: ratio to the bound alpha {float(ea.max()) / (2 * E):.3f} v^2 {float(ev.max()) / (2 * T):.3f} "
          f"x {float(ex.max()) / T:.3f}; worst error alpha {ulp_a:.2f} ulp, x {ulp_x:.2f} ulp; alpha != -a in {inexact} entries")
    assert same(np.sign(r.H[:, 0, 0]), np.sign(A[:, 0, 0])), "v = (a - alpha) f has the sign of a"
    k = int(np.argmax(ea))
    assert ea[k] <= 2 * E, f"alpha of a = {A[k, 0, 0]!r}: {r.al[k, 0]!r}"
    k = int(np.argmax(ev))
    assert ev[k] <= 2 * T, f"v of a = {A[k, 0, 0]!r}: {r.H[k, 0, 0]!r}"
    k = int(np.argmax(ex))
    assert ex[k] <= T, f"x of a = {A[k, 0, 0]!r}, b = {b[k, 0]!r}: {r.x[k, 0]!r}"
