"""Test-only helpers of the hard-input tests of the ComplexF64 small-matrix kernels (test_gpu_zhard_inputs.py on the MI355X,
test_emulated_zhard_inputs.py on the CPU): the complex counterpart of hard_inputs.py.  Matrices with signed parts, scaled to
2^+-500, with parts of very different size, with a part identically zero away from magnitude one, graded by column and by
row, nearly of rank one, triangular, with a zero pivot / a zero column -- all built on the host from the oracle's generator by
exact operations (2 u - 1 on the parts, np.ldexp on the parts), so the kernel under test and the oracle see identical bits --
and the criteria Z1-Z6 both files apply.

A test hands over a `backend`: functions on host arrays, however it runs them (api.py on device tensors, the C ABI of the
emulated library):
    backend.factor(A)                  A (batch, m, n)       -> (H (batch, m, n), alpha (batch, n)), A untouched
    backend.solve(H, al, b)            b (batch, m)          -> x (batch, n)
    backend.solve(H, al, B)            B (batch, m, K)       -> X (batch, n, K)
    backend.solve_full(H, al, b)       b (batch, m)          -> (x (batch, n), rows n .. m-1 of Q^H b (batch, m - n))
    backend.apply_q(H, al, B, trans)   B (batch, m, K)       -> Q^H B (trans) or Q B, (batch, m, K)
    backend.form_q(H, al) -> (batch, m, n)                   backend.form_r(H, al) -> (batch, n, n)
Every criterion is evaluated on the reference first -- the oracle (orc.householder_c / orc.solve_c), and where a criterion
compares WITH the oracle, the oracle's plain-numpy restatement (orc.householder_c_np / orc.solve_c_np) against it -- and the
reference missing a bound is reported as "change the input", never as a failure of the kernel.  The product never imports
this file.

THE BOUNDS are the project's: T = 8 max(n, 8) eps (zbatched_helpers.T = hard_inputs.tol(n, "f64"));
Z1  H and alpha element-wise against the oracle relative to max|H| under the rule of zbatched_helpers (no matrix above 8 T;
    one of a batch of <= 9 above T, 1 % of a larger one) -- where the oracle is a measure of H.  The reference forms the phase of
    alpha as -exp(i angle(h)): near 0, pi and +-pi/2 the rounded angle leaves an ABSOLUTE error of 1e-16 in the small part of
    the phase, and that error grows with every column by the ratio of column norm to pivot.  With parts 2^60 apart the
    oracle is up to 800 T (batches of 64 up to 64 x 32) and 185 000 T (128 x 128) from a long-double factor, and its numpy
    restatement, which goes through the angle too, goes with it; the kernels form -h / |h|, accurate in each part, and stay
    within 0.1 T of the long-double factor.  So the reference is evaluated first with TWO restatements, the second forming
    the phase by division (restated), and where the kernel misses the rule against the oracle AND the oracle's own
    restatements do, the kernel is judged under the same rule against the long-double restatement (check_class prints
    which).  That restatement forms the phase the way the kernels do: what is independent of them in the fallback is the
    long-double arithmetic and the plain order of the sums, not the formulation;
Z2  max_j ||(QR - A)[:, j]|| / ||A[:, j]|| <= T with QR formed in np.clongdouble, max_j | ||v_j||^2 - 2 | <= 2 T;
Z3  |x - xo|_inf / |xo|_inf <= 1e-9, or (rowgraded_up, lowrank: the condition number governs the forward error) the
    component-wise residual of the triangular system the kernel's own factor defines, <= T; for m > n the rows n .. m-1 of
    Q^H b within 1e-12 max(1, |Q^H b|_inf) (test_emulated_batched_complex.py) of those of the oracle's factor -- of the
    restatement in np.clongdouble where the oracle's restatements miss that themselves -- and, in rowgraded_up and lowrank,
    where the tail is as sensitive as x (the reference's own restatements are up to 8e9 times the bound apart), of Q^H b
    formed in np.clongdouble from the kernel's own factor;
Z4  bit for bit: factor(-A) = (-H, -alpha), solve(-A, b) = (-x, the same tail), solve(A, -b) = -(x, tail),
    factor(conj A) = (conj H, conj alpha), solve(conj A, conj b) = conj x; factor(i A) = i factor(A) only within T of max|H|
    (the order of the fma chains changes), for every matrix of Z1's classes and whatever the oracle makes of iA: a matrix
    that misses is judged as in Z1, both of its factors within T of the long-double restatement.  A matrix with a pivot of
    exactly zero is neither odd nor rotates: alphafactor(0) = -1 whatever the sign of the rest of the column -- it is left
    out of the negation and the rotation, not of the conjugation;
Z5  `degenerate`; Z6 a mixed batch (hard_inputs.check_mixed)."""
import numpy as np

import hard_inputs as HI
import zapplyq_helpers as Z
import zbatched_helpers as zh
from hard_inputs import same
from zbatched_helpers import T

LD, CLD = np.longdouble, np.clongdouble
EPS = zh.EPS
# one seed for every shape and class, chosen with the reference alone on the CPU.  Under Z1 a batch of 64 may have NO matrix
# above T, and of 95 seeds (100 .. 9000 in steps of 100, and 1 .. 3, 4100, 5700) none keeps the oracle and its two restatements
# inside the rule in the classes of magnitude one at every shape and batch of the two test files (the best miss it once).  2700
# does at all but 64 x 32 `signed` / `big` / `degenerate` (one matrix at 1.87 T), where its complex128 restatement is inside the
# rule against the long-double one (0.90 T); everywhere else the worst matrix is at 0.89 T or below.
SEED = 2700
Z1_CLASSES = ("signed", "big", "tiny", "re_heavy", "im_heavy", "real_only", "imag_only", "triangular")
FORWARD = Z1_CLASSES + ("colgraded", "rowgraded_down")  # the forward error of the solve is judged
RESIDUAL = ("rowgraded_up", "lowrank")                  # kappa governs the forward error: the residual is judged
CLASSES = FORWARD + RESIDUAL + ("degenerate",)
EXP, SKEW, LOWRANK_P = 500, 60, 40


def cplx(re, im):
    """re + i im without arithmetic (no -0 / NaN surprises of a complex product)"""
    out = np.empty(np.broadcast(re, im).shape, dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def signed(Zm):
    """(2 Re Z - 1) + i (2 Im Z - 1): exact in Float64"""
    return cplx(2.0 * Zm.real - 1.0, 2.0 * Zm.imag - 1.0)


def scaled(S, er, ei=None):
    return cplx(np.ldexp(S.real, er), np.ldexp(S.imag, er if ei is None else ei))


def times_i(X):
    """i X, exactly"""
    return cplx(-X.imag, X.real)


def make(orc, cls, m, n, batch, seed=SEED):
    """(A (batch, m, n), b (batch, m)) of class `cls`"""
    A = np.empty((batch, m, n), dtype=np.complex128)
    b = np.empty((batch, m), dtype=np.complex128)
    for k in range(batch):
        S = signed(orc.rand_matrix_c(m, n, seed + k))
        b[k] = signed(orc.rand_vector_c(m, seed + 5000 + k))
        if cls in ("signed", "degenerate"):
            M = S
        elif cls == "big":
            M = scaled(S, EXP)
        elif cls == "tiny":
            M = scaled(S, -EXP)
        elif cls == "re_heavy":
            M = scaled(S, 0, -SKEW)
        elif cls == "im_heavy":
            M = scaled(S, -SKEW, 0)
        elif cls == "real_only":
            M = cplx(np.ldexp(S.real, EXP), 0.0)
        elif cls == "imag_only":
            M = cplx(0.0, np.ldexp(S.imag, -EXP))
        elif cls == "colgraded":
            M = scaled(S, (-HI.grade(n, "f64") * np.arange(n))[None, :])
        elif cls in ("rowgraded_down", "rowgraded_up"):
            e = -((40 * np.arange(m)) // m)
            M = scaled(S, (e if cls == "rowgraded_down" else e[::-1])[:, None])
        elif cls == "lowrank":
            u1, u2 = orc.rand_vector_c(m, seed + 9000 + k), orc.rand_vector_c(n, seed + 13000 + k)
            M = np.outer(u1, u2) + scaled(S, -LOWRANK_P)
        elif cls == "triangular":  # triu(S_k); the last matrix of the batch is the m x n identity
            M = np.eye(m, n, dtype=np.complex128) if k == batch - 1 else np.triu(S)
        else:
            raise ValueError(cls)
        A[k] = M
    if cls == "degenerate":
        assert batch >= 4
        A[1, 0, 0] = 0.0       # zero pivot, non-zero column: alphafactor(0) = -1 (src:9)
        if n >= 4:
            A[2, :, 2] = 0.0   # all-zero column: alpha[2] = 0, non-finite behind it, as the reference does
    return A, b


# ---------------------------------------------------------------------------------------------- the reference
class one_thread:
    """the oracle runs its columns under OpenMP, and a team of threads costs a call on a 16 x 8 matrix a hundred times what the
    arithmetic does: the calls of this file run on one thread (the columns are independent, so the bits are the same) and
    leave the setting as they found it"""

    def __init__(self, orc):
        self.lib = orc.lib()

    def __enter__(self):
        self.old = self.lib.omp_get_max_threads()
        self.lib.omp_set_num_threads(1)

    def __exit__(self, *exc):
        self.lib.omp_set_num_threads(self.old)


def oracle(orc, A):
    with np.errstate(all="ignore"), one_thread(orc):
        return orc.householder_c(np.asfortranarray(A))


def oracle_solve(orc, H, al, b):
    with np.errstate(all="ignore"), one_thread(orc):
        return orc.solve_c(np.asfortranarray(H), al, b)


def twin(orc, A):
    """the oracle's plain-numpy restatement: what the Z1 / Z3 comparisons WITH the oracle are evaluated on first"""
    with np.errstate(all="ignore"):
        return orc.householder_c_np(np.asfortranarray(A))


def restated(A, dtype=np.complex128):
    """a second plain restatement of the reference's factor (src:9, 51-59, 122-148, 171-213), in complex128 or clongdouble,
    that forms the phase -exp(i angle(h)) as -h / |h| (csrc/dhqr_complex.h does it so).  The reference's own form goes through
    the angle, and near 0, pi and +-pi/2 the rounding of the angle leaves an absolute error of 1e-16 in the SMALL part of the
    phase where the quotient is accurate in each part: see check_class on what that does to Z1."""
    real = np.float64 if dtype == np.complex128 else LD
    H = np.array(A, dtype=dtype, order="F")
    m, n = H.shape
    alpha = np.zeros(n, dtype=dtype)
    with np.errstate(all="ignore"):
        for j in range(n):
            col = H[j:, j]
            s = real(np.sqrt(np.sum(col.real.astype(LD) ** 2 + col.imag.astype(LD) ** 2)))
            h = H[j, j]
            ah = np.hypot(h.real, h.imag)
            pr, pi = (-1.0, 0.0) if ah == 0 else (-h.real / ah, -h.imag / ah)  # angle(0) = 0
            alpha[j] = dtype(pr * s) + dtype(1j) * dtype(pi * s)
            f = 1 / np.sqrt(s * (s + ah))
            H[j, j] -= alpha[j]
            H[j:, j] *= f
            if j + 1 < n:
                v = H[j:, j].copy()
                H[j:, j + 1:] -= np.outer(v, np.conj(v) @ H[j:, j + 1:])
    return H, alpha


def twin_solve(orc, H, al, b):
    with np.errstate(all="ignore"):
        return orc.solve_c_np(H, al, b)


# ---------------------------------------------------------------------------------------------- criteria, one matrix
def unfinite(a):
    """non-finite entries -> 0"""
    return np.where(np.isfinite(a), a, 0.0).astype(a.dtype)


def form_qr_cld(H, al):
    """Q R in clongdouble from a factor (H, alpha): Q = H_0 ... H_{n-1}, H_j = I - v_j v_j^H"""
    m, n = H.shape
    V = H.astype(CLD)
    B = np.zeros((m, n), dtype=CLD)
    B[:n] = np.triu(V[:n], 1)
    B[np.arange(n), np.arange(n)] = al.astype(CLD)
    for j in range(n - 1, -1, -1):  # rows >= j, columns >= j: the rest is still zero / untouched
        v = V[j:, j]
        B[j:, j:] -= np.outer(v, np.conj(v) @ B[j:, j:])
    return B


def _abs2(X):
    return X.real * X.real + X.imag * X.imag  # (long double: 2^+-1000 is in range)


def z2(A, H, al):
    """(column-wise backward error / T, max_j | ||v_j||^2 - 2 | / 2 T)"""
    n = A.shape[1]
    Al = A.astype(CLD)
    D = form_qr_cld(H, al) - Al
    be = float((np.sqrt(_abs2(D).sum(axis=0)) / np.sqrt(_abs2(Al).sum(axis=0))).max())
    V = np.tril(H.astype(CLD))
    ev = float(np.abs(_abs2(V).sum(axis=0) - 2).max())
    return be / T(n), ev / (2 * T(n))


def qhb_cld(H, b):
    """Q^H b in clongdouble from the reflectors of a factor"""
    n = H.shape[1]
    V = H.astype(CLD)
    y = b.astype(CLD)
    for j in range(n):
        v = V[j:, j]
        y[j:] -= v * (np.conj(v) @ y[j:])
    return y


def qhb_plain(H, b):
    """Q^H b in plain complex128 (test_emulated_batched_complex.py forms it so)"""
    y = np.array(b, dtype=np.complex128)
    for j in range(H.shape[1]):
        y[j:] -= H[j:, j] * np.vdot(H[j:, j], y[j:])
    return y


def z3_forward(xo, x):
    return float(np.abs(x - xo).max() / np.abs(xo).max()) / 1e-9


def z3_residual(H, al, b, x):
    """the complex form of hard_inputs.c3_residual: y = Q^H b in long double from the factor itself,
    max_i |R x - y[:n]|_i / ((|R||x|)_i + ||b||_2) against T"""
    n = H.shape[1]
    y = qhb_cld(H, b)
    R = np.triu(H[:n].astype(CLD), 1)
    R[np.arange(n), np.arange(n)] = al.astype(CLD)
    xl = x.astype(CLD)
    num = np.abs(R @ xl - y[:n])
    den = np.abs(R) @ np.abs(xl) + np.sqrt(_abs2(b.astype(CLD)).sum())
    return float((num / den).max()) / T(n)


def z3_tail(yo, tail):
    """rows n .. m-1 of Q^H b against the oracle factor's, relative to 1e-12 max(1, |Q^H b|_inf)"""
    n = len(yo) - len(tail)
    return float(np.abs(tail.astype(CLD) - yo[n:]).max() / max(1.0, float(np.abs(yo).max()))) / 1e-12


# ---------------------------------------------------------------------------------------------- a whole class
class Result:
    def __init__(self, A, b, H, al, x, tail):
        self.A, self.b, self.H, self.al, self.x, self.tail = A, b, H, al, x, tail


def run(backend, A, b):
    H, al = backend.factor(A)
    x, tail = backend.solve_full(H, al, b)
    return Result(A, b, H, al, x, tail)


def _rule(label, ratios, batch):
    """the rule of zbatched_helpers, unchanged (it prints what it judges) -> None, or what it missed"""
    try:
        zh.check_rule(label, ratios, [], above_allowed=1 if batch <= 9 else batch // 100)
    except AssertionError as e:
        return str(e) or "not finite"
    return None


def check_class(backend, orc, cls, m, n, batch, what, seed=SEED, z4=None):
    """Z1-Z5 as they apply to `cls` on every matrix of a batch; z4: Z4 on the first z4 matrices only (the emulator pays half a
    second for a factorisation; the GPU file takes the whole batch).  Returns the Result (Z6 compares it with a mixed batch)."""
    A, b = make(orc, cls, m, n, batch, seed)
    r = run(backend, A, b)
    assert r.H.dtype == A.dtype and r.H.shape == A.shape and r.al.shape == (batch, n) and r.x.shape == (batch, n)
    assert r.tail.shape == (batch, m - n)
    zero_col = cls == "degenerate" and n >= 4
    keys = ("Z2 QR", "Z2 v", "Z3 x", "Z3 res", "Z3 tail")
    ref, ker = dict.fromkeys(keys, 0.0), dict.fromkeys(keys, 0.0)
    z1r, z1k, z1m = [], [], []
    tails_by_ld = 0
    Hos, aos, rd, rl = {}, {}, {}, {}
    label = f"{what} {m}x{n} {cls}"

    def rest(k):  # the complex128 restatement of matrix k, computed once
        if k not in rd:
            rd[k] = restated(A[k])
        return rd[k]

    def rest_ld(k):  # the long-double one, rounded to complex128
        if k not in rl:
            Hl, al_ = restated(A[k], CLD)
            rl[k] = (Hl, Hl.astype(np.complex128), al_.astype(np.complex128))
        return rl[k]

    def worse(d, key, v):
        d[key] = max(d[key], v) if np.isfinite(v) and np.isfinite(d[key]) else np.inf

    for k in range(batch):
        Ho, ao = Hos[k], aos[k] = oracle(orc, A[k])
        Hr, ar = twin(orc, A[k])
        H, al = r.H[k], r.al[k]
        if zero_col and k == 2:
            # Z5: alpha[2] = 0 and everything from row 2 on of the columns >= 2 non-finite, nothing else; the finite entries
            # (the columns before the zero column, the rows of R above it) under Z1; x not all finite
            bad = ~np.isfinite(Ho)
            assert ao[2] == 0 and not np.isfinite(ao[3:]).any() and np.isfinite(ao[:3]).all(), "the oracle"
            assert bad[2:, 2:].all() and not bad[:, :2].any() and not bad[:2].any(), "the oracle"
            assert np.array_equal(~np.isfinite(Hr), bad) and np.array_equal(np.isfinite(ar), np.isfinite(ao)), \
                "the reference's own non-finite pattern: change the input"
            assert al[2] == 0, f"{label}: alpha of the zero column {al[2]!r}"
            assert np.array_equal(np.isfinite(al), np.isfinite(ao)), f"{label}: alpha behind the zero column {al}"
            assert np.array_equal(~np.isfinite(H), bad), \
                f"{label}: behind a zero column the non-finite entries differ from the reference's (rows >= 2 of columns >= 2, nothing else) at (row, column) {np.argwhere(~np.isfinite(H) != bad)[:6].tolist()}"
            Hd, ad = rest(k)
            z1r.append(max(zh.ratio_H(unfinite(Ho), unfinite(ao), unfinite(Hr), unfinite(ar)),
                           zh.ratio_H(unfinite(Ho), unfinite(ao), unfinite(Hd), unfinite(ad))))
            z1k.append(zh.ratio_H(unfinite(Ho), unfinite(ao), unfinite(H), unfinite(al)))
            assert not np.isfinite(r.x[k]).all(), f"{label}: x of the zero-column matrix is finite"
            continue
        xo = oracle_solve(orc, Ho, ao, b[k])
        assert np.isfinite(Ho).all() and np.isfinite(ao).all() and np.isfinite(xo).all(), "the reference is not finite here: change the input"
        assert np.isfinite(H).all() and np.isfinite(al).all() and np.isfinite(r.x[k]).all() and np.isfinite(r.tail[k]).all(), \
            f"{label}: matrix {k} not finite"
        if cls in Z1_CLASSES or cls == "degenerate":
            z1r.append(max(zh.ratio_H(Ho, ao, Hr, ar), zh.ratio_H(Ho, ao, *rest(k))))
            z1k.append(zh.ratio_H(Ho, ao, H, al))
            z1m.append(k)
        for d, (Hx, ax) in ((ref, (Ho, ao)), (ker, (H, al))):
            be, ev = z2(A[k], Hx, ax)
            worse(d, "Z2 QR", be)
            worse(d, "Z2 v", ev)
        xr = twin_solve(orc, Hr, ar, b[k])
        if cls in RESIDUAL:
            worse(ref, "Z3 res", z3_residual(Ho, ao, b[k], xo))
            worse(ker, "Z3 res", z3_residual(H, al, b[k], r.x[k]))
            if m > n:
                # kappa governs the tail as it governs x (measured on the reference alone: the tails of the oracle's two restatements are up to 8e3
                # (rowgraded_up) and 8e9 (lowrank) times the bound from the oracle's), so the tail is judged as the residual is: against Q^H b formed in np.clongdouble
                # from the factor itself -- the reference's in plain complex128 from the oracle's factor
                yo = qhb_cld(Ho, b[k])
                worse(ref, "Z3 tail", z3_tail(yo, qhb_plain(Ho, b[k])[n:]))
                worse(ker, "Z3 tail", z3_tail(qhb_cld(H, b[k]), r.tail[k]))
        else:
            worse(ref, "Z3 x", z3_forward(xo, xr))
            worse(ker, "Z3 x", z3_forward(xo, r.x[k]))
            if m > n:
                # the reference first, with both restatements as in Z1 (below): the rows behind n of Q^H b turn with the phases
                # of the pivots, so where the oracle's factor is no measure of H it is none of the tail either, and the
                # tail is judged against that of the restatement in np.clongdouble
                yo = qhb_cld(Ho, b[k])
                t_ref = max(z3_tail(yo, qhb_cld(Hr, b[k])[n:]), z3_tail(yo, qhb_cld(rest(k)[0], b[k])[n:]))
                if t_ref <= 1.0:
                    worse(ref, "Z3 tail", t_ref)
                    worse(ker, "Z3 tail", z3_tail(yo, r.tail[k]))
                else:
                    tails_by_ld += 1
                    yl = qhb_cld(rest_ld(k)[0], b[k])
                    worse(ref, "Z3 tail", z3_tail(yl, qhb_cld(rest(k)[0], b[k])[n:]))
                    worse(ker, "Z3 tail", z3_tail(yl, r.tail[k]))
        if cls == "degenerate" and k == 1:
            # Z5, zero pivot: alphafactor(0) = -1, so alpha_0 = -||a_0||, real and negative, and the reflector is a proper one
            s = float(np.sqrt(_abs2(A[k][:, 0].astype(CLD)).sum()))
            assert ao[0].imag == 0 and ao[0].real < 0 and abs(abs(ao[0]) - s) <= 2 * EPS * s, "the oracle"
            assert al[0].imag == 0 and al[0].real < 0 and abs(abs(al[0]) - s) <= 2 * EPS * s, \
                f"{label}: zero pivot: alpha[0] = {al[0]!r}, the reference's -||a_0|| = {-s!r}"
    # Z4: symmetries, bit for bit, on the whole batch or its first z4 matrices (but the zero-pivot matrix under negation and
    # rotation)
    ks = list(range(batch if z4 is None else min(z4, batch)))
    keep = [k for k in ks if not (cls == "degenerate" and k == 1)]
    fin = [k for k in keep if not (zero_col and k == 2)]
    rs = Result(A[ks], b[ks], r.H[ks], r.al[ks], r.x[ks], r.tail[ks])
    rn = run(backend, -rs.A, rs.b)
    xm, tm = backend.solve_full(rs.H, rs.al, -rs.b)
    rc = run(backend, np.conj(rs.A), np.conj(rs.b))
    sym = {"factor(-A) H": same(rn.H[keep], -rs.H[keep]), "factor(-A) alpha": same(rn.al[keep], -rs.al[keep]),
           "solve(-A, b) x": same(rn.x[keep], -rs.x[keep]), "solve(-A, b) tail": same(rn.tail[keep], rs.tail[keep]),
           "solve(A, -b) x": same(xm, -rs.x), "solve(A, -b) tail": same(tm, -rs.tail),
           "factor(conj A) H": same(rc.H, np.conj(rs.H)), "factor(conj A) alpha": same(rc.al, np.conj(rs.al)),
           "solve(conj A, conj b) x": same(rc.x, np.conj(rs.x))}
    # factor(iA) against i factor(A), within T of max|H| for every matrix: a comparison of the kernel with itself, asserted
    # whatever the oracle does (its own figure is printed beside it).  An element-wise comparison of two factors, like Z1,
    # and judged in Z1's classes; a matrix that misses is judged as Z1 judges: both factors under the same bound against
    # the restatement in np.clongdouble, the restatement in complex128 first.
    rotates = cls in Z1_CLASSES or cls == "degenerate"
    Hi, ai = backend.factor(times_i(rs.A)) if rotates else (None, None)
    rots = {k: zh.ratio_H(times_i(r.H[k]), times_i(r.al[k]), Hi[k], ai[k]) for k in fin} if rotates else {}
    rot = max(rots.values(), default=0.0)
    rot_ref = max(zh.ratio_H(times_i(Hos[k]), times_i(aos[k]), *oracle(orc, times_i(A[k]))) for k in fin) if rotates else 0.0
    rot_ld = {}
    for k in (k for k in fin if rotates and not rots[k] <= 1.0):
        _, Hl, al_ = rest_ld(k)
        Hli, ali = (v.astype(np.complex128) for v in restated(times_i(A[k]), CLD))
        reference = max(zh.ratio_H(Hl, al_, *rest(k)), zh.ratio_H(Hli, ali, *restated(times_i(A[k]))))
        assert reference <= 1.0, f"factor(iA), matrix {k}: the reference misses the bound here: change the input ({reference:.3f})"
        rot_ld[k] = max(zh.ratio_H(Hl, al_, r.H[k], r.al[k]), zh.ratio_H(Hli, ali, Hi[k], ai[k]))
    broken = [k for k, v in sym.items() if not v]
    print(f"{label}: {batch} matrices, worst ratio to the bound, reference | kernel: "
          + (f"Z1 {max(z1r):.3f} | {max(z1k):.3f} " if z1r else "")
          + " ".join(f"{c} {ref[c]:.3f} | {ker[c]:.3f}" for c in keys if ref[c] or ker[c])
          + (f" ({tails_by_ld} tails against the long-double restatement)" if tails_by_ld else "")
          + f" Z4 {'bit for bit' if not broken else 'BROKEN'}"
          + (f", factor(iA) {rot_ref:.3f} | {rot:.3f}" if rotates else "")
          + (f" (matrices {sorted(rot_ld)} against the long-double restatement: {max(rot_ld.values()):.3f})" if rot_ld else "")
          + (f"; Z4 on {len(ks)} of {batch}" if len(ks) < batch else ""))
    for c in keys:
        assert ref[c] <= 1.0, f"{c}: the reference misses the bound here: change the input ({ref[c]:.3f})"
    if z1r:
        # Z1, the reference first: the oracle against TWO plain restatements of itself, one that differs in the order of the
        # sums (orc.householder_c_np) and one that forms the phase as -h / |h| (restated).  The kernel inside the rule against
        # the oracle is what the criterion asks.  Where it is outside AND the oracle's own restatements are too -- the classes
        # with parts 2^60 apart from n = 8 on, single matrices of a batch of 64: an error of 1e-16 in the small part of the
        # phase grows by the ratio of column norm to pivot with every column, 6e8 T at 128 x 128 -- the miss is the
        # reference's: the classes, shapes and batches being given there is no input to change, so the figures are printed
        # and the kernel is judged under the same rule against the restatement in np.clongdouble, after the restatement in
        # complex128 has been.
        ref_missed = _rule(f"{label} Z1, the oracle's two restatements", z1r, batch)
        missed = _rule(f"{label} Z1, the kernel", z1k, batch)
        assert missed is None or ref_missed is not None, missed
        if missed is not None:
            print(f"{label} Z1: NOT JUDGED AGAINST THE ORACLE, whose own restatements miss the rule.  Against the long-double restatement:")
            fr, fk = [], []
            for k in z1m:
                _, Hl, al_ = rest_ld(k)
                fr.append(zh.ratio_H(Hl, al_, *rest(k)))
                fk.append(zh.ratio_H(Hl, al_, r.H[k], r.al[k]))
            missed = _rule(f"{label} Z1, the complex128 restatement against the long-double one", fr, batch)
            assert missed is None, f"Z1: the reference misses the rule here: change the input ({missed})"
            missed = _rule(f"{label} Z1, the kernel against the long-double restatement", fk, batch)
            assert missed is None, missed
    for c in keys:
        assert ker[c] <= 1.0, f"{label}: {c} at {ker[c]:.3f} of its bound (reference {ref[c]:.3f})"
    assert not broken, f"{label}: symmetries that do not hold bit for bit: {broken}"
    for k in fin if rotates else ():
        assert rots[k] <= 1.0 or rot_ld[k] <= 1.0, \
            f"{label}: matrix {k}: factor(iA) is {rots[k]:.3f} T from i factor(A) and {rot_ld[k]:.3f} T from the long-double restatement (the oracle {rot_ref:.3f})"
    return r


def check_degenerate_neighbours(backend, orc, m, n, batch, what, r, seed=SEED, signed_result=None):
    """Z5: every matrix but 1 and 2 of the degenerate batch has the bits of the `signed` batch (the same matrices without the
    degenerate ones; signed_result: that batch's Result where the caller has it); matrices 0 and 3 share the workgroup of 1 and
    2 on the wave tier"""
    s = signed_result or run(backend, *make(orc, "signed", m, n, batch, seed))
    assert same(s.A[[0, 3]], r.A[[0, 3]]) and len(s.A) == batch
    keep = [k for k in range(batch) if k != 1 and (k != 2 or n < 4)]  # (no zero column for n < 4: matrix 2 is untouched too)
    assert same(r.H[keep], s.H[keep]) and same(r.al[keep], s.al[keep]) and same(r.x[keep], s.x[keep]) and same(r.tail[keep], s.tail[keep]), \
        f"{what}: a degenerate matrix disturbed a neighbour in its batch"


def check_mixed(backend, orc, m, n, what, results, which=None):
    """Z6: hard_inputs.check_mixed on the complex classes; which: these matrices of every class only"""
    if which is not None:
        results = {c: Result(r.A[which], r.b[which], r.H[which], r.al[which], r.x[which], r.tail[which]) for c, r in results.items()}
    HI.check_mixed(backend, orc, m, n, "c64", what, results)


def rhs_columns(orc, m, batch, K, seed=SEED):
    """B (batch, m, K): column r of B_k = the b of seed + 1000 r"""
    return np.stack([np.stack([signed(orc.rand_vector_c(m, seed + 1000 * r + 5000 + k)) for r in range(K)], axis=1) for k in range(batch)])


def check_nrhs(backend, orc, cls, m, n, batch, Ks, what, seed=SEED):
    """several right-hand sides on a hard class, for every column count K of Ks: column r of solve(H, B[..., :K]) has the bits of
    solve(H, B[..., r]); odd in B"""
    A, b = make(orc, cls, m, n, batch, seed)
    B = rhs_columns(orc, m, batch, max(Ks), seed)
    assert same(np.ascontiguousarray(B[:, :, 0]), b)
    H, al = backend.factor(A)
    alone = [backend.solve(H, al, np.ascontiguousarray(B[:, :, r])) for r in range(max(Ks))]
    for K in Ks:
        BK = np.ascontiguousarray(B[:, :, :K])
        X = backend.solve(H, al, BK)
        assert X.shape == (batch, n, K)
        for r in range(K):
            assert same(np.ascontiguousarray(X[:, :, r]), alone[r]), f"{what} {cls} {m}x{n}: column {r} of {K} differs from the single-column call"
        assert same(backend.solve(H, al, -BK), -X), f"{what} {cls} {m}x{n}: H \\ B is not odd in B ({K} columns)"
    print(f"{what} {m}x{n} {cls}: {list(Ks)} columns x {batch} matrices: every column the single-column call's bits, odd in B")


def check_apply(backend, orc, cls, m, n, batch, K, what, seed=SEED):
    """apply-Q, explicit Q and R on a hard class: zapplyq_helpers.check_r / check_qr on (form_q, form_r, A) -- with A and R
    scaled by the power of two that brings max|A| into [1/2, 1), so that Q^H Q - I is judged against Q's own magnitude and A -
    QR against A's --, Q (Q^H B) = B within T max|B|, form_q = Q [I; 0] bit for bit.  The reference: the oracle's factor with
    the reflectors applied in np.clongdouble."""
    A, _ = make(orc, cls, m, n, batch, seed)
    B = rhs_columns(orc, m, batch, K, seed)
    H, al = backend.factor(A)
    Q, R = backend.form_q(H, al), backend.form_r(H, al)
    W = backend.apply_q(H, al, B, True)
    back = backend.apply_q(H, al, W, False)
    E = backend.apply_q(H, al, np.stack([Z.eye_columns(m, n)] * batch), False)
    assert Q.shape == (batch, m, n) and R.shape == (batch, n, n) and back.shape == B.shape
    assert same(Q, E), f"{what} {cls} {m}x{n}: form_q != apply_q on [I; 0]"
    worst = {"ref": 0.0, "ker": 0.0}
    for k in range(batch):
        e = -int(np.frexp(np.abs(A[k]).max())[1])
        Ho, ao = oracle(orc, A[k])
        Ro = np.triu(Ho[:n], 1) + np.diag(ao)
        Qo = Z.reflect_clongdouble(Ho, Z.eye_columns(m, n), 0).astype(np.complex128)
        Z.check_qr(Qo, scaled(Ro, e), scaled(A[k], e), f"{what} {cls} {m}x{n} matrix {k}, the reference")
        Z.check_r(R[k], H[k], al[k])
        Z.check_qr(Q[k], scaled(R[k], e), scaled(A[k], e), f"{what} {cls} {m}x{n} matrix {k}")
        bo = Z.reflect_clongdouble(Ho, Z.reflect_clongdouble(Ho, B[k], 1).astype(np.complex128), 0).astype(np.complex128)
        scale = T(n) * float(np.abs(B[k]).max())
        worst["ref"] = max(worst["ref"], float(np.abs(bo - B[k]).max()) / scale)
        worst["ker"] = max(worst["ker"], float(np.abs(back[k] - B[k]).max()) / scale)
    print(f"{what} {m}x{n} {cls}: Q (Q^H B) - B over {batch} matrices, {K} columns, in units of T max|B|, reference | kernel: "
          f"{worst['ref']:.3f} | {worst['ker']:.3f}")
    assert worst["ref"] <= 1.0, "the reference misses the bound here: change the input"
    assert worst["ker"] <= 1.0, f"{what} {cls} {m}x{n}: Q (Q^H B) is {worst['ker']:.3f} T max|B| from B"


# ---------------------------------------------------------------------------------------------- the 1 x 1 sweep
def sweep_inputs(orc, count, seed=SEED):
    """a_k = +-(1 + u) 2^(e - d+) + i (+-(1 + u') 2^(e + d-)), signs independent, e stepping evenly through [-500, 500], d
    through [-60, 60] in a fixed shuffled order (d_k = 37 k mod 121 - 60), d+ = max(d, 0) shifting the real part down and d- =
    min(d, 0) the imaginary part; b_k = (1 + w) - i (1 + w')"""
    u, u2, w, w2 = (orc.rand_vector(count, seed + i) for i in range(4))
    sr = np.where(orc.rand_vector(count, seed + 4) < 0.5, -1.0, 1.0)
    si = np.where(orc.rand_vector(count, seed + 5) < 0.5, -1.0, 1.0)
    e = np.round(np.linspace(-EXP, EXP, count)).astype(np.int64)
    d = (37 * np.arange(count)) % (2 * SKEW + 1) - SKEW
    a = cplx(np.ldexp(sr * (1.0 + u), e - np.maximum(d, 0)), np.ldexp(si * (1.0 + u2), e + np.minimum(d, 0)))
    b = cplx(1.0 + w, -(1.0 + w2))
    assert e[0] == -EXP and e[-1] == EXP and d.min() == -SKEW and d.max() == SKEW and np.isfinite(a).all()
    return a.reshape(count, 1, 1), b.reshape(count, 1)


def sweep_figures(A, b, H, al, x):
    """(|alpha + a| / |a| / 2 eps, | |v|^2 - 2 | / 2 T(1), |x - b/a| / |b/a| / T(1)), per entry"""
    a, all_, v, xl = A[:, 0, 0].astype(CLD), al[:, 0].astype(CLD), H[:, 0, 0].astype(CLD), x[:, 0].astype(CLD)
    q = b[:, 0].astype(CLD) / a
    return (np.abs(all_ + a) / np.abs(a) / (2 * EPS)).astype(float), (np.abs(_abs2(v) - 2) / (2 * T(1))).astype(float), \
        (np.abs(xl - q) / np.abs(q) / T(1)).astype(float)


def check_sweep(backend, orc, count, what):
    """a batch of 1 x 1 matrices: alpha = -a up to the rounding of hypot and the phase, |v|^2 = 2, x = b / a -- hypot, the
    phase, f in plain division and both branches of Smith's division swept over the exponent range and over parts up to
    2^60 apart, in one launch"""
    A, b = sweep_inputs(orc, count)
    r = run(backend, A, b)
    Ho, ao, xo = (np.empty_like(v) for v in (r.H, r.al, r.x))
    for k in range(count):
        Ho[k], ao[k] = oracle(orc, A[k])
        xo[k] = oracle_solve(orc, Ho[k], ao[k], b[k])
    assert np.isfinite(Ho).all() and np.isfinite(ao).all() and np.isfinite(xo).all(), "the reference is not finite here: change the input"
    assert np.isfinite(r.al).all() and np.isfinite(r.H).all() and np.isfinite(r.x).all(), f"{what}: the sweep is not finite"
    fr, fk = sweep_figures(A, b, Ho, ao, xo), sweep_figures(A, b, r.H, r.al, r.x)
    names = ("alpha", "|v|^2", "x")
    print(f"{what} 1x1 sweep of {count}: worst ratio to the bound, reference | kernel: "
          + " ".join(f"{nm} {f.max():.3f} | {g.max():.3f}" for nm, f, g in zip(names, fr, fk)))
    for nm, f in zip(names, fr):
        assert f.max() <= 1.0, f"{nm}: the reference misses the bound here: change the input ({f.max():.3f})"
    for nm, g in zip(names, fk):
        k = int(np.argmax(g))
        assert g[k] <= 1.0, f"{what}: {nm} of a = {A[k, 0, 0]!r}, b = {b[k, 0]!r}: alpha {r.al[k, 0]!r} v {r.H[k, 0, 0]!r} x {r.x[k, 0]!r}"
