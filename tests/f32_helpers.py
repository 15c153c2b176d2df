"""Test-only helpers of the Float32 tests (test_emulated_f32.py, test_gpu_f32.py): the seeded inputs rounded to float32, a
numpy twin of the native kernels' arithmetic (float storage, double sums: csrc/dhqr_f32.h), the acceptance criteria against
the Float64 oracle and against LAPACK in Float32, and NaN-guarded float32 buffers (the layouts of layout_helpers.py with a
float32 quiet-NaN poison).  The product never imports this file."""
import numpy as np

from layout_helpers import GUARD, Guarded

EPS32 = float(np.finfo(np.float32).eps)
NATIVE_SHAPES = [(1, 1), (5, 3), (12, 6), (16, 8), (33, 9), (40, 17), (64, 32), (32, 32)]
OVERDETERMINED = [(5, 3), (16, 8), (33, 9), (40, 17), (64, 32)]
POISON32 = 0x7FC5A5A5  # float32 quiet NaN with a recognisable payload


def tol_factor(n):
    """|H32 - H64| element-wise and |alpha32 - alpha64| / |alpha64|: the expression of the Float64 batched tests with float32's eps"""
    return 8.0 * max(n, 8) * EPS32


def inputs(orc, m, n, batch, seed):
    """(A (batch, m, n) float32, b (batch, m) float32): the seeded generator's values, rounded"""
    A = np.ascontiguousarray(np.stack([orc.rand_matrix(m, n, seed + k) for k in range(batch)]), dtype=np.float32)  # (C order)
    b = np.ascontiguousarray(np.stack([orc.rand_vector(m, seed + 5000 + k) for k in range(batch)]), dtype=np.float32)
    return A, b


# ---------------------------------------------------------------------------------------------- the twin
def twin_factor(A32):
    """householder!(A, alpha) with the matrix stored in float32 and every sum taken in float64 (k_batched_qr_wave_s)"""
    a = np.array(A32, dtype=np.float32, order="F")
    m, n = a.shape
    alpha = np.zeros(n, dtype=np.float32)
    for j in range(n):
        x = a[:, j].astype(np.float64)
        s2 = float(np.sum(x[j:] * x[j:]))
        h = x[j]
        sn = np.sqrt(s2)
        f = 1.0 / np.sqrt(sn * (sn + abs(h)))
        al = sn * (-np.sign(h))
        v = np.zeros(m)
        v[j] = (h - al) * f
        v[j + 1:] = x[j + 1:] * f
        vf = v.astype(np.float32)
        a[j:, j] = vf[j:]
        alpha[j] = np.float32(al)
        if j + 1 < n:
            vd = vf[j:].astype(np.float64)
            t = a[j:, j + 1:].astype(np.float64)
            a[j:, j + 1:] = (t - np.outer(vd, vd @ t)).astype(np.float32)
    return a, alpha


def twin_solve(H32, al32, b32):
    """solve_householder!(b, H, alpha): b carried in float64, each entry rounded once at the end (k_batched_ldiv_wave_s)"""
    H = H32.astype(np.float64)
    m, n = H.shape
    b = b32.astype(np.float64)
    for j in range(n):
        b[j:] -= H[j:, j] * (H[j:, j] @ b[j:])
    for j in range(n - 1, -1, -1):
        b[j] /= float(al32[j])
        b[:j] -= H[:j, j] * b[j]
    return b.astype(np.float32)


# ---------------------------------------------------------------------------------------------- criteria
def factor_errors(orc, A32, H32, al32):
    """(max |H32 - H64|, max |alpha32 - alpha64| / |alpha64|, max | ||v_j||^2 - 2 |) against the Float64 oracle on the same
    float32 values widened exactly"""
    Ho, ao = orc.householder(A32.astype(np.float64))
    H = H32.astype(np.float64)
    eH = float(np.abs(H - Ho).max())
    ea = float((np.abs(al32.astype(np.float64) - ao) / np.where(ao == 0.0, 1.0, np.abs(ao))).max())  # (a zero pivot: alpha = -0 s)
    ev = float(np.abs((np.tril(H) ** 2).sum(axis=0) - 2.0).max())
    return eH, ea, ev


def check_factor(orc, A32, H32, al32, ks, what):
    """criterion 1 for the matrices `ks` of a batch: first the twin on the test's own seeds, then the result"""
    m, n = A32.shape[1:]
    tol = tol_factor(n)
    wt, wr = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for k in ks:
        wt = [max(a, b) for a, b in zip(wt, factor_errors(orc, A32[k], *twin_factor(A32[k])))]
        wr = [max(a, b) for a, b in zip(wr, factor_errors(orc, A32[k], H32[k], al32[k]))]
    print(f"{what} {m}x{n}: {len(ks)} matrices vs oracle: twin |dH|={wt[0]:.2e} |dalpha|/|alpha|={wt[1]:.2e} | result |dH|={wr[0]:.2e} "
          f"|dalpha|/|alpha|={wr[1]:.2e} (tol {tol:.2e}) | ||v||^2-2| twin {wt[2]:.2e} result {wr[2]:.2e} (tol {2 * tol:.2e})")
    assert wt[0] <= tol and wt[1] <= tol and wt[2] <= 2 * tol, "the numpy twin misses the bound at these seeds: change the seed"
    assert np.isfinite(H32[list(ks)]).all() and np.isfinite(al32[list(ks)]).all()
    assert wr[0] <= tol and wr[1] <= tol
    assert wr[2] <= 2 * tol


def check_solve(orc, H32, al32, b32, x32, ks, what):
    """criterion 2: x32 against the Float64 oracle's solve applied to the kernel's OWN factor, widened:
    |dx|_inf <= 4 eps32 |x|_inf (b is carried in double and every entry rounded once, eps32 / 2; a factor 8 over that)"""
    worst = 0.0
    for k in ks:
        xo = orc.solve(np.asfortranarray(H32[k].astype(np.float64)), al32[k].astype(np.float64), b32[k].astype(np.float64))
        worst = max(worst, float(np.abs(x32[k].astype(np.float64) - xo).max() / np.abs(xo).max()))
    print(f"{what} {H32.shape[1]}x{H32.shape[2]}: solve alone, {len(ks)} matrices: |dx|/|x|={worst:.2e} (tol {4 * EPS32:.2e})")
    assert worst <= 4 * EPS32


def lapack_f32_solve(A32, b32):
    """numpy.linalg.qr + triangular solve, everything in float32"""
    Q, R = np.linalg.qr(A32)
    assert Q.dtype == np.float32 and R.dtype == np.float32
    y = Q.T @ b32
    n = R.shape[0]
    x = np.zeros(n, dtype=np.float32)
    for j in range(n - 1, -1, -1):
        x[j] = (y[j] - R[j, j + 1:] @ x[j + 1:]) / R[j, j]
    return x


def check_vs_lapack(orc, A32, b32, x32, ks, what):
    """criterion 3 (overdetermined shapes): over the whole batch, max_k |x32 - x64| / |x64| is at most 4 x the same maximum
    for LAPACK in float32; x64 = the Float64 oracle's qr! + \\ on the widened inputs"""
    mine = theirs = 0.0
    for k in ks:
        A64 = A32[k].astype(np.float64)
        Ho, ao = orc.householder(A64)
        xo = orc.solve(Ho, ao, b32[k].astype(np.float64))
        s = np.abs(xo).max()
        mine = max(mine, float(np.abs(x32[k].astype(np.float64) - xo).max() / s))
        theirs = max(theirs, float(np.abs(lapack_f32_solve(A32[k], b32[k]).astype(np.float64) - xo).max() / s))
    print(f"{what} {A32.shape[1]}x{A32.shape[2]}: qr! + \\ over {len(ks)} matrices: max |x32-x64|/|x64| = {mine:.2e}, "
          f"LAPACK float32 {theirs:.2e}, ratio {mine / theirs:.2f} (bound 4)")
    assert mine <= 4.0 * theirs


# ---------------------------------------------------------------------------------------------- guarded float32 buffers
class GuardedF32(Guarded):
    def bits(self):
        b = self.buf
        if type(b).__module__.startswith("torch"):
            import torch
            return b.view(torch.int32).cpu().numpy().view(np.uint32)
        return b.view(np.uint32)


def guarded_f32(m, n, ld, off, device=None, content=None):
    """m x n column-major float32 window (leading dimension ld) whose first element lies GUARD + off elements into a
    256-byte-aligned buffer filled with POISON32; off = 1: a base 4 bytes off an 8-byte boundary.  n = 1 with a 1-D
    `content` gives a vector (view of shape (m,))."""
    vector = content is not None and np.ndim(content) == 1
    base = GUARD + off
    total = base + ld * max(n - 1, 0) + m + GUARD
    idx = base + np.arange(m)[:, None] + ld * np.arange(n)[None, :]
    inside = np.zeros(total, dtype=bool)
    inside[idx.reshape(-1)] = True
    if device is None:
        raw = np.empty(total + 64, dtype=np.float32)
        s = (-raw.ctypes.data % 256) // 4
        buf = raw[s:s + total]
        buf.view(np.uint32)[:] = POISON32
        view = np.ndarray((m, n), dtype=np.float32, buffer=buf, offset=base * 4, strides=(4, 4 * ld))
        if content is not None:
            view[...] = np.reshape(content, (m, n))
        assert buf.ctypes.data % 256 == 0
    else:
        import torch
        raw = torch.empty(total + 64, dtype=torch.float32, device=device)
        s = (-raw.data_ptr() % 256) // 4
        buf = raw[s:s + total]
        buf.view(torch.int32).fill_(POISON32)
        view = buf.as_strided((m, n), (1, ld), buf.storage_offset() + base)
        if content is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(np.reshape(content, (m, n)), dtype=np.float32)))
        assert buf.data_ptr() % 256 == 0
    g = GuardedF32(buf, view[:, 0] if vector else view, inside, base, ld)
    assert g.ptr % 4 == 0 and (off % 2 == 0 or g.ptr % 8 == 4)
    return g


def assert_f32_guards_intact(g, what="buffer"):
    bits = g.bits()
    bad = np.flatnonzero(~g.inside & (bits != np.uint32(POISON32)))
    if bad.size:
        el = bad - g.off
        raise AssertionError(f"{what}: {bad.size} word(s) outside the window changed; first element offsets from the base "
                             f"{el[:8].tolist()} (ld {g.ld}), e.g. now 0x{int(bits[bad[0]]):08x}")
