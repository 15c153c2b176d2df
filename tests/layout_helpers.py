"""Test-only helpers: matrices and vectors laid out the way a caller may hand them to the library -- a leading dimension
larger than the row count, a base that is not 16-byte aligned -- inside a larger buffer whose every element outside the
window holds a quiet NaN with a recognisable payload ("poison").  A stray store changes the poison's bits
(assert_guards_intact compares them bitwise); a stray load that is folded into arithmetic turns a result into NaN.

Works on numpy buffers (host arrays, and the "device" memory of the emulated library) and on torch CUDA buffers.
The product never imports this file."""
import numpy as np

POISON_BITS = 0x7FF8_DEAD_BEEF_5A5A  # quiet NaN, payload 0xDEADBEEF5A5A
GUARD = 64  # elements of guard before the base and after the last element of the window (at least)

# (lda - m, off): the control, even padding, odd stride, base 8 bytes off a 16-byte boundary, both, wide padding
LAYOUTS = [(0, 0), (2, 0), (1, 0), (0, 1), (1, 1), (64, 0)]
LAYOUT_IDS = ["control", "lda+2", "lda+1", "off1", "lda+1_off1", "lda+64"]


def each_layout(m, fn, layouts=None):
    """fn(lda, off) for every (name, (lda - m, off)) of `layouts` (default: LAYOUTS); AssertionErrors are collected so
    that one failure message names every layout that failed"""
    fails = []
    for name, (pad, off) in (layouts or zip(LAYOUT_IDS, LAYOUTS)):
        try:
            fn(m + pad, off)
        except AssertionError as e:
            fails.append(f"[{name}: lda = m + {pad}, off = {off}] {e}")
    assert not fails, "\n".join(fails)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class Guarded:
    """`buf`: the whole 1-D buffer (float64 or complex128); `view`: the m x n column-major window (leading dimension
    `ld`, first element `off` elements into `buf`) or, for a vector, the length-m window; `inside`: boolean numpy mask
    of `buf` that is True on the window."""

    def __init__(self, buf, view, inside, off, ld):
        self.buf, self.view, self.inside, self.off, self.ld = buf, view, inside, off, ld

    @property
    def ptr(self):
        """address of the window's first element"""
        return self.view.data_ptr() if _is_torch(self.view) else self.view.ctypes.data

    def host(self):
        """copy of the window as a column-major numpy array"""
        v = self.view.cpu().numpy() if _is_torch(self.view) else self.view
        return np.array(v, order="F")

    def bits(self):
        """the whole buffer as uint64 words (two per complex element), on the host"""
        b = self.buf
        if _is_torch(b):
            import torch
            if b.is_complex():
                b = torch.view_as_real(b)
            return b.reshape(-1).view(torch.int64).cpu().numpy().view(np.uint64)
        return b.view(np.uint64).reshape(-1)


def _alloc(total, dtype, device, align_bytes=256):
    """1-D buffer of `total` elements whose first element sits on an `align_bytes` boundary, filled with the poison"""
    isz = np.dtype(dtype).itemsize
    extra = align_bytes // isz
    if device is None:
        raw = np.empty(total + extra, dtype=dtype)
        s = (-raw.ctypes.data % align_bytes) // isz
        buf = raw[s:s + total]
        buf.view(np.uint64)[:] = POISON_BITS
    else:
        import torch
        tdt = torch.complex128 if np.dtype(dtype) == np.complex128 else torch.float64
        raw = torch.empty(total + extra, dtype=tdt, device=device)
        s = (-raw.data_ptr() % align_bytes) // isz
        buf = raw[s:s + total]
        words = torch.view_as_real(buf).reshape(-1) if buf.is_complex() else buf
        words.view(torch.int64).fill_(POISON_BITS)  # (a positive int64: the sign bit of the NaN is clear)
    assert (buf.data_ptr() if device is not None else buf.ctypes.data) % align_bytes == 0
    return buf


def guarded_matrix(m, n, ld, off, *, dtype=np.float64, device=None, content=None, guard=GUARD):
    """m x n column-major window with leading dimension `ld` starting `off` elements into a poisoned buffer (`guard`
    elements before it, at least `guard` after its last column).  `content` (m x n numpy array) is copied into the
    window; the padding rows m..ld-1 of every column keep the poison."""
    assert ld >= max(m, 1) and off >= 0
    base = guard + off
    total = base + ld * n + guard
    buf = _alloc(total, dtype, device)
    idx = base + np.arange(m)[:, None] + ld * np.arange(n)[None, :]
    inside = np.zeros(total, dtype=bool)
    inside[idx.reshape(-1)] = True
    if device is None:
        view = np.ndarray((m, n), dtype=dtype, buffer=buf, offset=base * buf.itemsize,
                          strides=(buf.itemsize, buf.itemsize * ld))
        if content is not None:
            view[...] = content
    else:
        view = buf.as_strided((m, n), (1, ld), buf.storage_offset() + base)
        if content is not None:
            import torch
            view.copy_(torch.from_numpy(np.asarray(content, dtype=dtype)))
    return Guarded(buf, view, inside, base, ld)


def guarded_vector(m, off, *, dtype=np.float64, device=None, content=None, guard=GUARD):
    """length-m window `off` elements past an aligned boundary inside a poisoned buffer, `guard` elements on each side"""
    g = guarded_matrix(m, 1, max(m, 1), off, dtype=dtype, device=device, content=None, guard=guard)
    g.view = g.view[:, 0]
    if content is not None:
        if device is None:
            g.view[...] = content
        else:
            import torch
            g.view.copy_(torch.from_numpy(np.asarray(content, dtype=dtype)))
    return g


def assert_guards_intact(g, what="buffer"):
    """every element of g.buf outside the window still holds the poison, bit for bit"""
    bits = g.bits()
    outside = ~np.repeat(g.inside, bits.size // g.inside.size)
    bad = np.flatnonzero(outside & (bits != np.uint64(POISON_BITS)))
    if bad.size:
        per = bits.size // g.inside.size
        el = bad // per - g.off
        raise AssertionError(f"{what}: {bad.size} word(s) outside the window changed; first element offsets from the base "
                             f"{el[:8].tolist()} (ld {g.ld}), e.g. element {el[0]} = row {el[0] % g.ld}, column "
                             f"{el[0] // g.ld} now 0x{int(bits[bad[0]]):016x}")
