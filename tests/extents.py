"""Memory-extent harness for the C ABI (include/nxsig.h): where does a call read, where does it write?

Every tensor of a checked call lives in an ARENA of its own: one allocation filled with the 32-bit pattern POISON, the tensor GUARD
bytes in (plus `offset_elems` elements for the sliced-tensor cases) and GUARD bytes of pattern behind its last element.  Input rows may
lie `row_stride` elements apart; the gap after every row holds the pattern as well.  POISON is a quiet NaN with a recognisable payload:
a NaN as f32, in either half of a c64 and — doubled — as f64, so a gap or guard element that reaches a result shows as a NaN the oracle
does not have, and a result element nobody wrote still carries the pattern.

Elements of one byte (the u8 mask of nxsig_nonzero) go by bytes: the guards stay whole words of the pattern, and the bytes between the
tensor's last element and the next word boundary hold the pattern too — a tail gap, every byte of it non-zero.  Integer results (the s32
[size][rank] table and the u32 count of nxsig_argrelextrema) are judged as tables: an element nobody wrote still holds POISON, which is
neither -1 nor a coordinate of any shape the suite uses, and the exact comparison names the row and the column.

After the call the whole arenas are read back and checked by the functions below, which work on plain numpy images: the same code
judges a HIP kernel (tests/test_gpu_strided_rows.py, tests/test_gpu_output_extents.py) and the numpy stand-ins with planted faults of
tests/test_extents_harness_host.py.  Every finding names its place: which guard and how far from the tensor, or which row and index.

No GPU code here: the device side is nxsig_alloc / nxsig_upload / nxsig_download through the context it is handed."""
import ctypes as C

import numpy as np

POISON = 0x7FF8DEAD           # quiet NaN as f32; doubled, 0x7FF8DEAD7FF8DEAD is a quiet NaN as f64 (0x7FC0... doubled would be finite)
POISON64 = (POISON << 32) | POISON
GUARD = 4096                  # bytes in front of and behind every tensor: a multiple of 256 (the interior keeps a fresh allocation's alignment)
WORDS = GUARD // 4
assert GUARD % 256 == 0 and GUARD >= 4096
assert np.isnan(np.array([POISON], np.uint32).view(np.float32)[0]) and np.isnan(np.array([POISON64], np.uint64).view(np.float64)[0])


class ExtentError(AssertionError):
    """a call read what it may not depend on, wrote outside its result, left a result element out or changed an input"""


class Arena:
    """`rows` rows of `row_len` elements of `dtype`, `row_stride` (>= row_len) elements apart, inside one poisoned allocation.

    image      uint32 words of the whole arena as uploaded
    first      element index of the tensor's first element in `view(image)`
    """

    def __init__(self, name, dtype, rows, row_len, row_stride=None, offset_elems=0, data=None):
        self.name, self.dtype = name, np.dtype(dtype)
        self.rows, self.row_len = int(rows), int(row_len)
        self.row_stride = self.row_len if row_stride is None else int(row_stride)
        assert self.row_stride >= self.row_len and 0 <= offset_elems <= 3
        self.wpe = self.dtype.itemsize // 4                       # 32-bit words per element (0: a one-byte type, laid out by bytes)
        self.narrow = self.dtype.itemsize < 4
        assert self.dtype.itemsize == 1 or self.dtype.itemsize % 4 == 0
        self.count = self.rows * self.row_stride                  # elements up to and including the gap of the last row
        if self.narrow:
            self.lead_bytes = GUARD + offset_elems                # bytes in front of the tensor
            self.end_bytes = self.lead_bytes + (self.rows - 1) * self.row_stride + self.row_len    # first byte behind the last element
            self.lead, self.first = WORDS, self.lead_bytes
            self.image = np.full((self.lead_bytes + self.count + 3) // 4 + WORDS, POISON, np.uint32)   # the tail gap: up to the next word
        else:
            self.lead = WORDS + offset_elems * self.wpe           # words in front of the tensor
            self.lead_bytes = self.lead * 4
            self.first = self.lead // self.wpe
            self.image = np.full(self.lead + self.count * self.wpe + WORDS, POISON, np.uint32)
        self.dev = None
        if data is not None:
            self.fill(data)

    # ---- layout
    @property
    def nbytes(self):
        return self.image.nbytes

    @property
    def offset_bytes(self):
        return self.lead_bytes

    def view(self, image=None):
        """the whole arena as elements of the tensor's type (what a kernel indexes from `first`)"""
        return (self.image if image is None else image).view(self.dtype)

    def tensor(self, image=None):
        """the [rows][row_len] tensor inside an image (a copy)"""
        v = self.view(image)[self.first:self.first + self.count].reshape(self.rows, self.row_stride)
        return v[:, :self.row_len].copy()

    def fill(self, data):
        data = np.ascontiguousarray(data, dtype=self.dtype).reshape(self.rows, self.row_len)
        v = self.view()[self.first:self.first + self.count].reshape(self.rows, self.row_stride)
        v[:, :self.row_len] = data
        return self

    def locate(self, word):
        """where in the arena a 32-bit word lies, in words a reader can act on"""
        word = int(word)
        if word < self.lead:
            return f"{self.name}: front guard, {(self.lead - word) * 4} bytes before the tensor"
        rel = word - self.lead
        end = ((self.rows - 1) * self.row_stride + self.row_len) * self.wpe
        if rel >= end:
            return f"{self.name}: back guard, {(rel - end) * 4} bytes past the tensor"
        elem, part = divmod(rel, self.wpe)
        row, idx = divmod(elem, self.row_stride)
        tail = f" (word {part} of the element)" if self.wpe > 1 else ""
        if idx >= self.row_len:
            return f"{self.name}: gap after row {row}, element {idx - self.row_len}{tail}"
        return f"{self.name}: row {row}, index {idx}{tail}"

    def locate_byte(self, byte):
        """where in the arena of a one-byte type a byte lies"""
        byte = int(byte)
        if byte < self.lead_bytes:
            return f"{self.name}: front guard, {self.lead_bytes - byte} bytes before the tensor"
        if byte >= self.end_bytes:
            past = byte - self.end_bytes
            return f"{self.name}: {'tail gap' if byte < -(-self.end_bytes // 4) * 4 else 'back guard'}, {past} bytes past the tensor"
        row, idx = divmod(byte - self.lead_bytes, self.row_stride)
        if idx >= self.row_len:
            return f"{self.name}: gap after row {row}, element {idx - self.row_len}"
        return f"{self.name}: row {row}, index {idx}"

    # ---- device side
    def upload(self, ctx):
        from nx_signal_amd import _lib
        self.dev = ctx.empty((self.image.size,), np.uint32)
        _lib.check(ctx._lib.nxsig_upload(ctx.handle, C.c_void_p(self.dev.ptr), self.image.ctypes.data_as(C.c_void_p), self.image.nbytes))
        return self

    @property
    def ptr(self):
        """device address of the tensor's first element"""
        return C.c_void_p(self.dev.ptr + self.offset_bytes)

    def download(self):
        return self.dev.numpy()


def _first(words, limit=4):
    return [int(w) for w in words[:limit]]


def _byte_inside(arena, nbytes):
    inside = np.zeros(nbytes, bool)
    rows = inside[arena.lead_bytes:arena.lead_bytes + arena.count].reshape(arena.rows, arena.row_stride)
    rows[:, :arena.row_len] = True
    return inside


def guard_findings(arena, image):
    """words of the two guards (and of the gap behind the last row) that no longer hold the pattern; bytes for a one-byte type"""
    image = np.asarray(image, np.uint32)
    assert image.shape == arena.image.shape
    if arena.narrow:
        b, pat = image.view(np.uint8), np.full(image.size, POISON, np.uint32).view(np.uint8)
        bad = np.flatnonzero(~_byte_inside(arena, b.size) & (b != pat))
        return [f"store outside the result — {arena.locate_byte(w)} holds 0x{int(b[w]):02X}" for w in _first(bad)] + \
               ([f"... {bad.size} guard bytes changed in all"] if bad.size > 4 else [])
    inside = np.zeros(image.size, bool)
    rows = inside[arena.lead:arena.lead + arena.count * arena.wpe].reshape(arena.rows, arena.row_stride * arena.wpe)
    rows[:, :arena.row_len * arena.wpe] = True
    bad = np.flatnonzero(~inside & (image != POISON))
    return [f"store outside the result — {arena.locate(w)} holds 0x{int(image[w]):08X}" for w in _first(bad)] + \
           ([f"... {bad.size} guard words changed in all"] if bad.size > 4 else [])


def unchanged_findings(arena, image):
    """an input arena must come back bit for bit as it was uploaded"""
    image = np.asarray(image, np.uint32)
    assert image.shape == arena.image.shape
    if arena.narrow:
        b, was = image.view(np.uint8), arena.image.view(np.uint8)
        bad = np.flatnonzero(b != was)
        return [f"input modified — {arena.locate_byte(w)}: 0x{int(was[w]):02X} became 0x{int(b[w]):02X}" for w in _first(bad)] + \
               ([f"... {bad.size} input bytes changed in all"] if bad.size > 4 else [])
    bad = np.flatnonzero(image != arena.image)
    return [f"input modified — {arena.locate(w)}: 0x{int(arena.image[w]):08X} became 0x{int(image[w]):08X}" for w in _first(bad)] + \
           ([f"... {bad.size} input words changed in all"] if bad.size > 4 else [])


def _components(a):
    a = np.ascontiguousarray(a)
    return a.view(np.float64 if a.dtype.itemsize // (2 if a.dtype.kind == "c" else 1) == 8 else np.float32)


def unwritten_findings(arena, image, expected):
    """result components that still carry the pattern where the expected result is finite"""
    got = _components(arena.tensor(image))
    fin = np.isfinite(_components(np.asarray(expected, arena.dtype).reshape(arena.rows, arena.row_len)))
    pat = got.view(np.uint64) == np.uint64(POISON64) if got.dtype == np.float64 else got.view(np.uint32) == np.uint32(POISON)
    per = got.shape[1] // arena.row_len
    bad = np.argwhere(pat & fin)
    return [f"result element never written — {arena.name}: row {r}, index {i // per}" for r, i in bad[:4].tolist()] + \
           ([f"... {len(bad)} result components unwritten in all"] if len(bad) > 4 else [])


def finite_findings(arena, got, expected, unit=1, what="index", by_frame=False):
    """the finite mask must equal the expected one exactly; `unit` groups a row into frames (unit = elements per frame).  by_frame: a
    frame counts as finite when all of it is (how the suite compares a non-finite sample's reach: np.fft leaves some components of a
    frame that holds a NaN finite, a complex transform none)"""
    g = np.isfinite(_components(np.asarray(got).reshape(arena.rows, arena.row_len)))
    e = np.isfinite(_components(np.asarray(expected).reshape(arena.rows, arena.row_len)))
    per = g.shape[1] // arena.row_len
    if by_frame:
        g, e = g.reshape(arena.rows, -1, unit * per).all(axis=-1), e.reshape(arena.rows, -1, unit * per).all(axis=-1)
        return [f"{arena.name}: row {r}, frame {m} is {'finite' if g[r, m] else 'not finite'}, the reference's is "
                f"{'finite' if e[r, m] else 'not finite'}" for r, m in np.argwhere(g != e)[:8].tolist()]
    bad = np.argwhere(g != e)
    out = []
    for r, c in bad[:4].tolist():
        i = c // per
        place = f"frame {i // unit}, index {i % unit}" if unit > 1 else f"{what} {i}"
        out.append(f"{arena.name}: row {r}, {place} is {'finite' if g[r, c] else 'not finite'}, the reference is "
                   f"{'finite' if e[r, c] else 'not finite'}")
    if len(bad) > 4:
        out.append(f"... {len(bad)} components differ in finiteness in all")
    return out


def value_findings(arena, got, expected, tol, unit=1, absolute=False, where=None):
    """largest error over the components finite in both (and selected by `where`, one flag per component), normalised by max |expected|
    (or absolute), against `tol`"""
    g = _components(np.asarray(got).reshape(arena.rows, arena.row_len)).astype(np.float64)
    e = _components(np.asarray(expected).reshape(arena.rows, arena.row_len)).astype(np.float64)
    ok = np.isfinite(g) & np.isfinite(e)
    if where is not None:
        ok &= np.asarray(where, bool).reshape(ok.shape)
    if not ok.any():
        return []
    d = np.where(ok, np.abs(np.where(ok, g, 0.0) - np.where(ok, e, 0.0)), 0.0)
    scale = 1.0 if absolute else max(float(np.max(np.abs(e[ok]))), 1e-300)
    r, i = np.unravel_index(int(np.argmax(d)), d.shape)
    err = float(d[r, i]) / scale
    if err <= tol:
        return []
    i //= g.shape[1] // arena.row_len
    place = f"frame {i // unit}, index {i % unit}" if unit > 1 else f"index {i}"
    return [f"{arena.name}: row {r}, {place}: error {err:.3e} above {tol:.1e}"]


def bit_findings(arena, got, want, unit=1):
    """two results that must agree bit for bit"""
    g = np.ascontiguousarray(np.asarray(got).reshape(arena.rows, arena.row_len)).view(np.uint32)
    w = np.ascontiguousarray(np.asarray(want).reshape(arena.rows, arena.row_len)).view(np.uint32)
    bad = np.argwhere(g != w)
    out = []
    for r, i in bad[:4].tolist():
        i //= arena.wpe
        place = f"frame {i // unit}, index {i % unit}" if unit > 1 else f"index {i}"
        out.append(f"{arena.name}: row {r}, {place} differs in bits")
    if len(bad) > 4:
        out.append(f"... {len(bad)} words differ in all")
    return out


def _table(arena, a):
    assert arena.dtype in (np.dtype(np.int32), np.dtype(np.uint32)), arena.dtype
    return np.ascontiguousarray(np.asarray(a).astype(arena.dtype, copy=False).reshape(arena.rows, arena.row_len))


def table_unwritten_findings(arena, image):
    """elements of an integer result ([rows][columns], s32 or u32) that still hold the 32-bit pattern"""
    bad = np.argwhere(_table(arena, arena.tensor(image)).view(np.uint32) == np.uint32(POISON))
    return [f"result element never written — {arena.name}: row {r}, column {c}" for r, c in bad[:4].tolist()] + \
           ([f"... {len(bad)} result elements unwritten in all"] if len(bad) > 4 else [])


def table_findings(arena, got, want):
    """an integer result against the expected table, exactly; elements still unwritten are table_unwritten_findings' to report"""
    g, w = _table(arena, got), _table(arena, want)
    bad = np.argwhere((g != w) & (g.view(np.uint32) != np.uint32(POISON)))
    return [f"{arena.name}: row {r}, column {c} holds {int(g[r, c])}, expected {int(w[r, c])}" for r, c in bad[:4].tolist()] + \
           ([f"... {len(bad)} elements differ from the expected table in all"] if len(bad) > 4 else [])


def findings(inputs, out, out_image, expected=None, tol=None, unit=1, absolute=False, same_bits_as=None, where=None, by_frame=False, table=None):
    """every check of one call: `inputs` = [(arena, image after the call)], `out` the result arena and its image after the call.
    expected + tol: the reference and its bound (finite mask exact); same_bits_as: a result the call must reproduce bit for bit;
    table: the expected integer result of an s32 / u32 arena, compared exactly."""
    found = []
    for arena, image in inputs:
        found += unchanged_findings(arena, image)
    found += guard_findings(out, out_image)
    got = out.tensor(out_image)
    if table is not None:
        found += table_unwritten_findings(out, out_image) + table_findings(out, got, table)
    if expected is not None:
        found += unwritten_findings(out, out_image, expected)
        found += finite_findings(out, got, expected, unit, by_frame=by_frame)
        if tol is not None:
            found += value_findings(out, got, expected, tol, unit, absolute, where)
    if same_bits_as is not None:
        found += bit_findings(out, got, same_bits_as, unit)
    return found


def verify(*args, **kw):
    found = findings(*args, **kw)
    if found:
        raise ExtentError("\n".join(found))


def call(ctx, fn, *args):
    """one C ABI call fn(ctx handle, *args) on `ctx`, waited for; returns the call's dispatch record"""
    from nx_signal_amd import _lib
    _lib.check(fn(ctx.handle, *args))
    ctx.sync()
    return ctx.last_dispatch()
