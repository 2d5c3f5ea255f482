"""tests/extents.py catches what it is for: numpy stand-ins for a kernel, correct ones and ones with a planted fault each, run through the
arena layout the GPU tests use (strided poisoned input rows, a poisoned result arena, guards on both sides) and judged by the same
check functions.  Every fault must be reported WITH ITS PLACE: which guard, or which row and index (row and column of an integer table).  The stand-ins: a
framing + FFT kernel over strided rows, the mask compaction of kernels_peaks.hip (u8 mask, s32 [size][rank] table, -1 fill in 16-byte
groups) and a 2-D tile writer of two columns per thread."""
import numpy as np
import pytest

import extents as E
from oracle import nx_oracle as O

B, N, HOP, K, M = 5, 64, 16, 64, 9
L = (M - 1) * HOP + N + 3          # three samples behind the last frame: the row end is not the last frame's end
W = O.hann(N).astype(np.float32)


def standin_stft(xmem, x0, length, batch, stride, zmem, z0, fault=None):
    """framing + FFT the way a kernel addresses memory: flat element arrays and the index of the first element"""
    frames = (length - N) // HOP + 1
    for r in range(batch):
        row = x0 + r * (length if fault == "dense rows" else stride)
        for m in range(frames):
            s = row + m * HOP
            fr = xmem[s:s + N].copy()
            if fault == "gap into last frame" and r == 2 and m == frames - 1:
                fr[N - 1] += 0.0 * xmem[row + length]          # the first gap element, weight zero: only a NaN shows
            if fault == "read before row 0" and r == 0 and m == 0:
                fr[0] += 0.0 * xmem[x0 - 1]
            z = np.fft.fft(fr.astype(np.float64) * W, K).astype(np.complex64)
            o = z0 + (r * frames + m) * K
            if fault == "one unwritten" and (r, m) == (3, 4):
                zmem[o:o + 17] = z[:17]
                zmem[o + 18:o + K] = z[18:]
                continue
            zmem[o:o + K] = z
    if fault == "store past":
        zmem[z0 + batch * frames * K] = 1.0
    if fault == "store before":
        zmem[z0 - 1] = 1.0
    if fault == "modifies input":
        xmem[x0 + stride + 7] = 0.0


def run(fault, d=3, offset=0):
    x = O.synth_signal(L, seed=11, channels=B)
    xin = E.Arena("x", np.float32, B, L, L + d, offset_elems=offset, data=x)
    out = E.Arena("z", np.complex64, B, M * K)
    ximg, zimg = xin.image.copy(), out.image.copy()
    standin_stft(xin.view(ximg), xin.first, L, B, L + d, out.view(zimg), out.first, fault)
    ref = O.stft(x, W, overlap_length=N - HOP, fft_length=K)[0].reshape(B, M * K)
    return E.findings([(xin, ximg)], out, zimg, expected=ref, tol=1e-5, unit=K)


@pytest.mark.parametrize("d", [0, 1, 2, 3, 4, 37, 64])
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_a_correct_stand_in_passes(d, offset):
    assert run(None, d, offset) == []


@pytest.mark.parametrize("fault,place", [
    ("dense rows", "z: row 1, frame 0, index 0 is not finite, the reference is finite"),
    ("gap into last frame", f"z: row 2, frame {M - 1}, index 0 is not finite"),
    ("read before row 0", "z: row 0, frame 0, index 0 is not finite"),
    ("store past", "z: back guard, 0 bytes past the tensor holds 0x3F800000"),
    ("store before", "z: front guard, 4 bytes before the tensor holds 0x00000000"),
    ("one unwritten", "result element never written — z: row 3, index 273"),
    ("modifies input", "input modified — x: row 1, index 7"),
])
def test_a_planted_fault_is_reported_with_its_place(fault, place):
    found = run(fault)
    assert found, fault
    assert any(place in f for f in found), (fault, found)
    with pytest.raises(E.ExtentError):
        x = E.Arena("x", np.float32, 1, 4, data=np.zeros(4))
        bad = x.image.copy()
        bad[0] = 0
        E.verify([(x, bad)], x, x.image)


def test_dense_row_indexing_shows_in_values_even_without_a_gap_element_in_reach():
    """rows read from r * L: row 1 starts d elements early — without the NaN the values alone must fail the bound"""
    x = O.synth_signal(L, seed=11, channels=B)
    xin = E.Arena("x", np.float32, B, L, L + 3, data=x)
    v = xin.view()
    v[np.isnan(v)] = 0.25                                    # finite gaps: only the value check is left
    out = E.Arena("z", np.complex64, B, M * K)
    zimg = out.image.copy()
    standin_stft(xin.view(), xin.first, L, B, L + 3, out.view(zimg), out.first, "dense rows")
    ref = O.stft(x, W, overlap_length=N - HOP, fft_length=K)[0].reshape(B, M * K)
    found = E.findings([], out, zimg, expected=ref, tol=1e-5, unit=K)
    assert len(found) == 1 and "z: row " in found[0] and "error" in found[0], found


def test_the_pattern_is_a_nan_in_every_element_type_and_the_layout_keeps_its_promises():
    for dt in (np.float32, np.complex64, np.float64, np.complex128):
        for off in (0, 1, 2, 3):
            a = E.Arena("t", dt, 3, 10, 13, offset_elems=off)
            assert np.isnan(a.view()).all()
            assert a.offset_bytes == E.GUARD + off * np.dtype(dt).itemsize and a.image.size * 4 - a.offset_bytes - 39 * np.dtype(dt).itemsize == E.GUARD
            a.fill(np.ones((3, 10)))
            t = a.view()[a.first:a.first + 39].reshape(3, 13)
            assert np.all(t[:, :10] == 1) and np.isnan(t[:, 10:]).all() and np.array_equal(a.tensor(), np.ones((3, 10), dt))
    a = E.Arena("t", np.float64, 2, 4, 6)
    assert a.locate(0) == "t: front guard, 4096 bytes before the tensor"
    assert a.locate(a.lead + 2 * 5 + 1) == "t: gap after row 0, element 1 (word 1 of the element)"
    assert a.locate(a.lead + 2 * 6 + 3) == "t: row 1, index 1 (word 1 of the element)"
    assert a.locate(a.lead + 2 * 10) == "t: back guard, 0 bytes past the tensor"
    assert a.locate(a.lead + 2 * 12) == "t: back guard, 16 bytes past the tensor"


# ------------------------------------------------------------------------------- one-byte inputs, integer tables, 2-D tiles
SHAPE = (3, 1371)                  # 4113 bytes: 4113 % 4 = 1, three bytes of tail gap behind the mask
TOTAL = SHAPE[0] * SHAPE[1]


def standin_nonzero(mmem, m0, shape, imem, i0, vmem, v0, fault=None):
    """the compaction of kernels_peaks.hip the way it addresses memory: the marks of a u8 mask, their coordinates at rows 0 .. valid - 1
    of the s32 [size][rank] table, then -1 over the elements [s0, s1) = [valid rank, size rank): scalars up to the first 16-byte
    boundary a0, groups of four to the last one a1, scalars again — the groups only when the table starts on such a boundary"""
    total, rank = int(np.prod(shape)), len(shape)
    hits = np.flatnonzero(mmem[m0:m0 + total + (1 if fault == "reads a tail byte" else 0)] != 0)
    valid = len(hits)
    vmem[v0] = valid
    s0, s1 = valid * rank, total * rank
    a0 = a1 = s1
    if i0 % 4 == 0:
        a0, a1 = (s0 + 3) & ~3, s1 & ~3
        if a0 > a1:
            a0 = a1 = s1
        elif fault == "fill one group long":
            a1 += 4
    if fault != "no scalar head":
        imem[i0 + s0:i0 + a0] = -1
    imem[i0 + a0:i0 + a1] = -1
    imem[i0 + a1:i0 + s1] = -1
    for p, e in enumerate(hits.tolist()):
        row = i0 + (p + 1 if fault == "last row at valid" and p == valid - 1 else p) * rank
        for d in range(rank - 1, -1, -1):
            imem[row + d] = e % shape[d]
            e //= shape[d]


def run_nonzero(fault, density=0.5, seed=0, shape=SHAPE, offset=0, moffset=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    total = int(np.prod(shape))
    m = (rng.random(total) < density).astype(np.uint8) * rng.integers(1, 256, total).astype(np.uint8)
    mask = E.Arena("mask", np.uint8, 1, total, offset_elems=moffset, data=m)
    idx = E.Arena("indices", np.int32, total, len(shape), offset_elems=offset)
    val = E.Arena("valid", np.uint32, 1, 1)
    mimg, iimg, vimg = mask.image.copy(), idx.image.copy(), val.image.copy()
    standin_nonzero(mask.view(mimg), mask.first, shape, idx.view(iimg), idx.first, val.view(vimg), val.first, fault)
    want = np.full((total, len(shape)), -1, np.int32)
    hits = np.argwhere(m.reshape(shape))
    want[:len(hits)] = hits
    return E.findings([(mask, mimg)], idx, iimg, table=want) + E.findings([], val, vimg, table=[len(hits)]), len(hits)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", [SHAPE, (TOTAL,), (3, 5, 7)])
def test_a_correct_compaction_stand_in_passes_in_every_fill_phase(shape, offset):
    phases = set()
    for seed in range(16):
        for density in (0.0, 0.5, 1.0):
            found, valid = run_nonzero(None, density, seed, shape, offset, moffset=seed % 4)
            assert found == [], (shape, offset, seed, density, found)
            phases.add(valid * len(shape) % 4)
    assert phases == ({0, 1, 2, 3} if len(shape) % 2 else {0, 2})      # an even rank has an even s0


def _seed_with(phase, rank_shape=SHAPE):
    """a seed whose count leaves the fill's first element `phase` elements into a 16-byte group"""
    for seed in range(64):
        rng = np.random.Generator(np.random.PCG64(seed))
        if int(np.sum(rng.random(TOTAL) < 0.5)) * len(rank_shape) % 4 == phase:
            return seed
    raise AssertionError(phase)


def test_planted_faults_of_the_compaction_are_reported_with_their_place():
    seed = _seed_with(2)                                   # s0 = 2 valid is 2 mod 4: the fill has a two-element scalar head
    _, valid = run_nonzero(None, seed=seed)
    found, _ = run_nonzero("fill one group long", seed=seed)      # s1 = 8226: the last group [8224, 8228) runs two elements past the table
    assert "store outside the result — indices: back guard, 0 bytes past the tensor holds 0xFFFFFFFF" in found, found
    assert any("back guard, 4 bytes past" in f for f in found) and len(found) == 2, found
    found, _ = run_nonzero("no scalar head", seed=seed)           # rows [valid, valid + 1) stay unwritten
    assert found == [f"result element never written — indices: row {valid}, column 0",
                     f"result element never written — indices: row {valid}, column 1"], found
    found, _ = run_nonzero("last row at valid", seed=seed)
    assert f"result element never written — indices: row {valid - 1}, column 0" in found, found
    assert any(f.startswith(f"indices: row {valid}, column 0 holds ") and f.endswith("expected -1") for f in found), found
    found, _ = run_nonzero("reads a tail byte", seed=seed)        # byte 4113 of the mask's arena: the pattern, non-zero -> one mark too many
    assert f"indices: row {valid}, column 0 holds 0, expected -1" in found, found          # flat index 4113 of (3, 1371) wraps to (0, 0)
    assert f"valid: row 0, column 0 holds {valid + 1}, expected {valid}" in found, found


def test_the_byte_arena_keeps_its_promises():
    for off in (0, 1, 2, 3):
        a = E.Arena("mask", np.uint8, 3, 1371, offset_elems=off, data=np.zeros((3, 1371)))
        assert a.offset_bytes == E.GUARD + off and a.image.nbytes == E.GUARD + (off + TOTAL + 3) // 4 * 4 + E.GUARD
        b = a.view()
        assert not b[a.first:a.first + TOTAL].any() and b[:a.first].all() and b[a.first + TOTAL:].all()     # every pattern byte is non-zero
        assert np.array_equal(a.tensor(), np.zeros((3, 1371), np.uint8))
        assert E.guard_findings(a, a.image) == [] and E.unchanged_findings(a, a.image) == []
    a = E.Arena("mask", np.uint8, 3, 1371, data=np.zeros((3, 1371)))
    img = a.image.copy()
    img.view(np.uint8)[a.first + TOTAL] = 0                  # one byte behind the mask
    assert E.guard_findings(a, img) == ["store outside the result — mask: tail gap, 0 bytes past the tensor holds 0x00"]
    assert E.unchanged_findings(a, img) == ["input modified — mask: tail gap, 0 bytes past the tensor: 0xDE became 0x00"]
    img = a.image.copy()
    img.view(np.uint8)[a.first + TOTAL + 3] = 1
    assert E.guard_findings(a, img) == ["store outside the result — mask: back guard, 3 bytes past the tensor holds 0x01"]
    img = a.image.copy()
    img.view(np.uint8)[a.first + 1371 + 5] = 7
    assert E.unchanged_findings(a, img) == ["input modified — mask: row 1, index 5: 0x00 became 0x07"]
    assert a.locate_byte(a.first - 2) == "mask: front guard, 2 bytes before the tensor"


def test_the_pattern_is_no_index_of_any_table():
    assert np.array([E.POISON], np.uint32).view(np.int32)[0] not in (-1,) and E.POISON > 2 ** 30      # no coordinate, no count of these shapes
    a = E.Arena("indices", np.int32, 5, 3)
    img = a.image.copy()
    assert len(E.table_unwritten_findings(a, img)) == 5 and E.table_findings(a, a.tensor(img), np.zeros((5, 3))) == []
    a.view(img)[a.first:a.first + 15] = np.arange(15)
    want = np.arange(15).reshape(5, 3)
    want[4, 1] = 0
    assert E.findings([], a, img, table=want) == ["indices: row 4, column 1 holds 13, expected 0"]


def standin_tile(xmem, x0, H, W, omem, o0, fault=None):
    """a 2-D tile writer, two adjacent outputs per thread like k_median_tile: thread t of a row owns columns j0 = 2 t and j0 + 1, the second
    one under `if (j0 + 1 < W)`.  The value is the median of the clamped 1 x 3 window (filters_oracle.median's rule)."""
    def med(i, j):
        s = min(j, W - 3)
        return np.sort(xmem[x0 + i * W + s:x0 + i * W + s + 3])[1]
    for i in range(H):
        for j0 in range(0, W, 2):
            if fault == "skips the odd last column" and j0 + 1 >= W:
                continue
            omem[o0 + i * W + j0] = med(i, j0)
            if j0 + 1 < W or fault == "no second-column guard":
                omem[o0 + i * W + j0 + 1] = med(i, min(j0 + 1, W - 1))


def run_tile(fault, W):
    import filters_oracle as F
    H = 7
    x = O.synth_signal(H * W, seed=W).reshape(H, W)
    xin, out = E.Arena("x", np.float32, H, W, data=x), E.Arena("out", np.float32, H, W)
    ximg, oimg = xin.image.copy(), out.image.copy()
    standin_tile(xin.view(ximg), xin.first, H, W, out.view(oimg), out.first, fault)
    ref = F.median(x, (1, 3))
    return E.findings([(xin, ximg)], out, oimg, expected=ref, same_bits_as=ref)


def test_a_tile_writer_of_two_columns_per_thread():
    assert run_tile(None, 131) == [] and run_tile(None, 130) == []
    assert run_tile("skips the odd last column", 130) == []                     # an even width has no such column
    found = run_tile("skips the odd last column", 131)
    assert found[:4] == [f"result element never written — out: row {r}, index 130" for r in range(4)] and "7 result components" in found[4], found
    found = run_tile("no second-column guard", 131)                             # column 131 of row i is column 0 of row i + 1; of the last row, the guard
    assert "store outside the result — out: back guard, 0 bytes past the tensor holds" in found[0], found
    assert run_tile("no second-column guard", 130) == []


def test_bit_comparison_names_the_frame():
    a = E.Arena("z", np.complex64, 2, 8)
    one = (np.arange(16) + 0j).astype(np.complex64).reshape(2, 8)
    two = one.copy()
    two[1, 5] = 13 + 1e-7j
    assert E.bit_findings(a, one, one) == []
    assert E.bit_findings(a, two, one, unit=4) == ["z: row 1, frame 1, index 1 differs in bits"]
