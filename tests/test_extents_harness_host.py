"""tests/extents.py catches what it is for: numpy stand-ins for a kernel, one correct and seven with a planted fault, run through the
arena layout the GPU tests use (strided poisoned input rows, a poisoned result arena, guards on both sides) and judged by the same
check functions.  Every fault must be reported WITH ITS PLACE: which guard, or which row and index."""
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


def test_bit_comparison_names_the_frame():
    a = E.Arena("z", np.complex64, 2, 8)
    one = (np.arange(16) + 0j).astype(np.complex64).reshape(2, 8)
    two = one.copy()
    two[1, 5] = 13 + 1e-7j
    assert E.bit_findings(a, one, one) == []
    assert E.bit_findings(a, two, one, unit=4) == ["z: row 1, frame 1, index 1 differs in bits"]
