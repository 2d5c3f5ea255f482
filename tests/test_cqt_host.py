"""Spectral.cqt / vqt without a GPU: the frame count, the refusals through Python and through the C entry, the length arithmetic and the
plan of cqt.mfma (tiles, sub-panels, LDS bytes, and that every tap of a bank lands in a table cell of its own)."""
import ctypes as C

import numpy as np
import pytest

from nx_signal_amd import ArgumentError, NxSignalUnsupported, _lib, spectral


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_frame_count():
    lib = _lib.load()
    assert [lib.nxsig_cqt_frames(n, h) for n, h in [(200, 16), (1500, 64), (900, 37), (6000, 512), (40, 64), (512, 16)]] == [13, 24, 25, 12, 1, 33]
    assert lib.nxsig_cqt_frames(0, 16) == _lib.ERR_INVALID_ARG and lib.nxsig_cqt_frames(16, 0) == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("kwargs,what", [
    (dict(hop=0), "hop must be an integer >= 1"), (dict(hop=2.0), "hop must be an integer"), (dict(n_bins=0), "n_bins must be an integer >= 1"),
    (dict(bins_per_octave=True), "bins_per_octave must be an integer"), (dict(fmin=0), "fmin must be a finite number > 0"),
    (dict(sr=float("inf")), "sr must be a finite number"), (dict(gamma=-1.0), "gamma must be a finite number >= 0"),
    (dict(n_bins=108), "below sr / 2"), (dict(fmin=2000, n_bins=20, filter_scale=0.01), "at least 2 samples"),
    (dict(output="real"), "output must be one of"), (dict(norm=3), "norm must be 1, 2 or None"), (dict(norm=True), "norm must be"),
    (dict(scale=1), "scale must be a boolean"),
])
def test_refused_by_python(kwargs, what):
    with pytest.raises(ArgumentError, match=what):
        spectral.vqt(np.ones(400, np.float32), **kwargs)


def test_refused_operands():
    with pytest.raises(NxSignalUnsupported, match="float64"):
        spectral.cqt(np.ones(400))
    for dtype in (np.complex64, np.int32):
        with pytest.raises(ArgumentError, match="f32"):
            spectral.cqt(np.ones(400, dtype))


def c_entry(batch=1, n=100, stride=100, hop=16, lo=(-4, -2), count=(8, 4), kind=0, taps=None):
    """nxsig_cqt_f32 with a null context: the checks come ahead of it, so it is never looked at"""
    x, out = np.ones(max(stride, 1) * max(batch, 1), np.float32), np.empty(4096, np.complex64)
    lo, count = np.array(lo, np.int64), np.array(count, np.int32)
    taps = np.ones(max(int(count.sum()), 1), np.complex64) if taps is None else taps
    return _lib.load().nxsig_cqt_f32(None, p(x), batch, n, stride, hop, len(lo), p(lo), p(count), p(taps), p(out), kind, _lib.HOST)


@pytest.mark.parametrize("kwargs,what", [
    (dict(n=0, stride=0), "length must be >= 1"), (dict(hop=0), "hop must be >= 1"), (dict(batch=-1), "batch must be >= 0"),
    (dict(stride=99), "batch_stride must be >= length"), (dict(lo=(), count=()), "n_bins must be >= 1"), (dict(count=(8, 1)), "at least 2 taps"),
    (dict(kind=3), "output_kind must be"), (dict(taps=np.full(12, np.nan, np.complex64)), "the taps must be finite"),
])
def test_refused_by_the_c_entry(kwargs, what):
    assert c_entry(**kwargs) == _lib.ERR_INVALID_ARG and what in _lib.last_error()


def test_the_c_entry_accepts_the_limits_up_to_the_context():
    assert c_entry() == _lib.ERR_INVALID_ARG and "null context" in _lib.last_error()
    assert c_entry(lo=(0,), count=((1 << 24) + 1,), taps=np.ones(1, np.complex64)) == _lib.ERR_UNSUPPORTED and "2^24 taps" in _lib.last_error()


@pytest.mark.parametrize("args", [(8000, 100, 40, 12, 1.0, 0.0), (22050, 32.703, 84, 12, 0.5, 7.5)])
def test_lengths_against_the_formulas(args):
    sr, fmin, n, B, q, gamma = args
    ell, lo, count = spectral.cqt_lengths(*args)
    f = spectral.cqt_frequencies(n, fmin, B)
    assert np.allclose(f, [fmin * 2 ** (k / B) for k in range(n)], rtol=1e-15) and lo.dtype == np.int64 and count.dtype == np.int32
    for k in range(n):
        want = q * sr / ((2 ** (1 / B) - 1) * f[k] + gamma)
        assert abs(ell[k] - want) <= 1e-12 * want and lo[k] == np.floor(-want / 2) and count[k] == np.floor(want / 2) - 1 - lo[k] + 1


# (sr, fmin, n_bins, B) of the GPU test's shapes and of the benchmark's first: N_max, bin tiles, sub-panels of 64 samples
@pytest.mark.parametrize("args,n_max,tiles,subs", [((8000, 500, 12, 12), 269, 1, 5), ((8000, 100, 40, 12), 1345, 3, 35),
                                                   ((16000, 110, 70, 24), 4963, 5, 191), ((22050, 32.7, 24, 12), 11341, 2, 249),
                                                   ((22050, 32.703, 84, 12), 11339, 6, 296)])
def test_plan(args, n_max, tiles, subs):
    _, lo, count = spectral.cqt_lengths(*args)
    n, total = len(lo), int(count.sum())
    summary, tl, cells = np.zeros(4, np.int64), np.zeros((tiles, 4), np.int64), np.full(total, -1, np.int64)
    assert _lib.load().nxsig_cqt_plan(n, p(lo), p(count), p(summary), p(tl), p(cells)) == total and count.max() == n_max
    assert list(summary) == [tiles, subs, subs * 1024, 128 * 68 * 4 + 8192] and summary[3] <= 160 * 1024 // 3
    assert list(tl[:, 0]) == [16] * (n // 16) + ([n % 16] if n % 16 else []) and tl[:, 2].sum() == subs
    first = tl[:, 3]   # bins ascend in frequency, so a tile's longest bin is its first and covers the others
    assert list(first) == list(range(0, n, 16)) and np.array_equal(tl[:, 1], lo[first]) and np.array_equal(tl[:, 2], -(-count[first] // 64))
    assert cells.min() >= 0 and cells.max() < summary[2] and len(np.unique(cells)) == total   # every (k, n) in exactly one cell
    # a tap's cell: sub-panel u of its tile, matrix step s, lane 16 g + m, for sample 64 u + 16 g + s past the tile's first n
    k, j = n - 1, 3
    at, m, tile = int(count[:k].sum()) + j, k % 16, k // 16
    i = lo[k] + j - tl[tile, 1]
    assert cells[at] == ((tl[:tile, 2].sum() + i // 64) * 16 + i % 16) * 64 + i % 64 // 16 * 16 + m
