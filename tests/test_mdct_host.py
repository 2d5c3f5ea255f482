"""Transforms.mdct / imdct: what needs no GPU — the frame count, the argument errors and the Princen-Bradley windows."""
import numpy as np
import pytest
import scipy.signal.windows as W

from nx_signal_amd import ArgumentError, NxSignalUnsupported, _lib, transforms as T


@pytest.mark.parametrize("L, N, pad", [(512, 512, False), (1000, 512, False), (1023, 512, False), (1024, 512, False), (36, 36, False),
                                       (1, 512, True), (256, 512, True), (257, 512, True), (1000, 512, True), (5, 4, True)])
def test_frame_count(L, N, pad):
    M = N // 2
    want = -(-L // M) + 1 if pad else (L - N) // M + 1
    assert _lib.load().nxsig_mdct_frames(L, N, int(pad)) == want


def test_argument_errors():
    x = np.zeros((2, 64), np.float32)
    with pytest.raises(ArgumentError, match="multiple of 4"):
        T.mdct(x, np.ones(18, np.float32))
    with pytest.raises(ArgumentError, match="window of 32 samples"):
        T.imdct(np.zeros((2, 3, 16), np.float32), np.ones(36, np.float32))
    with pytest.raises(ArgumentError, match="shorter than the frame length"):
        T.mdct(x, np.ones(128, np.float32))
    with pytest.raises(NxSignalUnsupported, match="float64"):
        T.mdct(x.astype(np.float64), np.ones(32, np.float32))
    with pytest.raises(NxSignalUnsupported, match="complex64"):
        T.imdct(np.zeros((3, 16), np.complex64), np.ones(32, np.float32))
    with pytest.raises(ArgumentError, match="norm must be"):
        T.mdct(x, np.ones(32, np.float32), norm="backward")
    lib = _lib.load()
    assert lib.nxsig_mdct_frames(100, 18, 0) == -1 and lib.nxsig_mdct_frames(100, 512, 0) == -1   # NXSIG_ERR_INVALID_ARG


@pytest.mark.parametrize("N", [4, 36, 512, 2048])
@pytest.mark.parametrize("kind", ["sine", "vorbis", "kbd"])
def test_windows_are_princen_bradley(kind, N):
    w = T.mdct_window(kind, N)
    assert w.dtype == np.float32 and w.shape == (N,)
    assert np.abs(w.astype(np.float64)[:N // 2] ** 2 + w.astype(np.float64)[N // 2:] ** 2 - 1).max() <= 1e-6
    if kind == "kbd":   # SciPy's definition, to the last f32 bit or one ulp
        ref = W.kaiser_bessel_derived(N, np.pi * 4.0).astype(np.float32)
        assert np.all(np.abs(w - ref) <= np.spacing(ref))
