"""Filters.hilbert in numpy f64: the definition of include/nxsig.h, word for word, on np.fft.  The GPU results are compared with this on
the same samples (tests/test_gpu_hilbert.py); tests/test_hilbert_host.py holds it to recorded SciPy 1.15.3 results."""
import numpy as np

OUTPUTS = ("analytic", "envelope", "quadrature")


def gain(N):
    """h[0 .. N): 1 at 0 (and at N / 2 for an even N), 2 on the positive frequencies in between, 0 elsewhere"""
    h = np.zeros(N, np.float64)
    h[0] = 1.0
    if N % 2 == 0:
        h[N // 2] = 1.0
        h[1:N // 2] = 2.0
    else:
        h[1:(N + 1) // 2] = 2.0
    return h


def hilbert(x, N=None, output="analytic"):
    """rows along the last axis of a real array, in double; a row with a non-finite sample among those used comes back all NaN"""
    x = np.asarray(x)
    assert x.dtype.kind == "f" and output in OUTPUTS
    L = x.shape[-1]
    N = L if N is None else int(N)
    rows = np.zeros(x.shape[:-1] + (N,), np.float64)
    used = min(L, N)
    rows[..., :used] = x[..., :used]
    with np.errstate(all="ignore"):
        a = np.fft.ifft(np.fft.fft(rows, axis=-1) * gain(N), axis=-1)
    bad = ~np.isfinite(rows).all(axis=-1)
    a[bad] = complex(np.nan, np.nan)
    if output == "analytic":
        return a
    return np.abs(a) if output == "envelope" else a.imag.copy()
