"""Filters.resample_poly in numpy f64, straight from the definition (include/nxsig.h: nxsig_resample_poly): the ratio reduced, then for
every output m the direct sum  y[m] = sum_j x[j] h[m down + half - j up]  over the j in [0, n) whose tap index lies in [0, L) — those
products and no others, so an Inf / NaN sample shows in exactly the outputs it belongs to.  `h` are the taps with the gain included.
design(up, down, window) is the default anti-alias filter in f64 (before the single rounding to f32)."""
import math

import numpy as np

import nx_signal_amd as S


def reduce(up, down):
    g = math.gcd(int(up), int(down))
    return int(up) // g, int(down) // g


def length(n, up, down):
    up, down = reduce(up, down)
    return -((-int(n) * up) // down)


def design(up, down, window=("kaiser", 5.0)):
    up, down = reduce(up, down)
    big = max(up, down)
    return up * S.filters.firwin(20 * big + 1, [1.0 / big], window=window, sampling_rate=2.0, type="f64")


def resample_poly(x, up, down, h):
    """x [..., n] real or complex, h 1-D real (gain included); f64 / c128 out"""
    up, down = reduce(up, down)
    x = np.asarray(x)
    x = x.astype(np.complex128 if x.dtype.kind == "c" else np.float64)
    if up == down:
        return x.copy()
    h = np.asarray(h, np.float64)
    n, L = x.shape[-1], h.shape[0]
    half = (L - 1) // 2
    y = np.zeros(x.shape[:-1] + (length(n, up, down),), x.dtype)
    for m in range(y.shape[-1]):
        c = m * down + half
        j_lo = max(0, -((L - 1 - c) // up))          # ceil((c - (L - 1)) / up)
        j_hi = min(n - 1, c // up)
        if j_hi < j_lo:
            continue
        j = np.arange(j_hi, j_lo - 1, -1)            # ascending tap index, the kernels' order
        with np.errstate(invalid="ignore", over="ignore"):
            y[..., m] = (x[..., j] * h[c - j * up]).sum(axis=-1)
    return y


def resample_poly_by_taps(x, up, down, h):
    """the same sums formed for all outputs at once, one tap index t of y[m] = sum_t x[q - t] h[r + t up] per pass (ascending t: the same
    order of additions as resample_poly, term by term; a term that does not exist adds nothing and is never multiplied).  What the GPU
    tests use for long rows; tests/test_resample_host.py holds it to resample_poly."""
    up, down = reduce(up, down)
    x = np.asarray(x)
    x = x.astype(np.complex128 if x.dtype.kind == "c" else np.float64)
    if up == down:
        return x.copy()
    h = np.asarray(h, np.float64)
    n, L = x.shape[-1], h.shape[0]
    c = np.arange(length(n, up, down), dtype=np.int64) * down + (L - 1) // 2
    q, r = c // up, c % up
    y = np.zeros(x.shape[:-1] + c.shape, x.dtype)
    for t in range(-(-L // up)):
        j, i = q - t, r + t * up
        ok = (j >= 0) & (j < n) & (i < L)
        if not ok.any():
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            y[..., ok] += x[..., j[ok]] * h[i[ok]]
    return y


def nmax_err(got, want):
    """normalised max error of one result against the oracle, per row: max |got - want| / max |want| over each row"""
    got, want = np.asarray(got), np.asarray(want)
    g = got.reshape(-1, got.shape[-1]).astype(np.complex128)
    w = want.reshape(-1, want.shape[-1]).astype(np.complex128)
    scale = np.maximum(np.abs(w).max(axis=-1), 1e-300)
    return float((np.abs(g - w).max(axis=-1) / scale).max())
