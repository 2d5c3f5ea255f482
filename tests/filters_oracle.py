"""numpy restatement of NxSignal.Filters.median/2 and wiener/2 (lib/nx_signal/filters.ex:17-55, :81-110, :281-303) — the rules
DESIGN.md section 3.8 states, vectorised.  It reproduces every literal of tests/golden/filters_vectors.json with == and is what the
GPU tiers are compared against.

median: the window of output i starts at min(i_d, n_d - k_d) on every axis (Nx.slice clamps its start indices), is not padded
and has k_d elements along axis d.  Values are ordered like np.sort (NaN above +Inf, -0.0 == +0.0; a zero median is returned as
+0.0).  Odd windows: the middle order statistic; even windows: (a + b) / 2 of the two middle ones, in f32 for f32 inputs and in
f64 (rounded once to f32) for every other input.  The result is always f32.

wiener: S1 / S2 = correlate(t, ones) / correlate(t * t, ones), mode :same (zero padding (k-1) - div(k-1, 2) low, div(k-1, 2)
high), accumulated in f64 from 0.0 over the window in row-major order; l_mean = S1 / size, l_var = S2 / size - l_mean^2,
noise = sequential mean of l_var when not given; out = l_var < noise ? l_mean : (t - l_mean) * (1 - noise / l_var) + l_mean in
f64, cast back to the input type."""
from __future__ import annotations

import itertools

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def median(t, kernel_shape, chunk_elems=1 << 25):
    x = np.asarray(t)
    ks = tuple(int(k) for k in kernel_shape)
    assert len(ks) == x.ndim and all(1 <= k <= n for k, n in zip(ks, x.shape))
    ct = np.float32 if x.dtype == np.float32 else np.float64
    x = x.astype(ct)
    x = np.where(x == 0, ct(0), x)   # -0.0 -> +0.0 (NaN passes)
    v = sliding_window_view(x, ks)
    K = int(np.prod(ks))
    out = np.empty(x.shape, np.float32)
    # the leading axis in chunks (the window copy is K x the input)
    n0 = x.shape[0]
    step = max(1, chunk_elems // max(1, K * (x.size // n0)))
    idx_rest = [np.minimum(np.arange(n), n - k) for n, k in zip(x.shape[1:], ks[1:])]
    for a in range(0, n0, step):
        rows = np.minimum(np.arange(a, min(n0, a + step)), n0 - ks[0])
        w = v[np.ix_(rows, *idx_rest)].reshape(len(rows), *x.shape[1:], K)
        s = np.sort(w, axis=-1)
        if K % 2:
            m = s[..., K // 2]
        else:
            with np.errstate(invalid="ignore", over="ignore"):   # -Inf + Inf is NaN, like the kernels' mean
                m = (s[..., K // 2 - 1] + s[..., K // 2]) / ct(2)
        out[a:a + len(rows)] = m.astype(np.float32)
    return out


def box_sums(x, ks):
    """S1, S2 of the :same correlation with ones, f64, window offsets in row-major order (the reference's per-output order)"""
    lo = [(k - 1) - (k - 1) // 2 for k in ks]
    hi = [(k - 1) // 2 for k in ks]
    xp = np.pad(x, list(zip(lo, hi)))
    x2p = xp * xp
    s1 = np.zeros_like(x)
    s2 = np.zeros_like(x)
    for off in itertools.product(*[range(k) for k in ks]):
        sl = tuple(slice(o, o + n) for o, n in zip(off, x.shape))
        s1 += xp[sl]
        s2 += x2p[sl]
    return s1, s2


def wiener(t, kernel_size=3, noise=None, return_noise=False):
    t = np.asarray(t)
    x = t.astype(np.float64)
    ks = (int(kernel_size),) * x.ndim if isinstance(kernel_size, (int, np.integer)) else tuple(int(k) for k in kernel_size)
    size = float(np.prod(ks))
    s1, s2 = box_sums(x, ks)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        l_mean = s1 / size
        l_var = s2 / size - l_mean * l_mean
        if noise is None:
            noise = float(np.cumsum(l_var.reshape(-1))[-1] / l_var.size)   # sequential order
        noise = float(noise)
        res = (x - l_mean) * (1.0 - noise / l_var)
        out = np.where(l_var < noise, l_mean, res + l_mean)
    out = out.astype(t.dtype if t.dtype in (np.float32, np.float64) else np.float64)
    return (out, noise) if return_noise else out
