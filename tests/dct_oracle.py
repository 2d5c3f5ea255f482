"""The definition of Transforms.dct / idct (include/nxsig.h) in f64 numpy: the cosine matrix of an integer argument reduced mod 4 n, so
the oracle rounds no argument either.  Rows are truncated or zero-padded to n along the last axis."""
import functools

import numpy as np

TYPES = (2, 3)
NORMS = (None, "ortho", "forward")


def _cos(m, n):
    """cos(pi m / (2 n)) of an integer array m, reduced to [0, n] first"""
    m = np.asarray(m, np.int64) % (4 * n)
    m = np.where(m > 2 * n, 4 * n - m, m)
    sign = np.where(m > n, -1.0, 1.0)
    m = np.where(m > n, 2 * n - m, m)
    return np.where(m == n, 0.0, sign * np.cos(np.pi * m / (2.0 * n)))


@functools.lru_cache(maxsize=4)
def _matrix(n, type):
    """type 2: C[k][j] = cos(pi k (2 j + 1) / (2 n)); type 3: C[k][j] = cos(pi (2 k + 1) j / (2 n)).  Kept for the last few n: a test
    runs many rows against one matrix"""
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    return _cos(k * (2 * j + 1), n) if type == 2 else _cos((2 * k + 1) * j, n)


def resize(x, n):
    x = np.asarray(x, np.float64)
    L = x.shape[-1]
    n = L if n is None else int(n)
    return x[..., :n] if n <= L else np.concatenate([x, np.zeros(x.shape[:-1] + (n - L,))], axis=-1)


def dct(x, type=2, n=None, norm=None, keep=None):
    x = resize(x, n)
    n = x.shape[-1]
    if type == 2:
        y = 2.0 * x @ _matrix(n, 2).T
        if norm == "ortho":
            y[..., 0] *= np.sqrt(1.0 / (4 * n))
            y[..., 1:] *= np.sqrt(1.0 / (2 * n))
    elif type == 3:
        c = _matrix(n, 3)[:, 1:]
        if norm == "ortho":
            y = x[..., :1] / np.sqrt(n) + np.sqrt(2.0 / n) * (x[..., 1:] @ c.T)
        else:
            y = x[..., :1] + 2.0 * (x[..., 1:] @ c.T)
    else:
        raise ValueError(type)
    if norm == "forward":
        y = y / (2 * n)
    return y if keep is None else y[..., :keep]


INVERSE_NORM = {None: "forward", "backward": "forward", "forward": None, "ortho": "ortho"}


def idct(x, type=2, n=None, norm=None):
    return dct(x, 5 - type, n, INVERSE_NORM[norm])


def dct_fast(x, type=2, n=None, norm=None, keep=None):
    """the same numbers through np.fft in double (Makhoul's form), for rows whose n x n cosine matrix is too large to form: 65 536 points
    would take 34 GB.  tests/test_dct_host.py holds it to dct() on every recorded length; the GPU tests hold it to the definition at
    sampled coefficients of the rows they use it on (places())"""
    x = resize(x, n)
    n = x.shape[-1]
    k = np.arange(n)
    w = np.exp(1j * np.pi * k / (2.0 * n))
    if type == 2:
        i = np.arange(n)
        V = np.fft.fft(x[..., np.where(i < (n + 1) // 2, 2 * i, 2 * (n - 1 - i) + 1)], axis=-1)
        y = 2.0 * (np.conj(w) * V).real
        if norm == "ortho":
            y[..., 0] *= np.sqrt(1.0 / (4 * n))
            y[..., 1:] *= np.sqrt(1.0 / (2 * n))
        elif norm == "forward":
            y = y / (2 * n)
    else:
        x = x.copy()
        if norm == "ortho":
            x[..., 0] /= np.sqrt(n)
            x[..., 1:] *= np.sqrt(2.0 / n) / 2.0
        elif norm == "forward":
            x = x / (2 * n)
        xe = np.concatenate([x, np.zeros(x.shape[:-1] + (1,))], axis=-1)
        W = w * (x - 1j * xe[..., n - k])
        W[..., 0] = x[..., 0]
        u = np.fft.ifft(W, axis=-1).real * n
        y = u[..., np.where(k % 2 == 0, k // 2, n - 1 - (k - 1) // 2)]
    return y if keep is None else y[..., :keep]


def places(n):
    """coefficients at which a long row is also held to the definition: the first and last 16 and 64 spread over the row"""
    return np.arange(n) if n <= 96 else np.unique(np.concatenate([np.arange(16), n - 16 + np.arange(16), (np.arange(64) * (n - 1)) // 63]))


def dct_at(x, at, type=2, n=None, norm=None):
    """the definition at the coefficients `at` only (an len(at) x n matrix)"""
    x = resize(x, n)
    n = x.shape[-1]
    k, j = np.asarray(at, np.int64)[:, None], np.arange(n)[None, :]
    if type == 2:
        y = 2.0 * x @ _cos(k * (2 * j + 1), n).T
        if norm == "ortho":
            y = y * np.where(np.asarray(at) == 0, np.sqrt(1.0 / (4 * n)), np.sqrt(1.0 / (2 * n)))
    else:
        c = _cos((2 * k + 1) * j, n)[:, 1:]
        if norm == "ortho":
            y = x[..., :1] / np.sqrt(n) + np.sqrt(2.0 / n) * (x[..., 1:] @ c.T)
        else:
            y = x[..., :1] + 2.0 * (x[..., 1:] @ c.T)
    return y / (2 * n) if norm == "forward" else y
