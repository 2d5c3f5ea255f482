"""The definition of Filters.savgol_filter (include/nxsig.h) in f64 numpy, and the exact least-squares weights over the rationals.

    y[i] = sum_j k[j] ext(i - L + j),  L = W // 2 for an odd window, W // 2 - 1 for an even one

with k the correlation weights (savgol_coeffs(..., use="dot") at the default pos) and ext the row extended by `mode`; mode "interp"
extends with zeros and then replaces the first and last W // 2 outputs by the fit through the first / last W samples.  Nothing here
looks at the library."""
import functools
from fractions import Fraction
from math import factorial

import numpy as np

MODES = ("mirror", "constant", "nearest", "wrap", "interp")


def left(W):
    return W // 2 if W % 2 else W // 2 - 1


@functools.lru_cache(maxsize=None)
def _normal_inverse(W, p):
    """inverse of the normal matrix of the monomials over the centred points t_j = j - (W - 1) / 2, exact"""
    c = Fraction(W - 1, 2)
    t = [Fraction(j) - c for j in range(W)]
    powers = [[Fraction(1)] * W]
    for _ in range(2 * p):
        powers.append([a * b for a, b in zip(powers[-1], t)])
    s = [sum(row) for row in powers]
    m = p + 1
    a = [[s[r + q] for q in range(m)] + [Fraction(int(r == q)) for q in range(m)] for r in range(m)]
    for col in range(m):   # Gauss-Jordan over the rationals
        piv = next(r for r in range(col, m) if a[r][col] != 0)
        a[col], a[piv] = a[piv], a[col]
        d = a[col][col]
        a[col] = [v / d for v in a[col]]
        for r in range(m):
            if r != col and a[r][col] != 0:
                f = a[r][col]
                a[r] = [v - f * w for v, w in zip(a[r], a[col])]
    return [row[m:] for row in a], powers[:m]


def exact_weights(W, p, deriv=0, delta=1.0, pos=None, use="dot"):
    """savgol_coeffs as Fractions: the weight of window sample j in the deriv-th derivative, at window position pos, of the degree-p
    least-squares polynomial through the W samples, divided by delta ** deriv"""
    if deriv > p:
        return [Fraction(0)] * W
    if pos is None:
        pos = Fraction(W // 2) if W % 2 else Fraction(W // 2) - Fraction(1, 2)
    inv, powers = _normal_inverse(W, p)
    t0 = Fraction(pos) - Fraction(W - 1, 2)
    v = [Fraction(factorial(m) // factorial(m - deriv)) * t0 ** (m - deriv) if m >= deriv else Fraction(0) for m in range(p + 1)]
    u = [sum(inv[r][q] * v[q] for q in range(p + 1)) for r in range(p + 1)]
    scale = Fraction(delta) ** deriv
    w = [sum(u[m] * powers[m][j] for m in range(p + 1)) / scale for j in range(W)]
    return w[::-1] if use == "conv" else w


@functools.lru_cache(maxsize=None)
def weights(W, p, deriv=0, delta=1.0):
    """the exact correlation weights at the default pos, rounded to double"""
    return np.array([float(v) for v in exact_weights(W, p, deriv, delta)], np.float64)


@functools.lru_cache(maxsize=None)
def edge_table(W, p, deriv=0, delta=1.0):
    """E[h][W] of mode "interp": row i is the deriv-th derivative at position i of the fit through W samples.  Formed in double on the
    Legendre basis over [-1, 1] (orthogonal enough at degree <= 15 for a QR to lose nothing that matters: rows agree with the exact
    rational ones to 1e-13 of their largest entry, tests/test_savgol_host.py)"""
    h = W // 2
    if h == 0 or deriv > p:
        return np.zeros((h, W))
    half = (W - 1) / 2.0
    x = (np.arange(W) - half) / half
    q, r = np.linalg.qr(np.polynomial.legendre.legvander(x, p))
    fit = np.linalg.solve(r, q.T)                    # Legendre coefficients of the fit, one column per sample
    der = np.polynomial.legendre.legder(fit, deriv)  # ... of its derivative
    return np.polynomial.legendre.legval(x[:h], der).T / (half * delta) ** deriv


def ext_index(i, n, mode):
    """index into the row for position i of the extended row; -1 where the extension holds a constant"""
    i = np.asarray(i, np.int64)
    if mode == "mirror":
        if n == 1:
            return np.zeros_like(i)
        m = np.mod(i, 2 * (n - 1))
        return np.where(m < n, m, 2 * (n - 1) - m)
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    if mode == "wrap":
        return np.mod(i, n)
    return np.where((i >= 0) & (i < n), i, -1)


def savgol_filter(x, W, p, deriv=0, delta=1.0, mode="interp", cval=0.0):
    """the definition along the last axis; the samples are widened to f64, the result stays f64"""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    if mode == "interp" and W > n:
        raise ValueError("If mode is 'interp', window_length must be less than or equal to the size of x.")
    k = weights(W, p, deriv, float(delta))
    idx = ext_index(np.arange(-left(W), n - left(W) + W - 1), n, mode)
    fill = cval if mode == "constant" else 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        extended = np.where(idx >= 0, x[..., np.maximum(idx, 0)], fill)
        y = np.zeros(x.shape, np.float64)
        for j in range(W):   # every product is formed, zero weights included: 0 * inf is nan, as the definition has it
            y += k[j] * extended[..., j:j + n]
        h = W // 2
        if mode == "interp" and h:
            E = edge_table(W, p, deriv, float(delta))
            sign = -1.0 if deriv % 2 else 1.0
            head, tail = x[..., :W], x[..., ::-1][..., :W]
            y[..., :h] = np.einsum("ij,...j->...ij", E, head).sum(axis=-1)
            y[..., n - h:] = sign * np.einsum("ij,...j->...ij", E, tail).sum(axis=-1)[..., ::-1]
    return y


def nerr(got, ref):
    """largest error of a row over the row's largest reference magnitude, worst row"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    ok = np.isfinite(ref)
    d = np.where(ok, np.abs(np.where(ok, got, 0.0) - np.where(ok, ref, 0.0)), 0.0)
    scale = np.maximum(np.where(ok, np.abs(ref), 0.0).max(axis=-1), 1e-300)
    return float((d.max(axis=-1) / scale).max()) if d.size else 0.0
