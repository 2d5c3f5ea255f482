"""The chirp z-transform by its definition (include/nxsig.h), numpy, double:

    X[k] = sum_{j<n} x[j] a^(-j) w^(j k),   w = w_abs exp(-2 pi i w_step / w_den),   a = a_abs exp(2 pi i a_turns)

as a direct sum, no chirps and no transform.  Every phase -j a_turns - j k w_step / w_den is reduced mod 1 in integer arithmetic before it
meets a sine: the two fractions of a turn are taken exactly (fractions.Fraction of the doubles) and kept to 128 binary places, and the
multiples j and j k are wrapping 128-bit products carried in two uint64 limbs, of which the leading 64 bits are the reduced phase.  What
is lost is under 2^-64 of a turn."""
import cmath
import math
from fractions import Fraction

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def contour_czt(m, w=None, a=1 + 0j):
    """(w_abs, w_step, w_den, a_abs, a_turns) of scipy.signal.czt(x, m, w, a)"""
    a = complex(a)
    if w is None:
        return 1.0, 1.0, int(m), abs(a), cmath.phase(a) / (2 * math.pi)
    w = complex(w)
    return abs(w), -cmath.phase(w) / (2 * math.pi), 1, abs(a), cmath.phase(a) / (2 * math.pi)


def contour_zoom(fn, m, fs=2, endpoint=False):
    """(w_abs, w_step, w_den, a_abs, a_turns) of scipy.signal.zoom_fft(x, fn, m, fs=fs, endpoint=endpoint); scale as SciPy computes it"""
    f1, f2 = (0.0, fn) if np.size(fn) == 1 else fn
    scale = ((f2 - f1) * m) / (fs * (m - 1)) if endpoint else (f2 - f1) / fs
    return 1.0, float(scale), int(m), 1.0, float(f1 / fs)


def turn_fraction(value, den=1):
    """floor(frac(value / den) 2^128) as (high, low) uint64 limbs; value a double taken exactly"""
    f = Fraction(float(value)) / int(den)
    f -= math.floor(f)
    q = (f.numerator << 128) // f.denominator
    return np.uint64(q >> 64), np.uint64(q & ((1 << 64) - 1))


def _mulhi(a, b):
    """the high 64 bits of the 128-bit products a * b, uint64 arrays"""
    a0, a1, b0, b1 = a & _M32, a >> _S32, b & _M32, b >> _S32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> _S32) + (p01 & _M32) + (p10 & _M32)
    return p11 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32)


def reduced_turns(mult, frac):
    """frac(mult * f) in [-1/2, 1/2) as float64, f the fraction held in the limbs `frac`; mult a uint64 array below 2^63"""
    hi, lo = frac
    with np.errstate(over="ignore"):
        top = mult * hi + _mulhi(mult, np.broadcast_to(lo, mult.shape))
    return top.astype(np.int64).astype(np.float64) * 2.0 ** -64


def kernel(n, m, contour, at=None):
    """the matrix [n][len(at)] of a^(-j) w^(j k), complex128; at: the output indices wanted (default: all m)"""
    w_abs, w_step, w_den, a_abs, a_turns = contour
    k = np.arange(m, dtype=np.uint64) if at is None else np.asarray(at, dtype=np.uint64)
    j = np.arange(n, dtype=np.uint64)
    jk = j[:, None] * k[None, :]
    turns = -reduced_turns(j, turn_fraction(a_turns))[:, None] - reduced_turns(jk, turn_fraction(w_step, w_den))
    out = np.exp(2j * np.pi * turns)
    if w_abs != 1.0 or a_abs != 1.0:
        out *= np.exp(jk.astype(np.float64) * math.log(w_abs) - j.astype(np.float64)[:, None] * math.log(a_abs))
    return out


def czt(x, m, contour, at=None, block=1 << 22):
    """X[..., at] of rows x[..., n] by the definition, complex128; the kernel is formed `block` entries at a time"""
    x = np.asarray(x)
    x = x.astype(np.complex128 if x.dtype.kind == "c" else np.float64)
    n = x.shape[-1]
    at = np.arange(m) if at is None else np.asarray(at)
    out = np.empty(x.shape[:-1] + (len(at),), np.complex128)
    step = max(1, block // n)
    for s in range(0, len(at), step):
        out[..., s:s + step] = x @ kernel(n, m, contour, at[s:s + step])
    return out
