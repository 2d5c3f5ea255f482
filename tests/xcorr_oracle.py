"""The f64 oracle of Convolution.correlate_rows / convolve_rows: the definition of include/nxsig.h evaluated directly in double
(np.convolve is the plain sum), SciPy's three windows and its correlation_lags restated, and the PHAT weighting through np.fft in double
at the contract's transform length P = max(1024, next power of two >= n1 + n2 - 1).  No SciPy: tests/test_xcorr_host.py holds this file
to tests/golden/xcorr_vectors.json, which tools/gen_xcorr_golden.py recorded from scipy.signal 1.15.3."""
import numpy as np

MODES = ("full", "same", "valid")
OPS = ("correlate", "convolve")


def _wide(v):
    v = np.asarray(v)
    return v.astype(np.complex128 if np.iscomplexobj(v) else np.float64)


def full(x, y, op):
    """one pair: full[k], k = 0 .. n1 + n2 - 2.  correlate: sum_l x[l] conj(y[l - k + n2 - 1]); convolve: sum_l x[l] y[k - l]"""
    x, y = _wide(x), _wide(y)
    return np.convolve(x, np.conj(y[::-1]) if op == "correlate" else y)


def out_start(n1, n2, mode):
    return {"full": 0, "same": (n2 - 1) // 2, "valid": min(n1, n2) - 1}[mode]


def out_length(n1, n2, mode):
    return {"full": n1 + n2 - 1, "same": n1, "valid": abs(n1 - n2) + 1}[mode]


def window(f, n1, n2, mode):
    s = out_start(n1, n2, mode)
    return f[..., s:s + out_length(n1, n2, mode)]


def pair(x, y, op, mode):
    return window(full(x, y, op), len(x), len(y), mode)


def rows(a, b, op, mode):
    """a [rows, n1]; b [rows, n2] or [n2] (one template): [rows, n_out]"""
    a, b = np.atleast_2d(a), np.asarray(b)
    return np.stack([pair(a[r], b if b.ndim == 1 else b[r], op, mode) for r in range(a.shape[0])])


def lags(n1, n2, mode):
    """scipy.signal.correlation_lags, restated"""
    if mode == "full":
        return np.arange(-n2 + 1, n1)
    if mode == "same":
        all_lags = np.arange(-n2 + 1, n1)
        mid, bound = all_lags.size // 2, n1 // 2
        return all_lags[mid - bound:mid + bound + (n1 % 2)]
    return np.arange(n1 - n2 + 1) if n1 >= n2 else np.arange(n1 - n2, 1)


def fft_length(n1, n2):
    P = 1024
    while P < n1 + n2 - 1:
        P *= 2
    return P


def circ_start(n1, n2, op, mode, P):
    """output element i of the mode's window is the circular result's element (circ_start + i) mod P"""
    return (out_start(n1, n2, mode) - (n2 - 1 if op == "correlate" else 0)) % P


def phat_rows(a, b, mode, floor=0.0):
    """the PHAT-weighted correlation of every pair at the contract's P, in double"""
    a, b = np.atleast_2d(a), np.asarray(b)
    n1, n2 = a.shape[-1], b.shape[-1]
    P = fft_length(n1, n2)
    X, Y = np.fft.fft(_wide(a), P, axis=-1), np.fft.fft(_wide(b), P, axis=-1)
    R = X * np.conj(Y)
    mag = np.abs(R)
    den = np.maximum(mag, floor * mag.max(axis=-1, keepdims=True))
    G = np.where(den > 0, R / np.where(den > 0, den, 1.0), 0.0)
    c = np.fft.ifft(G, axis=-1)
    idx = (circ_start(n1, n2, "correlate", mode, P) + np.arange(out_length(n1, n2, mode))) % P
    out = c[..., idx]
    return out if np.iscomplexobj(a) or np.iscomplexobj(b) else out.real


def modulus32(v):
    """what the peak sink ranks c64 results by: the f32 rounding of sqrt(re^2 + im^2) evaluated in double"""
    v = np.asarray(v)
    return np.sqrt(v.real.astype(np.float64) ** 2 + v.imag.astype(np.float64) ** 2).astype(np.float32)


def peak(rows_out, n1, n2, mode):
    """(lags, values) of rows as the peak sink reports them: the first maximum of the values (real) or of modulus32 (complex)"""
    rows_out = np.asarray(rows_out)
    key = modulus32(rows_out) if np.iscomplexobj(rows_out) else rows_out
    at = np.argmax(key, axis=-1)
    return lags(n1, n2, mode)[at].astype(np.int32), np.take_along_axis(rows_out, at[..., None], axis=-1)[..., 0]
