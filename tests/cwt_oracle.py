"""The definition of Transforms.cwt / Filters.fir_bank (include/nxsig.h) in numpy double, and nothing else: scipy.signal.cwt, morlet2 and
ricker as SciPy <= 1.14 had them (1.15 removed them)."""
import numpy as np

KINDS = ("complex", "real", "magnitude", "power")


def morlet2(M, s, w=5.0):
    t = (np.arange(0, M) - (M - 1.0) / 2) / s
    return np.sqrt(1 / s) * np.pi ** (-0.25) * np.exp(1j * w * t) * np.exp(-0.5 * t ** 2)


def ricker(M, a):
    v = np.arange(0, M) - (M - 1.0) / 2
    return 2 / (np.sqrt(3 * a) * np.pi ** 0.25) * (1 - v ** 2 / a ** 2) * np.exp(-v ** 2 / (2 * a ** 2))


def support(a, L):
    """N = min(ceil(10 a), L): len(arange(0, 10 a)), capped"""
    return int(min(np.ceil(10.0 * a), L))


def taps(wavelet, a, L, w=5.0):
    """h_a = conj(wavelet(N, a))[::-1]"""
    N = support(a, L)
    return np.conj(morlet2(N, a, w) if wavelet == "morlet2" else ricker(N, a))[::-1]


def same(x, h):
    """out[n] = full[n + (N - 1) // 2], 0 <= n < L"""
    x, h = np.asarray(x, np.float64), np.asarray(h)
    full = np.convolve(x, h)
    c = (len(h) - 1) // 2
    return full[c:c + len(x)]


def sink(y, kind):
    y = np.asarray(y, np.complex128)
    if kind == "complex":
        return y
    if kind == "real":
        return y.real
    if kind == "magnitude":
        return np.sqrt(y.real * y.real + y.imag * y.imag)
    return y.real * y.real + y.imag * y.imag


def fir_bank(x, bank, kind="complex"):
    """x [..., L], bank a list of 1-D arrays -> [..., S, L]"""
    x = np.asarray(x, np.float64)
    rows = x.reshape(-1, x.shape[-1])
    out = np.array([[same(r, h) for h in bank] for r in rows], np.complex128)
    return sink(out, kind).reshape(x.shape[:-1] + (len(bank), x.shape[-1]))


def cwt(x, widths, wavelet="morlet2", w=5.0, kind=None):
    L = np.asarray(x).shape[-1]
    if kind is None:
        kind = "real" if wavelet == "ricker" else "complex"
    return fir_bank(x, [taps(wavelet, a, L, w) for a in widths], kind)
