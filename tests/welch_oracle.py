"""The definition of Spectral.welch / csd / coherence in f64 numpy (scipy.signal.welch / csd / coherence, scipy 1.15.3, with
return_onesided=True and average="mean"): what the GPU tests compare with.  tests/test_welch_host.py holds it to the recorded scipy
results of tests/golden/welch_vectors.json (tools/gen_welch_golden.py); nothing here imports scipy."""
import numpy as np


def frames(x, n, hop):
    """f64[..., M, n]: frame m covers samples [m hop, m hop + n); M = (L - n) // hop + 1, the ragged tail dropped"""
    x = np.asarray(x, np.float64)
    m = (x.shape[-1] - n) // hop + 1
    if x.shape[-1] < n:
        raise ValueError("the rows are shorter than one frame")
    idx = np.arange(m)[:, None] * hop + np.arange(n)[None, :]
    return x[..., idx]


def csd(x, y, window, overlap_length=None, fft_length=None, sampling_rate=1.0, detrend="constant", scaling="density"):
    """(f, Pxy) in f64 / c128 over the last axis"""
    w = np.asarray(window, np.float64)
    n = w.shape[0]
    hop = n - (n // 2 if overlap_length is None else overlap_length)
    k = n if fft_length is None else fft_length
    fx, fy = frames(x, n, hop), frames(y, n, hop)
    if detrend == "constant":
        fx, fy = fx - fx.mean(-1, keepdims=True), fy - fy.mean(-1, keepdims=True)
    p = (np.conj(np.fft.rfft(fx * w, k)) * np.fft.rfft(fy * w, k)).mean(-2)
    p *= 1.0 / (sampling_rate * (w * w).sum()) if scaling == "density" else 1.0 / w.sum() ** 2
    p[..., 1:(k // 2 if k % 2 == 0 else None)] *= 2.0   # every bin but 0 and, for even k, k / 2
    return np.arange(k // 2 + 1) * sampling_rate / k, p


def welch(x, window, **opts):
    f, p = csd(x, x, window, **opts)
    return f, p.real


def coherence(x, y, window, **opts):
    f, pxy = csd(x, y, window, **opts)
    return f, np.abs(pxy) ** 2 / (welch(x, window, **opts)[1] * welch(y, window, **opts)[1])


def golden_y(x):
    """the second signal of the recorded cases, derived from the first: half of x delayed by three samples plus x reversed, as f32"""
    x = np.asarray(x, np.float32).astype(np.float64)
    return (0.5 * np.roll(x, 3, axis=-1) + x[..., ::-1]).astype(np.float32)
