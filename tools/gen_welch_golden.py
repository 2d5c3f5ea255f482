"""Records scipy.signal.welch / csd / coherence results for a few small cases into tests/golden/welch_vectors.json: what
tests/test_welch_host.py holds tests/welch_oracle.py to.  Needs scipy (the tests only read the file).

    python tools/gen_welch_golden.py
"""
import json
import os

import sys

import numpy as np
import scipy
import scipy.signal as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from welch_oracle import golden_y  # noqa: E402  (y is derived from x: only x is recorded)
OUT = os.path.join(ROOT, "tests", "golden", "welch_vectors.json")

# name, length, window length, overlap, fft_length, sampling_rate, detrend, scaling, offset of the rows
CASES = [
    ("even-default", 160, 64, 32, 64, 1.0, "constant", "density", 0.0),
    ("odd-fft", 130, 51, 25, 127, 8000.0, "constant", "density", 3.0),
    ("zero-pad-spectrum", 150, 60, 15, 256, 48000.0, "constant", "spectrum", -2.0),
    ("no-detrend", 100, 32, 0, 32, 2.0, False, "density", 0.5),
    ("hop-one", 40, 32, 31, 32, 1.0, "constant", "spectrum", 10.0),
    ("one-frame-odd-window", 63, 63, 31, 63, 16000.0, False, "density", 0.0),
]


def f32s(a):
    """f32 values in their shortest decimal form (they read back to the same f32)"""
    return [float(str(v)) for v in np.asarray(a, np.float32).ravel()]

def g14(a):
    """results to 14 significant digits: the test's bound is 1e-12 of the row maximum"""
    return [float("%.14g" % v) for v in a]


def main():
    rng = np.random.default_rng(20260417)
    cases = []
    for name, length, n, overlap, k, fs, detrend, scaling, offset in CASES:
        x = (rng.standard_normal((2, length)) + offset).astype(np.float32)
        y = golden_y(x)
        w = ss.get_window("hann", n).astype(np.float32)
        kw = dict(fs=fs, window=w.astype(np.float64), nperseg=n, noverlap=overlap, nfft=k, detrend=detrend, scaling=scaling)
        f, pxx = ss.welch(x.astype(np.float64), **kw)
        _, pxy = ss.csd(x.astype(np.float64), y.astype(np.float64), **kw)
        cases.append({
            "name": name, "length": length, "overlap_length": overlap, "fft_length": k, "sampling_rate": fs, "detrend": detrend,
            "scaling": scaling, "window": f32s(w), "x": [f32s(r) for r in x], "f": [float(v) for v in f], "pxx": [g14(r) for r in pxx], "pxy_re": [g14(r) for r in pxy.real], "pxy_im": [g14(r) for r in pxy.imag],
        })
    with open(OUT, "w") as fh:
        json.dump({"scipy": scipy.__version__, "cases": cases}, fh, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
