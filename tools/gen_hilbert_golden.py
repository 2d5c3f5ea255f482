"""Records scipy.signal.hilbert 1.15.3 for the host tests of Filters.hilbert (tests/test_hilbert_host.py holds the numpy oracle
tests/hilbert_oracle.py to these; needs scipy, the tests only read the file).

The cases: rows of 1, 2, 3, 7, 8, 1000, 1023, 1024, 2048 and 4096 samples at N = L, N longer and shorter than L (zero padding and
truncation, to even and odd N), a 2-D input along axis 0, and rows with a large offset (1000 + N(0, 1)).  The samples are f32 values on a
grid of 1 / 1024, which compresses; SciPy's c128 result does not, so a row of more than 64 points keeps its result at 96 places only —
the first and last 16 and 64 spread over the row — with their indices.  Every output depends on every sample, so a place is as good as
a row.  SciPy's answer for a row that holds a NaN or an Inf is recorded as the count of finite components it leaves ("nonfinite").
    usage: python tools/gen_hilbert_golden.py [--out tests/golden/hilbert_vectors.json]"""
import argparse
import base64
import json
import os
import warnings
import zlib

import numpy as np
import scipy
from scipy.signal import hilbert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "hilbert_vectors.json"))
args = ap.parse_args()

LENGTHS = [1, 2, 3, 7, 8, 1000, 1023, 1024, 2048, 4096]
RESIZED = [(1000, 1024), (1500, 1024), (1024, 1000), (7, 16), (8, 5), (100, 257), (3000, 2048)]   # (L, N)


def enc(a):
    a = np.ascontiguousarray(a)
    return {"dtype": a.dtype.str, "shape": list(a.shape), "z": base64.b64encode(zlib.compress(a.tobytes(), 9)).decode("ascii")}


def places(n):
    if n <= 64:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(16), n - 16 + np.arange(16), (np.arange(64) * (n - 1)) // 63]))


rng = np.random.Generator(np.random.PCG64(16))


def samples(shape, offset=0.0):
    return (np.round((rng.standard_normal(shape) + offset) * 1024) / 1024).astype(np.float32)


cases = []


def record(name, x, N=None, axis=-1):
    y = hilbert(x.astype(np.float64), N=N, axis=axis)   # the same samples, widened: SciPy transforms an f32 row in single precision
    assert y.dtype == np.complex128
    at = places(y.shape[axis])
    cases.append({"name": name, "N": N, "axis": axis, "x": enc(x), "at": enc(at.astype(np.int32)), "y": enc(np.take(y, at, axis=axis))})


for n in LENGTHS:
    record(f"L{n}", samples(n))
for L, N in RESIZED:
    record(f"L{L}_N{N}", samples(L), N=N)
record("axis0_37x3", samples((37, 3)), axis=0)
record("axis0_37x3_N64", samples((37, 3)), N=64, axis=0)
record("offset1000_L1024", samples(1024, offset=1000.0))
record("offset1000_2x1000", samples((2, 1000), offset=1000.0))

# what SciPy leaves of a row that holds a NaN or an Inf: finite components of the 2 N
nonfinite = {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    with np.errstate(all="ignore"):
        for n in (8, 1000, 1024):
            for bad in (np.nan, np.inf, -np.inf):
                x = samples(n).astype(np.float64)
                x[n // 3] = bad
                y = hilbert(x)
                nonfinite[f"L{n}_{bad}"] = int(np.isfinite(y.real).sum() + np.isfinite(y.imag).sum())

out = {"scipy": scipy.__version__, "numpy": np.__version__, "lengths": LENGTHS, "resized": [list(r) for r in RESIZED], "nonfinite": nonfinite,
       "cases": cases}
with open(args.out, "w") as f:
    json.dump(out, f, separators=(",", ":"))
    f.write("\n")
print(f"{len(cases)} cases, {os.path.getsize(args.out)} bytes, scipy {scipy.__version__}; finite components SciPy leaves of a bad row: {nonfinite}")
