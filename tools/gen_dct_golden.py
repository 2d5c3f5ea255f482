"""Records scipy.fft.dct / idct 1.15.3 for the host tests of Transforms.dct / idct (tests/test_dct_host.py holds the numpy oracle
tests/dct_oracle.py to these; needs scipy, the tests only read the file).

The cases: rows of 1, 2, 3, 8, 13, 80, 128, 255, 256, 257, 400, 1000, 1024 and 4099 samples at n = L, both types and the three norms,
dct and idct; padding (L, n) = (7, 16), (100, 257) and truncation (8, 5), (300, 128); a 2-D input along axis 0.  The samples are f32
values on a grid of 1 / 1024, which compresses; SciPy's f64 result does not, so a row of more than 64 points keeps its result at 96
places only — the first and last 16 and 64 spread over the row — with their indices.  Every output depends on every sample, so a place
is as good as a row.
    usage: python tools/gen_dct_golden.py [--out tests/golden/dct_vectors.json]"""
import argparse
import base64
import json
import os
import zlib

import numpy as np
import scipy
import scipy.fft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dct_vectors.json"))
args = ap.parse_args()

LENGTHS = [1, 2, 3, 8, 13, 80, 128, 255, 256, 257, 400, 1000, 1024, 4099]
RESIZED = [(7, 16), (100, 257), (8, 5), (300, 128)]   # (L, n)
TYPES = [2, 3]
NORMS = [None, "ortho", "forward"]


def enc(a):
    a = np.ascontiguousarray(a)
    return {"dtype": a.dtype.str, "shape": list(a.shape), "z": base64.b64encode(zlib.compress(a.tobytes(), 9)).decode("ascii")}


def places(n):
    if n <= 64:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(16), n - 16 + np.arange(16), (np.arange(64) * (n - 1)) // 63]))


rng = np.random.Generator(np.random.PCG64(17))


def samples(shape):
    return (np.round(rng.standard_normal(shape) * 1024) / 1024).astype(np.float32)


cases = []


def record(name, x, n=None, axis=-1):
    """one input, every (function, type, norm): results[fn][f"{type}_{norm}"]"""
    xd = x.astype(np.float64)   # the same samples, widened: SciPy transforms an f32 row in single precision
    at = places(x.shape[axis] if n is None else n)
    results = {}
    for fn in ("dct", "idct"):
        for t in TYPES:
            for norm in NORMS:
                y = getattr(scipy.fft, fn)(xd, type=t, n=n, axis=axis, norm=norm)
                assert y.dtype == np.float64
                results[f"{fn}_{t}_{norm}"] = enc(np.take(y, at, axis=axis))
    cases.append({"name": name, "n": n, "axis": axis, "x": enc(x), "at": enc(at.astype(np.int32)), "y": results})


for L in LENGTHS:
    record(f"L{L}", samples(L))
for L, n in RESIZED:
    record(f"L{L}_n{n}", samples(L), n=n)
record("axis0_37x3", samples((37, 3)), axis=0)
record("axis0_37x3_n64", samples((37, 3)), n=64, axis=0)

out = {"scipy": scipy.__version__, "numpy": np.__version__, "lengths": LENGTHS, "resized": [list(r) for r in RESIZED], "types": TYPES,
       "norms": NORMS, "cases": cases}
with open(args.out, "w") as f:
    json.dump(out, f, separators=(",", ":"))
    f.write("\n")
print(f"{len(cases)} cases of {len(cases[0]['y'])} results, {os.path.getsize(args.out)} bytes, scipy {scipy.__version__}")
