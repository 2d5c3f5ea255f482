"""Records scipy.signal.lombscargle 1.15.3 for the host tests of Spectral.lombscargle (tests/test_lombscargle_host.py holds the numpy
oracle tests/lombscargle_oracle.py to these; needs scipy, the tests only read the file).

The cases: (n, F) = (1, 3), (2, 5), (63, 17), (257, 96), two rows each on one time base, under all 24 option combinations — precenter x
floating_mean x weights x "power" / "normalize" / "amplitude".  freqs[0] = 0 in every case.  Times, frequencies, weights and samples
are seeded values on a grid of 1 / 1024 (the samples f32), which compresses; SciPy's f64 results are kept whole.
    usage: python tools/gen_lombscargle_golden.py [--out tests/golden/lombscargle_vectors.json]"""
import argparse
import base64
import json
import os
import sys
import warnings
import zlib

import numpy as np
import scipy
import scipy.signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from lombscargle_oracle import COMBOS, combo_name  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lombscargle_vectors.json"))
args = ap.parse_args()

SHAPES = [(1, 3), (2, 5), (63, 17), (257, 96)]   # (n, F)
ROWS = 2


def enc(a):
    a = np.ascontiguousarray(a)
    return {"dtype": a.dtype.str, "shape": list(a.shape), "z": base64.b64encode(zlib.compress(a.tobytes(), 9)).decode("ascii")}


def grid(v):
    return np.round(np.asarray(v, np.float64) * 1024) / 1024


rng = np.random.Generator(np.random.PCG64(19))
cases = []
for n, F in SHAPES:
    x = grid(rng.uniform(0.0, 100.0, n))
    freqs = np.r_[0.0, grid(np.sort(rng.uniform(0.01, 20.0, F - 1)))]
    weights = grid(rng.uniform(0.25, 2.0, n))
    y = grid(1.5 + rng.standard_normal((ROWS, n)) + np.sin(1.25 * x)).astype(np.float32)
    results = {}
    for pre, fm, wts, norm in COMBOS:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            rows = [scipy.signal.lombscargle(x, y[r].astype(np.float64), freqs, precenter=pre, normalize=norm,
                                             weights=weights.copy() if wts else None, floating_mean=fm) for r in range(ROWS)]
        results[combo_name(pre, fm, wts, norm)] = enc(np.stack([np.atleast_1d(r) for r in rows]))
    cases.append({"name": f"n{n}_F{F}", "n": n, "F": F, "x": enc(x), "freqs": enc(freqs), "weights": enc(weights), "y": enc(y), "pgram": results})

out = {"scipy": scipy.__version__, "numpy": np.__version__, "shapes": [list(s) for s in SHAPES],
       "combos": [combo_name(*c) for c in COMBOS], "cases": cases}
with open(args.out, "w") as f:
    json.dump(out, f, separators=(",", ":"))
    f.write("\n")
print(f"{len(cases)} cases of {len(COMBOS)} results, {os.path.getsize(args.out)} bytes, scipy {scipy.__version__}")
