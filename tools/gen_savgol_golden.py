"""Records scipy.signal.savgol_filter 1.15.3 for the host tests of Filters.savgol_filter (tests/test_savgol_host.py holds the numpy
oracle tests/savgol_oracle.py to these; needs scipy, the tests only read the file).

Only parameter sets on which scipy itself is sound are recorded: scipy solves an uncentred Vandermonde system with lstsq and loses digits
as the window grows, so for every recorded (window_length, polyorder, deriv, delta) this generator ASSERTS that scipy's weights lie within
1e-13 max|c| of the exact rational solution.  Between them the cases cover the five modes, delta = 0.5, cval = 0.5, f32 and f64 rows, and
n = 1, 3, W, W + 1 and 64, with one row shorter than half a window for each mode but interp; windows above 64 samples are recorded
under interp and one other mode each, which keeps the file below the largest fixture already there.  A row of one sample is recorded for
deriv = 0 only: the derivative of a constant row is exactly zero and what a double sum leaves of it is rounding noise.
    usage: python tools/gen_savgol_golden.py [--out tests/golden/savgol_vectors.json]"""
import argparse
import base64
import json
import os
import sys
import zlib

import numpy as np
import scipy
from scipy.signal import savgol_coeffs, savgol_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import savgol_oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "savgol_vectors.json"))
args = ap.parse_args()

SETS = [(5, 2, 0), (5, 4, 3), (6, 3, 1), (7, 2, 1), (9, 4, 2), (11, 3, 0), (15, 5, 3), (31, 3, 1), (32, 3, 0), (63, 4, 1), (101, 3, 1), (255, 3, 1)]
SOUND = 1e-13


def enc(a):
    a = np.ascontiguousarray(a)
    return {"dtype": a.dtype.str, "z": base64.b64encode(zlib.compress(a.tobytes(), 9)).decode("ascii")}


rng = np.random.Generator(np.random.PCG64(20))
cases, soundness = [], {}
for k, (w, p, d) in enumerate(SETS):
    delta = 0.5 if k % 3 == 1 else 1.0
    exact = np.array([float(v) for v in O.exact_weights(w, p, d, delta, use="conv")])
    gap = float(np.abs(savgol_coeffs(w, p, deriv=d, delta=delta) - exact).max() / np.abs(exact).max())
    assert gap <= SOUND, (w, p, d, gap)
    soundness[f"{w},{p},{d}"] = gap
    for m, mode in enumerate(O.MODES):
        if w > 64 and mode not in ("interp", ("mirror", "nearest", "wrap", "constant")[k % 4]):
            continue                   # the long windows: interp and one other mode each, to keep the file small
        lengths = [w] + ([w + 1] if w <= 64 or mode == "interp" else []) + ([64] if w <= 64 else [])
        if mode != "interp" and d == 0:
            lengths += [1, 3]          # (11, 3, 0) and (32, 3, 0): 3 < h, a row shorter than half a window
        elif mode != "interp" and w <= 7:
            lengths += [3]
        for n in sorted(set(lengths)):
            dtype = np.float32 if (k + m + n) % 2 else np.float64
            x = (np.round((rng.standard_normal(n) + 0.5) * 1024) / 1024).astype(dtype)   # on a grid of 1 / 1024: exact in f32, and it compresses
            cval = 0.5 if mode == "constant" else 0.0
            y = savgol_filter(x, w, p, deriv=d, delta=delta, mode=mode, cval=cval)
            assert y.dtype == dtype
            cases.append({"name": f"w{w}_p{p}_d{d}_{mode}_n{n}_{np.dtype(dtype).name}", "window_length": w, "polyorder": p, "deriv": d,
                          "delta": delta, "mode": mode, "cval": cval, "n": n, "x": enc(x), "y": enc(y)})

short = {c["mode"] for c in cases if c["n"] < c["window_length"] // 2}
assert short == set(O.MODES) - {"interp"}, short
assert {c["n"] for c in cases} >= {1, 3, 64} and {c["x"]["dtype"] for c in cases} == {"<f4", "<f8"}
assert {c["delta"] for c in cases} == {0.5, 1.0} and any(c["cval"] == 0.5 for c in cases)
out = {"scipy": scipy.__version__, "numpy": np.__version__, "sets": [list(s) for s in SETS], "scipy_weight_gap": soundness, "cases": cases}
with open(args.out, "w") as f:
    json.dump(out, f, separators=(",", ":"))
    f.write("\n")
print(f"{len(cases)} cases, {os.path.getsize(args.out)} bytes, scipy {scipy.__version__}; worst scipy weight gap {max(soundness.values()):.1e}")
