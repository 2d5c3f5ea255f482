"""Records scipy.signal.correlate / convolve / correlation_lags 1.15.3 for the host tests of Convolution.correlate_rows / convolve_rows
(tests/test_xcorr_host.py holds the numpy oracle tests/xcorr_oracle.py to these; needs scipy, the tests only read the file).

The cases: (n1, n2) = (1, 1), (2, 1), (5, 3), (3, 5), (8, 8), (7, 10), each real and complex, as small integers and as noise on a grid
of 1 / 1024, under both ops and all three modes (SciPy's default method, and method="direct" beside it: they agree to rounding), plus
correlation_lags for every mode on those shapes and on a sweep of odd and even lengths on either side of n1 = n2.
    usage: python tools/gen_xcorr_golden.py [--out tests/golden/xcorr_vectors.json]"""
import argparse
import json
import os

import numpy as np
import scipy
from scipy.signal import convolve, correlate, correlation_lags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "xcorr_vectors.json"))
args = ap.parse_args()

SHAPES = [(1, 1), (2, 1), (5, 3), (3, 5), (8, 8), (7, 10)]
MODES = ("full", "same", "valid")
LAG_SWEEP = [(n1, n2) for n1 in range(1, 10) for n2 in range(1, 10)] + [(600, 300), (301, 600), (1024, 1025), (1025, 1024)]


def cplx(a):
    a = np.asarray(a)
    return [[float(v.real), float(v.imag)] for v in a] if np.iscomplexobj(a) else [float(v) for v in a]


def rows(rng, n, kind, is_complex):
    def one():
        return rng.integers(-4, 5, n).astype(np.float64) if kind == "integers" else np.round(rng.standard_normal(n) * 1024) / 1024
    return one() + 1j * one() if is_complex else one()


rng = np.random.Generator(np.random.PCG64(20261021))
cases = []
for n1, n2 in SHAPES:
    for is_complex in (False, True):
        for kind in ("integers", "noise"):
            x, y = rows(rng, n1, kind, is_complex), rows(rng, n2, kind, is_complex)
            case = {"n1": n1, "n2": n2, "complex": is_complex, "kind": kind, "x": cplx(x), "y": cplx(y), "results": {}}
            for name, fn in (("correlate", correlate), ("convolve", convolve)):
                for mode in MODES:
                    auto, direct = fn(x, y, mode=mode), fn(x, y, mode=mode, method="direct")
                    assert auto.shape == direct.shape and np.abs(auto - direct).max() <= 1e-12 * max(np.abs(direct).max(), 1.0), (name, mode, n1, n2)
                    case["results"][f"{name}.{mode}"] = cplx(direct)
            cases.append(case)
lag_rows = [{"n1": n1, "n2": n2, "mode": mode, "lags": [int(v) for v in correlation_lags(n1, n2, mode)]}
            for n1, n2 in SHAPES + LAG_SWEEP for mode in MODES]
with open(args.out, "w") as f:
    json.dump({"scipy": scipy.__version__, "numpy": np.__version__, "cases": cases, "lags": lag_rows}, f, separators=(",", ":"))
    f.write("\n")
print(args.out, os.path.getsize(args.out), "bytes;", len(cases), "cases,", len(lag_rows), "lag rows")
