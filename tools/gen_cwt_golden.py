#!/usr/bin/env python
"""Write tests/golden/cwt_vectors.json: a handful of small continuous wavelet transforms (L <= 64) evaluated by the numpy oracle
tests/cwt_oracle.py — the definition of include/nxsig.h, scipy.signal.cwt as SciPy <= 1.14 had it — plus the two spot checks the
definition is pinned by: cwt(arange(8.), ricker, [1.0]) and a unit impulse, whose transform is the filter itself.

SciPy 1.15 removed cwt, morlet2 and ricker, so there is no installed implementation to record; the file pins the oracle against
silent change, and tests/test_cwt_host.py checks the oracle's convolution against scipy.signal.convolve(..., "same") separately.

    python tools/gen_cwt_golden.py [--write tests/golden/cwt_vectors.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cwt_oracle as O  # noqa: E402

# (name, L, widths, wavelet, w): N = 1, even and odd N, and N capped by L
CASES = [
    ("ricker-L64", 64, [0.1, 1.0, 2.5, 4.5], "ricker", 5.0),
    ("morlet2-L64", 64, [0.1, 1.0, 2.5, 4.5, 10.0], "morlet2", 5.0),
    ("morlet2-w3-L37", 37, [1.0, 2.5, 10.0], "morlet2", 3.0),
    ("ricker-L2", 2, [0.1, 1.0], "ricker", 5.0),
    ("morlet2-L1", 1, [0.1, 4.5], "morlet2", 5.0),
]
# cwt(arange(8.), ricker, [1.0])[0], from the formulas of the definition
SPOT_RAMP = [-0.816136597, -0.815461023, -0.240726683, -0.0179663738, 0.00472901446, 0.176834091, 1.80004885, 4.83860140]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--write", metavar="JSON", default=None)
    a = ap.parse_args()
    cases = []
    for i, (name, L, widths, wavelet, w) in enumerate(CASES):
        x = np.random.Generator(np.random.PCG64(100 + i)).standard_normal(L).astype(np.float32)
        y = O.cwt(x, widths, wavelet, w, kind="complex")
        cases.append({"name": name, "L": L, "widths": widths, "wavelet": wavelet, "w": w, "x": [float(v) for v in x],
                      "supports": [O.support(s, L) for s in widths], "re": y.real.tolist(), "im": y.imag.tolist()})
    doc = {"cases": cases, "spot_ramp": {"x": list(range(8)), "wavelet": "ricker", "widths": [1.0], "y": SPOT_RAMP},
           "spot_impulse": {"L": 48, "p": 17, "wavelet": "morlet2", "widths": [0.7, 2.0, 3.3], "w": 5.0}}
    text = json.dumps(doc, separators=(",", ":")) + "\n"
    if a.write:
        with open(a.write, "w") as f:
            f.write(text)
        print(f"{a.write}: {len(cases)} cases, {len(text)} bytes")
    else:
        print(text)


if __name__ == "__main__":
    main()
