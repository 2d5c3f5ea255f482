"""Records scipy.signal.czt / zoom_fft / czt_points 1.15.3 for the host tests of Transforms.czt (tests/test_czt_host.py holds the numpy
oracle tests/czt_oracle.py to these; needs scipy, the tests only read the file).

The cases: (n, m) = (1, 1), (3, 7), (600, 300), (512, 513), (513, 513), (1024, 1025), (1500, 549), (1025, 1025), (5000, 37) and
(100, 5000), each as czt's default, czt with a general unit w and a, and zoom_fft with and without endpoint and with a scalar fn; one
spiral (n = m = 64, |w| = 1.0005, |a| = 0.999), one c64 row, one 2-D input along axis 0, and the spiral sweep the gate of
csrc/czt_plan.hpp is measured on (n = m = 64 and n = 600, m = 300, |w| on either side of 1 at spreads 4 ... 64; parameters only: the
test evaluates the definition itself).  The samples are f32 values on a grid of 1 / 1024, one row per shape, which compresses; SciPy's
c128 result does not, so a result of more than 64 points keeps 96 places only — the first and last 16 and 64 spread over the row —
with their indices.  Every output depends on every sample, so a place is as good as a row.
    usage: python tools/gen_czt_golden.py [--out tests/golden/czt_vectors.json]"""
import argparse
import base64
import json
import math
import os
import zlib

import numpy as np
import scipy
from scipy.signal import czt, czt_points, zoom_fft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "czt_vectors.json"))
args = ap.parse_args()

SHAPES = [(1, 1), (3, 7), (600, 300), (512, 513), (513, 513), (1024, 1025), (1500, 549), (1025, 1025), (5000, 37), (100, 5000)]
W_UNIT, A_UNIT = [math.cos(0.37), -math.sin(0.37)], [math.cos(0.2), math.sin(0.2)]   # (re, im): exp(-0.37i), exp(0.2i)
FN, FS, FN_SCALAR = [0.1, 0.3], 2.0, 0.45
SWEEP_SPREADS = [4, 8, 16, 32, 64]


def enc(a):
    a = np.ascontiguousarray(a)
    return {"dtype": a.dtype.str, "shape": list(a.shape), "z": base64.b64encode(zlib.compress(a.tobytes(), 9)).decode("ascii")}


def places(n):
    if n <= 64:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(16), n - 16 + np.arange(16), (np.arange(64) * (n - 1)) // 63]))


rng = np.random.Generator(np.random.PCG64(20))


def samples(shape):
    return (np.round(rng.standard_normal(shape) * 1024) / 1024).astype(np.float32)


inputs, cases = {}, []


def record(name, key, call, m, axis=-1, **params):
    """call: SciPy on the widened samples (SciPy transforms an f32 row in single precision)"""
    x = inputs[key]
    wide = np.frombuffer(zlib.decompress(base64.b64decode(x["z"])), np.dtype(x["dtype"])).reshape(x["shape"])
    y = call(wide.astype(np.complex128 if wide.dtype.kind == "c" else np.float64))
    assert y.dtype == np.complex128 and y.shape[axis] == m
    at = places(m)
    cases.append({"name": name, "x": key, "m": m, "axis": axis, **params, "at": enc(at.astype(np.int32)), "y": enc(np.take(y, at, axis=axis))})


def cplx(p):
    return complex(p[0], p[1])


for n, m in SHAPES:
    key = f"n{n}"
    if key not in inputs:
        inputs[key] = enc(samples(n))
    tag = f"n{n}_m{m}"
    record(f"{tag}_czt", key, lambda x: czt(x, m), m, kind="czt", w=None, a=[1.0, 0.0])
    record(f"{tag}_czt_wa", key, lambda x: czt(x, m, cplx(W_UNIT), cplx(A_UNIT)), m, kind="czt", w=W_UNIT, a=A_UNIT)
    record(f"{tag}_zoom", key, lambda x: zoom_fft(x, FN, m, fs=FS), m, kind="zoom", fn=FN, fs=FS, endpoint=False)
    if m > 1:
        record(f"{tag}_zoom_endpoint", key, lambda x: zoom_fft(x, FN, m, fs=FS, endpoint=True), m, kind="zoom", fn=FN, fs=FS, endpoint=True)
    record(f"{tag}_zoom_scalar", key, lambda x: zoom_fft(x, FN_SCALAR, m, fs=FS), m, kind="zoom", fn=FN_SCALAR, fs=FS, endpoint=False)

# the spiral of the issue, a c64 row and another axis
W_SPIRAL = [1.0005 * math.cos(0.11), -1.0005 * math.sin(0.11)]
A_SPIRAL = [0.999 * math.cos(0.3), 0.999 * math.sin(0.3)]
inputs["n64"] = enc(samples(64))
record("spiral_n64_m64", "n64", lambda x: czt(x, 64, cplx(W_SPIRAL), cplx(A_SPIRAL)), 64, kind="czt", w=W_SPIRAL, a=A_SPIRAL)
inputs["c64_n300"] = enc((samples(300) + 1j * samples(300)).astype(np.complex64))
record("c64_n300_m200_czt_wa", "c64_n300", lambda x: czt(x, 200, cplx(W_UNIT), cplx(A_UNIT)), 200, kind="czt", w=W_UNIT, a=A_UNIT)
record("c64_n300_m200_zoom", "c64_n300", lambda x: zoom_fft(x, FN, 200, fs=FS), 200, kind="zoom", fn=FN, fs=FS, endpoint=False)
inputs["axis0_37x3"] = enc(samples((37, 3)))
record("axis0_37x3_m50_czt", "axis0_37x3", lambda x: czt(x, 50, axis=0), 50, axis=0, kind="czt", w=None, a=[1.0, 0.0])
record("axis0_37x3_m50_zoom", "axis0_37x3", lambda x: zoom_fft(x, FN, 50, fs=FS, axis=0), 50, axis=0, kind="zoom", fn=FN, fs=FS, endpoint=False)

# the sweep behind the spiral gate: |w| = exp(+- ln(spread) / ((max(n, m) - 1)^2 / 2)), |a| = 1, sixteen rows each
sweep = []
for n, m in [(64, 64), (600, 300)]:
    inputs[f"sweep_16x{n}"] = enc(samples((16, n)))
    for spread in SWEEP_SPREADS:
        for sign in (1, -1):
            # a hair inside the nominal spread, so that the entry at the gate's own value is one the gate admits
            w_abs = math.exp(sign * math.log(spread) * (1 - 1e-9) / ((max(n, m) - 1) ** 2 / 2))
            sweep.append({"x": f"sweep_16x{n}", "n": n, "m": m, "spread": spread, "w": [w_abs * math.cos(0.11), -w_abs * math.sin(0.11)],
                          "a": [math.cos(0.3), math.sin(0.3)]})

points = []
for m, w, a in [(1, None, [1.0, 0.0]), (16, None, [1.0, 0.0]), (7, None, [0.0, 2.0]), (91, [0.995 * math.cos(0.05 * math.pi), -0.995 * math.sin(0.05 * math.pi)],
                                                                                      [0.8 * math.cos(math.pi / 6), 0.8 * math.sin(math.pi / 6)])]:
    points.append({"m": m, "w": w, "a": a, "y": enc(czt_points(m, None if w is None else cplx(w), cplx(a)))})

out = {"scipy": scipy.__version__, "numpy": np.__version__, "shapes": [list(s) for s in SHAPES], "inputs": inputs, "cases": cases, "sweep": sweep,
       "points": points}
with open(args.out, "w") as f:
    json.dump(out, f, separators=(",", ":"))
    f.write("\n")
print(f"{len(cases)} cases, {len(sweep)} sweep entries, {os.path.getsize(args.out)} bytes, scipy {scipy.__version__}")
