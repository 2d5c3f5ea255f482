"""Records scipy.signal.find_peaks into tests/golden/find_peaks_vectors.json (run once, where scipy is installed; no test imports scipy).

    python tools/gen_find_peaks_golden.py [--out tests/golden/find_peaks_vectors.json]

Every array travels as bits: {"dtype": numpy's name, "z": base64 of the zlib-compressed little-endian bytes}.  The file holds ONE seeded
standard_normal row of 4096 f64 samples; a case names the row it runs on by recipe — "f64" the row itself, "f32" the row rounded to f32
(the rounding is exact IEEE, so the reader reproduces the bits), "halves" the row rounded to multiples of 0.5 (plateaus; the
plateau_size cases).  The short hand-made inputs are recorded whole.  A case: name, input, options (a pair as a list, an open side as
null), the peaks and every property SciPy returned.

The generator asserts what the issue asks of the recorded cases: every option set on a seeded row removes at least one peak and keeps at
least ten; no case with a distance holds two equal heights within d among the peaks the distance stage sees (SciPy leaves such ties to an
unstable sort; the library's own tie rule is tested against the rule, not against a recording); the flagship option set keeps 355 of 1360."""
import argparse
import base64
import json
import math
import os
import zlib

import numpy as np
import scipy
from scipy.signal import find_peaks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096


def enc(a):
    a = np.ascontiguousarray(a)
    return {"dtype": a.dtype.newbyteorder("<").str, "z": base64.b64encode(zlib.compress(a.astype(a.dtype.newbyteorder("<")).tobytes(), 9)).decode()}


def derive(row, recipe):
    return {"f64": row, "f32": row.astype(np.float32), "halves": np.round(row * 2) / 2}[recipe]


def opts_json(o):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in o.items()}


def record(name, x, opts, source):
    peaks, props = find_peaks(x, **opts)
    return {"name": name, "x": source, "opts": opts_json(opts), "peaks": enc(peaks.astype(np.int32)),
            "props": {k: enc(v.astype(np.int32) if v.dtype.kind == "i" else v.astype(np.float64)) for k, v in props.items()}}, peaks


# (name, options, the recipes it is recorded on)
SETS = [
    ("height", dict(height=2.0), ("f64", "f32")),
    ("height_two_sided", dict(height=(2.0, 2.3)), ("f32",)),
    ("threshold", dict(threshold=2.5), ("f64", "f32")),
    ("threshold_max_only", dict(threshold=(None, 0.15)), ("f64",)),
    ("distance_2_threshold", dict(distance=2, threshold=(2.5, None)), ("f64", "f32")),   # alone, 2 removes nothing from strict maxima
    ("distance_7p5", dict(distance=7.5), ("f32",)),
    ("distance_300", dict(distance=300), ("f64", "f32")),
    ("distance_1_height", dict(distance=1, height=(2.2, None)), ("f64",)),
    ("prominence", dict(prominence=3.5), ("f64", "f32")),
    ("prominence_two_sided_wlen_even", dict(prominence=(3.0, 3.5), wlen=64), ("f32",)),
    ("prominence_wlen_odd", dict(prominence=3.2, wlen=33), ("f64",)),
    ("width", dict(width=6), ("f64", "f32")),
    ("width_two_sided_rel_1_wlen_fractional", dict(width=(8, 12), rel_height=1.0, wlen=20.5), ("f64",)),
    ("height_width_rel_0", dict(height=2.0, width=0, rel_height=0), ("f32",)),
    ("prominence_width_max_rel_half", dict(prominence=3.0, width=(None, 4), rel_height=0.5), ("f32",)),
    ("plateau_size", dict(plateau_size=2), ("halves",)),
    ("plateau_size_two_sided_height", dict(plateau_size=(1, 1), height=2.0), ("halves",)),
    ("flagship", dict(distance=7.5, prominence=(0.3, None), width=1, wlen=101, rel_height=0.7), ("f64",)),
]


def no_ties_within_d(x, opts):
    if "distance" not in opts:
        return True
    before = {k: v for k, v in opts.items() if k in ("plateau_size", "height", "threshold")}
    peaks, _ = find_peaks(x, **before)
    d = math.ceil(opts["distance"])
    for a in range(len(peaks)):
        b = a + 1
        while b < len(peaks) and peaks[b] - peaks[a] < d:
            if x[peaks[a]] == x[peaks[b]]:
                return False
            b += 1
    return True


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "find_peaks_vectors.json"))
    a = ap.parse_args()
    assert scipy.__version__.startswith("1.15"), scipy.__version__
    row = np.random.default_rng(0).standard_normal(N)
    cases = []
    plateau = np.array([0, 1, 1, 1, 0, 2, 2, 0, 3, 3, 3, 3, 1, 5, 5], np.float64)
    c, peaks = record("plateau_array", plateau, dict(plateau_size=1), {"values": enc(plateau)})
    assert peaks.tolist() == [2, 5, 9]
    cases.append(c)
    naninf = np.array([0, 1, 0, np.nan, 0, 3, 0, np.inf, 0, 1, 0.5, 2, 0], np.float64)
    with np.errstate(invalid="ignore"):
        c, _ = record("nan_inf_array", naninf, dict(height=0, threshold=0, prominence=0, width=0), {"values": enc(naninf)})
    cases.append(c)
    short = np.array([1, 2, 1], np.float64)
    c, peaks = record("wlen_1p5", short, dict(prominence=0, wlen=1.5), {"values": enc(short)})
    assert peaks.tolist() == [1]
    cases.append(c)
    tie, _ = find_peaks(np.array([0, 2, 0, 2, 0, 2, 0, 2, 0], np.float64), distance=3)
    assert tie.tolist() == [3, 7], tie   # what 1.15.3 does, and what the library's larger-index-first rule gives
    for name, opts, recipes in SETS:
        for recipe in recipes:
            x = derive(row, recipe)
            total = len(find_peaks(x)[0])
            c, peaks = record(f"{name}_{recipe}", x, opts, {"row": recipe})
            assert 10 <= len(peaks) < total, (name, recipe, len(peaks), total)
            assert no_ties_within_d(x, opts), (name, recipe)
            if name == "flagship":
                assert (len(peaks), total) == (355, 1360), (len(peaks), total)
            c["kept_of"] = [len(peaks), total]
            cases.append(c)
    doc = {"scipy": scipy.__version__, "numpy": np.__version__, "seed": 0, "n": N, "row": enc(row), "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{a.out}: {len(cases)} cases, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
