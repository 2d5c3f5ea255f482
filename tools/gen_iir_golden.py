"""Writes tests/golden/iir_vectors.json: the cascades the recursive-filter tests use and what scipy.signal (1.15) computes with them
on two short rows — sosfilt_zi, sosfilt without and with zi (and zf), sosfiltfilt for every padtype.  Needs scipy; the tests only read
the file.  The rows are recorded whole; of every output the samples AT (every sixteenth and the last) are kept, which holds a recurrence as
well as all of them do — an error made at any sample is still there sixteen samples on — and keeps the file small.  The samples are f32 values, widened: scipy computes in f64 on them, which is what tests/iir_oracle.py restates.

    python tools/gen_iir_golden.py
"""
import json
import os
import sys

import numpy as np
import scipy
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "iir_vectors.json")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import iir_oracle as O  # noqa: E402  (its gap to scipy on the recurrence is measured here and recorded)
FS = 48000.0
ROWS, N = 2, 160
AT = list(range(15, N, 16))   # 15, 31, ... 159: the last sample included


def filters():
    r, th = 1.001, 0.3
    return [
        ("butter4_lp4k", signal.butter(4, 4000.0, fs=FS, output="sos")),
        ("butter2_hp20", signal.butter(2, 20.0, "hp", fs=FS, output="sos")),
        ("butter4_hp20", signal.butter(4, 20.0, "hp", fs=FS, output="sos")),
        ("ellip4_bp", signal.ellip(4, 0.5, 60.0, [300.0, 3400.0], "bp", fs=FS, output="sos")),
        ("cheby1_8_lp100", signal.cheby1(8, 1.0, 100.0, fs=FS, output="sos")),
        ("ellip16_bp", signal.ellip(16, 0.5, 60.0, [300.0, 3400.0], "bp", fs=FS, output="sos")),
        ("ellip20_bp", signal.ellip(20, 0.5, 60.0, [300.0, 3400.0], "bp", fs=FS, output="sos")),
        ("integrator", np.array([[1.0, 0.0, 0.0, 1.0, -1.0, 0.0]])),
        ("unstable_r1001", np.array([[1.0, 0.0, 0.0, 1.0, -2.0 * r * np.cos(th), r * r]])),
    ]


def lst(a):
    return np.asarray(a, np.float64).tolist()


def out(y):
    return lst(np.asarray(y)[:, AT])


def main():
    rng = np.random.Generator(np.random.PCG64(20261019))
    x32 = (rng.standard_normal((ROWS, N)) + 0.75).astype(np.float32)
    x = x32.astype(np.float64)
    cases = []
    for name, sos in filters():
        sos = np.ascontiguousarray(sos, np.float64)
        ns = sos.shape[0]
        try:
            zi = signal.sosfilt_zi(sos)
        except np.linalg.LinAlgError:   # a pole at z = 1 has no settled step response: recorded as null
            zi = None
        start = 0.1 * rng.standard_normal((ns, ROWS, 2))   # scipy's layout (n_sections, rows, 2)
        y = signal.sosfilt(sos, x, axis=-1)
        y_zi, zf = signal.sosfilt(sos, x, axis=-1, zi=start)
        c = dict(name=name, n_sections=ns, sos=lst(sos), sosfilt_zi=None if zi is None else lst(zi), y=out(y), zi=lst(start), y_zi=out(y_zi), zf=lst(zf),
                 largest_pole=float(np.abs(np.roots(np.r_[1.0, sos[0, 4:]])).max()) if ns == 1 else
                 float(max(np.abs(np.roots(s[3:])).max() for s in sos)))
        # what tests/iir_oracle.py gives against these results, measured with the numpy that writes the file: the host test holds the
        # oracle to ten times this under the same numpy (the recurrence is element-wise IEEE arithmetic: it does not vary by machine)
        oy, _ = O.sosfilt(sos, x)
        ozy, ozf = O.sosfilt(sos, x, start.transpose(1, 0, 2))
        c["oracle_gap"] = float(max(np.abs(oy - y).max() / np.abs(y).max(), np.abs(ozy - y_zi).max() / np.abs(y_zi).max(),
                                    np.abs(ozf.transpose(1, 0, 2) - zf).max() / np.abs(zf).max()))
        if zi is not None:
            c["sosfiltfilt"] = {str(p): out(signal.sosfiltfilt(sos, x, axis=-1, padtype=p)) for p in ("odd", "even", "constant", None)}
            c["default_padlen"] = int(3 * (2 * ns + 1 - min((sos[:, 2] == 0).sum(), (sos[:, 5] == 0).sum())))
        cases.append(c)
    doc = dict(scipy=scipy.__version__, numpy=np.__version__, sampling_rate=FS, at=AT, x=[[float(v) for v in r] for r in x32], cases=cases)
    with open(OUT, "w") as f:
        json.dump(doc, f)
        f.write("\n")
    print(f"{OUT}: {len(cases)} cascades, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
