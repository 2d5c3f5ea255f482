"""Writes tests/golden/lfilter_vectors.json: the transfer functions the lfilter tests use and what scipy.signal (1.15) computes with them
on two short rows — lfilter_zi, lfilter without and with zi (and zf), filtfilt for every padtype and one explicit padlen, lfiltic.
Needs scipy; the tests only read the file.  Of every output the samples AT (every thirty-second and the last) are kept, which holds a
recurrence as well as all of them do and keeps the file small.  The samples are f32 values, widened: scipy computes in f64 on them, which
is what tests/lfilter_oracle.py restates.

    python tools/gen_lfilter_golden.py
"""
import json
import os

import numpy as np
import scipy
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "lfilter_vectors.json")
FS = 48000.0
ROWS, N = 2, 96
AT = list(range(31, N, 32))   # 31, 63, 95: the last sample included
PADLEN = 7                    # the explicit padlen recorded beside the default


def filters():
    """(name, b, a, on_scan): the stable filters of DESIGN.md section 3.18's table, the coefficient-shape cases and every padded-order
    boundary.  on_scan: what the conditioning guard is expected to decide for long rows"""
    return [
        ("butter2_lp02", *signal.butter(2, 0.2), True),
        ("butter4_lp01", *signal.butter(4, 0.1), True),
        ("butter2_hp20", *signal.butter(2, 20.0, "hp", fs=FS), True),
        ("butter4_hp20", *signal.butter(4, 20.0, "hp", fs=FS), False),
        ("butter4_hp60", *signal.butter(4, 60.0, "hp", fs=FS), False),
        ("butter4_bp", *signal.butter(4, [0.2, 0.4], "bp"), True),
        ("ellip6", *signal.ellip(6, 0.5, 60.0, 0.3), True),
        ("butter12_lp03", *signal.butter(12, 0.3), False),
        ("butter16_lp04", *signal.butter(16, 0.4), True),
        ("cheby2_16", *signal.cheby2(16, 40.0, 0.5), False),
        ("integrator", [1.0], [1.0, -1.0], True),
        ("preemph", [1.0, -0.97], [1.0], True),
        ("gain", [0.5], [1.0], True),
        ("a0_is_2", [2.0, 1.0], [2.0, -1.0, 0.5], True),
        ("nb_gt_na", [0.2, 0.3, -0.1, 0.05], [1.0, -0.5], True),
        ("na_gt_nb", [0.3], [1.0, -0.9, 0.5, -0.1], True),
        ("butter3_lp09", *signal.butter(3, 0.9), True),
        ("butter5_lp05", *signal.butter(5, 0.5), True),
        ("butter9_lp03", *signal.butter(9, 0.3), True),
    ]


def lst(a):
    return np.asarray(a, np.float64).tolist()


def out(y):
    return lst(np.asarray(y)[:, AT])


def main():
    rng = np.random.Generator(np.random.PCG64(20261021))
    x32 = (rng.standard_normal((ROWS, N)) + 0.75).astype(np.float32)
    x = x32.astype(np.float64)
    cases = []
    for name, b, a, on_scan in filters():
        b, a = np.atleast_1d(np.asarray(b, np.float64)), np.atleast_1d(np.asarray(a, np.float64))
        order = max(len(b), len(a)) - 1
        try:
            zi = signal.lfilter_zi(b, a) if order else np.zeros(0)
        except np.linalg.LinAlgError:   # a pole at z = 1 has no settled step response: recorded as null
            zi = None
        start = 0.1 * rng.standard_normal((ROWS, order))
        y = signal.lfilter(b, a, x, axis=-1)
        y_zi, zf = signal.lfilter(b, a, x, axis=-1, zi=start) if order else (y, np.zeros((ROWS, 0)))
        past_y, past_x = rng.standard_normal(len(a) - 1), rng.standard_normal(max(len(b) - 2, 0))   # x one short: filled up with a zero
        c = dict(name=name, order=order, b=lst(b), a=lst(a), on_scan=on_scan, lfilter_zi=None if zi is None else lst(zi), y=out(y), zi=lst(start),
                 y_zi=out(y_zi), zf=lst(zf), past_y=lst(past_y), past_x=lst(past_x), lfiltic=lst(signal.lfiltic(b, a, past_y, past_x)))
        if zi is not None and order:
            c["filtfilt"] = {str(p): out(signal.filtfilt(b, a, x, axis=-1, padtype=p)) for p in ("odd", "even", "constant", None)}
            c["filtfilt_padlen"] = out(signal.filtfilt(b, a, x, axis=-1, padtype="even", padlen=PADLEN))
        cases.append(c)
    doc = dict(scipy=scipy.__version__, numpy=np.__version__, sampling_rate=FS, at=AT, padlen=PADLEN, x=[[float(v) for v in r] for r in x32], cases=cases)
    with open(OUT, "w") as f:
        json.dump(doc, f)
        f.write("\n")
    print(f"{OUT}: {len(cases)} filters, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
