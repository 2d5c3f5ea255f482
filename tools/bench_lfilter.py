"""Filters.lfilter / filtfilt, device-resident, beside a copy and sosfilt with as many states.  From ONE process, interleaved rounds,
warm-up before every timing, median of rounds:
    lfilter_N        nxsig_lfilter_f32 on 8 rows x 600 s at 48 kHz at order N = 1, 2, 4, 8, 16 (lfilter.scan)
    filtfilt_N       nxsig_filtfilt_f32 on the same buffer, N = 2, 4 (odd padding, scipy's default padlen)
    sosfilt_S        the yardstick: nxsig_sosfilt_f32 with S = ceil(N / 2) sections on the same buffer (sosfilt.scan)
    rows_scan / rows_generic   2048 rows x 1 s at order 2, on lfilter.scan and with NXSIG_DISABLE_LFILTER_SCAN (lfilter.generic)
    copy_input       hipMemcpyDtoD of the 8 x 600 s input (each byte read once and written once)
The filters are recorded designs the conditioning guard lets onto the scan (tests/golden/lfilter_vectors.json: a leaky integrator,
butter(2, .2), butter(4, .1), butter(4, [.2, .4], "bp"), butter(16, .4)); the sections of the yardstick are resonators with poles at
radius 0.99, as in tools/bench_iir.py.  The aim DESIGN.md section 3.18 reads off this file: order 2 S costs no more than S sections.
    usage: python tools/bench_lfilter.py [--rounds 5] [--reps 10] [--out profiles/lfilter/bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nx_signal_amd as S  # noqa: E402
from nx_signal_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

V = C.c_void_p
lib = _lib.load()
ctx = S.Context(0)
h_ = ctx.handle
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyDtoDAsync.restype, hip.hipMemcpyDtoDAsync.argtypes = C.c_int, [V, V, C.c_size_t, V]
stream = V(lib.nxsig_get_stream(h_))
rng = np.random.Generator(np.random.PCG64(5))
with open(os.path.join(ROOT, "tests", "golden", "lfilter_vectors.json")) as f:
    RECORDED = {c["name"]: (np.array(c["b"], np.float64), np.array(c["a"], np.float64)) for c in json.load(f)["cases"]}
BA = {1: (np.array([0.05]), np.array([1.0, -0.95])), 2: RECORDED["butter2_lp02"], 4: RECORDED["butter4_lp01"], 8: RECORDED["butter4_bp"],
      16: RECORDED["butter16_lp04"]}
ORDERS = (1, 2, 4, 8, 16)


def ok(rc):
    if rc != 0:
        raise RuntimeError(_lib.last_error())


def timed(fn, reps, warm=2):
    for _ in range(warm):
        ok(fn())
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def rows(batch, n):
    x = ctx.empty((batch, n), np.float32)
    for r in range(batch):   # filled row by row: no second copy of the whole tensor on the host
        row = rng.standard_normal(n, dtype=np.float32)
        ok(lib.nxsig_upload(h_, V(x.ptr + r * n * 4), row.ctypes.data_as(V), row.nbytes))
    return x


def cascade(sections):
    sos = np.zeros((sections, 6))
    for k in range(sections):
        r, th = 0.99, 0.02 + 0.11 * k
        a1, a2 = -2.0 * r * np.cos(th), r * r
        sos[k] = np.array([0.25, 0.5, 0.25, 0.0, 0.0, 0.0]) * (1.0 + a1 + a2) + np.array([0.0, 0.0, 0.0, 1.0, a1, a2])
    return np.ascontiguousarray(sos)


def lfilter_call(x, batch, n, ba, y):
    b, a = ba
    return lambda: lib.nxsig_lfilter_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), n, batch, n, b.ctypes.data_as(V), len(b), a.ctypes.data_as(V), len(a),
                                         None, 1, None, 0, V(y.ptr), _lib.DEVICE)


def filtfilt_call(x, batch, n, ba, y):
    b, a = ba
    return lambda: lib.nxsig_filtfilt_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), n, batch, n, b.ctypes.data_as(V), len(b), a.ctypes.data_as(V), len(a),
                                          1, -1, V(y.ptr), _lib.DEVICE)


def sosfilt_call(x, batch, n, sos, y):
    return lambda: lib.nxsig_sosfilt_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), n, batch, n, sos.ctypes.data_as(V), sos.shape[0], None, 1, None, 0,
                                         V(y.ptr), _lib.DEVICE)


B1, n1 = 8, 600 * 48000
x1, y1 = rows(B1, n1), ctx.empty((B1, n1), np.float32)
B2, n2 = 2048, 48000
x2, y2 = rows(B2, n2), ctx.empty((B2, n2), np.float32)
SOS = {s: cascade(s) for s in (1, 2, 4, 8)}


def copy():
    return hip.hipMemcpyDtoDAsync(V(y1.ptr), V(x1.ptr), B1 * n1 * 4, stream)


jobs = [(f"lfilter_{n}", lfilter_call(x1, B1, n1, BA[n], y1), None) for n in ORDERS]
jobs += [(f"filtfilt_{n}", filtfilt_call(x1, B1, n1, BA[n], y1), None) for n in (2, 4)]
jobs += [(f"sosfilt_{s}", sosfilt_call(x1, B1, n1, SOS[s], y1), None) for s in (1, 2, 4, 8)]
jobs += [("rows_scan", lfilter_call(x2, B2, n2, BA[2], y2), None), ("rows_generic", lfilter_call(x2, B2, n2, BA[2], y2), 1), ("copy_input", copy, None)]
res, disp = {k: [] for k, _, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn, force in jobs:
        if force:
            ctx.set_tuning("DISABLE_LFILTER_SCAN", 1)
        res[k].append(timed(fn, args.reps if k not in ("lfilter_16", "sosfilt_8", "rows_generic") else max(2, args.reps // 3)))
        disp[k] = ctx.last_dispatch() if k != "copy_input" else "hipMemcpyDtoDAsync"
        if force:
            ctx.clear_tuning("DISABLE_LFILTER_SCAN")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
samples = B1 * n1
out = {"workload": "device-resident f32 rows at 48 kHz; recorded designs the guard lets onto the scan", "rounds": args.rounds, "reps": args.reps,
       "device": ctx.name(), "samples": {"long": samples, "rows": B2 * n2},
       "chunk_tile": {str(n): [lib.nxsig_lfilter_chunk(n), lib.nxsig_lfilter_tile(n)] for n in ORDERS},
       "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
       "dispatch": disp,
       "over_copy": {k: round(med[k] / med["copy_input"], 2) for k in med if k.startswith(("lfilter", "filtfilt"))},
       # the aim: order N against sosfilt with ceil(N / 2) sections, timed in this run
       "over_sosfilt": {f"lfilter_{n}": round(med[f"lfilter_{n}"] / med[f"sosfilt_{(n + 1) // 2}"], 2) for n in ORDERS},
       "G_samples_per_s": {k: round(samples / med[k] / 1e6, 2) for k in med if k.startswith(("lfilter", "filtfilt"))},
       "rows_generic_over_scan": round(med["rows_generic"] / med["rows_scan"], 2)}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
