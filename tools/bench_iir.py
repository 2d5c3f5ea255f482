"""Filters.sosfilt / sosfiltfilt, device-resident, beside a copy and the FIR path.  From ONE process, interleaved rounds, warm-up before
every timing, median of rounds:
    sosfilt_S        nxsig_sosfilt_f32 on 8 rows x 600 s at 48 kHz with S = 1, 2, 4, 8, 16 sections (sosfilt.scan)
    sosfiltfilt_S    nxsig_sosfiltfilt_f32 on the same buffer, S = 2, 4 (odd padding, scipy's default padlen)
    rows_scan / rows_generic   2048 rows x 1 s, 2 sections, on sosfilt.scan and with NXSIG_DISABLE_SOSFILT_SCAN (sosfilt.generic)
    small_call       WALL CLOCK of one sosfilt call with 16 sections on 1 row x 8192 samples, waited for: the first call of the
                     context with this cascade (it forms the powers of the state matrix on the host, in extended precision) and the
                     median of the next 50 (the context's memo hands the matrices back) — host work that event timing does not see
    copy_input       hipMemcpyDtoD of the 8 x 600 s input (each byte read once and written once)
    fir_257          filters.fir with 257 taps, mode "same", on the same buffer
The cascades are low-pass resonator sections with poles at radius 0.99 (unit DC gain), so that every output stays of the input's size.
Where the kernel turns from memory-bound to f64-bound shows in ms per section: DESIGN.md section 3.13 reads it off this file.
    usage: python tools/bench_iir.py [--rounds 5] [--reps 10] [--out profiles/iir/bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

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


def sosfilt_call(x, batch, n, sos, y):
    return lambda: lib.nxsig_sosfilt_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), n, batch, n, sos.ctypes.data_as(V), sos.shape[0], None, 1, None, 0,
                                         V(y.ptr), _lib.DEVICE)


def filtfilt_call(x, batch, n, sos, y):
    return lambda: lib.nxsig_sosfiltfilt_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), n, batch, n, sos.ctypes.data_as(V), sos.shape[0], 1, -1, V(y.ptr),
                                             _lib.DEVICE)


B1, n1 = 8, 600 * 48000
x1, y1 = rows(B1, n1), ctx.empty((B1, n1), np.float32)
B2, n2 = 2048, 48000
x2, y2 = rows(B2, n2), ctx.empty((B2, n2), np.float32)
taps = S.filters.firwin(257, [4000], sampling_rate=48000)
SOS = {s: cascade(s) for s in (1, 2, 4, 8, 16)}


def copy():
    return hip.hipMemcpyDtoDAsync(V(y1.ptr), V(x1.ptr), B1 * n1 * 4, stream)


def fir():
    S.filters.fir(x1, taps, mode="same")
    return 0


def small_call():
    xs, ys = rows(1, 8192), ctx.empty((1, 8192), np.float32)
    sos = cascade(16) * np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.9999])   # a cascade this context has not seen
    fn, walls = sosfilt_call(xs, 1, 8192, np.ascontiguousarray(sos), ys), []
    for _ in range(51):
        ctx.sync()
        t0 = time.perf_counter()
        ok(fn())
        ctx.sync()
        walls.append((time.perf_counter() - t0) * 1e3)
    return {"first_ms": round(walls[0], 4), "median_of_next_50_ms": round(sorted(walls[1:])[25], 4), "dispatch": ctx.last_dispatch()}


small = small_call()
jobs = [(f"sosfilt_{s}", sosfilt_call(x1, B1, n1, SOS[s], y1), None) for s in (1, 2, 4, 8, 16)]
jobs += [(f"sosfiltfilt_{s}", filtfilt_call(x1, B1, n1, SOS[s], y1), None) for s in (2, 4)]
jobs += [("rows_scan", sosfilt_call(x2, B2, n2, SOS[2], y2), None), ("rows_generic", sosfilt_call(x2, B2, n2, SOS[2], y2), 1),
         ("copy_input", copy, None), ("fir_257", fir, None)]
res, disp = {k: [] for k, _, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn, force in jobs:
        if force:
            ctx.set_tuning("DISABLE_SOSFILT_SCAN", 1)
        res[k].append(timed(fn, args.reps if k not in ("sosfilt_16", "sosfilt_8", "rows_generic") else max(2, args.reps // 3)))
        disp[k] = ctx.last_dispatch() if k != "copy_input" else "hipMemcpyDtoDAsync"
        if force:
            ctx.clear_tuning("DISABLE_SOSFILT_SCAN")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
samples = B1 * n1
out = {"workload": "device-resident f32 rows at 48 kHz; resonator sections with poles at radius 0.99", "rounds": args.rounds, "reps": args.reps,
       "device": ctx.name(), "samples": {"long": samples, "rows": B2 * n2},
       "chunk_tile": {str(s): [lib.nxsig_sosfilt_chunk(s), lib.nxsig_sosfilt_tile(s)] for s in (1, 2, 4, 8, 16)},
       "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
       "dispatch": disp,
       "over_copy": {k: round(med[k] / med["copy_input"], 2) for k in med if k.startswith("sosfilt")},
       "G_samples_per_s": {k: round(samples / med[k] / 1e6, 2) for k in med if k.startswith("sosfilt")},
       # two reads and a write of the row, and the chunk states written by pass 1 and read by pass 2: 2 * (2 S doubles) per chunk
       "bytes_per_sample": {f"sosfilt_{s}": 12 + 32 * s / lib.nxsig_sosfilt_chunk(s) for s in (1, 2, 4, 8, 16)},
       "frac_of_8TBps": {f"sosfilt_{s}": round(samples * (12 + 32 * s / lib.nxsig_sosfilt_chunk(s)) / (med[f"sosfilt_{s}"] * 1e-3) / 8e12, 4)
                         for s in (1, 2, 4, 8, 16)},
       "small_call_wall_16_sections": small,
       "G_f64_fma_per_s_two_passes": {f"sosfilt_{s}": round(samples * 10 * s / med[f"sosfilt_{s}"] / 1e6, 1) for s in (1, 2, 4, 8, 16)},
       "rows_generic_over_scan": round(med["rows_generic"] / med["rows_scan"], 2)}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
