"""Filters.savgol_filter, device-resident, beside a copy, the direct convolution and the FIR path.  From ONE process, interleaved rounds,
warm-up before every timing, median of rounds:
    savgol_W_p_mode_dD[_generic]   nxsig_savgol_filter on 8 rows x 600 s at 48 kHz f32 with (W, p) = (5, 2), (11, 3), (31, 3), (101, 4),
                     (255, 5), modes interp and mirror, deriv 0 and 2, on savgol.tiles and with NXSIG_DISABLE_SAVGOL_TILES (savgol.generic)
    direct_W         nxsig_convolve_direct (convolve(x, k, method="direct", mode="same")) on the same buffer with the same weights as an
                     f32 [1, W] kernel: the same double sums, no boundary rule
    fir_W            filters.fir with W taps, mode "same", on the same buffer (f32 overlap-save)
    rows_tiles / rows_generic   2048 rows x 1 s at (31, 3), interp, deriv 0, on both tiers
    copy_input       hipMemcpyDtoD of the 8 x 600 s input (each byte read once and written once)
    small_call       WALL CLOCK of one call with W = 1025, p = 15 on 1 row x 8192 samples, waited for: the first call of the context
                     with this parameter set (it forms the weights and the 512 x 1025 edge table on the host, in extended precision) and
                     the median of the next 50 (the context's memo hands the tables back)
    usage: python tools/bench_savgol.py [--rounds 5] [--reps 5] [--out profiles/savgol/bench.json]"""
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
from nx_signal_amd import _lib, convolution  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
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
MODES = {"mirror": 0, "interp": 4}
DESIGNS = [(5, 2), (11, 3), (31, 3), (101, 4), (255, 5)]


def ok(rc):
    if rc != 0:
        raise RuntimeError(_lib.last_error())


def timed(fn, reps, warm=1):
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


def savgol_call(x, batch, n, w, p, deriv, mode, y):
    return lambda: lib.nxsig_savgol_filter(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), 0, n, batch, n, w, p, deriv, 1.0, MODES[mode], 0.0, V(y.ptr),
                                           _lib.DEVICE)


B1, n1 = 8, 600 * 48000
x1, y1 = rows(B1, n1), ctx.empty((B1, n1), np.float32)
B2, n2 = 2048, 48000
x2, y2 = rows(B2, n2), ctx.empty((B2, n2), np.float32)
WEIGHTS = {w: S.filters.savgol_coeffs(w, p).astype(np.float32) for w, p in DESIGNS}
KERNELS = {w: ctx.to_device(k.reshape(1, w)) for w, k in WEIGHTS.items()}
SH1 = (C.c_int64 * 2)(B1, n1)


def direct_call(w):
    sh2, osh = (C.c_int64 * 2)(1, w), (C.c_int64 * 2)()
    return lambda: lib.nxsig_convolve_direct(h_, V(x1.ptr), 1, SH1, V(KERNELS[w].ptr), 1, sh2, 2, convolution._MODES["same"], V(y1.ptr), osh,
                                             _lib.DEVICE)


def fir_call(w):
    def fn():
        S.filters.fir(x1, WEIGHTS[w], mode="same")
        return 0
    return fn


def copy():
    return hip.hipMemcpyDtoDAsync(V(y1.ptr), V(x1.ptr), B1 * n1 * 4, stream)


def small_call():
    xs, ys = rows(1, 8192), ctx.empty((1, 8192), np.float32)
    fn, walls = savgol_call(xs, 1, 8192, 1025, 15, 1, "interp", ys), []
    for _ in range(51):
        ctx.sync()
        t0 = time.perf_counter()
        ok(fn())
        ctx.sync()
        walls.append((time.perf_counter() - t0) * 1e3)
    return {"first_ms": round(walls[0], 4), "median_of_next_50_ms": round(sorted(walls[1:])[25], 4), "dispatch": ctx.last_dispatch()}


small = small_call()
jobs = []
for w, p in DESIGNS:
    for mode in ("interp", "mirror"):
        for d in (0, 2):
            jobs.append((f"savgol_{w}_{p}_{mode}_d{d}", savgol_call(x1, B1, n1, w, p, d, mode, y1), None))
            jobs.append((f"savgol_{w}_{p}_{mode}_d{d}_generic", savgol_call(x1, B1, n1, w, p, d, mode, y1), 1))
    jobs.append((f"direct_{w}", direct_call(w), None))
    jobs.append((f"fir_{w}", fir_call(w), None))
jobs += [("rows_tiles", savgol_call(x2, B2, n2, 31, 3, 0, "interp", y2), None), ("rows_generic", savgol_call(x2, B2, n2, 31, 3, 0, "interp", y2), 1),
         ("copy_input", copy, None)]
res, disp = {k: [] for k, _, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn, force in jobs:
        if force:
            ctx.set_tuning("DISABLE_SAVGOL_TILES", 1)
        res[k].append(timed(fn, args.reps))   # the yardsticks and the generic tier get the repetitions of the tile tier
        disp[k] = ctx.last_dispatch() if k != "copy_input" else "hipMemcpyDtoDAsync"
        if force:
            ctx.clear_tuning("DISABLE_SAVGOL_TILES")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
samples = B1 * n1
out = {"workload": "device-resident f32 rows at 48 kHz, standard normal samples", "rounds": args.rounds, "reps": args.reps,
       "device": ctx.name(), "samples": {"long": samples, "rows": B2 * n2}, "tile": lib.nxsig_savgol_tile(),
       "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
       "dispatch": disp,
       "tiles_over_direct": {f"{w}_{mode}_d{d}": round(med[f"savgol_{w}_{p}_{mode}_d{d}"] / med[f"direct_{w}"], 3)
                             for w, p in DESIGNS for mode in ("interp", "mirror") for d in (0, 2)},
       "tiles_over_copy": {f"{w}_{mode}_d{d}": round(med[f"savgol_{w}_{p}_{mode}_d{d}"] / med["copy_input"], 2)
                           for w, p in DESIGNS for mode in ("interp", "mirror") for d in (0, 2)},
       "G_f64_fma_per_s": {f"{w}": round(samples * w / med[f"savgol_{w}_{p}_mirror_d0"] / 1e6, 1) for w, p in DESIGNS},
       "generic_over_tiles": {f"{w}": round(med[f"savgol_{w}_{p}_mirror_d0_generic"] / med[f"savgol_{w}_{p}_mirror_d0"], 2) for w, p in DESIGNS},
       "rows_generic_over_tiles": round(med["rows_generic"] / med["rows_tiles"], 2),
       "small_call_wall_1025_15": small}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
