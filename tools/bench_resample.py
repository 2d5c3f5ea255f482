"""Filters.resample_poly on 8 x 600 s rows, device-resident: 48 k -> 16 k, 44.1 k -> 16 k, 48 k -> 44.1 k and 16 k -> 48 k in f32 and
48 k -> 16 k in c64, each with its default filter.  Per shape, from the same run: ms per call of nxsig_resample_poly (and of its generic
tier), the fraction of 8 TB/s its input + output bytes come to, a hipMemcpyDtoD that moves the same number of bytes (half of them read,
half written), and nxsig_fir_f32 with the same taps on the same input — the only device-side alternative without this entry point,
which computes every output at the input rate (`down` times more than needed; c64 rows: their two planes as 2 x rows).  Interleaved
rounds in one process, warm-up before every timing, median of rounds.
    usage: python tools/bench_resample.py [--rounds 5] [--reps 10] [--seconds 600] [--out profiles/resample/bench.json]"""
import argparse
import ctypes as C
import json
import math
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
ap.add_argument("--seconds", type=int, default=600)
ap.add_argument("--rows", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()

V = C.c_void_p
lib = _lib.load()
ctx = S.Context(0)
h_ = ctx.handle
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyDtoDAsync.restype, hip.hipMemcpyDtoDAsync.argtypes = C.c_int, [V, V, C.c_size_t, V]
stream = V(lib.nxsig_get_stream(h_))


def ok(rc):
    if rc != 0:
        raise RuntimeError(_lib.last_error())


def timed(fn, reps, warm=3):
    for _ in range(warm):
        ok(fn())
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


SHAPES = [("48k_to_16k_f32", 48000, 16000, np.float32), ("44k1_to_16k_f32", 44100, 16000, np.float32),
          ("48k_to_44k1_f32", 48000, 44100, np.float32), ("16k_to_48k_f32", 16000, 48000, np.float32),
          ("48k_to_16k_c64", 48000, 16000, np.complex64)]
B = args.rows
rng = np.random.Generator(np.random.PCG64(3))
out = {"workload": f"{B} rows x {args.seconds} s, default Kaiser(5.0) filters, device-resident", "rounds": args.rounds, "reps": args.reps,
       "tile": int(lib.nxsig_resample_tile()), "shapes": {}}
for name, fs_in, fs_out, dtype in SHAPES:
    g = math.gcd(fs_in, fs_out)
    up, down = fs_out // g, fs_in // g
    n = fs_in * args.seconds
    n_out = int(lib.nxsig_resample_length(n, up, down))
    es = np.dtype(dtype).itemsize
    is_c = int(es == 8)
    taps = S.filters.resample_poly_taps(up, down)
    hp = taps.ctypes.data_as(V)
    x = ctx.empty((B, n), dtype)
    for r in range(B):   # filled row by row: no second copy of the whole tensor on the host
        row = rng.standard_normal(n * (2 if is_c else 1), dtype=np.float32)
        ok(lib.nxsig_upload(h_, V(x.ptr + r * n * es), row.ctypes.data_as(V), row.nbytes))
    y = ctx.empty((B, n_out), dtype)
    yf = ctx.empty((B * (2 if is_c else 1), n), np.float32)          # fir's result: every output at the input rate
    traffic = B * (n + n_out) * es
    cp_src, cp_dst = ctx.empty((traffic // 2,), np.uint8), ctx.empty((traffic // 2,), np.uint8)

    def resample():
        return lib.nxsig_resample_poly(_lib.ctx_ptr(h_), V(x.ptr), is_c, n, B, n, hp, taps.shape[0], up, down, V(y.ptr), _lib.DEVICE)

    def copy():
        return hip.hipMemcpyDtoDAsync(V(cp_dst.ptr), V(cp_src.ptr), traffic // 2, stream)

    def fir():   # c64 rows: the interleaved planes are not rows of a real filter; an equal number of f32 samples stands in for them
        return lib.nxsig_fir_f32(h_, V(x.ptr), n, B * (2 if is_c else 1), n, hp, taps.shape[0], _lib.CONV_SAME, V(yf.ptr), _lib.DEVICE)

    jobs = [("resample", resample, None), ("resample_generic", resample, 1), ("copy_same_bytes", copy, None), ("fir_same_taps", fir, None)]
    res, disp = {k: [] for k, _, _ in jobs}, {}
    for _ in range(args.rounds):
        for k, fn, force in jobs:
            if force:
                ctx.set_tuning("DISABLE_RESAMPLE_LDS", 1)
            res[k].append(timed(fn, args.reps if k != "resample_generic" else max(2, args.reps // 3)))
            disp[k] = ctx.last_dispatch() if k != "copy_same_bytes" else "hipMemcpyDtoDAsync"
            if force:
                ctx.clear_tuning("DISABLE_RESAMPLE_LDS")
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    row = {"up": up, "down": down, "taps": int(taps.shape[0]), "samples_in": B * n, "samples_out": B * n_out, "in_plus_out_bytes": traffic}
    for k in med:
        row[k + "_ms"] = round(med[k], 4)
        row[k + "_dispatch"] = disp[k]
    row["resample_frac_of_8TBps"] = round(traffic / (med["resample"] * 1e-3) / 8e12, 4)
    row["copy_frac_of_8TBps"] = round(traffic / (med["copy_same_bytes"] * 1e-3) / 8e12, 4)
    row["resample_over_copy"] = round(med["resample"] / med["copy_same_bytes"], 3)
    row["fir_over_resample"] = round(med["fir_same_taps"] / med["resample"], 2)
    row["generic_over_lds"] = round(med["resample_generic"] / med["resample"], 2)
    row["G_outputs_per_s"] = round(B * n_out / (med["resample"] * 1e-3) / 1e9, 2)
    row["T_fma_per_s"] = round(B * n_out * math.ceil(taps.shape[0] / up) * (2 if is_c else 1) / (med["resample"] * 1e-3) / 1e12, 2)
    out["shapes"][name] = row
    print(name, json.dumps(row), flush=True)
    for b in (x, y, yf, cp_src, cp_dst):
        b.free()
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
