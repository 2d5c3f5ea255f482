"""Spectral.welch / csd, device-resident, beside what a user had before them.  From ONE process, interleaved rounds, warm-up before
every timing, median of rounds:
    welch_1024      nxsig_welch_f32 on 32 rows x 60 s at 48 kHz, N = fft_length = 1024, hop 256 (welch.pair)
    power_1024      nxsig_stft_magnitude_f32 (kind power) on the SAME buffer: the same transforms, 2 KB per frame stored — the only
                    on-device route to a spectrum that could then be averaged
    copy_input      hipMemcpyDtoD of the input's bytes (each byte read once and written once)
    welch_generic   the same welch call with NXSIG_DISABLE_WELCH_WAVE (welch.generic)
    welch_2048      8 rows x 600 s, N = fft_length = 2048, hop 512
    csd_1024        16 + 16 rows x 60 s, N = fft_length = 1024, hop 256 (csd.pair; Pxx, Pyy and Pxy)
The condition of DESIGN.md section 3.12: welch_1024 takes less time than power_1024 of the same run; the ratio to the copy is a figure.
    usage: python tools/bench_welch.py [--rounds 5] [--reps 10] [--out profiles/welch/bench.json]"""
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


def rows(batch, n):
    x = ctx.empty((batch, n), np.float32)
    for r in range(batch):   # filled row by row: no second copy of the whole tensor on the host
        row = rng.standard_normal(n, dtype=np.float32)
        ok(lib.nxsig_upload(h_, V(x.ptr + r * n * 4), row.ctypes.data_as(V), row.nbytes))
    return x


def welch_call(x, batch, n, w, N, hop, out):
    wp = w.ctypes.data_as(V)
    return lambda: lib.nxsig_welch_f32(_lib.ctx_ptr(h_, _lib._ctx_spectral), V(x.ptr), n, batch, n, wp, N, hop, N, 1, 0, 48000.0, V(out.ptr), _lib.DEVICE)


w1, w2 = S.windows.hann(1024), S.windows.hann(2048)
B1, n1 = 32, 60 * 48000
x1 = rows(B1, n1)
M1 = (n1 - 1024) // 256 + 1
pxx1 = ctx.empty((B1, 513), np.float32)
spec = ctx.empty((B1, M1, 512), np.float32)
cp = ctx.empty((B1, n1), np.float32)
params = _lib.StftParams(1024, 256, 1024, _lib.PAD_VALID, 0, 0, _lib.SCALE_NONE, 0, 48000.0)
nf = C.c_int64()
B2, n2 = 8, 600 * 48000
x2 = rows(B2, n2)
pxx2 = ctx.empty((B2, 1025), np.float32)
Bc = 16
pc = [ctx.empty((Bc, 513), np.float32), ctx.empty((Bc, 513), np.float32), ctx.empty((Bc, 513), np.complex64)]


def power():
    return lib.nxsig_stft_magnitude_f32(h_, V(x1.ptr), n1, B1, n1, w1.ctypes.data_as(V), C.byref(params), _lib.MAG_POWER, V(spec.ptr), C.byref(nf),
                                        _lib.DEVICE)


def copy():
    return hip.hipMemcpyDtoDAsync(V(cp.ptr), V(x1.ptr), B1 * n1 * 4, stream)


def csd():   # rows 0 .. 15 against rows 16 .. 31 of the same buffer
    return lib.nxsig_csd_f32(_lib.ctx_ptr(h_, _lib._ctx_spectral), V(x1.ptr), V(x1.ptr + Bc * n1 * 4), n1, Bc, n1, w1.ctypes.data_as(V), 1024, 256, 1024, 1, 0, 48000.0,
                             V(pc[0].ptr), V(pc[1].ptr), V(pc[2].ptr), _lib.DEVICE)


welch1 = welch_call(x1, B1, n1, w1, 1024, 256, pxx1)
jobs = [("welch_1024", welch1, None), ("power_1024", power, None), ("copy_input", copy, None), ("welch_generic", welch1, 1),
        ("welch_2048", welch_call(x2, B2, n2, w2, 2048, 512, pxx2), None), ("csd_1024", csd, None)]
res, disp = {k: [] for k, _, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn, force in jobs:
        if force:
            ctx.set_tuning("DISABLE_WELCH_WAVE", 1)
        res[k].append(timed(fn, args.reps if not force else max(2, args.reps // 3)))
        disp[k] = ctx.last_dispatch() if k != "copy_input" else "hipMemcpyDtoDAsync"
        if force:
            ctx.clear_tuning("DISABLE_WELCH_WAVE")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
M2 = (n2 - 2048) // 512 + 1
out = {"workload": "device-resident f32 rows at 48 kHz, hann windows, detrend constant, density", "rounds": args.rounds, "reps": args.reps,
       "device": ctx.name(), "frames": {"welch_1024": B1 * M1, "welch_2048": B2 * M2, "csd_1024": Bc * M1},
       "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
       "dispatch": disp,
       "welch_over_power": round(med["welch_1024"] / med["power_1024"], 3),
       "welch_over_copy": round(med["welch_1024"] / med["copy_input"], 3),
       "welch_frac_of_8TBps_input_bytes": round(B1 * n1 * 4 / (med["welch_1024"] * 1e-3) / 8e12, 4),
       "generic_over_pair": round(med["welch_generic"] / med["welch_1024"], 2),
       "M_frames_per_s": {"welch_1024": round(B1 * M1 / med["welch_1024"] / 1e3, 1), "power_1024": round(B1 * M1 / med["power_1024"] / 1e3, 1),
                          "welch_2048": round(B2 * M2 / med["welch_2048"] / 1e3, 1), "csd_1024": round(Bc * M1 / med["csd_1024"] / 1e3, 1)},
       "condition_welch_faster_than_power": bool(med["welch_1024"] < med["power_1024"])}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
