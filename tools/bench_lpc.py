"""Spectral.lpc, device-resident, on both tiers, beside a copy of its input, stft with the same framing and the traffic of the staged
tier.  From ONE process, interleaved rounds, warm-up before every timing, median of rounds, on x = f32 [32, 2 880 000] (32 x 60 s at
48 kHz):
    wave_<p> / rows_<p>   nxsig_lpc_f32 (a, k and e) at frame_length 1024, hop 256 (359 904 frames), orders 8 / 16 / 32, on lpc.wave and
                          on the same buffers under NXSIG_LPC_WAVE=0 (lpc.rows)
    whole_16              the first 8 rows whole (frame_length = n) at order 16: lpc.rows
    copy_input            hipMemcpyDtoD of the input bytes
    stft                  stft(x, hann(1024), overlap_length=768) through the Python mirror (its result comes from the pooled allocator)
    whole_traffic_16      16 hipMemcpyDtoD of 2 x 8 bytes per sample of the 8 rows: what lpc.rows' stage launches read and write
Every timing is `--reps` calls between two events.  Before the timing the first and last row's first and last three frames of every
workload are compared with the definition in float64; a difference above 1e-5 stops the run.
    usage: python tools/bench_lpc.py [--rounds 5] [--reps 3] [--out profiles/lpc/bench.json]"""
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rows", type=int, default=32)
ap.add_argument("--samples", type=int, default=2_880_000)
ap.add_argument("--whole-rows", type=int, default=8)
ap.add_argument("--out", default=None)
args = ap.parse_args()

V = C.c_void_p
lib = _lib.load()
ctx = S.Context(0)
h_ = ctx.handle
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyDtoDAsync.restype, hip.hipMemcpyDtoDAsync.argtypes = C.c_int, [V, V, C.c_size_t, V]
stream = V(lib.nxsig_get_stream(h_))
ROWS, N, WHOLE = args.rows, args.samples, min(args.whole_rows, args.rows)
L, HOP, ORDERS = 1024, 256, (8, 16, 32)
TINY = np.finfo(np.float64).tiny


def ok(rc):
    if rc != 0:
        raise RuntimeError(_lib.last_error())


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def burg(x, p):
    """the definition of include/nxsig.h on one frame, in float64"""
    x = x.astype(np.float64)
    f, b, a, ks = x[1:], x[:-1], np.ones(1), []
    for _ in range(p):
        k = -2 * np.sum(f * b) / (np.sum(f * f) + np.sum(b * b) + TINY)
        a = np.append(a, 0)
        a = a + k * a[::-1]
        f, b = (f + k * b)[1:], (b + k * f)[:-1]
        ks.append(k)
    return a, np.array(ks), np.sum(x * x) / len(x) * np.prod(1 - np.square(ks))


# an AR(2) resonance plus noise, so that the coefficients are not all near zero
rng = np.random.Generator(np.random.PCG64(5))
host = rng.standard_normal((ROWS, N), dtype=np.float32)
host[:, 1:] += 0.9 * host[:, :-1]
x = ctx.to_device(host)
F = int(lib.nxsig_lpc_frames(N, L, HOP))


def lpc_job(rows, frame, hop, p, wave):
    frames = int(lib.nxsig_lpc_frames(N, frame, hop))
    a, k, e = ctx.empty((rows, frames, p + 1), np.float32), ctx.empty((rows, frames, p), np.float32), ctx.empty((rows, frames), np.float32)

    def run():
        if not wave:
            ctx.set_tuning("LPC_WAVE", 0)
        try:
            ok(lib.nxsig_lpc_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), rows, N, N, frame, hop, p, V(a.ptr), V(k.ptr), V(e.ptr), _lib.DEVICE))
        finally:
            if not wave:
                ctx.clear_tuning("LPC_WAVE")

    run()
    disp = ctx.last_dispatch()
    ctx.sync()
    ga, gk, ge = a.numpy(), k.numpy(), e.numpy()
    worst = 0.0
    for r in (0, rows - 1):
        for fi in sorted({0, 1, 2, frames - 3, frames - 2, frames - 1} & set(range(frames))):
            ra, rk, re = burg(host[r, fi * hop:fi * hop + frame], p)
            worst = max(worst, np.abs(ga[r, fi] - ra).max() / np.abs(ra).max(), np.abs(gk[r, fi] - rk).max() / np.abs(rk).max(), abs(ge[r, fi] - re) / re)
    assert worst <= 1e-5, (disp, p, worst)
    return run, {"dispatch": disp, "frames_per_row": frames, "against_definition": float(worst)}


jobs, check = [], {}
for p in ORDERS:
    for name, wave in (("wave", True), ("rows", False)):
        run, check[f"{name}_{p}"] = lpc_job(ROWS, L, HOP, p, wave)
        jobs.append((f"{name}_{p}", run))
run, check["whole_16"] = lpc_job(WHOLE, N, N, 16, True)
jobs.append(("whole_16", run))

in_bytes = ROWS * N * 4
spare = ctx.empty((max(in_bytes, WHOLE * N * 16) // 4,), np.float32)
pairs = ctx.empty((WHOLE * N * 16 // 4,), np.float32)
w, o = S.windows.hann(L), {"overlap_length": L - HOP}
jobs += [("copy_input", lambda: hip.hipMemcpyDtoDAsync(V(spare.ptr), V(x.ptr), in_bytes, stream)),
         ("stft", lambda: S.stft(x, w, ctx, **o)),
         ("whole_traffic_16", lambda: [hip.hipMemcpyDtoDAsync(V(spare.ptr), V(pairs.ptr), WHOLE * N * 16, stream) for _ in range(16)])]

res, disp = {k: [] for k, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn in jobs:
        res[k].append(timed(fn, args.reps))
        disp[k] = "hipMemcpyDtoDAsync" if k in ("copy_input", "whole_traffic_16") else ctx.last_dispatch()
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
out = {"workload": f"device-resident f32 [{ROWS}, {N}]; frame_length {L}, hop {HOP}: {F} frames per row; whole rows: the first {WHOLE}",
       "rounds": args.rounds, "reps": args.reps, "device": ctx.name(), "input_bytes": in_bytes, "check": check,
       "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
       "dispatch": disp,
       "rows_over_wave": {str(p): round(med[f"rows_{p}"] / med[f"wave_{p}"], 2) for p in ORDERS},
       "wave_over_copy_input": {str(p): round(med[f"wave_{p}"] / med["copy_input"], 2) for p in ORDERS},
       "wave_over_stft": {str(p): round(med[f"wave_{p}"] / med["stft"], 2) for p in ORDERS},
       "wave_ms_per_order": {str(p): round(med[f"wave_{p}"] / p, 4) for p in ORDERS},
       "whole_over_traffic": round(med["whole_16"] / med["whole_traffic_16"], 3)}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
