"""Spectral.yin, device-resident, beside a copy of its input, spectral.lpc at order 16 and stft on the same framing.  From ONE process,
interleaved rounds, warm-up before every timing, median of rounds, on x = f32 [32, 2 880 000] (32 x 60 s at 48 kHz), sr = 48000,
center = 1:
    yin_<L>_<T> / yin_<L>_<T>_cmnd   nxsig_yin_f32 (f0 and v; with the cmnd sink also the rows of c) at frame_length L, hop L / 4, lags
                                     up to T: L = 2048 with fmin / fmax = 65 / 2093 Hz (T = 739) and 200 / 2000 Hz (T = 240), and
                                     L = 1024 with 200 / 2000 Hz (T = 240)
    copy_input                       hipMemcpyDtoD of the input bytes
    lpc_<L>, stft_<L>                spectral.lpc at order 16 / stft (hann) with the same frame length and hop
Every timing is `--reps` calls between two events.  The yardstick is arithmetic: a frame costs W (T + 1) pairs of one double subtraction
and one double FMA; the result gives the achieved pairs per second beside the chip's double-precision vector rate (256 CUs x 64 lanes x
2.4 GHz = 39.3 T instructions per second, so 19.7 T pairs).  Before the timing the first and last row's first and last three frames of
every workload are compared with the definition in float64; a difference above 1e-5 stops the run.
    usage: python tools/bench_yin.py [--rounds 5] [--reps 3] [--out profiles/yin/bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nx_signal_amd as S  # noqa: E402
from nx_signal_amd import _lib, _yin  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rows", type=int, default=32)
ap.add_argument("--samples", type=int, default=2_880_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()

V = C.c_void_p
lib = _lib.load()
ctx = S.Context(0)
h_ = ctx.handle
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyDtoDAsync.restype, hip.hipMemcpyDtoDAsync.argtypes = C.c_int, [V, V, C.c_size_t, V]
stream = V(lib.nxsig_get_stream(h_))
ROWS, N, SR, THR = args.rows, args.samples, 48000.0, 0.1
CONFIGS = [(2048, 65, 2093), (2048, 200, 2000), (1024, 200, 2000)]
PEAK_PAIRS = 256 * 64 * 2.4e9 / 2
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


def yin_frame(x, pmin, pmax):
    """the definition of include/nxsig.h on one frame, in float64: (f0, v, c)"""
    x, W = x.astype(np.float64), len(x) // 2
    d = np.array([np.sum((x[1:W + 1] - x[1 + t:W + 1 + t]) ** 2) for t in range(pmax + 1)])
    tau = np.arange(pmin, pmax + 1)
    c = d[tau] / (np.cumsum(d[1:])[tau - 1] / tau + TINY)
    trough = np.r_[c[0] < c[1], (c[1:-1] < c[:-2]) & (c[1:-1] <= c[2:]), c[-1] < c[-2]]
    hits = np.flatnonzero(trough & (c < THR))
    i, shift = int(hits[0]) if len(hits) else int(np.argmin(c)), 0.0
    if 0 < i < len(c) - 1:
        a, b = c[i + 1] + c[i - 1] - 2 * c[i], (c[i + 1] - c[i - 1]) / 2
        shift = -b / a if abs(b) < abs(a) else 0.0
    return SR / (pmin + i + shift), c[i], c


# a voiced row: five harmonics of a slowly gliding fundamental plus 5 % noise
rng = np.random.Generator(np.random.PCG64(5))
t = np.arange(N) / SR
f = 110.0 * 2.0 ** (np.arange(ROWS)[:, None] / 12)
phase = 2 * np.pi * f * t - 0.02 * f / 5 * np.cos(2 * np.pi * 5 * t)
host = sum(np.sin(k * phase) / k for k in range(1, 6)).astype(np.float32)
host += 0.05 * host.std() * rng.standard_normal(host.shape, dtype=np.float32)
del phase
x = ctx.to_device(host)


def yin_job(L, fmin, fmax, cmnd):
    hop = L // 4
    pmin, pmax = _yin.periods(fmin, fmax, SR, L)
    frames, m = int(lib.nxsig_yin_frames(N, L, hop, 1)), pmax - pmin + 1
    f0, v = ctx.empty((ROWS, frames), np.float32), ctx.empty((ROWS, frames), np.float32)
    cm = ctx.empty((ROWS, frames, m), np.float32) if cmnd else None

    def run():
        ok(lib.nxsig_yin_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), ROWS, N, N, L, hop, 1, pmin, pmax, SR, THR, V(f0.ptr), V(v.ptr),
                             V(cm.ptr) if cmnd else None, _lib.DEVICE))

    run()
    disp = ctx.last_dispatch()
    ctx.sync()
    g0, gv, gc = f0.numpy(), v.numpy(), cm.numpy() if cmnd else None
    padded = np.pad(host[[0, ROWS - 1]], ((0, 0), (L // 2, L // 2)))
    worst = 0.0
    for r, row in zip((0, ROWS - 1), padded):
        for fi in (0, 1, 2, frames - 3, frames - 2, frames - 1):
            r0, rv, rc = yin_frame(row[fi * hop:fi * hop + L], pmin, pmax)
            worst = max(worst, abs(g0[r, fi] - r0) / r0, abs(gv[r, fi] - rv) / rv)
            if cmnd:
                worst = max(worst, np.abs(gc[r, fi] - rc).max() / np.abs(rc).max())
    assert worst <= 1e-5, (disp, L, pmax, worst)
    pairs = ROWS * frames * (L // 2) * (pmax + 1)
    return run, {"dispatch": disp, "frames_per_row": frames, "min_period": pmin, "max_period": pmax, "pairs": pairs, "against_definition": float(worst)}


jobs, check = [], {}
for L, fmin, fmax in CONFIGS:
    for cmnd in (False, True):
        name = f"yin_{L}_{_yin.periods(fmin, fmax, SR, L)[1]}" + ("_cmnd" if cmnd else "")
        run, check[name] = yin_job(L, fmin, fmax, cmnd)
        jobs.append((name, run))

in_bytes = ROWS * N * 4
spare = ctx.empty((ROWS * N,), np.float32)
jobs.append(("copy_input", lambda: hip.hipMemcpyDtoDAsync(V(spare.ptr), V(x.ptr), in_bytes, stream)))
for L in (2048, 1024):
    w = S.windows.hann(L)
    jobs.append((f"lpc_{L}", lambda L=L: S.spectral.lpc(x, 16, L, L // 4, ctx=ctx)))
    jobs.append((f"stft_{L}", lambda L=L, w=w: S.stft(x, w, ctx, overlap_length=L - L // 4)))

res, disp = {k: [] for k, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn in jobs:
        res[k].append(timed(fn, args.reps))
        disp[k] = "hipMemcpyDtoDAsync" if k == "copy_input" else ctx.last_dispatch()
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
rate = {k: c["pairs"] / (med[k] * 1e-3) for k, c in check.items()}
out = {"workload": f"device-resident f32 [{ROWS}, {N}]; sr 48000, center 1, hop frame_length / 4; yin_<frame_length>_<max_period>",
       "rounds": args.rounds, "reps": args.reps, "device": ctx.name(), "input_bytes": in_bytes, "check": check,
       "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
       "dispatch": disp,
       "tera_pairs_per_s": {k: round(v / 1e12, 3) for k, v in rate.items()},
       "peak_tera_pairs_per_s": round(PEAK_PAIRS / 1e12, 2),
       "fraction_of_peak": {k: round(v / PEAK_PAIRS, 3) for k, v in rate.items()},
       "yin_over_copy_input": {k: round(med[k] / med["copy_input"], 1) for k in check},
       "yin_over_lpc": {k: round(med[k] / med[f"lpc_{k.split('_')[1]}"], 2) for k in check},
       "yin_over_stft": {k: round(med[k] / med[f"stft_{k.split('_')[1]}"], 2) for k in check}}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
