"""Spectral.cqt, device-resident, on both tiers beside a copy of its input + output bytes.  From ONE process, interleaved rounds, warm-up
before every timing, median of rounds, on x = f32 [32, 1 323 000] (32 x 60 s at 22 050 Hz), hop 512, fmin = C1 (32.703 Hz):
    cqt_<B>_mfma / cqt_<B>_direct    nxsig_cqt_f32 (complex output) on cqt.mfma / cqt.direct (NXSIG_CQT_MFMA=0), the same buffers:
                                     B = 12 bins per octave, 84 bins, and B = 36, 252 bins (7 octaves each)
    copy_<B>                         hipMemcpyDtoD of the input + output bytes
Every timing is `--reps` calls between two events.  The yardstick is arithmetic: a frame costs sum_k N_k products of a real sample and a
complex tap (2 multiply-adds each); cqt.mfma issues them for every cell of its padded table and every frame of its 128-frame blocks.  The
result gives useful and issued products per second and the issued ones as a fraction OF THE SPEC FIGURE of the f32 matrix rate (157
TFLOP/s, 4 flop per product; nobody has measured that rate on this machine).  Before the timing, 6 frames of 4 bins of the first and last
row are compared with the definition in float64; a difference above 1e-5 of the largest of them stops the run.
    usage: python tools/bench_cqt.py [--rounds 5] [--reps 3] [--out profiles/cqt/bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nx_signal_amd as S  # noqa: E402
from nx_signal_amd import _cqt, _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rows", type=int, default=32)
ap.add_argument("--samples", type=int, default=1_323_000)
ap.add_argument("--out", default=None)
args = ap.parse_args()

V = C.c_void_p
lib = _lib.load()
ctx = S.Context(0)
h_ = ctx.handle
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyDtoDAsync.restype, hip.hipMemcpyDtoDAsync.argtypes = C.c_int, [V, V, C.c_size_t, V]
stream = V(lib.nxsig_get_stream(h_))
ROWS, N, SR, HOP, FMIN = args.rows, args.samples, 22050.0, 512, 32.703
CONFIGS = [(12, 84), (36, 252)]
SPEC_PRODUCTS = 157e12 / 4


def p(a):
    return a.ctypes.data_as(V)


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


# a tone per row on a semitone grid plus noise
rng = np.random.Generator(np.random.PCG64(7))
t = np.arange(N) / SR
host = np.sin(2 * np.pi * (110.0 * 2.0 ** (np.arange(ROWS)[:, None] / 12)) * t).astype(np.float32)
host += 0.1 * rng.standard_normal(host.shape, dtype=np.float32)
x = ctx.to_device(host)
frames = int(lib.nxsig_cqt_frames(N, HOP))
jobs, check = [], {}
for B, bins in CONFIGS:
    lo, count, taps = _cqt._bank(SR, FMIN, bins, B, 1.0, 1, True, 0.0)
    out = ctx.empty((ROWS, bins, frames), np.complex64)
    summary = np.zeros(4, np.int64)
    total = int(lib.nxsig_cqt_plan(bins, p(lo), p(count), p(summary), None, None))

    def run(bins=bins, lo=lo, count=count, taps=taps, out=out):
        rc = lib.nxsig_cqt_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), ROWS, N, N, HOP, bins, p(lo), p(count), p(taps), V(out.ptr), 0, _lib.DEVICE)
        if rc != 0:
            raise RuntimeError(_lib.last_error())

    def direct(run=run):
        ctx.set_tuning("CQT_MFMA", 0)
        try:
            run()
        finally:
            ctx.clear_tuning("CQT_MFMA")

    off, worst = np.r_[0, np.cumsum(count)], {}
    for name, fn in (("mfma", run), ("direct", direct)):
        fn()
        assert ctx.last_dispatch() == "cqt." + name, ctx.last_dispatch()
        ctx.sync()
        got, ref = out.numpy(), {}
        for r in (0, ROWS - 1):
            row = np.pad(host[r].astype(np.float64), (int(count.max()), int(count.max())))
            for k in (0, 17, bins // 2, bins - 1):
                for f in (0, 1, 2, frames - 3, frames - 2, frames - 1):
                    s = int(count.max()) + f * HOP + int(lo[k])
                    ref[r, k, f] = row[s:s + count[k]] @ taps[off[k]:off[k + 1]].astype(np.complex128)
        worst[name] = max(abs(got[key] - v) for key, v in ref.items()) / max(abs(v) for v in ref.values())
        assert worst[name] <= 1e-5, (B, name, worst[name])
    io_bytes = ROWS * N * 4 + ROWS * bins * frames * 8
    spare = ctx.empty((io_bytes // 4,), np.float32)
    src = ctx.empty((io_bytes // 4,), np.float32)
    jobs += [(f"cqt_{B}_mfma", run), (f"cqt_{B}_direct", direct),
             (f"copy_{B}", lambda spare=spare, src=src, io_bytes=io_bytes: hip.hipMemcpyDtoDAsync(V(spare.ptr), V(src.ptr), io_bytes, stream))]
    check[B] = {"bins": bins, "longest_bin": int(count.max()), "taps": total, "table_cells": int(summary[2]), "useful_fraction": round(total / int(summary[2]), 3),
                "io_bytes": io_bytes, "useful_products": ROWS * frames * total,
                "issued_products": ROWS * (-(-frames // 128) * 128) * int(summary[2]), "against_definition": {k: float(v) for k, v in worst.items()}}

res, disp = {k: [] for k, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn in jobs:
        res[k].append(timed(fn, args.reps))
        disp[k] = "hipMemcpyDtoDAsync" if k.startswith("copy") else ctx.last_dispatch()
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
out = {"workload": f"device-resident f32 [{ROWS}, {N}]; sr 22050, hop 512, fmin 32.703, {frames} frames per row; cqt_<bins per octave>_<tier>",
       "rounds": args.rounds, "reps": args.reps, "device": ctx.name(), "check": check,
       "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
       "dispatch": disp,
       "direct_over_mfma": {B: round(med[f"cqt_{B}_direct"] / med[f"cqt_{B}_mfma"], 2) for B, _ in CONFIGS},
       "mfma_over_copy": {B: round(med[f"cqt_{B}_mfma"] / med[f"copy_{B}"], 1) for B, _ in CONFIGS},
       "tera_useful_products_per_s": {k: round(check[int(k.split("_")[1])]["useful_products"] / (med[k] * 1e-3) / 1e12, 3) for k in med if k.startswith("cqt")},
       "tera_issued_products_per_s": {B: round(check[B]["issued_products"] / (med[f"cqt_{B}_mfma"] * 1e-3) / 1e12, 3) for B, _ in CONFIGS},
       "issued_fraction_of_the_spec_figure": {B: round(check[B]["issued_products"] / (med[f"cqt_{B}_mfma"] * 1e-3) / SPEC_PRODUCTS, 3) for B, _ in CONFIGS},
       "spec_tera_products_per_s": round(SPEC_PRODUCTS / 1e12, 2)}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
