"""Spectral.lombscargle, device-resident f32 rows, on both tiers, beside SciPy on the host.  From ONE process, interleaved rounds, median
of rounds:
    long_B        n = 100 000 samples, F = 10 000 angular frequencies, batch B = 1, 8, 64, 512 ("power", no weights)
    bootstrap     n = 1 000, F = 1 000, batch 4 096 (shuffled rows on one time base: a false-alarm estimate)
    *_generic     the same call with NXSIG_LOMBSCARGLE_TILE=0 (lombscargle.generic); the two heaviest run once per round, unwarmed
    scipy_*       scipy.signal.lombscargle on the host for ONE row of the shape (the long shape on 200 of its frequencies, scaled to
                  10 000: SciPy forms n x F temporaries)
    host_*        wall clock of the call's host side — the finiteness checks, the normalised weights, hashing x / freqs / weights for
                  the table cache — in a first call (the tables are uploaded) and in a repeated one (nothing is)
Reported: ms per call and (t, w) pairs per second, n F batch / time.  The aims DESIGN.md section 3.19 reads off this file: the tile
tier is faster than the generic tier on every shape, and batch 8 costs less than twice batch 1.
    usage: python tools/bench_lombscargle.py [--rounds 5] [--out profiles/lombscargle/bench.json] [--no-scipy]"""
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
ap.add_argument("--out", default=None)
ap.add_argument("--no-scipy", action="store_true")
ap.add_argument("--scale", type=int, default=1, help="divide n and F of the long shape by this (a quick look)")
args = ap.parse_args()

V = C.c_void_p
lib = _lib.load()
ctx = S.Context(0)
h_ = ctx.handle
rng = np.random.Generator(np.random.PCG64(11))


def ok(rc):
    if rc != 0:
        raise RuntimeError(_lib.last_error())


def shape(n, F, batch):
    x = np.sort(rng.uniform(0.0, 1000.0, n))
    freqs = np.linspace(0.01, 50.0, F)
    y = (np.sin(7.5 * x) + rng.standard_normal((batch, n))).astype(np.float32)
    return x, freqs, y


def call(x, freqs, yd, batch, out):
    n, F = x.shape[0], freqs.shape[0]
    return lambda: lib.nxsig_lombscargle(_lib.ctx_ptr(h_, _lib._ctx_iir), V(yd.ptr), 0, n, batch, n, x.ctypes.data_as(V), freqs.ctypes.data_as(V), F,
                                         None, 0, 0, 0, V(out.ptr), _lib.DEVICE)


def timed(fn, reps, warm):
    for _ in range(warm):
        ok(fn())
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        ok(fn())
    return ctx.timer_stop() / reps


nL, FL = 100_000 // args.scale, 10_000 // args.scale
xL, fL, yL = shape(nL, FL, 512)
ydL, outL = ctx.to_device(yL), ctx.empty((512, FL), np.float32)
nB, FB_, BB = 1000, 1000, 4096
xB, fB, yB = shape(nB, FB_, 1)
yB = np.stack([rng.permutation(yB[0]) for _ in range(BB)])
ydB, outB = ctx.to_device(yB), ctx.empty((BB, FB_), np.float32)

# (name, call, pairs, generic?, reps, warm-up calls)
jobs = []
for b in (1, 8, 64, 512):
    pairs = nL * FL * b
    jobs.append((f"long_{b}", call(xL, fL, ydL, b, outL), pairs, False, 3 if b <= 8 else 1, 1))
    jobs.append((f"long_{b}_generic", call(xL, fL, ydL, b, outL), pairs, True, 1, 1 if b <= 8 else 0))
jobs.append(("bootstrap", call(xB, fB, ydB, BB, outB), nB * FB_ * BB, False, 3, 1))
jobs.append(("bootstrap_generic", call(xB, fB, ydB, BB, outB), nB * FB_ * BB, True, 1, 1))
res, disp = {k: [] for k, *_ in jobs}, {}
for r in range(args.rounds):
    for k, fn, pairs, generic, reps, warm in jobs:
        if generic:
            ctx.set_tuning("LOMBSCARGLE_TILE", 0)
        res[k].append(timed(fn, reps, warm))
        disp[k] = ctx.last_dispatch()
        if generic:
            ctx.clear_tuning("LOMBSCARGLE_TILE")
        print(f"round {r} {k}: {res[k][-1]:.3f} ms ({disp[k]})", file=sys.stderr, flush=True)
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
pairs_of = {k: p for k, _, p, *_ in jobs}


# the host side of a call: wall clock until the (asynchronous) call returns, on batch 1
def host_ms(x, freqs, yd, out, fresh):
    ts = []
    for i in range(5):
        xi = x + (i + 1) * 1e-9 if fresh else x      # other bits: a miss in the table cache, the tables are uploaded
        fn = call(xi, freqs, yd, 1, out)
        ctx.sync()
        t0 = time.perf_counter()
        ok(fn())
        ts.append((time.perf_counter() - t0) * 1e3)
        ctx.sync()
    return sorted(ts)[len(ts) // 2]


host = {"long_first": host_ms(xL, fL, ydL, outL, True), "long_repeat": host_ms(xL, fL, ydL, outL, False),
        "bootstrap_first": host_ms(xB, fB, ydB, outB, True), "bootstrap_repeat": host_ms(xB, fB, ydB, outB, False)}

scipy_ms = {}
if not args.no_scipy:
    import scipy
    import scipy.signal
    sub = fL[::max(1, FL // 200)]
    t0 = time.perf_counter()
    scipy.signal.lombscargle(xL, yL[0].astype(np.float64), sub)
    scipy_ms["long_one_row"] = (time.perf_counter() - t0) * 1e3 * FL / sub.shape[0]
    t0 = time.perf_counter()
    scipy.signal.lombscargle(xB, yB[0].astype(np.float64), fB)
    scipy_ms["bootstrap_one_row"] = (time.perf_counter() - t0) * 1e3
    scipy_ms["version"] = scipy.__version__
    scipy_ms["long_frequencies_timed"] = int(sub.shape[0])

out = {"workload": "device-resident f32 rows on one time base, normalize='power', no weights; x sorted uniform in [0, 1000), w in [0.01, 50]",
       "rounds": args.rounds, "device": ctx.name(), "block": [lib.nxsig_lombscargle_block(w) for w in range(3)],
       "shapes": {"long": [nL, FL], "bootstrap": [nB, FB_, BB]},
       "ms": {k: round(v, 3) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in res.items()},
       "dispatch": disp,
       "G_pairs_per_s": {k: round(pairs_of[k] / med[k] / 1e6, 2) for k in med},
       "generic_over_tile": {k: round(med[k + "_generic"] / med[k], 2) for k in med if not k.endswith("_generic")},
       "batch8_over_batch1": round(med["long_8"] / med["long_1"], 2),
       "host_ms": {k: round(v, 3) for k, v in host.items()},
       "scipy_ms": {k: (round(v, 1) if isinstance(v, float) else v) for k, v in scipy_ms.items()}}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
