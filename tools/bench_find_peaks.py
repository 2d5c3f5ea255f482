#!/usr/bin/env python
"""PeakFinding.find_peaks on device-resident tensors, timed on HIP events after warm-up, in ONE run next to the two
yardsticks on the same buffer: a device-to-device copy of the input and argrelmax(order=1), the parent's code.  Writes
profiles/find_peaks/bench.json and prints it as ONE JSON line:

  {"groups": [{"group", "shape", "axis", "copy_ms", "argrelmax_ms", "cases": [{"case", "family", "ms", "vs_argrelmax", "vs_copy", "valid", "rounds"}]}]}

Input: the signal of tools/bench_peaks.py (8 x 60 s at 48 kHz, f32 standard_normal, seed 0) and its spectrogram [8, 11247, 512] along
both axes.  vs_argrelmax and vs_copy are time ratios (2.0 = twice as long).  `rounds` is the round count of the distance stage
(nxsig_find_peaks_rounds).  A call with a distance waits for its rounds, so its time includes those waits.  The generic tier's
prominence cases walk whole lines on single threads and are timed once, without warm-up.

    python tools/bench_find_peaks.py [--seconds 60] [--out profiles/find_peaks/bench.json]"""
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
from nx_signal_amd import _find_peaks as PF  # noqa: E402

CONDITION_BITS = {k: 1 << i for i, k in enumerate(PF._CONDITIONS)}
PROPS = PF._F64_PROPS + PF._S32_PROPS


def timed(ctx, fn, laps, warm):
    for _ in range(warm):
        fn()
    ctx.sync()
    best = float("inf")
    for _ in range(3 if warm else 1):
        ctx.timer_start()
        for _ in range(laps):
            fn()
        best = min(best, ctx.timer_stop() / laps)
    return best


def copy_ms(ctx, nbytes):
    hip = C.CDLL("libamdhip64.so")
    a, b = ctx.empty((nbytes,), np.uint8), ctx.empty((nbytes,), np.uint8)
    for _ in range(3):
        hip.hipMemcpyDtoD(C.c_void_p(b.ptr), C.c_void_p(a.ptr), C.c_size_t(nbytes))
    hip.hipDeviceSynchronize()
    best = float("inf")
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(5):
            hip.hipMemcpyDtoD(C.c_void_p(b.ptr), C.c_void_p(a.ptr), C.c_size_t(nbytes))
        hip.hipDeviceSynchronize()
        best = min(best, (time.perf_counter() - t0) / 5)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "find_peaks", "bench.json"))
    a = ap.parse_args()
    ctx, lib = S.Context(0), _lib.load()
    L = 48000 * a.seconds
    rows = np.random.default_rng(0).standard_normal((8, L)).astype(np.float32)
    spec = np.ascontiguousarray(S.spectrogram(rows, S.windows.hann(1024), ctx=ctx, overlap_length=1024 - 256, fft_length=1024)[0])
    doc = {"bench": "find_peaks", "device": ctx.name(), "block": lib.nxsig_find_peaks_block(), "input": [8, L], "groups": []}

    def group(name, x, axis, sets):
        xd = ctx.to_device(x)
        r, size, n = x.ndim, x.size, x.shape[axis]
        sh = (C.c_int64 * r)(*x.shape)
        cp = copy_ms(ctx, x.nbytes)
        idx, valid = ctx.empty((size, r), np.int32), ctx.empty((), np.uint32)
        arg = lambda: _lib.check(lib.nxsig_argrelextrema(ctx.handle, C.c_void_p(xd.ptr), _lib.DT_F32, sh, r, axis, 1, _lib.CMP_GREATER,   # noqa: E731
                                                         C.c_void_p(idx.ptr), C.c_void_p(valid.ptr), _lib.DEVICE))
        am = timed(ctx, arg, 5, 3)
        del idx
        g = {"group": name, "shape": list(x.shape), "axis": axis, "copy_ms": round(cp, 4), "argrelmax_ms": round(am, 4),
             "argrelmax_vs_copy": round(am / cp, 2), "cases": []}
        capacity = (size // n) * ((n - 1) // 2)
        for label, opts, tiers in sets:
            names = [p for k in opts if k in PF._RETURNS for p in PF._RETURNS[k]]
            want = sum(1 << i for i, p in enumerate(PROPS) if p in names)
            nf, ni = bin(want & 0xFF).count("1"), bin(want >> 8).count("1")
            bounds = np.array([[-np.inf, np.inf]] * 5)
            for k, v in opts.items():
                if k in PF._BOUNDED:
                    bounds[PF._BOUNDED.index(k)] = PF._border(k, v)
            cond = sum(CONDITION_BITS[k] for k in opts if k in CONDITION_BITS)
            idx = ctx.empty((capacity, r), np.int32)
            fp, ip = ctx.empty((max(nf, 1), capacity), np.float64), ctx.empty((max(ni, 1), capacity), np.int32)
            fn = lambda: _lib.check(lib.nxsig_find_peaks(_lib.ctx_ptr(ctx.handle, _lib._ctx_peaks), C.c_void_p(xd.ptr), _lib.DT_F32, sh, r, axis,   # noqa: E731
                                                         bounds.ctypes.data_as(C.POINTER(C.c_double)), cond, float(opts.get("distance", 1.0)),
                                                         int(opts.get("wlen", -1)), 0.5, capacity, want, C.c_void_p(idx.ptr), C.c_void_p(valid.ptr),
                                                         C.c_void_p(fp.ptr), C.c_void_p(ip.ptr), _lib.DEVICE))
            for generic in tiers:
                if generic:
                    ctx.set_tuning("DISABLE_FIND_PEAKS_TABLES", 1)
                try:
                    slow = generic and ("prominence" in opts or "width" in opts)
                    ms = timed(ctx, fn, 1, 0) if slow else timed(ctx, fn, 3, 1)
                    row = {"case": label, "family": ctx.last_dispatch(), "ms": round(ms, 4), "vs_argrelmax": round(ms / am, 2),
                           "vs_copy": round(ms / cp, 2), "valid": int(valid.numpy()), "rounds": lib.nxsig_find_peaks_rounds()}
                finally:
                    if generic:
                        ctx.clear_tuning("DISABLE_FIND_PEAKS_TABLES")
                g["cases"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
            del idx, fp, ip
        doc["groups"].append(g)

    both = (False, True)
    group("rows", rows, 1, [("no condition", {}, both), ("height 1.0", {"height": 1.0}, both), ("distance 480", {"distance": 480}, both),
                            ("prominence 1.0", {"prominence": 1.0}, both), ("prominence 1.0, width 2", {"prominence": 1.0, "width": 2}, both),
                            ("prominence 1.0, wlen 4801", {"prominence": 1.0, "wlen": 4801}, both)])
    light = [("no condition", {}, both), ("prominence 1.0", {"prominence": 1.0}, (False,)), ("distance 8", {"distance": 8}, (False,))]
    group("spectrogram, time axis", spec, 1, light)
    group("spectrogram, bins axis", spec, 2, light)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
