#!/usr/bin/env python
"""Waveforms on device-resident tensors: every function at 2^26 elements, the median of warm runs timed on HIP
events, next to a device-to-device copy in the same process.  Prints ONE JSON line:

  {"cases": [{"case", "family", "ms", "GB_per_s", "hbm_frac", "vs_copy", "Gelem_per_s"}], "copy_hbm_frac": ...}

GB_per_s counts the algorithmic bytes: t (and a tensor duty) read once, every output written once; hbm_frac is that over 8 TB/s;
vs_copy is that rate over the copy's rate (the copy reads and writes 1 GiB)."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nx_signal_amd as S  # noqa: E402

HBM = 8.0e12
N = 1 << 26


def _time(ctx, fn, runs=7, warm=3):
    for _ in range(warm):
        fn()
    ctx.sync()
    ms = []
    for _ in range(runs):
        ctx.timer_start()
        fn()
        ms.append(ctx.timer_stop())
    return statistics.median(ms)


def _copy_rate(ctx, nbytes):
    """bytes per second (read + write) of hipMemcpyDtoD of nbytes, best of three series of five, host clock around synchronised copies"""
    import time
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
    return 2 * nbytes / best


def main():
    ctx = S.Context(0)
    W = S.waveforms
    rng = np.random.default_rng(0)
    copy = _copy_rate(ctx, 1 << 30)
    cases = []

    def run(name, fn, nbytes):
        fn()
        ctx.sync()
        fam = ctx.last_dispatch()
        ms = _time(ctx, fn)
        rate = nbytes / (ms * 1e-3)
        row = {"case": name, "family": fam, "ms": round(ms, 4), "GB_per_s": round(rate / 1e9, 1), "hbm_frac": round(rate / HBM, 4),
               "vs_copy": round(rate / copy, 4), "Gelem_per_s": round(N / (ms * 1e-3) / 1e9, 2)}
        cases.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
        es = np.dtype(dt).itemsize
        t = ctx.to_device(rng.uniform(-50.0, 50.0, N).astype(dt))
        duty = ctx.to_device(rng.uniform(0.0, 1.0, N).astype(dt))
        run(f"sawtooth width 0.25 {tag}", lambda: W.sawtooth(t, ctx=ctx, width=0.25), 2 * es * N)
        run(f"square duty 0.3 {tag}", lambda: W.square(t, ctx=ctx, duty=0.3), (es + 4) * N)
        run(f"square duty tensor {tag}", lambda: W.square(t, ctx=ctx, duty=duty), (2 * es + 4) * N)
        run(f"gaussian_pulse {tag}", lambda: W.gaussian_pulse(t, ctx=ctx, center_frequency=0.05), 4 * es * N)
        run(f"chirp linear {tag}", lambda: W.chirp(t, 2.0, 40.0, 3.0, ctx=ctx), 2 * es * N)
        run(f"chirp quadratic {tag}", lambda: W.chirp(t, 1.0, 40.0, 3.0, ctx=ctx, method="quadratic"), 2 * es * N)
        run(f"chirp logarithmic {tag}", lambda: W.chirp(t, 0.05, 25.0, 4.75, ctx=ctx, method="logarithmic"), 2 * es * N)
        run(f"chirp hyperbolic {tag}", lambda: W.chirp(t, 1.0, 40.0, 2.0, ctx=ctx, method="hyperbolic"), 2 * es * N)
        run(f"polynomial_sweep 3 coefs {tag}", lambda: W.polynomial_sweep(t, [0.002, 0.0, 0.5], ctx=ctx), 2 * es * N)
        run(f"unit_impulse {tag}", lambda: W.unit_impulse((N,), ctx=ctx, device=True, index="midpoint", type=dt), es * N)
        del t, duty
    print(json.dumps({"bench": "waveforms", "device": ctx.name(), "elements": N, "copy_hbm_frac": round(copy / HBM, 3), "cases": cases}))


if __name__ == "__main__":
    main()
