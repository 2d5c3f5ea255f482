#!/usr/bin/env python
"""Filters.median / wiener on device-resident tensors: every shape timed on HIP events after warm-up, next to a
device-to-device copy of the same input bytes on the same box.  Prints ONE JSON line:

  {"cases": [{"case", "family", "ms", "GB_per_s", "hbm_frac", "vs_copy", "Gout_per_s", ...}], "copy_hbm_frac": ...}

GB_per_s counts the algorithmic bytes (input read once + output written once); hbm_frac is that over 8 TB/s; vs_copy is that rate over
the copy's rate on the same box (the copy reads and writes the input's bytes).  Median rows also report the compare-exchange count of
their network per output (ops_per_out) and the lane-op rate it implies over the chip's 256 CUs x 128 lanes x 2.4 GHz (valu_frac)."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nx_signal_amd as S  # noqa: E402
from nx_signal_amd import _lib  # noqa: E402

HBM = 8.0e12
VALU = 256 * 128 * 2.4e9


def _time(ctx, fn, laps=5, warm=3):
    for _ in range(warm):
        fn()
    ctx.sync()
    best = float("inf")
    for _ in range(3):
        ctx.timer_start()
        for _ in range(laps):
            fn()
        best = min(best, ctx.timer_stop() / laps)
    return best


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


def _batcher_cx(n):
    """comparators of Batcher's odd-even merge sort on n live inputs (padded to a power of two; the ones that touch padding fold)"""
    P = 1
    while P < n:
        P *= 2
    cnt, p = 0, 1
    while p < P:
        k = p
        while k >= 1:
            j = k % p
            while j + k < P:
                for i in range(k):
                    a, b = i + j, i + j + k
                    if b < P and a // (2 * p) == b // (2 * p) and b < n:
                        cnt += 1
                j += 2 * k
            k //= 2
        p *= 2
    return cnt


def main():
    ctx = S.Context(0)
    lib = _lib.load()
    rng = np.random.default_rng(0)
    cases = []

    def run(name, shape, dtype, fn_kind, ks, noise=None, extra=None):
        x = ctx.to_device(rng.standard_normal(shape).astype(dtype))
        r = len(shape)
        sh, kc = (C.c_int64 * r)(*shape), (C.c_int64 * r)(*ks)
        n = int(np.prod(shape))
        if fn_kind == "median":
            y = ctx.empty(shape, np.float32)
            fn = lambda: _lib.check(lib.nxsig_median_filter(ctx.handle, C.c_void_p(x.ptr), int(dtype == np.float64), sh, r, kc, C.c_void_p(y.ptr), _lib.DEVICE))
            out_b = 4
        else:
            y = ctx.empty(shape, dtype)
            fn = lambda: _lib.check(lib.nxsig_wiener(ctx.handle, C.c_void_p(x.ptr), int(dtype == np.float64), sh, r, kc, int(noise is not None),
                                                     float(noise or 0.0), C.c_void_p(y.ptr), None, _lib.DEVICE))
            out_b = np.dtype(dtype).itemsize
        fn()
        ctx.sync()
        fam = ctx.last_dispatch()
        ms = _time(ctx, fn)
        in_b = np.dtype(dtype).itemsize
        rate = n * (in_b + out_b) / (ms * 1e-3)
        copy = _copy_rate(ctx, n * in_b)
        row = {"case": name, "family": fam, "ms": round(ms, 4), "GB_per_s": round(rate / 1e9, 1), "hbm_frac": round(rate / HBM, 3),
               "vs_copy": round(rate / copy, 3), "Gout_per_s": round(n / ms / 1e6, 2)}
        row.update(extra or {})
        if "ops_per_out" in row:
            row["valu_frac"] = round(row["ops_per_out"] * n / (ms * 1e-3) / VALU, 3)
        cases.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del x, y

    L = 48000 * 60
    for k in (3, 5, 9, 15, 31):
        # two outputs per thread share one network over k - 1 samples: per output half of it (2 ops a comparator) + the merge
        ops = (2 * _batcher_cx(k - 1) + (4 if k % 2 else 8)) / 2
        run(f"median rows 8 x 60 s @ 48 kHz {{1, {k}}} f32", (8, L), np.float32, "median", (1, k), extra={"ops_per_out": ops})
    for k in (3, 5, 7):
        run(f"median plane 16 x 1024^2 {k}x{k} f32", (16, 1024, 1024), np.float32, "median", (1, k, k))
    run("median generic 64^3 {3,3,3} f32", (64, 64, 64), np.float32, "median", (3, 3, 3))
    for k in (3, 5):
        for dt in (np.float32, np.float64):
            for noise in (None, 0.5):
                run(f"wiener plane 16 x 1024^2 {k}x{k} {np.dtype(dt).name} noise={'nil' if noise is None else noise}", (16, 1024, 1024), dt, "wiener",
                    (1, k, k), noise=noise, extra={"f64_adds_per_out": 2 * k * k})
    copy_frac = _copy_rate(ctx, 1 << 30) / HBM
    print(json.dumps({"bench": "filters", "device": ctx.name(), "copy_hbm_frac": round(copy_frac, 3), "cases": cases}))


if __name__ == "__main__":
    main()
