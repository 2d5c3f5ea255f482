#!/usr/bin/env python
"""PeakFinding on device-resident tensors: every case timed on HIP events after warm-up, next to a device-to-device
copy on the same box.  Prints ONE JSON line:

  {"cases": [{"case", "family", "ms", "GB_per_s", "hbm_frac", "vs_copy", "density"}], "copy_hbm_frac": ...}

GB_per_s counts the algorithmic bytes: the input read once, the s32 indices (4 * rank * size) and the u32 count written once; hbm_frac
is that over 8 TB/s; vs_copy is that rate over the copy's rate (the copy reads and writes 1 GiB); density is valid / size."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nx_signal_amd as S  # noqa: E402
from nx_signal_amd import _lib  # noqa: E402

HBM = 8.0e12
DT = {np.dtype(np.float32): _lib.DT_F32, np.dtype(np.float64): _lib.DT_F64, np.dtype(np.int64): _lib.DT_S64}


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


def main():
    ctx = S.Context(0)
    lib = _lib.load()
    rng = np.random.default_rng(0)
    copy = _copy_rate(ctx, 1 << 30)
    cases = []

    def run(name, x, axis, order, nonzero=False):
        shape, r = x.shape, x.ndim
        size = int(np.prod(shape))
        xd = x if isinstance(x, S.DeviceBuffer) else ctx.to_device(x)
        sh = (C.c_int64 * r)(*shape)
        idx, valid = ctx.empty((size, r), np.int32), ctx.empty((), np.uint32)
        if nonzero:
            fn = lambda: _lib.check(lib.nxsig_nonzero(ctx.handle, C.c_void_p(xd.ptr), sh, r, C.c_void_p(idx.ptr), C.c_void_p(valid.ptr), _lib.DEVICE))
        else:
            fn = lambda: _lib.check(lib.nxsig_argrelextrema(ctx.handle, C.c_void_p(xd.ptr), DT[np.dtype(xd.dtype)], sh, r, axis, order,
                                                            _lib.CMP_GREATER, C.c_void_p(idx.ptr), C.c_void_p(valid.ptr), _lib.DEVICE))
        fn()
        ctx.sync()
        fam = ctx.last_dispatch()
        ms = _time(ctx, fn)
        nbytes = size * np.dtype(xd.dtype).itemsize + 4 * r * size + 4
        rate = nbytes / (ms * 1e-3)
        row = {"case": name, "family": fam, "ms": round(ms, 4), "GB_per_s": round(rate / 1e9, 1), "hbm_frac": round(rate / HBM, 3),
               "vs_copy": round(rate / copy, 3), "density": round(int(valid.numpy()) / size, 4)}
        cases.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del xd, idx, valid

    L = 48000 * 60
    rows = rng.standard_normal((8, L)).astype(np.float32)
    for order in (1, 8, 64, 512):
        run(f"rows 8 x 60 s @ 48 kHz f32 axis 1 order {order}", rows, 1, order)
    run("rank-1 60 s @ 48 kHz f32 order 1", rows[0], 0, 1)
    run("rows 8 x 60 s f64 axis 1 order 1", rows.astype(np.float64), 1, 1)
    run("rows 8 x 60 s s64 axis 1 order 1", (rows * 1000).astype(np.int64), 1, 1)
    spec = S.spectrogram(rows, S.windows.hann(1024), ctx=ctx, overlap_length=1024 - 256, fft_length=1024)[0]
    spec = np.ascontiguousarray(spec)
    for axis, what in ((1, "time"), (2, "bins")):
        for order in (1, 8):
            run(f"spectrogram magnitude {list(spec.shape)} axis {axis} ({what}) order {order}", spec, axis, order)
    run("nonzero u8 mask 8 x 60 s (30 % set)", (rng.random((8, L)) < 0.3).astype(np.uint8), None, None, nonzero=True)
    print(json.dumps({"bench": "peaks", "device": ctx.name(), "copy_hbm_frac": round(copy / HBM, 3), "cases": cases}))


if __name__ == "__main__":
    main()
