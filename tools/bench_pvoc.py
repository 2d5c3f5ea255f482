"""Transforms.phase_vocoder, device-resident, beside a copy of the bytes it is given and returns, and time_stretch beside stft + istft.
From ONE process, interleaved rounds, warm-up before every timing, median of rounds, on z = c64 [8, 11247, 1024] (8 x 60 s at 48 kHz,
N = 1024, hop 256):
    pvoc_<rate>           nxsig_phase_vocoder_c64 at rates 0.8, 1.0, 1.25 (pvoc.scan)
    copy_<rate>           hipMemcpyDtoD that moves the same input + output bytes: (in + out) / 2 bytes read and written once
    time_stretch / stft_istft   transforms.time_stretch(x, 1.0, hann) and the stft + istft it contains, through the Python mirror (their
                          results come from the context's pooled allocator inside the timing)
`bytes_ratio` is (2 in + out) / (in + out): what a purely memory-bound pvoc.scan, which reads z twice, would take over the copy.
Every timing is `--reps` launches between two events.  Before the timing rows 0 and 7, bins 0 ... 7, of every rate are compared with the
wrap-free definition in long double; a difference above 1e-5 of the row's maximum stops the run.
    usage: python tools/bench_pvoc.py [--rounds 5] [--reps 10] [--out profiles/pvoc/bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nx_signal_amd as S  # noqa: E402
from nx_signal_amd import _lib, transforms as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rows", type=int, default=8)
ap.add_argument("--frames", type=int, default=11247)
ap.add_argument("--bins", type=int, default=1024)
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
ROWS, M, K = args.rows, args.frames, args.bins
RATES = (0.8, 1.0, 1.25)


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


def reference(z, rate):
    """the definition of include/nxsig.h on z[M, k], wrap-free in long double"""
    s = np.arange(len(np.arange(0, z.shape[0], rate)), dtype=np.float64) * rate
    i = np.floor(s).astype(np.int64)
    al = (s - i)[:, None]
    zp = np.concatenate([z, np.zeros_like(z[:2])]).astype(np.complex128)
    ang = np.where(zp == 0, 0, np.arctan2(zp.imag.astype(np.longdouble), zp.real.astype(np.longdouble)))
    d = ang[i + 1] - ang[i]
    phase = np.fmod(ang[:1] + np.cumsum(d, axis=0) - d, 2 * np.pi * np.longdouble(1)).astype(np.float64)
    return ((1 - al) * np.abs(zp[i]) + al * np.abs(zp[i + 1])) * np.exp(1j * phase)


z = ctx.empty((ROWS, M, K), np.complex64)
kept = {}
for r in range(ROWS):   # filled row by row: no second copy of the whole tensor on the host
    part = (rng.standard_normal((M, K), dtype=np.float32) + 1j * rng.standard_normal((M, K), dtype=np.float32)).astype(np.complex64)
    ok(lib.nxsig_upload(h_, V(z.ptr + r * M * K * 8), part.ctypes.data_as(V), part.nbytes))
    if r in (0, ROWS - 1):
        kept[r] = part[:, :8].copy()
    del part

in_bytes = ROWS * M * K * 8
jobs, check, moved, ratio_bytes, chunks = [], {}, {}, {}, {}
spare = ctx.empty((int(in_bytes / min(RATES)) // 8 + 1,), np.complex64)
for rate in RATES:
    n_out = int(lib.nxsig_pvoc_frames(M, rate))
    out = ctx.empty((ROWS, n_out, K), np.complex64)
    run = lambda out=out, rate=rate: ok(lib.nxsig_phase_vocoder_c64(_lib.ctx_ptr(h_, _lib._ctx_iir), V(z.ptr), ROWS, M, K, rate, V(out.ptr), _lib.DEVICE))
    run()
    disp = ctx.last_dispatch()
    ctx.sync()
    got = out.numpy()
    err = max(float(np.abs(got[r, :, :8] - ref).max() / np.abs(ref).max()) for r, ref in ((r, reference(kept[r], rate)) for r in kept))
    del got
    check[str(rate)] = {"rows_0_and_last_bins_0_to_7_against_definition": err, "dispatch": disp, "n_out": n_out}
    assert err <= 1e-5, check
    out_bytes = ROWS * n_out * K * 8
    moved[str(rate)] = in_bytes + out_bytes
    ratio_bytes[str(rate)] = round((2 * in_bytes + out_bytes) / (in_bytes + out_bytes), 3)
    src = z if in_bytes >= out_bytes else out
    jobs += [(f"pvoc_{rate}", run),
             (f"copy_{rate}", lambda src=src, n=(in_bytes + out_bytes) // 2: hip.hipMemcpyDtoDAsync(V(spare.ptr), V(src.ptr), n, stream))]

w, o = S.windows.hann(1024), {"overlap_length": 768}
x = ctx.to_device(rng.standard_normal((ROWS, (M - 1) * 256 + 1024), dtype=np.float32))
jobs += [("time_stretch", lambda: T.time_stretch(x, 1.0, w, ctx, **o)),
         ("stft_istft", lambda: S.istft(S.stft(x, w, ctx, **o)[0], w, ctx, **o))]

res, disp = {k: [] for k, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn in jobs:
        res[k].append(timed(fn, args.reps))
        disp[k] = "hipMemcpyDtoDAsync" if k.startswith("copy_") else ctx.last_dispatch()
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
out = {"workload": f"device-resident c64 [{ROWS}, {M}, {K}] standard normal spectrogram; time_stretch on f32 [{ROWS}, {(M - 1) * 256 + 1024}], hann 1024, hop 256",
       "rounds": args.rounds, "reps": args.reps, "device": ctx.name(), "bytes_in_plus_out": moved, "bytes_ratio": ratio_bytes, "check": check,
       "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()},
       "dispatch": disp, "pvoc_over_copy": {str(r): round(med[f"pvoc_{r}"] / med[f"copy_{r}"], 3) for r in RATES},
       "time_stretch_over_stft_istft": round(med["time_stretch"] / med["stft_istft"], 3)}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
