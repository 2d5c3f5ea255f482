"""Transforms.dct and mfcc, device-resident, beside a copy, the row transform of nxsig_fft and mel_spectrogram alone.  From ONE process,
interleaved rounds, warm-up before every timing, median of rounds:
    direct_<rows>x<n>_k<keep>   nxsig_dct_f32, type 2, norm "ortho", on 2^22 rows x 80 and x 128 at keep 13, 20 and n (dct.direct)
    fft_<rows>x<n>_k<keep>      the same calls under NXSIG_DISABLE_DCT_DIRECT (dct.fft)
    copy_<rows>x<n>_k<keep>     hipMemcpyDtoD of as many bytes as the call reads and writes (4 n + 4 keep per row)
    fft_32768x1024_k1024, fft_16384x2048_k2048          dct.fft where the plan chooses it, types 2 and 3 (…_t3)
    rowfft_32768x1024, rowfft_16384x2048                one forward nxsig_fft of the same rows (real in, c64 out)
    mel_<framing>, mfcc_<framing>   mel_spectrogram alone and mfcc on 32 rows x 60 s at 48 kHz: N = 1024 / hop 256 / 128 bands / 20
                                    coefficients, and a 400-sample window in a 512-point transform / hop 160 / 80 bands / 13
Every timing is `--reps` launches between two events.  The 2^22-row inputs (1.3 and 2.1 GB) do not fit the 256 MB last-level cache: the
direct rates are HBM rates.  Before the timing every dct shape is computed on its tier(s) at the timed size and the first 64 rows are
compared with the definition in numpy f64 (`check`); a difference above 1e-5 of a row's maximum stops the run.
    usage: python tools/bench_dct.py [--rounds 5] [--reps 20] [--out profiles/dct/bench.json]"""
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
ap.add_argument("--reps", type=int, default=20)
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
SLAB = 65536


def ok(rc):
    if rc != 0:
        raise RuntimeError(_lib.last_error())


def timed(fn, reps, warm=1):
    for _ in range(warm):
        ok(fn())
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def rows(batch, n):
    """standard normal rows; beyond SLAB rows the first slab repeats (the timing does not read the values, the check reads the first 64)"""
    x = ctx.empty((batch, n), np.float32)
    part = rng.standard_normal((min(SLAB, batch), n), dtype=np.float32)
    for r0 in range(0, batch, SLAB):
        take = min(SLAB, batch - r0)
        ok(lib.nxsig_upload(h_, V(x.ptr + r0 * n * 4), part.ctypes.data_as(V), take * n * 4))
    return x


def dct_call(x, batch, n, keep, out, t=2):
    return lambda: lib.nxsig_dct_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), n, batch, n, n, t, 1, keep, V(out.ptr), _lib.DEVICE)


def fft_call(x, batch, n, out):
    return lambda: lib.nxsig_fft(h_, V(x.ptr), 1, batch, n, n, 0, V(out.ptr), _lib.DEVICE)


def copy_call(src, dst, nbytes):
    return lambda: hip.hipMemcpyDtoDAsync(V(dst.ptr), V(src.ptr), nbytes, stream)


def py_call(fn, *a, **kw):
    def run():
        fn(*a, **kw)
        return 0
    return run


def definition(x, t):
    """include/nxsig.h's definition, norm "ortho", in numpy f64"""
    n = x.shape[-1]
    k, j = np.arange(n)[:, None], np.arange(n)[None, :]
    x = x.astype(np.float64)
    if t == 2:
        y = 2.0 * x @ np.cos(np.pi * k * (2 * j + 1) / (2.0 * n)).T
        y[:, 0] *= np.sqrt(1.0 / (4 * n))
        y[:, 1:] *= np.sqrt(1.0 / (2 * n))
        return y
    return x[:, :1] / np.sqrt(n) + np.sqrt(2.0 / n) * (x[:, 1:] @ np.cos(np.pi * (2 * k + 1) * j / (2.0 * n))[:, 1:].T)


def row_gap(a, b):
    return float((np.abs(a - b[:, :a.shape[1]]).max(axis=-1) / np.abs(b).max(axis=-1)).max())


def first_rows(buf, count, width):
    out = np.empty((count, width), np.float32)
    ok(lib.nxsig_download(h_, out.ctypes.data_as(V), V(buf.ptr), out.nbytes))
    return out


jobs, check = [], {}


def checked(name, x, batch, n, keep, out, t, force):
    if force:
        ctx.set_tuning("DISABLE_DCT_DIRECT", 1)
    ok(dct_call(x, batch, n, keep, out, t)())
    ctx.sync()
    rec = ctx.last_dispatch()
    if force:
        ctx.clear_tuning("DISABLE_DCT_DIRECT")
    gap = row_gap(first_rows(out, 64, keep).astype(np.float64), definition(first_rows(x, 64, n), t))
    check[name] = {"against_definition_64_rows": gap, "dispatch": rec}
    assert gap <= 1e-5 and rec.split("+")[0] == ("dct.fft" if force or n > 256 else "dct.direct"), (name, check[name])


BIG = 1 << 22
for n in (80, 128):
    x, out = rows(BIG, n), ctx.empty((BIG, n), np.float32)
    src = ctx.empty((BIG * n,), np.float32)
    for keep in (13, 20, n):
        shape = f"{BIG}x{n}_k{keep}"
        checked(f"direct_{shape}", x, BIG, n, keep, out, 2, False)
        checked(f"fft_{shape}", x, BIG, n, keep, out, 2, True)
        jobs.append((f"direct_{shape}", dct_call(x, BIG, n, keep, out), None))
        jobs.append((f"fft_{shape}", dct_call(x, BIG, n, keep, out), 1))
        # a copy of b bytes reads b and writes b; the call reads 4 n and writes 4 keep per row: the copy moves half of the sum each way
        jobs.append((f"copy_{shape}", copy_call(src, out, BIG * (n + keep) * 2), None))
    del x, out, src
for batch, n in ((32768, 1024), (16384, 2048)):
    x, out, spec = rows(batch, n), ctx.empty((batch, n), np.float32), ctx.empty((batch, n), np.complex64)
    shape = f"{batch}x{n}"
    for t, tag in ((2, ""), (3, "_t3")):
        checked(f"fft_{shape}_k{n}{tag}", x, batch, n, n, out, t, False)
        jobs.append((f"fft_{shape}_k{n}{tag}", dct_call(x, batch, n, n, out, t), None))
    jobs.append((f"rowfft_{shape}", fft_call(x, batch, n, spec), None))
    jobs.append((f"copy_{shape}_k{n}", copy_call(spec, out, batch * n * 4), None))

FS = 48000
audio = rows(32, 60 * FS)
FRAMINGS = {"1024_256_128_20": (S.windows.hann(1024), dict(overlap_length=768, fft_length=1024, sampling_rate=FS, mel_bins=128), 20),
            "400in512_160_80_13": (S.windows.hann(400), dict(overlap_length=240, fft_length=512, sampling_rate=FS, mel_bins=80), 13)}
frames = {}
for name, (w, o, n_mfcc) in FRAMINGS.items():
    got = S.mfcc(audio, w, ctx=ctx, n_mfcc=n_mfcc, **o)
    two = S.transforms.dct(S.mel_spectrogram(audio, w, ctx=ctx, **o), type=2, norm="ortho", keep=n_mfcc)
    a, b = got.numpy(), two.numpy()
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    frames[name] = int(a.shape[0] * a.shape[1])
    del got, two, a, b
    jobs.append((f"mel_{name}", py_call(S.mel_spectrogram, audio, w, ctx=ctx, **o), None))
    jobs.append((f"mfcc_{name}", py_call(S.mfcc, audio, w, ctx=ctx, n_mfcc=n_mfcc, **o), None))

res, disp = {k: [] for k, _, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn, force in jobs:
        if force:
            ctx.set_tuning("DISABLE_DCT_DIRECT", 1)
        res[k].append(timed(fn, args.reps))
        disp[k] = "hipMemcpyDtoDAsync" if k.startswith("copy_") else ctx.last_dispatch()
        if force:
            ctx.clear_tuning("DISABLE_DCT_DIRECT")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
small = [f"{BIG}x{n}_k{keep}" for n in (80, 128) for keep in (13, 20, n)]
long_ = ["32768x1024", "16384x2048"]
out = {"workload": "device-resident f32 rows, standard normal samples; type 2, norm ortho unless _t3", "rounds": args.rounds, "reps": args.reps,
       "device": ctx.name(), "check": check, "frames": frames, "ms": {k: round(v, 4) for k, v in med.items()},
       "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()}, "dispatch": disp,
       "direct_over_copy": {s: round(med[f"direct_{s}"] / med[f"copy_{s}"], 2) for s in small},
       "fft_over_direct": {s: round(med[f"fft_{s}"] / med[f"direct_{s}"], 2) for s in small},
       "direct_faster_than_fft_everywhere": all(med[f"direct_{s}"] < med[f"fft_{s}"] for s in small),
       "direct_gbytes_per_s": {s: round(BIG * (int(s.split("x")[1].split("_")[0]) + int(s.split("_k")[1])) * 4 / med[f"direct_{s}"] / 1e6, 1) for s in small},
       "fft_over_rowfft": {s: round(med[f"fft_{s}_k{s.split('x')[1]}"] / med[f"rowfft_{s}"], 2) for s in long_},
       "fft_t3_over_rowfft": {s: round(med[f"fft_{s}_k{s.split('x')[1]}_t3"] / med[f"rowfft_{s}"], 2) for s in long_},
       "mfcc_over_mel": {k: round(med[f"mfcc_{k}"] / med[f"mel_{k}"], 3) for k in FRAMINGS}}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
