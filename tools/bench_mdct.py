"""Transforms.mdct / imdct, device-resident, beside the generic tier, a copy of the bytes moved and the packed STFT pair.
From ONE process, interleaved rounds, warm-up before every timing, median of rounds, on 32 rows x 60 s at 48 kHz:
    mdct_<N> / imdct_<N>            nxsig_mdct_f32 / nxsig_imdct_f32 at N = 1024 and 2048, pad_edges = 0 (mdct.wave / imdct.wave)
    generic_mdct_<N> / _imdct_<N>   the same calls on the same buffers under NXSIG_MDCT_WAVE=0 (mdct.generic / imdct.generic)
    copy_<N>                        hipMemcpyDtoD of the bytes one call moves (4 in + 4 out per sample)
    stft_packed_<N> / istft_packed_<N>   the packed STFT pair at the same N with hop N / 2 through the Python mirror (its result comes
                                    from the context's pooled allocator inside the timing; 4 in + 8 out per sample and back)
Every timing is `--reps` launches between two events.  Before the timing both tiers are compared at the timed size, and the first row's
first 16 frames against the definition in double; a difference above 1e-5 of a row's maximum stops the run.
    usage: python tools/bench_mdct.py [--rounds 5] [--reps 10] [--out profiles/mdct/bench.json]"""
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
ap.add_argument("--rows", type=int, default=32)
ap.add_argument("--seconds", type=float, default=60.0)
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
ROWS, L = args.rows, int(args.seconds * 48000)


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


def row_gap(a, b):
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    return float((np.abs(a - b).max(axis=-1) / np.abs(b).max(axis=-1)).max())


x = ctx.empty((ROWS, L), np.float32)
for r in range(ROWS):   # filled row by row: no second copy of the whole tensor on the host
    part = rng.standard_normal(L, dtype=np.float32)
    ok(lib.nxsig_upload(h_, V(x.ptr + r * L * 4), part.ctypes.data_as(V), part.nbytes))

jobs, check, moved = [], {}, {}
for N in (1024, 2048):
    M = N // 2
    w = T.mdct_window("sine", N)
    F = int(lib.nxsig_mdct_frames(L, N, 0))
    X, y = ctx.empty((ROWS, F, M), np.float32), ctx.empty((ROWS, (F + 1) * M), np.float32)
    fwd = lambda X=X, w=w, N=N: ok(lib.nxsig_mdct_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), L, ROWS, L, w.ctypes.data_as(V), N, 0, 0, V(X.ptr), _lib.DEVICE))
    inv = lambda X=X, y=y, w=w, N=N, F=F: ok(lib.nxsig_imdct_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(X.ptr), F, ROWS, w.ctypes.data_as(V), N, 0, 0, V(y.ptr),
                                                                 (F + 1) * (N // 2), _lib.DEVICE))
    got = {}
    for tier, force in (("wave", None), ("generic", 0)):
        if force is not None:
            ctx.set_tuning("MDCT_WAVE", force)
        fwd()
        rec_f = ctx.last_dispatch()
        inv()
        rec_i = ctx.last_dispatch()
        ctx.sync()
        got[tier] = (X.numpy(), y.numpy(), rec_f, rec_i)
        if force is not None:
            ctx.clear_tuning("MDCT_WAVE")
    n = np.arange(N)
    Cm = np.cos(np.pi / M * (n + 0.5 + M / 2) * (np.arange(M)[:, None] + 0.5))
    x0 = x.numpy()[:1, :17 * M].astype(np.float64)
    ref = np.stack([x0[:, m * M:m * M + N] * w for m in range(16)], axis=1) @ Cm.T
    check[str(N)] = {"wave_against_generic_mdct": row_gap(got["wave"][0], got["generic"][0]), "wave_against_generic_imdct": row_gap(got["wave"][1], got["generic"][1]),
                     "wave_against_definition_16_frames": row_gap(got["wave"][0][:1, :16], ref), "round_trip_interior": row_gap(got["wave"][1][:, M:F * M], x.numpy()[:, M:F * M]),
                     "dispatch": [got["wave"][2], got["wave"][3]], "generic_dispatch": [got["generic"][2], got["generic"][3]], "frames": F}
    assert max(v for v in check[str(N)].values() if isinstance(v, float)) <= 1e-5, check
    del got
    moved[str(N)] = ROWS * (L + F * M) * 4
    spare = ctx.empty((ROWS, F * M), np.float32)
    z = S.stft_packed(x, w, ctx, overlap_length=M, fft_length=N)[0]   # (spectrum, times, frequencies)
    jobs += [(f"mdct_{N}", fwd, None), (f"imdct_{N}", inv, None), (f"generic_mdct_{N}", fwd, 0), (f"generic_imdct_{N}", inv, 0),
             (f"copy_{N}", lambda X=X, spare=spare, F=F, M=M: hip.hipMemcpyDtoDAsync(V(spare.ptr), V(X.ptr), ROWS * F * M * 4, stream), None),
             (f"stft_packed_{N}", lambda w=w, N=N: S.stft_packed(x, w, ctx, overlap_length=N // 2, fft_length=N), None),
             (f"istft_packed_{N}", lambda z=z, w=w, N=N: S.istft_packed(z, w, ctx, overlap_length=N // 2, fft_length=N), None)]

res, disp = {k: [] for k, _, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn, force in jobs:
        if force is not None:
            ctx.set_tuning("MDCT_WAVE", force)
        res[k].append(timed(fn, 2 if k.startswith("generic_") else args.reps))
        disp[k] = "hipMemcpyDtoDAsync" if k.startswith("copy_") else ctx.last_dispatch()
        if force is not None:
            ctx.clear_tuning("MDCT_WAVE")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
ratio = lambda a, b: {str(N): round(med[f"{a}_{N}"] / med[f"{b}_{N}"], 2) for N in (1024, 2048)}
out = {"workload": f"{ROWS} device-resident rows x {L} standard normal samples, sine window, pad_edges 0, norm none", "rounds": args.rounds, "reps": args.reps,
       "device": ctx.name(), "bytes_moved": moved, "check": check, "ms": {k: round(v, 4) for k, v in med.items()},
       "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()}, "dispatch": disp,
       "mdct_over_copy": ratio("mdct", "copy"), "imdct_over_copy": ratio("imdct", "copy"), "mdct_over_stft_packed": ratio("mdct", "stft_packed"),
       "imdct_over_istft_packed": ratio("imdct", "istft_packed"), "generic_over_wave_mdct": ratio("generic_mdct", "mdct"),
       "generic_over_wave_imdct": ratio("generic_imdct", "imdct")}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
