"""Convolution.correlate_rows, device-resident, beside hilbert.wave at the same transform length, one forward row transform and a copy.
From ONE process, interleaved rounds, warm-up before every timing, median of rounds:
    wave_<shape>_f32     nxsig_xcorr (correlate, full) on 32 768 real pairs x (600, 300) (K = 1024) and 16 384 x (1500, 549) (K = 2048): xcorr.wave
    wave_<shape>_c64     the same shapes as c64 pairs (xcorr.wave at K = 1024; at 2048 points c64 pairs are xcorr.generic's and say so)
    peak_<shape>_f32     the real pairs under the peak sink (lag and value per pair, no rows written)
    phat_<shape>_f32     the real pairs with the PHAT weighting
    generic_<shape>_*    the real and c64 calls on the same buffers under NXSIG_XCORR_WAVE=0 (xcorr.generic)
    generic_64x48000     64 real pairs x (48 000, 48 000), P = 131 072 (xcorr.generic)
    hilbert_<shape>      nxsig_hilbert_f32, the analytic signal of as many rows of n1 samples zero-padded to K (hilbert.wave): one forward and
                         one inverse core per row, the aim for a real pair
    fft_<shape>          one forward nxsig_fft of those rows at K points (real in, c64 out)
    copy_<shape>         hipMemcpyDtoD of as many bytes as the real call reads and writes (4 (n1 + n2 + n1 + n2 - 1) per pair)
Every timing is `--reps` launches between two events.  Before the timing every shape is computed on both tiers at the timed size and
compared: pair by pair against each other, and the first 8 pairs against the definition in double (tests/xcorr_oracle.py); a difference
above 1e-5 of a row's maximum stops the run.  The result line goes to --out, a Markdown table of it to --table.
    usage: python tools/bench_xcorr.py [--rounds 5] [--reps 20] [--out profiles/xcorr/bench.json] [--table profiles/xcorr/bench_table.md]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import xcorr_oracle as O  # noqa: E402
import nx_signal_amd as S  # noqa: E402
from nx_signal_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--table", default=None)
args = ap.parse_args()

V = C.c_void_p
lib = _lib.load()
ctx = S.Context(0)
h_ = ctx.handle
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyDtoDAsync.restype, hip.hipMemcpyDtoDAsync.argtypes = C.c_int, [V, V, C.c_size_t, V]
stream = V(lib.nxsig_get_stream(h_))
rng = np.random.Generator(np.random.PCG64(5))


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


def rows(batch, n, cplx=False):
    x = ctx.empty((batch, n), np.complex64 if cplx else np.float32)
    width = 2 * n if cplx else n
    for r0 in range(0, batch, 1024):   # filled in slabs: no second copy of the whole tensor on the host
        part = rng.standard_normal((min(1024, batch - r0), width), dtype=np.float32)
        ok(lib.nxsig_upload(h_, V(x.ptr + r0 * width * 4), part.ctypes.data_as(V), part.nbytes))
    return x


def xcorr_call(a, b, batch, n1, n2, cplx, out, weighting=0, sink=0, lags=None):
    return lambda: lib.nxsig_xcorr(_lib.ctx_ptr(h_, _lib._ctx_iir), V(a.ptr), n1, n1, V(b.ptr), n2, n2, batch, int(cplx), 1, 0, weighting, 0.0, sink,
                                   V(out.ptr), V(lags.ptr) if lags is not None else None, _lib.DEVICE)


def hilbert_call(x, batch, n, n_fft, out):
    return lambda: lib.nxsig_hilbert_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), n, batch, n, n_fft, 0, V(out.ptr), _lib.DEVICE)


def fft_call(x, batch, n, n_fft, out):
    return lambda: lib.nxsig_fft(h_, V(x.ptr), 1, batch, n, n_fft, 0, V(out.ptr), _lib.DEVICE)


def copy_call(src, dst, nbytes):
    return lambda: hip.hipMemcpyDtoDAsync(V(dst.ptr), V(src.ptr), nbytes, stream)


def row_gap(a, b):
    return float((np.abs(a - b).max(axis=-1) / np.abs(b).max(axis=-1)).max())


jobs, check, shapes, moved = [], {}, [], {}
for batch, n1, n2 in ((32768, 600, 300), (16384, 1500, 549)):
    shape = f"{batch}x{n1}_{n2}"
    shapes.append(shape)
    K, n_out = lib.nxsig_xcorr_fft_length(n1, n2), n1 + n2 - 1
    big = ctx.empty((batch, K), np.complex64)
    for cplx in (False, True):
        t = "c64" if cplx else "f32"
        a, b, out = rows(batch, n1, cplx), rows(batch, n2, cplx), ctx.empty((batch, n_out), np.complex64 if cplx else np.float32)
        call = xcorr_call(a, b, batch, n1, n2, cplx, out)
        ok(call())
        ctx.sync()
        wave_rec, wave = ctx.last_dispatch(), out.numpy()
        ctx.set_tuning("XCORR_WAVE", 0)
        ok(call())
        ctx.clear_tuning("XCORR_WAVE")
        ctx.sync()
        generic_rec, generic = ctx.last_dispatch(), out.numpy()
        ref = O.rows(a.numpy()[:8], b.numpy()[:8], "correlate", "full")
        check[f"{shape}_{t}"] = {"default_against_generic": row_gap(wave, generic), "default_against_definition_8_pairs": row_gap(wave[:8], ref),
                                 "generic_against_definition_8_pairs": row_gap(generic[:8], ref), "dispatch": wave_rec, "generic_dispatch": generic_rec, "K": K}
        assert max(v for v in check[f"{shape}_{t}"].values() if isinstance(v, float)) <= 1e-5, check
        del wave, generic
        jobs.append((f"wave_{shape}_{t}", call, None))
        jobs.append((f"generic_{shape}_{t}", call, 0))
        if not cplx:
            vals, lags = ctx.empty((batch,), np.float32), ctx.empty((batch,), np.int32)
            jobs.append((f"peak_{shape}_f32", xcorr_call(a, b, batch, n1, n2, False, vals, sink=1, lags=lags), None))
            jobs.append((f"phat_{shape}_f32", xcorr_call(a, b, batch, n1, n2, False, out, weighting=1), None))
            moved[shape] = batch * 4 * (n1 + n2 + n_out)
            src = ctx.empty((moved[shape] // 8 + 1,), np.float32)
            jobs.append((f"hilbert_{shape}", hilbert_call(a, batch, n1, K, big), None))
            jobs.append((f"fft_{shape}", fft_call(a, batch, n1, K, big), None))
            jobs.append((f"copy_{shape}", copy_call(src, big, moved[shape] // 2), None))
LB, LN = 64, 48000
al, bl, outl = rows(LB, LN), rows(LB, LN), ctx.empty((LB, 2 * LN - 1), np.float32)
long_call = xcorr_call(al, bl, LB, LN, LN, False, outl)
ok(long_call())
ctx.sync()
check["64x48000"] = {"generic_against_definition_1_pair": row_gap(outl.numpy()[:1], O.rows(al.numpy()[:1], bl.numpy()[:1], "correlate", "full")),
                     "dispatch": ctx.last_dispatch(), "P": lib.nxsig_xcorr_fft_length(LN, LN)}
assert check["64x48000"]["generic_against_definition_1_pair"] <= 1e-5, check
jobs.append(("generic_64x48000", long_call, None))

res, disp = {k: [] for k, _, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn, force in jobs:
        if force is not None:
            ctx.set_tuning("XCORR_WAVE", force)
        res[k].append(timed(fn, 3 if k == "generic_64x48000" else args.reps))
        disp[k] = "hipMemcpyDtoDAsync" if k.startswith("copy_") else ctx.last_dispatch()
        if force is not None:
            ctx.clear_tuning("XCORR_WAVE")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
out = {"workload": "device-resident pairs, standard normal samples, correlate, mode full", "rounds": args.rounds, "reps": args.reps, "device": ctx.name(),
       "bytes_moved": moved, "check": check, "ms": {k: round(v, 4) for k, v in med.items()},
       "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()}, "dispatch": disp,
       "generic_over_wave_f32": {s: round(med[f"generic_{s}_f32"] / med[f"wave_{s}_f32"], 2) for s in shapes},
       "wave_f32_over_hilbert_wave": {s: round(med[f"wave_{s}_f32"] / med[f"hilbert_{s}"], 2) for s in shapes},
       "wave_f32_over_fft": {s: round(med[f"wave_{s}_f32"] / med[f"fft_{s}"], 2) for s in shapes},
       "wave_f32_over_copy": {s: round(med[f"wave_{s}_f32"] / med[f"copy_{s}"], 2) for s in shapes},
       "peak_over_rows_f32": {s: round(med[f"peak_{s}_f32"] / med[f"wave_{s}_f32"], 2) for s in shapes},
       "c64_over_f32": {s: round(med[f"wave_{s}_c64"] / med[f"wave_{s}_f32"], 2) for s in shapes}}
line = json.dumps(out)
print(line)
table = ["| case | ms (median) | min .. max | dispatch |", "|---|---|---|---|"]
table += [f"| `{k}` | {med[k]:.4f} | {min(res[k]):.4f} .. {max(res[k]):.4f} | {disp[k]} |" for k, _, _ in jobs]
print("\n".join(table))
for path, text in ((args.out, line), (args.table, "\n".join(table))):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
