"""Filters.hilbert, device-resident, beside a copy, one forward row transform and the FIR path.  From ONE process, interleaved rounds,
warm-up before every timing, median of rounds:
    wave_<shape>_<output>      nxsig_hilbert_f32 on 16 384 rows x 2048 and 32 768 rows x 1024 (hilbert.wave), the three outputs
    generic_<shape>_<output>   the same calls under NXSIG_DISABLE_HILBERT_WAVE (hilbert.generic)
    generic_long_<N>_<output>  hilbert.generic on 8 rows x 60 s at 48 kHz, at N = L (2 880 000) and at the next power of two (4 194 304)
    fft_<shape>                one forward nxsig_fft of the same rows (real in, c64 out): the 4 + 8 bytes per sample of the analytic signal
    fir257_<shape>             filters.fir with 257 taps, mode "same", on the same buffer
    copy_<shape>_<output>      hipMemcpyDtoD of as many bytes as the call reads and writes (4 + 8 or 4 + 4 per sample)
Every timing is `--reps` launches between two events (40 by default: 4 - 25 ms per window for the row shapes).  The 134 MB inputs of the
row shapes fit the 256 MB last-level cache and the 134 + 134 MB of the envelope-sized copy nearly do, so the rates are what a pipeline
that keeps its rows on the chip sees, not HBM rates; the ratios between the cases of one shape are what the table is for.
Before the timing the analytic signal of every row shape is computed on both tiers at the timed size and compared: row by row against
each other, and the first 64 rows against the definition in numpy f64 (`check`); a difference above 1e-5 of a row's maximum stops the run.
    usage: python tools/bench_hilbert.py [--rounds 5] [--reps 40] [--out profiles/hilbert/bench.json]"""
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
ap.add_argument("--reps", type=int, default=40)
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
KIND = {"analytic": 0, "envelope": 1, "quadrature": 2}
TAPS = S.filters.firwin(257, [0.25])


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
    x = ctx.empty((batch, n), np.float32)
    for r0 in range(0, batch, 1024):   # filled in slabs: no second copy of the whole tensor on the host
        part = rng.standard_normal((min(1024, batch - r0), n), dtype=np.float32)
        ok(lib.nxsig_upload(h_, V(x.ptr + r0 * n * 4), part.ctypes.data_as(V), part.nbytes))
    return x


def hilbert_call(x, batch, length, n_fft, output, out):
    return lambda: lib.nxsig_hilbert_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), length, batch, length, n_fft, KIND[output], V(out.ptr), _lib.DEVICE)


def fft_call(x, batch, n, out):
    return lambda: lib.nxsig_fft(h_, V(x.ptr), 1, batch, n, n, 0, V(out.ptr), _lib.DEVICE)


def fir_call(x):
    def fn():
        S.filters.fir(x, TAPS, mode="same")
        return 0
    return fn


def copy_call(src, dst, nbytes):
    return lambda: hip.hipMemcpyDtoDAsync(V(dst.ptr), V(src.ptr), nbytes, stream)


def definition(x):
    """include/nxsig.h's definition in numpy f64"""
    n = x.shape[-1]
    h = np.zeros(n)
    h[0] = h[n // 2] = 1.0
    h[1:n // 2] = 2.0
    return np.fft.ifft(np.fft.fft(x.astype(np.float64), axis=-1) * h, axis=-1)


def row_gap(a, b):
    return float((np.abs(a - b).max(axis=-1) / np.abs(b).max(axis=-1)).max())


jobs, samples, check = [], {}, {}
for batch, n in ((16384, 2048), (32768, 1024)):
    shape = f"{batch}x{n}"
    samples[shape] = batch * n
    x, out = rows(batch, n), ctx.empty((batch, n), np.complex64)
    ok(hilbert_call(x, batch, n, n, "analytic", out)())
    ctx.sync()
    wave_rec, wave = ctx.last_dispatch(), out.numpy()
    ctx.set_tuning("DISABLE_HILBERT_WAVE", 1)
    ok(hilbert_call(x, batch, n, n, "analytic", out)())
    ctx.clear_tuning("DISABLE_HILBERT_WAVE")
    ctx.sync()
    generic = out.numpy()
    ref = definition(x.numpy()[:64])
    check[shape] = {"wave_against_generic": row_gap(wave, generic), "wave_against_definition_64_rows": row_gap(wave[:64], ref),
                    "generic_against_definition_64_rows": row_gap(generic[:64], ref), "dispatch": wave_rec}
    assert max(v for v in check[shape].values() if isinstance(v, float)) <= 1e-5 and wave_rec == "hilbert.wave", check[shape]
    del wave, generic
    src = ctx.empty((batch * n * 3,), np.float32)    # the copy's source: 12 bytes per sample, half of what it moves
    for o in KIND:
        jobs.append((f"wave_{shape}_{o}", hilbert_call(x, batch, n, n, o, out), None))
        jobs.append((f"generic_{shape}_{o}", hilbert_call(x, batch, n, n, o, out), 1))
    # a copy of b bytes reads b and writes b; the call reads 4 and writes 8 (4): the copy moves (4 + 8) / 2 bytes per sample each way
    jobs.append((f"copy_{shape}_analytic", copy_call(src, out, batch * n * 6), None))
    jobs.append((f"copy_{shape}_envelope", copy_call(src, out, batch * n * 4), None))
    jobs.append((f"fft_{shape}", fft_call(x, batch, n, out), None))
    jobs.append((f"fir257_{shape}", fir_call(x), None))
LB, LN = 8, 60 * 48000
xl = rows(LB, LN)
for n_fft in (LN, 1 << 22):
    outl = ctx.empty((LB, n_fft), np.complex64)
    samples[f"long_{n_fft}"] = LB * n_fft
    for o in ("analytic", "envelope"):
        jobs.append((f"generic_long_{n_fft}_{o}", hilbert_call(xl, LB, LN, n_fft, o, outl), None))

res, disp = {k: [] for k, _, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn, force in jobs:
        if force:
            ctx.set_tuning("DISABLE_HILBERT_WAVE", 1)
        res[k].append(timed(fn, args.reps))
        disp[k] = "hipMemcpyDtoDAsync" if k.startswith("copy_") else ctx.last_dispatch()
        if force:
            ctx.clear_tuning("DISABLE_HILBERT_WAVE")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
shapes = [s for s in samples if not s.startswith("long")]
out = {"workload": "device-resident f32 rows, standard normal samples", "rounds": args.rounds, "reps": args.reps, "device": ctx.name(),
       "samples": samples, "check": check, "ms": {k: round(v, 4) for k, v in med.items()},
       "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()}, "dispatch": disp,
       "generic_over_wave": {f"{s}_{o}": round(med[f"generic_{s}_{o}"] / med[f"wave_{s}_{o}"], 2) for s in shapes for o in KIND},
       "wave_over_fft": {f"{s}_{o}": round(med[f"wave_{s}_{o}"] / med[f"fft_{s}"], 2) for s in shapes for o in KIND},
       "wave_over_copy": {f"{s}_{o}": round(med[f"wave_{s}_{o}"] / med[f"copy_{s}_{'analytic' if o == 'analytic' else 'envelope'}"], 2)
                          for s in shapes for o in KIND},
       "wave_over_fir257": {f"{s}_{o}": round(med[f"wave_{s}_{o}"] / med[f"fir257_{s}"], 2) for s in shapes for o in KIND},
       "wave_faster_than_generic_everywhere": all(med[f"wave_{s}_{o}"] < med[f"generic_{s}_{o}"] for s in shapes for o in KIND)}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
