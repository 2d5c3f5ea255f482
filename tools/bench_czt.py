"""Transforms.zoom_fft, device-resident, beside hilbert.wave at the same L, one forward row transform, a copy and the padded transform
a caller would otherwise take.  From ONE process, interleaved rounds, warm-up before every timing, median of rounds:
    wave_<shape>       nxsig_czt on 32 768 rows x 1000 -> 25 bins (L = 1024) and 16 384 rows x 1500 -> 549 bins (L = 2048): czt.wave
    generic_<shape>    the same calls on the same buffers under NXSIG_CZT_WAVE=0 (czt.generic)
    generic_8x48000    8 rows x 1 s at 48 kHz -> 4 096 bins between 990 and 1 010 Hz (czt.generic, L = 65 536)
    hilbert_<shape>    nxsig_hilbert_f32, the analytic signal of the same rows zero-padded to L (hilbert.wave): the same two transforms of
                       L points in one wave, one table product less, and L results per row where the zoom stores m
    fft_<shape>        one forward nxsig_fft of the same rows at L points (real in, c64 out)
    copy_<shape>       hipMemcpyDtoD of as many bytes as the zoom reads and writes (4 n + 8 m per row)
    fft_padded_8x48000 one forward nxsig_fft of the 8 rows at 2^24 points: the next power of two above the 9 830 400 points whose bin spacing is the
                       zoom's 20 / 4 096 Hz (the row transforms refuse other lengths beyond 2^22), of which all but 6 991 bins would be discarded
Every timing is `--reps` launches between two events.  Before the timing every wave shape is computed on both tiers at the timed size
and compared: row by row against each other, and the first 16 rows against the definition in double (tests/czt_oracle.py); a
difference above 1e-5 of a row's maximum stops the run.  The result line goes to --out, a Markdown table of it to --table.
    usage: python tools/bench_czt.py [--rounds 5] [--reps 20] [--out profiles/czt/bench.json] [--table profiles/czt/bench_table.md]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import czt_oracle as O  # noqa: E402
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


def rows(batch, n):
    x = ctx.empty((batch, n), np.float32)
    for r0 in range(0, batch, 1024):   # filled in slabs: no second copy of the whole tensor on the host
        part = rng.standard_normal((min(1024, batch - r0), n), dtype=np.float32)
        ok(lib.nxsig_upload(h_, V(x.ptr + r0 * n * 4), part.ctypes.data_as(V), part.nbytes))
    return x


def czt_call(x, batch, n, m, contour, out):
    return lambda: lib.nxsig_czt(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), 0, n, batch, n, m, *contour, V(out.ptr), _lib.DEVICE)


def hilbert_call(x, batch, n, n_fft, out):
    return lambda: lib.nxsig_hilbert_f32(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), n, batch, n, n_fft, 0, V(out.ptr), _lib.DEVICE)


def fft_call(x, batch, n, n_fft, out):
    return lambda: lib.nxsig_fft(h_, V(x.ptr), 1, batch, n, n_fft, 0, V(out.ptr), _lib.DEVICE)


def copy_call(src, dst, nbytes):
    return lambda: hip.hipMemcpyDtoDAsync(V(dst.ptr), V(src.ptr), nbytes, stream)


def row_gap(a, b):
    return float((np.abs(a - b).max(axis=-1) / np.abs(b).max(axis=-1)).max())


jobs, check, shapes, moved = [], {}, [], {}
for batch, n, m, fn_, fs in ((32768, 1000, 25, [990.0, 1010.0], 8000.0), (16384, 1500, 549, [100.0, 300.0], 2000.0)):
    shape = f"{batch}x{n}_m{m}"
    shapes.append(shape)
    L = lib.nxsig_czt_conv_length(n, m)
    contour = O.contour_zoom(fn_, m, fs)
    x, out, big = rows(batch, n), ctx.empty((batch, m), np.complex64), ctx.empty((batch, L), np.complex64)
    ok(czt_call(x, batch, n, m, contour, out)())
    ctx.sync()
    wave_rec, wave = ctx.last_dispatch(), out.numpy()
    ctx.set_tuning("CZT_WAVE", 0)
    ok(czt_call(x, batch, n, m, contour, out)())
    ctx.clear_tuning("CZT_WAVE")
    ctx.sync()
    generic_rec, generic = ctx.last_dispatch(), out.numpy()
    ref = O.czt(x.numpy()[:16], m, contour)
    check[shape] = {"wave_against_generic": row_gap(wave, generic), "wave_against_definition_16_rows": row_gap(wave[:16], ref),
                    "generic_against_definition_16_rows": row_gap(generic[:16], ref), "dispatch": wave_rec, "generic_dispatch": generic_rec, "L": L}
    assert max(v for v in check[shape].values() if isinstance(v, float)) <= 1e-5 and wave_rec == "czt.wave", check[shape]
    del wave, generic
    moved[shape] = batch * (4 * n + 8 * m)
    src = ctx.empty((moved[shape] // 8 + 1,), np.float32)
    jobs.append((f"wave_{shape}", czt_call(x, batch, n, m, contour, out), None))
    jobs.append((f"generic_{shape}", czt_call(x, batch, n, m, contour, out), 0))
    jobs.append((f"hilbert_{shape}", hilbert_call(x, batch, n, L, big), None))
    jobs.append((f"fft_{shape}", fft_call(x, batch, n, L, big), None))
    jobs.append((f"copy_{shape}", copy_call(src, big, moved[shape] // 2), None))
LB, LN, LM, PAD = 8, 48000, 4096, 1 << 24   # 48 000 * 4 096 / 20 = 9 830 400 points give the zoom's spacing; the row transforms take powers of two beyond 2^22
long_contour = O.contour_zoom([990.0, 1010.0], LM, 48000.0)
xl, outl = rows(LB, LN), ctx.empty((LB, LM), np.complex64)
ok(czt_call(xl, LB, LN, LM, long_contour, outl)())
ctx.sync()
check["8x48000_m4096"] = {"generic_against_definition_2_rows": row_gap(outl.numpy()[:2], O.czt(xl.numpy()[:2], LM, long_contour)), "dispatch": ctx.last_dispatch(),
                          "L": lib.nxsig_czt_conv_length(LN, LM)}
assert check["8x48000_m4096"]["generic_against_definition_2_rows"] <= 1e-5, check
jobs.append(("generic_8x48000_m4096", czt_call(xl, LB, LN, LM, long_contour, outl), None))
padded_error = None
try:
    outp = ctx.empty((LB, PAD), np.complex64)
    ok(fft_call(xl, LB, LN, PAD, outp)())
    ctx.sync()
    jobs.append(("fft_padded_8x48000", fft_call(xl, LB, LN, PAD, outp), None))
except (RuntimeError, MemoryError) as e:   # what the row transforms refuse is reported, not timed
    padded_error = str(e)

res, disp = {k: [] for k, _, _ in jobs}, {}
for _ in range(args.rounds):
    for k, fn, force in jobs:
        if force is not None:
            ctx.set_tuning("CZT_WAVE", force)
        res[k].append(timed(fn, 2 if k.startswith("fft_padded") else args.reps))
        disp[k] = "hipMemcpyDtoDAsync" if k.startswith("copy_") else ctx.last_dispatch()
        if force is not None:
            ctx.clear_tuning("CZT_WAVE")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
out = {"workload": "device-resident f32 rows, standard normal samples, zoom_fft", "rounds": args.rounds, "reps": args.reps, "device": ctx.name(),
       "bytes_moved": moved, "check": check, "ms": {k: round(v, 4) for k, v in med.items()},
       "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()}, "dispatch": disp,
       "generic_over_wave": {s: round(med[f"generic_{s}"] / med[f"wave_{s}"], 2) for s in shapes},
       "wave_over_hilbert_wave": {s: round(med[f"wave_{s}"] / med[f"hilbert_{s}"], 2) for s in shapes},
       "wave_over_fft": {s: round(med[f"wave_{s}"] / med[f"fft_{s}"], 2) for s in shapes},
       "wave_over_copy": {s: round(med[f"wave_{s}"] / med[f"copy_{s}"], 2) for s in shapes},
       "padded_fft_over_zoom_8x48000": round(med["fft_padded_8x48000"] / med["generic_8x48000_m4096"], 1) if "fft_padded_8x48000" in med else None,
       "padded_fft_error": padded_error,
       "wave_faster_than_generic_everywhere": all(med[f"wave_{s}"] < med[f"generic_{s}"] for s in shapes)}
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
