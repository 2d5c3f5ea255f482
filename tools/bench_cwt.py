"""Transforms.cwt, device-resident, beside its yardsticks.  From ONE process, interleaved rounds, warm-up before every timing, median of
rounds.  Shapes: 32 rows x 2^20 samples with 16 morlet2 widths spaced geometrically from 2 to 51.2 (every filter in the K = 1024 class),
the same rows with widths up to 102.4 (adds the K = 2048 class), and 8 rows with widths up to 1000 (adds the generic class).
    wave_<shape>_<kind>     nxsig_cwt as it dispatches by default, kinds complex and power
    generic_<shape>_<kind>  (c) the same call on the same buffers under NXSIG_CWT_WAVE=0 (cwt.generic)
    copy_<shape>_<kind>     (a) hipMemcpyDtoD of the output's byte count
    fir_<shape>             (b) what a caller did before: 2 S filters.fir calls on the same buffer, the real and the imaginary taps of
                            every scale (the combination into a complex tensor or a power is NOT included)
Every timing is `--reps` launches between two events.  Before the timing every shape is computed at the timed size and its first two
rows (their first 2^14 samples, on both tiers) compared against the definition in double (tests/cwt_oracle.py); a difference above 1e-5 of a (row, scale) maximum stops the run.
The result line goes to --out, a Markdown table of it to --table, the accuracy lines to --accuracy.
    usage: python tools/bench_cwt.py [--rounds 5] [--reps 5] [--out profiles/cwt/bench.json] [--table profiles/cwt/bench_table.md]
                                     [--accuracy profiles/cwt/accuracy.txt] [--rows 32] [--log2n 20]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cwt_oracle as O  # noqa: E402
import nx_signal_amd as S  # noqa: E402
from nx_signal_amd import _lib, filters  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rows", type=int, default=32)
ap.add_argument("--log2n", type=int, default=20)
ap.add_argument("--out", default=None)
ap.add_argument("--table", default=None)
ap.add_argument("--accuracy", default=None)
args = ap.parse_args()

V = C.c_void_p
lib = _lib.load()
ctx = S.Context(0)
h_ = ctx.handle
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyDtoDAsync.restype, hip.hipMemcpyDtoDAsync.argtypes = C.c_int, [V, V, C.c_size_t, V]
stream = V(lib.nxsig_get_stream(h_))
rng = np.random.Generator(np.random.PCG64(5))
KINDS = {"complex": 0, "power": 3}
N = 1 << args.log2n


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
    for r0 in range(batch):
        part = rng.standard_normal(n, dtype=np.float32)
        ok(lib.nxsig_upload(h_, V(x.ptr + r0 * n * 4), part.ctypes.data_as(V), part.nbytes))
    return x


def cwt_call(x, batch, n, ws, kind, out):
    return lambda: lib.nxsig_cwt(_lib.ctx_ptr(h_, _lib._ctx_iir), V(x.ptr), n, batch, n, 0, ws.ctypes.data_as(C.POINTER(C.c_double)), len(ws), 5.0,
                                 KINDS[kind], V(out.ptr), _lib.DEVICE)


def fir_calls(x, taps):
    def run():
        for t in taps:
            filters.fir(x, t, mode="same", ctx=ctx)
        return 0
    return run


def copy_call(src, dst, nbytes):
    return lambda: hip.hipMemcpyDtoDAsync(V(dst.ptr), V(src.ptr), nbytes, stream)


def geometric(lo, hi, count=16):
    return np.ascontiguousarray(lo * (hi / lo) ** (np.arange(count) / (count - 1.0)))


SHAPES = [("k1024", args.rows, geometric(2.0, 51.2)), ("k2048", args.rows, geometric(2.0, 102.4)), ("generic", max(args.rows // 4, 1), geometric(2.0, 1000.0))]
x_all = rows(args.rows, N)
jobs, check, accuracy = [], {}, []
for shape, batch, ws in SHAPES:
    S_ = len(ws)
    outs = {"complex": ctx.empty((batch, S_, N), np.complex64), "power": ctx.empty((batch, S_, N), np.float32)}
    head = np.ascontiguousarray(x_all.numpy()[:2, :1 << min(args.log2n, 14)])
    hd = ctx.to_device(head)
    ref_c = O.cwt(head, ws, "morlet2", 5.0, kind="complex")
    for kind in KINDS:
        # the timed call once, for its dispatch record; the comparison with the definition on two rows of 2^14 samples (the oracle is O(L N))
        ok(cwt_call(x_all, batch, N, ws, kind, outs[kind])())
        ctx.sync()
        rec = ctx.last_dispatch()
        small = ctx.empty((2, S_, head.shape[1]), np.complex64 if kind == "complex" else np.float32)
        gaps = {}
        for label, force in (("default", None), ("generic", 0)):
            if force is not None:
                ctx.set_tuning("CWT_WAVE", force)
            ok(cwt_call(hd, 2, head.shape[1], ws, kind, small)())
            ctx.sync()
            if force is not None:
                ctx.clear_tuning("CWT_WAVE")
            ref = O.sink(ref_c, kind)
            got = small.numpy()
            gaps[label] = float((np.abs(got - ref).max(axis=-1) / np.abs(ref).max(axis=-1)).max())
            accuracy.append(f"cwt-accuracy bench {shape} {kind} {label} rows=2 L={head.shape[1]} S={S_}: {gaps[label]:.3e}")
        check[f"{shape}_{kind}"] = {"dispatch": rec, "against_definition": gaps, "supports": [int(lib.nxsig_cwt_support(a, N)) for a in ws]}
        assert max(gaps.values()) <= 1e-5, check
        nbytes = batch * S_ * N * (8 if kind == "complex" else 4)
        src = ctx.empty((nbytes // 4,), np.float32)
        jobs.append((f"wave_{shape}_{kind}", cwt_call(x_all, batch, N, ws, kind, outs[kind]), None, args.reps))
        jobs.append((f"generic_{shape}_{kind}", cwt_call(x_all, batch, N, ws, kind, outs[kind]), 0, max(args.reps // 2, 1)))
        jobs.append((f"copy_{shape}_{kind}", copy_call(src, outs[kind], nbytes), None, args.reps))
    taps = []
    for a in ws:
        h = O.taps("morlet2", a, N)
        taps += [np.ascontiguousarray(h.real.astype(np.float32)), np.ascontiguousarray(h.imag.astype(np.float32))]
    xb = x_all if batch == args.rows else ctx.to_device(x_all.numpy()[:batch])
    jobs.append((f"fir_{shape}", fir_calls(xb, taps), None, 1))

res, disp = {k: [] for k, *_ in jobs}, {}
for _ in range(args.rounds):
    for k, fn, force, reps in jobs:
        if force is not None:
            ctx.set_tuning("CWT_WAVE", force)
        res[k].append(timed(fn, reps))
        disp[k] = "hipMemcpyDtoDAsync" if k.startswith("copy_") else ctx.last_dispatch()
        if force is not None:
            ctx.clear_tuning("CWT_WAVE")
med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
keys = [f"{s}_{k}" for s, _, _ in SHAPES for k in KINDS]
out = {"workload": f"device-resident f32 rows of 2^{args.log2n} standard normal samples, 16 morlet2 widths", "rounds": args.rounds, "reps": args.reps,
       "device": ctx.name(), "rows": {s: b for s, b, _ in SHAPES}, "widths": {s: [round(float(a), 3) for a in w] for s, _, w in SHAPES}, "check": check,
       "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in res.items()}, "dispatch": disp,
       "default_over_copy": {k: round(med[f"wave_{k}"] / med[f"copy_{k}"], 2) for k in keys},
       "default_over_2S_fir_calls": {k: round(med[f"wave_{k}"] / med[f"fir_{k.rsplit('_', 1)[0]}"], 3) for k in keys},
       "default_over_generic": {k: round(med[f"wave_{k}"] / med[f"generic_{k}"], 3) for k in keys}}
line = json.dumps(out)
print(line)
table = ["| case | ms (median) | min .. max | dispatch |", "|---|---|---|---|"]
table += [f"| `{k}` | {med[k]:.4f} | {min(res[k]):.4f} .. {max(res[k]):.4f} | {disp[k]} |" for k, *_ in jobs]
print("\n".join(table))
for path, text in ((args.out, line), (args.table, "\n".join(table)), (args.accuracy, "\n".join(accuracy))):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
