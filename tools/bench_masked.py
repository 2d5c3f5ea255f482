"""Time-frequency masks on config-3 geometry (N=1024 hop=256, 16 x 60 s, device-resident): nxsig_istft_masked_c64 for the three mask
kinds (one launch, 14 / 12 / 18 KB of HBM traffic per frame) against the two-step form (spectrum_mask + istft, 30 KB per frame), the
source-separation case (one spectrum row, 16 masks), and beside them the yardsticks: plain istft and the chain spectrum_multiply ->
istft.  The yardsticks run from a SECOND build of libnxsig.so when one is given (the parent commit's, loaded side by side like
tools/ab_libs.py), so that the code under test is never its own yardstick.  Interleaved rounds in one process, warm-up before every
timing, median of rounds; bit-identity of the fused against the two-step output at the timed size is part of the JSON line.
    usage: python tools/bench_masked.py [--base tools/_ab/libnxsig_base.so] [--rounds 5] [--out profiles/masked/bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nx_signal_amd import _lib  # noqa: E402  (signature table + structs only)

ap = argparse.ArgumentParser()
ap.add_argument("--base", default=None, help="another build of libnxsig.so for the yardstick rows (default: this build)")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

N = int(os.environ.get("SWEEP_N", 1024))
hop, L, B = N // int(os.environ.get("SWEEP_R", 4)), int(os.environ.get("SWEEP_L", 2880000)), int(os.environ.get("SWEEP_B", 16))
M = (L - N) // hop + 1
out_len = M * hop + N - hop
V = C.c_void_p
REAL, ONESIDED, COMPLEX = 0, 1, 2


def bind(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, argt) in _lib.SIGNATURES.items():
        try:
            f = getattr(lib, name)
        except AttributeError:
            continue  # an older build without this symbol
        f.restype, f.argtypes = res, argt
    return lib


class Side:
    def __init__(self, path):
        self.lib = bind(path)
        self.ctx = V()
        self.ok(self.lib.nxsig_ctx_create(0, C.byref(self.ctx)))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.nxsig_last_error().decode())

    def alloc(self, nbytes):
        p = V()
        self.ok(self.lib.nxsig_alloc(self.ctx, nbytes, C.byref(p)))
        return p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self.ok(self.lib.nxsig_upload(self.ctx, p, arr.ctypes.data_as(V), arr.nbytes))
        return p

    def download(self, p, shape, dtype):
        out = np.empty(shape, dtype)
        self.ok(self.lib.nxsig_download(self.ctx, out.ctypes.data_as(V), p, out.nbytes))
        return out

    def time(self, fn, reps, warm=5):
        for _ in range(warm):
            self.ok(fn())
        self.ok(self.lib.nxsig_sync(self.ctx))
        self.ok(self.lib.nxsig_timer_start(self.ctx))
        for _ in range(reps):
            fn()
        ms = C.c_float()
        self.ok(self.lib.nxsig_timer_stop(self.ctx, C.byref(ms)))
        return ms.value / reps


new = Side(os.path.join(ROOT, "nx_signal_amd", "libnxsig.so"))
base = Side(args.base) if args.base else new
w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32)
wp = w.ctypes.data_as(V)
p = _lib.StftParams(N, hop, N, 0, 0, 0, 0, 0, 48000.0)
rng = np.random.Generator(np.random.PCG64(1))
x = rng.standard_normal((B, L), dtype=np.float32)


def spectrum(side):
    xd = side.upload(x)
    z = side.alloc(B * M * N * 8)
    side.ok(side.lib.nxsig_stft_f32(side.ctx, xd, L, B, L, wp, C.byref(p), z, None, 1))
    side.ok(side.lib.nxsig_sync(side.ctx))
    side.ok(side.lib.nxsig_free(side.ctx, xd))
    return z


# ---- the code under test
z = spectrum(new)
m_real = new.upload(rng.random((B, M, N), dtype=np.float32))
m_half = new.upload(rng.random((B, M, N // 2 + 1), dtype=np.float32))
m_cplx = new.upload((rng.random((B, M, N), dtype=np.float32) + 1j * rng.random((B, M, N), dtype=np.float32)).astype(np.complex64))
zm = new.alloc(B * M * N * 8)
y_fused, y_two = new.alloc(B * out_len * 8), new.alloc(B * out_len * 8)
lib, ctx = new.lib, new.ctx


def fused(mask, kind, z_rows=B):
    return lambda: lib.nxsig_istft_masked_c64(ctx, z, z_rows, M, wp, C.byref(p), mask, kind, B, y_fused, 1)


def two_step():
    rc = lib.nxsig_spectrum_mask_c64(ctx, z, B, m_real, REAL, B, M, N, zm, 1)
    return rc or lib.nxsig_istft_c64(ctx, zm, M, B, wp, C.byref(p), y_two, 1)


# ---- the yardsticks (the parent build when --base is given)
zb = spectrum(base) if base is not new else z
zfb = base.alloc(B * M * N * 8)
yb = base.alloc(B * out_len * 8)
h = np.ascontiguousarray(np.fft.fft(np.hanning(129) / np.hanning(129).sum(), N).astype(np.complex64))
hp = h.ctypes.data_as(V)
blib, bctx = base.lib, base.ctx


def base_istft():
    return blib.nxsig_istft_c64(bctx, zb, M, B, wp, C.byref(p), yb, 1)


def base_chain():
    rc = blib.nxsig_spectrum_mul_c64(bctx, zb, B * M, N, hp, zfb, 1)
    return rc or blib.nxsig_istft_c64(bctx, zfb, M, B, wp, C.byref(p), yb, 1)


jobs = [
    ("fused_real", new, fused(m_real, REAL)), ("fused_onesided", new, fused(m_half, ONESIDED)), ("fused_complex", new, fused(m_cplx, COMPLEX)),
    ("two_step_real", new, two_step), ("fused_real_1x16", new, fused(m_real, REAL, 1)),
    ("base_istft", base, base_istft), ("base_multiply_then_istft", base, base_chain),
]
res = {k: [] for k, _, _ in jobs}
for rnd in range(args.rounds):
    for k, side, fn in jobs:
        res[k].append(side.time(fn, args.reps))
# bit identity at the timed size (real mask): one more call of each form, then compare
new.ok(fused(m_real, REAL)())
new.ok(two_step())
new.ok(lib.nxsig_sync(ctx))
same = bool(np.array_equal(new.download(y_fused, (B * out_len * 2,), np.uint32), new.download(y_two, (B * out_len * 2,), np.uint32)))
buf = C.create_string_buffer(256)
new.ok(fused(m_real, REAL)())
lib.nxsig_ctx_last_dispatch(ctx, buf, 256)

out = {"workload": f"N={N} hop={hop} {B} x {L} samples, M={M}", "yardstick_lib": args.base or "this build", "rounds": args.rounds,
       "dispatch": buf.value.decode()}
med = {}
for k, v in res.items():
    v = sorted(v)
    med[k] = v[len(v) // 2]
    out[k + "_ms"] = round(med[k], 4)
# algorithmic bytes per frame: spectrum + mask + result (hop c64 samples)
per_frame = {"fused_real": N * 8 + N * 4 + hop * 8, "fused_onesided": N * 8 + (N // 2 + 1) * 4 + hop * 8, "fused_complex": N * 16 + hop * 8,
             "fused_real_1x16": N * 4 + hop * 8 + N * 8 // B}
for k, b in per_frame.items():
    out[k + "_Mframes_per_s"] = round(B * M / (med[k] * 1e-3) / 1e6, 1)
    out[k + "_algorithmic_GBps"] = round(B * M * b / (med[k] * 1e-3) / 1e9, 1)
    out[k + "_frac_of_8TBps"] = round(B * M * b / (med[k] * 1e-3) / 8e12, 4)
out["fused_real_over_base_istft"] = round(med["fused_real"] / med["base_istft"], 3)
out["fused_real_over_two_step"] = round(med["fused_real"] / med["two_step_real"], 3)
out["fused_real_over_base_multiply_then_istft"] = round(med["fused_real"] / med["base_multiply_then_istft"], 3)
out["fused_real_faster_than_base_chain"] = bool(med["fused_real"] < med["base_multiply_then_istft"])
out["bit_identical_to_two_step"] = same
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
