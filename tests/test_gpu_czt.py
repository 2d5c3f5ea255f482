"""Transforms.czt / zoom_fft on the GPU against the f64 oracle of tests/czt_oracle.py (the definition of include/nxsig.h as a direct sum
with exactly reduced phases) run on the SAME samples.  The error of a row is max |got - ref| / max |ref| over the row, bound 1e-5: the
project's bar for a single-precision transform (a numpy single-precision restatement of the scheme reads 1.6e-7 to 2.4e-7 on these
shapes, tests/test_czt_host.py).

Every run asserts its dispatch record: "czt.wave" alone for the fused tier, "czt.generic" followed by the row transforms' families for
the other.  The fused shapes run again under NXSIG_CZT_WAVE=0; equal bits between the tiers are not required.

Non-finite rule under test: a row that holds an Inf / NaN among its n samples has no finite output element; every other row of the
batch keeps its bits.

Nothing here loads the library while pytest collects: the sizes come from csrc/czt_plan.hpp's rule restated below (n + m - 1 <= 2048:
the wave tier at L = 1024 or 2048), and the reference of a (shape, contour) is formed once and shared."""
import cmath
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import czt_oracle as O
import extents as E
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, transforms

pytestmark = pytest.mark.gpu

TOL = 1e-5
WAVE, GENERIC = "czt.wave", "czt.generic"
# the recorded shapes of tests/golden/czt_vectors.json, plus a short zoom, one output point, and one four-step row
SHAPES = [(1, 1), (3, 7), (600, 300), (512, 513), (513, 513), (1024, 1025), (1500, 549), (1025, 1025), (5000, 37), (100, 5000),
          (1000, 25), (2048, 1), (40000, 64)]
W_UNIT, A_UNIT = cmath.exp(-0.37j), cmath.exp(0.2j)
FN, FS = [0.1, 0.3], 2.0
W_SPIRAL, A_SPIRAL = 1.0005 * cmath.exp(-0.11j), 0.999 * cmath.exp(0.3j)     # the recorded spiral, n = m = 64


def fused(n, m):
    return n + m - 1 <= 2048


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Tier:
    """NXSIG_CZT_WAVE=0 on one context for a block"""

    def __init__(self, ctx, generic):
        self.ctx, self.on = ctx, generic

    def __enter__(self):
        if self.on:
            self.ctx.set_tuning("CZT_WAVE", 0)

    def __exit__(self, *exc):
        if self.on:
            self.ctx.clear_tuning("CZT_WAVE")


class RowsPerWave:
    """NXSIG_WAVE_UNITS_PER_WAVE on one context for a block: the rows a wave of czt.wave walks (None: the launcher's heuristic, which
    gives every batch this suite can afford ONE row per wave, so the loop's second trip — the prefetched row, the reused LDS buffer —
    would never run)"""

    def __init__(self, ctx, rows):
        self.ctx, self.rows = ctx, rows

    def __enter__(self):
        if self.rows:
            self.ctx.set_tuning("WAVE_UNITS_PER_WAVE", self.rows)

    def __exit__(self, *exc):
        if self.rows:
            self.ctx.clear_tuning("WAVE_UNITS_PER_WAVE")


def noise(seed, shape, complex_rows=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal(shape).astype(np.float32)
    return (x + 1j * rng.standard_normal(shape).astype(np.float32)).astype(np.complex64) if complex_rows else x


def rows_for(seed, shape, m, kind, complex_rows=False):
    """standard normal rows.  With ONE output point the row maximum is that point alone, a sum of n samples that cancels to anything
    between 0 and 3 sqrt(n): no single-precision sum is within 1e-5 of a value it cancelled to (an f32 sum of 2048 samples is off by
    1e-5 absolute; one row in forty sums to less than 1).  So the rows of an m = 1 shape carry a tone at the point the transform
    evaluates, of the amplitude that puts 3 sqrt(n) there — the size the row maximum has at every other shape"""
    x = noise(seed, shape, complex_rows)
    n = shape[-1]
    if m == 1 and n > 1:
        tone = np.exp(2j * np.pi * CALLS[kind][1](m)[4] * np.arange(n))
        x = (x + 3 / np.sqrt(n) * tone).astype(np.complex64) if complex_rows else (x + 6 / np.sqrt(n) * tone.real).astype(np.float32)
    return x


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def family(rec, n, m, generic):
    """the record names the tier first; the generic tier's row transforms follow"""
    wave = fused(n, m) and not generic
    assert (rec == WAVE) if wave else (rec.split("+")[0] == GENERIC and WAVE not in rec), (rec, n, m, generic)
    return rec


# a call as the Python functions take it, and the contour the oracle evaluates for it
CALLS = {
    "czt": (lambda x, m, c: transforms.czt(x, m, ctx=c), lambda m: O.contour_czt(m)),
    "czt_wa": (lambda x, m, c: transforms.czt(x, m, W_UNIT, A_UNIT, ctx=c), lambda m: O.contour_czt(m, W_UNIT, A_UNIT)),
    "zoom": (lambda x, m, c: transforms.zoom_fft(x, FN, m, fs=FS, ctx=c), lambda m: O.contour_zoom(FN, m, FS)),
    "zoom_endpoint": (lambda x, m, c: transforms.zoom_fft(x, FN, m, fs=FS, endpoint=True, ctx=c), lambda m: O.contour_zoom(FN, m, FS, True)),
    "spiral": (lambda x, m, c: transforms.czt(x, m, W_SPIRAL, A_SPIRAL, ctx=c), lambda m: O.contour_czt(m, W_SPIRAL, A_SPIRAL)),
}
_KERNELS = {}


def reference(x, m, kind):
    """the definition on the rows x, complex128; the kernel matrix of an (n, m, contour) is formed once"""
    key = (x.shape[-1], m, kind)
    if key not in _KERNELS:
        _KERNELS[key] = O.kernel(x.shape[-1], m, CALLS[kind][1](m))
    return x.astype(np.complex128) @ _KERNELS[key]


def dev(ctx, x, m, kind, generic=False):
    """one call on a device tensor: (numpy result, dispatch record)"""
    with Tier(ctx, generic):
        out = CALLS[kind][0](ctx.to_device(x), m, ctx)
        ctx.sync()
        rec = ctx.last_dispatch()
    assert isinstance(out, S.DeviceBuffer)
    return out.numpy(), family(rec, x.shape[-1], m, generic)


def row_errors(got, ref):
    """per row: the error over the reference's magnitude; rows whose reference is not finite must hold no finite element"""
    assert got.shape == ref.shape and got.dtype == np.complex64
    errs = []
    for r in range(ref.shape[0]):
        if not np.isfinite(ref[r]).all():
            assert not (np.isfinite(got[r].real) | np.isfinite(got[r].imag)).any(), f"row {r} holds a finite element"
            continue
        assert np.isfinite(got[r]).all(), f"row {r} holds a non-finite element"
        errs.append(float(np.abs(got[r].astype(np.complex128) - ref[r]).max() / np.abs(ref[r]).max()))
    return errs


def check(name, got, ref):
    errs = row_errors(got, ref)
    worst = max(errs) if errs else 0.0
    assert worst <= TOL, (name, worst)
    return worst


# every shape as it dispatches by default, and the fused ones again with the wave tier switched off
PARITY = [(s, False) for s in SHAPES] + [(s, True) for s in SHAPES if fused(*s)]


@pytest.mark.parametrize("shape,generic", PARITY, ids=[f"n{s[0]}-m{s[1]}-{'switched-off' if g else 'default'}" for s, g in PARITY])
def test_parity_with_the_definition_on_both_tiers(ctx, shape, generic):
    """every recorded shape, (1000, 25), (2048, 1) and the four-step row (40000, 64): real rows through zoom_fft and czt's default, c64
    rows through czt with a general w and a, at batch 1, 5 and 65 (the same rows: a row's bits do not depend on the batch)"""
    n, m = shape
    tier = "generic" if generic or not fused(n, m) else "wave"
    for kind, complex_rows in (("zoom", False), ("czt_wa", True), ("czt", False)):
        x = rows_for(1000 + 7 * n + m, (65, n), m, kind, complex_rows)
        ref = reference(x, m, kind)
        whole = None
        for batch in (65, 5, 1):
            got, rec = dev(ctx, x[:batch], m, kind, generic)
            worst = check(f"{kind} n={n} m={m} batch={batch}", got, ref[:batch])
            print(f"czt-accuracy {tier} {kind} {'c64' if complex_rows else 'f32'} n={n} m={m} batch={batch}: {worst:.3e} [{rec}]")
            if whole is None:
                whole = got
            assert same_bits(got, whole[:batch]), (kind, n, m, batch)
    if shape == (40000, 64):
        assert "fft.tiled" in rec.split("+"), rec     # the two-pass tiled four-step of the row transforms


def test_one_point_and_endpoint_contours(ctx):
    for n, m, kind in [(2048, 1, "czt_wa"), (1, 2048, "zoom_endpoint"), (600, 300, "zoom_endpoint"), (5000, 37, "zoom_endpoint")]:
        x = rows_for(11 + n, (3, n), m, kind)
        for generic in (False, True):
            check(f"{kind} n={n} m={m}", dev(ctx, x, m, kind, generic)[0], reference(x, m, kind))


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
def test_one_output_point_of_plain_noise(ctx, generic):
    """the m = 1 shapes on rows WITHOUT the tone of rows_for: the one output is a sum that may cancel, so the row maximum is no scale
    for it; the error is held to 1e-5 of sqrt(n) max|x| of the row instead, the size a sum of n such samples has when it does not
    cancel (and within a factor 1.2 of the 3 sqrt(n) the row maximum has at the other shapes: max|x| of 2048 normal samples is 3.5)"""
    n, m = 2048, 1
    for kind, complex_rows in (("zoom", False), ("czt_wa", True), ("czt", False)):
        x = noise(1300 + len(kind), (65, n), complex_rows)
        got, _ = dev(ctx, x, m, kind, generic)
        ref = reference(x, m, kind)
        err = np.abs(got.astype(np.complex128) - ref).max(axis=-1) / (np.sqrt(n) * np.abs(x).max(axis=-1))
        print(f"czt-accuracy {'generic' if generic else 'wave'} {kind} plain noise n={n} m={m} batch=65: {err.max():.3e} of sqrt(n) max|x|, "
              f"{(np.abs(got - ref).max(axis=-1) / np.abs(ref).max(axis=-1)).max():.3e} of the row's one value")
        assert err.max() <= TOL, (kind, generic, float(err.max()))


@pytest.mark.parametrize("rows_per_wave", [2, 4])
@pytest.mark.parametrize("shape", [(600, 300), (1500, 549)], ids=lambda s: f"n{s[0]}-m{s[1]}")
def test_several_rows_per_wave_give_the_bits_of_one_row_per_wave(ctx, shape, rows_per_wave):
    """batch 65 at L = 1024 and 2048 with a wave walking 2 and 4 rows (the last workgroup ragged): in bound and the same uint32 words as
    the default geometry; then NaN and +Inf rows — one in the middle of a wave's walk with clean rows behind it on the same wave, one
    that a wave takes last, and the batch's last row — which take their own rows and leave every other row's bits alone"""
    n, m = shape
    bad_rows = [1, 10, 61, 64]
    keep = [r for r in range(65) if r not in bad_rows]
    for kind, complex_rows in (("zoom", False), ("czt_wa", True)):
        x = noise(2000 + n, (65, n), complex_rows)
        ref = reference(x, m, kind)
        base, _ = dev(ctx, x, m, kind)
        check(f"default geometry n={n} m={m}", base, ref)
        with RowsPerWave(ctx, rows_per_wave):
            got, rec = dev(ctx, x, m, kind)
        assert rec == WAVE and same_bits(got, base), (shape, kind, rows_per_wave)
        for bad in (np.nan, np.inf):
            xb = x.copy()
            for i, r in enumerate(bad_rows):
                xb[r, (n // 5) * (i + 1)] = bad
            with RowsPerWave(ctx, rows_per_wave):
                got, _ = dev(ctx, xb, m, kind)
            finite = np.isfinite(got.real) | np.isfinite(got.imag)
            assert not finite[bad_rows].any() and np.isfinite(got[keep]).all(), (shape, kind, rows_per_wave, bad)
            assert same_bits(got[keep], base[keep]), (shape, kind, rows_per_wave, bad)


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_sample_takes_its_row_and_no_other(ctx, bad, generic):
    for n, m in [(600, 300), (1500, 549), (3, 7)] + ([(5000, 37), (100, 5000)] if generic else []):
        for kind, complex_rows in (("zoom", False), ("czt_wa", True)):
            clean = noise(61 + n, (4, n), complex_rows)
            x = clean.copy()
            x[1, n // 3] = bad
            y, _ = dev(ctx, x, m, kind, generic)
            finite = np.isfinite(y.real) | np.isfinite(y.imag)
            assert not finite[1].any() and np.isfinite(y[[0, 2, 3]]).all(), (n, m, kind)
            assert same_bits(y[[0, 2, 3]], dev(ctx, clean, m, kind, generic)[0][[0, 2, 3]])


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
@pytest.mark.parametrize("complex_rows", [False, True], ids=["f32", "c64"])
def test_strided_rows_inside_poisoned_arenas(ctx, generic, complex_rows):
    """batch 3 with batch_stride = n + 5 through the C entry point, odd n and odd m, rows and results off their 8- / 16-byte boundaries,
    inside poisoned arenas: the guards and gaps untouched, every result element written, the input unchanged, the results in bound"""
    lib = _lib.load()
    fn = lambda h, *a: lib.nxsig_czt(_lib.ctx_ptr(h, _lib._ctx_iir), *a)   # noqa: E731
    idt = np.complex64 if complex_rows else np.float32
    kind = "czt_wa" if complex_rows else "zoom"
    for n, m in [(601, 301), (600, 300), (1501, 547), (3, 7)] + ([(5001, 37)] if generic else []):
        contour = CALLS[kind][1](m)
        x = noise(3 * n + m, (3, n), complex_rows)
        ref = reference(x, m, kind).astype(np.complex64)
        with Tier(ctx, generic):
            for gap, offset in ((5, 1), (5, 2), (5, 3), (0, 0)):
                xin = E.Arena("x", idt, 3, n, n + gap, offset_elems=offset, data=x).upload(ctx)
                out = E.Arena("out", np.complex64, 3, m, offset_elems=(offset + 1) % 4).upload(ctx)
                rec = E.call(ctx, fn, xin.ptr, int(complex_rows), n, 3, n + gap, m, *contour, out.ptr, _lib.DEVICE)
                family(rec, n, m, generic)
                E.verify([(xin, xin.download())], out, out.download(), expected=ref, tol=TOL)
                check(f"strided n={n} m={m} gap={gap}", out.tensor(out.download()), reference(x, m, kind))
            # host memory: the staged copy keeps the row stride
            xin = E.Arena("x", idt, 3, n, n + 5, offset_elems=1, data=x)
            out = E.Arena("out", np.complex64, 3, m)
            ximg, oimg = xin.image.copy(), out.image.copy()
            E.call(ctx, fn, C.c_void_p(ximg.ctypes.data + xin.offset_bytes), int(complex_rows), n, 3, n + 5, m, *contour,
                   C.c_void_p(oimg.ctypes.data + out.offset_bytes), _lib.HOST)
            E.verify([(xin, ximg)], out, oimg, expected=ref, tol=TOL)


def test_a_sequence_of_calls_on_one_context_then_the_first_again():
    """a seeded sequence of calls with different (n, m, w, a) on one context, both tiers and both row types, then the first call again:
    the same bits.  Host and device tensors give the same bits"""
    c = S.Context(0)
    rng = np.random.Generator(np.random.PCG64(5))
    x0 = noise(401, (5, 700))
    first, _ = dev(c, x0, 300, "zoom")
    first_generic, _ = dev(c, x0, 300, "zoom", True)
    for step in range(8):
        n, m = int(rng.integers(1, 2000)), int(rng.integers(1, 1000))
        w, a = cmath.exp(-1j * rng.uniform(0.001, 1.0)), cmath.exp(1j * rng.uniform(-3.0, 3.0))
        x = noise(500 + step, (int(rng.integers(1, 9)), n), bool(step % 2))
        with Tier(c, step % 3 == 0):
            got = transforms.czt(c.to_device(x), m, w, a, ctx=c).numpy()
            family(c.last_dispatch(), n, m, step % 3 == 0)
        check(f"step {step}: n={n} m={m}", got, O.czt(x, m, O.contour_czt(m, w, a)))
    assert same_bits(dev(c, x0, 300, "zoom")[0], first) and same_bits(dev(c, x0, 300, "zoom", True)[0], first_generic)
    host = transforms.zoom_fft(x0, FN, 300, fs=FS, ctx=c)
    family(c.last_dispatch(), 700, 300, False)
    assert isinstance(host, np.ndarray) and same_bits(host, first)
    xc = noise(402, (3, 5000), True)
    d, _ = dev(c, xc, 37, "czt_wa")
    assert same_bits(transforms.czt(xc, 37, W_UNIT, A_UNIT, ctx=c), d)


def test_a_host_array_along_axis_0_and_integers(ctx):
    x = noise(83, (700, 3))
    y = transforms.zoom_fft(x, FN, 300, fs=FS, ctx=ctx, axis=0)
    assert isinstance(y, np.ndarray) and y.shape == (300, 3) and y.flags.c_contiguous and y.dtype == np.complex64
    check("axis 0", np.ascontiguousarray(y.T), reference(np.ascontiguousarray(x.T), 300, "zoom"))
    ints = ((np.arange(64, dtype=np.int32) % 7) - 3).reshape(1, 64)
    check("integers", transforms.czt(ints, 50, ctx=ctx), reference(ints.astype(np.float32), 50, "czt"))
    assert transforms.czt(x[:, 0], ctx=ctx).shape == (700,)         # m defaults to n
    with pytest.raises(_lib.NxSignalUnsupported, match="last axis"):
        transforms.czt(ctx.to_device(x), axis=0)
    with pytest.raises(_lib.NxSignalUnsupported, match="unsupported"):
        transforms.czt(ctx.to_device(x.astype(np.float64)))


@pytest.mark.parametrize("generic", [False, True], ids=["wave", "generic"])
def test_the_spiral_passes_and_a_contour_beyond_the_gate_is_unsupported(ctx, generic):
    for complex_rows in (False, True):
        x = noise(97, (5, 64), complex_rows)
        worst = check("spiral", dev(ctx, x, 64, "spiral", generic)[0], reference(x, 64, "spiral"))
        print(f"czt-accuracy {'generic' if generic else 'wave'} spiral {'c64' if complex_rows else 'f32'} n=64 m=64 batch=5: {worst:.3e}")
    with Tier(ctx, generic):
        for w, a in ((1.004 * W_UNIT, 1.0), (W_UNIT, 1.2), (1 / 1.004 * W_UNIT, 0.9)):
            with pytest.raises(_lib.NxSignalUnsupported, match="the contour leaves single precision"):
                transforms.czt(ctx.to_device(noise(98, (2, 64))), 64, w, a, ctx=ctx)


def test_a_repeated_call_asks_for_no_new_table():
    """the first call of a contour forms its three tables (and the twiddle tables of its transforms); a second identical call makes no
    request, and neither does the same contour at another batch"""
    c = S.Context(0)
    requests = lambda: c.get_tuning("TABLE_REQUESTS")[0]   # noqa: E731
    for n, m, generic in ((600, 300, False), (1500, 549, False), (600, 300, True), (5000, 37, False)):
        x = noise(91 + n, (3, n))
        first, _ = dev(c, x, m, "zoom", generic)
        before = requests()
        again, _ = dev(c, x, m, "zoom", generic)
        one, _ = dev(c, x[:1], m, "zoom", generic)
        assert requests() == before and same_bits(first, again) and same_bits(one, first[:1]), (n, m, generic)


def test_batch_0_launches_nothing(ctx):
    lib = _lib.load()
    x = ctx.to_device(noise(93, (1, 8)))
    out = ctx.empty((8,), np.complex64)
    rc = lib.nxsig_czt(_lib.ctx_ptr(ctx.handle, _lib._ctx_iir), C.c_void_p(x.ptr), 0, 8, 0, 8, 8, 1.0, 1.0, 8, 1.0, 0.0, C.c_void_p(out.ptr), _lib.DEVICE)
    assert rc == 0 and ctx.last_dispatch() == ""


def test_the_switch_in_the_environment_of_a_fresh_process(tmp_path):
    """NXSIG_CZT_WAVE=0 read at context creation by a child process: the generic tier, the same bound"""
    x = noise(95, (3, 600))
    np.save(tmp_path / "x.npy", x)
    code = (
        "import sys, numpy as np, nx_signal_amd as S\n"
        "from nx_signal_amd import transforms\n"
        "c = S.Context(0)\n"
        "y = transforms.zoom_fft(c.to_device(np.load(sys.argv[1])), [0.1, 0.3], 300, fs=2.0, ctx=c); c.sync()\n"
        "print('DISPATCH', c.last_dispatch()); np.save(sys.argv[2], y.numpy())\n")
    env = dict(os.environ, NXSIG_CZT_WAVE="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "x.npy"), str(tmp_path / "y.npy")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DISPATCH " + GENERIC in r.stdout
    check("NXSIG_CZT_WAVE=0", np.load(tmp_path / "y.npy"), reference(x, 300, "zoom"))


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its CZT_TABLE_ENTRIES with a real context against tests/golden/abi_error_table_czt.json"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_error_probe as P
    with open(P.GOLDEN_CZT) as f:
        golden = json.load(f)
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.CZT_TABLE_ENTRIES)
    assert table == golden["real_ctx"]
    rows = table["nxsig_czt"]
    assert rows["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
    assert all(r["rc"] != 0 for k, r in rows.items() if k != "valid")
    assert len(rows) == len(golden["null_ctx"]["nxsig_czt"]) - 1     # batch = 0 runs with a null context alone
