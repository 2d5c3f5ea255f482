"""Spectral.lombscargle on the GPU (csrc/kernels_lombscargle.hip) against the numpy oracle tests/lombscargle_oracle.py, which
tests/test_lombscargle_host.py holds to recorded SciPy 1.15.3 results.

The error of a row is its largest |got - oracle| over the oracle row's largest magnitude.  f32 rows: 1e-5, the project's standing bar
for f32 results.  f64 rows: 1e-10, 300 times the 3.2e-13 a host emulation of the tile tier's one-pass form shows against SciPy on
these shapes.  "amplitude" is compared where the oracle's shifted CC and SS are both >= 1e-3; the seeded parity inputs leave no
frequency out (asserted here and, without a GPU, in tests/test_lombscargle_host.py).  The blocking sizes FB (frequencies per
workgroup), RB (rows per workgroup) and TT (samples per staged tile) are those nxsig_lombscargle_block answers (read from csrc/lombscargle_plan.hpp at import, held to the
function by a test).  Every test prints its worst
figure on a line that starts with "lombscargle-accuracy"."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import extents as E
import lombscargle_oracle as O
from conftest import ROOT

import nx_signal_amd as S
from nx_signal_amd import _lib, spectral

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-10}
TILE, GENERIC = "lombscargle.tile", "lombscargle.generic"
NORM_CODE = {"power": 0, "normalize": 1, "amplitude": 2}
# The blocking sizes, as csrc/lombscargle_plan.hpp states them.  The parametrised shapes need them when this module is imported, and
# importing a test module must not load libnxsig.so: pytest imports every module before the first test runs, and a process that maps the
# library (and the HIP runtime it links) ahead of a test that imports torch ends up with torch's own copy of the runtime beside it, which
# then answers ctypes.CDLL("libamdhip64.so") in the graph-capture tests of test_gpu_parity.py and knows no device.
# test_the_blocking_sizes_are_the_librarys holds nxsig_lombscargle_block() to these values.
with open(os.path.join(ROOT, "nx_signal_amd", "csrc", "lombscargle_plan.hpp")) as _f:
    _plan = _f.read()
FB, RB, TT = (int(re.search(r"constexpr int %s = (\d+);" % name, _plan).group(1)) for name in ("kLsFB", "kLsRB", "kLsTT"))


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Tier:
    """NXSIG_LOMBSCARGLE_TILE=0 on one context for a block"""

    def __init__(self, ctx, generic):
        self.ctx, self.generic = ctx, generic

    def __enter__(self):
        if self.generic:
            self.ctx.set_tuning("LOMBSCARGLE_TILE", 0)

    def __exit__(self, *exc):
        if self.generic:
            self.ctx.clear_tuning("LOMBSCARGLE_TILE")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def run(ctx, x, y, freqs, generic, device=True, **kw):
    """spectral.lombscargle on a device (or host) tensor: the numpy result, the tier asserted from the dispatch record"""
    with Tier(ctx, generic):
        out = spectral.lombscargle(x, ctx.to_device(y) if device else y, freqs, ctx=ctx, **kw)
        ctx.sync()
        rec = ctx.last_dispatch()
    assert rec == (GENERIC if generic else TILE), rec
    assert isinstance(out, S.DeviceBuffer if device else np.ndarray)
    amplitude = kw.get("normalize") == "amplitude"
    want = {(4, False): np.float32, (8, False): np.float64, (4, True): np.complex64, (8, True): np.complex128}[(y.dtype.itemsize, amplitude)]
    assert out.dtype == want and tuple(out.shape) == y.shape[:-1] + (len(freqs),)
    return out.numpy() if device else out


def line(what, figures):
    print(f"lombscargle-accuracy {what} " + " ".join(f"{k}={v:.3e}" for k, v in figures.items()), flush=True)


def inputs(seed, rows, n, F, tmax=100.0, wmax=20.0, zero=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(0.0, tmax, n)
    freqs = np.sort(rng.uniform(0.01, wmax, F))
    if zero:
        freqs[0] = 0.0
    weights = rng.uniform(0.25, 2.0, n)
    y = 1.5 + rng.standard_normal((rows, n)) + np.sin(1.25 * x)
    return x, y, freqs, weights


def test_the_blocking_sizes_are_the_librarys():
    lib = _lib.load()
    assert [lib.nxsig_lombscargle_block(w) for w in range(3)] == [FB, RB, TT] and min(FB, RB, TT) > 0


# ---- 1. parity: all 24 option combinations, f32 and f64 rows, host and device operands, both tiers
@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_parity_with_the_oracle(ctx, dtype, generic):
    x, y64, freqs, weights = O.parity_inputs()
    assert y64.shape == (3, 257) and freqs.shape == (96,) and freqs.min() > 0.01 and freqs.max() < 20 and x.min() >= 0 and x.max() < 100
    y = y64.astype(dtype)
    tol, worst = TOL[np.dtype(dtype)], {}
    for pre, fm, wts, norm in O.COMBOS:
        kw = dict(precenter=pre, normalize=norm, weights=weights if wts else None, floating_mean=fm)
        want, cc, ss = O.lombscargle(x, y.astype(np.float64), freqs, pre, norm, weights if wts else None, fm, parts=True)
        keep = O.conditioned(cc, ss) if norm == "amplitude" else np.ones(96, bool)
        assert keep.all(), (pre, fm, wts, norm)     # the seeded inputs leave no frequency out
        dev = run(ctx, x, y, freqs, generic, True, **kw)
        host = run(ctx, x, y, freqs, generic, False, **kw)
        assert same_bits(dev, host), (pre, fm, wts, norm)
        err = float(O.row_error(dev.astype(want.dtype), want).max())
        print(f"lombscargle-accuracy parity {np.dtype(dtype).name} {'generic' if generic else 'tile'} {O.combo_name(pre, fm, wts, norm)} {err:.3e}")
        assert err <= tol, (O.combo_name(pre, fm, wts, norm), err, tol)
        worst[norm] = max(worst.get(norm, 0.0), err)
    line(f"parity-worst {np.dtype(dtype).name} {'generic' if generic else 'tile'}", worst)


def test_the_spellings_of_normalize(ctx):
    x, y64, freqs, _ = O.parity_inputs()
    y = y64.astype(np.float32)
    assert same_bits(run(ctx, x, y, freqs, False, normalize=False), run(ctx, x, y, freqs, False, normalize="power"))
    assert same_bits(run(ctx, x, y, freqs, False, normalize=True), run(ctx, x, y, freqs, False, normalize="normalize"))
    # leading axes are kept, and integers are computed as f64
    cube = run(ctx, x, np.stack([y, y]), freqs, False)
    assert cube.shape == (2, 3, 96) and same_bits(cube[1], run(ctx, x, y, freqs, False))
    ints = np.round(4 * y64).astype(np.int32)
    got = spectral.lombscargle(x, ints, freqs, ctx=ctx)
    assert got.dtype == np.float64 and O.row_error(got, O.lombscargle(x, ints, freqs)).max() <= 1e-10


# ---- 2. w = 0 under "power" and "normalize" without floating_mean (with it SciPy divides rounding noise by the clamp there: ill
# conditioned in SciPy too, not compared)
@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_angular_frequency_zero(ctx, dtype, generic):
    x, y64, freqs, weights = inputs(7, 3, 130, 9, zero=True)
    y = y64.astype(dtype)
    worst = {}
    for norm in ("power", "normalize"):
        for pre in (False, True):
            for wts in (False, True):
                want = O.lombscargle(x, y.astype(np.float64), freqs, pre, norm, weights if wts else None, False)
                got = run(ctx, x, y, freqs, generic, precenter=pre, normalize=norm, weights=weights if wts else None)
                assert np.isfinite(got[:, 0]).all()
                err = float(O.row_error(got.astype(np.float64), want).max())
                # ... and the bin itself against the oracle's, on the row's scale
                at0 = float((np.abs(got[:, 0] - want[:, 0]) / np.abs(want).max(axis=-1)).max())
                assert err <= TOL[np.dtype(dtype)] and at0 <= TOL[np.dtype(dtype)], (norm, pre, wts, err, at0)
                worst[norm] = max(worst.get(norm, 0.0), err)
    line(f"zero-frequency {np.dtype(dtype).name} {'generic' if generic else 'tile'}", worst)


# ---- 3. boundary shapes: "power" with weights and precenter, one axis varied at a time around (n, F, batch) = (37, 5, 2)
BASE = (37, 5, 2)
SHAPES = sorted({(n, BASE[1], BASE[2]) for n in (1, 2, TT - 1, TT, TT + 1, 2 * TT + 3)} |
                {(BASE[0], F, BASE[2]) for F in (1, FB - 1, FB, FB + 1)} |
                {(BASE[0], BASE[1], b) for b in (1, RB - 1, RB, RB + 1, 2 * RB + 3) if b >= 1})


@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_F%d_b%d" % s)
def test_boundary_shapes(ctx, shape, generic):
    n, F, batch = shape
    x, y64, freqs, weights = inputs(1000 + 7 * n + 3 * F + batch, batch, n, F)
    figures = {}
    for dtype in (np.float32, np.float64):
        y = y64.astype(dtype)
        want = O.lombscargle(x, y.astype(np.float64), freqs, True, "power", weights, False)
        got = run(ctx, x, y, freqs, generic, precenter=True, normalize="power", weights=weights)
        err = float(O.row_error(got.astype(np.float64), want).max())
        assert err <= TOL[np.dtype(dtype)], (shape, np.dtype(dtype).name, err)
        figures[np.dtype(dtype).name] = err
    line(f"shape n={n} F={F} batch={batch} {'generic' if generic else 'tile'}", figures)


# ---- 4. batch independence and extents, through the C ABI on poisoned arenas
@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
@pytest.mark.parametrize("dtype,norm", [(np.float32, "power"), (np.float64, "amplitude"), (np.float32, "amplitude"), (np.float64, "normalize")],
                         ids=["f32-power", "f64-amplitude", "f32-amplitude", "f64-normalize"])
def test_rows_are_independent_and_stores_stay_inside_the_result(ctx, dtype, norm, generic):
    """2 RB + 3 rows, 5 elements of poison between them, the result between poisoned guards; then every row alone: the same bits"""
    x, y64, freqs, weights = O.parity_inputs()
    rows, n, F = 2 * RB + 3, x.shape[0], freqs.shape[0]
    rng = np.random.Generator(np.random.PCG64(31))
    y = (1.5 + rng.standard_normal((rows, n)) + np.sin(1.25 * x)).astype(dtype)
    odt = {(4, "amplitude"): np.complex64, (8, "amplitude"): np.complex128}.get((np.dtype(dtype).itemsize, norm), dtype)
    want, cc, ss = O.lombscargle(x, y.astype(np.float64), freqs, True, norm, weights, True, parts=True)
    assert norm != "amplitude" or O.conditioned(cc, ss).all()
    fn = _lib.load().nxsig_lombscargle
    pd = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    is64 = int(np.dtype(dtype) == np.float64)

    def call(yrows, stride_gap, offset):
        r = yrows.shape[0]
        yin = E.Arena("y", dtype, r, n, n + stride_gap, offset_elems=offset, data=yrows).upload(ctx)
        out = E.Arena("out", odt, r, F, offset_elems=(offset + 1) % 2).upload(ctx)
        with Tier(ctx, generic):
            rec = E.call(ctx, lambda h, *a: fn(_lib.ctx_ptr(h, _lib._ctx_iir), *a), yin.ptr, is64, n, r, n + stride_gap, pd(x), pd(freqs), F,
                         pd(weights), 1, NORM_CODE[norm], 1, out.ptr, _lib.DEVICE)
        assert rec == (GENERIC if generic else TILE), rec
        return yin, out

    yin, out = call(y, 5, 1)
    image = out.download()
    E.verify([(yin, yin.download())], out, image, expected=want.astype(odt), tol=TOL[np.dtype(dtype)])
    full = out.tensor(image)
    for r in (0, RB - 1, RB, 2 * RB + 2):
        yin1, out1 = call(y[r:r + 1], 0, 0)
        img1 = out1.download()
        E.verify([(yin1, yin1.download())], out1, img1, same_bits_as=full[r:r + 1])
    # the dense batch gives the strided batch's bits as well
    yin2, out2 = call(y, 0, 0)
    E.verify([(yin2, yin2.download())], out2, out2.download(), same_bits_as=full)


def test_a_host_call_with_strided_rows(ctx):
    """mem = NXSIG_HOST with batch_stride > n: the same bits as the dense device call, the poison between the rows never read"""
    x, y64, freqs, weights = O.parity_inputs()
    y = y64.astype(np.float32)
    n, F = y.shape[1], freqs.shape[0]
    yin = E.Arena("y", np.float32, 3, n, n + 3, offset_elems=1, data=y)
    out = E.Arena("out", np.float32, 3, F)
    yimg, oimg = yin.image.copy(), out.image.copy()
    pd = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fn = _lib.load().nxsig_lombscargle
    E.call(ctx, lambda h, *a: fn(_lib.ctx_ptr(h, _lib._ctx_iir), *a), C.c_void_p(yimg.ctypes.data + yin.offset_bytes), 0, n, 3, n + 3, pd(x), pd(freqs),
           F, pd(weights), 0, 0, 0, C.c_void_p(oimg.ctypes.data + out.offset_bytes), _lib.HOST)
    E.verify([(yin, yimg)], out, oimg, same_bits_as=run(ctx, x, y, freqs, False, weights=weights))


# ---- 5. large phases
@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
def test_large_phases(ctx, generic):
    """Times up to 1e5 and angular frequencies up to 1e2: phases up to 1e7 rad, f32 rows at 1e-5.  An f32 phase (spacing 1 rad at 1e7)
    or a fast sine misses this by orders of magnitude.  The phase fl(w t) is the same double in the kernels and in numpy; what remains
    is each sincos's rounding and the summation order.  f64 rows are not held to 1e-10 here: the rotated sums of the tile tier and
    SciPy's shifted phase w t - tau differ by the rounding of a number of size 1e7, about 1e7 * 2^-53 = 1.1e-9 per term."""
    x, y64, freqs, weights = inputs(77, 3, 300, 70, tmax=1e5, wmax=1e2)
    assert (freqs.max() * x.max()) > 5e6
    y = y64.astype(np.float32)
    worst = {}
    for norm in ("power", "normalize", "amplitude"):
        for fm in (False, True):
            want, cc, ss = O.lombscargle(x, y.astype(np.float64), freqs, True, norm, weights, fm, parts=True)
            keep = O.conditioned(cc, ss) if norm == "amplitude" else np.ones(70, bool)
            assert keep.sum() >= 0.98 * 70
            got = run(ctx, x, y, freqs, generic, precenter=True, normalize=norm, weights=weights, floating_mean=fm)
            err = float(O.row_error(got[:, keep].astype(want.dtype), want[:, keep]).max())
            assert err <= 1e-5, (norm, fm, err)
            worst[norm] = max(worst.get(norm, 0.0), err)
    line(f"large-phase f32 {'generic' if generic else 'tile'}", worst)
    # the f64 figure, printed and held only to the f32 bar
    want = O.lombscargle(x, y64, freqs, True, "power", weights, False)
    err = float(O.row_error(run(ctx, x, y64, freqs, generic, precenter=True, weights=weights), want).max())
    line(f"large-phase f64 {'generic' if generic else 'tile'}", {"power": err})
    assert err <= 1e-5


# ---- 6. non-finite rows
@pytest.mark.parametrize("generic", [False, True], ids=["tile", "generic"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_non_finite_row_is_nan_and_the_others_keep_their_bits(ctx, dtype, generic):
    x, y64, freqs, weights = inputs(13, 5, 2 * TT + 3, FB + 3)
    clean = y64.astype(dtype)
    weights[[5, TT + 1]] = 0.0       # a zero weight does not shield the sample it belongs to
    for norm in ("power", "normalize", "amplitude"):
        kw = dict(precenter=True, normalize=norm, weights=weights, floating_mean=True)
        base = run(ctx, x, clean, freqs, generic, **kw)
        assert np.isfinite(base.real).all() and np.isfinite(base.imag).all()
        for spots in ((5, TT + 1), (0, 2 * TT + 2)):
            y = clean.copy()
            y[3, spots[0]], y[3, spots[1]] = np.nan, np.inf
            got = run(ctx, x, y, freqs, generic, **kw)
            parts = np.stack([got[3].real, got[3].imag]) if norm == "amplitude" else got[3]
            assert np.isnan(parts).all(), (norm, spots)
            assert same_bits(got[[0, 1, 2, 4]], base[[0, 1, 2, 4]]), (norm, spots)
        y = clean.copy()
        y[3, 7] = -np.inf                # an Inf alone
        got = run(ctx, x, y, freqs, generic, **kw)
        assert np.isnan(got[3].real).all() and same_bits(got[[0, 1, 2, 4]], base[[0, 1, 2, 4]])


# ---- 7. dispatch
def test_the_dispatch_record_names_the_tier(ctx):
    x, y64, freqs, _ = O.parity_inputs()
    y = y64.astype(np.float32)
    run(ctx, x, y, freqs, False)
    run(ctx, x, y, freqs, True)
    run(ctx, x, y, freqs, False)     # the switch is cleared again
    # the tier does not depend on the batch
    for rows in (1, RB + 1):
        run(ctx, x, np.repeat(y[:1], rows, axis=0), freqs, False)
        run(ctx, x, np.repeat(y[:1], rows, axis=0), freqs, True)


def test_the_switch_in_the_environment_of_a_fresh_process(tmp_path):
    """NXSIG_LOMBSCARGLE_TILE=0 read at context creation by a child process: the generic tier, the same bound"""
    x, y64, freqs, weights = O.parity_inputs()
    y = y64.astype(np.float32)
    np.savez(tmp_path / "in.npz", x=x, y=y, freqs=freqs, weights=weights)
    code = (
        "import sys, numpy as np, nx_signal_amd as S\n"
        "from nx_signal_amd import spectral\n"
        "d = np.load(sys.argv[1])\n"
        "c = S.Context(0)\n"
        "p = spectral.lombscargle(d['x'], c.to_device(d['y']), d['freqs'], True, 'normalize', weights=d['weights'], ctx=c); c.sync()\n"
        "print('DISPATCH', c.last_dispatch()); np.save(sys.argv[2], p.numpy())\n")
    env = dict(os.environ, NXSIG_LOMBSCARGLE_TILE="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.npz"), str(tmp_path / "p.npy")], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DISPATCH " + GENERIC in r.stdout
    want = O.lombscargle(x, y.astype(np.float64), freqs, True, "normalize", weights)
    assert O.row_error(np.load(tmp_path / "p.npy").astype(np.float64), want).max() <= 1e-5


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its LOMBSCARGLE_TABLE_ENTRIES with a real context against its golden file"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_error_probe as P

    with open(P.GOLDEN_LOMBSCARGLE) as f:
        golden = json.load(f)["real_ctx"]
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.LOMBSCARGLE_TABLE_ENTRIES)
    assert table == golden
    assert table["nxsig_lombscargle"]["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
