"""Transforms.dct / idct and mfcc on the GPU against the f64 oracle of tests/dct_oracle.py (the definition of include/nxsig.h) run on the
SAME samples.  The error of a row is max_k |got[k] - ref[k]| / max_k |ref[k]| over the row, the maximum taken over all n coefficients
of the reference also where only `keep` of them are computed; bound 1e-5 for both dispatch families.  Rows of more than 2048 points use
the oracle's np.fft form (the n x n cosine matrix of 65 536 points would take 34 GB) and are also held to the definition itself at the
96 coefficients of dct_oracle.places().

Every run asserts its dispatch record: "dct.direct" alone for n <= 256, "dct.fft" followed by the row transform's families for every
other n and for every n under NXSIG_DISABLE_DCT_DIRECT.  Equal bits between the families are not required.

Offset rows (type 2, 1000 + N(0, 1)): the coefficients k >= 1 are also held to 1e-5 of max_{k>=1} |ref[k]|.

Non-finite rule under test: a row that holds an Inf / NaN among the min(L, n) samples used has no finite output element; the other rows
keep the bits of the all-finite run; a NaN at or beyond n is never read.

Each accuracy check prints one `dct-accuracy <family> ...` line; profiles/dct/accuracy.txt keeps the lines of one MI355X run."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import dct_oracle as O
import extents as E
from conftest import ROOT
from oracle import nx_oracle as NO

import nx_signal_amd as S
from nx_signal_amd import _lib, transforms

pytestmark = pytest.mark.gpu

TOL = 1e-5
DIRECT, FFT = "dct.direct", "dct.fft"
NORM_CODE = {None: 0, "backward": 0, "ortho": 1, "forward": 2}
PAIRS = [(t, norm) for t in O.TYPES for norm in O.NORMS]
DIRECT_N = [1, 2, 3, 8, 13, 64, 80, 128, 255, 256]
FFT_N = [257, 400, 1000, 1024, 2048, 4099, 65536]
FORCED_N = [13, 80, 256]


@pytest.fixture(scope="module")
def ctx():
    return S.Context(0)


class Forced:
    """NXSIG_DISABLE_DCT_DIRECT on one context for a block"""

    def __init__(self, ctx, on):
        self.ctx, self.on = ctx, on

    def __enter__(self):
        if self.on:
            self.ctx.set_tuning("DISABLE_DCT_DIRECT", 1)

    def __exit__(self, *exc):
        if self.on:
            self.ctx.clear_tuning("DISABLE_DCT_DIRECT")


def noise(seed, shape, offset=0.0, scale=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return ((rng.standard_normal(shape) + offset) * scale).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def family(rec, n, forced):
    """the record names the tier first; the fft tier's row transform follows"""
    if n <= 256 and not forced:
        assert rec == DIRECT, (rec, n)
        return "direct"
    assert rec.split("+")[0] == FFT and DIRECT not in rec and len(rec.split("+")) >= 2, (rec, n, forced)
    return "fft-forced" if forced else "fft"


def dev(ctx, x, type=2, n=None, norm=None, keep=None, forced=False, fn=transforms.dct):
    """dct / idct on a device tensor: (numpy result, family)"""
    kw = {} if keep is None else {"keep": keep}
    with Forced(ctx, forced):
        out = fn(ctx.to_device(x), type=type, n=n, norm=norm, ctx=ctx, **kw)
        ctx.sync()
        rec = ctx.last_dispatch()
    assert isinstance(out, S.DeviceBuffer) and out.dtype == np.float32
    return out.numpy(), family(rec, x.shape[-1] if n is None else n, forced)


def reference(x, type, n, norm, fn=O.dct):
    """the full f64 reference [rows][n]; rows longer than 2048 through the oracle's np.fft form, held to the definition at places()"""
    x = np.asarray(x, np.float64)
    nn = x.shape[-1] if n is None else n
    if fn is O.idct:
        type, norm = 5 - type, O.INVERSE_NORM[norm]
    if nn <= 2048:
        return O.dct(x, type, n, norm)
    ref = O.dct_fast(x, type, n, norm)
    at = O.places(nn)
    pin = O.dct_at(x[:3], at, type, n, norm)
    assert np.abs(ref[:3][..., at] - pin).max() <= 1e-11 * np.abs(ref[:3]).max()
    return ref


def row_errors(got, ref, k_from=0):
    """per row: max |got - ref| / max |ref| over the coefficients k >= k_from; got may hold the leading coefficients only.  A row whose
    reference is not finite must hold no finite element"""
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    assert got.shape[0] == ref.shape[0] and got.shape[1] <= ref.shape[1] and got.dtype == np.float32
    errs = []
    for r in range(ref.shape[0]):
        if not np.isfinite(ref[r]).all():
            assert not np.isfinite(got[r]).any(), f"row {r} holds a finite element"
            continue
        assert np.isfinite(got[r]).all(), f"row {r} holds a non-finite element"
        if got.shape[1] <= k_from:
            continue
        scale = np.abs(ref[r, k_from:]).max()
        errs.append(float(np.abs(got[r, k_from:].astype(np.float64) - ref[r, k_from:got.shape[1]]).max() / max(scale, 1e-300)))
    return errs


def check(name, got, ref, k_from=0):
    errs = row_errors(got, ref, k_from)
    worst = max(errs) if errs else 0.0
    assert worst <= TOL, (name, worst)
    return worst


def line(fam, what, figures):
    print(f"dct-accuracy {fam} {what}: " + " ".join(f"{k} {v:.3e}" for k, v in figures.items()))


def parity(ctx, n, forced):
    """every type / norm pair at batch 1, 3 and 65 with rows scaled 1e-4, 1 and 1e4 (rows of more than 2048 points: batch 3 for every
    pair and scale, batch 1 and 65 once per type)"""
    figures = {}
    for t, norm in PAIRS:
        worst = 0.0
        for batch in (1, 3, 65):
            for scale in (1e-4, 1.0, 1e4):
                if n > 2048 and batch != 3 and (norm is not None or scale != 1.0):
                    continue
                x = noise(1000 * batch + n + t, (batch, n), scale=scale)
                got, fam = dev(ctx, x, t, None, norm, None, forced)
                worst = max(worst, check(f"n={n} type={t} norm={norm} batch={batch} scale={scale}", got, reference(x, t, None, norm)))
        figures[f"t{t}/{norm}"] = worst
    line(fam, f"n={n}", figures)


@pytest.mark.parametrize("n", DIRECT_N)
def test_the_direct_family(ctx, n):
    parity(ctx, n, False)


@pytest.mark.parametrize("n", FFT_N)
def test_the_fft_family(ctx, n):
    parity(ctx, n, False)


@pytest.mark.parametrize("n", FORCED_N)
def test_the_fft_family_with_the_direct_one_switched_off(ctx, n):
    parity(ctx, n, True)


@pytest.mark.parametrize("forced", [False, True], ids=["direct", "fft"])
def test_70000_rows_of_8(ctx, forced):
    """rows live on gridDim.x: 70 000 of them pass (gridDim.y would stop at 65 535)"""
    x = noise(70, (70000, 8))
    figures = {}
    for t, norm in ((2, "ortho"), (3, None)):
        got, fam = dev(ctx, x, t, None, norm, None, forced)
        figures[f"t{t}/{norm}"] = check(f"70000 x 8 type={t}", got, O.dct(x, t, None, norm))
    line(fam, "n=8 batch=70000", figures)


@pytest.mark.parametrize("n,forced", [(80, False), (128, False), (256, False), (80, True), (256, True), (257, False), (1024, False), (4099, False)],
                         ids=lambda v: str(v))
def test_offset_rows(ctx, n, forced):
    """type 2 of 1000 + N(0, 1): y[0] carries the offset, the coefficients k >= 1 only the noise — and they too stay within 1e-5 of
    their own maximum.  dct.direct gets there by centring the row (include/nxsig.h), dct.fft as it stands"""
    x = noise(71 + n, (5, n), offset=1000.0)
    figures = {}
    for norm in O.NORMS:
        got, fam = dev(ctx, x, 2, None, norm, None, forced)
        ref = reference(x, 2, None, norm)
        check(f"offset rows n={n} norm={norm}: the whole row", got, ref)
        figures[f"k>=1/{norm}"] = check(f"offset rows n={n} norm={norm}: k >= 1", got, ref, k_from=1)
    line(f"offset-1000-{'fft' if fam.startswith('fft') else 'direct'}", f"n={n}{' forced' if forced else ''}", figures)


@pytest.mark.parametrize("n,forced", [(13, False), (80, False), (256, False), (13, True), (80, True), (256, True), (1000, False)], ids=lambda v: str(v))
def test_keep_is_the_leading_slice_to_the_bit(ctx, n, forced):
    x = noise(31 + n, (5, n))
    for t, norm in PAIRS:
        full, _ = dev(ctx, x, t, None, norm, None, forced)
        for keep in sorted({1, min(13, n - 1), n - 1, n}):
            got, _ = dev(ctx, x, t, None, norm, keep, forced)
            assert got.shape == (5, keep) and same_bits(got, full[:, :keep]), (n, t, norm, keep, forced)


SHAPES = [(7, 16), (100, 257), (8, 5), (300, 128), (80, 80), (13, 13), (128, 128), (1000, 1000)]   # (L, n)


@pytest.mark.parametrize("forced", [False, True], ids=["default", "fft"])
@pytest.mark.parametrize("t", O.TYPES)
def test_padding_truncation_and_strided_rows_inside_poisoned_arenas(ctx, t, forced):
    """batch 3 with batch_stride = L + 5 (and dense rows) through the C entry point, rows and results 0 .. 3 elements off a 16-byte
    boundary, inside poisoned arenas: the guards and gaps untouched, every result element written and nothing past out[batch][keep],
    the input unchanged, nothing at or past min(L, n) read (the gaps hold NaN), the results in bound"""
    lib = _lib.load()
    fn = lambda h, *a: lib.nxsig_dct_f32(_lib.ctx_ptr(h, _lib._ctx_iir), *a)   # noqa: E731
    for L, n in SHAPES:
        x = noise(3 * L + n, (3, L))
        for keep, norm in ((n, None), (min(n, 13), "ortho")):
            ref = O.dct(x, t, n, norm)
            exp = ref[:, :keep].astype(np.float32)
            with Forced(ctx, forced):
                for gap, offset in ((5, 1), (5, 2), (5, 3), (0, 0), (0, 1)):
                    xin = E.Arena("x", np.float32, 3, L, L + gap, offset_elems=offset, data=x).upload(ctx)
                    out = E.Arena("out", np.float32, 3, keep, offset_elems=(offset + 1) % 4).upload(ctx)
                    rec = E.call(ctx, fn, xin.ptr, L, 3, L + gap, n, t, NORM_CODE[norm], keep, out.ptr, _lib.DEVICE)
                    family(rec, n, forced)
                    E.verify([(xin, xin.download())], out, out.download(), expected=exp, tol=TOL)
                    check(f"strided L={L} n={n} gap={gap} keep={keep}", out.tensor(out.download()), ref)
                # host memory: the staged copy keeps the row stride
                xin = E.Arena("x", np.float32, 3, L, L + 5, offset_elems=1, data=x)
                out = E.Arena("out", np.float32, 3, keep)
                ximg, oimg = xin.image.copy(), out.image.copy()
                E.call(ctx, fn, C.c_void_p(ximg.ctypes.data + xin.offset_bytes), L, 3, L + 5, n, t, NORM_CODE[norm], keep,
                       C.c_void_p(oimg.ctypes.data + out.offset_bytes), _lib.HOST)
                E.verify([(xin, ximg)], out, oimg, expected=exp, tol=TOL)


@pytest.mark.parametrize("n,keep,forced", [(80, 13, False), (13, 13, False), (256, 40, False), (80, 13, True), (1000, 1000, False)], ids=lambda v: str(v))
def test_a_rows_bits_depend_neither_on_the_batch_nor_on_where_the_tensors_live(ctx, n, keep, forced):
    x = noise(41 + n, (65, n))
    for t, norm in ((2, "ortho"), (3, None)):
        whole, _ = dev(ctx, x, t, None, norm, keep, forced)
        alone, _ = dev(ctx, x[37:38], t, None, norm, keep, forced)
        assert same_bits(whole[37:38], alone), (n, t, forced)
        with Forced(ctx, forced):
            host = transforms.dct(x, type=t, norm=norm, keep=keep, ctx=ctx)
            family(ctx.last_dispatch(), n, forced)
        assert isinstance(host, np.ndarray) and same_bits(host, whole), (n, t, forced)


@pytest.mark.parametrize("n,forced", [(13, False), (80, False), (256, False), (13, True), (80, True), (256, True), (1000, False), (2048, False),
                                      (4099, False)], ids=lambda v: str(v))
def test_a_non_finite_sample_takes_its_row_and_no_other(ctx, n, forced):
    clean = noise(61 + n, (6, n))
    for t, norm in ((2, None), (2, "ortho"), (3, None), (3, "ortho")):
        base, _ = dev(ctx, clean, t, None, norm, None, forced)
        for spot in (0, n // 3, n - 1):
            x = clean.copy()
            x[1, spot], x[4, spot] = np.nan, np.inf
            with np.errstate(all="ignore"):
                y, _ = dev(ctx, x, t, None, norm, None, forced)
            assert not np.isfinite(y[[1, 4]]).any(), (n, t, norm, spot, forced)
            assert same_bits(y[[0, 2, 3, 5]], base[[0, 2, 3, 5]]), (n, t, norm, spot, forced)
        # keep < n: the kept coefficients of a bad row are not finite either
        y, _ = dev(ctx, x, t, None, norm, max(1, n // 4), forced)
        assert not np.isfinite(y[[1, 4]]).any() and np.isfinite(y[[0, 2, 3, 5]]).all()
    # at or beyond n a NaN is not part of the row: a truncated row keeps its bits
    long = noise(67 + n, (4, n + 9))
    want, _ = dev(ctx, long, 2, n, "ortho", None, forced)
    long[1, n:] = np.nan
    long[2, n] = np.inf
    got, _ = dev(ctx, long, 2, n, "ortho", None, forced)
    assert np.isfinite(got).all() and same_bits(got, want), (n, forced)


@pytest.mark.parametrize("n,forced", [(13, False), (80, False), (256, False), (80, True), (1000, False), (2048, False)], ids=lambda v: str(v))
def test_idct_of_dct_returns_the_row(ctx, n, forced):
    x = noise(51 + n, (3, n))
    figures = {}
    for t in O.TYPES:
        for norm in O.NORMS + ("backward",):
            with Forced(ctx, forced):
                y = transforms.dct(ctx.to_device(x), type=t, norm=norm, ctx=ctx)
                back = transforms.idct(y, type=t, norm=norm, ctx=ctx)
                rec = ctx.last_dispatch()
            fam = family(rec, n, forced)
            back = back.numpy()
            err = float((np.abs(back.astype(np.float64) - x).max(axis=-1) / np.abs(x).max(axis=-1)).max())
            assert err <= TOL, (n, t, norm, err)
            figures[f"t{t}/{norm}"] = err
            # idct itself against the oracle's
            got, _ = dev(ctx, x, t, None, norm, None, forced, fn=transforms.idct)
            check(f"idct n={n} type={t} norm={norm}", got, reference(x, t, None, norm, fn=O.idct))
    line(fam, f"round-trip n={n}", figures)


def test_a_repeated_call_asks_for_no_new_table():
    """the first call of a parameter set forms its table (and the row transform's twiddles); a second identical call makes no request"""
    c = S.Context(0)
    requests = lambda: c.get_tuning("TABLE_REQUESTS")[0]   # noqa: E731
    for n, keep, t, forced in ((80, 13, 2, False), (80, 80, 3, False), (256, 20, 2, False), (1000, None, 2, False), (1000, 7, 3, False), (80, 13, 2, True)):
        x = noise(91 + n, (3, n))
        first, _ = dev(c, x, t, None, "ortho", keep, forced)
        before = requests()
        again, _ = dev(c, x, t, None, "ortho", keep, forced)
        assert requests() == before and same_bits(first, again), (n, keep, t, forced)


def test_a_host_array_along_axis_0_and_integers(ctx):
    x = noise(83, (80, 3))
    y = transforms.dct(x, ctx=ctx, axis=0, norm="ortho", keep=13)
    assert isinstance(y, np.ndarray) and y.shape == (13, 3) and y.flags.c_contiguous
    check("axis 0", np.ascontiguousarray(y.T), O.dct(np.ascontiguousarray(x.T), 2, None, "ortho"))
    z = transforms.idct(x, n=50, ctx=ctx, axis=0)
    assert z.shape == (50, 3)
    check("axis 0, n=50", np.ascontiguousarray(z.T), O.idct(np.ascontiguousarray(x.T), 2, 50, None))
    ints = (np.arange(64, dtype=np.int32) % 7) - 3
    check("integers", transforms.dct(ints, ctx=ctx), O.dct(ints.astype(np.float64)))
    with pytest.raises(_lib.NxSignalUnsupported, match="last axis"):
        transforms.dct(ctx.to_device(x), axis=0)
    with pytest.raises(_lib.NxSignalUnsupported, match="unsupported"):
        transforms.dct(ctx.to_device(x.astype(np.float64)))


def test_batch_0_launches_nothing(ctx):
    lib = _lib.load()
    x = ctx.to_device(noise(93, (1, 8)))
    out = ctx.empty((8,), np.float32)
    rc = lib.nxsig_dct_f32(_lib.ctx_ptr(ctx.handle, _lib._ctx_iir), C.c_void_p(x.ptr), 8, 0, 8, 8, 2, 0, 8, C.c_void_p(out.ptr), _lib.DEVICE)
    assert rc == 0 and ctx.last_dispatch() == ""


MFCC = [
    ("whisper", dict(N=400, K=512, hop=160, bands=80, n_mfcc=13)),
    ("1024", dict(N=1024, K=1024, hop=256, bands=128, n_mfcc=20)),
]


@pytest.mark.parametrize("name,g", MFCC, ids=[m[0] for m in MFCC])
def test_mfcc(ctx, name, g):
    """3 rows of 4096 samples: the bits of transforms.dct(mel_spectrogram(...), type=2, norm="ortho", keep=n_mfcc), host input and
    device input alike, and within 1e-5 of the f64 oracle's transform of the oracle's log-mel"""
    x = noise(97 + g["N"], (3, 4096))
    w = S.windows.hann(g["N"])
    opts = dict(overlap_length=g["N"] - g["hop"], fft_length=g["K"], sampling_rate=16000, mel_bins=g["bands"])
    xd = ctx.to_device(x)
    got = S.mfcc(xd, w, ctx=ctx, n_mfcc=g["n_mfcc"], **opts)
    assert isinstance(got, S.DeviceBuffer) and ctx.last_dispatch() == DIRECT
    got = got.numpy()
    mel = S.mel_spectrogram(xd, w, ctx=ctx, **opts)
    two = transforms.dct(mel, type=2, norm="ortho", keep=g["n_mfcc"]).numpy()
    assert got.shape == mel.shape[:-1] + (g["n_mfcc"],) and same_bits(got, two)
    host = S.mfcc(x, w, ctx=ctx, n_mfcc=g["n_mfcc"], **opts)
    assert isinstance(host, np.ndarray) and same_bits(host, got)
    host_two = transforms.dct(S.mel_spectrogram(x, w, ctx=ctx, **opts), type=2, norm="ortho", keep=g["n_mfcc"], ctx=ctx)
    assert same_bits(host, host_two)
    mel_opts = {k: v for k, v in opts.items() if k != "mel_bins"}
    zo, _, _ = NO.stft(x, w, **mel_opts)
    melo = NO.stft_to_mel(zo.reshape(-1, g["K"]), 16000, g["K"], mel_bins=g["bands"]).reshape(zo.shape[:-1] + (g["bands"],))   # one tensor: one maximum
    worst = check(f"mfcc {name}", got, O.dct(melo, 2, None, "ortho"))
    line("mfcc", f"N={g['N']} K={g['K']} hop={g['hop']} bands={g['bands']} n_mfcc={g['n_mfcc']} rows=3x4096", {"worst": worst})


def test_c_abi_error_table_with_a_context():
    """tools/abi_error_probe.py over its DCT_TABLE_ENTRIES with a real context against tests/golden/abi_error_table_dct.json"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_error_probe as P
    with open(P.GOLDEN_DCT) as f:
        golden = json.load(f)
    table = P.probe(_lib.LIB_PATH, real=True, entries=P.DCT_TABLE_ENTRIES)
    assert table == golden["real_ctx"]
    rows = table["nxsig_dct_f32"]
    assert rows["valid"] == {"rc": 0, "err": "", "host_equals_device": True}
    assert all(r["rc"] != 0 for k, r in rows.items() if k != "valid")
