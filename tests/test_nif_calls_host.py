"""What the dirty-NIF shim (nif/nxsig_nif.c) hands to the C ABI and gives back to the BEAM, call by call, without a GPU.

tests/nif_trace.py builds the shim over a recording stand-in for libnxsig (tests/stub/nxsig_recorder.c and one definition per
function generated from include/nxsig.h): the host generators, length helpers and shard plans run in the real library, every call
that needs a context or a group is written down — name, every integer and double, nxsig_stft_params by field, counted arrays by
value, every other pointer as null / host / dev#k, the mem flag — and answered with 0, or with the code a test asked for.

For each entry of the funcs[] table: one well-formed call with the term shapes the Elixir wrappers build (batch 2, tens of samples,
a non-zero pad_lo, fft_length != frame_length); the same call with its compute entry failing (-1); with the result allocation
failing (a BEAM binary limit of 64 bytes and nxsig_alloc returning NXSIG_ERR_OOM; for three-member groups also the SECOND
nxsig_alloc); every argument replaced by an atom in turn (one letter per position, B = badarg); every binary / buffer operand one
element short and one element long; for buffers, one that belongs to another context / group.  Group NIFs run with 1 and 3 local
members.  A case is [returned term, records, [live binaries, live resources, live device blocks after everything is released]];
binaries appear as b<bytes>, device buffers as r<buf_size>, other resources as res.

tests/golden/nif_calls.json is the transcript of the commit named inside it; the shim must reproduce it byte for byte.

    python tests/test_nif_calls_host.py --write tests/golden/nif_calls.json --parent HASH
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nif_harness as H   # noqa: E402
import nif_trace as T   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "nif_calls.json")
CTX, GRP = "<ctx>", "<grp>"


class Bin:
    """a binary operand of `n` elements of `elem` bytes (never read: the stand-in computes nothing)"""

    def __init__(self, n, elem):
        self.n, self.elem = n, elem


class Buf(Bin):
    """the same in a device buffer of the case's context"""


class Bufs:
    """one device buffer per group member, member i holding n[i] elements"""

    def __init__(self, n, elem):
        self.n, self.elem = list(n), elem


# ---- the shapes: batch 2, 40 samples, frames of 16 every 4 -> 8 frames of the padded row, 32 bins
BATCH, LEN, N, HOP, K, M, OLA, TAPS, BINS = 2, 40, 16, 4, 32, 8, 44, 5, 4
P = (N, HOP, K, 3, 3, 1, 1, 100.0)   # {n, hop, k, pad_mode, pad_lo, pad_hi, scaling, sampling_rate}: explicit padding 3 + 1
X, XC, W, H5, Z, FILT = Bin(BATCH * LEN, 4), Bin(BATCH * LEN, 8), Bin(N, 4), Bin(TAPS, 4), Bin(BATCH * M * K, 8), Bin(BINS * K, 4)
XD, ZD = Buf(BATCH * LEN, 4), Buf(BATCH * M * K, 8)


def plan(kind, a, b, c, world, rank):
    return H.call("shard_range", kind, a, b, c, world, rank)[1]


def shard_elems(n, axis, per_row, kind, a, b, c, per_item=1):
    """elements of member i's INPUT shard: rows of the channel split, or the span the frame / sample split reads"""
    out = []
    for i in range(n):
        rows, items = BATCH, per_row
        if axis == 0:
            r = plan(0, BATCH, 0, 0, n, i)
            rows = r[1] - r[0]
        else:
            r = plan(kind, a, b, c, n, i)
            items = r[1] - r[0] if kind == 2 else r[3] - r[2]
        out.append(rows * items * per_item)
    return out


def row_parts(n, row_bytes):
    return [(r[0], r[1] - r[0], 0, row_bytes) for r in (plan(0, BATCH, 0, 0, n, i) for i in range(n))]


def stft_shards(n, axis):
    return Bufs(shard_elems(n, axis, LEN, 1, M, N, HOP), 4)


# name -> (the compute entry a failure is injected into, {variant: members -> arguments})
SPECS = {
    "device_count": ("nxsig_device_count", {"": lambda n: []}),
    "ctx_create": ("nxsig_ctx_create", {"": lambda n: [0]}),
    "sync": ("nxsig_sync", {"": lambda n: [CTX]}),
    "last_dispatch": ("nxsig_ctx_last_dispatch", {"": lambda n: [CTX]}),
    "window": ("nxsig_window_f32", {"": lambda n: [5, LEN, 1, 0.0, 1e-7]}),
    "window_f64": ("nxsig_window_f64", {"": lambda n: [6, LEN, 0, 9.0, 1e-7]}),
    "firwin": ("nxsig_firwin_f32", {"": lambda n: [21, [0.2, 0.5], 4, 0.0, 0, 1, 2.0]}),
    "firwin_f64": ("nxsig_firwin_f64", {"": lambda n: [21, [0.2, 0.5], 4, 0.0, 0, 1, 2.0]}),
    "fft_frequencies": ("nxsig_fft_frequencies_f32", {"": lambda n: [100.0, K, 0]}),
    "fft_frequencies_f64": ("nxsig_fft_frequencies_f64", {"": lambda n: [100, K, 1]}),
    "mel_filters": ("nxsig_mel_filters_f32", {"": lambda n: [K, BINS, 100.0, 3016.0, 200.0 / 3.0]}),
    "sinc": ("nxsig_sinc_f32", {"": lambda n: [Bin(LEN, 4)]}),
    "sinc_f64": ("nxsig_sinc_f64", {"": lambda n: [Bin(LEN, 8)]}),
    "stft": ("nxsig_stft_f32", {"": lambda n: [CTX, X, LEN, BATCH, W, P]}),
    "stft_c64": ("nxsig_stft_c64", {"": lambda n: [CTX, XC, LEN, BATCH, W, P]}),
    "stft_f64": ("nxsig_stft_f64", {"": lambda n: [CTX, XC, LEN, BATCH, W, 0, P], "w64": lambda n: [CTX, XC, LEN, BATCH, Bin(N, 8), 1, P]}),
    "stft_c128": ("nxsig_stft_c128", {"": lambda n: [CTX, Bin(BATCH * LEN, 16), LEN, BATCH, Bin(N, 8), 1, P]}),
    "istft": ("nxsig_istft_c64", {"": lambda n: [CTX, Z, M, BATCH, W, P]}),
    "istft_c128": ("nxsig_istft_c128", {"": lambda n: [CTX, Bin(BATCH * M * K, 16), M, BATCH, Bin(N, 8), 1, P]}),
    "istft_filtered": ("nxsig_istft_filtered_c64", {"": lambda n: [CTX, Z, M, BATCH, W, P, Bin(K, 8)]}),
    "fir": ("nxsig_fir_f32", {"": lambda n: [CTX, X, LEN, BATCH, H5, 1]}),
    "fir_f64": ("nxsig_fir_f64", {"": lambda n: [CTX, XC, LEN, BATCH, Bin(TAPS, 8), 2]}),
    "as_windowed": ("nxsig_as_windowed_f32", {"": lambda n: [CTX, X, LEN, BATCH, N, HOP, 3, 3, 1]}),
    "as_windowed_f64": ("nxsig_as_windowed_f64", {"": lambda n: [CTX, XC, LEN, BATCH, N, HOP, 3, 3, 1]}),
    "overlap_and_add": ("nxsig_overlap_and_add", {"": lambda n: [CTX, Bin(BATCH * M * N, 8), M, BATCH, N, 12, 2],
                                                  "overlap": lambda n: [CTX, Bin(BATCH * M * N, 4), M, BATCH, N, N, 1]}),
    "overlap_and_add_f64": ("nxsig_overlap_and_add_f64", {"": lambda n: [CTX, Bin(BATCH * M * N, 16), M, BATCH, N, 12, 2]}),
    "fft": ("nxsig_fft", {"": lambda n: [CTX, Bin(3 * 20, 4), 1, 3, 20, K, 0], "c64": lambda n: [CTX, Bin(3 * 20, 8), 0, 3, 20, K, 1]}),
    "fft_c128": ("nxsig_fft_c128", {"": lambda n: [CTX, Bin(3 * 20, 8), 1, 3, 20, K, 0], "c128": lambda n: [CTX, Bin(3 * 20, 16), 0, 3, 20, K, 1]}),
    "fftconvolve_c64": ("nxsig_fftconvolve_c64", {"": lambda n: [CTX, Bin(20, 8), Bin(TAPS, 8), 0]}),
    "fft_nd": ("nxsig_fft_nd", {"": lambda n: [CTX, Bin(40, 4), 1, [4, 10], [0, -1], [8, 16], 0]}),
    "fftconvolve_nd": ("nxsig_fftconvolve_nd", {"": lambda n: [CTX, Bin(40, 4), 1, [4, 10], Bin(6, 8), 0, [2, 3], 1],
                                                "ranks": lambda n: [CTX, Bin(40, 4), 1, [4, 10], Bin(6, 4), 1, [6], 0]}),
    "convolve_direct": ("nxsig_convolve_direct", {"": lambda n: [CTX, Bin(40, 4), 1, [4, 10], Bin(6, 4), 1, [2, 3], 2],
                                                  "ranks": lambda n: [CTX, Bin(40, 4), 1, [4, 10], Bin(6, 4), 1, [6], 0]}),
    "median": ("nxsig_median_filter", {"": lambda n: [CTX, Bin(40, 4), 0, [4, 10], [3, 3]]}),
    "wiener": ("nxsig_wiener", {"": lambda n: [CTX, Bin(40, 8), 1, [4, 10], [3, 1], 1, 0.5]}),
    "resample_poly": ("nxsig_resample_poly", {"": lambda n: [CTX, XC, 1, LEN, BATCH, Bin(7, 4), 3, 2]}),
    "resample_poly_dev": ("nxsig_resample_poly", {"": lambda n: [CTX, Buf(BATCH * LEN, 8), 1, LEN, BATCH, Bin(7, 4), 3, 2]}),
    "welch": ("nxsig_welch_f32", {"": lambda n: [CTX, X, LEN, BATCH, W, HOP, K, 1, 0, 100.0]}),
    "csd": ("nxsig_csd_f32", {"": lambda n: [CTX, X, X, LEN, BATCH, W, HOP, K, 1, 1, 100.0]}),
    "argrelextrema": ("nxsig_argrelextrema", {"": lambda n: [CTX, Bin(40, 8), 1, [4, 10], 1, 2, 1]}),
    "nonzero": ("nxsig_nonzero", {"": lambda n: [CTX, Bin(40, 1), [4, 10]]}),
    "sawtooth": ("nxsig_sawtooth", {"": lambda n: [CTX, Bin(LEN, 4), 0, 0.5]}),
    "square": ("nxsig_square", {"": lambda n: [CTX, Bin(LEN, 8), 1, 0.5, Bin(LEN, 8)], "number": lambda n: [CTX, Bin(LEN, 4), 0, 0.25, Bin(0, 4)]}),
    "gaussian_pulse": ("nxsig_gaussian_pulse", {"": lambda n: [CTX, Bin(LEN, 4), 0, 5.0, 0.5, -6.0]}),
    "chirp": ("nxsig_chirp", {"": lambda n: [CTX, Bin(LEN, 4), 0, (1.0, 10, 20.0), 1, 0, 0.0]}),
    "polynomial_sweep": ("nxsig_polynomial_sweep", {"": lambda n: [CTX, Bin(LEN, 4), 0, Bin(3, 8), 90.0, 1],
                                                    "many": lambda n: [CTX, Bin(LEN, 4), 0, Bin(33, 8), 0.0, 0]}),
    "unit_impulse": ("nxsig_unit_impulse", {"": lambda n: [CTX, 3, [4, 10], [1, 2]]}),
    "stft_to_mel": ("nxsig_stft_to_mel", {"": lambda n: [CTX, Bin(BATCH * M * K, 8), BATCH * M, K, BINS, FILT]}),
    "stft_mel": ("nxsig_stft_mel_f32", {"": lambda n: [CTX, X, LEN, BATCH, W, P, BINS, FILT]}),
    "stft_magnitude": ("nxsig_stft_magnitude_f32", {"": lambda n: [CTX, X, LEN, BATCH, W, P, 2]}),
    "to_device": ("nxsig_upload", {"": lambda n: [CTX, Bin(LEN, 4)]}),
    "from_device": ("nxsig_download", {"": lambda n: [Buf(LEN, 4)]}),
    "buf_size": (None, {"": lambda n: [Buf(LEN, 4)]}),
    "stft_dev": ("nxsig_stft_f32", {"": lambda n: [CTX, XD, LEN, BATCH, W, P]}),
    "stft_c64_dev": ("nxsig_stft_c64", {"": lambda n: [CTX, Buf(BATCH * LEN, 8), LEN, BATCH, W, P]}),
    "stft_onesided_dev": ("nxsig_stft_onesided_f32", {"": lambda n: [CTX, XD, LEN, BATCH, W, P]}),
    "stft_packed_dev": ("nxsig_stft_packed_f32", {"": lambda n: [CTX, XD, LEN, BATCH, W, P]}),
    "istft_packed_dev": ("nxsig_istft_packed_f32", {"": lambda n: [CTX, Buf(BATCH * M * K // 2, 8), M, BATCH, W, P]}),
    "istft_dev": ("nxsig_istft_c64", {"": lambda n: [CTX, ZD, M, BATCH, W, P]}),
    "istft_filtered_dev": ("nxsig_istft_filtered_c64", {"": lambda n: [CTX, ZD, M, BATCH, W, P, Bin(K, 8)]}),
    "fir_dev": ("nxsig_fir_f32", {"": lambda n: [CTX, XD, LEN, BATCH, H5, 0]}),
    "spectrum_mul_dev": ("nxsig_spectrum_mul_c64", {"": lambda n: [CTX, ZD, BATCH * M, K, Bin(K, 8)]}),
    "spectrum_mask": ("nxsig_spectrum_mask_c64", {"": lambda n: [CTX, Bin(M * K, 8), 1, Bin(BATCH * M * (K // 2 + 1), 4), 1, BATCH, M, K],
                                                  "dev": lambda n: [CTX, ZD, BATCH, Buf(BATCH * M * K, 4), 0, BATCH, M, K]}),
    "istft_masked": ("nxsig_istft_masked_c64", {"": lambda n: [CTX, Z, BATCH, M, W, P, Bin(M * K, 8), 2, 1],
                                                "dev": lambda n: [CTX, Buf(M * K, 8), 1, M, W, P, Buf(BATCH * M * (K // 2 + 1), 4), 1, BATCH]}),
    "group_create": ("nxsig_group_create_local", {"": lambda n: [[0] * n]}),
    "group_info": (None, {"": lambda n: [GRP]}),
    "stft_sharded": ("nxsig_stft_sharded_f32", {"": lambda n: [GRP, X, LEN, BATCH, W, P, 0, 1]}),
    "istft_sharded": ("nxsig_istft_sharded_c64", {"": lambda n: [GRP, Z, M, BATCH, W, P, 1, 0]}),
    "fir_sharded": ("nxsig_fir_sharded_f32", {"": lambda n: [GRP, X, LEN, BATCH, H5, 1, 0, 0]}),
    "stft_mel_sharded": ("nxsig_stft_mel_sharded_f32", {"": lambda n: [GRP, X, LEN, BATCH, W, P, BINS, FILT, 0]}),
    "shard_range": ("nxsig_shard_frames", {"": lambda n: [1, M, N, HOP, 3, 1], "range": lambda n: [0, BATCH, 0, 0, 3, 2],
                                           "istft": lambda n: [2, 100, N, HOP, 3, 1], "fir": lambda n: [3, LEN, TAPS, 1, 3, 2],
                                           "kind": lambda n: [4, 1, 1, 1, 1, 0]}),
    "group_scatter": ("nxsig_upload", {"": lambda n: [GRP, Bin(BATCH * 160, 1), BATCH, 160, row_parts(n, 160)]}),
    "group_gather": ("nxsig_download", {"": lambda n: [GRP, Bufs([p[1] * 160 for p in row_parts(n, 160)], 1), BATCH, 160, row_parts(n, 160)]}),
    "stft_sharded_dev": ("nxsig_stft_sharded_f32", {"": lambda n: [GRP, stft_shards(n, 0), LEN, BATCH, W, P, 0, 0],
                                                    "frames": lambda n: [GRP, stft_shards(n, 1), LEN, BATCH, W, P, 1, 0],
                                                    "gather": lambda n: [GRP, stft_shards(n, 0), LEN, BATCH, W, P, 0, 1]}),
    "istft_sharded_dev": ("nxsig_istft_sharded_c64",
                          {"": lambda n: [GRP, Bufs(shard_elems(n, 0, M, 2, M, N, HOP, N), 8), M, BATCH, W, P, 0, 0],
                           "frames": lambda n: [GRP, Bufs(shard_elems(n, 1, 100, 2, 100, N, HOP, N), 8), 100, BATCH, W, P, 1, 0],
                           "gather": lambda n: [GRP, Bufs(shard_elems(n, 1, 100, 2, 100, N, HOP, N), 8), 100, BATCH, W, P, 1, 1]}),
    "fir_sharded_dev": ("nxsig_fir_sharded_f32",
                        {"": lambda n: [GRP, Bufs(shard_elems(n, 0, LEN, 3, LEN, TAPS, 1), 4), LEN, BATCH, H5, 1, 0, 0],
                         "samples": lambda n: [GRP, Bufs(shard_elems(n, 1, LEN, 3, LEN, TAPS, 0), 4), LEN, BATCH, H5, 0, 1, 0],
                         "gather": lambda n: [GRP, Bufs(shard_elems(n, 1, LEN, 3, LEN, TAPS, 2), 4), LEN, BATCH, H5, 2, 1, 1]}),
    "stft_mel_sharded_dev": ("nxsig_stft_mel_sharded_f32", {"": lambda n: [GRP, stft_shards(n, 0), LEN, BATCH, W, P, BINS, FILT, 0],
                                                            "frames": lambda n: [GRP, stft_shards(n, 1), LEN, BATCH, W, P, BINS, FILT, 1]}),
}


class World:
    """the resources one case needs: made before the recorder is reset, released after the case's records are taken"""

    def __init__(self, members):
        self.members, self.ctx, self.grp, self.held = members, {}, {}, []

    def context(self, which="own"):
        if which not in self.ctx:
            self.ctx[which] = H.call("ctx_create", 0)[1]
        return self.ctx[which]

    def group(self, which="own"):
        if which not in self.grp:
            self.grp[which] = H.call("group_create", [0] * self.members)[1]
        return self.grp[which]

    def value(self, a, delta=0, foreign=False):
        which = "other" if foreign else "own"
        if a is CTX:
            return self.context()
        if a is GRP:
            return self.group()
        if isinstance(a, Buf):
            self.held.append(H.call("to_device", self.context(which), bytes(max(a.n + delta, 0) * a.elem))[1])
            return self.held[-1]
        if isinstance(a, Bin):
            return bytes(max(a.n + delta, 0) * a.elem)
        if isinstance(a, Bufs):   # member i's buffer: bytes [off_i, off_i + len_i) of one row
            lens = [max(n + (delta if i == 0 else 0), 0) * a.elem for i, n in enumerate(a.n)]
            total = max(sum(lens), 1)
            bufs = H.call("group_scatter", self.group(which), bytes(total), 1, total, [(0, 1, sum(lens[:i]), lens[i]) for i in range(len(lens))])[1]
            self.held += bufs
            return bufs
        return a

    def close(self):
        for r in self.held + list(self.ctx.values()) + list(self.grp.values()):
            r.release()


def render(v):
    if isinstance(v, H.Res):
        try:
            out = f"r{H.call('buf_size', v)}"
        except H.BadArg:
            out = "res"
        v.release()
        return out
    if isinstance(v, (bytes, bytearray)):
        return f"b{len(v)}"
    if isinstance(v, tuple):
        return [render(e) for e in v]
    if isinstance(v, list):
        return {"list": [render(e) for e in v]}
    return v


def run(L, name, make_args, members, *, fail=None, limit=None, delta=None, foreign=None, atom=None):
    world = World(members)
    try:
        args = make_args(members)
        args = [world.value(a, delta[1] if delta and delta[0] == i else 0, foreign == i) for i, a in enumerate(args)]
        if atom is not None:
            args[atom] = "x"
        L.rec_reset()
        if limit is not None:
            L.fake_set_alloc_limit(limit)
        for f in fail or ():
            L.rec_fail_next(*f)
        try:
            result = render(H.call(name, *args))
        except H.BadArg:
            result = "BadArg"
        except H.UndefinedNif:
            result = "UndefinedNif"
        except H.NifError as e:
            result = ["NifError", e.code, e.msg]
        finally:
            L.fake_set_alloc_limit(1 << 40)
            L.rec_fail_next(None, 0, 0)
        records = L.rec_log().decode().splitlines()
    finally:
        world.close()
    return [result, records, [L.fake_live_binaries(), L.fake_live_resources(), L.rec_live_allocs()]]


def transcript(parent):
    cases = {}
    with T.session() as L:
        for name, (entry, variants) in SPECS.items():
            for variant, make in variants.items():
                for members in ((1, 3) if any(a is GRP for a in make(1)) or name == "group_create" else (1,)):
                    probe = make(members)
                    key = f"{name}/{len(probe)}" + (f"[{variant}]" if variant else "") + (f"[g{members}]" if members > 1 or GRP in probe else "")
                    cases[f"{key}:ok"] = run(L, name, make, members)
                    cases[f"{key}:fail"] = run(L, name, make, members, fail=[(entry.encode(), -1, 0)] if entry else None)
                    cases[f"{key}:oom"] = run(L, name, make, members, limit=64, fail=[(b"nxsig_alloc", -5, 0)])
                    if members == 3:
                        cases[f"{key}:oom.second"] = run(L, name, make, members, fail=[(b"nxsig_alloc", -5, 1)])
                    terms = ""
                    for i in range(len(probe)):
                        r = run(L, name, make, members, atom=i)
                        assert r[1] == [] and r[2] == [0, 0, 0], (key, i, r)
                        terms += "B" if r[0] == "BadArg" else "E" if isinstance(r[0], list) and r[0][:1] == ["NifError"] else "o"
                    cases[f"{key}:terms"] = terms
                    for i, a in enumerate(probe):
                        if isinstance(a, (Bin, Bufs)):
                            cases[f"{key}:{i}-1"] = run(L, name, make, members, delta=(i, -1))
                            cases[f"{key}:{i}+1"] = run(L, name, make, members, delta=(i, 1))
                        if isinstance(a, (Buf, Bufs)):
                            cases[f"{key}:{i}.foreign"] = run(L, name, make, members, foreign=i)
    rows = ",\n".join(f" {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in cases.items())
    return f'{{"parent": {json.dumps(parent)}, "cases": {{\n{rows}\n}}}}\n'


_cache = {}


def _now():
    if "now" not in _cache:
        with open(GOLDEN) as f:
            _cache["want"] = f.read()
        _cache["now"] = transcript(json.loads(_cache["want"])["parent"])
    return _cache["want"], _cache["now"]


def test_the_stand_in_defines_every_function_the_shim_calls():
    protos, calls = T.prototypes(), T.shim_calls()
    assert len(calls) >= 79 and set(T.HANDWRITTEN) <= set(calls)
    fwd = {n for n in calls if n not in T.HANDWRITTEN and T.forwarded(n, protos[n][1])}
    assert {"nxsig_num_frames", "nxsig_ola_length", "nxsig_conv_length", "nxsig_resample_length", "nxsig_welch_bins", "nxsig_shard_range",
            "nxsig_shard_frames", "nxsig_shard_istft", "nxsig_shard_fir", "nxsig_window_f32", "nxsig_stft_times_f32"} <= fwd
    assert not any("ctx" in t or "group" in t for n in fwd for t, _ in protos[n][1])
    assert "LD_PRELOAD" not in open(T.RECORDER).read() + T.generate()


def test_every_table_entry_has_its_cases():
    cases = json.loads(_now()[1])["cases"]
    with T.session():
        table = H.funcs()
    assert len(table) == 76
    for name, arity in table:
        for kind in ("ok", "fail", "terms"):
            have = [k for k in cases if k.split("[")[0].split(":")[0] == f"{name}/{arity}" and k.endswith(":" + kind)]
            assert have, f"{name}/{arity} has no {kind} case"
        for k in cases:
            if k.startswith(f"{name}/{arity}") and k.endswith(":terms"):
                assert cases[k] == "B" * arity, (k, cases[k])


def test_nothing_outlives_a_case():
    cases = json.loads(_now()[1])["cases"]
    assert not {k: v[2] for k, v in cases.items() if not k.endswith(":terms") and v[2] != [0, 0, 0]}
    with T.session() as L:
        assert (L.fake_live_binaries(), L.fake_live_resources(), L.rec_live_allocs()) == (0, 0, 0)


def test_the_shim_reproduces_the_recorded_transcript():
    want, got = _now()
    if got != want:
        a, b = json.loads(want)["cases"], json.loads(got)["cases"]
        diff = [k for k in a if a[k] != b.get(k)] + [k for k in b if k not in a]
        k = diff[0] if diff else None
        raise AssertionError(f"{len(diff)} cases differ from {GOLDEN}: {diff[:20]}\nfirst, recorded: {a.get(k)}\nfirst, now:      {b.get(k)}")
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "python_marshalling.json"))


if __name__ == "__main__":
    path, parent = sys.argv[sys.argv.index("--write") + 1], sys.argv[sys.argv.index("--parent") + 1]
    with open(path, "w") as f:
        f.write(transcript(parent))
    print(f"wrote {path}")
