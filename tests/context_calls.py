"""A catalogue of calls for the tests of what a context carries from one call to the next (tests/test_gpu_context_state.py).

Every other GPU test checks one call at a time, most of them on a context made for that call.  A context in real use lives for hours
and keeps state between calls: 31 scratch slots that are grown, never cleared, and partly expected to be in a known state when the
next call starts (FIR row flags, the istft non-finite list, the log-mel / dBFS reduction cells); the content-addressed table cache with
the pointer caches in front of it; the caching allocator; the pinned slots of the host path.  The entries below are the calls those
tests string together.  An entry has

    name      its id
    build     (rng, size) -> {argument: numpy array}: seeded inputs at "small" and "large"
    call      (S, ctx, args, dev) -> result: the call through the Python mirror with the context passed in; dev(a) makes a tensor
              operand of the numpy array a — the array itself in host mode, a DeviceBuffer of `ctx` in device mode
    family    the dispatch record the call must LEAD with (tests/test_gpu_dispatch_table.py's rule), per size where the sizes differ;
              "" for the f64 tier, whose launchers note no family
    slots     {ScratchSlot enumerator: "file:line" of the ctx_scratch / HostIo line that takes it} in either mode
    host_slots  the same for the slots only the host mode stages through
    tables    the kinds of cached table the call builds (TABLE_KINDS)
    twin      (args) -> args with Inf / NaN put in, for the entries whose kernels keep non-finite state between passes
    switch    (name, value) of the dispatch switch that takes the entry's family away
    modes     ("host", "device"), or ("host",) where the Python mirror takes host tensors only

"small" is the shape tests/test_gpu_dispatch_table.py pins to the family (or the smallest that reaches the named path), "large" 3 - 6
times that in rows or frames, so that every slot the call uses has to grow.  The truth for every (entry, size, mode) is the same call on
a context created for that one call (fresh()), compared bit for bit with the dispatch record; the oracle is not consulted here, the
rest of the suite ties fresh-context results to it.  This module imports without a GPU (tests/test_context_calls_host.py).

Several families share one slot (enum ScratchSlot names the users): user_pairs() lists every ordered pair of entries that claim the
same slot, and tests/test_context_calls_host.py holds the catalogue to the sources — every `ctx_scratch(<ctx>, kScratch...` line is
cited by a claim or excused in EXCUSED_SITES, every DISABLE_* switch is some entry's `switch`."""
import json
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nx_signal_amd", "csrc")
SIZES = ("small", "large")
MODES = ("host", "device")

TABLE_KINDS = ("wave", "twQ", "rab", "r20", "8k", "two-level", "bluestein", "edge-fix", "fir-spectrum", "fir-delay-line", "mel-filterbank",
               "f64", "resample-phase", "resample-taps", "window", "iir-scan", "iir-zi", "lfilter-scan", "lfilter-zi", "savgol-kernel",
               "savgol-edge", "dct")

# the ctx_table tags of the kernel files that came after the first catalogue -> the kind of table behind each ({}: the file asks for no
# table of its own; welch and hilbert come in through ctx_window ("window") and the wave tables ("wave"))
TABLE_TAGS = {
    "kernels_iir.hip": {"0x11522149": "iir-zi", "0x11525343": "iir-scan", "0x11525443": "iir-scan"},
    "kernels_lfilter.hip": {"0x11f17a49": "lfilter-zi", "0x11f17e43": "lfilter-scan", "0x11f17f43": "lfilter-scan"},
    "kernels_savgol.hip": {"0x5A764B00": "savgol-kernel", "0x5A764500": "savgol-edge"},
    "kernels_dct.hip": {"0xDC700000": "dct"},
    "kernels_resample.hip": {"0x2E5A3B1E": "resample-phase", "0x2E5A3B1D": "resample-taps"},
    "kernels_hilbert.hip": {},
    "kernels_find_peaks.hip": {},
    "kernels_welch.hip": {},
}

# enumerators no entry claims, each with its reason
EXCUSED = {
    "kScratchSlots": "not a slot: the length of Ctx::scratch",
}

# ctx_scratch call sites no entry cites, each with its reason: a site the Python mirror cannot reach on one context
EXCUSED_SITES = {
    "group.cpp:1130": "nxsig_stft_mel_sharded's exchange step: reached through a Group of several contexts only; "
                      "test_a_trim_in_the_middle_of_a_sharded_call and test_a_members_dispatch_record_names_what_its_shard_ran_on run it",
}


# DISABLE_* switches of NXSIG_TUNABLES that are no entry's `switch`, each with its reason (none today)
EXCUSED_SWITCHES = {}


def scratch_sites():
    """[("file:line", enumerator)] of every `ctx_scratch(<ctx>, kScratch...` call under csrc, in file order"""
    sites = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".cpp", ".hpp", ".h")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            for at, text in enumerate(f, 1):
                for m in re.finditer(r"ctx_scratch\(\s*\w+\s*,\s*(kScratch\w+)", text):
                    sites.append((f"{name}:{at}", m.group(1)))
    return sites


def table_tags(name):
    """the tags of the ctx_table calls of one kernel file, as written there (hexadecimal, without the suffix)"""
    with open(os.path.join(CSRC, name)) as f:
        return re.findall(r"ctx_table\(\s*\w+\s*,\s*(0x[0-9A-Fa-f]+)ull", f.read())


def scratch_slots():
    """the enumerators of `enum ScratchSlot` (nxsig_internal.h), in order"""
    with open(os.path.join(CSRC, "nxsig_internal.h")) as f:
        src = f.read()
    body = re.search(r"enum ScratchSlot\s*:\s*int\s*\{(.*?)\};", src, re.S).group(1)
    return re.findall(r"^\s*(kScratch\w+)\s*=", body, re.M)


class Entry:
    def __init__(self, name, build, call, family, slots, tables=(), host_slots=None, twin=None, switch=None, modes=MODES):
        self.name, self.build, self.call, self.family = name, build, call, family
        self.slots, self.host_slots, self.tables = dict(slots), dict(host_slots or {}), tuple(tables)
        self.twin, self.switch, self.modes = twin, switch, tuple(modes)

    def inputs(self, size, twin=False):
        """the entry's seeded inputs (a new copy each time: nothing a call does to them reaches the next one)"""
        assert size in SIZES
        rng = np.random.Generator(np.random.PCG64(zlib.crc32(f"{self.name}:{size}".encode())))
        args = self.build(rng, size)
        return self.twin(args) if twin else args

    def family_of(self, size):
        return self.family[size] if isinstance(self.family, dict) else self.family

    def slots_of(self, mode):
        return {**self.slots, **(self.host_slots if mode == "host" else {})}


def bits(a):
    """the raw words of a result: NaN payloads and signed zeros count"""
    a = np.ascontiguousarray(a).reshape(-1)
    return a.view(np.uint64 if a.dtype in (np.dtype(np.float64), np.dtype(np.complex128)) else np.uint32)


def _flat(res):
    if isinstance(res, dict):
        return [res[k] for k in sorted(res)]
    if isinstance(res, (tuple, list)):
        return [r for item in res for r in _flat(item)]
    return [res]


def run(S, entry, size, mode, ctx, twin=False):
    """one call of the catalogue on `ctx` -> ([words of every result], the calling thread's dispatch record).  Device mode: the operands
    are uploaded, the results downloaded after ctx.sync(), and every buffer is dropped at once, so that the pool recycles it."""
    from nx_signal_amd import _lib

    args = entry.inputs(size, twin)
    if mode == "host":
        res = _flat(entry.call(S, ctx, args, lambda a: a))
        return [bits(r) for r in res], _lib.last_dispatch()
    held = []

    def dev(a):
        held.append(ctx.to_device(a))
        return held[-1]

    res = _flat(entry.call(S, ctx, args, dev))
    record = _lib.last_dispatch()
    ctx.sync()
    out = [bits(r.numpy() if isinstance(r, S.DeviceBuffer) else r) for r in res]
    for b in held + [r for r in res if isinstance(r, S.DeviceBuffer)]:
        b.free()
    return out, record


_TRUTH = {}


def fresh(S, entry, size, mode, twin=False, switch=None):
    """the truth: the same call on a context created for it (under `switch` = (name, value) when given); computed once"""
    key = (entry.name, size, mode, twin, switch)
    if key not in _TRUTH:
        ctx = S.Context(0)
        try:
            if switch:
                ctx.set_tuning(*switch)
            _TRUTH[key] = run(S, entry, size, mode, ctx, twin)
        finally:
            ctx.close()
    return _TRUTH[key]


def same(got, want):
    """do two run() results hold the same words and the same record?  -> "" or what differs"""
    (gw, gr), (ww, wr) = got, want
    if gr != wr:
        return f"dispatch record [{gr}], a fresh context's [{wr}]"
    if len(gw) != len(ww):
        return f"{len(gw)} results, a fresh context gives {len(ww)}"
    for i, (g, w) in enumerate(zip(gw, ww)):
        if g.shape != w.shape:
            return f"result {i}: {g.size} words, a fresh context gives {w.size}"
        bad = np.flatnonzero(g != w)
        if bad.size:
            return f"result {i}: {bad.size} of {g.size} words differ, the first at {int(bad[0])}: {int(g[bad[0]]):#x}, a fresh context's {int(w[bad[0]]):#x}"
    return ""


def leads(record, family):
    """a record may carry helper passes after the families named (poison, edge fix ...): the named ones must lead it"""
    return record == family or (family != "" and record.startswith(family + "+"))


# ---------------------------------------------------------------------------------------------------------------- builders
def _grow(size, small, factor=4):
    return small if size == "small" else small * factor


def _f32(rng, *shape):
    return rng.standard_normal(shape, dtype=np.float32)


def _c64(rng, *shape):
    return (rng.standard_normal(shape, dtype=np.float32) + 1j * rng.standard_normal(shape, dtype=np.float32)).astype(np.complex64)


def _poison(arr, where, values=(np.nan, np.inf, -np.inf)):
    """a copy of arr with non-finite values at the flat positions `where` (fractions of its size)"""
    out = np.array(arr, copy=True)
    flat = out.reshape(-1)
    for i, frac in enumerate(where):
        flat[int(frac * (flat.size - 1))] = values[i % len(values)]
    return out


def _twin(key, where):
    return lambda args: {**args, key: _poison(args[key], where)}


SR = 48000


def _stft_entry(name, N, hop, K, rows, M, family, slots, tables, switch=None, cplx=False, grow="rows", dtype=None, host_slots=None):
    def build(rng, size):
        r = _grow(size, rows) if grow == "rows" else rows
        m = _grow(size, M) if grow == "frames" else M
        L = (m - 1) * hop + N
        x = _c64(rng, r, L) if cplx else _f32(rng, r, L)
        return {"x": x.astype(dtype) if dtype else x}

    def call(S, ctx, a, dev):
        return S.stft(dev(a["x"]), S.windows.hann(N), ctx=ctx, overlap_length=N - hop, fft_length=K, sampling_rate=SR)[0]

    stage = {"kScratchStageIn": "api.cpp:806", "kScratchStageOut": "api.cpp:807"} if host_slots is None else host_slots
    return Entry(name, build, call, family, slots, tables, host_slots=stage, switch=switch)


def _istft_entry(name, N, hop, rows, M, family, slots, tables, twin=None, kind="plain", switch=None, wide=False, host_slots=None):
    """kind: plain / filtered / packed / masked"""
    def build(rng, size):
        r = _grow(size, rows)
        a = {"z": _c64(rng, r, M, N // 2 if kind == "packed" else N)}
        if wide:
            a["z"] = a["z"].astype(np.complex128)
        if kind == "filtered":
            a["h"] = _c64(rng, N)
        if kind == "masked":
            a["mask"] = np.abs(_f32(rng, r, M, N))
        return a

    def call(S, ctx, a, dev):
        w = S.windows.hann(N).astype(np.float64) if wide else S.windows.hann(N)
        o = dict(overlap_length=N - hop, fft_length=N, sampling_rate=SR)
        if kind == "filtered":
            return S.istft_filtered(dev(a["z"]), a["h"], w, ctx=ctx, **o)
        if kind == "packed":
            return S.istft_packed(dev(a["z"]), w, ctx=ctx, **o)
        if kind == "masked":
            return S.istft_masked(dev(a["z"]), dev(a["mask"]), w, ctx=ctx, **o)
        return S.istft(dev(a["z"]), w, ctx=ctx, **o)

    stage = {"kScratchStageIn": "api.cpp:923", "kScratchStageOut": "api.cpp:924"} if host_slots is None else host_slots
    if kind == "masked":
        stage = {**stage, "kScratchNdStageA": "api.cpp:923"}
    return Entry(name, build, call, family, slots, tables, host_slots=stage, twin=twin, switch=switch)


def _fir_entry(name, taps, rows, L, family, slots, tables, twin=None):
    def build(rng, size):
        return {"x": _f32(rng, _grow(size, rows, 3), L), "h": _f32(rng, taps) / np.float32(taps)}

    def call(S, ctx, a, dev):
        return S.filters.fir(dev(a["x"]), a["h"], mode="same", ctx=ctx)

    return Entry(name, build, call, family, slots, tables, host_slots={"kScratchStageIn": "api.cpp:1029", "kScratchStageOut": "api.cpp:1030"}, twin=twin)


def _sink_entry(name, fn, N, hop, K, rows, M, family, slots, tables, twin=None, **kw):
    """mel_spectrogram / spectrogram: the fused sinks of the stft"""
    def build(rng, size):
        return {"x": _f32(rng, _grow(size, rows), (M - 1) * hop + N)}

    def call(S, ctx, a, dev):
        r = getattr(S, fn)(dev(a["x"]), S.windows.hann(N), ctx=ctx, overlap_length=N - hop, fft_length=K, sampling_rate=16000, **kw)
        return r[0] if isinstance(r, tuple) else r

    return Entry(name, build, call, family, slots, tables, host_slots={"kScratchStageIn": "api.cpp:820", "kScratchStageOut": "api.cpp:820"}, twin=twin)


def _fft_nd_entry(name, K, rows, family, slots, tables, switch=None, factor=4):
    def build(rng, size):
        return {"x": _c64(rng, _grow(size, rows, factor), K)}

    def call(S, ctx, a, dev):
        return S.transforms.fft_nd(dev(a["x"]), ctx=ctx, axes=[-1])

    return Entry(name, build, call, family, slots, tables, host_slots={"kScratchNdStageA": "api.cpp:1665", "kScratchNdStageB": "api.cpp:1666"}, switch=switch)


_WAVE_SINK = "kScratchWaveSink"
_ND_STAGE_1 = {"kScratchNdStageA": "api.cpp:1697", "kScratchNdStageOut": "api.cpp:1697"}


def _entries():
    E = []
    # ---- stft, f32 samples
    E.append(_stft_entry("stft1024", 1024, 256, 1024, 1, 184, "stft.pair.1r", {_WAVE_SINK: "wave_stft.hpp:1463"}, ("wave",), switch=("DISABLE_WAVE", 1),
                         grow="frames"))
    E.append(_stft_entry("stft512", 512, 128, 512, 2, 400, "stft.quad2", {_WAVE_SINK: "wave_stft.hpp:1463"}, ("wave", "twQ")))
    E.append(_stft_entry("stft400", 400, 160, 400, 2, 400, "stft.r20", {_WAVE_SINK: "kernels_wave_r20.hip:607"}, ("r20",), switch=("DISABLE_R20", 1)))
    E.append(_stft_entry("stft960", 960, 240, 960, 2, 200, "stft.rab", {_WAVE_SINK: "wave_rab.hpp:1195"}, ("rab",), switch=("DISABLE_RAB", 1)))
    E.append(_stft_entry("stft4096", 4096, 1024, 4096, 2, 100, "stft.real2x.4k", {_WAVE_SINK: "wave_stft.hpp:1463"}, ("wave",)))
    E.append(_stft_entry("stft8192", 8192, 2048, 8192, 2, 50, "stft.8k", {}, ("8k",), switch=("DISABLE_8K", 1)))
    E.append(_stft_entry("stft443-bluestein", 443, 110, 443, 2, 400, "stft.blue", {}, ("bluestein",), switch=("DISABLE_BLUE_WAVE", 1)))
    E.append(_stft_entry("stft5000-long", 5000, 1250, 5000, 1, 4, "stft.big", {"kScratchLongStftFrames": "kernels_nd.hip:1053", "kScratchBluesteinA": "kernels_nd.hip:548",
                                                                                "kScratchBluesteinB": "kernels_nd.hip:549"}, ("bluestein",)))
    E.append(_stft_entry("stft16-c64-generic", 16, 4, 16, 2, 400, "stft_c64.frames", {"kScratchStftC64Frames": "kernels_generic.hip:1520"}, (), cplx=True))
    E.append(_stft_entry("stft512-f64", 512, 128, 512, 1, 40, "", {}, ("f64",), dtype=np.float64,
                         host_slots={"kScratchStageIn": "api.cpp:2195", "kScratchStageOut": "api.cpp:2195"}))
    # ---- istft
    nf = (0.31, 0.62, 0.93)
    E.append(_istft_entry("istft1024", 1024, 256, 2, 400, "istft.wave.deep+istft.edge_chunks", {_WAVE_SINK: "kernels_wave.hip:1245"}, ("wave", "edge-fix")))
    E.append(_istft_entry("istft1024-filtered", 1024, 256, 2, 400, "istft.wave.filt+istft.edge_chunks", {_WAVE_SINK: "kernels_wave.hip:1245"},
                          ("wave", "edge-fix"), kind="filtered", switch=("DISABLE_FUSED_FILTER", 1)))
    E.append(_istft_entry("istft4096", 4096, 1024, 2, 100, "istft.4k", {_WAVE_SINK: "kernels_wave.hip:1398"}, ("wave", "edge-fix"), switch=("DISABLE_4K", 1)))
    E.append(_istft_entry("istft256-quad", 256, 64, 2, 400, "istft.quad", {_WAVE_SINK: "kernels_wave.hip:1351", "kScratchIstftNfList": "kernels_generic.hip:1708"},
                          ("wave", "twQ", "edge-fix"), twin=_twin("z", nf)))
    E.append(_istft_entry("istft512-half", 512, 128, 2, 400, "istft.half.deep+istft.edge_chunks", {"kScratchIstftNfList": "kernels_generic.hip:1708"},
                          ("wave", "edge-fix"), twin=_twin("z", nf)))
    E.append(_istft_entry("istft443-generic", 443, 110, 2, 400, "fft.rows_generic.blue+istft.generic+istft.edge_fix", {"kScratchMultiStage": "kernels_generic.hip:1537"},
                          ("bluestein", "edge-fix")))
    E.append(_istft_entry("istft1024-packed", 1024, 256, 2, 400, "istft.packed", {_WAVE_SINK: "kernels_wave_packed.hip:189"}, ("wave", "edge-fix"),
                          kind="packed", twin=_twin("z", nf)))
    E.append(_istft_entry("istft444-packed-two-step", 444, 111, 2, 100, "fft.rows_generic.blue+istft.generic+istft.edge_fix", {"kScratchPackedSpectrum": "api.cpp:257", "kScratchPackedSignal": "api.cpp:258"},
                          ("edge-fix",), kind="packed"))
    E.append(_istft_entry("istft1024-masked", 1024, 256, 2, 400, "istft.wave.mask", {_WAVE_SINK: "kernels_wave_mask.hip:196"}, ("wave", "edge-fix"),
                          kind="masked", twin=_twin("mask", nf), switch=("DISABLE_FUSED_MASK", 1)))
    E.append(_istft_entry("istft512-masked-two-step", 512, 128, 2, 200, "spectrum_mask", {"kScratchIstftProduct": "api.cpp:271"}, ("wave", "edge-fix"), kind="masked"))
    E.append(_istft_entry("istft512-filtered-two-step", 512, 128, 2, 200, "spectrum_mul", {"kScratchIstftProduct": "api.cpp:281"}, ("wave", "edge-fix"),
                          kind="filtered"))
    E.append(_istft_entry("istft512-c128", 512, 128, 1, 40, "", {"kScratchIstftF64Frames": "kernels_f64.hip:679"}, ("f64",), wide=True,
                          host_slots={"kScratchStageIn": "api.cpp:2260", "kScratchStageOut": "api.cpp:2260"}))
    # ---- fir
    rows = (0.2, 0.7)
    E.append(_fir_entry("fir257", 257, 2, 1 << 20, "fir.pair+fir.pair.edge", {"kScratchFirRowFlags": "kernels_generic.hip:797"}, ("wave", "fir-spectrum"),
                        twin=_twin("x", rows)))
    E.append(_fir_entry("fir4097-delay-line", 4097, 2, 1 << 20, "fir.dline", {"kScratchFirRowFlags": "kernels_generic.hip:797", "kScratchFirLong": "kernels_wave_firlong.hip:380"},
                        ("wave", "fir-delay-line"), twin=_twin("x", rows)))
    E.append(_fir_entry("fir40001-one-transform", 40001, 1, 1 << 18, "fir.long", {"kScratchFirLong": "api.cpp:305", "kScratchConvNdA": "kernels_nd.hip:745",
                                                                                   "kScratchConvNdB": "kernels_nd.hip:746", "kScratchConvNdC": "kernels_nd.hip:747"},
                        ("two-level",)))
    # ---- the fused sinks
    E.append(_sink_entry("mel1024", "mel_spectrogram", 1024, 256, 1024, 2, 200, "mel.pair", {"kScratchReductionCells": "kernels_generic.hip:1945"}, ("wave", "mel-filterbank"),
                         twin=_twin("x", rows), mel_bins=80))
    E.append(_sink_entry("mel16-two-step", "mel_spectrogram", 16, 4, 16, 2, 400, "stft.generic.pow2", {"kScratchFusedSpectrum": "api.cpp:827",
                                                                                                       "kScratchReductionCells": "kernels_generic.hip:1945"},
                         ("mel-filterbank",), mel_bins=4))
    E.append(_sink_entry("dbfs1024", "spectrogram", 1024, 256, 1024, 2, 200, "mag.pair", {"kScratchReductionCells": "kernels_generic.hip:2128"}, ("wave",),
                         twin=_twin("x", rows), kind="dbfs"))
    # ---- Nx.fft rows through fft_nd
    nd = {"kScratchFftNdA": "kernels_nd.hip:623", "kScratchFftNdB": "kernels_nd.hip:624", "kScratchFftNdC": "kernels_nd.hip:625"}
    E.append(_fft_nd_entry("fft1024-rows", 1024, 128, "fft.rows_wave", nd, ("wave",), switch=("DISABLE_WAVE_ROWS", 1)))
    E.append(_fft_nd_entry("fft-2^21-four-step", 1 << 21, 1, "fft.transpose+fft.rows_wave", {**nd, "kScratchFourStepA": "kernels_nd.hip:231", "kScratchFourStepB": "kernels_nd.hip:232"},
                           ("two-level",), factor=3))
    E.append(_fft_nd_entry("fft5000-bluestein", 5000, 4, "fft.big.blue", {**nd, "kScratchBluesteinA": "kernels_nd.hip:548", "kScratchBluesteinB": "kernels_nd.hip:549"},
                           ("bluestein",)))

    # ---- convolution (host tensors only in the Python mirror)
    def conv1(rng, size):
        return {"a": _c64(rng, _grow(size, 3000)), "b": _c64(rng, 500)}

    E.append(Entry("fftconvolve-c64", conv1, lambda S, ctx, a, dev: S.convolution.fftconvolve(a["a"], a["b"], ctx=ctx, mode="full"),
                   {"small": "fft.rows_wave", "large": "fft.tiled"},
                   {"kScratchMultiStage": "kernels_generic.hip:1886"},
                   host_slots={"kScratchStageIn": "api.cpp:2007", "kScratchStageOut": "api.cpp:2007", "kScratchFusedSpectrum": "api.cpp:2008"}, modes=("host",)))

    def conv2(rng, size):
        n = 48 if size == "small" else 96
        return {"a": _f32(rng, n, n), "b": _f32(rng, 9, 9)}

    E.append(Entry("fftconvolve-2d", conv2, lambda S, ctx, a, dev: S.convolution.fftconvolve(a["a"], a["b"], ctx=ctx, mode="same"),
                   "fft.tiled.columns+fft.rows_generic.pow2+fft.transpose+fftconvolve_nd",
                   {"kScratchConvNdA": "kernels_nd.hip:745", "kScratchConvNdB": "kernels_nd.hip:746", "kScratchConvNdC": "kernels_nd.hip:747"},
                   host_slots={"kScratchNdStageA": "api.cpp:1084", "kScratchNdStageB": "api.cpp:1084", "kScratchNdStageOut": "api.cpp:1085"}, modes=("host",)))

    # ---- filters
    def rows2d(r, n):
        return lambda rng, size: {"x": _f32(rng, _grow(size, r), n)}

    E.append(Entry("median-rows", rows2d(8, 4096), lambda S, ctx, a, dev: S.filters.median(dev(a["x"]), ctx=ctx, kernel_shape=(1, 5)), "median.rows", {},
                   host_slots=_ND_STAGE_1, switch=("DISABLE_FILTER_TILES", 1)))
    E.append(Entry("wiener", rows2d(64, 256), lambda S, ctx, a, dev: S.filters.wiener(dev(a["x"]), ctx=ctx, kernel_size=3), "wiener.plane",
                   {"kScratchWienerSums": "kernels_filters.hip:508"}, host_slots={"kScratchNdStageA": "api.cpp:1746", "kScratchNdStageOut": "api.cpp:1746"}))
    E.append(Entry("resample-3-2", rows2d(2, 30000), lambda S, ctx, a, dev: S.filters.resample_poly(dev(a["x"]), 3, 2, ctx=ctx), "resample.poly.lds", {},
                   ("resample-phase",), host_slots={"kScratchStageIn": "api.cpp:1725", "kScratchStageOut": "api.cpp:1726"}, switch=("DISABLE_RESAMPLE_LDS", 1)))
    # ---- peak finding
    peak_stage = {"kScratchNdStageA": "api.cpp:1121", "kScratchNdStageB": "api.cpp:1121", "kScratchNdStageOut": "api.cpp:1121"}
    E.append(Entry("argrelmax-rows", rows2d(8, 4096), lambda S, ctx, a, dev: S.peak_finding.argrelmax(dev(a["x"]), ctx=ctx, axis=1), "peaks.rows",
                   {"kScratchPeakTiles": "kernels_peaks.hip:341"}, host_slots=peak_stage, switch=("DISABLE_PEAK_TILES", 1)))
    E.append(Entry("argrelmin-strided", lambda rng, size: {"x": _f32(rng, _grow(size, 512), 64)},
                   lambda S, ctx, a, dev: S.peak_finding.argrelmin(dev(a["x"]), ctx=ctx, axis=0, order=3), "peaks.strided",
                   {"kScratchPeakTiles": "kernels_peaks.hip:341", "kScratchPeakExtremes": "kernels_peaks.hip:285"}, host_slots=peak_stage))

    # ---- waveforms: two tensor operands
    def duty(rng, size):
        n = _grow(size, 1 << 16)
        return {"t": np.linspace(0, 40, n, dtype=np.float32), "duty": rng.random(n, dtype=np.float32)}

    E.append(Entry("square-duty", duty, lambda S, ctx, a, dev: S.waveforms.square(dev(a["t"]), ctx=ctx, duty=dev(a["duty"])), "waveform.square", {},
                   host_slots={"kScratchNdStageA": "api.cpp:1150", "kScratchNdStageB": "api.cpp:1150", "kScratchNdStageOut": "api.cpp:1151"}))
    return E + _newer_families()


def _golden(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def _held(switch, value, call):
    """`call` with a switch of the context held for its duration: a family that no shape reaches on its own"""
    def held(S, ctx, a, dev):
        ctx.set_tuning(switch, value)
        try:
            return call(S, ctx, a, dev)
        finally:
            ctx.clear_tuning(switch)

    return held


def _rows_entry(name, rows, n, call, family, slots, tables=(), stage=None, twin=None, switch=None, more=None):
    """rows of n f32 samples under "x" (`rows` of them, four times that at "large"); more(rng, rows) adds further arguments.  twin: the
    argument that gets the Inf / NaN (fractions 0.2 and 0.7 of it: inside the first row and inside a later one)"""
    def build(rng, size):
        a = {"x": _f32(rng, _grow(size, rows), n)}
        if more:
            a.update(more(rng, a["x"].shape[0]))
        return a

    return Entry(name, build, call, family, slots, tables, host_slots=stage, twin=_twin(twin, (0.2, 0.7)) if twin else None, switch=switch)


def _newer_families():
    """welch / csd / coherence, sosfilt / sosfiltfilt, lfilter / filtfilt, find_peaks, savgol_filter, hilbert, dct / idct / mfcc: none of them
    took a scratch slot of its own, they moved into the slots of older families (nxsig_internal.h: enum ScratchSlot).  Shapes: the
    smallest their own dispatch tests pin to the family (tests/test_gpu_welch.py, _iir, _lfilter, _find_peaks, _savgol, _hilbert, _dct,
    _resample); no "large" call moves more than 8 MB"""
    E = []
    frames16, spectrum4, product20, long21 = "kScratchLongStftFrames", "kScratchFusedSpectrum", "kScratchIstftProduct", "kScratchFirLong"
    stage_a, stage_b, stage_out = "kScratchNdStageA", "kScratchNdStageB", "kScratchNdStageOut"

    # ---- welch / csd / coherence: row flags, partial sums and (generic) frames in slot 16, the generic spectra in slot 4
    def welch(N, overlap, K):
        return lambda S, ctx, a, dev: S.spectral.welch(dev(a["x"]), S.windows.hann(N), ctx=ctx, overlap_length=overlap, fft_length=K, sampling_rate=48000.0)

    def csd(fn, N, overlap, K, **kw):
        return lambda S, ctx, a, dev: getattr(S.spectral, fn)(dev(a["x"]), dev(a["y"]), S.windows.hann(N), ctx=ctx, overlap_length=overlap, fft_length=K,
                                                              sampling_rate=48000.0, **kw)

    def second(n):
        return lambda rng, rows: {"y": _f32(rng, rows, n)}

    one = {stage_a: "api.cpp:2337", stage_out: "api.cpp:2337"}
    two = {stage_a: "api.cpp:2344", stage_b: "api.cpp:2344", stage_out: "api.cpp:2344"}
    three = {stage_a: "api.cpp:2339", stage_b: "api.cpp:2339", stage_out: "api.cpp:2340"}
    n1k, n2k = 1024 + 36 * 256 + 100, 2048 + 13 * 512 + 5
    E.append(_rows_entry("welch1024-pair", 3, n1k, welch(1024, 768, 1024), "welch.pair", {frames16: "kernels_welch.hip:406"}, ("wave", "window"), one,
                         twin="x", switch=("DISABLE_WELCH_WAVE", 1)))
    E.append(_rows_entry("welch2048-pair", 3, n2k, welch(2048, 1536, 2048), "welch.pair", {frames16: "kernels_welch.hip:406"}, ("wave", "window"), one,
                         twin="x", switch=("DISABLE_WELCH_WAVE", 1)))
    E.append(_rows_entry("welch400-in-512-generic", 3, 400 + 30 * 160, welch(400, 240, 512), "welch.generic",
                         {frames16: "kernels_welch.hip:406", spectrum4: "kernels_welch.hip:351"}, ("window",), one, twin="x"))
    E.append(_rows_entry("csd1024-pair", 3, n1k, csd("csd", 1024, 768, 1024), "csd.pair", {frames16: "kernels_welch.hip:406"}, ("wave", "window"), two,
                         twin="y", switch=("DISABLE_WELCH_WAVE", 1), more=second(n1k)))
    E.append(_rows_entry("csd255-generic-auto", 3, 255 * 9 + 11, csd("csd", 255, 127, 255, return_auto=True), "csd.generic",
                         {frames16: "kernels_welch.hip:406", spectrum4: "kernels_welch.hip:351"}, ("window",), three, twin="y", more=second(255 * 9 + 11)))
    E.append(_rows_entry("coherence1024", 3, n1k, csd("coherence", 1024, 768, 1024), "csd.pair", {frames16: "kernels_welch.hip:406"}, ("wave", "window"), three,
                         twin="x", more=second(n1k)))

    # ---- sosfilt / sosfiltfilt: chunk states, tile states, zi and zf (doubles) in slot 16, the extended rows and the forward result in
    # slot 21.  2 sections: chunks of 32 samples, tiles of 2048; 4 sections: 64 and 4096 (iir_plan.hpp) — and another kernel (SP = 2 / 4)
    sos = _golden("iir_vectors.json")
    sos2, sos4 = np.array(sos["butter4_lp4k"]["sos"], np.float64), np.array(sos["cheby1_8_lp100"]["sos"], np.float64)
    assert sos2.shape == (2, 6) and sos4.shape == (4, 6)
    iir16 = {frames16: "recurrence_scan.hpp:298"}
    E.append(_rows_entry("sosfilt-scan", 2, 2049, lambda S, ctx, a, dev: S.filters.sosfilt(dev(a["x"]), sos2, ctx=ctx), "sosfilt.scan", iir16, ("iir-scan",),
                         {stage_a: "api.cpp:2420", stage_out: "api.cpp:2421"}, twin="x", switch=("DISABLE_SOSFILT_SCAN", 1)))
    E.append(_rows_entry("sosfilt-one-chunk-generic", 2, 32, lambda S, ctx, a, dev: S.filters.sosfilt(dev(a["x"]), sos2, ctx=ctx), "sosfilt.generic", iir16, (),
                         {stage_a: "api.cpp:2420", stage_out: "api.cpp:2421"}))
    E.append(_rows_entry("sosfilt-scan-zi-zf", 2, 4097, lambda S, ctx, a, dev: S.filters.sosfilt(dev(a["x"]), sos4, zi=a["zi"], ctx=ctx), "sosfilt.scan", iir16,
                         ("iir-scan",), {stage_a: "api.cpp:2420", stage_out: "api.cpp:2421"}, twin="x",
                         more=lambda rng, rows: {"zi": 0.1 * rng.standard_normal((4, rows, 2))}))
    E.append(_rows_entry("sosfiltfilt-odd", 2, 4097, lambda S, ctx, a, dev: S.filters.sosfiltfilt(dev(a["x"]), sos4, ctx=ctx, padtype="odd"), "sosfilt.scan",
                         {**iir16, long21: "recurrence_scan.hpp:367"}, ("iir-scan", "iir-zi"), {stage_a: "api.cpp:2449", stage_out: "api.cpp:2450"}, twin="x"))

    # ---- lfilter / filtfilt: the same regions of the same two slots.  Order 2: chunks of 32, tiles of 2048; order 6: 64 and 4096 (NP = 2 / 8)
    ba = _golden("lfilter_vectors.json")
    b2, a2 = (np.array(ba["butter2_lp02"][k], np.float64) for k in "ba")
    b6, a6 = (np.array(ba["ellip6"][k], np.float64) for k in "ba")
    assert ba["butter2_lp02"]["on_scan"] and ba["ellip6"]["on_scan"] and len(a2) == 3 and len(a6) == 7
    lf16 = {frames16: "recurrence_scan.hpp:298"}
    E.append(_rows_entry("lfilter-scan", 2, 2049, lambda S, ctx, a, dev: S.filters.lfilter(dev(a["x"]), b2, a2, ctx=ctx), "lfilter.scan", lf16, ("lfilter-scan",),
                         {stage_a: "api.cpp:2503", stage_out: "api.cpp:2504"}, twin="x", switch=("DISABLE_LFILTER_SCAN", 1)))
    E.append(_rows_entry("lfilter-one-chunk-generic", 2, 32, lambda S, ctx, a, dev: S.filters.lfilter(dev(a["x"]), b2, a2, ctx=ctx), "lfilter.generic", lf16, (),
                         {stage_a: "api.cpp:2503", stage_out: "api.cpp:2504"}))
    E.append(_rows_entry("lfilter-scan-zi-zf", 2, 4097, lambda S, ctx, a, dev: S.filters.lfilter(dev(a["x"]), b6, a6, zi=a["zi"], ctx=ctx), "lfilter.scan", lf16,
                         ("lfilter-scan",), {stage_a: "api.cpp:2503", stage_out: "api.cpp:2504"}, twin="x",
                         more=lambda rng, rows: {"zi": 0.1 * rng.standard_normal((rows, 6))}))
    E.append(_rows_entry("filtfilt-odd", 2, 2049, lambda S, ctx, a, dev: S.filters.filtfilt(dev(a["x"]), b2, a2, ctx=ctx, padtype="odd"), "lfilter.scan",
                         {**lf16, long21: "recurrence_scan.hpp:367"}, ("lfilter-scan", "lfilter-zi"), {stage_a: "api.cpp:2534", stage_out: "api.cpp:2535"},
                         twin="x"))

    # ---- find_peaks: the layouts of slots 29 / 30 differ from argrelextrema's.  Prominence and width, so that the walks run; the generic
    # tier exists under its switch only, so its entry holds the switch for the call (and asks for a distance: the rounds and their flag)
    peaks = {"kScratchPeakTiles": "kernels_find_peaks.hip:421", "kScratchPeakExtremes": "kernels_find_peaks.hip:433"}
    fp_stage = {stage_a: "api.cpp:2576", stage_b: "api.cpp:2576", stage_out: "api.cpp:2576"}
    E.append(_rows_entry("find-peaks-tables", 4, 2048, lambda S, ctx, a, dev: S.peak_finding.find_peaks(dev(a["x"]), ctx=ctx, prominence=0.5, width=1.0),
                         "find_peaks.tables", peaks, (), fp_stage, switch=("DISABLE_FIND_PEAKS_TABLES", 1)))
    E.append(_rows_entry("find-peaks-generic", 4, 2048,
                         _held("DISABLE_FIND_PEAKS_TABLES", 1, lambda S, ctx, a, dev: S.peak_finding.find_peaks(dev(a["x"]), ctx=ctx, prominence=0.5, width=1.0,
                                                                                                                   distance=3)),
                         "find_peaks.generic", peaks, (), fp_stage))

    # ---- savgol_filter: no scratch, two cached tables behind a memo (the weights, the edge fit of mode "interp")
    sg_stage = {stage_a: "api.cpp:2633", stage_out: "api.cpp:2634"}
    E.append(_rows_entry("savgol-tiles", 2, 2048, lambda S, ctx, a, dev: S.filters.savgol_filter(dev(a["x"]), 5, 2, ctx=ctx), "savgol.tiles", {},
                         ("savgol-kernel", "savgol-edge"), sg_stage, switch=("DISABLE_SAVGOL_TILES", 1)))
    E.append(_rows_entry("savgol-short-row-generic", 2, 2047, lambda S, ctx, a, dev: S.filters.savgol_filter(dev(a["x"]), 7, 3, deriv=1, ctx=ctx), "savgol.generic",
                         {}, ("savgol-kernel", "savgol-edge"), sg_stage))

    # ---- hilbert: the generic tier's spectra in slot 4, its row means, dense rows and complex signal in slot 20
    hb_stage = {stage_a: "api.cpp:2659", stage_out: "api.cpp:2660"}
    hb = {spectrum4: "kernels_hilbert.hip:215", product20: "kernels_hilbert.hip:221"}
    E.append(_rows_entry("hilbert1024-wave", 3, 1024, lambda S, ctx, a, dev: S.filters.hilbert(dev(a["x"]), ctx=ctx), "hilbert.wave", {}, ("wave",), hb_stage,
                         switch=("DISABLE_HILBERT_WAVE", 1)))
    E.append(_rows_entry("hilbert1000-generic", 3, 1000, lambda S, ctx, a, dev: S.filters.hilbert(dev(a["x"]), ctx=ctx), "hilbert.generic", hb, (), hb_stage,
                         twin="x"))
    E.append(_rows_entry("hilbert1025-generic-envelope", 3, 1025, lambda S, ctx, a, dev: S.filters.hilbert(dev(a["x"]), ctx=ctx, output="envelope"),
                         "hilbert.generic", hb, (), hb_stage, twin="x"))

    # ---- dct / idct / mfcc: the fft tier's row transform in slot 4, its row means and permuted rows (type 2) or Hermitian spectra (type 3)
    # in slot 20.  mfcc is a fused mel call and a dct call on one context: its record is what the last call notes
    dct_stage = {stage_a: "api.cpp:2684", stage_out: "api.cpp:2685"}
    dct_fft = {spectrum4: "kernels_dct.hip:260", product20: "kernels_dct.hip:263"}
    E.append(_rows_entry("dct80-direct", 3, 80, lambda S, ctx, a, dev: S.transforms.dct(dev(a["x"]), ctx=ctx, norm="ortho"), "dct.direct", {}, ("dct",), dct_stage,
                         switch=("DISABLE_DCT_DIRECT", 1)))
    E.append(_rows_entry("dct400-fft", 3, 400, lambda S, ctx, a, dev: S.transforms.dct(dev(a["x"]), type=2, ctx=ctx), "dct.fft", dct_fft, ("dct",), dct_stage,
                         twin="x"))
    E.append(_rows_entry("idct257-fft", 3, 257, lambda S, ctx, a, dev: S.transforms.idct(dev(a["x"]), type=2, ctx=ctx, norm="ortho"), "dct.fft", dct_fft,
                         ("dct",), dct_stage, twin="x"))
    E.append(_rows_entry("mfcc1024", 2, 39 * 256 + 1024,
                         lambda S, ctx, a, dev: S.mfcc(dev(a["x"]), S.windows.hann(1024), ctx=ctx, n_mfcc=20, overlap_length=768, fft_length=1024,
                                                       sampling_rate=16000, mel_bins=80),
                         "dct.direct", {"kScratchReductionCells": "kernels_generic.hip:1945"}, ("wave", "mel-filterbank", "dct")))

    # ---- the second tier of resample_poly: 20 001 taps are an 80 KB phase table, past the LDS tier
    E.append(_rows_entry("resample-3-2-generic", 2, 3001, lambda S, ctx, a, dev: S.filters.resample_poly(dev(a["x"]), 3, 2, ctx=ctx, taps=a["taps"]),
                         "resample.poly.generic", {}, ("resample-taps",), {"kScratchStageIn": "api.cpp:1725", "kScratchStageOut": "api.cpp:1726"},
                         more=lambda rng, rows: {"taps": _f32(rng, 20001) / np.float32(100)}))

    # ---- call sites of older families that the first catalogue did not reach
    flags = "kScratchFirRowFlags"
    E.append(_rows_entry("fir4097-partitioned", 1, 1 << 18,
                         _held("FIR_DLINE", 0, lambda S, ctx, a, dev: S.filters.fir(dev(a["x"]), a["h"], mode="same", ctx=ctx)), "fir.partitioned",
                         {flags: "kernels_generic.hip:797", long21: "api.cpp:347"}, ("wave", "fir-spectrum"),
                         {"kScratchStageIn": "api.cpp:1029", "kScratchStageOut": "api.cpp:1030"}, twin="x",
                         more=lambda rng, rows: {"h": _f32(rng, 4097) / np.float32(4097)}))
    nd = {"kScratchFftNdA": "kernels_nd.hip:623", "kScratchFftNdB": "kernels_nd.hip:624", "kScratchFftNdC": "kernels_nd.hip:625"}
    E.append(_fft_nd_entry("fft16384-tiled", 16384, 2, "fft.tiled", {**nd, "kScratchFourStepA": "kernels_nd.hip:446"}, ("two-level",)))
    return E


ENTRIES = _entries()
BY_NAME = {e.name: e for e in ENTRIES}


# ---------------------------------------------------------------------------------------------------------------- call sequences
def slot_orders(steps):
    """{slot: set of (size, next size) over the consecutive steps of `steps` that use the slot}"""
    last, seen = {}, {}
    for kind, name, size, mode in steps:
        if kind == "refused":
            continue   # returns before anything is staged or launched
        for slot in BY_NAME[name].slots_of(mode):
            if slot in last:
                seen.setdefault(slot, set()).add((last[slot], size))
            last[slot] = size
    return seen


# Slots whose pairs run between one claimant per source file (the first in catalogue order) instead of between all of them.
# kScratchWaveSink is a write-only dummy target that no kernel reads back, with eleven claimants, most of them the largest calls of the
# catalogue: its 110 pairs measured 14.1 s on an MI355X (the next slowest slot's pairs 1.8 s), the 30 pairs of its six source files 3.5 s
THINNED = ("kScratchWaveSink",)


def slot_users(slot):
    """the entries whose kernel-side claims (Entry.slots) name `slot`, by name in catalogue order; for a THINNED slot one per source file"""
    users = [e for e in ENTRIES if slot in e.slots]
    if slot in THINNED:
        first = {}
        for e in users:
            first.setdefault(e.slots[slot].partition(":")[0], e)
        users = list(first.values())
    return [e.name for e in users]


def user_pairs():
    """{slot: [(A, B), ...]}: for every slot that two or more entries claim on the kernel side (Entry.slots; the staging slots of the
    host mode, host_slots, are claimed by nearly every entry and hold nothing a kernel reads back), every ordered pair of distinct
    claimants, by name.  plan() only guarantees that every SLOT sees a large call before a small one; with several families in one slot it
    is the order of its USERS that decides whose leftovers a kernel could pick up."""
    pairs = {}
    for slot in scratch_slots():
        users = slot_users(slot)
        if len(users) >= 2:
            pairs[slot] = [(a, b) for a in users for b in users if a != b]
    return pairs


def plan(seed, refused=()):
    """The call sequence of one seed on one long-lived context: every (entry, size, mode) twice over in shuffled order, and at seeded
    positions every non-finite twin (both modes), every entry with a dispatch switch under its switch, and the `refused` calls
    ((entry point, case) rows of tests/golden/abi_error_table.json: a broken argument that is refused before any launch).  Steps are
    (kind, name, size, mode), kind one of call / twin / switch / refused.  The shuffle alone does not guarantee that every slot sees a
    large call followed by a small one AND a small one followed by a large one: what is missing is appended."""
    import random

    rng = random.Random(seed)
    combos = [("call", e.name, size, mode) for e in ENTRIES for size in SIZES for mode in e.modes]
    steps = []
    for _ in range(2):
        part = list(combos)
        rng.shuffle(part)
        steps += part
    extras = [("twin", e.name, "small", mode) for e in ENTRIES if e.twin for mode in e.modes]
    extras += [("switch", e.name, "small", rng.choice(e.modes)) for e in ENTRIES if e.switch]
    extras += [("refused", name, label, "host") for name, label in refused]
    for x in extras:
        steps.insert(rng.randrange(len(steps) + 1), x)
    seen = slot_orders(steps)
    for slot in scratch_slots():
        if slot in EXCUSED or {("small", "large"), ("large", "small")} <= seen.get(slot, set()):
            continue
        e, mode = next((e, m) for e in ENTRIES for m in e.modes if slot in e.slots_of(m))
        steps += [("call", e.name, s, mode) for s in ("small", "large", "small")]
    return steps
