"""What a context carries from one call to the next.

The rest of the GPU suite checks one call at a time, most of it on a context made for that call.  A context in real use lives for
hours, is called from several threads, and keeps scratch slots, cached tables with pointer caches in front of them, recycled result
blocks and pinned staging slots between calls.  Here the calls of tests/context_calls.py run on contexts that have a history, and
every result must be the words and the dispatch record a context created for that one call gives (context_calls.fresh):

  * seeded sequences of every (entry, size, mode) on one context, with refused calls, non-finite twins and dispatch switches between;
  * every user of a shared scratch slot behind every other user of it (context_calls.user_pairs);
  * the trim of the table cache (NXSIG_TABLE_CACHE_MAX lowered, the default bound crossed for real, a trim inside a sharded call);
  * four threads on one context;
  * host staging of two large operands and of more than two chunks, under NXSIG_HOST_PIPE = 0 / 1 / 3;
  * the dispatch record of a group member after the sharded calls.

The oracle is not consulted: the rest of the suite ties fresh-context results to it, and the expected family of every entry is
asserted, so a wrong catalogue entry shows at once."""
import ctypes as C
import json
import os
import sys
import threading

import numpy as np
import pytest

import context_calls as CC
import nx_signal_amd as S
from nx_signal_amd import _lib, sharding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402

pytestmark = pytest.mark.gpu

with open(P.GOLDEN) as f:
    GOLDEN = json.load(f)["real_ctx"]
PROBE_ENTRIES = {name: (args, listed) for name, args, listed in P.ENTRIES}
# refused calls: rows of the recorded error table whose broken argument is refused before any launch, one of each kind of entry point
REFUSED = [("nxsig_stft_f32", "hop=0"), ("nxsig_istft_c64", "hop>frame_length"), ("nxsig_fir_f32", "mode=9"), ("nxsig_fft", "fft_length=0"),
           ("nxsig_stft_mel_f32", "mel_bins=0"), ("nxsig_istft_masked_c64", "mask_kind=9"), ("nxsig_fftconvolve_c64", "n2=0"),
           ("nxsig_median_filter", "kernel_shape>dimension"), ("nxsig_argrelextrema", "axis=1"), ("nxsig_fir_slice_f32", "slice past the end"),
           ("nxsig_istft_packed_f32", "fft_length=7"), ("nxsig_square", "n=-1")]


def _refuse(ctx, name, label):
    """one broken call of the error table on `ctx`: refused with the recorded code and message"""
    args, listed = PROBE_ENTRIES[name]
    broken = next(c[1] for c in P._cases(args, listed) if c[0] == label)
    rec, _ = P.Probe(_lib.load(), ctx.handle).call(name, args, broken, _lib.HOST)
    assert rec["rc"] != 0 and rec == GOLDEN[name][label], (name, label, rec)
    with pytest.raises(_lib.ArgumentError):   # what the Python mirror makes of that return code
        _lib.check(rec["rc"])


def _step(ctx, step):
    """runs one step of a plan on ctx -> "" or what differs from the fresh-context truth"""
    kind, name, size, mode = step
    if kind == "refused":
        _refuse(ctx, name, size)
        return ""
    e = CC.BY_NAME[name]
    if kind == "switch":
        ctx.set_tuning(*e.switch)
        try:
            got = CC.run(S, e, size, mode, ctx)
        finally:
            ctx.clear_tuning(e.switch[0])
        return CC.same(got, CC.fresh(S, e, size, mode, switch=e.switch))
    got = CC.run(S, e, size, mode, ctx, twin=kind == "twin")
    if ctx.last_dispatch() != got[1]:
        return f"the context's record [{ctx.last_dispatch()}] is not the thread's [{got[1]}]"
    return CC.same(got, CC.fresh(S, e, size, mode, twin=kind == "twin"))


# ------------------------------------------------------------------------------------------------ 1. the catalogue itself
@pytest.mark.parametrize("name", [e.name for e in CC.ENTRIES])
def test_an_entry_runs_on_its_family_and_is_bit_stable_from_context_to_context(name):
    e = CC.BY_NAME[name]
    for size in CC.SIZES:
        for mode in e.modes:
            words, rec = CC.fresh(S, e, size, mode)
            assert CC.leads(rec, e.family_of(size)), f"{name} {size} {mode}: dispatched to [{rec}], the catalogue says [{e.family_of(size)}]"
            ctx = S.Context(0)
            again = CC.run(S, e, size, mode, ctx)
            ctx.close()
            assert CC.same(again, (words, rec)) == "", f"{name} {size} {mode}: two fresh contexts disagree: {CC.same(again, (words, rec))}"
    if e.twin:
        for mode in e.modes:
            twin, plain = CC.fresh(S, e, "small", mode, twin=True), CC.fresh(S, e, "small", mode)
            assert CC.same(twin, plain) != "", f"{name}: the non-finite twin gives the plain result"
    if e.switch:
        assert CC.fresh(S, e, "small", e.modes[-1], switch=e.switch)[1] != CC.fresh(S, e, "small", e.modes[-1])[1], (name, e.switch)


# ------------------------------------------------------------------------------------------------ 2. seeded sequences
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_long_lived_context_gives_what_a_fresh_one_gives(seed):
    steps = CC.plan(seed, REFUSED)
    seen = CC.slot_orders(steps)
    for slot in CC.scratch_slots():   # large-then-small and small-then-large for every slot: asserted on the sequence that runs
        assert slot in CC.EXCUSED or {("small", "large"), ("large", "small")} <= seen[slot], slot
    ctx = S.Context(0)
    for at, step in enumerate(steps):
        diff = _step(ctx, step)
        assert diff == "", (f"seed {seed}, position {at}, {step}: {diff}\nthe ten calls before it (replay: run these and the step on one "
                            f"new context):\n" + "\n".join(f"  {s}" for s in steps[max(0, at - 10):at]))
    ctx.close()


# ------------------------------------------------------------------------------------------------ 2b. the users of a shared slot
def _pair(ctx, a, b, mode):
    """A at "large", A's non-finite twin (A again where it has none), then B at "small", on ctx -> "" or how B differs from a fresh context"""
    A, B = CC.BY_NAME[a], CC.BY_NAME[b]
    mode_a = mode if mode in A.modes else A.modes[0]
    CC.run(S, A, "large", mode_a, ctx)
    CC.run(S, A, "large", mode_a, ctx, twin=bool(A.twin))
    return CC.same(CC.run(S, B, "small", mode, ctx), CC.fresh(S, B, "small", mode))


@pytest.mark.parametrize("slot", sorted(CC.user_pairs()))
def test_every_user_of_a_shared_slot_after_every_other(slot):
    """Several families live in one scratch slot, with layouts of their own (nxsig_internal.h: "Two users of one slot ... overwrite each
    other silently").  A kernel that reads past what its own call wrote, or counts on the slot being zero, picks up the user before it:
    every ordered pair (A, B) of the slot's claimants (context_calls.THINNED: one claimant per source file) on one long-lived context,
    B's words and record against a fresh context's"""
    ctx = S.Context(0)
    done = []
    for a, b in CC.user_pairs()[slot]:
        for mode in CC.MODES[::-1]:   # device mode, then host mode where B has it
            if mode not in CC.BY_NAME[b].modes:
                continue
            diff = _pair(ctx, a, b, mode)
            if diff:
                new = S.Context(0)   # do the three calls alone show it, or does it take the pairs before them?
                alone = _pair(new, a, b, mode)
                new.close()
                replay = ("these three calls on a new context replay it" if alone else
                          f"these three calls on a new context do NOT replay it; the pairs before them on this context: {done[-6:]}")
                raise AssertionError(f"{slot}: {b} (small, {mode}) after {a} (large, then its {'twin' if CC.BY_NAME[a].twin else 'repeat'}): {diff}\n{replay}")
            done.append((a, b, mode))
    ctx.close()


# ------------------------------------------------------------------------------------------------ 3. the table-cache trim
SR = 48000


def _flood(ctx, windows, first=0):
    """`windows` distinct 8-point windows through stft: two cached tables each (the window and its fft_length form)"""
    x = np.arange(32, dtype=np.float32)
    for i in range(first, first + windows):
        w = (0.5 + np.arange(8, dtype=np.float32) / 16 + np.float32(i) / 4096).astype(np.float32)
        S.stft(x, w, ctx=ctx, overlap_length=4, fft_length=8, sampling_rate=SR)


def _small_entries_equal_fresh(ctx, when):
    for e in CC.ENTRIES:
        for mode in e.modes:
            diff = CC.same(CC.run(S, e, "small", mode, ctx), CC.fresh(S, e, "small", mode))
            assert diff == "", f"{e.name} {mode} {when}: {diff}"


def test_the_trim_forgets_every_pointer_into_the_table_cache():
    """NXSIG_TABLE_CACHE_MAX lowered to 24 tables: the catalogue's small entries fill the table cache and every pointer cache in front
    of it (wave_tables, f64_tables, the window memo, `memo`), four times the bound in distinct windows cross it — the next API entry
    frees every table — and the same entries must give the fresh-context words again, from rebuilt tables"""
    ctx = S.Context(0)
    ctx.set_tuning("TABLE_CACHE_MAX", 24)
    assert ctx.get_tuning("NXSIG_TABLE_CACHE_MAX") == (24, True)
    _small_entries_equal_fresh(ctx, "before the flood")   # with a bound of 24 this alone trims several times between entries
    _flood(ctx, 4 * 24)
    _small_entries_equal_fresh(ctx, "after the flood")
    for bad in (0, -1, (1 << 20) + 1):
        with pytest.raises(_lib.ArgumentError):
            ctx.set_tuning("TABLE_CACHE_MAX", bad)
    ctx.close()


def test_the_trim_at_the_default_bound():
    """the real thing once: 520 distinct windows are 1040 tables, more than the 1024 a context keeps"""
    ctx = S.Context(0)
    assert ctx.get_tuning("TABLE_CACHE_MAX") == (0, False)
    _small_entries_equal_fresh(ctx, "before the flood")
    _flood(ctx, 520)
    _small_entries_equal_fresh(ctx, "after the flood")
    ctx.close()


def test_a_trim_in_the_middle_of_a_sharded_call():
    """the sharded entry points call public entry points per member, each of which may trim: with a bound of 4 tables every compute call
    of a member leaves more than the bound behind, so the member's next entry (the download, the next call) trims"""
    g = sharding.Group.local(2, devices=[0, 0])
    for c in g.contexts:
        c.set_tuning("TABLE_CACHE_MAX", 4)
    _flood(g.contexts[0], 16)   # one member through its own context
    rng = np.random.Generator(np.random.PCG64(41))
    x = rng.standard_normal((4, 40000), dtype=np.float32)
    w = S.windows.hann(1024)
    o = dict(overlap_length=768, fft_length=1024, sampling_rate=16000)
    h = S.filters.firwin(257, [4000.0], sampling_rate=48000.0)
    calls = {
        "stft": lambda grp, axis: sharding.stft_sharded(grp, x, w, axis=axis, **o),
        "fir": lambda grp, axis: sharding.fir_sharded(grp, x, h, mode="same", axis=axis),
        "mel": lambda grp, axis: sharding.mel_spectrogram_sharded(grp, x, w, axis=axis, mel_bins=80, **o),
    }
    # channel shards equal the unsharded call bit for bit (tests/test_gpu_group.py); frame / sample shards pair frames differently at the
    # shard edge, so their truth is the same sharded call on a group nothing has happened to — and that group's distance from the
    # unsharded call is what tests/test_gpu_group.py allows
    one = S.Context(0)
    plain = {"stft": S.stft(x, w, ctx=one, **o)[0], "fir": S.filters.fir(x, h, mode="same", ctx=one), "mel": S.mel_spectrogram(x, w, ctx=one, mel_bins=80, **o)}
    one.close()
    quiet = sharding.Group.local(2, devices=[0, 0])
    want = {(name, "channels"): plain[name] for name in calls}
    for name, call in calls.items():
        want[(name, "frames")] = call(quiet, "frames")
        err = float(np.max(np.abs(want[(name, "frames")] - plain[name])))
        assert err < (2e-5 if name == "mel" else 1e-6 * float(np.max(np.abs(plain[name])))), (name, err)
    quiet.close()
    for axis in ("channels", "frames"):
        for _ in range(2):   # the second round starts from what the first left in the members
            for name, call in calls.items():
                assert np.array_equal(CC.bits(call(g, axis)), CC.bits(want[(name, axis)])), (name, axis)
            _flood(g.contexts[1], 4, first=100)
    g.close()


# ------------------------------------------------------------------------------------------------ 4. one context, several threads
THREADED = ("stft1024", "stft512", "stft400", "istft1024", "istft512-half", "istft1024-masked", "fir257", "mel1024", "dbfs1024", "median-rows",
            "resample-3-2", "fft1024-rows",
            # users of slots 4, 16 and 20 that came later: they share those slots with each other under the context's mutex
            "welch400-in-512-generic", "sosfilt-scan", "lfilter-scan-zi-zf", "hilbert1000-generic", "dct400-fft")


def test_four_threads_on_one_context():
    """DESIGN.md promises a mutex per context (dirty schedulers may call concurrently): every thread runs its own order of the
    THREADED entries, host and device mode, and checks its own results and its own (thread-local) record"""
    want = {(n, m): CC.fresh(S, CC.BY_NAME[n], "small", m) for n in THREADED for m in CC.MODES}   # computed before the threads start
    ctx = S.Context(0)
    failures = []

    def work(t):
        import random
        order = [(n, m) for n in THREADED for m in CC.MODES]
        random.Random(100 + t).shuffle(order)
        try:
            for n, m in order:
                diff = CC.same(CC.run(S, CC.BY_NAME[n], "small", m, ctx), want[(n, m)])
                if diff:
                    failures.append(f"thread {t}, {n} {m}: {diff}")
        except Exception as ex:   # noqa: BLE001 (reported by the main thread)
            failures.append(f"thread {t}: {type(ex).__name__}: {ex}")

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not failures, "\n".join(failures[:8])
    ctx.close()


# ------------------------------------------------------------------------------------------------ 5. host staging
PIPES = (0, 1, 3)


def _under_every_host_path(call_host, want, what):
    """call_host(ctx) on one context under the default path, NXSIG_HOST_PIPE = 1 and = 3: the device-resident call's words every time"""
    ctx = S.Context(0)
    for knob in PIPES:
        if knob:
            ctx.set_tuning("HOST_PIPE", knob)
        for rep in range(2):   # the second call finds the pinned slots and their events as the first left them
            got = call_host(ctx)
            diff = CC.same(([CC.bits(g) for g in CC._flat(got)], ""), (want, ""))
            assert diff == "", f"{what}: HOST_PIPE={knob}, call {rep}: {diff} (the device-resident call's)"
    ctx.close()


def _device_truth(call_dev):
    ctx = S.Context(0)
    res = CC._flat(call_dev(ctx))
    ctx.sync()
    out = [CC.bits(r.numpy()) for r in res]
    ctx.close()
    return out


def test_two_large_host_operands_of_one_call():
    """the slot-reuse case: the second host operand of a call used to be copied into the pinned slot the first operand's DMA was still
    reading (every Staged::in started at chunk 0 and only waited from chunk 2 on)"""
    rng = np.random.Generator(np.random.PCG64(51))
    w = S.windows.hann(1024)
    o = dict(overlap_length=768, sampling_rate=16000)
    z = CC._c64(rng, 4, 640, 1024)            # 20 MB: one chunk
    m = CC._c64(rng, 4, 640, 1024)            # a c64 mask the size of the spectrum
    want = _device_truth(lambda c: S.istft_masked(c.to_device(z), c.to_device(m), w, ctx=c, **o))
    _under_every_host_path(lambda c: S.istft_masked(z, m, w, ctx=c, **o), want, "istft_masked")
    want = _device_truth(lambda c: S.spectrum_mask(c.to_device(z), c.to_device(m), ctx=c))
    _under_every_host_path(lambda c: S.spectrum_mask(z, m, ctx=c), want, "spectrum_mask")
    del z, m
    t = np.linspace(0, 4000, 6 << 20, dtype=np.float32)     # 24 MB + 24 MB
    d = rng.random(6 << 20, dtype=np.float32)
    want = _device_truth(lambda c: S.waveforms.square(c.to_device(t), ctx=c, duty=c.to_device(d)))
    _under_every_host_path(lambda c: S.waveforms.square(t, ctx=c, duty=d), want, "square")


def test_fftconvolve_of_two_large_host_vectors():
    rng = np.random.Generator(np.random.PCG64(52))
    a, b = CC._c64(rng, 1 << 21), CC._c64(rng, 1 << 20)     # 16 MB and 8 MB
    n_out = a.size + b.size - 1
    lib = _lib.load()

    def dev(c):   # the Python mirror takes host tensors here: the device-resident call goes through the C ABI
        ad, bd, out = c.to_device(a), c.to_device(b), c.empty((n_out,), np.complex64)
        _lib.check(lib.nxsig_fftconvolve_c64(c.handle, C.c_void_p(ad.ptr), a.size, C.c_void_p(bd.ptr), b.size, _lib.CONV_FULL, C.c_void_p(out.ptr),
                                             _lib.DEVICE))
        return out

    want = _device_truth(dev)
    _under_every_host_path(lambda c: S.convolution.fftconvolve(a, b, ctx=c, mode="full"), want, "fftconvolve")


@pytest.mark.parametrize("n", [17000003, 8 << 20, (8 << 20) + 1], ids=["68MB-three-chunks", "32MiB", "32MiB+4"])
def test_host_operands_of_several_chunks_and_at_the_chunk_boundary(n):
    """68 MB of f32 end inside the third 32 MiB chunk (the k >= 2 event wait of the upload, and a download as long); exactly one chunk;
    one chunk and four bytes"""
    rng = np.random.Generator(np.random.PCG64(53))
    x = rng.standard_normal(n, dtype=np.float32)
    h = S.filters.firwin(33, [4000.0], sampling_rate=48000.0)
    want = _device_truth(lambda c: S.filters.fir(c.to_device(x), h, mode="same", ctx=c))
    _under_every_host_path(lambda c: S.filters.fir(x, h, mode="same", ctx=c), want, f"fir of {n} samples")


# ------------------------------------------------------------------------------------------------ 6. the record of a group member
def test_a_members_dispatch_record_names_what_its_shard_ran_on():
    g = sharding.Group.local(2, devices=[0, 0])
    rng = np.random.Generator(np.random.PCG64(61))
    x = rng.standard_normal((2, 60000), dtype=np.float32)
    w = S.windows.hann(1024)
    o = dict(overlap_length=768, fft_length=1024, sampling_rate=16000)
    h = S.filters.firwin(257, [4000.0], sampling_rate=48000.0)
    z = S.stft(x, w, **o)[0]

    def something_else(name):
        """a plain call of another kind on every member: what a stale record would name afterwards"""
        for c in g.contexts:
            if name == "fir":
                S.stft(x[0], w, ctx=c, **o)
                assert c.last_dispatch().startswith("stft."), c.last_dispatch()
            else:
                S.filters.fir(x[0], h, mode="same", ctx=c)
                assert c.last_dispatch().startswith("fir."), c.last_dispatch()

    def names(c, prefix):
        return any(f.startswith(prefix) for f in c.last_dispatch().split("+"))

    calls = {
        "stft": (lambda d, axis: sharding.stft_sharded(g, d, w, axis=axis, **o), x, "stft."),
        "fir": (lambda d, axis: sharding.fir_sharded(g, d, h, mode="same", axis=axis), x, "fir."),
        "istft": (lambda d, axis: sharding.istft_sharded(g, d, w, axis=axis, overlap_length=768, sampling_rate=16000), z, "istft."),
        "mel": (lambda d, axis: sharding.mel_spectrogram_sharded(g, d, w, axis=axis, mel_bins=80, **o), x, "mel."),
    }
    for name, (call, data, prefix) in calls.items():
        for axis in ("channels", "frames"):
            something_else(name)
            call(data, axis)
            for i, c in enumerate(g.contexts):
                assert names(c, prefix), f"{name}_sharded over {axis}: member {i} reads [{c.last_dispatch()}]"
        # one row over two members by channels: member 1 has no part, and its record says so instead of naming the call before
        something_else(name)
        call(data[:1], "channels")
        assert names(g.contexts[0], prefix), (name, g.contexts[0].last_dispatch())
        assert g.contexts[1].last_dispatch() == "", f"{name}_sharded: the member without a part reads [{g.contexts[1].last_dispatch()}]"
    g.close()
