"""What the compiler emits for the streaming loop of the headline STFT kernel (pair front-end, fft_length 1024, spectrum sink:
DESIGN.md 3.1), read off the gfx950 assembly of that one instantiation.  No GPU: hipcc cross-compiles a translation unit that holds
nothing but `k_stft_wave<1024, kModePair, false, false, 4, 2, false, 0, 1, true>`: the headline launch's kernel (HOP4, what a
hop = fft_length / 4 call in the four-wave geometry runs), in a few seconds.

Asserted for the loop:
  1. between the first spectrum store of a unit and the next unit's loads, or the way out of the loop, there is no
     `s_waitcnt vmcnt(N)` with N below the 16 stores just issued: the stores stay in flight across the next unit's butterflies;
  2. the hop-specialised instantiation issues at most 20 sample loads per frame pair (frame B reuses 12 of frame A's 16 registers);
  3. no loads are issued for a unit past the wave's last: the last unit is a straight-line copy of the body without any load;
  4. no table-preload loop with a `vmcnt(0)` per trip in front of the workgroup barrier: every table load of a thread is in flight
     before the first wait;
  5. at most 168 VGPRs, no scratch, three waves per SIMD.

The same checks run on the source as it was before this loop was rebuilt (`k_stft_wave<1024, kModePair, false, false, 4, 2, false, 0, 1>`,
then the headline's kernel and today still the kernel of every other hop) fail on
the first four: `vmcnt(1)` behind the 16 stores and `vmcnt(0)` at the latch; 32 loads per pair; the last unit re-loads itself inside
the one loop and no peeled copy exists; four table loops of load / `vmcnt(0)` / `ds_write` per trip.  The fifth held there too
(168 VGPRs, no scratch, occupancy 3)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nx_signal_amd", "csrc")
STORES_PER_UNIT = 16   # buffer_store_dwordx4 of one frame pair: 2 frames x 1024 bins x 8 bytes / (64 lanes x 16 bytes)

TU = """#include "wave_stft.hpp"
template __global__ void nxsig::k_stft_wave<1024, nxsig::kModePair, false, false, 4, 2, false, 0, 1, %s>(nxsig::WaveArgs);
"""


def kernel_asm(tmp, hop4):
    from nx_signal_amd import build as B

    src = os.path.join(tmp, "headline_%d.hip" % hop4)
    out = os.path.join(tmp, "headline_%d.s" % hop4)
    with open(src, "w") as f:
        f.write(TU % ("true" if hop4 else "false"))
    subprocess.run([B.hipcc(), f"--offload-arch={B.ARCH}", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I", CSRC, src, "-o", out],
                   check=True, capture_output=True, timeout=300)
    with open(out) as f:
        return f.read()


class Kernel:
    """the instruction stream of k_stft_wave in layout order, with labels, plus the resource lines the assembler prints behind it"""

    def __init__(self, text):
        m = re.search(r"^_ZN5nxsig11k_stft_wave\w+:[^\n]*\n(.*?)\n\.Lfunc_end\d+:", text, re.S | re.M)
        assert m, "k_stft_wave not found in the assembly"
        body = m.group(1)
        tail = text[m.end(): m.end() + 4000]
        self.ins = []          # (kind, text): kind in label / load / tload / bst / wait / branch / barrier / dsw / end / other
        self.label_at = {}
        for ln in body.split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln:
                continue
            lm = re.match(r"^(\.LBB\d+_\d+):", ln)
            if lm:
                self.label_at[lm.group(1)] = len(self.ins)
                self.ins.append(("label", lm.group(1)))
                continue
            if ln.startswith("."):
                continue
            op = ln.split()[0]
            if op == "global_load_dword":
                kind = "load"                      # one sample per lane
            elif op.startswith(("global_load", "buffer_load", "flat_load")):
                kind = "tload"                     # anything wider: tables
            elif op == "buffer_store_dwordx4":
                kind = "bst"
            elif op == "s_waitcnt" and "vmcnt" in ln:
                kind = "wait"
            elif op.startswith("s_cbranch") or op == "s_branch":
                kind = "branch"
            elif op == "s_barrier":
                kind = "barrier"
            elif op.startswith("ds_write"):
                kind = "dsw"
            elif op == "s_endpgm":
                kind = "end"
            else:
                kind = "other"
            self.ins.append((kind, ln))
        self.vgprs = int(re.search(r"; NumVgprs: (\d+)", tail).group(1))
        self.scratch = int(re.search(r"; ScratchSize: (\d+)", tail).group(1))
        self.occupancy = int(re.search(r"; Occupancy: (\d+)", tail).group(1))
        self.code_bytes = int(re.search(r"; codeLenInByte = (\d+)", tail).group(1))

    def loops(self):
        """(first, last) instruction index of every back edge's span"""
        out = []
        for i, (kind, ln) in enumerate(self.ins):
            if kind == "branch":
                t = self.label_at.get(ln.split()[-1])
                if t is not None and t <= i:
                    out.append((t, i))
        return out

    def kinds(self, lo, hi):
        return [k for k, _ in self.ins[lo:hi + 1]]

    def streaming_loop(self):
        """the widest back-edge span that holds sample loads and spectrum stores"""
        spans = [(a, b) for a, b in self.loops() if "load" in self.kinds(a, b) and "bst" in self.kinds(a, b)]
        assert spans, "no loop with sample loads and spectrum stores"
        a = min(s[0] for s in spans)
        return a, max(s[1] for s in spans if s[0] == a)


def vmcnt(ln):
    return int(re.search(r"vmcnt\((\d+)\)", ln).group(1))


def low_waits_after_first_store(seq):
    """waits below the unit's own stores, from the first spectrum store of `seq` on"""
    kinds = [k for k, _ in seq]
    if "bst" not in kinds:
        return []
    first = kinds.index("bst")
    return [ln for k, ln in seq[first:] if k == "wait" and vmcnt(ln) < STORES_PER_UNIT]


def check_stores_stay_in_flight(k):
    a, b = k.streaming_loop()
    loop = k.ins[a:b + 1]
    # one trip in execution order: the loop is laid out rotated (latch first), so start at the first sample load and wrap around
    first_load = [kind for kind, _ in loop].index("load")
    trip = loop[first_load:] + loop[:first_load]
    assert sum(1 for kind, _ in trip if kind == "bst") >= STORES_PER_UNIT
    low = low_waits_after_first_store(trip)
    assert not low, ("the loop drains a unit's stores before the next unit's loads", low)
    # the way out of the loop: up to the next sample load (the cold solo route) or the end of the kernel
    rest = []
    for kind, ln in k.ins[b + 1:]:
        if kind in ("load", "end"):
            break
        rest.append((kind, ln))
    low = low_waits_after_first_store(rest)
    assert not low, ("the last unit's stores are drained", low)


def check_loads_per_pair(k, most):
    a, b = k.streaming_loop()
    in_loop = k.kinds(a, b).count("load")
    before = k.kinds(0, a - 1).count("load")
    assert 0 < in_loop <= most, in_loop
    assert 0 < before <= most, before       # the first unit, loaded ahead of the loop


def check_last_unit_is_peeled(k):
    a, b = k.streaming_loop()
    assert k.kinds(a, b).count("load") <= 32, "more than one unit's loads inside the loop"
    # behind the loop: the last unit's transform and its 16 stores, reached without a single load
    n_bst = 0
    for kind, _ in k.ins[b + 1:]:
        if kind in ("load", "tload", "end"):
            break
        n_bst += kind == "bst"
    assert n_bst >= STORES_PER_UNIT, ("no load-free copy of the body for the wave's last unit", n_bst)


def check_table_preload(k):
    kinds = [kind for kind, _ in k.ins]
    bar = kinds.index("barrier")
    assert "tload" in kinds[:bar] or "load" in kinds[:bar]
    for a, b in k.loops():
        if b < bar:
            waits0 = [ln for kind, ln in k.ins[a:b + 1] if kind == "wait" and vmcnt(ln) == 0]
            assert not waits0, ("a preload loop waits for every trip's load", k.ins[a][1])
    # one round trip: every table load of the thread is issued before the first table wait
    first_wait = next(i for i, kind in enumerate(kinds[:bar]) if kind == "wait")
    assert not any(kind == "tload" for kind in kinds[first_wait:bar])


def check_resources(k):
    assert k.vgprs <= 168 and k.scratch == 0 and k.occupancy == 3, (k.vgprs, k.scratch, k.occupancy)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("isa"))
    return {True: Kernel(kernel_asm(tmp, True))}


def test_a_units_stores_stay_in_flight_until_the_next_units_loads(kernels, hop4=True):
    check_stores_stay_in_flight(kernels[hop4])


def test_hop_specialised_kernel_issues_at_most_20_sample_loads_per_frame_pair(kernels):
    check_loads_per_pair(kernels[True], 20)


def test_no_loads_for_a_unit_past_the_waves_last(kernels, hop4=True):
    check_last_unit_is_peeled(kernels[hop4])


def test_table_preload_is_one_round_trip(kernels, hop4=True):
    check_table_preload(kernels[hop4])


def test_registers_scratch_occupancy(kernels, hop4=True):
    k = kernels[hop4]
    print("VGPRs", k.vgprs, "scratch", k.scratch, "occupancy", k.occupancy, ".text bytes", k.code_bytes)
    check_resources(k)
