"""The call catalogue of tests/context_calls.py against the sources, without a GPU: every scratch slot of a context is claimed by an
entry (or excused with a reason), every claim cites the line that takes the slot, every kind of cached table appears, and the builders
are deterministic."""
import os

import numpy as np
import pytest

import context_calls as CC


def test_every_scratch_slot_is_claimed_or_excused():
    slots = CC.scratch_slots()
    assert len(slots) == 32 and slots[0] == "kScratchMultiStage" and slots[-1] == "kScratchSlots", slots   # 31 slots + the count
    claimed = {s for e in CC.ENTRIES for mode in e.modes for s in e.slots_of(mode)}
    gone = sorted((claimed | set(CC.EXCUSED)) - set(slots))
    assert not gone, f"claimed or excused, but no longer in enum ScratchSlot: {gone}"
    both = sorted(claimed & set(CC.EXCUSED))
    assert not both, f"claimed AND excused: {both}"
    missing = [s for s in slots if s not in claimed and s not in CC.EXCUSED]
    assert not missing, f"no catalogue entry uses {missing}: add one, or excuse the slot with a reason"
    assert all(reason.strip() for reason in CC.EXCUSED.values())


def _claims():
    return [(e.name, slot, cite) for e in CC.ENTRIES for slot, cite in {**e.slots, **e.host_slots}.items()]


@pytest.mark.parametrize("entry,slot,cite", _claims(), ids=[f"{n}-{s}" for n, s, _ in _claims()])
def test_a_claim_cites_a_line_that_takes_the_slot(entry, slot, cite):
    path, _, line = cite.partition(":")
    with open(os.path.join(CC.CSRC, path)) as f:
        text = f.read().splitlines()[int(line) - 1]
    assert slot in text, f"{entry}: {cite} reads [{text.strip()}], which does not name {slot}"


def test_every_kind_of_cached_table_appears():
    used = {t for e in CC.ENTRIES for t in e.tables}
    assert used <= set(CC.TABLE_KINDS), sorted(used - set(CC.TABLE_KINDS))
    assert not set(CC.TABLE_KINDS) - used, f"no entry builds {sorted(set(CC.TABLE_KINDS) - used)}"


def test_the_entries_with_non_finite_state_carry_a_twin():
    twins = {e.name for e in CC.ENTRIES if e.twin}
    # FIR row flags in both forms, a frame-packing istft, the packed istft, log-mel, dBFS, the masked istft
    assert {"fir257", "fir4097-delay-line", "istft512-half", "istft1024-packed", "mel1024", "dbfs1024", "istft1024-masked"} <= twins
    for e in CC.ENTRIES:
        if not e.twin:
            continue
        plain, twin = e.inputs("small"), e.inputs("small", twin=True)
        assert all(np.isfinite(v).all() for v in plain.values()), e.name
        assert any(not np.isfinite(v).all() for v in twin.values()), e.name
        assert plain.keys() == twin.keys() and all(plain[k].shape == twin[k].shape for k in plain), e.name


def test_names_are_unique_and_there_are_enough_entries():
    assert len(CC.BY_NAME) == len(CC.ENTRIES) >= 25
    for e in CC.ENTRIES:
        assert e.modes in (("host", "device"), ("host",)), e.name
        assert all(e.family_of(s) or "f64" in e.tables for s in CC.SIZES), e.name


@pytest.mark.parametrize("name", [e.name for e in CC.ENTRIES])
def test_builders_are_deterministic_and_the_two_sizes_differ(name):
    e = CC.BY_NAME[name]
    for size in CC.SIZES:
        a, b = e.inputs(size), e.inputs(size)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] is not b[k] and a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
            assert np.array_equal(CC.bits(a[k]), CC.bits(b[k])), (name, size, k)
    small, large = e.inputs("small"), e.inputs("large")
    grown = [k for k in small if large[k].shape != small[k].shape]
    assert grown, name
    ratio = sum(large[k].nbytes for k in grown) / sum(small[k].nbytes for k in grown)
    assert 3 <= ratio <= 6, (name, ratio)   # large is 3 - 6 times small in rows or frames: every slot the call uses has to grow
    assert sum(v.nbytes for v in large.values()) <= 64 << 20, name   # no single call moves more than a few tens of MB


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_plan_visits_everything_twice_and_every_slot_in_both_orders(seed):
    steps = CC.plan(seed, refused=[("nxsig_fft", "rows=0")])
    assert steps == CC.plan(seed, refused=[("nxsig_fft", "rows=0")])   # the seed decides
    calls = [s[1:] for s in steps if s[0] == "call"]
    for e in CC.ENTRIES:
        for size in CC.SIZES:
            for mode in e.modes:
                assert calls.count((e.name, size, mode)) >= 2, (e.name, size, mode)
    assert {s[1] for s in steps if s[0] == "twin"} == {e.name for e in CC.ENTRIES if e.twin}
    assert {s[1] for s in steps if s[0] == "switch"} == {e.name for e in CC.ENTRIES if e.switch}
    seen = CC.slot_orders(steps)
    for slot in CC.scratch_slots():
        if slot not in CC.EXCUSED:
            assert {("small", "large"), ("large", "small")} <= seen[slot], (slot, seen.get(slot))
    assert CC.plan(seed) != CC.plan(seed + 1)
