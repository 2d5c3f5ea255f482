"""The call catalogue of tests/context_calls.py against the sources, without a GPU: every scratch slot of a context is claimed by an
entry (or excused with a reason), every claim cites the line that takes the slot, every line that takes a slot is cited, every dispatch
switch is some entry's, every kind of cached table appears, every user of a shared slot runs behind every other, and the builders are
deterministic."""
import os
import re

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


def test_every_table_tag_of_the_newer_kernel_files_maps_to_a_kind():
    for name, kinds in CC.TABLE_TAGS.items():
        tags = CC.table_tags(name)
        assert set(tags) == set(kinds), f"{name}: ctx_table tags {sorted(set(tags) ^ set(kinds))} are not mapped (or no longer there)"
        assert set(kinds.values()) <= set(CC.TABLE_KINDS), name


def test_every_line_that_takes_a_scratch_slot_is_cited():
    """the next family that moves into an old slot fails here until it has an entry of its own: every `ctx_scratch(<ctx>, kScratch...`
    call under csrc is cited by a claim, or excused with a reason (a site the Python mirror cannot reach on one context)"""
    sites = CC.scratch_sites()
    # 50 today: 52 when this test was written, less the two pairs of sites of sosfilt and lfilter, which became one pair (recurrence_scan.hpp)
    assert len(sites) >= 50 and len({s for s, _ in sites}) == len(sites), len(sites)
    assert {slot for _, slot in sites} <= set(CC.scratch_slots())
    cited = {}
    for e in CC.ENTRIES:
        for slot, cite in {**e.slots, **e.host_slots}.items():
            cited.setdefault(cite, set()).add(slot)
    missing = [f"{site} ({slot})" for site, slot in sites if slot not in cited.get(site, ()) and site not in CC.EXCUSED_SITES]
    assert not missing, f"no catalogue entry cites {missing}: add an entry that reaches the line, or excuse it with a reason"
    known = {site for site, _ in sites}
    assert set(CC.EXCUSED_SITES) <= known, f"excused, but no ctx_scratch call: {sorted(set(CC.EXCUSED_SITES) - known)}"
    both = sorted(s for s in CC.EXCUSED_SITES if s in cited)
    assert not both, f"cited AND excused: {both}"
    assert all(reason.strip() for reason in CC.EXCUSED_SITES.values())


def test_every_dispatch_switch_has_an_entry():
    with open(os.path.join(CC.CSRC, "nxsig_internal.h")) as f:
        body = re.search(r"#define NXSIG_TUNABLES\(X\)(.*?)\nenum TuneKey", f.read(), re.S).group(1)
    switches = [n for n in re.findall(r"X\((\w+)\)", body) if n.startswith("DISABLE_")]
    assert len(switches) >= 19 and "DISABLE_WAVE" in switches and "DISABLE_LFILTER_SCAN" in switches, switches
    used = {e.switch[0] for e in CC.ENTRIES if e.switch}
    assert used <= set(switches), sorted(used - set(switches))
    missing = [n for n in switches if n not in used and n not in CC.EXCUSED_SWITCHES]
    assert not missing, f"no entry runs under {missing}: give the entry of that family the switch, or excuse it with a reason"
    assert not used & set(CC.EXCUSED_SWITCHES) and all(r.strip() for r in CC.EXCUSED_SWITCHES.values())


def _group(name):
    """the family group of an entry, for the coverage of user_pairs()"""
    for prefix, group in (("welch", "welch"), ("csd", "csd"), ("coherence", "csd"), ("sosfilt", "sosfilt"), ("lfilter", "lfilter"), ("filtfilt", "filtfilt"),
                          ("find-peaks", "find_peaks"), ("argrel", "argrel"), ("hilbert", "hilbert.generic"), ("dct", "dct.fft"), ("idct", "dct.fft")):
        if name.startswith(prefix):
            return "sosfiltfilt" if name.startswith("sosfiltfilt") else group
    return {"stft5000-long": "long stft", "mel16-two-step": "mel two-step", "istft512-masked-two-step": "masked istft two-step",
            "fir4097-delay-line": "fir delay-line", "fir40001-one-transform": "fir long"}.get(name, name)


def test_user_pairs_put_every_family_of_a_shared_slot_behind_every_other():
    pairs = CC.user_pairs()
    claims = {slot: CC.slot_users(slot) for slot in CC.scratch_slots()}
    assert set(pairs) == {slot for slot, users in claims.items() if len(users) >= 2}
    for slot in CC.scratch_slots():   # every claimant, but for the thinned slots: there one claimant of every source file that takes the slot
        users = [e for e in CC.ENTRIES if slot in e.slots]
        if slot in CC.THINNED:
            assert {CC.BY_NAME[n].slots[slot].partition(":")[0] for n in claims[slot]} == {e.slots[slot].partition(":")[0] for e in users}, slot
            assert len(claims[slot]) == len({e.slots[slot].partition(":")[0] for e in users}), slot
        else:
            assert claims[slot] == [e.name for e in users], slot
    assert set(CC.THINNED) == {"kScratchWaveSink"}   # the write-only dummy target; a slot whose content a kernel reads back is never thinned
    for slot, got in pairs.items():   # every ordered pair of distinct claimants, once
        assert len(got) == len(set(got)) == len(claims[slot]) * (len(claims[slot]) - 1), slot
        assert all(a != b and a in claims[slot] and b in claims[slot] for a, b in got), slot
    assert all("Stage" not in slot or slot == "kScratchMultiStage" for slot in pairs), "host staging slots are no kernel-side claims"
    want = {
        "kScratchLongStftFrames": {"long stft", "welch", "csd", "sosfilt", "lfilter"},
        "kScratchFusedSpectrum": {"mel two-step", "welch", "hilbert.generic", "dct.fft"},
        "kScratchIstftProduct": {"masked istft two-step", "hilbert.generic", "dct.fft"},
        "kScratchFirLong": {"fir delay-line", "fir long", "sosfiltfilt", "filtfilt"},
        "kScratchPeakTiles": {"argrel", "find_peaks"},
        "kScratchPeakExtremes": {"argrel", "find_peaks"},
    }
    for slot, groups in want.items():
        seen = {(_group(a), _group(b)) for a, b in pairs[slot]}
        missing = [(g, h) for g in sorted(groups) for h in sorted(groups) if g != h and (g, h) not in seen]
        assert not missing, f"{slot}: no pair runs {missing}"
    # slot 4's welch user is the generic tier, whose spectra live there
    assert any(a.startswith("welch") and "generic" in a for a, _ in pairs["kScratchFusedSpectrum"])


def test_the_entries_with_non_finite_state_carry_a_twin():
    twins = {e.name for e in CC.ENTRIES if e.twin}
    # FIR row flags in both forms, a frame-packing istft, the packed istft, log-mel, dBFS, the masked istft
    assert {"fir257", "fir4097-delay-line", "istft512-half", "istft1024-packed", "mel1024", "dbfs1024", "istft1024-masked"} <= twins
    # welch row flags on both tiers, the chunk states of the two recursive scans, the extended rows of the two forward-backward filters,
    # the row means of hilbert.generic and dct.fft
    assert {"welch1024-pair", "welch2048-pair", "welch400-in-512-generic", "sosfilt-scan", "sosfilt-scan-zi-zf", "lfilter-scan", "lfilter-scan-zi-zf",
            "sosfiltfilt-odd", "filtfilt-odd", "hilbert1000-generic", "hilbert1025-generic-envelope", "dct400-fft", "idct257-fft"} <= twins
    for e in CC.ENTRIES:
        if not e.twin:
            continue
        plain, twin = e.inputs("small"), e.inputs("small", twin=True)
        assert all(np.isfinite(v).all() for v in plain.values()), e.name
        assert any(not np.isfinite(v).all() for v in twin.values()), e.name
        assert plain.keys() == twin.keys() and all(plain[k].shape == twin[k].shape for k in plain), e.name


def test_names_are_unique_and_there_are_enough_entries():
    assert len(CC.BY_NAME) == len(CC.ENTRIES) >= 67
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
