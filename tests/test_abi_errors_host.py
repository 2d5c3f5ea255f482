"""Error table of the C ABI without a GPU: every compute entry point of include/nxsig.h is called with ctx = NULL, first with small valid
arguments and then with one argument broken at a time (tools/abi_error_probe.py).  The return code, nxsig_last_error() and what was
written to *num_frames_out must be what tests/golden/abi_error_table.json records, which was produced by the same probe from the build
before the entry points were folded onto one prologue and one staging helper.  Entry points that look at the context first say
"null context" every time; stft_onesided / stft_packed / stft_magnitude, the fir wrappers, spectrum_mul and the mask checks give the
argument's own message, and the first three write *num_frames_out before they look at the context."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402
from nx_signal_amd import _lib  # noqa: E402

with open(P.GOLDEN) as f:
    GOLDEN = json.load(f)["null_ctx"]


@pytest.fixture(scope="module")
def table():
    return P.probe(_lib.LIB_PATH, real=False)


def test_the_probe_covers_every_compute_entry_point_of_the_header():
    """every symbol of the signature table that takes a context and computes something has a row (the context's own management calls,
    the timers and the group calls aside)"""
    management = {"nxsig_ctx_destroy", "nxsig_ctx_set_tuning", "nxsig_ctx_get_tuning", "nxsig_ctx_clear_tuning", "nxsig_ctx_last_dispatch",
                  "nxsig_device_name", "nxsig_alloc", "nxsig_free", "nxsig_upload", "nxsig_download", "nxsig_sync", "nxsig_set_stream",
                  "nxsig_get_stream", "nxsig_timer_start", "nxsig_timer_stop", "nxsig_timer_lap", "nxsig_timer_laps", "nxsig_mem_info",
                  "nxsig_sinc_f32", "nxsig_sinc_f64"}   # (sinc: a host generator whose first argument is a pointer too)
    compute = {n for n, (_, args) in _lib.SIGNATURES.items()
               if args and args[0] is _lib._p and n not in management and "_group_" not in n and "_sharded_" not in n}
    assert compute == {name for name, _, _ in P.ENTRIES} == set(GOLDEN)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_null_context_error_table(table, name):
    assert table[name] == GOLDEN[name]


def test_context_first_and_validate_first_entry_points_keep_their_order():
    """pinned on the golden table itself, so that a regenerated file cannot move the order unnoticed"""
    validate_first = ("nxsig_stft_onesided_f32", "nxsig_stft_packed_f32", "nxsig_stft_magnitude_f32")
    for name, rows in GOLDEN.items():
        want = {"rc": -1, "err": "null context"}
        if "num_frames_out" in rows["valid"]:
            want["num_frames_out"] = 4 if name in validate_first else P.NF_SENTINEL
        assert rows["valid"] == want, name
    for name in ("nxsig_stft_f32", "nxsig_stft_c64", "nxsig_stft_mel_f32", "nxsig_as_windowed_f32", "nxsig_fft", "nxsig_fir_slice_f32"):
        assert {r["err"] for r in GOLDEN[name].values()} == {"null context"}, name
    for name in validate_first:
        assert GOLDEN[name]["batch=0"]["err"].endswith("batch must be in [1, 65535]") and GOLDEN[name]["hop=0"]["num_frames_out"] == P.NF_SENTINEL
    assert GOLDEN["nxsig_stft_packed_f32"]["fft_length=7"]["err"] == "stft_packed: fft_length must be even"
    assert GOLDEN["nxsig_stft_packed_f32"]["null x"]["err"] == "stft_onesided: null pointer argument"
    for name in ("nxsig_fir_f32", "nxsig_fir_f64"):
        assert GOLDEN[name]["length=0"]["err"] == "fir: batch, length and num_taps must be >= 1"
        assert GOLDEN[name]["mode=9"]["err"] == "expected mode to be one of [:full, :same, :valid]"
        assert GOLDEN[name]["batch=0"]["err"] == "null context"
