"""Error table of the C ABI with a real context (tools/abi_error_probe.py against tests/golden/abi_error_table.json, which the same
probe produced from the build before the entry points were folded onto one prologue and one staging helper): every validation message
of every entry point is reached and none of the broken cases launches anything; the valid row of each entry point — the smallest call
that works — runs once with NXSIG_HOST and once with NXSIG_DEVICE and the two results are equal bit for bit."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import abi_error_probe as P  # noqa: E402
from nx_signal_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

with open(P.GOLDEN) as f:
    GOLDEN = json.load(f)["real_ctx"]


@pytest.fixture(scope="module")
def table():
    return P.probe(_lib.LIB_PATH, real=True)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_real_context_error_table(table, name):
    assert table[name] == GOLDEN[name]


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_host_and_device_calls_agree_bit_for_bit(table, name):
    assert table[name]["valid"]["rc"] == 0 and table[name]["valid"]["host_equals_device"] is True


def test_every_broken_case_is_refused_with_a_message():
    for name, rows in GOLDEN.items():
        for label, rec in rows.items():
            assert (rec["rc"] == 0) == (label == "valid"), (name, label)
            assert label == "valid" or rec["err"], (name, label)
