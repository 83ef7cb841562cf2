"""The host side of the fold entries (csrc/cv_masked.hip, csrc/loo_xcov.hip, the inner, epilogue, wide and weighted entries of
csrc/kfold.hip) answers the calls of tools/fold_entry_probe.py as the build before their shared helpers did: every status, every
error text, the order of the checks and every workspace size, held to tests/golden/fold_entry_statuses.json (recorded from that
build by the tool).  No GPU: every call is refused before a pointer is read or a kernel launched."""
import importlib.util
import json
import os

import pytest

from cmtf_pls_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe():
    spec = importlib.util.spec_from_file_location("fold_entry_probe", os.path.join(ROOT, "tools", "fold_entry_probe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def result(probe):
    return probe.probe(_lib.load())


def test_every_status_text_and_size_is_the_recorded_one(result):
    with open(os.path.join(ROOT, "tests", "golden", "fold_entry_statuses.json")) as f:
        want = json.load(f)
    assert [c["call"] for c in result["calls"]] == [c["call"] for c in want["calls"]]
    for got, exp in zip(result["calls"], want["calls"]):
        assert got == exp
    assert result["sizes"] == want["sizes"]
    assert result["lds_sizes"] == want["lds_sizes"]


def test_the_table_names_every_entry_in_scope(probe, result):
    in_scope = {name for name in _lib.SIGNATURES if name.startswith(probe.PREFIXES) and not name.startswith(probe.OUT_OF_SCOPE)}
    assert len(in_scope) == 36
    assert in_scope - probe.named(result) == set()
    assert probe.named(result) <= set(_lib.SIGNATURES)
