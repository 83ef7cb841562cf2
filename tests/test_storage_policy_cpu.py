"""CPU-only: the one policy for 16-bit X (cmtf_pls_amd/storage.py): the route decision over its whole grid, the recorder on nested
routines, and the table of 16-bit entries against the backend's list and the binding table.

No kernel runs: the backend is a stand-in that only answers has_half.  Every expected reason is written out here."""
import itertools

import pytest
import torch

from cmtf_pls_amd import _lib, backend, kfold, storage
from cmtf_pls_amd.engine import EngineOptions

OPTIONS = (None, "half_folds", "half_diagnostics")
PREFIX = {None: "", "half_folds": "EngineOptions.half_folds: ", "half_diagnostics": "EngineOptions.half_diagnostics: "}
# one entry of each group of the table, and the two routines that always copy
ENTRIES = {"xcov_stats": "fit", "mttkrp": "projection", "kfold_wide_xcov": "folds", "resid_rows": "diagnostics", "impute": None,
           "q2x_heldout": None}
ALWAYS = {
    "impute": "impute returns a float32 tensor of X's size either way, so reading the 16-bit tensor in place would save nothing",
    "q2x_heldout": "get_q2x_heldout refits masked copies of X, and the refit writes them",
}
NO_FORM = {
    "xcov_stats": "the stand-in backend has no 16-bit form of cmtfpls_xcov_stats_*",
    "mttkrp": "the stand-in backend has no 16-bit form of cmtfpls_mttkrp_*",
    "kfold_wide_xcov": "the stand-in backend has no 16-bit form of cmtfpls_kfold_wide_xcov_*",
    "resid_rows": "the stand-in backend has no 16-bit form of cmtfpls_resid_rows_*",
}


class _Backend:
    name = "stand-in"

    def __init__(self, missing=()):
        self.missing = missing                       # names, or True: every entry

    def has_half(self, base):
        return self.missing is not True and base not in self.missing


class _Engine:
    def __init__(self, opt, be):
        self.opt, self.be = opt, be


class _Model:
    def __init__(self, opt, be):
        self._engine = _Engine(opt, be)

    def _get_engine(self):
        return self._engine


@pytest.mark.parametrize("option", OPTIONS)
@pytest.mark.parametrize("on", (False, True))
@pytest.mark.parametrize("lacking", ("none", "one", "all"))
def test_route_over_the_grid(option, on, lacking):
    opt = EngineOptions(half_folds=on, half_diagnostics=on)
    for entry, group in ENTRIES.items():
        assert group is None or entry in storage.HALF_ENTRIES[group]
        be = _Backend({"none": (), "one": (entry,), "all": True}[lacking])
        if option is not None and not on:
            want = (False, None)                     # the routine's general reason stands
        elif group is None:
            want = (False, PREFIX[option] + ALWAYS[entry])
        elif lacking != "none":
            want = (False, PREFIX[option] + NO_FORM[entry])
        else:
            want = (True, None)
        assert storage.half_route(_Model(opt, be), option, (entry,)) == want, (entry, want)
        assert storage.half_route(_Engine(opt, be), option, (entry,)) == want          # an engine answers as its model
        # a backend that lacks another entry only
        other = _Backend(("contrib_rows",))
        if group is not None and (option is None or on):
            assert storage.half_route(_Model(opt, other), option, (entry,)) == (True, None)


def test_route_names_every_missing_entry_of_a_group():
    m = _Model(EngineOptions(half_folds=True), _Backend(("kfold_xcov", "xcov")))
    assert storage.half_route(m, "half_folds", storage.HALF_ENTRIES["folds"]) == (
        False, "EngineOptions.half_folds: the stand-in backend has no 16-bit form of cmtfpls_kfold_xcov_*, cmtfpls_xcov_*")
    assert storage.half_route(m, None, storage.HALF_ENTRIES["fit"]) == (False, "the stand-in backend has no 16-bit form of cmtfpls_xcov_*")
    assert storage.half_route(m, None, storage.HALF_ENTRIES["projection"]) == (True, None)

    class Bare:                                      # a backend without has_half at all (the NumPy one)
        pass
    assert storage.half_route(_Engine(EngineOptions(), Bare()), None, ("mttkrp",)) == (False, "the Bare backend has no 16-bit form of cmtfpls_mttkrp_*")


def test_names():
    assert [storage.dtype_name(d) for d in (torch.bfloat16, torch.float16, torch.float32, torch.float64)] == [
        "bfloat16", "float16", "float32", "float64"]
    assert storage.entry_name("mttkrp", torch.bfloat16) == "cmtfpls_mttkrp_bf16"
    assert storage.entry_name("kfold_xcov", torch.float16) == "cmtfpls_kfold_xcov_f16"
    assert storage.entry_name("xcov", torch.float64) == "cmtfpls_xcov_f64"
    assert storage.fallback_text(["float16", "bfloat16", "float16"], "why") == "float32 private copy of the bfloat16 / float16 data: why"
    assert storage.ROUTINE_WHY == "the kernels of this routine have no 16-bit form and read an exact float32 upcast of the rounded data"
    assert storage.FOLDS_WHY == "the fold and resampling kernels have no 16-bit form and read an exact float32 upcast of the rounded data"


def _nested(inner_notes, outer_notes, inner_reads=4, outer_reads=2):
    class M:
        pass

    @storage.reports_storage("inner_report_", "inner general")
    def inner(pls):
        inner_notes(storage.notes_of(pls))
        pls.inner_report_ = {"form": "i", "x_reads": inner_reads}

    @storage.reports_storage("outer_report_", "outer general")
    def outer(pls):
        mine = pls._storage
        outer_notes(storage.notes_of(pls))
        inner(pls)
        inner(pls)                                   # twice: reasons and entries are not repeated
        assert pls._storage is mine                  # the outer routine's notes are back in place
        pls.outer_report_ = {"form": "o", "x_reads": outer_reads}

    m = M()
    outer(m)
    assert m._storage is None                        # nothing is left installed
    return m.inner_report_, m.outer_report_


def test_recorder_on_nested_routines():
    # in-place reads inside and outside: both reports list their own entries, the outer one the inner routine's too
    inner, outer = _nested(lambda n: n.in_place(torch.bfloat16, ("resid_rows",)), lambda n: n.in_place(torch.bfloat16, ("kfold_xcov", "mttkrp")))
    assert inner == {"form": "i", "x_reads": 4, "half_storage": {"in_place": True, "dtype": "bfloat16", "entries": ["cmtfpls_resid_rows_bf16"]}}
    assert outer == {"form": "o", "x_reads": 2, "half_storage": {
        "in_place": True, "dtype": "bfloat16", "entries": ["cmtfpls_kfold_xcov_bf16", "cmtfpls_mttkrp_bf16", "cmtfpls_resid_rows_bf16"]}}

    # an upcast inside with its own reason wins in both; the outer routine's own reason comes first, none is repeated
    def inner_notes(n):
        n.in_place(torch.float16, ("recon_r2",))
        n.upcast(torch.float16, "inner reason")
    inner, outer = _nested(inner_notes, lambda n: n.upcast(torch.bfloat16, "outer reason"))
    assert inner == {"form": "i", "x_reads": 4, "storage_fallback": "float32 private copy of the float16 data: inner reason"}
    assert outer == {"form": "o", "x_reads": 2,
                     "storage_fallback": "float32 private copy of the bfloat16 / float16 data: outer reason; inner reason"}

    # upcasts without reasons of their own: each report gives its routine's general reason
    inner, outer = _nested(lambda n: n.upcast(torch.float16), lambda n: None)
    assert inner["storage_fallback"] == "float32 private copy of the float16 data: inner general"
    assert outer["storage_fallback"] == "float32 private copy of the float16 data: outer general"

    # in place, but a report without reads of X (every model refitted): no key; float32 blocks are not noted at all
    inner, outer = _nested(lambda n: n.in_place(torch.bfloat16, ("mttkrp",)), lambda n: n.in_place(torch.float32, ("mttkrp",)), outer_reads=None)
    assert inner["half_storage"]["entries"] == ["cmtfpls_mttkrp_bf16"] and outer == {"form": "o", "x_reads": None}
    inner, outer = _nested(lambda n: n.upcast(torch.float32, "not noted"), lambda n: n.in_place(torch.float64, ("xcov",)))
    assert inner == {"form": "i", "x_reads": 4} and outer == {"form": "o", "x_reads": 2}


def test_notes_outside_a_reporting_routine_go_nowhere():
    class M:
        pass
    m = M()
    storage.notes_of(m).upcast(torch.float16, "dropped")
    storage.notes_of(None).in_place(torch.float16, ("mttkrp",))
    assert not hasattr(m, "_storage")


def test_the_table_the_backend_list_and_the_bindings_agree():
    groups = storage.HALF_ENTRIES
    assert list(groups) == ["fit", "projection", "folds", "diagnostics"]
    assert [len(groups[g]) for g in groups] == [4, 1, 5, 4]
    union = set(itertools.chain.from_iterable(groups.values()))
    assert union == set(backend._HALF_ENTRIES) and len(backend._HALF_ENTRIES) == len(union) == 11
    for g, names in groups.items():
        assert len(set(names)) == len(names) and set(names) <= set(backend._HALF_ENTRIES), g
    assert kfold.HALF_READS == groups["folds"]
    assert set(groups["projection"]) <= set(groups["fit"]) and set(groups["fit"]) & set(groups["folds"]) == {"mttkrp", "xcov"}
    assert not set(groups["diagnostics"]) & (set(groups["fit"]) | set(groups["folds"]))
    assert set(storage.HALF_ALWAYS_UPCAST) == {"impute", "q2x_heldout"} and not set(storage.HALF_ALWAYS_UPCAST) & union
    for name in union:
        f32 = _lib.SIGNATURES[f"cmtfpls_{name}_f32"]
        assert _lib.SIGNATURES[f"cmtfpls_{name}_bf16"] == f32 and _lib.SIGNATURES[f"cmtfpls_{name}_f16"] == f32, name
    assert storage.HALF_DTYPES == (torch.bfloat16, torch.float16)
    assert [storage.SUFFIX[d] for d in storage.HALF_DTYPES] == ["bf16", "f16"]
