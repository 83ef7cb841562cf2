"""CPU-only, no library, no backend: the route that the resampling drivers share (kfold._route), the one sentence of a masked
decline (kfold._masked_declined) and the report they assemble (kfold._passes_report, _masked_run_report, _form_entries), over stub
models holding the data and options of every row of tools/resample_dump.py's table.  The expected routes are written out here by
hand from what each driver did before it called _route: kfold_run, repeated_kfold and bootstrap ask masked, then masked coupled;
permutation_test asks masked coupled first and refits a ctPLS without EngineOptions.coupled_permutations; nested_kfold has no
masked form."""
import importlib.util
import os
from types import SimpleNamespace

import pytest

from cmtf_pls_amd import kfold as KF
from cmtf_pls_amd.engine import EngineOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("resample_dump", os.path.join(ROOT, "tools", "resample_dump.py"))
DUMP = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(DUMP)

NOT_BUILT = "coupled model: permutation device form not built"
FOLD, MODELS, T_FOLD, T_MODELS, COUPLED = (KF.MASKED_FORM, KF.MODELS_FORM, KF.MASKED_TENSOR_FORM, KF.MODELS_TENSOR_FORM, KF.COUPLED_FORM)
# case -> what _route answers for (kfold_run, the drivers of count-weighted models, permutation_test); a case not listed takes
# the device passes in all of them
MASKED_ROWS = {
    "t2/nan/masked_folds": (FOLD, MODELS), "t3/nan/masked_folds": (FOLD, MODELS), "t4/nan/masked_folds_alone": (FOLD, MODELS),
    "t4/nan/masked_tensor_folds": (T_FOLD, T_MODELS), "decline/nan_in_y/masked_folds": (FOLD, MODELS),
    "status/masked_folds": (FOLD, MODELS),
}
COUPLED_ROWS = ("c3/nan/masked_folds_coupled", "c4/nan/masked_folds_coupled", "status/masked_folds_coupled")
PERMUTATION_REFITS = ("c3/complete/off", "c4/complete/off", "c4/complete/tensor_folds_coupled", "c3/nan/off", "c4/nan/off")


def _stub(case, seed):
    _, _, Xr, Yr = DUMP.inputs(case, seed)
    opt = EngineOptions(small_fit=False, **case["options"])
    pls = SimpleNamespace(_get_engine=lambda: SimpleNamespace(opt=opt))
    return pls, (Xr if case["model"].startswith("c") else Xr[0]), opt


def _routes(pls, X, opt, device_folds):
    gate = (isinstance(X, list) and opt.coupled_permutations, NOT_BUILT)
    return {"kfold": KF._route(pls, X, device_folds, models=False), "models": KF._route(pls, X, device_folds),
            "permutation": KF._route(pls, X, device_folds, coupled_first=True, coupled_gate=gate),
            "nested": KF._route(pls, X, device_folds, masked=False)}


@pytest.mark.parametrize("seed,case", list(enumerate(DUMP.CASES, start=1)), ids=[c["name"] for c in DUMP.CASES])
def test_route_of_every_row_of_the_table(seed, case):
    pls, X, opt = _stub(case, seed)
    got = _routes(pls, X, opt, case["device_folds"])
    name = case["name"]
    if not case["device_folds"]:
        want = dict.fromkeys(got, (KF.OFF, "device folds switched off"))
    elif name in MASKED_ROWS:
        fold, models = MASKED_ROWS[name]
        want = {"kfold": (KF.MASKED, fold), "models": (KF.MASKED, models), "permutation": (KF.MASKED, models), "nested": (KF.PASSES, None)}
    elif name in COUPLED_ROWS:
        want = {**dict.fromkeys(got, (KF.MASKED_COUPLED, COUPLED)), "nested": (KF.PASSES, None)}
    else:
        want = dict.fromkeys(got, (KF.PASSES, None))
        if name in PERMUTATION_REFITS:
            want["permutation"] = (KF.REFIT, NOT_BUILT)
    assert got == want
    for route, entry in got.values():
        if route in (KF.MASKED, KF.MASKED_COUPLED):
            assert KF._masked_declined(entry, "missing values in Y") == f"the masked form ({entry}) declined: missing values in Y"
    assert set(MASKED_ROWS) | set(COUPLED_ROWS) | set(PERMUTATION_REFITS) <= {c["name"] for c in DUMP.CASES}


def test_a_masked_test_never_reads_the_other_kind_of_model(monkeypatch):
    """The two masked tests cannot both hold, whichever is asked first: a ctPLS is a list, which wants_masked turns away, and a
    tPLS is none, which wants_masked_coupled turns away, each before has_missing looks at the data."""
    seen = []
    monkeypatch.setattr(KF, "has_missing", lambda X: seen.append(X) or True)
    opt = EngineOptions(masked_folds=True, masked_folds_coupled=True, masked_tensor_folds=True)
    pls = SimpleNamespace(_get_engine=lambda: SimpleNamespace(opt=opt))
    x, blocks = SimpleNamespace(ndim=3), [SimpleNamespace(ndim=2), SimpleNamespace(ndim=3)]
    for first in (False, True):
        assert KF._route(pls, x, True, coupled_first=first) == (KF.MASKED, MODELS)
        assert KF._route(pls, blocks, True, coupled_first=first, coupled_gate=(False, NOT_BUILT)) == (KF.MASKED_COUPLED, COUPLED)
    assert all(s is x or s is blocks[0] for s in seen)
    assert KF._route(pls, blocks, False, coupled_gate=(False, NOT_BUILT)) == (KF.OFF, "device folds switched off")


def _permutation_report(coupled, passes, why, tensor=None):
    K, G, R = 3, 10, 2
    Xs = [None, None] if coupled else [None]
    return KF._passes_report(f"{K * G} models per pass ({G} permutations x {K} folds)", "cmtfpls_kfold_wide_xcov_*",
                             "cmtfpls_kfold_epilogue_grouped_f64", Xs, coupled, passes, 2 * R * passes, why, None if coupled else "fold",
                             "one refit per fold and permutation on the regular engine", {"permutations": 23}, ("models_per_pass", K * G),
                             [[1, 2]], tensor, grouped=True, more={"observed": {"folds": 3}})


def test_the_four_sentences_permutation_spelt_out():
    coupled = ("30 models per pass (10 permutations x 3 folds) from shared reads of every block (cmtfpls_kfold_wide_xcov_*, "
               "cmtfpls_kfold_inner_coupled_grouped_f64, cmtfpls_mttkrp_*, cmtfpls_kfold_combine_scores_f64, "
               "cmtfpls_kfold_epilogue_grouped_f64, cmtfpls_xcov_*)")
    single = ("30 models per pass (10 permutations x 3 folds) from shared reads of X (cmtfpls_kfold_wide_xcov_*, "
              "cmtfpls_kfold_inner_grouped_f64, cmtfpls_mttkrp_*, cmtfpls_kfold_epilogue_grouped_f64, cmtfpls_xcov_*)")
    assert _permutation_report(True, 3, None)["form"] == coupled
    assert _permutation_report(True, 3, "pass 1: refitted")["form"] == coupled          # a ctPLS's form never carried the note
    assert _permutation_report(False, 3, None)["form"] == single
    assert _permutation_report(False, 3, "pass 1: refitted")["form"] == single + "; failed passes refitted per fold on the regular engine"
    assert _permutation_report(False, 0, "K = 33 folds > 32")["form"] == "one refit per fold and permutation on the regular engine"
    assert KF._form_entries("cmtfpls_kfold_xcov_*", False, "cmtfpls_kfold_epilogue_f64") == \
        "(cmtfpls_kfold_xcov_*, cmtfpls_kfold_inner_f64, cmtfpls_mttkrp_*, cmtfpls_kfold_epilogue_f64, cmtfpls_xcov_*)"
    assert KF._form_entries("cmtfpls_kfold_xcov_*", True, "cmtfpls_kfold_epilogue_f64") == \
        ("(cmtfpls_kfold_xcov_*, cmtfpls_kfold_inner_coupled_f64, cmtfpls_mttkrp_*, cmtfpls_kfold_combine_scores_f64, "
         "cmtfpls_kfold_epilogue_f64, cmtfpls_xcov_*)")


def test_the_report_of_a_driver_of_passes():
    rep = _permutation_report(True, 3, None)
    assert rep == {"form": rep["form"], "permutations": 23, "passes": 3, "models_per_pass": 30, "x_reads": [12, 12], "n_iter": [[1, 2]],
                   "observed": {"folds": 3}}
    assert list(rep) == ["form", "permutations", "passes", "models_per_pass", "x_reads", "n_iter", "observed"]
    rep = _permutation_report(False, 0, "device folds switched off")
    assert rep["x_reads"] is None and rep["models_per_pass"] is None and rep["passes"] == 0 and rep["why"] == "device folds switched off"
    assert "rank1" not in _permutation_report(False, 0, "x", tensor=(3, 2))             # the refits ran no CP in a fold loop
    rep = _permutation_report(False, 3, None, tensor=(3, 2))
    assert rep["rank1"] == KF.TENSOR_RANK1 and "cmtfpls_kfold_inner_tensor_f64" in rep["form"] and "inner_grouped" not in rep["form"]
    assert rep["x_reads"] == 12
    rep = _permutation_report(True, 3, None, tensor=[(0, 0), (3, 2)])
    assert rep["rank1"] == KF.TENSOR_RANK1 and "cmtfpls_kfold_inner_coupled_tensor_f64" in rep["form"]
    nested = KF._passes_report("20 0/1-weighted models per pass", "cmtfpls_kfold_weighted_xcov_*", "cmtfpls_kfold_epilogue_weighted_f64",
                               [None], False, 2, 8, "pass 0: refitted", "model", "one refit per model on the regular engine",
                               {"models": 24, "outer_folds": 6, "inner_folds": 3}, ("models_per_pass", 20), [], None,
                               scored=", scored by cmtfpls_press_rows_f64")
    assert nested["form"] == ("20 0/1-weighted models per pass from shared reads of X (cmtfpls_kfold_weighted_xcov_*, cmtfpls_kfold_inner_f64, "
                              "cmtfpls_mttkrp_*, cmtfpls_kfold_epilogue_weighted_f64, cmtfpls_xcov_*), scored by cmtfpls_press_rows_f64; "
                              "failed passes refitted per model on the regular engine")
    assert list(nested)[:6] == ["form", "models", "outer_folds", "inner_folds", "passes", "models_per_pass"]


def test_a_masked_run_folded_into_a_drivers_report():
    masked = {"form": "f", "models": 69, "launches": 2, "x_reads": None}
    assert KF._masked_run_report(masked, "permutations", 23, "models_per_pass", [1], observed={}) == \
        {"form": "f", "models": 69, "launches": 2, "x_reads": None, "permutations": 23, "passes": 2, "models_per_pass": 35, "n_iter": [1],
         "observed": {}}
    assert KF._masked_run_report(masked, "splits", 23, "splits_per_pass", [1])["splits_per_pass"] == 12
