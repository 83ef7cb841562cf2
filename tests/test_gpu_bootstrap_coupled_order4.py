"""bootstrap_factors of a ctPLS with blocks of order 4 on the device (EngineOptions.tensor_resamples_coupled): the resamples
run through the weighted coupled passes with cmtfpls_kfold_inner_coupled_tensor_f64, whose wK / wL become the per-mode stacks of every
order-4 block, against literal refits (device_folds=False).  Tolerances: test_gpu_bootstrap_order4.py's (loadings and Q 1e-7 normwise
per column after alignment, coef 1e-7 relative, OOB Q2Y 1e-8)."""
import numpy as np
import pytest

from cmtf_pls_amd import ctPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import TENSOR_RANK1
from cmtf_pls_amd.validate import bootstrap_factors
from kfold_coupled_order4_ref import coupled_data

pytestmark = pytest.mark.gpu

I, M, R = 48, 3, 3
TWO = [(48, 6, 5, 4), (48, 7)]
THREE = [(48, 6, 5, 4), (48, 8, 6), (48, 3, 4, 7)]
OPT = EngineOptions(small_fit=False, tensor_resamples_coupled=True)
ENTRY = "cmtfpls_kfold_inner_coupled_tensor_f64"
OLD = "block 0 of order 4 (the device form takes order 2 and 3)"
REFIT = "one refit per resample on the regular engine"


def _fitted(shapes, options=OPT):
    Xs, y = coupled_data(shapes, M, 4, seed=7)
    m = ctPLS(R, dtype="float64", options=options)
    m.fit(Xs, y)
    return m


def _colwise(got, want):
    """Largest normwise relative error over the columns (components) of a (B, dim, R) stack."""
    return float((np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)).max())


@pytest.mark.parametrize("NB", [8, 33])                                              # 33: a pass of 32 and the odd tail of one
@pytest.mark.parametrize("shapes", [TWO, THREE], ids=["two_blocks", "three_blocks"])
def test_device_resamples_equal_literal_refits(shapes, NB):
    idx = np.random.default_rng(NB).integers(0, I, size=(NB, I))
    m = _fitted(shapes)
    got = bootstrap_factors(m, resamples=idx)
    rep = m.bootstrap_report_
    assert ENTRY in rep["form"] and rep["rank1"] == TENSOR_RANK1 and "why" not in rep, rep    # (the parent commit refits here)
    assert "cmtfpls_kfold_inner_coupled_f64" not in rep["form"]
    assert rep["passes"] == -(-NB // rep["models_per_pass"]) and rep["x_reads"] == [2 * R * rep["passes"]] * len(shapes)
    assert rep["resamples"] == NB
    want = bootstrap_factors(m, resamples=idx, device_folds=False)
    ref = m.bootstrap_report_
    assert ref["form"] == REFIT and "rank1" not in ref
    assert [list(v) for v in rep["n_iter"]] == [list(v) for v in ref["n_iter"]]
    assert len(got["X_factors"]) == len(shapes)
    for b, shape in enumerate(shapes):
        assert [s.shape for s in got["X_factors"][b]] == [(NB, d, R) for d in shape[1:]]      # an order-4 block: three stacks
        for mode, (a, w) in enumerate(zip(got["X_factors"][b], want["X_factors"][b])):
            print(f"B={NB} block {b} mode {mode + 1}: {_colwise(a, w):.2e}")
            assert _colwise(a, w) <= 1e-7, (b, mode)
        for key, lead in (("se", ()), ("ci", (2,))):                                     # the shapes the refit path returns
            assert [s.shape for s in got[key]["X_factors"][b]] == [s.shape for s in want[key]["X_factors"][b]] == \
                [lead + (d, R) for d in shape[1:]]
    print(f"B={NB} Q: {_colwise(got['Y_loadings'], want['Y_loadings']):.2e}")
    assert _colwise(got["Y_loadings"], want["Y_loadings"]) <= 1e-7
    assert np.abs(got["coef"] - want["coef"]).max() <= 1e-7 * np.abs(want["coef"]).max()
    print(f"B={NB} OOB Q2Y: {np.abs(got['oob_q2y'] - want['oob_q2y']).max():.2e}")
    assert got["oob_rows"] == want["oob_rows"] and np.abs(got["oob_q2y"] - want["oob_q2y"]).max() <= 1e-8
    for key in ("se", "ci"):
        assert got[key]["Y_loadings"].shape == want[key]["Y_loadings"].shape and got[key]["coef"].shape == want[key]["coef"].shape


@pytest.mark.parametrize("options", [EngineOptions(small_fit=False), EngineOptions(small_fit=False, tensor_folds_coupled=True)],
                         ids=["default", "tensor_folds_coupled"])
def test_without_the_option_the_refit_report_and_its_reason_are_unchanged(options):
    m = _fitted(TWO, options)
    bootstrap_factors(m, n_resamples=3, random_state=1)
    rep = m.bootstrap_report_
    assert rep["form"] == REFIT and rep["passes"] == 0 and rep["why"] == OLD and "rank1" not in rep, rep
