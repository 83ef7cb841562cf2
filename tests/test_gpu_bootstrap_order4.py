"""bootstrap_factors of a tPLS whose X has order 4 on the device (EngineOptions.tensor_folds): the resamples run through the
weighted passes with cmtfpls_kfold_inner_tensor_f64, whose wK / wL become the per-mode stacks, against literal refits
(device_folds=False).  Tolerances: loadings and Q 1e-7 normwise per column after alignment, OOB Q2Y 1e-8 (test_gpu_bootstrap.py's)."""
import numpy as np
import pytest

from cmtf_pls_amd import tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import TENSOR_RANK1
from cmtf_pls_amd.validate import bootstrap_factors
from loo_order4_ref import planted_xy

pytestmark = pytest.mark.gpu

SHAPE, M, R = (48, 6, 5, 4), 2, 3
OPT = EngineOptions(small_fit=False, tensor_folds=True)
ENTRY = "cmtfpls_kfold_inner_tensor_f64"


@pytest.fixture(scope="module")
def data():
    return planted_xy(SHAPE, M, rank=4, seed=9)


def _fitted(data, options=OPT):
    m = tPLS(R, dtype="float64", options=options)
    m.fit(*data)
    return m


def _colwise(got, want):
    """Largest normwise relative error over the columns (components) of a (B, dim, R) stack."""
    return float((np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)).max())


@pytest.mark.parametrize("NB", [8, 33])                                              # 33: a pass of 32 and the odd tail of one
def test_device_resamples_equal_literal_refits(data, NB):
    idx = np.random.default_rng(NB).integers(0, SHAPE[0], size=(NB, SHAPE[0]))
    m = _fitted(data)
    got = bootstrap_factors(m, resamples=idx)
    rep = m.bootstrap_report_
    assert ENTRY in rep["form"] and rep["rank1"] == TENSOR_RANK1 and "why" not in rep, rep
    assert rep["passes"] == -(-NB // rep["models_per_pass"]) and rep["x_reads"] == 2 * R * rep["passes"] and rep["resamples"] == NB
    want = bootstrap_factors(m, resamples=idx, device_folds=False)
    ref = m.bootstrap_report_
    assert ref["form"] == "one refit per resample on the regular engine" and "rank1" not in ref
    assert [list(v) for v in rep["n_iter"]] == [list(v) for v in ref["n_iter"]]
    assert len(got["X_factors"]) == 3 and [s.shape for s in got["X_factors"]] == [(NB, d, R) for d in SHAPE[1:]]
    for mode, (a, b) in enumerate(zip(got["X_factors"], want["X_factors"])):
        print(f"B={NB} mode {mode + 1}: {_colwise(a, b):.2e}")
        assert _colwise(a, b) <= 1e-7, mode
    print(f"B={NB} Q: {_colwise(got['Y_loadings'], want['Y_loadings']):.2e}")
    assert _colwise(got["Y_loadings"], want["Y_loadings"]) <= 1e-7
    assert np.abs(got["coef"] - want["coef"]).max() <= 1e-7 * np.abs(want["coef"]).max()
    print(f"B={NB} OOB Q2Y: {np.abs(got['oob_q2y'] - want['oob_q2y']).max():.2e}")
    assert got["oob_rows"] == want["oob_rows"] and np.abs(got["oob_q2y"] - want["oob_q2y"]).max() <= 1e-8
    for key in ("se", "ci"):                                                          # the shapes the refit path returns
        for a, b in zip(got[key]["X_factors"], want[key]["X_factors"]):
            assert a.shape == b.shape
        assert got[key]["Y_loadings"].shape == want[key]["Y_loadings"].shape and got[key]["coef"].shape == want[key]["coef"].shape
    assert [s.shape for s in got["se"]["X_factors"]] == [(d, R) for d in SHAPE[1:]]
    assert [s.shape for s in got["ci"]["X_factors"]] == [(2, d, R) for d in SHAPE[1:]]


def test_option_off_refits_with_the_report_it_always_had(data):
    m = _fitted(data, EngineOptions(small_fit=False))
    bootstrap_factors(m, n_resamples=3, random_state=1)
    rep = m.bootstrap_report_
    assert rep["form"] == "one refit per resample on the regular engine" and rep["passes"] == 0 and "rank1" not in rep
    assert rep["why"] == "X of order 4 (the device form takes order 2 and 3)"
