"""Leave-one-out Q2Y of a tPLS whose X has order 4 on the device (EngineOptions.tensor_folds): get_q2y and
loo_predictions through cmtfpls_loo_xcov_tensor_f64 against the per-fold refits on the regular engine (device_folds=False), the
unchanged default routing, and the declines.  Tolerance: the project's Q2Y tolerance, 1e-8."""
from types import SimpleNamespace

import numpy as np
import pytest

from cmtf_pls_amd import tPLS
from cmtf_pls_amd import validate as V
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import TENSOR_RANK1
from loo_order4_ref import planted_xy

pytestmark = pytest.mark.gpu

SHAPE, M, R = (24, 6, 5, 4), 2, 3
OPT = EngineOptions(small_fit=False, tensor_folds=True)
ENTRY = "cmtfpls_loo_xcov_tensor_f64"
OLD_WHY = "order > 3, missing values, min(J, K) > 256, M > 128 (or an M x M Gram beyond the LDS) or R > 64: outside both workgroup-per-fold kernels"


@pytest.fixture(scope="module")
def data():
    return planted_xy(SHAPE, M, seed=5)


@pytest.fixture(scope="module")
def refit(data):
    """Q2Y and report of the per-fold refit loop (computed once)."""
    m = tPLS(R, dtype="float64", options=OPT)
    m.fit(*data)
    q = V.get_q2y(m, device_folds=False)
    return q, dict(m.q2y_report_)


def test_get_q2y_takes_order4_on_the_device(data, refit):
    x, y = data
    m = tPLS(R, dtype="float64", options=OPT)
    m.fit(x, y)
    q = V.get_q2y(m)
    rep = m.q2y_report_
    assert ENTRY in rep["form"] and rep["rank1"] == TENSOR_RANK1 and rep["folds"] == SHAPE[0] and "why" not in rep, rep
    assert rep["n_iter_total"] >= 2 * R * SHAPE[0]                                   # at least two passes per fold and component
    q_ref, rep_ref = refit
    assert rep_ref == {"form": "one refit per fold on the regular engine", "folds": SHAPE[0], "why": "device folds switched off"}
    print("Q2Y", q, "refits", q_ref, "difference", abs(q - q_ref))
    assert abs(q - q_ref) <= 1e-8
    pred = V.loo_predictions(m)
    assert pred.shape == y.shape
    assert abs((1 - ((pred - y) ** 2).sum() / (y ** 2).sum()) - q) == 0.0            # the predictions get_q2y scored


def test_option_off_refits_with_the_report_it_always_had(data, refit):
    x, y = data
    m = tPLS(R, dtype="float64", options=EngineOptions(small_fit=False))
    m.fit(x, y)
    assert V.loo_predictions(m) is None
    q = V.get_q2y(m)
    assert m.q2y_report_ == {"form": "one refit per fold on the regular engine", "folds": SHAPE[0], "why": OLD_WHY}
    assert abs(q - refit[0]) <= 1e-8


def test_missing_values_keep_their_routing(data):
    x, y = data
    x = x.copy()
    x[3, 1, 2, 0] = np.nan
    m = tPLS(R, dtype="float64", options=OPT)
    m.fit(x, y)
    assert V._loo_device(m, 1e-8, 100) == (None, None)                                # get_q2y then refits with the old why


@pytest.mark.parametrize("shape,Mc,Rc,why", [
    ((4, 257, 272, 1), 2, 2, "mode-0 unfolding: min(257, 272) = 257 > 256"),
    ((4, 17, 257, 16), 2, 2, "mode-1 unfolding: min(257, 272) = 257 > 256"),
    ((4, 4, 200, 50), 2, 2, f"the fold's vectors need {8 * (4 + 20000 + 8 + 4 + 200 + 250 + 200 + 1024 + 8 + 4 + 6)} bytes of LDS > 153600 ({ENTRY})"),
    ((4, 6, 5, 4), 129, 2, f"M = 129 > 128 responses ({ENTRY})"),
    ((4, 6, 5, 4), 2, 65, f"R = 65 > 64 components ({ENTRY})"),
])
def test_a_shape_beyond_a_limit_declines_with_the_limit(shape, Mc, Rc, why):
    """The host-side predicate on a shape description (no tensor of that size exists), and the library's own status for it."""
    import torch

    from cmtf_pls_amd import _lib

    m = tPLS(R, dtype="float64", options=OPT)
    be = m._get_engine().be
    assert V._decline_loo_tensor(be, *shape[1:], Mc, Rc) == why
    lib = _lib.load()
    buf = torch.zeros(8, dtype=torch.float64, device="cuda:0")
    rc = lib.cmtfpls_loo_xcov_tensor_f64(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), *shape, Mc, Rc, 1e-8, 100, 0, 1,
                                         buf.data_ptr(), None, None, 0, None)
    assert rc == 4                                                                    # CMTFPLS_EUNSUPPORTED: the predicate and the entry agree


def test_get_q2y_reports_the_decline(data, monkeypatch):
    """A declined shape refits with the why of the limit (the decline forced on the small model: no large tensor is built)."""
    x, y = data
    m = tPLS(R, dtype="float64", options=OPT)
    m.fit(x, y)
    monkeypatch.setattr(V, "MAX_SIDE", 4)
    q = V.get_q2y(m)
    assert m.q2y_report_ == {"form": "one refit per fold on the regular engine", "folds": SHAPE[0],
                             "why": "mode-0 unfolding: min(6, 20) = 6 > 4"}
    assert np.isfinite(q)
