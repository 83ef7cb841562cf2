"""EngineOptions.half_folds: every resampling driver of a model with 16-bit storage on the caller's 16-bit device tensor itself
(kfold._device_blocks, cmtfpls_kfold_*xcov_{bf16,f16} with the 16-bit score pass and contraction), tPLS and ctPLS.

Data: half_storage_ref.fit_data at (300, 12, 10), coupled (300, 12, 10) + (300, 20) and order 4 (120, 12, 8, 5); R = 3, M = 2.
The twin of a 16-bit model is the float32 model (dtype="float32") on the exact upcast of the same 16-bit values: both see identical
numbers, and the in-place pass is the twin's arithmetic in another float64 summation order (the 16-bit MTTKRP is the tile form).

Bounds.  kfold_predictions: 1e-7 normwise relative against literal per-fold refits of the twin for every component count, the
project's bound for a float32-storage device form against refits (tests/test_gpu_kfold.py::_TOL).  The other drivers against the
twin's own device-form results at the tolerance their tests use against refits: the permutation test 1e-7
(tests/test_gpu_permutation.py), repeated K-fold 1e-9 (tests/test_gpu_repeated_kfold.py), nested K-fold 1e-5 on the predictions
and 1e-8 on the Q2Y (tests/test_gpu_nested_kfold.py), the bootstrap 1e-5 column-wise (tests/test_gpu_bootstrap.py).  n_iter is
printed, not gated.  Measured on MI355X: DESIGN 8w ("Resampling").
"""
from unittest import mock

import numpy as np
import pytest
import torch

import half_storage_ref as HS
from cmtf_pls_amd import validate as V
from cmtf_pls_amd.engine import EngineOptions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R, M, K = 3, 2, 5
SHAPES = {"tPLS": ("two-read", [(300, 12, 10)], 2), "ctPLS": ("coupled", [(300, 12, 10), (300, 20)], 9),
          "order-4": ("order-4", [(120, 12, 8, 5)], 3)}
ON = dict(small_fit=False, half_folds=True, coupled_permutations=True)
_cache = {}


@pytest.fixture(scope="module")
def api():
    import cmtf_pls_amd
    return cmtf_pls_amd


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()
    torch.cuda.empty_cache()


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def _colwise(a, b):
    return float((np.linalg.norm(a - b, axis=-2) / np.maximum(np.linalg.norm(b, axis=-2), 1e-300)).max())


def _case(api, which, kind, **opts):
    """The fitted 16-bit model on the caller's device tensors and its float32 twin on their upcasts (once per case)."""
    key = (which, kind, tuple(sorted(opts.items())))
    if key not in _cache:
        name, shapes, seed = SHAPES[which]
        with mock.patch.dict(HS.FIT_MODELS, {name: shapes}):
            blocks, y, _ = HS.fit_data(name, seed)
        y = np.ascontiguousarray(y[:, :M])
        X16 = [HS.quantise(b, kind)[0].to(DEV) for b in blocks]
        X32 = [x.to(torch.float32) for x in X16]
        coupled = len(blocks) > 1
        cls = api.ctPLS if coupled else api.tPLS
        m = cls(R, dtype=HS.NAMES[kind], algorithm="xcov", options=EngineOptions(**{**ON, **opts}))
        twin = cls(R, dtype="float32", algorithm="xcov", options=EngineOptions(**{**ON, **opts, "half_folds": False}))
        m.fit(X16 if coupled else X16[0], y)
        twin.fit(X32 if coupled else X32[0], y)
        assert m.fit_report_["half_storage"]["in_place"], m.fit_report_
        _cache[key] = dict(m=m, twin=twin, X16=X16, y=y, keep=[x.view(torch.int16).clone() for x in X16], ptr=[x.data_ptr() for x in X16])
    return _cache[key]


def _in_place(c, attr, kind, marks, builder):
    """The report of a run that read the 16-bit tensor in place; the caller's tensors as they were."""
    rep = getattr(c["m"], attr)
    assert "storage_fallback" not in rep and "why" not in rep, rep
    hs = rep["half_storage"]
    assert hs["in_place"] is True and hs["dtype"] == HS.NAMES[kind], rep
    assert f"cmtfpls_{builder}_{kind}" in hs["entries"] and f"cmtfpls_mttkrp_{kind}" in hs["entries"] and f"cmtfpls_xcov_{kind}" in hs["entries"]
    for mark in marks:
        assert mark in rep["form"], rep
    assert "refit" not in rep["form"], rep
    twin_rep = getattr(c["twin"], attr, {})                                       # (of the twin's last run, where it has had one)
    assert "half_storage" not in twin_rep and "storage_fallback" not in twin_rep
    for x, k, p in zip(c["X16"], c["keep"], c["ptr"]):
        assert x.data_ptr() == p and torch.equal(x.view(torch.int16), k), "the caller's tensor was touched"
    return rep


def _kfold_check(c, which, kind, marks):
    m, twin = c["m"], c["twin"]
    pred = V.kfold_predictions(m, n_splits=K)
    rep = _in_place(c, "q2y_report_", kind, marks, "kfold_xcov")
    dev = V.kfold_predictions(twin, n_splits=K)
    n_twin = twin.q2y_report_["n_iter"]
    assert "cmtfpls_kfold_xcov_*" in twin.q2y_report_["form"]
    lit = V.kfold_predictions(twin, n_splits=K, device_folds=False)               # one literal refit per fold of the float32 twin
    assert twin.q2y_report_["form"].startswith("one refit per fold")
    errs = [_rel(pred[r], lit[r]) for r in range(R)]
    print(f"{which} {kind} kfold_predictions: vs literal refits of the twin {['%.3g' % e for e in errs]}, vs the twin's device form "
          f"{_rel(pred, dev):.3g}; n_iter in place {rep['n_iter']} twin {n_twin}")
    assert max(errs) <= 1e-7, errs
    return rep


@pytest.mark.parametrize("kind", HS.KINDS)
@pytest.mark.parametrize("which", ["tPLS", "ctPLS"])
def test_kfold_in_place_against_literal_refits_of_the_twin(api, which, kind):
    c = _case(api, which, kind)
    _kfold_check(c, which, kind, ["cmtfpls_kfold_xcov_*", "cmtfpls_kfold_inner_coupled_f64" if which == "ctPLS" else "cmtfpls_kfold_inner_f64"])
    q, qt = V.get_q2y_kfold(c["m"], n_splits=K, per_component=True), V.get_q2y_kfold(c["twin"], n_splits=K, per_component=True)
    _in_place(c, "q2y_report_", kind, ["cmtfpls_kfold_xcov_*"], "kfold_xcov")
    print(f"{which} {kind} get_q2y_kfold: {np.abs(np.asarray(q) - np.asarray(qt)).max():.3g}")
    assert np.abs(np.asarray(q) - np.asarray(qt)).max() <= 1e-8 * max(1.0, np.abs(qt).max())     # get_q2y_kfold against refits, test_gpu_kfold.py


@pytest.mark.parametrize("kind", HS.KINDS)
@pytest.mark.parametrize("which", ["tPLS", "ctPLS"])
def test_the_other_drivers_in_place_against_the_twin(api, which, kind):
    c = _case(api, which, kind)
    m, twin = c["m"], c["twin"]

    a, b = (V.permutation_test_q2y(x, n_permutations=7, n_splits=K, random_state=3, per_component=True) for x in (m, twin))
    rep = _in_place(c, "q2y_report_", kind, ["cmtfpls_kfold_wide_xcov"], "kfold_wide_xcov")
    err = np.abs(a["null"] - b["null"]).max() / max(1.0, np.abs(b["null"]).max())
    print(f"{which} {kind} permutation_test_q2y: {err:.3g}; n_iter equal {rep['n_iter'] == twin.q2y_report_['n_iter']}")
    assert err <= 1e-7 and np.abs(a["q2y"] - b["q2y"]).max() <= 1e-7

    a, b = (V.get_q2y_repeated_kfold(x, n_splits=K, n_repeats=3, random_state=5, per_component=True) for x in (m, twin))
    rep = _in_place(c, "q2y_report_", kind, ["cmtfpls_kfold_epilogue_splits_f64"], "kfold_xcov")
    err = np.abs(a["q2y"] - b["q2y"]).max() / max(1.0, np.abs(b["q2y"]).max())
    print(f"{which} {kind} get_q2y_repeated_kfold: {err:.3g}; n_iter equal {rep['n_iter'] == twin.q2y_report_['n_iter']}")
    assert err <= 1e-9

    a, b = (V.get_q2y_nested_kfold(x, n_outer=3, n_inner=3, random_state=2) for x in (m, twin))
    rep = _in_place(c, "q2y_report_", kind, ["cmtfpls_kfold_weighted_xcov"], "kfold_weighted_xcov")
    errs = (_rel(a["predictions"], b["predictions"]), abs(a["q2y"] - b["q2y"]), np.abs(a["inner_q2y"] - b["inner_q2y"]).max(),
            np.abs(a["outer_q2y"] - b["outer_q2y"]).max())
    print(f"{which} {kind} get_q2y_nested_kfold: predictions {errs[0]:.3g} q2y {errs[1]:.3g} inner {errs[2]:.3g} outer {errs[3]:.3g}; "
          f"n_iter equal {rep['n_iter'] == twin.q2y_report_['n_iter']}")
    assert errs[0] <= 1e-5 and max(errs[1:]) <= 1e-8

    a, b = (V.bootstrap_factors(x, n_resamples=8, random_state=5) for x in (m, twin))
    rep = _in_place(c, "bootstrap_report_", kind, ["cmtfpls_kfold_weighted_xcov_*", "cmtfpls_kfold_epilogue_weighted_f64"], "kfold_weighted_xcov")
    fa, fb = (a["X_factors"], b["X_factors"]) if which == "ctPLS" else ([a["X_factors"]], [b["X_factors"]])
    errs = [_colwise(p, q) for ba, bb in zip(fa, fb) for p, q in zip(ba, bb)] + [_colwise(a["Y_loadings"], b["Y_loadings"]), _colwise(a["coef"], b["coef"])]
    print(f"{which} {kind} bootstrap_factors: {max(errs):.3g}, oob_q2y {np.abs(a['oob_q2y'] - b['oob_q2y']).max():.3g}; "
          f"n_iter equal {rep['n_iter'] == twin.bootstrap_report_['n_iter']}")
    assert max(errs) <= 1e-5 and np.abs(a["oob_q2y"] - b["oob_q2y"]).max() <= 1e-8


@pytest.mark.parametrize("kind", HS.KINDS)
def test_order_4_in_place(api, kind):
    c = _case(api, "order-4", kind, tensor_folds=True)
    rep = _kfold_check(c, "order-4", kind, ["cmtfpls_kfold_xcov_*", "cmtfpls_kfold_inner_tensor_f64"])
    assert "rank1" in rep and rep["half_storage"]["in_place"], rep


@pytest.mark.parametrize("kind", HS.KINDS)
def test_option_off_is_the_float32_twin_bit_for_bit(api, kind):
    c = _case(api, "tPLS", kind, half_folds=False)
    q, qt = V.get_q2y_kfold(c["m"], n_splits=K, per_component=True), V.get_q2y_kfold(c["twin"], n_splits=K, per_component=True)
    rep = c["m"].q2y_report_
    assert rep["storage_fallback"].startswith(f"float32 private copy of the {HS.NAMES[kind]} data: ") and "half_storage" not in rep, rep
    assert "cmtfpls_kfold_xcov_*" in rep["form"] and np.array_equal(np.asarray(q), np.asarray(qt))
    assert rep["form"] == c["twin"].q2y_report_["form"] and rep["n_iter"] == c["twin"].q2y_report_["n_iter"]


def test_routes_that_still_upcast_under_the_option(api):
    c = _case(api, "tPLS", "f16")
    phrase = "float32 private copy of the float16 data: "
    V.get_q2y(c["m"])                                                              # leave-one-out: cmtfpls_loo_* take float64 X
    rep = c["m"].q2y_report_
    assert "loo" in rep["form"] and rep["storage_fallback"].startswith(phrase) and "leave-one-out" in rep["storage_fallback"], rep
    assert "half_storage" not in rep
    gap = c["X16"][0].clone()
    gap[7, 3, 4] = float("nan")
    m = api.tPLS(R, dtype="float16", algorithm="xcov", options=EngineOptions(small_fit=False, half_folds=True, masked_folds=True))
    m.fit(gap, c["y"])
    V.get_q2y_kfold(m, n_splits=K)
    rep = m.q2y_report_
    assert "cmtfpls_cv_masked_f64" in rep["form"], rep
    assert rep["storage_fallback"].startswith(phrase) and "masked" in rep["storage_fallback"] and "half_storage" not in rep, rep


def test_no_float32_copy_is_made(api):
    """(16384, 64, 64) bfloat16: X is 128 MiB, the float32 copy that must not exist 256 MiB.  The rise of the peak allocation during
    get_q2y_kfold stays below I P 4 bytes; the float32 twin's own rise on its in-place tensor (the same workspaces) is below half of
    that, so the condition separates the two routes."""
    I, A, B = 16384, 64, 64
    g = torch.Generator(device=DEV).manual_seed(11)
    T = torch.randn(I, R, device=DEV, generator=g) * torch.tensor([1.0, 0.5, 0.25], device=DEV)
    X32 = torch.einsum("il,jl,kl->ijk", T, torch.randn(A, R, device=DEV, generator=g), torch.randn(B, R, device=DEV, generator=g))
    X32 += 0.05 * torch.randn(I, A, B, device=DEV, generator=g)
    y = (T.double() @ torch.randn(R, M, device=DEV, generator=g).double()).cpu().numpy()
    X16 = X32.to(torch.bfloat16)
    X32 = X16.to(torch.float32)
    copy = I * A * B * 4
    rises = {}
    for name, X, dtype in (("bfloat16 in place", X16, "bfloat16"), ("float32 twin", X32, "float32")):
        m = api.tPLS(R, dtype=dtype, algorithm="xcov", options=EngineOptions(small_fit=False, half_folds=True))
        m.fit(X, y)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        V.get_q2y_kfold(m, n_splits=K)
        torch.cuda.synchronize()
        rises[name] = torch.cuda.max_memory_allocated() - base
        rep = m.q2y_report_
        assert "cmtfpls_kfold_xcov_*" in rep["form"] and "storage_fallback" not in rep, rep
        assert ("half_storage" in rep) == (dtype == "bfloat16")
        del m
    print(f"peak rise during get_q2y_kfold: {rises} bytes; the float32 copy would be {copy}")
    assert rises["float32 twin"] < copy // 2
    assert rises["bfloat16 in place"] < copy
