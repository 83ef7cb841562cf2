"""Sparse fits on the GPU against the float64 mirror (tests/sparse_ref.py: the oracle with its extraction swapped for the
soft-thresholded rule) on inputs screened on the CPU (sparse_ref.CASES; tests/test_sparse_cpu.py asserts the margins).

float64 storage: factors and coef_ within 1e-9 normwise, R2X / R2Y within 1e-11, equal n_iter_, equal zero patterns,
no unconverged extraction, the switched-off fused forms named; transform / predict of new rows against oracle.transform / predict
on the mirror fit.  One float32-storage case at the project's f32 guard (1e-6 normwise).  K-fold Q2Y of a sparse
model equals a literal loop of sparse refits."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import oracle as O  # noqa: E402
import sparse_ref as S  # noqa: E402
from test_sparse_cpu import check_against_mirror  # noqa: E402

pytestmark = pytest.mark.gpu

_REF = {}


def _case(name):
    """The case's data and its mirror fit, computed once and shared (never modified)."""
    if name not in _REF:
        blocks, y, sparsity = S.case_data(name)
        _REF[name] = (blocks, y, sparsity, S.mirror_fit(blocks, y, sparsity, tol=S.case_tol(name)))
    return _REF[name]


def _fit(name, algorithm, dtype="float64", blocks=None):
    from cmtf_pls_amd import ctPLS, tPLS
    bl, y, sparsity, ref = _case(name)
    bl = bl if blocks is None else blocks
    if len(bl) > 1:
        m = ctPLS(S.N_COMP, dtype=dtype, algorithm=algorithm, sparsity=sparsity)
        m.fit([b.copy() for b in bl], y.copy(), tol=S.case_tol(name))
    else:
        m = tPLS(S.N_COMP, dtype=dtype, algorithm=algorithm, sparsity=sparsity)
        m.fit(bl[0].copy(), y.copy(), tol=S.case_tol(name))
    return m, ref


def _report_checks(m, algorithm, n_blocks):
    rep = m.fit_report_
    sp = rep["sparse"]
    assert rep["backend"] == "hip" and rep["form"] == "regular"
    assert sp["unconverged"] == 0 and 1 <= sp["sweeps_max"] <= 200 and sp["sweeps_total"] >= sum(m.n_iter_)
    assert len(sp["nonzeros"]) == n_blocks and len(sp["form"]) == n_blocks
    declined = " ".join(rep["declined"])
    assert "small_fit" in declined
    if algorithm == "direct":
        assert "fused direct iteration" in declined and rep["y_side"] == "separate launches"
    else:
        assert "xcov_iterate" in declined and "xcov_blocks_plan" in declined and "pipelined" in declined and rep["pipelined"] is False


@pytest.mark.parametrize("algorithm", ["direct", "xcov"])
@pytest.mark.parametrize("name", ["tpls_02", "tpls_05"])
def test_tpls_against_the_mirror(name, algorithm):
    m, ref = _fit(name, algorithm)
    check_against_mirror(m, ref)
    _report_checks(m, algorithm, 1)
    assert m.fit_report_["sparse"]["form"] == [1]
    nz = m.fit_report_["sparse"]["nonzeros"][0]
    assert nz[0] == [int(v) for v in (ref.loadings[0][0] != 0).sum(0)] and nz[1] == [int(v) for v in (ref.loadings[0][1] != 0).sum(0)]
    assert any(v < d for L, d in zip(nz, (12, 9)) for v in L)                      # the model IS sparse
    x = _case(name)[0][0]
    new = x[:9] * 1.1 + 0.05                                                       # new rows
    np.testing.assert_allclose(m.transform(new), O.transform(ref, new), rtol=0, atol=1e-9 * np.abs(O.transform(ref, new)).max())
    np.testing.assert_allclose(m.predict(new), O.predict(ref, new), rtol=0, atol=1e-9 * np.abs(O.predict(ref, new)).max())


def test_tpls_with_missing_values_direct():
    m, ref = _fit("tpls_nan", "direct")
    assert m.X_hasMiss
    check_against_mirror(m, ref)
    _report_checks(m, "direct", 1)


@pytest.mark.parametrize("algorithm", ["direct", "xcov"])
def test_ctpls_against_the_mirror(algorithm):
    m, ref = _fit("ctpls", algorithm)
    check_against_mirror(m, ref, 0, coupled=True)
    check_against_mirror(m, ref, 1, coupled=True)
    _report_checks(m, algorithm, 2)
    sp = m.fit_report_["sparse"]
    assert sp["lambda"] == [(0.2, 0.2), (0.3,)] and sp["form"] == [1, None]
    assert (m.Xs_factors[1][1] == 0).any()                                         # the matrix block's loading is sparse too
    blocks = _case("ctpls")[0]
    new = [b[:9] * 1.1 for b in blocks]
    np.testing.assert_allclose(m.transform(new), O.transform(ref, new), rtol=0, atol=1e-9 * np.abs(O.transform(ref, new)).max())
    np.testing.assert_allclose(m.predict(new), O.predict(ref, new), rtol=0, atol=1e-9 * np.abs(O.predict(ref, new)).max())


def test_float32_storage():
    """X rounded to float32 once, so that the mirror and the model see the same data; the engine then centres and deflates in
    float32 storage: the project's f32 guard, 1e-6 normwise, R2 to 1e-6."""
    blocks, y, sparsity, _ = _case("tpls_02")
    x32 = blocks[0].astype(np.float32).astype(np.float64)
    ref = S.mirror_fit([x32], y, sparsity, tol=S.case_tol("tpls_02"))
    m, _ = _fit("tpls_02", "direct", dtype="float32", blocks=[x32])
    assert m.fit_report_["storage"] == ["float32"]
    check_against_mirror(m, ref, bound=1e-6, r2=1e-6)
    assert m.fit_report_["sparse"]["unconverged"] == 0


def test_lambda_zero_is_the_dense_model_on_the_device():
    from cmtf_pls_amd import tPLS
    blocks, y, _, _ = _case("tpls_02")
    dense = tPLS(S.N_COMP, dtype="float64")
    dense.fit(blocks[0].copy(), y.copy())
    m = tPLS(S.N_COMP, dtype="float64", sparsity=0.0)
    m.fit(blocks[0].copy(), y.copy())
    assert list(m.n_iter_) == list(dense.n_iter_) and "sparse" not in dense.fit_report_
    for got, want in zip(m.X_factors, dense.X_factors):
        assert np.linalg.norm(got - want) <= 1e-9 * np.linalg.norm(want)
    assert np.linalg.norm(m.coef_ - dense.coef_) <= 1e-9 * np.linalg.norm(dense.coef_)
    np.testing.assert_allclose(m.R2X, dense.R2X, rtol=0, atol=1e-11)
    np.testing.assert_allclose(m.R2Y, dense.R2Y, rtol=0, atol=1e-11)


def test_kfold_q2y_equals_a_literal_loop_of_sparse_refits():
    from cmtf_pls_amd import tPLS
    from cmtf_pls_amd.validate import get_q2y_kfold
    blocks, y, sparsity, _ = _case("tpls_02")
    x = blocks[0]
    m, _ = _fit("tpls_02", "direct")
    got = get_q2y_kfold(m, n_splits=4, per_component=True)
    assert "sparse" in m.q2y_report_["why"] and m.q2y_report_["form"].startswith("one refit per fold")
    I = x.shape[0]
    sizes = np.full(4, I // 4)
    sizes[: I % 4] += 1
    ids = np.repeat(np.arange(4), sizes)
    pred = np.zeros((S.N_COMP,) + y.shape)
    for k in range(4):
        test = ids == k
        r = tPLS(S.N_COMP, dtype="float64", sparsity=sparsity)
        r.fit(x[~test].copy(), y[~test].copy())
        assert r.fit_report_["sparse"]["lambda"] == [tuple(sparsity)]
        scores = r.transform(x[test])
        for c in range(1, S.N_COMP + 1):
            pred[c - 1, test] = scores[:, :c] @ r.coef_[:c, :c] @ r.Y_factors[1][:, :c].T + r.Y_mean
    want = 1.0 - ((pred - y) ** 2).reshape(S.N_COMP, -1).sum(axis=1) / (y ** 2).sum()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
