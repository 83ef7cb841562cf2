"""Sparse loadings without a GPU: the engine's control flow on the NumPy test backend against the float64 mirror
(tests/sparse_ref.py: the oracle with its extraction swapped for the soft-thresholded rule), lambda = 0 against the dense model,
the routes of the resampling family, construction and limits, and a world-size-2 gloo fit.

Bounds: the project's float64-storage bounds: factors and coef_ within 1e-9 normwise, R2X / R2Y within 1e-11.  The
seeds are screened here, on the CPU, as the suite does elsewhere: no convergence norm within 10x of tol at a stopping iteration
or the one before, no pre-threshold magnitude within 1e-6 relative of theta in an extraction's final sweep (`sparse_ref.screen_case`)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import oracle as O  # noqa: E402
from cmtf_pls_amd import ctPLS, tPLS  # noqa: E402
import sparse_ref as S  # noqa: E402
from sparse_ref import SparseNumpyBackend  # noqa: E402

SHAPE, R = (60, 12, 9), S.N_COMP
LAMS = [(0.2, 0.2), (0.5, 0.3)]
CASE_OF = {(0.2, 0.2): "tpls_02", (0.5, 0.3): "tpls_05"}
TOL = 1e-8


def _data(seed=1, shape=SHAPE):
    x, y, _ = O.import_synthetic(shape, 3, R, error=0.1, seed=seed)
    return x, y


def _norm_close(got, want, bound):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300)
    assert err <= bound, err


def _align(loads, ref_loads):
    """The paired sign of every component (wA, wB) -> (-wA, -wB) leaves the model unchanged: align it with the reference's."""
    loads = [np.array(L, copy=True) for L in loads]
    if len(loads) == 2:
        for a in range(loads[0].shape[1]):
            if np.dot(loads[1][:, a], ref_loads[1][:, a]) < 0:
                loads[0][:, a] *= -1.0
                loads[1][:, a] *= -1.0
    return loads


def check_against_mirror(m, ref, block=0, coupled=False, bound=1e-9, r2=1e-11):
    loads = (m.Xs_factors[block] if coupled else m.X_factors)[1:]
    T = m.factor_T if coupled else m.X_factors[0]
    _norm_close(T, ref.T, bound)
    for got, want in zip(_align(loads, ref.loadings[block]), ref.loadings[block]):
        _norm_close(got, want, bound)
        assert np.array_equal(got == 0.0, want == 0.0)                       # the zero pattern of every loading column
    _norm_close(m.Y_factors[0], ref.U, bound)
    _norm_close(m.Y_factors[1], ref.Q, bound)
    _norm_close(m.coef_, ref.coef, bound)
    np.testing.assert_allclose(m.R2Xs[block] if coupled else m.R2X, ref.r2x[block], rtol=0, atol=r2)
    np.testing.assert_allclose(m.R2Y, ref.r2y, rtol=0, atol=r2)
    assert list(m.n_iter_) == list(ref.n_iter)


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_cases_are_screened(name):
    """The margins the comparisons of n_iter_ and of the zero patterns rely on, here and on the GPU, checked rather than assumed."""
    blocks, y, sparsity = S.case_data(name)
    margin, tol_ok, converged = S.screen_case(blocks, y, sparsity, tol=S.case_tol(name))
    assert margin > S.THETA_MARGIN, margin
    assert tol_ok and converged


def test_kernel_inputs_are_screened():
    """Every input of tests/test_gpu_sparse_kernels.py: the theta margin at the sweep counts it uses, convergence at the default
    tolerance, and the tie of the "tie" variant."""
    for shape in S.KERNEL_SHAPES:
        for variant in ("plain", "zero_row", "tie"):
            Z = S.kernel_case(shape, variant)
            pair = S.dense_pair(Z)
            if variant == "tie":
                top = int(np.argmax(np.abs(Z @ pair[1])))
                assert sum(np.array_equal(Z[top], row) for row in Z) == 2
            for lams in S.KERNEL_LAMS:
                for tol_s, sweeps in ((0.0, 1), (0.0, 5), (1e-10, 200)):
                    st = {}
                    S.sparse_rank1(Z, lams, tol_s, sweeps, dense=lambda z: pair, stats=st)
                    assert all(m > S.THETA_MARGIN for m in st["margins"])
                    assert tol_s == 0.0 or (st["info"][0] == 1 and st["info"][1] <= 22)


@pytest.mark.parametrize("algorithm", ["direct", "xcov"])
@pytest.mark.parametrize("lams", LAMS)
def test_engine_matches_the_mirror(lams, algorithm):
    name = CASE_OF[lams]
    blocks, y, _ = S.case_data(name)
    x, tol = blocks[0], S.case_tol(name)
    ref = S.mirror_fit(blocks, y, lams, tol=tol)
    m = tPLS(R, backend=SparseNumpyBackend(), algorithm=algorithm, sparsity=lams)
    m.fit(x, y, tol=tol)
    check_against_mirror(m, ref)
    rep = m.fit_report_
    sp = rep["sparse"]
    assert sp["lambda"] == [tuple(lams)] and sp["unconverged"] == 0 and 1 <= sp["sweeps_max"] <= 200
    assert sp["nonzeros"][0][0] == [int(v) for v in (ref.loadings[0][0] != 0).sum(0)]
    assert sp["nonzeros"][0][1] == [int(v) for v in (ref.loadings[0][1] != 0).sum(0)]
    assert min(sp["nonzeros"][0][0] + sp["nonzeros"][0][1]) >= 1                 # at least one entry always survives
    assert any(v < d for L, d in zip(sp["nonzeros"][0], SHAPE[1:]) for v in L)  # and the model IS sparse
    declined = " ".join(rep["declined"])
    assert "small_fit" in declined and ("fused direct" in declined if algorithm == "direct" else "xcov_iterate" in declined and "pipelined" in declined)
    if algorithm == "xcov":
        assert rep["pipelined"] is False
    # transform / predict read the factors: they work on a sparse model as they are
    np.testing.assert_allclose(m.transform(x[:7]), O.transform(ref, x[:7]), rtol=0, atol=1e-9)
    np.testing.assert_allclose(m.predict(x[:7]), O.predict(ref, x[:7]), rtol=0, atol=1e-9)


@pytest.mark.parametrize("algorithm", ["direct", "xcov"])
def test_lambda_zero_is_the_dense_model(algorithm):
    blocks, y, _ = S.case_data("tpls_02")
    x = blocks[0]
    dense = tPLS(R, backend=SparseNumpyBackend(), algorithm=algorithm)
    dense.fit(x, y, tol=TOL)
    m = tPLS(R, backend=SparseNumpyBackend(), algorithm=algorithm, sparsity=0.0)
    m.fit(x, y, tol=TOL)
    assert list(m.n_iter_) == list(dense.n_iter_)
    for got, want in zip(m.X_factors, dense.X_factors):
        _norm_close(got, want, 1e-9)
    _norm_close(m.coef_, dense.coef_, 1e-9)
    np.testing.assert_allclose(m.R2X, dense.R2X, rtol=0, atol=1e-11)
    np.testing.assert_allclose(m.R2Y, dense.R2Y, rtol=0, atol=1e-11)
    assert "sparse" not in dense.fit_report_ and dense.sparsity is None


def test_matrix_block_and_coupled_model():
    (x, xm), y, sparsity = S.case_data("ctpls")
    ref = S.mirror_fit([x, xm], y, sparsity, tol=S.case_tol("ctpls"))
    for algorithm in ("direct", "xcov"):
        m = ctPLS(R, backend=SparseNumpyBackend(), algorithm=algorithm, sparsity=sparsity)
        m.fit([x, xm], y, tol=S.case_tol("ctpls"))
        check_against_mirror(m, ref, 0, coupled=True)
        check_against_mirror(m, ref, 1, coupled=True)
        assert m.fit_report_["sparse"]["lambda"] == [(0.2, 0.2), (0.3,)] and m.fit_report_["sparse"]["form"] == [1, None]
        assert (m.Xs_factors[1][1] == 0).any()


# ---- routes ------------------------------------------------------------------------------------------------------------------
class _Spy(SparseNumpyBackend):
    """No fold, leave-one-out or masked entry may be reached by a sparse model: any attribute of those families raises."""
    FAMILIES = ("kfold", "loo_", "cv_masked", "masked_", "press")

    def __getattr__(self, name):
        if any(name.startswith(f) or f in name for f in _Spy.FAMILIES):
            raise AssertionError(f"a sparse model reached the device entry {name}")
        raise AttributeError(name)


def _fitted(spy=True, **kw):
    x, y = _data(shape=(24, 6, 5))
    m = tPLS(2, backend=_Spy() if spy else SparseNumpyBackend(), sparsity=(0.2, 0.3), **kw)
    m.fit(x, y)
    return m, x, y


def test_every_resampling_route_declines_with_a_sparse_why(monkeypatch):
    from cmtf_pls_amd import bootstrap, kfold, nested, permutation, repeated, validate
    m, x, y = _fitted()
    assert kfold._route(m, x, True) == (kfold.REFIT, kfold.SPARSE_WHY) and "sparse" in kfold.SPARSE_WHY
    assert kfold._route(m, x, True, masked=False)[0] == kfold.REFIT
    assert validate._loo_device(m, 1e-8, 100) == (None, kfold.SPARSE_WHY)
    # every refit model carries the sparsity
    built = []
    real_init = tPLS.__init__

    def spy_init(self, *a, **k):
        real_init(self, *a, **k)
        built.append(self.sparsity)
    monkeypatch.setattr(tPLS, "__init__", spy_init)
    validate.get_q2y_kfold(m, n_splits=3)
    assert "sparse" in m.q2y_report_["why"] and m.q2y_report_["form"].startswith("one refit per fold")
    validate.get_q2y(m)
    assert "sparse" in m.q2y_report_["why"]
    repeated.repeated_kfold(m, n_splits=3, n_repeats=2)
    assert "sparse" in m.q2y_report_["why"]
    permutation.permutation_test(m, n_permutations=2, n_splits=3)
    assert "sparse" in m.q2y_report_["why"]
    nested.nested_kfold(m, n_outer=3, n_inner=2)
    assert "sparse" in m.q2y_report_["why"]
    validate.bootstrap_factors(m, n_resamples=2)
    assert "sparse" in m.bootstrap_report_["why"]
    assert built and all(s == (0.2, 0.3) for s in built)


def test_coupled_routes_and_refits_carry_sparsity(monkeypatch):
    from cmtf_pls_amd import kfold, validate
    x, y = _data(shape=(24, 6, 5))
    xm = np.random.default_rng(1).normal(size=(24, 7))
    m = ctPLS(2, backend=_Spy(), sparsity=[(0.2, 0.3), 0.1])
    m.fit([x, xm], y)
    assert validate._loo_device_coupled(m, 1e-8, 100) == (None, kfold.SPARSE_WHY)
    built = []
    real_init = ctPLS.__init__

    def spy_init(self, *a, **k):
        real_init(self, *a, **k)
        built.append(self.sparsity)
    monkeypatch.setattr(ctPLS, "__init__", spy_init)
    validate.get_q2y(m)
    assert "sparse" in m.q2y_report_["why"]
    validate.get_q2y_kfold(m, n_splits=3)
    assert "sparse" in m.q2y_report_["why"]
    assert built and all(s == [(0.2, 0.3), 0.1] for s in built)


def test_q2x_heldout_refit_carries_sparsity():
    from cmtf_pls_amd import imputation
    m, x, y = _fitted(spy=False)
    seen = []
    real_fit = tPLS.fit

    def spy_fit(self, *a, **k):
        seen.append(self.sparsity)
        return real_fit(self, *a, **k)
    tPLS.fit = spy_fit
    try:
        imputation.get_q2x_heldout(m, fraction=0.1, n_repeats=1)
    finally:
        tPLS.fit = real_fit
    assert seen == [(0.2, 0.3)]


# ---- construction and limits -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5, (0.2, 1.0), float("nan"), "0.2"])
def test_lambda_outside_the_unit_interval_raises(bad):
    with pytest.raises(ValueError):
        tPLS(2, backend=SparseNumpyBackend(), sparsity=bad)
    with pytest.raises(ValueError):
        ctPLS(2, backend=SparseNumpyBackend(), sparsity=[bad, 0.1])


def test_graphs_with_sparsity_raises_and_values_are_stored():
    with pytest.raises(ValueError):
        tPLS(2, backend=SparseNumpyBackend(), sparsity=0.2, graphs=True)
    assert tPLS(2, backend=SparseNumpyBackend(), sparsity=0.2).sparsity == 0.2
    assert tPLS(2, backend=SparseNumpyBackend(), sparsity=[0.2, 0.3]).sparsity == (0.2, 0.3)
    assert tPLS(2, backend=SparseNumpyBackend()).sparsity is None
    assert ctPLS(2, backend=SparseNumpyBackend(), sparsity=[(0.2, 0.2), 0.3]).sparsity == [(0.2, 0.2), 0.3]
    assert tPLS(2, backend=SparseNumpyBackend(), graphs=True).sparsity is None           # graphs alone stays what it was


class _NoSweep(SparseNumpyBackend):
    def colstats(self, X2):
        raise AssertionError("a sweep over X ran before the limits were checked")


def test_order4_and_too_large_blocks_raise_before_any_sweep():
    y = np.random.default_rng(0).normal(size=(6, 2))
    with pytest.raises(NotImplementedError):
        tPLS(1, backend=_NoSweep(), sparsity=0.2).fit(np.zeros((6, 3, 4, 5)), y)
    with pytest.raises(ValueError):
        tPLS(1, backend=_NoSweep(), sparsity=0.2).fit(np.zeros((6, 257, 256)), y)        # A * B = 65792 > 65536
    with pytest.raises(ValueError):
        tPLS(1, backend=_NoSweep(), sparsity=0.2).fit(np.zeros((6, 1, 9)), y)            # A = 1 as an order-3 block
    with pytest.raises(ValueError):
        tPLS(1, backend=_NoSweep(), sparsity=(0.2, 0.2, 0.2)).fit(np.zeros((6, 3, 4)), y)  # one lambda too many
    with pytest.raises(ValueError):
        ctPLS(1, backend=_NoSweep(), sparsity=[0.2]).fit([np.zeros((6, 3, 4)), np.zeros((6, 5))], y)


def test_options_carry_the_sweep_defaults():
    from cmtf_pls_amd.engine import EngineOptions
    assert EngineOptions().sparse_tol == 1e-10 and EngineOptions().sparse_max_sweeps == 200
    x, y = _data()
    m = tPLS(R, backend=SparseNumpyBackend(), sparsity=(0.5, 0.3), options=EngineOptions(small_fit=False, sparse_tol=0.0, sparse_max_sweeps=3))
    m.fit(x, y)
    sp = m.fit_report_["sparse"]
    assert sp["sweeps_max"] == 3 and sp["unconverged"] == sum(m.n_iter_) and sp["sweeps_total"] == 3 * sum(m.n_iter_)


# ---- sharded ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, ret):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cmtf_pls_amd.engine import Comm
        blocks, y, _ = S.case_data("tpls_02")
        x = blocks[0]
        rows = slice(rank * 30, (rank + 1) * 30)
        m = tPLS(R, backend=SparseNumpyBackend(), comm=Comm(), sparsity=LAMS[0])
        m.fit(x[rows], y[rows], tol=TOL)
        ret[rank] = {"loads": [L.tobytes() for L in m.X_factors[1:]], "T": m.X_factors[0], "coef": m.coef_, "R2X": m.R2X, "R2Y": m.R2Y,
                     "n_iter": list(m.n_iter_), "sharded": m.fit_report_["sharded"]}
    except Exception as e:  # noqa: BLE001
        import traceback
        ret[rank] = traceback.format_exc() + repr(e)
    finally:
        dist.destroy_process_group()


def test_world2_sparse_fit_is_replicated_and_equals_one_process():
    blocks, y, _ = S.case_data("tpls_02")
    x = blocks[0]
    one = tPLS(R, backend=SparseNumpyBackend(), sparsity=LAMS[0])
    one.fit(x, y, tol=TOL)
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
        out = dict(ret)
    assert all(isinstance(out[r], dict) for r in (0, 1)), out
    assert out[0]["sharded"] and out[0]["loads"] == out[1]["loads"]               # bit-identical on both ranks
    for r in (0, 1):
        loads = [np.frombuffer(b, dtype=np.float64).reshape(L.shape) for b, L in zip(out[r]["loads"], one.X_factors[1:])]
        for got, want in zip(_align(loads, one.X_factors[1:]), one.X_factors[1:]):
            _norm_close(got, want, 1e-9)
            assert np.array_equal(got == 0.0, want == 0.0)
        _norm_close(out[r]["T"], one.X_factors[0][r * 30:(r + 1) * 30], 1e-9)
        _norm_close(out[r]["coef"], one.coef_, 1e-9)
        np.testing.assert_allclose(out[r]["R2X"], one.R2X, rtol=0, atol=1e-11)
        np.testing.assert_allclose(out[r]["R2Y"], one.R2Y, rtol=0, atol=1e-11)
        assert out[r]["n_iter"] == list(one.n_iter_)
