"""CPU-only: cross-validation of a ctPLS with missing values under EngineOptions.masked_folds_coupled on a backend without
cmtfpls_cv_masked_coupled_f64 (the NumPy test backend: refits with a why that names the form, results equal to the option off),
that masked_folds alone leaves a ctPLS untouched, the count-weighted coupled arithmetic of one model pinned against the oracle on
literally duplicated rows (coupled_masked_ref), and the limits the C entry declares -- checked before it touches a pointer or the
GPU -- with the host's LDS formula against the library's."""
import ctypes

import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.validate import bootstrap_factors, get_q2y_kfold, get_q2y_repeated_kfold, kfold_predictions, permutation_test_q2y
from coupled_masked_ref import coupled_masked_fit
from numpy_backend import NumpyBackend

FORM = "cmtfpls_cv_masked_coupled_f64"
LDS_CAP = 150 * 1024


def _coupled_data(shapes, M, L, seed, nan=(0.1,)):
    """Blocks with the given shapes (rows first, shared) driven by one latent score, a Y of M responses; nan[b] of block b's
    entries missing (the last value repeats), every row keeping an observed entry in every block."""
    rng = np.random.default_rng(seed)
    I = shapes[0][0]
    T = rng.standard_normal((I, L))
    Xs = []
    for b, shape in enumerate(shapes):
        X = O.cp_factors_to_tensor([T] + [rng.standard_normal((d, L)) for d in shape[1:]]) + 0.3 * rng.standard_normal(shape)
        frac = nan[min(b, len(nan) - 1)]
        if frac:
            hole = rng.random(shape) < frac
            hole.reshape(I, -1)[:, b % int(np.prod(shape[1:]))] = False
            X[hole] = np.nan
        Xs.append(X)
    Y = T @ rng.standard_normal((L, M)) + 0.3 * rng.standard_normal((I, M))
    return Xs, Y


def _pair(Xs, y, R, **on):
    a = ctPLS(R, backend=NumpyBackend(), options=EngineOptions(small_fit=False, **on))
    b = ctPLS(R, backend=NumpyBackend(), options=EngineOptions(small_fit=False))
    a.fit(Xs, y)
    b.fit(Xs, y)
    return a, b


def _declined(rep):
    assert f"the masked form ({FORM}) declined" in rep["why"], rep
    assert "numpy-test backend has no coupled masked model kernel" in rep["why"], rep


def test_the_option_is_a_new_field_and_off_by_default():
    assert EngineOptions().masked_folds_coupled is False
    assert EngineOptions().masked_folds is False
    assert EngineOptions(masked_folds=True).masked_folds_coupled is False


def test_kfold_without_the_kernel_refits_with_a_why():
    Xs, y = _coupled_data([(18, 4, 3), (18, 5)], 2, 3, seed=3)
    on, off = _pair(Xs, y, 2, masked_folds_coupled=True)
    got = kfold_predictions(on, n_splits=3)
    _declined(on.q2y_report_)
    assert on.q2y_report_["form"] == "one refit per fold on the regular engine"
    want = kfold_predictions(off, n_splits=3)
    np.testing.assert_array_equal(got, want)
    assert FORM not in off.q2y_report_["why"]
    np.testing.assert_array_equal(get_q2y_kfold(on, n_splits=18), get_q2y_kfold(off, n_splits=18))      # leave-one-out
    _declined(on.q2y_report_)


def test_permutation_without_the_kernel_refits_with_a_why():
    Xs, y = _coupled_data([(16, 4, 3), (16, 5)], 2, 3, seed=4)
    on, off = _pair(Xs, y, 2, masked_folds_coupled=True)
    got = permutation_test_q2y(on, n_permutations=3, n_splits=4, per_component=True)
    _declined(on.q2y_report_)
    assert on.q2y_report_["form"] == "one refit per fold and permutation on the regular engine"
    want = permutation_test_q2y(off, n_permutations=3, n_splits=4, per_component=True)
    assert off.q2y_report_["why"] == "coupled model: permutation device form not built"
    np.testing.assert_array_equal(got["null"], want["null"])
    np.testing.assert_array_equal(got["p_value"], want["p_value"])


def test_repeated_and_bootstrap_without_the_kernel_refit_with_a_why():
    Xs, y = _coupled_data([(15, 5), (15, 3, 4)], 2, 3, seed=5)
    on, off = _pair(Xs, y, 2, masked_folds_coupled=True)
    got = get_q2y_repeated_kfold(on, n_splits=3, n_repeats=2, per_component=True)
    _declined(on.q2y_report_)
    assert on.q2y_report_["form"] == "one refit per fold and split on the regular engine"
    want = get_q2y_repeated_kfold(off, n_splits=3, n_repeats=2, per_component=True)
    np.testing.assert_array_equal(got["q2y"], want["q2y"])
    got = bootstrap_factors(on, n_resamples=3)
    _declined(on.bootstrap_report_)
    assert on.bootstrap_report_["form"] == "one refit per resample on the regular engine"
    want = bootstrap_factors(off, n_resamples=3)
    np.testing.assert_array_equal(got["coef"], want["coef"])
    np.testing.assert_array_equal(got["oob_q2y"], want["oob_q2y"])


def test_masked_folds_alone_leaves_a_coupled_model_untouched():
    Xs, y = _coupled_data([(16, 4, 3), (16, 5)], 2, 3, seed=6)
    on, off = _pair(Xs, y, 2, masked_folds=True)
    np.testing.assert_array_equal(kfold_predictions(on, n_splits=4), kfold_predictions(off, n_splits=4))
    assert on.q2y_report_ == off.q2y_report_ and FORM not in str(on.q2y_report_)
    permutation_test_q2y(on, n_permutations=2, n_splits=4)
    assert on.q2y_report_["why"] == "coupled model: permutation device form not built"
    get_q2y_repeated_kfold(on, n_splits=4, n_repeats=2)
    assert FORM not in str(on.q2y_report_)
    bootstrap_factors(on, n_resamples=2)
    assert FORM not in str(on.bootstrap_report_)


def test_complete_blocks_keep_their_routing_under_the_option():
    Xs, y = _coupled_data([(16, 4, 3), (16, 5)], 2, 3, seed=7, nan=(0.0,))
    on, off = _pair(Xs, y, 2, masked_folds_coupled=True)
    np.testing.assert_array_equal(kfold_predictions(on, n_splits=4), kfold_predictions(off, n_splits=4))
    assert on.q2y_report_ == off.q2y_report_ and FORM not in str(on.q2y_report_)


# ---- the weighted coupled arithmetic against the oracle on duplicated rows --------------------------------------------------------
def _col_rel(got, want):
    """Worst relative error per column (last axis), normwise."""
    got, want = np.asarray(got), np.asarray(want)
    return float(max(np.linalg.norm(got[..., j] - want[..., j]) / np.linalg.norm(want[..., j]) for j in range(want.shape[-1])))


@pytest.mark.parametrize("nan,info0", [((0.1, 0.1), 3), ((0.1, 0.0), 1), ((0.0, 0.1), 2), ((0.0, 0.0), 0)])
@pytest.mark.parametrize("yperm", [False, True])
def test_weighted_arithmetic_equals_the_oracle_on_duplicated_rows(nan, info0, yperm):
    I, R = 30, 3
    Xs, y = _coupled_data([(I, 6, 5), (I, 7)], 2, R + 1, seed=30, nan=nan)
    rng = np.random.default_rng(I + 1)
    c = rng.integers(0, 4, size=I)
    c[:3] = 0                                                                  # at least three rows held out
    c[3] = 2                                                                   # a duplicated row (holding NaN where the block has any)
    for X, frac in zip(Xs, nan):
        if frac:
            X[3].flat[1] = np.nan
        assert (~np.isnan(X).reshape(I, -1)).sum(axis=1).min() >= 1            # every row observed in every block
    yrow = rng.permutation(I) if yperm else None
    loadings, Q, coef, pred, n_iter, info = coupled_masked_fit(Xs, y, c, R, yrow)
    assert info[0] == info0
    dup = np.repeat(np.arange(I), c)
    yp = y[np.arange(I) if yrow is None else yrow]
    fit = O.fit_ctpls([X[dup] for X in Xs], yp[dup], R)
    assert fit.has_miss == [bool(f) for f in nan]
    assert n_iter == fit.n_iter
    for b in range(2):
        for L, Lw in zip(loadings[b], fit.loadings[b]):
            assert _col_rel(L, Lw) <= 1e-12
    assert _col_rel(Q, fit.Q) <= 1e-12
    assert np.abs(coef - fit.coef).max() <= 1e-12 * np.abs(fit.coef).max()
    assert np.isfinite(pred).all() and pred.shape == (R, int((c == 0).sum()), 2)


def test_one_block_is_the_tpls_restatement():
    from weighted_masked_ref import weighted_masked_fit
    Xs, y = _coupled_data([(24, 5, 4)], 3, 4, seed=24)
    c = np.random.default_rng(1).integers(0, 3, size=24)
    c[:4] = 0
    got = coupled_masked_fit(Xs, y, c, 3)
    want = weighted_masked_fit(Xs[0], y, c, 3)
    for L, Lw in zip(got[0][0], want[0]):
        np.testing.assert_array_equal(L, Lw)
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    np.testing.assert_array_equal(got[3], want[3])
    assert got[4] == want[4]


# ---- the limits of the C entry ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from cmtf_pls_amd import _lib
    return _lib.load()


def _blocks(dims, orders=None):
    from cmtf_pls_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    orders = orders or [2 if A == 1 else 3 for A, _ in dims]
    arr = (_lib.CvCoupledBlock * len(dims))(*[_lib.CvCoupledBlock(p, o, A, B) for o, (A, B) in zip(orders, dims)])
    arr._keep = buf
    return arr, p


def _probe(lib, dims, I, M, R, nm=3, orders=None):
    """The entry's answer to a shape, with stand-in pointers and no workspace: 4 = declined, 2 = accepted (only the workspace
    is missing).  Neither touches a pointer."""
    arr, p = _blocks(dims, orders)
    return lib.cmtfpls_cv_masked_coupled_f64(arr, len(dims), p, p, None, nm, I, M, R, 1e-8, 100, 0, 1, p, None, None, None, None, None,
                                             p, None, None, 0, None)


def test_c_entry_limits(lib):
    from cmtf_pls_amd.kfold import MAX_BLOCKS
    assert MAX_BLOCKS == 8
    assert _probe(lib, [(64, 64), (1, 7)], 40, 2, 2) == 2              # min(A, B) = 64
    assert _probe(lib, [(6, 5), (65, 65)], 8, 2, 1) == 4
    assert _probe(lib, [(6, 5), (1, 7)], 40, 64, 2) == 2               # M = 64
    assert _probe(lib, [(6, 5), (1, 7)], 40, 65, 2) == 4
    assert _probe(lib, [(6, 5), (1, 7)], 40, 2, 16) == 2               # R = 16
    assert _probe(lib, [(6, 5), (1, 7)], 40, 2, 17) == 4
    assert _probe(lib, [(3, 2)] * 8, 40, 2, 2) == 2                    # nb = 8
    assert _probe(lib, [(3, 2)] * 9, 40, 2, 2) == 4
    assert _probe(lib, [(6, 5), (1, 7)], 40, 2, 2, orders=[3, 2]) == 2
    assert _probe(lib, [(6, 5), (1, 7)], 40, 2, 2, orders=[4, 2]) == 4  # an order-4 block
    dims = [(1, 3000), (6, 5)]
    I = 2
    while lib.cmtfpls_cv_masked_coupled_lds_bytes(_blocks(dims)[0], 2, I + 1, 2, 1) <= LDS_CAP:
        I += 1
    assert _probe(lib, dims, I, 2, 1) == 2                             # the LDS at its cap
    assert _probe(lib, dims, I + 1, 2, 1) == 4
    assert _probe(lib, [(6, 5)], 40, 2, 2, nm=0) == 1                  # no models: a bad argument
    assert _probe(lib, [(6, 5), (2, 7)], 40, 2, 2, orders=[3, 2]) == 1   # a matrix block has A = 1
    arr, _ = _blocks([(6, 5), (1, 7)])
    assert lib.cmtfpls_cv_masked_coupled_workspace_bytes(arr, 2, 40, 3, 2) == 8 * (40 * 30 + 2 * 30 + 40 * 7 + 2 * 7 + 40 * 3 + 40 * 2)
    assert lib.cmtfpls_cv_masked_coupled_workspace_bytes(arr, 2, 1, 3, 2) == 0
    assert lib.cmtfpls_cv_masked_coupled_workspace_bytes(arr, 9, 40, 3, 2) == 0


def _carve_up(dims, I, M, R):
    """The LDS of a workgroup as include/cmtfpls.h states it (doubles): the per-block scratch is shared, sized for the largest block."""
    Pmax, nmax, kmax = max(A * B for A, B in dims), max(min(d) for d in dims), max(max(d) for d in dims)
    return 8 * (3 * I + 3 * M + 2 * R * R + R * M + 3 * R + 256 + Pmax + 2 * nmax * nmax + nmax + kmax
                + sum((R + 1) * (A + B) + I for A, B in dims))


def test_host_lds_formula_is_the_librarys(lib):
    rng = np.random.default_rng(0)
    seen = set()
    for _ in range(300):
        nb = int(rng.integers(1, 9))
        dims = [(1, int(rng.integers(1, 2500))) if rng.random() < 0.4 else (int(rng.integers(1, 65)), int(rng.integers(1, 90)))
                for _ in range(nb)]
        I, M, R = int(rng.integers(2, 1500)), int(rng.integers(1, 65)), int(rng.integers(1, 17))
        arr, _ = _blocks(dims)
        want = _carve_up(dims, I, M, R)
        assert lib.cmtfpls_cv_masked_coupled_lds_bytes(arr, nb, I, M, R) == want
        fits = all(min(d) <= 64 for d in dims) and want <= LDS_CAP
        assert _probe(lib, dims, I, M, R) == (2 if fits else 4), (dims, I, M, R)
        seen.add(fits)
    assert seen == {True, False}
    # one block: the formula of cmtfpls_cv_masked_models_f64 (tests/test_cv_masked_models_cpu.py)
    I, A, B, M, R = 40, 6, 5, 3, 2
    n, k, P = min(A, B), max(A, B), A * B
    assert lib.cmtfpls_cv_masked_coupled_lds_bytes(_blocks([(A, B)])[0], 1, I, M, R) == 8 * (2 * I + P + A + B + 2 * M + 2 * n * n + n + k + M + R * R + R * (A + B) +
        R * M + R * R + 3 * R + 256 + 2 * I)
