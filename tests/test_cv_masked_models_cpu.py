"""CPU-only: the permutation test, repeated K-fold and the bootstrap with EngineOptions.masked_folds on a backend without
cmtfpls_cv_masked_models_f64 (the NumPy test backend: refits with a why that names the masked form), the weighted arithmetic of one
model pinned against the oracle on literally duplicated rows (weighted_masked_ref), and the limits the C entry declares -- checked
before it touches a pointer or the GPU."""
import ctypes

import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import MODELS_FORM
from cmtf_pls_amd.validate import bootstrap_factors, get_q2y_repeated_kfold, permutation_test_q2y
from numpy_backend import NumpyBackend
from weighted_masked_ref import weighted_masked_fit

ON = EngineOptions(small_fit=False, masked_folds=True)


def _nan_data(shape, M, R, seed, frac=0.1):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=seed)
    x[np.random.default_rng(seed).random(x.shape) < frac] = np.nan
    return x, y


def _pair(x, y, R):
    on = tPLS(R, backend=NumpyBackend(), options=ON)
    off = tPLS(R, backend=NumpyBackend(), options=EngineOptions(small_fit=False))
    on.fit(x, y)
    off.fit(x, y)
    return on, off


def _declined(rep):
    assert f"the masked form ({MODELS_FORM}) declined" in rep["why"], rep
    assert "numpy-test backend has no masked model kernel" in rep["why"], rep


def test_permutation_without_the_kernel_refits_with_a_why():
    x, y = _nan_data((16, 4, 3), 2, 2, seed=3)
    on, off = _pair(x, y, 2)
    got = permutation_test_q2y(on, n_permutations=3, n_splits=4, per_component=True)
    _declined(on.q2y_report_)
    assert on.q2y_report_["form"] == "one refit per fold and permutation on the regular engine"
    want = permutation_test_q2y(off, n_permutations=3, n_splits=4, per_component=True)
    np.testing.assert_allclose(got["null"], want["null"], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(got["p_value"], want["p_value"])


def test_repeated_without_the_kernel_refits_with_a_why():
    x, y = _nan_data((15, 5), 2, 2, seed=5)
    on, off = _pair(x, y, 2)
    got = get_q2y_repeated_kfold(on, n_splits=3, n_repeats=2, per_component=True)
    _declined(on.q2y_report_)
    assert on.q2y_report_["form"] == "one refit per fold and split on the regular engine"
    want = get_q2y_repeated_kfold(off, n_splits=3, n_repeats=2, per_component=True)
    np.testing.assert_allclose(got["q2y"], want["q2y"], rtol=1e-12, atol=1e-12)


def test_bootstrap_without_the_kernel_refits_with_a_why():
    x, y = _nan_data((14, 4, 3), 2, 2, seed=6)
    on, off = _pair(x, y, 2)
    got = bootstrap_factors(on, n_resamples=3)
    _declined(on.bootstrap_report_)
    assert on.bootstrap_report_["form"] == "one refit per resample on the regular engine"
    want = bootstrap_factors(off, n_resamples=3)
    np.testing.assert_allclose(got["coef"], want["coef"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["oob_q2y"], want["oob_q2y"], rtol=1e-12, atol=1e-12)


def _col_rel(got, want):
    """Worst relative error per column (last axis), normwise."""
    got, want = np.asarray(got), np.asarray(want)
    return float(max(np.linalg.norm(got[..., j] - want[..., j]) / np.linalg.norm(want[..., j]) for j in range(want.shape[-1])))


@pytest.mark.parametrize("shape,M,R,yperm", [((24, 5, 4), 3, 3, False), ((22, 7), 2, 2, True), ((20, 4, 6), 1, 2, False)])
def test_weighted_arithmetic_equals_the_oracle_on_duplicated_rows(shape, M, R, yperm):
    x, y = _nan_data(shape, M, R, seed=shape[0])
    I = shape[0]
    rng = np.random.default_rng(I + 1)
    c = rng.integers(0, 4, size=I)
    c[:3] = 0                                                                  # at least three rows held out
    c[3] = 2
    x[3].flat[0] = np.nan                                                      # a duplicated row holding a NaN
    yrow = rng.permutation(I) if yperm else None
    loadings, Q, coef, pred, n_iter = weighted_masked_fit(x, y, c, R, yrow)
    dup = np.repeat(np.arange(I), c)
    yp = y.reshape(I, -1)[np.arange(I) if yrow is None else yrow]
    fit = O.fit_tpls(x[dup], yp[dup], R)
    assert n_iter == fit.n_iter
    for L, Lw in zip(loadings, fit.loadings[0]):
        assert _col_rel(L, Lw) <= 1e-12
    assert _col_rel(Q, fit.Q) <= 1e-12
    assert np.abs(coef - fit.coef).max() <= 1e-12 * np.abs(fit.coef).max()
    held = x[c == 0]
    want = O.predict(fit, held)
    assert np.abs(pred[-1] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.fixture(scope="module")
def lib():
    from cmtf_pls_amd import _lib
    return _lib.load()


def _lds(I, A, B, M, R):
    n, k, P = min(A, B), max(A, B), A * B
    return 8 * (2 * I + P + A + B + 2 * M + 2 * n * n + n + k + M + R * R + R * (A + B) + R * M + R * R + 3 * R + 256 + 2 * I)


def _probe(lib, I, A, B, M, R, nm=3):
    """The entry's answer to a shape, with stand-in pointers and no workspace: 4 = declined, 2 = accepted (only the workspace
    is missing).  Neither touches a pointer."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    return lib.cmtfpls_cv_masked_models_f64(p, p, p, None, nm, I, A, B, M, R, 1e-8, 100, 0, 1, p, None, None, None, None, None, p,
                                            None, None, 0, None)


def test_c_entry_limits(lib):
    assert _probe(lib, 40, 64, 64, 2, 2) == 2                    # min(A, B) = 64
    assert _probe(lib, 40, 65, 65, 2, 2) == 4
    assert _probe(lib, 40, 6, 5, 64, 2) == 2                     # M = 64
    assert _probe(lib, 40, 6, 5, 65, 2) == 4
    assert _probe(lib, 40, 6, 5, 2, 16) == 2                     # R = 16
    assert _probe(lib, 40, 6, 5, 2, 17) == 4
    I = 2
    while _lds(I + 1, 1, 4000, 2, 1) <= 150 * 1024:
        I += 1
    assert _probe(lib, I, 1, 4000, 2, 1) == 2                    # the LDS at its cap
    assert _probe(lib, I + 1, 1, 4000, 2, 1) == 4
    assert _probe(lib, 40, 6, 5, 2, 2, nm=0) == 1                # no models: a bad argument
    assert lib.cmtfpls_cv_masked_model_workspace_bytes(40, 6, 5, 3, 2) == 8 * (40 * 30 + 40 * 3 + 40 * 2 + 2 * 30)
    assert lib.cmtfpls_cv_masked_model_workspace_bytes(1, 6, 5, 3, 2) == 0
