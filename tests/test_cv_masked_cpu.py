"""CPU-only: the opt-in switch of the masked cross-validation form (EngineOptions.masked_folds), its routing on a backend without
the kernel (the NumPy test backend: refits with a why that names the masked form), and the shape limits the C entry
cmtfpls_cv_masked_f64 declares -- checked before it touches a pointer or the GPU."""
import ctypes

import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import MASKED_FORM, fold_ids
from cmtf_pls_amd.validate import get_q2y, kfold_predictions
from numpy_backend import NumpyBackend


def test_masked_folds_is_off_by_default():
    assert EngineOptions().masked_folds is False
    assert EngineOptions(masked_folds=True).but(small_fit=False).masked_folds is True


def _nan_data(shape, M, R, seed):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=seed)
    x[np.random.default_rng(seed).random(x.shape) < 0.1] = np.nan
    return x, y


def test_kfold_without_the_kernel_refits_with_a_why():
    x, y = _nan_data((18, 4, 5), 2, 2, seed=4)
    m = tPLS(2, backend=NumpyBackend(), options=EngineOptions(small_fit=False, masked_folds=True))
    m.fit(x, y)
    pred = kfold_predictions(m, n_splits=3)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold")
    assert MASKED_FORM in rep["why"] and "numpy-test backend has no masked fold kernel" in rep["why"], rep
    ids, K = fold_ids(18, 3)
    want = np.zeros((2,) + y.shape)
    for k in range(K):
        test = ids == k
        for r in (1, 2):
            want[r - 1, test] = O.predict(O.fit_tpls(x[~test], y[~test], r), x[test])
    np.testing.assert_allclose(pred, want, rtol=1e-8, atol=1e-10)


def test_loo_without_the_kernel_refits_with_a_why():
    x, y = _nan_data((12, 4, 3), 2, 2, seed=8)
    m = tPLS(2, backend=NumpyBackend(), options=EngineOptions(small_fit=False, masked_folds=True))
    m.fit(x, y)
    q = get_q2y(m)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and MASKED_FORM in rep["why"], rep
    want = np.zeros(y.shape)
    for i in range(12):
        keep = np.arange(12) != i
        want[i] = O.predict(O.fit_tpls(x[keep], y[keep], 2), x[i:i + 1]).reshape(want[i].shape)
    assert abs(q - (1 - ((want - y) ** 2).sum() / (y ** 2).sum())) < 1e-8


@pytest.fixture(scope="module")
def lib():
    from cmtf_pls_amd import _lib
    return _lib.load()


def _lds(I, A, B, M, R):
    n, k, P = min(A, B), max(A, B), A * B
    return 8 * (2 * I + P + A + B + 2 * M + 2 * n * n + n + k + M + R * R + R * (A + B) + R * M + R * R + 3 * R + 256 + 2 * I)


def _probe(lib, I, A, B, M, R, K):
    """The entry's answer to a shape, with stand-in pointers and no workspace: 4 = declined, 2 = accepted (only the workspace
    is missing).  Neither touches a pointer."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    return lib.cmtfpls_cv_masked_f64(p, p, p, K, p, p, p, I, A, B, M, R, 1e-8, 100, 0, 1, p, p, p, None, None, 0, None)


def test_c_entry_limits(lib):
    assert _probe(lib, 40, 64, 64, 2, 2, 2) == 2                 # min(A, B) = 64
    assert _probe(lib, 40, 65, 65, 2, 2, 2) == 4
    assert _probe(lib, 40, 6, 5, 64, 2, 3) == 2                  # M = 64
    assert _probe(lib, 40, 6, 5, 65, 2, 3) == 4
    assert _probe(lib, 40, 6, 5, 2, 16, 3) == 2                  # R = 16
    assert _probe(lib, 40, 6, 5, 2, 17, 3) == 4
    assert _probe(lib, 40, 6, 5, 2, 2, 40) == 2                  # K = I (leave-one-out)
    assert _probe(lib, 40, 6, 5, 2, 2, 41) == 4
    I = 2
    while _lds(I + 1, 1, 4000, 2, 1) <= 150 * 1024:
        I += 1
    assert _probe(lib, I, 1, 4000, 2, 1, 2) == 2                 # the LDS at its cap
    assert _probe(lib, I + 1, 1, 4000, 2, 1, 2) == 4
    assert lib.cmtfpls_cv_masked_fold_workspace_bytes(40, 6, 5, 3, 2) == 8 * (40 * 30 + 40 * 3 + 40 * 2 + 2 * 30)
    assert lib.cmtfpls_cv_masked_fold_workspace_bytes(1, 6, 5, 3, 2) == 0
