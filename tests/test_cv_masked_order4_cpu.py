"""CPU-only: the opt-in switch of the masked order-4 cross-validation form (EngineOptions.masked_tensor_folds), its
routing on a backend without the kernel (the NumPy test backend: refits with a why that names the new entry), and the shape limits
the C entries cmtfpls_cv_masked_tensor_f64 / cmtfpls_cv_masked_tensor_models_f64 declare -- checked before they touch a pointer or
the GPU."""
import ctypes

import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import MASKED_TENSOR_FORM, fold_ids
from cmtf_pls_amd.validate import get_q2y, kfold_predictions, loo_predictions
from numpy_backend import NumpyBackend

LDS_CAP = 150 * 1024


def test_masked_tensor_folds_is_off_by_default():
    assert EngineOptions().masked_tensor_folds is False
    on = EngineOptions(masked_tensor_folds=True).but(small_fit=False)
    assert on.masked_tensor_folds is True and on.masked_folds is False and on.tensor_folds is False    # a field of its own


def _nan_data(shape, M, R, nan, seed):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=seed)
    x[np.random.default_rng(seed + 100).random(x.shape) < nan] = np.nan
    return x, y


def _all_columns_observed(x, ids, K):
    return all((~np.isnan(x[ids != k])).reshape((ids != k).sum(), -1).any(axis=0).all() for k in range(K))


def test_kfold_without_the_kernel_refits_with_a_why():
    x, y = _nan_data((24, 4, 3, 2), 2, 2, 0.05, seed=24)
    m = tPLS(2, backend=NumpyBackend(), options=EngineOptions(small_fit=False, masked_tensor_folds=True))
    m.fit(x, y)
    pred = kfold_predictions(m, n_splits=4)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold")
    assert MASKED_TENSOR_FORM in rep["why"] and "numpy-test backend has no masked order-4 fold kernel" in rep["why"], rep
    ids, K = fold_ids(24, 4)
    assert _all_columns_observed(x, ids, K)                     # where the oracle (masks before centring) is the reference's fit
    want = np.zeros((2,) + y.shape)
    for k in range(K):
        test = ids == k
        for r in (1, 2):
            want[r - 1, test] = O.predict(O.fit_tpls(x[~test], y[~test], r), x[test])
    np.testing.assert_allclose(pred, want, rtol=1e-8, atol=1e-10)


def test_loo_without_the_kernel_refits_with_a_why():
    x, y = _nan_data((30, 5, 4, 3), 3, 2, 0.1, seed=5)
    m = tPLS(2, backend=NumpyBackend(), options=EngineOptions(small_fit=False, masked_tensor_folds=True))
    m.fit(x, y)
    q = get_q2y(m)
    rep = m.q2y_report_
    assert rep["form"].startswith("one refit per fold") and MASKED_TENSOR_FORM in rep["why"], rep
    assert "numpy-test backend has no masked order-4 fold kernel" in rep["why"], rep
    assert loo_predictions(m) is None                          # no device form on this backend: the refits are the caller's
    pred = kfold_predictions(m, n_splits=30)[-1]               # ... and K = I is those refits, row by row
    assert m.q2y_report_["form"].startswith("one refit per fold") and MASKED_TENSOR_FORM in m.q2y_report_["why"]
    assert _all_columns_observed(x, np.arange(30), 30)
    want = np.zeros(y.shape)
    for i in range(30):
        keep = np.arange(30) != i
        want[i] = O.predict(O.fit_tpls(x[keep], y[keep], 2), x[i:i + 1]).reshape(want[i].shape)
    np.testing.assert_allclose(pred, want, rtol=1e-8, atol=1e-10)
    assert abs(q - (1 - ((want - y) ** 2).sum() / (y ** 2).sum())) < 1e-8


@pytest.fixture(scope="module")
def lib():
    from cmtf_pls_amd import _lib
    return _lib.load()


def _probe(lib, I, A, B1, B2, M, R, K):
    """The fold entry's answer to a shape, with stand-in pointers and no workspace: 4 = declined, 2 = accepted (only the workspace
    is missing).  Neither touches a pointer."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    return lib.cmtfpls_cv_masked_tensor_f64(p, p, p, K, p, p, p, I, A, B1, B2, M, R, 1e-8, 100, 0, 1, p, p, p, None, None, 0, None)


def _probe_models(lib, I, A, B1, B2, M, R):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    return lib.cmtfpls_cv_masked_tensor_models_f64(p, p, p, None, 3, I, A, B1, B2, M, R, 1e-8, 100, 0, 1, p, None, None, None, None, None,
                                                   None, p, None, None, 0, None)


def _short_side(A, B1, B2):
    """The largest short side of the three unfoldings of an A x B1 x B2 contraction."""
    return max(min(d, A * B1 * B2 // d) for d in (A, B1, B2))


def _carve_up(I, A, B1, B2, M, R):
    """The LDS of a workgroup of the two entries as include/cmtfpls.h states it (doubles)."""
    B, n = B1 * B2, _short_side(A, B1, B2)
    return 8 * (4 * I + A * B + A + 2 * B + 3 * M + 2 * n * n + n + 2 * R * R + R * (A + B) + R * M + 3 * R + 512 + B1 + B2
                + max(A, B1, B2) + 12)


# a cube, the Gram buffers from the B1 unfolding (16, not 3), M = 1, a mode of size 1, every limit reached, then one shape past each
# (a short side of 65, M = 65, R = 17): the byte count is not gated by them
LDS_SHAPES = [(12, 5, 5, 5, 2, 2), (12, 3, 16, 16, 1, 1), (40, 6, 5, 4, 1, 3), (9, 6, 1, 5, 2, 3), (12, 64, 8, 8, 64, 16), (8, 65, 13, 5, 2, 1),
              (8, 33, 65, 2, 2, 1), (40, 6, 5, 4, 65, 2), (40, 6, 5, 4, 2, 17), (2, 1, 1, 7, 1, 1)]


@pytest.mark.parametrize("shape", LDS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exported_lds_bytes_is_the_carve_up(lib, shape):
    assert lib.cmtfpls_cv_masked_tensor_lds_bytes(*shape) == _carve_up(*shape)


def test_exported_lds_bytes_over_the_cap_and_malformed(lib):
    lds_bytes = lib.cmtfpls_cv_masked_tensor_lds_bytes
    assert lds_bytes(12, 3, 16, 16, 1, 1) == 8 * (48 + 768 + 3 + 512 + 3 + 512 + 16 + 2 + 259 + 1 + 3 + 512 + 16 + 16 + 16 + 12)   # n: 16, not 3
    I = (LDS_CAP - _carve_up(0, 64, 8, 8, 2, 1)) // 32                     # the last I within the cap: a row costs 4 doubles
    assert _carve_up(I, 64, 8, 8, 2, 1) <= LDS_CAP < _carve_up(I + 1, 64, 8, 8, 2, 1)
    assert lds_bytes(I + 1, 64, 8, 8, 2, 1) == _carve_up(I + 1, 64, 8, 8, 2, 1) and _probe(lib, I + 1, 64, 8, 8, 2, 1, 2) == 4
    assert lds_bytes(I, 64, 8, 8, 2, 1) == _carve_up(I, 64, 8, 8, 2, 1) and _probe(lib, I, 64, 8, 8, 2, 1, 2) == 2
    for bad in range(6):
        for v in (0, -1):
            args = [12, 6, 5, 4, 2, 3]
            args[bad] = v
            assert lds_bytes(*args) == 0, args
    assert lds_bytes(1, 6, 5, 4, 2, 3) == 0                                # I = 1: no training row left


def test_c_entry_limits(lib):
    for probe in (lambda I, A, B1, B2, M, R: _probe(lib, I, A, B1, B2, M, R, 2), lambda *s: _probe_models(lib, *s)):
        assert _short_side(64, 8, 8) == 64 and _short_side(65, 13, 5) == 65
        assert probe(12, 64, 8, 8, 2, 2) == 2                    # the largest short side = 64: mode 0
        assert probe(12, 32, 64, 2, 2, 1) == 2                   # ... mode 1
        assert probe(12, 32, 2, 64, 2, 1) == 2                   # ... mode 2
        assert probe(8, 65, 13, 5, 2, 1) == 4                    # 65
        assert probe(8, 33, 65, 2, 2, 1) == 4
        assert probe(8, 33, 2, 65, 2, 1) == 4
        assert probe(40, 6, 5, 4, 64, 2) == 2                    # M = 64
        assert probe(40, 6, 5, 4, 65, 2) == 4
        assert probe(40, 6, 5, 4, 2, 16) == 2                    # R = 16
        assert probe(40, 6, 5, 4, 2, 17) == 4
        I = 2
        while lib.cmtfpls_cv_masked_tensor_lds_bytes(I + 1, 64, 8, 8, 2, 1) <= LDS_CAP:
            I += 1
        assert probe(I, 64, 8, 8, 2, 1) == 2                     # the LDS at its cap (the library's own count)
        assert probe(I + 1, 64, 8, 8, 2, 1) == 4
        assert probe(40, 1, 1, 1 << 30, 2, 1) == 4               # short sides of 1, and nothing that fits
    assert _probe(lib, 40, 6, 5, 4, 2, 2, 40) == 2               # K = I (leave-one-out)
    assert _probe(lib, 40, 6, 5, 4, 2, 2, 41) == 4
    for fn in (lib.cmtfpls_cv_masked_tensor_fold_workspace_bytes, lib.cmtfpls_cv_masked_tensor_model_workspace_bytes):
        assert fn(40, 6, 5, 4, 3, 2) == 8 * (40 * 120 + 40 * 3 + 40 * 2 + 6 * 120)      # Xf | Yf | T | cs | mu | Zt | U | yl | vr
        assert fn(1, 6, 5, 4, 3, 2) == 0 and fn(0, 6, 5, 4, 3, 2) == 0
