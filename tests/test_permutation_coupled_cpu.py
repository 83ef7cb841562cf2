"""CPU-only: EngineOptions.coupled_permutations (the device permutation test of a ctPLS, DESIGN 8d "coupled") exists and is off by
default; cmtfpls_kfold_inner_coupled_grouped_f64 is declared in the header, exported by the library and listed in _lib.SIGNATURES;
on a backend without the entry (the NumPy test backend) a ctPLS declines with a why and its null is exactly the option-off null;
and the C entry rejects nb, model_fold and groups before it looks at a pointer."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import _lib, ctPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.validate import permutation_test_q2y
from numpy_backend import NumpyBackend

ENTRY = "cmtfpls_kfold_inner_coupled_grouped_f64"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmtfpls.h")


def test_the_option_is_a_new_field_and_off_by_default():
    assert EngineOptions().coupled_permutations is False
    assert EngineOptions(masked_folds_coupled=True).coupled_permutations is False
    assert EngineOptions(coupled_permutations=True).masked_folds_coupled is False


def test_header_library_and_binding_table_have_the_entry():
    text = open(HEADER).read()
    assert re.search(r"\bint\s+" + ENTRY + r"\s*\(const cmtfpls_kfold_state\* blocks, int nb,\s*const int\* model_fold, int groups, int a, "
                     r"double tol,\s*int max_iter, void\* ws, size_t ws_bytes, void\* stream\);", text)
    assert ENTRY in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    assert restype is ctypes.c_int and len(argtypes) == 10
    assert getattr(_lib.load(), ENTRY) is not None


def test_without_the_kernels_a_coupled_model_refits_with_a_why():
    x, y, _ = O.import_synthetic((16, 4, 3), 2, 3, error=0.3, seed=4)
    z = y.reshape(16, -1) @ np.random.default_rng(8).standard_normal((2, 5)) + 0.5 * np.random.default_rng(9).standard_normal((16, 5))
    on = ctPLS(2, backend=NumpyBackend(), options=EngineOptions(small_fit=False, coupled_permutations=True))
    off = ctPLS(2, backend=NumpyBackend(), options=EngineOptions(small_fit=False))
    on.fit([x, z], y)
    off.fit([x, z], y)
    got = permutation_test_q2y(on, n_permutations=3, n_splits=4, per_component=True)
    rep = on.q2y_report_
    assert rep["why"] == "the numpy-test backend has no coupled K-fold kernels", rep
    assert rep["form"] == "one refit per fold and permutation on the regular engine" and rep["passes"] == 0 and rep["x_reads"] is None
    want = permutation_test_q2y(off, n_permutations=3, n_splits=4, per_component=True)
    assert off.q2y_report_["why"] == "coupled model: permutation device form not built"
    np.testing.assert_array_equal(got["null"], want["null"])
    np.testing.assert_array_equal(got["p_value"], want["p_value"])
    assert rep["n_iter"] == off.q2y_report_["n_iter"]


def test_c_entry_rejects_nb_model_fold_and_groups_before_any_pointer():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                                   # a stand-in for every pointer: never dereferenced
    views = (_lib.KfoldState * 9)()                              # zeroed views: any look at them would fail the view checks first
    fn = getattr(lib, ENTRY)
    for nb, mf, groups in [(0, p, 1), (9, p, 1), (-1, p, 1), (2, None, 1), (2, p, 0), (2, p, -3)]:
        assert fn(views, nb, mf, groups, 0, 1e-8, 100, p, 64, None) == 1, (nb, mf, groups)      # CMTFPLS_EINVAL
        assert b"kfold_inner_coupled_grouped" in lib.cmtfpls_last_error()
    assert fn(None, 2, p, 1, 0, 1e-8, 100, p, 64, None) == 1
