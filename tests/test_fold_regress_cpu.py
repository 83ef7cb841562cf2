"""csrc/fold_regress.hpp's fold_normal_solve -- the serial solve of every one-workgroup-per-fold kernel and of kfold_solve_kernel,
with the pivot rule -- compiled for the HOST and called through ctypes: bit for bit against its restatement in plain Python
floats (tests/small_algebra_ref.py; the host build forbids fused multiply-adds, so every operation rounds as Python's), and
against lstsq on the inputs and at the tolerances of test_gpu_round2.py's two normal_solve cases.  Then the chunk arithmetic of
the workgroup-per-fold wrappers (backend.chunk_size).  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import small_algebra_ref as SA
from cmtf_pls_amd.backend import chunk_size

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cmtf_pls_amd", "csrc")
WRAPPER = """#include "fold_regress.hpp"
extern "C" void fold_normal_solve_host(double* Gn, const double* gn, int kk, double* dd, double* bb) {
  cmtfpls::fold_normal_solve(Gn, gn, kk, dd, bb);
}
"""


@pytest.fixture(scope="module")
def solve(tmp_path_factory):
    d = tmp_path_factory.mktemp("fold_regress")
    src, lib = d / "wrapper.hip", d / "libfoldregress.so"
    src.write_text(WRAPPER)
    p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-x", "hip", "-O2", "-std=c++17",
                        "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, str(src), "-o", str(lib)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    fn = ctypes.CDLL(str(lib)).fold_normal_solve_host
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]

    def run(G, g):
        k = len(g)
        Gn, gn = np.array(G, dtype=np.float64).reshape(k * k), np.array(g, dtype=np.float64)      # copies: Gn is overwritten
        dd, bb = np.empty(k), np.empty(k)
        fn(Gn.ctypes.data, gn.ctypes.data, k, dd.ctypes.data, bb.ctypes.data)
        return bb
    return run


@pytest.mark.parametrize("k", [1, 2, 7, 16, 33, 64])
def test_host_build_equals_the_restatement(solve, k):
    rng = np.random.default_rng(k)
    T = rng.normal(size=(200, k)) * 10.0 ** rng.uniform(-8, 0, size=k)[None, :]
    if k >= 7:
        T[:, 2] = 0.0                                  # an all-zero score column
        T[:, 4] = 2.0 * T[:, 1]                        # an exactly dependent one
    G, g = T.T @ T, T.T @ rng.normal(size=200)
    want, dropped = SA.fold_normal_solve(G, g)
    got = solve(G, g)
    assert np.array_equal(got, want)
    if k >= 7:
        assert dropped == [2, 4]
        assert got[2] == 0.0 and got[4] == 0.0
    else:
        assert dropped == []


def test_non_finite_diagonal_drops_the_column(solve):
    G, g = [[1.0, np.nan], [np.nan, np.inf]], [1.0, 1.0]
    want, dropped = SA.fold_normal_solve(G, g)
    got = solve(G, g)
    assert dropped == [1]                              # dd[1] = 0: the equilibrated pivot is inf * 0 = NaN, not above tiny
    assert np.isnan(want[0]) and want[1] == 0.0
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("k", [1, 3, 10, 33, 64])
def test_matches_lstsq_on_badly_scaled_scores(solve, k):
    """test_gpu_round2.py::test_normal_solve_matches_lstsq_on_badly_scaled_scores on the serial solve."""
    rng = np.random.default_rng(k)
    T = rng.normal(size=(500, k)) * np.logspace(0, -12, k)[None, :]
    T[:, 1:] += 0.3 * T[:, :1] * np.logspace(0, -12, k)[None, 1:]          # not orthogonal
    u = rng.normal(size=500)
    want = np.linalg.lstsq(T, u, rcond=-1)[0]
    np.testing.assert_allclose(solve(T.T @ T, T.T @ u), want, rtol=1e-6, atol=0)


def test_drops_zero_and_dependent_columns(solve):
    """test_gpu_round2.py::test_normal_solve_drops_zero_and_dependent_columns on the serial solve."""
    rng = np.random.default_rng(3)
    T = rng.normal(size=(200, 5))
    T[:, 2] = 0.0
    T[:, 4] = 2.0 * T[:, 1]
    u = rng.normal(size=200)
    got = solve(T.T @ T, T.T @ u)
    assert got[2] == 0.0 and got[4] == 0.0 and np.all(np.isfinite(got))
    keep = [0, 1, 3]
    np.testing.assert_allclose(got[keep], np.linalg.lstsq(T[:, keep], u, rcond=None)[0], rtol=1e-10)


# ---- backend.chunk_size: items per launch of the chunked workgroup-per-fold calls ---------------------------------------------
def test_chunk_size_edges():
    assert chunk_size(100, 1000, 999) == 1               # a budget below one item still launches one at a time
    assert chunk_size(100, 1000, 10 ** 9) == 100         # a budget above all items: one launch
    assert chunk_size(100, 1000, 37 * 1000 + 999) == 37
    assert chunk_size(5000, 8, 1 << 40, cap=512) == 512  # the xcov forms' cap
    assert chunk_size(100, 8, 1 << 40, cap=512) == 100
    assert chunk_size(7, 0, 4 << 30) == 7                # no workspace per item: no division by zero
    assert chunk_size(7, 0, 0) == 1


@pytest.mark.parametrize("n,per,budget,cap", [(1, 10, 5, None), (97, 10, 95, None), (97, 10, 1 << 30, None), (1300, 1, 1 << 30, 512),
                                              (513, 0, 0, 512), (64, 3, 64, 5)])
def test_chunks_cover_every_item_once(n, per, budget, cap):
    chunk = chunk_size(n, per, budget, cap)
    lengths = [min(chunk, n - i0) for i0 in range(0, n, chunk)]      # the launches of HipBackend._chunked_launch
    assert sum(lengths) == n and min(lengths) >= 1
    assert chunk == 1 or chunk * per <= budget
    assert cap is None or max(lengths) <= cap
