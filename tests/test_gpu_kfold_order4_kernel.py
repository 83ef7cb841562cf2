"""cmtfpls_kfold_inner_tensor_f64 (the fold loop with the rank-1 CP of an A x B1 x B2 cross-covariance inside each fold's
workgroup, csrc/fold_loop.hpp: lx_cp3) against the NumPy float64 restatement tests/kfold_order4_ref.py, whose extraction is
oracle.nipals_oracle.rank1_factors.  The state is built by hand: K = 3 models, each S with a planted dominant rank-one term plus
5 % noise, G_y an identity-like SPD matrix in the first row tile's partial.

Tolerance: 1e-10 normwise on the loadings and q, the project's level for f64 kernels against the oracle (test_gpu_xcov_iterate.py);
the iteration counts must be equal."""
import ctypes

import numpy as np
import pytest
import torch

from cmtf_pls_amd import kfold
from cmtf_pls_amd.backend import HipBackend
from kfold_order4_ref import inner_loop, planted

pytestmark = pytest.mark.gpu

_TOL = 1e-10
_K, _R, _I = 3, 2, 8
# (A, B1, B2, M): tiny; nothing a multiple of 16; the mode-0 unfolding's short side the trailing one (lx_rank1's transpose path);
# full 16 x 16 tiles; a degenerate middle mode
SHAPES = [(5, 7, 3, 1), (17, 4, 33, 3), (40, 3, 2, 2), (3, 16, 16, 4), (6, 1, 5, 2)]


@pytest.fixture(scope="module")
def be():
    return HipBackend("cuda:0")


def _rel(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _hand_state(be, S, Gy, A, B):
    """A state of K models on S (K x M x P) whose summed row-tile partials of G_y are Gy (every model)."""
    K, M, _ = S.shape
    t = lambda a, dt=torch.float64: kfold._to_dev(a, be.device, dt)
    st, shared, own = kfold._state(be, t(np.arange(_I) % K, torch.int32), be.zeros(K, _I, M), [(A, B, t(S), be.zeros(K, A * B))], _R, 1)
    shared["Gy"].zero_()
    shared["Gy"][:, 0] = t(Gy)
    return st, shared, own


def _run(be, st, dims, model_fold=None, groups=1, a=0, B12=None):
    A, B1, B2 = dims
    b1, b2 = B12 if B12 is not None else (B1, B2)
    Wk, Wl = be.zeros(_K, _R, B1), be.zeros(_K, _R, B2)
    ws = torch.empty(max(be.kfold_inner_tensor_workspace_bytes(A, B1, B2, _K), 256), dtype=torch.uint8, device=be.device)
    ok = be.kfold_inner_tensor(st[0], b1, b2, a, 1e-8, 100, ws, model_fold, groups, Wk, Wl)
    torch.cuda.synchronize()
    return ok, Wk.cpu().numpy(), Wl.cpu().numpy()


def _check(shared, own, Wk, Wl, S, Gy, dims, a=0):
    A, B1, B2 = dims
    Wa, Wb, Q = own[0]["Wa"].cpu().numpy(), own[0]["Wb"].cpu().numpy(), shared["Q"].cpu().numpy()
    WA, WB = own[0]["WA"].cpu().numpy(), own[0]["WB"].cpu().numpy()
    n_iter = shared["n_iter"].cpu().numpy()
    assert not shared["status"].cpu().numpy().any()
    for k in range(S.shape[0]):
        want = inner_loop(S[k], Gy, dims, 1e-8, 100)
        errs = {"wA": _rel(Wa[k, a], want["wA"]), "wK": _rel(Wk[k, a], want["wK"]), "wL": _rel(Wl[k, a], want["wL"]),
                "wB": _rel(Wb[k, a], want["wB"]), "q": _rel(Q[k, a], want["q"])}
        print(f"dims {dims} model {k}: n_iter {int(n_iter[k, a])} (want {want['n_iter']}), errors {errs}")
        assert int(n_iter[k, a]) == want["n_iter"], (k, n_iter[k, a], want["n_iter"])
        assert max(errs.values()) <= _TOL, (k, errs)
        assert np.array_equal(WA[:, k], Wa[k, a]) and np.array_equal(WB[:, k], Wb[k, a])      # the MTTKRP operands
        assert np.array_equal(Wb[k, a], np.outer(Wk[k, a], Wl[k, a]).ravel())                # wB = wK (x) wL, C order


@pytest.mark.parametrize("A,B1,B2,M", SHAPES)
def test_inner_tensor_matches_float64_restatement(be, A, B1, B2, M):
    dims = (A, B1, B2)
    S, Gy = planted(dims, M, _K, seed=A + B1 + B2)
    st, shared, own = _hand_state(be, S, Gy, A, B1 * B2)
    ok, Wk, Wl = _run(be, st, dims)
    assert ok is True
    _check(shared, own, Wk, Wl, S, Gy, dims)
    vec = shared["vec"].cpu().numpy()                                                # mu = 0 in this state: mu^T w = 0
    assert np.all(vec[:, 3 * _R + M + 1] == 0.0)


def test_second_component_writes_g_and_its_own_slot(be):
    """a = 1 after a = 0 on the same S: slot 1 of Wk / Wl / Wa / Wb is written, slot 0 stays, and g_0 = (wA_0.wA_1)(wB_0.wB_1)."""
    dims, M = (5, 7, 3), 2
    S, Gy = planted(dims, M, _K, seed=3)
    st, shared, own = _hand_state(be, S, Gy, dims[0], dims[1] * dims[2])
    A, B1, B2 = dims
    Wk, Wl = be.zeros(_K, _R, B1), be.zeros(_K, _R, B2)
    ws = torch.empty(be.kfold_inner_tensor_workspace_bytes(A, B1, B2, _K), dtype=torch.uint8, device=be.device)
    for a in range(2):
        assert be.kfold_inner_tensor(st[0], B1, B2, a, 1e-8, 100, ws, None, 1, Wk, Wl) is True
    torch.cuda.synchronize()
    Wkh, Wlh = Wk.cpu().numpy(), Wl.cpu().numpy()
    assert np.array_equal(Wkh[:, 0], Wkh[:, 1]) and np.array_equal(Wlh[:, 0], Wlh[:, 1])   # (the same S: the same loadings)
    _check(shared, own, Wkh, Wlh, S, Gy, dims, a=1)
    g = shared["vec"].cpu().numpy()[:, 2 * _R + M + 1]
    Wa, Wb = own[0]["Wa"].cpu().numpy(), own[0]["Wb"].cpu().numpy()
    want = np.array([(Wa[k, 0] @ Wa[k, 1]) * (Wb[k, 0] @ Wb[k, 1]) for k in range(_K)])
    np.testing.assert_allclose(g, want, rtol=1e-13)


def test_grouped_layout_reads_the_held_out_folds_mean(be):
    """model_fold with groups = 2 over K = 4 models (2 folds x 2 groups): the loop is the plain one and mu^T w uses row
    model_fold[m] of the per-fold mean."""
    dims, M, K = (5, 7, 3), 2, 4
    A, B1, B2 = dims
    P = A * B1 * B2
    S, Gy = planted(dims, M, K, seed=11)
    mean = np.random.default_rng(2).standard_normal((2, P))
    t = lambda a, dt=torch.float64: kfold._to_dev(a, be.device, dt)
    st, shared, own = kfold._state(be, t(np.arange(_I) % 2, torch.int32), be.zeros(K, _I, M), [(A, B1 * B2, t(S), t(mean))], _R, 2)
    shared["Gy"].zero_()
    shared["Gy"][:, 0] = t(Gy)
    mf = t(np.array([0, 0, 1, 1]), torch.int32)
    Wk, Wl = be.zeros(K, _R, B1), be.zeros(K, _R, B2)
    ws = torch.empty(be.kfold_inner_tensor_workspace_bytes(A, B1, B2, K), dtype=torch.uint8, device=be.device)
    assert be.kfold_inner_tensor(st[0], B1, B2, 0, 1e-8, 100, ws, mf, 2, Wk, Wl) is True
    torch.cuda.synchronize()
    _check(shared, own, Wk.cpu().numpy(), Wl.cpu().numpy(), S, Gy, dims)
    mw = shared["vec"].cpu().numpy()[:, 3 * _R + M + 1]
    Wa, Wb = own[0]["Wa"].cpu().numpy(), own[0]["Wb"].cpu().numpy()
    want = np.array([mean[[0, 0, 1, 1][m]] @ np.kron(Wa[m, 0], Wb[m, 0]) for m in range(K)])
    np.testing.assert_allclose(mw, want, rtol=1e-12, atol=1e-14)


def test_limits_are_checked_before_the_launch(be):
    dims, M = (5, 7, 3), 1
    S, Gy = planted(dims, M, _K, seed=1)
    st, shared, own = _hand_state(be, S, Gy, 5, 21)
    lib, ws = be.lib, torch.empty(1 << 20, dtype=torch.uint8, device=be.device)

    def call(state, B1, B2):
        return lib.cmtfpls_kfold_inner_tensor_f64(ctypes.byref(state), None, 1, B1, B2, 0, 1e-8, 100, None, None, ws.data_ptr(),
                                                  ws.numel(), None)
    assert call(st[0], 7, 4) == 1                                                    # CMTFPLS_EINVAL: st->B != B1 * B2
    assert be.kfold_inner_tensor_workspace_bytes(5, 7, 3, _K) == _K * 8 * (6 * 105 + 2 * 7 * 7)
    # an unfolding with short side 257: A x B1 x B2 = 1 x 257 x 257 (mode 1: min(257, 257)); declined on the host, nothing launched
    big, big_shared, big_own = kfold._state(be, shared["fold_of"], be.zeros(_K, _I, M),
                                            [(1, 257 * 257, be.zeros(_K, M, 257 * 257), be.zeros(_K, 257 * 257))], _R, 1)
    assert call(big[0], 257, 257) == 4                                               # CMTFPLS_EUNSUPPORTED
    assert b"shorter side" in lib.cmtfpls_last_error()
    torch.cuda.synchronize()
    assert not big_shared["n_iter"].any() and not big_shared["status"].any() and not big_own[0]["Wa"].any()
