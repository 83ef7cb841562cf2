"""Device cross-validation of order-4 X, the parts that need no GPU: the NumPy restatement of the fold loop
(tests/kfold_order4_ref.py) against oracle fits, the Kronecker identities that let every pass see X as I x A x B1 B2, and the wording
of kfold._decline_blocks for order-4 blocks."""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import kfold
from cmtf_pls_amd.options import EngineOptions
from kfold_order4_ref import inner_loop


def _rel(got, want):
    return np.linalg.norm(np.asarray(got) - np.asarray(want)) / np.linalg.norm(want)


@pytest.mark.parametrize("shape,M,seed", [((30, 5, 7, 3), 1, 1), ((36, 6, 5, 4), 3, 2), ((28, 6, 1, 5), 2, 3)])
def test_fold_loop_restatement_reproduces_oracle_fits(shape, M, seed):
    x, y, _ = O.import_synthetic(shape, M, 3, error=0.2, seed=seed)
    y = y.reshape(shape[0], -1)
    for test in (np.arange(shape[0]) % 4 == 0, np.arange(shape[0]) < 7):            # the training rows of two folds
        xt, yt = x[~test], y[~test]
        fit = O.fit_tpls(xt, yt, 1)
        Xc = (xt - xt.mean(axis=0)).reshape(xt.shape[0], -1)
        Yc = yt - yt.mean(axis=0)
        got = inner_loop(Yc.T @ Xc, Yc.T @ Yc, shape[1:])
        assert got["n_iter"] == fit.n_iter[0]
        for name, m in (("wA", 0), ("wK", 1), ("wL", 2)):
            assert _rel(got[name], fit.loadings[0][m][:, 0]) <= 1e-10, name
        assert _rel(got["q"], fit.Q[:, 0]) <= 1e-10
        assert np.array_equal(got["wB"], np.kron(got["wK"], got["wL"]))


def test_kronecker_identities_of_the_passes():
    rng = np.random.default_rng(5)
    I, A, B1, B2, M, R = 20, 4, 3, 5, 2, 3
    B = B1 * B2
    X = rng.standard_normal((I, A, B1, B2))
    Y = rng.standard_normal((I, M))
    wA, wK, wL = rng.standard_normal((R, A)), rng.standard_normal((R, B1)), rng.standard_normal((R, B2))
    wB = np.stack([np.kron(wK[j], wL[j]) for j in range(R)])
    full = np.stack([np.einsum("a,k,l->akl", wA[j], wK[j], wL[j]).ravel() for j in range(R)])
    c = np.arange(A * B)
    for j in range(R):                                                               # wk[c] = wA[c / B] wB[c % B] (fold_loop.hpp)
        np.testing.assert_allclose(wA[j][c // B] * wB[j][c % B], full[j], rtol=1e-15, atol=0)
    a = R - 1
    for j in range(a):                                                               # g_j = (wA_j.wA_a)(wB_j.wB_a) = w_j.w_a
        g = (wA[j] @ wA[a]) * (wB[j] @ wB[a])
        np.testing.assert_allclose(g, (wA[j] @ wA[a]) * (wK[j] @ wK[a]) * (wL[j] @ wL[a]), rtol=1e-13)
        np.testing.assert_allclose(g, full[j] @ full[a], rtol=1e-13)
    mu = X.mean(axis=0)                                                              # mu^T w = the mean contracted mode by mode
    np.testing.assert_allclose(mu.ravel() @ full[a], np.einsum("akl,a,k,l->", mu, wA[a], wK[a], wL[a]), rtol=1e-12)
    t = O.score_contract(X, [wA[a], wK[a], wL[a]])                                   # the score pass on I x P
    np.testing.assert_allclose(X.reshape(I, -1) @ full[a], t, rtol=1e-12)
    Xd = X - np.einsum("i,a,k,l->iakl", t, wA[a], wK[a], wL[a])                      # the down-date of S with w = wA (x) wK (x) wL
    S = Y.T @ X.reshape(I, -1)
    np.testing.assert_allclose(Y.T @ Xd.reshape(I, -1), S - np.outer(Y.T @ t, wA[a][c // B] * wB[a][c % B]), rtol=1e-12, atol=1e-12)


class _StubBackend:
    name = "stub"

    def __init__(self, tensor=True):
        for f in ("kfold_xcov", "kfold_inner", "kfold_epilogue", "mttkrp", "xcov", "kfold_inner_coupled", "kfold_combine_scores"):
            setattr(self, f, lambda *a, **k: None)
        if tensor:
            self.kfold_inner_tensor = lambda *a, **k: None


def _stub_model(tensor=True, tensor_folds=True, R=3):
    eng = SimpleNamespace(be=_StubBackend(tensor), opt=EngineOptions(tensor_folds=tensor_folds))
    return SimpleNamespace(_get_engine=lambda: eng, _comm=None, n_components=R)


_ENTRIES = ("kfold_xcov", "kfold_inner", "kfold_epilogue", "mttkrp", "xcov")
_COUPLED = ("kfold_xcov", "kfold_inner_coupled", "kfold_combine_scores", "kfold_epilogue", "mttkrp", "xcov")


def _decline(shape, M=3, K=4, **kw):
    ok = kw.pop("tensor_ok", True)
    X = np.zeros(shape, dtype=np.float32)
    return kfold._decline_blocks(_stub_model(**kw), [X], ["X"], np.zeros((shape[0], M)), K, _ENTRIES, tensor_ok=ok)


def test_decline_wording_for_order4_blocks():
    assert _decline((48, 6, 5, 4)) is None
    assert kfold._dims(np.zeros((48, 6, 5, 4))) == (6, 20) and kfold._tensor_dims([np.zeros((48, 6, 5, 4))]) == (5, 4)
    old = "X of order 4 (the device form takes order 2 and 3)"
    assert _decline((48, 6, 5, 4), tensor_folds=False) == old                        # the option is off: as it always was
    assert _decline((48, 6, 5, 4), tensor_ok=False) == old                           # a caller whose passes do not take it (bootstrap)
    assert _decline((8, 2, 2, 2, 2)) == "X of order 5 (the device form takes order 2 and 3)"
    assert _decline((48, 6, 5, 4), tensor=False) == "the stub backend has no order-4 K-fold kernel"
    assert _decline((8, 300, 17, 16)) == "mode-0 unfolding: min(300, 272) = 272 > 256"
    assert _decline((8, 17, 257, 16)) == "mode-1 unfolding: min(257, 272) = 257 > 256"
    assert _decline((8, 17, 16, 257)) == "mode-2 unfolding: min(257, 272) = 257 > 256"
    lds = 8 * (4 + 2 * 10000 + 3 * 3 + 3 * 3 + 200 + 200 + 50 + 200 + 1024)     # A, 2 B, 3 M, M^2, nmax, B1, B2, max dim, part
    assert _decline((8, 4, 200, 50)) == f"the fold's vectors need {lds} bytes of LDS > 153600 (cmtfpls_kfold_inner_tensor_f64)"
    assert _decline((48, 6, 5, 4), M=65) == "M = 65 responses > 64"
    x = np.zeros((48, 6, 5, 4))
    x[3, 1, 2, 0] = np.nan
    assert kfold._decline_blocks(_stub_model(), [x], ["X"], np.zeros((48, 3)), 4, _ENTRIES, tensor_ok=True) == "missing values in X"
    blocks = [np.zeros((48, 6, 5)), np.zeros((48, 6, 5, 4))]                         # a ctPLS block of order 4 keeps refitting
    assert kfold._decline_blocks(_stub_model(), blocks, ["block 0", "block 1"], np.zeros((48, 3)), 4, _COUPLED, tensor_ok=True) \
        == "block 1 of order 4 (the device form takes order 2 and 3)"


def _carve_up(A, B1, B2, M):
    """The LDS of cmtfpls_kfold_inner_tensor_f64 as include/cmtfpls.h lists it, vector by vector (doubles)."""
    B, P = B1 * B2, A * B1 * B2
    vectors = {"wA": A, "wB": B, "q": M, "qn": M, "tq": M, "Gy": M * M, "xs": max(min(d, P // d) for d in (A, B1, B2)),
               "wK": B1, "wL": B2, "v": B, "tmp": max(A, B1, B2), "part": 1024}
    return 8 * sum(vectors.values())


# a cube, the Gram seed from the B1 unfolding (16, not 3), M = 1, a mode of size 1, then one shape past each limit of the entry (a
# short side of 257, M = 65, more than 2^24 cells) and the two sides of the 150 KB cap: the byte count is not gated by them
LDS_SHAPES = [(5, 5, 5, 2), (3, 16, 16, 1), (6, 5, 4, 1), (6, 1, 5, 3), (257, 272, 1, 2), (17, 257, 16, 2), (6, 5, 4, 65), (257, 256, 256, 2),
              (4, 200, 50, 3), (1, 1, 4540, 2), (1, 1, 4541, 2)]


@pytest.mark.parametrize("shape", LDS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exported_lds_bytes_is_the_carve_up(shape):
    from cmtf_pls_amd import _lib
    assert _lib.load().cmtfpls_kfold_inner_tensor_lds_bytes(*shape) == _carve_up(*shape)


def test_exported_lds_bytes_over_the_cap_and_malformed():
    from cmtf_pls_amd import _lib
    lds_bytes = _lib.load().cmtfpls_kfold_inner_tensor_lds_bytes
    assert lds_bytes(3, 16, 16, 1) == 8 * (3 + 2 * 256 + 3 + 1 + 16 + 16 + 16 + 16 + 1024)                # xs: 16, not 3
    assert lds_bytes(1, 1, 4541, 2) - 32 == lds_bytes(1, 1, 4540, 2) == 150 * 1024 - 24                  # wB, v, tmp and wL grow
    for bad in range(4):
        for v in (0, -1):
            args = [6, 5, 4, 2]
            args[bad] = v
            assert lds_bytes(*args) == 0, args
