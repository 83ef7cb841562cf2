"""Leave-one-out and the factor bootstrap of order-4 X on the device, the parts that need no GPU: the wording of the
host-side limit check of cmtfpls_loo_xcov_tensor_f64, its LDS formula against the carve-up include/cmtfpls.h documents, the oracle
leave-one-out helper, and the Kronecker identities that let the bootstrap align four modes from wA, wK and wL."""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import _lib
from cmtf_pls_amd import validate as V
from cmtf_pls_amd.bootstrap import align_factors
from loo_order4_ref import loo_case, planted_xy

ENTRY = "cmtfpls_loo_xcov_tensor_f64"


@pytest.fixture(scope="module")
def lds_bytes():
    return _lib.load().cmtfpls_loo_xcov_tensor_lds_bytes


def _be(tensor=True):
    be = SimpleNamespace(name="stub")
    if tensor:
        be.loo_tpls_tensor = lambda *a, **k: None
    return be


def test_decline_wording():
    d = V._decline_loo_tensor
    assert d(_be(), 6, 5, 4, 2, 3) is None
    assert d(_be(), 256, 256, 256, 128, 64) is not None and d(_be(), 256, 16, 16, 2, 3) is None
    assert d(_be(False), 6, 5, 4, 2, 3) == "the stub backend has no order-4 leave-one-out kernel"
    assert d(_be(), 257, 272, 1, 2, 2) == "mode-0 unfolding: min(257, 272) = 257 > 256"
    assert d(_be(), 17, 257, 16, 2, 2) == "mode-1 unfolding: min(257, 272) = 257 > 256"
    assert d(_be(), 17, 16, 257, 2, 2) == "mode-2 unfolding: min(257, 272) = 257 > 256"
    assert d(_be(), 6, 5, 4, 129, 2) == f"M = 129 > 128 responses ({ENTRY})"
    assert d(_be(), 6, 5, 4, 2, 65) == f"R = 65 > 64 components ({ENTRY})"
    lds = _carve_up(4, 200, 50, 2, 2)
    assert lds > 150 * 1024 and d(_be(), 4, 200, 50, 2, 2) == f"the fold's vectors need {lds} bytes of LDS > 153600 ({ENTRY})"
    assert d(_be(), 6, 1, 5, 2, 3) is None and d(_be(), 6, 5, 1, 2, 3) is None       # a mode of size 1 is a tensor, not a decline


def _carve_up(A, B1, B2, M, R):
    """The LDS of the kernel as include/cmtfpls.h lists it, vector by vector (doubles)."""
    B, P = B1 * B2, A * B1 * B2
    n = max(min(d, P // d) for d in (A, B1, B2))
    vectors = {"wA": A, "wB": B, "q": M, "qn": M, "tq": M, "my": M, "Gy": M * M, "xs": n,
               "wK": B1, "wL": B2, "v": B, "tmp": max(A, B1, B2), "part": 1024,
               "coef": R * R, "Qs": R * M, "Gn": R * R, "gn": R, "bb": R, "dd": R}
    return 8 * sum(vectors.values())


def test_lds_formula_is_the_documented_carve_up(lds_bytes):
    assert lds_bytes(6, 5, 4, 2, 3) == _carve_up(6, 5, 4, 2, 3) == 8 * (6 + 20 + 8 + 4 + 6 + 5 + 4 + 20 + 6 + 1024 + 9 + 6 + 9 + 9)
    assert lds_bytes(40, 3, 2, 128, 64) == _carve_up(40, 3, 2, 128, 64)
    # the Gram seed is sized by the largest short side of the three unfoldings, not by min(A, B1 B2)
    assert lds_bytes(3, 16, 16, 1, 1) == 8 * (3 + 2 * 256 + 4 + 1 + 16 + 16 + 16 + 16 + 1024 + 2 + 1 + 3)   # xs: 16, not 3


# a cube, the Gram seed from the B1 unfolding, M = 1, the cap's two sides, then one shape past each limit of the entry (a short side
# of 257, M = 129, R = 65, more than 2^24 cells, just over 150 KB): the byte count is not gated by them
LDS_SHAPES = [(5, 5, 5, 2, 2), (3, 16, 16, 1, 1), (6, 5, 4, 1, 3), (6, 1, 5, 2, 3), (141, 16, 16, 128, 10), (257, 272, 1, 2, 2),
              (17, 257, 16, 2, 2), (6, 5, 4, 129, 2), (6, 5, 4, 2, 65), (257, 256, 256, 2, 2), (1, 1, 4535, 2, 2), (1, 1, 4536, 2, 2)]


@pytest.mark.parametrize("shape", LDS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_exported_lds_bytes_is_the_carve_up(lds_bytes, shape):
    assert lds_bytes(*shape) == _carve_up(*shape)


def test_exported_lds_bytes_over_the_cap_and_malformed(lds_bytes):
    assert lds_bytes(1, 1, 4536, 2, 2) - 32 == lds_bytes(1, 1, 4535, 2, 2) == 150 * 1024 - 24          # wB, v, tmp and wL grow
    for bad in range(5):
        for v in (0, -1):
            args = [6, 5, 4, 2, 3]
            args[bad] = v
            assert lds_bytes(*args) == 0, args


def test_oracle_leave_one_out_helper():
    X, Y, pred, n_iter = loo_case((8, 6, 1, 5), 3, 3, 3)
    assert pred.shape == Y.shape and n_iter.shape == (8, 3) and 2 <= n_iter.min() and n_iter.max() < 100
    keep = np.arange(8) != 2
    fit = O.fit_tpls(X[keep], Y[keep], 3)
    np.testing.assert_array_equal(np.asarray(O.predict(fit, X[2:3])).reshape(-1), pred[2])
    assert np.abs(pred - Y).max() < np.abs(Y).max()                                   # the planted signal is predictable
    X2, _ = planted_xy((8, 6, 1, 5), 3, seed=3)
    assert np.array_equal(X, X2) and not X.flags.writeable


def test_kronecker_identities_of_the_four_mode_alignment():
    rng = np.random.default_rng(4)
    I, A, B1, B2, R, M = 12, 6, 5, 4, 3, 2
    X = rng.standard_normal((I, A, B1, B2))
    wA, wK, wL = rng.standard_normal((A, R)), rng.standard_normal((B1, R)), rng.standard_normal((B2, R))
    for r in range(R):
        wB = np.kron(wK[:, r], wL[:, r])                                              # what the passes hold (Wb)
        np.testing.assert_array_equal(wB.reshape(B1, B2), np.outer(wK[:, r], wL[:, r]))
        t3 = X.reshape(I, A, B1 * B2).reshape(I, -1) @ np.kron(wA[:, r], wB)         # the score of the I x A x B view
        t4 = np.einsum("iakl,a,k,l->i", X, wA[:, r], wK[:, r], wL[:, r])              # the mode products of the order-4 model
        np.testing.assert_allclose(t3, t4, rtol=1e-12, atol=1e-12)
        # flips of the modes: the Kronecker loading and the score change by the product of the flips
        for sa, sk, sl in ((1, -1, 1), (-1, -1, 1), (-1, -1, -1)):
            np.testing.assert_array_equal(np.kron(sk * wK[:, r], sl * wL[:, r]), (sk * sl) * wB)
            np.testing.assert_allclose(X.reshape(I, -1) @ np.kron(sa * wA[:, r], np.kron(sk * wK[:, r], sl * wL[:, r])), (sa * sk * sl) * t4,
                                       rtol=1e-12, atol=1e-12)
    # align_factors on three modes: d_a is the product of the three flips, and the aligned model predicts what the model did
    ref = [[wA, wK, wL]]
    flips = np.array([[1, -1, -1], [-1, -1, 1], [1, 1, -1]], dtype=float)            # mode x component
    model = [[wA * flips[0], wK * flips[1], wL * flips[2]]]
    Q, coef = rng.standard_normal((M, R)), np.triu(rng.standard_normal((R, R)))
    blocks, Qa, ca = align_factors(ref, model, Q, coef)
    for got, want in zip(blocks[0], ref[0]):
        np.testing.assert_array_equal(got, want)
    d = flips.prod(axis=0)
    np.testing.assert_array_equal(Qa, Q * d)
    np.testing.assert_array_equal(ca, coef * d[:, None] * d[None, :])
    T = np.stack([np.einsum("iakl,a,k,l->i", X, *(f[:, r] for f in model[0])) for r in range(R)], axis=1)
    Ta = np.stack([np.einsum("iakl,a,k,l->i", X, *(f[:, r] for f in blocks[0])) for r in range(R)], axis=1)
    np.testing.assert_allclose(Ta @ ca @ Qa.T, T @ coef @ Q.T, rtol=1e-11, atol=1e-11)
