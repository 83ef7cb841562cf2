"""Device cross-validation of a ctPLS with blocks of order 4, the parts that need no GPU: the NumPy restatement of the
coupled fold loop (tests/kfold_coupled_order4_ref.py) against the order-4 restatement and against oracle.fit_ctpls refits of whole
folds, the LDS formula of the entry, and the wording of kfold._decline_blocks for coupled blocks of order 4."""
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import _lib, kfold
from cmtf_pls_amd.backend import _int_pairs
from cmtf_pls_amd.options import EngineOptions
from kfold_coupled_order4_ref import coupled_data, coupled_inner_loop
from kfold_order4_ref import inner_loop, planted

SHAPES, M, R, K = [(48, 6, 5, 4), (48, 7)], 3, 3, 4


def _rel(got, want):
    return np.linalg.norm(np.asarray(got) - np.asarray(want)) / np.linalg.norm(want)


def test_one_block_is_the_order4_restatement():
    for dims, m, seed in (((5, 7, 3), 2, 1), ((6, 1, 5), 3, 2)):
        S, Gy = planted(dims, m, 2, seed)
        for k in range(2):
            got, want = coupled_inner_loop([S[k]], Gy, [dims]), inner_loop(S[k], Gy, dims)
            assert got["n_iter"] == want["n_iter"] and np.array_equal(got["q"], want["q"])
            for f, name in zip(got["blocks"][0]["modes"], ("wA", "wK", "wL")):
                assert np.array_equal(f, want[name]), name
            assert np.array_equal(got["blocks"][0]["w"], np.kron(want["wA"], want["wB"]))


def test_restatement_reproduces_oracle_refits_of_whole_folds():
    """Every fold of the K-fold case of tests/test_gpu_kfold_coupled_order4.py, every component: the restatement on S_b = Yc^T Xc_b
    of the deflated training data gives the loadings, q and n_iter of oracle.fit_ctpls.  The deflation between components is the
    oracle's (cmtf.py:130-139), done here on the host."""
    Xs, y = coupled_data(SHAPES, M, R + 1, seed=7)
    ids, _ = kfold.fold_ids(SHAPES[0][0], K)
    dims = [s[1:] for s in SHAPES]
    seen = []
    for k in range(K):
        tr = ids != k
        fit = O.fit_ctpls([X[tr] for X in Xs], y[tr], R)
        Xc = [(X[tr] - X[tr].mean(axis=0)).reshape(int(tr.sum()), -1) for X in Xs]
        Yc = y[tr] - y[tr].mean(axis=0)
        T = np.zeros((int(tr.sum()), R))
        for a in range(R):
            got = coupled_inner_loop([Yc.T @ X for X in Xc], Yc.T @ Yc, [(1, 7) if len(d) == 1 else d for d in dims])
            assert got["n_iter"] == fit.n_iter[a], (k, a, got["n_iter"], fit.n_iter[a])
            seen.append(got["n_iter"])
            for b in range(len(Xs)):
                for m, f in enumerate(got["blocks"][b]["modes"]):
                    assert _rel(f, fit.loadings[b][m][:, a]) <= 1e-10, (k, a, b, m)
            assert _rel(got["q"], fit.Q[:, a]) <= 1e-10
            T[:, a] = np.mean([X @ blk["w"] for X, blk in zip(Xc, got["blocks"])], axis=0)      # cmtf.py:120
            assert _rel(T[:, a], fit.T[:, a]) <= 1e-10
            Xc = [X - np.outer(T[:, a], blk["w"]) for X, blk in zip(Xc, got["blocks"])]
            coef = np.linalg.lstsq(T, Yc @ got["q"], rcond=-1)[0]
            Yc = Yc - np.outer(T @ coef, got["q"])
    print("inner iterations per fold and component:", seen)
    assert 6 <= min(seen) and max(seen) <= 38, seen                                              # converged, well inside max_iter


class _StubBackend:
    name = "stub"

    def __init__(self, entry=True):
        for f in ("kfold_xcov", "kfold_inner", "kfold_epilogue", "mttkrp", "xcov", "kfold_inner_coupled", "kfold_combine_scores",
                  "kfold_inner_tensor"):
            setattr(self, f, lambda *a, **k: None)
        if entry:
            self.kfold_inner_coupled_tensor = lambda *a, **k: None


def _stub_model(entry=True, **opt):
    eng = SimpleNamespace(be=_StubBackend(entry), opt=EngineOptions(**opt))
    return SimpleNamespace(_get_engine=lambda: eng, _comm=None, n_components=R)


_COUPLED = ("kfold_xcov", "kfold_inner_coupled", "kfold_combine_scores", "kfold_epilogue", "mttkrp", "xcov")


def _decline(shapes, m=M, entry=True, tensor_ok=True, **opt):
    opt = opt or {"tensor_folds_coupled": True}
    Xs = [np.zeros(s, dtype=np.float32) for s in shapes]
    return kfold._decline_blocks(_stub_model(entry, **opt), Xs, [f"block {b}" for b in range(len(Xs))], np.zeros((shapes[0][0], m)),
                                 K, _COUPLED, tensor_ok=tensor_ok)


def test_tensor_dims_per_block():
    Xs = [np.zeros(s) for s in [(8, 6, 5, 4), (8, 7), (8, 3, 2)]]
    assert kfold._tensor_dims(Xs, True) == [(5, 4), (0, 0), (0, 0)]
    assert kfold._tensor_dims(Xs[1:], True) is None and kfold._tensor_dims(Xs[:1], False) == (5, 4)
    assert [kfold._dims(X) for X in Xs] == [(6, 20), (1, 7), (3, 2)]


def _lds_bytes(dims, tensor, m, nb=None):
    """cmtfpls_kfold_inner_coupled_tensor_lds_bytes of blocks dims = [(A, B), ..], tensor = [(B1, B2), ..], on states with null buffers."""
    states = kfold._size_states(dims, m)
    return _lib.load().cmtfpls_kfold_inner_coupled_tensor_lds_bytes(states, len(dims) if nb is None else nb, _int_pairs(tensor))


def _carve_up(dims, tensor, m):
    """The LDS of the kernel as include/cmtfpls.h lists it (doubles): wA, wB, q, qn, tq, G_y, xs, ys, then the CP's wK, wL, v, tmp, part."""
    mats = [(A, B) for (A, B), (_, B2) in zip(dims, tensor) if B2 == 0]
    tens = [(A, B1, B2) for (A, _), (B1, B2) in zip(dims, tensor) if B2 > 0]
    xs = max([min(A, B) for A, B in mats] + [min(d, A * B1 * B2 // d) for A, B1, B2 in tens for d in (A, B1, B2)])
    ys = max([max(A, B) for A, B in mats], default=0)
    cp = [max((t[i] for t in tens), default=0) for i in (1, 2)] + [max((B1 * B2 for _, B1, B2 in tens), default=0),
                                                                    max((max(t) for t in tens), default=0), 1024]
    return 8 * (max(A for A, _ in dims) + max(B for _, B in dims) + 3 * m + m * m + xs + ys + sum(cp))


def test_lds_formula_of_the_coupled_tensor_entry():
    # one block of order 4: the formula of cmtfpls_kfold_inner_tensor_f64 (A, 2 B, 3 M, M^2, nmax, B1, B2, max dim, part)
    assert _lds_bytes([(6, 20)], [(5, 4)], 3) == 8 * (6 + 2 * 20 + 9 + 9 + 6 + 5 + 4 + 6 + 1024)
    # tensor + order 2 + order 3: amax 5, bmax 21, n = max(5, 7, 3 | 1 | 4) = 7, k = max(9, 6) = 9 over the matrix blocks alone
    got = _lds_bytes([(5, 21), (1, 9), (6, 4)], [(7, 3), (0, 0), (0, 0)], 3)
    assert got == 8 * (6 + 21 + 9 + 9 + 7 + 9 + 7 + 3 + 21 + 7 + 1024)


# a cube, the Gram seed from the B1 unfolding (16, not 3), M = 1, tensor blocks next to matrix blocks, 8 blocks, then blocks past a
# limit of the entry (a short side of 257 in an unfolding and in a matrix block, M = 65, more than 2^24 cells) and the two sides of
# the 150 KB cap ((1, 9000) next to 2 x 90 x 90 is 218 984 bytes: far past it): the byte count is not gated by them
LDS_BLOCKS = [([(5, 25)], [(5, 5)], 2), ([(3, 256)], [(16, 16)], 1), ([(6, 20), (1, 7)], [(5, 4), (0, 0)], 1),
              ([(5, 21), (1, 9), (6, 4)], [(7, 3), (0, 0), (0, 0)], 3), ([(3, 2)] * 7 + [(2, 6)], [(0, 0)] * 7 + [(3, 2)], 2),
              ([(17, 257 * 16), (1, 7)], [(257, 16), (0, 0)], 2), ([(257, 300), (6, 20)], [(0, 0), (5, 4)], 2),
              ([(6, 20), (1, 7)], [(5, 4), (0, 0)], 65), ([(257, 256 * 256)], [(256, 256)], 2), ([(1, 9000), (2, 8100)], [(0, 0), (90, 90)], 3),
              ([(1, 4540)], [(1, 4540)], 2), ([(1, 4541)], [(1, 4541)], 2)]


@pytest.mark.parametrize("dims, tensor, m", LDS_BLOCKS, ids=lambda v: str(v).replace(" ", ""))
def test_exported_lds_bytes_is_the_carve_up(dims, tensor, m):
    assert _lds_bytes(dims, tensor, m) == _carve_up(dims, tensor, m)
    if len(dims) == 1:                          # one block of order 4: the order-4 entry's own function
        assert _lds_bytes(dims, tensor, m) == _lib.load().cmtfpls_kfold_inner_tensor_lds_bytes(dims[0][0], *tensor[0], m)


def test_exported_lds_bytes_over_the_cap_and_malformed():
    assert _lds_bytes([(1, 4541)], [(1, 4541)], 2) - 32 == _lds_bytes([(1, 4540)], [(1, 4540)], 2) == 150 * 1024 - 24
    good = ([(6, 20), (1, 7)], [(5, 4), (0, 0)])
    assert _lds_bytes(*good, 3) > 0
    assert _lds_bytes(*good, 0) == 0 and _lds_bytes(*good, 3, nb=0) == 0
    assert _lds_bytes([(3, 2)] * 9, [(0, 0)] * 8 + [(2, 1)], 3) == 0                                       # nb = 9
    assert _lds_bytes([(6, 20), (1, 7)], [(5, 5), (0, 0)], 3) == 0                                         # B1 B2 != B
    assert _lds_bytes([(6, 20), (1, 7)], [(5, 4), (7, 0)], 3) == 0 and _lds_bytes([(6, 20), (1, 7)], [(-5, -4), (0, 0)], 3) == 0
    assert _lds_bytes([(0, 20), (1, 7)], [(5, 4), (0, 0)], 3) == 0 and _lds_bytes([(6, 20), (1, 0)], [(5, 4), (0, 0)], 3) == 0
    lib = _lib.load()
    assert lib.cmtfpls_kfold_inner_coupled_tensor_lds_bytes(None, 1, _int_pairs([(5, 4)])) == 0
    assert lib.cmtfpls_kfold_inner_coupled_tensor_lds_bytes(kfold._size_states([(6, 20)], 3), 1, None) == 0


def test_decline_wording_for_coupled_blocks_of_order4():
    old = "block 0 of order 4 (the device form takes order 2 and 3)"
    assert _decline(SHAPES) is None
    assert _decline([(48, 6, 5), (48, 7), (48, 3, 4, 7)]) is None
    assert _decline(SHAPES, tensor_folds=True) == old                                # the option is off: as it always was, verbatim
    assert _decline(SHAPES, small_fit=False) == old
    assert _decline(SHAPES, tensor_ok=False) == old                                  # a caller whose passes do not take it (bootstrap)
    assert _decline(SHAPES, entry=False) == "the stub backend has no order-4 coupled K-fold kernel"
    assert _decline([(8, 7), (8, 17, 257, 16)]) == "block 1: mode-1 unfolding: min(257, 272) = 257 > 256"
    assert _decline([(8, 300, 17, 16), (8, 7)]) == "block 0: mode-0 unfolding: min(300, 272) = 272 > 256"
    lds = 8 * (2 + 9000 + 9 + 9 + 90 + 9000 + 90 + 90 + 8100 + 90 + 1024)       # (1, 9000) and 2 x 90 x 90: each alone fits
    assert _decline([(8, 9000), (8, 2, 90, 90)]) == \
        f"the blocks' vectors need {lds} bytes of LDS > 153600 (cmtfpls_kfold_inner_coupled_tensor_f64)"
    assert _decline([(8, 2, 2, 2, 2), (8, 6, 5, 4)]) == "block 0 of order 5 (the device form takes order 2 and 3)"
    assert _decline([(8, 7), (8, 2, 2, 2, 2)]) == "block 1 of order 5 (the device form takes order 2 and 3)"
    assert _decline(SHAPES, m=65) == "M = 65 responses > 64"
    x = np.zeros(SHAPES[0])
    x[3, 1, 2, 0] = np.nan
    got = kfold._decline_blocks(_stub_model(tensor_folds_coupled=True), [x, np.zeros(SHAPES[1])], ["block 0", "block 1"],
                                np.zeros((48, M)), K, _COUPLED, tensor_ok=True)
    assert got == "missing values in block 0"
