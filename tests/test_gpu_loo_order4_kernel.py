"""cmtfpls_loo_xcov_tensor_f64 (leave-one-out of an I x A x B1 x B2 X, a workgroup per fold with the rank-1 CP of the fold's
cross-covariance inside it) against float64 oracle refits whose extraction is oracle.rank1_factors
(tests/loo_order4_ref.py): Ypred at DESIGN 8m's order-4 prediction tolerance (1e-7 relative to max|Y|), n_iter equal per fold and
component, a chunked call bitwise the whole one, the limits; and cmtfpls_loo_xcov_f64 through the templated kernel against the bits
the order-2/3 kernel gave before it was a template (tests/golden/loo_xcov_order3.npz, recorded on the GPU at the parent commit);
and the order-4 entry against the bits it gave before the fold's steps moved into fold_loop.hpp and loo_xcov_fold.hpp
(tests/golden/loo_xcov_tensor_parent.npz, written by tools/xcov_folds_dump.py on the GPU from the library of the commit before)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cmtf_pls_amd import _lib
from loo_order4_ref import loo_case

pytestmark = pytest.mark.gpu

R, SEED, TOL, MAX_ITER = 3, 3, 1e-8, 100
SHAPES = [(9, 5, 7, 3),        # the general case
          (8, 40, 3, 2),       # the transpose path of lx_rank1 (A > B1 B2)
          (7, 3, 16, 16),      # a whole MFMA tile in the unfolding Grams
          (8, 6, 1, 5),        # a mode of size 1, still a CP
          (8, 6, 5, 1),
          (10, 4, 17, 2)]      # a tile remainder
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_xcov_order3.npz")
PARENT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_xcov_tensor_parent.npz")


def _dev(a, dtype=torch.float64):
    return torch.from_numpy(np.array(a, order="C")).to(device="cuda:0", dtype=dtype)      # (a copy: the cached cases are read-only)


def _call(X, Y, chunks):
    """The C entry on X (I x A x B1 x B2), one launch per (fold0, nfolds) of `chunks`: (status of the last launch, Ypred, n_iter)."""
    lib = _lib.load()
    I, A, B1, B2 = X.shape
    M = Y.shape[1]
    Xd, Yd = _dev(X.reshape(I, -1)), _dev(Y)
    cx, cy = Xd.sum(dim=0), Yd.sum(dim=0)
    pred = torch.full((I, M), float("nan"), dtype=torch.float64, device="cuda:0")
    n_iter = torch.full((I, R), -1, dtype=torch.int32, device="cuda:0")
    per = lib.cmtfpls_loo_xcov_tensor_fold_workspace_bytes(I, A, B1, B2, M, R)
    rc = 0
    for f0, nf in chunks:
        nbytes = per * nf
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        rc = lib.cmtfpls_loo_xcov_tensor_f64(Xd.data_ptr(), Yd.data_ptr(), cx.data_ptr(), cy.data_ptr(), I, A, B1, B2, M, R, TOL, MAX_ITER,
                                             f0, nf, pred.data_ptr(), n_iter.data_ptr(), ws.data_ptr(), nbytes, None)
        torch.cuda.synchronize()
    return rc, pred.cpu().numpy(), n_iter.cpu().numpy()


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_entry_equals_oracle_refits(shape, M):
    X, Y, want, want_iter = loo_case(shape, M, R, SEED)
    I = shape[0]
    rc, pred, n_iter = _call(X, Y, [(0, I)])
    assert rc == 0
    err = float(np.abs(pred - want).max() / np.abs(Y).max())
    print(f"{shape} M={M}: max|Ypred - oracle| / max|Y| = {err:.2e}; iterations {int(n_iter.min())}..{int(n_iter.max())}")
    assert np.array_equal(n_iter, want_iter), (n_iter, want_iter)
    assert err <= 1e-7
    rc, pred2, n_iter2 = _call(X, Y, [(0, 4), (4, I - 4)])                             # two launches: the same bits
    assert rc == 0 and np.array_equal(pred2, pred) and np.array_equal(n_iter2, n_iter)


def test_order3_entry_keeps_the_bits_of_the_untemplated_kernel():
    g = np.load(GOLDEN)
    lib = _lib.load()
    for c in range(int(g["n_cases"])):
        X, Y = g[f"X{c}"], g[f"Y{c}"]
        I, A, B = X.shape
        M, Rc = Y.shape[1], int(g[f"n_iter{c}"].shape[1])
        Xd, Yd, cx, cy = _dev(X.reshape(I, -1)), _dev(Y), _dev(g[f"colsum_x{c}"]), _dev(g[f"colsum_y{c}"])
        pred = torch.zeros(I, M, dtype=torch.float64, device="cuda:0")
        n_iter = torch.zeros(I, Rc, dtype=torch.int32, device="cuda:0")
        nbytes = lib.cmtfpls_loo_xcov_fold_workspace_bytes(I, A, B, M, Rc) * I
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
        rc = lib.cmtfpls_loo_xcov_f64(Xd.data_ptr(), Yd.data_ptr(), cx.data_ptr(), cy.data_ptr(), I, A, B, M, Rc, TOL, MAX_ITER, 0, I,
                                      pred.data_ptr(), n_iter.data_ptr(), ws.data_ptr(), nbytes, None)
        torch.cuda.synchronize()
        assert rc == 0
        assert np.array_equal(pred.cpu().numpy(), g[f"Ypred{c}"]), (c, np.abs(pred.cpu().numpy() - g[f"Ypred{c}"]).max())
        assert np.array_equal(n_iter.cpu().numpy(), g[f"n_iter{c}"])


def test_order4_entry_keeps_the_bits_of_the_kernel_before_the_shared_steps():
    from cmtf_pls_amd.backend import HipBackend
    be = HipBackend(torch.device("cuda:0"))
    g = np.load(PARENT)
    assert os.path.getsize(PARENT) < 128 * 1024
    runs = 0
    for s in range(int(g["n_sets"])):
        if f"s{s}/shape1" in g.files:                                                 # several blocks: the coupled entry's
            continue
        A, B1, B2 = (int(v) for v in g[f"s{s}/shape0"])
        X = _dev(g[f"s{s}/X0"])
        R4 = int(g["R"])
        for j, M in enumerate(g["Ms"]):                                               # the runs' outputs lie side by side in M order
            Y = _dev(g[f"s{s}/Y"][:, :M])
            c0 = int(g["Ms"][:j].sum())
            for stop, (tol, max_iter) in zip(g["stops"], g["stop_values"]):
                pred, n_iter = be.loo_tpls_tensor(X, Y, A, B1, B2, R4, float(tol), int(max_iter))
                want = g[f"s{s}/t/{stop}/Ypred"][:, c0:c0 + M]
                assert np.array_equal(pred.cpu().numpy(), want), ((A, B1, B2), M, stop, np.abs(pred.cpu().numpy() - want).max())
                assert np.array_equal(n_iter.cpu().numpy(), g[f"s{s}/t/{stop}/n_iter"][:, R4 * j:R4 * (j + 1)]), ((A, B1, B2), M, stop)
                runs += 1
    assert runs == 30                                                                 # five shapes, M = 1, 5, 17, two stops


def _limit(I, A, B1, B2, M, Rr, ws_bytes):
    """The entry's status on a shape description: X, Y and the column sums are one small buffer, which a declined call never reads
    (a launch would leave Ypred's NaN overwritten and n_iter set)."""
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float64, device="cuda:0")
    pred = torch.full((64,), float("nan"), dtype=torch.float64, device="cuda:0")
    ws = torch.empty(64, dtype=torch.uint8, device="cuda:0")
    rc = lib.cmtfpls_loo_xcov_tensor_f64(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), I, A, B1, B2, M, Rr, TOL, MAX_ITER, 0, 1,
                                         pred.data_ptr(), None, ws.data_ptr(), ws_bytes, None)
    torch.cuda.synchronize()
    assert torch.isnan(pred).all()                                                    # nothing ran
    return rc, lib.cmtfpls_last_error().decode()


def test_limits_decline_before_any_launch():
    EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4
    lib = _lib.load()
    for dims in ((257, 272, 1), (17, 257, 16), (17, 16, 257)):                       # an unfolding with its shorter side > 256
        rc, msg = _limit(4, *dims, 2, 2, 1 << 40)
        assert rc == EUNSUPPORTED and "unfolding" in msg, (dims, rc, msg)
    assert _limit(4, 5, 7, 3, 129, 2, 1 << 40)[0] == EUNSUPPORTED                     # M > 128
    assert _limit(4, 5, 7, 3, 2, 65, 1 << 40)[0] == EUNSUPPORTED                      # R > 64
    assert _limit(4, 256, 256, 257, 2, 2, 1 << 40)[0] == EUNSUPPORTED                 # A B1 B2 > 2^24
    assert _limit(4, 4, 200, 50, 2, 2, 1 << 40)[0] == EUNSUPPORTED                    # 2 B1 B2 doubles of LDS alone > 150 KB
    assert _limit(4, 5, 0, 3, 2, 2, 1 << 40)[0] == EINVAL                             # B1 = 0
    assert _limit(4, 5, 7, -1, 2, 2, 1 << 40)[0] == EINVAL
    per = lib.cmtfpls_loo_xcov_tensor_fold_workspace_bytes(9, 5, 7, 3, 2, 3)
    # I P + I M + I R + M P + 6 P + 2 n^2 + 2 I + R (A + B): P = 105, n = 7 (the unfoldings' short sides are 5, 7, 3)
    assert per == 8 * (9 * 105 + 9 * 2 + 9 * 3 + 2 * 105 + 6 * 105 + 2 * 7 * 7 + 2 * 9 + 3 * (5 + 21))
    assert _limit(9, 5, 7, 3, 2, 3, per - 8)[0] == EWORKSPACE                         # one double short
    assert lib.cmtfpls_loo_xcov_tensor_fold_workspace_bytes(9, 5, 0, 3, 2, 3) == 0
