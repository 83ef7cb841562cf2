"""cmtfpls_loo_xcov_coupled_f64 (loo_xcov_coupled.hip: leave-one-out refits of a ctPLS on complete data, a 1024-thread workgroup per
held-out sample on the cross-covariances of the fold's blocks) through the backend and the C entry, at the limits it declares.

Declared limits: at most 8 blocks of order 2 or 3, min(A_b, B_b) <= 256, M <= 128, R <= 64, P_b <= 2^24, the fold's small vectors within
150 KB of dynamic LDS.  Which branch a case is there for is computed by loo_coupled_ref.loo_coupled_form, a mirror of the entry's
rules written from the kernel's header, and every case asserts it; tests/test_loo_coupled_ref_cpu.py proves the mirror against the
library's host functions and the input conditions without a GPU.

Reference: loo_coupled_ref.loo_literal, literal refits over the float64 oracle (oracle.fit_ctpls's loop, oracle.predict), on every
fold of the three basic cases and on the first, middle and last fold of the limit cases.  Every case runs twice: tol = 1e-8 with 100
passes at most (get_q2y's), and tol = 0 with 3 passes, where no convergence decision exists.
Predictions: normwise (max|got - want| / max(1, max|want|)) <= max(1e-8, 10 x condition_probe), the rule of
test_gpu_loo_xcov_limits.py; condition_probe is the distance of the same refits iterated on the S_b in NumPy from the literal ones
(two correct float64 evaluations), computed when the test runs, on the CPU.  Probes (CPU) and bounds:

    case                              run              condition_probe    bound    measured error (MI355X)
    I12-5x7+9-M3-R3                   tol 1e-8         3.5e-11            1e-8     4.2e-11
    I12-5x7+9-M3-R3                   tol 0, 3 passes  5.2e-11            1e-8     4.5e-11
    I10-17x33+33x17+40-M2-R2          tol 1e-8         3.7e-16            1e-8     3.0e-16
    I10-17x33+33x17+40-M2-R2          tol 0, 3 passes  1.3e-15            1e-8     8.5e-16
    I9-8blocks-M1-R2                  tol 1e-8         0                  1e-8     1.1e-15
    I9-8blocks-M1-R2                  tol 0, 3 passes  0                  1e-8     4.7e-16
    I8-256x256+40-M2-R2               tol 1e-8         3.0e-16            1e-8     5.9e-16
    I8-256x256+40-M2-R2               tol 0, 3 passes  7.4e-16            1e-8     4.5e-16
    I12-5x7+9-M128-R3                 tol 1e-8         6.7e-12            1e-8     6.9e-12
    I12-5x7+9-M128-R3                 tol 0, 3 passes  8.6e-12            1e-8     6.3e-12
    I70-8x9+12-M2-R64                 tol 1e-8         6.5e-11            1e-8     8.1e-11
    I70-8x9+12-M2-R64                 tol 0, 3 passes  4.4e-11            1e-8     8.1e-11
    I10-3x4+9574-M3-R2                tol 1e-8         4.7e-16            1e-8     3.7e-16
    I10-3x4+9574-M3-R2                tol 0, 3 passes  4.0e-16            1e-8     1.9e-16

(ten times every probe is below the floor of 1e-8, so every case is held to 1e-8.  The mixed-order, M = 128 and R = 64 cases are
low rank with noise 1e-10: with noisy inputs the coupled loop converges linearly with a ratio above 1/2, which puts nearly every
pass count on the threshold, and the R = 64 case is chaotic.)

Pass counts (tol = 1e-8): equal to the reference's for every (fold, component) whose reference convergence norm |u_old - u| lies
outside [tol / 2, 2 tol] on the passing step and on the step before it (loo_xcov_ref.on_threshold)."""
import numpy as np
import pytest
import torch

import loo_coupled_ref as C
import loo_xcov_ref as L

pytestmark = pytest.mark.gpu

_DEV = "cuda:0"
EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4
RUNS = [(C.TOL, C.MAX_ITER), (C.CAP_TOL, C.CAP_ITER)]
TAIL = 4096


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(_DEV))


def _dev(a, I):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C").reshape(I, -1)).to(_DEV)     # (a copy: the cached cases are read-only)


def _inputs(case):
    xs, y = C._data(case)
    return [_dev(x, case[0]) for x in xs], _dev(y, case[0]), [(len(t) + 1, *C.split(t)) for t in case[1]]


def _form(case):
    """The case's form from the mirror, with the branch values the table claims asserted."""
    form, why = C.loo_coupled_form(case[0], case[1], case[2], case[3])
    assert form is not None, (case, why)
    assert {k: form[k] for k in case[8]} == case[8], (case, form)
    return form


# ---- 1. every case against the literal refits --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol,max_iter", RUNS, ids=["converged", "capped"])
@pytest.mark.parametrize("case", C.MATCH_CASES, ids=[C.case_id(c) for c in C.MATCH_CASES])
def test_each_case_matches_the_literal_refits(be, case, tol, max_iter):
    I, R = case[0], case[3]
    _form(case)
    Xs, Y, dims = _inputs(case)
    out = be.loo_ctpls(Xs, Y, dims, R, tol, max_iter)
    assert out is not None and out[2] == "xcov_coupled"
    folds = list(C.case_folds(case))
    pred, n_iter = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert np.isfinite(pred).all()
    ref = C.reference(case, tol, max_iter)
    probe = C.case_probe(C.case_id(case), tol, max_iter)
    bound = C.case_bound(case, tol, max_iter)
    err = C.normwise(pred[folds], ref["pred"])
    print(f"{C.case_id(case)} tol={tol:g}: normwise {err:.2e} (probe {probe:.2e}, bound {bound:.2e}); passes {int(n_iter.min())}..{int(n_iter.max())}")
    if tol == 0.0:
        assert (n_iter == max_iter).all() and (ref["n_iter"] == max_iter).all()     # every fold, every component: the cap exactly
    else:
        firm = ~C.on_threshold(ref, tol)
        assert np.array_equal(n_iter[folds][firm], ref["n_iter"][firm]), (n_iter[folds], ref["n_iter"], firm)
    assert err <= bound, (err, bound)


# ---- 2. a fold range through the C entry -------------------------------------------------------------------------------------------
def _blocks(Xs, dims):
    from cmtf_pls_amd import _lib
    sums = [X.sum(dim=0) for X in Xs]
    arr = (_lib.LooCoupledBlock * len(Xs))(*[_lib.LooCoupledBlock(X.data_ptr(), s.data_ptr(), o, A, B) for X, s, (o, A, B) in zip(Xs, sums, dims)])
    return arr, sums


def test_a_fold_range_leaves_the_other_rows_alone(be):
    case = C.RANGE_CASE
    I, M, R = case[0], case[2], case[3]
    f0, nf = C.RANGE
    per = _form(case)["ws_bytes_per_fold"]
    Xs, Y, dims = _inputs(case)
    blocks, sums = _blocks(Xs, dims)
    cy = Y.sum(dim=0)
    pred = torch.full((I, M), float("nan"), dtype=torch.float64, device=_DEV)
    n_iter = torch.full((I, R), -7, dtype=torch.int32, device=_DEV)
    ws = torch.full((per * nf + TAIL,), 0xA5, dtype=torch.uint8, device=_DEV)
    rc = be.lib.cmtfpls_loo_xcov_coupled_f64(blocks, len(Xs), Y.data_ptr(), cy.data_ptr(), I, M, R, C.TOL, C.MAX_ITER, f0, nf,
                                             pred.data_ptr(), n_iter.data_ptr(), ws.data_ptr(), per * nf, be._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((ws[per * nf:] == 0xA5).all()), "workspace written past per * nfolds bytes"
    pred, n_iter = pred.cpu().numpy(), n_iter.cpu().numpy()
    mine = np.zeros(I, dtype=bool)
    mine[f0:f0 + nf] = True
    assert np.isnan(pred[~mine]).all() and (n_iter[~mine] == -7).all()
    # the same rows of a launch of all folds with the same column sums: bit for bit
    wpred = torch.empty((I, M), dtype=torch.float64, device=_DEV)
    wit = torch.empty((I, R), dtype=torch.int32, device=_DEV)
    wws = torch.empty((per * I,), dtype=torch.uint8, device=_DEV)
    rc = be.lib.cmtfpls_loo_xcov_coupled_f64(blocks, len(Xs), Y.data_ptr(), cy.data_ptr(), I, M, R, C.TOL, C.MAX_ITER, 0, I,
                                             wpred.data_ptr(), wit.data_ptr(), wws.data_ptr(), per * I, be._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(pred[mine], wpred.cpu().numpy()[mine]) and np.array_equal(n_iter[mine], wit.cpu().numpy()[mine])
    ref = C.reference(case, C.TOL, C.MAX_ITER)
    assert C.normwise(pred[mine], ref["pred"][mine]) <= C.case_bound(case, C.TOL, C.MAX_ITER)
    # one double short of the workspace: refused on the host, nothing written
    before = torch.full((I, M), float("nan"), dtype=torch.float64, device=_DEV)
    rc = be.lib.cmtfpls_loo_xcov_coupled_f64(blocks, len(Xs), Y.data_ptr(), cy.data_ptr(), I, M, R, C.TOL, C.MAX_ITER, f0, nf,
                                             before.data_ptr(), None, ws.data_ptr(), per * nf - 8, be._stream())
    torch.cuda.synchronize()
    be.lib.cmtfpls_clear_error()
    assert rc == EWORKSPACE and bool(torch.isnan(before).all())


def test_backend_chunks_of_three_folds_equal_its_default(be):
    case = C.BASIC_CASES[1]
    Xs, Y, dims = _inputs(case)
    per = _form(case)["ws_bytes_per_fold"]
    whole = be.loo_ctpls(Xs, Y, dims, case[3], C.TOL, C.MAX_ITER)
    three = be.loo_ctpls(Xs, Y, dims, case[3], C.TOL, C.MAX_ITER, max_ws_bytes=per * 3)
    assert torch.equal(whole[0], three[0]) and torch.equal(whole[1], three[1]) and bool(torch.isfinite(whole[0]).all())


# ---- 3. declines: host checks only, no launch --------------------------------------------------------------------------------------
def _status(be, I, dims, M, R, ws_bytes):
    """The entry's status on a shape description: every block, Y and the column sums are one small buffer that a call stopped by the
    host checks never reads; a launch would overwrite Ypred's NaN."""
    from cmtf_pls_amd import _lib
    buf = torch.zeros(64, dtype=torch.float64, device=_DEV)
    pred = torch.full((64,), float("nan"), dtype=torch.float64, device=_DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=_DEV)
    p = buf.data_ptr()
    blocks = (_lib.LooCoupledBlock * len(dims))(*[_lib.LooCoupledBlock(p, p, len(t) + 1, *C.split(t)) for t in dims])
    rc = be.lib.cmtfpls_loo_xcov_coupled_f64(blocks, len(dims), p, p, I, M, R, C.TOL, C.MAX_ITER, 0, 1, pred.data_ptr(), None,
                                             ws.data_ptr() if ws_bytes else None, ws_bytes, be._stream())
    torch.cuda.synchronize()
    be.lib.cmtfpls_clear_error()
    assert bool(torch.isnan(pred).all())                                            # nothing ran
    return rc


@pytest.mark.parametrize("limit", sorted(C.DECLINES))
def test_one_step_past_each_limit_declines_without_launching(be, limit):
    """9 blocks, n = 257, M = 129, R = 65 and LDS 16 bytes over the cap: status 4; one step inside only misses the workspace."""
    inside, past = C.DECLINES[limit]
    assert C.loo_coupled_form(*inside)[0] is not None and C.loo_coupled_form(*past) == (None, limit)
    assert _status(be, *past, 1 << 40) == EUNSUPPORTED
    assert _status(be, *inside, 0) == EWORKSPACE                                    # the shape check comes before the workspace check
    I, dims, M, R = past
    Xs = [torch.zeros(I, int(np.prod(t)), dtype=torch.float64, device=_DEV) for t in dims]
    Y = torch.zeros(I, M, dtype=torch.float64, device=_DEV)
    assert be.loo_ctpls(Xs, Y, [(len(t) + 1, *C.split(t)) for t in dims], R, C.TOL, C.MAX_ITER) is None


# ---- 4. one block: the tPLS kernel's answer ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 17, 33), (12, 33, 17), (10, 40)], ids=str)
def test_one_block_agrees_with_loo_xcov(be, shape):
    M, R = 3, 3
    x, y = L.case_data(shape, M, 4, 0.3, 7)
    I = shape[0]
    A, B = L.split(shape)
    X2, Y = _dev(x, I), _dev(y, I)
    single = be.loo_tpls(X2, Y, A, B, R, C.TOL, C.MAX_ITER, forms=("xcov",))
    mine = be.loo_ctpls([X2], Y, [(len(shape), A, B)], R, C.TOL, C.MAX_ITER)
    assert single is not None and mine is not None
    err = C.normwise(mine[0].cpu().numpy(), single[0].cpu().numpy())
    print(f"{shape}: one block against cmtfpls_loo_xcov_f64: normwise {err:.2e}")
    folds = (0, I // 2, I - 1)
    probe = L.normwise(L._loo(x, y, R, C.TOL, C.MAX_ITER, folds, True)["pred"], L.loo_literal(x, y, R, folds=folds)["pred"])
    assert err <= max(1e-8, 10.0 * probe)
    ref = L.loo_literal(x, y, R, folds=folds)
    firm = ~L.on_threshold(ref, C.TOL)
    assert np.array_equal(mine[1].cpu().numpy()[list(folds)][firm], ref["n_iter"][firm])
    assert C.normwise(mine[0].cpu().numpy()[list(folds)], ref["pred"]) <= max(1e-8, 10.0 * probe)
