"""cmtfpls_loo_xcov_coupled_tensor_f64 (loo_xcov_coupled.hip, loo_xcov_coupled_kernel<true>: leave-one-out refits of a ctPLS with blocks
of order 4 among blocks of order 2, 3 and 4, a 512-thread workgroup per held-out sample, the rank-1 CP of every order-4 block's
cross-covariance inside it) through the backend and the C entry, at the limits it declares; and cmtfpls_loo_xcov_coupled_f64 through
the templated kernel against the bits the order-2/3 kernel gave before it was a template.

Which branch a case is there for is computed by loo_coupled_order4_ref.form, a mirror of the entry's rules written from the kernel's
header, and every case asserts it; tests/test_loo_coupled_order4_cpu.py proves the mirror against the library's host functions and the
input conditions without a GPU.

Reference: loo_coupled_ref.loo_literal, literal refits over the float64 oracle (oracle.fit_ctpls's loop with oracle.rank1_factors for a
block of any order, oracle.predict), on every fold of the first six cases and on three folds of the limit cases.  Every case runs twice:
tol = 1e-8 with 100 passes at most (get_q2y's), and tol = 0 with 3 passes, where no convergence decision exists.
Predictions: normwise (max|got - want| / max(1, max|want|)) <= max(1e-8, 10 x condition_probe), the rule of
test_gpu_loo_coupled_kernel.py; condition_probe is the distance of the same refits iterated on the S_b in NumPy from the literal ones
(two correct float64 evaluations).  Probes (CPU) and bounds:

    case                              run              condition_probe    bound    measured error (MI355X)
    I10-5x7x3+9+4x6-M3-R3             tol 1e-8         2.1e-11            1e-8     2.3e-11
    I10-5x7x3+9+4x6-M3-R3             tol 0, 3 passes  3.0e-11            1e-8     3.2e-11
    I9-40x3x2+6-M2-R2                 tol 1e-8         5.4e-16            1e-8     1.6e-15
    I9-40x3x2+6-M2-R2                 tol 0, 3 passes  6.8e-16            1e-8     8.1e-16
    I8-3x16x16+17x33-M2-R2            tol 1e-8         3.1e-16            1e-8     2.4e-15
    I8-3x16x16+17x33-M2-R2            tol 0, 3 passes  8.3e-16            1e-8     1.2e-15
    I9-6x1x5+6x5x1+4-M2-R2            tol 1e-8         6.4e-16            1e-8     1.5e-15
    I9-6x1x5+6x5x1+4-M2-R2            tol 0, 3 passes  9.0e-16            1e-8     7.7e-16
    I10-4x17x2+2x3x19-M3-R3           tol 1e-8         3.4e-16            1e-8     6.0e-16
    I10-4x17x2+2x3x19-M3-R3           tol 0, 3 passes  4.7e-16            1e-8     4.3e-16
    I9-8blocks-M1-R2                  tol 1e-8         0                  1e-8     2.4e-16
    I9-8blocks-M1-R2                  tol 0, 3 passes  0                  1e-8     3.6e-16
    I6-256x16x16+40-M2-R2             tol 1e-8         5.3e-16            1e-8     1.2e-15
    I6-256x16x16+40-M2-R2             tol 0, 3 passes  5.3e-16            1e-8     7.1e-16
    I10-5x7x3+9-M128-R3               tol 1e-8         1.2e-11            1e-8     1.5e-11
    I10-5x7x3+9-M128-R3               tol 0, 3 passes  6.2e-12            1e-8     2.8e-12
    I10-3x4x5+9292-M3-R2              tol 1e-8         3.4e-16            1e-8     5.1e-16
    I10-3x4x5+9292-M3-R2              tol 0, 3 passes  3.4e-16            1e-8     3.4e-16

(ten times every probe is below the floor of 1e-8, so every case is held to 1e-8.)

Pass counts (tol = 1e-8): equal to the reference's for every (fold, component) whose reference convergence norm |u_old - u| lies
outside [tol / 2, 2 tol] on the passing step and on the step before it (loo_xcov_ref.on_threshold); 5 of the 151 compared pairs are
on the threshold.

tests/golden/loo_xcov_coupled_order23.npz holds two runs of cmtfpls_loo_xcov_coupled_f64 over all folds (tol 1e-8, 100 passes) recorded
on an MI355X from the library built at the commit before the kernel became a template: the first case of loo_coupled_ref.BASIC_CASES
(I 12, blocks 5 x 7 and 9, M 3, R 3) and loo_coupled_ref.case_data(8, ((17, 5), (5, 17), (11,)), 2, latent 3, noise 0.3, seed 5) with
R 2 (three blocks, both transposes, a tile edge past 16).  Per run c: nb, order, A, B (per block), the blocks X{c}_{b} (I x P_b) and
their column sums colsum_x{c}_{b} (NumPy sums over the rows), Y{c}, colsum_y{c}, and the entry's Ypred{c} and n_iter{c}.

tests/golden/loo_xcov_tensor_parent.npz holds the order-4 cases of tools/xcov_folds_dump.py (its head gives the layout) run through
cmtfpls_loo_xcov_coupled_tensor_f64 on an MI355X by the library of the commit before the fold's steps moved into fold_loop.hpp and
loo_xcov_fold.hpp: every order-4 trailing shape as one block, and the sets of two and three blocks with a block of order 4."""
import ctypes
import os

import numpy as np
import pytest
import torch

import loo_coupled_order4_ref as T
import loo_coupled_ref as C

pytestmark = pytest.mark.gpu

_DEV = "cuda:0"
EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4
RUNS = [(T.TOL, T.MAX_ITER), (T.CAP_TOL, T.CAP_ITER)]
TAIL = 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_xcov_coupled_order23.npz")
PARENT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_xcov_tensor_parent.npz")


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(_DEV))


def _dev(a, I):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C").reshape(I, -1)).to(_DEV)     # (a copy: the cached cases are read-only)


def _describe(dims):
    """(order, A, B) and (B1, B2) per block of the trailing shapes."""
    return [(len(t) + 1, *T.split(t)) for t in dims], [T.pair(t) for t in dims]


def _inputs(case):
    xs, y = T.data(case)
    return ([_dev(x, case[0]) for x in xs], _dev(y, case[0])) + _describe(case[1])


def _form(case):
    """The case's form from the mirror, with the branch values the table claims asserted."""
    form, why = T.form(case[0], case[1], case[2], case[3])
    assert form is not None, (case, why)
    assert {k: form[k] for k in case[8]} == case[8], (case, form)
    return form


def _pairs(pairs):
    flat = [int(v) for p in pairs for v in p]
    return (ctypes.c_int * len(flat))(*flat)


# ---- 1. every case against the literal refits --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol,max_iter", RUNS, ids=["converged", "capped"])
@pytest.mark.parametrize("case", T.CASES, ids=[T.case_id(c) for c in T.CASES])
def test_each_case_matches_the_literal_refits(be, case, tol, max_iter):
    R = case[3]
    _form(case)
    Xs, Y, dims, tensor = _inputs(case)
    out = be.loo_ctpls_tensor(Xs, Y, dims, tensor, R, tol, max_iter)
    assert out is not None
    folds = list(T.case_folds(case))
    pred, n_iter = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert np.isfinite(pred).all()
    ref = T.reference(case, tol, max_iter)
    probe = T.case_probe(T.case_id(case), tol, max_iter)
    bound = T.case_bound(case, tol, max_iter)
    err = T.normwise(pred[folds], ref["pred"])
    print(f"{T.case_id(case)} tol={tol:g}: normwise {err:.2e} (probe {probe:.2e}, bound {bound:.2e}); passes {int(n_iter.min())}..{int(n_iter.max())}")
    if tol == 0.0:
        assert (n_iter == max_iter).all() and (ref["n_iter"] == max_iter).all()     # every fold, every component: the cap exactly
    else:
        firm = ~T.on_threshold(ref, tol)
        assert np.array_equal(n_iter[folds][firm], ref["n_iter"][firm]), (n_iter[folds], ref["n_iter"], firm)
    assert err <= bound, (err, bound)


# ---- 2. a fold range through the C entry -------------------------------------------------------------------------------------------
def _blocks(Xs, dims):
    from cmtf_pls_amd import _lib
    sums = [X.sum(dim=0) for X in Xs]
    arr = (_lib.LooCoupledBlock * len(Xs))(*[_lib.LooCoupledBlock(X.data_ptr(), s.data_ptr(), o, A, B) for X, s, (o, A, B) in zip(Xs, sums, dims)])
    return arr, sums


def test_a_fold_range_leaves_the_other_rows_alone(be):
    case = T.RANGE_CASE
    I, M, R = case[0], case[2], case[3]
    f0, nf = T.RANGE
    per = _form(case)["ws_bytes_per_fold"]
    Xs, Y, dims, tensor = _inputs(case)
    blocks, sums = _blocks(Xs, dims)
    pairs = _pairs(tensor)
    cy = Y.sum(dim=0)
    fn = be.lib.cmtfpls_loo_xcov_coupled_tensor_f64
    pred = torch.full((I, M), float("nan"), dtype=torch.float64, device=_DEV)
    n_iter = torch.full((I, R), -7, dtype=torch.int32, device=_DEV)
    ws = torch.full((per * nf + TAIL,), 0xA5, dtype=torch.uint8, device=_DEV)
    rc = fn(blocks, len(Xs), pairs, Y.data_ptr(), cy.data_ptr(), I, M, R, T.TOL, T.MAX_ITER, f0, nf, pred.data_ptr(), n_iter.data_ptr(),
            ws.data_ptr(), per * nf, be._stream())
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
    rc = fn(blocks, len(Xs), pairs, Y.data_ptr(), cy.data_ptr(), I, M, R, T.TOL, T.MAX_ITER, 0, I, wpred.data_ptr(), wit.data_ptr(),
            wws.data_ptr(), per * I, be._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(pred[mine], wpred.cpu().numpy()[mine]) and np.array_equal(n_iter[mine], wit.cpu().numpy()[mine])
    ref = T.reference(case, T.TOL, T.MAX_ITER)
    assert T.normwise(pred[mine], ref["pred"][mine]) <= T.case_bound(case, T.TOL, T.MAX_ITER)
    # one double short of the workspace: refused on the host, nothing written
    before = torch.full((I, M), float("nan"), dtype=torch.float64, device=_DEV)
    rc = fn(blocks, len(Xs), pairs, Y.data_ptr(), cy.data_ptr(), I, M, R, T.TOL, T.MAX_ITER, f0, nf, before.data_ptr(), None, ws.data_ptr(),
            per * nf - 8, be._stream())
    torch.cuda.synchronize()
    be.lib.cmtfpls_clear_error()
    assert rc == EWORKSPACE and bool(torch.isnan(before).all())


def test_backend_chunks_of_three_folds_equal_its_default(be):
    case = T.CHUNK_CASE
    Xs, Y, dims, tensor = _inputs(case)
    per = _form(case)["ws_bytes_per_fold"]
    whole = be.loo_ctpls_tensor(Xs, Y, dims, tensor, case[3], T.TOL, T.MAX_ITER)
    three = be.loo_ctpls_tensor(Xs, Y, dims, tensor, case[3], T.TOL, T.MAX_ITER, max_ws_bytes=per * 3)
    assert torch.equal(whole[0], three[0]) and torch.equal(whole[1], three[1]) and bool(torch.isfinite(whole[0]).all())


# ---- 3. declines: host checks only, no launch --------------------------------------------------------------------------------------
def _status(be, I, dims, M, R, ws_bytes, orders=None, pairs=None, no_dims=False):
    """The entry's status on a shape description: every block, Y and the column sums are one small buffer that a call stopped by the
    host checks never reads; a launch would overwrite Ypred's NaN."""
    from cmtf_pls_amd import _lib
    buf = torch.zeros(64, dtype=torch.float64, device=_DEV)
    pred = torch.full((64,), float("nan"), dtype=torch.float64, device=_DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=_DEV)
    p = buf.data_ptr()
    orders = orders or [len(t) + 1 for t in dims]
    blocks = (_lib.LooCoupledBlock * len(dims))(*[_lib.LooCoupledBlock(p, p, o, *T.split(t)) for o, t in zip(orders, dims)])
    rc = be.lib.cmtfpls_loo_xcov_coupled_tensor_f64(blocks, len(dims), None if no_dims else _pairs(pairs or [T.pair(t) for t in dims]), p, p,
                                                    I, M, R, T.TOL, T.MAX_ITER, 0, 1, pred.data_ptr(), None,
                                                    ws.data_ptr() if ws_bytes else None, ws_bytes, be._stream())
    torch.cuda.synchronize()
    be.lib.cmtfpls_clear_error()
    assert bool(torch.isnan(pred).all())                                            # nothing ran
    return rc


@pytest.mark.parametrize("limit", sorted(T.DECLINES))
def test_one_step_past_each_limit_declines_without_launching(be, limit):
    """9 blocks, an unfolding at 257, a matrix block at min 257, M = 129, R = 65 and LDS 8 bytes over the cap: status 4; one step inside
    only misses the workspace."""
    inside, past = T.DECLINES[limit]
    assert T.form(*inside)[0] is not None and T.form(*past) == (None, limit)
    assert _status(be, *past, 1 << 40) == EUNSUPPORTED
    assert _status(be, *inside, 0) == EWORKSPACE                                    # the shape check comes before the workspace check
    I, dims, M, R = past
    Xs = [torch.zeros(I, int(np.prod(t)), dtype=torch.float64, device=_DEV) for t in dims]
    Y = torch.zeros(I, M, dtype=torch.float64, device=_DEV)
    assert be.loo_ctpls_tensor(Xs, Y, *_describe(dims), R, T.TOL, T.MAX_ITER) is None


def test_cells_and_bad_descriptions_decline_without_launching(be):
    assert T.form(*T.CELLS_PAST) == (None, "cells") and _status(be, *T.CELLS_PAST, 1 << 40) == EUNSUPPORTED    # P > 2^24
    dims = [(5, 7, 3), (8, 8), (5,)]
    big = 1 << 40
    assert _status(be, 6, dims, 2, 2, 0) == EWORKSPACE                              # the description itself is fine
    assert _status(be, 6, dims, 2, 2, big, no_dims=True) == EINVAL
    assert _status(be, 6, dims, 2, 2, big, pairs=[(7, 3), (0, -1), (0, 0)]) == EINVAL
    assert _status(be, 6, dims, 2, 2, big, pairs=[(7, 4), (0, 0), (0, 0)]) == EINVAL          # B1 B2 != B
    assert _status(be, 6, dims, 2, 2, big, pairs=[(21, 0), (0, 0), (0, 0)]) == EINVAL         # order 4 with B2 = 0
    assert _status(be, 6, dims, 2, 2, big, pairs=[(7, 3), (4, 2), (0, 0)]) == EINVAL          # order 3 with B2 > 0
    assert _status(be, 6, dims, 2, 2, big, orders=[5, 3, 2]) == EINVAL                        # order > 4
    assert _status(be, 6, [(8, 8), (5,)], 2, 2, big) == EINVAL                                # no block of order 4


# ---- 4. one order-4 block: the tPLS kernel's answer --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 5, 7, 3), (8, 40, 3, 2)], ids=str)
def test_one_block_agrees_with_loo_xcov_tensor(be, shape):
    M, R = 2, 2
    I, trail = shape[0], tuple(shape[1:])
    xs, y = C.case_data(I, (trail,), M, 2, 1e-10, 4)
    X2, Y = _dev(xs[0], I), _dev(y, I)
    single = be.loo_tpls_tensor(X2, Y, *trail, R, T.TOL, T.MAX_ITER)
    mine = be.loo_ctpls_tensor([X2], Y, *_describe([trail]), R, T.TOL, T.MAX_ITER)
    assert single is not None and mine is not None
    err = T.normwise(mine[0].cpu().numpy(), single[0].cpu().numpy())
    folds = (0, I // 2, I - 1)
    probe = C.condition_probe(xs, y, R, folds=folds)
    print(f"{shape}: one block against cmtfpls_loo_xcov_tensor_f64: normwise {err:.2e} (probe {probe:.2e})")
    assert err <= max(1e-8, 10.0 * probe)
    ref = C.loo_literal(xs, y, R, folds=folds)
    assert T.normwise(mine[0].cpu().numpy()[list(folds)], ref["pred"]) <= max(1e-8, 10.0 * probe)


# ---- 5. the order-2/3 entry through the templated kernel ---------------------------------------------------------------------------
def test_order23_entry_keeps_the_bits_of_the_untemplated_kernel(be):
    from cmtf_pls_amd import _lib
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 64 * 1024
    for c in range(int(g["n_cases"])):
        nb = int(g[f"nb{c}"])
        Y, cy = _dev(g[f"Y{c}"], g[f"Y{c}"].shape[0]), torch.from_numpy(g[f"colsum_y{c}"]).to(_DEV)
        I, M = Y.shape
        R = int(g[f"n_iter{c}"].shape[1])
        Xs = [_dev(g[f"X{c}_{b}"], I) for b in range(nb)]
        sums = [torch.from_numpy(g[f"colsum_x{c}_{b}"]).to(_DEV) for b in range(nb)]
        blocks = (_lib.LooCoupledBlock * nb)(*[_lib.LooCoupledBlock(X.data_ptr(), s.data_ptr(), int(o), int(A), int(B))
                                               for X, s, o, A, B in zip(Xs, sums, g[f"order{c}"], g[f"A{c}"], g[f"B{c}"])])
        nbytes = be.lib.cmtfpls_loo_xcov_coupled_fold_workspace_bytes(blocks, nb, I, M, R) * I
        ws = torch.empty(nbytes, dtype=torch.uint8, device=_DEV)
        pred = torch.zeros(I, M, dtype=torch.float64, device=_DEV)
        n_iter = torch.zeros(I, R, dtype=torch.int32, device=_DEV)
        rc = be.lib.cmtfpls_loo_xcov_coupled_f64(blocks, nb, Y.data_ptr(), cy.data_ptr(), I, M, R, 1e-8, 100, 0, I, pred.data_ptr(),
                                                 n_iter.data_ptr(), ws.data_ptr(), nbytes, be._stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert np.array_equal(pred.cpu().numpy(), g[f"Ypred{c}"]), (c, np.abs(pred.cpu().numpy() - g[f"Ypred{c}"]).max())
        assert np.array_equal(n_iter.cpu().numpy(), g[f"n_iter{c}"])


def test_tensor_entry_keeps_the_bits_of_the_kernel_before_the_shared_steps(be):
    g = np.load(PARENT)
    runs = 0
    for s in range(int(g["n_sets"])):
        nb = sum(f"s{s}/shape{b}" in g.files for b in range(8))
        trail = [tuple(int(v) for v in g[f"s{s}/shape{b}"]) for b in range(nb)]
        I = g[f"s{s}/Y"].shape[0]
        Xs = [_dev(g[f"s{s}/X{b}"], I) for b in range(nb)]
        dims = [(2, 1, t[1]) if t[0] == 1 and len(t) == 2 else (3, *t) if len(t) == 2 else (4, t[0], t[1] * t[2]) for t in trail]
        tensor = [(t[1], t[2]) if len(t) == 3 else (0, 0) for t in trail]
        R4 = int(g["R"])
        for j, M in enumerate(g["Ms"]):                                               # the runs' outputs lie side by side in M order
            Y = _dev(g[f"s{s}/Y"][:, :M], I)
            c0 = int(g["Ms"][:j].sum())
            for stop, (tol, max_iter) in zip(g["stops"], g["stop_values"]):
                pred, n_iter = be.loo_ctpls_tensor(Xs, Y, dims, tensor, R4, float(tol), int(max_iter))
                want = g[f"s{s}/c/{stop}/Ypred"][:, c0:c0 + M]
                assert np.array_equal(pred.cpu().numpy(), want), (trail, M, stop, np.abs(pred.cpu().numpy() - want).max())
                assert np.array_equal(n_iter.cpu().numpy(), g[f"s{s}/c/{stop}/n_iter"][:, R4 * j:R4 * (j + 1)]), (trail, M, stop)
                runs += 1
    assert runs == 48                                                                 # five single blocks and three sets, M = 1, 5, 17, two stops
