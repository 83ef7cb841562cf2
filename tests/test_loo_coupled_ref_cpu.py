"""tests/loo_coupled_ref.py without a GPU: the mirror of cmtfpls_loo_xcov_coupled_f64's shape rules against the library's own host
functions and host-side status codes (neither reads a data pointer nor touches the GPU), the literal leave-one-out against
oracle.fit_ctpls and oracle.predict, the one-block case against loo_xcov_ref, and the conditions on the inputs of
tests/test_gpu_loo_coupled_kernel.py and tests/test_gpu_loo_coupled.py -- every case on the branch its table claims, the pass counts
that sit on the convergence threshold within the cap, every case well-conditioned enough to test anything."""
import ctypes

import numpy as np
import pytest

import loo_coupled_ref as C
import loo_xcov_ref as L
import oracle as O

EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4


@pytest.fixture(scope="module")
def lib():
    from cmtf_pls_amd import _lib
    return _lib.load()


def _blocks(dims, ptr, orders=None):
    from cmtf_pls_amd import _lib
    orders = orders or [len(d) + 1 for d in dims]
    ab = [C.split(d[:2]) if len(d) <= 2 else (d[0], int(np.prod(d[1:]))) for d in dims]
    return (_lib.LooCoupledBlock * len(dims))(*[_lib.LooCoupledBlock(ptr, ptr, o, A, B) for o, (A, B) in zip(orders, ab)])


SHAPES = [(c[0], c[1], c[2], c[3]) for c in C.MATCH_CASES] + [v[0] for v in C.DECLINES.values()] + [(256, ((64, 64), (128,)), 8, 4)]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(i) for i in range(len(SHAPES))])
def test_lds_and_workspace_mirror_equal_the_library(lib, shape):
    I, dims, M, R = shape
    form, why = C.loo_coupled_form(I, dims, M, R)
    assert form is not None, why
    blocks = _blocks(dims, None)
    assert form["ws_bytes_per_fold"] == lib.cmtfpls_loo_xcov_coupled_fold_workspace_bytes(blocks, len(dims), I, M, R)
    assert form["lds_bytes"] == lib.cmtfpls_loo_xcov_coupled_lds_bytes(blocks, len(dims), I, M, R)


def test_one_block_formulas_are_loo_xcovs(lib):
    for I, A, B, M, R in [(12, 33, 17, 3, 3), (12, 141, 256, 128, 10), (10, 1, 500, 3, 2)]:
        dims = [(B,)] if A == 1 else [(A, B)]
        form, _ = C.loo_coupled_form(I, dims, M, R)
        single, _ = L.loo_xcov_form(I, A, B, M, R)
        assert form["lds_bytes"] == single["lds_bytes"] and form["ws_bytes_per_fold"] == single["ws_bytes_per_fold"]
        assert form["ws_bytes_per_fold"] == lib.cmtfpls_loo_xcov_fold_workspace_bytes(I, A, B, M, R)


def test_lds_bytes_is_the_hand_expanded_sum():
    # wA 5 + 1, wB 7 + 9, q qn tq my 4 x 3, G_y 9, xs 5, ys 9, coef 9, Qs 9, Gn 9, gn bb dd 9
    form, _ = C.loo_coupled_form(12, [(5, 7), (9,)], 3, 3)
    assert form["lds_bytes"] == 8 * (6 + 16 + 12 + 9 + 5 + 9 + 9 + 9 + 9 + 9) and not form["over_48k"]
    # sumP 44, Pmax 35, nmax 5: (12 + 3) 44 + 105 + 50 + 12 (3 + 3 + 2) + 3 (6 + 16)
    assert form["ws_bytes_per_fold"] == 8 * (15 * 44 + 105 + 50 + 96 + 66)
    J = C.longest_row([(3, 4)], 3, 2)
    assert 8 * C.lds_doubles([(3, 4), (J,)], 3, 2) <= C.LDS_CAP < 8 * C.lds_doubles([(3, 4), (J + 1,)], 3, 2)
    assert C.loo_coupled_form(10, [(3, 4), (J,)], 3, 2)[0]["lds_bytes"] == C.LDS_CAP                 # 2 J + 52 doubles


def _probe(lib, I, dims, M, R, ws_bytes, max_iter=100, fold0=0, nfolds=1, orders=None):
    """The entry's answer with stand-in pointers: every status below is decided before a data pointer is read or a kernel launched."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    rc = lib.cmtfpls_loo_xcov_coupled_f64(_blocks(dims, p, orders), len(dims), p, p, I, M, R, 1e-8, max_iter, fold0, nfolds, p, None,
                                          p if ws_bytes else None, ws_bytes, None)
    lib.cmtfpls_clear_error()
    return rc


@pytest.mark.parametrize("limit", sorted(C.DECLINES))
def test_host_checks_agree_with_the_mirror(lib, limit):
    inside, past = C.DECLINES[limit]
    assert C.loo_coupled_form(*inside)[0] is not None and C.loo_coupled_form(*past) == (None, limit)
    assert _probe(lib, *past, 0) == EUNSUPPORTED and _probe(lib, *past, 1 << 40) == EUNSUPPORTED
    assert _probe(lib, *inside, 0) == EWORKSPACE                                    # the shape check comes before the workspace check
    per = C.loo_coupled_form(*inside)[0]["ws_bytes_per_fold"]
    assert _probe(lib, *inside, per - 8) == EWORKSPACE                              # one double short
    if limit == "lds":
        assert C.loo_coupled_form(*inside)[0]["lds_bytes"] == C.LDS_CAP and 8 * C.lds_doubles(*past[1:]) == C.LDS_CAP + 16


def test_order_and_cells_declines(lib):
    assert C.loo_coupled_form(4, [(3, 4), (2, 3, 4)], 2, 2) == (None, "order")
    assert _probe(lib, 4, [(3, 4), (2, 3, 4)], 2, 2, 1 << 40) == EUNSUPPORTED        # an order-4 block (2 x 12 view)
    assert C.loo_coupled_form(4, [(3, 4), ((1 << 24) + 1,)], 2, 2) == (None, "cells")
    assert _probe(lib, 4, [(3, 4), ((1 << 24) + 1,)], 2, 2, 1 << 40) == EUNSUPPORTED
    assert C.loo_coupled_form(4, [(3, 4), (1 << 24,)], 2, 2) == (None, "lds")        # within the cells, past the LDS


def test_bad_arguments_on_the_host(lib):
    dims = [(8, 8), (5,)]
    assert _probe(lib, 1, dims, 2, 2, 0) == EINVAL
    assert _probe(lib, 6, dims, 2, 2, 0, fold0=4, nfolds=3) == EINVAL
    assert _probe(lib, 6, dims, 2, 2, 0, max_iter=0) == EINVAL
    assert _probe(lib, 6, dims, 2, 2, 0, orders=[2, 2]) == EINVAL                   # order 2 with A != 1
    assert _probe(lib, 6, dims, 2, 2, 0, fold0=3, nfolds=3) == EWORKSPACE
    assert lib.cmtfpls_loo_xcov_coupled_fold_workspace_bytes(_blocks(dims, None), 2, 1, 2, 2) == 0
    assert lib.cmtfpls_loo_xcov_coupled_lds_bytes(_blocks([(3,)] * 9, None), 9, 6, 2, 2) == 0


def test_literal_refit_is_the_oracles_fit_factor_for_factor():
    xs, y = C.case_data(9, ((5, 6), (7,), (4, 3)), 3, 3, 0.2, 2)
    keep = np.arange(9) != 4
    for tol, max_iter in ((C.TOL, C.MAX_ITER), (C.CAP_TOL, C.CAP_ITER)):
        mine, du_last, du_prev = C._refit([x[keep] for x in xs], y[keep], 3, tol, max_iter, on_s=False)
        fit = O.fit_ctpls([x[keep] for x in xs], y[keep], 3, tol, max_iter)
        assert np.array_equal(mine.T, fit.T) and np.array_equal(mine.Q, fit.Q) and np.array_equal(mine.U, fit.U)
        assert np.array_equal(mine.coef, fit.coef) and mine.n_iter == fit.n_iter
        for b in range(3):
            for m in range(len(fit.loadings[b])):
                assert np.array_equal(mine.loadings[b][m], fit.loadings[b][m])
        if tol > 0:
            assert (du_last < tol).all() and (du_prev >= tol).all()
    ref = C.loo_literal(xs, y, 3, folds=(0, 4, 8))
    for j, i in enumerate((0, 4, 8)):
        k = np.arange(9) != i
        fit = O.fit_ctpls([x[k] for x in xs], y[k], 3)
        assert np.array_equal(ref["pred"][j], np.asarray(O.predict(fit, [x[i:i + 1] for x in xs])).reshape(-1))
        assert list(ref["n_iter"][j]) == fit.n_iter


def test_one_block_case_equals_loo_xcov_refs_literal():
    x, y = L.case_data((12, 17, 33), 3, 4, 0.3, 7)
    for on_s in (False, True):
        mine = C._loo([x], y, 3, C.TOL, C.MAX_ITER, (0, 6, 11), on_s)
        single = L._loo(x, y, 3, C.TOL, C.MAX_ITER, (0, 6, 11), on_s)
        assert np.array_equal(mine["n_iter"], single["n_iter"])
        assert C.normwise(mine["pred"], single["pred"]) <= 1e-13                    # (np.average of one block and tq / 1: same values)


# ---- the conditions on the GPU suites' inputs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.MATCH_CASES, ids=[C.case_id(c) for c in C.MATCH_CASES])
def test_each_case_is_on_the_branch_its_table_claims(case):
    form, why = C.loo_coupled_form(case[0], case[1], case[2], case[3])
    assert form is not None, why
    assert {k: form[k] for k in case[8]} == case[8]


def test_case_tables_cover_the_limits():
    forms = [C.loo_coupled_form(c[0], c[1], c[2], c[3])[0] for c in C.MATCH_CASES]
    assert max(f["lds_bytes"] for f in forms) == C.LDS_CAP and max(f["nmax"] for f in forms) == C.MAX_N
    assert max(c[2] for c in C.MATCH_CASES) == C.MAX_M and max(c[3] for c in C.MATCH_CASES) == C.MAX_R
    assert max(f["blocks"] for f in forms) == C.MAX_BLOCKS and min(c[2] for c in C.MATCH_CASES) == 1
    assert all(c[0] <= 16 for c in C.MATCH_CASES if c[3] < C.MAX_R) and [c[0] for c in C.MATCH_CASES if c[3] == C.MAX_R] == [70]
    assert any(True in f["transposed"] and False in f["transposed"] for f in forms)
    f0, n = C.RANGE
    assert 0 < f0 and f0 + n < C.RANGE_CASE[0]


def test_pass_counts_on_the_threshold_stay_within_the_cap():
    """A condition on the inputs: of the (fold, component) pairs the GPU suite compares pass counts on, at most 10% may be decisions
    that sat on the threshold in the reference itself (and are therefore not compared)."""
    excluded = total = 0
    for case in C.MATCH_CASES:
        ref = C.reference(case, C.TOL, C.MAX_ITER)
        near = C.on_threshold(ref, C.TOL)
        assert (ref["n_iter"] >= 2).all()
        excluded, total = excluded + int(near.sum()), total + near.size
        capped = C.reference(case, C.CAP_TOL, C.CAP_ITER)
        assert (capped["n_iter"] == C.CAP_ITER).all() and np.isfinite(capped["pred"]).all()
    print(f"{excluded} of {total} pairs on the threshold")
    assert excluded <= C.EXCLUDED_CAP * total, (excluded, total)


@pytest.mark.parametrize("case", C.MATCH_CASES, ids=[C.case_id(c) for c in C.MATCH_CASES])
def test_cases_are_well_conditioned(case):
    """10 x condition_probe beyond 1e-4 would mean the case tests nothing: its seed or noise has to change then, not the factor."""
    for tol, max_iter in ((C.TOL, C.MAX_ITER), (C.CAP_TOL, C.CAP_ITER)):
        probe = C.case_probe(C.case_id(case), tol, max_iter)
        print(f"{C.case_id(case)} tol={tol:g}: condition_probe {probe:.2e}, bound {C.case_bound(case, tol, max_iter):.2e}")
        assert 10.0 * probe <= 1e-4
        assert C.case_bound(case, tol, max_iter) == max(1e-8, 10.0 * probe)
