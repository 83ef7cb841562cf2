"""tests/loo_xcov_ref.py without a GPU: the mirror of cmtfpls_loo_xcov_f64's shape rules against the library's own host function
and its host-side status codes (neither touches a pointer or the GPU), the literal leave-one-out against the oracle's own fit and
predict, the re-associated evaluation on a well-conditioned case, and the conditions on the inputs of
tests/test_gpu_loo_xcov_limits.py -- every case on the branch its table claims, the pass counts that sit on the convergence
threshold within the cap, the probed cases well-conditioned enough to test anything."""
import ctypes

import numpy as np
import pytest

import loo_xcov_ref as L
import oracle as O

EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4


@pytest.fixture(scope="module")
def lib():
    from cmtf_pls_amd import _lib
    return _lib.load()


WS_SHAPES = [(8, 255, 256, 2, 2), (8, 256, 255, 2, 2), (8, 241, 300, 3, 2), (8, 256, 256, 2, 2), (12, 16, 33, 3, 3), (12, 33, 17, 3, 3),
             (12, 141, 256, 128, 10), (40, 20, 70, 127, 3), (70, 8, 72, 2, 64), (10, 1, L.longest_row(3, 2), 3, 2), (6, 64, 65, 2, 4),
             (2, 1, 1, 1, 1), (512, 128, 128, 16, 4)]


@pytest.mark.parametrize("dims", WS_SHAPES, ids=[str(d) for d in WS_SHAPES])
def test_workspace_mirror_equals_the_library(lib, dims):
    form, why = L.loo_xcov_form(*dims)
    assert form is not None, why
    assert form["ws_bytes_per_fold"] == lib.cmtfpls_loo_xcov_fold_workspace_bytes(*dims)


def test_lds_bytes_is_the_hand_expanded_sum():
    # wA 141, wB 256, q qn tq my 4 x 128, G_y 128^2, xs 141, ys 256, coef 100, Qs 1280, Gn 100, gn bb dd 30
    assert 141 + 256 + 512 + 16384 + 141 + 256 + 100 + 1280 + 100 + 30 == 19200
    form, _ = L.loo_xcov_form(12, 141, 256, 128, 10)
    assert form["lds_bytes"] == 8 * 19200 == 153600 == L.LDS_CAP and form["over_48k"] and form["m_groups"] == 8
    assert L.loo_xcov_form(12, 141, 257, 128, 10) == (None, "lds")                  # wB and ys one double longer each
    # wA 33, wB 17, 4 x 3, G_y 9, xs 17, ys 33, coef 9, Qs 9, Gn 9, gn bb dd 9
    form, _ = L.loo_xcov_form(12, 33, 17, 3, 3)
    assert form["lds_bytes"] == 8 * (33 + 17 + 12 + 9 + 17 + 33 + 9 + 9 + 9 + 9) and not form["over_48k"]
    assert (form["n"], form["k"], form["transposed"], form["tiles"], form["m_groups"]) == (17, 33, True, 2, 1)
    B = L.longest_row(3, 2)
    assert 8 * L.lds_doubles(1, B, 3, 2) <= L.LDS_CAP < 8 * L.lds_doubles(1, B + 1, 3, 2) and B == (19200 - 43) // 2


def _probe(lib, I, A, B, M, R, ws_bytes, max_iter=100, fold0=0, nfolds=1):
    """The entry's answer with stand-in pointers: every status below is decided before a pointer is read or a kernel launched."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    rc = lib.cmtfpls_loo_xcov_f64(p, p, p, p, I, A, B, M, R, 1e-8, max_iter, fold0, nfolds, p, None, p if ws_bytes else None, ws_bytes, None)
    lib.cmtfpls_clear_error()
    return rc


@pytest.mark.parametrize("limit", sorted(L.DECLINES))
def test_host_checks_agree_with_the_mirror(lib, limit):
    inside, past = L.DECLINES[limit]
    assert L.loo_xcov_form(*inside)[0] is not None and L.loo_xcov_form(*past) == (None, limit)
    for other in set(L.DECLINES) - {limit}:                                         # past the named limit only
        moved = {"n": min(past[1], past[2]) > L.MAX_N, "M": past[3] > L.MAX_M, "R": past[4] > L.MAX_R,
                 "lds": 8 * L.lds_doubles(*past[1:]) > L.LDS_CAP}[other]
        assert not moved, (limit, other)
    assert _probe(lib, *past, 0) == EUNSUPPORTED and _probe(lib, *past, 1 << 40) == EUNSUPPORTED
    assert _probe(lib, *inside, 0) == EWORKSPACE                                    # the shape check comes before the workspace check
    per = lib.cmtfpls_loo_xcov_fold_workspace_bytes(*inside)
    assert _probe(lib, *inside, per - 8) == EWORKSPACE                              # one double short


def test_bad_arguments_on_the_host(lib):
    assert _probe(lib, 1, 8, 8, 2, 2, 0) == EINVAL
    assert _probe(lib, 6, 8, 8, 2, 2, 0, fold0=4, nfolds=3) == EINVAL
    assert _probe(lib, 6, 8, 8, 2, 2, 0, max_iter=0) == EINVAL
    assert _probe(lib, 6, 8, 8, 2, 2, 0, fold0=3, nfolds=3) == EWORKSPACE
    assert lib.cmtfpls_loo_xcov_fold_workspace_bytes(1, 8, 8, 2, 2) == 0


def test_literal_leave_one_out_is_the_oracles_fit_and_predict():
    x, y, _ = O.import_synthetic((9, 5, 6), 3, 3, error=0.2, seed=2)
    ref = L.loo_literal(x, y, 3, folds=(0, 4, 8))
    for j, i in enumerate((0, 4, 8)):
        keep = np.arange(9) != i
        fit = O.fit_tpls(x[keep], y[keep], 3)
        assert np.array_equal(ref["pred"][j], np.asarray(O.predict(fit, x[i:i + 1])).reshape(-1))
        assert list(ref["n_iter"][j]) == fit.n_iter
    assert (ref["du_last"] < 1e-8).all() and (ref["du_prev"] >= 1e-8).all() and list(ref["folds"]) == [0, 4, 8]
    capped = L.loo_literal(x, y, 3, 0.0, 3, folds=(4,))
    assert (capped["n_iter"] == 3).all() and (capped["du_last"] > 0).all()
    xm, ym, _ = O.import_synthetic((9, 30), 2, 3, error=0.2, seed=2)                # a matrix block
    fit = O.fit_tpls(xm[1:], ym[1:], 2)
    assert np.array_equal(L.loo_literal(xm, ym, 2, folds=(0,))["pred"][0], np.asarray(O.predict(fit, xm[:1])).reshape(-1))


def test_condition_probe_on_a_well_conditioned_case():
    x, y, _ = O.import_synthetic((12, 6, 7), 3, 3, error=0.1, seed=4)
    assert L.condition_probe(x, y, 2, folds=(0, 6, 11)) < 1e-10
    assert L.condition_probe(x, y, 2, 0.0, 3, folds=(0, 6, 11)) < 1e-10


def test_threshold_guard():
    ref = {"du_last": np.array([[4e-9, 5e-9, 1e-12, 3.0]]), "du_prev": np.array([[1e-3, 1e-3, 2e-8, np.inf]])}
    assert L.on_threshold(ref, 1e-8).tolist() == [[False, True, True, False]]


# ---- the conditions on the GPU suite's inputs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", L.MATCH_CASES + L.CHUNK_CASES, ids=[L.case_id(c) for c in L.MATCH_CASES + L.CHUNK_CASES])
def test_each_case_is_on_the_branch_its_table_claims(case):
    shape, M, R = case[:3]
    form, why = L.loo_xcov_form(shape[0], *L.split(shape), M, R)
    assert form is not None, why
    assert {k: form[k] for k in case[6]} == case[6]


def test_case_tables_cover_the_edges():
    forms = [L.loo_xcov_form(c[0][0], *L.split(c[0]), c[1], c[2])[0] for c in L.MATCH_CASES]
    assert max(f["lds_bytes"] for f in forms) == L.LDS_CAP and max(f["n"] for f in forms) == L.MAX_N
    assert max(c[1] for c in L.MATCH_CASES) == L.MAX_M and max(c[2] for c in L.MATCH_CASES) == L.MAX_R
    assert {15, 16, 17, 241, 255, 256} <= {f["n"] for f in forms} and any(f["transposed"] and f["n"] == 255 for f in forms)
    assert any(f["k"] % 32 and f["n"] > 128 for f in forms)
    assert {c[1] % 16 for c in L.MATCH_CASES} >= {0, 1, 15}                        # full, and both ragged ends of a response group
    assert [L.case_id(c) for c in L.PROBED] == ["(12, 141, 256)-M128-R10", "(40, 20, 70)-M127-R3", "(70, 8, 72)-M2-R64"]
    lds_form_n = 64                                                                 # kLooMaxN of the lds form (test_gpu_small_fit_limits)
    assert L.split((6, 64, 65)) == (lds_form_n, lds_form_n + 1)


def test_pass_counts_on_the_threshold_stay_within_the_cap():
    """A condition on the inputs: of the (fold, component) pairs the GPU suite compares pass counts on, at most 10% may be decisions
    that sat on the threshold in the reference itself (and are therefore not compared)."""
    excluded = total = 0
    for case in L.MATCH_CASES:
        ref = L.case_reference(*case[:6], L.TOL, L.MAX_ITER)
        near = L.on_threshold(ref, L.TOL)
        assert (ref["n_iter"] >= 2).all()
        excluded, total = excluded + int(near.sum()), total + near.size
        capped = L.case_reference(*case[:6], L.CAP_TOL, L.CAP_ITER)
        assert (capped["n_iter"] == L.CAP_ITER).all() and np.isfinite(capped["pred"]).all()
    print(f"{excluded} of {total} pairs on the threshold")
    assert excluded <= L.EXCLUDED_CAP * total, (excluded, total)


@pytest.mark.parametrize("case", L.PROBED, ids=[L.case_id(c) for c in L.PROBED])
def test_probed_cases_are_well_conditioned(case):
    """10 x condition_probe beyond 1e-4 would mean the case tests nothing: its seed or noise has to change then, not the factor."""
    for tol, max_iter in ((L.TOL, L.MAX_ITER), (L.CAP_TOL, L.CAP_ITER)):
        probe = L.case_probe(*case[:6], tol, max_iter)
        print(f"{L.case_id(case)} tol={tol:g}: condition_probe {probe:.2e}, bound {L.case_bound(case, tol, max_iter):.2e}")
        assert 10.0 * probe <= 1e-4
        assert L.case_bound(case, tol, max_iter) == max(1e-8, 10.0 * probe)
    assert L.case_bound(L.MATCH_CASES[0], L.TOL, L.MAX_ITER) == 1e-8
