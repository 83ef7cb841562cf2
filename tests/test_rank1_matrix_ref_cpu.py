"""CPU-only: the host helpers of the matrix rank-1 extraction tests (tests/rank1_matrix_ref.py) against LAPACK and the oracle,
the exact cases against the model, and the screening of every case list that tests/test_gpu_rank1_matrix_limits.py runs -- a
case that would sit on a convergence threshold fails here and never reaches a GPU."""
import functools

import numpy as np
import pytest

import oracle as O
import rank1_matrix_ref as R


@functools.lru_cache(maxsize=None)
def _dense(A, B, r):
    Z = R.dense_case(A, B, r)
    Z.setflags(write=False)
    return Z, R.model(Z, R.F3_BUDGET), R.svd_pair(Z)


@pytest.mark.parametrize("A,B,r", R.family3_cases())
def test_model_against_lapack_and_the_oracle(A, B, r):
    """The float64 restatement finds LAPACK's leading pair (2e-15 measured at s2/s1 = 0.93; 1e-13 asked), the oracle's
    parafac(Z, 1, init="svd") restatement at the tolerance of test_gpu_kernels.py, sigma_1 within its bound, and its own
    residual -- which the device is held to as well -- within the bound, with exact zeros where Z has a zero line."""
    Z, (wA, wB, sigma, converged, steps, gaps), (u, v, S) = _dense(A, B, r)
    assert converged
    np.testing.assert_allclose(wA, u, rtol=0, atol=1e-13)
    np.testing.assert_allclose(wB, v, rtol=0, atol=1e-13)
    fa, fb = O.rank1_factors(Z)
    if fb[int(np.argmax(np.abs(fb)))] < 0:
        fa, fb = -fa, -fb
    np.testing.assert_allclose(wA, fa, rtol=0, atol=1e-9)
    np.testing.assert_allclose(wB, fb, rtol=0, atol=1e-9)
    assert abs(sigma - S[0]) <= R.sigma_bound(A, B, S[0])
    assert R.residual(Z, wA, wB) <= R.residual_bound(Z, S[0])
    if A >= 4:
        assert wA[A // 2] == 0.0
    if B >= 4:
        assert wB[B // 3] == 0.0


def test_family3_screening():
    """info is asserted on the GPU exactly where every step's 1 - rho stays a factor MIN_MARGIN off both thresholds; s2/s1 is what
    the case states to 10 % (the zero lines move it); the 0.5 spectrum takes 5 squarings and 0.93 takes 8 wherever n > 1."""
    below = set()
    for A, B, r in R.family3_cases():
        Z, (_, _, _, converged, steps, gaps), (_, _, S) = _dense(A, B, r)
        if R.margin(gaps) < R.MIN_MARGIN:
            below.add((A, B, r))
        if min(A, B) > 1:
            assert abs(S[1] / S[0] - r) <= 0.1 * r, (A, B, r, S[1] / S[0])
            assert (converged, steps) == (True, 5 if r == 0.5 else 8), (A, B, r, steps)
        else:
            assert (converged, steps) == (True, 0)
    assert below == R.F3_INFO_NOT_ASSERTED
    assert all(r != 0.5 for _, _, r in below)                       # the 0.5 spectrum is asserted everywhere


def test_close_gap_case_is_what_it_says():
    Z = R.close_gap_case()
    wA, wB, sigma, converged, steps, gaps = R.model(Z, R.F3_BUDGET)
    u, v, S = R.svd_pair(Z)
    assert abs(S[1] / S[0] - R.CLOSE_GAP[1]) < 1e-12 and converged
    assert R.residual(Z, wA, wB) <= R.residual_bound(Z, S[0]) and abs(sigma - S[0]) <= R.sigma_bound(*Z.shape, S[0])
    assert max(np.abs(wA - u).max(), np.abs(wB - v).max()) < 1e-9   # (1.7e-11: governed by the gap, not asserted on the GPU)


@pytest.mark.parametrize("A,B", R.F1_SHAPES)
def test_exact_cases_against_the_model(A, B):
    """Family 1: the model returns the unit vectors and sigma = 1 exactly, converges, and no step comes near a threshold."""
    for i, j, s in R.family1_positions(A, B):
        c = R.exact_case(A, B, i, j, s)
        assert np.count_nonzero(c["Z"]) == min(A, B) and c["Z"][i, j] == float(s)
        assert (np.count_nonzero(c["Z"], axis=0) <= 1).all() and (np.count_nonzero(c["Z"], axis=1) <= 1).all()
        wA, wB, sigma, converged, steps, gaps = R.model(c["Z"], R.F1_BUDGET)
        assert np.array_equal(wA, c["wA"]) and np.array_equal(wB, c["wB"]) and sigma == 1.0, (A, B, i, j, s)
        assert converged and steps == (5 if min(A, B) > 1 else 0) and R.margin(gaps) >= R.MIN_MARGIN, (A, B, i, j, s)


@pytest.mark.parametrize("A,B", R.F2_SHAPES)
def test_tied_cases_against_the_model(A, B):
    """Family 2: rho = 1/2 at every step (margin 5e6), so the whole budget is walked; the first tied index wins on either order."""
    winners = set()
    for budget in R.F2_BUDGETS:
        for lead, tie in R.family2_ties(A, B):
            c = R.exact_case(A, B, lead[0], lead[1], 1, tie=tie)
            wA, wB, sigma, converged, steps, gaps = R.model(c["Z"], budget)
            assert np.array_equal(wA, c["wA"]) and np.array_equal(wB, c["wB"]) and sigma == 1.0
            assert (converged, steps) == (False, min(budget, R.MAX_STEPS)) and R.margin(gaps) >= 1e6
            assert all(0.45 < g < 0.75 for g in gaps) and abs(gaps[-1] - 0.5) < 1e-12
            winners.add((int(np.argmax(wA)) == lead[0]))
    assert winners == {True, False}


def test_exit_cases_take_the_exit_they_name():
    for name, Z, budget, info in R.exit_cases():
        wA, wB, sigma, converged, steps, gaps = R.model(Z, budget)
        assert (int(converged), steps) == info, (name, budget)
        assert R.margin(gaps) >= R.MIN_MARGIN
        if name == "rank_one_in":
            assert gaps == [0.0]                                    # small integers: G_0, its trace and its norm are exact


def test_margin_and_residual_helpers():
    assert R.margin([0.4, 1e-3, 5e-7]) == pytest.approx(5.0) and R.margin([2e-14]) == pytest.approx(5.0)
    assert R.margin([0.0]) == np.inf and R.margin([]) == np.inf
    assert R.margin([0.5 ** k for k in (2, 4, 8, 16, 32)]) > 100
    rng = np.random.default_rng(3)
    Z = rng.normal(size=(6, 9))
    u, v, S = R.svd_pair(Z)
    assert R.residual(Z, u, v) < 1e-14
    v2 = v + 1e-3 * np.eye(9)[0]
    assert 1e-4 < R.residual(Z, u, v2 / np.linalg.norm(v2)) < 1e-2


def test_scaled_inputs_stay_inside_the_double_range():
    """Family 4 scales Z by 2^e: step 1 sums the squares of unscaled Gram entries, so |Z|_F^4 2^(4e) must be a normal double
    with room for the smallest product that matters (2^-53 of it)."""
    for A, B in R.SCALE_SHAPES:
        f = float(np.sum(R.dense_case(A, B, 0.5) ** 2))
        for e in R.SCALE_EXPONENTS:
            assert -1022 + 2 * 53 < np.log2(f * f) + 4 * e < 1023


def test_score_cases_sit_on_both_sides_of_every_gate():
    fused = {c: R.score_is_fused(*c) for c in R.SCORE_CASES}
    assert fused[(64, 128, 64, 0)] and not fused[(64, 128, 65, 0)]
    assert fused[(64, 128, 3, 0)] and not fused[(63, 130, 3, 0)]
    assert fused[(65, 128, 4, 0)] and not fused[(128, 65, 4, 0)]
    assert fused[(2, 7678, 3, 0)] and not fused[(2, 7680, 3, 0)]
    assert fused[(256, 64, 5, 0)] and not fused[(64, 128, 3, 1)]


def test_zero_matrix_in_the_oracle_and_the_model():
    """The oracle divides by a zero norm: all-NaN factors, which is also what the device returns (pinned in the GPU module)."""
    with np.errstate(all="ignore"):
        fa, fb = O.rank1_factors(np.zeros((5, 7)))
    assert np.isnan(fa).all() and np.isnan(fb).all()
    wA, wB, sigma, converged, steps, _ = R.model(np.zeros((5, 7)), 30)
    assert np.isnan(wA).all() and np.isnan(wB).all() and (converged, steps) == (True, 0)


def test_workspace_bytes_to_the_byte():
    """cmtfpls_rank1_workspace_bytes is host arithmetic: the restated layout, byte for byte, on both sides of the chain's limit."""
    from cmtf_pls_amd import _lib
    lib = _lib.load()
    for A, B in R.F3_SHAPES + [(5, 7), (40, 56), (4096, 4096)]:
        assert lib.cmtfpls_rank1_workspace_bytes(A, B) == R.workspace_bytes(A, B), (A, B)
    assert lib.cmtfpls_rank1_workspace_bytes(0, 5) == 0
    assert R.uses_chain(256, 300, 31) and not R.uses_chain(256, 300, 32) and not R.uses_chain(257, 300, 30)
