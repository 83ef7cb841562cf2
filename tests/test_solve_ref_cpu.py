"""tests/solve_ref.py itself, no GPU: the long-double restatement of normal_solve against the plain-float restatement of the
one-thread form (small_algebra_ref.fold_normal_solve) and against lstsq; the backward-error bound accepts the restatement's
own solution and rejects three wrong solves; the row-solve restatement against np.linalg.solve; and the conditions that the
builders promise (pivot margins, the 2^53 cap, exactness of the Hadamard construction) for every case of
tests/test_gpu_solve_limits.py."""
import numpy as np
import pytest

import small_algebra_ref as SA
import solve_ref as S

LD = np.longdouble


def ratio(ref, b):
    r, bound = S.normal_solve_bound(ref, b)
    assert np.all(bound > 0) and np.all(np.isfinite(r))
    return float((r / bound).max(initial=0.0))


# ---- agreement with the references the suite already has ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 7, 16, 33, 64])
def test_agrees_with_the_one_thread_restatement(k):
    """The inputs of test_fold_regress_cpu.py::test_host_build_equals_the_restatement: same drop set, and the one-thread form's
    float64 result passes the bound (it rounds the equilibration as G (d_i d_j): two products, as the bound counts)."""
    rng = np.random.default_rng(k)
    T = rng.normal(size=(200, k)) * 10.0 ** rng.uniform(-8, 0, size=k)[None, :]
    if k >= 7:
        T[:, 2] = 0.0
        T[:, 4] = 2.0 * T[:, 1]
    G, g = T.T @ T, T.T @ rng.normal(size=200)
    fold_b, fold_dropped = SA.fold_normal_solve(G, g)
    ref = S.normal_solve(G, g)
    assert ref.dropped == fold_dropped == ([2, 4] if k >= 7 else [])
    assert np.all(ref.b[ref.dropped] == 0)
    assert ratio(ref, fold_b) <= 1.0


@pytest.mark.parametrize("k", [1, 5, 40, 100])
def test_agrees_with_lstsq_without_drops(k):
    rng = np.random.default_rng(100 + k)
    T, u = rng.normal(size=(3 * k + 5, k)), rng.normal(size=3 * k + 5)
    ref = S.normal_solve(T.T @ T, T.T @ u)
    assert ref.dropped == [] and np.all(ref.pivots > 0.01)
    np.testing.assert_allclose(ref.b.astype(np.float64), np.linalg.lstsq(T, u, rcond=None)[0], rtol=1e-10, atol=0)


def test_non_finite_diagonal_gives_the_one_thread_pattern():
    want, dropped = SA.fold_normal_solve(S.NONFINITE_G, S.NONFINITE_g)
    ref = S.normal_solve(S.NONFINITE_G, S.NONFINITE_g)
    assert ref.dropped == dropped == [1]
    assert np.isnan(want[0]) and want[1] == 0.0
    assert np.array_equal(ref.b.astype(np.float64), want, equal_nan=True)
    k, (c0, c1), diag = S.NONFINITE_EMBED
    big = S.normal_solve(*S.embed(S.NONFINITE_G, S.NONFINITE_g, list((c0, c1)), k, diag)).b.astype(np.float64)
    # row c1 of L is NaN from column c0 on and multiplies its own zero coefficient: 0 * NaN = NaN reaches every coefficient before
    # c1 in the backward solve (the zeros of the identity-like rows times a NaN coefficient), none after it
    assert np.all(np.isnan(big[:c1])) and big[c1] == 0.0 and np.all(big[c1 + 1:] == 1.0)


# ---- the bound has teeth ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[64, 300])
def deficient(request):
    k = request.param
    return S.rounding_normal(k, zero=S.rounding_zero_columns(k), shrunk=S.rounding_shrunk_column(k))


def test_bound_accepts_the_restatement(deficient):
    G, g, ref = deficient
    r = ratio(ref, ref.b.astype(np.float64))
    print(f"k = {ref.k}: restatement rounded to float64, error / bound {r:.2e}")
    assert r <= 1.0
    for k in (1, 2, 3):
        _, _, small = S.rounding_case(k, "plain")
        assert ratio(small, small.b.astype(np.float64)) <= 1.0


@pytest.mark.parametrize("k", [64, 300])
def test_bound_rejects_an_update_loop_that_stops_before_the_diagonal(k):
    """With the zero columns and without the shrunk one: every pivot stays at its first value, 1 or 0, the drop set is the right one
    and the wrong solution is finite.  (With the shrunk column kept at pivot 1 the factor overflows to NaN, which the GPU tests'
    `b finite` rejects before any bound.)"""
    G, g, ref = S.rounding_normal(k, zero=S.rounding_zero_columns(k))
    wrong = S.normal_solve(G, g, update_diagonal=False)
    assert wrong.dropped == ref.dropped and np.all(np.isfinite(wrong.b))
    r = ratio(ref, wrong.b.astype(np.float64))
    print(f"k = {ref.k}: update loop to j < i, error / bound {r:.2e}")
    assert r > 1.0
    G, g, ref = S.rounding_normal(k, zero=S.rounding_zero_columns(k), shrunk=S.rounding_shrunk_column(k))
    assert not np.all(np.isfinite(S.normal_solve(G, g, update_diagonal=False).b))


def test_bound_rejects_a_dropped_column_left_in_place(deficient):
    """The shrunk column: dropped with a sub-column of order 1.  (A zero column's sub-column is zero already.)"""
    G, g, ref = deficient
    (c,) = S.rounding_shrunk_column(ref.k)
    wrong = S.normal_solve(G, g, leave_dropped=c)
    assert np.all(np.isfinite(wrong.b)) and set(wrong.dropped) > set(ref.dropped)   # its entries of order 1 sink later pivots
    r = ratio(ref, wrong.b.astype(np.float64))
    print(f"k = {ref.k}: dropped column {c} not zeroed, error / bound {r:.2e}")
    assert r > 1.0


def test_bound_rejects_one_coefficient_off_by_1e_minus_9(deficient):
    G, g, ref = deficient
    b = ref.b.astype(np.float64)
    j = ref.kept[np.argmax(np.abs((ref.b / np.where(ref.d > 0, ref.d, 1))[ref.kept]))]
    b[j] *= 1.0 + 1e-9
    r = ratio(ref, b)
    print(f"k = {ref.k}: coefficient {j} times 1 + 1e-9, error / bound {r:.2e}")
    assert r > 1.0


# ---- unit_upper_solve_rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_shift", [True, False])
@pytest.mark.parametrize("R", S.UPPER_R)
def test_row_solve_matches_numpy(R, with_shift):
    M, Um, shift = S.rounding_upper(257, R)
    sh = shift if with_shift else None
    T, err = S.unit_upper_solve_rows(M, Um, sh)
    want = np.linalg.solve((np.eye(R) + np.triu(Um, 1)).T, (M - (shift if with_shift else 0.0)).T).T
    assert np.all(err > 0) and np.all(np.abs(T.astype(np.float64) - want) <= err)
    masked = Um.copy()
    masked[np.tril_indices(R)] = np.nan
    T2, err2 = S.unit_upper_solve_rows(M, masked, sh)
    assert np.array_equal(T, T2) and np.array_equal(err, err2)


def test_row_solve_bound_rejects_a_dropped_term():
    M, Um, shift = S.rounding_upper(257, 64)
    T, err = S.unit_upper_solve_rows(M, Um, shift)
    wrong = Um.copy()
    wrong[62, 63] = 0.0
    T2, _ = S.unit_upper_solve_rows(M, wrong, shift)
    assert np.all(np.abs((T2 - T)[:, 63].astype(np.float64)) > 1000 * err[:, 63])


# ---- the builders' promises, for every case of the GPU file ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", S.NORMAL_K)
def test_exact_inputs_are_exact(k):
    I = S.exact_rows(k)
    for variant in S.EXACT_VARIANTS:
        G, g, ref = S.exact_normal(k, I, variant)
        zeros, dups = S.special_columns(k, variant)
        assert ref.dropped == sorted(set(zeros) | set(dups))          # (asserted by the builder too)
        assert all(s < c and s not in zeros and s not in dups for c, s in dups.items())
        K = ref.kept
        assert np.array_equal(ref.Ahat[np.ix_(K, K)], np.eye(len(K), dtype=LD))       # bit for bit
        assert np.all((ref.Ahat == 0) | (ref.Ahat == 1))
        assert np.all(ref.Ahat[list(dups), list(dups.values())] == 1)
        d = ref.d.astype(np.float64)
        assert np.all(d == ref.d) and np.all((np.frexp(d)[0] == 0.5) | (d == 0))       # powers of two
        assert np.all((ref.pivots == 1) | (ref.pivots == 0))
        want = np.zeros(k, dtype=LD)
        want[K] = g[K].astype(LD) * ref.d[K] * ref.d[K]
        assert np.array_equal(ref.b, want) and np.array_equal(ref.b.astype(np.float64), ref.b)
        ints = g[K] * d[K] * np.sqrt(I)                                               # g 2^-e: T^T u of a +-1 matrix
        assert np.all(ints == np.round(ints)) and np.all(np.abs(ints) <= 8 * I)
        S.assert_pivot_margins(ref)
    if k >= 513:                                                       # a copy and its source in different 256-row passes
        _, dups = S.special_columns(k, "dups")
        assert any(c // 256 != s // 256 for c, s in dups.items())


@pytest.mark.parametrize("k", S.NORMAL_K)
def test_rounding_inputs_keep_their_pivots_away_from_the_threshold(k):
    for variant in S.ROUNDING_VARIANTS:
        G, g, ref = S.rounding_case(k, variant)                        # asserts the margins and the drop set
        S.assert_pivot_margins(ref)
        assert np.array_equal(G, G.T)
        assert len(ref.dropped) == (0 if variant == "plain" else len(S.rounding_zero_columns(k)) + len(S.rounding_shrunk_column(k)))


def test_the_other_normal_cases_build():
    ks, kb, pos = S.BOTH_FORMS
    assert 40 <= ks <= 64 and len(pos) == ks and pos[0] > 0 and pos[-1] >= 256 and pos[-1] < kb
    G, g, ref = S.rounding_case(ks, "deficient")
    big = S.normal_solve(*S.embed(G, g, list(pos), kb))
    S.assert_pivot_margins(big)
    assert [c for c in big.dropped if c in pos] == [pos[c] for c in ref.dropped]
    assert sorted(set(big.dropped) | set(big.kept)) == list(range(kb)) and len(big.kept) == len(ref.kept)
    for R, a in S.ABI_COLUMN_CASES:
        assert a + 1 < R and (a + 1 <= S.MAX_K_LDS) == (R == 8)
        S.rounding_case(a + 1, "plain")


@pytest.mark.parametrize("I,R", S.UPPER_CASES)
def test_exact_row_solve_inputs_stay_below_2_53(I, R):
    M, Um, shift = S.exact_upper(I, R)                                 # asserts the cap and one non-zero per column
    assert np.all(M == np.round(M)) and np.all(Um == np.round(Um)) and np.all(shift == np.round(shift))
    if R > 1:
        assert np.all((np.triu(Um, 1) != 0).sum(axis=0)[1:] == 1) and np.any(np.tril(Um) != 0)
    T, _ = S.unit_upper_solve_rows(M, Um, shift)
    assert np.array_equal(T.astype(np.float64), T)
    assert set(S.UPPER_NAN_ROWS[I]) == {0, min(255, I - 1), I - 1}
