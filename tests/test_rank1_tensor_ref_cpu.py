"""The host reference of the tensor rank-1 extraction (tests/rank1_tensor_ref.py) against the oracle it restates, and the
conditions its case table has to meet before the kernel is measured with it (tests/test_gpu_rank1_tensor_limits.py).  No GPU."""
import numpy as np
import pytest

import oracle as O
import rank1_tensor_ref as R
from oracle import nipals_oracle as NO

_seen = {}


def _run(case):
    """Z, the oracle's own init, and the float64 / long-double ALS from it (computed once per case)."""
    if case.name not in _seen:
        Z = R.make_z(case.dims, case.kind, case.seed)
        init = [NO._leading_left_singular(R.unfold(Z, m)) for m in range(Z.ndim)]
        f64, s64, margin = R.als(Z, init, case.tol, dtype=np.float64)
        d_case, fld, sld, _ = R.spread(Z, init, case.tol)
        _seen[case.name] = (Z, init, f64, s64, margin, d_case, fld, sld)
    return _seen[case.name]


def test_unfold_is_the_oracles_unfolding_element_by_element():
    """unfold(Z, m)[a, c] = Z[.., a, ..] with c the C-order index over the remaining modes, the last of them fastest -- stated
    with explicit index arithmetic, the way unfold_kernel decodes it."""
    Z = np.arange(2 * 3 * 4 * 5, dtype=np.float64).reshape(2, 3, 4, 5)
    for m in range(4):
        U = R.unfold(Z, m)
        assert np.array_equal(U, NO._unfold(Z, m))
        rest = [i for i in range(4) if i != m]
        for a in range(Z.shape[m]):
            for c in range(U.shape[1]):
                idx, r = [0] * 4, c
                idx[m] = a
                for i in reversed(rest):
                    idx[i], r = r % Z.shape[i], r // Z.shape[i]
                assert U[a, c] == Z[tuple(idx)]


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_float64_als_from_the_oracles_init_is_the_oracle_bit_for_bit(case):
    Z, init, f64, s64, margin, d_case, fld, sld = _run(case)
    want = O.rank1_factors(Z, case.tol)
    for m, (g, w) in enumerate(zip(f64, want)):
        assert g.dtype == np.float64 and np.array_equal(g, w), (m, np.abs(g - w).max())
    # the sweep count: the oracle does not return it, so cap it -- at s64 sweeps nothing changes, at s64 - 1 it has to
    capped = O.rank1_factors(Z, case.tol, n_iter_max=s64)
    assert all(np.array_equal(a, b) for a, b in zip(capped, want))
    if s64 > 2:
        short = O.rank1_factors(Z, case.tol, n_iter_max=s64 - 1)
        assert not all(np.array_equal(a, b) for a, b in zip(short, want))
    assert sld == s64


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_every_case_stops_by_its_data_and_not_by_rounding(case):
    """A condition on the table: the closest stop decision is 1e-11 or more away from falling the other way.  A case that misses
    it gets another seed in rank1_tensor_ref; nothing here is relaxed."""
    Z, init, f64, s64, margin, d_case, fld, sld = _run(case)
    print(f"{case.name}: sweeps {s64}, stop margin {margin:.3g}, d_case {d_case:.3g}")
    assert margin >= R.MIN_MARGIN, (case.name, margin)
    assert d_case < 1e-13, (case.name, d_case)          # float64 and long double went the same way throughout


def test_the_stop_rule_cases_are_what_they_say():
    by = {c.name: c for c in R.CASES}
    assert _run(by["9x8x7-noise-tol0"])[3] == R.MAX_SWEEPS
    assert _run(by["9x8x7-close-tol0.01"])[3] == 2
    assert _run(by["1024x3x2-noise"])[3] == R.MAX_SWEEPS            # a capped run at tol = 1e-8 too
    assert max(len(c.dims) for c in R.CASES) == 7 and {len(c.dims) for c in R.CASES} == {3, 4, 5, 6, 7}


def test_a_zero_tensor_gives_nan_factors_after_the_full_hundred_sweeps():
    """0 / 0 at the first update; NaN < tol is false, so the stop rule never fires (what the kernel has to do too)."""
    Z = np.zeros((4, 3, 2))
    init = [np.eye(d)[0] for d in Z.shape]
    fac, sweeps, _ = R.als(Z, init, 1e-8, dtype=np.float64)
    assert sweeps == R.MAX_SWEEPS and all(np.isnan(f).all() for f in fac)
