"""The one-workgroup tPLS fit (loo.hip: loo_tpls_kernel) at the limits it declares and through every branch it takes.

Two instances of the kernel: cmtfpls_fit_small_f64 (1024 threads, one workgroup fits all I rows: the product default for a
float64 block of order 2 or 3 with at most EngineOptions.small_fit_elements elements and no missing values, engine._fit_small)
and cmtfpls_loo_tpls_f64 (256 threads, one workgroup per held-out sample: the "lds" form of validate.get_q2y).  Declared limits:
min(A, B) <= 64, M <= 64, R <= 16 and 150 KB of LDS for the per-workgroup vectors; the fit also keeps the centred X and Y in LDS
when everything fits 158 KB.  Branches inside, n = min(A, B), k = max(A, B), P = A * B, NT the workgroup size:
  - A == 1 (a matrix block, or an order-3 block whose first trailing mode is 1): wB = Z / |Z|;
  - rank-1 inside one wavefront (n <= 8 and k <= 64), otherwise by Gram squaring over the workgroup (A <= B or Z transposed);
  - Z = X x_0 u with row groups added through `part` (P < NT) or one column per thread (P >= NT);
  - centred X and Y in LDS or in the global workspace (fit only).
Which branch a case takes is computed from a mirror of the kernel's rules (`_fit_form`, `_loo_form`), and every case asserts the
branch it is there for, so a change of the rules cannot quietly move a case off its branch.  Fits are compared with the float64
oracle WITHOUT sign alignment of the loadings, and with the regular multi-launch engine; leave-one-out predictions with literal
refits over the oracle."""
import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import oracle as O
from cmtf_pls_amd import tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.validate import get_q2y, loo_predictions

pytestmark = pytest.mark.gpu

_DEV = "cuda:0"
ON = EngineOptions(small_fit=True)
OFF = EngineOptions(small_fit=False)
ELEMENTS = ON.small_fit_elements
MAX_N, MAX_M, MAX_R = 64, 64, 16              # kLooMaxN, kLooMaxM, kLooMaxR
LDS_CAP, XY_CAP = 150 * 1024, 158 * 1024       # the vectors' limit; with the centred X and Y in LDS too
CAP = 100                                      # tPLS.fit's default max_iter


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(_DEV))


# ---- a mirror of the kernel's shape rules ---------------------------------------------------------------------------------------
def _split(shape):
    return (1, shape[1]) if len(shape) == 2 else (shape[1], shape[2])


def _lds_bytes(I, A, B, M, R, nt):
    """loo_lds_bytes (loo.hip): the per-workgroup vectors carved out of the dynamic LDS allocation."""
    n, k, P = min(A, B), max(A, B), A * B
    dbl = (2 * I + P + A + B + 2 * M + 2 * n * n + n + k + M + R * R + R * (A + B) + R * M + R * R + 3 * R + nt)
    return 8 * dbl


def _branches(A, B, nt):
    n, k, P = min(A, B), max(A, B), A * B
    rank1 = "vector" if A == 1 else ("wave" if n <= 8 and k <= 64 else "block")
    return {"rank1": rank1, "rows_a": A <= B, "z": "columns" if P >= nt else "row_groups"}


def _fit_form(I, A, B, M, R):
    """What cmtfpls_fit_small_f64 does with the shape: None when it declines (status 4), else the branches it takes."""
    lds = _lds_bytes(I, A, B, M, R, 1024)
    if min(A, B) > MAX_N or M > MAX_M or R > MAX_R or lds > LDS_CAP:
        return None
    return dict(_branches(A, B, 1024), x_in_lds=lds + 8 * (I * A * B + I * M) <= XY_CAP)


def _loo_form(I, A, B, M, R):
    lds = _lds_bytes(I, A, B, M, R, 256)
    if min(A, B) > MAX_N or M > MAX_M or R > MAX_R or lds > LDS_CAP:
        return None
    return _branches(A, B, 256)


def _last_rows(A, B, M, R, nt):
    """The largest I the vectors of an (I, A, B) problem fit in 150 KB of LDS, from the mirror (not a constant)."""
    I = 2
    while _lds_bytes(I + 1, A, B, M, R, nt) <= LDS_CAP:
        I += 1
    return I


def _normwise(got, want):
    scale = np.nanmax(np.abs(want), axis=0, keepdims=True)
    return float(np.nanmax(np.abs(got - want) / (np.abs(want) + scale)))


def _data(shape, M, latent, seed, error=0.2):
    return O.import_synthetic(shape, M, latent, error=error, seed=seed)[:2]


def _new_rows(x, seed):
    rng = np.random.default_rng(seed)
    return x[:6] + 0.3 * rng.standard_normal(x[:6].shape)


def _check_oracle(m, fit, x, tol=1e-9):
    """Every fitted quantity against the float64 oracle; loadings as they are (no sign alignment), iteration counts exactly."""
    assert m.n_iter_ == fit.n_iter
    for got, want in zip([m.X_factors[0], m.Y_factors[0], m.Y_factors[1]], [fit.T, fit.U, fit.Q]):
        assert got.shape == want.shape and _normwise(got, want) <= tol
    assert len(m.X_factors) == 1 + len(fit.loadings[0])
    for got, want in zip(m.X_factors[1:], fit.loadings[0]):
        assert got.shape == want.shape and _normwise(got, want) <= tol
    assert_allclose(m.coef_, fit.coef, rtol=0, atol=tol * np.abs(fit.coef).max())
    assert_allclose(m.R2X, fit.r2x[0], rtol=0, atol=1e-10)
    assert_allclose(m.R2Y, fit.r2y, rtol=0, atol=1e-10)
    assert_allclose(m.X_mean, fit.x_means[0], rtol=1e-13, atol=1e-15 * np.abs(x).max())
    xn = _new_rows(x, 5)
    assert _normwise(m.transform(xn), O.transform(fit, xn)) <= tol
    want = O.predict(fit, xn)
    assert_allclose(m.predict(xn), want, rtol=1e-7, atol=1e-9 * np.abs(want).max())


def _check_regular(one, reg):
    """test_gpu_round3.test_small_fit_in_one_launch_equals_the_regular_engine's tolerances."""
    assert one.n_iter_ == reg.n_iter_
    for f, g in zip(one.X_factors + one.Y_factors, reg.X_factors + reg.Y_factors):
        assert f.shape == g.shape and _normwise(f, g) <= 1e-10
    assert_allclose(one.R2X, reg.R2X, rtol=0, atol=1e-12)
    assert_allclose(one.R2Y, reg.R2Y, rtol=0, atol=1e-12)
    assert_allclose(one.coef_, reg.coef_, rtol=0, atol=1e-9 * np.abs(reg.coef_).max())
    assert_allclose(one.X_mean, reg.X_mean, rtol=1e-13, atol=1e-15)


# ---- 1. the small fit at every branch against the oracle and the regular engine ---------------------------------------------------
# (shape, M, R, the branches the case is there for); latent rank = R, noise 0.2
FIT_CASES = [
    ((10, 32, 40), 17, 4, dict(rank1="block", rows_a=True, z="columns", x_in_lds=True)),          # P = 1280 >= 1024
    ((16, 9, 64), 1, 5, dict(rank1="block", rows_a=True, z="row_groups", x_in_lds=True)),         # n = 9, k = 64
    ((16, 8, 65), 17, 4, dict(rank1="block", rows_a=True, x_in_lds=True)),                        # n = 8, k = 65: past the wave form
    ((16, 65, 8), 1, 4, dict(rank1="block", rows_a=False, x_in_lds=True)),                        # A > B: Z read transposed
    ((30, 40, 6), 17, 3, dict(rank1="wave", rows_a=False, x_in_lds=True)),                        # wave form, A > B
    ((8, 64, 64), 17, 4, dict(rank1="block", rows_a=True, z="columns", x_in_lds=False)),          # n = 64, 32768 elements
    ((20, 64, 20), 1, 4, dict(rank1="block", rows_a=False, z="columns", x_in_lds=False)),         # A > B, P >= 1024
    ((30, 4, 200), 17, 3, dict(rank1="block", rows_a=True, x_in_lds=False)),                      # k > 64 with n <= 8
    ((30, 200, 4), 1, 3, dict(rank1="block", rows_a=False, x_in_lds=False)),
    ((100, 16, 20), 64, 16, dict(rank1="block", rows_a=True, x_in_lds=False)),                    # M = 64, R = 16
    ((20, 1500), 17, 4, dict(rank1="vector", z="columns", x_in_lds=False)),                       # matrix block, P >= 1024
    ((2, 1), 1, 1, dict(rank1="vector", z="row_groups", x_in_lds=True)),                          # I = 2, P = 1
    ((128, 256), 1, 2, dict(rank1="vector", x_in_lds=False)),                                     # exactly the element budget
    ((40, 1, 800), 17, 4, dict(rank1="vector", z="row_groups", x_in_lds=False)),                  # order 3, A = 1
    ((20, 1, 300), 1, 3, dict(rank1="vector", x_in_lds=True)),                                    # order 3, A = 1, X in LDS
    ((40, 50, 1), 1, 3, dict(rank1="wave", rows_a=False, x_in_lds=True)),                         # order 3, B = 1
]


@pytest.mark.parametrize("shape,M,R,branches", FIT_CASES, ids=[f"{c[0]}-M{c[1]}-R{c[2]}" for c in FIT_CASES])
def test_small_fit_at_each_branch_matches_the_oracle_and_the_regular_engine(shape, M, R, branches):
    I, (A, B) = shape[0], _split(shape)
    form = _fit_form(I, A, B, M, R)
    assert form is not None and {k: form[k] for k in branches} == branches and I * A * B <= ELEMENTS
    x, y = _data(shape, M, R, seed=11)
    fit = O.fit_tpls(x, y, R)
    if len(shape) == 3 and A == 1:
        # parafac's sign rule on (I, 1, B): the case must reach it (wA = -1 on some component), or it could not see the kernel's
        # unsigned vector rule
        assert (fit.loadings[0][0] < 0).any()
    one = tPLS(R, options=ON)
    one.fit(x, y)
    assert one.fit_report_["form"] == "small_fit"
    _check_oracle(one, fit, x)
    reg = tPLS(R, options=OFF)
    reg.fit(x, y)
    assert reg.fit_report_["form"] == "regular"
    _check_regular(one, reg)
    _check_oracle(reg, fit, x)


# ---- 2. the iteration cap ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,M,R", [((16, 9, 64), 17, 3), ((20, 1500), 3, 2), ((200, 10, 8), 4, 3), ((20, 1, 300), 3, 2)])
@pytest.mark.parametrize("tol,max_iter", [(1e-8, 2), (1e-8, 3), (0.0, 7)])
def test_small_fit_stops_at_the_iteration_cap_like_the_oracle(shape, M, R, tol, max_iter):
    """Every component runs max_iter iterations (tol = 0 never converges: |du| < 0 is false) and the factors are the oracle's after
    the same number.  (M > 1: with one response u = +-Y_c, and the second iteration always converges.)"""
    x, y = _data(shape, M, R, seed=12)
    fit = O.fit_tpls(x, y, R, tol=tol, max_iter=max_iter)
    assert fit.n_iter == [max_iter] * R
    one = tPLS(R, options=ON)
    one.fit(x, y, tol=tol, max_iter=max_iter)
    assert one.fit_report_["form"] == "small_fit"
    _check_oracle(one, fit, x)
    reg = tPLS(R, options=OFF)
    reg.fit(x, y, tol=tol, max_iter=max_iter)
    _check_regular(one, reg)


# ---- 3. declines: one step past each limit, directly and end to end ------------------------------------------------------------------
# name -> ((I, A, B, M, R) one step inside, the same one step past); the LDS rows from the mirror
_LDS_ROWS = _last_rows(1, 3, 1, 2, 1024)
DECLINES = {
    "n": ((7, 64, 65, 2, 2), (7, 65, 65, 2, 2)),
    "M": ((40, 8, 8, 64, 3), (40, 8, 8, 65, 3)),
    "R": ((40, 8, 8, 3, 16), (40, 8, 8, 3, 17)),
    "lds": ((_LDS_ROWS, 1, 3, 1, 2), (_LDS_ROWS + 1, 1, 3, 1, 2)),
}


def _shape(I, A, B):
    return (I, B) if A == 1 else (I, A, B)


@pytest.mark.parametrize("limit", sorted(DECLINES))
def test_fit_small_kernel_declines_one_step_past_each_limit(be, limit):
    inside, past = DECLINES[limit]
    assert _fit_form(*inside) is not None and _fit_form(*past) is None
    assert _lds_bytes(*past, 1024) <= LDS_CAP or limit == "lds"            # past the named limit only
    for (I, A, B, M, R), accepted in ((inside, True), (past, False)):
        x, y = _data(_shape(I, A, B), M, min(R, 4), seed=13)
        X2 = torch.from_numpy(np.ascontiguousarray(x.reshape(I, -1))).to(_DEV)
        Y2 = torch.from_numpy(np.ascontiguousarray(y.reshape(I, -1))).to(_DEV)
        out = be.fit_small(X2, Y2, A, B, R, 1e-8, CAP)
        assert (out is not None) == accepted
        if accepted:
            assert len(out["n_iter"]) == R and torch.isfinite(out["T"]).all() and out["T"].shape == (I, R)


E2E_DECLINES = [(*DECLINES[k][0], True) for k in sorted(DECLINES)] + [(*DECLINES[k][1], False) for k in sorted(DECLINES)] + [
    (99, 1, 331, 1, 2, False)]                                             # 32769 elements: the element budget, not the kernel


@pytest.mark.parametrize("I,A,B,M,R,small", E2E_DECLINES, ids=[f"{c[:5]}-{'small' if c[5] else 'regular'}" for c in E2E_DECLINES])
def test_estimator_takes_the_regular_engine_past_each_limit(I, A, B, M, R, small):
    shape = _shape(I, A, B)
    assert (_fit_form(I, A, B, M, R) is not None and I * A * B <= ELEMENTS) == small
    if not small and (I, A, B) == (99, 1, 331):
        assert _fit_form(I, A, B, M, R) is not None and I * A * B == ELEMENTS + 1
    x, y = _data(shape, M, R, seed=14)
    m = tPLS(R, options=ON)
    m.fit(x, y)
    assert m.fit_report_["form"] == ("small_fit" if small else "regular")
    _check_oracle(m, O.fit_tpls(x, y, R), x)


def _with_inf(kind):
    x, y = _data((30, 9, 8), 3, 3, seed=15)
    if kind == "x+inf":
        x[3, 2, 1] = np.inf
    elif kind == "x-inf":
        x[3, 2, 1] = -np.inf
    elif kind == "x+-inf":                                                  # one column: its sum is NaN, not inf
        x[3, 2, 1], x[7, 2, 1] = np.inf, -np.inf
    else:
        y[5, 1] = np.inf
    return x, y


@pytest.mark.parametrize("kind", ["x+inf", "x-inf", "x+-inf", "y+inf"])
def test_non_finite_input_is_flagged_and_refitted_by_the_regular_engine(be, kind):
    x, y = _with_inf(kind)
    X2 = torch.from_numpy(np.ascontiguousarray(x.reshape(30, -1))).to(_DEV)
    assert _fit_form(30, 9, 8, 3, 3) is not None
    assert be.fit_small(X2, torch.from_numpy(y).to(_DEV), 9, 8, 3, 1e-8, CAP) is None
    one = tPLS(3, options=ON)
    one.fit(x, y)
    assert one.fit_report_["form"] == "regular"
    reg = tPLS(3, options=OFF)
    reg.fit(x, y)
    for f, g in zip(one.X_factors + one.Y_factors + [one.coef_, one.R2X, one.R2Y, one.X_mean],
                    reg.X_factors + reg.Y_factors + [reg.coef_, reg.R2X, reg.R2Y, reg.X_mean]):
        assert_allclose(f, g, rtol=1e-13, atol=0, equal_nan=True)
    assert one.n_iter_ == reg.n_iter_
    # nothing left behind: the same estimator then fits finite data in one launch
    xc, yc = _data((30, 9, 8), 3, 3, seed=16)
    one.fit(xc, yc)
    assert one.fit_report_["form"] == "small_fit"
    _check_oracle(one, O.fit_tpls(xc, yc, 3), xc)


# ---- 4. determinism: one workgroup, fixed summation order ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape,M,R", [((200, 10, 8), 4, 3), ((100, 16, 20), 64, 16), ((20, 1500), 17, 4), ((10, 32, 40), 1, 4),
                                       ((40, 1, 800), 3, 4)])
def test_small_fit_is_bitwise_reproducible(shape, M, R):
    x, y = _data(shape, M, R, seed=17)
    a, b = tPLS(R, options=ON), tPLS(R, options=ON)
    a.fit(x, y)
    b.fit(x, y)
    assert a.fit_report_["form"] == b.fit_report_["form"] == "small_fit"
    assert a.n_iter_ == b.n_iter_
    for f, g in zip(a.X_factors + a.Y_factors + [a.coef_, a.R2X, a.R2Y], b.X_factors + b.Y_factors + [b.coef_, b.R2X, b.R2Y]):
        assert np.array_equal(f, g)


# ---- 5. the leave-one-out form at its limits -----------------------------------------------------------------------------------------
# (shape, M, R, the branches the case is there for); every fold refitted over the oracle
LOO_CASES = [
    ((40, 64, 64), 2, 3, dict(rank1="block", rows_a=True, z="columns")),          # n = 64
    ((24, 12, 30), 64, 16, dict(rank1="block", rows_a=True, z="columns")),        # M = 64, R = 16, P >= 256
    ((24, 30, 12), 64, 16, dict(rank1="block", rows_a=False, z="columns")),
    ((30, 4, 100), 3, 3, dict(rank1="block", rows_a=True, z="columns")),          # k > 64 with n <= 8
    ((30, 100, 4), 1, 2, dict(rank1="block", rows_a=False, z="columns")),
    ((25, 1, 300), 2, 3, dict(rank1="vector", z="columns")),                      # order 3, A = 1
    ((3, 5, 6), 2, 1, dict(rank1="wave", rows_a=True, z="row_groups")),           # two training rows per fold
]


@pytest.mark.parametrize("shape,M,R,branches", LOO_CASES, ids=[f"{c[0]}-M{c[1]}-R{c[2]}" for c in LOO_CASES])
def test_loo_form_at_its_limits_matches_literal_refits(shape, M, R, branches):
    """test_gpu_round2.test_loo_all_folds_in_one_launch_matches_literal_refits's tolerances: 1e-7 per prediction, 1e-8 in Q2Y."""
    I, (A, B) = shape[0], _split(shape)
    form = _loo_form(I, A, B, M, R)
    assert form is not None and {k: form[k] for k in branches} == branches
    x, y = _data(shape, M, R, seed=21, error=0.3)
    m = tPLS(R, options=OFF)
    m.fit(x, y)
    pred = loo_predictions(m)
    assert pred is not None and pred.shape == y.shape
    assert "cmtfpls_loo_tpls_f64" in m.q2y_report_["form"]
    want = np.zeros_like(y)
    for i in range(I):
        keep = np.arange(I) != i
        want[i] = O.predict(O.fit_tpls(x[keep], y[keep], R), x[i:i + 1]).reshape(want[i].shape)
    assert_allclose(pred, want, rtol=1e-7, atol=1e-7 * np.abs(y).max())
    q_want = 1 - ((want - y) ** 2).sum() / (y ** 2).sum()
    assert abs(get_q2y(m) - q_want) < 1e-8
    assert "cmtfpls_loo_tpls_f64" in m.q2y_report_["form"]


_LOO_LDS_ROWS = _last_rows(1, 3, 1, 2, 256)
LOO_DECLINES = {
    "n": ((6, 64, 65, 2, 2), (6, 65, 65, 2, 2)),
    "M": ((10, 8, 8, 64, 2), (10, 8, 8, 65, 2)),
    "R": ((20, 8, 8, 2, 16), (20, 8, 8, 2, 17)),
    "lds": ((_LOO_LDS_ROWS, 1, 3, 1, 2), (_LOO_LDS_ROWS + 1, 1, 3, 1, 2)),
}


@pytest.mark.parametrize("limit", sorted(LOO_DECLINES))
def test_loo_form_declines_one_step_past_each_limit(be, limit):
    """Past the limit: status 4 and be.loo_tpls(forms=("lds",)) is None.  One step inside, probed without a workspace: status 2
    (the shape is accepted, only the workspace is missing) -- the inside shapes that fit a test's time run end to end above."""
    from cmtf_pls_amd.backend import _ptr
    inside, past = LOO_DECLINES[limit]
    assert _loo_form(*inside) is not None and _loo_form(*past) is None
    for (I, A, B, M, R), accepted in ((inside, True), (past, False)):
        x, y = _data(_shape(I, A, B), M, min(R, 4), seed=22)
        X2 = torch.from_numpy(np.ascontiguousarray(x.reshape(I, -1))).to(_DEV)
        Y2 = torch.from_numpy(np.ascontiguousarray(y.reshape(I, -1))).to(_DEV)
        cx, cy = X2.sum(dim=0), Y2.sum(dim=0)
        Yp = torch.empty(I, M, dtype=torch.float64, device=_DEV)
        it = torch.zeros(I, R, dtype=torch.int32, device=_DEV)
        rc = be.lib.cmtfpls_loo_tpls_f64(_ptr(X2), _ptr(Y2), _ptr(cx), _ptr(cy), I, A, B, M, R, 1e-8, CAP, 0, 1, _ptr(Yp), _ptr(it),
                                         None, 0, be._stream())
        be.lib.cmtfpls_clear_error()
        assert rc == (2 if accepted else 4)
        if not accepted:
            assert be.loo_tpls(X2, Y2, A, B, R, 1e-8, CAP, forms=("lds",)) is None
