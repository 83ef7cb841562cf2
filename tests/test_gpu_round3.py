"""Round-3 items on the GPU: limits lifted / validated up front (VERDICT r2 "Next" #4, ADVICE medium), the inner
regression beyond 64 components, rank-deficient score matrices (ADVICE low), the LDS boundary of project_rows (ADVICE
low), float64 X_reconstructed (ADVICE low)."""
import numpy as np
import pytest

from cmtf_pls_amd.engine import default_options
import torch
from numpy.testing import assert_allclose

import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    import cmtf_pls_amd
    return cmtf_pls_amd


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


# ---- inner regression with more than 64 components (tpls.py:110-112 has no limit) -------------------------------------
@pytest.mark.parametrize("k", [65, 100, 257])
def test_normal_solve_beyond_64_columns_matches_lstsq(be, k):
    rng = np.random.default_rng(k)
    T = rng.normal(size=(3 * k, k)) * np.logspace(0, -6, k)[None, :]
    T[:, 1:] += 0.2 * T[:, :1] * np.logspace(0, -6, k)[None, 1:]
    u = rng.normal(size=3 * k)
    want = np.linalg.lstsq(T, u, rcond=-1)[0]
    got = be.normal_solve(_dev(T.T @ T), _dev(T.T @ u)).cpu().numpy()
    assert_allclose(got, want, rtol=1e-6, atol=0)


def test_normal_solve_big_and_small_forms_agree_and_drop_the_same_columns(be):
    """The workspace form (k > 64) applies the pivot rule of the LDS form: embed a 40-column problem with a zero and a
    duplicated column into 70 columns (the extra 30 are zero) and compare with the 40-column solve."""
    rng = np.random.default_rng(5)
    T = rng.normal(size=(300, 40))
    T[:, 7] = 0.0
    T[:, 31] = -1.5 * T[:, 3]
    u = rng.normal(size=300)
    small = be.normal_solve(_dev(T.T @ T), _dev(T.T @ u)).cpu().numpy()
    Tb = np.concatenate([T, np.zeros((300, 30))], axis=1)
    big = be.normal_solve(_dev(Tb.T @ Tb), _dev(Tb.T @ u)).cpu().numpy()
    assert_allclose(big[:40], small, rtol=1e-12, atol=1e-14)
    assert np.all(big[40:] == 0.0) and big[7] == 0.0 and big[31] == 0.0


def test_rank_deficient_scores_fitted_values_equal_the_minimum_norm_solution(be):
    """a zero or exactly dependent score column gets coefficient 0 here, while lstsq(T, u, rcond=-1)
    (tpls.py:110-112) returns the minimum-norm solution, which spreads the coefficient over the dependent columns.
    The two differ in `coef_` but NOT in what the fit uses it for: T b -- the Y deflation (tpls.py:113) and every
    prediction (tpls.py:143) -- is the same projection of u onto span(T)."""
    rng = np.random.default_rng(9)
    T = rng.normal(size=(400, 6))
    T[:, 4] = 0.7 * T[:, 1]
    T[:, 5] = 0.0
    u = rng.normal(size=400)
    b = be.normal_solve(_dev(T.T @ T), _dev(T.T @ u)).cpu().numpy()
    b_min_norm = np.linalg.lstsq(T, u, rcond=None)[0]
    assert_allclose(T @ b, T @ b_min_norm, rtol=1e-10, atol=1e-12)
    assert b[4] == 0.0 and b[5] == 0.0 and abs(b_min_norm[4]) > 1e-3


@pytest.mark.parametrize("algorithm", ["direct", "xcov"])
def test_fit_with_more_than_64_components(api, algorithm):
    """n_components = 70 on a (160, 12, 10) tensor (rank 119 after centring), float64: the fit used to die at
    component 65 inside normal_solve.  Compared with the oracle on what is stable under the loop's
    own conditioning: R2X / R2Y, the fitted responses, and the leading components' factors."""
    rng = np.random.default_rng(70)
    x = rng.normal(size=(160, 12, 10))
    y = rng.normal(size=(160, 3))
    R = 70
    m = api.tPLS(R, algorithm=algorithm)
    m.fit(x, y)
    fit = O.fit_tpls(x, y, R)
    assert m.coef_.shape == (R, R) and np.all(np.isfinite(m.coef_))
    assert_allclose(m.R2X, fit.r2x[0], rtol=1e-6, atol=1e-8)
    assert_allclose(m.R2Y, fit.r2y, rtol=1e-6, atol=1e-8)
    assert_allclose(m.X_factors[0][:, :5], fit.T[:, :5], rtol=1e-6, atol=1e-7 * np.abs(fit.T[:, :5]).max())
    want = O.predict(fit, x)                                       # 70 non-orthogonal score columns through two different solvers
    assert_allclose(m.predict(x), want, rtol=0, atol=1e-5 * np.abs(want).max())
    assert_allclose(m.transform(x), m.X_factors[0], rtol=1e-6, atol=1e-8)       # tests/test_tpls.py:145-155 at R = 70


# ---- limits are refused BEFORE the first sweep ------------------------------------------------------------------------
def test_limits_raise_before_any_sweep(api, monkeypatch):
    from cmtf_pls_amd import engine
    calls = []
    from cmtf_pls_amd.backend import HipBackend
    orig = HipBackend.colstats
    monkeypatch.setattr(HipBackend, "colstats", lambda self, X2: (calls.append(1), orig(self, X2))[1])
    x = torch.zeros(4, 2, 2, 2, 2, 2, 2, 2, 2, device="cuda:0")   # order 9
    with pytest.raises(NotImplementedError, match="order > 8"):
        api.tPLS(1).fit(x, torch.zeros(4, 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="n_components"):
        api.tPLS(engine.MAX_COMPONENTS + 1).fit(torch.zeros(8, 4, 4, device="cuda:0"), torch.zeros(8, 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="rank-1 kernel"):
        api.tPLS(1).fit(torch.zeros(2, engine.MAX_RANK1_SIDE + 1, engine.MAX_RANK1_SIDE + 2, device="cuda:0", dtype=torch.float32),
                        torch.zeros(2, 1, dtype=torch.float64))
    assert calls == []                                            # not one statistics pass was launched


def test_fit_with_a_trailing_side_beyond_1024(api):
    """min(J, K) = 1100 (the rank-1 kernel's limit was 1024 in round 2): a short fit against the oracle."""
    x, y, _ = O.import_synthetic((24, 1100, 1150), 3, 3, error=0.1, seed=3)
    m = api.tPLS(2)
    m.fit(x, y, max_iter=5)
    fit = O.fit_tpls(x, y, 2, max_iter=5)                          # (two 1100 x 1150 LAPACK SVDs per oracle iteration)
    assert_allclose(m.X_factors[0], fit.T, rtol=1e-7, atol=1e-7 * np.abs(fit.T).max())
    s = np.sign(np.sum(m.X_factors[1] * fit.loadings[0][0], axis=0))
    assert_allclose(m.X_factors[1] * s, fit.loadings[0][0], rtol=0, atol=1e-8)
    assert_allclose(m.X_factors[2] * s, fit.loadings[0][1], rtol=0, atol=1e-8)
    assert_allclose(m.R2X, fit.r2x[0], rtol=1e-7)


# ---- project_rows at its LDS boundary -------------------------------------------------------------------
def test_nan_transform_with_64kb_of_loadings_in_lds(api):
    """R = 32 at 128 x 128 f32: the loadings take exactly 65536 bytes of dynamic LDS next to 64 static bytes -- above
    the default limit, so the launch must raise the kernel's dynamic-LDS attribute (or decline), not fail."""
    x, y, _ = O.import_synthetic((96, 128, 128), 4, 6, error=0.3, seed=11)
    x, y = _f32(x), _f32(y)
    m = api.tPLS(32, dtype="float32")
    m.fit(x, y, max_iter=15)
    xt = x[:40].copy()
    xt[np.random.default_rng(1).random(xt.shape) < 0.2] = np.nan
    got = m.transform(xt)
    fit = O.OracleFit(coupled=False, n_components=32, block_shapes=[x.shape], y_shape=y.shape, T=m.X_factors[0],
                      loadings=[[m.X_factors[1], m.X_factors[2]]], U=m.Y_factors[0], Q=m.Y_factors[1], coef=m.coef_,
                      r2x=[m.R2X], r2y=m.R2Y, x_means=[m.X_mean], y_mean=m.Y_mean, has_miss=[False])
    want = O.transform(fit, xt)                                   # the reference's masked sequence with the SAME factors
    scale = np.abs(want).max(axis=0, keepdims=True)
    assert (np.abs(got - want) / (np.abs(want) + scale)).max() <= 1e-5


# ---- X_reconstructed returns the exact float64 reconstruction ---------------------------------------------
def test_x_reconstructed_host_array_is_float64_exact(api):
    x, y, _ = O.import_synthetic((64, 24, 16), 3, 4, error=0.1, seed=2)
    x, y = _f32(x), _f32(y)
    m = api.tPLS(3, dtype="float32")
    m.fit(x, y)
    want = np.einsum("ir,jr,kr->ijk", *m.X_factors) + m.X_mean     # util.py:18-20 + tpls.py:188-189 in float64
    got = m.X_reconstructed()
    assert got.dtype == np.float64
    assert_allclose(got, want, rtol=1e-13, atol=1e-13 * np.abs(want).max())      # f32 rounding would show as 6e-8
    assert_allclose(m.X_reconstructed(rows=slice(10, 20)), want[10:20], rtol=1e-13, atol=1e-13 * np.abs(want).max())
    dev = m.X_reconstructed(device=True)                          # the device form stays in the storage type
    assert dev.dtype == torch.float32
    assert_allclose(dev.double().cpu().numpy(), want, rtol=2e-7, atol=2e-7 * np.abs(want).max())


# ---- one-read NaN transform for long rows and for coupled blocks (VERDICT r2 "Next" #5) ------------------------------------
def _oracle_fit_of(m, coupled):
    """OracleFit carrying the PRODUCT's fitted factors: O.transform then runs the reference's masked sequence
    (tpls.py:151-165 / cmtf.py:180-210 with miss_mmodedot) on them in float64 NumPy."""
    if coupled:
        loads, means, shapes = [list(f[1:]) for f in m.Xs_factors], list(m.Xs_mean), list(m.Xs_shape)
        T = m.factor_T
    else:
        loads, means, shapes, T = [list(m.X_factors[1:])], [m.X_mean], [m.X_shape], m.X_factors[0]
    R = m.n_components
    return O.OracleFit(coupled=coupled, n_components=R, block_shapes=shapes, y_shape=m.Y_shape, T=T, loadings=loads, U=m.Y_factors[0],
                       Q=m.Y_factors[1], coef=m.coef_, r2x=[np.zeros(R)] * len(loads), r2y=m.R2Y, x_means=means, y_mean=m.Y_mean,
                       has_miss=[False] * len(loads))


def _count_calls(monkeypatch, names):
    from cmtf_pls_amd.backend import HipBackend
    calls = {n: 0 for n in names}
    for n in names:
        orig = getattr(HipBackend, n)

        def wrapped(self, *a, __orig=orig, __n=n, **k):
            calls[__n] += 1
            return __orig(self, *a, **k)
        monkeypatch.setattr(HipBackend, n, wrapped)
    return calls


def _normwise(got, want):
    scale = np.nanmax(np.abs(want), axis=0, keepdims=True)
    return np.nanmax(np.abs(got - want) / (np.abs(want) + scale))


@pytest.mark.parametrize("dtype,shape", [("float32", (192, 256, 256)), ("float64", (96, 256, 128))])
def test_nan_transform_of_long_rows_from_one_read(api, monkeypatch, dtype, shape):
    """BASELINE configs[4]-shaped rows (256 x 256 f32 = 16384 vectors; 256 x 128 f64): the 1024-thread form of
    cmtfpls_project_rows_* keeps the row in registers; no score_deflate pass, no centring pass."""
    x, y, _ = O.import_synthetic(shape, 8, 6, error=0.1, seed=12)
    if dtype == "float32":
        x, y = _f32(x), _f32(y)
    m = api.tPLS(10, dtype=dtype)
    m.fit(x, y, max_iter=20)
    xt = x[:64].copy()
    xt[np.random.default_rng(4).random(xt.shape) < 0.3] = np.nan
    xt[5] = np.nan                                                # a sample without any observation: NaN scores
    calls = _count_calls(monkeypatch, ["project_rows", "score_deflate", "score", "deflate", "center"])
    got = m.transform(xt)
    assert calls["project_rows"] == 1 and calls["score_deflate"] == calls["score"] == calls["deflate"] == calls["center"] == 0
    want = O.transform(_oracle_fit_of(m, False), xt)
    assert np.all(np.isnan(got[5])) and np.all(np.isnan(want[5]))
    keep = np.arange(64) != 5
    assert _normwise(got[keep], want[keep]) <= (1e-5 if dtype == "float32" else 1e-9)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_coupled_nan_transform_from_one_read(api, monkeypatch, dtype):
    """BASELINE configs[2]'s shapes with missing values in BOTH blocks: ctPLS.transform / predict (cmtf.py:142-231) from one
    read of each block, the sample's two rows in one workgroup, the step's score averaged in the kernel."""
    trailing = (128, 128) if dtype == "float32" else (64, 64)
    x, y, cp = O.import_synthetic((512,) + trailing, 16, 10, error=0.1, seed=215)
    xm = cp.factors[0] @ np.random.default_rng(216).normal(size=(512, 10)).T + 0.1 * np.random.default_rng(5).normal(size=(512, 512))
    if dtype == "float32":
        x, xm, y = _f32(x), _f32(xm), _f32(y)
    m = api.ctPLS(10, dtype=dtype)
    m.fit([x, xm], y, max_iter=25)
    rng = np.random.default_rng(8)
    xt, xmt = x[:96].copy(), xm[:96].copy()
    xt[rng.random(xt.shape) < 0.3] = np.nan
    xmt[rng.random(xmt.shape) < 0.3] = np.nan
    xmt[7] = np.nan                                               # the matrix row of sample 7 is empty: every score of it is NaN
    calls = _count_calls(monkeypatch, ["project_rows2", "score", "deflate", "center"])
    got = m.transform([xt, xmt])
    assert calls["project_rows2"] == 1 and calls["score"] == calls["deflate"] == calls["center"] == 0
    fit = _oracle_fit_of(m, True)
    want = O.transform(fit, [xt, xmt])
    assert np.all(np.isnan(got[7])) and np.all(np.isnan(want[7]))
    keep = np.arange(96) != 7
    tol = 1e-5 if dtype == "float32" else 1e-9
    assert _normwise(got[keep], want[keep]) <= tol
    # NaN in one block only: the other block's rows are complete (the reference switches formula per block, cmtf.py:194-204)
    got1 = m.transform([xt, xm[:96]])
    assert _normwise(got1, O.transform(fit, [xt, xm[:96]])) <= tol
    p = m.predict([xt, xmt])
    wantp = O.predict(fit, [xt, xmt])
    assert _normwise(p[keep], wantp[keep]) <= 10 * tol


# ---- the whole small fit in one launch (VERDICT r2 "Next" #8) ------------------------------------------------------------------
@pytest.mark.small_fit
@pytest.mark.parametrize("shape,M,R", [((200, 10, 8), 4, 3), ((120, 40), 3, 4), ((64, 7, 33), 1, 16), ((200, 12, 12), 16, 5)])
def test_small_fit_in_one_launch_equals_the_regular_engine(api, monkeypatch, shape, M, R):
    """BASELINE configs[0] and neighbours: tPLS.fit of a small float64 problem is ONE kernel launch (cmtfpls_fit_small_f64);
    same iteration counts, factors equal to the multi-launch engine to 1e-12 and to the oracle."""
    opt = {}                                              # EngineOptions fields this test overrides
    x, y, _ = O.import_synthetic(shape, M, min(R, 4), error=0.1, seed=7)
    calls = _count_calls(monkeypatch, ["fit_small", "colstats", "mode0_contract", "mode0_contract_yq", "rank1"])
    one = api.tPLS(R, options=default_options().but(**opt))
    one.fit(x, y)
    assert calls["fit_small"] == 1 and calls["colstats"] == calls["mode0_contract"] == calls["mode0_contract_yq"] == calls["rank1"] == 0
    opt["small_fit"] = False
    reg = api.tPLS(R, options=default_options().but(**opt))
    reg.fit(x, y)
    assert calls["fit_small"] == 1 and calls["colstats"] > 0
    assert one.n_iter_ == reg.n_iter_
    for f, g in zip(one.X_factors + one.Y_factors, reg.X_factors + reg.Y_factors):
        assert f.shape == g.shape
        assert _normwise(f, g) <= 1e-10          # (late components of a noise-free remainder amplify rounding; early ones: 1e-14)
    assert _normwise(one.X_factors[0][:, :2], reg.X_factors[0][:, :2]) <= 1e-12
    assert_allclose(one.R2X, reg.R2X, rtol=0, atol=1e-12)
    assert_allclose(one.R2Y, reg.R2Y, rtol=0, atol=1e-12)
    assert_allclose(one.coef_, reg.coef_, rtol=0, atol=1e-9 * np.abs(reg.coef_).max())
    assert_allclose(one.X_mean, reg.X_mean, rtol=1e-13, atol=1e-15)
    fit = O.fit_tpls(x, y, R)
    assert one.n_iter_ == fit.n_iter
    assert _normwise(one.X_factors[0][:, :3], fit.T[:, :3]) <= 1e-9
    assert_allclose(one.R2X, fit.r2x[0], rtol=0, atol=1e-10)
    assert_allclose(one.transform(x), one.X_factors[0], rtol=1e-8, atol=1e-10)     # tests/test_tpls.py:145-155
    assert_allclose(one.predict(x[:9]), O.predict(fit, x[:9]), rtol=1e-7, atol=1e-9)


@pytest.mark.small_fit
def test_small_fit_declines_missing_values_and_large_inputs(api, monkeypatch):
    x, y, _ = O.import_synthetic((60, 9, 8), 3, 3, error=0.1, seed=8)
    xn = x.copy()
    xn[4, 2, 1] = np.nan
    calls = _count_calls(monkeypatch, ["fit_small", "colstats"])
    m = api.tPLS(2)
    m.fit(xn, y)
    assert calls["fit_small"] == 1 and calls["colstats"] > 0 and m.X_hasMiss          # flagged in the kernel, refitted by the masked engine
    fit = O.fit_tpls(xn, y, 2)
    assert _normwise(m.X_factors[0], fit.T) <= 1e-8
    big, yb, _ = O.import_synthetic((80, 40, 40), 3, 3, error=0.1, seed=9)        # 128000 elements: beyond the one-workgroup budget
    calls["fit_small"] = 0
    api.tPLS(2).fit(big, yb)
    assert calls["fit_small"] == 0


# ---- X of order 6 and 7 (round 2 stopped at 5; tpls.py:84-90 has no limit) ---------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 3, 4, 2, 3, 2), (30, 2, 3, 2, 2, 3, 2)])
@pytest.mark.parametrize("algorithm", ["direct", "xcov"])
def test_fit_of_order_6_and_7_tensors(api, shape, algorithm):
    x, y, _ = O.import_synthetic(shape, 3, 2, error=0.1, seed=17)
    m = api.tPLS(2, algorithm=algorithm)
    m.fit(x, y)
    fit = O.fit_tpls(x, y, 2)
    assert len(m.X_factors) == len(shape)
    assert m.n_iter_ == fit.n_iter
    assert _normwise(m.X_factors[0], fit.T) <= 1e-8
    for got, want in zip(m.X_factors[1:], fit.loadings[0]):
        assert_allclose(np.abs(got), np.abs(want), rtol=0, atol=1e-8)        # (signs: paired flips across modes)
        assert_allclose(np.linalg.norm(got, axis=0), 1, rtol=1e-12)
    assert_allclose(m.R2X, fit.r2x[0], rtol=0, atol=1e-9)
    assert_allclose(m.R2Y, fit.r2y, rtol=0, atol=1e-9)
    assert_allclose(m.transform(x), m.X_factors[0], rtol=1e-8, atol=1e-10)
    assert_allclose(m.predict(x[:5]), O.predict(fit, x[:5]), rtol=1e-7, atol=1e-9)
    xt = x[:6].copy()
    xt[2, 1, 2, 0, 1, 1] = np.nan                                             # the masked projection at this order too
    assert _normwise(m.transform(xt), O.transform(fit, xt)) <= 1e-8


def test_three_coupled_blocks_with_an_empty_row_keep_the_references_nan_semantics(api):
    """Three coupled blocks take the sequential passes (the one-read kernel holds two).  A sample whose row is empty in one
    block has a NaN average score at step 0 (cmtf.py:206); the reference's input-derived mask then makes every later score of
    that sample NaN as well -- not the finite values a mask re-read from the NaN-deflated rows would give."""
    rng = np.random.default_rng(23)
    lat = rng.normal(size=(80, 3))
    xs = [np.einsum("ir,jr,kr->ijk", lat, rng.normal(size=(6, 3)), rng.normal(size=(5, 3))) + 0.1 * rng.normal(size=(80, 6, 5)),
          lat @ rng.normal(size=(3, 12)) + 0.1 * rng.normal(size=(80, 12)),
          lat @ rng.normal(size=(3, 7)) + 0.1 * rng.normal(size=(80, 7))]
    y = lat @ rng.normal(size=(3, 2)) + 0.1 * rng.normal(size=(80, 2))
    m = api.ctPLS(3)
    m.fit(xs, y)
    new = [b[:12].copy() for b in xs]
    new[0][rng.random(new[0].shape) < 0.2] = np.nan
    new[1][4] = np.nan                                            # sample 4: no observation in the second block
    got = m.transform(new)
    want = O.transform(_oracle_fit_of(m, True), new)
    assert np.all(np.isnan(want[4])) and np.all(np.isnan(got[4]))
    keep = np.arange(12) != 4
    assert _normwise(got[keep], want[keep]) <= 1e-9


# ---- algorithm="xcov" on the caller's UNCENTRED tensor: never written, never copied, never centred (round 3) ---------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", ["tensor", "coupled", "order4", "matrix"])
def test_xcov_on_the_uncentred_tensor_equals_the_centred_form(api, monkeypatch, case, dtype):
    opt = {}                                              # EngineOptions fields this test overrides
    rng = np.random.default_rng(31)
    shape = {"tensor": (300, 24, 32), "coupled": (300, 24, 32), "order4": (120, 6, 5, 8), "matrix": (200, 96)}[case]
    x, y, cp = O.import_synthetic(shape, 5, 4, error=0.1, seed=13)
    x = x + 7.5                                                   # a mean 20x the spread: the corrections must not cancel badly
    blocks = [x]
    if case == "coupled":
        blocks.append(cp.factors[0] @ rng.normal(size=(64, 4)).T + 0.1 * rng.normal(size=(300, 64)) - 3.0)
    if dtype == "float32":
        blocks, y = [_f32(b) for b in blocks], _f32(y)
    make = (lambda: api.ctPLS(4, dtype=dtype, algorithm="xcov", options=default_options().but(**opt))) if case == "coupled" else (lambda: api.tPLS(4, dtype=dtype, algorithm="xcov", options=default_options().but(**opt)))
    arg = blocks if case == "coupled" else blocks[0]
    calls = _count_calls(monkeypatch, ["center", "axpy_scalar", "deflate", "score_deflate", "deflate_contract_yq"])
    raw = make()
    raw.fit(arg, y)
    assert calls["center"] == 1 and calls["axpy_scalar"] > 0                 # (the one centring call is Y's)
    assert calls["deflate"] == calls["score_deflate"] == calls["deflate_contract_yq"] == 0
    opt["xcov_raw"] = False
    cen = make()
    cen.fit(arg, y)
    assert calls["center"] == 1 + 1 + len(blocks)
    assert raw.n_iter_ == cen.n_iter_
    tol = 2e-6 if dtype == "float32" else 1e-10                   # f32: the centred copy is rounded once more than the raw tensor
    Tr = raw.factor_T if case == "coupled" else raw.X_factors[0]
    Tc = cen.factor_T if case == "coupled" else cen.X_factors[0]
    assert _normwise(Tr, Tc) <= tol
    assert _normwise(raw.Y_factors[1], cen.Y_factors[1]) <= tol
    r2r = raw.R2Xs if case == "coupled" else [raw.R2X]
    r2c = cen.R2Xs if case == "coupled" else [cen.R2X]
    for a, b in zip(r2r, r2c):
        assert_allclose(a, b, rtol=0, atol=tol)
    assert_allclose(raw.R2Y, cen.R2Y, rtol=0, atol=tol)
    fit = O.fit_ctpls(blocks, y, 4) if case == "coupled" else O.fit_tpls(blocks[0], y, 4)
    assert raw.n_iter_ == fit.n_iter
    assert _normwise(Tr, fit.T) <= (1e-5 if dtype == "float32" else 1e-9)
    assert_allclose(raw.R2Y, fit.r2y, rtol=0, atol=1e-5 if dtype == "float32" else 1e-10)
    new = [b[:20] for b in blocks]
    assert _normwise(raw.transform(new if case == "coupled" else new[0]), O.transform(fit, new if case == "coupled" else new[0])) <= (1e-5 if dtype == "float32" else 1e-9)


def test_xcov_fit_of_a_device_tensor_neither_writes_nor_copies_it(api):
    """tPLS(algorithm="xcov").fit(X_device): X is read R + 2 times and that is all -- same bits afterwards, and the fit's peak
    memory stays far below a second copy of X (inputs are never modified, tpls.py:74, without paying for a clone)."""
    from cmtf_pls_amd.synthetic import synthetic_shard_device
    X, Y = synthetic_shard_device((8192, 128, 128), 16, 10, error=0.1, device="cuda:0")          # 537 MB
    keep = X.clone()
    m = api.tPLS(5, dtype="float32", algorithm="xcov")
    m.fit(X, Y, max_iter=30)                                       # warm: workspaces sized
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m.fit(X, Y, max_iter=30)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert torch.equal(X, keep)
    assert extra < 0.25 * X.numel() * 4, f"the fit allocated {extra / 1e6:.0f} MB next to a {X.numel() * 4 / 1e6:.0f} MB tensor"
    d = api.tPLS(5, dtype="float32")                               # the direct loop deflates a private copy; the input stays as it was
    d.fit(X, Y, max_iter=30)
    assert torch.equal(X, keep) and d.n_iter_ == m.n_iter_
    s = np.abs(d.X_factors[0]).max()
    assert_allclose(m.X_factors[0], d.X_factors[0], rtol=0, atol=1e-5 * s)


# ---- one read of X per component in the xcov loop: score and its own contraction from the same pass (round 3) -------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,A,B,shift", [
    (300, 128, 128, True),      # the headline row: 4 (f32) / 8 (f64) vectors per lane, one wB set per lane
    (300, 128, 128, False),
    (7, 64, 64, True),          # fewer rows than workgroups
    (513, 100, 60, False),      # ragged row (6000 elements), a lane's vectors meet different mode-2 indices
    (256, 1, 4096, True),       # a matrix block
    (257, 3, 5000, False),      # 15000 elements: the last vector of most lanes does not exist
    (64, 16, 128, True),        # the shortest row the form takes for f32 (half the lanes idle)
    # round 4: rows beyond one workgroup's registers, split over G co-resident workgroups that exchange the partial dot products
    (700, 256, 256, True),      # the north-star row: 4 slabs (f32) / 8 (f64), 64 / 32 row streams, more rows than streams
    (40, 256, 256, False),      # fewer rows than row streams: some streams have nothing to do
    (301, 200, 128, True),      # 25600 elements: the last slab is partly empty
    (150, 3, 40000, False),     # a lane's vectors meet different mode-2 indices: 15 slabs of 8192 elements for f32 and f64
    (33, 3, 50000, False),      # 150000 elements: declined by f64 and by this f32 form (beyond 16 slabs of 8192)
    (129, 1, 100000, True),     # a matrix block with a 100000-long row
])
def test_score_contract_kernel_equals_the_two_passes(be, dtype, I, A, B, shift):
    rng = np.random.default_rng(I + A + B)
    x = rng.normal(size=(I, A * B)) + 2.0
    if dtype == torch.float32:
        x = _f32(x)
    wA, wB = rng.normal(size=A), rng.normal(size=B)
    sh = np.array([1.25]) if shift else None
    X = _dev(x).to(dtype)
    t, Z = be.empty(I), be.empty(A * B)
    out = be.score_contract(X, A, B, _dev(wA), _dev(wB), _dev(sh) if shift else None, t, Z)
    V = 4 if dtype == torch.float32 else 2
    if A * B > 16 * (16384 if (dtype == torch.float32 and (1024 * V) % B == 0) else 8192):
        assert out is None
        return
    assert out is not None
    want_t = x @ np.kron(wA, wB) - (1.25 if shift else 0.0)
    want_Z = x.T @ want_t
    assert np.abs(t.cpu().numpy() - want_t).max() <= 1e-12 * np.abs(want_t).max()
    assert np.abs(Z.cpu().numpy() - want_Z).max() <= 1e-12 * np.abs(want_Z).max()
    # against the two kernels it replaces, same inputs
    t2 = be.score(X, A, B, _dev(wA), _dev(wB), None, be.empty(I))
    if shift:
        t2 -= 1.25
    Z2 = be.mode0_contract(X, t2, False)
    assert np.abs((t - t2).cpu().numpy()).max() <= 1e-12 * np.abs(want_t).max()
    assert np.abs((Z - Z2).cpu().numpy()).max() <= 1e-12 * np.abs(want_Z).max()
    # the coupled form: own correction, the other blocks' scores, the block average
    sub, oth = rng.normal(size=I) * 10, rng.normal(size=I) * 10
    cs = be.empty(1)
    out = be.score_contract(X, A, B, _dev(wA), _dev(wB), _dev(sh) if shift else None, t, Z, sub_own=_dev(sub), add_other=_dev(oth), alpha=0.5,
                            csum=cs)
    assert out is not None
    want_c = 0.5 * (want_t - sub + oth)
    assert abs(float(cs.item()) - want_c.sum()) <= 1e-12 * np.abs(want_c).sum()
    assert np.abs(t.cpu().numpy() - (want_t - sub)).max() <= 1e-12 * np.abs(want_t).max()
    assert np.abs(Z.cpu().numpy() - x.T @ want_c).max() <= 1e-12 * np.abs(x.T @ want_c).max()


def test_score_contract_declines_rows_outside_the_registers_of_its_workgroups(be):
    """Rows shorter than half a workgroup's stride, a last mode that is not a whole number of 16-byte vectors, rows beyond 16
    workgroups' registers (round 4 lifted the limit from ONE workgroup's: 200 x 128 is served now)."""
    w = be.zeros(2100)
    for dtype, A, B in ((torch.float32, 2100, 128), (torch.float64, 1100, 128), (torch.float32, 4, 200), (torch.float32, 64, 66)):
        X = torch.zeros(8, A * B, dtype=dtype, device="cuda:0")
        assert be.score_contract(X, A, B, w[:A], w[:B], None, be.empty(8), be.empty(A * B)) is None
    for dtype in (torch.float32, torch.float64):
        X = torch.zeros(8, 200 * 128, dtype=dtype, device="cuda:0")
        assert be.score_contract(X, 200, 128, w[:200], w[:128], None, be.empty(8), be.empty(200 * 128)) is not None


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("dtype,shape", [("float32", (160, 128, 128)), ("float64", (160, 64, 128)), ("float32", (500, 4096)),
                                         ("float32", (300, 8, 16, 32)),
                                         ("float32", (72, 160, 256)), ("float64", (90, 160, 128))])      # round 4: rows split over workgroups
def test_xcov_fit_with_one_read_per_component_equals_the_two_reads(api, monkeypatch, dtype, shape, raw):
    """tPLS(algorithm="xcov") on one block reads X once per component (plus the two reads that build S and the norm): the second
    read is replaced by X_0^T yhat = sum_j b_j r_j with r_j = X_0^T t_j kept from the pass that formed t_j.  Same iterations, same
    factors as with the two reads (NipalsEngine.xcov_one_read = False) and as the oracle."""
    opt = {}                                              # EngineOptions fields this test overrides
    R = 5
    x, y, _ = O.import_synthetic(shape, 6, 4, error=0.1, seed=17)
    x = x + 4.0
    if dtype == "float32":
        x, y = _f32(x), _f32(y)
    opt["xcov_raw"] = raw
    from cmtf_pls_amd.backend import HipBackend
    calls = _count_calls(monkeypatch, ["score_contract"])
    calls["reads"] = 0                                             # passes over the I-row tensor (the inner loop makes the same calls on S)
    for name in ("mode0_contract", "score"):
        orig = getattr(HipBackend, name)

        def counted(self, X2, *a, __orig=orig, **k):
            calls["reads"] += X2.shape[0] == shape[0]
            return __orig(self, X2, *a, **k)
        monkeypatch.setattr(HipBackend, name, counted)
    one = api.tPLS(R, dtype=dtype, algorithm="xcov", options=default_options().but(**opt))
    one.fit(x, y)
    assert calls["score_contract"] == R - 1 and calls["reads"] == 1           # the last component's score
    opt["xcov_one_read"] = False
    two = api.tPLS(R, dtype=dtype, algorithm="xcov", options=default_options().but(**opt))
    two.fit(x, y)
    assert calls["score_contract"] == R - 1 and calls["reads"] == 1 + R + (R - 1)
    assert one.n_iter_ == two.n_iter_
    for f, g in zip(one.X_factors + one.Y_factors, two.X_factors + two.Y_factors):
        assert _normwise(f, g) <= 1e-10
    assert_allclose(one.R2X, two.R2X, rtol=0, atol=1e-11)
    assert_allclose(one.R2Y, two.R2Y, rtol=0, atol=1e-11)
    assert_allclose(one.coef_, two.coef_, rtol=1e-8, atol=1e-10 * np.abs(two.coef_).max())
    fit = O.fit_tpls(x, y, R)
    assert one.n_iter_ == fit.n_iter
    assert _normwise(one.X_factors[0], fit.T) <= (1e-5 if dtype == "float32" else 1e-9)
    assert_allclose(one.R2X, fit.r2x[0], rtol=0, atol=1e-6 if dtype == "float32" else 1e-9)


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("extra", [1, 2])
def test_xcov_coupled_fit_reads_the_largest_block_once_per_component(api, monkeypatch, raw, extra):
    """ctPLS(algorithm="xcov"): the deflation uses the block-AVERAGED score, so the pass over the largest block is handed the other
    blocks' scores (read first) and contracts with the average; the small blocks keep their two reads.  Same fit as with two
    reads everywhere, and as the oracle."""
    opt = {}                                              # EngineOptions fields this test overrides
    from cmtf_pls_amd.backend import HipBackend
    R, I = 5, 300
    rng = np.random.default_rng(5)
    x, y, cp = O.import_synthetic((I, 64, 64), 6, 4, error=0.1, seed=19)
    blocks = [cp.factors[0] @ rng.normal(size=(96, 4)).T + 0.1 * rng.normal(size=(I, 96)) - 2.0, _f32(x + 4.0)]     # the largest is second
    if extra == 2:
        blocks.append(np.einsum("ir,jr,kr->ijk", cp.factors[0], rng.normal(size=(6, 4)), rng.normal(size=(8, 4))) + 0.1 * rng.normal(size=(I, 6, 8)))
    blocks = [_f32(b) for b in blocks]
    y = _f32(y)
    opt["xcov_raw"] = raw
    seen = []
    orig = HipBackend.score_contract

    def counted(self, X2, *a, **k):
        out = orig(self, X2, *a, **k)
        seen.append((X2.shape[1], out is not None, k.get("alpha")))
        return out
    monkeypatch.setattr(HipBackend, "score_contract", counted)
    one = api.ctPLS(R, dtype="float32", algorithm="xcov", options=default_options().but(**opt))
    one.fit(blocks, y)
    assert seen == [(64 * 64, True, 1.0 / len(blocks))] * (R - 1)
    opt["xcov_one_read"] = False
    two = api.ctPLS(R, dtype="float32", algorithm="xcov", options=default_options().but(**opt))
    two.fit(blocks, y)
    assert len(seen) == R - 1 and one.n_iter_ == two.n_iter_
    assert _normwise(one.factor_T, two.factor_T) <= 1e-10
    for fs, gs in zip(one.Xs_factors, two.Xs_factors):
        for f, g in zip(fs[1:], gs[1:]):
            assert _normwise(f, g) <= 1e-10
    for r1, r2 in zip(one.R2Xs, two.R2Xs):
        assert_allclose(r1, r2, rtol=0, atol=1e-11)
    assert_allclose(one.R2Y, two.R2Y, rtol=0, atol=1e-11)
    fit = O.fit_ctpls(blocks, y, R)
    assert one.n_iter_ == fit.n_iter
    assert _normwise(one.factor_T, fit.T) <= 1e-5


@pytest.mark.parametrize("M", [6, 32, 40])
def test_xcov_masked_fit_builds_both_cross_covariances_in_one_pass(api, monkeypatch, M):
    """Blocks with missing values: S = X0^T Y and S2 = X0^T (Y * rowscale) are the halves of ONE matrix-core pass with the I x 2M
    right-hand side [Y, Y * rowscale] when 2 M <= 64 (M = 40: two passes as before).  Same fit as with two passes; equals the oracle."""
    opt = {}                                              # EngineOptions fields this test overrides
    from cmtf_pls_amd.backend import HipBackend
    R = 4
    x, y, _ = O.import_synthetic((300, 32, 64), M, 4, error=0.1, seed=23)
    rng = np.random.default_rng(2)
    x[rng.random(x.shape) < 0.3] = np.nan
    x, y = _f32(x), _f32(y)
    widths = []
    orig = HipBackend.xcov

    def counted(self, X2, Yd, *a, **k):
        widths.append(Yd.shape[1])
        return orig(self, X2, Yd, *a, **k)
    monkeypatch.setattr(HipBackend, "xcov", counted)
    opt["xcov_deflate_build"] = False          # (that form rebuilds S inside the deflation: its own test)
    one = api.tPLS(R, dtype="float32", algorithm="xcov", options=default_options().but(**opt))
    one.fit(x, y)
    assert widths == ([2 * M] * R if 2 * M <= 64 else [M] * (2 * R))
    opt["xcov_pair_build"] = False
    widths.clear()
    two = api.tPLS(R, dtype="float32", algorithm="xcov", options=default_options().but(**opt))
    two.fit(x, y)
    assert widths == [M] * (2 * R)
    assert one.n_iter_ == two.n_iter_
    for f, g in zip(one.X_factors + one.Y_factors, two.X_factors + two.Y_factors):
        assert _normwise(f, g) <= 1e-11
    fit = O.fit_tpls(x, y, R)
    assert one.n_iter_ == fit.n_iter
    assert _normwise(one.X_factors[0], fit.T) <= 1e-5
    assert_allclose(one.R2Y, fit.r2y, rtol=0, atol=1e-6)


@pytest.mark.parametrize("shape,dtype", [((400, 128, 128), "float32"), ((300, 24, 32), "float64"), ((500, 40, 200), "float32")])
def test_xcov_pipelined_inner_loop_is_bit_identical_to_the_waiting_loop(api, monkeypatch, shape, dtype):
    """The inner loop on S with iteration it + 1 enqueued before the host has seen iteration it's convergence norm (second buffer
    set; FitRun._inner_loop_xcov_pipelined): the same kernels on the same data in the same order as the loop that waits after
    every iteration -- identical bits and iteration counts; `max_iter` cutting the loop included."""
    opt = {}                                              # EngineOptions fields this test overrides
    x, y, _ = O.import_synthetic(shape, 6, 5, error=0.2, seed=29)
    if dtype == "float32":
        x, y = _f32(x), _f32(y)
    for max_iter in (100, 3):
        fits = []
        for pipeline in (False, True):
            opt["xcov_pipeline"] = pipeline
            m = api.tPLS(5, dtype=dtype, algorithm="xcov", options=default_options().but(**opt))
            m.fit(x, y, max_iter=max_iter)
            fits.append(m)
        wait, pipe = fits
        assert pipe.n_iter_ == wait.n_iter_
        for f, g in zip(pipe.X_factors + pipe.Y_factors, wait.X_factors + wait.Y_factors):
            assert np.array_equal(f, g)
        assert np.array_equal(pipe.coef_, wait.coef_) and np.array_equal(pipe.R2X, wait.R2X) and np.array_equal(pipe.R2Y, wait.R2Y)
    assert pipe.n_iter_ == [3] * 5 or max(pipe.n_iter_) <= 3


@pytest.mark.parametrize("case", ["coupled", "coupled_nan", "nan", "matrix"])
def test_xcov_pipelined_inner_loop_for_coupled_and_masked_blocks(api, monkeypatch, case):
    """Coupled blocks, blocks with missing values and matrix blocks run the pipelined inner loop through ONE host call per iteration
    (cmtfpls_xcov_iterate_blocks_f64): same iteration counts and factors (to rounding: the q update is one kernel there, two in the
    waiting loop) as the loop that waits after every iteration; equals the oracle."""
    opt = {}                                              # EngineOptions fields this test overrides
    from cmtf_pls_amd.backend import HipBackend
    rng = np.random.default_rng(33)
    x, y, cp = O.import_synthetic((300, 32, 64), 6, 4, error=0.2, seed=31)
    xm = cp.factors[0] @ rng.normal(size=(96, 4)).T + 0.2 * rng.normal(size=(300, 96))
    if case in ("coupled_nan", "nan"):
        x[rng.random(x.shape) < 0.2] = np.nan
    blocks = {"coupled": [x, xm], "coupled_nan": [x, xm], "nan": [x], "matrix": [xm]}[case]
    blocks, y = [_f32(b) for b in blocks], _f32(y)
    coupled = len(blocks) > 1
    plans = _count_calls(monkeypatch, ["xcov_blocks_plan"])
    fits = []
    for pipeline in (False, True):
        opt["xcov_pipeline"] = pipeline
        m = (api.ctPLS if coupled else api.tPLS)(4, dtype="float32", algorithm="xcov", options=default_options().but(**opt))
        m.fit(blocks if coupled else blocks[0], y)
        fits.append(m)
        assert (plans["xcov_blocks_plan"] > 0) == pipeline
    wait, pipe = fits
    assert pipe.n_iter_ == wait.n_iter_
    f1 = ([pipe.factor_T] + [f for fs in pipe.Xs_factors for f in fs[1:]]) if coupled else pipe.X_factors
    f2 = ([wait.factor_T] + [f for fs in wait.Xs_factors for f in fs[1:]]) if coupled else wait.X_factors
    for f, g in zip(f1 + list(pipe.Y_factors), f2 + list(wait.Y_factors)):
        assert _normwise(f, g) <= 1e-11
    ref = O.fit_ctpls(blocks, y, 4) if coupled else O.fit_tpls(blocks[0], y, 4)
    assert pipe.n_iter_ == ref.n_iter
    assert _normwise(f1[0], ref.T) <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,P,M", [(4096, 16384, 16), (1000, 4096, 32), (777, 1000, 5), (130, 514, 48), (64, 256, 1),
                                   (257, 288, 33), (300, 256, 17), (70, 64, 64), (37, 80, 4)])      # the shapes of test_gpu_kernels.py::test_xcov_mfma
def test_xcov_ssq_kernel_gives_s_and_the_centred_norm_from_one_read(be, dtype, I, P, M):
    rng = np.random.default_rng(I + P + M)
    x = rng.normal(size=(I, P)) * rng.uniform(0.5, 2.0, size=P) + rng.normal(size=P) * 5.0
    if dtype == torch.float32:
        x = _f32(x)
    y = rng.normal(size=(I, M))
    mean = x.mean(axis=0)
    X = _dev(x).to(dtype)
    S, ssq = be.xcov_ssq(X, _dev(y), _dev(mean), out=be.empty(M, P))
    want_S = y.T @ x
    assert np.abs(S.cpu().numpy() - want_S).max() <= 1e-12 * np.abs(want_S).max()
    assert torch.equal(S, be.xcov(X, _dev(y), False, out=be.empty(M, P)))          # the same matrix-core pass
    want = ((x - mean) ** 2).sum()
    assert abs(float(ssq.item()) - want) <= 1e-12 * want


@pytest.mark.parametrize("dtype,shape", [("float32", (400, 128, 128)), ("float64", (300, 24, 32)), ("float32", (350, 96))])
def test_xcov_raw_fit_takes_the_norm_from_the_s_build(api, monkeypatch, dtype, shape):
    """A fit on the uncentred tensor needs |X - X_mean|^2 for R2X: from the read that builds S (cmtfpls_xcov_ssq_*) instead of
    a read of its own (cmtfpls_recon_r2_* against a zero reconstruction).  Same R2X."""
    opt = {"xcov_stats_with_s": False}                    # (round 4 takes the column statistics out of that read too: tested in test_gpu_round4.py)
    x, y, _ = O.import_synthetic(shape, 5, 4, error=0.1, seed=41)
    x = x + 6.0
    if dtype == "float32":
        x, y = _f32(x), _f32(y)
    calls = _count_calls(monkeypatch, ["recon_r2", "xcov_ssq", "xcov"])
    one = api.tPLS(4, dtype=dtype, algorithm="xcov", options=default_options().but(**opt))
    one.fit(x, y)
    assert (calls["recon_r2"], calls["xcov_ssq"], calls["xcov"]) == (0, 1, 0)
    opt["xcov_ssq_with_s"] = False
    two = api.tPLS(4, dtype=dtype, algorithm="xcov", options=default_options().but(**opt))
    two.fit(x, y)
    assert (calls["recon_r2"], calls["xcov_ssq"], calls["xcov"]) == (1, 1, 1)
    assert one.n_iter_ == two.n_iter_
    assert_allclose(one.R2X, two.R2X, rtol=0, atol=1e-12)
    assert np.array_equal(one.X_factors[0], two.X_factors[0])
    fit = O.fit_tpls(x, y, 4)
    assert_allclose(one.R2X, fit.r2x[0], rtol=0, atol=1e-6 if dtype == "float32" else 1e-9)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,A,B,M", [(2048, 128, 128, 32), (300, 32, 64, 12), (257, 5, 52, 3), (96, 1, 1024, 64), (17, 4, 3, 8)])
def test_xcov_deflate_kernel_equals_deflating_then_building_s(be, dtype, I, A, B, M):
    """cmtfpls_xcov_deflate_*: X -= t (x) w in place, S = Y^T X0 of the deflated block, |X0|^2 -- bit for bit what the deflation
    kernel followed by the masked cross-covariance kernel give."""
    rng = np.random.default_rng(I + A + B + M)
    x = rng.normal(size=(I, A * B))
    x[rng.random(x.shape) < 0.25] = np.nan
    x[5] = np.nan                                                 # an empty row
    y, t, wA, wB = rng.normal(size=(I, M)), rng.normal(size=I), rng.normal(size=A), rng.normal(size=B)
    X1, X2 = _dev(x).to(dtype), _dev(x).to(dtype)
    ssq1 = be.deflate(X1, A, B, _dev(t), _dev(wA), _dev(wB))
    S1 = be.xcov(X1, _dev(y), True, out=be.empty(M, A * B))
    S2 = be.empty(M, A * B)
    ssq2 = be.xcov_deflate(X2, A, B, _dev(y), _dev(t), _dev(wA), _dev(wB), out=S2)
    assert ssq2 is not None
    assert torch.equal(torch.isnan(X1), torch.isnan(X2)) and torch.equal(torch.nan_to_num(X1, nan=-7.0), torch.nan_to_num(X2, nan=-7.0))
    assert torch.equal(S1, S2)
    assert abs(float(ssq1.item()) - float(ssq2.item())) <= 1e-12 * float(ssq1.item())
    xd = X1.double().cpu().numpy()
    want = y.T @ np.nan_to_num(xd)
    assert np.abs(S2.cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("dtype,shape,M", [("float32", (500, 64, 128), 16), ("float64", (300, 24, 32), 5), ("float32", (300, 7, 12), 4),
                                           ("float64", (17, 4, 3), 4)])
def test_xcov_masked_fit_deflates_inside_the_rebuild_of_s(api, monkeypatch, dtype, shape, M):
    """One block with missing values: per component the final score (one read), then ONE read + write that deflates X and builds
    [S; S2] of the next component (FitRun._finish_xcov_masked_fused) instead of a read + write and a read.  Same fit."""
    opt = {}                                              # EngineOptions fields this test overrides
    R = 4 if shape[0] > 100 else 2
    x, y, _ = O.import_synthetic(shape, M, 4, error=0.1, seed=43)
    x[np.random.default_rng(3).random(x.shape) < 0.25] = np.nan
    if dtype == "float32":
        x, y = _f32(x), _f32(y)
    calls = _count_calls(monkeypatch, ["xcov", "xcov_deflate", "score_deflate"])
    one = api.tPLS(R, dtype=dtype, algorithm="xcov", options=default_options().but(**opt))
    one.fit(x, y)
    assert (calls["xcov"], calls["xcov_deflate"], calls["score_deflate"]) == (1, R - 1, 1)
    opt["xcov_deflate_build"] = False
    two = api.tPLS(R, dtype=dtype, algorithm="xcov", options=default_options().but(**opt))
    two.fit(x, y)
    assert (calls["xcov"], calls["xcov_deflate"], calls["score_deflate"]) == (1 + R, R - 1, 1 + R)
    assert one.n_iter_ == two.n_iter_
    for f, g in zip(one.X_factors + one.Y_factors, two.X_factors + two.Y_factors):
        assert _normwise(f, g) <= 1e-10
    assert_allclose(one.R2X, two.R2X, rtol=0, atol=1e-11)
    assert_allclose(one.R2Y, two.R2Y, rtol=0, atol=1e-11)
    fit = O.fit_tpls(x, y, R)
    assert one.n_iter_ == fit.n_iter
    assert _normwise(one.X_factors[0], fit.T) <= (1e-5 if dtype == "float32" else 1e-9)
    assert_allclose(one.R2X, fit.r2x[0], rtol=0, atol=1e-6 if dtype == "float32" else 1e-9)


@pytest.mark.parametrize("A,B,M", [(128, 128, 16), (64, 256, 5), (256, 64, 32), (16, 512, 64), (128, 130, 3), (32, 64, 4), (128, 127, 4)])
def test_rank1_score_equals_rank1_then_score_bit_for_bit(be, A, B, M):
    """cmtfpls_rank1_score_f64: the extraction's last kernel and the score of the M rows of S in one launch (rows of >= 8192
    elements, B even; other shapes run the two entries) -- the same loadings and the same scores, bit for bit."""
    rng = np.random.default_rng(A + B + M)
    z = np.outer(rng.normal(size=A), rng.normal(size=B)) * 3.0 + 0.5 * rng.normal(size=(A, B))
    S = _dev(rng.normal(size=(M, A * B)))
    Z = _dev(z.reshape(-1))
    w1, v1, i1, t1 = be.empty(A), be.empty(B), be.zeros(2), be.empty(M)
    be.rank1(Z, A, B, w1, v1, info=i1)
    be.score_s(S, A, B, w1, v1, t1)                              # (the score of the M rows of S: cmtfpls_score_s_f64)
    w2, v2, i2, t2 = be.empty(A), be.empty(B), be.zeros(2), be.empty(M)
    be.rank1_score(Z, A, B, w2, v2, S, t2, info=i2)
    assert torch.equal(w1, w2) and torch.equal(v1, v2) and torch.equal(i1, i2) and torch.equal(t1, t2)
    u, s, vt = np.linalg.svd(z)
    assert abs(abs(w2.cpu().numpy() @ u[:, 0]) - 1.0) < 1e-12
