"""Response-permutation test of a coupled model (ctPLS) on the device (EngineOptions.coupled_permutations, DESIGN 8d "coupled"): G
permutations x K folds per pass from shared reads of every block (cmtfpls_kfold_wide_xcov_* per block,
cmtfpls_kfold_inner_coupled_grouped_f64, cmtfpls_kfold_combine_scores_f64, cmtfpls_kfold_epilogue_grouped_f64 with the MTTKRP and
the contraction per block), against literal ctPLS refits of every fold on Y[pi_p]; the grouped coupled entry with the identity map
against the coupled K-fold; a one-block ctPLS against the tPLS form; the declines; the C entry's checks and limits."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import _lib, ctPLS, kfold, tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import fold_ids
from cmtf_pls_amd.validate import get_q2y_kfold, kfold_predictions, permutation_test_q2y

pytestmark = pytest.mark.gpu

_TOL = {"float64": 1e-8, "float32": 1e-7}                     # tests/test_gpu_permutation.py
INNER = "cmtfpls_kfold_inner_coupled_grouped_f64"
NOT_BUILT = "coupled model: permutation device form not built"
ON = EngineOptions(small_fit=False, coupled_permutations=True)       # (small_fit as tests/conftest.py sets it for the others)


def _blocks(shapes, M, L, dtype="float64", seed=7):
    """The first block and Y from import_synthetic(shapes[0], M, L, error=0.3, seed); every further block Y_flat @ W + 0.5 noise
    with W and the noise from default_rng(8), block after block."""
    x, y, _ = O.import_synthetic(shapes[0], M, L, error=0.3, seed=seed)
    rng = np.random.default_rng(8)
    I = shapes[0][0]
    Xs = [x]
    for s in shapes[1:]:
        W = rng.standard_normal((M,) + tuple(s[1:]))
        Xs.append(np.tensordot(y.reshape(I, -1), W, axes=1) + 0.5 * rng.standard_normal(s))
    if dtype == "float32":
        Xs = [b.astype(np.float32).astype(np.float64) for b in Xs]
    return Xs, y


def _refit_q2y(Xs, y, ids, K, R, dtype):
    """(Q2Y of every component count, n_iter per fold) from one literal ctPLS refit per fold."""
    pred = np.zeros((R,) + y.shape)
    n_iter = []
    for k in range(K):
        test = ids == k
        m = ctPLS(R, dtype=dtype)
        m.fit([b[~test] for b in Xs], y[~test])
        s = m.transform([b[test] for b in Xs])
        Qr = m.Y_factors[1].T
        for r in range(1, R + 1):
            pred[r - 1, test] = ((s[:, :r] @ m.coef_[:r, :r]) @ Qr[:r] + m.Y_mean).reshape(pred[r - 1, test].shape)
        n_iter.append(list(m.n_iter_))
    return 1 - ((pred - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum(), n_iter


def _err(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def _shuffled(I, K):
    folds = np.random.default_rng(4).permutation(np.arange(I) % K)
    folds[:5] = 1                                               # unequal folds
    return folds


# ---- 1. the null against literal refits ---------------------------------------------------------------------------------------
CASES = [([(60, 10, 8), (60, 12)], 4, 3, 5, None), ([(48, 80, 96), (48, 130)], 3, 3, 3, None),
         ([(50, 30), (50, 7, 9), (50, 16)], 3, 3, 4, None), ([(36, 64, 64), (36, 256)], 16, 4, 6, None),
         ([(60, 10, 8), (60, 12)], 4, 3, 4, "shuffled")]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("shapes,M,R,K,folds", CASES)
def test_device_null_equals_literal_refits(shapes, M, R, K, folds, dtype):
    """The iteration counts are asserted equal: with the NumPy oracle every fold model of the three checked permutations of every
    case here (float64 and float32-rounded blocks, contiguous and the shuffled folds) keeps its counts when every block is
    perturbed by 1e-12 relative noise."""
    Xs, y = _blocks(shapes, M, R + 1, dtype)
    I, nb = shapes[0][0], len(shapes)
    if folds == "shuffled":
        folds = _shuffled(I, K)
    m = ctPLS(R, dtype=dtype, options=ON)
    m.fit(Xs, y)
    G = 32 // K
    P = 2 * G + 1                                               # three passes, the last one partial
    res = permutation_test_q2y(m, n_permutations=P, n_splits=K, folds=folds, random_state=3, per_component=True)
    rep = m.q2y_report_
    assert INNER in rep["form"] and "cmtfpls_kfold_combine_scores_f64" in rep["form"] and "every block" in rep["form"], rep
    assert "why" not in rep, rep
    assert rep["passes"] == 3 and rep["models_per_pass"] == K * G and rep["permutations"] == P
    assert rep["x_reads"] == [2 * R * 3] * nb
    assert res["null"].shape == (P, R) and np.all(np.isfinite(res["null"]))
    ids, K = fold_ids(I, K, folds)
    for p in (0, G + 1, P - 1):                                 # one permutation of every pass
        pi = res["permutations"][p]
        want, n_iter = _refit_q2y(Xs, y[pi], ids, K, R, dtype)
        err = _err(res["null"][p], want)
        print(f"coupled permutation null: case {shapes} {dtype} p {p}: err {err:.3g}, n_iter {rep['n_iter'][p]} / {n_iter}")
        assert err <= _TOL[dtype], (p, err, res["null"][p], want)
        assert rep["n_iter"][p] == n_iter, (p, rep["n_iter"][p], n_iter)
    q = get_q2y_kfold(m, n_splits=K, folds=folds, per_component=True)
    np.testing.assert_array_equal(res["q2y"], q)
    np.testing.assert_array_equal(res["p_value"], (1 + (res["null"] >= q).sum(axis=0)) / (P + 1))


# ---- 2. the identity map is bitwise the coupled K-fold --------------------------------------------------------------------------
@pytest.mark.parametrize("shapes,M,R,K,folds", CASES)
def test_grouped_coupled_run_with_identity_map_is_bitwise_coupled_kfold(shapes, M, R, K, folds):
    Xs, y = _blocks(shapes, M, R + 1, seed=9)
    I = shapes[0][0]
    if folds == "shuffled":
        folds = _shuffled(I, K)
    m = ctPLS(R, dtype="float64")
    m.fit(Xs, y)
    want = kfold_predictions(m, n_splits=K, folds=folds)
    assert "cmtfpls_kfold_inner_coupled_f64" in m.q2y_report_["form"]
    ids, K = fold_ids(I, K, folds)
    be = m._get_engine().be                                     # the coupled K-fold device form with model k = fold k in one group
    Yh = y.reshape(I, -1).astype(np.float64)
    order, off, ybar, nu, Yk = kfold._fold_y(Yh, ids, K)
    t = lambda a, dt=torch.float64: kfold._to_dev(a, be.device, dt)
    X2s, built = [], []
    for x in Xs:
        A, B = kfold._dims(x)
        X2 = t(x.reshape(I, A * B))
        S, mean = be.empty(K, M, A * B), be.empty(K, A * B)
        assert be.kfold_xcov(X2, A, B, t(Yh - ybar), t(order, torch.int32), t(off, torch.int32), K, t(nu - ybar), S, mean) is not None
        X2s.append(X2)
        built.append((A, B, S, mean))
    st, shared, own = kfold._state(be, t(ids, torch.int32), t(Yk), built, R, 1)
    mf = torch.arange(K, dtype=torch.int32, device=be.device)
    assert kfold._components(be, X2s, st, shared, own, R, 1e-8, 100, True, grouped=(mf, 1)) is None
    assert not shared["status"].any()
    got = kfold._held_out_predictions(shared["Tout"][0].cpu().numpy(), shared["coef"].cpu().numpy(), shared["Q"].cpu().numpy(), nu,
                                      ids, K, R, M)
    assert np.array_equal(got.reshape(want.shape), want)
    assert shared["n_iter"].cpu().numpy().tolist() == m.q2y_report_["n_iter"]


# ---- 3. one block is bitwise the tPLS form --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,M,R,K", [((60, 10, 8), 4, 3, 5), ((50, 30), 3, 3, 4), ((20, 6, 5), 2, 2, 2)])
def test_one_block_is_bitwise_the_tpls_form(shape, M, R, K):
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=7)
    c = ctPLS(R, dtype="float64", options=ON)
    c.fit([x], y)
    t = tPLS(R, dtype="float64")
    t.fit(x, y)
    P = 2 * (32 // K) + 1
    perms = np.stack([np.random.default_rng(s).permutation(shape[0]) for s in range(P)])
    rc = permutation_test_q2y(c, permutations=perms, n_splits=K, per_component=True)
    rt = permutation_test_q2y(t, permutations=perms, n_splits=K, per_component=True)
    assert INNER in c.q2y_report_["form"] and "why" not in c.q2y_report_, c.q2y_report_
    assert "cmtfpls_kfold_inner_grouped_f64" in t.q2y_report_["form"] and "why" not in t.q2y_report_, t.q2y_report_
    assert c.q2y_report_["x_reads"] == [t.q2y_report_["x_reads"]] and c.q2y_report_["passes"] == t.q2y_report_["passes"]
    assert np.array_equal(rc["null"], rt["null"]) and np.array_equal(rc["p_value"], rt["p_value"])
    assert c.q2y_report_["n_iter"] == t.q2y_report_["n_iter"]


# ---- 4. identity permutation, the caller's tensors, a strong signal ---------------------------------------------------------------
def test_identity_permutation_equals_observed():
    Xs, y = _blocks([(60, 10, 8), (60, 12)], 4, 4, seed=5)
    m = ctPLS(3, dtype="float64", options=ON)
    m.fit(Xs, y)
    perms = np.stack([np.random.default_rng(1).permutation(60), np.arange(60), np.random.default_rng(2).permutation(60)])
    res = permutation_test_q2y(m, permutations=perms, per_component=True)
    assert INNER in m.q2y_report_["form"] and "why" not in m.q2y_report_, m.q2y_report_
    assert np.abs(res["null"][1] - res["q2y"]).max() <= 1e-10, (res["null"][1], res["q2y"])


def test_callers_device_tensors_are_only_read():
    I, J, K, M, R = 4096, 24, 20, 4, 3
    g = torch.Generator(device="cuda:0").manual_seed(3)
    T = torch.randn(I, R, device="cuda:0", dtype=torch.float64, generator=g)
    X = torch.einsum("il,jl,kl->ijk", T, torch.randn(J, R, device="cuda:0", dtype=torch.float64, generator=g),
                     torch.randn(K, R, device="cuda:0", dtype=torch.float64, generator=g)).to(torch.float32)
    X += 0.5 * torch.randn(I, J, K, device="cuda:0", dtype=torch.float32, generator=g)
    Z = (T @ torch.randn(R, 40, device="cuda:0", dtype=torch.float64, generator=g)).to(torch.float32)
    Z += 0.5 * torch.randn(I, 40, device="cuda:0", dtype=torch.float32, generator=g)
    Y = T @ torch.randn(M, R, device="cuda:0", dtype=torch.float64, generator=g).T
    m = ctPLS(R, dtype="float32", options=ON)
    m.fit([X, Z], Y)
    bx, bz = X.clone(), Z.clone()
    res = permutation_test_q2y(m, n_permutations=8)
    assert INNER in m.q2y_report_["form"] and "why" not in m.q2y_report_, m.q2y_report_
    assert torch.equal(X, bx) and torch.equal(Z, bz)
    assert res["p_value"] == pytest.approx(1 / 9)                 # a strong signal beats every permutation


# ---- 5. declines ------------------------------------------------------------------------------------------------------------
def _decline_case(case):
    shapes, M, R, K = [(40, 6, 5), (40, 7)], 3, 2, 4
    if case == "order4":
        shapes = [(24, 4, 3, 5), (24, 7)]
    if case == "m65":
        M = 65
    if case == "9 blocks":
        shapes = [(40, 6, 5)] + [(40, 4)] * 8
    Xs, y = _blocks(shapes, M, R + 1, seed=12)
    if case == "nan":
        Xs[1][3, 2] = np.nan
    if case == "offset":
        Xs[1] = Xs[1] + 1e6
    return Xs, y, R, K


WHY = {"nan": "missing values in block 1", "order4": "block 0 of order 4", "m65": "M = 65 responses > 64", "9 blocks": "9 blocks > 8",
       "offset": "block 1: max|column mean| / spread"}


@pytest.mark.parametrize("case", list(WHY))
def test_declines_refit_with_why_and_equal_the_option_off(case):
    Xs, y, R, K = _decline_case(case)
    on, off = ctPLS(R, dtype="float64", options=ON), ctPLS(R, dtype="float64")
    on.fit(Xs, y)
    off.fit(Xs, y)
    got = permutation_test_q2y(on, n_permutations=2, n_splits=K, per_component=True)
    rep = on.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep["passes"] == 0 and WHY[case] in rep["why"], rep
    want = permutation_test_q2y(off, n_permutations=2, n_splits=K, per_component=True)
    assert off.q2y_report_["why"] == NOT_BUILT
    assert got["null"].shape == (2, R)
    np.testing.assert_array_equal(got["null"], want["null"])


def test_device_nan_declines_after_the_first_pass_statistics():
    Xs, y = _blocks([(40, 6, 5), (40, 7)], 3, 3, seed=13)
    xd, zd = torch.from_numpy(Xs[0]).cuda(), torch.from_numpy(Xs[1]).cuda()
    on, off = ctPLS(2, dtype="float64", options=ON), ctPLS(2, dtype="float64")
    on.fit([xd, zd], y)
    off.fit([xd, zd], y)
    zd[5, 2] = float("nan")                                     # (after the fit: only the permutation test sees it)
    got = permutation_test_q2y(on, n_permutations=2, n_splits=4)
    rep = on.q2y_report_
    assert rep["form"].startswith("one refit per fold") and rep["passes"] == 0, rep
    assert "non-finite" in rep["why"] and "block 1" in rep["why"], rep
    want = permutation_test_q2y(off, n_permutations=2, n_splits=4)
    np.testing.assert_array_equal(got["null"], want["null"])


def test_with_masked_folds_coupled_a_nan_takes_the_masked_form():
    Xs, y, R, K = _decline_case("nan")
    m = ctPLS(R, dtype="float64", options=ON.but(masked_folds_coupled=True))
    m.fit(Xs, y)
    permutation_test_q2y(m, n_permutations=2, n_splits=K)
    assert kfold.COUPLED_FORM in m.q2y_report_["form"] and INNER not in m.q2y_report_["form"], m.q2y_report_


# ---- 6. the option off --------------------------------------------------------------------------------------------------------
def test_option_off_keeps_the_refits_and_their_why():
    Xs, y = _blocks([(30, 6, 5), (30, 7)], 2, 3, seed=13)
    m = ctPLS(2, dtype="float64")
    m.fit(Xs, y)
    res = permutation_test_q2y(m, n_permutations=2, n_splits=3, per_component=True)
    rep = m.q2y_report_
    assert rep["why"] == NOT_BUILT and rep["passes"] == 0 and rep["x_reads"] is None and rep["models_per_pass"] is None
    assert rep["form"] == "one refit per fold and permutation on the regular engine"
    ids, K = fold_ids(30, 3)
    X, Y = kfold._training_data(m)
    for p in range(2):                                          # the refit path itself, permutation by permutation
        num, n_iter = kfold._refit_numerators(m, X, Y, ids, K, res["permutations"][p], 1e-8, 100)
        np.testing.assert_array_equal(res["null"][p], 1.0 - num / float((y.astype(np.float64) ** 2).sum()))
        assert rep["n_iter"][p] == n_iter
        want, _ = _refit_q2y(Xs, y[res["permutations"][p]], ids, K, 2, "float64")
        assert _err(res["null"][p], want) <= 1e-12


# ---- 7. the C entry's checks and limits ---------------------------------------------------------------------------------------
def _state_of(Xs, y, K, g, R):
    """A grouped coupled state of K g models on the device, as permutation._device_null lays it out (S and the means left
    uninitialised: for argument checks that launch nothing)."""
    from cmtf_pls_amd.backend import HipBackend
    be = HipBackend(torch.device("cuda:0"))
    I = Xs[0].shape[0]
    M = y.reshape(I, -1).shape[1]
    n = K * g
    ids, _ = fold_ids(I, K)
    built = [(A, B, be.empty(n, M, A * B), be.empty(K, A * B)) for A, B in (kfold._dims(x) for x in Xs)]
    st, shared, own = kfold._state(be, kfold._to_dev(ids, be.device, torch.int32), be.zeros(n, I, M), built, R, g)
    mf = torch.arange(n, dtype=torch.int32, device=be.device) // g
    ws = torch.empty(max(be.kfold_inner_coupled_workspace_bytes(st), 256), dtype=torch.uint8, device=be.device)
    return be, st, (shared, own), mf, ws


def test_c_entry_rejects_bad_arguments_before_any_launch():
    Xs, y = _blocks([(40, 6, 5), (40, 7)], 3, 3)
    be, st, keep, mf, ws = _state_of(Xs, y, 4, 2, 2)
    with pytest.raises(_lib.CmtfplsError, match="kfold_inner_coupled_grouped failed with status 1"):
        be.kfold_inner_coupled_grouped(st, mf, 3, 0, 1e-8, 100, ws)                       # 8 models in 3 groups
    be2, st2, keep2, _, _ = _state_of(Xs, y, 4, 2, 2)
    mixed = (_lib.KfoldState * 2)(st[0], st2[1])                                           # views that do not share a buffer
    with pytest.raises(_lib.CmtfplsError, match="kfold_inner_coupled_grouped failed with status 1"):
        be.kfold_inner_coupled_grouped(mixed, mf, 2, 0, 1e-8, 100, ws)
    torch.cuda.synchronize()
    assert not keep[0]["n_iter"].any() and not keep2[0]["n_iter"].any()                    # nothing was launched (a launch counts >= 1)


def test_c_entry_declines_a_side_of_257():
    Xs = [np.zeros((12, 257, 258)), np.zeros((12, 7))]
    be, st, keep, mf, ws = _state_of(Xs, np.zeros((12, 2)), 2, 2, 2)
    assert be.kfold_inner_coupled_grouped(st, mf, 2, 0, 1e-8, 100, ws) is None            # CMTFPLS_EUNSUPPORTED


def _limit_case(name):
    """(blocks, y, R, K, permutations) with one limit reached; data as tests/test_gpu_kfold_limits.py builds its K-fold limit
    cases (import_synthetic with R + 1 latent components, error 0.3, seed 7), so that no fold degenerates."""
    if name == "32 models":
        shapes, M, R, K, P = [(60, 10, 8), (60, 12)], 4, 3, 2, 16
    elif name == "M 64":
        shapes, M, R, K, P = [(60, 10, 8), (60, 12)], 64, 4, 3, 4
    elif name == "8 blocks":
        shapes, M, R, K, P = [(60, 10, 8)] + [(60, 5 + b) for b in range(7)], 4, 3, 5, 3
    elif name == "side 256":
        shapes, M, R, K, P = [(40, 256, 260), (40, 9)], 3, 2, 3, 2
    else:                                                       # "R 64": 133 training rows, both blocks of rank >= 64
        shapes, M, R, K, P = [(200, 10, 12), (200, 90)], 4, kfold.MAX_COMPONENTS, 3, 2
    Xs, y = _blocks(shapes, M, R + 1)
    return Xs, y, R, K, P


@pytest.mark.parametrize("name", ["32 models", "M 64", "8 blocks", "side 256", "R 64"])
def test_at_the_limits_equals_the_option_off_null(name):
    Xs, y, R, K, P = _limit_case(name)
    on, off = ctPLS(R, dtype="float64", options=ON), ctPLS(R, dtype="float64")
    on.fit(Xs, y)
    off.fit(Xs, y)
    got = permutation_test_q2y(on, n_permutations=P, n_splits=K, random_state=3, per_component=True)
    rep = on.q2y_report_
    assert INNER in rep["form"] and "why" not in rep, rep
    G = min(32 // K, P)
    assert rep["models_per_pass"] == K * G and rep["passes"] == -(-P // G) and rep["x_reads"] == [2 * R * rep["passes"]] * len(Xs)
    want = permutation_test_q2y(off, n_permutations=P, n_splits=K, random_state=3, per_component=True)
    assert off.q2y_report_["why"] == NOT_BUILT
    err = max(_err(got["null"][p], want["null"][p]) for p in range(P))
    print(f"coupled permutation at the limit {name}: err {err:.3g}")
    assert err <= _TOL["float64"], (name, err)
