"""The K-fold epilogue kernels of csrc/kfold.hip stage by stage against the long-double restatement tests/kfold_epilogue_ref.py:
kfold_rows_kernel<MODE>, kfold_solve_kernel, kfold_ydefl_kernel<MODE> (cmtfpls_kfold_epilogue_f64 / _grouped / _splits /
_weighted, stages 0 and 1), kfold_downdate_kernel<GROUPED> (stage 2), kfold_combine_kernel, and the tail of kfold_inner_kernel
(mu^T w and g).

Every case builds its state by hand (kfold._state), every field the stage does not own holding an input or the sentinel, and
runs the entry on two clones: both give the same bits; every element outside the stage's written-field mask keeps its bits;
EXACT inputs equal the restatement bit for bit; ROUNDING inputs lie inside the derived bound (never a fitted tolerance).  The
three kernels of stage 1 are separated by giving each restatement the device's own inputs (the row sums the device's T[:, a],
the solve the tile-order totals of the device's `part`, the deflation the device's vec[:kk], the Gram the device's Yk), then the
solve is bounded once from the original inputs (`composed`).  The worst error / bound per kernel is printed at teardown.

One narrowing against "once from the original inputs through all three kernels": the composed check runs from the original
inputs through the row kernel and the solve and stops at the residual of the restated normal equations.  A bound of the
deflated Yk from the original inputs would need a forward bound of b, that is the conditioning of the Gram, which the residual
form avoids on purpose; Yk and the next Gy are instead bounded from the device's own vec[:kk] and Yk, link by link.

Worst error / bound on the MI355X (rounding inputs, every case of this file):
  rows T 0.593 | rows part 0.267 | solve residual 0.220 | solve c = Gt b 0.924 | composed residual 0.083 | ydefl Yk 0.996 |
  ydefl Gy 0.078 | stage 0 Gy 0.060 | downdate Rm 0.490 | downdate S 0.335 | combine 0.403 | inner mu^T w < 0.001 | inner g 0.018
The three above 0.5 are the shortest chains, where the kernel makes nearly every rounding the bound allows.  rows T: t takes
a + 1 roundings (sc - mu^T w, then one per fused T g) against gamma_(a + 2), so the ratio can reach (a + 1) / (a + 2); 0.593 is
(257, 3, 3, 4, a = 1) weighted "single", two roundings against gamma_3 (at a = 0 it cannot pass 0.5).  c = Gt b at kk = 1 is one
product against gamma_1.  The deflated Yk at kk = 1 is one fused y - (t b) q whose result is as large as |y| + |t b q| when the
two have opposite signs, against u |y| + 3 u |t b q|.  The long sums sit far below their bounds, as sums of n terms in a tree do.
"""
import numpy as np
import pytest
import torch

import kfold_epilogue_ref as KE
import small_algebra_ref as SA
import solve_ref as SR
from cmtf_pls_amd import kfold

pytestmark = pytest.mark.gpu

LD = np.longdouble
KINDS = ["exact", "rounding"]


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend("cuda:0")


_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, r in sorted(_worst.items()):
        print(f"worst error / bound {k}: {r:.3f}")


def check(kernel, kind, got, want, bound):
    """exact inputs: equality with the restatement; rounding inputs: |got - want| <= bound elementwise (a bound of 0: equality),
    the worst ratio recorded."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=LD).reshape(got.shape)
    if kind == "exact":
        assert np.array_equal(got, want.astype(np.float64)), (kernel, np.argwhere(got != want.astype(np.float64))[:4])
        return
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape)
    assert np.all(np.isfinite(err)) and np.all(bound >= 0), kernel
    assert np.all(err[bound == 0] == 0), kernel
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"{kernel}: worst error / bound {ratio:.3f}")
    _worst[kernel] = max(_worst.get(kernel, 0.0), ratio)
    assert ratio <= 1.0, (kernel, ratio)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- a host state on the device ---------------------------------------------------------------------------------------------
def upload(be, st):
    """(view, tensors): kfold._state over the host state's shapes, every field filled from it."""
    t = lambda a, dt=torch.float64: kfold._to_dev(a, be.device, dt)
    n, I, M, R = KE.dims(st)
    A, B = st["Wa"].shape[2], st["Wb"].shape[2]
    views, shared, own = kfold._state(be, t(st["fold_of"], torch.int32), t(st["Yk"]), [(A, B, t(st["S"]), t(st["mean"]))], R,
                                      st["Tout"].shape[0])
    tensors = {**shared, **own[0]}
    for f, v in st.items():
        assert tuple(tensors[f].shape) == v.shape, (f, tensors[f].shape, v.shape)
        tensors[f].copy_(t(v, tensors[f].dtype))
    return views, tensors


def download(tensors):
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in tensors.items()}


def epilogue(be, lay, view, n, stage, a, src):
    if lay.mode == KE.GROUPED:
        mf = kfold._to_dev(lay.model_fold, be.device, torch.int32)
        return be.kfold_epilogue_grouped(view, mf, lay.div, stage, a, src)
    if lay.mode == KE.SPLITS:
        return be.kfold_epilogue_splits(view, n // lay.div, stage, a, src)
    if lay.mode == KE.WEIGHTED:
        return be.kfold_epilogue_weighted(view, stage, a, src)
    return be.kfold_epilogue(view, stage, a, src)


def run_twice(be, lay, st, stage, a, src):
    """The entry on two clones of the host state: the same bits; outside the written-field mask the bits of before.  Returns the
    state after."""
    n = st["Yk"].shape[0]
    srcd = None if src is None else kfold._to_dev(src, be.device)
    outs = []
    for _ in range(2):
        views, tensors = upload(be, st)
        assert epilogue(be, lay, views[0], n, stage, a, srcd) is True
        outs.append(download(tensors))
    masks = KE.written(stage, lay, st, a)
    for f in st:
        assert same(outs[0][f], outs[1][f]), ("two runs differ", f)
        m = masks.get(f, np.zeros(st[f].shape, dtype=bool))
        assert np.array_equal(bits(outs[0][f])[~m], bits(st[f])[~m]), ("written outside its mask", f)
    if srcd is not None:
        assert same(srcd.cpu().numpy(), src)
    return outs[0]


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------------
def check_stage1(be, kind, lay, st, sc, solve_exact, a, skip=()):
    """Stage 1 of component a on (lay, st, sc) against the restatement; `skip`: models whose numbers are not compared (a planted
    NaN).  Returns the state after."""
    n, I, M, R = KE.dims(st)
    kk, nv = a + 1, 2 * (a + 1) + 1 + M
    after = run_twice(be, lay, st, 1, a, sc)
    ks = [k for k in range(n) if k not in skip]
    # -- the row kernel on its own: T from the inputs; tm, Tout and the partial sums from the device's own column
    ref = KE.rows(lay, st, a, sc)
    tdev = np.ascontiguousarray(after["T"][:, :, a])
    check("rows T", kind, tdev[ks], ref["T"][ks], ref["T_err"][ks])
    for k in ks:
        train, w = KE.training(lay, st["fold_of"], k)
        assert same(after["tm"][:, k], np.where(train, w * tdev[k], 0.0)), ("tm", k)
    for slot, held, k in ref["tout"]:
        assert k in skip or same(after["Tout"][slot, held, a], tdev[k, held]), ("Tout", k)
    ref2 = KE.rows(lay, st, a, sc, t_dev=tdev)
    check("rows part", kind, after["part"][ks][:, :, :nv], ref2["part"][ks], ref2["part_err"][ks])
    # -- the solve on its own: from the tile-order float64 totals of the device's own partial sums
    st2 = KE.copy_state(st)
    st2["part"] = after["part"]
    bdev = np.ascontiguousarray(after["coef"][:, :kk, a])
    sv = KE.solve(st2, a, b_dev=bdev)
    tot = sv["tot"]
    assert same(after["vec"][:, :kk], bdev)
    for k in ks:
        assert same(after["Gt"][k, a, :kk], tot[k, :kk]) and same(after["Gt"][k, :kk, a], tot[k, :kk]), k
        assert same(after["vec"][k, 2 * R:2 * R + M], tot[k, 2 * kk + 1:nv]) and same(after["vec"][k, 2 * R + M], tot[k, 2 * kk]), k
        r = sv["ref"][k]
        assert r.dropped == sv["dropped"][k], (k, r.dropped, sv["dropped"][k])
        assert np.all(bdev[k][r.dropped] == 0.0), k
        assert after["status"][k] == st["status"][k] | (2 if sv["bad"][k] else 0), k
        if kind == "exact":
            if solve_exact:
                assert np.array_equal(bdev[k], r.b.astype(np.float64)) and np.array_equal(bdev[k], sv["b_serial"][k]), k
        elif len(r.kept):
            res, bnd = SR.normal_solve_bound(r, bdev[k])
            check("solve residual", kind, res, np.zeros_like(res), bnd)
        if kind == "rounding" or solve_exact:
            check("solve c = Gt b", kind, after["vec"][k, R:R + kk], sv["c"][k], sv["c_err"][k])
    # -- the deflation and the next Gram on their own: from the device's vec[:kk], then from the device's Yk
    if a + 1 < R:
        st3 = KE.copy_state(st)
        st3["T"][:, :, a], st3["vec"] = tdev, after["vec"]
        yd = KE.ydefl(lay, st3, a, 1, y_dev=after["Yk"])
        if kind == "rounding" or solve_exact:
            check("ydefl Yk", kind, after["Yk"][ks], yd["Yk"][ks], yd["Yk_err"][ks])
            check("ydefl Gy", kind, after["Gy"][ks], yd["Gy"][ks], yd["Gy_err"][ks])
    # -- once from the original inputs through rows and solve: the residual of the restated normal equations
    if kind == "rounding":
        for k in ks:
            G, g, eG, eg = KE.composed_system(lay, st, a, ref, k)
            ref0, rdev = SR.normal_solve(G, g), sv["ref"][k]
            assert ref0.dropped == rdev.dropped, k
            K, bnd = KE.composed_residual(rdev, bdev[k], ref0.d, eG, eg)
            if len(K):
                xh = bdev[k][K].astype(LD) / ref0.d[K]
                res = np.abs(ref0.Ahat[np.ix_(K, K)] @ xh - ref0.yhat[K]).astype(np.float64)
                check("composed residual", kind, res, np.zeros_like(res), bnd)
    return after


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", KE.row_stage_cases(), ids=lambda c: "-".join(str(x) for x in c))
def test_stage1(be, kind, case):
    I, M, K, R, a, mode, mp = case
    lay, st, sc, solve_exact = KE.row_state(kind, mode, mp, I, M, K, R, a)
    check_stage1(be, kind, lay, st, sc, solve_exact, a)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mode", KE.MODES)
@pytest.mark.parametrize("I,M,K,R", [(257, 3, 3, 4), (777, 17, 5, 3), (32769, 2, 2, 2)])
def test_stage0_gram(be, kind, mode, I, M, K, R):
    """Stage 0: the tiles' Y_k^T (C) Y_k and nothing else, whatever `a` is."""
    lay, st, _, _ = KE.row_state(kind, mode, "shuffled", I, M, K, R, 0)
    after = run_twice(be, lay, st, 0, 0, None)
    yd = KE.ydefl(lay, st, 0, 0)
    check("stage 0 Gy", kind, after["Gy"], yd["Gy"], yd["Gy_err"])


@pytest.mark.parametrize("a", [1, 3])
def test_zero_and_doubled_columns(be, a):
    """(257, 3, 3, 4), exact inputs: model 0's column a is identically zero on its training rows (coefficient 0, status 0), model
    1's is exactly twice its column 0 (dropped: coefficient 0, the other coefficients those of the kept columns)."""
    lay, st, sc, solve_exact = KE.row_state("exact", KE.PLAIN, "contiguous", 257, 3, 3, 4, a, special={0: "zero", 1: "double"})
    assert solve_exact
    after = check_stage1(be, "exact", lay, st, sc, True, a)
    assert np.all(after["coef"][:2, a, a] == 0.0) and after["coef"][2, a, a] != 0.0
    assert np.any(after["coef"][1, :a, a] != 0.0) and after["Gt"][0, a, a] == 0.0 and after["Gt"][1, a, a] == 4.0 * after["Gt"][1, 0, 0]
    assert np.array_equal(after["status"], st["status"])


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("mode", KE.MODES)
def test_one_non_finite_score_marks_one_model(be, mode, bad):
    """One NaN (one inf) in a training row of sc for model 1: that model gets status bit 2; every other model's outputs are the
    clean run's bits and its status stays."""
    I, M, K, R, a = 777, 17, 5, 3, 1
    lay, st, sc, _ = KE.row_state("rounding", mode, "shuffled", I, M, K, R, a)
    n = st["Yk"].shape[0]
    clean = run_twice(be, lay, st, 1, a, sc)
    row = int(np.flatnonzero(KE.training(lay, st["fold_of"], 1)[0])[200])
    sc2 = sc.copy()
    sc2[row, 1] = bad
    after = check_stage1(be, "rounding", lay, st, sc2, False, a, skip=(1,))
    assert after["status"][1] == st["status"][1] | 2
    others = [k for k in range(n) if k != 1]
    assert np.array_equal(after["status"][others], st["status"][others])
    for f in ("T", "Yk", "Gy", "Gt", "coef", "vec", "part"):
        assert same(after[f][others], clean[f][others]), f
    assert same(after["tm"][:, others], clean["tm"][:, others])
    tout = KE.written(1, lay, st, a)["Tout"]
    for slot, held, k in KE.rows(lay, st, a, sc)["tout"]:
        if k != 1:
            assert same(after["Tout"][slot, held, a], clean["Tout"][slot, held, a])
    assert tout.any() or mode == KE.WEIGHTED


# ---- stage 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
@pytest.mark.parametrize("a", [0, KE.DOWNDATE_R - 1])
@pytest.mark.parametrize("A,B", KE.DOWNDATE_AB)
def test_downdate(be, kind, grouped, a, A, B):
    lay, st, rs = KE.downdate_state(kind, grouped, A, B, KE.DOWNDATE_M, KE.DOWNDATE_R, a)
    after = run_twice(be, lay, st, 2, a, rs)
    ref = KE.downdate(lay, st, a, rs)
    check("downdate Rm", kind, after["Rm"][:, a], ref["Rm"], ref["Rm_err"])
    check("downdate S", kind, after["S"], ref["S"], ref["S_err"])


# ---- combine ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nb,n", KE.COMBINE_CASES)
def test_combine(be, kind, nb, n):
    rng = np.random.default_rng([37, nb, n, KINDS.index(kind)])
    sc = SA.inputs(kind, rng, nb, n)
    d = kfold._to_dev(sc, be.device)
    out = torch.full((n + 2,), KE.SENTINEL, dtype=torch.float64, device=be.device)
    got = be.kfold_combine_scores(d, out[1:n + 1]).cpu().numpy()
    want, bound, f64 = KE.combine(sc)
    assert np.array_equal(got, f64)                                                 # the kernel's own operations in block order
    check("combine", "rounding", got, want, bound)
    assert same(be.kfold_combine_scores(d, torch.empty(n, dtype=torch.float64, device=be.device)).cpu().numpy(), got)
    assert float(out[0]) == KE.SENTINEL and float(out[n + 1]) == KE.SENTINEL and same(d.cpu().numpy(), sc)


def test_combine_past_the_grid_cap(be):
    """nb = 2, n = 65536 * 256 + 3: the grid stops at 65536 workgroups, so the last three elements come from the stride loop.
    Integers: (a + b) / 2 is exact."""
    nb, n = KE.COMBINE_STRIDE_CASE
    g = torch.Generator(device="cpu").manual_seed(5)
    sc = torch.randint(-8, 9, (nb, n), generator=g, dtype=torch.int32).to(torch.float64)
    d = sc.to(be.device)
    out = torch.full((n + 2,), KE.SENTINEL, dtype=torch.float64, device=be.device)
    be.kfold_combine_scores(d, out[1:n + 1])
    want = ((sc[0] + sc[1]) / 2.0).to(be.device)
    assert torch.equal(out[1:n + 1], want)
    assert float(out[0]) == KE.SENTINEL and float(out[n + 1]) == KE.SENTINEL


# ---- the tail of kfold_inner: mu^T w and g -----------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
@pytest.mark.parametrize("A,B", [(1500, 1), (40, 33)], ids=["order2", "order3"])
def test_inner_tail_matches_the_devices_own_loadings(be, grouped, A, B):
    """be.kfold_inner / kfold_inner_grouped for a = 0 then a = 1 on a hand state with P past one 1024-thread stride: vec[3R+M+1]
    = mean[row] . (wA (x) wB) and g_0 = (wA_0 . wA_1)(wB_0 . wB_1), against the device's own Wa / Wb in long double.  Bounds:
    mu^T w is P fused terms of a rounded product (chain P + 1); g is the product of two sums known to gamma_A and gamma_B."""
    n, I, M, R, P = 4, 8, 2, 2, A * B
    rng = np.random.default_rng([41, A, B, int(grouped)])
    lay = KE.Layout(KE.GROUPED, (np.arange(n) // 2).astype(np.int32), 2, 2) if grouped else KE.Layout(KE.PLAIN, None, 1, 1)
    st = KE.empty_state(n, I, M, R, A, B, lay.slots, np.arange(I) % (2 if grouped else n), mean_rows=2 if grouped else n)
    for k in range(n):                                                             # a dominant rank-one term plus two smaller ones
        S = sum(s * np.outer(rng.normal(size=M), np.kron(rng.normal(size=A), rng.normal(size=B))) for s in (1.0, 0.3, 0.1))
        st["S"][k] = S
    st["mean"][:] = rng.normal(size=st["mean"].shape)
    st["Gy"][:] = 0.0
    st["Gy"][:, 0] = np.eye(M) * float(I)
    st["Wa"][:], st["Wb"][:] = 0.0, 0.0
    views, tensors = upload(be, st)
    ws = torch.empty(be.kfold_inner_workspace_bytes(A, B, n), dtype=torch.uint8, device=be.device)
    mf = kfold._to_dev(lay.model_fold, be.device, torch.int32) if grouped else None
    for a in range(2):
        ok = be.kfold_inner_grouped(views[0], mf, 2, a, 1e-8, 100, ws) if grouped else be.kfold_inner(views[0], a, 1e-8, 100, ws)
        assert ok is True
        after = download(tensors)
        assert not after["status"].any()
        for k in range(n):
            wa, wb = after["Wa"][k, a], after["Wb"][k, a]
            mu = st["mean"][k // 2 if grouped else k]
            w = SA.kron(wa, wb)
            want = mu.astype(LD) @ (wa.astype(LD)[:, None] * wb.astype(LD)[None, :]).reshape(-1)
            check("inner mu^T w", "rounding", after["vec"][k, 3 * R + M + 1], want, SA.bound_sum(P + 1, np.abs(mu) @ np.abs(w)))
            assert same(after["WA"][:, k], wa) and same(after["WB"][:, k], wb)
            if a == 1:
                sa, ma = after["Wa"][k, 0].astype(LD) @ wa.astype(LD), float(np.abs(after["Wa"][k, 0]) @ np.abs(wa))
                sb, mb = after["Wb"][k, 0].astype(LD) @ wb.astype(LD), float(np.abs(after["Wb"][k, 0]) @ np.abs(wb))
                ea, eb = SA.bound_sum(A, ma), SA.bound_sum(B, mb)
                bound = (ea * abs(float(sb)) + eb * abs(float(sa)) + ea * eb) * (1 + SA.U) + SA.U * abs(float(sa * sb)) * SA.REF_SLACK
                check("inner g", "rounding", after["vec"][k, 2 * R + M + 1], sa * sb, bound)
    for f in ("mean", "S", "Gy", "fold_of", "T", "Yk", "part", "tm", "Tout", "Gt", "coef", "Rm"):   # what the inner loop never writes
        assert same(after[f], st[f]), f
