"""tests/kfold_epilogue_ref.py checked on its own, no GPU: the restated stages chained over R = 3 components against a literal
computation per model, the tile arithmetic, the written-field masks, and the conditions the GPU file's inputs have to meet.

The chain: random X (I x A x B), Y, a fold map, and ARBITRARY unit loadings wA, wB and q per component and model (the identities
hold for any w and q, so no inner loop is run).  Stage 0; then per component sc = X_0 w, stage 1, rs = X_0^T tm, stage 2.  The
literal computation per model, on its centred training rows (a weighted model: row i repeated c_i times): t = X_a w,
b = lstsq(T_train, Y_a q), Y_{a+1} = Y_a - (T b) q^T, X_{a+1} = X_a - t w^T, S_{a+1} = X_{a+1,train}^T Y_{a+1,train}.
Tolerance 1e-10 relative (normwise), the project's level for float64 against the oracle."""
import numpy as np
import pytest

import kfold_epilogue_ref as KE
import solve_ref as SR

TOL = 1e-10
I, A, B, M, R = 300, 5, 7, 3, 3      # two row tiles of 150


def _rel(got, want):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - want) / max(np.linalg.norm(want), 1e-300))


def _unit(rng, *shape):
    v = rng.normal(size=shape)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


@pytest.mark.parametrize("mode", KE.MODES)
def test_chained_stages_match_literal_refits(mode):
    rng = np.random.default_rng([31, KE.MODES.index(mode)])
    P = A * B
    X = rng.normal(size=(I, P)) + 0.5
    Y0 = rng.normal(size=(I, M)) @ rng.normal(size=(M, M)) + X[:, :M]
    lay, fold_of = KE.layout(mode, "shuffled", I, 3, rng)
    n = KE.models_of(mode, 3)[0]
    groups = 2 if mode == KE.GROUPED else 1
    Ys = [Y0] + [Y0[rng.permutation(I)] for _ in range(groups - 1)]              # grouped: group p is fitted to Y[pi_p]
    mean_rows = n // 2 if mode == KE.GROUPED else n
    st = KE.empty_state(n, I, M, R, A, B, lay.slots, fold_of, mean_rows=mean_rows)
    st["Tout"][:] = 0.0
    lit = []                                                                      # per model: the literal X_a, Y_a (all rows), T
    for k in range(n):
        train, w = KE.training(lay, fold_of, k)
        rep = np.repeat(np.arange(I), w.astype(int))                              # the training rows, row i c_i times
        Yk = Ys[k % groups] if mode == KE.GROUPED else Y0
        mu, nu = X[rep].mean(axis=0), Yk[rep].mean(axis=0)
        Xc, Yc = X - mu, Yk - nu
        st["mean"][lay.model_fold[k] if mode == KE.GROUPED else k] = mu
        st["S"][k] = Yc[rep].T @ Xc[rep]
        st["Yk"][k] = Yc if mode == KE.WEIGHTED else np.where(train[:, None], Yc, 0.0)
        lit.append({"X": Xc, "Y": Yc, "rep": rep, "T": np.zeros((I, 0))})
    KE.apply_ydefl(st, KE.ydefl(lay, st, 0, 0))
    for k in range(n):
        rep = lit[k]["rep"]
        assert _rel(st["Gy"][k].sum(axis=0), lit[k]["Y"][rep].T @ lit[k]["Y"][rep]) <= TOL
    for a in range(R):
        wa, wb, q = _unit(rng, n, A), _unit(rng, n, B), _unit(rng, n, M)
        st["Wa"][:, a], st["Wb"][:, a], st["Q"][:, a] = wa, wb, q
        W = np.stack([np.kron(wa[k], wb[k]) for k in range(n)])                   # n x P
        for k in range(n):
            st["vec"][k, 3 * R + M + 1] = st["mean"][lay.model_fold[k] if mode == KE.GROUPED else k] @ W[k]
            st["vec"][k, 2 * R + M + 1:2 * R + M + 1 + a] = [(st["Wa"][k, j] @ wa[k]) * (st["Wb"][k, j] @ wb[k]) for j in range(a)]
        sc = X @ W.T
        KE.apply_rows(st, a, KE.rows(lay, st, a, sc))
        sv = KE.solve(st, a)
        KE.apply_solve(st, a, sv)
        assert not st["status"].any() and not any(sv["dropped"])
        assert [r.dropped for r in sv["ref"]] == sv["dropped"]
        if a + 1 < R:
            KE.apply_ydefl(st, KE.ydefl(lay, st, a, 1))
        rs = st["tm"].T @ X
        KE.apply_downdate(st, a, KE.downdate(lay, st, a, rs))
        for k in range(n):
            L = lit[k]
            train, w = KE.training(lay, fold_of, k)
            rep = L["rep"]
            t = L["X"] @ W[k]
            L["T"] = np.concatenate([L["T"], t[:, None]], axis=1)
            b = np.linalg.lstsq(L["T"][rep], L["Y"][rep] @ q[k], rcond=None)[0]
            L["Y"] = L["Y"] - np.outer(L["T"] @ b, q[k])
            L["X"] = L["X"] - np.outer(t, W[k])
            errs = {"T": _rel(st["T"][k][:, a], t), "coef": _rel(st["coef"][k][:a + 1, a], b),
                    "tm": _rel(st["tm"][:, k], w * t), "S": _rel(st["S"][k], L["Y"][rep].T @ L["X"][rep]),
                    "Gt": _rel(st["Gt"][k][:a + 1, :a + 1], L["T"][rep].T @ L["T"][rep])}
            if a + 1 < R:
                errs["Yk"] = _rel(st["Yk"][k][train], L["Y"][train])
                errs["Gy"] = _rel(st["Gy"][k].sum(axis=0), L["Y"][rep].T @ L["Y"][rep])
            slot = KE.tout_slot(lay, k)
            if slot is not None:
                errs["Tout"] = _rel(st["Tout"][slot, ~train, a], t[~train])
            assert max(errs.values()) <= TOL, (mode, a, k, errs)
    if mode in (KE.PLAIN, KE.SPLITS, KE.GROUPED):                                  # every slot's every row written exactly once
        assert np.all(st["Tout"] != 0.0)


def test_tile_arithmetic():
    """kf_tiles and kf_tile_rows as pure arithmetic: ceil(I / 256) tiles up to 128, ceil(I / NT) rows each, a ragged last tile,
    none empty; 193 doubles of partial sums per tile (what HipBackend.kfold_row_tiles reports)."""
    assert KE.PART_STRIDE == 193
    want = {5: [5], 257: [129, 128], 777: [195, 195, 195, 192], 300: [150, 150], 600: [200, 200, 200], 256: [256], 3001: [251] * 11 + [240]}
    for i, lens in want.items():
        assert [hi - lo for lo, hi in KE.tile_rows(i)] == lens, i
    for i, (ln, last) in {32768: (256, 256), 32769: (257, 130), 70001: (547, 532)}.items():
        tiles = KE.tile_rows(i)
        assert len(tiles) == KE.kf_tiles(i) == 128 and tiles[0][1] == ln and tiles[-1][1] - tiles[-1][0] == last
    for i in list(range(1, 1200)) + [32767, 32768, 32769, 32770, 40000, 65535, 70001, 1 << 20]:
        tiles = KE.tile_rows(i)
        assert len(tiles) == min(128, -(-i // 256)) and tiles[0][0] == 0 and tiles[-1][1] == i
        assert all(lo < hi for lo, hi in tiles) and all(tiles[j][1] == tiles[j + 1][0] for j in range(len(tiles) - 1))
    # I = 32769 with contiguous folds: tiles 0 - 62 hold no training row of model 0
    f = KE.fold_map("contiguous", 32769, 2, np.random.default_rng(0))
    assert all((f[lo:hi] == 0).all() for lo, hi in KE.tile_rows(32769)[:63])


def _changed(before, after):
    return {f: before[f].view(np.int64 if before[f].dtype == np.float64 else np.int32) !=
            after[f].view(np.int64 if after[f].dtype == np.float64 else np.int32) for f in before}


@pytest.mark.parametrize("mode", KE.MODES)
@pytest.mark.parametrize("a", [0, 1, 2])
def test_written_masks_are_exactly_what_a_stage_writes(mode, a):
    """Each stage applied to a sentinel-filled copy: every changed element is inside the mask, and every element of the mask has
    left the sentinel (status apart: it is only ORed)."""
    lay, st, sc, _ = KE.row_state("rounding", mode, "shuffled", 300, 2, 3, 3, a)
    R = 3
    before = KE.copy_state(st)
    KE.apply_rows(st, a, KE.rows(lay, st, a, sc))
    KE.apply_solve(st, a, KE.solve(st, a))
    if a + 1 < R:
        KE.apply_ydefl(st, KE.ydefl(lay, st, a, 1))
    masks, ch = KE.written(1, lay, st, a), _changed(before, st)
    for f in st:
        m = masks.get(f, np.zeros(st[f].shape, dtype=bool))
        assert not ch[f][~m].any(), f
        if f not in ("status", "Yk"):
            assert np.all(st[f][m] != KE.SENTINEL), f
    assert masks["Tout"].sum() == (0 if mode == KE.WEIGHTED else lay.slots * 300)   # a partition per slot
    st0 = KE.copy_state(before)
    KE.apply_ydefl(st0, KE.ydefl(lay, st0, a, 0))
    ch0 = _changed(before, st0)
    assert [f for f in st0 if ch0[f].any()] == ["Gy"] and ch0["Gy"].all() and KE.written(0, lay, st0, a)["Gy"].all()


@pytest.mark.parametrize("grouped", [False, True])
def test_downdate_mask(grouped):
    lay, st, rs = KE.downdate_state("rounding", grouped, 3, 4, 2, 4, 1)
    before = KE.copy_state(st)
    KE.apply_downdate(st, 1, KE.downdate(lay, st, 1, rs))
    masks, ch = KE.written(2, lay, st, 1), _changed(before, st)
    for f in st:
        m = masks.get(f, np.zeros(st[f].shape, dtype=bool))
        assert not ch[f][~m].any() and ch[f][m].all(), f


def test_downdate_reads_the_held_out_folds_mean():
    lay, st, rs = KE.downdate_state("exact", True, 3, 4, 2, 4, 0)
    out = KE.downdate(lay, st, 0, rs)
    for k in range(4):
        assert np.array_equal(out["Rm"][k].astype(np.float64), rs[k] - st["vec"][k, 2 * 4 + 2] * st["mean"][k // 2])


@pytest.mark.parametrize("case", KE.row_stage_cases(), ids=lambda c: "-".join(str(x) for x in c))
def test_gpu_row_cases_meet_their_conditions(case):
    """For every case of tests/test_gpu_kfold_epilogue_stages.py: on the rounding inputs the restated solve's pivots are far
    from the drop threshold (solve_ref.assert_pivot_margins) and the serial float64 form drops the same columns (none, but the
    exactly zero columns of a model with fewer training rows than columns); on the
    exact inputs the training Gram is exactly diagonal and, where the builder says so, a power of 4 on the non-zero columns."""
    i, m, k, r, a, mode, mp = case
    lay, st, sc, _ = KE.row_state("rounding", mode, mp, i, m, k, r, a)
    n = st["Yk"].shape[0]
    assert 2 <= n <= 32 and m <= 64 and r <= 64 and i >= n                        # the device form
    KE.apply_rows(st, a, KE.rows(lay, st, a, sc))
    sv = KE.solve(st, a)
    for km, (ref, dropped) in enumerate(zip(sv["ref"], sv["dropped"])):
        SR.assert_pivot_margins(ref)
        ntr = int(KE.training(lay, st["fold_of"], km)[0].sum())                    # the model's own training rows
        assert ref.dropped == dropped == list(range(ntr, a + 1)), (km, ntr, dropped)
    assert not sv["bad"].any()
    lay, st, sc, solve_exact = KE.row_state("exact", mode, mp, i, m, k, r, a)
    out = KE.rows(lay, st, a, sc)
    assert np.array_equal(out["part"], out["part"].astype(np.float64))            # nothing was rounded on the way
    KE.apply_rows(st, a, out)
    sv = KE.solve(st, a)
    for kk_, G in enumerate(sv["G"]):
        d = np.diagonal(G)
        assert np.array_equal(G, np.diag(d))
        if solve_exact:
            assert all(x == 0 or np.log2(x) % 2 == 0 for x in d), (kk_, d)
            assert np.array_equal(sv["b_serial"][kk_], sv["ref"][kk_].b.astype(np.float64))
