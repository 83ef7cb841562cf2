"""tests/resid_rows_ref.py on the CPU: both references against a plain triple loop, the float64 torch reference against the
longdouble one within its own bound, the bound against deliberately wrong results (a row dropped, doubled, swapped with its
neighbour's), the restated plans at the values the GPU tests rely on, and the discrimination condition for every case of the
tables.  No GPU."""
import math

import numpy as np
import pytest
import torch

import resid_rows_ref as RR
import small_algebra_ref as SA

LD = np.longdouble


def _rng(*k):
    return np.random.default_rng(list(k))


@pytest.mark.parametrize("st", RR.STORAGE)
@pytest.mark.parametrize("mean,nan", [(True, 0.0), (False, 0.0), (True, 0.3)])
def test_references_against_a_triple_loop(st, mean, nan):
    I, A, B, R = 7, 2, 3, 2
    X, T, WA, WB, mu = RR.inputs(_rng(1, int(mean), RR.STORAGE.index(st)), I, A, B, R, st, mean, nan_fraction=nan)
    assert T.shape == (I, R + 3) and np.isnan(T[:, R:]).all() and (mu is None) == (not mean)
    if nan:
        X[3] = np.nan                                        # a row with nothing observed
    rows, cols, brows, bcols = RR.reference_ld(X, T[:, :R], WA, WB, mu)
    wr, wc = np.zeros((I, 3)), np.zeros((A * B, 2))
    for i in range(I):
        e2, x2 = [], []
        for j in range(A):
            for k in range(B):
                c = j * B + k
                xc = X[i, c] - (mu[c] if mean else 0.0)
                if math.isfinite(xc):
                    d = xc - math.fsum(T[i, r] * WA[j, r] * WB[k, r] for r in range(R))
                    e2.append(d * d)
                    x2.append(xc * xc)
                    wc[c, 0] += d * d
                    wc[c, 1] += xc * xc
        wr[i] = math.fsum(e2), math.fsum(x2), len(x2)
    np.testing.assert_allclose(rows.astype(np.float64), wr, rtol=1e-13)
    np.testing.assert_allclose(cols.astype(np.float64), wc, rtol=1e-13)
    assert np.array_equal(rows[:, 2].astype(np.float64), wr[:, 2])
    live = wr[:, 2] > 0
    assert np.all(brows[live] > 0) and np.all(brows[live] < 1e-13 * wr[live, :2]) and np.all(bcols > 0)
    if nan:
        assert not rows[3].any() and not brows[3].any()      # nothing observed: sums and bound exactly 0
    # the float64 torch reference, in ragged chunks, against the longdouble one: within its (doubled) bound
    dt = torch.float32 if st == "f32" else torch.float64
    Td = torch.from_numpy(T)[:, :R]
    got = RR.reference_torch(torch.from_numpy(X).to(dt), Td, torch.from_numpy(WA), torch.from_numpy(WB),
                             None if mu is None else torch.from_numpy(mu), chunks=3)
    assert np.array_equal(got[0][:, 2], wr[:, 2])
    assert np.all(np.abs(got[0][:, :2].astype(LD) - rows[:, :2]).astype(np.float64) <= got[2])
    assert np.all(np.abs(got[1].astype(LD) - cols).astype(np.float64) <= got[3])
    np.testing.assert_allclose(got[2], 2.0 * brows, rtol=1e-6, atol=0)
    np.testing.assert_allclose(got[3], 2.0 * bcols, rtol=1e-6)


def test_bound_rejects_wrong_rows():
    """A 300 x 35 case computed in plain float64 NumPy passes; with a row dropped, added twice or swapped with its neighbour's
    sums the error is at least 1000 x the bound somewhere."""
    I, A, B, R = 300, 5, 7, 9
    X, T, WA, WB, mu = RR.inputs(_rng(2), I, A, B, R, "f64", True, nan_fraction=0.05)
    rows, cols, brows, bcols = RR.reference_ld(X, T[:, :R], WA, WB, mu)

    def plain(w=None):
        W = (WA[:, None, :] * WB[None, :, :]).reshape(A * B, R)
        xc = X - mu
        fin = np.isfinite(xc)
        d = np.where(fin, xc - T[:, :R] @ W.T, 0.0)
        x0 = np.where(fin, xc, 0.0)
        w = np.ones(I) if w is None else w
        return np.stack([(d * d).sum(1), (x0 * x0).sum(1)], 1), np.stack([w @ (d * d), w @ (x0 * x0)], 1)

    def ratios(r, c):
        return (np.abs(r.astype(LD) - rows[:, :2]).astype(np.float64) / brows).max(), (np.abs(c.astype(LD) - cols).astype(np.float64) / bcols).max()

    r, c = plain()
    assert max(ratios(r, c)) <= 1.0
    w = np.ones(I)
    w[70] = 0.0
    assert ratios(*plain(w))[1] >= 1000.0                    # row 70 never reached the column sums
    w[70] = 2.0
    assert ratios(*plain(w))[1] >= 1000.0                    # ... reached them twice
    swapped = r.copy()
    swapped[[64, 65]] = swapped[[65, 64]]
    assert ratios(swapped, c)[0] >= 1000.0                   # two lanes exchanged
    stale = r.copy()
    stale[128:136] = stale[64:72]
    assert ratios(stale, c)[0] >= 1000.0                     # a chunk's sums carried into the next


def test_resid_plan_values():
    for name, st, I, A, B, R, misaligned, mean, plan in RR.TALL_CASES:
        assert RR.resid_plan(I, A * B, RR.vec_width(st, B, misaligned)) == plan, (name, st)
    assert RR.vec_width("f32", 65) == 1 and RR.vec_width("f64", 260) == 2 and RR.vec_width("f32", 4, True) == 1
    # every shape of tests/test_gpu_diagnostics.py stays on the floor of 8 rows per block
    assert RR.resid_plan(5000, 48, 4)[:3] == (1, 625, 8) and RR.resid_plan(3000, 1280, 4)[:3] == (2, 375, 8)
    assert RR.resid_plan(65536, 128 * 128, 4) == (16, 128, 512, 512) and RR.chunks_per_block(512) == (8, 64)
    assert [RR.chunks_per_block(n) for n in (9, 21, 65, 70, 201)] == [(1, 9), (1, 21), (2, 1), (2, 6), (4, 9)]
    assert RR.resid_plan(1, 3, 4) == (1, 1, 8, 1) and RR.resid_plan(300, 35, 1) == (1, 38, 8, 4) and RR.resid_plan(257, 48, 2) == (1, 33, 8, 1)
    assert RR.resid_workspace_bytes(64, 64, 1) == RR.resid_workspace_bytes(64, 64, 4) == (64 * 3 + 8 * 64 * 2) * 8
    assert 21 % RR.UNROLL == 1 and RR.SPECIAL_SCORE_ROWS == (416, 390)


def test_contrib_plan_values():
    for (n, A, B, R, st), (g_start, G, lg) in RR.CONTRIB_LDS_CASES:
        got = RR.contrib_plan(n, R, A, B, RR.vec_width(st, B))
        assert RR.contrib_g_start(n) == g_start and got[:2] == (G, lg) and got[3] and got[2] <= 160 * 1024, got
        assert (2 * A * R + 2 * (2 * G) * A + 512 * 4) * 8 > 160 * 1024      # twice the rows would not fit
    for (n, A, B, R), (G, last) in RR.CONTRIB_ODD_G:
        for st in RR.STORAGE:
            got = RR.contrib_plan(n, R, A, B, RR.vec_width(st, B))
            assert got[0] == G and got[3] and n - (-(-n // G) - 1) * G == last
    # the shapes of tests/test_gpu_contributions.py: 3 and 8 rows per workgroup, the LDS limit with one row
    assert RR.contrib_plan(5000, 10, 4, 12, 4)[:2] == (3, 2) and RR.contrib_plan(20003, 10, 16, 16, 4)[:2] == (8, 2)
    assert RR.contrib_plan(6, 16, 542, 4, 4) == (1, 0, (2 * 542 * 17 + 2048) * 8, True) and not RR.contrib_plan(6, 16, 543, 4, 4)[3]
    assert RR.contrib_plan(3000, 10, 8, 160, 4)[1] == 6 and RR.contrib_plan(3000, 10, 8, 160, 2)[1] == 6 and RR.contrib_plan(300, 16, 5, 7, 1)[1] == 3


def test_every_case_meets_the_discrimination_condition():
    worst = {}

    def need(name, m):
        worst[name] = min(worst.get(name, np.inf), m)
        assert m >= 1000.0, (name, m)

    for name, st, I, A, B, R, misaligned, mean, plan in RR.TALL_CASES:         # against reference_torch: the doubled bound
        for n, what in ((A * B, "row"), (I, "column")):
            need(f"{name} {what} e2", RR.margin(n, R, True, RR.D_LO, RR.D_HI, mean))
            need(f"{name} {what} x2", RR.margin(n, R, True, RR.X_LO, RR.X_HI, mean))
    for I, A, B in RR.CHUNK_SHAPES:                                              # against reference_ld
        for n in (A * B, I):
            need("register chunks e2", RR.margin(n, 16, False, RR.D_LO, RR.D_HI))
            need("register chunks x2", RR.margin(n, 16, False, RR.X_LO, RR.X_HI))
    for k, v in sorted(worst.items()):
        print(f"smallest margin {k}: {v:.4g}")
    assert worst["c column e2"] == min(worst.values())
