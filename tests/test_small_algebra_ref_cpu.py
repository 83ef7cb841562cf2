"""tests/small_algebra_ref.py on the CPU: every restatement against an independent formulation (math.fsum per output or an
explicit loop), the bound against deliberately wrong restatements (it has to discriminate: 1000 x on the rounding inputs,
inequality on the exact inputs), and the discrimination condition for every shape that tests/test_gpu_small_algebra_limits.py
runs.  No GPU."""
import math

import numpy as np
import pytest

import small_algebra_ref as SA

KINDS = ["exact", "rounding"]
LD = np.longdouble


def _rng(*k):
    return np.random.default_rng(list(k))


def _fdot(x, y):
    """Exact dot product: every product split error-free (Dekker / fma-free two-product through fractions of 2^-26), then fsum."""
    terms = []
    for a, b in zip(np.asarray(x, dtype=np.float64).tolist(), np.asarray(y, dtype=np.float64).tolist()):
        ah = float(np.float32(a))
        al = a - ah
        bh = float(np.float32(b))
        bl = b - bh
        terms += [ah * bh, ah * bl, al * bh, al * bl]          # 24 x 24, 24 x 29, 29 x 29 bit products: each exact in float64
    return math.fsum(terms)


def _close(val, want, scale):
    """longdouble value against the exact one rounded to float64: half an ulp of it plus the longdouble sum's own 2^-58."""
    return abs(float(LD(val) - LD(want))) <= 2.0 ** -53 * abs(want) + 2.0 ** -58 * scale


# ---- 1. restatements against independent formulations ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_restatements_match_independent_formulations(kind):
    rng = _rng(1, KINDS.index(kind))
    I, a, b, M, R = 11, 3, 2, 4, 3
    A, B = SA.inputs(kind, rng, I, a), SA.inputs(kind, rng, I, b)
    C, mag = SA.gram_tn(A, B)
    for p in range(a):
        for q in range(b):
            assert _close(C[p, q], _fdot(A[:, p], B[:, q]), mag[p, q])
            assert mag[p, q] == pytest.approx(_fdot(np.abs(A[:, p]), np.abs(B[:, q])), rel=1e-14)
    assert SA.gram_tn(A[:, 0], B[:, 1])[0].shape == (1, 1)                 # 1-D operands
    # rowdot
    Y, qv, uo = SA.inputs(kind, rng, I, M), SA.inputs(kind, rng, M), SA.inputs(kind, rng, I)
    u, umag, du2 = SA.rowdot(Y, qv, uo)
    for i in range(I):
        assert _close(u[i], _fdot(Y[i], qv), umag[i])
    want = math.fsum((uo[i] - _fdot(Y[i], qv)) ** 2 for i in range(I))
    assert float(du2) == pytest.approx(want, rel=1e-13)
    assert SA.rowdot(Y, qv)[2] is None
    # y_deflate
    T, bv = SA.inputs(kind, rng, I, R + 2), SA.inputs(kind, rng, R)
    V, ev, ssq = SA.y_deflate(Y, T, R, bv, qv)
    loop = np.array([[Y[i, m] - _fdot(T[i, :R], bv) * qv[m] for m in range(M)] for i in range(I)])
    assert np.allclose(V.astype(np.float64), loop, rtol=1e-13, atol=1e-13) and ev.shape == (I, M) and np.all(ev > 0)
    assert float(ssq) == pytest.approx(math.fsum((loop ** 2).ravel().tolist()), rel=1e-12)
    # sum, scores_mean, axpy_scalar, colscale
    v = SA.inputs(kind, rng, 37)
    assert SA.total(v)[0] == pytest.approx(float(np.sum(v.astype(LD))), abs=1e-13)
    Ts = SA.inputs(kind, rng, 3, 9)
    sm, smag = SA.scores_mean(Ts)
    for i in range(9):
        assert float(sm[i]) == pytest.approx(math.fsum(Ts[:, i].tolist()) / 3.0, abs=1e-15)
        assert SA.scores_mean_f64(Ts)[i] == ((Ts[0, i] + Ts[1, i]) + Ts[2, i]) / 3.0
        assert smag[i] == pytest.approx(np.abs(Ts[:, i]).sum() / 3.0)
    y, al, x = SA.inputs(kind, rng, 9), SA.inputs(kind, rng, 1), SA.inputs(kind, rng, 9)
    assert np.allclose(SA.axpy_scalar(y, al, x)[0].astype(np.float64), [y[i] - al[0] * x[i] for i in range(9)], rtol=1e-15)
    assert np.allclose(SA.axpy_scalar(y, al)[0].astype(np.float64), y - al[0], rtol=1e-15)
    cnt = np.array([0.0, 2, 3, 0, 1, 5, 2, 2, 4])
    cs = SA.colscale(y, cnt, 7.0)
    assert all(cs[i] == (0.0 if cnt[i] == 0 else y[i] / cnt[i] * 7.0) for i in range(9))
    # normalize
    nv, nrm, rel_n, rel_v = SA.normalize(v)
    assert float(nrm) == pytest.approx(math.sqrt(_fdot(v, v)), rel=1e-15) and 0 < rel_n < rel_v < 1e-13
    assert np.allclose(nv.astype(np.float64), v / math.sqrt(_fdot(v, v)), rtol=1e-15)
    if kind == "exact":
        v64, n64 = SA.normalize_f64(v)
        assert n64 == math.sqrt(float(int(_fdot(v, v)))) and np.array_equal(v64, v / n64)
    # kr_gram, kr_gram_row
    L, G0 = SA.inputs(kind, rng, 6, R), SA.inputs(kind, rng, R, R)
    first, bfirst = SA.kr_gram(L, None, True, 3.0)
    mult, bmult = SA.kr_gram(L, G0, False, 0.5)
    for r in range(R):
        for s in range(R):
            d = _fdot(L[:, r], L[:, s])
            assert float(first[r, s]) == pytest.approx(3.0 * d, rel=1e-15, abs=1e-15)
            assert float(mult[r, s]) == pytest.approx(G0[r, s] * 0.5 * d, rel=1e-15, abs=1e-15)
    assert np.all(bfirst > 0) and np.all(bmult[G0 != 0] > 0)
    assert np.all(SA.kr_gram(L, G0, False, 0.5, G_err=1e-3)[1] > bmult)
    g0 = SA.inputs(kind, rng, R)
    row, brow = SA.kr_gram_row(L, 2, g0, False)
    assert [float(t) for t in row] == pytest.approx([g0[j] * _fdot(L[:, j], L[:, 2]) for j in range(2)], rel=1e-15, abs=1e-15)
    assert SA.kr_gram_row(L, 2, g0, True)[0].shape == (2,) and np.all(brow[g0[:2] != 0] > 0)
    # khatri_rao, kron
    Am, Bm = SA.inputs(kind, rng, 3, R), SA.inputs(kind, rng, 4, R)
    kr = SA.khatri_rao(Am, Bm)
    assert all(kr[j * 4 + k, r] == Am[j, r] * Bm[k, r] for j in range(3) for k in range(4) for r in range(R))
    kn = SA.kron(Am[:, 0], Bm[:, 0])
    assert all(kn[j * 4 + k] == Am[j, 0] * Bm[k, 0] for j in range(3) for k in range(4))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("mean,nan", [(True, 0.0), (False, 0.0), (True, 0.3)])
def test_recon_r2_restatement_against_a_loop(kind, mean, nan):
    rng = _rng(2, KINDS.index(kind), int(mean))
    I, A, B, R = 4, 2, 3, 2
    X, T, WA, WB, mu = SA.recon_r2_inputs(kind, rng, I, A, B, R, np.float32, mean, ldt_extra=1, nan_fraction=nan)
    assert T.shape == (I, R + 1) and (mu is None) == (not mean) and np.array_equal(X[np.isfinite(X)], X[np.isfinite(X)].astype(np.float32))
    val, bound = SA.recon_r2(X, T[:, :R], WA, WB, mu)
    res, ssq = [], []
    for i in range(I):
        for c in range(A * B):
            xc = X[i, c] - (mu[c] if mean else 0.0)
            if math.isfinite(xc):
                xhat = math.fsum(T[i, r] * WA[c // B, r] * WB[c % B, r] for r in range(R))
                res.append((xhat - xc) ** 2)
                ssq.append(xc ** 2)
    assert [float(val[0]), float(val[1])] == pytest.approx([math.fsum(res), math.fsum(ssq)], rel=1e-13)
    assert np.all(bound > 0) and np.all(bound < 1e-12 * np.maximum(val.astype(np.float64), 1.0))
    if kind == "exact":
        assert val[0] == val[1] == math.fsum(ssq)
    if nan:
        assert np.isnan(X[-1, -1]) and np.isnan(X[-1, 0]) and np.isnan(X[0, -1])
    want, mag = SA.recon(T[:, :R], WA, WB, mu)
    assert want.shape == mag.shape == (I, A * B)


def test_recon_r2_plan_of_the_ragged_case():
    st, A, B, I, chain = SA.RECON_R2_RAGGED
    assert SA.recon_r2_plan(I, A * B, 2) == (2, 923, 9) and chain == 9 * 2 + 10 + -(-2 * 923 // 8) + 8
    assert SA.recon_r2_plan(9, 650, 2) == (2, 2, 8) and SA.recon_r2_plan(9, 655, 1) == (3, 2, 8)
    assert SA.recon_r2_plan(9, 4160, 4) == (5, 2, 8) and SA.recon_r2_plan(1, 3, 4) == (1, 1, 8)


# ---- 2. the bound discriminates ------------------------------------------------------------------------------------------------------
def _f32_dot(A, B):
    return (A.astype(np.float32).T @ B.astype(np.float32)).astype(np.float64)


def _judge_f32(kind, wrong, want, bound):
    """f32 accumulation: the rounding inputs expose it.  The exact inputs cannot -- integer sums below 2^24 are exact in f32 as
    well -- which is why every GPU case runs both forms."""
    if kind == "rounding":
        _judge(kind, wrong, want, bound)


def _judge(kind, wrong, want, bound):
    """A wrong restatement: unequal on the exact inputs, beyond 1000 x bound somewhere on the rounding inputs."""
    wrong, want = np.asarray(wrong, dtype=np.float64).ravel(), np.asarray(want, dtype=LD).ravel()
    if kind == "exact":
        assert not np.array_equal(wrong, want.astype(np.float64))
    else:
        ratio = (np.abs(wrong.astype(LD) - want).astype(np.float64) / np.broadcast_to(np.asarray(bound, dtype=np.float64).ravel(), wrong.shape)).max()
        assert ratio >= 1000.0, ratio


@pytest.mark.parametrize("kind", KINDS)
def test_bound_rejects_wrong_gram_tn(kind):
    """The four wrong forms on a 2000 x 70 by 2000 x 66 Gram: last row dropped, column 63 (the last of the first 64-wide tile)
    replaced by its neighbour's, the leading dimension taken as the width, f32 accumulation."""
    rng = _rng(3, KINDS.index(kind))
    I, a, b, ld = 2000, 70, 66, 80
    W = SA.inputs(kind, rng, I, ld)
    A, B = W[:, :a], W[:, 8:8 + b]
    want, mag = SA.gram_tn(A, B)
    bound = SA.bound_sum(I, mag)
    good = (A.T @ B)                                                       # float64 BLAS: a right answer in another order
    if kind == "exact":
        assert np.array_equal(good, want.astype(np.float64))
    else:
        assert (np.abs(good.astype(LD) - want).astype(np.float64) / bound).max() <= 1.0
    _judge(kind, A[:-1].T @ B[:-1], want, bound)
    tile = good.copy()
    tile[:, 63] = 0.0                                                      # the tile's last column never accumulated
    _judge(kind, tile, want, bound)
    flat = np.ascontiguousarray(W).ravel()
    _judge(kind, flat[:I * a].reshape(I, a).T @ B, want, bound)            # lda taken as a
    _judge_f32(kind, _f32_dot(A, B), want, bound)


@pytest.mark.parametrize("kind", KINDS)
def test_bound_rejects_wrong_row_kernels(kind):
    """rowdot, y_deflate, scores_mean, axpy_scalar, sum, normalize: last row dropped (left at its old value), the leading
    dimension taken as the width, f32 accumulation."""
    rng = _rng(4, KINDS.index(kind))
    I, M, R = 3000, 16, 7
    Yw, q, Tw, b = SA.inputs(kind, rng, I, M + 3), SA.inputs(kind, rng, M), SA.inputs(kind, rng, I, R + 3), SA.inputs(kind, rng, R)
    Y = Yw[:, :M]
    u, mag, _ = SA.rowdot(Y, q)
    u_old = SA.away_from(kind, rng, u)
    du2 = SA.rowdot(Y, q, u_old)[2]
    bu, bd = SA.bound_sum(M, mag), SA.bound_du2(Y, q, u_old)
    u64 = Y @ q
    _judge(kind, Yw.ravel()[:I * M].reshape(I, M) @ q, u, bu)                                        # ldy taken as M
    _judge_f32(kind, Y.astype(np.float32) @ q.astype(np.float32), u, bu)
    _judge(kind, [np.sum((u_old[:-1] - u64[:-1]) ** 2)], [du2], [bd])                                 # last row dropped
    _judge_f32(kind, [np.sum((u_old - u64).astype(np.float32) ** 2, dtype=np.float32)], [du2], [bd])
    if kind == "rounding":
        assert abs(float(LD(np.sum((u_old - u64) ** 2)) - du2)) <= bd
    # y_deflate
    s = Tw[:, :R].astype(LD) @ b.astype(LD)
    Yd = Yw.copy()
    Yd[:, :M] = SA.away_from(kind, rng, np.outer(s, q.astype(LD)))
    V, ev, ssq = SA.y_deflate(Yd[:, :M], Tw, R, b, q)
    bs = SA.bound_ssq(V, ev)
    v64 = Yd[:, :M] - np.outer(Tw[:, :R] @ b, q)
    if kind == "rounding":
        assert (np.abs(v64.astype(LD) - V).astype(np.float64) / ev).max() <= 1.0 and abs(float(LD(np.sum(v64 ** 2)) - ssq)) <= bs
    dropped = v64.copy()
    dropped[-1] = Yd[-1, :M]
    _judge(kind, dropped, V, ev)
    _judge(kind, [np.sum(v64[:-1] ** 2)], [ssq], [bs])
    _judge(kind, Yd[:, :M] - np.outer(Tw.ravel()[:I * R].reshape(I, R) @ b, q), V, ev)               # ldt taken as R
    _judge_f32(kind, Yd[:, :M] - np.outer((Tw[:, :R].astype(np.float32) @ b.astype(np.float32)).astype(np.float64), q), V, ev)
    # scores_mean, axpy_scalar, sum
    Ts = SA.inputs(kind, rng, 3, I)
    sm, bsm = SA.scores_mean(Ts)[0], SA.bound_scores_mean(Ts)
    _judge(kind, (Ts[0] + Ts[1]) / 3.0, sm, bsm)                                                    # last block dropped
    _judge_f32(kind, (Ts.astype(np.float32).sum(axis=0, dtype=np.float32) / np.float32(3.0)), sm, bsm)
    y, al, x = SA.inputs(kind, rng, I), SA.inputs(kind, rng, 1) + 3.0, SA.inputs(kind, rng, I)
    ax, amag = SA.axpy_scalar(y, al, x)
    last = (y - al[0] * x)
    last[-1] = y[-1]
    _judge(kind, last, ax, SA.bound_sum(2, amag))
    tot, tmag = SA.total(y)
    _judge(kind, [np.sum(y[:-1])], [tot], [SA.bound_sum(I, tmag)])
    _judge_f32(kind, [float(np.sum(y.astype(np.float32), dtype=np.float32))], [tot], [SA.bound_sum(I, tmag)])
    nv, nrm, rel_n, rel_v = SA.normalize(y)
    _judge(kind, [np.linalg.norm(y[:-1])], [nrm], [rel_n * float(nrm)])
    if kind == "rounding":
        assert abs(float(LD(np.linalg.norm(y)) - nrm)) <= rel_n * float(nrm)
        assert (np.abs((y / np.linalg.norm(y)).astype(LD) - nv).astype(np.float64) <= rel_v * np.abs(nv.astype(np.float64))).all()


@pytest.mark.parametrize("kind", KINDS)
def test_bound_rejects_wrong_kr_gram_and_recon_r2(kind):
    rng = _rng(5, KINDS.index(kind))
    n, R = 130, 70
    Lw = SA.inputs(kind, rng, n, R + 2)
    L = np.ascontiguousarray(Lw[:, :R])
    G1, b1 = SA.kr_gram(L, None, True, 3.0)
    good = 3.0 * (L.T @ L)
    if kind == "rounding":
        assert (np.abs(good.astype(LD) - G1).astype(np.float64) / b1).max() <= 1.0
    _judge(kind, 3.0 * (L[:-1].T @ L[:-1]), G1, b1)                                               # last row dropped
    cut = good.copy()
    cut[:, 63] = cut[:, 62]
    _judge(kind, cut, G1, b1)                                                                     # a 64-wide tile's last column
    wide = Lw.ravel()[:n * R].reshape(n, R)
    _judge(kind, 3.0 * (wide.T @ wide), G1, b1)                                                   # ld taken as R
    _judge_f32(kind, 3.0 * _f32_dot(L, L), G1, b1)
    G2, b2 = SA.kr_gram(L, G1.astype(np.float64), False, 1.0, G_err=b1 + SA.U * np.abs(G1.astype(np.float64)))
    if kind == "rounding":
        assert (np.abs(((good * 1.0) * (L.T @ L)).astype(LD) - G2).astype(np.float64) / b2).max() <= 1.0
    _judge(kind, good * (L[:-1].T @ L[:-1]), G2, b2)
    g0 = SA.inputs(kind, rng, R)
    row, brow = SA.kr_gram_row(L, R - 1, g0, False)
    if kind == "rounding":
        assert (np.abs((g0[:R - 1] * (L[:, :R - 1].T @ L[:, R - 1])).astype(LD) - row).astype(np.float64) / brow).max() <= 1.0
    _judge(kind, g0[:R - 1] * (L[:-1, :R - 1].T @ L[:-1, R - 1]), row, brow)
    _judge(kind, g0[:R - 1] * (wide[:, :R - 1].T @ wide[:, R - 1]), row, brow)
    # recon_r2: f64 5 x 130 with 9 rows
    I, A, B, Rr = 9, 5, 130, 5
    X, T, WA, WB, mu = SA.recon_r2_inputs(kind, rng, I, A, B, Rr, np.float64, True, ldt_extra=2, nan_fraction=0.1)
    val, bound = SA.recon_r2(X, T[:, :Rr], WA, WB, mu)

    def plain(Xp, Tp, dtype=np.float64):
        W = (WA[:, None, :] * WB[None, :, :]).reshape(A * B, Rr).astype(dtype)
        xc = (Xp - mu).astype(dtype)
        d = Tp.astype(dtype) @ W.T - xc
        fin = np.isfinite(xc)
        return np.array([np.sum(d[fin] ** 2), np.sum(xc[fin] ** 2)], dtype=np.float64)

    if kind == "rounding":
        assert (np.abs(plain(X, T[:, :Rr]).astype(LD) - val).astype(np.float64) / bound).max() <= 1.0
    else:
        assert np.array_equal(plain(X, T[:, :Rr]), val.astype(np.float64))
    _judge(kind, plain(X[:-1], T[:-1, :Rr]), val, bound)                                          # last row dropped
    _judge(kind, plain(np.where(np.arange(A * B) == A * B - 2, np.nan, X), T[:, :Rr]), val, bound)   # a live column of the last tile
    if kind == "rounding":                                                                        # (exact form: T = 0, any ldt reads zeros)
        _judge(kind, plain(X, T.ravel()[:I * Rr].reshape(I, Rr)), val, bound)                     # ldt taken as R
    _judge_f32(kind, plain(X, T[:, :Rr], np.float32), val, bound)


# ---- 3. the discrimination condition for every shape of the GPU tests ---------------------------------------------------------------
def _two_level_margin(chain, n, lo, hi, e):
    """min square / bound of a sum of n squares of values of magnitude in [lo, hi] known to within e (bound_two_level)."""
    return lo * lo / (n * (2 * hi * e + e * e) + SA.gamma(chain) * n * (hi + e) ** 2)


def test_every_listed_shape_meets_the_discrimination_condition():
    lo, hi, U = SA.LO, SA.HI, SA.U
    p_lo, p_hi = lo * lo, hi * hi                          # a product of two rounding inputs
    worst = {}

    def need(name, margin):
        worst[name] = min(worst.get(name, np.inf), margin)
        assert margin >= 1000.0, (name, margin)

    for I, a in SA.GEMV_CASES:
        need("gram_tn gemv", SA.term_margin(I, I, p_lo, p_hi))
    assert {I for I, _ in SA.GEMV_CASES} == set(SA.GEMV_I) and {a for _, a in SA.GEMV_CASES} == set(SA.GEMV_A)
    for I in SA.TILED_I:
        need("gram_tn tiled", SA.term_margin(I, I, p_lo, p_hi))
    for a, b in SA.TILED_AB:
        ca, cb = SA.tiled_columns(a, b)
        assert 0 <= ca and ca + a <= SA.TILED_WIDTH and 0 <= cb and cb + b <= SA.TILED_WIDTH
    for I, M in SA.ROWDOT_CASES:
        need("rowdot u", SA.term_margin(M, M, p_lo, p_hi))
        bu = SA.gamma(M) * M * p_hi
        need("rowdot du2", _two_level_margin(I, I, lo, hi * 1.001, bu + U * (hi + bu)))
    for I, M, R, chain in SA.Y_DEFLATE_CASES:
        bs = SA.gamma(R) * R * p_hi
        y_hi = R * p_hi * hi + hi
        ev = bs * hi + U * y_hi + 2.01 * U * (R * p_hi + bs) * hi
        need("y_deflate Y", lo / ev)                       # an element of Y: the step it differs from (T b) q by, against ev
        n = I * M
        plain = _two_level_margin(n, n, lo * 0.999, hi * 1.001, ev)
        if chain is None:
            need("y_deflate ssq", plain)
        else:                                              # the case says why it carries a chain: n terms must really miss
            assert plain < 1000.0 and chain < n
            need("y_deflate ssq", _two_level_margin(chain, n, lo * 0.999, hi * 1.001, ev))
    for n in SA.SUM_N:
        need("sum", SA.term_margin(n, n, lo, hi))
    for n in SA.NORMALIZE_N:
        need("normalize", SA.term_margin(n, n, p_lo, p_hi))
    for nb, I in SA.SCORES_MEAN_CASES:
        need("scores_mean", lo / nb / (SA.gamma(nb) * hi * 1.01 + U * hi))
    need("axpy_scalar", SA.term_margin(2, 2, p_lo, hi + p_hi))
    for n, R in SA.KR_GRAM_CASES:
        need("kr_gram", SA.term_margin(n + 2, n + 2, p_lo, p_hi) / 1.01)
    for n, R, a in SA.KR_GRAM_ROW_CASES:
        need("kr_gram_row", SA.term_margin(n + 1, n, p_lo, p_hi) / 1.01)
        assert 0 <= a < R
    d_lo, d_hi = SA.RECON_R2_TERMS
    for st, A, B, I, chain in SA.RECON_R2_SHAPES + [SA.RECON_R2_RAGGED]:
        n = I * A * B
        e = SA.gamma(17) * 0.85 * 1.01 + 4 * U * 3.35       # xhat to gamma_(R+1) of at most 0.85, two subtractions
        plain = _two_level_margin(n, n, math.sqrt(d_lo), math.sqrt(d_hi), e)
        if chain is None:
            need("recon_r2", plain)
        else:
            assert plain < 1000.0 and chain < n
            need("recon_r2", _two_level_margin(chain, n, math.sqrt(d_lo), math.sqrt(d_hi), e))
    for k, v in sorted(worst.items()):
        print(f"smallest margin {k}: {v:.3g}")
    assert max(SA.EXACT_LIMITS.values()) < 2 ** 53
