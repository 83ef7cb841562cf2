"""The 16-bit forms of the three S builders of the resampling passes -- cmtfpls_kfold_xcov_{bf16,f16},
cmtfpls_kfold_wide_xcov_{bf16,f16}, cmtfpls_kfold_weighted_xcov_{bf16,f16} -- against the _f32 entry on the upcast values (bit for
bit) and against NumPy float64 written out per model (a derived bound).

Shapes, each the smallest that reaches its path.  (I, K): (37, 3) ragged folds below one 16-row trip, (700, 5) two row chunks per
fold, (70, 32) K at its limit.  (A, B): (5, 6) P = 30 scalar path with one partial wavefront, (8, 8) P = 64 vector path, (13, 20)
P = 260 vector path with a 4-column tail wavefront, (1, 257) a matrix block on the scalar path, and (8, 8) as a view one element
into a larger buffer: P % 4 == 0 with a base that is only 2-byte aligned, which must take the scalar path.  M of kfold_xcov: 1, 9,
17, 33 (the four MT instances); W of the wide entry: 3, 64, 65, 130 (nyb 1 / 1 / 2 / 3); n x (M + 1) of the weighted entry: 2 x 2,
32 x 4, 15 x 65 (W = 975), count columns summing to I with some counts 0.

The float64 bound (test_against_numpy_float64).  A 16-bit element enters the arithmetic exactly (to_f64), so only the float64 sums
err.  The kernels build, per column c and response m, the per-fold sums P_f = sum_{i in fold f} x_ic y_im in row chunks of
sequential fma (each product rounded once with its addition), add the chunk partials of a fold and then the K fold totals
t = sum_f P_f, and return S_k = (t - P_k) - n_k mu_kc ydev_km with mu_kc = (colsum_c - colsum_kc) / n_k.  A product x_ic y_im
passes through the additions of its chunk chain, of its fold's chunk partials and of the fold totals -- at most I + K in all, since
a fold that has several chunks has correspondingly shorter chains -- then the subtraction t - P_k and the final subtraction: at
most I + K + 2 roundings.  The correction term n_k mu ydev carries the division, two products and the roundings of mu's own sum,
which is the same chain on x_ic * 1.  With gamma_n = n u / (1 - n u), u = 2^-53 (Higham, Accuracy and Stability, Lemma 3.1):

    |S_k[m, c] - exact| <= gamma_{I+K+4} (2 sum_i |x_ic| |y_im| + n_k |mu_kc| |ydev_km|)

(2 sum_i: the all-rows total t and the own-fold total P_k are both bounded by the sum over all rows).  The same chain gives
|mean_k[c] - exact| <= gamma_{I+K+4} 2 sum_i |x_ic| / n_k, |stats[c] - exact| <= gamma_{I+K+4} sum_i |x_ic| and
|stats[P + c] - exact| <= gamma_{I+K+4} sum_i x_ic^2.  The weighted entry is the one-fold case without all-minus-own and without
the correction: S_b[m, c] within gamma_{I+1+4} 2 sum_i |x_ic| |y''_i|, its mean within gamma_{I+1+4} 2 sum_i c_bi |x_ic| / I.
Worst error / bound measured on MI355X: DESIGN 8w ("Resampling").
"""
import numpy as np
import pytest
import torch

import half_storage_ref as HS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -53
IK = [(37, 3), (700, 5), (70, 32)]
AB = [(5, 6, False), (8, 8, False), (13, 20, False), (1, 257, False), (8, 8, True)]          # (A, B, shifted view)
WIDTHS = {"kfold_xcov": [1, 9, 17, 33], "kfold_wide_xcov": [3, 64, 65, 130], "kfold_weighted_xcov": [(2, 1), (32, 3), (15, 64)]}
BUILDERS = list(WIDTHS)
_cache = {}


def _gamma(n):
    return n * U / (1.0 - n * U)


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()
    torch.cuda.empty_cache()


def _dev(a, dt=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)


def _x16(I, P, q, shifted):
    """The quantised block on the device as I x P: its own allocation, or a view one element into a larger buffer."""
    if not shifted:
        return q.reshape(I, P).to(DEV).contiguous()
    buf = torch.zeros(I * P + 8, dtype=q.dtype, device=DEV)
    buf[1:1 + I * P] = q.reshape(-1).to(DEV)
    X = buf[1:1 + I * P].view(I, P)
    assert X.data_ptr() % 8 == 2 and X.is_contiguous()
    return X


def _folds(rng, I, K):
    ids = rng.permutation(np.arange(I) % K)
    ids[:3] = 0                                                   # ragged
    order = np.argsort(ids, kind="stable").astype(np.int32)
    off = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=K))]).astype(np.int32)
    return ids, order, off


def _counts(rng, n, I):
    C = np.stack([np.bincount(rng.integers(0, I, size=I), minlength=I) for _ in range(n)]).astype(np.float64)
    assert np.all(C.sum(axis=1) == I) and np.any(C == 0)
    return C


def _build(be, builder, X2, A, B, args):
    """One call of the builder's backend method on X2 (any storage type): (S, mean, stats) as host arrays."""
    P = A * B
    if builder == "kfold_weighted_xcov":
        Yw, n, M = args
        S, mean = torch.full((n, M, P), 7.0, device=DEV, dtype=torch.float64), torch.full((n, P), 7.0, device=DEV, dtype=torch.float64)
        stats = be.kfold_weighted_xcov(X2, A, B, Yw, n, M, S, mean)
    else:
        Y, order, off, K, ydev = args
        W = Y.shape[1]
        S, mean = torch.full((K, W, P), 7.0, device=DEV, dtype=torch.float64), torch.full((K, P), 7.0, device=DEV, dtype=torch.float64)
        stats = getattr(be, builder)(X2, A, B, Y, order, off, K, ydev, S, mean)
    assert stats is not None
    torch.cuda.synchronize()
    return S.cpu().numpy(), mean.cpu().numpy(), stats.cpu().numpy()


def _reference(builder, up, host):
    """NumPy float64 on the upcast values, per model, and the bound of each output (module docstring)."""
    I, P = up.shape
    ax = np.abs(up)
    if builder == "kfold_weighted_xcov":
        Yw, n, M, C = host
        g = _gamma(I + 1 + 4)
        S = np.stack([np.stack([up.T @ Yw[:, b * M + m] for m in range(M)]) for b in range(n)])
        bS = np.stack([np.stack([g * 2.0 * (ax.T @ np.abs(Yw[:, b * M + m])) for m in range(M)]) for b in range(n)])
        mean = np.stack([up.T @ C[b] / I for b in range(n)])
        bmean = np.stack([g * 2.0 * (ax.T @ C[b]) / I for b in range(n)])
    else:
        Y, ids, K, ydev = host
        W = Y.shape[1]
        g = _gamma(I + K + 4)
        S, bS, mean, bmean = np.empty((K, W, P)), np.empty((K, W, P)), np.empty((K, P)), np.empty((K, P))
        mag = np.abs(Y).T @ ax                                                       # sum_i |x_ic| |y_im| over all rows
        for k in range(K):
            train = ids != k
            nk = int(train.sum())
            mu = up[train].mean(axis=0)
            S[k] = (Y[train] - ydev[k]).T @ (up[train] - mu)                         # X_c[train_k]^T (Y[train_k] - nu_k)
            mean[k] = mu
            bS[k] = g * (2.0 * mag + nk * np.abs(ydev[k])[:, None] * np.abs(mu)[None, :])
            bmean[k] = g * 2.0 * ax.sum(axis=0) / nk
    stats = np.concatenate([up.sum(axis=0), (up * up).sum(axis=0)])
    bstats = g * np.concatenate([ax.sum(axis=0), (up * up).sum(axis=0)])
    return (S, mean, stats), (bS, bmean, bstats)


def _cases(be, builder, kind, ik):
    """Every (A, B) x width of one (builder, kind, (I, K)): the 16-bit call twice, the _f32 call on the upcast, the float64
    reference -- computed once, shared by the bitwise and the float64 test."""
    key = (builder, kind, ik)
    if key in _cache:
        return _cache[key]
    I, K = ik
    out = []
    for a, (A, B, shifted) in enumerate(AB):
        P = A * B
        for w, width in enumerate(WIDTHS[builder]):
            rng = np.random.default_rng(1000 * IK.index(ik) + 10 * a + w)
            q, up = HS.quantise(rng.normal(0.3, 1.0, size=(I, P)), kind)
            X16 = _x16(I, P, q, shifted)
            keep = X16.view(torch.int16).clone()
            X32 = X16.to(torch.float32)
            assert np.array_equal(X32.double().cpu().numpy(), up)
            if builder == "kfold_weighted_xcov":
                n, M = width
                Y = rng.normal(size=(I, M))
                C = _counts(rng, n, I)
                nu = (C @ Y) / I
                Yw = np.concatenate([C[b][:, None] * (Y - nu[b]) for b in range(n)] + [C.T], axis=1)
                args, host = (_dev(Yw), n, M), (Yw, n, M, C)
            else:
                ids, order, off = _folds(rng, I, K)
                Y = rng.normal(size=(I, width))
                Y -= Y.mean(axis=0)
                ydev = np.stack([Y[ids != k].mean(axis=0) for k in range(K)])
                args, host = (_dev(Y), _dev(order, torch.int32), _dev(off, torch.int32), K, _dev(ydev)), (Y, ids, K, ydev)
            got = _build(be, builder, X16, A, B, args)
            again = _build(be, builder, X16, A, B, args)
            f32 = _build(be, builder, X32, A, B, args)
            want, bound = _reference(builder, up, host)
            out.append({"shape": (I, K, A, B, shifted, width), "got": got, "again": again, "f32": f32, "want": want, "bound": bound,
                        "unchanged": bool(torch.equal(X16.view(torch.int16), keep))})
    _cache[key] = out
    return out


@pytest.mark.parametrize("ik", IK, ids=lambda v: f"I{v[0]}K{v[1]}")
@pytest.mark.parametrize("kind", HS.KINDS)
@pytest.mark.parametrize("builder", BUILDERS)
def test_bits_of_the_f32_entry_on_the_upcast(be, builder, kind, ik):
    for c in _cases(be, builder, kind, ik):
        for name, g, a, f in zip(("S", "mean", "stats"), c["got"], c["again"], c["f32"]):
            assert np.array_equal(g, f), f"{builder}_{kind} {c['shape']}: {name} differs from the _f32 entry on the upcast values"
            assert np.array_equal(g, a), f"{builder}_{kind} {c['shape']}: {name} differs between two calls"
        assert c["unchanged"], f"{builder}_{kind} {c['shape']}: X was written"


@pytest.mark.parametrize("ik", IK, ids=lambda v: f"I{v[0]}K{v[1]}")
@pytest.mark.parametrize("kind", HS.KINDS)
@pytest.mark.parametrize("builder", BUILDERS)
def test_against_numpy_float64(be, builder, kind, ik):
    worst = (0.0, None, None)
    for c in _cases(be, builder, kind, ik):
        for name, g, w, b in zip(("S", "mean", "stats"), c["got"], c["want"], c["bound"]):
            assert np.all(np.isfinite(g)) and g.shape == w.shape
            ratio = float((np.abs(g - w) / np.maximum(b, 1e-300)).max())
            if ratio > worst[0]:
                worst = (ratio, name, c["shape"])
    print(f"cmtfpls_{builder}_{kind} I, K = {ik}: worst error / bound {worst[0]:.3g} ({worst[1]} at {worst[2]})")
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize("kind,value", [("bf16", float("nan")), ("f16", float("nan")), ("f16", float("inf"))])
@pytest.mark.parametrize("builder", BUILDERS)
def test_nan_and_inf_reach_the_statistics(be, builder, kind, value):
    I, K, A, B = 37, 3, 5, 6
    rng = np.random.default_rng(3)
    q, _ = HS.quantise(rng.normal(size=(I, A * B)), kind)
    q[11, 7] = value
    X16 = q.to(DEV)
    if builder == "kfold_weighted_xcov":
        n, M = 2, 1
        C = _counts(rng, n, I)
        args = (_dev(np.concatenate([C.T * rng.normal(size=(I, 1)), C.T], axis=1)), n, M)
    else:
        _, order, off = _folds(rng, I, K)
        args = (_dev(rng.normal(size=(I, 3))), _dev(order, torch.int32), _dev(off, torch.int32), K, _dev(np.zeros((K, 3))))
    _, _, stats = _build(be, builder, X16, A, B, args)
    bad = ~np.isfinite(stats)
    assert bad[7] and bad[A * B + 7], stats                       # the column's sum and its sum of squares
    assert np.all(np.isfinite(np.delete(stats, [7, A * B + 7])))  # and only that column's


def _raw(lib, builder, suffix, X, I, A, B, Y, width, order, off, K, ydev, S, mean, stats, ws, ws_bytes):
    """The C entry itself (its status, nothing checked): kfold_xcov / kfold_wide_xcov take (order, off, K, ydev), the weighted
    entry width = (n, M)."""
    fn = getattr(lib, f"cmtfpls_{builder}_{suffix}")

    def p(t):
        return None if t is None else t.data_ptr()

    if builder == "kfold_weighted_xcov":
        n, M = width
        return fn(p(X), I, A, B, p(Y), n, M, p(S), p(mean), p(stats), p(ws), ws_bytes, None)
    return fn(p(X), I, A, B, p(Y), width, p(order), p(off), K, p(ydev), p(S), p(mean), p(stats), p(ws), ws_bytes, None)


@pytest.mark.parametrize("kind", HS.KINDS)
@pytest.mark.parametrize("builder", BUILDERS)
def test_declines_as_the_f32_entry_and_writes_nothing(be, builder, kind):
    lib = be.lib
    I, A, B = 70, 8, 8
    P = A * B
    weighted = builder == "kfold_weighted_xcov"
    q, _ = HS.quantise(np.random.default_rng(9).normal(size=(I, P)), kind)
    X16 = q.to(DEV)
    X32 = X16.to(torch.float32)
    good = (2, 1) if weighted else 3
    ws_fn = getattr(lib, f"cmtfpls_{builder}_workspace_bytes")
    # W = 1025: n (M + 1) = 25 * 41 of the weighted entry; kfold_xcov has no W, M = 1025 is beyond its M <= 64 likewise
    cases = {"K = 1": dict(K=1), "K = 33": dict(K=33, width=(33, 1) if weighted else good),
             "W = 1025": dict(width=(25, 40) if weighted else 1025), "workspace one byte short": dict(short=1), "null X": dict(null=True)}
    if weighted:
        del cases["K = 1"]                                        # the weighted entry has no fold count; n = 33 is its K = 33
    seen = {}
    for name, c in cases.items():
        K, width = c.get("K", 5), c.get("width", good)
        models, resp = (width[0], width[1]) if weighted else (K, width)
        cols = models * (resp + 1) if weighted else width
        Y = torch.zeros(I, cols, device=DEV, dtype=torch.float64)
        order, off = torch.arange(I, device=DEV, dtype=torch.int32), torch.zeros(40, device=DEV, dtype=torch.int32)
        ydev = torch.zeros(40, cols, device=DEV, dtype=torch.float64)
        outs = [torch.full((models * resp * P,), 5.0, device=DEV, dtype=torch.float64),
                torch.full((models * P,), 5.0, device=DEV, dtype=torch.float64), torch.full((2 * P,), 5.0, device=DEV, dtype=torch.float64)]
        need = int(ws_fn(I, P, *(width if weighted else (width, K))))
        assert need > 0
        ws = torch.zeros(need + 16, device=DEV, dtype=torch.uint8)
        codes = [_raw(lib, builder, suffix, None if c.get("null") else X, I, A, B, Y, width, order, off, K, ydev, *outs, ws,
                      need - c.get("short", 0)) for suffix, X in (("f32", X32), (kind, X16))]
        torch.cuda.synchronize()
        assert codes[0] != 0 and codes[0] == codes[1], (builder, kind, name, codes)
        assert all(bool((o == 5.0).all()) for o in outs) and not bool(ws.any()), (builder, kind, name, "something was written")
        seen[name] = codes[0]
    print(f"cmtfpls_{builder}_{kind}: statuses {seen}")
    assert seen["K = 33"] == 4 and seen["W = 1025"] == 4 and (weighted or seen["K = 1"] == 4)               # CMTFPLS_EUNSUPPORTED
    assert seen["workspace one byte short"] == 2 and seen["null X"] == 1                                     # EWORKSPACE, EINVAL
