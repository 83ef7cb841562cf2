"""The projection side at its declared limits: cmtfpls_project_rows*_ (one block, two coupled blocks, the _idx forms),
cmtfpls_predict_rows_f64 and cmtfpls_recon_* against a float64 NumPy restatement of the reference, and transform / predict
end to end against the oracle on the model's own factors, every route named by `projection_report_`.

The reference for the masked sequence (missingvals.py:23-38, tpls.py:128-142, cmtf.py:143-177) rounds the centred copy and
every deflation to the storage type, as the kernel documents (csrc/project.hip).  `_rows_instance` / `_rows2_instance`
mirror block_fits / run_project_rows, so every case states which template instance -- or which decline -- it covers."""
import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd.engine import default_options

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
TOL = {F32: 1e-10, F64: 1e-12}      # f32: the reference rounds like the kernel, so a missed rounding to f32 (~1e-7) fails
LDS_MAX = 144 * 1024
SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def api():
    import cmtf_pls_amd
    return cmtf_pls_amd


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


def _dev(a, dtype=F64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV).to(dtype)


def _np_t(dtype):
    return np.float32 if dtype == F32 else np.float64


# ---- mirror of block_fits / run_project_rows (csrc/project.hip) ------------------------------------------------------
def _nv(A, B, NT, dtype, max_nv):
    V = 16 // (4 if dtype == F32 else 8)
    stride = NT * V
    nv = -(-(A * B) // stride)
    return None if (B % V or stride % B or nv > max_nv) else nv


def _rows_instance(A, B, R, dtype):
    """(NT, NV) of the one-block kernel that takes an aligned A x B row, or None for a decline."""
    if R * (A + B) * 8 > LDS_MAX:
        return None
    nv = _nv(A, B, 256, dtype, 16)
    if nv is not None:
        return (256, 2 if nv <= 2 else 4 if nv <= 4 else 8 if nv <= 8 else 16)
    nv = _nv(A, B, 1024, dtype, 16)
    return None if nv is None else (1024, 8 if nv <= 8 else 16)


def _rows2_instance(shapes, R, dtype):
    """(NV0, NV1) of the two-block kernel (256 threads, longer block first), or None for a decline."""
    if R * sum(A + B for A, B in shapes) * 8 > LDS_MAX:
        return None
    (A0, B0), (A1, B1) = sorted(shapes, key=lambda s: -s[0] * s[1])
    nv0, nv1 = _nv(A0, B0, 256, dtype, 16), _nv(A1, B1, 256, dtype, 4)
    if nv0 is None or nv1 is None:
        return None
    s0, s1 = (2 if nv0 <= 2 else 4 if nv0 <= 4 else 8 if nv0 <= 8 else 16), (1 if nv1 <= 1 else 4)
    return None if (s0, s1) == (16, 4) else (s0, s1)


# ---- float64 restatement of the reference's masked sequence ----------------------------------------------------------
def _ref_project(blocks, R, dtype):
    """blocks: [(x (I, A*B) float64 holding storage-type values, WA (A, R), WB (B, R), mean (A*B) or None)].  The centred copy
    and every deflation rounded to the storage type; the mask from the input, so a NaN score turns the row's observed entries
    NaN and every later score of the sample NaN (missingvals.py:23-38 on the deflated copy)."""
    st = _np_t(dtype)
    work, obs = [], []
    for x, WA, WB, mean in blocks:
        c = x - mean if mean is not None else x.copy()
        work.append(c.astype(st).astype(np.float64))
        obs.append(~np.isnan(x))
    S = np.empty((blocks[0][0].shape[0], R))
    for a in range(R):
        ts, ws = [], []
        for (x, WA, WB, _), c, o in zip(blocks, work, obs):
            w = np.outer(WA[:, a], WB[:, a]).ravel()
            with np.errstate(divide="ignore", invalid="ignore"):
                ts.append(np.where(o, c, 0.0) @ w / o.sum(axis=1) * w.size)
            ws.append(w)
        t = ts[0] if len(ts) == 1 else (ts[0] + ts[1]) / 2.0
        S[:, a] = t
        for b, w in enumerate(ws):
            work[b] = (work[b] - np.outer(t, w)).astype(st).astype(np.float64)
    return S


def _colwise(got, want):
    """Worst normwise error per score column: max_i |got - want| / max_i |want| over the finite entries; NaN patterns equal."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    worst = 0.0
    for a in range(want.shape[1]):
        m = ok[:, a]
        if m.any():
            worst = max(worst, np.abs(got[m, a] - want[m, a]).max() / max(np.abs(want[m, a]).max(), 1e-300))
    return worst


def _loadings(rng, n, R):
    W = rng.normal(size=(n, R))
    return W / np.linalg.norm(W, axis=0)


def _rows(rng, I, P, dtype, holes=True):
    """Uncentred rows (offset 3) in the storage type's values: complete rows, partly observed rows, row 1 without any
    observation (NaN scores)."""
    x = rng.normal(size=(I, P)) + 3.0
    if holes and I > 1:
        x[rng.random(x.shape) < 0.2] = np.nan
        x[::3] = np.nan_to_num(x[::3], nan=2.5)
        x[1] = np.nan
    return x.astype(_np_t(dtype)).astype(np.float64)


def _block(rng, I, A, B, R, dtype, holes=True, mean=True):
    x = _rows(rng, I, A * B, dtype, holes)
    m = (np.nanmean(x, axis=0) + 0.01) if mean else None
    if m is not None and np.isnan(m).any():
        m = np.nan_to_num(m, nan=3.0)
    return x, _loadings(rng, A, R), _loadings(rng, B, R), m


def _run_rows(be, blk, R, dtype, out=None, rows=None, X=None):
    x, WA, WB, m = blk
    I = x.shape[0]
    X = _dev(x, dtype) if X is None else X
    out = be.empty(I, R) if out is None else out
    return be.project_rows(X, WA.shape[0], WB.shape[0], _dev(WA), _dev(WB), None if m is None else _dev(m), out, rows=rows), X


_worst = {}


def _record(kernel, dtype, err):
    key = (kernel, str(dtype))
    _worst[key] = max(_worst.get(key, 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (k, d), e in sorted(_worst.items()):
        print(f"worst normwise error {k} {d}: {e:.2e}")


# ---- A. project_rows, one block --------------------------------------------------------------------------------------
ROWS_CASES = [
    (F32, (1, 512), (256, 2)), (F32, (40, 32), (256, 2)),
    (F32, (96, 32), (256, 4)), (F32, (128, 32), (256, 4)),
    (F32, (160, 32), (256, 8)), (F32, (64, 128), (256, 8)),
    (F32, (72, 128), (256, 16)), (F32, (128, 128), (256, 16)),
    (F32, (136, 128), (1024, 8)), (F32, (144, 256), (1024, 16)), (F32, (256, 256), (1024, 16)),
    (F32, (272, 256), None),
    (F64, (64, 128), (256, 16)), (F64, (68, 128), (1024, 8)), (F64, (256, 128), (1024, 16)),
    (F64, (264, 128), None),
    (F32, (16, 6), None),                    # B % V != 0
    (F32, (8, 96), None),                    # B does not divide the workgroup stride
]


@pytest.mark.parametrize("dtype,shape,inst", ROWS_CASES, ids=lambda v: str(v))
def test_project_rows_instances_and_declines(be, dtype, shape, inst):
    A, B = shape
    R = 5
    assert _rows_instance(A, B, R, dtype) == inst
    rng = np.random.default_rng(A * 1000 + B)
    blk = _block(rng, 23, A, B, R, dtype)
    X = _dev(blk[0], dtype)
    keep = X.clone()
    got, _ = _run_rows(be, blk, R, dtype, X=X)
    if inst is None:
        assert got is None
        return
    assert got is not None
    assert torch.equal(X.view(torch.int32 if dtype == F32 else torch.int64), keep.view(torch.int32 if dtype == F32 else torch.int64))
    g = got.cpu().numpy()
    assert np.isnan(g[1]).all()                                     # the row without any observation
    err = _colwise(g, _ref_project([blk], R, dtype))
    _record("project_rows", dtype, err)
    assert err <= TOL[dtype], (inst, err)
    again, _ = _run_rows(be, blk, R, dtype, X=X)                    # same bits on a second call
    assert torch.equal(again.view(torch.int64), got.view(torch.int64))


def test_project_rows_declines_a_misaligned_x(be):
    """X one element into its storage: never read with 16-byte loads, declined."""
    rng = np.random.default_rng(2)
    blk = _block(rng, 8, 40, 32, 3, F32)
    buf = torch.zeros(8 * 1280 + 1, dtype=F32, device=DEV)
    X = buf[1:].view(8, 1280)
    X.copy_(_dev(blk[0], F32))
    assert X.data_ptr() % 16 != 0 and _rows_instance(40, 32, 3, F32) is not None
    got, _ = _run_rows(be, blk, 3, F32, X=X)
    assert got is None


@pytest.mark.parametrize("R,runs", [(72, True), (73, False)])
def test_project_rows_at_the_lds_edge(be, R, runs):
    """Loadings of R components: R (A + B) 8 bytes = 144 KB at f32 128 x 128, R = 72 (runs); one component more declines."""
    assert (R * 256 * 8 <= LDS_MAX) == runs and (_rows_instance(128, 128, R, F32) is not None) == runs
    rng = np.random.default_rng(R)
    blk = _block(rng, 6, 128, 128, R, F32)
    got, _ = _run_rows(be, blk, R, F32)
    if not runs:
        assert got is None
        return
    err = _colwise(got.cpu().numpy(), _ref_project([blk], R, F32))
    _record("project_rows", F32, err)
    assert err <= TOL[F32], err


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("I,mean", [(1, True), (9000, True), (40, False)])
def test_project_rows_row_counts_and_no_mean(be, dtype, I, mean):
    """One row; 9000 rows (more than one row per workgroup of the 4096-workgroup grid-stride loop); mean = None."""
    rng = np.random.default_rng(I)
    blk = _block(rng, I, 8, 32, 4, dtype, holes=I > 1, mean=mean)
    got, _ = _run_rows(be, blk, 4, dtype)
    err = _colwise(got.cpu().numpy(), _ref_project([blk], 4, dtype))
    _record("project_rows", dtype, err)
    assert err <= TOL[dtype], err


@pytest.mark.parametrize("dtype", [F32, F64])
def test_project_rows_writes_only_its_columns_of_a_wider_output(be, dtype):
    """`out` a column slice of a wider tensor (ld > R): the columns beyond R keep their bits."""
    rng = np.random.default_rng(11)
    R = 4
    blk = _block(rng, 30, 40, 32, R, dtype)
    wide = torch.full((30, R + 3), SENTINEL, dtype=F64, device=DEV)
    got, _ = _run_rows(be, blk, R, dtype, out=wide[:, 1:1 + R])
    assert got is not None and got.stride(0) == R + 3
    w = wide.cpu().numpy()
    assert (w[:, 0] == SENTINEL).all() and (w[:, 1 + R:] == SENTINEL).all()
    err = _colwise(w[:, 1:1 + R], _ref_project([blk], R, dtype))
    _record("project_rows", dtype, err)
    assert err <= TOL[dtype], err


# ---- B. project_rows2, two coupled blocks ----------------------------------------------------------------------------
ROWS2_CASES = [
    (F32, ((40, 32), (1, 512)), (2, 1)), (F32, ((64, 32), (40, 32)), (2, 4)), (F32, ((96, 32), (1, 512)), (4, 1)),
    (F32, ((128, 32), (4, 1024)), (4, 4)), (F32, ((64, 128), (1, 512)), (8, 1)), (F32, ((64, 128), (3, 1024)), (8, 4)),
    (F32, ((128, 128), (1, 512)), (16, 1)),
    (F32, ((72, 128), (40, 32)), None), (F32, ((128, 128), (160, 32)), None),
    (F64, ((20, 32), (1, 512)), (2, 1)), (F64, ((32, 32), (20, 32)), (2, 4)), (F64, ((48, 32), (1, 512)), (4, 1)),
    (F64, ((64, 32), (4, 256)), (4, 4)), (F64, ((32, 128), (1, 512)), (8, 1)), (F64, ((32, 128), (3, 512)), (8, 4)),
    (F64, ((64, 128), (1, 512)), (16, 1)),
    (F64, ((36, 128), (20, 32)), None), (F64, ((64, 128), (80, 32)), None),
]


def _run_rows2(be, blks, R, dtype, out=None, rows=None, dtypes=None):
    dtypes = dtypes or [dtype, dtype]
    I = blks[0][0].shape[0]
    out = be.empty(I, R) if out is None else out
    return be.project_rows2([_dev(b[0], d) for b, d in zip(blks, dtypes)], [b[1].shape[0] for b in blks], [b[2].shape[0] for b in blks],
                            [_dev(b[1]) for b in blks], [_dev(b[2]) for b in blks], [None if b[3] is None else _dev(b[3]) for b in blks],
                            out, rows=rows)


@pytest.mark.parametrize("dtype,shapes,inst", ROWS2_CASES, ids=lambda v: str(v))
def test_project_rows2_instances_and_declines(be, dtype, shapes, inst):
    R = 4
    assert _rows2_instance(shapes, R, dtype) == inst
    rng = np.random.default_rng(sum(a * b for a, b in shapes))
    blks = [_block(rng, 21, A, B, R, dtype) for A, B in shapes]
    got = _run_rows2(be, blks, R, dtype)
    if inst is None:
        assert got is None
        return
    g = got.cpu().numpy()
    assert np.isnan(g[1]).all()
    err = _colwise(g, _ref_project(blks, R, dtype))
    _record("project_rows2", dtype, err)
    assert err <= TOL[dtype], (inst, err)
    swapped = _run_rows2(be, blks[::-1], R, dtype)                  # the score is the mean of the two: order does not matter
    assert torch.equal(swapped.view(torch.int64), got.view(torch.int64))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_project_rows2_order4_block_and_a_row_empty_in_one_block(be, api, dtype):
    """An order-4 block (WB the Khatri-Rao product of its trailing loadings, formed on the device) coupled with a matrix block;
    a sample whose matrix row is empty: NaN from the first component on, as O.transform gives."""
    rng = np.random.default_rng(4)
    R, I = 3, 17
    L1, L2 = _loadings(rng, 4, R), _loadings(rng, 8, R)
    WB = be.khatri_rao(_dev(L1), _dev(L2)).cpu().numpy()
    assert np.array_equal(WB, np.stack([np.kron(L1[:, r], L2[:, r]) for r in range(R)], axis=1))
    b0 = _block(rng, I, 16, 32, R, dtype)
    b0 = (b0[0], b0[1], WB, b0[3])
    b1 = _block(rng, I, 1, 64, R, dtype)
    b1 = (b1[0], np.ones((1, R)), b1[2], b1[3])                      # a matrix block: WA = ones (ProjectionMixin._kr_operands)
    b1[0][1] = 3.0                                                   # the first block's row 1 is empty, the matrix row is full
    b1[0][5] = np.nan                                                # row 5: empty in the matrix block only
    got = _run_rows2(be, [b0, b1], R, dtype).cpu().numpy()
    assert np.isnan(got[1]).all() and np.isnan(got[5]).all()
    err = _colwise(got, _ref_project([b0, b1], R, dtype))
    _record("project_rows2", dtype, err)
    assert err <= TOL[dtype], err
    fit = O.OracleFit(coupled=True, n_components=R, block_shapes=[(I, 16, 4, 8), (I, 64)], y_shape=(I, 1), T=np.zeros((I, R)),
                      loadings=[[b0[1], L1, L2], [b1[2]]], U=np.zeros((I, R)), Q=np.zeros((1, R)), coef=np.zeros((R, R)),
                      r2x=[np.zeros(R)] * 2, r2y=np.zeros(R), x_means=[b0[3].reshape(16, 4, 8), b1[3]], y_mean=np.zeros(1),
                      has_miss=[False, False])
    want = O.transform(fit, [b0[0].reshape(I, 16, 4, 8), b1[0]])
    assert np.isnan(want[5]).all() and np.array_equal(np.isnan(got), np.isnan(want))


def test_project_rows2_declines_blocks_of_different_storage_types(be):
    rng = np.random.default_rng(6)
    blks = [_block(rng, 5, 40, 32, 2, F32), _block(rng, 5, 1, 512, 2, F32)]
    assert _run_rows2(be, blks, 2, F32, dtypes=[F32, F64]) is None


# ---- C. the _idx forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("two", [False, True])
def test_idx_forms_touch_only_the_listed_rows(be, dtype, two):
    """An unsorted subset of rows: listed rows equal the full form's rows bit for bit, the others keep their bits; an empty
    list is a no-op."""
    rng = np.random.default_rng(8 + two)
    R, I = 4, 300
    blks = [_block(rng, I, 64, 32, R, dtype)] + ([_block(rng, I, 1, 512, R, dtype)] if two else [])
    run = (lambda **k: _run_rows2(be, blks, R, dtype, **k)) if two else (lambda **k: _run_rows(be, blks[0], R, dtype, **k)[0])
    full = run()
    rows = torch.from_numpy(rng.permutation(I)[:97].copy()).to(DEV)
    assert not torch.equal(rows, rows.sort().values)
    out = torch.full((I, R), SENTINEL, dtype=F64, device=DEV)
    assert run(out=out, rows=rows) is not None
    listed = torch.zeros(I, dtype=torch.bool, device=DEV)
    listed[rows] = True
    assert torch.equal(out[listed].view(torch.int64), full[listed].view(torch.int64))
    assert bool((out[~listed] == SENTINEL).all())
    before = out.clone()
    assert run(out=out, rows=torch.empty(0, dtype=torch.int64, device=DEV)) is not None
    assert torch.equal(out.view(torch.int64), before.view(torch.int64))


# ---- D. predict_rows -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I,R,M,strided,mean", [(50, 1, 1, False, True), (33, 7, 5, True, True), (33, 7, 5, False, False),
                                                 (70000, 10, 64, True, True), (40, 15, 512, False, True)])
def test_predict_rows_matches_float64(be, I, R, M, strided, mean):
    """out = S Bm + mean; (R + 1) M 8 bytes = 64 KB exactly at R = 15, M = 512 still runs."""
    rng = np.random.default_rng(I + M)
    S = rng.normal(size=(I, R + (3 if strided else 0)))
    Bm, mu = rng.normal(size=(R, M)), rng.normal(size=M) * 5
    Sd = _dev(S)[:, :R]
    got = be.predict_rows(Sd, _dev(Bm), _dev(mu) if mean else None)
    assert got is not None
    want = S[:, :R] @ Bm + (mu if mean else 0.0)
    mag = np.abs(S[:, :R]) @ np.abs(Bm) + (np.abs(mu) if mean else 0.0)
    err = (np.abs(got.cpu().numpy() - want) / mag).max()
    _record("predict_rows", F64, err)
    assert err <= 1e-14 * (R + 1), err


def test_predict_rows_declines_beyond_64_kb(be):
    assert be.predict_rows(_dev(np.ones((4, 15))), _dev(np.ones((15, 513))), None) is None


def test_predict_with_513_responses_falls_back_to_the_host(api, monkeypatch):
    x, y, _ = O.import_synthetic((120, 8, 6), 513, 4, error=0.1, seed=3)
    m = api.tPLS(15, dtype="float64")
    m.fit(x, y, max_iter=20)
    from cmtf_pls_amd.backend import HipBackend
    seen = []
    orig = HipBackend.predict_rows
    monkeypatch.setattr(HipBackend, "predict_rows", lambda self, *a: seen.append(orig(self, *a)) or seen[-1])
    got = m.predict(x[:20])
    assert len(seen) == 1 and seen[0] is None
    want = O.predict(_oracle_fit_of(m, False), x[:20])
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err <= 1e-9, err


# ---- E. recon ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("R", [5, 9, 13, 16, 17, 32, 33])
@pytest.mark.parametrize("form", ["vector", "B % V", "misaligned", "one row"])
def test_recon_matches_float64(be, dtype, R, form):
    """Xhat = T (WA (.) WB)^T + mean in the storage type: one pass for R <= 16, then accumulate passes of 16.  f32 rounds the
    partial sum to f32 between passes, so its bound is passes x 2^-24 x (|mean| + sum_r |t_r w_r|) per element; f64 1e-14
    of the same magnitude.  R = 5, 9, 13 are the first of the 8, 12 and 16 component instances (17 and 33 end in the one of 4):
    a bracket chosen one too low drops a component."""
    A, B = (6, 9) if form == "B % V" else (6, 64)
    I = 1 if form == "one row" else 37
    rng = np.random.default_rng(R)
    T, WA, WB, mu = rng.normal(size=(I, R + 2)), rng.normal(size=(A, R)), rng.normal(size=(B, R)), rng.normal(size=A * B)
    P = A * B
    if form == "misaligned":
        buf = torch.zeros(I * P + 1, dtype=dtype, device=DEV)
        out = buf[1:]
        assert out.data_ptr() % 16 != 0
    else:
        out = torch.zeros(I * P, dtype=dtype, device=DEV)
    assert be.recon(_dev(T)[:, :R], _dev(WA), _dev(WB), _dev(mu), out) is not None
    W = (WA[:, None, :] * WB[None, :, :]).reshape(P, R)
    want = T[:, :R] @ W.T + mu
    mag = np.abs(T[:, :R]) @ np.abs(W).T + np.abs(mu)
    passes = -(-R // 16)
    bound = passes * 2.0 ** -24 * 1.01 if dtype == F32 else 1e-14
    err = (np.abs(out.cpu().double().numpy().reshape(I, P) - want) / mag).max()
    _record("recon", dtype, err)
    assert err <= bound, (err, bound)


# ---- F. transform / predict end to end -----------------------------------------------------------------------------------
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


def _normwise(got, want):
    scale = np.nanmax(np.abs(want), axis=0, keepdims=True)
    return np.nanmax(np.abs(got - want) / (np.abs(want) + scale))


@pytest.mark.parametrize("R,form,why", [
    (16, "one-pass MTTKRP (one read, nothing written)", None),
    (17, "one-pass MTTKRP (one read, nothing written)", None),
    (32, "one-pass MTTKRP (one read, nothing written)", None),
    (33, "masked sequence, every row in registers (one read)", "one-pass MTTKRP declined: R = 33 > 32"),
    (64, "masked sequence, every row in registers (one read)", "one-pass MTTKRP declined: R = 64 > 32"),
])
def test_transform_routes_by_component_count(api, R, form, why):
    x, y, _ = O.import_synthetic((300, 16, 16), 4, 6, error=0.3, seed=R)
    m = api.tPLS(R, dtype="float64")
    m.fit(x, y, max_iter=20)
    fit = _oracle_fit_of(m, False)
    new = x[:64] + 0.05 * np.random.default_rng(1).normal(size=x[:64].shape)
    got = m.transform(new)
    rep = m.projection_report_
    assert rep["form"] == form and rep["why"] == why, rep
    err = _normwise(got, O.transform(fit, new))
    assert err <= 1e-9, err
    p = m.predict(new)
    assert _normwise(p, O.predict(fit, new)) <= 1e-9


def test_transform_of_three_coupled_blocks_with_missing_values(api):
    rng = np.random.default_rng(21)
    x, y, cp = O.import_synthetic((240, 8, 16), 3, 4, error=0.2, seed=21)
    blocks = [x, cp.factors[0] @ rng.normal(size=(4, 48)) + 0.2 * rng.normal(size=(240, 48)),
              np.einsum("ir,jr,kr->ijk", cp.factors[0], rng.normal(size=(6, 4)), rng.normal(size=(8, 4))) + 0.2 * rng.normal(size=(240, 6, 8))]
    m = api.ctPLS(4, dtype="float64")
    m.fit(blocks, y, max_iter=30)
    new = [b[:50].copy() for b in blocks]
    bad = rng.random(50) < 0.3                                       # some samples incomplete, most complete
    for b in new:
        hole = rng.random(b.shape) < 0.1
        hole[~bad] = False
        b[hole] = np.nan
    got = m.transform(new)
    rep = m.projection_report_
    assert rep["form"] == "one-pass MTTKRP for the complete samples + sequential passes on copies of the incomplete ones", rep
    fit = _oracle_fit_of(m, True)
    want = O.transform(fit, new)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and _normwise(got, want) <= 1e-9
    assert _normwise(m.predict(new), O.predict(fit, new)) <= 1e-9


@pytest.mark.parametrize("coupled", [False, True])
@pytest.mark.parametrize("offset", [1e6, 1e10])
def test_transform_of_badly_offset_data(api, coupled, offset):
    """x + offset x spread (in ctPLS one block only): the one-pass form on the uncentred rows would lose ~1e-16 x offset of
    the scores; the rows are centred first (in registers here).  transform matches O.transform to 1e-9 and reproduces the
    fitted scores from the training X (what new-row diagnostics rely on)."""
    x, y, cp = O.import_synthetic((200, 8, 16), 3, 4, error=0.2, seed=9)
    x = x + offset * x.std()
    blocks = [x]
    if coupled:
        blocks.append(cp.factors[0] @ np.random.default_rng(2).normal(size=(4, 32)) + 0.2 * np.random.default_rng(3).normal(size=(200, 32)))
    m = (api.ctPLS if coupled else api.tPLS)(4, dtype="float64")
    m.fit(blocks if coupled else x, y, max_iter=30)
    fit = _oracle_fit_of(m, coupled)
    arg = [b[:60] for b in blocks] if coupled else x[:60]
    got = m.transform(arg)
    rep = m.projection_report_
    assert rep["offset_ratio"] > 1e4 and rep["form"] == "masked sequence, every row in registers (one read)", rep
    err = _normwise(got, O.transform(fit, arg))
    T = m.factor_T if coupled else m.X_factors[0]
    err_fit = _normwise(m.transform(blocks if coupled else x), T)
    forced = (api.ctPLS if coupled else api.tPLS)(4, dtype="float64", options=default_options().but(project_raw_max_offset=float("inf")))
    forced.fit(blocks if coupled else x, y, max_iter=30)
    raw = _normwise(forced.transform(arg), O.transform(_oracle_fit_of(forced, coupled), arg))
    print(f"offset {offset:g} coupled={coupled}: centred first {err:.2e} (fitted scores {err_fit:.2e}); "
          f"uncentred one-pass form {raw:.2e} ({forced.projection_report_['form']})")
    assert err <= 1e-9 and err_fit <= 1e-9, (err, err_fit)
