"""GPU: the three kernels of csrc/impute.hip (cmtfpls_holdout_mask_*, cmtfpls_heldout_resid_*, cmtfpls_impute_*) against the
float64 restatement of tests/impute_ref.py, f32 and f64 storage, vector and scalar forms, every register chunk (R = 1, 4, 5, 12,
16), R = 17 declined, scores with a padded leading dimension, hold-out fractions 0.1 and 0.5, offsets 0 and 4099 (inside a Philox
block).  Bounds: mask and counts exact; each sum within (n + 2R + 8) 2^-53 sum_held (|x| + |mean| + sum_a |t_a w_a|)^2;
imputed entries within 2^-24 |want| (f32 only) + (R + 2) 2^-53 (|mean| + sum_a |t_a w_a|)."""
import numpy as np
import pytest
import torch

import impute_ref as ref

pytestmark = pytest.mark.gpu

# (name, I, A, B, trailing shape, elements the base pointer is advanced by)
SHAPES = [
    ("ragged_one_workgroup", 37, 6, 8, (6, 8), 0),
    ("scalar_B_not_a_vector", 33, 7, 5, (7, 5), 0),
    ("scalar_misaligned_base", 37, 6, 8, (6, 8), 1),
    ("two_column_tiles", 19, 40, 32, (40, 32), 0),
    ("matrix_many_row_blocks", 20003, 1, 8, (8,), 0),
    ("order4_kronecker", 21, 4, 24, (4, 3, 8), 0),
    # the shapes of tests/test_gpu_workspace_contract.py: scalar and vector rows over several row blocks with a short last one
    ("scalar_row_blocks", 517, 7, 9, (7, 9), 0),
    ("vector_row_blocks", 517, 12, 20, (12, 20), 0),
    ("vector_row_blocks_misaligned_base", 517, 12, 20, (12, 20), 1),
]
# P = 1320: five column tiles and a partial one.  Run at R = 1, 5, 16 with one fraction and offset (the NumPy restatement of the
# hold-out sums takes seconds at this size)
TILED_SHAPES = [("column_tiles_and_a_partial_one", 2100, 33, 40, (33, 40), 0)]
FLAT_SIZES = [3, 1021, 300001]             # holdout_mask on a flat tensor: below one vector, a tail of one, many workgroups
RS = [1, 4, 5, 12, 16]
FRACTIONS = [0.1, 0.5]
OFFSETS = [0, 4099]
GUARD = 8                                  # sentinel elements on either side of a buffer (a multiple of 16 bytes in both types)
_DT = {"f32": (torch.float32, np.float32, np.int32), "f64": (torch.float64, np.float64, np.int64)}


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device("cuda:0"))


def _case(shape, dt, R):
    """Host inputs of one case, seeded by the case: X (I, P) with 20 % NaN and a few infinities, factors, mean."""
    name, I, A, B, trailing, _ = shape
    rng = np.random.default_rng([I, A, B, R, len(name)])
    P = A * B
    X = rng.normal(size=(I, P)).astype(_DT[dt][1])
    X[rng.random((I, P)) < 0.2] = np.nan
    for v in (np.inf, -np.inf, np.inf):
        X[rng.integers(I), rng.integers(P)] = v
    T = rng.normal(size=(I, R))
    WA = rng.normal(size=(A, R)) if A > 1 else np.ones((1, R))
    if len(trailing) == 3:                                             # order 4: WB is the Kronecker (Khatri-Rao) of the last two modes
        L2, L3 = rng.normal(size=(trailing[1], R)), rng.normal(size=(trailing[2], R))
        WB = (L2[:, None, :] * L3[None, :, :]).reshape(B, R)
    else:
        WB = rng.normal(size=(B, R))
    return X, T, WA, WB, rng.normal(size=P)


def _guarded(host, shift, dev):
    """(buffer, view): the array on the device between two runs of sentinels, its first element `shift` elements past an aligned
    address."""
    n = host.size
    buf = torch.full((GUARD + shift + n + GUARD,), 12345.0, dtype=torch.from_numpy(host).dtype, device=dev)
    view = buf[GUARD + shift: GUARD + shift + n]
    view.copy_(torch.from_numpy(host.reshape(-1)))
    return buf, view.view(host.shape)


def _bits(t, dt):
    return t.detach().cpu().contiguous().numpy().view(_DT[dt][2])


def _guards_intact(buf, shift, n):
    return bool((buf[:GUARD + shift] == 12345.0).all().item()) and bool((buf[GUARD + shift + n:] == 12345.0).all().item())


def _scores(T, dev):
    """T on the device with ldt = R + 3 and NaN sentinels in the padding."""
    I, R = T.shape
    full = torch.full((I, R + 3), float("nan"), dtype=torch.float64, device=dev)
    full[:, :R] = torch.from_numpy(T).to(dev)
    return full[:, :R]


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_holdout_mask(be, shape, dt):
    X, *_ = _case(shape, dt, 1)
    shift = shape[5]
    dev = be.device
    xbuf, Xd = _guarded(X, shift, dev)
    before = _bits(xbuf, dt).copy()
    for fraction in FRACTIONS:
        for offset in OFFSETS:
            obuf, out = _guarded(np.zeros_like(X), shift, dev)
            counts = be.holdout_mask(Xd, out, fraction, 215, 3, offset)
            want, wcounts = ref.masked_copy(X, fraction, 215, block=1, offset=offset)
            got = out.cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(want))
            keep = ~np.isnan(want)
            assert np.array_equal(_bits(out, dt)[keep], want.view(_DT[dt][2])[keep])
            assert counts.cpu().tolist() == [float(c) for c in wcounts]
            assert _guards_intact(obuf, shift, X.size) and np.array_equal(_bits(xbuf, dt), before)       # input only read
            obuf2, out2 = _guarded(np.zeros_like(X), shift, dev)
            counts2 = be.holdout_mask(Xd, out2, fraction, 215, 3, offset)
            assert np.array_equal(_bits(out2, dt), _bits(out, dt)) and torch.equal(counts2, counts)


def test_holdout_mask_tail_after_the_last_vector(be):
    """n = 4 k + 3 elements on aligned buffers: the vector form's last three elements take the single-element path."""
    X = np.random.default_rng(5).normal(size=1027).astype(np.float32)
    xbuf, Xd = _guarded(X, 0, be.device)
    obuf, out = _guarded(np.zeros_like(X), 0, be.device)
    counts = be.holdout_mask(Xd, out, 0.5, 7, 2, 2)
    want, wcounts = ref.masked_copy(X, 0.5, 7, block=0, offset=2)
    keep = ~np.isnan(want)
    assert np.array_equal(np.isnan(out.cpu().numpy()), ~keep) and np.array_equal(_bits(out, "f32")[keep], want.view(np.int32)[keep])
    assert counts.cpu().tolist() == [float(c) for c in wcounts] and _guards_intact(obuf, 0, X.size)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_heldout_resid(be, shape, dt):
    dev = be.device
    shift = shape[5]
    worst = 0.0
    for R in RS:
        X, T, WA, WB, mean = _case(shape, dt, R)
        _, Xd = _guarded(X, shift, dev)
        Td, WAd, WBd, md = _scores(T, dev), torch.from_numpy(WA).to(dev), torch.from_numpy(WB).to(dev), torch.from_numpy(mean).to(dev)
        for fraction in FRACTIONS:
            for offset in OFFSETS:
                got = be.heldout_resid(Xd, Td, WAd, WBd, md, fraction, 991, 2, offset)
                again = be.heldout_resid(Xd, Td, WAd, WBd, md, fraction, 991, 2, offset)
                assert got is not None and torch.equal(got, again)
                want, bound = ref.heldout_sums(X, T, WA, WB, mean, fraction, 991, block=0, offset=offset)
                g = got.cpu().numpy()
                assert g[R + 1] == want[R + 1] and want[R + 1] > 0
                err = np.abs(g[:R + 1] - want[:R + 1]).max()
                worst = max(worst, err / bound)
                assert err <= bound, (R, fraction, offset, err, bound)
    print(f"heldout_resid {shape[0]} {dt}: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_impute(be, shape, dt):
    dev = be.device
    shift = shape[5]
    worst = 0.0
    for R in RS:
        X, T, WA, WB, mean = _case(shape, dt, R)
        xbuf, Xd = _guarded(X, shift, dev)
        before = _bits(xbuf, dt).copy()
        Td, WAd, WBd, md = _scores(T, dev), torch.from_numpy(WA).to(dev), torch.from_numpy(WB).to(dev), torch.from_numpy(mean).to(dev)
        obuf, out = _guarded(np.zeros_like(X), shift, dev)
        count = be.impute(Xd, out, Td, WAd, WBd, md)
        want, gap, tol = ref.imputed(X, T, WA, WB, mean)
        assert count is not None and count.item() == float(gap.sum())
        assert _guards_intact(obuf, shift, X.size) and np.array_equal(_bits(xbuf, dt), before)
        assert np.array_equal(_bits(out, dt)[~gap], X.view(_DT[dt][2])[~gap])                       # observed: bit for bit
        err = np.abs(out.cpu().numpy().astype(np.float64) - want)[gap]
        assert (err <= tol[gap]).all()
        worst = max(worst, float((err / tol[gap]).max()))
        obuf2, out2 = _guarded(np.zeros_like(X), shift, dev)
        count2 = be.impute(Xd, out2, Td, WAd, WBd, md)
        assert np.array_equal(_bits(out2, dt), _bits(out, dt)) and torch.equal(count2, count)
        ibuf, Xi = _guarded(X, shift, dev)                                                           # in place on a private copy
        count3 = be.impute(Xi, Xi, Td, WAd, WBd, md)
        assert np.array_equal(_bits(Xi, dt), _bits(out, dt)) and torch.equal(count3, count) and _guards_intact(ibuf, shift, X.size)
    print(f"impute {shape[0]} {dt}: worst error / bound = {worst:.3g}")


@pytest.mark.parametrize("R", [1, 5, 16])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape", TILED_SHAPES, ids=[s[0] for s in TILED_SHAPES])
def test_heldout_resid_and_impute_across_column_tiles(be, shape, dt, R):
    dev = be.device
    X, T, WA, WB, mean = _case(shape, dt, R)
    xbuf, Xd = _guarded(X, 0, dev)
    before = _bits(xbuf, dt).copy()
    Td, WAd, WBd, md = _scores(T, dev), torch.from_numpy(WA).to(dev), torch.from_numpy(WB).to(dev), torch.from_numpy(mean).to(dev)
    got = be.heldout_resid(Xd, Td, WAd, WBd, md, 0.5, 991, 2, 4099)
    assert got is not None and torch.equal(got, be.heldout_resid(Xd, Td, WAd, WBd, md, 0.5, 991, 2, 4099))
    want, bound = ref.heldout_sums(X, T, WA, WB, mean, 0.5, 991, block=0, offset=4099)
    g = got.cpu().numpy()
    assert g[R + 1] == want[R + 1] and want[R + 1] > 0
    assert np.abs(g[:R + 1] - want[:R + 1]).max() <= bound
    obuf, out = _guarded(np.zeros_like(X), 0, dev)
    count = be.impute(Xd, out, Td, WAd, WBd, md)
    wantx, gap, tol = ref.imputed(X, T, WA, WB, mean)
    assert count is not None and count.item() == float(gap.sum())
    assert _guards_intact(obuf, 0, X.size) and np.array_equal(_bits(xbuf, dt), before)
    assert np.array_equal(_bits(out, dt)[~gap], X.view(_DT[dt][2])[~gap])                           # observed: bit for bit
    assert (np.abs(out.cpu().numpy().astype(np.float64) - wantx)[gap] <= tol[gap]).all()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", FLAT_SIZES)
def test_holdout_mask_of_a_flat_tensor(be, n, dt, shift):
    X = np.random.default_rng(n).normal(size=n).astype(_DT[dt][1])
    X[np.random.default_rng(n + 1).random(n) < 0.2] = np.nan
    xbuf, Xd = _guarded(X, shift, be.device)
    before = _bits(xbuf, dt).copy()
    obuf, out = _guarded(np.zeros_like(X), shift, be.device)
    counts = be.holdout_mask(Xd, out, 0.5, 215, 3, 4099)
    want, wcounts = ref.masked_copy(X, 0.5, 215, block=1, offset=4099)
    keep = ~np.isnan(want)
    assert np.array_equal(np.isnan(out.cpu().numpy()), ~keep) and np.array_equal(_bits(out, dt)[keep], want.view(_DT[dt][2])[keep])
    assert counts.cpu().tolist() == [float(c) for c in wcounts]
    assert _guards_intact(obuf, shift, X.size) and np.array_equal(_bits(xbuf, dt), before)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_seventeen_components_decline_and_take_the_torch_form(be, dt):
    from cmtf_pls_amd.engine import NipalsEngine
    from cmtf_pls_amd.state import BlockState, FitState

    shape, R = SHAPES[0], 17
    X, T, WA, WB, mean = _case(shape, dt, R)
    dev = be.device
    Xd = torch.from_numpy(X).to(dev)
    Td, WAd, WBd, md = _scores(T, dev), torch.from_numpy(WA).to(dev), torch.from_numpy(WB).to(dev), torch.from_numpy(mean).to(dev)
    assert be.heldout_resid(Xd, Td, WAd, WBd, md, 0.5, 3, 2, 0) is None
    assert be.impute(Xd, torch.empty_like(Xd), Td, WAd, WBd, md) is None
    blk = BlockState(shape=(shape[1],) + shape[4], A=shape[2], B=shape[3], mean=md, has_miss=True, colcnt=None, rowcnt=None, ssq0=1.0,
                     dtype=_DT[dt][0], loadings=[WAd, WBd])
    st = FitState(coupled=False, n_components=R, blocks=[blk], T=Td, U=Td, Q=Td, coef=np.eye(R), r2y=np.zeros(R), y_mean=md[:1],
                  n_iter=[1] * R, n_samples_total=shape[1])
    eng = NipalsEngine(be)
    X3 = Xd.view((shape[1],) + shape[4])
    got = eng.heldout_sums(st, [X3], Td, 0.5, 3)[0].cpu().numpy()
    assert eng.last_heldout == [{"form": "torch fallback", "why": "R = 17 > 16: outside cmtfpls_heldout_resid"}]
    want, bound = ref.heldout_sums(X, T, WA, WB, mean, 0.5, 3)
    assert got[R + 1] == want[R + 1] and np.abs(got[:R + 1] - want[:R + 1]).max() <= bound
    (filled, n), = eng.impute_rows(st, [X3], Td, inplace=False)
    assert eng.last_imputation == [{"form": "torch fallback", "why": "R = 17 > 16: outside cmtfpls_impute"}]
    wantx, gap, tol = ref.imputed(X, T, WA, WB, mean)
    assert n == int(gap.sum()) and filled.data_ptr() != Xd.data_ptr()
    f = filled.view(X.shape)
    assert np.array_equal(_bits(f, dt)[~gap], X.view(_DT[dt][2])[~gap])
    assert (np.abs(f.cpu().numpy().astype(np.float64) - wantx)[gap] <= tol[gap]).all()


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_overlapping_buffers_are_refused_before_any_launch(be, dt):
    """out that overlaps X without being X: CMTFPLS_EINVAL from the host-side range check (nothing is launched)."""
    from cmtf_pls_amd._lib import CmtfplsError

    shape, R = SHAPES[0], 4
    X, T, WA, WB, mean = _case(shape, dt, R)
    dev = be.device
    n = X.size
    buf = torch.zeros(2 * n, dtype=_DT[dt][0], device=dev)
    Xd = buf[:n].view(X.shape)
    Xd.copy_(torch.from_numpy(X))
    before = _bits(buf, dt).copy()
    Td, WAd, WBd, md = _scores(T, dev), torch.from_numpy(WA).to(dev), torch.from_numpy(WB).to(dev), torch.from_numpy(mean).to(dev)
    for shift in (4, n - 4):
        over = buf[shift:shift + n].view(X.shape)
        with pytest.raises(CmtfplsError, match="overlap"):
            be.holdout_mask(Xd, over, 0.5, 1, 2)
        with pytest.raises(CmtfplsError, match="overlaps"):
            be.impute(Xd, over, Td, WAd, WBd, md)
    assert np.array_equal(_bits(buf, dt), before)
    assert be.impute(Xd, buf[n:].view(X.shape), Td, WAd, WBd, md) is not None            # adjacent, not overlapping: taken
