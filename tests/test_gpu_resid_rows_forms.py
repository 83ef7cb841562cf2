"""cmtfpls_resid_rows_* (csrc/resid.hip) in every form of its row blocking: more than 8 rows per block (lanes past 8 of the
lane-per-row layout), two and four 64-row chunks per block, a ragged last chunk, the unroll tail inside every block, two column
tiles at a tall shape, every register chunk and both sides of its boundaries, mean = NULL, a misaligned view, NaN score rows, a
row and a column of X entirely NaN, and the error codes that come before any launch.

Every case runs f32 and f64 storage against tests/resid_rows_ref.py -- float64 torch by row chunks for the tall shapes,
np.longdouble for the small ones -- within the bound derived in that module's docstring (nothing fitted), asserts the counts
exactly, a second call bit for bit, want_cols=False giving the same rows and X untouched, and asserts the plan (rows per block,
chunks per block) it was written for.  The worst |got - want| / bound per case is printed."""
import numpy as np
import pytest
import torch

import resid_rows_ref as RR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
SENTINEL = -7.25e300


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


def dev(a, dtype=F64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV).to(dtype)


def bits(t):
    return t.detach().contiguous().view(torch.int64 if t.dtype == F64 else torch.int32)


def _seed(*ints):
    return np.random.default_rng([int(i) for i in ints])


def _upload(X, T, WA, WB, mu, st, R, misaligned=False):
    dtype = F32 if st == "f32" else F64
    if misaligned:                                           # a view one element into its storage: one element per thread
        buf = torch.zeros(X.size + 1, dtype=dtype, device=DEV)
        buf[1:] = dev(X, dtype).reshape(-1)
        Xd = buf[1:].view(X.shape)
        assert Xd.data_ptr() % 16 != 0 and torch.equal(bits(Xd), bits(dev(X, dtype)))
    else:
        Xd = dev(X, dtype)
        assert Xd.data_ptr() % 16 == 0
    Tw = dev(T)
    Td = Tw[:, :R]                                           # ldt = R + 3, NaN behind the R columns
    assert Td.stride(0) == R + 3 and bool(torch.isnan(Tw[:, R:]).all())
    return Xd, Td, dev(WA), dev(WB), None if mu is None else dev(mu)


def _run(be, Xd, Td, WAd, WBd, mud):
    """The kernel with the checks every case makes beside the values: the same bits twice, the same rows without the column
    sums, X untouched."""
    keep = bits(Xd).clone()
    rows, cols = be.resid_rows(Xd, Td, WAd, WBd, mud, True)
    rows2, cols2 = be.resid_rows(Xd, Td, WAd, WBd, mud, True)
    assert torch.equal(bits(rows), bits(rows2)) and torch.equal(bits(cols), bits(cols2))
    rows3, none = be.resid_rows(Xd, Td, WAd, WBd, mud, False)
    assert none is None and torch.equal(bits(rows3), bits(rows))
    assert torch.equal(bits(Xd), keep)
    return rows.cpu().numpy(), cols.cpu().numpy()


def _compare(label, rows, cols, ref, skip_rows=(), cols_e2=True):
    """rows and cols against the reference within its bound, the counts exactly; returns and prints the worst ratio."""
    wr, wc, br, bc = ref
    assert np.array_equal(rows[:, 2], wr[:, 2].astype(np.float64)), label
    keep = np.ones(len(rows), dtype=bool)
    keep[list(skip_rows)] = False
    er = np.abs(rows[:, :2].astype(np.longdouble) - wr[:, :2]).astype(np.float64)
    ec = np.abs(cols.astype(np.longdouble) - wc).astype(np.float64)
    if not cols_e2:
        ec, bc = ec[:, 1:], bc[:, 1:]
    er, brk = er[keep], br[keep]
    assert np.all(np.isfinite(er)) and np.all(np.isfinite(ec)), label
    worst = 0.0
    for e, b in ((er, brk), (ec, bc)):
        assert np.all(e[b == 0] == 0), label                 # nothing observed: the sum is exactly 0
        if (b > 0).any():
            worst = max(worst, float((e[b > 0] / b[b > 0]).max()))
    print(f"{label}: worst |got - want| / bound = {worst:.3f}")
    assert worst <= 1.0, (label, worst)
    return worst


def _plan_of(st, I, A, B, misaligned):
    plan = RR.resid_plan(I, A * B, RR.vec_width(st, B, misaligned))
    return plan, RR.chunks_per_block(plan[2])


# ---- the tall cases: more than 8 rows per block ------------------------------------------------------------------------------------
CHUNKS = {"a": (1, 21), "a one element": (2, 6), "a view": (1, 21), "b": (2, 6), "b no mean": (2, 6), "c": (4, 9), "d": (2, 1),
          "e": (1, 9)}


@pytest.mark.parametrize("name,st,I,A,B,R,misaligned,mean,plan", RR.TALL_CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_tall_row_blocks(be, name, st, I, A, B, R, misaligned, mean, plan):
    got_plan, chunks = _plan_of(st, I, A, B, misaligned)
    assert got_plan == plan and chunks == CHUNKS[name] and plan[2] > 8            # the form this case was written for
    assert be.lib.cmtfpls_resid_rows_workspace_bytes(I, A * B) >= RR.resid_workspace_bytes(I, A * B, RR.vec_width(st, B, misaligned))
    X, T, WA, WB, mu = RR.inputs(_seed(21, I, A, B, R, int(mean)), I, A, B, R, st, mean, nan_fraction=0.05)
    ops = _upload(X, T, WA, WB, mu, st, R, misaligned)
    del X
    ref = RR.reference_torch(*ops)
    rows, cols = _run(be, *ops)
    _compare(f"resid_rows {name} {st} {(I, A, B, R)} plan {plan}", rows, cols, ref)


@pytest.mark.parametrize("st", RR.STORAGE)
def test_special_rows_and_columns(be, st):
    """Case b (70 rows per block, two chunks).  NaN score rows at lane 2 of a second chunk and lane 40 of a first: only those
    rows' sum e^2 is NaN, their sum x^2 and count are intact, every column's sum e^2 is NaN.  Then a row and a column of X
    entirely NaN: count 0 and sums exactly 0 (the reference's bound is 0 there)."""
    I, A, B, R = RR.SPECIAL
    plan, chunks = _plan_of(st, I, A, B, False)
    assert plan == (1, 2048, 70, 67) and chunks == (2, 6)
    assert [(r % 70) // 64 for r in RR.SPECIAL_SCORE_ROWS] == [1, 0] and [(r % 70) % 64 for r in RR.SPECIAL_SCORE_ROWS] == [2, 40]
    X, T, WA, WB, mu = RR.inputs(_seed(22, RR.STORAGE.index(st)), I, A, B, R, st, True, nan_fraction=0.05)
    Xd, Td, WAd, WBd, mud = _upload(X, T, WA, WB, mu, st, R)
    ref = RR.reference_torch(Xd, Td, WAd, WBd, mud)
    Tn = Td.clone()                                          # contiguous: ldt = R
    Tn[list(RR.SPECIAL_SCORE_ROWS)] = float("nan")
    rows, cols = be.resid_rows(Xd, Tn, WAd, WBd, mud, True)
    rows, cols = rows.cpu().numpy(), cols.cpu().numpy()
    nan_rows = np.flatnonzero(np.isnan(rows[:, 0]))
    assert nan_rows.tolist() == sorted(RR.SPECIAL_SCORE_ROWS) and not np.isnan(rows[:, 1:]).any()
    assert np.isnan(cols[:, 0]).all() and not np.isnan(cols[:, 1]).any()
    rows[nan_rows, 0] = ref[0][nan_rows, 0]                  # compared above; everything else against the reference
    _compare(f"resid_rows NaN score rows {st}", rows, cols, ref, cols_e2=False)
    # a row and a column with nothing observed
    row, col = 7 * 70 + 69, 5
    Xd[row] = float("nan")
    Xd[:, col] = float("nan")
    ops = (Xd, Td, WAd, WBd, mud)
    ref = RR.reference_torch(*ops)
    assert not ref[0][row].any() and not ref[1][col].any() and not ref[2][row].any() and not ref[3][col].any()
    rows, cols = _run(be, *ops)
    assert not rows[row].any() and not cols[col].any() and rows[:, 2].max() == A * B - 1
    _compare(f"resid_rows empty row and column {st}", rows, cols, ref)


# ---- register chunks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", RR.STORAGE)
@pytest.mark.parametrize("I,A,B", RR.CHUNK_SHAPES)
def test_register_chunk_boundaries(be, st, I, A, B):
    """R on both sides of 4 | 5, 8 | 9, 12 | 13 and at 16, ldt = R + 3 with NaN behind the R columns: a component at or past the
    chunk boundary is neither dropped (its term is far above the bound) nor read from the padding (NaN)."""
    for R in RR.CHUNK_R:
        X, T, WA, WB, mu = RR.inputs(_seed(23, I, A, B, R), I, A, B, R, st, True, nan_fraction=0.05)
        ref = RR.reference_ld(X, T[:, :R], WA, WB, mu)
        rows, cols = _run(be, *_upload(X, T, WA, WB, mu, st, R))
        _compare(f"resid_rows {st} {(I, A, B)} R = {R}", rows, cols, ref)
        # the last component carries weight: without it the reference moves far beyond the bound
        less = RR.reference_ld(X, np.concatenate([T[:, :R - 1], np.zeros((I, 1))], axis=1), WA, WB, mu)
        assert (np.abs(less[0][:, 0] - ref[0][:, 0]).astype(np.float64) / ref[2][:, 0]).max() >= 1000.0


# ---- before any launch -------------------------------------------------------------------------------------------------------------
def test_error_codes_come_before_any_launch(be):
    lib = be.lib
    I, A, B, R = 64, 8, 8, 4
    X, T, WA, WB, mu = RR.inputs(_seed(24), I, A, B, R, "f32", True, pad=0)
    Xd, Td, WAd, WBd, mud = dev(X, F32), dev(T), dev(WA), dev(WB), dev(mu)
    P = A * B
    need = lib.cmtfpls_resid_rows_workspace_bytes(I, P)
    assert need == RR.resid_workspace_bytes(I, P, 4) == RR.resid_workspace_bytes(I, P, 1)      # the same for every vector width
    assert lib.cmtfpls_resid_rows_workspace_bytes(0, P) == 0 and lib.cmtfpls_resid_rows_workspace_bytes(I, 0) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rows = torch.full((I, 3), SENTINEL, dtype=F64, device=DEV)
    cols = torch.full((P, 2), SENTINEL, dtype=F64, device=DEV)
    W17 = torch.ones(8, 17, dtype=F64, device=DEV)
    T17 = torch.ones(I, 17, dtype=F64, device=DEV)

    def call(ws_bytes=need, i=I, ldt=R, r=R, rows_ptr=rows.data_ptr(), t=Td, wa=WAd, wb=WBd):
        return lib.cmtfpls_resid_rows_f32(Xd.data_ptr(), t.data_ptr(), i, ldt, r, wa.data_ptr(), wb.data_ptr(), A, B, mud.data_ptr(),
                                          rows_ptr, cols.data_ptr(), ws.data_ptr(), ws_bytes, be._stream())

    assert call(ws_bytes=need - 1) == 2 and b"resid_rows" in lib.cmtfpls_last_error()          # CMTFPLS_EWORKSPACE
    assert call(ldt=R - 1) == 1 and call(i=0) == 1 and call(rows_ptr=None) == 1                # CMTFPLS_EINVAL
    assert call(ldt=17, r=17, t=T17, wa=W17, wb=W17) == 4                                      # CMTFPLS_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((rows == SENTINEL).all()) and bool((cols == SENTINEL).all())                   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    got = be.resid_rows(Xd, Td, WAd, WBd, mud, True)
    assert torch.equal(bits(rows), bits(got[0])) and torch.equal(bits(cols), bits(got[1])) and bool((rows[:, 2] == P).all())
