"""The X sweeps of csrc/sweeps.hip past one grid round and in their tall-tensor forms: every case of tests/sweep_cases.py first asks
the library which form it takes (be.sweep_form: the host function the entry launches from) and then compares EVERY output element
with plain float64 torch on the same stored values.

Inputs are drawn on the device in the case's storage type (the reference sees what is stored).  Masked cases, and every deflate and
center case, carry 20 % NaN, one all-NaN row and one all-NaN column (score_gram keeps the column only: an empty row makes every
partial sum of Y^T t NaN, for kernel and reference alike, and the comparison would see nothing).  Every output buffer is preset to
NaN, so an element that no workgroup wrote fails.  The contraction references are accumulated over row chunks of <= 4096 rows.

Bounds (from f64 accumulation of the stored values, not from what the kernels return)
  sums (Z, colsum, t, the summed qpart, ssq)   |got - want| <= c sum|terms| per output, c = 1e-13 = 900 x 2^-53: enough for a
      sequential chain + partial sums of 900 terms.  The longest chains: a thread of the contraction adds its workgroup's rows
      (<= 129 here, 2049 / 128 + 128 row lanes for the narrow form) and the second kernel ceil(row blocks / 8) + 8 <= 136 partial
      rows; a lane of a score adds <= 36879 / 64 + 6 = 583 terms; qpart 3 rows + 4 wavefronts + 512 workgroups.  Only the sum of
      squares of the deflation with loadings in global memory is longer: a lane adds its <= 36879 / 64 + 4 = 581 elements of each
      of its ceil(2085 / 2048) = 2 rows, then 6 butterfly levels, 4 wavefronts and 512 partials: (1162 + 522) 2^-53 = 1.87e-13.
      _ssq_coeff computes (chain + partials) 2^-53 from the form and takes the larger of it and 1e-13.
      u = Y q inside the kernel is one more chain of M <= 64 terms; sum|terms| is |X|^T (|Y| |q|).
  counts (colcnt, rowcnt)                       exact
  X written in place                            f32 rtol 3e-7 (one rounding to f32), f64 rtol 1e-13, atol 1e-10; loadings have unit norm
  NaN pattern                                   identical; the masked score of an empty row is NaN

Bit identity: the read-only entries are called twice; score_gram leaves the bits of score in t; the short-row form of score_deflate
(rows_narrow_kernel OP 2) is the arithmetic of its OP 0 and OP 1, so X and t have the bits of score followed by deflate.  (No test
claims that for score_deflate_kernel: a workgroup adds a row in another order than a wavefront.)

What these cases notice, tried once with faults planted in a scratch build: interleaved row blocks started at tile.rb + 1 fail the 36
ilv cases by value; a row sum of score_deflate_kernel that leaves out one wavefront from the third grid round on fails all 56
score_deflate_kernel cases (and no kernel-level test with I <= 256).  Reading and writing red[0] instead of red[parity] in
score_deflate_kernel fails NOTHING, here or elsewhere: the second buffer guards a write-after-read race whose window is 16 LDS
reads of the slowest wavefront against a whole row load and dot product of the fastest, and a comparison of values does not see a
race that the timing never lets happen.  The single barrier per row therefore rests on the kernel's text, not on a test."""
import time
import zlib

import pytest
import torch

import sweep_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
TDT = {"f32": torch.float32, "f64": torch.float64}
NAN = float("nan")
EPS = 2.0 ** -53
_t0 = [None, 0]


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    _t0[0] = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print(f"test_gpu_sweep_forms: {_t0[1]} cases in {time.perf_counter() - _t0[0]:.1f} s")


@pytest.fixture(autouse=True)
def _release():
    yield
    _t0[1] += 1
    torch.cuda.empty_cache()


def _cases(*ops):
    return [pytest.param(c, id=f"{c[0]}-{c[1]}-{c[2]}x{c[3]}x{c[4]}-{'m' if c[5] else 'u'}-M{c[6]}") for c in SC.CASES if c[0] in ops]


def _gen(case):
    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(repr(case[:7]).encode()))
    return g


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _chunk(P):
    return min(4096, max(1, (1 << 26) // P))


def _make_x(g, dt, I, P, nans, empty_row=True):
    X = torch.randn(I, P, generator=g, device=DEV, dtype=TDT[dt])
    if nans:
        step = max(1, (1 << 27) // P)
        for lo in range(0, I, step):
            xb = X[lo:lo + step]
            xb.masked_fill_(torch.rand(xb.shape, generator=g, device=DEV) < 0.2, NAN)
        X[:, P // 5] = NAN
        if empty_row:
            X[I // 3, :] = NAN
    return X


def _loadings(g, A, B):
    wa = torch.randn(A, generator=g, device=DEV, dtype=F64)
    wb = torch.randn(B, generator=g, device=DEV, dtype=F64)
    return wa / wa.norm(), wb / wb.norm()


def _nanbuf(*shape):
    return torch.full(shape, NAN, dtype=F64, device=DEV)


def _within(got, want, mag, coeff, what):
    assert bool(((got - want).abs() <= coeff * mag).all()), (what, float(((got - want).abs() / (coeff * mag + 1e-300)).nan_to_num(nan=1e300).max()))


def _same_x(X, want64, dt, what):
    """X written in place against the float64 value rounded to the storage type; the NaN pattern identical."""
    got = X.double()
    assert torch.equal(torch.isnan(got), torch.isnan(want64)), what
    rtol = 3e-7 if dt == "f32" else 1e-13
    ok = (got - want64).abs() <= 1e-10 + rtol * want64.abs()
    assert bool((ok | torch.isnan(want64)).all()), what
    return got


def _ssq_coeff(form, I, P):
    """(longest sequential chain of a lane + 6 butterfly levels + 4 wavefronts + 512 partials) 2^-53, at least 1e-13."""
    if form.startswith("wave"):
        chain = -(-I // 2048) * (P // 64 + 4)                      # a wavefront per row: 2048 rows a round, 64 lanes a row
    elif form.startswith("narrow"):
        chain = (-(-I // 2048) + 8) * 16                           # <= 8 rows of <= 16 elements per lane and round
    else:
        nseg = int(form.split("nseg")[1].split()[0]) if "nseg" in form else 1
        chain = -(-I * nseg // 512) * 64                           # a workgroup per row (segment): <= 16 vectors of 4 per lane
    return max(1e-13, (chain + 522) * EPS)


def _check_ssq(ssq, got64, form, I, P, what):
    want = torch.nan_to_num(got64, nan=0.0).square().sum()
    assert abs(float(ssq) - float(want)) <= _ssq_coeff(form, I, P) * float(want), (what, float(ssq), float(want))


# ---- contractions ------------------------------------------------------------------------------------------------------------------
def _ref_contract(X, u, umag, masked):
    """want = X^T u, mag = |X|^T umag, cnt = observations per column, over row chunks; masked: NaN counts as 0."""
    I, P = X.shape
    want, mag, cnt = (torch.zeros(P, dtype=F64, device=DEV) for _ in range(3))
    step = _chunk(P)
    for lo in range(0, I, step):
        xb = X[lo:lo + step].double()
        if masked:
            cnt += (~torch.isnan(xb)).sum(0)
            xb = torch.nan_to_num(xb, nan=0.0)
        want += xb.t() @ u[lo:lo + step]
        mag += xb.abs().t() @ umag[lo:lo + step]
    return want, mag, cnt


@pytest.mark.parametrize("case", _cases("colstats"))
def test_colstats_forms(be, case):
    op, dt, I, A, B, masked, M, form = case
    P = A * B
    assert be.sweep_form(op, dt, I, A, B, masked, M) == form
    X = _make_x(_gen(case), dt, I, P, True)
    ones = torch.ones(I, dtype=F64, device=DEV)
    want, mag, cnt = _ref_contract(X, ones, ones, True)
    ws = be._workspace("contract", be.lib.cmtfpls_colstats_workspace_bytes(I, P))
    out = []
    for _ in range(2):
        colsum, colcnt = _nanbuf(P), _nanbuf(P)
        rc = be._fn("colstats", X)(X.data_ptr(), I, P, colsum.data_ptr(), colcnt.data_ptr(), ws.data_ptr(), ws.numel(), be._stream())
        assert rc == 0
        out.append((colsum, colcnt))
    colsum, colcnt = out[0]
    _within(colsum, want, mag, 1e-13, case)
    assert torch.equal(colcnt, cnt) and float(colcnt[P // 5]) == 0.0 and float(colsum[P // 5]) == 0.0
    assert torch.equal(_bits(out[1][0]), _bits(colsum)) and torch.equal(out[1][1], colcnt)


@pytest.mark.parametrize("case", _cases("mode0_contract", "mode0_contract_yq"))
def test_contraction_forms(be, case):
    op, dt, I, A, B, masked, M, form = case
    P = A * B
    assert be.sweep_form(op, dt, I, A, B, masked, M) == form
    g = _gen(case)
    yq = op == "mode0_contract_yq"
    if form.startswith("unsupported"):
        X = _make_x(g, dt, I, P, False)
        Y, q = torch.randn(I, M, generator=g, device=DEV, dtype=F64), torch.randn(M, generator=g, device=DEV, dtype=F64)
        assert be.mode0_contract_yq(X, Y, q, masked, out=_nanbuf(P)) is None
        return
    X = _make_x(g, dt, I, P, masked)
    if yq:
        if M == 64:                                                 # a column view: ldy = 70
            Y = torch.randn(I, 70, generator=g, device=DEV, dtype=F64)[:, 3:67]
            assert Y.stride(0) == 70
        else:
            Y = torch.randn(I, M, generator=g, device=DEV, dtype=F64)
        q = torch.randn(M, generator=g, device=DEV, dtype=F64)
        u, umag = Y @ q, Y.abs() @ q.abs()
        run = lambda: be.mode0_contract_yq(X, Y, q, masked, out=_nanbuf(P))
    else:
        u = torch.randn(I, generator=g, device=DEV, dtype=F64)
        umag = u.abs()
        run = lambda: be.mode0_contract(X, u, masked, out=_nanbuf(P))
    want, mag, _ = _ref_contract(X, u, umag, masked)
    Z = run()
    assert Z is not None
    _within(Z, want, mag, 1e-13, case)
    if masked:
        assert float(Z[P // 5]) == 0.0                             # the column without an observation
    assert torch.equal(_bits(run()), _bits(Z))


# ---- score, score_gram ---------------------------------------------------------------------------------------------------------------
def _ref_score(X, w, masked):
    """t = X w (masked: NaN as 0, times P / observations of the row: NaN for an empty row), sum|terms| scaled alike, the counts."""
    x0 = X.double()
    rowcnt = None
    if masked:
        rowcnt = (~torch.isnan(x0)).sum(1).double()
        x0 = torch.nan_to_num(x0, nan=0.0)
    t, mag = x0 @ w, x0.abs() @ w.abs()
    if masked:
        scale = X.shape[1] / rowcnt                                 # inf for an empty row: 0 x inf = NaN
        t, mag = t * scale, torch.nan_to_num(mag * scale, nan=0.0, posinf=0.0)
    return t, mag, rowcnt


@pytest.mark.parametrize("case", _cases("score", "score_gram"))
def test_score_forms(be, case):
    op, dt, I, A, B, masked, M, form = case
    P = A * B
    assert be.sweep_form(op, dt, I, A, B, masked, M) == form
    g = _gen(case)
    gram = op == "score_gram"
    X = _make_x(g, dt, I, P, masked, empty_row=not gram)
    wa, wb = _loadings(g, A, B)
    if form.startswith("unsupported"):
        Y = torch.randn(I, M, generator=g, device=DEV, dtype=F64)
        assert be.score_gram(X, A, B, wa, wb, None, _nanbuf(I), Y, _nanbuf(be.n_partials * M)) is None
        return
    want, mag, rowcnt = _ref_score(X, torch.kron(wa, wb), masked)
    t = be.score(X, A, B, wa, wb, rowcnt, _nanbuf(I))
    assert torch.equal(torch.isnan(t), torch.isnan(want))
    if masked and not gram:
        assert bool(torch.isnan(t[I // 3])) and int(torch.isnan(t).sum()) == 1
    fin = ~torch.isnan(want)
    _within(t[fin], want[fin], mag[fin], 1e-13, case)
    assert torch.equal(_bits(be.score(X, A, B, wa, wb, rowcnt, _nanbuf(I))), _bits(t))
    if gram:
        assert be.sweep_form("score", dt, I, A, B, masked, 0) == form.replace(" gram", "")
        Y = torch.randn(I, M + 3, generator=g, device=DEV, dtype=F64)[:, 2:2 + M]             # ldy = M + 3
        out = []
        for _ in range(2):
            tg, qpart = _nanbuf(I), _nanbuf(be.n_partials * M)
            assert be.score_gram(X, A, B, wa, wb, rowcnt, tg, Y, qpart) is not None
            out.append((tg, qpart))
        tg, qpart = out[0]
        assert torch.equal(_bits(tg), _bits(t))                    # the score itself is that of cmtfpls_score_*
        _within(qpart.view(be.n_partials, M).sum(0), Y.t() @ t, Y.abs().t() @ t.abs(), 1e-13, case)
        assert torch.equal(_bits(out[1][1]), _bits(qpart))


# ---- deflate, score_deflate, center ------------------------------------------------------------------------------------------------
def _deflated(X, t, w):
    """x - t w in float64, rounded to the storage type of X."""
    return (X.double() - t[:, None] * w[None, :]).to(X.dtype).double()


@pytest.mark.parametrize("case", _cases("deflate"))
def test_deflate_forms(be, case):
    op, dt, I, A, B, masked, M, form = case
    P = A * B
    assert be.sweep_form(op, dt, I, A, B, masked, M) == form
    g = _gen(case)
    X = _make_x(g, dt, I, P, True)
    wa, wb = _loadings(g, A, B)
    t = torch.randn(I, generator=g, device=DEV, dtype=F64)
    want = _deflated(X, t, torch.kron(wa, wb))
    ssq = be.deflate(X, A, B, t, wa, wb)
    got = _same_x(X, want, dt, case)
    _check_ssq(ssq, got, form, I, P, case)


@pytest.mark.parametrize("case", _cases("score_deflate"))
def test_score_deflate_forms(be, case):
    op, dt, I, A, B, masked, M, form = case
    P = A * B
    assert be.sweep_form(op, dt, I, A, B, masked, M) == form
    g = _gen(case)
    X = _make_x(g, dt, I, P, masked)
    wa, wb = _loadings(g, A, B)
    if form.startswith("unsupported"):
        assert be.score_deflate(X, A, B, wa, wb, None, _nanbuf(I)) is None
        return
    w = torch.kron(wa, wb)
    t_want, mag, rowcnt = _ref_score(X, w, masked)
    want = _deflated(X, t_want, w)
    narrow = form.startswith("narrow")
    if narrow:                                                      # score, then deflate, on a copy: the same bits
        X2 = X.clone()
        t2 = be.score(X2, A, B, wa, wb, rowcnt, _nanbuf(I))
        ssq2 = be.deflate(X2, A, B, t2, wa, wb)
    t = _nanbuf(I)
    ssq = be.score_deflate(X, A, B, wa, wb, rowcnt, t)
    assert ssq is not None
    assert torch.equal(torch.isnan(t), torch.isnan(t_want))
    if masked:
        assert bool(torch.isnan(t[I // 3])) and int(torch.isnan(t).sum()) == 1
    fin = ~torch.isnan(t_want)
    _within(t[fin], t_want[fin], mag[fin], 1e-13, case)
    got = _same_x(X, want, dt, case)
    _check_ssq(ssq, got, form, I, P, case)
    if narrow:
        assert torch.equal(_bits(t), _bits(t2)) and torch.equal(_bits(X), _bits(X2)) and torch.equal(_bits(ssq), _bits(ssq2))


@pytest.mark.parametrize("case", _cases("center"))
def test_center_forms(be, case):
    op, dt, I, A, B, want_rowcnt, M, form = case
    P = A * B
    assert be.sweep_form(op, dt, I, A, B, want_rowcnt, M) == form
    g = _gen(case)
    X = _make_x(g, dt, I, P, True)
    mean = torch.randn(P, generator=g, device=DEV, dtype=F64)
    want = (X.double() - mean).to(X.dtype).double()
    rowcnt = _nanbuf(I) if want_rowcnt else None
    part = _nanbuf(be.n_partials)
    rc = be._fn("center", X)(X.data_ptr(), I, P, mean.data_ptr(), rowcnt.data_ptr() if want_rowcnt else None, part.data_ptr(), be._stream())
    assert rc == 0
    got = _same_x(X, want, dt, case)
    if want_rowcnt:
        assert torch.equal(rowcnt, (~torch.isnan(want)).sum(1).double()) and float(rowcnt[I // 3]) == 0.0
    assert not bool(torch.isnan(part).any())
    _check_ssq(be._close_partials(part), got, form, I, P, case)
