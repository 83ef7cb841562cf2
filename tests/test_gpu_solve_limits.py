"""The two solves of csrc/solve.hip at their limits, against the long-double restatements of tests/solve_ref.py: normal_solve in
its one-wavefront LDS form (k <= 64) and its workspace form (64 < k <= 1024: one to four passes of a thread's row loop), and
unit_upper_solve_rows up to R = 64 (the whole `Us` array in the LDS) past one block of rows and through column views.

EXACT inputs (Hadamard scores scaled by powers of two / small integers) must give the restatement's bits whatever the order of
operations; ROUNDING inputs must stay inside the derived bounds of solve_ref.py (a backward-error bound for normal_solve, a
running componentwise bound for the row solve), never a fitted tolerance.  Every case runs its call twice and asserts the
same bits and unchanged inputs.  The worst error / bound per kernel and the time of the k = 1024 solve are printed at teardown."""
import functools
import time

import numpy as np
import pytest
import torch

import solve_ref as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
SENTINEL = -7.25e300
LD = np.longdouble
KINDS = ["exact", "rounding"]
EUNSUPPORTED, EWORKSPACE = 4, 2


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(DEV)        # a copy: the builders' arrays are read-only


def host(t):
    return t.detach().cpu().double().numpy()


def bits(t):
    return t.detach().clone().contiguous().view(torch.int64)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


_worst, _times = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, r in sorted(_worst.items()):
        print(f"worst error / bound {k}: {r:.3f}")
    for k, t in sorted(_times.items()):
        print(f"normal_solve k = {k}: {t * 1e3:.1f} ms")


def record(kernel, ratio):
    print(f"{kernel}: error / bound {ratio:.3f}")
    _worst[kernel] = max(_worst.get(kernel, 0.0), float(ratio))
    assert ratio <= 1.0, (kernel, ratio)


def form(k):
    return "normal_solve LDS form" if k <= S.MAX_K_LDS else "normal_solve workspace form"


def run_normal(be, G, g):
    """be.normal_solve twice: the same bits, G and g unchanged bit for bit; the second call is timed."""
    Gd, gd = dev(G), dev(g)
    keep_G, keep_g = bits(Gd), bits(gd)
    b = be.normal_solve(Gd, gd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    again = be.normal_solve(Gd, gd)
    torch.cuda.synchronize()
    k = len(g)
    _times[k] = max(_times.get(k, 0.0), time.perf_counter() - t0)
    assert same_bits(b, again)
    assert torch.equal(bits(Gd), keep_G) and torch.equal(bits(gd), keep_g)
    return host(b)


def check_rounding(kernel, ref, got):
    """b finite, exactly 0.0 on the restatement's dropped columns and nowhere else, residual of the equilibrated system inside the bound."""
    assert np.all(np.isfinite(got))
    assert np.flatnonzero(got == 0.0).tolist() == ref.dropped
    r, bound = S.normal_solve_bound(ref, got)
    assert np.all(bound > 0) and np.all(np.isfinite(r))
    record(kernel, float((r / bound).max(initial=0.0)))
    return r, bound


# ---- normal_solve ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", S.EXACT_VARIANTS)
@pytest.mark.parametrize("k", S.NORMAL_K)
def test_normal_solve_exact_inputs(be, k, variant):
    """A^ is the identity (plus exact ones where a column is a power-of-two multiple of an earlier one): equality with the
    restatement; zero and duplicated columns at 0, k - 1 and on both sides of 64, 256, 512 and 768 give exactly 0.0."""
    G, g, ref = S.exact_normal(k, S.exact_rows(k), variant)
    got = run_normal(be, G, g)
    want = ref.b.astype(np.float64)
    assert np.array_equal(got, want), (form(k), np.flatnonzero(got != want)[:8])
    assert np.all(got[ref.dropped] == 0.0) and not np.any(np.signbit(got[ref.dropped]))


@pytest.mark.parametrize("variant", S.ROUNDING_VARIANTS)
@pytest.mark.parametrize("k", S.NORMAL_K)
def test_normal_solve_rounding_inputs(be, k, variant):
    G, g, ref = S.rounding_case(k, variant)
    check_rounding(form(k), ref, run_normal(be, G, g))


def test_normal_solve_same_problem_through_both_forms(be):
    """A 48-column problem (two zero columns and a shrunk one) at columns 5, 11, ..., 287 of a 300-column system whose other
    columns are zero: A^_KK (xhat_ws - xhat_lds) is the difference of the two residuals, inside the sum of both bounds."""
    ks, kb, pos = S.BOTH_FORMS
    pos = list(pos)
    G, g, ref = S.rounding_case(ks, "deficient")
    Gb, gb = S.embed(G, g, pos, kb)
    ref_big = S.normal_solve(Gb, gb)
    small, big = run_normal(be, G, g), run_normal(be, Gb, gb)
    r_s, bound_s = check_rounding(form(ks), ref, small)
    r_b, bound_b = check_rounding(form(kb), ref_big, big)
    assert np.array_equal(ref_big.kept, np.asarray(pos)[ref.kept])
    others = np.setdiff1d(np.arange(kb), pos)
    assert np.all(big[others] == 0.0)
    K = ref.kept
    diff = (big[pos][K].astype(LD) - small[K].astype(LD)) / ref.d[K]
    gap = np.abs(ref.Ahat[np.ix_(K, K)] @ diff).astype(np.float64)
    record("normal_solve workspace form against LDS form", float((gap / (bound_s + bound_b)).max()))


@pytest.mark.parametrize("R,a", S.ABI_COLUMN_CASES)
def test_normal_solve_writes_a_column_of_coef(be, R, a):
    """The C ABI with incb = R: b is column a of a row-major R x R matrix (coef_[:, a]); every other entry keeps its sentinel."""
    k = a + 1
    G, g, ref = S.rounding_case(k, "plain")
    Gd, gd = dev(G), dev(g)
    want = be.normal_solve(Gd, gd)
    nbytes = int(be.lib.cmtfpls_normal_solve_workspace_bytes(k))
    ws = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device=DEV)
    calls = [lambda p: be.lib.cmtfpls_normal_solve_ws_f64(Gd.data_ptr(), gd.data_ptr(), k, p, R, ws.data_ptr(), nbytes, be._stream())]
    if k <= S.MAX_K_LDS:
        assert nbytes == 0
        calls.append(lambda p: be.lib.cmtfpls_normal_solve_f64(Gd.data_ptr(), gd.data_ptr(), k, p, R, be._stream()))
    for call in calls:
        coef = torch.full((R, R), SENTINEL, dtype=F64, device=DEV)
        assert call(coef.data_ptr() + 8 * a) == 0
        assert same_bits(coef[:k, a], want)
        coef[:k, a] = SENTINEL
        assert bool((coef == SENTINEL).all())
    check_rounding(form(k), ref, host(want))


def test_normal_solve_workspace_size_and_refusals(be):
    lib, st = be.lib, be._stream()
    size = lib.cmtfpls_normal_solve_workspace_bytes
    assert size(64) == 0 and size(1025) == 0 and size(0) == 0
    for k in (65, 256, 1024):
        assert size(k) == (k * (k + 1) + 3 * k) * 8
    # k = 1025: refused before any launch, whatever the workspace
    k = 1025
    G, g = torch.zeros(k * k, dtype=F64, device=DEV), torch.zeros(k, dtype=F64, device=DEV)
    b = torch.full((k,), SENTINEL, dtype=F64, device=DEV)
    ws = torch.zeros(size(1024), dtype=torch.uint8, device=DEV)
    assert lib.cmtfpls_normal_solve_ws_f64(G.data_ptr(), g.data_ptr(), k, b.data_ptr(), 1, ws.data_ptr(), ws.numel(), st) == EUNSUPPORTED
    assert b"1024" in lib.cmtfpls_last_error()
    from cmtf_pls_amd._lib import CmtfplsError
    with pytest.raises(CmtfplsError, match="1024"):
        be.normal_solve(G.view(k, k), g, out=b)
    # the LDS entry point refuses 65 columns; the workspace form refuses a workspace one byte short
    k = 65
    need = size(k)
    assert lib.cmtfpls_normal_solve_f64(G.data_ptr(), g.data_ptr(), k, b.data_ptr(), 1, st) == EUNSUPPORTED
    assert b"64" in lib.cmtfpls_last_error()
    assert lib.cmtfpls_normal_solve_ws_f64(G.data_ptr(), g.data_ptr(), k, b.data_ptr(), 1, ws.data_ptr(), need - 1, st) == EWORKSPACE
    assert b"workspace" in lib.cmtfpls_last_error()
    assert lib.cmtfpls_normal_solve_ws_f64(G.data_ptr(), g.data_ptr(), k, b.data_ptr(), 1, None, need, st) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((b == SENTINEL).all())
    G65, g65, ref = S.rounding_case(k, "plain")
    Gd, gd = dev(G65), dev(g65)
    assert lib.cmtfpls_normal_solve_ws_f64(Gd.data_ptr(), gd.data_ptr(), k, b.data_ptr(), 1, ws.data_ptr(), need, st) == 0
    assert same_bits(b[:k], be.normal_solve(Gd, gd)) and bool((b[k:] == SENTINEL).all())


def test_normal_solve_non_finite_diagonal(be):
    """G = [[1, NaN], [NaN, inf]]: the inf diagonal gives d = 0 and a NaN pivot, the column is dropped with coefficient 0, and
    0 * NaN reaches the coefficients that the restatement says -- at k = 2 in the LDS form and at columns 70 and 200 of a
    260-column diagonal system in the workspace form."""
    ref = S.normal_solve(S.NONFINITE_G, S.NONFINITE_g)
    got = run_normal(be, S.NONFINITE_G, S.NONFINITE_g)
    assert ref.dropped == [1] and np.isnan(got[0]) and got[1] == 0.0
    assert np.array_equal(got, ref.b.astype(np.float64), equal_nan=True)
    k, cols, diag = S.NONFINITE_EMBED
    Gb, gb = S.embed(S.NONFINITE_G, S.NONFINITE_g, list(cols), k, diag)
    want = S.normal_solve(Gb, gb).b.astype(np.float64)
    got = run_normal(be, Gb, gb)
    assert got[cols[1]] == 0.0 and np.isnan(got[cols[0]]) and np.all(got[cols[1] + 1:] == 1.0)
    assert np.array_equal(got, want, equal_nan=True)


# ---- unit_upper_solve_rows ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def upper_ref(kind, I, R, with_shift):
    M, Um, shift = S.upper_inputs(kind, I, R)
    return S.unit_upper_solve_rows(M, Um, shift if with_shift else None)


def check_rows(kind, got, want, err, rows=None):
    rows = slice(None) if rows is None else rows
    got, want, err = got[rows], want[rows], err[rows]
    if kind == "exact":
        want64 = want.astype(np.float64)
        assert np.array_equal(got, want64), np.argwhere(got != want64)[:4]
        return
    e = np.abs(got.astype(LD) - want).astype(np.float64)
    assert np.all(np.isfinite(e)) and np.all(err > 0)
    record("unit_upper_solve_rows", float((e / err).max()))


@pytest.mark.parametrize("with_shift", [True, False])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("I,R", S.UPPER_CASES)
def test_row_solve(be, I, R, kind, with_shift):
    """M as the first R columns of an (I, R + 3) tensor of sentinels (ld = R + 3) and contiguous: the same bits, the padding
    untouched; U with NaN on and below its diagonal: the same bits; the NaN flag stays 0."""
    M, Um, shift = S.upper_inputs(kind, I, R)
    want, err = upper_ref(kind, I, R, with_shift)
    Ud, sd = dev(Um), (dev(shift) if with_shift else None)
    keep_U, keep_s = bits(Ud), (bits(sd) if with_shift else None)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    wide = torch.full((I, R + 3), SENTINEL, dtype=F64, device=DEV)
    wide[:, :R] = dev(M)
    out = be.unit_upper_solve_rows(wide[:, :R], Ud, sd, flag)
    assert out.data_ptr() == wide.data_ptr()
    check_rows(kind, host(wide[:, :R]), want, err)
    assert bool((wide[:, R:] == SENTINEL).all())
    again = dev(M)
    be.unit_upper_solve_rows(again, Ud, sd, flag)
    assert same_bits(again, wide[:, :R])
    masked = Um.copy()
    masked[np.tril_indices(R)] = np.nan
    third = dev(M)
    be.unit_upper_solve_rows(third, dev(masked), sd)                          # without a flag, too
    assert same_bits(third, again)
    assert int(flag.item()) == 0
    assert torch.equal(bits(Ud), keep_U) and (not with_shift or torch.equal(bits(sd), keep_s))


@pytest.mark.parametrize("I,R", S.UPPER_CASES)
def test_row_solve_nan_flag(be, I, R):
    """One NaN in row 0, in the last row of the first block, in the last row (the only row of the last block at I = 257, the last
    of its 113 rows at I = 70001): the flag becomes 1 and every other row keeps the bits of the run without NaN, inside the bound."""
    M, Um, shift = S.upper_inputs("rounding", I, R)
    want, err = upper_ref("rounding", I, R, True)
    Ud, sd = dev(Um), dev(shift)
    clean = dev(M)
    be.unit_upper_solve_rows(clean, Ud, sd)
    check_rows("rounding", host(clean), want, err)
    assert (257 - 1) % 256 == 0 and (70001 - 1) // 256 == 273
    for row in S.UPPER_NAN_ROWS[I]:
        col = (7 * row + 3) % R
        Md = dev(M)
        Md[row, col] = float("nan")
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        be.unit_upper_solve_rows(Md, Ud, sd, flag)
        assert int(flag.item()) == 1, (row, col)
        others = torch.arange(I, device=DEV) != row
        assert same_bits(Md[others], clean[others])
        assert bool(torch.isnan(Md[row, col:]).all()) and same_bits(Md[row, :col], clean[row, :col])


def test_row_solve_refuses_65_components(be):
    from cmtf_pls_amd._lib import CmtfplsError
    I, R = 5, 65
    M = torch.full((I, R), SENTINEL, dtype=F64, device=DEV)
    Ud, flag = torch.zeros(R, R, dtype=F64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(CmtfplsError, match="64"):
        be.unit_upper_solve_rows(M, Ud, None, flag)
    assert be.lib.cmtfpls_unit_upper_solve_rows_f64(M.data_ptr(), I, R, R, Ud.data_ptr(), None, None, be._stream()) == EUNSUPPORTED
    assert be.lib.cmtfpls_unit_upper_solve_rows_f64(M.data_ptr(), I, 63, 64, Ud.data_ptr(), None, None, be._stream()) == 1   # ld < R
    torch.cuda.synchronize()
    assert bool((M == SENTINEL).all()) and int(flag.item()) == 0
