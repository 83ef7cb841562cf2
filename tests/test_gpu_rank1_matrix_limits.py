"""Matrix rank-1 extraction (csrc/rank1.hip: syrk_step_kernel, syrk_chain_kernel, rank1_seed_xy_kernel, rank1_final_kernel,
rank1_final_score_kernel, the transpose) at its edges on a real MI355X.  Host side and case lists: tests/rank1_matrix_ref.py,
screened on the CPU by tests/test_rank1_matrix_ref_cpu.py.  There is no bit-level host mirror of the matrix cores' summation
order: bitwise assertions are made between device forms and against inputs whose arithmetic is exact.

  family 1  a permuted diagonal of powers of two with the dominant entry at every tile-row / chunk-column edge: the outputs are
            unit vectors, sigma = 1 and info = [1, 5] exactly (signed zeros compare equal), through the chain and the launches
  family 2  two equal largest entries: nothing converges, the whole budget is walked (30, 31 in the chain; 32, 48, 60 -> 48 in
            launches), every per-step array is used to its last row, the first tied index wins; then each exit on its own
  family 3  dense Z with a 0.5^i / 0.93^i spectrum against float64: residual, sigma, LAPACK's pair, unit norm, info, forms
  family 4  bitwise properties between device calls: power-of-two scaling, a misaligned view, repetition, the rank1_score gates
  family 5  entry checks: workspace one byte short / exact, bad arguments with untouched outputs, the zero matrix

Measured on an MI355X (worst over the cases; the bound of that case beside it):
  residual (family 3)      2.3e-15 at 48 x 513, 0.93^i (bound 1.2e-12); 3.3e-16 everywhere else (bounds 1.0e-13 .. 2.1e-12)
  |sigma - sigma_1|        8.9e-16 at 256 x 256, 0.93^i (bound 4.5e-13)
  loadings against LAPACK  6.2e-15 at 129 x 17, 0.5^i (bound 1e-10)
  tq against longdouble    9.3e-16 at 128 x 65, 2.2e-5 of its bound (P + 2) 2^-53 |S_row|^T |w|
  the close-gap case       residual 1.3e-16 (bound 6.1e-13), sigma 3.3e-16 (bound 1.4e-13)

Teeth -- each defect planted once in a scratch build of rank1.hip (never committed, all inside valid memory; in both the step
kernel and the chain kernel where both have the line, so that chain == launches alone cannot see it), and the tests of this
module that fail with it (failed cases of the 86):
  (a) `cok` compared with k - 1 (the last column of every product dropped)      77: exact_unit_vectors 11 / 11, whole_budget 15 / 15,
      each_exit 6 / 6, dense 34 / 34, close_gap, rank1_score 10 / 10
  (b) final_buf = out_buf (chain: = step) on the rank_one_in exit                13: exact_unit_vectors (1, 9), (9, 1), (1, 1), each_exit
      0 and 1 (Z of rank one), dense at n = 1 and (48, 513, 0.93) (which takes that exit at step 9), the zero matrix
  (c) the sign rule taken on wA instead of wB (both final kernels)               44: exact_unit_vectors 11 / 11, each_exit 6 / 6, dense 20,
      rank1_score 7
  (d) the chain's panel staging `pan[0][r][c]` one row on ((r + 1) & 15)         54: exact_unit_vectors 7 (every shape of the chain with n > 1),
      whole_budget 4 (budgets 30 and 31 at n <= 256), each_exit 4, dense 24, close_gap, scale 2 / 2, view 2 / 2, rank1_score 10 / 10
No defect of rank1.hip was found: all 86 cases pass on the library as it stands.
"""
import functools

import numpy as np
import pytest
import torch

import rank1_matrix_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHARED = ("the one-launch chain of squarings gave up waiting for a workgroup (info = [0, -1]): the GPU is shared with another "
          "process; the extraction is not repeated here")


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    b = HipBackend(DEV)
    assert b.lib.cmtfpls_rank1_chain_enabled() == 1, "the one-launch chain was switched off earlier in this process (a shared GPU?)"
    return b


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1)).to(DEV)


def bits(a):
    return np.atleast_1d(np.ascontiguousarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(x, y):
    """Equal bit patterns of two tuples of arrays / floats (None entries must match): NaNs and signed zeros count."""
    return len(x) == len(y) and all((a is None and b is None) or (a is not None and b is not None and np.array_equal(bits(a), bits(b)))
                                    for a, b in zip(x, y))


def extract(be, Zd, A, B, budget, launches=False, want_sigma=True, ws=None):
    """One call of the C entry: (wA, wB, info, sigma or None) on the host."""
    from cmtf_pls_amd import _lib
    lib = be.lib
    out = torch.full((A + B + 3,), 7.25, dtype=torch.float64, device=DEV)
    base, w = out.data_ptr(), ws if ws is not None else be._workspace("rank1", lib.cmtfpls_rank1_workspace_bytes(A, B))
    fn = lib.cmtfpls_rank1_launches_f64 if launches else lib.cmtfpls_rank1_f64
    _lib.check(fn(Zd.data_ptr(), A, B, base, base + 8 * A, (base + 8 * (A + B + 2)) if want_sigma else None, base + 8 * (A + B),
                  int(budget), w.data_ptr(), w.numel(), be._stream()), "rank1")
    h = out.cpu().numpy()
    wA, wB, info, sigma = h[:A], h[A:A + B], h[A + B:A + B + 2], h[A + B + 2]
    if info[0] == 0.0 and info[1] == -1.0:
        pytest.fail(SHARED)
    if not want_sigma:
        assert sigma == 7.25
    return wA, wB, info, (float(sigma) if want_sigma else None)


def both_forms(be, Zd, A, B, budget):
    """The entry (the chain where the shape and the budget allow) and the launch-per-squaring form: bit-equal, one returned."""
    one = extract(be, Zd, A, B, budget, launches=True)
    if R.uses_chain(A, B, budget):
        two = extract(be, Zd, A, B, budget, launches=False)
        assert same_bits(one, two), ("chain != launches", A, B, budget)
    return one


# ---- family 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,B", R.F1_SHAPES)
def test_exact_unit_vectors_with_the_dominant_entry_at_every_edge(be, A, B):
    """Z a permuted diagonal of +-2^-r: every squaring is exact, so wA = +-e_i, wB = +e_j, every other entry 0.0, sigma = 1.0 and
    info = [1, 5] ([1, 0] for n = 1: rank_one_in at once) whatever tile row (0, 15, 16, 17, A - 1) and chunk column (0, 7, 8, 31,
    32, 127, 128, 129, B - 1) the dominant entry sits in, of either sign."""
    want_info = [1.0, 5.0 if min(A, B) > 1 else 0.0]           # (the model's count: test_exact_cases_against_the_model)
    for i, j, s in R.family1_positions(A, B):
        c = R.exact_case(A, B, i, j, s)
        wA, wB, info, sigma = both_forms(be, dev(c["Z"]), A, B, R.F1_BUDGET)
        assert np.array_equal(wA, c["wA"]) and np.array_equal(wB, c["wB"]), (A, B, i, j, s, np.flatnonzero(wA), np.flatnonzero(wB))
        assert sigma == 1.0 and list(info) == want_info, (A, B, i, j, s, sigma, info)


# ---- family 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", R.F2_BUDGETS)
@pytest.mark.parametrize("A,B", R.F2_SHAPES)
def test_whole_budget_walked_on_a_tie(be, A, B, budget):
    """Magnitudes 1, 1, 1/2, 1/4, ...: rho = 1/2 at every step, so every squaring of the budget is computed -- trace row `budget`,
    the chain's buffer `budget` (31: its last), launches 32 .. 48 -- and the last G is read through last_buf; exact throughout:
    info = [0, min(budget, 48)], the unit vectors of the FIRST tied index, sigma = 1.0."""
    for lead, tie in R.family2_ties(A, B):
        c = R.exact_case(A, B, lead[0], lead[1], 1, tie=tie)
        wA, wB, info, sigma = both_forms(be, dev(c["Z"]), A, B, budget)
        assert np.array_equal(wA, c["wA"]) and np.array_equal(wB, c["wB"]), (A, B, budget, lead, np.flatnonzero(wA), np.flatnonzero(wB))
        assert sigma == 1.0 and list(info) == [0.0, float(min(budget, R.MAX_STEPS))], (A, B, budget, sigma, info)


@functools.lru_cache(maxsize=None)
def _exits():
    return [(name, Z, budget, info, R.model(Z, budget), R.svd_pair(Z)) for name, Z, budget, info in R.exit_cases()]


@pytest.mark.parametrize("k", range(6))
def test_each_exit_on_its_own(be, k):
    """rank_one_in at step 1 (final_buf = out_buf ^ 1, no squaring counted) at an even and an odd budget; rank_one_out (last_step
    = 5) at budgets 5 and 6; the budget running out at 3 and 4 (last_buf of either parity).  info as the model says; the
    loadings within 1e-12 of the model's (the same algorithm in another summation order: n eps = 1e-14 of rounding, no
    cancellation) and, once converged, of LAPACK's at the project's 1e-10."""
    name, Z, budget, want, (mA, mB, msig, _, _, _), (u, v, S) = _exits()[k]
    A, B = Z.shape
    wA, wB, info, sigma = both_forms(be, dev(Z), A, B, budget)
    assert (int(info[0]), int(info[1])) == want, (name, budget, info)
    np.testing.assert_allclose(wA, mA, rtol=0, atol=1e-12)
    np.testing.assert_allclose(wB, mB, rtol=0, atol=1e-12)
    assert abs(sigma - msig) <= R.sigma_bound(A, B, S[0])
    if want[0]:
        np.testing.assert_allclose(wA, u, rtol=0, atol=1e-10)
        np.testing.assert_allclose(wB, v, rtol=0, atol=1e-10)


# ---- family 3 ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense(A, B, r):
    Z = R.dense_case(A, B, r)
    Z.setflags(write=False)
    return Z, R.model(Z, R.F3_BUDGET), R.svd_pair(Z)


def _check_pair(be, Z, tag):
    """Residual and sigma of the device's pair against their bounds (printed first); returns what the entry gave."""
    A, B = Z.shape
    Zd = dev(Z)
    wA, wB, info, sigma = both_forms(be, Zd, A, B, R.F3_BUDGET)
    nA, nB, ni, _ = extract(be, Zd, A, B, R.F3_BUDGET, launches=False, want_sigma=False)
    assert same_bits((wA, wB, info), (nA, nB, ni)), "sigma = NULL changes the loadings"
    s1 = np.linalg.svd(Z, compute_uv=False)[0]
    res, rb = R.residual(Z, wA, wB), R.residual_bound(Z, s1)
    ds, sb = abs(sigma - s1), R.sigma_bound(A, B, s1)
    print(f"rank1-limits {tag} residual {res:.3e} bound {rb:.3e} sigma_err {ds:.3e} bound {sb:.3e}")
    assert res <= rb, (tag, res, rb)
    assert ds <= sb, (tag, ds, sb)
    np.testing.assert_allclose(np.linalg.norm(wA), 1, rtol=1e-14)
    np.testing.assert_allclose(np.linalg.norm(wB), 1, rtol=1e-14)
    return wA, wB, info, sigma


@pytest.mark.parametrize("A,B,r", R.family3_cases())
def test_dense_against_float64_at_the_edges(be, A, B, r):
    """Z = (U s) V^T with a zero row and a zero column.  residual <= (n + k + 8) 2^-53 |Z|_F^2 / sigma_1^2 + 1e-13 sqrt(n);
    |sigma - sigma_1| <= 8 2^-53 (n + k) sigma_1; LAPACK's sign-fixed pair at atol 1e-10; unit norms to 1e-14; exact zeros; info =
    [1, the model's squarings] where the margin is >= 5; chain == launches where n <= 256; sigma = NULL changes no bit."""
    Z, (mA, mB, msig, conv, steps, gaps), (u, v, S) = _dense(A, B, r)
    wA, wB, info, sigma = _check_pair(be, Z, f"{A}x{B} r={r}")
    err = max(np.abs(wA - u).max(), np.abs(wB - v).max())
    print(f"rank1-limits {A}x{B} r={r} loadings_err {err:.3e} bound 1e-10 info {info}")
    np.testing.assert_allclose(wA, u, rtol=0, atol=1e-10)
    np.testing.assert_allclose(wB, v, rtol=0, atol=1e-10)
    if A >= 4:
        assert wA[A // 2] == 0.0
    if B >= 4:
        assert wB[B // 3] == 0.0
    if (A, B, r) not in R.F3_INFO_NOT_ASSERTED:
        assert list(info) == [1.0, float(steps)], (info, steps, R.margin(gaps))
    else:
        assert info[0] == 1.0


def test_close_gap_residual_and_sigma(be):
    """(33, 129) with s2/s1 = 0.99999: the vectors are governed by the gap (1.7e-11 in the CPU model), the residual and sigma
    are not -- they keep their bounds."""
    wA, wB, info, sigma = _check_pair(be, R.close_gap_case(), "close gap")
    assert info[0] == 1.0


# ---- family 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,B", R.SCALE_SHAPES)
def test_power_of_two_scale_changes_only_sigma(be, A, B):
    """rank1(2^e Z): the Gram matrix scales by 2^2e exactly and the trace scaling undoes it, so wA, wB and info keep their bits
    and sigma scales by exactly 2^e -- as long as |G_0|_F^2 = O(|Z|^4 2^4e) stays a normal double (e = +-100: 2^+-400)."""
    Z = _dense(A, B, 0.5)[0]
    base = both_forms(be, dev(Z), A, B, R.F3_BUDGET)
    for e in R.SCALE_EXPONENTS:
        got = both_forms(be, dev(np.ldexp(Z, e)), A, B, R.F3_BUDGET)
        assert same_bits(base[:3], got[:3]), (A, B, e)
        assert got[3] == np.ldexp(base[3], e), (A, B, e, got[3], base[3])


@pytest.mark.parametrize("A,B", R.VIEW_SHAPES)
def test_misaligned_view_repeat_and_untouched_input(be, A, B):
    """Z 8 bytes into a larger allocation gives the bits of the aligned call; a second call gives the same bits; Z is not written."""
    Z = _dense(A, B, 0.93)[0]
    Zd = dev(Z)
    base = both_forms(be, Zd, A, B, R.F3_BUDGET)
    again = both_forms(be, Zd, A, B, R.F3_BUDGET)
    assert same_bits(base, again)
    assert np.array_equal(bits(Zd.cpu().numpy()), bits(Z.reshape(-1)))
    big = torch.zeros(A * B + 3, dtype=torch.float64, device=DEV)
    view = big[1:1 + A * B]
    view.copy_(Zd)
    assert view.data_ptr() % 16 == 8
    got = both_forms(be, view, A, B, R.F3_BUDGET)
    assert same_bits(base, got)
    assert big[0].item() == 0.0 and big[-1].item() == 0.0 and big[-2].item() == 0.0


@pytest.mark.parametrize("A,B,M,s_off", R.SCORE_CASES)
def test_rank1_score_on_both_sides_of_its_gates(be, A, B, M, s_off):
    """cmtfpls_rank1_score_f64 inside and outside its fused form (M <= 64, P >= 8192, even B, ((A + 1) & ~1) + B <= 7680 doubles
    of LDS, S 16-byte aligned): wA, wB, info and tq bit-equal to be.rank1 followed by the backend's score of S, and tq within
    (P + 2) 2^-53 |S_row|^T |w| of S kron(wA, wB) in longdouble."""
    rng = np.random.default_rng(A * 31 + B + M)
    Z = R.dense_case(A, B, 0.5, zero_lines=False)
    Sh = rng.normal(size=(M, A * B))
    buf = torch.zeros(M * A * B + 2, dtype=torch.float64, device=DEV)
    S = buf[s_off:s_off + M * A * B].view(M, A * B)
    S.copy_(torch.from_numpy(Sh))
    assert (S.data_ptr() % 16 == 0) == (s_off % 2 == 0)
    Zd = dev(Z)
    w1, v1, i1, t1 = be.empty(A), be.empty(B), be.zeros(2), be.empty(M)
    be.rank1(Zd, A, B, w1, v1, info=i1)
    be.score_s(S, A, B, w1, v1, t1)
    w2, v2, i2, t2 = be.empty(A), be.empty(B), be.zeros(2), be.empty(M)
    be.rank1_score(Zd, A, B, w2, v2, S, t2, info=i2)
    if tuple(i2.cpu().numpy()) == (0.0, -1.0):
        pytest.fail(SHARED)
    fused = R.score_is_fused(A, B, M, s_off)
    assert torch.equal(w1, w2) and torch.equal(v1, v2) and torch.equal(i1, i2) and torch.equal(t1, t2), (A, B, M, s_off, fused)
    wA, wB = w2.cpu().numpy(), v2.cpu().numpy()
    u, v, _ = R.svd_pair(Z)
    np.testing.assert_allclose(wA, u, rtol=0, atol=1e-10)
    np.testing.assert_allclose(wB, v, rtol=0, atol=1e-10)
    want = Sh.astype(np.longdouble) @ np.kron(wA.astype(np.longdouble), wB.astype(np.longdouble))
    err = np.abs(t2.cpu().numpy() - want).astype(np.float64)
    bound = R.tq_bound(Sh, wA, wB)
    print(f"rank1-limits score {A}x{B} M={M} off={s_off} fused={fused} tq_err/bound {float((err / bound).max()):.3e} err {err.max():.3e}")
    assert (err <= bound).all(), (A, B, M, float((err / bound).max()))


# ---- family 5 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,B", [(17, 129), (257, 257), (9, 1)])
def test_workspace_one_byte_short_is_refused_and_the_exact_size_is_enough(be, A, B):
    lib = be.lib
    need = lib.cmtfpls_rank1_workspace_bytes(A, B)
    assert need == R.workspace_bytes(A, B)
    Zd = dev(_dense(A, B, 0.5)[0])
    out = torch.full((A + B + 3,), 7.25, dtype=torch.float64, device=DEV)
    p = out.data_ptr()
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    for fn in (lib.cmtfpls_rank1_f64, lib.cmtfpls_rank1_launches_f64):
        rc = fn(Zd.data_ptr(), A, B, p, p + 8 * A, p + 8 * (A + B + 2), p + 8 * (A + B), 30, ws.data_ptr(), need - 1, be._stream())
        assert rc == 2 and b"workspace" in lib.cmtfpls_last_error()
    torch.cuda.synchronize()
    assert (out == 7.25).all().item()                              # nothing was launched
    ref = extract(be, Zd, A, B, 30)
    got = extract(be, Zd, A, B, 30, ws=ws)
    assert same_bits(ref, got)


def test_bad_arguments_are_refused_and_outputs_stay_untouched(be):
    lib = be.lib
    A, B = 5, 7
    Zd = dev(np.arange(35.0))
    out = torch.full((A + B + 3,), 7.25, dtype=torch.float64, device=DEV)
    p = out.data_ptr()
    ws = be._workspace("rank1", lib.cmtfpls_rank1_workspace_bytes(A, B))
    tail = (p + 8 * (A + B + 2), p + 8 * (A + B), 30, ws.data_ptr(), ws.numel(), be._stream())
    for fn in (lib.cmtfpls_rank1_f64, lib.cmtfpls_rank1_launches_f64):
        assert fn(None, A, B, p, p + 8 * A, *tail) == 1                          # null Z
        assert fn(Zd.data_ptr(), A, B, None, p + 8 * A, *tail) == 1              # null wA
        assert fn(Zd.data_ptr(), 0, B, p, p + 8 * A, *tail) == 1                 # A = 0
        assert b"bad argument" in lib.cmtfpls_last_error()
    assert lib.cmtfpls_rank1_workspace_bytes(0, B) == 0
    torch.cuda.synchronize()
    assert (out == 7.25).all().item()


def test_zero_matrix_gives_nan_loadings_as_the_oracle_does(be):
    """Z = 0 at (5, 7): the trace is 0, the first step takes its input as the result (info = [1, 0]) and the seed is 0 / 0 -- all-NaN
    loadings, which is what oracle.rank1_factors gives on the CPU (test_zero_matrix_in_the_oracle_and_the_model).  Pinned as it
    stands."""
    wA, wB, info, sigma = both_forms(be, dev(np.zeros((5, 7))), 5, 7, 30)
    assert np.isnan(wA).all() and np.isnan(wB).all() and list(info) == [1.0, 0.0]
