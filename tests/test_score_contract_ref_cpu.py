"""tests/score_contract_ref.py without a GPU: the mirror of run_score_contract against the library's own workspace function and
against the case tables that tests/test_gpu_score_contract_forms.py runs on the device -- every case on the instance it names,
the cases together on every instance the dispatch can select and on every remainder of the split kernel's unrolled step loop --
and the bounds against float64 evaluations of the same sums in three orders."""
from fractions import Fraction

import numpy as np
import pytest

import score_contract_ref as SC

DTYPES = ("f32", "f64")
ORDERS = ("forward", "reversed", "chunked")
CUS = 256                        # the count the case tables are written for (and kScGrid: more compute units change nothing)


@pytest.fixture(scope="module")
def lib():
    from cmtf_pls_amd import _lib
    return _lib.load()


def _all_shapes():
    extra = SC.NAN_CASES + [s for v in SC.CONTRACT_CASES.values() for s in v]
    return [c[0] for c in SC.ALL_CASES] + extra


def test_workspace_mirror_equals_the_library_and_covers_every_form(lib):
    for I, A, B in _all_shapes():
        P = A * B
        assert lib.cmtfpls_score_contract_workspace_bytes(I, P) == SC.workspace_bytes(I, P), (I, A, B)
        for dt in DTYPES:
            for cus in (CUS, 304, 64, 16):
                f = SC.form(dt, I, A, B, cus)
                assert "decline" in f or 0 < f["need"] <= SC.workspace_bytes(I, P), (dt, I, A, B, f)
    assert lib.cmtfpls_score_contract_workspace_bytes(0, 5) == 0 == SC.workspace_bytes(0, 5)
    assert lib.cmtfpls_score_contract_workspace_bytes(5, 0) == 0 == SC.workspace_bytes(5, 0)
    # the hand-expanded sums of one case per form
    assert SC.form("f32", 70, 32, 128, CUS)["need"] == 70 * 4097 * 8
    assert SC.form("f32", 20, 160, 128, CUS)["need"] == (20 * 20481 + 20 * 2) * 8
    assert SC.form("f64", 200, 256, 256, CUS)["need"] == (32 * 65537 + 200 * 8) * 8


def test_every_case_sits_on_the_instance_claimed_for_it():
    for dt in DTYPES:
        for shape, _, _ in SC.ALL_CASES:
            f = SC.check_claim(dt, shape, CUS)
            assert SC.check_claim(dt, shape, 304) == f          # more compute units than kScGrid change nothing
            if shape in SC.ROWS_PER_WORKGROUP and "decline" not in f:
                assert f["form"] == "rows" and f["rows"] == SC.ROWS_PER_WORKGROUP[shape], (dt, shape, f)
    f = SC.form
    # the geometry the tables' comments state
    assert f("f64", 300, 41, 100, CUS)["NV"] == 4 and f("f64", 300, 41, 100, CUS)["nv"] == 3      # one wholly absent vector
    assert f("f32", 70, 5, 6500, CUS)["S"] == 64 == f("f64", 70, 5, 6500, CUS)["S"]
    assert f("f32", 70, 5, 6500, CUS)["rows"] == (1, 2)
    assert (f("f32", 37, 512, 512, CUS)["G"], f("f32", 37, 512, 512, CUS)["S"]) == (16, 16)
    assert f("f32", 70, 3, 43000, CUS)["rows"] == (4, 5) == f("f64", 70, 3, 43000, CUS)["rows"]
    assert f("f32", 40, 160, 128, CUS)["rows"] == (1, 1) and f("f32", 40, 160, 128, CUS)["S"] == 40
    assert f("f32", 16, 256, 256, CUS)["S"] == 16 and f("f32", 65, 256, 256, CUS)["rows"] == (1, 2)     # I <= S; I = S + 1
    assert f("f64", 33, 256, 256, CUS)["rows"] == (1, 2) and f("f64", 33, 256, 256, CUS)["S"] == 32
    assert f("f32", 200, 256, 256, CUS)["rows"] == (3, 4) and f("f64", 200, 256, 256, CUS)["rows"] == (6, 7)
    assert f("f32", 129, 256, 256, CUS)["rows"] == (2, 3) and f("f64", 129, 256, 256, CUS)["rows"] == (4, 5)
    # WL: the LDS array full, and one mode-1 slice per stride
    full, one = f("f64", 60, 2048, 8, CUS), f("f64", 60, 8, 2048, CUS)
    assert full["WL"] and full["NV"] * full["jstep"] == 2048 == SC.K_SC_LDS_A and one["WL"] and one["jstep"] == 1
    assert not f("f64", 100, 4096, 4, CUS)["WL"] and not f("f64", 100, 120, 128, CUS)["WL"]
    # the robustness and the host-contract shapes: one per form
    for dt in DTYPES:
        assert [SC.form(dt, *s, cus=CUS)["form"] for s in SC.NAN_CASES] == ["rows", "split"]
        assert [SC.form(dt, *s, cus=CUS)["form"] for s in SC.CONTRACT_CASES[dt]] == ["rows", "split"]
        assert SC.form(dt, *SC.NAN_CASES[1], cus=CUS)["rows"][0] >= 2


def _reachable(dt):
    """Every instance run_score_contract<T> selects for some shape, by enumeration."""
    seen = set()
    stride = SC.stride_of(dt)
    Bs = sorted({2 ** k for k in range(1, 14)} | {12, 20, 100, 340, 1000, 2044, 3300, 6500, 43000, 131072})
    for B in Bs:
        for P in sorted({stride // 2, stride - B, stride, stride + B, 2 * stride, 2 * stride + B, 3 * stride, 4 * stride, 4 * stride + B,
                         5 * stride, 7 * stride, 8 * stride, 8 * stride + B, 9 * stride, 16 * stride, 33 * stride, 64 * stride}):
            A = max(P // B, 1)
            for I in (1, 300):
                inst = SC.instance(SC.form(dt, I, A, B, CUS))
                if inst is not None:
                    seen.add(inst)
    return seen


def test_the_cases_cover_every_instance_and_every_remainder():
    for k, dt in enumerate(DTYPES):
        covered, rem = set(), {}
        for c in SC.ALL_CASES:
            f = SC.form(dt, *c[0], cus=CUS)
            inst = SC.instance(f)
            if inst is None:
                continue
            covered.add(inst)
            if f["form"] == "split":
                rem.setdefault(inst, set()).update(f["remainders"])
        assert covered == set(SC.INSTANCES[dt]) == _reachable(dt), (dt, covered ^ set(SC.INSTANCES[dt]))
        # every exit of the step loop unrolled LAG + 2 times, for each split instance on its own (hence for both LAG values)
        for inst, got in rem.items():
            assert got == set(range(inst[3] + 2)), (dt, inst, got)
        assert {i[3] for i in rem} == {1, 2}
    assert len(SC.INSTANCES["f32"]) + len(SC.INSTANCES["f64"]) == 8 + 11
    # G: the smallest, the largest, and one past it, for either storage type
    for dt in DTYPES:
        gs = {f["G"] for f in (SC.form(dt, *c[0], cus=CUS) for c in SC.SPLIT_CASES) if f.get("form") == "split"}
        assert min(gs) <= 3 and max(gs) == 16
        assert any(SC.form(dt, *c[0], cus=CUS).get("decline") == "G = 17 > 16" for c in SC.SPLIT_CASES)
    assert SC.form("f32", 40, 160, 128, CUS)["G"] == 2


def test_the_seven_decline_rules_in_their_order():
    f = SC.form
    assert f("f32", 0, 16, 128, CUS)["status"] == SC.EINVAL and f("f32", 8, 0, 128, CUS)["status"] == SC.EINVAL
    assert f("f32", 8, 16, 0, CUS)["status"] == SC.EINVAL
    assert f("f32", 8, 64, 66, CUS) == {"decline": "B % V != 0", "status": SC.EUNSUPPORTED}
    assert f("f64", 8, 32, 65, CUS)["decline"] == "B % V != 0" and "decline" not in f("f64", 8, 64, 66, CUS)
    assert f("f32", 8, 1, 2044, CUS)["decline"] == "P < stride / 2" and "decline" not in f("f32", 8, 1, 2048, CUS)
    assert f("f64", 8, 1, 1022, CUS)["decline"] == "P < stride / 2" and "decline" not in f("f64", 8, 1, 1024, CUS)
    assert f("f32", 8, 1 << 16, 1 << 15, CUS)["decline"] == "P >= 2^31"
    assert f("f32", 8, 16, 128, CUS, aligned=False)["decline"] == "X not 16-byte aligned"
    assert f("f32", 8, 64, 66, CUS, aligned=False)["decline"] == "B % V != 0"            # the first rule that applies
    assert f("f32", 8, 513, 512, CUS)["decline"] == "G = 17 > 16" and f("f64", 8, 512, 512, CUS)["decline"] == "G = 32 > 16"
    # fewer compute units than slabs: no row stream at all
    assert f("f32", 37, 512, 512, 15)["decline"] == "S < 1" and f("f32", 37, 512, 512, 16)["S"] == 1
    assert f("f32", 37, 512, 512, 40)["S"] == 2 and f("f32", 37, 513, 512, 15)["decline"] == "G = 17 > 16"
    assert f("f64", 200, 256, 256, 7)["decline"] == "S < 1"
    for dt in DTYPES:
        for shape, _, _ in SC.SPLIT_CASES:
            SC.check_claim(dt, shape, 8)                          # on a card with 8 compute units every G > 8 case is a decline


def _exact(v):
    """A longdouble as a Fraction: its float64 head and the (exactly representable) rest."""
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - np.longdouble(hi)))


def test_the_reference_is_the_exact_value_on_a_small_case():
    """t, Z and sum(c) of a 5 x (3 x 8) case against exact rational arithmetic: the longdouble reference is within 2^-58 of
    sum|terms|, 32 times closer than one float64 rounding."""
    assert SC.LONGDOUBLE_IS_WIDER and np.finfo(np.longdouble).nmant >= 63
    d = SC.make_case("f64", 5, 3, 8)
    ref = SC.reference(d["x"], 3, 8, d["wA"], d["wB"], SC.SHIFT, d["sub_own"], d["add_other"], SC.ALPHA_COUPLED)
    F = Fraction
    x = [[F(v) for v in row] for row in d["x"]]
    w = [F(a) * F(b) for a in d["wA"] for b in d["wB"]]
    t = [sum(xi * wi for xi, wi in zip(row, w)) - F(SC.SHIFT) - F(s) for row, s in zip(x, d["sub_own"])]
    c = [F(SC.ALPHA_COUPLED) * (ti + F(o)) for ti, o in zip(t, d["add_other"])]
    for i in range(5):
        mag = sum(abs(xi * wi) for xi, wi in zip(x[i], w)) + F(SC.SHIFT) + abs(F(d["sub_own"][i]))
        assert abs(_exact(ref["t"][i]) - t[i]) <= F(2) ** -58 * mag
    for col in range(24):
        z = sum(c[i] * x[i][col] for i in range(5))
        mag = sum(abs(c[i] * x[i][col]) for i in range(5))
        assert abs(_exact(ref["Z"][col]) - z) <= F(2) ** -58 * mag
    assert abs(_exact(ref["csum"]) - sum(c)) <= F(2) ** -58 * sum(abs(v) for v in c)


def _calls(d):
    return {"plain": (SC.SHIFT, None, None, 1.0), "coupled": (SC.SHIFT, d["sub_own"], d["add_other"], SC.ALPHA_COUPLED)}


_BOUND_PARAMS = [pytest.param(dt, c[0], id=f"{dt}-{'x'.join(map(str, c[0]))}") for dt in DTYPES for c in SC.ALL_CASES
                 if SC.instance(SC.form(dt, *c[0], cus=CUS)) is not None]


@pytest.mark.parametrize("dt,shape", _BOUND_PARAMS)
def test_float64_sums_in_three_orders_stay_inside_the_bounds(dt, shape):
    """Every case that runs on the device, both calls, no case and no element left out: NumPy's own order against the reference
    and -- the orders a kernel is free to take -- the sums reversed and in chunks of 4096 terms.  Cases above 5 Mi elements
    ((37, 512, 512), (37, 257, 512), (129 | 200, 256, 256), (70, 3, 43000)) take the two extra orders on their first 16 rows
    only, as a case of their own with its own reference (the row length, which sets the bound of t, is the whole one)."""
    I, A, B = shape
    d = SC.make_case(dt, I, A, B)
    big = I * A * B > (5 << 20)
    for name, (sh, sub, oth, alpha) in _calls(d).items():
        ref = SC.reference(d["x"], A, B, d["wA"], d["wB"], sh, sub, oth, alpha)
        assert np.all(ref["bt"] > 0) and np.all(ref["bZ"] > 0) and ref["bc"] > 0
        for order in ("forward",) if big else ORDERS:
            t, Z, cs = SC.evaluate_f64(d["x"], A, B, d["wA"], d["wB"], sh, sub, oth, alpha, order)
            r = SC.ratios(ref, t, Z, cs)
            assert SC.within(r), (dt, shape, name, order, r)
    if big:
        sh, sub, oth, alpha = _calls(d)["coupled"]
        x, sub, oth = d["x"][:16], sub[:16], oth[:16]
        ref = SC.reference(x, A, B, d["wA"], d["wB"], sh, sub, oth, alpha)
        for order in ORDERS[1:]:
            r = SC.ratios(ref, *SC.evaluate_f64(x, A, B, d["wA"], d["wB"], sh, sub, oth, alpha, order))
            assert SC.within(r), (dt, shape, "first 16 rows", order, r)


def test_a_nan_in_any_one_output_fails_the_check():
    """`within` is what every bound assertion goes through: a NaN in t alone, in Z alone or in csum alone must fail it (max() of the
    ratios would keep a NaN only if it came first)."""
    I, A, B = 20, 8, 256
    d = SC.make_case("f64", I, A, B)
    sh, sub, oth, alpha = _calls(d)["coupled"]
    ref = SC.reference(d["x"], A, B, d["wA"], d["wB"], sh, sub, oth, alpha)
    t, Z, cs = SC.evaluate_f64(d["x"], A, B, d["wA"], d["wB"], sh, sub, oth, alpha, "forward")
    assert SC.within(SC.ratios(ref, t, Z, cs)) and SC.within(SC.ratios(ref, t, Z))
    nan = float("nan")
    for bad_t, bad_Z, bad_cs in ((True, False, False), (False, True, False), (False, False, True)):
        t2, Z2 = t.copy(), Z.copy()
        if bad_t:
            t2[I - 1] = nan
        if bad_Z:
            Z2[A * B - 1] = nan
        r = SC.ratios(ref, t2, Z2, nan if bad_cs else cs)
        assert not SC.within(r), r
        assert sum(v != v for v in r.values()) == 1
    assert not SC.within(SC.ratios(ref, t, Z * (1.0 + 1e-9), cs)) and not SC.within(SC.ratios(ref, t, Z, cs * (1.0 + 1e-9)))


def test_the_bounds_notice_one_wrong_loading_and_one_dropped_row():
    """The bounds are tight enough to bite: one mode-1 loading taken from the neighbouring slice, or one row left out of Z,
    is thousands of bounds away."""
    I, A, B = 60, 8, 2048
    d = SC.make_case("f64", I, A, B)
    ref = SC.reference(d["x"], A, B, d["wA"], d["wB"], SC.SHIFT, None, None, 1.0)
    wrong = d["wA"].copy()
    wrong[3] = d["wA"][4]
    t, Z, cs = SC.evaluate_f64(d["x"], A, B, wrong, d["wB"], SC.SHIFT, None, None, 1.0, "forward")
    assert SC.ratios(ref, t, Z, cs)["t"] > 1e3
    t, Z, cs = SC.evaluate_f64(d["x"][:-1], A, B, d["wA"], d["wB"], SC.SHIFT, None, None, 1.0, "forward")
    ref1 = {k: (v[:-1] if k in ("t", "bt") else v) for k, v in ref.items()}
    r = SC.ratios(ref1, t, Z, cs)
    assert r["t"] <= 1.0 and r["Z"] > 1e3 and r["csum"] > 1e3
