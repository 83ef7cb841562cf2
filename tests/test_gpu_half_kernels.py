"""The kernels that read 16-bit X (bfloat16 / float16) in place: cmtfpls_{xcov, xcov_stats, score_contract, mttkrp}_{bf16, f16}.

Random data is quantised to the storage type on the host and upcast to float64 (exact); the references and the elementwise
bounds are those of the f32 / f64 kernels on the upcast values (tests/half_storage_ref.py, matrix_core_ref.f64_bound,
score_contract_ref.reference): after the conversion on load the kernels ARE the float64 arithmetic of the existing entries, so the
bounds depend on the float64 accumulation only.  Every comparison asserts error / bound <= 1, a second call gives the same bits,
and the 16-bit tensor is bit-identical afterwards (it is only ever read).

  xcov / xcov_stats   I in {1, 37, 300} (300 rows: five row blocks of 64), P in {7 (scalar loads), 8 (one vector per lane group),
                      24, 264, 520 (second / third column tile with a remainder)}, M in {1, 17, 64}, ldy > M; masked with a NaN
                      in the last column; in stats a NaN makes its column's sum NaN and an Inf (f16) makes it non-finite
  score_contract      (16, 256) <NV 1, KC>, (128, 128) <NV 2, KC>, (171, 24) <NV 1, no KC, lanes without a vector>, (400, 24) <NV 2,
                      no KC, lanes whose second vector does not exist>;
                      I in {1, 2, 257, 700}; a plain call (no shift / sub_own / add_other / csum, alpha = 1) and a coupled call (all
                      present, alpha = 0.5); declines: B = 20, P one vector below / above the window, a misaligned view
  mttkrp              (16, 64), (5, 24), (1, 40) x R in {1, 10, 17, 32} x I in {1, 300}, ldo > R; R = 33 and loadings beyond the
                      LDS decline exactly as the f32 entry does
  arguments           null pointers and non-positive extents give CMTFPLS_EINVAL (nothing is launched)

Worst error / bound, printed by every run; on an MI355X (also in DESIGN.md, section 8w):
  xcov 0.081 (bf16) / 0.061 (f16); masked 0 (one row block adds in the reference's order); xcov_stats S the same, sums and sums of
  squares 0 (sums of 8- / 11-bit values are exact in float64); score_contract t 7.4e-5, Z 4.7e-5, csum 2.7e-5 (NV 2 without KC included); mttkrp 0.079 / 0.077
"""
import numpy as np
import pytest
import torch

import half_storage_ref as HS
import matrix_core_ref as MC
import score_contract_ref as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
SENTINEL = -7.25e300
EINVAL, EUNSUPPORTED = 1, 4


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k, e in sorted(_worst.items()):
        print(f"worst error / bound {k}: {e:.3g}")
    torch.cuda.empty_cache()


def _note(key, r):
    prev = _worst.get(key, 0.0)
    _worst[key] = float("nan") if (r != r or prev != prev) else max(prev, r)
    return r


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=F64, device=DEV).contiguous()


def _ratio(got, want, bound):
    """Worst |got - want| / bound over the entries (host float64 arrays); a NaN in `got` gives NaN, which fails `<= 1`."""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - want) / bound
    return float("nan") if np.isnan(r).any() else float(r.max())


def _case(kind, I, P, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((I, P)) * np.exp(rng.uniform(-2.0, 2.0, size=P)) + 0.5
    q, up = HS.quantise(x, kind)
    assert HS.is_exact_upcast(up, kind)
    Xd = q.to(DEV)
    assert np.array_equal(Xd.double().cpu().numpy(), up)             # the device holds exactly the reference's operand
    return Xd, up


# ---- S = Y^T X_(0) and the column statistics ------------------------------------------------------------------------------------
XCOV_I, XCOV_P, XCOV_M = (1, 37, 300), (7, 8, 24, 264, 520), (1, 17, 64)


@pytest.mark.parametrize("P", XCOV_P)
@pytest.mark.parametrize("kind", HS.KINDS)
def test_xcov_and_stats_against_float64_on_the_upcast_values(be, kind, P):
    tiny = np.finfo(np.float64).tiny
    for I in XCOV_I:
        Xd, up = _case(kind, I, P, 7919 * I + P)
        keep = Xd.view(torch.int16).clone()
        assert MC.plan_xcov(I, P)[2] == (5 if I == 300 else 1)
        for M in XCOV_M:
            rng = np.random.default_rng(I + 31 * M)
            Yh = rng.standard_normal((I, M))
            wide = torch.zeros(I, M + 2, dtype=F64, device=DEV)
            wide[:, :M] = _dev(Yh)
            Y = wide[:, :M]                                                 # ldy = M + 2
            ref = HS.xcov_reference(up, Yh)
            coeff = MC.f64_bound(I)
            S = be.xcov(Xd, Y, False, out=torch.full((M, P), SENTINEL, dtype=F64, device=DEV))
            assert S is not None
            r = _note(f"xcov {kind}", _ratio(S.cpu().numpy(), ref["S"], coeff * ref["magS"] + tiny))
            S2 = be.xcov(Xd, Y, False, out=torch.empty(M, P, dtype=F64, device=DEV))
            assert torch.equal(S.view(torch.int64), S2.view(torch.int64)), "a second call gives other bits"
            out = be.xcov_stats(Xd, Y, out=torch.full((M, P), SENTINEL, dtype=F64, device=DEV))
            assert out is not None
            St, stats = out
            rs = [_note(f"xcov_stats {kind} S", _ratio(St.cpu().numpy(), ref["S"], coeff * ref["magS"] + tiny)),
                  _note(f"xcov_stats {kind} sums", _ratio(stats[:P].cpu().numpy(), ref["sum"], coeff * ref["magsum"] + tiny)),
                  _note(f"xcov_stats {kind} sums of squares", _ratio(stats[P:].cpu().numpy(), ref["sq"], coeff * ref["sq"] + tiny))]
            out2 = be.xcov_stats(Xd, Y, out=torch.empty(M, P, dtype=F64, device=DEV))
            assert torch.equal(St.view(torch.int64), out2[0].view(torch.int64)) and torch.equal(stats.view(torch.int64), out2[1].view(torch.int64))
            print(f"xcov {kind} I={I} P={P} M={M}: error / bound {r:.3g}; stats {max(rs):.3g}")
            assert r <= 1.0 and all(v <= 1.0 for v in rs)
        assert torch.equal(Xd.view(torch.int16), keep), "the 16-bit tensor was written"


@pytest.mark.parametrize("P", (7, 264))
@pytest.mark.parametrize("kind", HS.KINDS)
def test_xcov_masked_and_what_the_statistics_show_of_a_missing_value(be, kind, P):
    I, M = 37, 17
    Xd, up = _case(kind, I, P, 104729 + P)
    Xd[5, P - 1] = float("nan")
    up[5, P - 1] = np.nan
    Yh = np.random.default_rng(5).standard_normal((I, M))
    Y = _dev(Yh)
    ref = HS.xcov_reference(np.nan_to_num(up, nan=0.0), Yh)
    S = be.xcov(Xd, Y, True, out=torch.empty(M, P, dtype=F64, device=DEV))
    r = _note(f"xcov masked {kind}", _ratio(S.cpu().numpy(), ref["S"], MC.f64_bound(I) * ref["magS"] + np.finfo(np.float64).tiny))
    assert r <= 1.0
    St, stats = be.xcov_stats(Xd, Y, out=torch.empty(M, P, dtype=F64, device=DEV))
    sums = stats[:P].cpu().numpy()
    assert np.isnan(sums[P - 1]) and np.isfinite(sums[:P - 1]).all()            # the NaN shows in its own column only
    clean = HS.xcov_reference(up[:, :P - 1], Yh)
    assert _ratio(sums[:P - 1], clean["sum"], MC.f64_bound(I) * clean["magsum"]) <= 1.0
    if kind == "f16":                                                           # an infinity is a value of the type
        Xd[5, P - 1] = float("inf")
        _, stats = be.xcov_stats(Xd, Y, out=torch.empty(M, P, dtype=F64, device=DEV))
        s = stats.cpu().numpy()
        assert not np.isfinite(s[P - 1]) and np.isfinite(s[:P - 1]).all()
        n = float(I)
        with np.errstate(invalid="ignore"):
            assert not np.isfinite((s[P:] - s[:P] * s[:P] / n).sum())           # what the fit tests before it goes on in place


# ---- t = X w - ..., Z = X^T c in one read ---------------------------------------------------------------------------------------
# (A, B) -> (NV, KC).  (400, 24): 9600 elements, lanes 176.. have no second vector and every vector its own mode-2 loadings
SC_SHAPES = {(16, 256): (1, True), (128, 128): (2, True), (171, 24): (1, False), (400, 24): (2, False)}
SC_I = (1, 2, 257, 700)


@pytest.mark.parametrize("I", SC_I)
@pytest.mark.parametrize("AB", list(SC_SHAPES), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", HS.KINDS)
def test_score_contract_against_the_longdouble_reference(be, kind, AB, I):
    A, B = AB
    P = A * B
    V, lo, hi = HS.window(kind)
    nv, kc = SC_SHAPES[AB]
    assert B % V == 0 and lo <= P <= hi and -(-P // HS.SC_STRIDE) == nv and (HS.SC_STRIDE % B == 0) == kc
    d = SC.make_case("f64", I, A, B)
    q, up = HS.quantise(d["x"], kind)
    Xd = q.to(DEV)
    keep = Xd.view(torch.int16).clone()
    g = {k: _dev(d[k]) for k in ("wA", "wB", "sub_own", "add_other")}
    sh = _dev([SC.SHIFT])
    for coupled in (False, True):
        kw = dict(sub_own=g["sub_own"], add_other=g["add_other"], alpha=SC.ALPHA_COUPLED) if coupled else {}
        shift = sh if coupled else None
        ref = SC.reference(up, A, B, d["wA"], d["wB"], SC.SHIFT if coupled else None, d["sub_own"] if coupled else None,
                           d["add_other"] if coupled else None, SC.ALPHA_COUPLED if coupled else 1.0)
        runs = []
        for _ in range(2):
            tf = torch.full((I + 8,), SENTINEL, dtype=F64, device=DEV)
            Zf = torch.full((P + 8,), SENTINEL, dtype=F64, device=DEV)
            cs = torch.full((1,), SENTINEL, dtype=F64, device=DEV) if coupled else None
            got = be.score_contract(Xd, A, B, g["wA"], g["wB"], shift, tf[:I], Zf[:P], csum=cs, **kw)
            assert got is not None, "a shape of the rows form was declined"
            assert bool((tf[I:] == SENTINEL).all()) and bool((Zf[P:] == SENTINEL).all())
            runs.append((tf[:I].clone(), Zf[:P].clone(), cs))
        assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))
        assert torch.equal(runs[0][1].view(torch.int64), runs[1][1].view(torch.int64))
        t, Z, cs = runs[0]
        r = SC.ratios(ref, t.cpu().numpy(), Z.cpu().numpy(), None if cs is None else float(cs.item()))
        for k, v in r.items():
            _note(f"score_contract {kind} <{nv}, {'KC' if kc else 'noKC'}> {k}", v)
        print(f"score_contract {kind} {(I, A, B)} coupled={coupled}: error / bound {r}")
        assert SC.within(r), r
    assert torch.equal(Xd.view(torch.int16), keep), "the 16-bit tensor was written"


@pytest.mark.parametrize("kind", HS.KINDS)
def test_score_contract_declines_outside_the_rows_form(be, kind):
    V, lo, hi = HS.window(kind)
    I = 3

    def call(X, A, B):
        w = torch.ones(max(A, B), dtype=F64, device=DEV)
        return be.score_contract(X, A, B, w[:A], w[:B], None, torch.empty(I, dtype=F64, device=DEV),
                                 torch.empty(A * B, dtype=F64, device=DEV))

    def zeros(P):
        return torch.zeros(I, P, dtype=HS.TORCH[kind], device=DEV)

    assert call(zeros(256 * 20), 256, 20) is None                            # B % 8 != 0
    assert call(zeros(lo - V), (lo - V) // V, V) is None                     # one vector below the window
    assert call(zeros(lo), lo // V, V) is not None
    assert call(zeros(hi), hi // V, V) is not None
    assert call(zeros(hi + V), (hi + V) // V, V) is None                     # one vector above: no split form at 16 bits
    flat = torch.zeros(I * lo + 8, dtype=HS.TORCH[kind], device=DEV)
    view = flat[1:1 + I * lo].view(I, lo)                                    # one element past a 16-byte boundary
    assert view.is_contiguous() and view.data_ptr() % 16 == 2
    assert call(view, lo // V, V) is None


# ---- M = X_(0) (WA (.) WB) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("AB", [(16, 64), (5, 24), (1, 40)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", HS.KINDS)
def test_mttkrp_against_float64_on_the_upcast_values(be, kind, AB):
    A, B = AB
    P = A * B
    for I in (1, 300):
        Xd, up = _case(kind, I, P, 15485863 + 17 * I + P)
        keep = Xd.view(torch.int16).clone()
        for R in (1, 10, 17, 32):
            rng = np.random.default_rng(R + P)
            WA, WB = rng.standard_normal((A, R)) + 0.25, rng.standard_normal((B, R)) - 0.125
            want, mag = HS.mttkrp_reference(up, A, B, WA, WB)
            runs = []
            for _ in range(2):
                wide = torch.full((I, R + 3), SENTINEL, dtype=F64, device=DEV)
                out = wide[:, 2:2 + R]                                           # ldo = R + 3
                assert be.mttkrp(Xd, A, B, _dev(WA), _dev(WB), out) is not None
                assert bool((wide[:, :2] == SENTINEL).all()) and bool((wide[:, 2 + R:] == SENTINEL).all())
                runs.append(out.clone())
            assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))
            r = _note(f"mttkrp {kind}", _ratio(runs[0].cpu().numpy(), want, MC.f64_bound(P) * mag + np.finfo(np.float64).tiny))
            print(f"mttkrp {kind} {(I, A, B)} R={R}: error / bound {r:.3g}")
            assert r <= 1.0
        assert torch.equal(Xd.view(torch.int16), keep)


@pytest.mark.parametrize("kind", HS.KINDS)
def test_mttkrp_declines_where_the_f32_entry_declines(be, kind):
    I = 4
    for (A, B, R) in [(4, 8, 33), (1, 1300, 1), (8, 1209, 16)]:                 # R > 32; (A + B) 128 B > 152 KB
        assert MC.mttkrp_instance("f32", I, A, B, R) is None
        WA, WB = torch.ones(A, R, dtype=F64, device=DEV), torch.ones(B, R, dtype=F64, device=DEV)
        out = torch.empty(I, R, dtype=F64, device=DEV)
        assert be.mttkrp(torch.zeros(I, A * B, dtype=torch.float32, device=DEV), A, B, WA, WB, out) is None
        assert be.mttkrp(torch.zeros(I, A * B, dtype=HS.TORCH[kind], device=DEV), A, B, WA, WB, out) is None
    A, B, R = 8, 1208, 16                                                       # the last shape that fits: accepted by both
    assert MC.mttkrp_instance("f32", I, A, B, R) is not None
    WA, WB = torch.ones(A, R, dtype=F64, device=DEV), torch.ones(B, R, dtype=F64, device=DEV)
    out = torch.empty(I, R, dtype=F64, device=DEV)
    X = torch.ones(I, A * B, dtype=HS.TORCH[kind], device=DEV)
    assert be.mttkrp(X, A, B, WA, WB, out) is not None
    assert bool((out == float(A * B)).all())


# ---- argument checks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", HS.KINDS)
def test_c_entries_check_their_arguments_before_anything_is_read(be, kind):
    lib = be.lib
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    X = torch.zeros(4, 4096, dtype=HS.TORCH[kind], device=DEV)
    d = torch.zeros(8192, dtype=F64, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    x, p, w = X.data_ptr(), d.data_ptr(), ws.data_ptr()
    fx = getattr(lib, f"cmtfpls_xcov_{kind}")
    assert fx(None, 4, 4096, p, 1, 1, p, 0, w, ws.numel(), st) == EINVAL
    assert fx(x, 4, 4096, None, 1, 1, p, 0, w, ws.numel(), st) == EINVAL
    assert fx(x, -4, 4096, p, 1, 1, p, 0, w, ws.numel(), st) == EINVAL
    assert fx(x, 4, 0, p, 1, 1, p, 0, w, ws.numel(), st) == EINVAL
    assert fx(x, 4, 4096, p, 1, 2, p, 0, w, ws.numel(), st) == EINVAL          # ldy < M
    fs = getattr(lib, f"cmtfpls_xcov_stats_{kind}")
    assert fs(None, 4, 4096, p, 1, 1, p, p, w, ws.numel(), st) == EINVAL
    assert fs(x, 4, 4096, p, 1, 1, p, None, w, ws.numel(), st) == EINVAL
    assert fs(x, 4, -1, p, 1, 1, p, p, w, ws.numel(), st) == EINVAL
    assert fs(x, 4, 4096, p, 65, 65, p, p, w, ws.numel(), st) == EUNSUPPORTED
    fc = getattr(lib, f"cmtfpls_score_contract_{kind}")
    assert fc(None, 4, 16, 256, p, p, None, None, None, 1.0, p, p, None, w, ws.numel(), st) == EINVAL
    assert fc(x, 4, 16, 256, None, p, None, None, None, 1.0, p, p, None, w, ws.numel(), st) == EINVAL
    assert fc(x, 0, 16, 256, p, p, None, None, None, 1.0, p, p, None, w, ws.numel(), st) == EINVAL
    assert fc(x, 4, -16, 256, p, p, None, None, None, 1.0, p, p, None, w, ws.numel(), st) == EINVAL
    fm = getattr(lib, f"cmtfpls_mttkrp_{kind}")
    assert fm(None, 4, 16, 256, p, p, 1, p, 1, st) == EINVAL
    assert fm(x, 4, 16, 256, p, None, 1, p, 1, st) == EINVAL
    assert fm(x, 4, 16, -256, p, p, 1, p, 1, st) == EINVAL
    assert fm(x, 4, 16, 256, p, p, 2, p, 1, st) == EINVAL                      # ldo < R
    torch.cuda.synchronize()
