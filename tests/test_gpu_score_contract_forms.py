"""The one-read score and contraction kernel (be.score_contract, cmtfpls_score_contract_{f32,f64}, csrc/scorecontract.hip) in
every form its host dispatch can select, against an np.longdouble reference of the same storage-rounded operands with
per-element bounds:

  t = X w - shift - sub_own,   c = alpha (t + add_other),   Z = X^T c,   csum = sum(c)

tests/score_contract_ref.py mirrors run_score_contract line by line; every case re-derives its instance from the device's own
compute-unit count, asserts that it is the one the table names (on a card with fewer compute units than slabs: a decline) and
that the library's workspace size is the mirror's and covers what the entry checks.

score_contract_rows_kernel<T, NV, KC, WL>  (I, A, B)      f32 instance          f64 instance
  (300, 25, 100)                                          <1, noKC>             <2, noKC>
  (300, 12, 340)      B > stride / 8                      <1, noKC>             <2, noKC>
  (300, 1, 2044)                                          declined P < 2048     <1, noKC>
  (513, 64, 128)      2 or 3 rows per workgroup           <2, KC>               <4, KC>
  (300, 41, 100)      f64: one wholly absent vector       <2, noKC>             <4, noKC>
  (300, 150, 100)     full registers without KC           <4, noKC>             <8, noKC>
  (100, 120, 128)     P != 8 stride                       <4, KC>               <8, KC>
  (100, 4096, 4)      A > kScLdsA; B = V for f32          <4, KC>               <8, KC>
  (60, 2048, 8)       wls[] full (A = kScLdsA)            <4, KC>               <8, KC, WL>
  (60, 8, 2048)       jstep = 1                           <4, KC>               <8, KC, WL>
  (64, 16, 128)       P = stride / 2 for f32              <1, KC>               <1, KC>
  (255 | 256 | 512, 32, 128)   1, 1, 2 rows / workgroup   <1, KC>               <2, KC>
  (769, 1, 2048)      3 or 4 rows per workgroup           <1, KC>               <1, KC>
  (1025, 8, 256)      4 or 5 rows per workgroup           <1, KC>               <1, KC>
score_contract_split_kernel<T, NVS, KC, LAG> and G (at >= 256 compute units)
  (40, 160, 128)      one row per stream                  <4, KC, 1> G 2        <4, KC, 2> G 3
  (60, 2049, 8)       the last slab almost empty          <4, KC, 1> G 2        <4, KC, 2> G 3
  (70, 5, 3300)                                           <2, noKC, 2> G 3      <4, noKC, 1> G 3
  (70, 5, 6500)       S = 64: 1 and 2 rows per stream     <2, noKC, 2> G 4      <4, noKC, 1> G 4
  (37, 512, 512)                                          <4, KC, 1> G 16       declined G = 32
  (37, 256, 512)                                          <4, KC, 1> G 8        <4, KC, 2> G 16
  (37, 257, 512)                                          <4, KC, 1> G 9        declined G = 17
  (37, 513, 512)                                          declined G = 17       declined G = 33
  (33, 1, 131072)     a matrix block at the limit         <2, noKC, 2> G 16     <4, noKC, 1> G 16
  (33, 1, 131074)                                         declined B % 4 != 0   declined G = 17
  (70, 3, 43000)      4 or 5 rows per stream              <2, noKC, 2> G 16     <4, noKC, 1> G 16
  (1 | 16 | 17 | 33 | 65 | 129 | 200, 256, 256)           <4, KC, 1> G 4        <4, KC, 2> G 8
                      the north-star row: I = 1, I <= S, I = S + 1 (f32 S = 64, f64 S = 32), 2 .. 7 rows per stream
These are all 19 instances the dispatch can select (8 for f32, 11 for f64; test_score_contract_ref_cpu.py finds the same set by
enumeration), and for each of the four split instances every remainder of (rows per stream + LAG) mod (LAG + 2), i.e. every
exit of the step loop that is unrolled LAG + 2 times.

  elsewhere      larger I and the comparison with score + mode0_contract: test_gpu_round3.py::test_score_contract_kernel_equals_
                 the_two_passes; the fits that run through the kernel: test_gpu_round3.py::test_xcov_fit_with_one_read_per_
                 component_equals_the_two_reads.
  unreachable    the P >= 2^31 decline (rows of 8 GB and more); the S < 1 decline needs a card with fewer compute units than
                 slabs (the mirror then asserts it in place of the instance); score_contract_rows_kernel<float, 8, *> is never
                 instantiated (kMaxNV = 4 for f32).

Every case, both storage types: a plain call (no sub_own / add_other, alpha = 1, no csum) and a coupled call (sub_own, add_other,
alpha = 0.5, csum), t, Z and csum within the elementwise bounds of score_contract_ref; a second call gives the same bits; X
is bit-identical afterwards; t and Z are views of buffers 8 doubles longer whose tails keep their sentinel.

Worst |error| / bound per instance over t, Z and csum of both calls, printed by every run; on an MI355X (256 compute units):
  f32  rows <1, KC> 1.2e-4   <1, noKC> 6.7e-5   <2, KC> 1.5e-5   <2, noKC> 3.9e-5   <4, KC> 6.3e-6   <4, noKC> 6.3e-6
       split <4, KC, 1> 5.3e-6   <2, noKC, 2> 4.6e-6
  f64  rows <1, KC> 1.2e-4   <1, noKC> 8.7e-5   <2, KC> 4.4e-5   <2, noKC> 6.7e-5   <4, KC> 1.5e-5   <4, noKC> 3.8e-5
       <8, KC> 6.1e-6   <8, noKC> 6.1e-6   <8, KC, WL> 5.7e-6      split <4, KC, 2> 3.8e-6   <4, noKC, 1> 3.6e-6
(far below 1, as expected of a worst-case bound on sums of thousands of randomly signed roundings.  What the bound is for is
what it rejects: one wrong loading or one dropped row is > 1000 bounds, test_score_contract_ref_cpu.py.)
"""
import numpy as np
import pytest
import torch

import score_contract_ref as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
TDT = {"f32": F32, "f64": F64}
SENTINEL = -7.25e300
TAIL = 8
DTYPES = ("f32", "f64")


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report_and_release():
    yield
    for k, e in sorted(_worst.items()):
        print(f"worst error / bound {k}: {e:.3g}")
    torch.cuda.empty_cache()


def _dev(a, dtype=F64):
    return torch.as_tensor(a, dtype=dtype, device=DEV).contiguous()


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int64)


def _outputs(I, P):
    """t and Z as the leading views of buffers TAIL doubles longer, everything preset to the sentinel."""
    tf = torch.full((I + TAIL,), SENTINEL, dtype=F64, device=DEV)
    Zf = torch.full((P + TAIL,), SENTINEL, dtype=F64, device=DEV)
    return tf, Zf


def _untouched(*bufs):
    return all(bool((b == SENTINEL).all()) for b in bufs)


def _name(dt, f):
    inst = SC.instance(f)
    return f"{dt} {inst[0]}<{inst[1]}, {'KC' if inst[2] else 'noKC'}, {'WL' if inst[3] is True else inst[3] if inst[0] == 'split' else '-'}>"


def _record(dt, f, r):
    k = _name(dt, f)
    vals = list(r.values()) + [_worst.get(k, 0.0)]
    _worst[k] = float("nan") if any(v != v for v in vals) else max(vals)          # (a NaN stays)


def _operands(dt, shape):
    I, A, B = shape
    d = SC.make_case(dt, I, A, B)
    X = _dev(d["x"], TDT[dt])
    assert np.array_equal(X.double().cpu().numpy(), d["x"])                     # the storage holds exactly the reference's operand
    return d, X, {k: _dev(d[k]) for k in ("wA", "wB", "sub_own", "add_other")}, _dev([SC.SHIFT])


def _call(be, X, A, B, g, sh, coupled, tf, Zf, cs):
    I, P = X.shape
    kw = dict(sub_own=g["sub_own"], add_other=g["add_other"], alpha=SC.ALPHA_COUPLED, csum=cs) if coupled else {}
    return be.score_contract(X, A, B, g["wA"], g["wB"], sh, tf[:I], Zf[:P], **kw)


_CASE_PARAMS = [pytest.param(dt, c[0], id=f"{dt}-{'x'.join(map(str, c[0]))}") for c in SC.ALL_CASES for dt in DTYPES]


@pytest.mark.parametrize("dt,shape", _CASE_PARAMS)
def test_every_form_against_the_longdouble_reference(be, cus, dt, shape):
    I, A, B = shape
    P = A * B
    f = SC.check_claim(dt, shape, cus)                           # the instance the table names, from this card's compute units
    nbytes = be.lib.cmtfpls_score_contract_workspace_bytes(I, P)
    assert nbytes == SC.workspace_bytes(I, P)
    tf, Zf = _outputs(I, P)
    if "decline" in f:
        X = torch.zeros(I, P, dtype=TDT[dt], device=DEV)
        w = torch.ones(max(A, B), dtype=F64, device=DEV)
        g = {"wA": w[:A], "wB": w[:B], "sub_own": w[:1].expand(I).contiguous(), "add_other": w[:1].expand(I).contiguous()}
        for coupled in (False, True):
            assert _call(be, X, A, B, g, None, coupled, tf, Zf, be.empty(1) if coupled else None) is None, f
        assert _untouched(tf, Zf)
        print(f"{dt} {shape}: declined, {f['decline']}")
        return
    assert nbytes >= f["need"]
    d, X, g, sh = _operands(dt, shape)
    keep = X.clone()
    for coupled in (False, True):
        ref = SC.reference(d["x"], A, B, d["wA"], d["wB"], SC.SHIFT, d["sub_own"] if coupled else None,
                           d["add_other"] if coupled else None, SC.ALPHA_COUPLED if coupled else 1.0)
        cs = torch.full((1,), SENTINEL, dtype=F64, device=DEV) if coupled else None
        tf.fill_(SENTINEL)
        Zf.fill_(SENTINEL)
        assert _call(be, X, A, B, g, sh, coupled, tf, Zf, cs) is not None
        t, Z = tf[:I].clone(), Zf[:P].clone()
        assert _untouched(tf[I:], Zf[P:])
        r = SC.ratios(ref, t.cpu().numpy(), Z.cpu().numpy(), float(cs.item()) if coupled else None)
        print(f"{dt} {shape} {_name(dt, f)} G={f.get('G')} {'coupled' if coupled else 'plain'}: error / bound "
              + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
        _record(dt, f, r)
        assert SC.within(r), (dt, shape, f, r)                  # (value by value: a NaN anywhere fails)
        # again: the same bits (the split form's exchange slots are preset afresh by every call)
        tf.fill_(SENTINEL)
        Zf.fill_(SENTINEL)
        cs2 = torch.full((1,), SENTINEL, dtype=F64, device=DEV) if coupled else None
        assert _call(be, X, A, B, g, sh, coupled, tf, Zf, cs2) is not None
        assert torch.equal(_bits(tf[:I]), _bits(t)) and torch.equal(_bits(Zf[:P]), _bits(Z)) and _untouched(tf[I:], Zf[P:])
        assert not coupled or torch.equal(_bits(cs2), _bits(cs))
    assert torch.equal(_bits(X), _bits(keep))


# ---- robustness: one NaN in X ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape", SC.NAN_CASES, ids=["rows", "split"])
def test_a_nan_in_one_row_stays_in_that_row_of_t(be, cus, dt, shape):
    """A NaN partial dot product is published and summed like any other value: the split form's "slot not yet written"
    pattern (all ones) is a NaN too, and must be confused neither with a computed NaN nor make a partner give up waiting --
    which would show as NaN in OTHER rows of t.  Z = X^T c is NaN in every column (NaN times anything)."""
    I, A, B = shape
    P = A * B
    f = SC.form(dt, I, A, B, cus)
    assert f.get("form") == ("rows", "split")[SC.NAN_CASES.index(shape)]
    d, X, g, sh = _operands(dt, shape)
    row, col = I // 2 + 1, P - 3                                # (the split form: in the last slab)
    X[row, col] = float("nan")
    ref = SC.reference(d["x"], A, B, d["wA"], d["wB"], SC.SHIFT, None, None, 1.0)
    tf, Zf = _outputs(I, P)
    assert _call(be, X, A, B, g, sh, False, tf, Zf, None) is not None
    t = tf[:I].cpu().numpy()
    assert np.isnan(t[row]) and not np.isnan(np.delete(t, row)).any(), np.flatnonzero(np.isnan(t))
    others = np.arange(I) != row
    assert np.max(np.abs(t[others].astype(np.longdouble) - ref["t"][others]) / ref["bt"][others]) <= 1.0
    assert bool(torch.isnan(Zf[:P]).all()) and _untouched(tf[I:], Zf[P:])


# ---- the host contract, through the C entry itself -----------------------------------------------------------------------------
def _entry(be, dt):
    return getattr(be.lib, f"cmtfpls_score_contract_{dt}")


def _raw(be, dt, X, I, A, B, wA, wB, sh, sub, oth, alpha, t, Z, cs, ws, ws_bytes):
    p = lambda v: None if v is None else v.data_ptr()          # noqa: E731
    rc = _entry(be, dt)(p(X), I, A, B, p(wA), p(wB), p(sh), p(sub), p(oth), float(alpha), p(t), p(Z), p(cs), p(ws), ws_bytes, be._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", [0, 1], ids=["rows", "split"])
def test_a_workspace_of_exactly_the_checked_size_is_enough_and_is_not_overrun(be, cus, dt, which):
    shape = SC.CONTRACT_CASES[dt][which]
    I, A, B = shape
    P = A * B
    f = SC.form(dt, I, A, B, cus)
    assert f.get("form") == ("rows", "split")[which]
    need, guard = f["need"], 4096
    d, X, g, sh = _operands(dt, shape)
    ref = SC.reference(d["x"], A, B, d["wA"], d["wB"], SC.SHIFT, d["sub_own"], d["add_other"], SC.ALPHA_COUPLED)
    ws = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device=DEV)       # (whatever a workspace holds must not matter)
    ws[need:] = 0xA5
    tf, Zf = _outputs(I, P)
    cs = be.empty(1)
    args = (X, I, A, B, g["wA"], g["wB"], sh, g["sub_own"], g["add_other"], SC.ALPHA_COUPLED, tf[:I], Zf[:P], cs, ws)
    # 8 bytes short (and no workspace at all): status 2, nothing written
    assert _raw(be, dt, *args, need - 8) == SC.EWORKSPACE and b"workspace" in be.lib.cmtfpls_last_error()
    assert _raw(be, dt, *args[:-1], None, need) == SC.EWORKSPACE
    assert _untouched(tf, Zf) and bool((ws[:need] == 0x5A).all())
    assert _raw(be, dt, *args, need) == 0
    r = SC.ratios(ref, tf[:I].cpu().numpy(), Zf[:P].cpu().numpy(), float(cs.item()))
    assert SC.within(r), r
    assert bool((ws[need:] == 0xA5).all()) and _untouched(tf[I:], Zf[P:])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("which", [0, 1], ids=["rows", "split"])
def test_declines_and_bad_arguments_return_their_status_and_write_nothing(be, cus, dt, which):
    """Every rule is checked before the form is chosen; asked of a row-form and of a split-form shape all the same."""
    V = 4 if dt == "f32" else 2
    stride = SC.stride_of(dt)
    I, A, B = SC.CONTRACT_CASES[dt][which]
    P = A * B
    assert SC.form(dt, I, A, B, cus).get("form") == ("rows", "split")[which]
    big = max(3 * stride, A * (B + V))
    w = torch.ones(big, dtype=F64, device=DEV)
    buf = torch.zeros(I * big + 1, dtype=TDT[dt], device=DEV)
    ws = torch.empty(SC.workspace_bytes(I, big), dtype=torch.uint8, device=DEV)
    tf, Zf = _outputs(I, big)
    X = buf[:I * P].view(I, P)

    def call(X, I_, A_, B_, wA=w, wB=w, t=tf, Z=Zf):
        return _raw(be, dt, X, I_, A_, B_, wA, wB, None, None, None, 1.0, t, Z, None, ws, ws.numel())

    assert call(X, I, A, B) == 0 and not _untouched(tf[:I]) and not _untouched(Zf[:P])       # the shape itself runs
    tf.fill_(SENTINEL)
    Zf.fill_(SENTINEL)
    # a view of X one element past a 16-byte boundary
    off = buf[1:1 + I * P].view(I, P)
    assert off.data_ptr() % 16 == buf.element_size() and SC.form(dt, I, A, B, cus, aligned=False)["status"] == 4
    assert call(off, I, A, B) == SC.EUNSUPPORTED
    # B % V != 0 (a row as long as the shape's own), P = stride / 2 - V
    Bodd = B + V // 2
    assert Bodd % V != 0 and SC.form(dt, I, A, Bodd, cus)["decline"] == "B % V != 0"
    assert call(buf[:I * A * Bodd].view(I, A * Bodd), I, A, Bodd) == SC.EUNSUPPORTED
    short = stride // 2 - V
    assert SC.form(dt, I, 1, short, cus)["decline"] == "P < stride / 2" and "decline" not in SC.form(dt, I, 1, stride // 2, cus)
    assert call(buf[:I * short].view(I, short), I, 1, short) == SC.EUNSUPPORTED
    assert b"score_contract" in be.lib.cmtfpls_last_error()
    # null and non-positive arguments
    assert call(None, I, A, B) == SC.EINVAL and call(X, I, A, B, wA=None) == SC.EINVAL and call(X, I, A, B, wB=None) == SC.EINVAL
    assert call(X, I, A, B, t=None) == SC.EINVAL and call(X, I, A, B, Z=None) == SC.EINVAL
    assert call(X, 0, A, B) == SC.EINVAL and call(X, I, 0, B) == SC.EINVAL and call(X, I, A, 0) == SC.EINVAL
    assert call(X, -1, A, B) == SC.EINVAL
    assert _untouched(tf, Zf)
