"""Every device entry that takes a caller-sized workspace, run with EXACTLY the stated bytes, on poisoned memory, between guards
(tests/guarded_memory.py), and compared bit for bit with the same call on an ordinary backend.

Each case runs three steps: (a) the entry on a fresh HipBackend, outputs cloned; (b) the same inputs on a GuardedBackend after
arena.reset(): every workspace is a view of exactly the stated size of an arena filled with 0xFF (NaN in every float type, -1 as
int32), every output the backend or the test allocates with empty() is such a view too (what zeros() makes is not); (c) arena.check() -- no byte outside the views changed --
every output of (b) has the bits of (a), and the inputs declared read-only are unchanged.  Bit equality is the library's own claim
(one fixed summation order), so there is no tolerance anywhere in this file.  What it notices: a size function that states too
little (EWORKSPACE at equality, or a guard hit), a ragged tile that stores past the end of a workspace or an output, and a partial
slot that a reduce reads without this call having written it (NaN in the result, where a fresh mapping reads as the correct 0).

Shapes are imported from the tables (or the parametrize lists) of the tests that compare the entry with float64; bit equality with
the ordinary call carries that comparison over.  A case in which an entry declines proves nothing: every case asserts a result.

Kept away from the poison, by the two rules of guarded_memory.py:
  * workgroups that wait on each other: the workspaces "rank1", "rank1t", "ceiling_sink" (never poisoned by GuardedBackend) and the
    split form of score_contract, whose workspace holds the exchange slots that the G workgroups of a row stream spin on
    (csrc/scorecontract.hip; its "empty" value is all ones, the poison itself).  The split cases name "score_contract" in
    plain_keys: the backend's own torch.empty buffer outside the arena (asserted in _tally); their outputs are still arena views.  The rank-1 entries and xcov_iterate* are not tested here at all.
  * integers: the `order` / `off` words ((I + 2) int32) at the tail of the weighted K-fold build's workspace are zero-filled
    before the call (cmtfpls_kfold_weighted_xcov_*: kfold_iota_kernel writes them, kfold_wide_kernel indexes rows with them).

The chunked families (leave-one-out, masked cross-validation) run with a budget that leaves a last chunk of ONE item -- twice the
per-item bytes wherever the item count is odd: 5 folds or models in three launches for the masked families, the table's own 25, 9
and 9 folds for the leave-one-out families (I = 12 of the loo_xcov table: 11 + 1) -- and the workspace that the launches of one call
share is poisoned again before every launch.

Teeth, planted once in a scratch build of csrc/press.hip (both stay inside valid memory).  Without the `prow[tid] = 0.0` store of a
tile that holds nothing of a model, both test_press_rows cases fail (128 of 2048 sums NaN); of the 18 cases of
test_gpu_nested_kfold.py::test_press_rows_kernel_against_numpy 9 fail as well and 9 pass, by what the caching allocator happened to
hand their fresh backends.  With cmtfpls_press_rows_workspace_bytes 8 bytes short, both cases fail in arena.check() ("0 bytes after
the end of workspace:press_rows") and all 18 cases of the float64 test pass."""
import zlib

import numpy as np
import pytest
import torch

import guarded_memory as GM
import score_contract_ref as SCR
import small_algebra_ref as SA
import solve_ref as SR
import sweep_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
TDT = {"f32": F32, "f64": F64}
NAN = float("nan")
MAX_X_BYTES = 100e6
_TABLE = {}                                  # entry -> [cases, largest stated workspace bytes, integer regions]


@pytest.fixture(scope="module")
def arena():
    a = GM.Arena(torch.device(DEV))
    yield a
    del a.buf
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for entry, (cases, nbytes, ints) in sorted(_TABLE.items()):
        print(f"workspace contract | {entry} | {cases} cases | largest stated workspace {nbytes} bytes | integer regions: {ints or 'none'}")


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.empty_cache()


def _params(fn, names):
    """The argument list of fn's @pytest.mark.parametrize(names, [...]): the float64 tests' shapes, imported, not copied."""
    for m in fn.pytestmark:
        if m.name == "parametrize" and m.args[0] == names:
            return list(m.args[1])
    raise KeyError(names)


def _pick(table, wanted, key=lambda c: c):
    """The rows of `table` whose key is in `wanted`, every wanted one present."""
    rows = [c for c in table if key(c) in wanted]
    assert {key(c) for c in rows} == set(wanted), (wanted, rows)
    return rows


def _gen(*what):
    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(repr(what).encode()))
    return g


def _randn(g, *shape, dtype=F64, nan=0.0):
    t = torch.randn(*shape, generator=g, device=DEV, dtype=F64)
    if nan:
        t.masked_fill_(torch.rand(t.shape, generator=g, device=DEV) < nan, NAN)
    return t.to(dtype)


def _misaligned(X):
    """A copy of X one element into a larger buffer (tests/test_gpu_kfold_limits.py::_as_view)."""
    from test_gpu_kfold_limits import _as_view
    return _as_view(X, 1)


def _strided(g, I, n):
    """(I, n) with a row stride of n + 3, as the engine passes a column block of its score matrix."""
    return _randn(g, I, n + 3)[:, :n]


def _xy(x, y):
    """Host x (I, ...) and y as (I, P) and (I, M) on the device."""
    I = x.shape[0]
    return tuple(torch.from_numpy(np.ascontiguousarray(a.reshape(I, -1))).to(DEV) for a in (x, y))


def _leaves(v, path="out"):
    """(path, leaf) of every tensor / scalar in a nest of tuples, lists and dicts; None stays a leaf."""
    if isinstance(v, dict):
        for k in sorted(v):
            yield from _leaves(v[k], f"{path}[{k!r}]")
    elif isinstance(v, (tuple, list)):
        for i, e in enumerate(v):
            yield from _leaves(e, f"{path}[{i}]")
    else:
        yield path, v


def _snapshot(v):
    return [(p, e.clone() if isinstance(e, torch.Tensor) else e) for p, e in _leaves(v)]


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for (p, g), (_, w) in zip(got, want):
        if isinstance(w, torch.Tensor):
            assert isinstance(g, torch.Tensor) and g.shape == w.shape and g.dtype == w.dtype, (what, p)
            diff = int((GM.bits(g) != GM.bits(w)).sum())
            assert diff == 0, f"{what}: {p} differs from the ordinary call in {diff} of {w.numel()} elements"
        elif isinstance(w, np.ndarray):
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, p)
        else:
            assert g == w, (what, p, g, w)


def _three_steps(entry, what, arena, monkeypatch, make, call, inplace=False, plain_keys=(), on_take=None, ints=""):
    """make() -> the inputs (a nest of tensors; called once, or once per run when the entry writes X in place);
    call(be, inputs) -> the outputs (a nest; tensors the test passes in come from be.empty).  Returns the outputs of the guarded run."""
    from cmtf_pls_amd.backend import HipBackend
    inputs = make()
    keep = _snapshot(inputs)
    out_a = call(HipBackend(torch.device(DEV)), inputs)
    assert out_a is not None, f"{entry} {what}: the entry declined; the case proves nothing"
    want = _snapshot(out_a)
    if inplace:
        inputs = make()
    arena.reset()
    arena.on_take = on_take
    be = GM.GuardedBackend(arena)
    be.plain_keys = tuple(plain_keys)
    try:
        with GM.guarded(monkeypatch, arena):
            out_b = call(be, inputs)
        assert out_b is not None, f"{entry} {what}: declined on the guarded backend only"
        arena.check()
    finally:
        arena.on_take = None
    _assert_same(_snapshot(out_b), want, f"{entry} {what}")
    if not inplace:
        _assert_same(_snapshot(inputs), keep, f"{entry} {what}: a read-only input changed")
    _tally(entry, arena, be, ints)
    return out_b


def _tally(entry, arena, be, ints=""):
    """One more case of `entry`; the largest bytes a size function stated in it: what the backend asked _workspace for (in the arena
    or, for the keys of waiting kernels, outside it) and what went through _scratch."""
    stated = [n for _, n, _ in be.stated] + [n for name, _, n in arena.views if name.startswith("scratch")]
    assert all(not arena.holds(buf) for buf in be._plain.values())
    row = _TABLE.setdefault(entry, [0, 0, ints])
    row[0] += 1
    row[1] = max([row[1]] + stated)


# ---- X-streaming entries: colstats, mode0_contract, mode0_contract_yq ---------------------------------------------------------------
_SWEEP_SHAPES = {(40000, 48), (5000, 1301), (5000, 2052), (5000, 1026), (5000, 2048), (5000, 1024), (333, 30724), (333, 15362)}
_SWEEP_FORMS = ("narrow", "scalar", "vec U2 guarded blocks1024", "vec U2 FULL blocks512", "vec U2 guarded ilv blocks1024")
SWEEP_CASES = [c for c in SC.CASES if c[0] in ("colstats", "mode0_contract", "mode0_contract_yq") and (c[2], c[3] * c[4]) in _SWEEP_SHAPES
               and c[6] in (0, 5) and c[2] * c[3] * c[4] * (4 if c[1] == "f32" else 8) <= MAX_X_BYTES]
assert {c[7].replace(" yqpre", "").replace(" yq", "") for c in SWEEP_CASES} == set(_SWEEP_FORMS)
assert {c[0] for c in SWEEP_CASES} == {"colstats", "mode0_contract", "mode0_contract_yq"}


@pytest.mark.parametrize("case", SWEEP_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}x{c[3] * c[4]}-{'m' if c[5] else 'u'}-M{c[6]}")
def test_sweeps(arena, monkeypatch, case):
    import test_gpu_sweep_forms as TSF
    from cmtf_pls_amd.backend import HipBackend
    op, dt, I, A, B, masked, M, form = case
    P = A * B
    assert HipBackend.sweep_form(op, dt, I, A, B, masked, M) == form

    def make():
        g = TSF._gen(case)
        X = TSF._make_x(g, dt, I, P, masked or op == "colstats")
        if op == "mode0_contract_yq":
            return X, _randn(g, I, M), _randn(g, M)
        return X, _randn(g, I)

    def call(be, inp):
        if op == "colstats":
            return be.colstats(inp[0])
        if op == "mode0_contract":
            return be.mode0_contract(inp[0], inp[1], masked, out=be.empty(P))
        return be.mode0_contract_yq(inp[0], inp[1], inp[2], masked, out=be.empty(P))

    _three_steps(op, case, arena, monkeypatch, make, call)


# ---- deflate_contract_yq: one shape per kind cmtfpls_sweep_form reports (column tiles, row groups), from its float64 test ------------
def _deflate_cases():
    import test_gpu_kernels as TK
    from cmtf_pls_amd.backend import HipBackend
    best = {}
    for shape, M in _params(TK.test_deflate_contract_yq, "shape,M"):
        I, A, B = shape
        for dt in ("f32", "f64"):
            if I * A * B * (4 if dt == "f32" else 8) > MAX_X_BYTES:
                continue
            kind = HipBackend.sweep_form("deflate_contract_yq", dt, I, A, B, False, M).split()[0]        # "tile" | "rows1024"
            if (kind, dt) not in best or I * A * B < np.prod(best[(kind, dt)][0]):
                best[(kind, dt)] = (shape, M)
    assert {k for k, _ in best} == {"tile", "rows1024"} and len(best) == 4, best
    return [(kind, dt, shape, M) for (kind, dt), (shape, M) in sorted(best.items())]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind,dt,shape,M", _deflate_cases())
def test_deflate_contract_yq(arena, monkeypatch, kind, dt, shape, M, masked):
    I, A, B = shape
    assert kind == "tile" or I >= 512

    def make():
        g = _gen("dcyq", shape, dt, masked)
        wa, wb = _randn(g, A), _randn(g, B)
        return (_randn(g, I, A * B, dtype=TDT[dt], nan=0.2 if masked else 0.0), _randn(g, I), wa / wa.norm(), wb / wb.norm(),
                _randn(g, I, M), _randn(g, M))

    def call(be, inp):
        X, t, wa, wb, Y, q = inp
        Z = be.empty(A * B)
        ssq = be.deflate_contract_yq(X, A, B, t, wa, wb, Y, q, masked, out=Z)
        return None if ssq is None else (X, Z, ssq)

    _three_steps("deflate_contract_yq", (kind, dt, shape, M, masked), arena, monkeypatch, make, call, inplace=True)


# ---- the matrix-core builds of S: xcov, xcov_ssq, xcov_stats, the f32 mixed form -------------------------------------------------------
def _xcov_cases():
    import test_gpu_kernels as TK
    table = _params(TK.test_xcov_mfma, "shape,M")
    rows = _pick(table, {((257, 24, 12), 33), ((300, 16, 16), 17), ((70, 8, 8), 64), ((37, 10, 8), 4)})
    over = [c for c in table if c[1] > 64]
    assert over, "no xcov case with more than 64 responses (tiles of 64)"
    return rows, over[:1]


XCOV_CASES, XCOV_OVER_64 = _xcov_cases()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("shape,M", XCOV_CASES + XCOV_OVER_64)
def test_xcov(arena, monkeypatch, shape, M, dt, masked):
    I, A, B = shape

    def make():
        g = _gen("xcov", shape, M, dt, masked)
        return _randn(g, I, A * B, dtype=TDT[dt], nan=0.3 if masked else 0.0), _strided(g, I, M)

    _three_steps("xcov", (shape, M, dt, masked), arena, monkeypatch, make, lambda be, inp: be.xcov(inp[0], inp[1], masked))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape,M", XCOV_CASES)
def test_xcov_f32_mixed(arena, monkeypatch, shape, M, masked):
    import test_gpu_mixed as TM
    assert (shape, M) in _params(TM.test_xcov_mixed, "shape,M")
    I, A, B = shape

    def make():
        g = _gen("xcov mixed", shape, M, masked)
        return _randn(g, I, A * B, dtype=F32, nan=0.3 if masked else 0.0), _randn(g, I, M)

    _three_steps("xcov_f32_mixed", (shape, M, masked), arena, monkeypatch, make, lambda be, inp: be.xcov(inp[0], inp[1], masked, mixed=True))


def _ipm(cases):
    return [(s[0], s[1] * s[2], M) for s, M in cases]


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("I,P,M", _ipm(XCOV_CASES))
def test_xcov_ssq_and_stats(arena, monkeypatch, I, P, M, dt):
    import test_gpu_round3 as T3
    import test_gpu_round4 as T4
    assert (I, P, M) in _params(T3.test_xcov_ssq_kernel_gives_s_and_the_centred_norm_from_one_read, "I,P,M")
    assert (I, P, M) in _params(T4.test_xcov_stats_kernel_gives_s_and_the_column_statistics_from_one_read, "I,P,M")

    def make():
        g = _gen("xcov ssq", I, P, M, dt)
        X = (_randn(g, I, P) * 1.5 + 5.0 * _randn(g, P)).to(TDT[dt])
        return X, _randn(g, I, M), X.double().mean(dim=0)

    _three_steps("xcov_ssq", (I, P, M, dt), arena, monkeypatch, make, lambda be, inp: be.xcov_ssq(inp[0], inp[1], inp[2], out=be.empty(M, P)))
    _three_steps("xcov_stats", (I, P, M, dt), arena, monkeypatch, make, lambda be, inp: be.xcov_stats(inp[0], inp[1], out=be.empty(M, P)))


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("P", (7, 264))
@pytest.mark.parametrize("M", (17, 64))
def test_xcov_16_bit(arena, monkeypatch, P, M, kind):
    """bfloat16 and float16 storage at the ragged shapes of the 16-bit table (five row blocks at I = 300)."""
    import test_gpu_half_diag_kernels as TD
    import test_gpu_half_kernels as TH
    I = 300
    assert I in TH.XCOV_I and P in TH.XCOV_P and M in TH.XCOV_M and kind in TH.HS.KINDS

    def make():
        g = _gen("xcov 16-bit", P, M, kind)
        return _randn(g, I, P, dtype=TD.KINDS[kind]), _randn(g, I, M)

    _three_steps(f"xcov ({kind})", (I, P, M), arena, monkeypatch, make, lambda be, inp: be.xcov(inp[0], inp[1], False))
    _three_steps(f"xcov_stats ({kind})", (I, P, M), arena, monkeypatch, make, lambda be, inp: be.xcov_stats(inp[0], inp[1], out=be.empty(M, P)))


def _masked_16_bit_widths():
    import test_gpu_half_kernels as TH
    return _params(TH.test_xcov_masked_and_what_the_statistics_show_of_a_missing_value, "P")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("P", _masked_16_bit_widths())
def test_xcov_16_bit_masked(arena, monkeypatch, P, kind):
    """The masked S build on 16-bit storage, at the shape of the 16-bit table's masked test (I = 37, M = 17), 30 % missing."""
    import test_gpu_half_diag_kernels as TD
    I, M = 37, 17

    def make():
        g = _gen("xcov 16-bit masked", P, kind)
        return _randn(g, I, P, dtype=TD.KINDS[kind], nan=0.3), _strided(g, I, M)

    _three_steps(f"xcov ({kind})", (I, P, M, "masked"), arena, monkeypatch, make, lambda be, inp: be.xcov(inp[0], inp[1], True))


# ---- score_contract: one case per instance of tests/score_contract_ref.py -------------------------------------------------------------
def _score_contract_cases():
    out = []
    for dt in ("f32", "f64"):
        for inst in SCR.INSTANCES[dt]:
            hit = [s for s, f32, f64 in SCR.ALL_CASES
                   if not isinstance((f32, f64)[dt == "f64"], str) and tuple((f32, f64)[dt == "f64"][:4]) == inst]
            assert hit, (dt, inst)
            out.append((dt, inst, hit[0]))
    return out


@pytest.mark.parametrize("dt,inst,shape", _score_contract_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_score_contract(arena, monkeypatch, dt, inst, shape):
    I, A, B = shape
    P = A * B
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    f = SCR.check_claim(dt, shape, cus)
    assert "decline" not in f, f
    d = SCR.make_case(dt, I, A, B)

    def make():
        dev = lambda a, t=F64: torch.as_tensor(a, dtype=t, device=DEV).contiguous()
        return (dev(d["x"], TDT[dt]), dev(d["wA"]), dev(d["wB"]), dev([SCR.SHIFT]), dev(d["sub_own"]), dev(d["add_other"]))

    def call(be, inp):
        X, wA, wB, sh, own, other = inp
        t, Z, cs = be.empty(I), be.empty(P), be.empty(1)
        got = be.score_contract(X, A, B, wA, wB, sh, t, Z, sub_own=own, add_other=other, alpha=SCR.ALPHA_COUPLED, csum=cs)
        t2, Z2 = be.empty(I), be.empty(P)
        plain = be.score_contract(X, A, B, wA, wB, sh, t2, Z2)
        return None if got is None or plain is None else (t, Z, cs, t2, Z2)

    # the split form's workgroups wait on exchange slots in the workspace: no poison there (the outputs stay guarded)
    split = inst[0] == "split"
    _three_steps("score_contract (split: ordinary workspace)" if split else "score_contract", (dt, inst, shape), arena, monkeypatch, make, call,
                 plain_keys=("score_contract",) if split else ())


# ---- the model-streaming passes: recon_r2, resid_rows, heldout_resid, impute, selectivity_cols ----------------------------------------
MODEL_SHAPES = [(517, 7, 9), (517, 12, 20), (2100, 33, 40)]          # scalar; vector; P = 1320: five column tiles and a partial one
MODEL_R = (1, 5, 16)


def _model_inputs(tag, shape, R, dtype, misaligned, nan=0.1):
    I, A, B = shape
    g = _gen(tag, shape, R, str(dtype), misaligned)
    X = _randn(g, I, A * B, dtype=dtype, nan=nan)
    if misaligned:
        X = _misaligned(X)
    return X, _strided(g, I, R), _randn(g, A, R), _randn(g, B, R), _randn(g, A * B)


_MODEL_PARAMS = [(s, dt, False) for s in MODEL_SHAPES for dt in (F32, F64)] + [(MODEL_SHAPES[1], F32, True), (MODEL_SHAPES[1], F64, True)]


@pytest.mark.parametrize("shape,dtype,misaligned", _MODEL_PARAMS, ids=lambda v: str(v).replace(" ", "").replace("torch.", ""))
def test_recon_r2_and_resid_rows(arena, monkeypatch, shape, dtype, misaligned):
    import test_gpu_diagnostics as TD
    for R in MODEL_R:
        assert (*shape, R, int(misaligned)) in [c[:5] for c in TD.RESID_KERNEL_CASES]      # the float64 tests run this very row
        make = lambda: _model_inputs("resid", shape, R, dtype, misaligned)
        _three_steps("recon_r2", (shape, R, dtype, misaligned), arena, monkeypatch, make, lambda be, inp: be.recon_r2(*inp))
        for want_cols in (True, False):
            _three_steps("resid_rows", (shape, R, dtype, misaligned, want_cols), arena, monkeypatch, make,
                         lambda be, inp: be.resid_rows(*inp, want_cols))




def test_recon_r2_and_resid_rows_16_bit(arena, monkeypatch):
    """bfloat16 storage at the 16-bit table's shapes: the one-element path, two column tiles, a misaligned view."""
    import test_gpu_half_diag_kernels as TH
    for I, A, B, offset in _pick(TH.RESID_SHAPES, {(37, 5, 6, 0), (9, 33, 32, 0), (70, 8, 8, 1)}):
        def make():
            X16, _ = TH._x16("bf16", I, A * B, seed=I + A + B, offset=offset)
            T, _, WA, WB, mean = TH._factors(I, A, B, 5, seed=5)
            return X16, T, WA, WB, mean
        _three_steps("recon_r2 (bf16)", (I, A, B, offset), arena, monkeypatch, make, lambda be, inp: be.recon_r2(*inp))
        _three_steps("resid_rows (bf16)", (I, A, B, offset), arena, monkeypatch, make, lambda be, inp: be.resid_rows(*inp, True))


@pytest.mark.parametrize("shape,dtype,misaligned", _MODEL_PARAMS, ids=lambda v: str(v).replace(" ", "").replace("torch.", ""))
def test_heldout_resid_and_impute(arena, monkeypatch, shape, dtype, misaligned):
    import test_gpu_impute_kernels as TI
    tiled = shape in [c[1:4] for c in TI.TILED_SHAPES]
    assert (*shape, int(misaligned)) in [(*c[1:4], c[5]) for c in (TI.TILED_SHAPES if tiled else TI.SHAPES)]
    assert set(MODEL_R) <= set(_params(TI.test_heldout_resid_and_impute_across_column_tiles, "R") if tiled else TI.RS)
    I, A, B = shape
    for R in MODEL_R:
        make = lambda: _model_inputs("impute", shape, R, dtype, misaligned, nan=0.2)
        _three_steps("heldout_resid", (shape, R, dtype, misaligned), arena, monkeypatch, make,
                     lambda be, inp: be.heldout_resid(*inp, 0.5, 991, 2, 4099))

        heads = []

        def impute_to_copy(be, inp):
            buf = be.empty(I * A * B + int(misaligned), dtype=dtype)          # out one element into its allocation, as X is
            out = buf[int(misaligned):].view(I, A * B)
            heads.append(buf[:int(misaligned)])
            count = be.impute(inp[0], out, *inp[1:])
            return None if count is None else (out, count)
        _three_steps("impute", (shape, R, dtype, misaligned), arena, monkeypatch, make, impute_to_copy)
        assert bool((heads[-1].view(torch.uint8) == GM.POISON).all())          # the element before a misaligned out is nobody's to write

        def impute_in_place(be, inp):
            count = be.impute(inp[0], inp[0], *inp[1:])
            return None if count is None else (inp[0], count)
        _three_steps("impute", (shape, R, dtype, misaligned, "in place"), arena, monkeypatch, make, impute_in_place, inplace=True)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape,dtype,misaligned", _MODEL_PARAMS, ids=lambda v: str(v).replace(" ", "").replace("torch.", ""))
def test_selectivity_cols(arena, monkeypatch, shape, dtype, misaligned, masked):
    import test_gpu_selectivity_kernel as TS
    I, A, B = shape
    P = A * B
    for M in (1, 17):
        assert (I, P, M, int(misaligned)) in TS.SHAPES

        def make():
            g = _gen("selectivity", shape, M, str(dtype), misaligned, masked)
            X = _randn(g, I, P, dtype=dtype, nan=0.1 if masked else 0.0)
            return (_misaligned(X) if misaligned else X), _strided(g, I, M), _randn(g, P)
        _three_steps("selectivity_cols", (shape, M, dtype, misaligned, masked), arena, monkeypatch, make,
                     lambda be, inp: be.selectivity_cols(*inp, masked))


def test_selectivity_cols_16_bit(arena, monkeypatch):
    import test_gpu_half_diag_kernels as TH
    for case in _pick(TH.SEL_CASES, {(70, 260, 33, False), (70, 260, 17, True), (65, 64, 16, False, 1)}):
        I, P, M, masked = case[:4]
        offset = case[4] if len(case) > 4 else 0

        def make():
            X16, _ = TH._x16("bf16", I, P, seed=I + P + M, offset=offset)
            g = _gen("selectivity bf16", case)
            return X16, _strided(g, I, M), 0.25 * _randn(g, P)
        _three_steps("selectivity_cols (bf16)", case, arena, monkeypatch, make, lambda be, inp: be.selectivity_cols(*inp, masked))


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [3, 1021, 300001])
def test_holdout_mask(arena, monkeypatch, n, dtype, misaligned):
    import test_gpu_impute_kernels as TI
    assert n in TI.FLAT_SIZES

    def make():
        g = _gen("holdout", n, str(dtype), misaligned)
        X = _randn(g, 1, n, dtype=dtype, nan=0.2)
        return ((_misaligned(X) if misaligned else X).view(n),)

    heads = []

    def call(be, inp):
        buf = be.empty(n + int(misaligned), dtype=dtype)
        out = buf[int(misaligned):]
        heads.append(buf[:int(misaligned)])
        counts = be.holdout_mask(inp[0], out, 0.5, 215, 3, 4099)
        return None if counts is None else (out, counts)
    _three_steps("holdout_mask", (n, dtype, misaligned), arena, monkeypatch, make, call)
    assert bool((heads[-1].view(torch.uint8) == GM.POISON).all())              # the element before a misaligned out is nobody's to write


# ---- the K-fold builds: kfold_xcov, kfold_wide_xcov, kfold_weighted_xcov ------------------------------------------------------------------
def _fold_order(I, K, seed):
    ids = np.random.default_rng(seed).permutation(np.arange(I) % K)
    ids[: min(3, I)] = 0                                                   # ragged folds
    counts = np.bincount(ids, minlength=K)
    assert counts.min() >= 1
    order = torch.from_numpy(np.argsort(ids, kind="stable").astype(np.int32)).to(DEV)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(DEV)
    return order, off


def _build_x(g, I, P, xdtype, base):
    X = (_randn(g, I, P) + 0.3).to(xdtype)
    return _misaligned(X) if base else X


def _kfold_xcov_cases():
    import test_gpu_kfold_limits as TL
    return [TL.XCOV_CASES[i - 1] for i in (1, 2, 4, 5, 8)]


@pytest.mark.parametrize("xdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("I,A,B,M,K,kind", _kfold_xcov_cases())
def test_kfold_xcov(arena, monkeypatch, I, A, B, M, K, kind, xdtype):
    import test_gpu_kfold_limits as TL
    P = A * B
    ids, K = TL._fold_split(I, K, kind, I)
    counts = np.bincount(ids, minlength=K)
    order = torch.from_numpy(np.argsort(ids, kind="stable").astype(np.int32)).to(DEV)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(DEV)

    def make():
        g = _gen("kfold_xcov", I, A, B, M, K, str(xdtype))
        return _build_x(g, I, P, xdtype, 0), _randn(g, I, M), order, off, _randn(g, K, M)

    def call(be, inp):
        X, Y, order, off, ydev = inp
        S, mean = be.empty(K, M, P), be.empty(K, P)
        stats = be.kfold_xcov(X, A, B, Y, order, off, K, ydev, S, mean)
        return None if stats is None else (S, mean, stats)
    _three_steps("kfold_xcov", (I, A, B, M, K, xdtype), arena, monkeypatch, make, call)


def _wide_cases():
    import test_gpu_permutation as TP
    return _pick(_params(TP.test_wide_build_against_float64_torch, "I,A,B,W,K"), {(300, 7, 9, 5, 2), (517, 1, 130, 37, 32)})


@pytest.mark.parametrize("xdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("I,A,B,W,K", _wide_cases())
def test_kfold_wide_xcov(arena, monkeypatch, I, A, B, W, K, xdtype):
    P = A * B
    order, off = _fold_order(I, K, W)

    def make():
        g = _gen("kfold_wide", I, A, B, W, K, str(xdtype))
        return _build_x(g, I, P, xdtype, 0), _randn(g, I, W), order, off, _randn(g, K, W)

    def call(be, inp):
        X, Y, order, off, ydev = inp
        S, mean = be.empty(K, W, P), be.empty(K, P)
        stats = be.kfold_wide_xcov(X, A, B, Y, order, off, K, ydev, S, mean)
        return None if stats is None else (S, mean, stats)
    _three_steps("kfold_wide_xcov", (I, A, B, W, K, xdtype), arena, monkeypatch, make, call)


def _weighted_cases():
    import test_gpu_kfold_limits as TL
    return [TL.WEIGHTED_CASES[i - 1] for i in (1, 3, 5, 7)]


@pytest.mark.parametrize("xdtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("I,A,B,M,n", _weighted_cases())
def test_kfold_weighted_xcov(arena, monkeypatch, I, A, B, M, n, xdtype):
    from cmtf_pls_amd import _lib
    P = A * B
    stated = int(_lib.load().cmtfpls_kfold_weighted_xcov_workspace_bytes(I, P, n, M))
    tail = (I + 2) * 4                                                     # order (I) | off (2), int32, behind the partial sums

    def zero_the_index_words(name, view):
        if name == "scratch":
            assert view.numel() == stated
            view[stated - tail:].zero_()

    def make():
        g = _gen("kfold_weighted", I, A, B, M, n, str(xdtype))
        draws = np.random.default_rng(n * M).integers(0, I, size=(n, I))                   # real bootstrap draws
        C = torch.from_numpy(np.stack([np.bincount(r, minlength=I) for r in draws])).to(DEV).double()
        Yd = _randn(g, I, M)
        Yc = Yd.unsqueeze(0) - ((C @ Yd) / I).unsqueeze(1)
        Yw = torch.cat([(C.unsqueeze(2) * Yc).permute(1, 0, 2).reshape(I, n * M), C.t()], dim=1).contiguous()
        return _build_x(g, I, P, xdtype, 0), Yw

    def call(be, inp):
        S, mean = be.empty(n, M, P), be.empty(n, P)
        stats = be.kfold_weighted_xcov(inp[0], A, B, inp[1], n, M, S, mean)
        return None if stats is None else (S, mean, stats)
    _three_steps("kfold_weighted_xcov", (I, A, B, M, n, xdtype), arena, monkeypatch, make, call, on_take=zero_the_index_words,
                 ints="order | off: the last (I + 2) int32 of the workspace, zero-filled")


# ---- press_rows: a model without rows and a whole empty row tile ----------------------------------------------------------------------
def _press_cases():
    import test_gpu_nested_kfold as TN
    t = TN.test_press_rows_kernel_against_numpy
    got = [(n, I, R, M) for n, I in _params(t, "n,I") for R in _params(t, "R") for M in _params(t, "M")]
    return _pick(got, {(2, 2500, 16, 16), (32, 1100, 64, 64)})


@pytest.mark.parametrize("n,I,R,M", _press_cases())
def test_press_rows(arena, monkeypatch, n, I, R, M):
    import test_gpu_nested_kfold as TN
    host = TN._kernel_inputs(n, I, R, M, seed=1000 * R + 10 * M + n)
    ev = host[5]
    assert not ev[1].any() and (I <= 1024 or not ev[0, :1024].any())     # a model without rows; a whole row tile without any

    def make():
        return tuple(torch.from_numpy(a).to(DEV) for a in host)

    def call(be, inp):
        pred = be.empty(R, I, M)
        press = be.press_rows(*inp, pred)
        return None if press is None else (press, pred, be.press_rows(*inp, None))
    # pred is written only where ev == 2: the rest of the guarded pred stays poison in (b) and garbage in (a); compare what is written
    written = torch.from_numpy((ev == 2).any(axis=0)).to(DEV)

    def call_written(be, inp):
        out = call(be, inp)
        return None if out is None else (out[0], out[1][:, written], out[1][:, ~written].view(torch.int64).eq(-1).all().item()
                                         if isinstance(be, GM.GuardedBackend) else True, out[2])
    _three_steps("press_rows", (n, I, R, M), arena, monkeypatch, make, call_written)


# ---- the "small" workspace (gram_tn), total, scores_mean, normal_solve_ws ---------------------------------------------------------------
def _ends(table):
    key = lambda c: int(np.prod(c)) if isinstance(c, tuple) else int(c)
    return [min(table, key=key), max(table, key=key)]


@pytest.mark.parametrize("I,a", _ends(SA.GEMV_CASES))
def test_gram_tn_gemv(arena, monkeypatch, I, a):
    def make():
        g = _gen("gemv", I, a)
        return _randn(g, I, a + 8)[:, 3:3 + a], _randn(g, I, 5)[:, 2:3]
    _three_steps("gram_tn", ("gemv", I, a), arena, monkeypatch, make, lambda be, inp: be.gram_tn(*inp))


@pytest.mark.parametrize("I", _ends(SA.TILED_I))
def test_gram_tn_tiled(arena, monkeypatch, I):
    for a, b in _ends(SA.TILED_AB):
        def make():
            W = _randn(_gen("tiled", I), I, SA.TILED_WIDTH)
            return W[:, :a], W[:, SA.TILED_WIDTH - b:]
        _three_steps("gram_tn", ("tiled", I, a, b), arena, monkeypatch, make, lambda be, inp: be.gram_tn(*inp))


@pytest.mark.parametrize("n", _ends(SA.SUM_N))
def test_total(arena, monkeypatch, n):
    _three_steps("total", n, arena, monkeypatch, lambda: (_randn(_gen("total", n), n),), lambda be, inp: be.total(inp[0]))


@pytest.mark.parametrize("nb,I", _ends(SA.SCORES_MEAN_CASES))
def test_scores_mean(arena, monkeypatch, nb, I):
    _three_steps("scores_mean", (nb, I), arena, monkeypatch, lambda: (_randn(_gen("scores_mean", nb, I), nb, I),),
                 lambda be, inp: be.scores_mean(inp[0], be.empty(I)))


@pytest.mark.parametrize("k", _ends(SR.NORMAL_K_WS))
def test_normal_solve_ws(arena, monkeypatch, k):
    def make():
        g = _gen("normal_solve", k)
        T = _randn(g, k + 40, k)
        return (T.t() @ T).contiguous(), T.t() @ _randn(g, k + 40)
    _three_steps("normal_solve_ws", k, arena, monkeypatch, make, lambda be, inp: be.normal_solve(*inp))


# ---- fit_small --------------------------------------------------------------------------------------------------------------------------
def test_fit_small(arena, monkeypatch):
    import test_gpu_small_fit_limits as TF
    shape, M, R, _ = TF.FIT_CASES[0]                                        # (10, 32, 40), M 17, R 4: X in LDS, Z by columns
    I, (A, B) = shape[0], TF._split(shape)
    x, y = TF._data(shape, M, R, seed=11)
    _three_steps("fit_small", (shape, M, R), arena, monkeypatch, lambda: _xy(x, y),
                 lambda be, inp: be.fit_small(inp[0], inp[1], A, B, R, 1e-8, 100))


# ---- the chunked fold families ----------------------------------------------------------------------------------------------------------
def _per_item_bytes(run):
    """The bytes per item that `run(be, max_ws_bytes)` counts against its budget: per_fn() + extra of its _chunked_launch."""
    from cmtf_pls_amd.backend import HipBackend
    be, seen = HipBackend(torch.device(DEV)), {}

    def spy(name, call, n, per_fn, budget, cap=None, extra=0, ws_key=None):
        assert call(0, 1, None, 0) != 4, f"{name} declines the shape"
        seen["per"], seen["n"] = int(per_fn()) + int(extra), n
        return None
    be._chunked_launch = spy
    be.lib.cmtfpls_clear_error()
    run(be, None)
    return seen["per"], seen["n"]


def _chunked(entry, what, arena, monkeypatch, make, run):
    """run(be, inputs, max_ws_bytes) with a budget of c items, c the smallest count that leaves a last chunk of ONE item: twice the
    per-item bytes for an odd number of items (5 items: three launches)."""
    inputs = make()
    per, n = _per_item_bytes(lambda be, budget: run(be, inputs, budget))
    c = next(c for c in range(2, n) if n % c == 1)
    launches = []

    def call(be, inp):
        inner = be._chunked_launch

        def counted(*args, **kwargs):
            launches.append(inner(*args, **kwargs))
            return launches[-1]
        be._chunked_launch = counted
        try:
            return run(be, inp, c * per)
        finally:
            del be._chunked_launch
    _three_steps(entry, what, arena, monkeypatch, make, call)
    assert launches == [-(-n // c)] * 2 and launches[0] >= 2, (launches, n, c)


def test_loo_tpls(arena, monkeypatch):
    import test_gpu_small_fit_limits as TF
    shape, M, R, _ = TF.LOO_CASES[5]                                        # (25, 1, 300): 25 folds in 13 launches
    assert shape[0] == 25
    I, (A, B) = shape[0], TF._split(shape)
    x, y = TF._data(shape, M, R, seed=21, error=0.3)
    _chunked("loo_tpls", (shape, M, R), arena, monkeypatch, lambda: _xy(x, y),
             lambda be, inp, budget: be.loo_tpls(inp[0], inp[1], A, B, R, 1e-8, 100, max_ws_bytes=budget, forms=("lds",)))


def test_loo_xcov(arena, monkeypatch):
    import loo_xcov_ref as L
    import test_gpu_loo_xcov_limits as TX
    case = _pick(L.MATCH_CASES, {((12, 17, 33), 3, 3)}, key=lambda c: c[:3])[0]          # 12 folds: a launch of 11 and one of 1
    shape, M, R = case[:3]
    A, B = L.split(shape)
    _chunked("loo_xcov", L.case_id(case), arena, monkeypatch, lambda: TX._inputs(case),
             lambda be, inp, budget: be.loo_tpls(inp[0], inp[1], A, B, R, L.TOL, L.MAX_ITER, max_ws_bytes=budget, forms=("xcov",)))


def test_loo_xcov_tensor(arena, monkeypatch):
    import test_gpu_loo_order4_kernel as T4
    I, A, B1, B2 = T4.SHAPES[0]                                             # (9, 5, 7, 3)
    make = lambda: (_randn(_gen("loo4"), I, A * B1 * B2), _randn(_gen("loo4 y"), I, 3))
    _chunked("loo_xcov_tensor", T4.SHAPES[0], arena, monkeypatch, make,
             lambda be, inp, budget: be.loo_tpls_tensor(inp[0], inp[1], A, B1, B2, T4.R, T4.TOL, T4.MAX_ITER, max_ws_bytes=budget))


def test_loo_xcov_coupled(arena, monkeypatch):
    import loo_coupled_ref as C
    import test_gpu_loo_coupled_kernel as TC
    case = min((c for c in C.MATCH_CASES if c[0] % 2 == 1), key=lambda c: c[0] * sum(int(np.prod(t)) for t in c[1]) * c[2])
    _chunked("loo_xcov_coupled", C.case_id(case), arena, monkeypatch, lambda: TC._inputs(case),
             lambda be, inp, budget: be.loo_ctpls(inp[0], inp[1], inp[2], case[3], C.TOL, C.MAX_ITER, max_ws_bytes=budget))


def test_loo_xcov_coupled_tensor(arena, monkeypatch):
    import loo_coupled_order4_ref as T
    import test_gpu_loo_coupled_order4_kernel as TC
    case = min((c for c in T.CASES if c[0] % 2 == 1), key=lambda c: c[0] * sum(int(np.prod(t)) for t in c[1]) * c[2])
    _chunked("loo_xcov_coupled_tensor", T.case_id(case), arena, monkeypatch, lambda: TC._inputs(case),
             lambda be, inp, budget: be.loo_ctpls_tensor(inp[0], inp[1], inp[2], inp[3], case[3], T.TOL, T.MAX_ITER, max_ws_bytes=budget))


def _counts(I, nm=5):
    rng = np.random.default_rng(11)
    return (torch.from_numpy(rng.integers(0, 3, size=(nm, I)).astype(np.int32)).to(DEV),
            torch.from_numpy(np.stack([rng.permutation(I) for _ in range(nm)]).astype(np.int32)).to(DEV))


def test_cv_masked_and_models(arena, monkeypatch):
    """The shape of tests/test_gpu_cv_masked.py's chunk test, 5 folds / 5 models in 3 launches."""
    import test_gpu_cv_masked as TM
    import test_gpu_cv_masked_models as TMM
    from cmtf_pls_amd.kfold import fold_ids
    I, (A, B), M, R = 36, (7, 6), 3, 3
    ids, K = fold_ids(I, 5)
    fo = torch.from_numpy(ids.astype(np.int32)).to(DEV)
    _chunked("cv_masked", (I, A, B, M, R, K), arena, monkeypatch, lambda: _xy(*TM._data((I, A, B), M, R, 0.1, seed=31)),
             lambda be, inp, budget: be.cv_masked(inp[0], inp[1], fo, K, A, B, R, 1e-8, 100, max_ws_bytes=budget))
    _chunked("cv_masked_models", (I, A, B, M, R, 5), arena, monkeypatch, lambda: _xy(*TMM._data((I, A, B), M, R, 0.1, seed=79)) + _counts(I),
             lambda be, inp, budget: be.cv_masked_models(inp[0], inp[1], inp[2], inp[3], A, B, R, 1e-8, 100, factors=True, max_ws_bytes=budget))


def test_cv_masked_tensor(arena, monkeypatch):
    import test_gpu_cv_masked_order4 as T4
    from cmtf_pls_amd.kfold import fold_ids
    I, (A, B1, B2), M, R = 36, (6, 4, 3), 2, 3
    ids, K = fold_ids(I, 5)
    fo = torch.from_numpy(ids.astype(np.int32)).to(DEV)
    make = lambda: _xy(*T4._data((I, A, B1, B2), M, R, 0.3, seed=36))
    _chunked("cv_masked_tensor", (I, A, B1, B2, M, R, K), arena, monkeypatch, make,
             lambda be, inp, budget: be.cv_masked_tensor(inp[0], inp[1], fo, K, A, B1, B2, R, 1e-8, 100, max_ws_bytes=budget))
    _chunked("cv_masked_tensor_models", (I, A, B1, B2, M, R, 5), arena, monkeypatch, lambda: make() + _counts(I),
             lambda be, inp, budget: be.cv_masked_tensor_models(inp[0], inp[1], inp[2], inp[3], A, B1, B2, R, 1e-8, 100, factors=True,
                                                                max_ws_bytes=budget))


def test_cv_masked_coupled(arena, monkeypatch):
    import test_gpu_cv_masked_coupled as TC
    I, M, R = 36, 3, 3
    Xs, y = TC._coupled_data(I, TC.TMT, M, R + 1, seed=79)
    counts, yrow = (t.cpu().numpy() for t in _counts(I))
    _chunked("cv_masked_coupled", ("TMT", I, M, R), arena, monkeypatch, lambda: (),
             lambda be, inp, budget: TC._kernel(be, Xs, y, counts, yrow, R, factors=True, max_ws_bytes=budget))


def test_cv_masked_coupled_tensor(arena, monkeypatch):
    import test_gpu_cv_masked_coupled_order4 as TC
    I, M, R = 36, 3, 3
    Xs, y = TC._coupled_data(I, TC.TMQ, M, R + 1, seed=79)
    counts, yrow = (t.cpu().numpy() for t in _counts(I))
    _chunked("cv_masked_coupled_tensor", ("TMQ", I, M, R), arena, monkeypatch, lambda: (),
             lambda be, inp, budget: TC._kernel(be, Xs, y, counts, yrow, R, factors=True, max_ws_bytes=budget))


# ---- the K-fold state family (kfold_inner plain, tensor, coupled, grouped) through its drivers; the estimator --------------------------
def _estimator_pass(entry, what, arena, monkeypatch, build, use):
    """build(backend or None) -> a fitted model; use(model) -> a nest of arrays.  The ordinary model against the one whose backend,
    and whose drivers' _scratch, allocate from the arena."""
    from cmtf_pls_amd.backend import HipBackend
    want = _snapshot(use(build(HipBackend(torch.device(DEV)))))
    arena.reset()
    be = GM.GuardedBackend(arena)
    with GM.guarded(monkeypatch, arena):
        got = _snapshot(use(build(be)))
    arena.check()
    _assert_same(got, want, f"{entry} {what}")
    _tally(entry, arena, be)


def test_kfold_state_plain_and_grouped(arena, monkeypatch):
    import oracle as O
    import test_gpu_kfold_limits as TL
    from cmtf_pls_amd import tPLS
    from cmtf_pls_amd.validate import get_q2y_kfold, permutation_test_q2y
    name, shape, M, R, K, _ = TL.KFOLD_CASES[0]                             # "M 17": (60, 10, 8), 3 components, 4 folds
    x, y, _ = O.import_synthetic(shape, M, R + 1, error=0.3, seed=7)

    def build(be):
        m = tPLS(R, dtype="float64", backend=be)
        m.fit(x, y)
        return m

    def kfold(m):
        q = get_q2y_kfold(m, n_splits=K, per_component=True)
        assert "cmtfpls_kfold_inner_f64" in m.q2y_report_["form"] and "why" not in m.q2y_report_, m.q2y_report_
        return q, m.q2y_report_["n_iter"]

    def permutation(m):
        res = permutation_test_q2y(m, n_permutations=4, n_splits=K, random_state=3, per_component=True)
        assert "cmtfpls_kfold_inner_grouped_f64" in m.q2y_report_["form"] and "why" not in m.q2y_report_, m.q2y_report_
        return res["q2y"], res["null"], m.q2y_report_["n_iter"]
    _estimator_pass("kfold_inner", name, arena, monkeypatch, build, kfold)
    _estimator_pass("kfold_inner_grouped", name, arena, monkeypatch, build, permutation)


def test_kfold_state_tensor(arena, monkeypatch):
    import test_gpu_kfold_order4 as T4
    from cmtf_pls_amd import tPLS
    from cmtf_pls_amd.validate import get_q2y_kfold
    x, y = T4._data()

    def build(be):
        m = tPLS(T4.R, dtype="float64", options=T4.OPT, backend=be)
        m.fit(x, y)
        return m

    def kfold(m):
        q = get_q2y_kfold(m, n_splits=T4.K, per_component=True)
        T4._device_report(m.q2y_report_)
        return q, m.q2y_report_["n_iter"]
    _estimator_pass("kfold_inner_tensor", T4.SHAPE, arena, monkeypatch, build, kfold)


def test_kfold_state_coupled(arena, monkeypatch):
    import test_gpu_kfold_coupled as TC
    from cmtf_pls_amd import ctPLS
    from cmtf_pls_amd.validate import get_q2y_kfold
    name, shapes, M, R, K, _ = TC.CASES[0]                                  # tensor + matrix
    Xs, y = TC._coupled_data(shapes, M, R + 1, seed=7)

    def build(be):
        m = ctPLS(R, dtype="float64", backend=be)
        m.fit(Xs, y)
        return m

    def kfold(m):
        q = get_q2y_kfold(m, n_splits=K, per_component=True)
        assert "cmtfpls_kfold_inner_coupled_f64" in m.q2y_report_["form"] and "why" not in m.q2y_report_, m.q2y_report_
        return q, m.q2y_report_["n_iter"]
    _estimator_pass("kfold_inner_coupled", name, arena, monkeypatch, build, kfold)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("algorithm", ["xcov", "direct"])
def test_estimator_fit_and_transform(arena, monkeypatch, algorithm, dtype):
    """tPLS(3) on 300 x 8 x 12 with 3 responses, every workspace and every backend-allocated output of fit and transform in the
    arena: the call sites that the entry tests above do not enumerate.  (The rank-1 workspaces stay ordinary memory.)"""
    import oracle as O
    from cmtf_pls_amd import tPLS
    x, y, _ = O.import_synthetic((300, 8, 12), 3, 4, error=0.2, seed=5)
    if dtype == "float32":
        x = x.astype(np.float32).astype(np.float64)

    def build(be):
        m = tPLS(3, dtype=dtype, algorithm=algorithm, graphs=False, backend=be)
        m.fit(x, y)
        assert m.fit_report_["algorithm"] == algorithm, m.fit_report_
        return m

    def use(m):
        return (m.X_factors, m.Y_factors, m.coef_, m.R2X, m.R2Y, m.X_mean, m.Y_mean, list(m.n_iter_), m.transform(x))
    _estimator_pass("tPLS fit + transform", (algorithm, dtype), arena, monkeypatch, build, use)
