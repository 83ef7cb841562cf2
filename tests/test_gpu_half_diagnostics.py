"""EngineOptions.half_diagnostics: the read-only diagnostics of a model with 16-bit storage on the caller's 16-bit tensor itself
(tpls.to_device_read with an entry, cmtfpls_{resid_rows,contrib_rows,selectivity_cols,recon_r2}_{bf16,f16}), tPLS and ctPLS.

Data: half_storage_ref.fit_data at (300, 12, 10), coupled (300, 12, 10) + (300, 20) and order 4 (120, 12, 8, 5); R = 3, M = 2.
The model is fitted with 16-bit storage, algorithm="xcov" and EngineOptions(small_fit=False, half_diagnostics=True) and compared
with the same model without the option -- the route that reads an exact float32 upcast, which tests/test_gpu_half_fit.py ties to
the float32 twin.  The 16-bit kernels use the f32 entries' thread-to-column mapping, so the comparison is EQUALITY: every array of
every result np.array_equal(equal_nan=True), the reports' form and x_reads equal.  Measured on MI355X: DESIGN 8w ("Diagnostics")."""
from unittest import mock

import numpy as np
import pytest
import torch

import half_storage_ref as HS
from cmtf_pls_amd import validate as V
from cmtf_pls_amd.engine import EngineOptions

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R, M = 3, 2
SHAPES = {"tPLS": ("two-read", [(300, 12, 10)], 2), "ctPLS": ("coupled", [(300, 12, 10), (300, 20)], 9),
          "order-4": ("order-4", [(120, 12, 8, 5)], 3)}
PHRASE = "float32 private copy of the {} data: "
_cache = {}


@pytest.fixture(scope="module")
def api():
    import cmtf_pls_amd
    return cmtf_pls_amd


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _cache.clear()
    torch.cuda.empty_cache()


def _fit(api, X16, y, kind, on, n_components=R):
    coupled = len(X16) > 1
    cls = api.ctPLS if coupled else api.tPLS
    m = cls(n_components, dtype=HS.NAMES[kind], algorithm="xcov", options=EngineOptions(small_fit=False, half_diagnostics=on))
    m.fit(X16 if coupled else X16[0], y)
    return m


def _case(api, which, kind):
    """Per case, once: the 16-bit blocks on the device (complete, and with a few NaN), new rows, and the four fitted models."""
    key = (which, kind)
    if key not in _cache:
        name, shapes, seed = SHAPES[which]
        with mock.patch.dict(HS.FIT_MODELS, {name: shapes}):
            blocks, y, new = HS.fit_data(name, seed)
        y = np.ascontiguousarray(y[:, :M])
        X16 = [HS.quantise(b, kind)[0].to(DEV) for b in blocks]
        gaps = []
        for b, x in enumerate(X16):
            xg = x.clone()
            flat = xg.view(-1)
            flat[torch.arange(7, flat.numel(), flat.numel() // 13, device=DEV)] = float("nan")
            gaps.append(xg)
        c = dict(X16=X16, gaps=gaps, y=y, new=[np.ascontiguousarray(n) for n in new],
                 new16=[HS.quantise(n, kind)[0].to(DEV) for n in new], coupled=len(blocks) > 1)
        c["on"], c["off"] = _fit(api, X16, y, kind, True), _fit(api, X16, y, kind, False)
        assert c["on"].fit_report_["half_storage"]["in_place"], c["on"].fit_report_
        c["gap_on"], c["gap_off"] = _fit(api, gaps, y, kind, True), _fit(api, gaps, y, kind, False)
        c["watch"] = [(x, x.data_ptr(), x.view(torch.int16).clone()) for x in X16 + gaps + c["new16"]]
        _cache[key] = c
    return _cache[key]


def _untouched(c):
    for x, ptr, bits in c["watch"]:
        assert x.data_ptr() == ptr and torch.equal(x.view(torch.int16), bits)


def _same(a, b, where):
    if isinstance(a, dict):
        assert set(a) == set(b), where
        for k in a:
            _same(a[k], b[k], f"{where}[{k}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (p, q) in enumerate(zip(a, b)):
            _same(p, q, f"{where}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (where, int((a != b).sum()))
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), (where, a, b)
    else:
        assert a == b, (where, a, b)


def _both(c, on, off, fn, attr, kind, entries, **kw):
    """fn on the model with the option and on the one without: equal results, equal form and x_reads, and each report naming its
    route (half_storage with the entries | storage_fallback with the float32 copy)."""
    a, b = fn(on, **kw), fn(off, **kw)
    _same(a, b, fn.__name__)
    ra, rb = getattr(on, attr), getattr(off, attr)
    assert ra["form"] == rb["form"] and ra["x_reads"] == rb["x_reads"], (ra, rb)
    assert "storage_fallback" not in ra and ra["half_storage"]["in_place"] is True, ra
    assert ra["half_storage"]["dtype"] == HS.NAMES[kind]
    assert ra["half_storage"]["entries"] == sorted(f"cmtfpls_{e}_{kind}" for e in entries), ra
    assert rb["storage_fallback"].startswith(PHRASE.format(HS.NAMES[kind])) and "half_storage" not in rb, rb
    assert "torch fallback" not in str(ra["form"]), ra
    _untouched(c)
    return a


@pytest.mark.parametrize("kind", HS.KINDS)
@pytest.mark.parametrize("which", list(SHAPES))
def test_every_routine_equals_the_upcast_route(api, which, kind):
    c = _case(api, which, kind)
    on, off, coupled = c["on"], c["off"], c["coupled"]
    one = (lambda v: v) if coupled else (lambda v: v[0])
    # sample_diagnostics: training rows (the training-statistics pass comes out of the same read), new rows on the device, new
    # rows as a NumPy array (uploaded once in the storage type)
    d = _both(c, on, off, V.sample_diagnostics, "diagnostics_report_", kind, ["resid_rows"])
    assert all(np.isfinite(s).all() for s in (d["spe"] if coupled else [d["spe"]])) and on.diagnostics_report_["training_stats"] == "computed"
    _both(c, on, off, V.sample_diagnostics, "diagnostics_report_", kind, ["resid_rows"], X=one(c["new16"]))
    _both(c, on, off, V.sample_diagnostics, "diagnostics_report_", kind, ["resid_rows"], X=one(c["new"]))
    # sample_contributions: a row subset, with and without the cells; new rows
    rows = np.array([0, 5, 99, 117])
    _both(c, on, off, V.sample_contributions, "contributions_report_", kind, ["contrib_rows"], rows=rows)
    k = _both(c, on, off, V.sample_contributions, "contributions_report_", kind, ["contrib_rows"], rows=rows, cells=True)
    assert "spe_cells" in k
    _both(c, on, off, V.sample_contributions, "contributions_report_", kind, ["contrib_rows"], X=one(c["new16"]), rows=np.array([1, 63]))
    # selectivity_ratio: complete, and a model whose training tensor holds a few NaN (the masked form)
    _both(c, on, off, V.selectivity_ratio, "importance_report_", kind, ["selectivity_cols"])
    assert on.importance_report_["masked"] == ["complete"] * len(c["X16"])
    _both(c, c["gap_on"], c["gap_off"], V.selectivity_ratio, "importance_report_", kind, ["selectivity_cols"])
    assert c["gap_on"].importance_report_["masked"] == ["masked"] * len(c["X16"])
    # ... whose other diagnostics read the NaN in place as well (a fresh model: the training statistics are computed by the
    # contributions call, through resid_rows)
    _both(c, c["gap_on"], c["gap_off"], V.sample_contributions, "contributions_report_", kind, ["contrib_rows", "resid_rows"], rows=rows)
    _both(c, c["gap_on"], c["gap_off"], V.sample_diagnostics, "diagnostics_report_", kind, ["resid_rows"])
    if not coupled:
        ra, rb = on.R2X_literal(c["X16"][0]), off.R2X_literal(c["X16"][0])
        assert ra == rb and np.isfinite(ra)
        assert on.r2x_literal_report_["half_storage"] == {"in_place": True, "dtype": HS.NAMES[kind], "entries": [f"cmtfpls_recon_r2_{kind}"]}
        assert "storage_fallback" not in on.r2x_literal_report_ and on.r2x_literal_report_["form"] == off.r2x_literal_report_["form"]
        assert off.r2x_literal_report_["storage_fallback"].startswith(PHRASE.format(HS.NAMES[kind]))
        _untouched(c)


@pytest.mark.parametrize("kind", HS.KINDS)
def test_the_routes_that_still_upcast_say_why(api, kind):
    c = _case(api, "tPLS", kind)
    on, off = c["on"], c["off"]
    phrase = PHRASE.format(HS.NAMES[kind])
    gap = c["gaps"][0]
    fa, fb = V.impute(on, gap), V.impute(off, gap)
    assert fa.dtype == torch.float32 and torch.equal(fa.view(torch.int32), fb.view(torch.int32))
    rep = on.imputation_report_
    assert rep["storage_fallback"].startswith(phrase + "EngineOptions.half_diagnostics: impute returns a float32 tensor") and "half_storage" not in rep
    assert off.imputation_report_["storage_fallback"].startswith(phrase) and "half_diagnostics" not in off.imputation_report_["storage_fallback"]
    qa, qb = V.get_q2x_heldout(on, n_repeats=1), V.get_q2x_heldout(off, n_repeats=1)
    strip = lambda q: {k: ({j: w for j, w in v.items() if j != "storage_fallback"} if k == "report" else v) for k, v in q.items()}   # noqa: E731
    _same(strip(qa), strip(qb), "get_q2x_heldout")                           # (the returned report names the copy's reason)
    rep = on.q2x_report_
    assert rep["storage_fallback"].startswith(phrase + "EngineOptions.half_diagnostics: get_q2x_heldout refits") and "half_storage" not in rep
    _untouched(c)
    # R = 17: every kernel with loadings in registers declines; the torch fallback reads a float32 upcast of the block
    g = torch.Generator(device=DEV).manual_seed(3)
    X16 = torch.randn(60, 20, 18, device=DEV, generator=g).to(HS.TORCH[kind])
    y = torch.randn(60, M, device=DEV, generator=g).double().cpu().numpy()
    keep = X16.view(torch.int16).clone()
    big_on, big_off = _fit(api, [X16], y, kind, True, 17), _fit(api, [X16], y, kind, False, 17)
    for fn, attr, kw in ((V.sample_diagnostics, "diagnostics_report_", {}), (V.sample_contributions, "contributions_report_", {"rows": np.array([2, 9])})):
        _same(fn(big_on, **kw), fn(big_off, **kw), fn.__name__)
        rep = getattr(big_on, attr)
        assert rep["storage_fallback"].startswith(phrase + "R = 17 > 16: outside cmtfpls_") and "half_storage" not in rep, rep
        assert "torch fallback" in str(rep["form"])
    assert big_on.R2X_literal(X16) == big_off.R2X_literal(X16)
    rep = big_on.r2x_literal_report_
    assert rep["storage_fallback"].startswith(phrase + "R = 17 > 16: outside cmtfpls_recon_r2") and "half_storage" not in rep
    # selectivity_cols holds no loadings: it takes 17 components in place
    _same(V.selectivity_ratio(big_on), V.selectivity_ratio(big_off), "selectivity_ratio R = 17")
    assert big_on.importance_report_["half_storage"]["entries"] == [f"cmtfpls_selectivity_cols_{kind}"]
    assert torch.equal(X16.view(torch.int16), keep)


def test_no_float32_copy_is_made(api):
    """(16384, 64, 64) bfloat16: X is 128 MiB, the float32 copy that must not exist 256 MiB.  The rise of the peak allocation
    during sample_diagnostics, selectivity_ratio and sample_contributions on 256 rows stays below I P 4 bytes; the float32 twin's own
    rise on its in-place tensor (the same workspaces) is below half of that, so the condition separates the two routes."""
    I, A, B = 16384, 64, 64
    g = torch.Generator(device=DEV).manual_seed(11)
    T = torch.randn(I, R, device=DEV, generator=g) * torch.tensor([1.0, 0.5, 0.25], device=DEV)
    X32 = torch.einsum("il,jl,kl->ijk", T, torch.randn(A, R, device=DEV, generator=g), torch.randn(B, R, device=DEV, generator=g))
    X32 += 0.05 * torch.randn(I, A, B, device=DEV, generator=g)
    y = (T.double() @ torch.randn(R, M, device=DEV, generator=g).double()).cpu().numpy()
    X16 = X32.to(torch.bfloat16)
    X32 = X16.to(torch.float32)
    copy = I * A * B * 4
    rows = np.arange(0, I, I // 256)
    routines = ((V.sample_diagnostics, "diagnostics_report_", {}), (V.selectivity_ratio, "importance_report_", {"cells": False}),
                (V.sample_contributions, "contributions_report_", {"rows": rows}))
    rises = {}
    for name, X, dtype in (("bfloat16 in place", X16, "bfloat16"), ("float32 twin", X32, "float32")):
        m = api.tPLS(R, dtype=dtype, algorithm="xcov", options=EngineOptions(small_fit=False, half_diagnostics=True))
        m.fit(X, y)
        for fn, attr, kw in routines:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn(m, **kw)
            torch.cuda.synchronize()
            rises[name, fn.__name__] = torch.cuda.max_memory_allocated() - base
            rep = getattr(m, attr)
            assert "storage_fallback" not in rep and "torch fallback" not in str(rep["form"]), rep
            assert ("half_storage" in rep) == (dtype == "bfloat16")
        del m
    print(f"peak rise: {rises} bytes; the float32 copy would be {copy}")
    for fn, _, _ in routines:
        assert rises["float32 twin", fn.__name__] < copy // 2, fn.__name__
        assert rises["bfloat16 in place", fn.__name__] < copy, fn.__name__
