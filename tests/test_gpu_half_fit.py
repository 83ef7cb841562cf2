"""Fit, transform and the routines beside them with 16-bit storage of X (dtype="bfloat16" / "float16"), on the GPU.

A 16-bit device tensor is only ever read: algorithm="xcov" runs on it in place (statistics and S from one read, then one read per
component through score_contract, or two through mttkrp + xcov where score_contract declines the block), transform / predict take
the one-pass MTTKRP in place.  Everything else runs on an exact float32 upcast and is therefore, bit for bit, a float32 model.

Models (tests/half_storage_ref.py): tPLS (300, 16, 256) one-read, (300, 12, 20) two-read, (300, 40), (120, 6, 4, 8); ctPLS (300, 16, 256)
+ (300, 24); R = 4, M = 3.  The data is quantised to the storage type on the host; the float64 oracle runs on the exact upcast.
Bounds against the oracle: those tests/test_gpu_r10_parity.py holds float64 storage to (factor columns and coef_ normwise 1e-9,
R2X / R2Y absolute 1e-11, transform normwise 1e-9) -- they apply because the upcast is exact: both sides compute in float64 on the
same values.  n_iter_ equals that of a float32 xcov model on the upcast tensor; the seeds were picked on the CPU such that the
oracle's convergence norm is nowhere within a factor 10 of tol at a stopping iteration or the one before (asserted here).
"""
import numpy as np
import pytest
import torch

import half_storage_ref as HS
import oracle as O
from parity_metrics import column_errors, fit_error_table, worst

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
R = HS.FIT_R
# seeds with clear convergence of every component (half_storage_ref.convergence_is_clear), found by running the oracle on the CPU
SEEDS = {
    ("one-read", "bf16"): 8, ("one-read", "f16"): 6, ("two-read", "bf16"): 2, ("two-read", "f16"): 8, ("matrix", "bf16"): 45,
    ("matrix", "f16"): 23, ("order-4", "bf16"): 3, ("order-4", "f16"): 3, ("coupled", "bf16"): 9, ("coupled", "f16"): 9,
}
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


def _case(name, kind):
    """The quantised blocks (device, 16-bit), their exact upcasts, y, the new rows likewise, the oracle's fit and its norms: once."""
    key = (name, kind)
    if key not in _cache:
        blocks, y, new = HS.fit_data(name, SEEDS[key])
        q = [HS.quantise(b, kind) for b in blocks]
        qn = [HS.quantise(b, kind) for b in new]
        ups = [u for _, u in q]
        fit, norms = HS.oracle_fit_with_norms(ups, y, R)
        _cache[key] = dict(X16=[t.to(DEV) for t, _ in q], up=ups, y=y, new16=[t.to(DEV) for t, _ in qn], newup=[u for _, u in qn],
                           fit=fit, norms=norms, coupled=len(blocks) > 1)
    return _cache[key]


def _arg(c, xs):
    return list(xs) if c["coupled"] else xs[0]


def _model(api, c, **kw):
    return (api.ctPLS if c["coupled"] else api.tPLS)(R, algorithm=kw.pop("algorithm", "xcov"), **kw)


def _bits(t):
    return t.view(torch.int16).clone()


def _attributes(m, coupled):
    out = {"coef_": m.coef_, "R2Y": np.asarray(m.R2Y), "Y_mean": m.Y_mean, "Q": m.Y_factors[1], "U": m.Y_factors[0],
           "n_iter_": np.asarray(m.n_iter_)}
    if coupled:
        for b, fac in enumerate(m.Xs_factors):
            for k, f in enumerate(fac):
                out[f"Xs_factors[{b}][{k}]"] = f
            out[f"R2Xs[{b}]"] = np.asarray(m.R2Xs[b])
            out[f"Xs_mean[{b}]"] = m.Xs_mean[b]
    else:
        for k, f in enumerate(m.X_factors):
            out[f"X_factors[{k}]"] = f
        out["R2X"], out["X_mean"] = np.asarray(m.R2X), m.X_mean
    return out


def _assert_same_bits(a, b, coupled, what):
    fa, fb = _attributes(a, coupled), _attributes(b, coupled)
    for k in fa:
        assert np.array_equal(fa[k], fb[k], equal_nan=True), f"{what}: {k} differs from the float32 model on the upcast data"


@pytest.mark.parametrize("kind", HS.KINDS)
@pytest.mark.parametrize("name", list(HS.FIT_MODELS))
def test_fit_and_transform_in_place_against_the_float64_oracle(api, name, kind):
    c = _case(name, kind)
    fit = c["fit"]
    assert HS.convergence_is_clear(fit, c["norms"]), (fit.n_iter, c["norms"])       # the precondition of the n_iter_ comparison
    keep, keep_new = [_bits(x) for x in c["X16"]], [_bits(x) for x in c["new16"]]
    m = _model(api, c, dtype=HS.NAMES[kind])
    m.fit(_arg(c, c["X16"]), c["y"])
    rep = m.fit_report_
    nb = len(c["X16"])
    for b in range(nb):
        rows, extra = fit_error_table(m, fit, b)
        err, fac, comp = worst(rows)
        print(f"{name} {kind} block {b}: factors {err:.3g} ({fac}[:, {comp}]) R2X {max(extra['R2X_abs']):.3g} R2Y {max(extra['R2Y_abs']):.3g} "
              f"coef {extra['coef_normwise']:.3g} n_iter {extra['n_iter']} oracle {extra['n_iter_oracle']}")
        assert err <= 1e-9, f"normwise error {err:.3e} in {fac}[:, {comp}]"
        assert max(extra["R2X_abs"]) <= 1e-11 and max(extra["R2Y_abs"]) <= 1e-11 and extra["coef_normwise"] <= 1e-9
    got = m.transform(_arg(c, c["new16"]))
    terr = column_errors(got, O.transform(fit, _arg(c, c["newup"])))["normwise"].max()
    print(f"{name} {kind}: transform {terr:.3g}")
    assert terr <= 1e-9
    prep = m.projection_report_
    assert prep["form"].startswith("one-pass MTTKRP") and "storage_fallback" not in prep
    assert prep["storage"] == [HS.NAMES[kind]] * nb
    # the same data as a float32 tensor on the same device: the same iterations
    ref = _model(api, c, dtype="float32")
    ref.fit(_arg(c, [x.to(torch.float32) for x in c["X16"]]), c["y"])
    assert list(m.n_iter_) == list(ref.n_iter_), (m.n_iter_, ref.n_iter_)
    # what ran
    assert rep["algorithm"] == "xcov" and rep["raw"] is True and rep["x_written"] is False and rep["stats_with_s"] is True
    assert rep["x_copy"].startswith("none") and rep["storage"] == [HS.NAMES[kind]] * nb
    hs = rep["half_storage"]
    assert hs["in_place"] is True and hs["fallback"] is None
    want_reads = {"one-read": ["one-read"], "two-read": ["two-read"], "matrix": ["two-read"], "order-4": ["two-read"],
                  "coupled": ["one-read", "two-read"]}[name]
    assert [r.split(" ")[0] for r in hs["reads"]] == want_reads, hs["reads"]
    # only ever read
    for x, k in zip(c["X16"] + c["new16"], keep + keep_new):
        assert torch.equal(x.view(torch.int16), k), "a 16-bit tensor was written"


@pytest.mark.parametrize("kind", HS.KINDS)
def test_fit_allocates_less_than_one_copy_of_x(api, kind):
    """(16384, 64, 64): X is 134 MB at 16 bits; the workspaces are about 16 MB, so a full-size copy in any type shows."""
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    I, A, B = 16384, 64, 64
    T = torch.randn(I, 3, generator=g, device=DEV)
    W = torch.randn(3, A * B, generator=g, device=DEV)
    X = (T @ W + 0.1 * torch.randn(I, A * B, generator=g, device=DEV)).to(HS.TORCH[kind]).view(I, A, B)
    y = (T @ torch.randn(3, 3, generator=g, device=DEV)).double().cpu().numpy()
    del T, W
    keep = _bits(X)
    nbytes = X.numel() * X.element_size()
    assert nbytes == 134217728
    m = api.tPLS(R, dtype=HS.NAMES[kind], algorithm="xcov")
    m._get_engine()                                                          # (the backend's own start-up is not the fit's)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m.fit(X, y)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"{kind}: peak rise during fit {rise / 2 ** 20:.1f} MiB, X {nbytes / 2 ** 20:.1f} MiB")
    assert rise < nbytes
    assert m.fit_report_["half_storage"]["in_place"] and m.fit_report_["half_storage"]["reads"] == ["one-read (score_contract)"]
    assert torch.equal(X.view(torch.int16), keep)
    del keep
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m.transform(X)
    rise = torch.cuda.max_memory_allocated() - base
    print(f"{kind}: peak rise during transform {rise / 2 ** 20:.1f} MiB")
    assert rise < nbytes and m.projection_report_["form"].startswith("one-pass MTTKRP")


@pytest.mark.parametrize("kind", HS.KINDS)
def test_a_single_component_reads_the_block_once_and_says_so(api, kind):
    c = _case("two-read", kind)
    m = api.tPLS(1, dtype=HS.NAMES[kind], algorithm="xcov")
    m.fit(c["X16"][0], c["y"])
    hs = m.fit_report_["half_storage"]
    assert hs["in_place"] is True and hs["reads"] == ["one read (mttkrp: a single component needs no down-date of S)"]
    ref = api.tPLS(1, dtype="float32", algorithm="xcov")
    ref.fit(c["X16"][0].to(torch.float32), c["y"])
    assert column_errors(m.X_factors[0], ref.X_factors[0])["normwise"].max() <= 1e-9 and list(m.n_iter_) == list(ref.n_iter_)


def _fallback_pair(api, c, kind, X16, **kw):
    m = _model(api, c, dtype=HS.NAMES[kind], **dict(kw))
    m.fit(_arg(c, X16), c["y"])
    ref = _model(api, c, dtype="float32", **dict(kw))
    ref.fit(_arg(c, [x.to(torch.float32) for x in X16]), c["y"])
    return m, ref


@pytest.mark.parametrize("kind", HS.KINDS)
@pytest.mark.parametrize("name", ["one-read", "coupled"])
def test_fallbacks_are_the_float32_model_bit_for_bit(api, name, kind):
    from cmtf_pls_amd.engine import default_options

    c = _case(name, kind)
    phrase = f"float32 private copy of the {HS.NAMES[kind]} data: "
    keep = [_bits(x) for x in c["X16"]]
    # algorithm="direct"
    m, ref = _fallback_pair(api, c, kind, c["X16"], algorithm="direct")
    _assert_same_bits(m, ref, c["coupled"], "direct")
    why = m.fit_report_["half_storage"]["fallback"]
    assert why.startswith(phrase) and "direct" in why and why in m.fit_report_["declined"] and not m.fit_report_["half_storage"]["in_place"]
    # a NaN in X
    Xn = [x.clone() for x in c["X16"]]
    Xn[0].view(Xn[0].shape[0], -1)[17, 5] = float("nan")
    m, ref = _fallback_pair(api, c, kind, Xn)
    _assert_same_bits(m, ref, c["coupled"], "NaN")
    why = m.fit_report_["half_storage"]["fallback"]
    assert why.startswith(phrase) and "missing" in why and m.fit_report_["missing"][0] is True
    # data offset beyond xcov_raw_max_offset
    opt = default_options().but(xcov_raw_max_offset=0.25)
    Xo = [(x.double() + 2.0).to(x.dtype) for x in c["X16"]]
    m, ref = _fallback_pair(api, c, kind, Xo, options=opt)
    _assert_same_bits(m, ref, c["coupled"], "offset")
    why = m.fit_report_["half_storage"]["fallback"]
    assert why.startswith(phrase) and "max|column mean| / spread" in why
    assert ref.fit_report_["raw"] is False and m.fit_report_["raw"] is False
    # a transform batch with a NaN row, on the in-place model and on the float32 model of the same upcast data
    m, ref = _fallback_pair(api, c, kind, c["X16"])
    assert m.fit_report_["half_storage"]["in_place"]
    new = [x.clone() for x in c["new16"]]
    new[0].view(new[0].shape[0], -1)[9, 3] = float("nan")
    twin = m.copy()
    twin._dtype = "float32"                                                   # the same fitted state, read as a float32 model reads it
    got = m.transform(_arg(c, new))
    why = m.projection_report_["storage_fallback"]
    want = twin.transform(_arg(c, [x.to(torch.float32) for x in new]))
    assert np.array_equal(got, want, equal_nan=True)
    assert why.startswith(phrase) and "missing" in why
    assert np.array_equal(m.predict(_arg(c, new)), twin.predict(_arg(c, [x.to(torch.float32) for x in new])), equal_nan=True)
    for x, k in zip(c["X16"], keep):
        assert torch.equal(x.view(torch.int16), k)


def test_the_other_routines_see_what_the_model_saw(api):
    from cmtf_pls_amd import validate as V

    c = _case("one-read", "f16")
    x64 = HS.fit_data("one-read", SEEDS[("one-read", "f16")])[0][0]           # float64 NumPy, NOT representable in float16
    assert not HS.is_exact_upcast(x64, "f16")
    m = api.tPLS(R, dtype="float16", algorithm="xcov")
    m.fit(x64, c["y"])
    assert m.fit_report_["half_storage"]["in_place"]                          # (the upload was cast to the storage type)
    x32 = x64.astype(np.float16).astype(np.float32)
    ref = api.tPLS(R, dtype="float32", algorithm="xcov")
    ref.fit(x32, c["y"])
    qa, qb = V.get_q2y_kfold(m, n_splits=5, per_component=True), V.get_q2y_kfold(ref, n_splits=5, per_component=True)
    print("q2y 16-bit model:", m.q2y_report_.get("form"), "| float32 model:", ref.q2y_report_.get("form"), np.asarray(qa) - np.asarray(qb))
    assert np.array_equal(np.asarray(qa), np.asarray(qb))
    phrase = "float32 private copy of the float16 data: "
    assert m.q2y_report_["storage_fallback"].startswith(phrase) and "storage_fallback" not in ref.q2y_report_
    # the same data in another container (a float64 torch tensor) is the same model, bit for bit
    m2 = api.tPLS(R, dtype="float16", algorithm="xcov")
    m2.fit(torch.from_numpy(x64), c["y"])
    _assert_same_bits(m2, m, False, "float64 torch tensor against float64 NumPy array")
    # a twin with the same fitted state, float32 storage and the upcast training tensor
    twin = m.copy()
    twin._dtype = "float32"
    twin.original_X = x32
    for fn, kw in ((V.sample_diagnostics, {}), (V.sample_contributions, {"rows": np.array([0, 5, 299])}), (V.selectivity_ratio, {})):
        a, b = fn(m, **kw), fn(twin, **kw)
        attr = {"sample_diagnostics": "diagnostics_report_", "sample_contributions": "contributions_report_",
                "selectivity_ratio": "importance_report_"}[fn.__name__]
        assert getattr(m, attr)["storage_fallback"].startswith(phrase), attr         # the report says that a float32 copy was made
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k], equal_nan=True), (fn.__name__, k)
            elif isinstance(a[k], list) and a[k] and isinstance(a[k][0], np.ndarray):
                assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a[k], b[k])), (fn.__name__, k)
    gap16 = x64.copy()
    gap16[3, 2, 7] = np.nan
    ia, ib = V.impute(m, gap16), V.impute(twin, gap16.astype(np.float16).astype(np.float32))
    assert ia.dtype == np.float64 and np.array_equal(ia[3, 2, 7], np.float64(ib[3, 2, 7])) and np.isfinite(ia[3, 2, 7])
    xd = torch.from_numpy(gap16).to(DEV)
    filled = V.impute(m, xd)
    assert filled.dtype == torch.float32 and filled.is_cuda                  # never rounded back to 16 bits
    assert float(filled[3, 2, 7]) == float(ib[3, 2, 7])
    assert m.imputation_report_["storage_fallback"].startswith(phrase) and "storage_fallback" not in twin.imputation_report_
    assert m.R2X_literal(x64) == twin.R2X_literal(x32)
