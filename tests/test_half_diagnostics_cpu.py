"""CPU-only: the declarations and the routing of EngineOptions.half_diagnostics (16-bit X read in place by the diagnostics).

No kernel runs here: the header, the binding table and the option are read, tpls.to_device_read is driven on a stand-in backend
that only answers has_half, and the routines run on the NumPy backend, which has no 16-bit entries: the option must change no
result there and the reports must say why a float32 copy was read."""
import os
import re

import numpy as np
import pytest
import torch

import half_storage_ref as HS
from cmtf_pls_amd import _lib, backend, storage, tpls
from cmtf_pls_amd import validate as V
from cmtf_pls_amd.engine import EngineOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = ("resid_rows", "recon_r2", "contrib_rows", "selectivity_cols")
NEW = [f"cmtfpls_{b}_{k}" for b in BASES for k in HS.KINDS]


def test_the_option_exists_and_is_off():
    assert EngineOptions().half_diagnostics is False
    assert EngineOptions(half_diagnostics=True).half_diagnostics is True
    assert EngineOptions().but(half_diagnostics=True).half_folds is False          # separate from half_folds


def test_the_eight_entries_are_declared_bound_and_listed():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cmtfpls.h")).read(), flags=re.S)
    for name in NEW:
        decl = re.search(rf"\bint {name}\s*\(\s*const uint16_t\*\s*X\b", text)
        assert decl, f"{name} is not declared with X as const uint16_t*"
        assert name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.rsplit("_", 1)[0] + "_f32"]      # every other argument is _f32's
    for b in BASES:
        assert b in backend._HALF_ENTRIES
    assert re.search(r"\bint cmtfpls_abi_version\b", text)


@pytest.mark.parametrize("kind", HS.KINDS)
def test_host_checks_answer_as_the_f32_entries(kind):
    """Every decline happens in the host code the 16-bit entries share with _f32, before a pointer is read or a kernel launched:
    the same status for R = 17, a workspace one byte short and a null X (stand-in pointers)."""
    import ctypes

    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    I, A, B, M = 70, 8, 8, 3

    def resid(sfx, X=p, R=5, short=0):
        need = lib.cmtfpls_resid_rows_workspace_bytes(I, A * B)
        return getattr(lib, f"cmtfpls_resid_rows_{sfx}")(X, p, I, R, R, p, p, A, B, p, p, p, p, need - short, None)

    def r2(sfx, X=p, R=5, short=0):
        need = lib.cmtfpls_recon_r2_workspace_bytes(I, A * B)
        return getattr(lib, f"cmtfpls_recon_r2_{sfx}")(X, p, I, R, R, p, p, A, B, p, p, p, need - short, None)

    def contrib(sfx, X=p, R=5, A_=A):
        return getattr(lib, f"cmtfpls_contrib_rows_{sfx}")(X, I, p, R, p, R, R, p, p, A_, B, p, None, I, p, p, p, p, None)

    def sel(sfx, X=p, short=0):
        need = lib.cmtfpls_selectivity_cols_workspace_bytes(I, A * B, M)
        return getattr(lib, f"cmtfpls_selectivity_cols_{sfx}")(X, I, A * B, p, M, M, p, 1, p, p, p, p, p, need - short, None)

    for fn in (resid, r2):
        for kw, status in ((dict(R=17), 4), (dict(short=1), 2), (dict(X=None), 1)):
            assert fn("f32", **kw) == fn(kind, **kw) == status, (fn.__name__, kw)
    for kw, status in ((dict(R=17), 4), (dict(A_=5000, R=16), 4), (dict(X=None), 1)):          # 2 A (R + 1) doubles beyond the LDS
        assert contrib("f32", **kw) == contrib(kind, **kw) == status, kw
    for kw, status in ((dict(short=1), 2), (dict(X=None), 1)):
        assert sel("f32", **kw) == sel(kind, **kw) == status, kw


class _Backend:
    name = "stand-in"

    def __init__(self, missing=()):
        self.missing = tuple(missing)

    def has_half(self, base):
        return base not in self.missing


class _Engine:
    def __init__(self, opt, be):
        self.opt, self.be = opt, be


class _Model:
    def __init__(self, opt, be):
        self._engine = _Engine(opt, be)
        self._storage = storage.StorageNotes()

    def _get_engine(self):
        return self._engine


@pytest.mark.parametrize("kind", HS.KINDS)
def test_the_read_follows_the_option_the_entry_and_the_backend(kind):
    x64 = np.random.default_rng(5).normal(size=(12, 4, 3))
    q, up = HS.quantise(x64, kind)
    dt, name = HS.TORCH[kind], HS.NAMES[kind]

    off = _Model(EngineOptions(), _Backend())
    X = tpls.to_device_read(q, dt, "cpu", pls=off, entry="resid_rows")
    assert X.dtype == torch.float32 and np.array_equal(X.double().numpy(), up)
    assert off._storage.upcasts == [name] and off._storage.whys == [] and off._storage.reads == []      # the general reason

    on = _Model(EngineOptions(half_diagnostics=True), _Backend())
    for entry in BASES:
        X = tpls.to_device_read(q, dt, "cpu", pls=on, entry=entry)
        assert X.dtype == dt and X.data_ptr() == q.data_ptr()                                  # the caller's own tensor
    host = tpls.to_device_read(x64, dt, "cpu", pls=on, entry="resid_rows")                     # a float64 array: rounded once
    assert host.dtype == dt and torch.equal(host.view(torch.int16), q.view(torch.int16))
    assert on._storage.upcasts == []
    assert on._storage.reads == [(name, (f"cmtfpls_{e}_{kind}",)) for e in BASES + ("resid_rows",)]

    for entry, word in (("impute", "impute returns a float32 tensor"), ("q2x_heldout", "the refit writes")):
        m = _Model(EngineOptions(half_diagnostics=True), _Backend())
        assert tpls.to_device_read(q, dt, "cpu", pls=m, entry=entry).dtype == torch.float32
        assert m._storage.upcasts == [name] and word in m._storage.whys[0] and m._storage.reads == []

    lacking = _Model(EngineOptions(half_diagnostics=True), _Backend(missing=("contrib_rows",)))
    assert tpls.to_device_read(q, dt, "cpu", pls=lacking, entry="contrib_rows").dtype == torch.float32
    assert "cmtfpls_contrib_rows_*" in lacking._storage.whys[0] and "stand-in" in lacking._storage.whys[0]
    assert tpls.to_device_read(q, dt, "cpu", pls=lacking, entry="resid_rows").dtype == dt

    # a read without an entry (the resampling drivers), and float32 storage, are what they were
    plain = _Model(EngineOptions(half_diagnostics=True), _Backend())
    assert tpls.to_device_read(q, dt, "cpu", pls=plain).dtype == torch.float32 and plain._storage.whys == []
    x32 = torch.randn(5, 3)
    assert tpls.to_device_read(x32, torch.float32, "cpu", pls=plain, entry="resid_rows").data_ptr() == x32.data_ptr()
    assert plain._storage.reads == []

    # a block whose kernel declined after an in-place read: noted as an upcast with the pass's own reason
    storage.notes_of(on).declined([q, x32], [{"form": "torch fallback", "why": "R = 17 > 16: outside cmtfpls_resid_rows"}, {"form": "f", "why": "x"}])
    assert on._storage.upcasts == [name] and on._storage.whys == ["R = 17 > 16: outside cmtfpls_resid_rows"]


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=True)
    return a == b or (a != a and b != b)


@pytest.mark.parametrize("kind", HS.KINDS)
def test_numpy_backend_results_do_not_change_and_the_reports_say_why(kind):
    from numpy_backend import NumpyBackend
    from cmtf_pls_amd import tPLS

    rng = np.random.default_rng(3)
    x, y = rng.normal(size=(30, 4, 5)), rng.normal(size=(30, 2))
    res = {}
    for on in (False, True):
        m = tPLS(3, dtype=HS.NAMES[kind], backend=NumpyBackend(), algorithm="xcov", options=EngineOptions(small_fit=False, half_diagnostics=on))
        m.fit(x, y)
        out = [V.sample_diagnostics(m), V.sample_contributions(m, rows=np.array([1, 4])), V.selectivity_ratio(m), m.R2X_literal(x)]
        reps = [m.diagnostics_report_, m.contributions_report_, m.importance_report_, m.r2x_literal_report_]
        phrase = f"float32 private copy of the {HS.NAMES[kind]} data: "
        for rep, entry in zip(reps, ("resid_rows", "contrib_rows", "selectivity_cols", "recon_r2")):
            assert rep["storage_fallback"].startswith(phrase) and "half_storage" not in rep
            assert (f"has no 16-bit form of cmtfpls_{entry}_*" in rep["storage_fallback"]) == on, rep
        res[on] = out
    assert _same(res[True], res[False])
