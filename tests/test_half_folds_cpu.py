"""CPU-only: the declarations and the routing of EngineOptions.half_folds (16-bit X read in place by the resampling drivers).

No kernel runs here: the header, the binding table and the option are read, and kfold._device_blocks is driven on a stand-in
backend that only answers has_half (the one question the routing asks of a backend)."""
import os
import re

import numpy as np
import pytest
import torch

import half_storage_ref as HS
from cmtf_pls_amd import _lib, backend, kfold, storage
from cmtf_pls_amd.engine import EngineOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDERS = ("kfold_xcov", "kfold_wide_xcov", "kfold_weighted_xcov")
NEW = [f"cmtfpls_{b}_{k}" for b in BUILDERS for k in HS.KINDS]


def test_the_six_entries_are_declared_bound_and_listed():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cmtfpls.h")).read(), flags=re.S)
    for name in NEW:
        decl = re.search(rf"\bint {name}\s*\(\s*const uint16_t\*\s*X\b", text)
        assert decl, f"{name} is not declared with X as const uint16_t*"
        assert name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.rsplit("_", 1)[0] + "_f32"]      # every other argument is _f32's
    assert EngineOptions().half_folds is False
    for b in BUILDERS:
        assert b in backend._HALF_ENTRIES
    assert set(kfold.HALF_READS) == set(BUILDERS) | {"mttkrp", "xcov"}


@pytest.mark.parametrize("kind", HS.KINDS)
def test_host_checks_answer_as_the_f32_entries(kind):
    """Every decline of the 16-bit builders happens in the host code they share with the _f32 entries, before a pointer is read or
    a kernel launched: the same status for K = 1, K = 33, W = 1025, a workspace one byte short and a null X (stand-in pointers)."""
    import ctypes

    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    I, A, B = 70, 8, 8

    def fold(name, X=p, W=3, K=5, short=0):                      # kfold_xcov / kfold_wide_xcov
        need = getattr(lib, f"cmtfpls_{name.rsplit('_', 1)[0]}_workspace_bytes")(I, A * B, W, K)
        return getattr(lib, f"cmtfpls_{name}")(X, I, A, B, p, W, p, p, K, p, p, p, p, p, need - short, None)

    def weighted(name, X=p, n=2, M=1, short=0):
        need = lib.cmtfpls_kfold_weighted_xcov_workspace_bytes(I, A * B, n, M)
        return getattr(lib, f"cmtfpls_{name}")(X, I, A, B, p, n, M, p, p, p, p, need - short, None)

    for base in ("kfold_xcov", "kfold_wide_xcov"):
        for kw, status in ((dict(K=1), 4), (dict(K=33), 4), (dict(W=1025), 4), (dict(short=1), 2), (dict(X=None), 1)):
            assert fold(f"{base}_f32", **kw) == fold(f"{base}_{kind}", **kw) == status, (base, kw)
    for kw, status in ((dict(n=33), 4), (dict(n=25, M=40), 4), (dict(short=1), 2), (dict(X=None), 1)):
        assert weighted("kfold_weighted_xcov_f32", **kw) == weighted(f"kfold_weighted_xcov_{kind}", **kw) == status, kw


class _Backend:
    """What the routing asks of a backend: whether an entry has 16-bit forms."""
    name = "stand-in"

    def __init__(self, missing=()):
        self.missing = tuple(missing)

    def has_half(self, base):
        return base not in self.missing


class _Engine:
    def __init__(self, opt, be):
        self.opt, self.be = opt, be


class _Model:
    """A model as kfold._device_blocks sees it: the storage type, the engine, and the notes that storage.reports_storage collects."""

    def __init__(self, dtype, opt, be):
        self._dtype = dtype
        self._engine = _Engine(opt, be)
        self._storage = storage.StorageNotes()

    def _get_engine(self):
        return self._engine


@pytest.mark.parametrize("kind", HS.KINDS)
def test_blocks_follow_the_option_and_the_backend(kind):
    rng = np.random.default_rng(5)
    x64 = rng.normal(size=(12, 4, 3))
    q, up = HS.quantise(x64, kind)
    mat16 = HS.quantise(rng.normal(size=(12, 5)), kind)[0]
    name = HS.NAMES[kind]

    off = _Model(name, EngineOptions(), _Backend())
    blocks = kfold._device_blocks(off, [q, mat16], "cpu")
    assert [b[0].dtype for b in blocks] == [torch.float32] * 2 and [tuple(b[0].shape) for b in blocks] == [(12, 12), (12, 5)]
    assert np.array_equal(blocks[0][0].double().numpy().reshape(up.shape), up)              # the exact upcast
    assert off._storage.upcasts == [name, name] and off._storage.whys == []          # noted, with the general reason

    on = _Model(name, EngineOptions(half_folds=True), _Backend())
    blocks = kfold._device_blocks(on, [q, mat16], "cpu")
    assert [b[0].dtype for b in blocks] == [HS.TORCH[kind]] * 2
    assert blocks[0][0].data_ptr() == q.data_ptr() and blocks[1][0].data_ptr() == mat16.data_ptr()     # the caller's own
    assert [b[1:] for b in blocks] == [(4, 3), (1, 5)]
    assert on._storage.upcasts == []
    host = kfold._device_blocks(on, [x64], "cpu")[0][0]                                     # a float64 array: the once-rounded upload
    assert host.dtype == HS.TORCH[kind] and torch.equal(host.view(torch.int16), q.view(12, -1).view(torch.int16))
    assert on._storage.upcasts == []

    lacking = _Model(name, EngineOptions(half_folds=True), _Backend(missing=("kfold_wide_xcov",)))
    blocks = kfold._device_blocks(lacking, [q], "cpu")
    assert blocks[0][0].dtype == torch.float32 and blocks[0][0].data_ptr() != q.data_ptr()
    assert lacking._storage.upcasts == [name]
    assert len(lacking._storage.whys) == 1 and "cmtfpls_kfold_wide_xcov_*" in lacking._storage.whys[0]
    assert "stand-in" in lacking._storage.whys[0]


def test_float32_storage_is_untouched_by_the_option():
    x = torch.randn(9, 4, 2)
    m = _Model("float32", EngineOptions(half_folds=True), _Backend())
    (X2, A, B), = kfold._device_blocks(m, [x], "cpu")
    assert X2.dtype == torch.float32 and X2.data_ptr() == x.data_ptr() and (A, B) == (4, 2)
    assert m._storage.upcasts == [] and m._storage.reads == []


def test_report_keys_of_the_decorator():
    """storage.reports_storage: in-place notes give half_storage only when the report shows reads of X; an upcast wins, with the
    reads' own reasons."""
    class M:
        pass

    def run(notes, x_reads):
        @storage.reports_storage("rep_", "general reason")
        def fn(pls):
            for n in notes:
                n(pls)
            pls.rep_ = {"form": "f", "x_reads": x_reads}
        m = M()
        fn(m)
        return m.rep_

    inplace = lambda p: storage.notes_of(p).in_place(torch.bfloat16, ["kfold_xcov", "mttkrp"])   # noqa: E731
    rep = run([inplace, inplace], 6)
    assert rep["half_storage"] == {"in_place": True, "dtype": "bfloat16", "entries": ["cmtfpls_kfold_xcov_bf16", "cmtfpls_mttkrp_bf16"]}
    assert "storage_fallback" not in rep
    assert "half_storage" not in run([inplace], None) and "storage_fallback" not in run([inplace], None)     # every model refitted
    rep = run([lambda p: storage.notes_of(p).upcast(torch.float16)], 6)
    assert rep["storage_fallback"] == "float32 private copy of the float16 data: general reason" and "half_storage" not in rep
    rep = run([lambda p: storage.notes_of(p).upcast(torch.float16, "its own reason")], 6)
    assert rep["storage_fallback"] == "float32 private copy of the float16 data: its own reason"
    assert run([], 6) == {"form": "f", "x_reads": 6}
