"""What tests/test_gpu_loo_coupled_order4_kernel.py stands on, proven without a GPU: the mirror of
cmtfpls_loo_xcov_coupled_tensor_f64's shape rules (loo_coupled_order4_ref.form) against the library's two host size functions and the
entry's own host checks, validate's LDS formula and decline texts against the same mirror, the conditions on the cases (the share of
pass counts on the threshold, the condition probes), and the host plumbing of the bootstrap (kfold._components hands Wk / Wl to the
backend, the option exists and is off by default)."""
import ctypes
import dataclasses
import inspect
import os
from types import SimpleNamespace

import numpy as np
import pytest

import loo_coupled_order4_ref as T

EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4
NAME = "cmtfpls_loo_xcov_coupled_tensor_f64"


@pytest.fixture(scope="module")
def lib():
    from cmtf_pls_amd import _lib
    return _lib.load()


def _blocks(dims, ptr, orders=None):
    from cmtf_pls_amd import _lib
    orders = orders or [len(d) + 1 for d in dims]
    return (_lib.LooCoupledBlock * len(dims))(*[_lib.LooCoupledBlock(ptr, ptr, o, *T.split(d)) for o, d in zip(orders, dims)])


def _pairs(dims, pairs=None):
    flat = [int(v) for p in (pairs or [T.pair(d) for d in dims]) for v in p]
    return (ctypes.c_int * len(flat))(*flat)


SHAPES = [(c[0], c[1], c[2], c[3]) for c in T.CASES] + [v[0] for v in T.DECLINES.values()] + [(256, ((64, 8, 8), (128,), (20, 30)), 8, 4)]


@pytest.mark.parametrize("shape", SHAPES, ids=[str(i) for i in range(len(SHAPES))])
def test_lds_and_workspace_mirror_equal_the_library(lib, shape):
    I, dims, M, R = shape
    form, why = T.form(I, dims, M, R)
    assert form is not None, why
    blocks, pairs = _blocks(dims, None), _pairs(dims)
    assert form["ws_bytes_per_fold"] == lib.cmtfpls_loo_xcov_coupled_tensor_fold_workspace_bytes(blocks, len(dims), pairs, I, M, R)
    assert form["lds_bytes"] == lib.cmtfpls_loo_xcov_coupled_tensor_lds_bytes(blocks, len(dims), pairs, I, M, R)


def test_sizes_are_the_hand_expanded_sums():
    # wA 5 + 1 + 4, wB 21 + 9 + 6, q qn tq my 4 x 3, G_y 9, xs 7 (the unfoldings' short sides are 5, 7, 3), ys 9, coef 9, Qs 9, Gn 9,
    # gn bb dd 9, then the CP's wK 7, wL 3, v 21, tmp 7, part 512
    form, _ = T.form(10, [(5, 7, 3), (9,), (4, 6)], 3, 3)
    assert form["lds_bytes"] == 8 * (10 + 36 + 12 + 9 + 7 + 9 + 9 + 9 + 9 + 9 + 7 + 3 + 21 + 7 + 512) == 5352 and not form["over_48k"]
    # sumP 105 + 9 + 24 = 138, Pmax = Ptmax = 105, nmax 7: (10 + 3) 138 + 315 + 315 + 98 + 10 (3 + 3 + 2) + 3 (10 + 36)
    assert form["ws_bytes_per_fold"] == 8 * (1794 + 315 + 315 + 98 + 80 + 138) == 21920
    # no matrix block: ys is empty
    assert T.form(10, [(4, 17, 2), (2, 3, 19)], 3, 3)[0]["kmax"] == 0
    # M = 128 next to one small tensor block: 147 368 bytes at 1024 threads, 512 doubles of partial sums fewer at 512
    assert T.form(10, [(5, 7, 3), (9,)], 128, 3)[0]["lds_bytes"] == 147368 - 8 * 512
    J = T.longest_row([(3, 4, 5)], 3, 2)
    assert J == T.J_STAR == 9292                                                    # 2 J + 616 doubles
    assert 8 * T.lds_doubles([(3, 4, 5), (J,)], 3, 2) == T.LDS_CAP < 8 * T.lds_doubles([(3, 4, 5), (J + 1,)], 3, 2)


def _probe(lib, I, dims, M, R, ws_bytes, max_iter=100, fold0=0, nfolds=1, orders=None, pairs=None, no_dims=False):
    """The entry's answer with stand-in pointers: every status below is decided before a data pointer is read or a kernel launched."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    rc = lib.cmtfpls_loo_xcov_coupled_tensor_f64(_blocks(dims, p, orders), len(dims), None if no_dims else _pairs(dims, pairs), p, p, I, M, R,
                                                 1e-8, max_iter, fold0, nfolds, p, None, p if ws_bytes else None, ws_bytes, None)
    msg = lib.cmtfpls_last_error().decode()
    lib.cmtfpls_clear_error()
    return rc, msg


@pytest.mark.parametrize("limit", sorted(T.DECLINES))
def test_host_checks_agree_with_the_mirror(lib, limit):
    inside, past = T.DECLINES[limit]
    assert T.form(*inside)[0] is not None and T.form(*past) == (None, limit)
    word = {"blocks": "8 blocks", "unfolding": "unfolding", "n": "min(A, B) > 256", "M": "M > 128", "R": "R > 64", "lds": "150 KB"}[limit]
    for ws_bytes in (0, 1 << 40):
        rc, msg = _probe(lib, *past, ws_bytes)
        assert rc == EUNSUPPORTED and word in msg and "loo_xcov_coupled_tensor" in msg, (rc, msg)
    assert _probe(lib, *inside, 0)[0] == EWORKSPACE                                 # the shape check comes before the workspace check
    per = T.form(*inside)[0]["ws_bytes_per_fold"]
    assert _probe(lib, *inside, per - 8)[0] == EWORKSPACE                           # one double short
    if limit == "lds":
        assert T.form(*inside)[0]["lds_bytes"] == T.LDS_CAP and 8 * T.lds_doubles(*past[1:]) == T.LDS_CAP + 8


def test_cells_decline(lib):
    assert T.form(*T.CELLS_PAST) == (None, "cells")
    rc, msg = _probe(lib, *T.CELLS_PAST, 1 << 40)
    assert rc == EUNSUPPORTED and "2^24" in msg
    I, dims, M, R = T.CELLS_PAST
    assert T.form(I, ((1, 256, 65536),) + dims[1:], M, R) == (None, "lds")           # at the cells limit: past the LDS
    assert lib.cmtfpls_loo_xcov_coupled_tensor_lds_bytes(_blocks(dims, None), len(dims), _pairs(dims), I, M, R) == 0


def test_bad_arguments_on_the_host(lib):
    dims = [(5, 7, 3), (8, 8), (5,)]
    assert _probe(lib, 6, dims, 2, 2, 0, fold0=3, nfolds=3)[0] == EWORKSPACE          # the description itself is fine
    assert _probe(lib, 1, dims, 2, 2, 0)[0] == EINVAL
    assert _probe(lib, 6, dims, 2, 2, 0, fold0=4, nfolds=3)[0] == EINVAL
    assert _probe(lib, 6, dims, 2, 2, 0, max_iter=0)[0] == EINVAL
    assert _probe(lib, 6, dims, 2, 2, 0, orders=[4, 2, 2])[0] == EINVAL               # order 2 with A != 1
    assert _probe(lib, 6, dims, 2, 2, 0, no_dims=True)[0] == EINVAL                   # dims == NULL
    assert _probe(lib, 6, dims, 2, 2, 0, pairs=[(7, 3), (0, -1), (0, 0)])[0] == EINVAL    # a negative dim
    assert _probe(lib, 6, dims, 2, 2, 0, pairs=[(-7, -3), (0, 0), (0, 0)])[0] == EINVAL
    assert _probe(lib, 6, dims, 2, 2, 0, pairs=[(7, 4), (0, 0), (0, 0)])[0] == EINVAL     # B1 B2 != B
    assert _probe(lib, 6, dims, 2, 2, 0, pairs=[(21, 0), (0, 0), (0, 0)])[0] == EINVAL    # order 4 with B2 = 0
    assert _probe(lib, 6, dims, 2, 2, 0, pairs=[(7, 3), (4, 2), (0, 0)])[0] == EINVAL     # order 3 with B2 > 0
    assert _probe(lib, 6, dims, 2, 2, 0, orders=[5, 3, 2])[0] == EINVAL                   # order > 4
    # EINVAL comes before EUNSUPPORTED: a bad description of nine blocks is a bad description
    nine = [(2, 2, 2)] + [(3,)] * 8
    assert _probe(lib, 6, nine, 2, 2, 0)[0] == EUNSUPPORTED and _probe(lib, 6, nine, 2, 2, 0, orders=[5] + [2] * 8)[0] == EINVAL
    # no block of order 4: cmtfpls_loo_xcov_coupled_f64's call, a bad argument here
    flat = [(8, 8), (5,)]
    assert _probe(lib, 6, flat, 2, 2, 1 << 40)[0] == EINVAL
    assert lib.cmtfpls_loo_xcov_coupled_tensor_lds_bytes(_blocks(flat, None), 2, _pairs(flat), 6, 2, 2) == 0
    assert lib.cmtfpls_loo_xcov_coupled_tensor_fold_workspace_bytes(_blocks(dims, None), 3, _pairs(dims), 1, 2, 2) == 0
    assert lib.cmtfpls_loo_xcov_coupled_tensor_fold_workspace_bytes(_blocks(dims, None), 3, None, 6, 2, 2) == 0
    assert lib.cmtfpls_loo_xcov_coupled_tensor_lds_bytes(_blocks(nine, None), 9, _pairs(nine), 6, 2, 2) == 0


def test_the_order23_entry_still_declines_order4(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    dims = [(5, 7, 3), (9,)]
    rc = lib.cmtfpls_loo_xcov_coupled_f64(_blocks(dims, p), 2, p, p, 6, 2, 2, 1e-8, 100, 0, 1, p, None, p, 1 << 40, None)
    msg = lib.cmtfpls_last_error().decode()
    lib.cmtfpls_clear_error()
    assert rc == EUNSUPPORTED and "order > 3" in msg


# ---- what validate asks the library, and its texts --------------------------------------------------------------------------------
def test_validate_lds_bytes_equals_the_mirror(lib):
    """The description validate._loo_coupled_why builds from its dims / tensor lists (null pointers, the order from the lists) gets the
    restatement's byte count from the library."""
    from cmtf_pls_amd import _lib
    from cmtf_pls_amd import validate as V
    for I, dims, M, R in SHAPES:
        ab, pairs = [T.split(d) for d in dims], [T.pair(d) for d in dims]
        blocks = V._size_blocks(_lib.LooCoupledBlock, ab, pairs)
        assert [b.order for b in blocks] == [len(d) + 1 for d in dims]
        assert lib.cmtfpls_loo_xcov_coupled_tensor_lds_bytes(blocks, len(dims), V._int_pairs(pairs), I, M, R) == T.form(I, dims, M, R)[0]["lds_bytes"]
    assert NAME in V.LOO_COUPLED_TENSOR_FORM


class _Shape:
    """A block's shape description: what the declines read of a block that is never built."""
    def __init__(self, *shape):
        self.shape, self.ndim = tuple(shape), len(shape)


def _model(R=2, comm=None, be=None, **opt):
    from cmtf_pls_amd.engine import EngineOptions
    be = be or SimpleNamespace(name="stub", loo_ctpls=None, loo_ctpls_tensor=None)
    eng = SimpleNamespace(be=be, opt=EngineOptions(small_fit=False, **opt))
    return SimpleNamespace(n_components=R, _comm=comm, _get_engine=lambda: eng)


def _xs(I, dims):
    return [_Shape(I, *d) for d in dims]


def test_every_text_of_the_decline(monkeypatch):
    from cmtf_pls_amd import validate as V
    monkeypatch.setattr(V, "has_missing", lambda X: bool(getattr(X, "nan", False)))
    Y = _Shape(4, 2)
    ok = _xs(4, [(5, 7, 3), (9,)])
    assert V._decline_loo_coupled_tensor(_model(), ok, Y) is None
    assert V._decline_loo_coupled_tensor(_model(be=SimpleNamespace(name="stub")), ok, Y) == \
        "the stub backend has no order-4 coupled leave-one-out kernel"
    assert V._decline_loo_coupled_tensor(_model(comm=object()), ok, Y) == "sharded model (comm)"
    assert V._decline_loo_coupled_tensor(_model(), _xs(4, [(5, 7, 3), (2, 2, 2, 2)]), Y) == f"block 1 of order 5 > 4 ({NAME})"
    I, dims, M, R = T.DECLINES["blocks"][1]
    assert V._decline_loo_coupled_tensor(_model(R), _xs(I, dims), _Shape(I, M)) == f"9 blocks > 8 ({NAME})"
    holed = _xs(4, [(5, 7, 3), (9,)])
    holed[1].nan = True
    assert V._decline_loo_coupled_tensor(_model(), holed, Y) == f"missing values in block 1 ({NAME} is the complete-data form)"
    nanY = _Shape(4, 2)
    nanY.nan = True
    assert V._decline_loo_coupled_tensor(_model(), ok, nanY) == "missing values in Y"
    I, dims, M, R = T.DECLINES["n"][1]
    assert V._decline_loo_coupled_tensor(_model(R), _xs(I, dims), _Shape(I, M)) == f"block 1: min(J, K) = 257 > 256 ({NAME})"
    I, dims, M, R = T.DECLINES["unfolding"][1]
    assert V._decline_loo_coupled_tensor(_model(R), _xs(I, dims), _Shape(I, M)) == \
        f"block 0: mode-0 unfolding: min(257, 272) = 257 > 256 ({NAME})"
    assert V._decline_loo_coupled_tensor(_model(), _xs(4, [(9,), (17, 257, 16)]), Y) == \
        f"block 1: mode-1 unfolding: min(257, 272) = 257 > 256 ({NAME})"
    I, dims, M, R = T.DECLINES["M"][1]
    assert V._decline_loo_coupled_tensor(_model(R), _xs(I, dims), _Shape(I, M)) == f"M = 129 > 128 responses ({NAME})"
    I, dims, M, R = T.DECLINES["R"][1]
    assert V._decline_loo_coupled_tensor(_model(R), _xs(I, dims), _Shape(I, M)) == f"R = 65 > 64 components ({NAME})"
    I, dims, M, R = T.CELLS_PAST
    assert V._decline_loo_coupled_tensor(_model(R), _xs(I, dims), _Shape(I, M)) == f"block 0: J K = {256 * 70000} > {1 << 24} ({NAME})"
    I, dims, M, R = T.DECLINES["lds"][1]
    assert V._decline_loo_coupled_tensor(_model(R), _xs(I, dims), _Shape(I, M)) == \
        f"the fold's vectors need {T.LDS_CAP + 8} bytes of LDS > {T.LDS_CAP} ({NAME})"
    for limit, (inside, _) in T.DECLINES.items():                                    # one step inside every limit: taken
        I, dims, M, R = inside
        assert V._decline_loo_coupled_tensor(_model(R), _xs(I, dims), _Shape(I, M)) is None, limit


def test_the_old_decline_keeps_its_text(monkeypatch):
    from cmtf_pls_amd import validate as V
    monkeypatch.setattr(V, "has_missing", lambda X: False)
    xs = _xs(4, [(5, 7, 3), (9,)])
    assert V._decline_loo_coupled(_model(), xs, _Shape(4, 2)) == "block 0 of order 4 > 3 (cmtfpls_loo_xcov_coupled_f64)"
    assert not V._wants_loo_coupled_tensor(_model(), xs) and not V._wants_loo_coupled_tensor(_model(tensor_folds_coupled=True), xs)
    assert V._wants_loo_coupled_tensor(_model(tensor_resamples_coupled=True), xs)
    assert not V._wants_loo_coupled_tensor(_model(tensor_resamples_coupled=True), _xs(4, [(5, 7), (9,)]))


# ---- the bootstrap's plumbing ----------------------------------------------------------------------------------------------------
def test_components_hands_the_mode_loadings_to_the_coupled_tensor_entry():
    from cmtf_pls_amd import kfold as K

    seen = {}

    class Stub:
        device = "cpu"

        def kfold_inner_coupled_tensor_workspace_bytes(self, st, tensor):
            return 0

        def kfold_inner_coupled_tensor(self, st, tensor, a, tol, max_iter, ws, mf=None, groups=1, Wk=None, Wl=None):
            seen[a] = (tensor, Wk, Wl)
            return None                                                              # decline: _components stops after this call

        def empty(self, *shape):
            import torch
            return torch.empty(*shape, dtype=torch.float64)

        def kfold_epilogue_weighted(self, *args):
            return True

    st = [SimpleNamespace(K=2, I=4, A=5, B=21), SimpleNamespace(K=2, I=4, A=1, B=9)]
    tensor = [(7, 3), (0, 0)]
    Wk, Wl = object(), object()
    why = K._components(Stub(), [None, None], st, {}, [{}, {}], 2, 1e-8, 100, True, weighted=True, tensor=tensor, tensor_out=(Wk, Wl))
    assert why == "shape outside cmtfpls_kfold_inner_coupled_tensor_f64" and seen[0][0] is tensor and seen[0][1] is Wk and seen[0][2] is Wl
    K._components(Stub(), [None, None], st, {}, [{}, {}], 2, 1e-8, 100, True, weighted=True, tensor=tensor)
    assert seen[0][1] is None and seen[0][2] is None                                 # None behaves as before
    assert "tensor_out" in inspect.signature(K._components).parameters


def test_mode_slices_follow_the_entrys_layout():
    from cmtf_pls_amd.bootstrap import _mode_slices
    n, R, tensor = 3, 2, [(0, 0), (4, 5), (0, 0), (2, 6)]
    Wk, Wl = np.arange(n * R * 6, dtype=float), np.arange(n * R * 11, dtype=float)
    ks, ls = _mode_slices(Wk, Wl, tensor, n, R)
    assert ks[0] is None and ls[2] is None and ks[1].shape == (3, 2, 4) and ls[1].shape == (3, 2, 5) and ks[3].shape == (3, 2, 2)
    assert ks[1][0, 0, 0] == 0 and ks[3][0, 0, 0] == n * R * 4 and ls[3][0, 0, 0] == n * R * 5 and ls[3][2, 1, 5] == Wl[-1]


def test_the_option_exists_and_is_off_by_default():
    from cmtf_pls_amd import options
    from cmtf_pls_amd.engine import EngineOptions
    fields = {f.name: f for f in dataclasses.fields(EngineOptions)}
    assert fields["tensor_resamples_coupled"].default is False and fields["tensor_resamples_coupled"].type in (bool, "bool")
    assert EngineOptions().tensor_resamples_coupled is False and EngineOptions().but(tensor_resamples_coupled=True).tensor_resamples_coupled
    src = open(os.path.splitext(options.__file__)[0] + ".py").read().split("\n")
    at = next(i for i, line in enumerate(src) if line.strip().startswith("tensor_resamples_coupled: bool"))
    comment = " ".join(line.strip() for line in src[at - 6:at])
    assert src[at - 1].strip().startswith("#") and "cmtfpls_loo_xcov_coupled_tensor_f64" in comment and "DESIGN 8t" in comment


# ---- the conditions on the GPU suite's inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", T.CASES, ids=[T.case_id(c) for c in T.CASES])
def test_each_case_is_on_the_branch_its_table_claims(case):
    form, why = T.form(case[0], case[1], case[2], case[3])
    assert form is not None, why
    assert {k: form[k] for k in case[8]} == case[8]


def test_case_table_covers_the_limits():
    forms = [T.form(c[0], c[1], c[2], c[3])[0] for c in T.CASES]
    assert max(f["lds_bytes"] for f in forms) == T.LDS_CAP and max(f["nmax"] for f in forms) == T.MAX_N
    assert max(c[2] for c in T.CASES) == T.MAX_M and min(c[2] for c in T.CASES) == 1 and max(f["blocks"] for f in forms) == T.MAX_BLOCKS
    assert any(f["kmax"] == 0 for f in forms) and any(f["tensors"] > 1 for f in forms) and any(True in f["mode0_transposed"] for f in forms)
    assert any(1 in t for c in T.CASES for t in c[1] if len(t) == 3)                 # B2 = 1 with order 4 is still a tensor
    assert all(c[0] <= 10 for c in T.CASES)
    f0, n = T.RANGE
    assert 0 < f0 and f0 + n < T.RANGE_CASE[0]


def test_pass_counts_on_the_threshold_stay_within_the_cap():
    """A condition on the inputs: of the (fold, component) pairs the GPU suite compares pass counts on, at most 10% may be decisions
    that sat on the threshold in the reference itself (and are therefore not compared)."""
    excluded = total = 0
    for case in T.CASES:
        ref = T.reference(case, T.TOL, T.MAX_ITER)
        near = T.on_threshold(ref, T.TOL)
        assert (ref["n_iter"] >= 2).all()
        excluded, total = excluded + int(near.sum()), total + near.size
        capped = T.reference(case, T.CAP_TOL, T.CAP_ITER)
        assert (capped["n_iter"] == T.CAP_ITER).all() and np.isfinite(capped["pred"]).all()
    print(f"{excluded} of {total} pairs on the threshold")
    assert excluded <= T.EXCLUDED_CAP * total, (excluded, total)


@pytest.mark.parametrize("case", T.CASES, ids=[T.case_id(c) for c in T.CASES])
def test_cases_are_well_conditioned(case):
    """10 x condition_probe beyond 1e-4 would mean the case tests nothing: its seed or noise has to change then, not the factor."""
    for tol, max_iter in ((T.TOL, T.MAX_ITER), (T.CAP_TOL, T.CAP_ITER)):
        probe = T.case_probe(T.case_id(case), tol, max_iter)
        print(f"{T.case_id(case)} tol={tol:g}: condition_probe {probe:.2e}, bound {T.case_bound(case, tol, max_iter):.2e}")
        assert 10.0 * probe <= 1e-4
        assert T.case_bound(case, tol, max_iter) == max(1e-8, 10.0 * probe)
