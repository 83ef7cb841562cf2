#!/usr/bin/env python3
"""What the host side of the fold entries answers, on a fixed table of calls: (status, cmtfpls_last_error()) of every call and the
value of every workspace-size and LDS-size export, as JSON.  No GPU: every call of the table is refused by a check of the entry's host code,
before a data pointer is read or a kernel launched (the pointers are stand-ins); the tool stops at the first call that is not.
The entries: the four of csrc/cv_masked.hip, the two of csrc/loo_xcov.hip and, of csrc/kfold.hip, the six inner entries, the four
epilogue entries and the wide and weighted cross-covariance builds.  The table reaches every `return CMTFPLS_E*` of those entries
and of the checks and launch helpers behind them; for every two neighbouring checks it has a call that fails both (the first
one's text must come back); every workspace check is met with a NULL workspace and with one double short of the requirement.
The library is the one CMTFPLS_LIB names (else the in-tree build).  tests/test_fold_entries_cpu.py holds the in-tree build to
tests/golden/fold_entry_statuses.json, recorded from the build before the entries were put on shared helpers.
Usage: python tools/fold_entry_probe.py OUT.json"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmtf_pls_amd import _lib  # noqa: E402

# the entries and exports of this table start with one of these; OUT_OF_SCOPE: those that do but live in files with one entry or
# one checked launch of their own (cv_masked_coupled.hip, loo_xcov_coupled.hip), and the _bf16 / _f16 forms of the wide and weighted
# builds: they did not exist in the build the table was recorded from, and they are run_kfold_wide / run_kfold_weighted -- the host
# checks this table probes through the _f32 / _f64 entries -- instantiated for another storage type (their statuses are held to the
# _f32 entry's on the device, tests/test_gpu_half_fold_kernels.py)
PREFIXES = ("cmtfpls_cv_masked_", "cmtfpls_loo_xcov_", "cmtfpls_kfold_inner", "cmtfpls_kfold_epilogue", "cmtfpls_kfold_wide_xcov",
            "cmtfpls_kfold_weighted_xcov")
OUT_OF_SCOPE = ("cmtfpls_cv_masked_coupled_", "cmtfpls_loo_xcov_coupled_", "cmtfpls_kfold_wide_xcov_bf16", "cmtfpls_kfold_wide_xcov_f16",
                "cmtfpls_kfold_weighted_xcov_bf16", "cmtfpls_kfold_weighted_xcov_f16")

_BUF = ctypes.create_string_buffer(64)
P = ctypes.addressof(_BUF)                 # the stand-in for every pointer that a check only compares with NULL
BIG = 1 << 24                              # the cell limit of the cross-covariance forms


def state(I=40, A=6, B=5, M=3, K=4, R=3, **fields):
    """A cmtfpls_kfold_state with every buffer the stand-in; fields: name=other pointer (0: NULL)."""
    return _lib.KfoldState(I, A, B, M, K, R, *[fields.get(f, P) for f, _ in _lib.KfoldState._fields_[6:]])


def views(*sts):
    return (_lib.KfoldState * len(sts))(*sts)


def pairs(*ds):
    flat = [v for d in ds for v in d]
    return (ctypes.c_int * len(flat))(*flat)


def table(lib):
    """[(label, symbol, args)]; ws arguments are (pointer, bytes) made by null() / short()."""
    rows = []

    def null():
        return (None, 0)

    def short(need):
        assert need >= 8, need                 # (a requirement of 0 would wrap to "enough")
        return (P, need - 8)

    def add(label, sym, *args):
        rows.append((f"{sym[8:]}: {label}", sym, args))

    # ---- csrc/cv_masked.hip: EINVAL (arguments), EUNSUPPORTED (form; K > I in the fold entries), EINVAL (range), EWORKSPACE
    def cv(sym, tensor, models, label, ws=None, I=20, A=6, B=(5,), M=3, R=3, n=4, first=0, count=2, max_iter=100, X=P, rows_=P, sums=P,
           Ypred=P, status=P):
        lead = (X, P, rows_, P, n) if models else (X, P, rows_, n, sums, sums, P)
        facs = ((P,) * (5 if tensor else 4)) if models else ()
        add(label, sym, *lead, I, A, *B, M, R, 1e-8, max_iter, first, count, Ypred, *facs, P, status, P, *(ws or null()), None)

    for sym, per_sym, tensor, models in (
            ("cmtfpls_cv_masked_f64", "cmtfpls_cv_masked_fold_workspace_bytes", False, False),
            ("cmtfpls_cv_masked_models_f64", "cmtfpls_cv_masked_model_workspace_bytes", False, True),
            ("cmtfpls_cv_masked_tensor_f64", "cmtfpls_cv_masked_tensor_fold_workspace_bytes", True, False),
            ("cmtfpls_cv_masked_tensor_models_f64", "cmtfpls_cv_masked_tensor_model_workspace_bytes", True, True)):
        c = lambda label, **kw: cv(sym, tensor, models, label, **kw)
        B = (4, 2) if tensor else (5,)
        per = getattr(lib, per_sym)(20, 6, *B, 3, 3)
        c("workspace NULL", B=B)
        c("workspace one double short", B=B, ws=short(2 * per))
        c("workspace for one item of two", B=B, ws=(P, per))
        c("I = 1", B=B, I=1)
        c("X NULL", B=B, X=None)
        c("rows NULL", B=B, rows_=None)
        c("column sums NULL", B=B, sums=None)                   # (the model entries take none)
        c("Ypred NULL", B=B, Ypred=None)
        c("status NULL", B=B, status=None)
        c("max_iter = 0", B=B, max_iter=0)
        c("count = 0", B=B, count=0)
        c("first = -1", B=B, first=-1)
        c("B = 0", B=(0, 2) if tensor else (0,))
        c("arguments and form", B=B, I=1, R=17)
        c("short side 65", A=65, B=(65, 2) if tensor else (65,))
        c("M = 65", B=B, M=65)
        c("R = 17", B=B, R=17)
        c("LDS", B=B, I=5000, n=5)
        c("more items than rows", B=B, I=3, n=4)                 # (declined by the fold entries only)
        c("2^31 cells", A=1 << 11, B=(1 << 10, 1 << 10) if tensor else (1 << 20,))
        c("form and range", B=B, R=17, first=3, count=2)
        c("range", B=B, first=3, count=2, ws=(P, 1 << 40))
        c("range and workspace", B=B, first=3, count=2)

    # ---- csrc/loo_xcov.hip: EINVAL, EUNSUPPORTED (the matrix entry: one text; the tensor entry: cells, unfolding, M / R, LDS), EWORKSPACE
    def lx(tensor, label, ws=None, I=20, A=6, B=None, M=3, R=3, first=0, count=2, max_iter=100, X=P, Ypred=P):
        sym = "cmtfpls_loo_xcov_tensor_f64" if tensor else "cmtfpls_loo_xcov_f64"
        B = B or ((4, 2) if tensor else (5,))
        add(label, sym, X, P, P, P, I, A, *B, M, R, 1e-8, max_iter, first, count, Ypred, P, *(ws or null()), None)

    for tensor in (False, True):
        c = lambda label, **kw: lx(tensor, label, **kw)
        per = (lib.cmtfpls_loo_xcov_tensor_fold_workspace_bytes(20, 6, 4, 2, 3, 3) if tensor
               else lib.cmtfpls_loo_xcov_fold_workspace_bytes(20, 6, 5, 3, 3))
        c("workspace NULL")
        c("workspace one double short", ws=short(2 * per))
        c("I = 1", I=1)
        c("X NULL", X=None)
        c("Ypred NULL", Ypred=None)
        c("max_iter = 0", max_iter=0)
        c("folds past I", first=19, count=2, ws=(P, 1 << 40))
        c("arguments and form", I=1, M=129)
        c("M = 129", M=129)
        c("R = 65", R=65)
        c("form and workspace", R=65)
    lx(False, "short side 257", A=257, B=(257,))
    lx(False, "LDS", A=256, B=(2000,), M=128)
    lx(False, "2^24 cells", A=1, B=(BIG + 1,))
    lx(True, "B2 = 0", B=(4, 0))
    lx(True, "2^24 cells", A=256, B=(256, 257))
    lx(True, "cells and unfolding", A=300, B=(300, 300))
    lx(True, "unfolding", A=8, B=(257, 33))
    lx(True, "unfolding and M", A=8, B=(257, 33), M=129)
    lx(True, "M and LDS", A=4, B=(4, 4000), M=129)
    lx(True, "LDS", A=4, B=(4, 4000))
    lx(True, "LDS and workspace", A=4, B=(4, 4000), ws=null())

    # ---- csrc/kfold.hip, the inner entries
    sym = "cmtfpls_kfold_inner_f64"
    inner = lambda label, st, a=0, max_iter=100, ws=None: add(label, sym, ctypes.byref(st) if st is not None else None, a, 1e-8, max_iter,
                                                               *(ws or null()), None)
    inner("workspace NULL", state())
    inner("workspace one double short", state(), ws=short(lib.cmtfpls_kfold_inner_workspace_bytes(6, 5, 4)))
    inner("state NULL", None)
    inner("a buffer NULL", state(part=0))
    inner("a = -1", state(), a=-1)
    inner("a = R", state(), a=3)
    inner("max_iter = 0", state(), max_iter=0)
    inner("arguments and form", state(K=33), a=-1)
    for label, kw in (("K = 1", dict(K=1)), ("K = 33", dict(K=33)), ("M = 65", dict(M=65)), ("R = 65", dict(R=65)), ("M = 0", dict(M=0)),
                      ("short side 257", dict(A=257, B=257)), ("I < K", dict(I=3)), ("2^24 cells", dict(A=1, B=BIG + 1)),
                      ("LDS", dict(A=1, B=10000))):
        inner(label, state(**kw))
    inner("form and workspace", state(M=65), ws=null())

    mf = P
    sym_g = "cmtfpls_kfold_inner_grouped_f64"
    grouped = lambda label, st, model_fold=mf, groups=2, a=0, max_iter=100, ws=None: add(
        label, sym_g, ctypes.byref(st) if st is not None else None, model_fold, groups, a, 1e-8, max_iter, *(ws or null()), None)
    grouped("workspace NULL", state(K=6))
    grouped("workspace NULL, fewer rows than models", state(I=4, K=6))
    grouped("workspace one double short", state(K=6), ws=short(lib.cmtfpls_kfold_inner_workspace_bytes(6, 5, 6)))
    grouped("state NULL", None)
    grouped("model_fold NULL", state(K=6), model_fold=None)
    grouped("groups = 0", state(K=6), groups=0)
    grouped("K % groups", state(K=6), groups=4)
    grouped("a = R", state(K=6), a=3)
    grouped("arguments and form", state(K=6, M=65), groups=0)
    grouped("one fold", state(K=4), groups=4)
    grouped("fewer rows than folds", state(I=2, K=6))
    grouped("M = 65", state(K=6, M=65))
    grouped("form and max_iter", state(K=6, M=65), max_iter=0)
    grouped("max_iter = 0", state(K=6), max_iter=0, ws=(P, 1 << 40))
    grouped("max_iter and workspace", state(K=6), max_iter=0)

    sym_t = "cmtfpls_kfold_inner_tensor_f64"
    tensor = lambda label, st, B1=4, B2=2, model_fold=None, groups=1, a=0, max_iter=100, ws=None: add(
        label, sym_t, ctypes.byref(st) if st is not None else None, model_fold, groups, B1, B2, a, 1e-8, max_iter, P, P, *(ws or null()), None)
    t8 = lambda **kw: state(B=8, **kw)
    long_row = dict(A=8, B=257 * 33), dict(B1=257, B2=33)      # min(A, B) = 8, but the unfolding 257 x (8 * 33) has a short side of 257
    lds_row = dict(A=2, B=9000, M=1), dict(B1=2, B2=4500)       # inside the order-3 LDS form, past the tensor form's
    tensor("workspace NULL", t8())
    tensor("workspace NULL, grouped", t8(K=6), model_fold=mf, groups=2)
    tensor("workspace one double short", t8(), ws=short(lib.cmtfpls_kfold_inner_tensor_workspace_bytes(6, 4, 2, 4)))
    tensor("state NULL", None)
    tensor("B1 * B2 != B", t8(), B1=3)
    tensor("B2 = 0", t8(), B2=0)
    tensor("groups without model_fold", t8(), groups=2)
    tensor("groups = 0", t8(), model_fold=mf, groups=0)
    tensor("max_iter = 0", t8(), max_iter=0)
    tensor("a = R", t8(), a=3)
    tensor("arguments and unfolding", state(**long_row[0]), **long_row[1], a=3)
    tensor("unfolding", state(**long_row[0]), **long_row[1])
    tensor("unfolding and form", state(M=65, **long_row[0]), **long_row[1])
    tensor("unfolding and grouped arguments", state(K=6, **long_row[0]), **long_row[1], model_fold=mf, groups=4)
    tensor("M = 65", t8(M=65))
    tensor("grouped: K % groups", t8(K=6), model_fold=mf, groups=4)
    tensor("grouped: one fold", t8(K=4), model_fold=mf, groups=4)
    tensor("grouped: M = 65", t8(K=6, M=65), model_fold=mf, groups=2)
    tensor("form and LDS", state(A=2, B=9000, M=1, K=33), **lds_row[1])
    tensor("LDS", state(**lds_row[0]), **lds_row[1])
    tensor("LDS, grouped", state(K=6, **lds_row[0]), **lds_row[1], model_fold=mf, groups=2)
    tensor("LDS and workspace", state(**lds_row[0]), **lds_row[1], ws=null())

    two = lambda **kw: (state(**kw), state(A=1, B=9, **kw))
    wide = lambda **kw: (state(A=9000, B=1, M=1, **kw), state(A=1, B=9000, M=1, **kw))   # each block inside the LDS form, the two together not
    sym_c = "cmtfpls_kfold_inner_coupled_f64"
    coupled = lambda label, sts, nb=None, a=0, max_iter=100, ws=None: add(
        label, sym_c, views(*sts) if sts is not None else None, len(sts) if nb is None else nb, a, 1e-8, max_iter, *(ws or null()), None)
    coupled("workspace NULL", two())
    coupled("workspace one double short", two(), ws=short(lib.cmtfpls_kfold_inner_coupled_workspace_bytes(views(*two()), 2)))
    coupled("views NULL", None, nb=2)
    coupled("nb = 0", two(), nb=0)
    coupled("nb = 9", two() + tuple(state() for _ in range(7)), nb=9)
    coupled("a buffer NULL in block 1", (state(), state(A=1, B=9, Rm=0)))
    coupled("M differs in block 1", (state(), state(A=1, B=9, M=2)))
    coupled("a shared buffer differs in block 1", (state(), state(A=1, B=9, vec=P + 8)))
    coupled("block 0: arguments and form", (state(S=0, M=65), state(A=1, B=9, M=65)))
    coupled("block 0 outside the form, block 1 differs", (state(M=65), state(A=1, B=9, M=2)))
    coupled("block 1 outside the form", (state(), state(A=1, B=BIG + 1)))
    coupled("views and a", (state(M=65), state(A=1, B=9, M=65)), a=3)
    coupled("a = R", two(), a=3)
    coupled("max_iter = 0", two(), max_iter=0)
    coupled("a and LDS", wide(), a=-1)
    coupled("LDS", wide(), ws=(P, 1 << 40))
    coupled("LDS and workspace", wide())

    sym_cg = "cmtfpls_kfold_inner_coupled_grouped_f64"
    cgrouped = lambda label, sts, nb=None, model_fold=mf, groups=2, a=0, max_iter=100, ws=None: add(
        label, sym_cg, views(*sts) if sts is not None else None, len(sts) if nb is None else nb, model_fold, groups, a, 1e-8, max_iter,
        *(ws or null()), None)
    cgrouped("workspace NULL", two(K=6))
    cgrouped("workspace NULL, fewer rows than models", two(I=4, K=6))
    cgrouped("workspace one double short", two(K=6), ws=short(lib.cmtfpls_kfold_inner_coupled_workspace_bytes(views(*two(K=6)), 2)))
    cgrouped("views NULL", None, nb=2)
    cgrouped("nb = 9", two(K=6), nb=9)
    cgrouped("model_fold NULL", two(K=6), model_fold=None)
    cgrouped("groups = 0", two(K=6), groups=0)
    cgrouped("groups = 0 and a = R", two(K=6), groups=0, a=3)
    cgrouped("K % groups", two(K=6), groups=4)
    cgrouped("a = R", two(K=6), a=3)
    cgrouped("max_iter = 0", two(K=6), max_iter=0)
    cgrouped("max_iter and views", (state(K=6), state(A=1, B=9, K=6, M=2)), max_iter=0)
    cgrouped("M differs in block 1", (state(K=6), state(A=1, B=9, K=6, M=2)))
    cgrouped("one fold", two(K=4), groups=4)
    cgrouped("fewer rows than folds", two(I=2, K=6))
    cgrouped("M = 65", two(K=6, M=65))
    cgrouped("views and LDS", wide(K=6, R=65))
    cgrouped("LDS", wide(K=6), ws=(P, 1 << 40))
    cgrouped("LDS and workspace", wide(K=6))

    sym_ct = "cmtfpls_kfold_inner_coupled_tensor_f64"
    ctensor = lambda label, sts, dims, nb=None, model_fold=None, groups=1, a=0, max_iter=100, ws=None: add(
        label, sym_ct, views(*sts) if sts is not None else None, len(sts) if nb is None else nb, pairs(*dims) if dims is not None else None,
        model_fold, groups, a, 1e-8, max_iter, P, P, *(ws or null()), None)
    tt = lambda **kw: (state(B=8, **kw), state(A=1, B=9, **kw))
    d2 = ((4, 2), (0, 0))
    need = lib.cmtfpls_kfold_inner_coupled_tensor_workspace_bytes(views(*tt()), 2, pairs(*d2))
    ctensor("workspace NULL", tt(), d2)
    ctensor("workspace NULL, grouped", tt(K=6), d2, model_fold=mf, groups=2)
    ctensor("workspace one double short", tt(), d2, ws=short(need))
    ctensor("views NULL", None, d2, nb=2)
    ctensor("nb = 9", tt(), d2, nb=9)
    ctensor("dims NULL", tt(), None)
    ctensor("B1 * B2 != B", tt(), ((3, 2), (0, 0)))
    ctensor("B1 = 0 alone", tt(), ((0, 2), (0, 0)))
    ctensor("groups = 0", tt(), d2, model_fold=mf, groups=0)
    ctensor("groups without model_fold", tt(), d2, groups=2)
    ctensor("dims and a", tt(), ((3, 2), (0, 0)), a=3)
    ctensor("K % groups", tt(K=6), d2, model_fold=mf, groups=4)
    ctensor("a = R", tt(), d2, a=3)
    ctensor("max_iter = 0", tt(), d2, max_iter=0)
    ctensor("max_iter and views", (state(B=8), state(A=1, B=9, M=2)), d2, max_iter=0)
    ctensor("M differs in block 1", (state(B=8), state(A=1, B=9, M=2)), d2)
    ctensor("M = 65", tt(M=65), d2)
    ctensor("grouped: one fold", tt(K=4), d2, model_fold=mf, groups=4)
    ctensor("form and unfolding", (state(M=65, **long_row[0]), state(A=1, B=9, M=65)), ((257, 33), (0, 0)))
    ctensor("unfolding", (state(**long_row[0]), state(A=1, B=9)), ((257, 33), (0, 0)))
    ctensor("unfolding and LDS", (state(M=1, **long_row[0]), state(**lds_row[0])), ((257, 33), (2, 4500)))
    ctensor("LDS", (state(**lds_row[0]),), ((2, 4500),), ws=(P, 1 << 40))
    ctensor("LDS and workspace", (state(**lds_row[0]),), ((2, 4500),))

    # ---- csrc/kfold.hip, the epilogue entries (no workspace: arguments, then the form)
    def epilogue(kind, label, st, stage=0, a=0, src=P, extra=()):
        add(label, f"cmtfpls_kfold_epilogue{kind}_f64", ctypes.byref(st) if st is not None else None, *extra, stage, a, src, None)

    for kind, extra, K in (("", (), 4), ("_weighted", (), 4), ("_splits", (2,), 6), ("_grouped", (mf, 2), 6)):
        e = lambda label, st, **kw: epilogue(kind, label, st, extra=kw.pop("extra", extra), **kw)
        e("state NULL", None)
        e("a buffer NULL", state(K=K, tm=0))
        e("stage = -1", state(K=K), stage=-1)
        e("stage = 3", state(K=K), stage=3)
        e("a = -1", state(K=K), a=-1)
        e("a = R", state(K=K), a=3)
        e("stage 1 without its input", state(K=K), stage=1, src=None)
        e("stage 2 without its input", state(K=K), stage=2, src=None)
        e("arguments and form", state(K=K, M=65), a=3)
        e("stage and form", state(K=K, M=65), stage=3)
        e("M = 65", state(K=K, M=65))
        e("K = 33", state(K=33 if not extra else 36))
        if kind != "_grouped":                                   # (grouped models may outnumber the rows)
            e("I < K", state(I=3, K=K))
    epilogue("_splits", "splits = 0", state(K=6), extra=(0,))
    epilogue("_splits", "K % splits", state(K=6), extra=(4,))
    epilogue("_splits", "splits and form", state(K=6, M=65), extra=(4,))
    epilogue("_splits", "one fold per split", state(K=4), extra=(4,))
    epilogue("_grouped", "model_fold NULL", state(K=6), extra=(None, 2))
    epilogue("_grouped", "groups = 0", state(K=6), extra=(mf, 0))
    epilogue("_grouped", "K % groups", state(K=6), extra=(mf, 4))
    epilogue("_grouped", "one fold", state(K=4), extra=(mf, 4))
    epilogue("_grouped", "one fold and stage", state(K=4), extra=(mf, 4), stage=3)
    epilogue("_grouped", "fewer rows than folds", state(I=2, K=6), extra=(mf, 2))

    # ---- csrc/kfold.hip, the wide and the weighted builds (float and double X)
    for suf in ("f64", "f32"):
        sym_w = "cmtfpls_kfold_wide_xcov_" + suf
        w = lambda label, ws=None, X=P, I=4096, A=6, B=5, W=40, K=4, S=P: add(label, sym_w, X, I, A, B, P, W, P, P, K, P, S, P, P,
                                                                             *(ws or null()), None)
        w("workspace NULL")
        w("workspace one double short", ws=short(lib.cmtfpls_kfold_wide_xcov_workspace_bytes(4096, 30, 40, 4)))
        w("X NULL", X=None)
        w("S NULL", S=None)
        w("W = 0", W=0)
        w("arguments and form", W=0, K=33)
        for label, kw in (("K = 1", dict(K=1)), ("K = 33", dict(K=33)), ("W = 1025", dict(W=1025)), ("I < K", dict(I=3)),
                          ("I > 2^30", dict(I=(1 << 30) + 1)), ("2^24 cells", dict(A=4097, B=4096))):
            w(label, **kw)
        w("form and workspace", K=33, ws=null())
        sym_b = "cmtfpls_kfold_weighted_xcov_" + suf
        b = lambda label, ws=None, X=P, I=4096, A=6, B=5, n=8, M=3, S=P: add(label, sym_b, X, I, A, B, P, n, M, S, P, P, *(ws or null()), None)
        b("workspace NULL")
        b("workspace one double short", ws=short(lib.cmtfpls_kfold_weighted_xcov_workspace_bytes(4096, 30, 8, 3)))
        b("X NULL", X=None)
        b("S NULL", S=None)
        b("n = 0", n=0)
        b("arguments and form", n=0, M=65)
        for label, kw in (("n = 33", dict(n=33)), ("M = 65", dict(M=65)), ("n (M + 1) = 1056", dict(n=32, M=32)),
                          ("I > 2^30", dict(I=(1 << 30) + 1)), ("2^24 cells", dict(A=4097, B=4096))):
            b(label, **kw)
        b("form and workspace", n=33, ws=null())
    return rows


def sizes(lib, lds=False):
    """[(export, printable arguments, value)] on about ten shapes each, some of which the export answers with 0: of the workspace-size
    exports, or (lds) of the LDS-size exports."""
    out = []

    def plain(sym, shapes):
        for s in shapes:
            out.append((sym, list(s), getattr(lib, sym)(*s)))

    five = [(20, 6, 5, 3, 3), (2, 1, 9, 1, 1), (21, 20, 16, 3, 3), (24, 4, 70, 64, 16), (512, 64, 64, 16, 10), (300, 128, 256, 128, 64),
            (100000, 256, 256, 8, 4), (1, 6, 5, 3, 3), (20, 0, 5, 3, 3), (20, 6, -1, 3, 3), (20, 6, 5, 0, 3), (20, 6, 5, 3, 0)]
    six = [(20, 6, 4, 2, 3, 3), (2, 1, 1, 9, 1, 1), (18, 3, 4, 2, 3, 3), (19, 6, 1, 5, 3, 3), (20, 2, 9, 3, 3, 3), (64, 16, 16, 16, 64, 16),
           (300, 64, 64, 64, 128, 64), (4096, 8, 257, 33, 8, 4), (1, 6, 4, 2, 3, 3), (20, 0, 4, 2, 3, 3), (20, 6, 0, 2, 3, 3),
           (20, 6, 4, -2, 3, 3), (20, 6, 4, 2, 0, 3), (20, 6, 4, 2, 3, 0)]
    for sym in ("cmtfpls_cv_masked_fold_workspace_bytes", "cmtfpls_cv_masked_model_workspace_bytes", "cmtfpls_loo_xcov_fold_workspace_bytes"):
        plain(sym, five)
    for sym in ("cmtfpls_cv_masked_tensor_fold_workspace_bytes", "cmtfpls_cv_masked_tensor_model_workspace_bytes",
                "cmtfpls_loo_xcov_tensor_fold_workspace_bytes"):
        plain(sym, six)
    plain("cmtfpls_kfold_inner_workspace_bytes", [(6, 5, 4), (1, 9, 2), (128, 128, 5), (256, 4096, 32), (300, 300, 32), (1, 1, 1), (4096, 4096, 8),
                                                  (0, 5, 4), (6, 0, 4), (6, 5, 0), (-1, 5, 4)])
    tensor4 = [(6, 4, 2, 4), (3, 4, 2, 2), (6, 1, 5, 5), (2, 9, 3, 32), (64, 64, 64, 8), (8, 257, 33, 4), (256, 256, 256, 32),
               (256, 256, 257, 4), (0, 4, 2, 4), (6, 0, 2, 4), (6, 4, 0, 4), (6, 4, 2, 0)]
    plain("cmtfpls_kfold_inner_tensor_workspace_bytes", tensor4)
    four = [(4096, 30, 40, 4), (40, 30, 3, 4), (65536, 16384, 16, 5), (65536, 16384, 1024, 32), (1 << 20, 64, 8, 2), (100, 1, 1, 1),
            (8192, 1 << 24, 16, 5), (0, 30, 40, 4), (4096, 0, 40, 4), (4096, 30, 0, 4), (4096, 30, 40, 0)]
    plain("cmtfpls_kfold_wide_xcov_workspace_bytes", four)
    plain("cmtfpls_kfold_weighted_xcov_workspace_bytes", [(4096, 30, 8, 3), (40, 30, 4, 3), (65536, 16384, 32, 16), (65536, 16384, 15, 64),
                                                          (1 << 20, 64, 2, 1), (100, 1, 1, 1), (8192, 1 << 24, 5, 16), (0, 30, 8, 3),
                                                          (4096, 0, 8, 3), (4096, 30, 0, 3), (4096, 30, 8, 0)])
    blocks = [[(40, 6, 5, 3, 4, 3)], [(40, 6, 5, 3, 4, 3), (40, 1, 9, 3, 4, 3)], [(40, 128, 128, 16, 5, 10), (40, 1, 256, 16, 5, 10)],
              [(40, 9000, 1, 1, 4, 3), (40, 1, 9000, 1, 4, 3)], [(40, 6, 5, 3, 32, 3)] * 8, [(40, 6, 5, 3, 4, 3)] * 9, [(40, 6, 5, 3, 0, 3)],
              [(40, 6, 5, 3, 4, 3), (40, 0, 9, 3, 4, 3)], [(40, 6, 0, 3, 4, 3)], []]
    for bl in blocks:
        arr = views(*[state(*b) for b in bl]) if bl else None
        out.append(("cmtfpls_kfold_inner_coupled_workspace_bytes", [list(b) for b in bl], lib.cmtfpls_kfold_inner_coupled_workspace_bytes(arr, len(bl))))
    tblocks = [([(40, 6, 8, 3, 4, 3)], [(4, 2)]), ([(40, 6, 8, 3, 4, 3), (40, 1, 9, 3, 4, 3)], [(4, 2), (0, 0)]),
               ([(40, 6, 8, 3, 4, 3), (40, 5, 21, 3, 4, 3)], [(4, 2), (7, 3)]), ([(40, 6, 5, 3, 4, 3)], [(0, 0)]),
               ([(40, 8, 8481, 3, 4, 3)], [(257, 33)]), ([(40, 64, 4096, 16, 32, 10), (40, 256, 256, 16, 32, 10)], [(64, 64), (0, 0)]),
               ([(40, 6, 8, 3, 4, 3)], [(3, 2)]), ([(40, 6, 8, 3, 4, 3)], [(0, 2)]), ([(40, 6, 8, 3, 0, 3)], [(4, 2)]),
               ([(40, 6, 8, 3, 4, 0)], [(4, 2)]), ([(40, 256, 65792, 3, 4, 3)], [(256, 257)]), ([(40, 6, 8, 3, 4, 3)] * 9, [(4, 2)] * 9)]
    for bl, ds in tblocks:
        out.append(("cmtfpls_kfold_inner_coupled_tensor_workspace_bytes", [[list(b) for b in bl], [list(d) for d in ds]],
                    lib.cmtfpls_kfold_inner_coupled_tensor_workspace_bytes(views(*[state(*b) for b in bl]), len(bl), pairs(*ds))))
    if not lds:
        return out
    # the LDS-size exports, a list of their own (the record of the workspace sizes is older): the same shapes, the last of tensor4's
    # four read as M; a shape past a limit of its entry keeps its byte count
    out = []
    plain("cmtfpls_cv_masked_tensor_lds_bytes", six)
    plain("cmtfpls_loo_xcov_tensor_lds_bytes", [s[1:] for s in six])
    plain("cmtfpls_kfold_inner_tensor_lds_bytes", tensor4)
    for bl, ds in tblocks:
        out.append(("cmtfpls_kfold_inner_coupled_tensor_lds_bytes", [[list(b) for b in bl], [list(d) for d in ds]],
                    lib.cmtfpls_kfold_inner_coupled_tensor_lds_bytes(views(*[state(*b) for b in bl]), len(bl), pairs(*ds))))
    return out


def probe(lib):
    lib.cmtfpls_clear_error()
    calls = []
    for label, sym, args in table(lib):
        rc = getattr(lib, sym)(*args)
        msg = lib.cmtfpls_last_error().decode()
        lib.cmtfpls_clear_error()
        assert rc in (1, 2, 4), f"{label}: status {rc} ({msg}) -- every call of the table must be refused on the host"
        calls.append({"call": label, "status": rc, "error": msg})
    assert len({c["call"] for c in calls}) == len(calls)
    return {"calls": calls, "sizes": [{"export": s, "args": a, "bytes": v} for s, a, v in sizes(lib)],
            "lds_sizes": [{"export": s, "args": a, "bytes": v} for s, a, v in sizes(lib, lds=True)]}


def named(result):
    """The SIGNATURES names the table reaches."""
    return {"cmtfpls_" + c["call"].split(":")[0] for c in result["calls"]} | {s["export"] for s in result["sizes"] + result["lds_sizes"]}


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    res = probe(_lib.load())
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"{len(res['calls'])} calls, {len(res['sizes'])} + {len(res['lds_sizes'])} sizes -> {sys.argv[1]}; library {_lib.LIB_PATH}")
