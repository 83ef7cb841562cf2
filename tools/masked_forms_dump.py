#!/usr/bin/env python3
"""Dump everything the five masked cross-validation entry points return on a fixed table of small inputs, to compare two builds
of the library bit for bit: HipBackend.cv_masked (cmtfpls_cv_masked_f64), cv_masked_models (cmtfpls_cv_masked_models_f64,
factors=True), cv_masked_coupled (cmtfpls_cv_masked_coupled_f64, factors=True) and, for X of order 4, cv_masked_tensor
(cmtfpls_cv_masked_tensor_f64) and cv_masked_tensor_models (cmtfpls_cv_masked_tensor_models_f64, factors=True).  Every returned tensor (Ypred, n_iter, status,
info, the factors) goes into one .npz under "<case>/<name>".  The library is the one CMTFPLS_LIB names (else the in-tree build).
Not a test: it carries no expected values.  The table is the smallest that reaches every branch of csrc/masked_fold.hpp:
  trailing shapes  (1, 9) matrix block, partial-row contraction | (6, 5) one-wavefront rank-1 | (12, 10) workgroup rank-1, two
                   partial rows | (20, 16) a thread per column | (4, 70) min <= 8 but max > 64: workgroup rank-1
  NaN patterns     10 % at random | confined to one row (its own fold trains unmasked) | a column observed only in the rows that
                   the first fold / model holds out (c_p = 0 there: a NaN mean, a masked held-out batch)
  splits           4 folds | leave-one-out | 4 models with counts 0..3 and a permuted yrow | chunked calls, one model per launch
  stops            tol 1e-8 within 100 iterations | max_iter = 2 (the cap ends the loop)
  statuses         1 a training row with nothing observed | 2 fewer than two training rows | 3 a negative count, a yrow out of range
  coupled          each trailing shape as one block | tensor + complete tensor | matrix + tensor + tensor
  order 4          (3, 4, 2) | (6, 1, 5) | (2, 9, 3): every NaN pattern and stop, 4 folds and 4 models; one chunked call
Usage: python tools/masked_forms_dump.py OUT.npz      then      python tools/masked_forms_dump.py --compare A.npz B.npz
--compare: every array of A and B by name; float arrays as their 64-bit integer views (NaN payloads and signed zeros count);
prints the number of arrays and cases, every difference, and exits 1 on any."""
import os, sys
import numpy as np

SHAPES = [(1, 9), (6, 5), (12, 10), (20, 16), (4, 70)]
PATTERNS = ("random", "one_row", "heldout_column")
STOPS = {"tol": (1e-8, 100), "cap": (1e-8, 2)}
TENSOR_SHAPES = [(3, 4, 2), (6, 1, 5), (2, 9, 3)]
M = R = 3
NM = 4


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x,
                                                                            y.view(np.int64) if y.dtype == np.float64 else y)
        if not same:
            bad.append(k)
    print(f"{len(a.files)} arrays of {len({k.rsplit('/', 1)[0] for k in a.files})} cases compared: "
          f"{'all identical' if not bad else str(len(bad)) + ' differ'}")
    for k in bad:
        print("  differs:", k)
    return 1 if bad else 0


def block(rng, I, shape, T, pattern, held):
    """(I, A * B) block driven by the latent T with the NaN pattern; `held`: the rows the first fold / model holds out."""
    P = shape[0] * shape[1]
    X = T @ rng.standard_normal((T.shape[1], P)) + 0.3 * rng.standard_normal((I, P))
    if pattern == "random":
        hole = rng.random((I, P)) < 0.1
        hole[:, 0] = False                                                  # every row keeps an observed entry
        X[hole] = np.nan
    elif pattern == "one_row":
        X[5, 1::2] = np.nan
    elif pattern == "heldout_column":
        X[~held, P - 1] = np.nan
    return X


def main(out_path):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cmtf_pls_amd import _lib
    from cmtf_pls_amd.backend import HipBackend
    dev = torch.device("cuda:0")
    be = HipBackend(dev)
    out = {}

    def d(a, dt=torch.float64):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)

    def keep(case, res):
        assert res is not None, case                                        # every shape of the table is inside the forms
        if isinstance(res, tuple):
            res = dict(zip(("Ypred", "n_iter", "status", "info"), res))
        for k, v in res.items():
            for j, t in enumerate(v if isinstance(v, list) else [v]):
                if isinstance(t, torch.Tensor):
                    out[f"{case}/{k}{j if isinstance(v, list) else ''}"] = t.cpu().numpy()

    def dims(shapes):
        return [(2 if A == 1 else 3, A, B) for A, B in shapes]

    def models(rng, I):
        counts = rng.integers(0, 4, size=(NM, I)).astype(np.int32)
        counts[:, :2] = 0
        return counts, np.stack([rng.permutation(I) for _ in range(NM)]).astype(np.int32)

    seed = 0
    for si, shape in enumerate(SHAPES):
        I = 18 + si + (2 if si == 4 else 0)                                 # 18, 19, 20, 21, 24
        A, B = shape
        for pattern in PATTERNS:
            seed += 1
            rng = np.random.default_rng(seed)
            T = rng.standard_normal((I, R + 1))
            Y = d(T @ rng.standard_normal((R + 1, M)) + 0.3 * rng.standard_normal((I, M)))
            counts, yrow = models(rng, I)
            splits = {"kfold": (np.arange(I) % 4, 4), "loo": (np.arange(I), I)}
            for stop, (tol, max_iter) in STOPS.items():
                for split, (ids, K) in splits.items():
                    X = d(block(np.random.default_rng(seed), I, shape, T, pattern, ids == 0))
                    keep(f"folds/{A}x{B}/{pattern}/{split}/{stop}", be.cv_masked(X, Y, d(ids, torch.int32), K, A, B, R, tol, max_iter))
                X = d(block(np.random.default_rng(seed), I, shape, T, pattern, counts[0] == 0))
                keep(f"models/{A}x{B}/{pattern}/{stop}",
                     be.cv_masked_models(X, Y, d(counts, torch.int32), d(yrow, torch.int32), A, B, R, tol, max_iter, factors=True))
                keep(f"coupled/{A}x{B}/{pattern}/{stop}",
                     be.cv_masked_coupled([X], dims([shape]), Y, d(counts, torch.int32), d(yrow, torch.int32), R, tol, max_iter, factors=True))

    # ---- coupled block lists: tensor + complete tensor, matrix + tensor + tensor
    for name, shapes, complete in (("t+t", [(6, 5), (4, 7)], (1,)), ("m+t+t", [(1, 9), (6, 5), (12, 10)], ())):
        I = 22
        for pattern in PATTERNS:
            seed += 1
            rng = np.random.default_rng(seed)
            T = rng.standard_normal((I, R + 1))
            Y = d(T @ rng.standard_normal((R + 1, M)) + 0.3 * rng.standard_normal((I, M)))
            counts, yrow = models(rng, I)
            Xs = [d(block(rng, I, s, T, None if b in complete else pattern, counts[0] == 0)) for b, s in enumerate(shapes)]
            for stop, (tol, max_iter) in STOPS.items():
                keep(f"coupled/{name}/{pattern}/{stop}",
                     be.cv_masked_coupled(Xs, dims(shapes), Y, d(counts, torch.int32), d(yrow, torch.int32), R, tol, max_iter, factors=True))

    # ---- chunked calls (one fold / model per launch) and the statuses, on (6, 5) and on matrix + tensor
    I, A, B = 20, 6, 5
    rng = np.random.default_rng(1000)
    T = rng.standard_normal((I, R + 1))
    Y = d(T @ rng.standard_normal((R + 1, M)) + 0.3 * rng.standard_normal((I, M)))
    counts, yrow = models(rng, I)
    X = block(rng, I, (A, B), T, "random", None)
    Xm = block(rng, I, (1, 9), T, "random", None)
    two, two_dims = [d(Xm), d(X)], dims([(1, 9), (A, B)])
    ids = np.arange(I) % 4
    per = int(be.lib.cmtfpls_cv_masked_fold_workspace_bytes(I, A, B, M, R))
    keep("folds/chunked", be.cv_masked(d(X), Y, d(ids, torch.int32), 4, A, B, R, 1e-8, 100, max_ws_bytes=per))
    per = int(be.lib.cmtfpls_cv_masked_model_workspace_bytes(I, A, B, M, R)) + R * I * M * 8
    res = be.cv_masked_models(d(X), Y, d(counts, torch.int32), d(yrow, torch.int32), A, B, R, 1e-8, 100, factors=True, max_ws_bytes=per)
    assert res["launches"] == NM >= 3
    keep("models/chunked", res)
    blocks = (_lib.CvCoupledBlock * 2)(*[_lib.CvCoupledBlock(None, o, a, b) for o, a, b in two_dims])
    per = int(be.lib.cmtfpls_cv_masked_coupled_workspace_bytes(blocks, 2, I, M, R)) + R * I * M * 8
    res = be.cv_masked_coupled(two, two_dims, Y, d(counts, torch.int32), d(yrow, torch.int32), R, 1e-8, 100, factors=True, max_ws_bytes=per)
    assert res["launches"] == NM >= 3
    keep("coupled/chunked", res)
    # status 1: row 7 has nothing observed (in the tensor block): every fold / model that trains on it
    X1 = X.copy()
    X1[7] = np.nan
    c1 = counts.copy()
    c1[0, 7], c1[1, 7] = 0, 2
    # status 2: one training row; status 3: a negative count, a yrow out of range (either side)
    c23 = counts.copy()
    c23[0] = 0
    c23[0, 3] = 1
    c23[1, 4] = -1
    y23 = yrow.copy()
    y23[2, 6], y23[3, 8] = I, -1
    lone = np.zeros(I, dtype=np.int32)
    lone[-1] = 1                                                            # fold 1 holds out all rows but one
    keep("folds/status1", be.cv_masked(d(X1), Y, d(ids, torch.int32), 4, A, B, R, 1e-8, 100))
    keep("folds/status2", be.cv_masked(d(X), Y, d(1 - lone, torch.int32), 2, A, B, R, 1e-8, 100))
    for case, Xc, cc, yc in (("status1", X1, c1, yrow), ("status23", X, c23, y23)):
        keep(f"models/{case}", be.cv_masked_models(d(Xc), Y, d(cc, torch.int32), d(yc, torch.int32), A, B, R, 1e-8, 100, factors=True))
        keep(f"coupled/{case}", be.cv_masked_coupled([d(Xm), d(Xc)], two_dims, Y, d(cc, torch.int32), d(yc, torch.int32), R, 1e-8, 100,
                                                     factors=True))

    # ---- X of order 4 (I x A x B1 x B2 as I x A B1 B2): 4 folds and 4 models per pattern and stop, then one chunked call
    ids = np.arange(I) % 4
    for ti, (A, B1, B2) in enumerate(TENSOR_SHAPES):
        for pattern in PATTERNS:
            seed = 2000 + 10 * ti + PATTERNS.index(pattern)
            rng = np.random.default_rng(seed)
            T = rng.standard_normal((I, R + 1))
            Y = d(T @ rng.standard_normal((R + 1, M)) + 0.3 * rng.standard_normal((I, M)))
            counts, yrow = models(rng, I)
            for stop, (tol, max_iter) in STOPS.items():
                X = d(block(np.random.default_rng(seed), I, (A, B1 * B2), T, pattern, ids == 0))
                keep(f"tensor_folds/{A}x{B1}x{B2}/{pattern}/{stop}",
                     be.cv_masked_tensor(X, Y, d(ids, torch.int32), 4, A, B1, B2, R, tol, max_iter))
                X = d(block(np.random.default_rng(seed), I, (A, B1 * B2), T, pattern, counts[0] == 0))
                keep(f"tensor_models/{A}x{B1}x{B2}/{pattern}/{stop}",
                     be.cv_masked_tensor_models(X, Y, d(counts, torch.int32), d(yrow, torch.int32), A, B1, B2, R, tol, max_iter, factors=True))
    per = int(be.lib.cmtfpls_cv_masked_tensor_model_workspace_bytes(I, A, B1, B2, M, R)) + R * I * M * 8
    res = be.cv_masked_tensor_models(X, Y, d(counts, torch.int32), d(yrow, torch.int32), A, B1, B2, R, 1e-8, 100, factors=True, max_ws_bytes=per)
    assert res["launches"] == NM >= 3
    keep("tensor_models/chunked", res)
    torch.cuda.synchronize()
    np.savez(out_path, **out)
    status = np.concatenate([v.ravel() for k, v in out.items() if k.endswith("/status")])
    print(f"{len(out)} arrays of {len({k.rsplit('/', 1)[0] for k in out})} cases -> {out_path}; library {_lib.LIB_PATH}; statuses seen "
          f"{sorted(set(status.tolist()))}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
