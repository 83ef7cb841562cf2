#!/usr/bin/env python3
"""Dump everything the cross-covariance fold kernels return on a fixed table of small inputs, to compare two builds of the library
bit for bit.  Leave-one-out: HipBackend.loo_tpls (form "xcov", cmtfpls_loo_xcov_f64), loo_tpls_tensor (cmtfpls_loo_xcov_tensor_f64),
loo_ctpls (cmtfpls_loo_xcov_coupled_f64) and loo_ctpls_tensor (cmtfpls_loo_xcov_coupled_tensor_f64): Ypred and n_iter.  K-fold
(K = 3): the state that kfold.py builds (_fold_y, kfold_xcov, _state) taken through kfold._components, whose inner entry is
cmtfpls_kfold_inner_f64, _tensor_f64, _coupled_f64, _coupled_tensor_f64 and, with model_fold = (0, 1, 2) in one group, _grouped_f64,
_coupled_grouped_f64 and the grouped layouts of the two tensor entries: Q, n_iter, status, vec, coef, T, Tout and per block Wa, Wb,
WA, WB, Wk, Wl.  Every array goes into one .npz under "<case>/<name>".  The library is the one CMTFPLS_LIB names (else the in-tree
build).  Not a test: it carries no expected values.  The table is the smallest that reaches every branch of csrc/fold_loop.hpp and
csrc/loo_xcov_fold.hpp:
  trailing shapes  (1, 9) matrix block | (5, 7) | (40, 6) the transpose path | (17, 20) a second MFMA tile with remainder |
                   order 4: (5, 7, 3), (40, 3, 2), (6, 1, 5), (4, 17, 2) | (2, 32, 33): B >= 1024, one row group in lx_cp3, and
                   P > 448, the unrolled trip of lx_wave_dot
  M                1 the tail only | 5 the unrolled trip plus tail | 17 a second 16-column chunk of the S build
  I = 9            the four-row loops have a remainder;  R = 3
  stops            tol 1e-8 within 100 passes | a cap of 2 passes
  chunked          the four leave-one-out entries four folds a launch (fold0 = 4, 8)
  coupled          each trailing shape as one block | two and three blocks mixing orders 2, 3 and 4
The inputs are small integers (a latent structure rounded), so they are exact in every storage type.
Usage: python tools/xcov_folds_dump.py OUT.npz [FIXTURE.npz]     then     python tools/xcov_folds_dump.py --compare A.npz B.npz
FIXTURE: what tests/golden/loo_xcov_tensor_parent.npz holds, the order-4 cases of the two tensor leave-one-out entries: per input set
s the blocks s/X{b} (int8, I x prod(shape)), s/shape{b} and s/Y (int8, I x 17, of which a case takes the first M columns), and per
entry e ("t": cmtfpls_loo_xcov_tensor_f64, one block alone; "c": cmtfpls_loo_xcov_coupled_tensor_f64) and stop the outputs
s/e/{stop}/Ypred (I x sum(Ms)) and /n_iter (I x R len(Ms)), the runs with M = Ms[0], Ms[1], .. side by side; Ms, stops and
stop_values (tol, max_iter) name the cases.
--compare: every array of A and B by name; float arrays as their 64-bit integer views (NaN payloads and signed zeros count);
prints the number of arrays and cases, every difference, and exits 1 on any."""
import ctypes, os, sys
import numpy as np

MATRIX_SHAPES = [(1, 9), (5, 7), (40, 6), (17, 20)]
TENSOR_SHAPES = [(5, 7, 3), (40, 3, 2), (6, 1, 5), (4, 17, 2), (2, 32, 33)]
SETS = {"m+t": [(1, 9), (5, 7)], "m+c": [(1, 9), (5, 7, 3)], "m+t+t": [(1, 9), (40, 6), (17, 20)], "m+t+c": [(1, 9), (5, 7), (4, 17, 2)],
        "c+t+c": [(6, 1, 5), (40, 6), (5, 7, 3)]}
MS = (1, 5, 17)
STOPS = {"tol": (1e-8, 100), "cap": (1e-8, 2)}
I, R, K = 9, 3, 3


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


def name_of(shapes):
    return "+".join("x".join(str(d) for d in s) for s in shapes)


def inputs(shapes, seed):
    """The blocks (I x prod(shape) each) and Y (I x 17) of one case: int8, driven by one latent T."""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((I, R + 1))

    def draw(P):
        return np.clip(np.rint(8.0 * (T @ rng.standard_normal((R + 1, P)) + 0.3 * rng.standard_normal((I, P)))), -127, 127).astype(np.int8)

    return [draw(int(np.prod(s))) for s in shapes], draw(max(MS))


def main(out_path, fixture_path=None):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cmtf_pls_amd import _lib, kfold as KF
    from cmtf_pls_amd.backend import HipBackend
    dev = torch.device("cuda:0")
    be = HipBackend(dev)
    out, fix, sets, declined = {}, {}, {}, []

    def d(a, dt=torch.float64):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)

    def keep(case, **arrays):
        for k, v in arrays.items():
            out[f"{case}/{k}"] = v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

    def views(shapes):
        """(order, A, B) and (B1, B2) per block: the I x A x B view of kfold._dims."""
        dims = [(2, 1, s[1]) if s[0] == 1 and len(s) == 2 else (3, s[0], s[1]) if len(s) == 2 else (4, s[0], s[1] * s[2]) for s in shapes]
        return dims, [(s[1], s[2]) if len(s) == 3 else (0, 0) for s in shapes]

    def loo(case, shapes, Xs, Y, tol, max_iter, coupled, chunked):
        dims, tensor = views(shapes)
        any4 = any(o == 4 for o, _, _ in dims)
        M = Y.shape[1]
        if coupled:
            blocks = (_lib.LooCoupledBlock * len(Xs))(*[_lib.LooCoupledBlock(None, None, o, A, B) for o, A, B in dims])
            pairs = (ctypes.c_int * (2 * len(Xs)))(*[v for p in tensor for v in p])
            per = int(be.lib.cmtfpls_loo_xcov_coupled_tensor_fold_workspace_bytes(blocks, len(Xs), pairs, I, M, R)) if any4 else \
                int(be.lib.cmtfpls_loo_xcov_coupled_fold_workspace_bytes(blocks, len(Xs), I, M, R))
            budget = 4 * per if chunked else None
            res = be.loo_ctpls_tensor(Xs, Y, dims, tensor, R, tol, max_iter, budget) if any4 else be.loo_ctpls(Xs, Y, dims, R, tol, max_iter, budget)
        else:
            (_, A, B), (B1, B2) = dims[0], tensor[0]
            per = int(be.lib.cmtfpls_loo_xcov_tensor_fold_workspace_bytes(I, A, B1, B2, M, R)) if any4 else \
                int(be.lib.cmtfpls_loo_xcov_fold_workspace_bytes(I, A, B, M, R))
            budget = 4 * per if chunked else None
            res = be.loo_tpls_tensor(Xs[0], Y, A, B1, B2, R, tol, max_iter, budget) if any4 else \
                be.loo_tpls(Xs[0], Y, A, B, R, tol, max_iter, budget, forms=("xcov",))
        assert res is not None, case                                         # every shape of the table is inside the forms
        keep(case, Ypred=res[0], n_iter=res[1])
        return any4

    def kfold(case, shapes, Xs, Y, tol, max_iter, coupled, grouped):
        dims, tensor = views(shapes)
        any4 = any(o == 4 for o, _, _ in dims)
        Yh = Y.cpu().numpy()
        M = Yh.shape[1]
        ids = np.arange(I) % K
        order, off, ybar, nu, Yk = KF._fold_y(Yh, ids, K)
        ydev, order_d, off_d, nudev = d(Yh - ybar), d(order, torch.int32), d(off, torch.int32), d(nu - ybar)
        blocks = []
        for X2, (_, A, B) in zip(Xs, dims):
            S, mean = be.empty(K, M, A * B), be.empty(K, A * B)
            assert be.kfold_xcov(X2, A, B, ydev, order_d, off_d, K, nudev, S, mean) is not None, case
            blocks.append((A, B, S, mean))
        st, shared, own = KF._state(be, d(ids, torch.int32), d(Yk), blocks, R, 1)
        tn = (tensor if coupled else tensor[0]) if any4 else None
        Wk = be.zeros(sum(K * R * b1 for b1, b2 in tensor if b2) + 1)
        Wl = be.zeros(sum(K * R * b2 for b1, b2 in tensor if b2) + 1)
        why = KF._components(be, Xs, st, shared, own, R, tol, max_iter, coupled, grouped=(d(np.arange(K), torch.int32), 1) if grouped else None,
                             tensor=tn, tensor_out=(Wk, Wl) if any4 else None)
        if why is not None:
            declined.append(f"{case}: {why}")
        keep(case, **{k: shared[k] for k in ("Q", "n_iter", "status", "vec", "coef", "T", "Tout")}, Wk=Wk, Wl=Wl,
             **{f"{k}{b}": o[k] for b, o in enumerate(own) for k in ("Wa", "Wb", "WA", "WB")})

    cases = [(name_of([s]), [s]) for s in MATRIX_SHAPES + TENSOR_SHAPES] + [(f"{k}:{name_of(v)}", v) for k, v in SETS.items()]
    for seed, (name, shapes) in enumerate(cases, start=1):
        X8, Y8 = inputs(shapes, seed)
        Xs = [d(x) for x in X8]
        for M in MS:
            Y = d(Y8[:, :M])
            for stop, (tol, max_iter) in STOPS.items():
                tag = f"{name}/M{M}/{stop}"
                for coupled in ((False, True) if len(shapes) == 1 else (True,)):
                    form = "coupled" if coupled else "single"
                    any4 = loo(f"loo/{form}/{tag}", shapes, Xs, Y, tol, max_iter, coupled, False)
                    if any4:                                                # (the fixture: the inputs once per input set)
                        key = f"s{sets.setdefault(name, len(sets))}"
                        for b, (sh, x) in enumerate(zip(shapes, X8)):
                            fix[f"{key}/X{b}"], fix[f"{key}/shape{b}"] = x, np.array(sh)
                        fix[f"{key}/Y"] = Y8
                        for k in ("Ypred", "n_iter"):                       # the Ms side by side: fewer, larger arrays
                            fk = f"{key}/{'c' if coupled else 't'}/{stop}/{k}"
                            fix[fk] = np.concatenate([fix[fk], out[f"loo/{form}/{tag}/{k}"]], axis=1) if fk in fix else out[f"loo/{form}/{tag}/{k}"]
                    if stop == "tol" and M == 5:
                        loo(f"loo/{form}/chunked/{tag}", shapes, Xs, Y, tol, max_iter, coupled, True)
                    for grouped in (False, True):
                        kfold(f"kfold/{form}{'_grouped' if grouped else ''}/{tag}", shapes, Xs, Y, tol, max_iter, coupled, grouped)
    torch.cuda.synchronize()
    np.savez(out_path, **out)
    if fixture_path:
        np.savez_compressed(fixture_path, n_sets=len(sets), Ms=np.array(MS), stops=np.array(list(STOPS)),
                            stop_values=np.array(list(STOPS.values())), R=R, **fix)
    print(f"{len(out)} arrays of {len({k.rsplit('/', 1)[0] for k in out})} cases -> {out_path}; library {_lib.LIB_PATH}; "
          f"{len(declined)} K-fold runs ended early")
    for w in declined:
        print("  ", w)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    main(*sys.argv[1:])
