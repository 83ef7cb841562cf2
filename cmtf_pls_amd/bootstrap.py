"""Bootstrap intervals of a fitted model's factors (validate.bootstrap_factors).

Resample b draws I rows with replacement (idx_b); its model is type(pls)(R, <the fitted model's settings>).fit(X[idx_b], Y[idx_b])
(a ctPLS: every block with the same rows), aligned to the fitted model (align_factors).  The result is the stack of the aligned
X loadings, Y loadings and coef_ over the resamples, their std and percentile intervals, and the out-of-bag (OOB) Q2Y.

Device form (tPLS and ctPLS): a resample differs from the fitted data only in each row's multiplicity c_bi, and the refit
on X[idx_b] is the fit in which every sum over rows is weighted by c_b.  n <= 32 resamples are the models of one
cmtfpls_kfold_state whose fold_of holds their n x I counts, and share every read of X.  Per pass and block:
  kfold_weighted_xcov   every model's S_b = X_0^T (c_b * (Y - nu_b)) and mean mu_b = X_0^T c_b / I from ONE pass over X
  per component         kfold_inner (a ctPLS: kfold_inner_coupled), the MTTKRP with n columns (a ctPLS: then kfold_combine_scores),
                        kfold_epilogue_weighted stage 1 (count-weighted row sums, tm = c t; the rows with c = 0 keep the score
                        predict gives them in T) and, but for the last component, the contraction X_0^T tm and stage 2
That is 2R reads of each block per pass.  The OOB prediction sums are built on the device from T, coef_ and Q and stay there;
per pass only the models' loadings, coef_, status and n_iter come back.  A one-model pass runs its resample twice (the
K-fold kernels take at least two models).  The passes run through kfold._device_passes: a pass whose status is set refits
its own resamples; anything outside the device form refits every resample on the regular engine.

A tPLS whose X has order 4 (I x A x B1 x B2), with EngineOptions.tensor_folds: the same passes on the I x A x B1 B2 view
with the Kronecker loading wB = wK (x) wL (kfold.py); the inner entry is cmtfpls_kfold_inner_tensor_f64 in the plain
layout, which also leaves every model's wK and wL, so a resample's loadings are [wA, wK, wL] as the refit's are.

With EngineOptions.masked_folds, a tPLS whose X has missing values runs every resample as a count-weighted workgroup of
cmtfpls_cv_masked_models_f64 instead (kfold.masked_models): factors and OOB predictions come back per model; X of order 4
with EngineOptions.masked_tensor_folds takes cmtfpls_cv_masked_tensor_models_f64, its per-mode stacks [wA, wK, wL].  With
EngineOptions.tensor_resamples_coupled, a ctPLS on complete data with a block of order 4 among blocks of order 2, 3 and 4 runs the
coupled passes with cmtfpls_kfold_inner_coupled_tensor_f64 as the inner entry: every block is taken as I x A x B (an order-4
block with B = B1 B2 and wB = wK (x) wL), the entry leaves every model's wK and wL of every order-4 block, and a resample's loadings of
such a block are [wA, wK, wL].  With
EngineOptions.masked_folds_coupled, a ctPLS with a missing value in some block does the same through cmtfpls_cv_masked_coupled_f64
(kfold.masked_models_coupled), every block's factors aligned by align_factors; with a block of order 4 and
EngineOptions.masked_tensor_folds_coupled through cmtfpls_cv_masked_coupled_tensor_f64, such a block's loadings [wA, wK, wL].

The route (kfold._route), the body of a pass (kfold._device_pass over kfold._weighted_models with kfold_weighted_xcov as the read; it
allocates the per-mode stacks Wk / Wl) and the report (kfold._passes_report, kfold._masked_run_report) are the shared ones of kfold.py.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .kfold import (MASKED, MASKED_COUPLED, MAX_FOLDS, OFF, PASSES, REFIT, _decline_blocks, _decline_coupled_tensor, _device_blocks, _device_pass,
                    _device_passes, _dims, _from_scores, _groups, _host, _masked_declined, _masked_run_report, _names, _passes_report,
                    _route, _tensor_dims, _to_dev, _training_data, _weighted_models, masked_coupled_report, masked_models,
                    masked_models_coupled, masked_models_report)
from .storage import FOLDS_WHY, reports_storage

_ENTRIES = ("kfold_weighted_xcov", "kfold_inner", "kfold_epilogue_weighted", "mttkrp", "xcov")
_ENTRIES_COUPLED = ("kfold_weighted_xcov", "kfold_inner_coupled", "kfold_combine_scores", "kfold_epilogue_weighted", "mttkrp", "xcov")
MAX_COLUMNS = 1024                # n (M + 1) columns of the weighted build (cmtfpls_kfold_weighted_xcov_*)


def resamples_for(I: int, n_resamples: int, resamples, random_state) -> np.ndarray:
    """The (B, I) row indices: `resamples` checked, or default_rng(random_state).integers(0, I, size=(n_resamples, I))."""
    if resamples is None:
        if int(n_resamples) < 2:
            raise ValueError(f"n_resamples must be at least 2, got {n_resamples}")
        return np.random.default_rng(random_state).integers(0, I, size=(int(n_resamples), I))
    rs = np.asarray(resamples)
    if rs.ndim != 2 or rs.shape[1] != I:
        raise ValueError(f"resamples must be a (B, {I}) array of row indices, got shape {rs.shape}")
    if rs.shape[0] < 2:
        raise ValueError(f"resamples must hold at least two resamples, got {rs.shape[0]}")
    if rs.dtype.kind not in "iu":
        raise ValueError("resamples must hold integer row indices")
    if rs.min() < 0 or rs.max() >= I:
        raise ValueError(f"row index out of range: resamples hold {int(rs.min())}..{int(rs.max())}, rows are 0..{I - 1}")
    return rs.astype(np.int64)


def model_factors(pls):
    """(X loadings per block, each the list of modes 1.. as (dim, R) arrays; Q (M, R); coef_ (R, R)) of a fitted tPLS / ctPLS."""
    from .cmtf import ctPLS

    blocks = [f[1:] for f in pls.Xs_factors] if isinstance(pls, ctPLS) else [pls.X_factors[1:]]
    return [[np.asarray(L, dtype=np.float64) for L in b] for b in blocks], np.asarray(pls.Y_factors[1], np.float64), \
        np.asarray(pls.coef_, np.float64)


def align_factors(ref_blocks, blocks, Q: np.ndarray, coef: np.ndarray):
    """A model's factors aligned to the fitted model's, component a at a time: every X-mode loading column (modes 1.. of every
    block) is flipped so that its inner product with the fitted model's column is >= 0 (a zero inner product counts as +1);
    d_a is the product of the flips of the FIRST block's modes; q_a becomes d_a q_a and coef_ becomes D coef_ D, D = diag(d).  For a
    tPLS the flips of a component's modes multiply its score by d_a, so the model's predictions are unchanged.
    ref_blocks / blocks: per block, the list of (dim, R) mode loadings; returns (blocks, Q, coef) aligned (new arrays)."""
    R = Q.shape[1]
    d = np.ones(R)
    out = []
    for bi, (ref, modes) in enumerate(zip(ref_blocks, blocks)):
        aligned = []
        for Lr, L in zip(ref, modes):
            s = np.where(np.einsum("jr,jr->r", Lr, L) < 0.0, -1.0, 1.0)
            aligned.append(L * s)
            if bi == 0:
                d = d * s
        out.append(aligned)
    return out, Q * d, coef * d[:, None] * d[None, :]


def aligned_factors(pls, model):
    """The factors of a fitted `model` aligned to the fitted `pls` (align_factors): (X loadings laid out like pls.X_factors[1:],
    a ctPLS like [Xs_factors[b][1:] for each block b]; Y loadings (M, R); coef_ (R, R))."""
    from .cmtf import ctPLS

    ref, _, _ = model_factors(pls)
    blocks, Q, coef = model_factors(model)
    blocks, Q, coef = align_factors(ref, blocks, Q, coef)
    return (blocks if isinstance(pls, ctPLS) else blocks[0]), Q, coef


def _take(X, idx: np.ndarray):
    if isinstance(X, torch.Tensor):
        return X.index_select(0, torch.from_numpy(idx).to(X.device))
    return X[idx]


def refit(pls, X, Y, idx: np.ndarray, oob: np.ndarray, tol: float, max_iter: int):
    """Resample idx's literal refit on the regular engine with the model's settings: (blocks, Q, coef_ of the refit, n_iter, the
    predictions (R, n_oob, M) of the rows `oob` with the first r = 1..R components)."""
    coupled = isinstance(X, list)
    R = pls.n_components
    m = type(pls)(R, dtype=pls._dtype, device=pls._device, backend=pls._backend, algorithm=pls._algorithm, graphs=pls._graphs,
                  matrix_precision="f32" if pls._mixed else "f64", options=pls._options, sparsity=getattr(pls, "sparsity", None))
    m.fit([_take(b, idx) for b in X] if coupled else _take(X, idx), _take(Y, idx), tol=tol, max_iter=max_iter)
    pred = None
    if oob.size:
        scores = m.transform([_take(b, oob) for b in X] if coupled else _take(X, oob))
        pred = np.stack([_from_scores(scores, m.coef_, m.Y_factors[1].T, m.Y_mean, r) for r in range(1, R + 1)])
    blocks, Q, coef = model_factors(m)
    return blocks, Q, coef, [int(v) for v in m.n_iter_], pred


def _device_resamples(pls, Xs, Y, counts: np.ndarray, tol: float, max_iter: int, coupled: bool, res: list, oob_sum, tensor=None):
    """The device form's run(pass, e0, g) of kfold._device_passes: resamples e0 .. e0 + g - 1 as the models of one state (a
    one-model pass as two copies of its resample).  Each resample's (blocks, Q, coef_) goes to res[e]; a pass without a status
    adds its models' OOB predictions to oob_sum = [sums (R, I, M), counts (I,)] on the device.  tensor = (B1, B2): a tPLS's
    order-4 X (kfold._tensor_dims); its loadings are [wA, wK, wL].  tensor = [(B1, B2), ..]: a ctPLS with blocks of order 4 ((0, 0):
    another order); an order-4 block's loadings are [wA, wK, wL], read from its slice of the entry's Wk / Wl."""
    be = pls._get_engine().be
    R = pls.n_components
    dev = be.device
    I = counts.shape[1]
    Yd = _to_dev(_host(Y).reshape(I, -1).astype(np.float64), dev)
    M = Yd.shape[1]
    blocks = _device_blocks(pls, Xs, dev)
    counts_d = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(dev)  # one upload of the counts

    def run(passes, e0, g):
        n, C, Cf = _weighted_models(counts_d, e0, g)
        nu = (Cf @ Yd) / I                                                            # n x M: the resamples' means of Y
        Yc = Yd.unsqueeze(0) - nu.unsqueeze(1)                                        # n x I x M
        Yw = torch.cat([(Cf.unsqueeze(2) * Yc).permute(1, 0, 2).reshape(I, n * M), Cf.t()], dim=1).contiguous()   # Y''
        Yk = torch.where(C.unsqueeze(2) > 0, Yc, 0.0).contiguous()                    # rows with c = 0 are 0
        got = _device_pass(pls, Xs, blocks, coupled, "kfold_weighted_xcov",           # one read of each block
                           [lambda X2, A, B, S, mean: be.kfold_weighted_xcov(X2, A, B, Yw, n, M, S, mean)],
                           C, Yk, 1, passes == 0, tol, max_iter, tensor, mode_loadings=True, weighted=True)
        if isinstance(got, str):
            return _declined(got)
        shared, own = got
        status = shared["status"][:g].cpu().numpy()
        n_iter = shared["n_iter"][:g].cpu().numpy()
        if not status.any():
            T, coef, Q = shared["T"][:g], shared["coef"][:g], shared["Q"][:g]
            out = (C[:g] == 0).to(torch.float64)                                      # g x I: the models' OOB rows
            H = torch.bmm(T, coef) * out.unsqueeze(2)                                 # g x I x R: scores @ coef_ on OOB rows
            step = torch.bmm(H.permute(2, 1, 0), Q.permute(1, 0, 2))                  # R x I x M: component c's term, summed
            oob_sum[0] += torch.cumsum(step, dim=0) + (out.t() @ nu[:g]).unsqueeze(0)  # r-component predictions, summed
            oob_sum[1] += out.sum(dim=0)
            coef_h, Q_h = coef.cpu().numpy(), Q.cpu().numpy()
            Wa = [o["Wa"][:g].cpu().numpy() for o in own]
            Wb = [o["Wb"][:g].cpu().numpy() for o in own]
            if isinstance(tensor, list):                                              # block b's slice: n x R x B1_b (B2_b), or None
                Wk, Wl = _mode_slices(shared["Wk"].cpu().numpy(), shared["Wl"].cpu().numpy(), tensor, n, R)
            elif tensor is not None:
                Wk, Wl = (shared[w][:g].cpu().numpy() for w in ("Wk", "Wl"))
            for j in range(g):
                if isinstance(tensor, list):
                    modes = [[wa[j].T, wk[j].T, wl[j].T] if X.ndim == 4 else [wb[j].T] if X.ndim == 2 else [wa[j].T, wb[j].T]
                             for X, wa, wb, wk, wl in zip(Xs, Wa, Wb, Wk, Wl)]
                elif tensor is not None:                                              # wB = wK (x) wL: the modes themselves
                    modes = [[Wa[0][j].T, Wk[j].T, Wl[j].T]]
                else:
                    modes = [([wb[j].T] if X.ndim == 2 else [wa[j].T, wb[j].T]) for X, wa, wb in zip(Xs, Wa, Wb)]
                res[e0 + j] = (modes, Q_h[j].T, coef_h[j])
        return np.zeros((g, R)), [n_iter[j].tolist() for j in range(g)], status

    def _declined(why):
        oob_sum[0].zero_()                                                            # every resample refits
        oob_sum[1].zero_()
        return why
    return run


def _mode_slices(Wk: np.ndarray, Wl: np.ndarray, tensor, n: int, R: int):
    """Per block the n x R x B1_b and n x R x B2_b views of cmtfpls_kfold_inner_coupled_tensor_f64's Wk / Wl (the tensor blocks'
    slices lie one after another in block order); None for a block of another order."""
    ks, ls, ok, ol = [], [], 0, 0
    for B1, B2 in tensor:
        if B2 == 0:
            ks.append(None)
            ls.append(None)
            continue
        ks.append(Wk[ok:ok + n * R * B1].reshape(n, R, B1))
        ls.append(Wl[ol:ol + n * R * B2].reshape(n, R, B2))
        ok += n * R * B1
        ol += n * R * B2
    return ks, ls


def _as_blocks_of_order3(Xs):
    """Order-4 blocks as the coupled passes see them, I x A x B1 B2 (kfold._dims), for the checks of _decline_blocks that do not
    depend on EngineOptions.tensor_folds_coupled; the other blocks as they are."""
    return [X.reshape(X.shape[0], X.shape[1], -1) if X.ndim == 4 else X for X in Xs]


def _spread(stack, level: float):
    """(std over the resamples with ddof 1, percentile interval (2, ...)) of a stack or of each stack in nested lists."""
    if isinstance(stack, list):
        pairs = [_spread(s, level) for s in stack]
        return [p[0] for p in pairs], [p[1] for p in pairs]
    q = 100.0 * (1.0 - level) / 2.0
    return stack.std(axis=0, ddof=1), np.percentile(stack, [q, 100.0 - q], axis=0)


@reports_storage("bootstrap_report_", FOLDS_WHY)
def bootstrap(pls, n_resamples: int = 100, resamples=None, random_state=0, level: float = 0.95, device_folds: bool = True,
              tol: float = 1e-8, max_iter: int = 100) -> dict:
    if not (0.0 < float(level) < 1.0):
        raise ValueError(f"level must be in (0, 1), got {level}")
    X, Y = _training_data(pls)
    coupled = isinstance(X, list)
    Xs = X if coupled else [X]
    I = Y.shape[0]
    idx = resamples_for(I, n_resamples, resamples, random_state)
    NB = idx.shape[0]
    R = pls.n_components
    counts = np.stack([np.bincount(r, minlength=I) for r in idx])
    Yh = _host(Y).reshape(I, -1).astype(np.float64)
    M = Yh.shape[1]
    ref, _, _ = model_factors(pls)

    G = 0
    masked = None
    ctensor = None                                                # (B1, B2) per block of a ctPLS under tensor_resamples_coupled
    route, detail = _route(pls, X, device_folds)
    why: Optional[str] = detail if route in (OFF, REFIT) else None
    if route in (MASKED, MASKED_COUPLED):       # EngineOptions.masked_folds, masked_tensor_folds (8s), masked_folds_coupled (8j)
        masked, mwhy = (masked_models if route == MASKED else masked_models_coupled)(pls, X, Y, counts.astype(np.int32), None, tol,
                                                                                      max_iter, factors=True)
        if masked is None:
            why = _masked_declined(detail, mwhy)
    elif route == PASSES:
        G = min(_groups(X, 1, min(NB, I, MAX_FOLDS, MAX_COLUMNS // (M + 1))) for X in Xs)   # the LDS of every block's score pass
        if coupled and pls._get_engine().opt.tensor_resamples_coupled and _tensor_dims(Xs, coupled=True) is not None:
            # EngineOptions.tensor_resamples_coupled: the checks of the coupled passes on the I x A x B1 B2 views, then
            # cmtfpls_kfold_inner_coupled_tensor_f64's own limits, as the K-fold path checks them
            ctensor = _tensor_dims(Xs, coupled=True)
            why = _decline_blocks(pls, _as_blocks_of_order3(Xs), _names(Xs, coupled), Y, max(G, 2),
                                  _ENTRIES_COUPLED + ("kfold_inner_coupled_tensor",))
            if why is None:
                why = _decline_coupled_tensor(pls._get_engine().be, [_dims(X) for X in Xs], ctensor, M)
        else:
            why = _decline_blocks(pls, Xs, _names(Xs, coupled), Y, max(G, 2), _ENTRIES_COUPLED if coupled else _ENTRIES,
                                  tensor_ok=not coupled)
    if ctensor is not None and why is None and masked is None:
        tensor = ctensor
    else:
        tensor = _tensor_dims(Xs) if not coupled and why is None and masked is None and pls._get_engine().opt.tensor_folds else None
    res = [None] * NB
    dev = pls._get_engine().be.device if why is None and masked is None else torch.device("cpu")
    oob_sum = [torch.zeros(R, I, M, dtype=torch.float64, device=dev), torch.zeros(I, dtype=torch.float64, device=dev)]

    def refit_one(e):
        oob = np.flatnonzero(counts[e] == 0)
        blocks, Q, coef, n_iter, pred = refit(pls, X, Y, idx[e], oob, tol, max_iter)
        res[e] = (blocks, Q, coef)
        if pred is not None:
            oob_sum[0][:, torch.from_numpy(oob).to(dev)] += torch.from_numpy(pred).to(dev)
            oob_sum[1][torch.from_numpy(oob).to(dev)] += 1.0
        return np.zeros(R), n_iter

    if masked is not None:                                                            # resample b is model b; Ypred is 0 in its bag
        n_iters, refitted = masked["n_iter"].tolist(), []
        for e in range(NB):
            if masked["status"][e]:
                _, n_iters[e] = refit_one(e)
                refitted.append(e)
                continue
            if coupled and "tensor" in masked:                                        # an order-4 block: [wA, wK, wL]
                modes = [[wa[e].T, wk[e].T, wl[e].T] if Xb.ndim == 4 else [wb[e].T] if Xb.ndim == 2 else [wa[e].T, wb[e].T]
                         for Xb, wa, wb, wk, wl in zip(Xs, masked["Wa"], masked["Wb"], masked["Wk"], masked["Wl"])]
            elif coupled:
                modes = [[wb[e].T] if Xb.ndim == 2 else [wa[e].T, wb[e].T] for Xb, wa, wb in zip(Xs, masked["Wa"], masked["Wb"])]
            elif "tensor" in masked:                                                  # order-4 X: wB = wK (x) wL, the modes themselves
                modes = [[masked["Wa"][e].T, masked["Wk"][e].T, masked["Wl"][e].T]]
            else:
                modes = [[masked["Wb"][e].T] if X.ndim == 2 else [masked["Wa"][e].T, masked["Wb"][e].T]]
            res[e] = (modes, masked["Q"][e].T, masked["coef"][e])
            oob_sum[0] += torch.from_numpy(masked["Ypred"][e])
            oob_sum[1] += torch.from_numpy((counts[e] == 0).astype(np.float64))
    else:
        _, n_iters, passes, why = _device_passes(pls, NB, G, "resamples", why,
                                                 lambda: _device_resamples(pls, Xs, Y, counts, tol, max_iter, coupled, res, oob_sum,
                                                                           tensor),
                                                 refit_one)
    aligned = [align_factors(ref, *r) for r in res]
    nmodes = [len(b) for b in ref]
    Xf = [[np.stack([a[0][b][j] for a in aligned]) for j in range(nmodes[b])] for b in range(len(ref))]
    stacks = {"X_factors": Xf if coupled else Xf[0], "Y_loadings": np.stack([a[1] for a in aligned]),
              "coef": np.stack([a[2] for a in aligned])}
    spread = {k: _spread(v, level) for k, v in stacks.items()}

    sums, seen = oob_sum[0].cpu().numpy(), oob_sum[1].cpu().numpy()
    rows = seen > 0
    oob_q2y = np.full(R, np.nan)                                                      # no row out of bag: no OOB Q2Y
    if rows.any():
        pred = sums[:, rows] / seen[rows][None, :, None]
        y = Yh[rows]
        oob_q2y = 1.0 - ((pred - y) ** 2).reshape(R, -1).sum(axis=1) / (y ** 2).sum()   # validate.py:35-37 on the OOB rows

    if masked is not None:
        rep = (masked_coupled_report if coupled else masked_models_report)(masked, refitted, "resamples")
        pls.bootstrap_report_ = _masked_run_report(rep, "resamples", NB, "models_per_pass", n_iters)
    else:
        pls.bootstrap_report_ = _passes_report(f"{G} resamples per pass", "cmtfpls_kfold_weighted_xcov_*", "cmtfpls_kfold_epilogue_weighted_f64",
                                               Xs, coupled, passes, 2 * R * passes, why, "resample",
                                               "one refit per resample on the regular engine", {"resamples": int(NB)},
                                               ("models_per_pass", G), n_iters, tensor)
    return {"resamples": idx, **stacks, "se": {k: v[0] for k, v in spread.items()}, "ci": {k: v[1] for k, v in spread.items()},
            "oob_q2y": oob_q2y, "oob_rows": int(rows.sum())}
