"""Contribution plots of a fitted tPLS / ctPLS (validate.sample_contributions): for a flagged sample, which slice of which mode
carries its Q residual (SPE) and its Hotelling T^2.  The unit is the mode, not the cell: which of the J subjects,
which of the K time points.

Per block b (a tPLS has one), x = X - X_mean, W the block's Khatri-Rao loadings (never materialised), t_i the row's scores (the
fitted ones for the training rows, transform's for new rows, as sample_diagnostics takes them), tbar and S^+ the cached training
statistics of diagnostics._training_stats:
  e_ic = x_ic - sum_r t_ir W_cr                        where x_ic is finite, 0 elsewhere (the mask of DESIGN 8g)
  g_i  = S^+ (t_i - tbar),  h_i = U^-1 g_i,  U = I + triu(mean_b W_b^T W_b, 1)       (the matrix of the one-pass projection,
                                                                                     T U = mean_b X_b W_b)
  d_ic = (1 / n_blocks) x_ic sum_r h_ir W_cr           where x_ic is finite, 0 elsewhere
  spe_mode[m][i, j] = sum of e_ic^2, t2_mode[m][i, j] = sum of d_ic, over the cells c whose index along trailing mode m is j
For every mode sum_j spe_mode[m][i, j] = spe_i of sample_diagnostics.  d is the usual linear attribution x (.) (W* S^-1 t): over a
row WITHOUT missing values sum_b sum_c d_ic = t_i^T S^+ (t_i - tbar) = "t2_closure", which is t2_i when tbar = 0 (a fit on complete
data) and differs from it by tbar^T g_i otherwise.  Rows with missing values get the same formula over their observed cells; the
closure is NOT claimed for them: their scores come from the masked sequence, which is not linear in x.

Per block the mode sums come from ONE read of the selected rows of X (cmtfpls_contrib_rows_*, ProjectionMixin.contribution_rows):
the kernel sums over the first trailing mode and over the folded rest; order >= 4 reshapes the latter on the host.  Sharded
models: rows stay local and nothing new is reduced (the statistics are the cached, all-reduced ones).
"""
from __future__ import annotations

import numpy as np
import torch

from .diagnostics import _PROJECTION_READS, _host, _kept_training_blocks, _training_stats
from .storage import _as_torch_dtype, notes_of, reports_storage, to_device_read

MAX_CELLS = 1 << 28        # n * P above which cells=True is refused (2 GiB per returned float64 array)


def _row_list(rows, n_rows: int):
    if rows is None:
        return None
    r = np.asarray(rows)
    if r.ndim != 1 or r.dtype.kind not in "iu":
        raise ValueError(f"rows must be a 1-D integer array, got shape {r.shape} and dtype {r.dtype}")
    r = r.astype(np.int64)
    if r.size and (r.min() < 0 or r.max() >= n_rows):
        raise ValueError(f"rows must lie in [0, {n_rows}), got {int(r.min())} .. {int(r.max())}")
    if np.unique(r).size != r.size:
        raise ValueError("rows must be distinct")
    return r


def _mode_sums(first, rest, shape):
    """[(n, D_m) per trailing mode] from the kernel's two sums: `first` over everything but the first trailing mode (None for a
    matrix block), `rest` (n, B) over the first trailing mode only, B the folded later modes."""
    if first is None:
        return [_host(rest).copy()]
    out = [_host(first).copy()]
    r = _host(rest).reshape((rest.shape[0],) + tuple(shape[2:]))
    for m in range(1, r.ndim):
        out.append(r.sum(axis=tuple(a for a in range(1, r.ndim) if a != m)) if r.ndim > 2 else r.copy())
    return out


@reports_storage("contributions_report_")
def sample_contributions(pls, X=None, rows=None, cells: bool = False, device: bool = True) -> dict:
    from .cmtf import ctPLS

    st = getattr(pls, "_state", None)
    if st is None:
        raise ValueError("sample_contributions needs a fitted tPLS or ctPLS")
    coupled = isinstance(pls, ctPLS)
    eng = pls._get_engine()
    dev = eng.be.device
    nb = len(st.blocks)
    training = X is None
    with eng.device_ctx():
        if training:
            Xs = _kept_training_blocks(pls, coupled)
            if Xs is None:
                raise ValueError("the model was fitted with copy_X=False, so the training X was not kept: pass X")
            idx = _row_list(rows, int(st.T.shape[0]))
            Xd = [to_device_read(x, blk.dtype or torch.float64, dev, pls=pls, entry="contrib_rows") for x, blk in zip(Xs, st.blocks)]
            scores, pform, proj_reads = st.T, None, 0
        else:
            Xs = list(X) if coupled else [X]
            if coupled and len(Xs) != pls.Xs_len:
                raise ValueError(f"Training Xs has {pls.Xs_len} blocks, while the new Xs has {len(Xs)}")
            idx = _row_list(rows, int(Xs[0].shape[0]))
            Xd = [to_device_read(x, _as_torch_dtype(pls._dtype, x), dev, pls=pls, entry="contrib_rows") for x in Xs]
            scores = pls._project_dev(Xd if coupled else Xd[0])           # transform's projection: shape checks, forms, bits
            pform = "sequential passes on private copies (f32 matrix precision)" if pls._mixed else eng.last_projection["form"]
            proj_reads = _PROJECTION_READS.get(pform)
        n_all = int(scores.shape[0])
        if idx is None:
            ridx, T = None, (scores if scores.stride(1) == 1 else scores.contiguous())
        else:
            ridx = torch.from_numpy(idx).to(scores.device)
            T = scores.index_select(0, ridx)
        n = int(T.shape[0])
        if cells:
            for blk in st.blocks:
                if n * blk.A * blk.B > MAX_CELLS:
                    raise ValueError(f"cells=True would form {n} x {blk.A * blk.B} = {n * blk.A * blk.B} cells of a block, above the "
                                     f"limit of 2**28 = {MAX_CELLS}: select fewer rows")
        stats, cached, train_reads = _training_stats(pls, eng, st, coupled, device, None)
        Z = T - stats["tbar"]
        Gd = Z @ stats["S_pinv"]                                           # S^+ is symmetric
        t2 = (Gd * Z).sum(dim=1)
        closure = (Gd * T).sum(dim=1)
        H = eng.t2_direction_solve(st, Gd) / nb
        res = eng.contribution_rows(st, Xd, T, H, ridx, device=device)
        forms = list(eng.last_contribution)
        notes_of(pls).declined(Xd, forms)
        spe, spe_mode, t2_mode, spe_cells, t2_cells = [], [], [], [], []
        for blk, X_b, (speA, speB, t2A, t2B) in zip(st.blocks, Xd, res):
            spe_mode.append(_mode_sums(speA, speB, blk.shape))
            t2_mode.append(_mode_sums(t2A, t2B, blk.shape))
            spe.append(_host(speB).sum(axis=1))
            if cells:
                X2 = X_b.reshape(X_b.shape[0], -1)
                X2 = X2 if ridx is None else X2.index_select(0, ridx.to(X2.device))
                WA, WB = eng._kr_operands(blk, st.n_components)
                e, d = eng.contribution_cells(X2, T, H, WA, WB, blk.mean)
                spe_cells.append(_host(e).reshape((n,) + tuple(blk.shape[1:])))
                t2_cells.append(_host(d).reshape((n,) + tuple(blk.shape[1:])))
        one = (lambda v: v) if coupled else (lambda v: v[0])
        out = {"rows": np.arange(n_all, dtype=np.int64) if idx is None else idx, "scores": _host(T).copy(), "t2": _host(t2),
               "t2_closure": _host(closure), "spe": one(spe), "spe_mode": one(spe_mode), "t2_mode": one(t2_mode)}
        if cells:
            out.update(spe_cells=one(spe_cells), t2_cells=one(t2_cells))
    pls.contributions_report_ = {
        "form": [f["form"] for f in forms],
        "why": [f["why"] for f in forms],
        "projection": pform,
        "rows": n,
        "x_reads": [None if proj_reads is None else proj_reads + 1 for _ in st.blocks],
        "training_stats": "cached" if cached else "computed",
        "training_reads": train_reads,
    }
    return out
