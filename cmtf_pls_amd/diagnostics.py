"""Sample diagnostics of a fitted tPLS / ctPLS (validate.sample_diagnostics): Hotelling's T^2 of every sample's scores, its Q
residual (SPE: the squared norm of the part of X the model leaves out), R2X per variable, and control limits.

With x = X - X_mean over the finite entries (the calcR2X mask, util.py:7-15) and e = x - t W^T (W: the block's Khatri-Rao
loadings, never materialised):
  spe_i = sum_c e_ic^2,  ssq_i = sum_c x_ic^2,  n_observed_i = #finite x_i.,  r2x_c = 1 - sum_i e_ic^2 / sum_i x_ic^2
  t2_i  = (t_i - tbar)^T S^+ (t_i - tbar),  tbar, S (ddof 1): mean and covariance of the TRAINING scores
Per block these sums come from ONE read of X (cmtfpls_resid_rows_*, ProjectionMixin.residual_rows).  The scores of the training
rows are the fitted ones; new rows take transform's projection (tpls._project_blocks), so they are bitwise transform(X).

Limits (NaN with a `why` when I <= R + 1, I the number of training rows over every rank):
  t2_limit   training rows: (I - 1)^2 / I * Beta.ppf(level, R / 2, (I - R - 1) / 2);
             new rows: R (I - 1)(I + 1) / (I (I - R)) * F.ppf(level, R, I - R)
  spe_limit  Box's approximation g chi2.ppf(level, h), g = v / (2 m), h = 2 m^2 / v; m, v (ddof 1): mean and variance of the
             training rows' SPE (NaN when v = 0 or the training X was not kept)
tbar, S, m and v are computed once per fitted model and cached on it (a refit drops them): S and tbar need no read of X, m and v one
read of every training block.  Sharded models (comm): rows stay local; I, tbar, S, m, v and the column sums are all-reduced.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from .storage import _as_torch_dtype, notes_of, reports_storage, to_device_read

# reads of the caller's X that each projection form takes (project_readonly's forms); other forms work on private copies
_PROJECTION_READS = {
    "one-pass MTTKRP (one read, nothing written)": 1,
    "masked sequence, every row in registers (one read)": 1,
    "one-pass MTTKRP for the complete samples + masked sequence in registers for the incomplete ones": 2,
}


def _host(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _kept_training_blocks(pls, coupled: bool) -> Optional[list]:
    Xs = getattr(pls, "original_Xs", None) if coupled else getattr(pls, "original_X", None)
    if Xs is None:
        return None
    return list(Xs) if coupled else [Xs]


def t2_limit(I: int, R: int, level: float, training: bool):
    """(limit, why) of Hotelling's T^2 at `level` for I training rows and R components."""
    from scipy import stats

    if I <= R + 1:
        return float("nan"), f"I = {I} training rows <= R + 1 = {R + 1}"
    if training:
        return (I - 1) ** 2 / I * float(stats.beta.ppf(level, R / 2, (I - R - 1) / 2)), None
    return R * (I - 1) * (I + 1) / (I * (I - R)) * float(stats.f.ppf(level, R, I - R)), None


def spe_limit(m: float, v: float, I: int, R: int, level: float):
    """(limit, why): Box's g chi2_h(level), g = v / (2 m), h = 2 m^2 / v, from the training SPE's mean m and variance v."""
    from scipy import stats

    if I <= R + 1:
        return float("nan"), f"I = {I} training rows <= R + 1 = {R + 1}"
    if not (v > 0) or not (m > 0):
        return float("nan"), "the training SPE has no spread (v = 0)" if v == 0 else "the training SPE is not finite"
    return v / (2 * m) * float(stats.chi2.ppf(level, 2 * m * m / v)), None


def _spe_moments(comm, spe: torch.Tensor):
    """(m, v): mean and variance (ddof 1) of the training SPE over every rank."""
    head = comm.allreduce(torch.stack([spe.new_tensor(float(spe.numel())), spe.sum()]))
    n, s = head.tolist()
    m = s / n
    d = spe - m
    v = comm.allreduce((d * d).sum().reshape(1)).item() / (n - 1) if n > 1 else float("nan")
    return m, v


def _training_stats(pls, eng, st, coupled: bool, device: bool, spe_train: Optional[List[torch.Tensor]]):
    """The cached training statistics {"state", "I", "tbar", "S_pinv", "moments" (per block (m, v) or None), "why"}; returns
    (stats, came from the cache, training-block reads this call made)."""
    cache = getattr(pls, "_diagnostics_cache", None)
    if cache is not None and cache["state"] is st:
        return cache, True, 0
    comm = eng.comm
    T = st.T
    head = comm.allreduce(torch.cat([T.new_tensor([float(T.shape[0])]), T.sum(dim=0)]))
    I = int(round(head[0].item()))
    tbar = head[1:] / I
    Z = T - tbar
    S = comm.allreduce(Z.T @ Z) / max(I - 1, 1)
    S_pinv = torch.from_numpy(np.linalg.pinv(_host(S))).to(T.device)
    reads, why = 0, None
    if spe_train is None:
        Xs = _kept_training_blocks(pls, coupled)
        if Xs is None:
            why = "the training X was not kept (copy_X=False): no training SPE"
        else:
            dev = eng.be.device
            Xd = [to_device_read(X, blk.dtype or torch.float64, dev, pls=pls, entry="resid_rows") for X, blk in zip(Xs, st.blocks)]
            spe_train = [r[:, 0] for r, _ in eng.residual_rows(st, Xd, T, want_cols=False, device=device)]
            notes_of(pls).declined(Xd, eng.last_residual)
            reads = 1
    moments = None if spe_train is None else [_spe_moments(comm, s) for s in spe_train]
    cache = {"state": st, "I": I, "tbar": tbar, "S_pinv": S_pinv, "moments": moments, "why": why}
    pls._diagnostics_cache = cache
    return cache, False, reads


@reports_storage("diagnostics_report_")
def sample_diagnostics(pls, X=None, Y=None, level: float = 0.95, device: bool = True) -> dict:
    from .cmtf import ctPLS

    if not (0.0 < float(level) < 1.0):
        raise ValueError(f"level must be in (0, 1), got {level}")
    st = getattr(pls, "_state", None)
    if st is None:
        raise ValueError("sample_diagnostics needs a fitted tPLS or ctPLS")
    coupled = isinstance(pls, ctPLS)
    eng = pls._get_engine()
    be = eng.be
    dev = be.device
    R = st.n_components
    training = X is None
    with eng.device_ctx():
        if training:
            Xs = _kept_training_blocks(pls, coupled)
            if Xs is None:
                raise ValueError("the model was fitted with copy_X=False, so the training X was not kept: pass X")
            if Y is None:
                Y = pls.original_Y
            Xd = [to_device_read(X, blk.dtype or torch.float64, dev, pls=pls, entry="resid_rows") for X, blk in zip(Xs, st.blocks)]
            scores = st.T
            form, proj_reads = "fitted scores + residual pass", 0
        else:
            Xs = list(X) if coupled else [X]
            if coupled and len(Xs) != pls.Xs_len:
                raise ValueError(f"Training Xs has {pls.Xs_len} blocks, while the new Xs has {len(Xs)}")
            Xd = [to_device_read(x, _as_torch_dtype(pls._dtype, x), dev, pls=pls, entry="resid_rows") for x in Xs]
            scores = pls._project_dev(Xd if coupled else Xd[0])          # transform's projection: shape checks, forms, bits
            pform = "sequential passes on private copies (f32 matrix precision)" if pls._mixed else eng.last_projection["form"]
            form, proj_reads = f"projection ({pform}) + residual pass", _PROJECTION_READS.get(pform)
        if scores.stride(1) != 1:
            scores = scores.contiguous()
        res = eng.residual_rows(st, Xd, scores, want_cols=True, device=device)
        resid_forms = list(eng.last_residual)
        notes_of(pls).declined(Xd, resid_forms)
        stats, cached, train_reads = _training_stats(pls, eng, st, coupled, device,
                                                     [r[:, 0] for r, _ in res] if training else None)
        fallback = [f["why"] for f in resid_forms if f["why"]]
        I = stats["I"]
        Z = scores - stats["tbar"]
        t2 = ((Z @ stats["S_pinv"]) * Z).sum(dim=1)
        t2_lim, t2_why = t2_limit(I, R, level, training)
        spe, ssq, nobs, r2v, lims, lim_whys = [], [], [], [], [], []
        for b, (rows, cols) in enumerate(res):
            cols = eng.comm.allreduce(cols)
            rh, ch = _host(rows), _host(cols)
            spe.append(rh[:, 0].copy())
            ssq.append(rh[:, 1].copy())
            nobs.append(rh[:, 2].copy())
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.where(ch[:, 1] > 0, 1.0 - ch[:, 0] / np.where(ch[:, 1] > 0, ch[:, 1], 1.0), np.nan)
            r2v.append(r.reshape(tuple(st.blocks[b].shape[1:])))
            if stats["moments"] is None:
                lims.append(float("nan"))
                lim_whys.append(stats["why"])
            else:
                m, v = stats["moments"][b]
                lim, why = spe_limit(m, v, I, R, level)
                lims.append(lim)
                lim_whys.append(why)
        out = {"scores": _host(scores).copy(), "t2": _host(t2), "t2_limit": t2_lim, "level": float(level)}
        one = (lambda v: v) if coupled else (lambda v: v[0])
        out.update(spe=one(spe), ssq=one(ssq), n_observed=one(nobs), spe_limit=one(lims), r2x_per_variable=one(r2v))
        if Y is not None:
            yh = _host(Y).astype(np.float64)
            yh = yh.reshape(yh.shape[0], -1)
            if yh.shape[0] != scores.shape[0]:
                raise ValueError(f"Y has {yh.shape[0]} rows, while X has {scores.shape[0]}")
            out["y_residual"] = ((yh - pls._predict_from_scores(scores)) ** 2).sum(axis=1)
        else:
            out["y_residual"] = None
    x_reads = [None if proj_reads is None else proj_reads + 1 + train_reads for _ in st.blocks]
    pls.diagnostics_report_ = {
        "form": "torch fallback" if fallback else form,
        "why": "; ".join(sorted(set(fallback))) if fallback else None,
        "projection": None if training else pform,
        "rows": int(scores.shape[0]),
        "x_reads": x_reads,
        "training_stats": "cached" if cached else "computed",
        "training_reads": train_reads,
        "t2_limit_why": t2_why,
        "spe_limit_why": one(lim_whys),
    }
    return out

