"""Variable importance of a fitted tPLS / ctPLS (validate.selectivity_ratio, validate.vip_scores): which variables
carry the prediction.

Selectivity ratio, by target projection (Rajalahti et al. 2009).  The fitted response tau = scores coef_ Q^T (I x M, not re-centred)
is a linear image of the centred X, so the part of a cell's column that predicts response m is its projection onto tau[:, m].  Per
block, with x = X - X_mean, o = isfinite(x) (the calcR2X mask of sample_diagnostics), c a cell (C-order over X.shape[1:]):
  a[m, c] = sum_i o x tau_im,   d[m, c] = sum_i o tau_im^2,   s[c] = sum_i o x^2,   n[c] = sum_i o
  tp_loading = a / d,  explained = a^2 / d,  residual = max(s - explained, 0),  sr = explained / residual
sr is NaN where d = 0 or n = 0 and inf where residual = 0 < explained.  Per mode k >= 1, sr_mode[k][m, j] = sum explained / sum
residual over the cells of slice j (NaN cells skipped, an all-NaN slice NaN).  f_limit = F.ppf(level, I - 2, I - 3) with I the
training rows over every rank (NaN with a why when I <= 3); with missing values a column has n[c] <= I observations, so the limit is
nominal there and n_observed is returned alongside.  The four sums come from ONE read of every block (cmtfpls_selectivity_cols_*,
ProjectionMixin.selectivity_cols); the scores of the training rows are the fitted ones, new rows take transform's projection.
Sharded models: rows stay local; a, d, s, n, sum tau^2 and the row count are all-reduced before any ratio.

VIP is host algebra on the fitted factors, no read of X: s_r = max(R2Y[r] - R2Y[r - 1], 0) (R2Y[-1] = 0) and, per mode k >= 1 with
unit-norm loadings W_k (J_k x R), vip[k][j] = sqrt(J_k sum_r s_r W_k[j, r]^2 / sum_r s_r), so that sum_j vip[k][j]^2 = J_k.
"""
from __future__ import annotations

import numpy as np
import torch

from .diagnostics import _PROJECTION_READS, _host, _kept_training_blocks
from .storage import _as_torch_dtype, notes_of, reports_storage, to_device_read

_ONE_PASS = "one-pass MTTKRP (one read, nothing written)"


def sr_f_limit(I: int, level: float):
    """(limit, why): the F quantile that a selectivity ratio is compared with, for I training rows."""
    from scipy import stats

    if I <= 3:
        return float("nan"), f"I = {I} training rows <= 3"
    return float(stats.f.ppf(level, I - 2, I - 3)), None


def _ratios(a: np.ndarray, d: np.ndarray, s: np.ndarray, n: np.ndarray):
    """(tp_loading, explained, residual, sr), all (M, P), from the four sums (d: (M, P) or (M, 1))."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = (d > 0) & (n > 0)[None, :]
        dd = np.where(ok, d, 1.0)
        tp = np.where(ok, a / dd, np.nan)
        explained = np.where(ok, a * a / dd, np.nan)
        residual = np.where(ok, np.maximum(s[None, :] - explained, 0.0), np.nan)
        sr = explained / residual                          # 0 / 0 -> NaN, positive / 0 -> inf
    return tp, explained, residual, sr


def _mode_ratios(explained: np.ndarray, residual: np.ndarray, shape) -> list:
    """[(M, J_k) per mode k >= 1]: sum of explained over sum of residual over the cells of every slice, NaN cells skipped."""
    M = explained.shape[0]
    full = (M,) + tuple(shape)
    seen = np.isfinite(explained).reshape(full)
    e = np.where(seen, explained.reshape(full), 0.0)
    r = np.where(seen, residual.reshape(full), 0.0)
    out = []
    for k in range(1, len(full)):
        others = tuple(ax for ax in range(1, len(full)) if ax != k)
        es, rs, cnt = e.sum(axis=others), r.sum(axis=others), seen.sum(axis=others)
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(np.where(cnt > 0, es / rs, np.nan))
    return out


@reports_storage("importance_report_")
def selectivity_ratio(pls, X=None, level: float = 0.95, cells: bool = True, device: bool = True) -> dict:
    from .cmtf import ctPLS

    if not (0.0 < float(level) < 1.0):
        raise ValueError(f"level must be in (0, 1), got {level}")
    st = getattr(pls, "_state", None)
    if st is None:
        raise ValueError("selectivity_ratio needs a fitted tPLS or ctPLS")
    coupled = isinstance(pls, ctPLS)
    eng = pls._get_engine()
    dev = eng.be.device
    training = X is None
    with eng.device_ctx():
        if training:
            Xs = _kept_training_blocks(pls, coupled)
            if Xs is None:
                raise ValueError("the model was fitted with copy_X=False, so the training X was not kept: pass X")
            Xd = [to_device_read(x, blk.dtype or torch.float64, dev, pls=pls, entry="selectivity_cols") for x, blk in zip(Xs, st.blocks)]
            scores, pform, proj_reads = st.T, None, 0
            masked = [bool(blk.has_miss) for blk in st.blocks]
        else:
            Xs = list(X) if coupled else [X]
            if coupled and len(Xs) != pls.Xs_len:
                raise ValueError(f"Training Xs has {pls.Xs_len} blocks, while the new Xs has {len(Xs)}")
            Xd = [to_device_read(x, _as_torch_dtype(pls._dtype, x), dev, pls=pls, entry="selectivity_cols") for x in Xs]
            scores = pls._project_dev(Xd if coupled else Xd[0])           # transform's projection: shape checks, forms, bits
            pform = "sequential passes on private copies (f32 matrix precision)" if pls._mixed else eng.last_projection["form"]
            proj_reads = _PROJECTION_READS.get(pform)
            # only the one-pass form has shown the batch to be free of missing values (its NaN flag); anything else: the mask
            # (sharded: every rank must reduce the same sums whatever its own rows held)
            masked = [pform != _ONE_PASS or bool(getattr(eng.comm, "sharded", False))] * len(st.blocks)
        Bm = torch.from_numpy(np.ascontiguousarray(pls.coef_ @ pls.Y_factors[1].T, dtype=np.float64)).to(scores.device)
        Tau = (scores @ Bm).contiguous()                                   # I x M: the fitted response, not re-centred
        M = int(Tau.shape[1])
        res = eng.selectivity_cols(st, Xd, Tau, device=device, masked=masked)
        forms = list(eng.last_selectivity)
        notes_of(pls).declined(Xd, forms)
        # one all-reduce: [rows, sum_i tau^2 (M), then per block a, (d), s, n]
        head = torch.cat([Tau.new_tensor([float(Tau.shape[0])]), (Tau * Tau).sum(dim=0)])
        parts = [head] + [t.reshape(-1) for a, d, s, n in res for t in (a, d, s, n) if t is not None]
        flat = _host(eng.comm.allreduce(torch.cat(parts)))
        tau2 = flat[1:1 + M]
        at = 1 + M
        # I of the limit: the TRAINING rows over every rank (the rows of this call when they are the training rows)
        I_train = int(round(flat[0])) if training else int(round(eng.comm.allreduce(Tau.new_tensor([float(st.T.shape[0])])).item()))
        keys = ("sr", "explained", "residual", "tp_loading")
        out = {k: [] for k in keys + ("n_observed", "sr_mode")}
        for blk, (a, d, s, n) in zip(st.blocks, res):
            P = blk.A * blk.B
            ah = flat[at:at + M * P].reshape(M, P)
            at += M * P
            if d is not None:
                dh = flat[at:at + M * P].reshape(M, P)
                at += M * P
            else:
                dh = np.broadcast_to(tau2[:, None], (M, P))
            sh, nh = flat[at:at + P], flat[at + P:at + 2 * P]
            at += 2 * P
            tp, explained, residual, sr = _ratios(ah, dh, sh, nh)
            tail = tuple(blk.shape[1:])
            out["sr_mode"].append(_mode_ratios(explained, residual, tail))
            out["n_observed"].append(nh.reshape(tail).copy())
            if cells:
                for k, v in zip(keys, (sr, explained, residual, tp)):
                    out[k].append(v.reshape((M,) + tail))
        lim, lim_why = sr_f_limit(I_train, float(level))
    one = (lambda v: v) if coupled else (lambda v: v[0])
    ret = {k: one(out[k]) for k in (keys if cells else ()) + ("n_observed", "sr_mode")}
    ret.update(f_limit=lim, level=float(level))
    fallback = [f["why"] for f in forms if f["why"]]
    pls.importance_report_ = {
        "form": [f["form"] for f in forms],
        "why": "; ".join(sorted(set(fallback))) if fallback else None,
        "projection": pform,
        "rows": int(Tau.shape[0]),
        "training_rows": I_train,
        "x_reads": [None if proj_reads is None else proj_reads + 1 for _ in st.blocks],
        "masked": ["masked" if f["masked"] else "complete" for f in forms],
        "f_limit_why": lim_why,
        "f_limit_nominal": any(f["masked"] for f in forms),
    }
    return ret


def _vip_block(loadings, weights: np.ndarray, per_component: bool) -> list:
    R = weights.shape[0]
    out = []
    for W in loadings:
        W = np.asarray(W, dtype=np.float64)
        norm = np.sqrt((W * W).sum(axis=0))
        W2 = (W / np.where(norm > 0, norm, 1.0)) ** 2                      # unit-norm columns: sum_j vip^2 = J_k exactly
        J = W.shape[0]
        num = np.cumsum(W2 * weights[None, :], axis=1)                     # (J, R): prefix sums over the components
        den = np.cumsum(weights)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.where(den[None, :] > 0, np.sqrt(J * num / np.where(den > 0, den, 1.0)[None, :]), np.nan)
        out.append(np.ascontiguousarray(v.T) if per_component else v[:, R - 1].copy())
    return out


def vip_scores(pls, per_component: bool = False) -> dict:
    from .cmtf import ctPLS

    if getattr(pls, "_state", None) is None:
        raise ValueError("vip_scores needs a fitted tPLS or ctPLS")
    coupled = isinstance(pls, ctPLS)
    r2y = np.asarray(pls.R2Y, dtype=np.float64).reshape(-1)
    inc = np.diff(np.concatenate([[0.0], r2y]))
    weights = np.maximum(inc, 0.0)
    clipped = [{"component": int(r), "increment": float(inc[r])} for r in np.nonzero(inc < 0)[0]]
    why = None if weights.sum() > 0 else "sum of the R2Y increments is 0: no component explains Y"
    blocks = [f[1:] for f in pls.Xs_factors] if coupled else [pls.X_factors[1:]]
    vip = [_vip_block(L, weights, per_component) for L in blocks]
    pls.vip_report_ = {"clipped": clipped, "why": why, "per_component": bool(per_component)}
    return {"vip": vip if coupled else vip[0], "component_weights": weights, "clipped": clipped, "why": why}
