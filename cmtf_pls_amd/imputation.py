"""The X side of validation for incomplete tensors: `impute` fills the gaps of X from the fitted model, and
`get_q2x_heldout` scores the X model on entries it never saw.

With xhat_r = X_mean + the first r components of T W^T (W: the block's Khatri-Rao loadings, never materialised):
  impute           X with every non-finite entry replaced by xhat_R there (rounded once to the storage type), observed entries
                   untouched: one read of every block (cmtfpls_impute_*, ProjectionMixin.impute_rows)
  get_q2x_heldout  per repeat: hide a random share of the observed entries (cmtfpls_holdout_mask_*), refit a copy of the model on
                   what is left, and sum (x - xhat_r)^2 over the hidden entries against the ORIGINAL blocks for every r = 1..R in one
                   read (cmtfpls_heldout_resid_*):  Q2X_r = 1 - sum (x - xhat_r)^2 / sum (x - X_mean)^2, X_mean the refit's

THE HOLD-OUT RULE (include/cmtfpls.h): element e of block b (C order) is held out iff
  unit_open(philox4x32_10(counter = (offset + e) / 4, stream = 2 + b, key = seed).v[(offset + e) % 4]) < fraction.
No mask tensor exists on the device; `holdout_mask_host` restates the rule in NumPy for the torch form of the two passes (backends
without the kernels, R > 16, device=False) and for the tests.
"""
from __future__ import annotations

import contextlib
import io
from typing import Optional

import numpy as np
import torch

from .diagnostics import _PROJECTION_READS, _kept_training_blocks
from .storage import _as_torch_dtype, reports_storage, to_device_read

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _philox4x32_10(ctr: np.ndarray, stream: int, seed: int):
    """The four uint32 words of Philox4x32-10 for the uint64 counters `ctr` (csrc/philox.hpp: counter words (lo, hi, stream, 0))."""
    c0, c1 = (ctr & _LOW).astype(np.uint32), (ctr >> _S32).astype(np.uint32)
    c2, c3 = np.full(len(ctr), stream, dtype=np.uint32), np.zeros(len(ctr), dtype=np.uint32)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0.astype(np.uint64), _M1 * c2.astype(np.uint64)
        c0, c1, c2, c3 = ((p1 >> _S32).astype(np.uint32) ^ c1 ^ np.uint32(k0), (p1 & _LOW).astype(np.uint32),
                          (p0 >> _S32).astype(np.uint32) ^ c3 ^ np.uint32(k1), (p0 & _LOW).astype(np.uint32))
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def holdout_mask_host(first: int, n: int, seed: int, stream: int, fraction: float) -> np.ndarray:
    """(n,) bool: which of the global elements first .. first + n - 1 of Philox stream `stream` keyed by `seed` are held out."""
    seed = int(seed) & (2 ** 64 - 1)
    out = np.empty(n, dtype=bool)
    q0, q1 = first // 4, (first + n + 3) // 4
    chunk = 1 << 20                                              # quads per step: bounds the uint64 temporaries
    for q in range(q0, q1, chunk):
        ctr = np.arange(q, min(q + chunk, q1), dtype=np.uint64)
        u = (np.stack(_philox4x32_10(ctr, stream, seed), axis=1).reshape(-1).astype(np.float64) + 0.5) * 2.3283064365386963e-10
        lo, hi = max(4 * q, first), min(4 * (q + len(ctr)), first + n)
        out[lo - first: hi - first] = u[lo - 4 * q: hi - 4 * q] < fraction
    return out


def _fitted_state(pls, what: str):
    st = getattr(pls, "_state", None)
    if st is None:
        raise ValueError(f"{what} needs a fitted tPLS or ctPLS")
    return st


def _first_empty_row(X: torch.Tensor) -> Optional[int]:
    """The first sample of X without an observed (non-NaN) entry, None when every sample has one: what `BlockState.rowcnt` of a
    fit on X would hold a zero for -- asked BEFORE the fit, which divides by that count (missingvals.py:23-38) and need not
    finish on such a sample.  Row blocks of <= 256 MB; one more read of the masked copy."""
    I = X.shape[0]
    X2 = X.view(I, -1)
    step = max(1, (256 << 20) // max(X2.shape[1] * X2.element_size(), 1))
    for r0 in range(0, I, step):
        empty = torch.isnan(X2[r0:r0 + step]).all(dim=1)
        if bool(empty.any().item()):
            return r0 + int(torch.nonzero(empty)[0].item())
    return None


@reports_storage("imputation_report_")
def impute(pls, X=None, device: bool = True):
    from .cmtf import ctPLS

    st = _fitted_state(pls, "impute")
    coupled = isinstance(pls, ctPLS)
    eng = pls._get_engine()
    dev = eng.be.device
    training = X is None
    with eng.device_ctx():
        if training:
            Xs = _kept_training_blocks(pls, coupled)
            if Xs is None:
                raise ValueError("the model was fitted with copy_X=False, so the training X was not kept: pass X")
            dtypes = [blk.dtype or torch.float64 for blk in st.blocks]
        else:
            Xs = list(X) if coupled else [X]
            if len(Xs) != len(st.blocks):
                raise ValueError(f"Training Xs has {len(st.blocks)} blocks, while the new Xs has {len(Xs)}")
            dtypes = [_as_torch_dtype(pls._dtype, x) for x in Xs]
        Xd = [to_device_read(x, dt, dev, pls=pls, entry="impute") for x, dt in zip(Xs, dtypes)]
        if training:
            scores, pform, proj_reads = st.T, None, 0
        else:
            scores = pls._project_dev(Xd if coupled else Xd[0])              # transform's projection: shape checks, forms, bits
            pform = "sequential passes on private copies (f32 matrix precision)" if pls._mixed else eng.last_projection["form"]
            proj_reads = _PROJECTION_READS.get(pform)
        if scores.stride(1) != 1:
            scores = scores.contiguous()
        # a block uploaded or converted for this call is completed in place; the caller's own device tensor is only read
        private = [xd is not x for xd, x in zip(Xd, Xs)]
        done = eng.impute_rows(st, Xd, scores, inplace=private, device=device)
        forms = list(eng.last_imputation)
        out = []
        for x, (filled, _) in zip(Xs, done):
            if isinstance(x, torch.Tensor):
                out.append(filled if filled.device == x.device else filled.to(x.device))      # a tensor comes back where it came from
            else:
                xh = np.array(x, copy=True)                                  # observed entries: the input's own bits
                gap = ~np.isfinite(xh)
                xh[gap] = filled.cpu().numpy()[gap]
                out.append(xh)
    fallback = [f["why"] for f in forms if f["why"]]
    pls.imputation_report_ = {
        "form": "torch fallback" if fallback else ("fitted scores" if training else f"projection ({pform})") + " + imputation pass",
        "why": "; ".join(sorted(set(fallback))) if fallback else None,
        "projection": pform,
        "rows": int(scores.shape[0]),
        "imputed": [n for _, n in done],
        "in_place_on_private_copy": private,
        "x_reads": [None if proj_reads is None else proj_reads + 1 for _ in st.blocks],
    }
    return out if coupled else out[0]


@reports_storage("q2x_report_")
def get_q2x_heldout(pls, fraction: float = 0.1, n_repeats: int = 5, random_state=0, device: bool = True, tol: float = 1e-8,
                    max_iter: int = 100) -> dict:
    from .cmtf import ctPLS

    st = _fitted_state(pls, "get_q2x_heldout")
    if not (0.0 < float(fraction) < 1.0):
        raise ValueError(f"fraction must be in (0, 1), got {fraction}")
    if int(n_repeats) != n_repeats or n_repeats < 1:
        raise ValueError(f"n_repeats must be an integer >= 1, got {n_repeats}")
    eng = pls._get_engine()
    if getattr(eng.comm, "world", 1) > 1:
        raise NotImplementedError("get_q2x_heldout on a sharded model (comm of world size > 1) is not implemented")
    coupled = isinstance(pls, ctPLS)
    Xs = _kept_training_blocks(pls, coupled)
    if Xs is None:
        raise ValueError("the model was fitted with copy_X=False, so the training X was not kept: get_q2x_heldout refits from it")
    fraction, n_repeats = float(fraction), int(n_repeats)
    R, nb = st.n_components, len(st.blocks)
    dev = eng.be.device
    seeds = np.random.default_rng(random_state).integers(0, 2 ** 63, n_repeats)
    sums = np.empty((n_repeats, nb, R + 2))
    n_iter, forms = [], []
    with eng.device_ctx():
        Xd = [to_device_read(X, blk.dtype or torch.float64, dev, pls=pls, entry="q2x_heldout") for X, blk in zip(Xs, st.blocks)]      # read only
        for g, seed in enumerate(int(s) for s in seeds):
            masked = eng.holdout_copies(Xd, fraction, seed, device=device)
            for b, (m, _) in enumerate(masked):
                row = _first_empty_row(m)
                if row is not None:
                    raise ValueError(f"repeat {g} (seed {seed}): sample {row} has no observed entry left in block {b} after holding "
                                     f"out {fraction:g} of the entries; the masked score divides by that count")
            refit = pls.copy()
            refit._copy_X = False                                                # the masked copies are private: fitted in place
            with contextlib.redirect_stdout(io.StringIO()):                      # (the reference's "X has missing values" notice)
                refit.fit([m for m, _ in masked] if coupled else masked[0][0], pls.original_Y, tol=tol, max_iter=max_iter)
            del masked
            rst = refit._state
            res = eng.heldout_sums(rst, Xd, rst.T if rst.T.stride(1) == 1 else rst.T.contiguous(), fraction, seed, device=device)
            sums[g] = torch.stack(res).cpu().numpy()
            n_iter.append(list(refit.n_iter_))
            forms += list(eng.last_heldout)
    with np.errstate(divide="ignore", invalid="ignore"):
        q2x = 1.0 - sums[:, :, :R] / sums[:, :, R:R + 1]
        pooled = sums.sum(axis=1)
        q2x_all = 1.0 - pooled[:, :R] / pooled[:, R:R + 1]

        def spread(a):
            return np.std(a, axis=0, ddof=1) if n_repeats > 1 else np.full(a.shape[1:], np.nan)

        out = {"q2x": q2x, "q2x_all": q2x_all, "mean": q2x.mean(axis=0), "std": spread(q2x), "mean_all": q2x_all.mean(axis=0),
               "std_all": spread(q2x_all), "n_heldout": np.rint(sums[:, :, R + 1]).astype(np.int64), "seeds": seeds}
    fallback = [f["why"] for f in forms if f["why"]]
    masked_on_device = device and hasattr(eng.be, "holdout_mask")
    out["report"] = pls.q2x_report_ = {
        "form": "torch fallback" if fallback else "mask, refit in place, held-out residual pass (cmtfpls_holdout_mask + cmtfpls_heldout_resid)",
        "why": "; ".join(sorted(set(fallback))) if fallback else None,
        "mask": "cmtfpls_holdout_mask" if masked_on_device else "host restatement of the counter rule",
        "repeats": n_repeats, "blocks": nb, "fraction": fraction,
        "reads_of_original_per_repeat": 2,              # the masking copy and the residual pass; the refit reads its private copy
        "reads_of_masked_copy_per_repeat_before_refit": 1,   # the empty-sample guard (_first_empty_row), then the refit's own reads
        "n_iter": n_iter,
    }
    return out
