"""Projection of new samples, reconstruction and the literal R2X: the engine's `transform` / `predict` side
(reference cmtf_pls/tpls.py:122-189, cmtf.py:142-237), as a mixin of `NipalsEngine`.

Forms, in the order they are tried (`NipalsEngine.last_projection` records which one ran):
  one-pass MTTKRP on the caller's uncentred rows (one read, nothing written)            _project_one_pass / project_readonly
  + the masked sequence for ONLY the incomplete samples, in registers or on compact copies   project_readonly
  the sequential project-and-deflate passes on private copies (the reference's loop)     _project
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import torch

from .state import BlockState, FitState
from .storage import HALF_DTYPES, HALF_ENTRIES, dtype_name, half_route, read_dtype


class ProjectionMixin:
    def project(self, state: FitState, Xs: List[torch.Tensor], one_pass: bool = True, mixed: bool = False) -> torch.Tensor:
        """Sequential project-and-deflate of new samples (tpls.py:128-142; cmtf.py:143-177).
        Xs are device copies and are consumed.  Rows are independent: no communication."""
        with self.device_ctx():
            return self._project(state, Xs, one_pass, mixed)

    def project_readonly(self, state: FitState, Xs: List[torch.Tensor]) -> Optional[torch.Tensor]:
        """Scores of new samples from ONE read of every block, the blocks neither copied nor written: the MTTKRP runs on
        the UNCENTRED rows and the centring `X - X_mean` (tpls.py:130,153; cmtf.py:150,187) is applied to its I x R output,
        (X - 1 mean^T) W = X W - 1 (mean^T W)^T.

        Samples are independent (tpls.py:128-142 works row by row).  A missing value in a sample shows as a NaN in its row of
        the MTTKRP output; such samples take the reference's masked sequence -- centre, then R times score with the per-row
        rescale, average the coupled blocks' scores and deflate (missingvals.py:23-38, cmtf.py:143-177) -- while the complete
        samples of the same batch KEEP their one-pass scores (`EngineOptions.project_split_rows`): in registers from one
        more read of just those rows (one block, or two coupled blocks in one workgroup), else on compact private copies of
        those rows through the sequential passes (any number of blocks, any storage types).  A strided sample of the batch
        is probed first: when most samples are incomplete the MTTKRP attempt would be a wasted read and every row goes
        through the masked sequence directly; when max|column mean| / spread exceeds `EngineOptions.project_raw_max_offset`
        the one-pass form would lose digits to cancellation, and the rows are centred first (in registers, else None).

        None when no read-only form applies (a training column without observations, a shape neither the MTTKRP nor the
        rows-in-registers kernel takes): the caller then runs `project` on private copies.  `last_projection` records the
        form taken."""
        with self.device_ctx():
            be = self.be
            nb, I, R = len(state.blocks), Xs[0].shape[0], state.n_components
            rep = self.last_projection = {"rows": int(I), "blocks": nb, "form": "sequential passes on private copies", "why": None}
            if any(bool(torch.isnan(blk.mean).any().item()) for blk in state.blocks):
                rep["why"] = "a training column without observations (NaN mean)"
                return None
            can_rows = (nb <= 2 and hasattr(be, "project_rows") and all(X.is_contiguous() for X in Xs)
                        and (nb == 1 or hasattr(be, "project_rows2")))
            ops = None

            def in_registers(out, rows):
                nonlocal ops
                ops = ops or [self._kr_operands(blk, R) for blk in state.blocks]
                if nb == 1:
                    blk = state.blocks[0]
                    return be.project_rows(Xs[0].view(I, -1), blk.A, blk.B, ops[0][0], ops[0][1], blk.mean, out, rows=rows)
                return be.project_rows2([X.view(I, -1) for X in Xs], [b.A for b in state.blocks], [b.B for b in state.blocks],
                                        [o[0].contiguous() for o in ops], [o[1].contiguous() for o in ops],
                                        [b.mean for b in state.blocks], out, rows=rows)

            # probe <= 256 samples strided over the batch: mostly incomplete -> skip the MTTKRP attempt (it would be one wasted
            # read); badly offset data -> centre first (the one-pass form below works on the uncentred rows by cancellation)
            frac, ratio = self._projection_probe(state, Xs) if I > 0 else (0.0, 0.0)
            rep["offset_ratio"] = ratio
            if can_rows:
                rep["probe_incomplete_fraction"] = frac
            if not ratio <= self.opt.project_raw_max_offset:
                rep["why"] = (f"max|column mean| / spread = {ratio:.3g} > {self.opt.project_raw_max_offset:g}: the one-pass form on "
                              "uncentred rows would lose digits; rows centred first")
                if can_rows:
                    out = be.empty(I, R)
                    if in_registers(out, None) is not None:
                        rep["form"] = "masked sequence, every row in registers (one read)"
                        return out
                return None
            if can_rows and frac > 0.5:
                out = be.empty(I, R)
                if in_registers(out, None) is not None:
                    rep.update(form="masked sequence, every row in registers (one read)", why="most samples have a missing value")
                    return out
            flag = torch.zeros(1, dtype=torch.int32, device=be.device)
            scores = self._project_one_pass(state, Xs, False, centred=False, nan_flag=flag)
            if scores is not None and int(flag.item()) == 0:
                rep.update(form="one-pass MTTKRP (one read, nothing written)")
                return scores
            rows = None
            if scores is not None and self.opt.project_split_rows:
                rows = torch.nonzero(torch.isnan(scores).any(dim=1)).view(-1).contiguous()    # samples with a missing value somewhere
                rep["incomplete_rows"] = int(rows.numel())
                if rows.numel() == I:
                    rows = None
            if can_rows:
                out = scores if rows is not None else be.empty(I, R)
                if in_registers(out, rows) is not None:
                    # scores None: the MTTKRP declined the shape, whether or not the batch has a missing value
                    why = "missing values in the batch" if scores is not None else (
                        f"one-pass MTTKRP declined: R = {R} > 32" if R > 32 else "one-pass MTTKRP declined: loadings beyond its LDS")
                    rep.update(form=("one-pass MTTKRP for the complete samples + masked sequence in registers for the incomplete ones"
                                     if rows is not None else "masked sequence, every row in registers (one read)"),
                               why=why)
                    return out
            if rows is not None:
                # any number of blocks / storage types / trailing extents: compact private copies of the incomplete samples only
                sub = [X.index_select(0, rows) for X in Xs]
                scores.index_copy_(0, rows, self._project(state, sub, one_pass=False, mixed=False))
                rep.update(form="one-pass MTTKRP for the complete samples + sequential passes on copies of the incomplete ones",
                           why="missing values in the batch; shape outside the rows-in-registers kernel")
                return scores
            rep["why"] = ("shape outside the MTTKRP and the rows-in-registers kernel" if scores is None
                          else "every sample has a missing value; shape outside the rows-in-registers kernel")
            return None

    def project_half(self, state: FitState, Xs: List[torch.Tensor]) -> Tuple[Optional[torch.Tensor], Optional[str]]:
        """A batch with 16-bit blocks (bfloat16 / float16 storage): (scores, None) from the one-pass MTTKRP on the blocks as they
        are -- one read, converted on load, nothing copied or written -- else (None, why): no other projection form reads 16-bit
        rows, so the caller upcasts the batch to float32 (exact) and takes the forms of `project_readonly` / `project`."""
        with self.device_ctx():
            be = self.be
            nb, I = len(state.blocks), Xs[0].shape[0]
            rep = self.last_projection = {"rows": int(I), "blocks": nb, "form": "sequential passes on private copies", "why": None}
            if not half_route(self, None, HALF_ENTRIES["projection"])[0]:
                return None, "the backend has no 16-bit MTTKRP"
            if any(bool(torch.isnan(blk.mean).any().item()) for blk in state.blocks):
                return None, "a training column without observations (NaN mean)"
            frac, ratio = self._projection_probe(state, Xs) if I > 0 else (0.0, 0.0)
            rep["offset_ratio"] = ratio
            if not ratio <= self.opt.project_raw_max_offset:
                return None, (f"max|column mean| / spread = {ratio:.3g} > {self.opt.project_raw_max_offset:g}: the one-pass form on "
                              "uncentred rows would lose digits")
            if frac > 0.0:
                return None, "rows with missing values in the batch"
            flag = torch.zeros(1, dtype=torch.int32, device=be.device)
            scores = self._project_one_pass(state, Xs, False, centred=False, nan_flag=flag)
            if scores is None:
                return None, "shape outside the one-pass MTTKRP"
            if int(flag.item()) != 0:
                return None, "rows with missing or non-finite values in the batch"
            rep.update(form="one-pass MTTKRP (one read, nothing written)",
                       storage=[dtype_name(X.dtype) for X in Xs])
            return scores, None

    @staticmethod
    def _projection_probe(state: FitState, Xs: List[torch.Tensor]) -> Tuple[float, float]:
        """(fraction of <= 256 samples strided over the batch with a missing value in some block, max over blocks of
        max|column mean| / rms spread of the observed centred entries of <= 256 strided samples, at most 65536 entries per
        block so that the float64 temporaries stay small next to X).  The one-pass form computes X W - 1 (mean^T W)^T with
        error ~ 1e-16 * that ratio relative to the scores (DESIGN "Conditioning guard").  Local to this rank: rows are
        independent, a transform communicates nothing.  One host transfer."""
        I = Xs[0].shape[0]
        bad, stats = None, []
        for blk, X in zip(state.blocks, Xs):
            X2 = X.view(I, -1)
            r = torch.isnan(X2[:: max(1, I // 256)][:256]).any(dim=1)
            bad = r if bad is None else (bad | r)
            k = max(1, min(256, (1 << 16) // max(X2.shape[1], 1)))
            d = X2[:: max(1, I // k)][:k].to(torch.float64) - blk.mean
            miss = torch.isnan(d)
            d = d.masked_fill_(miss, 0.0)
            stats += [(d * d).sum(), (~miss).sum().to(torch.float64), blk.mean.abs().max()]
        vals = torch.stack(stats + [bad.to(torch.float64).mean()]).cpu().tolist()
        worst = 0.0
        for ssq, cnt, top in zip(vals[0:-1:3], vals[1:-1:3], vals[2:-1:3]):
            if top == 0.0 or cnt == 0.0:                 # nothing to cancel / no observed entry to measure the spread on
                continue
            ratio = top / math.sqrt(ssq / cnt) if ssq > 0.0 else float("inf")
            worst = ratio if not ratio <= worst else worst
        return vals[-1], worst

    def _project(self, state: FitState, Xs: List[torch.Tensor], one_pass: bool, mixed: bool) -> torch.Tensor:
        be = self.be
        R = state.n_components
        I = Xs[0].shape[0]
        rowcnts = []
        for blk, X in zip(state.blocks, Xs):
            X2 = X.view(I, -1)
            rowcnt, _ = be.center(X2, blk.mean, True)
            miss = bool((rowcnt.min() < X2.shape[1] - 0.5).item()) or bool(torch.isnan(blk.mean).any().item())
            rowcnts.append(rowcnt if miss else None)
        if one_pass and all(rc is None for rc in rowcnts):
            scores = self._project_one_pass(state, Xs, mixed)
            if scores is not None:
                return scores
        scores = be.zeros(I, R)
        nb = len(Xs)
        Ts = be.empty(nb, I)
        t = be.empty(I)
        for a in range(R):
            was, wbs = [], []
            for blk in state.blocks:
                if len(blk.shape) == 2:
                    was.append(torch.ones(1, dtype=torch.float64, device=t.device))
                    wbs.append(blk.loadings[0][:, a].contiguous())
                else:
                    was.append(blk.loadings[0][:, a].contiguous())
                    wbs.append(self.kron_trailing([L[:, a] for L in blk.loadings[1:]], be.empty(blk.B)))
            if nb == 1:
                blk, X2 = state.blocks[0], Xs[0].view(I, -1)
                if be.score_deflate(X2, blk.A, blk.B, was[0], wbs[0], rowcnts[0], t) is None:
                    be.score(X2, blk.A, blk.B, was[0], wbs[0], rowcnts[0], t)
                    be.deflate(X2, blk.A, blk.B, t, was[0], wbs[0])
            else:
                for b, (blk, X) in enumerate(zip(state.blocks, Xs)):
                    be.score(X.view(I, -1), blk.A, blk.B, was[b], wbs[b], rowcnts[b], Ts[b])
                be.scores_mean(Ts, t)
                for b, (blk, X) in enumerate(zip(state.blocks, Xs)):
                    be.deflate(X.view(I, -1), blk.A, blk.B, t, was[b], wbs[b])
            scores[:, a].copy_(t)
        if nb > 1 and any(rc is not None for rc in rowcnts):
            # coupled blocks: a sample whose row is empty in ONE block gets a NaN average (cmtf.py:155,206); the reference's
            # mask comes from the input, so the NaN-deflated rows of its other blocks give NaN scores from then on, while the
            # masked score kernels read those entries as missing: restore the reference's outcome on the I x R result
            scores.masked_fill_(torch.isnan(scores).cumsum(dim=1) > 0, float("nan"))
        return scores

    def _kr_operands(self, blk: BlockState, R: int):
        """(WA, WB): the block's loading matrices as the factored Khatri-Rao operand the matrix kernels take,
        W[c, r] = WA[c / B, r] * WB[c % B, r] (a matrix block: WA = ones; order >= 4: WB = column-wise Kronecker
        product of the trailing modes' loadings, formed on the device)."""
        be = self.be
        loads = blk.loadings
        if len(blk.shape) == 2:
            WA = be.empty(1, R)
            WA.fill_(1.0)
            return WA, loads[0]
        WB = loads[1]
        for L in loads[2:]:
            WB = be.khatri_rao(WB, L)
        return loads[0], WB

    def reconstruct(self, state: FitState, block: int = 0, rows: Optional[slice] = None,
                    dtype: Optional[torch.dtype] = None) -> Optional[torch.Tensor]:
        """Rows of factors_to_tensor(X_factors) + X_mean (util.py:18-20 with tpls.py:188-189 / cmtf.py:233-237) for
        one block, formed on the GPU in `dtype` (default: the block's storage type; the estimators ask for float64 when
        they return a host array, as the reference does): Xhat = T (W_1 (.) W_2 (.) ...)^T + mean with the Khatri-Rao
        operand never materialised (cmtfpls_recon_*).  None when the backend / shape has no device form (the caller
        falls back to the host einsum)."""
        be = self.be
        if not hasattr(be, "recon"):
            return None
        blk = state.blocks[block]
        with self.device_ctx():
            T = state.T if rows is None else state.T[rows]
            WA, WB = self._kr_operands(blk, state.n_components)
            out = be.empty(T.shape[0], blk.A * blk.B, dtype=dtype or read_dtype(blk.dtype) or torch.float64)
            if T.shape[0] == 0 or be.recon(T, WA, WB, blk.mean, out) is None:
                return None
            return out.view((T.shape[0],) + tuple(blk.shape[1:]))

    def r2x_literal(self, state: FitState, X: torch.Tensor, block: int = 0) -> Optional[float]:
        """calcR2X(X - X_mean, factors_to_tensor(X_factors)) (util.py:7-15 as called at tpls.py:115-117) for the rows
        X (device, storage type, UNCENTRED, same rows as state.T) in one read of X, the reconstruction never
        materialised (cmtfpls_recon_r2_*).  None when the backend / shape has no device form."""
        be = self.be
        if not hasattr(be, "recon_r2"):
            return None
        blk = state.blocks[block]
        with self.device_ctx():
            WA, WB = self._kr_operands(blk, state.n_components)
            out = be.recon_r2(X.view(X.shape[0], -1), state.T, WA, WB, blk.mean)
            if out is None:
                return None
            res, ssq = self.comm.allreduce(out).cpu().tolist()
            return 1.0 - res / ssq

    @staticmethod
    def _fallback_block(X2: torch.Tensor) -> torch.Tensor:
        """The block as the torch fallbacks read it: a 16-bit block (read in place under EngineOptions.half_diagnostics, its kernel
        declined) as an exact float32 upcast of that block; anything else as it is."""
        return X2.to(torch.float32) if X2.dtype in HALF_DTYPES else X2

    def residual_rows(self, state: FitState, Xs: List[torch.Tensor], T: torch.Tensor, want_cols: bool = True,
                      device: bool = True) -> List[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
        """Per block, for the rows Xs[b] (device, storage type, UNCENTRED, read only) with scores T (I x R):
        (rows (I, 3) = [sum e^2, sum x^2, observed entries] per sample, cols (P, 2) = [sum e^2, sum x^2] per variable or
        None), x = X - mean over the finite entries (the calcR2X mask, util.py:7-15), e = x - T W_b^T.  One read of every
        block through cmtfpls_resid_rows_*; where the backend declines (R > 16, no such kernel, device=False) the same sums
        from torch ops on row blocks of <= 256 MB.  `last_residual` records, per block, the form that ran and why."""
        out, self.last_residual = self._stream_blocks(
            state, Xs, "resid_rows", "residual pass (cmtfpls_resid_rows)", device,
            kernel=lambda blk, X2, WA, WB, b: self.be.resid_rows(X2, T, WA, WB, blk.mean, want_cols),
            fallback=lambda blk, X2, WA, WB, b: self._residual_rows_torch(X2, T, WA, WB, blk.mean, want_cols),
            declined=lambda blk: f"R = {state.n_components} > 16: outside cmtfpls_resid_rows")
        return out

    def _stream_blocks(self, state: FitState, Xs: List[torch.Tensor], entry: str, form: str, device: bool, kernel, fallback,
                       declined=None, as_stored: bool = False, operands: bool = True, rows: Optional[int] = None):
        """The per-block loop of the streaming passes: (results, per-block {"form", "why"} records).  Block b as X2 (I, P) goes to
        `kernel(blk, X2, WA, WB, b)`, the backend's `entry`, unless `_streaming_form` rules it out or there is no row (`rows`, default
        I); a None from it is recorded as `declined(blk)`.  What the kernel did not do, `fallback(blk, X2, WA, WB, b)` does in torch ops.
        as_stored: the pass depends on the block's element order (the hold-out rule, a write in place), so the block must be
        contiguous (`view` raises otherwise), the operands are made contiguous and the fallback reads the stored block; otherwise any
        strides go (`reshape`) and the fallback reads `_fallback_block`.  operands False: a pass without loadings (WA = WB = None)."""
        R = state.n_components
        out, forms = [], []
        with self.device_ctx():
            for b, (blk, X) in enumerate(zip(state.blocks, Xs)):
                I = X.shape[0]
                X2 = X.view(I, -1) if as_stored else X.reshape(I, -1)
                WA, WB = self._kr_operands(blk, R) if operands else (None, None)
                if as_stored:
                    WA, WB = WA.contiguous(), WB.contiguous()
                why = self._streaming_form(entry, device)
                res = None
                if why is None and (I if rows is None else rows) > 0:
                    res = kernel(blk, X2, WA, WB, b)
                    if res is None and declined is not None:
                        why = declined(blk)
                if res is None:
                    res = fallback(blk, X2 if as_stored else self._fallback_block(X2), WA, WB, b)
                out.append(res)
                forms.append({"form": "torch fallback" if why else form, "why": why})
        return out, forms

    @staticmethod
    def _kr_dense(WA: torch.Tensor, WB: torch.Tensor, P: int) -> torch.Tensor:
        """W (P, R) of `_kr_operands`, materialised: for the torch fallbacks."""
        return (WA[:, None, :] * WB[None, :, :]).reshape(P, -1)

    @staticmethod
    def _row_step(P: int) -> int:
        """Rows of a fallback's row block: <= 256 MB of float64."""
        return max(1, (256 << 20) // max(P * 8, 1))

    @classmethod
    def _residual_rows_torch(cls, X2: torch.Tensor, T: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor, mean: Optional[torch.Tensor],
                             want_cols: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        I, P = X2.shape
        dev = T.device
        W = cls._kr_dense(WA, WB, P)
        rows = torch.empty(I, 3, dtype=torch.float64, device=dev)
        cols = torch.zeros(P, 2, dtype=torch.float64, device=dev) if want_cols else None
        step = cls._row_step(P)
        for r0 in range(0, I, step):
            x = X2[r0:r0 + step].to(device=dev, dtype=torch.float64)
            if mean is not None:
                x = x - mean
            fin = torch.isfinite(x)
            e = torch.where(fin, x - T[r0:r0 + step] @ W.T, 0.0)
            x = torch.where(fin, x, 0.0)
            e2, x2 = e * e, x * x
            rows[r0:r0 + step, 0] = e2.sum(dim=1)
            rows[r0:r0 + step, 1] = x2.sum(dim=1)
            rows[r0:r0 + step, 2] = fin.sum(dim=1).to(torch.float64)
            if want_cols:
                cols[:, 0] += e2.sum(dim=0)
                cols[:, 1] += x2.sum(dim=0)
        return rows, cols

    def selectivity_cols(self, state: FitState, Xs: List[torch.Tensor], Tau: torch.Tensor, device: bool = True,
                         masked: Optional[List[bool]] = None) -> List[tuple]:
        """Per block, for the rows Xs[b] (device, storage type, UNCENTRED, read only) and the fitted response Tau (I x M):
        (a (M, P), d (M, P) or None, s (P,), n (P,)) with x = X - mean and o = isfinite(x) (the calcR2X mask of `residual_rows`):
        a = sum_i o x tau, d = sum_i o tau^2, s = sum_i o x^2, n = sum_i o.  masked[b] False (default: the block's has_miss) declares
        the rows of block b complete: o = 1, d is None (it is sum_i tau^2 for every column) and a missing value shows as a NaN.
        One read of every block through cmtfpls_selectivity_cols_*; where the backend has no such kernel, and for device=False,
        the same sums from torch ops on row blocks of <= 256 MB.  `last_selectivity` records, per block, the form and why."""
        flags = [bool(blk.has_miss) for blk in state.blocks] if masked is None else [bool(f) for f in masked]
        with self.device_ctx():
            if Tau.stride(1) != 1:
                Tau = Tau.contiguous()
            out, forms = self._stream_blocks(
                state, Xs, "selectivity_cols", "selectivity pass (cmtfpls_selectivity_cols)", device, operands=False,
                kernel=lambda blk, X2, WA, WB, b: self.be.selectivity_cols(X2, Tau, blk.mean, flags[b]),
                fallback=lambda blk, X2, WA, WB, b: self._selectivity_cols_torch(X2, Tau, blk.mean, flags[b]))
        self.last_selectivity = [dict(f, masked=msk) for f, msk in zip(forms, flags)]
        return out

    @classmethod
    def _selectivity_cols_torch(cls, X2: torch.Tensor, Tau: torch.Tensor, mean: Optional[torch.Tensor], masked: bool):
        I, P = X2.shape
        M = Tau.shape[1]
        dev = Tau.device
        a = torch.zeros(M, P, dtype=torch.float64, device=dev)
        d = torch.zeros(M, P, dtype=torch.float64, device=dev) if masked else None
        s, n = (torch.zeros(P, dtype=torch.float64, device=dev) for _ in range(2))
        step = cls._row_step(P)
        for r0 in range(0, I, step):
            x = X2[r0:r0 + step].to(device=dev, dtype=torch.float64)
            tau = Tau[r0:r0 + step]
            if mean is not None:
                x = x - mean
            if masked:
                fin = torch.isfinite(x)
                x = torch.where(fin, x, 0.0)
                o = fin.to(torch.float64)
                d += (tau * tau).T @ o
                n += o.sum(dim=0)
            else:
                n += float(x.shape[0])
            a += tau.T @ x
            s += (x * x).sum(dim=0)
        return a, d, s, n

    def _streaming_form(self, kernel: str, device: bool) -> Optional[str]:
        """Why the streaming kernel `kernel` of the backend is NOT taken before it is tried (None: try it)."""
        if not device:
            return "device pass switched off"
        if not hasattr(self.be, kernel):
            return f"backend has no {kernel} kernel"
        return None

    def impute_rows(self, state: FitState, Xs: List[torch.Tensor], T: torch.Tensor, inplace=False,
                    device: bool = True) -> List[Tuple[torch.Tensor, int]]:
        """Per block, (the rows Xs[b] with every non-finite entry replaced by X_mean + T W_b^T there, rounded once to the storage type,
        the number of entries replaced); finite entries keep their bits.  Xs[b]: contiguous, storage type, UNCENTRED, scores T
        (I x R).  inplace (a bool, or one per block): Xs[b] itself is completed (a private copy of the caller's) and returned.  One read of every block through
        cmtfpls_impute_* (in place: only the vectors that held a gap are written); where the backend declines (R > 16, no such
        kernel, device=False) the same from torch ops on row blocks of <= 256 MB.  `last_imputation` records, per block, the form
        that ran and why."""
        flags = [bool(inplace)] * len(Xs) if isinstance(inplace, bool) else [bool(f) for f in inplace]

        def complete(step, blk, X2, WA, WB, b):            # a declining kernel has not touched dst
            dst = X2 if flags[b] else torch.empty_like(X2)
            count = step(X2, dst, T, WA, WB, blk.mean)
            return None if count is None else (dst, count)

        done, self.last_imputation = self._stream_blocks(
            state, Xs, "impute", "imputation pass (cmtfpls_impute)", device, as_stored=True,
            kernel=lambda *block: complete(self.be.impute, *block),
            fallback=lambda *block: complete(self._impute_rows_torch, *block),
            declined=lambda blk: f"R = {state.n_components} > 16: outside cmtfpls_impute")
        return [(dst.view(X.shape), int(round(float(count.item())))) for X, (dst, count) in zip(Xs, done)]

    @classmethod
    def _impute_rows_torch(cls, X2: torch.Tensor, dst: torch.Tensor, T: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor,
                           mean: Optional[torch.Tensor]) -> torch.Tensor:
        I, P = X2.shape
        W = cls._kr_dense(WA, WB, P)
        count = torch.zeros(1, dtype=torch.float64, device=T.device)
        step = cls._row_step(P)
        for r0 in range(0, I, step):
            x = X2[r0:r0 + step]
            gap = ~torch.isfinite(x)
            xhat = T[r0:r0 + step] @ W.T
            if mean is not None:
                xhat = xhat + mean
            dst[r0:r0 + step] = torch.where(gap, xhat.to(x.dtype), x)
            count += gap.sum()
        return count

    def holdout_copies(self, Xs: List[torch.Tensor], fraction: float, seed: int, device: bool = True,
                       offsets: Optional[List[int]] = None) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """Per block, (a private copy of Xs[b] whose held-out entries are NaN, counts (2,) = [entries newly hidden, finite entries
        left]).  The hold-out rule is a pure function of (seed, stream 2 + b, offsets[b] + element index) (include/cmtfpls.h;
        imputation.holdout_mask_host restates it): one read and one write through cmtfpls_holdout_mask_*, else the same mask
        from the host restatement."""
        from .imputation import holdout_mask_host

        be = self.be
        out = []
        with self.device_ctx():
            for b, X in enumerate(Xs):
                off = int(offsets[b]) if offsets is not None else 0
                dst = torch.empty_like(X)
                if device and hasattr(be, "holdout_mask") and X.numel() > 0:
                    counts = be.holdout_mask(X, dst, fraction, seed, 2 + b, off)
                else:
                    held = torch.from_numpy(holdout_mask_host(off, X.numel(), seed, 2 + b, fraction)).to(X.device).view(X.shape)
                    fin = torch.isfinite(X)
                    dst.copy_(torch.where(held, torch.full_like(X, float("nan")), X))
                    counts = torch.stack([(held & fin).sum(), (~held & fin).sum()]).to(torch.float64)
                out.append((dst, counts))
        return out

    def heldout_sums(self, state: FitState, Xs: List[torch.Tensor], T: torch.Tensor, fraction: float, seed: int, device: bool = True,
                     offsets: Optional[List[int]] = None) -> List[torch.Tensor]:
        """Per block, (R + 2,) f64 = [sum (x - xhat_r)^2 for r = 1..R, sum (x - mean)^2, count] over the entries of the ORIGINAL rows
        Xs[b] (contiguous, storage type, UNCENTRED, read only) that the hold-out rule of `holdout_copies` (same fraction, seed,
        offsets) hides AND that are finite; xhat_r = X_mean + the first r components of T W_b^T with the scores T (I x R) of `state`.
        One read of every block through cmtfpls_heldout_resid_*, no mask tensor; where the backend declines (R > 16, no such
        kernel, device=False) the same sums from torch ops on row blocks of <= 256 MB with the mask of the host restatement.
        `last_heldout` records, per block, the form that ran and why."""
        def sums(step, blk, X2, WA, WB, b):
            return step(X2, T, WA, WB, blk.mean, fraction, seed, 2 + b, int(offsets[b]) if offsets is not None else 0)

        out, self.last_heldout = self._stream_blocks(
            state, Xs, "heldout_resid", "held-out residual pass (cmtfpls_heldout_resid)", device, as_stored=True,
            kernel=lambda *block: sums(self.be.heldout_resid, *block),
            fallback=lambda *block: sums(self._heldout_sums_torch, *block),
            declined=lambda blk: f"R = {state.n_components} > 16: outside cmtfpls_heldout_resid")
        return out

    @classmethod
    def _heldout_sums_torch(cls, X2: torch.Tensor, T: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor, mean: Optional[torch.Tensor],
                            fraction: float, seed: int, stream: int, offset: int) -> torch.Tensor:
        from .imputation import holdout_mask_host

        I, P = X2.shape
        R = T.shape[1]
        dev = T.device
        W = cls._kr_dense(WA, WB, P)
        out = torch.zeros(R + 2, dtype=torch.float64, device=dev)
        step = cls._row_step(P)
        for r0 in range(0, I, step):
            x = X2[r0:r0 + step].to(device=dev, dtype=torch.float64)
            held = torch.from_numpy(holdout_mask_host(offset + r0 * P, x.numel(), seed, stream, fraction)).to(dev).view(x.shape)
            use = held & torch.isfinite(x)
            acc = torch.zeros_like(x) if mean is None else mean.expand_as(x).clone()
            d = torch.where(use, x - acc, 0.0)
            out[R] += (d * d).sum()
            out[R + 1] += use.sum()
            for r in range(R):
                acc += torch.outer(T[r0:r0 + step, r], W[:, r])
                d = torch.where(use, x - acc, 0.0)
                out[r] += (d * d).sum()
        return out

    def contribution_rows(self, state: FitState, Xs: List[torch.Tensor], T: torch.Tensor, H: torch.Tensor,
                          rows: Optional[torch.Tensor] = None, device: bool = True) -> List[tuple]:
        """Per block, for n samples with scores T and T^2 directions H (both n x R; H already divided by the number of blocks):
        (speA (n, A) or None for a matrix block, speB (n, B), t2A, t2B), the sums over the other mode of e^2 and d, where
        e = x - T W_b^T and d = x * (H W_b^T) over the finite entries of x = X - mean.  Sample i is row rows[i] of Xs[b] (int64;
        None: row i); only those rows of Xs[b] (device, storage type, UNCENTRED, read only) are read, once, through
        cmtfpls_contrib_rows_*.  Where the backend declines (R > 16, loadings beyond the LDS, no such kernel, device=False) the same
        sums from torch ops on row blocks of <= 256 MB.  `last_contribution` records, per block, the form that ran and why."""
        R = state.n_components
        out, self.last_contribution = self._stream_blocks(
            state, Xs, "contrib_rows", "contribution pass (cmtfpls_contrib_rows)", device, rows=T.shape[0],
            kernel=lambda blk, X2, WA, WB, b: self.be.contrib_rows(X2, T, H, WA.contiguous(), WB.contiguous(), blk.mean, rows),
            fallback=lambda blk, X2, WA, WB, b: self._contribution_rows_torch(X2, T, H, WA, WB, blk.mean, rows),
            declined=lambda blk: (f"R = {R} > 16: outside cmtfpls_contrib_rows" if R > 16 else
                                  f"first mode of {blk.A} slices x R = {R}: 2 A (R + 1) doubles beyond the LDS of cmtfpls_contrib_rows"))
        return out

    @classmethod
    def contribution_cells(cls, X2: torch.Tensor, T: torch.Tensor, H: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor,
                           mean: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """(e, d), both (n, P) float64: the signed residual and the T^2 contribution of every cell of the rows X2 (0 where
        x = X2 - mean is not finite), W materialised.  For a handful of rows; the callers bound n * P."""
        W = cls._kr_dense(WA, WB, X2.shape[1])
        x = X2.to(device=T.device, dtype=torch.float64)
        if mean is not None:
            x = x - mean
        fin = torch.isfinite(x)
        e = torch.where(fin, x - T @ W.T, 0.0)
        d = torch.where(fin, x * (H @ W.T), 0.0)
        return e, d

    @classmethod
    def _contribution_rows_torch(cls, X2: torch.Tensor, T: torch.Tensor, H: torch.Tensor, WA: torch.Tensor, WB: torch.Tensor,
                                 mean: Optional[torch.Tensor], rows: Optional[torch.Tensor]):
        n, P = T.shape[0], X2.shape[1]
        A, B = WA.shape[0], WB.shape[0]
        dev = T.device
        speB, t2B = (torch.empty(n, B, dtype=torch.float64, device=dev) for _ in range(2))
        speA, t2A = (torch.empty(n, A, dtype=torch.float64, device=dev) for _ in range(2)) if A > 1 else (None, None)
        step = cls._row_step(P)
        for r0 in range(0, n, step):
            sl = slice(r0, r0 + step)
            e, d = cls.contribution_cells(X2[sl] if rows is None else X2.index_select(0, rows[sl].to(X2.device)), T[sl], H[sl], WA, WB, mean)
            e2 = (e * e).view(-1, A, B)
            d = d.view(-1, A, B)
            speB[sl], t2B[sl] = e2.sum(dim=1), d.sum(dim=1)
            if A > 1:
                speA[sl], t2A[sl] = e2.sum(dim=2), d.sum(dim=2)
        return speA, speB, t2A, t2B

    def t2_direction_solve(self, state: FitState, Gd: torch.Tensor) -> torch.Tensor:
        """Rows h_i = U^-1 g_i of Gd (n x R), U = I + triu(mean_b W_b^T W_b, 1): the unit upper-triangular matrix of
        `_project_one_pass` (T U = mean_b X_b W_b), so that t_i^T g_i = mean_b x_ib^T W_b h_i over a complete row."""
        be = self.be
        R = state.n_components
        nb = len(state.blocks)
        with self.device_ctx():
            Gs = be.empty(nb, R * R)
            for b, blk in enumerate(state.blocks):
                for m, L in enumerate(blk.loadings):
                    be.kr_gram(L, Gs[b], first=(m == 0))
            Gbar = Gs.view(nb, R, R).mean(dim=0)
            U = torch.eye(R, dtype=torch.float64, device=Gd.device) + torch.triu(Gbar, 1)
            return torch.linalg.solve_triangular(U, Gd.T, upper=True).T.contiguous()

    def _project_one_pass(self, state: FitState, Xs: List[torch.Tensor], mixed: bool = False, centred: bool = True,
                          nan_flag: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """All R scores from ONE read of every NaN-free block (centred: already centred in place; otherwise the centring
        is applied to the MTTKRP output as the shift mean^T W, itself an MTTKRP of the one-row "tensor" mean).

        The deflations are linear without missing values: X_{b,a+1} = X_{b,a} - t_a w_{b,a}^T with the
        (block-averaged) score t_a, hence X_{b,a} w_{b,a} = M_b[:, a] - sum_{j<a} t_j G_b[j, a] where
        M_b = X_{b,0} (W_A (.) W_B) is one MTTKRP and G_b = W_b^T W_b.  Averaging over blocks
        (cmtf.py:155,206) gives T (I + triu(mean G, 1)) = mean M: an R x R triangular solve.
        Returns None when the MTTKRP kernel does not take the shape (caller falls back)."""
        be = self.be
        R = state.n_components
        I = Xs[0].shape[0]
        nb = len(Xs)
        if R > 64:
            return None
        Ms = be.empty(nb, I * R)
        Gs = be.empty(nb, R * R)
        shifts = None if centred else be.empty(nb, R)
        for b, (blk, X) in enumerate(zip(state.blocks, Xs)):
            loads = blk.loadings
            WA, WB = self._kr_operands(blk, R)
            if be.mttkrp(X.view(I, -1), blk.A, blk.B, WA, WB, Ms[b].view(I, R), mixed=mixed) is None:
                return None
            if not centred and be.mttkrp(blk.mean.view(1, -1), blk.A, blk.B, WA, WB, shifts[b].view(1, R)) is None:
                return None
            for m, L in enumerate(loads):                 # Gram of a Khatri-Rao product = Hadamard product of the mode Grams
                be.kr_gram(L, Gs[b], first=(m == 0))
        Mbar = be.scores_mean(Ms, be.empty(I * R)).view(I, R) if nb > 1 else Ms[0].view(I, R)
        Gbar = be.scores_mean(Gs, be.empty(R * R)).view(R, R) if nb > 1 else Gs[0].view(R, R)
        if centred:
            return be.unit_upper_solve_rows(Mbar, Gbar, None, nan_flag)      # T (I + triu(Gbar, 1)) = Mbar, on the device
        shift = be.scores_mean(shifts, be.empty(R)) if nb > 1 else shifts[0]
        return be.unit_upper_solve_rows(Mbar, Gbar, shift, nan_flag)
