"""Sparse loadings (`tPLS(n, sparsity=...)`, `ctPLS(n, sparsity=...)`): what the argument may be, the lambda of every
non-sample mode of every block once the shapes are known, and the limits of the device extraction -- all checked before the first sweep.

soft(v, lam): theta = lam * max_j |v_j|, out_j = sign(v_j) * max(|v_j| - theta, 0), 0 <= lam < 1.  A matrix block's loading is
soft(Z, lam) / |.|_2; an order-3 block's pair comes from the dense leading pair by alternating soft-thresholded sweeps
(cmtfpls_rank1_sparse_f64).  Everything else of the fit (tpls.py:73-120, cmtf.py:85-140) is unchanged."""
from __future__ import annotations

from numbers import Real
from typing import List, Optional, Sequence, Tuple

MAX_SPARSE_SIDE = 4096          # cmtfpls_rank1_sparse_f64: 2 <= A, B <= 4096 ...
MAX_SPARSE_CELLS = 65536        # ... and A * B <= 65536 (one workgroup walks Z twice per sweep)

# the forms of the fit that extract loadings inside a fused native call, and are therefore not taken by a sparse fit
SWITCHED_OFF = {
    "small_fit": "the one-launch fit (cmtfpls_fit_small_f64) extracts dense loadings inside its kernel",
    "fused direct iteration": "the direct loop keeps its unfused form, whose every extraction goes through NipalsEngine._rank1",
    "xcov_iterate / xcov_iterate_plan": "the single-call iteration on S (cmtfpls_xcov_iterate_f64) extracts the dense pair inside the call",
    "xcov_blocks_plan": "the single-call iteration of coupled blocks (cmtfpls_xcov_iterate_blocks_f64) extracts dense loadings inside the call",
    "pipelined xcov loop": "the pipelined inner loop on S is built on the two single-call iterations",
}


def _lam(v) -> float:
    if isinstance(v, bool) or not isinstance(v, Real):
        raise ValueError(f"sparsity: expected a number in [0, 1), got {v!r}")
    v = float(v)
    if not (0.0 <= v < 1.0):
        raise ValueError(f"sparsity: lambda = {v!r} outside [0, 1)")
    return v


def _entry(v):
    """One block's entry: a scalar, or one lambda per non-sample mode."""
    if isinstance(v, (list, tuple)):
        if len(v) == 0:
            raise ValueError("sparsity: an empty sequence")
        return tuple(_lam(x) for x in v)
    return _lam(v)


def check_sparsity(value, coupled: bool):
    """The constructor's check: None, a scalar, one lambda per non-sample mode (tPLS) or one such entry per block (ctPLS).  Returns the
    value with every lambda as a float (sequences as tuples / lists of the same nesting); raises ValueError otherwise."""
    if value is None:
        return None
    if hasattr(value, "tolist"):
        value = value.tolist()
    if not coupled:
        return _entry(value)
    if isinstance(value, (list, tuple)):
        return [_entry(v.tolist() if hasattr(v, "tolist") else v) for v in value]
    return _lam(value)


def resolve_sparsity(value, shapes: Sequence[Sequence[int]], coupled: bool) -> Optional[List[Tuple[float, ...]]]:
    """Per block, one lambda per non-sample mode; None for a dense model."""
    if value is None:
        return None
    if coupled and isinstance(value, (list, tuple)):
        if len(value) != len(shapes):
            raise ValueError(f"sparsity has {len(value)} entries for {len(shapes)} blocks")
        entries = list(value)
    else:
        entries = [value] * len(shapes)
    out = []
    for b, (e, shape) in enumerate(zip(entries, shapes)):
        modes = len(shape) - 1
        if isinstance(e, tuple):
            if len(e) != modes:
                raise ValueError(f"sparsity of block {b}: {len(e)} lambdas for {modes} non-sample modes")
            out.append(tuple(e))
        else:
            out.append((float(e),) * modes)
    return out


def validate_sparse_limits(shapes, lams) -> None:
    """Next to state.validate_limits: a sparse fit the device extraction cannot run, refused before the first sweep."""
    if lams is None:
        return
    for shape in shapes:
        order = len(shape)
        if order >= 4:
            raise NotImplementedError(f"sparsity: X block {tuple(shape)} has order {order}; sparse loadings are built for blocks of order 2 and 3")
        if order == 3:
            A, B = int(shape[1]), int(shape[2])
            if not (2 <= A <= MAX_SPARSE_SIDE and 2 <= B <= MAX_SPARSE_SIDE and A * B <= MAX_SPARSE_CELLS):
                raise ValueError(f"sparsity: X block {tuple(shape)}: the sparse extraction takes 2 <= J, K <= {MAX_SPARSE_SIDE} with "
                                 f"J * K <= {MAX_SPARSE_CELLS} (cmtfpls_rank1_sparse_f64)")
        if order == 2 and int(shape[1]) > (1 << 24):
            raise ValueError(f"sparsity: X block {tuple(shape)}: more than 2^24 variables (cmtfpls_soft_normalize_f64)")
