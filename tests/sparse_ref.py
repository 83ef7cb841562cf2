"""Float64 mirror of the sparse loadings -- TEST INFRASTRUCTURE ONLY.

  soft / sparse_rank1      the rule as the issue and include/cmtfpls.h state it, in NumPy
  sparse_oracle(lams)      context manager: oracle.nipals_oracle.rank1_factors is swapped for the sparse rule, lambda looked up by
                           Z.shape, so that oracle.fit_tpls / fit_ctpls ARE the sparse model in float64 (nothing under oracle/ changes)
  SparseNumpyBackend       tests/numpy_backend.NumpyBackend with the two new backend methods
  screen_*                 the margins a comparison of zero patterns and iteration counts needs (theta, tol)
"""
import contextlib

import numpy as np
import torch

import oracle.nipals_oracle as NO
from numpy_backend import NumpyBackend

_DENSE = NO.rank1_factors           # the oracle's own extraction, taken once: the patch below must never wrap itself


def soft(v, lam, margins=None):
    v = np.asarray(v, dtype=np.float64)
    theta = lam * np.max(np.abs(v))
    if margins is not None and theta > 0:
        margins.append(float(np.min(np.abs(np.abs(v) - theta)) / theta))       # relative distance of the closest entry to theta
    return np.sign(v) * np.maximum(np.abs(v) - theta, 0.0)


def soft_normalize(v, lam, margins=None):
    s = soft(v, lam, margins)
    with np.errstate(all="ignore"):
        return s / np.linalg.norm(s)


def sparse_rank1(Z, lams, tol_s=1e-10, max_sweeps=200, dense=None, stats=None):
    """The sparse pair of the A x B matrix Z (a vector Z: soft(Z, lam) / |.|, no sweeps).  Returns [wA, wB] ([w] for a vector);
    stats (a dict, optional) receives info = [converged, sweeps] and `margins`, the theta margins of the LAST sweep."""
    Z = np.asarray(Z, dtype=np.float64)
    if Z.ndim == 1:
        m = []
        w = soft_normalize(Z, lams[0], m)
        if stats is not None:
            stats.update(info=[1, 0], margins=m)
        return [w]
    dense = dense or _DENSE
    wA, wB = (np.asarray(f, dtype=np.float64).ravel() for f in dense(Z))
    conv, sweeps, margins = 0, 0, []
    for s in range(max_sweeps):
        margins = []
        a = soft_normalize(Z @ wB, lams[0], margins)
        b = soft_normalize(Z.T @ a, lams[1], margins)
        d = max(np.max(np.abs(a - wA)), np.max(np.abs(b - wB)))
        wA, wB = a, b
        sweeps = s + 1
        if d < tol_s:
            conv = 1
            break
    if stats is not None:
        stats.update(info=[conv, sweeps], margins=margins)
    return [wA, wB]


@contextlib.contextmanager
def sparse_oracle(lams_by_shape, tol_s=1e-10, max_sweeps=200, log=None):
    """lams_by_shape: {Z.shape: lambdas}.  log (a list, optional) receives the stats of every extraction."""
    def patched(Z, tol=1e-8, n_iter_max=100):
        Z = np.asarray(Z, dtype=float)
        lams = lams_by_shape[tuple(Z.shape)]
        st = {}
        out = sparse_rank1(Z, lams, tol_s, max_sweeps, dense=lambda z: _DENSE(z, tol, n_iter_max), stats=st)
        if log is not None:
            log.append(st)
        return out

    old = NO.rank1_factors
    NO.rank1_factors = patched
    try:
        yield
    finally:
        NO.rank1_factors = old


class SparseNumpyBackend(NumpyBackend):
    def rank1_sparse_form(self, A, B):
        return 1 if (A * B + 2 * (A + B) + 2048 + 32 + 1) * 8 <= 150 * 1024 else 2

    def rank1_sparsify(self, Z, A, B, wA, wB, lamA, lamB, info=None, tol_s=1e-10, max_sweeps=200):
        st = {}
        a, b = sparse_rank1(Z.numpy().reshape(A, B), (lamA, lamB), tol_s, max_sweeps,
                            dense=lambda z: [wA.numpy().copy(), wB.numpy().copy()], stats=st)
        wA.copy_(torch.from_numpy(a))
        wB.copy_(torch.from_numpy(b))
        if info is not None:
            info[0], info[1] = float(st["info"][0]), float(st["info"][1])

    def soft_normalize(self, v, lam):
        v.copy_(torch.from_numpy(soft_normalize(v.numpy(), lam)))


# ---- screened inputs: what the CPU and the GPU fits of the sparse suites run on -----------------------------------------------------------
FIT_TOL = 1e-8
# name -> (kind, shapes, sparsity as the estimator takes it, seed, fit tolerance, responses).  Seed and tolerance were found by
# scanning seeds 0, 1, 2, ... of each recipe, with tol from {1e-8, 3e-9, 1e-9, 3e-10, 1e-10}, for the first pair that passes
# `screen_case`: the inner loop converges geometrically, so two consecutive norms must lie more than two decades apart around tol in
# EVERY component -- one seed in a few hundred.  No seed of the coupled recipe did with three responses (1500 scanned); with two it
# converges faster.  tests/test_sparse_cpu.py asserts the margins of every case.
CASES = {
    "tpls_02": ("tpls", [(60, 12, 9)], (0.2, 0.2), 264, 1e-8, 3),
    "tpls_05": ("tpls", [(60, 12, 9)], (0.5, 0.3), 68, 1e-9, 3),
    "tpls_nan": ("tpls_nan", [(60, 12, 9)], (0.2, 0.2), 1483, 3e-10, 3),
    "ctpls": ("ctpls", [(80, 10, 8), (80, 20)], [(0.2, 0.2), 0.3], 326, 1e-8, 2),
}
N_RESP, N_COMP = 3, 3


def case_tol(name):
    return CASES[name][4]


def case_data(name, seed=None, n_resp=None):
    """(blocks, y, sparsity) of a case: the synthetic recipe of the suite (oracle.import_synthetic, error 0.1); `tpls_nan` with 10 % of
    the entries missing; `ctpls` with a second, matrix block that shares the sample mode's factors."""
    import oracle as O
    kind, shapes, sparsity, fixed = CASES[name][:4]
    seed = fixed if seed is None else seed
    x, y, cp = O.import_synthetic(shapes[0], n_resp or CASES[name][5], N_COMP, error=0.1, seed=seed)
    blocks = [x]
    if kind == "tpls_nan":
        x[np.random.default_rng(seed + 1000).random(x.shape) < 0.10] = np.nan
    if kind == "ctpls":
        rng = np.random.default_rng(seed + 2000)
        blocks.append(cp.factors[0] @ rng.normal(size=(shapes[1][1], N_COMP)).T + 0.1 * rng.normal(size=shapes[1]))
    return blocks, y, sparsity


def block_lams(blocks, sparsity):
    from cmtf_pls_amd.sparsity import check_sparsity, resolve_sparsity
    coupled = len(blocks) > 1
    return resolve_sparsity(check_sparsity(sparsity, coupled), [b.shape for b in blocks], coupled)


def mirror_fit(blocks, y, sparsity, tol=FIT_TOL, log=None, R=N_COMP):
    """The sparse model in float64: the oracle's fit with its extraction swapped for the sparse rule."""
    import oracle as O
    with sparse_oracle(lams_for([b.shape for b in blocks], block_lams(blocks, sparsity)), log=log):
        return O.fit_ctpls(list(blocks), y, R, tol=tol) if len(blocks) > 1 else O.fit_tpls(blocks[0], y, R, tol=tol)


def screen_case(blocks, y, sparsity, tol=FIT_TOL, R=N_COMP):
    """The margins a comparison of iteration counts and zero patterns needs: (the smallest relative distance of a pre-threshold
    magnitude to theta in the final sweep of any extraction of the mirror fit; True when no convergence norm lies within 10x of tol
    at a stopping iteration or the one before; every extraction converged).  The norms are the engine's own (FitRun.iterate
    returns them) on the float64 test backend."""
    from cmtf_pls_amd.engine import EngineOptions, NipalsEngine
    log = []
    mirror_fit(blocks, y, sparsity, tol, log=log, R=R)
    coupled = len(blocks) > 1
    eng = NipalsEngine(SparseNumpyBackend(), options=EngineOptions(small_fit=False))
    y2 = y.reshape(len(y), -1)
    run = eng.begin([torch.from_numpy(b.copy()) for b in blocks], torch.from_numpy(y2.copy()), R, coupled=coupled,
                    sparsity=sparsity if not isinstance(sparsity, list) or coupled else tuple(sparsity))
    ok = True
    for a in range(R):
        run.start_component(a)
        norms = []
        for it in range(100):
            du = run.iterate(it)
            if du is not None:
                norms.append(du)
                if du < tol:
                    break
        run.finish_component(a)
        ok = ok and len(norms) >= 1 and norms[-1] < tol and not any(tol / 10.0 <= v <= tol * 10.0 for v in norms[-2:])
    return min_theta_margin(log), ok, all(st["info"][0] == 1 for st in log)


def lams_for(shapes, sparsity_per_block):
    """{Z.shape: lambdas} for blocks of the given (I, ...) shapes."""
    return {tuple(s[1:]): tuple(l) for s, l in zip(shapes, sparsity_per_block)}


def min_theta_margin(log):
    m = [x for st in log for x in st["margins"]]
    return min(m) if m else np.inf


# ---- inputs of the kernel tests ---------------------------------------------------------------------------------------------------
KERNEL_SHAPES = [(12, 9), (7, 70), (2, 2), (128, 128), (130, 128), (256, 256), (16, 4096)]
KERNEL_LAMS = [(0.0, 0.0), (0.2, 0.2), (0.5, 0.3), (0.95, 0.95)]
THETA_MARGIN = 1e-6


def dense_pair(Z):
    """The leading singular pair with the engine's sign rule (largest-|.| entry of wB positive): what both the mirror and the
    kernel start from in the kernel tests, so that only the summation order differs between them."""
    U, _, Vt = np.linalg.svd(Z, full_matrices=False)
    u, v = U[:, 0].copy(), Vt[0].copy()
    if v[np.argmax(np.abs(v))] < 0:
        u, v = -u, -v
    return u, v


def kernel_case(shape, variant="plain", seed=0):
    """An A x B matrix with a dominant sparse-ish rank-1 part plus noise.  variant "zero_row": one all-zero row; "tie": the row that
    carries the largest |Z wB| appears twice, so max_j |(Z wB)_j| is attained by two entries with the same bits."""
    A, B = shape
    rng = np.random.default_rng(1000 * A + B + 7919 * seed)
    u = rng.normal(size=A) * (rng.random(A) < 0.6) + 0.05 * rng.normal(size=A)
    v = rng.normal(size=B) * (rng.random(B) < 0.6) + 0.05 * rng.normal(size=B)
    Z = 4.0 * np.outer(u / np.linalg.norm(u), v / np.linalg.norm(v)) + 0.3 * rng.normal(size=(A, B)) / np.sqrt(max(A, B))
    if variant == "zero_row":
        Z[A // 2] = 0.0
    if variant == "tie":
        _, wB = dense_pair(Z)
        top = int(np.argmax(np.abs(Z @ wB)))
        Z[(top + 1) % A] = Z[top]
    return np.ascontiguousarray(Z)
