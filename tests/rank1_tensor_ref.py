"""Host reference of the rank-1 CP extraction of a cross-covariance tensor (csrc/rank1_tensor.hip) and the cases its tests run.

`als` restates the sweep of oracle/nipals_oracle.py::rank1_factors -- the same formulae in the same order, the same stop rule, the
same normalisation -- from init vectors handed in, in a number type of the caller's choice: float64 is the oracle's arithmetic
(bit for bit from the oracle's own init, tests/test_rank1_tensor_ref_cpu.py), long double is what the kernel is compared with.
`unfold` is the host statement of unfold_kernel.  NumPy only: importable without a GPU and without the library.

The cases (`CASES`): three kinds of Z, every one from a fixed seed,
  strong   2 * a unit rank-one tensor + 0.5 * unit noise                           (the ALS stops after 3 or 4 sweeps)
  close    two unit rank-one terms with weights 1 and 0.97 + 0.05 * unit noise     (3 to 32 sweeps)
  noise    unit noise only                                                         (12 to 87 sweeps, 1024 x 3 x 2 runs into the cap of 100)
The seed is part of the case: with it the stop decision has a margin (`als` returns it) of at least 1e-11
(tests/test_rank1_tensor_ref_cpu.py) -- the sweep at which the ALS stops is then a property of the data and not of the rounding,
and the kernel must stop there too."""
from collections import namedtuple
from functools import reduce

import numpy as np

MAX_SWEEPS = 100
MIN_MARGIN = 1e-11               # 1e4 roundings of a reconstruction error of order one


def unfold(Z, m):
    """The mode-m unfolding of Z: row = index along m, column = C-order index over the remaining modes."""
    return np.reshape(np.moveaxis(Z, m, 0), (Z.shape[m], -1))


def sign_rule(v):
    """cp_rank1_als_kernel's sign rule: the largest-|.| entry positive, the first index on ties."""
    v = np.array(v, copy=True)
    return -v if v[np.argmax(np.abs(v))] < 0 else v


def _kron_all(vecs):
    return reduce(np.kron, [np.asarray(v).ravel() for v in vecs])


def als(Z, init, tol, max_sweeps=MAX_SWEEPS, dtype=np.longdouble):
    """(factors, sweeps run, stop margin) of the ALS of oracle.rank1_factors from the vectors `init` in `dtype`.

    The stop margin is min over the sweeps where the stop rule was evaluated of | |err_{s-1} - err_s| - tol |: how far the closest
    decision was from falling the other way (inf when the rule was never evaluated).  After a run that reached `max_sweeps` the
    factors are the last sweep's, normalised -- as the oracle returns them."""
    Z = np.asarray(Z, dtype=dtype)
    N = Z.ndim
    fac = [sign_rule(np.asarray(v, dtype=dtype)) for v in init]
    tol = dtype(tol)
    weight = dtype(1.0)
    norm_Z = np.linalg.norm(Z)
    errs = []
    margin = np.inf
    sweeps = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for sweep in range(max_sweeps):
            sweeps += 1
            mttkrp = None
            for m in range(N):
                others = [fac[i] for i in range(N) if i != m]
                gram = weight * weight * np.prod([o @ o for o in others])
                mttkrp = unfold(Z, m) @ (_kron_all(others) * weight)
                fac[m] = mttkrp / gram
            fnorm2 = weight * weight * np.prod([f @ f for f in fac])
            iprod = (mttkrp @ fac[-1]) * weight
            errs.append(np.sqrt(abs(norm_Z ** 2 + fnorm2 - 2.0 * iprod)) / norm_Z)
            if sweep >= 1:
                step = abs(errs[-2] - errs[-1])
                margin = min(margin, float(abs(step - tol)))         # (NaN never lowers it: a zero Z has no decision to miss)
                if step < tol:
                    break
            norms = [np.linalg.norm(f) for f in fac]
            weight = weight * np.prod(norms)
            fac = [f / n for f, n in zip(fac, norms)]
    return fac, sweeps, margin


def spread(Z, init, tol, max_sweeps=MAX_SWEEPS):
    """d_case: max |als(float64) - als(long double)| over every factor entry, both from `init` -- what rounding alone does to this
    case on the host.  Also returns the long-double factors, sweeps and margin (the reference of the GPU test)."""
    f64, s64, _ = als(Z, init, tol, max_sweeps, np.float64)
    fld, sld, margin = als(Z, init, tol, max_sweeps, np.longdouble)
    assert s64 == sld, (s64, sld)
    d = max(float(np.max(np.abs(a.astype(np.longdouble) - b))) for a, b in zip(f64, fld))
    return d, fld, sld, margin


def _unit(t):
    return t / np.linalg.norm(t)


def _rank_one(rng, dims):
    return _unit(reduce(np.multiply.outer, [rng.normal(size=d) for d in dims]))


def make_z(dims, kind, seed):
    rng = np.random.default_rng(seed)
    noise = _unit(rng.normal(size=dims))
    if kind == "strong":
        return 2.0 * _rank_one(rng, dims) + 0.5 * noise
    if kind == "close":
        return _rank_one(rng, dims) + 0.97 * _rank_one(rng, dims) + 0.05 * noise
    if kind == "noise":
        return noise
    raise ValueError(kind)


Case = namedtuple("Case", "name dims kind seed tol budget about")

KINDS = ("strong", "close", "noise")


def _case(dims, kind, about, tol=1e-8, budget=30, seed=0):
    name = "x".join(map(str, dims)) + "-" + kind + ("" if tol == 1e-8 else f"-tol{tol:g}") + ("" if budget == 30 else f"-sq{budget}")
    return Case(name, dims, kind, seed, tol, budget, about)


def _table():
    out = []
    for dims, about in (((9, 8, 7), "order 3"), ((5, 4, 3, 2), "order 4"), ((3, 2, 4, 2, 3), "order 5"),
                        ((2, 3, 2, 2, 3, 2), "order 6"), ((2, 2, 2, 2, 2, 2, 3), "order 7 = kMaxOrder"),
                        ((4, 1, 5), "a mode of size 1 in the middle"), ((1, 6, 5), "a mode of size 1 first"),
                        ((6, 5, 1), "a mode of size 1 last"),
                        ((70, 3, 65), "a mode longer than 64 lanes, more rows than 16 wavefronts"),
                        ((300, 20, 15), "mode-0 unfolding 300 x 300: the init through a launch per squaring"),
                        ((1024, 3, 2), "the 1024 limit first"), ((2, 1024, 3), "the 1024 limit in the middle"),
                        ((3, 2, 1024), "the 1024 limit last"), ((17, 16, 15, 3), "order 4, no size a multiple of 16")):
        out += [_case(dims, kind, about) for kind in KINDS]
    out.append(_case((48, 40, 36), "strong", "one workgroup walking 540 KB of Z"))
    out.append(_case((9, 8, 7), "noise", "tol = 0: to the cap of 100 sweeps", tol=0.0))
    # (seed 2: the first `close` Z whose error moves by less than 1e-2 between the first two sweeps -- every `strong` one moves more)
    out.append(_case((9, 8, 7), "close", "tol = 1e-2: stops at the second sweep, the earliest", tol=1e-2, seed=2))
    out.append(_case((9, 8, 7), "strong", "2 squarings: an init that has not converged", budget=2))
    out.append(_case((9, 8, 7), "close", "2 squarings: an init that has not converged", budget=2))
    return out


CASES = _table()
