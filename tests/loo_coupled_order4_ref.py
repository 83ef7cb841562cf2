"""cmtfpls_loo_xcov_coupled_tensor_f64 (csrc/loo_xcov_coupled.hip, loo_xcov_coupled_kernel<true>: leave-one-out refits of a ctPLS with
blocks of order 4 among blocks of order 2, 3 and 4, a 512-thread workgroup per fold) in plain NumPy (TEST INFRASTRUCTURE): a mirror of
the entry's shape rules, the case table, and cached references.  The refits themselves are loo_coupled_ref's, unchanged: its _refit,
loo_literal, loo_on_s and case_data take blocks of any order through oracle.rank1_factors.  Shared by
tests/test_loo_coupled_order4_cpu.py (which proves the mirror and the input conditions without a GPU) and
tests/test_gpu_loo_coupled_order4_kernel.py.  The references of a case are computed once per process and are read-only.

The mirror is written from the kernel's header comment, not by calling the library.  A block is given by its trailing shape: (J,) a
matrix block (A = 1, B = J), (J, K) an order-3 block (A = J, B = K), (A, B1, B2) a tensor block (B = B1 B2); P_b = A_b B_b.
  limits     at most 8 blocks; min(A_b, B_b) <= 256 in a block of order 2 or 3; the shorter side of each of the three unfoldings of a
             tensor block <= 256; M <= 128; R <= 64; P_b <= 2^24; the workgroup's vectors within 150 KB of dynamic LDS -- checked
             in this order, the first that fails is the reason;
  LDS        every block's wA_b (A_b) and wB_b (B_b), q, qn, tq, my (M each), G_y (M x M), xs (nmax), ys (kmax), the CP's wK (max
             B1), wL (max B2), v (max B1 B2), tmp (max single dim) and part (512), taken over the tensor blocks, coef (R x R), Qs
             (R x M), Gn (R x R), gn, bb, dd (R each); nmax = the largest of min(A_b, B_b) over the blocks of order 2 or 3 and of the
             unfoldings' shorter sides, kmax = max max(A_b, B_b) over the blocks of order 2 or 3 alone (0 without one):
             sum A_b + sum B_b + 4 M + M^2 + nmax + kmax + 2 R^2 + R M + 3 R + max B1 + max B2 + max B1 B2 + max dim + 512 doubles;
  workspace  per resident fold (I + M) sumP + 3 Pmax + 3 Ptmax + 2 nmax^2 + I (M + R + 2) + R (sum A_b + sum B_b) doubles, Ptmax the
             largest P_b of a tensor block."""
import functools

import numpy as np

import loo_coupled_ref as C
from loo_coupled_ref import CAP_ITER, CAP_TOL, EXCLUDED_CAP, MAX_ITER, TOL, normwise, on_threshold  # noqa: F401  (shared yardsticks)

MAX_BLOCKS, MAX_N, MAX_M, MAX_R = 8, 256, 128, 64
LDS_CAP = 150 * 1024
MAX_CELLS = 1 << 24
THREADS = 512


def split(trail):
    """(A, B) of the I x A x B view of a block's trailing shape."""
    if len(trail) == 3:
        return trail[0], trail[1] * trail[2]
    return C.split(trail)


def pair(trail):
    """The block's entry of the C entry's `dims`: (B1, B2) of a tensor block, (0, 0) otherwise."""
    return (trail[1], trail[2]) if len(trail) == 3 else (0, 0)


def unfoldings(trail):
    """The shorter side of each of the three unfoldings of a tensor block."""
    P = int(np.prod(trail))
    return [min(d, P // d) for d in trail]


def _sizes(dims):
    mats = [split(d) for d in dims if len(d) < 3]
    tens = [d for d in dims if len(d) == 3]
    nmax = max([min(A, B) for A, B in mats] + [s for t in tens for s in unfoldings(t)])
    kmax = max([max(A, B) for A, B in mats], default=0)
    return mats, tens, nmax, kmax


def lds_doubles(dims, M: int, R: int) -> int:
    _, tens, nmax, kmax = _sizes(dims)
    ab = [split(d) for d in dims]
    cp = max(t[1] for t in tens) + max(t[2] for t in tens) + max(t[1] * t[2] for t in tens) + max(max(t) for t in tens) + THREADS
    return sum(A + B for A, B in ab) + 4 * M + M * M + nmax + kmax + 2 * R * R + R * M + 3 * R + cp


def form(I: int, dims, M: int, R: int):
    """(form, None), or (None, why) when the entry declines with status 4: why is "blocks", "n", "unfolding", "M", "R", "cells" or
    "lds".  dims: the trailing shape of every block, at least one of them a tensor block."""
    assert any(len(d) == 3 for d in dims) and all(1 <= len(d) <= 3 for d in dims)
    if len(dims) > MAX_BLOCKS:
        return None, "blocks"
    if any(min(split(d)) > MAX_N for d in dims if len(d) < 3):
        return None, "n"
    if any(s > MAX_N for d in dims if len(d) == 3 for s in unfoldings(d)):
        return None, "unfolding"
    if M > MAX_M:
        return None, "M"
    if R > MAX_R:
        return None, "R"
    ab = [split(d) for d in dims]
    if any(A * B > MAX_CELLS for A, B in ab):
        return None, "cells"
    lds = 8 * lds_doubles(dims, M, R)
    if lds > LDS_CAP:
        return None, "lds"
    _, tens, nmax, kmax = _sizes(dims)
    sumP, Pmax, Ptmax = sum(A * B for A, B in ab), max(A * B for A, B in ab), max(int(np.prod(t)) for t in tens)
    ws = 8 * ((I + M) * sumP + 3 * Pmax + 3 * Ptmax + 2 * nmax * nmax + I * (M + R + 2) + R * sum(A + B for A, B in ab))
    return {"lds_bytes": lds, "ws_bytes_per_fold": ws, "blocks": len(dims), "nmax": nmax, "kmax": kmax, "tiles": -(-nmax // 16),
            "orders": [len(d) + 1 for d in dims], "tensors": len(tens), "over_48k": lds > 48 * 1024, "m_groups": -(-M // 16),
            "mode0_transposed": [t[0] > t[1] * t[2] for t in tens]}, None


def longest_row(others, M: int, R: int) -> int:
    """The largest J of a matrix block (J,) the LDS rule admits next to the blocks `others` with M responses and R components."""
    J = 1
    while 8 * lds_doubles(list(others) + [(J + 1,)], M, R) <= LDS_CAP:
        J += 1
    return J


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (I, trailing shapes of the blocks, M, R, latent rank, noise, seed, folds compared ("all" or a tuple), branch values of the form)
_ROW_OTHERS = [(3, 4, 5)]
J_STAR = longest_row(_ROW_OTHERS, 3, 2)
CASES = [
    (10, ((5, 7, 3), (9,), (4, 6)), 3, 3, 2, 1e-10, 1, "all", dict(orders=[4, 2, 3], tensors=1, nmax=7, kmax=9)),   # orders 4, 2 and 3 together
    (9, ((40, 3, 2), (6,)), 2, 2, 2, 1e-10, 0, "all", dict(mode0_transposed=[True], nmax=6)),          # A > B1 B2: the transpose path of mode 0
    (8, ((3, 16, 16), (17, 33)), 2, 2, 2, 0.05, 2, "all", dict(nmax=17, tiles=2)),                     # a whole MFMA tile next to a tile edge
    (9, ((6, 1, 5), (6, 5, 1), (4,)), 2, 2, 2, 0.05, 3, "all", dict(tensors=2, nmax=5)),               # unit modes; two tensor blocks share one CP scratch
    (10, ((4, 17, 2), (2, 3, 19)), 3, 3, 3, 1e-10, 0, "all", dict(tensors=2, kmax=0, nmax=8, tiles=1)),    # tile remainders; no matrix block
    (9, ((3, 2, 2),) * 8, 1, 2, 2, 0.3, 0, "all", dict(blocks=8, m_groups=1)),                         # 8 blocks, M = 1
    (6, ((256, 16, 16), (40,)), 2, 2, 3, 0.05, 0, (0, 3, 5), dict(nmax=256, tiles=16)),                # an unfolding's short side at 256
    (10, ((5, 7, 3), (9,)), 128, 3, 2, 1e-10, 0, (0, 5, 9), dict(m_groups=8, over_48k=True)),          # M at its maximum
    (10, ((3, 4, 5), (J_STAR,)), 3, 2, 2, 0.3, 1, (0, 5, 9), dict(kmax=J_STAR, over_48k=True)),        # exactly at the LDS cap
]
RANGE_CASE, RANGE = CASES[0], (3, 4)                           # fold0 = 3, nfolds = 4 into a sentinel-filled Ypred
CHUNK_CASE = CASES[3]

# limit -> ((I, dims, M, R) one step inside, one step past).  "cells" has no inside: P_b near 2^24 with every short side <= 256 puts a
# side of at least 65536 doubles in the LDS, so a step inside that limit is past the LDS cap.
DECLINES = {
    "blocks": ((4, ((2, 2, 2),) + ((3,),) * 7, 2, 2), (4, ((2, 2, 2),) + ((3,),) * 8, 2, 2)),
    "unfolding": ((4, ((256, 16, 16), (5,)), 2, 2), (4, ((257, 16, 17), (5,)), 2, 2)),
    "n": ((4, ((2, 2, 2), (256, 257)), 2, 2), (4, ((2, 2, 2), (257, 257)), 2, 2)),
    "M": ((4, ((5, 7, 3), (9,)), 128, 2), (4, ((5, 7, 3), (9,)), 129, 2)),
    "R": ((4, ((5, 7, 3), (9,)), 2, 64), (4, ((5, 7, 3), (9,)), 2, 65)),
    "lds": ((4, ((3, 4, 5), (J_STAR,)), 3, 2), (4, ((4, 4, 5), (J_STAR,)), 3, 2)),       # one more entry of wA_0: 8 bytes past
}
CELLS_PAST = (4, ((1, 256, 70000), (5,)), 2, 2)                # the unfoldings' short sides are 1, 256, 256; P = 256 * 70000 > 2^24


def case_id(case) -> str:
    dims = "+".join("x".join(str(d) for d in t) for t in case[1]) if len(case[1]) < 8 else f"{len(case[1])}blocks"
    return f"I{case[0]}-{dims}-M{case[2]}-R{case[3]}"


def case_folds(case):
    return tuple(range(case[0])) if case[7] == "all" else tuple(case[7])


def data(case):
    return C.case_data(case[0], case[1], case[2], *case[4:7])


@functools.lru_cache(maxsize=None)
def case_reference(case_key, tol, max_iter):
    """loo_coupled_ref.loo_literal of the case's compared folds; read-only."""
    case = _CASES[case_key]
    xs, y = data(case)
    ref = C.loo_literal(xs, y, case[3], tol, max_iter, case_folds(case))
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def case_probe(case_key, tol, max_iter) -> float:
    """loo_coupled_ref.condition_probe of the case's compared folds, sharing the cached literal refits."""
    case = _CASES[case_key]
    xs, y = data(case)
    on_s = C.loo_on_s(xs, y, case[3], tol, max_iter, case_folds(case))
    return normwise(on_s["pred"], case_reference(case_key, tol, max_iter)["pred"])


_CASES = {case_id(c): c for c in CASES}
assert len(_CASES) == len(CASES)


def case_bound(case, tol, max_iter) -> float:
    """The normwise bound of a case's predictions: max(1e-8, 10 x condition_probe), test_gpu_loo_coupled_kernel.py's rule."""
    return max(1e-8, 10.0 * case_probe(case_id(case), tol, max_iter))


def reference(case, tol, max_iter):
    return case_reference(case_id(case), tol, max_iter)
