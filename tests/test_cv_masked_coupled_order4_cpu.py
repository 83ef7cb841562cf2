"""CPU-only: the opt-in switch of the coupled masked order-4 cross-validation form (EngineOptions.masked_tensor_folds_coupled, DESIGN
8v), its routing on a backend without the kernel (the NumPy test backend: refits with a why that names the new entry, results equal
to the option off), that masked_folds_coupled alone still declines a block of order 4 with today's text, the argument and shape
checks that cmtfpls_cv_masked_coupled_tensor_f64 makes before it touches a pointer or the GPU, the host's LDS and workspace formulas
against the library's, and the restatement of the GPU tests (coupled_masked_order4_ref) against the oracle on duplicated rows."""
import ctypes

import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import COUPLED_FORM, COUPLED_TENSOR_FORM, MAX_BLOCKS, wants_masked_coupled
from cmtf_pls_amd.validate import bootstrap_factors, get_q2y, get_q2y_repeated_kfold, kfold_predictions, permutation_test_q2y
from coupled_masked_order4_ref import coupled_masked_order4_fit
from numpy_backend import NumpyBackend

LDS_CAP = 150 * 1024
EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4


def _coupled_data(shapes, M, L, seed, nan=(0.1,)):
    """Blocks with the given shapes (rows first, shared) driven by one latent score, a Y of M responses; nan[b] of block b's
    entries missing (the last value repeats), every row keeping an observed entry in every block."""
    rng = np.random.default_rng(seed)
    I = shapes[0][0]
    T = rng.standard_normal((I, L))
    Xs = []
    for b, shape in enumerate(shapes):
        X = O.cp_factors_to_tensor([T] + [rng.standard_normal((d, L)) for d in shape[1:]]) + 0.3 * rng.standard_normal(shape)
        frac = nan[min(b, len(nan) - 1)]
        if frac:
            hole = rng.random(shape) < frac
            hole.reshape(I, -1)[:, b % int(np.prod(shape[1:]))] = False
            X[hole] = np.nan
        assert (~np.isnan(X).reshape(I, -1)).sum(axis=1).min() >= 1
        Xs.append(X)
    Y = T @ rng.standard_normal((L, M)) + 0.3 * rng.standard_normal((I, M))
    return Xs, Y


def _pair(Xs, y, R, **on):
    a = ctPLS(R, backend=NumpyBackend(), options=EngineOptions(small_fit=False, **on))
    b = ctPLS(R, backend=NumpyBackend(), options=EngineOptions(small_fit=False))
    a.fit(Xs, y)
    b.fit(Xs, y)
    return a, b


def _declined(rep):
    assert f"the masked form ({COUPLED_TENSOR_FORM}) declined" in rep["why"], rep
    assert "numpy-test backend has no coupled masked order-4 model kernel" in rep["why"], rep


def test_the_option_is_a_field_of_its_own_and_off_by_default():
    assert EngineOptions().masked_tensor_folds_coupled is False
    on = EngineOptions(masked_tensor_folds_coupled=True)
    assert on.masked_tensor_folds_coupled is True
    assert not (on.masked_folds_coupled or on.masked_tensor_folds or on.masked_folds or on.tensor_folds_coupled or on.tensor_resamples_coupled)
    for other in ("masked_folds_coupled", "masked_tensor_folds", "tensor_folds_coupled", "tensor_resamples_coupled"):
        assert EngineOptions(**{other: True}).masked_tensor_folds_coupled is False


def test_what_the_option_governs():
    Xs, y = _coupled_data([(12, 3, 2, 2), (12, 5)], 2, 3, seed=1, nan=(0.0, 0.1))       # NaN in the matrix block alone
    on, off = _pair(Xs, y, 2, masked_tensor_folds_coupled=True)
    assert wants_masked_coupled(on, Xs) and not wants_masked_coupled(off, Xs)
    assert not wants_masked_coupled(on, [np.nan_to_num(X) for X in Xs])                 # complete data
    assert not wants_masked_coupled(on, [Xs[1], Xs[1]])                                 # no block of order 4
    assert not wants_masked_coupled(on, Xs[0])                                          # a tPLS's X


def test_kfold_and_leave_one_out_without_the_kernel_refit_with_a_why():
    Xs, y = _coupled_data([(18, 3, 2, 2), (18, 5)], 2, 3, seed=3)
    on, off = _pair(Xs, y, 2, masked_tensor_folds_coupled=True)
    got = kfold_predictions(on, n_splits=3)
    _declined(on.q2y_report_)
    assert on.q2y_report_["form"] == "one refit per fold on the regular engine"
    want = kfold_predictions(off, n_splits=3)
    np.testing.assert_array_equal(got, want)
    assert "masked form" not in off.q2y_report_["why"]
    assert get_q2y(on) == get_q2y(off)                                                  # leave-one-out
    _declined(on.q2y_report_)


def test_permutation_repeated_and_bootstrap_without_the_kernel_refit_with_a_why():
    Xs, y = _coupled_data([(16, 5), (16, 3, 2, 2)], 2, 3, seed=4)
    on, off = _pair(Xs, y, 2, masked_tensor_folds_coupled=True)
    got = permutation_test_q2y(on, n_permutations=3, n_splits=4, per_component=True)
    _declined(on.q2y_report_)
    assert on.q2y_report_["form"] == "one refit per fold and permutation on the regular engine"
    want = permutation_test_q2y(off, n_permutations=3, n_splits=4, per_component=True)
    np.testing.assert_array_equal(got["null"], want["null"])
    np.testing.assert_array_equal(got["p_value"], want["p_value"])
    got = get_q2y_repeated_kfold(on, n_splits=3, n_repeats=2, per_component=True)
    _declined(on.q2y_report_)
    assert on.q2y_report_["form"] == "one refit per fold and split on the regular engine"
    np.testing.assert_array_equal(got["q2y"], get_q2y_repeated_kfold(off, n_splits=3, n_repeats=2, per_component=True)["q2y"])
    got = bootstrap_factors(on, n_resamples=3)
    _declined(on.bootstrap_report_)
    assert on.bootstrap_report_["form"] == "one refit per resample on the regular engine"
    want = bootstrap_factors(off, n_resamples=3)
    np.testing.assert_array_equal(got["coef"], want["coef"])
    np.testing.assert_array_equal(got["oob_q2y"], want["oob_q2y"])
    assert [f.shape[1] for f in got["X_factors"][1]] == [3, 2, 2]                       # an order-4 block's per-mode stacks


class _WithOrder3Kernel(NumpyBackend):
    """A backend that has the order-2/3 entry (never reached: the order of a block declines first)."""

    def cv_masked_coupled(self, *args, **kwargs):
        raise AssertionError("the decline comes before the kernel")


def test_masked_folds_coupled_alone_still_declines_with_todays_text():
    Xs, y = _coupled_data([(16, 3, 2, 2), (16, 5)], 2, 3, seed=6)
    on = ctPLS(2, backend=_WithOrder3Kernel(), options=EngineOptions(small_fit=False, masked_folds_coupled=True))
    on.fit(Xs, y)
    _, off = _pair(Xs, y, 2)
    got = get_q2y_repeated_kfold(on, n_splits=2, n_repeats=2, per_component=True)
    rep = on.q2y_report_
    assert rep["form"] == "one refit per fold and split on the regular engine", rep
    assert rep["why"] == f"the masked form ({COUPLED_FORM}) declined: block 0 of order 4 (the masked form takes order 2 and 3)", rep
    np.testing.assert_array_equal(got["q2y"], get_q2y_repeated_kfold(off, n_splits=2, n_repeats=2, per_component=True)["q2y"])
    both, _ = _pair(Xs, y, 2, masked_folds_coupled=True, masked_tensor_folds_coupled=True)    # with both, the order-4 entry is asked
    kfold_predictions(both, n_splits=2)
    _declined(both.q2y_report_)


def test_complete_blocks_and_models_without_an_order4_block_keep_their_routing():
    Xs, y = _coupled_data([(16, 3, 2, 2), (16, 5)], 2, 3, seed=7, nan=(0.0,))
    on, off = _pair(Xs, y, 2, masked_tensor_folds_coupled=True)
    np.testing.assert_array_equal(kfold_predictions(on, n_splits=4), kfold_predictions(off, n_splits=4))
    assert on.q2y_report_ == off.q2y_report_ and COUPLED_TENSOR_FORM not in str(on.q2y_report_)
    Xs, y = _coupled_data([(16, 4, 3), (16, 5)], 2, 3, seed=8)
    on, off = _pair(Xs, y, 2, masked_tensor_folds_coupled=True)
    np.testing.assert_array_equal(kfold_predictions(on, n_splits=4), kfold_predictions(off, n_splits=4))
    assert on.q2y_report_ == off.q2y_report_ and COUPLED_TENSOR_FORM not in str(on.q2y_report_)


# ---- the restatement against the oracle on duplicated rows ------------------------------------------------------------------------
def _col_rel(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return float(max(np.linalg.norm(got[..., j] - want[..., j]) / np.linalg.norm(want[..., j]) for j in range(want.shape[-1])))


@pytest.mark.parametrize("nan,info0", [((0.1, 0.1), 3), ((0.1, 0.0), 1), ((0.0, 0.1), 2)])
def test_restatement_equals_the_oracle_on_duplicated_rows(nan, info0):
    I, R = 30, 3
    Xs, y = _coupled_data([(I, 4, 3, 2), (I, 7)], 2, R + 1, seed=30, nan=nan)
    rng = np.random.default_rng(I + 1)
    c = rng.integers(0, 4, size=I)
    c[:3] = 0
    yrow = rng.permutation(I)
    factors, Q, coef, pred, n_iter, info = coupled_masked_order4_fit(Xs, y, c, R, yrow)
    assert info[0] == info0 and max(n_iter) < 100
    dup = np.repeat(np.arange(I), c)
    fit = O.fit_ctpls([X[dup] for X in Xs], y[yrow][dup], R)
    assert fit.has_miss == [bool(f) for f in nan] and n_iter == fit.n_iter
    for key, want in zip(("Wa", "Wk", "Wl"), fit.loadings[0]):
        assert _col_rel(factors[0][key], want) <= 1e-12
    assert set(factors[1]) == {"Wb"} and _col_rel(factors[1]["Wb"], fit.loadings[1][0]) <= 1e-12
    for a in range(R):
        np.testing.assert_array_equal(factors[0]["Wb"][:, a], np.kron(factors[0]["Wk"][:, a], factors[0]["Wl"][:, a]))
    assert _col_rel(Q, fit.Q) <= 1e-12 and np.abs(coef - fit.coef).max() <= 1e-12 * np.abs(fit.coef).max()
    assert np.isfinite(pred).all() and pred.shape == (R, int((c == 0).sum()), 2)


# ---- the checks of the C entry ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from cmtf_pls_amd import _lib
    return _lib.load()


def _blocks(trailing, orders=None):
    """The entry's description of blocks of trailing shape `trailing` ((J,), (A, B) or (A, B1, B2)) with stand-in pointers."""
    from cmtf_pls_amd import _lib
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    dims = [(1, t[0]) if len(t) == 1 else (t[0], int(np.prod(t[1:]))) for t in trailing]
    orders = orders or [len(t) + 1 for t in trailing]
    arr = (_lib.CvCoupledBlock * len(dims))(*[_lib.CvCoupledBlock(p, o, A, B) for o, (A, B) in zip(orders, dims)])
    arr._keep = buf
    pairs = [(t[1], t[2]) if len(t) == 3 else (0, 0) for t in trailing]
    return arr, p, dims, pairs


def _ints(pairs):
    flat = [int(v) for p in pairs for v in p]
    return (ctypes.c_int * len(flat))(*flat)


def _probe(lib, trailing, I, M, R, nm=3, orders=None, pairs=None, no_dims=False):
    """The entry's answer with stand-in pointers and no workspace: 1 = a bad argument, 4 = declined, 2 = accepted (only the
    workspace is missing).  None touches a pointer."""
    arr, p, _, own = _blocks(trailing, orders)
    dims = None if no_dims else _ints(own if pairs is None else pairs)
    return lib.cmtfpls_cv_masked_coupled_tensor_f64(arr, len(trailing), dims, p, p, None, nm, I, M, R, 1e-8, 100, 0, 1, p, None, None, None,
                                                    None, None, None, None, p, None, None, 0, None)


def _short_side(A, B1, B2):
    """The largest short side of the three unfoldings of an A x B1 x B2 contraction."""
    return max(min(d, A * B1 * B2 // d) for d in (A, B1, B2))


def _carve_up(dims, pairs, I, M, R):
    """The LDS of a workgroup as include/cmtfpls.h states it (doubles), dims = [(A, B), ..], pairs = [(B1, B2), ..] ((0, 0): a matrix
    block): nmax over the matrix blocks' short sides and every unfolding's, kmax over the matrix blocks alone, the CP's four maxima
    over the tensor blocks, then its argmax scratch (12)."""
    mats = [(A, B) for (A, B), (_, B2) in zip(dims, pairs) if B2 == 0]
    tens = [(A, B1, B2) for (A, _), (B1, B2) in zip(dims, pairs) if B2 > 0]
    nmax = max([min(A, B) for A, B in mats] + [_short_side(*t) for t in tens])
    kmax = max([max(A, B) for A, B in mats], default=0)
    cp = max(t[1] for t in tens) + max(t[2] for t in tens) + max(t[1] * t[2] for t in tens) + max(max(t) for t in tens) + 12
    return 8 * (3 * I + 3 * M + 2 * R * R + R * M + 3 * R + 512 + max(A * B for A, B in dims) + 2 * nmax * nmax + nmax + kmax + cp
                + sum((R + 1) * (A + B) + I for A, B in dims))


def _workspace(dims, pairs, I, M, R):
    """The workspace of one resident model as include/cmtfpls.h states it: per block the working copy, counts and means, then
    Yf | T, then the CP's Zt | U | yl | vr sized for the largest tensor block."""
    ptmax = max(A * B for (A, B), (_, B2) in zip(dims, pairs) if B2 > 0)
    return 8 * (sum((I + 2) * A * B for A, B in dims) + I * M + I * R + 4 * ptmax)


def test_c_entry_bad_arguments(lib):
    ok = [(3, 2, 2), (5,)]
    assert _probe(lib, ok, 40, 2, 2) == EWORKSPACE                                      # accepted
    assert _probe(lib, ok, 40, 2, 2, no_dims=True) == EINVAL                            # dims == NULL
    assert _probe(lib, ok, 40, 2, 2, pairs=[(-2, -2), (0, 0)]) == EINVAL                # a negative dim
    assert _probe(lib, ok, 40, 2, 2, pairs=[(2, -2), (0, 0)]) == EINVAL
    assert _probe(lib, ok, 40, 2, 2, pairs=[(2, 3), (0, 0)]) == EINVAL                  # B1 * B2 != B
    assert _probe(lib, ok, 40, 2, 2, pairs=[(4, 0), (0, 0)]) == EINVAL                  # order 4 with B2 = 0
    assert _probe(lib, ok, 40, 2, 2, pairs=[(2, 2), (5, 1)]) == EINVAL                  # another order with B2 > 0
    assert _probe(lib, ok, 40, 2, 2, orders=[5, 2]) == EINVAL                           # order > 4
    assert _probe(lib, [(6, 5), (7,)], 40, 2, 2) == EINVAL                              # no block of order 4: the existing entry's call
    assert _probe(lib, ok, 40, 2, 2, nm=0) == EINVAL                                    # no models
    assert _probe(lib, [(3, 2, 2), (2, 7)], 40, 2, 2, orders=[4, 2]) == EINVAL          # a matrix block has A = 1
    assert _probe(lib, [(4, 3, 1), (5,)], 40, 2, 2) == EWORKSPACE                       # B2 = 1 is still a tensor
    assert _probe(lib, [(1, 3, 2), (3, 1, 2)], 40, 2, 2) == EWORKSPACE                  # unit modes
    arr, _, _, pairs = _blocks(ok)
    for fn in (lib.cmtfpls_cv_masked_coupled_tensor_workspace_bytes, lib.cmtfpls_cv_masked_coupled_tensor_lds_bytes):
        assert fn(arr, 2, _ints(pairs), 40, 3, 2) > 0
        assert fn(arr, 2, None, 40, 3, 2) == 0 and fn(arr, 2, _ints([(2, 3), (0, 0)]), 40, 3, 2) == 0
        assert fn(arr, 2, _ints(pairs), 1, 3, 2) == 0 and fn(arr, 9, _ints(pairs + [(0, 0)] * 7), 40, 3, 2) == 0


def test_c_entry_limits(lib):
    assert MAX_BLOCKS == 8
    assert _short_side(64, 8, 8) == 64 and _short_side(65, 13, 5) == 65
    assert _probe(lib, [(64, 8, 8), (7,)], 12, 2, 2) == EWORKSPACE                      # the largest short side = 64: mode 0
    assert _probe(lib, [(32, 64, 2), (7,)], 12, 2, 1) == EWORKSPACE                     # ... mode 1
    assert _probe(lib, [(32, 2, 64), (7,)], 12, 2, 1) == EWORKSPACE                     # ... mode 2
    assert _probe(lib, [(65, 13, 5), (7,)], 8, 2, 1) == EUNSUPPORTED                    # 65
    assert _probe(lib, [(33, 65, 2), (7,)], 8, 2, 1) == EUNSUPPORTED
    assert _probe(lib, [(33, 2, 65), (7,)], 8, 2, 1) == EUNSUPPORTED
    assert _probe(lib, [(3, 2, 2), (64, 64)], 24, 2, 2) == EWORKSPACE                   # a matrix block's min(A, B) = 64
    assert _probe(lib, [(3, 2, 2), (65, 65)], 8, 2, 1) == EUNSUPPORTED
    assert _probe(lib, [(3, 2, 2), (5,)], 40, 64, 2) == EWORKSPACE                      # M = 64
    assert _probe(lib, [(3, 2, 2), (5,)], 40, 65, 2) == EUNSUPPORTED
    assert _probe(lib, [(3, 2, 2), (5,)], 40, 2, 16) == EWORKSPACE                      # R = 16
    assert _probe(lib, [(3, 2, 2), (5,)], 40, 2, 17) == EUNSUPPORTED
    assert _probe(lib, [(3, 2, 2)] + [(3, 2)] * 7, 40, 2, 2) == EWORKSPACE              # nb = 8 with one tensor block
    assert _probe(lib, [(3, 2, 2)] + [(3, 2)] * 8, 40, 2, 2) == EUNSUPPORTED
    trailing = [(4000,), (3, 2, 2)]
    arr, _, _, pairs = _blocks(trailing)
    I = 2
    while lib.cmtfpls_cv_masked_coupled_tensor_lds_bytes(arr, 2, _ints(pairs), I + 1, 2, 1) <= LDS_CAP:
        I += 1
    assert _probe(lib, trailing, I, 2, 1) == EWORKSPACE                                 # the LDS at its cap (the library's own count)
    assert _probe(lib, trailing, I + 1, 2, 1) == EUNSUPPORTED
    assert _probe(lib, [(1, 1, 1 << 30)], 40, 2, 1) == EUNSUPPORTED                     # short sides of 1, and nothing that fits


def test_host_lds_and_workspace_formulas_are_the_librarys(lib):
    rng = np.random.default_rng(0)
    seen = set()
    for _ in range(300):
        nb = int(rng.integers(1, 9))
        trailing = []
        for b in range(nb):
            kind = rng.random()
            if b == 0 or kind < 0.3:                                                    # at least one block of order 4
                trailing.append(tuple(int(v) for v in rng.integers(1, 14, size=3)))
            elif kind < 0.6:
                trailing.append((int(rng.integers(1, 2500)),))
            else:
                trailing.append((int(rng.integers(1, 70)), int(rng.integers(1, 90))))
        if rng.random() < 0.2:
            trailing[0] = (int(rng.integers(60, 70)), int(rng.integers(1, 10)), int(rng.integers(8, 12)))
        order = rng.permutation(nb)
        trailing = [trailing[i] for i in order]
        I, M, R = int(rng.integers(2, 1500)), int(rng.integers(1, 65)), int(rng.integers(1, 17))
        arr, _, dims, pairs = _blocks(trailing)
        want = _carve_up(dims, pairs, I, M, R)
        assert lib.cmtfpls_cv_masked_coupled_tensor_lds_bytes(arr, nb, _ints(pairs), I, M, R) == want, (trailing, I, M, R)
        assert lib.cmtfpls_cv_masked_coupled_tensor_workspace_bytes(arr, nb, _ints(pairs), I, M, R) == \
            _workspace(dims, pairs, I, M, R), (trailing, I, M, R)
        sides = [_short_side(*t) if len(t) == 3 else min(A, B) for t, (A, B) in zip(trailing, dims)]
        fits = max(sides) <= 64 and want <= LDS_CAP
        assert _probe(lib, trailing, I, M, R) == (EWORKSPACE if fits else EUNSUPPORTED), (trailing, I, M, R)
        seen.add(fits)
    assert seen == {True, False}
    # one tensor block next to nothing: the order-3 coupled formula at 512 partials, ys gone, plus the CP's vectors and argmax scratch
    I, (A, B1, B2), M, R = 40, (6, 5, 4), 3, 2
    B, n = B1 * B2, _short_side(A, B1, B2)
    arr, _, _, pairs = _blocks([(A, B1, B2)])
    assert lib.cmtfpls_cv_masked_coupled_tensor_lds_bytes(arr, 1, _ints(pairs), I, M, R) == 8 * (
        3 * I + 3 * M + 2 * R * R + R * M + 3 * R + 512 + A * B + 2 * n * n + n + (B1 + B2 + B + max(A, B1, B2) + 12) + (R + 1) * (A + B) + I)
    arr, _, _, pairs = _blocks([(A, B1, B2), (7,)])
    assert lib.cmtfpls_cv_masked_coupled_tensor_workspace_bytes(arr, 2, _ints(pairs), I, M, R) == 8 * (
        (I + 2) * 120 + (I + 2) * 7 + I * M + I * R + 4 * 120)
