"""CPU-only: the hold-out rule's restatement (tests/impute_ref.py), and validate.impute / get_q2x_heldout on the NumPy test backend
(the torch form of the three passes, which shares the package's own restatement of the counter rule) against a literal host
loop; the argument errors and the agreement of header, binding table and backend on the new entries."""
import os
import re

import numpy as np
import pytest
import torch

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.imputation import holdout_mask_host
from cmtf_pls_amd.validate import get_q2x_heldout, impute
from impute_ref import holdout_mask, literal_q2x, masked_copy
from numpy_backend import NumpyBackend
from philox_ref import nan_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(shape, nan, seed, R=3):
    x, y, cp = O.import_synthetic(shape, 3, R, error=0.3, seed=seed)
    if nan:
        x[np.random.default_rng(seed).random(x.shape) < nan] = np.nan
    return x, y, cp


def _coupled(nan, seed):
    x, y, cp = _data((60, 8, 6), nan, seed)
    rng = np.random.default_rng(seed + 1)
    xm = cp.factors[0] @ rng.normal(size=(5, 3)).T + 0.2 * rng.normal(size=(60, 5))
    x4 = np.einsum("ir,jr,kr,lr->ijkl", cp.factors[0], *(rng.normal(size=(d, 3)) for d in (3, 2, 4))) + 0.2 * rng.normal(size=(60, 3, 2, 4))
    if nan:
        xm[rng.random(xm.shape) < nan] = np.nan
        x4[rng.random(x4.shape) < nan] = np.nan
    return [x, xm, x4], y


# ---- the rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fraction", [0.1, 0.5])
def test_mask_density(fraction):
    n = 100000
    k = int(holdout_mask(0, n, 215, 2, fraction).sum())
    assert abs(k - n * fraction) <= 4 * np.sqrt(n * fraction * (1 - fraction))


def test_mask_independent_of_the_synthetic_streams_and_of_other_blocks():
    n, seed = 100000, 99
    m2 = holdout_mask(0, n, seed, 2, 0.3)
    assert not np.array_equal(m2, nan_mask(0, n, seed, 0.3))                                   # stream 1: add_noise's NaN mask
    assert not np.array_equal(m2, holdout_mask(0, n, seed, 0, 0.3))                            # stream 0: add_noise's noise
    assert not np.array_equal(m2, holdout_mask(0, n, seed, 3, 0.3))                            # the next block
    for other in (nan_mask(0, n, seed, 0.3), holdout_mask(0, n, seed, 3, 0.3)):
        both = int((m2 & other).sum())                                                         # independent: P(both) = 0.09
        assert abs(both - n * 0.09) <= 4 * np.sqrt(n * 0.09 * 0.91)


@pytest.mark.parametrize("P", [48, 35])
def test_mask_shard_consistency(P):
    I, a, b, seed = 41, 7, 30, 2 ** 40 + 17
    whole = holdout_mask(0, I * P, seed, 2, 0.25).reshape(I, P)
    assert np.array_equal(holdout_mask(a * P, (b - a) * P, seed, 2, 0.25).reshape(b - a, P), whole[a:b])
    assert (a * P) % 4 != 0 or P % 4 == 0                                                      # P = 35: the shard starts inside a Philox block


@pytest.mark.parametrize("first,n", [(0, 1000), (5, 999), (2 ** 33 + 3, 4097), (7, 1)])
def test_package_restatement_is_the_same_rule(first, n):
    for seed in (0, 215, 2 ** 63 - 1):
        assert np.array_equal(holdout_mask_host(first, n, seed, 4, 0.37), holdout_mask(first, n, seed, 4, 0.37))


# ---- impute ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(30, 9), (28, 6, 5), (26, 4, 3, 5)])
def test_impute_tpls_against_reconstruction(shape):
    x, y, _ = _data(shape, 0.15, 3)
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    gap = np.isnan(x)
    filled = impute(m)
    assert isinstance(filled, np.ndarray) and filled.dtype == x.dtype and filled.shape == x.shape
    assert np.array_equal(filled[~gap], x[~gap]) and np.isfinite(filled).all()
    np.testing.assert_allclose(filled[gap], m.X_reconstructed()[gap], rtol=1e-12, atol=1e-12)
    rep = m.imputation_report_
    assert rep["form"] == "torch fallback" and "impute kernel" in rep["why"] and rep["imputed"] == [int(gap.sum())] and rep["x_reads"] == [1]
    xn, _, _ = _data((11,) + shape[1:], 0.2, 8)                                # new rows, some with missing values
    fn = impute(m, xn)
    T = m.transform(xn)
    want = (T @ _kr(m.X_factors[1:]).T).reshape(xn.shape) + m.X_mean
    gn = np.isnan(xn)
    assert np.array_equal(fn[~gn], xn[~gn])
    np.testing.assert_allclose(fn[gn], want[gn], rtol=1e-12, atol=1e-12)
    assert m.imputation_report_["imputed"] == [int(gn.sum())] and m.imputation_report_["rows"] == 11


def _kr(loadings):
    W = loadings[0]
    for L in loadings[1:]:
        W = (W[:, None, :] * L[None, :, :]).reshape(-1, W.shape[1])
    return W


def test_impute_ctpls_and_tensor_input():
    Xs, y = _coupled(0.15, 4)
    m = ctPLS(3, backend=NumpyBackend())
    m.fit(Xs, y)
    filled = impute(m)
    rec = m.Xs_reconstructed()
    assert len(filled) == 3 and m.imputation_report_["imputed"] == [int(np.isnan(x).sum()) for x in Xs]
    for x, f, r in zip(Xs, filled, rec):
        gap = np.isnan(x)
        assert np.array_equal(f[~gap], x[~gap])
        np.testing.assert_allclose(f[gap], r[gap], rtol=1e-12, atol=1e-12)
    xt = torch.from_numpy(Xs[0].copy())                                          # a tensor in: a new tensor out, the caller's only read
    k = tPLS(3, backend=NumpyBackend())
    k.fit(xt, y)
    before = xt.clone()
    ft = impute(k)
    assert isinstance(ft, torch.Tensor) and ft.data_ptr() != xt.data_ptr() and ft.dtype == torch.float64
    assert torch.equal(torch.nan_to_num(xt, nan=7.5), torch.nan_to_num(before, nan=7.5))
    assert k.imputation_report_["in_place_on_private_copy"] == [False]
    gap = np.isnan(Xs[0])
    assert np.array_equal(ft.numpy()[~gap], Xs[0][~gap]) and np.isfinite(ft.numpy()).all()


# ---- get_q2x_heldout ------------------------------------------------------------------------------------------------------------
def test_q2x_tpls_against_the_literal_loop():
    x, y, _ = _data((40, 7, 6), 0.1, 5)
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    T0, mean0 = m.X_factors[0].copy(), m.X_mean.copy()
    out = get_q2x_heldout(m, fraction=0.2, n_repeats=3, random_state=11)
    assert np.array_equal(out["seeds"], np.random.default_rng(11).integers(0, 2 ** 63, 3))
    sums, q2x, q2x_all, _ = literal_q2x(lambda: tPLS(3, backend=NumpyBackend()), x, y, 3, 0.2, out["seeds"])
    assert out["q2x"].shape == (3, 1, 3) and out["q2x_all"].shape == (3, 3)
    np.testing.assert_allclose(out["q2x"], q2x, rtol=0, atol=1e-8)
    np.testing.assert_allclose(out["q2x_all"], q2x_all, rtol=0, atol=1e-8)
    assert np.array_equal(out["n_heldout"], sums[:, :, -1].astype(np.int64))
    assert np.array_equal(out["n_heldout"][:, 0], [masked_copy(x, 0.2, int(s))[1][0] for s in out["seeds"]])
    np.testing.assert_allclose(out["mean"], q2x.mean(axis=0), atol=1e-8)
    np.testing.assert_allclose(out["std"], q2x.std(axis=0, ddof=1), atol=1e-8)
    rep = m.q2x_report_
    assert rep is out["report"] and rep["form"] == "torch fallback" and "heldout_resid kernel" in rep["why"]
    assert rep["mask"] == "host restatement of the counter rule" and rep["repeats"] == 3
    assert np.array_equal(m.X_factors[0], T0) and np.array_equal(m.X_mean, mean0) and m.original_X is x      # the model is untouched
    again = get_q2x_heldout(m, fraction=0.2, n_repeats=3, random_state=11)
    assert np.array_equal(again["q2x"], out["q2x"]) and np.array_equal(again["n_heldout"], out["n_heldout"])
    other = get_q2x_heldout(m, fraction=0.2, n_repeats=3, random_state=12)
    assert not np.array_equal(other["seeds"], out["seeds"]) and not np.array_equal(other["q2x"], out["q2x"])
    one = get_q2x_heldout(m, fraction=0.2, n_repeats=1, random_state=11)
    assert np.isnan(one["std"]).all() and np.array_equal(one["q2x"][0], out["q2x"][0])


def test_q2x_ctpls_against_the_literal_loop():
    Xs, y = _coupled(0.1, 6)
    m = ctPLS(3, backend=NumpyBackend())
    m.fit(Xs, y)
    out = get_q2x_heldout(m, fraction=0.1, n_repeats=2, random_state=3)
    sums, q2x, q2x_all, _ = literal_q2x(lambda: ctPLS(3, backend=NumpyBackend()), Xs, y, 3, 0.1, out["seeds"])
    assert out["q2x"].shape == (2, 3, 3)
    np.testing.assert_allclose(out["q2x"], q2x, rtol=0, atol=1e-8)
    np.testing.assert_allclose(out["q2x_all"], q2x_all, rtol=0, atol=1e-8)
    assert np.array_equal(out["n_heldout"], sums[:, :, -1].astype(np.int64))
    for b in range(3):                                                            # every block has a stream of its own
        assert out["n_heldout"][0, b] == masked_copy(Xs[b], 0.1, int(out["seeds"][0]), block=b)[1][0]


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    x, y, _ = _data((20, 5, 4), 0.0, 9)
    m = tPLS(2, backend=NumpyBackend())
    with pytest.raises(ValueError, match="impute needs a fitted"):
        impute(m)
    with pytest.raises(ValueError, match="get_q2x_heldout needs a fitted"):
        get_q2x_heldout(m)
    m.fit(x, y)
    for f in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match=r"fraction must be in \(0, 1\)"):
            get_q2x_heldout(m, fraction=f)
    for n in (0, -1, 1.5):
        with pytest.raises(ValueError, match="n_repeats must be an integer >= 1"):
            get_q2x_heldout(m, n_repeats=n)
    with pytest.raises(ValueError, match=r"Training X has shape \(20, 5, 4\), while the new X has shape \(3, 4, 5\)"):
        impute(m, np.zeros((3, 4, 5)))
    k = tPLS(2, backend=NumpyBackend(), copy_X=False)
    k.fit(torch.from_numpy(x.copy()), y)
    with pytest.raises(ValueError, match="copy_X=False"):
        impute(k)
    with pytest.raises(ValueError, match="copy_X=False"):
        get_q2x_heldout(k)
    assert np.isfinite(impute(k, x[:4])).all()                                    # new rows need no kept X
    c = ctPLS(2, backend=NumpyBackend())
    c.fit([x, x[:, :, 0]], y)
    with pytest.raises(ValueError, match="Training Xs has 2 blocks, while the new Xs has 1"):
        impute(c, [x])


def test_a_sample_left_without_observations_is_named():
    x, y, _ = _data((30, 2), 0.0, 10)                                             # two entries per sample: 0.7^2 of the rows lose both
    m = tPLS(1, backend=NumpyBackend())
    m.fit(x, y)
    seed = int(np.random.default_rng(0).integers(0, 2 ** 63, 1)[0])
    row = int(np.nonzero(holdout_mask(0, 60, seed, 2, 0.7).reshape(30, 2).all(axis=1))[0][0])
    with pytest.raises(ValueError, match=rf"repeat 0 \(seed {seed}\): sample {row} has no observed entry left in block 0"):
        get_q2x_heldout(m, fraction=0.7, n_repeats=1, random_state=0)


def test_sharded_model_is_refused():
    x, y, _ = _data((20, 5, 4), 0.0, 9)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)

    class TwoRanks:
        world, rank, sharded = 2, 0, True

        def allreduce(self, t):
            return t

    m._get_engine().comm = TwoRanks()
    with pytest.raises(NotImplementedError, match="sharded model"):
        get_q2x_heldout(m)


# ---- the entries' names ---------------------------------------------------------------------------------------------------------
def test_header_binding_table_and_backend_agree_on_the_new_entries():
    from cmtf_pls_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cmtfpls.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cmtfpls_\w+)\s*\(", text))
    backend = open(os.path.join(ROOT, "cmtf_pls_amd", "backend.py")).read()
    for base in ("holdout_mask", "heldout_resid", "impute"):
        names = {f"cmtfpls_{base}_f32", f"cmtfpls_{base}_f64", f"cmtfpls_{base}_workspace_bytes"}
        assert names <= declared and names <= set(_lib.SIGNATURES)
        assert re.search(rf"def {base}\(self", backend) and f'self._fn("{base}"' in backend and f"cmtfpls_{base}_workspace_bytes" in backend
    assert _lib.SIGNATURES["cmtfpls_holdout_mask_f32"] == _lib.SIGNATURES["cmtfpls_holdout_mask_f64"]
    units = open(os.path.join(ROOT, "cmtf_pls_amd", "csrc", "build.sh")).read()
    assert re.search(r"for src in [^;]*\bimpute\b", units)
    lib = _lib.load()
    assert lib.cmtfpls_abi_version() == 1
    assert lib.cmtfpls_holdout_mask_workspace_bytes(10 ** 9) >= 16 and lib.cmtfpls_holdout_mask_workspace_bytes(0) == 0
    assert lib.cmtfpls_heldout_resid_workspace_bytes(65536, 16384, 10) % (12 * 8) == 0
    assert lib.cmtfpls_impute_workspace_bytes(65536, 16384) > 0
