"""CPU-only: contribution plots (validate.sample_contributions) on the NumPy test backend, i.e. the torch form of the
contribution pass, against a float64 NumPy restatement (tests/contributions_ref.py); the identities of DESIGN 8l (mode sums
close to the SPE of sample_diagnostics and, on complete data, to t2_closure), the cells, planted faults and the argument errors."""
import numpy as np
import pytest

import oracle as O
from cmtf_pls_amd import ctPLS, tPLS
from cmtf_pls_amd.validate import sample_contributions, sample_diagnostics
from contributions_ref import check, contributions
from numpy_backend import NumpyBackend


def _data(shape, nan, seed):
    x, y, cp = O.import_synthetic(shape, 3, 3, error=0.3, seed=seed)
    if nan:
        x[np.random.default_rng(seed).random(x.shape) < nan] = np.nan
    return x, y, cp


def _coupled(nan, seed=4):
    x, y, cp = _data((30, 6, 5), nan, seed)
    xm = cp.factors[0] @ np.random.default_rng(1).normal(size=(7, 3)).T + 0.2 * np.random.default_rng(2).normal(size=(30, 7))
    if nan:
        xm[np.random.default_rng(seed + 1).random(xm.shape) < nan] = np.nan
    m = ctPLS(3, backend=NumpyBackend())
    m.fit([x, xm], y)
    return m, [x, xm], y


@pytest.mark.parametrize("shape,nan", [((30, 9), 0.0), ((28, 6, 5), 0.0), ((28, 6, 5), 0.1), ((26, 4, 3, 5), 0.0)])
def test_tpls_against_restatement(shape, nan):
    x, y, _ = _data(shape, nan, 3)
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    c = sample_contributions(m)
    check(c, contributions(m, train=x), False, 1e-10)
    rep = m.contributions_report_
    assert rep["form"] == ["torch fallback"] and rep["x_reads"] == [1] and rep["rows"] == shape[0] and rep["why"][0]
    assert len(c["spe_mode"]) == len(shape) - 1 and [a.shape for a in c["t2_mode"]] == [(shape[0], d) for d in shape[1:]]
    xn, _, _ = _data((12,) + shape[1:], nan, 8)
    cn = sample_contributions(m, xn)
    check(cn, contributions(m, xn), False, 1e-10)
    assert np.array_equal(cn["scores"], m.transform(xn)) and m.contributions_report_["training_stats"] == "cached"
    rows = np.random.default_rng(0).permutation(12)[:7]
    cs = sample_contributions(m, xn, rows=rows)
    check(cs, contributions(m, xn, rows=rows), False, 1e-10)
    for k in range(len(shape) - 1):
        np.testing.assert_array_equal(cs["spe_mode"][k], cn["spe_mode"][k][rows])
    trows = np.random.default_rng(1).permutation(shape[0])[:9]
    check(sample_contributions(m, rows=trows), contributions(m, rows=trows, train=x), False, 1e-10)


@pytest.mark.parametrize("nan", [0.0, 0.1])
def test_ctpls_against_restatement(nan):
    m, Xs, y = _coupled(nan)
    c = sample_contributions(m)
    check(c, contributions(m, train=Xs), True, 1e-10)
    assert len(c["spe_mode"]) == 2 and len(c["spe_mode"][0]) == 2 and len(c["spe_mode"][1]) == 1
    assert m.contributions_report_["x_reads"] == [1, 1]
    Xn = [Xs[0][:10] + 0.1, Xs[1][:10] - 0.1]
    rows = np.array([7, 2, 9, 0])
    check(sample_contributions(m, Xn, rows=rows), contributions(m, Xn, rows=rows), True, 1e-10)


@pytest.mark.parametrize("shape,nan,coupled", [((30, 9), 0.1, False), ((28, 6, 5), 0.1, False), ((26, 4, 3, 5), 0.1, False),
                                               ((30, 6, 5), 0.1, True)])
def test_spe_modes_sum_to_the_spe_of_sample_diagnostics(shape, nan, coupled):
    if coupled:
        m, X, _ = _coupled(nan)
    else:
        X, y, _ = _data(shape, nan, 5)
        m = tPLS(3, backend=NumpyBackend())
        m.fit(X, y)
    d, c = sample_diagnostics(m), sample_contributions(m)
    np.testing.assert_allclose(c["t2"], d["t2"], rtol=1e-12, atol=1e-12)
    for spe, modes, got in zip(*[v if coupled else [v] for v in (d["spe"], c["spe_mode"], c["spe"])]):
        np.testing.assert_allclose(got, spe, rtol=1e-10)
        for a in modes:
            np.testing.assert_allclose(a.sum(axis=1), spe, rtol=1e-10)


@pytest.mark.parametrize("shape,coupled", [((30, 9), False), ((28, 6, 5), False), ((26, 4, 3, 5), False), ((30, 6, 5), True)])
def test_t2_modes_close_on_complete_data(shape, coupled):
    if coupled:
        m, X, _ = _coupled(0.0)
        Xn = [X[0][:8] * 1.1 + 0.05, X[1][:8] * 0.9]
    else:
        X, y, _ = _data(shape, 0.0, 6)
        m = tPLS(3, backend=NumpyBackend())
        m.fit(X, y)
        Xn = _data((8,) + shape[1:], 0.0, 9)[0]
    for c in (sample_contributions(m), sample_contributions(m, Xn)):
        # the training scores of a fit on complete data have zero mean: the closure is t2 itself
        np.testing.assert_allclose(c["t2_closure"], c["t2"], rtol=1e-8, atol=1e-10)
        blocks = c["t2_mode"] if coupled else [c["t2_mode"]]
        for k in range(len(blocks[0])):
            if coupled and k >= 1:
                continue                                    # blocks share only the sample mode: compare mode 0 of every block
            total = sum(b[k].sum(axis=1) for b in blocks)
            np.testing.assert_allclose(total, c["t2_closure"], rtol=1e-8, atol=1e-10)
        if coupled:                                         # any one mode per block: the block totals add up as well
            total = blocks[0][1].sum(axis=1) + blocks[1][0].sum(axis=1)
            np.testing.assert_allclose(total, c["t2_closure"], rtol=1e-8, atol=1e-10)


def test_cells_sum_to_the_modes_and_the_size_limit():
    x, y, _ = _data((26, 4, 3, 5), 0.1, 7)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    rows = np.array([3, 20, 11])
    c = sample_contributions(m, rows=rows, cells=True)
    want = contributions(m, rows=rows, train=x)
    assert c["spe_cells"].shape == (3, 4, 3, 5) and c["t2_cells"].shape == (3, 4, 3, 5)
    np.testing.assert_allclose(c["spe_cells"], want["spe_cells"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(c["t2_cells"], want["t2_cells"], rtol=1e-8, atol=1e-12)
    for k, others in enumerate([(2, 3), (1, 3), (1, 2)]):
        np.testing.assert_allclose((c["spe_cells"] ** 2).sum(axis=others), c["spe_mode"][k], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(c["t2_cells"].sum(axis=others), c["t2_mode"][k], rtol=1e-10, atol=1e-13)
    mc, Xs, _ = _coupled(0.1)
    cc = sample_contributions(mc, rows=[1, 2], cells=True)
    assert cc["spe_cells"][0].shape == (2, 6, 5) and cc["t2_cells"][1].shape == (2, 7)
    from cmtf_pls_amd import contributions as C

    old = C.MAX_CELLS
    C.MAX_CELLS = 26 * 60 - 1
    try:
        with pytest.raises(ValueError, match="limit"):
            sample_contributions(m, cells=True)
        sample_contributions(m, rows=rows, cells=True)
    finally:
        C.MAX_CELLS = old
    assert old == 1 << 28


def _margin(v, at):
    rest = np.delete(v, at)
    return v[at] / max(rest.max(), 1e-300)


def test_planted_faults_point_at_their_slices():
    x, y, _ = _data((40, 7, 6), 0.0, 11)
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    js, ks = 4, 2
    xn = x[5:6].copy()
    xn[0, js, ks] += 25.0 * x.std()
    ref = contributions(m, xn)
    assert _margin(ref["spe_mode"][0][0], js) > 3 and _margin(ref["spe_mode"][1][0], ks) > 3      # the restatement shows it clearly
    c = sample_contributions(m, xn)
    assert int(np.argmax(c["spe_mode"][0][0])) == js and int(np.argmax(c["spe_mode"][1][0])) == ks
    WA, WB = m.X_factors[1], m.X_factors[2]
    jt = int(np.argmax(np.abs(WA[:, 0])))
    xt = x[9:10].copy()
    xt[0, jt, :] += 30.0 * x.std() * np.sqrt(WB.shape[0]) * np.sign(WA[jt, 0]) * WB[:, 0]          # along W[:, 0], slice jt only
    ref = contributions(m, xt)
    assert _margin(ref["t2_mode"][0][0], jt) > 3
    c = sample_contributions(m, xt)
    assert int(np.argmax(c["t2_mode"][0][0])) == jt
    assert c["t2"][0] > 10 * sample_contributions(m, x[9:10])["t2"][0]


def test_argument_errors():
    x, y, _ = _data((20, 5, 4), 0.0, 9)
    m = tPLS(2, backend=NumpyBackend())
    m.fit(x, y)
    for bad in ([0, 0], [-1], [20], [[0, 1]], [0.5], np.array([True, False])):
        with pytest.raises(ValueError, match="rows"):
            sample_contributions(m, rows=bad)
    with pytest.raises(ValueError, match="rows"):
        sample_contributions(m, x[:3], rows=[3])
    with pytest.raises(ValueError, match=r"Training X has shape \(20, 5, 4\), while the new X has shape \(3, 4, 5\)"):
        sample_contributions(m, np.zeros((3, 4, 5)))
    with pytest.raises(ValueError, match="fitted"):
        sample_contributions(tPLS(2, backend=NumpyBackend()))
    import torch

    k = tPLS(2, backend=NumpyBackend(), copy_X=False)
    k.fit(torch.from_numpy(x.copy()), y)
    with pytest.raises(ValueError, match="copy_X=False"):
        sample_contributions(k)
    assert sample_contributions(k, x[:4])["spe_mode"][0].shape == (4, 5)
    empty = sample_contributions(m, rows=np.zeros(0, dtype=np.int64))
    assert empty["spe_mode"][0].shape == (0, 5) and empty["t2"].shape == (0,)
