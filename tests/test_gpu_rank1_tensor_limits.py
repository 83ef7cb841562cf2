"""cmtfpls_rank1_tensor_f64 (csrc/rank1_tensor.hip: unfold_kernel, the matrix rank-1 init of every unfolding, cp_rank1_als_kernel)
at every declared order, at its size limits, at its stop rule and on its declines; the fit on top of it at the declared top
order; and what the entry does when the one-launch chain of squarings of an init gives up.

How the ALS is isolated from the init.  The test reproduces the device's init outside the entry: for each mode it uploads the
host-made unfolding (rank1_tensor_ref.unfold, the statement of unfold_kernel) and calls backend.rank1 -- the function the
entry calls, with the same squaring budget, hence the same bits -- and keeps wA.  The long-double ALS of rank1_tensor_ref is then
run from exactly these vectors.  A wrong unfold_kernel gives the entry another init than the test's and an O(1) disagreement.

Per case: every factor entry within bound = 16 max(d_case, 2^-52) of the long-double reference, where d_case =
max |als(float64) - als(long double)| from the same init is measured on the host (never against the kernel); 16 because the kernel
sums 64-lane strided partials through a butterfly with fma where NumPy sums pairwise -- both random walks of a few roundings.
info = [1, sweeps] with the reference's sweep count exactly (every case's stop decision has a margin >= 1e-11, asserted here
from the device's init as tests/test_rank1_tensor_ref_cpu.py asserts it from the oracle's); the columns of `factors` past
dims[m] keep their sentinel (ld = max(dims) + 3).

Norms.  The sweep loop leaves through its stop rule BEFORE the normalisation (oracle.rank1_factors does the same), so after a
STOPPED run the factors are the last sweep's raw output, |f| = 1 only to the convergence level (measured on the host: up to 9e-7
for the `noise` cases); they are compared with the reference only.  A run that reaches the cap of 100 ends on a normalisation:
there every factor has norm 1 to 1e-14.

Measured on the MI355X (err = max |kernel - long double| over all factor entries; bound = 16 max(d_case, 2^-52)):

  case                          d_case    bound     err       sweeps
  9x8x7-strong                  2.76e-16  4.41e-15  2.76e-16  4
  9x8x7-close                   1.34e-16  3.55e-15  2.24e-16  32
  9x8x7-noise                   4.31e-16  6.89e-15  2.08e-16  86
  5x4x3x2-strong                3.37e-16  5.40e-15  2.48e-16  4
  5x4x3x2-close                 3.15e-16  5.04e-15  2.40e-16  23
  5x4x3x2-noise                 3.55e-16  5.68e-15  3.20e-16  13
  3x2x4x2x3-strong              2.56e-16  4.10e-15  5.41e-16  4
  3x2x4x2x3-close               3.83e-16  6.13e-15  4.21e-16  9
  3x2x4x2x3-noise               5.80e-16  9.29e-15  2.11e-16  14
  2x3x2x2x3x2-strong            3.53e-16  5.64e-15  2.95e-16  4
  2x3x2x2x3x2-close             5.99e-16  9.58e-15  3.12e-16  8
  2x3x2x2x3x2-noise             3.28e-16  5.25e-15  1.11e-15  15
  2x2x2x2x2x2x3-strong          7.71e-16  1.23e-14  3.46e-16  4
  2x2x2x2x2x2x3-close           3.94e-16  6.30e-15  4.60e-16  7
  2x2x2x2x2x2x3-noise           5.58e-16  8.93e-15  4.47e-16  12
  4x1x5-strong                  2.22e-16  3.55e-15  1.58e-16  3
  4x1x5-close                   2.22e-16  3.55e-15  2.22e-16  3
  4x1x5-noise                   1.34e-16  3.55e-15  3.16e-16  3
  1x6x5-strong                  2.22e-16  3.55e-15  5.44e-17  3
  1x6x5-close                   2.22e-16  3.55e-15  1.19e-16  3
  1x6x5-noise                   4.44e-16  7.11e-15  2.36e-16  3
  6x5x1-strong                  1.28e-16  3.55e-15  1.28e-16  3
  6x5x1-close                   2.22e-16  3.55e-15  2.22e-16  3
  6x5x1-noise                   3.47e-16  5.55e-15  2.22e-16  3
  70x3x65-strong                1.92e-16  3.55e-15  1.90e-16  3
  70x3x65-close                 1.17e-16  3.55e-15  9.13e-17  38
  70x3x65-noise                 4.04e-16  6.46e-15  1.51e-16  37
  300x20x15-strong              6.20e-16  9.93e-15  1.57e-16  3
  300x20x15-close               4.62e-16  7.39e-15  1.02e-16  7
  300x20x15-noise               1.39e-15  2.23e-14  1.71e-16  83
  1024x3x2-strong               2.37e-15  3.79e-14  2.21e-16  3
  1024x3x2-close                9.38e-16  1.50e-14  2.72e-16  12
  1024x3x2-noise                2.12e-15  3.39e-14  3.12e-16  100
  2x1024x3-strong               1.25e-15  1.99e-14  5.13e-16  3
  2x1024x3-close                1.20e-15  1.92e-14  2.01e-16  7
  2x1024x3-noise                5.22e-16  8.36e-15  1.23e-16  81
  3x2x1024-strong               4.56e-16  7.30e-15  2.34e-16  3
  3x2x1024-close                6.34e-16  1.01e-14  6.34e-16  20
  3x2x1024-noise                5.73e-16  9.16e-15  2.04e-16  35
  17x16x15x3-strong             6.71e-16  1.07e-14  3.29e-16  3
  17x16x15x3-close              6.64e-16  1.06e-14  1.19e-16  6
  17x16x15x3-noise              8.11e-16  1.30e-14  1.08e-16  87
  48x40x36-strong               2.27e-16  3.63e-15  7.13e-17  3
  9x8x7-noise-tol0              1.52e-16  3.55e-15  1.60e-16  100
  9x8x7-close-tol0.01           3.04e-16  4.87e-15  9.53e-17  2
  9x8x7-strong-sq2              3.87e-16  6.19e-15  3.16e-16  4
  9x8x7-close-sq2               1.68e-16  3.55e-15  4.18e-16  32
  17x16x15x3-close-view         6.64e-16  1.06e-14  1.19e-16  6

No case needs more than the factor 16: the largest err / bound is 0.21 (2x3x2x2x3x2-noise).
"""
import ctypes
import inspect

import numpy as np
import pytest
import torch
from numpy.testing import assert_allclose

import oracle as O
import rank1_tensor_ref as R
from oracle import nipals_oracle as NO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.25e300
EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4          # include/cmtfpls.h


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


@pytest.fixture(scope="module")
def api():
    import cmtf_pls_amd
    return cmtf_pls_amd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def _full(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float64, device=DEV)


def _device_init(be, Z, budget):
    """The init vectors of the entry, made outside it: backend.rank1 on the host-made unfolding of every mode."""
    init, conv = [], []
    for m, d in enumerate(Z.shape):
        unf = R.unfold(Z, m)
        wA, wB, info = _full(d), _full(unf.shape[1]), _full(2)
        be.rank1(_dev(unf.ravel()), d, unf.shape[1], wA, wB, info=info, n_squarings=budget)
        init.append(wA.cpu().numpy())
        conv.append(info.cpu().numpy()[0])
    return init, conv


def _check(be, case, Z, dZ):
    dims = Z.shape
    init, conv = _device_init(be, Z, case.budget)
    d_case, want, sweeps, margin = R.spread(Z, init, case.tol)
    assert margin >= R.MIN_MARGIN, (case.name, margin)
    n, ld = len(dims), max(dims) + 3
    fac, info = _full(n, ld), _full(2)
    be.rank1_tensor(dZ, dims, case.tol, fac, info=info, n_squarings=case.budget)
    got, info = fac.cpu().numpy(), info.cpu().numpy()
    bound = 16.0 * max(d_case, 2.0 ** -52)
    err = max(float(np.max(np.abs(got[m, :d].astype(np.longdouble) - want[m]))) for m, d in enumerate(dims))
    print(f"{case.name:28s} d_case {d_case:.2e}  bound {bound:.2e}  err {err:.2e}  sweeps {int(info[1])} (reference {sweeps})")
    assert info.tolist() == [1.0, float(sweeps)], (case.name, info, sweeps)
    assert err <= bound, (case.name, err, bound)                      # (a NaN in got fails this)
    for m, d in enumerate(dims):
        assert np.all(got[m, d:] == SENTINEL), (case.name, m)
        if sweeps == R.MAX_SWEEPS:
            assert abs(np.linalg.norm(got[m, :d]) - 1.0) <= 1e-14, (case.name, m)
    if case.budget == 30:
        # the init itself (its squarings converged) against the oracle's SVD, at the tolerance of the matrix rank-1 tests
        assert all(c == 1.0 for c in conv), (case.name, conv)
        for m in range(n):
            assert_allclose(R.sign_rule(init[m]), NO._leading_left_singular(R.unfold(Z, m)), rtol=0, atol=1e-9, err_msg=f"{case.name} init {m}")


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_factors_sweeps_and_info_equal_the_long_double_als_from_the_devices_own_init(be, case):
    Z = R.make_z(case.dims, case.kind, case.seed)
    _check(be, case, Z, _dev(Z.ravel()))


def test_z_as_a_view_eight_bytes_into_its_allocation(be):
    """Mode 0's init reads Z in place (no unfolding copy): Z at an address that is no multiple of 16."""
    case = next(c for c in R.CASES if c.name == "17x16x15x3-close")
    Z = R.make_z(case.dims, case.kind, case.seed)
    buf = _full(Z.size + 1)
    view = buf[1:]
    view.copy_(_dev(Z.ravel()))
    assert view.data_ptr() % 16 == 8
    _check(be, case._replace(name=case.name + "-view"), Z, view)


def test_zero_z_gives_nan_factors_after_the_full_hundred_sweeps(be):
    """The oracle's 0 / 0 at the first update: NaN factors, a stop rule that never fires (NaN < tol is false), the cap."""
    dims = (4, 3, 2)
    want, sweeps, _ = R.als(np.zeros(dims), [np.eye(d)[0] for d in dims], 1e-8, dtype=np.float64)
    assert sweeps == R.MAX_SWEEPS and all(np.isnan(w).all() for w in want)
    fac, info = _full(3, 7), _full(2)
    be.rank1_tensor(torch.zeros(24, dtype=torch.float64, device=DEV), dims, 1e-8, fac, info=info)
    got = fac.cpu().numpy()
    assert info.cpu().tolist() == [1.0, 100.0]
    for m, d in enumerate(dims):
        assert np.isnan(got[m, :d]).all() and np.all(got[m, d:] == SENTINEL)


# ---- declines: a status, a message, nothing written -----------------------------------------------------------------------------
def _raw(be, dims, n=None, ld=None, ws_delta=0):
    """cmtfpls_rank1_tensor_f64 called directly; returns (status, factors, info, needed workspace bytes)."""
    lib = be.lib
    n = len(dims) if n is None else n
    arr = (ctypes.c_int * len(dims))(*dims)
    need = int(lib.cmtfpls_rank1_tensor_workspace_bytes(arr, n))
    ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=DEV)
    Z = torch.ones(max(int(np.prod(dims)), 1), dtype=torch.float64, device=DEV)
    width = max(max(dims), 1)
    fac, info = _full(max(len(dims), 1), width), _full(2)
    rc = lib.cmtfpls_rank1_tensor_f64(Z.data_ptr(), arr, n, 1e-8, fac.data_ptr(), width if ld is None else ld, info.data_ptr(), 30,
                                      ws.data_ptr(), (need + ws_delta) if need else ws.numel(), None)
    torch.cuda.synchronize()
    return rc, fac, info, need


def _untouched(fac, info):
    return bool((fac == SENTINEL).all()) and bool((info == SENTINEL).all())


@pytest.mark.parametrize("dims", [(1025, 2, 2), (2, 1025, 2), (2, 2, 1025)])
def test_a_mode_past_1024_is_declined_as_unsupported(be, dims):
    rc, fac, info, _ = _raw(be, dims)
    assert rc == EUNSUPPORTED and b"mode too large" in be.lib.cmtfpls_last_error()
    assert _untouched(fac, info)


@pytest.mark.parametrize("dims,ld,why", [((5, 4), None, "order 2"), ((2,) * 8, None, "order 8"), ((4, 0, 3), None, "a dim of 0"),
                                         ((4, 9, 3), 8, "ld = max(dims) - 1")], ids=lambda v: v if isinstance(v, str) else None)
def test_bad_arguments_are_declined_as_invalid(be, dims, ld, why):
    rc, fac, info, need = _raw(be, dims, ld=ld)
    assert rc == EINVAL, (why, rc)
    assert _untouched(fac, info)
    if ld is None:
        assert need == 0                                              # cmtfpls_rank1_tensor_workspace_bytes declines them too


def test_workspace_size_is_checked_to_the_byte(be):
    rc, fac, info, need = _raw(be, (9, 8, 7), ws_delta=-8)
    assert need > 0 and rc == EWORKSPACE and b"workspace" in be.lib.cmtfpls_last_error()
    assert _untouched(fac, info)
    rc, fac, info, _ = _raw(be, (9, 8, 7))                            # exactly the stated size: runs
    assert rc == 0 and info.cpu().tolist()[0] == 1.0 and not bool((fac[0] == SENTINEL).any())


# ---- end to end at the declared top: X of order 8 ------------------------------------------------------------------------------
def _normwise(got, want):
    scale = np.nanmax(np.abs(want), axis=0, keepdims=True)
    return np.nanmax(np.abs(got - want) / (np.abs(want) + scale))


@pytest.mark.parametrize("algorithm", ["direct", "xcov"])
def test_fit_of_an_order_8_tensor(api, be, algorithm):
    """The assertions of test_gpu_round3.py::test_fit_of_order_6_and_7_tensors at MAX_ORDER (Z of order 7 = kMaxOrder), and the
    Kronecker chain that forms wB from the six trailing loadings."""
    from cmtf_pls_amd.engine import NipalsEngine
    shape = (24, 2, 2, 2, 2, 2, 2, 3)
    x, y, _ = O.import_synthetic(shape, 3, 2, error=0.1, seed=17)
    m = api.tPLS(2, algorithm=algorithm)
    m.fit(x, y)
    fit = O.fit_tpls(x, y, 2)
    assert len(m.X_factors) == len(shape)
    assert m.n_iter_ == fit.n_iter
    assert _normwise(m.X_factors[0], fit.T) <= 1e-8
    for got, want in zip(m.X_factors[1:], fit.loadings[0]):
        assert_allclose(np.abs(got), np.abs(want), rtol=0, atol=1e-8)
        assert_allclose(np.linalg.norm(got, axis=0), 1, rtol=1e-12)
    assert_allclose(m.R2X, fit.r2x[0], rtol=0, atol=1e-9)
    assert_allclose(m.R2Y, fit.r2y, rtol=0, atol=1e-9)
    assert_allclose(m.transform(x), m.X_factors[0], rtol=1e-8, atol=1e-10)
    assert_allclose(m.predict(x[:5]), O.predict(fit, x[:5]), rtol=1e-7, atol=1e-9)
    xt = x[:6].copy()
    xt[2, 1, 0, 1, 0, 1, 1, 2] = np.nan
    assert _normwise(m.transform(xt), O.transform(fit, xt)) <= 1e-8
    vecs = [np.ascontiguousarray(f[:, 0]) for f in m.X_factors[2:]]
    assert len(vecs) == 6
    out = NipalsEngine(be).kron_trailing([_dev(v) for v in vecs], be.empty(int(np.prod(shape[2:]))))
    want = vecs[0]
    for v in vecs[1:]:
        want = np.kron(want, v)
    assert np.array_equal(out.cpu().numpy(), want)


def test_order_9_is_refused_before_any_backend_call(api, monkeypatch):
    from cmtf_pls_amd.backend import HipBackend
    names = [n for n, v in vars(HipBackend).items() if inspect.isfunction(v) and not n.startswith("_")]
    assert "rank1_tensor" in names and "colstats" in names
    calls = {n: 0 for n in names}
    for n in names:
        orig = getattr(HipBackend, n)

        def wrapped(self, *a, __orig=orig, __n=n, **k):
            calls[__n] += 1
            return __orig(self, *a, **k)
        monkeypatch.setattr(HipBackend, n, wrapped)
    x, y, _ = O.import_synthetic((12,) + (2,) * 8, 2, 2, error=0.1, seed=3)
    with pytest.raises(NotImplementedError, match="order > 8"):
        api.tPLS(2).fit(x, y)
    assert not any(calls.values()), {n: c for n, c in calls.items() if c}


# ---- the one-launch chain of an init gives up ------------------------------------------------------------------------------------
def test_a_chain_that_gives_up_shows_through_the_tensor_entry_and_the_fit_falls_back_to_launches(api):
    """cmtfpls_rank1_chain_enable(2) (the library's bounded test mode, as in test_gpu_round4.py) launches the chain of squarings
    of every unfolding whose smaller side is >= 17 with one row of workgroups missing: those inits give up and are NaN.  The tensor
    entry must report what cmtfpls_rank1_f64 reports -- info = [0, -1], NaN factors -- and not 100 sweeps on NaN as `converged`;
    a fit then switches the chain off for the process, repeats the iteration through the launch form and says so.

    The shapes.  Z of (40, 30, 20): every unfolding has more than one row of workgroups.  The fit: trailing modes (20, 18, 17),
    for the same reason -- with trailing modes (6, 5, 4) every unfolding is ONE workgroup (16 rows per tile), mode 2 removes
    nothing and no chain can give up; that fit is run too and must be the chain-off fit bit for bit with the mode left as it was."""
    from cmtf_pls_amd.backend import HipBackend
    be = HipBackend(DEV)
    lib = be.lib
    big = O.import_synthetic((30, 20, 18, 17), 3, 2, error=0.2, seed=9)[:2]
    small = O.import_synthetic((30, 6, 5, 4), 3, 2, error=0.2, seed=9)[:2]

    def fit(xy):
        m = api.tPLS(2, backend=HipBackend(DEV))
        m.fit(*xy)
        return m

    def same_bits(a, b):
        return all(np.array_equal(f, g) for f, g in zip(a.X_factors + a.Y_factors, b.X_factors + b.Y_factors))

    try:
        lib.cmtfpls_rank1_chain_enable(0)
        ref_big, ref_small = fit(big), fit(small)
        assert all(np.isfinite(f).all() for f in ref_big.X_factors + ref_big.Y_factors)
        # kernel level
        lib.cmtfpls_rank1_chain_enable(2)
        dims = (40, 30, 20)
        Z = R.make_z(dims, "strong", 0)
        fac, info = _full(3, 43), torch.zeros(2, dtype=torch.float64, device=DEV)
        be.rank1_tensor(_dev(Z.ravel()), dims, 1e-8, fac, info=info)
        got = fac.cpu().numpy()
        assert info.cpu().tolist() == [0.0, -1.0], info.cpu().tolist()
        for m, d in enumerate(dims):
            assert np.isnan(got[m, :d]).all() and np.all(got[m, d:] == SENTINEL)
        assert lib.cmtfpls_rank1_chain_enabled() == 2
        # engine level: nothing to give up on one-workgroup unfoldings
        m = fit(small)
        assert same_bits(m, ref_small) and lib.cmtfpls_rank1_chain_enabled() == 2
        assert not any("switched off" in d for d in m.fit_report_["declined"])
        # engine level: the give-up
        m = fit(big)
        assert all(np.isfinite(f).all() for f in m.X_factors + m.Y_factors)
        assert same_bits(m, ref_big)
        assert m.n_iter_ == ref_big.n_iter_
        assert lib.cmtfpls_rank1_chain_enabled() == 0
        assert any("switched off" in d for d in m.fit_report_["declined"]), m.fit_report_["declined"]
    finally:
        lib.cmtfpls_rank1_chain_enable(1)
