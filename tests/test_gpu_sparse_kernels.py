"""cmtfpls_rank1_sparse_f64 and cmtfpls_soft_normalize_f64 against the float64 mirror (tests/sparse_ref.py), on the GPU.

The kernel and the mirror start from the SAME dense pair, so with tol_s = 0 (exactly max_sweeps sweeps) only the summation order
differs: 1e-11 absolute on the unit-norm outputs, the bound the project holds its device contractions to, and exact zeros where
the mirror has them -- every input is screened on the CPU first: no pre-threshold magnitude within 1e-6 relative of theta
(sparse_ref.THETA_MARGIN).  Shapes: small and odd ones, 128 x 128 (Z in LDS, form 1), 130 x 128 (just past it, form 2), the limits
256 x 256 and 16 x 4096; a zero row; an exact tie for the maximum."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import sparse_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(shape, "plain") for shape in S.KERNEL_SHAPES] + [((12, 9), "zero_row"), ((130, 128), "zero_row"), ((7, 70), "tie"), ((128, 128), "tie")]
IDS = [f"{a}x{b}-{v}" for (a, b), v in CASES]
_WORST = {"tol0": 0.0, "default": 0.0}


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend()


def _dev(be, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(be.device)


def _run(be, Z, pair, lams, tol_s, max_sweeps):
    A, B = Z.shape
    Zd, wA, wB, info = _dev(be, Z), _dev(be, pair[0]), _dev(be, pair[1]), be.zeros(2)
    be.rank1_sparsify(Zd.view(-1), A, B, wA, wB, lams[0], lams[1], info, tol_s=tol_s, max_sweeps=max_sweeps)
    return wA.cpu().numpy(), wB.cpu().numpy(), info.cpu().numpy()


def test_form_is_observable(be):
    assert be.rank1_sparse_form(128, 128) == 1 and be.rank1_sparse_form(130, 128) == 2
    assert be.rank1_sparse_form(256, 256) == 2 and be.rank1_sparse_form(16, 4096) == 2 and be.rank1_sparse_form(12, 9) == 1
    assert be.rank1_sparse_form(257, 256) == 0 and be.rank1_sparse_form(1, 9) == 0 and be.rank1_sparse_form(4097, 2) == 0
    assert be.lib.cmtfpls_rank1_sparse_workspace_bytes(128, 128) == 0


@pytest.mark.parametrize("lams", S.KERNEL_LAMS, ids=lambda l: f"lam{l[0]}-{l[1]}")
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_sweep_count_against_the_mirror(be, case, lams):
    shape, variant = case
    Z = S.kernel_case(shape, variant)
    pair = S.dense_pair(Z)
    if shape == (128, 128):
        assert be.rank1_sparse_form(*shape) == 1
    if shape == (130, 128):
        assert be.rank1_sparse_form(*shape) == 2
    if variant == "zero_row":
        assert not Z[shape[0] // 2].any()
    if variant == "tie":
        top = int(np.argmax(np.abs(Z @ pair[1])))                                   # the row behind max |Z wB| is there twice: the
        assert sum(np.array_equal(Z[top], row) for row in Z) == 2                   # kernel sums both in the same order, so they tie
    for sweeps in (1, 5):
        st = {}
        wantA, wantB = S.sparse_rank1(Z, lams, 0.0, sweeps, dense=lambda z: pair, stats=st)
        assert all(m > S.THETA_MARGIN for m in st["margins"]), min(st["margins"])
        gotA, gotB, info = _run(be, Z, pair, lams, 0.0, sweeps)
        err = max(np.abs(gotA - wantA).max(), np.abs(gotB - wantB).max())
        _WORST["tol0"] = max(_WORST["tol0"], float(err))
        print(f"{shape} {variant} lam {lams} sweeps {sweeps}: max abs error {err:.3e} (worst so far {_WORST['tol0']:.3e})")
        assert err <= 1e-11, err
        assert np.array_equal(gotA == 0.0, wantA == 0.0) and np.array_equal(gotB == 0.0, wantB == 0.0)
        assert list(info) == [0.0, float(sweeps)]                                  # tol_s = 0 never stops early
        if lams[0] > 0:
            assert (gotA != 0).sum() >= 1 and (gotB != 0).sum() >= 1               # at least one entry survives
        againA, againB, _ = _run(be, Z, pair, lams, 0.0, sweeps)
        assert againA.tobytes() == gotA.tobytes() and againB.tobytes() == gotB.tobytes()   # a second call: the same bits
    if variant == "zero_row" and lams[0] > 0:
        assert gotA[shape[0] // 2] == 0.0


@pytest.mark.parametrize("lams", S.KERNEL_LAMS, ids=lambda l: f"lam{l[0]}-{l[1]}")
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_default_tolerance_against_the_mirror(be, case, lams):
    """tol_s = 1e-10, max_sweeps = 200: converged, sweeps within one of the mirror's, outputs within 1e-9 = 10 tol_s (a one-sweep
    disagreement moves the result by less than tol_s; the factor ten is the margin for that)."""
    shape, variant = case
    Z = S.kernel_case(shape, variant)
    pair = S.dense_pair(Z)
    st = {}
    wantA, wantB = S.sparse_rank1(Z, lams, 1e-10, 200, dense=lambda z: pair, stats=st)
    assert st["info"][0] == 1
    gotA, gotB, info = _run(be, Z, pair, lams, 1e-10, 200)
    assert info[0] == 1.0
    assert abs(int(info[1]) - st["info"][1]) <= 1, (info, st["info"])
    err = max(np.abs(gotA - wantA).max(), np.abs(gotB - wantB).max())
    _WORST["default"] = max(_WORST["default"], float(err))
    print(f"{shape} {variant} lam {lams}: sweeps {int(info[1])} (mirror {st['info'][1]}), max abs error {err:.3e}")
    assert err <= 1e-9, err


def test_zero_vector_gives_nan_loadings(be):
    """A zero a or b: NaN loadings, as normalising a zero vector does; the NaN distance never counts as converged."""
    Z = np.zeros((6, 4))
    gotA, gotB, info = _run(be, Z, (np.ones(6) / np.sqrt(6), np.ones(4) / 2.0), (0.2, 0.2), 1e-10, 3)
    assert np.isnan(gotA).all() and np.isnan(gotB).all() and list(info) == [0.0, 3.0]


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.95])
@pytest.mark.parametrize("n", [1, 3, 70, 4097])
def test_soft_normalize(be, n, lam):
    rng = np.random.default_rng(n)
    v = rng.normal(size=n)
    m = []
    want = S.soft_normalize(v, lam, m)
    assert all(x > S.THETA_MARGIN for x in m)
    d = _dev(be, v)
    be.soft_normalize(d, lam)
    got = d.cpu().numpy()
    assert np.array_equal(got == 0.0, want == 0.0)
    assert np.linalg.norm(got - want) <= 1e-13 * np.linalg.norm(want)
    nrm = be.zeros(1)
    d2 = _dev(be, v)
    from cmtf_pls_amd import _lib
    _lib.check(be.lib.cmtfpls_soft_normalize_f64(d2.data_ptr(), n, lam, nrm.data_ptr(), be._stream()))
    assert d2.cpu().numpy().tobytes() == got.tobytes()
    assert abs(float(nrm.item()) - np.linalg.norm(S.soft(v, lam))) <= 1e-13 * np.linalg.norm(S.soft(v, lam))


@pytest.mark.parametrize("args,status", [
    ((1, 65537, 0.2, 0.2, 1e-10, 200), 4),            # A * B = 65537 (and A = 1)
    ((257, 256, 0.2, 0.2, 1e-10, 200), 4),            # A * B = 65792 with both sides inside
    ((4097, 2, 0.2, 0.2, 1e-10, 200), 4),             # A = 4097
    ((12, 9, 1.0, 0.2, 1e-10, 200), 1),               # lambda = 1
    ((12, 9, 0.2, -0.1, 1e-10, 200), 1),
    ((12, 9, 0.2, 0.2, 1e-10, 0), 1),                 # max_sweeps = 0
])
def test_declines_fire_before_any_pointer_is_read(be, args, status):
    A, B, lamA, lamB, tol_s, sweeps = args
    rc = be.lib.cmtfpls_rank1_sparse_f64(None, A, B, None, None, lamA, lamB, tol_s, sweeps, None, None, 0, be._stream())
    assert rc == status
    be.lib.cmtfpls_clear_error()


def test_soft_normalize_declines(be):
    assert be.lib.cmtfpls_soft_normalize_f64(None, (1 << 24) + 1, 0.2, None, be._stream()) == 4
    assert be.lib.cmtfpls_soft_normalize_f64(None, 8, 1.0, None, be._stream()) == 1
    be.lib.cmtfpls_clear_error()
