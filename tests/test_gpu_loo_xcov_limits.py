"""cmtfpls_loo_xcov_f64 (loo_xcov.hip, its inner loop and matrix-core Gram squarings in fold_loop.hpp: the "xcov" form of
validate.get_q2y, a 1024-thread workgroup per held-out sample) at the limits it declares and at the edges of its tiles.

Declared limits: min(A, B) <= 256, M <= 128, R <= 64, the fold's small vectors within 150 KB of dynamic LDS (A B <= 2^24 is implied
by the LDS rule: tests/loo_xcov_ref.py).  Which branch a case is there for is computed by loo_xcov_ref.loo_xcov_form, a mirror of
the entry's rules written from the kernel's header, and every case asserts it; tests/test_loo_xcov_ref_cpu.py proves the mirror
against the library's host function and the input conditions without a GPU.

Reference: loo_xcov_ref.loo_literal, literal refits over the float64 oracle, on the first, middle and last fold of a case.  Every
case runs twice: tol = 1e-8 with 100 passes at most (get_q2y's), and tol = 0 with 3 passes, where no convergence decision exists.
Predictions: normwise (max|got - want| / max(1, max|want|)) 1e-8, the bound test_gpu_round4.
test_q2y_beyond_the_lds_shapes_equals_literal_refits holds this kernel to.  For the R = 64 and M >= 127 cases the bound is
10 x condition_probe (the same refits iterated on S = Y^T X in NumPy: two correct float64 evaluations), never below 1e-8; computed
when the test runs, on the CPU.  Measured:

    case                      run              condition_probe    bound
    (12, 141, 256), 128, 10   tol 1e-8         7.7e-14            1e-8
    (12, 141, 256), 128, 10   tol 0, 3 passes  7.9e-14            1e-8
    (40, 20, 70), 127, 3      tol 1e-8         5.2e-16            1e-8
    (40, 20, 70), 127, 3      tol 0, 3 passes  5.6e-16            1e-8
    (70, 8, 72), 2, 64        tol 1e-8         4.2e-11            1e-8
    (70, 8, 72), 2, 64        tol 0, 3 passes  3.5e-11            1e-8

(ten times every probe is below the floor of 1e-8, so all three are held to 1e-8 as well; the kernel's own distance from the literal
refits measured 5e-14 / 3e-13, 8e-16 / 6e-16 and 2e-11 / 2e-11.  The R = 64 case is chaotic at most seeds and noise levels -- two
NumPy evaluations of the same folds then differ by O(1) and more -- so its inputs are rank 4 with noise 1e-10, seed 2, where the
60 late components sit at noise level and both evaluations agree; tests/test_loo_xcov_ref_cpu.py holds every probed case to
10 x probe <= 1e-4.)

Pass counts (tol = 1e-8): equal to the reference's for every (fold, component) whose reference convergence norm |u_old - u| lies
outside [tol / 2, 2 tol] on the passing step and on the step before it (loo_xcov_ref.on_threshold)."""
import numpy as np
import pytest
import torch

import loo_xcov_ref as L

pytestmark = pytest.mark.gpu

_DEV = "cuda:0"
EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4
RUNS = [(L.TOL, L.MAX_ITER), (L.CAP_TOL, L.CAP_ITER)]
TAIL = 4096


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(_DEV))


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(_DEV)        # (a copy: the cached cases are read-only)


def _inputs(case):
    shape, M = case[0], case[1]
    x, y = L.case_data(case[0], case[1], *case[3:6])
    return _dev(x.reshape(shape[0], -1)), _dev(y.reshape(shape[0], M))


def _form(case):
    """The case's form from the mirror, with the branch values the table claims asserted."""
    shape, M, R = case[:3]
    form, why = L.loo_xcov_form(shape[0], *L.split(shape), M, R)
    assert form is not None, (case, why)
    assert {k: form[k] for k in case[6]} == case[6], (case, form)
    return form


# ---- 1. every edge against the literal refits ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol,max_iter", RUNS, ids=["converged", "capped"])
@pytest.mark.parametrize("case", L.MATCH_CASES, ids=[L.case_id(c) for c in L.MATCH_CASES])
def test_each_edge_matches_the_literal_refits(be, case, tol, max_iter):
    shape, M, R = case[:3]
    I, (A, B) = shape[0], L.split(shape)
    _form(case)
    X2, Y = _inputs(case)
    out = be.loo_tpls(X2, Y, A, B, R, tol, max_iter, forms=("xcov",))
    assert out is not None and out[2] == "xcov"
    folds = list(L.three_folds(I))
    pred, n_iter = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert np.isfinite(pred).all()
    ref = L.case_reference(*case[:6], tol, max_iter)
    bound = L.case_bound(case, tol, max_iter)
    err = L.normwise(pred[folds], ref["pred"])
    print(f"{L.case_id(case)} tol={tol:g}: normwise {err:.2e} (bound {bound:.2e}); passes {int(n_iter.min())}..{int(n_iter.max())}")
    if tol == 0.0:
        assert (n_iter == max_iter).all() and (ref["n_iter"] == max_iter).all()     # every fold, every component: the cap exactly
    else:
        firm = ~L.on_threshold(ref, tol)
        assert np.array_equal(n_iter[folds][firm], ref["n_iter"][firm]), (n_iter[folds], ref["n_iter"], firm)
    assert err <= bound, (err, bound)


# ---- 2. chunking, bounds, reproducibility (the C entry) ----------------------------------------------------------------------------
class _Raw:
    """One case on the device and launches of folds [f0, f0 + nf) through the C entry into fresh sentinel-filled outputs.  The
    workspace is the head of one buffer sized for ALL folds plus 4 KB, every byte 0xA5: the entry is told per * nf bytes, and
    everything behind them must still read 0xA5 afterwards."""

    def __init__(self, be, case):
        self.be, self.case = be, case
        shape, self.M, self.R = case[:3]
        self.I, (self.A, self.B) = shape[0], L.split(shape)
        self.per = _form(case)["ws_bytes_per_fold"]
        self.X2, self.Y = _inputs(case)
        self.cx, self.cy = self.X2.sum(dim=0), self.Y.sum(dim=0)

    def launch(self, chunks, tol=L.TOL, max_iter=L.MAX_ITER):
        from cmtf_pls_amd.backend import _ptr
        pred = torch.full((self.I, self.M), float("nan"), dtype=torch.float64, device=_DEV)
        n_iter = torch.full((self.I, self.R), -7, dtype=torch.int32, device=_DEV)
        ws = torch.full((self.per * self.I + TAIL,), 0xA5, dtype=torch.uint8, device=_DEV)
        for f0, nf in chunks:
            rc = self.be.lib.cmtfpls_loo_xcov_f64(_ptr(self.X2), _ptr(self.Y), _ptr(self.cx), _ptr(self.cy), self.I, self.A, self.B, self.M,
                                                  self.R, tol, max_iter, f0, nf, _ptr(pred), _ptr(n_iter), _ptr(ws), self.per * nf,
                                                  self.be._stream())
            torch.cuda.synchronize()
            assert rc == 0, (f0, nf, rc)
            assert bool((ws[self.per * nf:] == 0xA5).all()), ("workspace written past per * nfolds bytes", f0, nf)
            ws[:self.per * nf] = 0xA5
        return pred.cpu().numpy(), n_iter.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module", params=L.CHUNK_CASES, ids=[L.case_id(c) for c in L.CHUNK_CASES])
def raw(be, request):
    r = _Raw(be, request.param)
    r.whole = r.launch([(0, r.I)])
    return r


def test_whole_launch_is_complete_and_reproducible(raw):
    pred, n_iter = raw.whole
    assert np.isfinite(pred).all() and (n_iter >= 2).all() and (n_iter <= L.MAX_ITER).all()
    again = raw.launch([(0, raw.I)])
    assert np.array_equal(_bits(again[0]), _bits(pred)) and np.array_equal(again[1], n_iter)


@pytest.mark.parametrize("nfolds", [1, 5, 7])
def test_chunked_launches_equal_the_whole_one_bit_for_bit(raw, nfolds):
    chunks = [(f0, min(nfolds, raw.I - f0)) for f0 in range(0, raw.I, nfolds)]
    pred, n_iter = raw.launch(chunks)
    assert np.array_equal(_bits(pred), _bits(raw.whole[0])) and np.array_equal(n_iter, raw.whole[1])


@pytest.mark.parametrize("where", ["first", "inside", "last"])
def test_a_launch_of_some_folds_leaves_the_other_rows_alone(raw, where):
    nf = 3
    f0 = {"first": 0, "inside": (raw.I - nf) // 2 + 1, "last": raw.I - nf}[where]
    pred, n_iter = raw.launch([(f0, nf)])
    mine = np.zeros(raw.I, dtype=bool)
    mine[f0:f0 + nf] = True
    assert np.isnan(pred[~mine]).all() and (n_iter[~mine] == -7).all()
    assert np.array_equal(_bits(pred[mine]), _bits(raw.whole[0][mine])) and np.array_equal(n_iter[mine], raw.whole[1][mine])


def test_backend_chunks_of_three_folds_equal_its_default(be, raw):
    args = (raw.X2, raw.Y, raw.A, raw.B, raw.R, L.TOL, L.MAX_ITER)
    whole = be.loo_tpls(*args, forms=("xcov",))
    three = be.loo_tpls(*args, max_ws_bytes=raw.per * 3, forms=("xcov",))
    assert whole is not None and three is not None and whole[2] == three[2] == "xcov"
    assert torch.equal(whole[0], three[0]) and torch.equal(whole[1], three[1])
    assert bool(torch.isfinite(whole[0]).all())


# ---- 3. declines and bad arguments: host checks only, no leave-one-out launch ------------------------------------------------------
def _status(be, I, A, B, M, R, ws_bytes, max_iter=L.MAX_ITER, fold0=0, nfolds=1):
    """The entry's status on a shape description: X, Y and the column sums are one small buffer that a call stopped by the host
    checks never reads; a launch would overwrite Ypred's NaN."""
    buf = torch.zeros(64, dtype=torch.float64, device=_DEV)
    pred = torch.full((64,), float("nan"), dtype=torch.float64, device=_DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=_DEV)
    p = buf.data_ptr()
    rc = be.lib.cmtfpls_loo_xcov_f64(p, p, p, p, I, A, B, M, R, L.TOL, max_iter, fold0, nfolds, pred.data_ptr(), None,
                                     ws.data_ptr() if ws_bytes else None, ws_bytes, be._stream())
    torch.cuda.synchronize()
    be.lib.cmtfpls_clear_error()
    assert bool(torch.isnan(pred).all())                                            # nothing ran
    return rc


@pytest.mark.parametrize("limit", sorted(L.DECLINES))
def test_one_step_past_each_limit_declines_and_one_step_inside_only_misses_the_workspace(be, limit):
    inside, past = L.DECLINES[limit]
    assert L.loo_xcov_form(*inside)[0] is not None and L.loo_xcov_form(*past) == (None, limit)
    if limit == "lds":
        assert L.loo_xcov_form(*inside)[0]["lds_bytes"] == L.LDS_CAP and 8 * L.lds_doubles(*past[1:]) == L.LDS_CAP + 16    # wB and ys one double longer each
    assert _status(be, *past, 1 << 40) == EUNSUPPORTED
    assert _status(be, *inside, 0) == EWORKSPACE                                    # the shape check comes before the workspace check
    I, A, B, M, R = past
    X2 = torch.zeros(I, A * B, dtype=torch.float64, device=_DEV)
    Y = torch.zeros(I, M, dtype=torch.float64, device=_DEV)
    assert be.loo_tpls(X2, Y, A, B, R, L.TOL, L.MAX_ITER, forms=("xcov",)) is None


def test_bad_arguments_are_refused(be):
    assert _status(be, 1, 8, 8, 2, 2, 1 << 40) == EINVAL                            # I = 1: no training rows
    assert _status(be, 6, 8, 8, 2, 2, 1 << 40, fold0=4, nfolds=3) == EINVAL         # fold0 + nfolds > I
    assert _status(be, 6, 8, 8, 2, 2, 1 << 40, max_iter=0) == EINVAL
    assert _status(be, 6, 8, 8, 2, 2, 0) == EWORKSPACE                              # (the same shape is otherwise accepted)
