"""cmtfpls_kfold_inner_coupled_tensor_f64 (the coupled fold loop with the rank-1 CP of every order-4 block's cross-covariance inside
each fold's workgroup, csrc/kfold.hip: kfold_inner_coupled_kernel<GROUPED, TENSOR = true>) against the NumPy float64 restatement
tests/kfold_coupled_order4_ref.py, whose extraction is oracle.nipals_oracle.rank1_factors for every block.  The states are built by
hand: K = 3 models, each block's S with a planted dominant rank-one term plus 5 % noise, G_y an identity-like SPD matrix in the
first row tile's partial, a random mean per block.

Tolerance: 1e-10 normwise on every loading and on q, the tolerance of test_gpu_kfold_order4_kernel.py; the iteration counts must be
equal.  One block of order 4 must give the bits of cmtfpls_kfold_inner_tensor_f64."""
import ctypes

import numpy as np
import pytest
import torch

from cmtf_pls_amd import kfold
from cmtf_pls_amd.backend import HipBackend
from kfold_coupled_order4_ref import coupled_inner_loop, planted_blocks, view

pytestmark = pytest.mark.gpu

_TOL = 1e-10
_K, _R, _I, _M = 3, 2, 8, 3
# (A, B1, B2) per block, (A, B) for a matrix block: tensor + order 2 + order 3; two tensors (lx_rank1's transpose path, a long
# unfolding); B2 = 1 after a matrix (an offset that assumes the tensor comes first)
BLOCK_SETS = [[(5, 7, 3), (1, 9), (6, 4)], [(40, 3, 2), (17, 4, 33)], [(4, 6), (6, 1, 5)]]


@pytest.fixture(scope="module")
def be():
    return HipBackend("cuda:0")


def _rel(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _tensor(dims):
    return [(d[1], d[2]) if len(d) == 3 else (0, 0) for d in dims]


def _t(be, a, dt=torch.float64):
    return kfold._to_dev(a, be.device, dt)


def _hand_state(be, Ss, Gy, dims, means, folds=None, slots=1):
    """A state of K = Ss[0].shape[0] models on the blocks' S (K x M x P_b) whose summed row-tile partials of G_y are Gy."""
    K, M, _ = Ss[0].shape
    blocks = [(*view(d), _t(be, S), _t(be, mu)) for d, S, mu in zip(dims, Ss, means)]
    st, shared, own = kfold._state(be, _t(be, np.arange(_I) % (folds or K), torch.int32), be.zeros(K, _I, M), blocks, _R, slots)
    shared["Gy"].zero_()
    shared["Gy"][:, 0] = _t(be, Gy)
    return st, shared, own


def _means(dims, rows, seed=2):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((rows, int(np.prod(d)))) for d in dims]


def _loadings_out(be, dims, K):
    tens = [d for d in dims if len(d) == 3]
    return be.zeros(sum(K * _R * d[1] for d in tens)), be.zeros(sum(K * _R * d[2] for d in tens))


def _run(be, st, dims, a=0, model_fold=None, groups=1, out=True):
    K = st[0].K
    Wk, Wl = _loadings_out(be, dims, K) if out else (None, None)
    ws = torch.empty(max(be.kfold_inner_coupled_tensor_workspace_bytes(st, _tensor(dims)), 256), dtype=torch.uint8, device=be.device)
    ok = be.kfold_inner_coupled_tensor(st, _tensor(dims), a, 1e-8, 100, ws, model_fold, groups, Wk, Wl)
    torch.cuda.synchronize()
    return ok, Wk, Wl


def _slices(W, dims, K, mode):
    """Per block its K x R x B1 (mode 1) or B2 (mode 2) slice of Wk / Wl (None for a matrix block): one after another, in block order."""
    out, o = [], 0
    Wh = W.cpu().numpy()
    for d in dims:
        if len(d) != 3:
            out.append(None)
            continue
        n = K * _R * d[mode]
        out.append(Wh[o:o + n].reshape(K, _R, d[mode]))
        o += n
    assert o == Wh.size
    return out


def _check(shared, own, Wk, Wl, Ss, Gy, dims, means, a=0, model_fold=None):
    K = Ss[0].shape[0]
    Q, n_iter, vec = shared["Q"].cpu().numpy(), shared["n_iter"].cpu().numpy(), shared["vec"].cpu().numpy()
    wks, wls = _slices(Wk, dims, K, 1), _slices(Wl, dims, K, 2)
    assert not shared["status"].cpu().numpy().any()
    for k in range(K):
        want = coupled_inner_loop([S[k] for S in Ss], Gy, dims, 1e-8, 100)
        errs = {"q": _rel(Q[k, a], want["q"])}
        mw = 0.0
        for b, d in enumerate(dims):
            Wa, Wb = own[b]["Wa"].cpu().numpy(), own[b]["Wb"].cpu().numpy()
            WA, WB = own[b]["WA"].cpu().numpy(), own[b]["WB"].cpu().numpy()
            modes = want["blocks"][b]["modes"]
            if len(d) == 3:
                errs[f"wA{b}"], errs[f"wK{b}"], errs[f"wL{b}"] = _rel(Wa[k, a], modes[0]), _rel(wks[b][k, a], modes[1]), _rel(wls[b][k, a], modes[2])
                errs[f"wB{b}"] = _rel(Wb[k, a], np.kron(modes[1], modes[2]))
                assert np.array_equal(Wb[k, a], np.outer(wks[b][k, a], wls[b][k, a]).ravel())   # wB = wK (x) wL, C order
            elif d[0] == 1:                                                          # order 2: Z / norm(Z), wA = 1
                assert Wa[k, a, 0] == 1.0
                errs[f"wB{b}"] = _rel(Wb[k, a], modes[0])
            else:
                errs[f"wA{b}"], errs[f"wB{b}"] = _rel(Wa[k, a], modes[0]), _rel(Wb[k, a], modes[1])
            assert np.array_equal(WA[:, k], Wa[k, a]) and np.array_equal(WB[:, k], Wb[k, a])   # the MTTKRP operands
            mw += means[b][k if model_fold is None else model_fold[k]] @ np.kron(Wa[k, a], Wb[k, a])
        print(f"blocks {dims} a {a} model {k}: n_iter {int(n_iter[k, a])} (want {want['n_iter']}), errors {errs}")
        assert int(n_iter[k, a]) == want["n_iter"], (k, n_iter[k, a], want["n_iter"])
        assert max(errs.values()) <= _TOL, (k, errs)
        np.testing.assert_allclose(vec[k, 3 * _R + _M + 1], mw / len(dims), rtol=1e-12, atol=1e-14)   # the block-averaged mu^T w


@pytest.mark.parametrize("dims", BLOCK_SETS, ids=["tensor+order2+order3", "two tensors", "matrix then B2=1"])
def test_both_components_match_the_float64_restatement(be, dims):
    """a = 0, then a = 1 on fresh S (no down-date between them, as test_gpu_kfold_order4_kernel.py): slot 1 of every loading is
    written, slot 0 stays, and g_0 is the blocks' mean of (wA_0 . wA_1)(wB_0 . wB_1)."""
    seed = sum(sum(d) for d in dims)
    Ss, Gy = planted_blocks(dims, _M, _K, seed)
    means = _means(dims, _K)
    st, shared, own = _hand_state(be, Ss, Gy, dims, means)
    ok, Wk, Wl = _run(be, st, dims)
    assert ok is True
    _check(shared, own, Wk, Wl, Ss, Gy, dims, means)
    first = [(o["Wa"][:, 0].clone(), o["Wb"][:, 0].clone()) for o in own]
    Ss1, _ = planted_blocks(dims, _M, _K, seed + 1000)
    for o, S in zip(own, Ss1):
        o["S"].copy_(_t(be, S))
    Wk1, Wl1 = _loadings_out(be, dims, _K)
    Wk1.copy_(Wk)
    Wl1.copy_(Wl)
    ws = torch.empty(be.kfold_inner_coupled_tensor_workspace_bytes(st, _tensor(dims)), dtype=torch.uint8, device=be.device)
    assert be.kfold_inner_coupled_tensor(st, _tensor(dims), 1, 1e-8, 100, ws, None, 1, Wk1, Wl1) is True
    torch.cuda.synchronize()
    _check(shared, own, Wk1, Wl1, Ss1, Gy, dims, means, a=1)
    for b, d in enumerate(dims):
        assert torch.equal(own[b]["Wa"][:, 0], first[b][0]) and torch.equal(own[b]["Wb"][:, 0], first[b][1])
        if len(d) == 3:
            for W0, W1, m in ((Wk, Wk1, 1), (Wl, Wl1, 2)):
                s0, s1 = _slices(W0, dims, _K, m)[b], _slices(W1, dims, _K, m)[b]
                assert np.array_equal(s0[:, 0], s1[:, 0]) and s1[:, 1].any() and not s0[:, 1].any()
    g = shared["vec"].cpu().numpy()[:, 2 * _R + _M + 1]
    want = np.mean([[(o["Wa"][k, 0] @ o["Wa"][k, 1]).item() * (o["Wb"][k, 0] @ o["Wb"][k, 1]).item() for k in range(_K)] for o in own],
                   axis=0)
    np.testing.assert_allclose(g, want, rtol=1e-12, atol=1e-15)


def test_one_block_of_order4_gives_the_bits_of_the_tensor_entry(be):
    dims = [(3, 16, 16)]
    Ss, Gy = planted_blocks(dims, _M, _K, seed=35)
    means = _means(dims, _K)
    outs = []
    for coupled in (False, True):
        st, shared, own = _hand_state(be, Ss, Gy, dims, means)
        Wk, Wl = be.zeros(_K, _R, 16), be.zeros(_K, _R, 16)
        for a in range(_R):
            if coupled:
                ws = torch.empty(be.kfold_inner_coupled_tensor_workspace_bytes(st, [(16, 16)]), dtype=torch.uint8, device=be.device)
                assert be.kfold_inner_coupled_tensor(st, [(16, 16)], a, 1e-8, 100, ws, None, 1, Wk, Wl) is True
            else:
                ws = torch.empty(be.kfold_inner_tensor_workspace_bytes(3, 16, 16, _K), dtype=torch.uint8, device=be.device)
                assert be.kfold_inner_tensor(st[0], 16, 16, a, 1e-8, 100, ws, None, 1, Wk, Wl) is True
        torch.cuda.synchronize()
        assert ws.numel() == _K * 8 * (6 * 768 + 2 * 16 * 16)                        # the same scratch: 6 P + 2 n^2 per fold
        outs.append({"Q": shared["Q"], "Wa": own[0]["Wa"], "Wb": own[0]["Wb"], "Wk": Wk, "Wl": Wl, "WA": own[0]["WA"],
                     "WB": own[0]["WB"], "n_iter": shared["n_iter"], "vec": shared["vec"], "status": shared["status"]})
    assert outs[0]["Wk"][:, 1].any() and outs[0]["vec"][:, 2 * _R + _M + 1].any()     # (both components ran; g_0 and mu^T w written)
    for name in outs[0]:
        assert torch.equal(outs[0][name], outs[1][name]), name


def test_grouped_layout_reads_the_held_out_folds_means(be):
    """n = 6 models in 2 groups over 3 folds, model m holding out fold model_fold[m]: every bit is that of the plain layout on a
    state whose per-model means are rows model_fold[m] of the per-fold means."""
    dims, n, folds = BLOCK_SETS[0], 6, 3
    mf = np.array([2, 0, 1, 1, 2, 0])
    Ss, Gy = planted_blocks(dims, _M, n, seed=11)
    means = _means(dims, folds, seed=4)
    st, shared, own = _hand_state(be, Ss, Gy, dims, means, folds=folds, slots=2)
    ok, Wk, Wl = _run(be, st, dims, model_fold=_t(be, mf, torch.int32), groups=2)
    assert ok is True
    _check(shared, own, Wk, Wl, Ss, Gy, dims, means, model_fold=mf)
    pst, pshared, pown = _hand_state(be, Ss, Gy, dims, [mu[mf] for mu in means])
    ok, pWk, pWl = _run(be, pst, dims)
    assert ok is True
    assert torch.equal(Wk, pWk) and torch.equal(Wl, pWl)
    for name in ("Q", "vec", "n_iter", "status"):
        assert torch.equal(shared[name], pshared[name]), name
    for o, po in zip(own, pown):
        for name in ("Wa", "Wb", "WA", "WB"):
            assert torch.equal(o[name], po[name]), name


def test_null_mode_loadings_are_accepted(be):
    dims = BLOCK_SETS[2]
    Ss, Gy = planted_blocks(dims, _M, _K, seed=5)
    means = _means(dims, _K)
    got = []
    for out in (True, False):
        st, shared, own = _hand_state(be, Ss, Gy, dims, means)
        ok, _, _ = _run(be, st, dims, out=out)
        assert ok is True
        got.append((shared, own))
    assert got[1][0]["n_iter"][:, 0].all()
    for name in ("Q", "vec", "n_iter"):
        assert torch.equal(got[0][0][name], got[1][0][name]), name
    for o, po in zip(got[0][1], got[1][1]):
        assert torch.equal(o["Wa"], po["Wa"]) and torch.equal(o["Wb"], po["Wb"])


def _zero_state(be, dims, M):
    blocks = [(*view(d), be.zeros(_K, M, int(np.prod(d))), be.zeros(_K, int(np.prod(d)))) for d in dims]
    return kfold._state(be, _t(be, np.arange(_I) % _K, torch.int32), be.zeros(_K, _I, M), blocks, _R, 1)


def test_limits_are_checked_before_the_launch(be):
    lib, ws = be.lib, torch.empty(1 << 20, dtype=torch.uint8, device=be.device)

    def call(st, pairs, mf=None, groups=1):
        flat = (ctypes.c_int * (2 * len(pairs)))(*[v for p in pairs for v in p])
        return lib.cmtfpls_kfold_inner_coupled_tensor_f64(st, len(st), flat, mf, groups, 0, 1e-8, 100, None, None, ws.data_ptr(),
                                                          ws.numel(), None)

    def untouched(shared, own):
        torch.cuda.synchronize()
        assert not shared["n_iter"].any() and not shared["status"].any() and not any(o["Wa"].any() for o in own)

    dims = [(5, 7, 3), (1, 9)]
    st, shared, own = _zero_state(be, dims, 1)
    assert call(st, [(7, 4), (0, 0)]) == 1                                           # CMTFPLS_EINVAL: B != B1 * B2
    assert call(st, [(7, 3), (9, 0)]) == 1 and call(st, [(7, 3), (0, 0)], None, 2) == 1   # half a pair; groups without model_fold
    assert be.kfold_inner_coupled_tensor_workspace_bytes(st, [(7, 4), (0, 0)]) == 0
    # per fold: Z, Zt (2 pmax), G0, G1 (2 n^2, n = 7), the blocks' wk (psum), U, yl, vr (3 x the tensor block's P)
    assert be.kfold_inner_coupled_tensor_workspace_bytes(st, _tensor(dims)) == _K * 8 * (2 * 105 + 2 * 7 * 7 + (105 + 9) + 3 * 105)
    untouched(shared, own)
    # a mode-1 unfolding with short side min(257, 7 * 37) = 257, every other limit kept (min(A, B) = 7, 152288 bytes for kfold_inner)
    big = [(4, 6), (7, 257, 37)]
    st, shared, own = _zero_state(be, big, 1)
    assert be.kfold_inner_coupled_tensor(st, _tensor(big), 0, 1e-8, 100, ws) is None
    assert b"shorter side" in lib.cmtfpls_last_error()
    untouched(shared, own)
    # each block within its own limits, their vectors together beyond 150 KB of LDS
    wide = [(1, 9000), (2, 90, 90)]
    assert kfold.coupled_tensor_lds_bytes([view(d) for d in wide], _tensor(wide), 1) > 150 * 1024
    st, shared, own = _zero_state(be, wide, 1)
    assert be.kfold_inner_coupled_tensor(st, _tensor(wide), 0, 1e-8, 100, ws) is None
    assert b"LDS" in lib.cmtfpls_last_error()
    untouched(shared, own)
