"""The cross-covariance iteration and the carry of S between components, entry by entry, against float64 / extended precision.

What is specified here (tests/xcov_iterate_ref.py is the restatement, checked on the CPU by test_xcov_iterate_ref_cpu.py):

  cmtfpls_xcov_iterate_f64          Z = S^T q_cur (only when first), (wA, wB) = leading pair of Z, q_new = S w / |S w|,
                                    du2 = dq^T G dq, info = [converged, squarings used]; S and q_cur are read only
  cmtfpls_xcov_iterate_blocks_f64   the same per block with Z from S (x n / colcnt), Y^T t from S2, tq laid out (nb, M),
                                    q_new from the SUM of the rows, status = [du2, (converged, used) per block]
  cmtfpls_s_downdate_f64, cmtfpls_axpy_scalar_f64, cmtfpls_sum_f64, cmtfpls_kr_gram_row_f64, cmtfpls_kr_axpy_f64 (refusal)

Every stage is compared with the restatement evaluated on the DEVICE's output of the stage before it, so no tolerance
compounds.  Tolerances are of two kinds only:

  * the worst-case bound of the sum involved, |err| <= 2 n u sum|terms| with u = 2^-53 and n the length of the fma chain or
    dot product (one n u for the kernel in any order of summation, the other for the reference -- which is evaluated in
    np.longdouble where that is wider than float64, and then spends almost none of its half);
  * for the loadings against LAPACK, the figures of test_gpu_kernels.py on the same construction of Z (unit noise plus 3 x a
    rank-one term): atol 1e-10 for sides up to 256 (test_rank1_matches_lapack), atol 1e-9 beyond (test_rank1_large).
"""
import math

import numpy as np
import pytest
import torch

import xcov_iterate_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
BUDGET = 30            # the engine's budget ceiling of squarings (HipBackend.rank1_squarings)


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _host(t):
    return t.cpu().numpy().copy()


def _ld(a):
    return np.asarray(a, dtype=LD)


def _within(got, want, bound, what):
    """|got - want| <= bound elementwise; prints the worst figure first so that a run kept in a file shows every margin."""
    got, want, bound = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.size == 0:
        return
    assert np.isfinite(got).all(), (what, "not finite")
    err = np.abs(_ld(got) - _ld(want)).astype(np.float64)
    bound = np.broadcast_to(bound, err.shape)
    i = int(np.argmax(err - bound))
    print(f"{what}: worst err {err.flat[i]:.3e} against bound {bound.flat[i]:.3e} (max err {err.max():.3e})")
    assert (err <= bound).all(), (what, float(err.flat[i]), float(bound.flat[i]), i)


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, np.abs(a - b).max())


def _lapack_atol(A, B):
    # test_gpu_kernels.py: test_rank1_matches_lapack (sides up to 256) / test_rank1_large (beyond) on this construction of Z
    return 1e-10 if max(A, B) <= 256 else 1e-9


# ---- the stages, each against the restatement on the device's own input to it ---------------------------------------------

def _check_z(Zd, S, q, colcnt=None, n_samples=None, what="Z"):
    """Z[c] is one chain of M fmas (then / colcnt * n_samples: two more roundings): 2 (M + 2) u sum_m |q_m S_mc| (scaled alike)."""
    M = S.shape[0]
    want = R.z_of(_ld(S), _ld(q), colcnt, n_samples)
    terms = R.z_of(np.abs(S), np.abs(q), colcnt, n_samples)
    _within(Zd, want, 2 * (M + 2) * U * terms, what)
    if colcnt is not None:
        assert np.all(Zd[colcnt <= 0] == 0.0), what + ": a column never observed must be exactly 0"


def _check_loadings3(wA, wB, Zd, A, B, what="loadings"):
    rA, rB = R.loadings_of(Zd, A, B, 3)
    atol = _lapack_atol(A, B)
    _within(wA, rA, atol, what + " wA")
    _within(wB, rB, atol, what + " wB")


def _check_vector_loading(wB, Zd, what="wB"):
    """wB = Z / |Z|: a sum of P squares, a square root and a division: 2 (P + 2) u |wB_c|; an exact 0 stays an exact 0."""
    P = Zd.size
    z = _ld(Zd)
    want = z / np.sqrt((z * z).sum())
    _within(wB, want, 2 * (P + 2) * U * np.abs(want).astype(np.float64), what)
    assert np.all(wB[Zd == 0.0] == 0.0)


def _check_tq(tq, S, wA, wB, what="tq"):
    """tq[m] = S[m, :] . kron(wA, wB): a dot product of P terms, 2 P u sum_c |S_mc w_c| (P = 1: one rounding)."""
    P = S.shape[1]
    want = R.tq_of(_ld(S), _ld(wA), _ld(wB))
    terms = R.tq_of(np.abs(S), np.abs(wA), np.abs(wB))
    _within(tq, want, 2 * P * U * terms, what)


def _check_q(q_new, tq_rows, what="q_new"):
    """q = s / |s| with s the sum of the nb rows: nb - 1 additions per entry (2 nb u sum_b |tq_b,i| / |s|), then M squares,
    a square root and a division (2 (M + 2) u |q_i|)."""
    rows = np.atleast_2d(tq_rows)
    nb, M = rows.shape
    want = R.q_of(list(_ld(rows)))
    s_norm = float(np.sqrt((_ld(rows).sum(axis=0) ** 2).sum()))
    bound = 2 * (M + 2) * U * np.abs(want).astype(np.float64)
    if nb > 1:
        bound = bound + 2 * nb * U * np.abs(rows).sum(axis=0) / s_norm
    _within(q_new, want, bound, what)


def _check_du2(du2, G, q_new, q_cur, what="du2"):
    """du2 = sum_ij dq_i G_ij dq_j: M^2 terms of two products each on dq = fl(q_new - q_cur): 2 (M^2 + 4) u sum |dq_i G_ij dq_j|.
    (Near convergence the terms cancel and du2 may come out with either sign: only the bound is asserted.)"""
    M = q_new.size
    want = R.du2_of(_ld(G), _ld(q_new), _ld(q_cur))
    _within(float(du2), float(want), 2 * (M * M + 4) * U * float(R.du2_abs_terms(G, q_new, q_cur)), what)


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def _unit(rng, M):
    q = rng.normal(size=M)
    return q / np.linalg.norm(q)


def _make_s(rng, A, B, q):
    """S (M, A*B) = sum of rank-one rows plus noise such that Z = S^T q is exactly the construction of test_rank1_matches_lapack:
    unit normal noise plus 3 x outer(normal, normal).  (The coefficients c have c . q = 1, and |q| = 1 keeps the noise at unit variance.)"""
    M = q.size
    r = rng.normal(size=M)
    c = q + (r - (r @ q) * q)
    return np.outer(c, 3.0 * np.kron(rng.normal(size=A), rng.normal(size=B))) + rng.normal(size=(M, A * B))


def _make_z(rng, A, B):
    return rng.normal(size=A * B) + 3.0 * np.kron(rng.normal(size=A), rng.normal(size=B))


def _slow_z(rng, A, B):
    """The slowly decaying spectrum 0.93^k of test_rank1_chain_of_squarings_in_one_launch_...: two squarings do not converge."""
    n = min(A, B)
    Ua, _ = np.linalg.qr(rng.normal(size=(A, n)))
    Vb, _ = np.linalg.qr(rng.normal(size=(B, n)))
    return ((Ua * (0.93 ** np.arange(n))) @ Vb.T).ravel()


def _gram(rng, M):
    Y = rng.normal(size=(3 * M + 5, M))
    return Y.T @ Y


class _Bufs:
    """Output buffers of one order-3 block, filled with a sentinel."""

    def __init__(self, be, A, B, M, Z=None):
        self.Z = _dev(Z) if Z is not None else _dev(np.full(A * B, -7.0))
        self.wA, self.wB = _dev(np.full(A, -7.0)), _dev(np.full(B, -7.0))
        self.info, self.q_new, self.du2 = _dev(np.full(2, -7.0)), _dev(np.full(M, -7.0)), _dev(np.full(1, -7.0))

    def host(self):
        return {k: _host(getattr(self, k)) for k in ("Z", "wA", "wB", "info", "q_new", "du2")}


def _iterate(be, Sd, A, B, qd, Gd, first, Z=None, budget=BUDGET):
    b = _Bufs(be, A, B, qd.numel(), Z)
    be.xcov_iterate(Sd, A, B, qd, b.Z, b.wA, b.wB, b.info, budget, b.q_new, Gd, b.du2, first)
    return b.host()


def _all_same_bits(x, y, what, keys=("Z", "wA", "wB", "info", "q_new", "du2")):
    for k in keys:
        _same_bits(x[k], y[k], f"{what}: {k}")


# ---- 2a. cmtfpls_xcov_iterate_f64 ----------------------------------------------------------------------------------------------

ITERATE_CASES = [
    (128, 128, 16),    # P >= 8192: the extraction's final kernel and the score share a launch; the squarings run in one launch
    (64, 128, 64),     # P = 8192 exactly, M at its limit
    (64, 127, 5),      # P < 8192 and B odd: rank1 and score_s as two entries
    (90, 92, 33),      # P = 8280, no multiple of 2048: the tail loop of the row walk; M = 33: the 64-lane q_update layout
    (256, 64, 17),     # A > B: Z transposed inside; M = 17: the 32-lane layout
    (5, 7, 1),         # M = 1
    (600, 640, 4),     # min(A, B) beyond the one-launch chain: a launch per squaring
]


@pytest.mark.parametrize("A,B,M", ITERATE_CASES)
def test_xcov_iterate_stage_by_stage(be, A, B, M):
    rng = np.random.default_rng(1000 * A + 10 * B + M)
    q = _unit(rng, M)
    S, G = _make_s(rng, A, B, q), _gram(rng, M)
    Sd, qd, Gd = _dev(S), _dev(q), _dev(G)

    a = _iterate(be, Sd, A, B, qd, Gd, True)
    _same_bits(_host(Sd), S, "S is read only")
    _same_bits(_host(qd), q, "q_cur is read only")
    _check_z(a["Z"], S, q)
    _check_loadings3(a["wA"], a["wB"], a["Z"], A, B)
    assert a["info"][0] == 1.0 and 1 <= a["info"][1] <= BUDGET and a["info"][1] == int(a["info"][1]), a["info"]

    # the entry documents itself as rank1_score, then q_update, on the Z it formed: that pair shows Y^T t before the division
    Zd = _dev(a["Z"])
    wA, wB, tq, info, du2 = be.empty(A), be.empty(B), _dev(np.full(M, -7.0)), be.zeros(2), be.zeros(1)
    be.rank1_score(Zd, A, B, wA, wB, Sd, tq, info=info, n_squarings=BUDGET)
    tq_h = _host(tq)
    be.q_update(tq, None, True, Gd, qd, du2)
    pair = dict(Z=_host(Zd), wA=_host(wA), wB=_host(wB), info=_host(info), q_new=_host(tq), du2=_host(du2))
    _all_same_bits(a, pair, "first=True against rank1_score + q_update")
    _check_tq(tq_h, S, a["wA"], a["wB"])
    _check_q(a["q_new"], tq_h)
    _check_du2(a["du2"][0], G, a["q_new"], q)

    # first=False on the same Z: the same calls, the same bits
    _all_same_bits(_iterate(be, Sd, A, B, qd, Gd, False, Z=a["Z"]), pair, "first=False against rank1_score + q_update")
    # two identical calls
    _all_same_bits(_iterate(be, Sd, A, B, qd, Gd, True), a, "a second identical call")

    # first=False extracts from what Z holds and leaves it alone
    Z2 = _make_z(rng, A, B)
    b = _iterate(be, Sd, A, B, qd, Gd, False, Z=Z2)
    _same_bits(b["Z"], Z2, "first=False must not write Z")
    _check_loadings3(b["wA"], b["wB"], Z2, A, B, "loadings of Z2")
    _check_q_through_tq(b["q_new"], S, b["wA"], b["wB"], "q_new of Z2")
    _check_du2(b["du2"][0], G, b["q_new"], q, "du2 of Z2")
    assert b["info"][0] == 1.0

    # the plan's closure: du2 to status[0], (converged, used) to status[1:3], the bits of xcov_iterate
    p = _Bufs(be, A, B, M)
    status = _dev(np.full(3, -7.0))
    enqueue = be.xcov_iterate_plan(Sd, A, B, qd, p.Z, p.wA, p.wB, status, p.q_new, Gd)
    enqueue(BUDGET, True)
    ph, st = p.host(), _host(status)
    _all_same_bits(ph, a, "plan", keys=("Z", "wA", "wB", "q_new"))
    _same_bits(st[0:1], a["du2"], "plan: status[0] = du2")
    _same_bits(st[1:3], a["info"], "plan: status[1:3] = info")
    p.Z.copy_(_dev(Z2))
    enqueue(BUDGET, False)
    _all_same_bits(p.host(), b, "plan, first=False", keys=("Z", "wA", "wB", "q_new"))
    _same_bits(_host(status), np.concatenate([b["du2"], b["info"]]), "plan, first=False: status")

    # a second iteration from q_new is near convergence: du2 is tiny and still within its bound
    q1d = _dev(a["q_new"])
    c = _iterate(be, Sd, A, B, q1d, Gd, True)
    _check_z(c["Z"], S, a["q_new"], what="Z (second iteration)")
    _check_loadings3(c["wA"], c["wB"], c["Z"], A, B, "loadings (second iteration)")
    assert c["info"][0] == 1.0
    tq2 = _dev(np.full(M, -7.0))
    be.score_s(Sd, A, B, _dev(c["wA"]), _dev(c["wB"]), tq2)
    _check_tq(_host(tq2), S, c["wA"], c["wB"], "tq (second iteration, score_s)")
    _check_du2(c["du2"][0], G, c["q_new"], a["q_new"], "du2 (second iteration)")
    print(f"du2: first {a['du2'][0]:.3e}, second {c['du2'][0]:.3e}")
    assert abs(c["du2"][0]) <= abs(a["du2"][0])


def _check_q_through_tq(q_new, S, wA, wB, what):
    """q_new when Y^T t itself is not visible: tq within bt (the dot-product bound) moves q = t / |t| by at most
    bt_i / |t| + |q_i| sum_j |t_j| bt_j / |t|^2 to first order, plus the normalisation's own 2 (M + 2) u |q_i|."""
    P, M = S.shape[1], S.shape[0]
    t = R.tq_of(_ld(S), _ld(wA), _ld(wB))
    bt = 2 * P * U * R.tq_of(np.abs(S), np.abs(wA), np.abs(wB))
    nt = float(np.sqrt((t * t).sum()))
    want = t / nt
    aq = np.abs(want).astype(np.float64)
    bound = bt / nt + aq * float((np.abs(t).astype(np.float64) * bt).sum()) / nt ** 2 + 2 * (M + 2) * U * aq
    _within(q_new, want, bound, what)


@pytest.mark.parametrize("A,B", [(128, 128), (40, 30)])
def test_xcov_iterate_redo_contract(be, A, B):
    """What the pipelined loop relies on: a call whose budget ran out reports info[0] = 0, and the first=False call that follows
    with the full budget is a single call with the full budget, bit for bit."""
    rng = np.random.default_rng(A * 7 + B)
    M = 6
    q = _unit(rng, M)
    S = np.outer(q, _slow_z(rng, A, B)) + 1e-3 * rng.normal(size=(M, A * B))
    G = _gram(rng, M)
    Sd, qd, Gd = _dev(S), _dev(q), _dev(G)
    bufs = _Bufs(be, A, B, M)

    def call(budget, first):
        be.xcov_iterate(Sd, A, B, qd, bufs.Z, bufs.wA, bufs.wB, bufs.info, budget, bufs.q_new, Gd, bufs.du2, first)
        return bufs.host()

    short = call(2, True)
    assert short["info"].tolist() == [0.0, 2.0], short["info"]
    redo = call(BUDGET, False)
    assert redo["info"][0] == 1.0 and 2 < redo["info"][1] <= BUDGET, redo["info"]
    _same_bits(redo["Z"], short["Z"], "the redo leaves Z alone")
    _all_same_bits(redo, _iterate(be, Sd, A, B, qd, Gd, True), "redo against one call with the full budget")


def test_xcov_iterate_refuses_more_than_64_responses(be):
    from cmtf_pls_amd import _lib
    A, B, M = 8, 8, 65
    rng = np.random.default_rng(65)
    Sd, qd, Gd = _dev(rng.normal(size=(M, A * B))), _dev(_unit(rng, M)), _dev(_gram(rng, M))
    b = _Bufs(be, A, B, M)
    with pytest.raises(_lib.CmtfplsError, match="64 responses"):
        be.xcov_iterate(Sd, A, B, qd, b.Z, b.wA, b.wB, b.info, BUDGET, b.q_new, Gd, b.du2, True)
    torch.cuda.synchronize()
    for k, v in b.host().items():
        assert np.all(v == -7.0), k


# ---- 2b. cmtfpls_xcov_iterate_blocks_f64 ---------------------------------------------------------------------------------------

def _colcnt(rng, A, B, n_samples):
    """Observation counts with zeros (columns never observed); an order-3 block also loses one whole slice b = B // 3.  The last
    column stays observed: the scaling writes 0 over a column never observed, which would hide a tail of Z left unwritten."""
    P = A * B
    c = rng.integers(n_samples // 2, n_samples + 1, size=P).astype(np.float64)
    if P > 1:                                # (a matrix block of ONE column never observed has no loading at all: 0 / 0)
        c[rng.choice(P - 1, size=max(1, P // 7), replace=False)] = 0.0
    if A > 1:
        c.reshape(A, B)[:, B // 3] = 0.0
    return c


def _run_blocks(be, specs, M, seed, budgets=None, n_samples=40):
    """One first=True iteration of cmtfpls_xcov_iterate_blocks_f64 on blocks described by dicts (order, A, B, masked, slow),
    every stage checked; returns the status words.  masked: an S2 that is an INDEPENDENT random matrix (using S where S2 is due,
    or the reverse, is then far outside any bound) and a colcnt with zeros."""
    rng = np.random.default_rng(seed)
    nb = len(specs)
    q, G = _unit(rng, M), _gram(rng, M)
    host, blocks = [], []
    for sp in specs:
        A, B = sp["A"], sp["B"]
        P = A * B
        if sp.get("slow"):
            S = np.outer(q, _slow_z(rng, A, B)) + 1e-3 * rng.normal(size=(M, P))
        else:
            S = _make_s(rng, A, B, q)
        S2 = rng.normal(size=(M, P)) if sp.get("masked") else None
        cc = _colcnt(rng, A, B, n_samples) if sp.get("masked") else None
        host.append((S, S2, cc))
        blocks.append(dict(S=_dev(S), S2=None if S2 is None else _dev(S2), colcnt=None if cc is None else _dev(cc),
                           n_samples=float(n_samples), order=sp["order"], A=A, B=B, Z=_dev(np.full(P, -7.0)),
                           wA=_dev(np.ones(1)) if sp["order"] == 2 else _dev(np.full(A, -7.0)), wB=_dev(np.full(B, -7.0))))
    qd, Gd = _dev(q), _dev(G)
    tq, q_new, status = _dev(np.full(nb * M, -7.0)), _dev(np.full(M, -7.0)), _dev(np.full(1 + 2 * nb, -7.0))
    enqueue = be.xcov_blocks_plan(blocks, M, qd, tq, q_new, Gd, status)
    assert enqueue is not None
    budgets = budgets or [BUDGET] * nb
    enqueue(budgets, True)
    st, tq_h, q_h = _host(status), _host(tq).reshape(nb, M), _host(q_new)
    _same_bits(_host(qd), q, "q_cur is read only")
    for i, (sp, b, (S, S2, cc)) in enumerate(zip(specs, blocks, host)):
        A, B, tag = sp["A"], sp["B"], f"block {i} "
        _same_bits(_host(b["S"]), S, tag + "S is read only")
        Zd, wA, wB = _host(b["Z"]), _host(b["wA"]), _host(b["wB"])
        _check_z(Zd, S, q, cc, float(n_samples), tag + "Z")                               # Z comes from S ...
        if sp["order"] == 2:
            _check_vector_loading(wB, Zd, tag + "wB")
            assert wA.tolist() == [1.0]
            assert st[1 + 2 * i: 3 + 2 * i].tolist() == [-7.0, -7.0], tag + "a matrix block has no status words"
        else:
            flag, used = st[1 + 2 * i], st[2 + 2 * i]
            assert 1 <= used <= budgets[i] and used == int(used), (tag, st)
            if budgets[i] == BUDGET:
                assert flag == 1.0, (tag, st)
            if not sp.get("slow"):
                _check_loadings3(wA, wB, Zd, A, B, tag + "loadings")
        if cc is not None:                                                                 # exact zeros, not merely small ones
            assert (cc <= 0).any() or A * B == 1
            assert np.all(wB[(cc <= 0).reshape(A, B).all(axis=0)] == 0.0), tag + "wB of a slice never observed"
        _check_tq(tq_h[i], S if S2 is None else S2, wA, wB, tag + "tq")                  # ... and Y^T t from S2
    _check_q(q_h, tq_h)
    _check_du2(st[0], G, q_h, q)
    # a second identical call: the same bits
    enqueue(budgets, True)
    _same_bits(_host(status), st, "status of a second identical call")
    _same_bits(_host(tq).reshape(nb, M), tq_h, "tq of a second identical call")
    _same_bits(_host(q_new), q_h, "q_new of a second identical call")
    return st


MATRIX_CASES = [(1, 1), (1, 17), (63, 16), (63, 64), (1000, 1), (1000, 17), (1025, 16), (1025, 64), (8192, 17), (8192, 64),
                (8193, 16), (8200, 33)]        # the last two: s_contract + colscale + normalize_to + score_s


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("P,M", MATRIX_CASES)
def test_blocks_matrix_block(be, P, M, masked):
    _run_blocks(be, [dict(order=2, A=1, B=P, masked=masked)], M, seed=P * 100 + M)


@pytest.mark.parametrize("A,B,M", [(32, 64, 6),        # P < 8192: rank1, then score_s on S2
                                   (64, 128, 33)])     # P = 8192: the final kernel scores the rows of S2 in its own launch
def test_blocks_order3_with_s2_and_colcnt(be, A, B, M):
    _run_blocks(be, [dict(order=3, A=A, B=B, masked=True)], M, seed=A + B + M)


@pytest.mark.parametrize("M", [5, 40])
@pytest.mark.parametrize("nb", [2, 3])
def test_blocks_coupled(be, nb, M):
    specs = [dict(order=3, A=32, B=64), dict(order=2, A=1, B=96)]
    if nb == 3:
        specs = [dict(order=3, A=32, B=64), dict(order=3, A=64, B=128, masked=True), dict(order=2, A=1, B=96, masked=True)]
    _run_blocks(be, specs, M, seed=nb * 1000 + M)


def test_blocks_budgets_are_per_block(be):
    """Block 0 gets two squarings on the slow spectrum, block 1 the full budget: the flags read 0 and 1 (and the matrix block's
    words are left alone, _run_blocks)."""
    specs = [dict(order=3, A=32, B=64, slow=True), dict(order=3, A=64, B=128, masked=True), dict(order=2, A=1, B=96)]
    st = _run_blocks(be, specs, 5, seed=77, budgets=[2, BUDGET, BUDGET])
    assert st[1:3].tolist() == [0.0, 2.0] and st[3] == 1.0, st


def test_blocks_first_false_extracts_from_what_z_holds(be):
    """first=False: an order-3 block's Z is not rebuilt (the redo of an extraction whose budget ran out)."""
    rng = np.random.default_rng(78)
    A, B, M = 32, 64, 5
    q, G = _unit(rng, M), _gram(rng, M)
    S, Z2 = _make_s(rng, A, B, q), _make_z(rng, A, B)
    blk = dict(S=_dev(S), S2=None, colcnt=None, n_samples=1.0, order=3, A=A, B=B, Z=_dev(Z2), wA=be.empty(A), wB=be.empty(B))
    tq, q_new, status = be.empty(M), be.empty(M), be.zeros(3)
    enqueue = be.xcov_blocks_plan([blk], M, _dev(q), tq, q_new, _dev(G), status)
    enqueue([BUDGET], False)
    _same_bits(_host(blk["Z"]), Z2, "first=False must not write Z")
    _check_loadings3(_host(blk["wA"]), _host(blk["wB"]), Z2, A, B)
    _check_tq(_host(tq), S, _host(blk["wA"]), _host(blk["wB"]))


def test_blocks_declines(be):
    rng = np.random.default_rng(79)

    def blk(order, A, B, M):
        return dict(S=_dev(rng.normal(size=(M, A * B))), S2=None, colcnt=None, n_samples=1.0, order=order, A=A, B=B,
                    Z=be.empty(A * B), wA=be.empty(A), wB=be.empty(B))

    def plan(blocks, M, tq_len):
        return be.xcov_blocks_plan(blocks, M, be.empty(M), be.empty(tq_len), be.empty(M), be.empty(M, M), be.empty(1 + 2 * len(blocks)))

    assert plan([blk(3, 4, 5, 65)], 65, 65) is None               # more than 64 responses
    assert plan([blk(4, 4, 5, 3)], 3, 3) is None                  # a block of order 4
    assert plan([blk(3, 4, 5, 3)], 3, 4) is None                  # tq is not (nb, M)
    assert plan([blk(3, 4, 5, 3), blk(2, 1, 9, 3)], 3, 3) is None
    assert plan([blk(3, 4, 5, 3)], 3, 3) is not None


# ---- 2c. the carry between components -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("A,B,M", [(7, 37, 1), (1, 300, 5), (128, 128, 64), (33, 8, 17)])
def test_s_downdate(be, A, B, M):
    """Each element is S - ya w - q v by two fmas on w = fl(wA wB): 3 u (|S| + |ya w| + |q v|)."""
    rng = np.random.default_rng(A * 100 + B + M)
    P = A * B
    S = rng.normal(size=(M, P))
    ya, wA, wB, q, v = rng.normal(size=M), rng.normal(size=A), rng.normal(size=B), rng.normal(size=M), rng.normal(size=P)
    Sd = _dev(S)
    args = [_dev(x) for x in (ya, wA, wB, q, v)]
    be.s_downdate(Sd, A, B, *args)
    want = R.s_downdate_of(_ld(S), _ld(ya), _ld(wA), _ld(wB), _ld(q), _ld(v))
    terms = np.abs(S) + np.outer(np.abs(ya), np.kron(np.abs(wA), np.abs(wB))) + np.outer(np.abs(q), np.abs(v))
    _within(_host(Sd), want, 3 * U * terms, "S+")
    for x, h in zip(args, (ya, wA, wB, q, v)):
        _same_bits(_host(x), h, "the operands are read only")


@pytest.mark.parametrize("A,B,M", [(7, 37, 1), (1, 300, 5), (128, 128, 64), (33, 8, 17)])
def test_s_downdate_carries_s_across_a_deflation(be, A, B, M):
    """S = Y^T X from be.xcov on a device X, down-dated, is Y+^T X+ of the deflated pair: |S+ - S'|_inf <= 1e-12 |S'|_inf, the
    relative tolerance the project's xcov tests use (test_xcov_iterate_ref_cpu.py::test_carry_identity is the host side)."""
    rng = np.random.default_rng(A * 100 + B + M + 1)
    I, P = 50, A * B
    latent = rng.normal(size=I)
    X = 3.0 * np.outer(latent, np.kron(rng.normal(size=A), rng.normal(size=B))) + rng.normal(size=(I, P))
    Y = np.outer(latent, rng.normal(size=M)) + 0.5 * rng.normal(size=(I, M))
    X -= X.mean(axis=0)
    Y -= Y.mean(axis=0)
    q = _unit(rng, M)
    Sd = be.xcov(_dev(X), _dev(Y), False)
    S = _host(Sd)
    wA, wB = R.loadings_of(R.z_of(S, q), A, B, 3 if A > 1 else 2)
    w = np.kron(wA, wB)
    t = X @ w
    yhat = t * (t @ (Y @ q) / (t @ t))
    Xp, Yp = X - np.outer(t, w), Y - np.outer(yhat, q)
    be.s_downdate(Sd, A, B, _dev(Y.T @ t), _dev(wA), _dev(wB), _dev(q), _dev(Xp.T @ yhat))
    want = Yp.T @ Xp
    err, scale = np.abs(_host(Sd) - want).max(), np.abs(want).max()
    print(f"carry: err {err:.3e} against {1e-12 * scale:.3e}")
    assert err <= 1e-12 * scale


@pytest.mark.parametrize("with_x", [False, True])
@pytest.mark.parametrize("n", [1, 255, 257, 1024 * 256 + 3])       # the last: the grid-stride loop beyond the 1024-workgroup cap
def test_axpy_scalar(be, n, with_x):
    """y[i] = fma(-a, x[i], y[i]): one rounding of a result no larger than |y| + |a x|, so 2^-52 (|y| + |a x|) with room."""
    rng = np.random.default_rng(n)
    y, a = rng.normal(size=n), rng.normal(size=3)
    x = rng.normal(size=n) if with_x else None
    yd, ad = _dev(y), _dev(a)
    xd = _dev(x) if with_x else None
    be.axpy_scalar(yd, ad, xd)
    xx = x if with_x else np.ones(n)
    _within(_host(yd), _ld(y) - _ld(a[0]) * _ld(xx), 2.0 ** -52 * (np.abs(y) + np.abs(a[0] * xx)), "axpy_scalar")
    _same_bits(_host(ad), a, "a is read only")
    if with_x:
        _same_bits(_host(xd), x, "x is read only")


@pytest.mark.parametrize("n", [1, 1023, 1025, 100003])
def test_total(be, n):
    """A sum of n terms in any order: n 2^-53 sum |v| against math.fsum (exactly rounded); fixed order, so two calls agree bit for bit."""
    rng = np.random.default_rng(n)
    v = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, size=n)
    vd = _dev(v)
    got, again = _host(be.total(vd)), _host(be.total(vd))
    _within(got, np.array([math.fsum(v)]), n * U * math.fsum(np.abs(v)), "total")
    _same_bits(got, again, "two calls")
    _same_bits(_host(vd), v, "v is read only")


@pytest.mark.parametrize("Rk", [2, 10, 64, 300])                       # 300 with a = 299: the stride over j
def test_kr_gram_row(be, Rk):
    """g[:a] (*)= L[:, :a]^T L[:, a]: dot products of n terms, 2 n u sum |terms|; the second mode multiplies into g (one more
    rounding, and the first mode's error scaled by the second row).  n covers the 16-row unroll and its tail."""
    rng = np.random.default_rng(Rk)
    for n in (1, 15, 16, 17, 33, 128):
        L1, L2 = rng.normal(size=(n, Rk)), rng.normal(size=(n + 3, Rk))
        L1d, L2d = _dev(L1), _dev(L2)
        G = be.kr_gram(L2d, be.kr_gram(L1d, be.empty(Rk, Rk), True), False)
        G1 = _host(be.kr_gram(L1d, be.empty(Rk, Rk), True))
        Gh = _host(G)
        for a in sorted({0, 1, Rk - 1}):
            g = _dev(np.full(Rk, -7.0))
            be.kr_gram_row(L1d, a, g, True)
            g1 = _host(g)
            assert np.all(g1[a:] == -7.0), (n, a, "g[a:] keeps its sentinel (a = 0 writes nothing)")
            want1 = R.kr_gram_row_of(_ld(L1), a, _ld(np.full(Rk, -7.0)), True)[:a]
            b1 = 2 * n * U * (np.abs(L1[:, :a]) * np.abs(L1[:, a:a + 1])).sum(axis=0)
            _within(g1[:a], want1, b1, f"kr_gram_row first n={n} a={a}")
            _within(g1[:a], G1[a, :a], b1, f"kr_gram_row first against kr_gram n={n} a={a}")
            be.kr_gram_row(L2d, a, g, False)
            g2 = _host(g)
            assert np.all(g2[a:] == -7.0), (n, a)
            row2 = (_ld(L2[:, :a]) * _ld(L2[:, a:a + 1])).sum(axis=0)
            b2 = 2 * (n + 3) * U * (np.abs(L2[:, :a]) * np.abs(L2[:, a:a + 1])).sum(axis=0)
            # (g1 + e1)(row2 + e2) rounded once: |row2| b1 + |g1| b2 + u |g1 row2| (+ the product of the two errors, covered by the 2s)
            bound = np.abs(row2).astype(np.float64) * b1 + np.abs(want1).astype(np.float64) * b2 + U * np.abs(want1 * row2).astype(np.float64)
            _within(g2[:a], want1 * row2, bound, f"kr_gram_row second n={n} a={a}")
            _within(g2[:a], Gh[a, :a], bound, f"kr_gram_row second against kr_gram n={n} a={a}")


def test_kr_axpy_refuses_more_than_64_terms(be):
    from cmtf_pls_amd import _lib
    rng = np.random.default_rng(3)
    A, B, k = 5, 6, 65
    v = _dev(np.full(A * B, -7.0))
    with pytest.raises(_lib.CmtfplsError, match="64 terms"):
        be.kr_axpy(v, A, B, _dev(rng.normal(size=(A, k))), _dev(rng.normal(size=(B, k))), k, _dev(rng.normal(size=k)))
    torch.cuda.synchronize()
    assert np.all(_host(v) == -7.0)
