"""The small f64 kernels between the X sweeps (csrc/small.hip, csrc/solve.hip, kron of csrc/rank1_tensor.hip) and the calcR2X
pass of csrc/recon.hip at their edges: past one grid round, across the 64-wide tiles, with leading dimensions wider than the
operand, and in the forms the engine calls them (1-D operands, column views, an output inside a larger tensor).

Every case runs on the EXACT inputs of tests/small_algebra_ref.py (integers: the device result equals the restatement bit
for bit, whatever its summation order) and on the ROUNDING inputs (asserting the derived worst-case bound, never a fitted
tolerance), and repeats the call to assert the same bits.  The worst error / bound ratio per kernel is printed at teardown."""
import numpy as np
import pytest
import torch

import small_algebra_ref as SA

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
KINDS = ["exact", "rounding"]
SENTINEL = -7.25e300
LD = np.longdouble


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


def dev(a, dtype=F64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV).to(dtype)


def host(t):
    return t.detach().cpu().double().numpy()


def bits(t):
    return t.detach().clone().contiguous().view(torch.int64 if t.dtype == F64 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


_worst = {}


def _record(kernel, ratio):
    _worst[kernel] = max(_worst.get(kernel, 0.0), float(ratio))


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, r in sorted(_worst.items()):
        print(f"worst error / bound {k}: {r:.3f}")


def check(kernel, kind, got, want, bound):
    """exact inputs: equality with the restatement; rounding inputs: |got - want| <= bound elementwise, ratio recorded."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=LD).reshape(got.shape)
    if kind == "exact":
        assert np.array_equal(got, want.astype(np.float64)), (kernel, np.argwhere(got != want.astype(np.float64))[:4])
        return
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape)
    assert np.all(np.isfinite(err)) and np.all(bound > 0), kernel
    ratio = float((err / bound).max())
    print(f"{kernel}: worst error / bound {ratio:.3f}")
    _record(kernel, ratio)
    assert ratio <= 1.0, (kernel, ratio)


def seed(kind, *ints):
    return np.random.default_rng([KINDS.index(kind)] + [int(i) for i in ints])


# ---- gram_tn, gemv form (b = 1): Y^T t of tpls.py:100, T^T u, the rows of Ts ----------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("I,a", SA.GEMV_CASES)
def test_gram_tn_gemv_form(be, kind, I, a):
    rng = seed(kind, 1, I, a)
    W, Tm = SA.inputs(kind, rng, I, a + 8), SA.inputs(kind, rng, I, 5)
    Wd, Td = dev(W), dev(Tm)
    A, v = W[:, 3:3 + a], Tm[:, 2]
    want, mag = SA.gram_tn(A, v)
    bound = SA.bound_sum(I, mag)
    Ac, vc = Wd[:, 3:3 + a].contiguous(), Td[:, 2].contiguous()              # 1-D v: gram_tn(Y, t)
    forms = {"contiguous": (Ac, vc),
             "lda > a, v a column view (ldb = 5)": (Wd[:, 3:3 + a], Td[:, 2:3])}   # gram_tn(T[:, :a], u) / a column of T as v
    if a == 1:
        forms["1-D A and 1-D B"] = (Ac.reshape(I), vc)                        # gram_tn(Ts[b], t)
    first = None
    for name, (Ad, vd) in forms.items():
        got = be.gram_tn(Ad, vd)
        assert got.shape == (a, 1)
        check("gram_tn gemv", kind, host(got), want, bound)
        assert same_bits(got, be.gram_tn(Ad, vd)), name
        first = got if first is None else first
        assert same_bits(got, first), name                                    # the stride changes no bit
    log = torch.full((4, a + 2), SENTINEL, dtype=F64, device=DEV)             # out= a row of a larger tensor (dot_log[a, 0:1])
    be.gram_tn(Wd[:, 3:3 + a], Td[:, 2:3], out=log[1, 0:a])
    assert same_bits(log[1, :a], first.reshape(a))
    log[1, :a] = SENTINEL
    assert bool((log == SENTINEL).all())


# ---- gram_tn, tiled form -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiled_base():
    cache = {}

    def get(kind, I):
        if (kind, I) not in cache:
            W = SA.inputs(kind, seed(kind, 2, I), I, SA.TILED_WIDTH)
            cache[(kind, I)] = (W, dev(W)) + SA.gram_tn(W, W)                # one reference per (kind, I), shared and unchanged
        return cache[(kind, I)]
    return get


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("I", SA.TILED_I)
def test_gram_tn_tiled_form(be, tiled_base, kind, I):
    """TR = 128 / 64 / 32 by a + b, the 64-wide tile edge in both directions with the C + a0 * b + b0 offset, both operands as
    slices (lda = 136) and contiguous -- a contiguous operand wider than 64 has lda == a of the WHOLE but its tiles must take the
    strided branch -- and A and B the same tensor.  I = 128 * 130 + 5 gives 131 rows per workgroup (a second stage of 3 rows with
    TR = 128) and a last workgroup of 8 rows; I = 1, 5 leave workgroups without rows."""
    _, Wd, G, Gmag = tiled_base(kind, I)
    for a, b in SA.TILED_AB:
        ca, cb = SA.tiled_columns(a, b)
        want, bound = G[ca:ca + a, cb:cb + b], SA.bound_sum(I, Gmag[ca:ca + a, cb:cb + b])
        As, Bs = Wd[:, ca:ca + a], Wd[:, cb:cb + b]
        got = be.gram_tn(As, Bs)
        check("gram_tn tiled", kind, host(got), want, bound)
        assert same_bits(got, be.gram_tn(As, Bs)), (a, b)
        Ac, Bc = As.clone(memory_format=torch.contiguous_format), Bs.clone(memory_format=torch.contiguous_format)
        assert same_bits(got, be.gram_tn(Ac, Bc)), (a, b, "contiguous")
        if a == b:
            same = be.gram_tn(Ac, Ac)
            check("gram_tn tiled", kind, host(same), G[ca:ca + a, ca:ca + a], SA.bound_sum(I, Gmag[ca:ca + a, ca:ca + a]))
            assert same_bits(same, same.T), (a, "A^T A is symmetric bit for bit: fma(x, y, s) == fma(y, x, s)")


# ---- rowdot ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("I,M", SA.ROWDOT_CASES)
def test_rowdot(be, kind, I, M):
    """rowdot(T[:, :a], g, ...): ldy = M + 3 > M; with and without u_old."""
    rng = seed(kind, 3, I, M)
    Yw, q = SA.inputs(kind, rng, I, M + 3), SA.inputs(kind, rng, M)
    Y = Yw[:, :M]
    u_ref, mag, _ = SA.rowdot(Y, q)
    u_old = SA.away_from(kind, rng, u_ref)
    _, _, du2_ref = SA.rowdot(Y, q, u_old)
    Yd, qd, uod = dev(Yw)[:, :M], dev(q), dev(u_old)
    u = torch.full((I + 1,), SENTINEL, dtype=F64, device=DEV)
    assert be.rowdot(Yd, qd, u[:I], None) is None
    check("rowdot u", kind, host(u[:I]), u_ref, SA.bound_sum(M, mag))
    u2 = torch.full((I + 1,), SENTINEL, dtype=F64, device=DEV)
    du2 = be.rowdot(Yd, qd, u2[:I], uod, be.empty(1))
    assert same_bits(u, u2) and float(u[I]) == SENTINEL
    check("rowdot du2", kind, host(du2), [du2_ref], [SA.bound_du2(Y, q, u_old)])
    assert same_bits(du2, be.rowdot(Yd, qd, u2[:I], uod, be.empty(1))) and same_bits(u, u2)


# ---- y_deflate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("I,M,R,chain", SA.Y_DEFLATE_CASES)
def test_y_deflate(be, kind, I, M, R, chain):
    """ldy = M + 2 with the two columns past M left bit-identical, ldt = R + 3; Y in place and ssq."""
    rng = seed(kind, 4, I, M, R)
    Tw, b, q = SA.inputs(kind, rng, I, R + 3), SA.inputs(kind, rng, R), SA.inputs(kind, rng, M)
    s = Tw[:, :R].astype(LD) @ b.astype(LD)
    Yw = SA.inputs(kind, rng, I, M + 2)
    Yw[:, :M] = SA.away_from(kind, rng, np.outer(s, q.astype(LD)))
    V, ev, ssq_ref = SA.y_deflate(Yw[:, :M], Tw, R, b, q)
    Td, bd, qd = dev(Tw), dev(b), dev(q)
    Y1, Y2 = dev(Yw), dev(Yw)
    ssq = be.y_deflate(Y1[:, :M], Td, R, bd, qd)
    check("y_deflate Y", kind, host(Y1[:, :M]), V, ev)
    assert same_bits(Y1[:, M:], dev(Yw)[:, M:])
    check("y_deflate ssq", kind, host(ssq), [ssq_ref], [SA.bound_ssq(V, ev, chain)])
    assert same_bits(ssq, be.y_deflate(Y2[:, :M], Td, R, bd, qd)) and same_bits(Y1, Y2)


# ---- sum, normalize, scores_mean, axpy_scalar, colscale ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SA.SUM_N)
def test_total(be, kind, n):
    v = SA.inputs(kind, seed(kind, 5, n), n)
    want, mag = SA.total(v)
    vd = dev(v)
    got = be.total(vd)
    check("sum", kind, host(got), [want], [SA.bound_sum(n, mag)])
    assert same_bits(got, be.total(vd))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SA.NORMALIZE_N)
def test_normalize(be, kind, n):
    """The `nrm` output through be.lib, and a null `nrm` through the backend: same vector."""
    v = SA.inputs(kind, seed(kind, 6, n), n)
    if kind == "exact":
        v[0] = 3.0                                                       # never the zero vector
    v1, v2, nrm = dev(v), dev(v), torch.full((2,), SENTINEL, dtype=F64, device=DEV)
    assert be.lib.cmtfpls_normalize_f64(v1.data_ptr(), n, nrm.data_ptr(), be._stream()) == 0
    be.normalize(v2)
    assert same_bits(v1, v2) and float(nrm[1]) == SENTINEL
    if kind == "exact":
        want_v, want_n = SA.normalize_f64(v)
        assert np.array_equal(host(v1), want_v) and float(nrm[0]) == want_n
    else:
        want_v, want_n, rel_n, rel_v = SA.normalize(v)
        check("normalize nrm", kind, host(nrm[:1]), [want_n], [rel_n * float(want_n)])
        check("normalize v", kind, host(v1), want_v, rel_v * np.abs(want_v.astype(np.float64)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nb,I", SA.SCORES_MEAN_CASES)
def test_scores_mean(be, kind, nb, I):
    Ts = SA.inputs(kind, seed(kind, 7, nb, I), nb, I)
    Td = dev(Ts)
    got = be.scores_mean(Td, torch.full((I + 1,), SENTINEL, dtype=F64, device=DEV)[:I])
    if kind == "exact":
        assert np.array_equal(host(got), SA.scores_mean_f64(Ts))
    else:
        check("scores_mean", kind, host(got), SA.scores_mean(Ts)[0], SA.bound_scores_mean(Ts))
    assert same_bits(got, be.scores_mean(Td, be.empty(I)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_x", [True, False])
@pytest.mark.parametrize("n", SA.AXPY_N)
def test_axpy_scalar(be, kind, n, with_x):
    rng = seed(kind, 8, n, int(with_x))
    y, a, x = SA.inputs(kind, rng, n), SA.inputs(kind, rng, 1), (SA.inputs(kind, rng, n) if with_x else None)
    if kind == "exact":
        a[0] = 5.0
    want, mag = SA.axpy_scalar(y, a, x)
    buf = torch.full((n + 1,), SENTINEL, dtype=F64, device=DEV)
    buf[:n] = dev(y)
    ad, xd = dev(a), (dev(x) if with_x else None)
    be.axpy_scalar(buf[:n], ad, xd)
    check("axpy_scalar", kind, host(buf[:n]), want, SA.bound_sum(2, mag))
    assert float(buf[n]) == SENTINEL
    again = dev(y)
    assert same_bits(be.axpy_scalar(again, ad, xd), buf[:n])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", SA.COLSCALE_P)
def test_colscale(be, kind, P):
    """z / cnt * n in this order, both correctly rounded: equality on both input forms; a zero count gives 0."""
    rng = seed(kind, 9, P)
    Z = SA.inputs(kind, rng, P)
    cnt = rng.integers(0, 6, size=P).astype(np.float64)
    cnt[0] = 0.0 if P > 1 else 3.0
    cnt[-1] = 3.0
    buf = torch.full((P + 1,), SENTINEL, dtype=F64, device=DEV)
    buf[:P] = dev(Z)
    be.colscale(buf[:P], dev(cnt), 7.0)
    assert np.array_equal(host(buf[:P]), SA.colscale(Z, cnt, 7.0)) and float(buf[P]) == SENTINEL
    assert bool((buf[:P][dev(cnt) == 0] == 0).all())


# ---- kr_gram, kr_gram_row, khatri_rao, kron -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,R", SA.KR_GRAM_CASES)
def test_kr_gram(be, kind, n, R):
    """`first` with scale = 3 through be.lib, then a second mode (n + 2 rows) multiplied in with the backend's scale = 1."""
    rng = seed(kind, 10, n, R)
    L1, L2 = SA.inputs(kind, rng, n, R), SA.inputs(kind, rng, n + 2, R)
    L1d, L2d = dev(L1), dev(L2)
    G = torch.full((R * R + 1,), SENTINEL, dtype=F64, device=DEV)
    assert be.lib.cmtfpls_kr_gram_f64(L1d.data_ptr(), n, R, G.data_ptr(), 1, 3.0, be._stream()) == 0
    want1, bound1 = SA.kr_gram(L1, None, True, 3.0)
    check("kr_gram first", kind, host(G[:R * R]).reshape(R, R), want1, bound1)
    G1 = G.clone()
    be.kr_gram(L2d, G[:R * R].view(R, R), first=False)
    want1_64 = want1.astype(np.float64)
    want2, bound2 = SA.kr_gram(L2, want1_64, False, 1.0, G_err=bound1 + SA.U * np.abs(want1_64))
    check("kr_gram second mode", kind, host(G[:R * R]).reshape(R, R), want2, bound2)
    assert float(G[R * R]) == SENTINEL
    be.kr_gram(L2d, G1[:R * R].view(R, R), first=False)
    assert same_bits(G, G1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,R,a", SA.KR_GRAM_ROW_CASES)
def test_kr_gram_row(be, kind, n, R, a):
    """Row a of the Gram: `first`, then multiplied in; entries at and past a bit-identical (a = 0: all of g).  R = 301, a = 300:
    lanes 0 ... 43 take a second entry."""
    rng = seed(kind, 11, n, R, a)
    L1, L2, g0 = SA.inputs(kind, rng, n, R), SA.inputs(kind, rng, n, R), SA.inputs(kind, rng, R)
    L1d, L2d, g = dev(L1), dev(L2), dev(g0)
    be.kr_gram_row(L1d, a, g, True)
    assert same_bits(g[a:], dev(g0)[a:])
    if a:
        want, bound = SA.kr_gram_row(L1, a, g0, True)
        check("kr_gram_row", kind, host(g[:a]), want, bound)
    g1 = host(g).copy()
    be.kr_gram_row(L2d, a, g, False)
    assert same_bits(g[a:], dev(g0)[a:])
    if a:
        want, bound = SA.kr_gram_row(L2, a, g1, False)
        check("kr_gram_row", kind, host(g[:a]), want, bound)
    again = dev(g1)
    assert same_bits(be.kr_gram_row(L2d, a, again, False), g)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("na,nb", SA.KR_SIZES)
def test_khatri_rao_and_kron(be, kind, na, nb):
    """One product per output element: equality with NumPy on both input forms."""
    for R in SA.KR_R:
        rng = seed(kind, 12, na, nb, R)
        Am, Bm = SA.inputs(kind, rng, na, R), SA.inputs(kind, rng, nb, R)
        got = be.khatri_rao(dev(Am), dev(Bm))
        assert got.shape == (na * nb, R) and np.array_equal(host(got), SA.khatri_rao(Am, Bm))
    a, b = SA.inputs(kind, rng, na), SA.inputs(kind, rng, nb)
    out = torch.full((na * nb + 1,), SENTINEL, dtype=F64, device=DEV)
    be.kron(dev(a), dev(b), out[:na * nb])
    assert np.array_equal(host(out[:na * nb]), SA.kron(a, b)) and float(out[na * nb]) == SENTINEL


# ---- recon_r2 ----------------------------------------------------------------------------------------------------------------------
def _r2_call(be, Xd, T, WA, WB, mu, R):
    Td = dev(T)
    args = (Xd, Td[:, :R], dev(WA), dev(WB), None if mu is None else dev(mu))
    keep = bits(Xd)
    got = be.recon_r2(*args)
    assert got is not None and same_bits(got, be.recon_r2(*args))
    assert torch.equal(bits(Xd), keep)                                   # X is read only
    return host(got)


def _r2_case(be, kind, st, A, B, I, R, chain, mean, nan_fraction, misaligned=False):
    dtype, npd = (F32, np.float32) if st == "f32" else (F64, np.float64)
    rng = seed(kind, 13, A, B, I, R, int(misaligned))
    X, T, WA, WB, mu = SA.recon_r2_inputs(kind, rng, I, A, B, R, npd, mean, ldt_extra=2, nan_fraction=nan_fraction)
    if misaligned:                                                       # a view one element into its storage: the scalar form
        buf = torch.zeros(I * A * B + 1, dtype=dtype, device=DEV)
        buf[1:] = dev(X, dtype).reshape(-1)
        Xd = buf[1:].view(I, A * B)
        assert Xd.data_ptr() % 16 != 0
    else:
        Xd = dev(X, dtype)
    want, bound = SA.recon_r2(X, T[:, :R], WA, WB, mu, chain)
    got = _r2_call(be, Xd, T, WA, WB, mu, R)
    if kind == "exact":                                                  # T = 0: both sums are the integer sum of squares
        assert want[0] == want[1]
    check(f"recon_r2 {st}", kind, got, want, bound)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("st,A,B,I,chain", SA.RECON_R2_SHAPES + [("f64", 5, 131, 9, None), ("f32", 9, 133, 8, None)],
                         ids=lambda v: str(v))
def test_recon_r2_across_column_tiles(be, kind, st, A, B, I, chain):
    """Two and more column tiles of 256 lanes with a partly dead last tile (f64 V = 2: 650 -> 325 lanes, 1030 -> 515; f32 V = 4:
    1188 -> 297, 4160 -> 1040), the scalar form for B % V != 0 (655 and 1197 lanes), every R instance (RC = 4, 8, 12, 16 and the
    widths just past each), ldt = R + 2, no mean at R = 5, 10 % NaN at R = 8 and 13 (the last column of the last tile and of the
    last row among them)."""
    V = 4 if st == "f32" else 2
    assert SA.recon_r2_plan(I, A * B, V if B % V == 0 else 1)[0] >= 2
    for R in SA.RECON_R2_R:
        _r2_case(be, kind, st, A, B, I, R, chain, mean=(R != 5), nan_fraction=0.1 if R in (8, 13) else 0.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("st,A,B", [("f64", 5, 130), ("f32", 9, 132)])
def test_recon_r2_of_a_misaligned_view(be, kind, st, A, B):
    for R, nan in ((4, 0.0), (9, 0.1)):
        _r2_case(be, kind, st, A, B, 7, R, None, mean=True, nan_fraction=nan, misaligned=True)


@pytest.mark.parametrize("kind", KINDS)
def test_recon_r2_with_a_ragged_last_row_block(be, kind):
    """f64 5 x 130, I = 8300: 2 column tiles -> 1024 row blocks wanted -> 9 rows per block (more than the floor of 8), 923 row
    blocks, the last of 2 rows."""
    st, A, B, I, chain = SA.RECON_R2_RAGGED
    assert SA.recon_r2_plan(I, A * B, 2) == (2, 923, 9) and I - 922 * 9 == 2
    _r2_case(be, kind, st, A, B, I, 4, chain, mean=True, nan_fraction=0.1)


def test_recon_r2_declines_17_components_and_a_short_workspace(be):
    rng = seed("exact", 14)
    I, A, B = 9, 5, 130
    X, T, WA, WB, mu = SA.recon_r2_inputs("rounding", rng, I, A, B, 17, np.float64, True)
    Xd, Td, WAd, WBd = dev(X), dev(T), dev(WA), dev(WB)
    assert be.recon_r2(Xd, Td, WAd, WBd, dev(mu)) is None
    ct, rb, _ = SA.recon_r2_plan(I, A * B, 2)
    need = ct * rb * 2 * 8
    ws, out = torch.zeros(need, dtype=torch.uint8, device=DEV), torch.full((2,), SENTINEL, dtype=F64, device=DEV)
    WA16, WB16 = WAd[:, :16].contiguous(), WBd[:, :16].contiguous()

    def call(nbytes):
        return be.lib.cmtfpls_recon_r2_f64(Xd.data_ptr(), Td.data_ptr(), I, 17, 16, WA16.data_ptr(), WB16.data_ptr(), A, B, None,
                                           out.data_ptr(), ws.data_ptr(), nbytes, be._stream())
    assert call(need - 8) == 2 and b"recon_r2" in be.lib.cmtfpls_last_error()
    assert bool((out == SENTINEL).all())
    assert call(need) == 0


# ---- recon across column tiles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", [16, 17])
@pytest.mark.parametrize("st,A,B", [("f64", 5, 130), ("f64", 1, 1030), ("f32", 9, 132), ("f32", 8, 520)])
def test_recon_across_column_tiles(be, kind, st, A, B, R):
    """The multi-tile shapes of recon_r2 through recon (one pass, and a second accumulating pass for R = 17).  Rounding form: the
    inputs and the bound of test_recon_matches_float64 (passes x 2^-24 x 1.01 of |mean| + sum|t w| for f32, 1e-14 for f64).
    Exact form: integers (at most 17 x 512 + 8, exact in f32 too), equality."""
    dtype = F32 if st == "f32" else F64
    I, P = 9, A * B
    rng = seed(kind, 15, A, B, R)
    if kind == "exact":
        T, WA, WB, mu = (SA.exact_inputs(rng, *s) for s in ((I, R + 2), (A, R), (B, R), (P,)))
    else:
        T, WA, WB, mu = rng.normal(size=(I, R + 2)), rng.normal(size=(A, R)), rng.normal(size=(B, R)), rng.normal(size=P)
    buf = torch.full((I * P + 4,), -7.0, dtype=dtype, device=DEV)
    out = buf[:I * P]
    assert be.recon(dev(T)[:, :R], dev(WA), dev(WB), dev(mu), out) is not None
    want, mag = SA.recon(T[:, :R], WA, WB, mu)
    got = host(out).reshape(I, P)
    assert bool((buf[I * P:] == -7.0).all())
    if kind == "exact":
        assert np.array_equal(got, want)
        return
    passes = -(-R // 16)
    bound = passes * 2.0 ** -24 * 1.01 if dtype == F32 else 1e-14
    err = float((np.abs(got - want) / mag).max())
    _record(f"recon {st} (error / its bound)", err / bound)
    assert err <= bound, (err, bound)


# ---- statuses: the argument checks return before any launch ------------------------------------------------------------------------
def test_statuses(be):
    lib, st = be.lib, be._stream()
    z = torch.full((64,), SENTINEL, dtype=F64, device=DEV)
    p = z.data_ptr()
    nws = int(lib.cmtfpls_small_workspace_bytes())
    ws = torch.zeros(nws, dtype=torch.uint8, device=DEV).data_ptr()

    def named(rc, want, name):
        assert rc == want and name in lib.cmtfpls_last_error(), (rc, want, name, lib.cmtfpls_last_error())

    named(lib.cmtfpls_gram_tn_f64(p, 3, 4, p, 1, 1, 4, p, ws, nws, st), 1, b"gram_tn")          # lda < a
    named(lib.cmtfpls_gram_tn_f64(p, 4, 4, p, 1, 1, 0, p, ws, nws, st), 1, b"gram_tn")          # I = 0
    named(lib.cmtfpls_gram_tn_f64(None, 4, 4, p, 1, 1, 4, p, ws, nws, st), 1, b"gram_tn")       # null A
    named(lib.cmtfpls_gram_tn_f64(p, 4, 4, p, 1, 1, 4, p, ws, nws - 1, st), 2, b"gram_tn")      # short workspace
    named(lib.cmtfpls_rowdot_f64(p, 3, 4, 4, p, p, None, None, ws, nws, st), 1, b"rowdot")      # ldy < M
    named(lib.cmtfpls_rowdot_f64(p, 4, 4, 4, p, p + 256, p, None, ws, nws, st), 1, b"rowdot")   # u_old without du2: u untouched
    named(lib.cmtfpls_rowdot_f64(p, 4, 4, 4, p, p + 256, p, p, ws, 128 * 8 - 1, st), 2, b"rowdot")
    named(lib.cmtfpls_y_deflate_f64(p, 4, 4, 4, p, 1, 2, p, p, p, ws, nws, st), 1, b"y_deflate")  # ldt < R
    named(lib.cmtfpls_y_deflate_f64(p, 4, 4, 4, p, 2, 2, p, p, p, ws, 128 * 8 - 1, st), 2, b"y_deflate")
    named(lib.cmtfpls_sum_f64(p, 0, p, st), 1, b"sum")
    named(lib.cmtfpls_normalize_f64(None, 4, None, st), 1, b"normalize")
    named(lib.cmtfpls_scores_mean_f64(p, 0, 4, p, st), 1, b"scores_mean")
    named(lib.cmtfpls_axpy_scalar_f64(p, 4, None, None, st), 1, b"axpy_scalar")
    named(lib.cmtfpls_colscale_f64(p, 0, p, 2.0, st), 1, b"colscale")
    named(lib.cmtfpls_kr_gram_f64(p, 0, 2, p, 1, 1.0, st), 1, b"kr_gram")
    named(lib.cmtfpls_kr_gram_row_f64(p, 4, 2, 2, p, 1, st), 1, b"kr_gram_row")                 # a >= R
    named(lib.cmtfpls_khatri_rao_f64(p, 2, p, 2, 0, p, st), 1, b"khatri_rao")
    named(lib.cmtfpls_kron_f64(p, 2, None, 2, p, st), 1, b"kron")
    named(lib.cmtfpls_kr_axpy_f64(p, 2, 2, p, p, 65, 65, p, st), 4, b"kr_axpy")                 # more than 64 terms
    torch.cuda.synchronize()
    assert bool((z == SENTINEL).all())                                                         # nothing was launched
