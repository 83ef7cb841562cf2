"""The 16-bit forms of the read-only diagnostics passes through HipBackend: cmtfpls_{resid_rows,recon_r2,contrib_rows,
selectivity_cols}_{bf16,f16} (csrc/resid.hip, recon.hip, contrib.hip, selectivity.hip).

The contract is that of the other 16-bit entries, and stronger: a thread owns 4 columns as one 8-byte load, which is the f32
entry's thread-to-column mapping, so every sum runs in the f32 entry's order and every output has the BITS of the _f32 entry on
the exact float32 upcast of the stored values.  The tests therefore compare integer views with torch.equal; the float64
references (resid_rows_ref.reference_ld, small_algebra_ref.recon_r2, contributions_ref, selectivity_ref.sums) are met once per
entry within the bounds those modules and their kernel tests already state -- no tolerance is introduced here.

Every case's data holds NaN (also with the sign bit and a payload), +-Inf, +-0 and subnormals of the 16-bit type, written as bit
patterns; the upcast is torch's (exact) conversion on the device.  After every call the 16-bit tensor has the same data_ptr and bits."""
import ctypes

import numpy as np
import pytest
import torch

import contributions_ref as CR
import matrix_core_ref as MC
import resid_rows_ref as RR
import selectivity_ref as SR
import small_algebra_ref as SA
from cmtf_pls_amd.backend import HipBackend

pytestmark = pytest.mark.gpu

KINDS = {"bf16": torch.bfloat16, "f16": torch.float16}
# quiet NaN, NaN with the sign bit and a payload, +Inf, -Inf, +0, -0, the smallest subnormal, a negative subnormal
SPECIAL_BITS = {"bf16": [0x7FC0, 0xFFC1, 0x7F80, 0xFF80, 0x0000, 0x8000, 0x0001, 0x8003],
                "f16": [0x7E00, 0xFE01, 0x7C00, 0xFC00, 0x0000, 0x8000, 0x0001, 0x8003]}


def _bits16(values):
    return torch.tensor(np.array(values, dtype=np.uint16).view(np.int16))


def _x16(kind, I, P, seed, offset=0, specials=True, nan_row=None, nan_col=None):
    """(X16 (I, P) on the device, a view `offset` elements into its buffer; its float32 upcast, a view `offset` elements into ITS
    buffer: both sides misaligned the same way).  Random values of unit scale with the special bit patterns strided over it."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    flat = torch.randn(I * P + offset, generator=g, dtype=torch.float32).to(KINDS[kind])
    raw = flat.view(torch.int16)
    if specials:
        spec = _bits16(SPECIAL_BITS[kind])
        n = I * P
        at = offset + (torch.arange(len(spec)) * max(1, (n - 1) // len(spec)) + min(3, n - 1)) % n
        raw[at] = spec
    x = flat[offset:].view(I, P)
    if nan_row is not None:
        x[nan_row] = float("nan")
    if nan_col is not None:
        x[:, nan_col] = float("nan")
    X16 = flat.cuda()[offset:].view(I, P)
    buf32 = torch.empty(I * P + offset, dtype=torch.float32, device="cuda")
    X32 = buf32[offset:].view(I, P)
    X32.copy_(X16)                                        # the exact upcast, made on the device
    assert X16.is_contiguous() and X32.is_contiguous()
    return X16, X32


def _ivw(t):
    return t.view(torch.int64)


def _same_bits(got, want, label):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (label, k)
        if g is not None:
            assert g.dtype == torch.float64 and torch.equal(_ivw(g), _ivw(w)), (label, k, int((_ivw(g) != _ivw(w)).sum()))


class _Untouched:
    """X16 has the same data_ptr and the same bits after the block."""

    def __init__(self, X16):
        self.X, self.ptr, self.bits = X16, X16.data_ptr(), X16.view(torch.int16).clone()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        assert self.X.data_ptr() == self.ptr and torch.equal(self.X.view(torch.int16), self.bits)
        return False


def _factors(I, A, B, R, seed, n=None):
    g = torch.Generator(device="cpu").manual_seed(seed + 1000)
    n = I if n is None else n
    T = (torch.randn(n, R + 3, generator=g, dtype=torch.float64) / (4 * R)).cuda()[:, :R]        # a row stride > R
    H = torch.randn(n, R, generator=g, dtype=torch.float64).cuda()
    WA = torch.randn(A, R, generator=g, dtype=torch.float64).cuda()
    WB = torch.randn(B, R, generator=g, dtype=torch.float64).cuda()
    mean = (0.25 * torch.randn(A * B, generator=g, dtype=torch.float64)).cuda()
    return T, H, WA, WB, mean


def _vector_path(X16, X32, B):
    """(16-bit side, float32 side): whether each takes the vector path (4 columns per thread) -- they must agree."""
    return (B % 4 == 0 and X16.data_ptr() % 8 == 0), (B % 4 == 0 and X32.data_ptr() % 16 == 0)


# (I, A, B, offset): one-element path with one partial wavefront; vector path, ragged rows; P = 1056 > 1024: two column tiles; a
# matrix block; P % 4 == 0 on a view one element into its buffer (2-byte aligned only): one-element path.  The plan gives every
# row block of these 8 rows (rows_per_block only exceeds 8 beyond 8 x 2048 rows), so the last shape, case "b" of
# resid_rows_ref.TALL_CASES (2.3 MB at 16 bits), is there for the second, ragged 64-row chunk: 70 rows per block.
RESID_SHAPES = [(37, 5, 6, 0), (70, 8, 8, 0), (9, 33, 32, 0), (12, 1, 257, 0), (70, 8, 8, 1), (143357, 2, 4, 0)]
RESID_PATH = [(False, 1, 8), (True, 1, 8), (True, 2, 8), (False, 2, 8), (False, 1, 8), (True, 1, 70)]        # (vector, col_tiles, rows per block)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape,path", list(zip(RESID_SHAPES, RESID_PATH)), ids=lambda v: str(v).replace(" ", ""))
def test_resid_rows_and_recon_r2_have_the_bits_of_f32_on_the_upcast(kind, shape, path):
    be = HipBackend()
    I, A, B, offset = shape
    X16, X32 = _x16(kind, I, A * B, seed=I + A + B, offset=offset)
    v16, v32 = _vector_path(X16, X32, B)
    assert v16 == v32 == path[0], (X16.data_ptr() % 16, X32.data_ptr() % 16)
    V = 4 if v16 else 1
    ct, _, rpb, _ = RR.resid_plan(I, A * B, V)
    assert (ct, rpb) == path[1:] and SA.recon_r2_plan(I, A * B, V)[::2] == path[1:]
    assert be.lib.cmtfpls_resid_rows_workspace_bytes(I, A * B) >= RR.resid_workspace_bytes(I, A * B, V)
    for R in (3, 5, 12, 16):                                  # the four register-chunk instances
        T, _, WA, WB, mean = _factors(I, A, B, R, seed=R)
        with _Untouched(X16):
            got = be.resid_rows(X16, T, WA, WB, mean, True)
            r2 = be.recon_r2(X16, T, WA, WB, mean)
        want = be.resid_rows(X32, T, WA, WB, mean, True)
        _same_bits(got, want, f"resid_rows {kind} {shape} R={R}")
        _same_bits([r2], [be.recon_r2(X32, T, WA, WB, mean)], f"recon_r2 {kind} {shape} R={R}")
        up = X32.double() - mean
        assert np.array_equal(got[0][:, 2].cpu().numpy(), np.isfinite(up.cpu().numpy()).sum(axis=1).astype(np.float64))
    T, _, WA, WB, mean = _factors(I, A, B, 5, seed=77)
    with _Untouched(X16):
        _same_bits(be.resid_rows(X16, T, WA, WB, None, True), be.resid_rows(X32, T, WA, WB, None, True), f"{kind} {shape} mean=None")
        _same_bits([be.recon_r2(X16, T, WA, WB, None)], [be.recon_r2(X32, T, WA, WB, None)], f"{kind} {shape} recon_r2 mean=None")
        rows, cols = be.resid_rows(X16, T, WA, WB, mean, False)
    assert cols is None
    _same_bits([rows], [be.resid_rows(X32, T, WA, WB, mean, False)[0]], f"{kind} {shape} want_cols=False")


# (I rows of X, A, B, R, n outputs, row list?): a row subset with indices out of range; a matrix block; B = 260: two k-chunks at
# V = 4 (64 lanes x 4 columns = 256 per chunk, the smallest B % 4 == 0 beyond it); n = 2049 -> 2 rows per workgroup, a last group of one
CONTRIB_CASES = [(50, 6, 20, 10, 23, True), (64, 1, 260, 5, 64, False), (21, 3, 260, 12, 21, False), (40, 4, 8, 16, 2049, True),
                 (33, 5, 7, 3, 33, False)]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("case", CONTRIB_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_contrib_rows_has_the_bits_of_f32_on_the_upcast(kind, case):
    be = HipBackend()
    I, A, B, R, n, listed = case
    X16, X32 = _x16(kind, I, A * B, seed=I + B + R)
    T, H, WA, WB, mean = _factors(I, A, B, R, seed=n, n=n)
    assert mean.data_ptr() % 16 == 0
    rows = None
    if listed:
        rows = torch.randint(0, I, (n,), generator=torch.Generator().manual_seed(7))
        if n == 23:
            rows[[0, 11, n - 1]] = torch.tensor([-1, I, I + 7])
        rows = rows.cuda()
    if A > 1 and B % 4 == 0:
        G, lg, _, fits = RR.contrib_plan(n, R, A, B, 4)               # the plan of the f32 call: V = 4 for 16 bits too
        assert fits and (n != 2049 or (G == 2 and n % G == 1))        # a last group of one row
        assert B != 260 or ((1 << lg) * 4 == 256 and RR.contrib_plan(n, R, A, 256, 4)[1] == lg)      # 260: the first B of two k-chunks
    with _Untouched(X16):
        got = be.contrib_rows(X16, T, H, WA, WB, mean, rows)
    want = be.contrib_rows(X32, T, H, WA, WB, mean, rows)
    _same_bits(got, want, f"contrib_rows {kind} {case}")
    if n == 23:
        bad = [0, 11, n - 1]
        assert all(bool(torch.isnan(g[bad]).all()) for g in got)      # NaN outputs, nothing read out of bounds
    if A == 1:
        assert got[0] is None and got[2] is None
    with _Untouched(X16):
        _same_bits(be.contrib_rows(X16, T, H, WA, WB, None, rows), be.contrib_rows(X32, T, H, WA, WB, None, rows), f"{kind} {case} mean=None")


def _fast(I, P, M):
    _, rpb, _ = MC.plan_xcov(I, P)
    return P % 4 == 0 and P % 256 == 0 and M % 16 == 0 and M // 16 != 3 and I % rpb == 0 and rpb % 32 == 0


# (I, P, M, masked): complete M 1 / 17 / 33 / 70 (1, 2, 4 response tiles and a second pass), masked 1 / 17 / 33 (the second pass at
# 32); P = 30 (one-element loads), 64, 260 (a second workgroup); the smallest (I, 256, 16) that meets FAST, both forms
SEL_CASES = [(65, 30, 1, False), (65, 64, 17, False), (70, 260, 33, False), (65, 64, 70, False),
             (65, 30, 1, True), (70, 260, 17, True), (65, 64, 33, True), (64, 256, 16, False), (64, 256, 16, True), (65, 64, 16, False, 1)]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("case", SEL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_selectivity_cols_has_the_bits_of_f32_on_the_upcast(kind, case):
    be = HipBackend()
    I, P, M, masked = case[:4]
    offset = case[4] if len(case) > 4 else 0
    assert _fast(I, P, M) == ((I, P, M) == (64, 256, 16)) and not _fast(32, 256, 16)      # 64 rows: the smallest whole row block
    X16, X32 = _x16(kind, I, P, seed=I + P + M, offset=offset)
    assert (P % 4 == 0 and X16.data_ptr() % 8 == 0) == (P % 4 == 0 and X32.data_ptr() % 16 == 0) == (P % 4 == 0 and offset == 0)
    g = torch.Generator(device="cpu").manual_seed(M)
    Tau = torch.randn(I, M + 3, generator=g, dtype=torch.float64).cuda()[:, :M]
    mean = (0.25 * torch.randn(P, generator=g, dtype=torch.float64)).cuda()
    for mu in (mean, None):
        with _Untouched(X16):
            got = be.selectivity_cols(X16, Tau, mu, masked)
        _same_bits(got, be.selectivity_cols(X32, Tau, mu, masked), f"selectivity_cols {kind} {case} mean={'yes' if mu is not None else 'None'}")
        if masked:
            up = X32.double().cpu().numpy() - (0.0 if mu is None else mu.cpu().numpy())
            assert np.array_equal(got[3].cpu().numpy(), np.isfinite(up).sum(axis=0).astype(np.float64))
        else:
            assert bool((got[3] == float(I)).all())


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_row_and_a_column_entirely_nan(kind):
    """Row 3 and column 5 hold only NaN: their counts are 0, their sums 0, and every entry has the f32 entry's bits."""
    be = HipBackend()
    I, A, B, R, M = 70, 8, 8, 5, 3
    X16, X32 = _x16(kind, I, A * B, seed=5, nan_row=3, nan_col=5)
    T, H, WA, WB, mean = _factors(I, A, B, R, seed=9)
    Tau = T[:, :M].contiguous()
    fin = np.isfinite(X32.double().cpu().numpy() - mean.cpu().numpy())
    assert not fin[3].any() and not fin[:, 5].any() and fin.sum() < (I - 1) * (A * B - 1)          # the specials are skipped too
    with _Untouched(X16):
        rows, cols = be.resid_rows(X16, T, WA, WB, mean, True)
        r2 = be.recon_r2(X16, T, WA, WB, mean)
        con = be.contrib_rows(X16, T, H, WA, WB, mean)
        a, d, s, n = be.selectivity_cols(X16, Tau, mean, True)
    _same_bits((rows, cols), be.resid_rows(X32, T, WA, WB, mean, True), kind)
    _same_bits([r2], [be.recon_r2(X32, T, WA, WB, mean)], kind)
    _same_bits(con, be.contrib_rows(X32, T, H, WA, WB, mean), kind)
    _same_bits((a, d, s, n), be.selectivity_cols(X32, Tau, mean, True), kind)
    assert np.array_equal(rows[:, 2].cpu().numpy(), fin.sum(axis=1).astype(np.float64)) and float(rows[3, 2]) == 0.0
    assert np.array_equal(n.cpu().numpy(), fin.sum(axis=0).astype(np.float64)) and float(n[5]) == 0.0
    assert rows[3].tolist() == [0.0, 0.0, 0.0] and cols[5].tolist() == [0.0, 0.0]
    assert float(s[5]) == 0.0 and bool((a[:, 5] == 0).all()) and bool((d[:, 5] == 0).all())
    assert all(bool((c[3] == 0).all()) for c in con)


@pytest.mark.parametrize("kind", list(KINDS))
def test_against_the_float64_references(kind):
    """One case per entry against the float64 reference of that kernel on the upcast values, within that reference's own bound:
    resid_rows_ref.reference_ld (np.longdouble, its derived bounds), small_algebra_ref.recon_r2 (value, bound),
    contributions_ref.contributions / check at the float64 estimator tolerance of test_gpu_contributions.py (1e-9), and
    selectivity_ref.sums at the kernel tolerances of test_gpu_selectivity_kernel.py."""
    be = HipBackend()
    I, A, B, R, M = 70, 8, 8, 5, 3
    P = A * B
    X16, X32 = _x16(kind, I, P, seed=21)
    T, H, WA, WB, mean = _factors(I, A, B, R, seed=22)
    T = T.contiguous()
    up = X32.double().cpu().numpy()
    Tn, WAn, WBn, mu = (t.cpu().numpy() for t in (T, WA, WB, mean))
    # resid_rows
    rows, cols = be.resid_rows(X16, T, WA, WB, mean, True)
    wr, wc, br, bc = RR.reference_ld(up, Tn, WAn, WBn, mu)
    er = np.abs(rows.cpu().numpy()[:, :2].astype(RR.LD) - wr[:, :2]).astype(np.float64)
    ec = np.abs(cols.cpu().numpy().astype(RR.LD) - wc).astype(np.float64)
    print(f"{kind} resid_rows: worst err / bound rows {np.max(er / np.maximum(br, 1e-300)):.3g} cols {np.max(ec / np.maximum(bc, 1e-300)):.3g}")
    assert (er <= br).all() and (ec <= bc).all()
    assert np.array_equal(rows.cpu().numpy()[:, 2], wr[:, 2].astype(np.float64))
    # recon_r2
    val, bound = SA.recon_r2(up, Tn, WAn, WBn, mu)
    e2 = np.abs(be.recon_r2(X16, T, WA, WB, mean).cpu().numpy().astype(RR.LD) - val).astype(np.float64)
    print(f"{kind} recon_r2: err / bound {e2 / np.asarray(bound, dtype=np.float64)}")
    assert (e2 <= np.asarray(bound, dtype=np.float64)).all()
    # contrib_rows through the restatement of the routine: a stand-in model of one block whose fitted scores are T
    class Model:
        X_factors = [Tn, WAn, WBn]
        X_mean = mu.reshape(A, B)
    sel = np.array([0, 7, 33, 69])
    want = CR.contributions(Model, train=up.reshape(I, A, B), rows=sel)
    tbar = Tn.mean(axis=0)
    S_pinv = np.linalg.pinv((Tn - tbar).T @ (Tn - tbar) / (I - 1))
    gd = (Tn[sel] - tbar) @ S_pinv
    W = (WAn[:, None, :] * WBn[None, :, :]).reshape(P, R)
    h = np.linalg.solve(np.eye(R) + np.triu(W.T @ W, 1), gd.T).T
    ridx = torch.from_numpy(sel).cuda()
    speA, speB, t2A, t2B = be.contrib_rows(X16, T[ridx].contiguous(), torch.from_numpy(h).cuda().contiguous(), WA, WB, mean, ridx)
    got = {"rows": sel, "scores": Tn[sel], "t2": want["t2"], "t2_closure": want["t2_closure"], "spe": speB.sum(dim=1).cpu().numpy(),
           "spe_mode": [speA.cpu().numpy(), speB.cpu().numpy()], "t2_mode": [t2A.cpu().numpy(), t2B.cpu().numpy()]}
    CR.check(got, want, False, 1e-9)
    # selectivity_cols, masked
    Tau = T[:, :M].contiguous()
    a, d, s, n = be.selectivity_cols(X16, Tau, mean, True)
    wa, wd, ws, wn, absxt = (torch.from_numpy(v).cuda() for v in SR.sums(up, mu, Tau.cpu().numpy()))
    assert torch.equal(n, wn)
    torch.testing.assert_close(s, ws, rtol=1e-11, atol=1e-9)
    torch.testing.assert_close(d, wd, rtol=1e-11, atol=1e-9)
    assert bool(((a - wa).abs() <= 1e-11 * wa.abs() + (I + 2) * 2.0 ** -53 * absxt).all())


@pytest.mark.parametrize("kind", list(KINDS))
def test_more_than_16_components_decline_as_f32_and_write_nothing(kind):
    """R = 17: the backend answers None as for float32, and the entries themselves return the _f32 status (4) with every
    sentinel-filled output untouched."""
    be = HipBackend()
    I, A, B, R = 40, 4, 8, 17
    P = A * B
    X16, X32 = _x16(kind, I, P, seed=17)
    T, H, WA, WB, mean = _factors(I, A, B, R, seed=18)
    T = T.contiguous()
    with _Untouched(X16):
        assert be.resid_rows(X16, T, WA, WB, mean, True) is None and be.resid_rows(X32, T, WA, WB, mean, True) is None
        assert be.recon_r2(X16, T, WA, WB, mean) is None and be.recon_r2(X32, T, WA, WB, mean) is None
        assert be.contrib_rows(X16, T, H, WA, WB, mean) is None and be.contrib_rows(X32, T, H, WA, WB, mean) is None
    lib, st = be.lib, torch.cuda.current_stream().cuda_stream
    ws = torch.empty(max(lib.cmtfpls_resid_rows_workspace_bytes(I, P), lib.cmtfpls_recon_r2_workspace_bytes(I, P), 256), dtype=torch.uint8,
                     device="cuda")
    sentinel = -12345.0
    outs = [torch.full(shape, sentinel, dtype=torch.float64, device="cuda") for shape in ((I, 3), (P, 2), (2,), (I, A), (I, B), (I, A), (I, B))]
    rows, cols, r2, speA, speB, t2A, t2B = outs
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    for X, sfx in ((X16, kind), (X32, "f32")):
        with _Untouched(X16):
            rc = [getattr(lib, f"cmtfpls_resid_rows_{sfx}")(p(X), p(T), I, T.stride(0), R, p(WA), p(WB), A, B, p(mean), p(rows), p(cols), p(ws),
                                                          ws.numel(), st),
                  getattr(lib, f"cmtfpls_recon_r2_{sfx}")(p(X), p(T), I, T.stride(0), R, p(WA), p(WB), A, B, p(mean), p(r2), p(ws), ws.numel(), st),
                  getattr(lib, f"cmtfpls_contrib_rows_{sfx}")(p(X), I, p(T), T.stride(0), p(H), H.stride(0), R, p(WA), p(WB), A, B, p(mean), None,
                                                            I, p(speA), p(speB), p(t2A), p(t2B), st)]
        assert rc == [4, 4, 4], (sfx, rc)
    torch.cuda.synchronize()
    assert all(bool((t == sentinel).all()) for t in outs)
