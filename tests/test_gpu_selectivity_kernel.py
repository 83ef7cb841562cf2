"""The target-projection pass on the device (cmtfpls_selectivity_cols_*, csrc/selectivity.hip) against a float64 torch formula that
centres first: both storage types, the masked and the complete form, every branch of the tiling (scalar loads and a wave's tail,
one wave with the other three past the last column, a second workgroup with one live lane group, interior tiles; one row, row
blocks with a ragged tail; 1 / 2 / 4 response tiles, a ragged tile, the second pass over X), a row stride of Tau above M, a base
pointer one element into its storage, a row entirely NaN, a column with exactly one observed row, mean = NULL, bit-identical
repeats, X untouched, columns with a mean of 1e6 and unit spread, and the error codes that come before any launch.

Tolerances.  s and d are sums of non-negative terms: the project's rtol=1e-11, atol=1e-9 for such sums (test_gpu_contributions.py).
n is a count: exact.  a cancels, so it is held to the float64 accumulation bound: |got - want| <= 1e-11 |want| + (I + 2) 2^-53
sum_i |x tau|, the sum taken from the formula."""
import pytest
import torch

from cmtf_pls_amd.backend import HipBackend

pytestmark = pytest.mark.gpu


def _formula(X2, Tau, mean, masked):
    x = X2.double() if mean is None else X2.double() - mean
    o = torch.isfinite(x) if masked else torch.ones_like(x, dtype=torch.bool)
    x0 = torch.where(o, x, 0.0)
    of = o.double()
    a = Tau.T @ x0
    d = (Tau * Tau).T @ of if masked else None
    return a, d, (x0 * x0).sum(0), of.sum(0), Tau.abs().T @ x0.abs()


def _operands(I, P, M, dtype, seed, nan_frac=0.0, offset=0, mean_scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    mean = (mean_scale * torch.randn(P, generator=g, dtype=torch.float64))
    flat = torch.randn(I * P + offset, generator=g, dtype=torch.float64)
    flat[offset:] += mean.repeat(I)
    if nan_frac:
        flat[torch.rand(flat.shape, generator=g) < nan_frac] = float("nan")
    X2 = flat.to("cuda", dtype)[offset:].view(I, P)
    Tau = torch.randn(I, M + 3, generator=g, dtype=torch.float64).cuda()[:, :M]      # a row stride > M
    return X2, Tau, mean.cuda()


def _check(got, want, I, label):
    a, d, s, n = got
    wa, wd, ws, wn, absxt = want
    assert torch.equal(n, wn), label
    torch.testing.assert_close(s, ws, rtol=1e-11, atol=1e-9, equal_nan=True)
    if wd is None:
        assert d is None
    else:
        torch.testing.assert_close(d, wd, rtol=1e-11, atol=1e-9)
    bound = 1e-11 * wa.abs() + (I + 2) * 2.0 ** -53 * absxt
    err = (a - wa).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{label} a: worst |got - want| / bound = {worst:.3g}")
    assert bool((err <= bound).all()), (label, worst)


SHAPES = [
    (1, 3, 1, 0),          # one row, scalar loads, one response
    (63, 7, 16, 0),        # P % 4 != 0: scalar loads and a wave's tail; a row block short of 64 rows
    (64, 60, 17, 0),       # one wave, the other three past the last column; a ragged second response tile
    (65, 64, 64, 0),       # a whole wave; two row blocks, the second with one row; four response tiles (masked: two passes)
    (200, 60, 65, 0),      # four row blocks, the last with 8 rows; the second pass over X
    (200, 260, 16, 0),     # a second workgroup with one live lane group
    (65, 512, 16, 0),      # 256 x 2 columns, ragged rows
    (128, 512, 16, 0),     # interior tiles only: the form without clamps, one response tile
    (128, 512, 32, 0),     # ... two response tiles
    (64, 256, 64, 0),      # ... four response tiles (masked: two passes of two)
    (64, 256, 48, 0),      # three response tiles run as four with the last one masked off
    (65, 64, 16, 1),       # a view one element into its storage: misaligned base, scalar loads
    # the shapes of tests/test_gpu_workspace_contract.py: 9 row blocks with a short last one at P = 63 (scalar) and 240 (vector, also
    # misaligned); P = 1320: five column tiles and a partial one, 33 row blocks
    (517, 63, 1, 0), (517, 63, 17, 0), (517, 240, 1, 0), (517, 240, 17, 0), (517, 240, 1, 1), (517, 240, 17, 1),
    (2100, 1320, 1, 0), (2100, 1320, 17, 0),
]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("I,P,M,offset", SHAPES)
def test_kernel_against_formula(I, P, M, offset, dtype, masked):
    be = HipBackend()
    X2, Tau, mean = _operands(I, P, M, dtype, seed=I + P + M, nan_frac=0.1 if masked else 0.0, offset=offset)
    before = X2.clone()
    got = be.selectivity_cols(X2, Tau, mean, masked)
    _check(got, _formula(X2, Tau, mean, masked), I, f"{dtype} {(I, P, M, offset)} masked={masked}")
    again = be.selectivity_cols(X2, Tau, mean, masked)
    assert all((g is None and h is None) or torch.equal(g, h) for g, h in zip(got, again))      # deterministic: the same bits
    bits = torch.int32 if dtype == torch.float32 else torch.int64
    assert torch.equal(X2.view(bits), before.view(bits))                                       # read only


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nan_row_single_observation_and_no_mean(dtype):
    be = HipBackend()
    I, P, M = 70, 68, 5
    X2, Tau, mean = _operands(I, P, M, dtype, seed=7, nan_frac=0.05)
    X2[13] = float("nan")                                   # a row entirely NaN
    X2[:, 9] = float("nan")                                 # a column with exactly one observed row
    X2[41, 9] = 0.25
    X2[:, 30] = float("nan")                                # and one with none
    got = be.selectivity_cols(X2, Tau, mean, True)
    _check(got, _formula(X2, Tau, mean, True), I, f"{dtype} special rows and columns")
    a, d, s, n = got
    assert n[9].item() == 1.0 and n[30].item() == 0.0 and n.max().item() <= I - 1
    assert s[30].item() == 0.0 and not a[:, 30].any() and not d[:, 30].any()
    torch.testing.assert_close(d[:, 9], Tau[41] ** 2, rtol=1e-15, atol=0)
    for masked in (False, True):
        Xc = torch.nan_to_num(X2, nan=0.5)
        got = be.selectivity_cols(Xc, Tau, None, masked)    # mean = NULL: x = X
        _check(got, _formula(Xc, Tau, None, masked), I, f"{dtype} mean=NULL masked={masked}")


@pytest.mark.parametrize("masked", [False, True])
def test_large_column_means_keep_their_digits(masked):
    """Column means of 1e6 with unit spread, float64: centring in registers meets the same bounds (the route through
    sumsq - sum^2 / I loses 12 of its 16 digits here)."""
    be = HipBackend()
    I, P, M = 200, 132, 3
    g = torch.Generator(device="cpu").manual_seed(5)
    mean = 1e6 * (1.0 + torch.rand(P, generator=g, dtype=torch.float64))
    X = mean + torch.randn(I, P, generator=g, dtype=torch.float64)
    if masked:
        X[torch.rand(X.shape, generator=g) < 0.1] = float("nan")
    Tau = torch.randn(I, M, generator=g, dtype=torch.float64).cuda()
    X2, mean = X.cuda(), torch.nanmean(X, dim=0).cuda()
    got = be.selectivity_cols(X2, Tau, mean, masked)
    want = _formula(X2, Tau, mean, masked)
    assert 0.5 * I < want[2].min().item() and want[2].max().item() < 2.0 * I           # s is the spread, not the offset
    _check(got, want, I, f"means of 1e6 masked={masked}")


def test_error_codes_come_before_any_launch():
    be = HipBackend()
    lib = be.lib
    I, P, M = 64, 64, 4
    X2, Tau, mean = _operands(I, P, M, torch.float32, seed=1)
    Tau = Tau.contiguous()
    need = lib.cmtfpls_selectivity_cols_workspace_bytes(I, P, M)
    assert need > 0 and lib.cmtfpls_selectivity_cols_workspace_bytes(I, P, 0) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    a, d = torch.full((M, P), -7.0, dtype=torch.float64, device="cuda"), torch.full((M, P), -7.0, dtype=torch.float64, device="cuda")
    s, n = torch.full((P,), -7.0, dtype=torch.float64, device="cuda"), torch.full((P,), -7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(m, ws_bytes, dptr=d.data_ptr(), ld=M):
        return lib.cmtfpls_selectivity_cols_f32(X2.data_ptr(), I, P, Tau.data_ptr(), ld, m, mean.data_ptr(), 1, a.data_ptr(), dptr,
                                                s.data_ptr(), n.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    assert call(M, need - 1) == 2                            # CMTFPLS_EWORKSPACE
    assert call(0, need) == 1 and call(-3, need) == 1        # CMTFPLS_EINVAL
    assert call(M, need, dptr=None) == 1 and call(M, need, ld=M - 1) == 1
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in (a, d, s, n))                                  # nothing was launched
    assert call(M, need) == 0
    torch.cuda.synchronize()
    assert not bool((a == -7.0).any()) and bool((n == I).all())
