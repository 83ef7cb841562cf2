"""The two matrix-core contractions past one grid round and in their guard-free (FAST) form, every reachable template instance
against torch float64 on the same device operands:

  S = Y^T X_(0)            be.xcov / be.xcov_ssq / be.xcov(mixed=True)      csrc/xcov.hip, csrc/mixed.hip
  M = X_(0) (WA (.) WB)    be.mttkrp / be.mttkrp(mixed=True)                csrc/mttkrp.hip, csrc/mixed.hip

tests/matrix_core_ref.py mirrors the host dispatch (run_mttkrp, cmtfpls_mttkrp_f32_mixed, plan_xcov and the `fast` predicates);
every case names the instance it selects and asserts that the mirror says so, that the grid really turns over where the case is
about a second round, and -- where the library can be asked -- that the library agrees (declines, workspace bytes).

csrc/mttkrp.hip
  covered here   mttkrp_kj4_kernel<float, 2, 1|2|3>, <float, 1, 1|2|3>; mttkrp_kj_kernel<float, 2> (one chunk; two passes of two
                 chunks), <float, 1>, <double, 4>, <double, 2>; mttkrp_jk_kernel<T, 4, 1, true> and <T, 4, 1, false> (npj = 3) for
                 both storage types -- each at I = 8193 and 16421, where a wavefront takes a second and a third sample;
                 mttkrp_kernel<T, false, 1|2, false, 256>, <T, true, 1, false, 256>, <T, true, 1, true, 256> at I > 131072.
  elsewhere      the same per-sample instances within one grid round (I <= 300): test_gpu_kernels.py::
                 test_mttkrp_mfma; mttkrp_kernel with 512 / 1024 threads and RT = 2 with vector loads: test_mttkrp_mfma
                 ((16, 256, 256), (48, 16, 16)) and test_gpu_stress_shapes.py.
  unreachable    mttkrp_kj4_kernel<T, NL, 4>: KJ4N takes NG = 4 for R > 12, the 4x4x4 form is entered for R <= 12 only
                 (CMTFPLS_MTTKRP_KJ4_MAXR); kj4 with T = double (V == 4 is required).  mttkrp_jk_kernel<T, 8, 1, true>,
                 <T, 8, 2, true> and <T, 8, 1, false>: they need 128 / 256.. f32 or 64 / 128.. f64 columns with A % 16 == 0, and
                 every such shape satisfies `wide` or `half` of the k-row forms, which are tried first.  (All stay instantiated;
                 builds with CMTFPLS_MTTKRP_NO_KJ reach them.)  f64 (8, 128) is no per-sample shape (A % 16 != 0): tile form.
csrc/xcov.hip
  covered here   xcov_kernel<T, MASKED, true, 1|2|4, true>, <T, MASKED, true, 4, false> on an otherwise-FAST shape (M = 48),
                 <T, MASKED, false, 1, false> from a base that is not a whole vector, ldy > M with a second response tile through
                 Y + 64, two row blocks; the SSQ instances <T, false, true, 1|2|4, FAST, true> through be.xcov_ssq.
  elsewhere      guarded instances at ragged shapes: test_gpu_kernels.py::test_xcov_mfma, test_gpu_stress_shapes.py;
                 rows_per_block = 256 FAST MT = 1 with SSQ: test_gpu_round3.py::test_xcov_ssq_kernel_gives_s_and_the_centred_norm_
                 from_one_read; xcov_deflate_kernel: test_gpu_round3.py::test_xcov_deflate_kernel_equals_deflating_then_building_s;
                 the STATS instances: test_gpu_round4.py::test_xcov_stats_kernel_gives_s_and_the_column_statistics_from_one_read.
csrc/mixed.hip
  covered here   xcov_mixed_kernel<MASKED, true, 1|2|4, true>, <MASKED, true, 4, false> (M = 48), <MASKED, false, 1, false>, and
                 rows_per_block = 128 (four trips, an f32 chain flushed in the middle of a block); mttkrp_kj_mixed_kernel<2> with an
                 odd chunk count 3 and with 17 chunks (two f32 chains per pass), <1>; mttkrp_mixed_kernel<false, 2>, <true, 2> past
                 one grid round, <true, 1> at lds_kj = 64 KB + 1 KB, <false, 1> at the 96 KB limit; the R > 32 and LDS declines.
  elsewhere      guarded xcov_mixed instances, kj_mixed within one round: test_gpu_mixed.py.

The 96 KB limit of cmtfpls_mttkrp_f32_mixed is (A + B) 128 B <= 98 304 B at R <= 16: A + B = 768.  (1, 767) is the last shape that
runs; (1, 768) needs 98 432 B and (1, 769) 98 560 B, both declined.

Bounds: matrix_core_ref (f64 kernels (n + 4) 2^-53 sum|terms|; mixed kernels the stated contract 2e-6 sum|terms|)."""
import pytest
import torch

import matrix_core_ref as MC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
TDT = {"f32": F32, "f64": F64, "mixed": F32}
SENTINEL = -7.25e300
PREFIX = 4099                    # samples of the short run: a ragged last workgroup, every wavefront one sample


@pytest.fixture(scope="module")
def be():
    from cmtf_pls_amd.backend import HipBackend
    return HipBackend(torch.device(DEV))


_worst = {}
_held = {}                       # the operands and reference of the case in hand (one at a time)


@pytest.fixture(scope="module", autouse=True)
def _report_and_release():
    yield
    for k, e in sorted(_worst.items()):
        print(f"worst error / bound {k}: {e:.3g}")
    _held.clear()
    torch.cuda.empty_cache()


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int64)


def _ratio(kind, got, want, mag, coeff):
    """Worst |got - want| / (coeff sum|terms|); NaN (a NaN in got) fails every comparison."""
    r = ((got - want).abs() / (coeff * mag)).max().item()
    _worst[kind] = max(_worst.get(kind, 0.0), r) if r == r else float("nan")
    return r


# ---- A. M = X_(0) (WA (.) WB) ---------------------------------------------------------------------------------------------------
def _mttkrp_operands(storage, A, B, R, I):
    """X (I, A B) of the storage type (f32 values are exactly f32: drawn in f32), the loadings, and the float64 reference
    want = X W, mag = |X| |W| with W[c, r] = WA[c // B, r] WB[c % B, r], computed once for the longest run of the case in row
    chunks of <= 64 MB (rows are independent: a shorter run's reference is a prefix)."""
    key = (storage, A, B, R)
    if key not in _held or _held[key][0].shape[0] < I:
        _held.clear()
        g = _gen(1000 * A + B + R)
        P = A * B
        X = torch.randn(I, P, generator=g, device=DEV, dtype=TDT[storage])
        WA = torch.randn(A, R, generator=g, device=DEV, dtype=F64) + 0.25
        WB = torch.randn(B, R, generator=g, device=DEV, dtype=F64) - 0.125
        W = (WA[:, None, :] * WB[None, :, :]).reshape(P, R)
        Wabs = W.abs()
        want, mag = torch.empty(I, R, dtype=F64, device=DEV), torch.empty(I, R, dtype=F64, device=DEV)
        step = max(1, (8 << 20) // P)
        for lo in range(0, I, step):
            xd = X[lo:lo + step].double()
            want[lo:lo + step] = xd @ W
            mag[lo:lo + step] = xd.abs() @ Wabs               # (not in place: for f64 storage xd IS X)
        _held[key] = (X, WA, WB, want, mag)
    X, WA, WB, want, mag = _held[key]
    return X[:I], WA, WB, want[:I], mag[:I]


def _run_mttkrp(be, X, A, B, WA, WB, mixed):
    """Into a column view of a wider buffer (ldo = R + 3); the columns outside the view must keep the sentinel."""
    I, R = X.shape[0], WA.shape[1]
    wide = torch.full((I, R + 3), SENTINEL, dtype=F64, device=DEV)
    out = wide[:, 2:2 + R]
    assert out.stride(0) == R + 3
    got = be.mttkrp(X, A, B, WA, WB, out, mixed=mixed)
    if got is None:
        return None
    assert bool((wide[:, :2] == SENTINEL).all()) and bool((wide[:, 2 + R:] == SENTINEL).all())
    return out


def _check_mttkrp(be, storage, A, B, R, I, inst, per_sample):
    mixed = storage == "mixed"
    X, WA, WB, want, mag = _mttkrp_operands(storage, A, B, R, I)
    keep = X.clone() if X.numel() <= (1 << 24) else None
    out = _run_mttkrp(be, X, A, B, WA, WB, mixed)
    assert out is not None
    coeff = MC.MIXED_RTOL if mixed else MC.f64_bound(A * B)
    r = _ratio(f"mttkrp {storage} {inst[0]}", out, want, mag, coeff)
    print(f"mttkrp {storage} {(I, A, B)} R={R} {inst}: error / bound {r:.3g}")
    assert r <= 1.0, (inst, I, r)
    again = _run_mttkrp(be, X, A, B, WA, WB, mixed)
    assert torch.equal(_bits(again), _bits(out))
    if keep is not None:
        assert torch.equal(_bits(X), _bits(keep))
    if per_sample:
        # a wavefront owns whole samples and the instance does not depend on I: a short run gives the same bits
        short = _run_mttkrp(be, X[:PREFIX], A, B, WA, WB, mixed)
        assert torch.equal(_bits(short), _bits(out[:PREFIX]))


def _instance(storage, I, A, B, R):
    return MC.mttkrp_mixed_instance(I, A, B, R) if storage == "mixed" else MC.mttkrp_instance(storage, I, A, B, R)


_SAMPLE_PARAMS = [pytest.param(st, ab, R, inst, I, id=f"{st}-{ab[0]}x{ab[1]}-R{R}-{'_'.join(map(str, inst))}-I{I}")
                  for st, ab, R, inst, Is in MC.SAMPLE_CASES for I in sorted(Is, reverse=True)]   # the longer run first: its operands serve both


@pytest.mark.parametrize("storage,ab,R,inst,I", _SAMPLE_PARAMS)
def test_mttkrp_per_sample_forms_past_one_grid_round(be, storage, ab, R, inst, I):
    """I = 8193: exactly one wavefront takes a second sample (its carried prefetch is the first chunk of sample 8192; for every
    other wavefront xs_next is its own sample).  I = 16421 = 2 x 8192 + 37: two full rounds and a ragged third."""
    A, B = ab
    assert _instance(storage, I, A, B, R) == inst and _instance(storage, PREFIX, A, B, R) == inst
    assert MC.mttkrp_rounds(inst, I) == -(-I // 8192) >= 2 and MC.mttkrp_rounds(inst, PREFIX) == 1
    _check_mttkrp(be, storage, A, B, R, I, inst, per_sample=True)


def test_mttkrp_f64_8x128_takes_the_tile_form(be):
    """A % 16 != 0 bars every per-sample form: f64 (8, 128) is mttkrp_kernel<double, true, 1, false, 256>, one grid round."""
    st, (A, B), R, inst, (I,) = MC.NOT_PER_SAMPLE
    assert MC.mttkrp_instance(st, I, A, B, R) == inst and MC.mttkrp_rounds(inst, I) == 1
    _check_mttkrp(be, st, A, B, R, I, inst, per_sample=False)


_TILE_PARAMS = [pytest.param(st, ab, R, by_i[I], I, id=f"{st}-{ab[0]}x{ab[1]}-R{R}-{'_'.join(map(str, by_i[I]))}-I{I}")
                for st, ab, R, by_i in MC.TILE_CASES for I in sorted(by_i, reverse=True)]


@pytest.mark.parametrize("storage,ab,R,inst,I", _TILE_PARAMS)
def test_mttkrp_tile_forms_past_one_grid_round(be, storage, ab, R, inst, I):
    """More than 8192 groups of 16 rows: `grp += gridDim.x * NW` runs.  I = 131125: 8196 groups, the last of 5 rows (guarded);
    I = 135168: 8448 whole groups (FAST for vector loads and P % 64 == 0)."""
    A, B = ab
    assert _instance(storage, I, A, B, R) == inst
    assert MC.mttkrp_rounds(inst, I) == 2
    _check_mttkrp(be, storage, A, B, R, I, inst, per_sample=False)


@pytest.mark.parametrize("ab,R,inst", [
    ((16, 16), 33, None),                              # more than 32 components
    ((1, 769), 16, None),                              # 770 x 128 B = 98 560 B > 96 KB
    ((1, 768), 16, None),                              # 769 x 128 B = 98 432 B > 96 KB
    ((1, 767), 16, ("tile_mixed", False, 1)),          # 98 304 B = 96 KB exactly: runs
    ((256, 384), 16, ("kj_mixed", 2)),                 # lds_kj = 384 x 128 + 256 x 64 = 65 536 B exactly: still the k-row form
    ((272, 384), 16, ("tile_mixed", True, 1)),         # lds_kj = 66 560 B: the tile form, 83 968 B of loadings
], ids=lambda v: str(v).replace(" ", ""))
def test_mttkrp_mixed_declines_and_lds_edges(be, ab, R, inst):
    A, B = ab
    I = 40
    assert MC.mttkrp_mixed_instance(I, A, B, R) == inst
    X, WA, WB, want, mag = _mttkrp_operands("mixed", A, B, R, I)
    out = _run_mttkrp(be, X, A, B, WA, WB, True)
    if inst is None:
        assert out is None
        return
    assert out is not None
    r = _ratio(f"mttkrp mixed {inst[0]}", out, want, mag, MC.MIXED_RTOL)
    print(f"mttkrp mixed {(I, A, B)} R={R} {inst}: error / bound {r:.3g}")
    assert r <= 1.0, (inst, r)
    assert torch.equal(_bits(_run_mttkrp(be, X, A, B, WA, WB, True)), _bits(out))


# ---- B. S = Y^T X_(0) -------------------------------------------------------------------------------------------------------------
def _xcov_operands(path, I, P, M, masked, name):
    """X in the storage type (the misaligned case: the same values one f32 / two f64 elements into their storage), Y (M = 80: a
    column view with ldy = 86), and the float64 reference S = Y^T nan_to_num(X), mag = |Y|^T |nan_to_num(X)|."""
    _held.clear()
    dtype = F64 if path == "f64" else F32
    g = _gen(7 * I + P + M)
    X = torch.randn(I, P, generator=g, device=DEV, dtype=dtype) + 0.5
    if masked:
        X[torch.rand(I, P, generator=g, device=DEV) < 0.2] = float("nan")
    if "misaligned" in name:
        off = 1 if dtype == F32 else 2
        buf = torch.zeros(I * P + off, dtype=dtype, device=DEV)
        buf[off:].view(I, P).copy_(X)
        X = buf[off:].view(I, P)
        assert X.data_ptr() % (4 * X.element_size()) != 0 and X.is_contiguous()
    if M == 80:
        wide = torch.randn(I, 86, generator=g, device=DEV, dtype=F64)
        Y = wide[:, 3:83]
        assert Y.stride(0) == 86
    else:
        Y = torch.randn(I, M, generator=g, device=DEV, dtype=F64)
    x0 = torch.nan_to_num(X.double(), nan=0.0)
    want = Y.T @ x0
    mag = Y.abs().T @ x0.abs()
    return X, Y, want, mag


def _check_xcov(be, path, name, shape, plan, insts, masked):
    I, P, M = shape
    mixed = path == "mixed"
    storage = "f64" if path == "f64" else "f32"
    X, Y, want, mag = _xcov_operands(path, I, P, M, masked, name)
    base = X.data_ptr() % 32
    assert MC.plan_xcov(I, P) == plan
    assert [t[2] for t in MC.xcov_instances(storage, I, P, M, base=base, mixed=mixed)] == insts
    assert be.lib.cmtfpls_xcov_workspace_bytes(I, P, M) == MC.xcov_workspace_bytes(I, P, M) == plan[2] * min(M, 64) * P * 8
    keep = X.clone()
    S = be.xcov(X, Y, masked, mixed=mixed)
    coeff = MC.MIXED_RTOL if mixed else MC.f64_bound(I)
    r = _ratio(f"xcov {path}", S, want, mag, coeff)
    print(f"xcov {path} {shape} masked={masked} {name}: error / bound {r:.3g}")
    assert r <= 1.0, (name, r)
    assert torch.equal(_bits(be.xcov(X, Y, masked, mixed=mixed)), _bits(S))
    assert torch.equal(_bits(X), _bits(keep))
    if not mixed and not masked:
        # the SSQ instances of the same shape: S and |X - mean|^2 from one read
        mean = torch.randn(P, generator=_gen(P + M), device=DEV, dtype=F64)
        S2, ssq = be.xcov_ssq(X, Y, mean, be.empty(M, P))
        r2 = _ratio(f"xcov_ssq {path}", S2, want, mag, coeff)
        want_ssq = ((X.double() - mean) ** 2).sum()
        rs = abs(ssq.item() - want_ssq.item()) / (MC.f64_bound(I * P) * want_ssq.item())
        print(f"xcov_ssq {path} {shape} {name}: error / bound {r2:.3g}, norm {rs:.3g}")
        assert r2 <= 1.0 and rs <= 1.0, (name, r2, rs)
        assert torch.equal(_bits(X), _bits(keep))


@pytest.mark.parametrize("masked", [False, True], ids=["complete", "masked"])
@pytest.mark.parametrize("path", ["mixed", "f32", "f64"])
@pytest.mark.parametrize("name,shape,plan,insts", MC.XCOV_CASES, ids=[c[0].replace(" ", "_") for c in MC.XCOV_CASES])
def test_xcov_fast_forms_and_dispatch_edges(be, name, shape, plan, insts, path, masked):
    """path: "mixed" = xcov_mixed_kernel on f32 X; "f32" / "f64" = xcov_kernel<float | double> (and, unmasked, its SSQ form)."""
    _check_xcov(be, path, name, shape, plan, insts, masked)


@pytest.mark.parametrize("masked", [False, True], ids=["complete", "masked"])
def test_xcov_mixed_with_128_rows_per_block(be, masked):
    """(8192, 4096, 16): 64 row blocks of 128 rows -- four trips per block, the f32 chain of 64 rows flushed after the second
    trip and again at the end."""
    name, shape, plan, insts = MC.XCOV_BIG
    _check_xcov(be, "mixed", name, shape, plan, insts, masked)
