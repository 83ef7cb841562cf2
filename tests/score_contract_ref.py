"""Python mirror of the host dispatch of the one-read score and contraction kernel, its extended-precision reference and its
error bounds -- TEST INFRASTRUCTURE ONLY (NumPy, no backend, no torch; checked without a GPU by test_score_contract_ref_cpu.py).

  form       run_score_contract<T>                       csrc/scorecontract.hip
  reference  t = X w - shift - sub_own,  c = alpha (t + add_other),  Z = X^T c,  sum(c)   in np.longdouble

`form` is written from the dispatch code, line by line, and names the kernel template instance a shape selects (or the rule
that declines it), so that a test can state which instance it covers and a change of the dispatch shows as a failing mirror.

Bounds (none taken from a kernel's output; the convention of matrix_core_ref: (n + 4) 2^-53 sum|terms| for ANY order of a
float64 sum of n products, Higham eq. 3.5):
  t_i     (P + 6) 2^-53 (sum_c |x_ic w_c| + |shift| + |sub_own_i|)       P products, w_c = wA wB formed in either association,
                                                                         the two subtractions
  Z_col   (I + 4) 2^-53 sum_i |c_i x_ic|  +  sum_i |alpha x_ic| bt_i     the sum itself + what the error of t carries into c
  sum(c)  (I + 4) 2^-53 sum_i |c_i|  +  |alpha| sum_i bt_i
"""
import numpy as np

U64 = 2.0 ** -53
K_SC_GRID = 256                 # kScGrid: workgroups of the row form, row streams x slabs of the split form
K_SPLIT_MAX_G = 16              # kSplitMaxG
K_SC_LDS_A = 2048               # kScLdsA: mode-1 loadings the WL instance keeps in LDS
EINVAL, EWORKSPACE, EUNSUPPORTED = 1, 2, 4

# the reference's own arithmetic: x87 extended (64-bit significand) -- asserted, not assumed
LONGDOUBLE_IS_WIDER = np.finfo(np.longdouble).eps <= 2.0 ** -63


def _elem(dtype):
    return {"f32": 4, "f64": 8}[dtype]


def stride_of(dtype):
    return 1024 * (16 // _elem(dtype))


def workspace_bytes(I, P):
    """cmtfpls_score_contract_workspace_bytes: partial rows of Z | csum | exchange slots, for whichever form the entry takes."""
    if I <= 0 or P <= 0:
        return 0
    return (min(I, K_SC_GRID) * (P + 1) + I * K_SPLIT_MAX_G) * 8


def _rows(I, step):
    """Rows of workgroup / stream s = 0 .. step - 1 walking s, s + step, ...: (min, max) over those that have any."""
    n = [(I - s + step - 1) // step for s in range(step) if s < I]
    return min(n), max(n), sorted(set(n))


def form(dtype, I, A, B, cus, aligned=True):
    """run_score_contract<T>: {"decline": reason, "status": code} or the instance with its launch geometry.

    row form    {"form": "rows", "nv": vectors of 16 bytes a row needs per lane, "NV", "KC", "WL", "jstep": mode-1 slices per stride
                 (KC only, else None), "grid", "rows": (min, max) rows per workgroup, "need"}
    split form  {"form": "split", "nv", "NVS", "KC", "LAG", "G", "S", "rows": (min, max) rows per stream,
                 "remainders": the (nrows + LAG) % (LAG + 2) that occur, "need"}
    `cus` is the device's compute-unit count; `aligned`: X starts on a 16-byte boundary."""
    if I <= 0 or A <= 0 or B <= 0:
        return {"decline": "bad argument", "status": EINVAL}
    es = _elem(dtype)
    V = 16 // es
    P = A * B
    stride = 1024 * V
    nv = (P + stride - 1) // stride
    max_nv = 4 if V == 4 else 8
    for bad, why in ((B % V != 0, "B % V != 0"), (P < stride // 2, "P < stride / 2"), (P >= 1 << 31, "P >= 2^31"),
                     (not aligned, "X not 16-byte aligned")):
        if bad:
            return {"decline": why, "status": EUNSUPPORTED}
    kc = stride % B == 0
    if nv > max_nv:
        nvs = 2 if (es == 4 and not kc) else 4
        G = (nv + nvs - 1) // nvs
        cus = min(cus, K_SC_GRID)
        S = min(I, cus // G)
        if G > K_SPLIT_MAX_G:
            return {"decline": f"G = {G} > 16", "status": EUNSUPPORTED}
        if S < 1:
            return {"decline": "S < 1", "status": EUNSUPPORTED}
        if es == 8:
            lag = 2 if kc else 1
        else:
            lag = 1 if kc else 2
        lo, hi, counts = _rows(I, S)
        return {"form": "split", "nv": nv, "NVS": nvs, "KC": kc, "LAG": lag, "G": G, "S": S, "rows": (lo, hi),
                "remainders": sorted({(n + lag) % (lag + 2) for n in counts}), "need": (S * (P + 1) + I * G) * 8}
    grid = min(I, K_SC_GRID)
    NV = 1 if nv <= 1 else 2 if nv <= 2 else 4 if nv <= 4 else 8
    wl = NV == 8 and kc and P == 8 * stride and A <= K_SC_LDS_A
    lo, hi, _ = _rows(I, grid)
    return {"form": "rows", "nv": nv, "NV": NV, "KC": kc, "WL": wl, "jstep": stride // B if kc else None, "grid": grid,
            "rows": (lo, hi), "need": grid * (P + 1) * 8}


def instance(f):
    """The template instance of a form: ("rows", NV, KC, WL) | ("split", NVS, KC, LAG) | None (declined)."""
    if "decline" in f:
        return None
    return ("rows", f["NV"], f["KC"], f["WL"]) if f["form"] == "rows" else ("split", f["NVS"], f["KC"], f["LAG"])


# every instance the dispatch can select (test_score_contract_ref_cpu.py finds the same set by enumeration)
INSTANCES = {
    "f32": [("rows", nv, kc, False) for nv in (1, 2, 4) for kc in (False, True)] + [("split", 4, True, 1), ("split", 2, False, 2)],
    "f64": [("rows", nv, kc, False) for nv in (1, 2, 4, 8) for kc in (False, True)] + [("rows", 8, True, True),
                                                                                       ("split", 4, True, 2), ("split", 4, False, 1)],
}


# ---- data, reference and bounds ---------------------------------------------------------------------------------------------
SHIFT = 1.25
ALPHA_COUPLED = 0.5


def make_case(dtype, I, A, B):
    """x ~ N(0, 1) colscale + 2.0 rounded to the storage type (held as float64), random loadings and the coupled call's vectors."""
    rng = np.random.default_rng(100003 * I + 101 * A + B + (7 if dtype == "f64" else 0))
    P = A * B
    colscale = np.exp(rng.uniform(-2.0, 2.0, size=P))
    x = rng.standard_normal((I, P)) * colscale + 2.0
    if dtype == "f32":
        x = x.astype(np.float32).astype(np.float64)
    return {"x": x, "wA": rng.standard_normal(A), "wB": rng.standard_normal(B),
            "sub_own": rng.standard_normal(I) * 10.0, "add_other": rng.standard_normal(I) * 10.0}


def reference(x, A, B, wA, wB, shift, sub_own, add_other, alpha):
    """t, c, Z, sum(c) in np.longdouble from the storage-rounded x (float64 array), and the per-element bounds bt, bZ, bc in
    float64.  shift: float or None; sub_own, add_other: (I,) or None."""
    assert LONGDOUBLE_IS_WIDER, "np.longdouble is no wider than float64 on this host: the reference would prove nothing"
    LD = np.longdouble
    I, P = x.shape
    assert P == A * B
    w = (wA.astype(LD)[:, None] * wB.astype(LD)[None, :]).reshape(P)
    w64 = np.abs(w).astype(np.float64)
    xw = np.empty(I, dtype=LD)
    step = max(1, (1 << 22) // P)
    for lo in range(0, I, step):                               # row chunks: at most 64 MB of longdouble at a time
        xw[lo:lo + step] = (x[lo:lo + step].astype(LD) * w).sum(axis=1)
    ax = np.abs(x)
    mag_t = ax @ w64
    sh = LD(0.0 if shift is None else shift)
    t = xw - sh
    mag_t = mag_t + abs(float(sh))
    if sub_own is not None:
        t = t - sub_own.astype(LD)
        mag_t = mag_t + np.abs(sub_own)
    c = t if add_other is None else t + add_other.astype(LD)
    c = LD(alpha) * c
    Z = np.empty(P, dtype=LD)
    cstep = max(1, (1 << 22) // I)
    for lo in range(0, P, cstep):
        Z[lo:lo + cstep] = (c[:, None] * x[:, lo:lo + cstep].astype(LD)).sum(axis=0)
    bt = (P + 6) * U64 * mag_t * (1.0 + 2.0 ** -40)            # (the bound's own float64 rounding, upwards)
    c64 = np.abs(c).astype(np.float64)
    bZ = ((I + 4) * U64 * (c64 @ ax) + abs(alpha) * (bt @ ax)) * (1.0 + 2.0 ** -40)
    bc = ((I + 4) * U64 * c64.sum() + abs(alpha) * bt.sum()) * (1.0 + 2.0 ** -40)
    return {"t": t, "c": c, "Z": Z, "csum": c.sum(), "bt": bt, "bZ": bZ, "bc": bc}


def within(r):
    """Every ratio of `ratios` is at most 1.  Written per value: max() of a collection drops a NaN that does not come first, and a
    NaN (from a NaN in the kernel's output) must fail."""
    return all(v <= 1.0 for v in r.values())


def ratios(ref, t, Z, csum=None):
    """Worst |got - want| / bound of t, Z (and sum(c)); the differences are taken in longdouble.  NaN in `got` gives NaN."""
    LD = np.longdouble
    out = {"t": float(np.max(np.abs(t.astype(LD) - ref["t"]) / ref["bt"])), "Z": float(np.max(np.abs(Z.astype(LD) - ref["Z"]) / ref["bZ"]))}
    if csum is not None:
        out["csum"] = float(abs(LD(csum) - ref["csum"]) / ref["bc"])
    return out


def evaluate_f64(x, A, B, wA, wB, shift, sub_own, add_other, alpha, order):
    """The same sums in plain float64, in one of three orders -- "forward" (NumPy's own pairwise / BLAS order), "reversed",
    "chunked" (partial sums over chunks of 4096 terms, then the partial sums): what the bounds are checked against on the CPU."""
    I, P = x.shape
    w = (wA[:, None] * wB[None, :]).reshape(P)

    def total(terms, axis):
        if order == "forward":
            return terms.sum(axis=axis)
        tm = np.moveaxis(terms, axis, -1)                      # np.cumsum adds strictly one after the other
        if order == "reversed":
            return np.cumsum(tm[..., ::-1], axis=-1)[..., -1]
        parts = [np.cumsum(tm[..., lo:lo + 4096], axis=-1)[..., -1] for lo in range(0, tm.shape[-1], 4096)]
        return np.cumsum(np.stack(parts, axis=-1), axis=-1)[..., -1]

    t = total(x * w, 1) - (0.0 if shift is None else shift)
    if sub_own is not None:
        t = t - sub_own
    c = alpha * (t if add_other is None else t + add_other)
    Z = total(c[:, None] * x, 0)
    return t, Z, total(c, 0)


# ---- the cases of tests/test_gpu_score_contract_forms.py: (I, A, B) -> the f32 and the f64 instance at 256 compute units ------
# an instance is ("rows", NV, KC, WL) or ("split", NVS, KC, LAG, G); a string is the decline reason
def _r(nv, kc, wl=False):
    return ("rows", nv, kc, wl)


ROW_CASES = [
    ((300, 25, 100), _r(1, False), _r(2, False)),
    ((300, 12, 340), _r(1, False), _r(2, False)),              # B > stride / 8
    ((300, 1, 2044), "P < stride / 2", _r(1, False)),
    ((513, 64, 128), _r(2, True), _r(4, True)),                # 2 or 3 rows per workgroup
    ((300, 41, 100), _r(2, False), _r(4, False)),              # f64 nv = 3: one wholly absent vector
    ((300, 150, 100), _r(4, False), _r(8, False)),
    ((100, 120, 128), _r(4, True), _r(8, True)),               # f64 not WL: P != 8 stride
    ((100, 4096, 4), _r(4, True), _r(8, True)),                # f64 not WL: A > 2048; B = V for f32
    ((60, 2048, 8), _r(4, True), _r(8, True, True)),           # WL with wls[] full
    ((60, 8, 2048), _r(4, True), _r(8, True, True)),           # WL with jstep = 1
    ((64, 16, 128), _r(1, True), _r(1, True)),                 # the shortest f32 row
    # the two-buffer row loop and its exits: 1, 1, 2, 3|4 and 4|5 rows per workgroup
    ((255, 32, 128), _r(1, True), _r(2, True)),
    ((256, 32, 128), _r(1, True), _r(2, True)),
    ((512, 32, 128), _r(1, True), _r(2, True)),
    ((769, 1, 2048), _r(1, True), _r(1, True)),
    ((1025, 8, 256), _r(1, True), _r(1, True)),
]
ROWS_PER_WORKGROUP = {(255, 32, 128): (1, 1), (256, 32, 128): (1, 1), (512, 32, 128): (2, 2), (769, 1, 2048): (3, 4),
                      (1025, 8, 256): (4, 5), (513, 64, 128): (2, 3)}


def _s(nvs, kc, lag, G):
    return ("split", nvs, kc, lag, G)


SPLIT_CASES = [
    ((40, 160, 128), _s(4, True, 1, 2), _s(4, True, 2, 3)),            # the smallest G; one row per stream
    ((60, 2049, 8), _s(4, True, 1, 2), _s(4, True, 2, 3)),             # one slice past WL; the last slab almost empty
    ((70, 5, 3300), _s(2, False, 2, 3), _s(4, False, 1, 3)),
    ((70, 5, 6500), _s(2, False, 2, 4), _s(4, False, 1, 4)),           # S = 64: streams with 1 and 2 rows
    ((37, 512, 512), _s(4, True, 1, 16), "G = 32 > 16"),               # the f32 maximum
    ((37, 256, 512), _s(4, True, 1, 8), _s(4, True, 2, 16)),           # the f64 maximum
    ((37, 257, 512), _s(4, True, 1, 9), "G = 17 > 16"),
    ((37, 513, 512), "G = 17 > 16", "G = 33 > 16"),
    ((33, 1, 131072), _s(2, False, 2, 16), _s(4, False, 1, 16)),       # a matrix block at the limit
    ((33, 1, 131074), "B % V != 0", "G = 17 > 16"),
    ((70, 3, 43000), _s(2, False, 2, 16), _s(4, False, 1, 16)),        # 4 or 5 rows per stream
    # the north-star row at I = 1, I <= S, I = S + 1 (f32 S = 64, f64 S = 32) and 2 .. 7 rows per stream
    ((1, 256, 256), _s(4, True, 1, 4), _s(4, True, 2, 8)),
    ((16, 256, 256), _s(4, True, 1, 4), _s(4, True, 2, 8)),
    ((17, 256, 256), _s(4, True, 1, 4), _s(4, True, 2, 8)),
    # added for I = S + 1 only (one stream with a second row); they fill no remainder, those are complete without them
    ((33, 256, 256), _s(4, True, 1, 4), _s(4, True, 2, 8)),            # f64: I = S + 1
    ((65, 256, 256), _s(4, True, 1, 4), _s(4, True, 2, 8)),            # f32: I = S + 1
    ((129, 256, 256), _s(4, True, 1, 4), _s(4, True, 2, 8)),
    ((200, 256, 256), _s(4, True, 1, 4), _s(4, True, 2, 8)),
]
ALL_CASES = ROW_CASES + SPLIT_CASES

NAN_CASES = [(300, 128, 128), (129, 256, 256)]                  # one per form, for either storage type
CONTRACT_CASES = {"f32": [(70, 32, 128), (20, 160, 128)], "f64": [(70, 32, 128), (20, 160, 128)]}   # a row-form and a split-form shape


def claimed(dtype, shape):
    for s, f32, f64 in ALL_CASES:
        if s == shape:
            return f32 if dtype == "f32" else f64
    raise KeyError(shape)


def check_claim(dtype, shape, cus):
    """form() of the case at `cus` compute units, after asserting that it is what the table claims.  A split case whose G exceeds
    the compute units is a decline (S < 1) instead."""
    f = form(dtype, *shape, cus=cus)
    want = claimed(dtype, shape)
    if isinstance(want, str):
        assert f.get("decline") == want, (dtype, shape, f)
    elif want[0] == "split" and min(cus, K_SC_GRID) < want[4]:
        assert f.get("decline") == "S < 1", (dtype, shape, f)
    elif want[0] == "split":
        assert instance(f) + (f["G"],) == want, (dtype, shape, f)
    else:
        assert instance(f) == want, (dtype, shape, f)
    return f
