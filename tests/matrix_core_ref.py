"""Python mirrors of the host dispatch of the two matrix-core contractions, and their error bounds -- TEST INFRASTRUCTURE ONLY
(no backend, no torch; checked without a GPU by test_matrix_core_ref_cpu.py).

  mttkrp_instance        run_mttkrp<T>                  csrc/mttkrp.hip   (default build: no CMTFPLS_MTTKRP_* override)
  mttkrp_mixed_instance  cmtfpls_mttkrp_f32_mixed       csrc/mixed.hip
  plan_xcov              plan_xcov                      csrc/xcov.hip     (CMTFPLS_XCOV_BLOCKS = 1024)
  xcov_instances         run_xcov / run_xcov_tile and cmtfpls_xcov_f32_mixed

Every mirror is written from the dispatch code, line by line, and names the kernel template instance a shape selects (or None for
a decline), so that a test can state which instance it covers and a change of the dispatch shows as a failing mirror.

`base` is the byte offset of X's first element from a 32-byte boundary (what the alignment tests of the dispatch see).

Bounds (none taken from a kernel's output):
  f64 kernels    |got - want| <= (n + 4) 2^-53 sum|terms|, n products per entry: the float64 accumulation bound for ANY order of
                 summation (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5, gamma_n ~ n u), plus the rounding of
                 the reference's own operand product and of the two conversions.
  mixed kernels  |got - want| <= 2e-6 sum|terms|, the contract stated in csrc/mixed.hip and tests/test_gpu_mixed.py.  The worst
                 case of one f32 chain is 257 2^-24 sum|terms| (256 chained roundings and the one rounding of the second operand).
"""

U64 = 2.0 ** -53
MIXED_RTOL = 2e-6
MIXED_CHAIN_WORST = 257 * 2.0 ** -24

MTTKRP_LDS_MAX = 152 * 1024
MIXED_LDS_MAX = 96 * 1024
XCOV_MAX_RESPONSES = 64
XCOV_BLOCKS = 1024
JK_GRID = 2048                  # workgroups of the per-sample forms, 4 wavefronts each: 8192 samples per grid round
TILE_GROUPS = 8192              # 16-row groups per grid round of the tile forms: 131072 rows


def f64_bound(n):
    """Coefficient of sum|terms| for an f64 kernel that adds n products per entry."""
    return (n + 4) * U64


def _elem(dtype):
    return {"f32": 4, "f64": 8}[dtype]


# ---- M = X_(0) (WA (.) WB) ------------------------------------------------------------------------------------------------
def mttkrp_instance(dtype, I, A, B, R, base=0):
    """run_mttkrp<T>: ("kj4", NL, NG) | ("kj", NL) | ("jk", CH, NPJ, BREG) | ("tile", VEC, RT, FAST, NT) | None (declined)."""
    if R > 32:
        return None
    rt = (R + 15) // 16
    lds = (A + B) * 16 * rt * 8
    if lds > MTTKRP_LDS_MAX:
        return None
    es = _elem(dtype)
    V = 16 // es
    lds1 = (A + B) * 16 * 8
    if R <= 16 and A % 16 == 0 and base % 16 == 0 and lds1 <= MTTKRP_LDS_MAX:
        nlw = 2 if V == 4 else 4
        nlh = nlw // 2
        wide = B % (nlw * 16 * V) == 0 and A % (4 * (8 // nlw)) == 0
        half = B % (nlh * 16 * V) == 0 and A % (4 * (8 // nlh)) == 0
        if V == 4 and R <= 12:
            ng = 1 if R <= 4 else 2 if R <= 8 else 3 if R <= 12 else 4
            if wide:
                return ("kj4", nlw, ng)
            if half:
                return ("kj4", nlh, ng)
        if wide:
            return ("kj", nlw)
        if half:
            return ("kj", nlh)
        npatch = B // (4 * V) if B % (4 * V) == 0 else 0
        if npatch == 8:
            return ("jk", 8, 1, True)
        if npatch == 4:
            return ("jk", 4, 1, True)
        if npatch == 16 and V == 2:
            return ("jk", 8, 2, True)
        if npatch > 0 and npatch % 8 == 0:
            return ("jk", 8, 1, False)
        if npatch > 0 and npatch % 4 == 0:
            return ("jk", 4, 1, False)
    vec = B % 4 == 0 and base % (4 * es) == 0
    ngroups = (I + 15) // 16
    nt = 256
    if vec:
        wgs_per_cu = (160 * 1024) // lds
        while nt < 1024 and wgs_per_cu * (nt // 64) < 16:
            nt *= 2
        while nt > 256 and (ngroups + nt // 64 - 1) // (nt // 64) < 256:
            nt //= 2
    fast = vec and I % 16 == 0 and (A * B) % 64 == 0
    return ("tile", vec, rt, fast, nt)


def mttkrp_mixed_instance(I, A, B, R, base=0):
    """cmtfpls_mttkrp_f32_mixed: ("kj_mixed", NL) | ("tile_mixed", VEC, RT) | None (declined)."""
    if R > 32:
        return None
    rt = (R + 15) // 16
    if (A + B) * 16 * rt * 8 > MIXED_LDS_MAX:
        return None
    vec = B % 4 == 0 and base % 16 == 0
    if R <= 16 and vec:
        lds_kj = B * 16 * 8 + A * 16 * 4
        if lds_kj <= 64 * 1024:
            if B % 128 == 0 and A % 16 == 0:
                return ("kj_mixed", 2)
            if B % 64 == 0 and A % 32 == 0:
                return ("kj_mixed", 1)
    return ("tile_mixed", vec, rt)


def mttkrp_rounds(inst, I):
    """Grid rounds of the instance's outer loop: > 1 means that a wavefront takes a second sample / a second 16-row group."""
    if inst[0] in ("kj4", "kj", "jk", "kj_mixed"):
        grid = min((I + 3) // 4, JK_GRID)
        return -(-I // (grid * 4))
    ngroups = (I + 15) // 16
    nw = inst[4] // 64 if inst[0] == "tile" else 4
    grid = min((ngroups + nw - 1) // nw, TILE_GROUPS // nw)
    return -(-ngroups // (grid * nw))


def sample_chunks(inst, dtype, A, B):
    """Register-buffer chunks per sample of a per-sample instance (the loop that alternates b0 / b1)."""
    V = 16 // _elem(dtype)
    if inst[0] == "jk":
        _, ch, npj, breg = inst
        return (A // 16) * (npj if breg else B // (4 * V * ch))
    nl = inst[1]
    chj = 8 // nl
    return (B // (nl * 16 * V)) * (A // (4 * chj))            # passes x chunks per pass


# ---- S = Y^T X_(0) ----------------------------------------------------------------------------------------------------------
def plan_xcov(I, P):
    """(col_tiles, rows_per_block, row_blocks)."""
    col_tiles = (P + 255) // 256
    want = max((XCOV_BLOCKS + col_tiles - 1) // col_tiles, 1)
    rpb = max((-(-I // want) + 63) // 64 * 64, 64)
    return col_tiles, rpb, max(-(-I // rpb), 1)


def xcov_workspace_bytes(I, P, M):
    return plan_xcov(I, P)[2] * min(M, XCOV_MAX_RESPONSES) * P * 8


def xcov_instances(dtype, I, P, M, base=0, mixed=False):
    """One (first response, responses, (VEC, MT, FAST)) per pass over X: tiles of <= 64 responses.  MASKED (and SSQ for
    cmtfpls_xcov_ssq_*) are the caller's flags and select nothing else."""
    es = _elem(dtype)
    assert not mixed or dtype == "f32"
    _, rpb, _ = plan_xcov(I, P)
    vec = P % 4 == 0 and base % (16 if mixed else 4 * es) == 0
    out = []
    for lo in range(0, M, XCOV_MAX_RESPONSES):
        m = min(M - lo, XCOV_MAX_RESPONSES)
        mt = (m + 15) // 16
        fast = vec and P % 256 == 0 and m % 16 == 0 and m // 16 != 3 and I % rpb == 0 and rpb % 32 == 0
        out.append((lo, m, (vec, 4 if mt >= 3 else mt, fast)))
    return out


# ---- the cases of tests/test_gpu_matrix_core_limits.py: (storage | "mixed", (A, B), R, the instance, sample counts) ------------
ROUND_IS = (8193, 16421)        # one wavefront takes a second sample; two full grid rounds and a ragged third
TILE_IS = (131125, 135168)      # 8196 ragged row groups (guarded); 8448 whole groups (FAST where the loads are vectors)

SAMPLE_CASES = [
    ("f32", (16, 128), 3, ("kj4", 2, 1), ROUND_IS),
    ("f32", (16, 128), 7, ("kj4", 2, 2), ROUND_IS),
    ("f32", (16, 128), 10, ("kj4", 2, 3), ROUND_IS),
    ("f32", (16, 128), 12, ("kj4", 2, 3), ROUND_IS),            # three full component groups (NG = 4 is unreachable)
    ("f32", (32, 64), 3, ("kj4", 1, 1), ROUND_IS),
    ("f32", (32, 64), 7, ("kj4", 1, 2), ROUND_IS),
    ("f32", (32, 64), 10, ("kj4", 1, 3), ROUND_IS),
    ("f32", (16, 128), 14, ("kj", 2), ROUND_IS),
    ("f32", (32, 64), 14, ("kj", 1), ROUND_IS),
    ("f32", (32, 256), 16, ("kj", 2), ROUND_IS),                # two passes of two chunks: the pair loop's last prefetch
    ("f64", (16, 128), 10, ("kj", 4), ROUND_IS),                # two chunks
    ("f64", (16, 64), 10, ("kj", 2), ROUND_IS),
    ("f32", (16, 64), 10, ("jk", 4, 1, True), ROUND_IS),
    ("f64", (16, 32), 10, ("jk", 4, 1, True), ROUND_IS),
    ("f32", (16, 192), 10, ("jk", 4, 1, False), ROUND_IS),      # npj = 3
    ("f64", (16, 96), 10, ("jk", 4, 1, False), ROUND_IS),       # npj = 3
    ("mixed", (48, 128), 10, ("kj_mixed", 2), ROUND_IS),        # three chunks: one pair and the odd tail
    ("mixed", (32, 64), 7, ("kj_mixed", 1), ROUND_IS),
    ("mixed", (272, 128), 5, ("kj_mixed", 2), (8193,)),         # 17 chunks: an f32 chain of 16 and one of 1 per pass
]

# A % 16 != 0 keeps f64 (8, 128) out of the per-sample forms: it takes the tile form with vector loads
NOT_PER_SAMPLE = ("f64", (8, 128), 10, ("tile", True, 1, False, 256), (8193,))

TILE_CASES = [
    (st, (3, 5), 5, {I: ("tile", False, 1, False, 256) for I in TILE_IS}) for st in ("f32", "f64")] + [
    (st, (3, 5), 20, {I: ("tile", False, 2, False, 256) for I in TILE_IS}) for st in ("f32", "f64")] + [
    (st, (1, 64), 5, {131125: ("tile", True, 1, False, 256), 135168: ("tile", True, 1, True, 256)}) for st in ("f32", "f64")] + [
    ("mixed", (3, 5), 20, {I: ("tile_mixed", False, 2) for I in TILE_IS}),
    ("mixed", (1, 64), 20, {I: ("tile_mixed", True, 2) for I in TILE_IS}),
]

# (name, (I, P, M), plan, one (VEC, MT, FAST) per pass of <= 64 responses); the same instances for the f64 and the mixed kernel
XCOV_CASES = [
    ("FAST MT=1", (64, 256, 16), (1, 64, 1), [(True, 1, True)]),
    ("FAST MT=2", (64, 256, 32), (1, 64, 1), [(True, 2, True)]),
    ("FAST MT=4", (64, 256, 64), (1, 64, 1), [(True, 4, True)]),
    ("M=48 guarded MT=4", (64, 256, 48), (1, 64, 1), [(True, 4, False)]),
    ("M=80 FAST MT=4 + MT=1, ldy=86", (64, 256, 80), (1, 64, 1), [(True, 4, True), (True, 1, True)]),
    ("two row blocks FAST MT=1", (128, 256, 16), (1, 64, 2), [(True, 1, True)]),
    ("misaligned scalar MT=1", (64, 256, 16), (1, 64, 1), [(False, 1, False)]),
]
XCOV_BIG = ("rows_per_block=128 FAST MT=1", (8192, 4096, 16), (16, 128, 64), [(True, 1, True)])
