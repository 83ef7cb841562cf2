"""NumPy long-double restatements, written-field masks, derived bounds and input builders for the K-fold epilogue kernels of
csrc/kfold.hip: kfold_rows_kernel<MODE>, kfold_solve_kernel, kfold_ydefl_kernel<MODE>, kfold_downdate_kernel<GROUPED> and
kfold_combine_kernel.  No GPU and no torch here: tests/test_kfold_epilogue_ref_cpu.py checks this module on the CPU (a chain of
the stages against literal refits per model), tests/test_gpu_kfold_epilogue_stages.py runs the kernels against it.  `U`, `gamma`,
`bound_sum`, `LD` and `REF_SLACK` are those of tests/small_algebra_ref.py; the solve's bound is tests/solve_ref.py's.

The state
---------
A dict of NumPy arrays named after the fields of cmtfpls_kfold_state, n = K models:
  fold_of (I,) | (splits, I) | (n, I) counts     Yk (n, I, M)     Gy (n, NT, M, M)     Q (n, R, M)     T (n, I, R)
  Gt (n, R, R)   coef (n, R, R)   tm (I, n)   Tout (slots, I, R)   vec (n, 3R + M + 2)   status (n,)   part (n, NT, 193)
  S (n, M, P)   mean (rows, P)   Wa (n, R, A)   Wb (n, R, B)   Rm (n, R, P)   WA (A, n)   WB (B, n)   n_iter (n, R)
vec of a model: b (R) | c (R) | ya (M) | 1^T t (1) | g (R) | mu^T w (1).
A `Layout` says which rows train a model and where its held-out scores go: the mode, model_fold (grouped) and `div`, the
kernels' own last argument: the number of groups (grouped) or the folds per split (splits).

Every restatement returns the values of every field its kernel writes, in long double, next to the elementwise bound of the
float64 kernel; `apply_*` stores them (rounded to float64) into a state, which is how the CPU test chains the stages.

Bounds (u = 2^-53; "n terms in any order, fused or not" is bound_sum, Higham Lemma 3.1 / 8.4; each is restated at its line)
---------------------------------------------------------------------------------------------------------------------------
Where a quantity is a sum of products of factors that are themselves computed (u = c * sum Y q, tt = c * t, w = Wa * Wb), the
sum is FLATTENED: it is a sum of products of stored float64 numbers, and every such product passes at most `chain` roundings on
its way into the result (the roundings of the factors it is in, then the additions).  (1 + theta_chain) on every term gives
|error| <= gamma_chain * sum |terms| exactly as for a plain sum.  The chain length is stated next to each use.

The three kernels of stage 1 are bounded separately by giving each its device inputs: the row sums use the device's own T[:, a]
(`t_dev`), the solve the tile-order float64 totals of the device's own `part` (the kernel's own additions, so Gt, ya and 1^T t
are EQUAL to them), the deflation the device's vec[:kk] and the Gram partials the device's deflated Yk.  `composed_residual`
bounds the solve from the original inputs: with G, g the restated normal equations and G~, g~ the device's (|G~ - G| <= eG,
|g~ - g| <= eg from the row bounds, two-level for the squares), the device's b satisfies |D~ (G~ b - g~)| <= bound~ by
solve_ref.normal_solve_bound, so |D (G b - g)| <= (d / d~) bound~ + d (eG |b| + eg).

Exact inputs
------------
Rows come in aligned blocks of 2^p >= R rows; on a block a model's scores are the first columns of the Sylvester Hadamard matrix of
order 2^p scaled by powers of two, or zero.  Fold maps and bootstrap counts are constant on a block, so the training Gram of every
model is exactly diagonal, N 4^e with N the weighted number of non-zero training rows.  sc = mu^T w + T g + (the new Hadamard
column) with integer g; Yk holds -1, 0, 1 and q at most two entries of +-1, so |u| <= 3 * 2: every sum of the row kernel is a sum
of dyadic numbers far below 2^53 and the device has to EQUAL the restatement.  The builder keeps, per model, only as many
non-zero training blocks as make N a power of 4 (the heaviest counts first).  Where that works out (builder flag `solve_exact`)
the equilibration is exact, b = g / (N 4^e) is dyadic and the solve, the deflation and the next Gram are equal to the
restatement too; elsewhere those three are checked on rounding inputs only: 17 of the 144 cases of row_stage_cases() -- the
"single" map at K = 2 with blocks of more than one row ((600, 64, 2, 64, a) and (32769, 2, 2, 2, 1) in plain, grouped and splits
mode: the model that trains on the single row has no whole block), and five weighted cases whose counts do not add up to a
power of 4 ((257, 3, 3, 4, a) and (300, 16, 32, 2, 1) "contiguous", (600, 64, 2, 64, 62) "shuffled").  A column twice column 0
then has the pivot 1 - 1 * 1 = 0 in every evaluation order.
(The deflated y = Y - (T b) q is an integer over N of magnitude <= 1 + 6 kk; in ROW_CASES kk = 64 comes with N = 256 and N = 4^7
with kk <= 3: at most 9 + 8 or 5 + 14 bits, a square 40, and a tile's weighted sum of at most 547 * 3 squares stays below 2^53.)

Rounding inputs
---------------
Normal data, the score columns scaled over three decades and the responses over two, training Gram of the earlier columns
consistent with T.  tests/test_kfold_epilogue_ref_cpu.py asserts solve_ref.assert_pivot_margins for every case the GPU file
runs: kernel and restatement must take the same drop decisions.
"""
import collections
import math

import numpy as np

import small_algebra_ref as SA
import solve_ref as SR
from small_algebra_ref import LD, REF_SLACK, U, bound_sum, gamma

PLAIN, GROUPED, SPLITS, WEIGHTED = "plain", "grouped", "splits", "weighted"
MODES = [PLAIN, GROUPED, SPLITS, WEIGHTED]
ROW_THREADS, MAX_TILES, CHUNK, MAX_R, MAX_M = 256, 128, 32, 64, 64
PART_STRIDE = 2 * MAX_R + 1 + MAX_M
SENTINEL = -7.25e300

Layout = collections.namedtuple("Layout", "mode model_fold div slots")


# ---- the row tiles ---------------------------------------------------------------------------------------------------------
def kf_tiles(I):
    return min(MAX_TILES, max(1, -(-I // ROW_THREADS)))


def tile_rows(I):
    """[(lo, hi)] of kf_tile_rows for every tile of kf_tiles(I)."""
    NT = kf_tiles(I)
    ln = -(-I // NT)
    return [(min(I, t * ln), min(I, (t + 1) * ln)) for t in range(NT)]


def vec_len(R, M):
    return 3 * R + M + 2


def dims(st):
    n, I, M = st["Yk"].shape
    R = st["T"].shape[2]
    return n, I, M, R


def training(lay, fold_of, k):
    """(train (I,) bool, weight (I,) float64: the count of a weighted model, else the mask itself)."""
    if lay.mode == WEIGHTED:
        c = fold_of[k]
        return c > 0, c.astype(np.float64)
    if lay.mode == GROUPED:
        tr = fold_of != lay.model_fold[k]
    elif lay.mode == SPLITS:
        tr = fold_of[k // lay.div] != k % lay.div
    else:
        tr = fold_of != k
    return tr, tr.astype(np.float64)


def tout_slot(lay, k):
    return {PLAIN: 0, GROUPED: k % lay.div, SPLITS: k // lay.div, WEIGHTED: None}[lay.mode]


# ---- stage 1a: kfold_rows_kernel ---------------------------------------------------------------------------------------------
def rows(lay, st, a, sc, t_dev=None):
    """Component a of every model.  Returns a dict:
    T (n, I) long double, the new column, and T_err; tm (I, n); tout [(slot, rows, k)]; part (n, NT, nv) and part_err, the
    partials in the kernel's order T_train^T t (kk) | T_train^T u (kk) | 1^T t_train | Yk^T t (M), formed from the float64
    column `t_dev` (n, I) where it is given (the device's own), else from round(T)."""
    n, I, M, R = dims(st)
    kk, nv, tiles = a + 1, 2 * (a + 1) + 1 + M, tile_rows(I)
    out = {"T": np.zeros((n, I), dtype=LD), "T_err": np.zeros((n, I)), "tm": np.zeros((I, n), dtype=LD), "tout": [],
           "part": np.zeros((n, len(tiles), nv), dtype=LD), "part_err": np.zeros((n, len(tiles), nv)), "nv": nv}
    for k in range(n):
        vec = st["vec"][k]
        mw, g = vec[3 * R + M + 1], vec[2 * R + M + 1:2 * R + M + 1 + a]
        Tp = st["T"][k][:, :a]
        t = sc[:, k].astype(LD) - LD(mw) - Tp.astype(LD) @ g.astype(LD)
        # sc - mw rounds once, every fused T g once more: a + 2 terms, each through at most a + 1 roundings
        out["T"][k], out["T_err"][k] = t, bound_sum(a + 2, np.abs(sc[:, k]) + abs(mw) + np.abs(Tp) @ np.abs(g))
        train, w = training(lay, st["fold_of"], k)
        t64 = t.astype(np.float64) if t_dev is None else t_dev[k]
        tt = np.where(train, w.astype(LD) * t64.astype(LD), LD(0))               # the kernel's tm, one rounding (c t)
        out["tm"][:, k] = tt
        slot = tout_slot(lay, k)
        if slot is not None:
            out["tout"].append((slot, np.flatnonzero(~train), k))
        Tk = np.where(train[:, None], np.concatenate([Tp, t64[:, None]], axis=1), 0.0)   # T_train[:, :kk]
        Y, q = st["Yk"][k], st["Q"][k, a]
        u = np.where(train, w.astype(LD) * (Y.astype(LD) @ q.astype(LD)), LD(0))
        umag = np.where(train, w * (np.abs(Y) @ np.abs(q)), 0.0)
        ty = tt if lay.mode == WEIGHTED else t64.astype(LD)                       # Yk^T t runs over every row but weighted
        vals = np.concatenate([Tk.astype(LD) * tt[:, None], Tk.astype(LD) * u[:, None], tt[:, None], Y.astype(LD) * ty[:, None]], axis=1)
        att = np.abs(tt.astype(np.float64))
        mags = np.concatenate([np.abs(Tk) * att[:, None], np.abs(Tk) * umag[:, None], att[:, None],
                               np.abs(Y) * np.abs(ty.astype(np.float64))[:, None]], axis=1)
        for ti, (lo, hi) in enumerate(tiles):
            m = hi - lo
            # flattened sums over the tile's m rows: T t and 1^T t and Y t pass the rounding of c t and m additions (chain m + 1);
            # a term T c Y q of T^T u passes M fused additions, c *, T * and m additions (chain m + M + 2)
            ch = np.concatenate([np.full(kk, m + 1), np.full(kk, m + M + 2), np.full(1 + M, m + 1)])
            out["part"][k, ti] = vals[lo:hi].sum(axis=0)
            out["part_err"][k, ti] = np.array([gamma(c) for c in ch]) * mags[lo:hi].sum(axis=0) * REF_SLACK
    return out


def apply_rows(st, a, out):
    n = st["T"].shape[0]
    st["T"][:, :, a] = out["T"].astype(np.float64)
    st["tm"][:, :] = out["tm"].astype(np.float64)
    for slot, held, k in out["tout"]:
        st["Tout"][slot, held, a] = out["T"][k, held].astype(np.float64)
    st["part"][:, :, :out["nv"]] = out["part"].astype(np.float64)
    return n


# ---- stage 1b: kfold_solve_kernel ---------------------------------------------------------------------------------------------
def tile_totals(part, nv):
    """The kernel's own additions: s = 0.0; s += part[tile] in tile order, in float64 (every one correctly rounded)."""
    tot = np.zeros((part.shape[0], nv))
    for t in range(part.shape[1]):
        tot = tot + part[:, t, :nv]
    return tot


def solve(st, a, b_dev=None):
    """From st['part'] and the earlier rows of st['Gt'].  Returns a dict: tot (n, nv) float64 (equal on the device); G (n, kk, kk),
    g (n, kk) float64, the system; ref [solve_ref.NormalRef], the long-double solve; b_serial (n, kk) and dropped, csrc/
    fold_regress.hpp's operations in float64 (the branch decisions); c (n, kk) = Gt b with c_err, b the device's `b_dev` (n, kk)
    where given, else round(ref.b); bad (n,) bool: status bit 2."""
    n, I, M, R = dims(st)
    kk, nv = a + 1, 2 * (a + 1) + 1 + M
    tot = tile_totals(st["part"], nv)
    out = {"tot": tot, "G": np.zeros((n, kk, kk)), "g": tot[:, kk:2 * kk].copy(), "ref": [], "b_serial": np.zeros((n, kk)),
           "dropped": [], "c": np.zeros((n, kk), dtype=LD), "c_err": np.zeros((n, kk)), "bad": np.zeros(n, dtype=bool), "nv": nv}
    for k in range(n):
        G = st["Gt"][k][:kk, :kk].copy()
        G[a, :] = tot[k, :kk]
        G[:, a] = tot[k, :kk]
        out["G"][k] = G
        with np.errstate(all="ignore"):
            bs, dropped = SA.fold_normal_solve(G.tolist(), out["g"][k].tolist())
            ref = SR.normal_solve(G, out["g"][k])
        out["b_serial"][k] = bs
        out["ref"].append(ref)
        out["dropped"].append(dropped)
        b = np.asarray(b_dev[k], dtype=np.float64) if b_dev is not None else ref.b.astype(np.float64)
        with np.errstate(all="ignore"):
            out["c"][k] = G.astype(LD) @ b.astype(LD)
            out["c_err"][k] = bound_sum(kk, np.abs(G) @ np.abs(b))                # kk fused terms
        out["bad"][k] = not (math.isfinite(bs[a]) and math.isfinite(tot[k, 2 * kk]))
    return out


def apply_solve(st, a, out, b=None):
    n, I, M, R = dims(st)
    kk = a + 1
    for k in range(n):
        bk = out["ref"][k].b.astype(np.float64) if b is None else b[k]
        st["Gt"][k, a, :kk] = out["tot"][k, :kk]
        st["Gt"][k, :kk, a] = out["tot"][k, :kk]
        st["coef"][k, :kk, a] = bk
        st["vec"][k, :kk] = bk
        st["vec"][k, R:R + kk] = out["c"][k].astype(np.float64)
        st["vec"][k, 2 * R:2 * R + M] = out["tot"][k, 2 * kk + 1:2 * kk + 1 + M]
        st["vec"][k, 2 * R + M] = out["tot"][k, 2 * kk]
        if out["bad"][k]:
            st["status"][k] |= 2


def composed_residual(ref_dev, b_dev, d, eG, eg):
    """(|D (G b - g)| of the RESTATED system on the device's kept columns, its bound) -- see the module docstring.  ref_dev: the
    NormalRef of the device's own system; d: the restated system's equilibration; eG, eg: the bounds of the device's system."""
    K = ref_dev.kept
    _, bt = SR.normal_solve_bound(ref_dev, b_dev)
    ab = np.abs(np.asarray(b_dev, dtype=np.float64))
    dk = d[K].astype(np.float64)
    ratio = dk / ref_dev.d[K].astype(np.float64)
    return K, ratio * bt + dk * ((eG[np.ix_(K, K)] @ ab[K]) + eg[K]) * REF_SLACK


# ---- stage 0 / 1c: kfold_ydefl_kernel -------------------------------------------------------------------------------------------
def ydefl(lay, st, a, deflate, y_dev=None):
    """Returns a dict: Yk (n, I, M) long double with Yk_err (the rows that do not train a model unchanged, error 0), b = vec[:kk];
    Gy (n, NT, M, M) and Gy_err, the tiles' sums of c y y^T over round(Yk), or over the device's own `y_dev` where given."""
    n, I, M, R = dims(st)
    kk, tiles = a + 1, tile_rows(I)
    out = {"Yk": st["Yk"].astype(LD), "Yk_err": np.zeros((n, I, M)), "Gy": np.zeros((n, len(tiles), M, M), dtype=LD),
           "Gy_err": np.zeros((n, len(tiles), M, M))}
    for k in range(n):
        train, w = training(lay, st["fold_of"], k)
        if deflate:
            # small_algebra_ref.y_deflate: yh = T b in kk fused terms, y - yh q fused or not
            with np.errstate(all="ignore"):                                         # (a model marked bad carries NaN)
                V, ev, _ = SA.y_deflate(st["Yk"][k], st["T"][k], kk, st["vec"][k, :kk], st["Q"][k, a])
            out["Yk"][k][train] = V[train]
            out["Yk_err"][k][train] = ev[train]
        Y = out["Yk"][k].astype(np.float64) if y_dev is None else y_dev[k]
        cw = w if lay.mode == WEIGHTED else np.ones(I)                              # (held-out rows of Y_k are 0 in the workflow)
        for ti, (lo, hi) in enumerate(tiles):
            Yt, ct = Y[lo:hi], cw[lo:hi]
            out["Gy"][k, ti] = (Yt.astype(LD) * ct.astype(LD)[:, None]).T @ Yt.astype(LD)
            # hi - lo terms, weighted: one more rounding for y c
            out["Gy_err"][k, ti] = bound_sum(hi - lo + (lay.mode == WEIGHTED), (np.abs(Yt) * ct[:, None]).T @ np.abs(Yt))
    return out


def apply_ydefl(st, out):
    st["Yk"][:] = out["Yk"].astype(np.float64)
    st["Gy"][:] = out["Gy"].astype(np.float64)


# ---- stage 2: kfold_downdate_kernel ---------------------------------------------------------------------------------------------
def downdate(lay, st, a, rs):
    """Returns a dict: Rm (n, P) = rs - (1^T t) mean[row] with Rm_err; S (n, M, P) with S_err."""
    n, I, M, R = dims(st)
    P = st["S"].shape[2]
    out = {"Rm": np.zeros((n, P), dtype=LD), "Rm_err": np.zeros((n, P)), "S": np.zeros((n, M, P), dtype=LD), "S_err": np.zeros((n, M, P))}
    for k in range(n):
        vec = st["vec"][k]
        b, c, ya, s = vec[:a + 1], vec[R:R + a + 1], vec[2 * R:2 * R + M], vec[2 * R + M]
        mu = st["mean"][lay.model_fold[k] if lay.mode == GROUPED else k]
        r = rs[k].astype(LD) - LD(s) * mu.astype(LD)
        rmag = np.abs(rs[k]) + abs(s) * np.abs(mu)
        out["Rm"][k], out["Rm_err"][k] = r, bound_sum(2, rmag)                    # two terms, fused or not
        W = st["Wa"][k][:a + 1, :, None].astype(LD) * st["Wb"][k][:a + 1, None, :].astype(LD)
        W = W.reshape(a + 1, P)
        v = LD(b[a]) * r - c.astype(LD) @ W
        vmag = abs(b[a]) * rmag + np.abs(c) @ np.abs(W.astype(np.float64))
        if a:
            v = v + b[:a].astype(LD) @ st["Rm"][k][:a].astype(LD)
            vmag = vmag + np.abs(b[:a]) @ np.abs(st["Rm"][k][:a])
        q = st["Q"][k, a]
        out["S"][k] = st["S"][k].astype(LD) - (W[a][None, :] * ya.astype(LD)[:, None] + v[None, :] * q.astype(LD)[:, None])
        mag = np.abs(st["S"][k]) + np.abs(W[a].astype(np.float64))[None, :] * np.abs(ya)[:, None] + vmag[None, :] * np.abs(q)[:, None]
        # flattened: S, w ya, and 2a + 3 stored products under q; a term passes its own products (<= 3: s mean, b r, Wa Wb), the
        # 2a + 2 additions of v, v q, the fma with w ya and the subtraction from S: chain 2a + 8
        out["S_err"][k] = bound_sum(2 * a + 8, mag)
    return out


def apply_downdate(st, a, out):
    st["Rm"][:, a, :] = out["Rm"].astype(np.float64)
    st["S"][:] = out["S"].astype(np.float64)


# ---- kfold_combine_kernel ---------------------------------------------------------------------------------------------------
def combine(sc):
    """(mean over the nb leading slices in long double, bound, the kernel's own float64 operations in block order)."""
    return SA.scores_mean(sc)[0], SA.bound_scores_mean(sc), SA.scores_mean_f64(sc)


# ---- what a stage may write ---------------------------------------------------------------------------------------------------
def written(stage, lay, st, a):
    """{field: bool mask of its shape}: the elements stage `stage` of component a may write; a field that is not named is not
    written at all.  status is written only by |= 2."""
    n, I, M, R = dims(st)
    kk, nv = a + 1, 2 * (a + 1) + 1 + M
    z = lambda f: np.zeros(st[f].shape, dtype=bool)
    if stage == 0:
        return {"Gy": ~z("Gy")}
    if stage == 2:
        Rm = z("Rm")
        Rm[:, a, :] = True
        return {"Rm": Rm, "S": ~z("S")}
    m = {f: z(f) for f in ("T", "tm", "Tout", "part", "Gt", "coef", "vec", "status")}
    m["T"][:, :, a] = True
    m["tm"][:] = True
    m["part"][:, :, :nv] = True
    m["Gt"][:, a, :kk] = True
    m["Gt"][:, :kk, a] = True
    m["coef"][:, :kk, a] = True
    m["vec"][:, :kk] = True
    m["vec"][:, R:R + kk] = True
    m["vec"][:, 2 * R:2 * R + M + 1] = True
    m["status"][:] = True
    for k in range(n):
        slot = tout_slot(lay, k)
        if slot is not None:
            m["Tout"][slot, ~training(lay, st["fold_of"], k)[0], a] = True
    if a + 1 < R:
        m["Gy"] = ~z("Gy")
        m["Yk"] = z("Yk")
        for k in range(n):
            m["Yk"][k, training(lay, st["fold_of"], k)[0], :] = True
    return m


# ---- fold maps ------------------------------------------------------------------------------------------------------------------
MAPS = ["contiguous", "shuffled", "single"]


def fold_map(kind, I, F, rng, unit=1):
    """F folds over I rows, constant on aligned units of `unit` rows: contiguous runs; the same shuffled; or the last row alone as
    fold F - 1 and contiguous runs of the other folds before it."""
    last = 1 if kind == "single" else 0
    nf = F - last
    nu = (I - last) // unit
    assert nu >= nf >= 1, (I, F, unit)
    fu = np.arange(nu) * nf // nu
    if kind == "shuffled":
        fu = rng.permutation(fu)
    f = np.full(I, nf - 1, dtype=np.int32)                       # the rows past the last whole unit: the last contiguous fold
    f[:nu * unit] = np.repeat(fu, unit)
    if last:
        f[I - 1] = F - 1
    return f


def models_of(mode, K):
    """(models n, folds F) of a row-stage case with `K` in its shape: K models; grouped and split-major: 2 groups / splits of F
    folds with F = K, or K / 2 where 2 K models would pass the 32 of the device form."""
    if mode in (PLAIN, WEIGHTED):
        return K, K
    F = K if 2 * K <= 32 else K // 2
    return 2 * F, F


def layout(mode, kind, I, K, rng, unit=1):
    """(Layout, fold_of) of a case: grouped with groups = 2 (model m holds out fold m // 2), splits with 2 splits x F folds (two
    different maps), weighted with counts in 0 ... 3 constant on units -- "contiguous": four runs of equal counts, shifted by one
    from model to model; "shuffled": independent draws; "single": counts in 1 ... 3 and the last row alone with count 0, the
    bootstrap's form of a single held-out row -- and the first row tile of model 0 all 0 when there are more tiles than one."""
    n, F = models_of(mode, K)
    if mode == PLAIN:
        return Layout(mode, None, 1, 1), fold_map(kind, I, F, rng, unit)
    if mode == GROUPED:
        return Layout(mode, (np.arange(n) // 2).astype(np.int32), 2, 2), fold_map(kind, I, F, rng, unit)
    if mode == SPLITS:
        other = "shuffled" if kind != "shuffled" else "contiguous"
        return Layout(mode, None, F, 2), np.stack([fold_map(kind, I, F, rng, unit), fold_map(other, I, F, rng, unit)])
    nu = -(-I // unit)
    if kind == "contiguous":
        cu = (np.arange(nu)[None, :] * 4 // nu + np.arange(n)[:, None]) % 4
    elif kind == "shuffled":
        cu = rng.integers(0, 4, size=(n, nu))
    else:
        cu = rng.integers(1, 4, size=(n, nu))
    c = np.repeat(cu, unit, axis=1)[:, :I].astype(np.int32)
    if kind == "single":
        c[:, I - 1] = 0
    tiles = tile_rows(I)
    if len(tiles) > 1:
        c[0, :tiles[0][1]] = 0
        if unit > 1:                                              # keep the counts constant on the unit the tile's end cuts
            c[0, :-(-tiles[0][1] // unit) * unit] = 0
    for k in range(n):                                            # every model trains on something
        if not (c[k] > 0).any():
            c[k, -unit:] = 1
    return Layout(mode, None, 1, 1), c


# ---- states -----------------------------------------------------------------------------------------------------------------------
def empty_state(n, I, M, R, A, B, slots, fold_of, mean_rows=None):
    """Every field the sentinel; status and n_iter 0."""
    NT, P = kf_tiles(I), A * B
    f = lambda *s: np.full(s, SENTINEL)
    return {"fold_of": np.ascontiguousarray(fold_of, dtype=np.int32), "Yk": f(n, I, M), "Gy": f(n, NT, M, M), "Q": f(n, R, M),
            "T": f(n, I, R), "Gt": f(n, R, R), "coef": f(n, R, R), "tm": f(I, n), "Tout": f(slots, I, R), "vec": f(n, vec_len(R, M)),
            "n_iter": np.zeros((n, R), dtype=np.int32), "status": np.zeros(n, dtype=np.int32), "part": f(n, NT, PART_STRIDE),
            "S": f(n, M, P), "mean": f(mean_rows or n, P), "WA": f(A, n), "WB": f(B, n), "Wa": f(n, R, A), "Wb": f(n, R, B),
            "Rm": f(n, R, P)}


def copy_state(st):
    return {f: v.copy() for f, v in st.items()}


def _pow4_at_most(x):
    p = 1
    while p * 4 <= x:
        p *= 4
    return p


def row_state(kind, mode, map_kind, I, M, K, R, a, seed=0, special=None):
    """(Layout, state, sc, solve_exact): the inputs of stage 1 for component a -- T[:, :a], the training Gram of those columns in Gt,
    g and mu^T w in vec, Q[:, a], Yk (zero on a model's held-out rows, as the workflow keeps it, but for weighted models), sc --
    every other element the sentinel, status[n - 1] = 1.  kind "exact" / "rounding": the module docstring.  special = {model:
    "zero" | "double"}: the model's new column identically zero on its training rows / exactly twice column 0."""
    special = special or {}
    rng = np.random.default_rng([23, MODES.index(mode), MAPS.index(map_kind), I, M, K, R, a, seed, int(kind == "exact")])
    exact = kind == "exact"
    unit = 1 << max(0, (R - 1).bit_length()) if exact else 1
    unit = min(unit, 1 << 30)
    lay, fold_of = layout(mode, map_kind, I, K, rng, unit)
    n = models_of(mode, K)[0]
    st = empty_state(n, I, M, R, 1, 1, lay.slots, fold_of)
    st["status"][n - 1] = 1
    sc = np.zeros((I, n))
    solve_exact = exact
    for k in range(n):
        train, w = training(lay, fold_of, k)
        vec = st["vec"][k]
        if exact:
            T, new = np.zeros((I, a)), np.zeros(I)
            e = rng.integers(-1, 2, size=a + 1)
            H = SR.hadamard_columns(unit, a + 1) * 2.0 ** e[None, :]
            whole = [u0 for u0 in range(0, I - unit + 1, unit) if len(set(zip(train[u0:u0 + unit], w[u0:u0 + unit]))) == 1]
            trn = [u0 for u0 in whole if train[u0]]
            avail = sum(int(w[u0]) * unit for u0 in trn)
            target, acc, keep = (_pow4_at_most(avail) if avail else 0), 0, [u0 for u0 in whole if not train[u0]]
            for u0 in sorted(trn, key=lambda v: -w[v]):          # non-zero training units up to a power of 4 of weighted rows,
                if acc + int(w[u0]) * unit <= target:            # the heaviest first so that the lighter ones can fill the rest
                    acc += int(w[u0]) * unit
                    keep.append(u0)
            solve_exact = solve_exact and acc == target and target > 0
            for u0 in keep:
                T[u0:u0 + unit], new[u0:u0 + unit] = H[:, :a], H[:, a]
            g = rng.integers(-2, 3, size=a).astype(np.float64)
            mw = float(rng.integers(-8, 9))
            Y = rng.integers(-1, 2, size=(I, M)).astype(np.float64)
            q = np.zeros(M)                                      # at most two entries of +-1: |u| <= 6 (see the module docstring)
            q[0] = 1.0
            if M > 1:
                q[rng.integers(1, M)] = float(rng.choice([-1.0, 1.0]))
        else:
            scale = np.logspace(0, -3, R)
            T, new = rng.normal(size=(I, a)) * scale[None, :a], rng.normal(size=I) * scale[a]
            g, mw = 0.1 * rng.normal(size=a), float(rng.normal())
            Y = rng.normal(size=(I, M)) * np.logspace(0, -2, M)[None, :]
            q = rng.normal(size=M)
            q /= np.linalg.norm(q)
            ntr = int(train.sum())                               # fewer training rows than columns (the other model of a single-row
            T[np.ix_(train, np.arange(a) >= ntr)] = 0.0          # fold when K = 2): the columns past the rank are exactly zero on
            if a >= ntr:                                         # them, so they drop with a pivot of exactly 0, not of rounding noise
                new[train], g, mw = 0.0, np.zeros(a), 0.0        # (g = 0 and mu^T w = 0: t = sc, exactly 0 there)
        if special.get(k) == "zero":
            new = np.where(train, 0.0, new)
        if special.get(k) == "double":
            assert a >= 1
            new = 2.0 * T[:, 0]
        if mode != WEIGHTED:
            Y[~train] = 0.0
        sck = (new.astype(LD) + LD(mw) + T.astype(LD) @ g.astype(LD)).astype(np.float64)
        if exact:
            assert np.array_equal(sck.astype(LD) - LD(mw) - T.astype(LD) @ g.astype(LD), new.astype(LD))
        sc[:, k] = sck
        st["T"][k][:, :a] = T
        Tw = T * (w * train)[:, None]
        st["Gt"][k][:a, :a] = Tw.T @ T
        vec[2 * R + M + 1:2 * R + M + 1 + a], vec[3 * R + M + 1] = g, mw
        st["Q"][k, a], st["Yk"][k] = q, Y
    return lay, st, sc, solve_exact


def downdate_state(kind, grouped, A, B, M, R, a, seed=0):
    """(Layout, state, rs): n = 4 models (grouped: 2 folds x 2 groups, `mean` has 2 rows and model m reads row m // 2), I = 8 rows;
    the fields stage 2 reads (vec's b, c, ya, 1^T t; Q[:, a]; Wa, Wb and Rm up to a; S; mean) inputs of `kind`, the rest sentinel."""
    n, I, P = 4, 8, A * B
    rng = np.random.default_rng([29, A, B, M, R, a, seed, int(grouped), int(kind == "exact")])
    lay = Layout(GROUPED, (np.arange(n) // 2).astype(np.int32), 2, 2) if grouped else Layout(PLAIN, None, 1, 1)
    st = empty_state(n, I, M, R, A, B, lay.slots, np.arange(I) % (2 if grouped else n), mean_rows=2 if grouped else n)
    inp = lambda *s: SA.inputs(kind, rng, *s)
    st["vec"][:, :a + 1], st["vec"][:, R:R + a + 1], st["vec"][:, 2 * R:2 * R + M + 1] = inp(n, a + 1), inp(n, a + 1), inp(n, M + 1)
    st["Q"][:, a], st["Wa"][:, :a + 1], st["Wb"][:, :a + 1] = inp(n, M), inp(n, a + 1, A), inp(n, a + 1, B)
    st["Rm"][:, :a], st["S"][:], st["mean"][:] = inp(n, a, P), inp(n, M, P), inp(*st["mean"].shape)
    return lay, st, inp(n, P)


def composed_system(lay, st, a, r, k):
    """Model k's normal equations restated from the original inputs (r = rows(lay, st, a, sc), no device column), (G, g) rounded to
    float64, and (eG, eg): how far the device's tile-order totals may lie from them.  e = T_err + u |t| bounds the device's t
    against round(t).  A total differs by its tiles' part_err and NT additions (gamma_NT sum |part|), by the change of t inside it
    -- sum |T_p| w e for p < a, sum w (2 |t| e + e^2) for p = a, sum |u| e for g_a, each times 1 + gamma_(I + M + 2) for the
    magnitudes part_err was formed at -- and by u |G| for the rounding of the restated value.  The earlier a x a block of G is the
    state's own."""
    n, I, M, R = dims(st)
    kk = a + 1
    train, w = training(lay, st["fold_of"], k)
    t = np.abs(r["T"][k].astype(np.float64))
    e = r["T_err"][k] + U * t
    NT = r["part"].shape[1]
    tot = r["part"][k].sum(axis=0)
    etot = r["part_err"][k].sum(axis=0) + gamma(NT) * np.abs(r["part"][k].astype(np.float64)).sum(axis=0) * REF_SLACK
    wt = w * train
    Tp = np.abs(st["T"][k][:, :a])
    Y, q = st["Yk"][k], st["Q"][k, a]
    umag = wt * (np.abs(Y) @ np.abs(q))
    dG = np.concatenate([(Tp * (wt * e)[:, None]).sum(axis=0), [float((wt * (2 * t * e + e * e)).sum())]])
    dg = np.concatenate([np.zeros(a), [float((umag * e).sum())]])
    grow = 1 + gamma(I + M + 2)
    G = st["Gt"][k][:kk, :kk].copy()
    G[a, :] = G[:, a] = tot[:kk].astype(np.float64)
    g = tot[kk:2 * kk].astype(np.float64)
    eG = np.zeros((kk, kk))
    eG[a, :] = eG[:, a] = etot[:kk] + dG * grow + U * np.abs(G[a, :])
    eg = etot[kk:2 * kk] + dg * grow + U * np.abs(g)
    return G, g, eG, eg


# ---- case tables (shared by the CPU check of the builder conditions and the GPU tests) --------------------------------------------
# (I, M, K, R, a): the smallest shapes at which each path of the row kernels exists
ROW_CASES = [(5, 1, 2, 1, 0)] + [(257, 3, 3, 4, a) for a in (0, 1, 3)] + [(777, 17, 5, 3, a) for a in (0, 2)] + [(300, 16, 32, 2, 1)] + \
            [(600, 64, 2, 64, a) for a in (0, 62, 63)] + [(32769, 2, 2, 2, 1), (70001, 4, 3, 3, 2)]
DOWNDATE_AB = [(1, 30), (16, 16), (33, 40), (257, 1)]
DOWNDATE_R, DOWNDATE_M = 4, 3
COMBINE_CASES = [(nb, n) for nb in (1, 2, 3, 8) for n in (1, 255, 257)]
COMBINE_STRIDE_CASE = (2, 65536 * 256 + 3)                    # past the grid cap of 65536 workgroups of 256: the stride loop


def row_stage_cases():
    """(I, M, K, R, a, mode, map): every shape in every mode with each of the three fold maps."""
    return [shape + (mode, m) for shape in ROW_CASES for mode in MODES for m in MAPS]
