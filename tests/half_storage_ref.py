"""16-bit storage of X (bfloat16 / float16) -- TEST INFRASTRUCTURE ONLY (no backend; NumPy and torch on the host).

The 16-bit kernels convert every stored element to float64 on load, exactly, and from there on run the float64 arithmetic of the
f32 / f64 kernels.  A reference therefore needs nothing new: quantise the data on the host, upcast it to float64 (exact), and
hand the upcast values to the existing restatements and bounds (matrix_core_ref.f64_bound, score_contract_ref.reference), which
depend on the float64 accumulation only.

  quantise(x, kind)      float64 array -> (torch tensor of the 16-bit type holding round-to-nearest-even(x), its exact float64 upcast)
  xcov_reference         S = Y^T X, the column sums / sums of squares, and sum|terms| of each, in float64 on the upcast values
  mttkrp_reference       M = X (WA (.) WB) and sum|terms|
  window(kind)           the rows form of cmtfpls_score_contract_{bf16,f16}: (vector, smallest P, largest P)
"""
import numpy as np
import torch

KINDS = ("bf16", "f16")
TORCH = {"bf16": torch.bfloat16, "f16": torch.float16}
NAMES = {"bf16": "bfloat16", "f16": "float16"}
SIGNIFICAND_BITS = {"bf16": 8, "f16": 11}          # with the implicit bit
VECTOR = 8                                          # elements per 16-byte vector
SC_STRIDE = 1024 * VECTOR                           # elements one 1024-thread workgroup covers with one vector per lane
SC_MIN_P, SC_MAX_P = SC_STRIDE // 2, 2 * SC_STRIDE  # NV in {1, 2}


def quantise(x, kind):
    """(q, up): q = x rounded ONCE to the 16-bit type (to nearest, ties to even), up = q as float64, exactly.  Independent of the
    package's cast: float16 by NumPy's astype; bfloat16 by rounding the 8-bit significand in float64 arithmetic (exact; values in
    bfloat16's normal range), whose result torch then only re-labels.  torch's own float64 -> 16-bit cast goes through float32
    and rounds twice."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if kind == "f16":
        q = torch.from_numpy(x.astype(np.float16))
    else:
        fin = np.isfinite(x) & (x != 0.0)
        assert np.all(np.abs(x[fin]) > 2.0 ** -120) and np.all(np.abs(x[fin]) < 2.0 ** 120)
        m, e = np.frexp(np.where(fin, x, 1.0))
        r = np.where(fin, np.ldexp(np.rint(m * 256.0) / 256.0, e), x)              # m in [0.5, 1): m * 256 has 8 integer bits
        q = torch.from_numpy(r).to(torch.bfloat16)
        assert np.array_equal(q.to(torch.float64).numpy(), r, equal_nan=True)       # (the cast had nothing left to round)
    up = q.to(torch.float64).numpy()
    return q, up


def is_exact_upcast(up, kind):
    """Every finite value of `up` has at most the type's significand bits: frexp mantissa * 2^bits is an integer."""
    fin = np.isfinite(up)
    m, _ = np.frexp(up[fin])
    scaled = m * float(2 ** SIGNIFICAND_BITS[kind])
    return bool(np.all(scaled == np.rint(scaled)))


def xcov_reference(up, Y):
    """S (M, P), sums (P,), sumsq (P,) and the magnitudes sum|terms| of each, float64 on the upcast X (I, P) and Y (I, M)."""
    ax = np.abs(up)
    return {"S": Y.T @ up, "magS": np.abs(Y).T @ ax, "sum": up.sum(axis=0), "magsum": ax.sum(axis=0),
            "sq": (up * up).sum(axis=0)}


def mttkrp_reference(up, A, B, WA, WB):
    """M = X (WA (.) WB) (I, R) and sum|terms|."""
    R = WA.shape[1]
    W = (WA[:, None, :] * WB[None, :, :]).reshape(A * B, R)
    return up @ W, np.abs(up) @ np.abs(W)


def window(kind):
    assert kind in KINDS
    return VECTOR, SC_MIN_P, SC_MAX_P


# ---- the models of tests/test_gpu_half_fit.py --------------------------------------------------------------------------------
FIT_R, FIT_M, FIT_LATENT, FIT_NEW = 4, 3, 4, 64
FIT_MODELS = {                      # name -> shapes of the blocks (one: tPLS; two: ctPLS)
    "one-read": [(300, 16, 256)],
    "two-read": [(300, 12, 20)],
    "matrix": [(300, 40)],
    "order-4": [(120, 6, 4, 8)],
    "coupled": [(300, 16, 256), (300, 24)],
}


FIT_DECAY, FIT_NOISE = {"coupled": 1.0 / 4.0}, 1e-4          # scale ratio of successive components (default 1/8)


def fit_data(name, seed):
    """(blocks, y, new rows per block) in float64, not yet quantised.  A rank-4 CP tensor plus a little noise whose components
    have scales 1, 1/8, 1/64, 1/512 (the coupled model: 1, 1/4, 1/16, 1/64 -- its matrix block's fourth component would otherwise
    sit below the quantisation noise, where the float64 engine itself differs from the oracle by 1e-9) on orthogonal sample-mode factors; Y = the same scaled factors through an orthogonal 3 x 4
    map.  Well separated components make the inner loop converge by more than 100 x per iteration, which is what lets a seed
    satisfy `convergence_is_clear`; a second block shares the sample-mode factor (coupled data)."""
    from oracle.synthetic_oracle import _cp_dense

    shapes = FIT_MODELS[name]
    rng = np.random.default_rng(seed)
    I, L = shapes[0][0], FIT_LATENT
    scale = FIT_DECAY.get(name, 1.0 / 8.0) ** np.arange(L)
    T = np.linalg.qr(rng.normal(size=(I, L)))[0] * np.sqrt(I) * scale
    tn = rng.normal(size=(FIT_NEW, L)) * scale
    Qy = np.linalg.qr(rng.normal(size=(L, L)))[0][:FIT_M]
    y = T @ Qy.T + rng.normal(0, FIT_NOISE, size=(I, FIT_M))
    blocks, new = [], []
    for shape in shapes:
        modes = [rng.normal(size=(d, L)) for d in shape[1:]]
        blocks.append(_cp_dense([T] + modes) + rng.normal(0, FIT_NOISE, size=shape))
        new.append(_cp_dense([tn] + modes) + rng.normal(0, FIT_NOISE, size=(FIT_NEW,) + tuple(shape[1:])))
    return blocks, y, new


def oracle_fit_with_norms(blocks, y, R, tol=1e-8):
    """(OracleFit, per component the convergence norms |u_old - u| of its iterations after the first): the oracle unchanged, with
    numpy.linalg.norm watched for its calls on vectors of the sample count (only tpls.py:103 takes such a norm)."""
    import oracle as O

    I = blocks[0].shape[0]
    assert all(I not in b.shape[1:] and I != int(np.prod(b.shape[1:])) for b in blocks) and I != y.shape[1]
    seen = []
    real = np.linalg.norm

    def watching(a, *args, **kw):
        v = real(a, *args, **kw)
        if not args and not kw and getattr(a, "shape", None) == (I,):
            seen.append(float(v))
        return v

    np.linalg.norm = watching
    try:
        with np.errstate(invalid="ignore"):
            fit = O.fit_ctpls(blocks, y, R, tol=tol) if len(blocks) > 1 else O.fit_tpls(blocks[0], y, R, tol=tol)
    finally:
        np.linalg.norm = real
    norms, it = [], iter(seen)
    for n in fit.n_iter:
        comp = [next(it) for _ in range(n)]
        norms.append(comp[1:])                                   # (the first pass compares against +inf)
    return fit, norms


def convergence_is_clear(fit, norms, tol=1e-8, max_iter=100):
    """No component's convergence norm lies within a factor 10 of tol at its stopping iteration or the one before."""
    for n, comp in zip(fit.n_iter, norms):
        if n >= max_iter or not comp or not comp[-1] < tol / 10:
            return False
        if len(comp) > 1 and not comp[-2] > tol * 10:
            return False
    return True
