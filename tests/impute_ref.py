"""NumPy float64 restatement of csrc/impute.hip and of validate.impute / get_q2x_heldout -- TEST INFRASTRUCTURE.

The hold-out rule goes through philox_ref.philox4x32_10 (stream 2 + block), independently of the package's own restatement
(cmtf_pls_amd.imputation.holdout_mask_host); the three kernels are plain array expressions; the error bounds are the ones the
kernels are held to."""
import numpy as np

from philox_ref import MASK, philox4x32_10

EPS53 = 2.0 ** -53


def holdout_mask(first, n, seed, stream, fraction):
    """(n,) bool for the global elements first .. first + n - 1: unit_open(word (first + e) % 4 of block (first + e) / 4) < fraction."""
    q0, q1 = first // 4, (first + n + 3) // 4
    ctr = np.arange(q0, q1, dtype=np.uint64)
    v = philox4x32_10((ctr & MASK).astype(np.uint32), (ctr >> np.uint64(32)).astype(np.uint32), np.full(len(ctr), stream, np.uint32),
                      np.zeros(len(ctr), np.uint32), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = (np.stack(v, axis=1).reshape(-1).astype(np.float64) + 0.5) * 2.3283064365386963e-10
    s = first - 4 * q0
    return u[s:s + n] < fraction


def masked_copy(X, fraction, seed, block=0, offset=0):
    """kernel (a): (out, [entries newly hidden, finite entries left]) for the array X in its own dtype."""
    held = holdout_mask(offset, X.size, seed, 2 + block, fraction).reshape(X.shape)
    fin = np.isfinite(X)
    out = X.copy()
    out[held] = np.nan
    return out, [int((held & fin).sum()), int((~held & fin).sum())]


def _terms(T, WA, WB):
    """(I, P, R): t_a w_a per entry and component, W[c, a] = WA[c / B, a] WB[c % B, a]."""
    W = (WA[:, None, :] * WB[None, :, :]).reshape(-1, WA.shape[1])
    return T[:, None, :] * W[None, :, :]


def heldout_sums(X, T, WA, WB, mean, fraction, seed, block=0, offset=0):
    """kernel (b): (out (R + 2,), bound) with out = [sum (x - xhat_r)^2 for r = 1..R, sum (x - mean)^2, count] over the held-out
    finite entries of X (I, P), and bound = (n + 2R + 8) 2^-53 sum_held (|x| + |mean| + sum_a |t_a w_a|)^2, n the count."""
    I, P = X.shape
    R = T.shape[1]
    x = X.astype(np.float64)
    use = holdout_mask(offset, x.size, seed, 2 + block, fraction).reshape(I, P) & np.isfinite(x)
    terms = _terms(T, WA, WB)
    xhat = mean[None, :, None] + np.cumsum(terms, axis=2)
    xs = np.where(use, x, 0.0)
    d = np.where(use[:, :, None], xs[:, :, None] - xhat, 0.0)
    out = np.empty(R + 2)
    out[:R] = (d * d).sum(axis=(0, 1))
    out[R] = (np.where(use, xs - mean[None, :], 0.0) ** 2).sum()
    n = int(use.sum())
    out[R + 1] = n
    size = np.abs(xs) + np.abs(mean)[None, :] + np.abs(terms).sum(axis=2)
    bound = (n + 2 * R + 8) * EPS53 * float((np.where(use, size, 0.0) ** 2).sum())
    return out, bound


def imputed(X, T, WA, WB, mean):
    """kernel (c): (want (I, P) float64 = xhat_R, gap = ~isfinite(X), tol (I, P)) with tol = 2^-24 |want| (f32 storage only: the
    one rounding) + (R + 2) 2^-53 (|mean| + sum_a |t_a w_a|)."""
    R = T.shape[1]
    terms = _terms(T, WA, WB)
    want = mean[None, :] + terms.sum(axis=2)
    tol = (R + 2) * EPS53 * (np.abs(mean)[None, :] + np.abs(terms).sum(axis=2))
    if X.dtype == np.float32:
        tol = tol + 2.0 ** -24 * np.abs(want)
    return want, ~np.isfinite(X), tol


# ---- the public functions as a literal host loop -------------------------------------------------------------------------------
def literal_q2x(make_model, X, Y, R, fraction, seeds, tol=1e-8, max_iter=100):
    """get_q2x_heldout as a loop: per seed mask every block on the host, fit make_model() on the masked arrays, take
    X_reconstructed() (the first r columns of the factors for r < R) and form the sums in NumPy.
    Returns (sums (n_repeats, n_blocks, R + 2), q2x, q2x_all, bounds (n_repeats, n_blocks)): bounds[g, b] is the bound of
    `heldout_sums` (kernel check 2) for that repeat's refit and block, i.e. how far any conforming form of the sums may lie from
    their exact values."""
    from cmtf_pls_amd.util import factors_to_tensor

    coupled = isinstance(X, list)
    Xs = X if coupled else [X]
    sums = np.empty((len(seeds), len(Xs), R + 2))
    bounds = np.empty((len(seeds), len(Xs)))
    for g, seed in enumerate(int(s) for s in seeds):
        held = [holdout_mask(0, x.size, seed, 2 + b, fraction).reshape(x.shape) for b, x in enumerate(Xs)]
        masked = [np.where(h, np.nan, x) for h, x in zip(held, Xs)]
        m = make_model()
        m.fit(masked if coupled else masked[0], Y, tol=tol, max_iter=max_iter)
        factors = m.Xs_factors if coupled else [m.X_factors]
        means = m.Xs_mean if coupled else [m.X_mean]
        full = m.Xs_reconstructed() if coupled else [m.X_reconstructed()]
        for b, (x, h) in enumerate(zip(Xs, held)):
            use = h & np.isfinite(x)
            for r in range(1, R + 1):
                xhat = full[b] if r == R else factors_to_tensor([f[:, :r] for f in factors[b]]) + means[b]
                sums[g, b, r - 1] = ((x - xhat)[use] ** 2).sum()
            sums[g, b, R] = ((x - means[b])[use] ** 2).sum()
            sums[g, b, R + 1] = use.sum()
            loads = factors[b][1:]
            WA = loads[0] if len(loads) > 1 else np.ones((1, R))
            WB = loads[-1] if len(loads) <= 2 else loads[1]
            for L in loads[2:]:
                WB = (WB[:, None, :] * L[None, :, :]).reshape(-1, R)
            bounds[g, b] = heldout_sums(x.reshape(x.shape[0], -1), factors[b][0], WA, WB, np.asarray(means[b]).reshape(-1), fraction,
                                        seed, block=b)[1]
    q2x = 1.0 - sums[:, :, :R] / sums[:, :, R:R + 1]
    pooled = sums.sum(axis=1)
    return sums, q2x, 1.0 - pooled[:, :R] / pooled[:, R:R + 1], bounds
