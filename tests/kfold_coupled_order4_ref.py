"""NumPy float64 restatement of the coupled fold loop (csrc/kfold.hip: kfold_inner_coupled_kernel, cmtf.py:88-128 as the kernel
states it) for blocks of order 2, 3 and 4 (TEST INFRASTRUCTURE): the inner loop of one component over several blocks' cross-
covariances S_b (M x P_b) and a shared G_y, every block's extraction by oracle.nipals_oracle.rank1_factors, as oracle.fit_ctpls
does.  Shared by tests/test_kfold_coupled_order4_cpu.py, tests/test_gpu_kfold_coupled_order4_kernel.py and
tests/test_gpu_kfold_coupled_order4.py."""
import numpy as np

import oracle as O
from kfold_order4_ref import planted
from oracle.nipals_oracle import rank1_factors


def trailing(dims):
    """The trailing shape of the block that a test names (A, B1, B2) (order 4), (A, B) (order 3) or (1, B) (order 2: a vector)."""
    return tuple(dims[1:]) if len(dims) == 2 and dims[0] == 1 else tuple(dims)


def view(dims):
    """(A, B) of the I x A x B view the passes take of that block."""
    return (dims[0], int(np.prod(dims[1:])))


def coupled_inner_loop(Ss, Gy: np.ndarray, dims, tol: float = 1e-8, max_iter: int = 100) -> dict:
    """cmtf.py:88-128 on S_b = Y^T X_b (M x P_b) and G_y = Y^T Y: from q = e_0 (u = Y[:, 0]); per pass and block Z_b = S_b^T q and
    its rank-1 factors, tq = sum_b S_b w_b / nb (added in block order), q = tq / |tq|, until sqrt(dq^T G_y dq) < tol (never on the
    first pass) or max_iter passes.  Returns `blocks` (per block its mode loadings in the order of the modes, and their Kronecker
    product w), q and n_iter (the passes executed)."""
    M = Ss[0].shape[0]
    nb = len(Ss)
    q = np.zeros(M)
    q[0] = 1.0
    n_iter = 0
    blocks = [None] * nb
    for it in range(max_iter):
        n_iter = it + 1
        tq = np.zeros(M)
        for b, (S, d) in enumerate(zip(Ss, dims)):
            fac = rank1_factors((S.T @ q).reshape(trailing(d)), tol)           # X_b x_0 u = S_b^T q
            w = fac[-1]
            for f in fac[-2::-1]:                                                # wA (x) (wK (x) wL), as the kernel multiplies
                w = np.kron(f, w)
            blocks[b] = {"modes": fac, "w": w}
            tq = tq + S @ w                                                      # Y^T t_b = S_b w_b
        tq = tq / nb
        qn = tq / np.linalg.norm(tq)
        dq = qn - q
        d2 = float(dq @ Gy @ dq)                                                 # |u_old - u|^2
        q = qn
        if it > 0 and np.sqrt(max(d2, 0.0)) < tol:
            break
    return {"blocks": blocks, "q": q, "n_iter": n_iter}


def planted_blocks(dims, M: int, K: int, seed: int):
    """K models' S_b (K x M x P_b) per block by kfold_order4_ref.planted (a block of another order as A x B x 1 there: the same
    numbers, P_b columns), and the G_y of the first block's draw."""
    Ss, Gy = [], None
    for b, d in enumerate(dims):
        S, G = planted((tuple(d) + (1,))[:3], M, K, seed + 17 * b)
        Ss.append(S)
        Gy = G if Gy is None else Gy
    return Ss, Gy


def coupled_data(shapes, M: int, L: int, seed: int, error: float = 0.3):
    """Blocks sharing L latent scores and a Y of M responses (the _coupled_data of tests/test_gpu_kfold_coupled.py)."""
    rng = np.random.default_rng(seed)
    I = shapes[0][0]
    T = rng.standard_normal((I, L))
    Xs = [O.cp_factors_to_tensor([T] + [rng.standard_normal((d, L)) for d in shape[1:]]) + error * rng.standard_normal(shape)
          for shape in shapes]
    Y = T @ rng.standard_normal((L, M)) + error * rng.standard_normal((I, M))
    return Xs, Y


def oracle_fold_predictions(Xs, y, ids, K: int, R: int):
    """(pred (R, I, M), n_iter K x R) from oracle.fit_ctpls refits of every fold: pred[r - 1] with the first r components."""
    pred = np.zeros((R,) + y.shape)
    n_iter = []
    for k in range(K):
        test = ids == k
        fit = O.fit_ctpls([X[~test] for X in Xs], y[~test], R)
        s = O.transform(fit, [X[test] for X in Xs])
        for r in range(1, R + 1):
            pred[r - 1, test] = (s[:, :r] @ fit.coef[:r, :r]) @ fit.Q[:, :r].T + fit.y_mean
        n_iter.append(list(fit.n_iter))
    return pred, n_iter
