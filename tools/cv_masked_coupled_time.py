#!/usr/bin/env python3
"""Cross-validated Q2Y of a ctPLS (tensor + matrix) with 10 % missing values in every block: the whole public call
(validate.get_q2y_kfold) with EngineOptions.masked_folds_coupled off (the default: one refit per fold on the regular engine) against
the same call with it on (every fold a workgroup of cmtfpls_cv_masked_coupled_f64).  K = I (leave-one-out), 5-fold and 10-fold, at
(200, 10, 8) + (200, 12) M = 4 R = 3 and at a serology-sized (300, 24, 40) + (300, 40) M = 2 R = 3.  One process; every call is
warmed once, then timed three times: median and spread (max - min) are printed.  The K = I refits are timed on N folds
(kfold.refit_fold, the step the option-off call repeats per fold) and scaled; everything else is timed whole.
Usage: python tools/cv_masked_coupled_time.py [--refits N] [--loo-only]
--loo-only: fit the first shape and make ONE K = I call with the option on, nothing else -- for a kernel trace
(`rocprofv3 --kernel-trace --stats -- python tools/cv_masked_coupled_time.py --loo-only`: one cv_masked_coupled_kernel launch per chunk)."""
import contextlib, io, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmtf_pls_amd import ctPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.kfold import COUPLED_FORM, refit_fold
from cmtf_pls_amd.validate import get_q2y_kfold

n_refits = int(sys.argv[sys.argv.index("--refits") + 1]) if "--refits" in sys.argv else 24
OFF, ON = EngineOptions(), EngineOptions(masked_folds_coupled=True)
REPEATS = 3

OUT = sys.stdout
contextlib.redirect_stdout(io.StringIO()).__enter__()                        # the reference's "X has missing values" of every fit


def _data(I, trailing, M, L, seed):
    """Blocks (I, *trailing[b]) driven by one latent score, 10 % of every block missing, and Y (I, M)."""
    rng = np.random.default_rng(seed)
    T = rng.standard_normal((I, L))
    Xs = []
    for tr in trailing:
        X = np.einsum("il,jl->ijl", T, rng.standard_normal((int(np.prod(tr)), L)) if len(tr) == 1 else
                      np.einsum("jl,kl->jkl", rng.standard_normal((tr[0], L)), rng.standard_normal((tr[1], L))).reshape(-1, L)).sum(axis=2)
        X = X.reshape((I,) + tuple(tr)) + 0.1 * rng.standard_normal((I,) + tuple(tr))
        X[rng.random(X.shape) < 0.1] = np.nan
        Xs.append(X)
    return Xs, T @ rng.standard_normal((L, M)) + 0.1 * rng.standard_normal((I, M))


def _timed(fn, repeats=REPEATS):
    """(last result, median seconds, spread = max - min) of `repeats` calls after one warm call."""
    fn()                                                                     # warm (module load, code objects)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, float(np.median(ts)), max(ts) - min(ts)


for I, trailing, M, R in ((200, [(10, 8), (12,)], 4, 3), (300, [(24, 40), (40,)], 2, 3)):
    Xs, y = _data(I, trailing, M, R, seed=3)
    name = " + ".join(str((I,) + tuple(t)) for t in trailing) + f" M={M} R={R} 10% NaN per block"
    m_on, m_off = ctPLS(R, options=ON), ctPLS(R, options=OFF)
    m_on.fit(Xs, y)
    if "--loo-only" in sys.argv:
        q = get_q2y_kfold(m_on, n_splits=I, per_component=True)
        rep = m_on.q2y_report_
        print(f"{name} | K = I once: {rep['form']}, refitted {rep['refitted']}, q2y {q[-1]:.10f}", file=OUT, flush=True)
        break
    m_off.fit(Xs, y)
    # K = I: the option-on call whole; the refits on a sample of folds, scaled
    q_on, dt_on, sp_on = _timed(lambda: get_q2y_kfold(m_on, n_splits=I, per_component=True))
    rep = m_on.q2y_report_
    assert COUPLED_FORM in rep["form"] and rep["refitted"] == [], rep
    idx = np.linspace(0, I - 1, n_refits).astype(int)

    def refits():
        for i in idx:
            test = np.zeros(I, dtype=bool)
            test[i] = True
            refit_fold(m_off, Xs, y, test, 1e-8, 100)
    _, dt_s, sp_s = _timed(refits)
    per = dt_s / len(idx)
    print(f"{name} | K = I: option off (refit per fold, timed on {len(idx)} folds and scaled) {per * 1e3:.3f} ms per fold = {per * I:.3f} s "
          f"(spread {sp_s / len(idx) * I:.3f} s) | option on ({rep['launches']} launch(es)) {dt_on / I * 1e3:.4f} ms per fold = {dt_on:.4f} s "
          f"(spread {sp_on:.4f} s), q2y {q_on[-1]:.10f} | off / on = {per * I / dt_on:.1f}x", file=OUT, flush=True)
    for K in (5, 10):
        q_off, dt_off, sp_off = _timed(lambda: get_q2y_kfold(m_off, n_splits=K, per_component=True))
        assert m_off.q2y_report_["form"].startswith("one refit per fold")
        q_k, dt_k, sp_k = _timed(lambda: get_q2y_kfold(m_on, n_splits=K, per_component=True))
        rep = m_on.q2y_report_
        assert COUPLED_FORM in rep["form"] and rep["refitted"] == [], rep
        print(f"{name} | {K}-fold: option off {dt_off / K * 1e3:.3f} ms per fold = {dt_off:.4f} s (spread {sp_off:.4f} s) | option on "
              f"(masked blocks {rep['masked_blocks']}) {dt_k / K * 1e3:.4f} ms per fold = {dt_k:.4f} s (spread {sp_k:.4f} s) | off / on = "
              f"{dt_off / dt_k:.2f}x | max |Q2Y_r on - off| = {float(np.abs(q_k - q_off).max()):.1e}", file=OUT, flush=True)
