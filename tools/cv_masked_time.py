#!/usr/bin/env python3
"""Cross-validated Q2Y of a tPLS whose X has 10 % missing values: one refit per fold on the regular engine (EngineOptions.
masked_folds off, the default) against every fold in one launch (masked_folds on: cmtfpls_cv_masked_f64).  Leave-one-out
(validate.get_q2y) and 5- / 10-fold (validate.get_q2y_kfold), at (200, 10, 8) M = 4 R = 3 and at a serology-sized (300, 24, 40)
M = 2 R = 3.  The leave-one-out refits are timed on N folds and scaled (every fold costs the same); everything else is timed whole.
Usage: python tools/cv_masked_time.py [--refits N]"""
import contextlib, io, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmtf_pls_amd import tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.synthetic import import_synthetic
from cmtf_pls_amd.validate import get_q2y, get_q2y_kfold, loo_predictions

n_refits = int(sys.argv[sys.argv.index("--refits") + 1]) if "--refits" in sys.argv else 24
OFF, ON = EngineOptions(), EngineOptions(masked_folds=True)


OUT = sys.stdout
contextlib.redirect_stdout(io.StringIO()).__enter__()                        # the reference's "X has missing values" of every fit


def _timed(fn):
    fn()                                                                     # warm (module load, code objects)
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


for shape, M, R in (((200, 10, 8), 4, 3), ((300, 24, 40), 2, 3)):
    x, y, _ = import_synthetic(shape, M, R, error=0.1, seed=3)
    x[np.random.default_rng(4).random(x.shape) < 0.1] = np.nan
    I = shape[0]
    m_on = tPLS(R, options=ON)
    m_on.fit(x, y)
    # leave-one-out: masked form whole; refits on a sample of folds (literal tPLS.fit + predict without sample i)
    q_on, dt_on = _timed(lambda: get_q2y(m_on))
    form = m_on.q2y_report_["form"]
    pred = loo_predictions(m_on)
    idx = np.linspace(0, I - 1, n_refits).astype(int)
    r = tPLS(R, options=OFF)
    keep = np.ones(I, dtype=bool)
    keep[0] = False
    r.fit(x[keep], y[keep])                                                   # warm
    worst, t1 = 0.0, time.perf_counter()
    for i in idx:
        keep[:] = True
        keep[i] = False
        r.fit(x[keep], y[keep])
        want = r.predict(x[i:i + 1]).reshape(-1)
        worst = max(worst, float(np.abs(pred[i].reshape(-1) - want).max() / max(1.0, np.abs(want).max())))
    per_refit = (time.perf_counter() - t1) / len(idx)
    print(f"{shape} M={M} R={R} 10% NaN | LOO: option off (refit per fold, timed on {len(idx)} folds) {per_refit * 1e3:.3f} ms per fold "
          f"= {per_refit * I:.3f} s | option on ({form}) {dt_on / I * 1e3:.4f} ms per fold = {dt_on:.4f} s, q2y {q_on:.10f} | "
          f"speed-up {per_refit * I / dt_on:.1f}x | max |prediction - refit| = {worst:.1e} (relative)", file=OUT, flush=True)
    for K in (5, 10):
        m_off = tPLS(R, options=OFF)
        m_off.fit(x, y)
        q_off, dt_off = _timed(lambda: get_q2y_kfold(m_off, n_splits=K, per_component=True))
        assert m_off.q2y_report_["form"].startswith("one refit per fold")
        q_k, dt_k = _timed(lambda: get_q2y_kfold(m_on, n_splits=K, per_component=True))
        rep = m_on.q2y_report_
        print(f"{shape} M={M} R={R} 10% NaN | {K}-fold: option off {dt_off / K * 1e3:.3f} ms per fold = {dt_off:.4f} s | option on "
              f"({rep['form']}, {rep['masked_folds']} masked folds) {dt_k / K * 1e3:.4f} ms per fold = {dt_k:.4f} s | speed-up "
              f"{dt_off / dt_k:.1f}x | max |Q2Y_r on - off| = {float(np.abs(q_k - q_off).max()):.1e}", file=OUT, flush=True)
