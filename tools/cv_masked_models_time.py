#!/usr/bin/env python3
"""The permutation test (99 permutations x 5 folds), repeated K-fold (10 x 5) and the bootstrap (100 resamples) of a tPLS whose X
has 10 % missing values: one regular-engine refit per model (EngineOptions.masked_folds off, the default) against every model as
a workgroup of cmtfpls_cv_masked_models_f64 (masked_folds on), at (200, 10, 8) M = 4 R = 3 and at a serology-sized (300, 24, 40)
M = 2 R = 3.  Every run is timed whole after one warm-up call of the same tool on a small problem; the agreement is the largest
difference of the returned values.
Usage: python tools/cv_masked_models_time.py [--shape small|large|both]"""
import contextlib, io, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmtf_pls_amd import tPLS
from cmtf_pls_amd.engine import EngineOptions
from cmtf_pls_amd.synthetic import import_synthetic
from cmtf_pls_amd.validate import bootstrap_factors, get_q2y_repeated_kfold, permutation_test_q2y

which = sys.argv[sys.argv.index("--shape") + 1] if "--shape" in sys.argv else "both"
OFF, ON = EngineOptions(), EngineOptions(masked_folds=True)
SHAPES = {"small": ((200, 10, 8), 4, 3), "large": ((300, 24, 40), 2, 3)}

OUT = sys.stdout
contextlib.redirect_stdout(io.StringIO()).__enter__()                        # the reference's "X has missing values" of every fit

TOOLS = (("permutation test (99 x 5-fold)", lambda m: permutation_test_q2y(m, n_permutations=99, n_splits=5, per_component=True),
          lambda r: r["null"], "q2y_report_"),
         ("repeated K-fold (10 x 5)", lambda m: get_q2y_repeated_kfold(m, n_splits=5, n_repeats=10, per_component=True),
          lambda r: r["q2y"], "q2y_report_"),
         ("bootstrap (100)", lambda m: bootstrap_factors(m, n_resamples=100), lambda r: r["coef"], "bootstrap_report_"))


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


# warm-up: module load and code objects of every path, on a small problem
xw, yw, _ = import_synthetic((20, 5, 4), 2, 2, error=0.1, seed=1)
xw[np.random.default_rng(2).random(xw.shape) < 0.1] = np.nan
for opt in (OFF, ON):
    mw = tPLS(2, options=opt)
    mw.fit(xw, yw)
    permutation_test_q2y(mw, n_permutations=2, n_splits=3)
    get_q2y_repeated_kfold(mw, n_splits=3, n_repeats=2)
    bootstrap_factors(mw, n_resamples=2)

for key in (("small", "large") if which == "both" else (which,)):
    shape, M, R = SHAPES[key]
    x, y, _ = import_synthetic(shape, M, R, error=0.1, seed=3)
    x[np.random.default_rng(4).random(x.shape) < 0.1] = np.nan
    m_off, m_on = tPLS(R, options=OFF), tPLS(R, options=ON)
    m_off.fit(x, y)
    m_on.fit(x, y)
    for name, run, value, report in TOOLS:
        r_off, dt_off = _timed(lambda: run(m_off))
        rep_off = getattr(m_off, report)
        r_on, dt_on = _timed(lambda: run(m_on))
        rep_on = getattr(m_on, report)
        a, b = np.asarray(value(r_on)), np.asarray(value(r_off))
        diff = float(np.nanmax(np.abs(a - b)) / max(np.nanmax(np.abs(b)), 1e-300))
        print(f"{shape} M={M} R={R} 10% NaN | {name}: option off ({rep_off['form']}) {dt_off:.4f} s | option on ({rep_on['form']}, "
              f"{rep_on.get('masked_models')} masked models, {rep_on.get('masked_batches')} masked batches) {dt_on:.4f} s | speed-up "
              f"{dt_off / dt_on:.1f}x | max relative difference {diff:.1e}", file=OUT, flush=True)
