#!/usr/bin/env python
"""Resampling of a ctPLS with a block of order 4 and missing values: blocks (120, 12, 8, 5) and (120, 20) with 10 % NaN, M = 3
responses, R = 4 components, float64 -- leave-one-out (validate.get_q2y), 10-fold and 5-fold (validate.get_q2y_kfold) and
bootstrap_factors with 64 resamples through the workgroup-per-model kernel (cmtfpls_cv_masked_coupled_tensor_f64,
EngineOptions.masked_tensor_folds_coupled), each against the same call with device_folds=False (one refit per model on
the regular engine) in the same process.  Median of five timed calls after one warm-up call, each ended by a device synchronisation.
Recorded, not gated: writes one JSON object to --out (default profiles/cv_masked_coupled_order4_time.json) and prints it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cmtf_pls_amd import ctPLS  # noqa: E402
from cmtf_pls_amd.engine import EngineOptions  # noqa: E402
from cmtf_pls_amd.kfold import COUPLED_TENSOR_FORM  # noqa: E402
from cmtf_pls_amd.validate import bootstrap_factors, get_q2y, get_q2y_kfold  # noqa: E402

SHAPES, M, R, LATENT, NOISE, NAN, SEED, RESAMPLES = [(120, 12, 8, 5), (120, 20)], 3, 4, 5, 0.3, 0.1, 0, 64


def data():
    rng = np.random.default_rng(SEED)
    I = SHAPES[0][0]
    T = rng.standard_normal((I, LATENT))
    Xs = []
    for b, shape in enumerate(SHAPES):
        kr = np.ones((1, LATENT))
        for d in shape[1:]:
            kr = (kr[:, None, :] * rng.standard_normal((d, LATENT))[None, :, :]).reshape(-1, LATENT)
        x = (T @ kr.T).reshape(shape) + NOISE * rng.standard_normal(shape)
        hole = rng.random(shape) < NAN
        hole.reshape(I, -1)[:, b] = False                           # every row keeps an observed entry in every block
        x[hole] = np.nan
        Xs.append(x)
    y = T @ rng.standard_normal((LATENT, M)) + NOISE * rng.standard_normal((I, M))
    return Xs, y


def timed(model, call, device_folds: bool, repeats: int):
    times, value, rep = [], None, None
    for k in range(repeats + 1):                                    # the first call is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value, rep = call(model, device_folds)
        torch.cuda.synchronize()
        if k:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), float(value), dict(rep)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "cv_masked_coupled_order4_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    Xs, y = data()
    model = ctPLS(R, dtype="float64", options=EngineOptions(small_fit=False, masked_tensor_folds_coupled=True))
    model.fit(Xs, y)
    idx = np.random.default_rng(SEED + 1).integers(0, SHAPES[0][0], size=(RESAMPLES, SHAPES[0][0]))

    def boot(m, dev):                                               # the value compared: the OOB Q2Y with all R components
        out = bootstrap_factors(m, resamples=idx, device_folds=dev)
        return out["oob_q2y"][-1], m.bootstrap_report_

    cases = {"leave_one_out": lambda m, dev: (get_q2y(m, device_folds=dev), m.q2y_report_),
             "10_fold": lambda m, dev: (get_q2y_kfold(m, n_splits=10, device_folds=dev), m.q2y_report_),
             "5_fold": lambda m, dev: (get_q2y_kfold(m, n_splits=5, device_folds=dev), m.q2y_report_),
             f"bootstrap_{RESAMPLES}": boot}
    out = {"workload": f"ctPLS, blocks {SHAPES} with {int(100 * NAN)} % NaN, M = {M}, R = {R}, float64",
           "method": f"median of {args.repeats} calls after one warm-up, device and refits in the same process",
           "gpu": torch.cuda.get_device_name(0), "cases": {}}
    for name, call in cases.items():
        t_dev, q_dev, rep_dev = timed(model, call, True, args.repeats)
        assert COUPLED_TENSOR_FORM in rep_dev["form"], rep_dev
        t_ref, q_ref, rep_ref = timed(model, call, False, args.repeats)
        out["cases"][name] = {"device_seconds": t_dev, "device_form": rep_dev["form"], "device_q2y": q_dev,
                              "device_launches": rep_dev.get("launches"), "device_refitted": rep_dev.get("refitted"),
                              "max_n_iter": int(np.max(rep_dev["n_iter"])), "refit_seconds": t_ref, "refit_form": rep_ref["form"],
                              "refit_q2y": q_ref, "speedup": t_ref / t_dev, "q2y_difference": abs(q_dev - q_ref)}
        print(name, json.dumps(out["cases"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
