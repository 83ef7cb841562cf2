#!/usr/bin/env python
"""Leave-one-out Q2Y and the factor bootstrap of a coupled model with an order-4 block: a ctPLS on a (120, 12, 8, 5) tensor next to a
(120, 20) matrix, M = 3 responses, R = 4 components, float64, with EngineOptions.tensor_resamples_coupled.
  get_q2y            the workgroup-per-fold kernel (cmtfpls_loo_xcov_coupled_tensor_f64) against one ctPLS refit per fold on the
                     regular engine (device_folds=False)
  bootstrap_factors  64 resamples through the weighted coupled passes (cmtfpls_kfold_inner_coupled_tensor_f64) against one refit per
                     resample (device_folds=False)
Each pair is timed in the same process: the median of five calls after one warm-up call, each ended by a device synchronisation.
Recorded, not gated: writes one JSON object to --out (default profiles/loo_coupled_order4_time.json) and prints it."""
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
from cmtf_pls_amd.validate import bootstrap_factors, get_q2y  # noqa: E402

I, TENSOR, MATRIX, M, R, LATENT, NOISE, SEED, RESAMPLES = 120, (12, 8, 5), (20,), 3, 4, 5, 0.3, 0, 64


def data():
    rng = np.random.default_rng(SEED)
    T = rng.standard_normal((I, LATENT))
    xs = []
    for trail in (TENSOR, MATRIX):
        kr = np.ones((1, LATENT))
        for d in trail:
            kr = (kr[:, None, :] * rng.standard_normal((d, LATENT))[None, :, :]).reshape(-1, LATENT)
        xs.append((T @ kr.T).reshape((I,) + trail) + NOISE * rng.standard_normal((I,) + trail))
    y = T @ rng.standard_normal((LATENT, M)) + NOISE * rng.standard_normal((I, M))
    return xs, y


def timed(call, report, repeats: int):
    times, value = [], None
    for k in range(repeats + 1):                                    # the first call is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = call()
        torch.cuda.synchronize()
        if k:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), value, dict(report())


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "loo_coupled_order4_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    xs, y = data()
    model = ctPLS(R, dtype="float64", options=EngineOptions(small_fit=False, tensor_resamples_coupled=True))
    model.fit(xs, y)
    idx = np.random.default_rng(SEED).integers(0, I, size=(RESAMPLES, I))
    out = {"workload": f"ctPLS, blocks ({I}, {', '.join(map(str, TENSOR))}) + ({I}, {MATRIX[0]}), M = {M}, R = {R}, float64",
           "method": f"median of {args.repeats} calls after one warm-up, device and refits in the same process",
           "gpu": torch.cuda.get_device_name(0)}
    t_dev, q_dev, rep_dev = timed(lambda: get_q2y(model), lambda: model.q2y_report_, args.repeats)
    t_ref, q_ref, rep_ref = timed(lambda: get_q2y(model, device_folds=False), lambda: model.q2y_report_, args.repeats)
    out["get_q2y"] = {"device_seconds": t_dev, "device_form": rep_dev["form"], "device_n_iter_total": rep_dev.get("n_iter_total"),
                      "refit_seconds": t_ref, "refit_form": rep_ref["form"], "refit_n_iter_total": rep_ref.get("n_iter_total"),
                      "speedup": t_ref / t_dev, "q2y_difference": abs(float(q_dev) - float(q_ref))}
    t_dev, b_dev, rep_dev = timed(lambda: bootstrap_factors(model, resamples=idx), lambda: model.bootstrap_report_, args.repeats)
    t_ref, b_ref, rep_ref = timed(lambda: bootstrap_factors(model, resamples=idx, device_folds=False), lambda: model.bootstrap_report_,
                                  args.repeats)
    out["bootstrap_factors"] = {"resamples": RESAMPLES, "device_seconds": t_dev, "device_form": rep_dev["form"],
                                "device_passes": rep_dev["passes"], "refit_seconds": t_ref, "refit_form": rep_ref["form"],
                                "speedup": t_ref / t_dev,
                                "oob_q2y_difference": float(np.abs(b_dev["oob_q2y"] - b_ref["oob_q2y"]).max())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
