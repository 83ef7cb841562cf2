#!/usr/bin/env python
"""Leave-one-out Q2Y of a coupled model: validate.get_q2y of a ctPLS on a (256, 64, 64) tensor next to a (256, 128) matrix, M = 8
responses, R = 4 components, float64 -- the workgroup-per-fold kernel (cmtfpls_loo_xcov_coupled_f64) against one ctPLS
refit per fold on the regular engine (device_folds=False, what get_q2y_kfold(n_splits=I) falls back to).  Median of five timed
calls after one warm-up call, each ended by a device synchronisation.  Recorded, not gated: writes one JSON object to --out
(default profiles/loo_coupled_time.json) and prints it."""
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
from cmtf_pls_amd.validate import get_q2y  # noqa: E402

I, TENSOR, MATRIX, M, R, LATENT, NOISE, SEED = 256, (64, 64), (128,), 8, 4, 6, 0.3, 0


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


def timed(model, device_folds: bool, repeats: int):
    times, q = [], None
    for k in range(repeats + 1):                                    # the first call is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q = get_q2y(model, device_folds=device_folds)
        torch.cuda.synchronize()
        if k:
            times.append(time.perf_counter() - t0)
    return statistics.median(times), float(q), dict(model.q2y_report_)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "loo_coupled_time.json"))
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    xs, y = data()
    model = ctPLS(R, dtype="float64", options=EngineOptions(small_fit=False))
    model.fit(xs, y)
    t_dev, q_dev, rep_dev = timed(model, True, args.repeats)
    t_ref, q_ref, rep_ref = timed(model, False, args.repeats)
    out = {"workload": f"get_q2y(ctPLS), blocks ({I}, {TENSOR[0]}, {TENSOR[1]}) + ({I}, {MATRIX[0]}), M = {M}, R = {R}, float64",
           "method": f"median of {args.repeats} calls after one warm-up",
           "device_seconds": t_dev, "device_form": rep_dev["form"], "device_q2y": q_dev, "device_n_iter_total": rep_dev.get("n_iter_total"),
           "refit_seconds": t_ref, "refit_form": rep_ref["form"], "refit_q2y": q_ref, "refit_n_iter_total": rep_ref.get("n_iter_total"),
           "speedup": t_ref / t_dev, "q2y_difference": abs(q_dev - q_ref), "gpu": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
