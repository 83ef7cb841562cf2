"""Time the response-permutation test of a coupled model at the DESIGN 8c pair: a 65536 x 128 x 128 f32 tensor block plus a
65536 x 256 f32 matrix block (synthetic_shard_device with matrix_block=256), M = 16, R = 10, K = 5, P = 99 permutations, both blocks
on the device.  One warm-up, then one timed run each of
  (a) validate.permutation_test_q2y on a ctPLS with EngineOptions.coupled_permutations (the device form: floor(32 / K) permutations
      x K folds per pass, 2R reads of each block per pass);
  (b) the same call with the option off: one regular-engine ctPLS refit per fold and permutation, the path the option replaces
      and the baseline;
  (c) P x get_q2y_kfold, the model's original_Y replaced by Y[pi_p] (the coupled K-fold device form per permutation).
Also the largest difference between the null of (a) and those of (b) and (c).  One JSON line (printed, and written to --out when
given).

    python tools/perm_coupled_time.py [--perms 99] [--baseline-perms 99] [--skip-baselines] [--out profiles/perm_coupled_time.json]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/perm_coupled_time.py --perms 99 --skip-baselines`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--perms", type=int, default=99)
    ap.add_argument("--baseline-perms", type=int, default=99)
    ap.add_argument("--skip-baselines", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cmtf_pls_amd import ctPLS
    from cmtf_pls_amd.engine import EngineOptions
    from cmtf_pls_amd.synthetic import synthetic_shard_device
    from cmtf_pls_amd.validate import get_q2y_kfold, permutation_test_q2y

    I, J, K, Jm, M, R, F = 65536, 128, 128, 256, 16, 10, 5
    X, Y, Xm = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0", matrix_block=Jm)
    Xm = Xm.to(torch.float32).contiguous()
    Xs = [X, Xm]
    on = ctPLS(R, dtype="float32", options=EngineOptions(coupled_permutations=True))
    on.fit(Xs, Y)
    out = {"shapes": [[I, J, K], [I, Jm]], "M": M, "R": R, "K": F, "P": args.perms,
           "x_bytes": [x.numel() * x.element_size() for x in Xs]}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    permutation_test_q2y(on, n_permutations=2, n_splits=F)                      # warm-up (kernels loaded, allocator primed)
    out["device_s"], res = timed(lambda: permutation_test_q2y(on, n_permutations=args.perms, n_splits=F, per_component=True))
    rep = on.q2y_report_
    out["device_report"] = {k: v for k, v in rep.items() if k not in ("n_iter", "observed")}
    if rep["passes"]:
        it = np.array(rep["n_iter"])                                             # P x K x R
        out["n_iter_mean_max"] = [float(it.mean()), int(it.max())]
    out["q2y_per_component"] = [float(v) for v in res["q2y"]]
    out["p_value_per_component"] = [float(v) for v in res["p_value"]]
    out["null_last_min_max"] = [float(res["null"][:, -1].min()), float(res["null"][:, -1].max())]

    if not args.skip_baselines:
        perms = res["permutations"][: args.baseline_perms]
        scale = args.perms / len(perms)
        off = ctPLS(R, dtype="float32")
        off.fit(Xs, Y)
        permutation_test_q2y(off, n_permutations=1, n_splits=F)                  # warm-up
        t, base = timed(lambda: permutation_test_q2y(off, permutations=perms, n_splits=F, per_component=True))
        out["option_off_s"] = t * scale                                           # (b): the baseline
        out["option_off_report"] = {k: v for k, v in off.q2y_report_.items() if k not in ("n_iter", "observed")}
        out["baseline_measured_perms"] = len(perms)
        out["null_max_abs_diff_vs_option_off"] = float(np.abs(base["null"] - res["null"][: len(perms)]).max())
        out["device_over_option_off"] = out["device_s"] / out["option_off_s"]
        Y0 = off.original_Y
        nums = []
        off.original_Y = Y0[torch.from_numpy(perms[0]).cuda()]
        get_q2y_kfold(off, n_splits=F, per_component=True)                       # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for pi in perms:                                                          # (c): P x get_q2y_kfold on Y[pi_p]
            off.original_Y = Y0[torch.from_numpy(pi).cuda()]
            nums.append(get_q2y_kfold(off, n_splits=F, per_component=True))
        torch.cuda.synchronize()
        off.original_Y = Y0
        out["baseline_kfold_s"] = (time.perf_counter() - t0) * scale
        out["null_max_abs_diff_vs_kfold"] = float(np.abs(np.stack(nums) - res["null"][: len(perms)]).max())
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
