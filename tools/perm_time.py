"""Time the response-permutation test of K-fold Q2Y at cfg-2: a 65536 x 128 x 128 f32 tensor on the device, M = 16, R = 10, K = 5,
P = 99 permutations.  validate.permutation_test_q2y end to end (the device form: floor(32 / K) permutations x K folds per pass,
2R reads of X per pass) against the two Python loops a user would otherwise write:
  * P x get_q2y_kfold, the model's original_Y replaced by Y[pi_p] (the K-fold device form per permutation);
  * P x K literal algorithm="xcov" refits (each fold's training rows by index_select, fit, predict of the held-out rows).
Also the wide build alone (cmtfpls_kfold_wide_xcov_f32 at W = G M columns) against its f64-MFMA and HBM floors, and the largest
difference between the device null and the first baseline's.  One JSON line (printed, and written to --out when given).

    python tools/perm_time.py [--perms 99] [--baseline-perms 99] [--skip-baselines] [--out profiles/perm_time.json]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/perm_time.py --perms 99 --skip-baselines`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

F64_MFMA_PEAK = 78.6e12           # f64 matrix peak of the MI355X
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--perms", type=int, default=99)
    ap.add_argument("--baseline-perms", type=int, default=99)
    ap.add_argument("--skip-baselines", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cmtf_pls_amd import tPLS
    from cmtf_pls_amd.kfold import fold_ids
    from cmtf_pls_amd.synthetic import synthetic_shard_device
    from cmtf_pls_amd.validate import get_q2y_kfold, permutation_test_q2y

    I, J, K, M, R, F = 65536, 128, 128, 16, 10, 5
    X, Y = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0")
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    out = {"shape": [I, J, K], "M": M, "R": R, "K": F, "P": args.perms, "x_bytes": X.numel() * X.element_size()}

    permutation_test_q2y(m, n_permutations=2, n_splits=F)                       # warm-up (kernels loaded, allocator primed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = permutation_test_q2y(m, n_permutations=args.perms, n_splits=F, per_component=True)
    torch.cuda.synchronize()
    out["device_s"] = time.perf_counter() - t0
    out["device_report"] = {k: v for k, v in m.q2y_report_.items() if k not in ("n_iter", "observed")}
    out["q2y_per_component"] = [float(v) for v in res["q2y"]]
    out["p_value_per_component"] = [float(v) for v in res["p_value"]]
    out["null_last_min_max"] = [float(res["null"][:, -1].min()), float(res["null"][:, -1].max())]

    # the wide build alone: W = G M columns, K folds, cuda events around repeated calls
    be = m._get_engine().be
    G = out["device_report"]["models_per_pass"] // F
    W = G * M
    ids, _ = fold_ids(I, F)
    counts = np.bincount(ids, minlength=F)
    order = torch.from_numpy(np.argsort(ids, kind="stable").astype(np.int32)).cuda()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
    Yw = torch.randn(I, W, device="cuda:0", dtype=torch.float64)
    ydev = torch.zeros(F, W, device="cuda:0", dtype=torch.float64)
    S = torch.empty(F, W, J * K, device="cuda:0", dtype=torch.float64)
    mean = torch.empty(F, J * K, device="cuda:0", dtype=torch.float64)
    X2 = X.view(I, J * K)
    be.kfold_wide_xcov(X2, J, K, Yw, order, off, F, ydev, S, mean)
    ts = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        be.kfold_wide_xcov(X2, J, K, Yw, order, off, F, ydev, S, mean)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    wide = float(np.median(ts))
    flops = 2.0 * I * J * K * W
    out["wide_build"] = {"W": W, "median_s": wide, "runs_s": ts, "flops": flops,
                         "f64_mfma_floor_s": flops / F64_MFMA_PEAK, "hbm_floor_s": out["x_bytes"] / HBM_PEAK,
                         "f64_mfma_fraction": flops / F64_MFMA_PEAK / wide}
    del S, Yw

    if not args.skip_baselines:
        perms = res["permutations"][: args.baseline_perms]
        Y0 = m.original_Y
        nums = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for pi in perms:                                                           # P x get_q2y_kfold on Y[pi_p]
            m.original_Y = Y0[torch.from_numpy(pi).cuda()]
            nums.append(get_q2y_kfold(m, n_splits=F, per_component=True))
        torch.cuda.synchronize()
        m.original_Y = Y0
        out["baseline_kfold_s"] = (time.perf_counter() - t0) * args.perms / len(perms)
        out["baseline_kfold_measured_perms"] = len(perms)
        out["null_max_abs_diff_vs_kfold"] = float(np.abs(np.stack(nums) - res["null"][: len(perms)]).max())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for pi in perms:                                                           # P x K literal xcov refits
            Yp = Y0[torch.from_numpy(pi).cuda()]
            for k in range(F):
                test = ids == k
                tr = torch.from_numpy(np.flatnonzero(~test)).cuda()
                te = torch.from_numpy(np.flatnonzero(test)).cuda()
                r = tPLS(R, dtype="float32", algorithm="xcov")
                r.fit(X.index_select(0, tr), Yp.index_select(0, tr))
                r.predict(X.index_select(0, te))
        torch.cuda.synchronize()
        out["baseline_refits_xcov_s"] = (time.perf_counter() - t0) * args.perms / len(perms)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
