"""Time the three kernels of csrc/impute.hip at cfg-2: a 65536 x 128 x 128 f32 tensor on the device, R = 10, 10 % held out (mask,
held-out residual) or missing (impute), against the streaming ceilings measured in the same run.
  kernels    cmtfpls_holdout_mask_f32, cmtfpls_heldout_resid_f32, cmtfpls_impute_f32 out of place and in place (HIP events, median
             of --reps launches after a warm-up launch)
  ceilings   cmtfpls_ceiling_read and cmtfpls_ceiling_copy on the same buffers
  fallback   the torch forms of ProjectionMixin (impute: every row; held-out sums: --fallback-rows rows, because its mask comes
             from the host restatement of the counter rule) and the one-liner torch.where(isnan(X), Xhat, X) on a materialised Xhat
The factors are random: the kernels' time does not depend on their values.  One JSON line (printed, and written to --out).

    python tools/impute_time.py [--reps 10] [--out profiles/impute_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _events(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(np.min(ts))


def _wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=[65536, 128, 128])
    ap.add_argument("--fallback-rows", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cmtf_pls_amd.backend import HipBackend
    from cmtf_pls_amd.projection import ProjectionMixin

    I, J, K = args.shape
    R, P = 10, J * K
    dev = torch.device("cuda:0")
    be = HipBackend(dev)
    g = torch.Generator(device=dev).manual_seed(215)
    T = torch.randn(I, R, dtype=torch.float64, device=dev, generator=g)
    WA = torch.randn(J, R, dtype=torch.float64, device=dev, generator=g)
    WB = torch.randn(K, R, dtype=torch.float64, device=dev, generator=g)
    mean = torch.randn(P, dtype=torch.float64, device=dev, generator=g)
    X = torch.empty(I, P, dtype=torch.float32, device=dev)
    be.recon(T, WA, WB, mean, X)
    be.add_noise(X, 0.1, 215)
    Xm = X.clone()
    be.add_noise(Xm, 0.0, 216, 0, 0.1)                                       # 10 % missing, for impute
    out_buf = torch.empty_like(X)
    nbytes = X.numel() * X.element_size()
    res = {"shape": [I, J, K], "R": R, "dtype": "float32", "x_bytes": nbytes, "reps": args.reps, "fraction": 0.1}

    med, _ = _events(lambda: be.ceiling("read", X), args.reps)
    res["ceiling_read_ms"], read_tbs = med * 1e3, nbytes / med / 1e12
    med, _ = _events(lambda: be.ceiling("copy", X, dst=out_buf), args.reps)
    res["ceiling_copy_ms"], copy_tbs = med * 1e3, 2 * nbytes / med / 1e12
    res["ceiling_read_tbs"], res["ceiling_copy_tbs"] = read_tbs, copy_tbs

    def put(name, med, moved, ceiling):
        res[f"{name}_ms"], res[f"{name}_tbs"], res[f"{name}_of_ceiling"] = med * 1e3, moved / med / 1e12, moved / med / 1e12 / ceiling

    med, _ = _events(lambda: be.holdout_mask(X, out_buf, 0.1, 7, 2), args.reps)
    put("holdout_mask", med, 2 * nbytes, copy_tbs)
    med, _ = _events(lambda: be.heldout_resid(X, T, WA, WB, mean, 0.1, 7, 2), args.reps)
    put("heldout_resid", med, nbytes, read_tbs)
    med, _ = _events(lambda: be.impute(Xm, out_buf, T, WA, WB, mean), args.reps)
    put("impute_out_of_place", med, 2 * nbytes, copy_tbs)
    count = be.impute(Xm, out_buf, T, WA, WB, mean)
    res["imputed_fraction"] = float(count.item()) / X.numel()
    work = Xm.clone()

    def in_place():                                                           # restore the gaps, then time the pass alone
        work.copy_(Xm)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        be.impute(work, work, T, WA, WB, mean)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    in_place()
    med = float(np.median([in_place() for _ in range(args.reps)]))
    put("impute_in_place", med, nbytes, read_tbs)                            # against the read ceiling: the gaps' vectors are written too
    del work

    reps = max(3, args.reps // 3)
    res["fallback_impute_ms"] = _wall(lambda: ProjectionMixin._impute_rows_torch(Xm, out_buf, T, WA, WB, mean), reps) * 1e3

    def one_liner():
        xhat = torch.empty_like(Xm)
        be.recon(T, WA, WB, mean, xhat)
        return torch.where(torch.isnan(Xm), xhat, Xm)

    one_liner()
    res["one_liner_where_ms"] = _wall(one_liner, reps) * 1e3
    n = min(args.fallback_rows, I)
    t = _wall(lambda: ProjectionMixin._heldout_sums_torch(X[:n], T[:n], WA, WB, mean, 0.1, 7, 2, 0), 1)
    res["fallback_heldout_rows"], res["fallback_heldout_ms_for_those_rows"] = n, t * 1e3
    res["fallback_heldout_ms_scaled_to_all_rows"] = t * 1e3 * I / n
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
