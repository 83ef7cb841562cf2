"""Time the contribution pass at cfg-2: a 65536 x 128 x 128 f32 tensor on the device, M = 16, R = 10.
  kernel     cmtfpls_contrib_rows_f32 over every row and, in the same run, cmtfpls_resid_rows_f32 with columns (HIP events, warm-up,
             median of --reps calls each, the two alternating)
  fallback   the torch form of the same rows (ProjectionMixin._contribution_rows_torch, row blocks of <= 256 MB): what a user has
             without the kernel
  estimator  validate.sample_contributions(m) end to end with the training statistics cached, and for 16 flagged rows
The bytes behind the rate: X once (x_bytes) plus the four outputs (out_bytes).  One JSON line (printed, and written to --out).

    python tools/contributions_time.py [--reps 20] [--out profiles/contributions_time.json]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/contributions_time.py --reps 5`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _wall(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return out, float(np.median(ts)), float(np.min(ts))


def _event(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cmtf_pls_amd import tPLS
    from cmtf_pls_amd.diagnostics import _training_stats
    from cmtf_pls_amd.synthetic import synthetic_shard_device
    from cmtf_pls_amd.validate import sample_contributions

    I, J, K, M, R = args.rows, 128, 128, 16, 10
    X, Y = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0")[:2]
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    eng = m._get_engine()
    be, st = eng.be, m._state
    blk = st.blocks[0]
    WA, WB = eng._kr_operands(blk, R)
    X2 = X.view(I, -1)
    stats = _training_stats(m, eng, st, False, True, None)[0]
    T = st.T
    H = eng.t2_direction_solve(st, (T - stats["tbar"]) @ stats["S_pinv"])
    nbytes = X.numel() * X.element_size()
    obytes = I * (J + K) * 2 * 8
    out = {"shape": [I, J, K], "M": M, "R": R, "dtype": "float32", "x_bytes": nbytes, "out_bytes": obytes, "reps": args.reps}

    kernels = {"contrib_rows": lambda: be.contrib_rows(X2, T, H, WA, WB, blk.mean),
               "resid_rows_cols": lambda: be.resid_rows(X2, T, WA, WB, blk.mean, True)}
    times = {k: [] for k in kernels}
    for _ in range(3):
        for fn in kernels.values():
            fn()
    for _ in range(args.reps):                                    # alternating: both see the same neighbours on the card
        for k, fn in kernels.items():
            times[k].append(_event(fn))
    for k, ts in times.items():
        out[f"{k}_ms"], out[f"{k}_best_ms"] = float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3
    out["contrib_rows_tbs"] = (nbytes + obytes) / (out["contrib_rows_ms"] * 1e-3) / 1e12
    out["resid_rows_cols_tbs"] = nbytes / (out["resid_rows_cols_ms"] * 1e-3) / 1e12
    out["contrib_over_resid"] = out["contrib_rows_ms"] / out["resid_rows_cols_ms"]

    fallback = lambda: eng._contribution_rows_torch(X2, T, H, WA, WB, blk.mean, None)  # noqa: E731
    ref = fallback()
    _, med, best = _wall(fallback, max(3, args.reps // 4))
    out["torch_fallback_ms"], out["torch_fallback_best_ms"] = med * 1e3, best * 1e3
    out["fallback_over_contrib"] = out["torch_fallback_ms"] / out["contrib_rows_ms"]
    got = kernels["contrib_rows"]()
    out["max_rel_diff_spe_vs_fallback"] = float(max(((g - r).abs() / r.abs().clamp_min(1e-300)).max() for g, r in zip(got[:2], ref[:2])))
    out["max_abs_diff_t2_vs_fallback"] = float(max((g - r).abs().max() for g, r in zip(got[2:], ref[2:])))
    del ref, got

    sample_contributions(m)
    _, med, best = _wall(lambda: sample_contributions(m), max(3, args.reps // 4))
    out["estimator_all_rows_ms"], out["estimator_all_rows_best_ms"] = med * 1e3, best * 1e3
    out["estimator_report"] = dict(m.contributions_report_)
    flagged = np.random.default_rng(0).permutation(I)[:16]
    sample_contributions(m, rows=flagged)
    _, med, best = _wall(lambda: sample_contributions(m, rows=flagged), args.reps)
    out["estimator_16_rows_ms"], out["estimator_16_rows_best_ms"] = med * 1e3, best * 1e3
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
