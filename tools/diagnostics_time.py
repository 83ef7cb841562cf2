"""Time the sample diagnostics at cfg-2: a 65536 x 128 x 128 f32 tensor on the device, M = 16, R = 10.
  kernel     cmtfpls_resid_rows_f32 (rows and columns) and, in the same run, its neighbour cmtfpls_recon_r2_f32 (HIP events,
             median of --reps calls each)
  training   validate.sample_diagnostics(m) end to end, first call (builds the cached training statistics) and again
  new rows   sample_diagnostics(m, Xn) with the cache warm, against m.transform(Xn) alone (Xn: a second tensor of the same size)
  baseline   what a user writes without it: X_reconstructed(device=True) (writes a 4.3 GB tensor), then torch's subtraction and
             sums over the finite entries
One JSON line (printed, and written to --out when given).

    python tools/diagnostics_time.py [--reps 20] [--out profiles/diagnostics_time.json]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/diagnostics_time.py --reps 5`."""
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


def _events(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cmtf_pls_amd import tPLS
    from cmtf_pls_amd.synthetic import synthetic_shard_device
    from cmtf_pls_amd.validate import sample_diagnostics

    I, J, K, M, R = 65536, 128, 128, 16, 10
    X, Y = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0")[:2]
    Xn = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=216, device="cuda:0")[0]
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    eng = m._get_engine()
    be, st = eng.be, m._state
    blk = st.blocks[0]
    WA, WB = eng._kr_operands(blk, R)
    X2 = X.view(I, -1)
    nbytes = X.numel() * X.element_size()
    out = {"shape": [I, J, K], "M": M, "R": R, "dtype": "float32", "x_bytes": nbytes, "reps": args.reps}

    be.resid_rows(X2, st.T, WA, WB, blk.mean, True)
    be.recon_r2(X2, st.T, WA, WB, blk.mean)
    for name, fn in (("resid_rows_cols", lambda: be.resid_rows(X2, st.T, WA, WB, blk.mean, True)),
                     ("resid_rows_nocols", lambda: be.resid_rows(X2, st.T, WA, WB, blk.mean, False)),
                     ("recon_r2", lambda: be.recon_r2(X2, st.T, WA, WB, blk.mean))):
        med, best = _events(fn, args.reps)
        out[f"{name}_ms"] = med * 1e3
        out[f"{name}_tbs"] = nbytes / med / 1e12

    d, t_first = _wall(lambda: sample_diagnostics(m), 1)[:2]
    out["training_first_call_ms"] = t_first * 1e3
    out["training_first_report"] = dict(m.diagnostics_report_)
    _, med, best = _wall(lambda: sample_diagnostics(m), args.reps)
    out["training_ms"], out["training_best_ms"] = med * 1e3, best * 1e3
    out["training_report"] = dict(m.diagnostics_report_)
    out["training_spe_over_ssq"] = float(d["spe"].sum() / d["ssq"].sum())
    out["one_minus_R2X"] = float(1 - m.R2X[-1])

    sample_diagnostics(m, Xn)
    _, med, best = _wall(lambda: sample_diagnostics(m, Xn), args.reps)
    out["new_rows_warm_ms"], out["new_rows_warm_best_ms"] = med * 1e3, best * 1e3
    out["new_rows_report"] = dict(m.diagnostics_report_)
    m.transform(Xn)
    _, med, best = _wall(lambda: m.transform(Xn), args.reps)
    out["transform_ms"], out["transform_best_ms"] = med * 1e3, best * 1e3

    mean = blk.mean.view(1, -1)

    def baseline():
        rec = m.X_reconstructed(device=True).view(I, -1)
        x = X2.double() - mean
        fin = torch.isfinite(x)
        e = torch.where(fin, x - (rec.double() - mean), 0.0)
        return (e * e).sum(dim=1), torch.where(fin, x * x, 0.0).sum(dim=1)

    spe_b, _ = baseline()
    _, med, best = _wall(baseline, max(3, args.reps // 4))
    out["baseline_reconstruct_subtract_ms"], out["baseline_best_ms"] = med * 1e3, best * 1e3
    spe_d = torch.from_numpy(d["spe"]).to(spe_b.device)
    out["baseline_spe_max_rel_diff"] = float(((spe_b - spe_d).abs() / spe_d.abs().clamp_min(1e-300)).max())
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
