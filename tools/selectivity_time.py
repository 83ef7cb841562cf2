"""Time the target-projection pass behind validate.selectivity_ratio at cfg-2: a 65536 x 128 x 128 f32 tensor on the device, M = 16,
R = 10.
  complete   cmtfpls_selectivity_cols_f32 (masked = 0) and, in the same run, cmtfpls_xcov_stats_f32 with the same tau: the same MFMA
             work on uncentred X plus one subtraction per element (HIP events, warm-up, median of --reps, the kernels alternating)
  masked     cmtfpls_selectivity_cols_f32 (masked = 1) on a copy of X with 10 % NaN, against the torch row-block form
             (ProjectionMixin._selectivity_cols_torch) on the same inputs
  ceiling    cmtfpls_ceiling_read over the same buffer, in the same run
  estimator  validate.selectivity_ratio(m, cells=False) on the training rows, device=True against device=False
One JSON line (printed, and written to --out).

    python tools/selectivity_time.py [--reps 20] [--out profiles/selectivity_time.json]"""
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
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts))


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
    from cmtf_pls_amd.synthetic import synthetic_shard_device
    from cmtf_pls_amd.validate import selectivity_ratio

    I, J, K, M, R = args.rows, 128, 128, 16, 10
    X, Y = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0")[:2]
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    eng = m._get_engine()
    be, st = eng.be, m._state
    blk = st.blocks[0]
    X2 = X.view(I, -1)
    P = X2.shape[1]
    Bm = torch.from_numpy(np.ascontiguousarray(m.coef_ @ m.Y_factors[1].T)).to(X.device)
    Tau = (st.T @ Bm).contiguous()
    Xn = X2.clone()
    g = torch.Generator(device=X.device).manual_seed(1)
    for r0 in range(0, I, 4096):                                  # 10 % NaN, row blocks: no mask tensor of X's size
        sl = Xn[r0:r0 + 4096]
        sl[torch.rand(sl.shape, generator=g, device=X.device) < 0.1] = float("nan")
    nbytes = X.numel() * X.element_size()
    out = {"shape": [I, J, K], "M": M, "R": R, "dtype": "float32", "x_bytes": nbytes, "reps": args.reps}
    S = be.empty(M, P)
    kernels = {"selectivity_complete": lambda: be.selectivity_cols(X2, Tau, blk.mean, False),
               "xcov_stats": lambda: be.xcov_stats(X2, Tau, out=S),
               "selectivity_masked": lambda: be.selectivity_cols(Xn, Tau, blk.mean, True),
               "ceiling_read": lambda: be.ceiling("read", X2)}
    times = {k: [] for k in kernels}
    for _ in range(3):
        for fn in kernels.values():
            fn()
    for _ in range(args.reps):                                    # alternating: all see the same neighbours on the card
        for k, fn in kernels.items():
            times[k].append(_event(fn))
    for k, ts in times.items():
        out[f"{k}_ms"], out[f"{k}_best_ms"], out[f"{k}_std_ms"] = float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3, float(np.std(ts)) * 1e3
        out[f"{k}_tbs"] = nbytes / float(np.median(ts)) / 1e12
    out["complete_over_xcov_stats"] = out["selectivity_complete_ms"] / out["xcov_stats_ms"]
    out["complete_of_ceiling"] = out["selectivity_complete_tbs"] / out["ceiling_read_tbs"]
    out["masked_of_ceiling"] = out["selectivity_masked_tbs"] / out["ceiling_read_tbs"]

    fallback = lambda: eng._selectivity_cols_torch(Xn, Tau, blk.mean, True)  # noqa: E731
    ref = fallback()
    med, best = _wall(fallback, max(3, args.reps // 4))
    out["torch_masked_ms"], out["torch_masked_best_ms"] = med * 1e3, best * 1e3
    out["torch_over_masked"] = out["torch_masked_ms"] / out["selectivity_masked_ms"]
    got = kernels["selectivity_masked"]()
    out["max_rel_diff_s_vs_torch"] = float(((got[2] - ref[2]).abs() / ref[2].abs().clamp_min(1e-300)).max())
    out["max_rel_diff_d_vs_torch"] = float(((got[1] - ref[1]).abs() / ref[1].abs().clamp_min(1e-300)).max())
    out["max_abs_diff_a_vs_torch"] = float((got[0] - ref[0]).abs().max())
    out["n_equal_torch"] = bool(torch.equal(got[3], ref[3]))
    del ref, got

    selectivity_ratio(m, cells=False)
    med, best = _wall(lambda: selectivity_ratio(m, cells=False), max(3, args.reps // 4))
    out["estimator_ms"], out["estimator_best_ms"] = med * 1e3, best * 1e3
    out["estimator_report"] = dict(m.importance_report_)
    med, best = _wall(lambda: selectivity_ratio(m, cells=False, device=False), 3)
    out["estimator_torch_ms"], out["estimator_torch_best_ms"] = med * 1e3, best * 1e3
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
