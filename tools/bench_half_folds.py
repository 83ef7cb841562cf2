"""Cross-validation and bootstrap of a 16-bit model in place (EngineOptions.half_folds) against the float32 upcast route, one process.

  get_q2y_kfold      K = 5 folds
  bootstrap_factors  32 resamples

at 65536 x 128 x 128, M 8, R 10, for bfloat16 and float16, on the caller's 16-bit device tensor.  `half_folds` on: the passes read
that tensor (cmtfpls_kfold_xcov_* / kfold_weighted_xcov_*, cmtfpls_mttkrp_*, cmtfpls_xcov_* in their 16-bit forms); off: each call
first makes the exact float32 upcast (twice the tensor's bytes) and runs the float32 kernels on it -- the upcast is inside the
timed call, as a user pays it.  Wall time with a device synchronisation, median of --reps runs (default 5) after one warm-up, and
the rise of the peak allocation over the call (torch.cuda.max_memory_allocated).  Recorded, not gated: the S builds are bound by
the vector ALU and the f64 matrix cores, not by bytes, so no speed-up is promised.  Writes JSON to --out (default
profiles/half_folds_time.json).

    python tools/bench_half_folds.py [--reps N] [--rows I] [--resamples B] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cmtf_pls_amd import tPLS  # noqa: E402
from cmtf_pls_amd import validate as V  # noqa: E402
from cmtf_pls_amd.engine import EngineOptions  # noqa: E402

DEV = torch.device("cuda:0")
TYPES = {"bf16": (torch.bfloat16, "bfloat16"), "f16": (torch.float16, "float16")}


def make_x(I, A, B, dtype, seed):
    """(I, A, B) of `dtype`: a rank-4 signal plus noise, built row block by row block (no float32 tensor of the full size)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    W = (torch.randn(4, A, 1, generator=g, device=DEV) * torch.randn(4, 1, B, generator=g, device=DEV)).reshape(4, A * B)
    T = torch.randn(I, 4, generator=g, device=DEV) * torch.tensor([1.0, 0.5, 0.25, 0.125], device=DEV)
    X = torch.empty(I, A * B, dtype=dtype, device=DEV)
    step = max(1, (64 << 20) // (A * B))
    for lo in range(0, I, step):
        X[lo:lo + step] = (T[lo:lo + step] @ W + 0.25 * torch.randn(min(step, I - lo), A * B, generator=g, device=DEV)).to(dtype)
    Y = (T @ torch.randn(4, 8, generator=g, device=DEV)).double().cpu().numpy()
    return X.view(I, A, B), Y


def measure(fn, reps):
    """(median ms, rise of the peak allocation in bytes) of fn over `reps` runs after one warm-up."""
    fn()
    torch.cuda.synchronize()
    ms, rise = [], 0
    for _ in range(reps):
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        rise = max(rise, torch.cuda.max_memory_allocated() - base)
    return statistics.median(ms), rise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--resamples", type=int, default=32)
    ap.add_argument("--out", default=os.path.join("profiles", "half_folds_time.json"))
    a = ap.parse_args()
    R, K = 10, 5
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "shape": [a.rows, 128, 128], "R": R, "M": 8, "K": K,
              "resamples": a.resamples, "x_bytes": a.rows * 128 * 128 * 2, "float32_copy_bytes": a.rows * 128 * 128 * 4}
    for kind, (dt, name) in TYPES.items():
        X, Y = make_x(a.rows, 128, 128, dt, 7)
        row = {}
        for label, on in (("half_folds", True), ("upcast", False)):
            m = tPLS(R, dtype=name, algorithm="xcov", options=EngineOptions(half_folds=on))
            m.fit(X, Y)
            out = {}
            ms, rise = measure(lambda: V.get_q2y_kfold(m, n_splits=K, per_component=True), a.reps)
            rep = m.q2y_report_
            out["get_q2y_kfold"] = {"ms": ms, "peak_rise_bytes": rise, "form": rep.get("form"), "half_storage": rep.get("half_storage"),
                                    "storage_fallback": rep.get("storage_fallback"), "why": rep.get("why")}
            print(kind, label, "get_q2y_kfold", json.dumps(out["get_q2y_kfold"]), flush=True)
            ms, rise = measure(lambda: V.bootstrap_factors(m, n_resamples=a.resamples, random_state=5), a.reps)
            rep = m.bootstrap_report_
            out["bootstrap_factors"] = {"ms": ms, "peak_rise_bytes": rise, "form": rep.get("form"), "passes": rep.get("passes"),
                                        "half_storage": rep.get("half_storage"), "storage_fallback": rep.get("storage_fallback"),
                                        "why": rep.get("why")}
            print(kind, label, "bootstrap_factors", json.dumps(out["bootstrap_factors"]), flush=True)
            row[label] = out
            del m
        row["half_folds_vs_upcast"] = {d: {"time": row["half_folds"][d]["ms"] / row["upcast"][d]["ms"],
                                           "peak_rise": row["half_folds"][d]["peak_rise_bytes"] / max(row["upcast"][d]["peak_rise_bytes"], 1)}
                                       for d in ("get_q2y_kfold", "bootstrap_factors")}
        result[kind] = row
        del X
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:                                   # after every type: a partial run still leaves its figures
            json.dump(result, f, indent=1)
    print(json.dumps({k: result[k]["half_folds_vs_upcast"] for k in TYPES}))


if __name__ == "__main__":
    main()
