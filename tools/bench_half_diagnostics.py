"""The read-only diagnostics of a 16-bit model in place (EngineOptions.half_diagnostics) against the float32 upcast route, one process.

  sample_diagnostics     training rows (the training statistics cached by the warm-up call)
  selectivity_ratio      training rows, complete
  sample_contributions   256 training rows
  R2X_literal

at 65536 x 128 x 128, R 10, M 16, for bfloat16 and float16, on the caller's 16-bit device tensor.  Option on: the passes read that
tensor (cmtfpls_resid_rows_* / selectivity_cols_* / contrib_rows_* / recon_r2_* in their 16-bit forms); off: each call first makes
the exact float32 upcast (twice the tensor's bytes) and runs the float32 kernel on it -- the upcast is inside the timed call, as a
user pays it.  Per routine and route: wall time with a device synchronisation over --reps runs (default 7) after one warm-up
(median, min, max) and the rise of the peak allocation over the call; and the kernel alone through the backend, 16-bit on the
tensor and float32 on a prepared upcast (device events, median).  The condition recorded with the numbers: option on is not slower
than off by more than the spread (max - min) of the off route in this same run.  Writes JSON to --out (default
profiles/half_diagnostics.json).

    python tools/bench_half_diagnostics.py [--reps N] [--rows I] [--out PATH]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cmtf_pls_amd import tPLS  # noqa: E402
from cmtf_pls_amd import validate as V  # noqa: E402
from cmtf_pls_amd.engine import EngineOptions  # noqa: E402

DEV = torch.device("cuda:0")
TYPES = {"bf16": (torch.bfloat16, "bfloat16"), "f16": (torch.float16, "float16")}
A, B, R, M = 128, 128, 10, 16


def make_x(I, dtype, seed):
    """(I, A, B) of `dtype`: a rank-4 signal plus noise, built row block by row block (no float32 tensor of the full size)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    W = (torch.randn(4, A, 1, generator=g, device=DEV) * torch.randn(4, 1, B, generator=g, device=DEV)).reshape(4, A * B)
    T = torch.randn(I, 4, generator=g, device=DEV) * torch.tensor([1.0, 0.5, 0.25, 0.125], device=DEV)
    X = torch.empty(I, A * B, dtype=dtype, device=DEV)
    step = max(1, (64 << 20) // (A * B))
    for lo in range(0, I, step):
        X[lo:lo + step] = (T[lo:lo + step] @ W + 0.25 * torch.randn(min(step, I - lo), A * B, generator=g, device=DEV)).to(dtype)
    Y = (T @ torch.randn(4, M, generator=g, device=DEV)).double().cpu().numpy()
    return X.view(I, A, B), Y


def measure(fn, reps):
    """{median, min, max in ms; rise of the peak allocation in bytes} of fn over `reps` runs after one warm-up."""
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
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "peak_rise_bytes": rise}


def kernel_ms(fn, reps):
    """Median device time of fn() in ms (events on the current stream), after one warm-up."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join("profiles", "half_diagnostics.json"))
    a = ap.parse_args()
    I = a.rows
    rows = np.arange(0, I, max(1, I // 256))[:256]
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "shape": [I, A, B], "R": R, "M": M, "contribution_rows": int(rows.size),
              "x_bytes": I * A * B * 2, "float32_copy_bytes": I * A * B * 4}
    routines = {
        "sample_diagnostics": (lambda m, X: V.sample_diagnostics(m), "diagnostics_report_"),
        "selectivity_ratio": (lambda m, X: V.selectivity_ratio(m), "importance_report_"),
        "sample_contributions": (lambda m, X: V.sample_contributions(m, rows=rows), "contributions_report_"),
        "R2X_literal": (lambda m, X: m.R2X_literal(X), "r2x_literal_report_"),
    }
    for kind, (dt, name) in TYPES.items():
        X, Y = make_x(I, dt, 7)
        row = {}
        for label, on in (("half_diagnostics", True), ("upcast", False)):
            m = tPLS(R, dtype=name, algorithm="xcov", options=EngineOptions(half_diagnostics=on))
            m.fit(X, Y)
            out = {}
            for rname, (fn, attr) in routines.items():
                out[rname] = measure(lambda: fn(m, X), a.reps)
                rep = getattr(m, attr)
                out[rname].update(form=rep.get("form"), half_storage=rep.get("half_storage"), storage_fallback=rep.get("storage_fallback"))
                print(kind, label, rname, json.dumps(out[rname]), flush=True)
            row[label] = out
            if not on:                                            # the kernels alone, on the operands of this model
                eng, st = m._get_engine(), m._state
                be, blk = eng.be, st.blocks[0]
                with eng.device_ctx():
                    WA, WB = (w.contiguous() for w in eng._kr_operands(blk, R))
                    X16, X32 = X.view(I, -1), X.view(I, -1).to(torch.float32)
                    T = st.T.contiguous()
                    ridx = torch.from_numpy(rows).to(DEV)
                    Ts, Hs = T.index_select(0, ridx), torch.randn(rows.size, R, dtype=torch.float64, device=DEV)
                    Tau = torch.randn(I, M, dtype=torch.float64, device=DEV)
                    calls = {
                        "sample_diagnostics": lambda Xk: be.resid_rows(Xk, T, WA, WB, blk.mean, True),
                        "selectivity_ratio": lambda Xk: be.selectivity_cols(Xk, Tau, blk.mean, False),
                        "sample_contributions": lambda Xk: be.contrib_rows(Xk, Ts, Hs, WA, WB, blk.mean, ridx),
                        "R2X_literal": lambda Xk: be.recon_r2(Xk, T, WA, WB, blk.mean),
                    }
                    row["kernel_alone_ms"] = {rname: {kind: kernel_ms(lambda: call(X16), a.reps), "f32": kernel_ms(lambda: call(X32), a.reps)}
                                              for rname, call in calls.items()}
                    del X32
                print(kind, "kernel alone", json.dumps(row["kernel_alone_ms"]), flush=True)
            del m
        cond = {}
        for rname in routines:
            on_, off_ = row["half_diagnostics"][rname], row["upcast"][rname]
            spread = off_["ms_max"] - off_["ms_min"]
            cond[rname] = {"time": on_["ms"] / off_["ms"], "on_minus_off_ms": on_["ms"] - off_["ms"], "off_spread_ms": spread,
                           "not_slower_within_spread": on_["ms"] - off_["ms"] <= spread,
                           "peak_rise": on_["peak_rise_bytes"] / max(off_["peak_rise_bytes"], 1)}
        row["half_diagnostics_vs_upcast"] = cond
        result[kind] = row
        del X
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:                                   # after every type: a partial run still leaves its figures
            json.dump(result, f, indent=1)
    print(json.dumps({k: result[k]["half_diagnostics_vs_upcast"] for k in TYPES}))


if __name__ == "__main__":
    main()
