"""16-bit storage of X (bfloat16 / float16) against float32, one process, the same values in all three types.

  kernels    cmtfpls_xcov_stats_*, cmtfpls_score_contract_*, cmtfpls_mttkrp_* at 65536 x 128 x 128, M 8, R 10: time and bytes of X per second
  fit        tPLS(10, algorithm="xcov") on the device tensor (in place at 16 bits, on the caller's tensor at float32 too)
  transform  65536 rows of the same tensor (one-pass MTTKRP)
  two-read   the fit at 32768 x 256 x 256 (rows beyond the 16-bit score_contract: mttkrp + xcov per component; float32: split rows)

Median of --reps runs (default 5) after one warm-up, HIP events for the kernels, wall time with a device synchronisation for fit and
transform.  The values are small multiples of 1/8 plus a rank-4 signal rounded to 8 significant bits: exactly representable in
bfloat16, float16 and float32, so the three runs compute on the same numbers.  Every 16-bit figure is printed next to the float32
figure of the same run.  Writes JSON to --out (default profiles/half_storage_time.json).

    python tools/bench_half_storage.py [--reps N] [--rows I] [--skip-two-read] [--out PATH]
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
from cmtf_pls_amd.backend import HipBackend  # noqa: E402

DEV = torch.device("cuda:0")
TYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
NAMES = {"bf16": "bfloat16", "f16": "float16", "f32": "float32"}


def make_x(I, A, B, seed):
    """(I, A, B) float32 whose values are exact in bfloat16 AND float16: rounded to bfloat16 (8 significant bits), then to float16
    (a value that loses bits there loses them for good), row block by row block."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    WA = torch.randn(4, A, generator=g, device=DEV)
    WB = torch.randn(4, B, generator=g, device=DEV)
    W = (WA[:, :, None] * WB[:, None, :]).reshape(4, A * B)
    X = torch.empty(I, A * B, dtype=torch.float32, device=DEV)
    T = torch.randn(I, 4, generator=g, device=DEV)
    step = max(1, (64 << 20) // (A * B))
    for lo in range(0, I, step):
        blk = T[lo:lo + step] @ W + 0.25 * torch.randn(min(step, I - lo), A * B, generator=g, device=DEV)
        X[lo:lo + step] = blk.to(torch.bfloat16).to(torch.float16).to(torch.float32)
    Y = (T @ torch.randn(4, 8, generator=g, device=DEV)).double()
    return X.view(I, A, B), Y


def events(fn, reps):
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


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def kernels(be, X, Y, R, reps):
    I, A, B = X.shape
    X2 = X.view(I, -1)
    P = A * B
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    wA = torch.randn(A, generator=g, device=DEV, dtype=torch.float64)
    wB = torch.randn(B, generator=g, device=DEV, dtype=torch.float64)
    WA = torch.randn(A, R, generator=g, device=DEV, dtype=torch.float64)
    WB = torch.randn(B, R, generator=g, device=DEV, dtype=torch.float64)
    S, t, Z, out = be.empty(Y.shape[1], P), be.empty(I), be.empty(P), be.empty(I, R)
    nbytes = X.numel() * X.element_size()
    res = {}
    for name, fn in (("xcov_stats", lambda: be.xcov_stats(X2, Y, out=S)),
                     ("score_contract", lambda: be.score_contract(X2, A, B, wA, wB, None, t, Z)),
                     ("mttkrp", lambda: be.mttkrp(X2, A, B, WA, WB, out))):
        if fn() is None:
            res[name] = None
            continue
        ms = events(fn, reps)
        res[name] = {"ms": ms, "TB_per_s": nbytes / ms / 1e9, "Gelem_per_s": X.numel() / ms / 1e6}
    return res


def compare(table):
    """Every 16-bit figure as a ratio to float32 of the same run."""
    out = {}
    for kind in ("bf16", "f16"):
        out[kind] = {}
        for key, v in table[kind].items():
            ref = table["f32"].get(key)
            if isinstance(v, dict) and isinstance(ref, dict) and "ms" in v and "ms" in ref:
                out[kind][key] = {"time_vs_f32": v["ms"] / ref["ms"], "bytes_per_s_vs_f32": v["TB_per_s"] / ref["TB_per_s"]}
            elif isinstance(v, float) and isinstance(ref, float):
                out[kind][key] = {"time_vs_f32": v / ref}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--skip-two-read", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "half_storage_time.json"))
    a = ap.parse_args()
    be = HipBackend(DEV)
    R = 10
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "shape": [a.rows, 128, 128], "R": R, "M": 8}
    X32, Y = make_x(a.rows, 128, 128, 7)
    Yh = Y.cpu().numpy()
    table = {}
    for kind, dt in TYPES.items():
        X = X32 if dt is torch.float32 else X32.to(dt)
        assert torch.equal(X.to(torch.float32), X32)                          # the same values in every type
        row = kernels(be, X, Y, R, a.reps)
        m = tPLS(R, dtype=NAMES[kind], algorithm="xcov", backend=be)
        row["fit_ms"] = wall(lambda: m.fit(X, Yh), a.reps)
        rep = m.fit_report_
        row["fit_path"] = {"raw": rep.get("raw"), "x_passes_per_component": rep.get("x_passes_per_component"),
                           "half_storage": rep.get("half_storage"), "n_iter": list(m.n_iter_)}
        row["transform_ms"] = wall(lambda: m.transform(X), a.reps)
        row["transform_form"] = m.projection_report_["form"]
        table[kind] = row
        print(kind, json.dumps(row), flush=True)
        del X, m
    result["kernels_fit_transform"] = table
    result["vs_f32"] = compare(table)
    del X32
    torch.cuda.empty_cache()
    if not a.skip_two_read:
        X32, Y = make_x(a.rows // 2, 256, 256, 11)
        Yh = Y.cpu().numpy()
        two = {}
        for kind, dt in TYPES.items():
            X = X32 if dt is torch.float32 else X32.to(dt)
            m = tPLS(R, dtype=NAMES[kind], algorithm="xcov", backend=be)
            ms = wall(lambda: m.fit(X, Yh), max(1, min(a.reps, 3)))
            rep = m.fit_report_
            two[kind] = {"fit_ms": ms, "x_passes_per_component": rep.get("x_passes_per_component"), "half_storage": rep.get("half_storage"),
                         "n_iter": list(m.n_iter_)}
            print("two-read", kind, json.dumps(two[kind]), flush=True)
            del X, m
        result["two_read_32768x256x256"] = two
        result["two_read_vs_f32"] = {k: two[k]["fit_ms"] / two["f32"]["fit_ms"] for k in ("bf16", "f16")}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"vs_f32": result["vs_f32"], "two_read_vs_f32": result.get("two_read_vs_f32")}))


if __name__ == "__main__":
    main()
