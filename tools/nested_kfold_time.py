"""Time nested K-fold Q2Y at cfg-2: a 65536 x 128 x 128 f32 tensor on the device, M = 16, R = 10, 5 outer x 5 inner folds (30
models, one device pass), and the coupled shape of profiles/kfold_coupled_time.json (the tensor plus a 65536 x 256 f32 matrix
block, a ctPLS).
  (a) the scoring alone: cmtfpls_press_rows_f64 on a 30-model state (T, coef, Q, nu of the shape a pass leaves, random values,
      the eval rows of the real 5 x 5 split) against nested.torch_press, the torch-op scoring of the same state in
      kfold._device_numerators' formulation; median of `--runs` timed runs after a warm-up, with the bytes each moves;
  (b) validate.get_q2y_nested_kfold end to end: the device form against device_folds=False on a model with algorithm="xcov"
      refits and on one with the default algorithm, and the largest differences between their results.
One JSON line (printed, and written to --out when given).

    python tools/nested_kfold_time.py [--runs 5] [--skip-baselines] [--skip-coupled] [--out profiles/nested_kfold_time.json]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/nested_kfold_time.py --skip-baselines --skip-coupled`."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _time(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def _scoring(I, M, R, Ko, Ki, runs):
    """(a): one n = K_o (K_i + 1)-model pass scored by the kernel and by torch ops."""
    from cmtf_pls_amd.backend import HipBackend
    from cmtf_pls_amd.nested import model_rows, nested_fold_ids, torch_press

    be = HipBackend(torch.device("cuda:0"))
    outer, _, inner, _ = nested_fold_ids(I, Ko, Ki, random_state=0)
    _, ev = model_rows(outer, Ko, inner, Ki)
    n = ev.shape[0]
    g = torch.Generator(device="cuda").manual_seed(1)
    T = torch.randn(n, I, R, dtype=torch.float64, device="cuda", generator=g)
    coef = torch.triu(torch.randn(n, R, R, dtype=torch.float64, device="cuda", generator=g)).contiguous()
    Q = torch.randn(n, R, M, dtype=torch.float64, device="cuda", generator=g)
    nu = torch.randn(n, M, dtype=torch.float64, device="cuda", generator=g)
    Y = torch.randn(I, M, dtype=torch.float64, device="cuda", generator=g)
    ev_d = torch.from_numpy(ev).cuda()
    pred_k = torch.zeros(R, I, M, dtype=torch.float64, device="cuda")
    pred_t = torch.zeros_like(pred_k)
    args = (T, coef, Q, nu, Y, ev_d)
    pk = be.press_rows(*args, pred_k)                                                # warm-up of both
    pt = torch_press(*args, pred_t)
    tk = [_time(lambda: be.press_rows(*args, pred_k))[1] for _ in range(runs)]
    tt = [_time(lambda: torch_press(*args, pred_t))[1] for _ in range(runs)]
    scored = int((ev > 0).sum())                                                     # (model, row) pairs scored
    written = int((ev == 2).sum())
    small = n * (R * R + R * M + M) * 8
    return {"models": n, "scored_rows": scored, "predicted_rows": written,
            "kernel_s": statistics.median(tk), "kernel_runs_s": tk, "torch_s": statistics.median(tt), "torch_runs_s": tt,
            # the kernel: every eval word, T and Y of the scored rows, the models' coef / Q / nu, the predictions written once
            "kernel_bytes": ev.size * 4 + scored * (R + M) * 8 + small + written * R * M * 8,
            # torch ops: the same reads, plus five rows x R x M tensors written and read back (the products, their cumsum, + nu,
            # the residual, its square) and the gathered T / Y rows
            "torch_bytes": ev.size * 4 + 2 * scored * (R + M) * 8 + small + 2 * 5 * scored * R * M * 8 + written * R * M * 8,
            "press_max_rel_diff": float(((pk - pt).abs() / pt.abs().clamp_min(1e-300)).max()),
            "pred_max_abs_diff": float((pred_k - pred_t).abs().max())}


def _whole(make, Xs, Y, Ko, Ki, runs, skip_baselines):
    """(b): {device_s, report, results, refit baselines} for one model family: make(algorithm) gives a fitted tPLS / ctPLS."""
    from cmtf_pls_amd.validate import get_q2y_nested_kfold

    m = make(None)
    get_q2y_nested_kfold(m, n_outer=Ko, n_inner=Ki)                                  # warm-up (kernels loaded, allocator primed)
    res, times = None, []
    for _ in range(runs):
        res, dt = _time(lambda: get_q2y_nested_kfold(m, n_outer=Ko, n_inner=Ki, random_state=0))
        times.append(dt)
    out = {"device_s": statistics.median(times), "device_runs_s": times,
           "device_report": {k: v for k, v in m.q2y_report_.items() if k != "n_iter"},
           "n_iter_mean": float(np.mean(m.q2y_report_["n_iter"])), "q2y": res["q2y"], "selected": res["selected"].tolist(),
           "outer_q2y": [float(v) for v in res["outer_q2y"]], "inner_q2y_fold0": [float(v) for v in res["inner_q2y"][0]],
           "optimism": float(res["outer_q2y"].max() - res["q2y"])}
    if skip_baselines:
        return out
    for name, algorithm in (("refits_xcov", "xcov"), ("refits_default", None)):
        r = make(algorithm)
        ref, dt = _time(lambda: get_q2y_nested_kfold(r, n_outer=Ko, n_inner=Ki, random_state=0, device_folds=False))
        out[name + "_s"] = dt
        out[name + "_max_abs_diff"] = {"inner_q2y": float(np.abs(ref["inner_q2y"] - res["inner_q2y"]).max()),
                                       "outer_q2y": float(np.abs(ref["outer_q2y"] - res["outer_q2y"]).max()),
                                       "q2y": abs(ref["q2y"] - res["q2y"]), "selected_equal": bool(np.array_equal(ref["selected"], res["selected"]))}
    out["refits"] = Ko * (Ki + 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-baselines", action="store_true")
    ap.add_argument("--skip-coupled", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cmtf_pls_amd import ctPLS, tPLS
    from cmtf_pls_amd.synthetic import synthetic_shard_device

    I, J, K, Jm, M, R, Ko, Ki = 65536, 128, 128, 256, 16, 10, 5, 5
    out = {"shape": [I, J, K], "M": M, "R": R, "n_outer": Ko, "n_inner": Ki, "runs": args.runs}
    out["scoring"] = _scoring(I, M, R, Ko, Ki, args.runs)
    X, Y, Xm = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0", matrix_block=Jm)
    out["x_bytes"] = X.numel() * X.element_size()

    def make_tpls(algorithm):
        m = tPLS(R, dtype="float32") if algorithm is None else tPLS(R, dtype="float32", algorithm=algorithm)
        m.fit(X, Y)
        return m
    out["tpls"] = _whole(make_tpls, [X], Y, Ko, Ki, args.runs, args.skip_baselines)
    if not args.skip_coupled:
        Xm = Xm.to(torch.float32).contiguous()

        def make_ctpls(algorithm):
            c = ctPLS(R, dtype="float32") if algorithm is None else ctPLS(R, dtype="float32", algorithm=algorithm)
            c.fit([X, Xm], Y)
            return c
        out["matrix_block"] = [I, Jm]
        out["ctpls"] = _whole(make_ctpls, [X, Xm], Y, Ko, Ki, args.runs, args.skip_baselines)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
