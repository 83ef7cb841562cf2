"""Time the bootstrap of the factors at cfg-2: a 65536 x 128 x 128 f32 tensor on the device, M = 16, R = 10, B = 100 resamples.
validate.bootstrap_factors end to end (the device form: up to 32 resamples per pass, 2R reads of X per pass) against the Python
loop a user would otherwise write: B literal algorithm="xcov" refits (each resample's rows by index_select, fit).  Then the same
two for the coupled shape of DESIGN 8c (the tensor plus a 65536 x 256 f32 matrix block, a ctPLS), and the largest normwise
column difference between the device factors and the refits'.  One timed run of each after a warm-up; one JSON line (printed,
and written to --out when given).

    python tools/bootstrap_time.py [--resamples 100] [--skip-baselines] [--skip-coupled] [--out profiles/bootstrap_time.json]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bootstrap_time.py --skip-baselines --skip-coupled`."""
import argparse
import json
import os
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


def _colwise(a, b):
    return float((np.linalg.norm(a - b, axis=-2) / np.maximum(np.linalg.norm(b, axis=-2), 1e-300)).max())


def _run(m, Xs, R, B, skip_baselines):
    """{device_s, report, baselines} for one fitted model: tPLS (Xs one block) or ctPLS."""
    from cmtf_pls_amd import ctPLS, tPLS
    from cmtf_pls_amd.bootstrap import aligned_factors
    from cmtf_pls_amd.validate import bootstrap_factors

    coupled = isinstance(m, ctPLS)
    bootstrap_factors(m, n_resamples=2)                                              # warm-up (kernels loaded, allocator primed)
    res, dt = _time(lambda: bootstrap_factors(m, n_resamples=B, random_state=0))
    rep = m.bootstrap_report_
    out = {"device_s": dt, "device_report": {k: v for k, v in rep.items() if k != "n_iter"},
           "n_iter_mean": float(np.mean(rep["n_iter"])), "oob_q2y": [float(v) for v in res["oob_q2y"]], "oob_rows": res["oob_rows"]}
    if skip_baselines:
        return out
    Y = m.original_Y
    kind = ctPLS if coupled else tPLS

    def refit(idx):
        """One literal refit; its factors aligned to the fitted model (the refit, which holds its resampled X, is dropped)."""
        r = kind(R, dtype="float32", algorithm="xcov")
        sel = torch.from_numpy(idx).cuda()
        r.fit([X.index_select(0, sel) for X in Xs] if coupled else Xs[0].index_select(0, sel), Y.index_select(0, sel))
        return aligned_factors(m, r)

    refit(res["resamples"][0])                                                       # warm-up of the regular engine
    fits, dt = _time(lambda: [refit(idx) for idx in res["resamples"]])
    out["baseline_refits_xcov_s"] = dt
    out["baseline_refits"] = B
    diff = 0.0
    for b, (modes, Q, coef) in enumerate(fits):
        got = res["X_factors"] if coupled else [res["X_factors"]]
        for bi, bl in enumerate(modes if coupled else [modes]):
            for j, L in enumerate(bl):
                diff = max(diff, _colwise(got[bi][j][b], L))
        diff = max(diff, _colwise(res["Y_loadings"][b], Q), _colwise(res["coef"][b], coef))
    out["factors_max_colwise_diff_vs_refits"] = diff
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resamples", type=int, default=100)
    ap.add_argument("--skip-baselines", action="store_true")
    ap.add_argument("--skip-coupled", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cmtf_pls_amd import ctPLS, tPLS
    from cmtf_pls_amd.synthetic import synthetic_shard_device

    I, J, K, Jm, M, R, B = 65536, 128, 128, 256, 16, 10, args.resamples
    out = {"shape": [I, J, K], "M": M, "R": R, "B": B}
    X, Y, Xm = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0", matrix_block=Jm)
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    out["x_bytes"] = X.numel() * X.element_size()
    out["tpls"] = _run(m, [X], R, B, args.skip_baselines)
    if not args.skip_coupled:
        Xm = Xm.to(torch.float32).contiguous()
        c = ctPLS(R, dtype="float32")
        c.fit([X, Xm], Y)
        out["matrix_block"] = [I, Jm]
        out["ctpls"] = _run(c, [X, Xm], R, B, args.skip_baselines)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
