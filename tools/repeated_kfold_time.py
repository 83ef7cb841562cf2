"""Time repeated K-fold Q2Y at cfg-2: a 65536 x 128 x 128 f32 tensor on the device, M = 16, R = 10, K = 5, S = 10 splits.
validate.get_q2y_repeated_kfold end to end (the device form: floor(32 / K) splits x K folds per pass, G + 2R - 1 reads of X per
pass) against the two Python loops a user would otherwise write:
  * S x get_q2y_kfold(folds=ids_g) (the K-fold device form per split);
  * S x K literal algorithm="xcov" refits (each fold's training rows by index_select, fit, predict of the held-out rows).
Then the same three for the coupled shape of DESIGN 8c (the tensor plus a 65536 x 256 f32 matrix block, a ctPLS), and the largest
difference between the device Q2Y and the first baseline's.  One timed run of each after a warm-up; one JSON line (printed, and
written to --out when given).

    python tools/repeated_kfold_time.py [--repeats 10] [--skip-baselines] [--skip-coupled] [--out profiles/repeated_kfold_time.json]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/repeated_kfold_time.py --skip-baselines --skip-coupled`."""
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


def _run(m, Xs, R, F, S, skip_baselines):
    """{device_s, report, q2y, baselines} for one fitted model: tPLS (Xs one block) or ctPLS."""
    from cmtf_pls_amd import ctPLS, tPLS
    from cmtf_pls_amd.validate import get_q2y_kfold, get_q2y_repeated_kfold

    coupled = isinstance(m, ctPLS)
    get_q2y_repeated_kfold(m, n_splits=F, n_repeats=2)                               # warm-up (kernels loaded, allocator primed)
    res, dt = _time(lambda: get_q2y_repeated_kfold(m, n_splits=F, n_repeats=S, random_state=0, per_component=True))
    out = {"device_s": dt, "device_report": {k: v for k, v in m.q2y_report_.items() if k != "n_iter"},
           "q2y_mean": [float(v) for v in res["mean"]], "q2y_std": [float(v) for v in res["std"]], "one_se": res["one_se"]}
    if skip_baselines:
        return out
    get_q2y_kfold(m, n_splits=F)                                                     # warm-up of the K-fold form
    q, dt = _time(lambda: [get_q2y_kfold(m, folds=ids, per_component=True) for ids in res["folds"]])
    out["baseline_kfold_s"] = dt
    out["q2y_max_abs_diff_vs_kfold"] = float(np.abs(np.stack(q) - res["q2y"]).max())
    Y = m.original_Y

    def refits():
        for ids in res["folds"]:
            for k in range(F):
                test = ids == k
                tr = torch.from_numpy(np.flatnonzero(~test)).cuda()
                te = torch.from_numpy(np.flatnonzero(test)).cuda()
                if coupled:
                    r = ctPLS(R, dtype="float32", algorithm="xcov")
                    r.fit([X.index_select(0, tr) for X in Xs], Y.index_select(0, tr))
                    r.predict([X.index_select(0, te) for X in Xs])
                else:
                    r = tPLS(R, dtype="float32", algorithm="xcov")
                    r.fit(Xs[0].index_select(0, tr), Y.index_select(0, tr))
                    r.predict(Xs[0].index_select(0, te))

    out["baseline_refits_xcov_s"] = _time(refits)[1]
    out["baseline_refits"] = S * F
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--skip-baselines", action="store_true")
    ap.add_argument("--skip-coupled", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cmtf_pls_amd import ctPLS, tPLS
    from cmtf_pls_amd.synthetic import synthetic_shard_device

    I, J, K, Jm, M, R, F, S = 65536, 128, 128, 256, 16, 10, 5, args.repeats
    out = {"shape": [I, J, K], "M": M, "R": R, "K": F, "S": S}
    X, Y, Xm = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0", matrix_block=Jm)
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    out["x_bytes"] = X.numel() * X.element_size()
    out["tpls"] = _run(m, [X], R, F, S, args.skip_baselines)
    if not args.skip_coupled:
        Xm = Xm.to(torch.float32).contiguous()
        c = ctPLS(R, dtype="float32")
        c.fit([X, Xm], Y)
        out["matrix_block"] = [I, Jm]
        out["ctpls"] = _run(c, [X, Xm], R, F, S, args.skip_baselines)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
