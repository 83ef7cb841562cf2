"""Time K-fold cross-validation on the cfg-2 shape (65536 x 128 x 128 f32, M = 16, R = 10, K = 5, device-resident X):
get_q2y_kfold end to end (the device form: 2R reads of X for all folds) against K literal refits from the same device tensor
(X[train] by index_select, fit, predict of X[test]) with algorithm="xcov" (the fastest fit the package has: no-write, one read of X
per component) and with the default algorithm="direct".  Median of repeated windows after a warm-up; one JSON line.

    python tools/kfold_time.py [--reps 5] [--skip-refits]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/kfold_time.py --reps 1 --skip-refits`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-refits", action="store_true")
    args = ap.parse_args()
    from cmtf_pls_amd import tPLS
    from cmtf_pls_amd.kfold import fold_ids
    from cmtf_pls_amd.synthetic import synthetic_shard_device
    from cmtf_pls_amd.validate import get_q2y_kfold

    I, J, K, M, R, F = 65536, 128, 128, 16, 10, 5
    X, Y = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0")
    m = tPLS(R, dtype="float32")
    m.fit(X, Y)
    xbytes = X.numel() * X.element_size()

    def window(fn):
        fn()                                        # warm-up
        ts = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), ts

    out = {"shape": [I, J, K], "M": M, "R": R, "K": F, "x_bytes": xbytes}
    q = {}
    out["kfold_s"], out["kfold_runs_s"] = window(lambda: q.setdefault("v", get_q2y_kfold(m, n_splits=F, per_component=True)))
    out["kfold_report"] = {k: v for k, v in m.q2y_report_.items() if k != "n_iter"}
    out["kfold_x_reads"] = 2 * R
    out["q2y_per_component"] = [float(v) for v in q["v"]]
    if not args.skip_refits:
        ids, _ = fold_ids(I, F)

        def refits(algorithm):
            for k in range(F):
                test = ids == k
                tr = torch.from_numpy(np.flatnonzero(~test)).cuda()
                te = torch.from_numpy(np.flatnonzero(test)).cuda()
                r = tPLS(R, dtype="float32", algorithm=algorithm)
                r.fit(X.index_select(0, tr), Y.index_select(0, tr))
                r.predict(X.index_select(0, te))
        out["refits_xcov_s"], out["refits_xcov_runs_s"] = window(lambda: refits("xcov"))
        out["refits_direct_s"], out["refits_direct_runs_s"] = window(lambda: refits("direct"))
        # per fold: a copy of the training rows (read of ~0.8 X + write), the fit's reads (the no-write xcov path reads X R + 1
        # times, the direct loop more), a copy and read of the test rows for predict
        out["refits_copies_of_x"] = F
    print(json.dumps(out))


if __name__ == "__main__":
    main()
