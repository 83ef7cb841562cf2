"""Time K-fold cross-validation of a coupled model: a 65536 x 128 x 128 f32 tensor block plus a 65536 x 256 f32 matrix block
(synthetic_shard_device with matrix_block=256), M = 16, R = 10, K = 5, both blocks on the device.  get_q2y_kfold end to end on a
ctPLS (the device form: 2R reads of each block for all folds) against K literal ctPLS refits from the same device blocks (each
block's training rows by index_select, fit, predict of the held-out rows) with algorithm="xcov" and with algorithm="direct".
Median of repeated windows after a warm-up; one JSON line (printed, and written to --out when given).

    python tools/kfold_coupled_time.py [--reps 5] [--skip-refits] [--out profiles/kfold_coupled_time.json]
Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/kfold_coupled_time.py --reps 1 --skip-refits`."""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cmtf_pls_amd import ctPLS
    from cmtf_pls_amd.kfold import fold_ids
    from cmtf_pls_amd.synthetic import synthetic_shard_device
    from cmtf_pls_amd.validate import get_q2y_kfold

    I, J, K, Jm, M, R, F = 65536, 128, 128, 256, 16, 10, 5
    X, Y, Xm = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0", matrix_block=Jm)
    Xm = Xm.to(torch.float32).contiguous()
    Xs = [X, Xm]
    m = ctPLS(R, dtype="float32")
    m.fit(Xs, Y)
    xbytes = [x.numel() * x.element_size() for x in Xs]

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

    out = {"shapes": [[I, J, K], [I, Jm]], "M": M, "R": R, "K": F, "x_bytes": xbytes}
    q = {}
    out["kfold_s"], out["kfold_runs_s"] = window(lambda: q.setdefault("v", get_q2y_kfold(m, n_splits=F, per_component=True)))
    out["kfold_report"] = {k: v for k, v in m.q2y_report_.items() if k != "n_iter"}
    out["q2y_per_component"] = [float(v) for v in q["v"]]
    if not args.skip_refits:
        ids, _ = fold_ids(I, F)

        def refits(algorithm):
            for k in range(F):
                test = ids == k
                tr = torch.from_numpy(np.flatnonzero(~test)).cuda()
                te = torch.from_numpy(np.flatnonzero(test)).cuda()
                r = ctPLS(R, dtype="float32", algorithm=algorithm)
                r.fit([x.index_select(0, tr) for x in Xs], Y.index_select(0, tr))
                r.predict([x.index_select(0, te) for x in Xs])
        out["refits_xcov_s"], out["refits_xcov_runs_s"] = window(lambda: refits("xcov"))
        out["refits_direct_s"], out["refits_direct_runs_s"] = window(lambda: refits("direct"))
        out["refits_copies_of_blocks"] = F              # per fold: a copy of every block's training rows and of its test rows
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
