"""Time the sparse rank-1 extraction (cmtfpls_rank1_sparse_f64) next to the dense one, and a sparse fit next to a dense fit.
  kernel   128 x 128 (Z staged in LDS, form 1) and 256 x 256 (Z streamed, form 2), lambda = 0.2 on both modes, default sweep tolerance:
           the dense extraction (cmtfpls_rank1_f64) alone, and the dense extraction followed by the sparse sweeps, as the engine issues
           them; the sparse kernel's own time is the difference and is also timed alone on the dense pair (HIP events)
  fit      cfg-2 (65536 x 128 x 128 f32, M 16, R 10), sec-to-fit of tPLS.fit on the device tensor: dense direct / xcov, and
           sparsity = 0.2 direct / xcov (the fused forms a sparse fit does not take are the difference in the launch sequence)
Every figure is the median of five after one warm-up.  Recorded, not gated.  One JSON line (printed, and written to --out).

    python tools/bench_sparse_rank1.py [--rows 65536] [--out profiles/sparse_rank1_time.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPS = 5


def _event(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def _median(fn, timer):
    fn()                                                           # one warm-up
    torch.cuda.synchronize()
    return float(np.median([timer(fn) for _ in range(REPS)]))


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cmtf_pls_amd import tPLS
    from cmtf_pls_amd.backend import HipBackend
    from cmtf_pls_amd.synthetic import synthetic_shard_device

    be = HipBackend()
    out = {"reps": REPS, "lambda": 0.2, "kernel": {}, "fit": {}}
    for n in (128, 256):
        rng = np.random.default_rng(n)
        u, v = rng.normal(size=n) * (rng.random(n) < 0.6), rng.normal(size=n) * (rng.random(n) < 0.6)
        Z = torch.from_numpy(4.0 * np.outer(u / np.linalg.norm(u), v / np.linalg.norm(v)) + 0.3 * rng.normal(size=(n, n)) / np.sqrt(n)).to(be.device)
        wA, wB, info, sinfo = be.empty(n), be.empty(n), be.zeros(2), be.zeros(2)
        dA, dB = be.empty(n), be.empty(n)
        be.rank1(Z.view(-1), n, n, dA, dB, info=info)

        def dense():
            be.rank1(Z.view(-1), n, n, wA, wB, info=info)

        def both():
            be.rank1(Z.view(-1), n, n, wA, wB, info=info)
            be.rank1_sparsify(Z.view(-1), n, n, wA, wB, 0.2, 0.2, sinfo)

        def sparse_alone():
            wA.copy_(dA)
            wB.copy_(dB)
            be.rank1_sparsify(Z.view(-1), n, n, wA, wB, 0.2, 0.2, sinfo)

        def copies():
            wA.copy_(dA)
            wB.copy_(dB)

        t_dense, t_both = _median(dense, _event), _median(both, _event)
        t_alone, t_copy = _median(sparse_alone, _event), _median(copies, _event)
        both()                                                     # (the copies ran last: leave the sparse pair for the counts below)
        torch.cuda.synchronize()
        out["kernel"][f"{n}x{n}"] = {
            "form": be.rank1_sparse_form(n, n), "dense_us": t_dense * 1e6, "dense_plus_sparse_us": t_both * 1e6,
            "sparse_alone_us": (t_alone - t_copy) * 1e6, "sweeps": int(sinfo[1].item()), "converged": bool(sinfo[0].item() > 0.5),
            "dense_squarings": int(info[1].item()), "nonzeros": [int((wA != 0).sum().item()), int((wB != 0).sum().item())]}

    I, J, K, M, R = args.rows, 128, 128, 16, 10
    X, Y = synthetic_shard_device((I, J, K), M, R, error=0.1, seed=215, device="cuda:0")[:2]
    out["fit"]["shape"] = [I, J, K, M, R]
    for algorithm in ("direct", "xcov"):
        for name, sparsity in (("dense", None), ("sparse", 0.2)):
            m = tPLS(R, dtype="float32", algorithm=algorithm, sparsity=sparsity)
            sec = _median(lambda: m.fit(X, Y), _wall)
            rep = m.fit_report_
            entry = {"sec_to_fit": sec, "n_iter": [int(v) for v in m.n_iter_], "R2Y": float(m.R2Y[-1])}
            if sparsity is not None:
                sp = rep["sparse"]
                entry.update(sweeps_max=sp["sweeps_max"], sweeps_total=sp["sweeps_total"], unconverged=sp["unconverged"],
                             nonzeros_last=[L[-1] for L in sp["nonzeros"][0]], form=sp["form"])
            out["fit"][f"{name}_{algorithm}"] = entry
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
