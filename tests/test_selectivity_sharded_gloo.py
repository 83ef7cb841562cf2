"""Selectivity ratios of a sharded fit (world size 2 over gloo on CPU, NumPy test backend, uneven rows): rows stay local, the sums
a, d, s, n and sum tau^2 are all-reduced before any ratio, so every rank returns the single-process result: the float64
restatement (tests/selectivity_ref.py) on all the rows with the sharded model's own factors, to 1e-12 of the column's sum of
squares, and the same f_limit (its I is the training rows over every rank)."""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
SPLIT = 37                                                   # rank 0: rows [0, 37), rank 1: rows [37, 60)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _data(case):
    import oracle as O

    x, y, _ = O.import_synthetic((60, 8, 6), 3, 3, error=0.2, seed=21)
    if case == "nan":
        x[np.random.default_rng(3).random(x.shape) < 0.1] = np.nan
    return x, y


def _worker(rank, world, port, case, ret):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cmtf_pls_amd import tPLS
        from cmtf_pls_amd.engine import Comm
        from cmtf_pls_amd.validate import selectivity_ratio
        from numpy_backend import NumpyBackend

        x, y = _data(case)
        rows = slice(0, SPLIT) if rank == 0 else slice(SPLIT, 60)
        m = tPLS(3, backend=NumpyBackend(), comm=Comm())
        m.fit(x[rows], y[rows])
        g = selectivity_ratio(m)
        model = {"T": m.X_factors[0], "loadings": m.X_factors[1:], "X_mean": m.X_mean, "coef_": m.coef_, "Q": m.Y_factors[1]}
        ret[rank] = {"result": dict(g), "model": model, "report": dict(m.importance_report_)}
    except Exception as e:  # noqa: BLE001
        import traceback
        ret[rank] = traceback.format_exc() + repr(e)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", ["plain", "nan"])
def test_world2_uneven_rows_equal_the_single_process_result(case):
    sys.path.insert(0, HERE)
    from selectivity_ref import check, f_limit, selectivity

    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(2, _free_port(), case, ret), nprocs=2, join=True)
        got = dict(ret)
    assert all(isinstance(got[r], dict) for r in (0, 1)), got
    x, _ = _data(case)
    mod = got[0]["model"]
    whole = types.SimpleNamespace(X_factors=[np.concatenate([got[0]["model"]["T"], got[1]["model"]["T"]])] + list(mod["loadings"]),
                                  X_mean=mod["X_mean"], coef_=mod["coef_"], Y_factors=[None, mod["Q"]])
    want = selectivity(whole, train=x)
    for r in (0, 1):
        g = got[r]["result"]
        check(g, want, False, 1e-12)
        assert g["f_limit"] == f_limit(60) and got[r]["report"]["training_rows"] == 60
        assert got[r]["report"]["rows"] == (SPLIT if r == 0 else 60 - SPLIT)
        for key in ("sr", "explained", "residual", "tp_loading", "n_observed"):
            np.testing.assert_array_equal(g[key], got[0]["result"][key])                      # every rank: the same bits
