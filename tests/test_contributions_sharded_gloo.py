"""Contribution plots of a sharded fit (world size 2 over gloo on CPU, NumPy test backend): rows stay local, nothing new is
reduced (the training statistics are the cached, all-reduced ones), and the ranks' rows of every array, concatenated, equal the
single-process result."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("scores", "t2", "t2_closure", "spe")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _data(case):
    import oracle as O

    x, y, cp = O.import_synthetic((60, 8, 6), 3, 3, error=0.2, seed=21)
    if case == "nan":
        x[np.random.default_rng(3).random(x.shape) < 0.1] = np.nan
    xn, yn, _ = O.import_synthetic((20, 8, 6), 3, 3, error=0.2, seed=22)
    return x, y, xn, yn


def _diagnose(m, xn, yn):
    from cmtf_pls_amd.validate import sample_contributions

    return sample_contributions(m), sample_contributions(m, xn)


def _worker(rank, world, port, case, ret):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cmtf_pls_amd import tPLS
        from cmtf_pls_amd.engine import Comm
        from numpy_backend import NumpyBackend

        x, y, xn, yn = _data(case)
        rows, nrows = slice(rank * 30, (rank + 1) * 30), slice(rank * 10, (rank + 1) * 10)
        m = tPLS(3, backend=NumpyBackend(), comm=Comm())
        m.fit(x[rows], y[rows])
        ret[rank] = [{k: v for k, v in d.items()} for d in _diagnose(m, xn[nrows], yn[nrows])]
    except Exception as e:  # noqa: BLE001
        import traceback
        ret[rank] = traceback.format_exc() + repr(e)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", ["plain", "nan"])
def test_world2_rows_concatenate_to_the_single_process_result(case):
    sys.path.insert(0, HERE)
    from cmtf_pls_amd import tPLS
    from numpy_backend import NumpyBackend

    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(2, _free_port(), case, ret), nprocs=2, join=True)
        got = dict(ret)
    assert all(isinstance(got[r], list) for r in (0, 1)), got
    x, y, xn, yn = _data(case)
    m = tPLS(3, backend=NumpyBackend())
    m.fit(x, y)
    for which, want in enumerate(_diagnose(m, xn, yn)):
        parts = [got[0][which], got[1][which]]
        for k in KEYS:
            np.testing.assert_allclose(np.concatenate([p[k] for p in parts]), want[k], rtol=1e-6, atol=1e-8, err_msg=k)
        for key in ("spe_mode", "t2_mode"):
            for k in range(2):
                np.testing.assert_allclose(np.concatenate([p[key][k] for p in parts]), want[key][k], rtol=1e-6, atol=1e-8,
                                           err_msg=f"{key}[{k}]")
