"""CPU-only: bench.py's rank launcher.  `python bench.py --gpus N` must start its own N ranks
when WORLD_SIZE is unset, refuse a WORLD_SIZE that disagrees with --gpus before any GPU call, and exit
non-zero when a rank fails -- a scaling run must never record one GPU's work under n_gpus = N."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_resolve_world_single_rank_without_env():
    assert bench.resolve_world(bench.parse([]), {}) == ("rank", 1)


def test_resolve_world_launches_its_own_ranks():
    assert bench.resolve_world(bench.parse(["--gpus", "4"]), {}) == ("launch", 4)


def test_resolve_world_accepts_a_matching_world():
    assert bench.resolve_world(bench.parse(["--gpus", "8"]), {"WORLD_SIZE": "8"}) == ("rank", 8)


@pytest.mark.parametrize("gpus,ws", [(2, "3"), (1, "2"), (8, "1")])
def test_resolve_world_refuses_a_mismatch(gpus, ws):
    with pytest.raises(SystemExit) as e:
        bench.resolve_world(bench.parse(["--gpus", str(gpus)]), {"WORLD_SIZE": ws})
    assert e.value.code not in (0, None)


def test_launcher_command_is_one_rank_per_gpu_on_localhost():
    cmd = bench.launcher_command(4, ["--gpus", "4", "--steps", "7"], port=29777)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29777"
    assert cmd[-5:] == [os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "7"]


def test_mismatch_exits_non_zero_as_a_process():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert "WORLD_SIZE=3" in p.stderr and p.stdout.strip() == ""


def test_launcher_forwards_a_failing_rank(tmp_path):
    """No GPU here: both ranks die at torch.cuda.set_device; the parent must not print a result and must fail."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode != 0
    assert '"metric"' not in p.stdout


@pytest.mark.parametrize("steps,repeats", [(20, 5), (7, 5), (3, 5), (1, 1), (50, 1), (11, 4)])
def test_window_sizes_add_up_to_exactly_the_timed_steps(steps, repeats):
    sizes = bench.window_sizes(steps, repeats)
    assert sum(sizes) == steps and len(sizes) == min(steps, repeats) and max(sizes) - min(sizes) <= 1


def test_steps_below_one_are_refused_before_any_gpu_call():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--steps" in p.stderr and p.stdout.strip() == ""


def test_dump_outputs_writes_float64_within_the_limit_and_samples_the_same_entries(tmp_path):
    import numpy as np
    rng = np.random.default_rng(1)
    arrays = {"t": rng.normal(size=5000), "w": rng.normal(size=12).astype(np.float32)}
    limit = 2 * 8 * 1000                                     # 1000 float64 entries per array
    bench.dump_outputs(str(tmp_path / "a"), arrays, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), arrays, limit=limit)
    t, w = np.load(tmp_path / "a" / "t.npy"), np.load(tmp_path / "a" / "w.npy")
    assert t.dtype == np.float64 and w.dtype == np.float64
    assert t.size == 1000 and np.isin(t, arrays["t"]).all()
    np.testing.assert_array_equal(w, arrays["w"].astype(np.float64))
    np.testing.assert_array_equal(t, np.load(tmp_path / "b" / "t.npy"))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= limit + 2 * 128   # + the .npy headers
