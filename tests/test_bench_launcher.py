"""bench.py's multi-GPU launcher (the driver runs ``python bench.py --gpus N``): without a torchrun
environment it spawns N ranks itself (train_v6.py:465-468 mp.spawn), they form a process group and
rank 0 prints one JSON line whose n_gpus is the size of that group.  ``--dry-run`` replaces the GPU
workload with a CPU stub over gloo so the launcher, rendezvous, barrier and max-over-ranks timing
run here without a GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 2])
def test_bench_launches_n_ranks(n):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dry-run", "--steps", "4",
                        "--warmup", "1"], capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == n
    assert rec["steps"] == 4 and rec["warmup"] == 1
    assert rec["config"]["backend"] == ("gloo" if n > 1 else "none")
    assert rec["value"] > 0 and rec["scaling"] == "weak"


def test_dump_outputs_is_reproducible(tmp_path):
    """``--dump-outputs DIR`` writes float32 DIR/<name>.npy after the timed steps; the same arguments
    give the same arrays (seeded inputs).  ``--full`` is accepted and changes nothing of that."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    got = []
    for d, extra in (("a", []), ("b", ["--full"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dry-run", "--steps", "3",
                            "--warmup", "1", "--dump-outputs", str(tmp_path / d), *extra],
                           capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        assert os.listdir(tmp_path / d) == ["stub.npy"]
        got.append(np.load(tmp_path / d / "stub.npy"))
    assert got[0].dtype == np.float32 and got[0].shape == (256, 256) and np.isfinite(got[0]).all()
    np.testing.assert_array_equal(got[0], got[1])


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    """Arrays over the byte budget are cut to a fixed, seeded sample: the same elements every time."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    rng = np.random.default_rng(0)
    arrays = {"big": rng.standard_normal((50, 40)), "ints": np.arange(300, dtype=np.int32)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    total = 0
    for name, src in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and 0 < a.size < src.size
        np.testing.assert_array_equal(a, b)
        assert np.isin(a, src.astype(np.float32)).all()
        total += a.nbytes
    assert total <= 4000
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1 << 20)
    bench.dump_outputs(str(tmp_path / "c"), arrays)
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "ints.npy"), np.arange(300, dtype=np.float32))
