"""bench.py plumbing that needs no GPU: the PMC traffic lookup must find the dominant kernel in the committed
profile (a silent null was VERDICT r01 item 7), and `python bench.py --gpus N` must start N ranks by itself."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_pmc_traffic_finds_the_dominant_kernel():
    import bench
    traffic, src = bench.pmc_traffic(bench.ASSOC_KERNEL_PREFIX)
    assert traffic is not None and traffic > 0 and src
    with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
        keys = list(json.load(f)["kernels"])
    assert any(k.startswith(bench.ASSOC_KERNEL_PREFIX) for k in keys)


def test_pmc_traffic_fails_loudly_on_a_missing_kernel():
    import bench
    import pytest
    with pytest.raises(KeyError):
        bench.pmc_traffic("no_such_kernel")


def test_dump_outputs_writes_floats_and_samples_rows_above_the_limit(tmp_path, monkeypatch):
    """--dump-outputs: f64 (f32 kept) .npy per output; above the size limit the same seeded rows of every array, and their numbers."""
    import bench
    import numpy as np
    poses = np.arange(1000 * 7, dtype=np.float64).reshape(1000, 7)
    status = (np.arange(1000) % 3).astype(np.int32)
    bench.dump_outputs(str(tmp_path / "all"), {"poses": poses, "status": status})
    assert sorted(os.listdir(tmp_path / "all")) == ["poses.npy", "status.npy"]
    assert np.array_equal(np.load(tmp_path / "all" / "poses.npy"), poses)
    s = np.load(tmp_path / "all" / "status.npy")
    assert s.dtype == np.float64 and np.array_equal(s, status)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"poses": poses, "status": status})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["poses.npy", "sample_rows.npy", "status.npy"]
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in files) <= 20000
    rows = np.load(tmp_path / "a" / "sample_rows.npy").astype(np.int64)
    assert 0 < len(rows) < 1000 and np.array_equal(np.load(tmp_path / "a" / "poses.npy"), poses[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "status.npy"), status[rows])
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_plain_gpus_2_launches_two_ranks():
    """No GPU here: every rank must get as far as bench.py's own "needs a GPU" exit, i.e. the plain
    `python bench.py --gpus 2` form launched ranks instead of refusing to run."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES=""))
    err = out.stderr + out.stdout
    assert "launch with torch.distributed.run" not in err
    # the elastic agent SIGTERMs the other rank as soon as the first one exits, so only ONE rank is certain to get its
    # message out; that two ranks were started shows in the agent's failure report (one entry per rank)
    assert err.count("bench.py needs a GPU") >= 1, err[-2000:]
    assert "local_rank: 0" in err and "local_rank: 1" in err, err[-2000:]
    assert out.returncode != 0
