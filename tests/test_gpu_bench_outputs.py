"""bench.py's plain run times its steps and nothing else; `--full` adds the other legs; `--dump-outputs` writes what the
last timed step returned, the same arrays whichever of the two runs it was (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_full_run_adds_the_legs_and_both_dump_the_same_outputs(tmp_path):
    B = 64
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--scans", str(B), "--cpu-sample", "16", "--steady-steps", "4",
            "--no-worlds", "--stage-slam-scans", "4"]
    plain = _run(args + ["--dump-outputs", str(tmp_path / "plain")])
    full = _run(args + ["--full", "--dump-outputs", str(tmp_path / "full")])
    for d in (plain, full):
        assert d["steps"] == 3 and d["warmup"] == 1 and d["n_failed"] == 0 and d["unit"] == "registrations/s"
        assert abs(d["value"] - B * 3 / (d["ms_per_step"] * 3e-3)) < 1e-6 * d["value"]
        assert d["kernels_ms"]["assoc"] > 0
    assert plain["full"] is False and full["full"] is True
    for k in ("value_steady", "value_incl_h2d", "cpu_baseline", "stages", "knn"):
        assert plain[k] is None, k
        assert full[k] is not None, k
    assert plain["kernels_ms"]["fit"] is None and full["kernels_ms"]["fit"] > 0 and full["kernels_ms"]["index_build"] > 0
    assert plain["steady_steps"] == 0 and full["steady_steps"] == 4
    assert full["pose_delta_vs_oracle"]["max_m"] < 1e-4 and full["pose_delta_vs_oracle"]["max_rad"] < 1e-4
    for name, shape in (("poses", (B, 7)), ("status", (B,))):
        a, b = np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))
        assert a.shape == shape and a.dtype == np.float64
        assert np.array_equal(a, b), name
    assert not (np.load(tmp_path / "plain" / "status.npy") != 0).any()
    q = np.load(tmp_path / "plain" / "poses.npy")[:, 3:]                  # (x, y, z, quaternion)
    assert np.allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-9)
