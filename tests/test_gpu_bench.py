"""GPU tests (``-m gpu``) of bench.py's plain run: the headline alone, --steps timed steps, and --dump-outputs writing
what the last timed step returned - the same arrays from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

B, N, K = 1024, 100, 20


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "5",
           "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(tmp_path):
    rec = _plain_run(tmp_path / "a")
    assert rec["metric"] == "rod-steps/sec (N=100 segments, batch=1024)" and rec["unit"] == "rod-steps/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f64" and rec["steps"] == K and rec["warmup"] == 5
    # exactly --steps timed steps: one timed chunk (after two untimed warm chunks), value and ms_per_step from it
    tc = rec["timed_chunks"]
    assert tc["n"] == 1 and tc["warm_chunks"] == 2 and tc["steps_each"] == K and len(tc["wall_ms"]) == 1
    assert abs(rec["ms_per_step"] - tc["wall_ms"][0] / K) <= 1e-4
    assert rec["value"] > 0 and abs(rec["value"] - B * K / (rec["ms_per_step"] * K * 1e-3)) < 2e-2 * rec["value"]
    assert rec["config"]["unconverged_rod_steps"] == 0
    # nothing but the headline: the CPU baseline, the oracle check and the other configurations are --full's
    for key in ("extra", "cpu_baseline", "cpu_baseline_c", "cold_start", "tip_rel_l2_vs_oracle"):
        assert key not in rec, key

    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(a) == ["base_wrench", "status", "tip", "y", "z"]
    shapes = {"tip": (B, 3), "status": (B,), "base_wrench": (B, 6), "y": (B, 19, N), "z": (B, 6, N)}
    for name, v in a.items():
        assert v.shape == shapes[name] and v.dtype == np.float64 and np.all(np.isfinite(v)), name
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.all(a["status"] == 0)
    # the tip of the last step is the first three rows of the last grid point of the last state
    assert np.abs(a["tip"] - a["y"][:, :3, -1]).max() <= 1e-9 * np.abs(a["y"][:, :3, -1]).max()
    assert np.std(a["tip"][:, 0]) > 1e-4  # rods differ

    # same arguments, same inputs: the same outputs
    _plain_run(tmp_path / "b")
    for name, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (name + ".npy"))), name
