"""bench.py's two kinds of run: a plain one does only what the headline needs, --full adds everything else."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, *argv):
    import bench  # cheap: torch is only imported in main()
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_full_is_off_by_default(monkeypatch):
    assert _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "1").full is False
    assert _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "1", "--full").full is True


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only():
    """A plain run: the headline fields, consistent with each other, and null where only --full measures."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--chains", "1024"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["unit"] == "evals/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["metric"].startswith("ODE-solve+likelihood evals/sec") and out["steps"] == 3 and out["warmup"] == 1
    assert abs(out["value"] - 1024 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    assert out["status_counts"][0] == 1024
    assert out["config"]["full"] is False
    for k in ("value_strict", "roofline", "cpu_baseline", "other_workloads", "sampler_pipeline"):
        assert out[k] is None, k
    assert out["config"]["other_arith"] is None
