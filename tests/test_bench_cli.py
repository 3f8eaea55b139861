"""bench.py's command line: a plain run reports the headline only; what takes runs of its own (other precisions, parity legs, other
workloads, CPU baseline) is behind `--full`."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BENCH = os.path.join(ROOT, "bench.py")
EXTRAS = ("other_precisions", "parity_vs_oracle", "parity_vs_reference", "other_workloads")


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}


def test_full_is_an_option_off_by_default():
    r = subprocess.run([sys.executable, BENCH, "--help"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only():
    """`bench.py --gpus 1 --steps 1 --warmup 1`: the headline fields, no extras, and little time outside the steps"""
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "1", "--warmup", "1"], env=_env(), capture_output=True, text=True,
                       timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    outside = wall - 2 * line["ms_per_step"] / 1e3
    print({"value": line["value"], "ms_per_step": line["ms_per_step"], "wall_s": wall, "outside_steps_s": outside})
    assert line["unit"] == "rays/s" and line["higher_is_better"] is True and line["value"] > 1e5
    assert line["metric"].startswith("rays_per_sec") and line["dtype"] and line["steps"] == 1 and line["warmup"] == 1
    assert line["roofline"]["launches"] == 1
    assert all(line[k] is None for k in EXTRAS), {k: line[k] is None for k in EXTRAS}
    assert "cpu_baseline" not in line
    assert outside < 60.0, outside
