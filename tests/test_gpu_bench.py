"""bench.py on one GPU: a plain run prints the headline alone, --full adds the measurements that take runs of their own,
and both runs compute the same thing in their timed steps (--dump-outputs byte for byte)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu_lib")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COMMON = ["--gpus", "1", "--steps", "14", "--warmup", "7", "--repeats", "3", "--families", "6000", "--organisms", "200"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*argv):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), check=True, stdout=subprocess.PIPE,
                         timeout=600).stdout.decode()
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench(*COMMON, "--dump-outputs", str(tmp_path / "plain"))
    full = _bench(*COMMON, "--full", "--no-north-star", "--no-extras", "--cpu-iters", "2", "--dump-outputs", str(tmp_path / "full"))
    for rec in (plain, full):
        assert all(key in rec for key in HEADLINE)
        assert rec["metric"] == "em_family_x_organism_cells_per_sec" and rec["value"] > 0 and rec["ms_per_step"] > 0
        assert rec["steps"] == 14 and rec["warmup"] == 7 and rec["graphs_primed"]
        assert rec["roofline"]["whole_iteration_algorithmic_GBps"] > 0
    assert plain["config"] == full["config"] and plain["timed_steps"] == full["timed_steps"]
    # the plain line: nothing that takes runs of its own
    for key in ("cpu_baseline", "north_star_target", "also"):
        assert key not in plain
    assert "kernels" not in plain["roofline"]
    # --full: per-kernel figures and the CPU baseline; its parts still leave out what --no-* names
    assert full["roofline"]["kernels"] and all(r["avg_launch_ms"] > 0 for r in full["roofline"]["kernels"])
    assert full["cpu_baseline"]["value"] > 0 and full["speedup_vs_cpu_baseline"] > 0
    assert "north_star_target" not in full and "also" not in full
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names and names == sorted(os.listdir(tmp_path / "full"))
    for name in names:
        assert np.array_equal(np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name), equal_nan=True), name
