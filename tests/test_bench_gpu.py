"""bench.py on the GPU: a plain run prints the headline line and nothing measured beyond it; --full adds the roofline, box
probe, GPU denominators and (CIFAR-10) the whole-step graph to the same line.  CIFAR-10 at batch 4 keeps each run to seconds."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"roofline", "box", "gpu_denominators", "cpu_baseline", "other_configs"}


def _line(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "cifar", "--images-per-gpu", "4",
                        "--steps", "2", "--warmup", "1", *extra], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(cuda):
    d = _line()
    assert HEADLINE <= d.keys() and not FULL_ONLY & d.keys(), sorted(d)
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert "whole_step_graph_ms" not in d["config"] and "extra_batch" not in d["config"]


@pytest.mark.gpu
def test_full_run_adds_the_measurements_beyond_the_headline(cuda):
    d = _line("--full", "--no-cpu-baseline")
    assert HEADLINE <= d.keys() and {"roofline", "box", "gpu_denominators"} <= d.keys(), sorted(d)
    assert "cpu_baseline" not in d and d["roofline"]["launches_per_eval"] > 0
    assert d["config"]["whole_step_graph_ms"] > 0
