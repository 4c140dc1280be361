"""bench.py --dump-outputs and --steps, host side: what the last timed step returned lands in DIR/<name>.npy as float32,
within the 64 MB cap (a fixed, seeded sample of batch rows above it); --steps below 1 is refused.  No GPU here."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench                                                        # the repository root is on sys.path (conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrays(seed):
    g = torch.Generator().manual_seed(seed)
    return {"x_prev": torch.randn(8, 4, 16, 16, generator=g), "pred_x0": torch.randn(8, 4, 16, 16, generator=g),
            "eps": torch.randn(8, 4, 16, 16, generator=g).half()}


def test_dump_outputs_writes_every_array_as_float32(tmp_path):
    arrays = _arrays(0)
    info = bench.dump_outputs(str(tmp_path / "d"), arrays, 1, 0, None)
    assert sorted(os.listdir(tmp_path / "d")) == ["eps.npy", "pred_x0.npy", "x_prev.npy"]
    assert info["rows"] is None and info["arrays"] == {k: list(v.shape) for k, v in arrays.items()}
    for name, t in arrays.items():
        got = np.load(tmp_path / "d" / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, t.float().numpy())


def test_dump_outputs_samples_the_same_rows_above_the_cap(tmp_path, monkeypatch):
    arrays = _arrays(1)
    per_row = sum(t[0].numel() * 4 for t in arrays.values())
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 3 * per_row)
    a = bench.dump_outputs(str(tmp_path / "a"), arrays, 1, 0, None)
    b = bench.dump_outputs(str(tmp_path / "b"), _arrays(2), 1, 0, None)
    assert a["rows"] == b["rows"] and len(a["rows"]) == 3 and a["rows"] == sorted(set(a["rows"]))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 3 * per_row + 3 * 256                        # + the .npy headers
    for name, t in arrays.items():
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), t.float()[a["rows"]].numpy())


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--launch-check"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr
