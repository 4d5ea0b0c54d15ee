"""bench.py's own contract: a plain run prints the headline line without the --full side measurements, --steps sets
the timed steps, and --dump-outputs writes the last step's result from seeded inputs (the same on every run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_small_result_whole(tmp_path):
    s = torch.randn(300, 300, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path), {"sandwich": s, "f32": s.float(), "i32": torch.arange(7, dtype=torch.int32)})
    assert np.array_equal(np.load(tmp_path / "sandwich.npy"), s.numpy())
    f32 = np.load(tmp_path / "f32.npy")
    assert f32.dtype == np.float32 and np.array_equal(f32, s.float().numpy())
    i32 = np.load(tmp_path / "i32.npy")
    assert i32.dtype == np.float64 and np.array_equal(i32, np.arange(7.0))


def test_dump_outputs_large_result_fixed_sample_under_64mb(tmp_path):
    # a 4000 x 4000 float64 sandwich is 128 MB (the 'sparse_wide' design's 10k x 10k: 800 MB): a seeded sample
    s = torch.randn(4000, 4000, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "a"), {"sandwich": s})
    bench.dump_outputs(str(tmp_path / "b"), {"sandwich": s})
    a, b = np.load(tmp_path / "a" / "sandwich.npy"), np.load(tmp_path / "b" / "sandwich.npy")
    assert os.path.getsize(tmp_path / "a" / "sandwich.npy") < 64 << 20
    assert np.array_equal(a, b) and a.ndim == 1 and a.size > 1_000_000
    pos = np.unique(np.random.default_rng(0).integers(0, s.numel(), bench.DUMP_SAMPLE_ENTRIES))
    assert np.array_equal(a, s.numpy().reshape(-1)[pos])


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--breakdown"]])
def test_bench_rejects_bad_arguments(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit) as e:
        bench.parse_args()
    assert e.value.code == 2


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """Two plain runs with the same arguments: the line holds the headline keys and none of --full's, `steps` is the
    number asked for, and both runs dump the same p x p sandwich (seeded inputs; only the summation order of the
    kernels' atomics may differ)."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    lines, dumps = [], []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", "200000",
                              "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / run)],
                             env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        lines.append(json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1]))
        dumps.append(np.load(tmp_path / run / "sandwich.npy"))
    r = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["steps"] == 4 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0
    assert r["unit"] == "GB/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
    for k in ("roofline", "cpu_baseline", "matvec", "ms_per_step_min", "ms_per_step_hipgraph", "ingest_rebuild_ms"):
        assert k not in r, k
    a, b = dumps
    p = r["config"]["p"]
    assert a.shape == (p, p) and a.dtype == np.float64 and np.isfinite(a).all()
    scale = np.abs(a).max()
    assert np.abs(a - a.T).max() <= 1e-12 * scale
    assert np.abs(a - b).max() <= 1e-12 * scale
