"""bench.py's plain run and --dump-outputs: the plain line carries the headline figures and none of the legs
that --full adds, --steps sets the number of timed rounds, and two runs with the same arguments dump the same
last timed round (float32 arrays, bitwise equal: seeded dataset, initial weights, on-device z stream and
sampler, deterministic kernels)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 23, 3           # 23 = two 10-round graph launches + one of 3 (bench.round_chunks)
NAMES = {"g_output": (512, 784), "g_params": None, "d_params": None, "g_running": None, "losses": (6,)}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Two plain bench processes with the same arguments (started together), each with its own dump directory."""
    dirs = [str(tmp_path_factory.mktemp(f"dump{i}")) for i in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                               "--warmup", str(WARMUP), "--rows", "4096", "--dump-outputs", d],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for d in dirs]
    out = []
    for p, d in zip(procs, dirs):
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, se[-2000:]
        lines = [l for l in so.splitlines() if l.startswith("{")]
        assert len(lines) == 1, so
        out.append((json.loads(lines[0]), d))
    return out


def test_full_and_dump_options(monkeypatch):
    """--full is off by default and --dump-outputs takes the directory (argument parsing only: no GPU)."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.args_()
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.args_()
    assert a.full is True and a.dump_outputs == "out"
    assert bench.round_chunks(STEPS, 10) == [10, 10, 3] and sum(bench.round_chunks(7, 10)) == 7


@pytest.mark.gpu
def test_plain_line_is_lean(runs):
    line, _ = runs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["losses"]["round"] == STEPS + WARMUP          # exactly the requested rounds ran
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(256 * 1e3 / line["ms_per_step"], rel=1e-3)
    for k in ("roofline", "cpu_baseline", "parity", "conv_round", "ring_round", "lowp_variant"):
        assert k not in line, k                                # the --full legs


@pytest.mark.gpu
def test_dump_outputs_repeat_bitwise(runs):
    (line0, d0), (line1, d1) = runs
    assert sorted(os.listdir(d0)) == sorted(n + ".npy" for n in NAMES) == sorted(os.listdir(d1))
    total = 0
    for n, shape in NAMES.items():
        x, y = np.load(os.path.join(d0, n + ".npy")), np.load(os.path.join(d1, n + ".npy"))
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        if shape is not None:
            assert x.shape == shape, (n, x.shape)
        assert x.shape == y.shape and np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    x = np.load(os.path.join(d0, "losses.npy"))
    assert x[0] == np.float32(line0["losses"]["d_loss"]) and x[3] == np.float32(line0["losses"]["g_loss"])
    assert np.abs(np.load(os.path.join(d0, "g_output.npy"))).max() <= 1.0     # tanh images of the last round
    assert line0["losses"] == line1["losses"]
