"""bench.py's plain run and its options: --dump-outputs writes the last timed step's disparities (float32, a
fixed seeded sample past the size budget), and only --full adds the side measurements to the result line."""
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


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    g = torch.Generator().manual_seed(3)
    outs = [torch.randn(2, 30, 50, generator=g), torch.randn(2, 15, 25, generator=g, dtype=torch.float64)]
    bench.dump_outputs(str(tmp_path / "whole"), outs)
    for i, o in enumerate(outs):
        a = np.load(tmp_path / "whole" / f"disp_{i}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(o.shape)
        assert np.array_equal(a, o.to(torch.float32).numpy())
    # past the budget: the same share of every output, the same elements on every call, within the budget
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 1000)
    bench.dump_outputs(str(tmp_path / "s1"), outs)
    bench.dump_outputs(str(tmp_path / "s2"), [o.clone() for o in outs])
    total = 0
    for i, o in enumerate(outs):
        a, b = np.load(tmp_path / "s1" / f"disp_{i}.npy"), np.load(tmp_path / "s2" / f"disp_{i}.npy")
        assert a.dtype == np.float32 and a.ndim == 1 and np.array_equal(a, b)
        assert a.size == o.numel() * 1000 // (3000 + 750)
        flat = o.to(torch.float32).reshape(-1).numpy()
        # the documented selection: seed 0, k of the flattened elements without replacement, ascending indices
        assert np.array_equal(a, flat[np.sort(np.random.default_rng(0).choice(flat.size, size=a.size, replace=False))])
        total += a.nbytes
    assert total <= 4 * 1000


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")
def test_plain_run_dumps_outputs_and_skips_side_measurements(tmp_path):
    def run(tag, steps):
        r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                            "--warmup", "1", "--dump-outputs", str(tmp_path / tag)], cwd=ROOT, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        return json.loads(r.stdout.strip().splitlines()[-1]), np.load(tmp_path / tag / "disp_0.npy")

    line, a = run("a", 3)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] * line["ms_per_step"] - 1e3) < 1.0  # batch 1: pairs/s x ms per step = 1000
    for k in ("cpu_baseline", "roofline"):  # measured with --full only
        assert line.get(k) is None, k
    for k in ("epe_vs_reference", "forward_e2e", "concurrent", "roofline_cost_volume", "top_ops_in_graph"):
        assert k not in line, k
    assert a.dtype == np.float32 and a.shape == (1, 384, 1248) and np.isfinite(a).all() and a.std() > 0
    _, b = run("b", 2)  # the same arguments but the step count: the same inputs, the same disparities
    assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")
def test_full_run_keeps_the_moved_measurements():
    """--full: everything a plain run leaves out is still measured (short: 5 steps, the CPU baseline's minimum
    of three forwards)."""
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup",
                        "1", "--full", "--cpu-seconds", "0"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 5 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["roofline"]["kernel"] and line["roofline"]["avg_us"] > 0
    assert line["roofline_mfma"]["kernel"] == "group_stem"
    assert len(line["top_ops_in_graph"]) == 8 and line["sum_of_marginals_us"] > 0
    assert line["cpu_baseline"]["value"] > 0
    assert line["epe_vs_oracle"] <= 1e-3  # smoke()'s parity bound, on the benchmark input
    assert line["epe_vs_reference"]["epe_px"] <= 1e-3
    assert line["concurrent"]["outputs_identical"] is True and line["forward_e2e"]["value"] > 0
    for k in ("roofline_cost_volume", "roofline_cost_volume_configs2", "roofline_concat_volume_configs2"):
        assert line[k]["achieved"] > 0, k
