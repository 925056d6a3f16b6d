"""The N=1 line of bench.py, run in-process at the tiny config: a plain run carries the headline figure and the roofline
measured inside its timed steps and none of the legs that take runs of their own; --full adds them (the tiny config has
only the CPU baseline: fp8, gemma2_block and decode are 4B legs); --dump-outputs writes the last timed step's outputs
as float32 .npy, from inputs that depend only on the arguments."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULL_ONLY = ("fp8", "gemma2_block", "cpu_baseline", "decode")
STEPS, WARMUP, B = 3, 1, 2


def run_bench(monkeypatch, capsys, *extra):
    import torch
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--config", "tiny", "--batch", str(B),
                                      "--steps", str(STEPS), "--warmup", str(WARMUP), *extra])
    threads = torch.get_num_threads()
    capsys.readouterr()
    try:
        bench.main()
    finally:
        torch.set_num_threads(threads)  # the CPU baseline takes every usable core
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(cuda, monkeypatch, capsys, tmp_path):
    dumps = []
    for i in range(2):
        d = tmp_path / f"dump{i}"
        r = run_bench(monkeypatch, capsys, "--dump-outputs", str(d))
        assert not [k for k in FULL_ONLY if k in r]
        assert r["steps"] == STEPS and r["warmup"] == WARMUP and r["n_gpus"] == 1
        assert r["unit"] == "episodes/s" and r["higher_is_better"] is True and r["dtype"] == "bf16"
        assert r["ms_per_step"] > 0
        assert r["value"] == pytest.approx(B / (r["ms_per_step"] * 1e-3), rel=2e-2)
        # one gate/up GeGLU launch per Gemma2 layer per timed step, counted inside the timed steps only
        assert r["roofline"]["launches_timed"] > 0 and r["roofline"]["launches_timed"] % STEPS == 0
        out = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert set(out) == {"loss", "grad_norm", "params_sample", "grads_sample"}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
        assert sum(a.nbytes for a in out.values()) <= 64 << 20
        assert out["loss"].shape == (1,) and float(out["loss"][0]) == pytest.approx(r["final_loss"], abs=1e-4)
        assert out["grad_norm"][0] > 0 and np.count_nonzero(out["grads_sample"]) > 0
        assert out["params_sample"].shape == out["grads_sample"].shape
        dumps.append(out)
    # same arguments, same inputs: the runs may differ by the order of atomic fp32 sums ahead of a bf16 rounding,
    # a few bf16 ulps (2^-8) on a few elements; other inputs would differ by the gradients' own norm (relative 1)
    for k in dumps[0]:
        a, b = dumps[0][k].astype(np.float64), dumps[1][k].astype(np.float64)
        assert np.linalg.norm(a - b) <= 1e-2 * np.linalg.norm(a), k


def test_full_adds_the_other_legs(cuda, monkeypatch, capsys):
    r = run_bench(monkeypatch, capsys, "--full", "--cpu-iters", "1")
    assert r["cpu_baseline"]["value"] > 0 and r["cpu_baseline"]["unit"] == "episodes/s"
    assert r["ms_per_step"] > 0 and r["roofline"]["launches_timed"] > 0
    r = run_bench(monkeypatch, capsys, "--full", "--no-cpu-baseline")
    assert "cpu_baseline" not in r
