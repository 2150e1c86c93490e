"""bench.py's plain run against its --full run: a plain run measures the headline and nothing else, and computes what the --full run's headline
loop computes (the baked-pool loop that --full times first leaves no trace in the fresh-ray loop's training)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("occupancy_update", "value_including_occupancy_update", "roofline", "cpu_baseline", "rendered", "other_config")


def test_full_is_opt_in_and_reaches_the_profiler_children(monkeypatch):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "16", "--warmup", "4"])
    args = bench.parse()
    assert args.full is False
    # the rocprofv3 children time the baked-pool loop of a --full run
    assert "--full" in bench._replay_child_cmd(args, "ffmlp", 8192, "fp16", 416)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full is True


def _bench(extra, dump):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "16", "--warmup", "4", "--rays", "2048", "--dump-outputs", str(dump)] + extra
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])
    return res, {f[:-len(".npy")]: np.load(os.path.join(dump, f)) for f in os.listdir(dump)}


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone_and_trains_like_the_full_run(tmp_path):
    plain, plain_out = _bench([], tmp_path / "plain")
    assert plain["full"] is False and plain["metric"] == "ray-samples/s (train)" and plain["unit"] == "ray-samples/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f16" and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["config"]["headline_loop"] == "fresh rays through ngp_harness.accelerate"
    assert all(plain[k] is None for k in MOVED), {k: plain[k] is None for k in MOVED}
    # --full with the long side measurements switched off: the baked-pool loop, its kernel tables and the occupancy timing, then the headline loop
    full, full_out = _bench(["--full", "--no-other", "--no-cpu-baseline", "--no-infer", "--no-replay-profile"], tmp_path / "full")
    assert full["full"] is True and full["occupancy_update"] is not None and full["roofline"] is not None
    assert full["other_config"][0]["workload"].startswith("the same step with a pool of 8 ray batches BAKED")
    assert full["config"]["headline_loop"] == plain["config"]["headline_loop"]
    assert sorted(plain_out) == sorted(full_out) and {"loss", "step_samples"} <= set(plain_out)
    for name, a in plain_out.items():
        assert np.array_equal(a, full_out[name]), name
