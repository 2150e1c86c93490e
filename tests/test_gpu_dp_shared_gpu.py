"""The multi-process training step of bench.py (two replayed graphs per step, eager all-reduce of the fp16 gradients in between,
mean_count agreement) run end to end with TWO ranks on the ONE GPU of the test box: NERFTEX_DP_SHARE_GPU=1 puts both ranks on cuda:0
and exchanges through gloo (RCCL refuses two ranks on one device).  What it pins: the ranks finish with bit-identical replicas."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("extra", [[], ["--no-fused-opt"], ["--graph-allreduce"]], ids=["half-leaf-adam", "torch-adam", "allreduce-in-graph-or-fallback"])
def test_two_ranks_on_one_gpu_keep_identical_replicas(extra):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = dict(os.environ, NERFTEX_DP_SHARE_GPU="1")
    port = 29600 + os.getpid() % 200 + (0 if not extra else 7 if extra[0] == "--no-fused-opt" else 13)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "20", "--warmup", "4", "--rays", "2048", "--no-cpu-baseline",
           "--no-other", "--no-infer", "--no-kernel-timing", "--warm-seconds", "0"] + extra
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    res = json.loads(line)
    assert res["n_gpus"] == 2 and res["config"]["parallelism"] == "dp2"
    assert res["config"]["replicas_identical_after_run"] is True
    assert res["value"] > 0
    # --graph-allreduce: only RCCL collectives can be captured; under gloo (this test) the bench must fall back to the split structure and
    # say so (the branch itself runs on the driver's 8-GPU node)
    assert res["config"]["collective"]["allreduce_in_graph"] is False


def _bench(n_ranks, rays, extra, port):
    env = dict(os.environ, NERFTEX_DP_SHARE_GPU="1")
    common = ["--full", "--steps", "12", "--warmup", "4", "--rays", str(rays), "--no-cpu-baseline", "--no-other", "--no-infer", "--no-kernel-timing", "--no-perturb", "--warm-seconds", "0"] + extra
    if n_ranks == 1:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--graph-split"] + common
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_ranks), "--master-addr", "127.0.0.1", "--master-port",
               str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(n_ranks)] + common
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.parametrize("wire", ["fp32", "fp16"])
def test_two_ranks_train_like_one_rank_on_the_global_batch(wire):
    """2 ranks x 2048 rays == 1 rank x 4096 rays (the same global batch, sharded; no start jitter, which is seeded by the local ray index):
    the parameters after the run agree.  With the fp32 wire (SURVEY 8(e)'s parity form) the only difference is that each rank rounds its
    partial table gradient to fp16 before the sum."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    two = _bench(2, 2048, ["--wire", wire], 29650 + os.getpid() % 100 + (3 if wire == "fp16" else 0))
    one = _bench(1, 4096, [], 0)
    c = two["config"]["collective"]
    assert c["world_size"] == 2 and c["wire_dtype"] == ("float32" if wire == "fp32" else "float16") and c["allreduce_us_per_step"] > 0
    assert two["config"]["replicas_identical_after_run"] is True
    # Not bit-equal by construction: each rank rounds its partial table gradient to fp16, sizes its own sample buffer (the drop rule for
    # rays past the buffer's end sees different ends), and Adam turns any small gradient difference into a step of size lr.  The L1 norm of
    # all parameters after ~70 steps agrees to about a percent; without the all-reduce it does not come close.
    a, b = two["config"]["param_l1_after_run"], one["config"]["param_l1_after_run"]
    assert abs(a - b) <= 1.5e-2 * abs(b), (a, b)
    assert abs(two["config"]["samples_per_step_per_gpu"] * 2 - one["config"]["samples_per_step_per_gpu"]) <= 0.02 * one["config"]["samples_per_step_per_gpu"]


def test_march_one_step_ahead_trains_bit_identically():
    """bench.py's default single-GPU step (march of step k + 1 replayed on a second, high-priority stream under shade + backward +
    optimizer of step k) against the one-graph step (`--no-march-ahead`): the march needs the rays and the occupancy grid, not the
    weights, so the parameters after the run are the same bits."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = []
    for extra in ([], ["--no-march-ahead"]):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--steps", "40", "--warmup", "4", "--rays", "2048", "--no-cpu-baseline", "--no-other",
               "--no-infer", "--no-kernel-timing", "--warm-seconds", "0"] + extra
        run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        out.append(json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1]))
    ahead, single = out
    assert "second stream" in ahead["config"]["launch"] and "one replayed HIP graph" in single["config"]["launch"]
    assert ahead["config"]["param_l1_after_run"] == single["config"]["param_l1_after_run"]
    assert ahead["config"]["samples_per_step_per_gpu"] == single["config"]["samples_per_step_per_gpu"]


def _probe(script, args, timeout=600):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", script)] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert lines, out.stderr[-2000:]
    return out.returncode, json.loads(lines[-1])


def test_every_stage_of_the_step_is_bit_reproducible_beside_another_process():
    """Round 4: with packed-fp32 instructions in its record builder the hash-grid backward returned a slightly wrong table gradient in ~12% of the
    steps whenever a second process kept the same GPU busy (16 consecutive lanes of one wave built their records with a corner weight of 0) --
    the source of the run-to-run differences of the two-rank rig above.  csrc/Makefile now compiles that file without them; this repeats one
    training step 150 times on fixed rays beside a second process that trains on the same GPU and compares exact checksums of every stage."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    rc, res = _probe("step_concurrency_probe.py", ["--neighbour", "process", "--iters", "150"])
    assert res["beside_the_neighbour"] >= 100, res
    assert rc == 0 and not any(res["iterations_differing_by_stage"].values()), res


def test_framework_kernels_around_the_library_are_bit_reproducible_beside_another_process():
    """Round 6: the fault of DESIGN 7.1 needs packed-fp32 chains beside fp16 MFMAs, and this library can only keep ITS OWN code
    free of them.  BASELINE configs[1]'s step -- rocBLAS / hipBLASLt GEMMs for the nn.Linear MLPs and the framework's elementwise kernels between this
    library's kernels -- torch's fused Adam on the step's gradients, and bench.py's on-device ray generation (randint, einsum, norms), 150 times beside
    a process that trains with MFMA kernels on the same GPU: exact checksums of every stage against the quiet-GPU iteration."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    rc, res = _probe("step_concurrency_probe.py", ["--neighbour", "process", "--iters", "150", "--mlp", "torch", "--stages", "train,adam,draw"])
    assert res["beside_the_neighbour"] >= 100, res
    assert rc == 0 and not any(res["iterations_differing_by_stage"].values()), res


@pytest.mark.parametrize("neighbour", ["stream", "process"])
def test_table_gradient_is_bit_reproducible_beside_other_work(neighbour):
    """The same fixed hash-grid backward, 1000 launches, while an MLP runs on a second stream of the process / while another process trains:
    every launch returns the bits of the quiet-GPU launch (the old build: 22 of 2000 wrong beside a stream, 300-550 of 2000 beside a process)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    rc, res = _probe("g2_concurrency_probe.py", ["--neighbour", neighbour, "--launches", "1000"])
    assert res["launches_beside_the_neighbour"] >= 500, res
    assert rc == 0 and res["wrong_launches"] == 0, res
