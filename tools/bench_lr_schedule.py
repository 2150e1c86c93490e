"""The headline training loop with and without the reference's learning-rate schedule on the device: one JSON line.

    python tools/bench_lr_schedule.py [--rays 8192] [--rounds 24] [--calls 8] [--warmup 48]

Two trainers in one process, each the headline's loop (accelerate(renderer, steps_per_call=4, march_across_ring_end=True).step_group with
the next group's rays handed over, bench.py measure_accelerated): `plain` without a schedule, `sched` with
lr_scheduler=lambda opt: LambdaLR(opt, lambda it: 0.1 ** min(it / 40000, 1)) (main_nerf.py:131-133).  After an untimed warm-up of both,
they take turns: each round times --calls calls (4 steps each) of one, then of the other, order alternating per round.  Reported: the
median over rounds of ms per step of each, and their ratio.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "nerf-texture_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_loop(dev, grid, rays, schedule, total_steps):
    from torch.optim.lr_scheduler import LambdaLR

    from ngp_harness import scene
    from ngp_harness.accelerate import accelerate
    from ngp_harness.model import NGPField, Renderer

    torch.manual_seed(0)
    field = NGPField(bound=2.0, mlp="ffmlp", fused_glue=True).to(dev)
    torch.manual_seed(1)
    field.encoder.embeddings.data.uniform_(-1e-4, 1e-4)
    renderer = Renderer(field, bound=2.0, min_near=0.2, density_thresh=10.0).to(dev)
    renderer.set_occupancy(torch.from_numpy(grid).to(dev))
    k, n_pool = 4, 8
    pool = [scene.train_batch(rays, seed=100 + i, n_views=4) for i in range(n_pool)]
    po = [torch.stack([torch.from_numpy(pool[c * k + i][0]) for i in range(k)]).to(dev).contiguous() for c in range(n_pool // k)]
    pd = [torch.stack([torch.from_numpy(pool[c * k + i][1]) for i in range(k)]).to(dev).contiguous() for c in range(n_pool // k)]
    gt = torch.rand(n_pool, rays, 3, generator=torch.Generator().manual_seed(4321)).to(dev)
    pt = [gt[c * k:(c + 1) * k].contiguous() for c in range(n_pool // k)]
    field.train()
    kw = dict(lr_scheduler=lambda opt: LambdaLR(opt, lambda it: 0.1 ** min(it / 40000, 1)), total_steps=total_steps) if schedule else {}
    trainer = accelerate(renderer, dt_gamma=1 / 128, steps_per_call=k, march_across_ring_end=True, **kw)
    state = {"c": 0}

    def calls(n):
        for _ in range(n):
            c = state["c"]
            trainer.step_group(po[c % 2], pd[c % 2], pt[c % 2], next_rays=(po[(c + 1) % 2], pd[(c + 1) % 2]))
            state["c"] = c + 1

    return trainer, calls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--calls", type=int, default=8, help="calls (of 4 steps) per timed block")
    ap.add_argument("--warmup", type=int, default=48, help="untimed steps of each trainer first (priming, capture; at least 24)")
    args = ap.parse_args()
    from ngp_harness import scene

    dev = torch.device("cuda:0")
    grid, _, _ = scene.Scene(bound=2.0, seed=0).bitfield()
    total = max(args.warmup, 24) + args.rounds * args.calls * 4 + 64
    loops = {name: make_loop(dev, grid, args.rays, name == "sched", total) for name in ("plain", "sched")}
    # each trainer's first ring (full-size buffers) ends by releasing the library's scratch (AcceleratedTrainer._resize), which the other's
    # captured graphs would still point into: both first rings run before either trainer captures, then the rest of the warm-up
    for _, calls in loops.values():
        calls(16 // 4)
    for _, calls in loops.values():
        calls(max(args.warmup - 16, 8) // 4)
    torch.cuda.synchronize()
    ms = {name: [] for name in loops}
    for r in range(args.rounds):
        order = ("plain", "sched") if r % 2 == 0 else ("sched", "plain")
        for name in order:
            calls = loops[name][1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls(args.calls)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / (args.calls * 4))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    sched = loops["sched"][0].lr_scheduler
    print(json.dumps({"rays": args.rays, "steps_per_call": 4, "rounds": args.rounds, "steps_per_block": args.calls * 4,
                      "ms_per_step_plain": med["plain"], "ms_per_step_sched": med["sched"], "sched_over_plain": med["sched"] / med["plain"],
                      "sched_last_epoch": sched.last_epoch, "sched_last_lr": sched.get_last_lr()[0],
                      "ms_plain": [round(v, 4) for v in ms["plain"]], "ms_sched": [round(v, 4) for v in ms["sched"]]}))


if __name__ == "__main__":
    main()
