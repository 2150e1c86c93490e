"""What per-ray random backgrounds and RGBA pixels cost on the accelerated step: the headline loop with and without them, and the draw alone.
One JSON line.

    python tools/pixels_cost.py [--rays 8192] [--rounds 24] [--calls 8] [--warmup 48] [--launches 50] [--out profiles/pixels_cost.json]

Step: two trainers in one process, each the headline's loop (accelerate(renderer, steps_per_call=4, march_across_ring_end=True).step_group with
the next group's rays handed over, as tools/ema_cost.py times it): `plain` on [4,N,3] targets, and `pixels` with bg_color="random",
target_channels=4 on [4,N,4] targets.  After a warm-up (priming, capture) they take turns, order alternating per round; each block is --calls
replayed calls (4 steps each) between two device events.  Reported: the median ms per step of each and the difference in us.

Draw: torch.rand of [4,N,3] into a static buffer (what a "random" call enqueues in front of its replay), --launches back-to-back draws between two
device events per round: us per draw, and its share of a `pixels` call.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "nerf-texture_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def make_loop(dev, grid, rays, pixels):
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
    gt = torch.rand(n_pool, rays, 4 if pixels else 3, generator=torch.Generator().manual_seed(4321)).to(dev)
    pt = [gt[c * k:(c + 1) * k].contiguous() for c in range(n_pool // k)]
    field.train()
    more = dict(bg_color="random", target_channels=4, bg_generator=torch.Generator(device=dev).manual_seed(7)) if pixels else {}
    trainer = accelerate(renderer, dt_gamma=1 / 128, steps_per_call=k, march_across_ring_end=True, **more)
    state = {"c": 0}

    def calls(n):
        for _ in range(n):
            c = state["c"]
            trainer.step_group(po[c % 2], pd[c % 2], pt[c % 2], next_rays=(po[(c + 1) % 2], pd[(c + 1) % 2]))
            state["c"] = c + 1

    return trainer, calls


def draw_cost(dev, rays, rounds, launches):
    dst = torch.empty(4, rays, 3, device=dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    for _ in range(launches):
        torch.rand(dst.shape, generator=gen, out=dst)
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            torch.rand(dst.shape, generator=gen, out=dst)
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / launches)
    return {"shape": list(dst.shape), "launches_per_block": launches, "us_per_draw": float(np.median(us)), "us_blocks": [round(v, 2) for v in us]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--calls", type=int, default=8, help="calls (of 4 steps) per timed block")
    ap.add_argument("--warmup", type=int, default=48, help="untimed steps of each trainer first (priming, capture; at least 24)")
    ap.add_argument("--launches", type=int, default=50, help="draws per timed block of the draw measurement")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    from ngp_harness import scene

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    grid, _, _ = scene.Scene(bound=2.0, seed=0).bitfield()
    loops = {name: make_loop(dev, grid, args.rays, name == "pixels") for name in ("plain", "pixels")}
    # both first rings (full-size buffers; each ends by releasing the library's scratch) before either trainer captures, then the rest of the warm-up
    for _, calls in loops.values():
        calls(16 // 4)
    for _, calls in loops.values():
        calls(max(args.warmup - 16, 8) // 4)
    torch.cuda.synchronize()
    assert all(t._graphs is not None for t, _ in loops.values()), "the timed calls are replayed graphs"
    ms = {name: [] for name in loops}
    for r in range(args.rounds):
        for name in (("plain", "pixels") if r % 2 == 0 else ("pixels", "plain")):
            calls = loops[name][1]
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            calls(args.calls)
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / (args.calls * 4))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    step = {"rays": args.rays, "steps_per_call": 4, "rounds": args.rounds, "steps_per_block": args.calls * 4, "ms_per_step_plain": med["plain"],
            "ms_per_step_pixels": med["pixels"], "pixels_minus_plain_us": (med["pixels"] - med["plain"]) * 1e3, "pixels_over_plain": med["pixels"] / med["plain"],
            "ms_plain": [round(v, 4) for v in ms["plain"]], "ms_pixels": [round(v, 4) for v in ms["pixels"]]}
    loops.clear()
    draw = draw_cost(dev, args.rays, args.rounds, args.launches)
    draw["share_of_a_pixels_call"] = draw["us_per_draw"] / (med["pixels"] * 4e3)
    out = {"device": torch.cuda.get_device_name(0), "step": step, "draw": draw}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
