"""What the parameter EMA costs: the kernel alone against torch's lerp_, and the headline training loop with and without it.  One JSON line.

    python tools/ema_cost.py [--rays 8192] [--rounds 24] [--calls 8] [--warmup 48] [--launches 50] [--out profiles/ema_cost.json]

Kernel: nerftex_ema_update over ONE tensor of the benchmark field's table size (field.encoder.embeddings.numel()) against
`shadow.lerp_(param, w)` on two tensors of that size -- the same 12 B per parameter, and not code under test.  After a warm-up the two
take turns: each round times --launches back-to-back launches of one between two device events, then of the other, order alternating per
round.  Reported: the median over rounds of us per launch of each, their ratio, and the bytes per second the kernel's median stands for.

Step: two trainers in one process, each the headline's loop (accelerate(renderer, steps_per_call=4, march_across_ring_end=True).step_group
with the next group's rays handed over, as tools/bench_lr_schedule.py times it): `plain`, and `ema` with ema_decay=0.95.  They take turns
in the same way, --calls calls (4 steps each) per block, a host clock around work that ends in a device synchronise.  Reported: the median
ms per step of each, the difference in us, and the launches the step's average takes (the table and the two weight vectors: one).
"""
import argparse
import ctypes
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


def make_loop(dev, grid, rays, ema):
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
    trainer = accelerate(renderer, dt_gamma=1 / 128, steps_per_call=k, march_across_ring_end=True, **({"ema_decay": 0.95} if ema else {}))
    state = {"c": 0}

    def calls(n):
        for _ in range(n):
            c = state["c"]
            trainer.step_group(po[c % 2], pd[c % 2], pt[c % 2], next_rays=(po[(c + 1) % 2], pd[(c + 1) % 2]))
            state["c"] = c + 1

    return trainer, calls


def kernel_cost(dev, n, rounds, launches):
    from nerftex_hip import EmaDesc, check, lib, ptr, stream

    g = torch.Generator().manual_seed(0)
    param = ((torch.rand(n, generator=g) * 2 - 1) * 1e-4).to(dev)
    shadows = {"hip": param.clone().mul_(0.5), "lerp": param.clone().mul_(0.5)}
    num, ticket = torch.full((), 1000, dtype=torch.int32, device=dev), torch.zeros((), dtype=torch.int32, device=dev)
    desc = EmaDesc(0.95, ptr(num), ptr(ticket), None, 1)
    arr = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())  # noqa: E731
    nn = (ctypes.c_uint64 * 1)(n)
    w = 1.0 - 0.95

    def hip():
        check(lib.nerftex_ema_update(ctypes.byref(desc), 1, arr(shadows["hip"]), arr(param), None, nn, stream()))

    def lerp():
        shadows["lerp"].lerp_(param, w)

    run = {"hip": hip, "lerp": lerp}
    for f in run.values():
        for _ in range(launches):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in run}
    for r in range(rounds):
        for name in (("hip", "lerp") if r % 2 == 0 else ("lerp", "hip")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                run[name]()
            b.record()
            b.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / launches)
    med = {name: float(np.median(v)) for name, v in us.items()}
    return {"elements": n, "bytes_per_launch": 12 * n, "launches_per_block": launches, "us_hip": med["hip"], "us_lerp": med["lerp"],
            "hip_over_lerp": med["hip"] / med["lerp"], "hip_TB_per_s": 12 * n / med["hip"] * 1e-6,
            "us_hip_blocks": [round(v, 2) for v in us["hip"]], "us_lerp_blocks": [round(v, 2) for v in us["lerp"]]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--calls", type=int, default=8, help="calls (of 4 steps) per timed block of the step measurement")
    ap.add_argument("--warmup", type=int, default=48, help="untimed steps of each trainer first (priming, capture; at least 24)")
    ap.add_argument("--launches", type=int, default=50, help="launches per timed block of the kernel measurement")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    from ngp_harness import scene

    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda:0")
    grid, _, _ = scene.Scene(bound=2.0, seed=0).bitfield()
    loops = {name: make_loop(dev, grid, args.rays, name == "ema") for name in ("plain", "ema")}
    n_table = loops["plain"][0].field.encoder.embeddings.numel()
    # both first rings (full-size buffers; each ends by releasing the library's scratch) before either trainer captures, then the rest of the warm-up
    for _, calls in loops.values():
        calls(16 // 4)
    for _, calls in loops.values():
        calls(max(args.warmup - 16, 8) // 4)
    torch.cuda.synchronize()
    ms = {name: [] for name in loops}
    for r in range(args.rounds):
        for name in (("plain", "ema") if r % 2 == 0 else ("ema", "plain")):
            calls = loops[name][1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls(args.calls)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / (args.calls * 4))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    ema = loops["ema"][0].ema
    step = {"rays": args.rays, "steps_per_call": 4, "rounds": args.rounds, "steps_per_block": args.calls * 4, "ms_per_step_plain": med["plain"],
            "ms_per_step_ema": med["ema"], "ema_minus_plain_us": (med["ema"] - med["plain"]) * 1e3, "ema_over_plain": med["ema"] / med["plain"],
            "ema_elements": sum(s.numel() for s in ema.shadow_params), "ema_tensors": len(ema.shadow_params), "ema_num_updates": ema.num_updates,
            "ms_plain": [round(v, 4) for v in ms["plain"]], "ms_ema": [round(v, 4) for v in ms["ema"]]}
    loops.clear()
    out = {"device": torch.cuda.get_device_name(0), "kernel": kernel_cost(dev, n_table, args.rounds, args.launches), "step": step}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
