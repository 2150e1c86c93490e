"""The curved field's training step, eager against accelerate(): one JSON line.

    python tools/bench_curved_train.py [--rays 8192] [--steps 64] [--warmup 24]
    python tools/bench_curved_train.py --reg-loop 200     # only the regulariser, both forms, back to back (for rocprofv3 --kernel-trace --stats)

The field is CurvedField over curved.star_flower_mesh() at trained scale (table U(-0.5, 0.5), as tests/test_gpu_round3.py), after one
occupancy update.  eager_ms: the reference's loop (nerf/utils.py:637-666) -- render_train + MSE + regular_loss() (the host's level pick and
~30 framework ops) + GradScaler + torch's fused Adam, one launch at a time.  accelerated_ms: accelerate(renderer, steps_per_call=4) with the
next group's rays handed over (next_rays).  reg_us_eager / reg_us_kernel: one regulariser forward + backward, 1e-8 * clustering_loss() against
the step form of nerftex_grid_cluster_loss, device time between events over --reg-iters calls each.
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


def make(dev, seed=0):
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer

    v, f = star_flower_mesh()
    torch.manual_seed(seed)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
        for layer in field.encoder.cluster_layers:
            layer.cluster_centers.uniform_(-0.5, 0.5)
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        r.update_extra_state_device()
    field.train()
    return field, r


def batches(dev, n, k, seed=1000):
    from ngp_harness import scene

    out = [scene.train_batch(n, seed=seed + i, radius=1.6) for i in range(k)]
    o = torch.stack([torch.from_numpy(a) for a, _ in out]).to(dev)
    d = torch.stack([torch.from_numpy(b) for _, b in out]).to(dev)
    t = torch.rand(k, n, 3, generator=torch.Generator().manual_seed(seed)).to(dev) * 0.2 + 0.4
    return o, d, t


def eager_ms(dev, n, steps, warmup):
    field, r = make(dev)
    o, d, t = batches(dev, n, 8)
    opt = torch.optim.Adam(field.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, fused=True)
    scaler = torch.amp.GradScaler("cuda")
    np.random.seed(0)

    def one(i):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            image, _, _ = r.render_train(o[i % 8], d[i % 8], dt_gamma=1 / 128, bg_color=1, perturb=True, max_steps=1024)
            loss = ((image.float() - t[i % 8]) ** 2).mean()
        loss = loss + field.regular_loss()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        if r.local_step == 16:
            r.update_mean_count()

    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        one(warmup + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def accelerated_ms(dev, n, steps, warmup, k=4):
    from ngp_harness.accelerate import accelerate

    field, r = make(dev)
    o, d, t = batches(dev, n, 8 * k)
    o, d, t = o.view(8, k, n, 3), d.view(8, k, n, 3), t.view(8, k, n, 3)
    tr = accelerate(r, steps_per_call=k)
    np.random.seed(0)
    calls, wcalls = max(1, steps // k), max(1, warmup // k)
    for i in range(wcalls):
        tr.step_group(o[i % 8], d[i % 8], t[i % 8])
    torch.cuda.synchronize()
    assert tr._graphs is not None, "warm-up too short for the capture"
    i0 = wcalls
    t0 = time.perf_counter()
    for i in range(i0, i0 + calls):
        tr.step_group(o[i % 8], d[i % 8], t[i % 8], next_rays=(o[(i + 1) % 8], d[(i + 1) % 8]))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / (calls * k)
    return ms, float(tr.loss), float(tr.reg_loss)


def reg_forms(dev):
    """The two forms of one regulariser evaluation + gradient on the curved table (level 3)."""
    from gridencoder.grid_clustering import grid_cluster_step

    field, _ = make(dev)
    enc = field.encoder
    layers = list(enc.cluster_layers)
    level = torch.tensor(3, dtype=torch.int32, device=dev)
    gt = torch.zeros_like(enc.embeddings)
    gc = torch.zeros(len(layers), 4, 2, device=dev)
    loss = torch.zeros((), device=dev)

    def eager():
        enc.embeddings.grad = None
        (1e-8 * enc.clustering_loss()).backward()

    def kernel():
        grid_cluster_step(enc.embeddings.detach(), enc.offsets, torch.stack([layer.cluster_centers.detach() for layer in layers]), level, 1.0, 1e-8,
                          loss=loss, grad_table=gt, grad_centres=gc)

    return eager, kernel


def time_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--reg-iters", type=int, default=100)
    ap.add_argument("--reg-loop", type=int, default=0, help="only run both regulariser forms this many times each (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    eager, kernel = reg_forms(dev)
    if a.reg_loop:
        for fn in (eager, kernel):
            for _ in range(a.reg_loop):
                fn()
            torch.cuda.synchronize()
        print(json.dumps({"reg_loop": a.reg_loop}))
        return
    out = {"workload": "curved_field_train", "mesh": "star_flower", "rays": a.rays, "steps": a.steps, "warmup": a.warmup}
    out["reg_us_eager"] = round(time_us(eager, a.reg_iters), 1)
    out["reg_us_kernel"] = round(time_us(kernel, a.reg_iters), 1)
    del eager, kernel
    out["eager_ms"] = round(eager_ms(dev, a.rays, a.steps, a.warmup), 4)
    ms, loss, reg = accelerated_ms(dev, a.rays, a.steps, a.warmup)
    out.update(accelerated_ms=round(ms, 4), steps_per_call=4, loss=loss, reg_loss=reg)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
