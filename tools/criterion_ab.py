"""What the criterion and the error map cost on accelerate(steps_per_call=4).step_group (bench.py's scene, 8192 rays, fp16): ms per step of
  default   accelerate(...) as it always was (the MSE entries),
  l1        criterion="l1",
  l1_map    criterion="l1" with a [8, 16384] error map and the cells of every ray,
each in a process of its own, `--calls` timed calls after warm-up, `--reps` times, interleaved.  `--parent TREE`: a checkout of the parent
commit, built, whose default is timed beside them ("parent").
    python tools/criterion_ab.py [--parent ../parent] > profiles/criterion_ab.json"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(tree, config, rays, calls):
    sys.path[:0] = [tree, os.path.join(tree, "nerf-texture_amd")]
    import torch

    from ngp_harness import scene
    from ngp_harness.accelerate import accelerate
    from ngp_harness.model import NGPField, Renderer

    dev, k = torch.device("cuda:0"), 4
    sc = scene.Scene(bound=2.0, seed=0)
    grid, _, _ = sc.bitfield()
    torch.manual_seed(0)
    field = NGPField(bound=2.0, mlp="ffmlp", fused_glue=True).to(dev)
    torch.manual_seed(1)
    field.encoder.embeddings.data.uniform_(-1e-4, 1e-4)
    r = Renderer(field, bound=2.0, min_near=0.2, density_thresh=10.0).to(dev)
    r.set_occupancy(torch.from_numpy(grid).to(dev))
    field.train()
    pool = [scene.train_batch(rays, seed=100 + i, n_views=4) for i in range(8)]
    po = [torch.stack([torch.from_numpy(pool[c * k + i][0]) for i in range(k)]).to(dev).contiguous() for c in range(2)]
    pd = [torch.stack([torch.from_numpy(pool[c * k + i][1]) for i in range(k)]).to(dev).contiguous() for c in range(2)]
    gt = torch.rand(2, k, rays, 3, generator=torch.Generator().manual_seed(4321)).to(dev)
    kw, more = {}, [{}, {}]
    if config in ("l1", "l1_map"):
        kw["criterion"] = "l1"
    if config == "l1_map":
        kw["error_map"] = torch.zeros(8, 16384, device=dev)
        g = torch.Generator().manual_seed(7)
        more = [{"error_inds": torch.stack([torch.randperm(8 * 16384, generator=g)[:rays] for _ in range(k)]).to(dev)} for _ in range(2)]
    tr = accelerate(r, dt_gamma=1 / 128, steps_per_call=k, march_across_ring_end=True, **kw)

    def call(c):
        tr.step_group(po[c % 2], pd[c % 2], gt[c % 2], next_rays=(po[(c + 1) % 2], pd[(c + 1) % 2]), **more[c % 2])

    for c in range(12):  # three rings: priming, warm-up, capture, replayed calls
        call(c)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for c in range(12, 12 + calls):
        call(c)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / (calls * k)
    print(json.dumps({"config": config, "ms_per_step": round(ms, 5), "loss": float(tr.loss), "graphed": tr._groups is not None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.rays, a.calls)
    forms = ([("parent", os.path.abspath(a.parent), "default")] if a.parent else []) + [(c, ROOT, c) for c in ("default", "l1", "l1_map")]
    runs = {name: [] for name, _, _ in forms}
    for _ in range(a.reps):
        for name, tree, config in forms:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, config, "--rays", str(a.rays), "--calls", str(a.calls)],
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-2000:])
                sys.exit(f"{name}: exit status {p.returncode}")  # (nothing more is started on the GPU)
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps({"what": f"accelerate(steps_per_call=4).step_group, {a.rays} rays, fp16, {a.calls} timed calls of 4 steps after 12 calls of warm-up, "
                              f"{a.reps} interleaved runs each, one process per run", "ms_per_step": {k: [x["ms_per_step"] for x in v] for k, v in runs.items()},
                      "runs": runs}))


if __name__ == "__main__":
    main()
