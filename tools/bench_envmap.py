#!/usr/bin/env python3
"""Relighting's two kernels against their op-by-op counterparts on the same GPU:

  fit     one 100 x 200 map through nerftex_envmap_fit (envmap_to_sh on a GPU tensor, the two numbers of `info` read back: one wait)
          against envmap_to_sh(fused=False), the reference's loop of framework ops with loss.item() every step.
  probe   the head under per-probe lighting at 262 144 rows and the reference's 64 probes: nerftex_sh_light_probe_forward against
          sh_light_shade_probes op by op.

Host clock around work that ends in a synchronise; every shape warmed up first; the two sides of a comparison alternate inside one run; the
median and the spread of the repeats are printed.  One JSON line; needs a GPU and fails without one."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "nerf-texture_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def _summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def main():
    import numpy as np
    import torch

    from ngp_harness import light

    ap = argparse.ArgumentParser()
    ap.add_argument("--fit-repeats", type=int, default=5)
    ap.add_argument("--probe-repeats", type=int, default=50)
    ap.add_argument("--rows", type=int, default=262144)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_envmap: no GPU")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(0)
    out = {}

    # ---- the fit: noise plus a bright patch (runs all 5000 steps on both sides)
    envmap = rng.uniform(0.0, 0.6, (100, 200, 3)).astype(np.float32)
    envmap[16:41, 40:73] += 4.0
    m = torch.from_numpy(envmap).to(dev)
    fused, info = light.envmap_to_sh(m)  # (warm-up of the two kernels)
    loop, info_loop = light.envmap_to_sh(m, fused=False, max_steps=50)  # (warm-up of every framework op of the loop)
    t_fused, t_loop = [], []
    for _ in range(args.fit_repeats):
        t_fused.append(_timed(lambda: light.envmap_to_sh(m), sync))
        t_loop.append(_timed(lambda: light.envmap_to_sh(m, fused=False), sync))
    loop, info_loop = light.envmap_to_sh(m, fused=False)
    out["fit_100x200"] = {"entry": _summary(t_fused), "op_by_op": _summary(t_loop), "steps": [info["steps"], info_loop["steps"]],
                          "max_abs_difference": float((fused - loop).abs().max()), "largest_coefficient": float(loop.abs().max())}

    # ---- the probe head
    B, K = args.rows, 64
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)  # noqa: E731
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    brdf = t(rng.normal(0, 2.0, (B, 16)).astype(np.float16))
    n, d, n2 = (t(unit(rng.normal(size=(B, 3))).astype(np.float32)) for _ in range(3))
    H = W = 8
    phi, theta = torch.meshgrid([torch.linspace(np.pi / H, np.pi, H), torch.linspace(-0.5 * np.pi, 1.5 * np.pi, W)], indexing="ij")
    probes = torch.stack([torch.cos(theta) * torch.sin(phi), torch.cos(phi), torch.sin(theta) * torch.sin(phi)], dim=-1).reshape(-1, 3).to(dev)
    tables = rng.normal(0, 0.1, (K, 9, 3)).astype(np.float32)
    tables[:, 0] = rng.uniform(1.0, 3.0, (K, 3))
    tables = t(tables)
    kernel = lambda: light._shade_probes_fused(brdf, n, d, n2, probes, tables, None, light.GAMMA, True)  # noqa: E731
    ops = lambda: light.sh_light_shade_probes(brdf, n, d, n2, probes, tables, True, light.GAMMA, None)  # noqa: E731
    with torch.no_grad():
        for _ in range(3):
            a, b = kernel(), ops()
        t_kernel, t_ops = [], []
        for _ in range(args.probe_repeats):
            t_kernel.append(_timed(kernel, sync))
            t_ops.append(_timed(ops, sync))
    # the reference's grid has coinciding directions (its last row, its first and last columns): rows whose best two dot products lie within
    # 1e-6 in float64 are undecided, the kernel (lowest index) and the framework's argmax over its own rounding may light them differently
    top = (n2.double() @ probes.double().T).topk(2, dim=-1).values
    decided = (top[:, 0] - top[:, 1]) > 1e-6
    # bytes the kernel has to move per row: 8 (the four used BRDF halves) + 3 x 12 (normal, direction, secondary normal) in, 4 x 12 out
    moved = B * (8 + 36 + 48)
    out["probe_head"] = {"rows": B, "K": K, "kernel": _summary(t_kernel), "op_by_op": _summary(t_ops), "bytes_moved": moved,
                         "kernel_GBps_end_to_end": round(moved / (statistics.median(t_kernel) * 1e-3) / 1e9, 1),
                         "max_abs_difference_color_decided_rows": float(((a[0] - b[0].float()).abs().amax(-1) * decided).max()),
                         "rows_lit_by_different_probes": int(((a[0] - b[0].float()).abs().amax(-1) > 1e-4).sum()), "undecided_rows": int((~decided).sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
