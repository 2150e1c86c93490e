#!/usr/bin/env python3
"""Phase budget of the training march's count pass (march_count_parallel_kernel, csrc/raymarching.hip), on the GPU.

The kernel's ablation exits (`march_count_probe` knob: every segment stops after phase 1, 2 or 3; the rays still run all their segments) are
timed one after the other on the benchmark's rays and occupancy grid: 8192 rays, eager launches, the library's own hipEvent pair around the
launch.  A row is the time of the kernel up to and including that phase; the difference of two rows is what a phase costs.  Both builds of the
kernel (default and `march_lean`) are listed.  With a probe set the samples are garbage; probe 0 is the kernel as it ships.

    python tools/march_count_budget.py [--rays 8192] [--reps 200] >> profiles/march_count_budget.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "nerf-texture_amd"))

import torch  # noqa: E402

PHASES = [(1, "1 sequence members"), (2, "2 + classification"), (3, "3 + walk"), (0, "4 + sample log (the whole kernel)")]
KERNEL = "march_count_parallel_kernel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--label", default="", help="a word for the heading (which revision of the kernel this is)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")

    import nerftex_hip
    import raymarching
    from ngp_harness import scene

    sc = scene.Scene(bound=2.0, seed=0)
    bits = torch.from_numpy(sc.bitfield()[2]).to(dev)
    o, d = scene.train_batch(a.rays, seed=100, n_views=4)
    ro, rd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    aabb = torch.tensor([-2, -2, -2, 2, 2, 2.0], device=dev)
    nears, fars = raymarching.near_far_from_aabb(ro, rd, aabb, 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    raymarching.march_rays_train(ro, rd, 2.0, bits, sc.cascade, 128, nears, fars, counter, -1, True, 128, False, 1 / 128, 1024)
    total = int(counter[0].item())
    M = total + 128 - total % 128

    def timed(probe, lean):
        with nerftex_hip.tune(march_count_probe=probe, march_lean=lean):
            for rep in range(a.reps + 10):
                if rep == 10:  # warm
                    torch.cuda.synchronize()
                    nerftex_hip.kernel_profile(1, reset=True)
                counter.zero_()
                raymarching.march_rays_train(ro, rd, 2.0, bits, sc.cascade, 128, nears, fars, counter, M, True, -1, False, 1 / 128, 1024)
            torch.cuda.synchronize()
            nerftex_hip.kernel_profile(0)
            rec = nerftex_hip.kernel_profile()[KERNEL]
            nerftex_hip.kernel_profile(reset=True)
        assert rec["calls"] == a.reps, rec
        return rec["avg_us"]

    print(f"== {KERNEL} {a.label}: {a.rays} rays, {total} samples, {a.reps} eager launches per row, {torch.cuda.get_device_name(0)}")
    print(f"{'runs through phase':38s} {'default us':>10s} {'step':>7s} {'lean us':>10s} {'step':>7s}")
    prev = [0.0, 0.0]
    for probe, name in PHASES:
        us = [timed(probe, lean) for lean in (0, 1)]
        print(f"{name:38s} {us[0]:10.2f} {us[0] - prev[0]:+7.2f} {us[1]:10.2f} {us[1] - prev[1]:+7.2f}")
        prev = us
    print()


if __name__ == "__main__":
    main()
