"""What the device-count inference path buys the curved field: one 800 x 800 frame of bench.py's configs[3] scene (the star_flower-shaped mesh,
CurvedField(bound=1, h_threshold=0.05) with a table and a sigma net that make a thin opaque shell, its own occupancy grid), fp16 autocast, as
  reference   Renderer.render_infer, the reference loop (one alive-count read-back per iteration),
  pipelined   Renderer.render_infer_pipelined(slots_per_ray=4, parts=3): CurvedField.infer where the tree has it (nerftex_curved_field_infer
              behind the loop's device count), else forward() on every row of the buffer,
  graphed     Renderer.render_infer_graphed(slots_per_ray=3, parts=3), where the tree's CurvedField has `infer`,
each form in a process of its own under a time limit, `--frames` timed frames after a warm-up frame, `--reps` times, interleaved; the first child
that fails ends the run.  `--parent TREE`: a built checkout of the parent commit whose forms are timed beside this tree's ("parent_*"); the
child code uses only what both trees have.
Per form: ms per frame, Mpix/s, iterations, and the share of the rows its field launches covered that held a sample (delta > 0: live and
unmarked) -- samples counted by the reference loop run with the form's slots_per_ray, rows as the form reports them (for the graphed loop: the
full-size launches, an upper bound) -- and the image's distance from that reference loop's plus its SHA-1 (the same form of two trees: the same
digest).
`claim`: the graphed frame counts as faster only if its median beats the parent's best form's median by more than the spread (max - min) of that
form's own runs.
    python tools/curved_infer_ab.py [--parent ../parent] > profiles/curved_infer_ab.json"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"reference": dict(slots_per_ray=1), "pipelined": dict(slots_per_ray=4, parts=3), "graphed": dict(slots_per_ray=3, parts=3)}


def child(tree, form, side, frames):
    sys.path[:0] = [tree, os.path.join(tree, "nerf-texture_amd")]
    import numpy as np
    import torch

    from ngp_harness import scene
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer

    dev = torch.device("cuda:0")
    v, f = star_flower_mesh()
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
    field.eval()
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    pose = scene.rand_poses(1, 1.6, np.random.default_rng(3))[0]
    o, d = scene.get_rays(pose, scene.intrinsics(side, side), side, side)
    ro, rd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    kw = FORMS[form]
    render = {"reference": r.render_infer, "pipelined": r.render_infer_pipelined, "graphed": getattr(r, "render_infer_graphed", None)}[form]
    if form == "graphed" and not hasattr(field, "infer"):
        sys.exit("this tree's CurvedField has no infer(): no graphed form")
    with torch.autocast("cuda", dtype=torch.float16):
        r.update_extra_state_device()
        r.count_real_samples, r.real_samples = True, 0
        img_ref, _, _ = r.render_infer(ro, rd, dt_gamma=0.0, slots_per_ray=kw["slots_per_ray"])  # (also the warm-up of the lazily made 16-bit copies)
        real = int(r.real_samples)
        r.count_real_samples = False
        for _ in range(2 if form == "graphed" else 1):  # (graphed: the first frame records)
            img, _, rows = render(ro, rd, dt_gamma=0.0, **kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(frames):
            t0 = time.perf_counter()
            img, _, rows = render(ro, rd, dt_gamma=0.0, **kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
    best = min(ms)
    print(json.dumps({"form": form, "ms_per_frame": round(statistics.median(ms), 3), "ms_frames": [round(x, 3) for x in ms], "ms_best": round(best, 3),
                      "mpix_per_s": round(side * side / statistics.median(ms) / 1e3, 2), "iterations": int(r.last_iters), "rows_launched": int(rows),
                      "samples": real, "share_live_unmarked": round(real / max(int(rows), 1), 4), "equals_reference": bool(torch.equal(img, img_ref)),
                      "pixels_off_reference": int((img != img_ref).any(-1).sum()), "max_abs_off_reference": float((img - img_ref).abs().max()),
                      "image_sha1": hashlib.sha1(img.cpu().numpy().tobytes()).hexdigest(),
                      "uses_infer": hasattr(field, "infer")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--side", type=int, default=800)
    ap.add_argument("--limit", type=int, default=150, help="seconds a child may take")
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.side, a.frames)
    forms = [("parent_" + f, os.path.abspath(a.parent), f) for f in ("reference", "pipelined")] if a.parent else []
    forms += [(f, ROOT, f) for f in ("reference", "pipelined", "graphed")]
    runs = {name: [] for name, _, _ in forms}
    for _ in range(a.reps):
        for name, tree, form in forms:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, form, "--side", str(a.side), "--frames", str(a.frames)],
                                   capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                sys.exit(f"{name}: no result within {a.limit} s")  # (nothing more is started on the GPU)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-2000:])
                sys.exit(f"{name}: exit status {p.returncode}")
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
            sys.stderr.write(f"{name}: {runs[name][-1]['ms_per_frame']} ms\n")
    ms = {k: [x["ms_per_frame"] for x in v] for k, v in runs.items()}
    out = {"what": f"one {a.side} x {a.side} frame of the configs[3] scene through a CurvedField, fp16 autocast, dt_gamma = 0, median of {a.frames} timed frames "
                   f"after warm-up, {a.reps} interleaved runs per form, one process per run", "ms_per_frame": ms,
           "mpix_per_s": {k: [x["mpix_per_s"] for x in v] for k, v in runs.items()}, "runs": runs}
    base = [k for k in ms if k.startswith("parent_")] or ["reference"]
    best = min(base, key=lambda k: statistics.median(ms[k]))
    spread = max(ms[best]) - min(ms[best])
    gain = statistics.median(ms[best]) - statistics.median(ms["graphed"])
    out["claim"] = {"baseline": best, "baseline_median_ms": statistics.median(ms[best]), "baseline_spread_ms": round(spread, 3),
                    "graphed_median_ms": statistics.median(ms["graphed"]), "graphed_faster": bool(gain > spread)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
