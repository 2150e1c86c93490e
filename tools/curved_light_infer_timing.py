"""What CurvedField(light_model="SH").infer() costs with `fused_light_infer` on (nerftex_curved_light_infer: one library call, ten launches)
against the switch off (forward() on all rows: the framework-op chain with the fused head) -- the same process, the two forms in alternating
windows:
  * 262 144 rows, about 70 % of them inside the height mask, fp16 autocast: once with every row live, once with half of the units live (the
    switch-off form does not know about live rows: it shades all of them either way);
  * one 800 x 800 frame through Renderer.render_infer_graphed each way.
    timeout 900 python tools/curved_light_infer_timing.py > profiles/curved_light_infer_timing.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-texture_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frame", type=int, default=800, help="edge of the graphed frame in pixels (0: skip it)")
    ap.add_argument("--frame-reps", type=int, default=4)
    a = ap.parse_args()
    import numpy as np
    import torch

    from ngp_harness import scene
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev, B = torch.device("cuda:0"), a.samples // 128 * 128
    v, f = star_flower_mesh()
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05, light_model="SH").to(dev).eval()
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
        field.normal_net.encoder.embeddings.uniform_(-0.5, 0.5)
        field.light_net.envSHs[1:].normal_(0, 0.1)
    rng = np.random.default_rng(0)
    ids = rng.integers(0, v.shape[0], B)
    vn = field.projector.vertex_normals.cpu().numpy()
    x = torch.from_numpy((v[ids] + rng.uniform(-0.0714, 0.0714, size=(B, 1)).astype(np.float32) * vn[ids]).astype(np.float32)).to(dev)
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=dev), dim=-1)
    half = (torch.tensor([B // 256], dtype=torch.int32, device=dev), 128)

    def run(on, live):
        field.fused_light_infer = on
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return field.infer(x, d, live)

    s_on, c_on = run(True, None)
    s_off, c_off = run(False, None)
    inside = float((s_off != 0).float().mean())
    look = {"share_of_rows_inside_the_mask": round(inside, 4), "sigma_equal": bool(torch.equal(s_on, s_off)),
            "max_abs_colour_difference_between_forms": float((c_on - c_off).abs().max())}
    cases = {"all_live": None, "half_live": half}
    times = {f"{name}_{'on' if on else 'off'}": [] for name in cases for on in (True, False)}
    for name, live in cases.items():
        for on in (True, False):
            for _ in range(5):
                run(on, live)
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for name, live in cases.items():
            for on in (True, False):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    run(on, live)
                t1.record()
                torch.cuda.synchronize()
                times[f"{name}_{'on' if on else 'off'}"].append(t0.elapsed_time(t1) * 1e3 / a.iters)
    out = {"what": f"CurvedField(light_model='SH').infer(), {B} rows, fp16 autocast, eval, fc_weight 1.0, the default 20 k-triangle star-flower mesh; "
                   f"us per call between device events around {a.iters} eager calls (host launch time included for both forms), {a.reps} alternating "
                   "windows; on = fused_light_infer (nerftex_curved_light_infer), off = forward() on all rows; half_live: units_dev says half of the rows",
           "look": look,
           "median_us": {k: round(statistics.median(t), 1) for k, t in times.items()},
           "min_max_us": {k: [round(min(t), 1), round(max(t), 1)] for k, t in times.items()}}
    out["off_over_on"] = {name: round(out["median_us"][name + "_off"] / out["median_us"][name + "_on"], 2) for name in cases}
    if a.frame:
        r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
        with torch.autocast("cuda", dtype=torch.float16):
            r.update_extra_state_device()
        o, dd = scene.get_rays(scene.rand_poses(1, 1.6, np.random.default_rng(11))[0], scene.intrinsics(a.frame, a.frame), a.frame, a.frame)
        ro, rd = torch.from_numpy(o).to(dev), torch.from_numpy(dd).to(dev)
        frames = {"on": [], "off": []}
        images = {}
        for _ in range(2):  # on, off, on, off: a flipped switch re-records the graphs (one untimed call), then frame_reps replaying calls
            for on in (True, False):
                field.fused_light_infer = on
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    r.render_infer_graphed(ro, rd, dt_gamma=0.0, max_steps=256)
                    torch.cuda.synchronize()
                    for _ in range(a.frame_reps):
                        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        t0.record()
                        images[on] = r.render_infer_graphed(ro, rd, dt_gamma=0.0, max_steps=256)[0]
                        t1.record()
                        torch.cuda.synchronize()
                        frames["on" if on else "off"].append(t0.elapsed_time(t1))
        out["frame"] = {"what": f"one {a.frame} x {a.frame} frame, render_infer_graphed (3 slots per ray, 3 ranges, blocks of 2 iterations, max_steps 256), ms between "
                                "device events around a replaying call; on, off, on, off -- the graphs are re-recorded when the switch flips, outside the timed calls",
                        "median_ms": {k: round(statistics.median(t), 2) for k, t in frames.items()},
                        "min_max_ms": {k: [round(min(t), 2), round(max(t), 2)] for k, t in frames.items()},
                        "iterations": int(r.last_iters), "max_abs_image_difference_between_forms": float((images[True] - images[False]).abs().max())}
    field.fused_light_infer = False
    print(json.dumps(out))


if __name__ == "__main__":
    main()
