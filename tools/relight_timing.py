"""What relighting costs through the fused lit chains (`fused_relight_infer`: the chains' _relit entries) against the switch off
(forward() on all rows, the path without the switch) -- the same process, the two forms in alternating windows, fp16 autocast, eval:
  1. CurvedField(light_model="SH").infer() at 262 144 rows under per-probe imported lighting (the reference's 64 probes), switch on / off;
  2. the same with a lighting rotation added;
  3. one 800 x 800 frame through Renderer.render_infer_graphed under per-probe lighting, on / off;
  4. a 16-frame light turntable (Renderer.render_light_turntable) with the switch on: ms per frame and how often the graphs were recorded.
The uniform-lighting chain (no relighting: the plain entry) is timed by tools/curved_light_infer_timing.py, unchanged.
    timeout 900 python tools/relight_timing.py > profiles/relight_timing.json"""
import argparse
import json
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-texture_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frame", type=int, default=800, help="edge of the graphed frame in pixels (0: skip the frame and the turntable)")
    ap.add_argument("--frame-reps", type=int, default=4)
    ap.add_argument("--turntable", type=int, default=16)
    a = ap.parse_args()
    import numpy as np
    import torch

    from ngp_harness import scene
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer, _InferGraphPart

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev, B = torch.device("cuda:0"), a.samples // 128 * 128
    v, f = star_flower_mesh()
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05, light_model="SH").to(dev).eval()
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
        field.normal_net.encoder.embeddings.uniform_(-0.5, 0.5)
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_python_envmap.npz"))  # (the reference's 8 x 8 probe grid, seeded tables)
    field.light_net.load_envmap(env_shs=g["uniform_env_shs"], env_shs_vis=g["probe_shs"], probes=g["probes"])
    field.fused_light_infer = True
    rng = np.random.default_rng(0)
    ids = rng.integers(0, v.shape[0], B)
    vn = field.projector.vertex_normals.cpu().numpy()
    x = torch.from_numpy((v[ids] + rng.uniform(-0.0714, 0.0714, size=(B, 1)).astype(np.float32) * vn[ids]).astype(np.float32)).to(dev)
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=dev), dim=-1)
    euler = [0.4, -1.1, 0.7]

    def run(on, rotate):
        field.fused_relight_infer = on
        field.set_light_rotation(euler if rotate else None)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return field.infer(x, d)

    look = {}
    for rotate in (False, True):
        (s_on, c_on), (s_off, c_off) = run(True, rotate), run(False, rotate)
        look["rotated" if rotate else "per_probe"] = {"sigma_equal": bool(torch.equal(s_on, s_off)), "max_abs_colour_difference_between_forms": float((c_on - c_off).abs().max()),
                                                      "rows_whose_colour_differs_by_more_than_2e-2": int(((c_on - c_off).abs().amax(-1) > 2e-2).sum())}
    look["share_of_rows_inside_the_mask"] = round(float((s_off != 0).float().mean()), 4)
    cases = {"per_probe": False, "per_probe_rotated": True}
    times = {f"{name}_{'on' if on else 'off'}": [] for name in cases for on in (True, False)}
    for rotate in cases.values():
        for on in (True, False):
            for _ in range(3):
                run(on, rotate)
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for name, rotate in cases.items():
            for on in (True, False):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                run(on, rotate)  # (sets the state; the rotation's host-to-device copy stays outside the window)
                t0.record()
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    for _ in range(a.iters):
                        field.infer(x, d)
                t1.record()
                torch.cuda.synchronize()
                times[f"{name}_{'on' if on else 'off'}"].append(t0.elapsed_time(t1) * 1e3 / a.iters)
    out = {"what": f"CurvedField(light_model='SH').infer(), {B} rows, fp16 autocast, eval, fc_weight 1.0, the default 20 k-triangle star-flower mesh, an imported "
                   f"lighting with the reference's 64 probes (shade_visibility); us per call between device events around {a.iters} eager calls (host launch "
                   f"time included for both forms), {a.reps} alternating windows; on = fused_relight_infer (nerftex_curved_light_infer_relit), off = "
                   "forward() on all rows (the path without the switch); rotated: set_light_rotation([0.4, -1.1, 0.7])",
           "box": socket.gethostname(), "device": torch.cuda.get_device_name(0),
           "look": look,
           "median_us": {k: round(statistics.median(t), 1) for k, t in times.items()},
           "min_max_us": {k: [round(min(t), 1), round(max(t), 1)] for k, t in times.items()}}
    out["off_over_on"] = {name: round(out["median_us"][name + "_off"] / out["median_us"][name + "_on"], 2) for name in cases}
    if a.frame:
        field.set_light_rotation(None)
        r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
        with torch.autocast("cuda", dtype=torch.float16):
            r.update_extra_state_device()
        o, dd = scene.get_rays(scene.rand_poses(1, 1.6, np.random.default_rng(11))[0], scene.intrinsics(a.frame, a.frame), a.frame, a.frame)
        ro, rd = torch.from_numpy(o).to(dev), torch.from_numpy(dd).to(dev)
        frames, images = {"on": [], "off": []}, {}
        for _ in range(2):  # on, off, on, off: a flipped switch re-records the graphs (one untimed call), then frame_reps replaying calls
            for on in (True, False):
                field.fused_relight_infer = on
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
        out["frame"] = {"what": f"one {a.frame} x {a.frame} frame under per-probe lighting, render_infer_graphed (3 slots per ray, 3 ranges, blocks of 2 iterations, "
                                "max_steps 256), ms between device events around a replaying call; on, off, on, off -- the graphs are re-recorded when the switch "
                                "flips, outside the timed calls",
                        "median_ms": {k: round(statistics.median(t), 2) for k, t in frames.items()},
                        "min_max_ms": {k: [round(min(t), 2), round(max(t), 2)] for k, t in frames.items()},
                        "iterations": int(r.last_iters), "max_abs_image_difference_between_forms": float((images[True] - images[False]).abs().max())}
        out["frame"]["off_over_on"] = round(out["frame"]["median_ms"]["off"] / out["frame"]["median_ms"]["on"], 2)
        # the turntable, switch on: every capture of a ray range's graphs is counted
        field.fused_relight_infer = True
        captures, capture = [], _InferGraphPart.capture
        _InferGraphPart.capture = lambda self: (captures.append(1), capture(self))[1]
        per_frame, recorded_at = [], []
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                t0 = torch.cuda.Event(enable_timing=True)
                t0.record()
                seen = None
                for i, _ in enumerate(r.render_light_turntable(ro, rd, a.turntable, axis=0, dt_gamma=0.0, max_steps=256)):
                    t1 = torch.cuda.Event(enable_timing=True)
                    t1.record()
                    torch.cuda.synchronize()
                    per_frame.append(t0.elapsed_time(t1))
                    if r._infer_graphs is not seen:
                        recorded_at.append(i)
                        seen = r._infer_graphs
                    t0 = torch.cuda.Event(enable_timing=True)
                    t0.record()
        finally:
            _InferGraphPart.capture = capture
        replayed = [t for i, t in enumerate(per_frame) if i not in recorded_at]
        out["turntable"] = {"what": f"render_light_turntable, {a.turntable} frames of {a.frame} x {a.frame} on euler[0], switch on, per-probe lighting; ms per frame "
                                    "between device events (set_light_rotation and its 36-byte copy included), the frames that recorded listed apart",
                            "graph_recordings": len(recorded_at), "frames_that_recorded": recorded_at, "ray_range_captures": len(captures),
                            "recording_frame_ms": [round(per_frame[i], 2) for i in recorded_at],
                            "replayed_median_ms": round(statistics.median(replayed), 2), "replayed_min_max_ms": [round(min(replayed), 2), round(max(replayed), 2)]}
    field.fused_relight_infer = field.fused_light_infer = False
    field.set_light_rotation(None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
