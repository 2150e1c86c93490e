"""What rendering an imported planar feature texture costs (CurvedField.import_field): the same process, the forms in alternating windows:
  * the lookup entry (nerftex_planar_lookup: one launch) against the reference's expressions as framework ops (grid_sample, the mask, the
    height ladder: CurvedField._import_embed_reference) -- the FRAMEWORK BASELINE, not a bar;
  * infer() through nerftex_curved_import_infer (one library call, five launches) against forward() op by op (fused_glue = False);
  * one 800 x 800 frame through Renderer.render_infer_graphed.
262 144 rows, a 1024 x 1024 x 16 fp32 map (64 MiB), about 70 % of the rows inside the mask, fp16 autocast.
    timeout 900 python tools/import_field_timing.py > profiles/import_field_timing.json"""
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
    ap.add_argument("--map", type=int, default=1024, help="edge of the square feature map in texels")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frame", type=int, default=800, help="edge of the graphed frame in pixels (0: skip it)")
    ap.add_argument("--frame-reps", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch

    from ngp_harness import scene
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev, B, h = torch.device("cuda:0"), a.samples // 128 * 128, 0.0625
    v, f = star_flower_mesh(n_lat=18, n_lon=36)  # (the mesh is not read in import mode)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=h).to(dev).eval()
    with torch.no_grad():
        field.sigma_net.weights.mul_(3.0)
    gen = torch.Generator(device=dev).manual_seed(1)
    field.import_field(torch.rand(a.map, a.map, 16, device=dev, generator=gen) - 0.5, 1.0 / a.map)  # bounds (0.5, 0.5), rescale: u, v = x, y; sdf = z / 2
    x = torch.rand(B, 3, device=dev, generator=gen) * 2 - 1
    x[:, 2] *= 2 * h / 0.7  # |z / 2| < h on 70 % of the rows
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=dev, generator=gen), dim=-1)

    def lookup_kernel():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return field._import_lookup(x)

    def lookup_framework():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return field._import_embed_reference(x)

    def infer(fused):
        field.fused_glue = fused
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return field.infer(x, d)
        finally:
            field.fused_glue = True

    import nerftex_hip

    forms = {"lookup_kernel": lookup_kernel, "lookup_framework_baseline": lookup_framework, "infer_fused": lambda: infer(True),
             "infer_op_by_op": lambda: infer(False)}
    mask = lookup_kernel()[2]
    s_f, c_f = infer(True)
    s_o, c_o = infer(False)
    look = {"share_of_rows_inside_the_mask": round(float(mask.float().mean()), 4), "mask_equal_between_lookup_forms": bool(torch.equal(mask, lookup_framework()[2])),
            # (the glue kernels round sigma to half, as the mesh field's do; the op-by-op chain keeps trunc_exp's fp32: a logit above 11.09 is inf in half)
            "rows_whose_half_sigma_overflows": int((~torch.isfinite(s_f)).sum()),
            "max_rel_sigma_difference_fused_vs_op_by_op": float(((s_f - s_o).abs() / s_o.clamp(min=1e-3))[torch.isfinite(s_f)].max()),
            "max_abs_colour_difference_fused_vs_op_by_op": float((c_f - c_o).abs().max())}
    times = {k: [] for k in forms}
    for fn in forms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for name, fn in forms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e3 / a.iters)
    out = {"what": f"CurvedField with an imported {a.map} x {a.map} x 16 fp32 map, {B} rows, fp16 autocast, eval; us per call between device events around "
                   f"{a.iters} eager calls (host launch time and the output allocations included for every form), {a.reps} alternating windows, median (min .. max). "
                   "lookup_kernel = nerftex_planar_lookup, one thread per row; lookup_framework_baseline = the reference's expressions as framework ops "
                   "(a baseline, not a bar); infer_fused = nerftex_curved_import_infer; infer_op_by_op = forward() with fused_glue = False",
           "look": look,
           "median_us": {k: round(statistics.median(t), 1) for k, t in times.items()},
           "min_max_us": {k: [round(min(t), 1), round(max(t), 1)] for k, t in times.items()}}
    # the device time of the chain's launches alone (the library's own event pairs around each kernel; no host time), 3 windows
    chain = []
    for _ in range(3):
        nerftex_hip.kernel_profile(True, reset=True)
        for _ in range(a.iters):
            infer(True)
        torch.cuda.synchronize()
        prof = nerftex_hip.kernel_profile()
        nerftex_hip.kernel_profile(False)
        chain.append({k: v["avg_us"] for k, v in prof.items()})
    out["chain_kernels_avg_us"] = {k: round(statistics.median(w[k] for w in chain), 2) for k in chain[0]}
    out["lookup_kernel_avg_us"] = [round(w["planar_lookup_rows_kernel"], 2) for w in chain]
    out["lookup_bytes_per_row"] = {"read": 12 + 4 * 64, "written_rows_form": 1 + 12 + 96}
    out["framework_over_kernel"] = round(out["median_us"]["lookup_framework_baseline"] / out["median_us"]["lookup_kernel"], 2)
    out["op_by_op_over_fused"] = round(out["median_us"]["infer_op_by_op"] / out["median_us"]["infer_fused"], 2)
    if a.frame:
        r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
        r.initialize_states(2)
        o, dd = scene.get_rays(scene.rand_poses(1, 1.6, np.random.default_rng(11))[0], scene.intrinsics(a.frame, a.frame), a.frame, a.frame)
        ro, rd = torch.from_numpy(o).to(dev), torch.from_numpy(dd).to(dev)
        frames = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            img = r.render_infer_graphed(ro, rd, dt_gamma=0.0, max_steps=256)[0]  # records the graphs
            torch.cuda.synchronize()
            for _ in range(a.frame_reps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                img = r.render_infer_graphed(ro, rd, dt_gamma=0.0, max_steps=256)[0]
                t1.record()
                torch.cuda.synchronize()
                frames.append(t0.elapsed_time(t1))
        out["frame"] = {"what": f"one {a.frame} x {a.frame} frame of the imported map, render_infer_graphed (3 slots per ray, 3 ranges, blocks of 2 iterations, max_steps 256), "
                                "ms between device events around a replaying call",
                        "median_ms": round(statistics.median(frames), 2), "min_max_ms": [round(min(frames), 2), round(max(frames), 2)],
                        "iterations": int(r.last_iters), "image_std": float(img.std())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
