"""What rendering an imported texture through the SH-lit curved field costs (CurvedField.import_field with the phi_embed, local_tbn, sample_tbn and
sample_tbn_ids maps): the same process, the forms in alternating windows --
  * infer() through nerftex_curved_light_import_infer (one library call, five launches) against forward() on all rows (the switch off);
  * its two neighbours: nerftex_curved_import_infer (the same feature map under the static light model: the same lookup without the lit reads) and
    nerftex_curved_light_infer (the same back half behind the mesh front: neighbour search, projector, two hash-grid gathers);
  * the device time of every launch of the three chains (the library's own event pairs, the KernelTimer labels).
262 144 rows, 1024 x 1024 maps (16 features, 8 phi features, a 12-float frame texel), 64 patch frames, about 70 % of the rows inside the mask, fp16 autocast.
    timeout 900 python tools/import_light_timing.py > profiles/import_light_timing.json"""
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
    ap.add_argument("--map", type=int, default=1024, help="edge of the square maps in texels")
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch

    import nerftex_hip
    from ngp_harness.curved import CurvedField, star_flower_mesh

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev, B, h, M, P = torch.device("cuda:0"), a.samples // 128 * 128, 0.0625, a.map, a.patches
    v, f = star_flower_mesh(n_lat=72, n_lon=144)  # (20 k triangles: the mesh neighbour's front half; not read in import mode)
    gen = torch.Generator(device=dev).manual_seed(1)
    features = torch.rand(M, M, 16, device=dev, generator=gen) - 0.5

    def make(light):
        torch.manual_seed(0)
        field = CurvedField(v, f, bound=1.0, h_threshold=h, light_model=light).to(dev).eval()
        with torch.no_grad():
            field.sigma_net.weights.mul_(3.0)
            field.encoder.embeddings.uniform_(-0.5, 0.5)
        return field

    lit, unlit = make("SH"), make(None)
    with torch.no_grad():
        lit.normal_net.encoder.embeddings.uniform_(-0.5, 0.5)
        for mlp in (lit.normal_net.phi_net, lit.normal_net.theta_net):
            for layer in mlp.layers:
                layer.W.mul_(6.0)
                layer.c.fill_(2.0)
    lit.fc_weight = 0.7
    frames = torch.eye(3, device=dev).reshape(9) + 0.35 * torch.randn(M, M, 9, device=dev, generator=gen)
    patches = torch.eye(3, device=dev) + 0.2 * torch.randn(P, 3, 3, device=dev, generator=gen)
    ids = torch.randint(0, P, (M, M), device=dev, generator=gen).float()
    lit.import_field(features, 1.0 / M, phi_embed=torch.rand(M, M, 8, device=dev, generator=gen) - 0.5, local_tbn=frames, sample_tbn=patches, sample_tbn_ids=ids)
    unlit.import_field(features, 1.0 / M)  # bounds (0.5, 0.5), rescale: u, v = x, y; sdf = z / 2
    x = torch.rand(B, 3, device=dev, generator=gen) * 2 - 1
    x[:, 2] *= 2 * h / 0.7  # |z / 2| < h on 70 % of the rows
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=dev, generator=gen), dim=-1)
    # the mesh neighbour's points: within +-0.1 of the surface, as tools/import_shape_timing.py
    vn = lit.projector.vertex_normals
    pick = torch.randint(0, v.shape[0], (B,), device=dev, generator=gen)
    xm = (lit.projector.mesh_vertices[pick] + (torch.rand(B, 1, device=dev, generator=gen) * 0.2 - 0.1) * vn[pick]).contiguous()

    def run(field, pts, fused, imported):
        if field.imported != imported:
            field.switch_import()
        field.fused_light_infer = fused
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return field.infer(pts, d)

    forms = {"light_import_fused": lambda: run(lit, x, True, True), "light_import_forward_all_rows": lambda: run(lit, x, False, True),
             "import_fused_static_light": lambda: run(unlit, x, False, True), "light_mesh_fused": lambda: run(lit, xm, True, False)}
    s_f, c_f = forms["light_import_fused"]()
    s_o, c_o = forms["light_import_forward_all_rows"]()
    look = {"share_of_rows_inside_the_mask": round(float((s_f != 0).float().mean()), 4), "sigma_equal_fused_vs_forward": bool(torch.equal(s_f, s_o)),
            "max_abs_colour_difference_fused_vs_forward": float((c_f - c_o).abs().max()),
            "share_of_rows_inside_the_mask_mesh_neighbour": round(float((forms["light_mesh_fused"]()[0] != 0).float().mean()), 4)}
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
    out = {"what": f"CurvedField(light_model='SH') with imported {M} x {M} maps (16 features, 8 phi features, frame texels of 12 floats), {P} patch frames, {B} rows, "
                   f"fp16 autocast, eval, fc_weight 0.7; us per call between device events around {a.iters} eager calls (host launch time and the output "
                   f"allocations included for every form), {a.reps} alternating windows, median (min .. max).  light_import_fused = nerftex_curved_light_import_infer; "
                   "light_import_forward_all_rows = forward() with the switch off; import_fused_static_light = nerftex_curved_import_infer over the same feature map; "
                   "light_mesh_fused = nerftex_curved_light_infer on the field's own mesh (20 k triangles), points within 0.1 of it",
           "look": look,
           "median_us": {k: round(statistics.median(t), 1) for k, t in times.items()},
           "min_max_us": {k: [round(min(t), 1), round(max(t), 1)] for k, t in times.items()}}
    chains = {}
    for _ in range(a.reps):
        for name in ("light_import_fused", "import_fused_static_light", "light_mesh_fused"):
            nerftex_hip.kernel_profile(True, reset=True)
            for _ in range(a.iters):
                forms[name]()
            torch.cuda.synchronize()
            prof = nerftex_hip.kernel_profile()
            nerftex_hip.kernel_profile(False)
            chains.setdefault(name, []).append({k: (v["avg_us"], v["calls"] // a.iters) for k, v in prof.items()})
    out["launches_avg_us"] = {name: {k: {"median": round(statistics.median(w[k][0] for w in wins), 2), "min": round(min(w[k][0] for w in wins), 2),
                                         "max": round(max(w[k][0] for w in wins), 2), "launches_per_call": wins[0][k][1]} for k in wins[0]}
                              for name, wins in chains.items()}
    out["chain_device_us"] = {name: round(sum(e["median"] * e["launches_per_call"] for e in ks.values()), 1) for name, ks in out["launches_avg_us"].items()}
    read = 12 + 4 + 4 * 64 + 4 * 32 + 48 + 48
    written = 1 + 12 + 96 + 16 + 36 + 36
    lk = out["launches_avg_us"]["light_import_fused"]["planar_light_lookup_rows_kernel"]["median"]
    out["lookup_bytes_per_row"] = {"read": read, "read_as_random_texels": 4 * 64 + 4 * 32 + 48, "written_rows_form": written,
                                   "inside_share_ignored_TB_per_s": round((read + written) * B / (lk * 1e-6) / 1e12, 2)}
    out["forward_over_fused"] = round(out["median_us"]["light_import_forward_all_rows"] / out["median_us"]["light_import_fused"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
