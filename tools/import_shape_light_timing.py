"""What rendering imported maps on a new UV-mapped mesh costs under the SH light model (CurvedField.import_shape(new_tbn=...)), by the library's
own event pairs around each kernel (nerftex_profile_enable; no host time) and between device events around whole eager calls, the chains in
alternating windows of one process:
  * nerftex_curved_light_shape_infer of the lit field (neighbour search, lit shape lookup, sigma net, three-frame light mid, BRDF net, light out);
  * nerftex_curved_shape_infer of an unlit field over the SAME mesh and feature map (the same lookup without the lit reads, static light);
  * forward() of the lit field on all rows (the switch off): context, never the baseline.
262 144 rows within +-0.1 of star_flower_mesh(72, 144) (20 k triangles), 1024 x 1024 maps (64 + 32 + 48 MiB), 64 patch frames, fp16 autocast.
    timeout 600 python tools/import_shape_light_timing.py > profiles/import_shape_light_timing.json"""
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
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch

    import nerftex_hip
    from ngp_harness.curved import CurvedField, shape_preprocess, star_flower_mesh, uv_face_frames, vertex_normals

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev, B, h = torch.device("cuda:0"), a.samples // 128 * 128, 0.0625
    v, f = star_flower_mesh()
    gen = torch.Generator(device=dev).manual_seed(1)
    # per-vertex UVs from the sphere's angles (a seam at phi = 0: one column of long UV edges, as an unwrapped sphere has)
    r = np.linalg.norm(v, axis=-1)
    uvs = np.stack([np.arctan2(v[:, 2], v[:, 0]) / np.pi, 2 * np.arccos(np.clip(v[:, 1] / r, -1, 1)) / np.pi - 1], -1).astype(np.float32)
    # the reference's frames; the faces at the poles have no area (duplicated vertices) and get the identity -- no point's nearest hit is one of them
    uv = shape_preprocess(v, f, uvs, normalize=False)[1]
    fi = f.astype(np.int64)
    area = np.linalg.norm(np.cross(v[fi[:, 1]] - v[fi[:, 0]], v[fi[:, 2]] - v[fi[:, 0]]).astype(np.float64), axis=-1)
    e2 = (uv[fi][:, 1:] - uv[fi][:, :1]).astype(np.float64)
    good = (area > 1e-12) & (np.abs(np.linalg.det(e2)) > 1e-9)
    frames = np.tile(np.eye(3, dtype=np.float32), (len(f), 1, 1))
    frames[good] = uv_face_frames(v, fi[good], uv)
    bad = ~good | ~np.isfinite(frames).all((1, 2))
    frames[bad] = np.eye(3, dtype=np.float32)
    rng = np.random.default_rng(2)
    pick = rng.integers(0, len(v), B)
    vn = vertex_normals(v, f).numpy()
    x = torch.from_numpy((v[pick] + vn[pick] * rng.uniform(-0.1, 0.1, (B, 1)) + rng.normal(0, 0.01, (B, 3))).astype(np.float32)).to(dev)
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=dev, generator=gen), dim=-1)
    fmap = torch.rand(a.map, a.map, 16, device=dev, generator=gen) - 0.5

    fields = {}
    for name, light in (("unlit_shape", None), ("lit_shape", "SH")):
        torch.manual_seed(0)
        field = CurvedField(v, f, bound=1.0, h_threshold=h, light_model=light).to(dev).eval()
        with torch.no_grad():
            field.encoder.embeddings.uniform_(-0.5, 0.5)
        if light:
            field.fused_light_infer = True
            phi = torch.rand(a.map, a.map, 8, device=dev, generator=gen) - 0.5
            local = torch.eye(3, device=dev).reshape(9) + 0.35 * torch.randn(a.map, a.map, 9, device=dev, generator=gen)
            sample = torch.eye(3, device=dev) + 0.3 * torch.randn(a.patches, 3, 3, device=dev, generator=gen)
            ids = torch.randint(0, a.patches, (a.map, a.map), device=dev, generator=gen).float()
            field.import_field(fmap, 1.0 / a.map, phi_embed=phi, local_tbn=local, sample_tbn=sample, sample_tbn_ids=ids)
            field.import_shape(v, f, uvs, normalize=False, new_tbn=frames)
        else:
            field.import_field(fmap, 1.0 / a.map)
            field.import_shape(v, f, uvs, normalize=False)
        field.set_sdf_factor(1.0)
        fields[name] = field

    def call(field, how="infer"):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            if how == "infer":
                return field.infer(x, d)
            return field(x, d)[:2]

    def window(field):
        for _ in range(a.iters):
            call(field)
        torch.cuda.synchronize()
        nerftex_hip.kernel_profile(True, reset=True)
        for _ in range(a.iters):
            call(field)
        torch.cuda.synchronize()
        prof = nerftex_hip.kernel_profile()
        nerftex_hip.kernel_profile(False)
        runs = {k: p["avg_us"] for k, p in prof.items()}
        runs["chain_total"] = sum(p["total_us"] for p in prof.values()) / a.iters  # (the FFMLP kernel runs twice per call)
        return runs

    def whole(field, how, iters):
        for _ in range(3):
            call(field, how)
        torch.cuda.synchronize()
        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        for _ in range(iters):
            call(field, how)
        a1.record()
        torch.cuda.synchronize()
        return a0.elapsed_time(a1) * 1e3 / iters

    per = {name: [] for name in fields}
    calls = {"unlit_shape_infer": [], "lit_shape_infer": [], "lit_shape_forward": []}
    lit = fields["lit_shape"]
    for w in range(a.windows):
        for name, field in fields.items():
            per[name].append(window(field))
        calls["unlit_shape_infer"].append(whole(fields["unlit_shape"], "infer", a.iters))
        calls["lit_shape_infer"].append(whole(lit, "infer", a.iters))
        lit.fused_light_infer = False
        calls["lit_shape_forward"].append(whole(lit, "forward", 5))
        lit.fused_light_infer = True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        mask = lit._shape_light_lookup(x)[2]
        s_f, c_f = lit.infer(x, d)
        lit.fused_light_infer = False
        s_e, c_e = call(lit, "forward")
    K = lit._shape_scalars()[0]
    med = lambda xs: [round(statistics.median(xs), 2), round(min(xs), 2), round(max(xs), 2)]  # noqa: E731
    out = {"what": f"{B} rows within +-0.1 of star_flower_mesh(72, 144), {a.map} x {a.map} maps (16 + 8 + 12 floats per texel), {a.patches} patch frames, fp16 autocast, "
                   f"eval; avg us per launch by the library's event pairs over {a.iters} calls, {a.windows} alternating windows, median (min .. max) per kernel; "
                   "chain_total = all of a call's launches together; whole_call_us = between device events around eager calls (host launch time included)",
           "share_of_rows_inside_the_mask": round(float(mask.float().mean()), 4), "K_for_uv": K, "faces_without_area_given_the_identity": int(bad.sum()),
           "sigma_equal_fused_and_forward": bool(torch.equal(s_f, s_e.float())), "largest_colour_difference_fused_and_forward": float((c_f - c_e.float()).abs().max())}
    for name, ws in per.items():
        out[name] = {k: med([w[k] for w in ws]) for k in ws[0]}
    out["whole_call_us"] = {k: med(vs) for k, vs in calls.items()}
    out["lit_lookup_bytes_per_row"] = {"read": f"the unlit lookup's (12 + {8 * K} + {24 * K} + the BVH walk + 48 + 24 + 4 x 64) + 48 (the nearest frame texel) + 48 (the patch "
                                               "frame) + 4 x 32 (phi texels) + 8 + 48 (the hit's id and face frame, lane 1)",
                                       "written_rows_form": 1 + 12 + 96 + 16 + 3 * 36, "written_by_the_unlit_rows_form": 1 + 12 + 96}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
