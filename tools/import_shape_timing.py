"""What rendering an imported feature map on a new UV-mapped mesh costs (CurvedField.import_shape), by the library's own event pairs around
each kernel (nerftex_profile_enable; no host time), the chains in alternating windows of one process:
  * nerftex_curved_shape_infer over the imported mesh (neighbour search, shape lookup, the shared back half);
  * nerftex_curved_field_infer over the SAME mesh as the field's own (the path a field without an import takes: projector, hash-grid gather).
262 144 rows within +-0.1 of star_flower_mesh(72, 144) (20 k triangles), a 1024 x 1024 x 16 fp32 map, fp16 autocast.
    timeout 600 python tools/import_shape_timing.py > profiles/import_shape_timing.json"""
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
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch

    import nerftex_hip
    from ngp_harness.curved import CurvedField, star_flower_mesh, vertex_normals

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev, B, h = torch.device("cuda:0"), a.samples // 128 * 128, 0.0625
    v, f = star_flower_mesh()
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=h).to(dev).eval()
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
    gen = torch.Generator(device=dev).manual_seed(1)
    # per-vertex UVs from the sphere's angles (a seam at phi = 0: one column of long UV edges, as an unwrapped sphere has)
    r = np.linalg.norm(v, axis=-1)
    uvs = np.stack([np.arctan2(v[:, 2], v[:, 0]) / np.pi, 2 * np.arccos(np.clip(v[:, 1] / r, -1, 1)) / np.pi - 1], -1).astype(np.float32)
    rng = np.random.default_rng(2)
    pick = rng.integers(0, len(v), B)
    vn = vertex_normals(v, f).numpy()
    x = torch.from_numpy((v[pick] + vn[pick] * rng.uniform(-0.1, 0.1, (B, 1)) + rng.normal(0, 0.01, (B, 3))).astype(np.float32)).to(dev)
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=dev, generator=gen), dim=-1)

    def infer():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return field.infer(x, d)

    def windows():
        for _ in range(a.iters):
            infer()
        torch.cuda.synchronize()
        nerftex_hip.kernel_profile(True, reset=True)
        for _ in range(a.iters):
            infer()
        torch.cuda.synchronize()
        prof = nerftex_hip.kernel_profile()
        nerftex_hip.kernel_profile(False)
        runs = {k: p["avg_us"] for k, p in prof.items()}
        runs["chain_total"] = sum(p["total_us"] for p in prof.values()) / a.iters  # (the FFMLP kernel runs twice per call)
        return runs

    per = {"mesh_field": [], "shape_import": []}
    for w in range(a.windows):
        if field.features_imported is not None:
            field.switch_import()  # -> the mesh field
        assert not field.imported
        per["mesh_field"].append(windows())
        if field.features_imported is None:
            field.import_field(torch.rand(a.map, a.map, 16, device=dev, generator=gen) - 0.5, 1.0 / a.map)
            field.import_shape(v, f, uvs, normalize=False)
            field.set_sdf_factor(1.0)
        else:
            field.switch_import()
        assert field.imported and field.imported_type == "shape"
        per["shape_import"].append(windows())
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        mask = field._shape_lookup(x)[2]
    K = field._shape_scalars()[0]
    out = {"what": f"{B} rows within +-0.1 of star_flower_mesh(72, 144), a {a.map} x {a.map} x 16 fp32 map, fp16 autocast, eval; avg us per launch by the library's "
                   f"event pairs over {a.iters} calls, {a.windows} alternating windows, median (min .. max) per kernel; chain_total = all of a call's launches together",
           "share_of_rows_inside_the_mask": round(float(mask.float().mean()), 4), "K_for_uv": K, "K_mesh_field": int(field.projector.K)}
    for name, ws in per.items():
        out[name] = {k: [round(statistics.median(w[k] for w in ws), 2), round(min(w[k] for w in ws), 2), round(max(w[k] for w in ws), 2)] for k in ws[0]}
    out["shape_lookup_bytes_per_row"] = {"read": f"12 (x) + {8 * K} (the neighbour list) + {24 * K} (vertices and vertex normals, L2-resident) + the BVH walk + 48 (the hit's "
                                                 "triangle) + 24 (its UVs) + 4 x 64 (texels)", "written_rows_form": 1 + 12 + 96}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
