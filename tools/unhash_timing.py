"""What rendering the field baked onto a finely subdivided mesh costs (CurvedField.unhash at the reference's default, min_vnum = 5e5), on
star_flower_mesh(72, 144) and 262 144 rows within +-0.1 of it, fp16 autocast, eval:
  * the host side once: the midpoint subdivision, the BVH build over the fine mesh, the bake (encoder over every fine vertex);
  * nerftex_curved_unhash_infer by the library's own event pairs around each kernel (nerftex_profile_enable; no host time), and the whole call
    by a host clock around calls that end in a device synchronise;
  * forward() op by op on the same rows (fused_glue off: `_unhash_embed_reference`, two full trace launches and ~40 framework launches in front of
    the networks), by the same host clock -- the comparison, not the code under test;
  * nerftex_curved_field_infer of the mesh field on the same rows, for scale.
The three routes run in alternating windows of one process.
    timeout 900 python tools/unhash_timing.py > profiles/unhash_timing.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-texture_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--min-vnum", type=float, default=5e5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch

    import nerftex_hip
    from ngp_harness.curved import CurvedField, star_flower_mesh, subdivide_until, vertex_normals
    from RayTracer import RayTracer

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev, B, h = torch.device("cuda:0"), a.samples // 128 * 128, 0.0625
    v, f = star_flower_mesh()
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=h).to(dev).eval()
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
    rng = np.random.default_rng(2)
    pick = rng.integers(0, len(v), B)
    vn = vertex_normals(v, f).numpy()
    x = torch.from_numpy((v[pick] + vn[pick] * rng.uniform(-0.1, 0.1, (B, 1)) + rng.normal(0, 0.01, (B, 3))).astype(np.float32)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=dev, generator=gen), dim=-1)

    # the host side, each piece once (the subdivision and the BVH build are single-threaded host code)
    t0 = time.perf_counter()
    fv, ff = subdivide_until(v, f, a.min_vnum)
    t1 = time.perf_counter()
    fv32 = np.ascontiguousarray(fv, np.float32)
    RayTracer(fv32, ff)  # (the build alone; unhash() below builds its own)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    field.unhash(mesh=(fv32, ff))
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    host = {"subdivide_until_s": round(t1 - t0, 3), "bvh_build_and_upload_s": round(t2 - t1, 3), "unhash_of_a_given_mesh_s": round(t3 - t2, 3),
            "fine_vertices": int(len(fv)), "fine_faces": int(len(ff))}

    def call(fused):
        field.fused_glue = fused
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            return field.infer(x, d)

    def wall(fused):
        """ms per call: a host clock around a.iters calls that end in a synchronise"""
        for _ in range(3):
            call(fused)
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(a.iters):
            call(fused)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / a.iters * 1e3

    def kernels():
        for _ in range(3):
            call(True)
        torch.cuda.synchronize()
        nerftex_hip.kernel_profile(True, reset=True)
        for _ in range(a.iters):
            call(True)
        torch.cuda.synchronize()
        prof = nerftex_hip.kernel_profile()
        nerftex_hip.kernel_profile(False)
        runs = {k: p["avg_us"] for k, p in prof.items()}
        runs["chain_total"] = sum(p["total_us"] for p in prof.values()) / a.iters  # (the FFMLP kernel runs twice per call)
        return runs

    per = {"mesh_field_kernels": [], "unhash_kernels": []}
    walls = {"mesh_field_infer_ms": [], "unhash_infer_ms": [], "unhash_forward_op_by_op_ms": []}
    for w in range(a.windows):
        field.switch_import()
        assert not field.imported
        per["mesh_field_kernels"].append(kernels())
        walls["mesh_field_infer_ms"].append(wall(True))
        field.switch_import()
        assert field.imported and field.imported_type == "unhash"
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            field.fused_glue = True
            assert field._infer_route(x, d)[0] == "nerftex_curved_unhash_infer"
            field.fused_glue = False
            assert field._infer_route(x, d) is None and not field._source_fused(x)
        per["unhash_kernels"].append(kernels())
        walls["unhash_infer_ms"].append(wall(True))
        walls["unhash_forward_op_by_op_ms"].append(wall(False))
    field.fused_glue = True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        mask = field._unhash_lookup(x)[1]
        s1, c1 = call(True)
        s0, c0 = call(False)
    agree = (s1 == 0) == (s0 == 0)
    out = {"what": f"{B} rows within +-0.1 of star_flower_mesh(72, 144); the fine mesh: midpoint subdivision until {a.min_vnum:.0f} vertices; fp16 autocast, eval; kernels: "
                   f"avg us per launch by the library's event pairs over {a.iters} calls; walls: ms per call by a host clock around {a.iters} calls ending in a "
                   f"synchronise; {a.windows} alternating windows, median (min .. max)",
           "host_once": host, "share_of_rows_inside_the_mask": round(float(mask.float().mean()), 4),
           "fused_against_op_by_op": {"masks_agree_on": round(float(agree.float().mean()), 5),
                                      "largest_sigma_difference_relative": round(float(((s1 - s0).abs() / (s0.abs() + 1e-3))[agree].max()), 5),
                                      "largest_colour_difference": round(float((c1 - c0).abs()[agree].max()), 5)}}
    for name, ws in per.items():
        out[name] = {k: [round(statistics.median(w[k] for w in ws), 2), round(min(w[k] for w in ws), 2), round(max(w[k] for w in ws), 2)] for k in ws[0]}
    for name, ws in walls.items():
        out[name] = [round(statistics.median(ws), 3), round(min(ws), 3), round(max(ws), 3)]
    out["vertex_lookup_bytes_per_row"] = {"read": "12 (x) + 64 (the neighbour list, K = 8) + 192 (vertices and vertex normals of the field's own mesh) + the BVH walk over "
                                                  "the fine mesh + 48 (the hit's triangle) + 12 (its corner ids) + 3 x 64 (feature rows)", "written_rows_form": 1 + 12 + 96}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
