"""What rendering an imported feature patch costs (CurvedField.import_patch): a 128 x 128 patch (what export_field produces by default), 262 144
samples near it, fp16 autocast, eval.  Per figure: one warm-up call, then the median (min .. max) of five calls, each timed by an event pair
around the call on the stream (device time of everything the call enqueues; the op-by-op route's includes the gaps between its ~60 launches):
  * the fused chain, CurvedField.infer -> nerftex_curved_patch_infer (static) and nerftex_curved_light_patch_infer (SH-lit);
  * the op-by-op route, forward() over CurvedField._patch_embed_reference (the library's neighbour search, framework ops behind it);
  * the plain lookups alone (nerftex_patch_lookup, nerftex_patch_light_lookup).
The parent commit has no path that renders a patch: there is nothing to compare these figures with.
    timeout 600 python tools/import_patch_timing.py > profiles/import_patch_timing.json"""
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
    ap.add_argument("--patch", type=int, default=128, help="edge of the square patch in points")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch

    from ngp_harness.curved import CurvedField, star_flower_mesh

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev, B, h, S = torch.device("cuda:0"), a.samples // 128 * 128, 0.0625, a.patch
    gap = 1.0 / S  # the patch spans [-0.5, 0.5]^2
    rng = np.random.default_rng(3)
    c = (np.arange(S) - (S - 1) / 2) * gap
    gx, gy = np.meshgrid(c, c, indexing="ij")
    points = np.stack([gx, gy, 0.2 * (gx * gx - gy * gy)], -1).reshape(-1, 3).astype(np.float32)
    patch = dict(features=rng.uniform(-0.5, 0.5, (S * S, 16)).astype(np.float32), points=points, normals=np.float32([0, 0, 1]))
    lit_arrays = dict(phi_embed=rng.uniform(-0.5, 0.5, (S * S, 8)).astype(np.float32),
                      local_tbn=(np.eye(3, dtype=np.float32).reshape(9) + rng.normal(0, 0.35, (S * S, 9))).astype(np.float32))
    # samples: above and below seeded points by up to 1.3 h, a third of a gap to the side
    pick = rng.integers(0, S * S, B)
    x = torch.from_numpy((points[pick] + np.float32([0, 0, 1]) * rng.uniform(-1.3, 1.3, (B, 1)) * h + rng.normal(0, gap / 3, (B, 3)) * np.float32([1, 1, 0])).astype(np.float32)).to(dev)
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1)), dim=-1)
    v, f = star_flower_mesh(n_lat=18, n_lon=36)

    def timed(call):
        call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            call()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1) * 1e3)
        return [round(statistics.median(ms), 1), round(min(ms), 1), round(max(ms), 1)]

    out = {"what": f"{B} samples near a {S} x {S} patch on z = 0.2 (x^2 - y^2), h_threshold {h}, fp16 autocast, eval; us per call, one warm-up then median (min .. max) "
                   f"of {a.runs} calls, an event pair around each call",
           "parent_commit": "no path renders a patch: nothing to compare with"}
    for lit in (False, True):
        torch.manual_seed(0)
        field = CurvedField(v, f, bound=1.0, h_threshold=h, light_model="SH" if lit else None).to(dev).eval()
        field.import_patch(**patch, **(lit_arrays if lit else {}))
        field.fused_light_infer = lit
        key = "lit" if lit else "static"

        def infer():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return field.infer(x, d)

        def op_by_op():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                embed = field._patch_embed_reference(x, with_fine_normal=lit)
                return embed

        def forward_op_by_op():
            field.fused_glue = False  # (the static field's switch: forward() then goes through the op-by-op route)
            try:
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    assert not field._patch_fused(x)
                    return field(x, d)
            finally:
                field.fused_glue = True

        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._infer_route(x, d)[0] == ("nerftex_curved_light_patch_infer" if lit else "nerftex_curved_patch_infer")
            mask = field._patch_lookup(x)[1]
        res = {"share_of_rows_inside_the_mask": round(float(mask.float().mean()), 4)}
        res["fused_chain"] = timed(infer)
        res["plain_lookup"] = timed(lambda: field._patch_lookup(x, lit=lit))
        res["op_by_op_embed"] = timed(op_by_op)
        if not lit:
            res["op_by_op_forward"] = timed(forward_op_by_op)
        out[key] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
