"""What synthesizing a planar texture costs (ngp_harness.synthesis.synthesize_texture) at the size of the reference's own script: 128-pixel patches of
33 channels (16 features, 8 phi_embed, 9 local_tbn), a 2048 x 2048 output (25 x 25 cells of patch 32 + overlap 48), no mirrors, strict_match; P = 200
random patches and, with --large, P = 2000.  Two kinds of figures, taken in separate runs of the same call:
  * end to end: one warm-up call, then the median (min .. max) of --runs calls, a host clock around the call (it ends in a device synchronise and
    includes the upload of the patches, the build of the coarse databases and the read-back of the log);
  * per launch: the library's own event pairs around every launch (nerftex_hip.kernel_profile) in further calls -- per kernel the median over those
    calls of the mean time of a launch -- and the bytes the distance launch reads per interior cell (both databases once, the float64 query once per
    example), with its share of the HBM peak on those bytes.
--reference-cpu times the reference's own class (patch_matching_and_quilting.py, run as tools/make_golden.py runs it for the fixture: block_reduce
stubbed, no snapshots) on the SAME seeded inputs on the CPU of the machine at hand.  The reference is not on the GPU machine, so the two figures come
from different hosts; they are written into two files.
    timeout 900 python tools/synthesis_timing.py --large > profiles/synthesis_timing.json
    python tools/synthesis_timing.py --reference-cpu > profiles/synthesis_timing_reference_cpu.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s
S, FEATURES, PHI, OUTPUT, GRID_GAP = 128, 16, 8, 2048, 1.0 / 512


def inputs(P, seed=0):
    import numpy as np

    rng = np.random.default_rng(seed)
    C = FEATURES + PHI + 9
    patches = rng.random((P, S, S, C), dtype=np.float32) - np.float32(0.5)
    sample_tbn = (np.eye(3, dtype=np.float32).reshape(9) + rng.normal(0, 0.3, (P, 9))).astype(np.float32)
    picked = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    return patches, sample_tbn, picked


def reference_cpu(P):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import contextlib
    import io

    import make_golden as mg

    patches, sample_tbn, picked = inputs(P)
    case = dict(P=P, S=S, match_dim=FEATURES, phi_dim=PHI, max_patch_res=32, mirrors=False, output=OUTPUT, patch_length=S * GRID_GAP, seed=0)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        r = mg.run_reference_synthesis(case, patches, sample_tbn, picked)
    seconds = time.perf_counter() - t0
    print(json.dumps({"what": f"the reference's patchBasedTextureSynthesis (float64, sklearn KDTree, Python dynamic program) on the CPU of the build machine: P = {P}, "
                              f"S = {S}, C = {FEATURES + PHI + 9}, output {OUTPUT}, no mirrors; construction and resolveAll, one run, snapshots off",
                      "seconds": round(seconds, 1), "cells": int(r["id_map"].size), "canvas": list(r["canvas"].shape), "cpus": os.cpu_count()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--patches", type=int, default=200)
    ap.add_argument("--large", action="store_true", help="P = 2000 as well")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reference-cpu", action="store_true")
    a = ap.parse_args()
    if a.reference_cpu:
        return reference_cpu(a.patches)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-texture_amd")]
    import torch

    import nerftex_hip
    from ngp_harness.synthesis import synthesize_texture

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    out = {"what": f"synthesize_texture: S = {S}, C = {FEATURES + PHI + 9} (match_dim {FEATURES}), output {OUTPUT}, no mirrors, strict_match, max_patch_res 32; random "
                   f"patches (seeded; P = 200: the inputs of --reference-cpu); one warm-up call, then {a.runs} calls",
           "hbm_peak_GBs": HBM_PEAK_GBS}
    for P in [a.patches] + ([2000] if a.large else []):
        if P == a.patches:
            patches, sample_tbn, picked = (torch.from_numpy(x).to(dev) for x in inputs(P))
        else:  # (generated on the device: 4.3 GB)
            g = torch.Generator(device=dev).manual_seed(1)
            patches = torch.rand(P, S, S, FEATURES + PHI + 9, device=dev, generator=g) - 0.5
            sample_tbn = torch.eye(3, device=dev).reshape(1, 9) + 0.3 * torch.randn(P, 9, device=dev, generator=g)
            picked = torch.rand(P, 3, device=dev, generator=g) * 2 - 1
        result = {"patches": patches[..., :FEATURES], "patch_phi_embed": patches[..., FEATURES:FEATURES + PHI], "patch_local_tbn": patches[..., FEATURES + PHI:],
                  "grid_gap": GRID_GAP, "patch_sample_tbn": sample_tbn, "picked_vertices": picked}

        def call():
            texture, log = synthesize_texture(result, OUTPUT, seed=0)
            torch.cuda.synchronize()
            return log

        log = call()
        cells, strip = log["cells_per_side"] ** 2, log["strip_floats"]
        ms = []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        nerftex_hip.kernel_profile(True, reset=True)
        per = {}
        for _ in range(a.runs):
            nerftex_hip.kernel_profile(reset=True)
            call()
            for name, rec in nerftex_hip.kernel_profile().items():
                if name.startswith("synth_"):
                    per.setdefault(name, []).append((rec["avg_us"], rec["calls"]))
        nerftex_hip.kernel_profile(False)
        launches = {name: {"median_us": round(statistics.median(v[0] for v in rows), 2), "launches_per_call": rows[0][1]} for name, rows in per.items()}
        # an interior cell's distance launch: both fp32 databases once, and per example the float64 query of both strips (L2-resident after the first)
        padded = (strip + 3) // 4 * 4
        db_bytes = 2 * P * padded * 4
        dist_us = launches.get("synth_distance_kernel", {}).get("median_us")
        res = {"cells": cells, "canvas_side": int(log["canvas_id"].shape[0]), "examples": log["examples"], "coarse_values_per_strip": strip,
               "end_to_end_ms": [round(statistics.median(ms), 1), round(min(ms), 1), round(max(ms), 1)], "launches": launches,
               "distance_database_bytes_per_interior_cell": db_bytes,
               "note": "the distance launch's median is over all cells; first-row and first-column cells (49 of 624) read one database"}
        if dist_us:
            gbs = db_bytes / (dist_us * 1e-6) / 1e9
            res["distance_GBs_on_database_bytes"] = round(gbs, 1)
            res["distance_share_of_hbm_peak"] = round(gbs / HBM_PEAK_GBS, 3)
        out[f"P{P}"] = res
        del patches, result
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
