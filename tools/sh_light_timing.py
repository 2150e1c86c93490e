"""What the SH light head costs behind its BRDF MLP at 262 144 samples (fp16 autocast): the fused kernels (nerftex_sh_light_forward /
_backward through ngp_harness.light._SHLight) against the op-by-op sequence they replace (ngp_harness.light.sh_light_shade, the
reference's framework ops and torch autograd) -- the baseline; both from the same half BRDF rows [B, 5] of a 16-wide MLP output, the same
normals, directions, mask and lighting.  Per form: the forward alone (no_grad) and forward + backward (d loss / d color given), `--iters`
calls between two device events, `--reps` windows, the two forms alternating; medians and the spread.
    timeout 300 python tools/sh_light_timing.py > profiles/sh_light_timing.json"""
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--colors", type=int, default=1, help="1: white light (the reference's default), 3: coloured")
    a = ap.parse_args()
    import torch

    from ngp_harness.light import _SHLight, sh_light_shade

    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev, B = torch.device("cuda:0"), a.samples
    g = torch.Generator(device=dev).manual_seed(0)
    wide = (torch.randn(B, 16, device=dev, generator=g) * 2).half()
    n = torch.nn.functional.normalize(torch.randn(B, 3, device=dev, generator=g), dim=-1)
    d = torch.nn.functional.normalize(torch.randn(B, 3, device=dev, generator=g), dim=-1)
    mask = torch.rand(B, device=dev, generator=g) < 0.7
    gc = torch.randn(B, 3, device=dev, generator=g)
    env = torch.zeros(16, a.colors, device=dev)
    env[0] = 3
    env[1:] = torch.randn(15, a.colors, device=dev, generator=g) * 0.1

    def run(form, backward):
        brdf = wide[:, :5].detach().requires_grad_(backward)
        e = env.detach().requires_grad_(backward)
        with torch.autocast("cuda", dtype=torch.float16), torch.set_grad_enabled(backward):
            if form == "fused":
                color = _SHLight.apply(brdf, n, d, e, mask, 2.4, True)[0]
            else:
                color = sh_light_shade(brdf, n, d, e, True, 2.4, mask)[0]
            if backward:
                color.backward(gc)
        return color

    # the two forms compute the same thing at this size (the tests hold them to float64; here: a plain look)
    diff = float((run("fused", False) - run("ops", False)).abs().max())
    times = {f"{form}_{'fwd_bwd' if bw else 'fwd'}": [] for form in ("fused", "ops") for bw in (False, True)}
    for form in ("fused", "ops"):
        for bw in (False, True):
            for _ in range(10):
                run(form, bw)
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for bw in (False, True):
            for form in ("fused", "ops"):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    run(form, bw)
                t1.record()
                torch.cuda.synchronize()
                times[f"{form}_{'fwd_bwd' if bw else 'fwd'}"].append(t0.elapsed_time(t1) * 1e3 / a.iters)
    out = {"what": f"SH light head behind the BRDF MLP, {B} samples, {a.colors} colour(s), specular on, 70 % of the rows inside the mask, fp16 autocast; us per call "
                   f"between device events around {a.iters} eager calls (host launch time included for both forms), {a.reps} alternating windows",
           "max_abs_colour_difference_between_forms": diff,
           "median_us": {k: round(statistics.median(v), 2) for k, v in times.items()},
           "min_max_us": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}}
    out["ops_over_fused"] = {k: round(out["median_us"]["ops_" + k] / out["median_us"]["fused_" + k], 2) for k in ("fwd", "fwd_bwd")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
