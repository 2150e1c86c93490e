"""TEST INFRASTRUCTURE: float64 restatements for the relighting tests (tests/test_envmap_cpu.py, tests/test_gpu_envmap.py).

  moments      the three sums the fit is a function of: G = sum Y Y^T [9,9], b = sum Y y^T [9,3], s = sum y^2 [3] over the map's pixels, with Y
               the nine svox2 bases AS THE FRAMEWORK EVALUATES THEM IN FP32 at SH2Envmap's fp32 directions (the reference's float64 run reads
               the same fp32 bases: svox2_eval_sh_bases allocates its result in the directions' dtype) and the products and sums in float64.
  adam_fit     EnvMap2SH's loop on the moments: gradient 2 / (3 H W) (G c - b), loss (c^T G c - 2 c^T b + s) / (3 H W) of the parameters before
               the update, torch's single-tensor Adam, the stopping rule; all float64.  tests/test_envmap_cpu.py holds it to the reference's own
               float64 run (1e-9), which shows that the Gram form walks the same trajectory as the loop over the map.
  fit_tolerance / relative_fit_tolerance
               the bound the fit is held to: 4 x max|ref_fp32 - ref_float64| over the coefficients of a fixture case -- the reference's own
               rounding sensitivity along this trajectory, x 4 because the kernel's rounding points differ from both runs -- or, where that gap
               is below 1e-6 of the largest coefficient, 1e-6 of that coefficient.
  probe_candidates / check_probe_shading
               the probe choice with its margin -- every probe whose float64 dot is within 1e-6 of the best: the reference's grid has coinciding
               directions, ties are the rule -- and the shading of the rows GROUPED BY PROBE through tests/sh_light_float64.py (its bounds and
               kink bands; the head is not restated here).  A row passes if it matches the model's shading for ANY of its candidates.
"""
import numpy as np
import sh_light_float64 as f64
import torch

MARGIN = 1e-6


def basis_fp32(H, W):
    """The fp32 bases SH2Envmap evaluates: [H W, 9] float64 holding fp32 values."""
    from ngp_harness.light import svox2_basis9

    phi, theta = torch.meshgrid([torch.linspace(0.0, np.pi, H), torch.linspace(-0.5 * np.pi, 1.5 * np.pi, W)], indexing="ij")
    dirs = torch.stack([torch.cos(theta) * torch.sin(phi), torch.cos(phi), torch.sin(theta) * torch.sin(phi)], dim=-1).reshape(-1, 3)
    assert dirs.dtype == torch.float32
    return svox2_basis9(dirs).double().numpy()


def moments(envmap):
    """envmap [H,W,3] -> G [9,9], b [9,3], s [3], float64."""
    envmap = np.asarray(envmap)
    H, W = envmap.shape[:2]
    Y = basis_fp32(H, W)
    y = envmap.reshape(-1, 3).astype(np.float64)
    return Y.T @ Y, Y.T @ y, (y * y).sum(0)


def adam_fit(G, b, s, n_pixels, n_sh=16, lr=1e-2, max_steps=5000, min_loss=1e-5, min_steps=2000, beta1=0.9, beta2=0.999, eps=1e-8):
    """-> (env_shs [n_sh,3], updates made, losses [updates])."""
    n = 3.0 * n_pixels
    c, m, v = np.zeros((9, 3)), np.zeros((9, 3)), np.zeros((9, 3))
    losses = []
    for step in range(max_steps):
        Gc = G @ c
        loss = float(((c * Gc).sum() - 2.0 * (c * b).sum() + s.sum()) / n)
        g = (2.0 / n) * (Gc - b)
        t = step + 1
        m = m + (g - m) * (1 - beta1)  # lerp_
        v = v * beta2 + (1 - beta2) * g * g
        step_size = lr / (1 - beta1 ** t)
        denom = np.sqrt(v) / (1 - beta2 ** t) ** 0.5 + eps
        c = c + (-step_size) * m / denom
        losses.append(loss)
        if loss < min_loss and step > min_steps:
            break
    out = np.zeros((n_sh, 3))
    out[:9] = c
    return out, len(losses), np.array(losses)


def fit_tolerance(ref_fp32, ref_fp64):
    gap = float(np.abs(np.asarray(ref_fp32, np.float64) - ref_fp64).max())
    floor = 1e-6 * float(np.abs(ref_fp64).max())
    return floor if gap < floor else 4.0 * gap


def relative_fit_tolerance(golden):
    """For maps the fixture holds no reference run of: the larger of the two cases' tolerances relative to their largest coefficient -- a seeded
    map may be of either kind, stopping early as A does or running to the end as B does."""
    return max(fit_tolerance(golden[f"fit_{c}_fp32"], golden[f"fit_{c}_fp64"]) / float(np.abs(golden[f"fit_{c}_fp64"]).max()) for c in "ab")


def probe_candidates(normals_secondary, probes, margin=MARGIN):
    """-> [B,K] bool: every probe whose dot with the row's secondary normal is within `margin` of the best."""
    dots = np.asarray(normals_secondary, np.float64) @ np.asarray(probes, np.float64).T
    return dots >= dots.max(-1, keepdims=True) - margin


KEYS = ("color", "specular", "diffuse", "albedo")


def check_probe_shading(name, outs, albedo_h, spec_w_h, normals, dirs, normals_secondary, probes, probe_shs, gamma=2.4, use_specular=True, mask=None,
                        extra=None, kink_cap=0.02):
    """outs: the four outputs [4,B,3].  Every row must lie inside sh_light_float64's bounds (+ `extra`, absolute, for a caller whose inputs
    carry an error of their own) of the shading under ONE of its candidate probes, elements in that model's kink bands excepted; the excepted
    share of the rows' first candidates stays under kink_cap.  -> the share of rows with a single candidate."""
    outs = np.asarray(outs, np.float64)
    B = outs.shape[1]
    cands = probe_candidates(normals_secondary, probes)
    live = np.ones(B, bool) if mask is None else np.asarray(mask, bool)
    assert not outs[:, ~live].any(), f"{name}: masked rows are exactly 0"
    passed = np.zeros(B, bool)
    worst = np.full(B, np.inf)
    kinks, first = 0, cands.argmax(-1)
    for k in np.nonzero(cands.any(0))[0]:
        rows = np.nonzero(cands[:, k])[0]
        ref = f64.shade(albedo_h[rows], spec_w_h[rows], normals[rows], dirs[rows], probe_shs[k], gamma, use_specular, live[rows])
        ratio = np.zeros(len(rows))
        for i, key in enumerate(KEYS):
            assert np.isfinite(ref[key]).all() and np.isfinite(ref["bound_" + key]).all(), (name, key)
            err = np.abs(outs[i][rows] - ref[key])
            bound = ref["bound_" + key] + (0.0 if extra is None or key == "albedo" else extra)
            r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
            r = np.where(ref["kink_" + key], 0.0, r)
            ratio = np.maximum(ratio, r.max(-1))
            kinks += int(ref["kink_" + key][first[rows] == k].sum())
        passed[rows] |= ratio <= 1.0
        worst[rows] = np.minimum(worst[rows], ratio)
    single = float((cands.sum(-1) == 1).mean())
    print(f"{name}: worst error / bound {float(worst.max()):.3f}, rows with one candidate {single:.2%}, elements in kink bands {kinks / (12.0 * B):.4%}")
    assert kinks / (12.0 * B) <= kink_cap, (name, kinks)
    assert passed.all(), (name, np.nonzero(~passed)[0][:8], float(worst.max()))
    return single
