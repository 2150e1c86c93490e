#!/usr/bin/env python3
"""Generate tests/golden/ref_python_envmap.npz FROM THE REFERENCE ITSELF: nerf/sh_light_model.py imported at run time with the stand-ins of
tools/make_golden.py (tinycudann, `.cuda()` = identity, cv2 / imageio / tools.shape_tools stubbed) and run on the CPU.  Needs the reference
checkout (NERFTEX_REFERENCE); it never runs where the GPU tests run.  No reference text is stored in this repository.

  fit case A   a 16 x 32 map that IS an order-2 SH function with positive values: EnvMap2SH stops at its first opportunity, step 2001
  fit case B   a 13 x 29 map of seeded noise plus a bright patch, not representable: EnvMap2SH runs all 5000 steps
      per case: the map, EnvMap2SH's own result (fp32), the same loop with the parameters and the map cast to double (SH2Envmap called
      as EnvMap2SH calls it), the number of optimizer updates and the last loss of each, and the fp32 loss at step 2001.
      Asserted while generating: A's fp32 loss at step 2001 < 1e-6 (a decade under min_loss: both precisions stop at the same step),
      B's final loss > 1e-3 (both run to the end).
  probe case   300 rows of seeded geometry features, normals, view directions and secondary normals; the reference's 8 x 8 probe grid
      (:658-660); seeded [64, 9, 3] tables; SH_EnvmapMaterialNet.forward in eval with import_envmap set:
        probe_rows_*    shade_visibility on, ONE ROW PER CALL.  The reference builds its specular band attenuation from the first dimension of
                        the lighting it shades with (:594): [1, N, C] everywhere else, but [B, 9, 3] behind the per-probe gather, so row b of a
                        batch has its specular lighting scaled by exp(-floor(sqrt(b))^2 / 2 / glossiness) -- the sample's position in its
                        batch.  A row shaded as the first of its batch is free of that; these are what the tests compare with.
        probe_batch_*   the same 300 rows in one call, as the renderer calls it: stored to document the above (diffuse and albedo agree with
                        probe_rows_*, specular and colour agree in row 0 only).
        uniform_*       shade_visibility off with a seeded [16, 3] envSHs_import.
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (sets dont_write_bytecode; nothing runs on import)
import numpy as np  # noqa: E402


def _fit_loop(ref_sh, torch, envmap, dtype, n_sh=16):
    """EnvMap2SH's loop (:738-760) around the reference's own SH2Envmap, at `dtype`; -> coefficients, updates made, losses per step."""
    gt = torch.from_numpy(envmap).to(dtype)
    H, W = gt.shape[:2]
    env = torch.nn.Parameter(torch.zeros(n_sh, 3, dtype=dtype))
    opt = torch.optim.Adam([env], lr=1e-2)
    losses = []
    for step in range(5000):
        opt.zero_grad()
        env_map, _ = ref_sh.SH2Envmap(env, H=H, W=W, upper_hemi=False, clamp=False)
        loss = torch.mean((env_map - gt) * (env_map - gt))
        loss.backward()
        opt.step()
        losses.append(loss.item())
        if loss.item() < 1e-5 and step > 2000:
            break
    return env.detach().numpy().copy(), len(losses), np.array(losses, np.float64)


def main():
    import torch

    mg._install_map_imports()
    for name in ("imageio", "tools.shape_tools"):
        mg._stub(name, write_ply_rgb=None)
    sys.modules.pop("nerf.sh_light_model", None)
    import nerf.sh_light_model as ref_sh

    steps_seen = []

    def counting(it):
        for i in it:
            steps_seen.append(i)
            yield i

    ref_sh.tqdm = counting
    ref_sh.save_envmap = lambda *a, **k: None  # (images and .ply of the log: not the computation)
    real_save, ref_print = np.save, print
    out = {}

    # ---- the two fit cases
    # A's DC term of 5: Adam walks about lr = 1e-2 per step, so the fit arrives around step 1500 and at step 2001 its loss is ~2e-9 -- two
    # decades under 1e-6, and still far above the rounding floor.  (A DC term of 2.5 arrives by step 600; by step 2001 its loss is 1e-12, the
    # gradients 1e-13 and the second-moment estimate has decayed so far that the update amplifies the last bits: two float64 runs of that
    # case differ by 1e-4, and no restatement could be held to anything.)  Asserted below: fp32 and float64 agree to 1e-5.
    rng = np.random.default_rng(2026)
    coeff = np.zeros((16, 3), np.float32)
    coeff[0] = 5.0
    coeff[1:9] = rng.normal(0, 0.4, (8, 3)).astype(np.float32)
    with torch.no_grad():
        map_a = ref_sh.SH2Envmap(torch.from_numpy(coeff), H=16, W=32)[0].numpy().copy()
    assert map_a.min() > 0.0, map_a.min()
    rng = np.random.default_rng(7)
    map_b = rng.uniform(0.0, 0.6, (13, 29, 3)).astype(np.float32)
    map_b[2:5, 6:11] += 4.0  # the bright patch
    for case, envmap in (("a", map_a), ("b", map_b)):
        del steps_seen[:]
        with tempfile.TemporaryDirectory() as tmp:
            np.save = lambda *a, **k: None
            ref_sh.print = lambda *a, **k: None
            try:
                got = ref_sh.EnvMap2SH(envmap, sh_order=3, log_path=os.path.join(tmp, "log"), min_loss=1e-5, sv_path=os.path.join(tmp, "sh"))
            finally:
                np.save = real_save
                del ref_sh.print
        fp32 = got.detach().numpy().copy()
        steps32 = steps_seen[-1] + 1
        again, steps_again, losses32 = _fit_loop(ref_sh, torch, envmap, torch.float32)
        assert np.array_equal(again, fp32) and steps_again == steps32, "the restated loop is EnvMap2SH's"
        fp64, steps64, losses64 = _fit_loop(ref_sh, torch, envmap, torch.float64)
        if case == "a":
            assert losses32[2001] < 1e-6 and losses64[2001] < 1e-6 and steps32 == steps64 == 2002, (losses32[2001], losses64[2001], steps32, steps64)
            assert np.abs(fp64[:9] - coeff[:9]).max() < 1e-2 and np.abs(fp32 - fp64).max() < 1e-5
        else:
            assert losses32[-1] > 1e-3 and losses64[-1] > 1e-3 and steps32 == steps64 == 5000, (losses32[-1], losses64[-1], steps32, steps64)
        assert not fp32[9:].any() and not fp64[9:].any()
        out.update({f"fit_{case}_envmap": envmap, f"fit_{case}_fp32": fp32, f"fit_{case}_fp64": fp64, f"fit_{case}_steps_fp32": np.int64(steps32),
                    f"fit_{case}_steps_fp64": np.int64(steps64), f"fit_{case}_loss_fp32": np.float64(losses32[-1]), f"fit_{case}_loss_fp64": np.float64(losses64[-1]),
                    f"fit_{case}_loss2001_fp32": np.float64(losses32[2001]), f"fit_{case}_loss2001_fp64": np.float64(losses64[2001])})
        ref_print(f"fit {case}: steps {steps32} / {steps64}, loss[2001] {losses32[2001]:.3e}, final loss {losses32[-1]:.6e} / {losses64[-1]:.6e}, "
                  f"max|fp32 - fp64| {np.abs(fp32 - fp64).max():.3e}, max|coefficient| {np.abs(fp64).max():.3f}")
    out["fit_a_coefficients"] = coeff

    # ---- the probe-shading case
    B = 300
    rng = np.random.default_rng(91)
    net = ref_sh.SH_EnvmapMaterialNet(input_dim=15, sh_order=3, white_light=True, use_specular=True)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)  # noqa: E731
    geo = torch.from_numpy(rng.normal(0, 1.0, (B, 15)).astype(np.float32)).half()
    n = torch.from_numpy(unit(rng.normal(size=(B, 3))).astype(np.float32))
    d = torch.from_numpy((unit(rng.normal(size=(B, 3))) * rng.uniform(0.5, 2.0, (B, 1))).astype(np.float32))
    n2 = rng.normal(size=(B, 3))
    n2 = torch.from_numpy((n2 / (np.linalg.norm(n2, axis=-1, keepdims=True) + 1e-5)).astype(np.float32))
    H = W = 8
    phi, theta = torch.meshgrid([torch.linspace(np.pi / H, np.pi, H), torch.linspace(-0.5 * np.pi, 1.5 * np.pi, W)], indexing="ij")  # (:658-660)
    probes = torch.stack([torch.cos(theta) * torch.sin(phi), torch.cos(phi), torch.sin(theta) * torch.sin(phi)], dim=-1).reshape([-1, 3])
    tables = np.zeros((64, 9, 3), np.float32)
    tables[:, 0] = rng.uniform(1.0, 3.0, (64, 3))
    tables[:, 1:] = rng.normal(0, 0.3, (64, 8, 3))
    uniform = np.zeros((16, 3), np.float32)
    uniform[0] = rng.uniform(1.0, 3.0, 3)
    uniform[1:] = rng.normal(0, 0.3, (15, 3))
    net.envSHs_import = torch.nn.Parameter(torch.from_numpy(uniform), requires_grad=False)
    net.sh_order_import = 3
    net.envSHs_import_vis = torch.nn.Parameter(torch.from_numpy(tables), requires_grad=False)
    net.probes = torch.nn.Parameter(probes, requires_grad=False)
    net.sh_order_import_vis = 2
    net.import_envmap = True
    net.eval()
    seen = {}
    handle = net.brdf_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("brdf", o))
    names = ("color", "specular", "diffuse", "albedo")
    with torch.no_grad(), mg.emulated_autocast():
        batch = net(geo, n, d, shade_visibility=True, normal_secondary=n2)
        brdf = seen["brdf"].detach().numpy().copy()
        rows = [net(geo[b:b + 1], n[b:b + 1], d[b:b + 1], shade_visibility=True, normal_secondary=n2[b:b + 1]) for b in range(B)]
        flat = net(geo, n, d, shade_visibility=False)
    handle.remove()
    assert brdf.dtype == np.float16 and brdf.shape == (B, 5)
    for i, name in enumerate(names):
        out[f"probe_batch_{name}"] = batch[i].float().numpy()
        out[f"probe_rows_{name}"] = torch.cat([r[i] for r in rows]).float().numpy()
        out[f"uniform_{name}"] = flat[i].float().numpy()
    # (a call of one row and a call of 300 round the framework's vectorised sums differently in the last place: 1e-6, not equality)
    for name in ("diffuse", "albedo"):
        assert np.abs(out[f"probe_batch_{name}"] - out[f"probe_rows_{name}"]).max() < 1e-6, name
    moved = np.abs(out["probe_batch_color"] - out["probe_rows_color"]).max(-1)
    assert moved[0] < 1e-6 and (moved > 1e-3).sum() > B // 2, "the position in the batch enters the specular term of every row but the first"
    ref_print("probe case: rows whose colour depends on their position in the batch by more than 1e-3:", int((moved > 1e-3).sum()), "of", B, "max", moved.max())
    out.update({"probe_geo_feat": geo.numpy(), "probe_normals": n.numpy(), "probe_dirs": d.numpy(), "probe_normals_secondary": n2.numpy(),
                "probe_w_brdf": net.brdf_layer.net.weights.detach().numpy().copy(), "probe_brdf": brdf, "probes": probes.numpy(), "probe_shs": tables,
                "uniform_env_shs": uniform, "gamma": np.float64(net.gamma)})
    np.savez_compressed(os.path.join(mg.OUT, "ref_python_envmap.npz"), **out)
    ref_print("wrote ref_python_envmap.npz,", os.path.getsize(os.path.join(mg.OUT, "ref_python_envmap.npz")), "bytes")


if __name__ == "__main__":
    main()
