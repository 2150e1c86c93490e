"""The SH light model of the curved field: nerf/sh_light_model.py's SH_EnvmapMaterialNet (:509-616), the head `main.py` trains
(`light_model = 'SH'`): a BRDF MLP on the geometry features, two sigmoids, the irradiance of an order-2 SH environment at the shading
normal (diffuse) and at the reflected view direction (specular), a clamp and the 1 / gamma tone map.

    net = SHLightNet(input_dim=15, sh_order=3, white_light=True, use_specular=True)
    color, specular, diffuse, albedo = net(geo_feat, normals, view_dirs, mask=None, gamma=None)

Two paths with the same arithmetic:
  fused        one HIP launch per direction (csrc/shlight.inc: nerftex_sh_light_forward / _backward) behind the BRDF MLP, taken on the
               GPU under fp16 autocast.  Only `color` carries a gradient (the other three outputs are what the reference's viewer shows
               in eval); the shading normal and the view direction receive none, as in the reference's training (`normal.detach()`,
               network_curvedfield.py:331; the direction's gradient is camera optimisation).
  op by op     `sh_light_shade`: the reference's framework ops restated one by one, on any device and dtype -- what `fused = False`,
               fp32 / bf16 runs and the CPU use, and what the tests compare the kernels against.

As the reference EXECUTES it (sh_light_model.py:594-597): `order_coeff` is built from the first dimension of the [1, N, C] view of
envSHs, i.e. arange(0, 1), so every band's glossiness attenuation is exp(0) = 1: the glossiness does not change the value and the
gradient into brdf[:, 4] is exactly zero.

Relighting (the reference's load_envmap :625, switch_envmap_import :675, the eval branch of forward :561-571):
  envmap_to_sh      EnvMap2SH (:730): SH coefficients fitted to an equirectangular [H, W, 3] map.  On the GPU one call of nerftex_envmap_fit
                    (csrc/envmap.inc: the map's moments in one launch, the whole Adam loop in one wave); `fused = False` or a CPU tensor runs the
                    reference's loop op by op with torch.optim.Adam.
  load_envmap       takes such a map, or fitted coefficients (the reference's .npy), and optionally the reference's _vis.npz tables: one
                    lighting per probe direction, chosen per sample by its coarse normal (`shade_visibility`); fused: nerftex_sh_light_probe_forward.
                    With visibility=True it computes those tables itself:
  envmap_probe_tables   load_envmap_with_visibility without a file (:653-665): the 8 x 8 probe grid (probe_grid), the clamped-cosine lobe rotated onto
                    every probe (visibility_lobes: rotate_coeff_by_normal, :228-282) and, per probe, fit_product_of_SHs (:692-709): 800 Adam steps on
                    1024 fresh sphere points each, WITHOUT zero_grad, as the reference executes it.  On the GPU one call of nerftex_envmap_vis_fit
                    (csrc/envmap_vis.inc: a workgroup per probe walks all rounds) with this library's own counter-based points; `fused = False` or a
                    CPU tensor runs the reference's loop op by op (fit_product_of_shs) with torch.rand.
  lighting()        the coefficients in effect: the imported ones in eval once switched on, envSHs otherwise.  Training never sees the import.
Out of scope: reading image files, the SG and Envmap models.  The reference's `euler` lighting rotation lives in front
of the head, on the field: CurvedField.set_light_rotation / forward(euler=) hand this module rotated vectors.
"""
import math

import torch
import torch.nn as nn

GAMMA = 2.4
# svox2's constants (sh_light_model.py:22-30)
_C0, _C1 = 0.28209479177387814, 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_LOBE = (3.14, 2.09, 2.09, 2.09, 0.79, 0.79, 0.79, 0.79, 0.79)  # render_irrandiance_sh_sum, divided by pi there


def svox2_basis9(dirs):
    """svox2_eval_sh_bases(9, dirs) (sh_light_model.py:52-76): [..., 3] -> [..., 9].  Not the tcnn ordering of the SH encoder."""
    x, y, z = dirs.unbind(-1)
    xx, yy, zz = x * x, y * y, z * z
    xy, yz, xz = x * y, y * z, x * z
    return torch.stack([torch.full_like(x, _C0), -_C1 * y, _C1 * z, -_C1 * x, _C2[0] * xy, _C2[1] * yz, _C2[2] * (2.0 * zz - xx - yy), _C2[3] * xz,
                        _C2[4] * (xx - yy)], dim=-1)


def irradiance(coeffs, dirs):
    """render_irrandiance_sh_sum (:498-506): coeffs [1 or B, >= 9, C], dirs [B, 3] -> [B, C]."""
    lobe = torch.tensor(_LOBE, dtype=torch.float32, device=dirs.device).type_as(dirs)[None, :] / math.pi
    coeffs = coeffs[:, :9, :] * lobe[:, :, None]
    return (coeffs * svox2_basis9(dirs)[..., None]).sum(dim=1)


def _normalize(t):
    return t / (t.norm(dim=-1, keepdim=True) + 1e-9)


def _safe_pow(x, p):
    base = torch.relu(torch.where(torch.abs(x - 0.0) <= 1e-6, torch.ones_like(x) * 1e-6, x))
    return torch.pow(base, p)


def sh_light_shade(brdf, normals, view_dirs, env_shs, use_specular=True, gamma=GAMMA, mask=None):
    """SH_EnvmapMaterialNet.forward behind the BRDF MLP (:579-616), op by op.  brdf [B, >= 5] (half under autocast: the sigmoids then are
    half tensors), normals / view_dirs [B, 3], env_shs [(order + 1)^2, C] -> (color, specular, diffuse, albedo), each [B, 3]; rows with
    mask == False are 0 in all four."""
    return _shade(brdf, normals, view_dirs, env_shs[None], use_specular, gamma, mask)


def _shade(brdf, normals, view_dirs, envs, use_specular, gamma, mask):
    """sh_light_shade behind its [1, N, C] view of the lighting; sh_light_shade_probes hands it one lighting per row, [B, N, C]."""
    albedo = torch.sigmoid(brdf[..., :3])
    specular = torch.sigmoid(brdf[..., 3:4])
    glossiness = torch.nn.functional.softplus(brdf[..., 4:5]) + 1.0
    diffuse_rgb = irradiance(envs[:, :9, :3], normals).clamp(0)
    diffuse = albedo * diffuse_rgb
    if use_specular:
        rays_d = _normalize(view_dirs)
        cos_theta = -(rays_d * normals).sum(dim=-1, keepdim=True)
        reflect_d = _normalize(2 * cos_theta * normals + rays_d)
        # (the [1, N, C] view's first dimension: arange(0, 1).  Under per-probe lighting the reference's view is [B, 9, 3] and its arange(0, B)
        # attenuates the specular lighting of row b by exp(-floor(sqrt(b))^2 / 2 / glossiness): the sample's position in its batch.  Not followed:
        # a row is lit as the first row of a batch is.)
        order_coeff = torch.arange(0, 1, device=envs.device)[:, None]
        order_coeff = torch.pow(order_coeff, 0.5).floor()
        sh_coeff = torch.exp(-order_coeff * order_coeff / 2 / glossiness.float())[..., None] * envs[:, :9, :3]
        specular = specular * irradiance(sh_coeff, reflect_d)
    else:
        specular = torch.zeros_like(diffuse)
    color = (diffuse + specular).clamp(0)
    diffuse = diffuse.clamp(0, 1)
    specular = specular.clamp(0, 1)
    if specular.shape[-1] == 1:
        specular = specular.expand_as(color)
    albedo = albedo.clamp(0, 1)
    out = (_safe_pow(color, 1 / gamma), _safe_pow(specular, 1 / gamma), _safe_pow(diffuse, 1 / gamma), albedo)
    if mask is not None:
        out = tuple(torch.where(mask.unsqueeze(-1), o, torch.zeros_like(o)) for o in out)
    return out


def sh_light_shade_probes(brdf, normals, view_dirs, normals_secondary, probes, probe_shs, use_specular=True, gamma=GAMMA, mask=None):
    """The head under per-probe imported lighting, op by op: the probe choice of sh_light_model.py:566-567 -- argmax over the [B, K] products of
    the secondary normal with the probe directions, the [B, 9, 3] gather -- and then sh_light_shade's arithmetic with one lighting per row."""
    prob_idx = (normals_secondary[:, None] * probes[None]).sum(dim=-1).argmax(dim=-1)
    return _shade(brdf, normals, view_dirs, probe_shs[prob_idx], use_specular, gamma, mask)


def sh_to_envmap(env_shs, H, W):
    """SH2Envmap (:712-727) op by op: [>= 9, C] coefficients -> the [H, W, C] equirectangular map (Mitsuba's convention) and its directions."""
    phi, theta = torch.meshgrid([torch.linspace(0.0, math.pi, H), torch.linspace(-0.5 * math.pi, 1.5 * math.pi, W)], indexing="ij")
    viewdirs = torch.stack([torch.cos(theta) * torch.sin(phi), torch.cos(phi), torch.sin(theta) * torch.sin(phi)], dim=-1)
    viewdirs = viewdirs.to(device=env_shs.device, dtype=env_shs.dtype).reshape(-1, 3)
    rgb = (env_shs[None, :9, :3] * svox2_basis9(viewdirs)[..., None]).sum(dim=1)
    return rgb.reshape(H, W, rgb.shape[-1]), viewdirs.reshape(H, W, 3)


def image_to_envmap(array, force_white=True):
    """image2envmap's arithmetic (:769-791) on an array ALREADY in [0, 1] (the reference divides the 8-bit image by 255): ** (1 / 1.24), then the
    channel mean in every channel under force_white.  It does not read files and does not do the reference's cv2 resize of images taller than
    200 rows: hand it the array at the size it is to be fitted at."""
    import numpy as np

    envmap = np.asarray(array)[..., :3] ** (1 / 1.24)
    if force_white:
        envmap[..., :] = envmap.mean(axis=-1, keepdims=True)
    return envmap


def _envmap_fit_reference(envmap, n_sh, min_loss, max_steps, min_steps, lr):
    """EnvMap2SH's loop (:738-760) op by op, without its logging."""
    H, W = envmap.shape[:2]
    env_shs = nn.Parameter(torch.zeros(n_sh, 3, dtype=envmap.dtype, device=envmap.device))
    optimizer = torch.optim.Adam([env_shs], lr=lr)
    steps, value = 0, float("nan")
    for step in range(max_steps):
        optimizer.zero_grad()
        env_map, _ = sh_to_envmap(env_shs, H, W)
        loss = torch.mean((env_map - envmap) * (env_map - envmap))
        loss.backward()
        optimizer.step()
        steps, value = step + 1, loss.item()
        if value < min_loss and step > min_steps:
            break
    return env_shs.detach(), {"steps": steps, "loss": value}


def envmap_to_sh(envmap, sh_order=3, *, min_loss=1e-5, max_steps=5000, min_steps=2000, lr=1e-2, fused=None):
    """EnvMap2SH (:730-766): envmap [H, W, 3] (array or tensor) -> (envSHs [(sh_order + 1)^2, 3] on the map's device, info) with info["steps"]
    the optimizer updates made and info["loss"] the loss of the last step (of the parameters before its update, as the reference prints it).
    A GPU tensor goes through nerftex_envmap_fit -- two launches, and one wait here for the two numbers of info; fused = False or a CPU tensor
    runs the reference's loop op by op."""
    envmap = torch.as_tensor(envmap)
    if envmap.dim() != 3 or envmap.shape[2] != 3 or envmap.shape[0] * envmap.shape[1] == 0:
        raise ValueError(f"envmap_to_sh: an [H, W, 3] map, but got {tuple(envmap.shape)}")
    if sh_order < 2:
        raise ValueError(f"envmap_to_sh: the map is fitted with the SH bands 0..2, sh_order must be at least 2 (got {sh_order})")
    n_sh = (sh_order + 1) ** 2
    if fused is None:
        fused = envmap.is_cuda
    if not fused:
        return _envmap_fit_reference(envmap if envmap.dtype == torch.float64 else envmap.float(), n_sh, min_loss, max_steps, min_steps, lr)
    if not envmap.is_cuda:
        raise RuntimeError("envmap_to_sh(fused=True) needs the map on the GPU: there is no fused CPU path")
    import ctypes

    from nerftex_hip import EnvmapFitDesc, check, lib, ptr, stream

    envmap = envmap.contiguous().float()
    H, W = envmap.shape[:2]
    dev = envmap.device
    phi, theta = torch.linspace(0.0, math.pi, H).to(dev), torch.linspace(-0.5 * math.pi, 1.5 * math.pi, W).to(dev)  # (as sh_to_envmap: made on the host)
    env_shs = torch.empty(n_sh, 3, dtype=torch.float32, device=dev)
    steps, loss = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    scratch = torch.empty(lib.nerftex_envmap_fit_scratch_bytes(H, W) // 8, dtype=torch.float64, device=dev)
    desc = EnvmapFitDesc(envmap=ptr(envmap), phi=ptr(phi), theta=ptr(theta), H=H, W=W, n_sh=n_sh, max_steps=int(max_steps), min_steps=int(min_steps),
                         lr=float(lr), min_loss=float(min_loss), env_shs=ptr(env_shs), steps_run=ptr(steps), final_loss=ptr(loss), scratch=ptr(scratch),
                         scratch_bytes=scratch.numel() * 8)
    check(lib.nerftex_envmap_fit(ctypes.byref(desc), stream()))
    return env_shs, {"steps": int(steps.item()), "loss": float(loss.item())}


_VIS_LOBE = (0.8754318, 0.0, 1.023545, 0.0, 0.0, 0.0, 0.449686, 0.0, 0.0)  # the clamped cosine about +z, bands 0..2 (:661)


def probe_grid(H=8, W=8):
    """The probe directions of load_envmap_with_visibility (:657-660), made as the reference makes them: [H W, 3] fp32 on the host.  As executed:
    both linspaces include their ends, so the last column repeats the first and the last row (polar angle pi) is W copies of the pole (0, -1, 0)
    up to sin(fp32 pi); the first row sits at pi / H, not on the other pole.  The probe head takes the lowest index among equal probes."""
    phi, theta = torch.meshgrid([torch.linspace(math.pi / H, math.pi, H), torch.linspace(-0.5 * math.pi, 1.5 * math.pi, W)], indexing="ij")
    return torch.stack([torch.cos(theta) * torch.sin(phi), torch.cos(phi), torch.sin(theta) * torch.sin(phi)], dim=-1).reshape([-1, 3])


def _band2_rotation(r1):
    """The band-2 SH rotation [B, 5, 5] from the band-1 rotation r1 [B, 3, 3] by the recursion of Ivanic and Ruedenberg as compute_band_rotation
    (:194-219) runs it for l = 2, rows and columns by centred indices -2..2.  With l = 2 the coefficient w is zero for every (m, n), so only the U
    and V terms exist."""
    def e(i, j):
        return r1[:, i + 1, j + 1]

    def P(i, a, b):  # (:131-142) with l = 2: the previous band is band 1 itself
        if b == 2:
            return e(i, 1) * e(a, 1) - e(i, -1) * e(a, -1)
        if b == -2:
            return e(i, 1) * e(a, -1) + e(i, -1) * e(a, 1)
        return e(i, 0) * e(a, b)

    out = torch.zeros(r1.shape[0], 5, 5, dtype=r1.dtype, device=r1.device)
    for m in range(-2, 3):
        for n in range(-2, 3):
            d = 1.0 if m == 0 else 0.0
            denom = 12.0 if abs(n) == 2 else (2 + n) * (2 - n)
            u = math.sqrt((2 + m) * (2 - m) / denom)
            v = 0.5 * math.sqrt((1 + d) * (abs(m) + 1.0) * (abs(m) + 2) / denom) * (1 - 2 * d)
            if u != 0.0:
                u = u * P(0, m, n)
            if m == 0:
                v = v * (P(1, 1, n) + P(-1, -1, n))
            elif m > 0:
                v = v * (P(1, m - 1, n) * math.sqrt(2.0 if m == 1 else 1.0) - P(-1, -m + 1, n) * (0.0 if m == 1 else 1.0))
            else:
                v = v * (P(1, m + 1, n) * (0.0 if m == -1 else 1.0) + P(-1, -m - 1, n) * math.sqrt(2.0 if m == -1 else 1.0))
            out[:, m + 2, n + 2] = u + v
    return out


def visibility_lobes(probes, lobe=None):
    """rotate_coeff_by_normal(2, probes, lobe) (:228-282) op by op: the order-2 lobe about +z ([9], default the reference's clamped cosine) rotated
    onto each of probes [K, 3] -> [K, 9].  The frame is x = normalize(n x z), y = n x x, columns (x, y, n); |n_z| > 0.999 takes the identity
    (n_z > 0) or diag(-1, 1, -1) (n_z < 0) instead, where n x z degenerates.  The band-1 matrix is read off the frame, band 2 comes from
    _band2_rotation.  Runs on the host: K x 9 numbers, computed once.  (The reference calls torch.cross without `dim`, which picks the FIRST
    dimension of size 3: for exactly three normals that is the wrong one.  It only ever passes 64; here the cross product is always per row.)"""
    n = torch.as_tensor(probes, dtype=torch.float32).detach().cpu()
    if n.dim() != 2 or n.shape[1] != 3:
        raise ValueError(f"visibility_lobes: probes is [K, 3], but got {tuple(n.shape)}")
    coeff = torch.tensor(_VIS_LOBE, dtype=torch.float32) if lobe is None else torch.as_tensor(lobe, dtype=torch.float32).detach().cpu().reshape(9)
    n = n / (n.norm(dim=1, keepdim=True) + 1e-9)
    z = torch.zeros_like(n)
    z[:, 2] = 1
    x = torch.linalg.cross(n, z, dim=1)
    x = x / (x.norm(dim=1, keepdim=True) + 1e-9)
    y = torch.linalg.cross(n, x, dim=1)
    R = torch.stack([x, y, n], dim=-1)
    R[n[:, 2] > 0.999] = torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 0, 1]])
    R[n[:, 2] < -0.999] = torch.tensor([[-1.0, 0, 0], [0, 1, 0], [0, 0, -1]])
    r1 = torch.stack([R[:, 1, 1], -R[:, 1, 2], R[:, 1, 0], -R[:, 2, 1], R[:, 2, 2], -R[:, 2, 0], R[:, 0, 1], -R[:, 0, 2], R[:, 0, 0]], dim=-1).reshape(-1, 3, 3)
    out = coeff[None, :].repeat(n.shape[0], 1)
    out[:, 1:4] = torch.bmm(r1, coeff[None, 1:4, None].repeat(n.shape[0], 1, 1))[:, :, 0]
    out[:, 4:9] = torch.bmm(_band2_rotation(r1), coeff[None, 4:9, None].repeat(n.shape[0], 1, 1))[:, :, 0]
    return out


def _eval_sh2(coeffs, dirs):
    """evaluate_spherical_harmonics(2, coeffs, dirs) (nerf/spherical_harmonics.py:64-105), term by term in its order: coeffs [..., C, 9],
    dirs [N, 3] -> [N, C].  The same polynomials and signs as svox2_basis9."""
    x, y, z = dirs[..., 0:1], dirs[..., 1:2], dirs[..., 2:3]
    result = _C0 * coeffs[..., 0]
    result = result - _C1 * y * coeffs[..., 1] + _C1 * z * coeffs[..., 2] - _C1 * x * coeffs[..., 3]
    xx, yy, zz = x * x, y * y, z * z
    xy, yz, xz = x * y, y * z, x * z
    return (result + _C2[0] * xy * coeffs[..., 4] + _C2[1] * yz * coeffs[..., 5] + _C2[2] * (2.0 * zz - xx - yy) * coeffs[..., 6]
            + _C2[3] * xz * coeffs[..., 7] + _C2[4] * (xx - yy) * coeffs[..., 8])


def sphere_points(u_phi, u_theta):
    """The points fit_product_of_SHs draws (:701-703) from two uniforms in [0, 1): [...] -> [..., 3]."""
    phi = 2 * math.pi * u_phi
    theta = torch.arccos(1 - 2 * u_theta)
    return torch.stack([torch.cos(phi) * torch.sin(theta), torch.sin(phi) * torch.sin(theta), torch.cos(theta)], dim=-1)


def fit_product_of_shs(sh1, sh2, *, rounds=800, batch=1024, lr=1e-3, points=None, generator=None):
    """fit_product_of_SHs (:692-709) op by op: sh1 [9, 3] (the lighting), sh2 [9] or [9, 3] (the lobe) -> [9, 3], the coefficients after `rounds`
    steps of torch.optim.Adam(lr) from sh1 towards the product of the two on `batch` points per step.  AS EXECUTED: no zero_grad(), so the
    gradient of step t is added to those of steps 1..t-1 and Adam sees the sum; the result is not converged and is defined by the trajectory.
    points [rounds, batch, 3] are used if given; otherwise each step calls torch.rand twice, phi first, as the reference (with `generator`)."""
    sh1 = sh1.detach()[None, :9]
    sh2 = sh2.detach().to(sh1)
    sh2 = (sh2[:, None].repeat(1, 3) if sh2.dim() == 1 else sh2)[None]
    sh = nn.Parameter(sh1.clone())
    optimizer = torch.optim.Adam([sh], lr=lr)
    for r in range(rounds):
        if points is None:
            u_phi = torch.rand([batch], device=sh.device, generator=generator)
            pts = sphere_points(u_phi, torch.rand([batch], device=sh.device, generator=generator)).to(sh.dtype)
        else:
            pts = points[r]
        with torch.enable_grad():  # (a caller that relights holds no_grad)
            gt = _eval_sh2(sh1.permute(0, 2, 1), pts) * _eval_sh2(sh2.permute(0, 2, 1), pts)
            pred = _eval_sh2(sh.permute(0, 2, 1), pts)
            loss = ((gt - pred) ** 2).sum(dim=-1).mean()
            loss.backward()
        optimizer.step()
    return sh.detach()[0]


def envmap_probe_tables(env_shs, probes=None, *, rounds=800, batch=1024, lr=1e-3, seed=0, points=None, points_out=False, fused=None):
    """load_envmap_with_visibility without a file (:653-665): env_shs [N >= 9, 3] -> (tables [K, 9, 3], probes [K, 3]) on env_shs' device, with
    probes = probe_grid() unless given (1 <= K <= 256); with points_out=True a third result, the points used [K, rounds, batch, 3].
    A GPU tensor goes through nerftex_envmap_vis_fit: one launch, no wait; its points come from the library's own counter-based stream keyed by
    (seed, probe, round, sample) -- not torch.rand's -- unless points [K, rounds, batch, 3] are given.  fused = False or a CPU tensor runs
    fit_product_of_shs per probe, drawing from torch.Generator().manual_seed(seed).  The two agree bit for bit on given points only as far as
    fp32 summation order allows (tests/test_gpu_probe_table.py), and on their own points statistically."""
    env_shs = torch.as_tensor(env_shs).detach()
    if env_shs.dim() != 2 or env_shs.shape[0] < 9 or env_shs.shape[1] != 3:
        raise ValueError(f"envmap_probe_tables: env_shs is [N >= 9, 3], but got {tuple(env_shs.shape)}")
    dev = env_shs.device
    probes = probe_grid() if probes is None else torch.as_tensor(probes).detach()
    K = probes.shape[0] if probes.dim() == 2 else 0
    if tuple(probes.shape) != (K, 3) or not 1 <= K <= 256:
        raise ValueError(f"envmap_probe_tables: probes is [K, 3] with 1 <= K <= 256, but got {tuple(probes.shape)}")
    rounds, batch = int(rounds), int(batch)
    if rounds < 1 or batch < 1 or not (lr > 0 and math.isfinite(lr)):
        raise ValueError(f"envmap_probe_tables: rounds and batch are positive and lr is positive and finite, but got {rounds}, {batch}, {lr}")
    if points is not None and tuple(points.shape) != (K, rounds, batch, 3):
        raise ValueError(f"envmap_probe_tables: points is [K, rounds, batch, 3] = {(K, rounds, batch, 3)}, but got {tuple(points.shape)}")
    lobes = visibility_lobes(probes)
    probes = probes.to(device=dev, dtype=torch.float32).contiguous()
    if fused is None:
        fused = env_shs.is_cuda
    if not fused:
        env = env_shs if env_shs.dtype == torch.float64 else env_shs.float()
        lobes = lobes.to(env)
        gen = None if points is not None else torch.Generator(device=dev).manual_seed(int(seed))
        used = torch.empty(K, rounds, batch, 3, dtype=env.dtype, device=dev) if points_out and points is None else points
        tables = torch.empty(K, 9, 3, dtype=env.dtype, device=dev)
        for i in range(K):
            if points is None and points_out:
                for r in range(rounds):
                    u_phi = torch.rand([batch], device=dev, generator=gen)
                    used[i, r] = sphere_points(u_phi, torch.rand([batch], device=dev, generator=gen))
            tables[i] = fit_product_of_shs(env, lobes[i], rounds=rounds, batch=batch, lr=lr, points=None if used is None else used[i].to(env),
                                           generator=gen)
        return (tables, probes, used) if points_out else (tables, probes)
    if not env_shs.is_cuda:
        raise RuntimeError("envmap_probe_tables(fused=True) needs the lighting on the GPU: there is no fused CPU path")
    import ctypes

    from nerftex_hip import EnvmapVisFitDesc, check, lib, ptr, stream

    env = env_shs.contiguous().float()
    lobes = lobes.to(dev).contiguous()
    if points is not None:
        points = points.detach().to(device=dev, dtype=torch.float32).contiguous()
    used = torch.empty(K, rounds, batch, 3, dtype=torch.float32, device=dev) if points_out else None
    tables = torch.empty(K, 9, 3, dtype=torch.float32, device=dev)
    desc = EnvmapVisFitDesc(env_shs=ptr(env), n_sh=env.shape[0], lobes=ptr(lobes), K=K, rounds=rounds, batch=batch, lr=float(lr),
                            seed=int(seed) & 0xFFFFFFFFFFFFFFFF, points=ptr(points), points_out=ptr(used), tables=ptr(tables))
    check(lib.nerftex_envmap_vis_fit(ctypes.byref(desc), stream()))
    return (tables, probes, used) if points_out else (tables, probes)


class _SHLight(torch.autograd.Function):
    """brdf [B, 5] half (rows of the BRDF MLP's 16-wide output), normals, dirs [B, 3] fp32, envSHs -> the four outputs [B, 3] fp32: one launch;
    the backward recomputes the forward from the inputs (nerftex_sh_light_backward) and sums the lighting gradient in a fixed order."""

    @staticmethod
    def forward(ctx, brdf, normals, dirs, env_shs, mask, gamma, use_specular):
        import ctypes

        from nerftex_hip import SH_LIGHT_SPECULAR, SHLightDesc, check, lib, ptr, stream

        assert brdf.dtype == torch.float16 and brdf.dim() == 2 and brdf.shape[1] >= 5
        if brdf.stride(1) != 1 or brdf.stride(0) < 5:
            brdf = brdf.contiguous()
        normals, dirs, env = normals.contiguous().float(), dirs.contiguous().float(), env_shs.detach().contiguous().float()
        mask_b = None if mask is None else mask.contiguous().view(torch.uint8)
        B = brdf.shape[0]
        out = torch.empty(4, B, 3, dtype=torch.float32, device=brdf.device)
        desc = SHLightDesc(brdf=ptr(brdf), brdf_stride=int(brdf.stride(0)) if B else 16, normals=ptr(normals), dirs=ptr(dirs), env_shs=ptr(env), n_sh=env.shape[0],
                           n_color=env.shape[1], mask=ptr(mask_b), B=B, gamma=float(gamma), flags=SH_LIGHT_SPECULAR if use_specular else 0,
                           color=ptr(out[0]), specular=ptr(out[1]), diffuse=ptr(out[2]), albedo=ptr(out[3]))
        check(lib.nerftex_sh_light_forward(ctypes.byref(desc), stream()))
        ctx.save_for_backward(brdf, normals, dirs, env, mask_b)
        ctx.conf = (float(gamma), bool(use_specular))
        color, specular, diffuse, albedo = out.unbind(0)  # (bound once: autograd matches the marked outputs by object)
        ctx.mark_non_differentiable(specular, diffuse, albedo)
        ctx.set_materialize_grads(False)
        return color, specular, diffuse, albedo

    @staticmethod
    def backward(ctx, g_color, *_):
        import ctypes

        from nerftex_hip import SH_LIGHT_SPECULAR, SHLightDesc, check, lib, ptr, stream

        if g_color is None:
            return (None,) * 7
        brdf, normals, dirs, env, mask_b = ctx.saved_tensors
        gamma, use_specular = ctx.conf
        B, stride = brdf.shape[0], int(brdf.stride(0)) if brdf.shape[0] else 16
        g_color = g_color.contiguous().float()
        g_brdf = torch.empty(B, stride, dtype=torch.float16, device=brdf.device)
        g_env = torch.empty_like(env)
        scratch = torch.empty(lib.nerftex_sh_light_scratch_bytes(B), dtype=torch.uint8, device=brdf.device)
        desc = SHLightDesc(brdf=ptr(brdf), brdf_stride=stride, normals=ptr(normals), dirs=ptr(dirs), env_shs=ptr(env), n_sh=env.shape[0], n_color=env.shape[1],
                           mask=ptr(mask_b), B=B, gamma=gamma, flags=SH_LIGHT_SPECULAR if use_specular else 0, grad_color=ptr(g_color), grad_brdf=ptr(g_brdf),
                           grad_env_shs=ptr(g_env), scratch=ptr(scratch), scratch_bytes=scratch.numel())
        check(lib.nerftex_sh_light_backward(ctypes.byref(desc), stream()))
        return g_brdf[:, :brdf.shape[1]], None, None, g_env, None, None, None


def _shade_probes_fused(brdf, normals, dirs, normals_secondary, probes, probe_shs, mask, gamma, use_specular):
    """nerftex_sh_light_probe_forward: one launch, no gradient (imported lighting is eval only)."""
    import ctypes

    from nerftex_hip import SH_LIGHT_SPECULAR, SHLightProbeDesc, check, lib, ptr, stream

    brdf = brdf.detach()
    if brdf.stride(1) != 1 or brdf.stride(0) < 5:
        brdf = brdf.contiguous()
    normals, dirs, n2 = normals.detach().contiguous().float(), dirs.detach().contiguous().float(), normals_secondary.detach().contiguous().float()
    probes, tables = probes.contiguous().float(), probe_shs.contiguous().float()
    mask_b = None if mask is None else mask.contiguous().view(torch.uint8)
    B = brdf.shape[0]
    out = torch.empty(4, B, 3, dtype=torch.float32, device=brdf.device)
    desc = SHLightProbeDesc(brdf=ptr(brdf), brdf_stride=int(brdf.stride(0)) if B else 16, normals=ptr(normals), dirs=ptr(dirs), normals_secondary=ptr(n2),
                            probes=ptr(probes), probe_shs=ptr(tables), K=probes.shape[0], mask=ptr(mask_b), B=B, gamma=float(gamma),
                            flags=SH_LIGHT_SPECULAR if use_specular else 0, color=ptr(out[0]), specular=ptr(out[1]), diffuse=ptr(out[2]), albedo=ptr(out[3]))
    check(lib.nerftex_sh_light_probe_forward(ctypes.byref(desc), stream()))
    return out.unbind(0)


class SHLightNet(nn.Module):
    """SH_EnvmapMaterialNet (sh_light_model.py:509-552): envSHs zeros with row 0 = 3; sh_pow_num / sh_s under the reference's names, shapes
    and dtypes so that its state_dict loads -- the reference never reads them (its fast_sh_sum is commented out as buggy, :506) and neither
    does this module, so they are buffers; brdf_layer = FFMLP(16 -> 64 x 3 -> 5) on the input padded with ones, as tcnn pads."""

    def __init__(self, input_dim=15, sh_order=3, white_light=True, use_specular=True):
        super().__init__()
        from ffmlp import FFMLP

        if sh_order < 2:
            raise ValueError(f"SHLightNet: the irradiance reads the SH bands 0..2, sh_order must be at least 2 (got {sh_order})")
        self.input_dim, self.sh_order, self.white_light, self.use_specular = input_dim, sh_order, white_light, use_specular
        init_light = torch.zeros((sh_order + 1) ** 2, 1 if white_light else 3)
        init_light[0, :] = 3  # a white ambient light
        self.envSHs = nn.Parameter(init_light)
        self.register_buffer("sh_pow_num", torch.zeros(20, 3, dtype=torch.int64))
        self.register_buffer("sh_s", torch.zeros(16, 20, dtype=torch.float32))
        self.gamma = GAMMA
        self.in_pad = (input_dim + 15) // 16 * 16
        self.brdf_layer = FFMLP(input_dim=self.in_pad, output_dim=5, hidden_dim=64, num_layers=3)  # albedo[3], specular[1], glossiness[1]
        self.fused = True
        # imported lighting under the reference's names (:546-548, :652): not part of the checkpoint, as there
        self.import_envmap = False
        for name in ("envSHs_import", "envSHs_import_vis", "probes"):
            self.register_buffer(name, None, persistent=False)

    def load_envmap(self, envmap=None, *, env_shs=None, env_shs_vis=None, probes=None, force_white=True, visibility=False, seed=0, vis_fit=None):
        """load_envmap (:625-645) without the files: an [H, W, 3] array in [0, 1] that is tone-mapped (image_to_envmap) and fitted (envmap_to_sh),
        or fitted coefficients env_shs [N >= 9, 3] (the reference's .npy); optionally the contents of its _vis.npz, env_shs_vis [K, 9, 3] and
        probes [K, 3], 1 <= K <= 256 -- or visibility=True, which computes the tables from the lighting just fitted or handed in, as the reference
        does when it finds no _vis.npz (load_envmap_with_visibility(seed); vis_fit: keyword overrides for envmap_probe_tables, such as rounds and
        batch).  visibility=False without tables leaves them None: forward() then raises under shade_visibility.  Switches the imported lighting
        on and returns True; ValueError for shapes that do not match and for visibility=True together with given tables."""
        dev = self.envSHs.device
        if visibility and (env_shs_vis is not None or probes is not None):
            raise ValueError("SHLightNet.load_envmap: visibility=True computes the probe tables; it does not go together with env_shs_vis= / probes=")
        if (envmap is None) == (env_shs is None):
            raise ValueError("SHLightNet.load_envmap: give either an [H, W, 3] map or fitted coefficients env_shs [N, 3]")
        if (env_shs_vis is None) != (probes is None):
            raise ValueError("SHLightNet.load_envmap: env_shs_vis [K, 9, 3] and probes [K, 3] come together")
        if env_shs_vis is not None:
            env_shs_vis = torch.as_tensor(env_shs_vis).detach().to(device=dev, dtype=torch.float32)
            probes = torch.as_tensor(probes).detach().to(device=dev, dtype=torch.float32)
            K = probes.shape[0] if probes.dim() == 2 else 0
            if tuple(probes.shape) != (K, 3) or tuple(env_shs_vis.shape) != (K, 9, 3) or not 1 <= K <= 256:
                raise ValueError(f"SHLightNet.load_envmap: probes [K, 3] and env_shs_vis [K, 9, 3] with 1 <= K <= 256, but got {tuple(probes.shape)} "
                                 f"and {tuple(env_shs_vis.shape)}")
        if envmap is not None:
            envmap = torch.as_tensor(envmap)
            if envmap.dim() != 3 or envmap.shape[2] != 3 or envmap.shape[0] * envmap.shape[1] == 0:
                raise ValueError(f"SHLightNet.load_envmap: an [H, W, 3] map, but got {tuple(envmap.shape)}")
            tone = torch.from_numpy(image_to_envmap(envmap.detach().cpu().numpy().copy(), force_white=force_white))
            env_shs, _ = envmap_to_sh(tone.to(device=dev, dtype=torch.float32), sh_order=self.sh_order)
        else:
            env_shs = torch.as_tensor(env_shs).detach().to(device=dev, dtype=torch.float32)
            if env_shs.dim() != 2 or env_shs.shape[0] < 9 or env_shs.shape[1] != 3:
                raise ValueError(f"SHLightNet.load_envmap: env_shs is [N >= 9, 3], but got {tuple(env_shs.shape)}")
        self.envSHs_import = env_shs.contiguous().clone()
        self.envSHs_import_vis = None if env_shs_vis is None else env_shs_vis.contiguous().clone()
        self.probes = None if probes is None else probes.contiguous().clone()
        if visibility:
            self.load_envmap_with_visibility(seed=seed, **(vis_fit or {}))
        self.import_envmap = True
        return True

    def load_envmap_with_visibility(self, seed=0, **fit):
        """load_envmap_with_visibility's branch without a file (:653-665): computes envSHs_import_vis [64, 9, 3] and probes [64, 3] for the lighting
        already imported (envmap_probe_tables; `fit`: its keywords).  RuntimeError if none is imported.  Returns True."""
        if self.envSHs_import is None:
            raise RuntimeError("SHLightNet.load_envmap_with_visibility: no lighting is imported: call load_envmap first")
        tables, probes = envmap_probe_tables(self.envSHs_import, seed=seed, **fit)[:2]
        self.envSHs_import_vis, self.probes = tables.float().contiguous(), probes.contiguous()
        return True

    def probe_tables(self):
        """{"envSHs": [K, 9, 3], "probes": [K, 3]} as numpy: exactly the content of the reference's _vis.npz (:666), for np.savez.  RuntimeError
        without tables."""
        if self.envSHs_import_vis is None or self.probes is None:
            raise RuntimeError("SHLightNet.probe_tables: no probe tables are loaded or computed")
        return {"envSHs": self.envSHs_import_vis.detach().cpu().numpy(), "probes": self.probes.detach().cpu().numpy()}

    def switch_envmap_import(self):
        """switch_envmap_import (:675-681): toggles the imported lighting and returns the new state; False while nothing is loaded."""
        self.import_envmap = False if self.envSHs_import is None else not self.import_envmap
        return self.import_envmap

    def _imported(self):
        return bool(self.import_envmap) and not self.training and self.envSHs_import is not None

    def lighting(self):
        """The coefficients in effect (:561-571): envSHs_import in eval with the import switched on, envSHs otherwise."""
        return self.envSHs_import if self._imported() else self.envSHs

    def probe_lighting(self, shade_visibility=True):
        """Whether a forward with this shade_visibility lights every sample by its probe: eval, imported lighting, the tables loaded."""
        return bool(shade_visibility) and self._imported() and self.envSHs_import_vis is not None

    def _fused(self, brdf, normals):
        return (self.fused and brdf.is_cuda and brdf.dtype == torch.float16 and normals.dtype == torch.float32 and torch.is_autocast_enabled()
                and torch.get_autocast_dtype("cuda") == torch.float16)

    def forward(self, geo_feat, normals, view_dirs, mask=None, gamma=None, normal_secondary=None, shade_visibility=False):
        probe = self.probe_lighting(shade_visibility)
        if shade_visibility and self._imported() and not probe:
            raise RuntimeError("SHLightNet: shade_visibility asks for one imported lighting per visibility probe, but no probe tables are loaded: "
                               "give them to load_envmap(env_shs_vis=, probes=), compute them with load_envmap(visibility=True), or set field.shade_visibility = False to light every sample "
                               "with envSHs_import")
        if probe and normal_secondary is None:
            raise ValueError("SHLightNet: shade_visibility needs normal_secondary, the normal the probe is chosen by")
        prefix = geo_feat.shape[:-1]
        geo_feat, normals, view_dirs = geo_feat.reshape(-1, geo_feat.shape[-1]), normals.reshape(-1, 3), view_dirs.reshape(-1, 3)
        mask = None if mask is None else mask.reshape(-1)
        ones = torch.ones(geo_feat.shape[0], self.in_pad - self.input_dim, dtype=geo_feat.dtype, device=geo_feat.device)
        brdf = self.brdf_layer(torch.cat([geo_feat, ones], dim=-1))
        gamma = self.gamma if gamma is None else gamma
        if probe:
            n2 = normal_secondary.reshape(-1, 3)
            if self._fused(brdf, normals):
                out = _shade_probes_fused(brdf, normals, view_dirs, n2, self.probes, self.envSHs_import_vis, mask, gamma, self.use_specular)
            else:
                out = sh_light_shade_probes(brdf, normals, view_dirs, n2, self.probes, self.envSHs_import_vis, self.use_specular, gamma, mask)
        elif self._fused(brdf, normals):
            out = _SHLight.apply(brdf, normals, view_dirs, self.lighting(), mask, gamma, self.use_specular)
        else:
            out = sh_light_shade(brdf, normals, view_dirs, self.lighting(), self.use_specular, gamma, mask)
        return tuple(o.reshape(*prefix, 3) for o in out)
