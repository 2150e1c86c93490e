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
gradient into brdf[:, 4] is exactly zero.  Out of scope: imported environment maps, visibility probes, the SG and Envmap models.
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
    envs = env_shs[None]
    albedo = torch.sigmoid(brdf[..., :3])
    specular = torch.sigmoid(brdf[..., 3:4])
    glossiness = torch.nn.functional.softplus(brdf[..., 4:5]) + 1.0
    diffuse_rgb = irradiance(envs[:, :9, :3], normals).clamp(0)
    diffuse = albedo * diffuse_rgb
    if use_specular:
        rays_d = _normalize(view_dirs)
        cos_theta = -(rays_d * normals).sum(dim=-1, keepdim=True)
        reflect_d = _normalize(2 * cos_theta * normals + rays_d)
        order_coeff = torch.arange(0, envs.shape[0], device=envs.device)[:, None]  # (the [1, N, C] view's first dimension: arange(0, 1))
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

    def _fused(self, brdf, normals):
        return (self.fused and brdf.is_cuda and brdf.dtype == torch.float16 and normals.dtype == torch.float32 and torch.is_autocast_enabled()
                and torch.get_autocast_dtype("cuda") == torch.float16)

    def forward(self, geo_feat, normals, view_dirs, mask=None, gamma=None):
        prefix = geo_feat.shape[:-1]
        geo_feat, normals, view_dirs = geo_feat.reshape(-1, geo_feat.shape[-1]), normals.reshape(-1, 3), view_dirs.reshape(-1, 3)
        mask = None if mask is None else mask.reshape(-1)
        ones = torch.ones(geo_feat.shape[0], self.in_pad - self.input_dim, dtype=geo_feat.dtype, device=geo_feat.device)
        brdf = self.brdf_layer(torch.cat([geo_feat, ones], dim=-1))
        gamma = self.gamma if gamma is None else gamma
        if self._fused(brdf, normals):
            out = _SHLight.apply(brdf, normals, view_dirs, self.envSHs, mask, gamma, self.use_specular)
        else:
            out = sh_light_shade(brdf, normals, view_dirs, self.envSHs, self.use_specular, gamma, mask)
        return tuple(o.reshape(*prefix, 3) for o in out)
