"""TEST INFRASTRUCTURE: a float64 restatement of the SH light head behind its two sigmoids (steps 2-5 of nerf/sh_light_model.py:583-616 and
their gradients) with a per-element bound on the fp32 error, for tests/test_sh_light_cpu.py and tests/test_gpu_sh_light.py.  Plain numpy.

It STARTS FROM THE HALF-VALUED albedo / spec_w (`half_sigmoid`): the sigmoid's rounding point is pinned bit for bit by the GPU tests, so no
double rounding enters here.

    irr(v)_c   = sum_{k<9} env[k, c] lobe_k Y_k(v),   lobe = [3.14, 2.09 x 3, 0.79 x 5] / pi,  Y = the svox2 basis
    diffuse_c  = albedo_c max(irr(n)_c', 0)                                       (c' = c, or 0 under white light)
    spec_c'    = spec_w irr(w)_c',  w = normalize(2 cos n + r), r = d / (|d| + 1e-9), cos = -(r . n)        (0 without specular)
    color_c    = safe_pow(max(diffuse_c + spec_c', 0), 1 / gamma),   safe_pow(x, p) = pow(relu(where(|x| <= 1e-6, 1e-6, x)), p)
    specular / diffuse out = safe_pow(clamp(., 0, 1), 1 / gamma),  albedo out = clamp(albedo, 0, 1)
    gs_c       = grad_color_c p x^(p-1) where diffuse_c + spec_c' > 1e-6, else 0
    d albedo_c = gs_c max(irr(n)_c', 0),   d spec_w = sum_c' (sum_{c -> c'} gs_c) irr(w)_c'
    grad_brdf  = the fp16 sigmoid backward (half(g) (1 - y)) y of those two, column 4 = 0
    grad_env[k, c'] = lobe_k sum_b ( [irr(n)_c' >= 0] (sum_{c -> c'} gs_c albedo_c) Y_k(n) + spec_w (sum_{c -> c'} gs_c) Y_k(w) )

THE ERROR MODEL: u = 2^-24 (half an fp32 ulp, relative), every rounding of the fp32 evaluation enters once at its worst case, first order,
as  c u sum|terms|  with the sums of magnitudes formed here in float64 and c counted from the operations:
  basis        Y_k: the constant's rounding, at most two products and, for k = 6 (2zz - xx - yy) and k = 8 (xx - yy), the squares' roundings
               and one or two subtractions: |dY_k| <= 5 u absY_k with absY_6 = C (2zz + xx + yy), absY_8 = C (xx + yy), absY_k = |Y_k| else.
  coefficient  env_k lobe_k: 3.14f, pi's fp32 value, their quotient (or the product with its reciprocal) and the product with env: 4 u.
  irradiance   9 products (u each) and 8 additions whatever their order (u sum|terms| each at most): 18 u S, S = sum_k |env_k| lobe_k absY_k --
               plus, at the reflected direction, the basis' derivative times the direction's own error:
  direction    r: squares, two additions, the square root (correctly rounded on the CPU, the device library's within 1 ulp = 2 u), + 1e-9, the
               quotient: 6 u |r_c|.  cos: 6 u + 3 u on sum_c |r_c n_c|.  w0 = 2 cos n + r: 2 |n_c| |dcos| + u |2 cos n_c| + |dr_c| + u |w0_c|;
               w = w0 / (|w0| + 1e-9): (|dw0_c| + |w_c| sum_j |w_j| |dw0_j|) / |w0| + 6 u |w_c|.
  products     albedo x clamp, spec_w x irr, their sum: u on each result.
  pow          OpenCL C 3.0 specification, section 7.4 "Relative Error as ULPs" (the table the ROCm device library's float functions are
               built to; the framework's CPU pow is tighter): pow <= 16 ulp, one ulp <= 2 u |value|; plus the exponent's own rounding to
               fp32, u p |ln x| relative (x >= 1e-6: |ln x| <= 13.9).  The backward's p x^(p-1): 16 ulp, the exponent p - 1 (u |p - 1| |ln x|),
               p's rounding, two products: (35 + |p - 1| |ln x|) u relative, plus the derivative p |p - 1| x^(p-2) times x's error.
  grad_brdf    the fp32 gradient's error carried through (1 - y) y, plus FOUR half roundings (relative 2^-11 each, and 2^-25 absolute for a
               result in the subnormal range): the cast of the fp32 gradient to half, and the three operations of the fp16 sigmoid backward.
  grad_env     per sample the products' errors; the sum over B: the kernels add at most ceil(B / 262144) values per thread, 6 butterfly
               levels, 4 waves, at most 16 partials per lane and 6 more butterfly levels -- under 40 additions in a chain for B <= 2^22; the
               framework's reductions are shallower: 40 u sum_b |term_b|.  Then the lobe: 4 u.

KINK BANDS: where the float64 value in front of a clamp or of safe_pow's threshold lies within its own bound of the kink, fp32 may take the
other branch; such elements are flagged (`kink_*`) and excluded from value comparisons by the tests, which cap the excluded share.
"""
import numpy as np

U = 2.0 ** -24
UH = 2.0 ** -11
POW_ULP = 16
C0, C1 = 0.28209479177387814, 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
LOBE = np.array([3.14, 2.09, 2.09, 2.09, 0.79, 0.79, 0.79, 0.79, 0.79]) / np.pi


def half_sigmoid(x_half):
    """The head's starting point: sigmoid evaluated in float64 from the half inputs and rounded ONCE to half (what an fp32 sigmoid narrowed
    to half gives except within an fp32 error of a half rounding boundary -- the GPU test pins that point against torch.sigmoid itself)."""
    x = np.asarray(x_half, np.float16).astype(np.float64)
    return (1.0 / (1.0 + np.exp(-x))).astype(np.float16)


def basis9(v):
    """-> Y [B,9], absY [B,9], J [B,9,3] = dY/dv."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    o, zero = np.ones_like(x), np.zeros_like(x)
    Y = np.stack([C0 * o, -C1 * y, C1 * z, -C1 * x, C2[0] * x * y, C2[1] * y * z, C2[2] * (2 * z * z - x * x - y * y), C2[3] * x * z, C2[4] * (x * x - y * y)], -1)
    absY = np.abs(Y)
    absY[:, 6] = abs(C2[2]) * (2 * z * z + x * x + y * y)
    absY[:, 8] = abs(C2[4]) * (x * x + y * y)
    J = np.stack([np.stack([zero, zero, zero], -1), np.stack([zero, -C1 * o, zero], -1), np.stack([zero, zero, C1 * o], -1), np.stack([-C1 * o, zero, zero], -1),
                  np.stack([C2[0] * y, C2[0] * x, zero], -1), np.stack([zero, C2[1] * z, C2[1] * y], -1),
                  np.stack([-2 * C2[2] * x, -2 * C2[2] * y, 4 * C2[2] * z], -1), np.stack([C2[3] * z, zero, C2[3] * x], -1),
                  np.stack([2 * C2[4] * x, -2 * C2[4] * y, zero], -1)], 1)
    return Y, absY, J


def _irradiance(env, v, dv):
    """-> irr [B,C], its bound [B,C], Y, dY [B,9] (the basis' own error bound, direction error included)."""
    Y, absY, J = basis9(v)
    el = env[:9] * LOBE[:, None]                                        # [9,C]
    dY_dir = (np.abs(J) * dv[:, None, :]).sum(-1)                       # [B,9]
    irr = Y @ el
    S = absY @ np.abs(el)
    bound = 18 * U * S + dY_dir @ np.abs(el)
    return irr, bound, Y, 5 * U * absY + dY_dir


def reflect(n, d):
    """-> w [B,3] and the bound on its fp32 error per component."""
    L = np.linalg.norm(d, axis=-1, keepdims=True)
    r = d / (L + 1e-9)
    dr = 6 * U * np.abs(r)
    A = (np.abs(r) * np.abs(n)).sum(-1, keepdims=True)
    cos = -(r * n).sum(-1, keepdims=True)
    dcos = 9 * U * A
    w0 = 2 * cos * n + r
    dw0 = 2 * np.abs(n) * dcos + U * np.abs(2 * cos * n) + dr + U * np.abs(w0)
    L0 = np.linalg.norm(w0, axis=-1, keepdims=True)
    w = w0 / (L0 + 1e-9)
    dw = (dw0 + np.abs(w) * (np.abs(w) * dw0).sum(-1, keepdims=True)) / np.maximum(L0, 1e-30) + 6 * U * np.abs(w)
    return w, dw


def _tone(x, dx, p, lo_hi):
    """safe_pow(clamp(x), p) with bound and kink flag; x the value in front of the clamp, dx its bound; lo_hi = (0, None) or (0, 1)."""
    kink = (np.abs(x) <= dx) & (dx > 0)
    c = np.maximum(x, 0.0)
    if lo_hi[1] is not None:
        kink |= (np.abs(x - lo_hi[1]) <= dx) & (dx > 0)
        c = np.minimum(c, lo_hi[1])
    kink |= (np.abs(x - 1e-6) <= dx + U * 1e-6) & (dx > 0)                  # (x, not its clamp: a firmly negative x is exactly 0 behind it)
    base = np.where(np.abs(c) <= 1e-6, 1e-6, c)
    val = base ** p
    passes = (x > 1e-6) if lo_hi[1] is None else ((x > 1e-6) & (x < 1.0))
    bound = np.where(passes, p * base ** (p - 1) * dx, 0.0) + (2 * POW_ULP + p * np.abs(np.log(base))) * U * val
    return val, bound, kink, base, passes


def shade(albedo_h, spec_w_h, normals, dirs, env_shs, gamma=2.4, use_specular=True, mask=None, grad_color=None):
    """albedo_h [B,3], spec_w_h [B,1]: the half sigmoids; normals, dirs [B,3] fp32; env_shs [n_sh, C] fp32.  -> dict of float64 arrays:
    color / specular / diffuse / albedo [B,3], bound_* and kink_* of each; with grad_color [B,3] also g_albedo_h [B,3] / g_spec_w_h [B,1] (the
    half sigmoid backward's results: compare with grad_brdf[:, :3] / [:, 3:4]) with bound_g_* and kink_g (per row), grad_env [n_sh, C] and
    bound_grad_env.  Masked rows: zeros everywhere, no contribution."""
    a = np.asarray(albedo_h, np.float16).astype(np.float64)
    sw = np.asarray(spec_w_h, np.float16).astype(np.float64).reshape(-1, 1)
    n, d, env = np.asarray(normals, np.float64), np.asarray(dirs, np.float64), np.asarray(env_shs, np.float64)
    B, C = a.shape[0], env.shape[1]
    cmap = np.arange(3) if C == 3 else np.zeros(3, int)
    p = 1.0 / gamma
    live = np.ones(B, bool) if mask is None else np.asarray(mask, bool)
    irr, dirr, Yn, dYn = _irradiance(env, n, np.zeros_like(n))
    kink_irr = np.abs(irr) <= dirr                                       # [B,C]: the clamp on diffuse_rgb
    drgb = np.maximum(irr, 0.0)
    diffuse = a * drgb[:, cmap]
    ddrgb = np.where(irr < -dirr, 0.0, dirr)                             # (firmly negative: exactly 0 behind the clamp in fp32 too)
    ddiffuse = a * ddrgb[:, cmap] + U * np.abs(diffuse)
    if use_specular:
        w, dw = reflect(n, d)
        srgb, dsrgb, Yw, dYw = _irradiance(env, w, dw)
        spec = sw * srgb
        dspec = sw * dsrgb + U * np.abs(spec)
    else:
        srgb, dsrgb, Yw, dYw = np.zeros((B, C)), np.zeros((B, C)), np.zeros((B, 9)), np.zeros((B, 9))
        spec, dspec = np.zeros((B, C)), np.zeros((B, C))
    total = diffuse + spec[:, cmap]
    dtotal = ddiffuse + dspec[:, cmap] + U * np.abs(total)
    out = {}
    color, bcolor, kcolor, base, passes = _tone(total, dtotal, p, (0, None))
    out["color"], out["bound_color"], out["kink_color"] = color, bcolor, kcolor | kink_irr[:, cmap]
    v, b, k, _, _ = _tone(diffuse, ddiffuse, p, (0, 1))
    out["diffuse"], out["bound_diffuse"], out["kink_diffuse"] = v, b, k | kink_irr[:, cmap]
    v, b, k, _, _ = _tone(spec[:, cmap], dspec[:, cmap], p, (0, 1))
    out["specular"], out["bound_specular"], out["kink_specular"] = v, b, k
    out["albedo"], out["bound_albedo"], out["kink_albedo"] = np.clip(a, 0, 1), np.zeros_like(a), np.zeros(a.shape, bool)
    for key in ("color", "diffuse", "specular", "albedo"):
        out[key] = np.where(live[:, None], out[key], 0.0)
        out["bound_" + key] = np.where(live[:, None], out["bound_" + key], 0.0)
        out["kink_" + key] = out["kink_" + key] & live[:, None]
    if grad_color is None:
        return out
    g = np.asarray(grad_color, np.float64) * live[:, None]
    lnx = np.abs(np.log(base))
    q = p * base ** (p - 1)
    gs = np.where(passes, g * q, 0.0)
    dgs = np.where(passes, np.abs(g) * p * abs(p - 1) * base ** (p - 2) * dtotal + (2 * POW_ULP + 3 + abs(p - 1) * lnx) * U * np.abs(gs), 0.0)
    kink_row = (kcolor | kink_irr[:, cmap]).any(-1) & live
    # albedo: fp32 gradient, then cast to half + the fp16 sigmoid backward (4 half roundings)
    ga = gs * drgb[:, cmap]
    dga = drgb[:, cmap] * dgs + np.abs(gs) * np.where(irr[:, cmap] > 0, dirr[:, cmap], 0.0) + U * np.abs(ga)
    out["g_albedo_h"] = ga * (1 - a) * a
    out["bound_g_albedo_h"] = dga * (1 - a) * a + 4 * (UH * np.abs(out["g_albedo_h"]) + 2.0 ** -25)
    gspec = np.zeros((B, C))
    dgspec = np.zeros((B, C))
    agspec = np.zeros((B, C))
    np.add.at(gspec.T, cmap, gs.T), np.add.at(dgspec.T, cmap, dgs.T), np.add.at(agspec.T, cmap, np.abs(gs).T)
    dgspec += 2 * U * agspec
    gsw = (gspec * srgb).sum(-1, keepdims=True)
    dgsw = (dgspec * np.abs(srgb) + np.abs(gspec) * dsrgb + (1 + C) * U * np.abs(gspec * srgb)).sum(-1, keepdims=True)
    out["g_spec_w_h"] = gsw * (1 - sw) * sw
    out["bound_g_spec_w_h"] = dgsw * (1 - sw) * sw + 4 * (UH * np.abs(out["g_spec_w_h"]) + 2.0 ** -25)
    out["kink_g"] = kink_row
    # lighting: per sample  g_irr_c' Y_k(n) + g_srgb_c' Y_k(w)
    ga_c = gs * a
    girr, dgirr, agirr = np.zeros((B, C)), np.zeros((B, C)), np.zeros((B, C))
    np.add.at(girr.T, cmap, ga_c.T), np.add.at(dgirr.T, cmap, (a * dgs + U * np.abs(ga_c)).T), np.add.at(agirr.T, cmap, np.abs(ga_c).T)
    dgirr += 2 * U * agirr
    on = irr >= 0
    girr, dgirr = girr * on, dgirr * on
    gsr = sw * gspec
    dgsr = sw * dgspec + U * np.abs(gsr)
    terms = girr[:, None, :] * Yn[:, :, None] + gsr[:, None, :] * Yw[:, :, None]                     # [B,9,C]
    aterms = np.abs(girr)[:, None, :] * np.abs(Yn)[:, :, None] + np.abs(gsr)[:, None, :] * np.abs(Yw)[:, :, None]
    dterms = (dgirr[:, None, :] * np.abs(Yn)[:, :, None] + np.abs(girr)[:, None, :] * dYn[:, :, None] + dgsr[:, None, :] * np.abs(Yw)[:, :, None]
              + np.abs(gsr)[:, None, :] * dYw[:, :, None] + 3 * U * aterms)
    # a sample in a kink band may take the other branch in fp32: its whole contribution is in doubt
    dterms = np.where(kink_row[:, None, None], dterms + aterms + np.abs(g).sum(-1)[:, None, None] * q.max(-1)[:, None, None] * (np.abs(Yn) + np.abs(Yw))[:, :, None], dterms)
    grad_env = np.zeros_like(env)
    bound_env = np.zeros_like(env)
    grad_env[:9] = LOBE[:, None] * terms.sum(0)
    bound_env[:9] = LOBE[:, None] * (dterms.sum(0) + (40 + 4) * U * aterms.sum(0))
    out["grad_env"], out["bound_grad_env"] = grad_env, bound_env
    return out
