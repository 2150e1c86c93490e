"""TEST INFRASTRUCTURE: a float64 restatement of the planar lookup of an imported feature map (the `imported_type == 'field'` branch of
MeshFeatureField.forward, tools/map.py:646-668: grid_sample(bilinear, align_corners=True, padding zeros) of a [H, W, C] map, and
FreqEncoder(height)) with a per-element bound on the error of an fp32 evaluation narrowed to half, for tests/test_import_field_cpu.py and
tests/test_gpu_import_field.py.  Plain numpy.

It STARTS FROM THE fp32 u, v, sdf BITS: the three are pinned bit for bit against the framework's own expressions by the GPU test, and the
mask is decided on them by exact comparisons, so nothing upstream of the interpolation enters here.

    iu = ((u + 1) / 2) (H - 1),  iv = ((v + 1) / 2) (W - 1),  i0 = floor(iu),  j0 = floor(iv)                 (u along the map's FIRST axis)
    value_c = (i0+1-iu)(j0+1-iv) F[i0,j0,c] + (iu-i0)(j0+1-iv) F[i0+1,j0,c] + (i0+1-iu)(iv-j0) F[i0,j0+1,c] + (iu-i0)(iv-j0) F[i0+1,j0+1,c]
    with F = 0 outside [0,H) x [0,W)
    ladder  = [sdf, sin(sdf 2^0), cos(sdf 2^0), ..., sin(sdf 2^11), cos(sdf 2^11)]

THE ERROR MODEL: u = 2^-24 (half an fp32 ulp, relative), every rounding enters once at its worst case, first order.
  position     iu in fp32: the addition, the division and the product round once each -- |d iu| <= 3 u max(|iu|, |u + 1| (H - 1) / 2); likewise iv.
               The interpolant is continuous and piecewise bilinear, so a position error moves the value by at most the steepest slope it can
               meet: slope_u,c = the largest |F[i+1,j,c] - F[i,j,c]| over the cell and its two neighbours along u (an fp32 iu on the other side
               of a texel border lands in the neighbouring cell, which is why no row is excluded), both j rows; likewise slope_v.  The
               padding zeros are part of F here, so the ramp from a border texel down to 0 outside the map is covered by the same term.
  weights      i0 + 1 is exact; each 1-D difference rounds once (u, relative), their product once: |dw_k| <= 3 u w_k.
  sum          four products (u |F w| each) and three additions (u times a partial sum of magnitudes each, at most u sum_k |F_k| w_k):
               together with the weights (3 + 1 + 3) u sum_k |F_k| w_k = 7 u A, A = sum_k |F_k| w_k.
  narrowing    one rounding to half of the fp32 value: 2^-11 relative (of the float64 value plus the fp32 bound), 2^-25 absolute in the
               subnormal range.
  ladder       the argument sdf 2^k is exact (a power of two); sinf / cosf within 4 fp32 ulp = 8 u |value| (OpenCL C 3.0 section 7.4, the table the
               ROCm device library's float functions are built to; the figure tests/normal_net_float64.py uses), then the half rounding.
No row and no element is excluded.
"""
import numpy as np

U = 2.0 ** -24
UH = 2.0 ** -11
HALF_TINY = 2.0 ** -25
N_FREQS = 12


def _half_bound(value, fp32_bound):
    return fp32_bound + UH * (np.abs(value) + fp32_bound) + HALF_TINY


def bilinear(features, u, v):
    """features [H,W,C] fp32, u, v [N] fp32 -> (value [N,C] float64, bound [N,C] on |half(fp32 evaluation) - value|)."""
    F = np.asarray(features)
    assert F.dtype == np.float32 and np.asarray(u).dtype == np.float32 and np.asarray(v).dtype == np.float32
    H, W, C = F.shape
    P = 3  # padding zeros: the cell, its neighbours, and one texel beyond the map for coordinates just outside
    Fp = np.zeros((H + 2 * P, W + 2 * P, C), np.float64)
    Fp[P:P + H, P:P + W] = F
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    iu, iv = ((u + 1) / 2) * (H - 1), ((v + 1) / 2) * (W - 1)
    far = ~(np.isfinite(iu) & np.isfinite(iv)) | (iu < -1.5) | (iu > H + 0.5) | (iv < -1.5) | (iv > W + 0.5)  # beyond every texel's support: 0
    iuc, ivc = np.where(far, 0.0, iu), np.where(far, 0.0, iv)
    i0, j0 = np.floor(iuc).astype(np.int64), np.floor(ivc).astype(np.int64)
    wu1, wv1 = iuc - i0, ivc - j0
    wu0, wv0 = 1 - wu1, 1 - wv1
    a, b = i0 + P, j0 + P
    t = [Fp[a, b], Fp[a + 1, b], Fp[a, b + 1], Fp[a + 1, b + 1]]
    w = [wu0 * wv0, wu1 * wv0, wu0 * wv1, wu1 * wv1]
    value = sum(tk * wk[:, None] for tk, wk in zip(t, w))
    A = sum(np.abs(tk) * wk[:, None] for tk, wk in zip(t, w))
    slope_u = np.zeros_like(value)
    slope_v = np.zeros_like(value)
    for d in (-1, 0, 1):
        for e in (0, 1):
            slope_u = np.maximum(slope_u, np.abs(Fp[a + d + 1, b + e] - Fp[a + d, b + e]))
            slope_v = np.maximum(slope_v, np.abs(Fp[a + e, b + d + 1] - Fp[a + e, b + d]))
    d_iu = 3 * U * np.maximum(np.abs(iuc), np.abs(np.where(far, 0.0, u) + 1) * (H - 1) / 2)
    d_iv = 3 * U * np.maximum(np.abs(ivc), np.abs(np.where(far, 0.0, v) + 1) * (W - 1) / 2)
    fp32_bound = 7 * U * A + slope_u * d_iu[:, None] + slope_v * d_iv[:, None]
    value = np.where(far[:, None], 0.0, value)
    fp32_bound = np.where(far[:, None], 0.0, fp32_bound)
    return value, _half_bound(value, fp32_bound)


def ladder(sdf):
    """sdf [N] fp32 -> (FreqEncoder(sdf) [N,25] float64, bound [N,25] on |half(fp32 evaluation) - value|)."""
    assert np.asarray(sdf).dtype == np.float32
    s = np.asarray(sdf, np.float64)
    cols, bounds = [s], [np.zeros_like(s)]
    for k in range(N_FREQS):
        for fn in (np.sin, np.cos):
            val = fn(s * 2.0 ** k)
            cols.append(val)
            bounds.append(8 * U * np.abs(val))
    value, fp32_bound = np.stack(cols, -1), np.stack(bounds, -1)
    return value, _half_bound(value, fp32_bound)


def lookup_reference(features, u, v, sdf):
    """-> (value [N, C + 25] float64, bound): the embedding columns the kernel writes, half-narrowed, against float64."""
    f, fb = bilinear(features, u, v)
    z, zb = ladder(sdf)
    return np.concatenate([f, z], -1), np.concatenate([fb, zb], -1)


# ---- the cases the CPU and GPU tests share: inputs that sit on every edge of the lookup, and the framework's own expressions on them ----------------
MAPS = [(1, 1), (2, 3), (5, 4), (64, 48)]  # (the non-square ones catch a swapped axis)
H_THRESHOLD = 0.0625


def map_bounds(H, W):
    """grid_gap = 1 / H: bounds = [0.5, 0.5 W / H] -- bounds[0] = 0.5 makes |sdf| == h_threshold representable in both modes."""
    return 0.5, 0.5 * W / H


def seeded_map(H, W, seed=7):
    return np.random.default_rng(seed + 1000 * H + W).uniform(-0.5, 0.5, (H, W, 16)).astype(np.float32)


def case_points(H, W, B, rescale, rate, offset, seed=0):
    """[B,3] fp32 sample positions: first the edge cases -- exact texel centres (the corners and seeded others), u, v = +-1 exactly and one fp32
    step outwards, |sdf| exactly at the threshold (where rate and offset leave it representable) and one step either side -- then seeded points
    in [-1.2, 1.2]^2 x 1.4 h.  The positions are built by inverting the mode's map in fp32; what u, v, sdf they really give is the framework
    expressions' business (`torch_expressions`), which the tests evaluate on the same bits."""
    rng = np.random.default_rng(seed + 7919 * H + 31 * W + B)
    one = np.float32(1)
    b0, b1 = (np.float32(b) for b in map_bounds(H, W))
    rate, offset = np.float32(rate), np.float32(offset)

    def centres(n, count):
        if n == 1:
            return [np.float32(0)]  # (any coordinate reads texel 0 with weight 1 at iu = 0; u = 0 is as good as any)
        idx = sorted({0, n - 1, *rng.integers(0, n, count).tolist()})
        return [np.float32(2 * i) / np.float32(n - 1) - one for i in idx]

    uv = [(cu, cv) for cu in centres(H, 3) for cv in centres(W, 3)]
    edge = [one, -one, np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(-2)), np.nextafter(one, np.float32(0)), np.nextafter(-one, np.float32(0))]
    uv += [(e, np.float32(0.25)) for e in edge] + [(np.float32(-0.5), e) for e in edge] + [(e, e) for e in edge[:4]]
    h = np.float32(H_THRESHOLD)
    heights = [np.float32(0), h, -h, np.nextafter(h, np.float32(0)), np.nextafter(h, np.float32(1)), np.nextafter(-h, np.float32(0)), np.nextafter(-h, np.float32(-1))]
    rows = [(cu, cv, np.float32(0)) for cu, cv in uv] + [(np.float32(0.125), np.float32(-0.375), s) for s in heights]
    n_rand = max(B - len(rows), 0)
    rand = np.concatenate([rng.uniform(-1.2, 1.2, (n_rand, 2)), rng.uniform(-1.4, 1.4, (n_rand, 1)) * float(h)], -1).astype(np.float32)
    target = np.concatenate([np.asarray(rows, np.float32).reshape(-1, 3), rand], 0)
    if B < len(rows):  # (a small batch: spread what it can hold over the kinds of edge)
        target = target[np.linspace(0, len(rows) - 1, B).round().astype(np.int64)]
    u, v, s = target[:, 0], target[:, 1], target[:, 2]
    if rescale:
        xyz = np.stack([u / rate, v / rate, ((s + offset) / rate) / b0], -1)
    else:
        xyz = np.stack([u * b0, v * b1, s + offset], -1)
    return np.ascontiguousarray(xyz, np.float32)


def torch_expressions(x, features, bounds, rescale, rate, offset, h_threshold):
    """The reference's expressions (tools/map.py:649-663) as framework ops on x's device: -> p_uv [N,2], sdf [N], h_mask [N], x_embed [N,C] fp32.
    features: [H,W,C] tensor on the same device.  The divisors are tensors (a true division on every device)."""
    import torch

    b0, b1 = (torch.tensor(b, dtype=torch.float32, device=x.device) for b in bounds)
    if rescale:
        p_sur = x[..., :2] * rate
        sdf = x[..., -1:] * bounds[0] * rate
    else:
        p_sur = torch.stack([x[..., 0] / b0, x[..., 1] / b1], dim=-1)
        sdf = x[..., -1:]
    sdf = sdf - offset
    h_mask = sdf[..., 0].abs() < h_threshold
    h_mask = torch.logical_and(h_mask, (p_sur >= -1.0).all(dim=-1))
    h_mask = torch.logical_and(h_mask, (p_sur <= 1.0).all(dim=-1))
    image = features.permute(2, 1, 0).unsqueeze(0)  # [1, C, W, H]: the grid's first coordinate (u) indexes the last axis = the map's first
    x_embed = torch.nn.functional.grid_sample(image, p_sur[None, None], align_corners=True, padding_mode="zeros")[0, :, 0].permute(1, 0)
    return p_sur, sdf[..., 0], h_mask, x_embed
