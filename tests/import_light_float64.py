"""TEST INFRASTRUCTURE: tests/normal_net_float64.py's fine-normal chain for an IMPORTED planar map (the `pred_normal` part of the 'field' branch
of MeshFeatureField.forward, tools/map.py:670-675, :722-730), in float64 with the same running per-element bound, for
tests/test_import_light_cpu.py and tests/test_gpu_import_light.py.  Plain numpy.  It imports normal_net_float64 and adds what the import
branch adds: the normal net is fed from the sampled phi map, and the local normal is rotated TWICE -- by the texel's frame, then by the sampled
patch's inverted frame -- each rotation the half product the mesh chain's single one is:

    rotation 1  n1_a = half(sum_b half(F1[b, a]) half(l_b))                 F1 = the sampled local_tbn
    rotation 2  n2_a = half(sum_b half(F2[b, a]) half(n1_b))                F2 = row `id` of sample_tbn_inv; half(n1) = n1
    normalise   twice; eval: the blend with the coarse normal (0, 0, 1) normalised twice; normalise        (as normal_net_float64)

THE ERROR MODEL is normal_net_float64's (u = 2^-24, UH = 2^-11, SUB = 2^-24), with one more rotation term
    |F2| err_in + 2 u mag + 2 UH |s| + SUB,   err_in = err(n1) + 2 UH |n1| + SUB  (the half rounding of the product's input, on each side)
`fp32_inputs` widens it for an evaluation that never rounded its INPUTS to half -- the framework's ops on the CPU, where no autocast rounds the
features, the normalised weights or the frames (the reference's run behind tests/golden/ref_python_import_field_sh.npz): the exact differences
|x - half(x)| of the features and the frames enter as input errors, the weights' |W - half(W)| as |dW| (|x| + err) per product.
"""
import numpy as np

import normal_net_float64 as nn64

U, UH, SUB = nn64.U, nn64.UH, nn64.SUB
_half = nn64._half


def _gemm(W, x, err, dW=None):
    g, bound = nn64._gemm(W, x, err)
    if dW is not None:
        bound = bound + (np.abs(x) + err) @ np.abs(dW).T
    return g, bound


def lip_mlp(weights, biases, x, err, dweights=None):
    """nn64.lip_mlp with an error on the inputs and (dweights) on the weights: with zeros and None it is that function."""
    a, err = np.asarray(x, np.float64), np.asarray(err, np.float64)
    for i, (W, b) in enumerate(zip(weights, biases)):
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        g, bound = _gemm(W, a, err, None if dweights is None else dweights[i])
        y = g + b[None, :]
        bound = bound + U * np.abs(y)
        if i == len(weights) - 1:
            return y[:, 0], bound[:, 0]
        r = np.maximum(y, 0.0)
        a = _half(r)
        err = bound + 2 * UH * np.abs(r) + SUB


def _rotate(F32, v, e_v, fp32_inputs):
    """half(sum_b half(F[b, a]) v_b) for half-valued v with bound e_v -> (n, e_n)."""
    F32 = np.asarray(F32, np.float64).reshape(-1, 3, 3)
    F = _half(F32)
    s = np.einsum("nba,nb->na", F, v)
    mag = np.einsum("nba,nb->na", np.abs(F), np.abs(v))
    e = np.einsum("nba,nb->na", np.abs(F), e_v) + 2 * U * mag + 2 * UH * np.abs(s) + SUB
    if fp32_inputs:
        e = e + np.einsum("nba,nb->na", np.abs(F32 - F), np.abs(v) + e_v)
    return _half(s), e


def fine_normal(phi_feat, x_feat, z, weights, biases, local_tbn, sample_tbn_inv, fc_weight=1.0, blend=False, fp32_inputs=False, dweights=None):
    """phi_feat [B,8] (the sampled phi map), x_feat [B,16], z [B,>=12]; weights / biases as nn64.pack gives them; local_tbn, sample_tbn_inv
    [B,3,3] fp32.  blend: the eval branch with the coarse normal (0, 0, 1) and fc_weight.  fp32_inputs (+ dweights = {name: [|W32 - half(W32)|]}):
    see the module docstring.  -> dict(local, bound_local, fine, bound_fine, normal, bound_normal): `fine` is MeshFeatureField's normal_fine
    (normalised once, :730), `normal` the shading normal handed to the light head."""
    zz = np.asarray(z, np.float64)[:, :nn64.N_BANDS]
    ins = {"phi": np.concatenate([np.asarray(phi_feat, np.float64), zz], -1), "theta": np.concatenate([np.asarray(x_feat, np.float64)[:, :16], zz], -1)}
    ang = {}
    for name in ("phi", "theta"):
        xh = _half(ins[name])
        err = np.abs(ins[name] - xh) if fp32_inputs else np.zeros(xh.shape)
        ang[name] = lip_mlp(weights[name], biases[name], xh, err, None if dweights is None else dweights[name])
    (phi, e_phi), (theta, e_theta) = ang["phi"], ang["theta"]
    st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
    e_st, e_ct = e_theta + 8 * U * np.abs(st), e_theta + 8 * U * np.abs(ct)
    e_sp, e_cp = e_phi + 8 * U * np.abs(sp), e_phi + 8 * U * np.abs(cp)
    local = np.stack([st * cp, st * sp, ct], -1)
    e_local = np.stack([np.abs(st) * e_cp + np.abs(cp) * e_st + U * np.abs(st * cp), np.abs(st) * e_sp + np.abs(sp) * e_st + U * np.abs(st * sp), e_ct], -1)
    n1, e1 = _rotate(local_tbn, _half(local), e_local + 2 * UH * np.abs(local) + SUB, fp32_inputs)
    n2, e2 = _rotate(sample_tbn_inv, n1, e1 + 2 * UH * np.abs(n1) + SUB, fp32_inputs)
    fine, e_fine = nn64._unit(n2, e2)
    n, e_n = nn64._unit(fine, e_fine)
    if blend:
        fc = float(np.float32(fc_weight))
        coarse = np.zeros(n.shape)
        coarse[:, 2] = 1.0
        c, e_c = nn64._unit(coarse, np.zeros(n.shape))
        c, e_c = nn64._unit(c, e_c)
        s = fc * n + (1 - fc) * c
        e_s = abs(fc) * e_n + abs(1 - fc) * e_c + U * (np.abs(fc * n) + 2 * np.abs((1 - fc) * c) + np.abs(s))
        n, e_n = nn64._unit(s, e_s)
    return dict(phi=phi, theta=theta, local=local, bound_local=e_local, fine=fine, bound_fine=e_fine, normal=n, bound_normal=e_n)


def pack_fp32(net):
    """nn64.pack(net)'s weights and biases, and |normalization() - normalization().half()| per layer (the `dweights` of an fp32 evaluation)."""
    import torch

    weights, biases, _, _ = nn64.pack(net)
    dweights = {}
    with torch.no_grad():
        for name, mlp in (("phi", net.phi_net), ("theta", net.theta_net)):
            dweights[name] = [np.abs(layer.normalization().detach().double().numpy() - w) for layer, w in zip(mlp.layers, weights[name])]
    return weights, biases, dweights


# ---- what the CPU and the GPU test share: seeded maps for a planar_float64.MAPS size, and a field carrying the fixture's networks --------------------

def seeded_light_maps(H, W, P, seed=3):
    """-> phi_embed [H,W,8], local_tbn [H,W,9], sample_tbn [P,3,3], sample_tbn_ids [H,W] fp32: frames that are not orthonormal and differ per texel
    and per patch, every id in [0, P)."""
    rng = np.random.default_rng(seed + 1000 * H + W)
    phi = rng.uniform(-0.5, 0.5, (H, W, 8)).astype(np.float32)
    local = (np.eye(3, dtype=np.float32).reshape(9) + rng.normal(0, 0.35, (H, W, 9))).astype(np.float32)
    sample = (np.eye(3, dtype=np.float32) + rng.normal(0, 0.3, (P, 3, 3))).astype(np.float32)
    ids = rng.integers(0, P, (H, W)).astype(np.float32)
    return phi, local, sample, ids


def load_normal_net(net, g):
    """The fixture's LipMLP parameters into a FactorizedNormalNet."""
    import torch

    with torch.no_grad():
        for name, mlp in (("phi", net.phi_net), ("theta", net.theta_net)):
            for i, layer in enumerate(mlp.layers):
                layer.W.copy_(torch.from_numpy(g[f"{name}_W{i}"])), layer.b.copy_(torch.from_numpy(g[f"{name}_b{i}"])), layer.c.fill_(float(g[f"{name}_c{i}"]))
    return net


def import_fixture_maps(field, g, times=1):
    """import_field with the fixture's six arrays, `times` times (1: `rescale` True, the fixture's mode A; 2: mode B)."""
    for _ in range(times):
        field.import_field(g["features"], float(g["grid_gap"]), phi_embed=g["phi_embed"], local_tbn=g["local_tbn"], sample_tbn=g["sample_tbn"],
                           sample_tbn_ids=g["sample_tbn_ids"])
    return field
