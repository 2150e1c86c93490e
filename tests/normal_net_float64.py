"""TEST INFRASTRUCTURE: a float64 restatement of the curved field's fine-normal chain as the framework executes it under fp16 autocast
(FactorizedNormalNet.forward, CurvedField.embed's rotation and normalisation, _forward_light's second normalisation and eval blend), with a
running per-element bound, for tests/test_normal_net_float64_cpu.py and tests/test_gpu_curved_light_infer.py.  Plain numpy.

It STARTS FROM HALF VALUES: the 8 features of the normal table, the 16 texture features, the first 12 height bands rounded to half, and the
six normalised weight matrices rounded to half (`layer.normalization().half()`: what the half GEMM multiplies with).  Biases are fp32.

    layer      s = W x                      exact in float64 (a product of two half values is exact in fp32, too)
               g = half(s)                  the half GEMM's output
               y = g + b                    fp32
               a = half(relu(y))            fp32 ReLU; the next layer's GEMM rounds its input to half         (hidden layers)
    angles     phi = g + b, theta = g + b   of the two nets' last layers, fp32
    toCoor     l = (sin t cos p, sin t sin p, cos t)                                                            fp32
    rotation   n_a = half(sum_b half(F[b, a]) half(l_b))        einsum("nba,nb->na") under autocast: a half product, fp32 accumulation
    normalise  n <- n / (|n| + 1e-5), twice   (tools/map.py:732, network_curvedfield.py:285)                   fp32
    eval       c = the raw coarse normal normalised twice (tools/map.py:720, :285);  n <- fc n + (1 - fc) c;  n <- n / (|n| + 1e-5)

THE ERROR MODEL bounds |v - helper| for ANY evaluation v of the same chain that accumulates every sum in fp32 in whatever order and rounds to
half at most where the list above does -- the HIP kernel (ascending order), the framework's GEMMs (unknown order), and the chain without any of
the half roundings.  u = 2^-24 (fp32, relative), UH = 2^-11 (half, relative), first order, every rounding once at its worst case:
  GEMM         |W| err_in  +  (n - 1) u sum_i |w_i x_i|  (n - 1 additions, each at most u times the sum of magnitudes)
               +  one half rounding of the output on EACH side: two values that differ by anything may land on neighbouring halfs,
                  2 UH |s| + 2^-24 (the subnormal spacing)
  bias, ReLU   + u |y| (the fp32 addition); ReLU is 1-Lipschitz
  next input   half(relu(y)): 2 UH |a| + 2^-24
  sin, cos     |d/dx| <= 1 times the angle's bound + 4 ulp = 8 u |value| (OpenCL C 3.0 section 7.4, the table the ROCm device library's
               functions are built to) + 2^-149-free: a value of 0 has no error term, which the products below do not need
  products     err(a b) = |a| err_b + |b| err_a + u |a b|
  rotation     half(l_b): 2 UH |l_b| + 2^-24; three exact products, two fp32 additions 2 u sum|terms|; the output's half rounding
  normalise    L = sqrt(sum v^2) + 1e-5: |dL| <= sum_j |v_j| err_j / |v| + 6 u L (three squares, two additions, the square root within
               1 ulp, the addition); out_c = v_c / L: err_c / L + |v_c| |dL| / L^2 + 3 u |out_c| (the quotient within 1 ulp + u)
  blend        fc err_n + (1 - fc) err_c + u (|fc n| + 2 |(1 - fc) c| + |s|)  (1 - fc is itself an fp32 difference: one more u on its product)
"""
import numpy as np

U = 2.0 ** -24
UH = 2.0 ** -11
SUB = 2.0 ** -24  # spacing of the half subnormals
N_BANDS = 12
SHAPES = {"phi": [(16, 20), (16, 16), (1, 16)], "theta": [(16, 28), (16, 16), (1, 16)]}


def _half(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _gemm(W, x, err):
    """-> half(W x) and its bound.  W [out, in] half-valued float64, x [B, in] half-valued float64, err [B, in]."""
    s = x @ W.T
    mag = np.abs(x) @ np.abs(W).T
    bound = err @ np.abs(W).T + (W.shape[1] - 1) * U * mag + 2 * UH * np.abs(s) + SUB
    return _half(s), bound


def lip_mlp(weights, biases, x):
    """One LipMLP in -> 16 -> 16 -> 1 from half-valued inputs x [B, in] (no error on them).  weights: three half-valued matrices [out, in];
    biases: three fp32 vectors.  -> angle [B], bound [B]."""
    a, err = np.asarray(x, np.float64), np.zeros(x.shape)
    for i, (W, b) in enumerate(zip(weights, biases)):
        W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
        g, bound = _gemm(W, a, err)
        y = g + b[None, :]
        bound = bound + U * np.abs(y)
        if i == len(weights) - 1:
            return y[:, 0], bound[:, 0]
        r = np.maximum(y, 0.0)
        a = _half(r)
        err = bound + 2 * UH * np.abs(r) + SUB


def _unit(v, err):
    n2 = np.linalg.norm(v, axis=-1, keepdims=True)
    L = n2 + 1e-5
    dL = (np.abs(v) * err).sum(-1, keepdims=True) / np.maximum(n2, 1e-300) + 6 * U * L
    out = v / L
    return out, err / L + np.abs(v) * dL / L ** 2 + 3 * U * np.abs(out)


def fine_normal(phi_feat, x_feat, z, weights, biases, tbn=None, coarse_raw=None, fc_weight=1.0, blend=False):
    """phi_feat [B,8], x_feat [B,16], z [B,>=12]: half values (any float dtype); weights / biases: {"phi": [W0, W1, W2], "theta": [...]};
    tbn [B,3,3] fp32 frames (rows t, b, n) or None (no rotation, no normalisation: the local normal of FactorizedNormalNet.forward);
    blend: the eval branch with coarse_raw [B,3] (the projector's raw normal) and fc_weight.
    -> dict(phi, theta, bound_phi, bound_theta, local, bound_local, normal, bound_normal) of float64 arrays."""
    z = _half(z)[:, :N_BANDS]
    phi, e_phi = lip_mlp(weights["phi"], biases["phi"], np.concatenate([_half(phi_feat), z], -1))
    theta, e_theta = lip_mlp(weights["theta"], biases["theta"], np.concatenate([_half(x_feat)[:, :16], z], -1))
    st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
    e_st, e_ct = e_theta + 8 * U * np.abs(st), e_theta + 8 * U * np.abs(ct)
    e_sp, e_cp = e_phi + 8 * U * np.abs(sp), e_phi + 8 * U * np.abs(cp)
    local = np.stack([st * cp, st * sp, ct], -1)
    e_local = np.stack([np.abs(st) * e_cp + np.abs(cp) * e_st + U * np.abs(st * cp), np.abs(st) * e_sp + np.abs(sp) * e_st + U * np.abs(st * sp), e_ct], -1)
    out = dict(phi=phi, theta=theta, bound_phi=e_phi, bound_theta=e_theta, local=local, bound_local=e_local)
    if tbn is None:
        out["normal"], out["bound_normal"] = local, e_local
        return out
    F = _half(np.asarray(tbn, np.float64).reshape(-1, 3, 3))                 # (the same fp32 input on every side: its rounding carries no error)
    lh = _half(local)
    e_lh = e_local + 2 * UH * np.abs(local) + SUB
    s = np.einsum("nba,nb->na", F, lh)
    mag = np.einsum("nba,nb->na", np.abs(F), np.abs(lh))
    e_n = np.einsum("nba,nb->na", np.abs(F), e_lh) + 2 * U * mag + 2 * UH * np.abs(s) + SUB
    n = _half(s)
    n, e_n = _unit(n, e_n)
    n, e_n = _unit(n, e_n)
    if blend:
        fc = float(np.float32(fc_weight))
        c, e_c = _unit(np.asarray(coarse_raw, np.float64), np.zeros((n.shape[0], 3)))
        c, e_c = _unit(c, e_c)
        s = fc * n + (1 - fc) * c
        e_s = abs(fc) * e_n + abs(1 - fc) * e_c + U * (np.abs(fc * n) + 2 * np.abs((1 - fc) * c) + np.abs(s))
        n, e_n = _unit(s, e_s)
    out["normal"], out["bound_normal"] = n, e_n
    return out


def pack(net):
    """The weights and biases of a FactorizedNormalNet as the fused chain's host side packs them: every layer's normalization().half() and its
    fp32 bias.  -> (weights, biases) dicts of numpy arrays, and the flat blocks (half [1312], fp32 [66]) in the C ABI's order."""
    import torch

    weights, biases, flat_w, flat_b = {}, {}, [], []
    with torch.no_grad():
        for name, mlp in (("phi", net.phi_net), ("theta", net.theta_net)):
            ws = [layer.normalization().detach().float().half().cpu() for layer in mlp.layers]
            bs = [layer.b.detach().float().cpu() for layer in mlp.layers]
            assert [tuple(w.shape) for w in ws] == SHAPES[name]
            weights[name], biases[name] = [w.double().numpy() for w in ws], [b.double().numpy() for b in bs]
            flat_w += [w.reshape(-1) for w in ws]
            flat_b += [b.reshape(-1) for b in bs]
    return weights, biases, torch.cat(flat_w).numpy(), torch.cat(flat_b).numpy()
