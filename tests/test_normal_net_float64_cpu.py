"""CPU: tests/normal_net_float64.py (the float64 restatement of the fine-normal chain at the framework's rounding points, with its running
bound) against FactorizedNormalNet's own networks run in float64 WITHOUT any of the roundings: the difference -- what the half roundings of the
layer outputs make of the angles, the rotation and the normalisations -- sits inside the helper's own bound on every element, for the plain
local normal, the rotated and normalised one and the eval blend.  The double-precision twin multiplies with the half-rounded normalised
weights (the helper's starting point), so nothing but the listed roundings separates the two."""
import numpy as np
import pytest
import torch

import normal_net_float64 as nn64


def _net(seed, scale):
    """A FactorizedNormalNet with weights large enough for angles of order 1.  scale 1: the Lipschitz constants out of the way (c = 50);
    scale 8: the constructor's c = 1 under row sums far above softplus(1) -- the normalisation is active on every row."""
    from ngp_harness.curved import FactorizedNormalNet

    torch.manual_seed(seed)
    net = FactorizedNormalNet(x_dim=16, z_dim=25)
    with torch.no_grad():
        for mlp in (net.phi_net, net.theta_net):
            for layer in mlp.layers:
                layer.W.mul_(4.0 * scale)
                layer.b.normal_(0, 0.2)
                if scale == 1.0:
                    layer.c.fill_(50.0)
    return net


def _twin_angles(net, weights, phi_in, theta_in):
    """phi, theta of the module's two LipMLPs in float64 with W = the half-rounded normalised weights and the bound out of the way."""
    import copy

    out = []
    for name, mlp, x in (("phi", net.phi_net, phi_in), ("theta", net.theta_net, theta_in)):
        twin = copy.deepcopy(mlp).double()
        with torch.no_grad():
            for layer, W in zip(twin.layers, weights[name]):
                layer.W.copy_(torch.from_numpy(W))
                layer.c.fill_(1e4)  # softplus(1e4) exceeds every row sum: normalization() returns W itself
                assert torch.equal(layer.normalization(), layer.W)
            out.append(twin(torch.from_numpy(x)))
    return out


def _inputs(B, seed):
    rng = np.random.default_rng(seed)
    phi_feat = rng.uniform(-0.5, 0.5, (B, 8)).astype(np.float16)
    x_feat = rng.uniform(-0.5, 0.5, (B, 16)).astype(np.float16)
    h = rng.uniform(-0.05, 0.05, (B, 1))
    bands = [h] + [f(h * 2.0 ** k) for k in range(12) for f in (np.sin, np.cos)]
    z = np.concatenate(bands, -1).astype(np.float32).astype(np.float16)
    q, _ = np.linalg.qr(rng.normal(size=(B, 3, 3)))
    coarse = rng.normal(size=(B, 3)).astype(np.float32)
    return phi_feat, x_feat, z, q.astype(np.float32), coarse


def _inside(name, got, want, bound):
    assert np.isfinite(want).all() and np.isfinite(bound).all(), name
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    print(f"{name}: max error / bound {float(ratio.max()):.3f}, max error {float(err.max()):.3e}, median bound {float(np.median(bound)):.3e}")
    assert ratio.max() <= 1.0, (name, float(ratio.max()))


@pytest.mark.parametrize("scale", (1.0, 8.0))
def test_helper_against_the_module_in_float64(scale):
    net = _net(3, scale)
    weights, biases, flat_w, flat_b = nn64.pack(net)
    assert flat_w.shape == (1312,) and flat_w.dtype == np.float16 and flat_b.shape == (66,) and flat_b.dtype == np.float32
    if scale > 1:
        with torch.no_grad():
            assert any(bool((l.W.abs().sum(1) > l.bound()).any()) for l in net.phi_net.layers), "the Lipschitz normalisation is active"
    B = 3000
    phi_feat, x_feat, z, tbn, coarse = _inputs(B, 11)
    phi_in = np.concatenate([phi_feat, z[:, :12]], -1).astype(np.float64)
    theta_in = np.concatenate([x_feat, z[:, :12]], -1).astype(np.float64)
    with torch.no_grad():
        phi, theta = _twin_angles(net, weights, phi_in, theta_in)
        local = net.toCoor(phi=phi, theta=theta)
        F = torch.from_numpy(tbn).double()
        fine = torch.einsum("nba,nb->na", F, local)
        fine = fine / (fine.norm(dim=-1, keepdim=True) + 1e-5)
        fine = fine / (fine.norm(dim=-1, keepdim=True) + 1e-5)
        c = torch.from_numpy(coarse).double()
        c = c / (c.norm(dim=-1, keepdim=True) + 1e-5)
        c = c / (c.norm(dim=-1, keepdim=True) + 1e-5)
        fc = float(np.float32(0.7))
        blend = fc * fine + (1 - fc) * c
        blend = blend / (blend.norm(dim=-1, keepdim=True) + 1e-5)
    if scale == 1.0:
        assert float(phi.std()) > 0.1 and float(theta.std()) > 0.1, "angles of a tenth of a radian and more that vary with the inputs"
    plain = nn64.fine_normal(phi_feat, x_feat, z, weights, biases)
    _inside(f"phi | scale {scale}", phi[:, 0].numpy(), plain["phi"], plain["bound_phi"])
    _inside(f"theta | scale {scale}", theta[:, 0].numpy(), plain["theta"], plain["bound_theta"])
    _inside(f"local normal | scale {scale}", local.numpy(), plain["normal"], plain["bound_normal"])
    rot = nn64.fine_normal(phi_feat, x_feat, z, weights, biases, tbn=tbn)
    _inside(f"fine normal | scale {scale}", fine.numpy(), rot["normal"], rot["bound_normal"])
    ev = nn64.fine_normal(phi_feat, x_feat, z, weights, biases, tbn=tbn, coarse_raw=coarse, fc_weight=0.7, blend=True)
    _inside(f"eval blend | scale {scale}", blend.numpy(), ev["normal"], ev["bound_normal"])
    assert float(np.abs(rot["normal"] - plain["normal"]).max()) > 1e-2, "the rotation is applied"
    # the bound is a worst case over the layers (every |W| row sum multiplies what came in), not a tolerance: it stays a small fraction of a unit
    # vector's components even with these weights, 4 to 32 times the constructor's
    assert float(np.median(plain["bound_phi"])) < 0.1 and float(np.median(rot["bound_normal"])) < 0.5
    # ... and the helper does round: without the roundings its angles would equal the twin's to float64 precision
    assert float(np.abs(phi[:, 0].numpy() - plain["phi"]).max()) > 1e-6


def test_helper_rounds_where_the_framework_does():
    """One layer by hand: half inputs, half weights, the exact sum rounded to half, the fp32 bias added behind it."""
    W = np.array([[0.5, 2.0 ** -12]], np.float64)
    x = np.array([[1.0, 1.0]], np.float64)
    g, bound = nn64._gemm(W, x, np.zeros_like(x))
    assert g[0, 0] == 0.5 and bound[0, 0] >= 2.0 ** -12  # 0.5 + 2^-12 is a tie between two halfs: rounds to even
    angle, _ = nn64.lip_mlp([np.eye(16, 20), np.eye(16), np.ones((1, 16)) / 16], [np.zeros(16), np.zeros(16), np.array([0.25])],
                            np.full((1, 20), 1.0 + 2.0 ** -10))
    assert angle[0] == (1.0 + 2.0 ** -10) + 0.25
