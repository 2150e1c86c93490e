"""The clustering regulariser's closed-form gradient (csrc/grid_cluster.inc, include/nerftex_hip.h: nerftex_grid_cluster_loss) and the
curved trainer's level picks, on the host: no GPU, no library."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nerf-texture_amd"))


def reference_loss(x, c, alpha=1.0):
    """gridencoder/grid_clustering.py:93-127 of the reference (ClusteringLayer.forward + clustering_loss), any dtype."""
    d2 = ((x.unsqueeze(1) - c) ** 2).sum(2)
    q = (1.0 / (1.0 + d2 / alpha)) ** (float(alpha + 1) / 2)
    q = q / q.sum(dim=1, keepdim=True)
    p = (q ** 2) / q.sum(0)
    p = (p / p.sum(dim=1, keepdim=True)).detach()
    return torch.nn.KLDivLoss(reduction="mean")(q.log(), p)


def closed_form(x, c, weight, alpha=1.0):
    """What the kernel computes: d loss / d x_i = sum_k w / (N K) (p_ik - q_ik) ((alpha + 1) / 2) / (alpha + d_ik) 2 (x_i - c_k);
    d loss / d c_k = minus that summed over i."""
    N, K = x.shape[0], c.shape[0]
    diff = x.unsqueeze(1) - c  # [N, K, C]
    d2 = (diff ** 2).sum(2)
    n = (1.0 / (1.0 + d2 / alpha)) ** ((alpha + 1) / 2)
    q = n / n.sum(1, keepdim=True)
    p = q ** 2 / q.sum(0)
    p = p / p.sum(1, keepdim=True)
    coef = weight / (N * K) * (p - q) * ((alpha + 1) / 2) / (alpha + d2)  # [N, K]
    g = coef.unsqueeze(-1) * 2 * diff
    return g.sum(1), -g.sum(0)


@pytest.mark.parametrize("K", [4, 6])
@pytest.mark.parametrize("alpha", [1.0, 2.5])
def test_closed_form_gradient_equals_autograd_float64(K, alpha):
    gen = torch.Generator().manual_seed(K)
    x = (torch.rand(3000, 2, generator=gen, dtype=torch.float64) - 0.5).requires_grad_(True)  # trained scale: U(-0.5, 0.5)
    c = (torch.rand(K, 2, generator=gen, dtype=torch.float64) - 0.5).requires_grad_(True)
    w = 1e-2
    (w * reference_loss(x, c, alpha)).backward()
    gx, gc = closed_form(x.detach(), c.detach(), w, alpha)
    assert float(x.grad.abs().max()) > 0 and float(c.grad.abs().max()) > 0
    torch.testing.assert_close(gx, x.grad, rtol=1e-10, atol=1e-22)
    torch.testing.assert_close(gc, c.grad, rtol=1e-9, atol=1e-20)


def test_ring_levels_follow_the_reference_draws():
    from ngp_harness.accelerate import RING, draw_ring_levels

    np.random.seed(123)
    want = [int(np.random.choice(np.arange(8), [1])[0]) for _ in range(3 * RING)]  # the reference: one pick per training step
    np.random.seed(123)
    got = np.concatenate([draw_ring_levels(8) for _ in range(3)])
    assert got.dtype == np.int32 and got.shape == (3 * RING,)
    assert got.tolist() == want
    assert len(set(want)) > 1
