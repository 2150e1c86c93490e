"""`gridencoder.grid_clustering` -- drop-in for the reference's gridencoder/grid_clustering.py.

`GridEncoder_clustering` (grid_clustering.py:93-217) is the same hash-grid encoder as `GridEncoder` plus a
per-level `ClusteringLayer` (:93-127) whose Student-t soft-assignment KL loss is evaluated on slices
`embeddings[offsets[i]:offsets[i+1]]` of the table.  The encode runs on the HIP kernels; `clustering_loss` stays
plain torch with the host's level pick, as in the reference (it only needs the table to remain sliceable by `offsets`).

`grid_clustering_loss(embeddings, offsets, centres, level, alpha, weight)` is the same loss as one HIP call
(nerftex_grid_cluster_loss): the level is a DEVICE int32 (-1 = every level summed), nothing is read back, the backward is
the closed-form gradient -- capturable in a graph.  `GridEncoder_clustering.clustering_loss_device(level)` uses it;
`grid_cluster_step` is the step form a trainer calls after its backward: it ADDS grad_scale * d loss / d x into gradients
it already holds (ngp_harness/accelerate.py).
"""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .grid import GridEncoder, _grid_encode, grid_encode  # noqa: F401  (the reference module carries its own copy of both)


class ClusteringLayer(nn.Module):
    def __init__(self, n_clusters=4, hidden=2, cluster_centers=None, alpha=1.0):
        super().__init__()
        self.n_clusters = n_clusters
        self.alpha = alpha
        self.hidden = hidden
        if cluster_centers is None:
            dev = "cuda" if torch.cuda.is_available() else "cpu"  # the reference hard-codes .cuda()
            cluster_centers = torch.zeros(n_clusters, hidden, dtype=torch.float, device=dev)
            cluster_centers.uniform_(-1e-4, 1e-4)
        self.cluster_centers = nn.Parameter(cluster_centers)
        self.kl_loss = nn.KLDivLoss(reduction="mean")

    def forward(self, x):
        # x [N, hidden] -> soft assignment [N, n_clusters] with a Student-t kernel
        dist2 = ((x.unsqueeze(1) - self.cluster_centers) ** 2).sum(2)
        q = (1.0 / (1.0 + dist2 / self.alpha)) ** (float(self.alpha + 1) / 2)
        return q / q.sum(dim=1, keepdim=True)

    @staticmethod
    def _target(q):
        p = (q ** 2) / q.sum(0)
        return (p / p.sum(dim=1, keepdim=True)).detach()

    def clustering_loss(self, x):
        q = self(x)
        return self.kl_loss(q.log(), self._target(q))


def _max_level_rows(offsets):
    """The largest level's row count: sizes the launch (the kernels read every level's own count from `offsets` on the device).  One
    host copy per offsets tensor (and version), on first sight -- outside any capture, as the encoder's own registration is."""
    cached = getattr(offsets, "_nerftex_cluster_rows", None)
    if cached is None or cached[0] != (offsets.data_ptr(), offsets._version):
        host = offsets.detach().to("cpu", torch.int64)
        cached = ((offsets.data_ptr(), offsets._version), int((host[1:] - host[:-1]).max()))
        try:
            offsets._nerftex_cluster_rows = cached
        except AttributeError:
            pass
    return cached[1]


_SCRATCH_BYTES = {}


def grid_cluster_step(embeddings, offsets, centres, level, alpha=1.0, weight=1.0, loss=None, grad_table=None, grad_centres=None, grad_scale=None):
    """nerftex_grid_cluster_loss on torch tensors: embeddings fp32 [rows, C], offsets int32 [L + 1], centres fp32 [L, K, C], level a device
    int32 scalar (a view of a larger tensor is fine) -- 0..L-1, or -1 for every level summed.  Writes `loss` (a device fp32 scalar, allocated
    if None) = weight * KLDivLoss(mean) and returns it; grad_table [rows, C] / grad_centres [L, K, C] (fp32, optional) get grad_scale *
    d loss / d x ADDED (grad_scale: a device fp32 scalar, None = 1).  No host read, no synchronisation."""
    import ctypes

    from nerftex_hip import GridClusterDesc, check, lib, ptr, stream

    L, K, C = centres.shape
    assert embeddings.dtype == torch.float32 and embeddings.is_contiguous() and embeddings.dim() == 2 and embeddings.shape[1] == C, "embeddings: fp32 [rows, C]"
    assert centres.dtype == torch.float32 and centres.is_contiguous(), "centres: contiguous fp32 [L, K, C]"
    assert offsets.dtype == torch.int32 and offsets.numel() == L + 1 and level.dtype == torch.int32 and level.numel() == 1
    for t in (grad_table, grad_centres):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous()), "gradients: contiguous fp32"
    assert grad_table is None or grad_table.shape == embeddings.shape
    assert grad_centres is None or grad_centres.shape == centres.shape
    assert grad_scale is None or (grad_scale.dtype == torch.float32 and grad_scale.numel() == 1)
    if loss is None:
        loss = torch.empty((), dtype=torch.float32, device=embeddings.device)
    d = GridClusterDesc(ptr(embeddings), ptr(offsets), C, L, K, _max_level_rows(offsets), ptr(centres), float(alpha), float(weight), ptr(level),
                        ptr(grad_scale), ptr(loss), ptr(grad_table), ptr(grad_centres), None, 0)
    key = (C, L, K, d.max_level_rows)
    if key not in _SCRATCH_BYTES:
        n = ctypes.c_size_t()
        check(lib.nerftex_grid_cluster_scratch_bytes(ctypes.byref(d), ctypes.byref(n)))
        _SCRATCH_BYTES[key] = n.value
    scratch = torch.empty(_SCRATCH_BYTES[key], dtype=torch.uint8, device=embeddings.device)
    d.scratch, d.scratch_bytes = ptr(scratch), scratch.numel()
    check(lib.nerftex_grid_cluster_loss(ctypes.byref(d), stream()))
    return loss


class _GridClusteringLoss(Function):
    @staticmethod
    def forward(ctx, embeddings, offsets, centres, level, alpha, weight):
        embeddings, centres = embeddings.detach().contiguous(), centres.detach().contiguous()
        ctx.save_for_backward(embeddings, offsets, centres, level)
        ctx.alpha, ctx.weight = alpha, weight
        return grid_cluster_step(embeddings, offsets, centres, level, alpha, weight)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        embeddings, offsets, centres, level = ctx.saved_tensors
        gt = torch.zeros_like(embeddings) if ctx.needs_input_grad[0] else None  # dense: zero outside the level
        gc = torch.zeros_like(centres) if ctx.needs_input_grad[2] else None
        if gt is not None or gc is not None:  # the same kernel with the incoming gradient as its scale
            grid_cluster_step(embeddings, offsets, centres, level, ctx.alpha, ctx.weight, grad_table=gt, grad_centres=gc,
                              grad_scale=g.detach().float().reshape(()).contiguous())
        return gt, None, gc, None, None, None


def grid_clustering_loss(embeddings, offsets, centres, level, alpha=1.0, weight=1.0):
    """weight * the reference's clustering loss of level `level` (device int32; -1 = every level summed) as one HIP call, differentiable in
    the table and the stacked centres [L, K, C]."""
    return _GridClusteringLoss.apply(embeddings, offsets, centres, level, alpha, weight)


class GridEncoder_clustering(GridEncoder):
    def __init__(self, input_dim=3, num_levels=4, level_dim=2, per_level_scale=2, base_resolution=16, log2_hashmap_size=19,
                 desired_resolution=None, gridtype="hash", align_corners=False):
        super().__init__(input_dim, num_levels, level_dim, per_level_scale, base_resolution, log2_hashmap_size, desired_resolution,
                         gridtype, align_corners)
        self.cluster_layers = nn.ModuleList([ClusteringLayer() for _ in range(num_levels)])
        self.kl_loss = nn.KLDivLoss(reduction="mean")

    def clustering_loss(self, pick_level=True):
        levels = np.random.choice(np.arange(self.num_levels), [1]) if pick_level else np.arange(self.num_levels)
        offsets = self.offsets.tolist()
        loss = 0.0
        for i in levels:
            rows = self.embeddings[offsets[i]: offsets[i + 1]]
            q = self.cluster_layers[i](rows)
            loss = loss + self.kl_loss(q.log(), ClusteringLayer._target(q))
        return loss

    def clustering_loss_device(self, level=None):
        """clustering_loss on the device: `level` a device int32 tensor (one element) picks the level, None = every level summed
        (pick_level=False).  The per-level centres are stacked on the device; nothing is read back."""
        layers = self.cluster_layers
        assert all(l.alpha == layers[0].alpha and l.hidden == self.level_dim for l in layers), "one alpha, hidden == level_dim"
        centres = torch.stack([l.cluster_centers for l in layers])
        if level is None:
            level = torch.full((), -1, dtype=torch.int32, device=self.embeddings.device)
        return grid_clustering_loss(self.embeddings, self.offsets, centres, level, float(layers[0].alpha), 1.0)
