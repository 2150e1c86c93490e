"""GPU: the curved field's training step on the accelerated path.

  * nerftex_grid_cluster_loss (csrc/grid_cluster.inc): the reference's clustering regulariser (gridencoder/grid_clustering.py:93-217) and its
    closed-form gradient against the reference's fixture, float64 autograd per level of a curved-size table, itself (bit for bit), a captured
    graph, and the autograd Function gridencoder.grid_clustering_loss;
  * accelerate(Renderer(CurvedField)): replayed graphs against the same trainer run eagerly, one step's gradients against the reference-shaped
    eager step (render_train + regular_loss), and the regulariser's gradient on table rows no sample touched.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _reference_loss(x, c, alpha=1.0):
    """ClusteringLayer.forward + clustering_loss of the reference (gridencoder/grid_clustering.py:93-127)."""
    d2 = ((x.unsqueeze(1) - c) ** 2).sum(2)
    q = (1.0 / (1.0 + d2 / alpha)) ** (float(alpha + 1) / 2)
    q = q / q.sum(dim=1, keepdim=True)
    p = (q ** 2) / q.sum(0)
    p = (p / p.sum(dim=1, keepdim=True)).detach()
    return torch.nn.KLDivLoss(reduction="mean")(q.log(), p)


def _level(dev, v):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _step(emb, offsets, centres, level, weight=1.0, **kw):
    from gridencoder.grid_clustering import grid_cluster_step

    return grid_cluster_step(emb, offsets, centres, level, 1.0, weight, **kw)


# ------------------------------------------------------------------------------------------------------------------------ 1. the kernel
def test_kernel_matches_the_reference_fixture(dev):
    """The reference's own numbers (tests/golden/ref_host_pieces.npz): GridEncoder_clustering.clustering_loss(pick_level=False) of a 3-level
    table and ClusteringLayer.clustering_loss with K = 6.  Both sit at init scale, where the loss is fp32 rounding noise of the framework's
    op sequence: the kernel reproduces those roundings (correctly rounded logs, no contraction), hence rtol 1e-5."""
    h = np.load(os.path.join(GOLDEN, "ref_host_pieces.npz"))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    loss = _step(t(h["gc_emb"]), t(h["gc_offsets"]), t(h["gc_centers"]), _level(dev, -1))
    print("gc loss", float(loss), float(h["gc_loss_all"]))
    np.testing.assert_allclose(float(loss), float(h["gc_loss_all"]), rtol=1e-5)
    x = t(h["cl_x"])
    loss = _step(x, torch.tensor([0, x.shape[0]], dtype=torch.int32, device=dev), t(h["cl_centers"])[None].contiguous(), _level(dev, 0))
    print("cl loss", float(loss), float(h["cl_loss"]))
    np.testing.assert_allclose(float(loss), float(h["cl_loss"]), rtol=1e-5)


def _curved_table(dev, scale, seed=0):
    from gridencoder import GridEncoder_clustering

    torch.manual_seed(seed)
    enc = GridEncoder_clustering(input_dim=3, num_levels=8, level_dim=2, base_resolution=512, log2_hashmap_size=19, desired_resolution=1024,
                                 gridtype="hash", align_corners=True).to(dev)  # CurvedField's table: 8 levels of 2^19 rows x 2
    with torch.no_grad():
        enc.embeddings.uniform_(-scale, scale)
        for layer in enc.cluster_layers:
            layer.cluster_centers.uniform_(-scale, scale)
    centres = torch.stack([layer.cluster_centers.detach() for layer in enc.cluster_layers]).contiguous()
    return enc, centres


# measured on an MI355X, worst of the 8 levels: loss 4.5e-8 relative, table 5.7e-6 and centres 6.2e-7 of the largest entry
BAR_LEVEL = {"loss": 1e-6, "table": 1e-4, "centres": 1e-5}


def test_kernel_per_level_against_float64_autograd(dev):
    enc, centres = _curved_table(dev, 0.5)
    emb, off = enc.embeddings.detach(), enc.offsets
    assert emb.shape == (8 << 19, 2)
    offs = off.cpu().tolist()
    worst = {k: 0.0 for k in BAR_LEVEL}
    for lvl in range(8):
        gt, gc = torch.zeros_like(emb), torch.zeros_like(centres)
        loss = _step(emb, off, centres, _level(dev, lvl), weight=1.0, grad_table=gt, grad_centres=gc)
        x = emb[offs[lvl]:offs[lvl + 1]].double().requires_grad_(True)
        c = centres[lvl].double().requires_grad_(True)
        want = _reference_loss(x, c)
        want.backward()
        err = {"loss": abs(float(loss) - float(want)) / abs(float(want)),
               "table": float((gt[offs[lvl]:offs[lvl + 1]].double() - x.grad).abs().max() / x.grad.abs().max()),
               "centres": float((gc[lvl].double() - c.grad).abs().max() / c.grad.abs().max())}
        assert float(gt[:offs[lvl]].abs().max() if lvl else 0) == 0 and (gt[offs[lvl + 1]:] == 0).all()
        assert (gc[:lvl] == 0).all() and (gc[lvl + 1:] == 0).all()
        worst = {k: max(worst[k], err[k]) for k in err}
    print("cluster loss vs float64 autograd, worst level:", worst)
    assert all(worst[k] < BAR_LEVEL[k] for k in BAR_LEVEL), worst


def test_kernel_is_bitwise_reproducible_and_init_scale_is_finite(dev):
    enc, centres = _curved_table(dev, 0.5, seed=1)
    emb, off = enc.embeddings.detach(), enc.offsets
    outs = []
    for _ in range(2):
        gt, gc = torch.zeros_like(emb), torch.zeros_like(centres)
        loss = _step(emb, off, centres, _level(dev, 3), weight=1e-8, grad_table=gt, grad_centres=gc)
        outs.append((loss.clone(), gt, gc))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(_bits(a), _bits(b))
    # init scale (+-1e-4, the reference's reset_parameters and centre init): q = 1/K up to an ulp, p - q cancels and the reference's own gradient
    # is rounding noise of its fp32 ops -- nothing to compare the gradient against.  The loss is tiny, non-negative and finite, as is the gradient.
    enc, centres = _curved_table(dev, 1e-4, seed=2)
    emb, off = enc.embeddings.detach(), enc.offsets
    gt, gc = torch.zeros_like(emb), torch.zeros_like(centres)
    loss = _step(emb, off, centres, _level(dev, -1), weight=1.0, grad_table=gt, grad_centres=gc)
    assert torch.isfinite(loss) and 0 <= float(loss) < 1e-6 and torch.isfinite(gt).all() and torch.isfinite(gc).all()
    # a level out of range: NaN loss, no gradient
    gt2 = torch.zeros_like(emb)
    loss = _step(emb, off, centres, _level(dev, 8), grad_table=gt2)
    assert torch.isnan(loss) and (gt2 == 0).all()


# ------------------------------------------------------------------------------------------------------------------- 2. the gradient path
def test_autograd_function_equals_the_step_form(dev):
    from gridencoder.grid_clustering import grid_clustering_loss

    enc, centres = _curved_table(dev, 0.5, seed=3)
    emb, off = enc.embeddings, enc.offsets
    level, s = _level(dev, 5), 1024.0
    e = emb.detach().clone().requires_grad_(True)
    c = centres.clone().requires_grad_(True)
    loss = grid_clustering_loss(e, off, c, level, 1.0, 1e-2)
    (loss * s).backward()
    gt = torch.zeros_like(emb.detach())
    gc = torch.zeros_like(centres)
    scale = torch.tensor(s, dtype=torch.float32, device=dev)
    loss2 = _step(emb.detach(), off, centres, level, weight=1e-2, grad_table=gt, grad_centres=gc, grad_scale=scale)
    assert torch.equal(_bits(loss.detach()), _bits(loss2))
    assert torch.equal(_bits(e.grad), _bits(gt)) and torch.equal(_bits(c.grad), _bits(gc))
    assert float(gt.abs().max()) > 0
    # the step form ADDS into the level's rows and leaves every other row as it was, bit for bit
    base = torch.randn_like(gt)
    acc = base.clone()
    _step(emb.detach(), off, centres, level, weight=1e-2, grad_table=acc, grad_scale=scale)
    offs = off.cpu().tolist()
    lo, hi = offs[5], offs[6]
    assert torch.equal(_bits(acc[:lo]), _bits(base[:lo])) and torch.equal(_bits(acc[hi:]), _bits(base[hi:]))
    assert torch.equal(acc[lo:hi], base[lo:hi] + gt[lo:hi])
    # the device form on the encoder: centres stacked on the device, gradients reach the per-level parameters
    enc.zero_grad()
    enc.clustering_loss_device(level).backward()
    assert float(enc.cluster_layers[5].cluster_centers.grad.abs().max()) > 0 and enc.cluster_layers[4].cluster_centers.grad.abs().max() == 0


# ------------------------------------------------------------------------------------------------------------------------------ 3. capture
def test_step_form_captures_with_a_device_level(dev):
    from ngp_harness.streams import capture_section

    enc, centres = _curved_table(dev, 0.5, seed=4)
    emb, off = enc.embeddings.detach(), enc.offsets
    level = _level(dev, 0)
    gt, gc = torch.zeros_like(emb), torch.zeros_like(centres)
    loss = torch.zeros((), dtype=torch.float32, device=dev)
    scale = torch.tensor(8.0, device=dev)
    _step(emb, off, centres, level, weight=1e-3, loss=loss, grad_table=gt, grad_centres=gc, grad_scale=scale)  # (warm: the host copy of offsets)
    torch.cuda.synchronize()
    with capture_section():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            gt.zero_(), gc.zero_()
            _step(emb, off, centres, level, weight=1e-3, loss=loss, grad_table=gt, grad_centres=gc, grad_scale=scale)
    for lv in (2, 7, -1, 2):
        level.fill_(lv)
        g.replay()
        wt, wc = torch.zeros_like(emb), torch.zeros_like(centres)
        wl = _step(emb, off, centres, _level(dev, lv), weight=1e-3, grad_table=wt, grad_centres=wc, grad_scale=scale)
        assert torch.equal(_bits(loss), _bits(wl)) and torch.equal(_bits(gt), _bits(wt)) and torch.equal(_bits(gc), _bits(wc)), lv
    del g


# ------------------------------------------------------------------------------------------------------------------------------ 4-6. trainer
def _curved_renderer(dev, seed=0, like=None):
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer

    v, f = star_flower_mesh(n_lat=36, n_lon=72)
    torch.manual_seed(seed)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05).to(dev)
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    if like is not None:
        r.load_state_dict(like.state_dict())
        r.mean_density = like.mean_density
    else:
        with torch.no_grad():
            field.encoder.embeddings.uniform_(-0.5, 0.5)  # trained scale
            field.sigma_net.weights.mul_(3.0)
            for layer in field.encoder.cluster_layers:
                layer.cluster_centers.uniform_(-0.5, 0.5)
        with torch.autocast("cuda", dtype=torch.float16):
            r.update_extra_state_device()
    field.train()
    return field, r


def _rays(dev, n, k, seed=300):
    from ngp_harness import scene

    out = []
    for i in range(k):
        o, d = scene.train_batch(n, seed=seed + i, radius=1.6)
        out.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
    tgt = torch.rand(k, n, 3, generator=torch.Generator().manual_seed(seed)).to(dev) * 0.2 + 0.4
    return out, tgt


@pytest.mark.parametrize("k,ahead", [(1, False), (1, True), (4, True)], ids=["step", "step_ahead", "group4_ahead"])
def test_accelerated_curved_trainer_replays_the_eager_step(dev, k, ahead):
    from ngp_harness.accelerate import CurvedTrainer, accelerate

    N, n_calls = 2048, (56 if k == 1 else 14)
    rays, tgt = _rays(dev, N, 6)
    _, r0 = _curved_renderer(dev)

    def run(graph):
        field, r = _curved_renderer(dev, like=r0)
        tr = accelerate(r, graph=graph, perturb=False, steps_per_call=k)
        assert isinstance(tr, CurvedTrainer)
        np.random.seed(7)
        losses = []
        for i in range(n_calls):
            if k == 1:
                nxt = rays[(i + 1) % 6] if ahead else None
                losses.append(tr.step(*rays[i % 6], tgt[i % 6], next_rays=nxt).clone())
            else:
                idx = [(i * k + j) % 6 for j in range(k)]
                o = torch.stack([rays[j][0] for j in idx]).contiguous()
                d = torch.stack([rays[j][1] for j in idx]).contiguous()
                if i == 0 or not ahead:
                    cur = (o, d)
                nidx = [((i + 1) * k + j) % 6 for j in range(k)]
                nxt = (torch.stack([rays[j][0] for j in nidx]).contiguous(), torch.stack([rays[j][1] for j in nidx]).contiguous()) if ahead else None
                losses.append(tr.step_group(cur[0], cur[1], tgt[idx], next_rays=nxt).clone())
                if ahead:
                    cur = nxt
        torch.cuda.synchronize()
        return torch.stack(losses).cpu().numpy(), tr, field

    eager, _, fe = run(False)
    graphed, tr, fg = run(True)
    assert tr._graphs is not None, "the later steps ran as replayed graphs"
    assert np.isfinite(graphed).all() and graphed[-3:].mean() < graphed[:3].mean(), (graphed[:3], graphed[-3:])
    assert float(tr.reg_loss) > 0
    diffs = {n: float((a.detach().float() - b.detach().float()).abs().max()) for (n, a), (_, b) in zip(fg.named_parameters(), fe.named_parameters())}
    print("graph vs eager, max |diff| per parameter:", diffs, "losses equal:", np.array_equal(graphed, eager))
    for (n, a), (_, b) in zip(fg.named_parameters(), fe.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), n
    assert np.array_equal(graphed, eager)


def _one_step_grads(dev, weight, n=4096):
    """One training step of the accelerated trainer (eager launch of the same step the graphs record) and of the reference-shaped loop
    (render_train + MSE + weight * clustering_loss(), GradScaler, nerf/utils.py:637-666) on identical fields and the same level pick.
    -> (reference field, trainer's field, trainer, picked level, the reference's renderer: parameters as before the step)."""
    from ngp_harness.accelerate import accelerate

    rays, tgt = _rays(dev, n, 1, seed=500)
    fa, ra = _curved_renderer(dev)
    fb, rb = _curved_renderer(dev, like=ra)
    np.random.seed(11)
    tr = accelerate(rb, graph=False, perturb=False, regular_weight=weight)
    tr.step(*rays[0], tgt[0])
    level = int(tr.ring_levels[0])
    np.random.seed(11)
    scaler = torch.amp.GradScaler("cuda")
    with torch.autocast("cuda", dtype=torch.float16):
        image, depth, _ = ra.render_train(*rays[0], dt_gamma=1 / 128, bg_color=1, perturb=False, max_steps=1024)
        img_loss = ((image.float() - tgt[0]) ** 2).mean()
    loss = img_loss + weight * fa.encoder.clustering_loss()  # (the level: the reference's np.random.choice after the same seed)
    scaler.scale(loss).backward()
    scaler.unscale_(torch.optim.Adam(fa.parameters()))
    return fa, fb, tr, level, ra


def test_trainer_gradients_match_the_reference_shaped_step(dev):
    """One step's gradients, not parameters (Adam's sign-like update of near-zero gradients would amplify rounding), with the regulariser raised
    to 1e-2 so that it is not lost under the image loss's gradient."""
    fa, fb, tr, level, _ = _one_step_grads(dev, 1e-2)
    ga, gb = fa.encoder.embeddings.grad, fb.encoder.embeddings.grad
    err = {"table": float((ga - gb).abs().max() / ga.abs().max())}
    grad = lambda p: torch.zeros_like(p) if p.grad is None else p.grad  # noqa: E731  (the reference touches the picked level's centres only)
    ca = torch.stack([grad(layer.cluster_centers) for layer in fa.encoder.cluster_layers])
    cb = torch.stack([grad(layer.cluster_centers) for layer in fb.encoder.cluster_layers])
    err["centres"] = float((ca - cb).abs().max() / ca.abs().max())
    off = fa.encoder.offsets.cpu().tolist()
    rows = slice(off[level], off[level + 1])
    err["table, picked level"] = float((ga[rows] - gb[rows]).abs().max() / ga[rows].abs().max())
    print("trainer vs reference-shaped step, gradient errors (max |diff| / max |want|):", err, "level", level)
    assert float(ca[level].abs().max()) > 0
    assert err["table"] < 2e-2 and err["centres"] < 1e-3 and err["table, picked level"] < 2e-2, err


def test_the_regulariser_reaches_rows_no_sample_touched(dev):
    """With the reference's weight (1e-8), the regulariser's gradient on a table row of the picked level that no sample of the batch touched is
    what the standalone kernel gives, bit for bit (it reached Adam in fp32: through an fp16 gradient it would be zero); rows of the other levels
    that no sample touched have no gradient."""
    from ngp_harness.accelerate import accelerate

    weight = 1e-8
    fa, _, _, _, ra = _one_step_grads(dev, 0.0)  # fa.grad: the image loss's gradient alone -> the rows the batch touched
    touched = (fa.encoder.embeddings.grad != 0).any(1)
    fb, rb = _curved_renderer(dev, like=ra)
    rays, tgt = _rays(dev, 4096, 1, seed=500)
    np.random.seed(11)
    tr = accelerate(rb, graph=False, perturb=False, regular_weight=weight)
    tr.step(*rays[0], tgt[0])
    level = int(tr.ring_levels[0])
    table0 = ra.field.encoder.embeddings.detach()
    centres0 = torch.stack([layer.cluster_centers.detach() for layer in ra.field.encoder.cluster_layers]).contiguous()
    standalone = torch.zeros_like(table0)
    _step(table0, ra.field.encoder.offsets, centres0, _level(dev, level), weight=weight, grad_table=standalone)
    g = fb.encoder.embeddings.grad
    off = fb.encoder.offsets.cpu().tolist()
    in_level = torch.zeros(g.shape[0], dtype=torch.bool, device=dev)
    in_level[off[level]:off[level + 1]] = True
    free = in_level & ~touched
    assert int(free.sum()) > 1000 and int((~in_level & ~touched).sum()) > 1000
    assert float((g[free] != 0).any(1).float().mean()) > 0.99, "the regulariser's gradient survives on rows no ray touched"
    assert torch.equal(_bits(g[free]), _bits(standalone[free]))
    assert (g[~in_level & ~touched] == 0).all()
