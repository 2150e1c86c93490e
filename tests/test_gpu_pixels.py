"""Per-ray backgrounds and RGBA pixels on the fused training step: the four nerftex_*_px entries with a nerftex_step_pixels_desc, fused.render_tail
/ composite_tail with a tensor bg or an [N,4] target, accelerate(bg_color="random" | "given", target_channels=4).  Reference statements: the
reference's own torch expressions (nerf/utils.py:602-615, renderer.py:424) in float32 for what must be equal bit for bit, tests/test_pixels_cpu.py's
float64 statement and torch's float32 autograd for the rest.  Tolerances: those tests/test_gpu_criterion.py::test_criteria_match_torch holds the
same quantities to."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from test_gpu_criterion import _bits, _curved_renderer, _desc, _field_backward_args, _ngp_case
from test_pixels_cpu import pixels_float64

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
MSE, L1, HUBER = 0, 1, 2
CRITERIA = [("mse", MSE, 0.0), ("l1", L1, 0.0), ("huber0.1", HUBER, 0.1)]
MUL = 0.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


_CASES = {}


def _case(dev, N):
    """Ragged rays as tests/test_gpu_criterion.py::_ragged makes them, with the chunk edges pinned: an empty ray, rays of 1, 63, 64, 65 and 300
    samples (more than 64 * 4, the most chunks composite_step keeps), a last record that runs past M; backgrounds uniform in [0, 1), colours in
    (0, 1], alpha 0 on a third of the rays, 1 on a third, uniform in (0, 1) on the rest.  Made once per N, never modified."""
    if N not in _CASES:
        g = torch.Generator(device="cpu").manual_seed(4000 + N)
        counts = torch.randint(0, 150, (N,), generator=g)
        pinned = {1: [70], 3: [0, 300, 64]}.get(N, [0, 1, 63, 64, 65, 300])
        counts[:len(pinned)] = torch.tensor(pinned)
        offsets = torch.cumsum(counts, 0) - counts
        M = int(counts.sum()) + 8
        if N > 2:
            counts[-1] = counts[-1] + 9  # offset + count >= M: the record runs past the buffer, the ray composites nothing
        rays = torch.stack([torch.arange(N), offsets, counts], dim=1).to(torch.int32).to(dev)
        sigmas = (torch.rand(M, generator=g) * 30).to(dev)
        rgbs = torch.rand(M, 3, generator=g).to(dev)
        deltas = torch.stack([torch.rand(M, generator=g) * 0.02 + 0.003, torch.rand(M, generator=g) * 0.03 + 0.003], dim=1).to(dev)
        nears = (torch.rand(N, generator=g) + 0.2).to(dev)
        fars = nears + (torch.rand(N, generator=g) * 3 + 0.1).to(dev)
        bg = torch.rand(N, 3, generator=g)
        colour = 1.0 - torch.rand(N, 3, generator=g)
        alpha = torch.rand(N, generator=g) * (1 - 2 ** -10) + 2 ** -11  # inside (0, 1)
        which = torch.arange(N) % 3 if N > 1 else torch.tensor([2])
        alpha[which == 0], alpha[which == 1] = 0.0, 1.0
        rgba = torch.cat([colour, alpha[:, None]], 1).contiguous()
        assert float(colour.min()) > 0 and float(bg.max()) < 1 and (N < 3 or (int((alpha == 0).sum()) >= N // 3 and int((alpha == 1).sum()) >= N // 3))
        _CASES[N] = dict(rays=rays, sigmas=sigmas, rgbs=rgbs, deltas=deltas, nears=nears, fars=fars, bg=bg.to(dev), rgba=rgba.to(dev),
                         target=colour.to(dev).contiguous(), M=M, N=N, empty=(counts == 0).to(dev), past=((offsets + counts >= M) & (counts > 0)).to(dev))
    return _CASES[N]


def _pixels(bg, rgba=None, gt=None):
    from nerftex_hip import StepPixelsDesc, ptr

    return StepPixelsDesc(ptr(bg), ptr(rgba), ptr(gt))


def _three_launches(dev, c, scale, desc, how, bg=1.0, target=None, px=None):
    """Compositing forward, render tail, compositing backward with a root gradient of one.  how: "ex" (the _ex entries), "px" (the _px entries
    with `px`, None: NULL).  -> per-ray outputs [9, N], (loss, scaled loss), gradients [4 M], step flags."""
    from nerftex_hip import check, lib, ptr, stream

    M, N = c["M"], c["N"]
    by = None if desc is None else ctypes.byref(desc)
    one = torch.ones((), device=dev)
    per_ray = torch.full((9, N), float("nan"), device=dev)
    ws, depth, depth_out, image, image_out = per_ray[0], per_ray[1], per_ray[2], per_ray[3:6].view(N, 3), per_ray[6:9].view(N, 3)
    losses = torch.full((2,), float("nan"), device=dev)
    ticket, partial = torch.zeros(1, dtype=torch.int32, device=dev), torch.empty(1024, device=dev)
    words = (M + 31) // 32
    flags = torch.full((words,), 7, dtype=torch.int32, device=dev)
    g = torch.full((4 * M,), float("nan"), device=dev)
    check(lib.nerftex_composite_rays_train_forward(ptr(c["sigmas"]), ptr(c["rgbs"]), ptr(c["deltas"]), ptr(c["rays"]), M, N, ptr(ws), ptr(depth), ptr(image), stream()))
    fwd = (ptr(ws), ptr(depth), ptr(image), ptr(c["nears"]), ptr(c["fars"]), ptr(target), bg, MUL, N, ptr(image_out), ptr(depth_out), ptr(partial), ptr(ticket),
           ptr(losses), ptr(scale), losses.data_ptr() + 4, ptr(flags), words)
    bwd = (ptr(one), ptr(scale), MUL, ptr(image_out), ptr(target), bg, ptr(c["sigmas"]), ptr(c["rgbs"]), ptr(c["deltas"]), ptr(c["rays"]), ptr(ws), ptr(image), M, N,
           ptr(g[:M]), ptr(g[M:]), ptr(flags))
    if how == "ex":
        check(lib.nerftex_render_tail_forward_ex(*fwd, by, stream()))
        check(lib.nerftex_composite_tail_backward_ex(*bwd, by, stream()))
    else:
        pby = None if px is None else ctypes.byref(px)
        check(lib.nerftex_render_tail_forward_px(*fwd, by, pby, stream()))
        check(lib.nerftex_composite_tail_backward_px(*bwd, by, pby, stream()))
    assert int(ticket[0]) == 0
    return per_ray, losses, g, flags


def _one_launch(dev, c, scale, desc, how, bg=1.0, target=None, px=None, with_loss=True):
    from nerftex_hip import check, lib, ptr, stream

    M, N = c["M"], c["N"]
    per_ray = torch.full((9, N), float("nan"), device=dev)
    ws, depth, depth_out, image, image_out = per_ray[0], per_ray[1], per_ray[2], per_ray[3:6].view(N, 3), per_ray[6:9].view(N, 3)
    losses = torch.full((2,), float("nan"), device=dev)
    err = torch.full((N,), float("nan"), device=dev)
    flags = torch.zeros((M + 31) // 32, dtype=torch.int32, device=dev)
    g = torch.full((4 * M,), float("nan"), device=dev)
    args = (ptr(c["sigmas"]), ptr(c["rgbs"]), ptr(c["deltas"]), ptr(c["rays"]), M, N, ptr(c["nears"]), ptr(c["fars"]), ptr(target), bg, MUL, ptr(scale), ptr(ws),
            ptr(depth), ptr(image), ptr(image_out), ptr(depth_out), ptr(err), ptr(losses) if with_loss else None, losses.data_ptr() + 4 if with_loss else None,
            ptr(g[:M]), ptr(g[M:]), ptr(flags))
    by = None if desc is None else ctypes.byref(desc)
    if how == "ex":
        check(lib.nerftex_composite_step_ex(*args, by, stream()))
    else:
        check(lib.nerftex_composite_step_px(*args, by, None if px is None else ctypes.byref(px), stream()))
    return per_ray, losses, g, flags, err


def _tail_backward(dev, c, scale, desc, how, image_out, gl, bg=1.0, target=None, px=None):
    """The stand-alone backward of the render tail -> grad_image [N,3], grad_weights_sum [N]."""
    from nerftex_hip import check, lib, ptr, stream

    N = c["N"]
    gi, gw = torch.full((N, 3), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)
    args = (ptr(gl), ptr(scale), MUL, ptr(image_out), ptr(target), bg, N, ptr(gi), ptr(gw))
    by = None if desc is None else ctypes.byref(desc)
    if how == "ex":
        check(lib.nerftex_render_tail_backward_ex(*args, by, stream()))
    else:
        check(lib.nerftex_render_tail_backward_px(*args, by, None if px is None else ctypes.byref(px), stream()))
    return gi, gw


def _same(a, b, what):
    names = ("per-ray outputs", "loss, scaled loss", "gradients")
    for x, y, n in zip(a[:3], b[:3], names):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: {n}"
    assert torch.equal(a[3] != 0, b[3] != 0), f"{what}: step flags"


# ------------------------------------------------------------------------------------------------- 1. NULL pixels: the _ex entry
@pytest.mark.parametrize("name,kind", [("mse", None), ("l1", L1)])
@pytest.mark.parametrize("N", [3, 1000])
def test_px_entries_without_pixels_are_the_ex_entries(dev, N, name, kind):
    """Each _px entry with a NULL pixels descriptor against the _ex entry it extends (scalar bg 0.75, with a loss scale): every output, the loss,
    the gradients, the step flags, err[], the rays' losses and the stand-alone tail backward, bit for bit."""
    c = _case(dev, N)
    scale = torch.full((), 1024.0, device=dev)
    rl = {h: torch.full((2, N), float("nan"), device=dev) for h in ("ex", "px")}
    desc = lambda h, i: None if kind is None else _desc(kind, 0.0, rl[h][i])  # noqa: E731
    old3 = _three_launches(dev, c, scale, desc("ex", 0), "ex", bg=0.75, target=c["target"])
    new3 = _three_launches(dev, c, scale, desc("px", 0), "px", bg=0.75, target=c["target"])
    assert float(old3[2][:c["M"]].abs().max()) > 0 and torch.isfinite(old3[1]).all()
    _same(old3, new3, "three launches")
    old1 = _one_launch(dev, c, scale, desc("ex", 1), "ex", bg=0.75, target=c["target"])
    new1 = _one_launch(dev, c, scale, desc("px", 1), "px", bg=0.75, target=c["target"])
    _same(old1, new1, "one launch")
    assert torch.equal(_bits(old1[4]), _bits(new1[4])), "err[]"
    if kind is not None:
        assert torch.isfinite(rl["ex"]).all() and torch.equal(_bits(rl["ex"]), _bits(rl["px"])), "ray_loss"
    image_out, gl = old3[0][6:9].view(N, 3).contiguous(), torch.full((), 3.0, device=dev)
    a = _tail_backward(dev, c, scale, desc("ex", 0), "ex", image_out, gl, bg=0.75, target=c["target"])
    b = _tail_backward(dev, c, scale, desc("px", 0), "px", image_out, gl, bg=0.75, target=c["target"])
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1])), "render_tail_backward"


# ------------------------------------------------------------------------------------------------- 2. against torch
@pytest.mark.parametrize("name,kind,param", CRITERIA, ids=[c[0] for c in CRITERIA])
@pytest.mark.parametrize("N", [1, 3, 257, 1000])
def test_pixels_match_torch(dev, N, name, kind, param):
    """The three-launch form with RGBA pixels over per-ray backgrounds.  target_out and image_out: the reference's float32 torch expressions, bit
    for bit (a == 0: the background; a == 1: the colour; an empty or cut-off ray's image: its background).  loss: within 1e-5 relative of
    float64 (a tree of at most 20 roundings over non-negative terms plus at most seven per element -- the two blends and the criterion --: under
    40 * 2^-24 = 2.4e-6).  grad_image: within 4 * 2^-24 relative of torch's float32 autograd (the difference, one multiply and one division may
    round differently).  grad_weights_sum: rtol 1e-5 / atol 1e-7 against torch's autograd, the bar of test_criteria_match_torch for the same
    three-term sum (root gradient one: the terms are below 1 / 3N * 0.5, their roundings below 2^-25 of that)."""
    c = _case(dev, N)
    bg, rgba = c["bg"], c["rgba"]
    gt = torch.full((N, 3), float("nan"), device=dev)
    rl = torch.full((N,), float("nan"), device=dev)
    px = _pixels(bg, rgba, gt)
    out = _three_launches(dev, c, None, _desc(kind, param, rl), "px", px=px)
    ws, image, image_out = out[0][0], out[0][3:6].view(N, 3), out[0][6:9].view(N, 3)
    gt_torch = rgba[..., :3] * rgba[..., 3:] + bg * (1 - rgba[..., 3:])  # nerf/utils.py:604
    ws1, im1 = ws.clone().requires_grad_(True), image.clone().requires_grad_(True)
    image_torch = im1 + (1 - ws1).unsqueeze(-1) * bg  # renderer.py:424
    assert torch.equal(_bits(gt), _bits(gt_torch)), "target_out"
    assert torch.equal(_bits(image_out), _bits(image_torch.detach())), "image_out"
    a = rgba[:, 3]
    assert torch.equal(_bits(gt[a == 0]), _bits(bg[a == 0])) and torch.equal(_bits(gt[a == 1]), _bits(rgba[a == 1, :3]))
    blank = c["empty"] | c["past"]
    assert torch.equal(_bits(image_out[blank]), _bits(bg[blank])) and (N < 3 or (bool(c["empty"].any()) and bool(c["past"].any())))
    ref = pixels_float64(image, ws, bg, rgba=rgba, kind=kind, param=param, loss_mul=MUL)
    want = float(ref["loss"])
    print(f"N {N} {name}: loss {out[1][0].item():.9g} float64 {want:.9g} rel {abs(out[1][0].item() - want) / want:.3g}")
    assert abs(out[1][0].item() - want) <= 1e-5 * want and out[1][1].item() == out[1][0].item()
    assert torch.isfinite(rl).all()
    # torch's float32 backward of the same criterion, root gradient one
    crit = {MSE: F.mse_loss, L1: F.l1_loss, HUBER: lambda x, y: F.huber_loss(x, y, delta=param)}[kind]
    (crit(image_torch, gt_torch) * MUL).backward()
    gl = torch.ones((), device=dev)
    gi, gw = _tail_backward(dev, c, None, _desc(kind, param), "px", image_out.contiguous(), gl, px=px)  # (with rgba: target_out is its target)
    rel = ((gi - im1.grad).abs() / im1.grad.abs().clamp_min(1e-30)).max().item()
    print(f"N {N} {name}: grad_image max rel {rel / EPS:.3g} * 2^-24, grad_ws max abs diff {(gw - ws1.grad).abs().max().item():.3g}")
    assert ((gi - im1.grad).abs() <= 4 * EPS * im1.grad.abs()).all()
    torch.testing.assert_close(gw, ws1.grad, rtol=1e-5, atol=1e-7)
    # the same backward with the blended target handed over as `target` (no rgba): the same bits
    gi2, gw2 = _tail_backward(dev, c, None, _desc(kind, param), "px", image_out.contiguous(), gl, target=gt, px=_pixels(bg))
    assert torch.equal(_bits(gi), _bits(gi2)) and torch.equal(_bits(gw), _bits(gw2))
    # and fused.render_tail, the autograd node over the two entries: a tensor bg and an [N,4] target, the blended target as a fifth output
    from ngp_harness import fused

    ws2, im2 = ws.clone().requires_grad_(True), image.clone().requires_grad_(True)
    criterion = {MSE: "mse", L1: "l1", HUBER: ("huber", param)}[kind]
    img, _, loss, scaled, gt2 = fused.render_tail(ws2, out[0][1], im2, c["nears"], c["fars"], rgba, bg, MUL, criterion=criterion)
    scaled.backward(gl)
    assert torch.equal(_bits(img), _bits(image_out)) and torch.equal(_bits(gt2), _bits(gt)) and loss.item() == out[1][0].item()
    assert torch.equal(_bits(im2.grad), _bits(gi)) and torch.equal(_bits(ws2.grad), _bits(gw))


# ------------------------------------------------------------------------------------------------- 3. one launch equals three launches
@pytest.mark.parametrize("name,kind,param", CRITERIA, ids=[c[0] for c in CRITERIA])
@pytest.mark.parametrize("N", [3, 1000])
def test_one_launch_equals_three_launches_with_pixels(dev, knobs, N, name, kind, param):
    """nerftex_composite_step_px against the three _px launches, for every number of kept chunks, with and without a loss scale: outputs, loss,
    gradients, step flags, the blended target, err[], the per-ray loss and the error map bit for bit -- and the deferred loss (loss = NULL:
    err[] finished by nerftex_field_backward_live_consume, or by the trailer of nerftex_field_backward_live_deferred run as a launch of its
    own).  The structure of tests/test_gpu_criterion.py::test_one_launch_equals_three_launches_per_criterion."""
    from nerftex_hip import StepLoss, StepTrailer, check, lib, ptr, stream

    c = _case(dev, N)
    R = 4096
    gen = torch.Generator(device="cpu").manual_seed(77 + N)
    prefill = torch.rand(R, generator=gen).to(dev)
    inds = torch.randperm(R, generator=gen)[:N].to(dev)
    inds[0] = -1
    core, B, _keepalive = _field_backward_args(dev)
    for scale in (None, torch.full((), 1024.0, device=dev)):
        rl3, map3, gt3 = torch.full((N,), float("nan"), device=dev), prefill.clone(), torch.full((N, 3), float("nan"), device=dev)
        three = _three_launches(dev, c, scale, _desc(kind, param, rl3, map3, inds), "px", px=_pixels(c["bg"], c["rgba"], gt3))
        assert torch.isfinite(rl3).all() and torch.isfinite(gt3).all() and not torch.equal(map3, prefill)
        assert float(three[2][:c["M"]].abs().max()) > 0 and torch.isfinite(three[1]).all()
        for keep in (0, 1, 3, 4):
            knobs(composite_keep=keep)
            rl1, map1, gt1 = torch.full((N,), float("nan"), device=dev), prefill.clone(), torch.full((N, 3), float("nan"), device=dev)
            one = _one_launch(dev, c, scale, _desc(kind, param, rl1, map1, inds), "px", px=_pixels(c["bg"], c["rgba"], gt1))
            _same(three, one, f"{name}, keep {keep}")
            assert torch.equal(_bits(gt3), _bits(gt1)), f"{name}, keep {keep}: the blended target"
            assert torch.equal(_bits(rl3), _bits(rl1)) and torch.equal(_bits(map3), _bits(map1)), f"{name}, keep {keep}: ray_loss / map"
        # without rgba (a tensor background over a plain [N,3] target): the same, against each other
        three_bg = _three_launches(dev, c, scale, _desc(kind, param), "px", target=c["target"], px=_pixels(c["bg"]))
        one_bg = _one_launch(dev, c, scale, _desc(kind, param), "px", target=c["target"], px=_pixels(c["bg"]))
        _same(three_bg, one_bg, f"{name}: background only")
        # the deferred loss: the same err[], finished elsewhere
        rl2, map2, gt2 = torch.full((N,), float("nan"), device=dev), prefill.clone(), torch.full((N, 3), float("nan"), device=dev)
        deferred = _one_launch(dev, c, scale, _desc(kind, param, rl2, map2, inds), "px", px=_pixels(c["bg"], c["rgba"], gt2), with_loss=False)
        assert torch.equal(_bits(deferred[4]), _bits(one[4])) and torch.isnan(deferred[1]).all() and torch.equal(_bits(gt2), _bits(gt3))
        got = torch.full((2,), float("nan"), device=dev)
        job = StepLoss(ptr(deferred[4]), N, MUL, ptr(scale), ptr(got), got.data_ptr() + 4)
        flags = torch.ones(B // 32, dtype=torch.int32, device=dev)
        check(lib.nerftex_field_backward_live_consume(*core, ptr(flags), ctypes.byref(job), None, stream()))
        assert torch.equal(_bits(got), _bits(three[1])), f"{name}: loss finished by the field backward {got.tolist()} {three[1].tolist()}"
        got2, trailer = torch.full((2,), float("nan"), device=dev), StepTrailer()
        job = StepLoss(ptr(deferred[4]), N, MUL, ptr(scale), ptr(got2), got2.data_ptr() + 4)
        flags.fill_(1)
        check(lib.nerftex_field_backward_live_deferred(*core, ptr(flags), ctypes.byref(job), None, ctypes.byref(trailer), stream()))
        check(lib.nerftex_step_trailer_run(ctypes.byref(trailer), stream()))
        assert torch.equal(_bits(got2), _bits(three[1])), f"{name}: loss finished by the trailer launch"


# ------------------------------------------------------------------------------------------------- 4. the constant case is today's step
@pytest.mark.parametrize("name,kind", [("mse", None), ("l1", L1), ("huber0.1", HUBER)])
@pytest.mark.parametrize("N", [3, 1000])
def test_ones_and_opaque_pixels_are_the_scalar_step(dev, N, name, kind):
    """bg_rays == 1 and rgba = (rgb, 1) with rgb > 0 through the four _px entries against the scalar bg = 1 _ex calls on target = rgb: every
    output bit for bit (gt = rgb * 1 + 1 * 0; the blend's (1 - ws) * 1; -(gi0 * 1 + gi1 * 1 + gi2 * 1) for -(sum * 1))."""
    c = _case(dev, N)
    rgb = c["target"]
    ones = torch.ones(N, 3, device=dev)
    opaque = torch.cat([rgb, torch.ones(N, 1, device=dev)], 1).contiguous()
    param = 0.1 if kind == HUBER else 0.0
    scale = torch.full((), 1024.0, device=dev)
    rl = torch.full((4, N), float("nan"), device=dev)
    desc = lambda i: None if kind is None else _desc(kind, param, rl[i])  # noqa: E731
    gt3, gt1 = torch.full((N, 3), float("nan"), device=dev), torch.full((N, 3), float("nan"), device=dev)
    old3 = _three_launches(dev, c, scale, desc(0), "ex", bg=1.0, target=rgb)
    new3 = _three_launches(dev, c, scale, desc(1), "px", px=_pixels(ones, opaque, gt3))
    _same(old3, new3, "three launches")
    old1 = _one_launch(dev, c, scale, desc(2), "ex", bg=1.0, target=rgb)
    new1 = _one_launch(dev, c, scale, desc(3), "px", px=_pixels(ones, opaque, gt1))
    _same(old1, new1, "one launch")
    assert torch.equal(_bits(old1[4]), _bits(new1[4])), "err[]"
    assert torch.equal(_bits(gt3), _bits(rgb)) and torch.equal(_bits(gt1), _bits(rgb)), "the blended target is the colour"
    if kind is not None:
        assert torch.isfinite(rl).all() and torch.equal(_bits(rl[0]), _bits(rl[1])) and torch.equal(_bits(rl[2]), _bits(rl[3])), "ray_loss"
    image_out, gl = old3[0][6:9].view(N, 3).contiguous(), torch.full((), 3.0, device=dev)
    a = _tail_backward(dev, c, scale, desc(0), "ex", image_out, gl, bg=1.0, target=rgb)
    b = _tail_backward(dev, c, scale, desc(1), "px", image_out, gl, px=_pixels(ones, opaque, gt3))
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1])), "render_tail_backward"


# ------------------------------------------------------------------------------------------------- 5. the trainer, ngp field
_PIXELS = {}


def _rgba_case(dev):
    """RGBA targets of the analytic scene for the 8 ray batches of tests/test_gpu_criterion.py::_ngp_case (scene.render_targets with the rays'
    opacity: premultiplied colours over opacity), and 8 given backgrounds.  Made once."""
    if not _PIXELS:
        from ngp_harness import scene

        s = _ngp_case(dev)
        sc = scene.Scene(bound=2.0, seed=0)
        rgba = []
        for o, d in s["rays"]:
            pre, a = scene.render_targets(sc, o, d, n_samples=128, bg=0.0, opacity=True)
            a = a.clamp(0, 1)
            rgba.append(torch.cat([(pre / a.clamp_min(1e-6)[:, None]).clamp(0, 1), a[:, None]], 1))
        _PIXELS["rgba"] = torch.stack(rgba).contiguous()
        _PIXELS["bg"] = torch.rand(8, 2048, 3, generator=torch.Generator().manual_seed(11)).to(dev)
        assert 0.05 < float(_PIXELS["rgba"][..., 3].mean()) < 0.95, "the rays both hit and miss the scene"
    return _PIXELS


def _ngp_trainer(dev, mlp_dtype=torch.float16, **kw):
    """The trainer of tests/test_gpu_criterion.py::_ngp_trainer; mlp_dtype bfloat16: over the bf16 field."""
    from ngp_harness.accelerate import accelerate
    from ngp_harness.model import NGPField, Renderer

    torch.manual_seed(0)
    field = NGPField(bound=2.0, mlp="ffmlp", fused_glue=True, mlp_dtype=mlp_dtype).to(dev)
    torch.manual_seed(1)
    field.encoder.embeddings.data.uniform_(-1e-4, 1e-4)
    r = Renderer(field, bound=2.0, min_near=0.2, density_thresh=10.0).to(dev)
    r.set_occupancy(_ngp_case(dev)["grid"])
    field.train()
    return field, accelerate(r, perturb=False, **kw)


def _train(dev, calls, k=1, ahead=False, targets=None, bgs=None, overflow_at=None, seed=None, **kw):
    """`calls` calls of k steps each over the 8 batches of rays, targets [8, 2048, C] and (bg_color="given") backgrounds [8, 2048, 3]
    -> dict(params after sync(), losses, ray_loss, map, trainer, per-call gt_rgb / last_bg, notes)."""
    s = _ngp_case(dev)
    emap = torch.full((8, 2048), 0.5, device=dev)
    if seed is not None:
        kw["bg_generator"] = torch.Generator(device=dev).manual_seed(seed)
    field, tr = _ngp_trainer(dev, steps_per_call=k, error_map=emap, criterion="l1", **kw)
    losses, gts, last_bgs, notes = [], [], [], {}

    def batch(i):
        idx = [(i * k + j) % 8 for j in range(k)]
        o = torch.stack([s["rays"][j][0] for j in idx]).contiguous()
        d = torch.stack([s["rays"][j][1] for j in idx]).contiguous()
        return o, d, targets[idx].contiguous(), s["inds"][idx].contiguous(), None if bgs is None else bgs[idx].contiguous()

    cur = batch(0)
    for i in range(calls):
        nxt = batch(i + 1)
        if overflow_at == i:
            tr.sync()
            notes["before"] = ({n: p.detach().clone() for n, p in field.named_parameters()}, emap.clone(), float(tr.opt.step_count))
            tr.amp.scale.fill_(2.0 ** 40)
            if tr._gt is not None:
                tr._gt.fill_(-1.0)  # (every ring slot: the step must write its own)
        more = {} if cur[4] is None else {"bg": cur[4] if k > 1 else cur[4][0]}
        if k > 1:
            tr.step_group(cur[0], cur[1], cur[2], next_rays=(nxt[0], nxt[1]) if ahead else None, error_inds=cur[3], **more)
        else:
            tr.step(cur[0][0], cur[1][0], cur[2][0], next_rays=(nxt[0][0], nxt[1][0]) if ahead else None, error_inds=cur[3][0], **more)
        if overflow_at == i:
            tr.sync()
            notes["after"] = ({n: p.detach().clone() for n, p in field.named_parameters()}, emap.clone(), float(tr.opt.step_count))
        losses.append(tr.loss.clone())
        gts.append(None if tr.gt_rgb is None else tr.gt_rgb.clone())
        last_bgs.append(None if tr.last_bg is None else tr.last_bg.clone())
        cur = nxt
    torch.cuda.synchronize()
    tr.sync()
    params = {n: p.detach().clone() for n, p in field.named_parameters()}
    return dict(params=params, losses=torch.stack(losses), ray_loss=tr.ray_loss.clone(), map=emap, tr=tr, gts=gts, bgs=last_bgs, notes=notes)


def _equal_runs(a, b, what, every=1):
    for n in a["params"]:
        assert torch.equal(a["params"][n], b["params"][n]), f"{what}: parameter {n}"
    assert torch.equal(_bits(a["losses"][every - 1::every]), _bits(b["losses"])), f"{what}: losses"
    assert torch.equal(_bits(a["ray_loss"]), _bits(b["ray_loss"])), f"{what}: ray_loss"
    assert torch.equal(_bits(a["map"]), _bits(b["map"])), f"{what}: error map"


STEPS = 24


def test_given_ones_and_opaque_pixels_train_like_the_default_trainer(dev):
    """(a) bg_color="given" with all-ones backgrounds and alpha 1 against accelerate(renderer) as it was: parameters, losses, ray_loss and the
    map bit for bit over 24 steps, the later ones replayed graphs; the default trainer builds no descriptor and no buffer."""
    rgb = _ngp_case(dev)["tgt"]
    plain = _train(dev, STEPS, targets=rgb)
    tr = plain["tr"]
    assert tr._graphs is not None and tr._bg is None and tr._gt is None and tr.gt_rgb is None and tr.last_bg is None and "target_out" not in tr._loss_args(0)
    assert tr._targets.shape == (16, 2048, 3) and tr._bg_arg(0) == 1
    opaque = torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1).contiguous()
    given = _train(dev, STEPS, targets=opaque, bgs=torch.ones_like(rgb), bg_color="given", target_channels=4)
    assert given["tr"]._graphs is not None and given["tr"]._targets.shape == (16, 2048, 4)
    _equal_runs(plain, given, "given ones, alpha 1")
    assert torch.equal(_bits(given["gts"][-1]), _bits(rgb[(STEPS - 1) % 8])) and float(given["bgs"][-1].min()) == 1.0


@pytest.fixture(scope="module")
def random_graphed(dev):
    return _train(dev, STEPS, targets=_rgba_case(dev)["rgba"], bg_color="random", target_channels=4, seed=1234)


def test_random_backgrounds_replayed_equal_eager(dev, random_graphed):
    """(b) bg_color="random" with a seeded generator: the replayed graphs against graph=False with the same seed, parameters and losses bit for
    bit; last_bg is what torch.rand with that generator yields, call by call; gt_rgb is the torch blend of the batch over it, bitwise.
    (f) and it trains: RGBA targets of the analytic scene, the mean loss of the last 4 steps below that of the first 4."""
    rgba = _rgba_case(dev)["rgba"]
    eager = _train(dev, STEPS, targets=rgba, bg_color="random", target_channels=4, seed=1234, graph=False)
    assert random_graphed["tr"]._graphs is not None and eager["tr"]._graphs is None, "steps 19.. ran as replayed graphs"
    _equal_runs(random_graphed, eager, "graph=True against graph=False")
    gen = torch.Generator(device=dev).manual_seed(1234)
    for i in range(STEPS):
        bg = torch.rand((1, 2048, 3), generator=gen, device=dev)[0]
        px = rgba[i % 8]
        for run in (random_graphed, eager):
            assert torch.equal(_bits(run["bgs"][i]), _bits(bg)), f"step {i}: last_bg"
            assert torch.equal(_bits(run["gts"][i]), _bits(px[:, :3] * px[:, 3:] + bg * (1 - px[:, 3:]))), f"step {i}: gt_rgb"
    losses = random_graphed["losses"]
    print("losses", [round(v, 5) for v in losses.tolist()])
    assert float(losses[-4:].mean()) < float(losses[:4].mean()), "it trains"


@pytest.fixture(scope="module")
def given_single(dev):
    p = _rgba_case(dev)
    return _train(dev, STEPS, targets=p["rgba"], bgs=p["bg"], bg_color="given", target_channels=4)


def test_groups_of_four_with_given_backgrounds(dev, given_single):
    """(c) steps_per_call=4: six step_group calls against 24 single steps, "given" backgrounds and RGBA targets, bit for bit."""
    p = _rgba_case(dev)
    grouped = _train(dev, STEPS // 4, k=4, targets=p["rgba"], bgs=p["bg"], bg_color="given", target_channels=4)
    assert grouped["tr"]._groups is not None and given_single["tr"]._graphs is not None
    _equal_runs(given_single, grouped, "step_group", every=4)
    assert torch.equal(_bits(grouped["gts"][-1]), _bits(given_single["gts"][-1])) and torch.equal(_bits(grouped["bgs"][-1]), _bits(p["bg"][(STEPS - 1) % 8]))
    px, bg = p["rgba"][(STEPS - 1) % 8], p["bg"][(STEPS - 1) % 8]
    assert torch.equal(_bits(grouped["gts"][-1]), _bits(px[:, :3] * px[:, 3:] + bg * (1 - px[:, 3:])))


def test_next_rays_with_given_backgrounds(dev, given_single):
    """(d) the same training with the next batch marched ahead."""
    p = _rgba_case(dev)
    ahead = _train(dev, STEPS, ahead=True, targets=p["rgba"], bgs=p["bg"], bg_color="given", target_channels=4)
    assert ahead["tr"]._side is not None, "a march ran ahead"
    _equal_runs(given_single, ahead, "next_rays")


def test_a_skipped_step_still_writes_the_target_and_the_map(dev):
    """(e) a forced overflow inside the replayed part (tests/test_gpu_criterion.py::test_a_skipped_step_still_updates_the_map): parameters and the
    optimizer's step count unchanged; gt_rgb (overwritten with -1 before the call) and the map's cells are written all the same."""
    p = _rgba_case(dev)
    at = 21
    out = _train(dev, STEPS, targets=p["rgba"], bgs=p["bg"], bg_color="given", target_channels=4, overflow_at=at)
    (p0, m0, s0), (p1, m1, s1) = out["notes"]["before"], out["notes"]["after"]
    assert out["tr"]._graphs is not None and s1 == s0, "the step was skipped"
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n
    px, bg = p["rgba"][at % 8], p["bg"][at % 8]
    assert torch.equal(_bits(out["gts"][at]), _bits(px[:, :3] * px[:, 3:] + bg * (1 - px[:, 3:]))), "gt_rgb of the skipped step"
    cells = _ngp_case(dev)["inds"][at % 8]
    assert not torch.equal(m0.view(-1)[cells], m1.view(-1)[cells]) and float((m0 != m1).sum()) <= 2048


# ------------------------------------------------------------------------------------------------- 7. bf16
def test_random_backgrounds_bf16(dev):
    """One case of (b) with amp_dtype=torch.bfloat16 (bf16 networks over the fp16 table): replayed against eager, bit for bit."""
    rgba = _rgba_case(dev)["rgba"]
    kw = dict(targets=rgba, bg_color="random", target_channels=4, seed=99, amp_dtype=torch.bfloat16, mlp_dtype=torch.bfloat16)
    graphed, eager = _train(dev, STEPS, **kw), _train(dev, STEPS, graph=False, **kw)
    assert graphed["tr"]._graphs is not None and graphed["tr"].field.fused_field_bf16 and graphed["tr"].fused, "the bf16 field on the fused AMP step"
    _equal_runs(graphed, eager, "bf16: graph=True against graph=False")
    assert torch.equal(_bits(graphed["bgs"][-1]), _bits(eager["bgs"][-1])) and torch.equal(_bits(graphed["gts"][-1]), _bits(eager["gts"][-1]))
    assert torch.isfinite(graphed["losses"]).all()


# ------------------------------------------------------------------------------------------------- 6. the curved field
def test_curved_trainer_with_random_backgrounds_and_rgba(dev):
    """main.py's configuration: CurvedTrainer, criterion="l1", target_channels=4, bg_color="random", regular_weight=1e-8 -- replayed against eager
    over the same 24 steps, bit for bit (losses, parameters, ray_loss, gt_rgb, last_bg)."""
    from ngp_harness import scene
    from ngp_harness.accelerate import CurvedTrainer, accelerate

    N = 2048
    rays = []
    for i in range(6):
        o, d = scene.train_batch(N, seed=300 + i, radius=1.6)
        rays.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
    g = torch.Generator().manual_seed(301)
    rgba = torch.cat([torch.rand(6, N, 3, generator=g) * 0.2 + 0.4, (torch.rand(6, N, 1, generator=g) * 3 - 1).clamp(0, 1)], -1).to(dev).contiguous()
    _, r0 = _curved_renderer(dev)

    def run(graph):
        field, r = _curved_renderer(dev, like=r0)
        tr = accelerate(r, graph=graph, perturb=False, criterion="l1", target_channels=4, bg_color="random", regular_weight=1e-8,
                        bg_generator=torch.Generator(device=dev).manual_seed(5))
        assert isinstance(tr, CurvedTrainer)
        np.random.seed(7)
        losses = [tr.step(*rays[i % 6], rgba[i % 6]).clone() for i in range(STEPS)]
        torch.cuda.synchronize()
        return torch.stack(losses), tr, field

    eager, graphed = run(False), run(True)
    assert graphed[1]._graphs is not None and eager[1]._graphs is None, "the later steps ran as replayed graphs"
    assert torch.isfinite(graphed[0]).all() and torch.equal(_bits(eager[0]), _bits(graphed[0])), "losses"
    for (n, a), (_, b) in zip(graphed[2].named_parameters(), eager[2].named_parameters()):
        assert torch.equal(a.detach(), b.detach()), n
    for name in ("ray_loss", "gt_rgb", "last_bg"):
        assert torch.equal(_bits(getattr(eager[1], name)), _bits(getattr(graphed[1], name))), name
    px, bg = rgba[(STEPS - 1) % 6], graphed[1].last_bg
    assert torch.equal(_bits(graphed[1].gt_rgb), _bits(px[:, :3] * px[:, 3:] + bg * (1 - px[:, 3:]))) and 0 <= float(bg.min()) and float(bg.max()) < 1
