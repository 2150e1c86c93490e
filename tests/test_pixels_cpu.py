"""CPU: per-ray backgrounds and RGBA pixels on the fused training step (nerftex_*_px with a nerftex_step_pixels_desc; accelerate(bg_color=,
target_channels=, bg_generator=)) -- the descriptor's layout, what the C entries and the trainers refuse and when (before anything is launched, so
no GPU is needed to see them refuse), and the float64 statement of the step's arithmetic that tests/test_gpu_pixels.py compares against."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

from ngp_harness.accelerate import AcceleratedTrainer, CurvedTrainer

MSE, L1, HUBER = 0, 1, 2


def pixels_float64(image, weights_sum, bg, rgba=None, target=None, kind=MSE, param=0.0, loss_mul=1.0, grad_loss=1.0):
    """The reference's train_step around the renderer (nerf/utils.py:602-615, renderer.py:424) in float64:
        gt = rgb * a + bg * (1 - a)   (or the given [N,3] target);   image_out = image + (1 - weights_sum)[:, None] * bg
        loss = criterion(image_out, gt) * loss_mul;   grad_image, grad_weights_sum = d (loss * grad_loss) / d (image, weights_sum)
    bg and alpha are constants (no gradient reaches them).  -> dict of float64 tensors: gt, image_out, loss, ray_loss, grad_image, grad_ws."""
    assert (rgba is None) != (target is None)
    image = image.detach().double().clone().requires_grad_(True)
    ws = weights_sum.detach().double().clone().requires_grad_(True)
    bg = bg.detach().double()
    if rgba is not None:
        rgba = rgba.detach().double()
        gt = rgba[..., :3] * rgba[..., 3:] + bg * (1 - rgba[..., 3:])
    else:
        gt = target.detach().double()
    image_out = image + (1 - ws).unsqueeze(-1) * bg
    crit = {MSE: F.mse_loss, L1: F.l1_loss, HUBER: lambda a, b, reduction: F.huber_loss(a, b, reduction=reduction, delta=param)}[kind]
    elements = crit(image_out, gt, reduction="none")
    loss = elements.mean() * loss_mul
    (loss * grad_loss).backward()
    return dict(gt=gt, image_out=image_out.detach(), loss=loss.detach(), ray_loss=elements.detach().mean(-1), grad_image=image.grad, grad_ws=ws.grad)


def test_descriptor_layouts():
    import nerftex_hip

    px = nerftex_hip.StepPixelsDesc(8, 16, 24)
    assert ctypes.sizeof(px) == 24 and (px.bg_rays, px.rgba, px.target_out) == (8, 16, 24)  # three pointers
    assert [f[0] for f in nerftex_hip.StepPixelsDesc._fields_] == ["bg_rays", "rgba", "target_out"]
    assert ctypes.sizeof(nerftex_hip.StepLossDesc(0, 0.0, None, None, None, 0, 0.1, 0.9)) == 48, "the criterion's descriptor keeps its layout"
    for name in ("nerftex_render_tail_forward", "nerftex_render_tail_backward", "nerftex_composite_tail_backward", "nerftex_composite_step"):
        ex, px = nerftex_hip._SIGNATURES[name + "_ex"], nerftex_hip._SIGNATURES[name + "_px"]
        assert px == ex[:-1] + [ctypes.c_void_p] + ex[-1:], f"{name}_px is {name}_ex with one more descriptor before the stream"


P = 1 << 20  # a pointer that is never dereferenced: every call below is refused before a launch
BAD = [
    (dict(bg_rays=None, rgba=None, target_out=None, target=P), "needs bg_rays"),
    (dict(bg_rays=None, rgba=P, target_out=P, target=None), "needs bg_rays"),
    (dict(bg_rays=P, rgba=P, target_out=P, target=P), "exactly one of the pixels descriptor's rgba [N,4] and the entry's target [N,3] (got both)"),
    (dict(bg_rays=P, rgba=None, target_out=None, target=None), "exactly one of the pixels descriptor's rgba [N,4] and the entry's target [N,3] (got neither)"),
    (dict(bg_rays=P, rgba=None, target_out=P, target=None), "(got neither)"),
    (dict(bg_rays=P, rgba=P, target_out=None, target=None), "rgba needs target_out"),
]


@pytest.mark.parametrize("with_loss_desc", [False, True], ids=["mse", "l1"])
@pytest.mark.parametrize("bad,message", BAD, ids=["no_bg", "no_bg_rgba", "both", "neither", "neither_with_out", "no_target_out"])
def test_the_px_entries_refuse_a_bad_pixels_descriptor_before_launching(bad, message, with_loss_desc):
    """NERFTEX_ERR_INVALID (1) with a message from each of the four entries; no pointer handed over here is ever dereferenced."""
    from nerftex_hip import StepLossDesc, StepPixelsDesc, lib

    px = ctypes.byref(StepPixelsDesc(bad["bg_rays"], bad["rgba"], bad["target_out"]))
    desc = ctypes.byref(StepLossDesc(L1, 0.0, None, None, None, 0, 0.1, 0.9)) if with_loss_desc else None
    t = bad["target"]
    calls = [
        (lib.nerftex_composite_step_px, (P, P, P, P, 128, 4, P, P, t, 1.0, 1.0, None, P, P, P, P, P, P, P, P, P, P, None)),
        (lib.nerftex_render_tail_forward_px, (P, P, P, P, P, t, 1.0, 1.0, 4, P, P, P, P, P, None, P, None, 0)),
        (lib.nerftex_composite_tail_backward_px, (P, None, 1.0, P, t, 1.0, P, P, P, P, P, P, 128, 4, P, P, None)),
        (lib.nerftex_render_tail_backward_px, (P, None, 1.0, P, t, 1.0, 4, P, P)),
    ]
    for fn, args in calls:
        assert fn(*args, desc, px, None) == 1, fn.__name__
        assert message in lib.nerftex_last_error().decode(), (fn.__name__, lib.nerftex_last_error().decode())


def test_a_bad_criterion_is_still_refused_by_the_px_entries():
    from nerftex_hip import StepLossDesc, StepPixelsDesc, lib

    px, desc = ctypes.byref(StepPixelsDesc(P, None, None)), ctypes.byref(StepLossDesc(7, 0.0, None, None, None, 0, 0.1, 0.9))
    assert lib.nerftex_render_tail_backward_px(P, None, 1.0, P, P, 1.0, 4, P, P, desc, px, None) == 1
    assert "unknown criterion kind 7" in lib.nerftex_last_error().decode()


NOTHING = types.SimpleNamespace(field=None)


@pytest.mark.parametrize("kw,message", [
    (dict(bg_color="rand"), "bg_color: a number"), (dict(bg_color=""), "bg_color: a number"), (dict(bg_color="Random"), "bg_color: a number"),
    (dict(bg_color=None), "bg_color: a number"), (dict(bg_color=(1, 1, 1)), "bg_color: a number"),
    (dict(target_channels=2), "target_channels: 3"), (dict(target_channels=5), "target_channels: 3"), (dict(target_channels="4"), "target_channels: 3"),
    (dict(target_channels=True), "target_channels: 3"), (dict(target_channels=4.5), "target_channels: 3"),
    (dict(bg_generator=torch.Generator()), "bg_generator: a torch.Generator"), (dict(bg_color="given", bg_generator=torch.Generator()), "bg_generator: a torch.Generator"),
    (dict(bg_color="random", bg_generator=7), "bg_generator: a torch.Generator"),
], ids=lambda v: repr(v)[:50] if isinstance(v, dict) else None)
def test_trainers_refuse_before_the_renderer_is_looked_at(kw, message):
    for cls in (AcceleratedTrainer, CurvedTrainer):
        with pytest.raises(ValueError, match=message):
            cls(NOTHING, **kw)


@pytest.mark.parametrize("kw", [dict(bg_color="random"), dict(bg_color="given"), dict(bg_color=0.5, target_channels=4), dict(target_channels=4),
                                dict(bg_color="random", target_channels=4, bg_generator=torch.Generator()), dict(bg_color=0), dict(bg_color=torch.ones(()))],
                         ids=lambda v: repr(sorted(v))[:50])
def test_accepted_arguments_get_past_the_refusal(kw):
    for cls in (AcceleratedTrainer, CurvedTrainer):
        with pytest.raises(AssertionError, match="field|CurvedField"):  # (the renderer is looked at, and is no renderer)
            cls(NOTHING, **kw)


def _bare(cls, **kw):
    """A trainer with its pixel constants and nothing else: what `step` looks at before anything is copied or launched."""
    tr = cls.__new__(cls)
    tr._init_pixels(kw.get("bg_color", 1), kw.get("target_channels", 3), kw.get("bg_generator"))
    tr.group = 4
    return tr


@pytest.mark.parametrize("cls", [AcceleratedTrainer, CurvedTrainer])
def test_a_mismatched_batch_is_refused_before_anything_is_copied(cls):
    o = torch.zeros(8, 3)
    o4 = torch.zeros(4, 8, 3)
    rgb, rgba, bg = torch.zeros(8, 3), torch.zeros(8, 4), torch.zeros(8, 3)
    # (a trainer that got this far would touch `renderer`, which these do not have: AttributeError, not ValueError)
    with pytest.raises(ValueError, match=r"target: a floating-point \[N,4\] tensor .*target_channels=4.*got torch.float32 \(8, 3\)"):
        _bare(cls, target_channels=4).step(o, o, rgb)
    with pytest.raises(ValueError, match=r"target: a floating-point \[k,N,4\]"):
        _bare(cls, target_channels=4).step_group(o4, o4, torch.zeros(4, 8, 3))
    with pytest.raises(ValueError, match=r"target: a floating-point \[N,3\]"):
        _bare(cls, bg_color="random").step(o, o, rgba)
    with pytest.raises(ValueError, match=r"target: a floating-point \[N,4\]"):
        _bare(cls, target_channels=4).step(o, o, rgba.to(torch.int32))
    with pytest.raises(ValueError, match='bg= without bg_color="given": this trainer blends over a constant colour'):
        _bare(cls).step(o, o, rgb, bg=bg)
    with pytest.raises(ValueError, match='bg= without bg_color="given": this trainer draws its backgrounds itself'):
        _bare(cls, bg_color="random", target_channels=4).step(o, o, rgba, bg=bg)
    with pytest.raises(ValueError, match='bg_color="given": pass the rays. backgrounds'):
        _bare(cls, bg_color="given").step(o, o, rgb)
    with pytest.raises(ValueError, match=r"bg: a torch.float32 tensor of shape \(8, 3\)"):
        _bare(cls, bg_color="given").step(o, o, rgb, bg=torch.zeros(8, 4))
    with pytest.raises(ValueError, match=r"bg: a torch.float32 tensor of shape \(8, 3\)"):
        _bare(cls, bg_color="given").step(o, o, rgb, bg=torch.zeros(7, 3))
    with pytest.raises(ValueError, match=r"bg: a torch.float32 tensor of shape \(8, 3\)"):
        _bare(cls, bg_color="given", target_channels=4).step(o, o, rgba, bg=bg.double())
    with pytest.raises(ValueError, match=r"bg: a torch.float32 tensor of shape \(4, 8, 3\)"):
        _bare(cls, bg_color="given", target_channels=4).step_group(o4, o4, torch.zeros(4, 8, 4), bg=torch.zeros(8, 3))
    # what matches gets past the check (and fails on the renderer these bare trainers lack)
    with pytest.raises(AttributeError):
        _bare(cls, bg_color="given", target_channels=4).step(o, o, rgba, bg=bg)
    with pytest.raises(AttributeError):
        _bare(cls).step(o, o, rgb)


def test_step_pixels_refuses_on_the_host():
    from ngp_harness import fused

    dev = torch.device("cpu")
    rgb, rgba, bg = torch.zeros(8, 3), torch.zeros(8, 4), torch.zeros(8, 3)
    assert fused.step_pixels(1.0, rgb, 8, dev) is None, "a number and [N,3]: the entries as ever"
    desc, bg_rays, target, gt = fused.step_pixels(bg, rgb, 8, dev)
    assert (desc.bg_rays, desc.rgba, desc.target_out) == (bg.data_ptr(), None, None) and target is rgb and gt is None
    desc, bg_rays, target, gt = fused.step_pixels(bg, rgba, 8, dev)
    assert (desc.bg_rays, desc.rgba, desc.target_out) == (bg.data_ptr(), rgba.data_ptr(), gt.data_ptr()) and target is None and gt.shape == (8, 3)
    out = torch.zeros(8, 3)
    desc, bg_rays, _, gt = fused.step_pixels(0.25, rgba, 8, dev, out)
    assert gt is out and bg_rays.shape == (8, 3) and float(bg_rays.min()) == float(bg_rays.max()) == 0.25, "a number under RGBA pixels is spread over the rays"
    for bad in (torch.zeros(8, 4), torch.zeros(7, 3), torch.zeros(8, 3, dtype=torch.float64), torch.zeros(3, 8).t()):
        with pytest.raises(ValueError, match="bg: a number, or a contiguous torch.float32"):
            fused.step_pixels(bad, rgb, 8, dev)
    with pytest.raises(ValueError, match=r"target: \[N,3\] colours or \[N,4\] RGBA"):
        fused.step_pixels(bg, torch.zeros(8, 5), 8, dev)
    with pytest.raises(ValueError, match="target_out: only an"):
        fused.step_pixels(1.0, rgb, 8, dev, out)
    with pytest.raises(ValueError, match="target_out: a contiguous torch.float32"):
        fused.step_pixels(bg, rgba, 8, dev, torch.zeros(8, 4))


def test_the_float64_statement():
    """pixels_float64 against the closed forms: a == 0 gives the background, a == 1 the colour; an empty ray's image is its background; the MSE's
    gradients are 2 d g / 3N and -(sum_c grad_image[c] * bg[c]); with bg == 1 and a == 1 it is the scalar step on target = rgb."""
    g = torch.Generator().manual_seed(0)
    N = 7
    image, ws, bg = torch.rand(N, 3, generator=g), torch.rand(N, generator=g), torch.rand(N, 3, generator=g)
    rgba = torch.rand(N, 4, generator=g)
    rgba[0, 3], rgba[1, 3] = 0.0, 1.0
    image[2], ws[2] = 0.0, 0.0
    for kind, param in ((MSE, 0.0), (L1, 0.0), (HUBER, 0.1)):
        r = pixels_float64(image, ws, bg, rgba=rgba, kind=kind, param=param, loss_mul=0.5, grad_loss=3.0)
        assert torch.equal(r["gt"][0], bg[0].double()) and torch.equal(r["gt"][1], rgba[1, :3].double()) and torch.equal(r["image_out"][2], bg[2].double())
        assert torch.allclose(r["grad_ws"], -(r["grad_image"] * bg.double()).sum(-1), rtol=1e-12, atol=0)
        assert abs(float(r["ray_loss"].mean() * 0.5) - float(r["loss"])) <= 1e-15
    r = pixels_float64(image, ws, bg, rgba=rgba, loss_mul=0.5, grad_loss=3.0)
    d = r["image_out"] - r["gt"]
    assert torch.allclose(r["grad_image"], 2 * d * 0.5 * 3.0 / (3 * N), rtol=1e-12, atol=0)
    ones = torch.ones(N, 3)
    opaque = torch.cat([rgba[:, :3], torch.ones(N, 1)], 1)
    a, b = pixels_float64(image, ws, ones, rgba=opaque, kind=L1), pixels_float64(image, ws, ones, target=rgba[:, :3], kind=L1)
    assert all(torch.equal(a[k], b[k]) for k in a)
