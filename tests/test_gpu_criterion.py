"""L1 / Huber criteria, the per-ray loss and the error map on the fused training step (nerftex_*_ex with a nerftex_step_loss_desc;
fused.render_tail / composite_tail, accelerate(criterion=, error_map=)).  Reference statements: torch in float64 -- F.mse_loss / l1_loss /
huber_loss of the blended image, `0.1 * map.gather(...) + 0.9 * error; scatter_` for the map (nerf/utils.py:617-632) -- and torch's own float32
backward for grad_image.  Tolerances are those of the number formats: see each test."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
MSE, L1, HUBER = 0, 1, 2
CRITERIA = [("l1", L1, 0.0), ("huber0.1", HUBER, 0.1), ("huber_wide", HUBER, 64.0)]  # (64 > every |d|: images and targets lie in [0, 2])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _desc(kind, param=0.0, ray_loss=None, error_map=None, error_inds=None, keep=0.1, take=0.9):
    from nerftex_hip import StepLossDesc, ptr

    return StepLossDesc(kind, param, ptr(ray_loss), ptr(error_map), ptr(error_inds), 0 if error_map is None else error_map.numel(), keep, take)


def _criterion64(kind, param, a, b, reduction="mean"):
    a, b = a.double(), b.double()
    if kind == MSE:
        return F.mse_loss(a, b, reduction=reduction)
    if kind == L1:
        return F.l1_loss(a, b, reduction=reduction)
    return F.huber_loss(a, b, reduction=reduction, delta=param)


_RAGGED = {}


def _ragged(dev, N):
    """The synthetic ragged rays of tests/test_gpu_trainstep.py::test_composite_tail_equals_compositing_then_render_tail: an empty ray, a ray past
    the buffer's end, counts up to 150 (more than two 64-sample chunks).  Made once per N, never modified."""
    if N not in _RAGGED:
        g = torch.Generator(device="cpu").manual_seed(N)
        counts = torch.randint(0, 150, (N,), generator=g)
        counts[0] = 0
        offsets = torch.cumsum(counts, 0) - counts
        M = int(counts.sum()) + 8
        if N > 2:
            counts[-1] = counts[-1] + 9
        rays = torch.stack([torch.arange(N), offsets, counts], dim=1).to(torch.int32).to(dev)
        sigmas = (torch.rand(M, generator=g) * 30).to(dev)
        rgbs = torch.rand(M, 3, generator=g).to(dev)
        deltas = torch.stack([torch.rand(M, generator=g) * 0.02 + 0.003, torch.rand(M, generator=g) * 0.03 + 0.003], dim=1).to(dev)
        nears = (torch.rand(N, generator=g) + 0.2).to(dev)
        fars = nears + (torch.rand(N, generator=g) * 3 + 0.1).to(dev)
        target = torch.rand(N, 3, generator=g).to(dev)
        _RAGGED[N] = dict(rays=rays, sigmas=sigmas, rgbs=rgbs, deltas=deltas, nears=nears, fars=fars, target=target, M=M, N=N)
    return _RAGGED[N]


BG, MUL = 1.0, 0.5


def _three_launches(dev, c, scale, desc, ex):
    """Compositing forward, render tail, compositing backward with a root gradient of one: the entries as they were (ex False) or their _ex
    siblings with `desc` (None: NULL).  -> per-ray outputs [9, N], (loss, scaled loss), gradients [4 M], step flags."""
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
    fwd = (ptr(ws), ptr(depth), ptr(image), ptr(c["nears"]), ptr(c["fars"]), ptr(c["target"]), BG, MUL, N, ptr(image_out), ptr(depth_out), ptr(partial), ptr(ticket),
           ptr(losses), ptr(scale), losses.data_ptr() + 4, ptr(flags), words)
    bwd = (ptr(one), ptr(scale), MUL, ptr(image_out), ptr(c["target"]), BG, ptr(c["sigmas"]), ptr(c["rgbs"]), ptr(c["deltas"]), ptr(c["rays"]), ptr(ws), ptr(image), M, N,
           ptr(g[:M]), ptr(g[M:]), ptr(flags))
    if ex:
        check(lib.nerftex_render_tail_forward_ex(*fwd, by, stream()))
        check(lib.nerftex_composite_tail_backward_ex(*bwd, by, stream()))
    else:
        check(lib.nerftex_render_tail_forward_live(*fwd, stream()))
        check(lib.nerftex_composite_tail_backward_live(*bwd, stream()))
    assert int(ticket[0]) == 0
    return per_ray, losses, g, flags


def _one_launch(dev, c, scale, desc, ex, with_loss=True):
    from nerftex_hip import check, lib, ptr, stream

    M, N = c["M"], c["N"]
    per_ray = torch.full((9, N), float("nan"), device=dev)
    ws, depth, depth_out, image, image_out = per_ray[0], per_ray[1], per_ray[2], per_ray[3:6].view(N, 3), per_ray[6:9].view(N, 3)
    losses = torch.full((2,), float("nan"), device=dev)
    err = torch.full((N,), float("nan"), device=dev)
    flags = torch.zeros((M + 31) // 32, dtype=torch.int32, device=dev)
    g = torch.full((4 * M,), float("nan"), device=dev)
    args = (ptr(c["sigmas"]), ptr(c["rgbs"]), ptr(c["deltas"]), ptr(c["rays"]), M, N, ptr(c["nears"]), ptr(c["fars"]), ptr(c["target"]), BG, MUL, ptr(scale), ptr(ws),
            ptr(depth), ptr(image), ptr(image_out), ptr(depth_out), ptr(err), ptr(losses) if with_loss else None, losses.data_ptr() + 4 if with_loss else None,
            ptr(g[:M]), ptr(g[M:]), ptr(flags))
    if ex:
        check(lib.nerftex_composite_step_ex(*args, None if desc is None else ctypes.byref(desc), stream()))
    else:
        check(lib.nerftex_composite_step(*args, stream()))
    return per_ray, losses, g, flags, err


def _same(a, b, what):
    names = ("per-ray outputs", "loss, scaled loss", "gradients")
    for x, y, n in zip(a[:3], b[:3], names):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: {n}"
    assert torch.equal(a[3] != 0, b[3] != 0), f"{what}: step flags"


# ------------------------------------------------------------------------------------------------- 1. the old path is untouched
@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("N", [3, 1000])
def test_ex_entries_without_a_criterion_are_the_entries_they_extend(dev, N, scaled):
    """Each _ex entry with a NULL descriptor, and with {kind = MSE} and no outputs (the general instantiation), against the entry it extends:
    every output, the loss, the scaled loss, the gradients and the step flags bit for bit."""
    from nerftex_hip import check, lib, ptr, stream

    c = _ragged(dev, N)
    scale = torch.full((), 1024.0, device=dev) if scaled else None
    old3, old1 = _three_launches(dev, c, scale, None, ex=False), _one_launch(dev, c, scale, None, ex=False)
    assert float(old3[2][:c["M"]].abs().max()) > 0 and torch.isfinite(old3[1]).all()
    for name, desc in (("NULL", None), ("MSE", _desc(MSE))):
        _same(old3, _three_launches(dev, c, scale, desc, ex=True), f"three launches, {name}")
        new1 = _one_launch(dev, c, scale, desc, ex=True)
        _same(old1, new1, f"one launch, {name}")
        assert torch.equal(_bits(old1[4]), _bits(new1[4])), f"err[] ({name})"
        # the stand-alone backward of the render tail
        image_out, gl = old3[0][6:9].view(N, 3).contiguous(), torch.full((), 3.0, device=dev)
        out = []
        for ex in (False, True):
            gi, gw = torch.full((N, 3), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)
            args = (ptr(gl), ptr(scale), MUL, ptr(image_out), ptr(c["target"]), BG, N, ptr(gi), ptr(gw))
            if ex:
                check(lib.nerftex_render_tail_backward_ex(*args, None if desc is None else ctypes.byref(desc), stream()))
            else:
                check(lib.nerftex_render_tail_backward(*args, stream()))
            out.append((gi, gw))
        assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(_bits(out[0][1]), _bits(out[1][1])), f"render_tail_backward ({name})"


# ------------------------------------------------------------------------------------------------- 2. L1 and Huber against torch
@pytest.mark.parametrize("name,kind,param", CRITERIA, ids=[c[0] for c in CRITERIA])
@pytest.mark.parametrize("N", [1, 257, 1000])
def test_criteria_match_torch(dev, N, name, kind, param):
    """fused.render_tail(criterion=) (the three-launch form's tail) against the framework: images bit-equal to the MSE call's; the loss within
    1e-5 relative of float64 (a tree of at most 20 roundings over non-negative terms plus at most four per element: < 30 * 2^-24 = 1.8e-6);
    grad_image within 4 * 2^-24 relative of torch's float32 backward of the same criterion (one division and one multiply may round
    differently), and exactly torch's where d == 0 (0) and where |d| == delta (the quadratic branch: d itself); grad_ws at the tolerance of the
    MSE test for the same three-term sum."""
    from ngp_harness import fused

    g = torch.Generator(device="cpu").manual_seed(1000 + N)
    ws = torch.rand(N, generator=g).to(dev)
    depth = (torch.rand(N, generator=g) * 3).to(dev)
    image = torch.rand(N, 3, generator=g).to(dev)
    nears = (torch.rand(N, generator=g) + 0.2).to(dev)
    fars = nears + (torch.rand(N, generator=g) * 3 + 0.1).to(dev)
    target = torch.rand(N, 3, generator=g).to(dev)
    delta = np.float32(0.1)
    # rays whose d is exactly 0, +delta, -delta: an opaque ray (weights_sum 1: the blend adds (1 - 1) * bg = 0) against a target of 0 or itself
    special = [0] if N == 1 else [1, N // 2, N - 1]
    for n in special:
        ws[n] = 1.0
        image[n] = torch.tensor([0.375, float(delta), 0.0])
        target[n] = torch.tensor([0.375, 0.0, float(delta)])
    gl = torch.full((), 128.0, device=dev)
    crit = {L1: "l1", HUBER: ("huber", param)}[kind]

    _, _, mse_loss, _ = fused.render_tail(ws, depth, image, nears, fars, target, BG, MUL)
    ws1, im1 = ws.clone().requires_grad_(True), image.clone().requires_grad_(True)
    img_ref = im1 + (1 - ws1).unsqueeze(-1) * BG
    torch_loss = (F.l1_loss(img_ref, target) if kind == L1 else F.huber_loss(img_ref, target, delta=param)) * MUL
    torch_loss.backward(gl)
    d = (img_ref.detach() - target)
    assert all(d[n, 0] == 0 and d[n, 1] == delta and d[n, 2] == -delta for n in special)

    ws2, im2 = ws.clone().requires_grad_(True), image.clone().requires_grad_(True)
    img, dep, loss, scaled = fused.render_tail(ws2, depth, im2, nears, fars, target, BG, MUL, criterion=crit)
    scaled.backward(gl)
    img_mse, dep_mse, _, _ = fused.render_tail(ws, depth, image, nears, fars, target, BG, MUL)
    assert torch.equal(_bits(img), _bits(img_mse)) and torch.equal(_bits(dep), _bits(dep_mse)) and torch.equal(img, img_ref.detach())
    want = float(_criterion64(kind, param, img, target) * MUL)
    print(f"N {N} {name}: loss {loss.item():.9g} float64 {want:.9g} rel {abs(loss.item() - want) / want:.3g}")
    assert abs(loss.item() - want) <= 1e-5 * want and scaled.item() == loss.item()
    rel = ((im2.grad - im1.grad).abs() / im1.grad.abs().clamp_min(1e-30)).max().item()
    print(f"N {N} {name}: grad_image max rel {rel / EPS:.3g} * 2^-24")
    assert ((im2.grad - im1.grad).abs() <= 4 * EPS * im1.grad.abs()).all()
    for n in special:  # d == 0: exactly 0; |d| == delta: the quadratic branch (Huber: d; L1: the sign)
        assert im2.grad[n, 0].item() == 0.0 and im1.grad[n, 0].item() == 0.0
        assert im2.grad[n, 1].item() > 0 and im2.grad[n, 2].item() == -im2.grad[n, 1].item()
    torch.testing.assert_close(ws2.grad, ws1.grad, rtol=1e-5, atol=1e-7)
    if name == "huber_wide":  # every element on the quadratic branch: half the squared error
        assert abs(loss.item() - 0.5 * mse_loss.item()) <= 2 * EPS * 0.5 * mse_loss.item(), (loss.item(), mse_loss.item())
    # under a loss scaler's device scalar the scaled loss and the gradient carry it
    ws3, im3 = ws.clone().requires_grad_(True), image.clone().requires_grad_(True)
    scale = torch.full((), 128.0, device=dev)
    _, _, loss3, scaled3 = fused.render_tail(ws3, depth, im3, nears, fars, target, BG, MUL, scale, criterion=crit)
    scaled3.backward(torch.ones((), device=dev))
    assert loss3.item() == loss.item() and scaled3.item() == loss.item() * 128.0
    assert torch.equal(im3.grad, im2.grad) and torch.equal(ws3.grad, ws2.grad)


# ------------------------------------------------------------------------------------------------- 3. one launch equals three launches
def _field_backward_args(dev):
    """A small field backward (128 * 8 rows) for the entries that finish a step's loss beside their reduction."""
    from nerftex_hip import check, lib, ptr, stream

    B = 128 * 8
    g = torch.Generator(device=dev).manual_seed(2)
    ws = ((torch.rand(64 * (32 + 64 + 16), device=dev, generator=g) - 0.5) * 0.3).half()
    wc = ((torch.rand(64 * (32 + 128 + 16), device=dev, generator=g) - 0.5) * 0.3).half()
    feats = (torch.rand(16, B, 2, device=dev, generator=g) - 0.5).half()
    dirs = F.normalize(torch.randn(B, 3, device=dev, generator=g), dim=-1)
    sigma, rgbs = torch.empty(B, device=dev), torch.empty(B, 3, device=dev)
    x_rows, h, cin = (torch.empty(B, 32, dtype=torch.float16, device=dev), torch.empty(B, 16, dtype=torch.float16, device=dev),
                      torch.empty(B, 32, dtype=torch.float16, device=dev))
    check(lib.nerftex_field_forward(ptr(feats), ptr(dirs), ptr(ws), ptr(wc), B, ptr(sigma), ptr(rgbs), ptr(x_rows), ptr(h), ptr(cin), None, stream()))
    gs, gc = torch.randn(B, device=dev, generator=g) * 1e-2, torch.randn(B, 3, device=dev, generator=g) * 1e-2
    grad_cin, grad_x = torch.zeros(B, 32, dtype=torch.float16, device=dev), torch.empty(B, 32, dtype=torch.float16, device=dev)
    gws, gwc = torch.empty_like(ws), torch.empty_like(wc)
    keep = (ws, wc, feats, dirs, sigma, rgbs, x_rows, h, cin, gs, gc, grad_cin, grad_x, gws, gwc)
    return (ptr(gs), ptr(gc), ptr(rgbs), ptr(h), ptr(cin), ptr(x_rows), ptr(ws), ptr(wc), B, ptr(grad_cin), ptr(grad_x), ptr(gws), ptr(gwc)), B, keep


@pytest.mark.parametrize("name,kind,param", [("mse", MSE, 0.0)] + CRITERIA[:2], ids=["mse", "l1", "huber0.1"])
@pytest.mark.parametrize("N", [3, 1000])
def test_one_launch_equals_three_launches_per_criterion(dev, knobs, N, name, kind, param):
    """nerftex_composite_step_ex against the three _ex launches, for every number of kept chunks, with and without a loss scale: outputs, loss,
    gradients, step flags, the per-ray loss and the error map bit for bit -- and the deferred loss (loss = NULL: err[] finished by
    nerftex_field_backward_live_consume, or by the trailer of nerftex_field_backward_live_deferred run as a launch of its own)."""
    from nerftex_hip import StepLoss, StepTrailer, check, lib, ptr, stream

    c = _ragged(dev, N)
    R = 4096
    gen = torch.Generator(device="cpu").manual_seed(77 + N)
    prefill = torch.rand(R, generator=gen).to(dev)
    inds = torch.randperm(R, generator=gen)[:N].to(dev)
    inds[0] = -1
    core, B, _keepalive = _field_backward_args(dev)
    for scale in (None, torch.full((), 1024.0, device=dev)):
        rl3, map3 = torch.full((N,), float("nan"), device=dev), prefill.clone()
        three = _three_launches(dev, c, scale, _desc(kind, param, rl3, map3, inds), ex=True)
        assert torch.isfinite(rl3).all() and not torch.equal(map3, prefill)
        for keep in (0, 1, 3, 4):
            knobs(composite_keep=keep)
            rl1, map1 = torch.full((N,), float("nan"), device=dev), prefill.clone()
            one = _one_launch(dev, c, scale, _desc(kind, param, rl1, map1, inds), ex=True)
            _same(three, one, f"{name}, keep {keep}")
            assert torch.equal(_bits(rl3), _bits(rl1)) and torch.equal(_bits(map3), _bits(map1)), f"{name}, keep {keep}: ray_loss / map"
        # the deferred loss: the same err[], finished elsewhere
        rl2, map2 = torch.full((N,), float("nan"), device=dev), prefill.clone()
        deferred = _one_launch(dev, c, scale, _desc(kind, param, rl2, map2, inds), ex=True, with_loss=False)
        assert torch.equal(_bits(deferred[4]), _bits(one[4])) and torch.isnan(deferred[1]).all()
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


# ------------------------------------------------------------------------------------------------- 4. per-ray loss and the map
@pytest.mark.parametrize("name,kind,param", [("mse", MSE, 0.0)] + CRITERIA[:2], ids=["mse", "l1", "huber0.1"])
@pytest.mark.parametrize("form", ["three_launches", "one_launch"])
def test_ray_loss_and_error_map(dev, form, name, kind, param):
    """ray_loss within 8 * 2^-24 relative of float64 criterion(image_out, target).mean(-1) (per channel: the difference, the element -- up to
    three operations for Huber --, then two adds and the division by 3, all on non-negative terms); the named cells of a 4096-cell map within
    8 * 2^-24 relative of float64 0.1 * old + 0.9 * error (two multiplies and an add on top of an error that is itself within 6 roundings:
    positive terms, so the relative errors do not grow); every other cell bit-identical; -1 and R touch nothing; a second call applies the
    moving average to the first call's result."""
    N, R = 1000, 4096
    c = _ragged(dev, N)
    gen = torch.Generator(device="cpu").manual_seed(5)
    prefill = torch.rand(R, generator=gen).to(dev)
    inds = torch.randperm(R, generator=gen)[:N].to(dev)
    inds[torch.randperm(N, generator=gen)[:N // 10].to(dev)] = -1
    inds[7] = R
    named = (inds >= 0) & (inds < R)
    assert int(named.sum()) == N - N // 10 - 1 and inds[named].unique().numel() == int(named.sum())
    ray_loss, emap = torch.full((N,), float("nan"), device=dev), prefill.clone()
    run = (lambda d: _three_launches(dev, c, None, d, ex=True)) if form == "three_launches" else (lambda d: _one_launch(dev, c, None, d, ex=True))
    out = run(_desc(kind, param, ray_loss, emap, inds))
    image_out = out[0][6:9].view(N, 3)
    want = _criterion64(kind, param, image_out, c["target"], reduction="none").mean(-1)
    rel = ((ray_loss.double() - want).abs() / want).max().item()
    print(f"{form} {name}: ray_loss max rel {rel / EPS:.3g} * 2^-24")
    assert ((ray_loss.double() - want).abs() <= 8 * EPS * want).all()

    def ema(old, error):  # nerf/utils.py:617-632, in float64
        new = old.double().clone()
        cells = inds[named]
        new.scatter_(0, cells, 0.1 * new.gather(0, cells) + 0.9 * error[named])
        return new

    want_map = ema(prefill, want)
    touched = torch.zeros(R, dtype=torch.bool, device=dev)
    touched[inds[named]] = True
    assert ((emap.double() - want_map).abs() <= 8 * EPS * want_map)[touched].all()
    assert torch.equal(_bits(emap[~touched]), _bits(prefill[~touched])), "cells no ray names (the rays at -1 and at R included) keep their bits"
    first = emap.clone()
    run(_desc(kind, param, ray_loss, emap, inds))
    want2 = ema(first, want)
    assert ((emap.double() - want2).abs() <= 8 * EPS * want2)[touched].all() and not torch.equal(emap[touched], first[touched])
    assert torch.equal(_bits(emap[~touched]), _bits(prefill[~touched]))
    # other factors than the reference's
    emap3 = prefill.clone()
    run(_desc(kind, param, None, emap3, inds, keep=0.5, take=0.25))
    want3 = prefill.double().clone()
    want3[inds[named]] = 0.5 * prefill.double()[inds[named]] + 0.25 * want[named]
    assert ((emap3.double() - want3).abs() <= 8 * EPS * want3).all()


# ------------------------------------------------------------------------------------------------- descriptor rejections
@pytest.mark.parametrize("bad", ["kind", "delta", "map_without_indices"])
def test_bad_descriptors_launch_nothing(dev, bad):
    c = _ragged(dev, 3)
    emap = torch.zeros(16, device=dev)
    desc = {"kind": _desc(9), "delta": _desc(HUBER, 0.0), "map_without_indices": _desc(L1, error_map=emap)}[bad]
    from nerftex_hip import lib, ptr, stream

    M, N = c["M"], c["N"]
    out = torch.full((9 * N + 2 + N + 4 * M,), float("nan"), device=dev)
    p = out.data_ptr()
    by = ctypes.byref(desc)
    rc = lib.nerftex_composite_step_ex(ptr(c["sigmas"]), ptr(c["rgbs"]), ptr(c["deltas"]), ptr(c["rays"]), M, N, ptr(c["nears"]), ptr(c["fars"]), ptr(c["target"]), BG, MUL,
                                       None, p, p + 4 * N, p + 12 * N, p + 24 * N, p + 8 * N, p + 4 * (9 * N + 2), p + 36 * N, p + 36 * N + 4, p + 4 * (10 * N + 2),
                                       p + 4 * (10 * N + 2 + M), None, by, stream())
    assert rc == 1 and lib.nerftex_last_error().decode(), "NERFTEX_ERR_INVALID with a message"
    rc = lib.nerftex_render_tail_forward_ex(p, p + 4 * N, p + 12 * N, ptr(c["nears"]), ptr(c["fars"]), ptr(c["target"]), BG, MUL, N, p + 24 * N, p + 8 * N, p + 4 * (10 * N + 2),
                                            None, p + 36 * N, None, p + 36 * N + 4, None, 0, by, stream())
    assert rc == 1 and lib.nerftex_last_error().decode()
    if bad != "map_without_indices":
        rc = lib.nerftex_composite_tail_backward_ex(p + 36 * N, None, MUL, p + 24 * N, ptr(c["target"]), BG, ptr(c["sigmas"]), ptr(c["rgbs"]), ptr(c["deltas"]), ptr(c["rays"]),
                                                    p, p + 12 * N, M, N, p + 4 * (10 * N + 2), p + 4 * (10 * N + 2 + M), None, by, stream())
        assert rc == 1 and lib.nerftex_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and int(emap.abs().sum()) == 0, "nothing was launched"


# ------------------------------------------------------------------------------------------------- 5. the trainer
_SCENE = {}


def _ngp_case(dev):
    """The scene, rays and targets of tests/test_gpu_round3.py::test_accelerate_replays_the_eager_step, made once."""
    if not _SCENE:
        from ngp_harness import scene

        sc = scene.Scene(bound=2.0, seed=0)
        grid, _, _ = sc.bitfield()
        rays = [scene.train_batch(2048, seed=200 + k, n_views=2) for k in range(8)]
        _SCENE["grid"] = torch.from_numpy(grid).to(dev)
        _SCENE["rays"] = [(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)) for o, d in rays]
        _SCENE["tgt"] = torch.rand(8, 2048, 3, generator=torch.Generator().manual_seed(9)).to(dev) * 0.2 + 0.4
        g = torch.Generator().manual_seed(10)
        _SCENE["inds"] = torch.stack([torch.randperm(8 * 2048, generator=g)[:2048] for _ in range(8)]).to(dev)
    return _SCENE


def _ngp_trainer(dev, **kw):
    from ngp_harness.accelerate import accelerate
    from ngp_harness.model import NGPField, Renderer

    torch.manual_seed(0)
    field = NGPField(bound=2.0, mlp="ffmlp", fused_glue=True).to(dev)
    torch.manual_seed(1)
    field.encoder.embeddings.data.uniform_(-1e-4, 1e-4)
    r = Renderer(field, bound=2.0, min_near=0.2, density_thresh=10.0).to(dev)
    r.set_occupancy(_ngp_case(dev)["grid"])
    field.train()
    return field, accelerate(r, perturb=False, **kw)


def _train(dev, calls, k=1, ahead=False, use_map=True, overflow_at=None, **kw):
    """`calls` calls of k steps each over the 8 batches -> (parameters after sync(), losses, last ray_loss, the map, the trainer)."""
    s = _ngp_case(dev)
    emap = torch.full((8, 2048), 0.5, device=dev) if use_map else None
    field, tr = _ngp_trainer(dev, steps_per_call=k, **({"error_map": emap} if use_map else {}), **kw)
    losses, notes = [], {}

    def batch(i):
        idx = [(i * k + j) % 8 for j in range(k)]
        o = torch.stack([s["rays"][j][0] for j in idx]).contiguous()
        d = torch.stack([s["rays"][j][1] for j in idx]).contiguous()
        return o, d, s["tgt"][idx].contiguous(), s["inds"][idx].contiguous()

    cur = batch(0)
    for i in range(calls):
        nxt = batch(i + 1)
        if overflow_at == i:
            tr.sync()
            notes["before"] = ({n: p.detach().clone() for n, p in field.named_parameters()}, emap.clone(), float(tr.opt.step_count))
            tr.amp.scale.fill_(2.0 ** 40)
        more = {"error_inds": cur[3] if k > 1 else cur[3][0]} if use_map else {}
        if k > 1:
            tr.step_group(cur[0], cur[1], cur[2], next_rays=(nxt[0], nxt[1]) if ahead else None, **more)
        else:
            tr.step(cur[0][0], cur[1][0], cur[2][0], next_rays=(nxt[0][0], nxt[1][0]) if ahead else None, **more)
        if overflow_at == i:
            tr.sync()
            notes["after"] = ({n: p.detach().clone() for n, p in field.named_parameters()}, emap.clone(), float(tr.opt.step_count))
        losses.append(tr.loss.clone())
        cur = nxt
    torch.cuda.synchronize()
    tr.sync()
    params = {n: p.detach().clone() for n, p in field.named_parameters()}
    return params, torch.stack(losses), None if tr.ray_loss is None else tr.ray_loss.clone(), emap, tr, notes


def _equal_runs(a, b, what):
    for n in a[0]:
        assert torch.equal(a[0][n], b[0][n]), f"{what}: parameter {n}"
    assert torch.equal(_bits(a[1]), _bits(b[1])), f"{what}: losses"
    if a[2] is not None or b[2] is not None:
        assert torch.equal(_bits(a[2]), _bits(b[2])), f"{what}: ray_loss"
    if a[3] is not None or b[3] is not None:
        assert torch.equal(_bits(a[3]), _bits(b[3])), f"{what}: error map"


@pytest.fixture(scope="module")
def l1_graphed(dev):
    """accelerate(criterion="l1", error_map=) replayed: two rings of steps plus one call (the reference run the trainer tests share)."""
    return _train(dev, 33, criterion="l1")


def test_trainer_replays_the_eager_l1_step_with_a_map(dev, l1_graphed):
    eager = _train(dev, 33, criterion="l1", graph=False)
    tr = l1_graphed[4]
    assert tr._graphs is not None and tr.criterion == (L1, 0.0), "steps 19.. ran as replayed graphs"
    _equal_runs(l1_graphed, eager, "graph=True against graph=False")
    emap, ray_loss = l1_graphed[3], l1_graphed[2]
    assert torch.isfinite(ray_loss).all() and float(ray_loss.min()) >= 0 and ray_loss.shape == (2048,)
    assert abs(float(ray_loss.double().mean()) - float(l1_graphed[1][-1])) <= 1e-5 * float(l1_graphed[1][-1]), "the loss is the mean of the rays' losses"
    assert int((emap != 0.5).sum()) > 2048, "cells were updated"
    assert float(l1_graphed[1][-4:].mean()) < float(l1_graphed[1][:4].mean()), "and it trains"


def test_trainer_takes_the_reference_criterion_object(dev, l1_graphed):
    _equal_runs(l1_graphed, _train(dev, 33, criterion=torch.nn.L1Loss()), 'torch.nn.L1Loss() against "l1"')


def test_trainer_l1_with_next_rays(dev, l1_graphed):
    ahead = _train(dev, 33, ahead=True, criterion="l1")
    assert ahead[4]._side is not None, "a march ran ahead"
    _equal_runs(l1_graphed, ahead, "next_rays")


def test_trainer_l1_in_groups_of_four(dev, l1_graphed):
    """steps_per_call = 4 trains like single steps (tests/test_gpu_round4.py holds the MSE step to this): here with the L1 criterion and the
    map cells of four steps per call.  32 steps, against the first 32 of the single-step run: the maps and the parameters of step 32."""
    single = _train(dev, 32, criterion="l1")
    grouped = _train(dev, 8, k=4, ahead=True, criterion="l1")
    assert grouped[4]._groups is not None
    for n in single[0]:
        assert torch.equal(single[0][n], grouped[0][n]), n
    assert torch.equal(_bits(single[3]), _bits(grouped[3])) and torch.equal(_bits(single[2]), _bits(grouped[2]))
    assert torch.equal(_bits(single[1][3::4]), _bits(grouped[1]))
    with pytest.raises(ValueError, match="error_inds without a map"):
        _ngp_trainer(dev, criterion="l1")[1].step(*_ngp_case(dev)["rays"][0], _ngp_case(dev)["tgt"][0], error_inds=_ngp_case(dev)["inds"][0])


def test_a_skipped_step_still_updates_the_map(dev):
    """A forced overflow (the loss scale set out of fp16's range, as tests/test_gpu_round6.py forces one) inside the replayed part: the step is
    skipped -- parameters and the optimizer's step count unchanged -- and the map is updated all the same (the reference writes it before
    backward())."""
    out = _train(dev, 24, criterion="l1", overflow_at=21)
    (p0, m0, s0), (p1, m1, s1) = out[5]["before"], out[5]["after"]
    assert out[4]._graphs is not None and s1 == s0, "the step was skipped"
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n
    cells = _ngp_case(dev)["inds"][21 % 8]
    assert not torch.equal(m0.view(-1)[cells], m1.view(-1)[cells]) and float((m0 != m1).sum()) <= 2048


def test_default_trainer_is_the_mse_trainer(dev):
    """accelerate(renderer) with no new argument against criterion="mse" (the general instantiation with kind MSE, per-ray loss on): the same
    training, bit for bit; and the default makes none of the new calls."""
    plain = _train(dev, 20, use_map=False)
    assert plain[2] is None and plain[4]._loss_args(0) == {}
    mse = _train(dev, 20, use_map=False, criterion="mse")
    assert mse[2] is not None and mse[4].criterion == (MSE, 0.0)
    for n in plain[0]:
        assert torch.equal(plain[0][n], mse[0][n]), n
    assert torch.equal(_bits(plain[1]), _bits(mse[1]))


# ------------------------------------------------------------------------------------------------- 6. the curved field
def _curved_renderer(dev, like=None):
    """The smallest case of tests/test_gpu_curved_training.py."""
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer

    v, f = star_flower_mesh(n_lat=36, n_lon=72)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05).to(dev)
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    if like is not None:
        r.load_state_dict(like.state_dict())
        r.mean_density = like.mean_density
    else:
        with torch.no_grad():
            field.encoder.embeddings.uniform_(-0.5, 0.5)
            field.sigma_net.weights.mul_(3.0)
            for layer in field.encoder.cluster_layers:
                layer.cluster_centers.uniform_(-0.5, 0.5)
        with torch.autocast("cuda", dtype=torch.float16):
            r.update_extra_state_device()
    field.train()
    return field, r


def test_curved_trainer_with_the_reference_criterion(dev):
    """CurvedTrainer(criterion="l1") -- main.py:187's -- replayed against eager, bit for bit (three-launch tail under GradScaler), and the first
    step's image loss against F.l1_loss in float64 of the step's own image."""
    from ngp_harness import scene
    from ngp_harness.accelerate import CurvedTrainer, accelerate

    N = 2048
    rays = []
    for i in range(6):
        o, d = scene.train_batch(N, seed=300 + i, radius=1.6)
        rays.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
    tgt = torch.rand(6, N, 3, generator=torch.Generator().manual_seed(300)).to(dev) * 0.2 + 0.4
    inds = torch.stack([torch.randperm(4 * N, generator=torch.Generator().manual_seed(i))[:N] for i in range(6)]).to(dev)
    _, r0 = _curved_renderer(dev)

    # the first step's image, by the renderer itself (no perturbation: the trainer's first step marches the same samples)
    _, ra = _curved_renderer(dev, like=r0)
    ray_loss0 = torch.empty(N, device=dev)
    with torch.autocast("cuda", dtype=torch.float16):
        image, _, loss0, _, _ = ra.render_train(*rays[0], dt_gamma=1 / 128, bg_color=1, perturb=False, max_steps=1024, target=tgt[0], criterion="l1",
                                                ray_loss=ray_loss0)
    want = float(F.l1_loss(image.double(), tgt[0].double()))
    print(f"curved, first step: L1 loss {loss0.item():.9g} float64 {want:.9g}")
    assert abs(loss0.item() - want) <= 1e-5 * want

    def run(graph):
        field, r = _curved_renderer(dev, like=r0)
        emap = torch.zeros(4 * N, device=dev)
        tr = accelerate(r, graph=graph, perturb=False, criterion="l1", error_map=emap)
        assert isinstance(tr, CurvedTrainer)
        np.random.seed(7)
        losses, first = [], None
        for i in range(24):
            losses.append(tr.step(*rays[i % 6], tgt[i % 6], error_inds=inds[i % 6]).clone())
            if i == 0:
                first = (tr.ray_loss.clone(), (tr.loss - tr.reg_loss).clone())
        torch.cuda.synchronize()
        return torch.stack(losses), tr, field, emap, first

    eager, graphed = run(False), run(True)
    assert graphed[1]._graphs is not None, "the later steps ran as replayed graphs"
    assert torch.equal(_bits(graphed[4][0]), _bits(ray_loss0)), "the trainer's first step is the step whose image was checked"
    assert abs(float(graphed[4][1]) - want) <= (1e-5 + 4 * EPS) * want  # (loss + regulariser - regulariser: one more rounding pair)
    assert torch.equal(_bits(eager[0]), _bits(graphed[0])), "losses"
    for (n, a), (_, b) in zip(graphed[2].named_parameters(), eager[2].named_parameters()):
        assert torch.equal(a.detach(), b.detach()), n
    assert torch.equal(_bits(eager[3]), _bits(graphed[3])) and torch.equal(_bits(eager[1].ray_loss), _bits(graphed[1].ray_loss))
    assert int((graphed[3] != 0).sum()) > N
