"""GPU: the SH light head (csrc/shlight.inc behind ngp_harness.light.SHLightNet and CurvedField(light_model="SH")).

  * nerftex_sh_light_forward / _backward through the C ABI against the float64 restatement of tests/sh_light_float64.py and its per-element
    bounds, at wave and workgroup edges, white and coloured light, with and without the specular term and the mask; the half sigmoids bit for
    bit; zeros where the contract says zero; the lighting gradient's bits run to run and beside a busy second stream; B == 0;
  * the op-by-op path on the same GPU under the same bounds (a bound the framework's own fp32 ops miss would be a wrong bound);
  * the autograd Function behind SHLightNet against the op-by-op path;
  * CurvedField(light_model="SH"): train and eval, fused head and fused = False, the inference loops, the accelerated trainer.
Every comparison prints its largest error-to-bound ratio and the share of elements excluded as kink bands (DESIGN.md 4.13 records them)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sh_light_float64 as f64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINK_CAP = 0.02
SIZES = (1, 63, 64, 65, 255, 256, 257, 4099)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(dev, B, C, seed, dark=False, marker=False):
    """brdf rows as the BRDF MLP leaves them (16 wide, columns 5.. arbitrary), unit normals, view directions of lengths 0.5..2 -- one of them the
    march's unused-slot marker where asked for --, the reference's DC term of 3 with small higher bands (dark: a DC of 0.05 under bands of 0.4)."""
    rng = np.random.default_rng(seed)
    brdf = torch.from_numpy(rng.normal(0, 2.0, (B, 16)).astype(np.float16))
    n = rng.normal(size=(B, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    d = rng.normal(size=(B, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.5, 2.0, (B, 1))).astype(np.float32)
    marker = B // 2 if marker else None
    if marker is not None:
        d[marker] = (1e30, 0.0, 0.0)  # (|d| overflows in fp32: the row's values are not float64's, they only have to be finite)
    env = rng.normal(0, 0.4 if dark else 0.1, (16, C)).astype(np.float32)
    env[0] = 0.05 if dark else 3.0
    mask = rng.uniform(size=B) < 0.7
    gc = rng.normal(size=(B, 3)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return dict(brdf=brdf.to(dev), n=t(n), d=t(d), env=t(env), mask=t(mask), gc=t(gc), marker=marker)


def _desc(p, spec, masked, outs=None, grads=None, gamma=2.4):
    from nerftex_hip import SH_LIGHT_SPECULAR, SHLightDesc, ptr

    kw = {}
    if outs is not None:
        kw.update(color=ptr(outs[0]), specular=ptr(outs[1]), diffuse=ptr(outs[2]), albedo=ptr(outs[3]))
    if grads is not None:
        g_color, g_brdf, g_env, scratch = grads
        kw.update(grad_color=ptr(g_color), grad_brdf=ptr(g_brdf), grad_env_shs=ptr(g_env), scratch=ptr(scratch), scratch_bytes=scratch.numel())
    mask_b = p["mask"].view(torch.uint8) if masked else None
    return SHLightDesc(brdf=ptr(p["brdf"]), brdf_stride=p["brdf"].stride(0), normals=ptr(p["n"]), dirs=ptr(p["d"]), env_shs=ptr(p["env"]), n_sh=p["env"].shape[0],
                       n_color=p["env"].shape[1], mask=ptr(mask_b), B=p["brdf"].shape[0], gamma=gamma, flags=SH_LIGHT_SPECULAR if spec else 0, **kw)


def _forward(p, spec, masked):
    from nerftex_hip import check, lib, stream

    B = p["brdf"].shape[0]
    outs = torch.full((4, B, 3), float("nan"), dtype=torch.float32, device=p["brdf"].device)
    desc = _desc(p, spec, masked, outs=outs)
    check(lib.nerftex_sh_light_forward(ctypes.byref(desc), stream()))
    return outs


def _backward(p, spec, masked, g_color=None, scratch_fill=None):
    from nerftex_hip import check, lib, stream

    B, dev = p["brdf"].shape[0], p["brdf"].device
    g_brdf = torch.full((B, 16), float("nan"), dtype=torch.float16, device=dev)
    g_env = torch.full_like(p["env"], float("nan"))
    scratch = torch.empty(lib.nerftex_sh_light_scratch_bytes(B), dtype=torch.uint8, device=dev)
    if scratch_fill is not None:
        scratch.fill_(scratch_fill)
    desc = _desc(p, spec, masked, grads=(p["gc"] if g_color is None else g_color, g_brdf, g_env, scratch))
    check(lib.nerftex_sh_light_backward(ctypes.byref(desc), stream()))
    return g_brdf, g_env


def _reference(p, spec, masked, with_grad=False, g_color=None):
    """float64 from the half sigmoids torch.sigmoid gives on this GPU."""
    a_h = torch.sigmoid(p["brdf"][:, :3]).cpu().numpy()
    sw_h = torch.sigmoid(p["brdf"][:, 3:4]).cpu().numpy()
    gc = (p["gc"] if g_color is None else g_color).cpu().numpy() if with_grad else None
    return f64.shade(a_h, sw_h, p["n"].cpu().numpy(), p["d"].cpu().numpy(), p["env"].cpu().numpy(), 2.4, spec, p["mask"].cpu().numpy() if masked else None, gc)


def _inside(name, got, want, bound, kink, cap=KINK_CAP):
    got = np.asarray(got, np.float64)
    assert np.isfinite(want).all() and np.isfinite(bound).all(), name  # (nothing is excused by an overflowing reference or bound)
    keep = ~kink
    err = np.abs(got - want)[keep]
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound[keep], 1e-300))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{name}: max error / bound {worst:.3f}, excluded {kink.mean():.4%}")
    assert kink.mean() <= cap, (name, float(kink.mean()))
    assert worst <= 1.0, (name, worst)


COMBOS = [(C, spec, masked) for C in (1, 3) for spec in (True, False) for masked in (False, True)]


@pytest.mark.parametrize("B", SIZES)
def test_forward_through_the_c_abi(dev, B):
    from ngp_harness.light import sh_light_shade

    for C, spec, masked in COMBOS:
        p = _inputs(dev, B, C, seed=100 + B, marker=B >= 63)  # (one row of 63 is inside the 2 % cap; the single row of B = 1 is compared)
        outs = _forward(p, spec, masked).cpu().numpy()
        ref = _reference(p, spec, masked)
        if p["marker"] is not None:
            for key in ("color", "specular"):
                ref["kink_" + key][p["marker"]] = True
        live = p["mask"].cpu().numpy() if masked else np.ones(B, bool)
        assert np.isfinite(outs).all(), "every row is written, the marked direction's included"
        assert not outs[:, ~live].any(), "masked rows are exactly 0"
        want_albedo = torch.sigmoid(p["brdf"][:, :3]).float().cpu().numpy()
        assert np.array_equal(outs[3][live].view(np.int32), want_albedo[live].view(np.int32)), "the half sigmoid, bit for bit"
        with torch.no_grad():
            ops = sh_light_shade(p["brdf"], p["n"], p["d"], p["env"], spec, 2.4, p["mask"] if masked else None)
        tag = f"B={B} C={C} spec={int(spec)} mask={int(masked)}"
        for i, key in enumerate(("color", "specular", "diffuse", "albedo")):
            _inside(f"forward kernel {key} | {tag}", outs[i], ref[key], ref["bound_" + key], ref["kink_" + key])
            _inside(f"forward op-by-op {key} | {tag}", ops[i].float().cpu().numpy(), ref[key], ref["bound_" + key], ref["kink_" + key])


def test_forward_dark_lighting_agrees_outside_the_kink_bands(dev):
    p = _inputs(dev, 4099, 3, seed=7, dark=True)
    outs = _forward(p, True, False).cpu().numpy()
    ref = _reference(p, True, False)
    floor = (ref["color"] <= (1e-6) ** (1 / 2.4) * (1 + 1e-6)).mean()
    assert floor > 0.05, floor  # the clamps and safe_pow's floor are reached
    for i, key in enumerate(("color", "specular", "diffuse")):
        _inside(f"forward dark {key}", outs[i], ref[key], ref["bound_" + key], ref["kink_" + key])


@pytest.mark.parametrize("B", (1, 65, 257, 4099))
def test_backward_through_the_c_abi(dev, B):
    for C, spec, masked in COMBOS:
        p = _inputs(dev, B, C, seed=200 + B)
        g_brdf, g_env = _backward(p, spec, masked)
        ref = _reference(p, spec, masked, with_grad=True)
        gb, ge = g_brdf.float().cpu().numpy(), g_env.cpu().numpy()
        live = p["mask"].cpu().numpy() if masked else np.ones(B, bool)
        assert np.isfinite(gb).all() and np.isfinite(ge).all()
        assert not gb[:, 4:].any(), "the glossiness and the padding columns receive exactly 0"
        assert not gb[~live].any(), "masked rows receive exactly 0"
        assert not ge[9:].any(), "the bands the head does not read receive exactly 0"
        if not spec:
            assert not gb[:, 3].any()
        tag = f"B={B} C={C} spec={int(spec)} mask={int(masked)}"
        rows = np.broadcast_to(ref["kink_g"][:, None], (B, 3))
        _inside(f"backward kernel grad_brdf albedo | {tag}", gb[:, :3], ref["g_albedo_h"], ref["bound_g_albedo_h"], rows)
        _inside(f"backward kernel grad_brdf spec_w | {tag}", gb[:, 3:4], ref["g_spec_w_h"], ref["bound_g_spec_w_h"], ref["kink_g"][:, None])
        _inside(f"backward kernel grad_env | {tag}", ge, ref["grad_env"], ref["bound_grad_env"], np.zeros(ge.shape, bool))


def test_backward_scaled_gradient_is_not_clamped(dev):
    """grad_color x 65536 (a loss scaler's factor): the lighting gradient scales exactly (a power of two commutes with every fp32 rounding of the
    chain), and grad_brdf is the scaled gradient's fp16 sigmoid backward -- infinite where the half range ends, as the framework's is, not
    saturated."""
    p = _inputs(dev, 4099, 3, seed=31)
    _, ge1 = _backward(p, True, False)
    gb, ge = _backward(p, True, False, g_color=p["gc"] * 65536.0)
    assert torch.equal(ge, ge1 * 65536.0)
    ref = _reference(p, True, False, with_grad=True, g_color=p["gc"] * 65536.0)
    gbn = gb.float().cpu().numpy()
    # the overflow is in the cast of the fp32 gradient to half, in front of the sigmoid backward's (1 - y) y
    a = torch.sigmoid(p["brdf"][:, :3]).double().cpu().numpy()
    inner = (a > 0) & (a < 1) & ~ref["kink_g"][:, None]
    ga = np.where(inner, ref["g_albedo_h"] / np.where(inner, (1 - a) * a, 1.0), 0.0)
    big = inner & (np.abs(ga) > 65504 * 1.01)
    assert big.mean() > 0.01 and np.isinf(gbn[:, :3][big]).all(), "past the half range the gradient is infinite, as autograd's cast makes it"
    ok = inner & (np.abs(ga) < 65504 * 0.99)
    assert ok.mean() > 0.3 and np.isfinite(gbn[:, :3][ok]).all()
    assert (np.abs(gbn[:, :3][ok] - ref["g_albedo_h"][ok]) <= ref["bound_g_albedo_h"][ok]).all()
    assert float(np.abs(gbn[:, :3][ok]).max()) > 1000  # far above what an unscaled gradient reaches


def test_backward_is_deterministic_alone_and_beside_a_busy_stream(dev):
    p = _inputs(dev, 4099, 3, seed=41)
    gb0, ge0 = _backward(p, True, True, scratch_fill=0)
    gb1, ge1 = _backward(p, True, True, scratch_fill=255)  # (what the scratch held does not matter: it is written before it is read)
    assert torch.equal(gb0.view(torch.int16), gb1.view(torch.int16)) and torch.equal(ge0.view(torch.int32), ge1.view(torch.int32))
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            a = torch.tanh(a @ a * 1e-3)
    gb2, ge2 = _backward(p, True, True)
    torch.cuda.synchronize()
    assert torch.equal(gb0.view(torch.int16), gb2.view(torch.int16)) and torch.equal(ge0.view(torch.int32), ge2.view(torch.int32))


def test_empty_batch_contract(dev):
    from nerftex_hip import SHLightDesc, check, lib, ptr, stream

    env = torch.ones(16, 3, device=dev)
    g_env = torch.full_like(env, float("nan"))
    desc = SHLightDesc(brdf_stride=16, env_shs=ptr(env), n_sh=16, n_color=3, B=0, gamma=2.4, flags=1, grad_env_shs=ptr(g_env))
    check(lib.nerftex_sh_light_forward(ctypes.byref(desc), stream()))
    check(lib.nerftex_sh_light_backward(ctypes.byref(desc), stream()))
    assert not g_env.any(), "B == 0: the lighting gradient is written as 0"
    for bad in (dict(n_sh=8), dict(n_color=2), dict(brdf_stride=4), dict(gamma=0.0), dict(flags=2)):
        kw = dict(brdf_stride=16, env_shs=ptr(env), n_sh=16, n_color=3, B=0, gamma=2.4, flags=1, grad_env_shs=ptr(g_env))
        kw.update(bad)
        assert lib.nerftex_sh_light_forward(ctypes.byref(SHLightDesc(**kw)), stream()) != 0, bad
        assert lib.nerftex_last_error()
    kw = dict(brdf_stride=16, env_shs=ptr(env), n_sh=16, n_color=3, B=64, gamma=2.4, flags=1)
    assert lib.nerftex_sh_light_forward(ctypes.byref(SHLightDesc(**kw)), stream()) != 0, "NULL buffers are refused before anything is launched"


@pytest.mark.parametrize("white", (True, False))
def test_autograd_fused_against_op_by_op(dev, white):
    """SHLightNet with the fused head and with fused = False from the same geometry features: the colour, the gradient that reaches the BRDF
    MLP's output and the lighting gradient of both inside the float64 bounds; the BRDF weights' gradients of the two paths then differ by what
    the MLP's backward makes of half-ulp differences in its input gradient."""
    from ngp_harness.light import SHLightNet

    B = 1000
    p = _inputs(dev, B, 1 if white else 3, seed=51)
    torch.manual_seed(3)
    net = SHLightNet(white_light=white).to(dev).train()
    with torch.no_grad():
        net.envSHs.copy_(p["env"])
    geo = torch.randn(B, 15, device=dev).half()
    got = {}
    for fused in (True, False):
        net.fused = fused
        net.zero_grad(set_to_none=True)
        seen = {}
        handle = net.brdf_layer.register_forward_hook(lambda m, i, o: (o.retain_grad(), seen.__setitem__("brdf", o))[1])
        with torch.autocast("cuda", dtype=torch.float16):
            color, specular, diffuse, albedo = net(geo, p["n"], p["d"], mask=p["mask"])
            (color * p["gc"]).sum().backward()
        handle.remove()
        assert color.dtype == torch.float32 and seen["brdf"].dtype == torch.float16 and seen["brdf"].shape == (B, 5)
        got[fused] = dict(brdf=seen["brdf"].detach(), color=color.detach(), specular=specular.detach().float(), diffuse=diffuse.detach(), albedo=albedo.detach().float(),
                          g_brdf=seen["brdf"].grad.clone(), g_env=net.envSHs.grad.clone(), g_w=net.brdf_layer.weights.grad.clone())
    assert torch.equal(got[True]["brdf"], got[False]["brdf"])
    q = dict(p, brdf=got[True]["brdf"])
    ref = _reference(q, True, True, with_grad=True)
    rows = np.broadcast_to(ref["kink_g"][:, None], (B, 3))
    for fused in (True, False):
        g, name = got[fused], "fused" if fused else "op-by-op"
        for key in ("color", "specular", "diffuse", "albedo"):
            _inside(f"autograd {name} {key} | white={int(white)}", g[key].cpu().numpy(), ref[key], ref["bound_" + key], ref["kink_" + key])
        gb = g["g_brdf"].float().cpu().numpy()
        assert not gb[:, 4].any()
        _inside(f"autograd {name} grad_brdf albedo | white={int(white)}", gb[:, :3], ref["g_albedo_h"], ref["bound_g_albedo_h"], rows)
        _inside(f"autograd {name} grad_brdf spec_w | white={int(white)}", gb[:, 3:4], ref["g_spec_w_h"], ref["bound_g_spec_w_h"], ref["kink_g"][:, None])
        _inside(f"autograd {name} grad_env | white={int(white)}", g["g_env"].cpu().numpy(), ref["grad_env"], ref["bound_grad_env"], np.zeros((16, 1 if white else 3), bool))
    same = float((got[True]["g_brdf"] == got[False]["g_brdf"]).float().mean())
    print(f"grad_brdf elements equal between the paths: {same:.4%}")
    assert same > 0.99
    gw, gw_ops = got[True]["g_w"].float(), got[False]["g_w"].float()
    assert float((gw - gw_ops).abs().max()) <= 2e-2 * float(gw_ops.abs().max()) and float(gw_ops.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------------------ the field
def _sh_field(dev, **kw):
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05, **kw).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
        if field.normal_net is not None:
            field.normal_net.encoder.embeddings.uniform_(-0.5, 0.5)
    return field, v


@pytest.fixture(scope="module")
def sh_setup(dev):
    field, v = _sh_field(dev, light_model="SH")
    with torch.no_grad():
        field.light_net.envSHs[1:].normal_(0, 0.1)
    rng = np.random.default_rng(5)
    n = 2048
    ids = 36 + np.arange(n) % (v.shape[0] - 72)
    vn = field.projector.vertex_normals.cpu().numpy()
    x = (v[ids] + rng.uniform(-0.1, 0.1, size=(n, 1)).astype(np.float32) * vn[ids]).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return dict(field=field, x=torch.from_numpy(x).to(dev), d=torch.from_numpy(d).to(dev))


def test_field_without_a_light_model_is_todays_field(dev):
    field, _ = _sh_field(dev)
    assert [n for n, _ in field.named_children()] == ["projector", "encoder", "sigma_net", "encoder_dir", "color_net"]
    assert [n for n, _ in field.named_parameters() if not n.startswith("encoder.cluster_layers")] == ["encoder.embeddings", "sigma_net.weights", "color_net.weights"]
    assert field.light_model is None and field.normal_net is None and len(field.graph_stamp()) == 11
    sh, _ = _sh_field(dev, light_model="SH")
    assert sh.color_net is None and sh.encoder_dir is None and sh.normal_net is not None and sh.light_net.envSHs.shape == (16, 1)
    assert len(sh.graph_stamp()) > 11 and {"light_net.envSHs", "light_net.brdf_layer.weights"} <= {n for n, _ in sh.named_parameters()}
    assert {id(q) for g in sh.get_params(1e-2) for q in g["params"]} >= {id(sh.light_net.envSHs), id(sh.light_net.brdf_layer.weights)}


@pytest.mark.parametrize("mode", ("train", "eval"))
def test_field_shades_with_the_light_head(dev, sh_setup, mode):
    """forward(x, d) of the SH field: what reaches the head (geometry features, the shading normal -- fine and detached in training, the
    fc_weight blend in eval --, the direction, the height mask) is captured, and the colour of the fused head and of fused = False both lie
    inside the float64 bounds of those inputs; sigma is density()'s; masked samples are exactly 0."""
    field, x, d = sh_setup["field"], sh_setup["x"], sh_setup["d"]
    field.train(mode == "train")
    field.fc_weight = 0.7
    seen = {}
    handle = field.light_net.register_forward_pre_hook(lambda m, a, k: seen.update(geo=a[0], n=a[1], d=a[2], mask=k["mask"]), with_kwargs=True)
    out = {}
    try:
        for fused in (True, False):
            field.light_net.fused = fused
            with torch.autocast("cuda", dtype=torch.float16), torch.set_grad_enabled(mode == "train"):
                sigma, color, extra = field(x, d)
                dens = field.density(x)
            out[fused] = (sigma.detach(), color.detach())
            assert extra == {} and color.shape == (x.shape[0], 3)
            assert torch.equal(sigma, dens["sigma"])
    finally:
        handle.remove()
        field.light_net.fused = True
    mask = seen["mask"]
    inside = float(mask.float().mean())
    assert 0.2 < inside < 0.8, inside
    assert not seen["n"].requires_grad and torch.equal(seen["d"], d)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        fine, coarse, _ = field.fine_normal(x)
        fine = fine / (fine.norm(dim=-1, keepdim=True) + 1e-5)
        if mode == "eval":
            coarse = coarse / (coarse.norm(dim=-1, keepdim=True) + 1e-5)
            fine = 0.7 * fine + (1 - 0.7) * coarse
            fine = fine / (fine.norm(dim=-1, keepdim=True) + 1e-5)
        ones = torch.ones(x.shape[0], 1, dtype=seen["geo"].dtype, device=dev)
        brdf = field.light_net.brdf_layer(torch.cat([seen["geo"].detach(), ones], dim=-1))
    assert torch.allclose(seen["n"], fine, atol=1e-6)
    p = dict(brdf=brdf, n=seen["n"].detach().float(), d=d, env=field.light_net.envSHs.detach(), mask=mask)
    ref = _reference(p, True, True)
    for fused in (True, False):
        sigma, color = out[fused]
        assert not color[~mask].any() and not sigma[~mask].any() and float(sigma.max()) > 0
        _inside(f"field {mode} {'fused' if fused else 'op-by-op'} colour", color.float().cpu().numpy(), ref["color"], ref["bound_color"], ref["kink_color"])
    try:
        if mode == "eval":
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                for name in ("Specular", "Diffuse", "Albedo"):
                    field.light_visual_mode = name
                    c = field(x, d)[1]
                    key = name.lower()
                    _inside(f"field eval {name}", c.float().cpu().numpy(), ref[key], ref["bound_" + key], ref["kink_" + key])
    finally:
        field.light_visual_mode, field.fc_weight = "Full", 1.0


def test_field_normal_supervision(dev, sh_setup):
    """forward(x, d, normal_supervision=True) in training: 'normal' is the fine normal on the graph, 'normal_grad' the detached blend
    0.9 density normal + 0.1 coarse normal, renormalised; in eval the dict stays empty."""
    field, x, d = sh_setup["field"], sh_setup["x"][:512], sh_setup["d"][:512]
    field.train()
    with torch.autocast("cuda", dtype=torch.float16):
        sigma, color, extra = field(x, d, normal_supervision=True)
        _, ng, hm = field.density_normal(x)
        fine, coarse, _ = field.fine_normal(x)
    assert set(extra) == {"normal", "normal_grad"} and extra["normal"].requires_grad and not extra["normal_grad"].requires_grad
    assert torch.allclose(extra["normal"], fine, atol=1e-6)
    want = ng * 0.9 + coarse * 0.1
    want = want / (want.norm(dim=-1, keepdim=True) + 1e-5)
    ok = hm & torch.isfinite(want).all(-1)
    assert float(ok.float().mean()) > 0.2 and torch.allclose(extra["normal_grad"][ok], want[ok], atol=1e-5)
    assert not sigma[~hm].any() and not color[~hm].any()
    (color.sum() + (extra["normal"] * extra["normal_grad"].nan_to_num()).sum()).backward()
    assert field.light_net.envSHs.grad.abs().sum() > 0 and field.light_net.brdf_layer.weights.grad.abs().sum() > 0
    assert sum(float(q.grad.abs().sum()) for q in field.normal_net.parameters() if q.grad is not None) > 0
    field.zero_grad(set_to_none=True)
    field.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert field(x, d, normal_supervision=True)[2] == {}


def test_inference_loops_render_the_light_field(dev, sh_setup):
    """A light-model field is not the fused inference entry's: infer() and the two loops go through forward() and give the reference loop's image."""
    from ngp_harness import scene
    from ngp_harness.model import Renderer

    field = sh_setup["field"].eval()
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        r.update_extra_state_device()
    o, d = scene.get_rays(scene.rand_poses(1, 1.6, np.random.default_rng(11))[0], scene.intrinsics(32, 32), 32, 32)
    ro, rd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    kw = dict(dt_gamma=0.0, max_steps=256)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert not field._infer_fused(sh_setup["x"], sh_setup["d"])
        img, dep, _ = r.render_infer(ro, rd, slots_per_ray=4, **kw)
        img_p, dep_p, _ = r.render_infer_pipelined(ro, rd, slots_per_ray=4, parts=2, **kw)
        img_g, dep_g, _ = r.render_infer_graphed(ro, rd, slots_per_ray=4, parts=2, block=2, **kw)
    assert float(img.std()) > 1e-3
    assert torch.equal(img_p, img) and torch.equal(dep_p, dep)
    assert torch.equal(img_g, img) and torch.equal(dep_g, dep)


def test_accelerated_trainer_trains_the_light_field(dev):
    """accelerate() over the SH field with main.py's trainer configuration and the normal supervision: three replayed calls of two steps equal
    three eager calls bit for bit in every parameter; the lighting, the BRDF weights, the table, the sigma net and the normal net have moved;
    the bands the head does not read have not; without normal_loss the normal net stays where it was (the head shades with the detached
    normal) while the rest still trains.  2048 rays on the 36 x 72 mesh, as tests/test_gpu_curved_training.py: below 16384 samples the hash table's gradient is summed
    with float atomics (csrc/gridencoder.hip kOwnerMinBatch) and its bits are not reproducible, whatever the field behind it."""
    from ngp_harness import scene
    from ngp_harness.accelerate import accelerate
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer

    N, k = 2048, 2
    v, f = star_flower_mesh(n_lat=36, n_lon=72)

    def build():
        torch.manual_seed(0)
        field = CurvedField(v, f, bound=1.0, h_threshold=0.05, light_model="SH").to(dev)
        with torch.no_grad():
            field.encoder.embeddings.uniform_(-0.5, 0.5)
            field.sigma_net.weights.mul_(3.0)
            field.light_net.envSHs[1:].normal_(0, 0.1, generator=torch.Generator(device=dev).manual_seed(1))
            for layer in field.encoder.cluster_layers:
                layer.cluster_centers.uniform_(-0.5, 0.5)
        r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
        with torch.autocast("cuda", dtype=torch.float16):
            r.update_extra_state_device()
        field.train()
        return field, r

    rays = []
    for i in range(k * 3):
        o, d = scene.train_batch(N, seed=300 + i, radius=1.6)
        rays.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
    tgt = (torch.rand(k * 3, N, 4, generator=torch.Generator().manual_seed(9)) * 0.5 + 0.25).to(dev)

    def run(graph, normal_loss=True, k=k, calls=3):
        field, r = build()
        start = {n: q.detach().clone() for n, q in field.named_parameters()}
        tr = accelerate(r, graph=graph, perturb=False, criterion="l1", bg_color="random", target_channels=4, ema_decay=0.95, steps_per_call=k,
                        normal_loss=normal_loss, bg_generator=torch.Generator(device=dev).manual_seed(5))
        np.random.seed(7)
        for c in range(calls):
            if k == 1:
                loss = tr.step(*rays[c], tgt[c].contiguous())
                continue
            o = torch.stack([rays[c * k + j][0] for j in range(k)]).contiguous()
            d = torch.stack([rays[c * k + j][1] for j in range(k)]).contiguous()
            loss = tr.step_group(o, d, tgt[c * k:(c + 1) * k].contiguous())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss).all())
        assert tr.normal_loss.is_cuda and tr.normal_loss.shape == () and (float(tr.normal_loss) != 0) == normal_loss
        if normal_loss:
            import math

            assert -math.cos(math.pi / 8) - 1e-6 <= float(tr.normal_loss) <= 1.0
        return field, start

    fe, _ = run(False)
    fg, start = run(True)
    moved = {}
    for (n, a), (_, b) in zip(fg.named_parameters(), fe.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), n
        moved[n] = float((a.detach() - start[n]).abs().max())
    print("moved:", {n: m for n, m in moved.items() if not n.startswith("encoder.cluster")})
    env, env0 = fg.light_net.envSHs.detach(), start["light_net.envSHs"]
    assert moved["light_net.envSHs"] > 0 and torch.equal(env[9:], env0[9:]) and moved["light_net.brdf_layer.weights"] > 0
    assert moved["encoder.embeddings"] > 0 and moved["sigma_net.weights"] > 0
    normal_names = [n for n in moved if n.startswith("normal_net.")]
    # (its table and its weight matrices; a Lipschitz constant whose row scale is not active has a zero gradient)
    assert moved["normal_net.encoder.embeddings"] > 0 and sum(moved[n] > 0 for n in normal_names) >= 3, {n: moved[n] for n in normal_names}
    fp, start = run(True, normal_loss=False)
    plain = {n: float((q.detach() - start[n]).abs().max()) for n, q in fp.named_parameters()}
    assert all(plain[n] == 0 for n in normal_names), "without the supervision nothing reaches the normal net"
    assert plain["light_net.envSHs"] > 0 and plain["light_net.brdf_layer.weights"] > 0 and plain["encoder.embeddings"] > 0
    # "differs only through the normal net's path", in the form in which it holds: the supervision's gradient enters the normal net and, through
    # the texture features the normal net reads, the shared hash table -- so from the second step on every parameter differs.  After exactly ONE
    # step the lighting, the BRDF MLP and the sigma net are bit for bit what the run without the supervision has; the table and the normal net
    # are not.
    one_on, _ = run(False, normal_loss=True, k=1, calls=1)
    one_off, _ = run(False, normal_loss=False, k=1, calls=1)
    for (n, a), (_, b) in zip(one_on.named_parameters(), one_off.named_parameters()):
        if n.startswith(("light_net.", "sigma_net.")):
            assert torch.equal(a.detach(), b.detach()), n
    assert not torch.equal(one_on.encoder.embeddings.detach(), one_off.encoder.embeddings.detach())
    assert not torch.equal(one_on.normal_net.encoder.embeddings.detach(), one_off.normal_net.encoder.embeddings.detach())


def test_shade_train_refuses_extras_of_a_field_without_a_light_model(dev):
    from ngp_harness.model import Renderer

    field, _ = _sh_field(dev)
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    z = torch.zeros(4, 3, device=dev)
    with pytest.raises(ValueError, match="normal supervision"):
        r.shade_train((None, None, z, z, z[:, :2], None), extras_out={})


def test_fused_head_marks_the_viewer_outputs_non_differentiable(dev):
    """Only `color` carries a gradient on the fused path: specular, diffuse and albedo come out with requires_grad False, so a loss on them is
    refused by autograd instead of being dropped."""
    from ngp_harness.light import _SHLight

    p = _inputs(dev, 257, 3, seed=61)
    brdf = p["brdf"][:, :5].detach().requires_grad_(True)
    env = p["env"].detach().requires_grad_(True)
    color, specular, diffuse, albedo = _SHLight.apply(brdf, p["n"], p["d"], env, p["mask"], 2.4, True)
    assert color.requires_grad and not specular.requires_grad and not diffuse.requires_grad and not albedo.requires_grad
    with pytest.raises(RuntimeError):
        specular.sum().backward()
    color.sum().backward()
    assert brdf.grad is not None and brdf.grad.shape == (257, 5) and env.grad is not None


def test_backward_beyond_one_sample_per_thread(dev):
    """B > 1024 blocks x 256 threads: the backward's grid is capped and a thread adds several samples (a training step shades ~4.6e5).  The
    gradients against float64 and the lighting gradient's bits from two runs."""
    B = 262144 + 40000 + 3
    p = _inputs(dev, B, 1, seed=71)
    gb0, ge0 = _backward(p, True, True, scratch_fill=0)
    gb1, ge1 = _backward(p, True, True, scratch_fill=255)
    assert torch.equal(ge0.view(torch.int32), ge1.view(torch.int32)) and torch.equal(gb0.view(torch.int16), gb1.view(torch.int16))
    ref = _reference(p, True, True, with_grad=True)
    gb, ge = gb0.float().cpu().numpy(), ge0.cpu().numpy()
    live = p["mask"].cpu().numpy()
    assert not gb[:, 4:].any() and not gb[~live].any() and not ge[9:].any()
    rows = np.broadcast_to(ref["kink_g"][:, None], (B, 3))
    _inside("backward large grad_brdf albedo", gb[:, :3], ref["g_albedo_h"], ref["bound_g_albedo_h"], rows)
    _inside("backward large grad_brdf spec_w", gb[:, 3:4], ref["g_spec_w_h"], ref["bound_g_spec_w_h"], ref["kink_g"][:, None])
    _inside("backward large grad_env", ge, ref["grad_env"], ref["bound_grad_env"], np.zeros(ge.shape, bool))


# ------------------------------------------------------------------------------------------------------ against the reference's modules, executed
@pytest.mark.parametrize("case", ("w1s1", "w0s1", "w0s0"))
def test_module_with_the_references_weights(dev, case):
    """SHLightNet.forward with the BRDF MLP weights, the lighting and the geometry features of tests/golden/ref_python_sh_light.npz: the MLP's
    five outputs as the reference's head saw them (its tcnn stand-in pads the 15 features with ones to 16: a wrong padding value or a wrong
    wiring moves every output), the colour, and the gradient of the BRDF weights.  The MLP runs on the MFMA kernels here and on the oracle's C
    loops in the fixture: fp32 accumulation in another order, then one rounding to half per layer -- an output may land on the neighbouring half
    (one ulp: 2^-10 of its magnitude at most) and a hidden activation that did so moves it by a fraction of another: two ulps, 2^-9 relative
    (absolute below 1); the weight gradient within 4e-2 of its largest entry as for the curved field's networks
    (tests/test_gpu_round3.py BAR_CURVED)."""
    from ngp_harness.light import SHLightNet

    g = np.load(os.path.join(GOLDEN, "ref_python_sh_light.npz"))
    t = lambda k: torch.from_numpy(g[f"{case}_{k}"]).to(dev)  # noqa: E731
    net = SHLightNet(white_light=case[1] == "1", use_specular=case[3] == "1").to(dev).train()
    with torch.no_grad():
        net.brdf_layer.weights.copy_(t("w_brdf"))
        net.envSHs.copy_(t("env_shs"))
    for fused in (True, False):
        net.fused = fused
        net.zero_grad(set_to_none=True)
        seen = {}
        handle = net.brdf_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("brdf", o))
        with torch.autocast("cuda", dtype=torch.float16):
            color = net(t("geo_feat"), t("normals"), t("dirs"))[0]
            (color * t("grad_color")).sum().backward()
        handle.remove()
        brdf, want = seen["brdf"].detach().float().cpu().numpy(), g[f"{case}_brdf"].astype(np.float32)
        err = np.abs(brdf - want) / np.maximum(np.abs(want), 1.0)
        gw, gw_want = net.brdf_layer.weights.grad.float().cpu().numpy(), g[f"{case}_g_w_brdf"]
        rel = float(np.abs(gw - gw_want).max() / np.abs(gw_want).max())
        cerr = float(np.abs(color.detach().cpu().numpy() - g[f"{case}_color"]).max())
        print(f"{case} fused={fused}: brdf equal {np.mean(brdf == want):.4%}, max err {err.max():.2e}; colour max err {cerr:.2e}; g_w_brdf rel {rel:.2e}")
        assert err.max() <= 2.0 ** -9
        # a brdf error e moves a sigmoid by at most e / 4 and the colour (irradiance <= ~1.1 pi here, tone map slope <= ~0.5 above 0.5) by less than e
        assert cerr <= 2.0 ** -9 * float(np.abs(want).max())
        assert rel <= 4e-2
        ge = net.envSHs.grad.cpu().numpy()
        assert np.abs(ge - g[f"{case}_g_env_shs"]).max() <= 1e-2 * np.abs(g[f"{case}_g_env_shs"]).max()


def _field_from_fixture(dev):
    from ngp_harness.curved import CurvedField

    g = np.load(os.path.join(GOLDEN, "ref_python_curvedfield_sh.npz"))
    c = np.load(os.path.join(GOLDEN, "ref_python_curvedfield.npz"))
    p = np.load(os.path.join(GOLDEN, "ref_python_projector.npz"))
    field = CurvedField(p["vertices"], p["faces"], bound=1.0, h_threshold=float(p["h_threshold"]), vertex_normals=p["vertex_normals"], tbn=p["tbn"], light_model="SH")
    with torch.no_grad():
        gen = torch.Generator().manual_seed(int(g["table_seed"]))
        field.encoder.embeddings.copy_(torch.rand(field.encoder.embeddings.shape, generator=gen) - 0.5)
        gen = torch.Generator().manual_seed(int(g["normal_table_seed"]))
        field.normal_net.encoder.embeddings.copy_(torch.rand(field.normal_net.encoder.embeddings.shape, generator=gen) - 0.5)
        for name, mlp in (("phi", field.normal_net.phi_net), ("theta", field.normal_net.theta_net)):
            for i, layer in enumerate(mlp.layers):
                layer.W.copy_(torch.from_numpy(g[f"{name}_W{i}"])), layer.b.copy_(torch.from_numpy(g[f"{name}_b{i}"])), layer.c.fill_(float(g[f"{name}_c{i}"]))
        field.sigma_net.weights.copy_(torch.from_numpy(g["w_sigma"]))
        field.light_net.brdf_layer.weights.copy_(torch.from_numpy(g["w_brdf"]))
        field.light_net.envSHs.copy_(torch.from_numpy(g["env_shs"]))
    field.fc_weight = float(g["fc_weight"])
    field = field.to(dev)
    x, d = torch.from_numpy(c["xyz"]).to(dev), torch.from_numpy(c["dirs"]).to(dev)
    # rays that grazed an edge may have picked the neighbouring triangle: compare where the projector agrees with the reference's (as
    # tests/test_gpu_round3.py does for the static field)
    face = field.projector.project_fused(x)[5].cpu().numpy()
    same = face == np.where(p["depth_pos"] < p["depth_neg"], p["face_pos"], p["face_neg"])
    near_edge = np.abs(np.abs(p["sdf"][:, 0]) - float(p["h_threshold"])) < 1e-4
    ok = same & ~near_edge
    assert ok.mean() > 0.99
    return g, field, x, d, ok


@pytest.mark.parametrize("fused", (True, False), ids=("fused", "op_by_op"))
def test_field_matches_the_reference_network_executed(dev, fused):
    """network_curvedfield.NeRFNetwork.forward with render_light_model=True over MeshFeatureField(pred_normal=True), executed by
    tools/make_golden.py (ref_python_curvedfield_sh.npz), against CurvedField(light_model="SH"): eval with fc_weight = 0.7 -- the normals, the
    mask, sigma and the four visual modes -- and training -- sigma, colour, and the ret_dict's fine normal and supervising normal.
    The fixture's lighting has bands 1 and 2 of the DC term's size, and it holds the shading normal and the view direction the reference's
    network hands to its head: `check_handed` compares them.
    Tolerances: sigma and colours as the static field's against its fixture (tests/test_gpu_round3.py: fp16 table and MLPs; rtol 3e-2 /
    atol 3e-3 and atol 2e-2); the fine normal, a unit vector out of fp32 LipMLPs on half features, 5e-3 per component; the supervising normal
    as the density gradient's direction is held in tests/test_gpu_round4.py (cosine: 1st percentile > 0.999, minimum > 0.98)."""
    g, field, x, d, ok = _field_from_fixture(dev)
    field.light_net.fused = fused
    handed = {}  # what the field hands to the light head, as the fixture holds what the reference's network handed to its head (:331-341)
    field.light_net.register_forward_pre_hook(lambda m, a, k: handed.update(normal=a[1], view_dirs=a[2]), with_kwargs=True)

    def check_handed(mode):
        """WHICH normal shades the sample: the fine normal detached in training; fc_weight x fine + (1 - fc_weight) x coarse, renormalised, in
        eval (:293-301).  In the fixture the blend lies a median 2 degrees (3.5e-2) from the fine normal and 4.7 from the coarse one, so the fine
        normal's bar of 5e-3 per component tells them apart; its length is 1 - 1e-5 up to fp32 rounding in both (5e-4: a blend that is not
        renormalised is 1.4e-3 short at the median).  The view direction is the ray's, not its negative (:333)."""
        got, want = handed["normal"].detach().float().cpu().numpy()[ok], g[mode + "_shading_normal"][ok]
        err = np.abs(got - want)
        print(f"{mode} shading normal: max |diff| {float(err.max()):.2e}; the fixture's own fine normal is {float(np.abs(g[mode + '_shading_normal'] - g['eval_normal_fine'])[ok].max()):.2e} away")
        assert err.max() <= 5e-3
        np.testing.assert_allclose(np.linalg.norm(got, axis=-1), np.linalg.norm(want, axis=-1), rtol=0, atol=5e-4)
        assert not handed["normal"].requires_grad
        assert np.array_equal(handed["view_dirs"].detach().float().cpu().numpy(), g[mode + "_view_dirs"])

    field.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        _, nc, hm, nf = field.embed(x, with_fine_normal=True)
        out = {}
        for mode in ("Full", "Specular", "Diffuse", "Albedo"):
            field.light_visual_mode = mode
            sigma, out[mode], extra = field(x, d)
            assert extra == {}
        field.light_visual_mode = "Full"
    check_handed("eval")
    assert np.array_equal(hm.cpu().numpy()[ok], g["eval_h_mask"][ok]) and 0.2 < float(hm.float().mean()) < 0.9
    np.testing.assert_allclose(nc.float().cpu().numpy(), g["eval_normal_coarse"], rtol=0, atol=3e-5)
    nf_err = np.abs(nf.float().cpu().numpy() - g["eval_normal_fine"])[ok]
    print("fine normal max |diff|", float(nf_err.max()))
    assert nf_err.max() <= 5e-3
    np.testing.assert_allclose(sigma.float().cpu().numpy()[ok], g["eval_sigma"][ok], rtol=3e-2, atol=3e-3)
    for mode, color in out.items():
        err = np.abs(color.float().cpu().numpy() - g["eval_color_" + mode.lower()])[ok]
        print(f"eval {mode}: max |diff| {float(err.max()):.2e}")
        assert err.max() <= 2e-2, mode
        assert not color[~hm].any()
    assert float(out["Full"].float().std()) > 1e-2 and not torch.equal(out["Full"], out["Diffuse"])
    field.train()
    with torch.autocast("cuda", dtype=torch.float16):
        sigma, color, extra = field(x, d, normal_supervision=True)
    check_handed("train")
    assert np.abs(g["train_shading_normal"] - g["eval_shading_normal"])[ok].max() > 5e-2 and np.abs(g["train_color"] - g["eval_color_full"])[ok].max() > 3e-2, \
        "the fixture tells the training normal from the eval blend, in the normal and in the colour"
    shaded = (sigma.detach() != 0) | (color.detach() != 0).any(-1)
    assert np.array_equal(shaded.cpu().numpy()[ok], g["train_h_mask"][ok])
    np.testing.assert_allclose(sigma.detach().float().cpu().numpy()[ok], g["train_sigma"][ok], rtol=3e-2, atol=3e-3)
    err = np.abs(color.detach().float().cpu().numpy() - g["train_color"])[ok]
    print(f"train colour: max |diff| {float(err.max()):.2e}")
    assert err.max() <= 2e-2
    assert np.abs(extra["normal"].detach().float().cpu().numpy() - g["train_normal"])[ok].max() <= 5e-3
    got, want = extra["normal_grad"].float().cpu().numpy()[ok], g["train_normal_grad"][ok]
    assert np.isfinite(got).all() and np.isfinite(want).all()
    cos = (got * want).sum(-1) / (np.linalg.norm(got, axis=-1) * np.linalg.norm(want, axis=-1) + 1e-12)
    print("supervising normal: cosine min %.5f, 1st percentile %.5f" % (cos.min(), np.percentile(cos, 1)))
    assert np.percentile(cos, 1) > 0.999 and cos.min() > 0.98
    np.testing.assert_allclose(np.linalg.norm(got, axis=-1), 1.0, atol=1e-3)
