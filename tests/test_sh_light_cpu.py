"""CPU: the SH light head -- the op-by-op restatement (ngp_harness.light.sh_light_shade) and the float64 helper (tests/sh_light_float64.py)
against what the reference's own SH_EnvmapMaterialNet.forward and its autograd produced (tests/golden/ref_python_sh_light.npz, written by
tools/make_golden.py --sh-light-only), the svox2 basis, the module's state_dict, the refusals and the C ABI's declarations."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sh_light_float64 as f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("w1s1", True, True), ("w1s0", True, False), ("w0s1", False, True), ("w0s0", False, False), ("dark", False, True))
KINK_CAP = 0.02


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_sh_light.npz"))


def _inside(name, got, want, bound, kink, cap=KINK_CAP):
    """|got - want| <= bound outside the kink bands; the excluded share stays under the cap.  Prints the largest error-to-bound ratio."""
    got, keep = np.asarray(got, np.float64), ~kink
    ratio = np.abs(got - want)[keep] / np.maximum(bound[keep], 1e-300)
    exact = np.abs(got - want)[keep] == 0
    worst = float(np.max(np.where(exact, 0.0, ratio))) if ratio.size else 0.0
    print(f"{name}: max error / bound {worst:.3f}, excluded {kink.mean():.4%}")
    assert kink.mean() <= cap, (name, kink.mean())
    assert worst <= 1.0, (name, worst)
    return worst


@pytest.mark.parametrize("case,white,spec", CASES)
def test_op_by_op_and_float64_match_the_reference(golden, case, white, spec):
    from ngp_harness.light import sh_light_shade

    g = {k[len(case) + 1:]: golden[k] for k in golden.files if k.startswith(case + "_")}
    brdf = torch.from_numpy(g["brdf"]).requires_grad_(True)
    env = torch.from_numpy(g["env_shs"]).requires_grad_(True)
    assert brdf.dtype == torch.float16 and env.shape == (16, 1 if white else 3)
    outs = sh_light_shade(brdf, torch.from_numpy(g["normals"]), torch.from_numpy(g["dirs"]), env, use_specular=spec, gamma=float(golden["gamma"]))
    (outs[0] * torch.from_numpy(g["grad_color"])).sum().backward()
    # the half sigmoids as the reference made them: its albedo output, and the same op on column 3
    a_h = g["albedo"].astype(np.float16)
    assert np.array_equal(a_h.astype(np.float32), g["albedo"])
    sw_h = torch.sigmoid(torch.from_numpy(g["brdf"][:, 3:4])).numpy()
    ref = f64.shade(a_h, sw_h, g["normals"], g["dirs"], g["env_shs"], float(golden["gamma"]), spec, grad_color=g["grad_color"])
    cap = KINK_CAP  # (the dark set too: it takes every branch -- clamped irradiance, clamped sum, safe_pow's floor -- but few samples sit ON a kink)
    for i, key in enumerate(("color", "specular", "diffuse", "albedo")):
        _inside(f"{case} fixture {key}", g[key], ref[key], ref["bound_" + key], ref["kink_" + key], cap)
        _inside(f"{case} op-by-op {key}", outs[i].detach().float().numpy(), ref[key], ref["bound_" + key], ref["kink_" + key], cap)
    for name, gb, ge in (("fixture", g["g_brdf"], g["g_env_shs"]), ("op-by-op", brdf.grad.numpy(), env.grad.numpy())):
        assert gb.dtype == np.float16 and not gb[:, 4].any(), "the glossiness receives exactly zero"
        assert not ge[9:].any()
        rows = np.broadcast_to(ref["kink_g"][:, None], (gb.shape[0], 3))
        _inside(f"{case} {name} grad_brdf[:, :3]", gb[:, :3], ref["g_albedo_h"], ref["bound_g_albedo_h"], rows, cap)
        _inside(f"{case} {name} grad_brdf[:, 3]", gb[:, 3:4], ref["g_spec_w_h"], ref["bound_g_spec_w_h"], ref["kink_g"][:, None], cap)
        _inside(f"{case} {name} grad_env", ge, ref["grad_env"], ref["bound_grad_env"], np.zeros(ge.shape, bool))
    if not spec:
        assert not brdf.grad[:, 3].any() and not g["g_brdf"][:, 3].any()


def test_main_lighting_stays_clear_of_the_kinks_and_dark_lighting_does_not(golden):
    """The reference's DC term of 3 with small higher bands keeps the op-by-op fp32 path's excluded share under the cap on its own; the
    dark set is the one that exercises the clamps and safe_pow's threshold."""
    shares = {}
    for case, white, spec in CASES:
        g = {k[len(case) + 1:]: golden[k] for k in golden.files if k.startswith(case + "_")}
        sw_h = torch.sigmoid(torch.from_numpy(g["brdf"][:, 3:4])).numpy()
        ref = f64.shade(g["albedo"].astype(np.float16), sw_h, g["normals"], g["dirs"], g["env_shs"], 2.4, spec)
        shares[case] = max(ref["kink_" + k].mean() for k in ("color", "specular", "diffuse"))
        dark_rows = (ref["color"] <= (1e-6) ** (1 / 2.4) * (1 + 1e-6)).any(-1).mean()
        if case == "dark":
            assert dark_rows > 0.05, "the dark set reaches safe_pow's floor"
        else:
            assert shares[case] <= KINK_CAP and dark_rows == 0
    print(shares)


def test_svox2_basis_order_and_signs():
    from ngp_harness.light import svox2_basis9

    s = 1 / np.sqrt(2)
    v = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [s, s, 0], [0, s, s], [s, 0, s]], np.float32)
    Y = svox2_basis9(torch.from_numpy(v)).numpy()
    c1, c2 = 0.4886025119029199, 1.0925484305920792
    assert np.allclose(Y[:, 0], 0.28209479177387814)
    assert np.allclose(Y[0, 1:4], [0, 0, -c1]) and np.allclose(Y[1, 1:4], [-c1, 0, 0]) and np.allclose(Y[2, 1:4], [0, c1, 0])  # order (y, z, x), signs (-, +, -)
    assert np.isclose(Y[3, 4], c2 / 2) and np.isclose(Y[4, 5], -c2 / 2) and np.isclose(Y[5, 7], -c2 / 2)
    assert np.isclose(Y[2, 6], 2 * 0.31539156525252005) and np.isclose(Y[0, 6], -0.31539156525252005)
    assert np.isclose(Y[0, 8], 0.5462742152960396) and np.isclose(Y[1, 8], -0.5462742152960396)
    rng = np.random.default_rng(3)
    r = rng.normal(size=(64, 3)).astype(np.float32)
    assert np.allclose(svox2_basis9(torch.from_numpy(r)).numpy(), f64.basis9(r.astype(np.float64))[0], rtol=1e-5, atol=1e-6)
    # the helper's derivative of the basis against central differences
    Yp, _, J = f64.basis9(r.astype(np.float64))
    for c in range(3):
        e = np.zeros(3)
        e[c] = 1e-6
        num = (f64.basis9(r + e)[0] - f64.basis9(r - e)[0]) / 2e-6
        assert np.allclose(num, J[:, :, c], atol=1e-7)


def test_reference_shaped_state_dict_loads_strictly(golden):
    from ngp_harness.light import SHLightNet

    shapes = dict(zip(golden["state_dict_keys"].tolist(), golden["state_dict_shapes"].tolist()))
    net = SHLightNet(input_dim=15, sh_order=3, white_light=False, use_specular=True)
    sd = {}
    for key, spec in shapes.items():
        shape, dtype = spec.split(":")
        ours = key.replace("brdf_layer.net.", "brdf_layer.")  # (the fixture's tcnn stand-in wraps the MLP in `.net`)
        sd[ours] = torch.ones([int(v) for v in shape.split(",")], dtype=getattr(torch, dtype.split(".")[1]))
    assert net.load_state_dict(sd, strict=True).missing_keys == []
    assert {n for n, _ in net.named_buffers()} == {"sh_pow_num", "sh_s"} and {n for n, _ in net.named_parameters()} == {"envSHs", "brdf_layer.weights"}
    fresh = SHLightNet(white_light=True)
    assert fresh.envSHs.shape == (16, 1) and float(fresh.envSHs[0, 0]) == 3 and not fresh.envSHs[1:].any() and fresh.gamma == float(golden["gamma"])
    assert fresh.brdf_layer.input_dim == 16 and fresh.brdf_layer.output_dim == 5 and fresh.brdf_layer.hidden_dim == 64 and fresh.brdf_layer.num_layers == 3


def test_refusals():
    from ngp_harness.curved import CurvedField
    from ngp_harness.light import SHLightNet

    with pytest.raises(ValueError, match="sh_order"):
        SHLightNet(sh_order=1)
    v = torch.zeros(3, 3)
    f = torch.zeros(1, 3, dtype=torch.int64)
    for model in ("SG", "Envmap"):
        with pytest.raises(NotImplementedError, match="SH"):
            CurvedField(v, f, light_model=model)
    with pytest.raises(ValueError, match="light_model"):
        CurvedField(v, f, light_model="phong")


def test_normal_cosine_loss_is_the_references_masked_mean():
    """nerf/utils.py:650-657 with its boolean-mask indexing, against the torch.where + device-count form the trainer records into a graph."""
    from ngp_harness.accelerate import normal_cosine_loss

    g = torch.Generator().manual_seed(0)
    ng, ne = torch.randn(300, 3, generator=g), torch.randn(300, 3, generator=g).requires_grad_(True)
    ng[::7, 1] = float("nan")
    ng[5] = ne.detach()[5] * 3  # (a ray past the threshold: cos = 1 is cut at cos(pi / 8) and passes no gradient)
    thr = float(np.cos(np.pi / 8))
    keep = torch.logical_not(ng.isnan().any(dim=-1))
    a = ng[keep] / (ng[keep].norm(dim=-1, keepdim=True) + 1e-5)
    b = ne[keep] / (ne[keep].norm(dim=-1, keepdim=True) + 1e-5)
    want = -torch.minimum((a * b).sum(dim=-1), thr * torch.ones_like(a[..., 0])).mean()
    (gw,) = torch.autograd.grad(want, ne)
    got = normal_cosine_loss(ng, ne)
    (gg,) = torch.autograd.grad(got, ne)
    assert torch.allclose(got, want, atol=1e-6) and torch.allclose(gg, gw, atol=1e-7) and not gg[::7].any() and not gg[5].any()
    assert torch.isnan(normal_cosine_loss(torch.full((4, 3), float("nan")), torch.ones(4, 3)))


def test_header_declares_and_library_exports_the_entry_points():
    import nerftex_hip

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerftex_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(nerftex_hip.LIB_PATH)
    for name in ("nerftex_sh_light_forward", "nerftex_sh_light_backward", "nerftex_sh_light_scratch_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header) and hasattr(lib, name) and name in nerftex_hip.EXPORTS, name
    fields = re.search(r"typedef struct nerftex_sh_light_desc \{(.*?)\} nerftex_sh_light_desc;", header, flags=re.S).group(1)
    declared = []
    for decl in fields.split(";"):
        decl = decl.strip()
        if decl:
            declared += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl).split(",")]
    assert declared == [n for n, _ in nerftex_hip.SHLightDesc._fields_], declared
    assert nerftex_hip.SH_LIGHT_SPECULAR == 1
    # the scratch is a function of B alone (the summation order must not depend on the machine): partials of 27 floats, at most 1024 of them
    sb = nerftex_hip.lib.nerftex_sh_light_scratch_bytes
    assert sb(0) == 108 and sb(1) == 108 and sb(257) == 216 and sb(262144) == 1024 * 108 and sb(1 << 22) == 1024 * 108
