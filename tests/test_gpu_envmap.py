"""GPU: relighting under an imported environment map.
  * nerftex_envmap_fit (csrc/envmap.inc) through the C ABI: the fixture's two cases against the reference's own EnvMap2SH result, seeded maps
    of 1 x 2, 8 x 8 and 50 x 100 pixels against the float64 model (tests/envmap_float64.py), the step counts, the same bits on every run.
    The tolerance is the reference's own fp32-against-float64 gap (envmap_float64.fit_tolerance), never the kernel's output.
  * nerftex_sh_light_probe_forward (csrc/shlight.inc) through the C ABI: every row inside sh_light_float64's bounds for one of the probes the
    float64 model cannot tell apart (within 1e-6 of the best dot product), masked rows exactly 0.
  * SHLightNet with the fixture's weights, fused and op by op, against the reference's outputs.
  * CurvedField(light_model="SH"): a uniform imported lighting renders exactly as a field trained to that lighting would -- forward(), the
    fused chain, the graphed loop, which re-records when the lighting in effect changes; per-probe lighting goes through forward().
Every comparison prints its figures (DESIGN.md 4.22 records them)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import envmap_float64 as e64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ref_python_envmap.npz"))


# ---- the fit --------------------------------------------------------------------------------------------------------------------------------------------

def _fit(dev, envmap, n_sh=16, scratch_fill=None):
    """nerftex_envmap_fit with the reference's settings -> (env_shs [n_sh,3] device tensor, updates made, last loss)."""
    from nerftex_hip import EnvmapFitDesc, check, lib, ptr, stream

    m = torch.from_numpy(np.ascontiguousarray(envmap, np.float32)).to(dev)
    H, W = m.shape[:2]
    phi, theta = torch.linspace(0.0, np.pi, H).to(dev), torch.linspace(-0.5 * np.pi, 1.5 * np.pi, W).to(dev)
    out = torch.full((n_sh, 3), float("nan"), dtype=torch.float32, device=dev)
    steps, loss = torch.full((1,), -1, dtype=torch.int32, device=dev), torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    scratch = torch.empty(lib.nerftex_envmap_fit_scratch_bytes(H, W) // 8, dtype=torch.float64, device=dev)
    if scratch_fill is not None:
        scratch.view(torch.uint8).fill_(scratch_fill)
    desc = EnvmapFitDesc(envmap=ptr(m), phi=ptr(phi), theta=ptr(theta), H=H, W=W, n_sh=n_sh, max_steps=5000, min_steps=2000, lr=1e-2, min_loss=1e-5,
                         env_shs=ptr(out), steps_run=ptr(steps), final_loss=ptr(loss), scratch=ptr(scratch), scratch_bytes=scratch.numel() * 8)
    check(lib.nerftex_envmap_fit(ctypes.byref(desc), stream()))
    torch.cuda.synchronize()
    return out, int(steps.item()), float(loss.item())


@pytest.mark.parametrize("case", ("a", "b"))
def test_fit_of_the_fixtures_maps(dev, golden, case):
    ref32, ref64 = golden[f"fit_{case}_fp32"], golden[f"fit_{case}_fp64"]
    tol = e64.fit_tolerance(ref32, ref64)
    got, steps, loss = _fit(dev, golden[f"fit_{case}_envmap"])
    got = got.cpu().numpy()
    err32, err64 = float(np.abs(got - ref32).max()), float(np.abs(got - ref64).max())
    print(f"fit case {case}: max|kernel - ref fp32| {err32:.3e}, max|kernel - ref float64| {err64:.3e}, reference gap {np.abs(ref32 - ref64).max():.3e}, "
          f"tolerance {tol:.3e}; steps {steps}, loss {loss:.6e} (reference {float(golden[f'fit_{case}_loss_fp32']):.6e})")
    assert steps == int(golden[f"fit_{case}_steps_fp32"])
    assert not got[9:].any(), "rows 9.. are written as 0"
    assert err32 <= tol
    assert abs(loss - float(golden[f"fit_{case}_loss_fp64"])) <= 1e-6 * max(1.0, loss)


def _seeded_map(H, W):
    """Case B's recipe, noise plus a bright patch -- not noise alone.  Under noise alone the best lighting is nearly constant and the eight
    higher bands hover about 0, where Adam's normalised update turns the sign of a rounding error into a step of the order of lr: the
    reference's own loop, run on the CPU in fp32 and in float64 on a 50 x 100 map of uniform noise, ends 2.7e-4 apart, and its float64 run
    and the float64 model fed bases perturbed by 1e-7 end 1e-3 apart.  Nothing can be held to 1e-6 of a coefficient on such a map.  With the
    patch the same two runs end 1.7e-7 (50 x 100) and 1.4e-7 (8 x 8) of the largest coefficient apart.  The two pixels of 1 x 2 (both at the
    pole: one direction) have no room for a patch: noise alone, 2.4e-7 between the reference loop's two precisions."""
    rng = np.random.default_rng(1000 * H + W)
    if H * W < 9:
        return rng.uniform(0.0, 1.5, (H, W, 3)).astype(np.float32)
    envmap = rng.uniform(0.0, 0.6, (H, W, 3)).astype(np.float32)
    envmap[H // 6:H // 6 + max(1, H // 4), W // 5:W // 5 + max(1, W // 6)] += 4.0
    return envmap


@pytest.mark.parametrize("H,W", ((1, 2), (8, 8), (50, 100)), ids=("1x2", "8x8_one_wave", "50x100_partials"))
def test_fit_of_seeded_maps_against_the_float64_model(dev, golden, H, W):
    envmap = _seeded_map(H, W)
    want, want_steps, losses = e64.adam_fit(*e64.moments(envmap), H * W)
    tol = e64.relative_fit_tolerance(golden) * float(np.abs(want).max())
    got, steps, loss = _fit(dev, envmap)
    err = float(np.abs(got.cpu().numpy() - want).max())
    print(f"fit {H} x {W}: max|kernel - float64 model| {err:.3e}, tolerance {tol:.3e} ({e64.relative_fit_tolerance(golden):.2e} of the largest coefficient "
          f"{np.abs(want).max():.3f}); steps {steps} (model {want_steps}), loss {loss:.6e} (model {losses[-1]:.6e})")
    assert steps == want_steps and err <= tol
    assert abs(loss - losses[-1]) <= 1e-6 * max(1.0, losses[-1])


def test_fit_returns_the_same_bits_alone_and_beside_a_busy_stream(dev, golden):
    envmap = _seeded_map(50, 100)
    a, steps_a, loss_a = _fit(dev, envmap, scratch_fill=0)
    b, steps_b, loss_b = _fit(dev, envmap, scratch_fill=255)  # (what the scratch held does not matter: it is written before it is read)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and steps_a == steps_b and loss_a == loss_b
    side = torch.cuda.Stream()
    busy = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            busy = torch.tanh(busy @ busy * 1e-3)
    c, steps_c, loss_c = _fit(dev, envmap)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and steps_a == steps_c and loss_a == loss_c
    sixteen, _, _ = _fit(dev, envmap)
    nine, _, _ = _fit(dev, envmap, n_sh=9)
    assert torch.equal(nine, sixteen[:9])


def test_the_module_level_fit_takes_the_entry_on_the_gpu(dev, golden, monkeypatch):
    import nerftex_hip
    from ngp_harness.light import envmap_to_sh

    calls = []
    entry = nerftex_hip.lib.nerftex_envmap_fit
    monkeypatch.setattr(nerftex_hip.lib, "nerftex_envmap_fit", lambda *a: (calls.append(1), entry(*a))[1])
    m = torch.from_numpy(golden["fit_a_envmap"]).to(dev)
    got, info = envmap_to_sh(m)
    assert calls == [1] and got.is_cuda and got.shape == (16, 3) and info["steps"] == 2002
    want, _, _ = _fit(dev, golden["fit_a_envmap"])
    assert torch.equal(got, want)


# ---- the probe head through the C ABI -------------------------------------------------------------------------------------------------------------------

def _probe_inputs(dev, golden, B, K, seed):
    rng = np.random.default_rng(seed)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)  # noqa: E731
    p = dict(brdf=rng.normal(0, 2.0, (B, 16)).astype(np.float16), n=unit(rng.normal(size=(B, 3))).astype(np.float32),
             d=(unit(rng.normal(size=(B, 3))) * rng.uniform(0.5, 2.0, (B, 1))).astype(np.float32), mask=rng.uniform(size=B) < 0.7)
    n2 = rng.normal(size=(B, 3))
    p["n2"] = (n2 / (np.linalg.norm(n2, axis=-1, keepdims=True) + 1e-5)).astype(np.float32)
    p["probes"] = golden["probes"] if K == 64 else unit(rng.normal(size=(K, 3))).astype(np.float32)  # (64: the reference's grid, with its coinciding directions)
    tables = rng.normal(0, 0.1, (K, 9, 3)).astype(np.float32)
    tables[:, 0] = rng.uniform(1.0, 3.0, (K, 3))
    p["tables"] = tables
    return p, {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in p.items()}


def _probe_forward(t, spec, masked, gamma=2.4):
    from nerftex_hip import SH_LIGHT_SPECULAR, SHLightProbeDesc, check, lib, ptr, stream

    B = t["brdf"].shape[0]
    outs = torch.full((4, B, 3), float("nan"), dtype=torch.float32, device=t["brdf"].device)
    mask_b = t["mask"].view(torch.uint8) if masked else None
    desc = SHLightProbeDesc(brdf=ptr(t["brdf"]), brdf_stride=t["brdf"].stride(0), normals=ptr(t["n"]), dirs=ptr(t["d"]), normals_secondary=ptr(t["n2"]),
                            probes=ptr(t["probes"]), probe_shs=ptr(t["tables"]), K=t["probes"].shape[0], mask=ptr(mask_b), B=B, gamma=gamma,
                            flags=SH_LIGHT_SPECULAR if spec else 0, color=ptr(outs[0]), specular=ptr(outs[1]), diffuse=ptr(outs[2]), albedo=ptr(outs[3]))
    check(lib.nerftex_sh_light_probe_forward(ctypes.byref(desc), stream()))
    return outs


@pytest.mark.parametrize("B", (1, 63, 64, 65, 257))
def test_probe_forward_through_the_c_abi(dev, golden, B):
    from ngp_harness.light import sh_light_shade_probes

    for K in (64, 1, 3):
        for spec in (True, False):
            for masked in (False, True):
                p, t = _probe_inputs(dev, golden, B, K, seed=1000 * K + B)
                outs = _probe_forward(t, spec, masked).cpu().numpy()
                assert np.isfinite(outs).all(), "every row is written"
                a_h, sw_h = torch.sigmoid(t["brdf"][:, :3]).cpu().numpy(), torch.sigmoid(t["brdf"][:, 3:4]).cpu().numpy()
                live = p["mask"] if masked else np.ones(B, bool)
                assert np.array_equal(outs[3][live], a_h.astype(np.float32)[live]), "the half sigmoid, bit for bit"
                tag = f"B={B} K={K} spec={int(spec)} mask={int(masked)}"
                cap = 0.02  # (tests/test_gpu_sh_light.py's KINK_CAP)
                single = e64.check_probe_shading("probe kernel | " + tag, outs, a_h, sw_h, p["n"], p["d"], p["n2"], p["probes"], p["tables"], 2.4, spec,
                                                 p["mask"] if masked else None, kink_cap=cap)
                with torch.no_grad():
                    ops = sh_light_shade_probes(t["brdf"], t["n"], t["d"], t["n2"], t["probes"], t["tables"], spec, 2.4, t["mask"] if masked else None)
                e64.check_probe_shading("probe op-by-op | " + tag, torch.stack([o.float() for o in ops]).cpu().numpy(), a_h, sw_h, p["n"], p["d"], p["n2"],
                                        p["probes"], p["tables"], 2.4, spec, p["mask"] if masked else None, kink_cap=cap)
                if K == 3 and B >= 63:
                    assert single >= 0.9, "generic probes: the choice is decided for nearly every row, the check is not vacuous"


def test_probe_choice_takes_the_lowest_index_among_equal_maxima(dev, golden):
    """Identical probe directions with different tables: every row is lit by the first."""
    p, t = _probe_inputs(dev, golden, 130, 3, seed=5)
    t["probes"] = t["probes"][:1].repeat(3, 1).contiguous()
    outs = _probe_forward(t, True, False)
    t1 = dict(t, probes=t["probes"][:1].contiguous(), tables=t["tables"][:1].contiguous())
    assert torch.equal(outs, _probe_forward(t1, True, False))
    t2 = dict(t, tables=t["tables"].flip(0).contiguous())
    assert not torch.equal(outs[0], _probe_forward(t2, True, False)[0])


# ---- the module with the reference's weights ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused", (True, False), ids=("fused", "op_by_op"))
def test_module_with_the_references_weights_under_probe_lighting(dev, golden, fused):
    """SHLightNet in eval with the fixture's BRDF weights and probe tables under fp16 autocast, against the reference's outputs (each row shaded
    as the first of its batch: tools/make_envmap_golden.py), at the tolerance tests/test_gpu_sh_light.py::test_module_with_the_references_weights
    holds the head to: 2^-9 of the largest BRDF output.  Rows whose probe the float64 model calls undecided may have been lit by another of
    their candidates than the reference took: they are held to the model's shading of any candidate, at the same tolerance."""
    from ngp_harness.light import SHLightNet

    t = lambda k: torch.from_numpy(golden[k]).to(dev)  # noqa: E731
    net = SHLightNet(white_light=True, use_specular=True).to(dev).eval()
    with torch.no_grad():
        net.brdf_layer.weights.copy_(t("probe_w_brdf"))
    net.load_envmap(env_shs=golden["uniform_env_shs"], env_shs_vis=golden["probe_shs"], probes=golden["probes"])
    net.fused = fused
    seen = {}
    handle = net.brdf_layer.register_forward_hook(lambda m, i, o: seen.__setitem__("brdf", o))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        outs = net(t("probe_geo_feat"), t("probe_normals"), t("probe_dirs"), normal_secondary=t("probe_normals_secondary"), shade_visibility=True)
        flat = net(t("probe_geo_feat"), t("probe_normals"), t("probe_dirs"), shade_visibility=False)
    handle.remove()
    brdf, want = seen["brdf"].detach().float().cpu().numpy()[:, :5], golden["probe_brdf"].astype(np.float32)
    assert (np.abs(brdf - want) / np.maximum(np.abs(want), 1.0)).max() <= 2.0 ** -9
    tol = 2.0 ** -9 * float(np.abs(want).max())
    outs = np.stack([o.float().cpu().numpy() for o in outs])
    ref = np.stack([golden["probe_rows_" + k] for k in e64.KEYS])
    row_err = np.abs(outs - ref).max(axis=(0, 2))
    cands = e64.probe_candidates(golden["probe_normals_secondary"], golden["probes"])
    undecided = cands.sum(-1) > 1
    print(f"fused={fused}: max|module - reference| decided rows {row_err[~undecided].max():.3e}, undecided rows {row_err[undecided].max():.3e} "
          f"({int(undecided.sum())} of {len(undecided)}), tolerance {tol:.3e}")
    assert row_err[~undecided].max() <= tol
    rows = np.nonzero(undecided & (row_err > tol))[0]
    if len(rows):
        a_h, sw_h = torch.sigmoid(torch.from_numpy(golden["probe_brdf"][rows, :3])).numpy(), torch.sigmoid(torch.from_numpy(golden["probe_brdf"][rows, 3:4])).numpy()
        e64.check_probe_shading(f"undecided rows fused={fused}", outs[:, rows], a_h, sw_h, golden["probe_normals"][rows], golden["probe_dirs"][rows],
                                golden["probe_normals_secondary"][rows], golden["probes"], golden["probe_shs"], float(golden["gamma"]), extra=tol, kink_cap=1.0)
    flat_err = max(float(np.abs(flat[i].float().cpu().numpy() - golden["uniform_" + k]).max()) for i, k in enumerate(e64.KEYS))
    print(f"fused={fused}: uniform imported lighting max|module - reference| {flat_err:.3e}")
    assert flat_err <= tol


# ---- the field ------------------------------------------------------------------------------------------------------------------------------------------

def _sh_field(dev):
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05, light_model="SH").to(dev)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
        field.normal_net.encoder.embeddings.uniform_(-0.5, 0.5)
    return field, v


@pytest.fixture(scope="module")
def fields(dev, golden):
    """The relit field and its twin: the same seeds, the twin's envSHs REPLACED by the coefficients the first imports."""
    field, v = _sh_field(dev)
    twin, _ = _sh_field(dev)
    env = torch.from_numpy(golden["uniform_env_shs"]).to(dev)
    twin.light_net.envSHs = torch.nn.Parameter(env.clone())
    for a, b in zip(field.parameters(), twin.parameters()):
        assert a.shape != b.shape or torch.equal(a, b)
    rng = np.random.default_rng(5)
    n = 256
    ids = 36 + np.arange(n) % (v.shape[0] - 72)
    vn = field.projector.vertex_normals.cpu().numpy()
    x = (v[ids] + rng.uniform(-0.04, 0.04, size=(n, 1)).astype(np.float32) * vn[ids]).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return dict(field=field, twin=twin, env=env, x=torch.from_numpy(x).to(dev), d=torch.from_numpy(d).to(dev))


def _reset(field):
    net = field.light_net
    net.import_envmap, net.envSHs_import, net.envSHs_import_vis, net.probes = False, None, None, None
    field.shade_visibility, field.fused_light_infer = True, False
    field.eval()


def test_field_under_a_uniform_imported_lighting_is_the_field_trained_to_it(dev, golden, fields, monkeypatch):
    from ngp_harness.curved import CurvedField

    field, twin, x, d = (fields[k] for k in ("field", "twin", "x", "d"))
    _reset(field), _reset(twin)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            before = field(x, d)
            assert field.light_net.load_envmap(env_shs=golden["uniform_env_shs"])
            with pytest.raises(RuntimeError, match="shade_visibility"):
                field(x, d)  # (the reference's default asks for the probe tables)
            field.shade_visibility = False
            sigma, color, _ = field(x, d)
            want_sigma, want_color, _ = twin(x, d)
            assert torch.equal(sigma, want_sigma) and torch.equal(color, want_color) and not torch.equal(color, before[1]) and float(color.abs().sum()) > 0
            calls = []
            call = CurvedField._infer_call
            monkeypatch.setattr(CurvedField, "_infer_call", lambda self, name, *a, **k: (calls.append(name), call(self, name, *a, **k))[1])
            field.fused_light_infer = twin.fused_light_infer = True
            got, want = field.infer(x, d), twin.infer(x, d)
            assert calls == ["nerftex_curved_light_infer"] * 2, "both go through the fused chain"
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert float((got[1] - color.float()).abs().max()) <= 2e-2, "the chain follows forward()"
            field.light_net.switch_envmap_import()
            assert torch.equal(field.infer(x, d)[1], field.infer(x, d)[1]) and not torch.equal(field.infer(x, d)[1], got[1])
            assert torch.equal(field(x, d)[1], before[1]), "switched off: envSHs again"
    finally:
        _reset(field), _reset(twin)


def test_field_in_training_ignores_the_import(dev, golden, fields):
    field, x, d = fields["field"], fields["x"], fields["d"]
    _reset(field)
    try:
        field.train()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            want = field(x, d)
            field.light_net.load_envmap(env_shs=golden["uniform_env_shs"], env_shs_vis=golden["probe_shs"], probes=golden["probes"])
            got = field(x, d)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    finally:
        _reset(field)


def test_field_under_per_probe_lighting_goes_through_forward(dev, golden, fields, monkeypatch):
    from ngp_harness.curved import CurvedField

    field, x, d = fields["field"], fields["x"], fields["d"]
    _reset(field)
    try:
        field.light_net.load_envmap(env_shs=golden["uniform_env_shs"], env_shs_vis=golden["probe_shs"], probes=golden["probes"])
        field.fused_light_infer = True
        calls = []
        monkeypatch.setattr(CurvedField, "_infer_call", lambda self, name, *a, **k: calls.append(name))
        asked = []
        predicate = CurvedField._infer_light_back_fused
        monkeypatch.setattr(CurvedField, "_infer_light_back_fused", lambda self, xx: (asked.append(1), predicate(self, xx))[1])
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            sigma, color, _ = field(x, d)
            got = field.infer(x, d)
            assert asked and not calls, "the lit chains were asked and stepped aside"
            assert torch.equal(got[0], sigma.float()) and torch.equal(got[1], color.float())
            field.shade_visibility = False
            flat = field(x, d)[1]
            assert not torch.equal(flat, color), "per-probe lighting is another lighting than the uniform one"
            field.infer(x, d)
            assert calls == ["nerftex_curved_light_infer"], "the uniform imported lighting takes the chain"
    finally:
        _reset(field)


def test_the_graphed_loop_re_records_when_the_lighting_in_effect_changes(dev, golden, fields):
    from ngp_harness import scene
    from ngp_harness.model import Renderer

    field = fields["field"]
    _reset(field)
    try:
        r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
        with torch.autocast("cuda", dtype=torch.float16):
            r.update_extra_state_device()
        o, d = scene.get_rays(scene.rand_poses(1, 1.6, np.random.default_rng(11))[0], scene.intrinsics(32, 32), 32, 32)
        ro, rd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        kw = dict(dt_gamma=0.0, max_steps=256, slots_per_ray=4)
        field.shade_visibility = False
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            img0, _, _ = r.render_infer_graphed(ro, rd, parts=2, block=2, **kw)
            graphs = r._infer_graphs
            r.render_infer_graphed(ro, rd, parts=2, block=2, **kw)
            assert r._infer_graphs is graphs
            field.light_net.load_envmap(env_shs=golden["uniform_env_shs"])
            img1, dep1, _ = r.render_infer_graphed(ro, rd, parts=2, block=2, **kw)
            assert r._infer_graphs is not graphs and not torch.equal(img1, img0), "a loaded lighting re-records"
            want = r.render_infer(ro, rd, **kw)
            assert torch.equal(img1, want[0]) and torch.equal(dep1, want[1])
            graphs = r._infer_graphs
            field.light_net.switch_envmap_import()
            img2, _, _ = r.render_infer_graphed(ro, rd, parts=2, block=2, **kw)
            assert r._infer_graphs is not graphs and torch.equal(img2, img0), "the switch re-records: the trained lighting again"
    finally:
        _reset(field)
