"""GPU: the SH-lit curved field on the device-count inference path -- nerftex_curved_light_infer (the whole no-grad chain as one call whose
kernels read the live row count from the device) and CurvedField.infer with `fused_light_infer = True` behind the three inference loops.

  * the rows contract with outputs pre-filled by a sentinel; sigma and the height mask bit for bit forward()'s;
  * the shading normal (read through the entry's optional output) inside the bound of tests/normal_net_float64.py on every row of the mask, in
    eval with fc_weight 1.0 and 0.7 and in training mode;
  * the colour in the four visual modes inside the bound of tests/sh_light_float64.py evaluated at the kernel's own shading normal and at the
    BRDF rows brdf_layer gives for the same features;
  * a batch where the two gathers run as the level-per-XCD kernel; two calls, the same bits; the reference's executed network;
  * 32 x 32 frames through the three loops; the switch off; shapes the entry does not serve.
Every comparison prints its largest error-to-bound ratio (DESIGN.md 4.14 records them)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import normal_net_float64 as nn64
import sh_light_float64 as f64

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
KINK_CAP = 0.02
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _sh_field(dev, **kw):
    """The star-flower field of tests/test_gpu_sh_light.py with a normal net whose angles are of order 1 (the constructor's weights give a
    fine normal within a few degrees of the frame's: a wrong rotation or a wrong weight order would hide inside the bars)."""
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05, light_model="SH", **kw).to(dev)
    gen = torch.Generator(device=dev).manual_seed(2)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
        field.normal_net.encoder.embeddings.uniform_(-0.5, 0.5)
        field.light_net.envSHs[1:].normal_(0, 0.1, generator=gen)
        for mlp in (field.normal_net.phi_net, field.normal_net.theta_net):
            for layer in mlp.layers:
                layer.W.mul_(6.0)
                layer.b.normal_(0, 0.3, generator=gen)
                layer.c.fill_(2.0)
    return field.eval(), v


def _points(dev, field, v, n, seed=5):
    """n points around the mesh (vertices pushed along their normals by up to +-0.1), in ray-like order: four consecutive rows share a direction."""
    rng = np.random.default_rng(seed)
    ids = 36 + np.arange(n) % (v.shape[0] - 72)
    vn = field.projector.vertex_normals.cpu().numpy()
    x = (v[ids] + rng.uniform(-0.1, 0.1, size=(n, 1)).astype(np.float32) * vn[ids]).astype(np.float32)
    d = rng.normal(size=(n // 4, 3)).astype(np.float32)
    d = np.repeat(d / np.linalg.norm(d, axis=-1, keepdims=True), 4, axis=0)
    return torch.from_numpy(x).to(dev), torch.from_numpy(d).to(dev).contiguous()


def _marks(dev, n):
    marked = torch.zeros(n, dtype=torch.bool, device=dev)
    marked[::7] = True       # single slots
    marked[64:96] = True     # a whole 32-row step of an FFMLP wave
    if n >= 384:
        marked[256:384] = True   # a whole 128-row workgroup
    return marked


CONFIGS = [("eval", 1.0), ("eval", 0.7), ("train", 1.0)]


def _configure(field, mode, fc, visual="Full"):
    field.train(mode == "train")
    field.fc_weight, field.light_visual_mode = fc, visual


def _reference(field, x, d, mode, fc):
    """What forward() (the switch off) computes for the batch, and the float64 helper's shading normal with its bound from forward()'s own
    inputs to the normal net.  Computed once per configuration and shared."""
    _configure(field, mode, fc)
    assert not getattr(field, "fused_light_infer", False)
    handed = {}
    handle = field.light_net.register_forward_pre_hook(lambda m, a, k: handed.update(geo=a[0], n=a[1]), with_kwargs=True)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            p_sur, _, h_mask, raw, tbn, _, z = field.projector.project_fused(x, multires=field.multires)
            x_embed = field.encoder(p_sur, bound=field.bound)
            phi_embed = field.normal_net.encoder(p_sur)
            assert x_embed.dtype == torch.float16 and phi_embed.dtype == torch.float16 and z.dtype == torch.float32
            sigma, color, _ = field(x, d)
            ones = torch.ones(x.shape[0], 1, dtype=handed["geo"].dtype, device=x.device)
            brdf = field.light_net.brdf_layer(torch.cat([handed["geo"], ones], dim=-1))
    finally:
        handle.remove()
    weights, biases, _, _ = nn64.pack(field.normal_net)
    ref = nn64.fine_normal(phi_embed.cpu().numpy(), x_embed.cpu().numpy(), z.half().cpu().numpy(), weights, biases, tbn=tbn.cpu().numpy(),
                           coarse_raw=raw.cpu().numpy(), fc_weight=fc, blend=mode == "eval")
    assert sigma.dtype == torch.float32 and color.dtype == torch.float32
    return dict(sigma=sigma, color=color, mask=h_mask, brdf=brdf, normal_fwd=handed["n"].float(), normal=ref["normal"], bound_normal=ref["bound_normal"])


@pytest.fixture(scope="module")
def setup(dev):
    field, v = _sh_field(dev)
    n = 1024
    x, d = _points(dev, field, v, n)
    marked = _marks(dev, n)
    xm, dm = x.clone(), d.clone()
    xm[marked] = 1e30
    dm[marked, 0] = 1e30
    refs = {cfg: _reference(field, x, d, *cfg) for cfg in CONFIGS}
    inside = float(refs[CONFIGS[0]]["mask"].float().mean())
    assert 0.2 < inside < 0.8, inside  # both sides of the height mask are exercised
    return dict(field=field, v=v, x=x, d=d, xm=xm, dm=dm, marked=marked, refs=refs)


def _call(field, x, d, live=None, want_normal=True):
    """nerftex_curved_light_infer through the descriptor CurvedField builds, outputs pre-filled with the sentinel."""
    from nerftex_hip import check, lib, stream

    n, dev = x.shape[0], x.device
    sigma = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
    rgbs = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dev)
    normal = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dev) if want_normal else None
    scratch = torch.empty(lib.nerftex_curved_light_infer_scratch_bytes(n), dtype=torch.uint8, device=dev)
    field.fused_light_infer = True
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._infer_light_fused(x, d) and not field._infer_fused(x, d)
            desc, keep = field._infer_light_desc(x, d, live, sigma, rgbs, scratch, normal)
            check(lib.nerftex_curved_light_infer(ctypes.byref(desc), stream()))
        torch.cuda.synchronize()
    finally:
        field.fused_light_infer = False
    return sigma, rgbs, normal


def _inside(name, got, want, bound, kink=None, cap=KINK_CAP):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all() and np.isfinite(want).all() and np.isfinite(bound).all(), name
    kink = np.zeros(got.shape, bool) if kink is None else kink
    err = np.abs(got - want)[~kink]
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound[~kink], 1e-300))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{name}: max error / bound {worst:.3f}, max error {float(err.max()) if err.size else 0.0:.3e}, excluded {kink.mean():.4%}")
    assert kink.mean() <= cap, (name, float(kink.mean()))
    assert worst <= 1.0, (name, worst)


# B = 128 with no unit and with one (of 5 rows, and of the whole batch); B = 384 with two of its three workgroups live
@pytest.mark.parametrize("n,units,rows_per_unit,want_live", [(128, 0, 5, 0), (128, 1, 5, 5), (128, 1, 128, 128), (384, 2, 128, 256), (384, None, 0, 384)])
def test_rows_contract_at_the_c_abi(dev, setup, n, units, rows_per_unit, want_live):
    """Unmarked live rows: sigma and the height mask are forward()'s, bit for bit, and the colour is shaded; marked live rows (one of them,
    row 0, inside every live unit) are exactly 0; rows >= live keep the sentinel in all three outputs."""
    field, ref = setup["field"], setup["refs"][("eval", 1.0)]
    _configure(field, "eval", 1.0)
    x, d, marked = setup["xm"][:n].contiguous(), setup["dm"][:n].contiguous(), setup["marked"][:n]
    live = None if units is None else (torch.tensor([units], dtype=torch.int32, device=dev), rows_per_unit)
    sigma, rgbs, normal = _call(field, x, d, live)
    rows = torch.arange(n, device=dev)
    alive, past = rows < want_live, rows >= want_live
    plain, unused = alive & ~marked, alive & marked
    if want_live:
        assert bool(unused.any()) and bool(plain.any())
    mask = ref["mask"][:n]
    assert torch.equal(sigma[plain], ref["sigma"][:n][plain]), "sigma: the same kernels as the static chain up to the exp"
    assert torch.equal(((sigma != 0) | (rgbs != 0).any(-1))[plain & mask], torch.ones_like(mask)[plain & mask]) and not rgbs[plain & ~mask].any()
    assert not sigma[plain & ~mask].any()
    assert bool((sigma[unused] == 0).all()) and bool((rgbs[unused] == 0).all()) and bool((normal[unused] == 0).all())
    assert bool((sigma[past] == SENTINEL).all()) and bool((rgbs[past] == SENTINEL).all()) and bool((normal[past] == SENTINEL).all())
    if want_live >= 128:
        assert float(sigma[plain].max()) > 0 and float(rgbs[plain].max()) > 0
        unit = normal[plain & mask].norm(dim=-1)
        assert float((unit - 1).abs().max()) < 1e-3


@pytest.mark.parametrize("mode,fc", CONFIGS)
def test_sigma_mask_and_shading_normal(dev, setup, mode, fc):
    field, ref, marked = setup["field"], setup["refs"][(mode, fc)], setup["marked"]
    _configure(field, mode, fc)
    sigma, rgbs, normal = _call(field, setup["xm"], setup["dm"])
    plain = ~marked
    assert torch.equal(sigma[plain], ref["sigma"][plain]), "sigma and the height mask of the unmarked rows: forward()'s bits"
    assert torch.equal((sigma != 0)[plain], (ref["sigma"] != 0)[plain]) and not rgbs[plain & ~ref["mask"]].any()
    rows = (plain & ref["mask"]).cpu().numpy()
    assert rows.sum() > 200
    tag = f"{mode} fc={fc}"
    _inside(f"kernel shading normal | {tag}", normal.cpu().numpy()[rows], ref["normal"][rows], ref["bound_normal"][rows])
    # the framework's own evaluation under the same bound (a bound forward() misses would be a wrong bound)
    _inside(f"forward() shading normal | {tag}", ref["normal_fwd"].cpu().numpy()[rows], ref["normal"][rows], ref["bound_normal"][rows])
    print(f"median bound on a component of the shading normal | {tag}: {float(np.median(ref['bound_normal'][rows])):.3e}")
    # the normal is not the frame's: the net's angles are of order 1 here
    with torch.no_grad():
        tbn = field.projector.project_fused(setup["x"], multires=0)[4]
    assert float((normal - tbn[:, 2]).abs().max(-1).values[torch.from_numpy(rows).to(dev)].median()) > 0.05
    if mode == "eval" and fc != 1.0:
        other = setup["refs"][("eval", 1.0)]["normal"]
        assert float(np.abs(other - ref["normal"])[rows].max()) > 5e-2, "the blend moves the normal by more than its bound"


@pytest.mark.parametrize("visual", ("Full", "Specular", "Diffuse", "Albedo"))
def test_colour_in_the_four_visual_modes(dev, setup, visual):
    field, ref, marked = setup["field"], setup["refs"][("eval", 0.7)], setup["marked"]
    _configure(field, "eval", 0.7, visual)
    try:
        sigma, rgbs, normal = _call(field, setup["xm"], setup["dm"])
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            fwd = field(setup["x"], setup["d"])[1].float()
    finally:
        field.light_visual_mode = "Full"
    plain = (~marked).cpu().numpy()
    key = {"Full": "color"}.get(visual, visual.lower())
    a_h = torch.sigmoid(ref["brdf"][:, :3]).cpu().numpy()
    sw_h = torch.sigmoid(ref["brdf"][:, 3:4]).cpu().numpy()
    env, mask = field.light_net.envSHs.detach().cpu().numpy(), ref["mask"].cpu().numpy()
    d = setup["d"].cpu().numpy()
    at_kernel = f64.shade(a_h, sw_h, normal.cpu().numpy(), d, env, field.light_net.gamma, field.light_net.use_specular, mask)
    _inside(f"kernel {visual}", rgbs.cpu().numpy()[plain], at_kernel[key][plain], at_kernel["bound_" + key][plain], at_kernel["kink_" + key][plain])
    # forward() itself, at the normal it handed to its head, stays under the cap with this lighting and these inputs
    at_fwd = f64.shade(a_h, sw_h, ref["normal_fwd"].cpu().numpy(), d, env, field.light_net.gamma, field.light_net.use_specular, mask)
    _inside(f"forward() {visual}", fwd.cpu().numpy(), at_fwd[key], at_fwd["bound_" + key], at_fwd["kink_" + key])
    assert float(rgbs[torch.from_numpy(plain & mask).to(dev)].std()) > 1e-3
    print(f"{visual}: largest |fused - forward()| over the unmarked rows {float((rgbs - fwd).abs()[torch.from_numpy(plain).to(dev)].max()):.3e}")


def test_where_the_gathers_run_by_level(dev, setup):
    """8192 rows (csrc/grid_common.hpp kLevelFwdMinBatch): both tables' gathers are the level-per-XCD kernel.  Sigma (the texture table) bit for
    bit, the shading normal (both tables) inside its bound; 5000 live rows of them (a partial wave inside a partial workgroup)."""
    field, v = setup["field"], setup["v"]
    n = 8192
    x, d = _points(dev, field, v, n, seed=9)
    ref = _reference(field, x, d, "eval", 0.7)
    marked = _marks(dev, n)
    xm, dm = x.clone(), d.clone()
    xm[marked] = 1e30
    dm[marked, 0] = 1e30
    _configure(field, "eval", 0.7)
    sigma, rgbs, normal = _call(field, xm, dm, (torch.tensor([1000], dtype=torch.int32, device=dev), 5))
    rows = torch.arange(n, device=dev)
    plain, past = (rows < 5000) & ~marked, rows >= 5000
    assert torch.equal(sigma[plain], ref["sigma"][plain]) and float(sigma[plain].max()) > 0
    assert bool((sigma[past] == SENTINEL).all()) and bool((rgbs[past] == SENTINEL).all()) and bool((normal[past] == SENTINEL).all())
    assert not sigma[(rows < 5000) & marked].any() and not rgbs[(rows < 5000) & marked].any()
    keep = (plain & ref["mask"]).cpu().numpy()
    _inside("kernel shading normal | 8192 rows", normal.cpu().numpy()[keep], ref["normal"][keep], ref["bound_normal"][keep])


def test_two_calls_give_the_same_bits(dev, setup):
    field = setup["field"]
    _configure(field, "eval", 0.7)
    a = _call(field, setup["xm"], setup["dm"])
    b = _call(field, setup["xm"], setup["dm"])
    for p, q in zip(a, b):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))


def test_fused_infer_matches_the_reference_network_executed(dev):
    """tests/golden/ref_python_curvedfield_sh.npz (the reference's network, executed) loaded as tests/test_gpu_sh_light.py loads it; the batch
    padded to a multiple of 128 with marked slots; the fused infer() meets the bars forward() is held to there: 5e-3 per component on the
    shading normals, 2e-2 on the colours, mask equality on the decided rows -- eval (fc_weight 0.7, the four visual modes) and training."""
    from test_gpu_sh_light import _field_from_fixture

    g, field, x, d, ok = _field_from_fixture(dev)
    B = x.shape[0]
    pad = -B % 128 or 128
    xp = torch.full((B + pad, 3), 1e30, device=dev)
    dp = torch.full((B + pad, 3), 1e30, device=dev)
    xp[:B], dp[:B] = x, d
    for mode in ("eval", "train"):
        field.train(mode == "train")
        for visual in (("Full", "Specular", "Diffuse", "Albedo") if mode == "eval" else ("Full",)):
            field.light_visual_mode = visual
            sigma, rgbs, normal = _call(field, xp, dp)
            assert not sigma[B:].any() and not rgbs[B:].any() and not normal[B:].any()
            want = g["eval_color_" + visual.lower()] if mode == "eval" else g["train_color"]
            err = np.abs(rgbs[:B].cpu().numpy() - want)[ok]
            nerr = np.abs(normal[:B].cpu().numpy() - g[mode + "_shading_normal"])[ok]
            shaded = ((sigma != 0) | (rgbs != 0).any(-1))[:B].cpu().numpy()
            hm = g[mode + "_h_mask"]
            print(f"{mode} {visual}: colour max |diff| {float(err.max()):.2e}, shading normal max |diff| {float(nerr[hm[ok]].max()):.2e}")
            assert np.array_equal(shaded[ok], hm[ok])
            assert err.max() <= 2e-2
            assert nerr[hm[ok]].max() <= 5e-3
            np.testing.assert_allclose(sigma[:B].cpu().numpy()[ok], g[mode + "_sigma"][ok], rtol=3e-2, atol=3e-3)
    field.light_visual_mode = "Full"


KW = dict(dt_gamma=0.0, max_steps=256)


@pytest.fixture(scope="module")
def frame_setup(dev, setup):
    """The field behind a Renderer and two 32 x 32 poses.  The three loops cut a ray's samples into iterations differently, and with the switch
    OFF -- forward() on every row, no code of this chain -- the eager pipelined loop of this scene differs from the reference loop in one ray of
    some poses (seen: ray 777 of the first pose, depth 0.39367 against 0.39353, in `parts=1` and `parts=2` alike, run after run): that is the
    loops', not the field's.  The poses are therefore the first two of a seeded sequence for which the switch-off loops agree bit for bit; the
    precondition is established here, on the parent's path only, and the test below then holds the switch-on loops to the same equality."""
    from ngp_harness import scene
    from ngp_harness.model import Renderer

    field = setup["field"]
    _configure(field, "eval", 0.7)
    assert not getattr(field, "fused_light_infer", False)
    torch.manual_seed(0)
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        r.update_extra_state_device()
    frames, tried = [], 0
    for pose in scene.rand_poses(8, 1.6, np.random.default_rng(11)):
        o, d = scene.get_rays(pose, scene.intrinsics(32, 32), 32, 32)
        ro, rd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        tried += 1
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            a = r.render_infer(ro, rd, slots_per_ray=4, **KW)
            p = r.render_infer_pipelined(ro, rd, slots_per_ray=4, parts=2, **KW)
        if torch.equal(a[0], p[0]) and torch.equal(a[1], p[1]):
            frames.append((ro, rd))
        if len(frames) == 2:
            break
    print(f"poses tried for two on which the switch-off loops agree: {tried}")
    assert len(frames) == 2, tried
    return dict(field=field, r=r, frames=frames)


def test_the_three_loops_render_the_same_frame(dev, frame_setup, monkeypatch):
    """fused_light_infer = True: render_infer, render_infer_pipelined and render_infer_graphed give the same image and depth; a second pose
    replays the graphs; changed normal-net weights and the flipped switch re-record them.
    The poses are ones on which the loops agree with the switch off (frame_setup): what is held here is that the fused chain keeps that."""
    import nerftex_hip

    field, r, frames = (frame_setup[k] for k in ("field", "r", "frames"))
    _configure(field, "eval", 0.7)
    calls = []
    entry = nerftex_hip.lib.nerftex_curved_light_infer
    monkeypatch.setattr(nerftex_hip.lib, "nerftex_curved_light_infer", lambda *a: (calls.append(1), entry(*a))[1])
    saved = field.normal_net.phi_net.layers[0].b.detach().clone()
    (ro, rd) = frames[0]
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            img_off, dep_off, _ = r.render_infer(ro, rd, slots_per_ray=4, **KW)
            assert not calls
            field.fused_light_infer = True
            img, dep, _ = r.render_infer(ro, rd, slots_per_ray=4, **KW)
            assert calls, "the reference loop goes through the fused chain, too"
            img_p, dep_p, _ = r.render_infer_pipelined(ro, rd, slots_per_ray=4, parts=2, **KW)
            img_g, dep_g, _ = r.render_infer_graphed(ro, rd, slots_per_ray=4, parts=2, block=2, **KW)
            assert float(img.std()) > 1e-3
            print(f"32 x 32 frame: largest |switch on - switch off| image {float((img - img_off).abs().max()):.3e}, depth {float((dep - dep_off).abs().max()):.3e}")
            print(f"values that differ from render_infer: pipelined {int((img_p != img).sum())} image (max {float((img_p - img).abs().max()):.3e}) / "
                  f"{int((dep_p != dep).sum())} depth, graphed {int((img_g != img).sum())} image (max {float((img_g - img).abs().max()):.3e}) / "
                  f"{int((dep_g != dep).sum())} depth")
            assert torch.equal(img_p, img) and torch.equal(dep_p, dep)
            assert torch.equal(img_g, img) and torch.equal(dep_g, dep)
            graphs = r._infer_graphs
            img_2, dep_2, _ = r.render_infer_graphed(*frames[1], slots_per_ray=4, parts=2, block=2, **KW)
            assert r._infer_graphs is graphs, "another pose replays the recorded graphs"
            want_2 = r.render_infer(*frames[1], slots_per_ray=4, **KW)
            assert torch.equal(img_2, want_2[0]) and torch.equal(dep_2, want_2[1])
            with torch.no_grad():
                # in place, version counter bumped (as an optimizer step does): a new weight block.  (A bias: these rows' l1 norms are above their
                # Lipschitz bound, so a scaled W is normalised back to the same matrix)
                field.normal_net.phi_net.layers[0].b.add_(0.5)
            img_new, dep_new, _ = r.render_infer_graphed(ro, rd, slots_per_ray=4, parts=2, block=2, **KW)
            assert r._infer_graphs is not graphs, "changed normal-net weights re-record the graphs"
            want = r.render_infer(ro, rd, slots_per_ray=4, **KW)
            assert torch.equal(img_new, want[0]) and torch.equal(dep_new, want[1]) and not torch.equal(img_new, img)
            graphs = r._infer_graphs
            field.fused_light_infer = False
            n_calls = len(calls)
            img_f, dep_f, _ = r.render_infer_graphed(ro, rd, slots_per_ray=4, parts=2, block=2, **KW)
            assert r._infer_graphs is not graphs and len(calls) == n_calls, "the flipped switch re-records the graphs, through forward()"
            want = r.render_infer(ro, rd, slots_per_ray=4, **KW)
            assert torch.equal(img_f, want[0]) and torch.equal(dep_f, want[1])
    finally:
        field.fused_light_infer = False
        with torch.no_grad():
            field.normal_net.phi_net.layers[0].b.copy_(saved)


def test_switch_off_is_forward_on_all_rows(dev, setup, monkeypatch):
    """Without the attribute (and with it False) infer() is forward() on every row, whatever `live` says, and the new entry is not called."""
    import nerftex_hip

    field, x, d = setup["field"], setup["x"], setup["d"]
    _configure(field, "eval", 0.7)
    calls = []
    entry = nerftex_hip.lib.nerftex_curved_light_infer
    monkeypatch.setattr(nerftex_hip.lib, "nerftex_curved_light_infer", lambda *a: (calls.append(1), entry(*a))[1])
    none_live = (torch.zeros(1, dtype=torch.int32, device=dev), 5)
    for state in ("absent", False):
        if state == "absent":
            if hasattr(field, "fused_light_infer"):
                del field.fused_light_infer
        else:
            field.fused_light_infer = False
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert not field._infer_light_fused(x, d) and not field._infer_fused(x, d)
            sigma, rgbs = field.infer(x, d, none_live)
            want_s, want_c, _ = field(x, d)
        assert sigma.dtype == torch.float32 and rgbs.dtype == torch.float32
        assert torch.equal(sigma, want_s.float()) and torch.equal(rgbs, want_c.float()) and float(sigma.max()) > 0
    assert not calls
    field.fused_light_infer = True
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            sigma, rgbs = field.infer(x, d)
        assert len(calls) == 1 and torch.equal(sigma, want_s.float()), "the switch on: one library call, forward()'s sigma"
        with torch.no_grad():  # no autocast: the chain does not apply
            assert not field._infer_light_fused(x, d)
    finally:
        field.fused_light_infer = False


def test_eager_scratch_is_one_buffer_per_stream(dev, setup):
    """As tests/test_gpu_curved_infer.py's test of the same name, for the light chain: infer() keeps ONE scratch buffer per stream in
    `_infer_scratch`, grown to the largest batch seen (a field of its own: the shared one has rendered frames on several streams)."""
    from nerftex_hip import lib

    field, _ = _sh_field(dev)
    field.fused_light_infer = True
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for n in (384, 128):
            x, d = setup["xm"][:n].contiguous(), setup["dm"][:n].contiguous()
            assert field._infer_light_fused(x, d)
            sigma, rgbs = field.infer(x, d)
            assert sigma.shape == (n,) and rgbs.shape == (n, 3) and float(sigma.max()) > 0
    held = field._infer_scratch
    assert len(held) == 1 and next(iter(held.values())).numel() == lib.nerftex_curved_light_infer_scratch_bytes(384)


@pytest.mark.parametrize("kw", (dict(hidden_dim=64), dict(prob_model=True), dict(bound_output=True)), ids=("sigma64", "prob_model", "bound_output"))
def test_other_shapes_go_through_forward(dev, setup, monkeypatch, kw):
    """A 64-wide sigma net, the probabilistic table and bounded angles are not the entry's: with the switch on, infer() still serves them by
    forward() on all rows and never hands them to the library."""
    import nerftex_hip

    kw = dict(kw)
    bound_output = kw.pop("bound_output", False)
    field, _ = _sh_field(dev, **kw)
    field.normal_net.bound_output = bound_output
    field.fused_light_infer = True
    calls = []
    entry = nerftex_hip.lib.nerftex_curved_light_infer
    monkeypatch.setattr(nerftex_hip.lib, "nerftex_curved_light_infer", lambda *a: (calls.append(1), entry(*a))[1])
    x, d = setup["x"][:256].contiguous(), setup["d"][:256].contiguous()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert not field._infer_light_fused(x, d)
        torch.manual_seed(4)  # (prob_model draws its noise with torch.randn)
        sigma, rgbs = field.infer(x, d, (torch.zeros(1, dtype=torch.int32, device=dev), 5))
        torch.manual_seed(4)
        want_s, want_c, _ = field(x, d)
    assert not calls
    assert torch.equal(sigma, want_s.float()) and torch.equal(rgbs, want_c.float()) and float(sigma.max()) > 0
