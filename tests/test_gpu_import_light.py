"""GPU: an imported texture rendered through the SH-lit curved field -- nerftex_planar_light_lookup against nerftex_planar_lookup (bit for bit),
the framework's grid_sample(mode='nearest') (bit for bit) and the float64 bound of tests/planar_float64.py; nerftex_curved_light_import_infer
under the rows contract, its shading normal and colour against forward() inside the bounds of tests/import_light_float64.py and
tests/sh_light_float64.py; the reference's own run (tests/golden/ref_python_import_field_sh.npz); a 32 x 32 frame through the three loops.
Every comparison prints its largest error-to-bound ratio (DESIGN.md 4.17 records them)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import import_light_float64 as il64
import normal_net_float64 as nn64
import planar_float64 as pf
import sh_light_float64 as f64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.5
KINK_CAP = 0.02  # (tests/test_gpu_curved_light_infer.py's)
KW = dict(dt_gamma=0.0, max_steps=256)
P_LOOKUP = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lit_field(dev, h_threshold=0.0625):
    """tests/test_gpu_curved_light_infer.py's star-flower field (a normal net whose angles are of order 1) with the import's threshold."""
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=h_threshold, light_model="SH").to(dev)
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
    return field.eval()


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


# ---- 1. the plain lookup ------------------------------------------------------------------------------------------------------------------------------------

def _hand_placed(H, W):
    """(u, v) at every texel centre, exactly half-way between neighbouring texels along each axis (ix = k + 0.5: round half to even), at +-1 and
    one fp32 step outside, paired with seeded partners."""
    one = np.float32(1)

    def axis(n):
        if n == 1:
            return [np.float32(0), one, -one, np.float32(0.5)]
        c = [np.float32(2 * k) / np.float32(n - 1) - one for k in range(n)]
        h = [np.float32(2 * k + 1) / np.float32(n - 1) - one for k in range(n - 1)]
        return c + h + [one, -one, np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(-2)), np.float32(1.5), np.float32(-3)]

    us, vs = axis(H), axis(W)
    return np.float32([(u, v) for u in us for v in vs])


@pytest.fixture(scope="module")
def lookup_field(dev):
    return _lit_field(dev)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (5, 4)])
@pytest.mark.parametrize("rescale", [True, False], ids=["modeA", "modeB"])
def test_plain_lookup_against_the_unlit_lookup_grid_sample_and_float64(dev, lookup_field, H, W, rescale):
    field = lookup_field
    phi_map, local_map, sample, ids_map = il64.seeded_light_maps(H, W, P_LOOKUP)
    field._init_import_state()
    field.import_field(pf.seeded_map(H, W), 1.0 / H, rescale=rescale, phi_embed=phi_map, local_tbn=local_map, sample_tbn=sample, sample_tbn_ids=ids_map)
    assert np.allclose(field.bounds, pf.map_bounds(H, W), rtol=1e-6)
    field.bounds = list(pf.map_bounds(H, W))  # (the exact values case_points inverts)
    rate, offset = (1.0, 0.0) if rescale else (1.7, 0.01)
    field.set_uv_utilize_rate(rate), field.set_sdf_offset(offset)
    hand = _hand_placed(H, W)
    b0, b1 = (np.float32(b) for b in field.bounds)
    hand_xyz = np.concatenate([hand if rescale else hand * np.float32([b0, b1]), np.zeros((len(hand), 1), np.float32)], -1).astype(np.float32)
    x = torch.from_numpy(np.concatenate([pf.case_points(H, W, 1024, rescale, rate, offset), hand_xyz], 0)).to(dev)
    p_uv, sdf, mask, xin, phi, ids, local, smp = field._import_light_lookup(x)
    w_uv, w_sdf, w_mask, w_xin = field._import_lookup(x)
    assert torch.equal(p_uv, w_uv) and torch.equal(sdf, w_sdf) and torch.equal(mask, w_mask), "p_uv, sdf and mask: nerftex_planar_lookup's bits"
    assert torch.equal(xin.view(torch.int16), w_xin.view(torch.int16)), "xin: nerftex_planar_lookup's bits"
    assert int(mask.sum()) > 0 and int((~mask).sum()) > 0
    # the nearest reads: the framework's grid_sample fed the kernel's own p_uv, on every row
    grid = p_uv[None, None]
    gs = torch.nn.functional.grid_sample

    def image(m):
        return m.permute(2, 1, 0).unsqueeze(0)

    want_id = gs(image(field.sample_tbn_ids_imported[..., None]), grid, mode="nearest", align_corners=True, padding_mode="zeros")[0, 0, 0].long()
    want_local = gs(image(field.local_tbn_imported), grid, mode="nearest", align_corners=True, padding_mode="zeros")[0, :, 0].permute(1, 0).reshape(-1, 3, 3)
    assert torch.equal(ids.long(), want_id), int((ids.long() != want_id).sum())
    assert torch.equal(local, want_local), int((local != want_local).any(-1).any(-1).sum())
    assert torch.equal(smp, field.sample_tbn_inv_imported[want_id])
    if H * W > 1:
        assert len(set(ids.tolist())) > 1 and bool((local == 0).all(-1).all(-1).any()), "several patches, and rows outside the map"
    # the hand-placed half-way points really sit on ties where the extents allow the coordinate to be exact
    iu = ((p_uv[-len(hand):, 0] + 1) / 2) * (H - 1)
    if H in (2, 5):
        assert int(((iu - iu.floor()) == 0.5).sum()) > 0
    # the bilinear phi read inside the feature read's float64 bound (the fp32 value, and its narrowing)
    value, bound = pf.bilinear(phi_map, p_uv[:, 0].cpu().numpy(), p_uv[:, 1].cpu().numpy())
    for name, got in (("fp32", phi.double().cpu().numpy()), ("narrowed", phi.half().double().cpu().numpy())):
        ratio = np.abs(got - value) / bound
        print(f"map {H}x{W} {'A' if rescale else 'B'}: phi {name}, largest error / bound {float(ratio.max()):.3f}")
        assert ratio.max() <= 1.0


# ---- 2. the chain -------------------------------------------------------------------------------------------------------------------------------------------

CONFIGS = [("eval", 1.0), ("eval", 0.7), ("train", 1.0)]


def _configure(field, mode, fc, visual="Full"):
    field.train(mode == "train")
    field.fc_weight, field.light_visual_mode = fc, visual


def _marks(dev, n):
    marked = torch.zeros(n, dtype=torch.bool, device=dev)
    marked[::7] = True       # single slots
    marked[64:96] = True     # a whole 32-row step of an FFMLP wave
    if n >= 384:
        marked[256:384] = True   # a whole 128-row workgroup
    return marked


def _chain_points(n, bounds, h, seed=5):
    """n points over the slab and past every edge of it (mode A: u, v = x, y and sdf = z bounds[0]), four consecutive rows sharing a direction."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32) * np.float32([1.1, 1.1, 1.4 * h / bounds[0]])
    d = rng.normal(size=(n // 4, 3)).astype(np.float32)
    d = np.repeat(d / np.linalg.norm(d, axis=-1, keepdims=True), 4, axis=0)
    return x, d


def _reference(field, x, d, mode, fc):
    """What forward() (the switch off) computes for the batch, and the float64 helper's shading normal with its bound from the plain lookup's
    outputs (forward()'s own inputs to the normal net and the rotations).  Computed once per configuration and shared."""
    _configure(field, mode, fc)
    assert not getattr(field, "fused_light_infer", False)
    handed = {}
    handle = field.light_net.register_forward_pre_hook(lambda m, a, k: handed.update(geo=a[0], n=a[1]), with_kwargs=True)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            _, _, h_mask, xin, phi, _, local, smp = field._import_light_lookup(x)
            sigma, color, _ = field(x, d)
            ones = torch.ones(x.shape[0], 1, dtype=handed["geo"].dtype, device=x.device)
            brdf = field.light_net.brdf_layer(torch.cat([handed["geo"], ones], dim=-1))
    finally:
        handle.remove()
    weights, biases, _, _ = nn64.pack(field.normal_net)
    ref = il64.fine_normal(phi.half().cpu().numpy(), xin[:, :16].cpu().numpy(), xin[:, 16:28].cpu().numpy(), weights, biases, local.cpu().numpy(),
                           smp.cpu().numpy(), fc_weight=fc, blend=mode == "eval")
    assert sigma.dtype == torch.float32 and color.dtype == torch.float32
    return dict(sigma=sigma, color=color, mask=h_mask, brdf=brdf, normal_fwd=handed["n"].float(), normal=ref["normal"], bound_normal=ref["bound_normal"],
                local=local)


@pytest.fixture(scope="module")
def setup(dev):
    field = _lit_field(dev)
    H, W, P = 24, 20, 5
    phi_map, local_map, sample, ids_map = il64.seeded_light_maps(H, W, P)
    field.import_field(pf.seeded_map(H, W, seed=21), 1.0 / 32, phi_embed=phi_map, local_tbn=local_map, sample_tbn=sample, sample_tbn_ids=ids_map)
    assert field.rescale
    n = 1024
    xn, dn = _chain_points(n, field.bounds, field.h_threshold)
    x, d = torch.from_numpy(xn).to(dev), torch.from_numpy(dn).to(dev).contiguous()
    marked = _marks(dev, n)
    xm, dm = x.clone(), d.clone()
    xm[marked] = 1e30
    dm[marked, 0] = 1e30
    refs = {cfg: _reference(field, x, d, *cfg) for cfg in CONFIGS}
    inside = float(refs[CONFIGS[0]]["mask"].float().mean())
    assert 0.2 < inside < 0.8, inside  # both sides of the mask are exercised
    return dict(field=field, x=x, d=d, xm=xm, dm=dm, marked=marked, refs=refs)


def _call(field, x, d, live=None, want_normal=True):
    """nerftex_curved_light_import_infer through the descriptor CurvedField builds, outputs pre-filled with the sentinel."""
    from nerftex_hip import check, lib, stream

    n, dev = x.shape[0], x.device
    sigma = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
    rgbs = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dev)
    normal = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dev) if want_normal else None
    scratch = torch.empty(lib.nerftex_curved_light_import_infer_scratch_bytes(n), dtype=torch.uint8, device=dev)
    field.fused_light_infer = True
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._infer_light_import_fused(x, d)
            desc, keep = field._infer_light_import_desc(x, d, live, sigma, rgbs, scratch, normal)
            check(lib.nerftex_curved_light_import_infer(ctypes.byref(desc), stream()))
        torch.cuda.synchronize()
    finally:
        field.fused_light_infer = False
    return sigma, rgbs, normal


# B = 128 with no unit and with one (of 5 rows, and of the whole batch); B = 384 with two of its three workgroups live
@pytest.mark.parametrize("n,units,rows_per_unit,want_live", [(128, 0, 5, 0), (128, 1, 5, 5), (128, 1, 128, 128), (384, 2, 128, 256), (384, None, 0, 384)])
def test_rows_contract_at_the_c_abi(dev, setup, n, units, rows_per_unit, want_live):
    """Unmarked live rows: sigma and the mask are forward()'s, bit for bit, and the colour is shaded; marked live rows (one of them, row 0, inside
    every live unit) are exactly 0; rows >= live keep the sentinel in all three outputs."""
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
    assert torch.equal(sigma[plain], ref["sigma"][:n][plain]), "sigma: forward()'s bits"
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
    assert torch.equal(sigma[plain], ref["sigma"][plain]), "sigma and the mask of the unmarked rows: forward()'s bits"
    assert torch.equal((sigma != 0)[plain], (ref["sigma"] != 0)[plain]) and not rgbs[plain & ~ref["mask"]].any()
    rows = (plain & ref["mask"]).cpu().numpy()
    assert rows.sum() > 200
    tag = f"{mode} fc={fc}"
    _inside(f"kernel shading normal | {tag}", normal.cpu().numpy()[rows], ref["normal"][rows], ref["bound_normal"][rows])
    # the framework's own evaluation under the same bound (a bound forward() misses would be a wrong bound)
    _inside(f"forward() shading normal | {tag}", ref["normal_fwd"].cpu().numpy()[rows], ref["normal"][rows], ref["bound_normal"][rows])
    print(f"median bound on a component of the shading normal | {tag}: {float(np.median(ref['bound_normal'][rows])):.3e}")
    # the normal is not the texel frame's third row: the net's angles are of order 1 and the patch frame turns it again
    assert float((normal - ref["local"][:, 2]).abs().max(-1).values[torch.from_numpy(rows).to(dev)].median()) > 0.05
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
    at_fwd = f64.shade(a_h, sw_h, ref["normal_fwd"].cpu().numpy(), d, env, field.light_net.gamma, field.light_net.use_specular, mask)
    _inside(f"forward() {visual}", fwd.cpu().numpy(), at_fwd[key], at_fwd["bound_" + key], at_fwd["kink_" + key])
    assert float(rgbs[torch.from_numpy(plain & mask).to(dev)].std()) > 1e-3
    print(f"{visual}: largest |fused - forward()| over the unmarked rows {float((rgbs - fwd).abs()[torch.from_numpy(plain).to(dev)].max()):.3e}")


def test_two_calls_give_the_same_bits_and_infer_goes_through_the_entry(dev, setup, monkeypatch):
    import nerftex_hip

    field = setup["field"]
    _configure(field, "eval", 0.7)
    a = _call(field, setup["xm"], setup["dm"])
    b = _call(field, setup["xm"], setup["dm"])
    for p, q in zip(a, b):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
    calls = []
    entry = nerftex_hip.lib.nerftex_curved_light_import_infer
    monkeypatch.setattr(nerftex_hip.lib, "nerftex_curved_light_import_infer", lambda *args: (calls.append(1), entry(*args))[1])
    x, d = setup["x"], setup["d"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        want_s, want_c, _ = field(x, d)
        sigma, rgbs = field.infer(x, d)
        assert not calls and torch.equal(sigma, want_s.float()) and torch.equal(rgbs, want_c.float()), "the switch off: forward() on all rows"
        dens = field.density(x)
        assert torch.equal(dens["sigma"], want_s), "density() takes the planar lookup for the lit field, too"
        field.fused_light_infer = True
        try:
            sigma, rgbs = field.infer(x, d)
            assert len(calls) == 1 and torch.equal(sigma, want_s.float())
            odd_s, odd_c = field.infer_padded(x[:333].contiguous(), d[:333].contiguous())
            assert len(calls) == 2 and torch.equal(odd_s, sigma[:333]) and torch.equal(odd_c, rgbs[:333]), "a padded batch: the same bits per row"
        finally:
            field.fused_light_infer = False


# ---- 3. the reference's own run -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_field(dev):
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_python_import_field_sh.npz"))
    field = _lit_field(dev, float(g["h_threshold"]))
    il64.load_normal_net(field.normal_net, g)
    with torch.no_grad():
        field.sigma_net.weights.copy_(torch.from_numpy(g["w_sigma"]))
        field.light_net.brdf_layer.weights.copy_(torch.from_numpy(g["w_brdf"]))
        field.light_net.envSHs.copy_(torch.from_numpy(g["env_shs"]))
    return field, g


@pytest.mark.parametrize("mode,times", [("A", 1), ("B", 2)])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "forward"])
def test_the_field_reproduces_the_reference_fixture(dev, golden_field, mode, times, fused):
    """The tolerances tests/test_gpu_curved_light_infer.py applies to ref_python_curvedfield_sh.npz (the project's for this chain's 16-bit path):
    5e-3 per component on the shading normals, 2e-2 on the colours, mask equality, sigma rtol 3e-2 / atol 3e-3 -- both rescale states, fc_weight
    1.0 and 0.7, the four visual modes; through the fused entry and through forward()."""
    field, g = golden_field
    field._init_import_state()
    il64.import_fixture_maps(field, g, times)
    assert field.rescale == (mode == "A")
    x, d = torch.from_numpy(g["xyz"]).to(dev), torch.from_numpy(g["dirs"]).to(dev)
    hm = g[mode + "_h_mask"]
    field.eval()
    handed = {}
    handle = field.light_net.register_forward_pre_hook(lambda m, a, k: handed.update(n=a[1]), with_kwargs=True)
    try:
        for fc in (1.0, 0.7):
            for visual in ("Full", "Specular", "Diffuse", "Albedo"):
                _configure(field, "eval", fc, visual)
                if fused:
                    sigma, rgbs, normal = _call(field, x, d)
                else:
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                        sigma, rgbs, _ = field(x, d)
                    sigma, rgbs, normal = sigma.float(), rgbs.float(), handed["n"].float()
                want = g[f"{mode}_fc{fc}_color_{visual.lower()}"]
                err = np.abs(rgbs.cpu().numpy() - want)
                nerr = np.abs(normal.cpu().numpy() - g[f"{mode}_fc{fc}_shading_normal"])[hm]
                shaded = ((sigma != 0) | (rgbs != 0).any(-1)).cpu().numpy()
                print(f"{mode} fc={fc} {visual} {'fused' if fused else 'forward()'}: colour max |diff| {float(err.max()):.2e}, shading normal max |diff| "
                      f"{float(nerr.max()):.2e}, {int(hm.sum())} rows inside the mask")
                assert np.array_equal(shaded, hm)
                assert err.max() <= 2e-2
                assert nerr.max() <= 5e-3
                np.testing.assert_allclose(sigma.cpu().numpy(), g[mode + "_sigma"], rtol=3e-2, atol=3e-3)
    finally:
        handle.remove()
        field.light_visual_mode = "Full"


# ---- 4. a frame ----------------------------------------------------------------------------------------------------------------------------------------------

def test_a_frame_of_the_imported_lit_field(dev, monkeypatch):
    """32 x 32 through render_infer, render_infer_pipelined and render_infer_graphed with `fused_light_infer` on, behind initialize_states(): the
    same image bit for bit, not a trivial one; other maps re-record the graphs and change the image; switch_import() gives the mesh field's."""
    import nerftex_hip
    from ngp_harness import scene
    from ngp_harness.model import Renderer

    field = _lit_field(dev)
    _configure(field, "eval", 0.7)
    field.fused_light_infer = True
    frames = []
    for pose in scene.rand_poses(2, 1.6, np.random.default_rng(11)):
        o, d = scene.get_rays(pose, scene.intrinsics(32, 32), 32, 32)
        frames.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
    r_mesh = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        r_mesh.update_extra_state_device()
        mesh_ref = r_mesh.render_infer(*frames[0], slots_per_ray=4, **KW)[:2]
    mesh_stamp = field.graph_stamp()
    calls = []
    entry = nerftex_hip.lib.nerftex_curved_light_import_infer
    monkeypatch.setattr(nerftex_hip.lib, "nerftex_curved_light_import_infer", lambda *a: (calls.append(1), entry(*a))[1])
    H = W = 64
    maps = dict(zip(("phi_embed", "local_tbn", "sample_tbn", "sample_tbn_ids"), il64.seeded_light_maps(H, W, 5)))
    field.import_field(pf.seeded_map(H, W, seed=21), 1.0 / 64, **maps)  # bounds (0.5, 0.5); rescale: u, v = x, y and sdf = z / 2
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)  # (a grid of its own: initialize_states keeps a maximum)
    r.initialize_states(2)
    assert int((r.density_grid[0] > 0).sum()) > 0 and int((r.density_grid[0] == 0).sum()) > 0
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            img, dep, _ = r.render_infer(*frames[0], slots_per_ray=4, **KW)
            assert calls, "the reference loop goes through the fused chain"
            img_p, dep_p, _ = r.render_infer_pipelined(*frames[0], slots_per_ray=4, parts=2, **KW)
            img_g, dep_g, _ = r.render_infer_graphed(*frames[0], slots_per_ray=4, parts=2, block=2, **KW)
            print(f"values that differ from render_infer: pipelined {int((img_p != img).sum())} image / {int((dep_p != dep).sum())} depth, graphed "
                  f"{int((img_g != img).sum())} image / {int((dep_g != dep).sum())} depth; image std {float(img.std()):.3e}")
            assert torch.equal(img_p, img) and torch.equal(dep_p, dep)
            assert torch.equal(img_g, img) and torch.equal(dep_g, dep)
            assert float(img.std()) > 1e-3 and not torch.equal(img, mesh_ref[0])
            graphs = r._infer_graphs
            img_2, dep_2, _ = r.render_infer_graphed(*frames[1], slots_per_ray=4, parts=2, block=2, **KW)
            assert r._infer_graphs is graphs, "another pose replays the recorded graphs"
            want_2 = r.render_infer(*frames[1], slots_per_ray=4, **KW)
            assert torch.equal(img_2, want_2[0]) and torch.equal(dep_2, want_2[1])
            # other maps (the features and the rescale state as they were): the graphs are re-recorded and the image changes
            other = dict(zip(("phi_embed", "local_tbn", "sample_tbn", "sample_tbn_ids"), il64.seeded_light_maps(H, W, 5, seed=9)))
            field.import_field(pf.seeded_map(H, W, seed=21), 1.0 / 64, rescale=True, **other)
            img_o, dep_o, _ = r.render_infer_graphed(*frames[0], slots_per_ray=4, parts=2, block=2, **KW)
            assert r._infer_graphs is not graphs, "other maps re-record the graphs"
            want = r.render_infer(*frames[0], slots_per_ray=4, **KW)
            assert torch.equal(img_o, want[0]) and torch.equal(dep_o, want[1]) and not torch.equal(img_o, img)
            assert torch.equal(dep_o, dep), "the density does not read the normal's maps"
            # back to the mesh field, behind the renderer that holds the mesh's occupancy grid: its frame bit for bit
            field.switch_import()
            assert not field.imported and field.graph_stamp() == mesh_stamp
            n_calls = len(calls)
            img_m, dep_m, _ = r_mesh.render_infer(*frames[0], slots_per_ray=4, **KW)
            assert torch.equal(img_m, mesh_ref[0]) and torch.equal(dep_m, mesh_ref[1]) and len(calls) == n_calls
    finally:
        field.fused_light_infer = False
