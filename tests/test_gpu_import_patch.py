"""GPU: an exported feature patch rendered through the curved field -- nerftex_patch_lookup / nerftex_patch_light_lookup against the float64
model of tests/patch_import_float64.py (its derived bound), against CurvedField._patch_embed_reference (the same bound) and against
nerftex_knn_query (bit for bit); the two lane mappings; nerftex_curved_patch_infer against its pieces and nerftex_curved_light_patch_infer
against forward() under the rows contract; a frame through the three inference loops; export_field -> import_patch; a field that never
imported.  Every comparison with a bound prints or reports its worst element."""
import ctypes
import os

import numpy as np
import pytest
import torch

import import_light_float64 as il64
import normal_net_float64 as nn64
import patch_float64 as pf64
import patch_import_float64 as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.5
KW = dict(dt_gamma=0.0, max_steps=256)
PATCHES = [(3, False), (12, False), (12, True), (33, False)]  # (S, per-point normals that differ)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _field(dev, lit, h_threshold=pm.H_THRESHOLD):
    """The star-flower field of the other import tests (lit: a normal net whose angles are of order 1)."""
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=h_threshold, light_model="SH" if lit else None).to(dev)
    gen = torch.Generator(device=dev).manual_seed(2)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
        if lit:
            field.normal_net.encoder.embeddings.uniform_(-0.5, 0.5)
            field.light_net.envSHs[1:].normal_(0, 0.1, generator=gen)
            for mlp in (field.normal_net.phi_net, field.normal_net.theta_net):
                for layer in mlp.layers:
                    layer.W.mul_(6.0)
                    layer.b.normal_(0, 0.3, generator=gen)
                    layer.c.fill_(2.0)
    return field.eval()


@pytest.fixture(scope="module")
def lit_field(dev):
    return _field(dev, True)


@pytest.fixture(scope="module")
def static_field(dev):
    return _field(dev, False)


def _import(field, S, per_point=False):
    patch = pm.seeded_patch(S, per_point, lit=field._lit())
    field._init_import_state()
    field.import_patch(**patch)
    return patch


def _lookup(field, x, lit):
    """The plain entry over the field's patch, every output pre-filled with a sentinel."""
    from nerftex_hip import check, lib, ptr, stream

    n, dev, f = x.shape[0], x.device, field.features_imported
    sdf = torch.full((n,), SENTINEL, device=dev)
    mask = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    normal = torch.full((n, 3), SENTINEL, device=dev)
    xin = torch.full((n, 48), SENTINEL, dtype=torch.float16, device=dev)
    idx = torch.full((n, 8), -9, dtype=torch.int32, device=dev)
    dis, w = torch.full((n, 8), SENTINEL, device=dev), torch.full((n, 8), SENTINEL, device=dev)
    head = (field._patch_knn.value, ptr(x), ptr(field.patch_geom), ptr(f))
    tail = (f.shape[0], float(field.h_threshold), 12, n, ptr(sdf), ptr(mask), ptr(normal), ptr(xin), ptr(idx), ptr(dis), ptr(w))
    if not lit:
        check(lib.nerftex_patch_lookup(*head, *tail, stream()))
        return sdf, mask, normal, xin, idx, dis, w
    phi, tbn = torch.full((n, 8), SENTINEL, device=dev), torch.full((n, 9), SENTINEL, device=dev)
    check(lib.nerftex_patch_light_lookup(*head, ptr(field.patch_lit), *tail, ptr(phi), ptr(tbn), stream()))
    return sdf, mask, normal, xin, idx, dis, w, phi, tbn


# ---- 1. the plain lookups -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S,per_point", PATCHES)
def test_plain_lookups_against_float64_the_op_by_op_route_and_the_search(dev, lit_field, S, per_point):
    field = lit_field
    patch = _import(field, S, per_point)
    normals = pm.full_normals(patch)
    sides = np.zeros((3, 2), np.int64)
    for B in (1, 200, 1000):
        xn = pm.case_queries(patch, B)
        x = torch.from_numpy(xn).to(dev)
        sdf, mask, normal, xin, idx, dis, w, phi, tbn = _lookup(field, x, True)
        plain = _lookup(field, x, False)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(plain, (sdf, mask, normal, xin, idx, dis, w))), "the unlit lookup: the same bits"
        k_idx, k_dis = field._patch_neighbours(x)
        assert torch.equal(idx, k_idx) and torch.equal(dis, k_dis), "idx and dis: nerftex_knn_query's bits"
        assert bool((xin[:, 41:] == 1).all())
        pm.check_neighbours(patch["points"], xn, idx.cpu().numpy())
        m = pm.resample(patch["points"], normals, patch["features"], xn, idx.cpu().numpy(), pm.H_THRESHOLD, patch["phi_embed"], patch["local_tbn"])
        rows, decided = m["compare"], ~m["undecided"]
        assert m["undecided"].mean() <= 0.02, (B, float(m["undecided"].mean()))
        sides += np.asarray(m["sides"])
        with torch.no_grad():
            r_embed, r_nc, r_mask, r_fine, r_sdf, r_normal, r_idx, r_dis, r_w, r_phi, r_tbn = field._patch_embed_reference(x, with_fine_normal=True, details=True)
        for name, got, ref, key in (("normal", normal, r_normal, "normal"), ("sdf", sdf, r_sdf, "sdf"), ("weights", w, r_w, "weights"),
                                    ("embed", xin[:, :41], r_embed.half(), "embed"), ("phi", phi, r_phi, "phi"), ("tbn", tbn, r_tbn.reshape(-1, 9), "tbn")):
            pm.assert_within(got.double().cpu().numpy(), m[key], rows, f"kernel {name} S={S} B={B}")
            pm.assert_within(ref.double().cpu().numpy(), m[key], rows, f"op-by-op {name} S={S} B={B}")
            # (against the route's fp32 values as it returns them: two values narrowed to half apart can differ by a whole half ulp, twice the bound's share)
            plain_ref = r_embed if name == "embed" else ref
            pm.assert_within(got.double().cpu().numpy(), (plain_ref.double().cpu().numpy(), m[key][1]), rows, f"kernel against op-by-op {name} S={S} B={B}")
        got_mask = mask.bool().cpu().numpy()
        assert np.array_equal(got_mask[decided], m["mask"][decided]) and np.array_equal(r_mask.cpu().numpy()[decided], m["mask"][decided])
        failed = ~m["above"] & decided
        assert not got_mask[failed].any(), "a row that fails the direct-above test is outside the mask"
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._patch_fused(x) and torch.equal(field.embed(x)[2], mask.bool())
    assert (sides[:, :] > 0).all(), sides.tolist()  # decided rows on both sides of each of the three tests
    print(f"S={S}: decided rows (inside, outside) of the direct-above test, |sdf| < h, min dis < h: {sides.tolist()}")


# ---- 2. the chains against their pieces ------------------------------------------------------------------------------------------------------------------------

def _half_weights(n, seed, scale, dev):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-scale, scale, n).astype(np.float16)).to(dev)


def _marked(x, d):
    marked = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    marked[::7] = True
    marked[32:64] = True
    xm, dm = x.clone(), d.clone()
    xm[marked] = 1e30
    dm[marked, 0] = 1e30
    return marked, xm, dm


def _dirs(B, dev):
    d = np.random.default_rng(B).normal(size=(B, 3)).astype(np.float32)
    return torch.from_numpy(d / np.linalg.norm(d, axis=-1, keepdims=True)).to(dev)


@pytest.mark.parametrize("S,per_point", PATCHES)
def test_static_chain_is_its_pieces_under_the_rows_contract(dev, static_field, S, per_point):
    from nerftex_hip import CurvedPatchInferDesc, check, lib, ptr, stream

    field = static_field
    patch = _import(field, S, per_point)
    ws, wc = _half_weights(3072, 3, 0.6, dev), _half_weights(11264, 4, 0.25, dev)
    for B in (128, 384):
        x, d = torch.from_numpy(pm.case_queries(patch, B, seed=1)).to(dev), _dirs(B, dev)
        _, mask, normal, xin = _lookup(field, x, False)[:4]
        h = torch.empty(B, 16, dtype=torch.float16, device=dev)
        buf = torch.empty(B, 64, dtype=torch.float16, device=dev)
        check(lib.nerftex_ffmlp_inference(ptr(xin), ptr(ws), B, 48, 16, 32, 2, 0, 6, ptr(buf), ptr(h), stream()))
        sigma_raw, cin = torch.empty(B, dtype=torch.float16, device=dev), torch.empty(B, 32, dtype=torch.float16, device=dev)
        check(lib.nerftex_curved_mid_forward(ptr(h), ptr(normal), ptr(d), B, 1.0, 3, ptr(sigma_raw), ptr(cin), stream()))
        hc = torch.empty(B, 16, dtype=torch.float16, device=dev)
        check(lib.nerftex_ffmlp_inference(ptr(cin), ptr(wc), B, 32, 16, 64, 3, 0, 6, ptr(buf), ptr(hc), stream()))
        s16, c16 = torch.empty(B, dtype=torch.float16, device=dev), torch.empty(B, 3, dtype=torch.float16, device=dev)
        check(lib.nerftex_curved_out_forward(ptr(hc), 16, ptr(sigma_raw), ptr(mask), B, ptr(s16), ptr(c16), stream()))
        want_sigma, want_rgb = s16.float(), c16.float()
        assert float(want_sigma.max()) > 0 and float(want_rgb.max()) > 0  # (not a comparison of zeros)
        assert int((mask == 0).sum()) > 0 and not want_sigma[mask == 0].any() and not want_rgb[mask == 0].any(), "outside the mask: sigma 0 and colour 0"
        marked, xm, dm = _marked(x, d)
        scratch = torch.empty(lib.nerftex_curved_patch_infer_scratch_bytes(B), dtype=torch.uint8, device=dev)
        for units, rows_per_unit, live in ((0, 128, 0), (1, 128, 128), (None, 0, B), (B // 64, 64, B)):
            units_dev = None if units is None else torch.tensor([units], dtype=torch.int32, device=dev)
            sigma = torch.full((B,), SENTINEL, dtype=torch.float32, device=dev)
            rgbs = torch.full((B, 3), SENTINEL, dtype=torch.float32, device=dev)
            desc = CurvedPatchInferDesc(
                knn=field._patch_knn.value, xyz=ptr(xm), dirs=ptr(dm), B=B, n_points=S * S, geom=ptr(field.patch_geom), features=ptr(field.features_imported),
                n_features=16, h_threshold=pm.H_THRESHOLD, n_freqs=12, sigma_weights=ptr(ws), sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16,
                color_weights=ptr(wc), color_in=32, color_hidden=64, color_layers=3, color_out=3, fc_weight=1.0, eval=3, sigma=ptr(sigma), rgbs=ptr(rgbs),
                units_dev=ptr(units_dev), rows_per_unit=rows_per_unit, scratch=ptr(scratch), scratch_bytes=scratch.numel())
            check(lib.nerftex_curved_patch_infer(ctypes.byref(desc), stream()))
            torch.cuda.synchronize()
            rows = torch.arange(B, device=dev)
            plain, unused, past = (rows < live) & ~marked, (rows < live) & marked, rows >= live
            assert torch.equal(sigma[plain], want_sigma[plain]) and torch.equal(rgbs[plain], want_rgb[plain]), (B, units)
            assert bool((sigma[unused] == 0).all()) and bool((rgbs[unused] == 0).all())
            assert bool((sigma[past] == SENTINEL).all()) and bool((rgbs[past] == SENTINEL).all())


def _call_lit(field, x, d, live=None):
    """nerftex_curved_light_patch_infer through the descriptor CurvedField builds, outputs pre-filled with the sentinel."""
    from nerftex_hip import check, lib, stream

    n, dev = x.shape[0], x.device
    sigma = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
    rgbs = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dev)
    normal = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.nerftex_curved_light_patch_infer_scratch_bytes(n), dtype=torch.uint8, device=dev)
    field.fused_light_infer = True
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._infer_light_patch_fused(x, d)
            desc, keep = field._infer_light_patch_desc(x, d, live, sigma, rgbs, scratch, normal)
            check(lib.nerftex_curved_light_patch_infer(ctypes.byref(desc), stream()))
        torch.cuda.synchronize()
    finally:
        field.fused_light_infer = False
    return sigma, rgbs, normal


@pytest.mark.parametrize("S,per_point", PATCHES)
def test_lit_chain_is_its_pieces_under_the_rows_contract(dev, lit_field, S, per_point):
    """The lit chain has no plain entries for its back half; its pieces are the plain lit lookup and forward(): sigma and the mask are
    forward()'s bit for bit, the shading normal lies inside the float64 bound of tests/import_light_float64.py evaluated on the lookup's own
    outputs (ONE rotation: the second frame is the identity, which a half product leaves as it is), the colour within the 2e-2 the fixture
    tests apply to this back half; rows are independent (marked slots and rows past `live` as specified, every other row the unmarked call's
    bits)."""
    field = lit_field
    patch = _import(field, S, per_point)
    field.fc_weight, field.light_visual_mode = 0.7, "Full"
    weights, biases, _, _ = nn64.pack(field.normal_net)
    try:
        for B in (128, 384):
            x, d = torch.from_numpy(pm.case_queries(patch, B, seed=2)).to(dev), _dirs(B, dev)
            handed = {}
            handle = field.light_net.register_forward_pre_hook(lambda m, a, k: handed.update(n=a[1]), with_kwargs=True)
            try:
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    f_sigma, f_color, _ = field(x, d)
            finally:
                handle.remove()
            _, mask, normal_raw, xin, _, _, _, phi, tbn = _lookup(field, x, True)
            full_s, full_c, full_n = _call_lit(field, x, d)
            inside = mask.bool()
            assert int(inside.sum()) > 0 and int((~inside).sum()) > 0
            assert torch.equal(full_s, f_sigma.float()), "sigma and the mask: forward()'s bits"
            assert not full_c[~inside].any() and not full_s[~inside].any()
            eye = np.broadcast_to(np.eye(3, dtype=np.float32), (B, 3, 3))
            rows = inside.cpu().numpy()
            ref = il64.fine_normal(phi.half().cpu().numpy(), xin[:, :16].cpu().numpy(), xin[:, 16:28].cpu().numpy(), weights, biases, tbn.cpu().numpy().reshape(-1, 3, 3),
                                   eye, fc_weight=1.0, blend=False)
            # the eval blend of il64.fine_normal, restated with the coarse normal the lookup wrote in place of the planar chain's (0, 0, 1)
            fc = float(np.float32(0.7))
            c, e_c = nn64._unit(normal_raw.double().cpu().numpy(), np.zeros((B, 3)))
            c, e_c = nn64._unit(c, e_c)
            s_ = fc * ref["normal"] + (1 - fc) * c
            e_s = abs(fc) * ref["bound_normal"] + abs(1 - fc) * e_c + pm.U * (np.abs(fc * ref["normal"]) + 2 * np.abs((1 - fc) * c) + np.abs(s_))
            blend, bound = nn64._unit(s_, e_s)
            err = np.abs(full_n.double().cpu().numpy() - blend)
            print(f"S={S} B={B}: shading normal max error / bound {float((err / bound)[rows].max()):.3f}, against forward() "
                  f"{float((full_n - handed['n'].float()).abs()[inside].max()):.3e}; colour against forward() {float((full_c - f_color.float()).abs().max()):.3e}")
            assert (err <= bound)[rows].all()
            assert float((full_c - f_color.float()).abs().max()) <= 2e-2
            marked, xm, dm = _marked(x, d)
            for units, rows_per_unit, live in ((0, 128, 0), (1, 128, 128), (None, 0, B)):
                lv = None if units is None else (torch.tensor([units], dtype=torch.int32, device=dev), rows_per_unit)
                sigma, rgbs, normal = _call_lit(field, xm, dm, lv)
                r = torch.arange(B, device=dev)
                plain, unused, past = (r < live) & ~marked, (r < live) & marked, r >= live
                for got, want in ((sigma, full_s), (rgbs, full_c), (normal, full_n)):
                    assert torch.equal(got[plain], want[plain]), (B, units)
                    assert bool((got[unused] == 0).all()) and bool((got[past] == SENTINEL).all())
    finally:
        field.fc_weight = 1.0


# ---- 3. the reference's own runs ------------------------------------------------------------------------------------------------------------------------------

def _golden_fields(dev, name):
    g = np.load(os.path.join(ROOT, "tests", "golden", name))
    lit = "w_brdf" in g
    field = _field(dev, lit, float(g["h_threshold"]))
    with torch.no_grad():
        if lit:
            il64.load_normal_net(field.normal_net, g)
            field.sigma_net.weights.copy_(torch.from_numpy(g["w_sigma"]))
            field.light_net.brdf_layer.weights.copy_(torch.from_numpy(g["w_brdf"]))
            field.light_net.envSHs.copy_(torch.from_numpy(g["env_shs"]))
        else:
            c = np.load(os.path.join(ROOT, "tests", "golden", "ref_python_curvedfield.npz"))
            field.sigma_net.weights.copy_(torch.from_numpy(c["w_sigma"]))
            field.color_net.weights.copy_(torch.from_numpy(c["w_color"]))
    return field, g


def _model_of_fixture(g, idx, lit):
    return pm.resample(g["points"], np.ascontiguousarray(np.broadcast_to(g["normals"], g["points"].shape)), g["features"], g["xyz"], idx, float(g["h_threshold"]),
                       g["phi_embed"] if lit else None, g["local_tbn"] if lit else None)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_by_op"])
def test_the_field_reproduces_the_reference_fixture(dev, fused):
    """ref_python_import_patch.npz: the mask on the model's decided rows, the embedding inside the model's bound where the lookup enters, sigma and
    colour within the tolerances tests/test_gpu_import_field.py applies to the shared back half."""
    field, g = _golden_fields(dev, "ref_python_import_patch.npz")
    field.import_patch(features=g["features"], points=g["points"], normals=g["normals"])
    x, d = torch.from_numpy(g["xyz"]).to(dev), torch.from_numpy(g["dirs"]).to(dev)
    field.fused_glue = fused
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._patch_fused(x) == fused and field._infer_patch_fused(x, d) == fused
            embed, normal, mask = field.embed(x)
            sigma, color, _ = field(x, d)
            dens = field.density(x)
            got_s, got_c = field.infer(x, d)
    finally:
        field.fused_glue = True
    idx = field._patch_neighbours(x)[0].cpu().numpy()
    pm.check_neighbours(g["points"], g["xyz"], idx)
    m = _model_of_fixture(g, idx, False)
    decided, rows = ~m["undecided"], m["compare"]
    want_mask = g["h_mask"]
    assert np.array_equal(mask.cpu().numpy()[decided], want_mask[decided]) and m["undecided"].mean() <= 0.02
    pm.assert_within(embed.half().double().cpu().numpy(), m["embed"], rows, "the field's embedding")
    pm.assert_within(g["embed"].astype(np.float16).astype(np.float64), m["embed"], rows, "the fixture's embedding")
    ok = torch.from_numpy(decided).to(dev)
    want_s, want_c = torch.from_numpy(g["sigma"]).to(dev), torch.from_numpy(g["color"]).to(dev).float()
    assert torch.equal((sigma == 0)[ok], ~torch.from_numpy(want_mask).to(dev)[ok])
    torch.testing.assert_close(sigma.float()[ok], want_s[ok], rtol=3e-2, atol=3e-3)
    torch.testing.assert_close(color.float()[ok], want_c[ok], rtol=0, atol=2e-2)
    torch.testing.assert_close(dens["sigma"].float()[ok], want_s[ok], rtol=3e-2, atol=3e-3)
    assert got_s.dtype == torch.float32 and torch.equal(got_s, sigma.float()) and torch.equal(got_c, color.float())
    assert int(want_mask.sum()) > 50 and int((~want_mask).sum()) > 50


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "forward"])
def test_the_lit_field_reproduces_the_reference_fixture(dev, fused):
    """ref_python_import_patch_sh.npz with the tolerances tests/test_gpu_import_light.py applies to this back half: 5e-3 per component on the
    shading normals, 2e-2 on the colours, sigma rtol 3e-2 / atol 3e-3, the mask on the model's decided rows."""
    field, g = _golden_fields(dev, "ref_python_import_patch_sh.npz")
    field.import_patch(features=g["features"], points=g["points"], normals=g["normals"], local_tbn=g["local_tbn"], phi_embed=g["phi_embed"])
    x, d = torch.from_numpy(g["xyz"]).to(dev), torch.from_numpy(g["dirs"]).to(dev)
    idx = field._patch_neighbours(x)[0].cpu().numpy()
    pm.check_neighbours(g["points"], g["xyz"], idx)
    m = _model_of_fixture(g, idx, True)
    decided, hm = ~m["undecided"], g["h_mask"]
    assert m["undecided"].mean() <= 0.02
    handed = {}
    handle = field.light_net.register_forward_pre_hook(lambda mod, a, k: handed.update(n=a[1]), with_kwargs=True)
    try:
        for fc in (1.0, 0.7):
            for visual in ("Full", "Specular", "Diffuse", "Albedo"):
                field.fc_weight, field.light_visual_mode = fc, visual
                if fused:
                    sigma, rgbs, normal = _call_lit(field, x, d)
                else:
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                        sigma, rgbs, _ = field(x, d)
                    sigma, rgbs, normal = sigma.float(), rgbs.float(), handed["n"].float()
                err = np.abs(rgbs.cpu().numpy() - g[f"fc{fc}_color_{visual.lower()}"])[decided]
                nerr = np.abs(normal.cpu().numpy() - g[f"fc{fc}_shading_normal"])[hm & decided]
                shaded = ((sigma != 0) | (rgbs != 0).any(-1)).cpu().numpy()
                print(f"fc={fc} {visual} {'fused' if fused else 'forward()'}: colour max |diff| {float(err.max()):.2e}, shading normal max |diff| {float(nerr.max()):.2e}")
                assert np.array_equal(shaded[decided], hm[decided])
                assert err.max() <= 2e-2 and nerr.max() <= 5e-3
                np.testing.assert_allclose(sigma.cpu().numpy()[decided], g["sigma"][decided], rtol=3e-2, atol=3e-3)
    finally:
        handle.remove()
        field.fc_weight, field.light_visual_mode = 1.0, "Full"


# ---- 4. a frame ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lit", [False, True], ids=["static", "lit"])
def test_a_frame_of_the_imported_patch(dev, monkeypatch, lit):
    """32 x 32 through render_infer, render_infer_pipelined and render_infer_graphed behind initialize_states(): the same image bit for bit, not a
    trivial one, through the fused chain; another patch re-records the graphs and changes the image; switch_import() gives the mesh field's."""
    import nerftex_hip
    from ngp_harness import scene
    from ngp_harness.model import Renderer

    field = _field(dev, lit)
    field.fc_weight, field.fused_light_infer = (0.7, True) if lit else (1.0, False)
    frames = []
    for pose in scene.rand_poses(2, 1.6, np.random.default_rng(11)):
        o, d = scene.get_rays(pose, scene.intrinsics(32, 32), 32, 32)
        frames.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
    r_mesh = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        r_mesh.update_extra_state_device()
        mesh_ref = r_mesh.render_infer(*frames[0], slots_per_ray=4, **KW)[:2]
    mesh_stamp = field.graph_stamp()
    name = "nerftex_curved_light_patch_infer" if lit else "nerftex_curved_patch_infer"
    calls, entry = [], getattr(nerftex_hip.lib, name)
    monkeypatch.setattr(nerftex_hip.lib, name, lambda *a: (calls.append(1), entry(*a))[1])
    field.import_patch(**pm.seeded_patch(33, True, lit=lit))
    assert field.imported and field.imported_type == "patch" and field.graph_stamp() != mesh_stamp
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)  # (a grid of its own: initialize_states keeps a maximum)
    r.initialize_states(2)
    grid = r.density_grid[0]
    assert int((grid > 0).sum()) > 0 and int((grid == 0).sum()) > int((grid > 0).sum()), "the patch fills a thin slab of the box"
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            img, dep, _ = r.render_infer(*frames[0], slots_per_ray=4, **KW)
            assert bool(calls) == lit, "the reference loop: the lit field through its fused chain (infer_padded), the static field through forward()"
            img_p, dep_p, _ = r.render_infer_pipelined(*frames[0], slots_per_ray=4, parts=2, **KW)
            assert calls, "the device-count loops go through the fused chain"
            img_g, dep_g, _ = r.render_infer_graphed(*frames[0], slots_per_ray=4, parts=2, block=2, **KW)
            assert torch.equal(img_p, img) and torch.equal(dep_p, dep)
            assert torch.equal(img_g, img) and torch.equal(dep_g, dep)
            assert float(img.std()) > 1e-3 and not torch.equal(img, mesh_ref[0])
            graphs = r._infer_graphs
            img_2, dep_2, _ = r.render_infer_graphed(*frames[1], slots_per_ray=4, parts=2, block=2, **KW)
            assert r._infer_graphs is graphs, "another pose replays the recorded graphs"
            want_2 = r.render_infer(*frames[1], slots_per_ray=4, **KW)
            assert torch.equal(img_2, want_2[0]) and torch.equal(dep_2, want_2[1])
            other = pm.seeded_patch(33, True, lit=lit, seed=9)  # (the same points, other features)
            field.import_patch(**other)
            img_o, dep_o, _ = r.render_infer_graphed(*frames[0], slots_per_ray=4, parts=2, block=2, **KW)
            assert r._infer_graphs is not graphs, "another patch re-records the graphs"
            want = r.render_infer(*frames[0], slots_per_ray=4, **KW)
            assert torch.equal(img_o, want[0]) and torch.equal(dep_o, want[1]) and not torch.equal(img_o, img)
            field.switch_import()
            assert not field.imported and field.graph_stamp() == mesh_stamp
            n_calls = len(calls)
            img_m, dep_m, _ = r_mesh.render_infer(*frames[0], slots_per_ray=4, **KW)
            assert torch.equal(img_m, mesh_ref[0]) and torch.equal(dep_m, mesh_ref[1]) and len(calls) == n_calls
    finally:
        field.fused_light_infer = False


# ---- 5. export_field -> import_patch ------------------------------------------------------------------------------------------------------------------------------

def test_an_exported_patch_is_imported_and_read(dev, lit_field):
    """export_field on the small star-flower mesh, import_patch(result, 0): embed() at sample points above that patch is the float64 model over the
    exported arrays; the counter follows the reference's."""
    field = lit_field
    field._init_import_state()
    prob = pf64.patch_problem(8, False)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        result = field.export_field(prob["points"][:12], prob["normals"][:12], patch_size=8, pattern_rate=0.5, max_patch_num=4)
    P = result["patches"].shape[0]
    assert P >= 2 and result["patch_phi_embed"] is not None
    field.import_patch(result, 0)
    assert field.imported_type == "patch" and field.patch_id == 0 and field.features_imported.shape == (64, 16)
    pts = result["patch_coors"][0].reshape(-1, 3).astype(np.float32)
    nrm = np.ascontiguousarray(np.broadcast_to(result["patch_norms"][0].astype(np.float32), pts.shape))
    rng = np.random.default_rng(4)
    gap = float(np.linalg.norm(pts[1] - pts[0]))
    xn = (pts[rng.integers(0, 64, 256)] + nrm[0] * rng.uniform(-1.2, 1.2, (256, 1)) * field.h_threshold + rng.normal(0, 0.05 * gap, (256, 3))).astype(np.float32)
    x = torch.from_numpy(xn).to(dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        embed, normal, mask, fine = field.embed(x, with_fine_normal=True)
    idx = field._patch_neighbours(x)[0].cpu().numpy()
    pm.check_neighbours(pts, xn, idx)
    m = pm.resample(pts, nrm, result["patches"][0].reshape(-1, 16).astype(np.float32), xn, idx, field.h_threshold,
                    result["patch_phi_embed"][0].reshape(-1, 8).astype(np.float32), result["patch_local_tbn"][0].reshape(-1, 9).astype(np.float32))
    rows, decided = m["compare"], ~m["undecided"]
    assert rows.sum() > 50 and m["undecided"].mean() <= 0.02
    pm.assert_within(embed.double().cpu().numpy(), m["embed"], rows, "embed over the exported patch")
    assert np.array_equal(mask.cpu().numpy()[decided], m["mask"][decided]) and int(mask.sum()) > 20
    unit = torch.nn.functional.normalize(torch.from_numpy(m["normal"][0]).to(dev).float(), dim=-1)
    assert float((normal - unit).abs()[torch.from_numpy(rows).to(dev)].max()) < 1e-4
    assert float((fine.norm(dim=-1) - 1).abs()[mask].max()) < 1e-3
    field.import_patch(result)  # the counter: patch 0, then 1, ... modulo P
    assert field.patch_id == 1
    for k in range(1, P + 1):
        field.import_patch(result)
        assert field.patch_id == (k % P) + 1
    field.switch_import()


# ---- 6. a field that never imported ------------------------------------------------------------------------------------------------------------------------------

def test_a_field_that_never_imported_is_untouched(dev):
    field = _field(dev, False)
    stamp = field.graph_stamp()
    assert len(stamp) == 11 and not any(isinstance(s, str) for s in stamp)
    assert not field.imported and field._import_stamp() == () and field.imported_type is None and field._patch_knn is None and field.patch_id == 0
    rng = np.random.default_rng(5)
    v = field.projector.mesh_vertices.cpu().numpy()
    ids = 36 + np.arange(256) % (v.shape[0] - 72)
    x = torch.from_numpy((v[ids] * (1 + rng.uniform(-0.08, 0.08, (256, 1)))).astype(np.float32)).to(dev)
    d = _dirs(256, dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert field._infer_fused(x, d) and not field._infer_patch_fused(x, d) and not field._infer_light_patch_fused(x, d)
        assert field._infer_route(x, d)[0] == "nerftex_curved_field_infer"
        sigma, color, _ = field(x, d)
        got_s, got_c = field.infer(x, d)
    assert torch.equal(got_s, sigma.float()) and torch.equal(got_c, color.float()) and float(got_s.max()) > 0
    with pytest.raises(RuntimeError):
        field.import_shape(np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int64), np.zeros((3, 2), np.float32))
    with pytest.raises(RuntimeError):
        field.switch_import()
