"""GPU: an imported planar feature texture rendered through the curved field -- nerftex_planar_lookup against the framework's own expressions
(bit for bit where they are exact operations, inside the float64 bound of tests/planar_float64.py where they are sums), nerftex_curved_import_infer
against its pieces under the rows contract, CurvedField.import_field against the reference's fixture (tools/make_golden.py: import_field_goldens),
a frame through the three inference loops, and a field that never imported."""
import ctypes
import os

import numpy as np
import pytest
import torch

import planar_float64 as pf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.5
KW = dict(dt_gamma=0.0, max_steps=256)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _scalars(H, W, rescale, rate, offset):
    """nerftex_planar_lookup's (mode, plane scales, height scales, offset, threshold) for a case of planar_float64.case_points."""
    from nerftex_hip import PLANAR_DIVIDE, PLANAR_MULTIPLY

    b0, b1 = pf.map_bounds(H, W)
    return (PLANAR_MULTIPLY, rate, rate, b0, rate, offset, pf.H_THRESHOLD) if rescale else (PLANAR_DIVIDE, b0, b1, 1.0, 1.0, offset, pf.H_THRESHOLD)


def _lookup(x, fmap, scalars):
    from nerftex_hip import check, lib, ptr, stream

    n, dev = x.shape[0], x.device
    p_uv, sdf = torch.full((n, 2), SENTINEL, device=dev), torch.full((n,), SENTINEL, device=dev)
    mask = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    xin = torch.full((n, 48), SENTINEL, dtype=torch.float16, device=dev)
    check(lib.nerftex_planar_lookup(ptr(x), ptr(fmap), fmap.shape[0], fmap.shape[1], *scalars, 12, n, ptr(p_uv), ptr(sdf), ptr(mask), ptr(xin), stream()))
    return p_uv, sdf, mask, xin


# ---- 1. the plain entry -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", pf.MAPS)
@pytest.mark.parametrize("rescale", [True, False], ids=["modeA", "modeB"])
def test_plain_lookup_against_the_framework_and_float64(dev, H, W, rescale):
    """p_uv, sdf and mask equal the framework's expressions on the same device bit for bit; features and ladder are inside the float64 bound on
    every element, and so is the framework's own grid_sample."""
    F = pf.seeded_map(H, W)
    fmap = torch.from_numpy(F).to(dev)
    worst = worst_torch = 0.0
    masked_in = masked_out = 0
    for rate in (1.0, 0.5, 1.7):
        for offset in (0.0, 0.01):
            for B in (1, 127, 128, 129, 384):
                x = torch.from_numpy(pf.case_points(H, W, B, rescale, rate, offset)).to(dev)
                p_uv, sdf, mask, xin = _lookup(x, fmap, _scalars(H, W, rescale, rate, offset))
                w_uv, w_sdf, w_mask, w_embed = pf.torch_expressions(x, fmap, pf.map_bounds(H, W), rescale, rate, offset, pf.H_THRESHOLD)
                assert torch.equal(p_uv, w_uv) and torch.equal(sdf, w_sdf), (B, rate, offset)
                assert torch.equal(mask, w_mask.to(torch.uint8)), (B, rate, offset)
                assert bool((xin[:, 41:] == 1).all())
                value, bound = pf.lookup_reference(F, p_uv[:, 0].cpu().numpy(), p_uv[:, 1].cpu().numpy(), sdf.cpu().numpy())
                ratio = np.abs(xin[:, :41].double().cpu().numpy() - value) / bound
                worst = max(worst, float(ratio.max()))
                ratio_t = np.abs(w_embed.half().double().cpu().numpy() - value[:, :16]) / bound[:, :16]
                worst_torch = max(worst_torch, float(ratio_t.max()))
                masked_in, masked_out = masked_in + int(mask.sum()), masked_out + int((mask == 0).sum())
    print(f"map {H}x{W} {'A' if rescale else 'B'}: largest error / bound -- kernel {worst:.3f}, the framework's grid_sample {worst_torch:.3f}; "
          f"{masked_in} rows inside the mask, {masked_out} outside")
    assert worst <= 1.0 and worst_torch <= 1.0
    assert masked_in > 0 and masked_out > 0


def test_the_threshold_and_the_plane_edges(dev):
    """|sdf| exactly h_threshold is outside (strict); u, v = +-1 exactly are inside (inclusive), one fp32 step outwards is outside -- and still
    interpolates towards the padding zeros."""
    H, W = 5, 4
    F = pf.seeded_map(H, W)
    fmap = torch.from_numpy(F).to(dev)
    one, h = np.float32(1), np.float32(pf.H_THRESHOLD)
    up, below = np.nextafter(one, np.float32(2)), np.nextafter(h, np.float32(0))
    rows = np.float32([[1, 1, 0], [-1, -1, 0], [up, 0, 0], [0, -up, 0], [0, 0, h / 0.5], [0, 0, -h / 0.5], [0, 0, below / 0.5], [1, -1, 0]])
    p_uv, sdf, mask, xin = _lookup(torch.from_numpy(rows).to(dev), fmap, _scalars(H, W, True, 1.0, 0.0))
    assert mask.tolist() == [1, 1, 0, 0, 0, 0, 1, 1]
    assert float(sdf[4]) == pf.H_THRESHOLD and float(sdf[5]) == -pf.H_THRESHOLD
    got = xin[:, :16].float().cpu().numpy()
    assert np.array_equal(got[0], F[H - 1, W - 1].astype(np.float16).astype(np.float32)), "u runs along the first axis: (1, 1) is features[H-1, W-1]"
    assert np.array_equal(got[1], F[0, 0].astype(np.float16).astype(np.float32)) and np.array_equal(got[7], F[H - 1, 0].astype(np.float16).astype(np.float32))
    rows_b = np.float32([[0.5, 0.4, 0], [0, 0, h], [0, 0, below]])  # mode B: bounds (0.5, 0.4), sdf = z
    _, sdf_b, mask_b, xin_b = _lookup(torch.from_numpy(rows_b).to(dev), fmap, _scalars(H, W, False, 1.0, 0.0))
    assert mask_b.tolist() == [1, 0, 1] and float(sdf_b[1]) == pf.H_THRESHOLD
    assert np.array_equal(xin_b[0, :16].float().cpu().numpy(), F[H - 1, W - 1].astype(np.float16).astype(np.float32))


# ---- 2. the chain against its pieces -------------------------------------------------------------------------------------------------------------------------

def _half_weights(n, seed, scale, dev):
    w = torch.from_numpy(np.random.default_rng(seed).uniform(-scale, scale, n).astype(np.float16))
    return w.to(dev)


def _pieces(x, d, fmap, scalars, ws, wc, eval_bits):
    """nerftex_planar_lookup, nerftex_ffmlp_inference, nerftex_curved_mid_forward, nerftex_ffmlp_inference, nerftex_curved_out_forward one after
    the other: -> sigma [B] fp32, rgbs [B,3] fp32 (the half outputs widened)."""
    from nerftex_hip import check, lib, ptr, stream

    n, dev = x.shape[0], x.device
    _, _, mask, xin = _lookup(x, fmap, scalars)
    h = torch.empty(n, 16, dtype=torch.float16, device=dev)
    buf = torch.empty(n, 64, dtype=torch.float16, device=dev)
    check(lib.nerftex_ffmlp_inference(ptr(xin), ptr(ws), n, 48, 16, 32, 2, 0, 6, ptr(buf), ptr(h), stream()))
    normal = torch.zeros(n, 3, device=dev)
    normal[:, 2] = 1.0
    sigma_raw, cin = torch.empty(n, dtype=torch.float16, device=dev), torch.empty(n, 32, dtype=torch.float16, device=dev)
    check(lib.nerftex_curved_mid_forward(ptr(h), ptr(normal), ptr(d), n, 1.0, eval_bits, ptr(sigma_raw), ptr(cin), stream()))
    hc = torch.empty(n, 16, dtype=torch.float16, device=dev)
    check(lib.nerftex_ffmlp_inference(ptr(cin), ptr(wc), n, 32, 16, 64, 3, 0, 6, ptr(buf), ptr(hc), stream()))
    sigma, color = torch.empty(n, dtype=torch.float16, device=dev), torch.empty(n, 3, dtype=torch.float16, device=dev)
    check(lib.nerftex_curved_out_forward(ptr(hc), 16, ptr(sigma_raw), ptr(mask), n, ptr(sigma), ptr(color), stream()))
    return sigma.float(), color.float()


@pytest.mark.parametrize("H,W", pf.MAPS)
@pytest.mark.parametrize("rescale", [True, False], ids=["modeA", "modeB"])
def test_chain_is_its_pieces_under_the_rows_contract(dev, H, W, rescale):
    from nerftex_hip import CurvedImportInferDesc, check, lib, ptr, stream

    fmap = torch.from_numpy(pf.seeded_map(H, W)).to(dev)
    ws, wc = _half_weights(3072, 3, 0.6, dev), _half_weights(11264, 4, 0.25, dev)
    for B in (128, 384):
        for rate, offset in ((1.0, 0.0), (1.7, 0.01)):
            scalars = _scalars(H, W, rescale, rate, offset)
            x = torch.from_numpy(pf.case_points(H, W, B, rescale, rate, offset)).to(dev)
            rng = np.random.default_rng(B)
            d = rng.normal(size=(B, 3)).astype(np.float32)
            d = torch.from_numpy(d / np.linalg.norm(d, axis=-1, keepdims=True)).to(dev)
            want_sigma, want_rgb = _pieces(x, d, fmap, scalars, ws, wc, 3)
            assert float(want_sigma.max()) > 0 and float(want_rgb.max()) > 0  # (not a comparison of zeros)
            marked = torch.zeros(B, dtype=torch.bool, device=dev)
            marked[::7] = True
            marked[32:64] = True
            xm, dm = x.clone(), d.clone()
            xm[marked] = 1e30
            dm[marked, 0] = 1e30
            scratch = torch.empty(lib.nerftex_curved_import_infer_scratch_bytes(B), dtype=torch.uint8, device=dev)
            for units, rows_per_unit, live in ((0, 128, 0), (1, 128, 128), (None, 0, B), (B // 64, 64, B)):
                units_dev = None if units is None else torch.tensor([units], dtype=torch.int32, device=dev)
                sigma = torch.full((B,), SENTINEL, dtype=torch.float32, device=dev)
                rgbs = torch.full((B, 3), SENTINEL, dtype=torch.float32, device=dev)
                mode, p0, p1, h0, h1, off, h = scalars
                desc = CurvedImportInferDesc(
                    xyz=ptr(xm), dirs=ptr(dm), B=B, map=ptr(fmap), map_h=H, map_w=W, n_features=16, mode=mode, plane_scale0=p0, plane_scale1=p1, height_scale0=h0,
                    height_scale1=h1, sdf_offset=off, h_threshold=h, n_freqs=12, sigma_weights=ptr(ws), sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16,
                    color_weights=ptr(wc), color_in=32, color_hidden=64, color_layers=3, color_out=3, fc_weight=1.0, eval=3, sigma=ptr(sigma), rgbs=ptr(rgbs),
                    units_dev=ptr(units_dev), rows_per_unit=rows_per_unit, scratch=ptr(scratch), scratch_bytes=scratch.numel())
                check(lib.nerftex_curved_import_infer(ctypes.byref(desc), stream()))
                torch.cuda.synchronize()
                rows = torch.arange(B, device=dev)
                plain, unused, past = (rows < live) & ~marked, (rows < live) & marked, rows >= live
                assert torch.equal(sigma[plain], want_sigma[plain]) and torch.equal(rgbs[plain], want_rgb[plain]), (B, rate, units)
                assert bool((sigma[unused] == 0).all()) and bool((rgbs[unused] == 0).all())
                assert bool((sigma[past] == SENTINEL).all()) and bool((rgbs[past] == SENTINEL).all())


# ---- 3. the field on the reference's fixture -----------------------------------------------------------------------------------------------------------------

def _field(dev, h_threshold=0.0625):
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=h_threshold).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
    return field.eval()


@pytest.fixture(scope="module")
def golden_field(dev):
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_python_import_field.npz"))
    c = np.load(os.path.join(ROOT, "tests", "golden", "ref_python_curvedfield.npz"))
    field = _field(dev, float(g["h_threshold"]))
    with torch.no_grad():
        field.sigma_net.weights.copy_(torch.from_numpy(c["w_sigma"]))
        field.color_net.weights.copy_(torch.from_numpy(c["w_color"]))
    return field, g


@pytest.mark.parametrize("key", ["A0", "A1", "B0", "B1"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_by_op"])
def test_the_field_reproduces_the_reference_fixture(dev, golden_field, key, fused):
    field, g = golden_field
    field._init_import_state()
    field.import_field(g["features"], float(g["grid_gap"]))
    if key[0] == "B":
        field.import_field(torch.from_numpy(g["features"]), float(g["grid_gap"]))
    assert field.rescale == (key[0] == "A")
    field.set_uv_utilize_rate(float(g[key + "_rate"]))
    field.set_sdf_offset(float(g[key + "_offset"]))
    x, d = torch.from_numpy(g["xyz"]).to(dev), torch.from_numpy(g["dirs"]).to(dev)
    field.fused_glue = fused
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._import_fused(x) == fused
            embed, normal, mask = field.embed(x)
            sigma, color, _ = field(x, d)
            dens = field.density(x)
            got_s, got_c = field.infer(x, d)
            assert field._infer_import_fused(x, d) == fused
    finally:
        field.fused_glue = True
    want_mask = torch.from_numpy(g[key + "_h_mask"]).to(dev)
    assert torch.equal(mask, want_mask)
    assert torch.equal(normal, torch.tensor([0.0, 0.0, 1.0], device=dev).expand(512, 3) / (1 + 1e-5))
    if key + "_embed" in g:
        want = torch.from_numpy(g[key + "_embed"]).to(dev)
        e_feat, e_z = float((embed[:, :16].float() - want[:, :16]).abs().max()), float((embed[:, 16:].float() - want[:, 16:]).abs().max())
        print(f"{key} {'fused' if fused else 'op by op'}: embedding error, features {e_feat:.3e} (bar 1e-3), ladder {e_z:.3e} (bar 2e-3)")
        assert e_feat <= 1e-3 and e_z <= 2e-3
    want_s, want_c = torch.from_numpy(g[key + "_sigma"]).to(dev), torch.from_numpy(g[key + "_color"]).to(dev).float()
    print(f"{key} {'fused' if fused else 'op by op'}: sigma error {float((sigma.float() - want_s).abs().max()):.3e}, colour error "
          f"{float((color.float() - want_c).abs().max()):.3e}; {int(want_mask.sum())} rows inside the mask")
    assert torch.equal(sigma == 0, ~want_mask) and torch.equal((color == 0).all(-1), ~want_mask)
    torch.testing.assert_close(sigma.float(), want_s, rtol=3e-2, atol=3e-3)
    torch.testing.assert_close(color.float(), want_c, rtol=0, atol=2e-2)
    torch.testing.assert_close(dens["sigma"].float(), want_s, rtol=3e-2, atol=3e-3)
    assert got_s.dtype == torch.float32 and torch.equal(got_s, sigma.float()) and torch.equal(got_c, color.float())


def test_infer_marks_and_live_rows_on_the_field(dev, golden_field):
    field, g = golden_field
    field._init_import_state()
    field.import_field(g["features"], float(g["grid_gap"]))
    x, d = torch.from_numpy(g["xyz"]).to(dev), torch.from_numpy(g["dirs"]).to(dev)
    marked = torch.zeros(512, dtype=torch.bool, device=dev)
    marked[::5] = True
    xm, dm = x.clone(), d.clone()
    xm[marked] = 1e30
    dm[marked, 0] = 1e30
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        sigma, color, _ = field(x, d)
        got_s, got_c = field.infer(xm, dm, (torch.tensor([3], dtype=torch.int32, device=dev), 128))
    rows = torch.arange(512, device=dev)
    plain, unused = (rows < 384) & ~marked, (rows < 384) & marked
    assert torch.equal(got_s[plain], sigma.float()[plain]) and torch.equal(got_c[plain], color.float()[plain]) and float(got_s[plain].max()) > 0
    assert bool((got_s[unused] == 0).all()) and bool((got_c[unused] == 0).all())


# ---- 4. a frame ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frame_setup(dev):
    """A mesh field behind a Renderer and its frame through the reference loop; a second Renderer, its grid still empty, for the map to import."""
    from ngp_harness import scene
    from ngp_harness.model import Renderer

    field = _field(dev)
    with torch.no_grad():
        field.sigma_net.weights.mul_(3.0)
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        r.update_extra_state_device()
    frames = []
    for pose in scene.rand_poses(2, 1.6, np.random.default_rng(11)):
        o, d = scene.get_rays(pose, scene.intrinsics(32, 32), 32, 32)
        frames.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
    stamp = field.graph_stamp()
    with torch.autocast("cuda", dtype=torch.float16):
        mesh_ref = r.render_infer(*frames[0], slots_per_ray=4, **KW)[:2]
        mesh_graphed = r.render_infer_graphed(*frames[0], slots_per_ray=4, parts=2, block=2, **KW)[:2]
    # the imported map gets a renderer of its own over the same field: initialize_states() keeps the larger of the old and the new density
    # (decay 1, a maximum: nerf/renderer.py:644), so "empty outside the slab" is a statement about a grid that starts empty
    r_import = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    return dict(field=field, r=r_import, r_mesh=r, frames=frames, mesh_ref=mesh_ref, mesh_graphed=mesh_graphed, mesh_stamp=stamp)


def test_a_frame_of_the_imported_map(dev, frame_setup):
    import raymarching

    field, r, frames = (frame_setup[k] for k in ("field", "r", "frames"))
    H = r.grid_size
    assert r.cascade == 1
    field.import_field(pf.seeded_map(64, 64, seed=21), 1.0 / 64)  # bounds (0.5, 0.5); rescale: u, v = x, y and sdf = z / 2
    assert field.rescale and field.h_threshold == 0.0625
    r.initialize_states(2)
    # occupancy: cell centres from the Morton index, the slab |x|, |y| <= 1, |z| / 2 < h
    coords = raymarching.morton3D_invert(torch.arange(H ** 3, dtype=torch.int32, device=dev)).float()
    half_cell = 1.0 / H
    centres = (2 * coords / (H - 1) - 1) * (1.0 - half_cell)
    cell = 2.0 / H
    dist_z = (centres[:, 2].abs() - 2 * field.h_threshold)  # > 0: outside the slab along z (x and y fill the whole box)
    grid = r.density_grid[0]
    far, inside = dist_z > 1.5 * cell, dist_z < -1.0 * cell
    assert int(far.sum()) > 0 and int(inside.sum()) > 0
    assert bool((grid[far] == 0).all()), "cells farther than one cell from the slab are exactly empty"
    assert bool((grid[inside] > 0).all()), "cells inside the slab are occupied"
    with torch.autocast("cuda", dtype=torch.float16):
        img_ref, dep_ref, _ = r.render_infer(*frames[0], slots_per_ray=4, **KW)
        img_g, dep_g, _ = r.render_infer_graphed(*frames[0], slots_per_ray=4, parts=2, block=2, **KW)
        assert torch.equal(img_g, img_ref) and torch.equal(dep_g, dep_ref)
        assert float(img_ref.std()) > 1e-3 and not torch.equal(img_ref, frame_setup["mesh_ref"][0])
        for k in (0, 1):
            want = r.render_infer(*frames[k], slots_per_ray=4, **KW)
            img_p, dep_p, _ = r.render_infer_pipelined(*frames[k], slots_per_ray=4, parts=2, **KW)
            assert torch.equal(img_p, want[0]) and torch.equal(dep_p, want[1]), k
        graphs = r._infer_graphs
        img_2, dep_2, _ = r.render_infer_graphed(*frames[1], slots_per_ray=4, parts=2, block=2, **KW)
        assert r._infer_graphs is graphs, "another pose replays the recorded graphs"
        field.set_sdf_offset(0.02)
        img_o, dep_o, _ = r.render_infer_graphed(*frames[0], slots_per_ray=4, parts=2, block=2, **KW)
        assert r._infer_graphs is not graphs, "a changed offset re-records the graphs"
        want = r.render_infer(*frames[0], slots_per_ray=4, **KW)
        assert torch.equal(img_o, want[0]) and torch.equal(dep_o, want[1]) and not torch.equal(img_o, img_ref)
        # back to the mesh field (behind the renderer that holds the mesh's occupancy grid): its frame bit for bit
        field.switch_import()
        assert not field.imported and field.graph_stamp() == frame_setup["mesh_stamp"]
        r = frame_setup["r_mesh"]
        img_m, dep_m, _ = r.render_infer_graphed(*frames[0], slots_per_ray=4, parts=2, block=2, **KW)
        assert torch.equal(img_m, frame_setup["mesh_ref"][0]) and torch.equal(dep_m, frame_setup["mesh_ref"][1])
        img_m, dep_m, _ = r.render_infer(*frames[0], slots_per_ray=4, **KW)
        assert torch.equal(img_m, frame_setup["mesh_ref"][0]) and torch.equal(dep_m, frame_setup["mesh_ref"][1])


# ---- 5. a field that never imported ----------------------------------------------------------------------------------------------------------------------------

def test_a_field_that_never_imported_is_untouched(dev, frame_setup):
    """The stamp carries nothing new (eleven entries, as before this feature), infer() is forward() bit for bit through the mesh chain, and the
    graphed frame is the reference loop's (frame_setup rendered both before anything was imported)."""
    field = _field(dev)
    stamp = field.graph_stamp()
    assert len(stamp) == 11 and not any(isinstance(s, str) for s in stamp) and len(frame_setup["mesh_stamp"]) == 11
    assert not field.imported and field._import_stamp() == ()
    rng = np.random.default_rng(5)
    v = field.projector.mesh_vertices.cpu().numpy()
    ids = 36 + np.arange(256) % (v.shape[0] - 72)
    x = torch.from_numpy((v[ids] * (1 + rng.uniform(-0.08, 0.08, (256, 1)))).astype(np.float32)).to(dev)
    d = rng.normal(size=(256, 3)).astype(np.float32)
    d = torch.from_numpy(d / np.linalg.norm(d, axis=-1, keepdims=True)).to(dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert field._infer_fused(x, d)
        sigma, color, _ = field(x, d)
        got_s, got_c = field.infer(x, d)
    assert torch.equal(got_s, sigma.float()) and torch.equal(got_c, color.float()) and float(got_s.max()) > 0
    assert torch.equal(frame_setup["mesh_graphed"][0], frame_setup["mesh_ref"][0]) and torch.equal(frame_setup["mesh_graphed"][1], frame_setup["mesh_ref"][1])
    assert float(frame_setup["mesh_ref"][0].std()) > 1e-3
