"""GPU: an imported feature map rendered on a new UV-mapped mesh through the curved field -- nerftex_shape_lookup against the float64
statement of tests/shape_float64.py and against the op-by-op route, nerftex_curved_shape_infer against its pieces under the rows contract,
CurvedField.import_shape against the reference's fixture (tools/make_golden.py: import_shape_goldens), and a frame through the three
inference loops."""
import ctypes
import os

import numpy as np
import pytest
import torch

import planar_float64 as pf
import shape_float64 as sf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.5
NERFTEX_ERR_INVALID = 1
KW = dict(dt_gamma=0.0, max_steps=256)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def trace32(oracle):
    return lambda v, f, o, d: oracle.raytrace(v, f, o, d)[:4]


class Mesh:
    """the device structures of one of shape_float64's meshes: raytracer, neighbour grid, vertex arrays, face_uv"""
    _made = {}

    def __init__(self, name, dev):
        from ngp_harness.curved import MeshProjector

        self.v, self.f, self.vn, self.uvs = sf.mesh_of(name)
        self.proj = MeshProjector(self.v, self.f, vertex_normals=self.vn).to(dev)
        face_uv = self.uvs[self.f.astype(np.int64)].reshape(-1, 6)
        if len(face_uv) <= 8:  # (the RayTracer wrapper pads the BVH of so small a mesh with 8 far-away faces; CurvedField.import_shape pads the table likewise)
            face_uv = np.concatenate([face_uv, np.zeros((8, 6), np.float32)], 0)
        self.face_uv = torch.from_numpy(np.ascontiguousarray(face_uv)).to(dev)

    @classmethod
    def of(cls, name, dev):
        if name not in cls._made:
            cls._made[name] = cls(name, dev)
        return cls._made[name]


def _lookup(mesh, x, idx, dis, fmap, scale, offset, rate, h, n_faces=None, K=None, n_freqs=12, expect=0):
    from nerftex_hip import lib, ptr, stream

    n, dev, p = x.shape[0], x.device, mesh.proj
    p_uv, sdf = torch.full((n, 2), SENTINEL, device=dev), torch.full((n,), SENTINEL, device=dev)
    mask = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    normal = torch.full((n, 3), SENTINEL, device=dev)
    face = torch.full((n,), -9, dtype=torch.int64, device=dev)
    xin = torch.full((n, 48), SENTINEL, dtype=torch.float16, device=dev)
    rc = lib.nerftex_shape_lookup(p.tracer._handle, ptr(x), ptr(idx), ptr(dis), n, idx.shape[1] if K is None else K, ptr(p.mesh_vertices), ptr(p.vertex_normals),
                                  p.mesh_vertices.shape[0], ptr(mesh.face_uv), mesh.face_uv.shape[0] if n_faces is None else n_faces, ptr(fmap), fmap.shape[0],
                                  fmap.shape[1], scale, offset, rate, h, n_freqs, ptr(p_uv), ptr(sdf), ptr(mask), ptr(normal), ptr(face), ptr(xin), stream())
    assert rc == expect, lib.nerftex_last_error().decode()
    return p_uv, sdf, mask, normal, face, xin


def _case(name, dev, trace32):
    P = sf.problem(name, device=dev)
    if "tol_t" not in P:
        R = P["rays"]
        sf.set_tolerances(P, trace32(R["v"], R["f"], R["o"], R["d"]))
    return P


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- 1. the plain entry against float64 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sf.CASES))
def test_plain_entry_passes_the_float64_check(dev, trace32, name):
    """Every case of shape_float64 (the quad, the height field, the star mesh; K 2..16 and K clamped to 4 vertices; maps 1x1, 5x4, 64x48; rate 1,
    0.5, 1.3; scale 1, 2.5; offset 0, 0.01; row 0 exactly on a vertex), whole and at batch sizes around the 32-point wave."""
    P = _case(name, dev, trace32)
    mesh = Mesh.of(sf.CASES[name][0], dev)
    fmap = _t(P["features"], dev)
    for N in (P["x"].shape[0], 1, 127, 128, 129, 384):
        Q = P if N == P["x"].shape[0] else sf.head(P, N)
        out = _lookup(mesh, _t(Q["x"], dev), _t(Q["idx"], dev), _t(Q["dis"], dev), fmap, P["scale"], P["offset"], P["rate"], P["h_threshold"])
        r = sf.check(Q, *(o.cpu().numpy() for o in out))
        if N == P["x"].shape[0]:
            print(f"{name}: kernel ratios " + " ".join(f"{k} {v:.3f}" for k, v in r.items()), sf.describe(P))
    assert not bool(out[2][0]) and int(out[4][0]) == -1, "the query on a vertex has no normal: mask 0"


def test_the_wrapper_clamps_k_to_the_vertices_and_searches_itself(dev):
    """CurvedField._shape_scalars clamps K_for_uv = 8 to the quad's 4 vertices; the library's own neighbour search feeds the kernel."""
    mesh = Mesh.of("quad", dev)
    x = _t(sf.sample_points(mesh.v, mesh.f, mesh.vn, 129, np.random.default_rng(3)), dev)
    idx, dis = mesh.proj.knn(x, 8)
    assert idx.shape == (129, 4)
    p_uv, sdf, mask, normal, face, xin = _lookup(mesh, x, idx, dis, _t(pf.seeded_map(5, 4), dev), 1.0, 0.0, 1.0, 0.05)
    assert int(mask.sum()) > 10 and bool((face[mask.bool()] >= 0).all()) and bool((normal[mask.bool()][:, 2].abs() > 0.99).all())
    # the same through the field: K_for_uv = 5 over 4 vertices, the UV table padded to the padded BVH's face count
    field = _shape_field(dev, "quad", (5, 4))
    assert field.K_for_uv == 5 and field._shape_scalars()[0] == 4 and field.shape_face_uv.shape == (10, 6)
    field.set_sdf_factor(1.0)
    got = field._shape_lookup(x)
    # (import_shape maps the UVs to [-1, 1] once more, an ulp here and there: u, v and the features are compared to that)
    assert torch.equal(got[1], sdf) and torch.equal(got[2], mask.bool()) and torch.equal(got[3], normal) and torch.equal(got[4], face)
    assert float((got[0] - p_uv).abs().max()) <= 4 * 2.0 ** -24


# ---- 2. the plain entry against the op-by-op route --------------------------------------------------------------------------------------------------------

def _shape_field(dev, mesh_name="height", map_hw=(64, 48), h_threshold=0.05):
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=h_threshold).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
    field.import_field(pf.seeded_map(*map_hw), 1.0 / map_hw[0])
    mv, mf, mvn, muv = sf.mesh_of(mesh_name)
    field.import_shape(mv, mf, muv, vertex_normals=mvn, normalize=False)
    return field.eval()


@pytest.mark.parametrize("name", ["height_k5", "height_scaled", "star_k8"])
def test_plain_entry_against_the_op_by_op_route(dev, trace32, name):
    """Which outputs are bit-reproducible: on the rows where the framework's normal has the kernel's bits, sdf, mask and face are the route's bit
    for bit (the same tracer on the same ray, a true division, an exact subtraction).  p_uv is not (the framework's cross product and norm
    kernels contract and sum in their own order): both routes are inside the float64 bar, so they differ by at most twice that bar.  The
    op-by-op route passes the float64 check itself."""
    mesh_name, N, K, h, scale, offset, rate, _, map_hw = sf.CASES[name]
    field = _shape_field(dev, mesh_name, map_hw, h)
    field.set_k_for_uv(K), field.set_sdf_factor(scale * rate), field.set_uv_utilize_rate(rate), field.set_sdf_offset(offset)
    P0 = _case(name, dev, trace32)
    # the field's UV table (import_shape maps the UVs once more: an ulp here and there), so the statement is rebuilt over it
    mesh = (P0["v"], P0["f"], P0["vn"], field.shape_uvs.cpu().numpy())
    P = sf.build_problem(name + " on the field", mesh, P0["x"], K, h, float(field.sdf_scale_factor) / float(field.uv_utilize_rate), offset, rate, map_hw,
                         device=dev, neighbours=(P0["idx"], P0["dis"]))
    R = P["rays"]
    sf.set_tolerances(P, trace32(R["v"], R["f"], R["o"], R["d"]))
    assert field._shape_scalars()[1] == P["scale"]
    x, nb = _t(P["x"], dev), (_t(P["idx"], dev), _t(P["dis"], dev))
    with torch.no_grad():
        p_uv, sdf, mask, normal, face, xin = field._shape_lookup(x, neighbours=nb)
        embed, _, w_mask, w_uv, w_sdf, w_normal, w_face = field._shape_embed_reference(x, neighbours=nb, details=True)
    sf.check(P, *(o.cpu().numpy() for o in (p_uv, sdf, mask, normal, face, xin)))
    nan = _t(P["nan"], dev)
    assert bool(torch.isnan(w_normal[nan]).all()) and not bool(w_mask[nan].any()), "the reference's 0 / 0 rows: NaN and a miss"
    zero = lambda t, fill=0: torch.where(nan.view(-1, *[1] * (t.dim() - 1)), torch.full_like(t, fill), t)  # noqa: E731
    xin_w = torch.cat([embed.half(), torch.ones(len(x), 7, dtype=torch.float16, device=dev)], -1)
    xin_w[nan, :41] = 0
    r = sf.check(P, *(o.cpu().numpy() for o in (zero(w_uv), zero(w_sdf), w_mask, zero(w_normal), zero(w_face, -1), xin_w)))
    same = (normal == w_normal).all(-1) & ~nan
    print(f"{name}: op-by-op ratios " + " ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"; the framework's normal has the kernel's bits on {float(same.float().mean()):.3f} of the rows, "
          f"p_uv bits on {float((p_uv == w_uv).all(-1)[same].float().mean()):.3f} of those")
    assert torch.equal(sdf[same], w_sdf[same]) and torch.equal(mask.bool()[same], w_mask[same]) and torch.equal(face[same], w_face[same])
    u = _t(P["decided"] & P["unique"] & ~P["far"], dev)
    assert bool(((p_uv - w_uv).abs() <= 2 * _t(P["tol_uv"], dev))[u].all())


# ---- 3. the chain against its pieces -----------------------------------------------------------------------------------------------------------------------

def _half_weights(n, seed, scale, dev):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-scale, scale, n).astype(np.float16)).to(dev)


def _pieces(mesh, x, d, K, fmap, scalars, ws, wc, eval_bits):
    """nerftex_knn_query, nerftex_shape_lookup, nerftex_ffmlp_inference, nerftex_curved_mid_forward, nerftex_ffmlp_inference,
    nerftex_curved_out_forward one after the other: -> sigma [B] fp32, rgbs [B,3] fp32, mask, whether the row has a normal"""
    from nerftex_hip import check, lib, ptr, stream

    n, dev = x.shape[0], x.device
    idx, dis = mesh.proj.knn(x, K)
    _, _, mask, normal, face, xin = _lookup(mesh, x, idx, dis, fmap, *scalars)
    h = torch.empty(n, 16, dtype=torch.float16, device=dev)
    buf = torch.empty(n, 64, dtype=torch.float16, device=dev)
    check(lib.nerftex_ffmlp_inference(ptr(xin), ptr(ws), n, 48, 16, 32, 2, 0, 6, ptr(buf), ptr(h), stream()))
    sigma_raw, cin = torch.empty(n, dtype=torch.float16, device=dev), torch.empty(n, 32, dtype=torch.float16, device=dev)
    check(lib.nerftex_curved_mid_forward(ptr(h), ptr(normal), ptr(d), n, 1.0, eval_bits, ptr(sigma_raw), ptr(cin), stream()))
    hc = torch.empty(n, 16, dtype=torch.float16, device=dev)
    check(lib.nerftex_ffmlp_inference(ptr(cin), ptr(wc), n, 32, 16, 64, 3, 0, 6, ptr(buf), ptr(hc), stream()))
    sigma, color = torch.empty(n, dtype=torch.float16, device=dev), torch.empty(n, 3, dtype=torch.float16, device=dev)
    check(lib.nerftex_curved_out_forward(ptr(hc), 16, ptr(sigma_raw), ptr(mask), n, ptr(sigma), ptr(color), stream()))
    return sigma.float(), color.float(), mask.bool(), (normal != 0).any(-1)


@pytest.mark.parametrize("mesh_name,K,map_hw,scalars", [("quad", 4, (5, 4), (1.0, 0.0, 1.0, 0.05)), ("height", 5, (64, 48), (2.5, 0.01, 0.5, 0.05)),
                                                       ("star", 2, (1, 1), (1.0, 0.0, 1.3, 0.05)), ("star", 16, (64, 48), (2.5, 0.0, 1.0, 20.0))])
def test_chain_is_its_pieces_under_the_rows_contract(dev, mesh_name, K, map_hw, scalars):
    from nerftex_hip import CurvedShapeInferDesc, check, lib, ptr, stream

    mesh = Mesh.of(mesh_name, dev)
    p = mesh.proj
    fmap = _t(pf.seeded_map(*map_hw), dev)
    ws, wc = _half_weights(3072, 3, 0.6, dev), _half_weights(11264, 4, 0.25, dev)
    for B in (128, 384):
        rng = np.random.default_rng(B + K)
        x = _t(sf.sample_points(mesh.v, mesh.f, mesh.vn, B, rng, on_vertex=True), dev)
        d = rng.normal(size=(B, 3)).astype(np.float32)
        d = _t(d / np.linalg.norm(d, axis=-1, keepdims=True), dev)
        want_sigma, want_rgb, want_mask, has_normal = _pieces(mesh, x, d, K, fmap, scalars, ws, wc, 3)
        assert float(want_sigma.max()) > 0 and float(want_rgb.max()) > 0  # (not a comparison of zeros)
        assert not bool(has_normal[0]) and float(want_sigma[0]) == 0 and not bool(want_rgb[0].any()), "the row on a vertex: mask 0, sigma 0, colour 0"
        if mesh_name == "star" and K == 2:
            assert int((~has_normal).sum()) > 1, "the duplicated pole vertices tie both kept distances"
        assert bool((want_sigma[~has_normal] == 0).all()) and bool((want_rgb[~has_normal] == 0).all())
        marked = torch.zeros(B, dtype=torch.bool, device=dev)
        marked[::7] = True
        marked[32:64] = True
        marked[0] = False
        xm, dm = x.clone(), d.clone()
        xm[marked] = 1e30
        dm[marked, 0] = 1e30
        scratch = torch.empty(lib.nerftex_curved_shape_infer_scratch_bytes(B), dtype=torch.uint8, device=dev)
        for units, rows_per_unit, live in ((0, 128, 0), (1, 128, 128), (None, 0, B), (B // 64, 64, B)):
            units_dev = None if units is None else torch.tensor([units], dtype=torch.int32, device=dev)
            sigma = torch.full((B,), SENTINEL, dtype=torch.float32, device=dev)
            rgbs = torch.full((B, 3), SENTINEL, dtype=torch.float32, device=dev)
            scale, off, rate, h = scalars
            desc = CurvedShapeInferDesc(
                knn=p._knn.value, tracer=p.tracer._handle.value, xyz=ptr(xm), dirs=ptr(dm), B=B, n_verts=p.mesh_vertices.shape[0], mesh_vertices=ptr(p.mesh_vertices),
                vertex_normals=ptr(p.vertex_normals), face_uv=ptr(mesh.face_uv), n_faces=mesh.face_uv.shape[0], K=K, map=ptr(fmap), map_h=map_hw[0], map_w=map_hw[1],
                n_features=16, sdf_scale=scale, sdf_offset=off, uv_rate=rate, h_threshold=h, n_freqs=12, sigma_weights=ptr(ws), sigma_in=48, sigma_hidden=32,
                sigma_layers=2, sigma_out=16, color_weights=ptr(wc), color_in=32, color_hidden=64, color_layers=3, color_out=3, fc_weight=1.0, eval=3,
                sigma=ptr(sigma), rgbs=ptr(rgbs), units_dev=ptr(units_dev), rows_per_unit=rows_per_unit, scratch=ptr(scratch), scratch_bytes=scratch.numel())
            check(lib.nerftex_curved_shape_infer(ctypes.byref(desc), stream()))
            torch.cuda.synchronize()
            rows = torch.arange(B, device=dev)
            plain, unused, past = (rows < live) & ~marked, (rows < live) & marked, rows >= live
            assert torch.equal(sigma[plain], want_sigma[plain]) and torch.equal(rgbs[plain], want_rgb[plain]), (B, units)
            assert bool((sigma[unused] == 0).all()) and bool((rgbs[unused] == 0).all())
            assert bool((sigma[past] == SENTINEL).all()) and bool((rgbs[past] == SENTINEL).all())


# ---- 4. refusals of the plain entry, in the documented order, without a launch ---------------------------------------------------------------------------

def test_the_plain_entry_refuses_in_the_documented_order(dev):
    from nerftex_hip import lib, ptr, stream

    mesh = Mesh.of("quad", dev)
    p = mesh.proj
    x = _t(sf.sample_points(mesh.v, mesh.f, mesh.vn, 5, np.random.default_rng(1)), dev)
    idx, dis = p.knn(x, 4)
    fmap = _t(pf.seeded_map(5, 4), dev)
    outs = dict(p_uv=torch.full((5, 2), SENTINEL, device=dev), sdf=torch.full((5,), SENTINEL, device=dev), mask=torch.full((5,), 7, dtype=torch.uint8, device=dev),
                normal=torch.full((5, 3), SENTINEL, device=dev), face=torch.full((5,), -9, dtype=torch.int64, device=dev),
                xin=torch.full((5, 48), SENTINEL, dtype=torch.float16, device=dev))
    base = dict(rt=p.tracer._handle, xyz=ptr(x), idx=ptr(idx), dis=ptr(dis), N=5, K=4, verts=ptr(p.mesh_vertices), vn=ptr(p.vertex_normals), n_verts=4,
                face_uv=ptr(mesh.face_uv), n_faces=10, map=ptr(fmap), map_h=5, map_w=4, scale=1.0, offset=0.0, rate=1.0, h=0.05, n_freqs=12,
                **{k: ptr(v) for k, v in outs.items()})
    # each case breaks one argument and everything the order puts BEHIND it: the message names the first
    order = [(dict(xyz=None), "must not be NULL"), (dict(K=17), "1 <= K <= 16"), (dict(n_faces=3), "face_uv holds 3 faces"), (dict(map_w=16385), "between 1 and 16384"),
             (dict(n_freqs=10), "12 height bands"), (dict(map=ptr(fmap) + 4), "16-byte aligned"), (dict(scale=0.0), "positive and finite"),
             (dict(offset=float("nan")), "sdf_offset must be finite")]
    for k, (over, text) in enumerate(order):
        broken = dict(base)
        for later, _ in order[k:]:
            broken.update(later)
        assert lib.nerftex_shape_lookup(*broken.values(), stream()) == NERFTEX_ERR_INVALID
        assert text in lib.nerftex_last_error().decode(), (over, lib.nerftex_last_error().decode())
    for over, text in [(dict(K=0), "1 <= K <= 16"), (dict(map_h=0), "between 1 and 16384"), (dict(xin=ptr(outs["xin"]) + 2), "16-byte aligned"),
                       (dict(rate=float("inf")), "positive and finite"), (dict(h=-1.0), "positive and finite"), (dict(face=None), "must not be NULL")]:
        assert lib.nerftex_shape_lookup(*dict(base, **over).values(), stream()) == NERFTEX_ERR_INVALID
        assert text in lib.nerftex_last_error().decode(), (over, lib.nerftex_last_error().decode())
    assert lib.nerftex_shape_lookup(*dict(base, N=0).values(), stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((v == (7 if k == "mask" else -9 if k == "face" else SENTINEL)).all()) for k, v in outs.items()), "nothing was launched"


# ---- 5. the field on the reference's fixture -----------------------------------------------------------------------------------------------------------------

# the bars of the fixture test: the largest absolute error of u, v; of the height; of the normalised normal; of the features; of the ladder.
# Each is about four to five times the larger of what the fused and the op-by-op route measure against the fixture (u, v
# 2.4e-7 / 3.6e-7, height 1.1e-8 / 7.5e-9, normal 4.2e-7 both, features 1.22e-4 / 3.2e-6, ladder 4.0e-4 / 1.5e-5); features and ladder stay
# under DESIGN.md 4.15's 1e-3 and 2e-3.  Sigma and colour keep 4.15's own bars.
BAR_UV, BAR_SDF, BAR_NORMAL, BAR_FEATURES, BAR_LADDER = 2e-6, 5e-8, 2e-6, 5e-4, 1.6e-3


@pytest.fixture(scope="module")
def golden_field(dev):
    from ngp_harness.curved import CurvedField, star_flower_mesh

    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_python_import_shape.npz"))
    c = np.load(os.path.join(ROOT, "tests", "golden", "ref_python_curvedfield.npz"))
    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=float(g["h_threshold"])).to(dev).eval()
    with torch.no_grad():
        field.sigma_net.weights.copy_(torch.from_numpy(c["w_sigma"]))
        field.color_net.weights.copy_(torch.from_numpy(c["w_color"]))
    field.import_field(g["features"], float(g["grid_gap"]))
    field.import_shape(g["vertices_raw"], g["faces"], g["uvs_raw"], vertex_normals=g["vertex_normals"])
    return field, g


def test_import_shape_builds_the_fixtures_mesh(dev, golden_field):
    field, g = golden_field
    p = field.shape_projector
    assert field.imported and field.imported_type == "shape" and field.rescale
    assert np.array_equal(p.mesh_vertices.cpu().numpy(), g["vertices"]) and np.array_equal(field.shape_uvs.cpu().numpy(), g["uvs"])
    assert abs(field.recommended_sdf_factor / float(g["recommended_sdf_factor"]) - 1) < 1e-6
    assert abs(field.sdf_scale_factor / float(g["sdf_scale_factor"]) - 1) < 1e-6


@pytest.mark.parametrize("key", ["S0", "S1", "S2"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_by_op"])
def test_the_field_reproduces_the_reference_fixture(dev, golden_field, key, fused):
    field, g = golden_field
    rate = float(g[key + "_rate"])
    field.set_k_for_uv(int(g[key + "_K"])), field.set_uv_utilize_rate(rate), field.set_sdf_factor(float(g[key + "_sdf_factor"])), field.set_sdf_offset(float(g[key + "_offset"]))
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
            if fused:
                p_uv, sdf = field._shape_lookup(x)[:2]
            else:
                p_uv, sdf = field._shape_embed_reference(x, details=True)[3:5]
    finally:
        field.fused_glue = True
    want_mask = torch.from_numpy(g[key + "_h_mask"]).to(dev)
    assert torch.equal(mask, want_mask)
    uvh = torch.from_numpy(g[key + "_uvh"]).to(dev)
    e_uv, e_sdf = float((p_uv - uvh[:, :2] * rate).abs().max()), float((sdf - uvh[:, 2]).abs().max())
    e_n = float((normal.float() - torch.from_numpy(g[key + "_normal"]).to(dev)).abs().max())
    who = f"{key} {'fused' if fused else 'op by op'}"
    print(f"{who}: u, v error {e_uv:.3e} (bar {BAR_UV:.0e}), height error {e_sdf:.3e} (bar {BAR_SDF:.0e}), normal error {e_n:.3e} (bar {BAR_NORMAL:.0e})")
    assert e_uv <= BAR_UV and e_sdf <= BAR_SDF and e_n <= BAR_NORMAL
    if key + "_embed" in g:
        want = torch.from_numpy(g[key + "_embed"]).to(dev)
        e_feat, e_z = float((embed[:, :16].float() - want[:, :16]).abs().max()), float((embed[:, 16:].float() - want[:, 16:]).abs().max())
        print(f"{who}: embedding error, features {e_feat:.3e} (bar {BAR_FEATURES:.0e}), ladder {e_z:.3e} (bar {BAR_LADDER:.0e})")
        assert e_feat <= BAR_FEATURES and e_z <= BAR_LADDER
    want_s, want_c = torch.from_numpy(g[key + "_sigma"]).to(dev), torch.from_numpy(g[key + "_color"]).to(dev).float()
    print(f"{who}: sigma error {float((sigma.float() - want_s).abs().max()):.3e}, colour error {float((color.float() - want_c).abs().max()):.3e}; "
          f"{int(want_mask.sum())} rows inside the mask")
    assert torch.equal(sigma == 0, ~want_mask) and torch.equal((color == 0).all(-1), ~want_mask)
    torch.testing.assert_close(sigma.float(), want_s, rtol=3e-2, atol=3e-3)
    torch.testing.assert_close(color.float(), want_c, rtol=0, atol=2e-2)
    torch.testing.assert_close(dens["sigma"].float(), want_s, rtol=3e-2, atol=3e-3)
    assert got_s.dtype == torch.float32 and torch.equal(got_s, sigma.float()) and torch.equal(got_c, color.float()), "infer() is forward()"


def test_infer_marks_and_live_rows_on_the_field(dev, golden_field):
    field, g = golden_field
    field.set_k_for_uv(5), field.set_uv_utilize_rate(1.0), field.set_sdf_factor(float(g["sdf_scale_factor"])), field.set_sdf_offset(0.0)
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


# ---- 6. a frame ----------------------------------------------------------------------------------------------------------------------------------------------

def test_a_frame_of_the_map_on_the_height_field(dev):
    import raymarching
    from ngp_harness import scene
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.0625).to(dev).eval()
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
    never = field.graph_stamp()
    assert len(never) == 11 and not any(isinstance(s, str) for s in never), "a field that never imported keeps its stamp"
    r_mesh = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        r_mesh.update_extra_state_device()
    o, d = scene.get_rays(scene.rand_poses(1, 1.6, np.random.default_rng(11))[0], scene.intrinsics(32, 32), 32, 32)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    loops = dict(slots_per_ray=4, **KW)
    with torch.autocast("cuda", dtype=torch.float16):
        mesh_img, mesh_dep, _ = r_mesh.render_infer(o, d, **loops)
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_python_import_shape.npz"))
    field.import_field(pf.seeded_map(64, 64, seed=21), 1.0 / 64)
    field.import_shape(g["vertices_raw"], g["faces"], g["uvs_raw"], vertex_normals=g["vertex_normals"])
    assert field.graph_stamp()[:11] == never and field.graph_stamp()[11] == "import-shape"
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)  # (a grid that starts empty: initialize_states keeps the maximum)
    r.initialize_states(2)
    # occupancy: nothing beyond the threshold slab around the mesh.  |sdf| < h means the hit along the normal is nearer than h scale, and the
    # surface is never farther than that hit: a cell all of whose points are farther than h scale from every vertex PLUS the longest edge is empty
    H = r.grid_size
    coords = raymarching.morton3D_invert(torch.arange(H ** 3, dtype=torch.int32, device=dev)).float()
    centres = (2 * coords / (H - 1) - 1) * (1.0 - 1.0 / H)
    mv = field.shape_projector.mesh_vertices
    nearest = torch.cat([torch.cdist(centres[a:a + (1 << 16)], mv).min(-1)[0] for a in range(0, H ** 3, 1 << 16)])
    fi = torch.from_numpy(g["faces"].astype(np.int64)).to(dev)
    longest = float(torch.stack([(mv[fi[:, a]] - mv[fi[:, b]]).norm(dim=-1) for a, b in ((0, 1), (1, 2), (2, 0))]).max())
    slab = field.h_threshold * field._shape_scalars()[1]
    cell = 2.0 / H
    far = nearest > slab + longest + 2 * cell
    inside = (nearest < 0.25 * slab) & (centres[:, :2].abs().max(-1)[0] < 0.5)
    grid = r.density_grid[0]
    assert int(far.sum()) > H ** 3 // 2 and int(inside.sum()) > 100
    assert bool((grid[far] == 0).all()), "cells beyond the slab around the mesh are exactly empty"
    assert bool((grid[inside] > 0).all()), "cells at the surface are occupied"
    with torch.autocast("cuda", dtype=torch.float16):
        def frame():
            img, dep, _ = r.render_infer(o, d, **loops)
            img_g, dep_g, _ = r.render_infer_graphed(o, d, parts=2, block=2, **loops)
            img_p, dep_p, _ = r.render_infer_pipelined(o, d, parts=2, **loops)
            assert torch.equal(img_g, img) and torch.equal(dep_g, dep) and torch.equal(img_p, img) and torch.equal(dep_p, dep), "the three loops give one image"
            return img

        images = [frame()]
        assert float(images[0].std()) > 1e-3 and not torch.equal(images[0], mesh_img)
        graphs = r._infer_graphs
        r.render_infer_graphed(o, d, parts=2, block=2, **loops)
        assert r._infer_graphs is graphs, "the same state replays the recorded graphs"
        for change in (lambda: field.set_k_for_uv(2), lambda: field.set_sdf_factor(3.0), field.switch_shape_feature):
            change()
            r.initialize_states(2)
            graphs = r._infer_graphs
            images.append(frame())
            assert r._infer_graphs is not graphs, "a changed state re-records the graphs"
            assert not any(torch.equal(images[-1], im) for im in images[:-1]), "... and changes the image"
        assert field.imported_type == "field"
        field.switch_import()
        assert not field.imported and field.graph_stamp() == never
        img_m, dep_m, _ = r_mesh.render_infer_graphed(o, d, parts=2, block=2, **loops)
        assert torch.equal(img_m, mesh_img) and torch.equal(dep_m, mesh_dep), "switch_import() restores the mesh field's image bit for bit"
