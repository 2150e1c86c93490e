"""GPU: the curved field baked onto the vertices of a fine mesh (the unhash import) -- nerftex_vertex_lookup against the float64 statement of
tests/unhash_float64.py and against the op-by-op route, nerftex_curved_unhash_infer against its six pieces under the rows contract,
CurvedField.unhash / import_unhash_vertices against the reference's fixture (tools/make_golden.py: unhash_goldens), infer() with marks and live
rows, and a frame through the graphed loop."""
import ctypes
import os

import numpy as np
import pytest
import torch

import geometry_float64 as g
import shape_float64 as sf
import unhash_float64 as uf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.5
NERFTEX_ERR_INVALID = 1
KW = dict(dt_gamma=0.0, max_steps=256)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def trace32(oracle):
    return lambda v, f, o, d: oracle.raytrace(v, f, o, d)[:4]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Scene:
    """the device structures of one of unhash_float64's mesh pairs: the field's own projector (tracer, neighbour grid, vertex arrays), the fine
    mesh's tracer, vertices and corner table, the seeded per-vertex rows"""
    _made = {}

    def __init__(self, name, dev):
        from ngp_harness.curved import MeshProjector
        from RayTracer import RayTracer

        (self.v, self.f, self.vn), (self.fv, self.ff) = uf.mesh_of(name)
        self.proj = MeshProjector(self.v, self.f, vertex_normals=self.vn).to(dev)
        self.tracer = RayTracer(self.fv, self.ff)
        table = self.ff.astype(np.int32)
        if len(table) <= 8:  # (the RayTracer wrapper pads the BVH of so small a mesh with 8 far-away faces; CurvedField pads the table likewise)
            table = np.concatenate([table, np.zeros((8, 3), np.int32)], 0)
        self.fine_vertices, self.table, self.rows = _t(self.fv, dev), _t(table, dev), _t(uf.seeded_rows(len(self.fv)), dev)

    @classmethod
    def of(cls, name, dev):
        if name not in cls._made:
            cls._made[name] = cls(name, dev)
        return cls._made[name]


def _outputs(n, dev):
    return dict(sdf=torch.full((n,), SENTINEL, device=dev), mask=torch.full((n,), 7, dtype=torch.uint8, device=dev), normal=torch.full((n, 3), SENTINEL, device=dev),
                face=torch.full((n,), -9, dtype=torch.int64, device=dev), bary=torch.full((n, 3), SENTINEL, device=dev),
                xin=torch.full((n, 48), SENTINEL, dtype=torch.float16, device=dev))


def _arguments(scene, x, idx, dis, scale, offset, h, outs):
    from nerftex_hip import ptr

    p = scene.proj
    return dict(rt=scene.tracer._handle, xyz=ptr(x), idx=ptr(idx), dis=ptr(dis), N=x.shape[0], K=idx.shape[1], verts=ptr(p.mesh_vertices), vn=ptr(p.vertex_normals),
                n_verts=p.mesh_vertices.shape[0], wdist=0.05, fine=ptr(scene.fine_vertices), n_fine=scene.fine_vertices.shape[0], table=ptr(scene.table),
                n_faces=scene.table.shape[0], rows=ptr(scene.rows), scale=scale, offset=offset, h=h, n_freqs=12, **{k: ptr(v) for k, v in outs.items()})


def _lookup(scene, x, idx, dis, scale, offset, h):
    from nerftex_hip import lib, stream

    outs = _outputs(x.shape[0], x.device)
    rc = lib.nerftex_vertex_lookup(*_arguments(scene, x, idx, dis, scale, offset, h, outs).values(), stream())
    assert rc == 0, lib.nerftex_last_error().decode()
    return tuple(outs.values())


def _case(name, dev, trace32):
    P = uf.problem(name, device=dev)
    if "tol_t" not in P:
        R = P["rays"]
        uf.set_tolerances(P, trace32(R["v"], R["f"], R["o"], R["d"]))
    return P


def _fmt(r):
    return " ".join(f"{k} {v:.3f}" for k, v in r.items())


# ---- 1. the plain entry against float64 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(uf.CASES))
def test_plain_entry_passes_the_float64_check(dev, trace32, name):
    """Every case of unhash_float64: N = 1, 127 (odd: the last pair of lanes) and 512 on the subdivided star with its duplicated pole vertices, two
    faces under the tracer's padding with K clamped to 4 vertices, a row on a vertex, rows both traces miss, a scale with an offset, heights right
    at the mask threshold."""
    P = _case(name, dev, trace32)
    scene = Scene.of(uf.CASES[name][0], dev)
    assert P["features"].shape == tuple(scene.rows.shape)
    out = _lookup(scene, _t(P["x"], dev), _t(P["idx"], dev), _t(P["dis"], dev), P["scale"], P["offset"], P["h_threshold"])
    torch.cuda.synchronize()
    r = uf.check(P, *(o.cpu().numpy() for o in out))
    print(f"{name}: kernel ratios {_fmt(r)}", uf.describe(P))


# ---- 2. the plain entry against the op-by-op route --------------------------------------------------------------------------------------------------------

def _field(dev, h_threshold=0.0625, unhash=True):
    """a CurvedField over unhash_float64's star with the subdivided star and the seeded rows imported"""
    from ngp_harness.curved import CurvedField

    (v, f, vn), (fv, ff) = uf.mesh_of("star")
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=h_threshold, vertex_normals=vn).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
    if unhash:
        field.import_unhash_vertices(fv, ff, uf.seeded_rows(len(fv)))
    return field.eval()


@pytest.mark.parametrize("name", ["star_n512", "star_scaled", "star_far"])
def test_plain_entry_against_the_op_by_op_route(dev, trace32, name):
    """`_unhash_embed_reference` passes the float64 check itself; mask and face are the kernel's on every decided row; where the framework's normal
    has the kernel's bits, sdf is the route's bit for bit (the same tracer on the same ray, a true division, a subtraction).  Barycentrics and
    features are not bit-reproducible (the framework's cross product and norm sum in their own order): both routes are inside the float64 bars,
    so they differ by at most twice those."""
    _, N, h, scale, offset, *_ = uf.CASES[name]
    field = _field(dev, h)
    field.set_sdf_factor(scale), field.set_sdf_offset(offset)
    P = _case(name, dev, trace32)
    K, f_scale, f_offset, f_h = field._unhash_scalars()
    assert (K, f_scale, float(np.float32(f_offset)), f_h) == (8, P["scale"], P["offset"], h) and np.array_equal(field.features_imported.cpu().numpy(), P["features"])
    x, nb = _t(P["x"], dev), (_t(P["idx"], dev), _t(P["dis"], dev))
    with torch.no_grad():
        sdf, mask, normal, face, bary, xin = field._unhash_lookup(x, neighbours=nb)
        embed, _, w_mask, w_sdf, w_normal, w_face, w_bary = field._unhash_embed_reference(x, neighbours=nb, details=True)
    uf.check(P, *(o.cpu().numpy() for o in (sdf, mask, normal, face, bary, xin)))
    xin_w = torch.cat([embed.half(), torch.ones(len(x), 7, dtype=torch.float16, device=dev)], -1)
    r = uf.check(P, *(o.cpu().numpy() for o in (w_sdf, w_mask, w_normal, w_face, w_bary, xin_w)))
    same = (normal == w_normal).all(-1)
    print(f"{name}: op-by-op ratios {_fmt(r)}; the framework's normal has the kernel's bits on {float(same.float().mean()):.3f} of the rows")
    assert torch.equal(sdf[same], w_sdf[same]) and torch.equal(mask[same], w_mask[same]) and torch.equal(face[same], w_face[same])
    dec, dm, far = _t(P["decided"], dev), _t(P["decided_mask"], dev), _t(P["far"], dev)
    assert torch.equal(mask[dm], w_mask[dm]) and torch.equal(face[dec & _t(P["unique"], dev)], w_face[dec & _t(P["unique"], dev)])
    rows = dec & ~far
    assert bool(((sdf - w_sdf).abs() <= 2 * _t(P["tol_sdf"], dev))[rows].all())
    assert bool(((bary - w_bary).abs() <= 2 * _t(P["tol_bary"], dev))[rows].all())
    assert bool(((xin[:, :16].double() - embed[:, :16].double()).abs() <= 2 * _t(P["tol_feature"], dev))[rows].all())


# ---- 3. the chain against its pieces -----------------------------------------------------------------------------------------------------------------------

def _half_weights(n, seed, scale, dev):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-scale, scale, n).astype(np.float16)).to(dev)


def _pieces(scene, x, d, K, scalars, ws, wc, eval_bits):
    """nerftex_knn_query, nerftex_vertex_lookup, nerftex_ffmlp_inference, nerftex_curved_mid_forward, nerftex_ffmlp_inference,
    nerftex_curved_out_forward one after the other: -> sigma [B] fp32, rgbs [B,3] fp32, mask"""
    from nerftex_hip import check, lib, ptr, stream

    n, dev = x.shape[0], x.device
    idx, dis = scene.proj.knn(x, K)
    _, mask, normal, _, _, xin = _lookup(scene, x, idx, dis, *scalars)
    h = torch.empty(n, 16, dtype=torch.float16, device=dev)
    buf = torch.empty(n, 64, dtype=torch.float16, device=dev)
    check(lib.nerftex_ffmlp_inference(ptr(xin), ptr(ws), n, 48, 16, 32, 2, 0, 6, ptr(buf), ptr(h), stream()))
    sigma_raw, cin = torch.empty(n, dtype=torch.float16, device=dev), torch.empty(n, 32, dtype=torch.float16, device=dev)
    check(lib.nerftex_curved_mid_forward(ptr(h), ptr(normal), ptr(d), n, 1.0, eval_bits, ptr(sigma_raw), ptr(cin), stream()))
    hc = torch.empty(n, 16, dtype=torch.float16, device=dev)
    check(lib.nerftex_ffmlp_inference(ptr(cin), ptr(wc), n, 32, 16, 64, 3, 0, 6, ptr(buf), ptr(hc), stream()))
    sigma, color = torch.empty(n, dtype=torch.float16, device=dev), torch.empty(n, 3, dtype=torch.float16, device=dev)
    check(lib.nerftex_curved_out_forward(ptr(hc), 16, ptr(sigma_raw), ptr(mask), n, ptr(sigma), ptr(color), stream()))
    return sigma.float(), color.float(), mask.bool()


@pytest.mark.parametrize("mesh_name,scalars", [("quad", (1.0, 0.0, 0.0625)), ("star", (2.5, 0.01, 0.0625)), ("star", (1.0, 0.0, 20.0))])
def test_chain_is_its_pieces_under_the_rows_contract(dev, mesh_name, scalars):
    from nerftex_hip import CurvedUnhashInferDesc, check, lib, ptr, stream

    scene = Scene.of(mesh_name, dev)
    p, K, B = scene.proj, min(8, len(scene.v)), 256
    ws, wc = _half_weights(3072, 3, 0.6, dev), _half_weights(11264, 4, 0.25, dev)
    rng = np.random.default_rng(B + len(scene.v))
    x = _t(sf.sample_points(scene.v, scene.f, scene.vn, B, rng, far_share=0.05, on_vertex=True), dev)
    d = rng.normal(size=(B, 3)).astype(np.float32)
    d = _t(d / np.linalg.norm(d, axis=-1, keepdims=True), dev)
    want_sigma, want_rgb, want_mask = _pieces(scene, x, d, K, scalars, ws, wc, 3)
    assert float(want_sigma.max()) > 0 and float(want_rgb.max()) > 0 and 0 < int(want_mask.sum()) < B  # (not a comparison of zeros)
    assert bool((want_sigma[~want_mask] == 0).all()) and bool((want_rgb[~want_mask] == 0).all())
    marked = torch.zeros(B, dtype=torch.bool, device=dev)
    marked[::7] = True
    marked[32:64] = True
    marked[0] = False
    xm, dm = x.clone(), d.clone()
    xm[marked] = 1e30
    dm[marked, 0] = 1e30
    scratch = torch.empty(lib.nerftex_curved_unhash_infer_scratch_bytes(B), dtype=torch.uint8, device=dev)
    scale, off, h = scalars
    for units, rows_per_unit, live in ((0, 128, 0), (1, 128, 128), (3, 64, 192), (None, 0, B)):
        units_dev = None if units is None else torch.tensor([units], dtype=torch.int32, device=dev)
        sigma = torch.full((B,), SENTINEL, dtype=torch.float32, device=dev)
        rgbs = torch.full((B, 3), SENTINEL, dtype=torch.float32, device=dev)
        desc = CurvedUnhashInferDesc(
            knn=p._knn.value, tracer=scene.tracer._handle.value, xyz=ptr(xm), dirs=ptr(dm), B=B, n_verts=p.mesh_vertices.shape[0], mesh_vertices=ptr(p.mesh_vertices),
            vertex_normals=ptr(p.vertex_normals), K=K, dir_vec_wdist=0.05, fine_vertices=ptr(scene.fine_vertices), n_fine_verts=scene.fine_vertices.shape[0],
            face_vertices=ptr(scene.table), n_faces=scene.table.shape[0], vertex_features=ptr(scene.rows), n_features=16, sdf_scale=scale, sdf_offset=off,
            h_threshold=h, n_freqs=12, sigma_weights=ptr(ws), sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16, color_weights=ptr(wc), color_in=32,
            color_hidden=64, color_layers=3, color_out=3, fc_weight=1.0, eval=3, sigma=ptr(sigma), rgbs=ptr(rgbs), units_dev=ptr(units_dev),
            rows_per_unit=rows_per_unit, scratch=ptr(scratch), scratch_bytes=scratch.numel())
        check(lib.nerftex_curved_unhash_infer(ctypes.byref(desc), stream()))
        torch.cuda.synchronize()
        rows = torch.arange(B, device=dev)
        plain, unused, past = (rows < live) & ~marked, (rows < live) & marked, rows >= live
        assert torch.equal(sigma[plain], want_sigma[plain]) and torch.equal(rgbs[plain], want_rgb[plain]), (units, rows_per_unit)
        assert bool((sigma[unused] == 0).all()) and bool((rgbs[unused] == 0).all())
        assert bool((sigma[past] == SENTINEL).all()) and bool((rgbs[past] == SENTINEL).all())
    # the chain's own refusals that need a raytracer: the face count, then the lookup's values, then the pointers and the scratch
    base = {n: getattr(desc, n) for n, _ in CurvedUnhashInferDesc._fields_}
    for over, text in ((dict(n_faces=3), "must hold its"), (dict(n_fine_verts=0), "fine mesh needs"), (dict(n_freqs=10), "12 height bands"),
                       (dict(vertex_features=ptr(scene.rows) + 4), "16-byte aligned"), (dict(sdf_scale=0.0), "positive and finite"),
                       (dict(sdf_offset=float("inf")), "sdf_offset must be finite"), (dict(fine_vertices=None), "must not be NULL"),
                       (dict(scratch_bytes=scratch.numel() - 1), "must not be NULL"), (dict(scratch=ptr(scratch) + 16), "256-byte aligned"),
                       (dict(color_weights=ptr(wc) + 2), "weight vectors must be 16-byte aligned")):
        assert lib.nerftex_curved_unhash_infer(ctypes.byref(CurvedUnhashInferDesc(**dict(base, **over))), stream()) == NERFTEX_ERR_INVALID
        assert text in lib.nerftex_last_error().decode(), (over, lib.nerftex_last_error().decode())
    assert lib.nerftex_curved_unhash_infer(ctypes.byref(CurvedUnhashInferDesc(**dict(base, B=0, xyz=None))), stream()) == 0


# ---- 4. refusals of the plain entry, in the documented order, without a launch ---------------------------------------------------------------------------

def test_the_plain_entry_refuses_in_the_documented_order(dev):
    from nerftex_hip import lib, ptr, stream

    scene = Scene.of("quad", dev)
    x = _t(sf.sample_points(scene.v, scene.f, scene.vn, 5, np.random.default_rng(1)), dev)
    idx, dis = scene.proj.knn(x, 4)
    outs = _outputs(5, dev)
    base = _arguments(scene, x, idx, dis, 1.0, 0.0, 0.0625, outs)
    assert base["n_faces"] == 10 and base["n_verts"] == 4 and base["K"] == 4
    # each case breaks one argument and everything the order puts BEHIND it: the message names the first
    order = [(dict(xyz=None), "must not be NULL"), (dict(K=17), "1 <= K <= 16"), (dict(n_verts=0), "the field's mesh needs"), (dict(n_fine=0), "the fine mesh needs"),
             (dict(n_faces=3), "face_vertices holds 3 faces"), (dict(n_freqs=10), "12 height bands"), (dict(rows=ptr(scene.rows) + 4), "16-byte aligned"),
             (dict(scale=0.0), "positive and finite"), (dict(offset=float("nan")), "sdf_offset must be finite")]
    for k, (over, text) in enumerate(order):
        broken = dict(base)
        for later, _ in order[k:]:
            broken.update(later)
        assert lib.nerftex_vertex_lookup(*broken.values(), stream()) == NERFTEX_ERR_INVALID
        assert text in lib.nerftex_last_error().decode(), (over, lib.nerftex_last_error().decode())
    for over, text in [(dict(K=0), "1 <= K <= 16"), (dict(xin=ptr(outs["xin"]) + 2), "16-byte aligned"), (dict(scale=float("inf")), "positive and finite"),
                       (dict(h=-1.0), "positive and finite"), (dict(bary=None), "must not be NULL"), (dict(fine=None), "must not be NULL")]:
        assert lib.nerftex_vertex_lookup(*dict(base, **over).values(), stream()) == NERFTEX_ERR_INVALID
        assert text in lib.nerftex_last_error().decode(), (over, lib.nerftex_last_error().decode())
    assert lib.nerftex_vertex_lookup(*dict(base, N=0).values(), stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((v == (7 if k == "mask" else -9 if k == "face" else SENTINEL)).all()) for k, v in outs.items()), "nothing was launched"


# ---- 5. the field on the reference's fixture -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_field(dev):
    from ngp_harness.curved import CurvedField

    G = np.load(os.path.join(ROOT, "tests", "golden", "ref_python_unhash.npz"))
    torch.manual_seed(0)
    field = CurvedField(G["vertices"], G["faces"], bound=1.0, h_threshold=float(G["h_threshold"]), vertex_normals=G["vertex_normals"]).to(dev).eval()
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
    return field, G


def _fixture_statement(field, G, key, features, dev, trace32):
    """the float64 statement over the fixture's meshes with the FIELD's own neighbour lists (the star's pole vertices are duplicated: which copies a
    search returns is its own business), and the rows on which the fixture's search returned the same lists"""
    x = torch.from_numpy(G["xyz"]).to(dev)
    idx, dis = field.projector.knn(x, 8)
    coarse = (G["vertices"], G["faces"].astype(np.uint32), G["vertex_normals"])
    fine = (G["fine_vertices"], G["fine_faces"].astype(np.int64))
    P = uf.build_problem("fixture " + key, coarse, fine, features, G["xyz"], float(G["h_threshold"]), float(G[key + "_sdf_factor"]), float(G[key + "_offset"]),
                         device=dev, neighbours=(idx.cpu().numpy(), dis.cpu().numpy()))
    R = P["rays"]
    uf.set_tolerances(P, trace32(R["v"], R["f"], R["o"], R["d"]))
    return P, (idx, dis), (idx.cpu().numpy() == G["knn_idx"]).all(1)


def test_unhash_bakes_the_encoder_onto_one_subdivision_and_keeps_the_surface(dev, golden_field, trace32):
    """unhash(min_vnum) on the fixture's mesh: one round gives the fixture's fine mesh; the baked rows are encoder(vertices) in fp32 bit for bit, under
    an fp16 autocast too; sdf and h_mask agree with the mesh field's own projector on decided rows -- midpoint subdivision leaves the surface where
    it was, up to the rounding of the midpoints to fp32: half an ulp of a coordinate below 1 per component, sqrt(3) 2^-25, over the cosine between
    ray and face; each kernel is within tol_sdf of its own float64 statement."""
    field, G = golden_field
    n_fine = len(G["fine_vertices"])
    with torch.autocast("cuda", dtype=torch.float16):
        out = field.unhash(min_vnum=n_fine)
    assert field.imported and field.imported_type == "unhash" and set(out) == {"vertices", "faces", "features", "sdf_factor"} and out["sdf_factor"] == 1.0
    assert np.array_equal(out["vertices"], G["fine_vertices"]) and np.array_equal(out["faces"], G["fine_faces"])
    with torch.no_grad():
        want = field.encoder(torch.from_numpy(out["vertices"]).to(dev), bound=field.bound)
    assert want.dtype == torch.float32 and field.features_imported.dtype == torch.float32 and float(want.abs().max()) > 0.1
    assert torch.equal(field.features_imported, want) and np.array_equal(out["features"], want.cpu().numpy())
    assert tuple(field.unhash_face_vertices.shape) == (len(G["fine_faces"]), 3) and field.unhash_face_vertices.dtype == torch.int32
    more = field.unhash(min_vnum=n_fine + 1)
    assert len(more["vertices"]) > 3 * n_fine and len(more["faces"]) == 16 * len(G["faces"]), "a second round"
    field.import_unhash_vertices(**out)
    P, nb, _ = _fixture_statement(field, G, "U0", out["features"], dev, trace32)
    x = torch.from_numpy(G["xyz"]).to(dev)
    with torch.no_grad():
        sdf, mask, normal, face, bary, xin = field._unhash_lookup(x, neighbours=nb)
        _, p_sdf, p_mask, p_normal, _, _, _ = field.projector.project_fused(x, neighbours=nb, h_threshold=field.h_threshold)
    uf.check(P, *(o.cpu().numpy() for o in (sdf, mask, normal, face, bary, xin)))
    assert torch.equal(normal, p_normal), "the hoisted normal: the projector's bits"
    N = len(G["xyz"])
    ref = P["rays"]["ref"]
    cos = np.where(ref["t_best"][:N] < ref["t_best"][N:], ref["cos"][:N], ref["cos"][N:])  # (of the nearer hit)
    rows = P["decided"] & ~P["far"]
    moved = 2 * P["tol_sdf"] + np.sqrt(3.0) * 2.0 ** -25 / np.maximum(cos, g.GRAZE)
    err = np.abs(sdf.cpu().numpy() - p_sdf[:, 0].cpu().numpy())
    print(f"unhash against the mesh field's projector: sdf differs by at most {err[rows].max():.3e} ({(err / moved)[rows].max():.3f} of the bound)")
    assert (err <= moved)[rows].all()
    clear = rows & (np.abs(np.abs(P["sdf"]) - P["h_limit"]) > 1e-4 + moved)
    assert clear.mean() > 0.9 and np.array_equal(mask.cpu().numpy().astype(bool)[clear], p_mask.cpu().numpy()[clear])
    field.switch_import()
    assert not field.imported


@pytest.mark.parametrize("key", ["U0", "U1", "U2"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_by_op"])
def test_the_field_reproduces_the_reference_fixture(dev, golden_field, trace32, key, fused):
    """Through embed() with the field's own search, fused and op by op: inside the float64 bars of the statement over the field's neighbour lists; and
    where the reference's search returned the same lists, within twice those bars of the fixture's values (the fixture is inside them, too:
    tests/test_unhash_cpu.py), mask and face equal."""
    field, G = golden_field
    features = G["U2_features"] if key == "U2" else G["features"]
    field.import_unhash_vertices(G["fine_vertices"], G["fine_faces"], features, sdf_factor=float(G[key + "_sdf_factor"]))
    field.set_sdf_offset(float(G[key + "_offset"]))
    assert field.sdf_scale_factor == float(G[key + "_sdf_factor"])
    P, nb, same_lists = _fixture_statement(field, G, key, features, dev, trace32)
    assert same_lists.mean() > 0.9
    x = torch.from_numpy(G["xyz"]).to(dev)
    field.fused_glue = fused
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._unhash_fused(x) == fused and field._source_fused(x) == fused
            embed, normal, mask = field.embed(x)
            dens = field.density(x)
            if fused:
                sdf, _, raw, face, bary, _ = field._unhash_lookup(x)
            else:
                sdf, raw, face, bary = field._unhash_embed_reference(x, details=True)[3:]
    finally:
        field.fused_glue = True
    assert embed.shape == (512, 41) and embed.dtype == (torch.float16 if fused else torch.float32)
    xin = torch.cat([embed.half(), torch.ones(512, 7, dtype=torch.float16, device=dev)], -1)
    r = uf.check(P, *(o.cpu().numpy() for o in (sdf, mask, raw, face, bary, xin)))
    e_n = float((normal.float() - raw / (raw.norm(dim=-1, keepdim=True) + 1e-5)).abs().max())
    assert e_n <= 4 * U, "normal_coarse is the raw normal over its length + 1e-5 (tools/map.py:720)"
    assert bool((dens["sigma"][~mask] == 0).all())
    rows = same_lists & P["decided"] & ~P["far"]
    dm = same_lists & P["decided_mask"]
    assert np.array_equal(mask.cpu().numpy()[dm], G[key + "_h_mask"][dm])
    u = rows & P["unique"]
    assert np.array_equal(face.cpu().numpy()[u], G[key + "_face"][u].astype(np.int64))
    e_sdf = np.abs(sdf.cpu().numpy() - G[key + "_sdf"]) / (2 * P["tol_sdf"])
    e_f = (np.abs(embed[:, :16].double().cpu().numpy() - G[key + "_embed"][:, :16]) / (2 * P["tol_feature"])).max(1)
    print(f"{key} {'fused' if fused else 'op by op'}: float64 ratios {_fmt(r)}; against the fixture, of twice the bars: sdf {e_sdf[rows].max():.3f} features {e_f[rows].max():.3f}; "
          f"the same neighbour lists on {same_lists.mean():.3f} of the rows, {int(mask.sum())} rows inside the mask")
    assert (e_sdf[rows] <= 1).all() and (e_f[rows] <= 1).all()


def test_infer_is_forward_with_marks_and_live_rows(dev, golden_field):
    field, G = golden_field
    field.import_unhash_vertices(G["fine_vertices"], G["fine_faces"], G["features"])
    field.set_sdf_offset(0.0)
    with torch.no_grad():
        field.sigma_net.weights.mul_(3.0)
    rng = np.random.default_rng(5)
    x = torch.from_numpy(G["xyz"]).to(dev)
    d = rng.normal(size=(512, 3)).astype(np.float32)
    d = _t(d / np.linalg.norm(d, axis=-1, keepdims=True), dev)
    marked = torch.zeros(512, dtype=torch.bool, device=dev)
    marked[::5] = True
    xm, dm = x.clone(), d.clone()
    xm[marked] = 1e30
    dm[marked, 0] = 1e30
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._infer_unhash_fused(x, d) and field._infer_route(x, d)[0] == "nerftex_curved_unhash_infer"
            sigma, color, _ = field(x, d)
            all_s, all_c = field.infer(x, d)
            got_s, got_c = field.infer(xm, dm, (torch.tensor([3], dtype=torch.int32, device=dev), 128))
            field.fused_glue = False
            assert field._infer_route(x, d) is None, "fused_glue off: forward(), op by op"
    finally:
        field.fused_glue = True
        with torch.no_grad():
            field.sigma_net.weights.div_(3.0)
    assert all_s.dtype == torch.float32 and torch.equal(all_s, sigma.float()) and torch.equal(all_c, color.float()), "infer() is forward()"
    rows = torch.arange(512, device=dev)
    plain, unused = (rows < 384) & ~marked, (rows < 384) & marked
    assert torch.equal(got_s[plain], sigma.float()[plain]) and torch.equal(got_c[plain], color.float()[plain]) and float(got_s[plain].max()) > 0
    assert bool((got_s[unused] == 0).all()) and bool((got_c[unused] == 0).all())


# ---- 6. a frame ----------------------------------------------------------------------------------------------------------------------------------------------

def test_a_frame_through_the_graphed_loop_and_back_to_the_mesh_field(dev):
    from ngp_harness import scene
    from ngp_harness.model import Renderer

    field = _field(dev, unhash=False)
    with torch.no_grad():
        field.sigma_net.weights.mul_(3.0)
    never = field.graph_stamp()
    r_mesh = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        r_mesh.update_extra_state_device()
    o, d = scene.get_rays(scene.rand_poses(1, 1.6, np.random.default_rng(11))[0], scene.intrinsics(64, 64), 64, 64)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    loops = dict(slots_per_ray=4, **KW)
    with torch.autocast("cuda", dtype=torch.float16):
        mesh_img, mesh_dep, _ = r_mesh.render_infer(o, d, **loops)
    baked = field.unhash(min_vnum=2000)
    assert len(baked["vertices"]) == len(uf.mesh_of("star")[1][0]) and field.graph_stamp()[:len(never)] == never and field.graph_stamp()[len(never)] == "import-unhash"
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)  # (a grid that starts empty: initialize_states keeps the maximum)
    r.initialize_states(2)
    with torch.autocast("cuda", dtype=torch.float16):
        img, dep, _ = r.render_infer(o, d, **loops)
        img_g, dep_g, _ = r.render_infer_graphed(o, d, parts=2, block=2, **loops)
        assert torch.equal(img_g, img) and torch.equal(dep_g, dep), "the graphed loop gives the reference loop's frame"
        assert float(img.std()) > 1e-3 and not torch.equal(img, mesh_img), "the baked rows are not the table's values between the vertices"
        graphs = r._infer_graphs
        r.render_infer_graphed(o, d, parts=2, block=2, **loops)
        assert r._infer_graphs is graphs, "the same state replays the recorded graphs"
        field.set_sdf_factor(2.0)
        r.initialize_states(2)
        img2, _, _ = r.render_infer_graphed(o, d, parts=2, block=2, **loops)
        assert r._infer_graphs is not graphs and not torch.equal(img2, img), "a changed state re-records the graphs and changes the image"
        field.switch_import()
        assert not field.imported and field.graph_stamp() == never
        img_m, dep_m, _ = r_mesh.render_infer_graphed(o, d, parts=2, block=2, **loops)
        assert torch.equal(img_m, mesh_img) and torch.equal(dep_m, mesh_dep), "switch_import() restores the mesh field's image bit for bit"
