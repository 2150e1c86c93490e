"""GPU: an imported texture rendered on a new UV-mapped mesh through the SH-lit curved field -- nerftex_shape_light_lookup against
nerftex_shape_lookup (bit for bit), the framework's grid_sample(mode='nearest') fed the kernel's own p_uv (bit for bit), the face table (bit for
bit) and the feature read's float64 bound for phi; nerftex_curved_light_shape_infer under the rows contract, its shading normal and colour
against forward() inside the bounds of tests/shape_light_float64.py and tests/sh_light_float64.py; a 32 x 32 frame through the three loops.
Every comparison prints its largest error-to-bound ratio (DESIGN.md 4.18 records them)."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import import_light_float64 as il64
import normal_net_float64 as nn64
import planar_float64 as pf
import sh_light_float64 as f64
import shape_float64 as sf
import shape_light_float64 as sl64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.5
NERFTEX_ERR_INVALID = 1
KINK_CAP = 0.02  # (DESIGN.md 4.17's cap on the rows a kink of the head excludes)
KW = dict(dt_gamma=0.0, max_steps=256)
P_LOOKUP = 3
SIZES = (1, 127, 128, 129, 384)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _lit_field(dev, h_threshold=0.0625):
    """tests/test_gpu_import_light.py's star-flower field: a normal net whose angles are of order 1."""
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


# ---- 1. the plain entry -----------------------------------------------------------------------------------------------------------------------------------

class Mesh:
    """the device structures of one of shape_float64's meshes: raytracer, neighbour grid, vertex arrays, face_uv, and seeded face frames that are
    not orthonormal and differ per face (the kernel copies them; `uv_face_frames` has its own test)"""
    _made = {}

    def __init__(self, name, dev):
        from ngp_harness.curved import MeshProjector

        self.v, self.f, self.vn, self.uvs = sf.mesh_of(name)
        self.proj = MeshProjector(self.v, self.f, vertex_normals=self.vn).to(dev)
        face_uv = self.uvs[self.f.astype(np.int64)].reshape(-1, 6)
        frames = (np.eye(3, dtype=np.float32) + np.random.default_rng(len(self.f)).normal(0, 0.3, (len(self.f), 3, 3))).astype(np.float32)
        if len(face_uv) <= 8:  # (the RayTracer wrapper pads the BVH of so small a mesh with 8 far-away faces)
            face_uv = np.concatenate([face_uv, np.zeros((8, 6), np.float32)], 0)
        self.face_uv = _t(face_uv, dev)
        self.face_tbn = _t(sl64.padded_table(frames), dev)

    @classmethod
    def of(cls, name, dev):
        if name not in cls._made:
            cls._made[name] = cls(name, dev)
        return cls._made[name]


def _maps_on(dev, H, W, P=P_LOOKUP):
    phi, local, sample, ids = il64.seeded_light_maps(H, W, P)
    frame = np.zeros((H, W, 12), np.float32)
    frame[..., :9], frame[..., 9] = local, ids
    inv = np.linalg.inv(sample.astype(np.float32)).astype(np.float32)
    rows = np.zeros((P, 12), np.float32)
    rows[:, :9] = inv.reshape(P, 9)
    return dict(phi=_t(phi, dev), local=_t(local, dev), ids=_t(ids, dev), inv=_t(inv, dev), frame=_t(frame, dev), rows=_t(rows, dev), phi_np=phi)


def _unlit(mesh, x, idx, dis, fmap, scale, offset, rate, h):
    from nerftex_hip import check, lib, ptr, stream

    n, dev, p = x.shape[0], x.device, mesh.proj
    out = dict(p_uv=torch.empty(n, 2, device=dev), sdf=torch.empty(n, device=dev), mask=torch.empty(n, dtype=torch.uint8, device=dev),
               normal=torch.empty(n, 3, device=dev), face=torch.empty(n, dtype=torch.int64, device=dev), xin=torch.empty(n, 48, dtype=torch.float16, device=dev))
    check(lib.nerftex_shape_lookup(p.tracer._handle, ptr(x), ptr(idx), ptr(dis), n, idx.shape[1], ptr(p.mesh_vertices), ptr(p.vertex_normals), p.mesh_vertices.shape[0],
                                   ptr(mesh.face_uv), mesh.face_uv.shape[0], ptr(fmap), fmap.shape[0], fmap.shape[1], scale, offset, rate, h, 12,
                                   *(ptr(v) for v in out.values()), stream()))
    return out


def _lit_outputs(n, dev):
    return dict(p_uv=torch.full((n, 2), SENTINEL, device=dev), sdf=torch.full((n,), SENTINEL, device=dev), mask=torch.full((n,), 7, dtype=torch.uint8, device=dev),
                normal=torch.full((n, 3), SENTINEL, device=dev), face=torch.full((n,), -9, dtype=torch.int64, device=dev),
                xin=torch.full((n, 48), SENTINEL, dtype=torch.float16, device=dev), phi=torch.full((n, 8), SENTINEL, device=dev),
                ids=torch.full((n,), -9, dtype=torch.int32, device=dev), local=torch.full((n, 9), SENTINEL, device=dev),
                sample=torch.full((n, 9), SENTINEL, device=dev), new=torch.full((n, 9), SENTINEL, device=dev))


def _lit_args(mesh, x, idx, dis, fmap, m, scale, offset, rate, h, out):
    from nerftex_hip import ptr

    p = mesh.proj
    return dict(rt=p.tracer._handle, xyz=ptr(x), idx=ptr(idx), dis=ptr(dis), N=x.shape[0], K=idx.shape[1], verts=ptr(p.mesh_vertices), vn=ptr(p.vertex_normals),
                n_verts=p.mesh_vertices.shape[0], face_uv=ptr(mesh.face_uv), n_faces=mesh.face_uv.shape[0], face_tbn=ptr(mesh.face_tbn),
                n_tbn_faces=mesh.face_tbn.shape[0], map=ptr(fmap), phi_map=ptr(m["phi"]), frame_map=ptr(m["frame"]), rows=ptr(m["rows"]), map_h=fmap.shape[0],
                map_w=fmap.shape[1], P=m["rows"].shape[0], scale=scale, offset=offset, rate=rate, h=h, n_freqs=12, **{k: ptr(v) for k, v in out.items()})


@pytest.mark.parametrize("name", list(sf.CASES))
def test_plain_entry_against_the_unlit_lookup_grid_sample_and_the_face_table(dev, name):
    """shape_float64's cases (the quad, the height field, the star mesh; K 2, 4, 5, 8, 16; maps 1x1, 5x4, 64x48), at batch sizes around the
    32-point wave, row 0 exactly on a vertex.  The points are the cases' own recipe over the library's neighbour search."""
    from nerftex_hip import check, lib, stream

    mesh_name, _, K, h, scale, offset, rate, far, map_hw = sf.CASES[name]
    mesh = Mesh.of(mesh_name, dev)
    fmap, m = _t(pf.seeded_map(*map_hw), dev), _maps_on(dev, *map_hw)
    rng = np.random.default_rng(sum(map(ord, name)) + 4000)
    xs = _t(sf.sample_points(mesh.v, mesh.f, mesh.vn, max(SIZES), rng, far_share=far, on_vertex=True), dev)
    gs = torch.nn.functional.grid_sample
    image = lambda a: a.permute(2, 1, 0).unsqueeze(0)  # noqa: E731
    for n in SIZES:
        x = xs[:n].contiguous()
        idx, dis = mesh.proj.knn(x, min(K, len(mesh.v)))
        idx, dis = idx.int().contiguous(), dis.float().contiguous()
        want = _unlit(mesh, x, idx, dis, fmap, scale, offset, rate, h)
        out = _lit_outputs(n, dev)
        check(lib.nerftex_shape_light_lookup(*_lit_args(mesh, x, idx, dis, fmap, m, scale, offset, rate, h, out).values(), stream()))
        for k, w in want.items():
            same = torch.equal(out[k].view(torch.int16), w.view(torch.int16)) if k == "xin" else torch.equal(out[k], w)
            assert same, f"{name} N={n}: {k} is not nerftex_shape_lookup's"
        none = ~(want["normal"] != 0).any(-1)  # rows without a finite normal
        assert bool(none[0]), "the row on a vertex has no normal"
        ok = ~none
        p_uv = out["p_uv"]
        grid = p_uv[None, None]
        want_id = gs(image(m["ids"][..., None]), grid, mode="nearest", align_corners=True, padding_mode="zeros")[0, 0, 0].long()
        want_local = gs(image(m["local"]), grid, mode="nearest", align_corners=True, padding_mode="zeros")[0, :, 0].permute(1, 0)
        assert torch.equal(out["ids"].long()[ok], want_id[ok]) and torch.equal(out["local"][ok], want_local[ok]), f"{name} N={n}: the nearest reads"
        assert torch.equal(out["sample"][ok], m["inv"].reshape(-1, 9)[want_id[ok]])
        assert torch.equal(out["new"][ok], mesh.face_tbn[out["face"].clamp(min=0)][ok][:, :9]), f"{name} N={n}: new_tbn = face_tbn[max(face, 0)]"
        # rows without a normal: zeros for phi and all three frames, id -1, on top of the unlit constants
        for k in ("phi", "local", "sample", "new"):
            assert not out[k][none].any(), k
        assert bool((out["ids"][none] == -1).all()) and bool((out["face"][none] == -1).all())
        # the bilinear phi read inside the feature read's float64 bound, from the kernel's own (u, v); its narrowing too
        value, bound = pf.bilinear(m["phi_np"], p_uv[:, 0].cpu().numpy(), p_uv[:, 1].cpu().numpy())
        okn = ok.cpu().numpy()
        for got in (out["phi"].double().cpu().numpy(), out["phi"].half().double().cpu().numpy()):
            assert (np.abs(got - value) / bound)[okn].max(initial=0.0) <= 1.0
    hit = out["face"] >= 0
    print(f"{name}: {int(hit.sum())} of {n} rows hit a face, {int(none.sum())} without a normal, {len(set(out['ids'][ok].tolist()))} patches, "
          f"{len(set(out['face'][hit].tolist()))} faces")
    assert int(hit.sum()) > n // 4 and bool((out["new"][hit] != 0).any(-1).all())


def test_the_plain_entry_refuses_in_the_documented_order(dev):
    from nerftex_hip import lib, ptr, stream

    mesh = Mesh.of("quad", dev)
    x = _t(sf.sample_points(mesh.v, mesh.f, mesh.vn, 5, np.random.default_rng(1)), dev)
    idx, dis = mesh.proj.knn(x, 4)
    idx, dis = idx.int().contiguous(), dis.float().contiguous()
    fmap, m = _t(pf.seeded_map(5, 4), dev), _maps_on(dev, 5, 4)
    out = _lit_outputs(5, dev)
    base = _lit_args(mesh, x, idx, dis, fmap, m, 1.0, 0.0, 1.0, 0.05, out)
    assert base["n_faces"] == 10 and base["n_tbn_faces"] == 10
    # each case breaks one argument and everything the order puts BEHIND it: the message names the first
    order = [(dict(xyz=None), "must not be NULL"), (dict(K=17), "1 <= K <= 16"), (dict(n_faces=3), "face_uv holds 3 faces"), (dict(map_w=16385), "between 1 and 16384"),
             (dict(n_freqs=10), "12 height bands"), (dict(map=ptr(fmap) + 4), "16-byte aligned"), (dict(scale=0.0), "positive and finite"),
             (dict(offset=float("nan")), "sdf_offset must be finite"), (dict(P=0), "patch frames"), (dict(phi_map=None), "lit outputs must not be NULL"),
             (dict(frame_map=ptr(m["frame"]) + 4), "phi must be 16-byte aligned"), (dict(n_tbn_faces=2), "one frame per face")]
    for k, (over, text) in enumerate(order):
        broken = dict(base)
        for later, _ in order[k:]:
            broken.update(later)
        assert lib.nerftex_shape_light_lookup(*broken.values(), stream()) == NERFTEX_ERR_INVALID
        assert text in lib.nerftex_last_error().decode(), (over, lib.nerftex_last_error().decode())
    for over, text in [(dict(face_tbn=None), "must not be NULL"), (dict(new=None), "must not be NULL"), (dict(ids=None), "must not be NULL"),
                       (dict(face_tbn=ptr(mesh.face_tbn) + 8), "16-byte aligned"), (dict(phi=ptr(out["phi"]) + 4), "16-byte aligned"), (dict(P=(1 << 24) + 1), "patch frames")]:
        assert lib.nerftex_shape_light_lookup(*dict(base, **over).values(), stream()) == NERFTEX_ERR_INVALID
        assert text in lib.nerftex_last_error().decode(), (over, lib.nerftex_last_error().decode())
    assert lib.nerftex_shape_light_lookup(*dict(base, N=0).values(), stream()) == 0
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v == (7 if k == "mask" else -9 if k in ("face", "ids") else SENTINEL)).all()), f"{k}: nothing was launched"


# ---- 2. the chain -----------------------------------------------------------------------------------------------------------------------------------------

CONFIGS = [("eval", 1.0), ("eval", 0.7), ("train", 1.0)]


def _configure(field, mode, fc, visual="Full"):
    field.train(mode == "train")
    field.fc_weight, field.light_visual_mode = fc, visual


def _shape_lit_field(dev, map_hw=(24, 20), P=5, new_tbn="uv"):
    """The lit star-flower field with seeded maps imported and shape_float64's height field as the new mesh."""
    field = _lit_field(dev)
    phi_map, local_map, sample, ids_map = il64.seeded_light_maps(*map_hw, P)
    field.import_field(pf.seeded_map(*map_hw, seed=21), 1.0 / 32, phi_embed=phi_map, local_tbn=local_map, sample_tbn=sample, sample_tbn_ids=ids_map)
    v, f, vn, uvs = sf.mesh_of("height")
    field.import_shape(v, f, uvs, vertex_normals=vn, normalize=False, new_tbn=new_tbn)
    return field


def _chain_points(field, n, seed=5):
    """n points within 1.6 thresholds of the new mesh (both sides of the mask), row 0 exactly on a vertex (no normal), four consecutive rows sharing
    a direction."""
    rng = np.random.default_rng(seed)
    v, f, vn, _ = sf.mesh_of("height")
    shell = 1.6 * field.h_threshold * field._shape_scalars()[1]
    x = sf.sample_points(v, f, vn, n, rng, shell=shell, on_vertex=True)
    d = rng.normal(size=(n // 4, 3)).astype(np.float32)
    d = np.repeat(d / np.linalg.norm(d, axis=-1, keepdims=True), 4, axis=0)
    dev = field.sigma_net.weights.device
    return _t(x, dev), _t(d, dev)


def _marks(dev, n):
    marked = torch.zeros(n, dtype=torch.bool, device=dev)
    marked[::7] = True       # single slots
    marked[64:96] = True     # a whole 32-row step of an FFMLP wave
    marked[256:384] = True   # a whole 128-row workgroup
    marked[0] = False        # (row 0 is the row without a normal: it stays a live unmarked row)
    return marked


def _reference(field, x, d, mode, fc):
    """What forward() (the switch off) computes for the batch, and the float64 helper's shading normal with its bound from the plain lookup's
    outputs (forward()'s own inputs to the normal net and the rotations).  Computed once per configuration and shared."""
    _configure(field, mode, fc)
    assert not getattr(field, "fused_light_infer", False)
    handed = {}
    handle = field.light_net.register_forward_pre_hook(lambda m, a, k: handed.update(geo=a[0], n=a[1]), with_kwargs=True)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._shape_light_fused(x)
            _, _, h_mask, raw, face, xin, phi, _, local, smp, new = field._shape_light_lookup(x)
            sigma, color, _ = field(x, d)
            ones = torch.ones(x.shape[0], 1, dtype=handed["geo"].dtype, device=x.device)
            brdf = field.light_net.brdf_layer(torch.cat([handed["geo"], ones], dim=-1))
    finally:
        handle.remove()
    weights, biases, _, _ = nn64.pack(field.normal_net)
    has_normal = (raw != 0).any(-1)
    coarse = torch.where(has_normal[:, None], raw, torch.tensor([0.0, 0.0, 1.0], device=x.device)).cpu().numpy()  # (a row without a normal is masked out)
    ref = sl64.fine_normal(phi.half().cpu().numpy(), xin[:, :16].cpu().numpy(), xin[:, 16:28].cpu().numpy(), weights, biases, local.cpu().numpy(), smp.cpu().numpy(),
                           new.cpu().numpy(), coarse_raw=coarse, fc_weight=fc, blend=mode == "eval")
    assert sigma.dtype == torch.float32 and color.dtype == torch.float32
    return dict(sigma=sigma, color=color, mask=h_mask, brdf=brdf, normal_fwd=handed["n"].float(), normal=ref["normal"], bound_normal=ref["bound_normal"], new=new,
                has_normal=has_normal)


@pytest.fixture(scope="module")
def setup(dev):
    field = _shape_lit_field(dev)
    n = 1024
    x, d = _chain_points(field, n)
    marked = _marks(dev, n)
    xm, dm = x.clone(), d.clone()
    xm[marked] = 1e30
    dm[marked, 0] = 1e30
    refs = {cfg: _reference(field, x, d, *cfg) for cfg in CONFIGS}
    first = refs[CONFIGS[0]]
    inside = float(first["mask"].float().mean())
    assert 0.2 < inside < 0.8, inside  # both sides of the mask are exercised
    assert not bool(first["has_normal"][0]) and not bool(first["mask"][0]), "row 0 sits on a vertex"
    return dict(field=field, x=x, d=d, xm=xm, dm=dm, marked=marked, refs=refs)


def _call(field, x, d, live=None, want_normal=True):
    """nerftex_curved_light_shape_infer through the descriptor CurvedField builds, outputs pre-filled with the sentinel."""
    from nerftex_hip import check, lib, stream

    n, dev = x.shape[0], x.device
    sigma = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
    rgbs = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dev)
    normal = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dev) if want_normal else None
    scratch = torch.empty(lib.nerftex_curved_light_shape_infer_scratch_bytes(n), dtype=torch.uint8, device=dev)
    field.fused_light_infer = True
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert field._infer_light_shape_fused(x, d)
            desc, keep = field._infer_light_shape_desc(x, d, live, sigma, rgbs, scratch, normal)
            check(lib.nerftex_curved_light_shape_infer(ctypes.byref(desc), stream()))
        torch.cuda.synchronize()
    finally:
        field.fused_light_infer = False
    return sigma, rgbs, normal


# B = 1024: no unit; one workgroup; the whole batch through units of 64 rows; no device count at all
@pytest.mark.parametrize("units,rows_per_unit,want_live", [(0, 128, 0), (1, 128, 128), (16, 64, 1024), (None, 0, 1024)])
def test_rows_contract_at_the_c_abi(dev, setup, units, rows_per_unit, want_live):
    """Unmarked live rows: sigma and the mask are forward()'s, bit for bit, and the colour is shaded; marked live rows are exactly 0; rows >= live
    keep the sentinel in all three outputs; the row without a normal answers 0 through its mask."""
    field, ref = setup["field"], setup["refs"][("eval", 1.0)]
    _configure(field, "eval", 1.0)
    x, d, marked = setup["xm"], setup["dm"], setup["marked"]
    n = x.shape[0]
    live = None if units is None else (torch.tensor([units], dtype=torch.int32, device=dev), rows_per_unit)
    sigma, rgbs, normal = _call(field, x, d, live)
    rows = torch.arange(n, device=dev)
    alive, past = rows < want_live, rows >= want_live
    plain, unused = alive & ~marked, alive & marked
    mask = ref["mask"]
    assert torch.equal(sigma[plain], ref["sigma"][plain]), "sigma: forward()'s bits"
    assert torch.equal(((sigma != 0) | (rgbs != 0).any(-1))[plain & mask], torch.ones_like(mask)[plain & mask]) and not rgbs[plain & ~mask].any()
    assert not sigma[plain & ~mask].any()
    assert bool((sigma[unused] == 0).all()) and bool((rgbs[unused] == 0).all()) and bool((normal[unused] == 0).all())
    assert bool((sigma[past] == SENTINEL).all()) and bool((rgbs[past] == SENTINEL).all()) and bool((normal[past] == SENTINEL).all())
    if want_live:
        assert bool(unused.any()) and float(sigma[plain].max()) > 0 and float(rgbs[plain].max()) > 0
        assert float(sigma[0]) == 0 and not bool(rgbs[0].any()) and bool(torch.isfinite(normal[0]).all()), "the row without a normal"
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
    # the third rotation is there: without it the normal is the planar chain's, which lies outside the bound on most rows
    P = setup["refs"][(mode, fc)]
    assert float((normal - P["new"][:, 2]).abs().max(-1).values[torch.from_numpy(rows).to(dev)].median()) > 0.05
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
    entry = nerftex_hip.lib.nerftex_curved_light_shape_infer
    monkeypatch.setattr(nerftex_hip.lib, "nerftex_curved_light_shape_infer", lambda *args: (calls.append(1), entry(*args))[1])
    x, d = setup["x"], setup["d"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        want_s, want_c, _ = field(x, d)
        sigma, rgbs = field.infer(x, d)
        assert not calls and torch.equal(sigma, want_s.float()) and torch.equal(rgbs, want_c.float()), "the switch off: forward() on all rows"
        dens = field.density(x)
        assert torch.equal(dens["sigma"], want_s), "density() takes the unlit shape lookup for the lit field: forward()'s bits"
        fine, coarse, h_mask = field.fine_normal(x)
        assert torch.equal(h_mask, setup["refs"][("eval", 0.7)]["mask"]) and bool(torch.isfinite(fine[h_mask]).all())
        field.fused_light_infer = True
        try:
            sigma, rgbs = field.infer(x, d)
            assert len(calls) == 1 and torch.equal(sigma, want_s.float())
            odd_s, odd_c = field.infer_padded(x[:333].contiguous(), d[:333].contiguous())
            assert len(calls) == 2 and torch.equal(odd_s, sigma[:333]) and torch.equal(odd_c, rgbs[:333]), "a padded batch: the same bits per row"
        finally:
            field.fused_light_infer = False


def test_the_op_by_op_route_agrees_with_the_lookup(dev, setup):
    """`_shape_light_embed_reference` (what forward() runs without fp16 autocast) against the plain lookup: where the framework's normal has the
    kernel's bits, face, mask and new_tbn are the route's bit for bit, id and the sampled frames on all but the rows at a texel's edge; the fine
    normal of the route (fp32 rotations) inside the helper's fp32-inputs bound."""
    field = setup["field"]
    _configure(field, "eval", 1.0)
    x = setup["x"]
    with torch.no_grad():
        embed, coarse, w_mask, fine, w_uv, w_sdf, w_face, w_phi, w_local, w_ids, w_smp, w_new = field._shape_light_embed_reference(x, details=True)
        with torch.autocast("cuda", dtype=torch.float16):
            p_uv, sdf, mask, raw, face, xin, phi, ids, local, smp, new = field._shape_light_lookup(x)
    same = (raw == field._shape_embed_reference(x, details=True)[5]).all(-1)
    texel = same & (ids.long() == w_ids) & (local == w_local).all(-1).all(-1)
    print(f"op by op: the framework's normal has the kernel's bits on {float(same.float().mean()):.3f} of the rows, the nearest texel is the same on "
          f"{float(texel.float().sum() / same.float().sum()):.4f} of those")
    assert float(same.float().mean()) > 0.2
    assert torch.equal(face[same], w_face[same]) and torch.equal(mask[same], w_mask[same]) and torch.equal(new[same], w_new[same])
    # (p_uv is not bit-reproducible, DESIGN.md 4.16: a row whose ix or iy lies within an ulp of a half-integer may round to the neighbouring texel)
    assert float(texel.float().sum() / same.float().sum()) >= 0.99 and torch.equal(smp[texel], w_smp[texel])
    value, bound = pf.bilinear(field.phi_embed_imported.cpu().numpy(), p_uv[:, 0].cpu().numpy(), p_uv[:, 1].cpu().numpy())
    s = same.cpu().numpy()
    assert (np.abs(phi.double().cpu().numpy() - value) / bound)[s].max() <= 1.0
    weights, biases, dweights = il64.pack_fp32(copy.deepcopy(field.normal_net).cpu())
    ref = sl64.fine_normal(w_phi.cpu().numpy(), embed[:, :16].cpu().numpy(), embed[:, 16:28].cpu().numpy(), weights, biases, w_local.cpu().numpy(), w_smp.cpu().numpy(),
                           w_new.cpu().numpy(), fp32_inputs=True, dweights=dweights)
    rows = (w_mask & (w_face >= 0)).cpu().numpy()
    _inside("op-by-op fine normal (fp32)", fine.cpu().numpy()[rows], ref["fine"][rows], ref["bound_fine"][rows])


# ---- 3. the reference's own run -----------------------------------------------------------------------------------------------------------------------------

# u, v, the height and the coarse normal: DESIGN.md 4.16's bars for the same quantities of the same mesh and points; the shading normal, the
# colour and sigma: DESIGN.md 4.17's for the same chain behind them.  normal_fine takes 4.17's shading-normal bar (it is that normal at fc = 1).
BAR_UV, BAR_SDF, BAR_NORMAL, BAR_SHADING, BAR_COLOUR = 2e-6, 5e-8, 2e-6, 5e-3, 2e-2


@pytest.fixture(scope="module")
def golden_field(dev):
    load = lambda n: np.load(os.path.join(ROOT, "tests", "golden", n))  # noqa: E731
    g, gs, gl = load("ref_python_import_shape_sh.npz"), load("ref_python_import_shape.npz"), load("ref_python_import_field_sh.npz")
    field = _lit_field(dev, float(gl["h_threshold"]))
    il64.load_normal_net(field.normal_net, gl)
    with torch.no_grad():
        field.sigma_net.weights.copy_(torch.from_numpy(gl["w_sigma"]))
        field.light_net.brdf_layer.weights.copy_(torch.from_numpy(gl["w_brdf"]))
        field.light_net.envSHs.copy_(torch.from_numpy(gl["env_shs"]))
    il64.import_fixture_maps(field, gl, 1)
    field.import_shape(gs["vertices_raw"], gs["faces"], gs["uvs_raw"], vertex_normals=gs["vertex_normals"], new_tbn="uv")
    assert np.array_equal(field.shape_face_tbn[:, :9].cpu().numpy().reshape(-1, 3, 3), g["tbn"]), "the reference's own calculate_tbn, bit for bit"
    assert abs(field.sdf_scale_factor / float(gs["sdf_scale_factor"]) - 1) < 1e-6
    return field, g, gs


@pytest.mark.parametrize("key", ["S0", "S1", "S2"])
@pytest.mark.parametrize("route", ["fused", "forward", "op_by_op"])
def test_the_field_reproduces_the_reference_fixture(dev, golden_field, key, route):
    """fused: nerftex_curved_light_shape_infer; forward: forward() over the plain lookup; op_by_op: `_shape_light_embed_reference` in fp32 (no
    network behind it but the normal net).  Mask and face equal on every row (the fixture's mesh has no undecided row for these points: 4.16
    asserts the same mask equality); the rest inside the bars above."""
    field, g, gs = golden_field
    rate = float(gs[key + "_rate"])
    field.set_k_for_uv(int(gs[key + "_K"])), field.set_uv_utilize_rate(rate), field.set_sdf_factor(float(gs[key + "_sdf_factor"])), field.set_sdf_offset(float(gs[key + "_offset"]))
    x, d = torch.from_numpy(gs["xyz"]).to(dev), torch.from_numpy(gs["dirs"]).to(dev)
    hm, uvh = g[key + "_h_mask"], torch.from_numpy(g[key + "_uvh"]).to(dev)
    want_face = torch.from_numpy(g[key + "_face"]).to(dev).long()
    if route == "op_by_op":
        with torch.no_grad():
            embed, coarse, mask, fine, p_uv, sdf, face, phi, local, ids, smp, new = field._shape_light_embed_reference(x, details=True)
        lookup = None
    else:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            p_uv, sdf, mask, raw, face, xin, phi, ids, local, smp, new = field._shape_light_lookup(x)
            fine, coarse, _ = field.fine_normal(x)
    e_uv, e_sdf = float((p_uv - uvh[:, :2] * rate).abs().max()), float((sdf - uvh[:, 2]).abs().max())
    e_n = float((coarse.float() - torch.from_numpy(g[key + "_normal"]).to(dev)).abs().max())
    inside = torch.from_numpy(hm).to(dev)
    e_fine = float((fine.float() - torch.from_numpy(g[key + "_normal_fine"]).to(dev)).abs()[inside].max())
    who = f"{key} {route}"
    print(f"{who}: u, v error {e_uv:.3e} (bar {BAR_UV:.0e}), height error {e_sdf:.3e} (bar {BAR_SDF:.0e}), coarse normal error {e_n:.3e} (bar {BAR_NORMAL:.0e}), "
          f"normal_fine error {e_fine:.3e} (bar {BAR_SHADING:.0e})")
    assert torch.equal(mask, inside) and torch.equal(face, want_face)
    assert torch.equal(ids.long().cpu(), torch.from_numpy(g[key + "_id"]).long()), "the nearest texel: no row of the fixture sits at a texel's edge"
    assert np.array_equal(local.reshape(-1, 3, 3).cpu().numpy(), g[key + "_local_tbn"])
    # (the patch frames are inverted on the host by LAPACK, whose last bits follow the machine: the field's own rows exactly, the fixture's closely)
    assert torch.equal(smp.reshape(-1, 3, 3), field.sample_tbn_inv_imported[ids.long()]) and np.abs(smp.reshape(-1, 3, 3).cpu().numpy() - g[key + "_sample_tbn_inv"]).max() <= 1e-5
    assert np.array_equal(new.reshape(-1, 3, 3).cpu().numpy(), g[key + "_new_tbn"])
    assert e_uv <= BAR_UV and e_sdf <= BAR_SDF and e_n <= BAR_NORMAL and e_fine <= BAR_SHADING
    assert float((phi.float().cpu() - torch.from_numpy(g[key + "_phi"])).abs().max()) <= 1e-5
    if route == "op_by_op":
        return
    field.eval()
    handed = {}
    handle = field.light_net.register_forward_pre_hook(lambda m, a, k: handed.update(n=a[1]), with_kwargs=True)
    try:
        for fc in (1.0, 0.7):
            for visual in ("Full", "Specular", "Diffuse", "Albedo"):
                _configure(field, "eval", fc, visual)
                if route == "fused":
                    sigma, rgbs, normal = _call(field, x, d)
                else:
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                        sigma, rgbs, _ = field(x, d)
                    sigma, rgbs, normal = sigma.float(), rgbs.float(), handed["n"].float()
                err = np.abs(rgbs.cpu().numpy() - g[f"{key}_fc{fc}_color_{visual.lower()}"].astype(np.float32))
                nerr = np.abs(normal.cpu().numpy() - g[f"{key}_fc{fc}_shading_normal"])[hm]
                shaded = ((sigma != 0) | (rgbs != 0).any(-1)).cpu().numpy()
                print(f"{who} fc={fc} {visual}: colour max |diff| {float(err.max()):.2e}, shading normal max |diff| {float(nerr.max()):.2e}, {int(hm.sum())} rows inside the mask")
                assert np.array_equal(shaded, hm)
                assert err.max() <= BAR_COLOUR and nerr.max() <= BAR_SHADING
                np.testing.assert_allclose(sigma.cpu().numpy(), g[key + "_sigma"], rtol=3e-2, atol=3e-3)
    finally:
        handle.remove()
        field.light_visual_mode = "Full"


# ---- 4. a frame -------------------------------------------------------------------------------------------------------------------------------------------

def test_a_frame_of_the_lit_maps_on_the_height_field(dev, monkeypatch):
    """32 x 32 through render_infer, render_infer_pipelined and render_infer_graphed with `fused_light_infer` on, behind initialize_states(): one
    image; another pose replays the graphs; other frames re-record them and change the image but not the depth; switch_shape_feature() gives the
    planar lit frame, switch_import() the mesh field's bit for bit."""
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
    loops = dict(slots_per_ray=4, **KW)
    r_mesh = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        r_mesh.update_extra_state_device()
        mesh_ref = r_mesh.render_infer(*frames[0], **loops)[:2]
    mesh_stamp = field.graph_stamp()
    calls = []
    entry = nerftex_hip.lib.nerftex_curved_light_shape_infer
    monkeypatch.setattr(nerftex_hip.lib, "nerftex_curved_light_shape_infer", lambda *a: (calls.append(1), entry(*a))[1])
    H = W = 64
    maps = dict(zip(("phi_embed", "local_tbn", "sample_tbn", "sample_tbn_ids"), il64.seeded_light_maps(H, W, 5)))
    field.import_field(pf.seeded_map(H, W, seed=21), 1.0 / 64, **maps)
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_python_import_shape.npz"))
    mesh = (g["vertices_raw"], g["faces"], g["uvs_raw"])
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            r_planar = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
            r_planar.initialize_states(2)
            planar_ref = r_planar.render_infer(*frames[0], **loops)[:2]
        field.import_shape(*mesh, vertex_normals=g["vertex_normals"], new_tbn="uv")
        assert field.graph_stamp()[:len(mesh_stamp)] == mesh_stamp and "import-shape" in field.graph_stamp()
        r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)  # (a grid of its own: initialize_states keeps a maximum)
        r.initialize_states(2)
        assert int((r.density_grid[0] > 0).sum()) > 0 and int((r.density_grid[0] == 0).sum()) > 0
        with torch.autocast("cuda", dtype=torch.float16):
            img, dep, _ = r.render_infer(*frames[0], **loops)
            assert calls, "the reference loop goes through the fused chain"
            img_p, dep_p, _ = r.render_infer_pipelined(*frames[0], parts=2, **loops)
            img_g, dep_g, _ = r.render_infer_graphed(*frames[0], parts=2, block=2, **loops)
            assert torch.equal(img_p, img) and torch.equal(dep_p, dep) and torch.equal(img_g, img) and torch.equal(dep_g, dep), "the three loops give one image"
            assert float(img.std()) > 1e-3 and not torch.equal(img, mesh_ref[0]) and not torch.equal(img, planar_ref[0])
            graphs = r._infer_graphs
            img_2, dep_2, _ = r.render_infer_graphed(*frames[1], parts=2, block=2, **loops)
            assert r._infer_graphs is graphs, "another pose replays the recorded graphs"
            want_2 = r.render_infer(*frames[1], **loops)
            assert torch.equal(img_2, want_2[0]) and torch.equal(dep_2, want_2[1])
            # other frames of the new mesh (an array, taken as given): the graphs are re-recorded, the image changes, the depth does not
            F = len(g["faces"])
            turned = np.tile(np.float32([[0, 1, 0], [0, 0, 1], [1, 0, 0]]), (F, 1, 1))
            field.import_shape(*mesh, vertex_normals=g["vertex_normals"], new_tbn=turned)
            img_o, dep_o, _ = r.render_infer_graphed(*frames[0], parts=2, block=2, **loops)
            assert r._infer_graphs is not graphs, "other frames re-record the graphs"
            want = r.render_infer(*frames[0], **loops)
            assert torch.equal(img_o, want[0]) and torch.equal(dep_o, want[1]) and not torch.equal(img_o, img)
            assert torch.equal(dep_o, dep), "the density does not read the frames"
            # the planar map behind the renderer that holds its occupancy grid: DESIGN.md 4.17's frame, bit for bit
            field.switch_shape_feature()
            assert field.imported_type == "field"
            n_calls = len(calls)
            img_f, dep_f, _ = r_planar.render_infer(*frames[0], **loops)
            assert torch.equal(img_f, planar_ref[0]) and torch.equal(dep_f, planar_ref[1]) and len(calls) == n_calls
            # back to the mesh field
            field.switch_import()
            assert not field.imported and field.graph_stamp() == mesh_stamp
            img_m, dep_m, _ = r_mesh.render_infer(*frames[0], **loops)
            assert torch.equal(img_m, mesh_ref[0]) and torch.equal(dep_m, mesh_ref[1]) and len(calls) == n_calls
    finally:
        field.fused_light_infer = False
