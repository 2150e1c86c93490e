"""The eight curved-field inference descriptors as compositions of member blocks (ngp_harness/curved.py), the CPU side (no GPU): every builder
passes exactly the members its ctypes structure declares -- a member no block names would be the NULL / 0 ctypes fills in, which only a GPU run
finds; a member two blocks name is a TypeError where they are composed -- and the one route picks the chain both infer() and infer_padded() take."""
import types

import pytest
import torch

DESCS = {  # the descriptor's class -> its builder, whether the field is lit, what is imported: a map onto a new mesh ("shape"), planar ("field"), a "patch", nothing
    "CurvedInferDesc": ("_infer_desc", False, None),
    "CurvedImportInferDesc": ("_infer_import_desc", False, "field"),
    "CurvedShapeInferDesc": ("_infer_shape_desc", False, "shape"),
    "CurvedLightInferDesc": ("_infer_light_desc", True, None),
    "CurvedLightImportInferDesc": ("_infer_light_import_desc", True, "field"),
    "CurvedLightShapeInferDesc": ("_infer_light_shape_desc", True, "shape"),
    "CurvedPatchInferDesc": ("_infer_patch_desc", False, "patch"),
    "CurvedLightPatchInferDesc": ("_infer_light_patch_desc", True, "patch"),
}


def _net(i, h, n, o):
    return types.SimpleNamespace(input_dim=i, hidden_dim=h, num_layers=n, output_dim=o, padded_output_dim=o, dtype=torch.float16)


def _projector(n_verts=7):
    return types.SimpleNamespace(_knn=types.SimpleNamespace(value=11), tracer=types.SimpleNamespace(_handle=types.SimpleNamespace(value=12)),
                                 mesh_vertices=torch.zeros(n_verts, 3), vertex_normals=torch.zeros(n_verts, 3), tbn=torch.zeros(4, 3, 3), K=8,
                                 _height_limit=lambda *a: 0.0625)


def _encoder(levels):
    table = torch.zeros(64, 2, dtype=torch.float16)
    return types.SimpleNamespace(_table=lambda: table, offsets=torch.zeros(levels + 1, dtype=torch.int32), input_dim=3, level_dim=2, num_levels=levels,
                                 per_level_scale=2.0, base_resolution=16, gridtype_id=0, align_corners=False, output_dim=2 * levels)


def _field(lit, imported):
    """tests/test_import_shape_light_cpu.py's bare field with stand-ins for everything a descriptor points into: CPU tensors, whose addresses are
    never dereferenced here."""
    from ngp_harness.curved import CurvedField

    f = object.__new__(CurvedField)
    torch.nn.Module.__init__(f)
    f.light_model, f.multires, f.h_threshold, f.fc_weight, f.bound, f.encoder_var = ("SH" if lit else None), 12, 0.0625, 0.7, 1.0, None
    f.encoder, f.projector, f.sigma_net, f.color_net = _encoder(8), _projector(), _net(48, 32, 2, 16), _net(32, 64, 3, 3)
    f.normal_net = types.SimpleNamespace(encoder=_encoder(4)) if lit else None
    f.light_net = types.SimpleNamespace(brdf_layer=_net(16, 64, 3, 5), envSHs=torch.zeros(9, 3), gamma=2.4, use_specular=True, fused=True) if lit else None
    f.light_visual_mode = "Diffuse"
    half, single = torch.zeros(8, dtype=torch.float16), torch.zeros(8)
    f._infer_weights = lambda *a, **k: (half, half)  # (the cached 16-bit copies: `_infer_weights` asks the library to register the offsets)
    f._infer_light_weights = lambda: (half, half, half, single)
    f._init_import_state()
    if imported == "patch":
        f.imported, f.imported_type = True, imported
        f.features_imported, f.patch_geom, f._patch_knn = torch.zeros(8, 16), torch.zeros(8, 8), types.SimpleNamespace(value=13)
        if lit:
            f.patch_lit, f.patch_phi_embed = torch.zeros(8, 20), torch.zeros(8, 8)
    elif imported:
        f.imported, f.imported_type, f.bounds = True, imported, (0.5, 0.5)
        f.features_imported = torch.zeros(2, 3, 16)
        f.phi_embed_imported, f.frame_map_imported, f.sample_inv_rows_imported = torch.zeros(2, 3, 8), torch.zeros(2, 3, 12), torch.zeros(5, 12)
        f.local_tbn_imported, f.sample_tbn_ids_imported, f.sample_tbn_inv_imported = torch.zeros(2, 3, 9), torch.zeros(2, 3), torch.zeros(5, 3, 3)
        f.shape_projector, f.shape_face_uv, f.shape_face_tbn = _projector(9), torch.zeros(10, 8), torch.zeros(10, 12)
    return f.eval()


def _members(monkeypatch, name, live=None, **kw):
    """The keyword arguments the builder of descriptor `name` passes to it, and the structure's declared members."""
    import nerftex_hip
    from ngp_harness import curved

    builder, lit, imported = DESCS[name]
    monkeypatch.setattr(curved, name, lambda **members: members)
    f = _field(lit, imported)
    B = 128
    x, d, out, scratch = torch.zeros(B, 3), torch.zeros(B, 3), torch.zeros(4 * B), torch.zeros(256, dtype=torch.uint8)
    passed, keep = getattr(f, builder)(x, d, live, out[:B], out[B:].view(B, 3), scratch, **kw)
    return passed, keep, [n for n, _ in getattr(nerftex_hip, name)._fields_], f


@pytest.mark.parametrize("name", DESCS)
def test_a_builder_passes_every_member_of_its_descriptor_and_nothing_else(monkeypatch, name):
    passed, keep, fields, f = _members(monkeypatch, name)
    assert len(set(fields)) == len(fields)
    assert set(passed) == set(fields), (sorted(set(fields) - set(passed)), sorted(set(passed) - set(fields)))
    # ... and none of them with the value ctypes would have filled in, but for the two a call without a device count leaves at NULL / 0
    # (and the lit chains' optional output)
    empty = {n for n, v in passed.items() if v is None or (v == 0 and not isinstance(v, float))}
    assert empty <= {"units_dev", "rows_per_unit", "shading_normal", "gridtype", "align_corners", "normal_gridtype", "normal_align_corners"}, empty
    # the real structure takes them, and the tensors kept alive are the ones it points into
    import nerftex_hip

    desc = getattr(nerftex_hip, name)(**passed)
    held = {t.data_ptr() for t in keep if torch.is_tensor(t)}
    pointers = [n for n in ("table", "normal_table", "map", "phi_map", "frame_map", "sample_tbn_inv", "sigma_weights", "color_weights", "brdf_weights",
                            "normal_weights", "normal_biases", "env_shs", "geom", "features", "lit") if n in passed]
    assert pointers and all(getattr(desc, n) in held for n in pointers), [n for n in pointers if getattr(desc, n) not in held]
    if DESCS[name][2] == "patch":  # the neighbour grid is the patch's own, kept alive with the records
        assert passed["knn"] == 13 and f._patch_knn in keep and {"geom", "features"} <= set(pointers) and ("lit" in pointers) == DESCS[name][1]
    assert desc.B == 128 and desc.eval == (1 if DESCS[name][1] else 3) and desc.fc_weight == pytest.approx(0.7)


def test_the_device_count_the_training_rule_and_the_shading_normal_reach_the_members(monkeypatch):
    units, normal = torch.zeros(1, dtype=torch.int32), torch.zeros(128, 3)
    passed, _, _, _ = _members(monkeypatch, "CurvedLightShapeInferDesc", live=(units, 128), shading_normal=normal)
    assert (passed["units_dev"], passed["rows_per_unit"], passed["shading_normal"]) == (units.data_ptr(), 128, normal.data_ptr())
    assert passed["visual_mode"] == 2 and passed["eval"] == 1 and passed["K"] == 5 and passed["n_verts"] == 9  # "Diffuse"; the imported mesh, K_for_uv
    # in training the head shows "Full" whatever the visual mode says, and the static chains keep bit 1 of eval
    from ngp_harness import curved

    f = _field(True, "field").train()
    back, _ = f._infer_lit_back(torch.zeros(128, 3), torch.zeros(128, 3), None, torch.zeros(128), torch.zeros(128, 3), torch.zeros(256, dtype=torch.uint8), None)
    assert back["visual_mode"] == 0 and back["eval"] == 0
    g = _field(False, None).train()
    back, _ = g._infer_static_back(torch.zeros(128, 3), torch.zeros(128, 3), None, torch.zeros(128), torch.zeros(128, 3), torch.zeros(256, dtype=torch.uint8))
    assert back["eval"] == 2 and curved.CurvedField._SIGMA_NET == (48, 32, 2, 16)


def test_composing_two_blocks_that_name_the_same_member_raises():
    f = _field(True, "shape")
    rows = (torch.zeros(128, 3), torch.zeros(128, 3), None, torch.zeros(128), torch.zeros(128, 3), torch.zeros(256, dtype=torch.uint8))
    front, _ = f._infer_front_desc()
    patch = _field(True, "patch")._infer_patch()
    for a, b, twice in [(front, f._infer_shape(), "knn"),  # two meshes
                        (patch, f._infer_shape(), "knn"),  # a patch and a mesh
                        (f._infer_planar(), f._infer_shape(), "map"),  # two lookups of the one map
                        (f._infer_static_back(*rows)[0], f._infer_lit_back(*rows, None)[0], "sigma_weights")]:  # two light models
        assert twice in a and twice in b
        with pytest.raises(TypeError, match="multiple values for keyword argument"):
            dict(**a, **b)


def test_one_route_serves_infer_and_infer_padded(monkeypatch):
    """The table, once: lit patch, patch; lit shape, lit import, shape, import; lit mesh, mesh; forward().  infer() takes whatever the route names;
    infer_padded() pads for the lit chains alone and leaves every other batch to infer()."""
    from ngp_harness.curved import CurvedField

    rungs = ["_infer_light_patch_fused", "_infer_patch_fused", "_infer_light_shape_fused", "_infer_light_import_fused", "_infer_import_fused",
             "_infer_light_fused", "_infer_fused"]

    def field(imported, shape, *true):
        f = _field(True, (shape if isinstance(shape, str) else "shape" if shape else "field") if imported else None)
        for r in rungs:
            setattr(f, r, lambda x, d, on=r in true: on)
        return f

    x = d = torch.zeros(128, 3)
    entry = lambda f: (lambda r: None if r is None else (r[0], r[1].__name__))(f._infer_route(x, d))  # noqa: E731
    assert entry(field(True, "patch", *rungs)) == ("nerftex_curved_light_patch_infer", "_infer_light_patch_desc")
    assert entry(field(True, "patch", *rungs[1:])) == ("nerftex_curved_patch_infer", "_infer_patch_desc")
    assert entry(field(True, "patch", *rungs[2:])) is None, "an imported patch never takes a map's chains, nor the mesh field's"
    assert entry(field(True, True, *rungs)) == ("nerftex_curved_light_shape_infer", "_infer_light_shape_desc")
    assert entry(field(True, True, *rungs[3:])) == ("nerftex_curved_light_import_infer", "_infer_light_import_desc")
    assert entry(field(True, True, *rungs[4:])) == ("nerftex_curved_shape_infer", "_infer_shape_desc")
    assert entry(field(True, False, *rungs[4:])) == ("nerftex_curved_import_infer", "_infer_import_desc")
    assert entry(field(True, False, *rungs[5:])) is None, "an imported map never takes the mesh field's chains"
    assert entry(field(False, False, *rungs)) == ("nerftex_curved_light_infer", "_infer_light_desc")
    assert entry(field(False, False, "_infer_fused")) == ("nerftex_curved_field_infer", "_infer_desc")
    assert entry(field(False, False)) is None

    calls = []

    def call(self, entry, make_desc, x, d, live, *more):
        calls.append((entry, x.shape[0], live))
        return torch.zeros(x.shape[0]), torch.zeros(x.shape[0], 3)

    def forward(self, x, d):
        calls.append(("forward", x.shape[0], None))
        return torch.zeros(x.shape[0]), torch.zeros(x.shape[0], 3), {}

    monkeypatch.setattr(CurvedField, "_infer_call", call)
    monkeypatch.setattr(CurvedField, "forward", forward)
    odd = torch.zeros(100, 3)
    f = field(True, False, "_infer_light_import_fused")
    f.fused_light_infer = True
    sigma, rgbs = f.infer_padded(odd, odd)
    assert calls == [("nerftex_curved_light_import_infer", 128, None)] and sigma.shape == (100,) and rgbs.shape == (100, 3)
    calls.clear()
    f.infer(x, d, live="live")
    f.fused_light_infer = False  # the switch is off: no padding, infer() on the batch as it is
    f.infer_padded(odd, odd)
    g = field(True, False, "_infer_import_fused")  # a static chain is not padded for
    g.fused_light_infer = True
    g.infer_padded(odd, odd)
    h = field(False, False)
    h.infer(x, d)
    assert calls == [("nerftex_curved_light_import_infer", 128, "live"), ("nerftex_curved_light_import_infer", 100, None), ("nerftex_curved_import_infer", 100, None),
                     ("forward", 128, None)]
