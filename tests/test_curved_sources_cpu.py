"""CurvedField's imported sources on the CPU side (no GPU): what `_import_stamp()` pins of each of them -- a recorded graph's validity hangs on it --
and which of the eight `_infer_*_fused` predicates (and of the lit back half they share) hold one deviation away from the default state.  Both are pinned against literal data: the stamp
against a tuple written out here from the field's attributes, the predicates against the table the commit before the sources got their one lookup
produced for these very fields (EXPECTED: recorded there once, never recomputed from the code under test)."""
import types

import pytest
import torch

from test_curved_infer_members_cpu import _field

MAPS = ("phi_embed_imported", "local_tbn_imported", "sample_tbn_inv_imported", "sample_tbn_ids_imported", "frame_map_imported", "sample_inv_rows_imported")
STATES = {"planar": (False, "field"), "shape": (False, "shape"), "lit planar": (True, "field"), "lit shape": (True, "shape"), "patch": (False, "patch"),
          "lit patch": (True, "patch")}


def _written_out(f, lit, kind):
    """(the stamp, the tensors in it as (owner, attribute)) of the bare field `f`, from its attributes."""
    from nerftex_hip import PLANAR_DIVIDE

    ft, version = f.features_imported, f._import_version
    maps = [(f, m) for m in MAPS] if lit else []
    if kind == "patch":
        stamp = ("import-patch", ft.data_ptr(), tuple(ft.shape), 13, f.patch_geom.data_ptr(), f.patch_lit.data_ptr() if lit else None, 0.0625, version)
        return stamp, [(f, "features_imported"), (f, "patch_geom")] + ([(f, "patch_lit")] if lit else [])
    if kind == "shape":
        p = f.shape_projector
        maps += [(f, "shape_face_tbn")] if lit else []
        stamp = ("import-shape", ft.data_ptr(), tuple(ft.shape), 11, 12, p.mesh_vertices.data_ptr(), p.vertex_normals.data_ptr(), f.shape_face_uv.data_ptr(),
                 5, 1.0, 0.0, 1.0, 0.0625, version)  # (K_for_uv, sdf_scale_factor / uv_utilize_rate, sdf_offset, uv_utilize_rate, h_threshold)
        tensors = [(f, "features_imported"), (p, "mesh_vertices"), (p, "vertex_normals"), (f, "shape_face_uv")]
    else:
        stamp = ("import", ft.data_ptr(), tuple(ft.shape), PLANAR_DIVIDE, 0.5, 0.5, 1.0, 1.0, 0.0, 0.0625, version)  # (not rescaled: the bounds divide)
        tensors = [(f, "features_imported")]
    return stamp + tuple((getattr(o, m).data_ptr(), tuple(getattr(o, m).shape)) for o, m in maps), tensors + maps


@pytest.mark.parametrize("state", STATES)
def test_the_import_stamp_is_the_tuple_written_out_and_follows_every_tensor_in_it(state):
    lit, kind = STATES[state]
    f = _field(lit, kind)
    f._import_version = 3
    want, tensors = _written_out(f, lit, kind)
    stamp = f._import_stamp()
    assert stamp == want and len(stamp) == len(want)
    assert f.graph_stamp()[-len(stamp):] == stamp
    for owner, name in tensors:
        old = getattr(owner, name)
        setattr(owner, name, old.clone())
        assert f._import_stamp() != stamp, name
        setattr(owner, name, old)
        assert f._import_stamp() == stamp
    f._import_version += 1
    assert f._import_stamp() != stamp and f._import_stamp() == _written_out(f, lit, kind)[0]
    f.imported = False
    assert f._import_stamp() == ()


# ---- the predicate table ---------------------------------------------------------------------------------------------------------------------------------

PREDICATES = ("_infer_fused", "_infer_import_fused", "_infer_light_fused", "_infer_light_import_fused", "_infer_light_shape_fused", "_infer_patch_fused",
              "_infer_light_patch_fused", "_infer_front_fused", "_infer_light_back_fused")
FIELDS = {"mesh": (False, None), "lit mesh": (True, None), **STATES}


def _lip(*shapes):
    return types.SimpleNamespace(layers=[types.SimpleNamespace(W=torch.zeros(*s)) for s in shapes])


def _default(lit, kind):
    """The bare field in the state every chain that fits it serves: the default shapes, both switches on."""
    f = _field(lit, kind)
    f.in_dim, f.in_pad, f.geo_feat_dim, f.color_pad, f.encoder_dir = 41, 48, 15, 32, types.SimpleNamespace(output_dim=16)
    f.fused_glue = f.fused_light_infer = True
    if lit:
        f.light_visual_mode = "Full"
        nn = f.normal_net
        nn.bound_output, nn.low_freq_band_len_x, nn.low_freq_band_len_z = False, 16, 12
        nn.phi_net, nn.theta_net = _lip((16, 20), (16, 16), (1, 16)), _lip((16, 28), (16, 16), (1, 16))
    return f


def _batch(B=128):
    """A stand-in for a contiguous fp32 [B, 3] device tensor that lives where the bare field's CPU tensors do."""
    return types.SimpleNamespace(shape=(B, 3), dtype=torch.float32, is_cuda=True, device=torch.device("cpu"), is_contiguous=lambda: True)


def _elsewhere(t):
    return None if t is None else types.SimpleNamespace(device=torch.device("meta"), shape=tuple(t.shape), data_ptr=t.data_ptr)


def _lit_records_elsewhere(f):
    f.phi_embed_imported, f.patch_lit = _elsewhere(f.phi_embed_imported), _elsewhere(f.patch_lit)


def _no_lit_records(f):
    f.phi_embed_imported = f.patch_lit = None


DEVIATIONS = {  # one term away from the default state each: name -> what it does to the field (the two that are the call's are handled below)
    "default": lambda f: None,
    "autocast off": lambda f: None,
    "multires = 10": lambda f: setattr(f, "multires", 10),
    "encoder_var set": lambda f: setattr(f, "encoder_var", object()),
    "sigma_net.dtype float32": lambda f: setattr(f.sigma_net, "dtype", torch.float32),
    "fused_glue = False": lambda f: setattr(f, "fused_glue", False),
    "features on another device": lambda f: setattr(f, "features_imported", _elsewhere(f.features_imported)),
    "lit records on another device": _lit_records_elsewhere,
    "B = 100": lambda f: None,
    "lit records absent": _no_lit_records,
    "shape_face_tbn absent": lambda f: setattr(f, "shape_face_tbn", None),
    "fused_light_infer off": lambda f: setattr(f, "fused_light_infer", False),
}


def _short(predicate):
    return predicate[len("_infer_"):-len("_fused")] or "mesh"


def predicates_that_hold(field, deviation):
    """The names of the predicates that hold (without their `_infer_` and `_fused`; `_infer_fused`: mesh), `name!Error` for one that raises."""
    f = _default(*FIELDS[field])
    DEVIATIONS[deviation](f)
    x = d = _batch(100 if deviation == "B = 100" else 128)
    was = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    torch.set_autocast_enabled("cuda", deviation != "autocast off")
    torch.set_autocast_dtype("cuda", torch.float16)
    try:
        out = []
        for p in PREDICATES:
            try:
                if getattr(f, p)(*((x,) if p == "_infer_light_back_fused" else (x, d))):
                    out.append(_short(p))
            except Exception as e:  # noqa: BLE001  (a predicate asked about a state it is never asked about: recorded, and pinned like any other cell)
                out.append(f"{_short(p)}!{type(e).__name__}")
        return " ".join(out)
    finally:
        torch.set_autocast_enabled("cuda", was[0])
        torch.set_autocast_dtype("cuda", was[1])


EXPECTED = {
    'mesh': {'default': 'mesh import!AttributeError front',
             'autocast off': '',
             'multires = 10': '',
             'encoder_var set': '',
             'sigma_net.dtype float32': '',
             'fused_glue = False': 'front',
             'features on another device': 'mesh import!AttributeError front',
             'lit records on another device': 'mesh import!AttributeError front',
             'B = 100': '',
             'lit records absent': 'mesh import!AttributeError front',
             'shape_face_tbn absent': 'mesh import!AttributeError front',
             'fused_light_infer off': 'mesh import!AttributeError front'},
    'lit mesh': {'default': 'light front light_back',
                 'autocast off': 'light_back',
                 'multires = 10': 'light_back',
                 'encoder_var set': 'light_back',
                 'sigma_net.dtype float32': 'light_back',
                 'fused_glue = False': 'light front light_back',
                 'features on another device': 'light front light_back',
                 'lit records on another device': 'light front light_back',
                 'B = 100': 'light_back',
                 'lit records absent': 'light front light_back',
                 'shape_face_tbn absent': 'light front light_back',
                 'fused_light_infer off': 'front'},
    'planar': {'default': 'mesh import front',
               'autocast off': '',
               'multires = 10': '',
               'encoder_var set': '',
               'sigma_net.dtype float32': '',
               'fused_glue = False': 'front',
               'features on another device': 'mesh front',
               'lit records on another device': 'mesh import front',
               'B = 100': '',
               'lit records absent': 'mesh import front',
               'shape_face_tbn absent': 'mesh import front',
               'fused_light_infer off': 'mesh import front'},
    'shape': {'default': 'mesh import front',
              'autocast off': '',
              'multires = 10': '',
              'encoder_var set': '',
              'sigma_net.dtype float32': '',
              'fused_glue = False': 'front',
              'features on another device': 'mesh front',
              'lit records on another device': 'mesh import front',
              'B = 100': '',
              'lit records absent': 'mesh import front',
              'shape_face_tbn absent': 'mesh import front',
              'fused_light_infer off': 'mesh import front'},
    'lit planar': {'default': 'light light_import front light_back',
                   'autocast off': 'light_back',
                   'multires = 10': 'light_back',
                   'encoder_var set': 'light_back',
                   'sigma_net.dtype float32': 'light_back',
                   'fused_glue = False': 'light light_import front light_back',
                   'features on another device': 'light front light_back',
                   'lit records on another device': 'light front light_back',
                   'B = 100': 'light_back',
                   'lit records absent': 'light front light_back',
                   'shape_face_tbn absent': 'light light_import front light_back',
                   'fused_light_infer off': 'front'},
    'lit shape': {'default': 'light light_shape front light_back',
                  'autocast off': 'light_back',
                  'multires = 10': 'light_back',
                  'encoder_var set': 'light_back',
                  'sigma_net.dtype float32': 'light_back',
                  'fused_glue = False': 'light light_shape front light_back',
                  'features on another device': 'light front light_back',
                  'lit records on another device': 'light front light_back',
                  'B = 100': 'light_back',
                  'lit records absent': 'light front light_back',
                  'shape_face_tbn absent': 'light front light_back',
                  'fused_light_infer off': 'front'},
    'patch': {'default': 'mesh import patch front',
              'autocast off': '',
              'multires = 10': '',
              'encoder_var set': '',
              'sigma_net.dtype float32': '',
              'fused_glue = False': 'front',
              'features on another device': 'mesh front',
              'lit records on another device': 'mesh import patch front',
              'B = 100': '',
              'lit records absent': 'mesh import patch front',
              'shape_face_tbn absent': 'mesh import patch front',
              'fused_light_infer off': 'mesh import patch front'},
    'lit patch': {'default': 'light light_patch front light_back',
                  'autocast off': 'light_back',
                  'multires = 10': 'light_back',
                  'encoder_var set': 'light_back',
                  'sigma_net.dtype float32': 'light_back',
                  'fused_glue = False': 'light light_patch front light_back',
                  'features on another device': 'light front light_back',
                  'lit records on another device': 'light front light_back',
                  'B = 100': 'light_back',
                  'lit records absent': 'light front light_back',
                  'shape_face_tbn absent': 'light light_patch front light_back',
                  'fused_light_infer off': 'front'},
}


@pytest.mark.parametrize("field", FIELDS)
def test_the_infer_predicates_hold_where_they_held(field):
    assert set(EXPECTED[field]) == set(DEVIATIONS)
    got = {deviation: predicates_that_hold(field, deviation) for deviation in DEVIATIONS}
    assert got == EXPECTED[field], {k: (got[k], EXPECTED[field][k]) for k in got if got[k] != EXPECTED[field][k]}
