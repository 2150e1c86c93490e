"""An imported texture on a new UV-mapped mesh under the SH-lit curved field, the CPU side (no GPU): `uv_face_frames` against the float64
statement of tests/shape_light_float64.py, the helper's third rotation against an emulation of the half product and against its mutants,
CurvedField.import_shape(new_tbn=...)'s refusals, the state a refused call leaves, the graph stamp, and the C ABI's declarations."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import import_light_float64 as il64
import normal_net_float64 as nn64
import planar_float64 as pf
import shape_float64 as sf
import shape_light_float64 as sl64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
NERFTEX_ERR_INVALID = 1


def _bare_field(lit=True):
    """tests/test_import_light_cpu.py's field without mesh structures and MLPs: the import state reads none of them."""
    from ngp_harness.curved import CurvedField, FactorizedNormalNet

    f = object.__new__(CurvedField)
    torch.nn.Module.__init__(f)
    f.light_model, f.multires, f.h_threshold, f.in_dim, f.fc_weight = ("SH" if lit else None), 12, 0.0625, 41, 1.0
    f.encoder = types.SimpleNamespace(output_dim=16)
    f.sigma_net = types.SimpleNamespace(weights=torch.zeros(1), dtype=torch.float16)
    f.projector = types.SimpleNamespace(h_threshold=0.0625)
    f.normal_net = FactorizedNormalNet(x_dim=16, z_dim=25) if lit else None
    f.light_visual_mode, f.smooth_grad_weight, f.encoder_var = "Full", 1e-1, None
    f._init_import_state()
    return f.eval()


def _maps(H=2, W=3, P=3):
    phi, local, sample, ids = il64.seeded_light_maps(H, W, P)
    return dict(phi_embed=phi, local_tbn=local, sample_tbn=sample, sample_tbn_ids=ids)


# ---- the per-face frames ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["quad", "height", "star"])
def test_uv_face_frames_against_the_float64_statement(name):
    """The bar is shape_light_float64.frames_bar's: fp32 rounding of a float64 result (2^-24 on a component of a unit row) plus the fp32
    inverse's error, 16 roundings times the condition number of the face's UV edge matrix (the UVs the reference hands over are fp32)."""
    from ngp_harness.curved import shape_preprocess, uv_face_frames

    v, f, _, uvs = sf.mesh_of(name)
    vp, uvp, face_uv, _ = shape_preprocess(v, f, uvs, normalize=True)
    got = uv_face_frames(vp, f, uvp)
    assert got.dtype == np.float32 and got.shape == (len(f), 3, 3)
    want, bar = sl64.uv_face_frames(vp, f, uvp), sl64.frames_bar(vp, f, uvp)
    err = np.abs(got - want).max((1, 2))
    print(f"{name}: {len(f)} faces, largest error / bar {float((err / bar).max()):.3f}, largest error {float(err.max()):.3e}, largest bar {float(bar.max()):.3e}")
    assert (err <= bar).all()
    # orthonormal rows with the face normal last, right-handed: b = n x t
    eye = np.einsum("fab,fcb->fac", want, want)
    assert np.abs(eye - np.eye(3)).max() < 1e-12 and np.abs(np.cross(want[:, 2], want[:, 0]) - want[:, 1]).max() < 1e-12
    # float64 UVs in: the inverse is numpy's float64 one, and the result the statement's rounded to fp32
    got64 = uv_face_frames(vp, f, uvp.astype(np.float64))
    assert np.abs(got64 - want).max() <= 2 * sl64.U


def test_a_rank_deficient_uv_triangle_takes_the_1e3_rule():
    from ngp_harness.curved import uv_face_frames

    v = np.float64([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]])
    f = np.array([[0, 1, 2], [1, 3, 2]])
    uv = np.float64([[0, 0], [0.5, 0], [1, 0], [0.5, 0.7]])  # face 0: three collinear UV corners (rank 1); face 1: a proper triangle
    got = uv_face_frames(v, f, uv)
    assert np.isfinite(got).all()
    # face 0 by hand: edges (0.5, 0), (1, 0) -> [1, 1] += 1e-3 -> inverse [[2, 0], [-2000, 1000]]; t = 2 e0 = (2, 0, 0) -> (1, 0, 0); n = (0, 0, 1); b = n x t
    assert np.allclose(got[0], [[1, 0, 0], [0, 1, 0], [0, 0, 1]], atol=1e-6)
    want = sl64.uv_face_frames(v, f, uv)
    assert np.abs(got - want).max() <= 2 * sl64.U
    # without the rule the inverse of face 0 does not exist
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.inv((uv[f][:, 1:] - uv[f][:, :1])[:1])


# ---- the third rotation of the float64 helper ---------------------------------------------------------------------------------------------------------------

def _rotation_problem(n=2048, seed=11):
    """Seeded inputs for the rotations alone: a fixed normal net, frames that are far from the identity and differ per row, orthonormal face frames
    of the star mesh taken by face id; `order`: a permutation standing in for the BVH's reordering of the faces."""
    from ngp_harness.curved import FactorizedNormalNet, shape_preprocess, uv_face_frames

    rng = np.random.default_rng(seed)
    torch.manual_seed(3)
    net = FactorizedNormalNet(x_dim=16, z_dim=25).eval()
    with torch.no_grad():
        for mlp in (net.phi_net, net.theta_net):
            for layer in mlp.layers:
                layer.W.mul_(6.0), layer.c.fill_(2.0)
    weights, biases, _, _ = nn64.pack(net)
    v, f, _, uvs = sf.mesh_of("star")
    vp, uvp, _, _ = shape_preprocess(v, f, uvs, normalize=False)
    table = uv_face_frames(vp, f, uvp)
    face = rng.integers(0, len(f), n)
    order = rng.permutation(len(f))
    half = lambda a: a.astype(np.float16).astype(np.float32)  # noqa: E731
    return dict(phi=half(rng.uniform(-0.5, 0.5, (n, 8))), x=half(rng.uniform(-0.5, 0.5, (n, 16))), z=half(rng.uniform(-1, 1, (n, 12))), weights=weights, biases=biases,
                local=(np.eye(3).reshape(1, 3, 3) + rng.normal(0, 0.35, (n, 3, 3))).astype(np.float32),
                sample=(np.eye(3).reshape(1, 3, 3) + rng.normal(0, 0.3, (n, 3, 3))).astype(np.float32), table=table, face=face, order=order,
                coarse=rng.normal(size=(n, 3)).astype(np.float32))


@pytest.fixture(scope="module")
def rotations():
    return _rotation_problem()


def _emulated(P, new_tbn):
    """The three half products and the two normalisations in fp32, from the helper's own local normal (float64, rounded to half by the first)."""
    base = sl64.fine_normal(P["phi"], P["x"], P["z"], P["weights"], P["biases"], P["local"], P["sample"], new_tbn)
    n = sl64.rotate_half(new_tbn, sl64.rotate_half(P["sample"], sl64.rotate_half(P["local"], base["local"])))
    for _ in range(2):
        n = (n / (np.sqrt((n * n).sum(-1, keepdims=True, dtype=np.float32)) + np.float32(1e-5))).astype(np.float32)
    return n, base


def test_the_third_rotation_is_inside_its_own_bound_and_the_mutants_are_not(rotations):
    P = rotations
    new_tbn = P["table"][P["face"]]
    got, ref = _emulated(P, new_tbn)
    ratio = np.abs(got - ref["normal"]) / ref["bound_normal"]
    print(f"emulated half products against the float64 statement: largest error / bound {float(ratio.max()):.3f}, median bound {float(np.median(ref['bound_normal'])):.3e}")
    assert ratio.max() <= 1.0
    for mutant in sl64.MUTANTS:
        frames = P["table"][P["order"]][P["face"]] if mutant == "bvh_position" else new_tbn  # (the BVH's reordered position instead of the face's id)
        wrong = sl64.fine_normal(P["phi"], P["x"], P["z"], P["weights"], P["biases"], P["local"], P["sample"], frames,
                                 mutate=None if mutant == "bvh_position" else mutant)
        outside = (np.abs(got - wrong["normal"]) > wrong["bound_normal"]).any(-1)
        print(f"mutant {mutant}: {float(outside.mean()):.3f} of the rows outside the bound")
        if mutant != "frames_multiplied":
            assert outside.mean() > 0.5, mutant
    # Frames multiplied together before rounding differ from the sequential products by ONE half rounding, which a bound that grants every
    # rotation its own rounding cannot see (measured above: about 0.1 % of the rows).  That mutant is caught where the arithmetic is exact: the
    # half products themselves, whose bits the two orders do not share.
    n1 = sl64.rotate_half(P["local"], ref["local"])
    seq = sl64.rotate_half(new_tbn, sl64.rotate_half(P["sample"], n1))
    merged = sl64.rotate_half(np.einsum("nbc,nca->nba", P["sample"].astype(np.float64), new_tbn.astype(np.float64)).astype(np.float32), n1)
    differ = (seq != merged).any(-1)
    print(f"mutant frames_multiplied: the half results differ in their bits on {float(differ.mean()):.3f} of the rows")
    assert differ.mean() > 0.5


def test_the_blend_takes_the_new_meshs_coarse_normal(rotations):
    P = rotations
    new_tbn = P["table"][P["face"]]
    full = sl64.fine_normal(P["phi"], P["x"], P["z"], P["weights"], P["biases"], P["local"], P["sample"], new_tbn)
    blend = sl64.fine_normal(P["phi"], P["x"], P["z"], P["weights"], P["biases"], P["local"], P["sample"], new_tbn, coarse_raw=P["coarse"], fc_weight=0.7, blend=True)
    c = P["coarse"] / np.linalg.norm(P["coarse"], axis=-1, keepdims=True)
    want = 0.7 * full["normal"] + (1 - np.float64(np.float32(0.7))) * c
    want /= np.linalg.norm(want, axis=-1, keepdims=True)
    assert np.abs(blend["normal"] - want).max() < 1e-4 and (blend["bound_normal"] >= 0.5 * full["bound_normal"].min()).all()
    one = sl64.fine_normal(P["phi"], P["x"], P["z"], P["weights"], P["biases"], P["local"], P["sample"], new_tbn, coarse_raw=P["coarse"], fc_weight=1.0, blend=True)
    assert np.abs(one["normal"] - full["normal"]).max() < 1e-4


# ---- the reference's own run (tests/golden/ref_python_import_shape_sh.npz, tools/make_golden.py --import-shape-sh-only) ------------------------------------

@pytest.fixture(scope="module")
def golden():
    load = lambda n: np.load(os.path.join(ROOT, "tests", "golden", n))  # noqa: E731
    return load("ref_python_import_shape_sh.npz"), load("ref_python_import_shape.npz"), load("ref_python_import_field_sh.npz")


def test_uv_face_frames_reproduce_the_fixtures_tbn(golden):
    """The reference's own calculate_tbn over the normalised float64 mesh and the mapped fp32 UVs, against the restatement over the same two
    (`shape_vertices`, `shape_preprocess`'s UVs -- what import_shape(new_tbn="uv") hands it): the bar is frames_bar's (fp32 rounding of a
    float64 result plus the fp32 inverse's error)."""
    from ngp_harness.curved import shape_preprocess, shape_vertices, uv_face_frames

    g, gs, _ = golden
    v32, uv, _, _ = shape_preprocess(gs["vertices_raw"], gs["faces"], gs["uvs_raw"], normalize=True)
    assert np.array_equal(v32, gs["vertices"]) and np.array_equal(uv, gs["uvs"])
    v = shape_vertices(gs["vertices_raw"], True)
    got = uv_face_frames(v, gs["faces"], uv)
    err, bar = np.abs(got - g["tbn"]).max((1, 2)), sl64.frames_bar(v, gs["faces"], uv)
    print(f"fixture tbn: {len(got)} faces, largest error {float(err.max()):.3e}, largest error / bar {float((err / bar).max()):.3f}, largest bar {float(bar.max()):.3e}")
    assert got.shape == g["tbn"].shape == (1058, 3, 3) and (err <= bar).all()
    want = sl64.uv_face_frames(v, gs["faces"], uv)
    assert (np.abs(g["tbn"] - want).max((1, 2)) <= bar).all(), "the float64 statement, too"
    assert [int(g[f"S{k}_near_texel_edge"]) for k in range(3)] == [0, 0, 0], "rows within the nearest read's margin of a texel edge: the generator's cap is 1 %"


@pytest.mark.parametrize("key", ["S0", "S1", "S2"])
def test_the_float64_statement_reproduces_the_fixtures_normals_and_the_mutants_do_not(golden, key):
    """normal_fine and the shading normals of the reference's run (fp32 on the CPU: no half rounding anywhere) inside the helper's bound widened
    for fp32 inputs.  The statement is fed the fixture's own sampled inputs (phi, the embedding's 28 columns, the three frames, the raw coarse
    normal of ref_python_import_shape.npz), so EVERY row is decided: shape_float64's undecided rows and the rows at a texel's edge (0 in this
    fixture) concern a statement that projects the points itself.  Excluded share: 0 of the 6 % the cap allows."""
    g, gs, gl = golden
    f = _bare_field()
    il64.load_normal_net(f.normal_net, gl)
    weights, biases, dweights = il64.pack_fp32(f.normal_net)
    new_tbn, face = g[key + "_new_tbn"], g[key + "_face"]
    assert np.array_equal(new_tbn, g["tbn"][np.maximum(face, 0)]) and np.array_equal(face, gs[key + "_face"]), "new_tbn = tbn[face], -1 reads face 0"
    args = (g[key + "_phi"], g[key + "_embed28"][:, :16], g[key + "_embed28"][:, 16:], weights, biases, g[key + "_local_tbn"], g[key + "_sample_tbn_inv"])
    kw = dict(fp32_inputs=True, dweights=dweights)
    ref = sl64.fine_normal(*args, new_tbn, **kw)
    fine = g[key + "_normal_fine"]
    ratio = np.abs(fine - ref["fine"]) / ref["bound_fine"]
    print(f"{key} fixture normal_fine: max error / bound {float(ratio.max()):.3f}, median bound {float(np.median(ref['bound_fine'])):.3e}, excluded rows 0.0000 (cap 0.06)")
    assert ratio.max() <= 1.0
    for fc in (1.0, 0.7):
        ev = sl64.fine_normal(*args, new_tbn, coarse_raw=gs[key + "_normal_raw"], fc_weight=fc, blend=True, **kw)
        r = np.abs(g[f"{key}_fc{fc}_shading_normal"] - ev["normal"]) / ev["bound_normal"]
        print(f"{key} fc={fc} fixture shading normal: max error / bound {float(r.max()):.3f}")
        assert r.max() <= 1.0
    # the mutants: the fixture's normal lies outside their bound on most rows.  (Frames multiplied together before rounding are not a mutant of
    # an fp32 run, which rounds to half nowhere: that one is caught on the half products, above.)
    order = np.random.default_rng(3).permutation(len(g["tbn"]))
    for mutant in ("no_third", "third_transposed", "bvh_position"):
        frames = g["tbn"][order][np.maximum(face, 0)] if mutant == "bvh_position" else new_tbn
        wrong = sl64.fine_normal(*args, frames, mutate=None if mutant == "bvh_position" else mutant, **kw)
        outside = (np.abs(fine - wrong["fine"]) > wrong["bound_fine"]).any(-1)
        print(f"{key} mutant {mutant}: {float(outside.mean()):.3f} of the rows outside the bound")
        assert outside.mean() > 0.5, mutant


# ---- import_shape(new_tbn=...): refusals, the state a refused call leaves, the stamp ------------------------------------------------------------------------

TRI_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.2]], np.float32)
TRI_F = np.array([[0, 1, 2], [1, 3, 2]])
TRI_UV = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float32)
_STATE = ("imported", "imported_type", "shape_projector", "shape_faces", "shape_uvs", "shape_face_uv", "shape_face_tbn", "sdf_scale_factor", "recommended_sdf_factor",
          "_import_version")


def _state(f):
    return {k: getattr(f, k) for k in _STATE}


def test_new_tbn_is_refused_in_the_documented_cases_and_the_field_stays_as_it_was():
    f = _bare_field()
    assert f.shape_face_tbn is None
    with pytest.raises(RuntimeError, match="has to be imported first"):
        f.import_shape(TRI_V, TRI_F, TRI_UV, new_tbn="uv")
    f.import_field(pf.seeded_map(2, 3), 0.5, **_maps())
    before = _state(f)
    with pytest.raises(NotImplementedError, match="phi_embed.*local_tbn.*sample_tbn.*new mesh's frames"):
        f.import_shape(TRI_V, TRI_F, TRI_UV)  # the default: today's refusal, word for word
    for bad, text in [(np.zeros((3, 3, 3), np.float32), r"one frame per face, \[F, 3, 3\]"), (np.zeros((2, 9), np.float32), r"one frame per face"),
                      (np.full((2, 3, 3), np.nan, np.float32), "must be finite"), (np.full((2, 3, 3), np.inf, np.float32), "must be finite"),
                      ("xatlas", "\"uv\" or an array")]:
        with pytest.raises(ValueError, match=text):
            f.import_shape(TRI_V, TRI_F, TRI_UV, new_tbn=bad)
        assert _state(f) == before, bad
    # UV corners that coincide on every face: the reference's frames are not finite, and "uv" says so
    with pytest.raises(ValueError, match="must be finite"):
        f.import_shape(TRI_V, TRI_F, np.float32([[0, 0], [1, 1], [1, 1], [1, 1]]), new_tbn="uv")
    assert _state(f) == before
    # a lit field whose four maps were never imported
    g = _bare_field()
    g.features_imported, g.imported, g.imported_type = torch.zeros(2, 3, 16), True, "field"
    with pytest.raises(RuntimeError, match="import them first"):
        g.import_shape(TRI_V, TRI_F, TRI_UV, new_tbn="uv")
    # a field without a normal net would ignore the frames
    u = _bare_field(lit=False)
    u.import_field(pf.seeded_map(2, 3), 0.5)
    before = _state(u)
    with pytest.raises(ValueError, match="would ignore it"):
        u.import_shape(TRI_V, TRI_F, TRI_UV, new_tbn="uv")
    assert _state(u) == before


def test_the_padded_table_and_the_stamp(monkeypatch):
    """import_shape with a stand-in for the device structures: shape_face_tbn is [F + 8, 12] for a mesh of at most 8 faces, nine floats and three
    zeros per face in the ORIGINAL face order; the lit field's "import-shape" stamp carries the six lit maps and the frames, the unlit one is the
    tuple it was."""
    from ngp_harness import curved

    def projector(v, faces, **kw):
        p = types.SimpleNamespace(_knn=types.SimpleNamespace(value=11), tracer=types.SimpleNamespace(_handle=types.SimpleNamespace(value=12)),
                                  mesh_vertices=torch.as_tensor(v), vertex_normals=torch.zeros(len(v), 3))
        p.to = lambda dev: p
        return p

    monkeypatch.setattr(curved, "MeshProjector", projector)
    f = _bare_field()
    f.import_field(pf.seeded_map(2, 3), 0.5, **_maps())
    f.import_shape(TRI_V, TRI_F, TRI_UV, normalize=False, new_tbn="uv")
    assert f.imported_type == "shape" and tuple(f.shape_face_tbn.shape) == (10, 12) == (f.shape_face_uv.shape[0], 12)
    want = curved.uv_face_frames(TRI_V, TRI_F, f.shape_uvs.numpy())
    assert np.array_equal(f.shape_face_tbn.numpy(), sl64.padded_table(want)) and not f.shape_face_tbn[2:].any() and not f.shape_face_tbn[:, 9:].any()
    base = f._import_stamp()
    assert base[0] == "import-shape"
    for name in ("phi_embed_imported", "local_tbn_imported", "sample_tbn_inv_imported", "sample_tbn_ids_imported", "frame_map_imported", "sample_inv_rows_imported",
                 "shape_face_tbn"):
        kept = getattr(f, name)
        setattr(f, name, kept.clone())
        assert f._import_stamp() != base, name
        setattr(f, name, kept)
        assert f._import_stamp() == base
    # frames handed over as an array are taken as given; the stamp moves with them
    given = np.tile(np.eye(3, dtype=np.float32)[[1, 2, 0]], (2, 1, 1))
    f.import_shape(TRI_V, TRI_F, TRI_UV, normalize=False, new_tbn=torch.from_numpy(given))
    assert np.array_equal(f.shape_face_tbn.numpy(), sl64.padded_table(given)) and f._import_stamp() != base
    # a mesh of more than 8 faces is not padded
    v, fc, _, uvs = sf.mesh_of("height")
    f.import_shape(v, fc, uvs, normalize=False, new_tbn="uv")
    assert tuple(f.shape_face_tbn.shape) == (len(fc), 12)
    # the switches and setters work as they do for the unlit field
    f.set_k_for_uv(4), f.set_sdf_factor(2.0), f.set_uv_utilize_rate(0.8), f.set_sdf_offset(0.01), f.set_h_threshold(0.03)
    assert f._shape_scalars() == (4, float(np.float32(2.0 / 0.8)), 0.01, 0.8, 0.03)
    f.switch_shape_feature()
    assert f.imported_type == "field" and f._import_stamp()[0] == "import"
    f.switch_shape_feature(), f.switch_import()
    assert f._import_stamp() == ()
    f.switch_import()
    with pytest.raises(NotImplementedError, match="without gradients to the sample position"):
        f.embed(torch.zeros(4, 3), requires_grad_xyz=True, with_fine_normal=True)
    # the unlit field: the tuple it was, no frames
    u = _bare_field(lit=False)
    u.import_field(pf.seeded_map(2, 3), 0.5)
    u.import_shape(TRI_V, TRI_F, TRI_UV, normalize=False)
    p = u.shape_projector
    assert u.shape_face_tbn is None
    assert u._import_stamp() == (("import-shape", u.features_imported.data_ptr(), (2, 3, 16), 11, 12, p.mesh_vertices.data_ptr(), p.vertex_normals.data_ptr(),
                                  u.shape_face_uv.data_ptr()) + u._shape_scalars() + (u._import_version,))


def test_a_field_that_never_imported_keeps_its_init_state():
    f = _bare_field()
    assert f.shape_face_tbn is None and f._import_stamp() == ()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------------------

def _struct_fields():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nerftex_curved_light_shape_infer_desc \{(.*?)\} nerftex_curved_light_shape_infer_desc;", src, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            names.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", first.strip()).group(1))
            names += [m.strip() for m in more]
    return names


def test_the_header_declares_and_the_library_exports_the_entry_points(tmp_path):
    import nerftex_hip

    src = open(HEADER).read()
    for name in ("nerftex_shape_light_lookup", "nerftex_curved_light_shape_infer", "nerftex_curved_light_shape_infer_scratch_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(ctypes.CDLL(nerftex_hip.LIB_PATH), name) and name in nerftex_hip.EXPORTS
    fields = _struct_fields()
    assert [n for n, _ in nerftex_hip.CurvedLightShapeInferDesc._fields_] == fields
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {",
             '    printf("sizeof %lu\\n", (unsigned long)sizeof(nerftex_curved_light_shape_infer_desc));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof(nerftex_curved_light_shape_infer_desc, {n}));' for n in fields]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(nerftex_hip.CurvedLightShapeInferDesc)
    for n in fields:
        assert int(out[n]) == getattr(nerftex_hip.CurvedLightShapeInferDesc, n).offset, n
    # the plain entry's argument list: the header's parameters, one ctypes entry each
    decl = re.search(r"int nerftex_shape_light_lookup\((.*?)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S).group(1)
    assert len(decl.split(",")) == len(nerftex_hip._SIGNATURES["nerftex_shape_light_lookup"]) == 37


def test_scratch_query():
    from nerftex_hip import lib

    sizes = [lib.nerftex_curved_light_shape_infer_scratch_bytes(b) for b in (0, 128, 256, 1 << 20)]
    assert sizes[0] == 0 and sizes[1] > 0 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    # the neighbour lists, then the lit import chain's buffers with a third frame
    assert sizes[3] == (1 << 20) * (64 + 64 + 1 + 12 + 96 + 32 + 16 + 36 + 36 + 36 + 4 + 32 + 32 + 12)


FAKE = 0x10000  # a non-NULL, 256-byte aligned address that is never dereferenced: every case below is refused before the tracer is looked at


def _desc(**over):
    from nerftex_hip import CurvedLightShapeInferDesc

    kw = dict(B=128, n_verts=100, n_faces=10, n_tbn_faces=10, K=5, map_h=24, map_w=20, n_features=16, n_phi=8, n_patches=5, sdf_scale=1.0, sdf_offset=0.0, uv_rate=1.0,
              h_threshold=0.0625, n_freqs=12, sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16, normal_hidden=16, normal_layers=2, brdf_in=16,
              brdf_hidden=64, brdf_layers=3, brdf_out=5, n_sh=16, n_color=1, gamma=2.4, flags=1, visual_mode=0, fc_weight=1.0, eval=1, scratch_bytes=1 << 40)
    kw.update({name: FAKE for name in ("knn", "xyz", "dirs", "mesh_vertices", "vertex_normals", "face_uv", "face_tbn", "map", "phi_map", "frame_map", "sample_tbn_inv",
                                       "sigma_weights", "normal_weights", "normal_biases", "brdf_weights", "env_shs", "sigma", "rgbs", "scratch")})
    kw["tracer"] = None  # (a real tracer needs a device: the refusals in front of it are what this file can reach)
    kw.update(over)
    return CurvedLightShapeInferDesc(**kw)


REFUSED = [
    (dict(B=100), "multiple of 128"),
    (dict(n_verts=0), "between 1 and 2^31 - 1 vertices"),
    (dict(K=17), "1 <= K <= 16"),
    (dict(n_features=8), "default SH-lit curved field"),
    (dict(n_phi=16), "default SH-lit curved field"),
    (dict(sigma_hidden=64), "default SH-lit curved field"),
    (dict(normal_layers=3), "default SH-lit curved field"),
    (dict(brdf_out=3), "default SH-lit curved field"),
    (dict(n_sh=4), "at least 9 SH rows"),
    (dict(gamma=0.0), "gamma is positive and finite"),
    (dict(visual_mode=4), "NERFTEX_LIGHT_VISUAL_"),
    (dict(eval=2), "eval is 0 or 1"),
    (dict(B=64, K=0), "multiple of 128"),  # the batch before K
    (dict(K=0, n_phi=4), "1 <= K <= 16"),  # K before the shapes
    (dict(n_phi=4, n_sh=4), "default SH-lit curved field"),  # the shapes before the head
    (dict(), "a raytracer is required"),  # ... and the head before the tracer
    (dict(B=0, n_patches=0, map_h=0), "a raytracer is required"),  # the tracer is looked at before the maps and before the empty batch returns
]


@pytest.mark.parametrize("over,text", REFUSED, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) or "tracer" if isinstance(v, dict) else None)
def test_the_chain_refuses_before_any_launch(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_curved_light_shape_infer(ctypes.byref(_desc(**over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_the_chain_null_descriptor_and_the_plain_entry_without_a_tracer():
    from nerftex_hip import lib

    assert lib.nerftex_curved_light_shape_infer(None, None) == NERFTEX_ERR_INVALID
    assert "NULL descriptor" in lib.nerftex_last_error().decode()
    args = [None, FAKE, FAKE, FAKE, 4, 5, FAKE, FAKE, 100, FAKE, 10, FAKE, 10, FAKE, FAKE, FAKE, FAKE, 24, 20, 5, 1.0, 0.0, 1.0, 0.0625, 12] + [FAKE] * 11 + [None]
    assert lib.nerftex_shape_light_lookup(*args) == NERFTEX_ERR_INVALID
    assert "shape_light_lookup" in lib.nerftex_last_error().decode() and "must not be NULL" in lib.nerftex_last_error().decode()
