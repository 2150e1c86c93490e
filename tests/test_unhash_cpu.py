"""The curved field baked onto the vertices of a fine mesh (the unhash import), the CPU side (no GPU): the float64 statement of
tests/unhash_float64.py reproduces the reference fixture tests/golden/ref_python_unhash.npz (tools/make_golden.py: unhash_goldens), the fp32
emulation of the kernel passes the check, every deliberately wrong lookup fails it, the excluded share of every case is under its cap, midpoint
subdivision has its properties, and the state machine, the binding and the refusals that need no device."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import geometry_float64 as g
import unhash_float64 as uf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
NERFTEX_ERR_INVALID = 1
EXCLUDED_CAP = 0.05
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        print("\n" + "\n".join(REPORT))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_unhash.npz"))


@pytest.fixture(scope="module")
def trace32(oracle):
    return lambda v, f, o, d: oracle.raytrace(v, f, o, d)[:4]


def _case(name, trace32):
    P = uf.problem(name)
    if "tol_t" not in P:
        R = P["rays"]
        uf.set_tolerances(P, trace32(R["v"], R["f"], R["o"], R["d"]))
    return P


def _fmt(r):
    return " ".join(f"{k} {v:.3f}" for k, v in r.items())


# ---- the float64 statement against the reference's own run ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["U0", "U1", "U2"])
def test_the_float64_statement_reproduces_the_fixture(golden, trace32, key):
    G = golden
    coarse = (G["vertices"], G["faces"].astype(np.uint32), G["vertex_normals"])
    fine = (G["fine_vertices"], G["fine_faces"].astype(np.int64))
    features = G["U2_features"] if key == "U2" else G["features"]
    P = uf.build_problem("fixture " + key, coarse, fine, features, G["xyz"], float(G["h_threshold"]), float(G[key + "_sdf_factor"]), float(G[key + "_offset"]),
                         neighbours=(G["knn_idx"], G["knn_dis"]))  # (the reference's own search: which copies of a duplicated pole vertex it returns is its business)
    R = P["rays"]
    uf.set_tolerances(P, trace32(R["v"], R["f"], R["o"], R["d"]))
    s = uf.describe(P)
    assert s["excluded"] <= EXCLUDED_CAP and 0.02 < s["far"] < 0.04 and s["N"] == 512
    embed = G[key + "_embed"]
    xin = np.ones((512, 48), np.float16)
    xin[:, :41] = embed.astype(np.float16)
    assert np.array_equal(embed[:, 16], G[key + "_sdf"])
    r = uf.check(P, G[key + "_sdf"], G[key + "_h_mask"], G[key + "_normal_raw"], G[key + "_face"].astype(np.int64), G[key + "_bary"], xin)
    raw = G[key + "_normal_raw"].astype(np.float64)
    assert np.abs(G[key + "_normal"] - raw / (np.linalg.norm(raw, axis=-1, keepdims=True) + 1e-5)).max() < 1e-6  # tools/map.py:720
    outside = float(1 - G[key + "_h_mask"].mean())
    assert 0.02 < outside < 0.2, "some rows miss or fall outside the mask"
    REPORT.append(f"fixture {key}: excluded {s['excluded']:.4f} far {s['far']:.3f} masked in {s['masked_in']:.3f}  reference ratios {_fmt(r)}")


def test_the_fixtures_fine_mesh_is_one_subdivision_of_its_coarse_mesh(golden):
    fv, ff = uf.subdivide_midpoint(golden["vertices"], golden["faces"])
    assert np.array_equal(fv.astype(np.float32), golden["fine_vertices"]) and np.array_equal(ff, golden["fine_faces"])


# ---- the check itself: the emulation passes, the mutants fail, the cases are the ones described -----------------------------------------------------

@pytest.mark.parametrize("name", list(uf.CASES))
def test_the_case_is_the_one_described_and_the_emulation_passes(name, trace32):
    P = _case(name, trace32)
    s = uf.describe(P)
    mesh, N, h, scale, offset, far, on_vertex, at_threshold = uf.CASES[name]
    assert s["N"] == N and s["K"] == min(8, len(P["v"]))
    assert s["excluded"] <= EXCLUDED_CAP, f"{name}: {s['excluded']:.4f} of the rows are undecided for the reference alone"
    if on_vertex:
        assert np.array_equal(P["x"][0], P["v"][len(P["v"]) // 2]) and not P["decided"][0], "row 0 sits on a vertex: its answer is at 0"
    if far:
        assert s["far"] > 0.5 * far, "rows both traces miss"
    if at_threshold:
        rows = 1 + np.arange(at_threshold)
        assert (np.abs(np.abs(P["sdf"][rows]) - P["h_limit"]) < 1e-6).all(), "rows right at the mask threshold"
    if mesh == "quad":
        assert len(P["ff"]) == 2 and s["K"] == 4, "two faces (the tracer pads them), K clamped to the vertex count"
    r = uf.check(P, *uf.emulate(P, trace32))
    REPORT.append(f"{name:12s} excluded {s['excluded']:.4f} (at the threshold {s['at_threshold']:.4f}) far {s['far']:.3f} masked in {s['masked_in']:.3f} "
                  f"inside {s['inside']:.3f}  emulation ratios {_fmt(r)}")


@pytest.mark.parametrize("mutant", uf.MUTANTS)
def test_a_wrong_lookup_fails_the_check(mutant, trace32):
    caught = []
    for name in ("star_n512", "star_scaled", "star_far"):
        P = _case(name, trace32)
        try:
            uf.check(P, *uf.emulate(P, trace32, mutate=mutant))
        except AssertionError as e:
            caught.append(f"{name}: {str(e)[:100]}")
    assert caught, f"the mutant {mutant} passes every case"
    REPORT.append(f"mutant {mutant:14s} caught by {len(caught)} of 3 cases; {caught[0]}")


# ---- midpoint subdivision ---------------------------------------------------------------------------------------------------------------------------------

def _edges(f):
    e = np.sort(np.asarray(f, np.int64)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    return np.unique(e, axis=0, return_counts=True)


def _area(v, f):
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    return 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=-1)


def _welded(v, f):
    """the mesh with vertices at the same position made one (the star's poles are duplicated; sin(pi) leaves its south pole's copies 1e-17 apart)"""
    uniq, inverse = np.unique(np.round(np.asarray(v, np.float64), 6), axis=0, return_inverse=True)
    f = inverse.reshape(-1)[np.asarray(f, np.int64)]
    return uniq, f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]


@pytest.mark.parametrize("mesh", ["star", "quad", "tetrahedron"])
def test_midpoint_subdivision_has_its_properties(mesh):
    from ngp_harness.subdivide import subdivide_midpoint

    if mesh == "tetrahedron":
        v, f = np.float32([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]), np.asarray([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    else:
        v, f, _ = uf.mesh_of(mesh)[0]
    edges, _ = _edges(f)
    fv, ff = subdivide_midpoint(v, f)
    V, E, F = len(v), len(edges), len(f)
    assert fv.dtype == np.float64 and fv.shape == (V + E, 3) and ff.shape == (4 * F, 3) and ff.dtype == np.int64
    assert np.array_equal(fv[:V], np.asarray(v, np.float64)), "the originals keep their numbers"
    mid = 0.5 * (np.asarray(v, np.float64)[edges[:, 0]] + np.asarray(v, np.float64)[edges[:, 1]])
    assert np.array_equal(fv[V:], mid), "every new vertex is the float64 midpoint of one unique edge"
    assert sorted(np.unique(ff).tolist()) == list(range(V + E)), "every vertex is used"
    a0, a1 = _area(v, f), _area(fv, ff).reshape(F, 4)
    assert np.allclose(a1, a0[:, None] / 4, rtol=1e-12, atol=1e-18), "four children of a quarter of the parent's area each, in the parent's slot"
    assert abs(a1.sum() / a0.sum() - 1) < 1e-13
    # children keep the parent's orientation
    n0 = np.cross(fv[np.asarray(f, np.int64)[:, 1]] - fv[np.asarray(f, np.int64)[:, 0]], fv[np.asarray(f, np.int64)[:, 2]] - fv[np.asarray(f, np.int64)[:, 0]])
    n1 = np.cross(fv[ff[:, 1]] - fv[ff[:, 0]], fv[ff[:, 2]] - fv[ff[:, 0]]).reshape(F, 4, 3)
    assert ((n1 * n0[:, None]).sum(-1) > 0).all() or (a0 == 0).any()
    if mesh != "quad":  # a closed surface stays closed: every edge of the welded mesh lies in exactly two faces
        for vv, tri in ((v, f), (fv, ff)):
            _, count = _edges(_welded(vv, tri)[1])
            assert (count == 2).all()


def test_subdivide_until_loops_and_refuses():
    from ngp_harness.subdivide import subdivide_midpoint, subdivide_until

    v, f, _ = uf.mesh_of("quad")[0]
    same = subdivide_until(v, f, 4)
    assert same[0].shape == (4, 3) and np.array_equal(same[1], f.astype(np.int64))
    fv, ff = subdivide_until(v, f, 20)
    assert len(fv) == 25 and len(ff) == 32, "4 -> 9 -> 25 vertices"
    once = subdivide_midpoint(*subdivide_midpoint(v, f))
    assert np.array_equal(fv, once[0]) and np.array_equal(ff, once[1])
    with pytest.raises(ValueError, match="indexes into"):
        subdivide_midpoint(v, np.asarray([[0, 1, 4]]))
    with pytest.raises(ValueError, match=r"\[V, 3\]"):
        subdivide_midpoint(v[:, :2], f)
    with pytest.raises(ValueError, match="never grows"):
        subdivide_until(v, np.zeros((0, 3), np.int64), 10)


# ---- the state machine ----------------------------------------------------------------------------------------------------------------------------------

def _bare_field(h_threshold=0.0625):
    """A CurvedField without its mesh structures (they need a device)."""
    from ngp_harness.curved import CurvedField

    f = object.__new__(CurvedField)
    torch.nn.Module.__init__(f)
    f.normal_net, f.light_model, f.multires, f.h_threshold, f.in_dim = None, None, 12, h_threshold, 41
    f.encoder = types.SimpleNamespace(output_dim=16)
    f.sigma_net = types.SimpleNamespace(weights=torch.zeros(1), dtype=torch.float16)
    f.projector = types.SimpleNamespace(h_threshold=h_threshold, mesh_vertices=torch.zeros(5, 3))
    f._init_import_state()
    return f


def _fake_unhash(f, V=6, F=3):
    """the state unhash() leaves, with a stand-in for the tracer"""
    f.unhash_tracer = types.SimpleNamespace(_handle=types.SimpleNamespace(value=21))
    f.unhash_vertices, f.unhash_faces, f.unhash_face_vertices = torch.zeros(V, 3), torch.zeros(F, 3, dtype=torch.int64), torch.zeros(F + 8, 3, dtype=torch.int32)
    f.features_imported = torch.zeros(V, 16)
    f.imported, f.imported_type = True, "unhash"


def _snapshot(f):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(f).items() if not k.startswith("_modules")}


def _same(a, b):
    return a.keys() == b.keys() and all((torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] is b[k] or a[k] == b[k]) for k in a)


def test_a_lit_field_is_refused_and_says_why():
    v, faces = uf.mesh_of("quad")[1]
    for lit in (dict(normal_net=object()), dict(light_model="SH")):
        f = _bare_field()
        for k, val in lit.items():
            setattr(f, k, val)
        before = _snapshot(f)
        with pytest.raises(NotImplementedError, match="query_tbn returns a tuple"):
            f.import_unhash_vertices(v, faces, np.zeros((4, 16), np.float32))
        with pytest.raises(NotImplementedError, match="only the static light model"):
            f.unhash(min_vnum=100)
        with pytest.raises(NotImplementedError, match="only the static light model"):
            f.unhash(mesh=(v, faces))
        assert _same(before, _snapshot(f))


BAD = [
    (dict(vertices=np.zeros((4, 2), np.float32)), r"\[V', 3\]"),
    (dict(faces=np.zeros((2, 4), np.int64)), r"\[F', 3\]"),
    (dict(faces=np.zeros((0, 3), np.int64)), r"\[F', 3\]"),
    (dict(faces=np.asarray([[0, 1, 4]])), "indexes into the 4 fine vertices"),
    (dict(faces=np.asarray([[0, 1, -1]])), "indexes into the 4 fine vertices"),
    (dict(faces=np.asarray([[0.0, 1.0, 2.0]])), "whole numbers"),
    (dict(vertices=np.float32([[0, 0, 0], [1, 0, 0], [0, 1, np.nan], [1, 1, 0]])), "fine vertex must be finite"),
    (dict(features=np.zeros((4, 8), np.float32)), r"features are \[V', 16\]"),
    (dict(features=np.zeros((5, 16), np.float32)), r"features are \[V', 16\]"),
    (dict(features=np.full((4, 16), np.inf, np.float32)), "feature must be finite"),
    (dict(sdf_factor=float("nan")), "sdf_factor must be finite"),
]


@pytest.mark.parametrize("over,text", BAD, ids=[f"{i}-{next(iter(o))}" for i, (o, _) in enumerate(BAD)])
def test_a_refused_import_leaves_every_attribute_as_it_was(over, text):
    v, faces = uf.mesh_of("quad")[1]
    for start in ("fresh", "unhash"):
        f = _bare_field()
        if start == "unhash":
            _fake_unhash(f)
            f.set_sdf_factor(1.5)
        before = _snapshot(f)
        kw = dict(vertices=v, faces=faces, features=np.zeros((4, 16), np.float32), sdf_factor=1.0)
        kw.update(over)
        with pytest.raises(ValueError, match=text):
            f.import_unhash_vertices(**kw)
        assert _same(before, _snapshot(f)), "a refused call changes nothing of the field's state"


def test_the_stamp_is_the_tuple_written_out_and_follows_every_tensor_setter_and_switch():
    f = _bare_field()
    assert f.unhash_tracer is None and f._import_stamp() == () and not f._unhash_active()
    _fake_unhash(f)
    f._import_version = 3
    ft = f.features_imported
    want = ("import-unhash", ft.data_ptr(), (6, 16), f.unhash_vertices.data_ptr(), f.unhash_face_vertices.data_ptr(), 21, 1.0, 0.0, 0.0625, 3)
    stamp = f._import_stamp()
    assert stamp == want and f._unhash_active() and f._unhash_scalars() == (5, 1.0, 0.0, 0.0625)
    for name in ("features_imported", "unhash_vertices", "unhash_face_vertices"):
        old = getattr(f, name)
        setattr(f, name, old.clone())
        assert f._import_stamp() != stamp, name
        setattr(f, name, old)
        assert f._import_stamp() == stamp
    f.unhash_tracer._handle.value = 22
    assert f._import_stamp() != stamp
    f.unhash_tracer._handle.value = 21
    seen = [stamp]
    for change in (lambda: f.set_sdf_factor(2.5), lambda: f.set_sdf_offset(0.01), lambda: f.set_h_threshold(0.03)):
        change()
        assert f._import_stamp() not in seen
        seen.append(f._import_stamp())
    assert f._unhash_scalars() == (5, 2.5, 0.01, 0.03) and f.projector.h_threshold == 0.03
    f.set_sdf_factor(0.0)
    assert f._unhash_scalars()[1] == float(np.float32(1e-5)), "the reference's max(1e-5, sdf_scale)"
    f.projector.mesh_vertices = torch.zeros(40, 3)
    assert f._unhash_scalars()[0] == 8, "knn()'s default K"
    with pytest.raises(RuntimeError, match="no shape has been imported"):
        f.switch_shape_feature()
    v, faces = uf.mesh_of("quad")[1]
    with pytest.raises(RuntimeError, match="imported first"):
        f.import_shape(v, faces, v[:, :2])
    with pytest.raises(NotImplementedError, match="without gradients"):
        f.embed(torch.zeros(4, 3), requires_grad_xyz=True)
    with pytest.raises(NotImplementedError, match="without a fine normal"):
        f.embed(torch.zeros(4, 3), with_fine_normal=True)
    f.switch_import()
    assert not f.imported and f._import_stamp() == () and not f._unhash_active()
    f.switch_import()
    assert f._unhash_active() and f._import_stamp()[0] == "import-unhash" and f._import_stamp() not in seen


def test_the_unhash_source_takes_its_own_row_of_the_routes_and_no_other():
    from ngp_harness.curved import CurvedField
    from test_curved_infer_members_cpu import _field

    assert len(CurvedField._INFER_ROUTES) == 9 and CurvedField._INFER_ROUTES[-1] == (("unhash",), "_infer_unhash_fused", "nerftex_curved_unhash_infer",
                                                                                      "_infer_unhash_desc", False)
    assert sum("unhash" in row[0] for row in CurvedField._INFER_ROUTES) == 1
    x = d = torch.zeros(128, 3)
    f = _field(False, None)
    _fake_unhash(f)
    for row in CurvedField._INFER_ROUTES:
        setattr(f, row[1], lambda x, d: True)
    assert f._infer_route(x, d)[0] == "nerftex_curved_unhash_infer"
    f._infer_unhash_fused = lambda x, d: False
    assert f._infer_route(x, d) is None, "baked features never take a map's chain, a patch's or the mesh field's"
    # the lookup predicate: not for a fine normal, not with fused_glue off, not off the device of x
    g_ = _field(False, None)
    _fake_unhash(g_)
    g_._sigma_fused = lambda x=None: True
    here = types.SimpleNamespace(device=torch.device("cpu"))
    assert g_._unhash_fused(here) and g_._source_fused(here) and not g_._source_fused(here, lit=True)
    g_.fused_glue = False
    assert not g_._unhash_fused(here)
    g_.fused_glue = True
    assert not g_._unhash_fused(types.SimpleNamespace(device=torch.device("meta")))


def test_the_builder_passes_every_member_of_its_descriptor_and_nothing_else(monkeypatch):
    import nerftex_hip
    from ngp_harness import curved
    from test_curved_infer_members_cpu import _field

    monkeypatch.setattr(curved, "CurvedUnhashInferDesc", lambda **members: members)
    f = _field(False, None)
    _fake_unhash(f)
    B = 128
    x, d, out, scratch = torch.zeros(B, 3), torch.zeros(B, 3), torch.zeros(4 * B), torch.zeros(256, dtype=torch.uint8)
    passed, keep = f._infer_unhash_desc(x, d, None, out[:B], out[B:].view(B, 3), scratch)
    fields = [n for n, _ in nerftex_hip.CurvedUnhashInferDesc._fields_]
    assert len(set(fields)) == len(fields) and set(passed) == set(fields), (sorted(set(fields) - set(passed)), sorted(set(passed) - set(fields)))
    empty = {n for n, v in passed.items() if v is None or (v == 0 and not isinstance(v, float))}
    assert empty <= {"units_dev", "rows_per_unit"}, empty
    desc = nerftex_hip.CurvedUnhashInferDesc(**passed)
    held = {t.data_ptr() for t in keep if torch.is_tensor(t)}
    assert all(getattr(desc, n) in held for n in ("fine_vertices", "face_vertices", "vertex_features", "sigma_weights", "color_weights"))
    assert f.unhash_tracer in keep and desc.tracer == 21 and desc.knn == 11, "the FINE mesh's tracer, the field's OWN neighbour grid"
    assert (desc.K, desc.n_verts, desc.n_fine_verts, desc.n_faces, desc.n_features, desc.B, desc.eval) == (7, 7, 6, 11, 16, 128, 3)
    assert desc.dir_vec_wdist == pytest.approx(0.05) and desc.sdf_scale == 1.0 and desc.h_threshold == pytest.approx(0.0625) and desc.n_freqs == 12


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------------

def _struct_fields():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nerftex_curved_unhash_infer_desc \{(.*?)\} nerftex_curved_unhash_infer_desc;", src, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            names.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", first.strip()).group(1))
            names += [m.strip() for m in more]
    return names


def test_the_descriptor_is_bound_field_for_field_with_the_compilers_layout(tmp_path):
    import subprocess

    import nerftex_hip

    fields = _struct_fields()
    assert [n for n, _ in nerftex_hip.CurvedUnhashInferDesc._fields_] == fields
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {",
             '    printf("sizeof %lu\\n", (unsigned long)sizeof(nerftex_curved_unhash_infer_desc));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof(nerftex_curved_unhash_infer_desc, {n}));' for n in fields]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(nerftex_hip.CurvedUnhashInferDesc)
    for n in fields:
        assert int(out[n]) == getattr(nerftex_hip.CurvedUnhashInferDesc, n).offset, n


def test_the_plain_entry_is_bound_argument_for_argument():
    import nerftex_hip

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    args = re.search(r"int nerftex_vertex_lookup\((.*?)\);", src, flags=re.S).group(1).split(",")
    kinds = {"float": ctypes.c_float, "uint32_t": ctypes.c_uint32}
    want = [ctypes.c_void_p if "*" in a else kinds[a.split()[-2]] for a in args]
    assert nerftex_hip._SIGNATURES["nerftex_vertex_lookup"] == want
    for name in ("nerftex_vertex_lookup", "nerftex_curved_unhash_infer", "nerftex_curved_unhash_infer_scratch_bytes"):
        assert hasattr(ctypes.CDLL(nerftex_hip.LIB_PATH), name) and name in nerftex_hip.EXPORTS


def test_scratch_query():
    from nerftex_hip import lib

    sizes = [lib.nerftex_curved_unhash_infer_scratch_bytes(b) for b in (0, 128, 256, 1 << 20)]
    assert sizes[0] == 0 and sizes[1] > 0 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    # the neighbour list (16 ids and 16 distances), mask, normal, the two networks' inputs and outputs, the raw density: the shape chain's
    assert sizes[3] == (1 << 20) * (64 + 64 + 1 + 12 + 96 + 32 + 2 + 64 + 32) == lib.nerftex_curved_shape_infer_scratch_bytes(1 << 20)


FAKE = 0x10000  # a non-NULL address that is never dereferenced: every case below is refused before the raytracer is looked at


def _desc(**over):
    from nerftex_hip import CurvedUnhashInferDesc

    kw = dict(B=128, n_verts=4, K=4, dir_vec_wdist=0.05, n_fine_verts=4, n_faces=10, n_features=16, sdf_scale=1.0, sdf_offset=0.0, h_threshold=0.0625, n_freqs=12,
              sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16, color_in=32, color_hidden=64, color_layers=3, color_out=3, fc_weight=1.0, eval=3,
              scratch_bytes=1 << 40, tracer=None)
    kw.update({name: FAKE for name in ("knn", "xyz", "dirs", "mesh_vertices", "vertex_normals", "fine_vertices", "face_vertices", "vertex_features", "sigma_weights",
                                       "color_weights", "sigma", "rgbs", "scratch")})
    kw.update(over)
    return CurvedUnhashInferDesc(**kw)


REFUSED = [
    (dict(B=100), "multiple of 128"),
    (dict(B=64, K=0), "multiple of 128"),  # the batch before K
    (dict(n_verts=0), "between 1 and 2^31 - 1 vertices"),
    (dict(K=0), "1 <= K <= 16"),
    (dict(K=17), "1 <= K <= 16"),
    (dict(K=17, n_features=8), "1 <= K <= 16"),  # K before the shapes
    (dict(n_features=8), "default curved field"),
    (dict(sigma_hidden=64), "default curved field"),
    (dict(color_layers=2), "default curved field"),
    (dict(), "a raytracer over the fine mesh is required"),  # (a NULL raytracer: behind the shapes, in front of everything of the lookup)
    (dict(n_fine_verts=0), "a raytracer over the fine mesh is required"),
    (dict(n_freqs=10), "a raytracer over the fine mesh is required"),
]


@pytest.mark.parametrize("over,text", REFUSED, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) or "null-tracer" if isinstance(v, dict) else None)
def test_the_chain_refuses_before_any_launch(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_curved_unhash_infer(ctypes.byref(_desc(**over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_the_chain_null_descriptor_and_the_plain_entrys_null_pointers():
    from nerftex_hip import lib

    assert lib.nerftex_curved_unhash_infer(None, None) == NERFTEX_ERR_INVALID
    assert "NULL descriptor" in lib.nerftex_last_error().decode()
    args = [None, FAKE, FAKE, FAKE, 5, 8, FAKE, FAKE, 4, 0.05, FAKE, 4, FAKE, 10, FAKE, 1.0, 0.0, 0.0625, 12, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None]
    assert lib.nerftex_vertex_lookup(*args) == NERFTEX_ERR_INVALID  # (a NULL raytracer: the first refusal, nothing is dereferenced)
    assert "must not be NULL" in lib.nerftex_last_error().decode()
    for k in (1, 2, 3, 6, 7, 10, 12, 14, 19, 20, 21, 22, 23, 24):  # every other pointer: refused before the raytracer is dereferenced
        broken = list(args)
        broken[0], broken[k] = FAKE, None
        assert lib.nerftex_vertex_lookup(*broken) == NERFTEX_ERR_INVALID and "must not be NULL" in lib.nerftex_last_error().decode(), k
    # K and the two vertex counts come behind the pointers and in front of the raytracer's face count (which dereferences it)
    for over, text in (({5: 0}, "1 <= K <= 16"), ({5: 17}, "1 <= K <= 16"), ({5: 17, 8: 0}, "1 <= K <= 16"), ({8: 0}, "the field's mesh needs"),
                       ({8: 0, 11: 0}, "the field's mesh needs"), ({11: 0}, "the fine mesh needs")):
        broken = list(args)
        broken[0] = FAKE
        for k, val in over.items():
            broken[k] = val
        assert lib.nerftex_vertex_lookup(*broken) == NERFTEX_ERR_INVALID and text in lib.nerftex_last_error().decode(), (over, lib.nerftex_last_error().decode())
