"""An imported feature map on a new UV-mapped mesh under the curved field, the CPU side (no GPU): the float64 statement of
tests/shape_float64.py reproduces the reference fixture tests/golden/ref_python_import_shape.npz (tools/make_golden.py:
import_shape_goldens), the fp32 emulation of the kernel passes the check, every deliberately wrong lookup fails it, the excluded share of
every case is under its cap, the Python preprocessing gives the fixture's values, and the state machine, the binding and the refusals that
need no device."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import planar_float64 as pf
import shape_float64 as sf

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
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_import_shape.npz"))


@pytest.fixture(scope="module")
def trace32(oracle):
    return lambda v, f, o, d: oracle.raytrace(v, f, o, d)[:4]


def _case(name, trace32):
    P = sf.problem(name)
    if "tol_t" not in P:
        R = P["rays"]
        sf.set_tolerances(P, trace32(R["v"], R["f"], R["o"], R["d"]))
    return P


def _fmt(r):
    return " ".join(f"{k} {v:.3f}" for k, v in r.items())


# ---- the float64 statement against the reference's own run ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["S0", "S1", "S2"])
def test_the_float64_statement_reproduces_the_fixture(golden, trace32, key):
    G = golden
    mesh = (G["vertices"], G["faces"].astype(np.uint32), G["vertex_normals"], G["uvs"])
    K, rate, factor, offset = int(G[key + "_K"]), float(G[key + "_rate"]), float(G[key + "_sdf_factor"]), float(G[key + "_offset"])
    P = sf.build_problem("fixture " + key, mesh, G["xyz"], K, float(G["h_threshold"]), factor / rate, offset, rate, (24, 20))
    P["features"] = G["features"]
    R = P["rays"]
    sf.set_tolerances(P, trace32(R["v"], R["f"], R["o"], R["d"]))
    s = sf.describe(P)
    assert not P["nan"].any(), "the fixture's mesh has no duplicated vertex: the reference itself produces no NaN row"
    assert s["excluded"] <= EXCLUDED_CAP and 0.05 < s["far"] < 0.15
    uvh = G[key + "_uvh"]
    p_uv = uvh[:, :2] * np.float32(rate)  # (tools/map.py:696)
    xin = None
    if key + "_embed" in G:
        xin = np.ones((512, 48), np.float16)
        xin[:, :41] = G[key + "_embed"].astype(np.float16)
        assert np.array_equal(G[key + "_embed"][:, 16], uvh[:, 2])
    r = sf.check(P, p_uv, uvh[:, 2], G[key + "_h_mask"], G[key + "_normal_raw"], G[key + "_face"].astype(np.int64), xin)
    if key == "S2":
        assert np.abs(p_uv).max() > 1.0, "rate 1.3 pushes UVs past the map: the zero-padding path"
    REPORT.append(f"fixture {key}: excluded {s['excluded']:.4f} far {s['far']:.3f} masked in {s['masked_in']:.3f}  reference ratios {_fmt(r)}")


# ---- the check itself: the emulation passes, the mutants fail, the cases are the ones described -----------------------------------------------------

@pytest.mark.parametrize("name", list(sf.CASES))
def test_the_case_is_the_one_described_and_the_emulation_passes(name, trace32):
    P = _case(name, trace32)
    s = sf.describe(P)
    mesh, N, K, *_ = sf.CASES[name]
    assert s["N"] == N and s["K"] == min(K, len(P["v"]))
    assert s["excluded"] <= EXCLUDED_CAP, f"{name}: {s['excluded']:.4f} of the rows are undecided for the reference alone"
    assert P["nan"][0], "row 0 sits on a vertex: its normal is 0 / 0"
    if mesh == "star" and K == 2:
        assert s["nan"] > 0.005, "the duplicated pole vertices tie both kept distances"
    r = sf.check(P, *sf.emulate(P, trace32))
    REPORT.append(f"{name:14s} excluded {s['excluded']:.4f} (consistency {s['consistency']:.4f}, small sum w {s['small_wsum']:.4f}) nan {s['nan']:.4f} far {s['far']:.3f} "
                  f"masked in {s['masked_in']:.3f}  emulation ratios {_fmt(r)}")


@pytest.mark.parametrize("mutant", sf.MUTANTS)
def test_a_wrong_lookup_fails_the_check(mutant, trace32):
    caught = []
    for name in ("height_scaled", "height_far", "star_k8"):
        P = _case(name, trace32)
        try:
            sf.check(P, *sf.emulate(P, trace32, mutate=mutant))
        except AssertionError as e:
            caught.append(f"{name}: {str(e)[:100]}")
    assert caught, f"the mutant {mutant} passes every case"
    REPORT.append(f"mutant {mutant:15s} caught by {len(caught)} of 3 cases; {caught[0]}")


def test_the_normal_emulation_follows_the_float64_chain():
    P = sf.problem("star_k8")
    emu = sf.normal_emulation(P["x"], P["idx"], P["dis"], P["v"], P["vn"])
    ok = ~P["nan"]
    assert np.isnan(emu[P["nan"]]).all() and np.isfinite(emu[ok]).all()
    assert np.median(np.abs(emu[ok] - P["normal"][ok]).max(1)) < 1e-6


# ---- the preprocessing ----------------------------------------------------------------------------------------------------------------------------------

def test_the_preprocessing_gives_the_fixtures_mesh(golden):
    from ngp_harness.curved import shape_preprocess

    v, uv, face_uv, factor = shape_preprocess(golden["vertices_raw"], golden["faces"], golden["uvs_raw"])
    assert v.dtype == np.float32 and np.array_equal(v, golden["vertices"])
    assert uv.dtype == np.float32 and np.array_equal(uv, golden["uvs"]) and uv.min() == -1.0 and uv.max() == 1.0
    assert face_uv.shape == (len(golden["faces"]), 6) and np.array_equal(face_uv.reshape(-1, 3, 2), golden["uvs"][golden["faces"].astype(np.int64)])
    assert abs(factor / float(golden["recommended_sdf_factor"]) - 1) < 1e-6
    v2, _, _, _ = shape_preprocess(golden["vertices"], golden["faces"], golden["uvs_raw"], normalize=False)
    assert np.array_equal(v2, golden["vertices"])


def test_the_op_by_op_normal_is_the_float64_normal():
    from ngp_harness.curved import shape_knn_normal

    P = sf.problem("star_k8")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    n = shape_knn_normal(t(P["x"]), t(P["idx"]), t(P["dis"]), t(P["v"]), t(P["vn"])).numpy()
    ok = ~P["nan"]
    assert np.isnan(n[P["nan"]]).all(), "0 / 0 is NaN in the reference's expressions"
    assert (np.abs(n[ok] - P["normal"][ok]).max(1) <= P["tol_normal"][ok]).all()


# ---- the state machine ----------------------------------------------------------------------------------------------------------------------------------

def _bare_field(h_threshold=0.0625):
    """A CurvedField without its mesh structures (they need a device)."""
    from ngp_harness.curved import CurvedField

    f = object.__new__(CurvedField)
    torch.nn.Module.__init__(f)
    f.normal_net, f.light_model, f.multires, f.h_threshold, f.in_dim = None, None, 12, h_threshold, 41
    f.encoder = types.SimpleNamespace(output_dim=16)
    f.sigma_net = types.SimpleNamespace(weights=torch.zeros(1), dtype=torch.float16)
    f.projector = types.SimpleNamespace(h_threshold=h_threshold)
    f._init_import_state()
    return f


def _fake_shape(f):
    """the state import_shape leaves, with stand-ins for the device structures"""
    handle = types.SimpleNamespace(value=1)
    f.shape_projector = types.SimpleNamespace(mesh_vertices=torch.zeros(4, 3), vertex_normals=torch.zeros(4, 3), _knn=handle, tracer=types.SimpleNamespace(_handle=handle))
    f.shape_face_uv = torch.zeros(2, 6)
    f.imported, f.imported_type = True, "shape"


def test_import_shape_needs_a_map_and_refuses_what_import_field_refuses():
    f = _bare_field()
    v, faces = sf.quad_mesh()
    with pytest.raises(RuntimeError, match="imported first"):
        f.import_shape(v, faces, v[:, :2])
    with pytest.raises(RuntimeError, match="no shape has been imported"):
        f.switch_shape_feature()
    f.import_field(pf.seeded_map(5, 4), 1 / 32)
    with pytest.raises(RuntimeError, match="no shape has been imported"):
        f.switch_shape_feature()
    f.normal_net = object()
    with pytest.raises(NotImplementedError, match="phi_embed.*local_tbn.*sample_tbn"):
        f.import_shape(v, faces, v[:, :2])
    f.normal_net, f.light_model = None, "SH"
    with pytest.raises(NotImplementedError, match="phi_embed"):
        f.import_shape(v, faces, v[:, :2])


def test_the_setters_and_switches_change_the_stamp_and_the_effective_scale():
    f = _bare_field()
    assert f.K_for_uv == 5 and f.sdf_scale_factor == 1.0 and f.imported_type is None and f._import_stamp() == ()
    f.import_field(pf.seeded_map(5, 4), 1 / 32)
    assert f.imported_type == "field"
    field_stamp = f._import_stamp()
    _fake_shape(f)
    seen = [field_stamp, f._import_stamp()]
    assert seen[1][0] == "import-shape" and seen[1] != seen[0]
    for change in (lambda: f.set_k_for_uv(3), lambda: f.set_sdf_factor(2.0), lambda: f.set_uv_utilize_rate(1.3), lambda: f.set_sdf_offset(0.01),
                   lambda: f.set_h_threshold(0.03)):
        change()
        assert f._import_stamp() not in seen
        seen.append(f._import_stamp())
    K, scale, off, rate, h = f._shape_scalars()
    assert (K, off, rate, h) == (3, 0.01, 1.3, 0.03) and scale == float(np.float32(2.0 / 1.3))
    f.set_k_for_uv(16)
    assert f._shape_scalars()[0] == 4, "K is clamped to the number of vertices"
    f.set_sdf_factor(0.0)
    assert f._shape_scalars()[1] == float(np.float32(1e-5)), "the reference's max(1e-5, sdf_scale)"
    f.switch_shape_feature()
    assert f.imported_type == "field" and f._import_stamp()[0] == "import" and f._import_stamp() not in seen
    f.switch_shape_feature()
    assert f.imported_type == "shape" and f._import_stamp() not in seen
    f.switch_import()
    assert not f.imported and f._import_stamp() == ()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------------

def _struct_fields():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nerftex_curved_shape_infer_desc \{(.*?)\} nerftex_curved_shape_infer_desc;", src, flags=re.S).group(1)
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
    assert [n for n, _ in nerftex_hip.CurvedShapeInferDesc._fields_] == fields
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {",
             '    printf("sizeof %lu\\n", (unsigned long)sizeof(nerftex_curved_shape_infer_desc));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof(nerftex_curved_shape_infer_desc, {n}));' for n in fields]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(nerftex_hip.CurvedShapeInferDesc)
    for n in fields:
        assert int(out[n]) == getattr(nerftex_hip.CurvedShapeInferDesc, n).offset, n


def test_scratch_query():
    from nerftex_hip import lib

    sizes = [lib.nerftex_curved_shape_infer_scratch_bytes(b) for b in (0, 128, 256, 1 << 20)]
    assert sizes[0] == 0 and sizes[1] > 0 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    # the neighbour list (16 ids and 16 distances), mask, normal, the two networks' inputs and outputs, the raw density
    assert sizes[3] == (1 << 20) * (64 + 64 + 1 + 12 + 96 + 32 + 2 + 64 + 32)


FAKE = 0x10000  # a non-NULL address that is never dereferenced: every case below is refused before the raytracer is looked at


def _desc(**over):
    from nerftex_hip import CurvedShapeInferDesc

    kw = dict(B=128, n_verts=4, n_faces=2, K=5, map_h=24, map_w=20, n_features=16, sdf_scale=1.0, sdf_offset=0.0, uv_rate=1.0, h_threshold=0.0625, n_freqs=12,
              sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16, color_in=32, color_hidden=64, color_layers=3, color_out=3, fc_weight=1.0, eval=3,
              scratch_bytes=1 << 40, tracer=None)
    kw.update({name: FAKE for name in ("knn", "xyz", "dirs", "mesh_vertices", "vertex_normals", "face_uv", "map", "sigma_weights", "color_weights", "sigma", "rgbs", "scratch")})
    kw.update(over)
    return CurvedShapeInferDesc(**kw)


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
    (dict(), "a raytracer is required"),  # (a NULL raytracer: behind the shapes, in front of the map)
    (dict(map_h=0), "a raytracer is required"),
]


@pytest.mark.parametrize("over,text", REFUSED, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) or "null-tracer" if isinstance(v, dict) else None)
def test_the_chain_refuses_before_any_launch(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_curved_shape_infer(ctypes.byref(_desc(**over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_the_chain_null_descriptor_and_the_plain_entrys_null_pointers():
    from nerftex_hip import lib

    assert lib.nerftex_curved_shape_infer(None, None) == NERFTEX_ERR_INVALID
    assert "NULL descriptor" in lib.nerftex_last_error().decode()
    args = [None, FAKE, FAKE, FAKE, 5, 5, FAKE, FAKE, 4, FAKE, 2, FAKE, 24, 20, 1.0, 0.0, 1.0, 0.0625, 12, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None]
    assert lib.nerftex_shape_lookup(*args) == NERFTEX_ERR_INVALID  # (a NULL raytracer: the first refusal, nothing is dereferenced)
    assert "must not be NULL" in lib.nerftex_last_error().decode()
