"""An imported feature patch under the curved field, the CPU side (no GPU): the reference fixtures tests/golden/ref_python_import_patch.npz and
ref_python_import_patch_sh.npz (tools/make_golden.py: import_patch_goldens, import_patch_sh_goldens) lie inside the float64 model's bound
(tests/patch_import_float64.py), CurvedField._patch_embed_reference reproduces them, the model refuses deliberately wrong lookups, the
undecided share of every shared case is under its cap, and the state machine, the binding and the refusals that need no device."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import import_light_float64 as il64
import patch_import_float64 as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
NERFTEX_ERR_INVALID = 1
UNDECIDED_CAP = 0.02


def _bare_field(lit=False, h_threshold=pm.H_THRESHOLD):
    """A CurvedField without its mesh, tables and networks: what the import state and the 'patch' branch read."""
    from ngp_harness.curved import CurvedField, FactorizedNormalNet

    f = object.__new__(CurvedField)
    torch.nn.Module.__init__(f)
    f.light_model, f.multires, f.h_threshold, f.in_dim, f.fc_weight = ("SH" if lit else None), 12, h_threshold, 41, 1.0
    f.encoder = types.SimpleNamespace(output_dim=16)
    f.sigma_net = types.SimpleNamespace(weights=torch.zeros(1), dtype=torch.float16)
    f.projector = types.SimpleNamespace(h_threshold=h_threshold)
    f.normal_net = FactorizedNormalNet(x_dim=16, z_dim=25) if lit else None
    f.light_visual_mode, f.smooth_grad_weight, f.encoder_var = "Full", 1e-1, None
    f._init_import_state()
    return f.eval()


def _golden(lit):
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_import_patch_sh.npz" if lit else "ref_python_import_patch.npz"))


def _golden_field(g, lit):
    f = _bare_field(lit, float(g["h_threshold"]))
    if lit:
        il64.load_normal_net(f.normal_net, g)
        f.import_patch(features=g["features"], points=g["points"], normals=g["normals"], local_tbn=g["local_tbn"], phi_embed=g["phi_embed"])
    else:
        f.import_patch(features=g["features"], points=g["points"], normals=g["normals"])
    return f


def _model(g, idx, lit):
    normals = np.ascontiguousarray(np.broadcast_to(g["normals"], g["points"].shape))
    return pm.resample(g["points"], normals, g["features"], g["xyz"], idx, float(g["h_threshold"]), g["phi_embed"] if lit else None, g["local_tbn"] if lit else None)


# ---- the fixtures, the model and the op-by-op route ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lit", [False, True], ids=["static", "lit"])
def test_the_fixture_lies_inside_the_models_bound(lit):
    """On the exact neighbour set: every element of the embedding (features and ladder, narrowed to half as the networks read them) and of the
    coarse normal on the rows that pass the direct-above test, the mask on every decided row; rows that fail it are outside the mask."""
    g = _golden(lit)
    idx, _ = pm.bruteforce_neighbours(g["points"], g["xyz"])
    pm.check_neighbours(g["points"], g["xyz"], idx)
    m = _model(g, idx, lit)
    rows, decided = m["compare"], ~m["undecided"]
    assert m["undecided"].mean() <= UNDECIDED_CAP and all(min(s) > 20 for s in m["sides"]), (m["undecided"].mean(), m["sides"])
    pm.assert_within(g["embed"].astype(np.float16), m["embed"], rows, "the fixture's embedding, narrowed")
    pm.assert_within(g["embed"][:, 16], m["sdf"], rows, "the fixture's height")
    unit = m["normal"][0] / (np.linalg.norm(m["normal"][0], axis=-1, keepdims=True) + 1e-5)
    pm.assert_within(g["normal"], (unit, m["normal"][1] * 2 + 4 * pm.U), rows, "the fixture's coarse normal (normalised once more: twice the bound and the division's roundings)")
    assert np.array_equal(g["h_mask"][decided], m["mask"][decided])
    assert not g["h_mask"][~m["above"] & decided].any() and (g["embed"][~m["above"] & decided][:, 16] == 0).all()
    print(f"{'lit' if lit else 'static'}: {int(rows.sum())} rows compared, {int(m['undecided'].sum())} undecided, sides {m['sides']}, median bound on the height "
          f"{np.median(m['sdf'][1][rows]):.2e}, on a feature {np.median(m['embed'][1][rows][:, :16]):.2e}")


@pytest.mark.parametrize("lit", [False, True], ids=["static", "lit"])
def test_the_op_by_op_route_reproduces_the_fixture(lit):
    g = _golden(lit)
    f = _golden_field(g, lit)
    x = torch.from_numpy(g["xyz"])
    with torch.no_grad():
        out = f.embed(x, with_fine_normal=lit)
        details = f._patch_embed_reference(x, with_fine_normal=lit, details=True)
    embed, normal, mask = out[:3]
    idx = details[(4 if lit else 3) + 2].numpy()
    pm.check_neighbours(g["points"], g["xyz"], idx)
    m = _model(g, idx, lit)
    rows, decided = m["compare"], ~m["undecided"]
    assert m["undecided"].mean() <= UNDECIDED_CAP, "the op-by-op route stays within the undecided share on the fixture's points"
    pm.assert_within(embed.half().numpy(), m["embed"], rows, "the op-by-op embedding")
    pm.assert_within(embed.numpy(), (g["embed"].astype(np.float64), m["embed"][1]), rows, "the op-by-op embedding against the fixture's")
    assert np.array_equal(mask.numpy()[decided], g["h_mask"][decided])
    assert np.abs(normal.numpy() - g["normal"])[rows].max() <= 1e-5
    if lit:
        err = np.abs(out[3].numpy() - g["normal_fine"])[g["h_mask"] & decided]
        print(f"fine normal: max |diff| to the fixture {err.max():.2e} (bar 5e-3, the lit import tests' for this chain's normals)")
        assert err.max() <= 5e-3


def test_the_model_refuses_wrong_lookups():
    """The bound is tight enough to tell the squared in-plane distance from :438's norm of squares, the Shepard weights from the dual-distance
    ones, and a neighbour set with a wrong point from a legitimate one.  (It is NOT tight enough to see the 1e-5 of the weights' normalisation:
    3e-6 of a weight, inside the bound of most rows.)"""
    patch = pm.seeded_patch(12, True, lit=True)
    x = pm.case_queries(patch, 400)
    idx, _ = pm.bruteforce_neighbours(patch["points"], x)
    normals = pm.full_normals(patch)
    m = pm.resample(patch["points"], normals, patch["features"], x, idx, pm.H_THRESHOLD, patch["phi_embed"], patch["local_tbn"])
    rows = m["compare"]
    p = patch["points"].astype(np.float64)[idx]
    dv = x.astype(np.float64)[:, None] - p
    normal = m["normal"][0]
    s = (dv * normal[:, None]).sum(-1)
    r = dv - s[..., None] * normal[:, None]

    def weights(t):
        dk, d1 = t.max(-1, keepdims=True), t.min(-1, keepdims=True)
        w = (dk - t) / (dk - d1 + 1e-5) * (dk + d1) / (dk + t)
        return w / (w.sum(-1, keepdims=True) + 1e-5)

    right = weights(np.sqrt(((r * r) ** 2).sum(-1)))
    pm.assert_within(right, m["weights"], rows, "the restated weights")
    shepard = 1 / (np.sqrt((dv * dv).sum(-1)) + 1e-7)
    for name, wrong in (("squared in-plane distance", weights((r * r).sum(-1))), ("Shepard weights", shepard / shepard.sum(-1, keepdims=True))):
        with pytest.raises(AssertionError):
            pm.assert_within(wrong, m["weights"], rows, name)
    bad = idx.copy()
    bad[:, 7] = (bad[:, 7] + 60) % len(patch["points"])
    with pytest.raises(AssertionError):
        pm.check_neighbours(patch["points"], x, bad)


@pytest.mark.parametrize("S", pm.SIZES)
@pytest.mark.parametrize("per_point", [False, True], ids=["one_normal", "per_point_normals"])
def test_the_shared_cases_are_decided_and_hold_both_sides(S, per_point):
    """The cases tests/test_gpu_import_patch.py runs: the op-by-op route on the CPU inside the bound, its undecided share under the cap, decided
    rows on both sides of each of the three tests (B >= 200), and V = 9 drops exactly one point per query."""
    patch = pm.seeded_patch(S, per_point, lit=True)
    f = _bare_field(True)
    f.import_patch(**patch)
    for B in (1, 200, 1000):
        xn = pm.case_queries(patch, B)
        with torch.no_grad():
            embed, nc, mask, fine, sdf, normal, idx, dis, w, phi, tbn = f._patch_embed_reference(torch.from_numpy(xn), with_fine_normal=True, details=True)
        idx = idx.numpy()
        pm.check_neighbours(patch["points"], xn, idx)
        if S == 3:
            assert all(len(set(range(9)) - set(row.tolist())) == 1 for row in idx)
        m = pm.resample(patch["points"], pm.full_normals(patch), patch["features"], xn, idx, pm.H_THRESHOLD, patch["phi_embed"], patch["local_tbn"])
        rows, decided = m["compare"], ~m["undecided"]
        assert m["undecided"].mean() <= UNDECIDED_CAP
        if B >= 200:
            assert all(min(side) > 0 for side in m["sides"]), m["sides"]
        else:
            assert m["above"].all() and m["mask"].all(), "the single row passes all three tests"
        for name, got, key in (("normal", normal, "normal"), ("sdf", sdf, "sdf"), ("weights", w, "weights"), ("embed", embed.half(), "embed"), ("phi", phi, "phi"),
                               ("tbn", tbn.reshape(-1, 9), "tbn")):
            pm.assert_within(got.numpy(), m[key], rows, f"{name} S={S} B={B}")
        assert np.array_equal(mask.numpy()[decided], m["mask"][decided])
        assert not mask.numpy()[~m["above"] & decided].any()


# ---- state handling ---------------------------------------------------------------------------------------------------------------------------------------

def _field_dict(P=3, S=4, lit=True, seed=1):
    rng = np.random.default_rng(seed)
    d = dict(patches=rng.normal(size=(P, S, S, 16)).astype(np.float32), patch_coors=rng.normal(size=(P, S, S, 3)).astype(np.float32),
             patch_norms=rng.normal(size=(P, 3)).astype(np.float32), patch_local_tbn=rng.normal(size=(P, S, S, 9)).astype(np.float32),
             patch_phi_embed=rng.normal(size=(P, S, S, 8)).astype(np.float32) if lit else None, grid_gap=0.1)
    return d


def _state(f):
    return (f.imported, f.imported_type, f.patch_id, f._import_version, f.features_imported, f.patch_points, f.patch_geom, f.patch_lit, f._patch_knn)


@pytest.mark.parametrize("lit", [False, True], ids=["static", "lit"])
def test_the_counter_and_the_field_dict_against_explicit_arrays(lit):
    f, d = _bare_field(lit), _field_dict(lit=lit)
    assert f.patch_id == 0 and f.imported_type is None and f._patch_knn is None
    for k in range(5):  # the reference's counter: modulo the patch count, advanced after the import
        f.import_patch(d)
        assert f.imported and f.imported_type == "patch" and f.patch_id == k % 3 + 1
        assert torch.equal(f.features_imported, torch.from_numpy(d["patches"][k % 3].reshape(-1, 16)))
    f.import_patch(d, 1)
    assert f.patch_id == 2, "an explicit patch_id leaves the counter alone"
    g = _bare_field(lit)
    more = dict(local_tbn=d["patch_local_tbn"][1].reshape(-1, 3, 3), phi_embed=d["patch_phi_embed"][1].reshape(-1, 8)) if lit else {}
    g.import_patch(features=d["patches"][1].reshape(-1, 16), points=torch.from_numpy(d["patch_coors"][1].reshape(-1, 3)), normals=d["patch_norms"][1], **more)
    assert g.patch_id == 0
    for name in ("features_imported", "patch_points", "patch_normals", "patch_geom", "patch_lit", "patch_phi_embed", "patch_local_tbn"):
        a, b = getattr(f, name), getattr(g, name)
        assert (a is None and b is None and not lit) or torch.equal(a, b), name
    assert f.patch_geom.shape == (16, 8) and bool((f.patch_geom[:, 3] == 0).all()) and bool((f.patch_geom[:, 7] == 0).all())
    assert torch.equal(f.patch_geom[:, 4:7], torch.from_numpy(d["patch_norms"][1]).expand(16, 3)), "the one patch normal at every point"
    if lit:
        assert f.patch_lit.shape == (16, 20) and bool((f.patch_lit[:, 17:] == 0).all())
        assert torch.equal(f.patch_lit[:, :8], f.patch_phi_embed) and torch.equal(f.patch_lit[:, 8:17], f.patch_local_tbn)
    per_point = np.random.default_rng(2).normal(size=(16, 3)).astype(np.float32)
    g.import_patch(features=d["patches"][0].reshape(-1, 16), points=d["patch_coors"][0].reshape(-1, 3), normals=per_point, **more)
    assert torch.equal(g.patch_geom[:, 4:7], torch.from_numpy(per_point))


def test_refusals_leave_the_state_untouched():
    d = _field_dict()
    ok = dict(features=d["patches"][0].reshape(-1, 16), points=d["patch_coors"][0].reshape(-1, 3), normals=d["patch_norms"][0])
    lit_ok = dict(ok, local_tbn=d["patch_local_tbn"][0].reshape(-1, 9), phi_embed=d["patch_phi_embed"][0].reshape(-1, 8))
    nan_points = ok["points"].copy()
    nan_points[3, 1] = np.nan
    for lit, first in ((False, ok), (True, lit_ok)):
        f = _bare_field(lit)
        f.import_patch(**first)
        before = _state(f)
        cases = [(ValueError, dict(field_dict=d, **ok)), (ValueError, dict()), (ValueError, dict(features=ok["features"])), (ValueError, dict(patch_id=0, **first)),
                 (ValueError, dict(field_dict=d, patch_id=3)), (ValueError, dict(field_dict=d, patch_id=-1)),
                 (ValueError, dict(field_dict={k: v for k, v in d.items() if k != "patch_norms"})),
                 (ValueError, dict(first, features=ok["features"][:, :8])), (ValueError, dict(first, features=ok["features"][:7], points=ok["points"][:7])),
                 (ValueError, dict(first, points=ok["points"][:9])), (ValueError, dict(first, points=nan_points)), (ValueError, dict(first, normals=np.zeros((4, 3), np.float32)))]
        if lit:
            cases += [(NotImplementedError, ok), (ValueError, dict(ok, phi_embed=lit_ok["phi_embed"])), (ValueError, dict(lit_ok, phi_embed=lit_ok["phi_embed"][:, :4])),
                      (ValueError, dict(lit_ok, local_tbn=lit_ok["local_tbn"][:, :6])), (NotImplementedError, dict(field_dict=dict(d, patch_phi_embed=None)))]
        else:
            cases += [(ValueError, lit_ok), (ValueError, dict(ok, phi_embed=lit_ok["phi_embed"]))]
        for error, kw in cases:
            with pytest.raises(error, match="CurvedField.import_patch"):
                f.import_patch(**kw)
            after = _state(f)
            assert all(a is b or a == b for a, b in zip(before, after)), kw.keys()
    _bare_field(False).import_patch(d)  # (a static field reads a lit field's dict: the frames and phi are not looked at)


def test_the_interplay_with_import_field_switch_import_and_import_shape():
    f, d = _bare_field(False), _field_dict(lit=False)
    with pytest.raises(RuntimeError):
        f.switch_import()
    f.import_patch(d)
    assert f._patch_active() and not f._shape_active()
    with pytest.raises(RuntimeError, match="import_field"):
        f.import_shape(np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int64), np.zeros((3, 2), np.float32))  # (no map has been imported)
    with pytest.raises(RuntimeError):
        f.switch_shape_feature()
    with pytest.raises(NotImplementedError):
        f.embed(torch.zeros(4, 3), requires_grad_xyz=True)
    with pytest.raises(NotImplementedError):
        f.embed(torch.zeros(4, 3), with_fine_normal=True)
    f.switch_import()
    assert not f.imported and f.imported_type == "patch" and f._import_stamp() == () and not f._patch_active()
    f.switch_import()
    assert f._patch_active()
    f.import_field(np.zeros((3, 2, 16), np.float32), 0.5)  # replaces the patch
    assert f.imported and f.imported_type == "field" and f.features_imported.shape == (3, 2, 16) and f._import_stamp()[0] == "import"
    f.import_patch(d)  # ... and the other way round
    assert f.imported_type == "patch" and f.features_imported.shape == (16, 16) and f.patch_id == 2


def test_the_stamp_changes_with_everything_a_graph_bakes_in():
    f, d = _bare_field(True), _field_dict()
    assert f._import_stamp() == ()
    seen = []
    for change in (lambda: f.import_patch(d), lambda: f.import_patch(d), lambda: f.import_patch(d, 0), lambda: f.set_h_threshold(0.03)):
        change()
        stamp = f._import_stamp()
        assert stamp[0] == "import-patch" and stamp not in seen
        seen.append(stamp)
    assert f.h_threshold == 0.03
    f.switch_import()
    assert f._import_stamp() == ()


def test_the_new_rungs_skip_every_other_field():
    f = _bare_field(True)
    x = torch.zeros(128, 3)
    assert f._infer_patch_fused(x, x) is False and f._infer_light_patch_fused(x, x) is False
    f.import_field(np.zeros((3, 2, 16), np.float32), 0.5, phi_embed=np.zeros((3, 2, 8), np.float32), local_tbn=np.zeros((3, 2, 9), np.float32),
                   sample_tbn=np.eye(3, dtype=np.float32)[None], sample_tbn_ids=np.zeros((3, 2), np.float32))
    assert f._infer_patch_fused(x, x) is False and f._infer_light_patch_fused(x, x) is False
    f.import_patch(_field_dict())
    assert f._infer_route(x, x) is None, "a patch on the CPU: forward(), and never the planar chain over the maps of the earlier import_field"


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------------------------

DESCS = {"nerftex_curved_patch_infer_desc": "CurvedPatchInferDesc", "nerftex_curved_light_patch_infer_desc": "CurvedLightPatchInferDesc"}


def _struct_fields(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", src, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            names.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", first.strip()).group(1))
            names += [m.strip() for m in more]
    return names


@pytest.mark.parametrize("c_name", sorted(DESCS))
def test_the_descriptors_are_bound_field_for_field_with_the_compilers_layout(tmp_path, c_name):
    import subprocess

    import nerftex_hip

    cls = getattr(nerftex_hip, DESCS[c_name])
    fields = _struct_fields(c_name)
    assert [n for n, _ in cls._fields_] == fields
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {", f'    printf("sizeof %lu\\n", (unsigned long)sizeof({c_name}));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof({c_name}, {n}));' for n in fields]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(cls)
    for n in fields:
        assert int(out[n]) == getattr(cls, n).offset, n


def test_the_symbols_and_the_constants():
    import nerftex_hip

    header = open(HEADER).read()
    for name in ("nerftex_patch_lookup", "nerftex_patch_light_lookup", "nerftex_curved_patch_infer", "nerftex_curved_light_patch_infer",
                 "nerftex_curved_patch_infer_scratch_bytes", "nerftex_curved_light_patch_infer_scratch_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header) and hasattr(ctypes.CDLL(nerftex_hip.LIB_PATH), name) and name in nerftex_hip.EXPORTS, name
    assert (nerftex_hip.PATCH_GEOM_STRIDE, nerftex_hip.PATCH_LIT_STRIDE) == (8, 20)
    assert re.search(r"#define NERFTEX_PATCH_GEOM_STRIDE 8\b", header) and re.search(r"#define NERFTEX_PATCH_LIT_STRIDE 20\b", header)


def test_scratch_queries():
    from nerftex_hip import lib

    for entry, per_row in ((lib.nerftex_curved_patch_infer_scratch_bytes, 1 + 12 + 96 + 32 + 2 + 64 + 32),
                           # the lit chain: mask, normal, the sigma net's input and output, phi (half), the weighted frame, raw density, the BRDF net's input and output, the shading normal
                           (lib.nerftex_curved_light_patch_infer_scratch_bytes, 1 + 12 + 96 + 32 + 16 + 36 + 4 + 32 + 32 + 12)):
        sizes = [entry(b) for b in (0, 128, 256, 1 << 20)]
        assert sizes[0] == 0 and sizes[1] > 0 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
        assert sizes[3] == (1 << 20) * per_row
    assert lib.nerftex_curved_patch_infer_scratch_bytes(384) == lib.nerftex_curved_import_infer_scratch_bytes(384), "the planar chain's buffers"


class _Grid(ctypes.Structure):
    """A stand-in for the neighbour grid's host-side record (csrc/knn.hip: struct nerftex_knn) for the refusals, which read its point count and
    nothing else: no device is needed to build it, and every case below is refused before a device pointer is looked at."""
    _fields_ = [("cell_start", ctypes.c_void_p), ("points", ctypes.c_void_p), ("n_points", ctypes.c_uint32), ("dims", ctypes.c_int * 3), ("lo", ctypes.c_float * 3),
                ("cell", ctypes.c_float), ("inv_cell", ctypes.c_float), ("eps", ctypes.c_float), ("device", ctypes.c_int)]


FAKE = 0x10000  # a non-NULL, 16-byte aligned address that is never dereferenced
GRID = _Grid(n_points=144)
GRID7 = _Grid(n_points=7)
INF = float("inf")


def _desc(is_lit, **over):
    import nerftex_hip

    kw = dict(knn=ctypes.addressof(GRID), B=128, n_points=144, n_features=16, h_threshold=0.0625, n_freqs=12, sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16,
              fc_weight=1.0, eval=1 if is_lit else 3, scratch_bytes=1 << 40)
    names = ["xyz", "dirs", "geom", "features", "sigma_weights", "sigma", "rgbs", "scratch"]
    if is_lit:
        kw.update(n_phi=8, normal_hidden=16, normal_layers=2, brdf_in=16, brdf_hidden=64, brdf_layers=3, brdf_out=5, n_sh=16, n_color=1, gamma=2.2, flags=1, visual_mode=0)
        names += ["lit", "normal_weights", "normal_biases", "brdf_weights", "env_shs"]
    else:
        kw.update(color_in=32, color_hidden=64, color_layers=3, color_out=3)
        names += ["color_weights"]
    kw.update({name: FAKE for name in names})
    kw.update(over)
    return (nerftex_hip.CurvedLightPatchInferDesc if is_lit else nerftex_hip.CurvedPatchInferDesc)(**kw)


# in the header's order; every case carries the later cases' faults too where it can, to pin the order
CHAIN_REFUSED = [
    (dict(B=100, knn=None), "multiple of 128"),
    (dict(knn=None, n_features=8), "a neighbour grid over the patch's points is required"),
    (dict(n_points=143, n_features=8), "n_points must be its point count (144)"),
    (dict(knn=ctypes.addressof(GRID7), n_points=7, sigma_hidden=64), "between 8 and 2^31 - 1 points"),
    (dict(n_features=8, xyz=None), "default"),
    (dict(n_freqs=10, xyz=None), "default"),
    (dict(sigma_hidden=64, xyz=None), "default"),
    (dict(xyz=None, sigma_weights=FAKE + 8), "must not be NULL"),
    (dict(geom=None, h_threshold=0.0), "must not be NULL"),
    (dict(scratch=FAKE + 16, h_threshold=0.0), "256-byte aligned"),
    (dict(scratch_bytes=1000, h_threshold=0.0), "256-byte aligned"),
    (dict(sigma_weights=FAKE + 8, geom=FAKE + 4), "weight vectors must be 16-byte aligned"),
    (dict(geom=FAKE + 4, h_threshold=0.0), "records and xin must be 16-byte aligned"),
    (dict(features=FAKE + 8, h_threshold=0.0), "records and xin must be 16-byte aligned"),
    (dict(h_threshold=0.0), "h_threshold must be positive and finite"),
    (dict(h_threshold=-1.0), "h_threshold must be positive and finite"),
    (dict(h_threshold=INF), "h_threshold must be positive and finite"),
    (dict(h_threshold=float("nan")), "h_threshold must be positive and finite"),
]
STATIC_ONLY = [(dict(color_layers=2, xyz=None), "default"), (dict(color_weights=None, h_threshold=0.0), "must not be NULL"), (dict(color_weights=FAKE + 8, geom=FAKE + 4), "weight vectors")]
LIT_ONLY = [(dict(n_phi=4, n_sh=4), "default"), (dict(brdf_out=3, n_sh=4), "default"), (dict(n_sh=4, xyz=None), "at least 9 SH rows"), (dict(gamma=0.0, xyz=None), "gamma is positive"),
            (dict(eval=2, xyz=None), "eval is 0 or 1"), (dict(lit=None, h_threshold=0.0), "must not be NULL"), (dict(env_shs=None, h_threshold=0.0), "must not be NULL"),
            (dict(normal_weights=FAKE + 2, lit=FAKE + 4), "4-byte aligned"), (dict(lit=FAKE + 4, h_threshold=0.0), "records and xin must be 16-byte aligned")]


def _ids(v):
    return "-".join(f"{k}" for k in v) if isinstance(v, dict) else None


@pytest.mark.parametrize("over,text", CHAIN_REFUSED + STATIC_ONLY, ids=_ids)
def test_the_static_chain_refuses_before_any_launch(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_curved_patch_infer(ctypes.byref(_desc(False, **over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


@pytest.mark.parametrize("over,text", CHAIN_REFUSED + LIT_ONLY, ids=_ids)
def test_the_lit_chain_refuses_before_any_launch(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_curved_light_patch_infer(ctypes.byref(_desc(True, **over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_null_descriptors_and_empty_batches():
    from nerftex_hip import lib

    for lit, entry in ((False, lib.nerftex_curved_patch_infer), (True, lib.nerftex_curved_light_patch_infer)):
        assert entry(None, None) == NERFTEX_ERR_INVALID and "NULL descriptor" in lib.nerftex_last_error().decode()
        assert entry(ctypes.byref(_desc(lit, B=0, xyz=None, scratch=None, h_threshold=0.0)), None) == 0, "B = 0: nothing to do, behind the shapes"
        assert entry(ctypes.byref(_desc(lit, B=0, n_features=8)), None) == NERFTEX_ERR_INVALID


def _plain(is_lit, **over):
    """The argument list of nerftex_patch_lookup / nerftex_patch_light_lookup with stand-in addresses."""
    kw = dict(knn=ctypes.addressof(GRID), xyz=FAKE, geom=FAKE, features=FAKE, lit=FAKE, n_points=144, h_threshold=0.0625, n_freqs=12, B=5, sdf=FAKE, mask=FAKE, normal=FAKE,
              xin=FAKE, idx=FAKE, dis=FAKE, weights=FAKE, phi=FAKE, local_tbn=FAKE)
    kw.update(over)
    order = ["knn", "xyz", "geom", "features"] + (["lit"] if is_lit else []) + ["n_points", "h_threshold", "n_freqs", "B", "sdf", "mask", "normal", "xin", "idx", "dis", "weights"]
    order += ["phi", "local_tbn"] if is_lit else []
    return [kw[k] for k in order] + [None]


PLAIN_REFUSED = [
    (dict(knn=None, n_freqs=10), "a neighbour grid over the patch's points is required"),
    (dict(n_points=100, n_freqs=10), "n_points must be its point count"),
    (dict(knn=ctypes.addressof(GRID7), n_points=7, n_freqs=10), "between 8 and 2^31 - 1"),
    (dict(n_freqs=10, xyz=None), "12 height bands"),
    (dict(xyz=None, geom=None), "inputs and outputs must not be NULL"),
    (dict(weights=None, geom=None), "inputs and outputs must not be NULL"),
    (dict(geom=None, features=FAKE + 4), "records must not be NULL"),
    (dict(features=None, h_threshold=0.0), "records must not be NULL"),
    (dict(features=FAKE + 4, h_threshold=0.0), "16-byte aligned"),
    (dict(xin=FAKE + 8, h_threshold=0.0), "16-byte aligned"),
    (dict(h_threshold=0.0), "h_threshold must be positive and finite"),
    (dict(h_threshold=INF), "h_threshold must be positive and finite"),
]
PLAIN_LIT_ONLY = [(dict(phi=None, geom=None), "inputs and outputs must not be NULL"), (dict(phi=FAKE + 4, geom=None), "phi must be 16-byte aligned"),
                  (dict(lit=None, h_threshold=0.0), "records must not be NULL"), (dict(lit=FAKE + 8, h_threshold=0.0), "16-byte aligned")]


@pytest.mark.parametrize("lit", [False, True], ids=["static", "lit"])
def test_the_plain_entries_refuse_before_any_launch(lit):
    from nerftex_hip import lib

    entry = lib.nerftex_patch_light_lookup if lit else lib.nerftex_patch_lookup
    for over, text in PLAIN_REFUSED + (PLAIN_LIT_ONLY if lit else []):
        assert entry(*_plain(lit, **over)) == NERFTEX_ERR_INVALID, over
        assert text in lib.nerftex_last_error().decode(), (over, lib.nerftex_last_error().decode())
    assert entry(*_plain(lit, B=0, xyz=None, geom=None, h_threshold=0.0)) == 0, "B = 0: nothing to do, behind the patch and n_freqs"
