"""An imported texture under the SH-lit curved field, the CPU side (no GPU): CurvedField.import_field with the four maps of the reference's
`pred_normal` part, the op-by-op route (`_import_light_embed_reference`, `_forward_light` in import mode) and the float64 helper
(tests/import_light_float64.py) against the reference's own run (tests/golden/ref_python_import_field_sh.npz, written by
tools/make_golden.py --import-field-sh-only), the refusals, the graph stamp and the C ABI's declarations."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import import_light_float64 as il64
import planar_float64 as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
NERFTEX_ERR_INVALID = 1
MODES = [("A", 1), ("B", 2)]
FCS = [1.0, 0.7]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_import_field_sh.npz"))


def _bare_field(h_threshold=0.0625, lit=True):
    """A CurvedField without its mesh structures and MLPs (they need a device): the import state and the op-by-op embedding read none of them."""
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


@pytest.fixture(scope="module")
def fields(golden):
    """One field per rescale state, carrying the fixture's normal net; the light head and the sigma net are stand-ins that record what they are
    handed (the MLPs run on the GPU only: tests/test_gpu_import_light.py holds sigma and the colours)."""
    out = {}
    for mode, times in MODES:
        f = _bare_field(float(golden["h_threshold"]))
        il64.load_normal_net(f.normal_net, golden)
        il64.import_fixture_maps(f, golden, times)
        assert f.rescale == (mode == "A")
        out[mode] = f
    return out


def _inside(name, got, want, bound):
    assert np.isfinite(want).all() and np.isfinite(bound).all(), name
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    print(f"{name}: max error / bound {float(ratio.max()):.3f}, max error {float(err.max()):.3e}, median bound {float(np.median(bound)):.3e}")
    assert ratio.max() <= 1.0, (name, float(ratio.max()))


# ---- the op-by-op route against the fixture -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,times", MODES)
def test_the_op_by_op_embedding_reproduces_the_fixture(golden, fields, mode, times):
    """h_mask, the sampled id and both sampled frames exact; the embedding and the sampled phi to 1e-6 (tests/test_import_field_cpu.py's bar for
    the same grid_sample); the fine normal inside the float64 helper's bound for an fp32 evaluation."""
    f = fields[mode]
    x = torch.from_numpy(golden["xyz"])
    with torch.no_grad():
        embed, coarse, mask, fine, phi, local_tbn, ids, sample_inv = f._import_light_embed_reference(x, details=True)
        again = f.embed(x, with_fine_normal=True)
    assert np.array_equal(mask.numpy(), golden[mode + "_h_mask"])
    assert np.array_equal(ids.numpy(), golden[mode + "_id"]) and len(set(ids.tolist())) == 5
    assert np.array_equal(local_tbn.numpy(), golden[mode + "_local_tbn"])
    assert np.array_equal(sample_inv.numpy(), golden[mode + "_sample_tbn_inv"])
    assert np.array_equal(f.sample_tbn_inv_imported.numpy(), golden["sample_tbn_inv"]), "inverted once, in fp32 on the host, as the reference's"
    assert torch.equal(coarse, torch.tensor([0.0, 0.0, 1.0]).expand(512, 3) / (1 + 1e-5))
    assert embed.dtype == torch.float32 and np.abs(embed.numpy() - golden[mode + "_embed"]).max() <= 1e-6
    assert np.abs(phi.numpy() - golden[mode + "_phi"]).max() <= 1e-6
    for a, b in zip(again, (embed, coarse, mask, fine)):
        assert torch.equal(a, b), "embed(with_fine_normal=True) on the CPU is the op-by-op route"
    weights, biases, dweights = il64.pack_fp32(f.normal_net)
    ref = il64.fine_normal(golden[mode + "_phi"], golden[mode + "_embed"][:, :16], golden[mode + "_embed"][:, 16:], weights, biases, golden[mode + "_local_tbn"],
                           golden[mode + "_sample_tbn_inv"], fp32_inputs=True, dweights=dweights)
    _inside(f"{mode} op-by-op normal_fine", fine.numpy(), ref["fine"], ref["bound_fine"])
    got = fine.numpy()[golden[mode + "_h_mask"]]
    assert float(np.abs(got - golden[mode + "_normal_fine"][golden[mode + "_h_mask"]]).max()) < 1e-4, "two fp32 runs of the same expressions"


@pytest.mark.parametrize("fc", FCS)
@pytest.mark.parametrize("mode,times", MODES)
def test_forward_hands_the_fixtures_shading_normal_to_the_head(golden, fields, mode, times, fc):
    """_forward_light in import mode, eval: the normal the head receives, in the four visual modes (the head and the sigma net are stand-ins)."""
    f = fields[mode]
    handed = {}

    def head(geo, normal, d, mask=None):
        handed.update(normal=normal, mask=mask)
        return tuple(torch.full((geo.shape[0], 3), float(i)) for i in range(4))

    f.light_net, f._sigma, f.fc_weight = head, (lambda embed: (torch.ones(embed.shape[0]), torch.zeros(embed.shape[0], 15))), fc
    x, d = torch.from_numpy(golden["xyz"]), torch.from_numpy(golden["dirs"])
    weights, biases, dweights = il64.pack_fp32(f.normal_net)
    ref = il64.fine_normal(golden[mode + "_phi"], golden[mode + "_embed"][:, :16], golden[mode + "_embed"][:, 16:], weights, biases, golden[mode + "_local_tbn"],
                           golden[mode + "_sample_tbn_inv"], fc_weight=fc, blend=True, fp32_inputs=True, dweights=dweights)
    try:
        for i, visual in enumerate(("Full", "Specular", "Diffuse", "Albedo")):
            f.light_visual_mode = visual
            with torch.no_grad():
                sigma, color, ret = f(x, d)
            assert ret == {} and float(color[0, 0]) == float(i), "light_visual_mode picks the head's output"
            assert np.array_equal(handed["mask"].numpy(), golden[mode + "_h_mask"]) and np.array_equal((sigma != 0).numpy(), golden[mode + "_h_mask"])
            _inside(f"{mode} fc={fc} {visual} op-by-op shading normal", handed["normal"].numpy(), ref["normal"], ref["bound_normal"])
    finally:
        f.light_visual_mode = "Full"
        del f.light_net, f._sigma


# ---- the float64 helper ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,times", MODES)
def test_the_float64_helper_checks_itself_against_the_fixture(golden, fields, mode, times):
    """The reference's own normal_fine and shading normals (an fp32 run: no half rounding anywhere) inside the helper's bound widened for fp32
    inputs, on every row; the bound stays a small fraction of a unit vector's component; the second rotation is applied and is not the
    transpose's."""
    f = fields[mode]
    weights, biases, dweights = il64.pack_fp32(f.normal_net)
    args = (golden[mode + "_phi"], golden[mode + "_embed"][:, :16], golden[mode + "_embed"][:, 16:], weights, biases, golden[mode + "_local_tbn"])
    inv = golden[mode + "_sample_tbn_inv"]
    ref = il64.fine_normal(*args, inv, fp32_inputs=True, dweights=dweights)
    _inside(f"{mode} fixture normal_fine", golden[mode + "_normal_fine"], ref["fine"], ref["bound_fine"])
    for fc in FCS:
        ev = il64.fine_normal(*args, inv, fc_weight=fc, blend=True, fp32_inputs=True, dweights=dweights)
        _inside(f"{mode} fc={fc} fixture shading normal", golden[f"{mode}_fc{fc}_shading_normal"], ev["normal"], ev["bound_normal"])
    assert float(np.median(ref["bound_fine"])) < 0.05
    tight = il64.fine_normal(*args, inv)
    assert (tight["bound_fine"] <= ref["bound_fine"]).all(), "the fp32-input terms only widen"
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), inv.shape)
    one = il64.fine_normal(*args, eye)
    assert float(np.abs(one["fine"] - ref["fine"]).max()) > 0.1, "the second rotation moves the normal"
    transposed = il64.fine_normal(*args, np.swapaxes(golden["sample_tbn"][golden[mode + "_id"]], 1, 2))
    assert float(np.abs(transposed["fine"] - ref["fine"]).max()) > 0.05, "the inverse is not the transpose: the frames are not orthonormal"
    blended = il64.fine_normal(*args, inv, fc_weight=0.7, blend=True)
    assert float(np.abs(blended["normal"] - ref["normal"]).max()) > 5e-2, "the blend moves the normal by more than its bound"


def test_the_helper_without_input_errors_is_normal_net_float64s():
    """Its LipMLP with zero input error is nn64.lip_mlp, and with an identity second frame it is nn64.fine_normal's rotation, value for value."""
    import normal_net_float64 as nn64

    rng = np.random.default_rng(5)
    B = 64
    phi_feat, x_feat = rng.uniform(-0.5, 0.5, (B, 8)).astype(np.float16), rng.uniform(-0.5, 0.5, (B, 16)).astype(np.float16)
    z = rng.uniform(-1, 1, (B, 25)).astype(np.float16)
    weights = {k: [rng.normal(0, 0.4, s).astype(np.float16).astype(np.float64) for s in shapes] for k, shapes in nn64.SHAPES.items()}
    biases = {k: [rng.normal(0, 0.2, s[0]) for s in shapes] for k, shapes in nn64.SHAPES.items()}
    tbn = rng.normal(size=(B, 3, 3)).astype(np.float32)
    a = nn64.fine_normal(phi_feat, x_feat, z, weights, biases, tbn=tbn)
    b = il64.fine_normal(phi_feat, x_feat, z, weights, biases, tbn, np.broadcast_to(np.eye(3, dtype=np.float32), tbn.shape))
    assert np.array_equal(a["phi"], b["phi"]) and np.array_equal(a["theta"], b["theta"]) and np.array_equal(a["bound_local"], b["bound_local"])
    assert np.array_equal(a["normal"], b["normal"]), "a unit second frame multiplies exactly: the same normal"
    assert (b["bound_normal"] >= a["bound_normal"]).all(), "... under a bound that carries the second product's terms"


# ---- the import state: refusals, stamp ----------------------------------------------------------------------------------------------------------------

def _maps(H=2, W=3, P=3):
    phi, local, sample, ids = il64.seeded_light_maps(H, W, P)
    return dict(phi_embed=phi, local_tbn=local, sample_tbn=sample, sample_tbn_ids=ids)


def test_a_lit_field_imports_with_the_four_maps_and_refuses_without():
    f = _bare_field()
    with pytest.raises(NotImplementedError, match="phi_embed.*local_tbn.*sample_tbn"):
        f.import_field(pf.seeded_map(2, 3), 0.5)
    assert not f.imported and f.features_imported is None
    f.light_model = None  # (a normal net without a light model: the same)
    with pytest.raises(NotImplementedError, match="phi_embed"):
        f.import_field(pf.seeded_map(2, 3), 0.5)
    f = _bare_field()
    m = _maps()
    f.import_field(pf.seeded_map(2, 3), 0.5, **m)
    assert f.imported and f.rescale and f.imported_type == "field"
    assert tuple(f.phi_embed_imported.shape) == (2, 3, 8) and tuple(f.local_tbn_imported.shape) == (2, 3, 9) and tuple(f.sample_tbn_inv_imported.shape) == (3, 3, 3)
    assert tuple(f.frame_map_imported.shape) == (2, 3, 12) and tuple(f.sample_inv_rows_imported.shape) == (3, 12)
    assert torch.equal(f.frame_map_imported[..., :9], f.local_tbn_imported) and torch.equal(f.frame_map_imported[..., 9], f.sample_tbn_ids_imported)
    assert not f.frame_map_imported[..., 10:].any() and not f.sample_inv_rows_imported[:, 9:].any()
    want = torch.linalg.inv(torch.from_numpy(m["sample_tbn"]))
    assert torch.equal(f.sample_tbn_inv_imported, want) and torch.equal(f.sample_inv_rows_imported[:, :9], want.reshape(3, 9))
    # the other accepted layouts of the frames: the same state
    g = _bare_field()
    g.import_field(pf.seeded_map(2, 3), 0.5, **dict(m, local_tbn=m["local_tbn"].reshape(2, 3, 3, 3), sample_tbn=torch.from_numpy(m["sample_tbn"]).reshape(3, 9)))
    assert torch.equal(g.frame_map_imported, f.frame_map_imported) and torch.equal(g.sample_inv_rows_imported, f.sample_inv_rows_imported)
    # the setters and the switch work as for the unlit field
    f.set_uv_utilize_rate(0.8), f.set_sdf_offset(0.01), f.set_h_threshold(0.03)
    assert f._import_scalars()[1] == 0.8 and f.projector.h_threshold == 0.03
    f.switch_import()
    assert not f.imported and f._import_stamp() == ()
    f.switch_import()
    assert f.imported


WRONG = [
    (dict(phi_embed=np.zeros((2, 3, 4), np.float32)), r"phi_embed is \[H, W, 8\]"),
    (dict(phi_embed=np.zeros((3, 2, 8), np.float32)), r"phi_embed is \[H, W, 8\]"),
    (dict(local_tbn=np.zeros((2, 3, 3), np.float32)), r"local_tbn is \[H, W, 9\]"),
    (dict(local_tbn=np.zeros((2, 2, 9), np.float32)), r"local_tbn is \[H, W, 9\]"),
    (dict(sample_tbn=np.zeros((3, 3), np.float32)), r"sample_tbn is \[P, 3, 3\]"),
    (dict(sample_tbn=np.zeros((0, 3, 3), np.float32)), r"sample_tbn is \[P, 3, 3\]"),
    (dict(sample_tbn_ids=np.zeros((3, 2), np.float32)), r"sample_tbn_ids is \[H, W\]"),
    (dict(sample_tbn_ids=np.full((2, 3), 3.0, np.float32)), r"\[0, P\)"),
    (dict(sample_tbn_ids=np.full((2, 3), -1.0, np.float32)), r"\[0, P\)"),
    (dict(sample_tbn_ids=np.full((2, 3), np.nan, np.float32)), r"\[0, P\)"),
    (dict(phi_embed=None), "all four or none"),
    (dict(sample_tbn_ids=None), "all four or none"),
]


@pytest.mark.parametrize("over,text", WRONG, ids=lambda v: "-".join(f"{k}{getattr(x, 'shape', x)}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_wrong_maps_are_refused_and_leave_the_field_as_it_was(over, text):
    f = _bare_field()
    with pytest.raises(ValueError, match=text):
        f.import_field(pf.seeded_map(2, 3), 0.5, **dict(_maps(), **over))
    assert not f.imported and f.features_imported is None and f.phi_embed_imported is None and not f.rescale


def test_an_unlit_field_refuses_the_maps_and_its_stamp_is_unchanged():
    f = _bare_field(lit=False)
    for name, value in _maps().items():
        with pytest.raises(ValueError, match="would ignore them"):
            f.import_field(pf.seeded_map(2, 3), 0.5, **{name: value})
    assert not f.imported
    f.import_field(pf.seeded_map(2, 3), 0.5)
    stamp = f._import_stamp()
    feat = f.features_imported
    assert stamp == ("import", feat.data_ptr(), (2, 3, 16)) + f._import_scalars() + (f._import_version,), "the tuple of the unlit field, as it was"


def test_the_stamp_changes_with_each_of_the_four_maps():
    f = _bare_field()
    f.import_field(pf.seeded_map(2, 3), 0.5, **_maps())
    base = f._import_stamp()
    assert base[0] == "import" and len(base) > len(("import", 0, ()) + f._import_scalars() + (0,))
    for name in ("phi_embed_imported", "local_tbn_imported", "sample_tbn_inv_imported", "sample_tbn_ids_imported", "frame_map_imported", "sample_inv_rows_imported"):
        kept = getattr(f, name)
        setattr(f, name, kept.clone())  # other storage, the same version: what a re-import makes of the map
        assert f._import_stamp() != base, name
        setattr(f, name, kept)
        assert f._import_stamp() == base
    seen = [base]
    m = _maps()
    for name in m:  # ... and through import_field itself, one map replaced at a time
        changed = dict(m, **{name: (m[name] + (0 if name == "sample_tbn_ids" else 0.25)).astype(np.float32)})
        f.import_field(pf.seeded_map(2, 3), 0.5, **changed)
        assert f._import_stamp() not in seen
        seen.append(f._import_stamp())


def test_import_shape_and_the_trainer_still_refuse():
    from ngp_harness.accelerate import CurvedTrainer

    f = _bare_field()
    f.import_field(pf.seeded_map(2, 3), 0.5, **_maps())
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    with pytest.raises(NotImplementedError, match="phi_embed.*local_tbn.*sample_tbn.*new mesh's frames"):
        f.import_shape(v, np.array([[0, 1, 2]]), v[:, :2])
    with pytest.raises(NotImplementedError, match="import mode is for rendering"):
        CurvedTrainer(types.SimpleNamespace(field=f))
    x = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="without gradients to the sample position"):
        f.embed(x, requires_grad_xyz=True, with_fine_normal=True)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------------

def _struct_fields():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nerftex_curved_light_import_infer_desc \{(.*?)\} nerftex_curved_light_import_infer_desc;", src, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            names.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", first.strip()).group(1))
            names += [m.strip() for m in more]
    return names


def test_the_header_declares_and_the_library_exports_the_entry_points(tmp_path):
    import subprocess

    import nerftex_hip

    src = open(HEADER).read()
    for name in ("nerftex_planar_light_lookup", "nerftex_curved_light_import_infer", "nerftex_curved_light_import_infer_scratch_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(ctypes.CDLL(nerftex_hip.LIB_PATH), name) and name in nerftex_hip.EXPORTS
    assert int(re.search(r"#define NERFTEX_FRAME_MAP_STRIDE (\d+)", src).group(1)) == nerftex_hip.FRAME_MAP_STRIDE == 12
    fields = _struct_fields()
    assert [n for n, _ in nerftex_hip.CurvedLightImportInferDesc._fields_] == fields
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {",
             '    printf("sizeof %lu\\n", (unsigned long)sizeof(nerftex_curved_light_import_infer_desc));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof(nerftex_curved_light_import_infer_desc, {n}));' for n in fields]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(nerftex_hip.CurvedLightImportInferDesc)
    for n in fields:
        assert int(out[n]) == getattr(nerftex_hip.CurvedLightImportInferDesc, n).offset, n


def test_scratch_query():
    from nerftex_hip import lib

    sizes = [lib.nerftex_curved_light_import_infer_scratch_bytes(b) for b in (0, 128, 256, 1 << 20)]
    assert sizes[0] == 0 and sizes[1] > 0 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    # mask, normal, xin, h, the phi features, two frames, the raw density, the BRDF net's input and output, the shading normal
    assert sizes[3] == (1 << 20) * (1 + 12 + 96 + 32 + 16 + 36 + 36 + 4 + 32 + 32 + 12)


FAKE = 0x10000  # a non-NULL, 256-byte aligned address that is never dereferenced: every case below is refused before anything is launched
POINTERS = ("xyz", "dirs", "map", "phi_map", "frame_map", "sample_tbn_inv", "sigma_weights", "normal_weights", "normal_biases", "brdf_weights", "env_shs", "sigma",
            "rgbs", "scratch")


def _desc(**over):
    from nerftex_hip import CurvedLightImportInferDesc

    kw = dict(B=128, map_h=24, map_w=20, n_features=16, n_phi=8, n_patches=5, mode=0, plane_scale0=1.0, plane_scale1=1.0, height_scale0=0.375, height_scale1=1.0,
              sdf_offset=0.0, h_threshold=0.0625, n_freqs=12, sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16, normal_hidden=16, normal_layers=2,
              brdf_in=16, brdf_hidden=64, brdf_layers=3, brdf_out=5, n_sh=16, n_color=1, gamma=2.4, flags=1, visual_mode=0, fc_weight=1.0, eval=1,
              scratch_bytes=1 << 40)
    kw.update({name: FAKE for name in POINTERS})
    kw.update(over)
    return CurvedLightImportInferDesc(**kw)


REFUSED = [
    (dict(B=100), "multiple of 128"),
    (dict(n_features=8), "default SH-lit curved field"),
    (dict(n_phi=16), "default SH-lit curved field"),
    (dict(n_freqs=10), "default SH-lit curved field"),
    (dict(sigma_hidden=64), "default SH-lit curved field"),
    (dict(normal_hidden=32), "default SH-lit curved field"),
    (dict(brdf_out=3), "default SH-lit curved field"),
    (dict(n_sh=4), "at least 9 SH rows"),
    (dict(n_color=2), "at least 9 SH rows"),
    (dict(gamma=0.0), "gamma is positive and finite"),
    (dict(flags=2), "NERFTEX_SH_LIGHT_SPECULAR or nothing"),
    (dict(visual_mode=4), "NERFTEX_LIGHT_VISUAL_"),
    (dict(eval=2), "eval is 0 or 1"),
    (dict(map_h=0), "between 1 and 16384"),
    (dict(map_w=16385), "between 1 and 16384"),
    (dict(n_patches=0), "patch frames"),
    (dict(B=64, n_features=8), "multiple of 128"),  # the batch is looked at before the shapes
    (dict(B=0, n_phi=4), "default SH-lit curved field"),  # the shapes, the maps and P are looked at before the empty batch returns
    (dict(B=0, n_patches=0), "patch frames"),
    (dict(n_patches=0, xyz=None), "patch frames"),  # P before the pointers
    (dict(scratch=FAKE + 0x80), "256-byte aligned"),
    (dict(scratch_bytes=1), "256-byte aligned and hold"),
    (dict(map=FAKE + 8), "16-byte aligned"),
    (dict(phi_map=FAKE + 8), "16-byte aligned"),
    (dict(frame_map=FAKE + 4), "16-byte aligned"),
    (dict(sample_tbn_inv=FAKE + 8), "16-byte aligned"),
    (dict(brdf_weights=FAKE + 8), "16-byte aligned"),
    (dict(normal_weights=FAKE + 2), "4-byte aligned"),
    (dict(xyz=None, mode=2), "must not be NULL"),  # the pointers before the mode
    (dict(mode=2), "NERFTEX_PLANAR_MULTIPLY or NERFTEX_PLANAR_DIVIDE"),
    (dict(plane_scale0=0.0), "positive and finite"),
    (dict(height_scale1=float("nan")), "positive and finite"),
    (dict(h_threshold=0.0), "positive and finite"),
    (dict(sdf_offset=float("nan")), "finite"),
] + [({name: None}, "must not be NULL") for name in POINTERS]


@pytest.mark.parametrize("over,text", REFUSED, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_the_chain_refuses_before_any_launch(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_curved_light_import_infer(ctypes.byref(_desc(**over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_the_chain_null_descriptor_empty_batch_and_a_scratch_one_byte_short():
    from nerftex_hip import lib

    assert lib.nerftex_curved_light_import_infer(None, None) == NERFTEX_ERR_INVALID
    assert "NULL descriptor" in lib.nerftex_last_error().decode()
    assert lib.nerftex_curved_light_import_infer(ctypes.byref(_desc(B=0, **{name: None for name in POINTERS})), None) == 0  # nothing is looked at for no rows
    need = lib.nerftex_curved_light_import_infer_scratch_bytes(128)
    assert lib.nerftex_curved_light_import_infer(ctypes.byref(_desc(scratch_bytes=need - 1)), None) == NERFTEX_ERR_INVALID
    assert str(need) in lib.nerftex_last_error().decode()


def _lookup(**over):
    from nerftex_hip import lib

    kw = dict(xyz=FAKE, map=FAKE, phi_map=FAKE, frame_map=FAKE, sample_tbn_inv=FAKE, map_h=24, map_w=20, n_patches=5, mode=1, p0=0.375, p1=0.3125, h0=1.0, h1=1.0,
              offset=0.0, h=0.0625, n_freqs=12, B=5, p_uv=FAKE, sdf=FAKE, mask=FAKE, xin=FAKE, phi=FAKE, patch_id=FAKE, local_tbn=FAKE, sample_tbn=FAKE)
    kw.update(over)
    return lib.nerftex_planar_light_lookup(*kw.values(), None)


LOOKUP_REFUSED = [
    (dict(n_freqs=10), "12 height bands"),
    (dict(map_h=0), "between 1 and 16384"),
    (dict(n_patches=0), "patch frames"),
    (dict(B=0, n_freqs=4), "12 height bands"),
    (dict(phi_map=None), "must not be NULL"),
    (dict(frame_map=None), "must not be NULL"),
    (dict(sample_tbn_inv=None), "must not be NULL"),
    (dict(phi=None), "must not be NULL"),
    (dict(patch_id=None), "must not be NULL"),
    (dict(local_tbn=None), "must not be NULL"),
    (dict(sample_tbn=None), "must not be NULL"),
    (dict(phi_map=FAKE + 4), "16-byte aligned"),
    (dict(frame_map=FAKE + 8), "16-byte aligned"),
    (dict(phi=FAKE + 4), "16-byte aligned"),
    (dict(mode=3), "NERFTEX_PLANAR_MULTIPLY or NERFTEX_PLANAR_DIVIDE"),
    (dict(p0=0.0), "positive and finite"),
    (dict(offset=float("inf")), "finite"),
]


@pytest.mark.parametrize("over,text", LOOKUP_REFUSED, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_the_plain_lookup_refuses_before_any_launch(over, text):
    from nerftex_hip import lib

    assert _lookup(**over) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_the_plain_lookup_with_no_rows_is_ok():
    assert _lookup(B=0, xyz=None, map=None, phi_map=None) == 0
