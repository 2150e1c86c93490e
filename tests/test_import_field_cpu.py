"""An imported planar feature texture under the curved field, the CPU side (no GPU): the reference's own outputs and the framework's
grid_sample meet the float64 bound of tests/planar_float64.py on every element (so the bar the GPU kernel is held to is one the reference
itself clears), the import state machine of CurvedField, the refusals of the two C entries, and the op-by-op route against the fixture
tests/golden/ref_python_import_field.npz (tools/make_golden.py: import_field_goldens)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import planar_float64 as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
NERFTEX_ERR_INVALID = 1
CONFIGS = [("A0", True), ("A1", True), ("B0", False), ("B1", False)]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_import_field.npz"))


def _bare_field(h_threshold=0.0625):
    """A CurvedField without its mesh structures (they need a device): the import state and the op-by-op route read none of them."""
    from ngp_harness.curved import CurvedField

    f = object.__new__(CurvedField)
    torch.nn.Module.__init__(f)
    f.normal_net, f.light_model, f.multires, f.h_threshold, f.in_dim = None, None, 12, h_threshold, 41
    f.encoder = types.SimpleNamespace(output_dim=16)
    f.sigma_net = types.SimpleNamespace(weights=torch.zeros(1), dtype=torch.float16)
    f.projector = types.SimpleNamespace(h_threshold=h_threshold)
    f._init_import_state()
    return f


def _golden_field(golden, key):
    f = _bare_field(float(golden["h_threshold"]))
    f.import_field(golden["features"], float(golden["grid_gap"]))
    if key[0] == "B":
        f.import_field(golden["features"], float(golden["grid_gap"]))
    f.set_uv_utilize_rate(float(golden[key + "_rate"]))
    f.set_sdf_offset(float(golden[key + "_offset"]))
    return f


# ---- the reference alone meets the bar ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["A0", "B1"])
def test_the_reference_fixture_is_inside_the_float64_bound_on_every_element(golden, key):
    f = _golden_field(golden, key)
    x = torch.from_numpy(golden["xyz"])
    p_uv, sdf, mask, x_embed = pf.torch_expressions(x, torch.from_numpy(golden["features"]), f.bounds, f.rescale, f.uv_utilize_rate, f.sdf_offset, f.h_threshold)
    embed = golden[key + "_embed"]
    assert np.array_equal(mask.numpy(), golden[key + "_h_mask"])
    assert np.array_equal(embed[:, 16], sdf.numpy()), "the fixture's height is the expressions' height, bit for bit"
    value, bound = pf.lookup_reference(golden["features"], p_uv[:, 0].numpy(), p_uv[:, 1].numpy(), sdf.numpy())
    narrowed = embed.astype(np.float16).astype(np.float64)  # (the bound is for an fp32 evaluation narrowed to half)
    ratio = np.abs(narrowed - value) / bound
    print(f"{key}: reference fixture, largest error / bound {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    assert np.abs(x_embed.numpy() - embed[:, :16]).max() == 0.0, "the framework's grid_sample IS the reference's lookup"


@pytest.mark.parametrize("H,W", pf.MAPS)
@pytest.mark.parametrize("rescale", [True, False])
def test_cpu_grid_sample_is_inside_the_bound_on_the_gpu_tests_inputs(H, W, rescale):
    F = pf.seeded_map(H, W)
    worst = 0.0
    for rate in (1.0, 0.5, 1.7):
        for offset in (0.0, 0.01):
            for B in (1, 127, 128, 129, 384):
                x = torch.from_numpy(pf.case_points(H, W, B, rescale, rate, offset))
                p_uv, sdf, _, x_embed = pf.torch_expressions(x, torch.from_numpy(F), pf.map_bounds(H, W), rescale, rate, offset, pf.H_THRESHOLD)
                from ngp_harness.curved import freq_encode

                got = torch.cat([x_embed, freq_encode(sdf[:, None], 12)], -1).half().double().numpy()
                value, bound = pf.lookup_reference(F, p_uv[:, 0].numpy(), p_uv[:, 1].numpy(), sdf.numpy())
                worst = max(worst, float((np.abs(got - value) / bound).max()))
    print(f"map {H}x{W} rescale={rescale}: CPU grid_sample, largest error / bound {worst:.3f}")
    assert worst <= 1.0


def test_u_runs_along_the_first_axis():
    F = pf.seeded_map(5, 4)
    value, _ = pf.bilinear(F, np.float32([-1, 1, 1]), np.float32([-1, 1, -1]))
    assert np.array_equal(value[0], F[0, 0]) and np.array_equal(value[1], F[4, 3]) and np.array_equal(value[2], F[4, 0])
    x = torch.tensor([[-1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [1.0, -1.0, 0.0]])
    _, _, _, e = pf.torch_expressions(x, torch.from_numpy(F), (1.0, 1.0), True, 1.0, 0.0, 1.0)
    assert np.array_equal(e.numpy(), value.astype(np.float32))


def test_the_threshold_is_strict_and_the_plane_bounds_inclusive():
    F = pf.seeded_map(2, 3)
    h = np.float32(pf.H_THRESHOLD)
    x = torch.tensor([[1.0, -1.0, float(h) / 0.5], [1.0, -1.0, float(np.nextafter(h, np.float32(0))) / 0.5], [float(np.nextafter(np.float32(1), np.float32(2))), 0.0, 0.0]])
    _, sdf, mask, _ = pf.torch_expressions(x, torch.from_numpy(F), pf.map_bounds(2, 3), True, 1.0, 0.0, pf.H_THRESHOLD)
    assert float(sdf[0]) == pf.H_THRESHOLD and mask.tolist() == [False, True, False]


# ---- the state machine ----------------------------------------------------------------------------------------------------------------------------------

def test_import_toggles_rescale_and_the_keyword_overrides_it():
    f = _bare_field()
    assert not f.imported and not f.rescale and f._import_stamp() == ()
    F = pf.seeded_map(5, 4)
    f.import_field(F, 1 / 32)
    assert f.imported and f.rescale and f.bounds == [0.5 / 32 * 5, 0.5 / 32 * 4]
    assert f.features_imported.dtype == torch.float32 and tuple(f.features_imported.shape) == (5, 4, 16) and f.features_imported.is_contiguous()
    f.import_field(torch.from_numpy(F).double(), 1 / 32)
    assert f.imported and not f.rescale and f.features_imported.dtype == torch.float32
    f.import_field(F, 1 / 32, rescale=False)
    assert not f.rescale
    f.import_field(F, 1 / 32, rescale=True)
    assert f.rescale
    f.import_field(F, 1 / 32)
    assert not f.rescale


def test_switch_import_and_the_setters_change_the_stamp():
    f = _bare_field()
    with pytest.raises(RuntimeError, match="nothing has been imported"):
        f.switch_import()
    f.import_field(pf.seeded_map(2, 3), 0.5)
    seen = [f._import_stamp()]
    assert seen[0][0] == "import" and seen[0][2] == (2, 3, 16)
    for change in (lambda: f.set_uv_utilize_rate(0.8), lambda: f.set_sdf_offset(0.01), lambda: f.set_h_threshold(0.03),
                   lambda: f.import_field(pf.seeded_map(2, 3), 0.5)):
        change()
        assert f._import_stamp() not in seen
        seen.append(f._import_stamp())
    assert f.h_threshold == 0.03 and f.projector.h_threshold == 0.03
    f.switch_import()
    assert not f.imported and f._import_stamp() == (), "a field that is not rendering its import stamps as one that never imported"
    f.switch_import()
    assert f.imported and f._import_stamp() not in seen  # (the version moved: a graph recorded before the switch is not replayed)


def test_import_is_refused_with_a_normal_net_or_a_light_model_and_for_other_shapes():
    f = _bare_field()
    f.normal_net = object()
    with pytest.raises(NotImplementedError, match="phi_embed.*local_tbn.*sample_tbn"):
        f.import_field(pf.seeded_map(2, 3), 0.5)
    f = _bare_field()
    f.light_model = "SH"
    with pytest.raises(NotImplementedError, match="phi_embed"):
        f.import_field(pf.seeded_map(2, 3), 0.5)
    with pytest.raises(ValueError, match=r"\[H, W, 16\]"):
        _bare_field().import_field(np.zeros((4, 4, 8), np.float32), 0.5)


def test_the_trainer_refuses_an_imported_field():
    from ngp_harness.accelerate import CurvedTrainer

    f = _bare_field()
    f.encoder_var = None
    f.import_field(pf.seeded_map(2, 3), 0.5)
    with pytest.raises(NotImplementedError, match="import mode is for rendering"):
        CurvedTrainer(types.SimpleNamespace(field=f))


# ---- the op-by-op route against the fixture -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,rescale", CONFIGS)
def test_the_op_by_op_route_reproduces_the_fixture(golden, key, rescale):
    f = _golden_field(golden, key)
    assert f.rescale == rescale
    embed, normal, mask = f.embed(torch.from_numpy(golden["xyz"]))
    assert np.array_equal(mask.numpy(), golden[key + "_h_mask"])
    assert torch.equal(normal, torch.tensor([0.0, 0.0, 1.0]).expand(512, 3) / (1 + 1e-5))
    if key + "_embed" in golden:
        assert embed.dtype == torch.float32 and embed.shape == (512, 41)
        assert np.abs(embed.numpy() - golden[key + "_embed"]).max() <= 1e-6


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------------

def _struct_fields():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nerftex_curved_import_infer_desc \{(.*?)\} nerftex_curved_import_infer_desc;", src, flags=re.S).group(1)
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
    assert [n for n, _ in nerftex_hip.CurvedImportInferDesc._fields_] == fields
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {",
             '    printf("sizeof %lu\\n", (unsigned long)sizeof(nerftex_curved_import_infer_desc));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof(nerftex_curved_import_infer_desc, {n}));' for n in fields]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(nerftex_hip.CurvedImportInferDesc)
    for n in fields:
        assert int(out[n]) == getattr(nerftex_hip.CurvedImportInferDesc, n).offset, n


def test_scratch_query():
    from nerftex_hip import lib

    sizes = [lib.nerftex_curved_import_infer_scratch_bytes(b) for b in (0, 128, 256, 1 << 20)]
    assert sizes[0] == 0 and sizes[1] > 0 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    # mask, normal, the two networks' inputs and outputs, the raw density
    assert sizes[3] == (1 << 20) * (1 + 12 + 96 + 32 + 2 + 64 + 32)


FAKE = 0x10000  # a non-NULL, 256-byte aligned address that is never dereferenced: every case below is refused before anything is launched
POINTERS = ("xyz", "dirs", "map", "sigma_weights", "color_weights", "sigma", "rgbs", "scratch")


def _desc(**over):
    from nerftex_hip import CurvedImportInferDesc

    kw = dict(B=128, map_h=24, map_w=20, n_features=16, mode=0, plane_scale0=1.0, plane_scale1=1.0, height_scale0=0.375, height_scale1=1.0, sdf_offset=0.0,
              h_threshold=0.0625, n_freqs=12, sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16, color_in=32, color_hidden=64, color_layers=3,
              color_out=3, fc_weight=1.0, eval=3, scratch_bytes=1 << 40)
    kw.update({name: FAKE for name in POINTERS})
    kw.update(over)
    return CurvedImportInferDesc(**kw)


REFUSED = [
    (dict(B=100), "multiple of 128"),
    (dict(B=129), "multiple of 128"),
    (dict(n_features=8), "default curved field"),
    (dict(n_freqs=10), "default curved field"),
    (dict(sigma_in=32), "default curved field"),
    (dict(sigma_hidden=64), "default curved field"),
    (dict(color_layers=2), "default curved field"),
    (dict(color_out=16), "default curved field"),
    (dict(map_h=0), "between 1 and 16384"),
    (dict(map_w=16385), "between 1 and 16384"),
    (dict(B=64, n_features=8), "multiple of 128"),  # the batch is looked at before the shapes
    (dict(B=0, n_freqs=10), "default curved field"),  # the shapes and the map are looked at before the empty batch returns
    (dict(B=0, map_h=0), "between 1 and 16384"),
    (dict(map_h=0, xyz=None), "between 1 and 16384"),  # the map's size before the pointers
    (dict(scratch=FAKE + 0x80), "256-byte aligned"),
    (dict(scratch_bytes=1), "256-byte aligned and hold"),
    (dict(map=FAKE + 8), "16-byte aligned"),
    (dict(sigma_weights=FAKE + 8), "16-byte aligned"),
    (dict(color_weights=FAKE + 8), "16-byte aligned"),
    (dict(xyz=None, mode=2), "must not be NULL"),  # the pointers before the mode
    (dict(mode=2), "NERFTEX_PLANAR_MULTIPLY or NERFTEX_PLANAR_DIVIDE"),
    (dict(plane_scale0=0.0), "positive and finite"),
    (dict(plane_scale1=float("inf")), "positive and finite"),
    (dict(height_scale0=-1.0), "positive and finite"),
    (dict(height_scale1=float("nan")), "positive and finite"),
    (dict(h_threshold=0.0), "positive and finite"),
    (dict(sdf_offset=float("nan")), "finite"),
] + [({name: None}, "must not be NULL") for name in POINTERS]


@pytest.mark.parametrize("over,text", REFUSED, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_the_chain_refuses_before_any_launch(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_curved_import_infer(ctypes.byref(_desc(**over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_the_chain_null_descriptor_empty_batch_and_a_scratch_one_byte_short():
    from nerftex_hip import lib

    assert lib.nerftex_curved_import_infer(None, None) == NERFTEX_ERR_INVALID
    assert "NULL descriptor" in lib.nerftex_last_error().decode()
    assert lib.nerftex_curved_import_infer(ctypes.byref(_desc(B=0)), None) == 0
    assert lib.nerftex_curved_import_infer(ctypes.byref(_desc(B=0, **{name: None for name in POINTERS})), None) == 0  # nothing is looked at for no rows
    need = lib.nerftex_curved_import_infer_scratch_bytes(128)
    assert lib.nerftex_curved_import_infer(ctypes.byref(_desc(scratch_bytes=need - 1)), None) == NERFTEX_ERR_INVALID
    assert str(need) in lib.nerftex_last_error().decode()


def _lookup(**over):
    from nerftex_hip import lib

    kw = dict(xyz=FAKE, map=FAKE, map_h=24, map_w=20, mode=1, p0=0.375, p1=0.3125, h0=1.0, h1=1.0, offset=0.0, h=0.0625, n_freqs=12, B=5, p_uv=FAKE, sdf=FAKE,
              mask=FAKE, xin=FAKE)
    kw.update(over)
    return lib.nerftex_planar_lookup(*kw.values(), None)


LOOKUP_REFUSED = [
    (dict(n_freqs=10), "12 height bands"),
    (dict(map_h=0), "between 1 and 16384"),
    (dict(map_w=20000), "between 1 and 16384"),
    (dict(B=0, n_freqs=4), "12 height bands"),
    (dict(xyz=None), "must not be NULL"),
    (dict(map=None), "must not be NULL"),
    (dict(p_uv=None), "must not be NULL"),
    (dict(sdf=None), "must not be NULL"),
    (dict(mask=None), "must not be NULL"),
    (dict(xin=None), "must not be NULL"),
    (dict(map=FAKE + 4), "16-byte aligned"),
    (dict(xin=FAKE + 2), "16-byte aligned"),
    (dict(mode=3), "NERFTEX_PLANAR_MULTIPLY or NERFTEX_PLANAR_DIVIDE"),
    (dict(p0=0.0), "positive and finite"),
    (dict(h1=float("inf")), "positive and finite"),
    (dict(h=float("nan")), "positive and finite"),
    (dict(offset=float("inf")), "finite"),
]


@pytest.mark.parametrize("over,text", LOOKUP_REFUSED, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_the_plain_lookup_refuses_before_any_launch(over, text):
    from nerftex_hip import lib

    assert _lookup(**over) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_the_plain_lookup_with_no_rows_is_ok():
    assert _lookup(B=0, xyz=None, map=None) == 0


def test_the_binding_restates_the_mode_constants():
    import nerftex_hip

    src = open(HEADER).read()
    assert int(re.search(r"#define NERFTEX_PLANAR_MULTIPLY (\d+)", src).group(1)) == nerftex_hip.PLANAR_MULTIPLY
    assert int(re.search(r"#define NERFTEX_PLANAR_DIVIDE (\d+)", src).group(1)) == nerftex_hip.PLANAR_DIVIDE
