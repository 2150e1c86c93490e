"""C-ABI surface of the SH-lit curved field's device-count inference entry (CPU only): nerftex_curved_light_infer, its scratch query and its
descriptor are declared, exported and bound field for field, and what the kernels do not serve is refused before anything touches a device, in
the order the header states: NULL descriptor, B % 128, shapes, B == 0 is OK, then pointers."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
NERFTEX_ERR_INVALID = 1


def _struct_fields():
    """The member names of nerftex_curved_light_infer_desc, in the header's order."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nerftex_curved_light_infer_desc \{(.*?)\} nerftex_curved_light_infer_desc;", src, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            names.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", first.strip()).group(1))
            names += [m.strip() for m in more]
    return names


def test_entry_scratch_query_and_descriptor_are_declared_exported_and_bound(tmp_path):
    import nerftex_hip

    src = open(HEADER).read()
    assert re.search(r"\bint nerftex_curved_light_infer\(const nerftex_curved_light_infer_desc\* d, void\* stream\);", src)
    assert re.search(r"\bsize_t nerftex_curved_light_infer_scratch_bytes\(uint32_t B\);", src)
    lib = ctypes.CDLL(nerftex_hip.LIB_PATH)
    for name in ("nerftex_curved_light_infer", "nerftex_curved_light_infer_scratch_bytes"):
        assert hasattr(lib, name) and name in nerftex_hip.EXPORTS, name
    fields = _struct_fields()
    assert [n for n, _ in nerftex_hip.CurvedLightInferDesc._fields_] == fields
    for must in ("knn", "tracer", "xyz", "dirs", "B", "mesh_vertices", "vertex_normals", "tbn", "K", "dir_vec_wdist", "h_threshold", "n_freqs", "table",
                 "offsets", "normal_table", "normal_offsets", "normal_S", "normal_in_mul", "sigma_weights", "normal_weights", "normal_biases", "brdf_weights",
                 "env_shs", "n_sh", "n_color", "gamma", "flags", "visual_mode", "fc_weight", "eval", "sigma", "rgbs", "shading_normal", "units_dev",
                 "rows_per_unit", "scratch", "scratch_bytes"):
        assert must in fields, must
    # the static entry's descriptor is left as it was: the new fields live in the new struct only
    assert "normal_table" not in [n for n, _ in nerftex_hip.CurvedInferDesc._fields_]
    assert re.search(r"#define NERFTEX_NORMAL_NET_WEIGHTS 1312\b", src) and re.search(r"#define NERFTEX_NORMAL_NET_BIASES 66\b", src)
    assert (nerftex_hip.NORMAL_NET_WEIGHTS, nerftex_hip.NORMAL_NET_BIASES) == (1312, 66)
    for name, value in nerftex_hip.LIGHT_VISUAL.items():
        assert re.search(rf"#define NERFTEX_LIGHT_VISUAL_{name.upper()} {value}\b", src), name
    # the C compiler's layout of the struct is the binding's
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {",
             '    printf("sizeof %lu\\n", (unsigned long)sizeof(nerftex_curved_light_infer_desc));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof(nerftex_curved_light_infer_desc, {n}));' for n in fields]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(nerftex_hip.CurvedLightInferDesc)
    for n in fields:
        assert int(out[n]) == getattr(nerftex_hip.CurvedLightInferDesc, n).offset, n


def test_scratch_query():
    from nerftex_hip import lib

    sizes = [lib.nerftex_curved_light_infer_scratch_bytes(b) for b in (0, 128, 256, 1 << 20)]
    assert sizes[0] == 0 and sizes[1] > 0 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    # 16 neighbours (index + distance), surface point, normal, frame, mask, the two tables' features, the sigma net's input and output, the raw
    # density (fp32), the BRDF net's input and output, the shading normal
    assert sizes[3] == (1 << 20) * (64 + 64 + 12 + 12 + 36 + 1 + 32 + 16 + 96 + 32 + 4 + 32 + 32 + 12)


def _default_desc(**over):
    """A descriptor with the default curved field's shapes and no buffers: the refusals under test come before any pointer is looked at."""
    from nerftex_hip import CurvedLightInferDesc

    kw = dict(B=128, n_verts=100, K=8, n_freqs=12, dir_vec_wdist=0.05, h_threshold=0.05, D=3, C=2, L=8, S=0.1, H=512, in_add=1.0, in_mul=0.5,
              normal_C=2, normal_L=4, normal_S=0.1, normal_H=512, normal_align_corners=1, normal_in_add=1.0, normal_in_mul=0.5,
              sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16, normal_hidden=16, normal_layers=2, brdf_in=16, brdf_hidden=64, brdf_layers=3,
              brdf_out=5, n_sh=16, n_color=1, gamma=2.4, flags=1, visual_mode=0, fc_weight=1.0, eval=1)
    kw.update(over)
    return CurvedLightInferDesc(**kw)


REFUSED = [
    (dict(B=64), "multiple of 128"),
    (dict(B=100), "multiple of 128"),
    (dict(B=129), "multiple of 128"),
    (dict(B=64, sigma_in=32), "multiple of 128"),  # the batch is looked at before the shapes
    (dict(n_verts=0), "vertices"),
    (dict(K=0), "1 <= K <= 16"),
    (dict(K=17), "1 <= K <= 16"),
    (dict(sigma_in=32), "default SH-lit curved field"),
    (dict(sigma_hidden=64), "default SH-lit curved field"),
    (dict(sigma_layers=3), "default SH-lit curved field"),
    (dict(brdf_in=32), "default SH-lit curved field"),
    (dict(brdf_hidden=32), "default SH-lit curved field"),
    (dict(brdf_layers=2), "default SH-lit curved field"),
    (dict(brdf_out=16), "default SH-lit curved field"),
    (dict(normal_hidden=32), "default SH-lit curved field"),
    (dict(normal_layers=3), "default SH-lit curved field"),
    (dict(normal_L=8), "default SH-lit curved field"),
    (dict(normal_C=4), "default SH-lit curved field"),
    (dict(n_freqs=10), "default SH-lit curved field"),
    (dict(L=16), "default SH-lit curved field"),
    (dict(B=0, L=16), "default SH-lit curved field"),  # the shapes are looked at before the empty batch returns
    (dict(n_sh=8), "at least 9 SH rows"),
    (dict(n_color=2), "at least 9 SH rows"),
    (dict(gamma=0.0), "gamma is positive"),
    (dict(flags=2), "flags"),
    (dict(visual_mode=4), "visual_mode"),
    (dict(eval=2), "eval is 0 or 1"),
    (dict(), "must not be NULL"),  # default shapes, no handles and no buffers
]


@pytest.mark.parametrize("over,text", REFUSED)
def test_what_the_kernels_do_not_serve_is_refused(over, text):
    from nerftex_hip import lib

    desc = _default_desc(**over)
    assert lib.nerftex_curved_light_infer(ctypes.byref(desc), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_null_descriptor_is_refused():
    from nerftex_hip import lib

    assert lib.nerftex_curved_light_infer(None, None) == NERFTEX_ERR_INVALID
    assert "NULL descriptor" in lib.nerftex_last_error().decode()


def test_empty_batch_is_ok_and_launches_nothing():
    from nerftex_hip import lib

    assert lib.nerftex_curved_light_infer(ctypes.byref(_default_desc(B=0)), None) == 0
    assert lib.nerftex_curved_light_infer(ctypes.byref(_default_desc(B=0, n_verts=0)), None) == 0  # the mesh is looked at for a batch with rows only


POINTERS = ("knn", "tracer", "xyz", "dirs", "mesh_vertices", "vertex_normals", "tbn", "table", "offsets", "normal_table", "normal_offsets",
            "sigma_weights", "normal_weights", "normal_biases", "brdf_weights", "env_shs", "sigma", "rgbs", "scratch")
FAKE = 0x10000  # a non-NULL, 256-byte aligned address that is never dereferenced: every case below is refused before anything is launched


def _pointed_desc(**over):
    """_default_desc with every required pointer set and a scratch that is large enough: one step short of a launch."""
    kw = dict({name: FAKE for name in POINTERS}, scratch_bytes=1 << 40)
    kw.update(over)
    return _default_desc(**kw)


def _refused_at_the_pointers():
    cases = [({name: None}, "must not be NULL") for name in POINTERS]  # (shading_normal is not among them: an optional output)
    cases += [(dict(scratch=FAKE + 0x80), "256-byte aligned"),
              (dict(sigma_weights=FAKE + 8), "16-byte aligned"),
              (dict(brdf_weights=FAKE + 8), "16-byte aligned"),
              (dict(normal_weights=FAKE + 2), "4-byte aligned"),
              (dict(in_mul=0.0), "positive and finite"),
              (dict(in_mul=float("inf")), "positive and finite"),
              (dict(normal_in_mul=0.0), "positive and finite")]
    return cases


@pytest.mark.parametrize("over,text", _refused_at_the_pointers(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, dict) else None)
def test_pointers_alignment_and_scales_are_refused_before_any_launch(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_curved_light_infer(ctypes.byref(_pointed_desc(**over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_a_scratch_one_byte_short_is_refused_with_the_size_it_needs():
    from nerftex_hip import lib

    need = lib.nerftex_curved_light_infer_scratch_bytes(128)
    assert lib.nerftex_curved_light_infer(ctypes.byref(_pointed_desc(scratch_bytes=need - 1)), None) == NERFTEX_ERR_INVALID
    text = lib.nerftex_last_error().decode()
    assert "must not be NULL" in text and str(need) in text, text
