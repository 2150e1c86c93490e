"""C-ABI surface of the curved field's device-count inference entry (CPU only): nerftex_curved_field_infer, its scratch query and its
descriptor are declared, exported and bound field for field, and what the kernels do not serve is refused before anything touches a device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
NERFTEX_ERR_INVALID = 1


def _struct_fields():
    """The member names of nerftex_curved_infer_desc, in the header's order."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nerftex_curved_infer_desc \{(.*?)\} nerftex_curved_infer_desc;", src, flags=re.S).group(1)
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
    assert re.search(r"\bint nerftex_curved_field_infer\(const nerftex_curved_infer_desc\* d, void\* stream\);", src)
    assert re.search(r"\bsize_t nerftex_curved_field_infer_scratch_bytes\(uint32_t B\);", src)
    lib = ctypes.CDLL(nerftex_hip.LIB_PATH)
    for name in ("nerftex_curved_field_infer", "nerftex_curved_field_infer_scratch_bytes"):
        assert hasattr(lib, name) and name in nerftex_hip.EXPORTS, name
    fields = _struct_fields()
    assert [n for n, _ in nerftex_hip.CurvedInferDesc._fields_] == fields
    for must in ("knn", "tracer", "xyz", "dirs", "B", "mesh_vertices", "vertex_normals", "tbn", "K", "dir_vec_wdist", "h_threshold", "n_freqs", "table",
                 "offsets", "sigma_weights", "color_weights", "fc_weight", "eval", "sigma", "rgbs", "units_dev", "rows_per_unit", "scratch"):
        assert must in fields, must
    # the C compiler's layout of the struct is the binding's
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {",
             '    printf("sizeof %lu\\n", (unsigned long)sizeof(nerftex_curved_infer_desc));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof(nerftex_curved_infer_desc, {n}));' for n in fields]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(nerftex_hip.CurvedInferDesc)
    for n in fields:
        assert int(out[n]) == getattr(nerftex_hip.CurvedInferDesc, n).offset, n


def test_scratch_query():
    from nerftex_hip import lib

    sizes = [lib.nerftex_curved_field_infer_scratch_bytes(b) for b in (0, 128, 256, 1 << 20)]
    assert sizes[0] == 0 and sizes[1] > 0 and sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    # 16 neighbours (index + distance), surface point, normal, mask, features, the two networks' inputs and outputs, the raw density
    assert sizes[3] == (1 << 20) * (64 + 64 + 12 + 12 + 1 + 32 + 96 + 32 + 2 + 64 + 32)


def _default_desc(**over):
    """A descriptor with the default curved field's shapes and no buffers: the refusals under test come before any pointer is looked at."""
    from nerftex_hip import CurvedInferDesc

    kw = dict(B=128, n_verts=100, K=8, n_freqs=12, dir_vec_wdist=0.05, h_threshold=0.05, D=3, C=2, L=8, S=0.1, H=512, in_add=1.0, in_mul=0.5,
              sigma_in=48, sigma_hidden=32, sigma_layers=2, sigma_out=16, color_in=32, color_hidden=64, color_layers=3, color_out=3, fc_weight=1.0, eval=3)
    kw.update(over)
    return CurvedInferDesc(**kw)


REFUSED = [
    (dict(B=100), "multiple of 128"),
    (dict(B=129), "multiple of 128"),
    (dict(n_verts=0), "vertices"),
    (dict(K=0), "1 <= K <= 16"),
    (dict(K=17), "1 <= K <= 16"),
    (dict(sigma_in=32), "default curved field"),
    (dict(sigma_hidden=64), "default curved field"),
    (dict(sigma_layers=3), "default curved field"),
    (dict(color_hidden=32), "default curved field"),
    (dict(color_layers=2), "default curved field"),
    (dict(color_out=16), "default curved field"),
    (dict(n_freqs=10), "default curved field"),
    (dict(L=16), "default curved field"),
    (dict(), "must not be NULL"),  # default shapes, no handles and no buffers
    (dict(B=64, sigma_in=32), "multiple of 128"),  # the batch is looked at before the shapes
    (dict(B=0, L=16), "default curved field"),  # the shapes are looked at before the empty batch returns
]


@pytest.mark.parametrize("over,text", REFUSED)
def test_what_the_kernels_do_not_serve_is_refused(over, text):
    from nerftex_hip import lib

    desc = _default_desc(**over)
    assert lib.nerftex_curved_field_infer(ctypes.byref(desc), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_null_descriptor_is_refused():
    from nerftex_hip import lib

    assert lib.nerftex_curved_field_infer(None, None) == NERFTEX_ERR_INVALID
    assert "NULL descriptor" in lib.nerftex_last_error().decode()


def test_empty_batch_is_ok_and_launches_nothing():
    from nerftex_hip import lib

    assert lib.nerftex_curved_field_infer(ctypes.byref(_default_desc(B=0)), None) == 0
    assert lib.nerftex_curved_field_infer(ctypes.byref(_default_desc(B=0, n_verts=0)), None) == 0  # the mesh is looked at for a batch with rows only


POINTERS = ("knn", "tracer", "xyz", "dirs", "mesh_vertices", "vertex_normals", "table", "offsets", "sigma_weights", "color_weights", "sigma", "rgbs",
            "scratch")
FAKE = 0x10000  # a non-NULL, 256-byte aligned address that is never dereferenced: every case below is refused before anything is launched


def _pointed_desc(**over):
    """_default_desc with every required pointer set and a scratch that is large enough: one step short of a launch."""
    kw = dict({name: FAKE for name in POINTERS}, scratch_bytes=1 << 40)
    kw.update(over)
    return _default_desc(**kw)


def _refused_at_the_pointers():
    cases = [({name: None}, "must not be NULL") for name in POINTERS]  # (tbn is not among them: the static light model does not read the frames)
    cases += [(dict(scratch=FAKE + 0x80), "256-byte aligned"),
              (dict(sigma_weights=FAKE + 8), "16-byte aligned"),
              (dict(color_weights=FAKE + 8), "16-byte aligned"),
              (dict(in_mul=0.0), "positive and finite"),
              (dict(in_mul=float("inf")), "positive and finite")]
    return cases


@pytest.mark.parametrize("over,text", _refused_at_the_pointers(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, dict) else None)
def test_pointers_alignment_and_scales_are_refused_before_any_launch(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_curved_field_infer(ctypes.byref(_pointed_desc(**over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_a_scratch_one_byte_short_is_refused_with_the_size_it_needs():
    from nerftex_hip import lib

    need = lib.nerftex_curved_field_infer_scratch_bytes(128)
    assert lib.nerftex_curved_field_infer(ctypes.byref(_pointed_desc(scratch_bytes=need - 1)), None) == NERFTEX_ERR_INVALID
    text = lib.nerftex_last_error().decode()
    assert "must not be NULL" in text and str(need) in text, text
