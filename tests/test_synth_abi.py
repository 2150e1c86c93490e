"""C-ABI surface of the texture synthesis (nerftex_synth_*): declared, exported and bound field for field, and every invalid descriptor refused with
an error code before anything touches a device (CPU only, but for first_patch, which is checked against a handle)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every case below is refused before anything is launched
ENTRIES = ("nerftex_synth_create", "nerftex_synth_resolve", "nerftex_synth_finish", "nerftex_synth_result", "nerftex_synth_read", "nerftex_synth_destroy")


def _struct_fields(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            names.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", first.strip()).group(1))
            names += [m.strip() for m in more]
    return names


@pytest.mark.parametrize("struct,binding", [("nerftex_synth_desc", "SynthDesc"), ("nerftex_synth_view", "SynthView")])
def test_structs_are_bound_field_for_field(tmp_path, struct, binding):
    import nerftex_hip

    cls = getattr(nerftex_hip, binding)
    fields = _struct_fields(struct)
    assert [n for n, _ in cls._fields_] == fields
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {", f'    printf("sizeof %lu\\n", (unsigned long)sizeof({struct}));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof({struct}, {n}));' for n in fields]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(cls)
    for n in fields:
        assert int(out[n]) == getattr(cls, n).offset, n


def test_entries_and_constants():
    import nerftex_hip

    lib = ctypes.CDLL(nerftex_hip.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in nerftex_hip.EXPORTS, name
    header = open(HEADER).read()
    for name in ("ERR_EXHAUSTED", "SYNTH_CUT", "SYNTH_BLEND", "SYNTH_LOG_STRIDE", "SYNTH_CANVAS", "SYNTH_CANVAS_ID", "SYNTH_ID_MAP", "SYNTH_LOG_IDS", "SYNTH_LOG_DIST",
                 "SYNTH_TBN_IDS", "SYNTH_TBN", "SYNTH_TOTAL_ID"):
        assert int(re.search(r"#define NERFTEX_%s (\d+)" % name, header).group(1)) == getattr(nerftex_hip, name), name
    assert nerftex_hip.SYNTH_LOG_STRIDE == 4 + 16 + 16


def _desc(**over):
    from nerftex_hip import SynthDesc

    kw = dict(patches=FAKE, sample_tbn=FAKE, picked_vertices=FAKE, P=24, S=13, C=33, match_dim=16, patch_size=3, overlap_size=5, output_h=30, output_w=30,
              mirror_hor=1, mirror_vert=1, attenuation=3, max_patch_res=4, mode=0, quilt=0, close_threshold=0.2, patch_length=1.0)
    kw.update(over)
    return SynthDesc(**kw)


REFUSED = [
    (dict(output_w=31), "non-square"),
    (dict(match_dim=34), "match_dim"),
    (dict(match_dim=0), "match_dim"),
    (dict(overlap_size=4), "overlap_size * 2 + patch_size"),
    (dict(patch_size=4), "overlap_size * 2 + patch_size"),
    (dict(overlap_size=0, patch_size=13), "overlap_size"),
    (dict(mode=1), "blend"),
    (dict(quilt=1), "quilt"),
    (dict(picked_vertices=None), "checkForMirrors"),
    (dict(patches=None), "must not be NULL"),
    (dict(sample_tbn=None), "must not be NULL"),
    (dict(P=0), "positive"),
    (dict(attenuation=2), "attenuation"),
    (dict(max_patch_res=0), "max_patch_res"),
    (dict(output_h=5, output_w=5), "larger than the overlap"),
    (dict(output_h=20000, output_w=20000), "16384"),
    (dict(P=20000), "65535 examples"),
]


@pytest.mark.parametrize("over,text", REFUSED, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_an_invalid_descriptor_is_refused_before_any_device_call(over, text):
    from nerftex_hip import ERR_INVALID, lib

    handle = ctypes.c_void_p(0x1234)
    assert lib.nerftex_synth_create(ctypes.byref(_desc(**over)), ctypes.byref(handle)) == ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()
    assert handle.value is None, "no handle comes back"


def test_null_arguments_are_refused():
    from nerftex_hip import ERR_INVALID, SynthView, lib

    handle = ctypes.c_void_p()
    assert lib.nerftex_synth_create(None, ctypes.byref(handle)) == ERR_INVALID
    assert lib.nerftex_synth_create(ctypes.byref(_desc()), None) == ERR_INVALID
    assert lib.nerftex_synth_resolve(None, 0, None, None, 0, 1, None) == ERR_INVALID
    assert lib.nerftex_synth_finish(None, None) == ERR_INVALID
    assert lib.nerftex_synth_result(None, ctypes.byref(SynthView())) == ERR_INVALID
    assert lib.nerftex_synth_read(None, 0, FAKE, 4, None) == ERR_INVALID
    assert lib.nerftex_synth_destroy(None) == 0


@pytest.mark.gpu
def test_resolve_refuses_first_patch_and_cell_ranges():
    import torch

    from nerftex_hip import ERR_INVALID, SynthView, lib, ptr

    dev = torch.device("cuda:0")
    patches = torch.zeros(20, 8, 8, 4, device=dev)
    tbn, picked = torch.zeros(20, 9, device=dev), torch.zeros(20, 3, device=dev)
    draws = torch.zeros(4, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    d = _desc(patches=ptr(patches), sample_tbn=ptr(tbn), picked_vertices=ptr(picked), P=20, S=8, C=4, match_dim=4, patch_size=2, overlap_size=3, output_h=13,
              output_w=13, mirror_hor=0, mirror_vert=0, max_patch_res=8)
    handle = ctypes.c_void_p()
    assert lib.nerftex_synth_create(ctypes.byref(d), ctypes.byref(handle)) == 0
    try:
        view = SynthView()
        assert lib.nerftex_synth_result(handle, ctypes.byref(view)) == 0
        assert (view.side, view.cells_per_side, view.examples, view.channels, view.block, view.strip_floats) == (13, 2, 20, 4, 1, 3 * 8 * 4)
        assert lib.nerftex_synth_resolve(handle, 20, ptr(draws), None, 0, 4, None) == ERR_INVALID
        assert "first_patch" in lib.nerftex_last_error().decode()
        assert lib.nerftex_synth_resolve(handle, 0, ptr(draws), None, 0, 5, None) == ERR_INVALID
        assert lib.nerftex_synth_resolve(handle, 0, ptr(draws), None, 1, 4, None) == ERR_INVALID  # raster order: cell 0 comes first
        assert lib.nerftex_synth_resolve(handle, 0, None, None, 0, 4, None) == ERR_INVALID
        assert lib.nerftex_synth_read(handle, 99, ptr(draws), 8, None) == ERR_INVALID
        assert lib.nerftex_synth_read(handle, 2, ptr(draws), 8, None) == ERR_INVALID  # the id map holds 16 bytes
    finally:
        assert lib.nerftex_synth_destroy(handle) == 0
