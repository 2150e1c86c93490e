"""C-ABI surface of the patch export's front (CPU only): nerftex_patch_front and its descriptor are declared, exported and bound field for
field, and every invalid descriptor is refused before anything touches a device."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
NERFTEX_ERR_INVALID = 1
REQUIRED = ("tracer", "frames", "calibration", "origins", "intersections", "stats", "verdict", "slot", "count")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every case below is refused before anything is launched


def _struct_fields():
    """The member names of nerftex_patch_front_desc, in the header's order."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nerftex_patch_front_desc \{(.*?)\} nerftex_patch_front_desc;", src, flags=re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *more = decl.split(",")
            names.append(re.search(r"([A-Za-z_][A-Za-z0-9_]*)$", first.strip()).group(1))
            names += [m.strip() for m in more]
    return names


def test_entry_and_descriptor_are_declared_exported_and_bound(tmp_path):
    import nerftex_hip

    assert re.search(r"\bint nerftex_patch_front\(const nerftex_patch_front_desc\* d, void\* stream\);", open(HEADER).read())
    lib = ctypes.CDLL(nerftex_hip.LIB_PATH)
    assert hasattr(lib, "nerftex_patch_front") and "nerftex_patch_front" in nerftex_hip.EXPORTS
    fields = _struct_fields()
    assert [n for n, _ in nerftex_hip.PatchFrontDesc._fields_] == fields
    for must in REQUIRED + ("scan", "rays", "B", "S", "max_scan_dist", "max_patch_num"):
        assert must in fields, must
    # the C compiler's layout of the struct is the binding's
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {",
             '    printf("sizeof %lu\\n", (unsigned long)sizeof(nerftex_patch_front_desc));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof(nerftex_patch_front_desc, {n}));' for n in fields]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(nerftex_hip.PatchFrontDesc)
    for n in fields:
        assert int(out[n]) == getattr(nerftex_hip.PatchFrontDesc, n).offset, n


def test_verdict_codes_are_the_documented_ones():
    import nerftex_hip
    from ngp_harness import patches

    codes = (nerftex_hip.PATCH_ACCEPTED, nerftex_hip.PATCH_BELOW, nerftex_hip.PATCH_NAN, nerftex_hip.PATCH_FAR, nerftex_hip.PATCH_MISSED,
             nerftex_hip.PATCH_NOT_NEEDED)
    assert codes == (0, 1, 2, 3, 4, 5) == (patches.ACCEPTED, patches.BELOW, patches.NAN_ORIGIN, patches.FAR, patches.MISSED, patches.NOT_NEEDED)


def _desc(**over):
    """A descriptor one step short of a launch: every required pointer set, one candidate of 3 x 3 pixels."""
    from nerftex_hip import PatchFrontDesc

    kw = dict({name: FAKE for name in REQUIRED}, B=1, S=3, max_scan_dist=0.1, max_patch_num=1)
    kw.update(over)
    return PatchFrontDesc(**kw)


REFUSED = [({name: None}, "must not be NULL") for name in REQUIRED] + [
    (dict(B=0), "at least one candidate"),
    (dict(S=0), "at least one candidate"),
    (dict(max_patch_num=0), "at least one candidate"),
    (dict(S=65536), "32 bits"),            # S^2 alone is 2^32
    (dict(S=4096, B=256), "32 bits"),      # S^2 B = 2^32
    (dict(S=65535, B=2), "32 bits"),
    (dict(B=65536), "65535 candidates"),   # one grid row per candidate
    (dict(B=0, tracer=None), "must not be NULL"),  # the pointers are looked at first
]


@pytest.mark.parametrize("over,text", REFUSED, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_an_invalid_descriptor_is_refused_before_any_launch(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_patch_front(ctypes.byref(_desc(**over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_null_descriptor_is_refused():
    from nerftex_hip import lib

    assert lib.nerftex_patch_front(None, None) == NERFTEX_ERR_INVALID
    assert "NULL descriptor" in lib.nerftex_last_error().decode()


def test_an_imported_field_refuses_before_anything_else_is_looked_at():
    """export_field's refusal needs no device: the import state is read first."""
    from ngp_harness import patches

    class Imported:
        imported = True

    with pytest.raises(NotImplementedError, match="switch_import"):
        patches.export_field(Imported(), None, None)
    with pytest.raises(NotImplementedError, match="switch_import"):
        patches._export_field_reference(Imported(), None, None)
