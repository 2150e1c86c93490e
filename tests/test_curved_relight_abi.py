"""C-ABI surface of relighting through the four lit chains (CPU only): nerftex_relight_desc is declared and bound field for field, the four
_relit entries are declared, exported and bound, and every refusal the header lists returns NERFTEX_ERR_INVALID with its message before
anything touches a device -- the descriptors below point at addresses that are never dereferenced, on a machine without a GPU.  The chains'
own descriptors are the ones their own ABI tests build (imported from those files, so that this file cannot drift from them)."""
import ctypes
import os
import re
import subprocess

import pytest

import test_curved_light_infer_abi as mesh_abi
import test_import_light_cpu as planar_abi
import test_import_patch_cpu as patch_abi
import test_import_shape_light_cpu as shape_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
NERFTEX_ERR_INVALID = 1
FAKE = 0x10000  # a non-NULL, aligned address that is never dereferenced

# chain -> (the entry's name without "_relit", its descriptor's C name, a builder of a descriptor one step short of a launch)
CHAINS = {
    "mesh": ("nerftex_curved_light_infer", "nerftex_curved_light_infer_desc", lambda **kw: mesh_abi._pointed_desc(**kw)),
    "planar": ("nerftex_curved_light_import_infer", "nerftex_curved_light_import_infer_desc", lambda **kw: planar_abi._desc(**kw)),
    "shape": ("nerftex_curved_light_shape_infer", "nerftex_curved_light_shape_infer_desc", lambda **kw: shape_abi._desc(**kw)),
    "patch": ("nerftex_curved_light_patch_infer", "nerftex_curved_light_patch_infer_desc", lambda **kw: patch_abi._desc(True, **kw)),
}
FIELDS = ["probes", "probe_shs", "K", "rotation"]


def _relight(**kw):
    from nerftex_hip import RelightDesc

    return RelightDesc(**kw)


def test_the_struct_is_declared_and_bound_field_for_field(tmp_path):
    import nerftex_hip

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nerftex_relight_desc \{(.*?)\} nerftex_relight_desc;", src, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["const float* probes", "const float* probe_shs", "uint32_t K", "const float* rotation"]
    assert [n for n, _ in nerftex_hip.RelightDesc._fields_] == FIELDS
    # the C compiler's layout of the struct is the binding's
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {",
             '    printf("sizeof %lu\\n", (unsigned long)sizeof(nerftex_relight_desc));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof(nerftex_relight_desc, {n}));' for n in FIELDS]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(nerftex_hip.RelightDesc)
    for n in FIELDS:
        assert int(out[n]) == getattr(nerftex_hip.RelightDesc, n).offset, n


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_the_relit_entry_is_declared_exported_and_bound(chain):
    import nerftex_hip

    entry, desc, _ = CHAINS[chain]
    src = open(HEADER).read()
    assert re.search(rf"\bint {entry}_relit\(const {desc}\* d, const nerftex_relight_desc\* r, void\* stream\);", src)
    assert re.search(rf"\bint {entry}\(const {desc}\* d, void\* stream\);", src), "the plain entry is declared as before"
    assert hasattr(ctypes.CDLL(nerftex_hip.LIB_PATH), entry + "_relit") and entry + "_relit" in nerftex_hip.EXPORTS
    fn = getattr(nerftex_hip.lib, entry + "_relit")
    assert list(fn.argtypes) == [ctypes.c_void_p] * 3 and fn.restype is ctypes.c_int


# (what the chain's descriptor holds, what the relight descriptor holds, a piece of the message)
REFUSED = [
    (dict(n_color=3), dict(K=257, probes=FAKE, probe_shs=FAKE), "at most 256 probes"),
    (dict(n_color=3), dict(K=64, probes=None, probe_shs=FAKE), "is NULL"),
    (dict(n_color=3), dict(K=64, probes=FAKE, probe_shs=None), "is NULL"),
    (dict(n_color=1), dict(K=64, probes=FAKE, probe_shs=FAKE), "three colours"),
    (dict(n_color=3, eval=0), dict(K=64, probes=FAKE, probe_shs=FAKE), "eval-only"),
    (dict(n_color=1, eval=0), dict(rotation=FAKE), "eval-only"),
    (dict(n_color=1, eval=0), dict(), "eval-only"),  # a non-NULL descriptor, even an empty one
    (dict(n_color=1), dict(rotation=FAKE + 2), "rotation must be 4-byte aligned"),
    (dict(n_color=3), dict(K=64, probes=FAKE, probe_shs=FAKE, rotation=FAKE + 1), "rotation must be 4-byte aligned"),
    (dict(n_color=3, B=0), dict(K=257, probes=FAKE, probe_shs=FAKE), "at most 256 probes"),  # looked at before the empty batch returns
]


@pytest.mark.parametrize("chain", sorted(CHAINS))
@pytest.mark.parametrize("over,relight,text", REFUSED, ids=[f"{i}-{t[2].split()[0]}" for i, t in enumerate(REFUSED)])
def test_what_the_relit_entries_refuse(chain, over, relight, text):
    from nerftex_hip import lib

    entry, _, make = CHAINS[chain]
    d, r = make(**over), _relight(**relight)
    assert getattr(lib, entry + "_relit")(ctypes.byref(d), ctypes.byref(r), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_the_chains_own_refusals_come_first_and_a_null_descriptor_is_refused(chain):
    from nerftex_hip import lib

    entry, _, make = CHAINS[chain]
    fn = getattr(lib, entry + "_relit")
    r = _relight(K=257, probes=FAKE, probe_shs=FAKE)
    assert fn(None, ctypes.byref(r), None) == NERFTEX_ERR_INVALID and "NULL descriptor" in lib.nerftex_last_error().decode()
    assert fn(None, None, None) == NERFTEX_ERR_INVALID and "NULL descriptor" in lib.nerftex_last_error().decode()
    assert fn(ctypes.byref(make(B=100)), ctypes.byref(r), None) == NERFTEX_ERR_INVALID and "multiple of 128" in lib.nerftex_last_error().decode()
    assert fn(ctypes.byref(make(n_color=2)), ctypes.byref(r), None) == NERFTEX_ERR_INVALID and "at least 9 SH rows" in lib.nerftex_last_error().decode()


@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_an_empty_batch_is_ok_with_and_without_a_relight_descriptor(chain):
    from nerftex_hip import lib

    entry, _, make = CHAINS[chain]
    fn = getattr(lib, entry + "_relit")
    if chain == "shape":
        # its descriptor needs a tracer in front of the empty batch's return, and a tracer needs a device: what a CPU can see is that a valid
        # relight descriptor is let through to that refusal, where the plain entry ends too
        for r in (None, ctypes.byref(_relight()), ctypes.byref(_relight(K=64, probes=FAKE, probe_shs=FAKE, rotation=FAKE))):
            assert fn(ctypes.byref(make(B=0, n_color=3)), r, None) == NERFTEX_ERR_INVALID and "a raytracer is required" in lib.nerftex_last_error().decode()
        return
    assert fn(ctypes.byref(make(B=0)), None, None) == 0
    assert fn(ctypes.byref(make(B=0)), ctypes.byref(_relight()), None) == 0
    assert fn(ctypes.byref(make(B=0, n_color=3)), ctypes.byref(_relight(K=64, probes=FAKE, probe_shs=FAKE, rotation=FAKE)), None) == 0
    assert getattr(lib, entry)(ctypes.byref(make(B=0)), None) == 0, "the plain entry is the _relit body with r == NULL"
