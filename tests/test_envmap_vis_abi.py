"""C-ABI surface of nerftex_envmap_vis_fit (CPU only): the descriptor is declared and bound field for field, the entry is declared, exported and
bound, and every refusal the header lists returns NERFTEX_ERR_INVALID with its message before anything touches a device -- the descriptors below
point at addresses that are never dereferenced, on a machine without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
NERFTEX_ERR_INVALID = 1
FAKE = 0x10000  # a non-NULL, aligned address that is never dereferenced
FIELDS = ["env_shs", "n_sh", "lobes", "K", "rounds", "batch", "lr", "seed", "points", "points_out", "tables"]


def _desc(**over):
    from nerftex_hip import EnvmapVisFitDesc

    kw = dict(env_shs=FAKE, n_sh=16, lobes=FAKE, K=64, rounds=800, batch=1024, lr=1e-3, seed=0, points=None, points_out=None, tables=FAKE)
    kw.update(over)
    return EnvmapVisFitDesc(**kw)


def test_the_struct_is_declared_and_bound_field_for_field(tmp_path):
    import nerftex_hip

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct nerftex_envmap_vis_fit_desc \{(.*?)\} nerftex_envmap_vis_fit_desc;", src, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["const float* env_shs", "uint32_t n_sh", "const float* lobes", "uint32_t K", "uint32_t rounds", "uint32_t batch", "double lr",
                     "uint64_t seed", "const float* points", "float* points_out", "float* tables"]
    assert [n for n, _ in nerftex_hip.EnvmapVisFitDesc._fields_] == FIELDS
    # the C compiler's layout of the struct is the binding's
    prog = tmp_path / "layout.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "nerftex_hip.h"', "int main(void) {",
             '    printf("sizeof %lu\\n", (unsigned long)sizeof(nerftex_envmap_vis_fit_desc));']
    lines += [f'    printf("{n} %lu\\n", (unsigned long)offsetof(nerftex_envmap_vis_fit_desc, {n}));' for n in FIELDS]
    lines += ["    return 0;", "}"]
    prog.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["sizeof"]) == ctypes.sizeof(nerftex_hip.EnvmapVisFitDesc)
    for n in FIELDS:
        assert int(out[n]) == getattr(nerftex_hip.EnvmapVisFitDesc, n).offset, n


def test_the_entry_is_declared_exported_and_bound():
    import nerftex_hip

    src = open(HEADER).read()
    assert re.search(r"\bint nerftex_envmap_vis_fit\(const nerftex_envmap_vis_fit_desc\* d, void\* stream\);", src)
    assert "NOT torch.rand's" in src, "the header says whose random stream the points come from"
    assert hasattr(ctypes.CDLL(nerftex_hip.LIB_PATH), "nerftex_envmap_vis_fit") and "nerftex_envmap_vis_fit" in nerftex_hip.EXPORTS
    fn = nerftex_hip.lib.nerftex_envmap_vis_fit
    assert list(fn.argtypes) == [ctypes.c_void_p] * 2 and fn.restype is ctypes.c_int


REFUSED = [
    (dict(env_shs=None), "env_shs, lobes and tables must not be NULL"),
    (dict(lobes=None), "env_shs, lobes and tables must not be NULL"),
    (dict(tables=None), "env_shs, lobes and tables must not be NULL"),
    (dict(n_sh=8), "at least 9 SH rows, but got 8"),
    (dict(n_sh=0), "at least 9 SH rows, but got 0"),
    (dict(K=0), "1 to 256 probes, but got 0"),
    (dict(K=257), "1 to 256 probes, but got 257"),
    (dict(rounds=0), "rounds and batch are positive, but got 0 and 1024"),
    (dict(batch=0), "rounds and batch are positive, but got 800 and 0"),
    (dict(lr=0.0), "lr is positive and finite"),
    (dict(lr=-1e-3), "lr is positive and finite"),
    (dict(lr=float("inf")), "lr is positive and finite"),
    (dict(lr=float("nan")), "lr is positive and finite"),
]


@pytest.mark.parametrize("over,text", REFUSED, ids=[f"{i}-{next(iter(t[0]))}" for i, t in enumerate(REFUSED)])
def test_what_the_entry_refuses(over, text):
    from nerftex_hip import lib

    assert lib.nerftex_envmap_vis_fit(ctypes.byref(_desc(**over)), None) == NERFTEX_ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_a_null_descriptor_is_refused():
    from nerftex_hip import lib

    assert lib.nerftex_envmap_vis_fit(None, None) == NERFTEX_ERR_INVALID and "NULL descriptor" in lib.nerftex_last_error().decode()
