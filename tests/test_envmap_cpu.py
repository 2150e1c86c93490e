"""CPU: relighting the SH light model under an imported environment map (ngp_harness/light.py: envmap_to_sh, sh_to_envmap, image_to_envmap,
SHLightNet.load_envmap / switch_envmap_import / lighting, sh_light_shade_probes; CurvedField's stamp) against what the reference's own
nerf/sh_light_model.py produced on the CPU (tests/golden/ref_python_envmap.npz, tools/make_envmap_golden.py), the float64 model of
tests/envmap_float64.py against the reference's float64 run, and the C ABI of nerftex_envmap_fit / nerftex_sh_light_probe_forward: declared,
exported, bound field for field, every invalid descriptor refused before anything touches a device."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import envmap_float64 as e64
import sh_light_float64 as f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
FAKE = 0x10000  # a non-NULL address that is never dereferenced: every case below is refused before anything is launched


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_envmap.npz"))


# ---- the fit ------------------------------------------------------------------------------------------------------------------------------------------

def test_the_fixture_holds_the_cases_the_stopping_rule_needs(golden):
    assert golden["fit_a_envmap"].shape == (16, 32, 3) and golden["fit_b_envmap"].shape == (13, 29, 3) and golden["fit_a_envmap"].min() > 0
    assert golden["fit_a_loss2001_fp32"] < 1e-6 and golden["fit_a_loss2001_fp64"] < 1e-6 and int(golden["fit_a_steps_fp32"]) == int(golden["fit_a_steps_fp64"]) == 2002
    assert golden["fit_b_loss_fp32"] > 1e-3 and golden["fit_b_loss_fp64"] > 1e-3 and int(golden["fit_b_steps_fp32"]) == int(golden["fit_b_steps_fp64"]) == 5000
    for case in "ab":
        print(f"case {case}: max|fp32 - fp64| {np.abs(golden[f'fit_{case}_fp32'] - golden[f'fit_{case}_fp64']).max():.3e}, tolerance "
              f"{e64.fit_tolerance(golden[f'fit_{case}_fp32'], golden[f'fit_{case}_fp64']):.3e}, max|coefficient| {np.abs(golden[f'fit_{case}_fp64']).max():.3f}")


@pytest.mark.parametrize("case", ("a", "b"))
def test_the_float64_model_on_the_moments_walks_the_references_trajectory(golden, case):
    envmap = golden[f"fit_{case}_envmap"]
    G, b, s = e64.moments(envmap)
    got, steps, losses = e64.adam_fit(G, b, s, envmap.shape[0] * envmap.shape[1])
    err = float(np.abs(got - golden[f"fit_{case}_fp64"]).max())
    print(f"case {case}: the Gram form against the reference's float64 loop: max error {err:.3e}, steps {steps}, loss {losses[-1]:.6e}")
    assert steps == int(golden[f"fit_{case}_steps_fp64"])
    assert err <= 1e-9
    assert abs(losses[-1] - float(golden[f"fit_{case}_loss_fp64"])) <= 1e-9


@pytest.mark.parametrize("case", ("a", "b"))
def test_the_op_by_op_fit_reproduces_the_references(golden, case):
    from ngp_harness.light import envmap_to_sh

    got, info = envmap_to_sh(golden[f"fit_{case}_envmap"], fused=False)
    tol = e64.fit_tolerance(golden[f"fit_{case}_fp32"], golden[f"fit_{case}_fp64"])
    err = float(np.abs(got.numpy() - golden[f"fit_{case}_fp32"]).max())
    print(f"case {case}: op-by-op fit against EnvMap2SH: max error {err:.3e} (tolerance {tol:.3e}), steps {info['steps']}, loss {info['loss']:.6e}")
    assert got.shape == (16, 3) and got.dtype == torch.float32 and not got[9:].any()
    assert info["steps"] == int(golden[f"fit_{case}_steps_fp32"]) and err <= tol
    assert abs(info["loss"] - float(golden[f"fit_{case}_loss_fp32"])) <= 1e-6 * max(1.0, float(golden[f"fit_{case}_loss_fp32"]))


def test_the_fit_renders_back_to_the_map(golden):
    from ngp_harness.light import envmap_to_sh, sh_to_envmap

    got, _ = envmap_to_sh(golden["fit_a_envmap"], fused=False)
    back, dirs = sh_to_envmap(got, 16, 32)
    assert back.shape == (16, 32, 3) and dirs.shape == (16, 32, 3)
    assert float(np.abs(back.numpy() - golden["fit_a_envmap"]).max()) <= 1e-2
    assert np.allclose(dirs.norm(dim=-1).numpy(), 1.0, atol=1e-6)


def test_image_to_envmap_is_the_references_tone_curve():
    from ngp_harness.light import image_to_envmap

    im = np.random.default_rng(0).uniform(0, 1, (5, 7, 4))
    white = image_to_envmap(im.copy())
    want = im[..., :3] ** (1 / 1.24)
    assert white.shape == (5, 7, 3) and np.array_equal(white, np.repeat(want.mean(-1, keepdims=True), 3, -1))
    assert np.array_equal(image_to_envmap(im.copy(), force_white=False), want)


def test_fit_refusals():
    from ngp_harness.light import envmap_to_sh

    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        envmap_to_sh(np.zeros((4, 4)))
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        envmap_to_sh(np.zeros((0, 4, 3)))
    with pytest.raises(ValueError, match="sh_order"):
        envmap_to_sh(np.zeros((2, 2, 3)), sh_order=1)
    with pytest.raises(RuntimeError, match="GPU"):
        envmap_to_sh(np.zeros((2, 2, 3), np.float32), fused=True)


# ---- the head under imported lighting -------------------------------------------------------------------------------------------------------------------

def _probe_args(golden):
    t = lambda k: torch.from_numpy(golden[k])  # noqa: E731
    return t("probe_brdf"), t("probe_normals"), t("probe_dirs"), t("probe_normals_secondary"), t("probes"), t("probe_shs")


def test_the_op_by_op_probe_path_reproduces_the_reference(golden):
    """The four outputs against the reference's, each row shaded as the first of its batch (the fixture's probe_rows_*: the reference scales
    the specular lighting of row b of a batch by exp(-floor(sqrt(b))^2 / 2 / glossiness), tools/make_envmap_golden.py): inside sh_light_float64's
    bounds on both sides of a comparison of two fp32 evaluations, i.e. twice the bound, for the candidate probe either took."""
    from ngp_harness.light import sh_light_shade_probes

    brdf, n, d, n2, probes, tables = _probe_args(golden)
    with torch.no_grad():
        outs = sh_light_shade_probes(brdf, n, d, n2, probes, tables, True, float(golden["gamma"]))
    a_h, sw_h = torch.sigmoid(brdf[:, :3]).numpy(), torch.sigmoid(brdf[:, 3:4]).numpy()
    args = (a_h, sw_h, golden["probe_normals"], golden["probe_dirs"], golden["probe_normals_secondary"], golden["probes"], golden["probe_shs"])
    single = e64.check_probe_shading("op-by-op", np.stack([o.float().numpy() for o in outs]), *args)
    e64.check_probe_shading("the reference, row by row", np.stack([golden["probe_rows_" + k] for k in e64.KEYS]), *args)
    assert single < 1.0, "the reference's grid has coinciding directions: some rows have several candidates"
    for i, key in enumerate(e64.KEYS):
        err = float(np.abs(outs[i].float().numpy() - golden["probe_rows_" + key]).max())
        print(f"{key}: max |op by op - reference| {err:.3e}")
    # rows with one candidate: both sides shaded the same table, the difference is the two fp32 evaluations' rounding
    one = e64.probe_candidates(golden["probe_normals_secondary"], golden["probes"]).sum(-1) == 1
    for i, key in enumerate(("diffuse", "albedo")):
        assert np.abs(outs[2 + i].float().numpy()[one] - golden["probe_rows_" + key][one]).max() <= 1e-5
    assert np.abs(golden["probe_batch_diffuse"] - golden["probe_rows_diffuse"]).max() < 1e-6, "the position in the batch enters the specular term only"


def test_the_uniform_imported_lighting_reproduces_the_reference(golden):
    from ngp_harness.light import sh_light_shade

    brdf, n, d, _, _, _ = _probe_args(golden)
    env = golden["uniform_env_shs"]
    with torch.no_grad():
        outs = sh_light_shade(brdf, n, d, torch.from_numpy(env), True, float(golden["gamma"]))
    ref = f64.shade(torch.sigmoid(brdf[:, :3]).numpy(), torch.sigmoid(brdf[:, 3:4]).numpy(), golden["probe_normals"], golden["probe_dirs"], env, float(golden["gamma"]))
    for i, key in enumerate(e64.KEYS):
        for name, got in (("op by op", outs[i].float().numpy()), ("reference", golden["uniform_" + key])):
            ok = (np.abs(got - ref[key]) <= ref["bound_" + key]) | ref["kink_" + key]
            assert ok.all() and ref["kink_" + key].mean() <= 0.02, (name, key)


def _net():
    from ngp_harness.light import SHLightNet

    torch.manual_seed(0)
    return SHLightNet()


def test_the_import_state_machine(golden):
    net = _net()
    keys = sorted(net.state_dict())
    assert net.import_envmap is False and net.envSHs_import is None and net.envSHs_import_vis is None and net.probes is None
    assert net.switch_envmap_import() is False and net.lighting() is net.envSHs
    env = torch.from_numpy(golden["uniform_env_shs"])
    assert net.load_envmap(env_shs=env) is True and net.import_envmap is True
    net.train()
    assert net.lighting() is net.envSHs, "training ignores the import"
    net.eval()
    assert net.lighting() is net.envSHs_import and torch.equal(net.lighting(), env) and net.lighting() is not env
    assert not net.probe_lighting(True)
    assert net.switch_envmap_import() is False and net.lighting() is net.envSHs
    assert net.switch_envmap_import() is True and net.lighting() is net.envSHs_import
    assert net.load_envmap(env_shs=env, env_shs_vis=golden["probe_shs"], probes=golden["probes"]) is True
    assert net.probe_lighting(True) and not net.probe_lighting(False) and net.envSHs_import_vis.shape == (64, 9, 3) and net.probes.shape == (64, 3)
    net.train()
    assert not net.probe_lighting(True)
    assert sorted(net.state_dict()) == keys, "the imported lighting is not part of the checkpoint"
    assert {"envSHs_import", "envSHs_import_vis", "probes"} <= {n for n, _ in net.named_buffers()}, "it moves with the module"


def test_load_envmap_fits_a_map(golden):
    net = _net()
    assert net.load_envmap(golden["fit_a_envmap"] ** 1.24, force_white=False)  # (load_envmap applies the tone curve ** (1 / 1.24))
    assert net.envSHs_import.shape == (16, 3)
    assert float((net.envSHs_import - torch.from_numpy(golden["fit_a_fp32"])).abs().max()) <= 1e-3


def test_load_envmap_refusals(golden):
    net = _net()
    env, tables, probes = golden["uniform_env_shs"], golden["probe_shs"], golden["probes"]
    for kw in (dict(), dict(envmap=np.zeros((2, 2, 3)), env_shs=env), dict(env_shs=env[:8]), dict(env_shs=env[:, :1]), dict(env_shs=env.reshape(-1)),
               dict(envmap=np.zeros((4, 4))), dict(envmap=np.zeros((4, 0, 3))), dict(env_shs=env, probes=probes), dict(env_shs=env, env_shs_vis=tables),
               dict(env_shs=env, env_shs_vis=tables, probes=probes[:63]), dict(env_shs=env, env_shs_vis=tables[:, :8], probes=probes),
               dict(env_shs=env, env_shs_vis=np.zeros((257, 9, 3)), probes=np.zeros((257, 3))), dict(env_shs=env, env_shs_vis=np.zeros((0, 9, 3)), probes=np.zeros((0, 3)))):
        with pytest.raises(ValueError, match="load_envmap"):
            net.load_envmap(**kw)
    assert net.import_envmap is False and net.envSHs_import is None, "a refused call leaves nothing behind"


def test_forward_shades_with_the_lighting_in_effect(golden, monkeypatch):
    """The head's routing with the BRDF MLP replaced by the fixture's outputs (the MLP runs on the GPU only)."""
    from ngp_harness import light

    net = _net()
    brdf, n, d, n2, probes, tables = _probe_args(golden)
    del net.brdf_layer  # (a registered module: replaced by a plain attribute)
    net.brdf_layer = lambda x: brdf
    geo = torch.zeros(brdf.shape[0], 15)
    env = torch.from_numpy(golden["uniform_env_shs"])
    net.eval()
    with torch.no_grad():
        base = net(geo, n, d)
        net.load_envmap(env_shs=env)
        uniform = net(geo, n, d)
        assert all(torch.equal(a, b) for a, b in zip(uniform, light.sh_light_shade(brdf, n, d, env, True, net.gamma)))
        assert not torch.equal(uniform[0], base[0])
        with pytest.raises(RuntimeError, match=r"load_envmap\(env_shs_vis=, probes=\).*field\.shade_visibility = False"):
            net(geo, n, d, normal_secondary=n2, shade_visibility=True)
        net.load_envmap(env_shs=env, env_shs_vis=tables, probes=probes)
        lit = net(geo, n, d, normal_secondary=n2, shade_visibility=True)
        assert all(torch.equal(a, b) for a, b in zip(lit, light.sh_light_shade_probes(brdf, n, d, n2, probes, tables, True, net.gamma)))
        mask = torch.arange(brdf.shape[0]) % 3 != 0
        masked = net(geo, n, d, mask=mask, normal_secondary=n2, shade_visibility=True)
        assert all(not o[~mask].any() and torch.equal(o[mask], l[mask]) for o, l in zip(masked, lit))
        with pytest.raises(ValueError, match="normal_secondary"):
            net(geo, n, d, shade_visibility=True)
        assert all(torch.equal(a, b) for a, b in zip(net(geo, n, d, normal_secondary=n2, shade_visibility=False), uniform))
        net.switch_envmap_import()
        assert all(torch.equal(a, b) for a, b in zip(net(geo, n, d, normal_secondary=n2, shade_visibility=True), base))
        net.switch_envmap_import()
    net.train()
    assert all(torch.equal(a, b) for a, b in zip(net(geo, n, d, normal_secondary=n2, shade_visibility=True), base)), "training ignores the import"


# ---- the field's stamp ----------------------------------------------------------------------------------------------------------------------------------

def _bare_lit_field(fused_infer):
    from ngp_harness.curved import CurvedField

    f = object.__new__(CurvedField)
    torch.nn.Module.__init__(f)
    f.light_model, f.light_visual_mode, f.fused_light_infer, f.shade_visibility = "SH", "Full", fused_infer, True
    f.light_net = _net()
    enc = types.SimpleNamespace(embeddings=torch.zeros(4), offsets=torch.zeros(2, dtype=torch.int32))
    f.normal_net = types.SimpleNamespace(encoder=enc, phi_net=torch.nn.Linear(2, 2), theta_net=torch.nn.Linear(2, 2))
    return f.eval()


@pytest.mark.parametrize("fused_infer", (False, True))
def test_the_stamp_without_an_import_is_unchanged_and_follows_the_lighting_in_effect(golden, fused_infer):
    f = _bare_lit_field(fused_infer)
    net, nn = f.light_net, f.normal_net
    head = ("SH", "Full", float(net.gamma), True, True, net.envSHs.data_ptr(), (16, 1))
    if fused_infer:
        want = head + (True, nn.encoder.embeddings.data_ptr(), nn.encoder.offsets.data_ptr(),
                       tuple((q.data_ptr(), q._version) for q in list(nn.phi_net.parameters()) + list(nn.theta_net.parameters())))
    else:
        want = head + (False,)
    assert f._light_stamp() == want and len(want) == (11 if fused_infer else 8), "_light_stamp's documented members, nothing more"
    net.load_envmap(env_shs=golden["uniform_env_shs"])
    s1 = f._light_stamp()
    assert s1[:len(want)] == want and s1[len(want):] == (net.envSHs_import.data_ptr(), (16, 3), True, True, 0, 0)
    net.switch_envmap_import()
    s2 = f._light_stamp()
    assert s2 != s1 and s2[len(want):] == (net.envSHs.data_ptr(), (16, 1), False, True, 0, 0)
    net.switch_envmap_import()
    assert f._light_stamp() == s1
    f.shade_visibility = False
    s3 = f._light_stamp()
    assert s3 != s1 and s3[len(want) + 3] is False
    net.load_envmap(env_shs=golden["uniform_env_shs"], env_shs_vis=golden["probe_shs"], probes=golden["probes"])
    s4 = f._light_stamp()
    assert s4 != s3 and s4[-2:] == (net.envSHs_import_vis.data_ptr(), net.probes.data_ptr())
    f.train()
    assert f._light_stamp()[len(want):len(want) + 2] == (net.envSHs.data_ptr(), (16, 1)), "training shades with envSHs"


def test_the_fused_chains_step_aside_for_per_probe_lighting(golden):
    """_infer_light_back_fused over stand-ins that meet every one of its conditions: True under a uniform imported lighting, False while every
    sample is lit by its probe (infer() then takes forward())."""
    f = _bare_lit_field(True)
    mlp = lambda shapes: types.SimpleNamespace(layers=[types.SimpleNamespace(W=torch.zeros(s)) for s in shapes])  # noqa: E731
    f.normal_net = types.SimpleNamespace(bound_output=False, low_freq_band_len_x=16, low_freq_band_len_z=12, phi_net=mlp([(16, 20), (16, 16), (1, 16)]),
                                         theta_net=mlp([(16, 28), (16, 16), (1, 16)]))
    del f.light_net.brdf_layer
    f.light_net.brdf_layer = types.SimpleNamespace(dtype=torch.float16, input_dim=16, hidden_dim=64, num_layers=3, output_dim=5)
    x = types.SimpleNamespace(is_cuda=True)
    assert f._infer_light_back_fused(x) is True
    f.light_net.load_envmap(env_shs=golden["uniform_env_shs"])
    assert f._infer_light_back_fused(x) is False, "shade_visibility without tables: forward() refuses it, the chain must not render it"
    f.shade_visibility = False
    assert f._infer_light_back_fused(x) is True, "a uniform imported lighting renders through the chains"
    f.shade_visibility = True
    f.light_net.load_envmap(env_shs=golden["uniform_env_shs"], env_shs_vis=golden["probe_shs"], probes=golden["probes"])
    assert f._infer_light_back_fused(x) is False
    f.light_net.switch_envmap_import()
    assert f._infer_light_back_fused(x) is True
    f.light_net.switch_envmap_import()
    f.train()
    assert f._infer_light_back_fused(x) is True, "training never sees the import"


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------------

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


@pytest.mark.parametrize("struct,binding", [("nerftex_envmap_fit_desc", "EnvmapFitDesc"), ("nerftex_sh_light_probe_desc", "SHLightProbeDesc"),
                                            ("nerftex_sh_light_desc", "SHLightDesc")])
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
    header = open(HEADER).read()
    for name in ("nerftex_envmap_fit", "nerftex_envmap_fit_scratch_bytes", "nerftex_sh_light_probe_forward"):
        assert hasattr(lib, name) and name in nerftex_hip.EXPORTS and re.search(r"\b" + name + r"\s*\(", header), name
    assert nerftex_hip.SH_LIGHT_MAX_PROBES == 256 and nerftex_hip.SH_LIGHT_SPECULAR == 1
    sizes = nerftex_hip.lib.nerftex_envmap_fit_scratch_bytes
    assert sizes(1, 2) == sizes(8, 8) == sizes(16, 16) == 75 * 8 and sizes(13, 29) == 2 * 75 * 8 and sizes(50, 100) == 20 * 75 * 8
    assert sizes(4096, 8192) == 1024 * 75 * 8, "the grid is capped: a function of H W alone"


def _fit_desc(**over):
    from nerftex_hip import EnvmapFitDesc

    kw = dict(envmap=FAKE, phi=FAKE, theta=FAKE, H=4, W=8, n_sh=16, max_steps=5000, min_steps=2000, lr=1e-2, min_loss=1e-5, env_shs=FAKE, steps_run=FAKE,
              final_loss=FAKE, scratch=FAKE, scratch_bytes=75 * 8)
    kw.update(over)
    return EnvmapFitDesc(**kw)


FIT_REFUSED = [(dict(H=0), "at least one pixel"), (dict(W=0), "at least one pixel"), (dict(n_sh=8), "at least 9 SH rows"), (dict(lr=0.0), "lr is positive"),
               (dict(lr=-1e-2), "lr is positive"), (dict(lr=float("nan")), "lr is positive"), (dict(lr=float("inf")), "lr is positive"),
               (dict(min_loss=float("nan")), "min_loss"), (dict(max_steps=0), "max_steps"), (dict(envmap=None), "must not be NULL"), (dict(phi=None), "must not be NULL"),
               (dict(theta=None), "must not be NULL"), (dict(env_shs=None), "must not be NULL"), (dict(steps_run=None), "must not be NULL"),
               (dict(final_loss=None), "must not be NULL"), (dict(scratch=None), "8-byte aligned"), (dict(scratch=FAKE + 4), "8-byte aligned"),
               (dict(final_loss=FAKE + 4), "8-byte aligned"), (dict(scratch_bytes=75 * 8 - 1), "hold 600 bytes"), (dict(H=13, W=29), "hold 1200 bytes")]
IDS = lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None  # noqa: E731


@pytest.mark.parametrize("over,text", FIT_REFUSED, ids=IDS)
def test_an_invalid_fit_descriptor_is_refused_before_any_device_call(over, text):
    from nerftex_hip import ERR_INVALID, lib

    assert lib.nerftex_envmap_fit(ctypes.byref(_fit_desc(**over)), None) == ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def _probe_desc(**over):
    from nerftex_hip import SHLightProbeDesc

    kw = dict(brdf=FAKE, brdf_stride=16, normals=FAKE, dirs=FAKE, normals_secondary=FAKE, probes=FAKE, probe_shs=FAKE, K=64, mask=None, B=8, gamma=2.4, flags=1,
              color=FAKE, specular=None, diffuse=None, albedo=None)
    kw.update(over)
    return SHLightProbeDesc(**kw)


PROBE_REFUSED = [(dict(K=0), "between 1 and 256 probes"), (dict(K=257), "between 1 and 256 probes"), (dict(brdf_stride=4), "at least 5 values"),
                 (dict(gamma=0.0), "gamma is positive"), (dict(gamma=-2.4), "gamma is positive"), (dict(gamma=float("nan")), "gamma is positive"),
                 (dict(gamma=float("inf")), "gamma is positive"), (dict(flags=2), "unknown flags"), (dict(brdf=None), "must not be NULL"),
                 (dict(normals=None), "must not be NULL"), (dict(dirs=None), "must not be NULL"), (dict(normals_secondary=None), "must not be NULL"),
                 (dict(probes=None), "must not be NULL"), (dict(probe_shs=None), "must not be NULL"), (dict(color=None), "must not be NULL")]


@pytest.mark.parametrize("over,text", PROBE_REFUSED, ids=IDS)
def test_an_invalid_probe_descriptor_is_refused_before_any_device_call(over, text):
    from nerftex_hip import ERR_INVALID, lib

    assert lib.nerftex_sh_light_probe_forward(ctypes.byref(_probe_desc(**over)), None) == ERR_INVALID
    assert text in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()


def test_null_descriptors_and_the_empty_batch():
    from nerftex_hip import ERR_INVALID, lib

    assert lib.nerftex_envmap_fit(None, None) == ERR_INVALID and "NULL descriptor" in lib.nerftex_last_error().decode()
    assert lib.nerftex_sh_light_probe_forward(None, None) == ERR_INVALID and "NULL descriptor" in lib.nerftex_last_error().decode()
    assert lib.nerftex_sh_light_probe_forward(ctypes.byref(_probe_desc(B=0, brdf=None, color=None)), None) == 0, "B == 0: nothing to do, nothing launched"
