"""CPU: the host side of relighting through the fused lit chains -- the rotation matrix against the reference's scipy matrices
(tests/golden/ref_python_relight.npz, tools/make_relight_golden.py), the state machine of CurvedField.set_light_rotation and forward(euler=), the
graph stamp, the predicate over the stand-ins of tests/test_envmap_cpu.py, and the op-by-op rotation against what the reference handed its light
head.

The op-by-op rotation runs HERE, on the CPU, as the fixture was made: the framework does not autocast CPU tensors, so the einsum is an fp32 product
on both sides (the fixture records that as cpu_einsum_is_fp32).  The half product the GPU computes is held to the same captured vectors through
tests/relight_float64.py -- one half ulp for each of the recorded rounding points, plus the fp32 error of the captured vectors; the framework's
own half einsum is compared with that model on the GPU (tests/test_gpu_relight.py)."""
import os
import types

import numpy as np
import pytest
import torch

import relight_float64 as r64
import test_envmap_cpu as env_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_relight.npz"))


@pytest.fixture(scope="module")
def envmap():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_envmap.npz"))


def test_the_fixture_holds_what_the_tests_need(golden):
    assert bool(golden["cpu_einsum_is_fp32"]) and golden["sigma"].shape == (768,) and 0.3 < golden["h_mask"].mean() < 0.9
    assert [list(golden[f"r{i}_euler"]) for i in range(3)] == [[0, 0, 0], [0, np.pi / 3, 0], [0.4, -1.1, 0.7]]
    for i in range(3):
        for key in ("head_normal", "head_view_dirs", "head_normal_secondary", "uniform_full", "probe_full"):
            assert golden[f"r{i}_{key}"].shape == (768, 3) and np.isfinite(golden[f"r{i}_{key}"]).all(), (i, key)
    for mode in ("specular", "diffuse", "albedo"):
        assert golden[f"r2_uniform_{mode}"].shape == golden[f"r2_probe_{mode}"].shape == (768, 3)
    assert np.abs(golden["r1_uniform_full"] - golden["r0_uniform_full"]).max() > 1e-2 and np.abs(golden["r2_probe_full"] - golden["r0_probe_full"]).max() > 1e-2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_python_relight.npz")) < 300 * 1024


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------------------------------

def test_the_matrix_is_scipys_to_1e_15(golden):
    from ngp_harness.curved import CurvedField

    for i in range(3):
        got = CurvedField.light_rotation_matrix(golden[f"r{i}_euler"])
        assert got.dtype == np.float64 and got.shape == (3, 3)
        err = float(np.abs(got - golden[f"r{i}_matrix"]).max())
        print(f"euler {list(golden[f'r{i}_euler'])}: max|Rodrigues - scipy| {err:.3e}")
        assert err <= 1e-15
        assert np.abs(r64.rodrigues(golden[f"r{i}_euler"]) - golden[f"r{i}_matrix"]).max() <= 1e-15, "the test model's own matrix"
    assert np.array_equal(CurvedField.light_rotation_matrix([0.0, 0.0, 0.0]), np.eye(3)), "a zero vector: the identity exactly"
    for bad in ([1.0, 2.0], [0.0, float("nan"), 0.0], [[1.0, 0.0, 0.0]] * 2):
        with pytest.raises(ValueError, match="rotation vector of 3 values"):
            CurvedField.light_rotation_matrix(bad)


# ---- the state machine ------------------------------------------------------------------------------------------------------------------------------------------

def test_set_light_rotation_writes_one_persistent_buffer_in_place(golden):
    f = env_cpu._bare_lit_field(True)
    assert f.light_rotation() is None and not f._light_rotation_active() and f._relight_desc() is None
    f.set_light_rotation(None)  # (nothing set: nothing to switch off)
    assert f.light_rotation() is None and getattr(f, "_light_rotation", None) is None, "None gives no rotation, and no buffer"
    f.set_light_rotation(golden["r1_euler"])
    buf = f._light_rotation
    assert buf.dtype == torch.float32 and buf.shape == (9,) and buf.device == f.light_net.envSHs.device
    assert np.array_equal(buf.numpy().reshape(3, 3), golden["r1_matrix"].astype(np.float32))
    assert f.light_rotation() == tuple(golden["r1_euler"]) and f._light_rotation_active()
    where = buf.data_ptr()
    f.set_light_rotation(golden["r2_euler"])
    assert f._light_rotation is buf and buf.data_ptr() == where, "a second vector: the same storage"
    assert np.array_equal(buf.numpy().reshape(3, 3), golden["r2_matrix"].astype(np.float32))
    f.set_light_rotation([0.0, 0.0, 0.0])
    assert f._light_rotation_active() and f.light_rotation() == (0.0, 0.0, 0.0), "a zero vector is a rotation: the identity product rounds to half"
    assert np.array_equal(buf.numpy().reshape(3, 3), np.eye(3, dtype=np.float32)) and buf.data_ptr() == where
    f.train()
    assert not f._light_rotation_active() and f.light_rotation() == (0.0, 0.0, 0.0), "training: kept, not applied (the reference's `not self.training`)"
    f.eval()
    f.set_light_rotation(None)
    assert f.light_rotation() is None and not f._light_rotation_active()
    f.set_light_rotation(golden["r1_euler"])
    assert f._light_rotation.data_ptr() == where, "switched on again: still the same storage"


def test_forward_takes_euler_and_it_overrides_the_stored_rotation(golden, monkeypatch):
    from ngp_harness.curved import CurvedField

    f = env_cpu._bare_lit_field(True)
    seen = []
    monkeypatch.setattr(CurvedField, "_forward_light", lambda self, x, d, normal_supervision=False, rotation=None: seen.append(rotation))
    x = d = torch.zeros(4, 3)
    f.forward(x, d)
    assert seen[-1] is None
    f.forward(x, d, euler=golden["r2_euler"])
    assert seen[-1].dtype == torch.float32 and np.array_equal(seen[-1].numpy(), golden["r2_matrix"].astype(np.float32)), "no stored rotation: the keyword's"
    f.set_light_rotation(golden["r1_euler"])
    f.forward(x, d)
    assert seen[-1].data_ptr() == f._light_rotation.data_ptr() and tuple(seen[-1].shape) == (3, 3), "the stored rotation: a view of the buffer"
    f.forward(x, d, euler=golden["r2_euler"])
    assert np.array_equal(seen[-1].numpy(), golden["r2_matrix"].astype(np.float32)), "the keyword overrides the stored rotation"
    f.forward(x, d, euler=None)
    assert seen[-1] is None, "euler=None: no rotation for this call"
    assert f.light_rotation() == tuple(golden["r1_euler"]), "the override does not touch what is stored"
    f.train()
    f.forward(x, d)
    assert seen[-1] is None, "training does not rotate"


def test_the_static_field_refuses_a_rotation():
    from ngp_harness.curved import CurvedField

    f = object.__new__(CurvedField)
    torch.nn.Module.__init__(f)
    f.light_model = None
    f.eval()
    f.set_light_rotation(None)
    with pytest.raises(ValueError, match="static field has no light model"):
        f.set_light_rotation([0.0, 1.0, 0.0])
    with pytest.raises(ValueError, match="static field has no light model"):
        f.forward(torch.zeros(2, 3), torch.zeros(2, 3), euler=[0.0, 1.0, 0.0])
    f._light_rotation_on = True  # (however it got there: it is not ignored)
    with pytest.raises(ValueError, match="static field has no light model"):
        f.forward(torch.zeros(2, 3), torch.zeros(2, 3))


# ---- the stamp --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fused_infer", (False, True))
def test_the_stamp_gains_three_members_and_never_the_rotations_values(envmap, golden, fused_infer):
    f = env_cpu._bare_lit_field(fused_infer)
    net, nn = f.light_net, f.normal_net
    head = ("SH", "Full", float(net.gamma), True, True, net.envSHs.data_ptr(), (16, 1))
    if fused_infer:
        want = head + (True, nn.encoder.embeddings.data_ptr(), nn.encoder.offsets.data_ptr(),
                       tuple((q.data_ptr(), q._version) for q in list(nn.phi_net.parameters()) + list(nn.theta_net.parameters())))
    else:
        want = head + (False,)
    # switch off, no rotation: today's tuple, through the cases of test_the_stamp_without_an_import_is_unchanged...
    assert f._light_stamp() == want
    f.fused_relight_infer = False
    f.set_light_rotation(None)
    assert f._light_stamp() == want, "the switch explicitly off and the rotation explicitly off: still today's tuple"
    net.load_envmap(env_shs=envmap["uniform_env_shs"])
    imported = (net.envSHs_import.data_ptr(), (16, 3), True, True, 0, 0)
    assert f._light_stamp() == want + imported
    net.load_envmap(env_shs=envmap["uniform_env_shs"], env_shs_vis=envmap["probe_shs"], probes=envmap["probes"])
    tables = (net.envSHs_import.data_ptr(), (16, 3), True, True, net.envSHs_import_vis.data_ptr(), net.probes.data_ptr())
    assert f._light_stamp() == want + tables
    # the switch on: exactly three more members
    f.fused_relight_infer = True
    assert f._light_stamp() == want + tables + (True, False, 0)
    f.set_light_rotation(golden["r1_euler"])
    s1 = f._light_stamp()
    assert s1 == want + tables + (True, True, f._light_rotation.data_ptr())
    f.set_light_rotation(golden["r2_euler"])
    assert f._light_stamp() == s1, "another rotation vector: an equal stamp (the recorded graphs replay)"
    f.set_light_rotation([0.0, 0.0, 0.0])
    assert f._light_stamp() == s1
    f.set_light_rotation(None)
    assert f._light_stamp() == want + tables + (True, False, 0) != s1, "rotation off: another stamp (the graphs re-record)"
    # a rotation without the switch: the three members too (infer() is forward() then, which reads the buffer)
    f.fused_relight_infer = False
    f.set_light_rotation(golden["r1_euler"])
    assert f._light_stamp() == want + tables + (False, True, f._light_rotation.data_ptr())
    net.load_envmap(env_shs=envmap["uniform_env_shs"], env_shs_vis=envmap["probe_shs"] * 2, probes=envmap["probes"])
    assert f._light_stamp()[-5:-3] == (net.envSHs_import_vis.data_ptr(), net.probes.data_ptr()), "new probe tables: their storage is in the stamp"


def test_the_static_fields_stamp_is_empty():
    from ngp_harness.curved import CurvedField

    f = object.__new__(CurvedField)
    torch.nn.Module.__init__(f)
    f.light_model, f.fused_relight_infer = None, True
    assert f._light_stamp() == ()


# ---- the predicate and the descriptor ---------------------------------------------------------------------------------------------------------------------------

def _chain_field():
    """test_the_fused_chains_step_aside_for_per_probe_lighting's stand-ins: every condition of _infer_light_back_fused met."""
    f = env_cpu._bare_lit_field(True)
    mlp = lambda shapes: types.SimpleNamespace(layers=[types.SimpleNamespace(W=torch.zeros(s)) for s in shapes])  # noqa: E731
    f.normal_net = types.SimpleNamespace(bound_output=False, low_freq_band_len_x=16, low_freq_band_len_z=12, phi_net=mlp([(16, 20), (16, 16), (1, 16)]),
                                         theta_net=mlp([(16, 28), (16, 16), (1, 16)]))
    del f.light_net.brdf_layer
    f.light_net.brdf_layer = types.SimpleNamespace(dtype=torch.float16, input_dim=16, hidden_dim=64, num_layers=3, output_dim=5)
    return f, types.SimpleNamespace(is_cuda=True, device=torch.device("cpu"))  # (the tables of these stand-ins live on the CPU)


def test_the_predicate_holds_under_per_probe_lighting_only_with_the_switch_and_the_tables(envmap, golden):
    f, x = _chain_field()
    assert f._infer_light_back_fused(x) is True and f._relight_desc() is None
    f.light_net.load_envmap(env_shs=envmap["uniform_env_shs"], env_shs_vis=envmap["probe_shs"], probes=envmap["probes"])
    assert f._infer_light_back_fused(x) is False, "switch off, per-probe lighting: forward()"
    f.fused_relight_infer = True
    assert f._infer_light_back_fused(x) is True, "switch on with tables"
    desc, keep = f._relight_desc()
    assert desc.K == 64 and desc.probes == f.light_net.probes.data_ptr() and desc.probe_shs == f.light_net.envSHs_import_vis.data_ptr() and not desc.rotation
    elsewhere = types.SimpleNamespace(is_cuda=True, device=torch.device("meta"))
    assert f._infer_light_back_fused(elsewhere) is False, "tables on another device than x"
    f.light_net.load_envmap(env_shs=envmap["uniform_env_shs"])
    assert f._infer_light_back_fused(x) is False, "switch on without tables: forward() raises there, the chain must not render it"
    f.shade_visibility = False
    assert f._infer_light_back_fused(x) is True and f._relight_desc() is None, "a uniform imported lighting: the plain entry"
    f.shade_visibility = True
    f.light_net.load_envmap(env_shs=envmap["uniform_env_shs"], env_shs_vis=envmap["probe_shs"], probes=envmap["probes"])
    f.train()
    assert f._infer_light_back_fused(x) is True and f._relight_desc() is None, "training: True, and no relight descriptor is built"
    f.set_light_rotation(golden["r1_euler"])
    assert f._infer_light_back_fused(x) is True and f._relight_desc() is None, "training with a stored rotation: still none"


def test_a_rotation_sends_infer_to_forward_unless_the_switch_is_on(envmap, golden):
    f, x = _chain_field()
    f.set_light_rotation(golden["r2_euler"])
    assert f._infer_light_back_fused(x) is False, "switch off, a rotation set: forward()"
    f.fused_relight_infer = True
    assert f._infer_light_back_fused(x) is True
    desc, keep = f._relight_desc()
    assert desc.K == 0 and not desc.probes and not desc.probe_shs and desc.rotation == f._light_rotation.data_ptr(), "a rotation alone (n_color 1 or 3)"
    assert f._infer_light_back_fused(types.SimpleNamespace(is_cuda=True, device=torch.device("meta"))) is False, "the buffer on another device than x"
    f.light_net.load_envmap(env_shs=envmap["uniform_env_shs"], env_shs_vis=envmap["probe_shs"], probes=envmap["probes"])
    desc, keep = f._relight_desc()
    assert desc.K == 64 and desc.rotation == f._light_rotation.data_ptr() and desc.probes == f.light_net.probes.data_ptr()
    f.set_light_rotation(None)
    assert f._relight_desc()[0].rotation is None


# ---- the op-by-op rotation against what the reference handed its head ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", (0, 1, 2))
def test_the_op_by_op_rotation_reproduces_the_references_head_inputs(golden, i):
    from ngp_harness.curved import CurvedField

    rot = torch.from_numpy(CurvedField.light_rotation_matrix(golden[f"r{i}_euler"]).astype(np.float32))
    names = ("head_view_dirs", "head_normal", "head_normal_secondary")
    before = [torch.from_numpy(golden["none_" + n]) for n in names]
    got = CurvedField._rotate_lighting(rot, *before)
    assert CurvedField._rotate_lighting(rot, before[0], before[1], None)[2] is None
    for name, v, g in zip(names, before, got):
        want = golden[f"r{i}_{name}"]
        mag = np.abs(v.numpy().astype(np.float64)) @ np.abs(rot.numpy().astype(np.float64)).T
        err = np.abs(g.numpy().astype(np.float64) - want)
        # fp32 on both sides: three products and two additions each, in whatever order: 5 u sum|terms| per side
        assert g.dtype == torch.float32 and float((err / (10 * U * mag + 1e-30)).max()) <= 1.0, name
        # the GPU's half product, through its recorded rounding points: half roundings of the inputs and of the output, two fp32 accumulations
        # (relight_float64), plus the captured vector's own fp32 error
        m = r64.rotate(rot.numpy(), v.numpy())
        bar = m["bound"] + r64.unrounded_bound(rot.numpy(), v.numpy()) + 5 * U * mag
        herr = np.abs(m["value"] - want)
        print(f"r{i} {name}: fp32 op by op against the reference max {float(err.max()):.2e}; the half product against it max {float(herr.max()):.2e}, "
              f"largest error / bar {float((herr / bar).max()):.3f} (a half ulp near 1: {2.0 ** -11:.1e})")
        assert float((herr / bar).max()) <= 1.0, name
        if i == 0:
            assert np.array_equal(m["value"], r64.half(v.numpy())), "zeros: the identity product is the half rounding, nothing else"
