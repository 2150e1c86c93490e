"""CPU: computing the per-probe visibility lighting of an imported map (ngp_harness/light.py: probe_grid, visibility_lobes, fit_product_of_shs,
envmap_probe_tables, SHLightNet.load_envmap(visibility=True) / load_envmap_with_visibility / probe_tables) against what the reference's own
nerf/sh_light_model.py produced on the CPU (tests/golden/ref_python_probe_tables.npz, tools/make_probe_table_golden.py), and the float64 loop of
tests/probe_table_float64.py against the reference's float64 run.  The reference never clears its gradient between steps; a variant that does is
shown NOT to pass."""
import os

import numpy as np
import pytest
import torch

import probe_table_float64 as p64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(rounds=3, batch=8)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_probe_tables.npz"))


@pytest.fixture(scope="module")
def head():
    return np.load(os.path.join(ROOT, "tests", "golden", "ref_python_envmap.npz"))


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------------------

def test_the_probe_grid_is_the_references_bit_for_bit(golden):
    from ngp_harness.light import probe_grid

    got = probe_grid()
    assert got.dtype == torch.float32 and got.shape == (64, 3)
    assert np.array_equal(got.numpy(), golden["probes"])
    grid = got.reshape(8, 8, 3)
    assert float((grid[:, 7] - grid[:, 0]).abs().max()) < 1e-6, "both ends of the azimuth are included: the last column repeats the first"
    assert float(grid[0, 0, 1]) == float(torch.cos(torch.tensor(np.pi / 8, dtype=torch.float32))), "the first row sits at pi / 8, not on the pole"
    pole = grid[7]
    assert (pole[:, 1] == -1.0).all() and float(pole[:, [0, 2]].abs().max()) <= 1e-7, "the last row is eight copies of the pole"
    assert pole[:, [0, 2]].abs().max() > 0, "... as float32 computes it: sin(fp32 pi) is -8.7e-8, not 0"
    assert probe_grid(2, 3).shape == (6, 3)


def test_the_rotated_lobes_are_the_references(golden):
    from ngp_harness.light import visibility_lobes

    got = visibility_lobes(torch.from_numpy(golden["probes"]))
    err = float(np.abs(got.numpy() - golden["lobes"]).max())
    extra = visibility_lobes(golden["extra_normals"])
    err_extra = float(np.abs(extra.numpy() - golden["extra_lobes"]).max())
    print(f"lobes: max error on the grid {err:.3e}, on the extra normals {err_extra:.3e}; largest value {np.abs(golden['lobes']).max():.3f}")
    assert got.shape == (64, 9) and got.dtype == torch.float32
    assert err <= 1e-6 and err_extra <= 1e-6  # fp32 rounding of values up to about 1
    assert np.allclose(extra[0].numpy(), golden["lobe"], atol=1e-7), "+z: the identity"
    assert not np.allclose(extra[2].numpy(), golden["lobe"], atol=1e-4) or golden["extra_normals"][2, 2] > 0.999, "n_z = 0.9995 takes the special case"
    assert np.array_equal(extra[2].numpy(), extra[0].numpy()), "n_z > 0.999: the frame is replaced by the identity"
    # the lobe at its own probe direction has the unrotated lobe's value at +z
    own = (p64.basis9(golden["probes"]) * got.double().numpy()).sum(-1)
    assert np.abs(own - float(golden["lobe_at_z"])).max() < 1e-5
    with pytest.raises(ValueError, match="visibility_lobes"):
        visibility_lobes(torch.zeros(4))


# ---- the fit on the fixture's points --------------------------------------------------------------------------------------------------------------------

def test_the_fixture_tells_a_cleared_gradient_apart(golden):
    g = float(golden["g_replay"])
    assert golden["replay_points"].shape == (3, 40, 96, 3) and list(golden["replay_probe_index"]) == [9, 27, 63]
    assert np.abs(golden["replay_fp32"] - golden["replay_fp64"]).max() == pytest.approx(g) and g < 5e-6 and float(golden["g_full"]) < 2e-5
    assert np.abs(golden["replay_zero_grad"] - golden["replay_fp32"]).max() > 100 * g
    print(f"g_replay {g:.3e}, g_full {float(golden['g_full']):.3e}, sigma_max {float(golden['sigma_max']):.4f}")


def test_the_float64_loop_walks_the_references_float64_trajectory(golden):
    for j, i in enumerate(golden["replay_probe_index"]):
        got = p64.fit(golden["env_shs"], golden["lobes"][i], golden["replay_points"][j])
        err = float(np.abs(got - golden["replay_fp64"][j]).max())
        print(f"probe {i}: float64 loop against the reference's float64 run: {err:.3e}")
        assert err <= float(golden["g_replay"])


def test_the_op_by_op_fit_reproduces_the_references(golden):
    from ngp_harness.light import fit_product_of_shs

    env, tol = torch.from_numpy(golden["env_shs"]), 4 * float(golden["g_replay"])
    for j, i in enumerate(golden["replay_probe_index"]):
        got = fit_product_of_shs(env, torch.from_numpy(golden["lobes"][i]), rounds=40, batch=96, points=torch.from_numpy(golden["replay_points"][j]))
        err = float(np.abs(got.numpy() - golden["replay_fp32"][j]).max())
        print(f"probe {i}: op-by-op fit against fit_product_of_SHs: max error {err:.3e} (tolerance {tol:.3e})")
        assert got.shape == (9, 3) and got.dtype == torch.float32 and err <= tol


def test_a_fit_that_clears_its_gradient_does_not_pass(golden):
    """What the reference does NOT do.  The same checks as above, applied to a loop with zero_grad: both fail, by orders of magnitude."""
    for j, i in enumerate(golden["replay_probe_index"]):
        cleared = p64.fit(golden["env_shs"], golden["lobes"][i], golden["replay_points"][j], zero_grad=True)
        miss = float(np.abs(cleared - golden["replay_fp64"][j]).max())
        assert miss > 100 * p64.tolerance(golden["g_replay"]), miss
        assert float(np.abs(cleared - golden["replay_zero_grad"][j]).max()) <= p64.tolerance(golden["g_replay"]), "... and it is the cleared loop the fixture holds"


def test_envmap_probe_tables_on_the_cpu(golden):
    from ngp_harness.light import envmap_probe_tables, fit_product_of_shs, probe_grid, visibility_lobes

    env = torch.from_numpy(golden["env_shs"])
    probes = torch.from_numpy(golden["probes"][[9, 27, 63]])
    pts = torch.from_numpy(golden["replay_points"])
    tables, out_probes = envmap_probe_tables(env, probes, rounds=40, batch=96, points=pts)
    assert tables.shape == (3, 9, 3) and torch.equal(out_probes, probes)
    assert float(np.abs(tables.numpy() - golden["replay_fp32"]).max()) <= 4 * float(golden["g_replay"])
    # its own points: torch.rand, phi first, from the seed; handed back, they give the same bits
    a, grid, used = envmap_probe_tables(env, seed=3, points_out=True, **SMALL)
    b, _ = envmap_probe_tables(env, seed=3, **SMALL)
    c, _ = envmap_probe_tables(env, seed=4, **SMALL)
    d, _ = envmap_probe_tables(env, points=used, **SMALL)
    assert a.shape == (64, 9, 3) and torch.equal(grid, probe_grid()) and used.shape == (64, 3, 8, 3)
    assert torch.equal(a, b) and torch.equal(a, d) and not torch.equal(a, c)
    assert float((used.norm(dim=-1) - 1).abs().max()) < 1e-6
    assert torch.equal(a[5], fit_product_of_shs(env, visibility_lobes(grid)[5], points=used[5], **SMALL))
    for kw in (dict(rounds=0), dict(batch=0), dict(lr=0.0), dict(lr=float("nan")), dict(probes=torch.zeros(257, 3)), dict(probes=torch.zeros(0, 3)),
               dict(points=torch.zeros(64, 3, 7, 3), **SMALL)):
        with pytest.raises(ValueError, match="envmap_probe_tables"):
            envmap_probe_tables(env, **kw)
    with pytest.raises(ValueError, match="envmap_probe_tables"):
        envmap_probe_tables(env[:8])
    with pytest.raises(RuntimeError, match="no fused CPU path"):
        envmap_probe_tables(env, fused=True, **SMALL)


# ---- the module -----------------------------------------------------------------------------------------------------------------------------------------

def _net():
    from ngp_harness.light import SHLightNet

    torch.manual_seed(0)
    return SHLightNet()


def test_load_envmap_computes_the_tables_and_forward_takes_them(golden, head):
    from ngp_harness import light

    net = _net()
    t = lambda k: torch.from_numpy(head[k])  # noqa: E731
    brdf, n, d, n2 = t("probe_brdf"), t("probe_normals"), t("probe_dirs"), t("probe_normals_secondary")
    del net.brdf_layer  # (a registered module: replaced by a plain attribute; the MLP runs on the GPU only)
    net.brdf_layer = lambda x: brdf
    geo = torch.zeros(brdf.shape[0], 15)
    env = torch.from_numpy(golden["env_shs"])
    net.eval()
    with torch.no_grad():
        assert net.load_envmap(env_shs=env) is True
        assert net.envSHs_import_vis is None and net.probes is None, "visibility=False: the state of before"
        with pytest.raises(RuntimeError, match="no probe tables are loaded"):
            net(geo, n, d, normal_secondary=n2, shade_visibility=True)
        with pytest.raises(RuntimeError, match="probe_tables"):
            net.probe_tables()
        assert net.load_envmap(env_shs=env, visibility=True, seed=5, vis_fit=SMALL) is True
        assert net.envSHs_import_vis.shape == (64, 9, 3) and net.envSHs_import_vis.dtype == torch.float32 and net.probes.shape == (64, 3)
        assert torch.equal(net.probes, light.probe_grid()) and net.probe_lighting(True)
        want, _ = light.envmap_probe_tables(env, seed=5, **SMALL)
        assert torch.equal(net.envSHs_import_vis, want)
        lit = net(geo, n, d, normal_secondary=n2, shade_visibility=True)
        assert all(torch.equal(a, b) for a, b in zip(lit, light.sh_light_shade_probes(brdf, n, d, n2, net.probes, net.envSHs_import_vis, True, net.gamma)))
        # the reference's _vis.npz content, round trip
        saved = net.probe_tables()
        assert sorted(saved) == ["envSHs", "probes"] and saved["envSHs"].shape == (64, 9, 3) and saved["envSHs"].dtype == np.float32
        other = _net()
        del other.brdf_layer
        other.brdf_layer = lambda x: brdf
        other.eval()
        other.load_envmap(env_shs=env, env_shs_vis=saved["envSHs"], probes=saved["probes"])
        assert all(torch.equal(a, b) for a, b in zip(other(geo, n, d, normal_secondary=n2, shade_visibility=True), lit))
        # under the reference's name, for a lighting already imported
        third = _net()
        third.load_envmap(env_shs=env)
        assert third.load_envmap_with_visibility(seed=5, **SMALL) is True and torch.equal(third.envSHs_import_vis, want)
        assert third.load_envmap_with_visibility(seed=6, **SMALL) and not torch.equal(third.envSHs_import_vis, want), "another seed, other points"


def test_load_envmap_fits_a_map_and_its_tables(head):
    net = _net()
    assert net.load_envmap(head["fit_a_envmap"] ** 1.24, force_white=False, visibility=True, vis_fit=SMALL)
    assert net.envSHs_import.shape == (16, 3) and net.envSHs_import_vis.shape == (64, 9, 3)
    # three rounds at lr 1e-3 move a coefficient by at most 3e-3 (Adam's step is bounded by lr while the gradient keeps its sign; loosely 2 x)
    assert float((net.envSHs_import_vis - net.envSHs_import[None, :9]).abs().max()) <= 6e-3


def test_refusals(golden):
    net = _net()
    with pytest.raises(RuntimeError, match="no lighting is imported"):
        net.load_envmap_with_visibility()
    env = golden["env_shs"]
    tables, probes = np.zeros((64, 9, 3), np.float32), golden["probes"]
    for kw in (dict(env_shs_vis=tables, probes=probes), dict(probes=probes), dict(env_shs_vis=tables)):
        with pytest.raises(ValueError, match="visibility=True"):
            net.load_envmap(env_shs=env, visibility=True, **kw)
    assert net.import_envmap is False and net.envSHs_import is None and net.envSHs_import_vis is None, "a refused call leaves nothing behind"
