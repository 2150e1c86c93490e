"""GPU: the per-probe visibility lighting of an imported map through nerftex_envmap_vis_fit (csrc/envmap_vis.inc).
  * the fixture's replay case (3 probes, 40 rounds x 96 points, the reference's own points) against the reference's float64 run on them;
  * the library's own stream at 4 probes x 800 rounds x 1024 points with points_out: unit points, a uniform z, points that differ between probes,
    rounds and seeds, the same bits from the same seed, the tables against the float64 loop (tests/probe_table_float64.py) on the points used,
    and the points fed back;
  * the default 64-probe fit against the mean of the reference's runs under 8 torch seeds;
  * batch = 1 and 257, K = 1 and 256;
  * SHLightNet.load_envmap(visibility=True) on a small SH-lit field: forward(), the _relit chain, the graphed frame.
Tolerances are the reference's own fp32-against-float64 gaps on replayed streams (g_replay, g_full in tests/golden/ref_python_probe_tables.npz),
x 8, + 1e-6 (probe_table_float64.tolerance) -- never the kernel's output.  Every comparison prints its figures (DESIGN.md 4.24 records them)."""
import os

import numpy as np
import pytest
import torch

import probe_table_float64 as p64

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OWN = dict(rounds=800, batch=1024, seed=11)
OWN_PROBES = [9, 27, 36, 63]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ref_python_probe_tables.npz"))


@pytest.fixture(scope="module")
def head():
    return np.load(os.path.join(GOLDEN, "ref_python_envmap.npz"))


def _fit(dev, golden, probes, **kw):
    from ngp_harness.light import envmap_probe_tables

    return envmap_probe_tables(torch.from_numpy(golden["env_shs"]).to(dev), torch.from_numpy(np.ascontiguousarray(probes)), **kw)


@pytest.fixture(scope="module")
def own(dev, golden):
    """One run on the library's own points, shared (and left unchanged) by the tests below."""
    tables, _, points = _fit(dev, golden, golden["probes"][OWN_PROBES], points_out=True, **OWN)
    torch.cuda.synchronize()
    return tables, points


def test_the_replay_case_against_the_references_float64_run(dev, golden):
    points = torch.from_numpy(golden["replay_points"]).to(dev)
    tables, _ = _fit(dev, golden, golden["probes"][golden["replay_probe_index"]], rounds=40, batch=96, points=points)
    err = np.abs(tables.cpu().numpy().astype(np.float64) - golden["replay_fp64"]).max(axis=(1, 2))
    tol = p64.tolerance(golden["g_replay"])
    print(f"replay case: max |kernel - reference float64| per probe {err}, tolerance {tol:.3e}; the reference's own fp32 run: {float(golden['g_replay']):.3e}")
    assert tables.shape == (3, 9, 3) and tables.dtype == torch.float32
    assert err.max() <= tol
    assert np.abs(golden["replay_zero_grad"] - golden["replay_fp64"]).max() > 100 * tol, "a cleared gradient would miss by orders of magnitude"
    again, _ = _fit(dev, golden, golden["probes"][golden["replay_probe_index"]], rounds=40, batch=96, points=points)
    assert torch.equal(again, tables)


def test_the_own_stream_is_uniform_on_the_sphere(own):
    _, points = own
    assert points.shape == (4, 800, 1024, 3) and points.dtype == torch.float32
    off = float((points.double().norm(dim=-1) - 1).abs().max())
    z_mean = points[..., 2].double().mean(dim=-1)
    print(f"own stream: largest | |p| - 1 | {off:.3e}; largest |mean z| over a round {float(z_mean.abs().max()):.4f} (bound {5 / np.sqrt(3 * 1024):.4f})")
    assert off <= 1e-6
    assert float(z_mean.abs().max()) <= 5 / np.sqrt(3 * 1024)  # a uniform z has variance 1 / 3; 5 sigma of a round's mean
    assert not torch.equal(points[0], points[1]) and not torch.equal(points[2], points[3]), "probes have their own points"
    assert not torch.equal(points[0, 0], points[0, 1]) and not torch.equal(points[0, 1], points[0, 799]), "rounds have their own points"
    assert torch.unique(points[0, 0], dim=0).shape[0] == 1024, "samples have their own points"


def test_the_same_seed_gives_the_same_bits_and_another_seed_other_points(dev, golden, own):
    tables, points = own
    again_t, _, again_p = _fit(dev, golden, golden["probes"][OWN_PROBES], points_out=True, **OWN)
    assert torch.equal(again_t, tables) and torch.equal(again_p, points)
    plain, _ = _fit(dev, golden, golden["probes"][OWN_PROBES], **OWN)
    assert torch.equal(plain, tables), "storing the points does not change them"
    other_t, _, other_p = _fit(dev, golden, golden["probes"][OWN_PROBES], points_out=True, **dict(OWN, seed=12))
    assert not torch.equal(other_p, points) and not torch.equal(other_t, tables)
    fed, _ = _fit(dev, golden, golden["probes"][OWN_PROBES], rounds=800, batch=1024, points=points)
    assert torch.equal(fed, tables), "the points fed back give the bits of the run that drew them"


def test_the_own_stream_tables_against_the_float64_loop_on_the_points_used(golden, own):
    tables, points = own
    pts = points.cpu().numpy()
    tol = p64.tolerance(golden["g_full"])
    got = tables.cpu().numpy().astype(np.float64)
    for j, i in enumerate(OWN_PROBES):
        want = p64.fit(golden["env_shs"], golden["lobes"][i], pts[j])
        err = float(np.abs(got[j] - want).max())
        print(f"probe {i}, 800 x 1024 on its own points: max |kernel - float64| {err:.3e} (tolerance {tol:.3e}); DC {golden['env_shs'][0, 0]:.2f} -> {got[j, 0, 0]:.4f}")
        assert err <= tol


def test_the_default_fit_lies_within_the_references_spread_over_seeds(dev, golden):
    from ngp_harness.light import envmap_probe_tables

    tables, probes = envmap_probe_tables(torch.from_numpy(golden["env_shs"]).to(dev))
    assert tables.shape == (64, 9, 3) and np.array_equal(probes.cpu().numpy(), golden["probes"])
    got = tables.cpu().numpy().astype(np.float64)[golden["seed_probe_index"]]
    miss = np.abs(got - golden["seed_mean"])
    sigma = float(golden["sigma_max"])
    print(f"seed case: largest |kernel - mean of 8 reference runs| {miss.max():.4f} = {miss.max() / sigma:.2f} sigma_max (sigma_max {sigma:.4f}, bound 6); "
          f"per probe {miss.max(axis=(1, 2))}")
    assert np.isfinite(got).all() and miss.max() <= 6 * sigma  # 108 numbers against a mean of eight


@pytest.mark.parametrize("K,batch", [(2, 1), (2, 257), (1, 96)])
def test_small_and_odd_batches_and_one_probe(dev, golden, K, batch):
    rng = np.random.default_rng(100 * K + batch)
    pts = rng.normal(size=(K, 5, batch, 3))
    pts = (pts / np.linalg.norm(pts, axis=-1, keepdims=True)).astype(np.float32)
    idx = [27, 63][:K]
    tables, _ = _fit(dev, golden, golden["probes"][idx], rounds=5, batch=batch, points=torch.from_numpy(pts).to(dev))
    tol = p64.tolerance(golden["g_replay"])
    for j, i in enumerate(idx):
        want = p64.fit(golden["env_shs"], golden["lobes"][i], pts[j])
        err = float(np.abs(tables[j].cpu().numpy() - want).max())
        print(f"K {K}, batch {batch}, probe {i}: max |kernel - float64| {err:.3e} (tolerance {tol:.3e})")
        assert err <= tol


def test_256_probes_run(dev, golden):
    probes = np.tile(golden["probes"], (4, 1))
    pts = torch.from_numpy(np.tile(golden["replay_points"][:1, :4], (256, 1, 1, 1))).to(dev)
    tables, _ = _fit(dev, golden, probes, rounds=4, batch=96, points=pts)
    assert tables.shape == (256, 9, 3) and bool(torch.isfinite(tables).all())
    assert torch.equal(tables[:64], tables[64:128]) and torch.equal(tables[:64], tables[192:]), "the same probe on the same points: the same bits in every workgroup"
    assert not torch.equal(tables[0], tables[9])
    with pytest.raises(ValueError, match="1 <= K <= 256"):
        _fit(dev, golden, np.tile(golden["probes"], (5, 1))[:257], rounds=1, batch=1)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------

def test_a_field_relit_with_computed_tables(dev, golden, head, monkeypatch):
    import nerftex_hip
    from ngp_harness import scene
    from ngp_harness.model import Renderer
    from test_gpu_envmap import _reset, _sh_field

    field, v = _sh_field(dev)
    net = field.light_net
    rng = np.random.default_rng(5)
    n = 256
    ids = 36 + np.arange(n) % (v.shape[0] - 72)
    vn = field.projector.vertex_normals.cpu().numpy()
    x = torch.from_numpy((v[ids] + rng.uniform(-0.04, 0.04, size=(n, 1)).astype(np.float32) * vn[ids]).astype(np.float32)).to(dev)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d = torch.from_numpy(d / np.linalg.norm(d, axis=-1, keepdims=True)).to(dev)
    envmap = head["fit_a_envmap"] ** 1.24  # (load_envmap applies the tone curve ** (1 / 1.24))
    _reset(field)
    try:
        r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
        with torch.autocast("cuda", dtype=torch.float16):
            r.update_extra_state_device()
        o, dd = scene.get_rays(scene.rand_poses(1, 1.6, np.random.default_rng(11))[0], scene.intrinsics(32, 32), 32, 32)
        ro, rd = torch.from_numpy(o).to(dev), torch.from_numpy(dd).to(dev)
        kw = dict(dt_gamma=0.0, max_steps=256, slots_per_ray=4)
        graphed = lambda: r.render_infer_graphed(ro, rd, parts=2, block=2, **kw)  # noqa: E731
        field.fused_light_infer = field.fused_relight_infer = True
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            img0, _, _ = graphed()
            before = r._infer_graphs
            graphed()
            assert r._infer_graphs is before
            assert net.load_envmap(envmap, force_white=False, visibility=True, seed=2) is True
            assert net.envSHs_import_vis.shape == (64, 9, 3) and net.envSHs_import_vis.is_cuda and net.probe_lighting(True)
            img1, dep1, _ = graphed()
            after = r._infer_graphs
            assert after is not before and not torch.equal(img1, img0), "the tables appear: the frame is re-recorded"
            graphed()
            assert r._infer_graphs is after, "... once"
            want = r.render_infer(ro, rd, **kw)
            assert torch.equal(img1, want[0]) and torch.equal(dep1, want[1])
            # infer() takes the _relit chain
            calls = []
            fn = nerftex_hip.lib.nerftex_curved_light_infer_relit
            monkeypatch.setattr(nerftex_hip.lib, "nerftex_curved_light_infer_relit", lambda *a: (calls.append("relit"), fn(*a))[1])
            field.infer(x, d)
            assert calls == ["relit"]
            monkeypatch.undo()
            # forward() with computed tables is forward() with the same tables handed in
            sigma, color, _ = field(x, d)
            saved, env = net.probe_tables(), net.envSHs_import.clone()
            _reset(field)
            net.load_envmap(env_shs=env, env_shs_vis=saved["envSHs"], probes=saved["probes"])
            sigma2, color2, _ = field(x, d)
            assert torch.equal(sigma, sigma2) and torch.equal(color, color2) and float(color.float().std()) > 1e-3
            field.shade_visibility = False
            assert not torch.equal(field(x, d)[1], color), "per-probe lighting is another lighting than the uniform one"
    finally:
        _reset(field)
        field.fused_relight_infer = False
