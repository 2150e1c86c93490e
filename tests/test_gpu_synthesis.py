"""The texture synthesis on the GPU (ngp_harness.synthesis.synthesize_texture over nerftex_synth_*, csrc/synthesis.inc) against the float64 host
model of tests/synthesis_model.py, which tests/test_synthesis_model_cpu.py holds to the reference's own run.

Tolerances, fixed before any GPU output (tests/synthesis_cases.py derives them from fp32 storage of the coarse sums and of the seam pixels):
  distances   relative error at most rho(cell) = (2^-24 max|db| + 2^-22 |q|) / min d
  decisions   equal to the model's in every cell none of whose margins (rank gap < 2 rho, draw within 4 a rho sum x^(a-1) / sum x^a of a cdf edge,
              a dynamic-program gap below 2 S match_dim 2^-20 max|v|^2) lies under its bound; at most one of a case's 15 cells may be undecided
  canvas      bit-equal to the model on every pixel that is a plain copy of an example pixel, within 2 fp32 ulp of the model's float64 value on
              the pixels that went through a seam's mean (possibly twice in a corner; the model marks them); canvas_id equal everywhere
"""
import numpy as np
import pytest
import torch

import synthesis_cases as sc
import synthesis_model as sm

pytestmark = pytest.mark.gpu
CASES = ("A", "B")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _result(patches, sample_tbn, picked, grid_gap, match_dim, phi_dim):
    """The dict export_field returns, as far as synthesize_texture reads it."""
    has_tbn = patches.shape[-1] > match_dim + phi_dim
    return {"patches": patches[..., :match_dim], "grid_gap": grid_gap, "patch_sample_tbn": sample_tbn, "picked_vertices": picked,
            "patch_phi_embed": patches[..., match_dim:match_dim + phi_dim] if phi_dim else None,
            "patch_local_tbn": patches[..., match_dim + phi_dim:] if has_tbn else None}


def _device_run(name, forced):
    from ngp_harness.synthesis import synthesize_texture

    c = sc.case_inputs(name)
    S = c["patches"].shape[1]
    res = _result(c["patches"], c["sample_tbn"], c["picked_vertices"], c["patch_length"] / S, c["match_dim"], c["phi_dim"])
    return synthesize_texture(res, c["output"], mirror_hor=bool(c["mirrors"]), mirror_vert=bool(c["mirrors"]), max_patch_res=c["max_patch_res"],
                              first_patch=c["first_patch"], draws=c["draws"], forced=c["forced"] if forced else None)


@pytest.fixture(scope="module")
def device_runs(dev):
    return {(name, forced): _device_run(name, forced) for name in CASES for forced in (True, False)}


def _check_canvas(canvas, run, where=None):
    got = canvas.cpu().numpy() if torch.is_tensor(canvas) else canvas
    want, averaged = run["canvas"], run["averaged"]
    if where is not None:
        got, want, averaged = got[where], want[where], averaged[where]
    w32 = want.astype(np.float32)
    copied = ~averaged
    assert np.array_equal(w32[copied].astype(np.float64), want[copied]), "the model's copies are fp32 numbers"
    assert np.array_equal(got[copied].view(np.uint32), w32[copied].view(np.uint32)), "a copied pixel is the example's pixel bit for bit"
    err = np.abs(got.astype(np.float64) - want)[averaged]
    ulp = np.spacing(np.abs(w32)).astype(np.float64)[averaged]
    print("canvas: pixels", averaged.size, "averaged on a seam", int(averaged.sum()), "their largest error in ulp", float((err / ulp).max()) if err.size else 0.0)
    assert averaged.any() and (err <= 2 * ulp).all()


def _check_cells(log, run, cells, und=()):
    """Per cell: k, the ranked ids, the survivors in order, the id the draw picks, the placed id, the distances within rho."""
    worst = 0.0
    for cell in cells:
        if cell in und:
            continue
        m = run["cells"][cell]
        assert log["k"][cell] == m["k"], cell
        assert np.array_equal(log["ranked_ids"][cell], m["ranked_ids"][:16]), cell
        ns = len(m["survivors"])
        assert log["survivor_count"][cell] == ns, cell
        assert np.array_equal(log["survivors"][cell][:min(ns, 16)], m["survivors"][:16]) and (log["survivors"][cell][ns:] == -1).all(), cell
        assert log["drawn"][cell] == m["drawn"] and log["placed"][cell] == m["placed"], cell
        rel = np.abs(log["ranked_dist"][cell] / m["ranked_dist"][:16] - 1).max()
        rho = sc.distance_bound(run, cell)
        worst = max(worst, rel / rho)
        assert rel <= rho, (cell, rel, rho)
    print("ranked distances: largest relative error over its bound", worst)


@pytest.mark.parametrize("name", CASES)
def test_forced_run_follows_the_model(device_runs, name):
    texture, log = device_runs[(name, True)]
    run, c = sc.model_run(name, True), sc.case_inputs(name)
    und = sc.undecided_cells(name, True)
    print("undecided cells:", und)
    assert len(und) <= sc.MAX_UNDECIDED
    assert log["cells_per_side"] == run["n"] and log["examples"] == run["examples"] and log["block"] == run["block"]
    assert log["first_patch"] == c["first_patch"] == log["placed"][0]
    _check_cells(log, run, range(1, run["n"] ** 2), und)
    assert np.array_equal(log["id_map"], run["id_map"])  # forced
    if not any("dp" in why for why in und.values()):
        assert np.array_equal(log["canvas_id"], run["canvas_id"])
        _check_canvas(log["canvas"], run)
        assert np.array_equal(log["total_id"], run["total_id"]) and np.array_equal(log["sample_tbn_ids"], run["sample_tbn_ids"])
        assert np.array_equal(log["sample_tbn"].astype(np.float64), run["sample_tbn"])
        md, phi = c["match_dim"], c["phi_dim"]
        full = log["canvas"]
        assert torch.equal(texture["features"], full[..., :md]) and torch.equal(texture["phi_embed"], full[..., md:md + phi])
        assert torch.equal(texture["local_tbn"], full[..., md + phi:]) and texture["local_tbn"].shape[-1] == 9
        assert set(texture) == {"features", "grid_gap", "phi_embed", "local_tbn", "sample_tbn", "sample_tbn_ids"}
        assert texture["features"].dtype == torch.float32 and texture["sample_tbn_ids"].dtype == torch.int32


@pytest.mark.parametrize("name", CASES)
def test_free_run_follows_the_model(device_runs, name):
    _, log = device_runs[(name, False)]
    run = sc.model_run(name, False)
    und = sc.undecided_cells(name, False)
    assert len(und) <= sc.MAX_UNDECIDED
    cells = run["n"] ** 2
    upto = min(und) if und else cells
    _check_cells(log, run, range(1, upto))
    assert np.array_equal(log["id_map"].reshape(-1)[:upto], run["id_map"].reshape(-1)[:upto])
    if not und:
        assert np.array_equal(log["id_map"], run["id_map"]) and np.array_equal(log["canvas_id"], run["canvas_id"])
        _check_canvas(log["canvas"], run)


def test_two_runs_give_the_same_bits(device_runs):
    _, a = device_runs[("B", False)]
    _, b = _device_run("B", False)
    assert torch.equal(a["canvas"].view(torch.int32), b["canvas"].view(torch.int32))
    for k in ("id_map", "canvas_id", "k", "survivor_count", "drawn", "placed", "ranked_ids", "survivors", "sample_tbn_ids", "total_id"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["ranked_dist"].view(np.uint64), b["ranked_dist"].view(np.uint64))


# ---- cell topologies and row strides: a 2 x 2 and a 3 x 3 canvas, features only ------------------------------------------------------------------------
def _small_problem(P, S, C, seed, n_cells, mirror_hor=False, mirror_vert=False, close_threshold=0.05, max_patch_res=8):
    rng = np.random.default_rng(seed)
    patches = rng.uniform(-0.5, 0.5, (P, S, S, C)).astype(np.float32)
    sample_tbn = (np.eye(3, dtype=np.float32).reshape(9) + rng.normal(0, 0.3, (P, 9))).astype(np.float32)
    picked = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    ps, ov = sm.default_sizes(S)
    output = ov + n_cells * (ps + ov)
    grid_gap = 0.125
    examples = P * (2 if mirror_hor else 1) * (2 if mirror_vert else 1)
    kw = dict(mirror_hor=mirror_hor, mirror_vert=mirror_vert, close_threshold=close_threshold, max_patch_res=max_patch_res,
              first_patch=int(rng.integers(0, examples)), draws=rng.random(n_cells * n_cells - 1))
    run = sm.synthesize(patches, sample_tbn, picked, S * grid_gap, output, match_dim=C, strict_match=True, **kw)
    assert run["n"] == n_cells
    return _result(patches, sample_tbn, picked, grid_gap, C, 0), output, kw, run, float(np.abs(patches).max())


@pytest.mark.parametrize("n_cells,hor,vert,seed", [(2, True, False, 11), (3, False, True, 12)], ids=["2x2-rowflip", "3x3-colflip"])
def test_first_row_first_column_and_interior_cells(dev, n_cells, hor, vert, seed):
    from ngp_harness.synthesis import synthesize_texture

    S, C = 8, 16
    res, output, kw, run, vmax = _small_problem(20, S, C, seed, n_cells, mirror_hor=hor, mirror_vert=vert)
    und = {cell: why for cell in range(1, n_cells ** 2) if (why := sc.undecided(run, cell, S, C, vmax))}
    assert not und, und  # (a property of the seeded inputs, checked on the host)
    texture, log = synthesize_texture(res, output, **kw)
    assert texture["phi_embed"] is None and texture["local_tbn"] is None and texture["sample_tbn"] is None and texture["sample_tbn_ids"] is None
    assert tuple(texture["features"].shape) == (run["side"], run["side"], C)
    groups = {"first row": [c for c in range(1, n_cells)], "first column": [c * n_cells for c in range(1, n_cells)],
              "interior": [r * n_cells + c for r in range(1, n_cells) for c in range(1, n_cells)]}
    ps, ov = run["patch_size"], run["overlap_size"]
    # the log is compared per group of cells, the canvas as a whole and on the last cell's rectangle
    for name, cells in groups.items():
        assert cells, name
        _check_cells(log, run, cells)
        assert np.array_equal(log["id_map"].reshape(-1)[cells], run["id_map"].reshape(-1)[cells]), name
    assert (log["id_map"] >= 20).any(), "a flipped example is placed"
    assert np.array_equal(log["canvas_id"], run["canvas_id"])
    _check_canvas(log["canvas"], run)
    assert np.array_equal(log["sample_tbn"].astype(np.float64), run["sample_tbn"]) and np.array_equal(log["sample_tbn_ids"], run["sample_tbn_ids"])
    # the last cell's rectangle, which nothing overwrote: the seams of an interior cell (2 x 2: the one cell with both cuts)
    y0 = (ps + ov) * (n_cells - 1)
    _check_canvas(log["canvas"], run, (slice(y0, y0 + S), slice(y0, y0 + S)))


# ---- example counts at wave and workgroup edges of the select launch (64 lanes, 1024 threads) ------------------------------------------------------------
@pytest.mark.parametrize("P", [63, 64, 65, 257, 1025])
def test_ranking_at_example_count_edges(dev, P):
    from ngp_harness.synthesis import synthesize_texture

    S, C = 8, 4
    res, output, kw, run, _ = _small_problem(P, S, C, 100 + P, 2)
    _, log = synthesize_texture(res, output, **kw)
    m = run["cells"][1]
    rho = sc.distance_bound(run, 1)
    assert m["rank_margin"] >= 2 * rho, "the seeded inputs rank without a close call"
    assert np.array_equal(log["ranked_ids"][1], m["ranked_ids"][:16])
    rel = np.abs(log["ranked_dist"][1] / m["ranked_dist"][:16] - 1).max()
    print("P", P, "relative error", rel, "bound", rho)
    assert rel <= rho and log["k"][1] == 16 and log["survivor_count"][1] == 16


# ---- the error path ---------------------------------------------------------------------------------------------------------------------------------------
def test_k_past_the_example_set_is_a_host_visible_status(dev):
    from ngp_harness.synthesis import SynthesisExhausted, synthesize_texture

    c = sc.case_inputs("B")
    S = c["patches"].shape[1]
    res = _result(c["patches"], c["sample_tbn"], c["picked_vertices"], 1e3 / S, c["match_dim"], c["phi_dim"])  # every vertex is "close" to every other
    with pytest.raises(SynthesisExhausted, match="cell 1"):
        synthesize_texture(res, c["output"], mirror_hor=True, mirror_vert=True, max_patch_res=c["max_patch_res"], first_patch=c["first_patch"], draws=c["draws"])
    # the process is healthy: the same inputs with the fixture's patch_length run through
    _, log = _device_run("B", True)
    assert np.array_equal(log["id_map"], sc.model_run("B", True)["id_map"])


def test_first_patch_and_refused_options(dev):
    from ngp_harness.synthesis import synthesize_texture

    res, output, kw, _, _ = _small_problem(20, 8, 4, 5, 2)
    with pytest.raises(ValueError, match="first_patch"):
        synthesize_texture(res, output, **dict(kw, first_patch=20))
    with pytest.raises(NotImplementedError, match="blend"):
        synthesize_texture(res, output, mode="blend", **kw)
    with pytest.raises(NotImplementedError, match="quilt"):
        synthesize_texture(res, output, quilt=True, **kw)
    with pytest.raises(NotImplementedError, match="non-square"):
        synthesize_texture(res, (output, output + 1), **kw)
    with pytest.raises(NotImplementedError, match="picked_vertices"):
        synthesize_texture(dict(res, picked_vertices=None), output, **kw)
    with pytest.raises(RuntimeError, match="overlap_size"):
        synthesize_texture(res, output, patch_size=3, overlap_size=3, **kw)


# ---- end to end: export -> synthesize -> import -> infer --------------------------------------------------------------------------------------------------
def test_export_synthesize_import_infer(dev):
    import patch_float64 as pm
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=pm.H_THRESHOLD, light_model="SH").to(dev)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.normal_net.encoder.embeddings.uniform_(-0.5, 0.5)
    field.eval()
    P = pm.patch_problem(12, True)
    out = field.export_field(P["points"], P["normals"], scan_points=P["scan"], first_component=pm.FIRST_COMPONENT, grid_gap=P["grid_gap"], patch_size=P["S"],
                             sample_mesh=(P["v"], P["cast_f"]))
    n_patches = out["patches"].shape[0]
    assert n_patches >= 4
    # (close_threshold 0: the filter removes nothing, so the four-fold example set of even a few patches holds k = 16)
    texture, log = field.synthesize_field(out, 40, mirror_hor=True, mirror_vert=True, close_threshold=0.0, max_patch_res=4, seed=7)
    assert set(texture) == {"features", "grid_gap", "phi_embed", "local_tbn", "sample_tbn", "sample_tbn_ids"} and field.imported
    side = log["canvas_id"].shape[0]
    assert tuple(texture["features"].shape) == (side, side, 16) and tuple(texture["phi_embed"].shape) == (side, side, 8) and side >= 40
    assert np.array_equal(log["draws"], np.random.RandomState(7).random_sample(log["cells_per_side"] ** 2 - 1))
    # an interior copied pixel: the middle of the last cell, outside both overlaps
    n, ps, ov, S = log["cells_per_side"], log["patch_size"], log["overlap_size"], 12
    y = (ps + ov) * (n - 1) + ov + ps // 2
    ex = int(log["canvas_id"][y, y])
    assert ex == log["id_map"][n - 1, n - 1]
    base, m = ex % n_patches, ex // n_patches
    i = j = ov + ps // 2
    ii, jj = (S - 1 - i if m & 1 else i), (S - 1 - j if m >> 1 else j)
    assert np.array_equal(texture["features"][y, y].cpu().numpy(), out["patches"][base, ii, jj])
    assert np.array_equal(texture["phi_embed"][y, y].cpu().numpy(), out["patch_phi_embed"][base, ii, jj])
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.rand(512, 2, generator=g) * 1.6 - 0.8, torch.rand(512, 1, generator=g) * 0.5 * pm.H_THRESHOLD], dim=1).to(dev)
    d = torch.nn.functional.normalize(torch.randn(512, 3, generator=g), dim=-1).to(dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        sigma, rgbs = field.infer(x, d)
    assert torch.isfinite(sigma).all() and torch.isfinite(rgbs).all() and tuple(rgbs.shape) == (512, 3)
    assert (sigma > 0).any(), "points above the plane lie inside the field's shell"
