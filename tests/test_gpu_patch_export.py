"""CurvedField.export_field on the GPU (nerftex_patch_front): the batched form against the staged form bit for bit, against the float64 model of
tests/patch_float64.py on everything float64 can decide, the table reads against the package's own calls on the exported coordinates, one patch
back in through import_field, and the refusal of an imported field.  The cases are tests/patch_float64.py's (48 candidates, S in {3, 8, 12}).

Tolerances (fixed in tests/test_patch_export_cpu.py before any GPU output): verdicts equal on every decided candidate, hits within 2 tol_t +
origin bound (1 + 1 / cos) on every decided ray of an accepted patch, no share of failures.  `patches`, `patch_local_tbn` and `patch_phi_embed` are
not held to float64 -- the hash cell of a rounded point is not float64's to decide -- but to the staged form and to projector / encoder /
phi_embedding called on `patch_coors`, bit for bit."""
import numpy as np
import pytest
import torch

import patch_float64 as m

pytestmark = pytest.mark.gpu
ARRAYS = ("patches", "patch_coors", "patch_norms", "patch_sample_tbn", "patch_local_tbn", "picked_vertices", "patch_phi_embed", "patch_rays",
          "candidate_ids", "verdicts")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _field(dev, light_model):
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=m.H_THRESHOLD, light_model=light_model).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        if field.normal_net is not None:
            field.normal_net.encoder.embeddings.uniform_(-0.5, 0.5)
    return field.eval()


@pytest.fixture(scope="module")
def fields(dev):
    return {True: _field(dev, "SH"), False: _field(dev, None)}


def _export(field, P, **kw):
    return field.export_field(P["points"], P["normals"], scan_points=P["scan"], first_component=m.FIRST_COMPONENT, grid_gap=P["grid_gap"], patch_size=P["S"],
                              sample_mesh=(P["v"], P["cast_f"]), **kw)


def _same(a, b, what):
    assert set(a) == set(b)
    assert a["grid_gap"] == b["grid_gap"]
    for k in ARRAYS:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (what, k)


def _shapes(out, P, lit, rays):
    S, n = P["S"], len(out["candidate_ids"])
    want = {"patches": (n, S, S, 16), "patch_coors": (n, S, S, 3), "patch_norms": (n, 3), "patch_sample_tbn": (n, 9), "patch_local_tbn": (n, S, S, 9),
            "picked_vertices": (n, 3), "candidate_ids": (n,), "verdicts": (P["n"],)}
    for k, shape in want.items():
        assert out[k].shape == shape and out[k].dtype == (np.int64 if k == "candidate_ids" else np.uint8 if k == "verdicts" else np.float32), k
    assert (out["patch_phi_embed"].shape == (n, S, S, 8)) if lit else out["patch_phi_embed"] is None
    assert (out["patch_rays"].shape == (n, S, S, 6)) if rays else out["patch_rays"] is None
    assert isinstance(out["grid_gap"], float)


# ---- 1. the batched form against the staged form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", [True, False], ids=["scan", "noscan"])
@pytest.mark.parametrize("S", m.SIZES)
def test_fused_equals_staged_bit_for_bit(fields, S, scan):
    """Every chunking (1, 7 and 64 candidates per call), the cap reached in mid-chunk, never and at once; with and without a
    normal net; with the rays recorded."""
    P = m.patch_problem(S, scan)
    n_pass = int((m.verdicts(P)[0] == m.ACCEPTED).sum())
    for lit, rays, caps in ((True, True, (2000, 5)), (False, False, (2000,))):
        field = fields[lit]
        for cap in caps:
            staged = _export(field, P, max_patch_num=cap, record_rays=rays, fused=False)
            _shapes(staged, P, lit, rays)
            if cap == 5:
                assert (staged["verdicts"] == m.NOT_NEEDED).sum() >= 3 and len(staged["candidate_ids"]) == 5 < n_pass - 2
            for chunk in (1, 7, 64):
                fused = _export(field, P, max_patch_num=cap, record_rays=rays, patches_per_chunk=chunk)
                _same(fused, staged, f"S={S} scan={scan} lit={lit} cap={cap} chunk={chunk}")
    # all refused: a cast mesh none of the rays meets (far away), every sent candidate is a miss or far from the scan cloud
    away = (P["v"] + np.float32([50, 0, 0]), P["cast_f"])
    kw = dict(scan_points=P["scan"], first_component=m.FIRST_COMPONENT, grid_gap=P["grid_gap"], patch_size=S, sample_mesh=away)
    none_f = fields[False].export_field(P["points"], P["normals"], patches_per_chunk=7, **kw)
    none_s = fields[False].export_field(P["points"], P["normals"], fused=False, **kw)
    _same(none_f, none_s, "all refused")
    assert len(none_f["candidate_ids"]) == 0 and none_f["patches"].shape == (0, S, S, 16) and not (none_f["verdicts"] == m.ACCEPTED).any()
    # all accepted: only the candidates the model accepts, uncapped and capped at exactly their number
    keep = np.flatnonzero(m.verdicts(P)[0] == m.ACCEPTED)[:9]
    kw.update(sample_mesh=(P["v"], P["cast_f"]))
    for cap in (2000, len(keep)):
        all_f = fields[True].export_field(P["points"][keep], P["normals"][keep], max_patch_num=cap, patches_per_chunk=4, **kw)
        all_s = fields[True].export_field(P["points"][keep], P["normals"][keep], max_patch_num=cap, fused=False, **kw)
        _same(all_f, all_s, "all accepted")
        decided = m.verdicts(P)[1][keep]
        assert (all_f["verdicts"][decided] == m.ACCEPTED).all()


# ---- 2. against float64 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", [True, False], ids=["scan", "noscan"])
@pytest.mark.parametrize("S", m.SIZES)
def test_against_the_float64_model(fields, oracle, S, scan):
    P = m.set_tolerances(m.patch_problem(S, scan), lambda v, f, o, d: oracle.raytrace(v, f, o, d)[:4])
    for cap, chunk in ((2000, 7), (10, 64), (10, 3)):
        out = _export(fields[False], P, max_patch_num=cap, patches_per_chunk=chunk)
        r = m.check_export(P, out, cap)
        print(f"S {S} scan {scan} cap {cap}: {r['decided']} of {P['n']} candidates decided, {r['rays']} rays compared, worst position error {r['worst']:.3f} of its tolerance")
        assert r["rays"] > 0


def test_the_default_arguments_are_the_helpers(fields):
    """first_component, grid_gap and the cast mesh default to the field's own mesh, its principal direction and its edges."""
    from ngp_harness import patches
    from ngp_harness.curved import star_flower_mesh

    P = m.patch_problem(8, False)
    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    field = fields[False]
    out = field.export_field(P["points"][:12], P["normals"][:12], patch_size=4, pattern_rate=0.5)
    assert out["grid_gap"] == patches.patch_grid_gap(v, f, 0.5)
    again = field.export_field(P["points"][:12], P["normals"][:12], patch_size=4, grid_gap=patches.patch_grid_gap(v, f, 0.5),
                               first_component=patches.principal_direction(v), sample_mesh=(v, f), fused=False)
    _same(out, again, "defaults")
    assert len(out["candidate_ids"]) >= 1


# ---- 3. what is not held to float64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", m.SIZES)
def test_table_reads_are_the_packages_own_calls_on_the_exported_coordinates(fields, dev, S):
    field = fields[True]
    out = _export(field, m.patch_problem(S, True))
    assert len(out["candidate_ids"]) >= 3
    x = torch.from_numpy(out["patch_coors"].reshape(-1, 3)).to(dev)
    with torch.no_grad(), torch.autocast("cuda", enabled=False):
        p_sur, _, _, _, tbn = field.projector.project(x, K=field.projector.K, h_threshold=field.h_threshold)
        want = {"patches": field.encoder(p_sur, bound=field.bound), "patch_local_tbn": tbn.reshape(-1, 9), "patch_phi_embed": field.normal_net.phi_embedding(p_sur)}
    for k, t in want.items():
        got = out[k].reshape(-1, out[k].shape[-1])
        assert np.array_equal(got.view(np.uint32), t.float().cpu().numpy().view(np.uint32)), k
    assert np.abs(out["patches"]).max() > 0.1 and np.abs(out["patch_phi_embed"]).max() > 0.1


# ---- 4. round trip -----------------------------------------------------------------------------------------------------------------------------------------
def test_an_exported_patch_goes_back_in_through_import_field(dev):
    S = 8
    field = _field(dev, "SH")
    out = _export(field, m.patch_problem(S, True))
    i = 1
    field.import_field(out["patches"][i], out["grid_gap"], phi_embed=out["patch_phi_embed"][i], local_tbn=out["patch_local_tbn"][i],
                       sample_tbn=out["patch_sample_tbn"][i:i + 1], sample_tbn_ids=np.zeros((S, S), np.float32))
    assert field.imported and field.rescale
    # texel (a, b)'s centre: u = 2 a / (S - 1) - 1 along the map's first axis, v along its second; rescale: u, v = x, y
    a, b = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    x = np.stack([2 * a / (S - 1) - 1, 2 * b / (S - 1) - 1, np.zeros_like(a, dtype=np.float64)], -1).reshape(-1, 3).astype(np.float32)
    x = torch.from_numpy(np.concatenate([x, x])).to(dev)  # 128 rows
    d = torch.zeros_like(x)
    d[:, 2] = -1.0
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        embed = field.embed(x)[0]
        sigma, rgbs = field.infer(x, d)
    assert torch.isfinite(sigma).all() and torch.isfinite(rgbs).all() and sigma.shape == (128,) and rgbs.shape == (128, 3)
    got = embed[:S * S, :16].float().cpu().numpy().astype(np.float64)
    want = out["patches"][i].reshape(-1, 16).astype(np.float64)
    # the texel itself: its bilinear weight is 1 up to the float32 rounding of the texel coordinate (a neighbour enters with at most 2^-20 S), and the
    # features leave as 16-bit values (2^-11 relative)
    tol = 2.0 ** -11 * np.abs(want) + 2.0 ** -20 * S * np.abs(want).max() + 2.0 ** -24
    assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) / tol).max())
    # ... and an imported field refuses to export
    with pytest.raises(NotImplementedError, match="switch_import"):
        _export(field, m.patch_problem(S, True))
    field.switch_import()
    again = _export(field, m.patch_problem(S, True))
    _same(again, out, "after switch_import")


def test_an_imported_field_refuses(dev):
    field = _field(dev, None)
    field.import_field(np.zeros((4, 4, 16), np.float32), 0.1)
    P = m.patch_problem(3, True)
    for fused in (True, False):
        with pytest.raises(NotImplementedError, match="switch_import"):
            _export(field, P, fused=fused)
