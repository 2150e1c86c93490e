"""The patch export on the CPU: the host helpers of ngp_harness/patches.py against the reference's numpy lines restated here, the cases of
tests/patch_float64.py (each is the one described, under its exclusion cap), and the model's checker against deliberately wrong fronts."""
import numpy as np
import pytest

import patch_float64 as m

REPORT = []
CANDIDATE_CAP, RAY_CAP = 0.25, 0.02
CASES = [(S, scan, cap) for S in m.SIZES for scan in (True, False) for cap in (2000, 10)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        print("\n" + "\n".join(REPORT))


def _mesh():
    import geometry_float64 as g

    return g.star_flower_mesh(18, 36)


# ------------------------------------------------------------------------------------------------------------------------ helpers
def test_patch_grid_gap_is_the_reference_lines():
    from ngp_harness.patches import patch_grid_gap

    v, f = _mesh()
    v8, fi = v.astype(np.float64), f.astype(np.int64)
    # trimesh's edges_unique: the sorted vertex pairs of every face's three edges, unique rows (tools/map.py:966-969)
    pairs = set()
    for a, b, c in fi.tolist():
        pairs |= {tuple(sorted(p)) for p in ((a, b), (b, c), (c, a))}
    edges_unique = np.array(sorted(pairs))
    edges = v8[edges_unique]
    edges = np.linalg.norm(edges[:, 0] - edges[:, 1], axis=-1)
    mean_edge_length = edges.mean()
    for rate in (1 / 50, 0.125):
        assert patch_grid_gap(v, f, rate) == mean_edge_length * rate
    assert patch_grid_gap(v, f) == mean_edge_length * (1 / 50)


def test_principal_direction_is_sklearns_first_component():
    from ngp_harness.patches import principal_direction

    rng = np.random.default_rng(3)
    clouds = [_mesh()[0], rng.normal(size=(500, 3)) * np.array([0.3, 2.0, 1.0]), -np.abs(rng.normal(size=(40, 3))) * np.array([5.0, 1.0, 0.2]) + 7.0]
    for v in clouds:
        c = principal_direction(v)
        v8 = np.asarray(v, dtype=np.float64)
        # the definition: the unit eigenvector of the covariance's largest eigenvalue, largest entry positive
        w, vec = np.linalg.eigh(np.cov((v8 - v8.mean(0)).T))
        e = vec[:, -1]
        e = e * np.sign(e[np.argmax(np.abs(e))])
        assert abs(np.linalg.norm(c) - 1) < 1e-12 and np.abs(c - e).max() < 1e-9 and c[np.argmax(np.abs(c))] > 0
    try:
        from sklearn.decomposition import PCA
    except ImportError:
        return  # (the comparison with sklearn itself needs sklearn)
    for v in clouds:
        pca = PCA(n_components=3)
        pca.fit(np.asarray(v, dtype=np.float64))
        assert np.abs(principal_direction(v) - pca.components_[0]).max() < 1e-9  # (two solvers of one eigenproblem: not bit for bit)


def test_patch_calibration_and_pixel_order():
    from ngp_harness.patches import patch_calibration

    for S, gap in ((3, 0.01), (8, 0.0037), (128, 1.2345e-3)):
        calibration = np.linspace(-S * gap / 2, S * gap / 2, S)
        assert np.array_equal(patch_calibration(S, gap), calibration)
    # pixel p = i S + j sits at (cal[i], cal[j]): tools/map.py:986-987
    cal = patch_calibration(4, 0.5)
    x, y = np.meshgrid(cal, cal, indexing="ij")
    patch_coor = np.stack([x, y], axis=-1).reshape([-1, 2])
    for i in range(4):
        for j in range(4):
            assert tuple(patch_coor[i * 4 + j]) == (cal[i], cal[j])


def test_patch_frames_are_the_reference_lines():
    from ngp_harness.patches import patch_frames

    rng = np.random.default_rng(9)
    n = rng.normal(size=(40, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    p = rng.normal(size=(40, 3))
    first = np.array([0.6, -0.64, 0.48])
    n[3] = first                      # parallel, generic direction: the fallback's 1.01 makes a frame
    n[4] = np.array([1.0, 1.0, 0.0]) / np.sqrt(2)  # y_axis sums to zero without being zero: the fallback as written
    got = patch_frames(p, n, first)
    assert got.shape == (40, 3, 4) and got.dtype == np.float64
    assert np.array_equal(got, m.reference_frames(p, n, first), equal_nan=True)
    assert np.isfinite(got).all()
    ok = np.delete(np.arange(40), [3])
    R = got[ok][:, :, :3]
    assert np.abs(np.einsum("nab,nac->nbc", R, R) - np.eye(3)).max() < 1e-12 and np.array_equal(got[:, :, 2], n) and np.array_equal(got[:, :, 3], p)
    # an axis-aligned first component: the fallback is zero as well and the frame NaN (refused later by the NaN test)
    axis = np.array([1.0, 0.0, 0.0])
    bad = patch_frames(p[:2], np.stack([axis, n[0]]), axis)
    assert np.isnan(bad[0, :, :2]).all() and np.isfinite(bad[1]).all()
    assert np.array_equal(bad, m.reference_frames(p[:2], np.stack([axis, n[0]]), axis), equal_nan=True)
    assert np.array_equal(patch_frames(m.patch_problem(3, True)["points"], m.patch_problem(3, True)["normals"], m.FIRST_COMPONENT),
                          m.patch_problem(3, True)["frames"], equal_nan=True)


def test_scan_limit_is_the_reference_value_in_float32():
    from ngp_harness.patches import scan_limit

    assert scan_limit(0.05) == float(np.float32(0.1)) == m.LIMIT and scan_limit(0.01) == float(np.float32(3 * 0.01))


# ---------------------------------------------------------------------------------------------------------------- the model's cases
@pytest.mark.parametrize("S,scan,cap", CASES)
def test_case_is_the_one_described(S, scan, cap):
    P = m.patch_problem(S, scan)
    d = m.describe(P, cap)
    assert P["n"] == 48 and P["frames32"].shape == (48, 3, 4) and P["cal32"].shape == (S,)
    from ngp_harness.patches import patch_grid_gap

    assert abs(S * P["grid_gap"] / (2.5 * patch_grid_gap(P["v"], P["cast_f"], 1.0)) - 1) < 1e-12 and 0 < P["cast_f"].shape[0] < P["f"].shape[0] / 2
    assert np.isnan(P["frames"][7]).any() and np.isfinite(np.delete(P["frames"], 7, axis=0)).all()
    assert (P["scan"] is not None) == scan and (scan or P["below"].sum() >= 3)
    assert d["undecided_candidates"] <= CANDIDATE_CAP and d["undecided_rays"] <= RAY_CAP, d
    codes = d["codes"]
    must = {m.ACCEPTED, m.FAR if scan else m.BELOW} | ({m.MISSED} if cap == 2000 else {m.NOT_NEEDED})
    assert all(codes[c] >= 3 for c in must) and codes[m.NAN_ORIGIN] == 1, d
    assert cap == 10 or codes[m.NOT_NEEDED] == 0
    REPORT.append(f"patch case S {S:2d} scan {scan!s:5s} cap {cap:4d}: undecided candidates {d['undecided_candidates']:.3f} rays {d['undecided_rays']:.4f} codes {codes}")


@pytest.mark.parametrize("S,scan,cap", CASES)
def test_the_model_passes_its_own_check(S, scan, cap, oracle):
    """The float64 answers rounded to float32 pass, within a quarter of the position tolerance -- which is fixed here, from the float32 brute
    force's own error on the case's rays (the tracer's rule), before any GPU output is looked at."""
    P = m.set_tolerances(m.patch_problem(S, scan), lambda v, f, o, d: oracle.raytrace(v, f, o, d)[:4])
    r = m.check_export(P, m.emulate(P, cap), cap)
    assert r["worst"] < 0.25 and (cap == 10 or r["rays"] > 5 * S * S)


def test_every_wrong_front_is_rejected():
    """Each deliberately wrong variant fails the check on at least one case, and the tail-lane one on every S^2 that is no multiple of 64 and none that is."""
    caught = {k: [] for k in m.MUTANTS}
    for S, scan, cap in CASES:
        P = m.patch_problem(S, scan)
        for k in m.MUTANTS:
            try:
                m.check_export(P, m.emulate(P, cap, mutate=k), cap)
            except AssertionError:
                caught[k].append((S, scan, cap))
    REPORT.append("wrong fronts rejected on: " + ", ".join(f"{k} {len(v)}/{len(CASES)}" for k, v in caught.items()))
    assert all(caught.values()), caught
    assert {c[0] for c in caught["tail_lanes"]} == {3, 12}, "9 and 144 pixels leave tail lanes, 64 does not"
    assert all(c[2] == 10 for c in caught["uncapped"])
