"""tests/geometry_float64.py checked on the CPU: every case is the one described (sizes, hit share, excluded share under its cap), the
float32 brute force (oracle.raytrace) and the float32 emulations pass the check functions with room to spare, and every deliberately
wrong tracer, neighbour search and projector is rejected by the same check functions on at least one case.  The tolerances are fixed
here -- from the oracle's and the emulation's own float32 error -- before any GPU output is looked at."""
import numpy as np
import pytest

import geometry_float64 as g

REPORT = []
TRACE_CAP, PROJECT_CAP = 0.01, 0.03


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        print("\n" + "\n".join(REPORT))


@pytest.fixture(scope="module")
def trace32(oracle):
    return lambda v, f, o, d: oracle.raytrace(v, f, o, d)[:4]


def _trace_case(name, trace32):
    P = g.trace_problem(name)
    if "tol_t" not in P:
        g.set_trace_tolerances(P, trace32(P["v"], P["f"], P["o"], P["d"]))
    return P


def _project_case(name, trace32):
    P = g.project_problem(name)
    if "tol_t" not in P:
        R = P["rays"]
        g.set_project_tolerances(P, trace32(R["v"], R["f"], R["o"], R["d"]))
    return P


def _fmt(r):
    return " ".join(f"{k} {v:.3f}" for k, v in r.items())


# ------------------------------------------------------------------------------------------------------------------------- tracer
@pytest.mark.parametrize("name", g.TRACE_CASES)
def test_tracer_case_is_the_one_described(name):
    P = g.trace_problem(name)
    s = g.describe_trace(P)
    want_n = {"A": int(name[1:] or 0) if name[0] == "A" else 0, "B": 2 * 4099, "C": 2051, "D": 1031, "E": 1031, "F": 2051, "G": 2048}[name[0]]
    want_f = {"A": 1224, "B": 1224, "C": 1152, "D": int(name[1:]) if name[0] == "D" else 0, "E": 203, "F": 1224, "G": 20448}[name[0]]
    assert (s["N"], s["F"]) == (want_n, want_f)
    assert s["excluded"] <= TRACE_CAP, f"{name}: {s['excluded']:.4f} of the rays are excluded"
    if s["N"] >= 100:
        lo_hit, lo_miss = g.TRACE_SHARES.get(name, (0.25, 0.05))
        assert s["hits"] >= lo_hit and 1 - s["hits"] >= lo_miss, s
    o, d = P["o"], P["d"]
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1, atol=1e-6)
    if name[0] == "A":
        assert P["ref"]["face"][0] >= 0, "the single ray of A1 is a hit"
    if name == "B":
        assert np.array_equal(o[:4099], o[4099:]) and np.array_equal(d[:4099], -d[4099:])
    if name == "C":
        vx, vz = set(P["v"][:, 0].tolist()), set(P["v"][:, 2].tolist())
        down, along = d[:, 1] == -1, d[:, 0] == 1
        assert down.sum() == 1025 and along.sum() == 1026 and all(x in vx for x in o[down, 0].tolist()) and all(z in vz for z in o[along, 2].tolist())
        assert (np.count_nonzero(d, axis=1) == 1).all()
        assert (P["v"][:, 1] == 0).sum() >= 63, "the plateau"
    if name == "E":
        f = P["f"]
        assert all(np.array_equal(f[:40], f[40 * k:40 * k + 40]) for k in range(1, 5))
        tri = P["v"][f[200:].astype(np.int64)].astype(np.float64)
        assert (np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) == 0).all()
        hit = P["ref"]["face"] >= 0
        assert (P["ref"]["second"][hit] == P["ref"]["t_best"][hit]).all(), "every hit is a tie among the copies"
    if name == "F":
        raw = P["ref"]["raw"]
        assert (np.isfinite(raw) & (raw > 10)).mean() > 0.05 and (raw < 10).mean() > 0.2, "closest hits on both sides of the limit"
    REPORT.append(f"tracer {name:6s} N {s['N']:5d} F {s['F']:5d} hits {s['hits']:.3f} excluded {s['excluded']:.4f}")


@pytest.mark.parametrize("name", g.TRACE_CASES)
def test_float32_brute_force_passes_check_trace(name, trace32):
    """oracle.raytrace within a quarter of tol_t (it defines tol_t: this pins the floor and the bookkeeping) and, through the same check,
    the float64 reference's own outputs rounded to float32."""
    P = _trace_case(name, trace32)
    r = g.check_trace(P, *trace32(P["v"], P["f"], P["o"], P["d"]))
    assert max(r["depth"], r["position"], r["face_t"]) <= 0.25 and r["normal"] <= 0.25, r
    g.check_trace(P, *g.outputs_from_reference(P, P["ref"]))
    REPORT.append(f"tracer {name:6s} oracle float32 error: depth/position {P['oracle_err_t']:.3g} normal {P['oracle_err_n']:.3g}  tol_t {float(np.min(P['tol_t'])):.3g} tol_n {P['tol_n']:.3g}  ratios {_fmt(r)}")


@pytest.mark.parametrize("mutant", g.TRACE_MUTANTS)
def test_check_trace_rejects_a_wrong_tracer(mutant, trace32):
    rejected = []
    for name in g.TRACE_CASES:
        P = _trace_case(name, trace32)
        ref = g.trace_reference(P["v"], P["f"], P["o"], P["d"], mutate=mutant)
        try:
            g.check_trace(P, *g.outputs_from_reference(P, ref))
        except AssertionError as e:
            rejected.append(f"{name}: {str(e)[:100]}")
    REPORT.append(f"tracer mutant {mutant:14s} rejected on {len(rejected)} of {len(g.TRACE_CASES)} cases; first {rejected[:1]}")
    assert rejected, f"{mutant} passes check_trace on every case"
    must = {"shrunk_box": "C", "no_limit": "F"}.get(mutant)
    assert must is None or any(r.startswith(must + ":") for r in rejected), f"{mutant} is what case {must} exists to catch"


# -------------------------------------------------------------------------------------------------------------- neighbour search
@pytest.mark.parametrize("name", g.KNN_CLOUDS)
def test_knn_cloud_is_the_one_described_and_float32_passes(name):
    P = g.knn_problem(name)
    pts, q = P["points"], P["queries"]
    V = {"sphere": 5000, "clusters": 3300, "one": 1, "sixteen": 16, "seventeen": 17, "identical": 100, "planar": 2000, "collinear": 500, "long": 5000}[name]
    assert pts.shape == (V, 3) and 550 <= len(q) <= 650
    lo, hi = pts.min(0), pts.max(0)
    _, cell, dims = g.grid_of(pts)
    ext0 = int((hi - lo == 0).sum())
    assert ext0 == {"identical": 3, "one": 3, "planar": 1, "collinear": 2}.get(name, 0) and int((dims == 1).sum()) >= ext0
    on = (q[:, None] == pts[None]).all(-1).any(1)
    assert on.sum() >= 100, "queries exactly on points"
    for ax in range(3):
        assert (q[:, ax] < lo[ax]).sum() >= 12 and (q[:, ax] > hi[ax]).sum() >= 12, "queries outside every face of the box"
    size = max(float((hi - lo).max()), 1e-2)
    assert (np.linalg.norm(q - (lo + hi) / 2, axis=1) > 29 * size).sum() >= 12
    if name == "long":
        assert dims[0] == 256 and cell > 5 * float(2 * np.sqrt(2 * (100 * 0.01 * 2) / V)), "the 256-cell cap binds"
        assert V / 256 > 15, "cells hold dozens of points"
    if name == "clusters":
        assert len(np.unique(pts, axis=0)) <= V - 250, "duplicates"
        assert ((P["ref_dist"][:, 0] > 1.0) & ((q > lo) & (q < hi)).all(1)).sum() <= 64, "at most 64 queries between the clusters"
    if name == "identical":
        assert (P["ref_dist"][on] == 0).all()
    if name in ("sphere", "planar", "long"):
        assert g.beyond_block(P, min(8, V), 1) > 0.15 and g.beyond_block(P, min(8, V), 3) > 0.1, "rings 2 and beyond 3 are ordinary here, not a few far queries"
    worst = {}
    for K in g.knn_ks(name, V):
        r = g.check_knn(P, *g.knn_float32(pts, q, K))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    assert worst["distance"] <= 0.5, "float32 arithmetic uses at most half of the 2^-21"
    REPORT.append(f"knn {name:10s} V {V:5d} queries {len(q)} cells {dims.tolist()} K {g.knn_ks(name, V)}  float32 brute force: {_fmt(worst)}")


@pytest.mark.parametrize("mutant", g.KNN_MUTANTS)
def test_check_knn_rejects_a_wrong_search(mutant):
    rejected = []
    for name in g.KNN_CLOUDS:
        P = g.knn_problem(name)
        K = min(8, len(P["points"]))
        try:
            g.check_knn(P, *g.knn_float32(P["points"], P["queries"], K, mutate=mutant))
        except AssertionError as e:
            rejected.append(f"{name}: {str(e)[:100]}")
    REPORT.append(f"knn mutant {mutant:10s} rejected on {len(rejected)} of {len(g.KNN_CLOUDS)} clouds; first {rejected[:1]}")
    assert rejected, f"{mutant} passes check_knn on every cloud"
    if mutant == "duplicate":
        assert any(r.startswith("identical:") for r in rejected), "all distances 0: only the distinctness check can tell"


# ---------------------------------------------------------------------------------------------------------------------- projector
@pytest.mark.parametrize("name", list(g.PROJECT_CASES))
def test_projector_case_is_the_one_described_and_the_emulation_passes(name, trace32):
    P = _project_case(name, trace32)
    N, K, h, pad, far_share = g.PROJECT_CASES[name]
    s = g.describe_project(P)
    assert P["x"].shape == (N, 3) and P["idx"].shape == (N, K) and P["idx"].dtype == np.int32 and P["dis"].dtype == np.float32
    assert s["excluded"] <= PROJECT_CAP, f"{name}: {s['excluded']:.4f} of the points are excluded"
    assert abs(s["far"] - far_share) < 0.002
    assert P["h_limit"] == (9.5 if h > 9.5 else float(np.float32(h)))
    if pad:
        assert (P["idx"][:, -2:] == -1).all() and (P["dis"][:, -2:] == 100).all() and (P["idx"][:, :-2] >= 0).all()
    if N >= 1000:
        assert 0.3 < s["inside"] < 0.7 and (0.3 < s["masked_in"] < 0.9 if h < 1 else s["masked_in"] >= 0.94)
    assert P["tol_normal"] <= 2e-6
    r = g.check_project(P, *g.emulate_project(P, trace32))
    assert max(r.values()) <= 0.5, r
    REPORT.append(f"projector {name:7s} N {N:5d} K {K:2d} excluded {s['excluded']:.4f} far {s['far']:.3f}  emulation error {P['emulation_err']:.3g} tol_normal {P['tol_normal']:.3g} "
                  f"oracle error {P['rays']['oracle_err_t']:.3g}  emulation ratios {_fmt(r)}")


@pytest.mark.parametrize("mutant", g.PROJECT_MUTANTS)
def test_check_project_rejects_a_wrong_projector(mutant, trace32):
    rejected = []
    for name in g.PROJECT_CASES:
        P = _project_case(name, trace32)
        try:
            g.check_project(P, *g.emulate_project(P, trace32, mutate=mutant))
        except AssertionError as e:
            rejected.append(f"{name}: {str(e)[:100]}")
    REPORT.append(f"projector mutant {mutant:12s} rejected on {len(rejected)} of {len(g.PROJECT_CASES)} cases; first {rejected[:1]}")
    assert rejected, f"{mutant} passes check_project on every case"
    if mutant == "clamp_pad":
        assert any(r.startswith("padded:") for r in rejected)
    if mutant == "partner":
        assert any(r.startswith("n31:") for r in rejected) and any(r.startswith("n33:") for r in rejected), "below and just above one workgroup"
