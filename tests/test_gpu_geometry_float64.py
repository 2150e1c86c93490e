"""The BVH tracer, the neighbour search and the curved projector against float64 (tests/geometry_float64.py; its check functions, its
tolerances and the cases are validated without a GPU in tests/test_geometry_float64_cpu.py).  No check here allows a share of failures:
the only exclusions are the references' `decided` flags, whose share is capped in the CPU test."""
import ctypes

import numpy as np
import pytest

import geometry_float64 as g

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

REPORT = []


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import nerftex_hip  # noqa: F401

    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if REPORT:
        print("\nworst |kernel - float64| / tolerance:\n" + "\n".join(REPORT))


@pytest.fixture(scope="module")
def trace32(oracle):
    return lambda v, f, o, d: oracle.raytrace(v, f, o, d)[:4]


def _fmt(r):
    return " ".join(f"{k} {v:.3f}" for k, v in r.items())


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def test_the_mesh_generator_is_the_projects():
    from ngp_harness.curved import star_flower_mesh

    for args in ((), (18, 36), (72, 144)):
        (v0, f0), (v1, f1) = star_flower_mesh(*args), g.star_flower_mesh(*args)
        assert v0.dtype == v1.dtype and f0.dtype == f1.dtype and np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) and np.array_equal(f0, f1)


# ------------------------------------------------------------------------------------------------------------------------- tracer
@pytest.mark.parametrize("name", g.TRACE_CASES)
def test_tracer_against_float64(dev, trace32, name):
    from RayTracer import RayTracer

    P = g.trace_problem(name, dev)
    if "tol_t" not in P:
        g.set_trace_tolerances(P, trace32(P["v"], P["f"], P["o"], P["d"]))
    rt = RayTracer(P["v"], P["f"])
    o, d = torch.from_numpy(P["o"]).to(dev), torch.from_numpy(P["d"]).to(dev)
    out = rt.trace(o, d)
    r = g.check_trace(P, *(t.cpu().numpy() for t in out))
    REPORT.append(f"tracer {name:6s} tol_t {float(np.min(P['tol_t'])):.3g} tol_n {P['tol_n']:.3g} (oracle error {P['oracle_err_t']:.3g}, {P['oracle_err_n']:.3g})  {_fmt(r)}")
    o2, d2 = o.clone(), d.clone()
    again = rt.trace(o2, d2, inplace=True)
    assert again[0].data_ptr() == o2.data_ptr() and again[1].data_ptr() == d2.data_ptr()
    for a, b, what in zip(out, again, ("positions", "normals", "depth", "face")):
        assert torch.equal(_bits(a), _bits(b)), f"{name}: in-place {what} differ"


# -------------------------------------------------------------------------------------------------------------- neighbour search
@pytest.mark.parametrize("name", g.KNN_CLOUDS)
def test_neighbour_search_against_float64(dev, name):
    from nerftex_hip import check, lib, ptr, stream

    P = g.knn_problem(name, dev)
    pts = np.ascontiguousarray(P["points"], dtype=np.float32)
    V, Q = pts.shape[0], P["queries"].shape[0]
    handle = ctypes.c_void_p()
    check(lib.nerftex_knn_create(pts.ctypes.data, V, ctypes.byref(handle)))
    try:
        xyz = torch.from_numpy(P["queries"]).to(dev)
        worst = {}
        for K in g.knn_ks(name, V):
            for n in (1, 255, 256, 257, Q):
                q = xyz[:n].contiguous()
                idx = torch.full((n, K), -7, dtype=torch.int32, device=dev)
                dis = torch.full((n, K), float("nan"), dtype=torch.float32, device=dev)
                check(lib.nerftex_knn_query(handle, ptr(q), n, K, ptr(idx), ptr(dis), stream()))
                r = g.check_knn(P, idx.cpu().numpy(), dis.cpu().numpy(), rows=slice(0, n))
                worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
        if V < 16:
            with pytest.raises(RuntimeError, match="1 <= K"):
                check(lib.nerftex_knn_query(handle, ptr(xyz), 1, V + 1, None, None, stream()))
    finally:
        lib.nerftex_knn_destroy(handle)
    REPORT.append(f"knn {name:10s} V {V:5d} K {g.knn_ks(name, V)}  (of 2^-21) {_fmt(worst)}")


# ---------------------------------------------------------------------------------------------------------------------- projector
@pytest.mark.parametrize("name", list(g.PROJECT_CASES))
def test_projector_against_float64(dev, trace32, name):
    from ngp_harness.curved import MeshProjector

    P = g.project_problem(name, dev)
    if "tol_t" not in P:
        R = P["rays"]
        g.set_project_tolerances(P, trace32(R["v"], R["f"], R["o"], R["d"]))
    proj = MeshProjector(P["v"], P["f"], h_threshold=P["h_threshold"], K=P["K"], vertex_normals=P["vn"], tbn=P["tbn"]).to(dev)
    assert torch.equal(proj.vertex_normals.cpu(), torch.from_numpy(P["vn"])) and torch.equal(proj.tbn.cpu(), torch.from_numpy(P["tbn"]))
    neighbours = (torch.from_numpy(P["idx"]).to(dev), torch.from_numpy(P["dis"]).to(dev))
    p_sur, sdf, mask, normal, tbn, face, z = proj.project_fused(torch.from_numpy(P["x"]).to(dev), multires=g.N_FREQS, neighbours=neighbours)
    r = g.check_project(P, *(t.cpu().numpy() for t in (p_sur, sdf, mask, normal, face, tbn, z)))
    REPORT.append(f"projector {name:7s} tol_normal {P['tol_normal']:.3g} (emulation error {P['emulation_err']:.3g}) tol_t {float(np.min(P['tol_t'])):.3g} "
                  f"(oracle error {P['rays']['oracle_err_t']:.3g}) trig bar {P['trig_bar']:.3g}  {_fmt(r)}")
