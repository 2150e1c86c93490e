"""Float64 references, problem generators and check functions for the geometry of the curved-field path: the BVH closest-hit tracer
(csrc/raytracer.hip), the neighbour search (csrc/knn.hip) and the curved projector (curved_project_kernel).

numpy and torch only: imported by tests/test_geometry_float64_cpu.py (no GPU, no libnerftex_hip.so) and by
tests/test_gpu_geometry_float64.py.  The brute forces run in torch on whatever device they are given, in chunks.

What is compared with what
  tracer     Moeller-Trumbore in float64 over ALL triangles, the reference's semantics (0 <= u <= 1, v >= 0, u + v <= 1, t >= 0; a
             closest hit at t >= 10 is a miss: depth 10, face -1, zero normal).  A ray is DECIDED unless float32 could legitimately
             answer otherwise: an edge / vertex hit in front of or at the answer, a grazing best hit, an answer at 0 or at the 10
             limit ("at 0" is read for every triangle: one hit within 1e-3 of the origin, on either side of it, is enough, since
             float32 may put it on the other side and so change the answer).  The generators keep the excluded share under 1 % (3 %
             for the projector); the CPU test asserts it.  On decided rays `check_trace` allows no share of failures.  Its two
             tolerances are not taken from the kernel: 4 x the worst error of the float32 brute force (oracle.raytrace) against
             float64 on the decided rays of the same case -- depth and position together for tol_t, the unit normal for tol_n.
  neighbours float64 distances from the float32 inputs, top K.  `check_knn` has no exclusions: ids in range and distinct, distances
             ascending, each reported distance the float64 distance of its id within 2^-21 relative, none beyond the true K-th.
  projector  tools/map.py:414-433, 454-501 in float64 with the neighbours given; the two traces are reference traces.
"""
import functools

import numpy as np
import torch

F8 = torch.float64
MAX_DIST = 10.0
EDGE = 1e-4      # barycentric margin below which a hit is an edge / vertex hit; also the depth window in front of the answer
GRAZE = 1e-3     # |cos| between ray and face normal below which the best hit is grazing
LIMIT = 1e-3     # distance of the answer to 0 or to MAX_DIST below which hit / miss is float32's to decide
TIE = 1e-4       # the second-closest hit must be this far behind for the face to be unique
KNN_RTOL = 2.0 ** -21
TOL_T_FLOOR = 2.0 ** -22
TOL_N_FLOOR = 2.0 ** -21
TOL_NORMAL_FLOOR = 2.0 ** -20
TRIG_FLOOR = 2.0 ** -22


# ------------------------------------------------------------------------------------------------------------------------ meshes
def star_flower_mesh(n_lat=72, n_lon=144, lobes=5, amp=0.18, radius=0.7):
    """ngp_harness.curved.star_flower_mesh, copied (that module loads the HIP library on import); the GPU test asserts equality bit for bit."""
    theta = np.linspace(0, np.pi, n_lat + 1)
    phi = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    T, P = np.meshgrid(theta, phi, indexing="ij")
    r = radius * (1 + amp * np.sin(T) ** 2 * np.cos(lobes * P))
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.cos(T), r * np.sin(T) * np.sin(P)], -1).reshape(-1, 3)
    faces = []
    for i in range(n_lat):
        for j in range(n_lon):
            a = i * n_lon + j
            b = i * n_lon + (j + 1) % n_lon
            c = (i + 1) * n_lon + j
            d = (i + 1) * n_lon + (j + 1) % n_lon
            if i > 0:
                faces.append((a, c, b))
            if i < n_lat - 1:
                faces.append((b, c, d))
    return v.astype(np.float32), np.asarray(faces, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def height_field_mesh(n=24, seed=11):
    """n x n cells over [-1, 1]^2 in x, z; vertices jittered by a quarter cell in x and z, heights in +-0.1.  Faces row by row, two per
    cell, so eight consecutive faces are four cells of one row.  Cells [8, 14) x [8, 16) are a plateau at y = 0 exactly: the boxes of
    its leaves have no thickness in y, where a slab test lives on its widening alone."""
    rng = np.random.default_rng(seed)
    h = 2.0 / n
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x = -1 + h * j + rng.uniform(-0.25, 0.25, i.shape) * h
    z = -1 + h * i + rng.uniform(-0.25, 0.25, i.shape) * h
    y = rng.uniform(-0.1, 0.1, i.shape)
    y[8:15, 8:17] = 0.0
    v = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    faces = []
    for a in range(n):
        for b in range(n):
            p, q, r, s = a * (n + 1) + b, a * (n + 1) + b + 1, (a + 1) * (n + 1) + b, (a + 1) * (n + 1) + b + 1
            faces += [(p, r, q), (q, r, s)]
    return v, np.asarray(faces, np.uint32)


def vertex_normals(v, f):
    """area-weighted vertex normals, float64 arithmetic, rounded to float32 (the table the projector is given)"""
    v8, f = v.astype(np.float64), f.astype(np.int64)
    fn = np.cross(v8[f[:, 1]] - v8[f[:, 0]], v8[f[:, 2]] - v8[f[:, 0]])
    vn = np.zeros_like(v8)
    for k in range(3):
        np.add.at(vn, f[:, k], fn)
    return (vn / (np.linalg.norm(vn, axis=1, keepdims=True) + 1e-12)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the reference trace
def _pairs(v, f, o, d, device, budget=1 << 22):
    """yields (rows, t, u, w, det) for chunks of rays against all triangles, float64 [R, F].  Every triple product is split into two
    matrix products ((o - a) . x = o . x - a . x): nothing of shape [R, F, 3] is ever held."""
    V = torch.as_tensor(v.astype(np.float64), device=device)
    fi = torch.as_tensor(f.astype(np.int64), device=device)
    a, e1, e2 = V[fi[:, 0]], V[fi[:, 1]] - V[fi[:, 0]], V[fi[:, 2]] - V[fi[:, 0]]
    n = torch.linalg.cross(e1, e2)
    na = (n * a).sum(-1)
    e1a, e2a = torch.linalg.cross(e1, a), torch.linalg.cross(e2, a)
    O, D = torch.as_tensor(o.astype(np.float64), device=device), torch.as_tensor(d.astype(np.float64), device=device)
    step = max(1, budget // max(1, f.shape[0]))
    for r0 in range(0, o.shape[0], step):
        oo, dd = O[r0:r0 + step], D[r0:r0 + step]
        od = torch.linalg.cross(oo, dd)
        det = dd @ n.T
        # q = (o - a) x d;  q . e = (o x d) . e - d . (e x a)
        u = -(od @ e2.T - dd @ e2a.T) / det
        w = (od @ e1.T - dd @ e1a.T) / det
        t = (na[None] - oo @ n.T) / det
        yield slice(r0, r0 + step), t, u, w, det, n


def trace_reference(v, f, o, d, device="cpu", mutate=None):
    """-> dict of numpy arrays per ray: t_best, face, margin, cos, second, decided (and raw: the closest hit's t before the 10 limit).
    mutate: a deliberately wrong variant (tests/test_geometry_float64_cpu.py), see TRACE_MUTANTS."""
    N, F = o.shape[0], f.shape[0]
    out = {k: np.zeros(N) for k in ("t_best", "margin", "cos", "second", "raw")}
    out["face"], out["decided"] = np.full(N, -1, np.int64), np.zeros(N, bool)
    inf = float("inf")
    if mutate == "shrunk_box":
        V = torch.as_tensor(v.astype(np.float64), device=device)
        tri = V[torch.as_tensor(f.astype(np.int64), device=device)]  # [F, 3, 3]
        grp = torch.arange(F, device=device) // 8
        lo = torch.full((int(grp.max()) + 1, 3), inf, dtype=F8, device=device).scatter_reduce(0, grp[:, None].expand(-1, 3), tri.amin(1), "amin")
        hi = torch.full((int(grp.max()) + 1, 3), -inf, dtype=F8, device=device).scatter_reduce(0, grp[:, None].expand(-1, 3), tri.amax(1), "amax")
        lo, hi = lo[grp] + 1e-5, hi[grp] - 1e-5
    for rows, t, u, w, det, n in _pairs(v, f, o, d, device):
        m = torch.minimum(torch.minimum(u, w), 1 - u - w)
        if mutate == "parallelogram":
            hit = (u >= 0) & (u <= 1) & (w >= 0) & (w <= 1) & (t >= 0)
        elif mutate == "negative_t":
            hit = (u >= 0) & (u <= 1) & (w >= 0) & (u + w <= 1)
        else:
            hit = (u >= 0) & (u <= 1) & (w >= 0) & (u + w <= 1) & (t >= 0)
        if mutate == "shrunk_box":
            O, D = torch.as_tensor(o[rows].astype(np.float64), device=device), torch.as_tensor(d[rows].astype(np.float64), device=device)
            for k in range(3):
                p = O[:, k, None] + t * D[:, k, None]
                hit &= (p >= lo[None, :, k]) & (p <= hi[None, :, k])
        th = torch.where(hit, t, torch.full_like(t, inf))
        if mutate == "drop_closest":
            r = torch.arange(rows.start, rows.start + t.shape[0], device=device)
            first = th.argmin(1)
            drop = (r % 2000 == 0)
            th[drop, first[drop]] = inf
        k2 = min(2, F)
        two, idx = torch.topk(th, k2, dim=1, largest=False)
        raw, face = two[:, 0], idx[:, 0]
        second = two[:, 1] if k2 == 2 else torch.full_like(raw, inf)
        limit = inf if mutate == "no_limit" else MAX_DIST
        is_hit = raw < limit
        t_best = torch.where(is_hit, raw, torch.full_like(raw, MAX_DIST))
        g = face[:, None]
        nl = torch.linalg.norm(n, dim=1)
        dl = torch.linalg.norm(torch.as_tensor(d[rows].astype(np.float64), device=device), dim=1)
        cos = (det.gather(1, g)[:, 0] / (nl[face] * dl)).abs()
        margin = m.gather(1, g)[:, 0]
        # undecided: an edge / vertex hit in front of or at the answer; a grazing best hit; an answer at 0 or at the limit (a hit
        # that float32 may see on the other side of t = 0 counts, whichever triangle it belongs to)
        edge = ((m.abs() < EDGE) & (t > -EDGE) & (t < t_best[:, None] + EDGE)).any(1)
        at_zero = ((m > -EDGE) & (t.abs() < LIMIT)).any(1)
        has = torch.isfinite(raw)
        at_limit = has & ((raw - MAX_DIST).abs() < LIMIT)
        graze = is_hit & (cos < GRAZE)
        decided = ~(edge | at_zero | at_limit | graze)
        put = lambda k, x: out[k].__setitem__(rows, x.cpu().numpy())  # noqa: E731
        put("t_best", t_best), put("raw", raw), put("second", second), put("decided", decided)
        put("face", torch.where(is_hit, face, torch.full_like(face, -1)))
        put("margin", torch.where(is_hit, margin, torch.zeros_like(margin))), put("cos", torch.where(is_hit, cos, torch.zeros_like(cos)))
    return out


TRACE_MUTANTS = ("drop_closest", "shrunk_box", "parallelogram", "negative_t", "no_limit")


def face_geometry(v, f, o, d, face):
    """the given face of every ray intersected in float64: (t, margin, unit normal); rows with face < 0 are nan"""
    v8, o8, d8 = v.astype(np.float64), o.astype(np.float64), d.astype(np.float64)
    tri = v8[f.astype(np.int64)[np.clip(face, 0, f.shape[0] - 1)]]
    a, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = np.cross(e1, e2)
    rov0 = o8 - a
    q = np.cross(rov0, d8)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / (d8 * n).sum(1)
        u, w, t = -inv * (q * e2).sum(1), inv * (q * e1).sum(1), -inv * (n * rov0).sum(1)
        unit = n / np.linalg.norm(n, axis=1, keepdims=True)
    bad = face < 0
    t, m = np.where(bad, np.nan, t), np.where(bad, np.nan, np.minimum(np.minimum(u, w), 1 - u - w))
    unit[bad] = np.nan
    return t, m, unit


def outputs_from_reference(P, ref):
    """(positions, normals, depth, face) in float32 from a reference record: what a perfect (or a mutated) tracer would return"""
    depth = ref["t_best"].astype(np.float32)
    face = ref["face"]
    _, _, unit = face_geometry(P["v"], P["f"], P["o"], P["d"], face)
    nrm = np.where((face >= 0)[:, None], unit, 0.0).astype(np.float32)
    pos = (P["o"].astype(np.float64) + ref["t_best"][:, None] * P["d"].astype(np.float64)).astype(np.float32)
    return pos, nrm, depth, face


def _floor_t(t):
    return TOL_T_FLOOR * np.maximum(1.0, np.abs(t))


def trace_errors(P, positions, normals, depth, face):
    """worst errors of a float32 tracer's outputs on the decided rays, for deriving the tolerances from the oracle: (depth and position,
    normal).  The position is held to o + depth d with the tracer's OWN depth, the normal to the float64 normal of its OWN face."""
    ref, dec = P["ref"], P["ref"]["decided"]
    hit = dec & (ref["face"] >= 0) & (face >= 0)
    e_t = np.abs(depth.astype(np.float64) - ref["t_best"])[dec].max(initial=0.0)
    want = P["o"].astype(np.float64) + depth.astype(np.float64)[:, None] * P["d"].astype(np.float64)
    e_p = np.abs(positions - want)[dec].max(initial=0.0)
    _, _, unit = face_geometry(P["v"], P["f"], P["o"], P["d"], face)
    e_n = np.abs(normals - unit)[hit].max(initial=0.0)
    return float(max(e_t, e_p)), float(e_n)


def set_trace_tolerances(P, oracle_outputs):
    """tol_t = 4 x the oracle's worst depth / position error on this case's decided rays, never below 2^-22 max(1, t);
    tol_n = 4 x its worst normal error, never below 2^-21."""
    e_t, e_n = trace_errors(P, *oracle_outputs)
    P["oracle_err_t"], P["oracle_err_n"] = e_t, e_n
    P["tol_t"] = np.maximum(4 * e_t, _floor_t(P["ref"]["t_best"]))
    P["tol_n"] = max(4 * e_n, TOL_N_FLOOR)
    return P


def check_trace(P, positions, normals, depth, face):
    """Asserts the outputs of a tracer on the decided rays of problem P (all of them: no share of failures); -> worst ratios to the tolerances."""
    positions, normals, depth, face = (np.asarray(x) for x in (positions, normals, depth, face))
    ref, dec, tol_t, tol_n = P["ref"], P["ref"]["decided"], P["tol_t"], P["tol_n"]
    N = P["o"].shape[0]
    assert positions.shape == (N, 3) and normals.shape == (N, 3) and depth.shape == (N,) and face.shape == (N,)
    want_hit = ref["face"] >= 0
    got_hit = face >= 0
    bad = dec & (want_hit != got_hit)
    assert not bad.any(), f"{P['name']}: hit / miss differs on {bad.sum()} decided rays, first {np.flatnonzero(bad)[:5]}, depth {depth[bad][:5]} want {ref['t_best'][bad][:5]}"
    miss = dec & ~want_hit
    assert (depth[miss] == np.float32(MAX_DIST)).all() and (face[miss] == -1).all() and not normals[miss].any(), f"{P['name']}: a miss is depth 10, face -1, zero normal"
    hit = dec & want_hit
    assert ((face[hit] >= 0) & (face[hit] < P["f"].shape[0])).all(), f"{P['name']}: face out of range"
    r = {}
    err = np.abs(depth.astype(np.float64) - ref["t_best"])
    r["depth"] = float((err / tol_t)[dec].max(initial=0.0))
    assert r["depth"] <= 1.0, f"{P['name']}: depth off by {err[dec].max():.3g} ({r['depth']:.3g} of the tolerance) at ray {np.flatnonzero(dec)[(err / tol_t)[dec].argmax()]}"
    t_f, m_f, unit = face_geometry(P["v"], P["f"], P["o"], P["d"], face)
    r["face_t"] = float((np.abs(t_f - ref["t_best"]) / tol_t)[hit].max(initial=0.0))
    assert r["face_t"] <= 1.0 and (m_f[hit] >= -EDGE).all(), f"{P['name']}: the reported face is not hit at the reported depth ({r['face_t']:.3g} of the tolerance, margin {m_f[hit].min(initial=0):.3g})"
    unique = hit & (ref["second"] - ref["t_best"] > TIE)
    assert np.array_equal(face[unique], ref["face"][unique]), f"{P['name']}: {(face[unique] != ref['face'][unique]).sum()} faces differ where the hit is unique"
    r["normal"] = float(np.abs(normals - unit)[hit].max(initial=0.0) / tol_n)
    assert r["normal"] <= 1.0, f"{P['name']}: normal {r['normal']:.3g} of the tolerance"
    want_pos = P["o"].astype(np.float64) + depth.astype(np.float64)[:, None] * P["d"].astype(np.float64)
    r["position"] = float((np.abs(positions - want_pos).max(1) / tol_t)[dec].max(initial=0.0))
    assert r["position"] <= 1.0, f"{P['name']}: position {r['position']:.3g} of the tolerance"
    return r


# --------------------------------------------------------------------------------------------------------------- tracer problems
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _shell(rng, N):
    """signed offsets within +-0.08 of the surface, none closer than 0.004: a point ON the surface has its answer at t = 0, which is
    float32's to decide"""
    return rng.uniform(0.004, 0.08, (N, 1)) * rng.choice([-1.0, 1.0], (N, 1))


def _aimed_rays(v, f, N, rng, origin_scale, jitter, inside=0.0):
    """rays towards jittered centroids; every third starts inside (origin scaled by `inside`) when inside > 0"""
    cent = v[f.astype(np.int64)].astype(np.float64).mean(1)
    target = cent[rng.integers(0, len(cent), N)] + rng.normal(size=(N, 3)) * jitter
    o = rng.uniform(-1, 1, (N, 3)) * origin_scale
    if inside:
        o[np.arange(N) % 3 == 0] *= inside
    d = _unit(target - o)
    rnd = np.arange(N) % 3 == 0
    if inside:
        d[rnd] = _unit(rng.normal(size=(int(rnd.sum()), 3)))
    return o.astype(np.float32), d.astype(np.float32)


def _height_rays(v, N, rng):
    """axis-parallel rays over the height field: half along -y from above with x copied from a vertex (z off it by 0.005 .. 0.03), half
    along +x with z copied from a vertex and y in +-0.3 -- a direction component of 0 and an origin on a node face: 0 * inf slabs"""
    n1 = N // 2
    pick = v[rng.integers(0, len(v), N)].astype(np.float64)
    o, d = np.zeros((N, 3)), np.zeros((N, 3))
    o[:n1, 0], o[:n1, 1] = pick[:n1, 0], rng.uniform(0.5, 3.0, n1)
    o[:n1, 2] = pick[:n1, 2] + rng.uniform(0.005, 0.03, n1) * rng.choice([-1.0, 1.0], n1)
    far = np.arange(n1) % 5 == 0  # beside the field: misses
    o[:n1][far, 2] += rng.choice([-1.0, 1.0], int(far.sum())) * 2.5
    d[:n1, 1] = -1.0
    o[n1:, 0], o[n1:, 1], o[n1:, 2] = rng.uniform(-3.0, -1.5, N - n1), rng.uniform(-0.3, 0.3, N - n1), pick[n1:, 2]
    d[n1:, 0] = 1.0
    return o.astype(np.float32), d.astype(np.float32)


TREE_SIZES = (1, 8, 9, 10, 17, 32, 33, 65)
A_SIZES = (1, 63, 64, 65, 4099)
TRACE_CASES = tuple(f"A{n}" for n in A_SIZES) + ("B", "C") + tuple(f"D{n}" for n in TREE_SIZES) + ("E", "F", "G")
# minimum share of hits and of misses among a case's rays (cases of fewer than 100 rays are too small to hold to a share)
TRACE_SHARES = {"F": (0.20, 0.20)}
_cache = {}


def trace_problem(name, device="cpu"):
    """the tracer case `name` with its float64 reference, built once and shared (treat as read-only)"""
    if ("trace", name) in _cache:
        return _cache[("trace", name)]
    rng = np.random.default_rng(sum(map(ord, name)) + 1000)
    if name[0] in "ABFG":
        v, f = star_flower_mesh(72, 144) if name == "G" else star_flower_mesh(18, 36)
    if name[0] == "A" or name == "G":
        N = 2048 if name == "G" else int(name[1:])
        o, d = _aimed_rays(v, f, N, rng, 1.5, 0.35, inside=0.2)
    elif name == "B":
        N, fi = 4099, f.astype(np.int64)
        pick = rng.integers(0, len(f), N)
        bary = rng.dirichlet([1, 1, 1], N)
        on = (v[fi[pick]].astype(np.float64) * bary[..., None]).sum(1)
        n = _unit((vertex_normals(v, f)[fi[pick]].astype(np.float64) * bary[..., None]).sum(1))
        x = on + n * _shell(rng, N)
        o, d = np.concatenate([x, x]).astype(np.float32), np.concatenate([n, -n]).astype(np.float32)
    elif name == "C":
        v, f = height_field_mesh()
        o, d = _height_rays(v, 2051, rng)
    elif name[0] == "D":
        v, f = height_field_mesh()
        f = f[np.sort(rng.choice(len(f), int(name[1:]), replace=False))]
        o, d = _aimed_rays(v, f, 1031, rng, 1.5, 0.03)
    elif name == "E":
        v, f = height_field_mesh()
        some = f[rng.choice(len(f), 40, replace=False)]
        a, b = some[0, 0], some[0, 1]
        f = np.concatenate([np.tile(some, (5, 1)), np.array([[a, a, a], [a, a, b], [a, b, b]], np.uint32)])
        o, d = _aimed_rays(v, some, 1031, rng, 1.5, 0.03)
    elif name == "F":
        v = v * np.float32(8)
        N = 2051
        o = _unit(rng.normal(size=(N, 3))) * rng.uniform(13.5, 17.5, (N, 1))
        d = _unit(_unit(rng.normal(size=(N, 3))) * rng.uniform(0, 5.5, (N, 1)) - o)
        o, d = o.astype(np.float32), d.astype(np.float32)
    P = dict(name=name, v=np.ascontiguousarray(v), f=np.ascontiguousarray(f), o=np.ascontiguousarray(o), d=np.ascontiguousarray(d))
    P["ref"] = trace_reference(P["v"], P["f"], P["o"], P["d"], device)
    _cache[("trace", name)] = P
    return P


def describe_trace(P):
    ref = P["ref"]
    return dict(N=P["o"].shape[0], F=P["f"].shape[0], hits=float((ref["face"] >= 0).mean()), excluded=float(1 - ref["decided"].mean()))


# ------------------------------------------------------------------------------------------------------------- neighbour search
def knn_reference(points, queries, K, device="cpu", chunk=2048):
    """float64 distances from the float32 inputs, K smallest ascending: (idx int64 [N,K], dist float64 [N,K])"""
    Pt, Q = torch.as_tensor(points.astype(np.float64), device=device), torch.as_tensor(queries.astype(np.float64), device=device)
    idx, dist = [], []
    for a in range(0, Q.shape[0], chunk):
        dd = torch.linalg.norm(Q[a:a + chunk, None] - Pt[None], dim=-1)  # the difference of two float32 is exact in float64 unless they are 2^29 apart
        dk, ik = torch.topk(dd, K, dim=1, largest=False, sorted=True)
        idx.append(ik), dist.append(dk)
    return torch.cat(idx).cpu().numpy(), torch.cat(dist).cpu().numpy()


def check_knn(P, idx, dist, K=None, rows=None):
    """Every query, no exclusions.  P holds points, queries and the reference's distances `ref_dist` [N, >= K]; rows: the queries that were run."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    K = idx.shape[1] if K is None else K
    q = P["queries"] if rows is None else P["queries"][rows]
    D_K = (P["ref_dist"] if rows is None else P["ref_dist"][rows])[:, K - 1]
    V = P["points"].shape[0]
    assert idx.shape == (q.shape[0], K) and dist.shape == idx.shape, (idx.shape, dist.shape)
    assert ((idx >= 0) & (idx < V)).all(), f"{P['name']} K={K}: ids outside [0, {V}): {idx[(idx < 0) | (idx >= V)][:5]}"
    s = np.sort(idx, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all(), f"{P['name']} K={K}: {int((s[:, 1:] == s[:, :-1]).any(1).sum())} rows repeat an id"
    assert (dist[:, 1:] >= dist[:, :-1]).all(), f"{P['name']} K={K}: distances do not ascend"
    true = np.linalg.norm(q.astype(np.float64)[:, None] - P["points"].astype(np.float64)[idx], axis=-1)
    err = np.abs(dist.astype(np.float64) - true)
    r = {"distance": float((err / np.maximum(KNN_RTOL * true, 1e-300)).max()) if (true > 0).any() else 0.0}
    assert (err <= KNN_RTOL * true).all(), f"{P['name']} K={K}: a reported distance is not its id's: worst {r['distance']:.3g} of the tolerance, {int((err > KNN_RTOL * true).sum())} entries"
    over = true - D_K[:, None] * (1 + KNN_RTOL)
    assert (over <= 0).all(), f"{P['name']} K={K}: {int((over > 0).any(1).sum())} rows hold a vertex beyond the true K-th distance, worst by {over.max():.3g}"
    with np.errstate(divide="ignore", invalid="ignore"):
        r["kth"] = float(np.nan_to_num((true.max(1) - D_K) / (KNN_RTOL * D_K), nan=0.0, posinf=0.0).max())
    return r


KNN_CLOUDS = ("sphere", "clusters", "one", "sixteen", "seventeen", "identical", "planar", "collinear", "long")
KNN_ALL_K = (1, 3, 4, 5, 8, 9, 16)


def knn_ks(name, V):
    return [k for k in (KNN_ALL_K if name in ("sphere", "clusters") else (1, 8, 16)) if k <= V]


def knn_problem(name, device="cpu"):
    """cloud `name` with ~600 queries (near points, exactly on points, outside each face of the box, at its corners, 30 box sizes away;
    for the clusters at most 64 midway between them) and the float64 distances of the 16 nearest"""
    if ("knn", name) in _cache:
        return _cache[("knn", name)]
    rng = np.random.default_rng(sum(map(ord, name)) + 2000)
    if name == "sphere":
        pts = _unit(rng.normal(size=(5000, 3)))
    elif name == "clusters":
        centres = np.array([[-5.0, -4.0, -3.0], [5.0, 3.0, -2.0], [0.5, 4.0, 5.0]])
        pts = np.concatenate([c + rng.normal(size=(1000, 3)) * 0.004 for c in centres])
        pts = np.concatenate([pts, pts[rng.integers(0, len(pts), 300)]])  # duplicates
    elif name in ("one", "sixteen", "seventeen"):
        pts = rng.uniform(-1, 1, ({"one": 1, "sixteen": 16, "seventeen": 17}[name], 3))
    elif name == "identical":
        pts = np.tile(np.array([[0.3, -0.2, 0.5]]), (100, 1))
    elif name == "planar":
        pts = rng.uniform(-1, 1, (2000, 3))
        pts[:, 1] = 0.25
    elif name == "collinear":
        pts = np.zeros((500, 3))
        pts[:, 0], pts[:, 1], pts[:, 2] = rng.uniform(-2, 2, 500), -0.5, 0.125
    elif name == "long":
        pts = rng.uniform(0, 1, (5000, 3)) * np.array([100.0, 0.01, 0.01]) + np.array([-50.0, 0.0, 0.0])
    pts = pts.astype(np.float32)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    size = max(float((hi - lo).max()), 1e-2)
    local = 0.04 if name == "clusters" else size  # (a cluster's own size: a query between the clusters walks many empty rings, 64 of them do)
    near = pts[rng.integers(0, len(pts), 300)] + rng.normal(size=(300, 3)) * local * np.array([1e-3, 1e-2, 5e-2])[rng.integers(0, 3, 300), None]
    on = pts[rng.integers(0, len(pts), 120)]
    mid = rng.uniform(lo, hi, (64, 3))  # anywhere in the box: for the clusters, the empty space between them
    faces = []
    for ax in range(3):
        for side in (0, 1):
            p = rng.uniform(lo, hi, (12, 3))
            p[:, ax] = (hi[ax] + rng.uniform(0.01, 0.7, 12) * size) if side else (lo[ax] - rng.uniform(0.01, 0.7, 12) * size)
            faces.append(p)
    corners = np.array([[(hi if (c >> k) & 1 else lo)[k] for k in range(3)] for c in range(8)])
    corners = np.concatenate([corners, corners + np.sign(corners - (lo + hi) / 2) * 0.3 * size])
    away = (lo + hi) / 2 + _unit(rng.normal(size=(12, 3))) * 30 * size
    q = np.concatenate([near, on, mid] + faces + [corners, away]).astype(np.float32)
    q = np.ascontiguousarray(q[rng.permutation(len(q))])
    P = dict(name=name, points=np.ascontiguousarray(pts), queries=q)
    _, P["ref_dist"] = knn_reference(pts, q, min(16, len(pts)), device)
    _cache[("knn", name)] = P
    return P


def grid_of(points):
    """the cell grid csrc/knn.hip builds on the host, restated: (lo, cell, dims) -- for the mutants that search it wrongly"""
    p = points.astype(np.float32)
    lo, hi = p.min(0), p.max(0)
    ex = (hi - lo).astype(np.float32)
    longest = np.float32(max(ex.max(), 1e-6))
    area = np.float32(2) * (ex[0] * ex[1] + ex[1] * ex[2] + ex[2] * ex[0])
    cell = np.float32(2) * np.sqrt(np.float32(max(area, longest * longest * np.float32(1e-3))) / np.float32(len(p)))
    cell = np.float32(max(cell, longest / np.float32(256)))
    dims = np.clip(np.floor(ex / cell).astype(np.int64) + 1, 1, 256)
    return lo, cell, dims


def beyond_block(P, K, r):
    """share of the queries whose true K-th neighbour lies farther than the block of cells [c - r, c + r]^3 reaches (the kernel's stop
    test, in float64): those cannot stop before ring r + 1"""
    lo, cell, dims = grid_of(P["points"])
    lo, cell, q = lo.astype(np.float64), float(cell), P["queries"].astype(np.float64)
    c = np.clip(np.floor((q - lo) / cell), 0, dims - 1)
    reach = np.full(len(q), np.inf)
    for d in range(3):
        below = np.where(c[:, d] - r > 0, q[:, d] - (lo[d] + (c[:, d] - r) * cell), np.inf)
        above = np.where(c[:, d] + r < dims[d] - 1, (lo[d] + (c[:, d] + r + 1) * cell) - q[:, d], np.inf)
        reach = np.minimum(reach, np.minimum(below, above))
    return float((P["ref_dist"][:, K - 1] > reach).mean())


def knn_float32(points, queries, K, mutate=None):
    """the search in float32 by brute force (the kernel's distance: differences, squares summed in float32, one square root), ties in
    index order; mutate: a deliberately wrong search, see KNN_MUTANTS.  -> (idx int32, dist float32); -1 / inf where nothing was found"""
    p, q = points.astype(np.float32), queries.astype(np.float32)
    lo, cell, dims = grid_of(p)
    cell_of = lambda x: np.clip(np.floor((x - lo) * (np.float32(1) / cell)), 0, dims - 1).astype(np.int64)  # noqa: E731
    cp, cq = cell_of(p), cell_of(q)
    df = q[:, None] - p[None]
    d2 = (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]
    if mutate == "one_block":
        d2 = np.where((np.abs(cq[:, None] - cp[None]) <= 1).all(-1), d2, np.inf)
    elif mutate == "skip_last":
        flat = (cp[:, 2] * dims[1] + cp[:, 1]) * dims[0] + cp[:, 0]
        order = np.argsort(flat, kind="stable")
        last = order[np.r_[flat[order][1:] != flat[order][:-1], True]]  # the last vertex of every cell's range
        d2[:, last] = np.inf
    idx = np.argsort(d2, axis=1, kind="stable")[:, :K]
    dist = np.sqrt(np.take_along_axis(d2, idx, 1)).astype(np.float32)
    idx = np.where(np.isfinite(dist), idx, -1).astype(np.int32)
    if mutate == "duplicate" and K > 1:
        idx[:, K - 1], dist[:, K - 1] = idx[:, K - 2], dist[:, K - 2]
    return idx, dist


KNN_MUTANTS = ("one_block", "skip_last", "duplicate")


# ---------------------------------------------------------------------------------------------------------------------- projector
DIR_VEC_WDIST = 0.05
N_FREQS = 12


def normal_reference(x, idx, dis, verts, vnormals, mutate=None):
    """knn() of tools/map.py:454-501 (weighting 'Shepard', use_dir_vec) in float64 from the float32 inputs; a -1 id is the last row"""
    x, dis, verts, vn = (a.astype(np.float64) for a in (x, dis, verts, vnormals))
    idx = idx.astype(np.int64)
    row = np.where(idx < 0, 0 if mutate == "clamp_pad" else idx + len(verts), idx)
    n = vn[row]                                          # [N, K, 3]
    dvec = x[:, None] - verts[row]
    dvec = dvec / (np.linalg.norm(dvec, axis=-1, keepdims=True) + 1e-5)
    w = 1 / (dis + 1e-7)
    mean_dir = (w[..., None] * dvec).sum(1)
    flip = (mean_dir * n.mean(1)).sum(-1) < 0
    mean_dir = np.where(flip[:, None], -mean_dir, mean_dir)
    mean_dir = mean_dir / (np.linalg.norm(mean_dir, axis=-1, keepdims=True) + 1e-5)
    if mutate != "no_mean_dir":
        n = np.concatenate([n, mean_dir[:, None]], 1)
        w = np.concatenate([w, np.full((len(x), 1), 1 / (max(DIR_VEC_WDIST, 1e-5) + 1e-7))], 1)
    w = w / w.sum(-1, keepdims=True)
    n = n / (np.linalg.norm(n, axis=-1, keepdims=True) + 1e-5)
    nrm = (n * w[..., None]).sum(1)
    return nrm / (np.linalg.norm(nrm, axis=-1, keepdims=True) + 1e-5)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)  # the product is exact in float64


def _dot32(a, b):
    return _fma(a[..., 2], b[..., 2], _fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def normal_emulation(x, idx, dis, verts, vnormals):
    """the same chain in float32 in curved_project_kernel's operation order (one neighbour after the other, fused multiply-adds where
    the kernel has them)"""
    f4 = np.float32
    x, dis, verts, vn = (a.astype(f4) for a in (x, dis, verts, vnormals))
    N, K = idx.shape
    mean_dir, nsum, acc, wsum = np.zeros((N, 3), f4), np.zeros((N, 3), f4), np.zeros((N, 3), f4), np.zeros(N, f4)
    for k in range(K):
        row = idx[:, k].astype(np.int64)
        row = np.clip(np.where(row < 0, row + len(verts), row), 0, len(verts) - 1)
        n, d = vn[row], x - verts[row]
        dl = np.sqrt(_dot32(d, d)) + f4(1e-5)
        w = f4(1) / (dis[:, k] + f4(1e-7))
        mean_dir = _fma(w[:, None], d / dl[:, None], mean_dir)
        nsum = nsum + n
        nl = np.sqrt(_dot32(n, n)) + f4(1e-5)
        acc = _fma(w[:, None], n / nl[:, None], acc)
        wsum = wsum + w
    mean_dir = np.where((_dot32(mean_dir, nsum) < 0)[:, None], -mean_dir, mean_dir)
    mean_dir = mean_dir / (np.sqrt(_dot32(mean_dir, mean_dir)) + f4(1e-5))[:, None]
    w = f4(1) / (np.maximum(f4(DIR_VEC_WDIST), f4(1e-5)) + f4(1e-7))
    nl = np.sqrt(_dot32(mean_dir, mean_dir)) + f4(1e-5)
    acc = _fma(np.full((N, 1), w, f4), mean_dir / nl[:, None], acc)
    wsum = wsum + w
    nrm = acc / wsum[:, None]
    return nrm / (np.sqrt(_dot32(nrm, nrm)) + f4(1e-5))[:, None]


def freq_reference(sdf32, n_freqs=N_FREQS):
    """float64 sin / cos of the float32 height times 2^k (an exact product): (arguments float32 [N, n], sin, cos)"""
    arg = sdf32.astype(np.float32)[:, None] * (2.0 ** np.arange(n_freqs)).astype(np.float32)[None]
    return arg, np.sin(arg.astype(np.float64)), np.cos(arg.astype(np.float64))


PROJECT_CASES = {  # name: (N, K, h_threshold, pad the last two neighbour columns with -1, share of points 30 away)
    "n1": (1, 8, 0.05, False, 0.0), "n31": (31, 8, 0.05, False, 0.0), "n32": (32, 8, 0.05, False, 0.0), "n33": (33, 8, 0.05, False, 0.0),
    "k8": (4099, 8, 0.05, False, 0.0), "k1": (4099, 1, 0.05, False, 0.0), "k16": (4099, 16, 0.05, False, 0.0),
    "h20": (4099, 8, 20.0, False, 0.0), "padded": (4099, 8, 0.05, True, 0.0), "far": (4099, 8, 20.0, False, 0.05),
}


def project_problem(name, device="cpu"):
    """projector case `name` on star_flower_mesh(18, 36): shell points at +-0.08, neighbours from the float64 search (distances rounded
    to float32), the float64 normal, the two reference traces along +-normal and everything project() derives from them"""
    if ("project", name) in _cache:
        return _cache[("project", name)]
    N, K, h_threshold, pad, far_share = PROJECT_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 3000)
    v, f = star_flower_mesh(18, 36)
    fi = f.astype(np.int64)
    vn = vertex_normals(v, f)
    tbn = rng.normal(size=(len(f), 3, 3)).astype(np.float32)
    pick, bary = rng.integers(0, len(f), N), rng.dirichlet([1, 1, 1], N)
    on = (v[fi[pick]].astype(np.float64) * bary[..., None]).sum(1)
    x = on + _unit(on) * _shell(rng, N)
    n_far = int(round(far_share * N))
    if n_far:
        x[rng.choice(N, n_far, replace=False)] = _unit(rng.normal(size=(n_far, 3))) * 30.0
    x = np.ascontiguousarray(x.astype(np.float32))
    idx, dist = knn_reference(v, x, K, device)
    idx, dis = idx.astype(np.int32), dist.astype(np.float32)
    if pad:
        idx[:, -2:], dis[:, -2:] = -1, 100.0
    P = dict(name=name, v=v, f=f, vn=vn, tbn=tbn, x=x, idx=np.ascontiguousarray(idx), dis=np.ascontiguousarray(dis), K=K, h_threshold=h_threshold,
             h_limit=float(np.float32(min(9.5, h_threshold))))
    P["normal"] = normal_reference(x, idx, dis, v, vn)
    emu = normal_emulation(x, idx, dis, v, vn)
    P["emulation_err"] = float(np.abs(emu - P["normal"]).max())
    P["tol_normal"] = max(4 * P["emulation_err"], TOL_NORMAL_FLOOR)
    # the reference traces run along the float64 normal rounded to float32 (2^-25, far inside tol_normal): the same rays then serve
    # the float32 brute force that sets tol_t
    d32 = P["normal"].astype(np.float32)
    P["rays"] = dict(name=f"project {name}", v=v, f=f, o=np.concatenate([x, x]), d=np.concatenate([d32, -d32]))
    P["rays"]["ref"] = trace_reference(v, f, P["rays"]["o"], P["rays"]["d"], device)
    finish_project(P)
    _cache[("project", name)] = P
    return P


def finish_project(P, mutate=None):
    ref, N = P["rays"]["ref"], P["x"].shape[0]
    d1, d2, f1, f2 = ref["t_best"][:N], ref["t_best"][N:], ref["face"][:N], ref["face"][N:]
    inner = d1 < d2
    P["d1"], P["d2"] = d1, d2
    P["sdf"] = np.where(inner, -d1, d2)
    P["face"] = np.where(inner, f1, f2)
    P["p_sur"] = P["x"].astype(np.float64) + np.where(inner, d1, d2)[:, None] * np.where(inner[:, None], 1.0, -1.0) * P["rays"]["d"][:N].astype(np.float64)
    P["mask"] = np.abs(P["sdf"]) < P["h_limit"]
    P["far"] = (f1 < 0) & (f2 < 0) & ref["decided"][:N] & ref["decided"][N:]
    P["unique"] = np.where(inner, ref["second"][:N] - d1, ref["second"][N:] - d2) > TIE
    P["decided"] = (ref["decided"][:N] & ref["decided"][N:] & (np.abs(d1 - d2) > 1e-4) & (np.abs(np.abs(P["sdf"]) - P["h_limit"]) > 1e-4)) | P["far"]
    return P


def set_project_tolerances(P, oracle_outputs):
    """tol_t of the projector case: the tracer's rule on the case's own 2 N rays"""
    set_trace_tolerances(P["rays"], oracle_outputs)
    N = P["x"].shape[0]
    tol = P["rays"]["tol_t"]
    P["tol_t"] = np.maximum(tol[:N], tol[N:])
    return P


def emulate_project(P, trace32, mutate=None):
    """what the kernel computes, from the float32 normal emulation and a float32 tracer `trace32(v, f, o, d) -> (pos, nrm, depth, face)`
    (the test passes oracle.raytrace): the kernel's eight outputs.  mutate: a deliberately wrong projector, see PROJECT_MUTANTS."""
    f4 = np.float32
    x, N = P["x"], P["x"].shape[0]
    if mutate in ("clamp_pad", "no_mean_dir"):
        nrm = normal_reference(x, P["idx"], P["dis"], P["v"], P["vn"], mutate).astype(f4)
    else:
        nrm = normal_emulation(x, P["idx"], P["dis"], P["v"], P["vn"])
    out = trace32(P["v"], P["f"], np.concatenate([x, x]), np.concatenate([nrm, -nrm]))
    depth, face = out[2], out[3]
    d1, d2, b1, b2 = depth[:N], depth[N:], face[:N], face[N:]
    if mutate == "partner":  # the -normal hit of the neighbouring point: a shuffle across the wrong pair
        sw = np.arange(N) ^ 1
        sw[sw >= N] = N - 1
        d2, b2 = d2[sw], b2[sw]
    inner = (d1 > d2) if mutate == "farther" else (d1 < d2)
    d = np.where(inner, d1, d2)
    direction = np.where(inner[:, None], nrm, -nrm)
    sdf = np.where(inner, -d1, d2).astype(f4)
    if mutate == "sign":
        sdf = -sdf
    p_sur = _fma(d[:, None], direction, x)
    fidx = np.where(inner, b1, b2).astype(np.int64)
    mask = np.abs(sdf) < f4(P["h_limit"])
    tbn_out = P["tbn"][np.where(fidx >= 0, fidx, 0)]
    arg, _, _ = freq_reference(sdf)
    z = np.empty((N, 1 + 2 * N_FREQS), f4)
    z[:, 0], z[:, 1::2], z[:, 2::2] = sdf, np.sin(arg), np.cos(arg)
    return p_sur, sdf, mask, nrm, fidx, tbn_out, z


PROJECT_MUTANTS = ("farther", "sign", "clamp_pad", "no_mean_dir", "partner")


def check_project(P, p_sur, sdf, mask, normal, face, tbn_out, z_embed):
    """Asserts the projector's outputs; -> worst ratios to the tolerances."""
    p_sur, sdf, mask, normal, face, tbn_out, z_embed = (np.asarray(a) for a in (p_sur, sdf, mask, normal, face, tbn_out, z_embed))
    N, name = P["x"].shape[0], P["name"]
    sdf, mask, tbn_out = sdf.reshape(N), mask.reshape(N).astype(bool), tbn_out.reshape(N, 3, 3)
    assert p_sur.shape == (N, 3) and normal.shape == (N, 3) and face.shape == (N,) and z_embed.shape == (N, 1 + 2 * N_FREQS)
    r = {}
    r["normal"] = float(np.abs(normal - P["normal"]).max() / P["tol_normal"])
    assert r["normal"] <= 1.0, f"{name}: normal {r['normal']:.3g} of the tolerance at point {np.abs(normal - P['normal']).max(1).argmax()}"
    far = P["far"]
    dec = P["decided"] & ~far
    assert (sdf[far] == np.float32(MAX_DIST)).all() and (face[far] == -1).all() and not mask[far].any(), f"{name}: a point both traces miss is sdf 10, face -1, masked out"
    tol = P["tol_t"] + P["tol_normal"] * np.abs(P["sdf"])
    r["sdf"] = float((np.abs(sdf - P["sdf"]) / tol)[dec].max(initial=0.0))
    assert r["sdf"] <= 1.0, f"{name}: sdf {r['sdf']:.3g} of the tolerance at point {np.flatnonzero(dec)[(np.abs(sdf - P['sdf']) / tol)[dec].argmax()]}"
    r["p_sur"] = float((np.abs(p_sur - P["p_sur"]).max(1) / tol)[dec].max(initial=0.0))
    assert r["p_sur"] <= 1.0, f"{name}: p_sur {r['p_sur']:.3g} of the tolerance"
    u = dec & P["unique"]
    assert np.array_equal(face[u], P["face"][u]), f"{name}: {(face[u] != P['face'][u]).sum()} faces differ where the hit is unique"
    assert ((face[dec] >= 0) & (face[dec] < len(P["f"]))).all()
    assert np.array_equal(mask[dec], P["mask"][dec]), f"{name}: {(mask[dec] != P['mask'][dec]).sum()} mask bits differ"
    assert np.array_equal(tbn_out[dec].view(np.uint32), P["tbn"][face[dec]].view(np.uint32)), f"{name}: tbn_out is not tbn[face]"
    assert np.array_equal(z_embed[:, 0].view(np.uint32), sdf.astype(np.float32).view(np.uint32)), f"{name}: z_embed[:, 0] is not sdf"
    arg, s8, c8 = freq_reference(sdf)
    P["trig_bar"] = bar = max(4 * max(np.abs(np.sin(arg) - s8).max(), np.abs(np.cos(arg) - c8).max()), TRIG_FLOOR)
    r["trig"] = float(max(np.abs(z_embed[:, 1::2] - s8).max(), np.abs(z_embed[:, 2::2] - c8).max()) / bar)
    assert r["trig"] <= 1.0, f"{name}: sin / cos {r['trig']:.3g} of the bar {bar:.3g}"
    return r


def describe_project(P):
    dec = P["decided"]
    return dict(N=P["x"].shape[0], K=P["K"], excluded=float(1 - dec.mean()), far=float(P["far"].mean()), inside=float((P["sdf"] < 0).mean()),
                masked_in=float(P["mask"].mean()), tol_normal=P["tol_normal"], emulation_err=P["emulation_err"])
