"""TEST INFRASTRUCTURE: a float64 statement of the `imported_type == 'shape'` branch of MeshFeatureField.forward (tools/map.py:693-700 over
MeshProjector.uvh / barycentric_mapping, :503-543, knn(use_dir_vec=False, weighting='DualD', nn_consis_check=True), :454-501, and
points_to_barycentric, :85-93), an fp32 emulation of the shape lookup kernel's normal, per-row tolerances and the check function of
tests/test_import_shape_cpu.py and tests/test_gpu_import_shape.py.  numpy and torch only; builds on geometry_float64 (the reference tracer,
the neighbour search, the tolerance rules of the projector) and planar_float64 (the bilinear read and the ladder).

What is compared with what
  normal    the DualD chain in float64 from the fp32 inputs and the fp32-ROUNDED neighbour distances; tolerance per row 4 x that row's
            |fp32 emulation - float64|, never below TOL_NORMAL_FLOOR (2^-20).
  sdf       (inner ? -d1 : d2) / scale - offset from the two reference traces; tolerance the projector's tol_t + tol_normal |d| (the
            row's own tol_normal), divided by the scale.
  uv        sum_k b_k uv_k rate, b = s / (s0 + s1 + s2 + 1e-5), s_i = |p_j x p_k|, p = corner - p_sur.  First order in the row's p_sur
            tolerance tol_p (per component; |dp| <= sqrt(3) tol_p): d(p_j x p_k) = dp x (p_k - p_j), so |ds_i| <= |dp| L_i with L_i the
            length of the edge opposite corner i, plus 8 u |p_j| |p_k| for the fp32 cross product and norm; S = sum s + 1e-5,
            |dS| <= sum |ds|; |db_i| <= (|ds_i| + b_i |dS|) / S;  |d uv| <= rate (sum_i |uv_i| |db_i| + 8 u sum_i b_i |uv_i|)
            (the quotient, the three products, the two sums and the rate), u = 2^-24.  Computed per row in float64.
  features  and the ladder: from the kernel's OWN fp32 (u, v, sdf) bits with planar_float64's bound; nothing is excluded.
  decided   the projector's rule (both traces decided, |d1 - d2| > 1e-4, a 1e-4 margin at the threshold -- on the scaled height, so 1e-4
            over the scale where that is larger), minus rows with some |cos_k| < 1e-3 (fp32 may decide the consistency test the other way),
            minus rows with 0 < sum w < 1e-2 (the division by sum w amplifies).  Rows with sum w == 0 EXACTLY (K == 1, every kept
            distance ties, the point on its nearest vertex) are decided: the reference's normal is NaN and both its traces miss; the kernel
            answers mask 0.  Rows both traces miss are decided: face -1, mask 0.  Faces and UVs are compared where the hit is unique.
"""
import numpy as np

import geometry_float64 as g
import planar_float64 as pf

U = 2.0 ** -24
COS_MARGIN = 1e-3
WSUM_MARGIN = 1e-2


# ------------------------------------------------------------------------------------------------------------------------ the normal
def _rows(idx, n_verts):
    idx = idx.astype(np.int64)
    return np.clip(np.where(idx < 0, idx + n_verts, idx), 0, n_verts - 1)


def normal_reference(x, idx, dis, verts, vnormals, mutate=None):
    """-> (normal [N,3] float64 (NaN where sum w == 0), cos [N,K], wsum [N]).  mutate: 'shepard', 'no_consistency', 'mean_dir'."""
    x, dis, verts, vn = (a.astype(np.float64) for a in (x, dis, verts, vnormals))
    row = _rows(idx, len(verts))
    n = vn[row]
    dvec = x[:, None] - verts[row]
    dvec = dvec / (np.linalg.norm(dvec, axis=-1, keepdims=True) + 1e-5)
    cos = (dvec * dvec[:, :1]).sum(-1)
    if mutate != "no_consistency":
        dis = np.where(cos > 0, dis, 1e5)
    if mutate == "mean_dir":  # use_dir_vec left on: the mean direction joins the candidates at distance 0.05
        w = 1 / (dis + 1e-7)
        mean_dir = (w[..., None] * dvec).sum(1)
        flip = (mean_dir * n.mean(1)).sum(-1) < 0
        mean_dir = np.where(flip[:, None], -mean_dir, mean_dir)
        mean_dir = mean_dir / (np.linalg.norm(mean_dir, axis=-1, keepdims=True) + 1e-5)
        n = np.concatenate([n, mean_dir[:, None]], 1)
        dis = np.concatenate([dis, np.full((len(x), 1), g.DIR_VEC_WDIST)], 1)
    if mutate == "shepard":
        w = 1 / (dis + 1e-7)
    else:
        dk, d1 = dis.max(-1, keepdims=True), dis.min(-1, keepdims=True)
        w = (dk - dis) / (dk - d1 + 1e-5) * (dk + d1) / (dk + dis)
    wsum = w.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = w / wsum[:, None]
        n = n / (np.linalg.norm(n, axis=-1, keepdims=True) + 1e-5)
        nrm = (n * w[..., None]).sum(1)
        nrm = nrm / (np.linalg.norm(nrm, axis=-1, keepdims=True) + 1e-5)
    return nrm, cos, wsum


def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normal_emulation(x, idx, dis, verts, vnormals):
    """the chain in fp32 in shape_lookup_kernel's operation order: plain products and sums, one neighbour after the other"""
    f4 = np.float32
    x, dis, verts, vn = (a.astype(f4) for a in (x, dis, verts, vnormals))
    N, K = idx.shape
    row = _rows(idx, len(verts))
    kept, dir0 = np.empty((N, K), f4), None
    for k in range(K):
        d = x - verts[row[:, k]]
        dl = np.sqrt(_dot32(d, d)) + f4(1e-5)
        dvec = d / dl[:, None]
        dir0 = dvec if k == 0 else dir0
        kept[:, k] = np.where(_dot32(dvec, dir0) > 0, dis[:, k], f4(1e5))
    dk, d1 = kept.max(-1), kept.min(-1)
    w = np.empty((N, K), f4)
    for k in range(K):
        w[:, k] = (dk - kept[:, k]) / (dk - d1 + f4(1e-5)) * (dk + d1) / (dk + kept[:, k])
    wsum = w[:, 0].copy()
    for k in range(1, K):
        wsum = wsum + w[:, k]
    nrm = None
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(K):
            n = vn[row[:, k]]
            nl = np.sqrt(_dot32(n, n)) + f4(1e-5)
            t = (n / nl[:, None]) * (w[:, k] / wsum)[:, None]
            nrm = t if k == 0 else nrm + t
        return nrm / (np.sqrt(_dot32(nrm, nrm)) + f4(1e-5))[:, None]


# ------------------------------------------------------------------------------------------------------------------------ meshes, problems
def quad_mesh():
    """two triangles over [-0.5, 0.5]^2 at z = 0 (4 vertices: a K above 4 is clamped by the wrapper)"""
    v = np.float32([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [-0.5, 0.5, 0.0], [0.5, 0.5, 0.0]])
    return v, np.asarray([[0, 1, 2], [1, 3, 2]], np.uint32)


def mesh_uvs(v, seed=5):
    """per-vertex UVs in [-1, 1]: an affine image of the two widest coordinates, perturbed, mapped by its global minimum and maximum"""
    rng = np.random.default_rng(seed + len(v))
    ext = v.max(0) - v.min(0)
    a, b = np.argsort(-ext)[:2]
    uv = np.stack([0.9 * v[:, a] + 0.2 * v[:, b], -0.3 * v[:, a] + 0.8 * v[:, b]], -1) + rng.uniform(-0.004, 0.004, (len(v), 2))
    uv = uv.astype(np.float32)
    return ((uv - uv.min()) / (uv.max() - uv.min()) * np.float32(2) - np.float32(1)).astype(np.float32)


def mesh_of(name):
    if name == "quad":
        v, f = quad_mesh()
    elif name == "height":
        v, f = g.height_field_mesh()
    else:
        v, f = g.star_flower_mesh(18, 36)
    return v, f, g.vertex_normals(v, f), mesh_uvs(v)


def sample_points(v, f, vn, N, rng, shell=0.08, far_share=0.0, on_vertex=False):
    """points within +-shell of the surface along the interpolated vertex normal; a share 30 away; optionally row 0 exactly on a vertex"""
    fi = f.astype(np.int64)
    pick, bary = rng.integers(0, len(f), N), rng.dirichlet([1, 1, 1], N)
    on = (v[fi[pick]].astype(np.float64) * bary[..., None]).sum(1)
    nn = (vn[fi[pick]].astype(np.float64) * bary[..., None]).sum(1)
    x = on + g._unit(nn) * rng.uniform(-shell, shell, (N, 1))
    n_far = int(round(far_share * N))
    if n_far:
        x[rng.choice(N, n_far, replace=False)] = g._unit(rng.normal(size=(n_far, 3))) * 30.0
    x = x.astype(np.float32)
    if on_vertex:
        x[0] = v[len(v) // 2]
    return np.ascontiguousarray(x)


# name: (mesh, N, K, h_threshold, scale, offset, rate, far share, map)
CASES = {
    "height_k5": ("height", 4099, 5, 0.05, 1.0, 0.0, 1.0, 0.0, (64, 48)),
    "height_scaled": ("height", 4099, 5, 0.05, 2.5, 0.01, 0.5, 0.0, (5, 4)),
    "height_far": ("height", 2051, 8, 20.0, 2.5, 0.0, 1.3, 0.1, (64, 48)),
    "star_k2": ("star", 4099, 2, 0.05, 1.0, 0.01, 1.3, 0.0, (5, 4)),
    "star_k8": ("star", 4099, 8, 0.05, 2.5, 0.0, 1.0, 0.0, (64, 48)),
    "star_k16": ("star", 2051, 16, 0.05, 1.0, 0.0, 0.5, 0.0, (1, 1)),
    "quad_k4": ("quad", 384, 4, 0.05, 1.0, 0.0, 1.0, 0.0, (5, 4)),
}
_cache = {}


def build_problem(name, mesh, x, K, h_threshold, scale, offset, rate, map_hw, device="cpu", neighbours=None):
    """the float64 statement for the points x: neighbours from the float64 search (distances rounded to fp32) unless given"""
    v, f, vn, uvs = mesh_of(mesh) if isinstance(mesh, str) else mesh
    K = min(K, len(v))
    if neighbours is None:
        idx, dist = g.knn_reference(v, x, K, device)
        idx, dis = np.ascontiguousarray(idx.astype(np.int32)), np.ascontiguousarray(dist.astype(np.float32))
    else:
        idx, dis = neighbours
    scale32, offset32, rate32 = np.float32(max(1e-5, scale)), np.float32(offset), np.float32(rate)
    P = dict(name=name, v=v, f=f, vn=vn, uvs=uvs, face_uv=np.ascontiguousarray(uvs[f.astype(np.int64)].reshape(-1, 6)), x=x, idx=idx, dis=dis, K=K,
             h_threshold=h_threshold, h_limit=float(np.float32(min(9.5, h_threshold))), scale=float(scale32), offset=float(offset32), rate=float(rate32),
             features=pf.seeded_map(*map_hw))
    P["normal"], P["cos"], P["wsum"] = normal_reference(x, idx, dis, v, vn)
    P["nan"] = P["wsum"] == 0.0
    emu = normal_emulation(x, idx, dis, v, vn)
    with np.errstate(invalid="ignore"):
        P["emulation_err"] = np.where(P["nan"], 0.0, np.abs(emu - P["normal"]).max(1))
    P["tol_normal"] = np.maximum(4 * P["emulation_err"], g.TOL_NORMAL_FLOOR)
    d32 = np.where(P["nan"][:, None], np.float32([0, 0, 1]), P["normal"]).astype(np.float32)  # (a NaN row's rays are placeholders: the row is answered apart)
    P["rays"] = dict(name=f"shape {name}", v=v, f=f, o=np.concatenate([x, x]), d=np.concatenate([d32, -d32]))
    P["rays"]["ref"] = g.trace_reference(v, f, P["rays"]["o"], P["rays"]["d"], device)
    return finish(P)


def problem(name, device="cpu"):
    if name not in _cache:
        mesh, N, K, h, scale, offset, rate, far, map_hw = CASES[name]
        v, f, vn, _ = mesh_of(mesh)
        rng = np.random.default_rng(sum(map(ord, name)) + 4000)
        x = sample_points(v, f, vn, N, rng, far_share=far, on_vertex=True)
        _cache[name] = build_problem(name, mesh, x, K, h, scale, offset, rate, map_hw, device)
    return _cache[name]


def barycentric_uv(P, p_sur, face, mutate=None):
    """-> (uv [N,2] float64 (times rate), the terms of its tolerance).  face -1 reads face 0."""
    v8, fi = P["v"].astype(np.float64), P["f"].astype(np.int64)
    f0 = np.where(face < 0, 0, face)
    tri = v8[fi[f0]]
    p = tri - p_sur[:, None]
    s = np.stack([np.linalg.norm(np.cross(p[:, 1], p[:, 2]), axis=-1), np.linalg.norm(np.cross(p[:, 2], p[:, 0]), axis=-1),
                  np.linalg.norm(np.cross(p[:, 0], p[:, 1]), axis=-1)], -1)
    S = s.sum(-1, keepdims=True) + (0.0 if mutate == "no_eps" else 1e-5)
    b = s / S
    uvk = P["face_uv"].astype(np.float64).reshape(-1, 3, 2)[f0]
    uv = (uvk * b[..., None]).sum(1) * P["rate"]
    if mutate == "swap_uv":
        uv = uv[:, ::-1]
    L = np.stack([np.linalg.norm(tri[:, 2] - tri[:, 1], axis=-1), np.linalg.norm(tri[:, 0] - tri[:, 2], axis=-1), np.linalg.norm(tri[:, 1] - tri[:, 0], axis=-1)], -1)
    pl = np.linalg.norm(p, axis=-1)
    pp = np.stack([pl[:, 1] * pl[:, 2], pl[:, 2] * pl[:, 0], pl[:, 0] * pl[:, 1]], -1)
    return uv, dict(L=L, pp=pp, S=S, b=b, uvk=uvk)


def finish(P):
    ref, N = P["rays"]["ref"], P["x"].shape[0]
    d1, d2, f1, f2 = ref["t_best"][:N], ref["t_best"][N:], ref["face"][:N], ref["face"][N:]
    inner = d1 < d2
    d = np.where(inner, d1, d2)
    P["d"] = d
    P["sdf"] = np.where(inner, -d1, d2) / P["scale"] - P["offset"]
    P["face"] = np.where(inner, f1, f2)
    P["p_sur"] = P["x"].astype(np.float64) + d[:, None] * np.where(inner[:, None], 1.0, -1.0) * P["rays"]["d"][:N].astype(np.float64)
    P["mask"] = (np.abs(P["sdf"]) < P["h_limit"]) & (P["face"] >= 0) & ~P["nan"]
    P["uv"], P["uv_terms"] = barycentric_uv(P, P["p_sur"], P["face"])
    both = ref["decided"][:N] & ref["decided"][N:]
    P["far"] = (f1 < 0) & (f2 < 0) & both & ~P["nan"]
    P["unique"] = np.where(inner, ref["second"][:N] - d1, ref["second"][N:] - d2) > g.TIE
    margin = max(1e-4, 1e-4 / P["scale"])
    with np.errstate(invalid="ignore"):
        shaky = (np.abs(P["cos"]) < COS_MARGIN).any(1) | ((P["wsum"] > 0) & (P["wsum"] < WSUM_MARGIN))
    P["decided"] = ((both & (np.abs(d1 - d2) > 1e-4) & (np.abs(np.abs(P["sdf"]) - P["h_limit"]) > margin)) | P["far"]) & ~shaky & ~P["nan"]
    return P


def set_tolerances(P, oracle_outputs):
    """tol_t: the tracer's rule on the case's own 2 N rays (4 x the fp32 brute force's worst error, floored); then the row's p_sur, sdf and uv bars"""
    g.set_trace_tolerances(P["rays"], oracle_outputs)
    N = P["x"].shape[0]
    tol = P["rays"]["tol_t"]
    P["tol_t"] = np.maximum(tol[:N], tol[N:])
    P["tol_p"] = P["tol_t"] + P["tol_normal"] * np.abs(P["d"])
    P["tol_sdf"] = P["tol_p"] / P["scale"]
    t = P["uv_terms"]
    dp = np.sqrt(3.0) * P["tol_p"][:, None]
    ds = dp * t["L"] + 8 * U * t["pp"]
    db = (ds + t["b"] * ds.sum(-1, keepdims=True)) / t["S"]
    P["tol_uv"] = P["rate"] * ((np.abs(t["uvk"]) * db[..., None]).sum(1) + 8 * U * (np.abs(t["uvk"]) * t["b"][..., None]).sum(1))
    return P


# ------------------------------------------------------------------------------------------------------------------------ emulation, mutants
MUTANTS = ("shepard", "no_consistency", "mean_dir", "no_face_test", "unscaled_mask", "times_scale", "no_eps", "swap_uv", "rate_on_height")


def embed_columns(P, u, v, sdf):
    """what a perfect kernel writes into xin from its own fp32 (u, v, sdf): float64 values narrowed to half"""
    value, _ = pf.lookup_reference(P["features"], u.astype(np.float32), v.astype(np.float32), sdf.astype(np.float32))
    xin = np.ones((len(u), 48), np.float16)
    xin[:, :41] = value.astype(np.float16)
    return xin


def emulate(P, trace32, mutate=None):
    """the kernel's outputs (p_uv, sdf, mask, normal, face, xin) from the fp32 normal emulation and an fp32 tracer
    `trace32(v, f, o, d) -> (pos, nrm, depth, face)`; mutate: a deliberately wrong lookup, see MUTANTS"""
    f4 = np.float32
    x, N = P["x"], P["x"].shape[0]
    if mutate in ("shepard", "no_consistency", "mean_dir"):
        nrm = normal_reference(x, P["idx"], P["dis"], P["v"], P["vn"], mutate)[0].astype(f4)
    else:
        nrm = normal_emulation(x, P["idx"], P["dis"], P["v"], P["vn"])
    bad = ~np.isfinite(nrm).all(1) | P["nan"]  # (a wrong normal is to be caught as a wrong normal, not through the rows that have none)
    nrm = np.where(bad[:, None], f4(0), nrm)
    rays_d = np.where(bad[:, None], f4([0, 0, 1]), nrm)
    out = trace32(P["v"], P["f"], np.concatenate([x, x]), np.concatenate([rays_d, -rays_d]))
    depth, hit = out[2], out[3]
    d1, d2, b1, b2 = depth[:N], depth[N:], hit[:N], hit[N:]
    inner = d1 < d2
    d = np.where(inner, d1, d2)
    raw = np.where(inner, -d1, d2).astype(f4)
    scale, offset, rate = f4(P["scale"]), f4(P["offset"]), f4(P["rate"])
    sdf = (raw * scale if mutate == "times_scale" else raw / scale) - offset
    if mutate == "rate_on_height":
        sdf = sdf * rate
    face = np.where(inner, b1, b2).astype(np.int64)
    tested = np.abs(raw if mutate == "unscaled_mask" else sdf) < f4(P["h_limit"])
    mask = tested if mutate == "no_face_test" else tested & (face >= 0)
    p_sur = g._fma(d[:, None], np.where(inner[:, None], rays_d, -rays_d), x)
    Q = dict(P, rate=float(rate))
    uv = barycentric_uv(Q, p_sur.astype(np.float64), face, mutate)[0].astype(f4)
    xin = embed_columns(P, uv[:, 0], uv[:, 1], sdf)
    # a row without a finite normal: the constants
    uv[bad], sdf[bad], mask[bad], face[bad] = 0, 0, False, -1
    xin[bad, :41] = 0
    return uv, sdf, mask, nrm, face, xin


def check(P, p_uv, sdf, mask, normal, face, xin=None):
    """Asserts the lookup's outputs; -> worst ratios to the tolerances.  xin None (a record without the embedding): everything but features and ladder."""
    p_uv, sdf, mask, normal, face = (np.asarray(a) for a in (p_uv, sdf, mask, normal, face))
    N, name = P["x"].shape[0], P["name"]
    sdf, mask = sdf.reshape(N), mask.reshape(N).astype(bool)
    assert p_uv.shape == (N, 2) and normal.shape == (N, 3) and face.shape == (N,)
    r = {}
    nan, ok = P["nan"], ~P["nan"]
    # rows without a finite normal: a defined answer
    assert not mask[nan].any() and not normal[nan].any() and not p_uv[nan].any() and not sdf[nan].any() and (face[nan] == -1).all(), f"{name}: a row whose normal is 0 / 0 answers mask 0 and the constants"
    err_n = np.abs(normal - np.where(nan[:, None], 0.0, P["normal"])).max(1)
    r["normal"] = float((err_n / P["tol_normal"])[ok].max(initial=0.0))
    assert r["normal"] <= 1.0, f"{name}: normal {r['normal']:.3g} of the tolerance at point {np.flatnonzero(ok)[(err_n / P['tol_normal'])[ok].argmax()]}"
    far = P["far"]
    dec = P["decided"] & ~far
    assert (face[far] == -1).all() and not mask[far].any(), f"{name}: a point both traces miss is face -1, masked out"
    want_far = np.float32(g.MAX_DIST) / np.float32(P["scale"]) - np.float32(P["offset"])
    assert (sdf[far] == want_far).all(), f"{name}: a point both traces miss has the height 10 / scale - offset"
    e = np.abs(sdf - P["sdf"]) / P["tol_sdf"]
    r["sdf"] = float(e[dec].max(initial=0.0))
    assert r["sdf"] <= 1.0, f"{name}: sdf {r['sdf']:.3g} of the tolerance at point {np.flatnonzero(dec)[e[dec].argmax()]}"
    assert np.array_equal(mask[dec], P["mask"][dec]), f"{name}: {(mask[dec] != P['mask'][dec]).sum()} mask bits differ"
    u = dec & P["unique"]
    assert np.array_equal(face[u], P["face"][u]), f"{name}: {(face[u] != P['face'][u]).sum()} faces differ where the hit is unique"
    assert ((face[dec] >= 0) & (face[dec] < len(P["f"]))).all()
    e = (np.abs(p_uv - P["uv"]) / P["tol_uv"]).max(1)
    r["uv"] = float(e[u].max(initial=0.0))
    assert r["uv"] <= 1.0, f"{name}: uv {r['uv']:.3g} of the tolerance at point {np.flatnonzero(u)[e[u].argmax()]}"
    if xin is None:
        return r
    xin = np.asarray(xin)
    assert xin.shape == (N, 48)
    assert not xin[nan, :41].any() and (xin[nan, 41:] == 1).all(), f"{name}: a row whose normal is 0 / 0 has an empty input row"
    # features and ladder from the kernel's own (u, v, sdf) bits: every finite-normal row, nothing excluded
    value, bound = pf.lookup_reference(P["features"], p_uv[:, 0].astype(np.float32), p_uv[:, 1].astype(np.float32), sdf.astype(np.float32))
    e = np.abs(xin[:, :41].astype(np.float64) - value) / bound
    r["embed"] = float(e[ok].max(initial=0.0))
    assert r["embed"] <= 1.0, f"{name}: features / ladder {r['embed']:.3g} of the bound"
    assert (xin[ok, 41:] == 1).all(), f"{name}: the padding columns are ones"
    return r


def describe(P):
    dec = P["decided"] | P["nan"]
    with np.errstate(invalid="ignore"):
        return dict(N=P["x"].shape[0], K=P["K"], excluded=float(1 - dec.mean()), nan=float(P["nan"].mean()), far=float(P["far"].mean()),
                    consistency=float((np.abs(P["cos"]) < COS_MARGIN).any(1).mean()), small_wsum=float(((P["wsum"] > 0) & (P["wsum"] < WSUM_MARGIN)).mean()),
                    masked_in=float(P["mask"].mean()))


def head(P, N):
    """the first N rows of a problem with its tolerances, as a problem of its own (the GPU test's batch sizes)"""
    rows = P["x"].shape[0]
    Q = {k: (v[:N] if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == rows and k not in ("v", "f", "vn", "uvs", "face_uv", "features") else v) for k, v in P.items()}
    Q["uv_terms"] = {k: v[:N] for k, v in P["uv_terms"].items()}
    Q["name"] = f"{P['name']}[:{N}]"
    return Q
