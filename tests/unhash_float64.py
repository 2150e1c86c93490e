"""TEST INFRASTRUCTURE: a float64 statement of the `imported_type == 'unhash'` branch of MeshFeatureField.forward (tools/map.py:708-714 over
knn() with its defaults, :454-501, barycentric_mapping, :503-528, and points_to_barycentric, :85-93), an fp32 emulation of the vertex lookup
kernel, per-row tolerances and the check function of tests/test_unhash_cpu.py and tests/test_gpu_unhash.py.  numpy and torch only; builds on
geometry_float64 (the reference tracer, the neighbour search, the projector's normal and its emulation), shape_float64 (the point sampler, the
two-face mesh) and planar_float64 (the ladder and the half-precision bound).

What is compared with what
  normal    the projector's chain (Shepard weights, use_dir_vec) in float64 over the field's OWN mesh from the fp32 inputs and the fp32-ROUNDED
            neighbour distances; tolerance per row 4 x that row's |fp32 emulation - float64|, never below 2^-20.
  sdf       (inner ? -d1 : d2) / scale - offset from the two reference traces over the FINE mesh; tolerance the projector's
            tol_p = tol_t + tol_normal |d| over the scale, plus 2 u (|raw / scale| + |offset|) for the division and the subtraction.
  bary      b = s / (s0 + s1 + s2 + 1e-5), s_i = |p_j x p_k|, p = corner - p_sur.  First order in the row's p_sur tolerance (per component;
            |dp| <= sqrt(3) tol_p): d(p_j x p_k) = dp x (p_k - p_j), so |ds_i| <= |dp| L_i with L_i the length of the edge opposite corner i, plus
            8 u |p_j| |p_k| for the fp32 cross product and norm; S = sum s + 1e-5, |dS| <= sum |ds|; |db_i| <= (|ds_i| + b_i |dS|) / S + 2 u b_i
            (the sum and the quotient), u = 2^-24.
  features  sum_i b_i f_i: |d| <= sum_i |f_i| |db_i| + 4 u sum_i b_i |f_i| (the three products and the two sums), then the narrowing to half:
            + 2^-11 (|value| + that bound) + 2^-25 (planar_float64._half_bound).  The ladder: from the kernel's OWN fp32 sdf bits with
            planar_float64's bound, every row.
  decided   both traces decided by the tracer's rule (no edge or vertex hit in front of or at the answer -- a subdivided mesh has many edges, and
            the rule lumps a hit on the answer's own edge, across which sdf and features are continuous, with one on a silhouette edge, across
            which they are not: both are excluded from every comparison, and the excluded share stays under the cap all the same --, no grazing
            hit, no answer at 0 or at the 10 limit) and |d1 - d2| > 1e-4; the mask bit wants a 1e-4 margin at the threshold as well (on the
            scaled height: 1e-4 over the scale where that is larger), so a row right at the threshold still has its height compared.  Rows both
            traces miss are decided: face -1, mask 0, sdf exactly 10 / scale - offset.  sdf, barycentrics and features are compared on every
            decided row; the face id where, beyond that, the runner-up hit lies 1e-4 behind.  Every row, decided or not, must come out finite.
"""
import numpy as np

import geometry_float64 as g
import planar_float64 as pf
import shape_float64 as sf

U = 2.0 ** -24
N_FEATURES = 16


def subdivide_midpoint(v, f):
    from ngp_harness.subdivide import subdivide_midpoint as sub  # (numpy only: no library is loaded)

    return sub(v, f)


# ------------------------------------------------------------------------------------------------------------------------ meshes, problems
def seeded_rows(n_vertices, seed=23):
    return np.random.default_rng(seed + n_vertices).uniform(-0.5, 0.5, (n_vertices, N_FEATURES)).astype(np.float32)


_meshes = {}


def mesh_of(name):
    """-> (v, f, vn) of the field's own mesh, (fine vertices fp32, fine faces int64): 'star' = star_flower_mesh(18, 36) (its pole vertices are
    duplicated n_lon times) and ONE midpoint subdivision of it; 'quad' = two faces, the fine mesh the same two (the tracer pads it to 10 faces)."""
    if name not in _meshes:
        if name == "quad":
            v, f = sf.quad_mesh()
            fine = (v.copy(), f.astype(np.int64))
        else:
            v, f = g.star_flower_mesh(18, 36)
            fv, ff = subdivide_midpoint(v, f)
            fine = (np.ascontiguousarray(fv.astype(np.float32)), ff)
        _meshes[name] = (v, f, g.vertex_normals(v, f)), fine
    return _meshes[name]


# name: (mesh, N, h_threshold, scale, offset, far share, row 0 on a vertex, rows at the mask threshold)
CASES = {
    "star_n1": ("star", 1, 0.0625, 1.0, 0.0, 0.0, False, 0),
    "star_n127": ("star", 127, 0.0625, 1.0, 0.0, 0.0, True, 0),
    "star_n512": ("star", 512, 0.0625, 1.0, 0.0, 0.05, True, 4),
    "star_scaled": ("star", 512, 0.0625, 2.5, 0.01, 0.0, True, 4),
    "star_far": ("star", 512, 20.0, 2.5, 0.0, 0.1, False, 0),
    "quad": ("quad", 127, 0.0625, 1.0, 0.0, 0.05, True, 0),
}
_cache = {}


def build_problem(name, coarse, fine, features, x, h_threshold, scale, offset, device="cpu", neighbours=None):
    """the float64 statement for the points x: neighbours over the field's own mesh from the float64 search (distances rounded to fp32) unless given"""
    v, f, vn = coarse
    fv, ff = fine
    K = min(8, len(v))
    if neighbours is None:
        idx, dist = g.knn_reference(v, x, K, device)
        idx, dis = np.ascontiguousarray(idx.astype(np.int32)), np.ascontiguousarray(dist.astype(np.float32))
    else:
        idx, dis = neighbours
    P = dict(name=name, v=v, f=f, vn=vn, fv=fv, ff=np.asarray(ff, np.int64), features=features, x=x, idx=idx, dis=dis, K=K, h_threshold=h_threshold,
             h_limit=float(np.float32(min(9.5, h_threshold))), scale=float(np.float32(max(1e-5, scale))), offset=float(np.float32(offset)))
    P["normal"] = g.normal_reference(x, idx, dis, v, vn)
    emu = g.normal_emulation(x, idx, dis, v, vn)
    P["emulation_err"] = np.abs(emu - P["normal"]).max(1)
    P["tol_normal"] = np.maximum(4 * P["emulation_err"], g.TOL_NORMAL_FLOOR)
    d32 = P["normal"].astype(np.float32)
    P["rays"] = dict(name=f"unhash {name}", v=fv, f=P["ff"].astype(np.uint32), o=np.concatenate([x, x]), d=np.concatenate([d32, -d32]))
    P["rays"]["ref"] = g.trace_reference(fv, P["rays"]["f"], P["rays"]["o"], P["rays"]["d"], device)
    return finish(P)


def problem(name, device="cpu"):
    if name not in _cache:
        mesh, N, h, scale, offset, far, on_vertex, at_threshold = CASES[name]
        coarse, fine = mesh_of(mesh)
        v, f, vn = coarse
        rng = np.random.default_rng(sum(map(ord, name)) + 5000)
        x = sf.sample_points(v, f, vn, N, rng, shell=0.08, far_share=far, on_vertex=on_vertex)
        if at_threshold:  # rows whose height is the threshold itself, as nearly as fp32 positions give it: a vertex pushed out along its own normal
            rows = 1 + np.arange(at_threshold)
            pick = rng.integers(0, len(v), at_threshold)
            side = np.where(np.arange(at_threshold) % 2 == 0, 1.0, -1.0)[:, None]
            x[rows] = (v[pick].astype(np.float64) + side * g._unit(vn[pick].astype(np.float64)) * (min(9.5, h) + offset) * scale).astype(np.float32)
            for _ in range(4):  # ... then moved along the float64 normal by what the float64 height still lacks
                Q = build_problem("threshold", coarse, fine, seeded_rows(len(fine[0])), np.ascontiguousarray(x[rows]), h, scale, offset, device)
                lacks = (np.abs(Q["sdf"]) - Q["h_limit"]) * Q["scale"]
                x[rows] = (x[rows].astype(np.float64) - (np.sign(Q["sdf"]) * lacks)[:, None] * Q["normal"]).astype(np.float32)
        _cache[name] = build_problem(name, coarse, fine, seeded_rows(len(fine[0])), np.ascontiguousarray(x), h, scale, offset, device)
    return _cache[name]


def interpolate(P, p_sur, face, mutate=None):
    """-> (b [N,3], features [N,16] float64, the terms of their tolerances).  face -1 reads face 0."""
    v8 = P["fv"].astype(np.float64)
    f0 = np.where(face < 0, 0, face)
    corners = P["ff"][f0]
    tri = v8[corners]
    p = tri - p_sur[:, None]
    s = np.stack([np.linalg.norm(np.cross(p[:, 1], p[:, 2]), axis=-1), np.linalg.norm(np.cross(p[:, 2], p[:, 0]), axis=-1),
                  np.linalg.norm(np.cross(p[:, 0], p[:, 1]), axis=-1)], -1)
    S = s.sum(-1, keepdims=True) + 1e-5
    b = s / S
    if mutate == "bary_order":
        b = b[:, [1, 2, 0]]
    rows = P["features"].astype(np.float64)[corners[:, [2, 0, 1]] if mutate == "wrong_corner" else corners]  # [N, 3, 16]
    value = (rows * b[..., None]).sum(1)
    L = np.stack([np.linalg.norm(tri[:, 2] - tri[:, 1], axis=-1), np.linalg.norm(tri[:, 0] - tri[:, 2], axis=-1), np.linalg.norm(tri[:, 1] - tri[:, 0], axis=-1)], -1)
    pl = np.linalg.norm(p, axis=-1)
    pp = np.stack([pl[:, 1] * pl[:, 2], pl[:, 2] * pl[:, 0], pl[:, 0] * pl[:, 1]], -1)
    return b, value, dict(L=L, pp=pp, S=S, b=b, rows=rows)


def finish(P):
    ref, N = P["rays"]["ref"], P["x"].shape[0]
    d1, d2, f1, f2 = ref["t_best"][:N], ref["t_best"][N:], ref["face"][:N], ref["face"][N:]
    inner = d1 < d2
    d = np.where(inner, d1, d2)
    P["d"] = d
    P["raw"] = np.where(inner, -d1, d2)
    P["sdf"] = P["raw"] / P["scale"] - P["offset"]
    P["face"] = np.where(inner, f1, f2)
    P["p_sur"] = P["x"].astype(np.float64) + d[:, None] * np.where(inner[:, None], 1.0, -1.0) * P["rays"]["d"][:N].astype(np.float64)
    P["mask"] = (np.abs(P["sdf"]) < P["h_limit"]) & (P["face"] >= 0)
    P["bary"], P["value"], P["terms"] = interpolate(P, P["p_sur"], P["face"])
    both = ref["decided"][:N] & ref["decided"][N:]
    P["far"] = (f1 < 0) & (f2 < 0) & both
    P["unique"] = np.where(inner, ref["second"][:N] - d1, ref["second"][N:] - d2) > g.TIE
    margin = max(1e-4, 1e-4 / P["scale"])
    P["decided"] = (both & (np.abs(d1 - d2) > 1e-4)) | P["far"]  # sdf, barycentrics, features, face
    P["decided_mask"] = P["decided"] & ((np.abs(np.abs(P["sdf"]) - P["h_limit"]) > margin) | P["far"])  # ... and the mask bit
    return P


def set_tolerances(P, oracle_outputs):
    """tol_t: the tracer's rule on the case's own 2 N rays over the fine mesh (4 x the fp32 brute force's worst error, floored); then the row's p_sur,
    sdf, barycentric and feature bars (the module docstring's derivation)"""
    g.set_trace_tolerances(P["rays"], oracle_outputs)
    N = P["x"].shape[0]
    tol = P["rays"]["tol_t"]
    P["tol_t"] = np.maximum(tol[:N], tol[N:])
    P["tol_p"] = P["tol_t"] + P["tol_normal"] * np.abs(P["d"])
    P["tol_sdf"] = P["tol_p"] / P["scale"] + 2 * U * (np.abs(P["raw"] / P["scale"]) + abs(P["offset"]))
    t = P["terms"]
    dp = np.sqrt(3.0) * P["tol_p"][:, None]
    ds = dp * t["L"] + 8 * U * t["pp"]
    P["tol_bary"] = db = (ds + t["b"] * ds.sum(-1, keepdims=True)) / t["S"] + 2 * U * t["b"]
    fp32 = (np.abs(t["rows"]) * db[..., None]).sum(1) + 4 * U * (np.abs(t["rows"]) * t["b"][..., None]).sum(1)
    P["tol_feature"] = pf._half_bound(P["value"], fp32)
    return P


# ------------------------------------------------------------------------------------------------------------------------ emulation, mutants
MUTANTS = ("bary_order", "wrong_corner", "fine_normals", "offset_first", "no_face_rule", "times_scale", "unscaled_mask")


def _cross32(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1)


def _norm32(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def emulate(P, trace32, mutate=None):
    """the kernel's outputs (sdf, mask, normal, face, bary, xin) in fp32 in vertex_lookup_kernel's operation order, over an fp32 tracer
    `trace32(v, f, o, d) -> (pos, nrm, depth, face)`; mutate: a deliberately wrong lookup, see MUTANTS"""
    f4 = np.float32
    x, N = P["x"], P["x"].shape[0]
    if mutate == "fine_normals":  # the fine mesh's own vertices and normals where the field's own belong
        fvn = g.vertex_normals(P["fv"], P["ff"])
        idx, dist = g.knn_reference(P["fv"], x, min(8, len(P["fv"])))
        nrm = g.normal_emulation(x, idx.astype(np.int32), dist.astype(f4), P["fv"], fvn)
    else:
        nrm = g.normal_emulation(x, P["idx"], P["dis"], P["v"], P["vn"])
    out = trace32(P["fv"], P["rays"]["f"], np.concatenate([x, x]), np.concatenate([nrm, -nrm]))
    depth, hit = out[2], out[3]
    d1, d2, b1, b2 = depth[:N], depth[N:], hit[:N], hit[N:]
    inner = d1 < d2
    d = np.where(inner, d1, d2)
    raw = np.where(inner, -d1, d2).astype(f4)
    scale, offset = f4(P["scale"]), f4(P["offset"])
    if mutate == "offset_first":
        sdf = (raw - offset) / scale
    elif mutate == "times_scale":
        sdf = raw * scale - offset
    else:
        sdf = raw / scale - offset
    face = np.where(inner, b1, b2).astype(np.int64)
    tested = np.abs(raw if mutate == "unscaled_mask" else sdf) < f4(P["h_limit"])
    mask = tested if mutate == "no_face_rule" else tested & (face >= 0)
    p_sur = g._fma(d[:, None], np.where(inner[:, None], nrm, -nrm), x)
    corners = P["ff"][np.where(face < 0, 0, face)]
    tri = P["fv"][corners]
    p0, p1, p2 = tri[:, 0] - p_sur, tri[:, 1] - p_sur, tri[:, 2] - p_sur
    s0, s1, s2 = _norm32(_cross32(p1, p2)), _norm32(_cross32(p2, p0)), _norm32(_cross32(p0, p1))
    den = ((s0 + s1) + s2) + f4(1e-5)
    b = np.stack([s0 / den, s1 / den, s2 / den], -1)
    if mutate == "bary_order":
        b = b[:, [1, 2, 0]]
    rows = P["features"][corners[:, [2, 0, 1]] if mutate == "wrong_corner" else corners]
    feat = (rows[:, 0] * b[:, 0, None] + rows[:, 1] * b[:, 1, None]) + rows[:, 2] * b[:, 2, None]
    assert feat.dtype == f4 and b.dtype == f4 and sdf.dtype == f4
    xin = np.ones((N, 48), np.float16)
    xin[:, :16] = feat.astype(np.float16)
    xin[:, 16:41] = pf.ladder(sdf)[0].astype(np.float16)
    return sdf, mask, nrm, face, b, xin


def check(P, sdf, mask, normal, face, bary=None, xin=None):
    """Asserts the lookup's outputs; -> worst ratios to the tolerances.  bary None, xin None: a record without them."""
    sdf, mask, normal, face = (np.asarray(a) for a in (sdf, mask, normal, face))
    N, name = P["x"].shape[0], P["name"]
    sdf, mask = sdf.reshape(N), mask.reshape(N).astype(bool)
    assert normal.shape == (N, 3) and face.shape == (N,)
    assert np.isfinite(sdf).all() and np.isfinite(normal).all(), f"{name}: every row comes out finite"
    r = {}
    e = np.abs(normal - P["normal"]).max(1) / P["tol_normal"]
    r["normal"] = float(e.max(initial=0.0))
    assert r["normal"] <= 1.0, f"{name}: normal {r['normal']:.3g} of the tolerance at point {e.argmax()}"
    far = P["far"]
    dec = P["decided"] & ~far
    assert (face[far] == -1).all() and not mask[far].any(), f"{name}: a point both traces miss is face -1, masked out"
    want_far = np.float32(g.MAX_DIST) / np.float32(P["scale"]) - np.float32(P["offset"])
    assert (sdf[far] == want_far).all(), f"{name}: a point both traces miss has the height 10 / scale - offset"
    e = np.abs(sdf - P["sdf"]) / P["tol_sdf"]
    r["sdf"] = float(e[dec].max(initial=0.0))
    assert r["sdf"] <= 1.0, f"{name}: sdf {r['sdf']:.3g} of the tolerance at point {np.flatnonzero(dec)[e[dec].argmax()]}"
    dm = P["decided_mask"] & ~far
    assert np.array_equal(mask[dm], P["mask"][dm]), f"{name}: {(mask[dm] != P['mask'][dm]).sum()} mask bits differ"
    u = dec & P["unique"]
    assert np.array_equal(face[u], P["face"][u]), f"{name}: {(face[u] != P['face'][u]).sum()} faces differ where the hit is unique"
    assert ((face[dec] >= 0) & (face[dec] < len(P["ff"]))).all()
    if bary is not None:
        bary = np.asarray(bary)
        assert bary.shape == (N, 3) and np.isfinite(bary).all()
        e = (np.abs(bary - P["bary"]) / P["tol_bary"]).max(1)
        r["bary"] = float(e[dec].max(initial=0.0))
        assert r["bary"] <= 1.0, f"{name}: barycentrics {r['bary']:.3g} of the tolerance at point {np.flatnonzero(dec)[e[dec].argmax()]}"
    if xin is None:
        return r
    xin = np.asarray(xin)
    assert xin.shape == (N, 48) and np.isfinite(xin.astype(np.float32)).all()
    e = (np.abs(xin[:, :16].astype(np.float64) - P["value"]) / P["tol_feature"]).max(1)
    r["feature"] = float(e[dec].max(initial=0.0))
    assert r["feature"] <= 1.0, f"{name}: features {r['feature']:.3g} of the bound at point {np.flatnonzero(dec)[e[dec].argmax()]}"
    value, bound = pf.ladder(sdf.astype(np.float32))  # from the kernel's own sdf bits: every row, nothing excluded
    r["ladder"] = float((np.abs(xin[:, 16:41].astype(np.float64) - value) / bound).max(initial=0.0))
    assert r["ladder"] <= 1.0, f"{name}: ladder {r['ladder']:.3g} of the bound"
    assert (xin[:, 41:] == 1).all(), f"{name}: the padding columns are ones"
    return r


def describe(P):
    return dict(N=P["x"].shape[0], K=P["K"], excluded=float(1 - P["decided_mask"].mean()), at_threshold=float((P["decided"] & ~P["decided_mask"]).mean()), far=float(P["far"].mean()), masked_in=float(P["mask"].mean()),
                inside=float((P["raw"] < 0).mean()))
