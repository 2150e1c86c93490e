"""Float64 model of the patch export's front (CurvedField.export_field, nerftex_patch_front): per candidate the frame, the ray origins, the
verdict and what of it float32 may legitimately decide otherwise.  numpy and torch only (tests/geometry_float64.py's brute-force tracer):
imported by tests/test_patch_export_cpu.py (no GPU) and tests/test_gpu_patch_export.py.

The construction (`patch_problem(S, with_scan)`)
  mesh        star_flower_mesh(18, 36) -- its faces wind INWARD, so a candidate's outward normal is minus the face's cross product;
  cast mesh   the faces whose centroid lies beyond z = CUT_Z: an OPEN cap, less than half of the mesh (the reference's picked faces) -- the
              rays of a patch on its rim that pass the rim leave through the open side and miss (code 4);
  candidates  47 centroids of cast-mesh faces with their outward face normals, plus ONE whose normal is first_component = (1, 0, 0): its
              frame is NaN (code 2); with no scan cloud those below y = 0 are code 1;
  patch       edge = S grid_gap = 2.5 mean edge lengths of the cast mesh;
  scan cloud  random points on the faces of the FULL mesh with centroid x < SCAN_X: patches beyond are farther than the limit (code 3).

What is compared with what
  inputs      the device gets float32 frames and a float32 calibration; the model reads exactly those values in float64, so the only float32
              arithmetic between the two is the origin's: (T0 x + T1 y) + T3, three roundings -- |error| <= 3 u (|T0 x| + |T1 y| + |T3|)
              (1 + 3 u), u = 2^-24 -- and the lift's two more.
  verdict     NaN, then the scan distance, then the depth, then the cap, in the reference's order.  A candidate is DECIDED when float32 cannot
              legitimately answer otherwise: its maximum scan distance is farther from the limit than SCAN MARGIN = the origin bound (a
              distance is 1-Lipschitz in the query) + 2^-21 limit (the neighbour search's distance bound, KNN_RTOL) + 2^-24 limit (the limit
              itself is rounded to float32); and, where the depth test is reached, every ray is decided by the tracer's own rules
              (`trace_reference`).  With a cap, a candidate behind undecided ones is decided only if the cap falls on the same side of it however they go.
  positions   on decided rays of accepted patches: |hit - reference hit| <= 2 tol_t + origin bound (1 + 1 / cos): tol_t is the tracer's own
              tolerance (`set_trace_tolerances`: depth, and position against its own depth), and a ray displaced by e meets a face whose normal makes
              the angle with cos at most e (1 + 1 / cos) away.
"""
import functools

import numpy as np

import geometry_float64 as g

U = 2.0 ** -24
N_CANDIDATES = 48
CUT_Z, SCAN_X = 0.1, 0.35
H_THRESHOLD = 0.05
LIMIT = float(np.float32(min(1e-1, 3 * H_THRESHOLD)))
MISS_DEPTH, LIFT = 9.5, float(np.float32(0.1))
FIRST_COMPONENT = np.array([1.0, 0.0, 0.0])
SIZES = (3, 8, 12)
SEEDS = {3: 7, 8: 7, 12: 7}  # tuned on the CPU until every case holds its exclusion cap (tests/test_patch_export_cpu.py)
ACCEPTED, BELOW, NAN_ORIGIN, FAR, MISSED, NOT_NEEDED = 0, 1, 2, 3, 4, 5
MUTANTS = ("xy_order", "no_lift", "transposed", "mean_depth", "uncapped", "tail_lanes")


def reference_frames(points, normals, first_component):
    """tools/map.py:1030-1038 restated: T[:3,:4] per candidate, float64."""
    out = np.empty((points.shape[0], 3, 4))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(points.shape[0]):
            z_axis = normals[i]
            y_axis = np.cross(z_axis, first_component)
            if y_axis.sum() == 0:
                y_axis = np.cross(z_axis, np.array([1., 1., 1.01]) * first_component)
            y_axis = y_axis / np.linalg.norm(y_axis)
            x_axis = np.cross(y_axis, z_axis)
            T = np.eye(4)
            T[:3, :3] = np.stack([x_axis, y_axis, z_axis], -1)
            T[:3, 3] = points[i]
            out[i] = T[:3, :4]
    return out


def _origins(frames32, cal32, variant=None):
    """-> (pre-lift origins [n,S^2,3], lifted [n,S^2,3], directions [n,3], origin bound [n,S^2], lift bound) in float64 from the float32 inputs."""
    T = frames32.astype(np.float64).reshape(-1, 3, 4)
    if variant == "transposed":
        T = np.concatenate([T[:, :, :3].transpose(0, 2, 1), T[:, :, 3:]], axis=2)
    c = cal32.astype(np.float64)
    a, b = np.meshgrid(c, c, indexing="xy" if variant == "xy_order" else "ij")
    x, y = a.reshape(-1), b.reshape(-1)
    tx, ty = T[:, None, :, 0] * x[None, :, None], T[:, None, :, 1] * y[None, :, None]
    o = tx + ty + T[:, None, :, 3]
    bound = 3 * U * (1 + 3 * U) * (np.abs(tx) + np.abs(ty) + np.abs(T[:, None, :, 3]))
    lift = np.zeros_like(T[:, :, 2]) if variant == "no_lift" else LIFT * T[:, :, 2]
    lifted = o + lift[:, None, :]
    lift_bound = 2 * U * (1 + 2 * U) * (np.abs(o) + np.abs(lift[:, None, :]))
    return o, lifted, -T[:, :, 2], np.linalg.norm(bound, axis=-1), np.linalg.norm(bound + lift_bound, axis=-1)


def _scan_distance(o, scan):
    """nearest scan point of every origin, float64 brute force: [n, S^2]"""
    s = scan.astype(np.float64)
    flat = o.reshape(-1, 3)
    out = np.empty(flat.shape[0])
    for a in range(0, flat.shape[0], 512):
        d = flat[a:a + 512, None, :] - s[None]
        out[a:a + 512] = np.sqrt((d * d).sum(-1).min(1))
    return out.reshape(o.shape[:2])


GEOMETRIC = ("xy_order", "no_lift", "transposed")  # the variants that move the rays; the others read the true rays' results differently


def _evaluate(P, variant=None):
    """The front in float64 (or a deliberately wrong variant of it): every candidate's own code (no cap), and for the true model what decides it."""
    moved = variant if variant in GEOMETRIC else None
    cache = P.setdefault("_geometry", {})
    if moved not in cache:
        cache[moved] = _geometry(P, moved)
    return _codes(P, dict(cache[moved]), variant)


def _geometry(P, variant):
    n, S2 = P["n"], P["S"] * P["S"]
    o, lifted, d, ob, ob_lift = _origins(P["frames32"], P["cal32"], variant)
    nan = np.isnan(o).any(axis=(1, 2))
    ok = ~nan & ~P["below"]
    E = {"o": o, "lifted": lifted, "d": d, "ob": ob, "ob_lift": ob_lift, "nan": nan}
    far = np.zeros(n, bool)
    scan_ok = np.ones(n, bool)
    if P["scan"] is not None:
        dist = np.zeros((n, S2))
        dist[ok] = _scan_distance(o[ok], P["scan"])
        dmax = dist.max(1)
        margin = ob.max(1, initial=0.0, where=~np.isnan(ob)) + (g.KNN_RTOL + U) * LIMIT
        far = ok & (dmax > LIMIT)
        scan_ok = ~ok | (np.abs(dmax - LIMIT) > margin)
        E["scan_dist"], E["scan_margin"] = dmax, margin
    # the traces: every candidate that is neither below nor NaN (the device casts those too; a far one's rays decide nothing)
    rays = np.flatnonzero(ok)
    o32 = lifted[rays].reshape(-1, 3).astype(np.float32)
    d32 = np.repeat(d[rays].astype(np.float32), S2, axis=0)
    ref = g.trace_reference(P["v"], P["cast_f"], o32, d32)
    E["rays"] = {"name": f"patch S={P['S']}", "v": P["v"], "f": P["cast_f"], "o": o32, "d": d32, "ref": ref, "rows": rays}
    depth = np.full((n, S2), 0.0)
    depth[rays] = ref["t_best"].reshape(-1, S2)
    ray_decided = np.ones((n, S2), bool)
    ray_decided[rays] = ref["decided"].reshape(-1, S2)
    pos = np.zeros((n, S2, 3))
    pos[rays] = (o32.astype(np.float64) + ref["t_best"][:, None] * d32.astype(np.float64)).reshape(-1, S2, 3)
    cos = np.ones((n, S2))
    cos[rays] = ref["cos"].reshape(-1, S2)
    E.update(ok=ok, far=far, scan_ok=scan_ok, depth=depth, ray_decided=ray_decided, pos=pos, cos=cos)
    return E


def _codes(P, E, variant):
    n, S2 = P["n"], P["S"] * P["S"]
    nan, ok, far, scan_ok, depth, ray_decided = E["nan"], E["ok"], E["far"], E["scan_ok"], E["depth"], E["ray_decided"]
    if variant == "mean_depth":
        stat = depth.mean(1)
    elif variant == "tail_lanes" and S2 % 64:
        stat = np.maximum(depth.max(1), g.MAX_DIST)  # the lanes past S^2 of the last wave traced garbage: a miss
    else:
        stat = depth.max(1)
    missed = ok & ~far & (stat > MISS_DEPTH)
    code = np.zeros(n, np.uint8)
    code[P["below"]], code[nan], code[far], code[missed] = BELOW, NAN_ORIGIN, FAR, MISSED
    E["code"] = code
    # decided (the true model's): NaN and below always; otherwise the scan margin, and the rays where the depth test is reached
    E["own_decided"] = P["below"] | nan | (scan_ok & (far | ray_decided.all(1)))
    return E


@functools.lru_cache(maxsize=None)
def patch_problem(S, with_scan, seed=None):
    seed = SEEDS[S] if seed is None else seed
    rng = np.random.default_rng(seed)
    v, f = g.star_flower_mesh(18, 36)
    v8, fi = v.astype(np.float64), f.astype(np.int64)
    cen = v8[fi].mean(1)
    fn = -np.cross(v8[fi[:, 1]] - v8[fi[:, 0]], v8[fi[:, 2]] - v8[fi[:, 0]])  # outward: the faces wind inward
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    assert ((fn * cen).sum(1) > 0).all()
    cast = np.flatnonzero(cen[:, 2] > CUT_Z)
    cast_f = np.ascontiguousarray(f[cast])
    pick = rng.choice(cast, N_CANDIDATES, replace=False)
    points, normals = cen[pick].copy(), fn[pick].copy()
    normals[7] = FIRST_COMPONENT  # parallel to first_component: the fallback is zero too, the frame NaN
    e = np.unique(np.sort(cast_f.astype(np.int64)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1), axis=0)
    mean_edge = np.linalg.norm(v8[e[:, 0]] - v8[e[:, 1]], axis=-1).mean()
    grid_gap = 2.5 * mean_edge / S
    scan = None
    if with_scan:
        src = np.flatnonzero(cen[:, 0] < SCAN_X)
        t = src[rng.integers(0, src.shape[0], 6000)]
        w = rng.dirichlet(np.ones(3), 6000)
        scan = (v8[fi[t]] * w[:, :, None]).sum(1).astype(np.float32)
    frames = reference_frames(points, normals, FIRST_COMPONENT)
    cal = np.linspace(-S * grid_gap / 2, S * grid_gap / 2, S)
    P = {"S": S, "n": N_CANDIDATES, "v": v, "f": f, "cast_f": cast_f, "points": points, "normals": normals, "grid_gap": float(grid_gap), "scan": scan,
         "frames": frames, "frames32": frames.astype(np.float32), "cal": cal, "cal32": cal.astype(np.float32),
         "below": (points[:, 1] < 0) if scan is None else np.zeros(N_CANDIDATES, bool)}
    P["model"] = _evaluate(P)
    return P


def _capped(code, own_decided, max_patch_num):
    """(verdicts, decided) with the cap: a candidate is 'not needed' iff max_patch_num were accepted in front of it; decided only if that holds or
    fails however the undecided ones in front of it go."""
    n = code.shape[0]
    verdict, decided = code.copy(), own_decided.copy()
    sure = maybe = model = 0  # accepted in front: among the decided ones; those plus every undecided candidate; as the model itself answers
    for k in range(n):
        if sure >= max_patch_num:
            verdict[k], decided[k] = NOT_NEEDED, True
        elif maybe >= max_patch_num:
            decided[k] = False
            if model >= max_patch_num:
                verdict[k] = NOT_NEEDED
        hit = int(code[k] == ACCEPTED)
        model += hit
        if own_decided[k]:
            sure, maybe = sure + hit, maybe + hit
        else:
            maybe += 1
    return verdict, decided


def verdicts(P, max_patch_num=2000):
    M = P["model"]
    return _capped(M["code"], M["own_decided"], max_patch_num)


def emulate(P, max_patch_num=2000, mutate=None):
    """What a perfect front (or a deliberately wrong one, MUTANTS) returns: the keys of export_field's dict that `check_export` reads."""
    E = P["model"] if mutate is None else _evaluate(P, None if mutate == "uncapped" else mutate)
    verdict, _ = _capped(E["code"], np.ones(P["n"], bool), 1 << 30 if mutate == "uncapped" else max_patch_num)
    ids = np.flatnonzero(verdict == ACCEPTED)
    S = P["S"]
    f32 = P["frames32"].reshape(-1, 3, 4)[ids]
    return {"verdicts": verdict, "candidate_ids": ids.astype(np.int64), "patch_coors": E["pos"][ids].reshape(-1, S, S, 3).astype(np.float32),
            "patch_norms": P["normals"][ids].astype(np.float32), "picked_vertices": P["points"][ids].astype(np.float32),
            "patch_sample_tbn": np.ascontiguousarray(f32[:, :, :3].transpose(0, 2, 1)).reshape(-1, 9), "grid_gap": P["grid_gap"]}


def set_tolerances(P, trace32):
    """tol_t of the case's own rays from a float32 brute-force tracer `trace32(v, f, o, d) -> (pos, nrm, depth, face)` (the tracer's rule)."""
    R = P["model"]["rays"]
    if "tol_t" not in R:
        g.set_trace_tolerances(R, trace32(R["v"], R["f"], R["o"], R["d"]))
    tol = np.zeros((P["n"], P["S"] * P["S"]))
    tol[R["rows"]] = np.broadcast_to(R["tol_t"], R["ref"]["t_best"].shape).reshape(-1, P["S"] * P["S"])
    P["tol_t"] = tol
    return P


def check_export(P, out, max_patch_num=2000):
    """Asserts an export result against the model; -> {'decided': candidates, 'rays': decided rays compared, 'worst': worst position error over its tolerance}."""
    M, S, S2 = P["model"], P["S"], P["S"] * P["S"]
    want, decided = verdicts(P, max_patch_num)
    got = np.asarray(out["verdicts"])
    assert got.shape == want.shape
    bad = decided & (got != want)
    assert not bad.any(), f"S={S}: verdicts differ on decided candidates {np.flatnonzero(bad)[:8]}: got {got[bad][:8]}, want {want[bad][:8]}"
    ids = np.asarray(out["candidate_ids"])
    assert np.array_equal(ids, np.flatnonzero(got == ACCEPTED)), "candidate_ids are the accepted candidates in candidate order"
    assert len(ids) <= max_patch_num, f"{len(ids)} patches accepted with max_patch_num = {max_patch_num}"
    f32 = P["frames32"].reshape(-1, 3, 4)[ids]
    assert np.array_equal(out["patch_sample_tbn"], f32[:, :, :3].transpose(0, 2, 1).reshape(-1, 9)), "patch_sample_tbn = float32(T)[:3,:3].T"
    assert np.array_equal(out["patch_norms"], P["normals"][ids].astype(np.float32)) and np.array_equal(out["picked_vertices"], P["points"][ids].astype(np.float32))
    coors = np.asarray(out["patch_coors"], dtype=np.float64).reshape(-1, S2, 3)
    assert coors.shape[0] == len(ids)
    tol_t = P.get("tol_t", np.full((P["n"], S2), g.TOL_T_FLOOR * g.MAX_DIST))
    worst, rays = 0.0, 0
    for row, k in enumerate(ids):
        if not (decided[k] and want[k] == ACCEPTED):
            continue
        ok = M["ray_decided"][k]
        tol = 2 * tol_t[k] + M["ob_lift"][k] * (1 + 1 / np.maximum(M["cos"][k], g.GRAZE))
        err = np.abs(coors[row] - M["pos"][k]).max(-1)
        ratio = (err / tol)[ok].max(initial=0.0)
        assert ratio <= 1.0, f"S={S}: candidate {k}: a hit is {err[ok].max():.3g} off ({ratio:.3g} of the tolerance) at pixel {np.flatnonzero(ok)[(err / tol)[ok].argmax()]}"
        worst, rays = max(worst, float(ratio)), rays + int(ok.sum())
    return {"decided": int(decided.sum()), "rays": rays, "worst": worst}


def describe(P, max_patch_num=2000):
    want, decided = verdicts(P, max_patch_num)
    M = P["model"]
    sent = ~P["below"] & ~M["nan"]
    return {"S": P["S"], "undecided_candidates": float((~decided).mean()), "undecided_rays": float((~M["ray_decided"][sent]).mean()),
            "codes": {int(c): int(((want == c) & decided).sum()) for c in range(6)}}
