"""TEST INFRASTRUCTURE: a float64 restatement of the resampling of an imported feature patch (the `imported_type == 'patch'` branch of
MeshFeatureField.forward, tools/map.py:676-692, over weighted_project(weighting='DualD'), :435-452, and knn(use_dir_vec=False,
direct_above_check=True, direct_above_threshold=1., weighting='Shepard'), :454-501) with a per-element first-order bound on the error of an
fp32 evaluation, for tests/test_import_patch_cpu.py and tests/test_gpu_import_patch.py.  Plain numpy.

It STARTS FROM THE fp32 INPUTS (sample positions, the patch's points, normals and records) AND FROM THE NEIGHBOUR SET UNDER TEST (`idx`), after
`check_neighbours` has found that set legitimate: ties and near-ties at the 8th distance may be broken either way by an fp32 search, and which
way is not this model's business.

    dv_k = x - p[idx_k],  dis_k = |dv_k|,  dir_k = dv_k / (|dv_k| + 1e-5),  A = 2 min_k |n_k x dir_k|          (the direct-above quantity)
    A >= 1:  every dis_k and every component of every dv_k becomes 1e5
    a_k = 1 / (dis_k + 1e-7),  a_k /= sum a;  normal = sum_k a_k n_k / (|n_k| + 1e-5),  normal /= |normal| + 1e-5
    s_k = dv_k . normal,  t_k = |(dv_k - s_k normal)^2|_2,  dk = max t,  d1 = min t
    w_k = (dk - t_k) / (dk - d1 + 1e-5) (dk + d1) / (dk + t_k),  w_k /= sum w + 1e-5,  sdf = sum_k s_k w_k
    x_embed = sum_k w_k F[idx_k]  (likewise phi_embed, local_tbn),  ladder = FreqEncoder(sdf),  mask = A < 1 and |sdf| < h and min dis < h

THE ERROR MODEL: u = 2^-24 (half an fp32 ulp, relative); every operation of the fp32 evaluation rounds once, and an operand's error reaches the
result through the operation's first derivative -- a running error analysis, carried along with the float64 values by the class `E` below
(value v, bound e >= 0 on |fp32 evaluation - v|).  The rules, one per operation, and where each named term of the chain enters:
  inputs       fp32 values: e = 0.  The constants 1e-5, 1e-7, 1e5 are the fp32 ones.
  a +- b       e = e_a + e_b + u |a +- b|.  THE CANCELLATION in r = dv - s normal enters here: e_r = e_dv + e(s normal) + u |r|, an ABSOLUTE error
               of the size of u |dv| while r itself may be much smaller (a sample right above a point) -- and then twice more through the squares,
               e(r^2) = 2 |r| e_r + u r^2, e(q^2) likewise, so t = |r^2|_2 carries about 4 u |dv|^2 |r|^2 / t + ..., not 4 u t.
  a b          e = |a| e_b + |b| e_a + u |a b|.
  a / b        e = e_a / |b| + |a| e_b / b^2 + u |a / b|.  THE DIVISION BY dk - d1 + 1e-5 enters here with e_b = e_dk + e_d1 + 2 u (...): where the
               eight t_k are nearly equal (a sample high above a flat patch) the divisor is close to 1e-5 and e_b / b^2 is what makes the bound on
               the weights wide; THE DIVISION BY sum w + 1e-5 the same way with e_b = the sum's bound.
  sqrt a       e = sqrt(a + e_a) - sqrt(max(a - e_a, 0)) + u sqrt(a): the exact width of the image of [a - e_a, a + e_a], which is the first-order
               term e_a / (2 sqrt a) away from 0 and stays finite at 0 (|dv_k| of a sample on a point, t_k of a sample above one).
  min, max     over k: e = max_k e_k (the extremum of perturbed values moves by at most the largest perturbation).
  sum          of n terms, in ANY order: e = sum_k e_k + (n - 1) u sum_k |v_k| (each of the n - 1 additions rounds a partial sum that is at most
               sum |v_k|), so the bound holds for the kernel's ascending order and for a framework reduction alike.
  sin, cos     of sdf 2^k (the product is exact): min(2^k e_sdf, 2) + 8 u |value| (4 fp32 ulp: OpenCL C 3.0 section 7.4, as tests/planar_float64.py).
  narrowing    the 41 embedding columns and the lit chain's phi go to half: + 2^-11 (|value| + e) + 2^-25.
The bound is this propagation, evaluated per element; it is not fitted to any output.

THE THREE TESTS of a row are decided in float64; a row is UNDECIDED when float64 puts A within its bound of 1, |sdf| within its bound of h, or
min dis within its bound of h.  Undecided rows are left out of the MASK comparison only -- with one consequence spelled out: a row whose A is
undecided may have taken either side of the select in fp32, and like every row that FAILS the direct-above test (`above` False: its
intermediate values are of the order of 1e10 and are not compared) its values are not compared (`compare` = above and A decided).
"""
import numpy as np

U = 2.0 ** -24
UH = 2.0 ** -11
HALF_TINY = 2.0 ** -25
TINY = 2.0 ** -149
N_FREQS = 12
K = 8
C5, C7, BIG = float(np.float32(1e-5)), float(np.float32(1e-7)), float(np.float32(1e5))


class E:
    """value v (float64) and a bound e on |fp32 evaluation - v|; the operators are the fp32 operations of the module docstring."""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    @staticmethod
    def lift(a):
        return a if isinstance(a, E) else E(a)

    def _rounded(self, v, e):
        return E(v, e + U * np.abs(v) + TINY)

    def __add__(self, o):
        o = E.lift(o)
        return self._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = E.lift(o)
        return self._rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.lift(o) - self

    __radd__ = __add__

    def __mul__(self, o):
        o = E.lift(o)
        return self._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = E.lift(o)
        return self._rounded(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))

    def __rtruediv__(self, o):
        return E.lift(o) / self

    def sqrt(self):
        v = np.sqrt(self.v)
        return self._rounded(v, np.sqrt(self.v + self.e) - np.sqrt(np.maximum(self.v - self.e, 0.0)))

    def __getitem__(self, i):
        return E(self.v[i], self.e[i])

    def where(self, cond, other):
        other = E.lift(other)
        return E(np.where(cond, self.v, other.v), np.where(cond, self.e, other.e))

    def extremum(self, fn, axis):
        return E(fn(self.v, axis=axis), self.e.max(axis=axis))

    def sum(self, axis):
        n = self.v.shape[axis]
        return E(self.v.sum(axis=axis), self.e.sum(axis=axis) + (n - 1) * U * np.abs(self.v).sum(axis=axis) + TINY)


def norm3(a):
    """|a| over the last axis of an E of shape [..., 3]: three squares, two additions, one square root."""
    return (a * a).sum(-1).sqrt()


def _half_bound(value, fp32_bound):
    return fp32_bound + UH * (np.abs(value) + fp32_bound) + HALF_TINY


def check_neighbours(points, x, idx):
    """The neighbour set under test is legitimate: no returned point lies farther than the true 8th distance plus the slack, and every point
    closer than the 8th distance minus the slack is present.  The slack is 8 u D8: the search's squared distance rounds q - p once per axis
    (u |d| each, 2 u in the square), and adds the three squares with fused multiply-adds (<= 3 u d^2) -- 5 u d^2, 2.5 u in the distance; a
    comparison is between two such values (5 u), rounded up to 8 u."""
    p, q = np.asarray(points, np.float64), np.asarray(x, np.float64)
    d = np.sqrt(((q[:, None, :] - p[None, :, :]) ** 2).sum(-1))  # [N, V]
    d8 = np.sort(d, axis=-1)[:, K - 1]
    slack = 8 * U * d8 + TINY
    idx = np.asarray(idx).astype(np.int64)
    assert idx.shape == (len(q), K) and idx.min() >= 0 and idx.max() < len(p)
    assert all(len(set(row.tolist())) == K for row in idx), "a point returned twice"
    got = np.take_along_axis(d, idx, axis=-1)
    assert (got <= (d8 + slack)[:, None]).all(), "a returned point lies beyond the 8th distance"
    present = np.zeros(d.shape, bool)
    np.put_along_axis(present, idx, True, axis=-1)
    assert present[d < (d8 - slack)[:, None]].all(), "a closer point is missing"


def resample(points, normals, features, x, idx, h_threshold, phi_embed=None, local_tbn=None):
    """points [V,3], normals [V,3], features [V,16], x [N,3] (all fp32), idx [N,8] the neighbour set under test
    -> dict of (value float64, bound) pairs `normal` [N,3] (the raw coarse normal), `sdf` [N], `weights` [N,8], `embed` [N,41] (half-narrowed),
       and with phi_embed [V,8] / local_tbn [V,9]: `phi` [N,8] (fp32), `phi_half` (narrowed) and `tbn` [N,9];
       and the booleans `above`, `mask` (float64's), `undecided` [N], `compare` [N] (module docstring), `sides`: per test the decided rows on
       either side, as ((A < 1, A >= 1), (|sdf| < h, >= h), (min dis < h, >= h)) counts."""
    for a in (points, normals, features, x):
        assert np.asarray(a).dtype == np.float32
    idx = np.asarray(idx).astype(np.int64)
    h = float(np.float32(h_threshold))
    with np.errstate(all="ignore"):
        p, n = E(np.asarray(points)[idx]), E(np.asarray(normals)[idx])  # [N,8,3]
        dv = E(np.asarray(x)[:, None, :]) - p
        dis = norm3(dv)
        direction = dv / E((dis + C5).v[..., None], (dis + C5).e[..., None])
        nv, dr = n, direction
        cross = [nv[..., 1] * dr[..., 2] - nv[..., 2] * dr[..., 1], nv[..., 2] * dr[..., 0] - nv[..., 0] * dr[..., 2],
                 nv[..., 0] * dr[..., 1] - nv[..., 1] * dr[..., 0]]
        cr = (cross[0] * cross[0] + cross[1] * cross[1] + cross[2] * cross[2]).sqrt()
        A = E(2.0) * cr.extremum(np.min, -1)
        above = A.v < 1.0
        a_undecided = np.abs(A.v - 1.0) <= A.e
        dis = dis.where(above[:, None], BIG)
        dv = dv.where(above[:, None, None], BIG)
        a = 1.0 / (dis + C7)
        a = a / E(a.sum(-1).v[:, None], a.sum(-1).e[:, None])
        nlen = norm3(n) + C5
        unit = n / E(nlen.v[..., None], nlen.e[..., None])
        normal = (unit * E(a.v[..., None], a.e[..., None])).sum(1)
        nl = norm3(normal) + C5
        normal = normal / E(nl.v[:, None], nl.e[:, None])
        nb = E(normal.v[:, None, :], normal.e[:, None, :])
        s = (dv * nb).sum(-1)
        r = dv - E(s.v[..., None], s.e[..., None]) * nb  # (the cancellation)
        q2 = r * r
        t = (q2 * q2).sum(-1).sqrt()
        dk, d1 = t.extremum(np.max, -1), t.extremum(np.min, -1)
        dkb, d1b = E(dk.v[:, None], dk.e[:, None]), E(d1.v[:, None], d1.e[:, None])
        w = (dkb - t) / (dkb - d1b + C5) * (dkb + d1b) / (dkb + t)
        W = w.sum(-1) + C5
        w = w / E(W.v[:, None], W.e[:, None])
        sdf = (s * w).sum(-1)
        wb = E(w.v[..., None], w.e[..., None])

        def gather(table):
            return (wb * E(np.asarray(table, np.float32)[idx])).sum(1)

        fe = gather(features)
        cols, bounds = [sdf.v], [sdf.e]
        for k in range(N_FREQS):
            for fn in (np.sin, np.cos):
                val = fn(sdf.v * 2.0 ** k)
                cols.append(val)
                bounds.append(np.minimum(2.0 ** k * sdf.e, 2.0) + 8 * U * np.abs(val))
        zv, zb = np.stack(cols, -1), np.stack(bounds, -1)
        ev, eb = np.concatenate([fe.v, zv], -1), np.concatenate([fe.e, zb], -1)
        out = dict(normal=(normal.v, normal.e), sdf=(sdf.v, sdf.e), weights=(w.v, w.e), embed=(ev, _half_bound(ev, eb)))
        if phi_embed is not None:
            ph, tb = gather(phi_embed), gather(np.asarray(local_tbn, np.float32).reshape(len(points), 9))
            out.update(phi=(ph.v, ph.e), phi_half=(ph.v, _half_bound(ph.v, ph.e)), tbn=(tb.v, tb.e))
        dis0 = dis.extremum(np.min, -1)
        s_in, d_in = np.abs(sdf.v) < h, dis0.v < h
        s_undecided, d_undecided = np.abs(np.abs(sdf.v) - h) <= sdf.e, np.abs(dis0.v - h) <= dis0.e
        # (a row that fails the direct-above test has sdf = 0 and dis = 1e5 exactly, whatever its values were: decided)
        s_undecided, d_undecided = s_undecided & above, d_undecided & above
    undecided = a_undecided | s_undecided | d_undecided
    sides = ((int((above & ~a_undecided).sum()), int((~above & ~a_undecided).sum())), (int((s_in & ~s_undecided).sum()), int((~s_in & ~s_undecided).sum())),
             (int((d_in & ~d_undecided).sum()), int((~d_in & ~d_undecided).sum())))
    out.update(above=above, mask=above & s_in & d_in, undecided=undecided, compare=above & ~a_undecided, sides=sides, A=(A.v, A.e))
    return out


def assert_within(got, pair, rows, what):
    """|got - value| <= bound on the rows `rows`, with the worst element in the message."""
    value, bound = pair
    got = np.asarray(got, np.float64)
    err = np.abs(got - value)
    bad = (~(err <= bound)) & (rows[:, None] if err.ndim == 2 else rows)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound; worst at {i}: got {got[i]!r}, float64 {value[i]!r}, "
                             f"error {err[i]:.3e}, bound {bound[i]:.3e}")


# ---- the cases the CPU and GPU tests share ---------------------------------------------------------------------------------------------------------
GRID_GAP, H_THRESHOLD, CURVATURE = 1.0 / 32, 0.0625, 0.2  # (the grid gap and threshold of the import_field tests; z = a (x^2 - y^2))
SIZES = (3, 12, 33)  # V = 9: every query drops exactly one point; 144: the general case; 1089: the search leaves the first block of cells


def seeded_patch(S, per_point_normals=False, lit=False, seed=5):
    """-> dict(points [S^2,3], normals [S^2,3] or [3], features [S^2,16], + lit: phi_embed [S^2,8], local_tbn [S^2,9]), fp32: an S x S grid on
    z = a (x^2 - y^2) -- gently curved: the surface normal leans by at most 2 a (S - 1) gap / 2 = 0.2 rad at the rim of S = 33.  normals: the
    one patch normal (0, 0, 1) as the reference stores it at every point, or (per_point_normals) the surface's own, which differ."""
    rng = np.random.default_rng(seed + 100 * S + int(per_point_normals))
    c = (np.arange(S, dtype=np.float64) - (S - 1) / 2) * GRID_GAP
    gx, gy = np.meshgrid(c, c, indexing="ij")
    pts = np.stack([gx, gy, CURVATURE * (gx * gx - gy * gy)], -1).reshape(-1, 3).astype(np.float32)
    if per_point_normals:
        nr = np.stack([-2 * CURVATURE * gx, 2 * CURVATURE * gy, np.ones_like(gx)], -1).reshape(-1, 3)
        nr = (nr / np.linalg.norm(nr, axis=-1, keepdims=True)).astype(np.float32)
    else:
        nr = np.array([0.0, 0.0, 1.0], np.float32)
    out = dict(points=pts, normals=nr, features=rng.uniform(-0.5, 0.5, (S * S, 16)).astype(np.float32))
    if lit:
        out["phi_embed"] = rng.uniform(-0.5, 0.5, (S * S, 8)).astype(np.float32)
        out["local_tbn"] = (np.eye(3, dtype=np.float32).reshape(9) + rng.normal(0, 0.35, (S * S, 9))).astype(np.float32)
    return out


def full_normals(patch):
    n = np.asarray(patch["normals"], np.float32)
    return np.ascontiguousarray(np.broadcast_to(n, patch["points"].shape)) if n.ndim == 1 else n


def case_queries(patch, B, seed=0):
    """[B,3] fp32 sample positions, five kinds in turn: right above (and below) a point along its normal, at heights up to 1.3 h; between four
    points, likewise; outside the patch's rim by up to three gaps; beyond h_threshold (1.05 .. 1.6 h above or below); and seeded points of the
    patch's box, grown by two gaps, x 1.4 h.  The first row is of the first kind, so B = 1 holds a row that passes the direct-above test."""
    pts, nr = np.asarray(patch["points"], np.float64), full_normals(patch).astype(np.float64)
    S = int(round(np.sqrt(len(pts))))
    rng = np.random.default_rng(seed + 7919 * S + B)
    h, half = H_THRESHOLD, (S - 1) / 2 * GRID_GAP
    rows = []
    for b in range(B):
        kind = b % 5
        i = int(rng.integers(0, len(pts)))
        t = rng.uniform(-1.3, 1.3) * h if b else 0.55 * h
        if kind == 0:
            q = pts[i] + t * nr[i] + rng.normal(0, 1e-3, 3) * GRID_GAP
        elif kind == 1:
            xy = pts[i, :2] + 0.5 * GRID_GAP * np.where(pts[i, :2] > 0, -1.0, 1.0) if S > 1 else pts[i, :2]
            q = np.array([xy[0], xy[1], CURVATURE * (xy[0] ** 2 - xy[1] ** 2) + t])
        elif kind == 2:
            side, along = rng.integers(0, 4), rng.uniform(-half, half)
            out = half + rng.uniform(0.2, 3.0) * GRID_GAP
            xy = [(out, along), (-out, along), (along, out), (along, -out)][side]
            q = np.array([xy[0], xy[1], CURVATURE * (xy[0] ** 2 - xy[1] ** 2) + t])
        elif kind == 3:
            q = pts[i] + np.sign(t if t else 1.0) * rng.uniform(1.05, 1.6) * h * nr[i] + rng.normal(0, 0.1, 3) * GRID_GAP * np.array([1, 1, 0])
        else:
            xy = rng.uniform(-(half + 2 * GRID_GAP), half + 2 * GRID_GAP, 2)
            q = np.array([xy[0], xy[1], CURVATURE * (xy[0] ** 2 - xy[1] ** 2) + rng.uniform(-1.4, 1.4) * h])
        rows.append(q)
    return np.ascontiguousarray(np.asarray(rows, np.float64).reshape(B, 3).astype(np.float32))


def bruteforce_neighbours(points, x):
    """The exact 8 nearest points in float64, ascending, ties in index order: (idx [N,8] int32, dis [N,8] float64)."""
    p, q = np.asarray(points, np.float64), np.asarray(x, np.float64)
    d = np.sqrt(((q[:, None, :] - p[None, :, :]) ** 2).sum(-1))
    idx = np.argsort(d, axis=-1, kind="stable")[:, :K]
    return idx.astype(np.int32), np.take_along_axis(d, idx, axis=-1)
