"""TEST INFRASTRUCTURE: a host model of the occupancy-grid maintenance of csrc/occupancy.hip (nerftex_occupancy_sample_full,
nerftex_occupancy_sample_partial[_ordered], nerftex_occupancy_update in include/nerftex_hip.h), for tests/test_gpu_occupancy_edges.py; checked on
the CPU by tests/test_occupancy_model_cpu.py.  Plain numpy, no GPU import.  The only native code it calls is the oracle's Morton code, packbits and
the restatement of the library's own draw (oracle.morton3D / morton3D_invert / packbits / occupancy_partial_draw): there is no second Morton code here.

THE OPERATION (NeRFRenderer.update_extra_state, nerf/renderer.py:566-660, as the header states it).  The grid is [cascade, H^3] float32 in Morton
order, H a power of two.

  cascade constants   b_k = min(2^k, bound), h_k = b_k / H, both formed in double (the Python scalars of renderer.py:596-599);
                      span_k = float32(b_k - h_k), half_k = float32(h_k).
  cell position       float32, one rounding per operation, per component d of cell (c_x, c_y, c_z) with jitter u in [0, 1):
                          inv  = float32(1) / float32(H - 1)
                          unit = (2 c_d) inv - 1
                          pos  = unit span_k
                          jit  = (u_d 2 - 1) half_k
                          out  = pos + jit
                      (`tensor / python_scalar` on a GPU multiplies by the scalar's float32 reciprocal: that is `inv`).
  full sweep          row k H^3 + m is the cell of cascade k whose Morton index is m; its density estimate IS tmp[k, m].
  occupied list       of cascade k: the ascending Morton indices m with grid[k, m] > 0 (zero is not occupied), and their count n_k.
  partial rows        2N rows per cascade.  Row j < N is the cell rand_coords[k, j]; row j >= N is list_k[rand_pick[k, j - N]], or index -1 and
                      position (0, 0, 0) when n_k = 0.  With NULL picks the library draws its own: oracle.occupancy_partial_draw.
  update              tmp = the estimates (full sweep), or -1 everywhere and then, over the rows with index >= 0 and estimate >= 0, the maximum
                      of the estimates that name a cell (a NaN or negative estimate never lands; -0 does, `-0 >= 0`, and counts as 0);
                      valid = force_full_grid or (grid >= 0 and tmp >= 0);  grid = max(grid decay, tmp) where valid (float32);
                      mean = float32(exact sum of max(grid, 0) / n), n = cascade H^3;  thresh = min(mean, density_thresh);
                      bitfield = packbits(grid > thresh).
                      The sum is exact (integer arithmetic on the float32 significands, the same number math.fsum returns), so the model's
                      mean does not depend on a summation order; the device adds block partials in double in some order and may land on
                      the neighbouring float32.

THE POSITION BOUND.  position_float64 evaluates the same expression in double from the same float32 inputs (b_k and h_k in double, as above).
u = 2^-24 is the unit roundoff.  Each float32 rounding enters once, at its worst case, to first order:
    inv                  relative u on a factor of a product of at most 2 (2 c / (H - 1) <= 2)        2 u
    (2 c) inv            the product, at most 2                                                       2 u
    ... - 1              |unit| <= 1                                                                  1 u
                         so |d unit| <= 5 u, carried into pos by |span| = b - h                       5 u (b - h)
    span                 float32(b - h) under |unit| <= 1                                             1 u (b - h)
    unit span            the product, at most b - h                                                   1 u (b - h)
    u 2 - 1              (u 2 is exact) at most 1, carried by h                                       1 u h
    half                 float32(h) under a factor of at most 1                                       1 u h
    (...) half           the product, at most h                                                       1 u h
    pos + jit            at most (b - h) + h = b                                                      1 u b
    total                7 u (b - h) + 3 u h + u b = 8 u b - 4 u h  <=  8 u b.
POSITION_ROUNDINGS = 8: |float32 position - float64 position| <= 8 * 2^-24 * b_k per component.  The constant is this count, not a measurement.

THE CASES.  cases() builds every input of every GPU case from fixed seeds, so that the CPU module (which asserts what the inputs must be for the
GPU comparison to mean something) and the GPU module see the same bytes.  See cases() for the shapes and what each is there for.

KNOWN DIFFERENCE, not exercised: with force_full_grid in a FULL sweep a NaN estimate reaches max(grid decay, NaN).  The reference's
torch.maximum propagates the NaN (and its mean, threshold and bitfield are gone with it); the kernel's fmaxf keeps grid decay.  The forced
full-sweep variants therefore carry the estimates without their NaN entries (Case.full_estimates_forced).
"""
import functools
from collections import namedtuple

import numpy as np

f32 = np.float32
U = 2.0 ** -24
POSITION_ROUNDINGS = 8

DECAYS = (1.0, 0.95)
FORCES = (0, 1)
THRESH_LOW = 2.0 ** -10   # below every case's mean (asserted on the CPU): the packing threshold is density_thresh itself
THRESH_HIGH = 1.0e4       # above every case's mean: the packing threshold is the mean
PATTERNS = ("unset", "zero", "first", "last", "full", "first256", "alternate", "random")


def _orc():
    from oracle import oracle as orc

    return orc


# ------------------------------------------------------------------------------------------------------------------ the model
class Model:
    """One method per mechanism, so that tests/test_occupancy_model_cpu.py can break exactly one of them (its mutants subclass this)."""

    def cascade_consts(self, cascade, H, bound):
        b = [min(float(2 ** k), float(bound)) for k in range(cascade)]
        return b, [f32(bk - bk / H) for bk in b], [f32(bk / H) for bk in b]

    def occupied(self, grid_c):
        """(list padded to H^3 with -1, count): the ascending Morton indices of the cells with density > 0."""
        idx = np.nonzero(grid_c > 0)[0].astype(np.int32)
        out = np.full(grid_c.shape[0], -1, np.int32)
        out[: idx.shape[0]] = idx
        return out, idx.shape[0]

    def scatter(self, tmp_c, idx, est):
        """tmp_c[idx] = max(tmp_c[idx], est) over the rows that land: index >= 0 and estimate >= 0 (NaN >= 0 is false)."""
        with np.errstate(invalid="ignore"):
            lands = (idx >= 0) & (est >= 0)
        np.maximum.at(tmp_c, idx[lands], est[lands])

    def ema(self, grid, tmp, decay, force_full_grid, partial):
        with np.errstate(invalid="ignore"):
            valid = np.ones(grid.shape, bool) if force_full_grid else (grid >= 0) & (tmp >= 0)
        out = grid.copy()
        out[valid] = np.maximum(grid[valid] * f32(decay), tmp[valid])
        return out

    def finish(self, grid, density_thresh):
        """(mean, threshold, bitfield) of the updated grid."""
        mean = exact_mean(grid)
        thresh = min(mean, f32(density_thresh))
        return mean, thresh, _orc().packbits(grid.reshape(-1), float(thresh))


MODEL = Model()


def exact_mean(grid):
    """float32(fsum(max(grid, 0)) / n): every float32 is an integer significand times a power of two; the significands are summed per exponent in
    integers (each sum < 2^53) and the exponents are put together in Python integers -- the exact sum, whatever the order."""
    v = np.maximum(grid.reshape(-1), f32(0)).astype(np.float64)
    assert np.isfinite(v).all()
    m, e = np.frexp(v)
    sig = (m * 2.0 ** 24).astype(np.int64)  # exact: a float32 significand has 24 bits
    e = e.astype(np.int64)
    lo = int(e.min())
    per_exp = np.bincount(e - lo, weights=sig.astype(np.float64))  # each bin < 2^24 n < 2^53: exact
    total = sum(int(s) << k for k, s in enumerate(per_exp))  # times 2^(lo - 24)
    shift = lo - 24
    num, den = (total << shift, 1) if shift >= 0 else (total, 1 << -shift)
    s = num / den  # Python's integer true division is correctly rounded: this is math.fsum's result
    return f32(s / v.shape[0])


def cell_positions(H, coords, span, half, u):
    """float32 positions [n, 3] of cells coords [n, 3] jittered by u [n, 3]: one rounding per operation, the sequence of the docstring."""
    inv = f32(1) / f32(H - 1)
    unit = (f32(2) * coords.astype(f32)) * inv - f32(1)
    pos = unit * f32(span)
    jit = (u.astype(f32) * f32(2) - f32(1)) * f32(half)
    return pos + jit


def position_float64(H, coords, b, u):
    """(position in float64 from the same float32 inputs, the magnitude b the bound scales with)."""
    h = b / H
    unit = 2.0 * coords.astype(np.float64) / (H - 1) - 1.0
    return unit * (b - h) + (u.astype(np.float64) * 2.0 - 1.0) * h, b


def position_tolerance(b):
    return POSITION_ROUNDINGS * U * b


def morton_coords(H):
    return _orc().morton3D_invert(np.arange(H ** 3, dtype=np.int32))


def full_positions(case, noise, model=MODEL):
    """[cascade * H^3, 3] float32: row k H^3 + m is Morton cell m of cascade k."""
    H3 = case.H ** 3
    _, span, half = model.cascade_consts(case.cascade, case.H, case.bound)
    coords = morton_coords(case.H)
    return np.concatenate([cell_positions(case.H, coords, span[k], half[k], noise[k * H3:(k + 1) * H3]) for k in range(case.cascade)])


def full_positions_float64(case, noise):
    H3 = case.H ** 3
    b, _, _ = MODEL.cascade_consts(case.cascade, case.H, case.bound)
    coords = morton_coords(case.H)
    pos = np.concatenate([position_float64(case.H, coords, b[k], noise[k * H3:(k + 1) * H3])[0] for k in range(case.cascade)])
    return pos, np.repeat(np.asarray(b), H3)[:, None]


def occupied_lists(case, model=MODEL):
    """(lists [cascade, H^3] int32 padded with -1, counts [cascade])."""
    both = [model.occupied(case.grid[k]) for k in range(case.cascade)]
    return np.stack([b[0] for b in both]), np.asarray([b[1] for b in both], np.int64)


def rows_positions(case, indices, noise, model=MODEL):
    """Positions of the rows `indices` [cascade, R] (Morton cell, -1 = none: position 0) with jitter noise [cascade * R, 3]."""
    R = indices.shape[1]
    _, span, half = model.cascade_consts(case.cascade, case.H, case.bound)
    out = np.zeros((case.cascade * R, 3), f32)
    for k in range(case.cascade):
        idx = indices[k]
        coords = _orc().morton3D_invert(np.maximum(idx, 0))
        pos = cell_positions(case.H, coords, span[k], half[k], noise[k * R:(k + 1) * R])
        pos[idx < 0] = 0
        out[k * R:(k + 1) * R] = pos
    return out


def partial_rows(case, draw, model=MODEL):
    """(indices [cascade, 2N] int32, xyzs [cascade * 2N, 3] float32, counts) for explicit picks."""
    lists, counts = occupied_lists(case, model)
    N = draw.N
    indices = np.empty((case.cascade, 2 * N), np.int32)
    for k in range(case.cascade):
        indices[k, :N] = _orc().morton3D(draw.rand_coords[k])
        indices[k, N:] = lists[k][draw.rand_pick[k]] if counts[k] > 0 else -1
    return indices, rows_positions(case, indices, draw.noise, model), counts


def library_rows(case, N, stratified, model=MODEL):
    """The same for the library's own draw (NULL picks) at case.seed."""
    lists, counts = occupied_lists(case, model)
    indices, jitter = _orc().occupancy_partial_draw(case.seed, case.cascade, case.H, N, [lists[k][:counts[k]] for k in range(case.cascade)], stratified)
    return indices, rows_positions(case, indices, jitter, model), counts


def update(case, estimates, indices, decay, force_full_grid, density_thresh, model=MODEL, grid=None):
    """(grid, mean, thresh, bitfield).  indices None: a full sweep, estimates [cascade * H^3]; else indices [cascade, R], estimates [cascade * R]."""
    grid = case.grid if grid is None else grid
    if indices is None:
        tmp = estimates.reshape(grid.shape).astype(f32)
    else:
        tmp = np.full(grid.shape, -1, f32)
        est = estimates.reshape(indices.shape)
        for k in range(case.cascade):
            model.scatter(tmp[k], indices[k], est[k])
    out = model.ema(grid, tmp, decay, bool(force_full_grid), indices is not None)
    return (out,) + tuple(model.finish(out, density_thresh))


def variants():
    """(mode, decay, force_full_grid, density_thresh) of the update test: the whole product."""
    return [(mode, d, f, t) for mode in ("full", "partial") for d in DECAYS for f in FORCES for t in (THRESH_LOW, THRESH_HIGH)]


def update_variant(case, mode, decay, force, thresh, model=MODEL):
    if mode == "full":
        return update(case, case.full_estimates_forced if force else case.full_estimates, None, decay, force, thresh, model)
    draw = case.draws[case.update_draw]
    indices, _, _ = partial_rows(case, draw, model)
    return update(case, draw.estimates, indices, decay, force, thresh, model)


# ------------------------------------------------------------------------------------------------------------------ the cases
Case = namedtuple("Case", "name H cascade bound patterns grid full_noise full_estimates full_estimates_forced draws update_draw library_N seed why")
Draw = namedtuple("Draw", "N rand_coords rand_pick noise estimates")

# (H, cascade, bound, one prior-grid pattern per cascade, N of the partial update, further N of row-only draws, N of the library's draws, why)
_SHAPES = (
    (8, 1, 1.0, ("random",), 3, (1, 128, 512), (1, 128, 512),
     "2 compaction blocks, 1 update block with half its threads idle, 64 bitfield bytes; 6 rows: cascade 2N not a multiple of 256"),
    (8, 2, 1.5, ("first", "unset"), 128, (1, 3, 512), (1, 128, 512),
     "a 1-cell list beside an empty one; bound 1.5 cuts the last cascade; 1 full update block"),
    (8, 3, 4.0, ("first256", "last", "zero"), 512, (3,), (),
     "a list that ends exactly on a block edge, a 1-cell list at H^3 - 1, all zero (not occupied); N = H^3; 2 update blocks, one half full"),
    (8, 5, 16.0, ("alternate", "unset", "full", "first", "random"), 128, (1,), (),
     "5 different occupancies in one call (cas * nblk and cas * H^3 indexing) at 2 blocks per cascade; 10 rows at N = 1"),
    (16, 1, 1.0, ("first256",), 1024, (1, 3, 4096), (1, 1024, 4096),
     "16 compaction blocks (inside one scan round), list = exactly the first block; 4 update blocks"),
    (16, 2, 1.5, ("full", "last"), 4096, (3,), (1, 1024, 4096),
     "a list of all H^3 cells (arange picks over the whole list, N = H^3) beside a 1-cell list at H^3 - 1; bound 1.5"),
    (16, 3, 4.0, ("random", "zero", "alternate"), 3, (1024,), (),
     "an update of 6 rows per cascade (18 rows, scatter of less than one block) over 12 update blocks"),
    (32, 2, 1.5, ("alternate", "random"), 8192, (1, 32768), (),
     "128 compaction blocks: the scan ends inside its only round; 64 update blocks, fewer than the mean kernel's threads"),
    (32, 5, 16.0, ("last", "full", "unset", "first256", "random"), 8192, (3,), (),
     "5 cascades at 128 blocks each; 160 update blocks, fewer than the mean kernel's threads"),
    (64, 1, 1.0, ("random",), 65536, (1,), (),
     "1024 compaction blocks: four whole scan rounds with a carry between them; 256 update blocks, one per thread of the mean kernel"),
    (64, 3, 4.0, ("first", "alternate", "last"), 65536, (3,), (),
     "cell 0 and cell H^3 - 1 alone at four scan rounds (the last block of the last round); 768 update blocks, 3 per thread"),
    (64, 5, 16.0, ("random", "unset", "first256", "full", "alternate"), 65536, (), (),
     "the largest: 1.3 M cells, 5 cascades of four scan rounds, 1280 update blocks, 5 per thread of the mean kernel"),
)


# one generator seed per shape.  tests/test_occupancy_model_cpu.py asserts what the inputs must satisfy (no cell within 2 ulps of a mean, ...); a seed
# that fails there is replaced there, on the CPU: the device never has a say in it
_SEEDS = (20240, 20241, 20242, 20243, 20244, 20245, 20246, 20247, 20248, 20249, 20250, 20264)


def _prior(pattern, H3, rng):
    values = (rng.random(H3, dtype=f32) * f32(30) + f32(1)).astype(f32)  # positives in [1, 31)
    g = np.full(H3, -1, f32)
    m = np.arange(H3)
    if pattern == "unset":
        pass
    elif pattern == "zero":
        g[:] = 0
    elif pattern == "first":
        g[0] = values[0]
    elif pattern == "last":
        g[H3 - 1] = values[H3 - 1]
    elif pattern == "full":
        g = values
    elif pattern == "first256":
        g[:256] = values[:256]
    elif pattern == "alternate":
        full = (m // 256) % 2 == 0
        g[full] = values[full]
        g[~full] = 0  # the empty blocks hold zeros: `> 0`, not `>= 0`
    elif pattern == "random":
        r = rng.random(H3)
        g = np.where(r < 0.3, values, np.where(r < 0.6, f32(0), np.where(r < 0.8, f32(-1), -values))).astype(f32)
    else:
        raise ValueError(pattern)
    return g


def _draw(case_grid, H, N, rng, with_estimates):
    """Explicit picks for every cascade.  With N >= 3 the rows are planted so that, per cascade with a non-empty list (A = the list's first cell):
    rows 0, 1 and N name A (three rows, both halves) with estimates 9, NaN, 7 (the maximum is neither the last row nor the NaN); row 2 carries
    -3; row N + 1 picks the list's last cell with estimate +0; row N + 2 carries -0 (its cell is occupied, so max(grid decay, -0) has one answer).
    A cascade with an empty list: rows 0, 1, 2 name one cell with 9, NaN, -3; row N (index -1) carries 1e6, row N + 1 +0."""
    cascade, H3 = case_grid.shape
    orc = _orc()
    coords = rng.integers(0, H, (cascade, N, 3), dtype=np.int32)
    pick = np.zeros((cascade, N), np.int32)
    noise = rng.random((cascade * 2 * N, 3), dtype=f32)
    est = None
    if with_estimates:
        assert N >= 3
        e = rng.random((cascade, 2 * N), dtype=f32) * f32(40)
        e[rng.random((cascade, 2 * N)) < 0.2] = 0  # the field's "nothing here": +0
        est = e
    for k in range(cascade):
        occ = np.nonzero(case_grid[k] > 0)[0]
        n = occ.shape[0]
        if n:
            pick[k] = rng.integers(0, n, N, dtype=np.int32)
            pick[k, 0] = 0 if (N > 1 or k % 2 == 0) else n - 1
            if N > 1:
                pick[k, 1] = n - 1
        if N >= 3:
            a = occ[0] if n else int(rng.integers(0, H3))
            coords[k, 0] = coords[k, 1] = orc.morton3D_invert(np.asarray([a], np.int32))[0]
            if not n:
                coords[k, 2] = coords[k, 0]
        if est is not None:
            est[k, 0], est[k, 1], est[k, 2] = 9.0, np.nan, -3.0
            est[k, N], est[k, N + 1] = (7.0, 0.0) if n else (1.0e6, 0.0)
            est[k, N + 2] = -0.0 if n else est[k, N + 2]
    return Draw(N, np.ascontiguousarray(coords), pick, noise, None if est is None else est.reshape(-1))


@functools.lru_cache(maxsize=None)
def cases():
    """Every input of every GPU case.  Per case: the prior grid (one occupancy pattern per cascade), jitter and estimates of a full sweep (with
    negative, NaN and +0 entries), explicit partial draws keyed by name -- "update" (the one the update test uses, planted as _draw says), "N<k>"
    (rows only) and, at H = 8 and 16, "list" (rand_pick = arange over the whole list, N = H^3) --, and the N of the library's own draws.
    One cell of a cascade that has a positive cell nobody names holds THRESH_LOW exactly and its neighbour in the list the next float32 above it:
    with decay 1 they sit on and just over the packing threshold of the THRESH_LOW variants (`>`, not `>=`)."""
    out = []
    for i, (H, cascade, bound, patterns, n_update, n_rows, n_library, why) in enumerate(_SHAPES):
        rng = np.random.default_rng(_SEEDS[i])
        H3 = H ** 3
        grid = np.stack([_prior(p, H3, rng) for p in patterns])
        draws = {"update": _draw(grid, H, n_update, rng, True)}
        for n in n_rows:
            draws[f"N{n}"] = _draw(grid, H, n, rng, False)
        if H <= 16:
            d = _draw(grid, H, H3, rng, False)
            counts = (grid > 0).sum(1)
            pick = np.stack([np.minimum(np.arange(H3), max(int(c) - 1, 0)) for c in counts]).astype(np.int32)
            draws["list"] = d._replace(rand_pick=pick)
        full_noise = rng.random((cascade * H3, 3), dtype=f32)
        est = rng.random(cascade * H3, dtype=f32) * f32(40)
        kind = rng.random(cascade * H3)
        est[kind < 0.25] = 0
        est[(kind >= 0.25) & (kind < 0.30)] = -2.5
        forced = est.copy()
        est[(kind >= 0.30) & (kind < 0.33)] = np.nan
        forced[(kind >= 0.30) & (kind < 0.33)] = -2.0
        # the two cells on the threshold: positive cells of the prior that no row of the update draw names, with a full-sweep estimate below them
        up = draws["update"]
        named = np.zeros(grid.shape, bool)
        for k in range(cascade):
            named[k, _orc().morton3D(up.rand_coords[k])] = True
            occ = np.nonzero(grid[k] > 0)[0]
            if occ.shape[0]:
                named[k, occ[up.rand_pick[k]]] = True
        for k in range(cascade):
            free = np.nonzero((grid[k] > 0) & ~named[k])[0]
            if free.shape[0] >= 2:
                grid[k, free[0]] = f32(THRESH_LOW)
                grid[k, free[1]] = np.nextafter(f32(THRESH_LOW), f32(1))
                for cell in free[:2]:
                    est[k * H3 + cell] = forced[k * H3 + cell] = 0
                break
        out.append(Case(f"H{H}c{cascade}", H, cascade, bound, patterns, grid, full_noise, est, forced, draws, "update", n_library, 77 + i, why))
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)
