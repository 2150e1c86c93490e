"""TEST INFRASTRUCTURE: the cases of the training march's dispatch tests (numpy and the oracle only, no GPU import).

One builder for tests/test_march_paths_cases_cpu.py, which asserts with the oracle alone that every case exercises what it names, and for
tests/test_gpu_march_paths.py, which runs the cases through every kernel combination `march_train_impl` (csrc/raymarching.hip) can launch.

Grids are occupancy bitfields of C * H^3 bits, H a power of two: the Morton index of a grid of another size runs past C * H^3 bits (in the
reference as well), so such a case would read outside the bitfield.  Rays are `scene.train_batch(N, seed=5)` with the degenerate rays of
tests/test_gpu_parity.py::_rays written over the first six, and the same batch mirrored through the origin.  The reference of a case -- near /
far and the oracle's march -- is computed once, cached and read-only; its row budget M comes from the oracle's own demand.
"""
import copy
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

BOUND, CASCADES, DT_GAMMA, MIN_NEAR = 2.0, 2, 1 / 128, 0.2
SIZES = (128, 256, 512)
GRIDS = ("scene", "ones", "alternate", "zeros")
BATCHES = (31, 65, 97)  # 31, 65: N % 64 in [1, 32], the expand pass's last block has one total word nobody wrote; 97: two 64-ray blocks, four
#                         32-ray count workgroups, the last ragged
AABB = np.array([-BOUND] * 3 + [BOUND] * 3, np.float32)
AABB.setflags(write=False)

_grids, _rays, _refs = {}, {}, {}


def is_pow2(H):
    return H > 0 and H & (H - 1) == 0


def _morton_order(dense):
    """[H, H, H] indexed (x, y, z) -> [H^3] indexed by the Morton code of (x, y, z): bit 3b of the code is bit b of x, 3b + 1 of y, 3b + 2 of z."""
    n = dense.shape[0].bit_length() - 1
    bits = dense.reshape((2,) * (3 * n))  # axes: x from its top bit down, then y, then z
    perm = [a for b in range(n) for a in (2 * n + b, n + b, b)]  # the code from its top bit down: z, y, x of the top bit, ...
    return bits.transpose(perm).reshape(-1)


def scene_bitfield(H):
    """The bits of `scene.Scene(bound=2.0, seed=1).bitfield(H)[2]`, which takes minutes and 11 GB at H = 512 because it evaluates all twenty
    blobs at every cell.  A blob adds exactly +0.0 outside 1.6 of its radii, and x + 0.0 == x, so here every blob is evaluated -- by Scene.density
    itself, in the same order -- on the cells of its bounding box only; the grid is then laid out and thresholded as Scene does it.
    What holds this to the harness: at H = 128 the whole bitfield equals Scene.bitfield (test_march_paths_cases_cpu.py); at every H, each time
    the grid is built, five x-slabs of each cascade are compared here, value by value at their Morton indices, with Scene.density of all blobs
    at Scene.density_grid's cell centres, and the threshold is Scene.bitfield's own expression over the whole grid.  The cells between the slabs
    at H = 256 and 512 are not compared with the harness by any test.  Peak host memory at H = 512 is about 3 GB (the float grid, np.clip's copy
    of it, one cascade in (x, y, z) order)."""
    from ngp_harness import scene

    assert is_pow2(H)
    sc = scene.Scene(bound=BOUND, seed=1)
    assert sc.cascade == CASCADES and sc.kind == "sparse"
    blobs = []
    for k in range(len(sc.radii)):
        one = copy.copy(sc)
        one.centers, one.radii, one.amps = sc.centers[k:k + 1], sc.radii[k:k + 1], sc.amps[k:k + 1]
        blobs.append(one)
    unit = 2.0 * np.arange(H, dtype=np.int32).astype(np.float32) / np.float32(H - 1) - 1.0  # Scene.density_grid, one axis of it
    grid = np.zeros((sc.cascade, H ** 3), np.float32)
    for cas in range(sc.cascade):
        b = min(2.0 ** cas, sc.bound)
        axis = unit * np.float32(b - b / H)
        slabs = []  # (blob, its bounding box cut into slabs along x of at most 2^21 cells: bounded temporaries)
        for one in blobs:
            reach = 1.7 * float(one.radii[0])  # past the blob's cut at 1.6 radii
            lo, hi = [], []
            for a in range(3):
                inside = np.nonzero(np.abs(axis.astype(np.float64) - float(one.centers[0, a])) <= reach)[0]
                lo.append(int(inside[0]) if inside.size else 0)
                hi.append(int(inside[-1]) + 1 if inside.size else 0)
            thick = max(1, (1 << 21) // max(1, (hi[1] - lo[1]) * (hi[2] - lo[2])))
            for x0 in range(lo[0], hi[0], thick):
                slabs.append((one, (slice(x0, min(x0 + thick, hi[0])), slice(lo[1], hi[1]), slice(lo[2], hi[2]))))

        def in_its_slab(job):
            one, box = job
            xx, yy, zz = np.meshgrid(axis[box[0]], axis[box[1]], axis[box[2]], indexing="ij")
            return box, one.density(np.stack([xx, yy, zz], -1))

        dense = np.zeros((H, H, H), np.float32)
        with ThreadPoolExecutor(max_workers=8) as pool:  # (numpy releases the interpreter lock inside its loops)
            for box, term in pool.map(in_its_slab, slabs):  # added in the blobs' order, as Scene.density adds them
                dense[box] += term
        grid[cas] = _morton_order(dense)
        del dense
        ax = np.arange(H, dtype=np.int32)
        for x in (0, H // 2 - 1, H // 2, 3 * H // 4 + 1, H - 1):  # both sides of the top coordinate bit, the faces, one inside the upper half
            xx, yy, zz = np.meshgrid(ax[x:x + 1], ax, ax, indexing="ij")
            coords = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], -1)
            pts = (2.0 * coords.astype(np.float32) / np.float32(H - 1) - 1.0) * np.float32(b - b / H)  # Scene.density_grid
            assert np.array_equal(grid[cas, scene.morton3d(coords).astype(np.int64)], sc.density(pts)), (H, cas, x)
    thresh = min(float(np.clip(grid, 0, None).mean()), sc.density_thresh)  # Scene.bitfield
    return np.packbits((grid.reshape(-1) > np.float32(thresh)).astype(np.uint8), bitorder="little")


def grid(name, H):
    """Occupancy bitfield of C * H^3 bits, cached and read-only."""
    assert H in SIZES and is_pow2(H) and name in GRIDS
    if (name, H) not in _grids:
        nbytes = CASCADES * H ** 3 // 8
        g = scene_bitfield(H) if name == "scene" else np.full(nbytes, {"ones": 0xFF, "alternate": 0x55, "zeros": 0x00}[name], np.uint8)
        assert g.shape == (nbytes,) and g.dtype == np.uint8
        g.setflags(write=False)
        _grids[(name, H)] = g
    return _grids[(name, H)]


def rays(N, degenerate=True, mirrored=False):
    """scene.train_batch(N, seed=5); degenerate: with the six special rays of tests/test_gpu_parity.py::_rays written over the first six.
    mirrored: the same rays reflected through the origin.  The batch comes from ONE view, so two of its three direction components have the same
    sign on nearly every ray, and with that sign a coordinate bit lost on the way to a voxel's exit only shortens the skip, which changes no
    sample; the mirrored batch walks the upper half of every axis with the other sign."""
    if (N, degenerate, mirrored) not in _rays:
        from ngp_harness import scene

        o, d = scene.train_batch(N, seed=5)
        if degenerate:
            d[0] = [0, 0, -1]  # axis-aligned (1 / 0 = inf is relied upon)
            o[0] = [0.1, 0.2, 1.9]
            d[1] = [1, 0, 0]
            o[1] = [-3, 0.3, 0.1]
            d[2] = -d[2]  # pointing away
            o[3] = [0.05, -0.1, 0.02]  # starting inside
            o[4] = [5.0, 5.0, 5.0]  # outside, looking away: misses the box on the first slab pair
            d[4] = [0.6, 0.64, 0.48]
            o[5] = [0.0, 5.0, 0.0]  # passes the x / y slabs' overlap test but misses in z
            d[5] = [0.0, -0.6, 0.8]
        if mirrored:
            o, d = -o, -d
        o.setflags(write=False)
        d.setflags(write=False)
        _rays[(N, degenerate, mirrored)] = (o, d)
    return _rays[(N, degenerate, mirrored)]


# o, d, nears, fars: the inputs.  M: the row budget.  base: counter[0] on entry.  total: the samples all rays ask for (the demand).
# xyzs, dirs, deltas, ts [M, .], records [N, 3], counter [2]: what the oracle gives.  dropped [N]: rays with samples that the budget cuts off.
Case = namedtuple("Case", "grid_name H max_steps N perturb budget mirrored o d nears fars M base total xyzs dirs deltas ts records counter dropped")


def budget_rows(budget, total):
    """`fits`: the demand rounded up to a multiple of 4, plus 4.  `cut`: half of it, rounded down to a multiple of 4.  `preset`: the march
    starts at counter[0] = 1000 and needs the demand + 1004."""
    return {"fits": (total + 3) // 4 * 4 + 4, "cut": (total // 2) // 4 * 4, "preset": total + 1004}[budget]


def reference(oracle, grid_name, H, max_steps, N, perturb, budget="fits", degenerate=True, mirrored=False):
    """The oracle's near / far and march (with sample parameters, for the differentiable form) of one case."""
    key = (grid_name, H, max_steps, N, bool(perturb), budget, degenerate, mirrored)
    if key not in _refs:
        bits = grid(grid_name, H)
        o, d = rays(N, degenerate, mirrored)
        nears, fars = oracle.near_far_from_aabb(o, d, AABB, MIN_NEAR)
        march = lambda M, counter=None: oracle.march_rays_train(o, d, BOUND, bits, CASCADES, H, nears, fars, M, perturb, DT_GAMMA, max_steps,  # noqa: E731
                                                                with_ts=True, counter=counter)
        total = int(march(4)[4][0])  # the demand does not depend on the budget: the counter still reports every ray
        M = budget_rows(budget, total)
        base = 1000 if budget == "preset" else 0
        # counter[1] stays zero: the reference indexes its ray records by it, a non-zero value would write past [N, 3]
        xyzs, dirs, deltas, records, counter, ts = march(M, np.array([base, 0], np.int32))
        assert counter.tolist() == [base + total, N] and records[:, 2].sum() == total
        dropped = (records[:, 2] > 0) & (records[:, 1] + records[:, 2] >= M)
        for a in (nears, fars, xyzs, dirs, deltas, ts, records, counter, dropped):
            a.setflags(write=False)
        _refs[key] = Case(grid_name, H, max_steps, N, bool(perturb), budget, mirrored, o, d, nears, fars, M, base, total, xyzs, dirs, deltas, ts, records, counter,
                          dropped)
    return _refs[key]


def stats(case):
    """(samples, rays without a sample, most samples on a ray, rays that stop at max_steps)."""
    per_ray = case.records[:, 2]
    return case.total, int((per_ray == 0).sum()), int(per_ray.max()), int((per_ray == case.max_steps).sum())
