"""CPU: the cases of tests/march_cases.py exercise what they name -- asserted with the oracle alone, so that the premises of
tests/test_gpu_march_paths.py are checked without a GPU.

What matters at each grid size H (N = 97 rays, bound 2, C = 2, dt_gamma = 1 / 128):
  * `ones`, max_steps 1024: the longest ray has 383 samples at H = 128 (three kMcSeg = 128 segments of the data-parallel count pass), 393 at
    H = 256 (a fourth segment) and 487 at H = 512 (where the dispatch has left that pass);
  * `ones`, max_steps 160: most rays stop at the cap, inside a later segment;
  * `ones`, max_steps 32: dt_min > dt_max;
  * `scene` under the `cut` budget: rays with samples land on both sides of the drop rule;
  * `zeros`: no sample on any ray;
  * no Morton index a case can produce reaches C * H^3.
"""
import numpy as np
import pytest

import march_cases as mc

FLT_MAX = np.float32(3.402823466e38)

# oracle, N = 97, perturb off: (samples, rays without a sample, most samples on a ray, rays that stop at max_steps)
# ... of scene.train_batch(97, seed=5) as it comes
PLAIN_97 = {
    ("ones", 1024): {128: (35170, 0, 383, 0), 256: (35481, 0, 393, 0), 512: (42084, 0, 487, 0)},
    ("ones", 160): {128: (15512, 0, 160, 89), 256: (15519, 0, 160, 96), 512: (15520, 0, 160, 97)},
    ("ones", 32): {128: (3104, 0, 32, 97), 256: (3104, 0, 32, 97), 512: (3104, 0, 32, 97)},
}
# ... and of the cases' rays: the same with six degenerate rays over the first six, two of which miss the box
CASES_97 = {
    ("ones", 1024): {128: (33870, 2, 383, 0), 256: (34174, 2, 393, 0), 512: (40542, 2, 487, 0)},
    ("ones", 160): {128: (14982, 2, 160, 84), 256: (14991, 2, 160, 92), 512: (15043, 2, 160, 94)},
    ("ones", 32): {128: (3009, 2, 32, 94), 256: (3010, 2, 32, 94), 512: (3011, 2, 32, 94)},
    ("alternate", 1024): {128: (16781, 2, 200, 0), 256: (17252, 2, 353, 0), 512: (20485, 2, 408, 0)},
    ("scene", 1024): {128: (6306, 19, 150, 0), 256: (6312, 19, 149, 0), 512: (6947, 19, 163, 0)},
    ("zeros", 1024): {128: (0, 97, 0, 0), 256: (0, 97, 0, 0), 512: (0, 97, 0, 0)},
}
# `scene`, N = 97, perturb on, `cut` budget: (rays with samples that are dropped, rays with samples that are kept)
PLAIN_CUT_97 = {128: (41, 42), 256: (41, 42), 512: (40, 43)}
CASES_CUT_97 = {128: (39, 39), 256: (39, 39), 512: (39, 39)}


def test_grid_sizes_are_powers_of_two_and_every_morton_index_stays_inside_the_bitfield(oracle):
    rng = np.random.default_rng(0)
    for H in mc.SIZES:
        assert mc.is_pow2(H) and H <= 1024  # (the Morton code interleaves 10 bits per coordinate)
        corners = np.array([[a, b, c] for a in (0, H - 1) for b in (0, H - 1) for c in (0, H - 1)], np.int32)
        coords = np.concatenate([corners, rng.integers(0, H, size=(4096, 3), dtype=np.int32)])
        codes = oracle.morton3D(coords).astype(np.int64)
        assert codes.min() == 0 and codes.max() == H ** 3 - 1  # the far corner has the largest code of the grid
        # the march reads bit level * H^3 + code with level <= C - 1 and coordinates clamped to [0, H - 1]
        assert (mc.CASCADES - 1) * H ** 3 + int(codes.max()) < mc.CASCADES * H ** 3
        for name in mc.GRIDS:
            assert mc.grid(name, H).size * 8 == mc.CASCADES * H ** 3


def test_scene_grid_is_the_bitfield_of_the_harness_scene():
    from ngp_harness import scene

    assert np.array_equal(mc.scene_bitfield(128), scene.Scene(bound=mc.BOUND, seed=1).bitfield(128)[2])
    for H in mc.SIZES:  # partly occupied in both cascades
        per_cascade = np.unpackbits(mc.grid("scene", H)).reshape(mc.CASCADES, -1).mean(1)
        assert (per_cascade > 0.01).all() and (per_cascade < 0.5).all()


def test_batches_are_ragged_where_the_kernels_care():
    for N in (31, 65):
        assert 1 <= N % 64 <= 32  # the expand pass's last 64-ray block has a second total word that no 32-ray count workgroup wrote
    assert -(-97 // 64) == 2 and -(-97 // 32) == 4 and 97 % 32 != 0
    assert mc.BATCHES == (31, 65, 97)


def test_degenerate_rays_are_what_they_are_named(oracle):
    for N in mc.BATCHES:
        c = mc.reference(oracle, "ones", 128, 1024, N, False)
        assert c.o.shape == (N, 3) and (c.d[0] == [0, 0, -1]).all() and (c.d[1] == [1, 0, 0]).all()
        assert c.nears[3] == np.float32(mc.MIN_NEAR)  # starts inside the box
        assert c.fars[4] < 0 < c.nears[4]  # the box lies behind the ray: far < near, no step is taken
        assert c.nears[5] == FLT_MAX and c.fars[5] == FLT_MAX  # misses the box
        assert c.records[4, 2] == 0 and c.records[5, 2] == 0 and (c.records[:4, 2] > 0).all()


@pytest.mark.parametrize("H", [256, 512])
def test_both_direction_signs_walk_the_upper_half_of_every_axis(oracle, H):
    """A ray that moves up an axis leaves a voxel through its upper face: if a top coordinate bit is lost on the way to that face, the exit comes
    out behind the ray and the skip merely ends at the next member -- no sample changes.  Only a ray that moves DOWN an axis, in the half where
    that bit is set, jumps too far.  A batch of one view need not have such rays on every axis; with its mirror image it has -- on the grids
    where rays skip."""
    for name in ("scene", "alternate"):
        up_in_upper_half, down_in_upper_half = np.zeros(3, np.int64), np.zeros(3, np.int64)
        for mirrored in (False, True):
            c = mc.reference(oracle, name, H, 1024, 97, True, mirrored=mirrored)
            x, d = c.xyzs[:c.total], c.dirs[:c.total]
            assert c.total > 5000
            up_in_upper_half += ((x > 0) & (d > 0)).sum(0)
            down_in_upper_half += ((x > 0) & (d < 0)).sum(0)
        assert up_in_upper_half.min() > 500 and down_in_upper_half.min() > 500, name
    mirrored = mc.reference(oracle, "ones", H, 1024, 97, True, mirrored=True)
    assert mc.stats(mirrored)[2] > 384 and np.array_equal(mirrored.o, -mc.rays(97)[0]) and np.array_equal(mirrored.d, -mc.rays(97)[1])


@pytest.mark.parametrize("H", mc.SIZES)
def test_oracle_statistics_are_pinned(oracle, H):
    for (name, max_steps), want in PLAIN_97.items():
        assert mc.stats(mc.reference(oracle, name, H, max_steps, 97, False, degenerate=False)) == want[H], (name, max_steps)
    for (name, max_steps), want in CASES_97.items():
        assert mc.stats(mc.reference(oracle, name, H, max_steps, 97, False)) == want[H], (name, max_steps)


@pytest.mark.parametrize("perturb", [False, True])
def test_the_fourth_segment_is_reached_from_256_cells_on(oracle, perturb):
    """tests/test_gpu_march_walk.py relies on "no ray has more than 384 sequence members" at H = 128; that does not hold above."""
    most = {H: mc.stats(mc.reference(oracle, "ones", H, 1024, 97, perturb))[2] for H in mc.SIZES}
    assert most[128] < 384 < most[256] < most[512]


@pytest.mark.parametrize("H", mc.SIZES)
def test_the_cap_falls_inside_a_later_segment(oracle, H):
    for perturb in (False, True):
        c = mc.reference(oracle, "ones", H, 160, 97, perturb)
        at_cap = mc.stats(c)[3]
        assert at_cap >= 84 and 128 < c.max_steps < 256  # the cap of most rays lies in the second segment
        assert c.records[:, 2].max() == 160 and at_cap < 97  # ... and some rays end before it


@pytest.mark.parametrize("H", mc.SIZES)
def test_32_steps_is_the_case_of_dt_min_above_dt_max(oracle, H):
    dt_min = np.float32(2 * np.sqrt(3)) / np.float32(32)
    dt_max = np.float32(2 * np.sqrt(3)) * np.float32(1 << (mc.CASCADES - 1)) / np.float32(H)
    assert dt_min > dt_max
    for perturb in (False, True):
        c = mc.reference(oracle, "ones", H, 32, 97, perturb)
        assert mc.stats(c)[3] == 94
        with_samples = c.records[:, 2] > 0
        assert (c.deltas[:c.total, 0] == dt_max).all() and with_samples.sum() >= 94  # every step is dt_max whatever t is


@pytest.mark.parametrize("H", mc.SIZES)
def test_cut_budget_drops_some_rays_and_keeps_others(oracle, H):
    for degenerate, pinned in ((False, PLAIN_CUT_97), (True, CASES_CUT_97)):
        c = mc.reference(oracle, "scene", H, 1024, 97, True, "cut", degenerate)
        with_samples = c.records[:, 2] > 0
        dropped, kept = int(c.dropped.sum()), int((with_samples & ~c.dropped).sum())
        assert (dropped, kept) == pinned[H]
        assert c.M == (c.total // 2) // 4 * 4 and c.counter[0] == c.total  # the counter still reports the whole demand
    # every cut case of the GPU module has rays on both sides, at least a quarter of those with samples on each
    for name, max_steps in (("scene", 1024), ("ones", 1024), ("ones", 160), ("ones", 32), ("alternate", 1024)):
        for N in mc.BATCHES:
            for perturb in (False, True):
                c = mc.reference(oracle, name, H, max_steps, N, perturb, "cut")
                with_samples = int((c.records[:, 2] > 0).sum())
                dropped = int(c.dropped.sum())
                assert 4 * dropped >= with_samples and 4 * (with_samples - dropped) >= with_samples, (name, max_steps, N, perturb)
                rows = np.zeros(c.M, bool)  # the rows of the kept rays, and nothing else, hold samples
                for _, off, cnt in c.records[(c.records[:, 2] > 0) & ~c.dropped]:
                    rows[off:off + cnt] = True
                assert (c.deltas[rows, 0] > 0).all() and not c.deltas[~rows].any() and not c.xyzs[~rows].any()


@pytest.mark.parametrize("H", mc.SIZES)
def test_budgets_come_from_the_oracles_demand(oracle, H):
    for name in ("scene", "ones"):
        fits = mc.reference(oracle, name, H, 1024, 97, True, "fits")
        assert fits.M % 4 == 0 and fits.total + 4 <= fits.M < fits.total + 8 and not fits.dropped.any()
        pre = mc.reference(oracle, name, H, 1024, 97, True, "preset")
        assert pre.base == 1000 and pre.M == pre.total + 1004 and not pre.dropped.any()
        assert pre.counter.tolist() == [1000 + pre.total, 97] and pre.records[0, 1] == 1000
        assert np.array_equal(pre.records[:, 1] - 1000, fits.records[:, 1]) and not pre.xyzs[:1000].any()
        assert np.array_equal(pre.xyzs[1000:1000 + pre.total], fits.xyzs[:fits.total])


@pytest.mark.parametrize("H", mc.SIZES)
def test_empty_grid_gives_no_sample(oracle, H):
    for N in mc.BATCHES:
        c = mc.reference(oracle, "zeros", H, 1024, N, True)
        assert c.total == 0 and not c.records[:, 2].any() and not c.records[:, 1].any() and c.M == 4
        assert not c.xyzs.any() and not c.deltas.any()


def test_references_are_shared_and_read_only(oracle):
    a = mc.reference(oracle, "ones", 256, 1024, 97, True)
    assert a is mc.reference(oracle, "ones", 256, 1024, 97, True)
    for arr in (a.o, a.d, a.nears, a.fars, a.xyzs, a.dirs, a.deltas, a.ts, a.records, a.counter, mc.grid("ones", 256)):
        assert not arr.flags.writeable
