"""CPU: tests/occupancy_model.py is right, and its cases can tell a wrong kernel from a right one.

  * for every case the model's positions, grid, mean and bitfield equal a torch-CPU restatement of the reference's op sequence
    (nerf/renderer.py:592-601 and 639-654, as _cell_positions and _finish of tests/test_gpu_occupancy.py spell it out) on the same numbers;
  * the conditions on the inputs that the GPU comparison leans on (nothing near the threshold, every planted row where it has to be,
    every cascade count and occupancy pattern present) are asserted HERE, where no device is involved;
  * eleven ways of getting the operation subtly wrong (mutants of the model) each change at least one case's expected output.
"""
import math

import numpy as np
import pytest
import torch

import occupancy_model as om

f32 = np.float32
CASES = om.cases()
NAMES = [c.name for c in CASES]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same(a, b):
    """Bit for bit (float arrays by their bit patterns, so that NaN and the sign of zero count)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype == f32 and b.dtype == f32:
        return bool(np.array_equal(_bits(a), _bits(b)))
    return bool(np.array_equal(a, b))


# ------------------------------------------------------------------------------------------ every output of a case, lazily and in a fixed order
def outputs(case, model):
    """(key, arrays) for everything the GPU module compares: cheap things first."""
    lists, counts = om.occupied_lists(case, model)
    yield "lists", (lists, counts)
    for label, draw in case.draws.items():
        yield f"rows/{label}", om.partial_rows(case, draw, model)[:2]
    for N in case.library_N:
        for stratified in (True, False):
            yield f"library/{N}/{int(stratified)}", om.library_rows(case, N, stratified, model)[:2]
    yield "full", (om.full_positions(case, case.full_noise, model),)
    for v in om.variants():
        yield "update/%s/%g/%d/%g" % v, om.update_variant(case, *v, model=model)


_BASE = {}


def base(case):
    if case.name not in _BASE:
        _BASE[case.name] = dict(outputs(case, om.MODEL))
    return _BASE[case.name]


# ------------------------------------------------------------------------------------------ the reference's op sequence in torch on the CPU
def _torch_positions(case, coords, k, u):
    """renderer.py:592-601 with the jitter given (tests/test_gpu_occupancy.py: _cell_positions)."""
    H = case.H
    xyzs = 2 * torch.from_numpy(coords).float() / (H - 1) - 1
    bound = min(2 ** k, case.bound)
    half = bound / H
    cas_xyzs = xyzs * (bound - half)
    cas_xyzs += (torch.from_numpy(u) * 2 - 1) * half
    return cas_xyzs.numpy()


def _torch_finish(grid, tmp, decay, force_full_grid, density_thresh):
    """renderer.py:644-654 on explicit tensors (tests/test_gpu_occupancy.py: _finish), packbits spelled out; the mean in float64."""
    valid = (grid >= 0) & (tmp >= 0)
    if force_full_grid:
        valid = torch.ones_like(valid)
    grid = grid.clone()
    grid[valid] = torch.maximum(grid[valid] * decay, tmp[valid])
    mean64 = grid.clamp(min=0).double().mean().item()
    mean32 = torch.mean(grid.clamp(min=0)).item()
    return grid, mean64, mean32


def _pack(grid, thresh):
    weights = (1 << np.arange(8)).astype(np.uint32)
    return ((grid.reshape(-1, 8) > f32(thresh)) * weights).sum(1).astype(np.uint8)


def _check_positions(case, got, coords, k, u, what):
    """Bit-equal to torch, except where torch's true division by the Python scalar H - 1 on the CPU rounds differently from the multiplication by
    the float32 reciprocal that a GPU (and the model) does: there the torch result is held to the float64 bound of occupancy_model instead."""
    want = _torch_positions(case, coords, k, u)
    differs = _bits(got) != _bits(want)
    b = min(2.0 ** k, case.bound)
    exact, _ = om.position_float64(case.H, coords, b, u)
    tol = om.position_tolerance(b)
    assert np.abs(got.astype(np.float64) - exact).max() <= tol, what
    if differs.any():
        assert np.abs(want.astype(np.float64) - exact)[differs].max() <= tol, what
        assert np.abs(got.astype(np.float64) - want.astype(np.float64))[differs].max() <= 2 * tol, what
    return float(differs.mean())


@pytest.mark.parametrize("name", NAMES)
def test_positions_equal_the_reference_op_sequence(name, oracle):
    case = om.case(name)
    H3 = case.H ** 3
    coords = om.morton_coords(case.H)
    got = base(case)["full"][0]
    worst = 0.0
    for k in range(case.cascade):
        worst = max(worst, _check_positions(case, got[k * H3:(k + 1) * H3], coords, k, case.full_noise[k * H3:(k + 1) * H3], f"full sweep, cascade {k}"))
    for label, draw in case.draws.items():
        indices, xyzs = base(case)[f"rows/{label}"]
        R = 2 * draw.N
        for k in range(case.cascade):
            occ = torch.nonzero(torch.from_numpy(case.grid[k]) > 0).squeeze(-1)
            uni = torch.from_numpy(oracle.morton3D(draw.rand_coords[k])).long()
            if occ.numel() == 0:  # renderer.py:617
                assert (indices[k, draw.N:] == -1).all() and not xyzs[k * R + draw.N:(k + 1) * R].any()
                want_idx, rows = uni, slice(k * R, k * R + draw.N)
            else:
                want_idx, rows = torch.cat([uni, occ[torch.from_numpy(draw.rand_pick[k]).long()]]), slice(k * R, (k + 1) * R)
            n = want_idx.numel()
            assert np.array_equal(indices[k, :n], want_idx.numpy())
            cc = oracle.morton3D_invert(want_idx.numpy().astype(np.int32))
            _check_positions(case, xyzs[rows], cc, k, draw.noise[rows], f"draw {label}, cascade {k}")
    assert worst < 0.5, "the reciprocal and the division agree on most cells"


@pytest.mark.parametrize("name", NAMES)
def test_update_equals_the_reference_op_sequence(name, oracle):
    case = om.case(name)
    H3 = case.H ** 3
    grid0 = torch.from_numpy(case.grid)
    draw = case.draws[case.update_draw]
    indices = base(case)[f"rows/{case.update_draw}"][0]
    for v in om.variants():
        mode, decay, force, thresh = v
        if mode == "full":
            tmp = torch.from_numpy(case.full_estimates_forced if force else case.full_estimates).view(case.cascade, H3).clone()
        else:
            tmp = -torch.ones_like(grid0)
            est = torch.from_numpy(draw.estimates).view(case.cascade, -1)
            for k in range(case.cascade):
                idx = torch.from_numpy(indices[k]).long()
                keep = idx >= 0  # renderer.py:617: a cascade without occupied cells has no second half
                # a cell named twice: the larger estimate (tests/test_gpu_occupancy.py).  A NaN row is left out: it never lands (amax would let
                # it bury the cell's other estimates); a negative one needs no such care, amax(-1, negative) is -1
                e = est[k][keep]
                ok = ~torch.isnan(e)
                tmp[k].scatter_reduce_(0, idx[keep][ok], e[ok], "amax", include_self=True)
        want_grid, mean64, mean32 = _torch_finish(grid0, tmp, decay, bool(force), thresh)
        grid, mean, th, bits = base(case)["update/%s/%g/%d/%g" % v]
        assert _same(grid, want_grid.numpy()), v
        assert abs(float(mean) - mean64) <= abs(mean64) * 2.0 ** -23, v
        assert abs(float(mean) - mean32) <= 2e-6 * abs(mean64), v  # the framework's fp32 tree, as tests/test_gpu_occupancy.py allows
        assert th == min(mean, f32(thresh))
        assert np.array_equal(bits, _pack(grid, th)), v


def test_exact_mean_is_fsum():
    for case in CASES[:8]:
        for g in (case.grid, base(case)["update/full/0.95/1/%g" % om.THRESH_HIGH][0]):
            want = f32(math.fsum(np.maximum(g.reshape(-1), 0).astype(np.float64).tolist()) / g.size)
            assert om.exact_mean(g) == want


# ------------------------------------------------------------------------------------------ conditions on the inputs
def _ulp(x):
    return float(np.spacing(f32(abs(x))))


@pytest.mark.parametrize("name", NAMES)
def test_no_cell_sits_within_two_ulps_of_the_threshold(name):
    """The device adds its block partials in double in another order: its mean may be the model's neighbour in float32, and that ulp must not move
    a bit.  So no cell of any resulting grid lies within 2 ulps of the mean, unless density_thresh is the smaller of the two by more than that
    (then the mean does not set the threshold).  Also: THRESH_LOW really is below every mean and THRESH_HIGH above."""
    case = om.case(name)
    for v in om.variants():
        grid, mean, th, _ = base(case)["update/%s/%g/%d/%g" % v]
        m = float(mean)
        assert np.isfinite(grid).all() and np.isfinite(m) and m > 0
        assert om.THRESH_LOW < m - 2 * _ulp(m) and m + 2 * _ulp(m) < om.THRESH_HIGH, v
        if v[3] == om.THRESH_HIGH:
            assert th == mean
            assert np.abs(grid.astype(np.float64) - m).min() > 2 * _ulp(m), v
        else:
            assert th == f32(om.THRESH_LOW)


@pytest.mark.parametrize("name", NAMES)
def test_update_draw_names_what_it_has_to(name):
    case = om.case(name)
    draw = case.draws[case.update_draw]
    N = draw.N
    indices = base(case)[f"rows/{case.update_draw}"][0]
    est = draw.estimates.reshape(case.cascade, 2 * N)
    counts = base(case)["lists"][1]
    both = thrice = 0
    for k in range(case.cascade):
        first, second = indices[k, :N], indices[k, N:]
        both += np.intersect1d(first, second[second >= 0]).shape[0]
        cells, times = np.unique(indices[k][indices[k] >= 0], return_counts=True)
        thrice += int((times >= 3).sum())
        if counts[k] == 0:
            assert (second == -1).all() and est[k, N:].max() >= 1e5, "a large estimate on a row whose index is -1"
        else:
            assert 0 in draw.rand_pick[k] and counts[k] - 1 in draw.rand_pick[k], "picks 0 and n - 1"
    assert both >= 1 and thrice >= 1
    assert (est < 0).any() and np.isnan(est).any() and ((est == 0) & ~np.signbit(est)).any()
    # beyond what the issue lists: a -0 estimate (`-0 >= 0`: it lands, the cell is valid and decays), on a row whose cell is occupied
    minus_zero = (est == 0) & np.signbit(est)
    assert minus_zero.any() and all(case.grid[k, indices[k][minus_zero[k]]].min() > 0 for k in range(case.cascade) if minus_zero[k].any())
    for e in (case.full_estimates, case.full_estimates_forced):
        assert (e < 0).any() and ((e == 0) & ~np.signbit(e)).any()
    assert np.isnan(case.full_estimates).any() and not np.isnan(case.full_estimates_forced).any()
    # a NaN that is the only estimate of its cell, a negative one likewise: the cell must stay as it was without force_full_grid
    grid = base(case)["update/partial/0.95/0/%g" % om.THRESH_HIGH][0]
    tmp_named = np.zeros(grid.shape, bool)
    for k in range(case.cascade):
        ok = (indices[k] >= 0) & (est[k] >= 0)
        tmp_named[k, indices[k][ok]] = True
    assert _same(grid[~tmp_named], case.grid[~tmp_named]) and (~tmp_named).any()


def test_the_case_set_covers_the_counts_patterns_and_sizes():
    assert {c.cascade for c in CASES} == {1, 2, 3, 5}
    assert {(c.cascade, c.bound) for c in CASES} == {(1, 1.0), (2, 1.5), (3, 4.0), (5, 16.0)}
    assert {c.H for c in CASES} == {8, 16, 32, 64}
    assert {p for c in CASES for p in c.patterns} == set(om.PATTERNS)
    assert any(len(set(c.patterns)) == c.cascade >= 5 for c in CASES), "different occupancy per cascade within one call"
    assert any((c.cascade * 2 * d.N) % 256 for c in CASES for d in c.draws.values())
    for c in CASES:
        H3 = c.H ** 3
        assert {d.N for d in c.draws.values()} <= {1, 3, H3 // 4, H3}
        if c.H <= 16:
            assert c.draws["list"].N == H3
    assert {n for c in CASES for d in c.draws.values() for n in (d.N,) if n in (1, 3)} == {1, 3}
    # the patterns are what their names say
    for c in CASES:
        H3 = c.H ** 3
        for k, p in enumerate(c.patterns):
            occ = np.nonzero(c.grid[k] > 0)[0]
            want = {"unset": 0, "zero": 0, "first": 1, "last": 1, "full": H3, "first256": 256, "alternate": H3 // 2}.get(p)
            if want is not None:
                assert occ.shape[0] == want, (c.name, p)
            if p == "zero":
                assert not c.grid[k].any()
            if p == "last":
                assert occ[0] == H3 - 1
            if p == "random":
                assert 0.2 * H3 < occ.shape[0] < 0.4 * H3 and (c.grid[k] < 0).any() and (c.grid[k] == 0).any()


# ------------------------------------------------------------------------------------------ sensitivity: mutants of the model
def _compact(grid_c, block_carry, round_carry):
    """The three-pass compaction as the kernels do it -- per-block counts, a scan of them in rounds of 256 blocks, a write at offset + rank --
    with a carry that can be dropped."""
    H3 = grid_c.shape[0]
    flags = grid_c > 0
    counts = flags.reshape(-1, 256).sum(1)
    offs = np.cumsum(counts) - counts
    total = int(counts.sum())
    if not block_carry:  # the first block's count never reaches the blocks behind it
        offs[1:] -= counts[0]
        total -= int(counts[0])
    if not round_carry:  # each round of 256 blocks starts from zero
        start = offs[(np.arange(offs.shape[0]) // 256) * 256]
        offs = offs - start
        total -= int(start[-1])
    out = np.full(H3, -1, np.int32)
    rank = np.cumsum(flags.reshape(-1, 256), 1) - 1
    m = np.arange(H3).reshape(-1, 256)
    where = (offs[:, None] + rank)[flags.reshape(-1, 256)]
    out[where] = m[flags.reshape(-1, 256)]
    return out, total


class OccupiedIncludesZero(om.Model):
    def occupied(self, grid_c):
        return om.Model.occupied(self, np.where(grid_c >= 0, f32(1), f32(-1)))


class BlockCarryDropped(om.Model):
    def occupied(self, grid_c):
        return _compact(grid_c, False, True)


class RoundCarryDropped(om.Model):
    def occupied(self, grid_c):
        return _compact(grid_c, True, False)


class LastWriteWins(om.Model):
    def scatter(self, tmp_c, idx, est):
        with np.errstate(invalid="ignore"):
            lands = (idx >= 0) & (est >= 0)
        for i, e in zip(idx[lands], est[lands]):
            tmp_c[i] = e


class NegativeZeroDoesNotLand(om.Model):
    """What an integer atomicMax on the bit patterns does when nothing clears the sign: -0.0 is the smallest int, below the fill's -1.0."""

    def scatter(self, tmp_c, idx, est):
        om.Model.scatter(self, tmp_c, idx[~np.signbit(est)], est[~np.signbit(est)])


class MinusOneLandsInCellZero(om.Model):
    def scatter(self, tmp_c, idx, est):
        om.Model.scatter(self, tmp_c, np.maximum(idx, 0), est)


class DecayEverywhere(om.Model):
    def ema(self, grid, tmp, decay, force_full_grid, partial):
        out = om.Model.ema(self, grid, tmp, decay, force_full_grid, partial)
        with np.errstate(invalid="ignore"):
            valid = np.ones(grid.shape, bool) if force_full_grid else (grid >= 0) & (tmp >= 0)
        out[~valid] = grid[~valid] * f32(decay)
        return out


class ForceIgnoredWhenPartial(om.Model):
    def ema(self, grid, tmp, decay, force_full_grid, partial):
        return om.Model.ema(self, grid, tmp, decay, force_full_grid and not partial, partial)


class MeanPerCascade(om.Model):
    def finish(self, grid, density_thresh):
        parts = [om.Model.finish(self, g, density_thresh) for g in grid]
        return parts[0][0], parts[0][1], np.concatenate([p[2] for p in parts])


class ThresholdInclusive(om.Model):
    def finish(self, grid, density_thresh):
        mean, thresh, _ = om.Model.finish(self, grid, density_thresh)
        return mean, thresh, np.packbits(grid.reshape(-1) >= thresh, bitorder="little")


class BoundDoesNotCut(om.Model):
    def cascade_consts(self, cascade, H, bound):
        return om.Model.cascade_consts(self, cascade, H, float(2 ** cascade))


MUTANTS = [OccupiedIncludesZero, BlockCarryDropped, RoundCarryDropped, LastWriteWins, NegativeZeroDoesNotLand, MinusOneLandsInCellZero, DecayEverywhere,
           ForceIgnoredWhenPartial, MeanPerCascade, ThresholdInclusive, BoundDoesNotCut]


def test_the_simulated_compaction_with_its_carries_is_the_model():
    for case in CASES[:10]:
        for k in range(case.cascade):
            a, b = om.MODEL.occupied(case.grid[k]), _compact(case.grid[k], True, True)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m.__name__)
def test_every_mutant_changes_some_expected_output(mutant):
    seen = []
    for case in CASES:
        want = base(case)
        for key, got in outputs(case, mutant()):
            if not all(_same(a, b) for a, b in zip(got, want[key])):
                seen.append((case.name, key))
                break
        if seen:
            break
    assert seen, f"no case can tell {mutant.__name__} from the model: add one"
    print(mutant.__name__, "seen by", seen[0])
