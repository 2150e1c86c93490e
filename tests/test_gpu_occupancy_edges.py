"""GPU: the ten kernels of csrc/occupancy.hip at the C ABI (lib.nerftex_occupancy_*, not through Renderer) against the host model
tests/occupancy_model.py, at the smallest grids where each of their mechanisms can still go wrong.  The model, its cases and the conditions the
cases must meet are checked on the CPU by tests/test_occupancy_model_cpu.py; both modules build their inputs with occupancy_model.cases().

WHY THESE GRID SIZES.  H = 8, 16, 32, 64:
  * the compaction runs H^3 / 256 = 2, 16, 128 and 1024 blocks per cascade, and its block-sum scan walks them in rounds of 256: far below one
    round, inside one round (the scan ends in the middle of it), and four whole rounds with a carry from each to the next;
  * the update runs cascade H^3 / 1024 blocks, from 1 (H = 8, one cascade: half its threads have no cell) to 1280 (H = 64, five cascades: 5 block
    partials per thread of the mean kernel), through 64 and 160 (fewer partials than the mean kernel has threads), 256 (one each) and 768;
  * packbits writes from 64 bytes up.
Cascade counts and bounds (1, 1.0), (2, 1.5), (3, 4.0), (5, 16.0) are spread over the sizes (occupancy_model._SHAPES says what each shape is there
for); bound 1.5 is where min(2^k, bound) cuts the last cascade.  Every cascade of a call has its own occupancy pattern -- all -1, all zero, cell 0
alone, cell H^3 - 1 alone, all positive, exactly the first 256 cells, alternating blocks of 256, 30 % random among zeros and negatives -- so that a
`cas * nblk` or `cas * H^3` that is off shows.  Nothing here needs H = 128: tests/test_gpu_occupancy.py runs there.

Every output buffer has 64 guard elements behind it holding a sentinel (the buffer itself is pre-filled with it as well, so an element that was not
written cannot pass for one that was); every test checks them.
"""
import numpy as np
import pytest
import torch

import occupancy_model as om

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = {torch.float32: -7777.0, torch.int32: -123456789, torch.uint8: 0xA5}
CASES = om.cases()
NAMES = [c.name for c in CASES]
OK, ERR_INVALID = 0, 1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Guarded:
    """n elements followed by GUARD sentinels."""

    def __init__(self, n, dtype, dev, init=None):
        self.n = n
        self.whole = torch.full((n + GUARD,), SENTINEL[dtype], dtype=dtype, device=dev)
        self.t = self.whole[:n]
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init).reshape(-1)))

    def ptr(self):
        return self.whole.data_ptr()

    def numpy(self):
        assert bool((self.whole[self.n:] == SENTINEL[self.whole.dtype]).all()), "a write behind the end of the buffer"
        return self.t.cpu().numpy()


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_floats(got, want):
    return np.array_equal(_bits(got).reshape(-1), _bits(want).reshape(-1))


def _ulps_apart(a, b):
    """Distance of two finite float32 in units in the last place (their ordered integer representations)."""
    ia, ib = (int(np.float32(x).view(np.int32)) for x in (a, b))
    ia, ib = (i if i >= 0 else -(i & 0x7FFFFFFF) for i in (ia, ib))
    return abs(ia - ib)


# ------------------------------------------------------------------------------------------------------------------ the calls
def sample_full(case, dev, noise, seed=0):
    from nerftex_hip import check, lib, stream

    rows = case.cascade * case.H ** 3
    xyzs = Guarded(rows * 3, torch.float32, dev)
    u = None if noise is None else _up(noise, dev)
    check(lib.nerftex_occupancy_sample_full(xyzs.ptr(), case.cascade, case.H, case.bound, None if u is None else u.data_ptr(), seed, stream()))
    return xyzs.numpy().reshape(rows, 3)


def sample_partial(case, dev, N, draw=None, stratified=None, seed=0, with_counts=True, grid=None):
    """draw: explicit picks (through nerftex_occupancy_sample_partial); None: the library's own at `seed` (through .._ordered).  Returns
    (indices [cascade, 2N], xyzs [cascade * 2N, 3], counts or None); density_grid must come back unchanged, bit for bit."""
    from nerftex_hip import check, lib, stream

    grid = case.grid if grid is None else grid
    g = Guarded(grid.size, torch.float32, dev, grid)
    rows = case.cascade * 2 * N
    indices, xyzs = Guarded(rows, torch.int32, dev), Guarded(rows * 3, torch.float32, dev)
    n_occ = Guarded(case.cascade, torch.int32, dev) if with_counts else None
    keep = [_up(a, dev) for a in ((draw.rand_coords, draw.rand_pick, draw.noise) if draw is not None else ())]
    picks = [t.data_ptr() for t in keep] if draw is not None else [None, None, None]
    n_ptr = n_occ.ptr() if with_counts else None
    if stratified is None:
        check(lib.nerftex_occupancy_sample_partial(g.ptr(), case.cascade, case.H, case.bound, N, *picks, seed, indices.ptr(), xyzs.ptr(), n_ptr, stream()))
    else:
        check(lib.nerftex_occupancy_sample_partial_ordered(g.ptr(), case.cascade, case.H, case.bound, N, *picks, seed, indices.ptr(), xyzs.ptr(), n_ptr,
                                                           int(stratified), stream()))
    assert _same_floats(g.numpy(), grid), "the sampler must leave density_grid alone"
    return indices.numpy().reshape(case.cascade, 2 * N), xyzs.numpy().reshape(rows, 3), (n_occ.numpy() if with_counts else None)


def update(case, dev, estimates, indices, decay, force, thresh, grid=None):
    """(grid, mean, thresh, bitfield) as the device leaves them."""
    from nerftex_hip import check, lib, stream

    grid = case.grid if grid is None else grid
    g = Guarded(grid.size, torch.float32, dev, grid)
    mt = Guarded(2, torch.float32, dev)
    bits = Guarded(grid.size // 8, torch.uint8, dev)
    est = _up(estimates, dev)
    idx = None if indices is None else _up(indices, dev)
    rows = case.H ** 3 if indices is None else indices.shape[1]
    check(lib.nerftex_occupancy_update(g.ptr(), est.data_ptr(), None if idx is None else idx.data_ptr(), rows, case.cascade, case.H, decay, force, thresh,
                                       mt.ptr(), bits.ptr(), stream()))
    m = mt.numpy()
    return g.numpy().reshape(grid.shape), m[0], m[1], bits.numpy()


# ------------------------------------------------------------------------------------------------------------------ 1. full-sweep positions
@pytest.mark.parametrize("name", NAMES)
def test_full_sweep_positions(dev, oracle, name):
    case = om.case(name)
    rows = case.cascade * case.H ** 3
    got = sample_full(case, dev, case.full_noise)
    assert _same_floats(got, om.full_positions(case, case.full_noise)), "given jitter: bit-equal to the float32 model"
    exact, b = om.full_positions_float64(case, case.full_noise)
    ratio = float((np.abs(got.astype(np.float64) - exact) / om.position_tolerance(b)).max())
    print(f"{name}: worst |device - float64| / (8 * 2^-24 * b) = {ratio:.4f}")
    assert ratio <= 1.0
    # the library's generator: row r, component d draws counter 3 r + d of `seed`
    u = oracle.counter_uniform01(case.seed, np.arange(rows * 3, dtype=np.uint64)).reshape(rows, 3)
    assert u.min() >= 0 and u.max() < 1
    assert _same_floats(sample_full(case, dev, None, seed=case.seed), om.full_positions(case, u)), "NULL noise: the counter generator"
    # jitter 0.5 everywhere: the cell centres
    half = np.full((rows, 3), 0.5, np.float32)
    centre = sample_full(case, dev, half)
    assert _same_floats(centre, om.full_positions(case, half))
    exact, b = om.full_positions_float64(case, half)
    assert (np.abs(centre.astype(np.float64) - exact) <= om.position_tolerance(b)).all()
    H3 = case.H ** 3
    for k in range(case.cascade):  # a centre is (2 c / (H - 1) - 1) scaled by the cascade's span: Morton cell 0 is the corner at -span, exactly
        bk = min(2.0 ** k, case.bound)
        assert (centre[k * H3] == -np.float32(bk - bk / case.H)).all()


# ------------------------------------------------------------------------------------------------------------------ 2. occupied lists and counts
@pytest.mark.parametrize("name", NAMES)
def test_occupied_lists_and_counts(dev, name):
    case = om.case(name)
    lists, counts = om.occupied_lists(case)
    label = "list" if "list" in case.draws else case.update_draw
    draw = case.draws[label]
    indices, xyzs, n_occ = sample_partial(case, dev, draw.N, draw)
    assert n_occ.tolist() == counts.tolist()
    again, xyzs2, none = sample_partial(case, dev, draw.N, draw, with_counts=False)
    assert none is None and np.array_equal(indices, again) and _same_floats(xyzs, xyzs2), "n_occupied == NULL: the counts live in the scratch"
    if label == "list":  # rand_pick = arange over the whole list (N = H^3 >= its length): the second half IS the list
        for k in range(case.cascade):
            n = int(counts[k])
            second = indices[k, draw.N:]
            if n == 0:
                assert (second == -1).all()
            else:
                assert np.array_equal(second[:n], lists[k, :n]) and (second[n:] == lists[k, n - 1]).all()
                assert (np.diff(second[:n]) > 0).all()


# ------------------------------------------------------------------------------------------------------------------ 3. explicit picks
@pytest.mark.parametrize("name,label", [(c.name, label) for c in CASES for label in c.draws])
def test_partial_rows_with_explicit_picks(dev, name, label):
    case = om.case(name)
    draw = case.draws[label]
    want_idx, want_xyz, counts = om.partial_rows(case, draw)
    indices, xyzs, n_occ = sample_partial(case, dev, draw.N, draw)
    assert n_occ.tolist() == counts.tolist()
    assert np.array_equal(indices, want_idx)
    assert _same_floats(xyzs, want_xyz)
    for k in range(case.cascade):
        if counts[k] == 0:
            rows = slice(k * 2 * draw.N + draw.N, (k + 1) * 2 * draw.N)
            assert (indices[k, draw.N:] == -1).all() and (_bits(xyzs[rows]) == 0).all(), "no occupied cell: index -1, position +0"


# ------------------------------------------------------------------------------------------------------------------ 4. the library's own draws
@pytest.mark.parametrize("name,N,stratified", [(c.name, N, s) for c in CASES for N in c.library_N for s in (1, 0)])
def test_library_draws(dev, name, N, stratified):
    case = om.case(name)
    want_idx, want_xyz, counts = om.library_rows(case, N, bool(stratified))
    indices, xyzs, n_occ = sample_partial(case, dev, N, None, stratified=stratified, seed=case.seed)
    assert n_occ.tolist() == counts.tolist()
    assert np.array_equal(indices, want_idx)
    assert _same_floats(xyzs, want_xyz)
    if not stratified:  # the unordered entry point is the ordered one with stratified = 0
        plain = sample_partial(case, dev, N, None, stratified=None, seed=case.seed)
        assert np.array_equal(plain[0], indices) and _same_floats(plain[1], xyzs)


# ------------------------------------------------------------------------------------------------------------------ 5. update
def _check_update(case, got, want, thresh, what):
    """Returns the distance in ulps between the device's mean and the model's."""
    grid, mean, th, bits = got
    want_grid, want_mean, want_th, want_bits = want
    wrong = np.nonzero(_bits(grid).reshape(-1) != _bits(want_grid).reshape(-1))[0]
    assert wrong.size == 0, (what, f"{wrong.size} cells differ, the first at {wrong[:4].tolist()}: device {grid.reshape(-1)[wrong[:4]].tolist()}, "
                             f"model {want_grid.reshape(-1)[wrong[:4]].tolist()}, before {case.grid.reshape(-1)[wrong[:4]].tolist()}")
    apart = _ulps_apart(mean, want_mean)
    assert apart <= 1, (what, float(mean), float(want_mean))
    assert _bits(th) == _bits(min(np.float32(mean), np.float32(thresh))), (what, "threshold = min(the device's own mean, density_thresh)")
    assert np.array_equal(bits, want_bits), what  # every byte: the CPU module keeps every cell 2 ulps clear of the mean
    return apart


@pytest.mark.parametrize("mode", ["full", "partial"])
@pytest.mark.parametrize("name", NAMES)
def test_update(dev, name, mode):
    case = om.case(name)
    draw = case.draws[case.update_draw]
    indices = om.partial_rows(case, draw)[0] if mode == "partial" else None
    moved = 0
    for v in om.variants():
        if v[0] != mode:
            continue
        _, decay, force, thresh = v
        est = draw.estimates if mode == "partial" else (case.full_estimates_forced if force else case.full_estimates)
        got = update(case, dev, est, indices, decay, force, thresh)
        moved += _check_update(case, got, om.update_variant(case, *v), thresh, (name,) + v)
    print(f"{name} {mode}: device mean one float32 ulp from the exact one in {moved} of 8 variants")


# ------------------------------------------------------------------------------------------------------------------ 6. scratch reuse
def _everything(case, dev):
    """One partial update and one full sweep, each from the case's prior grid; every output."""
    draw = case.draws[case.update_draw]
    indices, xyzs, n_occ = sample_partial(case, dev, draw.N, draw)
    part = update(case, dev, draw.estimates, indices, 0.95, 0, om.THRESH_HIGH)
    lib_rows = sample_partial(case, dev, draw.N if (case.H ** 3) % draw.N == 0 else 1, None, stratified=1, seed=case.seed)
    pos = sample_full(case, dev, None, seed=case.seed)
    full = update(case, dev, case.full_estimates, None, 0.95, 0, om.THRESH_HIGH)
    return [indices, xyzs, n_occ, *part, lib_rows[0], lib_rows[1], pos, *full]


def _identical(a, b):
    """Byte for byte, whatever the type (a NaN or the sign of a zero counts)."""
    raw = lambda x: np.ascontiguousarray(x).reshape(-1).view(np.uint8)  # noqa: E731
    return len(a) == len(b) and all(np.array_equal(raw(x), raw(y)) for x, y in zip(a, b))


def test_small_after_large_on_the_same_scratch(dev):
    """The scratch only grows: the smallest case, then the largest, then the smallest again -- what the large call left behind (block sums, lists,
    block partials, a tmp grid) must not reach the small one's results."""
    small, large = CASES[0], CASES[-1]
    assert small.cascade * small.H ** 3 == 512 and large.cascade * large.H ** 3 == 5 * 64 ** 3
    first = _everything(small, dev)
    big = _everything(large, dev)
    third = _everything(small, dev)
    assert _identical(first, third)
    assert _identical(big, _everything(large, dev))


@pytest.mark.parametrize("name", NAMES[1:-1])
def test_a_repeat_gives_the_same_bits(dev, name):
    case = om.case(name)
    assert _identical(_everything(case, dev), _everything(case, dev))


# ------------------------------------------------------------------------------------------------------------------ 7. refused shapes
def _refusal(rc):
    from nerftex_hip import lib

    return rc, lib.nerftex_last_error().decode()


def test_refused_shapes_launch_nothing():
    """Only calls that cannot reach a kernel, whatever check_shape says: N = 0 with null buffers returns before the first launch.  A grid size that
    is no power of two (Morton indices run past H^3) and a cell count of 2^32 are refused; H = 64 with 5 cascades stays."""
    from nerftex_hip import lib

    def shape(cascade, H):
        return _refusal(lib.nerftex_occupancy_sample_partial_ordered(None, cascade, H, 2.0, 0, None, None, None, 0, None, None, None, 0, None))

    rc, msg = shape(1, 24)
    assert rc == ERR_INVALID and "power of two" in msg
    for H in (12, 40, 96, 1000, 4, 2048, 0):
        assert shape(1, H)[0] == ERR_INVALID, H
    rc, msg = shape(4, 1024)
    assert rc == ERR_INVALID and "32-bit" in msg
    for cascade in (5, 8):
        assert shape(cascade, 1024)[0] == ERR_INVALID
    assert shape(3, 1024) == (OK, "") and shape(8, 512) == (OK, "")
    assert shape(5, 64) == (OK, "")
    for H in (8, 16, 32, 64, 128, 256, 512, 1024):
        assert shape(1, H)[0] == OK, H
    assert shape(0, 64)[0] == ERR_INVALID and shape(9, 64)[0] == ERR_INVALID


def test_refused_row_counts_launch_nothing():
    """cascade * 2 N and cascade * rows_per_cascade of 2^32 and more.  These calls end in a refusal on every path: the stratified draw refuses an N
    that does not divide H^3, and the update refuses a NULL mean_thresh, both before anything is allocated or launched -- the row check comes first
    and is told from them by its message."""
    from nerftex_hip import lib

    def partial(cascade, N):
        return _refusal(lib.nerftex_occupancy_sample_partial_ordered(None, cascade, 8, 2.0, N, None, None, None, 0, None, None, None, 1, None))

    def upd(cascade, rows):
        return _refusal(lib.nerftex_occupancy_update(None, None, None, rows, cascade, 8, 0.95, 0, 10.0, None, None, None))

    rc, msg = partial(8, 2 ** 28 + 1)  # 8 * 2 * (2^28 + 1) > 2^32
    assert rc == ERR_INVALID and "32-bit row index" in msg
    rc, msg = partial(8, 2 ** 28 - 1)  # fits: the stratified rule refuses it
    assert rc == ERR_INVALID and "divide" in msg
    rc, msg = partial(1, 2 ** 31 + 1)
    assert rc == ERR_INVALID and "32-bit row index" in msg
    rc, msg = upd(8, 2 ** 29)
    assert rc == ERR_INVALID and "32-bit row index" in msg
    rc, msg = upd(8, 2 ** 29 - 1)
    assert rc == ERR_INVALID and "mean_thresh" in msg
