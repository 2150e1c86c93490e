"""GPU: every kernel combination and entry form of the training march (csrc/raymarching.hip, march_train_impl), at the grid sizes where its
dispatch and its packed voxel change, bit for bit against the oracle.

    path      count pass                           write pass                              chosen by
    default   march_count_parallel_kernel<false>   march_expand_kernel, two totals a block  nothing set, H <= 256
    lean      march_count_parallel_kernel<true>    march_expand_kernel, two totals a block  march_lean = 1, H <= 256
    serial    march_count_kernel with a log        march_expand_kernel, one total a block   march_serial = 1 -- or H > 256 with nothing set
    replay    march_count_kernel without a log     march_write_kernel                       march = 1

Forms: plain (nerftex_march_rays_train), differentiable (nerftex_march_rays_train_differentiable: + the samples' parameters) and fresh
(nerftex_march_rays_train_fresh: near / far computed by the march, garbage in the counter, NaN in the sample buffers; where the data-parallel
count pass is not taken, behind a prologue of near_far_kernel + zero_words_kernel).

H = 256 is the last size of the data-parallel pass: its packed voxel holds 8-bit coordinates, and coordinates >= 128 use the top bit of each;
its longest rays need a fourth 128-member segment.  H = 512 switches to the serial count pass by itself.  The cases and what each of them
exercises: tests/march_cases.py, asserted on the CPU by tests/test_march_paths_cases_cpu.py.  Everything is compared for EXACT equality:
counter, ray records, every sample row as uint32 -- the rows behind the total and the rows of the rays a `cut` budget drops are zero on both
sides.  Each test asserts that the kernels of its path, and no others, were launched (the library's kernel timers) and what the knobs hold.
"""
import numpy as np
import pytest
import torch

import march_cases as mc

pytestmark = pytest.mark.gpu

PATHS = {"default": {}, "lean": {"march_lean": 1}, "serial": {"march_serial": 1}, "replay": {"march": 1}}
FORMS = ("plain", "differentiable", "fresh")
STEPS = {"scene": (1024,), "ones": (1024, 160, 32), "alternate": (1024,), "zeros": (1024,)}
SENTINEL = -7.0  # in the rows in front of a preset counter: nobody may touch them
MARCH_KERNELS = {"march_count_parallel_kernel", "march_count_kernel", "march_expand_kernel", "march_write_kernel", "near_far_kernel", "zero_words_kernel"}


def _paths_at(H):
    return ("default", "replay") if H == 512 else tuple(PATHS)  # (above 256 cells the two knobs of the count pass select nothing)


def _kernels_of(path, form, H):
    parallel = path in ("default", "lean") and H <= 256
    if parallel:
        # (the fresh form is folded into these two.  The timer has ONE name for both instances of the count pass: that march_lean = 1 ran the
        # <true> one is shown by nerftex_tune_get in _select and by march_train_impl, which launches it exactly when that knob is set)
        return {"march_count_parallel_kernel", "march_expand_kernel"}
    names = {"march_count_kernel", "march_write_kernel" if path == "replay" else "march_expand_kernel"}
    return names | ({"near_far_kernel", "zero_words_kernel"} if form == "fresh" else set())


class _Device:
    """Grids and rays on the device, uploaded once per module."""

    def __init__(self, dev):
        self.dev, self.held = dev, {}

    def put(self, key, make):
        if key not in self.held:
            self.held[key] = torch.from_numpy(np.array(make())).to(self.dev)
        return self.held[key]

    def grid(self, name, H):
        return self.put(("grid", name, H), lambda: mc.grid(name, H))

    def rays(self, N, mirrored=False):
        return self.put(("o", N, mirrored), lambda: mc.rays(N, mirrored=mirrored)[0]), self.put(("d", N, mirrored), lambda: mc.rays(N, mirrored=mirrored)[1])

    def aabb(self):
        return self.put("aabb", lambda: mc.AABB)


@pytest.fixture(scope="module")
def data():
    assert torch.cuda.is_available()
    d = _Device(torch.device("cuda:0"))
    yield d
    d.held.clear()


def _select(knobs, path):
    """Set all three knobs of the dispatch (the ones a path does not name to 0) and check what the library holds."""
    from nerftex_hip import lib

    want = {"march": 0, "march_lean": 0, "march_serial": 0, **PATHS[path]}
    knobs(**want)
    assert {k: lib.nerftex_tune_get(k.encode()) for k in want} == want


class _Launch:
    """One call of a C entry on the current stream.  Building it allocates, fills and uploads the tensors of the call (the uploads wait for the
    stream); run() is the library call alone and waits for nothing."""

    def __init__(self, data, form, case):
        from nerftex_hip import check, lib, ptr, stream

        dev, N, M = data.dev, case.N, case.M
        self.form, self.case = form, case
        self.o, self.d = data.rays(N, case.mirrored)
        self.bits = data.grid(case.grid_name, case.H)
        fresh = form == "fresh"
        assert M > 0 and (M % 4 == 0 or not fresh) and (case.base == 0 or not fresh)
        self.flat = torch.full((M * 8,), float("nan"), device=dev) if fresh else torch.zeros(M * 8, device=dev)
        self.xyzs, self.dirs, self.deltas = self.flat[:3 * M].view(M, 3), self.flat[3 * M:6 * M].view(M, 3), self.flat[6 * M:].view(M, 2)
        self.ts = torch.zeros(M, 1, device=dev) if form == "differentiable" else None
        for a in (self.xyzs, self.dirs, self.deltas, self.ts):
            if a is not None and case.base:
                a[:case.base] = SENTINEL
        self.records = torch.full((N, 3), -1, dtype=torch.int32, device=dev)
        self.counter = torch.tensor([12345, 678] if fresh else [case.base, 0], dtype=torch.int32, device=dev)  # fresh: garbage, overwritten
        if fresh:
            self.nears, self.fars = torch.full((N,), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)
            self.aabb = data.aabb()
        else:
            self.nears, self.fars = torch.from_numpy(np.array(case.nears)).to(dev), torch.from_numpy(np.array(case.fars)).to(dev)
        head = (ptr(self.o), ptr(self.d), ptr(self.bits), mc.BOUND, mc.DT_GAMMA, case.max_steps, N, mc.CASCADES, case.H, M)
        if fresh:
            call = lambda: lib.nerftex_march_rays_train_fresh(*head, ptr(self.aabb), mc.MIN_NEAR, ptr(self.nears), ptr(self.fars), ptr(self.xyzs),  # noqa: E731
                                                              ptr(self.dirs), ptr(self.deltas), ptr(self.records), ptr(self.counter), int(case.perturb), stream())
        elif form == "differentiable":
            call = lambda: lib.nerftex_march_rays_train_differentiable(*head, ptr(self.nears), ptr(self.fars), ptr(self.xyzs), ptr(self.dirs),  # noqa: E731
                                                                       ptr(self.deltas), ptr(self.ts), ptr(self.records), ptr(self.counter),
                                                                       int(case.perturb), stream())
        else:
            call = lambda: lib.nerftex_march_rays_train(*head, ptr(self.nears), ptr(self.fars), ptr(self.xyzs), ptr(self.dirs), ptr(self.deltas),  # noqa: E731
                                                        ptr(self.records), ptr(self.counter), int(case.perturb), stream())
        self.call = lambda: check(call())

    def run(self):
        self.call()
        return self

    def again(self):
        """The fresh form once more into the same, dirtied buffers."""
        assert self.form == "fresh"
        for a in (self.flat, self.nears, self.fars):
            a.fill_(float("nan"))
        self.counter.copy_(torch.tensor([-3, 99], dtype=torch.int32))
        self.records.fill_(-1)
        return self.run()

    def assert_same(self):
        """Everything the call wrote against the oracle, exactly."""
        c, u32 = self.case, lambda a: np.ascontiguousarray(a).view(np.uint32)  # noqa: E731
        assert self.counter.cpu().tolist() == c.counter.tolist() == [c.base + c.total, c.N]
        records = self.records.cpu().numpy()
        assert np.array_equal(records, c.records)
        pairs = [("xyzs", self.xyzs, c.xyzs), ("dirs", self.dirs, c.dirs), ("deltas", self.deltas, c.deltas)]
        if self.form == "differentiable":
            pairs.append(("ts", self.ts, c.ts))
        if self.form == "fresh":
            assert np.array_equal(u32(self.nears.cpu().numpy()), u32(c.nears)) and np.array_equal(u32(self.fars.cpu().numpy()), u32(c.fars))
        end = min(c.base + c.total, c.M)
        for name, got, want in pairs:
            got = got.cpu().numpy()
            assert got.shape == want.shape and got.shape[0] == c.M
            assert (got[:c.base] == SENTINEL).all(), name  # the rows in front of a preset counter are untouched
            assert not got[end:].any(), name  # nothing behind the total
            for n in np.nonzero(c.dropped)[0]:  # nothing in the rows of a dropped ray
                assert not got[records[n, 1]:records[n, 1] + records[n, 2]].any(), (name, int(n))
            assert np.array_equal(u32(got[c.base:]), u32(want[c.base:])), name  # the samples, and zero wherever the oracle left zero


def _launched(fn):
    """fn() with the library's kernel timers on: -> (its result, the names of the march's kernels that were launched)."""
    import nerftex_hip

    nerftex_hip.kernel_profile(True, reset=True)
    try:
        out = fn()
        names = set(nerftex_hip.kernel_profile())
    finally:
        nerftex_hip.kernel_profile(False)
        nerftex_hip.kernel_profile(reset=True)
    return out, names & MARCH_KERNELS


def _sweeps(grid_name, H):
    """(max_steps, N, perturb, mirrored): the statistics cases at N = 97 with perturbation; at the sizes nothing ran at before, also the batch
    mirrored (the other direction signs in the upper half of each axis: march_cases.rays) and, on the two grids with long rays, the ragged batches
    and the unperturbed start."""
    s = [(ms, 97, True, False) for ms in STEPS[grid_name]]
    if H >= 256:
        s += [(1024, 97, True, True)]
        if grid_name in ("scene", "ones"):
            s += [(1024, N, True, False) for N in (31, 65)] + [(1024, N, False, False) for N in mc.BATCHES]
    return s


COMBINATIONS = [(path, form, H, grid_name) for H in mc.SIZES for path in _paths_at(H) for form in FORMS for grid_name in mc.GRIDS]


@pytest.mark.parametrize("path,form,H,grid_name", COMBINATIONS, ids=["-".join(map(str, c)) for c in COMBINATIONS])
def test_every_path_and_form_gives_the_oracles_bits(oracle, data, knobs, path, form, H, grid_name):
    _select(knobs, path)
    first = True
    for max_steps, N, perturb, mirrored in _sweeps(grid_name, H):
        for budget in ("fits", "cut"):
            case = mc.reference(oracle, grid_name, H, max_steps, N, perturb, budget, mirrored=mirrored)
            if budget == "cut" and case.total == 0:
                continue  # (an empty grid: nothing to cut)
            print(f"{path} {form} {grid_name}/{H} max_steps={max_steps} N={N} perturb={perturb}{' mirrored' if mirrored else ''} {budget}: {case.total} samples into {case.M} rows, "
                  f"most {int(case.records[:, 2].max())} on a ray, {int(case.dropped.sum())} rays dropped")
            if first:  # the path this test names is the one that runs
                run, names = _launched(_Launch(data, form, case).run)
                assert names == _kernels_of(path, form, H)
                first = False
            else:
                run = _Launch(data, form, case).run()
            run.assert_same()
            if form == "fresh":  # twice, as a trainer calls it: the second call finds dirty buffers
                run.again()
                run.assert_same()


PRESET = [(path, H) for H in (256, 512) for path in _paths_at(H)]


@pytest.mark.parametrize("form", ["plain", "differentiable"])
@pytest.mark.parametrize("path,H", PRESET, ids=[f"{p}-{H}" for p, H in PRESET])
def test_a_preset_counter_moves_every_offset(oracle, data, knobs, path, H, form):
    """counter = [1000, 0] on entry: offsets start at 1000, the counter ends at [1000 + total, N], rows [0, 1000) keep what they held."""
    _select(knobs, path)
    case = mc.reference(oracle, "ones", H, 1024, 97, True, "preset")
    assert case.base == 1000 and case.M == case.total + 1004 and case.records[0, 1] == 1000 and case.counter.tolist() == [1000 + case.total, 97]
    print(f"{path} {form} ones/{H} preset: {case.total} samples behind 1000 rows")
    run, names = _launched(_Launch(data, form, case).run)
    assert names == _kernels_of(path, form, H)
    run.assert_same()


def test_paths_back_to_back_share_nothing(oracle, data, knobs):
    """Five launches on one stream, nothing waited for in between, each on another path, batch and grid: the totals and the log they leave in
    the shared march workspace -- laid out per 32 rays by one path and per 64 by another, with the log behind a head whose size depends on N --
    must not show in the next one.  Every tensor of the five calls is made and uploaded first (a blocking copy waits for the stream); between
    the library calls only the knobs change, which are read on the host.  The first call asks for the largest workspace of the five, so none
    of the later ones makes the library allocate."""
    plan = [("default", "plain", mc.reference(oracle, "ones", 256, 1024, 97, True)),
            ("serial", "plain", mc.reference(oracle, "scene", 256, 1024, 31, True)),
            ("replay", "fresh", mc.reference(oracle, "scene", 512, 1024, 65, True)),
            ("lean", "plain", mc.reference(oracle, "zeros", 128, 1024, 97, True))]
    plan.append(plan[0])
    assert all(case.N * case.max_steps <= plan[0][2].N * plan[0][2].max_steps for _, _, case in plan)
    runs = [_Launch(data, form, case) for _, form, case in plan]  # uploads, fills: they wait
    torch.cuda.synchronize()
    for (path, _, _), run in zip(plan, runs):
        _select(knobs, path)
        run.run()
    for (path, form, case), run in zip(plan, runs):
        print(f"{path} {form} {case.grid_name}/{case.H} N={case.N}: {case.total} samples")
        run.assert_same()


@pytest.mark.parametrize("grid_name", ["scene", "alternate"])
@pytest.mark.parametrize("H", [256, 512])
def test_inference_march_on_the_same_dda(oracle, data, H, grid_name):
    """raymarching.march_rays walks the same Dda: 65 alive rays in reversed order, one and eight samples a call, from the near plane and from the
    middle of the box (coordinates on both sides of 128), with and without the perturbed start."""
    import raymarching

    N = 65
    o, d = mc.rays(N)
    nears, fars = oracle.near_far_from_aabb(o, d, mc.AABB, mc.MIN_NEAR)
    alive = np.arange(N, dtype=np.int32)[::-1].copy()
    bits = mc.grid(grid_name, H)
    ot, dt = data.rays(N)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(data.dev)  # noqa: E731
    nt, ft, at, bt = up(nears), up(fars), up(alive), data.grid(grid_name, H)
    hits = 0
    for start in ("near", "middle"):
        middle = np.float32(0.5) * nears[alive] + np.float32(0.5) * fars[alive]  # (halves first: near = far = FLT_MAX for a ray that misses)
        rays_t = nears[alive] if start == "near" else np.where(fars[alive] > nears[alive], middle, nears[alive]).astype(np.float32)
        for n_step in (1, 8):
            for seed in (0, 7):
                wx, wd, wl = oracle.march_rays(N, n_step, alive, rays_t, o, d, mc.BOUND, bits, mc.CASCADES, H, nears, fars, -1, seed, mc.DT_GAMMA, 1024)
                xyzs, dirs, deltas = raymarching.march_rays(N, n_step, at, up(rays_t), ot, dt, mc.BOUND, bt, mc.CASCADES, H, nt, ft, -1, seed, mc.DT_GAMMA, 1024)
                print(f"{grid_name}/{H} from {start} n_step={n_step} seed={seed}: {int((wl[:, 0] > 0).sum())} samples")
                hits += int((wl[:, 0] > 0).sum())
                for got, want in ((xyzs, wx), (dirs, wd), (deltas, wl)):
                    got = got.cpu().numpy()
                    assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert hits > 8 * N  # the case marches
