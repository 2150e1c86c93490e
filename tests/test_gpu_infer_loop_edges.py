"""GPU: the inference loop's kernels at the C ABI (lib.nerftex_compact_rays*, nerftex_composite_rays*, nerftex_march_rays_dev) against the host
model tests/infer_loop_model.py, at the smallest sizes where their mechanisms can go wrong.  The model, its cases and the conditions the cases
must meet are checked on the CPU by tests/test_infer_loop_model_cpu.py; both modules build their inputs with the model's case builders.

WHY THESE SIZES.  The compaction ballots per wave of 64, ranks inside a wave, sums four waves per workgroup of 256 and the workgroups' partials
in strides of 256: list lengths 1, 63 .. 65, 255 .. 257, 511 .. 513 sit on every one of those seams, and 66049 = 257 x 257 runs 259 workgroups, where
thread 0 of the last ones takes a second pass over the partials.  Compositing runs one thread per alive slot: 1, 63, 64, 65 and 129 slots with 1, 4, 8
and 32 samples each, the alive list never the identity, and AUTO codes that come to F, 8 F and a value between.  The loop case walks 193 rays
(192 = 3 x 64 after the first iteration) until nothing is alive, and until a budget of 40 steps is used up.

Every output buffer is pre-filled with a sentinel and followed by 64 guard elements holding it; every test checks both.
"""
import numpy as np
import pytest
import torch

import infer_loop_model as m
import march_cases as mc

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = {torch.float32: -7777.0, torch.int32: -123456789}
NAN_BITS = 0x7FC12345  # the pattern the march's buffers are filled with
OK, ERR_INVALID = 0, 1
F4 = np.float32
WORST = {}  # worst |device - float64| / tolerance per (test, output)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Guarded:
    """n elements followed by GUARD sentinels; the elements hold the sentinel too unless `init` is given."""

    def __init__(self, n, dtype, dev, init=None, fill=None):
        self.n = n
        self.guard = SENTINEL[dtype] if fill is None else fill
        self.whole = torch.full((n + GUARD,), self.guard, dtype=dtype, device=dev)
        self.t = self.whole[:n]
        if init is not None:
            self.t.copy_(torch.from_numpy(np.array(init).reshape(-1)))  # (np.array: a writable copy of a read-only case array)

    def ptr(self):
        return self.whole.data_ptr()

    def numpy(self):
        assert bool((self.whole[self.n:] == self.guard).all()), "a write behind the end of the buffer"
        return self.t.cpu().numpy()


def nan_buffer(n, dev):
    """n floats of NAN_BITS + guard (kept as int32: a NaN compares unequal to itself)"""
    return Guarded(n, torch.int32, dev, fill=NAN_BITS)


def _up(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # (a writable copy: the cases' arrays are read-only)


def _bits(a):
    return np.ascontiguousarray(a, F4).view(np.uint32).reshape(-1)


def _same_floats(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _settle():
    """an event behind the launch, completed: from here the host may read the pinned mirror"""
    ev = torch.cuda.Event()
    ev.record()
    ev.synchronize()


_pinned = []


def _mirror():
    """two pinned host words, both -1: the kernel is given the second"""
    if not _pinned:
        _pinned.append(torch.empty(2, dtype=torch.int32).pin_memory())
    _pinned[0].fill_(-1)
    return _pinned[0]


def _note(test, ratios):
    for k, v in ratios.items():
        WORST[(test, k)] = max(WORST.get((test, k), 0.0), v)


# ------------------------------------------------------------------------------------------------------------------------------ compaction
def run_compaction(dev, case, call, old=None, bound=None):
    """One call of the entry `call.form` names -> (rc, new alive list, new rays_t, counter, step word, mirror) as the device leaves them.  The
    counter holds call.base, the step word call.steps_done (or a sentinel), the mirror -1 on entry."""
    from nerftex_hip import lib, stream

    bound = case.bound if bound is None else bound
    alive_old, t_old = old if old is not None else (_up(case.alive_old, dev), _up(case.t_old, dev))
    size = case.bound + (call.base if call.form == "plain" else 0)
    ra, rt = Guarded(size, torch.int32, dev), Guarded(size, torch.float32, dev)
    cnt = Guarded(1, torch.int32, dev, [call.base])
    steps = Guarded(1, torch.int32, dev, None if call.steps_done is None else [call.steps_done])
    n_dev = torch.tensor([case.count], dtype=torch.int32, device=dev)
    host = _mirror()
    lists = (ra.ptr(), alive_old.data_ptr(), rt.ptr(), t_old.data_ptr(), cnt.ptr())
    if call.form == "plain":
        rc = lib.nerftex_compact_rays(bound, *lists, stream())
    elif call.form == "dev":
        rc = lib.nerftex_compact_rays_dev(bound, n_dev.data_ptr(), *lists, stream())
    elif call.form == "budget":
        rc = lib.nerftex_compact_rays_budget_dev(bound, n_dev.data_ptr(), *lists, steps.ptr(), call.max_steps, call.code, stream())
    else:
        rc = lib.nerftex_compact_rays_budget_mirror_dev(bound, n_dev.data_ptr(), *lists, steps.ptr(), call.max_steps, call.code, host.data_ptr() + 4, stream())
    _settle()
    assert int(host[0]) == -1, "the word before the mirror"
    return rc, ra.numpy(), rt.numpy(), int(cnt.numpy()[0]), int(steps.numpy()[0]), int(host[1])


def check_compaction(dev, case, call, old=None):
    rc, ra, rt, counter, steps, mirror = run_compaction(dev, case, call, old)
    want = m.compact_call(case, call)
    what = (case.name,) + tuple(call)
    assert rc == OK, what
    want_ra, want_rt = m.filled(want, ra.size, SENTINEL[torch.int32], SENTINEL[torch.float32])  # everything not listed as written: the sentinel
    assert np.array_equal(ra, want_ra), what
    assert _same_floats(rt, want_rt), what
    assert counter == (call.base if want.counter is None else want.counter), what
    assert steps == ((SENTINEL[torch.int32] if call.steps_done is None else call.steps_done) if want.steps is None else want.steps), what
    assert mirror == (-1 if want.mirror is None else want.mirror), what


@pytest.mark.parametrize("n", m.SIZES)
def test_compaction_at_wave_and_workgroup_seams(dev, n):
    for case in m.compaction_cases(n):
        old = (_up(case.alive_old, dev), _up(case.t_old, dev))
        for call in m.compaction_calls(case):
            check_compaction(dev, case, call, old)


def test_compaction_step_word_under_every_code(dev):
    for case in m.budget_cases():
        old = (_up(case.alive_old, dev), _up(case.t_old, dev))
        for call in m.compaction_calls(case):
            check_compaction(dev, case, call, old)


def test_compaction_with_bound_zero_writes_nothing(dev):
    """A call with bound 0 launches nothing: the lists, the counter (stale and non-zero here), the step word and the mirror keep what they held.
    No caller issues it with a counter it goes on to read: the graphed loop sizes every launch by N, the pipelined loop stops at bound 0."""
    case = m.compaction_cases(65)[0]
    for call in (m.Call("plain", m.BASE, None, 0, 0), m.Call("dev", m.STALE, None, 0, 0), m.Call("budget", m.STALE, 0, m.MAX_STEPS, 4),
                 m.Call("mirror", m.STALE, 0, m.MAX_STEPS, m.rows_auto(100, 4))):
        rc, ra, rt, counter, steps, mirror = run_compaction(dev, case, call, bound=0)
        want = m.compact(call.form, 0, case.count, case.alive_old, case.t_old, call.base, call.steps_done, call.max_steps, call.code)
        assert want.counter is None and want.steps is None and want.mirror is None and want.k == 0
        assert rc == OK and (ra == SENTINEL[torch.int32]).all() and (rt == SENTINEL[torch.float32]).all()
        assert counter == call.base and mirror == -1
        assert steps == (SENTINEL[torch.int32] if call.steps_done is None else call.steps_done)


def test_budget_forms_refuse_null_words(dev):
    from nerftex_hip import lib, stream

    case = m.compaction_cases(65)[0]
    alive_old, t_old = _up(case.alive_old, dev), _up(case.t_old, dev)
    ra, rt = Guarded(case.bound, torch.int32, dev), Guarded(case.bound, torch.float32, dev)
    cnt, steps = Guarded(1, torch.int32, dev, [m.STALE]), Guarded(1, torch.int32, dev, [0])
    n_dev = torch.tensor([case.count], dtype=torch.int32, device=dev)
    host = torch.full((1,), -1, dtype=torch.int32).pin_memory()
    lists = (ra.ptr(), alive_old.data_ptr(), rt.ptr(), t_old.data_ptr(), cnt.ptr())
    refusals = [lib.nerftex_compact_rays_budget_dev(case.bound, n_dev.data_ptr(), *lists, None, 1024, 4, stream()),
                lib.nerftex_compact_rays_budget_dev(case.bound, None, *lists, steps.ptr(), 1024, 4, stream())]
    assert "steps_done and n_alive_dev must not be NULL" in lib.nerftex_last_error().decode()
    refusals += [lib.nerftex_compact_rays_budget_mirror_dev(case.bound, n_dev.data_ptr(), *lists, None, 1024, 4, host.data_ptr(), stream()),
                 lib.nerftex_compact_rays_budget_mirror_dev(case.bound, None, *lists, steps.ptr(), 1024, 4, host.data_ptr(), stream()),
                 lib.nerftex_compact_rays_budget_mirror_dev(case.bound, n_dev.data_ptr(), *lists, steps.ptr(), 1024, 4, None, stream())]
    assert "host_mirror must not be NULL" in lib.nerftex_last_error().decode()
    assert refusals == [ERR_INVALID] * 5
    _settle()
    assert (ra.numpy() == SENTINEL[torch.int32]).all() and (rt.numpy() == SENTINEL[torch.float32]).all()
    assert cnt.numpy()[0] == m.STALE and steps.numpy()[0] == 0 and int(host[0]) == -1


# ------------------------------------------------------------------------------------------------------------------------------ compositing
def run_compositing(dev, case, entry):
    """-> rays_t [bound], weights_sum, depth [N], image [N, 3] after one call of nerftex_composite_rays (entry "plain": n_alive = the true count,
    n_step the plain number) or nerftex_composite_rays_dev (the bound, the count word and the code)."""
    from nerftex_hip import check, lib, stream

    alive, sg, c, dl = (_up(a, dev) for a in (case.rays_alive, case.sigmas, case.rgbs, case.deltas))
    rt = Guarded(case.bound, torch.float32, dev, case.rays_t)
    ws, dp, im = (Guarded(a.size, torch.float32, dev, a) for a in (case.ws, case.depth, case.image))
    n_dev = torch.tensor([case.count], dtype=torch.int32, device=dev)
    rest = (alive.data_ptr(), rt.ptr(), sg.data_ptr(), c.data_ptr(), dl.data_ptr(), ws.ptr(), dp.ptr(), im.ptr(), stream())
    if entry == "plain":
        check(lib.nerftex_composite_rays(case.count, case.n_step, *rest))
    else:
        check(lib.nerftex_composite_rays_dev(case.bound, n_dev.data_ptr(), case.code, *rest))
    return rt.numpy(), ws.numpy(), dp.numpy(), im.numpy().reshape(-1, 3)


@pytest.mark.parametrize("name", [c.name for c in m.composite_cases()])
def test_compositing_against_float64(dev, name):
    case = m.composite_case(name)
    want_t, acc, _ = m.composite_reference(case)
    rays = case.rays_alive[:case.count]
    others = np.setdiff1d(np.arange(case.N), rays)
    got = {entry: run_compositing(dev, case, entry) for entry in ("plain", "dev")}
    for entry, (rt, ws, dp, im) in got.items():
        assert _same_floats(rt[:case.count], want_t[:case.count]), (entry, "rays_t, bit for bit")
        assert _same_floats(rt[case.count:], case.rays_t[case.count:]), (entry, "slots at and behind the true count")
        for out, given in ((ws, case.ws), (dp, case.depth), (im, case.image)):
            assert _same_floats(out[others], given[others]), (entry, "rays that are not in the alive list")
        ratios = m.acc_ratios(ws, dp, im, acc, rays)
        print(f"{name} {entry}: worst |device - float64| / tolerance: " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
        _note("compositing", ratios)
        assert max(ratios.values()) <= 1.0, (entry, ratios)
    for a, b in zip(got["plain"], got["dev"]):  # the same kernel: the same bits, whatever the bound and the code
        assert _same_floats(a, b)


# ------------------------------------------------------------------------------------------------------------------------------ march: the device count
@pytest.fixture(scope="module")
def march_scene(dev, oracle):
    """150 of the loop case's rays, in a scrambled order, on the sparse scene grid: some rays fill their slots, some do not"""
    import raymarching

    o, d, nears, fars = m.loop_rays(oracle)
    count = 150
    alive = np.random.default_rng(11).permutation(m.LOOP_N)[:count].astype(np.int32)
    t = nears[alive].astype(F4)
    s = dict(o=_up(o, dev), d=_up(d, dev), nears=_up(nears, dev), fars=_up(fars, dev), bits=_up(mc.grid("scene", m.LOOP_H), dev), alive=_up(alive, dev),
             t=_up(t, dev), count=count, ref={})

    def reference(n_step):
        if n_step not in s["ref"]:
            x, dd, dl = raymarching.march_rays(count, n_step, s["alive"], s["t"], s["o"], s["d"], mc.BOUND, s["bits"], mc.CASCADES, m.LOOP_H, s["nears"], s["fars"],
                                               -1, False, mc.DT_GAMMA, 1024)
            s["ref"][n_step] = tuple(a.cpu().numpy() for a in (x, dd, dl))
        return s["ref"][n_step]

    s["reference"] = reference
    return s


def _march_dev(dev, s, bound, count, code, rows):
    from nerftex_hip import check, lib, stream

    x, d, l = nan_buffer(rows * 3, dev), nan_buffer(rows * 3, dev), nan_buffer(rows * 2, dev)
    n_dev = torch.tensor([count], dtype=torch.int32, device=dev)
    check(lib.nerftex_march_rays_dev(bound, n_dev.data_ptr(), code, s["alive"].data_ptr(), s["t"].data_ptr(), s["o"].data_ptr(), s["d"].data_ptr(), mc.BOUND,
                                     mc.DT_GAMMA, 1024, mc.CASCADES, m.LOOP_H, s["bits"].data_ptr(), s["fars"].data_ptr(), x.ptr(), d.ptr(), l.ptr(), 0, stream()))
    return (a.numpy().view(np.uint32).reshape(rows, w) for a, w in ((x, 3), (d, 3), (l, 2)))


def check_march_rows(x, d, l, ref, live_rows):
    """x, d, l: uint32 views of what the device-count march left in NaN-filled buffers; ref: (xyzs, dirs, deltas) of the reference-shaped march on
    zeroed buffers (or of the oracle) over the first live_rows rows.  Returns the share of used slots."""
    rx, rd, rl = (np.ascontiguousarray(a[:live_rows], F4).view(np.uint32) for a in ref)
    used = ref[2][:live_rows, 0] > 0
    assert np.array_equal(x[:live_rows][used], rx[used]) and np.array_equal(d[:live_rows][used], rd[used]) and np.array_equal(l[:live_rows][used], rl[used])
    mark = F4(1e30).view(np.uint32)
    assert (x[:live_rows][~used] == mark).all() and (d[:live_rows][~used, 0] == mark).all() and (l[:live_rows][~used, 0] == 0).all(), "unused slots of a live ray"
    for a in (x, d, l):
        assert (a[live_rows:] == NAN_BITS).all(), "rows at and behind the true count"
    return float(used.mean()) if live_rows else 0.0


@pytest.mark.parametrize("code", [12, m.rows_auto(m.LOOP_N, m.LOOP_F), m.rows_auto(1500, 4)])
@pytest.mark.parametrize("slack", [0, 1, 500])
def test_march_reads_the_count_from_the_device(dev, march_scene, code, slack):
    s = march_scene
    count = s["count"]
    n_step = m.unit_rows(code, count)
    assert n_step == {12: 12, m.rows_auto(m.LOOP_N, m.LOOP_F): 5, m.rows_auto(1500, 4): 32}[code]
    rows = (count + 3) * n_step
    x, d, l = _march_dev(dev, s, count + slack, count, code, rows)
    used = check_march_rows(x, d, l, s["reference"](n_step), count * n_step)
    assert 0.2 < used < 0.98, "some rays fill their slots, some do not"


@pytest.mark.parametrize("code", [12, m.rows_auto(m.LOOP_N, m.LOOP_F)])
def test_march_with_a_device_count_of_zero_touches_nothing(dev, march_scene, code):
    rows = 40 * m.unit_rows(code, 0)
    for a in _march_dev(dev, march_scene, 500, 0, code, rows):
        assert (a == NAN_BITS).all()


# ------------------------------------------------------------------------------------------------------------------------------ the loop
@pytest.mark.parametrize("max_steps", m.LOOP_MAX_STEPS)
@pytest.mark.parametrize("grid", m.LOOP_GRIDS)
def test_loop_through_the_device_entries(dev, oracle, grid, max_steps):
    """compact_rays_budget_mirror_dev -> march_rays_dev -> (the stand-in field on the host, from the positions read back) -> composite_rays_dev, every
    launch sized by N, until the mirrored count is 0: every iteration's lists, words and march outputs equal the model's, the final accumulators lie
    within the tolerance carried through all iterations."""
    from nerftex_hip import check, lib, stream

    model = m.loop_model(oracle, max_steps, grid=grid)
    N, code = m.LOOP_N, m.LOOP_CODE
    o, d, nears, fars = m.loop_rays(oracle)
    ro, rd, far = _up(o, dev), _up(d, dev), _up(fars, dev)
    bits = _up(mc.grid(grid, m.LOOP_H), dev)
    ra = [Guarded(N, torch.int32, dev, np.arange(N, dtype=np.int32)), Guarded(N, torch.int32, dev)]
    rt = [Guarded(N, torch.float32, dev, nears), Guarded(N, torch.float32, dev)]
    cnt = [Guarded(1, torch.int32, dev, [N]), Guarded(1, torch.int32, dev, [m.STALE])]
    steps = Guarded(1, torch.int32, dev, [0])
    host = torch.full((1,), -1, dtype=torch.int32).pin_memory()
    ws, dp, im = Guarded(N, torch.float32, dev, np.zeros(N, F4)), Guarded(N, torch.float32, dev, np.zeros(N, F4)), Guarded(3 * N, torch.float32, dev, np.zeros(3 * N, F4))
    rows = m.LOOP_F * N + 64  # count * n_step <= F N whatever the iteration; some rows behind
    for i, it in enumerate(model):
        cur, old = (i + 1) % 2, i % 2
        ra[cur].t.fill_(SENTINEL[torch.int32])
        rt[cur].t.fill_(SENTINEL[torch.float32])
        check(lib.nerftex_compact_rays_budget_mirror_dev(N, cnt[old].ptr(), ra[cur].ptr(), ra[old].ptr(), rt[cur].ptr(), rt[old].ptr(), cnt[cur].ptr(), steps.ptr(),
                                                         max_steps, code, host.data_ptr(), stream()))
        _settle()
        k = int(host[0])
        assert (k, int(cnt[cur].numpy()[0]), int(steps.numpy()[0])) == (it.count, it.count, it.steps), i
        alive, t = ra[cur].numpy(), rt[cur].numpy()
        assert np.array_equal(alive[:k], it.rays_alive) and _same_floats(t[:k], it.rays_t), i
        assert (alive[it.survivors:] == SENTINEL[torch.int32]).all() and (t[it.survivors:] == SENTINEL[torch.float32]).all(), i
        if k == 0:
            break
        n_step = it.n_step
        live = k * n_step
        assert live <= rows - 32
        x, dd, dl = nan_buffer(rows * 3, dev), nan_buffer(rows * 3, dev), nan_buffer(rows * 2, dev)
        check(lib.nerftex_march_rays_dev(N, cnt[cur].ptr(), code, ra[cur].ptr(), rt[cur].ptr(), ro.data_ptr(), rd.data_ptr(), mc.BOUND, mc.DT_GAMMA, max_steps,
                                         mc.CASCADES, m.LOOP_H, bits.data_ptr(), far.data_ptr(), x.ptr(), dd.ptr(), dl.ptr(), 0, stream()))
        xb, db, lb = (a.numpy().view(np.uint32).reshape(rows, w) for a, w in ((x, 3), (dd, 3), (dl, 2)))
        check_march_rows(xb, db, lb, (it.xyzs, it.dirs, it.deltas), live)
        sigmas, rgbs = m.standin_field(xb[:live].view(F4))  # the positions the device wrote (the marks of unused slots among them)
        used = it.deltas[:, 0] > 0
        assert _same_floats(sigmas[used], it.sigmas[used]) and _same_floats(rgbs[used], it.rgbs[used])
        sg, c = _up(sigmas, dev), _up(rgbs, dev)
        check(lib.nerftex_composite_rays_dev(N, cnt[cur].ptr(), code, ra[cur].ptr(), rt[cur].ptr(), sg.data_ptr(), c.data_ptr(), dl.ptr(), ws.ptr(), dp.ptr(),
                                             im.ptr(), stream()))
        t = rt[cur].numpy()
        assert _same_floats(t[:k], it.rays_t_out), i
        assert (t[max(k, it.survivors):] == SENTINEL[torch.float32]).all(), i
    else:
        raise AssertionError("the device loop outlived the model's")
    assert i == len(model) - 1
    acc = model[-1].acc
    ratios = m.acc_ratios(ws.numpy(), dp.numpy(), im.numpy(), acc)
    print(f"loop, {grid} grid, max_steps {max_steps}, {i} iterations: worst |device - float64| / carried tolerance: " + ", ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    _note(f"loop {grid} {max_steps}", ratios)
    assert max(ratios.values()) <= 1.0, ratios
    assert float(acc["ws"].max()) > 0.1


def test_worst_ratios_are_printed():
    """(the record for the model's docstring and DESIGN.md; runs last in this module)"""
    for (test, out), v in sorted(WORST.items()):
        print(f"worst |device - float64| / tolerance, {test}, {out}: {v:.4f}")
