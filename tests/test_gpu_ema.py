"""The parameter EMA on the accelerated training step: nerftex_ema_update (csrc/trainstep.hip), ngp_harness.ema.DeviceEMA and
accelerate(ema_decay=).  The reference statement is torch_ema's update() (use_num_updates=True) as torch runs it on the device,

    n = num_updates + 1;  d = min(decay, (1 + n) / (10 + n));  tmp = s - p;  tmp.mul_(1.0 - d);  s.sub_(tmp)

and every comparison here is of BITS: the kernel does those three fp32 roundings and nothing else, so there is no tolerance to state."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INVALID = 1  # NERFTEX_ERR_INVALID


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _decay(decay, n):
    return min(decay, (1 + n) / (10 + n))


def _torch_update(shadow, params, decay, n):
    """torch_ema's update that makes `n` the count, on `shadow` in place."""
    w = 1.0 - _decay(decay, n)
    with torch.no_grad():
        for s, p in zip(shadow, params):
            tmp = s - p
            tmp.mul_(w)
            s.sub_(tmp)


# ------------------------------------------------------------------------------------------------- the C entry
def _arr(ts):
    return None if ts is None else (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _call(shadow, p0, p1=None, live=None, decay=0.95, num=None, ticket=None, advance=1, count=None):
    from nerftex_hip import EmaDesc, lib, ptr, stream

    desc = EmaDesc(decay, ptr(num), ptr(ticket), ptr(live), advance)
    n = (ctypes.c_uint64 * len(shadow))(*[s.numel() for s in shadow])
    return lib.nerftex_ema_update(ctypes.byref(desc), len(shadow) if count is None else count, _arr(shadow), _arr(p0), _arr(p1), n, stream())


def _sizes(dev):
    """1, 7, 8, 1023, a little over two grid strides plus a ragged tail, and a little over EMA_UNROLL of them (where every thread takes the
    unrolled loop, and the first ones another group behind it) -- from the launch's own shape: a tensor gets at most EMA_BLOCKS_PER_CU blocks
    per compute unit, a block EMA_THREADS threads, a thread EMA_VEC floats per access and EMA_UNROLL accesses per turn."""
    from nerftex_hip import EMA_BLOCKS_PER_CU, EMA_THREADS, EMA_UNROLL, EMA_VEC

    stride = torch.cuda.get_device_properties(dev).multi_processor_count * EMA_BLOCKS_PER_CU * EMA_THREADS * EMA_VEC
    return [1, 7, 8, 1023, 2 * stride + 3 * EMA_THREADS * EMA_VEC + 3, EMA_UNROLL * stride + 2 * EMA_THREADS * EMA_VEC + 1]


_VALUES = {}


def _values(dev):
    """Per size a (shadow, param) pair, made once and never modified: table-scale (+-1e-4), O(1), +-0 and fp32 subnormals, interleaved so that
    every size holds every kind and every pairing of kinds."""
    if not _VALUES:
        g = torch.Generator().manual_seed(11)

        def mixed(n, shift):
            kinds = torch.stack([(torch.rand(n, generator=g) * 2 - 1) * 1e-4, torch.randn(n, generator=g),
                                 torch.zeros(n) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0),
                                 (torch.randint(1, 1 << 23, (n,), generator=g, dtype=torch.int32)
                                  | (torch.randint(0, 2, (n,), generator=g, dtype=torch.int32) << 31)).view(torch.float32)])
            pick = (torch.arange(n) // shift) % 4
            return kinds.gather(0, pick.unsqueeze(0)).squeeze(0).contiguous()

        for n in _sizes(dev):
            _VALUES[n] = (mixed(n, 1).to(dev), mixed(n, 4).to(dev))
        s, p = _VALUES[_sizes(dev)[-2]]
        sub = lambda t: ((_bits(t) & 0x7f800000) == 0) & ((_bits(t) & 0x007fffff) != 0)  # noqa: E731
        assert int(sub(s).sum()) > 1000 and int((sub(s) & sub(p)).sum()) > 100 and int(((_bits(s) == -2 ** 31) & (p == 0)).sum()) > 100
    return _VALUES


def test_decay_formula_changes_branch_where_the_cap_binds():
    """The chained starts below (169 .. 172) straddle the point where min() switches from the warm-up ratio to the cap 0.95."""
    assert _decay(0.95, 169) == 170 / 179 < 0.95
    assert _decay(0.95, 170) == 171 / 180 == 0.95
    assert 172 / 181 > 0.95 == _decay(0.95, 171) and 0.95 == _decay(0.95, 173)
    assert all(_decay(0.999, n) == (1 + n) / (10 + n) < 0.999 for n in range(1, 175))


@pytest.mark.parametrize("decay", [0.95, 0.999])
def test_kernel_equals_torch_bit_for_bit(dev, decay):
    """One call over the six tensors: three chained updates from num_updates = 0, then one each from 169, 170, 171 and 172."""
    vals = _values(dev)
    sizes = _sizes(dev)
    params = [vals[n][1] for n in sizes]
    num, ticket = torch.zeros((), dtype=torch.int32, device=dev), torch.zeros((), dtype=torch.int32, device=dev)
    got, want = [vals[n][0].clone() for n in sizes], [vals[n][0].clone() for n in sizes]
    for start in (0, 1, 2, 169, 170, 171, 172):
        if start >= 169:  # fresh shadows: after hundreds of updates towards fixed parameters nothing would move any more
            got, want = [vals[n][0].clone() for n in sizes], [vals[n][0].clone() for n in sizes]
        num.fill_(start)
        assert _call(got, params, decay=decay, num=num, ticket=ticket) == 0
        _torch_update(want, params, decay, start + 1)
        assert int(num) == start + 1 and int(ticket) == 0
        for n, a, b in zip(sizes, got, want):
            bad = int((_bits(a) != _bits(b)).sum())
            assert bad == 0, f"decay {decay}, update {start + 1}, size {n}: {bad} elements differ"
        assert not torch.equal(got[-1], vals[sizes[-1]][0]), "and the shadow moved"
    for n in sizes:
        assert torch.equal(_bits(params[sizes.index(n)]), _bits(vals[n][1])), "the parameters are only read"


def test_live_word_picks_the_parameter_set(dev):
    sizes = _sizes(dev)[:4] + [8192 + 5]
    g = torch.Generator().manual_seed(12)
    s0 = [torch.randn(n, generator=g).to(dev) for n in sizes]
    sets = [[torch.randn(n, generator=g).to(dev) for n in sizes] for _ in range(2)]
    num, ticket = torch.zeros((), dtype=torch.int32, device=dev), torch.zeros((), dtype=torch.int32, device=dev)
    for word, which in ((0, 0), (1, 1), (2, 0), (3, 1)):  # (only bit 0 counts)
        live = torch.full((), word, dtype=torch.int32, device=dev)
        got, want = [s.clone() for s in s0], [s.clone() for s in s0]
        num.zero_()
        assert _call(got, sets[0], sets[1], live, num=num, ticket=ticket) == 0
        _torch_update(want, sets[which], 0.95, 1)
        assert _same(got, want), f"*live = {word} reads set {which}"
        assert int(live) == word
    got, want = [s.clone() for s in s0], [s.clone() for s in s0]
    num.zero_()
    assert _call(got, sets[0], sets[1], None, num=num, ticket=ticket) == 0  # no live word: param0, whatever param1 is
    _torch_update(want, sets[0], 0.95, 1)
    assert _same(got, want)


def test_counter_and_split_launches(dev):
    g = torch.Generator().manual_seed(13)
    sizes = [1023, 7, 100003, 8, 1]
    s0 = [torch.randn(n, generator=g).to(dev) for n in sizes]
    params = [torch.randn(n, generator=g).to(dev) for n in sizes]
    num, ticket = torch.full((), 5, dtype=torch.int32, device=dev), torch.zeros((), dtype=torch.int32, device=dev)
    want = [s.clone() for s in s0]
    _torch_update(want, params, 0.95, 6)

    got = [s.clone() for s in s0]
    assert _call(got, params, num=num, ticket=ticket, advance=0) == 0
    assert int(num) == 5 and int(ticket) == 0 and _same(got, want), "advance = 0: the same update, the counter as it was"
    got = [s.clone() for s in s0]
    assert _call(got, params, num=num, ticket=ticket, advance=1) == 0
    assert int(num) == 6 and int(ticket) == 0 and _same(got, want)
    # two launches, the counter advanced by the second: one update over their union
    num.fill_(5)
    got = [s.clone() for s in s0]
    assert _call(got[:2], params[:2], num=num, ticket=ticket, advance=0) == 0
    assert _call(got[2:], params[2:], num=num, ticket=ticket, advance=1) == 0
    assert int(num) == 6 and int(ticket) == 0 and _same(got, want)
    # an empty tensor among the others is skipped; a launch of empty tensors alone still counts
    empty = torch.empty(0, device=dev)
    got = [s.clone() for s in s0]
    num.fill_(5)
    assert _call([got[0], empty] + got[1:], [params[0], empty] + params[1:], num=num, ticket=ticket) == 0
    assert int(num) == 6 and _same(got, want)
    assert _call([empty], [empty], num=num, ticket=ticket) == 0
    assert int(num) == 7 and int(ticket) == 0


def test_invalid_descriptors_launch_nothing(dev):
    from nerftex_hip import EmaDesc, lib, ptr, stream

    g = torch.Generator().manual_seed(14)
    buf = [torch.randn(64 + 1, generator=g).to(dev) for _ in range(3)]
    s, p0, p1 = [b[:64] for b in buf]
    keep = s.clone()
    num, ticket = torch.full((), 3, dtype=torch.int32, device=dev), torch.zeros((), dtype=torch.int32, device=dev)
    live = torch.zeros((), dtype=torch.int32, device=dev)
    n1 = (ctypes.c_uint64 * 1)(64)
    ok = dict(num=num, ticket=ticket)
    cases = {
        "decay 0": lambda: _call([s], [p0], decay=0.0, **ok),
        "decay 1": lambda: _call([s], [p0], decay=1.0, **ok),
        "decay < 0": lambda: _call([s], [p0], decay=-0.5, **ok),
        "decay nan": lambda: _call([s], [p0], decay=float("nan"), **ok),
        "count 0": lambda: _call([s], [p0], count=0, **ok),
        "count 9": lambda: _call([s] * 9, [p0] * 9, **ok),
        "count -1": lambda: _call([s], [p0], count=-1, **ok),
        "live without param1": lambda: _call([s], [p0], None, live, **ok),
        "misaligned shadow": lambda: _call([buf[0][1:]], [p0], **ok),
        "misaligned param0": lambda: _call([s], [buf[1][1:]], **ok),
        "misaligned param1": lambda: _call([s], [p0], [buf[2][1:]], live, **ok),
        "NULL descriptor": lambda: lib.nerftex_ema_update(None, 1, _arr([s]), _arr([p0]), None, n1, stream()),
        "NULL shadow": lambda: lib.nerftex_ema_update(ctypes.byref(EmaDesc(0.95, ptr(num), ptr(ticket), None, 1)), 1, None, _arr([p0]), None, n1, stream()),
        "NULL param0": lambda: lib.nerftex_ema_update(ctypes.byref(EmaDesc(0.95, ptr(num), ptr(ticket), None, 1)), 1, _arr([s]), None, None, n1, stream()),
        "NULL n": lambda: lib.nerftex_ema_update(ctypes.byref(EmaDesc(0.95, ptr(num), ptr(ticket), None, 1)), 1, _arr([s]), _arr([p0]), None, None, stream()),
        "NULL num_updates": lambda: _call([s], [p0], num=None, ticket=ticket),
        "NULL ticket": lambda: _call([s], [p0], num=num, ticket=None),
    }
    for name, call in cases.items():
        assert call() == INVALID and lib.nerftex_last_error().decode(), name
        torch.cuda.synchronize()
        assert torch.equal(_bits(s), _bits(keep)) and int(num) == 3 and int(ticket) == 0, f"{name}: nothing was launched"
    assert _call([s], [p0], [p1], live, **ok) == 0 and int(num) == 4 and not torch.equal(s, keep), "and the valid call next to them runs"


# ------------------------------------------------------------------------------------------------- the trainers
_SCENE = {}


def _ngp_case(dev):
    """The scene, rays and targets of tests/test_gpu_criterion.py's trainer tests, made once."""
    if not _SCENE:
        from ngp_harness import scene

        sc = scene.Scene(bound=2.0, seed=0)
        grid, _, _ = sc.bitfield()
        rays = [scene.train_batch(2048, seed=200 + k, n_views=2) for k in range(8)]
        _SCENE["grid"] = torch.from_numpy(grid).to(dev)
        _SCENE["rays"] = [(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)) for o, d in rays]
        _SCENE["tgt"] = torch.rand(8, 2048, 3, generator=torch.Generator().manual_seed(9)).to(dev) * 0.2 + 0.4
    return _SCENE


def _ngp_trainer(dev, field_kw=None, **kw):
    from ngp_harness.accelerate import accelerate
    from ngp_harness.model import NGPField, Renderer

    torch.manual_seed(0)
    field = NGPField(bound=2.0, **(field_kw or dict(mlp="ffmlp", fused_glue=True))).to(dev)
    torch.manual_seed(1)
    field.encoder.embeddings.data.uniform_(-1e-4, 1e-4)
    r = Renderer(field, bound=2.0, min_near=0.2, density_thresh=10.0).to(dev)
    r.set_occupancy(_ngp_case(dev)["grid"])
    field.train()
    return field, accelerate(r, perturb=False, **kw)


def _ema_params(field):
    return [p for p in field.parameters() if p.dtype != torch.long]  # nerf/utils.py:461


def _ngp_batch(dev, k):
    s = _ngp_case(dev)

    def batch(i):
        idx = [(i * k + j) % 8 for j in range(k)]
        return (torch.stack([s["rays"][j][0] for j in idx]).contiguous(), torch.stack([s["rays"][j][1] for j in idx]).contiguous(),
                s["tgt"][idx].contiguous())

    return batch


class Run:
    """`calls` calls of k steps each.  ema: accelerate(ema_decay=0.95), else a trainer WITHOUT the average whose fp32 parameters -- after a
    sync() behind every call, so k = 1 -- go through the host restatement (`shadow`; `snaps[c]`: its clone after call c).  overflow_at: that
    call's loss scale is forced out of fp16's range (and put back to 65536 behind it).  during(c, run): called between calls c - 1 and c."""

    def __init__(self, dev, calls, k=1, ahead=False, ema=True, overflow_at=None, during=None, snap_at=(), first_call=0, make=_ngp_trainer, batch=None,
                 prepare=None, **kw):
        self.field, self.tr = make(dev, steps_per_call=k, **({"ema_decay": 0.95} if ema else {}), **kw)
        field, tr = self.field, self.tr
        self.restate_from = None  # (shadow, count) for the restatement to go on from, set by `prepare`
        if prepare is not None:
            prepare(self)
        assert (tr.ema is not None) == ema
        batch = batch or _ngp_batch(dev, k)
        self.shadow, self.snaps, self.notes, losses = None, {}, {}, []
        n = 0 if tr.ema is None else tr.ema.num_updates
        if not ema:
            assert k == 1
            tr.sync()
            self.shadow = [p.detach().clone() for p in _ema_params(field)]
            if self.restate_from is not None:
                self.shadow, n = self.restate_from
        cur = batch(first_call)
        for c in range(first_call, first_call + calls):
            nxt = batch(c + 1)
            if during is not None:
                during(c, self)
            if overflow_at == c:
                self.notes["steps_before"] = float(tr.opt.step_count)
                tr.amp.scale.fill_(2.0 ** 40)
            if k > 1:
                tr.step_group(*cur, next_rays=nxt[:2] if ahead else None)
            else:
                tr.step(cur[0][0], cur[1][0], cur[2][0], next_rays=(nxt[0][0], nxt[1][0]) if ahead else None)
            if overflow_at == c:
                self.notes["steps_after"] = float(tr.opt.step_count)
                self.notes["updates_after"] = None if tr.ema is None else tr.ema.num_updates
                tr.amp.scale.fill_(65536.0)  # (halved once, 2^39 would overflow the next steps too: this test skips ONE)
            if not ema:
                tr.sync()
                n += 1
                _torch_update(self.shadow, [p.detach() for p in _ema_params(field)], 0.95, n)
                if c + 1 in snap_at:
                    self.snaps[c + 1] = ([s.clone() for s in self.shadow], [p.detach().clone() for p in _ema_params(field)])
            losses.append(tr.loss.clone())
            cur = nxt
        torch.cuda.synchronize()
        tr.sync()
        self.params = [p.detach().clone() for p in _ema_params(field)]
        self.losses = torch.stack(losses)
        if ema:
            self.shadow = [s.clone() for s in tr.ema.shadow_params]


CALLS = 33  # two rings of steps plus one call: the replayed graphs start at step 19


@pytest.fixture(scope="module")
def graphed(dev):
    return Run(dev, CALLS)


@pytest.fixture(scope="module")
def restated(dev):
    """The trainer without the average, its parameters read after every step and averaged on the host: snapshots after 16, 24 and 32 steps."""
    return Run(dev, CALLS, ema=False, snap_at=(16, 24, 32))


def test_fused_trainer_keeps_torch_emas_average(dev, graphed, restated):
    tr = graphed.tr
    assert tr._graphs is not None and tr.fused_table_update and tr.opt.live is not None, "the default fused step, replayed"
    assert tr.ema.num_updates == CALLS and tr.ema.decay == 0.95 and len(tr.ema.shadow_params) == len(_ema_params(graphed.field))
    eager = Run(dev, CALLS, graph=False)
    assert eager.tr._graphs is None
    assert _same(graphed.shadow, eager.shadow), "(a) replayed == graph=False"
    assert _same(graphed.shadow, restated.shadow), "(b) == torch_ema's statement over the parameters of a trainer without the average"
    assert not _same(graphed.shadow, graphed.params) and all(torch.isfinite(s).all() for s in graphed.shadow)
    assert _same(graphed.params, restated.params) and torch.equal(_bits(graphed.losses), _bits(restated.losses)), "(c) training is not disturbed"
    assert restated.tr.ema is None


def test_fused_trainer_in_groups_of_four_with_next_rays(dev, restated):
    """(d) steps_per_call = 4 with the next group's marches ahead: 32 steps, against the restatement's snapshot after 32 single steps."""
    want_shadow, want_params = restated.snaps[32]
    grouped = Run(dev, 8, k=4, ahead=True)
    assert grouped.tr._groups is not None and grouped.tr._side is not None and grouped.tr.ema.num_updates == 32
    eager = Run(dev, 8, k=4, graph=False)
    assert _same(grouped.shadow, eager.shadow) and _same(grouped.shadow, want_shadow)
    assert _same(grouped.params, want_params) and torch.equal(_bits(grouped.losses), _bits(restated.losses[3:32:4]))


def test_a_skipped_step_still_moves_the_average(dev):
    """An overflow forced inside the replayed part, fused_table_update on (the live word does not flip): the optimizer's step count stays, the
    average counts and moves towards the unchanged parameters -- the restatement does exactly that, its trainer skipping the same step."""
    got = Run(dev, 24, overflow_at=21)
    want = Run(dev, 24, ema=False, overflow_at=21)
    assert got.tr._graphs is not None and got.tr.fused_table_update
    for run in (got, want):
        assert run.notes["steps_after"] == run.notes["steps_before"] == 21.0, "the step was skipped"
    assert got.notes["updates_after"] == 22 and got.tr.ema.num_updates == 24
    assert float(got.tr.opt.step_count) == 23.0
    assert _same(got.shadow, want.shadow) and _same(got.params, want.params)


def test_swap_in_and_out(dev, graphed):
    seen = {}

    def swap(c, run):
        if c != 20:
            return
        tr, ema = run.tr, run.tr.ema
        tr.sync()
        before = [p.detach().clone() for p in _ema_params(run.field)], [leaf.detach().clone() for leaf in tr.opt.leaves]
        where = [p.data_ptr() for p in _ema_params(run.field)]
        ema.store()
        ema.copy_to()
        tr.sync()
        seen["params"] = _same([p.detach() for p in _ema_params(run.field)], ema.shadow_params)
        index = {id(m): i for i, m in enumerate(tr.opt.masters)}
        seen["leaves"] = all(torch.equal(tr.opt.leaves[index[id(p)]].detach(), s.to(tr.opt.leaves[index[id(p)]].dtype))
                             for p, s in zip(_ema_params(run.field), ema.shadow_params))
        b = _ngp_batch(dev, 1)(c)
        with pytest.raises(RuntimeError, match="swapped in"):
            tr.step(b[0][0], b[1][0], b[2][0])
        ema.restore()
        tr.sync()
        seen["restored"] = (_same([p.detach() for p in _ema_params(run.field)], before[0])
                            and all(torch.equal(a.detach(), b_) for a, b_ in zip(tr.opt.leaves, before[1])))
        seen["in_place"] = [p.data_ptr() for p in _ema_params(run.field)] == where

    swapped = Run(dev, CALLS, during=swap)
    assert seen == {"params": True, "leaves": True, "restored": True, "in_place": True}, seen
    assert swapped.tr._graphs is not None
    assert _same(swapped.params, graphed.params) and _same(swapped.shadow, graphed.shadow), "a run that swapped in and out ends where one that never did"
    assert torch.equal(_bits(swapped.losses), _bits(graphed.losses))
    # the context manager form, once the run is over
    tr = swapped.tr
    with tr.ema.average_parameters():
        tr.sync()
        assert _same([p.detach() for p in _ema_params(swapped.field)], tr.ema.shadow_params)
    tr.sync()
    assert _same([p.detach() for p in _ema_params(swapped.field)], swapped.params)


def test_checkpoint_round_trip(dev, tmp_path):
    """8 steps, a checkpoint through save_checkpoint(ema=), a FRESH trainer loaded through load_checkpoint(ema=) with optimizer and scaler, and on:
      * after 8 more steps its shadow and parameters are the bits of the uninterrupted 16-step run.  16, because that is as far as TRAINING
        itself resumes bit for bit: a fresh trainer runs its first ring on full-size sample buffers, the uninterrupted one leaves them after
        step 16, and the MLP weight gradients are summed over another number of row blocks then (tests/test_gpu_round3.py: "the fp16
        accumulation-order noise of the MLP gradients");
      * it goes on through its own capture into replayed steps, 33 in all, and its shadow stays torch_ema's statement continued from the
        checkpoint's shadow and count over the parameters of a twin loaded from the same file without the average."""
    from ngp_harness import checkpoint

    whole = Run(dev, 16)
    first = Run(dev, 8)
    sd = first.tr.ema.state_dict()
    assert set(sd) == {"decay", "num_updates", "shadow_params", "collected_params"}
    assert type(sd["decay"]) is float and sd["decay"] == 0.95 and type(sd["num_updates"]) is int and sd["num_updates"] == 8
    assert isinstance(sd["shadow_params"], list) and _same(sd["shadow_params"], first.shadow) and sd["collected_params"] is None
    assert [tuple(s.shape) for s in sd["shadow_params"]] == [tuple(p.shape) for p in _ema_params(first.field)]
    path = str(tmp_path / "ema.pth")
    state = checkpoint.save_checkpoint(path, first.tr.renderer, optimizer=first.tr.opt, scaler=first.tr.amp, ema=first.tr.ema)
    assert set(state["ema"]) == set(sd) and "ema" not in checkpoint.save_checkpoint(str(tmp_path / "plain.pth"), first.tr.renderer)

    def load(run):
        tr = run.tr
        checkpoint.load_checkpoint(path, tr.renderer, optimizer=tr.opt, scaler=tr.amp, ema=tr.ema)
        if tr.ema is not None:
            assert tr.ema.num_updates == 8 and _same(tr.ema.shadow_params, first.shadow)
        else:  # the twin: the restatement goes on from the checkpoint's average
            run.restate_from = ([s.clone() for s in first.shadow], 8)

    at16 = {}

    def snap(c, run):
        if c == 16:
            run.tr.sync()
            at16["shadow"], at16["params"] = [s.clone() for s in run.tr.ema.shadow_params], [p.detach().clone() for p in _ema_params(run.field)]

    resumed = Run(dev, CALLS - 8, first_call=8, prepare=load, during=snap)
    assert _same(at16["shadow"], whole.shadow), "the resumed run's average is the uninterrupted run's"
    assert _same(at16["params"], whole.params)
    twin = Run(dev, CALLS - 8, ema=False, first_call=8, prepare=load)
    assert resumed.tr._graphs is not None and resumed.tr.ema.num_updates == CALLS
    assert _same(resumed.shadow, twin.shadow) and _same(resumed.params, twin.params)
    # model_only leaves the average alone
    fresh = _ngp_trainer(dev, ema_decay=0.95)[1]
    checkpoint.load_checkpoint(path, fresh.renderer, optimizer=fresh.opt, model_only=True, ema=fresh.ema)
    assert fresh.ema.num_updates == 0


# ------------------------------------------------------------------------------------------------- the other optimizer paths
def _three_way(dev, calls, **kw):
    graphed, eager, want = Run(dev, calls, **kw), Run(dev, calls, graph=False, **kw), Run(dev, calls, ema=False, **kw)
    assert graphed.tr._graphs is not None and eager.tr._graphs is None and graphed.tr.ema.num_updates == calls
    assert _same(graphed.shadow, eager.shadow), "replayed == eager"
    assert _same(graphed.shadow, want.shadow), "== the restatement"
    assert _same(graphed.params, want.params) and torch.equal(_bits(graphed.losses), _bits(want.losses)), "training is not disturbed"
    assert not _same(graphed.shadow, graphed.params)
    return graphed


def test_two_launch_fused_step(dev):
    """HalfLeafAdam + FusedAmp without the fused table update: single-buffered state, no live word."""
    run = _three_way(dev, 20, fused_table_update=False)
    assert run.tr.fused and run.tr.opt.live is None


def test_torch_adam_path(dev):
    """The nn.Linear field on torch's fused Adam + GradScaler: the average reads the optimizer's own fp32 parameters."""
    run = _three_way(dev, 20, field_kw=dict(mlp="torch", split_k_linear=False))
    assert not run.tr.fused and run.tr.scaler is not None and len(run.tr.ema.shadow_params) > 3


def _curved_renderer(dev, like=None):
    """The smallest case of tests/test_gpu_curved_training.py."""
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer

    v, f = star_flower_mesh(n_lat=36, n_lon=72)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05).to(dev)
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    if like is not None:
        r.load_state_dict(like.state_dict())
        r.mean_density = like.mean_density
    else:
        with torch.no_grad():
            field.encoder.embeddings.uniform_(-0.5, 0.5)
            field.sigma_net.weights.mul_(3.0)
            for layer in field.encoder.cluster_layers:
                layer.cluster_centers.uniform_(-0.5, 0.5)
        with torch.autocast("cuda", dtype=torch.float16):
            r.update_extra_state_device()
    field.train()
    return field, r


def test_curved_trainer(dev):
    """CurvedTrainer on the small curved field: a cluster-centre tensor per level, more tensors than one launch holds."""
    from nerftex_hip import EMA_MAX_TENSORS
    from ngp_harness import scene
    from ngp_harness.accelerate import CurvedTrainer, accelerate

    N = 2048
    rays = []
    for i in range(6):
        o, d = scene.train_batch(N, seed=300 + i, radius=1.6)
        rays.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
    tgt = torch.rand(6, N, 3, generator=torch.Generator().manual_seed(300)).to(dev) * 0.2 + 0.4
    _, r0 = _curved_renderer(dev)

    def make(dev, **kw):
        field, r = _curved_renderer(dev, like=r0)
        np.random.seed(7)  # (the ring's level picks: the reference's own np.random call)
        return field, accelerate(r, perturb=False, **kw)

    def batch(i):
        return rays[i % 6][0].unsqueeze(0), rays[i % 6][1].unsqueeze(0), tgt[i % 6].unsqueeze(0)

    run = _three_way(dev, 24, make=make, batch=batch)
    assert isinstance(run.tr, CurvedTrainer) and len(run.tr.ema.shadow_params) > EMA_MAX_TENSORS
