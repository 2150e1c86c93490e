"""CPU: the host side of the parameter EMA (ngp_harness/ema.py, accelerate(ema_decay=)) -- the refused values, the decay per update, and
DeviceEMA's torch_ema interface (state_dict / load_state_dict, store / copy_to / restore) over CPU tensors with a torch stand-in for the
launch, alone and over the double-buffered optimizer's stand-in (tests/cpu_half_adam.py).  tests/test_gpu_ema.py holds the kernel."""
import types

import pytest
import torch

from ngp_harness.accelerate import AcceleratedTrainer, CurvedTrainer, _refuse_options
from ngp_harness.ema import DeviceEMA, check_decay, decay_at


class HostEMA(DeviceEMA):
    """nerftex_ema_update restated with torch: the set the live word names, torch_ema's three operations, the counter."""
    _needs_device = False

    def _launch(self):
        p0, p1, live = self._sets()
        src = p1 if live is not None and int(live) & 1 else p0
        w = 1.0 - decay_at(self.decay, int(self._num_updates) + 1)
        for s, p in zip(self.shadow_params, src):
            tmp = s - p
            tmp.mul_(w)
            s.sub_(tmp)
        self._num_updates += 1


@pytest.mark.parametrize("value", [0, 1, 1.5, True, "0.95", 0.0, 1.0, -0.5, float("nan")])
def test_bad_ema_decay_is_refused_before_the_renderer_is_looked_at(value):
    nothing = types.SimpleNamespace(field=None)
    for cls in (AcceleratedTrainer, CurvedTrainer):
        with pytest.raises(ValueError, match="ema_decay"):
            cls(nothing, ema_decay=value)
    with pytest.raises(ValueError, match="ema_decay"):
        _refuse_options(None, 0, value)


@pytest.mark.parametrize("value", [None, 0.95, 0.999])
def test_good_ema_decay_passes_the_refusal(value):
    _refuse_options(None, 0, value)
    assert check_decay(value) == value
    nothing = types.SimpleNamespace(field=None)
    for cls in (AcceleratedTrainer, CurvedTrainer):
        with pytest.raises(AssertionError, match="field|CurvedField"):  # (past the refusal: the renderer is looked at, and is no renderer)
            cls(nothing, ema_decay=value)


def test_decay_per_update_is_torch_emas_formula():
    for decay in (0.95, 0.999):
        for n in range(1, 401):
            assert decay_at(decay, n) == min(decay, (1 + n) / (10 + n))
    # where the reference's cap starts to bind
    assert decay_at(0.95, 169) == 170 / 179 < 0.95 and decay_at(0.95, 170) == 0.95 == 171 / 180 and 172 / 181 > 0.95 == decay_at(0.95, 171)


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 2), (7,), (1,))]


def test_update_follows_torch_emas_statement():
    params = _params()
    ema = HostEMA(params, 0.95)
    want = [p.detach().clone() for p in params]
    assert all(torch.equal(s, p) and s.data_ptr() != p.data_ptr() for s, p in zip(ema.shadow_params, params))
    for n in range(1, 6):
        with torch.no_grad():
            for p in params:
                p.add_(0.1 * n)
        ema.update()
        d = min(0.95, (1 + n) / (10 + n))
        for s, p in zip(want, params):
            tmp = s - p.detach()
            tmp.mul_(1.0 - d)
            s.sub_(tmp)
        assert ema.num_updates == n and all(torch.equal(a, b) for a, b in zip(ema.shadow_params, want))


def test_state_dict_round_trip():
    params = _params()
    ema = HostEMA(params, 0.95)
    for _ in range(3):
        with torch.no_grad():
            params[0].mul_(1.5)
        ema.update()
    ema.store()
    sd = ema.state_dict()
    assert set(sd) == {"decay", "num_updates", "shadow_params", "collected_params"}
    assert type(sd["decay"]) is float and sd["decay"] == 0.95 and type(sd["num_updates"]) is int and sd["num_updates"] == 3
    assert isinstance(sd["shadow_params"], list) and all(isinstance(t, torch.Tensor) and not t.requires_grad for t in sd["shadow_params"])
    assert isinstance(sd["collected_params"], list) and all(torch.equal(c, p) for c, p in zip(sd["collected_params"], params))
    assert all(t.data_ptr() != s.data_ptr() for t, s in zip(sd["shadow_params"], ema.shadow_params)), "a snapshot, not the live buffers"

    other = HostEMA(_params(seed=1), 0.95)
    keep = [s.data_ptr() for s in other.shadow_params], other._num_updates.data_ptr()
    other.load_state_dict(sd)
    assert ([s.data_ptr() for s in other.shadow_params], other._num_updates.data_ptr()) == keep, "loaded in place: a captured step keeps its buffers"
    assert other.num_updates == 3 and all(torch.equal(a, b) for a, b in zip(other.shadow_params, ema.shadow_params))
    assert all(torch.equal(a, b) for a, b in zip(other.collected_params, ema.collected_params))
    sd2 = other.state_dict()
    assert sd2["num_updates"] == 3 and all(torch.equal(a, b) for a, b in zip(sd2["shadow_params"], sd["shadow_params"]))
    # without stored parameters the entry is None, as torch_ema's
    fresh = HostEMA(_params(), 0.95)
    assert fresh.state_dict()["collected_params"] is None
    fresh.load_state_dict({**sd, "collected_params": None})
    assert fresh.collected_params is None

    for bad in ({**sd, "decay": 0.9}, {**sd, "num_updates": -1}, {**sd, "num_updates": None}, {**sd, "shadow_params": sd["shadow_params"][:2]},
                {**sd, "shadow_params": [torch.zeros(3)] * 3}):
        with pytest.raises(ValueError):
            other.load_state_dict(bad)


def test_store_copy_to_restore_write_in_place():
    params = _params()
    ema = HostEMA(params, 0.95)
    with torch.no_grad():
        for p in params:
            p.add_(1.0)
    ema.update()
    before, where = [p.detach().clone() for p in params], [p.data_ptr() for p in params]
    with pytest.raises(RuntimeError, match="store"):
        ema.restore()
    ema.store()
    ema.copy_to()
    assert ema.swapped_in and all(torch.equal(p.detach(), s) for p, s in zip(params, ema.shadow_params))
    with pytest.raises(RuntimeError, match="swapped in"):
        ema.update()
    ema.restore()
    assert not ema.swapped_in and all(torch.equal(p.detach(), b) for p, b in zip(params, before))
    assert [p.data_ptr() for p in params] == where, "never rebinds a tensor"
    with ema.average_parameters():
        assert ema.swapped_in and all(torch.equal(p.detach(), s) for p, s in zip(params, ema.shadow_params))
    assert not ema.swapped_in and all(torch.equal(p.detach(), b) for p, b in zip(params, before))
    with pytest.raises(KeyError):  # the parameters come back on the way out of a failing block too
        with ema.average_parameters():
            raise KeyError("x")
    assert not ema.swapped_in and all(torch.equal(p.detach(), b) for p, b in zip(params, before))


def test_over_the_double_buffered_optimizer():
    """The live word picks the set update() reads; copy_to / restore write the live set and re-derive the 16-bit leaves."""
    from cpu_half_adam import CpuFusedAmp, CpuHalfLeafAdam

    torch.manual_seed(3)
    mods = [types.SimpleNamespace(w=torch.nn.Parameter(torch.randn(6, 2))), types.SimpleNamespace(w=torch.nn.Parameter(torch.randn(9)))]
    for m in mods:  # (enable_double_buffer registers state-dict hooks on its owners)
        m.register_state_dict_pre_hook = m.register_load_state_dict_pre_hook = lambda fn: None
    opt = CpuHalfLeafAdam([(m, "w") for m in mods], lr=1e-2)
    amp = CpuFusedAmp(opt)
    opt.enable_double_buffer()
    extra = torch.nn.Parameter(torch.randn(4))  # a parameter the optimizer does not own: its own second set
    params = [mods[0].w, extra, mods[1].w]
    ema = HostEMA(params, 0.95, optimizer=opt)
    want = [p.detach().clone() for p in params]

    def step(overflow=False):
        for leaf in opt.leaves:
            leaf.grad = torch.full_like(leaf, float("inf") if overflow else 0.5)
        amp.step()
        ema.update()
        opt.sync()
        d = decay_at(0.95, ema.num_updates)
        for s, p in zip(want, params):
            tmp = s - p.detach()
            tmp.mul_(1.0 - d)
            s.sub_(tmp)

    step()
    assert int(opt.live) == 1 and all(torch.equal(a, b) for a, b in zip(ema.shadow_params, want)), "read set 1, the one the step wrote"
    step(overflow=True)
    assert int(opt.live) == 1 and float(opt.step_count) == 1 and ema.num_updates == 2, "a skipped step still counts for the average"
    assert all(torch.equal(a, b) for a, b in zip(ema.shadow_params, want))
    step()
    assert int(opt.live) == 0 and all(torch.equal(a, b) for a, b in zip(ema.shadow_params, want))

    before = [p.detach().clone() for p in params], [leaf.detach().clone() for leaf in opt.leaves]
    stale = [t.clone() for t in opt._p[1]]
    with ema.average_parameters():
        opt.sync()
        assert all(torch.equal(p.detach(), s) for p, s in zip(params, ema.shadow_params))
        assert torch.equal(opt.leaves[0].detach(), ema.shadow_params[0].half()) and torch.equal(opt.leaves[1].detach(), ema.shadow_params[2].half())
        assert all(torch.equal(a, b) for a, b in zip(opt._p[1], stale)), "the other set is not touched"
    opt.sync()
    assert all(torch.equal(p.detach(), b) for p, b in zip(params, before[0]))
    assert all(torch.equal(leaf.detach(), b) for leaf, b in zip(opt.leaves, before[1]))
