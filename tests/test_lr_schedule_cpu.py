"""CPU: the device learning-rate schedule's host side (ngp_harness/lr_schedule.py) -- the factor table against torch's own LambdaLR, bit for bit;
the host mirror's state against a host LambdaLR's; what is refused.  The kernels that read the table are held to these values on the GPU
(tests/test_gpu_lr_schedule.py)."""
import types

import pytest
import torch
from torch.optim.lr_scheduler import LambdaLR, StepLR

from cpu_half_adam import CpuHalfLeafAdam
from ngp_harness.lr_schedule import DeviceLRSchedule, device_schedule_of
from ngp_harness.optim import FusedAmp


def _reference_lambda(iters):
    return lambda it: 0.1 ** min(it / iters, 1)  # main_nerf.py:133


def _opt(base_lrs):
    groups = [{"params": [torch.nn.Parameter(torch.zeros(4))], "lr": b} for b in base_lrs]
    return torch.optim.Adam(groups, betas=(0.9, 0.99), eps=1e-15)


@pytest.mark.parametrize("base_lrs", [[1e-2], [5e-3, 5e-3, 5e-3], [1e-2, 3.3e-4]], ids=["one_group", "three_groups", "two_rates"])
def test_device_table_is_lambdalr_bit_for_bit(base_lrs):
    """base_g * factor[t] from the device table (float64, read back) equals LambdaLR.get_last_lr() at every step of the reference's 40000."""
    iters = 40000
    dev_sched = DeviceLRSchedule(LambdaLR(_opt(base_lrs), _reference_lambda(iters)), iters, "cpu")
    host = LambdaLR(_opt(base_lrs), _reference_lambda(iters))
    factor = dev_sched.factor.tolist()
    assert dev_sched.factor.dtype == torch.float64 and len(factor) == iters + 1 and int(dev_sched.iter) == 0
    for t in range(iters + 1):
        want = host.get_last_lr()
        got = [b * factor[min(t, len(factor) - 1)] for b in dev_sched.base_lrs]
        assert got == want, t
        host.step()
    assert factor[-1] == 0.1 ** 1 and factor[0] == 1.0


def test_host_mirror_state_dict_is_lambdalrs():
    """After k training steps (in calls of 1 and of 4) the trainer's LambdaLR has the state_dict -- and param_groups lr -- of a host LambdaLR
    stepped k times; nothing is read from the device."""
    lam = _reference_lambda(48)
    opt = _opt([1e-2, 1e-2])
    sched = LambdaLR(opt, lam)
    dev_sched = DeviceLRSchedule(sched, 48, "cpu")
    host_opt = _opt([1e-2, 1e-2])
    host = LambdaLR(host_opt, lam)
    assert sched.state_dict() == host.state_dict()
    k = 0
    for n in (1, 4, 4, 1, 1, 4, 1):
        dev_sched.check(n)
        dev_sched.advance(n)
        for _ in range(n):
            host.step()
        k += n
        assert sched.state_dict() == host.state_dict(), k
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in host_opt.param_groups]
        assert sched.get_last_lr() == host.get_last_lr() and sched.last_epoch == k


def test_running_past_total_steps_is_refused():
    dev_sched = DeviceLRSchedule(LambdaLR(_opt([1e-2]), _reference_lambda(8)), 8, "cpu")
    dev_sched.check(8)
    dev_sched.advance(4)
    dev_sched.check(4)
    with pytest.raises(RuntimeError, match="total_steps"):
        dev_sched.check(5)
    dev_sched.advance(4)
    with pytest.raises(RuntimeError, match="total_steps"):
        dev_sched.check(1)


def test_only_lambdalr_and_a_total_are_accepted():
    with pytest.raises(TypeError, match="LambdaLR"):
        DeviceLRSchedule(StepLR(_opt([1e-2]), step_size=10), 100, "cpu")
    with pytest.raises(ValueError, match="total_steps"):
        DeviceLRSchedule(LambdaLR(_opt([1e-2]), _reference_lambda(8)), None, "cpu")
    opt = _opt([1e-2, 1e-2])
    with pytest.raises(ValueError, match="different factors"):
        DeviceLRSchedule(LambdaLR(opt, [lambda t: 1.0, lambda t: 0.5]), 8, "cpu")
    # per-group lambdas that agree are one table
    DeviceLRSchedule(LambdaLR(_opt([1e-2, 2e-2]), [lambda t: 0.9 ** t, lambda t: 0.9 ** t]), 8, "cpu")


def test_paths_that_cannot_follow_a_schedule_are_refused_at_construction():
    from ngp_harness.accelerate import AcceleratedTrainer, CurvedTrainer

    factory = lambda opt: LambdaLR(opt, _reference_lambda(100))  # noqa: E731
    nothing = types.SimpleNamespace(field=None)  # (refused before the renderer is looked at)
    for cls in (AcceleratedTrainer, CurvedTrainer):
        with pytest.raises(ValueError, match="pipeline_adam"):
            cls(nothing, pipeline_adam=4, lr_scheduler=factory, total_steps=100)


def test_half_leaf_adam_hands_the_schedule_to_the_table_update():
    """HalfLeafAdam.table_adam: with a schedule, lr is the base rate and `sched` points at the descriptor of the device table."""
    import ctypes

    mod = torch.nn.Module()
    mod.embeddings = torch.nn.Parameter(torch.zeros(64, 2))
    opt = CpuHalfLeafAdam([(mod, "embeddings")], lr=1e-2)
    amp = FusedAmp(opt)
    opt.enable_double_buffer()
    sched = LambdaLR(opt, _reference_lambda(16))
    dev_sched = DeviceLRSchedule(sched, 16, "cpu")
    t = opt.table_adam(0, amp)
    assert t.lr == 1e-2 and not t.sched
    opt.lr_schedule = dev_sched
    dev_sched.advance(3)
    t = opt.table_adam(0, amp)
    assert t.lr == 1e-2 and t.sched == ctypes.addressof(dev_sched.desc)
    assert dev_sched.desc.factor == dev_sched.factor.data_ptr() and dev_sched.desc.n == 17 and dev_sched.desc.iter == dev_sched.iter.data_ptr()
    assert opt.param_groups[0]["lr"] == 1e-2 * 0.1 ** (3 / 16)


def test_scheduler_state_loads_into_the_counter_and_the_mirror():
    """load_state_dict: last_epoch into the device counter and the host mirror; a reference state (one base_lrs entry per reference param group)
    is accepted when every entry equals this optimizer's base rate."""
    lam = _reference_lambda(40)
    host = LambdaLR(_opt([1e-2, 1e-2, 1e-2]), lam)  # the reference's --ff network: three groups at one rate
    for _ in range(24):
        host.step()
    opt = _opt([1e-2])
    sched = LambdaLR(opt, lam)
    dev_sched = DeviceLRSchedule(sched, 40, "cpu")
    assert device_schedule_of(sched) is dev_sched and device_schedule_of(host) is None
    dev_sched.load_state_dict(host.state_dict())
    assert int(dev_sched.iter) == 24 and sched.last_epoch == 24 and sched._step_count == host._step_count
    assert opt.param_groups[0]["lr"] == host.get_last_lr()[0] and sched.get_last_lr() == host.get_last_lr()[:1]
    bad = dict(host.state_dict(), base_lrs=[1e-2, 5e-3, 1e-2])
    with pytest.raises(ValueError, match="base_lrs"):
        dev_sched.load_state_dict(bad)
    with pytest.raises(ValueError, match="last_epoch"):
        dev_sched.load_state_dict(dict(host.state_dict(), last_epoch=41))
