"""Per-step learning-rate schedules on the graphed training path: torch's `LambdaLR` with its factors in a device table.

The reference trains with `LambdaLR(optimizer, lambda iter: 0.1 ** min(iter / opt.iters, 1))` and steps it after every optimizer step,
skipped ones included (main_nerf.py:131-133, nerf/utils.py:1020-1025).  A replayed graph holds whatever learning rate its launches were
recorded with, and one graph of `steps_per_call` steps cannot take a new host value between its steps.  So the rate lives on the device:

  * `factor` float64 [total_steps + 1] = the user's own lambda at t = 0 .. total_steps (any LambdaLR lambda, called once per t, here);
  * `iter`, a device word: the training step number.  It starts at the scheduler's `last_epoch`, and the launch that ends a step advances it,
    applied or skipped -- the loss scaler's tail of nerftex_adam_mixed_step_amp[_db]_sched, or nerftex_lr_schedule_publish in front of
    torch's fused Adam;
  * step t trains at base_lr * factor[min(t, n - 1)], multiplied in double: the very value LambdaLR would put in param_groups[g]["lr"].

The host mirrors the counter without a read-back: after each training call the trainer calls `advance(k)`, which sets `last_epoch`,
`_step_count`, `_last_lr` and the float `param_groups[g]["lr"]` to what a host LambdaLR stepped k more times holds -- so logging and
`state_dict()` keep working.  Running past total_steps raises.  (An fp32 tensor lr of torch's fused Adam is written on the device in front of
the optimizer, so between calls it holds the rate of the last step launched; the mirror holds the next one, as LambdaLR does.)
"""
import ctypes
import weakref

import torch

_SCHEDULES = weakref.WeakKeyDictionary()  # LambdaLR -> its DeviceLRSchedule (an attribute on the scheduler would land in its state_dict)


def device_schedule_of(scheduler):
    """The DeviceLRSchedule a trainer built over `scheduler` (None: a plain host scheduler)."""
    return None if scheduler is None else _SCHEDULES.get(scheduler)


def factor_table(scheduler, total_steps):
    """lr_lambda(t) for t = 0 .. total_steps as Python floats; every param group must have the same factors (one device table)."""
    tables = {}
    for lam in scheduler.lr_lambdas:
        if id(lam) not in tables:
            tables[id(lam)] = [float(lam(t)) for t in range(int(total_steps) + 1)]
    first = next(iter(tables.values()))
    if any(t != first for t in tables.values()):
        raise ValueError("lr_scheduler: the param groups' lr_lambdas give different factors; the device schedule holds one factor table")
    return first


class DeviceLRSchedule:
    def __init__(self, scheduler, total_steps, device):
        from torch.optim.lr_scheduler import LambdaLR

        if not isinstance(scheduler, LambdaLR):
            raise TypeError(f"lr_scheduler: only torch.optim.lr_scheduler.LambdaLR can run on the device (the reference's schedule), got "
                            f"{type(scheduler).__name__}")
        if total_steps is None or int(total_steps) < 1:
            raise ValueError("lr_scheduler needs total_steps >= 1: the length of the device table of lr_lambda(t)")
        self.scheduler = scheduler
        self.total_steps = int(total_steps)
        self.base_lrs = [float(b) for b in scheduler.base_lrs]
        if not 1 <= len(self.base_lrs) <= 8:
            raise ValueError("lr_scheduler: 1 to 8 param groups")
        self.factors = factor_table(scheduler, self.total_steps)
        self.t = int(scheduler.last_epoch)
        if not 0 <= self.t <= self.total_steps:
            raise ValueError(f"lr_scheduler: last_epoch {self.t} outside [0, total_steps={self.total_steps}]")
        self.factor = torch.tensor(self.factors, dtype=torch.float64, device=device)
        self.iter = torch.full((), self.t, dtype=torch.int32, device=device)  # (the kernels' uint32 word)
        from nerftex_hip import LrSchedule

        self.desc = LrSchedule(self.factor.data_ptr(), len(self.factors), self.iter.data_ptr())
        self.lr_tensors = None
        _SCHEDULES[scheduler] = self
        self._mirror()

    def lr_at(self, t, g=0):
        """What LambdaLR holds in param_groups[g]["lr"] at last_epoch t."""
        return self.base_lrs[g] * self.factors[min(t, len(self.factors) - 1)]

    @property
    def desc_ptr(self):
        return ctypes.addressof(self.desc)

    # ---- host mirror ----
    def check(self, k):
        """Refuse, before anything is launched, k more training steps that would run past total_steps."""
        if self.t + k > self.total_steps:
            raise RuntimeError(f"lr_scheduler: {k} more step(s) from step {self.t} would run past total_steps={self.total_steps} (the device table's "
                               f"length); build the trainer with a larger total_steps")

    def advance(self, k):
        """k training steps have been launched: LambdaLR.step() k times, without calling the lambda or reading the device."""
        self.t += k
        self.scheduler._step_count += k
        self._mirror()

    def _mirror(self):
        s = self.scheduler
        s.last_epoch = self.t
        lrs = [self.lr_at(self.t, g) for g in range(len(self.base_lrs))]
        for group, lr in zip(s.optimizer.param_groups, lrs):
            if not isinstance(group["lr"], torch.Tensor):  # (a tensor lr is written by the device: nerftex_lr_schedule_publish)
                group["lr"] = lr
        s._last_lr = lrs

    # ---- torch.optim.Adam(fused=True): the rate as an fp32 tensor the optimizer reads at each step ----
    def use_tensor_lr(self, optimizer):
        assert optimizer is self.scheduler.optimizer
        self.lr_tensors = [torch.full((), self.lr_at(self.t, g), dtype=torch.float32, device=self.iter.device)
                           for g in range(len(self.base_lrs))]
        for group, t in zip(optimizer.param_groups, self.lr_tensors):
            group["lr"] = t
        self._pub = ((ctypes.c_double * len(self.base_lrs))(*self.base_lrs),
                     (ctypes.c_void_p * len(self.lr_tensors))(*[t.data_ptr() for t in self.lr_tensors]))
        return self

    def publish(self):
        """nerftex_lr_schedule_publish on the current stream: this step's rate into the lr tensors, then the counter advances."""
        from nerftex_hip import check, lib, stream

        check(lib.nerftex_lr_schedule_publish(self.desc_ptr, self._pub[0], self._pub[1], len(self.lr_tensors), stream()))

    # ---- checkpoints ----
    def state_dict(self):
        return self.scheduler.state_dict()

    def load_state_dict(self, sd):
        """Restore last_epoch into the device counter and the host mirror.  A reference checkpoint has one base_lrs entry per reference param
        group: accepted when they are all this optimizer's (every group of the reference's --ff network trains at the same base rate)."""
        theirs = [float(b) for b in sd["base_lrs"]]
        same = theirs == self.base_lrs or (len(set(theirs)) == 1 and set(self.base_lrs) == set(theirs))
        if not same:
            raise ValueError(f"lr_scheduler state: base_lrs {theirs} do not match this optimizer's {self.base_lrs}")
        t = int(sd["last_epoch"])
        if not 0 <= t <= self.total_steps:
            raise ValueError(f"lr_scheduler state: last_epoch {t} outside [0, total_steps={self.total_steps}]")
        self.t = t
        self.iter.fill_(t)
        self.scheduler._step_count = int(sd.get("_step_count", t + 1))
        if self.lr_tensors is not None:  # (an optimizer state load may have replaced the groups' lr objects: the graphs hold these)
            for g, (group, lt) in enumerate(zip(self.scheduler.optimizer.param_groups, self.lr_tensors)):
                group["lr"] = lt
                lt.fill_(self.lr_at(t, g))
        self._mirror()
