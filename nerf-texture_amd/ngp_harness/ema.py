"""`DeviceEMA`: the reference trainer's exponential moving average of the parameters, kept on the device by the training step itself.

The reference builds its trainer with ema_decay=0.95 (main.py:190, main_nerf.py:133): nerf/utils.py:460-462 wraps every non-integer parameter
in torch_ema.ExponentialMovingAverage, :1027-1028 / :1358-1359 call `ema.update()` after every optimizer step, :1394-1396 / :1529-1537 swap
the average in for evaluation and for the "best" checkpoint, :1504-1505 / :1567-1568 carry it in the checkpoint under 'ema'.

On the accelerated step a Python `ema.update()` cannot do that: the optimizer state is double-buffered (the fp32 module parameters are one of
two sets, stale until a blocking `sync()`), and the step is replayed as a graph.  Here `update()` is ONE launch (nerftex_ema_update,
csrc/trainstep.hip) that reads the optimizer's live word on the device and is captured as the step's last launch.  The arithmetic is
torch_ema's, bit for bit (tests/test_gpu_ema.py):

    num_updates += 1;  decay = min(decay, (1 + num_updates) / (10 + num_updates));  w = 1.0 - decay
    tmp = shadow - param;  tmp.mul_(w);  shadow.sub_(tmp)

`store()` / `copy_to()` / `restore()` / `average_parameters()` / `state_dict()` / `load_state_dict()` are torch_ema's, host-level, between
steps: they copy IN PLACE into the buffers the graphs hold (the live fp32 set; the 16-bit leaves are re-derived) and never rebind a tensor.
"""
import contextlib
import ctypes

import torch


def decay_at(decay, num_updates):
    """torch_ema's decay of the update that makes `num_updates` the count (use_num_updates=True): min(decay, (1 + n) / (10 + n)).  The cap
    0.95 binds from n = 171 on."""
    return min(float(decay), (1 + num_updates) / (10 + num_updates))


def check_decay(ema_decay):
    """accelerate(ema_decay=): None (no average) or a float in (0, 1); anything else -- 0, 1, True, "0.95" -- is a ValueError."""
    if ema_decay is None:
        return None
    if isinstance(ema_decay, bool) or not isinstance(ema_decay, float) or not 0.0 < ema_decay < 1.0:
        raise ValueError(f"ema_decay: a float in (0, 1) (the reference trains with 0.95) or None, got {ema_decay!r}")
    return float(ema_decay)


class DeviceEMA:
    _needs_device = True  # update() is a HIP kernel; tests of the host-side logic subclass this with a torch stand-in for _launch

    def __init__(self, parameters, decay, optimizer=None):
        """parameters: the fp32 parameters, in the reference's order `[p for p in model.parameters() if p.dtype != torch.long]` (shadow_params[i]
        then lines up with a reference checkpoint's).  optimizer: the ngp_harness.optim.HalfLeafAdam that owns (some of) them, or None -- its
        sync() / resync() and, when its state is double-buffered, its two parameter sets and live word.  The shadow starts as a clone of the
        current parameters (after a sync())."""
        self.decay = check_decay(decay)
        assert self.decay is not None
        self.params = list(parameters)
        assert self.params and all(p.dtype == torch.float32 and p.is_contiguous() for p in self.params), "fp32 contiguous parameters"
        assert all(p.is_cuda for p in self.params) or not self._needs_device
        self.opt = optimizer if hasattr(optimizer, "resync") else None
        if self.opt is not None:
            self.opt.sync()
        dev = self.params[0].device
        with torch.no_grad():
            self.shadow_params = [p.detach().clone() for p in self.params]
        self.collected_params = None
        self._num_updates = torch.zeros((), dtype=torch.int32, device=dev)  # device word: a replayed step counts without the host
        self._ticket = torch.zeros((), dtype=torch.int32, device=dev)
        self.swapped_in = False  # between copy_to() and restore(): the parameters ARE the average, training must not step

    # ---- the launch -------------------------------------------------------------------------------------------------------------------
    def _sets(self):
        """-> (param0 tensors, param1 tensors or None, live word or None): what the launch reads.  Over a double-buffered optimizer the two
        sets' buffers (a parameter it does not own is its own second set); else the parameters' own storage."""
        opt = self.opt
        if opt is None or opt.live is None:
            return [p.data for p in self.params], None, None
        index = {id(m): i for i, m in enumerate(opt.masters)}
        own = [index.get(id(p)) for p in self.params]
        p0 = [p.data if i is None else opt._p[0][i] for p, i in zip(self.params, own)]
        p1 = [p.data if i is None else opt._p[1][i] for p, i in zip(self.params, own)]
        return p0, p1, opt.live

    def _launch(self):
        from nerftex_hip import EMA_MAX_TENSORS, EmaDesc, check, lib, ptr, stream

        p0, p1, live = self._sets()
        arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
        count = len(self.params)
        # more tensors than one launch holds (the curved field: a cluster-centre tensor per level): several launches that all read the same
        # count, the last one advancing it
        for a in range(0, count, EMA_MAX_TENSORS):
            b = min(a + EMA_MAX_TENSORS, count)
            desc = EmaDesc(self.decay, ptr(self._num_updates), ptr(self._ticket), ptr(live), int(b == count))
            n = (ctypes.c_uint64 * (b - a))(*[s.numel() for s in self.shadow_params[a:b]])
            check(lib.nerftex_ema_update(ctypes.byref(desc), b - a, arr(self.shadow_params[a:b]), arr(p0[a:b]), None if p1 is None else arr(p1[a:b]),
                                         n, stream()))

    def update(self):
        """torch_ema's update(): enqueued on the current stream, capturable (the buffers' addresses are baked into a capture, as the optimizer's
        are).  Reads the parameters of the optimizer's live set: call it behind the optimizer's launch of the step."""
        if self.swapped_in:
            raise RuntimeError("DeviceEMA.update(): the average is swapped in (copy_to() without restore()): the parameters are the average itself")
        self._launch()

    # ---- host level, between steps ----------------------------------------------------------------------------------------------------
    @property
    def num_updates(self):
        """The number of updates so far (one 4-byte read-back)."""
        return int(self._num_updates.item())

    def _current(self):
        """The parameters' current tensors: over a HalfLeafAdam, after sync() (module parameters point at the live set)."""
        if self.opt is not None:
            self.opt.sync()
        return [p.data for p in self.params]

    @torch.no_grad()
    def _write(self, values):
        """values -> the live fp32 set, in place; the 16-bit leaves follow."""
        for dst, src in zip(self._current(), values):
            dst.copy_(src)
        if self.opt is not None:
            self.opt.resync()

    @torch.no_grad()
    def store(self):
        """Keep a copy of the current parameters for restore()."""
        self.collected_params = [p.clone() for p in self._current()]

    def copy_to(self):
        """The average into the parameters (and their 16-bit leaves).  Until restore() the trainer refuses to step."""
        self._write(self.shadow_params)
        self.swapped_in = True

    def restore(self):
        """The store()d parameters back: the bits they were, leaves included."""
        if self.collected_params is None:
            raise RuntimeError("This DeviceEMA has no `store()`ed weights to `restore()`")
        self._write(self.collected_params)
        self.swapped_in = False

    @contextlib.contextmanager
    def average_parameters(self):
        """`with ema.average_parameters(): evaluate / save_checkpoint(...)` -- store(), copy_to(), and restore() on the way out."""
        self.store()
        self.copy_to()
        try:
            yield
        finally:
            self.restore()

    def state_dict(self):
        """torch_ema's keys and types (what the reference saves under 'ema', nerf/utils.py:1504-1505)."""
        clone = lambda ts: None if ts is None else [t.detach().clone() for t in ts]  # noqa: E731
        return {"decay": self.decay, "num_updates": self.num_updates, "shadow_params": clone(self.shadow_params),
                "collected_params": clone(self.collected_params)}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Inverse of state_dict(), in place (a captured step keeps reading the same shadow buffers and counter).  The decay is a constant of the
        captured launches: a checkpoint with another one is refused."""
        decay, num_updates = state_dict["decay"], state_dict["num_updates"]
        if float(decay) != self.decay:
            raise ValueError(f"the checkpoint's EMA decay is {decay!r}, this trainer's {self.decay!r} (accelerate(ema_decay=) fixes it for the captured steps)")
        if isinstance(num_updates, bool) or not isinstance(num_updates, int) or not 0 <= num_updates < 2 ** 31:
            raise ValueError(f"num_updates must be a non-negative int (use_num_updates=True), got {num_updates!r}")

        def fits(ts, what):
            if not isinstance(ts, (list, tuple)) or len(ts) != len(self.shadow_params) or any(
                    not isinstance(t, torch.Tensor) or t.shape != s.shape for t, s in zip(ts, self.shadow_params)):
                raise ValueError(f"{what} must be a list of {len(self.shadow_params)} tensors of the parameters' shapes")

        fits(state_dict["shadow_params"], "shadow_params")
        collected = state_dict.get("collected_params")
        if collected is not None:
            fits(collected, "collected_params")
        for s, t in zip(self.shadow_params, state_dict["shadow_params"]):
            s.copy_(t)
        self.collected_params = None if collected is None else [t.detach().to(device=s.device, dtype=s.dtype).clone() for t, s in zip(collected, self.shadow_params)]
        self._num_updates.fill_(num_updates)
