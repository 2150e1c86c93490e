"""`accelerate(renderer, ...)`: ONE call that gives a training loop the benchmarked path.

The reference trainer's step (nerf/utils.py:1011-1022, :559-620) is
    pred = model.render(rays_o, rays_d, staged=False, bg_color=..., perturb=True, force_all_rays=..., **opt)
    loss = criterion(pred['image'], gt);  scaler.scale(loss).backward();  scaler.step(optimizer);  scaler.update()
-- ~90 framework launches per step on the HIP kernels of the drop-in packages, bound by the host's launch rate (1.0-1.4 ms per
8192-ray step depending on the host, against 0.57 ms of kernels).  What the headline adds on top of the drop-in packages is host-side
only, and this module packages it behind one call for a loop that feeds FRESH rays every step (bench.py's headline bakes its ray pool
into the graphs; a trainer cannot):

    trainer = accelerate(renderer)                       # renderer: ngp_harness.model.Renderer over an NGPField
    loss = trainer.step(rays_o, rays_d, target_rgb)      # one training step; a device scalar, nothing is read back
    loss = trainer.step(rays_o, rays_d, target_rgb, next_rays=(o2, d2))   # ... and start marching the NEXT batch beside it
    trainer = accelerate(renderer, steps_per_call=4)     # the benchmarked structure for a loop that has 4 batches at a time:
    loss = trainer.step_group(o4, d4, t4, next_rays=(o4n, d4n))           # [4, N, 3] tensors: one graph for 4 steps, 4 marches ahead

  * the step replayed as HIP graphs over the renderer's 16-entry step-counter ring (renderer.py:656-660): the march of a batch (near / far,
    DDA, sample expansion: it needs the rays and the occupancy grid, NOT the weights) is one graph per ring slot, the rest (field, compositing
    + loss, backward, loss scaler, optimizer) of the `steps_per_call` steps of a call is one graph per call of the ring; both read rays /
    targets from static buffers the call copies into.  `step` is `step_group` with one batch: one body (`_steps`) enqueues either;
  * `next_rays`: a trainer that has its next batch's rays when it calls `step` (one `get_rays` ahead: software pipelining) hands them over
    and their march runs on a second, high-priority stream UNDER this step's kernels -- latency-bound work on issue slots the step leaves
    idle -- instead of in front of the next step; the next call must then pass the same rays (checked).  It is ordered behind the
    production of those rays (an event recorded at the call), not behind this step.  Without `next_rays` the march runs inline;
  * `NGPField(fused_glue=True)`: everything behind the hash-grid gather as one kernel forward, the glue folded into the MLP backward;
  * `HalfLeafAdam` + `FusedAmp`: Adam on the fp16 gradients and GradScaler's device side as two launches (FFMLP fields); a field with
    nn.Linear MLPs (BASELINE configs[1]) gets torch's fused capturable Adam + GradScaler inside the same graph;
  * sample buffers of a FIXED size, the ring's mean count rounded up to 4096 + 4096 (the reference sizes every step's buffers by the
    mean itself and silently drops the rays that do not fit, raymarching.cu:419; with the margin none are dropped); every 16 steps the
    mean is read back (the reference does the same in update_extra_state) and, if it left the size, two eager steps at the new size
    and a new capture follow.
  * `ema_decay=0.95`: the reference trainer's EMA of the parameters (torch_ema), kept by the step's last launch (ema.DeviceEMA: `trainer.ema`
    has update / store / copy_to / restore / average_parameters / state_dict); evaluate and save the "best" checkpoint under
    `with trainer.ema.average_parameters():` -- `step` raises while the average is swapped in.
The occupancy update stays the caller's (`renderer.update_extra_state_device()` every 16 steps writes grid and bitfield in place: the
graphs keep reading the same tensors).  A march started by `next_rays` reads the grid as it is at that moment: hand the next rays over
AFTER the update when one is due (the ring's end, where nothing is marched ahead anyway: the read-back comes first there).
Values: the same kernels in the same order as the eager step -- tests/test_gpu_round3.py::test_accelerate_replays_the_eager_step holds the
replayed step to the eager loss trajectory (bit for bit with and without `next_rays` on the FFMLP field), tests/test_gpu_round4.py::
test_step_group_trains_like_single_steps holds `step_group` to `step`, parameters bit for bit.
"""
import torch

RING = 16


class AcceleratedTrainer:
    def __init__(self, renderer, rays_per_batch=None, lr=1e-2, betas=(0.9, 0.99), eps=1e-15, dt_gamma=1 / 128, bg_color=1, perturb=True, max_steps=1024,
                 amp_dtype=torch.float16, graph=True, steps_per_call=1, march_across_ring_end=False, pipeline_adam=0, skip_dead_samples=None,
                 fused_table_update=None, fused_composite_step=None, lr_scheduler=None, total_steps=None, criterion=None, error_map=None,
                 ema_decay=None, target_channels=3, bg_generator=None):
        from .model import NGPField

        _refuse_options(lr_scheduler, pipeline_adam, ema_decay)
        self._init_pixels(bg_color, target_channels, bg_generator)
        self._init_criterion(criterion, error_map)
        field = renderer.field
        assert isinstance(field, NGPField), "accelerate() knows the ngp field (hash grid + two MLPs)"
        self._init_loop(renderer, field, rays_per_batch, dt_gamma, bg_color, perturb, max_steps, amp_dtype, graph, steps_per_call, march_across_ring_end)
        bf16 = amp_dtype == torch.bfloat16 and getattr(field, "fused_field_bf16", False)  # bf16 networks over the fp16 table (round 5)
        self.fused = field.mlp == "ffmlp" and ((field.fused_glue and amp_dtype == torch.float16) or bf16)
        if self.fused:
            from .optim import FusedAmp, HalfLeafAdam

            mlp_dt = torch.bfloat16 if bf16 else torch.float16
            self.opt = HalfLeafAdam([(field.encoder, "embeddings"), (field.sigma_net, "weights", mlp_dt), (field.color_net, "weights", mlp_dt)], lr=lr,
                                    betas=betas, eps=eps)
            # bf16 keeps the loss scaler: the table gradient is fp16 and unscaled gradients of ~1e-6 sit in its subnormals (profiles/r04_precision.json)
            self.amp, self.scaler = FusedAmp(self.opt), None
            if field.fused_field or bf16:
                self.amp.attach(field.encoder)  # found_inf raised by the kernels that write the gradients: no separate scan launch
        elif field.mlp == "torch" and amp_dtype == torch.float16 and self._split_k_layers(field):
            # configs[1] (nn.Linear MLPs on PyTorch-ROCm; round 5): the same optimizer path as the FFMLP field -- fp16 leaves for the table and the
            # five weight matrices (SplitKLinear hands its leaf to F.linear under autocast), one Adam launch, the loss scaler's device side in two
            # launches -- instead of torch's capturable fused Adam + GradScaler: no per-step cast of the 48 MB table, no widening of its gradient
            from .optim import FusedAmp, HalfLeafAdam

            self.fused = True
            self.opt = HalfLeafAdam([(field.encoder, "embeddings")] + [(layer, "weight") for layer in self._split_k_layers(field)], lr=lr, betas=betas, eps=eps)
            self.amp, self.scaler = FusedAmp(self.opt), None
        else:
            self.opt = torch.optim.Adam(field.get_params(lr), betas=betas, eps=eps, fused=True, capturable=self.use_graph)
            self.amp, self.scaler = None, torch.amp.GradScaler("cuda", enabled=amp_dtype in (torch.float16, torch.bfloat16))  # (the table gradient is fp16 either way)
        # skip_dead_samples (round 6; None = on wherever it exists -- the fused FFMLP field): the compositing backward flags the 32-sample steps that
        # carry a gradient and both MLP backward kernels and the hash-grid backward's record builder walk the flagged steps only.  In a trained scene
        # most samples sit behind the point where their ray's transmittance has underflowed and get EXACTLY zero gradients (raymarching.cu:843-870:
        # 42 % of the samples after 100 steps of the bench's scene, 99.6 % after 1000): the backward then costs what the live samples cost.  Exact: the
        # same parameters bit for bit (tests/test_gpu_round6.py); a young field, where every sample carries a gradient, pays one ballot per 64 steps.
        can_skip = bool(self.fused and field.mlp == "ffmlp")
        self.skip_dead_samples = can_skip if skip_dead_samples is None else bool(skip_dead_samples)
        assert not self.skip_dead_samples or can_skip, "skip_dead_samples needs the fused FFMLP field"
        renderer.skip_dead_samples = self.skip_dead_samples
        # fused_table_update (round 6; None = on wherever it exists): the hash-grid backward's summing kernel applies Adam to the hashed levels' rows
        # from its LDS tiles -- the record walk of some workgroups beside the parameter stream of others -- instead of writing their gradient for
        # the optimizer launch to read back (optim.FusedAmp.fuse_table_update).  Same parameters bit for bit, skipped overflow steps included; the
        # optimizer state is double-buffered: the fp32 module parameters are current after `trainer.sync()` (state_dict() calls it).
        can_fuse = bool(self.fused and self.amp is not None and hasattr(self.amp, "covered") and field.mlp == "ffmlp")
        self.fused_table_update = can_fuse if fused_table_update is None else bool(fused_table_update)
        assert not self.fused_table_update or can_fuse, "fused_table_update needs the fused FFMLP field under FusedAmp"
        if self.fused_table_update:
            self.amp.fuse_table_update(field.encoder)
        # fused_composite_step (round 6; None = on under the fused AMP step): compositing forward, render tail and their backward -- three adjacent,
        # latency-bound launches -- as ONE (fused.composite_tail's `one`: the step's root gradient is the tensor `_one`, so the forward's launch can
        # form the loss gradient itself).  Same outputs and gradients bit for bit (tests/test_gpu_round6.py).
        can_step = bool(self.fused and self.amp is not None)
        self.fused_composite_step = can_step if fused_composite_step is None else bool(fused_composite_step)
        assert not self.fused_composite_step or can_step, "fused_composite_step needs the fused AMP step (the root gradient must be known to be one)"
        renderer.root_one = self._one if self.fused_composite_step else None
        renderer.defer_step_loss = bool(self.fused_composite_step)  # (`_shade` reads the loss after the backward: the field's backward may finish it)
        self._attach_schedule(lr_scheduler, total_steps)
        self._attach_ema(ema_decay)

    def _init_criterion(self, criterion, error_map):
        """criterion / error_map of accelerate(): refused here, before the renderer is looked at, when they are not what the kernels do.  With
        neither, the step makes the very calls it always made (the MSE entries); with either, `trainer.ray_loss` is the last step's [N] per-ray
        loss, criterion(pred, gt).mean(-1), and `step(..., error_inds=)` updates the map in place (fused.step_loss_desc)."""
        self._loss_outputs = criterion is not None or error_map is not None
        self.criterion = parse_criterion("mse" if criterion is None else criterion)
        if error_map is not None and not (isinstance(error_map, torch.Tensor) and error_map.dtype == torch.float32 and error_map.is_contiguous()):
            raise ValueError("error_map: a contiguous float32 device tensor (any shape; it is updated in place at flat cell indices)")
        self.error_map = error_map
        self.ray_loss = None
        self._ray_loss, self._error_inds = None, None  # static per-ring-slot buffers, beside the targets

    def _init_pixels(self, bg_color, target_channels, bg_generator):
        """bg_color / target_channels / bg_generator of accelerate(): refused here, before the renderer is looked at, when they are not what the
        kernels do.  The reference's train_step draws a background per pixel and blends RGBA images over it (nerf/utils.py:602-615):
        bg_color="random" draws it per call, "given" takes it from `step(..., bg=)`; target_channels=4 makes the batches [N,4] RGBA pixels.
        With a number and 3 channels the step makes the very calls it always made: no descriptor, no buffer.  Both are constants of the graphs."""
        if isinstance(bg_color, str):
            if bg_color not in ("random", "given"):
                raise ValueError(f'bg_color: a number, "random" (a colour per ray drawn every call) or "given" (step(..., bg=) passes them); got {bg_color!r}')
            self.bg_mode = bg_color
        else:
            try:
                float(bg_color)
            except (TypeError, ValueError):
                raise ValueError(f'bg_color: a number, "random" (a colour per ray drawn every call) or "given" (step(..., bg=) passes them); got {bg_color!r}') from None
            self.bg_mode = None
        if isinstance(target_channels, bool) or target_channels not in (3, 4):
            raise ValueError(f"target_channels: 3 (RGB targets) or 4 (RGBA pixels, blended over the background by the step); got {target_channels!r}")
        if bg_generator is not None and not (self.bg_mode == "random" and isinstance(bg_generator, torch.Generator)):
            raise ValueError('bg_generator: a torch.Generator on the field\'s device, with bg_color="random" (it seeds the per-call draw)')
        self.target_channels, self.bg_generator = int(target_channels), bg_generator
        self._pixels = self.bg_mode is not None or self.target_channels == 4
        self._bg, self._gt = None, None  # static per-ring-slot buffers, beside the targets: the rays' backgrounds, the blended targets
        self.gt_rgb, self.last_bg = None, None  # after a call: the last step's target [N,3] (blended, with RGBA pixels) and background [N,3]

    def _check_batch(self, target, bg, grouped):
        """A call's targets and backgrounds against the trainer's constants: ValueError before anything is copied or launched (shapes and dtypes
        only: nothing on the device is looked at)."""
        if bg is not None and self.bg_mode != "given":
            raise ValueError('bg= without bg_color="given": this trainer ' + ("draws its backgrounds itself" if self.bg_mode == "random" else "blends over a constant colour"))
        if self.bg_mode == "given" and bg is None:
            raise ValueError('bg_color="given": pass the rays\' backgrounds, step(..., bg=[N,3]) / step_group(..., bg=[k,N,3])')
        if not self._pixels:
            return
        dims, C = (3 if grouped else 2), self.target_channels
        if not (isinstance(target, torch.Tensor) and target.dim() == dims and target.shape[-1] == C and target.dtype.is_floating_point):
            got = f"{target.dtype} {tuple(target.shape)}" if isinstance(target, torch.Tensor) else repr(type(target))
            raise ValueError(f"target: a floating-point {'[k,N,' if grouped else '[N,'}{C}] tensor (this trainer was built with target_channels={C}), got {got}")
        if bg is not None and not (isinstance(bg, torch.Tensor) and bg.dtype == torch.float32 and tuple(bg.shape) == tuple(target.shape[:-1]) + (3,)):
            got = f"{bg.dtype} {tuple(bg.shape)}" if isinstance(bg, torch.Tensor) else repr(type(bg))
            raise ValueError(f"bg: a torch.float32 tensor of shape {tuple(target.shape[:-1]) + (3,)}, one colour per ray, got {got}")

    def _fill_backgrounds(self, slot0, k, bg):
        """The backgrounds of the k steps at ring slots slot0 .. slot0 + k into their static buffers, on the step's stream in front of the steps and
        outside the graphs: "given" copies them like the targets; "random" is ONE torch.rand of [k,N,3] per call -- the reference's
        torch.rand_like, reproducible from bg_generator (a call of k steps draws once: k single steps draw the same numbers only for k = 1)."""
        if self.bg_mode is None:
            return
        if slot0 + k <= RING:
            dst = self._bg[slot0:slot0 + k]
            if self.bg_mode == "given":
                dst.copy_(bg.reshape(k, self.n_rays, 3), non_blocking=True)
            else:
                torch.rand(dst.shape, generator=self.bg_generator, out=dst)
            return
        # (eager steps that cross the ring's end: `step` and `step_group` mixed before the graphs run)
        src = bg.reshape(k, self.n_rays, 3) if self.bg_mode == "given" else torch.rand((k, self.n_rays, 3), generator=self.bg_generator, device=self.dev)
        for i in range(k):
            self._bg[(slot0 + i) % RING].copy_(src[i], non_blocking=True)

    def _published(self, slot):
        """After a call whose last step ran at ring slot `slot`: what the step trained against."""
        if self._loss_outputs:
            self.ray_loss = self._ray_loss[slot]
        if self._pixels:
            self.gt_rgb = self._gt[slot] if self._gt is not None else self._targets[slot]
            self.last_bg = self._bg[slot]

    def _init_loop(self, renderer, field, rays_per_batch, dt_gamma, bg_color, perturb, max_steps, amp_dtype, graph, steps_per_call, march_across_ring_end):
        """What the step loop keeps, whatever the field and its optimizer (both constructors start here)."""
        self.renderer, self.field = renderer, field
        self.dev = next(field.parameters()).device
        self.n_rays = rays_per_batch
        self.dt_gamma, self.bg_color, self.perturb, self.max_steps = dt_gamma, bg_color, perturb, max_steps
        self.amp_dtype = amp_dtype
        self.use_graph = bool(graph)
        self._one = torch.ones((), dtype=torch.float32, device=self.dev)
        # steps_per_call = k > 1: `step_group` takes the batches of k consecutive steps at once and replays ONE graph for their shade + backward +
        # optimizer (the hand-over between two graph launches idles the device ~10 us: bench.py's --steps-per-graph), their k marches being
        # graphs of their own that run ahead on the second stream when the caller hands the NEXT group's rays over
        self.group = int(steps_per_call)
        assert self.group in (1, 2, 4, 8, 16), "steps_per_call must divide the 16-entry step-counter ring"
        # march_across_ring_end: at the ring's last call, `next_rays` are marched ahead as well (right behind the mean_count read-back) instead
        # of inline at the start of the next ring.  That march reads the occupancy grid while this call's steps still run: a trainer that
        # updates the grid every 16 steps (nerf/utils.py:1011) must then do so BEFORE the ring's last call, not after it.  Off by default.
        # It acts for steps_per_call > 1 only: single steps never march across the ring's end.
        self.march_across_ring_end = bool(march_across_ring_end) and self.group > 1
        self._graphs, self._groups, self._M = None, None, 0  # per ring slot (march graph, marched tensors); per call of the ring its shade graph; the buffer size
        self._rays, self._targets = None, None  # static inputs per ring slot: rays (the march of slot g + 1 may run while slot g's is still read), targets
        self._primed, self._warm = 0, 0
        self._ahead = None  # (first slot, data_ptr of rays_o, data_ptr of rays_d) of the marches started by `next_rays`
        self._side = None
        if self.dev.type == "cuda":
            from .streams import ensure_pool

            ensure_pool(self.dev)  # (every stream of the package exists BEFORE this trainer's captures: streams.py)
        self.loss = torch.zeros((), dtype=torch.float32, device=self.dev)

    def _attach_schedule(self, factory, total_steps):
        """lr_scheduler = factory (the reference Trainer's shape: `lambda optimizer: LambdaLR(optimizer, ...)`), called on this trainer's optimizer:
        its lambda's factors go into a device table every optimizer launch reads (lr_schedule.py).  trainer.lr_scheduler is the LambdaLR, kept
        current on the host after every call.  Without a schedule the graphs hold the rate of their capture: a changed param_groups[g]["lr"]
        makes the next replay raise (_lr_guard)."""
        self.lr_scheduler, self._lr_sched, self._captured_lr = None, None, None
        if factory is None:
            return
        from torch.optim.lr_scheduler import LRScheduler

        from .lr_schedule import DeviceLRSchedule

        if isinstance(factory, LRScheduler) or not callable(factory):
            raise TypeError("lr_scheduler: pass a factory, `lambda optimizer: LambdaLR(optimizer, ...)` (it is called on the trainer's own optimizer)")
        sched = factory(self.opt)
        self._lr_sched = DeviceLRSchedule(sched, total_steps, self.dev)
        if self.fused:
            self.opt.lr_schedule = self._lr_sched  # HalfLeafAdam: the _sched launches (and the table update's descriptor)
        else:
            self._lr_sched.use_tensor_lr(self.opt)  # torch's fused Adam reads an fp32 tensor written by nerftex_lr_schedule_publish
        self.lr_scheduler = sched

    def _attach_ema(self, ema_decay):
        """ema_decay = the reference Trainer's (0.95 in main.py:190 / main_nerf.py:133): `trainer.ema` is an ema.DeviceEMA over the field's
        non-integer parameters in the reference's order (nerf/utils.py:461), updated by the last launch of every step, applied or skipped.
        None: no buffer, no launch, the same captured graphs."""
        self.ema = None
        if ema_decay is None:
            return
        from .ema import DeviceEMA

        self.ema = DeviceEMA([p for p in self.field.parameters() if p.dtype != torch.long], ema_decay, optimizer=self.opt)

    def _lr_guard(self):
        """Without a schedule the replayed launches train at the rate they were captured with: refuse to replay after it changed."""
        if self._lr_sched is None and self._captured_lr is not None and self._captured_lr != _host_lrs(self.opt):
            raise RuntimeError(f"param_groups lr changed from {self._captured_lr} to {_host_lrs(self.opt)} after the training graphs were captured; "
                               "they would keep training at the old rate.  Attach the schedule with accelerate(..., lr_scheduler=, total_steps=)")

    @staticmethod
    def _split_k_layers(field):
        """The nn.Linear field's layers when every one of them is a SplitKLinear (at most 7: HalfLeafAdam takes 8 tensors), else []."""
        from .model import SplitKLinear

        layers = list(field.sigma_net) + list(field.color_net)
        return layers if layers and len(layers) <= 7 and all(isinstance(m, SplitKLinear) for m in layers) else []

    # ---- the two halves of one eager step; mean_count None = the ring's (full-size buffers while it is unknown)
    def _march(self, ro, rd, mean_count=None):
        with torch.autocast("cuda", dtype=self.amp_dtype):
            return self.renderer.march_train(ro, rd, dt_gamma=self.dt_gamma, perturb=self.perturb, max_steps=self.max_steps, mean_count=mean_count)

    def _shade(self, marched, slot):
        r, tgt = self.renderer, self._targets[slot]
        if self.fused:
            for leaf in self.opt.leaves:
                leaf.grad = None
        else:
            self.opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=self.amp_dtype):
            image, depth, loss, scaled = r.shade_train(marched, self._bg_arg(slot), target=tgt, scale=self.amp.scale if self.amp else None,
                                                       **self._loss_args(slot))[:4]  # (a fifth, with RGBA pixels: the blended target, which is _gt[slot])
        if self.amp:
            scaled.backward(self._one)
            self.amp.step()
        else:
            self.scaler.scale(scaled).backward()  # (scale None: `scaled` is the loss itself, with its graph)
            if self._lr_sched is not None:
                self._lr_sched.publish()  # this step's rate into the optimizer's lr tensors; counts skipped steps too
            self.scaler.step(self.opt)
            self.scaler.update()
        self.loss.copy_(loss.detach().reshape(()))
        if self.ema is not None:
            self.ema.update()  # the step's last launch: behind the optimizer's, reads the set its live word names (a skipped step: the unchanged one)

    def _loss_args(self, slot):
        """shade_train's criterion / per-ray loss / error map / blended-target arguments of a step at ring slot `slot`: none unless accelerate()
        was given any."""
        kw = {}
        if self._loss_outputs:
            kw.update(criterion=self.criterion, ray_loss=self._ray_loss[slot], error_map=self.error_map,
                      error_inds=None if self.error_map is None else self._error_inds[slot])
        if self._gt is not None:
            kw.update(target_out=self._gt[slot])
        return kw

    def _bg_arg(self, slot):
        """shade_train's bg_color of a step at ring slot `slot`: the number, or the slot's static [N,3] backgrounds."""
        return self.bg_color if self._bg is None else self._bg[slot]

    def _capture(self):
        """Record the graphs: a march graph per ring slot into `_graphs`, a shade graph (shade + backward + optimizer of its `group` steps) per
        call of the ring into `_groups`.  Nothing is executed here: the eager steps at this buffer size that ran just before (real training
        steps) have sized the library's workspaces and done every lazy initialisation outside the capture."""
        from .streams import capture_section

        r, k = self.renderer, self.group
        with capture_section():
            keep_step = r.local_step
            graphs, pool, pool_m = [], None, None  # (the march graphs share one memory pool, the shade graphs another: a march may run beside a shade)

            def shade_graph(g0):
                nonlocal pool
                gg = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gg, pool=pool, capture_error_mode="thread_local"):
                    for g in range(g0, g0 + k):
                        self._shade(graphs[g][1], g)
                pool = gg.pool()
                return gg

            groups = []
            for g in range(RING):  # per ring slot: the step's counter is slot g, as in the eager loop
                r.local_step = g
                gm = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gm, pool=pool_m, capture_error_mode="thread_local"):
                    marched, _ = self._march(*self._rays[g], mean_count=self._M)
                pool_m = gm.pool()
                graphs.append((gm, marched))  # (the sample tensors stay alive: the shade graph reads them)
                if k == 1:  # a single step's shade graph is recorded right behind its march, a group's behind all sixteen (the order lays out the two pools)
                    groups.append(shade_graph(g))
            if k > 1:
                groups = [shade_graph(g0) for g0 in range(0, RING, k)]
            self._graphs, self._groups = graphs, groups
            r.local_step = keep_step % RING
            self._captured_lr = _host_lrs(self.opt)

    def _ensure_buffers(self, n_rays):
        if self._rays is None:
            self.n_rays = n_rays
            self._ray_o = torch.empty(RING, n_rays, 3, dtype=torch.float32, device=self.dev)
            self._ray_d = torch.empty(RING, n_rays, 3, dtype=torch.float32, device=self.dev)
            self._rays = [(self._ray_o[g], self._ray_d[g]) for g in range(RING)]
            self._targets = torch.empty(RING, n_rays, self.target_channels, dtype=torch.float32, device=self.dev)
            if self._pixels:  # (a number under RGBA pixels: spread over the rays once, here)
                self._bg = torch.full((RING, n_rays, 3), 0.0 if self.bg_mode is not None else float(self.bg_color), dtype=torch.float32, device=self.dev)
            if self.target_channels == 4:
                self._gt = torch.zeros(RING, n_rays, 3, dtype=torch.float32, device=self.dev)
            if self._loss_outputs:
                self._ray_loss = torch.zeros(RING, n_rays, dtype=torch.float32, device=self.dev)
                self.ray_loss = self._ray_loss[0]
            if self.error_map is not None:
                assert self.error_map.device == self.dev, "error_map lives on the field's device"
                self._error_inds = torch.full((RING, n_rays), -1, dtype=torch.int64, device=self.dev)
        assert n_rays == self.n_rays, "a captured step has a fixed batch size"

    def _ring_end(self, ready):
        """One read-back per 16 steps, as in the reference.  Every march of the ring has run by now, so with a second stream at hand the
        read-back waits for the marches only, not for the last step's backward.  Nothing is marched ahead across the ring's end: that is
        where the trainer updates the occupancy grid (nerf/utils.py:1011, before the next step), and a march started here would read the grid
        while the update writes it."""
        r = self.renderer
        if ready is not None:
            with torch.cuda.stream(self._side_stream()):
                self._side.wait_event(ready)
                r.update_mean_count()
        else:
            r.update_mean_count()
        self._resize()

    def step_group(self, rays_o, rays_d, target, next_rays=None, error_inds=None, bg=None):
        """steps_per_call = k consecutive training steps in one call: rays_o / rays_d / target [k, N, 3] -- batch i is step i's (FRESH rays every
        call: they are copied into the graphs' static buffers).  next_rays = (rays_o, rays_d) [k, N, 3] of the NEXT call: their k marches start
        now, on the second stream, beside this group's kernels; the next call must pass those very tensors.  Same arithmetic as k calls of
        `step`: the same kernels in the same order on the same data (tests/test_gpu_round4.py::test_step_group_trains_like_single_steps).
        error_inds [k, N] int64 (accelerate(error_map=)): each ray's flat cell of the map; omitted, no cell is updated.
        target [k, N, 4] with accelerate(target_channels=4); bg [k, N, 3] fp32 with accelerate(bg_color="given"): the rays' backgrounds.
        Returns the last step's loss (device scalar)."""
        assert self.group > 1 and rays_o.dim() == 3 and rays_o.shape[0] == self.group, "step_group: [steps_per_call, N, 3] rays (steps_per_call > 1)"
        self._check_batch(target, bg, True)
        return self._steps(rays_o, rays_d, target, next_rays, error_inds, bg)

    def step(self, rays_o, rays_d, target, next_rays=None, error_inds=None, bg=None):
        """One training step on a batch of rays [N,3], [N,3] and their target colours [N,3] (device tensors; N fixed after the first call).
        next_rays = (rays_o, rays_d) of the batch the NEXT call will pass: its march starts now, beside this step (module docstring).
        error_inds [N] int64 (accelerate(error_map=)): each ray's flat cell of the map; omitted, no cell is updated.
        target [N,4] RGBA pixels with accelerate(target_channels=4): the step blends them over the rays' backgrounds (`trainer.gt_rgb` is the
        blended target afterwards, `trainer.last_bg` the backgrounds); bg [N,3] fp32 with accelerate(bg_color="given").
        Returns the loss as a device scalar that the NEXT call overwrites.  It is `step_group` with one batch."""
        self._check_batch(target, bg, False)
        # views, for contiguous rays: the hand-over of `next_rays` is recognised by the address of these tensors (a reshape of a non-contiguous
        # tensor would be a fresh copy with a fresh address every call)
        return self._steps(rays_o.reshape(1, -1, 3), rays_d.reshape(1, -1, 3), target.reshape(1, -1, self.target_channels), next_rays,
                           None if error_inds is None else error_inds.reshape(1, -1), None if bg is None else bg.reshape(1, -1, 3))

    def _steps(self, rays_o, rays_d, target, next_rays, error_inds=None, bg=None):
        """The k steps of one call, on ring slots g0 .. g0 + k: `step_group`, and `step` as its k = 1.  rays_o / rays_d: [k, N, 3]; target
        [k, N, target_channels]; bg: [k, N, 3] or None (`_check_batch` has seen both)."""
        r, k = self.renderer, rays_o.shape[0]
        assert rays_o.is_contiguous() and rays_d.is_contiguous(), "rays_o / rays_d must be contiguous tensors (next_rays are recognised by their address)"
        if error_inds is not None and self.error_map is None:
            raise ValueError("error_inds without a map: pass accelerate(..., error_map=) the tensor they index")
        if self.ema is not None and self.ema.swapped_in:
            raise RuntimeError("the EMA is swapped in (trainer.ema.copy_to() without restore()): the parameters are the average, not the weights being "
                               "trained; call trainer.ema.restore() before the next step")
        self._ensure_buffers(rays_o.shape[1])
        if self._lr_sched is not None:
            self._lr_sched.check(k)
        if not self.use_graph or self._primed < RING or self._warm < max(2, self.group):
            # the reference's first steps: full-size sample buffers until the ring holds a mean count (its update_extra_state cadence); then -- and
            # after every change of the buffer size -- eager steps at the size the graphs will be recorded with: two, or `group` of them, so that
            # the ring slot is a multiple of `group` when the graphs start
            assert self._ahead is None
            self._fill_backgrounds(r.local_step % RING, k, bg)
            for i in range(k):
                self._eager_step(rays_o[i], rays_d[i], target[i], None if error_inds is None else error_inds[i])
            return self.loss
        g0 = r.local_step
        assert k == self.group, "this trainer was built with steps_per_call > 1: call step_group"
        assert g0 % k == 0, "step_group and step must not be mixed once the graphs run (the ring slot must stay a multiple of steps_per_call)"
        if g0 == 0:
            self._ring_start()
        if self._graphs is None:
            self._capture()
        self._lr_guard()
        main = torch.cuda.current_stream()
        ahead, self._ahead = self._ahead, None
        if ahead is not None:
            main.wait_stream(self._side)  # marched beside the previous call
            if ahead != (g0, rays_o.data_ptr(), rays_d.data_ptr()):  # ... but other tensors: it is forgotten (the next call starts clean), this call refused
                raise AssertionError("next_rays of the previous call must be the rays of this call (same tensors)")
        else:
            self._ray_o[g0:g0 + k].copy_(rays_o, non_blocking=True), self._ray_d[g0:g0 + k].copy_(rays_d, non_blocking=True)
            for g in range(g0, g0 + k):
                self._graphs[g][0].replay()
        self._targets[g0:g0 + k].copy_(target, non_blocking=True)
        self._fill_backgrounds(g0, k, bg)
        self._set_error_inds(g0, k, error_inds)
        ready = None
        if next_rays is not None:
            ready = torch.cuda.Event()
            ready.record(main)  # everything enqueued so far (the production of the next rays, an occupancy update, this call's marches) -- NOT the rest of this call
        self._groups[g0 // k].replay()
        r.local_step = g0 + k
        self._published(g0 + k - 1)
        if self._lr_sched is not None:
            self._lr_sched.advance(k)
        if g0 + k < RING:
            if ready is not None:
                self._march_ahead(g0 + k, k, next_rays, ready)
        else:
            self._ring_end(ready)
            if ready is not None and self.march_across_ring_end and self._graphs is not None:  # (graphs dropped: the buffer size changed)
                self._march_ahead(0, k, next_rays, ready)
        return self.loss

    def _set_error_inds(self, slot, k, error_inds):
        """The map cells of the k steps at ring slots slot .. slot + k into their static buffers: -1 (no cell) where the caller names none."""
        if self._error_inds is None:
            return
        if error_inds is None:
            self._error_inds[slot:slot + k].fill_(-1)
        else:
            self._error_inds[slot:slot + k].copy_(error_inds.reshape(k, self.n_rays), non_blocking=True)

    def _eager_step(self, rays_o, rays_d, target, error_inds=None):
        """One step launched kernel by kernel, through the static buffers of its ring slot (graph=False keeps the same buffer-size policy)."""
        r = self.renderer
        g = r.local_step % RING
        if g == 0:
            self._ring_start()
        sized = self._primed >= RING
        (ro, rd), tg = self._rays[g], self._targets[g]
        ro.copy_(rays_o, non_blocking=True), rd.copy_(rays_d, non_blocking=True), tg.copy_(target, non_blocking=True)
        self._set_error_inds(g, 1, error_inds)
        marched, _ = self._march(ro, rd, mean_count=self._M if sized else None)
        self._shade(marched, g)
        self._published(g)
        if self._lr_sched is not None:
            self._lr_sched.advance(1)
        self._primed += 1
        self._warm += 1 if sized else 0
        if r.local_step == RING:
            r.update_mean_count()
            self._resize()

    def _ring_start(self):
        """Called before a step is issued at ring slot 0, eager or replayed (CurvedTrainer draws the ring's levels here)."""

    def sync(self):
        """Make the fp32 module parameters and the optimizer's moment tensors current (double-buffered optimizer state, `fused_table_update`): one
        4-byte read-back.  The 16-bit copies the kernels read are always current."""
        if self.fused:
            self.opt.sync()

    def _side_stream(self):
        if self._side is None:
            from .streams import side_stream

            self._side = side_stream(self.dev)  # the process-wide high-priority stream (streams.py: why it is shared)
        return self._side

    def _march_ahead(self, slot0, k, next_rays, ready):
        """The marches of the next call's k batches, into slots slot0 .. slot0 + k, on the side stream: behind `ready`, beside this call's kernels."""
        no, nd = next_rays
        assert no.is_contiguous() and nd.is_contiguous() and no.numel() == nd.numel() == k * self.n_rays * 3, \
            "next_rays: the contiguous rays of the next call (they are recognised by address there)"
        with torch.cuda.stream(self._side_stream()):
            self._side.wait_event(ready)
            self._ray_o[slot0:slot0 + k].copy_(no.view(k, -1, 3), non_blocking=True), self._ray_d[slot0:slot0 + k].copy_(nd.view(k, -1, 3), non_blocking=True)
            for g in range(slot0, slot0 + k):
                self._graphs[g][0].replay()
        self._ahead = (slot0, no.data_ptr(), nd.data_ptr())

    def _resize(self):
        """After a mean_count read-back: (re)choose the sample-buffer size; a change drops the graphs (eager steps at the new size, then a new capture)."""
        r = self.renderer
        if self._M == 0 or r.mean_count + 128 > self._M or r.mean_count < 0.8 * self._M:
            if self._M == 0:
                # the first ring ran on full-size buffers (N * max_steps rows, as the reference's first steps do): the library's scratch grew to
                # match -- gigabytes of binning records -- and would stay that size; give it back once, now that a sample count exists
                from nerftex_hip import check, lib

                torch.cuda.synchronize()
                check(lib.nerftex_release_workspaces())
            self._M = (r.mean_count + 4095) // 4096 * 4096 + 4096
            self._graphs, self._groups, self._warm = None, None, 0


def _host_lrs(opt):
    return [None if isinstance(g["lr"], torch.Tensor) else float(g["lr"]) for g in opt.param_groups]


LOSS_KINDS = {"mse": 0, "l1": 1, "huber": 2}  # NERFTEX_LOSS_MSE / _L1 / _HUBER of include/nerftex_hip.h


def parse_criterion(criterion):
    """-> (kind, param) of a nerftex_step_loss_desc.  Accepted: "mse", "l1", ("huber", delta) with a finite delta > 0; an already parsed
    (kind, param); and the reference Trainer's own `criterion=` objects -- torch.nn.MSELoss, L1Loss, HuberLoss instances with reduction 'mean'
    or 'none' (the reference takes .mean(-1).mean() of the unreduced loss: rows of equal length, so the same number).  Anything else -- reduction
    'sum', other modules, bare callables -- is a ValueError: the kernels would train another objective.  Host only."""
    import math

    accepted = ('criterion: "mse", "l1", ("huber", delta > 0), or a torch.nn.MSELoss / L1Loss / HuberLoss instance with reduction "mean" or "none"')

    def huber(delta):
        if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not (math.isfinite(delta) and delta > 0):
            raise ValueError(f"{accepted}; got a Huber delta of {delta!r}")
        return LOSS_KINDS["huber"], float(delta)

    if isinstance(criterion, str):
        if criterion in ("mse", "l1"):
            return LOSS_KINDS[criterion], 0.0
        raise ValueError(f"{accepted}; got {criterion!r}" + (" (Huber needs its delta)" if criterion == "huber" else ""))
    if isinstance(criterion, tuple) and len(criterion) == 2:
        if criterion[0] == "huber":
            return huber(criterion[1])
        if not isinstance(criterion[0], bool) and isinstance(criterion[0], int) and criterion[0] in LOSS_KINDS.values():
            return huber(criterion[1]) if criterion[0] == LOSS_KINDS["huber"] else (int(criterion[0]), 0.0)
        raise ValueError(f"{accepted}; got {criterion!r}")
    if isinstance(criterion, torch.nn.Module):
        kinds = {torch.nn.MSELoss: "mse", torch.nn.L1Loss: "l1", torch.nn.HuberLoss: "huber"}
        name = kinds.get(type(criterion))
        if name is None:
            raise ValueError(f"{accepted}; got a {type(criterion).__name__}")
        if criterion.reduction not in ("mean", "none"):
            raise ValueError(f"{accepted}; got reduction={criterion.reduction!r}")
        return huber(criterion.delta) if name == "huber" else (LOSS_KINDS[name], 0.0)
    raise ValueError(f"{accepted}; got {criterion!r}")


def _refuse_options(lr_scheduler, pipeline_adam, ema_decay=None):
    """What neither trainer does is refused at construction, before the renderer is looked at: the removed pipeline_adam (the keyword stays so
    that callers passing 0 keep working), an ema_decay that is not a float in (0, 1), and a learning-rate schedule where the rate cannot be
    read from the device schedule -- never run at a constant rate instead."""
    from .ema import check_decay

    check_decay(ema_decay)
    if pipeline_adam:
        raise ValueError(f"pipeline_adam={pipeline_adam!r}: pipelined Adam was removed (built, bit-identical, measured slower, and GradScaler could no "
                         "longer skip a whole step: DESIGN_HISTORY.md, VERDICT r4 item 2 row; profiles/r05_pipeline_adam.json); pass 0 or leave it out")
    if lr_scheduler is None:
        return
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError("lr_scheduler: the device learning-rate schedule is single-process (world size 1)")


def draw_ring_levels(num_levels, count=RING):
    """The hash-grid levels the reference's clustering_loss picks in `count` consecutive training steps: its own call,
    np.random.choice(np.arange(L), [1]) once per step, in step order (gridencoder/grid_clustering.py:204-207) -- after the same
    np.random.seed, the same levels as the reference trainer.  Host only; int32 [count]."""
    import numpy as np

    return np.array([int(np.random.choice(np.arange(num_levels), [1])[0]) for _ in range(count)], dtype=np.int32)


def normal_cosine_loss(normal_grad, normal_est, threshold=None):
    """nerf/utils.py:646-657 on the per-ray composited normals [N,3]: -mean(min(n_grad . n_est, cos(pi / 8))) over the rays whose supervising
    normal is a number, both normalised with + 1e-5.  The reference selects those rays with a boolean mask (a read-back of their count); here
    they are selected with torch.where and counted on the device: nothing is read back and the expression can be recorded into a graph.  No
    such ray: 0 / 0, not a number, as the reference's mean over an empty selection."""
    import math

    threshold = math.cos(math.pi / 8) if threshold is None else threshold
    normal_grad = normal_grad.detach().float()
    normal_est = normal_est.float()
    valid = torch.logical_not(normal_grad.isnan().any(dim=-1))
    g = torch.where(valid.unsqueeze(-1), normal_grad, torch.zeros_like(normal_grad))
    e = torch.where(valid.unsqueeze(-1), normal_est, torch.zeros_like(normal_est))
    g = g / (g.norm(dim=-1, keepdim=True) + 1e-5)
    e = e / (e.norm(dim=-1, keepdim=True) + 1e-5)
    cos = torch.minimum((g * e).sum(dim=-1), torch.full_like(g[..., 0], threshold))
    return -torch.where(valid, cos, torch.zeros_like(cos)).sum() / valid.sum()


class CurvedTrainer(AcceleratedTrainer):
    """accelerate() of a Renderer over `curved.CurvedField`: the NeRF-Texture training step (main.py:85-190, nerf/utils.py:637-666) --
    image loss + regular_weight * clustering loss, torch's fused capturable Adam over field.get_params(lr) (cluster centres included) under
    GradScaler -- with the structure of the ngp field's trainer: a march graph and a shade graph per ring slot, `steps_per_call` groups,
    `next_rays` march-ahead.  The regulariser is the step form of nerftex_grid_cluster_loss, run inside the shade graph after the backward
    and before the optimizer: it ADDS scale * d reg / d x into the fp32 table gradient and the centres' gradient (never through an fp16
    gradient: at 1e-8 / (2^19 * 4) it would flush to zero).  The level of each step of a ring is drawn at the ring's start with the
    reference's own np.random call (draw_ring_levels) into a device int32[16] the slot graphs index.  trainer.loss = image loss + regulariser,
    trainer.reg_loss = the regulariser: device scalars, nothing is read back.  The fp32 parameters are current after every step (no sync()).
    criterion="l1" is main.py:187's (the reference trains this field with torch.nn.L1Loss; the default stays the MSE); error_map= is its
    --error_map (nerf/utils.py:617-632).
    normal_loss=True (a field with light_model="SH"): the step adds the reference's cosine term on the per-ray composited normals
    (nerf/utils.py:650-657, `normal_cosine_loss`); trainer.normal_loss is its value, a device scalar.
    Not here: prob_model (the log-variance table), world size > 1, and the ngp field's fused AMP options (HalfLeafAdam, fused table update,
    dead-sample skipping, the one-launch composite step), which are refused if asked for."""

    def __init__(self, renderer, regular_weight=1e-8, rays_per_batch=None, lr=1e-2, betas=(0.9, 0.99), eps=1e-15, dt_gamma=1 / 128, bg_color=1,
                 perturb=True, max_steps=1024, amp_dtype=torch.float16, graph=True, steps_per_call=1, march_across_ring_end=False, pipeline_adam=0,
                 skip_dead_samples=None, fused_table_update=None, fused_composite_step=None, lr_scheduler=None, total_steps=None, criterion=None,
                 error_map=None, ema_decay=None, target_channels=3, bg_generator=None, normal_loss=False):
        from .curved import CurvedField

        _refuse_options(lr_scheduler, pipeline_adam, ema_decay)
        self._init_pixels(bg_color, target_channels, bg_generator)
        self._init_criterion(criterion, error_map)

        field = renderer.field
        assert isinstance(field, CurvedField), "CurvedTrainer trains a curved.CurvedField"
        if getattr(field, "imported", False):
            raise NotImplementedError("CurvedTrainer: the field renders an imported feature map (CurvedField.import_field); import mode is for rendering -- "
                                      "switch_import() back to the mesh field to train")
        assert field.encoder_var is None, "accelerate(): prob_model=True (the log-variance table) is not on the graphed path (main.py:86 trains without it)"
        assert not normal_loss or getattr(field, "light_model", None) == "SH", "accelerate(normal_loss=True) supervises the fine normal of CurvedField(light_model='SH')"
        self.use_normal_loss = bool(normal_loss)
        dist = torch.distributed
        assert not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1), "accelerate() of the curved field: world size 1"
        for name, v in (("skip_dead_samples", skip_dead_samples), ("fused_table_update", fused_table_update), ("fused_composite_step", fused_composite_step)):
            assert not v, f"{name}: an option of the ngp field's fused AMP step; the curved field trains with torch's fused Adam + GradScaler"
        self._init_loop(renderer, field, rays_per_batch, dt_gamma, bg_color, perturb, max_steps, amp_dtype, graph, steps_per_call, march_across_ring_end)
        self.fused, self.amp = False, None
        self.skip_dead_samples = self.fused_table_update = self.fused_composite_step = False
        renderer.skip_dead_samples, renderer.root_one, renderer.defer_step_loss = False, None, False
        # (capturable either way: graph=False runs the very optimizer arithmetic the graphs replay)
        self.opt = torch.optim.Adam(field.get_params(lr), betas=betas, eps=eps, fused=True, capturable=True)
        self.scaler = torch.amp.GradScaler("cuda", enabled=amp_dtype in (torch.float16, torch.bfloat16))
        # the regulariser: static level picks of the ring's 16 steps, the centres' gradient as one [L, K, C] buffer the per-level parameters'
        # .grad are views of (zeroed every step, never set to None: the kernel adds into it), its loss
        enc = field.encoder
        self.regular_weight = float(regular_weight)
        self._layers = list(enc.cluster_layers)
        self._alpha = float(self._layers[0].alpha)
        assert all(float(l.alpha) == self._alpha for l in self._layers)
        self._levels = torch.zeros(RING, dtype=torch.int32, device=self.dev)
        self.ring_levels = None  # (the host copy of the current ring's picks)
        centres = [l.cluster_centers for l in self._layers]
        self._centres_grad = torch.zeros((len(centres),) + tuple(centres[0].shape), dtype=torch.float32, device=self.dev)
        for i, c in enumerate(centres):
            c.grad = self._centres_grad[i]
        keep = {id(c) for c in centres}
        self._other_params = [p for p in field.parameters() if id(p) not in keep]
        self.reg_loss = torch.zeros((), dtype=torch.float32, device=self.dev)
        self.normal_loss = torch.zeros((), dtype=torch.float32, device=self.dev)
        self._attach_schedule(lr_scheduler, total_steps)  # (the optimizer's learning rates become fp32 tensors the schedule writes)
        self._attach_ema(ema_decay)

    def _ring_start(self):
        self.ring_levels = draw_ring_levels(self.field.encoder.num_levels)
        self._levels.copy_(torch.from_numpy(self.ring_levels))  # (stream-ordered behind the previous ring's steps)

    def _shade(self, marched, slot):
        r, enc = self.renderer, self.field.encoder
        for p in self._other_params:
            p.grad = None
        self._centres_grad.zero_()
        extras = {} if self.use_normal_loss else None
        with torch.autocast("cuda", dtype=self.amp_dtype):
            image, depth, loss, scaled = r.shade_train(marched, self._bg_arg(slot), target=self._targets[slot], scale=None, extras_out=extras,
                                                       **self._loss_args(slot))[:4]
        if extras is not None:
            normal_error = normal_cosine_loss(extras["normal_grad"], extras["normal"])
            self.normal_loss.copy_(normal_error.detach())
            scaled, loss = scaled + normal_error, loss + normal_error.detach()
        self.scaler.scale(scaled).backward()
        from gridencoder.grid_clustering import grid_cluster_step

        grid_cluster_step(enc.embeddings.detach(), enc.offsets, torch.stack([l.cluster_centers.detach() for l in self._layers]), self._levels[slot],
                          self._alpha, self.regular_weight, loss=self.reg_loss, grad_table=enc.embeddings.grad, grad_centres=self._centres_grad,
                          grad_scale=self.scaler.scale(self._one))
        if self._lr_sched is not None:
            self._lr_sched.publish()
        self.scaler.step(self.opt)
        self.scaler.update()
        self.loss.copy_(loss.detach().reshape(()) + self.reg_loss)
        if self.ema is not None:
            self.ema.update()


def accelerate(renderer, **kw):
    """See the module docstring.  Keyword arguments: rays_per_batch, lr, betas, eps, dt_gamma, bg_color, perturb, max_steps, amp_dtype, graph,
    steps_per_call (k > 1: `step_group` takes the batches of k consecutive steps and replays one graph for them), march_across_ring_end,
    lr_scheduler + total_steps (a factory `lambda optimizer: LambdaLR(optimizer, lr_lambda)`, as the reference's Trainer takes it, and the number
    of training steps its device table covers: every step, replayed or eager, trains at the rate LambdaLR gives it; `trainer.lr_scheduler`),
    criterion ("mse" -- the default --, "l1", ("huber", delta), or the reference Trainer's MSELoss / L1Loss / HuberLoss object: `parse_criterion`)
    and error_map (a contiguous fp32 device tensor updated in place as 0.1 * old + 0.9 * ray loss at the cells `step(..., error_inds=)` names; the
    map is written by every step, skipped by the loss scaler or not; `trainer.ray_loss` is the last step's per-ray loss),
    ema_decay (a float in (0, 1), the reference Trainer's 0.95: `trainer.ema` is an ema.DeviceEMA -- torch_ema's interface -- whose update is the
    last launch of every step, applied or skipped; None, the default: no average),
    bg_color (a number, the default 1; "random": the reference's per-pixel torch.rand_like background, one torch.rand of [k,N,3] per call in front
    of the replay, seeded by bg_generator; "given": `step(..., bg=[N,3])` / `step_group(..., bg=[k,N,3])` pass it) and target_channels (3, or 4:
    the batches are RGBA pixels [N,4] the step blends over the background, nerf/utils.py:602-615; `trainer.gt_rgb` / `trainer.last_bg` are the
    last step's blended target and background).  Not here: color_space == 'linear', the background network (bg_radius > 0), gradients to the
    background or to alpha; eval_step's blend over white is one torch expression on the caller's side.
    A renderer over a curved.CurvedField gets a CurvedTrainer (its docstring; regular_weight, default 1e-8)."""
    from .curved import CurvedField

    if isinstance(renderer.field, CurvedField):
        return CurvedTrainer(renderer, **kw)
    return AcceleratedTrainer(renderer, **kw)
