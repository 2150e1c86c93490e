"""GPU: per-step learning-rate schedules on the graphed training path (ngp_harness/lr_schedule.py).

  * the C ABI: nerftex_adam_mixed_step_amp[_db]_sched and nerftex_table_adam.sched against the unscheduled calls fed base * factor[t] -- the
    same parameters, moments and 16-bit leaves, bit for bit, over steps that include a skipped one (the counter advances, Adam's step does not);
  * accelerate(..., lr_scheduler=reference-style LambdaLR factory) with replayed graphs against the same trainer run eagerly with a host LambdaLR
    over trainer.opt stepped after every step -- fp16 and bf16 FFMLP fields, the nn.Linear (SplitKLinear) field, torch's fused Adam fallback and
    the curved field; a constant schedule against no schedule; resuming from a checkpoint; the stale-rate guard.
The reference's schedule: LambdaLR(optimizer, lambda iter: 0.1 ** min(iter / opt.iters, 1)), stepped after every optimizer step, skipped ones
included (main_nerf.py:131-133, nerf/utils.py:1020-1025).
"""
import ctypes

import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import LambdaLR

pytestmark = pytest.mark.gpu

TOTAL = 48


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _lam(total=TOTAL):
    return lambda it: 0.1 ** min(it / total, 1)  # main_nerf.py:133 with a short horizon: the rate moves every step


def _arr(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _schedule(dev, n_steps, start=0):
    from nerftex_hip import LrSchedule

    factor = torch.tensor([_lam(n_steps)(t) for t in range(n_steps + 1)], dtype=torch.float64, device=dev)
    it = torch.full((), start, dtype=torch.int32, device=dev)
    return factor, it, LrSchedule(factor.data_ptr(), factor.numel(), it.data_ptr())


# ------------------------------------------------------------------------------------------------------------------------- 1. the C ABI
@pytest.mark.parametrize("double_buffered", [False, True], ids=["amp", "amp_db"])
def test_sched_entries_equal_the_plain_ones_fed_the_product(dev, double_buffered):
    from nerftex_hip import check, lib, ptr, stream

    n_t, n_w, base = 100003 * 2, 7168, 1e-2
    hyper = (0.9, 0.99, 1e-15)
    amp_consts = (2.0, 0.5, 3)
    factor, it, desc = _schedule(dev, 8, start=2)

    def fresh():
        g = torch.Generator(device=dev).manual_seed(5)
        st = {"p": (torch.rand(n_t, device=dev, generator=g) - 0.5) * 1e-2, "wp": torch.rand(n_w, device=dev, generator=g) - 0.5}
        for k in ("p", "wp"):
            st[k[:-1] + "m"], st[k[:-1] + "v"] = torch.zeros_like(st[k]), torch.zeros_like(st[k])
            st[k[:-1] + "h"] = st[k].half() if k == "p" else st[k].bfloat16()
            st[k + "1"], st[k[:-1] + "m1"], st[k[:-1] + "v1"] = [torch.full_like(st[k], float("nan")) for _ in range(3)]
        st.update(step=torch.zeros((), device=dev), scale=torch.full((), 65536.0, device=dev), tracker=torch.zeros((), dtype=torch.int32, device=dev),
                  found=torch.zeros((), device=dev), ticket=torch.zeros((), dtype=torch.int32, device=dev), live=torch.zeros((), dtype=torch.int32, device=dev))
        return st

    def grads(step):
        g = torch.Generator(device=dev).manual_seed(100 + step)
        return (torch.randn(n_t, device=dev, generator=g) * 3e-2).half(), (torch.randn(n_w, device=dev, generator=g) * 1e-1).bfloat16()

    def run(sched):
        st = fresh()
        n = (ctypes.c_uint64 * 2)(n_t, n_w)
        for step in range(6):
            gt, gw = grads(step)
            if step == 3:
                st["found"].fill_(1.0)  # a skipped step
            lr = base * factor[min(2 + step, 8)].item()
            tail = (ptr(st["scale"]), ptr(st["tracker"]), ptr(st["found"]), ptr(st["ticket"]), *amp_consts)
            p0 = (_arr([st["p"], st["wp"]]), _arr([st["m"], st["wm"]]), _arr([st["v"], st["wv"]]))
            if double_buffered:
                sets = p0 + (_arr([st["p1"], st["wp1"]]), _arr([st["m1"], st["wm1"]]), _arr([st["v1"], st["wv1"]]))
                common = (2, *sets, _arr([gt, gw]), _arr([st["h"], st["wh"]]), n, 0b10, ptr(st["step"]))
                rest = (*hyper, *tail, ptr(st["live"]), None, None, None, 0, stream())
                if sched:
                    check(lib.nerftex_adam_mixed_step_amp_db_sched(*common, base, ctypes.byref(desc), *rest))
                else:
                    check(lib.nerftex_adam_mixed_step_amp_db(*common, lr, *rest))
            else:
                common = (2, *p0, _arr([gt, gw]), _arr([st["h"], st["wh"]]), n, 0b10, ptr(st["step"]))
                if sched:
                    check(lib.nerftex_adam_mixed_step_amp_sched(*common, base, ctypes.byref(desc), *hyper, *tail, stream()))
                else:
                    check(lib.nerftex_adam_mixed_step_amp(*common, lr, *hyper, *tail, stream()))
        torch.cuda.synchronize()
        return st

    it.fill_(2)
    a, b = run(False), run(True)
    assert int(it) == 2 + 6, "the schedule's counter advances on every step, the skipped one included"
    assert float(a["step"]) == float(b["step"]) == 5.0, "Adam's step count does not advance on the skipped step"
    for k in ("p", "m", "v", "h", "wp", "wm", "wv", "wh", "p1", "m1", "v1", "wp1", "wm1", "wv1", "scale", "tracker", "live"):
        assert torch.equal(_bits(a[k]) if a[k].is_floating_point() else a[k], _bits(b[k]) if b[k].is_floating_point() else b[k]), k


@pytest.mark.parametrize("align_corners", [0, 1])
def test_table_adam_sched_equals_the_plain_table_adam_fed_the_product(dev, oracle, align_corners):
    """nerftex_grid_encode_backward_adam with nerftex_table_adam.sched (the hashed rows' update reads the step's rate) + the closing
    nerftex_adam_mixed_step_amp_db_sched, against both calls without a schedule at lr = base * factor[t]: same state sets, fp16 table, bits."""
    from nerftex_hip import F16, LAYOUT_BLC, LAYOUT_GRAD_OVERWRITE, TableAdam, check, lib, ptr, stream

    off_np, rows = oracle.grid_offsets(3, 16, 1.447269, 16, 19, bool(align_corners))
    off = torch.from_numpy(off_np).to(dev)
    check(lib.nerftex_grid_register_offsets(ptr(off), 16, off_np.ctypes.data))
    S = float(np.log2(1.447269))
    B, base = 65536, 1e-2
    hyper = (0.9, 0.99, 1e-15)
    amp_consts = (2.0, 0.5, 3)
    x = torch.rand(B, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(B)) * 4 - 2
    factor, it, desc = _schedule(dev, 6)

    def run(sched):
        g = torch.Generator(device=dev).manual_seed(5)
        p = (torch.rand(rows, 2, device=dev, generator=g) - 0.5) * 1e-2
        sets = {"p": [p, torch.full_like(p, float("nan"))], "m": [torch.zeros_like(p), torch.full_like(p, float("nan"))],
                "v": [torch.zeros_like(p), torch.full_like(p, float("nan"))]}
        h = p.half()
        step, scale, found = torch.zeros((), device=dev), torch.full((), 65536.0, device=dev), torch.zeros((), device=dev)
        tracker, ticket, live = [torch.zeros((), dtype=torch.int32, device=dev) for _ in range(3)]
        ta = TableAdam()
        for k in range(2):
            ta.param[k], ta.exp_avg[k], ta.exp_avg_sq[k] = sets["p"][k].data_ptr(), sets["m"][k].data_ptr(), sets["v"][k].data_ptr()
        ta.param_half, ta.live, ta.step, ta.grad_scale, ta.found_inf = h.data_ptr(), live.data_ptr(), step.data_ptr(), scale.data_ptr(), found.data_ptr()
        ta.beta1, ta.beta2, ta.eps = hyper
        it.zero_()
        for t in range(5):
            gx = (torch.randn(B, 32, device=dev, generator=torch.Generator(device=dev).manual_seed(1000 + t)) * 3e-2).half()
            if t == 2:
                gx[B // 3, 9] = float("inf")  # skipped
            if sched:
                ta.lr, ta.sched = base, ctypes.addressof(desc)
            else:
                ta.lr, ta.sched = base * factor[t].item(), None
            gt = torch.full((rows, 2), float("nan"), dtype=torch.float16, device=dev)
            first = ctypes.c_uint32(12345)
            check(lib.nerftex_grid_encode_backward_adam(ptr(gx), ptr(x), ptr(off), ptr(gt), B, 3, 2, 16, S, 16, 0, align_corners, F16,
                                                        LAYOUT_BLC | LAYOUT_GRAD_OVERWRITE, 2.0, 0.25, ctypes.byref(ta), ctypes.byref(first), stream()))
            f = int(first.value)
            n = (ctypes.c_uint64 * 1)(f * 2)
            cut = lambda t_: t_[:f]  # noqa: E731
            args = (1, *[_arr([cut(sets[k][j])]) for j in range(2) for k in ("p", "m", "v")], _arr([cut(gt)]), _arr([cut(h)]), n, 0, ptr(step))
            tail = (ptr(scale), ptr(tracker), ptr(found), ptr(ticket), *amp_consts, ptr(live), ptr(h[f:]), ptr(sets["p"][0][f:]), ptr(sets["p"][1][f:]),
                    (rows - f) * 2, stream())
            if sched:
                check(lib.nerftex_adam_mixed_step_amp_db_sched(*args, base, ctypes.byref(desc), *hyper, *tail))
            else:
                check(lib.nerftex_adam_mixed_step_amp_db(*args, ta.lr, *hyper, *tail))
        torch.cuda.synchronize()
        return sets, h, float(step), int(live), int(it)

    a, b = run(False), run(True)
    assert b[4] == 5 and a[2] == b[2] == 4.0 and a[3] == b[3]
    k = a[3]
    for name in ("p", "m", "v"):
        assert torch.equal(_bits(a[0][name][k]), _bits(b[0][name][k])), name
    assert torch.equal(_bits(a[1]), _bits(b[1]))


def test_publish_writes_lambdalrs_fill(dev):
    """nerftex_lr_schedule_publish: (float)(base_g * factor[t]) into each fp32 lr tensor -- what LambdaLR's group["lr"].fill_() stores -- then t += 1."""
    from nerftex_hip import check, lib, stream

    factor, it, desc = _schedule(dev, TOTAL)
    bases = [1e-2, 3.3e-4, 7e-3]
    outs = [torch.zeros((), device=dev) for _ in bases]
    host = LambdaLR(torch.optim.SGD([{"params": [torch.zeros(1, requires_grad=True)], "lr": b} for b in bases]), _lam())
    want = [torch.zeros((), device=dev) for _ in bases]
    for t in range(TOTAL + 3):
        check(lib.nerftex_lr_schedule_publish(ctypes.addressof(desc), (ctypes.c_double * 3)(*bases), _arr(outs), 3, stream()))
        for w, v in zip(want, host.get_last_lr() if t <= TOTAL else [b * factor[-1].item() for b in bases]):
            w.fill_(v)
        assert all(torch.equal(_bits(o), _bits(w)) for o, w in zip(outs, want)), t
        if t < TOTAL:
            host.optimizer.step()
            host.step()
    assert int(it) == TOTAL + 3


# ------------------------------------------------------------------------------------------------------------------------- 2-3. trainers
def _ngp(dev, kind):
    from ngp_harness import scene
    from ngp_harness.model import NGPField, Renderer

    sc = scene.Scene(bound=2.0, seed=0)
    grid, _, _ = sc.bitfield()
    torch.manual_seed(0)
    if kind in ("fp16", "fp16_two_launch"):
        field = NGPField(bound=2.0, mlp="ffmlp", fused_glue=True)
    elif kind == "bf16":
        field = NGPField(bound=2.0, mlp="ffmlp", fused_glue=True, mlp_dtype=torch.bfloat16)
    elif kind == "split_k":
        field = NGPField(bound=2.0, mlp="torch")
    else:
        field = NGPField(bound=2.0, mlp="torch", split_k_linear=False)
    field = field.to(dev).train()
    torch.manual_seed(1)
    field.encoder.embeddings.data.uniform_(-1e-4, 1e-4)
    r = Renderer(field, bound=2.0, min_near=0.2).to(dev)
    r.set_occupancy(torch.from_numpy(grid).to(dev))
    return field, r


def _batches(dev, n=4096, n_pool=8):
    from ngp_harness import scene

    pool = []
    for j in range(n_pool):
        o, d = scene.train_batch(n, seed=500 + j, n_views=2)
        pool.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
    gt = torch.rand(n_pool, n, 3, generator=torch.Generator().manual_seed(23)).to(dev)
    return pool, gt


def _kw(kind):
    return {"amp_dtype": torch.bfloat16} if kind == "bf16" else ({"fused_table_update": False} if kind == "fp16_two_launch" else {})


def _overflow(tr):
    if tr.amp is not None:
        tr.amp.scale.fill_(2.0 ** 31)
    else:
        tr.scaler._scale.fill_(2.0 ** 31)


def _state(tr, field):
    torch.cuda.synchronize()
    tr.sync()
    out = {"param." + n: p.detach().clone() for n, p in field.named_parameters()}
    if tr.fused:
        for i in range(len(tr.opt.masters)):
            out[f"m{i}"], out[f"v{i}"], out[f"leaf{i}"] = tr.opt.exp_avg[i].clone(), tr.opt.exp_avg_sq[i].clone(), tr.opt.leaves[i].detach().clone()
        out["step"] = tr.opt.step_count.clone()
    else:
        for i, (p, st) in enumerate(tr.opt.state.items()):
            out[f"m{i}"], out[f"v{i}"], out[f"step{i}"] = st["exp_avg"].clone(), st["exp_avg_sq"].clone(), st["step"].clone()
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert torch.equal(_bits(x) if x.dtype in (torch.float32, torch.float16, torch.bfloat16) else x,
                           _bits(y) if y.dtype in (torch.float32, torch.float16, torch.bfloat16) else y), k


def _run_scheduled(dev, make, kind, k=4, steps=TOTAL, overflow_at=28, factory=None, **kw):
    """The scheduled trainer: graphs, steps_per_call k, `steps` steps, the loss scale forced to overflow at step `overflow_at`."""
    from ngp_harness.accelerate import accelerate

    pool, gt = _batches(dev)
    field, r = make(dev, kind)
    tr = accelerate(r, dt_gamma=1 / 128, steps_per_call=k, lr_scheduler=factory or (lambda opt: LambdaLR(opt, _lam())), total_steps=TOTAL, **_kw(kind), **kw)
    for c in range(steps // k):
        if c * k == overflow_at:
            _overflow(tr)
        idx = [(c * k + i) % len(pool) for i in range(k)]
        if k == 1:
            tr.step(*pool[idx[0]], gt[idx[0]])
        else:
            tr.step_group(torch.stack([pool[i][0] for i in idx]), torch.stack([pool[i][1] for i in idx]), gt[idx])
    assert tr._graphs is not None, "the later steps ran as replayed graphs"
    return tr, field


def _run_host_lambdalr(dev, make, kind, steps=TOTAL, overflow_at=28, tensor_lr=False, **kw):
    """The yardstick: graph=False, one step per call, a host LambdaLR over trainer.opt stepped after every step (what works without the feature)."""
    from ngp_harness.accelerate import accelerate

    pool, gt = _batches(dev)
    field, r = make(dev, kind)
    tr = accelerate(r, dt_gamma=1 / 128, graph=False, **_kw(kind), **kw)
    host = LambdaLR(tr.opt, _lam())
    if tensor_lr:  # torch's fused Adam reading an fp32 tensor lr that LambdaLR fills
        for g in tr.opt.param_groups:
            g["lr"] = torch.tensor(g["lr"], dtype=torch.float32, device=dev)
    for t in range(steps):
        if t == overflow_at:
            _overflow(tr)
        tr.step(*pool[t % len(pool)], gt[t % len(pool)])
        host.step()
    return tr, field, host


@pytest.mark.parametrize("kind", ["fp16", "fp16_two_launch", "bf16", "split_k", "torch_adam"])
def test_scheduled_graphs_train_like_an_eager_host_lambdalr(dev, kind):
    tr, field = _run_scheduled(dev, _ngp, kind)
    assert tr.fused == (kind != "torch_adam") and tr.fused_table_update == (kind in ("fp16", "bf16"))
    ref, ref_field, host = _run_host_lambdalr(dev, _ngp, kind, tensor_lr=kind == "torch_adam")
    a, b = _state(tr, field), _state(ref, ref_field)
    if tr.fused:
        assert float(a["step"]) < TOTAL, "the forced overflow skipped a step"
        assert int(tr.opt.lr_schedule.iter) == TOTAL, "... and the schedule counted it"
    _assert_same(a, b)
    assert tr.lr_scheduler.state_dict() == host.state_dict() or kind == "torch_adam"
    assert tr.lr_scheduler.last_epoch == TOTAL and tr.lr_scheduler.get_last_lr() == [b * _lam()(TOTAL) for b in host.base_lrs]


def _curved(dev, like=None):
    from ngp_harness.curved import CurvedField, star_flower_mesh
    from ngp_harness.model import Renderer

    v, f = star_flower_mesh(n_lat=36, n_lon=72)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05).to(dev)
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    if like is not None:  # (the same field and occupancy state in both runs: tests/test_gpu_curved_training.py)
        r.load_state_dict(like.state_dict())
        r.mean_density = like.mean_density
    else:
        with torch.autocast("cuda", dtype=torch.float16):
            r.update_extra_state_device()
    field.train()
    return field, r


def test_scheduled_curved_trainer_trains_like_an_eager_host_lambdalr(dev):
    _, r0 = _curved(dev)
    make = lambda dev_, kind: _curved(dev_, like=r0)  # noqa: E731
    np.random.seed(7)
    tr, field = _run_scheduled(dev, make, "curved", perturb=False)
    np.random.seed(7)
    ref, ref_field, host = _run_host_lambdalr(dev, make, "curved", tensor_lr=True, perturb=False)
    assert all(isinstance(g["lr"], torch.Tensor) for g in tr.opt.param_groups)
    assert float(tr.scaler.get_scale()) < 2.0 ** 31
    _assert_same(_state(tr, field), _state(ref, ref_field))
    # (a tensor lr holds the rate of the last step launched -- nerftex_lr_schedule_publish runs in front of the optimizer -- where the host
    # LambdaLR has already filled in the next one; the host mirror, trainer.lr_scheduler, holds the next one)
    assert [float(g["lr"]) for g in tr.opt.param_groups] == [float(torch.tensor(b * _lam()(TOTAL - 1), dtype=torch.float32)) for b in host.base_lrs]
    assert tr.lr_scheduler.get_last_lr() == [b * _lam()(TOTAL) for b in host.base_lrs]


def test_constant_schedule_is_no_schedule(dev):
    from ngp_harness.accelerate import accelerate

    tr, field = _run_scheduled(dev, _ngp, "fp16", factory=lambda opt: LambdaLR(opt, lambda t: 1.0))
    pool, gt = _batches(dev)
    f2, r2 = _ngp(dev, "fp16")
    t2 = accelerate(r2, dt_gamma=1 / 128, steps_per_call=4)
    for c in range(TOTAL // 4):
        if c * 4 == 28:
            _overflow(t2)
        idx = [(c * 4 + i) % len(pool) for i in range(4)]
        t2.step_group(torch.stack([pool[i][0] for i in idx]), torch.stack([pool[i][1] for i in idx]), gt[idx])
    _assert_same(_state(tr, field), _state(t2, f2))


def test_resume_restores_the_schedule(dev, tmp_path):
    """Train 24 scheduled steps, save with lr_scheduler=, load into a fresh scheduled trainer and train 24 more: the saved entry is
    LambdaLR.state_dict()'s, last_epoch 24 lands in the device counter, and the resumed run trains like the same checkpoint resumed into an eager
    trainer whose host LambdaLR loads that entry and steps after every step.  (Against 48 uninterrupted steps a resumed run differs with or
    without a schedule: a fresh trainer primes on full-size sample buffers again; that is the checkpoint path's, not the schedule's.)"""
    from ngp_harness import checkpoint
    from ngp_harness.accelerate import accelerate

    half, _ = _run_scheduled(dev, _ngp, "fp16", k=1, steps=TOTAL // 2, overflow_at=-1)
    path = str(tmp_path / "ck.pth")
    saved = checkpoint.save_checkpoint(path, half.renderer, optimizer=half.opt, scaler=half.amp, lr_scheduler=half.lr_scheduler)
    ref_keys = LambdaLR(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=1.0), _lam()).state_dict().keys()
    assert saved["lr_scheduler"].keys() == ref_keys and saved["lr_scheduler"]["last_epoch"] == TOTAL // 2

    fr, rr = _ngp(dev, "fp16")
    res = accelerate(rr, dt_gamma=1 / 128, lr_scheduler=lambda opt: LambdaLR(opt, _lam()), total_steps=TOTAL)
    checkpoint.load_checkpoint(path, rr, optimizer=res.opt, scaler=res.amp, lr_scheduler=res.lr_scheduler)
    assert res.lr_scheduler.last_epoch == TOTAL // 2 and int(res.opt.lr_schedule.iter) == TOTAL // 2
    fe, re_ = _ngp(dev, "fp16")
    ref = accelerate(re_, dt_gamma=1 / 128, graph=False)
    host = LambdaLR(ref.opt, _lam())
    checkpoint.load_checkpoint(path, re_, optimizer=ref.opt, scaler=ref.amp, lr_scheduler=host)
    assert host.last_epoch == TOTAL // 2 and ref.opt.param_groups[0]["lr"] == res.opt.param_groups[0]["lr"] == 1e-2 * _lam()(TOTAL // 2)
    pool, gt = _batches(dev)
    for t in range(TOTAL // 2, TOTAL):
        res.step(*pool[t % len(pool)], gt[t % len(pool)])
        ref.step(*pool[t % len(pool)], gt[t % len(pool)])
        host.step()
    assert res._graphs is not None
    _assert_same(_state(res, fr), _state(ref, fe))
    assert res.lr_scheduler.state_dict() == host.state_dict()


def test_stale_rate_guard(dev):
    """No schedule: the replayed graphs hold the rate of their capture -- a changed param_groups lr makes the next replay raise."""
    from ngp_harness.accelerate import accelerate

    pool, gt = _batches(dev)
    field, r = _ngp(dev, "fp16")
    tr = accelerate(r, dt_gamma=1 / 128)
    for t in range(20):
        tr.step(*pool[t % len(pool)], gt[t % len(pool)])
    assert tr._graphs is not None
    tr.opt.param_groups[0]["lr"] *= 0.5
    with pytest.raises(RuntimeError, match="captured"):
        tr.step(*pool[0], gt[0])
    torch.cuda.synchronize()
