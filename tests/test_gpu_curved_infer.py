"""GPU: the curved field on the device-count inference path -- nerftex_curved_field_infer (the whole no-grad chain as one call whose kernels read
the live row count from the device) and CurvedField.infer behind Renderer.render_infer_pipelined / render_infer_graphed.

Everything is compared bit for bit: the chain's kernels share their per-row arithmetic with the kernels CurvedField.forward launches, and a ray's
samples and the order they are composited in do not depend on how an inference loop cuts them into iterations.
"""
import ctypes

import numpy as np
import pytest
import torch

from infer_loop_model import unit_rows as _unit_rows  # unit_rows of csrc/common.hpp, restated once for the tests

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
B = 512  # the issue's batch; a second one where the gather takes its other kernel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _curved_field(dev):
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05).to(dev)
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
    return field.eval(), v


def _batch(dev, n):
    """n points around the mesh (its vertices pushed along their normals by up to +-0.1, two height thresholds), in ray-like order: four
    consecutive rows share a direction, as the n_step slots of one ray do.  The reference -- forward() on the batch without marks -- is computed
    once."""
    field, v = _curved_field(dev)
    rng = np.random.default_rng(5)
    ids = 36 + np.arange(n) % (v.shape[0] - 72)  # (the first and the last ring of the UV sphere are the poles, 36 times each)
    vn = field.projector.vertex_normals.cpu().numpy()
    x = (v[ids] + rng.uniform(-0.1, 0.1, size=(n, 1)).astype(np.float32) * vn[ids]).astype(np.float32)
    d = rng.normal(size=(n // 4, 3)).astype(np.float32)
    d = np.repeat(d / np.linalg.norm(d, axis=-1, keepdims=True), 4, axis=0)
    x, d = torch.from_numpy(x).to(dev), torch.from_numpy(d).to(dev).contiguous()
    marked = torch.zeros(n, dtype=torch.bool, device=dev)
    marked[::7] = True       # single slots
    marked[64:96] = True     # a whole 32-row step of an FFMLP wave
    marked[256:384] = True   # a whole 128-row workgroup
    xm, dm = x.clone(), d.clone()
    xm[marked] = 1e30        # the marks nerftex_march_rays_dev writes into the slots a ray leaves unused
    dm[marked, 0] = 1e30
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        h_mask = field.projector.project_fused(x, multires=field.multires)[2]
        sigma, rgb, _ = field(x, d)
    inside = float(h_mask.float().mean())
    assert 0.2 < inside < 0.8, inside  # both sides of the height mask are exercised
    assert sigma.dtype == torch.float16 and float((sigma > 0).float().mean()) > 0.15
    return dict(field=field, x=xm, d=dm, x_plain=x, d_plain=d, marked=marked, sigma=sigma.float(), rgb=rgb.float())


@pytest.fixture(scope="module")
def batch(dev):
    return _batch(dev, B)


@pytest.fixture(scope="module")
def batch_large(dev):
    """8192 rows: from this size on the gather runs as its level-per-XCD kernel (smaller batches: one thread per point)."""
    return _batch(dev, 8192)


def _rows_auto(n, f):
    from nerftex_hip import rows_auto

    return rows_auto(n, f)


CASES = [(None, 0, 512), (0, 5, 0), (37, 5, 185), (3, 128, 384), (5, 128, 512), (64, "auto", 256), (5, "auto", 160), (1000, "auto", 512)]


def _check_rows_contract(dev, batch, units, code, want_live):
    from nerftex_hip import check, lib, stream

    field, x, d, marked = batch["field"], batch["x"], batch["d"], batch["marked"]
    n = x.shape[0]
    live = n if units is None else min(n, units * _unit_rows(code, units))
    assert live == want_live
    units_dev = None if units is None else torch.tensor([units], dtype=torch.int32, device=dev)
    sigma = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
    rgbs = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.nerftex_curved_field_infer_scratch_bytes(n), dtype=torch.uint8, device=dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert field._infer_fused(x, d)
        desc, keep = field._infer_desc(x, d, None if units is None else (units_dev, code), sigma, rgbs, scratch)
        check(lib.nerftex_curved_field_infer(ctypes.byref(desc), stream()))
    torch.cuda.synchronize()
    rows = torch.arange(n, device=dev)
    alive, past = rows < live, rows >= live
    plain, unused = alive & ~marked, alive & marked
    n_bad = int((sigma[plain] != batch["sigma"][plain]).sum()) + int((rgbs[plain] != batch["rgb"][plain]).sum())
    print(f"B={n} units={units} code={code:#x} live={live}: {int(plain.sum())} plain rows, {n_bad} values differ from forward(); "
          f"{int(unused.sum())} marked rows, {int(past.sum())} rows past the live ones")
    assert torch.equal(sigma[plain], batch["sigma"][plain]) and torch.equal(rgbs[plain], batch["rgb"][plain])
    assert bool((sigma[unused] == 0).all()) and bool((rgbs[unused] == 0).all())
    assert bool((sigma[past] == SENTINEL).all()) and bool((rgbs[past] == SENTINEL).all())
    if live:
        assert float(sigma[plain].max()) > 0 and float(rgbs[plain].max()) > 0  # (not a comparison of zeros)


@pytest.mark.parametrize("units,code,want_live", CASES)
def test_rows_contract_at_the_c_abi(dev, batch, units, code, want_live):
    """nerftex_curved_field_infer with outputs pre-filled by a sentinel: unmarked live rows are forward()'s values cast with .float(), bit for bit;
    marked live rows are exactly 0; rows >= live = min(B, units * unit_rows(code, units)) keep the sentinel."""
    _check_rows_contract(dev, batch, units, _rows_auto(64, 4) if code == "auto" else code, want_live)


# 5000 = 39 x 128 + 8: a partial wave inside a partial workgroup; NERFTEX_ROWS_AUTO(2048, 4) with 300 units: n_step = 27, 8100 rows
@pytest.mark.parametrize("units,code,want_live", [(None, 0, 8192), (1000, 5, 5000), (300, "auto", 8100)])
def test_rows_contract_where_the_gather_runs_by_level(dev, batch_large, units, code, want_live):
    """The same contract at the batch size from which the chain's gather is the level-per-XCD kernel (what a frame's iterations run)."""
    _check_rows_contract(dev, batch_large, units, _rows_auto(2048, 4) if code == "auto" else code, want_live)


@pytest.fixture(scope="module")
def frame_setup(dev):
    """The field behind a Renderer with its occupancy grid, two 50 x 50 frames (a range of 1250 rays is a multiple of neither 64 nor 128) and
    their reference images: render_infer, the reference loop as written."""
    from ngp_harness import scene
    from ngp_harness.model import Renderer

    field, _ = _curved_field(dev)
    r = Renderer(field, bound=1.0, min_near=0.05, density_thresh=0.01).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        r.update_extra_state_device()
    rng = np.random.default_rng(11)
    frames, refs = [], []
    for pose in scene.rand_poses(2, 1.6, rng):
        o, d = scene.get_rays(pose, scene.intrinsics(50, 50), 50, 50)
        frames.append((torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)))
    with torch.autocast("cuda", dtype=torch.float16):
        for ro, rd in frames:
            refs.append(r.render_infer(ro, rd, dt_gamma=0.0, max_steps=256, slots_per_ray=4)[:2])
        ro, rd = frames[0]
        # weights_sum of the reference loop: image(bg = 1) - image(bg = 0) = 1 - weights_sum
        ws = 1 - (refs[0][0] - r.render_infer(ro, rd, dt_gamma=0.0, bg_color=0, max_steps=256, slots_per_ray=4)[0])[:, 0]
    opaque = float((ws > 0.5).float().mean())
    assert opaque >= 0.1 and 1 - opaque >= 0.1, opaque  # rays that terminate early and rays that run on, in the same ranges
    return dict(field=field, r=r, frames=frames, refs=refs)


# one marching schedule for the three loops: the step length of dt_gamma = 0 is a function of max_steps
KW = dict(dt_gamma=0.0, max_steps=256)


def test_the_frame_is_the_reference_loops_frame(dev, frame_setup):
    """render_infer_graphed, render_infer_pipelined and render_infer give the same image and depth (torch.equal); a second pose replays the
    recorded graphs; a changed table re-records them."""
    field, r, frames, refs = (frame_setup[k] for k in ("field", "r", "frames", "refs"))
    (ro, rd), (img_ref, dep_ref) = frames[0], refs[0]
    saved = field.encoder.embeddings.detach().clone()
    try:
        with torch.autocast("cuda", dtype=torch.float16):
            img_g, dep_g, _ = r.render_infer_graphed(ro, rd, slots_per_ray=4, parts=2, block=2, **KW)
            iters = r.last_iters
            img_p, dep_p, _ = r.render_infer_pipelined(ro, rd, slots_per_ray=4, parts=2, **KW)
            print(f"graphed frame: {iters} iterations; values that differ from render_infer: graphed {int((img_g != img_ref).sum())} image / "
                  f"{int((dep_g != dep_ref).sum())} depth, pipelined {int((img_p != img_ref).sum())} image / {int((dep_p != dep_ref).sum())} depth")
            assert iters > 2, iters  # more than one block: compaction and a smaller block graph ran
            assert torch.equal(img_p, img_ref) and torch.equal(dep_p, dep_ref)
            assert torch.equal(img_g, img_ref) and torch.equal(dep_g, dep_ref)
            assert float(img_ref.std()) > 1e-3
            graphs = r._infer_graphs
            img_2, dep_2, _ = r.render_infer_graphed(*frames[1], slots_per_ray=4, parts=2, block=2, **KW)
            assert r._infer_graphs is graphs, "another pose replays the recorded graphs"
            assert torch.equal(img_2, refs[1][0]) and torch.equal(dep_2, refs[1][1])
            with torch.no_grad():
                field.encoder.embeddings.mul_(1.01)  # in place, version counter bumped (as an optimizer step does): a new 16-bit table
            img_new, dep_new, _ = r.render_infer_graphed(ro, rd, slots_per_ray=4, parts=2, block=2, **KW)
            assert r._infer_graphs is not graphs, "a changed table re-records the graphs"
            img_want, dep_want, _ = r.render_infer(ro, rd, slots_per_ray=4, **KW)
            assert torch.equal(img_new, img_want) and torch.equal(dep_new, dep_want)
            assert not torch.equal(img_want, img_ref)
    finally:
        with torch.no_grad():
            field.encoder.embeddings.copy_(saved)


def test_fallback_serves_all_rows_through_forward(dev, batch, frame_setup):
    """fused_glue = False: infer() is forward() on every row, whatever `live` says, cast to fp32 -- and the pipelined frame is still the reference's."""
    field, r, frames = (frame_setup[k] for k in ("field", "r", "frames"))
    x, d = batch["x_plain"], batch["d_plain"]
    none_live = (torch.zeros(1, dtype=torch.int32, device=dev), 5)
    field.fused_glue = False
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            assert not field._infer_fused(x, d)
            sigma, rgbs = field.infer(x, d, none_live)
            want_s, want_c, _ = field(x, d)
            assert sigma.dtype == torch.float32 and rgbs.dtype == torch.float32
            assert torch.equal(sigma, want_s.float()) and torch.equal(rgbs, want_c.float()) and float(sigma.max()) > 0
            # (the reference loop under the same switch: the framework-op chain keeps sigma in fp32 where the glue kernels round it to half)
            img_want, dep_want, _ = r.render_infer(*frames[0], slots_per_ray=4, **KW)
            img_p, dep_p, _ = r.render_infer_pipelined(*frames[0], slots_per_ray=4, parts=2, **KW)
        assert torch.equal(img_p, img_want) and torch.equal(dep_p, dep_want) and float(img_want.std()) > 1e-3
    finally:
        field.fused_glue = True


def test_other_network_widths_go_through_forward(dev, batch):
    """A curved field the entry's kernels are not built for (a 64-wide sigma net: in_dim is still 41, the glue kernels still apply) is served by
    forward() on all rows -- infer() must not hand it to the library, which refuses it."""
    from ngp_harness.curved import CurvedField, star_flower_mesh

    v, f = star_flower_mesh(n_lat=18, n_lon=36)
    torch.manual_seed(0)
    field = CurvedField(v, f, bound=1.0, h_threshold=0.05, hidden_dim=64).to(dev).eval()
    with torch.no_grad():
        field.encoder.embeddings.uniform_(-0.5, 0.5)
        field.sigma_net.weights.mul_(3.0)
    x, d = batch["x_plain"], batch["d_plain"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        assert field._glue_fused() and not field._infer_fused(x, d)
        sigma, rgbs = field.infer(x, d, (torch.zeros(1, dtype=torch.int32, device=dev), 5))
        want_s, want_c, _ = field(x, d)
    assert sigma.dtype == torch.float32 and rgbs.dtype == torch.float32
    assert torch.equal(sigma, want_s.float()) and torch.equal(rgbs, want_c.float()) and float(sigma.max()) > 0


def test_eager_scratch_is_one_buffer_per_stream(dev, batch_large):
    """The inference loop's batch size changes with nearly every iteration: infer() keeps ONE scratch buffer per stream, grown to the largest
    batch seen, not one per size."""
    field = batch_large["field"]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for n in (8192, 512, 1024, 4096, 8192):
            sigma, rgbs = field.infer(batch_large["x"][:n].contiguous(), batch_large["d"][:n].contiguous())
            plain = ~batch_large["marked"][:n]
            assert torch.equal(sigma[plain], batch_large["sigma"][:n][plain]) and torch.equal(rgbs[plain], batch_large["rgb"][:n][plain])
    from nerftex_hip import lib

    held = field._infer_scratch
    assert len(held) == 1 and next(iter(held.values())).numel() == lib.nerftex_curved_field_infer_scratch_bytes(8192)


def test_ngp_field_graphed_frame_is_untouched(dev):
    """The stamp the curved field extends is shared: one graphed frame of an NGPField still equals the reference loop's, and its stamp carries
    nothing new (tests/test_gpu_round5.py has the full version of this test)."""
    from ngp_harness import scene
    from ngp_harness.model import NGPField, Renderer

    sc = scene.Scene(bound=2.0, seed=0)
    grid, _, _ = sc.bitfield()
    torch.manual_seed(0)
    field = NGPField(bound=2.0, mlp="ffmlp", fused_glue=True).to(dev)
    torch.manual_seed(1)
    field.encoder.embeddings.data.uniform_(-0.3, 0.3)
    field.eval()
    r = Renderer(field, bound=2.0, min_near=0.2).to(dev)
    r.set_occupancy(torch.from_numpy(grid).to(dev))
    pose = scene.rand_poses(1, 2.0, np.random.default_rng(3))[0]
    o, d = scene.get_rays(pose, scene.intrinsics(64, 48), 64, 48)
    ro, rd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    with torch.autocast("cuda", dtype=torch.float16):
        img_ref, dep_ref, _ = r.render_infer(ro, rd, dt_gamma=1 / 128)
        img_g, dep_g, _ = r.render_infer_graphed(ro, rd, dt_gamma=1 / 128, slots_per_ray=4, parts=3, block=2)
    assert torch.equal(img_g, img_ref) and torch.equal(dep_g, dep_ref) and float(img_ref.std()) > 1e-3
    assert not hasattr(field, "graph_stamp")  # (what render_infer_graphed appends to its stamp, where a field has it)
