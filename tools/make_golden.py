#!/usr/bin/env python3
"""Generate the committed golden vectors under tests/golden/ FROM THE REFERENCE ITSELF.

Runs only in the build container (needs /root/reference, which never travels to the GPU box).
What can be executed / evaluated there without nvcc:

  sh_golden.npz       the 64 SH basis polynomials and their 192 partial derivatives, evaluated from
                      the reference's own expression text (shencoder/src/shencoder.cu:51-351) in
                      float64 on seeded inputs.  The .cu is read at run time and its right-hand
                      sides are evaluated with numpy; no reference text is stored in this repo.
  grid_offsets.json   GridEncoder.__init__ level tables (gridencoder/grid.py:93-131), obtained by
                      importing the reference class with a stubbed `_gridencoder` backend.
  ffmlp_params.json   FFMLP.__init__ parameter counts (ffmlp/ffmlp.py:99-144), same mechanism.

  api_signatures.json, ref_python_*.npz, ref_host_pieces.npz
                      the reference's OWN Python (raymarching/raymarching.py, gridencoder/grid.py, grid_clustering.py,
                      shencoder/sphere_harmonics.py, ffmlp/ffmlp.py, nerf/renderer.py, nerf/network_ff.py, tools/activation.py,
                      tools/encoding.py) imported and RUN on the CPU: the four native modules it binds are replaced by the
                      oracle's C restatement (oracle/backends.py), `.cuda()` by the identity, and custom_fwd's input casts are
                      applied to CPU tensors too (they only touch CUDA tensors otherwise), so the wrappers' allocation rules,
                      autograd plumbing, renderer control flow (run / run_cuda train + inference / update_extra_state /
                      mark_untrained_grid) and the network's op sequence are the reference's, executed -- see
                      reference_python_goldens().

Import discipline (SURVEY.md incident): the reference wrappers fall back to a JIT build that
hipifies sources INTO /root/reference unless the `_X` backend modules are pre-seeded, so every
`_gridencoder/_raymarching/_shencoder/_ffmlp` (+ `turtle`) is stubbed and bytecode writing is off.
"""
import json
import os
import re
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np

REF = os.environ.get("NERFTEX_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


_installed = False


def install_reference_imports():
    """Put /root/reference on the path with its native modules backed by the oracle and its absent third-party imports stubbed."""
    global _installed
    if _installed:
        return
    _installed = True
    import torch

    repo = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    sys.path.insert(0, repo)  # for `oracle` only: the drop-in packages under nerf-texture_amd/ must NOT be importable here
    assert not any(p.rstrip("/").endswith("nerf-texture_amd") for p in sys.path)
    from oracle import backends

    sys.modules["_raymarching"] = backends.Raymarching
    sys.modules["_gridencoder"] = backends.GridEncoder
    sys.modules["_shencoder"] = backends.SHEncoder
    sys.modules["_ffmlp"] = backends.FFMLP
    _stub("turtle", backward=None, forward=None, bgcolor=None)
    _stub("trimesh")
    _stub("nerf.utils", custom_meshgrid=lambda *a: torch.meshgrid(*a, indexing="ij"))  # nerf/utils.py:107-112 (its other imports are absent here)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "external", "RayTracer"))
    # no GPU here: `.cuda()` is the identity, and custom_fwd casts CPU tensors the way it casts CUDA tensors on a GPU
    torch.Tensor.cuda = lambda self, *a, **k: self
    import torch.amp.autocast_mode as am

    def cast_any_device(value, device_type, dtype):
        if isinstance(value, torch.Tensor):
            return value.to(dtype) if value.is_floating_point() and value.dtype is not torch.float64 else value
        if isinstance(value, (str, bytes)):
            return value
        if isinstance(value, dict):
            return {cast_any_device(k, device_type, dtype): cast_any_device(v, device_type, dtype) for k, v in value.items()}
        if isinstance(value, (list, tuple)):
            out = [cast_any_device(v, device_type, dtype) for v in value]
            return type(value)(out) if isinstance(value, (list, tuple)) and type(value) in (list, tuple) else out
        return value

    am._cast = cast_any_device


class emulated_autocast:
    """`with torch.cuda.amp.autocast()` as the reference's Python sees it: is_autocast_enabled() is true (grid.py:41 then narrows the
    table), custom_fwd(cast_inputs=...) casts; framework ops on CPU tensors are not autocast -- the ones on this path (cat, sigmoid,
    slicing) behave the same either way."""

    def __enter__(self):
        import torch

        torch.set_autocast_enabled("cuda", True)
        torch.set_autocast_dtype("cuda", torch.float16)

    def __exit__(self, *exc):
        import torch

        torch.set_autocast_enabled("cuda", False)
        return False


def sh_golden():
    src = open(os.path.join(REF, "shencoder/src/shencoder.cu")).read()
    # assignments of the form  <lhs>[<idx>] = <expr> ;   with lhs in outputs/dx/dy/dz
    pat = re.compile(r"^\s*(outputs|dx|dy|dz)\[(\d+)\]\s*=\s*(.*?)\s*;", re.M)
    exprs = {"outputs": {}, "dx": {}, "dy": {}, "dz": {}}
    for lhs, idx, rhs in pat.findall(src):
        rhs = re.sub(r"(\d+\.\d*(?:[eE][-+]?\d+)?|\d+)f\b", r"\1", rhs)  # strip float suffix
        rhs = rhs.replace("pow(", "np.power(")
        exprs[lhs][int(idx)] = rhs
    for k in exprs:
        assert sorted(exprs[k]) == list(range(64)), (k, len(exprs[k]))

    rng = np.random.default_rng(20260926)
    B = 96
    pts = rng.uniform(-1.0, 1.0, size=(B, 3))
    unit = rng.normal(size=(B // 2, 3))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    pts[: B // 2] = unit  # half on the unit sphere, half raw points in the cube
    pts = pts.astype(np.float32).astype(np.float64)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    env = dict(np=np, x=x, y=y, z=z, xy=x * y, xz=x * z, yz=y * z, x2=x * x, y2=y * y, z2=z * z)
    env["xyz"] = env["xy"] * z
    for v in "xyz":
        env[v + "4"] = env[v + "2"] ** 2
        env[v + "6"] = env[v + "4"] * env[v + "2"]

    def ev(table):
        out = np.zeros((B, 64))
        for i in range(64):
            out[:, i] = eval(table[i], {"__builtins__": {}}, env) + np.zeros(B)
        return out

    np.savez_compressed(
        os.path.join(OUT, "sh_golden.npz"),
        inputs=pts.astype(np.float32),
        outputs=ev(exprs["outputs"]),
        dx=ev(exprs["dx"]),
        dy=ev(exprs["dy"]),
        dz=ev(exprs["dz"]),
    )
    print("sh_golden.npz: 64 basis + 3x64 derivative polynomials on", B, "points")


def checkpoint_roundtrip():
    """N2, both directions, with the REAL reference class: a checkpoint written like Trainer.save_checkpoint (nerf/utils.py:1485-1523)
    from a reference NeRFNetwork is loaded by the drop-in harness in a child process (tools/ckpt_roundtrip_child.py: the two sets of
    same-named packages cannot share an interpreter), every tensor compared, written back by the harness, and loaded here with
    load_state_dict(strict=True) into a fresh reference network.  The record goes into checkpoint_keys.json."""
    import subprocess
    import tempfile

    import torch

    install_reference_imports()
    from nerf.network_ff import NeRFNetwork

    torch.manual_seed(3)
    model = NeRFNetwork(bound=2, cuda_ray=True, min_near=0.2, density_thresh=10)
    with torch.no_grad():
        model.encoder.embeddings.uniform_(-1, 1)
        model.density_grid.uniform_(0, 20)
        model.density_bitfield.random_(0, 256)
        model.step_counter.random_(0, 5000)
    model.mean_count, model.mean_density = 4321, 1.25
    state = {"epoch": 7, "global_step": 1234, "stats": {"loss": [0.5], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None},
             "mean_count": model.mean_count, "mean_density": model.mean_density, "model": model.state_dict()}
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, "ref.pth"), os.path.join(tmp, "dropin.pth")
        torch.save(state, a)
        env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
        out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "ckpt_roundtrip_child.py"), a, b], env=env,
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        back = torch.load(b, weights_only=False)
        torch.manual_seed(4)
        fresh = NeRFNetwork(bound=2, cuda_ray=True, min_near=0.2, density_thresh=10)
        res = fresh.load_state_dict(back["model"], strict=True)
        same = all(torch.equal(v, state["model"][k]) for k, v in fresh.state_dict().items())
        assert same and back["epoch"] == 7 and back["global_step"] == 1234 and back["mean_count"] == 4321 and back["mean_density"] == 1.25
    return {"reference_checkpoint_loaded_by_dropin": json.loads(out.stdout.strip().splitlines()[-1])["loaded_keys"],
            "dropin_checkpoint_loaded_by_reference_strict": {"missing": list(res.missing_keys), "unexpected": list(res.unexpected_keys), "tensors_equal": same}}


def module_goldens():
    import torch

    install_reference_imports()

    from gridencoder.grid import GridEncoder  # noqa: E402

    cases = [
        dict(name="fox_bound2", kw=dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=4096)),
        # tools/encoding.py:45 get_encoder defaults align_corners=True: what network_ff.py / network.py actually build
        dict(name="fox_bound2_align", kw=dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=4096, align_corners=True)),
        dict(name="bound1_align", kw=dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048, align_corners=True)),
        dict(name="bound1", kw=dict(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048)),
        dict(name="curved_L8", kw=dict(input_dim=3, num_levels=8, level_dim=2, base_resolution=512, log2_hashmap_size=19, desired_resolution=1024, align_corners=True)),
        dict(name="normal_L4", kw=dict(input_dim=3, num_levels=4, level_dim=2, base_resolution=16, log2_hashmap_size=19, per_level_scale=2 ** (1 / 3))),
        dict(name="default", kw=dict()),
        dict(name="2d_tiled", kw=dict(input_dim=2, num_levels=8, level_dim=4, base_resolution=16, log2_hashmap_size=12, per_level_scale=2, gridtype="tiled")),
        dict(name="small_C1", kw=dict(input_dim=3, num_levels=6, level_dim=1, base_resolution=4, log2_hashmap_size=10, per_level_scale=1.5, align_corners=True)),
    ]
    out = []
    for c in cases:
        enc = GridEncoder(**c["kw"])
        out.append(
            dict(
                name=c["name"],
                kwargs=c["kw"],
                per_level_scale=float(enc.per_level_scale),
                offsets=[int(v) for v in enc.offsets.tolist()],
                rows=int(enc.embeddings.shape[0]),
                output_dim=int(enc.output_dim),
            )
        )
    json.dump(out, open(os.path.join(OUT, "grid_offsets.json"), "w"), indent=1)
    print("grid_offsets.json:", [c["name"] for c in out])

    from ffmlp.ffmlp import FFMLP  # noqa: E402

    rows = []
    for kw in [
        dict(input_dim=32, output_dim=16, hidden_dim=64, num_layers=2),
        dict(input_dim=32, output_dim=3, hidden_dim=64, num_layers=3),
        dict(input_dim=16, output_dim=1, hidden_dim=32, num_layers=2),
        dict(input_dim=64, output_dim=16, hidden_dim=64, num_layers=4),
        dict(input_dim=48, output_dim=8, hidden_dim=128, num_layers=2),
    ]:
        m = FFMLP(**kw)
        w = m.weights.detach()
        rows.append(
            dict(
                kwargs=kw,
                num_parameters=int(m.num_parameters),
                padded_output_dim=int(m.padded_output_dim),
                init_bound=float(w.abs().max()),
                first8=[float(v) for v in w[:8].tolist()],
            )
        )
    json.dump(rows, open(os.path.join(OUT, "ffmlp_params.json"), "w"), indent=1)
    print("ffmlp_params.json:", len(rows), "modules")

    # checkpoint wire format: parameter / buffer names, shapes and dtypes of the --ff network
    # (nerf/network_ff.py:11-56 = NeRFRenderer buffers + encoder + two FFMLPs).  The network class itself cannot be imported here
    # (nerf/utils.py needs a dozen absent packages), so the entries come from the component classes it is built from, instantiated
    # exactly as network_ff.py / tools/encoding.py:45 do, plus the register_buffer names read from nerf/renderer.py.
    enc = GridEncoder(input_dim=3, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19, desired_resolution=2048 * 2,
                      align_corners=True)
    sig = FFMLP(input_dim=32, output_dim=16, hidden_dim=64, num_layers=2)
    col = FFMLP(input_dim=32, output_dim=3, hidden_dim=64, num_layers=3)
    entries = {}
    for prefix, mod in (("encoder", enc), ("sigma_net", sig), ("color_net", col)):
        for k, v in mod.state_dict().items():
            entries[f"{prefix}.{k}"] = [list(v.shape), str(v.dtype).replace("torch.", "")]
    src = open(os.path.join(REF, "nerf/renderer.py")).read()
    buffers = sorted(set(re.findall(r"register_buffer\(\s*['\"](\w+)['\"]", src)))
    roundtrip = checkpoint_roundtrip()
    json.dump(dict(bound=2, cascade=2, grid_size=128, entries=entries, renderer_buffers=buffers, roundtrip=roundtrip),
              open(os.path.join(OUT, "checkpoint_keys.json"), "w"), indent=1)
    print("checkpoint_keys.json:", sorted(entries), buffers, roundtrip)

    # guard: nothing may have been written into the reference tree
    import subprocess

    new = subprocess.run(
        ["find", REF, "-newer", os.path.join(OUT, "..", "..", "BASELINE.json"), "-type", "f"], capture_output=True, text=True
    ).stdout.strip()
    assert new == "", "files appeared under the reference tree:\n" + new


# ---------------------------------------------------------------------------------------------------------------------------
# The reference's own Python, executed on the CPU over the oracle's kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _scene_bitfield(bound, cascade, H=128):
    """An analytic occupancy (a ball of radius 0.45 bound plus two blobs), Morton-ordered and packed exactly like update_extra_state does
    (nerf/renderer.py:592-599, 648-654).  Densities take the values 0 / 5 / 40 only, so no cell sits near a threshold."""
    import torch

    import raymarching

    g = torch.arange(H, dtype=torch.int32)
    xx, yy, zz = torch.meshgrid(g, g, g, indexing="ij")
    coords = torch.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], -1)
    idx = raymarching.morton3D(coords).long()
    unit = 2 * coords.float() / (H - 1) - 1
    grid = torch.zeros(cascade, H ** 3)
    for cas in range(cascade):
        b = min(2 ** cas, bound)
        x = unit * (b - b / H)
        d = torch.zeros(H ** 3)
        d[(x.norm(dim=-1) < 0.45 * bound)] = 40.0
        d[((x - torch.tensor([0.9, 0.3, -0.2]) * bound * 0.5).norm(dim=-1) < 0.12 * bound)] = 5.0
        d[((x - torch.tensor([-0.5, -0.8, 0.6]) * bound * 0.5).norm(dim=-1) < 0.10 * bound)] = 40.0
        grid[cas, idx] = d
    mean = float(grid.clamp(min=0).mean())
    return grid, raymarching.packbits(grid, min(mean, 10.0))


def _rays(n, seed, radius=2.6):
    """n rays from a few look-at-origin cameras (pixel centres of an 800 x 800, fovy 50 camera), as float32 arrays."""
    rng = np.random.default_rng(seed)
    f = 800 / (2 * np.tan(np.radians(25)))
    o, d = [], []
    for k in range(n):
        th, ph = rng.uniform(np.pi / 3, 2 * np.pi / 3), rng.uniform(0, 2 * np.pi)
        c = radius * np.array([np.sin(th) * np.sin(ph), np.cos(th), np.sin(th) * np.cos(ph)])
        fw = -c / np.linalg.norm(c)
        rt = np.cross(fw, [0, -1, 0]); rt /= np.linalg.norm(rt)
        up = np.cross(rt, fw)
        i, j = rng.uniform(200, 600, 2)
        v = np.array([(i - 400) / f, (j - 400) / f, 1.0])
        w = v[0] * rt + v[1] * up + v[2] * fw
        o.append(c); d.append(w / np.linalg.norm(w))
    return np.asarray(o, np.float32), np.asarray(d, np.float32)


def _table(model, seed):
    """The hash table as the tests rebuild it: uniform(-0.5, 0.5) from torch's CPU generator (values must be O(1) for the encoding to matter)."""
    import torch

    gen = torch.Generator().manual_seed(seed)
    model.encoder.embeddings.data.copy_(torch.rand(model.encoder.embeddings.shape, generator=gen) - 0.5)


def reference_python_goldens():
    import inspect

    import torch

    install_reference_imports()
    import ffmlp.ffmlp as ref_ffmlp
    import gridencoder.grid as ref_grid
    import gridencoder.grid_clustering as ref_gc
    import raymarching.raymarching as ref_rm
    import shencoder.sphere_harmonics as ref_sh
    from nerf.network_ff import NeRFNetwork
    from nerf.renderer import NeRFRenderer, sample_pdf
    from tools.activation import trunc_exp
    from tools.encoding import FreqEncoder

    # ---- 1. the API surface: every autograd.Function's forward, every public function / module constructor and forward
    def sig(fn):
        out = []
        for n, p in inspect.signature(fn).parameters.items():
            d = None if p.default is inspect.Parameter.empty else repr(p.default)
            out.append([n, d])
        return out

    api = {}
    for mod in (ref_rm, ref_grid, ref_gc, ref_sh, ref_ffmlp):
        name = mod.__name__
        for k, v in vars(mod).items():
            if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v.__module__ == name:
                api[f"{name}.{k}.forward"] = sig(v.forward)
            elif isinstance(v, type) and issubclass(v, torch.nn.Module) and v.__module__ == name:
                api[f"{name}.{k}.__init__"] = sig(v.__init__)
                api[f"{name}.{k}.forward"] = sig(v.forward)
    api["public"] = {m.__name__: sorted(k for k, v in vars(m).items() if not k.startswith("_") and (callable(v)) and getattr(v, "__module__", m.__name__) in (m.__name__, "torch.autograd.function"))
                     for m in (ref_rm, ref_grid, ref_gc, ref_sh, ref_ffmlp)}
    json.dump(api, open(os.path.join(OUT, "api_signatures.json"), "w"), indent=1, sort_keys=True)
    print("api_signatures.json:", len(api) - 1, "callables")

    # ---- 2. small host-side pieces: trunc_exp, FreqEncoder, sample_pdf, ClusteringLayer, GridEncoder_clustering
    torch.manual_seed(11)
    host = {}
    x = (torch.randn(64) * 8).requires_grad_(True)
    y = trunc_exp(x)
    y.backward(torch.linspace(-1, 1, 64))
    host.update(trunc_exp_x=x.detach().numpy(), trunc_exp_y=y.detach().numpy(), trunc_exp_gx=x.grad.numpy())
    fx = torch.rand(16, 1) * 0.1
    host.update(freq_x=fx.numpy(), freq_y=FreqEncoder(input_dim=1, max_freq_log2=5, N_freqs=6, log_sampling=True)(fx).numpy())  # tools/map.py:229 style
    bins = torch.sort(torch.rand(8, 33), dim=-1)[0]
    w = torch.rand(8, 32)
    host.update(pdf_bins=bins.numpy(), pdf_w=w.numpy(), pdf_out=sample_pdf(bins, w, 16, det=True).numpy())
    torch.manual_seed(12)
    layer = ref_gc.ClusteringLayer(n_clusters=6, hidden=2)
    feats = torch.rand(40, 2) * 2e-4 - 1e-4
    q = layer(feats)
    host.update(cl_centers=layer.cluster_centers.detach().numpy(), cl_x=feats.numpy(), cl_q=q.detach().numpy(),
                cl_loss=float(layer.clustering_loss(feats)))
    torch.manual_seed(13)
    enc = ref_gc.GridEncoder_clustering(input_dim=3, num_levels=3, level_dim=2, base_resolution=8, log2_hashmap_size=9, desired_resolution=32)
    pts = torch.rand(50, 3) * 2 - 1
    host.update(gc_emb=enc.embeddings.detach().numpy(), gc_offsets=enc.offsets.numpy(), gc_x=pts.numpy(), gc_y=enc(pts, bound=1).detach().numpy(),
                gc_centers=np.stack([l.cluster_centers.detach().numpy() for l in enc.cluster_layers]),
                gc_loss_all=float(enc.clustering_loss(pick_level=False)),
                gc_scale=float(enc.per_level_scale))
    np.savez_compressed(os.path.join(OUT, "ref_host_pieces.npz"), **host)
    print("ref_host_pieces.npz:", sorted(host))

    # ---- 3. the --ff network (nerf/network_ff.py) through NeRFRenderer.run_cuda: one training step and one inference render
    bound = 2
    torch.manual_seed(0)
    model = NeRFNetwork(bound=bound, cuda_ray=True, min_near=0.2, density_thresh=10)
    _table(model, 5)
    grid, bits = _scene_bitfield(bound, model.cascade)
    model.density_grid.copy_(grid)
    model.density_bitfield = bits
    ro, rd = _rays(96, 21)
    tgt = np.random.default_rng(22).uniform(0, 1, (96, 3)).astype(np.float32)
    out = {"bitfield": bits.numpy(), "rays_o": ro, "rays_d": rd, "target": tgt, "table_seed": 5, "bound": bound}
    model.train()
    with emulated_autocast():
        res = model.render(torch.from_numpy(ro)[None], torch.from_numpy(rd)[None], staged=False, bg_color=1, perturb=True, force_all_rays=False,
                           dt_gamma=1 / 128, max_steps=1024)
        loss = torch.nn.functional.mse_loss(res["image"][0], torch.from_numpy(tgt)) * 1024.0
    loss.backward()
    g = model.encoder.embeddings.grad
    nz = torch.nonzero(g.abs().sum(-1)).squeeze(-1)
    pick = nz[torch.from_numpy(np.random.default_rng(23).choice(nz.numel(), 2048, replace=False)).long()]
    off = model.encoder.offsets.long()
    out.update(train_image=res["image"][0].detach().numpy(), train_depth=res["depth"][0].detach().numpy(),
               train_counter=model.step_counter[0].numpy().copy(), train_loss=float(loss),
               g_sigma=model.sigma_net.weights.grad.numpy(), g_color=model.color_net.weights.grad.numpy(),
               g_table_rows=pick.numpy(), g_table_vals=g[pick].numpy(), g_table_nonzero_rows=int(nz.numel()),
               g_table_level_abs=np.array([float(g[off[l]:off[l + 1]].abs().double().sum()) for l in range(16)]),
               g_table_level_sum=np.array([float(g[off[l]:off[l + 1]].double().sum()) for l in range(16)]))
    model.eval()
    ro2, rd2 = _rays(256, 31)
    with torch.no_grad(), emulated_autocast():
        res = model.render(torch.from_numpy(ro2)[None], torch.from_numpy(rd2)[None], staged=False, bg_color=1, perturb=False, dt_gamma=1 / 128,
                           max_steps=1024)
    out.update(infer_rays_o=ro2, infer_rays_d=rd2, infer_image=res["image"][0].numpy(), infer_depth=res["depth"][0].numpy())
    # march_rays_train_differentiable (raymarching.py:238-287): forward + its Python backward, on the first 24 training rays
    o24 = torch.from_numpy(ro[:24]).requires_grad_(True)
    d24 = torch.from_numpy(rd[:24]).requires_grad_(True)
    n24, f24 = ref_rm.near_far_from_aabb(o24.detach(), d24.detach(), model.aabb_train, 0.2)
    cnt = torch.zeros(2, dtype=torch.int32)
    xyzs, dirs, deltas, rays24 = ref_rm.march_rays_train_differentiable(o24, d24, bound, bits, model.cascade, 128, n24, f24, cnt, -1, False, 128, False, 1 / 128, 64)
    gx = torch.from_numpy(np.random.default_rng(24).standard_normal(tuple(xyzs.shape)).astype(np.float32))
    xyzs.backward(gx)
    out.update(diff_max_steps=64, diff_grad_xyzs=gx.numpy(), diff_counter=cnt.numpy().copy(), diff_rays=rays24.numpy(), diff_xyzs=xyzs.detach().numpy(),
               diff_grad_o=o24.grad.numpy(), diff_grad_d=d24.grad.numpy())
    np.savez_compressed(os.path.join(OUT, "ref_python_run_cuda.npz"), **out)
    print("ref_python_run_cuda.npz: train", int(out["train_counter"][0]), "samples /", int(out["train_counter"][1]), "rays; loss", out["train_loss"])

    # ---- 4. the same network through NeRFRenderer.run (cuda_ray=False: uniform samples, sample_pdf upsampling, cumprod compositing)
    torch.manual_seed(0)
    m2 = NeRFNetwork(bound=bound, cuda_ray=False, min_near=0.2, density_thresh=10)
    _table(m2, 5)
    m2.eval()
    ro3, rd3 = _rays(48, 41)
    with torch.no_grad(), emulated_autocast():
        r0 = m2.render(torch.from_numpy(ro3)[None], torch.from_numpy(rd3)[None], staged=False, bg_color=1, perturb=False, num_steps=64, upsample_steps=32)
        r1 = m2.render(torch.from_numpy(ro3)[None], torch.from_numpy(rd3)[None], staged=False, bg_color=1, perturb=False, num_steps=96, upsample_steps=0)
    np.savez_compressed(os.path.join(OUT, "ref_python_run.npz"), rays_o=ro3, rays_d=rd3, table_seed=5, bound=bound,
                        image_64_32=r0["image"][0].numpy(), depth_64_32=r0["depth"][0].numpy(), image_96_0=r1["image"][0].numpy(),
                        depth_96_0=r1["depth"][0].numpy())
    print("ref_python_run.npz: 48 rays, (64+32) and (96+0) samples")

    # ---- 5. occupancy maintenance on an analytic density: mark_untrained_grid, two full updates, two partial updates
    class Analytic(NeRFRenderer):
        def density(self, x):
            s = torch.zeros(x.shape[0])
            s[x.norm(dim=-1) < 0.9] = 40.0
            s[(x - torch.tensor([1.1, 0.4, -0.3])).norm(dim=-1) < 0.35] = 5.0
            s[(x - torch.tensor([-0.7, -1.2, 0.8])).norm(dim=-1) < 0.3] = 40.0
            return {"sigma": s}

    r = Analytic(bound=bound, cuda_ray=True, min_near=0.2, density_thresh=10)
    po, pd = _rays(6, 51, radius=3.0)
    poses = np.tile(np.eye(4, dtype=np.float32), (6, 1, 1))
    for k in range(6):  # c2w with the camera looking along +z at the origin (mark_untrained_grid keeps points with z_cam > 0)
        fw = -po[k] / np.linalg.norm(po[k])
        rt = np.cross(fw, [0, -1, 0]); rt /= np.linalg.norm(rt)
        poses[k, :3, 0], poses[k, :3, 1], poses[k, :3, 2], poses[k, :3, 3] = rt, np.cross(fw, rt), fw, po[k]
    intr = np.array([900.0, 900.0, 150.0, 150.0], np.float32)  # fx fy cx cy: narrow cameras (+-9.5 degrees), so that part of the volume stays unseen
    torch.manual_seed(7)
    r.mark_untrained_grid(poses, intr)
    states = {"poses": poses, "intrinsic": intr, "untrained": np.packbits((r.density_grid < 0).numpy().reshape(-1), bitorder="little")}
    probe = np.random.default_rng(52).choice(r.density_grid.numel(), 8192, replace=False)
    states["probe"] = probe
    for step in range(4):
        if step == 2:
            r.iter_density = 16  # from here on update_extra_state takes its partial-update branch
        r.local_step, r.step_counter[:5, 0] = 5, torch.tensor([700, 720, 690, 710, 705], dtype=torch.int32)
        r.update_extra_state()
        states[f"grid_probe_{step}"] = r.density_grid.reshape(-1).numpy()[probe].copy()
        states[f"grid_sum_{step}"] = float(r.density_grid.double().sum())
        states[f"bitfield_{step}"] = r.density_bitfield.numpy().copy()
        states[f"mean_density_{step}"] = r.mean_density
        states[f"mean_count_{step}"] = r.mean_count
    np.savez_compressed(os.path.join(OUT, "ref_python_extra_state.npz"), **states)
    print("ref_python_extra_state.npz: mean densities", [round(states[f"mean_density_{k}"], 5) for k in range(4)], "mean_count", states["mean_count_3"])


def main():
    os.makedirs(OUT, exist_ok=True)
    if "--import-field-only" in sys.argv:
        import_field_goldens()
        return
    if "--import-field-sh-only" in sys.argv:
        import_field_sh_goldens()
        return
    if "--import-shape-only" in sys.argv:
        import_shape_goldens()
        return
    if "--import-shape-sh-only" in sys.argv:
        import_shape_sh_goldens()
        return
    if "--import-patch-only" in sys.argv:
        import_patch_goldens()
        return
    if "--import-patch-sh-only" in sys.argv:
        import_patch_sh_goldens()
        return
    if "--synthesis-only" in sys.argv:
        synthesis_goldens()
        return
    if "--unhash-only" in sys.argv:
        unhash_goldens()
        return
    if "--sh-light-only" in sys.argv:
        sh_light_goldens()
        sh_field_goldens()
        return
    if "--round5-only" in sys.argv:
        round5_goldens()
        return
    if "--round3-only" not in sys.argv and "--round4-only" not in sys.argv:
        sh_golden()
        module_goldens()
        reference_python_goldens()
    if "--round4-only" not in sys.argv:
        round3_goldens()
    round4_goldens()
    round5_goldens()


# ---------------------------------------------------------------------------------------------------------------------------
# Round 3: the nn.Linear field (configs[1]), the curved-field projector and the curved field, all run from the reference's Python
# ---------------------------------------------------------------------------------------------------------------------------
def _small_star_flower(n_lat=24, n_lon=48, lobes=5, amp=0.18, radius=0.7):
    """A small star_flower-shaped closed mesh (UV sphere with a 5-lobe radial modulation), float32 vertices + uint32 faces, its
    area-weighted vertex normals (the role of open3d's compute_vertex_normals, tools/map.py:366,396) and a per-face frame."""
    theta = np.linspace(0, np.pi, n_lat + 1)
    phi = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    T, P = np.meshgrid(theta, phi, indexing="ij")
    r = radius * (1 + amp * np.sin(T) ** 2 * np.cos(lobes * P))
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.cos(T), r * np.sin(T) * np.sin(P)], -1).reshape(-1, 3).astype(np.float32)
    faces = []
    for i in range(n_lat):
        for j in range(n_lon):
            a, b = i * n_lon + j, i * n_lon + (j + 1) % n_lon
            c, d = (i + 1) * n_lon + j, (i + 1) * n_lon + (j + 1) % n_lon
            if i > 0:
                faces.append((a, c, b))
            if i < n_lat - 1:
                faces.append((b, c, d))
    f = np.asarray(faces, np.uint32)
    fi = f.astype(np.int64)
    e1, e2 = v[fi[:, 1]] - v[fi[:, 0]], v[fi[:, 2]] - v[fi[:, 0]]
    fn = np.cross(e1, e2)
    vn = np.zeros_like(v)
    for k in range(3):
        np.add.at(vn, fi[:, k], fn)
    vn /= np.linalg.norm(vn, axis=-1, keepdims=True) + 1e-12
    t = e1 / (np.linalg.norm(e1, axis=-1, keepdims=True) + 1e-12)
    n = fn / (np.linalg.norm(fn, axis=-1, keepdims=True) + 1e-12)
    tbn = np.stack([t, np.cross(n, t), n], axis=1).astype(np.float32)
    return v, f, vn.astype(np.float32), tbn


def _install_map_imports():
    """tools/map.py and nerf/network_curvedfield.py import a dozen packages this image lacks.  Stubs for the ones whose code is never
    reached here; WORKING stand-ins, declared as such, for the three that are:
      frnn.frnn_grid_points   (un-vendored, tools/map.py:396,456)  -> exact brute-force K nearest (squared distances, ascending)
      _raytracing             (external/RayTracer/src: CUDA)       -> the oracle's brute-force closest hit behind the reference's own
                                                                      RayTracer wrapper (external/RayTracer/RayTracer/raytracer.py)
      tinycudann              (un-vendored, unpinned)              -> Network = the reference's in-tree transplant of the same kernel
                                                                      (ffmlp/ffmlp.py, over the oracle) with tcnn's input padding
                                                                      (to a multiple of 16, padded with ONES); Encoding = the
                                                                      reference's SHEncoder on 2x-1 (tcnn's SH takes [0,1] inputs)."""
    import torch

    install_reference_imports()
    from oracle import oracle as orc

    def frnn_grid_points(p1, p2, l1, l2, K, r, grid=None, return_nn=False, return_sorted=True):
        d2 = torch.cdist(p1[0].double(), p2[0].double()) ** 2
        dd, ii = torch.topk(d2, K, dim=-1, largest=False, sorted=True)
        return dd.float()[None], ii[None], None, grid

    _stub("frnn", frnn_grid_points=frnn_grid_points)

    class _Impl:
        def __init__(self, v, f):
            self.v, self.f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.uint32)

        def trace(self, rays_o, rays_d, positions, face_normals, depth, face_idx):
            pos, nrm, dep, face, _ = orc.raytrace(self.v, self.f, rays_o.detach().numpy(), rays_d.detach().numpy())  # (the native op reads the storage whatever requires_grad says)
            positions.copy_(torch.from_numpy(pos)); face_normals.copy_(torch.from_numpy(nrm))
            depth.copy_(torch.from_numpy(dep)); face_idx.copy_(torch.from_numpy(face))

    _stub("_raytracing", create_raytracer=lambda v, f: _Impl(v, f))
    for name in ("xatlas", "pytorch3d", "pytorch3d._C", "pytorch3d.io", "pytorch3d.structures", "open3d", "pymesh", "mcubes", "plyfile", "cv2"):
        _stub(name)
    sys.modules["pytorch3d"]._C = sys.modules["pytorch3d._C"]
    sys.modules["pytorch3d.io"].load_obj = None
    sys.modules["pytorch3d.structures"].Meshes = sys.modules["pytorch3d.structures"].Pointclouds = None
    sys.modules["plyfile"].PlyElement = sys.modules["plyfile"].PlyData = None
    sys.modules["pytorch3d"].io = sys.modules["pytorch3d.io"]

    from ffmlp.ffmlp import FFMLP
    from shencoder import SHEncoder

    class Network(torch.nn.Module):
        def __init__(self, n_input_dims, n_output_dims, network_config):
            super().__init__()
            # (case-insensitive: nerf/sh_light_model.py:538 spells it "Relu")
            assert network_config["otype"] == "FullyFusedMLP" and network_config["activation"].lower() == "relu" and network_config["output_activation"] == "None"
            self.n_in, self.n_out = n_input_dims, n_output_dims
            self.pad_in = (n_input_dims + 15) // 16 * 16
            self.net = FFMLP(input_dim=self.pad_in, output_dim=n_output_dims, hidden_dim=network_config["n_neurons"],
                             num_layers=network_config["n_hidden_layers"] + 1)

        def forward(self, x):
            ones = torch.ones(x.shape[0], self.pad_in - self.n_in, dtype=x.dtype)
            return self.net(torch.cat([x, ones], dim=-1))

    class Encoding(torch.nn.Module):
        def __init__(self, n_input_dims, encoding_config):
            super().__init__()
            assert encoding_config["otype"] == "SphericalHarmonics"
            self.enc = SHEncoder(input_dim=n_input_dims, degree=encoding_config["degree"])
            self.n_output_dims = self.enc.output_dim

        def forward(self, x):
            return self.enc(x * 2 - 1)

    _stub("tinycudann", Network=Network, Encoding=Encoding)
    sys.modules.pop("nerf.utils", None)
    _stub("nerf.utils", custom_meshgrid=lambda *a: torch.meshgrid(*a, indexing="ij"))


def round3_goldens():
    import torch

    install_reference_imports()
    # ---- 6. configs[1]: nerf/network.py (nn.Linear MLPs) through run_cuda, one training render + backward.  The grid encoder returns
    # half under autocast and nn.Linear is an autocast op: CPU autocast (fp16) stands in for the GPU's
    from nerf.network import NeRFNetwork as RefLinearNetwork

    class LinearNetwork(RefLinearNetwork):
        """nerf/network.py:96-124 as written returns (sigma, color) and takes no keywords, while this repository's renderer calls
        `self(xyzs, dirs, frame_index=...)` and unpacks three values (nerf/renderer.py:376): the torch-ngp network was left behind when
        the renderer grew its third return value.  The adapter only bridges that call; the field arithmetic is the reference's."""

        def forward(self, x, d, **kwargs):
            sigma, color = RefLinearNetwork.forward(self, x, d)
            return sigma, color, {}

    bound = 2
    torch.manual_seed(0)
    model = LinearNetwork(bound=bound, cuda_ray=True, min_near=0.2, density_thresh=10)
    _table(model, 5)
    grid, bits = _scene_bitfield(bound, model.cascade)
    model.density_grid.copy_(grid)
    model.density_bitfield = bits
    ro, rd = _rays(96, 21)
    tgt = np.random.default_rng(22).uniform(0, 1, (96, 3)).astype(np.float32)
    out = {"bitfield": bits.numpy(), "rays_o": ro, "rays_d": rd, "target": tgt, "table_seed": 5, "bound": bound}
    for i, l in enumerate(model.sigma_net):
        out[f"w_sigma_{i}"] = l.weight.detach().numpy().copy()
    for i, l in enumerate(model.color_net):
        out[f"w_color_{i}"] = l.weight.detach().numpy().copy()
    model.train()
    with emulated_autocast(), torch.autocast("cpu", dtype=torch.float16):
        res = model.render(torch.from_numpy(ro)[None], torch.from_numpy(rd)[None], staged=False, bg_color=1, perturb=True, force_all_rays=False,
                           dt_gamma=1 / 128, max_steps=1024)
        loss = torch.nn.functional.mse_loss(res["image"][0].float(), torch.from_numpy(tgt)) * 1024.0
    loss.backward()
    g = model.encoder.embeddings.grad
    nz = torch.nonzero(g.abs().sum(-1)).squeeze(-1)
    pick = nz[torch.from_numpy(np.random.default_rng(23).choice(nz.numel(), 2048, replace=False)).long()]
    off = model.encoder.offsets.long()
    out.update(train_image=res["image"][0].detach().float().numpy(), train_depth=res["depth"][0].detach().float().numpy(),
               train_counter=model.step_counter[0].numpy().copy(), train_loss=float(loss),
               g_table_rows=pick.numpy(), g_table_vals=g[pick].numpy(), g_table_nonzero_rows=int(nz.numel()),
               g_table_level_abs=np.array([float(g[off[l]:off[l + 1]].abs().double().sum()) for l in range(16)]))
    for i, l in enumerate(model.sigma_net):
        out[f"g_sigma_{i}"] = l.weight.grad.numpy().copy()
    for i, l in enumerate(model.color_net):
        out[f"g_color_{i}"] = l.weight.grad.numpy().copy()
    np.savez_compressed(os.path.join(OUT, "ref_python_run_cuda_linear.npz"), **out)
    print("ref_python_run_cuda_linear.npz: train", int(out["train_counter"][0]), "samples /", int(out["train_counter"][1]), "rays; loss", out["train_loss"])

    # ---- 7. MeshProjector.knn / .project (tools/map.py:414-433, 452-502) executed: frnn -> exact brute force, tracer -> oracle B2
    _install_map_imports()
    import tools.map as ref_map
    from RayTracer import RayTracer as RefRayTracer

    v, f, vn, tbn = _small_star_flower()
    mp = object.__new__(ref_map.MeshProjector)  # past the trimesh / xatlas / open3d constructor: only what knn() and project() read
    mp.mesh_vertices, mp.vertex_normals, mp.tbn = torch.from_numpy(v), torch.from_numpy(vn), torch.from_numpy(tbn)
    mp.grid, mp.radius, mp.max_K, mp.depth_threshold = None, 100.0, v.shape[0], 9.5
    mp.raytracer = RefRayTracer(v, f)
    rng = np.random.default_rng(61)
    base = v[rng.integers(0, v.shape[0], 768)]
    pts = (base * (1 + rng.uniform(-0.12, 0.12, (768, 1))) + rng.normal(0, 0.01, (768, 3))).astype(np.float32)
    x = torch.from_numpy(pts)
    normal, dir_vec_ori, idx, dis = mp.knn(xyz=x, K=8, use_dir_vec=True)
    p_sur, sdf, h_mask, normal2, tbn_out = mp.project(x, K=8, h_threshold=0.05)
    assert torch.equal(normal, normal2)
    _, _, d1, f1 = mp.raytracer.trace(x, normal)
    _, _, d2, f2 = mp.raytracer.trace(x, -normal)
    proj = dict(vertices=v, faces=f, vertex_normals=vn, tbn=tbn, xyz=pts, knn_idx=idx.numpy().astype(np.int32), knn_dis=dis[:, :8].numpy(), normal=normal.numpy(),
                p_sur=p_sur.numpy(), sdf=sdf.numpy(), h_mask=h_mask.numpy(), tbn_out=tbn_out.numpy(), depth_pos=d1.numpy(), depth_neg=d2.numpy(),
                face_pos=f1.numpy(), face_neg=f2.numpy(), h_threshold=0.05)
    np.savez_compressed(os.path.join(OUT, "ref_python_projector.npz"), **proj)
    print("ref_python_projector.npz:", pts.shape[0], "points,", int(h_mask.sum()), "inside the height threshold,", int((d1 < d2).sum()), "inner")

    # ---- 8. the curved field: MeshFeatureField.forward (tools/map.py:620-641, 717-737; hash=True, clustering, no prob model, no normal net)
    # and network_curvedfield.NeRFNetwork.forward / density (nerf/network_curvedfield.py:229-243, 283-300, 382-409) with the light model off
    for name, cls in (("sg_light_model", "SG_EnvmapMaterialNet"), ("sh_light_model", "SH_EnvmapMaterialNet"), ("envmap_light_model", "Envmap_EnvmapMaterialNet")):
        _stub("nerf." + name, **{cls: None})  # this fixture runs with light_model=None, which never builds one (the SH model: sh_light_goldens)
    import nerf.network_curvedfield as ref_cf
    from tools.encoding import get_encoder

    torch.manual_seed(0)
    mff = object.__new__(ref_map.MeshFeatureField)
    torch.nn.Module.__init__(mff)
    mff.h_threshold, mff.K, mff.bound, mff.hash, mff.prob_model, mff.pred_normal, mff.clustering = 0.05, 8, 1, True, False, False, True
    mff.imported, mff.imported_type, mff.normal_net = False, None, None
    mff.encoder, mff.encoder_f_out_dim = get_encoder("hashgrid_clustering", desired_resolution=1024, input_dim=3, num_levels=8, level_dim=2, base_resolution=512,
                                                     log2_hashmap_size=19, align_corners=True)
    mff.encoder_z, mff.encoder_z_outdim = get_encoder("frequency", input_dim=1, multires=12)
    mff.meshprojector = mp
    gen = torch.Generator().manual_seed(9)
    mff.encoder.embeddings.data.copy_(torch.rand(mff.encoder.embeddings.shape, generator=gen) - 0.5)
    net = object.__new__(ref_cf.NeRFNetwork)
    torch.nn.Module.__init__(net)
    net.visual_mode, net.render_light_model, net.use_grad_normal, net.fc_weight, net.dir_degree = "RGB", False, False, 1.0, 4
    net.optimize_gamma, net.meshfea_field = False, mff
    tcnn = sys.modules["tinycudann"]
    torch.manual_seed(42)
    net.sigma_net = tcnn.Network(n_input_dims=mff.encoder_z_outdim + mff.encoder_f_out_dim, n_output_dims=16,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 1})
    net.encoder_dir = tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "SphericalHarmonics", "degree": 4})
    net.color_net = tcnn.Network(n_input_dims=net.encoder_dir.n_output_dims + 15, n_output_dims=3,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2})
    dirs = rng.normal(size=(768, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)
    cf = dict(xyz=pts, dirs=dirs, table_seed=9, w_sigma=net.sigma_net.net.weights.detach().numpy().copy(), w_color=net.color_net.net.weights.detach().numpy().copy(),
              table_rows=int(mff.encoder.embeddings.shape[0]), offsets=mff.encoder.offsets.numpy().copy(), per_level_scale=float(mff.encoder.per_level_scale))
    for mode in ("eval", "train"):
        net.train(mode == "train")
        with emulated_autocast():
            if mode == "eval":
                with torch.no_grad():
                    embed, nc, nf, hm = mff(x)
                    sigma, color, _ = net(x, torch.from_numpy(dirs))
                    dens = net.density(x)
                cf.update(embed=embed.float().numpy(), normal_coarse=nc.numpy(), h_mask=hm.numpy(), sigma=sigma.float().numpy(), color=color.float().numpy(),
                          density_sigma=dens["sigma"].float().numpy(), density_geo=dens["geo_feat"].float().numpy())
            else:
                sigma, color, _ = net(x, torch.from_numpy(dirs))
                gs = torch.from_numpy(rng.normal(size=sigma.shape).astype(np.float32)) * 1e-2
                gc = torch.from_numpy(rng.normal(size=color.shape).astype(np.float32))
                ((sigma.float() * gs).sum() + (color.float() * gc).sum()).backward()
                gt = mff.encoder.embeddings.grad
                nz = torch.nonzero(gt.abs().sum(-1)).squeeze(-1)
                cf.update(train_sigma=sigma.detach().float().numpy(), train_color=color.detach().float().numpy(), grad_sigma=gs.numpy(), grad_color=gc.numpy(),
                          g_w_sigma=net.sigma_net.net.weights.grad.numpy().copy(), g_w_color=net.color_net.net.weights.grad.numpy().copy(),
                          g_table_rows=nz[:4096].numpy(), g_table_vals=gt[nz[:4096]].numpy(), g_table_abs=float(gt.abs().double().sum()))
    np.savez_compressed(os.path.join(OUT, "ref_python_curvedfield.npz"), **cf)
    print("ref_python_curvedfield.npz: sigma range", float(cf["sigma"].min()), float(cf["sigma"].max()), "masked", int((~cf["h_mask"]).sum()))

    import subprocess

    new = subprocess.run(["find", REF, "-newer", os.path.join(OUT, "..", "..", "BASELINE.json"), "-type", "f"], capture_output=True, text=True).stdout.strip()
    assert new == "", "files appeared under the reference tree:\n" + new


# ---------------------------------------------------------------------------------------------------------------------------
# Round 4: the whole chain in fp32, NO autocast -- the configuration north_star's "within 1e-4 rel on rendered RGB / sigma" is about
# ---------------------------------------------------------------------------------------------------------------------------
def round4_goldens():
    """nerf/network.py:96-124 (nn.Linear MLPs, fp32) through nerf/renderer.py:338-425 (training branch of run_cuda, with backward) and
    :436-487 (its inference loop), executed WITHOUT autocast: fp32 table, fp32 SH, fp32 MLPs, fp32 compositing.  512 rays each.  Besides the
    images the fixture keeps the per-sample sigma / rgb the network returned for the training render (first 8192 samples), the ray records,
    and fp32 gradients (weights, 2048 sampled table rows, per-level L1)."""
    import torch

    install_reference_imports()
    from nerf.network import NeRFNetwork as RefLinearNetwork

    class LinearNetwork(RefLinearNetwork):
        """The same call bridge as in round3_goldens (the renderer passes keywords and unpacks three values); it also keeps what the
        network returned, so that sigma / rgb can be pinned per sample."""

        def forward(self, x, d, **kwargs):
            sigma, color = RefLinearNetwork.forward(self, x, d)
            self.last_xyz, self.last_sigma, self.last_color = x.detach(), sigma.detach(), color.detach()
            return sigma, color, {}

    bound = 2
    torch.manual_seed(0)
    model = LinearNetwork(bound=bound, cuda_ray=True, min_near=0.2, density_thresh=10)
    _table(model, 5)
    grid, bits = _scene_bitfield(bound, model.cascade)
    model.density_grid.copy_(grid)
    model.density_bitfield = bits
    with torch.no_grad():  # nn.Linear's default init leaves sigma = exp(h0) within 0.9 .. 1.15: widen the sigma row so that densities span decades
        model.sigma_net[-1].weight[0] *= 40.0
    ro, rd = _rays(512, 61)
    tgt = np.random.default_rng(62).uniform(0, 1, (512, 3)).astype(np.float32)
    out = {"bitfield": bits.numpy(), "rays_o": ro, "rays_d": rd, "target": tgt, "table_seed": 5, "bound": bound}
    for i, l in enumerate(model.sigma_net):
        out[f"w_sigma_{i}"] = l.weight.detach().numpy().copy()
    for i, l in enumerate(model.color_net):
        out[f"w_color_{i}"] = l.weight.detach().numpy().copy()
    model.train()
    assert not torch.is_autocast_enabled("cuda") and not torch.is_autocast_enabled("cpu")
    res = model.render(torch.from_numpy(ro)[None], torch.from_numpy(rd)[None], staged=False, bg_color=1, perturb=True, force_all_rays=False,
                       dt_gamma=1 / 128, max_steps=1024)
    assert res["image"].dtype == torch.float32 and model.last_sigma.dtype == torch.float32
    loss = torch.nn.functional.mse_loss(res["image"][0], torch.from_numpy(tgt))
    loss.backward()
    m = int(model.step_counter[0, 0])
    keep = min(m, 8192)
    g = model.encoder.embeddings.grad
    assert g.dtype == torch.float32
    nz = torch.nonzero(g.abs().sum(-1)).squeeze(-1)
    pick = nz[torch.from_numpy(np.random.default_rng(63).choice(nz.numel(), 2048, replace=False)).long()]
    off = model.encoder.offsets.long()
    out.update(train_image=res["image"][0].detach().numpy(), train_depth=res["depth"][0].detach().numpy(),
               train_counter=model.step_counter[0].numpy().copy(), train_loss=float(loss),
               train_xyz=model.last_xyz[:keep].numpy(), train_sigma=model.last_sigma[:keep].numpy(), train_rgb=model.last_color[:keep].numpy(),
               g_table_rows=pick.numpy(), g_table_vals=g[pick].numpy(), g_table_nonzero_rows=int(nz.numel()),
               g_table_level_abs=np.array([float(g[off[l]:off[l + 1]].abs().double().sum()) for l in range(16)]))
    for i, l in enumerate(model.sigma_net):
        out[f"g_sigma_{i}"] = l.weight.grad.numpy().copy()
    for i, l in enumerate(model.color_net):
        out[f"g_color_{i}"] = l.weight.grad.numpy().copy()
    model.eval()
    ro2, rd2 = _rays(512, 71)
    with torch.no_grad():
        res = model.render(torch.from_numpy(ro2)[None], torch.from_numpy(rd2)[None], staged=False, bg_color=1, perturb=False, dt_gamma=1 / 128,
                           max_steps=1024)
    out.update(infer_rays_o=ro2, infer_rays_d=rd2, infer_image=res["image"][0].numpy(), infer_depth=res["depth"][0].numpy())
    np.savez_compressed(os.path.join(OUT, "ref_python_run_cuda_fp32.npz"), **out)
    print("ref_python_run_cuda_fp32.npz: train", m, "samples /", int(out["train_counter"][1]), "rays; loss", out["train_loss"],
          "sigma range", float(out["train_sigma"].min()), float(out["train_sigma"].max()))


    round4_projector_gradients()


def round4_projector_gradients():
    """MeshProjector.project(requires_grad_xyz=True) -- diff_project_layer, tools/map.py:171-186, :431-432 -- and its use_dir_vec=False
    form, executed on the mesh and points of ref_python_projector.npz; and the branch of network_curvedfield.NeRFNetwork.forward that
    differentiates sigma with respect to the sample position (nerf/network_curvedfield.py:236-259, use_grad_normal=True) executed with the
    curved field of ref_python_curvedfield.npz: the normal it forms from that gradient is captured as torch.autograd.grad returns it."""
    import torch

    install_reference_imports()
    _install_map_imports()
    import tools.map as ref_map
    from RayTracer import RayTracer as RefRayTracer

    g = np.load(os.path.join(OUT, "ref_python_projector.npz"))
    c = np.load(os.path.join(OUT, "ref_python_curvedfield.npz"))
    v, f, vn, tbn, pts = g["vertices"], g["faces"], g["vertex_normals"], g["tbn"], g["xyz"]
    mp = object.__new__(ref_map.MeshProjector)
    mp.mesh_vertices, mp.vertex_normals, mp.tbn = torch.from_numpy(v), torch.from_numpy(vn), torch.from_numpy(tbn)
    mp.grid, mp.radius, mp.max_K, mp.depth_threshold = None, 100.0, v.shape[0], 9.5
    mp.raytracer = RefRayTracer(v, f)
    rng = np.random.default_rng(81)
    x = torch.from_numpy(pts).clone().requires_grad_(True)
    p_sur, sdf, h_mask, normal, _ = mp.project(x, K=8, h_threshold=0.05, requires_grad_xyz=True)
    assert np.array_equal(p_sur.detach().numpy(), g["p_sur"])
    g_psur = rng.normal(size=p_sur.shape).astype(np.float32)
    g_sdf = rng.normal(size=sdf.shape).astype(np.float32)
    ((p_sur * torch.from_numpy(g_psur)).sum() + (sdf * torch.from_numpy(g_sdf)).sum()).backward()
    out = dict(g_psur=g_psur, g_sdf=g_sdf, grad_xyz=x.grad.numpy().copy())
    with torch.no_grad():
        p2, s2, m2, n2, _ = mp.project(torch.from_numpy(pts), K=8, h_threshold=None, use_dir_vec=False)
    out.update(nodir_p_sur=p2.numpy(), nodir_sdf=s2.numpy(), nodir_h_mask=m2.numpy(), nodir_normal=n2.numpy())

    # the curved field as round3_goldens builds it (same seeds -> same table and weights: checked against the fixture)
    for name, cls in (("sg_light_model", "SG_EnvmapMaterialNet"), ("sh_light_model", "SH_EnvmapMaterialNet"), ("envmap_light_model", "Envmap_EnvmapMaterialNet")):
        _stub("nerf." + name, **{cls: None})
    import nerf.network_curvedfield as ref_cf
    from tools.encoding import get_encoder

    torch.manual_seed(0)
    mff = object.__new__(ref_map.MeshFeatureField)
    torch.nn.Module.__init__(mff)
    mff.h_threshold, mff.K, mff.bound, mff.hash, mff.prob_model, mff.pred_normal, mff.clustering = 0.05, 8, 1, True, False, False, True
    mff.imported, mff.imported_type, mff.normal_net = False, None, None
    mff.encoder, mff.encoder_f_out_dim = get_encoder("hashgrid_clustering", desired_resolution=1024, input_dim=3, num_levels=8, level_dim=2, base_resolution=512,
                                                     log2_hashmap_size=19, align_corners=True)
    mff.encoder_z, mff.encoder_z_outdim = get_encoder("frequency", input_dim=1, multires=12)
    mff.meshprojector = mp
    gen = torch.Generator().manual_seed(int(c["table_seed"]))
    mff.encoder.embeddings.data.copy_(torch.rand(mff.encoder.embeddings.shape, generator=gen) - 0.5)
    net = object.__new__(ref_cf.NeRFNetwork)
    torch.nn.Module.__init__(net)
    net.visual_mode, net.render_light_model, net.use_grad_normal, net.fc_weight, net.dir_degree = "RGB", False, True, 1.0, 4
    net.optimize_gamma, net.meshfea_field = False, mff
    tcnn = sys.modules["tinycudann"]
    torch.manual_seed(42)
    net.sigma_net = tcnn.Network(n_input_dims=mff.encoder_z_outdim + mff.encoder_f_out_dim, n_output_dims=16,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 1})
    net.encoder_dir = tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "SphericalHarmonics", "degree": 4})
    net.color_net = tcnn.Network(n_input_dims=net.encoder_dir.n_output_dims + 15, n_output_dims=3,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2})
    assert np.array_equal(net.sigma_net.net.weights.detach().numpy(), c["w_sigma"]), "the curved field of ref_python_curvedfield.npz"
    net.train()  # (the in-tree FFMLP that stands in for tcnn keeps no activations in eval mode: its backward needs the training forward)
    captured = []
    real_grad = torch.autograd.grad

    def spy(*a, **k):
        res = real_grad(*a, **k)
        captured.append(res[0].detach().clone())
        return res

    torch.autograd.grad = spy
    try:
        with emulated_autocast():
            sigma, color, _ = net(torch.from_numpy(pts).clone(), torch.from_numpy(c["dirs"]))
    finally:
        torch.autograd.grad = real_grad
    assert len(captured) == 1
    out.update(grad_normal_sigma=sigma.detach().float().numpy(), grad_normal_dsigma_remap_dx=captured[0].float().numpy())
    np.savez_compressed(os.path.join(OUT, "ref_python_projector_grad.npz"), **out)
    print("ref_python_projector_grad.npz: |dL/dxyz| max", float(np.abs(out["grad_xyz"]).max()), "; d sigma_remap / dx max", float(np.abs(out["grad_normal_dsigma_remap_dx"]).max()),
          "nonzero rows", int((np.abs(out["grad_normal_dsigma_remap_dx"]).sum(-1) > 0).sum()), "of", pts.shape[0])


# ---------------------------------------------------------------------------------------------------------------------------
# Round 5: the factorized normal net of MeshFeatureField (tools/map.py:189-337, used at :585-588, :637-641, :726-732)
# ---------------------------------------------------------------------------------------------------------------------------
def round5_goldens():
    """`Factorized_Normal_Net(x_dim=16, z_dim=25, lip=True, direct_pred_coor=False)` -- the reference's class, executed in fp32 on the CPU over the
    oracle's hash-grid kernels (its phi table: get_encoder('hashgrid', L = 4, 512 -> 1024), tools/map.py:235) -- with LipMLP / LipLayer as they are:
    forward (local normal, the two angles, the bound_output form), MeshFeatureField's rotation into the world (:727, :732), regularization(), and
    the gradients of a scalar loss with respect to every LipLayer parameter, the phi table, the surface points (the hash grid's input gradient,
    G3), the texture features and the height bands."""
    import torch

    _install_map_imports()
    import tools.map as ref_map

    torch.manual_seed(11)
    net = ref_map.Factorized_Normal_Net(x_dim=16, z_dim=25, lip=True, direct_pred_coor=False, bound_output=False)
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        net.encoder.embeddings.copy_(torch.rand(net.encoder.embeddings.shape, generator=gen) - 0.5)
        for mlp in (net.phi_net, net.theta_net):
            for layer in mlp.layers:  # biases and bounds away from their initial 0 / 1, so that both sides of the row clamp occur
                layer.b.copy_(torch.rand(layer.b.shape, generator=gen) * 0.2 - 0.1)
                layer.c.copy_(torch.rand((), generator=gen) * 1.5 + 0.25)
    N = 640
    p_sur = ((torch.rand(N, 3, generator=gen) * 2 - 1) * 0.9).requires_grad_(True)
    z_embed = (torch.randn(N, 25, generator=gen) * 0.7).requires_grad_(True)
    x_embed = (torch.randn(N, 16, generator=gen) * 0.5).requires_grad_(True)
    q, _ = torch.linalg.qr(torch.randn(N, 3, 3, generator=gen))
    tbn = q.contiguous()
    out = dict(p_sur=p_sur.detach().numpy(), z_embed=z_embed.detach().numpy(), x_embed=x_embed.detach().numpy(), tbn=tbn.numpy(), table_seed=12,
               table_rows=int(net.encoder.embeddings.shape[0]), offsets=net.encoder.offsets.numpy().copy(), per_level_scale=float(net.encoder.per_level_scale))
    for name, mlp in (("phi", net.phi_net), ("theta", net.theta_net)):
        for i, layer in enumerate(mlp.layers):
            out[f"{name}_W{i}"], out[f"{name}_b{i}"], out[f"{name}_c{i}"] = layer.W.detach().numpy().copy(), layer.b.detach().numpy().copy(), float(layer.c)
            out[f"{name}_Wn{i}"] = layer.normalization().detach().numpy()
    local = net(p_sur=p_sur, z_embed=z_embed, x_embed=x_embed)                       # tools/map.py:639
    theta, phi = net(p_sur=p_sur, z_embed=z_embed, x_embed=x_embed, return_rot_angles=True)  # :643
    fine = torch.einsum("nba,nb->na", tbn, local)                                    # :727
    fine = fine / (fine.norm(dim=-1, keepdim=True) + 1e-5)                           # :732
    reg = net.regularization()
    gw = torch.randn(N, 3, generator=gen)
    loss = (fine * gw).sum() + 0.1 * reg
    loss.backward()
    gt = net.encoder.embeddings.grad
    nz = torch.nonzero(gt.abs().sum(-1)).squeeze(-1)
    out.update(normal_local=local.detach().numpy(), theta=theta.detach().numpy(), phi=phi.detach().numpy(), normal_fine=fine.detach().numpy(), regularization=float(reg),
               phi_embed=net.phi_embedding(p_sur).detach().numpy(), grad_w=gw.numpy(), g_p_sur=p_sur.grad.numpy().copy(), g_z_embed=z_embed.grad.numpy().copy(),
               g_x_embed=x_embed.grad.numpy().copy(), g_table_rows=nz.numpy(), g_table_vals=gt[nz].numpy(), g_table_abs=float(gt.abs().double().sum()))
    for name, mlp in (("phi", net.phi_net), ("theta", net.theta_net)):
        for i, layer in enumerate(mlp.layers):
            out[f"g_{name}_W{i}"], out[f"g_{name}_b{i}"], out[f"g_{name}_c{i}"] = layer.W.grad.numpy().copy(), layer.b.grad.numpy().copy(), float(layer.c.grad)
    net.bound_output = True
    with torch.no_grad():
        out["normal_local_bounded"] = net(p_sur=p_sur, z_embed=z_embed, x_embed=x_embed, tbn=tbn).numpy()  # (with its own `tbn` argument: :335-337)
    np.savez_compressed(os.path.join(OUT, "ref_python_normal_net.npz"), **out)
    print("ref_python_normal_net.npz: theta", float(theta.min()), float(theta.max()), "phi", float(phi.min()), float(phi.max()), "regularization", float(reg),
          "rows with a gradient", int(nz.shape[0]), "|dL/dp_sur| max", float(p_sur.grad.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------
# The SH light head: nerf/sh_light_model.py's SH_EnvmapMaterialNet.forward (:554-616) and its autograd, executed
# ---------------------------------------------------------------------------------------------------------------------------
def sh_light_goldens():
    """ref_python_sh_light.npz: the real nerf.sh_light_model imported (cv2, imageio and tools.shape_tools stubbed: file output and image
    loading, never reached; tinycudann = the stand-in of _install_map_imports) and SH_EnvmapMaterialNet.forward run on the CPU under the
    emulated autocast with its backward, 768 samples per case.  Cases `w<white_light>s<use_specular>` + `dark` (coloured light whose
    irradiance changes sign over the sphere: the clamps and safe_pow's threshold are exercised).  Per case: geo_feat, normals, dirs, the BRDF
    MLP's weights, envSHs, brdf (the MLP's 5 outputs as the head saw them), the four outputs, grad_color and the gradients that reached
    brdf and envSHs.  Writes this one file; no other fixture is touched."""
    import torch

    _install_map_imports()
    for name in ("imageio", "tools.shape_tools"):
        _stub(name, write_ply_rgb=None)
    sys.modules.pop("nerf.sh_light_model", None)  # (round3_goldens stubs it when it ran first)
    import nerf.sh_light_model as ref_sh

    N = 768
    rng = np.random.default_rng(71)
    out = {}
    for case, white, spec in (("w1s1", True, True), ("w1s0", True, False), ("w0s1", False, True), ("w0s0", False, False), ("dark", False, True)):
        net = ref_sh.SH_EnvmapMaterialNet(input_dim=15, sh_order=3, white_light=white, use_specular=spec)
        C = 1 if white else 3
        env = net.envSHs.data  # zeros with row 0 = 3: the reference's initialisation
        if case == "dark":
            env[0] = 0.05
            env[1:] = torch.from_numpy(rng.normal(0, 0.4, (15, C)).astype(np.float32))
        else:
            env[1:] = torch.from_numpy(rng.normal(0, 0.1, (15, C)).astype(np.float32))
        geo = torch.from_numpy(rng.normal(0, 1.0, (N, 15)).astype(np.float32)).half()
        n = rng.normal(size=(N, 3))
        n = torch.from_numpy((n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32))
        d = rng.normal(size=(N, 3))
        d = torch.from_numpy((d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32))
        gc = torch.from_numpy(rng.normal(size=(N, 3)).astype(np.float32))
        seen = {}
        handle = net.brdf_layer.register_forward_hook(lambda m, i, o: (o.retain_grad(), seen.__setitem__("brdf", o))[1])
        net.train()
        with emulated_autocast():
            color, specular, diffuse, albedo = net(geo, n, d)
            (color * gc).sum().backward()
        handle.remove()
        brdf = seen["brdf"]
        assert brdf.dtype == torch.float16 and brdf.shape == (N, 5) and color.dtype == torch.float32 and albedo.dtype == torch.float16
        out.update({f"{case}_geo_feat": geo.numpy(), f"{case}_normals": n.numpy(), f"{case}_dirs": d.numpy(), f"{case}_grad_color": gc.numpy(),
                    f"{case}_w_brdf": net.brdf_layer.net.weights.detach().numpy().copy(), f"{case}_env_shs": env.numpy().copy(),
                    f"{case}_brdf": brdf.detach().numpy().copy(), f"{case}_color": color.detach().numpy(), f"{case}_specular": specular.detach().float().numpy(),
                    f"{case}_diffuse": diffuse.detach().numpy(), f"{case}_albedo": albedo.detach().float().numpy(),
                    f"{case}_g_brdf": brdf.grad.numpy().copy(), f"{case}_g_env_shs": net.envSHs.grad.numpy().copy(),
                    f"{case}_g_w_brdf": net.brdf_layer.net.weights.grad.numpy().copy()})
        print(f"ref_python_sh_light.npz[{case}]: color range", float(color.min()), float(color.max()), "|g_brdf[:, 4]| max", float(brdf.grad[:, 4].abs().max()),
              "g_env rows >= 9 abs max", float(net.envSHs.grad[9:].abs().max()))
    sd = net.state_dict()
    out["state_dict_keys"] = np.array(sorted(sd))
    out["state_dict_shapes"] = np.array([",".join(map(str, sd[k].shape)) + ":" + str(sd[k].dtype) for k in sorted(sd)])
    out["gamma"] = np.float64(net.gamma)
    np.savez_compressed(os.path.join(OUT, "ref_python_sh_light.npz"), **out)


def sh_field_goldens():
    """ref_python_curvedfield_sh.npz: network_curvedfield.NeRFNetwork.forward executed with render_light_model=True (light_model 'SH', the
    real SH_EnvmapMaterialNet, white light as NeRFNetwork's default) over MeshFeatureField(pred_normal=True) with the reference's
    Factorized_Normal_Net, on the mesh and points of ref_python_projector.npz -- the setup of ref_python_curvedfield.npz plus the normal
    net and the light head.  Eval with fc_weight = 0.7 (the fine / coarse blend of :299-301 is exercised) and the four light_visual_modes;
    train (the branch of :236-258 that differentiates sigma, create_graph and all) with the ret_dict; in both, the shading normal and the
    view direction as the light head receives them (:331-341), captured by a hook on the head.  Values only.  Reads two existing
    fixtures; writes this one file."""
    import torch

    net, mff, x, d, out = sh_field_network()
    handed = {}  # what NeRFNetwork.forward hands to the light head (:341): the shading normal and the view direction
    net.light_net.register_forward_pre_hook(lambda m, a: handed.update(normal=a[1].detach().float().numpy().copy(), view_dirs=a[2].detach().float().numpy().copy(),
                                                                       normal_attached=bool(a[1].requires_grad)))
    net.eval()
    with torch.no_grad(), emulated_autocast():
        _, nc, nf, hm = mff(x)
        out.update(eval_normal_coarse=nc.float().numpy(), eval_normal_fine=nf.float().numpy(), eval_h_mask=hm.numpy())
        for mode in ("Full", "Specular", "Diffuse", "Albedo"):
            net.light_visual_mode = mode
            sigma, color, ret = net(x, d, is_gui_mode=False)
            assert ret == {}
            out["eval_sigma"], out["eval_color_" + mode.lower()] = sigma.float().numpy(), color.float().numpy()
        net.light_visual_mode = "Full"
        out.update(eval_shading_normal=handed["normal"], eval_view_dirs=handed["view_dirs"])
    net.train()
    with emulated_autocast():
        sigma, color, ret = net(x.clone(), d)
    assert sorted(ret) == ["normal", "normal_grad"] and ret["normal"].requires_grad
    assert not handed["normal_attached"], "the training head shades with the detached normal (:331)"
    out.update(train_shading_normal=handed["normal"], train_view_dirs=handed["view_dirs"])
    out.update(train_sigma=sigma.detach().float().numpy(), train_color=color.detach().float().numpy(), train_normal=ret["normal"].detach().float().numpy(),
               train_normal_grad=ret["normal_grad"].detach().float().numpy(), train_h_mask=(sigma.detach() != 0).numpy() | (color.detach() != 0).any(-1).numpy())
    np.savez_compressed(os.path.join(OUT, "ref_python_curvedfield_sh.npz"), **out)
    print("ref_python_curvedfield_sh.npz: eval colour", float(out["eval_color_full"].min()), float(out["eval_color_full"].max()), "inside", float(out["eval_h_mask"].mean()),
          "train rows shaded", float(out["train_h_mask"].mean()), "normal_grad not a number on", int(np.isnan(out["train_normal_grad"]).any(-1).sum()), "rows")


def sh_field_network():
    """The construction of ref_python_curvedfield_sh.npz (sh_field_goldens; tools/make_relight_golden.py builds on it too): -> the reference's
    NeRFNetwork with the SH light head over its MeshFeatureField, that field, the 768 points and directions as tensors, and the dictionary of
    the seeds and weights the fixture records."""
    import torch

    _install_map_imports()
    _stub("imageio")
    for name in ("nerf.sh_light_model", "nerf.network_curvedfield", "tools.shape_tools"):  # (stubs of earlier functions: tools/map.py needs the real shape_tools)
        sys.modules.pop(name, None)
    for name, cls in (("sg_light_model", "SG_EnvmapMaterialNet"), ("envmap_light_model", "Envmap_EnvmapMaterialNet")):
        _stub("nerf." + name, **{cls: None})
    import nerf.network_curvedfield as ref_cf
    import nerf.sh_light_model as ref_sh
    import tools.map as ref_map
    from RayTracer import RayTracer as RefRayTracer
    from tools.encoding import get_encoder

    g = np.load(os.path.join(OUT, "ref_python_projector.npz"))
    c = np.load(os.path.join(OUT, "ref_python_curvedfield.npz"))
    v, f, vn, tbn, pts, dirs = g["vertices"], g["faces"], g["vertex_normals"], g["tbn"], g["xyz"], c["dirs"]
    mp = object.__new__(ref_map.MeshProjector)
    mp.mesh_vertices, mp.vertex_normals, mp.tbn = torch.from_numpy(v), torch.from_numpy(vn), torch.from_numpy(tbn)
    mp.grid, mp.radius, mp.max_K, mp.depth_threshold = None, 100.0, v.shape[0], 9.5
    mp.raytracer = RefRayTracer(v, f)
    torch.manual_seed(0)
    mff = object.__new__(ref_map.MeshFeatureField)
    torch.nn.Module.__init__(mff)
    mff.h_threshold, mff.K, mff.bound, mff.hash, mff.prob_model, mff.pred_normal, mff.clustering = 0.05, 8, 1, True, False, True, True
    mff.imported, mff.imported_type = False, None
    mff.encoder, mff.encoder_f_out_dim = get_encoder("hashgrid_clustering", desired_resolution=1024, input_dim=3, num_levels=8, level_dim=2, base_resolution=512,
                                                     log2_hashmap_size=19, align_corners=True)
    mff.encoder_z, mff.encoder_z_outdim = get_encoder("frequency", input_dim=1, multires=12)
    mff.meshprojector = mp
    gen = torch.Generator().manual_seed(int(c["table_seed"]))
    mff.encoder.embeddings.data.copy_(torch.rand(mff.encoder.embeddings.shape, generator=gen) - 0.5)
    torch.manual_seed(11)
    mff.normal_net = ref_map.Factorized_Normal_Net(x_dim=mff.encoder_f_out_dim, z_dim=mff.encoder_z_outdim, lip=True, direct_pred_coor=False, bound_output=False)
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        mff.normal_net.encoder.embeddings.copy_(torch.rand(mff.normal_net.encoder.embeddings.shape, generator=gen) - 0.5)
    net = object.__new__(ref_cf.NeRFNetwork)
    torch.nn.Module.__init__(net)
    net.visual_mode, net.render_light_model, net.use_grad_normal, net.fc_weight, net.dir_degree = "RGB", True, False, 0.7, 4
    net.optimize_gamma, net.meshfea_field, net.light_model, net.smooth_grad_weight = False, mff, "SH", 1e-1
    net.use_coarse_normal, net.coarse_as_primary, net.no_visibility, net.shade_visibility, net.light_visual_mode = False, False, False, True, "Full"
    tcnn = sys.modules["tinycudann"]
    torch.manual_seed(42)
    net.sigma_net = tcnn.Network(n_input_dims=mff.encoder_z_outdim + mff.encoder_f_out_dim, n_output_dims=16,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 1})
    assert np.array_equal(net.sigma_net.net.weights.detach().numpy(), c["w_sigma"]), "the sigma net of ref_python_curvedfield.npz"
    net.color_net = None
    net.light_net = ref_sh.SH_EnvmapMaterialNet(input_dim=15, sh_order=3, white_light=True, use_specular=True)
    rng = np.random.default_rng(91)
    with torch.no_grad():
        # bands 1 and 2 comparable to the DC term: the colour then depends on WHICH normal shades the sample (fine, coarse or their blend)
        net.light_net.envSHs[1:] = torch.from_numpy(rng.normal(0, 1.5, (15, 1)).astype(np.float32))
    x, d = torch.from_numpy(pts), torch.from_numpy(dirs)
    out = dict(table_seed=int(c["table_seed"]), normal_table_seed=12, fc_weight=0.7, w_sigma=c["w_sigma"], w_brdf=net.light_net.brdf_layer.net.weights.detach().numpy().copy(),
               env_shs=net.light_net.envSHs.detach().numpy().copy())
    for name, mlp in (("phi", mff.normal_net.phi_net), ("theta", mff.normal_net.theta_net)):
        for i, layer in enumerate(mlp.layers):
            out[f"{name}_W{i}"], out[f"{name}_b{i}"], out[f"{name}_c{i}"] = layer.W.detach().numpy().copy(), layer.b.detach().numpy().copy(), float(layer.c)
    return net, mff, x, d, out


def import_field_goldens():
    """ref_python_import_field.npz: MeshFeatureField.import_field (tools/map.py:912-927) and the `imported_type == 'field'` branch of its forward
    (:646-668, 719-720) executed, with network_curvedfield.NeRFNetwork.forward / density behind it (static light model, the sigma and colour nets
    of ref_python_curvedfield.npz), on the CPU: a seeded 24 x 20 x 16 feature map, grid_gap 1/32, h_threshold 0.0625, 512 points uniform in
    [-1.1, 1.1]^2 x [-0.22, 0.22], seeded directions.  Mode A (`rescale` True: the state after the first import) and mode B (after a second
    import), each with (uv_utilize_rate, sdf_offset) = (1, 0) and (0.8, 0.01).  The embedding is kept for A (1, 0) and B (0.8, 0.01); mask,
    sigma and colour for all four.  Inputs and outputs only: the weights are the other fixture's.  Reads one fixture; writes this one file."""
    import time

    import torch

    started = time.time()

    _install_map_imports()
    for name, cls in (("sg_light_model", "SG_EnvmapMaterialNet"), ("sh_light_model", "SH_EnvmapMaterialNet"), ("envmap_light_model", "Envmap_EnvmapMaterialNet")):
        if "nerf." + name not in sys.modules:
            _stub("nerf." + name, **{cls: None})
    import nerf.network_curvedfield as ref_cf
    import tools.map as ref_map
    from tools.encoding import get_encoder

    c = np.load(os.path.join(OUT, "ref_python_curvedfield.npz"))
    H, W, grid_gap, h_threshold = 24, 20, 1.0 / 32, 0.0625
    rng = np.random.default_rng(151)
    features = rng.uniform(-0.5, 0.5, (H, W, 16)).astype(np.float32)
    pts = rng.uniform(-1.0, 1.0, (512, 3)).astype(np.float32) * np.array([1.1, 1.1, 0.22], np.float32)
    dirs = rng.normal(size=(512, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)

    mff = object.__new__(ref_map.MeshFeatureField)
    torch.nn.Module.__init__(mff)
    mff.device, mff.h_threshold, mff.K, mff.bound, mff.hash, mff.prob_model, mff.pred_normal, mff.clustering = "cpu", h_threshold, 8, 1, True, False, False, True
    mff.imported, mff.imported_type, mff.normal_net, mff.rescale = False, None, None, False  # (the constructor's values, :604-618)
    mff.sdf_scale_factor, mff.sdf_offset, mff.uv_utilize_rate, mff.K_for_uv = 1.0, 0.0, 1.0, 5
    mff.encoder_f_out_dim = 16
    mff.encoder_z, mff.encoder_z_outdim = get_encoder("frequency", input_dim=1, multires=12)
    net = object.__new__(ref_cf.NeRFNetwork)
    torch.nn.Module.__init__(net)
    net.visual_mode, net.render_light_model, net.use_grad_normal, net.fc_weight, net.dir_degree = "RGB", False, False, 1.0, 4
    net.optimize_gamma, net.meshfea_field = False, mff
    tcnn = sys.modules["tinycudann"]
    torch.manual_seed(42)
    net.sigma_net = tcnn.Network(n_input_dims=mff.encoder_z_outdim + mff.encoder_f_out_dim, n_output_dims=16,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 1})
    net.encoder_dir = tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "SphericalHarmonics", "degree": 4})
    net.color_net = tcnn.Network(n_input_dims=net.encoder_dir.n_output_dims + 15, n_output_dims=3,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2})
    assert np.array_equal(net.sigma_net.net.weights.detach().numpy(), c["w_sigma"]) and np.array_equal(net.color_net.net.weights.detach().numpy(), c["w_color"])
    net.eval()

    def do_import():  # (the maps only a normal net reads: placeholders of the right rank)
        mff.import_field(features, bounds=[0.5 * grid_gap * H, 0.5 * grid_gap * W], sample_tbn=np.eye(3, dtype=np.float32)[None], sample_tbn_ids=np.zeros((H, W), np.float32),
                         local_tbn=np.zeros((H, W, 9), np.float32), phi_embed=np.zeros((H, W, 8), np.float32))

    x, d = torch.from_numpy(pts), torch.from_numpy(dirs)
    out = dict(features=features, grid_gap=grid_gap, h_threshold=h_threshold, xyz=pts, dirs=dirs, weights_of="ref_python_curvedfield.npz")
    for mode in ("A", "B"):
        do_import()
        assert mff.rescale == (mode == "A") and tuple(mff.features_imported.shape) == (1, 16, W, H)
        for k, (rate, off) in enumerate(((1.0, 0.0), (0.8, 0.01))):
            mff.uv_utilize_rate, mff.sdf_offset = rate, off
            with torch.no_grad(), emulated_autocast():
                embed, nc, _, hm = mff(x)
                sigma, color, _ = net(x, d)
                dens = net.density(x)
            assert torch.equal(dens["sigma"], sigma) and torch.equal(color.half().float(), color.float())
            key = f"{mode}{k}"
            out.update({key + "_rate": rate, key + "_offset": off, key + "_h_mask": hm.numpy(), key + "_sigma": sigma.float().numpy(),
                        key + "_color": color.half().numpy()})
            if key in ("A0", "B1"):
                out.update({key + "_embed": embed.float().numpy()})
                assert torch.equal(nc, torch.tensor([0.0, 0.0, 1.0]).expand_as(nc) / (1 + 1e-5))
            print("ref_python_import_field.npz:", key, "inside the mask", float(hm.float().mean()), "sigma max", float(sigma.max()))
    np.savez_compressed(os.path.join(OUT, "ref_python_import_field.npz"), **out)
    new = [os.path.join(r, n) for r, _, names in os.walk(REF) for n in names if os.lstat(os.path.join(r, n)).st_mtime >= started]
    assert not new, "files appeared under the reference tree:\n" + "\n".join(new[:20])


def import_field_sh_goldens():
    """ref_python_import_field_sh.npz: MeshFeatureField.import_field (tools/map.py:912-927) with all six arguments and the `pred_normal` part of
    the `imported_type == 'field'` branch (:646-675, :722-730) executed, with network_curvedfield.NeRFNetwork.forward behind it in eval with
    the real SH_EnvmapMaterialNet (light_model 'SH', white light), on the CPU under emulated_autocast.  A seeded 24 x 20 map set (16
    features, 8 phi features, a frame and a patch id per texel), P = 5 patch frames; the frames are NOT orthonormal (inverse != transpose)
    and differ per texel and per patch.  512 points: the first half uniform in [-1.1, 1.1]^2 x [-0.22, 0.22] (both sides of every edge with
    `rescale`), the second in [-0.42, 0.42] x [-0.35, 0.35] x [-0.09, 0.09] (likewise without).  Mode A (`rescale` True: after the first
    import) and mode B (after a second import), fc_weight 1.0 and 0.7, the four light_visual_modes.  Recorded: inputs, weights, h_mask, what
    the four grid_sample calls and the table of inverted frames returned (a recorder around grid_sample and a hook on the normal net), the
    fine normal, the shading normal handed to the head (a hook on the head), sigma and the four colours.  The normal net's weights are
    scaled up so that its angles are of order 1.  Values only.  Reads one fixture (the sigma net's weights, as a check); writes this one."""
    import time

    import torch

    started = time.time()
    _install_map_imports()
    _stub("imageio")
    for name in ("nerf.sh_light_model", "nerf.network_curvedfield", "tools.shape_tools"):
        sys.modules.pop(name, None)
    for name, cls in (("sg_light_model", "SG_EnvmapMaterialNet"), ("envmap_light_model", "Envmap_EnvmapMaterialNet")):
        _stub("nerf." + name, **{cls: None})
    import nerf.network_curvedfield as ref_cf
    import nerf.sh_light_model as ref_sh
    import tools.map as ref_map
    from tools.encoding import get_encoder

    c = np.load(os.path.join(OUT, "ref_python_curvedfield.npz"))
    H, W, P, grid_gap, h_threshold = 24, 20, 5, 1.0 / 32, 0.0625
    rng = np.random.default_rng(171)
    features = rng.uniform(-0.5, 0.5, (H, W, 16)).astype(np.float32)
    phi_embed = rng.uniform(-0.5, 0.5, (H, W, 8)).astype(np.float32)
    local_tbn = (np.eye(3, dtype=np.float32).reshape(9) + rng.normal(0, 0.35, (H, W, 9))).astype(np.float32)
    sample_tbn = (np.eye(3, dtype=np.float32) + rng.normal(0, 0.3, (P, 3, 3))).astype(np.float32)
    assert np.linalg.cond(sample_tbn.astype(np.float64)).max() < 50
    assert np.abs(np.linalg.inv(sample_tbn.astype(np.float64)) - np.swapaxes(sample_tbn, 1, 2)).max() > 0.1, "inverse != transpose"
    sample_tbn_ids = rng.integers(0, P, (H, W)).astype(np.float32)
    pts = rng.uniform(-1.0, 1.0, (512, 3)).astype(np.float32)
    pts[:256] *= np.array([1.1, 1.1, 0.22], np.float32)
    pts[256:] *= np.array([0.42, 0.35, 0.09], np.float32)
    dirs = rng.normal(size=(512, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)

    mff = object.__new__(ref_map.MeshFeatureField)
    torch.nn.Module.__init__(mff)
    mff.device, mff.h_threshold, mff.K, mff.bound, mff.hash, mff.prob_model, mff.pred_normal, mff.clustering = "cpu", h_threshold, 8, 1, True, False, True, True
    mff.imported, mff.imported_type, mff.rescale = False, None, False  # (the constructor's values, :604-618)
    mff.sdf_scale_factor, mff.sdf_offset, mff.uv_utilize_rate, mff.K_for_uv = 1.0, 0.0, 1.0, 5
    mff.encoder_f_out_dim = 16
    mff.encoder_z, mff.encoder_z_outdim = get_encoder("frequency", input_dim=1, multires=12)
    torch.manual_seed(11)
    mff.normal_net = ref_map.Factorized_Normal_Net(x_dim=mff.encoder_f_out_dim, z_dim=mff.encoder_z_outdim, lip=True, direct_pred_coor=False, bound_output=False)
    gen = torch.Generator().manual_seed(13)
    with torch.no_grad():
        for mlp in (mff.normal_net.phi_net, mff.normal_net.theta_net):
            for layer in mlp.layers:
                layer.W.mul_(6.0)
                layer.b.copy_(torch.randn(layer.b.shape, generator=gen) * 0.3)
                layer.c.fill_(2.0)
    net = object.__new__(ref_cf.NeRFNetwork)
    torch.nn.Module.__init__(net)
    net.visual_mode, net.render_light_model, net.use_grad_normal, net.fc_weight, net.dir_degree = "RGB", True, False, 1.0, 4
    net.optimize_gamma, net.meshfea_field, net.light_model, net.smooth_grad_weight = False, mff, "SH", 1e-1
    net.use_coarse_normal, net.coarse_as_primary, net.no_visibility, net.shade_visibility, net.light_visual_mode = False, False, False, True, "Full"
    tcnn = sys.modules["tinycudann"]
    torch.manual_seed(42)
    net.sigma_net = tcnn.Network(n_input_dims=mff.encoder_z_outdim + mff.encoder_f_out_dim, n_output_dims=16,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 1})
    assert np.array_equal(net.sigma_net.net.weights.detach().numpy(), c["w_sigma"]), "the sigma net of ref_python_curvedfield.npz"
    net.color_net = None
    net.light_net = ref_sh.SH_EnvmapMaterialNet(input_dim=15, sh_order=3, white_light=True, use_specular=True)
    with torch.no_grad():
        net.light_net.envSHs[1:] = torch.from_numpy(np.random.default_rng(91).normal(0, 1.5, (15, 1)).astype(np.float32))
    out = dict(features=features, phi_embed=phi_embed, local_tbn=local_tbn, sample_tbn=sample_tbn, sample_tbn_ids=sample_tbn_ids, grid_gap=grid_gap,
               h_threshold=h_threshold, xyz=pts, dirs=dirs, w_sigma=c["w_sigma"], w_brdf=net.light_net.brdf_layer.net.weights.detach().numpy().copy(),
               env_shs=net.light_net.envSHs.detach().numpy().copy())
    for name, mlp in (("phi", mff.normal_net.phi_net), ("theta", mff.normal_net.theta_net)):
        for i, layer in enumerate(mlp.layers):
            out[f"{name}_W{i}"], out[f"{name}_b{i}"], out[f"{name}_c{i}"] = layer.W.detach().numpy().copy(), layer.b.detach().numpy().copy(), float(layer.c)
    handed, sampled = {}, []
    net.light_net.register_forward_pre_hook(lambda m, a: handed.update(normal=a[1].detach().float().numpy().copy()))
    mff.normal_net.register_forward_pre_hook(lambda m, a, k: handed.update(phi=k["phi_embed"].detach().float().numpy().copy()), with_kwargs=True)
    real_grid_sample = torch.nn.functional.grid_sample

    def recording_grid_sample(*a, **k):
        r = real_grid_sample(*a, **k)
        sampled.append((k.get("mode", "bilinear"), r))
        return r

    x, d = torch.from_numpy(pts), torch.from_numpy(dirs)
    net.eval()
    torch.nn.functional.grid_sample = recording_grid_sample
    try:
        for mode in ("A", "B"):
            mff.import_field(features, bounds=[0.5 * grid_gap * H, 0.5 * grid_gap * W], sample_tbn=sample_tbn, sample_tbn_ids=sample_tbn_ids, local_tbn=local_tbn,
                             phi_embed=phi_embed)
            assert mff.rescale == (mode == "A") and tuple(mff.phi_embed_imported.shape) == (1, 8, W, H)
            with torch.no_grad(), emulated_autocast():
                del sampled[:]
                embed, nc, nf, hm = mff(x)
                assert [m for m, _ in sampled] == ["bilinear", "nearest", "nearest", "bilinear"]  # features, ids, local_tbn, phi_embed (:663-674)
                ids = sampled[1][1].squeeze().long()
                s_local = sampled[2][1].squeeze().permute(1, 0).reshape(-1, 3, 3)
                s_phi = sampled[3][1].squeeze().permute(1, 0)
                assert np.array_equal(s_phi.numpy(), handed["phi"])
                assert torch.equal(nc, torch.tensor([0.0, 0.0, 1.0]).expand_as(nc) / (1 + 1e-5))
                out.update({mode + "_h_mask": hm.numpy(), mode + "_embed": embed.float().numpy(), mode + "_phi": s_phi.numpy(), mode + "_local_tbn": s_local.numpy(),
                            mode + "_id": ids.numpy().astype(np.int32), mode + "_sample_tbn_inv": mff.sample_tbn_inv_imported[ids].numpy(),
                            mode + "_normal_fine": nf.float().numpy()})
                for fc in (1.0, 0.7):
                    net.fc_weight = fc
                    key = f"{mode}_fc{fc}"
                    for visual in ("Full", "Specular", "Diffuse", "Albedo"):
                        net.light_visual_mode = visual
                        sigma, color, ret = net(x, d, is_gui_mode=False)
                        assert ret == {}
                        out[f"{key}_color_{visual.lower()}"] = color.float().numpy()
                    out[mode + "_sigma"], out[key + "_shading_normal"] = sigma.float().numpy(), handed["normal"]
                print("ref_python_import_field_sh.npz:", mode, "inside the mask", float(hm.float().mean()), "sigma max", float(sigma.max()),
                      "fine normal away from the texel frame's third row by (median)", float(np.median(np.abs(nf.numpy() - s_local.numpy()[:, 2]).max(-1)[hm.numpy()])))
    finally:
        torch.nn.functional.grid_sample = real_grid_sample
    out["sample_tbn_inv"] = mff.sample_tbn_inv_imported.numpy().copy()
    np.savez_compressed(os.path.join(OUT, "ref_python_import_field_sh.npz"), **out)
    new = [os.path.join(r, n) for r, _, names in os.walk(REF) for n in names if os.lstat(os.path.join(r, n)).st_mtime >= started]
    assert not new, "files appeared under the reference tree:\n" + "\n".join(new[:20])


def import_shape_goldens():
    """ref_python_import_shape.npz: MeshFeatureField.import_shape (tools/map.py:939-949) and the `imported_type == 'shape'` branch of its forward
    (:693-700, 719-720) over MeshProjector.uvh / barycentric_mapping / knn (:454-543) executed on the CPU, with NeRFNetwork.forward / density
    behind it (the nets of ref_python_curvedfield.npz, the 24 x 20 x 16 map of ref_python_import_field.npz's recipe).  The new mesh: a seeded
    height field of 24 x 24 vertices over [-0.8, 0.8]^2 (no duplicated vertex: the reference produces no NaN row), per-vertex UVs an affine
    image of (x, y) plus a seeded perturbation of a tenth of the mean UV edge.  The MeshProjector is made past its trimesh / xatlas / open3d
    constructor: the three lines of it that matter (the UV mapping :361, the edge means :374-386) and NeRFNetwork.import_shape's
    normalisation (:496-498, behind trimesh.load_mesh) are restated here on the arrays.  frnn -> exact brute force, tracer -> the oracle.
    512 points within +-0.1 of the surface, a tenth pushed beyond the footprint (both traces miss).  Three states of (K_for_uv,
    uv_utilize_rate, sdf_scale_factor, sdf_offset): (5, 1, recommended, 0), (5, 0.8, recommended, 0.01), (3, 1.3, 2.0, 0).  Inputs and outputs
    only (uvh, mask, the coarse normal raw and normalised, the hit face, sigma, colour); the embedding is kept for the first and the last state."""
    import time

    import torch

    started = time.time()
    _install_map_imports()
    for name, cls in (("sg_light_model", "SG_EnvmapMaterialNet"), ("sh_light_model", "SH_EnvmapMaterialNet"), ("envmap_light_model", "Envmap_EnvmapMaterialNet")):
        if "nerf." + name not in sys.modules:
            _stub("nerf." + name, **{cls: None})
    import nerf.network_curvedfield as ref_cf
    import tools.map as ref_map
    from RayTracer import RayTracer as RefRayTracer
    from tools.encoding import get_encoder

    c = np.load(os.path.join(OUT, "ref_python_curvedfield.npz"))
    H, W, grid_gap, h_threshold = 24, 20, 1.0 / 32, 0.0625
    features = np.random.default_rng(151).uniform(-0.5, 0.5, (H, W, 16)).astype(np.float32)  # (ref_python_import_field.npz's map)
    rng = np.random.default_rng(163)
    n = 24
    gx, gy = np.meshgrid(np.linspace(-0.8, 0.8, n), np.linspace(-0.8, 0.8, n), indexing="ij")
    cell = 1.6 / (n - 1)
    gx, gy = gx + rng.uniform(-0.2, 0.2, gx.shape) * cell, gy + rng.uniform(-0.2, 0.2, gy.shape) * cell
    gz = 0.06 * np.sin(3.0 * gx) * np.cos(2.5 * gy) + rng.uniform(-0.01, 0.01, gx.shape)
    vertices_raw = np.stack([gx, gy, gz], -1).reshape(-1, 3)
    faces = []
    for a in range(n - 1):
        for b in range(n - 1):
            p, q, r, s = a * n + b, a * n + b + 1, (a + 1) * n + b, (a + 1) * n + b + 1
            faces += [(p, r, q), (q, r, s)]
    faces = np.asarray(faces, np.int64)
    uv_affine = np.stack([0.55 * vertices_raw[:, 0] + 0.1 * vertices_raw[:, 1] + 0.5, -0.08 * vertices_raw[:, 0] + 0.5 * vertices_raw[:, 1] + 0.5], -1)
    uvs_raw = (uv_affine + rng.uniform(-1, 1, uv_affine.shape) * 0.1 * 0.55 * cell).astype(np.float32)

    # NeRFNetwork.import_shape (:496-498) on the arrays
    vertices = vertices_raw.copy()
    vertices -= np.mean(vertices, axis=0)
    vertices /= (np.absolute(vertices).max() + 1e-5)
    vertices /= 1.2
    v32 = vertices.astype(np.float32)
    fn = np.cross(vertices[faces[:, 1]] - vertices[faces[:, 0]], vertices[faces[:, 2]] - vertices[faces[:, 0]])
    vn = np.zeros_like(vertices)
    for k in range(3):
        np.add.at(vn, faces[:, k], fn)
    vn = (vn / (np.linalg.norm(vn, axis=-1, keepdims=True) + 1e-12)).astype(np.float32)  # (the role of open3d's compute_vertex_normals)

    mp = object.__new__(ref_map.MeshProjector)
    uvs = torch.FloatTensor(uvs_raw)
    mp.uvs = (uvs - uvs.min()) / (uvs.max() - uvs.min()) * 2 - 1.  # :361
    edges_unique = np.unique(np.sort(faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1), axis=0)  # (trimesh's edges_unique as a set)
    edges = vertices[edges_unique]
    mp.mean_edge_length = np.linalg.norm(edges[:, 0] - edges[:, 1], axis=-1).mean()  # :374-376
    edges_uv = mp.uvs.numpy()[edges_unique]
    mp.recommended_sdf_factor = mp.mean_edge_length / np.linalg.norm(edges_uv[:, 0] - edges_uv[:, 1], axis=-1).mean()  # :382-386
    mp.mesh_vertices, mp.vertex_normals, mp.tbn = torch.FloatTensor(vertices), torch.from_numpy(vn), None
    mp.grid, mp.radius, mp.max_K, mp.depth_threshold = None, 100.0, v32.shape[0], 9.5
    mp.raytracer = RefRayTracer(v32, faces.astype(np.uint32))
    mp.faces = torch.from_numpy(faces).long()
    assert np.unique(v32, axis=0).shape[0] == v32.shape[0]

    # points: on the surface +- 0.1 along z, a tenth beyond the footprint
    pick, bary = rng.integers(0, len(faces), 512), rng.dirichlet([1, 1, 1], 512)
    pts = (vertices[faces[pick]] * bary[..., None]).sum(1)
    pts[:, 2] += rng.uniform(-0.1, 0.1, 512)
    out_rows = rng.choice(512, 51, replace=False)
    pts[out_rows, :2] = np.sign(pts[out_rows, :2] + 1e-9) * rng.uniform(1.0, 1.3, (51, 2))
    pts = pts.astype(np.float32)
    dirs = rng.normal(size=(512, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)

    mff = object.__new__(ref_map.MeshFeatureField)
    torch.nn.Module.__init__(mff)
    mff.device, mff.h_threshold, mff.K, mff.bound, mff.hash, mff.prob_model, mff.pred_normal, mff.clustering = "cpu", h_threshold, 8, 1, True, False, False, True
    mff.imported, mff.imported_type, mff.normal_net, mff.rescale = False, None, None, False
    mff.sdf_scale_factor, mff.sdf_offset, mff.uv_utilize_rate, mff.K_for_uv = 1.0, 0.0, 1.0, 5
    mff.encoder_f_out_dim = 16
    mff.encoder_z, mff.encoder_z_outdim = get_encoder("frequency", input_dim=1, multires=12)
    net = object.__new__(ref_cf.NeRFNetwork)
    torch.nn.Module.__init__(net)
    net.visual_mode, net.render_light_model, net.use_grad_normal, net.fc_weight, net.dir_degree = "RGB", False, False, 1.0, 4
    net.optimize_gamma, net.meshfea_field = False, mff
    tcnn = sys.modules["tinycudann"]
    torch.manual_seed(42)
    net.sigma_net = tcnn.Network(n_input_dims=mff.encoder_z_outdim + mff.encoder_f_out_dim, n_output_dims=16,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 1})
    net.encoder_dir = tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "SphericalHarmonics", "degree": 4})
    net.color_net = tcnn.Network(n_input_dims=net.encoder_dir.n_output_dims + 15, n_output_dims=3,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2})
    assert np.array_equal(net.sigma_net.net.weights.detach().numpy(), c["w_sigma"]) and np.array_equal(net.color_net.net.weights.detach().numpy(), c["w_color"])
    net.eval()
    mff.import_field(features, bounds=[0.5 * grid_gap * H, 0.5 * grid_gap * W], sample_tbn=np.eye(3, dtype=np.float32)[None], sample_tbn_ids=np.zeros((H, W), np.float32),
                     local_tbn=np.zeros((H, W, 9), np.float32), phi_embed=np.zeros((H, W, 8), np.float32))
    # MeshFeatureField.import_shape (:939-949) behind its MeshProjector(...) call
    assert mff.imported_type == "field"
    mff.meshprojector_imported = mp
    mff.sdf_scale_factor = mp.recommended_sdf_factor / mff.bounds[0]
    mff.imported, mff.imported_type = True, "shape"

    x, d = torch.from_numpy(pts), torch.from_numpy(dirs)
    out = dict(features=features, grid_gap=grid_gap, h_threshold=h_threshold, xyz=pts, dirs=dirs, weights_of="ref_python_curvedfield.npz",
               vertices_raw=vertices_raw, faces=faces.astype(np.int32), uvs_raw=uvs_raw, vertices=v32, uvs=mp.uvs.numpy(), vertex_normals=vn,
               recommended_sdf_factor=float(mp.recommended_sdf_factor), sdf_scale_factor=float(mff.sdf_scale_factor))
    recommended = float(mff.sdf_scale_factor)
    for k, (K, rate, factor, off) in enumerate(((5, 1.0, recommended, 0.0), (5, 0.8, recommended, 0.01), (3, 1.3, 2.0, 0.0))):
        mff.K_for_uv, mff.uv_utilize_rate, mff.sdf_scale_factor, mff.sdf_offset = K, rate, factor, off
        with torch.no_grad(), emulated_autocast():
            uvh, hm_u, normal, _ = mp.uvh(x, K=K, h_threshold=h_threshold, sdf_scale=factor / rate, sdf_offset=off)
            embed, nc, _, hm = mff(x)
            sigma, color, _ = net(x, d)
            dens = net.density(x)
            _, _, d1, f1 = mp.raytracer.trace(x, normal)
            _, _, d2, f2 = mp.raytracer.trace(x, -normal)
        face = torch.where(d1 < d2, f1, f2)  # (barycentric_mapping overwrites its -1 with 0: kept here as the tracer gives it)
        assert torch.equal(hm, hm_u) and torch.equal(dens["sigma"], sigma) and not torch.isnan(normal).any()
        key = f"S{k}"
        out.update({key + "_normal_raw": normal.float().numpy(), key + "_face": face.numpy().astype(np.int32)})
        out.update({key + "_K": K, key + "_rate": rate, key + "_sdf_factor": factor, key + "_offset": off, key + "_uvh": uvh.float().numpy(),
                    key + "_h_mask": hm.numpy(), key + "_normal": nc.float().numpy(), key + "_sigma": sigma.float().numpy(), key + "_color": color.half().numpy()})
        if k in (0, 2):
            out[key + "_embed"] = embed.float().numpy()
        print("ref_python_import_shape.npz:", key, "inside the mask", float(hm.float().mean()), "sigma max", float(sigma.max()),
              "|uv| max", float(uvh[:, :2].abs().max() * rate))
    np.savez_compressed(os.path.join(OUT, "ref_python_import_shape.npz"), **out)
    new = [os.path.join(r, n) for r, _, names in os.walk(REF) for n in names if os.lstat(os.path.join(r, n)).st_mtime >= started]
    assert not new, "files appeared under the reference tree:\n" + "\n".join(new[:20])


def _import_patch_goldens(lit):
    """The two import_patch fixtures: MeshFeatureField.import_patch (tools/map.py:929-937) and the `imported_type == 'patch'` branch of its
    forward (:676-692, :719-730) over MeshProjector.weighted_project / knn (:435-501) executed on the CPU under emulated_autocast, with
    NeRFNetwork.forward (and, static, density) behind it.  The patch: 12 x 12 points, grid gap 1/32, on z = 0.2 (x^2 - y^2), the one patch normal
    (0, 0, 1) at every point as NeRFNetwork.import_patch stores it (:485-486), seeded features (lit: phi_embed and frames that are not
    orthonormal).  import_patch's MeshProjector(...) call is answered by a projector made past its trimesh / open3d constructor from the
    arrays (mesh_vertices, vertex_normals, the search's members); frnn -> exact brute force.  512 points, h_threshold 0.0625: right above and
    below points, between four points, outside the rim, beyond the threshold, and seeded ones in the patch's box.  Values only."""
    import time

    import torch

    started = time.time()
    _install_map_imports()
    if lit:
        _stub("imageio")
        for name in ("nerf.sh_light_model", "nerf.network_curvedfield", "tools.shape_tools"):
            sys.modules.pop(name, None)
        for name, cls in (("sg_light_model", "SG_EnvmapMaterialNet"), ("envmap_light_model", "Envmap_EnvmapMaterialNet")):
            _stub("nerf." + name, **{cls: None})
        import nerf.sh_light_model as ref_sh
    else:
        for name, cls in (("sg_light_model", "SG_EnvmapMaterialNet"), ("sh_light_model", "SH_EnvmapMaterialNet"), ("envmap_light_model", "Envmap_EnvmapMaterialNet")):
            if "nerf." + name not in sys.modules:
                _stub("nerf." + name, **{cls: None})
    import nerf.network_curvedfield as ref_cf
    import tools.map as ref_map
    from tools.encoding import get_encoder

    c = np.load(os.path.join(OUT, "ref_python_curvedfield.npz"))
    S, gap, h_threshold, curve = 12, 1.0 / 32, 0.0625, 0.2
    rng = np.random.default_rng(171 if lit else 151)
    axis = (np.arange(S) - (S - 1) / 2) * gap
    gx, gy = np.meshgrid(axis, axis, indexing="ij")
    points = np.stack([gx, gy, curve * (gx * gx - gy * gy)], -1).reshape(-1, 3).astype(np.float32)
    V, half = S * S, (S - 1) / 2 * gap
    normal = np.array([0.0, 0.0, 1.0], np.float32)
    features = rng.uniform(-0.5, 0.5, (V, 16)).astype(np.float32)
    phi_embed = rng.uniform(-0.5, 0.5, (V, 8)).astype(np.float32)
    local_tbn = (np.eye(3, dtype=np.float32).reshape(9) + rng.normal(0, 0.35, (V, 9))).astype(np.float32)
    rows = []
    for b in range(512):
        i, t = int(rng.integers(0, V)), rng.uniform(-1.3, 1.3) * h_threshold
        kind = b % 5
        if kind == 0:
            q = points[i].astype(np.float64) + t * normal + rng.normal(0, 1e-3, 3) * gap
        elif kind == 1:
            xy = points[i, :2] + 0.5 * gap * np.where(points[i, :2] > 0, -1.0, 1.0)
            q = np.array([xy[0], xy[1], curve * (xy[0] ** 2 - xy[1] ** 2) + t])
        elif kind == 2:
            out_, along = half + rng.uniform(0.2, 3.0) * gap, rng.uniform(-half, half)
            xy = [(out_, along), (-out_, along), (along, out_), (along, -out_)][int(rng.integers(0, 4))]
            q = np.array([xy[0], xy[1], curve * (xy[0] ** 2 - xy[1] ** 2) + t])
        elif kind == 3:
            q = points[i].astype(np.float64) + np.sign(t) * rng.uniform(1.05, 1.6) * h_threshold * normal + rng.normal(0, 0.1, 3) * gap * np.array([1, 1, 0])
        else:
            xy = rng.uniform(-(half + 2 * gap), half + 2 * gap, 2)
            q = np.array([xy[0], xy[1], curve * (xy[0] ** 2 - xy[1] ** 2) + rng.uniform(-1.4, 1.4) * h_threshold])
        rows.append(q)
    pts = np.asarray(rows, np.float64).astype(np.float32)
    dirs = rng.normal(size=(512, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(np.float32)

    mff = object.__new__(ref_map.MeshFeatureField)
    torch.nn.Module.__init__(mff)
    mff.device, mff.h_threshold, mff.K, mff.bound, mff.hash, mff.prob_model, mff.pred_normal, mff.clustering = "cpu", h_threshold, 8, 1, True, False, lit, True
    mff.imported, mff.imported_type, mff.rescale = False, None, False  # (the constructor's values, :604-618)
    mff.sdf_scale_factor, mff.sdf_offset, mff.uv_utilize_rate, mff.K_for_uv = 1.0, 0.0, 1.0, 5
    mff.encoder_f_out_dim = 16
    mff.encoder_z, mff.encoder_z_outdim = get_encoder("frequency", input_dim=1, multires=12)
    mff.meshprojector = types.SimpleNamespace(mean_edge_length=gap)  # (import_patch hands it on; the 'patch' branch does not read it)
    mff.normal_net = None
    if lit:
        torch.manual_seed(11)
        mff.normal_net = ref_map.Factorized_Normal_Net(x_dim=mff.encoder_f_out_dim, z_dim=mff.encoder_z_outdim, lip=True, direct_pred_coor=False, bound_output=False)
        gen = torch.Generator().manual_seed(13)
        with torch.no_grad():
            for mlp in (mff.normal_net.phi_net, mff.normal_net.theta_net):
                for layer in mlp.layers:
                    layer.W.mul_(6.0)
                    layer.b.copy_(torch.randn(layer.b.shape, generator=gen) * 0.3)
                    layer.c.fill_(2.0)
    net = object.__new__(ref_cf.NeRFNetwork)
    torch.nn.Module.__init__(net)
    net.visual_mode, net.render_light_model, net.use_grad_normal, net.fc_weight, net.dir_degree = "RGB", lit, False, 1.0, 4
    net.optimize_gamma, net.meshfea_field = False, mff
    tcnn = sys.modules["tinycudann"]
    torch.manual_seed(42)
    net.sigma_net = tcnn.Network(n_input_dims=mff.encoder_z_outdim + mff.encoder_f_out_dim, n_output_dims=16,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 1})
    if lit:
        net.light_model, net.smooth_grad_weight = "SH", 1e-1
        net.use_coarse_normal, net.coarse_as_primary, net.no_visibility, net.shade_visibility, net.light_visual_mode = False, False, False, True, "Full"
        net.color_net = None
        net.light_net = ref_sh.SH_EnvmapMaterialNet(input_dim=15, sh_order=3, white_light=True, use_specular=True)
        with torch.no_grad():
            net.light_net.envSHs[1:] = torch.from_numpy(np.random.default_rng(91).normal(0, 1.5, (15, 1)).astype(np.float32))
    else:
        net.encoder_dir = tcnn.Encoding(n_input_dims=3, encoding_config={"otype": "SphericalHarmonics", "degree": 4})
        net.color_net = tcnn.Network(n_input_dims=net.encoder_dir.n_output_dims + 15, n_output_dims=3,
                                     network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2})
        assert np.array_equal(net.color_net.net.weights.detach().numpy(), c["w_color"])
    assert np.array_equal(net.sigma_net.net.weights.detach().numpy(), c["w_sigma"]), "the sigma net of ref_python_curvedfield.npz"
    net.eval()

    real_projector = ref_map.MeshProjector

    def projector_past_its_constructor(device, mesh, **kw):  # (the members knn() and weighted_project() read, :396-400)
        mp = object.__new__(real_projector)
        mp.mesh_vertices, mp.vertex_normals = torch.FloatTensor(mesh.vertices), torch.FloatTensor(mesh.normals)
        mp.grid, mp.radius, mp.max_K, mp.depth_threshold, mp.mean_edge_length = None, 100.0, len(mesh.vertices), 9.5, kw["mean_edge_length"]
        return mp

    # NeRFNetwork.import_patch (:484-487) on the arrays: the patch's points, its one normal at every point
    normals = np.zeros_like(points)
    normals[:] = normal
    mesh = types.SimpleNamespace(vertices=points, normals=normals)
    ref_map.MeshProjector = projector_past_its_constructor
    try:
        mff.import_patch(features=features, mesh=mesh, local_tbn=local_tbn, phi_embed=phi_embed if lit else None)
    finally:
        ref_map.MeshProjector = real_projector
    assert mff.imported and mff.imported_type == "patch"

    x, d = torch.from_numpy(pts), torch.from_numpy(dirs)
    name = "ref_python_import_patch_sh.npz" if lit else "ref_python_import_patch.npz"
    out = dict(features=features, points=points, normals=normal, grid_gap=gap, h_threshold=h_threshold, xyz=pts, dirs=dirs)
    with torch.no_grad(), emulated_autocast():
        embed, nc, nf, hm = mff(x)
        out.update(h_mask=hm.numpy(), embed=embed.float().numpy(), normal=nc.float().numpy())
        if not lit:
            sigma, color, _ = net(x, d)
            dens = net.density(x)
            assert torch.equal(dens["sigma"], sigma) and torch.equal(color.half().float(), color.float())
            out.update(sigma=sigma.float().numpy(), color=color.half().numpy(), weights_of="ref_python_curvedfield.npz")
        else:
            handed = {}
            net.light_net.register_forward_pre_hook(lambda m, a: handed.update(normal=a[1].detach().float().numpy().copy()))
            out.update(phi_embed=phi_embed, local_tbn=local_tbn, normal_fine=nf.float().numpy(), w_sigma=c["w_sigma"],
                       w_brdf=net.light_net.brdf_layer.net.weights.detach().numpy().copy(), env_shs=net.light_net.envSHs.detach().numpy().copy())
            for nm, mlp in (("phi", mff.normal_net.phi_net), ("theta", mff.normal_net.theta_net)):
                for i, layer in enumerate(mlp.layers):
                    out[f"{nm}_W{i}"], out[f"{nm}_b{i}"], out[f"{nm}_c{i}"] = layer.W.detach().numpy().copy(), layer.b.detach().numpy().copy(), float(layer.c)
            for fc in (1.0, 0.7):
                net.fc_weight = fc
                for visual in ("Full", "Specular", "Diffuse", "Albedo"):
                    net.light_visual_mode = visual
                    sigma, color, ret = net(x, d, is_gui_mode=False)
                    assert ret == {}
                    out[f"fc{fc}_color_{visual.lower()}"] = color.float().numpy()
                out["sigma"], out[f"fc{fc}_shading_normal"] = sigma.float().numpy(), handed["normal"]
    print(name + ":", "inside the mask", float(hm.float().mean()), "sigma max", float(sigma.max()), "rows that fail the direct-above test (sdf exactly 0)",
          int((embed[:, 16] == 0).sum()))
    np.savez_compressed(os.path.join(OUT, name), **out)
    new = [os.path.join(r, n) for r, _, names in os.walk(REF) for n in names if os.lstat(os.path.join(r, n)).st_mtime >= started]
    assert not new, "files appeared under the reference tree:\n" + "\n".join(new[:20])


def import_patch_goldens():
    """ref_python_import_patch.npz: the static light model (the sigma and colour nets of ref_python_curvedfield.npz); see _import_patch_goldens.
    Reads one fixture; writes this one file."""
    _import_patch_goldens(False)


def import_patch_sh_goldens():
    """ref_python_import_patch_sh.npz: the `pred_normal` part too (:687-692: the weighted phi_embed and local_tbn, ONE rotation), NeRFNetwork.forward
    in eval with the real SH_EnvmapMaterialNet, fc_weight 1.0 and 0.7, the four light_visual_modes; the normal net and the lighting of
    ref_python_import_field_sh.npz's recipe.  See _import_patch_goldens.  Reads one fixture (the sigma net's weights, as a check); writes this one."""
    _import_patch_goldens(True)


def import_shape_sh_goldens():
    """ref_python_import_shape_sh.npz: the `pred_normal` part of the `imported_type == 'shape'` branch of MeshFeatureField.forward
    (tools/map.py:693-707, :722-730) executed on the CPU under emulated_autocast, with network_curvedfield.NeRFNetwork.forward behind it in eval
    with the real SH_EnvmapMaterialNet.  It joins import_shape_goldens (the mesh, the UVs, the points and the directions are READ from
    ref_python_import_shape.npz; the MeshProjector is made past its constructor as there, frnn -> exact brute force, tracer -> the oracle) with
    import_field_sh_goldens (the real six-argument import_field; the 24 x 20 maps, the P = 5 patch frames, the normal net, the sigma and BRDF
    nets and the lighting are its recipe, re-made from its seeds and asserted equal to ref_python_import_field_sh.npz, where they are READ from
    by the tests).  mp.tbn is the reference's OWN calculate_tbn (:119-138) over a namespace with vertices, faces and face_normals of the
    normalised mesh, and mp.uvs.  The three states of ref_python_import_shape.npz, fc_weight 1.0 and 0.7, the four light_visual_modes.
    Recorded, outputs only: uvh, mask, face, the sampled id, the three sampled frames, phi, the 28 columns of the embedding the normal net
    reads (16 features, the first 12 height bands), normal_fine, the shading normal, sigma and the colours; `tbn` [F,3,3]; per state the count of rows within the nearest read's margin of a texel edge."""
    import time
    import types

    import torch

    started = time.time()
    _install_map_imports()
    _stub("imageio")
    for name in ("nerf.sh_light_model", "nerf.network_curvedfield", "tools.shape_tools"):
        sys.modules.pop(name, None)
    for name, cls in (("sg_light_model", "SG_EnvmapMaterialNet"), ("envmap_light_model", "Envmap_EnvmapMaterialNet")):
        _stub("nerf." + name, **{cls: None})
    import nerf.network_curvedfield as ref_cf
    import nerf.sh_light_model as ref_sh
    import tools.map as ref_map
    from RayTracer import RayTracer as RefRayTracer
    from tools.encoding import get_encoder

    c = np.load(os.path.join(OUT, "ref_python_curvedfield.npz"))
    gs = np.load(os.path.join(OUT, "ref_python_import_shape.npz"))
    gl = np.load(os.path.join(OUT, "ref_python_import_field_sh.npz"))
    H, W, P, grid_gap, h_threshold = 24, 20, 5, float(gl["grid_gap"]), float(gl["h_threshold"])
    assert h_threshold == float(gs["h_threshold"]) and grid_gap == float(gs["grid_gap"])
    # the maps: import_field_sh_goldens' recipe, equal to what that fixture stores
    rng = np.random.default_rng(171)
    features = rng.uniform(-0.5, 0.5, (H, W, 16)).astype(np.float32)
    phi_embed = rng.uniform(-0.5, 0.5, (H, W, 8)).astype(np.float32)
    local_tbn = (np.eye(3, dtype=np.float32).reshape(9) + rng.normal(0, 0.35, (H, W, 9))).astype(np.float32)
    sample_tbn = (np.eye(3, dtype=np.float32) + rng.normal(0, 0.3, (P, 3, 3))).astype(np.float32)
    sample_tbn_ids = rng.integers(0, P, (H, W)).astype(np.float32)
    for name, a in (("features", features), ("phi_embed", phi_embed), ("local_tbn", local_tbn), ("sample_tbn", sample_tbn), ("sample_tbn_ids", sample_tbn_ids)):
        assert np.array_equal(a, gl[name]), name

    # the mesh: import_shape_goldens' construction on the arrays of its fixture
    vertices_raw, faces, uvs_raw = gs["vertices_raw"], gs["faces"].astype(np.int64), gs["uvs_raw"]
    vertices = vertices_raw.copy()
    vertices -= np.mean(vertices, axis=0)
    vertices /= (np.absolute(vertices).max() + 1e-5)
    vertices /= 1.2
    v32 = vertices.astype(np.float32)
    assert np.array_equal(v32, gs["vertices"])
    mp = object.__new__(ref_map.MeshProjector)
    uvs = torch.FloatTensor(uvs_raw)
    mp.uvs = (uvs - uvs.min()) / (uvs.max() - uvs.min()) * 2 - 1.  # :361
    assert np.array_equal(mp.uvs.numpy(), gs["uvs"])
    e1, e2 = vertices[faces[:, 1]] - vertices[faces[:, 0]], vertices[faces[:, 2]] - vertices[faces[:, 0]]
    face_normals = np.cross(e1, e2)
    face_normals /= np.linalg.norm(face_normals, axis=-1, keepdims=True)  # (trimesh's face_normals)
    uv_np = mp.uvs.cpu().numpy()
    uv_edges = uv_np[faces][:, 1:] - uv_np[faces][:, :1]
    det = np.abs(np.linalg.det(uv_edges.astype(np.float64)))
    assert np.linalg.matrix_rank(uv_edges).min() == 2, "every UV edge matrix has rank 2"
    tbn = ref_map.calculate_tbn(types.SimpleNamespace(vertices=vertices, faces=faces, face_normals=face_normals), uv_np)  # :366
    assert np.isfinite(tbn).all() and len(np.unique(tbn.round(6), axis=0)) == len(faces)
    assert np.abs(np.einsum("fab,fcb->fac", tbn, tbn) - np.eye(3)).max() < 1e-6, "orthonormal frames"
    print("ref_python_import_shape_sh.npz:", len(faces), "faces, smallest |det| of a UV edge matrix", float(det.min()))
    mp.tbn = torch.from_numpy(tbn).float()
    edges_unique = np.unique(np.sort(faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1), axis=0)
    edges = vertices[edges_unique]
    mp.mean_edge_length = np.linalg.norm(edges[:, 0] - edges[:, 1], axis=-1).mean()
    edges_uv = uv_np[edges_unique]
    mp.recommended_sdf_factor = mp.mean_edge_length / np.linalg.norm(edges_uv[:, 0] - edges_uv[:, 1], axis=-1).mean()
    assert abs(float(mp.recommended_sdf_factor) / float(gs["recommended_sdf_factor"]) - 1) < 1e-12
    mp.mesh_vertices, mp.vertex_normals = torch.FloatTensor(vertices), torch.from_numpy(gs["vertex_normals"])
    mp.grid, mp.radius, mp.max_K, mp.depth_threshold = None, 100.0, v32.shape[0], 9.5
    mp.raytracer = RefRayTracer(v32, faces.astype(np.uint32))
    mp.faces = torch.from_numpy(faces).long()

    # the lit field: import_field_sh_goldens' construction, equal to what that fixture stores
    mff = object.__new__(ref_map.MeshFeatureField)
    torch.nn.Module.__init__(mff)
    mff.device, mff.h_threshold, mff.K, mff.bound, mff.hash, mff.prob_model, mff.pred_normal, mff.clustering = "cpu", h_threshold, 8, 1, True, False, True, True
    mff.imported, mff.imported_type, mff.rescale = False, None, False
    mff.sdf_scale_factor, mff.sdf_offset, mff.uv_utilize_rate, mff.K_for_uv = 1.0, 0.0, 1.0, 5
    mff.encoder_f_out_dim = 16
    mff.encoder_z, mff.encoder_z_outdim = get_encoder("frequency", input_dim=1, multires=12)
    torch.manual_seed(11)
    mff.normal_net = ref_map.Factorized_Normal_Net(x_dim=mff.encoder_f_out_dim, z_dim=mff.encoder_z_outdim, lip=True, direct_pred_coor=False, bound_output=False)
    gen = torch.Generator().manual_seed(13)
    with torch.no_grad():
        for mlp in (mff.normal_net.phi_net, mff.normal_net.theta_net):
            for layer in mlp.layers:
                layer.W.mul_(6.0)
                layer.b.copy_(torch.randn(layer.b.shape, generator=gen) * 0.3)
                layer.c.fill_(2.0)
    for name, mlp in (("phi", mff.normal_net.phi_net), ("theta", mff.normal_net.theta_net)):
        for i, layer in enumerate(mlp.layers):
            assert np.array_equal(layer.W.detach().numpy(), gl[f"{name}_W{i}"]) and np.array_equal(layer.b.detach().numpy(), gl[f"{name}_b{i}"])
    net = object.__new__(ref_cf.NeRFNetwork)
    torch.nn.Module.__init__(net)
    net.visual_mode, net.render_light_model, net.use_grad_normal, net.fc_weight, net.dir_degree = "RGB", True, False, 1.0, 4
    net.optimize_gamma, net.meshfea_field, net.light_model, net.smooth_grad_weight = False, mff, "SH", 1e-1
    net.use_coarse_normal, net.coarse_as_primary, net.no_visibility, net.shade_visibility, net.light_visual_mode = False, False, False, True, "Full"
    tcnn = sys.modules["tinycudann"]
    torch.manual_seed(42)
    net.sigma_net = tcnn.Network(n_input_dims=mff.encoder_z_outdim + mff.encoder_f_out_dim, n_output_dims=16,
                                 network_config={"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 32, "n_hidden_layers": 1})
    assert np.array_equal(net.sigma_net.net.weights.detach().numpy(), c["w_sigma"])
    net.color_net = None
    net.light_net = ref_sh.SH_EnvmapMaterialNet(input_dim=15, sh_order=3, white_light=True, use_specular=True)
    with torch.no_grad():
        net.light_net.envSHs[1:] = torch.from_numpy(np.random.default_rng(91).normal(0, 1.5, (15, 1)).astype(np.float32))
    assert np.array_equal(net.light_net.brdf_layer.net.weights.detach().numpy(), gl["w_brdf"]) and np.array_equal(net.light_net.envSHs.detach().numpy(), gl["env_shs"])
    handed, sampled = {}, []
    net.light_net.register_forward_pre_hook(lambda m, a: handed.update(normal=a[1].detach().float().numpy().copy()))
    real_grid_sample = torch.nn.functional.grid_sample

    def recording_grid_sample(*a, **k):
        r = real_grid_sample(*a, **k)
        sampled.append((k.get("mode", "bilinear"), r))
        return r

    mff.import_field(features, bounds=[0.5 * grid_gap * H, 0.5 * grid_gap * W], sample_tbn=sample_tbn, sample_tbn_ids=sample_tbn_ids, local_tbn=local_tbn,
                     phi_embed=phi_embed)
    # MeshFeatureField.import_shape (:939-949) behind its MeshProjector(...) call
    assert mff.imported_type == "field" and mff.rescale
    mff.meshprojector_imported = mp
    mff.sdf_scale_factor = mp.recommended_sdf_factor / mff.bounds[0]
    mff.imported, mff.imported_type = True, "shape"
    assert abs(float(mff.sdf_scale_factor) / float(gs["sdf_scale_factor"]) - 1) < 1e-12

    x, d = torch.from_numpy(gs["xyz"]), torch.from_numpy(gs["dirs"])
    out = dict(mesh_and_points_of="ref_python_import_shape.npz", maps_and_weights_of="ref_python_import_field_sh.npz", tbn=tbn.astype(np.float32))
    net.eval()
    torch.nn.functional.grid_sample = recording_grid_sample
    try:
        for k in range(3):
            key = f"S{k}"
            K, rate, factor, off = int(gs[key + "_K"]), float(gs[key + "_rate"]), float(gs[key + "_sdf_factor"]), float(gs[key + "_offset"])
            mff.K_for_uv, mff.uv_utilize_rate, mff.sdf_scale_factor, mff.sdf_offset = K, rate, factor, off
            with torch.no_grad(), emulated_autocast():
                uvh, hm_u, normal, new_tbn = mp.uvh(x, K=K, h_threshold=h_threshold, sdf_scale=factor / rate, sdf_offset=off)
                del sampled[:]
                embed, nc, nf, hm = mff(x)
                assert [m for m, _ in sampled] == ["bilinear", "nearest", "nearest", "bilinear"]  # features, ids, local_tbn, phi_embed (:697-706)
                ids = sampled[1][1].squeeze().long()
                s_local = sampled[2][1].squeeze().permute(1, 0).reshape(-1, 3, 3)
                s_phi = sampled[3][1].squeeze().permute(1, 0)
                _, _, d1, f1 = mp.raytracer.trace(x, normal)
                _, _, d2, f2 = mp.raytracer.trace(x, -normal)
            face = torch.where(d1 < d2, f1, f2)  # (-1 kept as the tracer gives it; new_tbn is tbn[max(face, 0)])
            assert torch.equal(hm, hm_u) and np.array_equal(uvh.numpy(), gs[key + "_uvh"]) and np.array_equal(hm.numpy(), gs[key + "_h_mask"])
            assert np.array_equal(face.numpy().astype(np.int32), gs[key + "_face"]) and torch.equal(new_tbn, mp.tbn[face.clamp(min=0)])
            # rows whose ix or iy lies within the nearest read's margin of a half-integer: the u, v bar of 2e-6 times (size - 1) / 2
            p_sur = uvh[:, :2].double().numpy() * rate
            near = np.zeros(len(p_sur), bool)
            for axis, size in ((0, H), (1, W)):
                i = (p_sur[:, axis] + 1) / 2 * (size - 1)
                near |= np.abs(i - np.floor(i) - 0.5) <= 2e-6 * (size - 1) / 2
            assert near.sum() <= 0.01 * len(near), (key, int(near.sum()))
            out.update({key + "_uvh": uvh.float().numpy(), key + "_h_mask": hm.numpy(), key + "_face": face.numpy().astype(np.int32),
                        key + "_id": ids.numpy().astype(np.int32), key + "_local_tbn": s_local.numpy(), key + "_sample_tbn_inv": mff.sample_tbn_inv_imported[ids].numpy(),
                        key + "_new_tbn": new_tbn.numpy(), key + "_phi": s_phi.numpy(), key + "_embed28": embed.float().numpy()[:, :28], key + "_normal": nc.float().numpy(), key + "_normal_fine": nf.float().numpy(),
                        key + "_near_texel_edge": int(near.sum())})
            for fc in (1.0, 0.7):
                net.fc_weight = fc
                with torch.no_grad(), emulated_autocast():
                    for visual in ("Full", "Specular", "Diffuse", "Albedo"):
                        net.light_visual_mode = visual
                        sigma, color, ret = net(x, d, is_gui_mode=False)
                        assert ret == {}
                        out[f"{key}_fc{fc}_color_{visual.lower()}"] = color.half().numpy()
                out[key + "_sigma"], out[f"{key}_fc{fc}_shading_normal"] = sigma.float().numpy(), handed["normal"]
            print("ref_python_import_shape_sh.npz:", key, "inside the mask", float(hm.float().mean()), "sigma max", float(sigma.max()), "rows near a texel edge",
                  int(near.sum()), "fine normal away from the face normal by (median)",
                  float(np.median(np.abs(nf.numpy() - new_tbn.numpy()[:, 2]).max(-1)[hm.numpy()])))
    finally:
        torch.nn.functional.grid_sample = real_grid_sample
    np.savez_compressed(os.path.join(OUT, "ref_python_import_shape_sh.npz"), **out)
    new = [os.path.join(r, n) for r, _, names in os.walk(REF) for n in names if os.lstat(os.path.join(r, n)).st_mtime >= started]
    assert not new, "files appeared under the reference tree:\n" + "\n".join(new[:20])


# the two cases of ref_python_synthesis.npz: patch count, patch side, channels (features + phi_embed + local_tbn), max_patch_res, mirrors, output side,
# patch_length, and the seed of both the inputs and the reference's random streams
SYNTHESIS_CASES = {
    "A": dict(P=40, S=12, match_dim=16, phi_dim=8, max_patch_res=4, mirrors=False, output=30, patch_length=1.0, seed=2),
    "B": dict(P=24, S=13, match_dim=16, phi_dim=8, max_patch_res=4, mirrors=True, output=30, patch_length=7.5, seed=10),
}


def unhash_goldens():
    """ref_python_unhash.npz: the `imported_type == 'unhash'` branch of MeshFeatureField.forward (tools/map.py:708-714, :719-720) executed on the
    CPU -- knn() with its defaults over the field's own mesh, query_tbn (dead work there, but it runs), barycentric_mapping over the fine mesh
    (:503-528), the three-row interpolation and FreqEncoder(height).  The coarse mesh is `_small_star_flower`, the fine one ONE round of
    ngp_harness/subdivide.py's subdivide_midpoint of it (loaded by path: the drop-in packages are not importable here), rounded to fp32; both
    MeshProjectors are made past their trimesh / open3d constructors from the arrays; frnn -> exact brute force (its neighbour lists are kept), tracer -> the oracle.
    Per-vertex features: a seeded table of multiples of 2^-10.  512 points at h_threshold 0.0625: most within +-0.055 of the surface, 8 % between 0.07 and 0.12 from it
    (outside the mask), 3 % thirty away (both traces miss).  Three cases: U0 the state unhash() leaves (:853-857), U1 sdf_scale_factor 2.5 and
    sdf_offset 0.01, U2 the real import_unhash_vertices (:862-873) on a file written to a temporary directory (another table, sdf_factor 0.8; its
    BvhMeshProjector(...) call is answered by the fine projector).  Values only."""
    import importlib.util
    import tempfile
    import time

    import torch

    started = time.time()
    _install_map_imports()
    for name, cls in (("sg_light_model", "SG_EnvmapMaterialNet"), ("sh_light_model", "SH_EnvmapMaterialNet"), ("envmap_light_model", "Envmap_EnvmapMaterialNet")):
        if "nerf." + name not in sys.modules:
            _stub("nerf." + name, **{cls: None})
    import tools.map as ref_map
    from RayTracer import RayTracer as RefRayTracer
    from tools.encoding import get_encoder

    spec = importlib.util.spec_from_file_location("_subdivide", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "nerf-texture_amd", "ngp_harness",
                                                                            "subdivide.py"))
    subdivide = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(subdivide)

    h_threshold = 0.0625
    v, f, vn, tbn = _small_star_flower()
    faces = f.astype(np.int64)
    fine_v64, fine_faces = subdivide.subdivide_midpoint(v, faces)
    fine_v = fine_v64.astype(np.float32)
    assert len(fine_v) > len(v) and len(fine_faces) == 4 * len(faces)

    def area_normals(vertices, tris):
        v8 = vertices.astype(np.float64)
        fn = np.cross(v8[tris[:, 1]] - v8[tris[:, 0]], v8[tris[:, 2]] - v8[tris[:, 0]])
        out = np.zeros_like(v8)
        for k in range(3):
            np.add.at(out, tris[:, k], fn)
        return (out / (np.linalg.norm(out, axis=-1, keepdims=True) + 1e-12)).astype(np.float32)

    def projector(vertices, tris, normals, frames=None):  # (the members knn(), query_tbn() and barycentric_mapping() read)
        mp = object.__new__(ref_map.MeshProjector)
        mp.mesh_vertices, mp.vertex_normals = torch.from_numpy(vertices), torch.from_numpy(normals)
        mp.tbn = None if frames is None else torch.from_numpy(frames)
        mp.grid, mp.radius, mp.max_K, mp.depth_threshold = None, 100.0, vertices.shape[0], 9.5
        mp.raytracer = RefRayTracer(vertices, tris.astype(np.uint32))
        mp.faces = torch.from_numpy(tris).long()
        return mp

    coarse, fine = projector(v, faces, vn, tbn), projector(fine_v, fine_faces, area_normals(fine_v, fine_faces))

    rng = np.random.default_rng(181)
    # (multiples of 2^-10: ten bits a value, so that the compressed fixture stays a third of the size raw fp32 noise would have)
    features = (np.round(rng.uniform(-0.5, 0.5, (len(fine_v), 16)) * 1024) / 1024).astype(np.float32)
    features_u2 = (np.round(rng.uniform(-0.5, 0.5, (len(fine_v), 16)) * 1024) / 1024).astype(np.float32)
    N = 512
    pick, bary = rng.integers(0, len(faces), N), rng.dirichlet([1, 1, 1], N)
    on = (v[faces[pick]].astype(np.float64) * bary[..., None]).sum(1)
    nn = (vn[faces[pick]].astype(np.float64) * bary[..., None]).sum(1)
    nn /= np.linalg.norm(nn, axis=-1, keepdims=True)
    offset = rng.uniform(-0.055, 0.055, N)
    rows = rng.permutation(N)
    beyond, away = rows[:41], rows[41:56]
    offset[beyond] = rng.uniform(0.07, 0.12, len(beyond)) * rng.choice([-1.0, 1.0], len(beyond))
    pts = on + nn * offset[:, None]
    far = rng.normal(size=(len(away), 3))
    pts[away] = far / np.linalg.norm(far, axis=-1, keepdims=True) * 30.0
    pts = pts.astype(np.float32)

    mff = object.__new__(ref_map.MeshFeatureField)
    torch.nn.Module.__init__(mff)
    mff.device, mff.h_threshold, mff.K, mff.bound, mff.hash, mff.prob_model, mff.pred_normal, mff.clustering = "cpu", h_threshold, 8, 1, True, False, False, True
    mff.imported, mff.imported_type, mff.normal_net, mff.rescale = False, None, None, False
    mff.sdf_scale_factor, mff.sdf_offset, mff.uv_utilize_rate, mff.K_for_uv = 1.0, 0.0, 1.0, 5
    mff.encoder_f_out_dim = 16
    mff.encoder_z, mff.encoder_z_outdim = get_encoder("frequency", input_dim=1, multires=12)
    mff.meshprojector, mff.meshprojector_imported = coarse, None

    x = torch.from_numpy(pts)
    out = dict(vertices=v, faces=faces.astype(np.int32), vertex_normals=vn, fine_vertices=fine_v, fine_faces=fine_faces.astype(np.int32), xyz=pts,
               h_threshold=h_threshold, features=features, U2_features=features_u2)

    def record(key):
        with torch.no_grad(), emulated_autocast():
            embed, nc, nf, hm = mff(x)
            normal, _, indices, dis = coarse.knn(x)
            _, b, sdf, hm_b = fine.barycentric_mapping(x, normal=normal, h_threshold=h_threshold, sdf_scale=mff.sdf_scale_factor, sdf_offset=mff.sdf_offset)
            _, _, d1, f1 = fine.raytracer.trace(x, normal)
            _, _, d2, f2 = fine.raytracer.trace(x, -normal)
        face = torch.where(d1 < d2, f1, f2)  # (barycentric_mapping overwrites its -1 with 0: kept here as the tracer gives it)
        assert nf is None and torch.equal(hm, hm_b) and torch.equal(embed[:, 16], sdf[:, 0]) and embed.dtype == torch.float32
        out.update({key + "_sdf_factor": float(mff.sdf_scale_factor), key + "_offset": float(mff.sdf_offset), key + "_embed": embed.numpy(), key + "_normal": nc.numpy(),
                    key + "_normal_raw": normal.numpy(), key + "_h_mask": hm.numpy(), key + "_sdf": sdf[:, 0].numpy(), key + "_face": face.numpy().astype(np.int32),
                    key + "_bary": b.numpy()})
        # the neighbours knn() found, the same for every case (the pole vertices are duplicated: which copies a search returns is its own business)
        out.update(knn_idx=indices.numpy().astype(np.int32), knn_dis=dis[:, :8].numpy())
        print("ref_python_unhash.npz:", key, "inside the mask", float(hm.float().mean()), "both traces miss", float((face < 0).float().mean()))

    # U0, U1: the state unhash() leaves (:853-857) behind its subdivision and its encoder call
    mff.meshprojector_imported = fine
    mff.features_imported = torch.nn.Parameter(torch.from_numpy(features))
    mff.imported, mff.imported_type = True, "unhash"
    record("U0")
    mff.sdf_scale_factor, mff.sdf_offset = 2.5, 0.01
    record("U1")
    # U2: import_unhash_vertices itself
    mff.sdf_offset, mff.meshprojector_imported, mff.features_imported, mff.imported_type = 0.0, None, None, None
    _stub("tools.map_bvh", BvhMeshProjector=lambda **kw: fine)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "unhash.npz")
        np.savez(path, mesh=np.array(types.SimpleNamespace(vertices=fine_v, faces=fine_faces), dtype=object), features=features_u2, sdf_factor=0.8)
        mff.import_unhash_vertices(path)
    sys.modules.pop("tools.map_bvh", None)
    assert mff.imported_type == "unhash" and mff.sdf_scale_factor == 0.8 and mff.meshprojector_imported is fine
    record("U2")
    np.savez_compressed(os.path.join(OUT, "ref_python_unhash.npz"), **out)
    new = [os.path.join(r, n) for r, _, names in os.walk(REF) for n in names if os.lstat(os.path.join(r, n)).st_mtime >= started]
    assert not new, "files appeared under the reference tree:\n" + "\n".join(new[:20])


def synthesis_inputs(case):
    """The random inputs of one synthesis case: fp32 values, as an export holds them.  The patch values are multiples of 1 / 256 in [-0.5, 0.5): eight
    random bits a value keep the compressed fixture small."""
    rng = np.random.default_rng(1000 + case["seed"])
    P, S, C = case["P"], case["S"], case["match_dim"] + case["phi_dim"] + 9
    patches = (rng.integers(-128, 128, (P, S, S, C)) / 256).astype(np.float32)
    sample_tbn = (np.eye(3, dtype=np.float32).reshape(9) + rng.normal(0, 0.3, (P, 9))).astype(np.float32)
    picked_vertices = rng.uniform(-1, 1, (P, 3)).astype(np.float32)
    return patches, sample_tbn, picked_vertices


def run_reference_synthesis(case, patches=None, sample_tbn=None, picked_vertices=None):
    """One run of the reference's patchBasedTextureSynthesis (patch_matching_and_quilting.py) with the options of its __main__ -- mode 'Cut',
    coarse_KDtree, rotate=False, strict_match, picked_vertices given -- on the CPU, and the closing lines of __main__ (:485-511) behind it.
    skimage is absent: block_reduce is stubbed as what its defaults compute, the zero-padded block sum.  visualize, saveParams, the directory check
    and the PCA of the snapshots do nothing.  `random` and `np.random` are seeded; np.random.choice is wrapped by a recorder that calls through."""
    import random

    os.environ.setdefault("MPLBACKEND", "Agg")

    def block_reduce(a, block_size):
        a = np.asarray(a)
        pad = [(0, (-s) % b) for s, b in zip(a.shape, block_size)]
        a = np.pad(a, pad)
        shape = []
        for s, b in zip(a.shape, block_size):
            shape += [s // b, b]
        return a.reshape(shape).sum(axis=tuple(range(1, 2 * a.ndim, 2)))

    _stub("skimage")
    _stub("skimage.measure", block_reduce=block_reduce)
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import patch_matching_and_quilting as ref

    ref.get_transform = lambda data, dim: None
    if patches is None:
        patches, sample_tbn, picked_vertices = synthesis_inputs(case)
    S, match_dim = case["S"], case["match_dim"]
    patch_size = int(S / 4)
    if (S - patch_size) % 2 == 1:
        patch_size -= 1
    overlap = int((S - patch_size) / 2)
    record = dict(k=[], survivors=[], distances=[], probabilities=[], chosen=[], draws=[])

    class Recorded(ref.patchBasedTextureSynthesis):
        def checkIfDirectoryExists(self):
            pass

        def saveParams(self):
            pass

        def visualize(self):
            pass

        def initKDtrees(self):
            self.max_patch_res = case["max_patch_res"]
            return super().initKDtrees()

        def resolveNext(self):
            self.ks = []
            super().resolveNext()
            record["k"].append(self.ks[-1])

        def findMostSimilarPatches(self, top, left, coord, in_k=16):
            self.ks.append(in_k)
            return super().findMostSimilarPatches(top, left, coord, in_k=in_k)

        def distances2probability(self, distances, truncation, attenuation):
            record["distances"].append(np.array(distances, dtype=np.float64))
            p = super().distances2probability(distances, truncation, attenuation)
            record["probabilities"].append(np.array(p, dtype=np.float64))
            return p

    real_choice = np.random.choice

    def recording_choice(a, size=None, replace=True, p=None):
        peek = np.random.RandomState()
        peek.set_state(np.random.get_state())
        record["draws"].append(float(peek.random_sample()))
        out = real_choice(a, size, replace, p)
        record["survivors"].append(np.array(a, dtype=np.int64))
        record["chosen"].append(int(out[0]))
        return out

    random.seed(case["seed"])
    np.random.seed(case["seed"])
    np.random.choice = recording_choice
    try:
        mirrors = case["mirrors"]
        pbts = Recorded(patches.astype(np.float64), "unused/", [case["output"], case["output"]], patch_size, overlap, in_windowStep=5, in_mirror_hor=mirrors,
                        in_mirror_vert=mirrors, rotate=False, in_shapshots=True, picked_vertices=picked_vertices.astype(np.float64), patch_length=case["patch_length"],
                        coarse_KDtree=True, sample_tbn=sample_tbn.astype(np.float64), match_dim=match_dim, strict_match=True, mode="Cut")
        canvas, canvas_id = pbts.resolveAll()
    finally:
        np.random.choice = real_choice
    # __main__ :485-511
    canvas_id = np.array(canvas_id, dtype=np.int32)
    raw_id = canvas_id.copy()
    total_id = np.sort(np.unique(canvas_id.reshape([-1])))
    index = {total_id[i]: i for i in range(total_id.shape[0])}
    for i in range(canvas_id.shape[0]):
        for j in range(canvas_id.shape[1]):
            canvas_id[i, j] = index[canvas_id[i, j]]
    return dict(record=record, canvas=pbts.canvas, canvas_id=raw_id, id_map=pbts.idMap.astype(np.int32), total_id=total_id.astype(np.int32),
                sample_tbn=pbts.example_tbn[total_id], sample_tbn_ids=canvas_id, examples=pbts.examplePatches.shape[0], block=pbts.block_size,
                patch_size=patch_size, overlap_size=overlap, inputs=(patches, sample_tbn, picked_vertices))


def synthesis_goldens():
    """ref_python_synthesis.npz: the reference's own texture synthesis class run on the two cases of SYNTHESIS_CASES (see run_reference_synthesis).
    Stored per case: the inputs, the first patch, the draws the seeded stream gave, per cell k, the survivors, their distances, the probabilities
    and the chosen id (ragged lists, flattened with the survivor counts beside them), the final canvas (float64), canvas_id and idMap, and the
    closing arrays.  Reads nothing; writes this one file."""
    import time

    started = time.time()
    out = {}
    for name, case in SYNTHESIS_CASES.items():
        r = run_reference_synthesis(case)
        rec = r["record"]
        patches, sample_tbn, picked_vertices = r["inputs"]
        counts = np.array([len(s) for s in rec["survivors"]], dtype=np.int32)
        cells = r["id_map"].size
        assert len(rec["chosen"]) == cells - 1 == len(rec["draws"]) == len(rec["k"]) and r["canvas_id"].min() >= 0
        assert np.array_equal(np.array(rec["chosen"]), r["id_map"].reshape(-1)[1:])
        pre = name + "_"
        out.update({pre + "patches": patches, pre + "sample_tbn_in": sample_tbn, pre + "picked_vertices": picked_vertices,
                    pre + "options": np.array([case["match_dim"], case["phi_dim"], case["max_patch_res"], int(case["mirrors"]), case["output"], case["seed"],
                                               r["patch_size"], r["overlap_size"], r["block"], r["examples"]], dtype=np.int64),
                    pre + "patch_length": np.float64(case["patch_length"]), pre + "first_patch": np.int32(r["id_map"][0, 0]),
                    pre + "draws": np.array(rec["draws"]), pre + "k": np.array(rec["k"], dtype=np.int32), pre + "survivor_counts": counts,
                    pre + "survivors": np.concatenate(rec["survivors"]).astype(np.int32), pre + "distances": np.concatenate(rec["distances"]),
                    pre + "probabilities": np.concatenate(rec["probabilities"]), pre + "chosen": np.array(rec["chosen"], dtype=np.int32),
                    pre + "canvas": r["canvas"], pre + "canvas_id": r["canvas_id"], pre + "id_map": r["id_map"], pre + "total_id": r["total_id"],
                    pre + "sample_tbn": r["sample_tbn"], pre + "sample_tbn_ids": r["sample_tbn_ids"].astype(np.int32)})
        print("ref_python_synthesis.npz: case", name, "canvas", r["canvas"].shape, "examples", r["examples"], "k per cell", rec["k"], "survivors per cell",
              counts.tolist())
    np.savez_compressed(os.path.join(OUT, "ref_python_synthesis.npz"), **out)
    new = [os.path.join(r, n) for r, _, names in os.walk(REF) for n in names if os.lstat(os.path.join(r, n)).st_mtime >= started]
    assert not new, "files appeared under the reference tree:\n" + "\n".join(new[:20])


if __name__ == "__main__":
    main()
