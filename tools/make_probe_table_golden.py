#!/usr/bin/env python3
"""Generate tests/golden/ref_python_probe_tables.npz FROM THE REFERENCE ITSELF: nerf/sh_light_model.py imported at run time with the stand-ins of
tools/make_golden.py and run on the CPU -- load_envmap_with_visibility's branch without a file (:653-665): the 8 x 8 probe grid,
rotate_coeff_by_normal on the clamped-cosine lobe, fit_product_of_SHs (:692-709).  Needs the reference checkout (NERFTEX_REFERENCE); it never runs
where the GPU tests run.  No reference text is stored in this repository.

fit_product_of_SHs draws its points with torch.rand (twice per step: phi, then theta) and has its sizes as literals.  Both are dealt with from
outside: `torch.rand` is replaced, while the reference's function runs, by a replayer of a RECORDED stream (which hands out the recorded row
whatever size is asked for), and the name `range` is bound in the reference module's namespace to cut the number of rounds.  Every line of the
loop that runs is the reference's.

  geometry     probes [64, 3], lobes [64, 9] = rotate_coeff_by_normal(2, probes, lobe); the same for four extra normals: +z, -z, one with
               n_z = 0.9995 (past the 0.999 special case), one unnormalised
  replay case  probes 9, 27, 63 (63: the duplicated pole row), 40 rounds x 96 points, a seeded non-white lighting [16, 3]: the points, the reference's
               fp32 result, the same loop in float64, their gap g_replay, and the same loop WITH zero_grad (what the reference does NOT do)
  g_full       the gap between the fp32 and the float64 loop on one replayed 800 x 1024 stream, two probes
  seed case    probes 9, 27, 36, 63 at the reference's 800 x 1024 under 8 torch seeds each: per-coefficient mean and standard deviation
               (ddof = 1), sigma_max

Asserted while generating (what the restatements in ngp_harness/light.py rest on):
  * a restated loop WITHOUT zero_grad on the replayed points equals fit_product_of_SHs bit for bit, at 40 x 96 (patched) and at 800 x 1024
    (untouched function under torch.manual_seed, stream recorded by re-seeding); WITH zero_grad it misses by more than 100 x g_replay
  * the result is not the minimiser: its DC coefficient is far from the L2 projection of the product
  * g_replay < 5e-6 and g_full < 2e-5: on the same points the trajectory is stable
  * the rotated lobe, evaluated at its own probe direction, has the unrotated lobe's value at +z, for all 64 probes
  * column 7 of the grid repeats column 0 and the last row is eight copies of the pole (0, -1, 0), to fp32 rounding of the angles
"""
import builtins
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (sets dont_write_bytecode; nothing runs on import)
import numpy as np  # noqa: E402

LOBE = [0.8754318, 0, 1.023545, 0, 0., 0., 0.449686, 0., 0.]  # (:661, a value of the reference's run: data)
REPLAY_PROBES, REPLAY_ROUNDS, REPLAY_BATCH = (9, 27, 63), 40, 96
SEED_PROBES, SEEDS = (9, 27, 36, 63), tuple(range(100, 108))
FULL_PROBES = (9, 36)


def _points(torch, u, dtype):
    """u [rounds, 2, batch] uniforms (fp32, as torch.rand gave them) -> the reference's points (:701-703) at `dtype`."""
    u = u.to(dtype)
    phi = 2 * np.pi * u[:, 0]
    theta = torch.arccos(1 - 2 * u[:, 1])
    return torch.stack([torch.cos(phi) * torch.sin(theta), torch.sin(phi) * torch.sin(theta), torch.cos(theta)], dim=-1)


def _loop(torch, evaluate, sh1, sh2, points, zero_grad=False):
    """fit_product_of_SHs' loop (:696-709) on given points [rounds, batch, 3], at the dtype of its arguments."""
    sh = torch.nn.Parameter(sh1.clone())
    opt = torch.optim.Adam([sh], lr=1e-3)
    for p in points:
        if zero_grad:
            opt.zero_grad()
        gt = evaluate(2, sh1.permute(0, 2, 1), p) * evaluate(2, sh2.permute(0, 2, 1), p)
        pred = evaluate(2, sh.permute(0, 2, 1), p)
        loss = ((gt - pred) ** 2).sum(dim=-1).mean()
        loss.backward()
        opt.step()
    return sh.detach()[0]


class _Replay:
    """What stands in for torch.rand while the reference's function runs: the recorded rows, in order."""

    def __init__(self, torch, u):
        self.rows, self.at, self.torch, self.real = u.reshape(-1, u.shape[-1]), 0, torch, torch.rand

    def __call__(self, size, **kw):
        row = self.rows[self.at]
        self.at += 1
        return row.clone()

    def __enter__(self):
        self.torch.rand = self
        return self

    def __exit__(self, *exc):
        self.torch.rand = self.real
        return False


def main():
    import torch

    mg._install_map_imports()
    for name in ("imageio", "tools.shape_tools"):
        mg._stub(name, write_ply_rgb=None)
    sys.modules.pop("nerf.sh_light_model", None)
    import nerf.sh_light_model as ref_sh
    from nerf.spherical_harmonics import evaluate_spherical_harmonics as evaluate

    out = {}
    # ---- geometry (:657-662)
    H = W = 8
    phi, theta = torch.meshgrid([torch.linspace(np.pi / H, np.pi, H), torch.linspace(-0.5 * np.pi, 1.5 * np.pi, W)], indexing="ij")
    probes = torch.stack([torch.cos(theta) * torch.sin(phi), torch.cos(phi), torch.sin(theta) * torch.sin(phi)], dim=-1).reshape([-1, 3])
    lobe = torch.FloatTensor(LOBE)[None, :]
    lobes = ref_sh.rotate_coeff_by_normal(2, probes, lobe)
    assert lobes.shape == (64, 9) and lobes.dtype == torch.float32
    grid = probes.reshape(8, 8, 3)
    assert (grid[:, 7] - grid[:, 0]).abs().max() < 1e-6, "column 7 repeats column 0"
    assert (grid[7] - torch.tensor([0.0, -1.0, 0.0])).abs().max() < 1e-6, "the last row is the pole, eight times"
    assert abs(float(grid[0, 0, 1]) - np.cos(np.pi / 8)) < 1e-6, "the first row sits at polar angle pi / 8"
    at_z = float(evaluate(2, lobe, torch.tensor([[0.0, 0.0, 1.0]]))[0, 0])
    own = torch.stack([evaluate(2, lobes[i:i + 1], probes[i:i + 1])[0, 0] for i in range(64)])
    assert abs(at_z - 1.0307) < 1e-4 and (own - at_z).abs().max() < 1e-5, (at_z, own)
    s = float(np.sqrt(1 - 0.9995 ** 2))
    extra = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.6 * s, -0.8 * s, 0.9995], [0.6, -1.4, 0.9]])
    extra_lobes = ref_sh.rotate_coeff_by_normal(2, extra.clone(), lobe)
    out.update(probes=probes.numpy(), lobes=lobes.numpy(), lobe=lobe[0].numpy(), extra_normals=extra.numpy(), extra_lobes=extra_lobes.numpy(),
               lobe_at_z=np.float64(at_z))
    print(f"geometry: lobe at +z {at_z:.6f}, max deviation over the 64 probes {float((own - at_z).abs().max()):.2e}")

    rng = np.random.default_rng(4242)
    env = np.zeros((16, 3), np.float32)
    env[0] = (1.8, 1.5, 1.1)
    env[1:9] = rng.normal(0, 0.12, (8, 3)).astype(np.float32)
    env[9:] = rng.normal(0, 0.2, (7, 3)).astype(np.float32)  # rows the fit must not read
    env_t = torch.from_numpy(env)
    sh1 = env_t[None, :9]
    vis = lobes[..., None].repeat([1, 1, 3])  # (:662)
    out["env_shs"] = env

    def reference_fit(i, u, rounds):
        """The reference's own function on the recorded uniforms u [rounds, 2, batch]."""
        ref_sh.range = lambda n: builtins.range(rounds)
        try:
            with _Replay(torch, u) as r:
                got = ref_sh.fit_product_of_SHs(sh1, vis[i:i + 1])
            assert r.at == 2 * rounds
        finally:
            del ref_sh.range
        return got.detach()[0].clone()

    # ---- replay case
    gen = torch.Generator().manual_seed(77)
    pts, fp32, fp64, cleared = [], [], [], []
    for i in REPLAY_PROBES:
        u = torch.rand(REPLAY_ROUNDS, 2, REPLAY_BATCH, generator=gen)
        ref = reference_fit(i, u, REPLAY_ROUNDS)
        p32 = _points(torch, u, torch.float32)
        again = _loop(torch, evaluate, sh1, vis[i:i + 1], p32)
        assert torch.equal(again, ref), "the restated loop without zero_grad is fit_product_of_SHs"
        pts.append(p32.numpy())
        fp32.append(ref.numpy())
        # (the float64 loop on the fp32 points: what a restatement handed these points computes)
        fp64.append(_loop(torch, evaluate, sh1.double(), vis[i:i + 1].double(), p32.double()).numpy())
        cleared.append(_loop(torch, evaluate, sh1, vis[i:i + 1], p32, zero_grad=True).numpy())
    fp32, fp64, cleared = np.stack(fp32), np.stack(fp64), np.stack(cleared)
    g_replay = float(np.abs(fp32 - fp64).max())
    gap_cleared = float(np.abs(cleared - fp32).max())
    assert g_replay < 5e-6 and gap_cleared > 100 * g_replay, (g_replay, gap_cleared)
    out.update(replay_probe_index=np.array(REPLAY_PROBES, np.int64), replay_points=np.stack(pts), replay_fp32=fp32, replay_fp64=fp64,
               replay_zero_grad=cleared, g_replay=np.float64(g_replay))
    print(f"replay case: g_replay {g_replay:.3e}, the zero_grad variant is {gap_cleared:.3e} away")

    # ---- the untouched function at its own size: the stream recorded by re-seeding; g_full; not the minimiser
    t0, g_full = time.time(), 0.0
    for i in FULL_PROBES:
        torch.manual_seed(5)
        ref = ref_sh.fit_product_of_SHs(sh1, vis[i:i + 1]).detach()[0]
        torch.manual_seed(5)
        u = torch.stack([torch.stack([torch.rand([1024]), torch.rand([1024])]) for _ in range(800)])
        p32 = _points(torch, u, torch.float32)
        again = _loop(torch, evaluate, sh1, vis[i:i + 1], p32)
        assert torch.equal(again, ref), "replaying torch.rand reproduces the reference bit for bit"
        wide = _loop(torch, evaluate, sh1.double(), vis[i:i + 1].double(), p32.double())
        g_full = max(g_full, float((again.double() - wide).abs().max()))
        # the L2 projection of the product, by least squares on many points (float64)
        q = _points(torch, torch.rand(1, 2, 40000, generator=gen), torch.float64)[0]
        basis = torch.stack([evaluate(2, torch.eye(9, dtype=torch.float64)[k:k + 1], q)[:, 0] for k in range(9)], dim=-1)
        target = evaluate(2, sh1.double().permute(0, 2, 1), q) * evaluate(2, vis[i:i + 1].double().permute(0, 2, 1), q)
        proj = torch.linalg.lstsq(basis, target).solution
        print(f"probe {i}: DC {env[0, 0]:.2f} -> {float(ref[0, 0]):.3f} after 800 rounds, the projection has {float(proj[0, 0]):.3f}")
        assert abs(float(ref[0, 0]) - float(proj[0, 0])) > 0.1, "the reference's result is defined by its trajectory, not by a minimiser"
    assert g_full < 2e-5, g_full
    out["g_full"] = np.float64(g_full)
    print(f"full size: g_full {g_full:.3e} ({(time.time() - t0) / len(FULL_PROBES):.1f} s per probe for the three loops)")

    # ---- seed case
    runs = np.zeros((len(SEED_PROBES), len(SEEDS), 9, 3), np.float32)
    for a, i in enumerate(SEED_PROBES):
        for b, s in enumerate(SEEDS):
            torch.manual_seed(s)
            runs[a, b] = ref_sh.fit_product_of_SHs(sh1, vis[i:i + 1]).detach()[0].numpy()
    mean, std = runs.astype(np.float64).mean(1), runs.astype(np.float64).std(1, ddof=1)
    out.update(seed_probe_index=np.array(SEED_PROBES, np.int64), seed_mean=mean, seed_std=std, sigma_max=np.float64(std.max()),
               seed_spread=np.float64((runs.max(1) - runs.min(1)).max()))
    print(f"seed case: sigma_max {std.max():.4f}, largest spread over the {len(SEEDS)} seeds {float(out['seed_spread']):.4f}")
    path = os.path.join(mg.OUT, "ref_python_probe_tables.npz")
    np.savez_compressed(path, **out)
    print("wrote ref_python_probe_tables.npz,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
