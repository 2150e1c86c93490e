#!/usr/bin/env python3
"""Generate tests/golden/ref_python_relight.npz FROM THE REFERENCE ITSELF: network_curvedfield.NeRFNetwork.forward(x, d, euler=...) executed on the
CPU, in eval, under an imported lighting -- on the construction of ref_python_curvedfield_sh.npz (make_golden.sh_field_network: 768 points,
fc_weight 0.7, the weights that fixture records), with the probe grid, the probe tables and the uniform lighting of ref_python_envmap.npz.
Needs the reference checkout (NERFTEX_REFERENCE) and scipy; it never runs where the GPU tests run.  Values only: no reference text is stored.

Three rotation vectors -- zeros (the reference multiplies by the identity, it does not skip), [0, pi/3, 0] (a turn about the axis the
reference's shape turntable uses) and one generic vector.  Per vector i:
    r{i}_euler, r{i}_matrix   the vector and scipy's R.from_rotvec(euler).as_matrix(), float64
    r{i}_head_normal / _view_dirs / _normal_secondary
                              what NeRFNetwork.forward hands to the light head (:334-341), captured by a pre-hook with kwargs
    r{i}_uniform_full         the returned colours, light_visual_mode 'Full', shade_visibility False: envSHs_import lights every sample
    r{i}_probe_full           the same under per-probe lighting, ROW BY ROW: the head is fed one captured row at a time (the reference scales a
                              row's specular term by its position in the batch, ref_python_envmap.npz's probe_rows_*; a row shaded as the
                              first of its batch is free of that), then masked as :396-397 does
    r2_{uniform,probe}_{specular,diffuse,albedo}   the generic vector's other three visual modes
and once: sigma, h_mask, head_geo_feat (the half features the head is fed), the unrotated head inputs (euler=None), which fixtures the
weights and the lighting come from.

CPU emulation: make_golden.emulated_autocast switches the autocast FLAG on (the reference's Python reads it), but the framework does not
autocast CPU tensors under it, so `torch.einsum('ab,nb->na', rot, v)` here is an fp32 product and the captured rotated vectors are NOT
rounded to half as the GPU's are.  The difference is one half rounding of the matrix, one of the vector and one of the result -- each bounded by
half a half ulp, 2^-11 relative (4.9e-4 near 1) -- recorded as `cpu_einsum_is_fp32`; the tests bound it (tests/relight_float64.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (sets dont_write_bytecode; nothing runs on import)
import numpy as np  # noqa: E402

EULERS = ([0.0, 0.0, 0.0], [0.0, np.pi / 3, 0.0], [0.4, -1.1, 0.7])
MODES = ("Full", "Specular", "Diffuse", "Albedo")


def main():
    import torch
    from scipy.spatial.transform import Rotation

    net, mff, x, d, made = mg.sh_field_network()
    env = np.load(os.path.join(mg.OUT, "ref_python_envmap.npz"))
    head = net.light_net
    head.envSHs_import = torch.nn.Parameter(torch.from_numpy(env["uniform_env_shs"]), requires_grad=False)
    head.sh_order_import = 3
    head.envSHs_import_vis = torch.nn.Parameter(torch.from_numpy(env["probe_shs"]), requires_grad=False)
    head.probes = torch.nn.Parameter(torch.from_numpy(env["probes"]), requires_grad=False)
    head.sh_order_import_vis = 2
    head.import_envmap = True
    net.eval()

    handed = {}

    def capture(module, args, kwargs):
        handed.update(geo=args[0].detach().clone(), normal=args[1].detach().clone(), view=args[2].detach().clone(),
                      secondary=kwargs["normal_secondary"].detach().clone(), visibility=bool(kwargs["shade_visibility"]))

    hook = head.register_forward_pre_hook(capture, with_kwargs=True)
    out = dict(weights_of="ref_python_curvedfield_sh.npz", lighting_of="ref_python_envmap.npz", fc_weight=np.float64(made["fc_weight"]),
               cpu_einsum_is_fp32=np.bool_(True))

    def run(euler, mode, visibility):
        net.light_visual_mode, net.shade_visibility = mode, visibility
        with torch.no_grad(), mg.emulated_autocast():
            sigma, color, ret = net(x, d, euler=None if euler is None else np.array(euler, np.float64), is_gui_mode=False)
        assert ret == {} and handed["visibility"] is visibility
        return sigma.float().numpy(), color.float().numpy()

    def rows(mode_index, h_mask):
        """The head on the rows captured last, one row per call, per-probe lighting; -> [N, 3] masked as the network masks its colour."""
        got, h = [], dict(handed)  # (the hook fires on the calls below too)
        with torch.no_grad(), mg.emulated_autocast():
            for b in range(x.shape[0]):
                res = head(h["geo"][b:b + 1], h["normal"][b:b + 1], h["view"][b:b + 1], normal_secondary=h["secondary"][b:b + 1], shade_visibility=True, gamma=None)
                got.append(res[mode_index].float())
        color = torch.cat(got).numpy()
        return np.where(h_mask[:, None], color, np.zeros_like(color))

    sigma, _ = run(None, "Full", False)
    h_mask = sigma != 0
    out.update(sigma=sigma, h_mask=h_mask, head_geo_feat=handed["geo"].numpy(), none_head_normal=handed["normal"].float().numpy(),
               none_head_view_dirs=handed["view"].float().numpy(), none_head_normal_secondary=handed["secondary"].float().numpy())
    assert handed["geo"].dtype == torch.float16
    for i, euler in enumerate(EULERS):
        matrix = Rotation.from_rotvec(np.array(euler, np.float64)).as_matrix()
        s, full = run(euler, "Full", False)
        assert np.array_equal(s, sigma), "the rotation turns the lighting, not the density"
        assert handed["normal"].dtype == torch.float32, "the CPU einsum stayed fp32 (see the module's docstring)"
        out.update({f"r{i}_euler": np.array(euler, np.float64), f"r{i}_matrix": matrix, f"r{i}_head_normal": handed["normal"].numpy(),
                    f"r{i}_head_view_dirs": handed["view"].numpy(), f"r{i}_head_normal_secondary": handed["secondary"].numpy(), f"r{i}_uniform_full": full})
        want = np.einsum("ab,nb->na", matrix, out["none_head_normal"].astype(np.float64))
        assert np.abs(out[f"r{i}_head_normal"] - want).max() < 1e-6, "the head is handed the rotated shading normal"
        run(euler, "Full", True)  # (captures the same rows under shade_visibility; its batched colours are not kept)
        out[f"r{i}_probe_full"] = rows(0, h_mask)
        if i == 2:
            for k, mode in enumerate(MODES[1:], start=1):
                out[f"r2_uniform_{mode.lower()}"] = run(euler, mode, False)[1]
                out[f"r2_probe_{mode.lower()}"] = rows(k, h_mask)
        print(f"euler {euler}: uniform colour {full.min():.4f} .. {full.max():.4f}, per-probe {out[f'r{i}_probe_full'].min():.4f} .. "
              f"{out[f'r{i}_probe_full'].max():.4f}, moved by the rotation (uniform) {np.abs(full - out.get('r0_uniform_full', full)).max():.4f}")
    hook.remove()
    assert np.abs(out["r1_uniform_full"] - out["r0_uniform_full"]).max() > 1e-2, "the rotation shows"
    path = os.path.join(mg.OUT, "ref_python_relight.npz")
    np.savez_compressed(path, **out)
    print("wrote ref_python_relight.npz,", os.path.getsize(path), "bytes; rows inside the height band:", int(h_mask.sum()), "of", h_mask.shape[0])


if __name__ == "__main__":
    main()
