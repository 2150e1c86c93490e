"""GPU: relighting through the fused lit chains (csrc/curved_light.inc: curved_relight_out_rows_kernel behind the four _relit entries).
  * relight absent: _relit with r = NULL, and with K = 0 and a NULL rotation, is the plain entry bit for bit on all four chains;
  * per-probe lighting through nerftex_curved_light_infer_relit under the rows contract: sigma and mask forward()'s bits, NO row left out --
    every shaded row inside sh_light_float64's bound at the kernel's own shading normal for one of the probes the float64 dot product cannot
    tell apart (the pattern of tests/envmap_float64.py), rows with one candidate also within 2e-2 of forward();
  * the rotation, restated in float64 through its rounding points (tests/relight_float64.py): the framework's own half einsum is that model bit
    for bit on every decided component, the kernel's colours lie inside the composed bound, forward(euler=) within 2e-2;
  * the reference's network executed (tests/golden/ref_python_relight.npz): infer() and forward(euler=) at the bars
    tests/test_gpu_curved_light_infer.py applies to it;
  * the planar, shape and patch chains; the three loops, the graphs kept across rotation vectors, the turntable; the default path.
The field is the 18 x 36 star-flower mesh of the other lit tests.  Every comparison prints its figures (DESIGN.md 4.23 records them)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import envmap_float64 as e64
import relight_float64 as r64
import sh_light_float64 as f64
import test_gpu_curved_light_infer as lit
from test_gpu_curved_light_infer import dev, frame_setup, setup  # noqa: F401  (module-scoped fixtures: the field, its reference, two 32 x 32 poses)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = lit.SENTINEL
EULERS = {"none": None, "zeros": [0.0, 0.0, 0.0], "y60": [0.0, np.pi / 3, 0.0], "generic": [0.4, -1.1, 0.7]}
GAMMA = 2.4


@pytest.fixture(scope="module")
def envmap():
    return np.load(os.path.join(GOLDEN, "ref_python_envmap.npz"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "ref_python_relight.npz"))


@contextlib.contextmanager
def _lighting(field, env_shs=None, tables=None, probes=None, visibility=True, fused=False, relight=False, euler=None, fc=0.7):
    """The field in eval under the given lighting state; everything this file touches is put back."""
    net = field.light_net
    lit._configure(field, "eval", fc)
    try:
        if env_shs is not None:
            net.load_envmap(env_shs=env_shs, env_shs_vis=tables, probes=probes)
        field.shade_visibility, field.fused_light_infer, field.fused_relight_infer = visibility, fused, relight
        field.set_light_rotation(euler)
        yield field
    finally:
        net.import_envmap, net.envSHs_import, net.envSHs_import_vis, net.probes = False, None, None, None
        field.shade_visibility, field.fused_light_infer, field.fused_relight_infer = True, False, False
        field.set_light_rotation(None)
        field.light_visual_mode = "Full"


def _forward(field, x, d, **kw):
    """forward() under fp16 autocast and what it handed to the head -> sigma, colour, dict(n, d, n2)."""
    handed = {}
    handle = field.light_net.register_forward_pre_hook(lambda m, a, k: handed.update(n=a[1].float(), d=a[2].float(), n2=k.get("normal_secondary")), with_kwargs=True)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            sigma, color, _ = field(x, d, **kw)
    finally:
        handle.remove()
    return sigma.float(), color.float(), handed


CHAIN_CALLS = {  # chain -> (entry, the field's descriptor builder, the predicate that must hold)
    "mesh": ("nerftex_curved_light_infer", "_infer_light_desc", "_infer_light_fused"),
    "planar": ("nerftex_curved_light_import_infer", "_infer_light_import_desc", "_infer_light_import_fused"),
    "shape": ("nerftex_curved_light_shape_infer", "_infer_light_shape_desc", "_infer_light_shape_fused"),
    "patch": ("nerftex_curved_light_patch_infer", "_infer_light_patch_desc", "_infer_light_patch_fused"),
}


def _call(field, chain, x, d, relight="plain", live=None):
    """The chain's entry through the descriptor CurvedField builds, outputs pre-filled with the sentinel.  relight: "plain" (the entry without
    _relit), None (_relit with r = NULL) or a RelightDesc."""
    from nerftex_hip import check, lib, stream

    entry, builder, predicate = CHAIN_CALLS[chain]
    n, dv = x.shape[0], x.device
    sigma = torch.full((n,), SENTINEL, dtype=torch.float32, device=dv)
    rgbs = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dv)
    normal = torch.full((n, 3), SENTINEL, dtype=torch.float32, device=dv)
    scratch = torch.empty(getattr(lib, entry + "_scratch_bytes")(n), dtype=torch.uint8, device=dv)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        desc, keep = getattr(field, builder)(x, d, live, sigma, rgbs, scratch, normal)
        if isinstance(relight, str):
            check(getattr(lib, entry)(ctypes.byref(desc), stream()))
        else:
            check(getattr(lib, entry + "_relit")(ctypes.byref(desc), None if relight is None else ctypes.byref(relight), stream()))
    torch.cuda.synchronize()
    return sigma, rgbs, normal


def _marked(x, d, marked):
    xm, dm = x.clone(), d.clone()
    xm[marked] = 1e30
    dm[marked, 0] = 1e30
    return xm, dm


def _t(a, dv):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dv)


def _tables(envmap, K, seed=None):
    """The reference's 8 x 8 grid and its seeded tables (K = 64), or K seeded unit vectors with tables drawn the same way."""
    if K == 64:
        return envmap["probes"], envmap["probe_shs"]
    rng = np.random.default_rng(1000 + K if seed is None else seed)
    p = rng.normal(size=(K, 3))
    tables = rng.normal(0, 0.3, (K, 9, 3)).astype(np.float32)
    tables[:, 0] = rng.uniform(1.0, 3.0, (K, 3))
    return (p / np.linalg.norm(p, axis=-1, keepdims=True)).astype(np.float32), tables


def _half_sigmoids(brdf):
    return torch.sigmoid(brdf[:, :3]).cpu().numpy(), torch.sigmoid(brdf[:, 3:4]).cpu().numpy()


def _check_colours(name, rgbs, rows, a_h, sw_h, vectors, lights, cap=lit.KINK_CAP):
    """rgbs [B,3] (visual mode Full); rows: the indices to hold.  vectors: a list of (normals [B,3], dirs [B,3]) the kernel may have shaded with;
    lights: per row index a list of lightings [>= 9, C] it may have shaded under.  Every row must lie inside sh_light_float64's bound for ONE
    combination; elements in that model's kink bands are excepted, their share capped.  -> the largest error / bound over the rows."""
    got = np.asarray(rgbs, np.float64)
    worst, kinks = 0.0, 0
    for b in rows:
        best, first_kink = np.inf, None
        for n, d in vectors:
            for env in lights[b]:
                ref = f64.shade(a_h[b:b + 1], sw_h[b:b + 1], n[b:b + 1], d[b:b + 1], env, GAMMA, True)
                err = np.abs(got[b] - ref["color"][0])
                ratio = np.where(err == 0, 0.0, err / np.maximum(ref["bound_color"][0], 1e-300))
                ratio = np.where(ref["kink_color"][0], 0.0, ratio)
                if first_kink is None:
                    first_kink = int(ref["kink_color"][0].sum())
                best = min(best, float(ratio.max()))
        kinks += first_kink
        worst = max(worst, best)
    print(f"{name}: {len(rows)} rows, largest colour error / bound {worst:.3f}, elements in kink bands {kinks / max(1, 3 * len(rows)):.4%}")
    assert kinks <= cap * 3 * max(1, len(rows)), (name, kinks)
    assert worst <= 1.0, (name, worst)
    return worst


def _rotation_models(field, euler, *vectors):
    """tests/relight_float64.rotate of each [B,3] array by the fp32 matrix the field's buffer holds for `euler` (None: the vectors as they are)."""
    if euler is None:
        return [dict(value=np.asarray(v, np.float64), other=np.asarray(v, np.float64), decided=np.ones(v.shape, bool)) for v in vectors]
    matrix = field.light_rotation_matrix(euler).astype(np.float32)
    return [r64.rotate(matrix, v) for v in vectors]


# ---- relight absent ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chains(dev, setup):  # noqa: F811
    """One field per chain with 256 points around it, four rows sharing a direction."""
    import import_light_float64 as il64
    import patch_import_float64 as pm
    import planar_float64 as pf
    import test_gpu_import_light as planar_t
    import test_gpu_import_patch as patch_t
    import test_gpu_import_shape_light as shape_t

    n = 256
    out = {"mesh": (setup["field"], setup["x"][:n].contiguous(), setup["d"][:n].contiguous())}
    field = planar_t._lit_field(dev)
    phi_map, local_map, sample, ids_map = il64.seeded_light_maps(24, 20, 5)
    field.import_field(pf.seeded_map(24, 20, seed=21), 1.0 / 32, phi_embed=phi_map, local_tbn=local_map, sample_tbn=sample, sample_tbn_ids=ids_map)
    xn, dn = planar_t._chain_points(n, field.bounds, field.h_threshold)
    out["planar"] = (field, _t(xn, dev), _t(dn, dev))
    field = shape_t._shape_lit_field(dev)
    out["shape"] = (field,) + tuple(t.contiguous() for t in shape_t._chain_points(field, n))
    field = patch_t._field(dev, True)
    patch = patch_t._import(field, patch_t.PATCHES[0][0], patch_t.PATCHES[0][1])
    out["patch"] = (field, _t(pm.case_queries(patch, n, seed=1), dev), patch_t._dirs(n, dev))
    return out


@pytest.mark.parametrize("chain", sorted(CHAIN_CALLS))
def test_without_relighting_the_relit_entry_is_the_plain_entry(dev, chains, chain):  # noqa: F811
    from nerftex_hip import RelightDesc

    field, x, d = chains[chain]
    with _lighting(field, fused=True):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):  # (no_grad: the encoders hand out their fp16 tables in inference only)
            assert getattr(field, CHAIN_CALLS[chain][2])(x, d)
        want = _call(field, chain, x, d, "plain")
        assert float(want[0].max()) > 0 and float(want[1].max()) > 0 and float(want[2].abs().max()) > 0  # (not a comparison of zeros)
        for name, r in (("r = NULL", None), ("K = 0, rotation NULL", RelightDesc())):
            got = _call(field, chain, x, d, r)
            for what, a, b in zip(("sigma", "rgbs", "shading normal"), got, want):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (chain, name, what)


# ---- per-probe lighting through the mesh chain --------------------------------------------------------------------------------------------------------------------

PROBE_CASES = [(128, 64, "all"), (256, 1, "all"), (256, 3, "marked"), (256, 256, "live"), (256, 64, "marked"), (128, 256, "all")]


@pytest.mark.parametrize("B,K,rows", PROBE_CASES, ids=[f"B{b}-K{k}-{r}" for b, k, r in PROBE_CASES])
def test_per_probe_lighting_through_the_mesh_chain(dev, setup, envmap, B, K, rows):  # noqa: F811
    from nerftex_hip import RelightDesc, ptr

    field, x, d = setup["field"], setup["x"][:B].contiguous(), setup["d"][:B].contiguous()
    probes, tables = _tables(envmap, K)
    marked = lit._marks(dev, B) if rows == "marked" else torch.zeros(B, dtype=torch.bool, device=dev)
    live_rows = 128 if rows == "live" else B
    live = (torch.tensor([1], dtype=torch.int32, device=dev), 128) if rows == "live" else None
    xm, dm = _marked(x, d, marked)
    with _lighting(field, envmap["uniform_env_shs"], tables, probes, fused=True) as field:
        sigma_f, color_f, handed = _forward(field, x, d)
        pt, tt = _t(probes, dev), _t(tables, dev)
        sigma, rgbs, normal = _call(field, "mesh", xm, dm, RelightDesc(probes=ptr(pt), probe_shs=ptr(tt), K=K), live)
    idx = torch.arange(B, device=dev)
    plain, unused, past = (idx < live_rows) & ~marked, (idx < live_rows) & marked, idx >= live_rows
    assert torch.equal(sigma[plain].view(torch.int32), sigma_f[plain].view(torch.int32)), "sigma: forward()'s bits"
    shaded = (sigma != 0) | (rgbs != 0).any(-1)
    mask = (sigma_f != 0) | (color_f != 0).any(-1)
    assert torch.equal(shaded[plain], mask[plain]) and 0 < int(mask[plain].sum()) < int(plain.sum()), "the mask: forward()'s, both sides exercised"
    assert not sigma[unused].any() and not rgbs[unused].any(), "marked slots are exactly 0"
    assert bool((sigma[past] == SENTINEL).all()) and bool((rgbs[past] == SENTINEL).all()) and bool((normal[past] == SENTINEL).all()), "untouched rows keep the sentinel"
    assert torch.isfinite(rgbs[plain]).all()
    # no row is left out: every shaded row against the float64 model at the kernel's own shading normal, under one of its candidate probes
    ref = setup["refs"][("eval", 0.7)]
    a_h, sw_h = _half_sigmoids(ref["brdf"][:B])
    cands = e64.probe_candidates(handed["n2"].cpu().numpy(), probes)
    hold = np.nonzero((plain & mask).cpu().numpy())[0]
    lights = {b: [tables[k] for k in np.nonzero(cands[b])[0]] for b in hold}
    _check_colours(f"per-probe B={B} K={K} {rows}", rgbs.cpu().numpy(), hold, a_h, sw_h, [(normal.cpu().numpy(), d.cpu().numpy())], lights)
    single = cands.sum(-1) == 1
    print(f"B={B} K={K}: rows with a single candidate {single.mean():.2%}")
    if K != 64:
        assert single.mean() >= 0.95, "seeded probes decide nearly every row: the candidate check is not vacuous"
    strict = hold[single[hold]]
    err = float((rgbs - color_f)[strict].abs().max())
    print(f"B={B} K={K}: largest |chain - forward()| colour on {len(strict)} single-candidate rows {err:.3e}")
    assert err <= 2e-2
    assert float((normal - handed["n"])[hold].abs().max()) <= 5e-3, "shading_normal is the (unrotated) normal forward() shades with"


def test_the_lowest_index_wins_among_equal_probe_directions(dev, setup, envmap):  # noqa: F811
    from nerftex_hip import RelightDesc, ptr

    field, x, d = setup["field"], setup["x"][:128].contiguous(), setup["d"][:128].contiguous()
    probes, tables = _tables(envmap, 3)
    same = np.repeat(probes[:1], 3, axis=0)
    with _lighting(field, envmap["uniform_env_shs"], visibility=False, fused=True):
        run = lambda p, t: _call(field, "mesh", x, d, RelightDesc(probes=ptr(p), probe_shs=ptr(t), K=p.shape[0]))[1]  # noqa: E731
        got = run(_t(same, dev), _t(tables, dev))
        assert torch.equal(got, run(_t(same[:1], dev), _t(tables[:1], dev)))
        assert not torch.equal(got, run(_t(same, dev), _t(tables[::-1], dev)))


# ---- the rotation ---------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lighting", ("uniform3", "white1"))
def test_rotation_through_the_mesh_chain(dev, setup, envmap, lighting):  # noqa: F811
    from nerftex_hip import RelightDesc, ptr

    field, B = setup["field"], 256
    x, d = setup["x"][:B].contiguous(), setup["d"][:B].contiguous()
    ref = setup["refs"][("eval", 0.7)]
    a_h, sw_h = _half_sigmoids(ref["brdf"][:B])
    env = envmap["uniform_env_shs"] if lighting == "uniform3" else None
    colours = {}
    for tag, euler in EULERS.items():
        with _lighting(field, env, visibility=False, fused=True, euler=euler) as field:
            light = field._lighting().detach().cpu().numpy()
            assert light.shape[1] == (3 if lighting == "uniform3" else 1)
            _, _, plain = _forward(field, x, d, euler=None)
            sigma_f, color_f, handed = _forward(field, x, d, euler=euler)
            r = None if euler is None else RelightDesc(rotation=ptr(field._light_rotation))
            sigma, rgbs, normal = _call(field, "mesh", x, d, r)
        mask = ((sigma_f != 0) | (color_f != 0).any(-1)).cpu().numpy()
        assert torch.equal(sigma.view(torch.int32), sigma_f.view(torch.int32)), "the rotation turns the lighting, not the density"
        assert np.array_equal(((sigma != 0) | (rgbs != 0).any(-1)).cpu().numpy(), mask)
        # the framework's own half einsum against the float64 model through the recorded rounding points: bit for bit where decided
        for key in ("n", "d"):
            (m,) = _rotation_models(field, euler, plain[key].cpu().numpy())
            got = handed[key].cpu().numpy().astype(np.float64)
            dec = m["decided"]
            assert np.array_equal(got[dec], m["value"][dec]), (tag, key, "forward()'s rotated vector is the model's on every decided component")
            assert np.all((got == m["value"]) | (got == m["other"])), (tag, key)
            if euler is not None:
                err = np.abs(got - m["exact"])
                print(f"{lighting} {tag} {key}: undecided components {int((~dec).sum())} of {dec.size}, largest |einsum - exact| / bound {float((err / m['bound']).max()):.3f}")
                assert float((err / m["bound"]).max()) <= 1.0
        # the kernel: its own (unrotated) shading normal and the direction, rotated by the model, then sh_light_float64's bound
        mn, md = _rotation_models(field, euler, normal.cpu().numpy(), d.cpu().numpy())
        hold = np.nonzero(mask)[0]
        vectors = [(mn["value"], md["value"])] + [v for v in r64.variants(mn, md)][1:]
        decided_rows = (mn["decided"].all(-1) & md["decided"].all(-1))
        _check_colours(f"rotation {lighting} {tag} (decided rows)", rgbs.cpu().numpy(), hold[decided_rows[hold]], a_h, sw_h, vectors[:1], {b: [light] for b in hold})
        if (~decided_rows[hold]).any():
            _check_colours(f"rotation {lighting} {tag} (undecided rows)", rgbs.cpu().numpy(), hold[~decided_rows[hold]], a_h, sw_h, vectors, {b: [light] for b in hold}, cap=1.0)
        err = float((rgbs - color_f)[hold].abs().max())
        print(f"rotation {lighting} {tag}: largest |chain - forward(euler=)| colour {err:.3e}, values that differ {int((rgbs != color_f).sum())}")
        assert err <= 2e-2
        assert float((normal - plain["n"])[hold].abs().max()) <= 5e-3, "shading_normal stays the unrotated normal"
        colours[tag] = rgbs
    moved = float((colours["zeros"] - colours["none"]).abs().max())
    print(f"{lighting}: zeros against None, largest colour difference {moved:.3e} (the half rounding of the vectors); y60 against None "
          f"{float((colours['y60'] - colours['none']).abs().max()):.3e}")
    assert 0 < moved <= 2e-2, "a zero vector is the identity product rounded to half: not None, and no further from it than the colour bar"
    # (under the trained white lighting bands 1.. are a tenth of the DC term: 2.1e-2 seen, against 1.1e-1 under the imported lighting)
    assert float((colours["y60"] - colours["none"]).abs().max()) > 5e-3 and float((colours["generic"] - colours["y60"]).abs().max()) > 5e-3, "the rotation shows"


# ---- the reference's network, executed ----------------------------------------------------------------------------------------------------------------------------------

def test_the_references_network_under_relighting(dev, envmap, golden):  # noqa: F811
    from test_gpu_sh_light import _field_from_fixture

    g, field, x, d, ok = _field_from_fixture(dev)
    B = x.shape[0]
    pad = -B % 128 or 128
    xp, dp = torch.full((B + pad, 3), 1e30, device=dev), torch.full((B + pad, 3), 1e30, device=dev)
    xp[:B], dp[:B] = x, d
    hm = golden["h_mask"]
    rows = ok & hm
    probes, tables = envmap["probes"], envmap["probe_shs"]
    fc = float(g["fc_weight"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ones = torch.ones(B, 1, dtype=torch.float16, device=dev)
        brdf = field.light_net.brdf_layer(torch.cat([_t(golden["head_geo_feat"], dev), ones], dim=-1))
    a_h, sw_h = _half_sigmoids(brdf)
    for i in range(3):
        euler = golden[f"r{i}_euler"]
        for mode in ("uniform", "probe"):
            with _lighting(field, envmap["uniform_env_shs"], tables, probes, visibility=mode == "probe", fused=True, relight=True, euler=euler, fc=fc) as field:
                sigma_f, color_f, handed = _forward(field, x, d)
                _, color_kw, _ = _forward(field, x, d, euler=euler)
                assert torch.equal(color_kw, color_f), "the keyword and the stored rotation are one path"
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    assert field._infer_light_fused(xp, dp)
                    sigma, rgbs = field.infer(xp, dp)
                _, _, normal = _call(field, "mesh", xp, dp, field._relight_desc()[0])
            assert not sigma[B:].any() and not rgbs[B:].any()
            want = golden[f"r{i}_{mode}_full"]
            for name, s, c in (("infer()", sigma[:B], rgbs[:B]), ("forward(euler=)", sigma_f, color_f)):
                shaded = ((s != 0) | (c != 0).any(-1)).cpu().numpy()
                assert np.array_equal(shaded[ok], hm[ok]), (i, mode, name, "mask")
                np.testing.assert_allclose(s.cpu().numpy()[ok], golden["sigma"][ok], rtol=3e-2, atol=3e-3)
                err = np.abs(c.cpu().numpy() - want).max(-1)
                if mode == "uniform":
                    print(f"r{i} {mode} {name}: colour max |diff| {float(err[ok].max()):.2e}")
                    assert err[ok].max() <= 2e-2
                    continue
                # per-probe: the reference's row-by-row values; a row whose probe a half ulp of the rotated coarse normal could change
                # (margin: one half ulp of each component, 3 x 2^-11) is held to the shading under any of its candidates
                cands = e64.probe_candidates(golden[f"r{i}_head_normal_secondary"], probes, margin=3 * 2.0 ** -11)
                single = cands.sum(-1) == 1
                print(f"r{i} {mode} {name}: colour max |diff| on {int((rows & single).sum())} single-candidate rows {float(err[rows & single].max()):.2e}; "
                      f"{int((rows & ~single).sum())} rows with several candidates")
                assert err[ok & single].max() <= 2e-2
                for b in np.nonzero(rows & ~single & (err > 2e-2))[0]:
                    alt = [f64.shade(a_h[b:b + 1], sw_h[b:b + 1], golden[f"r{i}_head_normal"][b:b + 1], golden[f"r{i}_head_view_dirs"][b:b + 1], tables[k], GAMMA, True)
                           ["color"][0] for k in np.nonzero(cands[b])[0]]
                    assert min(float(np.abs(c[b].cpu().numpy() - a).max()) for a in alt) <= 2e-2, (i, name, b)
            # the normals handed to the head: forward()'s rotated one against the reference's, the chain's shading_normal (unrotated) against the
            # reference's unrotated one
            nerr = np.abs(handed["n"].cpu().numpy() - golden[f"r{i}_head_normal"])[rows]
            uerr = np.abs(normal[:B].cpu().numpy() - golden["none_head_normal"])[rows]
            derr = np.abs(handed["d"].cpu().numpy() - golden[f"r{i}_head_view_dirs"])[rows]
            print(f"r{i} {mode}: handed normal max |diff| {float(nerr.max()):.2e}, view direction {float(derr.max()):.2e}, chain's shading normal {float(uerr.max()):.2e}")
            assert nerr.max() <= 5e-3 and uerr.max() <= 5e-3 and derr.max() <= 5e-3


# ---- the other three chains -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chain", ("planar", "shape", "patch"))
def test_the_import_chains_relit(dev, chains, envmap, chain, monkeypatch):  # noqa: F811
    import nerftex_hip

    field, x, d = chains[chain]
    x, d = x[:128].contiguous(), d[:128].contiguous()
    probes, tables = _tables(envmap, 64)
    euler = EULERS["generic"]
    calls = []
    for name in [c[0] for c in CHAIN_CALLS.values()]:
        for suffix in ("", "_relit"):
            fn = getattr(nerftex_hip.lib, name + suffix)
            monkeypatch.setattr(nerftex_hip.lib, name + suffix, lambda *a, _fn=fn, _n=name + suffix: (calls.append(_n), _fn(*a))[1])
    with _lighting(field, envmap["uniform_env_shs"], tables, probes, fused=True, relight=True, euler=euler) as field:
        _, _, plain = _forward(field, x, d, euler=None)
        sigma_f, color_f, handed = _forward(field, x, d)
        assert not calls
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            sigma, rgbs = field.infer(x, d)
        (m,) = _rotation_models(field, euler, plain["n2"].cpu().numpy())
    assert calls == [CHAIN_CALLS[chain][0] + "_relit"], calls
    assert torch.equal(sigma.view(torch.int32), sigma_f.view(torch.int32)), "sigma: forward()'s bits"
    mask = (sigma_f != 0) | (color_f != 0).any(-1)
    assert torch.equal((sigma != 0) | (rgbs != 0).any(-1), mask) and 0 < int(mask.sum()) < 128
    single = (e64.probe_candidates(m["value"], probes).sum(-1) == 1) & m["decided"].all(-1)
    hold = np.nonzero(mask.cpu().numpy() & single)[0]
    err = float((rgbs - color_f)[hold].abs().max())
    print(f"{chain}: largest |chain - forward()| colour on {len(hold)} single-candidate rows {err:.3e} ({int(mask.sum())} rows inside the mask)")
    assert len(hold) > 16 and err <= 2e-2


# ---- the loops ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_loops_under_per_probe_lighting_and_a_turning_light(dev, frame_setup, envmap):  # noqa: F811
    field, r, frames = (frame_setup[k] for k in ("field", "r", "frames"))
    ro, rd = frames[0]
    probes, tables = _tables(envmap, 64)
    kw = dict(slots_per_ray=4, **lit.KW)
    graphed = lambda: r.render_infer_graphed(ro, rd, parts=2, block=2, **kw)  # noqa: E731
    with _lighting(field, envmap["uniform_env_shs"], tables, probes, fused=True, relight=True) as field, torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        img, dep, _ = r.render_infer(ro, rd, **kw)
        img_p, dep_p, _ = r.render_infer_pipelined(ro, rd, parts=2, **kw)
        img_g, dep_g, _ = graphed()
        assert float(img.std()) > 1e-3
        assert torch.equal(img_p, img) and torch.equal(dep_p, dep) and torch.equal(img_g, img) and torch.equal(dep_g, dep), "the three loops agree"
        unrotated = r._infer_graphs
        field.set_light_rotation(EULERS["y60"])
        img_1, _, _ = graphed()
        graphs = r._infer_graphs
        assert graphs is not unrotated and not torch.equal(img_1, img), "a rotation switched on re-records"
        field.set_light_rotation(EULERS["generic"])
        img_2, dep_2, _ = graphed()
        assert r._infer_graphs is graphs, "another rotation vector KEEPS the recorded graphs"
        assert not torch.equal(img_2, img_1), "... and changes the image"
        want = r.render_infer(ro, rd, **kw)
        assert torch.equal(img_2, want[0]) and torch.equal(dep_2, want[1]), "the replayed frame is render_infer's under the same rotation"
        print(f"32 x 32 frame: largest |y60 - unrotated| {float((img_1 - img).abs().max()):.3e}, |generic - y60| {float((img_2 - img_1).abs().max()):.3e}")
        field.set_light_rotation(None)
        img_0, _, _ = graphed()
        assert r._infer_graphs is not graphs and torch.equal(img_0, img), "rotation off re-records: the unrotated image again"
        # the turntable: 4 frames, linspace(0, 2 pi, 4) on euler[0]
        field.set_light_rotation(EULERS["generic"])
        seen, out = [], []
        for frame in r.render_light_turntable(ro, rd, 4, axis=0, parts=2, block=2, **kw):
            seen.append(r._infer_graphs)
            out.append(frame[0])
        assert len(out) == 4 and all(s is seen[0] for s in seen), "the frames of a turntable replay one recording"
        assert field.light_rotation() == tuple(EULERS["generic"]), "the rotation set before is restored"
        field.set_light_rotation(EULERS["zeros"])
        zero, _, _ = graphed()
        assert r._infer_graphs is seen[0], "at most one recording for the whole turntable (and none for a vector set afterwards)"
        assert torch.equal(out[0], zero), "frame 0 is the zero-vector frame"
        assert not torch.equal(out[0], out[1]) and not torch.equal(out[1], out[2]) and not torch.equal(out[0], out[2])
        # (linspace closes the turn: the last frame's matrix differs from the identity by sin(2 pi) = -2.4e-16, which rounds to -0 in half)
        assert torch.equal(out[3], out[0]) and not torch.equal(out[3], out[1]) and not torch.equal(out[3], out[2])


# ---- the default path ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_with_the_switch_off_per_probe_lighting_and_rotations_are_forwards(dev, setup, envmap, monkeypatch):  # noqa: F811
    import nerftex_hip

    field, x, d = setup["field"], setup["x"][:256].contiguous(), setup["d"][:256].contiguous()
    probes, tables = _tables(envmap, 64)
    calls = []
    for name in [c[0] for c in CHAIN_CALLS.values()]:
        for suffix in ("", "_relit"):
            fn = getattr(nerftex_hip.lib, name + suffix)
            monkeypatch.setattr(nerftex_hip.lib, name + suffix, lambda *a, _fn=fn, _n=name + suffix: (calls.append(_n), _fn(*a))[1])
    for euler in (None, EULERS["generic"]):
        with _lighting(field, envmap["uniform_env_shs"], tables, probes, fused=True, relight=False, euler=euler) as field:
            sigma_f, color_f, _ = _forward(field, x, d)
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                sigma, rgbs = field.infer(x, d)
        assert not calls, "no entry of the lit chains is called"
        assert torch.equal(sigma, sigma_f) and torch.equal(rgbs, color_f), "infer() is forward()"
    with _lighting(field, envmap["uniform_env_shs"], visibility=False, fused=True, relight=False, euler=EULERS["generic"]) as field:
        sigma_f, color_f, _ = _forward(field, x, d)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            sigma, rgbs = field.infer(x, d)
    assert not calls and torch.equal(rgbs, color_f), "a rotation alone, switch off: forward()"
    with _lighting(field, envmap["uniform_env_shs"], visibility=False, fused=True, relight=True) as field:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            field.infer(x, d)
    assert calls == ["nerftex_curved_light_infer"], "switch on, nothing to relight: the plain entry with its existing arguments"
