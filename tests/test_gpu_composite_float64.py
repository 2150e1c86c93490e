"""The training compositing kernels of csrc/raymarching.hip -- composite_train_fwd_kernel, composite_train_bwd_kernel<TAIL, EX> and
composite_step_kernel<KEEP, EX> -- against the float64 restatement of tests/composite_float64.py, value by value, at the edges of the
wave-per-ray design: ray lengths on both sides of every multiple of 64 samples and of 64 * keep, three opacities, forced boundary
samples, permuted output slots, a ray count that is no multiple of the four rays of a workgroup, and three buffer ends (slack rows, the
last ray ending at M, a budget cut in the middle).  The tolerance is C * 2^-24 * (each value's own error magnitude) with the C fixed on
the CPU (tests/test_composite_float64_cpu.py); nothing is compared with another kernel here -- test_gpu_round6.py, test_gpu_criterion.py
and test_gpu_trainstep.py do that.

Every output buffer is filled with NaN first; every call runs twice and must repeat its bits.

Worst |got - float64| / tolerance per group, as printed under `pytest -s` on an MI355X (a record, not an input to C):
    group                      weights_sum  depth   image   image_out  depth_out  grad_sigmas  grad_rgbs  loss, scaled loss / (N 2^-24)
    1 forward                  0.0510       0.0383  0.0937
    2 plain backward                                                              0.0210       0.3114
    3 three launches, mse      0.0510       0.0383  0.0937  0.0409     0.0122     0.0198       0.2579     0.0025
    3 three launches, l1       0.0510       0.0383  0.0937  0.0409     0.0122     0.0176       0.3112     0.0064
    3 three launches, huber0.1 0.0510       0.0383  0.0937  0.0409     0.0122     0.0156       0.3112     0.0041
    3 three launches, huber64  0.0510       0.0383  0.0937  0.0409     0.0122     0.0210       0.2579     0.0025
    4 one launch, <criterion>: the figures of "3 three launches" of the same criterion, digit for digit (every keep).
54 cases, 8.4 s.
"""
import ctypes

import numpy as np
import pytest
import torch

import composite_float64 as cf

pytestmark = pytest.mark.gpu

CRITERIA = [("mse", cf.MSE, 0.0), ("l1", cf.L1, 0.0), ("huber0.1", cf.HUBER, 0.1), ("huber64", cf.HUBER, 64.0)]
VARIANTS = ("slack", "exact", "cut")
WORST = {}


def _note(group, v):
    WORST[group] = max(WORST.get(group, 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nworst |got - float64| / tolerance per group:")
        for k in sorted(WORST):
            print(f"  {k:58s} {WORST[k]:.4f}")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import nerftex_hip  # noqa: F401

    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(dev):
    """The ladder problem on the device, one set of buffers per M variant (exactly M rows long).  Made once, never modified."""
    p = cf.ladder_problem()
    out = {}
    for v in VARIANTS:
        M = p["M"][v]
        t = {k: torch.from_numpy(np.ascontiguousarray(p[k][:M])).to(dev) for k in ("sigmas", "rgbs", "deltas")}
        t.update({k: torch.from_numpy(p[k]).to(dev) for k in ("rays", "nears", "fars", "target", "g_ws", "g_img")})
        out[v] = dict(p=p, M=M, N=p["N"], t=t, live=cf.alive(p, M), covered=cf.covered_rows(p, M))
    return out


_REF = {}


def _reference(c, kind, param, scale):
    key = (c["M"], kind, param, scale)
    if key not in _REF:
        _REF[key] = cf.step_reference(c["p"], c["M"], kind, param, scale)
    return _REF[key]


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _desc(kind, param):
    from nerftex_hip import StepLossDesc

    return StepLossDesc(kind, param, None, None, None, 0, 0.1, 0.9)


def _np(d):
    return {k: v.detach().cpu().numpy() for k, v in d.items()}


def _twice(run):
    """run() -> dict of tensors; a second run must repeat every bit"""
    a, b = _np(run()), _np(run())
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{k}: the second run does not repeat the first one's bits"
    return a


def _forward(dev, c):
    from nerftex_hip import check, lib, ptr, stream

    t, M, N = c["t"], c["M"], c["N"]
    o = dict(weights_sum=_nan(dev, N), depth=_nan(dev, N), image=_nan(dev, N, 3))
    check(lib.nerftex_composite_rays_train_forward(ptr(t["sigmas"]), ptr(t["rgbs"]), ptr(t["deltas"]), ptr(t["rays"]), M, N, ptr(o["weights_sum"]), ptr(o["depth"]),
                                                   ptr(o["image"]), stream()))
    return o


def _three_launches(dev, c, scale, desc, ex):
    """forward, render tail, compositing backward with a root gradient of one (tests/test_gpu_criterion.py::_three_launches)"""
    from nerftex_hip import check, lib, ptr, stream

    t, M, N = c["t"], c["M"], c["N"]
    by = None if desc is None else ctypes.byref(desc)
    o = _forward(dev, c)
    o.update(image_out=_nan(dev, N, 3), depth_out=_nan(dev, N), losses=_nan(dev, 2), grad_sigmas=_nan(dev, M), grad_rgbs=_nan(dev, M, 3))
    one = torch.ones((), device=dev)
    ticket, partial = torch.zeros(1, dtype=torch.int32, device=dev), torch.empty(1024, device=dev)
    words = (M + 31) // 32
    o["flags"] = torch.full((words,), 7, dtype=torch.int32, device=dev)  # (the tail's forward clears them)
    fwd = (ptr(o["weights_sum"]), ptr(o["depth"]), ptr(o["image"]), ptr(t["nears"]), ptr(t["fars"]), ptr(t["target"]), cf.BG, cf.MUL, N, ptr(o["image_out"]),
           ptr(o["depth_out"]), ptr(partial), ptr(ticket), ptr(o["losses"]), ptr(scale), o["losses"].data_ptr() + 4, ptr(o["flags"]), words)
    bwd = (ptr(one), ptr(scale), cf.MUL, ptr(o["image_out"]), ptr(t["target"]), cf.BG, ptr(t["sigmas"]), ptr(t["rgbs"]), ptr(t["deltas"]), ptr(t["rays"]),
           ptr(o["weights_sum"]), ptr(o["image"]), M, N, ptr(o["grad_sigmas"]), ptr(o["grad_rgbs"]), ptr(o["flags"]))
    if ex:
        check(lib.nerftex_render_tail_forward_ex(*fwd, by, stream()))
        check(lib.nerftex_composite_tail_backward_ex(*bwd, by, stream()))
    else:
        check(lib.nerftex_render_tail_forward_live(*fwd, stream()))
        check(lib.nerftex_composite_tail_backward_live(*bwd, stream()))
    assert int(ticket[0]) == 0
    return o


def _one_launch(dev, c, scale, desc, ex):
    from nerftex_hip import check, lib, ptr, stream

    t, M, N = c["t"], c["M"], c["N"]
    o = dict(weights_sum=_nan(dev, N), depth=_nan(dev, N), image=_nan(dev, N, 3), image_out=_nan(dev, N, 3), depth_out=_nan(dev, N), losses=_nan(dev, 2),
             err=_nan(dev, N), grad_sigmas=_nan(dev, M), grad_rgbs=_nan(dev, M, 3), flags=torch.zeros((M + 31) // 32, dtype=torch.int32, device=dev))
    args = (ptr(t["sigmas"]), ptr(t["rgbs"]), ptr(t["deltas"]), ptr(t["rays"]), M, N, ptr(t["nears"]), ptr(t["fars"]), ptr(t["target"]), cf.BG, cf.MUL, ptr(scale),
            ptr(o["weights_sum"]), ptr(o["depth"]), ptr(o["image"]), ptr(o["image_out"]), ptr(o["depth_out"]), ptr(o["err"]), ptr(o["losses"]),
            o["losses"].data_ptr() + 4, ptr(o["grad_sigmas"]), ptr(o["grad_rgbs"]), ptr(o["flags"]))
    if ex:
        check(lib.nerftex_composite_step_ex(*args, None if desc is None else ctypes.byref(desc), stream()))
    else:
        check(lib.nerftex_composite_step(*args, stream()))
    return o


# ---------------------------------------------------------------------------------------------------------------------------- checks
def _check_rays(group, what, got, want, c):
    """weights_sum, depth, image of every ray within the bound; dead and empty rays: exact zeros"""
    dead = c["p"]["rays"][~c["live"], 0]
    for k in ("weights_sum", "depth", "image"):
        r = cf.ratio(got[k], want[k], want[k + "_mag"])
        _note(f"{group}: {k}", r)
        assert r <= 1.0, f"{what}: {k} beyond the bound (worst ratio {r:.3g})"
        assert (got[k][dead] == 0).all(), f"{what}: {k} of a dead or empty ray is not zero"
    assert dead.size >= (2 if c["M"] == c["p"]["M"]["slack"] else 3)


def _check_gradients(group, what, got, want, c, rows=None):
    """both gradients row by row on the rows live rays cover (rows: a further mask)"""
    mask = c["covered"] if rows is None else c["covered"] & rows
    for k in ("grad_sigmas", "grad_rgbs"):
        r = cf.ratio(got[k], want[k], want[k + "_mag"], mask)
        _note(f"{group}: {k}", r)
        if r > 1.0:
            err = np.abs(got[k].astype(np.float64) - want[k]) / cf.tolerance(want[k + "_mag"])
            err = np.where(np.isnan(err), np.inf, err).reshape(c["M"], -1).max(axis=1) * mask
            bad = np.nonzero(err > 1.0)[0]
            off = c["p"]["rays"][:, 1]
            where = [(int(np.searchsorted(off, i, side="right") - 1), int(i - off[np.searchsorted(off, i, side="right") - 1])) for i in bad[:8]]
            raise AssertionError(f"{what}: {k} beyond the bound on {bad.size} rows, worst ratio {r:.3g}; (record, sample) of the first: {where}")


def _check_step(group, what, got, want, c, kind, param, scale):
    """Everything a step's compositing leaves, against float64 (the checks of the three-launch and the one-launch test)."""
    p, M, N = c["p"], c["M"], c["N"]
    _check_rays(group, what, got, want, c)
    for k in ("image_out", "depth_out"):
        r = cf.ratio(got[k], want[k], want[k + "_mag"])
        _note(f"{group}: {k}", r)
        assert r <= 1.0, f"{what}: {k} beyond the bound (worst ratio {r:.3g})"
    # the loss, given the float64 mean of the criterion of the kernel's own float32 image: N roundings at most along its sum
    e, _ = cf.criterion64(kind, float(np.float32(param)), got["image_out"].astype(np.float64) - p["target"].astype(np.float64))
    loss64 = e.sum() / (3.0 * N) * cf.MUL
    for i, (name, w) in enumerate((("loss", loss64), ("scaled loss", loss64 * scale))):
        rel = abs(float(got["losses"][i]) - w) / w
        _note(f"{group}: {name}, / (N 2^-24)", rel / (N * cf.EPS32))
        assert rel <= N * cf.EPS32, f"{what}: {name} {float(got['losses'][i]):.9g}, float64 {w:.9g}"
    rows = None
    if kind == cf.L1:  # an element with |d| < 1e-6 may take either sign: its ray's rows are left out
        ambiguous = np.abs(want["d"]) < 1e-6
        assert ambiguous.mean() < 0.01
        rows = cf.l1_row_mask(p, M, ambiguous)
    _check_gradients(group, what, got, want, c, rows)
    unc = ~c["covered"]
    assert unc.any() and (got["grad_sigmas"][unc] == 0).all() and (got["grad_rgbs"][unc] == 0).all(), f"{what}: a row no live ray covers is not exactly zero"
    # step flags: set exactly where the kernel's own output has a non-zero sample; and wherever float64 says a gradient is above its tolerance
    words = (M + 31) // 32
    pad = words * 32 - M
    nz = (got["grad_sigmas"] != 0) | (got["grad_rgbs"] != 0).any(axis=1)
    own = np.pad(nz, (0, pad)).reshape(words, 32).any(axis=1)
    assert np.array_equal(got["flags"] != 0, own), f"{what}: step flags differ from the non-zero steps of the launch's own gradients"
    big = (np.abs(want["grad_sigmas"]) > cf.tolerance(want["grad_sigmas_mag"])) | (np.abs(want["grad_rgbs"]) > cf.tolerance(want["grad_rgbs_mag"])).any(axis=1)
    if rows is not None:
        big &= rows
    must = np.pad(big, (0, pad)).reshape(words, 32).any(axis=1)
    assert must.any() and (got["flags"][must] != 0).all(), f"{what}: a step with a gradient above its tolerance is not flagged"


# ----------------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("variant", VARIANTS)
def test_forward(dev, cases, variant):
    """nerftex_composite_rays_train_forward: weights_sum, depth and image per ray"""
    c = cases[variant]
    got = _twice(lambda: _forward(dev, c))
    _check_rays("1 forward", f"forward, {variant}", got, cf.forward_reference(c["p"], c["M"]), c)


@pytest.mark.parametrize("variant", VARIANTS)
def test_plain_backward(dev, cases, variant):
    """nerftex_composite_rays_train_backward with given grad_weights_sum / grad_image (an eighth of the rays: exactly zero), weights_sum and
    image from the forward call.  The header: "grad_sigmas/grad_rgbs pre-zeroed" -- the entry writes the rows of live rays and nothing else,
    so the rows of dead rays and the rows no ray covers keep the NaN they were given."""
    from nerftex_hip import check, lib, ptr, stream

    c = cases[variant]
    t, M, N, p = c["t"], c["M"], c["N"], c["p"]
    fw = _forward(dev, c)

    def run():
        o = dict(grad_sigmas=_nan(dev, M), grad_rgbs=_nan(dev, M, 3))
        check(lib.nerftex_composite_rays_train_backward(ptr(t["g_ws"]), ptr(t["g_img"]), ptr(t["sigmas"]), ptr(t["rgbs"]), ptr(t["deltas"]), ptr(t["rays"]),
                                                        ptr(fw["weights_sum"]), ptr(fw["image"]), M, N, ptr(o["grad_sigmas"]), ptr(o["grad_rgbs"]), stream()))
        return o

    got = _twice(run)
    want = cf.backward_reference(p, M, p["g_img"], p["g_ws"])
    _check_gradients("2 plain backward", f"plain backward, {variant}", got, want, c)
    unc = ~c["covered"]
    assert unc.any() and np.isnan(got["grad_sigmas"][unc]).all() and np.isnan(got["grad_rgbs"][unc]).all(), "rows no live ray covers were written"
    zero = (p["g_ws"] == 0) & (p["g_img"] == 0).all(axis=1)
    rows = ~cf.l1_row_mask(p, M, np.repeat(zero[:, None], 3, axis=1)) & c["covered"]
    assert rows.any() and (got["grad_sigmas"][rows] == 0).all() and (got["grad_rgbs"][rows] == 0).all(), "a ray without a gradient has zero gradients"


@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("name,kind,param", CRITERIA, ids=[c[0] for c in CRITERIA])
@pytest.mark.parametrize("variant", VARIANTS)
def test_three_launches(dev, cases, variant, name, kind, param, scaled):
    """forward, nerftex_render_tail_forward_ex, nerftex_composite_tail_backward_ex (for the MSE also the _live entries they extend, and the
    _ex entries with a NULL descriptor)"""
    c = cases[variant]
    scale = torch.full((), 1024.0, device=dev) if scaled else None
    want = _reference(c, kind, param, 1024.0 if scaled else 1.0)
    forms = [("_ex", _desc(kind, param), True)] + ([("_live", None, False), ("_ex(NULL)", None, True)] if kind == cf.MSE else [])
    for form, desc, ex in forms:
        got = _twice(lambda: _three_launches(dev, c, scale, desc, ex))
        _check_step(f"3 three launches, {name}", f"three launches{form}, {variant}, {name}", got, want, c, kind, param, 1024.0 if scaled else 1.0)


@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("name,kind,param", CRITERIA, ids=[c[0] for c in CRITERIA])
@pytest.mark.parametrize("variant", VARIANTS)
def test_one_launch(dev, cases, knobs, variant, name, kind, param, scaled):
    """nerftex_composite_step_ex (for the MSE also nerftex_composite_step: the instantiations per KEEP) for every number of kept chunks --
    the ladder has lengths on both sides of 64 * keep for each -- against float64, not against the three launches."""
    c = cases[variant]
    scale = torch.full((), 1024.0, device=dev) if scaled else None
    want = _reference(c, kind, param, 1024.0 if scaled else 1.0)
    for keep in (0, 1, 3, 4):
        knobs(composite_keep=keep)
        forms = [("_ex", _desc(kind, param), True)] + ([("", None, False)] if kind == cf.MSE else [])
        for form, desc, ex in forms:
            got = _twice(lambda: _one_launch(dev, c, scale, desc, ex))
            _check_step(f"4 one launch, {name}", f"composite_step{form}, keep {keep}, {variant}, {name}", got, want, c, kind, param, 1024.0 if scaled else 1.0)
            e, _ = cf.criterion64(kind, float(np.float32(param)), got["image_out"].astype(np.float64) - c["p"]["target"].astype(np.float64))
            assert (np.abs(got["err"] - e.sum(axis=1)) <= 8 * cf.EPS32 * e.sum(axis=1)).all(), "err[]: three differences, three elements of up to three operations, two sums"
