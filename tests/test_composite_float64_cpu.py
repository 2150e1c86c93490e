"""tests/composite_float64.py checked on the CPU: its closed-form backward against float64 autograd through its own forward, its bound
against two float32 emulations of the walk (accepted at a ratio of at most 0.5) and against nine deliberately wrong tree walks (each
rejected on at least one output).  The bound and its constant are fixed here, before any GPU output is looked at."""
import numpy as np
import pytest
import torch

import composite_float64 as cf

CRITERIA = [("mse", cf.MSE, 0.0), ("l1", cf.L1, 0.0), ("huber0.1", cf.HUBER, 0.1), ("huber64", cf.HUBER, 64.0)]
VARIANTS = ("slack", "exact", "cut")
WORST = {}


@pytest.fixture(scope="module")
def problem():
    return cf.ladder_problem()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nworst |emulation - float64| / tolerance:")
        for k in sorted(WORST):
            print(f"  {k:40s} {WORST[k]:.4f}")


def test_the_problem_is_the_one_described(problem):
    p = problem
    rays = p["rays"].astype(np.int64)
    N = p["N"]
    assert N == 297 and N % 4 != 0 and sorted(rays[:, 0]) == list(range(N)) and not np.array_equal(rays[:, 0], np.arange(N))
    assert np.array_equal(rays[:, 1], np.cumsum(rays[:, 2]) - rays[:, 2])
    for n in cf.LADDER:
        assert int((rays[:, 2] == n).sum()) >= 3
    for keep in (1, 2, 3, 4):
        assert (rays[:, 2] == 64 * keep).any() and (rays[:, 2] == 64 * keep + 1).any() and (rays[:, 2] == 64 * keep - 1).any()
    assert p["M"]["slack"] == p["total"] + 8 and p["M"]["exact"] == rays[-1, 1] + rays[-1, 2] and rays[-1, 2] > 0
    live = {v: cf.alive(p, p["M"][v]) for v in VARIANTS}
    assert live["slack"].sum() == (rays[:, 2] > 0).sum() and live["exact"].sum() == live["slack"].sum() - 1 and not live["exact"][-1]
    cut = p["cut_ray"]
    assert live["cut"][:cut].sum() == (rays[:cut, 2] > 0).sum() and not live["cut"][cut:].any() and rays[cut, 1] < p["M"]["cut"] < rays[cut, 1] + rays[cut, 2]
    # the three opacities, and the forced boundary samples of the thin and the medium rays
    x = p["sigmas"].astype(np.float64) * p["deltas"][:, 0]
    half = (N - 3 * len(cf.LADDER)) // 2
    for j, n in enumerate(cf.LADDER):
        for o, tau in enumerate(cf.OPACITIES):
            _, off, cnt = rays[half + 3 * j + o]
            assert cnt == n
            alpha = 1 - np.exp(-x[off:off + cnt])
            at = [i for i in [63] + list(range(64, n, 64)) if i < n]
            if o < 2 and at:
                assert (alpha[at] > 0.19).all() and (alpha[at] < 0.51).all()
                rest = np.delete(x[off:off + cnt], at).sum()
                assert abs(rest - tau) < 0.5 * tau
            elif n:
                assert abs(x[off:off + cnt].sum() - tau) < 1e-3 * tau


# ------------------------------------------------------------------------------------------------------- the reference against autograd
def _autograd(p, M, kind, param, scale, given=None):
    """tests/test_independent_anchors.py::_composite_reference, extended with the depth, the tail and the criterion"""
    F8 = torch.float64
    s = torch.from_numpy(p["sigmas"][:M]).double().requires_grad_(True)
    c = torch.from_numpy(p["rgbs"][:M]).double().requires_grad_(True)
    d = torch.from_numpy(p["deltas"][:M]).double()
    N = p["N"]
    ws, dep, img = [torch.zeros((), dtype=F8)] * N, [torch.zeros((), dtype=F8)] * N, [torch.zeros(3, dtype=F8)] * N
    for (rid, off, cnt), a in zip(p["rays"], cf.alive(p, M)):
        if not a:
            continue
        al = 1 - torch.exp(-s[off:off + cnt] * d[off:off + cnt, 0])
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=F8), 1 - al]), 0)[:-1]
        w = al * T
        ws[rid], img[rid], dep[rid] = w.sum(), (w[:, None] * c[off:off + cnt]).sum(0), (w * torch.cumsum(d[off:off + cnt, 1], 0)).sum()
    ws, dep, img = torch.stack(ws), torch.stack(dep), torch.stack(img)
    if given is not None:
        loss = (ws * torch.from_numpy(given[0]).double()).sum() + (img * torch.from_numpy(given[1]).double()).sum()
        loss.backward()
        return dict(weights_sum=ws, depth=dep, image=img, grad_sigmas=s.grad, grad_rgbs=c.grad)
    image_out = img + (1 - ws)[:, None] * cf.BG
    near, far, tgt = (torch.from_numpy(p[k]).double() for k in ("nears", "fars", "target"))
    depth_out = torch.clamp(dep - near, min=0) / (far - near)
    if kind == cf.MSE:
        crit = torch.nn.functional.mse_loss(image_out, tgt)
    elif kind == cf.L1:
        crit = torch.nn.functional.l1_loss(image_out, tgt)
    else:
        crit = torch.nn.functional.huber_loss(image_out, tgt, delta=float(np.float32(param)))
    loss = crit * cf.MUL
    (loss * scale).backward()
    return dict(weights_sum=ws, depth=dep, image=img, image_out=image_out, depth_out=depth_out, loss=loss, scaled_loss=loss * scale, grad_sigmas=s.grad,
                grad_rgbs=c.grad)


def _close(name, got, want, floor=0.0):
    want = want.detach().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    err = np.abs(np.asarray(got) - want)
    assert (err <= 1e-12 * np.maximum(np.abs(want), floor)).all(), f"{name}: worst {float((err / np.maximum(np.abs(want), 1e-300)).max()):.3g} relative"


@pytest.mark.parametrize("name,kind,param", CRITERIA, ids=[c[0] for c in CRITERIA])
def test_reference_backward_is_autograd_of_its_forward(problem, name, kind, param):
    """Values to 1e-12 relative.  Gradients to 1e-12 of max(|gradient|, its magnitude -- a small multiple of the sum of its terms' absolute
    values): autograd sums the same terms in another order, image_out - target cancels in both, and behind an opaque surface the suffix
    does.  (1e-12 of the magnitude is 2e-5 of the fp32 tolerance built on it.)"""
    p = problem
    M = p["M"]["exact"] if kind == cf.L1 else p["M"]["slack"]
    for scale in (1.0, 1024.0):
        want, got = _autograd(p, M, kind, param, scale), cf.step_reference(p, M, kind, param, scale)
        for k in ("weights_sum", "depth", "image", "image_out", "depth_out", "loss", "scaled_loss"):
            _close(f"{name} {k}", got[k], want[k])
        _close(f"{name} grad_rgbs", got["grad_rgbs"], want["grad_rgbs"], got["grad_rgbs_mag"])
        _close(f"{name} grad_sigmas", got["grad_sigmas"], want["grad_sigmas"], got["grad_sigmas_mag"])
        assert (got["grad_sigmas"][~cf.covered_rows(p, M)] == 0).all() and (got["grad_rgbs"][~cf.covered_rows(p, M)] == 0).all()


def test_reference_backward_with_given_gradients_is_autograd(problem):
    p = problem
    M = p["M"]["cut"]
    want = _autograd(p, M, 0, 0.0, 1.0, given=(p["g_ws"], p["g_img"]))
    got = cf.backward_reference(p, M, p["g_img"], p["g_ws"])
    _close("grad_rgbs", got["grad_rgbs"], want["grad_rgbs"], got["grad_rgbs_mag"])
    _close("grad_sigmas", got["grad_sigmas"], want["grad_sigmas"], got["grad_sigmas_mag"])
    assert np.abs(got["grad_sigmas"]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------- acceptance
def _masks(p, M, kind, want):
    if kind != cf.L1:
        return None
    ambiguous = np.abs(want["d"]) < 1e-6
    assert ambiguous.mean() < 0.01
    return cf.l1_row_mask(p, M, ambiguous)


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), max(r.values()))


@pytest.mark.parametrize("name,kind,param", CRITERIA, ids=[c[0] for c in CRITERIA])
@pytest.mark.parametrize("variant", VARIANTS)
def test_the_bound_accepts_both_emulations(problem, variant, name, kind, param):
    """The serial walk of the reference and the 64-lane tree walk, in float32 with numpy's float32 exp, within HALF the tolerance on every
    output, for every M variant, every criterion, with and without a loss scale."""
    p, M = problem, problem["M"][variant]
    for scale in (1.0, 1024.0):
        want = cf.step_reference(p, M, kind, param, scale)
        mask = _masks(p, M, kind, want)
        for who, got in (("tree walk", cf.emulate_tree(p, M, kind, param, scale)), ("serial walk", cf.emulate_serial(p, M, kind, param, scale))):
            r = cf.ratios(got, want, skip_l1=mask)
            _note(who, r)
            assert max(r.values()) <= 0.5, f"{who}, {variant}, {name}, scale {scale}: {r}"
            dead = ~cf.alive(p, M)
            assert (got["weights_sum"][p["rays"][dead, 0]] == 0).all() and (got["grad_sigmas"][~cf.covered_rows(p, M)] == 0).all()


def test_the_bound_accepts_both_emulations_of_the_plain_backward(problem):
    p, M = problem, problem["M"]["slack"]
    want = cf.backward_reference(p, M, p["g_img"], p["g_ws"])
    for who, got in (("tree walk", cf.emulate_tree(p, M, given=(p["g_ws"], p["g_img"]))), ("serial walk", cf.emulate_serial(p, M, given=(p["g_ws"], p["g_img"])))):
        r = cf.ratios(got, want, groups=("grad_sigmas", "grad_rgbs"))
        _note(who + ", given gradients", r)
        assert max(r.values()) <= 0.5, f"{who}: {r}"


def test_numpy_float32_exp_stays_within_the_whole_tolerance(problem):
    """The same two walks over numpy's own float32 exp loop, which is off by up to 2.4 ulp where the model assumes 1 for the hardware:
    beyond half the tolerance (grad_rgbs of thin samples, where 1 - exp(-x) cancels and the exponential's error is all there is), within
    the whole of it."""
    p, M = problem, problem["M"]["slack"]
    want = cf.step_reference(p, M)
    for who, got in (("tree walk", cf.emulate_tree(p, M, exp=cf.exp32_native)), ("serial walk", cf.emulate_serial(p, M, exp=cf.exp32_native))):
        r = cf.ratios(got, want)
        _note(who + ", numpy float32 exp loop", r)
        assert max(r.values()) <= 1.0, f"{who}: {r}"


def test_the_kept_chunks_do_not_change_the_tree_walk(problem):
    """keep = 1, 3, 4 against 2: a walk restarted from the state at `keep` repeats the bits of the walk that was kept"""
    p, M = problem, problem["M"]["slack"]
    base = cf.emulate_tree(p, M, keep=2)
    for keep in (1, 3, 4):
        got = cf.emulate_tree(p, M, keep=keep)
        for k in base:
            assert np.array_equal(base[k].view(np.int32), got[k].view(np.int32)), (keep, k)


# ----------------------------------------------------------------------------------------------------------------------- rejection
@pytest.mark.parametrize("mutation", cf.MUTATIONS)
def test_the_bound_rejects_a_wrong_walk(problem, mutation):
    """Each mutation of the tree walk lands beyond the tolerance on at least one output (at every `keep` it applies to)."""
    p, M = problem, problem["M"]["slack"]
    kind, param = (cf.HUBER, 0.1) if mutation == "huber_l1" else (cf.MSE, 0.0)
    want = cf.step_reference(p, M, kind, param, 1.0)
    for keep in ((1, 2, 3, 4) if mutation == "fresh_restart" else (2,)):
        r = cf.ratios(cf.emulate_tree(p, M, kind, param, 1.0, keep=keep, mutate=mutation), want)
        print(mutation, keep, {k: f"{v:.3g}" for k, v in r.items()})
        assert max(r.values()) > 1.0, f"{mutation} (keep {keep}) passes the bound: {r}"
