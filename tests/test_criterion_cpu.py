"""CPU: the training criterion of the accelerated trainers (ngp_harness/accelerate.py parse_criterion, accelerate(criterion=, error_map=)) -- what
is accepted, what is refused and when -- and the descriptor checks of the C entries that take a nerftex_step_loss_desc (they refuse before
anything is launched, so no GPU is needed to see them refuse)."""
import ctypes
import math
import types

import pytest
import torch

from ngp_harness.accelerate import LOSS_KINDS, AcceleratedTrainer, CurvedTrainer, parse_criterion

MSE, L1, HUBER = LOSS_KINDS["mse"], LOSS_KINDS["l1"], LOSS_KINDS["huber"]


def test_kinds_are_the_header_constants():
    import nerftex_hip

    assert (MSE, L1, HUBER) == (nerftex_hip.LOSS_MSE, nerftex_hip.LOSS_L1, nerftex_hip.LOSS_HUBER) == (0, 1, 2)
    d = nerftex_hip.StepLossDesc(HUBER, 0.5, None, None, None, 0, 0.1, 0.9)
    assert ctypes.sizeof(d) == 48 and (d.kind, d.param, d.error_cells) == (2, 0.5, 0)  # the C struct's layout: 4 + 4 + 3 * 8 + 8 + 4 + 4


@pytest.mark.parametrize("spelling,want", [
    ("mse", (MSE, 0.0)), ("l1", (L1, 0.0)), (("huber", 0.1), (HUBER, 0.1)), (("huber", 2), (HUBER, 2.0)),
    (torch.nn.MSELoss(), (MSE, 0.0)), (torch.nn.MSELoss(reduction="none"), (MSE, 0.0)),
    (torch.nn.L1Loss(), (L1, 0.0)), (torch.nn.L1Loss(reduction="none"), (L1, 0.0)),
    (torch.nn.HuberLoss(), (HUBER, 1.0)), (torch.nn.HuberLoss(reduction="none", delta=0.1), (HUBER, 0.1)),
    ((MSE, 0.0), (MSE, 0.0)), ((L1, 0.0), (L1, 0.0)), ((HUBER, 0.25), (HUBER, 0.25)),  # already parsed: what the trainer hands to the tail
], ids=lambda v: repr(v)[:40])
def test_accepted_spellings(spelling, want):
    got = parse_criterion(spelling)
    assert got == want and isinstance(got[0], int) and isinstance(got[1], float)


def _ident(v):
    """a test id that is the same in every process: a function's repr carries its address"""
    return f"<function {v.__name__}>" if isinstance(v, (types.FunctionType, types.BuiltinFunctionType)) else repr(v)[:40]


REFUSED = [
    "huber", "L1", "smooth_l1", "", None, 1, ("huber",), ("huber", 0), ("huber", 0.0), ("huber", -1.0), ("huber", math.inf), ("huber", math.nan),
    ("huber", "0.1"), ("huber", True), ("l1", 0.0), (7, 0.0), (HUBER, 0.0),
    torch.nn.MSELoss(reduction="sum"), torch.nn.L1Loss(reduction="sum"), torch.nn.HuberLoss(reduction="sum"), torch.nn.SmoothL1Loss(),
    torch.nn.BCELoss(), torch.nn.functional.l1_loss, lambda a, b: (a - b).abs().mean(), torch.nn.L1Loss,
]


@pytest.mark.parametrize("spelling", REFUSED, ids=_ident)
def test_refused_spellings(spelling):
    with pytest.raises(ValueError, match="criterion: .*mse.*l1.*huber.*MSELoss.*reduction"):
        parse_criterion(spelling)


@pytest.mark.parametrize("spelling", ["huber", torch.nn.L1Loss(reduction="sum"), torch.nn.functional.mse_loss, ("huber", 0)], ids=_ident)
def test_trainers_refuse_before_the_renderer_is_looked_at(spelling):
    nothing = types.SimpleNamespace(field=None)
    for cls in (AcceleratedTrainer, CurvedTrainer):
        with pytest.raises(ValueError, match="criterion: "):
            cls(nothing, criterion=spelling)
        with pytest.raises(ValueError, match="error_map: a contiguous float32"):
            cls(nothing, criterion="l1", error_map=torch.zeros(4, 4, dtype=torch.float64))
        with pytest.raises(ValueError, match="error_map: a contiguous float32"):
            cls(nothing, error_map=torch.zeros(4, 4).t())


@pytest.mark.parametrize("kw", [dict(criterion="l1"), dict(criterion=("huber", 0.1)), dict(criterion=torch.nn.L1Loss()), dict(error_map=torch.zeros(8, 8)),
                                dict(criterion="mse", error_map=torch.zeros(64))], ids=lambda v: repr(sorted(v))[:40])
def test_accepted_arguments_get_past_the_refusal(kw):
    nothing = types.SimpleNamespace(field=None)
    for cls in (AcceleratedTrainer, CurvedTrainer):
        with pytest.raises(AssertionError, match="field|CurvedField"):  # (the renderer is looked at, and is no renderer)
            cls(nothing, **kw)


def test_error_inds_without_a_map_are_refused():
    from ngp_harness import fused

    inds = torch.arange(8)
    with pytest.raises(ValueError, match="error_map and error_inds go together"):
        fused.step_loss_desc("l1", None, None, inds, 8, inds.device)
    with pytest.raises(ValueError, match="error_map and error_inds go together"):
        fused.step_loss_desc(None, None, torch.zeros(16), None, 8, inds.device)
    with pytest.raises(ValueError, match="error_inds: a contiguous torch.int64"):
        fused.step_loss_desc(None, None, torch.zeros(16), inds.int(), 8, inds.device)
    with pytest.raises(ValueError, match="ray_loss: a contiguous torch.float32"):
        fused.step_loss_desc("l1", torch.zeros(9), None, None, 8, inds.device)
    assert fused.step_loss_desc(None, None, None, None, 8, inds.device) is None, "nothing asked for: the MSE entries, as ever"
    d = fused.step_loss_desc(("huber", 0.5), torch.zeros(8), torch.zeros(4, 4), inds, 8, inds.device)
    assert (d.kind, d.param, d.error_cells, d.keep, d.take) == (HUBER, 0.5, 16, ctypes.c_float(0.1).value, ctypes.c_float(0.9).value)
    # the trainer's step: refused before any buffer is made
    tr = AcceleratedTrainer.__new__(AcceleratedTrainer)
    tr.renderer, tr.error_map = types.SimpleNamespace(), None
    rays = torch.zeros(1, 8, 3)
    with pytest.raises(ValueError, match="error_inds without a map"):
        tr._steps(rays, rays, rays, None, inds.reshape(1, 8))


@pytest.mark.parametrize("bad,message", [
    (dict(kind=7), "unknown criterion kind 7"),
    (dict(kind=HUBER, param=0.0), "finite delta > 0"),
    (dict(kind=HUBER, param=math.inf), "finite delta > 0"),
    (dict(kind=HUBER, param=math.nan), "finite delta > 0"),
    (dict(kind=L1, error_map=1 << 20), "error_map and error_inds go together"),
    (dict(kind=L1, error_inds=1 << 20), "error_map and error_inds go together"),
], ids=lambda v: repr(v)[:40])
def test_the_c_entries_refuse_a_bad_descriptor_before_launching(bad, message):
    """NERFTEX_ERR_INVALID with a message; the pointers handed over here are never dereferenced (nothing is launched)."""
    from nerftex_hip import StepLossDesc, lib

    desc = StepLossDesc(bad.get("kind", 0), bad.get("param", 0.0), None, bad.get("error_map"), bad.get("error_inds"), 16, 0.1, 0.9)
    by = ctypes.byref(desc)
    forward = "error_map" in message
    calls = [
        (lib.nerftex_composite_step_ex, (None, None, None, None, 128, 4, None, None, None, 1.0, 1.0, None, None, None, None, None, None, None, None, None, None, None, None)),
        (lib.nerftex_render_tail_forward_ex, (None, None, None, None, None, None, 1.0, 1.0, 4, None, None, None, None, None, None, None, None, 0)),
    ]
    if not forward:  # (the two backward entries read kind and param only)
        calls += [
            (lib.nerftex_composite_tail_backward_ex, (None, None, 1.0, None, None, 1.0, None, None, None, None, None, None, 128, 4, None, None, None)),
            (lib.nerftex_render_tail_backward_ex, (None, None, 1.0, None, None, 1.0, 4, None, None)),
        ]
    for fn, args in calls:
        assert fn(*args, by, None) == 1, fn.__name__  # NERFTEX_ERR_INVALID
        assert message in lib.nerftex_last_error().decode(), lib.nerftex_last_error().decode()
