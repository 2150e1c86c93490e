"""CPU: the options both accelerated trainers refuse at construction (ngp_harness/accelerate.py) -- the removed `pipeline_adam` keyword."""
import types

import pytest

from ngp_harness.accelerate import AcceleratedTrainer, CurvedTrainer, _refuse_options


@pytest.mark.parametrize("value", [4, 1, True])
def test_pipeline_adam_is_refused_without_a_schedule_too(value):
    nothing = types.SimpleNamespace(field=None)  # (refused before the renderer is looked at)
    for cls in (AcceleratedTrainer, CurvedTrainer):
        with pytest.raises(ValueError, match="pipeline_adam.*removed.*DESIGN_HISTORY.md"):
            cls(nothing, pipeline_adam=value)


@pytest.mark.parametrize("value", [0, None, False])
def test_pipeline_adam_off_is_accepted_and_ignored(value):
    _refuse_options(None, value)
    nothing = types.SimpleNamespace(field=None)
    for cls in (AcceleratedTrainer, CurvedTrainer):
        with pytest.raises(AssertionError, match="field|CurvedField"):  # (past the refusal: the renderer is looked at, and is no renderer)
            cls(nothing, pipeline_adam=value)
