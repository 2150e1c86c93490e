"""The tuning knobs (nerftex_tune_set / nerftex_tune_get, CPU only): the names include/nerftex_hip.h lists are the names the library knows -- both
come from the one list in csrc/common.hpp -- and the knobs of the retired A/B forms are gone."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex_hip.h")
RETIRED = ("ffmlp_bwd_tr", "planar_lanes", "patch_lanes")


def _listed_names():
    """The "Names:" sentence of the nerftex_tune_set comment: from "Names:" to the parenthesis that closes the list."""
    text = re.search(r"Names:(.*?)\(", open(HEADER).read(), re.S).group(1)
    return [n for n in re.split(r"[\s,*]+", text) if n]


def test_every_name_the_header_lists_is_a_knob_with_default_zero():
    from nerftex_hip import lib

    names = _listed_names()
    assert len(names) == len(set(names)) >= 15 and all(re.fullmatch(r"[a-z][a-z0-9_]*", n) for n in names), names
    for n in names:
        assert lib.nerftex_tune_get(n.encode()) == 0, n
    assert not set(RETIRED) & set(names)


@pytest.mark.parametrize("name", RETIRED + ("no_such_knob",))
def test_retired_and_made_up_names_are_unknown(name):
    from nerftex_hip import ERR_INVALID, lib

    assert lib.nerftex_tune_set(name.encode(), 1) == ERR_INVALID
    assert lib.nerftex_tune_get(name.encode()) == -1


def test_tune_sets_and_restores_also_when_the_body_raises():
    import nerftex_hip

    get = lambda: nerftex_hip.lib.nerftex_tune_get(b"march_serial")  # noqa: E731
    assert get() == 0
    with nerftex_hip.tune(march_serial=1):
        assert get() == 1
    assert get() == 0
    with pytest.raises(KeyError):
        with nerftex_hip.tune(march_serial=1):
            assert get() == 1
            raise KeyError("from the body")
    assert get() == 0
