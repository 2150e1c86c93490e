"""The float64 host model of the texture synthesis (tests/synthesis_model.py) against the reference's own class, run on the CPU for
tests/golden/ref_python_synthesis.npz (tools/make_golden.py: synthesis_goldens): case A (P=40, S=12, block 3 exact, no mirrors) and case B (P=24,
S=13, the last block partial, both mirrors, a patch_length at which the close-patch filter bites)."""
import numpy as np
import pytest

import synthesis_cases as sc
import synthesis_model as sm

CASES = ("A", "B")


def _ragged(g, name, key):
    counts = g[name + "_survivor_counts"]
    return np.split(g[name + "_" + key], np.cumsum(counts)[:-1])


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("forced", (True, False), ids=("forced", "free"))
def test_model_reproduces_the_reference(name, forced):
    g, c, run = sc.fixture(), sc.case_inputs(name), sc.model_run(name, forced)
    n = run["n"]
    assert n == 4 and run["examples"] == c["examples"] and run["block"] == c["block"] == 3
    assert (run["patch_size"], run["overlap_size"]) == (c["patch_size"], c["overlap_size"])
    survivors, distances, probs = (_ragged(g, name, k) for k in ("survivors", "distances", "probabilities"))
    for cell in range(1, n * n):
        m = run["cells"][cell]
        assert m["k"] == g[name + "_k"][cell - 1], cell
        assert np.array_equal(m["survivors"], survivors[cell - 1]), cell  # the same set, in the same order
        assert np.abs(m["survivor_dist"] / distances[cell - 1] - 1).max() < 1e-12, cell
        assert np.abs(m["probabilities"] - probs[cell - 1]).max() < 1e-12, cell
        assert m["drawn"] == g[name + "_chosen"][cell - 1] == m["placed"], cell
    assert np.array_equal(run["id_map"], g[name + "_id_map"])
    assert np.array_equal(run["canvas_id"], g[name + "_canvas_id"])
    assert np.array_equal(run["sample_tbn_ids"], g[name + "_sample_tbn_ids"]) and np.array_equal(run["total_id"], g[name + "_total_id"])
    assert np.array_equal(run["sample_tbn"], g[name + "_sample_tbn"])
    assert run["canvas"].dtype == g[name + "_canvas"].dtype == np.float64
    assert np.abs(run["canvas"] - g[name + "_canvas"]).max() < 1e-12


@pytest.mark.parametrize("name", CASES)
def test_draws_are_the_seeded_stream(name):
    c, run = sc.case_inputs(name), sc.model_run(name, False)
    assert np.array_equal(run["draws"], np.random.RandomState(c["seed"]).random_sample(15))


def test_fixture_shapes_and_paths():
    g = sc.fixture()
    a, b = sc.case_inputs("A"), sc.case_inputs("B")
    assert a["patches"].shape == (40, 12, 12, 33) and not a["mirrors"] and a["examples"] == 40 and g["A_canvas"].shape == (33, 33, 33)
    assert b["patches"].shape == (24, 13, 13, 33) and b["mirrors"] and b["examples"] == 96 and g["B_canvas"].shape == (37, 37, 33)
    assert a["first_patch"] < 40 and b["first_patch"] < 96
    assert a["patches"].dtype == np.float32
    # B: the filter bites, at least one cell doubles k and none runs past the example set; a single survivor takes the NaN -> uniform path
    assert (g["B_k"] > 16).any() and g["B_k"].max() <= 96
    assert (g["B_survivor_counts"] < 16).all() and (g["B_survivor_counts"] == 1).any()
    single = int(np.flatnonzero(g["B_survivor_counts"] == 1)[0])
    assert _ragged(g, "B", "probabilities")[single].tolist() == [1.0]
    assert (g["A_k"] == 16).all() and (g["A_survivor_counts"] == 16).all()  # no mirror: no filter
    mirrored = g["B_id_map"].reshape(-1) >= 24
    assert mirrored.any(), "a mirrored example is placed"


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("forced", (True, False), ids=("forced", "free"))
def test_margins_clear_the_device_bounds(name, forced):
    """The cap of the GPU test, on the model alone: at most one of the 15 cells is within the derived bounds of deciding differently."""
    und = sc.undecided_cells(name, forced)
    assert len(und) <= sc.MAX_UNDECIDED, und
    run = sc.model_run(name, forced)
    ties = sum(c["dp_ties"] for c in run["cells"][1:])
    total = sum(c["dp_decisions"] for c in run["cells"][1:])
    assert 0 < ties < 0.15 * total  # exact ties exist (zero errors where the patch already is the canvas) and are the minority


def test_k_past_the_example_set_is_an_error():
    c = sc.case_inputs("B")
    with pytest.raises(sm.KExceedsExamples):
        sm.synthesize(c["patches"], c["sample_tbn"], c["picked_vertices"], 1e3, c["output"], **sc.model_kwargs(c))


def test_flip_order_and_frames_of_the_example_set():
    rng = np.random.default_rng(0)
    p, t = rng.normal(size=(3, 4, 4, 2)), rng.normal(size=(3, 9))
    ex, tbn = sm.example_set(p, t, True, True)
    assert ex.shape[0] == 12 and np.array_equal(ex[3:6], p[:, ::-1]) and np.array_equal(ex[6:9], p[:, :, ::-1]) and np.array_equal(ex[9:], p[:, ::-1, ::-1])
    t3 = t.reshape(3, 3, 3)
    assert np.array_equal(tbn[4].reshape(3, 3)[:, 0], -t3[1][:, 0]) and np.array_equal(tbn[7].reshape(3, 3)[:, 1], -t3[1][:, 1])
    assert np.array_equal(tbn[10].reshape(3, 3)[:, :2], -t3[1][:, :2]) and np.array_equal(tbn[10].reshape(3, 3)[:, 2], t3[1][:, 2])
    assert sm.default_sizes(128) == (32, 48) and sm.default_sizes(12) == (2, 5) and sm.default_sizes(13) == (3, 5)
    assert sm.canvas_cells(2048, 32, 48) == (25, 25 * 32 + 26 * 48)
