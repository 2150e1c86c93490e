"""The two cases of tests/golden/ref_python_synthesis.npz (tools/make_golden.py: synthesis_goldens), the host model's run of each -- computed once and
shared, never modified -- and the bounds under which a decision of the float64 model may come out differently on the device.

What differs on the device (csrc/synthesis.inc), and nothing else: the coarse databases are stored in fp32 (each entry within 2^-24 relative of the
float64 block sum), and a canvas pixel that was averaged on a seam is allowed 2 fp32 ulp = 2^-22 relative of the float64 value (the contract's
bound; the device keeps the mean's residual beside the canvas and comes closer).  Every sum is accumulated in float64 (its own rounding, ~1e-16 a
term, is left out below).

  distance   d = |q - db|.  By the triangle inequality |d' - d| <= |db' - db| + |q' - q| <= 2^-24 |db| + 2^-22 |q|, so the relative error of a
             cell's distances is at most  rho = (2^-24 max|db| + 2^-22 |q|) / min d.  Two ranked distances can swap if their relative gap is
             below 2 rho (both move).
  draw       the cdf entries are sums of w_i / Z with w_i = x_i^a, x_i = 1 - d_i / d_max, Z = sum w.  |delta x_i| <= 2 rho, so
             |delta w_i| <= 2 a rho x_i^(a-1) and every partial sum, Z included, moves by at most D = 2 a rho sum x_i^(a-1); an entry
             c = (partial sum) / Z <= 1 moves by at most (D + c D) / Z <= 4 a rho sum x^(a-1) / sum x^a.  One survivor: nothing is drawn.
  dp         a window compares accumulated energies, each a sum of at most H per-pixel errors e = sum over match_dim channels of (c - p)^2.  The
             patch side p is exact (the left cut's mean is formed in float64 on both sides); a canvas value moves by at most 2^-22 v, v = max|value|,
             and |c - p| <= 2 v, so |delta e| <= match_dim 2 (2 v) 2^-22 v = match_dim 2^-20 v^2, and the gap between two energies moves by at most
             2 H match_dim 2^-20 v^2 (absolute).  An exact tie (gap 0) is decided by the first-index rule on both sides.
"""
import functools
import os

import numpy as np

import synthesis_model as sm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_python_synthesis.npz")
OPTIONS = ("match_dim", "phi_dim", "max_patch_res", "mirrors", "output", "seed", "patch_size", "overlap_size", "block", "examples")
MAX_UNDECIDED = 1  # of the 15 cells of a case


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case_inputs(name):
    g = fixture()
    o = dict(zip(OPTIONS, (int(v) for v in g[name + "_options"])))
    return dict(patches=g[name + "_patches"], sample_tbn=g[name + "_sample_tbn_in"], picked_vertices=g[name + "_picked_vertices"],
                patch_length=float(g[name + "_patch_length"]), first_patch=int(g[name + "_first_patch"]), draws=g[name + "_draws"],
                forced=g[name + "_id_map"].reshape(-1).astype(np.int64), **o)


def model_kwargs(c):
    return dict(match_dim=c["match_dim"], mirror_hor=bool(c["mirrors"]), mirror_vert=bool(c["mirrors"]), strict_match=True, close_threshold=0.2,
                max_patch_res=c["max_patch_res"], first_patch=c["first_patch"], draws=c["draws"])


@functools.lru_cache(maxsize=None)
def model_run(name, forced):
    """The host model on a fixture case, with the reference's choices forced or with the draws alone."""
    c = case_inputs(name)
    return sm.synthesize(c["patches"], c["sample_tbn"], c["picked_vertices"], c["patch_length"], c["output"], forced=c["forced"] if forced else None,
                         **model_kwargs(c))


def distance_bound(run, cell):
    """rho of the module docstring for one cell of a model run."""
    c = run["cells"][cell]
    return (2.0 ** -24 * run["db_norm_max"] + 2.0 ** -22 * c["query_norm"]) / float(c["ranked_dist"].min())


def undecided(run, cell, S, match_dim, vmax, strict_match=True):
    """-> the list of reasons ('rank', 'draw', 'dp') for which the device may decide this cell differently from the model."""
    c = run["cells"][cell]
    rho = distance_bound(run, cell)
    why = []
    if c["rank_margin"] < 2 * rho:
        why.append("rank")
    n = len(c["survivors"])
    if n > 1 and c["weight_sum"] > 0 and c["draw_margin"] < 4 * (3 if strict_match else 1) * rho * c["weight_sum_prev"] / c["weight_sum"]:
        why.append("draw")
    if c["dp_margin_abs"] < 2 * S * match_dim * 2.0 ** -20 * vmax * vmax:
        why.append("dp")
    return why


def undecided_cells(name, forced):
    c, run = case_inputs(name), model_run(name, forced)
    S, vmax = c["patches"].shape[1], float(np.abs(c["patches"]).max())
    return {cell: why for cell in range(1, run["n"] ** 2) if (why := undecided(run, cell, S, c["match_dim"], vmax))}
