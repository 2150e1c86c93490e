"""Float64 host model of the patch-based texture synthesis (`ngp_harness.synthesis`, csrc/synthesis.inc): the path the reference's
patch_matching_and_quilting.py runs -- mode 'Cut', no quilting, coarse strips, no rotation, the close-patch filter over picked_vertices --
restated in numpy with brute-force distances (no KD-tree, no skimage).  It takes the same draws, first patch and forced ids as the device
path and reports, per decision, how far it was from going the other way:

  rank     the relative gap (d[r+1] - d[r]) / d[r+1] at every rank boundary that mattered: between the k ranked examples and to the first one
           that was left out
  draw     |u - nearest cdf edge|
  dp       per dynamic-program minimum (every window minimum and the trace's start) the gap between the best and the second-best value,
           relative (to the second best) and absolute.  Exact ties have gap 0: they are decided by the first-index rule on both sides, since
           they come from exactly equal copies (mostly zero errors where the patch already is the canvas), and are not counted as close calls.
"""
import math

import numpy as np


def example_set(patches, sample_tbn, mirror_hor, mirror_vert):
    """-> (examples [E,S,S,C], example_tbn [E,9]): the patches, then their row-flipped copies, then the column-flipped copies of all of those."""
    ex = np.asarray(patches, dtype=np.float64)
    tbn = np.asarray(sample_tbn, dtype=np.float64).reshape(-1, 3, 3)
    if mirror_hor:
        ex = np.concatenate([ex, ex[:, ::-1]])
        flip = tbn.copy()
        flip[..., 0] *= -1
        tbn = np.concatenate([tbn, flip])
    if mirror_vert:
        ex = np.concatenate([ex, ex[:, :, ::-1]])
        flip = tbn.copy()
        flip[..., 1] *= -1
        tbn = np.concatenate([tbn, flip])
    return ex, tbn.reshape(-1, 9)


def default_sizes(S):
    """The script's patch and overlap size for S-pixel patches."""
    ps = int(S / 4)
    if (S - ps) % 2 == 1:
        ps -= 1
    return ps, (S - ps) // 2


def canvas_cells(output_size, ps, ov):
    n = int(math.ceil((output_size - ov) / (ps + ov)))
    return n, n * ps + (n + 1) * ov


def block_sum(a, block, axis):
    """skimage's block_reduce with its defaults along one axis: zero-padded to a multiple of `block`, summed."""
    a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, 0)
    pad = (-a.shape[0]) % block
    if pad:
        a = np.concatenate([a, np.zeros((pad,) + a.shape[1:])])
    a = a.reshape((a.shape[0] // block, block) + a.shape[1:]).sum(axis=1)
    return np.moveaxis(a, 0, axis)


def probabilities(d, attenuation):
    """distances2probability with PARM_truncation = 0, over the survivors' distances."""
    with np.errstate(invalid="ignore", divide="ignore"):
        p = 1 - d / np.max(d)
        p /= np.sum(p)
        p *= (p > 0.0)
        p = pow(p, attenuation)
        p /= np.sum(p)
    if np.isnan(p).any():
        p = np.ones_like(p) / p.shape[0]
    return p


class KExceedsExamples(Exception):
    """The filter removed every candidate and the next k is larger than the example set (sklearn raises here)."""

    def __init__(self, cell, k):
        super().__init__(f"cell {cell}: k = {k} exceeds the example set")
        self.cell, self.k = cell, k


def _gaps(vals):
    """(first index of the minimum, relative gap, absolute gap) of a window of float64 values; one value: infinite gaps."""
    j = int(np.argmin(vals))
    if len(vals) == 1:
        return j, math.inf, math.inf
    rest = np.delete(vals, j)
    second = float(rest.min())
    gap = second - float(vals[j])
    return j, (gap / second if second != 0 else 0.0), gap


def min_err_cut(B1, B2, match_dim, margins):
    """MinErrBouCut without quilting: -> (B, mask [H,W] True left of the trace, trace [H]).  `margins` collects (relative, absolute) gaps."""
    H, W = B1.shape[:2]
    e = ((B1[..., :match_dim] - B2[..., :match_dim]) ** 2).sum(axis=-1)
    E = np.zeros_like(e)
    E[0] = e[0]
    T = np.zeros(e.shape, dtype=np.int64)
    T[0] = np.arange(W)
    for i in range(1, H):
        for j in range(W):
            lo, hi = max(0, j - 1), min(j + 1, W - 1)
            k, rel, ab = _gaps(E[i - 1, lo:hi + 1])
            margins.append((rel, ab))
            E[i, j] = e[i, j] + E[i - 1, lo + k]
            T[i, j] = lo + k
    dest, rel, ab = _gaps(E[-1])
    margins.append((rel, ab))
    trace = np.zeros(H, dtype=np.int64)
    trace[-1] = dest
    for i in range(2, H + 1):
        trace[-i] = T[-i + 1, trace[-i + 1]]
    B = np.zeros_like(B1)
    mask = np.zeros((H, W), dtype=bool)
    for i in range(H):
        t = trace[i]
        B[i, :t] = B1[i, :t]
        B[i, t:] = B2[i, t:]
        B[i, t] = (B1[i, t] + B2[i, t]) / 2
        mask[i, :t] = True
    return B, mask, trace


def synthesize(patches, sample_tbn, picked_vertices, patch_length, output_size, *, match_dim, patch_size=None, overlap_size=None, mirror_hor=False,
               mirror_vert=False, strict_match=True, close_threshold=0.2, max_patch_res=32, first_patch=0, draws=None, forced=None, stop_after=None):
    """-> dict.  patches [P,S,S,C]; draws [n*n - 1], one per cell behind the first; forced [n*n] or None (the placed ids; what the draw would
    have picked is still recorded).  stop_after: resolve only the cells below this index."""
    ex, ex_tbn = example_set(patches, sample_tbn, mirror_hor, mirror_vert)
    P, E, S, C = np.asarray(patches).shape[0], ex.shape[0], ex.shape[1], ex.shape[3]
    ps, ov = default_sizes(S)
    ps = ps if patch_size is None else int(patch_size)
    ov = ov if overlap_size is None else int(overlap_size)
    assert ps + 2 * ov == S and 0 < match_dim <= C and 0 <= first_patch < E
    n, side = canvas_cells(output_size, ps, ov)
    block = max(int(S / max_patch_res), 1)
    att = 3 if strict_match else 1
    db_top = block_sum(ex[:, :ov, :, :match_dim], block, 2).reshape(E, -1)
    db_left = block_sum(ex[:, :, :ov, :match_dim], block, 1).reshape(E, -1)
    pv = np.asarray(picked_vertices, dtype=np.float64)
    vdist = ((pv[None] - pv[:, None]) ** 2).sum(axis=-1) ** .5
    limit = close_threshold * patch_length
    canvas = np.zeros((side, side, C))
    canvas_id = -np.ones((side, side), dtype=np.int64)
    averaged = np.zeros((side, side), dtype=bool)  # pixels whose value went through a seam's mean
    id_map = -np.ones(n * n, dtype=np.int64)
    canvas[:S, :S] = ex[first_patch]
    canvas_id[:S, :S] = first_patch
    id_map[0] = first_patch
    cells = [None]
    draws = np.zeros(n * n - 1) if draws is None else np.asarray(draws, dtype=np.float64)
    for cell in range(1, n * n if stop_after is None else stop_after):
        r, c = cell // n, cell % n
        y0, x0 = (ps + ov) * r, (ps + ov) * c
        region = canvas[y0:y0 + S, x0:x0 + S]
        d2 = np.zeros(E)
        qnorm2 = 0.0
        if r > 0:
            q = block_sum(region[:ov, :, :match_dim], block, 1).reshape(-1)
            d2 += ((db_top - q) ** 2).sum(axis=1)
            qnorm2 += float((q ** 2).sum())
        if c > 0:
            q = block_sum(region[:, :ov, :match_dim], block, 0).reshape(-1)
            d2 += ((db_left - q) ** 2).sum(axis=1)
            qnorm2 += float((q ** 2).sum())
        d = np.sqrt(d2)
        order = np.lexsort((np.arange(E), d))
        k = 16
        while True:
            if k > E:
                raise KExceedsExamples(cell, k)
            ind, dist = order[:k], d[order[:k]]
            keep = np.ones(k, dtype=bool)
            if mirror_hor or mirror_vert:
                if r > 0:
                    keep &= ~(vdist[ind % P, id_map[cell - n] % P] < limit)
                if c > 0:
                    keep &= ~(vdist[ind % P, id_map[cell - 1] % P] < limit)
            if keep.any():
                break
            k *= 2
        ranked = d[order[:min(k + 1, E)]]
        rank_margin = float(np.min((ranked[1:] - ranked[:-1]) / ranked[1:])) if len(ranked) > 1 else math.inf
        surv, sd = ind[keep], dist[keep]
        p = probabilities(sd, att)
        cdf = np.cumsum(p)
        cdf /= cdf[-1]
        u = draws[cell - 1]
        drawn = int(surv[min(int(np.searchsorted(cdf, u, side="right")), len(surv) - 1)])
        with np.errstate(invalid="ignore", divide="ignore"):
            raw = float(np.sum((1 - sd / np.max(sd)) ** att))
            raw_prev = float(np.sum((1 - sd / np.max(sd)) ** (att - 1)))
        placed = drawn if forced is None else int(forced[cell])
        # the placement: the left cut, then the top cut on the patch as the left cut left it
        patch = ex[placed].copy()
        pid = np.full((S, S), placed, dtype=np.int64)
        avg, was = np.zeros((S, S), dtype=bool), averaged[y0:y0 + S, x0:x0 + S]
        dp = []
        traces = {}
        if c > 0:
            B, mask, traces["left"] = min_err_cut(region[:, :ov], patch[:, :ov].copy(), match_dim, dp)
            patch[:, :ov] = B
            pid[:, :ov] = np.where(mask, canvas_id[y0:y0 + S, x0:x0 + ov], pid[:, :ov])
            avg[:, :ov] = mask & was[:, :ov]
            avg[np.arange(S), traces["left"]] = True
        if r > 0:
            B, mask, traces["top"] = min_err_cut(np.moveaxis(region[:ov], 0, 1), np.moveaxis(patch[:ov].copy(), 0, 1), match_dim, dp)
            patch[:ov] = np.moveaxis(B, 0, 1)
            pid[:ov] = np.where(mask.T, canvas_id[y0:y0 + ov, x0:x0 + S], pid[:ov])
            avg[:ov] = np.where(mask.T, was[:ov], avg[:ov])
            avg[traces["top"], np.arange(S)] = True
        canvas[y0:y0 + S, x0:x0 + S] = patch
        canvas_id[y0:y0 + S, x0:x0 + S] = pid
        averaged[y0:y0 + S, x0:x0 + S] = avg
        id_map[cell] = placed
        close = [g for g in dp if g[1] != 0]
        cells.append(dict(
            k=k, ranked_ids=order[:k].copy(), ranked_dist=dist.copy(), survivors=surv.copy(), survivor_dist=sd.copy(), probabilities=p, drawn=drawn,
            placed=placed, draw=float(u), rank_margin=rank_margin, draw_margin=float(np.min(np.abs(cdf[:-1] - u))) if len(cdf) > 1 else math.inf,
            weight_sum=raw, weight_sum_prev=raw_prev, dp_decisions=len(dp), dp_ties=len(dp) - len(close), dp_margin_rel=min((g[0] for g in close), default=math.inf),
            dp_margin_abs=min((g[1] for g in close), default=math.inf), query_norm=math.sqrt(qnorm2), traces=traces))
    total_id = np.sort(np.unique(canvas_id.reshape(-1)))
    done = total_id[0] >= 0
    remap = np.searchsorted(total_id, canvas_id) if done else None
    db_norm = np.sqrt((db_top ** 2).sum(axis=1) + (db_left ** 2).sum(axis=1))
    return dict(canvas=canvas, canvas_id=canvas_id, averaged=averaged, id_map=id_map.reshape(n, n), cells=cells, total_id=total_id, sample_tbn=ex_tbn[total_id] if done else None,
                sample_tbn_ids=remap, n=n, side=side, patch_size=ps, overlap_size=ov, block=block, examples=E, example_tbn=ex_tbn, db_norm_max=float(db_norm.max()),
                draws=draws.copy())
