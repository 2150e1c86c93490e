"""TEST INFRASTRUCTURE: a float64 restatement of the training compositing (forward, render tail, criterion, backward) with the magnitude
every value's fp32 error scales with, for tests/test_gpu_composite_float64.py (checked on the CPU by tests/test_composite_float64_cpu.py).
Plain numpy, no GPU import.  Also here: the one ragged problem both test modules use (ladder_problem) and two float32 emulations of the
walk -- the serial one of the reference's kernels and the 64-lane tree walk with chunk carry of csrc/raymarching.hip -- which exist to
check the bound, not to be compared with the GPU.

The operation (float64, from the float32 inputs; per ray of n samples at rows offset .. offset + n - 1, straightforward cumprod / cumsum):
    x_i = sigma_i delta_i0,  f_i = exp(-x_i),  alpha_i = 1 - f_i,  T_i = prod_{j<i} f_j,  w_i = alpha_i T_i,  t_i = sum_{j<=i} delta_j1
    weights_sum = sum w_i,  image_c = sum w_i c_i,  depth = sum w_i t_i            (zeros when n == 0 or offset + n >= M: a dead ray)
    image_out_c = image_c + (1 - weights_sum) bg,  depth_out = max(depth - near, 0) / (far - near)
    err = sum_c e(image_out_c - target_c),  e = d^2 | |d| | Huber_delta(d)  (kinds 0 / 1 / 2 of step_loss.hpp)
    loss = sum_rays err / 3N * loss_mul,  scaled_loss = loss * scale
    gi_c = d scaled_loss / d image_c = scale loss_mul e'(d_c) / 3N,   gws = -(sum_c gi_c) bg
    grad_rgb_ic = gi_c w_i
    grad_sigma_i = delta_i0 [ sum_c gi_c (T_{i+1} c_i - S_c(i)) + gws (T_{i+1} - S_ws(i)) ],  S(i) = sum_{j>i} terms   (the suffix)
Rows of dead rays and rows no ray covers have zero gradients.  The suffix sums are formed here by a reversed cumsum, not as total - running.

THE ERROR MODEL.  u = 2^-24.  Every magnitude below is a first-order bound on the fp32 error of the tree walk in units of u: each rounding
of the walk enters once, at its worst case (u times the absolute value of what is rounded).

  factor.  The kernels form alpha = 1 - exp(-sigma delta0) and f = 1 - alpha.  The product sigma delta0 rounds (relative u: moves the
      exponential by u x f), the exponential itself is off by E ulps of f (E u f, taking an ulp of f in [1/2, 1) as the unit), 1 - exp
      rounds (u alpha) and so does 1 - alpha (u f):
          |d alpha_j| = u (alpha_j + (E + x_j) f_j),     |d f_j| = u (alpha_j + f_j + (E + x_j) f_j) = u (1 + (E + x_j) f_j).
      E = 1 IS AN ASSUMPTION: the ISA documentation states 1 ulp for v_exp_f32.  It is not something measured here.
  transmittance.  T_i is a product of i factors formed along `levels(i)` multiplications: 6 scan levels and 1 carry per 64-sample chunk,
      levels(i) = 7 (i // 64 + 1).  In leave-one-out form (no division: an opaque sample, f_j = 0, is like any other)
          |d T_i| = sum_{j<i} (prod_{k<i, k != j} f_k) |d f_j|  +  u levels(i) T_i,
      the first part by the recurrence A_0 = 0, A_{i+1} = A_i f_i + T_i |d f_i|.
  weight.   |d w_i| = T_i |d alpha_i| + alpha_i |d T_i| + u w_i.
  running sums.  R(i) = sum_{j<=i} term_j carries the terms' own errors plus levels(i) u sum_{j<=i} |term_j| (6 scan levels + 1 carry
      add per chunk).  term = w_j c_j: c_j |d w_j| + u w_j c_j;  term = w_j: |d w_j|;  term = w_j t_j: t_j |d w_j| + w_j |d t_j| + u w_j t_j
      with |d t_j| = u levels(j) t_j.  The ray's totals are R(n - 1).
  tail.     image_out: |d image| + bg |d ws| + u (|1 - ws| bg + |back| + |image_out|);  depth_out: (|d depth| + u |depth - near|) /
      (far - near) + 2 u depth_out (max(., 0) is 1-Lipschitz).
  criterion.  d = image_out - target: |d d| = |d image_out| + u |d|.  With k = scale loss_mul / 3N:  MSE gi = norm d gl, |d gi| = 2 k |d d|
      + 4 u |gi| (norm, gl, two products);  L1 gi = sign gl / count, 3 u |gi|;  Huber k |d d| + 4 u |gi| on the quadratic branch, 4 u |gi| on
      the linear one (plus k |d d| where |d| is within the tolerance of delta: the gradient is continuous there, the branch is not).
      gws: sum_c |d gi_c| + 2 u sum_c |gi_c| + u |gws|.  With given grad_image / grad_weights_sum these errors are zero.
  gradients.  grad_rgb: w |d gi| + |gi| |d w| + u |gi w|.  grad_sigma: the kernels (as the reference's CUDA) form the suffix as
      fin - running, so behind an opaque surface the honest error is an ulp of the ray's TOTAL, not of the suffix:
          inner_c = T_{i+1} c_i - (fin_c - R_c(i)):  c_i |d T_{i+1}| + |d fin_c| + |d R_c(i)| + u |S_c(i)| + u |inner_c|
      (|d fin_c| = |d R_c(n - 1)| contains levels(n - 1) u sum_i |w_i c_i|, and likewise sum_i w_i for the opacity term), and
          acc = sum_c gi_c inner_c + gws inner_ws:  sum (|inner| |d gi| + |gi| |d inner|) + 4 u sum |gi inner|   (four fused steps)
          grad_sigma = delta0 acc:  delta0 |d acc| + u |grad_sigma|.

THE CONSTANT.  tolerance = C u magnitude + 2^-126.  Every rounding of the tree walk is already counted once in the magnitude, so to first
order the tree walk in exact-rounding fp32 arithmetic lies within 1 x u magnitude.  C = 2: the bound must hold the two CPU emulations
at a ratio of at most 0.5; the factor of 2 that leaves is the margin for the hardware's exponential (its argument is scaled by log2 e
first: a second u x f) and for products contracted into the additions that follow them.  The serial emulation is not covered term by
term -- its sums are n deep, not levels(n) -- but its roundings are not aligned, and it has to pass the same 0.5.
Measured on the CPU (ladder_problem, every M variant, every criterion, with and without a loss scale; tests/test_composite_float64_cpu.py
asserts <= 0.5), worst |emulation - float64| / tolerance:
    tree walk 0.2437, serial walk 0.2437 (both: grad_rgbs of a thin sample; every other output <= 0.094).
THE EMULATIONS' EXPONENTIAL is numpy's exp of the float32 argument rounded once to float32 (exp32, half an ulp).  numpy's own float32
loop is not used for the acceptance: its vector kernels are off by up to 2.4 ulp (measured; 1.98 ulp for arguments in [-0.01, 0]) --
more than the E = 1 assumed for the hardware -- and where alpha = 1 - exp(-x) cancels (x ~ 0.003) that error is all of the weight's error.
With that loop both walks come to 0.62 (grad_rgbs; asserted <= 1, test_numpy_float32_exp_stays_within_the_whole_tolerance): the missing
term is the emulation's, not the kernels', so neither E nor C moves for it.
These figures are a record, not an input to C.
"""
import numpy as np

EPS32 = 2.0 ** -24
TINY = 2.0 ** -126  # smallest normal fp32
E_EXP = 1.0         # assumed error of the hardware exponential, in ulps (see above)
C = 2.0
WAVE = 64
MSE, L1, HUBER = 0, 1, 2
F4, F8 = np.float32, np.float64

LADDER = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 700)
OPACITIES = (0.5, 3.0, 40.0)  # total optical depth: thin, medium, opaque
BG, MUL = 1.0, 0.5


# ------------------------------------------------------------------------------------------------------------------------- the problem
def ladder_problem(seed=0, n_fill=234):
    """One ragged batch: half of the filler rays (0 .. 150 samples), the ladder (every length at three opacities, sorted by length), the
    other fillers.  Record n writes output slot rays[n, 0], a permutation; offsets are the exclusive prefix sums of the counts.  On thin
    and medium rays the samples 63, 64 and every 64 k get alpha in [0.2, 0.5].  Buffers are total + 8 rows long; M is one of
    p["M"]: "slack" (total + 8), "exact" (total: the last ray is dead by `offset + num_steps >= M`), "cut" (inside the medium 192-sample
    ray: that ray and every later one is dead).  N = 63 + n_fill = 297 = 4 * 74 + 1.  Never modified by its users."""
    rng = np.random.default_rng(seed)
    fill = rng.integers(0, 151, n_fill)
    fill[-1] = max(int(fill[-1]), 5)  # the last record has samples: the "exact" variant kills it
    half = n_fill // 2
    counts = np.concatenate([fill[:half], np.repeat(LADDER, 3), fill[half:]]).astype(np.int64)
    taus = np.concatenate([rng.uniform(0.3, 20, half), np.tile(OPACITIES, len(LADDER)), rng.uniform(0.3, 20, n_fill - half)])
    forced = np.concatenate([np.zeros(half, bool), np.tile([True, True, False], len(LADDER)), np.zeros(n_fill - half, bool)])
    N = counts.size
    offsets = np.cumsum(counts) - counts
    total = int(counts.sum())
    rows = total + 8
    d0 = rng.uniform(0.003, 0.03, rows).astype(F4)
    d1 = rng.uniform(0.003, 0.04, rows).astype(F4)
    x = rng.uniform(0.0, 0.5, rows)  # (the slack rows: anything)
    for n in range(N):
        o, c = int(offsets[n]), int(counts[n])
        if c == 0:
            continue
        share = rng.uniform(0.05, 1.0, c)
        x[o:o + c] = taus[n] * share / share.sum()
        if forced[n]:
            at = sorted({63} | set(range(64, c, 64)))
            at = [i for i in at if i < c]
            x[o + np.array(at, dtype=np.int64)] = -np.log(1.0 - rng.uniform(0.2, 0.5, len(at)))
    sigmas = (x / d0.astype(F8)).astype(F4)
    rays = np.stack([rng.permutation(N), offsets, counts], axis=1).astype(np.int32)
    nears = (rng.uniform(0, 1, N) + 0.2).astype(F4)
    fars = (nears + (rng.uniform(0, 1, N) * 3 + 0.1).astype(F4)).astype(F4)
    g_ws = rng.standard_normal(N).astype(F4)
    g_img = rng.standard_normal((N, 3)).astype(F4)
    none = rng.permutation(N)[:N // 8]  # rays with exactly zero gradient (plain backward)
    g_ws[none], g_img[none] = 0.0, 0.0
    cut_ray = half + 3 * LADDER.index(192) + 1
    assert counts[cut_ray] == 192 and taus[cut_ray] == 3.0
    return dict(sigmas=sigmas, rgbs=rng.uniform(0, 1, (rows, 3)).astype(F4), deltas=np.stack([d0, d1], axis=1), rays=rays, nears=nears, fars=fars,
                target=rng.uniform(0, 1, (N, 3)).astype(F4), g_ws=g_ws, g_img=g_img, N=N, total=total, cut_ray=cut_ray,
                M={"slack": rows, "exact": total, "cut": int(offsets[cut_ray]) + 100})


def alive(p, M):
    """per record: the kernels' rule"""
    off, cnt = p["rays"][:, 1].astype(np.int64), p["rays"][:, 2].astype(np.int64)
    return (cnt != 0) & (off + cnt < M)


def covered_rows(p, M):
    """[M] bool: rows some live ray covers"""
    cov = np.zeros(M, bool)
    for (_, off, cnt), a in zip(p["rays"], alive(p, M)):
        if a:
            cov[off:off + cnt] = True
    return cov


# ----------------------------------------------------------------------------------------------------------------------- the reference
def levels(i):
    return 7.0 * (np.asarray(i) // WAVE + 1)


def _ray_forward(s, c, d0, d1):
    """One live ray in float64 -> dict of per-sample values and their magnitudes (units of u)."""
    n = s.size
    x = s * d0
    f = np.exp(-x)
    a = -np.expm1(-x)
    T = np.concatenate([[1.0], np.cumprod(f)])  # T[i]: before sample i; T[i + 1]: after it
    da = a + (E_EXP + x) * f
    df = 1.0 + (E_EXP + x) * f
    A = np.zeros(n + 1)
    acc = 0.0
    for i in range(n):  # leave-one-out sum: A_{i+1} = A_i f_i + T_i |d f_i|
        acc = acc * f[i] + T[i] * df[i]
        A[i + 1] = acc
    lv = levels(np.arange(n))
    dT0, dT1 = A[:-1] + lv * T[:-1], A[1:] + lv * T[1:]
    w = a * T[:-1]
    dw = T[:-1] * da + a * dT0 + w
    wc = w[:, None] * c
    run = np.cumsum(wc, axis=0)
    drun = np.cumsum(c * dw[:, None] + wc, axis=0) + lv[:, None] * run  # (the terms are non-negative: sum |terms| = run)
    rws = np.cumsum(w)
    drws = np.cumsum(dw) + lv * rws
    t = np.cumsum(d1)
    wt = w * t
    ddepth = np.sum(t * dw + w * lv * t + wt) + lv[-1] * wt.sum()
    suf = np.cumsum(wc[::-1], axis=0)[::-1] - wc  # sum_{j>i}
    sws = np.cumsum(w[::-1])[::-1] - w
    return dict(w=w, dw=dw, T1=T[1:], dT1=dT1, run=run, drun=drun, rws=rws, drws=drws, suf=suf, sws=sws, depth=wt.sum(), ddepth=ddepth)


_FORWARD = {}


def forward_reference(p, M):
    """-> dict: weights_sum, depth [N], image [N, 3] by output slot, each with *_mag; `per_ray`: the per-sample dicts by record (None: dead).
    Cached per (problem, M): do not modify."""
    key = (id(p), M)
    if key not in _FORWARD:
        N = p["N"]
        out = {k: np.zeros(sh) for k, sh in (("weights_sum", N), ("depth", N), ("image", (N, 3)), ("weights_sum_mag", N), ("depth_mag", N), ("image_mag", (N, 3)))}
        per = [None] * N
        s8, c8, d8 = p["sigmas"].astype(F8), p["rgbs"].astype(F8), p["deltas"].astype(F8)
        for n, ((idx, off, cnt), a) in enumerate(zip(p["rays"], alive(p, M))):
            if not a:
                continue
            r = _ray_forward(s8[off:off + cnt], c8[off:off + cnt], d8[off:off + cnt, 0], d8[off:off + cnt, 1])
            per[n] = r
            out["weights_sum"][idx], out["weights_sum_mag"][idx] = r["rws"][-1], r["drws"][-1]
            out["image"][idx], out["image_mag"][idx] = r["run"][-1], r["drun"][-1]
            out["depth"][idx], out["depth_mag"][idx] = r["depth"], r["ddepth"]
        out["per_ray"] = per
        _FORWARD[key] = out
    return _FORWARD[key]


def criterion64(kind, param, d):
    """elementwise criterion and its slope (torch's semantics: mse_loss, l1_loss with sign(0) = 0, huber_loss quadratic where |d| <= delta)"""
    if kind == MSE:
        return d * d, 2.0 * d
    if kind == L1:
        return np.abs(d), np.sign(d)
    a = np.abs(d)
    return np.where(a <= param, 0.5 * d * d, param * (a - 0.5 * param)), np.where(a <= param, d, param * np.sign(d))


def tail_reference(p, M, kind=MSE, param=0.0, scale=1.0):
    """The render tail and the criterion on top of forward_reference -> image_out, depth_out (+ *_mag), err [N], loss, scaled_loss, and the
    gradient of scaled_loss with respect to image / weights_sum: gi [N, 3], gws [N] (+ *_mag)."""
    fw = forward_reference(p, M)
    N = p["N"]
    param = float(F4(param))
    ws, img = fw["weights_sum"], fw["image"]
    back = (1.0 - ws) * BG
    image_out = img + back[:, None]
    image_out_mag = fw["image_mag"] + (BG * fw["weights_sum_mag"] + np.abs(1.0 - ws) * BG + np.abs(back))[:, None] + np.abs(image_out)
    near, far = p["nears"].astype(F8), p["fars"].astype(F8)
    depth_out = np.maximum(fw["depth"] - near, 0.0) / (far - near)
    depth_out_mag = (fw["depth_mag"] + np.abs(fw["depth"] - near)) / (far - near) + 2.0 * depth_out
    d = image_out - p["target"].astype(F8)
    dd = image_out_mag + np.abs(d)
    e, slope = criterion64(kind, param, d)
    loss = e.sum() / (3.0 * N) * MUL
    k = scale * MUL / (3.0 * N)
    gi = k * slope
    if kind == MSE:
        gi_mag = 2.0 * k * dd + 4.0 * np.abs(gi)
    elif kind == L1:
        gi_mag = 3.0 * np.abs(gi)
    else:
        a = np.abs(d)
        gi_mag = 4.0 * np.abs(gi) + np.where((a <= param) | (np.abs(a - param) <= C * EPS32 * dd), k * dd, 0.0)
    gws = -gi.sum(axis=1) * BG
    gws_mag = BG * (gi_mag.sum(axis=1) + 2.0 * np.abs(gi).sum(axis=1)) + np.abs(gws)
    return dict(image_out=image_out, image_out_mag=image_out_mag, depth_out=depth_out, depth_out_mag=depth_out_mag, err=e.sum(axis=1), loss=loss,
                scaled_loss=loss * scale, gi=gi, gi_mag=gi_mag, gws=gws, gws_mag=gws_mag, d=d)


def backward_reference(p, M, gi, gws, gi_mag=None, gws_mag=None):
    """grad_sigmas [M], grad_rgbs [M, 3] (+ *_mag) for the gradients gi [N, 3], gws [N] (by output slot) of the rays' image and opacity sum;
    gi_mag / gws_mag: their own error magnitudes (None: given exactly).  Rows no live ray covers: zeros."""
    fw = forward_reference(p, M)
    gi, gws = np.asarray(gi, F8), np.asarray(gws, F8)
    gi_mag = np.zeros_like(gi) if gi_mag is None else gi_mag
    gws_mag = np.zeros_like(gws) if gws_mag is None else gws_mag
    gs, gs_mag, gc, gc_mag = np.zeros(M), np.zeros(M), np.zeros((M, 3)), np.zeros((M, 3))
    c8, d8 = p["rgbs"].astype(F8), p["deltas"].astype(F8)
    for (idx, off, cnt), r in zip(p["rays"], fw["per_ray"]):
        if r is None:
            continue
        sl = slice(off, off + cnt)
        c, d0 = c8[sl], d8[sl, 0]
        q, dq, qw, dqw = gi[idx], gi_mag[idx], gws[idx], gws_mag[idx]
        gc[sl] = q * r["w"][:, None]
        gc_mag[sl] = r["w"][:, None] * dq + np.abs(q) * r["dw"][:, None] + np.abs(gc[sl])
        inner = r["T1"][:, None] * c - r["suf"]
        dinner = c * r["dT1"][:, None] + r["drun"][-1] + r["drun"] + np.abs(r["suf"]) + np.abs(inner)
        iws = r["T1"] - r["sws"]
        diws = r["dT1"] + r["drws"][-1] + r["drws"] + np.abs(r["sws"]) + np.abs(iws)
        acc = (q * inner).sum(axis=1) + qw * iws
        terms = (np.abs(q) * np.abs(inner)).sum(axis=1) + abs(qw) * np.abs(iws)
        dacc = (np.abs(inner) * dq + np.abs(q) * dinner).sum(axis=1) + np.abs(iws) * dqw + abs(qw) * diws + 4.0 * terms
        gs[sl] = d0 * acc
        gs_mag[sl] = d0 * dacc + np.abs(gs[sl])
    return dict(grad_sigmas=gs, grad_sigmas_mag=gs_mag, grad_rgbs=gc, grad_rgbs_mag=gc_mag)


def step_reference(p, M, kind=MSE, param=0.0, scale=1.0):
    """Everything a training step's compositing produces, for a root gradient of one on scaled_loss."""
    fw = forward_reference(p, M)
    tail = tail_reference(p, M, kind, param, scale)
    res = {k: v for k, v in fw.items() if k != "per_ray"}
    res.update(tail)
    res.update(backward_reference(p, M, tail["gi"], tail["gws"], tail["gi_mag"], tail["gws_mag"]))
    return res


def tolerance(mag):
    return C * EPS32 * np.asarray(mag, F8) + TINY


def ratio(got, want, mag, mask=None):
    """worst |got - want| / tolerance (inf for a NaN) over the elements of mask"""
    err = np.abs(np.asarray(got, F8) - want)
    r = np.where(np.isnan(err), np.inf, err / tolerance(mag))
    if mask is not None:
        r = r[mask]
    return float(r.max()) if r.size else 0.0


# ----------------------------------------------------------------------------------------------------------- float32 emulations (numpy)
def exp32(x):
    """The emulations' float32 exponential: numpy's exp of the float32 argument, rounded once to float32 (within half an ulp)."""
    return np.exp(np.asarray(x, F4).astype(F8)).astype(F4)


def exp32_native(x):
    """numpy's own float32 loop (measured at up to 2.4 ulp with its AVX512 kernels: beyond the E = 1 assumed for the hardware)"""
    return np.exp(np.asarray(x, F4))


def _fmaf(a, b, c):
    """fmaf in float32: the product of two float32 is exact in float64"""
    return (np.asarray(a, F8) * np.asarray(b, F8) + np.asarray(c, F8)).astype(F4)


def _tail32(ws, depth, img, near, far, tgt, kind, param):
    """ray_tail_forward (contraction off): -> image_out [.., 3], depth_out, err, all float32"""
    one, half = F4(1.0), F4(0.5)
    back = (one - ws) * F4(BG)
    out = (img + back[..., None]).astype(F4)
    e = out - tgt
    if kind == MSE:
        el = e * e
    elif kind == L1:
        el = np.abs(e)
    else:
        a, dl = np.abs(e), F4(param)
        el = np.where(a <= dl, half * a * a, dl * (a - half * dl))
    err = ((F4(0.0) + el[..., 0]) + el[..., 1]) + el[..., 2]
    depth_out = np.maximum(depth - near, F4(0.0)) / (far - near)
    return out, depth_out.astype(F4), err.astype(F4)


def _ray_gradient32(out, tgt, N, kind, param, scale, mutate=None):
    """ray_loss_gradient / ray_criterion_gradient -> gi [.., 3], gws, float32.  gl = scale * loss_mul"""
    gl = F4(scale) * F4(MUL)
    d = out - tgt
    if kind == MSE:
        gi = F4(2.0 / (N * 3.0)) * d * gl
    else:
        sign = np.sign(d).astype(F4)
        if kind == HUBER and mutate != "huber_l1":
            slope = np.where(np.abs(d) <= F4(param), d, F4(param) * sign)
        else:
            slope = sign
        gi = slope * gl / F4(N * 3.0)
    s = ((F4(0.0) + gi[..., 0]) + gi[..., 1]) + gi[..., 2]
    gws = -(s * F4(BG))
    if mutate == "gws_sign":
        gws = -gws
    return gi.astype(F4), gws.astype(F4)


def _empty_outputs(p, M):
    N = p["N"]
    return dict(weights_sum=np.zeros(N, F4), depth=np.zeros(N, F4), image=np.zeros((N, 3), F4), grad_sigmas=np.zeros(M, F4), grad_rgbs=np.zeros((M, 3), F4))


def _finish(p, res, kind, param, scale, given, mutate=None):
    """tail + criterion gradient per output slot (or the given gradients)"""
    N = p["N"]
    res["image_out"], res["depth_out"], res["err"] = _tail32(res["weights_sum"], res["depth"], res["image"], p["nears"], p["fars"], p["target"], kind, param)
    if given is not None:
        return given[1].astype(F4), given[0].astype(F4)
    return _ray_gradient32(res["image_out"], p["target"], N, kind, param, scale, mutate)


def emulate_serial(p, M, kind=MSE, param=0.0, scale=1.0, given=None, exp=exp32):
    """(a) The reference's serial walk in float32, all rays at once, one sample per iteration: T, the running sums and the depth in a
    ray's own order; the backward with the suffix as final - running and plain products and sums.  given = (grad_weights_sum,
    grad_image): the plain backward; otherwise the tail and the criterion's gradient (the tree emulation's expressions) sit between."""
    res = _empty_outputs(p, M)
    rays, live = p["rays"], alive(p, M)
    idx, off, cnt = rays[live, 0], rays[live, 1].astype(np.int64), rays[live, 2].astype(np.int64)
    sg, c, d0, d1 = p["sigmas"], p["rgbs"], p["deltas"][:, 0], p["deltas"][:, 1]
    R = idx.size
    one = F4(1.0)

    def walk(backward, gi=None, gws=None, fin=None):
        T, t, d, ws = np.ones(R, F4), np.zeros(R, F4), np.zeros(R, F4), np.zeros(R, F4)
        rgb = np.zeros((R, 3), F4)
        for k in range(int(cnt.max()) if R else 0):
            on = cnt > k
            i = off[on] + k
            alpha = one - exp(-sg[i] * d0[i])
            weight = alpha * T[on]
            rgb[on] = rgb[on] + weight[:, None] * c[i]
            ws[on] = ws[on] + weight
            if not backward:
                t[on] = t[on] + d1[i]
                d[on] = d[on] + weight * t[on]
            T[on] = T[on] * (one - alpha)
            if backward:
                res["grad_rgbs"][i] = gi[on] * weight[:, None]
                inner = T[on][:, None] * c[i] - (fin[0][on] - rgb[on])
                acc = ((gi[on, 0] * inner[:, 0] + gi[on, 1] * inner[:, 1]) + gi[on, 2] * inner[:, 2]) + gws[on] * (T[on] - (fin[1][on] - ws[on]))
                res["grad_sigmas"][i] = d0[i] * acc
        return rgb, ws, d

    rgb, ws, d = walk(False)
    res["image"][idx], res["weights_sum"][idx], res["depth"][idx] = rgb, ws, d
    gi, gws = _finish(p, res, kind, param, scale, given)
    walk(True, gi[idx], gws[idx], (rgb, ws))
    return res


def _shr(v, s, ident):
    """row_shr:s -- lane l of a 16-lane row takes lane l - s of its row; a lane without a source keeps the identity"""
    o = np.full((4, 16), ident, F4)
    o[:, s:] = v.reshape(4, 16)[:, :-s]
    return o.reshape(64)


def _scan(v, op, ident):
    """wave_scan_add / wave_scan_mul: row_shr 1, 2, 4, 8, then row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3"""
    for s in (1, 2, 4, 8):
        v = op(v, _shr(v, s, ident))
    b = np.full(64, ident, F4)
    b[16:32], b[48:64] = v[15], v[47]
    v = op(v, b)
    b = np.full(64, ident, F4)
    b[32:64] = v[31]
    return op(v, b)


def _scan_add(v):
    return _scan(v.astype(F4), np.add, 0.0)


def _load(p, off, k0, steps, drop=None):
    """load_chunk: samples k0 .. k0 + 63 of the ray at `off`; idle lanes are fed zeros"""
    k = k0 + np.arange(WAVE)
    on = k < steps
    if drop is not None:
        on = on & (k != drop)
    i = np.where(on, off + k, 0)
    z = F4(0.0)
    return dict(on=on, i=off + k, sg=np.where(on, p["sigmas"][i], z), d0=np.where(on, p["deltas"][i, 0], z), d1=np.where(on, p["deltas"][i, 1], z),
                c=np.where(on[:, None], p["rgbs"][i], z), k0=k0)


def _new_carry():
    return dict(T=F4(1.0), t=F4(0.0), rgb=np.zeros(3, F4), ws=F4(0.0), d=F4(0.0))


def _chunk_walk(inp, c, depth, mutate=None, exp=exp32):
    """chunk_walk<DEPTH>, in its expression order; updates the carry c"""
    one = F4(1.0)
    alpha = one - exp(-inp["sg"] * inp["d0"])
    incl = _scan(one - alpha, np.multiply, 1.0)
    excl = np.concatenate([[one], incl[:-1]]).astype(F4)  # wave_shr:1
    cT = one if (mutate == "no_carry_T" and inp["k0"] == WAVE) else c["T"]
    weight = alpha * (cT * (incl if mutate == "weight_after" else excl))
    twice = np.ones(WAVE, F4)
    if mutate == "double_64" and inp["k0"] == WAVE:
        twice[0] = 2.0
    o = dict(weight=weight, T=cT * incl)
    o["rgb"] = np.stack([c["rgb"][ch] + _scan_add(weight * inp["c"][:, ch] * twice) for ch in range(3)], axis=1)
    o["ws"] = c["ws"] + _scan_add(weight * twice)
    if depth:
        t = c["t"] + _scan_add(inp["d1"])
        c["d"] = (c["d"] + _scan_add(weight * (inp["d0"] if mutate == "depth_delta0" else t) * twice))[-1]
        c["t"] = t[-1]
    c["T"] = cT * incl[-1]
    c["rgb"], c["ws"] = o["rgb"][-1].copy(), o["ws"][-1]
    return o


def _sample_backward(res, inp, o, gi, gws, fin):
    """sample_backward's expressions"""
    on, i = inp["on"], inp["i"][inp["on"]]
    w, T = o["weight"], o["T"]
    res["grad_rgbs"][i] = (gi[None, :] * w[:, None])[on]
    acc = gi[0] * _fmaf(T, inp["c"][:, 0], -(fin["rgb"][0] - o["rgb"][:, 0]))
    acc = _fmaf(gi[1], _fmaf(T, inp["c"][:, 1], -(fin["rgb"][1] - o["rgb"][:, 1])), acc)
    acc = _fmaf(gi[2], _fmaf(T, inp["c"][:, 2], -(fin["rgb"][2] - o["rgb"][:, 2])), acc)
    acc = _fmaf(gws, T - (fin["ws"] - o["ws"]), acc)
    res["grad_sigmas"][i] = (inp["d0"] * acc)[on]


MUTATIONS = ("no_carry_T", "drop_63", "double_64", "weight_after", "totals_before_last", "fresh_restart", "depth_delta0", "gws_sign", "huber_l1")


def emulate_tree(p, M, kind=MSE, param=0.0, scale=1.0, keep=2, given=None, mutate=None, exp=exp32):
    """(b) The 64-lane tree walk with chunk carry in float32, structured as composite_step_kernel: the first `keep` chunks walked once and
    kept, the others walked for the totals and again -- from the state at `keep` -- for their gradients.  (The three launches compute the
    same values: a walk restarted from the beginning repeats its bits.)  mutate: one of MUTATIONS, a deliberately wrong walk."""
    assert mutate is None or mutate in MUTATIONS
    res = _empty_outputs(p, M)
    drop = 63 if mutate == "drop_63" else None
    state = {}
    for (idx, off, cnt), a in zip(p["rays"], alive(p, M)):
        if not a:
            continue
        off, steps = int(off), int(cnt)
        c, kept, fin = _new_carry(), [], None
        for j in range(keep):
            if j * WAVE < steps:
                inp = _load(p, off, j * WAVE, steps, drop)
                if mutate == "totals_before_last" and j * WAVE + WAVE >= steps and j > 0:
                    fin = {k: np.copy(v) for k, v in c.items()}
                kept.append((inp, _chunk_walk(inp, c, True, mutate, exp)))
        at_keep = {k: np.copy(v) for k, v in c.items()}
        for k0 in range(keep * WAVE, steps, WAVE):
            if mutate == "totals_before_last" and k0 + WAVE >= steps:
                fin = {k: np.copy(v) for k, v in c.items()}
            _chunk_walk(_load(p, off, k0, steps, drop), c, True, mutate, exp)
        if fin is None:
            fin = c
        res["weights_sum"][idx], res["depth"][idx], res["image"][idx] = fin["ws"], fin["d"], fin["rgb"]
        state[int(idx)] = (off, steps, kept, at_keep, fin)
    gi, gws = _finish(p, res, kind, param, scale, given, mutate)
    for idx, (off, steps, kept, at_keep, fin) in state.items():
        for inp, o in kept:
            _sample_backward(res, inp, o, gi[idx], gws[idx], fin)
        c = _new_carry() if mutate == "fresh_restart" else at_keep
        for k0 in range(keep * WAVE, steps, WAVE):
            inp = _load(p, off, k0, steps, drop)
            _sample_backward(res, inp, _chunk_walk(inp, c, False, mutate, exp), gi[idx], gws[idx], fin)
    return res


GROUPS = ("weights_sum", "depth", "image", "image_out", "depth_out", "grad_sigmas", "grad_rgbs")


def ratios(got, want, groups=GROUPS, skip_l1=None):
    """worst ratio per output of `got` (arrays by name) against a reference dict.  skip_l1 [N, 3] bool: elements whose L1 sign is ambiguous --
    their rays are left out of the gradient groups by the caller's mask (see l1_row_mask)."""
    return {g: ratio(got[g], want[g], want[g + "_mag"], None if skip_l1 is None or not g.startswith("grad_") else skip_l1) for g in groups}


def l1_row_mask(p, M, ambiguous):
    """[M] bool: rows whose ray has no ambiguous L1 element (ambiguous [N, 3] by output slot)"""
    ok = np.ones(M, bool)
    bad = ambiguous.any(axis=1)
    for idx, off, cnt in p["rays"]:
        if bad[idx]:
            ok[off:min(off + cnt, M)] = False
    return ok
