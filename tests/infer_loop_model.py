"""TEST INFRASTRUCTURE: a host model of the inference loop's kernels (csrc/raymarching.hip: compact_count_kernel / compact_write_kernel,
composite_rays_kernel, and the device-count contract of march_rays_kernel) for tests/test_gpu_infer_loop_edges.py, checked on the CPU by
tests/test_infer_loop_model_cpu.py.  Plain numpy, no GPU import.  Both test modules build their inputs with the case builders below.

THE OPERATIONS.

  unit_rows(code, count).  csrc/common.hpp in integers: a plain number passes through; with bit 31 set the code carries F (bits 24..30) and N
      (bits 0..23) and means clamp(F N // max(count, 1), F, 8 F).

  compact.  The five compaction entries.  With n_eff = min(bound, count) (plain form: n_eff = bound) entry n of the old lists is kept iff
      n < n_eff and rays_t_old[n] >= 0 -- so -0.0 is kept and NaN is dropped, as the reference's `rays_t_old[n] >= 0` does.  The k survivors keep
      their order.  Plain form: they land at [base, base + k), base the counter's value on entry, and the counter becomes base + k.
      Device-count form: they land at [0, k) and the counter is OVERWRITTEN with k.  Budget form: if steps_done >= max_steps the counter
      is 0 (the survivors are still written) and the step word stays; otherwise the step word gains unit_rows(code, k).  Mirror form: the host word
      equals the counter.  A call with bound 0 launches nothing: no word is written.  Everything a call does not write keeps what it held.

  composite64.  One compositing call in float64 from the float32 inputs.  Slot n < n_alive with index = rays_alive[n] reads samples
      i = 0 .. n_step - 1 at rows n n_step + i and stops at the first delta0 == 0:
          x_i = sigma_i delta0_i,  f_i = exp(-x_i),  alpha_i = 1 - f_i,  T_i = (1 - weights_sum_in) prod_{j<i} f_j,  w_i = alpha_i T_i,
          t_i = rays_t[n] + sum_{j<=i} delta1_j   (a sequential FLOAT32 sum: formed in float32 here and compared bit for bit),
          weights_sum[index] += w_i,  depth[index] += w_i t_i,  image[index] += w_i c_i.
      A sample with T_i < 1e-4 is still accumulated, and it is the ray's last.  rays_t[n] becomes -1 if the walk stopped before n_step samples
      (an unused slot, or the transmittance cut -- also on the last slot), else t.

  emulate32.  The kernel's operation sequence in float32 (fmaf for the three accumulations, exp32 for the exponential).  It exists to check the
      bound below; it is never compared with the GPU.

  loop.  N = 193 rays of tests/march_cases.py through `compact (budget, mirror) -> march -> field -> composite` per iteration, n_step derived from
      the alive count (F = 4), on the all-occupied and on the scene grid of tests/march_cases.py at H = 128, with max_steps 1024 and 40.  The
      march is the oracle's on the CPU; the field is standin_field (float32 numpy from the positions).

THE ERROR MODEL.  u = 2^-24; magnitudes are first-order bounds on the fp32 error of composite_rays_kernel in units of u, every rounding of the
walk entering once at its worst case, in the manner of tests/composite_float64.py -- with two differences: the walk is serial, so sample i's
running sums have taken i + 1 additions, each rounded at the partial sum it produced (no tree levels); and the kernel does not carry T as a
product, it forms T = 1 - weight_sum from its running sum.

  factor.   |d alpha_i| = u (alpha_i + (E + x_i) f_i): the product sigma delta0 rounds (u x f), the exponential is off by E ulps of f, 1 - exp
      rounds (u alpha).  E = composite_float64.E_EXP = 1 IS AN ASSUMPTION (the ISA's stated 1 ulp for v_exp_f32), not measured here.
  transmittance.  T_i = fl(1 - S_i), S_i the running weight sum with error e_i:  |d T_i| = e_i + u T_i  (the sum's error plus one rounding).
  weight.   w_i = fl(alpha_i T_i):  |d w_i| = T_i |d alpha_i| + alpha_i |d T_i| + u w_i = T_i |d alpha_i| + alpha_i e_i + 2 u w_i.
  weight sum.  S_{i+1} = fl(S_i + w_i).  The sum's own error comes back through T with the factor -alpha_i, so it is carried with 1 - alpha_i = f_i:
          e_{i+1} = f_i e_i + T_i |d alpha_i| + 2 u w_i + u S_{i+1}.
  image, depth.  I_{i+1} = fma(w_i, c_i, I_i): one rounding, of the new partial sum:  |d I_{i+1}| = |d I_i| + c_i |d w_i| + u |I_{i+1}|, and
      the same for depth with t_i (exact: the float32 t is part of the definition) in place of c_i.
  between calls.  weights_sum, depth and image are read back as the float32 the last call stored: the errors carry, so the magnitudes are carried
      with the values (e_0 of a call is the weights_sum magnitude the previous call left for that ray; zero for given inputs).

THE CONSTANT.  tolerance = C u magnitude + 2^-126 with composite_float64's C = 2: exact-rounding fp32 arithmetic lies within 1 x u magnitude to
first order, the emulation has to pass at 0.5, and the factor of 2 that leaves is the margin for the hardware's exponential (its argument is
scaled by log2 e first: a second u x f).

THE DECISION.  `T < 1e-4` is a branch, so a ray whose T sits within the error of 1e-4 could legitimately stop one sample apart.  The cases are built
so that none does: at every sample of every ray the float64 T_i lies outside 1e-4 +- 4 x (absolute tolerance of weights_sum at that sample).  No
ray is excluded from any comparison; tests/test_infer_loop_model_cpu.py asserts that the excluded share is zero.

Measured on the CPU (every compositing case; tests/test_infer_loop_model_cpu.py asserts emulate32 <= 0.5 and the oracle <= 1.0), worst
|x - float64| / tolerance:
    emulate32:  weights_sum 0.3075, depth 0.2934, image 0.3657;
                through the loops (carried magnitudes, every iteration): weights_sum 0.2052, depth 0.2095, image 0.2090 (scene grid, 40 steps;
                after the 88 iterations of the all-occupied grid the final accumulators sit at 0.0061, 0.0068, 0.0103: the magnitude grows with
                every addition, the error like a random walk)
    oracle.composite_rays (host libm expf):  weights_sum 0.3075, depth 0.2934, image 0.3657
Measured on an MI355X (tests/test_gpu_infer_loop_edges.py prints them), worst |device - float64| / tolerance:
    single calls (both entries, the same bits):  weights_sum 0.3075, depth 0.2934, image 0.3657
    final accumulators of the loops:  weights_sum 0.2052, depth 0.2095, image 0.2090 (scene grid, 40 steps; all-occupied grid, 1024 steps:
                0.0079, 0.0037, 0.0162)
These figures are a record, not an input to C.
"""
from collections import namedtuple

import numpy as np

from composite_float64 import C, E_EXP, EPS32, F4, F8, TINY, _fmaf, exp32, tolerance  # noqa: F401

T_CUT = 1e-4
FORMS = ("plain", "dev", "budget", "mirror")  # nerftex_compact_rays, .._dev, .._budget_dev, .._budget_mirror_dev
MAX_STEPS = 1024


# ------------------------------------------------------------------------------------------------------------------------------ unit_rows
def rows_auto(N, F):
    """NERFTEX_ROWS_AUTO(N, F) of include/nerftex_hip.h"""
    assert 0 < N < (1 << 24) and 0 < F <= 127
    return 0x80000000 | (F << 24) | N


def unit_rows(code, count, mutate=None):
    """csrc/common.hpp.  mutate: "no_upper", "no_lower", "no_zero_guard" (an unguarded 32-bit division by zero: all ones)"""
    code, count = int(code) & 0xFFFFFFFF, int(count) & 0xFFFFFFFF
    if not code >> 31:
        return code
    F, N = (code >> 24) & 127, code & 0xFFFFFF
    if count == 0 and mutate == "no_zero_guard":
        q = 0xFFFFFFFF
    else:
        q = (F * N & 0xFFFFFFFF) // max(count, 1)
    if q < F and mutate != "no_lower":
        return F
    if q > 8 * F and mutate != "no_upper":
        return 8 * F
    return q


# ------------------------------------------------------------------------------------------------------------------------------ compaction
# alive, t: the k survivors.  at: where they land in the new lists.  counter / steps / mirror: the words after the call, None = not written.
Compacted = namedtuple("Compacted", "k alive t at counter steps mirror")


def compact(form, bound, count, alive_old, t_old, base=0, steps_done=None, max_steps=0, code=0, mutate=None):
    """One compaction call.  base: alive_counter[0] on entry (it matters to the plain form only).  The elements the call may write are
    new lists [at, at + k) and the words that are not None."""
    assert form in FORMS
    if bound == 0:
        return Compacted(0, np.zeros(0, np.int32), np.zeros(0, F4), 0, None, None, None)
    n_eff = bound if (form == "plain" or mutate == "count_ignored") else min(bound, count)
    told = np.asarray(t_old, F4)[:n_eff]
    with np.errstate(invalid="ignore"):
        keep = (told > 0) if mutate == "gt_zero" else (told >= 0)
    alive, t = np.asarray(alive_old, np.int32)[:n_eff][keep], told[keep]
    k = int(keep.sum())
    if form == "plain":
        at = 0 if mutate == "ignore_base" else base
        return Compacted(k, alive, t, at, at + k, None, None)
    at = base if mutate == "base_in_dev" else 0
    counter, steps = at + k, None
    if form in ("budget", "mirror"):
        exhausted = (steps_done > max_steps) if mutate == "budget_gt" else (steps_done >= max_steps)
        if exhausted:
            counter = 0
            if mutate == "advance_on_exhausted":
                steps = steps_done + unit_rows(code, k)
        else:
            plain_F = (code >> 24) & 127 if code >> 31 else code
            steps = steps_done + (plain_F if mutate == "advance_plain_F" else unit_rows(code, k))
    return Compacted(k, alive, t, at, counter, steps, counter if form == "mirror" else None)


def filled(res, size, sentinel_alive, sentinel_t):
    """The new lists of `size` elements as a call leaves them when they held the sentinels before."""
    alive, t = np.full(size, sentinel_alive, np.int32), np.full(size, sentinel_t, F4)
    alive[res.at:res.at + res.k], t[res.at:res.at + res.k] = res.alive, res.t
    return alive, t


CompactCase = namedtuple("CompactCase", "name bound count alive_old t_old")
SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 66049)  # 66049 = 257 x 257: 259 workgroups, a second pass over the partials
PATTERNS = ("all", "none", "alternating", "lane0", "lane63", "dead_wave", "last_only", "first_only", "random37", "special")


def _keep_pattern(pattern, n, rng):
    i = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": i % 2 == 0, "lane0": i % 64 == 0, "lane63": i % 64 == 63,
            "dead_wave": (i // 64) % 3 != 1, "last_only": i == n - 1, "first_only": i == 0, "random37": rng.random(n) < 0.37,
            "special": rng.random(n) < 0.5}[pattern]


def _compact_case(name, n, pattern, count, seed):
    rng = np.random.default_rng(seed)
    keep = _keep_pattern(pattern, n, rng)
    t = (rng.random(n) + 0.1).astype(F4)
    t[~keep] = -1.0
    if pattern == "special":  # zeros of both signs and +inf are kept; NaN, -inf and a tiny negative are dropped
        kinds = rng.integers(0, 4, n)
        t[keep & (kinds == 0)] = -0.0
        t[keep & (kinds == 1)] = 0.0
        t[keep & (kinds == 2)] = np.inf
        t[~keep & (kinds == 0)] = np.nan
        t[~keep & (kinds == 1)] = -np.inf
        t[~keep & (kinds == 2)] = -1e-30
    if count < n:  # what lies behind the true count looks alive
        t[count:] = np.abs(np.nan_to_num(t[count:], nan=0.5, posinf=2.0, neginf=2.0)) + F4(0.25)
    alive = (rng.permutation(n) + 1000).astype(np.int32)  # a permutation, not arange
    for a in (alive, t):
        a.setflags(write=False)
    return CompactCase(name, n, count, alive, t)


_compaction = {}


def compaction_cases(n):
    """The cases of one list length: every keep pattern at count = bound, and the counts bound - 5 (a ragged last wave), 0 and 1."""
    if n not in _compaction:
        out = [_compact_case(f"{n}-{p}", n, p, n, 100 * n + j) for j, p in enumerate(PATTERNS)]
        for j, p in enumerate(("all", "random37", "alternating", "last_only")):
            if n > 5:
                out.append(_compact_case(f"{n}-{p}-count{n - 5}", n, p, n - 5, 100 * n + 20 + j))
        for j, p in enumerate(("all", "random37")):
            out.append(_compact_case(f"{n}-{p}-count0", n, p, 0, 100 * n + 30 + j))
            out.append(_compact_case(f"{n}-{p}-count1", n, p, 1, 100 * n + 40 + j))
        _compaction[n] = out
    return _compaction[n]


BUDGET_DONE = (0, MAX_STEPS - 1, MAX_STEPS, MAX_STEPS + 3)
# plain 4; the three AUTO codes; (5, 4): F N = 20 < 8 F, where a division by a zero count that is not guarded shows
BUDGET_CODES = (4, rows_auto(100, 4), rows_auto(2048, 4), rows_auto(16777215, 127), rows_auto(5, 4))
# survivor counts.  F N = 400: 101 and 133 -> 3 (below F), 100 -> 4 (on F), 99 and 80 -> 4 and 5, 33 -> 12 and 13 -> 30 (floors), 12 -> 33 (over 8 F).
# F N = 8192: 2049 -> 3, 2048 -> 4, 2047 -> 4, 1638 -> 5, 257 -> 31, 256 -> 32 (on 8 F), 255 -> 32, 248 -> 33.  0 and 1: the guard, F N itself.
BUDGET_SURVIVORS = (0, 1, 12, 13, 33, 80, 99, 100, 101, 133, 248, 255, 256, 257, 1638, 2047, 2048, 2049)


def budget_cases():
    """Lists with an exact number of survivors (BUDGET_SURVIVORS), scattered, for the step word under every code."""
    if "budget" not in _compaction:
        out = []
        for j, k in enumerate(BUDGET_SURVIVORS):
            rng = np.random.default_rng(7000 + j)
            n = k + k // 3 + 7
            t = np.full(n + 3, -1.0, F4)
            where = rng.permutation(n - 2)[:k]  # (the last two before the count are dead)
            t[where] = (rng.random(k) + 0.1).astype(F4)
            t[n:] = 0.75  # behind the count: looks alive
            alive = (rng.permutation(n + 3) + 5).astype(np.int32)
            for a in (alive, t):
                a.setflags(write=False)
            out.append(CompactCase(f"budget-k{k}", n + 3, n, alive, t))  # bound = count + 3
        _compaction["budget"] = out
    return _compaction["budget"]


STALE = 123   # what the counter of a device-count call holds on entry: overwritten, never added to
BASE = 37     # the non-zero base of the plain form: the new lists have room for it behind the survivors
Call = namedtuple("Call", "form base steps_done max_steps code")


def compaction_calls(case):
    """The calls both test modules make on a case: all five entries on every case (the plain one from base 0 and from BASE); on the budget cases
    every code at every state of the budget, through both budget entries."""
    calls = [Call("plain", 0, None, 0, 0), Call("plain", BASE, None, 0, 0), Call("dev", STALE, None, 0, 0)]
    if case.name.startswith("budget"):
        calls += [Call(form, STALE, done, MAX_STEPS, code) for code in BUDGET_CODES for done in BUDGET_DONE for form in ("budget", "mirror")]
    else:
        calls += [Call("budget", STALE, 0, MAX_STEPS, rows_auto(100, 4)), Call("budget", STALE, MAX_STEPS, MAX_STEPS, rows_auto(100, 4)),
                  Call("mirror", STALE, MAX_STEPS - 1, MAX_STEPS, 4), Call("mirror", STALE, MAX_STEPS + 3, MAX_STEPS, rows_auto(2048, 4))]
    return calls


def compact_call(case, call, mutate=None):
    return compact(call.form, case.bound, case.count, case.alive_old, case.t_old, call.base, call.steps_done, call.max_steps, call.code, mutate)


# ------------------------------------------------------------------------------------------------------------------------------ compositing
def new_acc(N):
    """weights_sum, depth [N], image [N, 3] and the magnitudes their errors scale with (units of u)"""
    return dict(ws=np.zeros(N), depth=np.zeros(N), image=np.zeros((N, 3)), ws_mag=np.zeros(N), depth_mag=np.zeros(N), image_mag=np.zeros((N, 3)))


def acc_from(ws, depth, image):
    """given float32 accumulators: exact, magnitudes zero"""
    a = new_acc(len(ws))
    a["ws"], a["depth"], a["image"] = np.asarray(ws, F8).copy(), np.asarray(depth, F8).copy(), np.asarray(image, F8).reshape(-1, 3).copy()
    return a


COMPOSITE_MUTATIONS = ("T_after", "break_before", "depth_t_before", "by_index", "ignore_stop", "keep_rays_t")


def composite64(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, acc, mutate=None):
    """-> (rays_t after the call [len(rays_t)] float32, the accumulators after the call, decisions).  `acc` is not modified.  decisions:
    (T, tolerance of weights_sum there) float64 arrays over every sample that was accumulated.  mutate: one of COMPOSITE_MUTATIONS."""
    assert mutate is None or mutate in COMPOSITE_MUTATIONS
    out = {k: v.copy() for k, v in acc.items()}
    rays_t = np.array(rays_t, F4)
    if n_alive == 0:
        return rays_t, out, (np.zeros(0), np.zeros(0))
    idx = np.asarray(rays_alive[:n_alive], np.int64)
    slot = idx % n_alive if mutate == "by_index" else np.arange(n_alive)
    sg = np.asarray(sigmas, F8).reshape(-1)
    c8, d8 = np.asarray(rgbs, F8).reshape(-1, 3), np.asarray(deltas, F8).reshape(-1, 2)
    d1_32 = np.asarray(deltas, F4).reshape(-1, 2)[:, 1]
    S, D, I = out["ws"][idx], out["depth"][idx], out["image"][idx]
    eS, eD, eI = out["ws_mag"][idx], out["depth_mag"][idx], out["image_mag"][idx]
    T = 1.0 - S
    t = rays_t[slot].copy()
    active, early = np.ones(n_alive, bool), np.zeros(n_alive, bool)
    dec_T, dec_tol = [], []
    for i in range(n_step):
        row = slot * n_step + i
        if mutate != "ignore_stop":
            stop = active & (d8[row, 0] == 0)
            early |= stop
            active &= ~stop
        if mutate == "break_before":
            cut = active & (T < T_CUT)
            early |= cut
            active &= ~cut
        on = np.nonzero(active)[0]
        if on.size == 0:
            break
        r = row[on]
        x = sg[r] * d8[r, 0]
        f, a = np.exp(-x), -np.expm1(-x)
        Tn = T[on]
        w = a * (Tn * f if mutate == "T_after" else Tn)
        da = a + (E_EXP + x) * f
        dw = Tn * da + a * eS[on] + 2.0 * w
        t_before = t[on].astype(F8)
        t[on] = (t[on] + d1_32[r]).astype(F4)
        tt = t_before if mutate == "depth_t_before" else t[on].astype(F8)
        e_before = eS[on]
        S[on] = S[on] + w
        eS[on] = f * eS[on] + Tn * da + 2.0 * w + np.abs(S[on])
        D[on] = D[on] + w * tt
        eD[on] = eD[on] + np.abs(tt) * dw + np.abs(D[on])
        I[on] = I[on] + w[:, None] * c8[r]
        eI[on] = eI[on] + c8[r] * dw[:, None] + np.abs(I[on])
        dec_T.append(Tn.copy())
        dec_tol.append(tolerance(np.maximum(e_before, eS[on])))
        T[on] = Tn * f
        if mutate != "break_before":
            cut = np.zeros(n_alive, bool)
            cut[on] = Tn < T_CUT
            early |= cut
            active &= ~cut
    new_t = np.where(early & (mutate != "keep_rays_t"), F4(-1.0), t).astype(F4)
    rays_t[slot] = new_t
    out["ws"][idx], out["depth"][idx], out["image"][idx] = S, D, I
    out["ws_mag"][idx], out["depth_mag"][idx], out["image_mag"][idx] = eS, eD, eI
    return rays_t, out, (np.concatenate(dec_T) if dec_T else np.zeros(0), np.concatenate(dec_tol) if dec_tol else np.zeros(0))


def emulate32(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, ws, depth, image):
    """composite_rays_kernel in float32, slot by slot -> (rays_t, weights_sum, depth, image) after the call; the inputs are not modified."""
    rays_t, ws, depth, image = np.array(rays_t, F4), np.array(ws, F4), np.array(depth, F4), np.array(image, F4).reshape(-1, 3)
    sg, c, dl = np.asarray(sigmas, F4).reshape(-1), np.asarray(rgbs, F4).reshape(-1, 3), np.asarray(deltas, F4).reshape(-1, 2)
    one = F4(1.0)
    for n in range(n_alive):
        index = int(rays_alive[n])
        t, S, d, rgb = rays_t[n], ws[index], depth[index], image[index].copy()
        step = 0
        while step < n_step:
            r = n * n_step + step
            if dl[r, 0] == 0:
                break
            alpha = one - exp32(-sg[r] * dl[r, 0])
            T = one - S
            w = F4(alpha * T)
            S = F4(S + w)
            t = F4(t + dl[r, 1])
            d = _fmaf(w, t, d)
            rgb = _fmaf(w, c[r], rgb)
            if float(T) < T_CUT:
                break
            step += 1
        rays_t[n] = F4(-1.0) if step < n_step else t
        ws[index], depth[index], image[index] = S, d, rgb
    return rays_t, ws, depth, image


def n_step_of(code, count, mutate=None):
    """the rows per slot every kernel of an iteration derives.  mutate "stride_from_code": the F of the code, whatever the count"""
    if mutate == "stride_from_code" and code >> 31:
        return (code >> 24) & 127
    return unit_rows(code, count, mutate)


# N rays; the launch is sized by `bound`, `count` slots are alive; code: n_step (plain or AUTO), n_step: what it comes to.  rays_alive, rays_t
# [bound]; sigmas [bound n_step], rgbs [.., 3], deltas [.., 2] (the rows behind count n_step hold plausible samples nobody may read);
# ws, depth [N], image [N, 3]: the accumulators on entry.  kinds [count]: what each slot's ray is.
CompositeCase = namedtuple("CompositeCase", "name N bound count code n_step rays_alive rays_t sigmas rgbs deltas ws depth image kinds")
KINDS = ("thin", "wall_mid", "wall_last", "wall_first", "stop0", "stop_mid", "stop_last", "tail", "zero_sigma")
N_ALIVE = (1, 63, 64, 65, 129)
N_STEP = (1, 4, 8, 32)


def _composite_case(name, count, code, order, carried, slack, seed, shift):
    rng = np.random.default_rng(seed)
    n_step = unit_rows(code, count)
    bound = count + slack
    N = 2 * bound + 3
    if order == "reversed":
        ids = (N - 1 - np.arange(bound)).astype(np.int32)
    else:  # strided
        ids = (1 + 2 * np.arange(bound)).astype(np.int32)
    rows = bound * n_step
    d0 = rng.uniform(0.003, 0.03, rows).astype(F4)
    d1 = rng.uniform(0.003, 0.04, rows).astype(F4)
    x = rng.uniform(0.01, 0.2, rows)
    if carried:
        ws = rng.uniform(0.05, 0.6, N).astype(F4)
        depth = (ws * rng.uniform(0.5, 2.0, N)).astype(F4)
        image = (ws[:, None] * rng.uniform(0, 1, (N, 3))).astype(F4)
    else:
        ws, depth, image = np.zeros(N, F4), np.zeros(N, F4), np.zeros((N, 3), F4)
    kinds = []
    for n in range(count):
        kind = KINDS[(n + shift) % len(KINDS)]
        o = n * n_step
        T0 = 1.0 - float(ws[ids[n]])
        share = rng.uniform(0.05, 1.0, n_step)
        x[o:o + n_step] = rng.uniform(0.1, 3.0) * share / share.sum()  # thin: total optical depth <= 3
        mid = n_step // 2
        if kind == "wall_mid" and n_step >= 2:
            x[o:o + mid] *= 0.3
            x[o + mid] = rng.uniform(20, 40)
        elif kind == "wall_last" and n_step >= 2:
            x[o + n_step - 1] = rng.uniform(20, 40)
        elif kind == "wall_first":
            x[o] = rng.uniform(20, 40)
        elif kind == "stop0":
            d0[o] = 0.0
        elif kind == "stop_mid" and n_step >= 3:
            d0[o + mid] = 0.0
        elif kind == "stop_last" and n_step >= 2:
            d0[o + n_step - 1] = 0.0
        elif kind == "tail" and n_step >= 2:
            # sample j - 1 takes T from >= 1e-2 down to about 5e-5; sample j (alpha about 1) must still add its weight, and is the last
            j = min(n_step - 1, 1 + n % 3)
            x[o:o + j - 1] = rng.uniform(0.01, 0.1, j - 1)
            T_before = T0 * np.exp(-x[o:o + j - 1].sum())
            assert T_before >= 1e-2
            x[o + j - 1] = np.log(T_before / 5e-5)
            x[o + j] = 20.0
        elif kind == "zero_sigma":
            x[o:o + n_step] = 0.0
        else:
            kind = "thin"
        kinds.append(kind)
    sigmas = np.where(d0 > 0, x / np.where(d0 > 0, d0, 1).astype(F8), 1.0).astype(F4)
    rays_t = rng.uniform(0.2, 3.0, bound).astype(F4)
    arrays = (ids, rays_t, sigmas, rng.uniform(0, 1, (rows, 3)).astype(F4), np.stack([d0, d1], axis=1), ws, depth, image)
    for a in arrays:
        a.setflags(write=False)
    return CompositeCase(name, N, bound, count, code, n_step, *arrays, tuple(kinds))


_composite = []


def composite_cases():
    """Every (n_alive, n_step) twice -- reversed alive list, zero accumulators, count = bound; strided list, carried-in accumulators, count 7 below
    the bound -- and three AUTO codes that come to F, 8 F and a value between."""
    if not _composite:
        j = 0
        for n_alive in N_ALIVE:
            for n_step in N_STEP:
                _composite.append(_composite_case(f"a{n_alive}-s{n_step}-reversed", n_alive, n_step, "reversed", False, 0, 9000 + j, j))
                _composite.append(_composite_case(f"a{n_alive}-s{n_step}-strided-carried-slack", n_alive, n_step, "strided", True, 7, 9500 + j, j + 4))
                j += 1
        for name, count, code, slack in (("auto-F", 129, rows_auto(129, 4), 0), ("auto-between", 65, rows_auto(325, 4), 7), ("auto-8F", 3, rows_auto(100, 4), 61),
                                         ("auto-F-slack", 64, rows_auto(50, 3), 1)):
            _composite.append(_composite_case(name, count, code, "strided", True, slack, 9900 + j, j))
            j += 1
        assert [c.n_step for c in _composite[-4:]] == [4, 20, 32, 3]
    return _composite


def composite_case(name):
    return next(c for c in composite_cases() if c.name == name)


def composite_reference(case, mutate=None):
    """composite64 of a case -> (rays_t, acc, decisions); a stride mutation changes the rows a slot reads"""
    n_step = case.n_step
    if mutate == "stride_from_code":
        n_step = n_step_of(case.code, case.count, mutate)
        mutate = None
    return composite64(case.count, n_step, case.rays_alive, case.rays_t, case.sigmas, case.rgbs, case.deltas, acc_from(case.ws, case.depth, case.image), mutate)


def acc_ratios(got_ws, got_depth, got_image, acc, rays=None):
    """worst |got - float64| / tolerance per output over `rays` (default: all)"""
    out = {}
    for name, got in (("ws", got_ws), ("depth", got_depth), ("image", got_image)):
        want, mag = acc[name], acc[name + "_mag"]
        got = np.asarray(got, F8).reshape(want.shape)
        err = np.abs(got - want)
        r = np.where(np.isnan(err), np.inf, err / tolerance(mag))
        if rays is not None:
            r = r[rays]
        out[name] = float(r.max()) if r.size else 0.0
    return out


# ------------------------------------------------------------------------------------------------------------------------------ the loop case
LOOP_N, LOOP_F, LOOP_H = 193, 4, 128
LOOP_CODE = rows_auto(LOOP_N, LOOP_F)
LOOP_MAX_STEPS = (1024, 40)
LOOP_GRID = "ones"  # the grid the premises are asserted on: every cell occupied, rays live until the wall, the box or the budget ends them
LOOP_GRIDS = ("ones", "scene")  # the sparse scene grid as well: the count and n_step change nearly every iteration, many slots stay unused
PLANE_X, SIGMA_THIN = 1.2, 0.4
SIGMA_WALL = 20.0 / (2.0 * np.sqrt(3.0) / 1024) * 1.01  # >= 20 / dt_min of the finer march: one sample behind the plane is a wall


def standin_field(xyzs):
    """The host stand-in for the field, float32 from the sample positions: a thin constant density in front of the plane x = PLANE_X and a wall
    behind it; rgb = 0.5 + 0.5 sin(3 x) (the sine in float64, rounded once: the same bits on every host)."""
    p = np.asarray(xyzs, F4).reshape(-1, 3)
    sigma = np.where(p[:, 0] > F4(PLANE_X), F4(SIGMA_WALL), F4(SIGMA_THIN)).astype(F4)
    rgb = (0.5 + 0.5 * np.sin(3.0 * p.astype(F8))).astype(F4)
    return sigma, rgb


def loop_rays(oracle):
    """o, d, nears, fars of the loop case: march_cases.rays(193) without its degenerate rays, and ray 7 replaced by one that misses the box -- it
    dies in the first iteration, which leaves 192 = 3 x 64 alive for the iterations that follow"""
    import march_cases as mc

    o, d = (a.copy() for a in mc.rays(LOOP_N, degenerate=False))
    o[7], d[7] = [5.0, 5.0, 5.0], [0.6, 0.64, 0.48]
    nears, fars = oracle.near_far_from_aabb(o, d, mc.AABB, mc.MIN_NEAR)
    return o, d, nears, fars


# per iteration: count = the alive word the compaction left (0: the loop is over), steps = the step word, n_step; rays_alive, rays_t [count] after
# the compaction; xyzs, dirs, deltas: the oracle's march [count n_step, .]; rays_t_out [count] after compositing; acc: the accumulators after it
LoopIteration = namedtuple("LoopIteration", "count survivors steps n_step rays_alive rays_t xyzs dirs deltas sigmas rgbs rays_t_out acc decisions")
_loops = {}


def loop_model(oracle, max_steps, arithmetic="float64", grid=None, limit=400):
    """The loop through the model -> list of LoopIteration (the last one has count 0).  arithmetic "emulate32": the accumulators walked by
    emulate32 (acc then holds float32 values and no magnitudes) -- for the CPU check of the carried bound."""
    grid = LOOP_GRID if grid is None else grid
    key = (max_steps, arithmetic, grid)
    if key in _loops:
        return _loops[key]
    import march_cases as mc

    bits = mc.grid(grid, LOOP_H)
    o, d, nears, fars = loop_rays(oracle)
    N = LOOP_N
    alive_old, t_old, count, steps = np.arange(N, dtype=np.int32), nears.astype(F4).copy(), N, 0
    acc = new_acc(N)
    if arithmetic == "emulate32":
        acc = dict(ws=np.zeros(N, F4), depth=np.zeros(N, F4), image=np.zeros((N, 3), F4))
    out = []
    for _ in range(limit):
        res = compact("mirror", N, count, alive_old, t_old, steps_done=steps, max_steps=max_steps, code=LOOP_CODE)
        if res.steps is not None:
            steps = res.steps
        k = res.counter
        alive, t = res.alive[:k].copy(), res.t[:k].copy()
        if k == 0:
            out.append(LoopIteration(0, res.k, steps, unit_rows(LOOP_CODE, 0), alive, t, None, None, None, None, None, None, acc, None))
            break
        n_step = unit_rows(LOOP_CODE, k)
        xyzs, dirs, deltas = oracle.march_rays(k, n_step, alive, t, o, d, mc.BOUND, bits, mc.CASCADES, LOOP_H, nears, fars, dt_gamma=mc.DT_GAMMA,
                                               max_steps=max_steps)
        sigmas, rgbs = standin_field(xyzs)
        if arithmetic == "emulate32":
            t_out, ws, dp, im = emulate32(k, n_step, alive, t, sigmas, rgbs, deltas, acc["ws"], acc["depth"], acc["image"])
            acc, dec = dict(ws=ws, depth=dp, image=im), None
        else:
            t_out, acc, dec = composite64(k, n_step, alive, t, sigmas, rgbs, deltas, acc)
        out.append(LoopIteration(k, res.k, steps, n_step, alive, t, xyzs, dirs, deltas, sigmas, rgbs, t_out, acc, dec))
        alive_old, t_old, count = alive, t_out, k
    else:
        raise AssertionError("the loop did not end")
    _loops[key] = out
    return out
