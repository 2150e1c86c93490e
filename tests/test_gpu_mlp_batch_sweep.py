"""FFMLP and the fused ngp field against float64 (tests/mlp_float64.py) at the batch sizes where the persistent grids go round more than once.

Every MLP kernel walks the batch in 128-row blocks with a grid capped by the CU count (ffmlp_body.inc):
  forward / inference / field forward   persistent_grid: min(B / 128, nCU * per_cu), per_cu <= 4 (1 with knob ffmlp_wg_per_cu = 1)
  fused backward, field backward        launch_fused:    min(B / 128, nCU) workgroups, one fp32 partial each, then the reduction
  split backward (dgrad + wgrad)        wgrad:           min(B / 128, nCU / 2)
so the block counts below sit on both sides of each cap, up to the benchmark's 459264 rows (3588 blocks).

Per case:
  * dense output gradient: outputs, hidden activations and input gradients row by row -- every element of every row within ROW_ULPS
    storage ulps of max(|ref|, its dot product's sum|terms|), no fraction allowed to fail; weight gradients within C_WGRAD eps32 sum|terms|
    + eps_T (|ref| + sqrt(sum terms^2)) (see C_WGRAD);
  * block probe: the output gradient is zero but on four 32-row steps weighted 1, 2, 4, 8 -- the first step, the last step of workgroup
    n_parts - 1, the first step of the second sweep and the last step of the batch.  A lost, doubled or misattributed step moves a weight
    gradient far beyond the bound (each case checks that the bound rejects the reference without its weight-1 step), and the input
    gradient of every other row must be exactly zero;
  * every output is filled with NaN first, so a row a kernel skips fails; every call runs twice and must repeat its bits.
The worst |got - ref| / tolerance of each group is printed at the end of the module (pytest -s).
"""
import pytest
import torch

import mlp_float64 as ref

pytestmark = pytest.mark.gpu

F16, BF16, F64 = torch.float16, torch.bfloat16, torch.float64
EPS = {F16: 2.0 ** -10, BF16: 2.0 ** -7}  # storage epsilon: 10 / 7 stored significand bits
BENCH_BLOCKS = 3588  # bench.py's 459264 rows
# A stored value's dot product sum_k W[o, k] in[k] runs over 16-bit inputs that the kernel rounded from fp32 and the reference from float64:
# where the two land on either side of a rounding boundary the inputs differ by an ulp, which moves the value by up to an ulp of its
# sum_k |W[o, k] in[k]| (mlp_float64.mlp_forward's magnitudes) -- near zero that, not |ref|, is the scale of an honest difference.
ROW_ULPS = 2.0
# The kernels sum a weight gradient in fp32 along a chain of at most ~90 roundings: one 32-deep MFMA contraction per step (<= 32), the
# steps of one wave (<= 28 at 3588 blocks), the 4-wave combine (2), one slice of the partials in the reduction (<= 32 of 256) and the 8 slices
# (8).  To first order such a sum is off by at most (chain length) eps32 sum|terms|; C_WGRAD = 128 covers that chain.  The final rounding
# to the storage type is the "+ 1 storage ulp" of |ref|.  And the 16-bit dPre the kernel rounds from fp32 and the reference from float64
# differ by an ulp where the two straddle a rounding boundary: a sparse random subset of the terms moves by up to eps_T |term| with random
# signs, for which eps_T sqrt(sum terms^2) is allowed on top.  It matters where few rows contribute (the probes: measured up to 3.8x the
# other two terms), and it is far below what one lost probe step moves (each case asserts that the bound sees it).
C_WGRAD = 128

BLOCKS = ["1", "ncu/2+1", "ncu-1", "ncu", "ncu+1", "4ncu+3", "bench"]  # ascending for any CU count up to 896


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count  # the source device_cus() reads too


def _blocks(label):
    n = _ncu()
    return {"1": 1, "ncu/2+1": n // 2 + 1, "ncu-1": n - 1, "ncu": n, "ncu+1": n + 1, "4ncu+3": 4 * n + 3, "bench": BENCH_BLOCKS}[label]


WORST = {}


def _note(group, v):
    WORST[group] = max(WORST.get(group, 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nworst |got - ref| / tolerance per group:")
        for k in sorted(WORST):
            print(f"  {k:58s} {WORST[k]:.4f}")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import nerftex_hip  # noqa: F401

    return torch.device("cuda:0")


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _uniform(shape, lo, hi, gen, dtype):
    return (torch.rand(shape, generator=gen, device="cuda") * (hi - lo) + lo).to(dtype)


def _randn(shape, scale, gen, dtype):
    return (torch.randn(shape, generator=gen, device="cuda") * scale).to(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------- checks
def _row_chunks(n, chunk=1 << 16):
    return [(s, min(n, s + chunk)) for s in range(0, n, chunk)]


def _check_rows(group, name, got, want, mag, dtype, rows=None, ulps=ROW_ULPS):
    """got [n, ...] (any type), want [n, ...] float64 (or T), mag: the magnitude of each value's dot product.  Every element within
    ulps eps_T max(|want|, mag).  A NaN -- a row the kernel did not write -- fails.  rows: the batch row of each got row (for the message)."""
    n = got.shape[0]
    got, want, mag = got.reshape(n, -1), want.reshape(n, -1), mag.reshape(n, -1)
    worst, bad_rows = 0.0, []
    for s, e in _row_chunks(n):
        w = want[s:e].to(F64)
        tol = ulps * EPS[dtype] * torch.maximum(w.abs(), mag[s:e].to(F64))
        err = (got[s:e].to(F64) - w).abs()
        ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / tol.clamp_min(1e-300))
        worst = max(worst, float(ratio.max()))
        bad = (ratio > 1).any(dim=1).nonzero()[:, 0] + s
        bad_rows += bad[:8].tolist()
    _note(group, worst)
    if bad_rows:
        rr = [int(rows[i]) if rows is not None else i for i in bad_rows[:8]]
        raise AssertionError(f"{name}: rows {rr} (blocks {[r // 128 for r in rr]}) beyond {ulps} storage ulps; worst ratio {worst:.3g}")


def _wgrad_ratio(got, want, terms, dtype):
    """terms [2, n]: sum |terms|, sum terms^2 (mlp_float64.mlp_backward)"""
    tol = C_WGRAD * ref.EPS32 * terms[0] + EPS[dtype] * (want.abs() + terms[1].sqrt()) + (2.0 ** -24 if dtype == F16 else 0.0)  # (+ fp16's subnormal spacing)
    err = (got.to(F64) - want).abs()
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / tol.clamp_min(1e-300))
    return float(ratio.max())


def _check_wgrad(group, name, got, want, terms, dtype):
    worst = _wgrad_ratio(got, want, terms, dtype)
    _note(group, worst)
    assert worst <= 1.0, f"{name}: weight gradient beyond {C_WGRAD} eps32 sum|terms| + eps_T (|ref| + sqrt(sum terms^2)) (worst ratio {worst:.3g})"


def _probe_steps(B, n_parts):
    """{32-row step: weight}: the first step, the last of workgroup n_parts - 1, the first of the second sweep, the last of the batch."""
    steps = {}
    for s, wt in ((0, 1), (4 * n_parts - 1, 2), (4 * n_parts, 4), (B // 32 - 1, 8)):
        if s < B // 32 and s not in steps:
            steps[s] = wt
    return steps


def _probe_grad(g, steps):
    gp = torch.zeros_like(g)
    for s, wt in steps.items():
        gp[32 * s:32 * s + 32] = g[32 * s:32 * s + 32] * wt  # powers of two: exact
    return gp


def _rows_of(steps):
    return torch.cat([torch.arange(32 * s, 32 * s + 32, device="cuda") for s in sorted(steps)])


def _assert_bound_rejects(got, want, terms, dtype, name):
    """the self-check of a probe: the reference WITHOUT the weight-1 step must fail the bound the kernel passed"""
    assert _wgrad_ratio(got, want, terms, dtype) > 1.0, f"{name}: the bound does not see a lost probe step"


# ------------------------------------------------------------------------------------------------------------------------------ FFMLP calls
def _fns(dtype):
    from nerftex_hip import lib

    s = "" if dtype == F16 else "_bf16"
    return getattr(lib, "nerftex_ffmlp_forward" + s), getattr(lib, "nerftex_ffmlp_inference" + s), getattr(lib, "nerftex_ffmlp_backward" + s)


def _forward(dtype, x, w, IN, H, NL, act, out_act, inference):
    from nerftex_hip import check, ptr, stream

    fwd, inf, _ = _fns(dtype)
    B = x.shape[0]
    out = _nan((B, 16), dtype)
    fb = None if inference else _nan((NL, B, H), dtype)
    if inference:
        check(inf(ptr(x), ptr(w), B, IN, 16, H, NL, act, out_act, None, ptr(out), stream()))
    else:
        check(fwd(ptr(x), ptr(w), B, IN, 16, H, NL, act, out_act, ptr(fb), ptr(out), stream()))
    torch.cuda.synchronize()
    return out, fb


def _backward(dtype, g, x, w, fb, IN, H, NL, act, out_act, cgi):
    from nerftex_hip import check, ptr, stream

    B = x.shape[0]
    gi, gw = _nan((B, IN), dtype), _nan(tuple(w.shape), dtype)
    bb = _nan((NL, B, H), dtype) if fb is not None else None
    check(_fns(dtype)[2](ptr(g), ptr(x), ptr(w), ptr(fb), B, IN, 16, H, NL, act, out_act, int(cgi), ptr(bb), ptr(gi), ptr(gw), stream()))
    torch.cuda.synchronize()
    return gi, gw, bb


def _mlp_problem(IN, H, NL, act, B, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    bound = (3.0 / H) ** 0.5 * (0.25 if act == 1 else 1.0)  # a chain of exponentials stays in range
    w = _uniform((ref.n_params(IN, H, NL),), -bound, bound, gen, dtype)
    x = _uniform((B, IN), -1.0, 1.0, gen, dtype)  # a different row everywhere: a misplaced row cannot match by accident
    g = _randn((B, 16), 0.05, gen, dtype)
    return x, w, g


def _fused_instantiated(IN, H, NL):
    return H == 64 and 2 <= NL <= 4 and IN % 16 == 0 and IN <= 64


def _run_mlp_case(knobs, group, IN, H, NL, act, out_act, dtype, blocks, backward, seed):
    n = _ncu()
    B = 128 * blocks
    x, w, g = _mlp_problem(IN, H, NL, act, B, dtype, seed)
    want = ref.mlp_reference(x, w, IN, H, NL, act, out_act, dtype, keep_hidden=True)
    out, fb = _forward(dtype, x, w, IN, H, NL, act, out_act, False)
    _check_rows(f"{group} outputs", "forward outputs", out, want["out"], want["out_mag"], dtype)
    for l in range(NL):
        _check_rows(f"{group} hidden", f"forward_buffer[{l}]", fb[l], want["hidden"][l], want["hidden_mag"][l], dtype)
    del want["hidden"], want["hidden_mag"]
    out2, fb2 = _forward(dtype, x, w, IN, H, NL, act, out_act, False)
    assert torch.equal(out2, out) and torch.equal(fb2, fb), "forward: a second call gives other bits"
    inf, _ = _forward(dtype, x, w, IN, H, NL, act, out_act, True)
    assert torch.equal(inf, out), "inference must equal the training forward bit for bit"
    if not backward:
        return
    # the backward reference starts from the kernel's activations, checked above (see mlp_float64.mlp_reference)
    want = ref.mlp_reference(x, w, IN, H, NL, act, out_act, dtype, g=g, hidden=fb)
    fused = _fused_instantiated(IN, H, NL)
    variants = ([("stored", fb, 0), ("recompute", None, 0)] if fused else []) + [("split", fb, 1)]
    bits = {}
    for name, fbuf, split in variants:
        knobs(ffmlp_bwd_split=split)
        n_parts = min(blocks, n // 2 if split or not fused else n)
        gi, gw, bb = _backward(dtype, g, x, w, fbuf, IN, H, NL, act, out_act, True)
        _check_rows(f"{group} grad_inputs", f"{name} grad_inputs", gi, want["grad_inputs"], want["grad_inputs_mag"], dtype)
        _check_wgrad(f"{group} grad_weights", f"{name} grad_weights", gw, want["gw"], want["terms"], dtype)
        gi2, gw2, _ = _backward(dtype, g, x, w, fbuf, IN, H, NL, act, out_act, True)
        assert torch.equal(gi2, gi) and torch.equal(gw2, gw), f"{name}: a second call gives other bits"
        gi0, gw0, _ = _backward(dtype, g, x, w, fbuf, IN, H, NL, act, out_act, False)
        assert torch.equal(gw0, gw), f"{name}: calc_grad_inputs = 0 changes the weight gradient"
        assert torch.isnan(gi0).all(), f"{name}: calc_grad_inputs = 0 wrote grad_inputs"
        if bb is not None:
            if split:
                assert not torch.isnan(bb).any(), "split: backward_buffer has rows the dgrad kernel did not write"
            else:
                assert torch.isnan(bb).all(), "the fused backward must not touch backward_buffer"
        bits[name] = (gi, gw)

        # block probe
        steps = _probe_steps(B, n_parts)
        gp = _probe_grad(g, steps)
        rows = _rows_of(steps)
        pr = ref.mlp_reference(x[rows], w, IN, H, NL, act, out_act, dtype, g=gp[rows], hidden=fb[:, rows])
        gi, gw, _ = _backward(dtype, gp, x, w, fbuf, IN, H, NL, act, out_act, True)
        _check_wgrad(f"{group} probe grad_weights", f"{name} probe grad_weights (steps {steps})", gw, pr["gw"], pr["terms"], dtype)
        _check_rows(f"{group} probe grad_inputs", f"{name} probe grad_inputs", gi[rows], pr["grad_inputs"], pr["grad_inputs_mag"], dtype, rows=rows)
        outside = torch.ones(B, dtype=torch.bool, device="cuda")
        outside[rows] = False
        assert (gi[outside] == 0).all(), f"{name}: non-zero input gradient outside the probe steps {steps}"
        first = [s for s, wt in steps.items() if wt == 1]
        kept = _rows_of({s: wt for s, wt in steps.items() if wt != 1})
        pr1 = ref.mlp_reference(x[kept], w, IN, H, NL, act, out_act, dtype, g=gp[kept], hidden=fb[:, kept])
        assert first, steps
        _assert_bound_rejects(gw, pr1["gw"], pr1["terms"], dtype, name)
    if "recompute" in bits:
        assert all(torch.equal(a, b) for a, b in zip(bits["stored"], bits["recompute"])), "recompute != stored activations"
    knobs(ffmlp_bwd_split=0)


FIELD_NETS = [(32, 64, 2), (32, 64, 3)]  # the ngp field's sigma and colour networks
SWEEP = []
for _i, _b in enumerate(BLOCKS):
    for _net in FIELD_NETS:
        for _dt in (F16, BF16):
            SWEEP.append((_i, 1, _b, _net, _dt, True, False))
    if _b == "ncu+1":
        for _net in FIELD_NETS:
            for _dt in (F16, BF16):
                SWEEP.append((_i, 0, _b, _net, _dt, False, True))  # forward looping at a small size: one workgroup per CU
    if _b in ("ncu+1", "bench"):
        SWEEP += [(_i, 2, _b, (32, 256, 3), F16, False, False), (_i, 2, _b, (64, 128, 6), F16, False, False),
                  (_i, 3, _b, (32, 256, 2), F16, True, False)]  # the streamed forms, and hidden 256 through the split backward
SWEEP.sort(key=lambda c: (c[0], c[1]))


def _sweep_id(c):
    _, _, b, (IN, H, NL), dt, bwd, wg1 = c
    return f"{b}-in{IN}_h{H}_L{NL}-{'fp16' if dt == F16 else 'bf16'}{'-fwdbwd' if bwd else '-fwd'}{'-wg1' if wg1 else ''}"


@pytest.mark.parametrize("case", SWEEP, ids=[_sweep_id(c) for c in SWEEP])
def test_ffmlp_batch_sweep(dev, knobs, case):
    _, _, label, (IN, H, NL), dtype, backward, wg1 = case
    if wg1:
        knobs(ffmlp_wg_per_cu=1)
    group = f"mlp {'fp16' if dtype == F16 else 'bf16'} h{H}"
    _run_mlp_case(knobs, group, IN, H, NL, 0, 6, dtype, _blocks(label), backward, seed=100 + 7 * NL + H + IN)


ACTS = [(F16, a, 6) for a in range(7)] + [(F16, 0, oa) for oa in (0, 1, 3, 4, 5)] + [(BF16, a, 6) for a in (1, 3, 4, 5)]


@pytest.mark.parametrize("dtype,act,out_act", ACTS, ids=[f"{'fp16' if d == F16 else 'bf16'}-act{a}-out{o}" for d, a, o in ACTS])
def test_ffmlp_activations(dev, knobs, dtype, act, out_act):
    """blocks = nCU + 1, 64 hidden, 3 layers: every hidden activation with its backward (sine: forward only -- the reference defines no
    backward for it), the output activations in forward and inference."""
    group = f"act {'fp16' if dtype == F16 else 'bf16'} act{act} out{out_act}"
    _run_mlp_case(knobs, group, 32, 64, 3, act, out_act, dtype, _blocks("ncu+1"), act != 2 and out_act == 6, seed=300 + 10 * act + out_act)


# ------------------------------------------------------------------------------------------------------------------------------ the field
def _field_fns(dtype):
    from nerftex_hip import lib

    if dtype == F16:
        return dict(fwd=lib.nerftex_field_forward, rows=lib.nerftex_field_forward_rows, density=lib.nerftex_field_density,
                    bwd=lambda *a: lib.nerftex_field_backward(*a[:-2], a[-1]), amp=lib.nerftex_field_backward_amp,
                    live=lib.nerftex_field_backward_live, consume=lib.nerftex_field_backward_live_consume)
    return dict(fwd=lib.nerftex_field_forward_bf16, rows=lib.nerftex_field_forward_rows_bf16, density=lib.nerftex_field_density_bf16,
                bwd=lib.nerftex_field_backward_bf16, amp=lib.nerftex_field_backward_bf16, live=lib.nerftex_field_backward_live_bf16,
                consume=lib.nerftex_field_backward_live_consume_bf16)


def _field_problem(B, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    b = (3.0 / 64) ** 0.5
    ws = _uniform((ref.n_params(*ref.SIGMA_NET),), -b, b, gen, dtype)
    wc = _uniform((ref.n_params(*ref.COLOUR_NET),), -b, b, gen, dtype)
    feats = _uniform((16, B, 2), -1.0, 1.0, gen, F16)  # level-major, fp16 whatever the networks compute in
    dirs = torch.nn.functional.normalize(torch.randn(B, 3, generator=gen, device="cuda"), dim=-1)
    gs = _randn((B,), 0.05, gen, torch.float32)
    gr = _randn((B, 3), 0.05, gen, torch.float32)
    return ws, wc, feats, dirs, gs, gr


def _field_backward(fns, kind, dtype, gs, gr, saved, ws, wc, flags=None, found=None):
    from nerftex_hip import check, ptr, stream

    rgbs, h, cin, x = saved
    B = rgbs.shape[0]
    gcin, gx = _nan((B, 32), dtype), _nan((B, 32), F16)
    gws, gwc = _nan(tuple(ws.shape), dtype), _nan(tuple(wc.shape), dtype)
    common = [ptr(gs), ptr(gr), ptr(rgbs), ptr(h), ptr(cin), ptr(x), ptr(ws), ptr(wc), B, ptr(gcin), ptr(gx), ptr(gws), ptr(gwc)]
    if kind in ("bwd", "amp"):
        check(fns[kind](*common, ptr(found), stream()))
    elif kind == "live":
        check(fns[kind](*common, ptr(flags), ptr(found), stream()))
    else:
        check(fns[kind](*common, ptr(flags), None, ptr(found), stream()))
    torch.cuda.synchronize()
    return gcin, gx, gws, gwc


def _check_field_grads(group, name, got, want, dtype, rows=None):
    gcin, gx, gws, gwc = got
    sel = slice(None) if rows is None else rows
    _check_rows(f"{group} grad_cin", f"{name} grad_cin", gcin[sel], want["grad_cin"], want["grad_cin_mag"], dtype, rows=rows)
    _check_rows(f"{group} grad_x", f"{name} grad_x", gx[sel], want["grad_x"], want["grad_x_mag"], dtype, rows=rows)
    _check_wgrad(f"{group} grad_weights", f"{name} sigma-net grad_weights", gws, want["gw_s"], want["terms_s"], dtype)
    _check_wgrad(f"{group} grad_weights", f"{name} colour-net grad_weights", gwc, want["gw_c"], want["terms_c"], dtype)


FIELD_CASES = [(b, dt) for b in ("ncu+1", "bench") for dt in (F16, BF16)]


@pytest.mark.parametrize("label,dtype", FIELD_CASES, ids=[f"{b}-{'fp16' if d == F16 else 'bf16'}" for b, d in FIELD_CASES])
def test_field_against_float64(dev, label, dtype):
    from nerftex_hip import check, ptr, stream

    n = _ncu()
    blocks = _blocks(label)
    B = 128 * blocks
    group = f"field {'fp16' if dtype == F16 else 'bf16'}"
    fns = _field_fns(dtype)
    ws, wc, feats, dirs, gs, gr = _field_problem(B, dtype, 500 + blocks)
    want = ref.field_forward(feats, dirs, ws, wc, dtype)

    # ---- forward (training), then the no-grad forms against it
    sigma, rgbs = _nan((B,), torch.float32), _nan((B, 3), torch.float32)
    x_rows, h, cin, hc = _nan((B, 32), dtype), _nan((B, 16), dtype), _nan((B, 32), dtype), _nan((B, 16), dtype)
    check(fns["fwd"](ptr(feats), ptr(dirs), ptr(ws), ptr(wc), B, ptr(sigma), ptr(rgbs), ptr(x_rows), ptr(h), ptr(cin), ptr(hc), stream()))
    torch.cuda.synchronize()
    assert torch.equal(x_rows.to(F64), want["x_rows"]), "x_rows: the features as rows, narrowed to the networks' type"
    _check_rows(f"{group} h", "h", h, want["h"], want["h_mag"], dtype)
    _check_rows(f"{group} cin", "cin", cin, want["cin"], want["cin_mag"], dtype)
    _check_rows(f"{group} rgbs", "rgbs", rgbs, want["rgbs"], want["rgbs_mag"], dtype)
    # sigma = exp(h0): its logarithm is held to h0's bound (fp32 exp adds ~1e-7 relative)
    _check_rows(f"{group} log sigma", "log sigma", torch.log(sigma.to(F64)), want["h"][:, 0], want["h_mag"][:, 0], dtype)
    assert torch.isfinite(hc).all()

    s2, r2 = _nan((B,), torch.float32), _nan((B, 3), torch.float32)
    check(fns["fwd"](ptr(feats), ptr(dirs), ptr(ws), ptr(wc), B, ptr(s2), ptr(r2), None, None, None, None, stream()))
    s3 = _nan((B,), torch.float32)
    check(fns["density"](ptr(feats), ptr(ws), B, ptr(s3), stream()))
    units = blocks - 3 if blocks > 3 else blocks  # the device count: units of 128 rows; rows past it are not computed
    units_dev = torch.tensor([units], dtype=torch.int32, device="cuda")
    s4, r4 = _nan((B,), torch.float32), _nan((B, 3), torch.float32)
    check(fns["rows"](ptr(feats), ptr(dirs), ptr(ws), ptr(wc), B, ptr(s4), ptr(r4), ptr(units_dev), 128, stream()))
    torch.cuda.synchronize()
    assert torch.equal(s2, sigma) and torch.equal(r2, rgbs), "field inference != training forward"
    assert torch.equal(s3, sigma), "field density != training forward's sigma"
    live_rows = 128 * units
    assert torch.equal(s4[:live_rows], sigma[:live_rows]) and torch.equal(r4[:live_rows], rgbs[:live_rows]), "forward_rows != training forward"
    assert torch.isnan(s4[live_rows:]).all() and torch.isnan(r4[live_rows:]).all(), "forward_rows wrote rows past the device count"

    # ---- backward from the reference's side outputs (T-valued), dense
    saved = (want["rgbs"].float(), want["h"].to(dtype), want["cin"].to(dtype), want["x_rows"].to(dtype))
    # the networks' activations as the kernels compute them: the recomputing backward runs the forward kernel's chain verbatim
    hs = _forward(dtype, saved[3], ws, *ref.SIGMA_NET, 0, 6, False)[1]
    hcn = _forward(dtype, saved[2], wc, *ref.COLOUR_NET, 0, 6, False)[1]
    wb = ref.field_backward(gs, gr, *(t.to(F64) for t in saved), ws, wc, dtype, hs, hcn)
    plain = _field_backward(fns, "bwd", dtype, gs, gr, saved, ws, wc)
    _check_field_grads(group, "field_backward", plain, wb, dtype)
    again = _field_backward(fns, "bwd", dtype, gs, gr, saved, ws, wc)
    assert all(torch.equal(a, b) for a, b in zip(again, plain)), "field backward: a second call gives other bits"
    found = torch.zeros(1, dtype=torch.float32, device="cuda")
    amp = _field_backward(fns, "amp", dtype, gs, gr, saved, ws, wc, found=found)
    assert all(torch.equal(a, b) for a, b in zip(amp, plain)) and float(found) == 0.0, "_amp on finite gradients"
    gs_inf = gs.clone()
    gs_inf[B - 1] = float("inf")  # the last row of the last block
    _field_backward(fns, "amp", dtype, gs_inf, gr, saved, ws, wc, found=found)
    assert float(found) == 1.0, "_amp: an inf in grad_sigma of the batch's last row did not set found_inf"

    # ---- block probe on grad_sigma and grad_rgbs
    steps = _probe_steps(B, min(blocks, n))
    rows = _rows_of(steps)
    gsp, grp = _probe_grad(gs, steps), _probe_grad(gr, steps)
    sub = tuple(t[rows].to(F64) for t in saved)
    wp = ref.field_backward(gsp[rows], grp[rows], *sub, ws, wc, dtype, hs[:, rows], hcn[:, rows])
    probe = _field_backward(fns, "bwd", dtype, gsp, grp, saved, ws, wc)
    _check_field_grads(f"{group} probe", f"probe {steps}", probe, wp, dtype, rows=rows)
    outside = torch.ones(B, dtype=torch.bool, device="cuda")
    outside[rows] = False
    assert (probe[0][outside] == 0).all() and (probe[1][outside] == 0).all(), f"non-zero input gradients outside the probe steps {steps}"
    kept = _rows_of({s: wt for s, wt in steps.items() if wt != 1})
    wp1 = ref.field_backward(gsp[kept], grp[kept], *(t[kept].to(F64) for t in saved), ws, wc, dtype, hs[:, kept], hcn[:, kept])
    _assert_bound_rejects(probe[2], wp1["gw_s"], wp1["terms_s"], dtype, "field sigma net")
    _assert_bound_rejects(probe[3], wp1["gw_c"], wp1["terms_c"], dtype, "field colour net")

    # ---- step flags: random, all dead, all live.  The reference zeroes the gradients of the dead steps
    gen = torch.Generator(device="cuda").manual_seed(7 + blocks)
    for kind in ("random", "dead", "live"):
        if kind == "random":
            flags = (torch.rand(B // 32, generator=gen, device="cuda") < 0.5).to(torch.int32)
        else:
            flags = torch.full((B // 32,), int(kind == "live"), dtype=torch.int32, device="cuda")
        row_live = flags.repeat_interleave(32).bool()
        z = row_live.to(torch.float32)
        wl = ref.field_backward(gs * z, gr * z[:, None], *(t.to(F64) for t in saved), ws, wc, dtype, hs, hcn)
        found.zero_()
        got = _field_backward(fns, "live", dtype, gs, gr, saved, ws, wc, flags=flags, found=found)
        lr = row_live.nonzero()[:, 0]
        name = f"live ({kind} flags)"
        if lr.numel():
            _check_rows(f"{group} grad_cin", f"{name} grad_cin", got[0][lr], wl["grad_cin"][lr], wl["grad_cin_mag"][lr], dtype, rows=lr)
        _check_rows(f"{group} grad_x", f"{name} grad_x", got[1], wl["grad_x"], wl["grad_x_mag"], dtype)
        assert (got[1][~row_live] == 0).all(), f"{name}: grad_x of dead steps must be written as exact zeros"
        _check_wgrad(f"{group} grad_weights", f"{name} sigma-net grad_weights", got[2], wl["gw_s"], wl["terms_s"], dtype)
        _check_wgrad(f"{group} grad_weights", f"{name} colour-net grad_weights", got[3], wl["gw_c"], wl["terms_c"], dtype)
        assert float(found) == 0.0
        if kind == "live":
            assert all(torch.equal(a, b) for a, b in zip(got, plain)), "all steps live != the plain backward"
        fl = flags.clone()
        con = _field_backward(fns, "consume", dtype, gs, gr, saved, ws, wc, flags=fl, found=found)
        assert not fl.any(), f"{name}: _live_consume must leave every flag 0"
        assert torch.equal(con[1], got[1]) and torch.equal(con[2], got[2]) and torch.equal(con[3], got[3]), f"{name}: consume != live"
        assert torch.equal(con[0][lr], got[0][lr])


# --------------------------------------------------------------------------------------------------------------- scratch reuse
def test_small_batch_after_bench_batch_repeats_its_bits(dev, knobs):
    """The weight-gradient partials live in grow-only library scratch: a 3588-block call in between must not change a small call's bits."""
    n = _ncu()
    IN, H, NL = 32, 64, 3

    def run(blocks):
        B = 128 * blocks
        x, w, g = _mlp_problem(IN, H, NL, 0, B, F16, 900)
        _, fb = _forward(F16, x, w, IN, H, NL, 0, 6, False)
        res = []
        for fbuf, split in ((fb, 0), (None, 0), (fb, 1)):
            knobs(ffmlp_bwd_split=split)
            res += list(_backward(F16, g, x, w, fbuf, IN, H, NL, 0, 6, True)[:2])
        knobs(ffmlp_bwd_split=0)
        fns = _field_fns(F16)
        ws, wc, feats, dirs, gs, gr = _field_problem(B, F16, 901)
        want = ref.field_forward(feats, dirs, ws, wc, F16)
        saved = (want["rgbs"].float(), want["h"].half(), want["cin"].half(), want["x_rows"].half())
        res += list(_field_backward(fns, "bwd", F16, gs, gr, saved, ws, wc))
        return res

    small = run(n + 1)
    run(BENCH_BLOCKS)
    again = run(n + 1)
    assert all(torch.equal(a, b) for a, b in zip(small, again)), "a small call after a bench-size call gives other bits"
