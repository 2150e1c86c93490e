"""The float64 restatements of tests/mlp_float64.py (the references of test_gpu_mlp_batch_sweep.py) against the oracle, on the CPU: the same
roundings -- hidden activations, outputs, per-layer gradients and the derivative factors stored in 16 bits -- for every activation, in
fp16 and bf16 storage, and the same degree-4 SH basis.  The oracle accumulates in double too, so what is left is the odd 16-bit value
that lands on the other side of a rounding boundary."""
import numpy as np
import pytest
import torch

import mlp_float64 as ref


def test_sh4_matches_the_oracle(oracle):
    rng = np.random.default_rng(0)
    d = rng.standard_normal((2000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    want, _ = oracle.sh_encode_forward(d, 4)
    np.testing.assert_allclose(ref.sh4(torch.from_numpy(d)).numpy(), want, rtol=0, atol=2e-6)


def _frac_beyond(got, want, ulps, eps, floor):
    return float(np.mean(np.abs(got - want) > ulps * eps * np.maximum(np.abs(want), floor)))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4, 5, 6])
def test_mlp_reference_matches_the_oracle(oracle, act, bf16):
    IN, H, NL, B = 32, 64, 3, 512
    rng = np.random.default_rng(10 + act)
    wscale = 0.25 if act == 1 else 1.0  # keeps a chain of exponentials in range
    w = (rng.uniform(-1, 1, ref.n_params(IN, H, NL)) * np.sqrt(3.0 / H) * wscale).astype(np.float32)
    x = rng.uniform(-1, 1, (B, IN)).astype(np.float32)
    g = (rng.standard_normal((B, 16)) * 0.05).astype(np.float32)
    dtype, eps = (torch.bfloat16, 2.0 ** -7) if bf16 else (torch.float16, 2.0 ** -10)
    wt, xt, gt = (torch.from_numpy(a).to(dtype) for a in (w, x, g))
    out_act = 3 if act == 0 else 6
    want = ref.mlp_reference(xt, wt, IN, H, NL, act, out_act, dtype, g=None if act == 2 else gt, keep_hidden=True)

    def to_orc(t):
        return oracle.to_bf16(t.float().numpy()) if bf16 else t.numpy()

    def from_orc(a):
        return oracle.from_bf16(a).astype(np.float64) if bf16 else a.astype(np.float64)

    ctx = oracle.ffmlp_bf16() if bf16 else torch.no_grad()
    with ctx:
        o_out, o_fb = oracle.ffmlp_forward(to_orc(xt), to_orc(wt), IN, 16, H, NL, act, out_act)
        if act != 2:
            o_gw, o_gi, _ = oracle.ffmlp_backward(to_orc(gt), to_orc(xt), to_orc(wt), o_fb, IN, 16, H, NL, act, True)
    hidden = want["hidden"].float().numpy()
    # the first layer sees identical inputs: exact sums, one rounding each -> identical bits but for double-rounding ties
    assert _frac_beyond(hidden[0], from_orc(o_fb[0]), 1.01, eps, 1e-3) < 1e-3
    for l in range(1, NL):
        assert _frac_beyond(hidden[l], from_orc(o_fb[l]), 2.0, eps, 1e-2) < 1e-3
    assert _frac_beyond(want["out"].numpy(), from_orc(o_out), 2.0, eps, 5e-2) < 2e-3
    if act == 2:
        return
    gw, o_gw = want["gw"].numpy(), from_orc(o_gw)
    np.testing.assert_allclose(gw, o_gw, rtol=0, atol=4 * eps * np.abs(o_gw).max())
    gi, o_gi = want["grad_inputs"].numpy(), from_orc(o_gi)
    np.testing.assert_allclose(gi, o_gi, rtol=0, atol=4 * eps * np.abs(o_gi).max())
    assert (want["terms"][0].numpy() >= np.abs(gw) * (1 - 1e-12)).all()
