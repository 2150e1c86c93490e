"""TEST INFRASTRUCTURE: float64 restatements of the FFMLP and of the fused ngp field, for tests/test_gpu_mlp_batch_sweep.py (and checked
against the oracle by tests/test_mlp_float64_cpu.py).  Plain torch on whatever device the tensors live on.

Every value is exact float64 except where the kernels -- and the reference's ffmlp.cu -- store a 16-bit value: hidden activations, outputs
and per-layer gradients are rounded to the storage type T, and so are the derivative factors of sigmoid, squareplus and softplus
(utils.h:537-582, K_ACT = 10).  What remains between this and the kernels is the order of their fp32 accumulations.  The backward follows
the reference, not calculus: the output activation is not differentiated (ffmlp.cu:781), and sine has no backward there (its fragment is
left unwritten), so it has none here.

Weight layout (ffmlp/ffmlp.py): one flat vector [W0 (H x IN) | W1 .. W_{NL-1} (H x H) | W_out (16 x H)], row-major [out, in].
Along with every weight gradient the backward returns sum_n |dPre[n, o] In[n, i]| and sum_n (dPre[n, o] In[n, i])^2 in float64 (as
`terms` [2, n_params]): the scales that bounds on an fp32 summation of those terms, and on ulp-sized differences of a random subset of
them, are proportional to.
"""
import torch

F64 = torch.float64
K_ACT = 10.0
EPS32 = 2.0 ** -24  # unit roundoff of fp32
CHUNK = 1 << 15     # rows per pass: the float64 intermediates of a 459264-row batch are computed a slice at a time


def rnd(x, dtype):
    """float64 -> the storage type -> float64."""
    return x.to(dtype).to(F64)


def act_forward(a, x):
    if a == 0:
        return x.clamp_min(0.0)
    if a == 1:
        return torch.exp(x)
    if a == 2:
        return torch.sin(x)
    if a == 3:
        return 1.0 / (1.0 + torch.exp(-x))
    if a == 4:
        s = x * K_ACT
        return 0.5 * (s + torch.sqrt(s * s + 4.0)) / K_ACT
    if a == 5:
        return torch.log(torch.exp(x * K_ACT) + 1.0) / K_ACT
    return x


def act_backward(a, g, y, dtype):
    """dL/dpre from the (already rounded) dL/dpost g and the stored post-activation y."""
    if a == 0:
        return torch.where(y > 0, g, torch.zeros_like(g))
    if a == 1:
        return g * y
    if a == 2:
        raise ValueError("sine has no backward in the reference (ffmlp.cu leaves its fragment unwritten)")
    if a == 3:
        return g * rnd(y * (1.0 - y), dtype)
    if a == 4:
        s = y * K_ACT
        return g * rnd(s * s / (s * s + 1.0), dtype)
    if a == 5:
        return g * rnd(1.0 - torch.exp(-y * K_ACT), dtype)
    return g


def n_params(IN, H, NL):
    return H * (IN + H * (NL - 1) + 16)


def split_weights(w, IN, H, NL):
    """[W0, W1 .. W_{NL-1}, W_out] as float64 [out, in] views of the flat vector."""
    w = w.to(F64)
    mats, o = [], 0
    for a, b in [(H, IN)] + [(H, H)] * (NL - 1) + [(16, H)]:
        mats.append(w[o:o + a * b].view(a, b))
        o += a * b
    assert o == w.numel()
    return mats


def _slope(a, y):
    """a bound on |d act / d pre| at the stored value y: y for the exponential, 1 for the others"""
    return y.abs() if a == 1 else 1.0


def mlp_forward(x, mats, act, out_act, dtype, mags=None):
    """x [n, IN] float64 (T-valued) -> (outputs [n, 16], [post-activations of hidden layer 0 .. NL-1]), all T-valued float64.
    mags (a list): receives, per hidden layer and then for the outputs, the magnitude of each value's dot product, sum_k |W[o, k] in[k]|
    times the activation's slope -- the scale at which different roundings of the layer's inputs move the value."""
    ys, h = [], x
    for W in mats[:-1]:
        pre = h @ W.t()
        hn = rnd(act_forward(act, pre), dtype)
        if mags is not None:
            mags.append((h.abs() @ W.abs().t()) * _slope(act, hn))
        h = hn
        ys.append(h)
    out = rnd(act_forward(out_act, h @ mats[-1].t()), dtype)
    if mags is not None:
        mags.append((h.abs() @ mats[-1].abs().t()) * _slope(out_act, out))
    return out, ys


def mlp_backward(g, x, mats, ys, act, dtype):
    """g [n, 16] T-valued.  Returns (dL/dx unrounded [n, IN], [dW per matrix], [(sum |terms|, sum terms^2) per matrix], [dPre per hidden
    layer 0 .. NL-1], sum_k |dPre_0[k] W0[k, i]| per element of dL/dx)."""
    NL = len(ys)
    gw, terms, dpres = [None] * (NL + 1), [None] * (NL + 1), [None] * NL
    gw[NL] = g.t() @ ys[-1]
    terms[NL] = torch.stack([g.abs().t() @ ys[-1].abs(), (g * g).t() @ (ys[-1] * ys[-1])])
    d = g @ mats[NL]
    for l in reversed(range(NL)):
        dpre = rnd(act_backward(act, rnd(d, dtype), ys[l], dtype), dtype)
        dpres[l] = dpre
        inp = ys[l - 1] if l > 0 else x
        gw[l] = dpre.t() @ inp
        terms[l] = torch.stack([dpre.abs().t() @ inp.abs(), (dpre * dpre).t() @ (inp * inp)])
        d = dpre @ mats[l]
    return d, gw, terms, dpres, dpres[0].abs() @ mats[0].abs()


def mlp_reference(x, w, IN, H, NL, act, out_act, dtype, g=None, keep_hidden=False, hidden=None, chunk=CHUNK):
    """The whole batch a slice at a time.  x [B, IN] and w in T (any float type holding T values), g [B, 16] or None.
    Returns a dict: out [B, 16] float64 with its magnitudes out_mag (float32, see mlp_forward); hidden [NL, B, H] in T and hidden_mag
    (fp16, to keep a 459264 x 256 network's in memory) with keep_hidden; with g: grad_inputs [B, IN] (rounded to T) float64 and its
    magnitudes grad_inputs_mag (float32), gw / terms [n_params] float64.
    hidden [NL, B, H] (T): the kernel's stored activations, for the backward to start from.  Where a value near a rounding boundary (or a
    ReLU input near zero) comes out differently in fp32 and float64, the two backward passes would otherwise differ by a whole term."""
    mats = split_weights(w, IN, H, NL)
    B = x.shape[0]
    res = {"out": torch.empty(B, 16, dtype=F64, device=x.device), "out_mag": torch.empty(B, 16, device=x.device)}
    if keep_hidden:
        res["hidden"] = torch.empty(NL, B, H, dtype=dtype, device=x.device)
        res["hidden_mag"] = torch.empty(NL, B, H, dtype=torch.float16, device=x.device)
    if g is not None:
        res["grad_inputs"] = torch.empty(B, IN, dtype=F64, device=x.device)
        res["grad_inputs_mag"] = torch.empty(B, IN, device=x.device)
        res["gw"] = torch.zeros(n_params(IN, H, NL), dtype=F64, device=x.device)
        res["terms"] = torch.zeros(2, n_params(IN, H, NL), dtype=F64, device=x.device)
    for s in range(0, B, chunk):
        e = min(B, s + chunk)
        xs = x[s:e].to(F64)
        mags = []
        out, ys = mlp_forward(xs, mats, act, out_act, dtype, mags)
        res["out"][s:e], res["out_mag"][s:e] = out, mags[-1]
        if keep_hidden:
            for l, y in enumerate(ys):
                res["hidden"][l, s:e] = y.to(dtype)
                res["hidden_mag"][l, s:e] = mags[l].clamp_max(6e4)
        if g is not None:
            if hidden is not None:
                ys = [hidden[l, s:e].to(F64) for l in range(NL)]
            d, gw, terms, _, dmag = mlp_backward(g[s:e].to(F64), xs, mats, ys, act, dtype)
            res["grad_inputs"][s:e], res["grad_inputs_mag"][s:e] = rnd(d, dtype), dmag
            res["gw"] += torch.cat([m.reshape(-1) for m in gw])
            res["terms"] += torch.cat([m.reshape(2, -1) for m in terms], dim=1)
    return res


# ------------------------------------------------------------------------------------------------------------------------- the ngp field
def sh4(d):
    """Real spherical harmonics up to degree 4 (16 values) of unit directions [n, 3], written out in float64 (tiny-cuda-nn's basis, the
    reference's shencoder)."""
    x, y, z = d.to(F64).unbind(-1)
    xy, yz, xz = x * y, y * z, x * z
    x2, y2, z2 = x * x, y * y, z * z
    return torch.stack([
        torch.full_like(x, 0.28209479177387814),
        -0.48860251190291987 * y,
        0.48860251190291987 * z,
        -0.48860251190291987 * x,
        1.0925484305920792 * xy,
        -1.0925484305920792 * yz,
        0.94617469575755997 * z2 - 0.31539156525251999,
        -1.0925484305920792 * xz,
        0.54627421529603959 * x2 - 0.54627421529603959 * y2,
        0.59004358992664352 * y * (-3.0 * x2 + y2),
        2.8906114426405538 * xy * z,
        0.45704579946446572 * y * (1.0 - 5.0 * z2),
        0.3731763325901154 * z * (5.0 * z2 - 3.0),
        0.45704579946446572 * x * (1.0 - 5.0 * z2),
        1.4453057213202769 * z * (x2 - y2),
        0.59004358992664352 * x * (-x2 + 3.0 * y2),
    ], dim=-1)


SIGMA_NET = (32, 64, 2)   # (IN, H, NL): features -> 64 -> 64 -> 16, ReLU
COLOUR_NET = (32, 64, 3)  # [SH16 | geo15 | 0] -> 64 -> 64 -> 64 -> 16, ReLU


def field_forward(feats_lbc, dirs, ws, wc, dtype, chunk=CHUNK):
    """feats_lbc [16, B, 2] fp16 (level-major), dirs [B, 3] fp32, the two weight vectors in T.  The composition of ngp_harness/model.py:
    sigma net -> trunc_exp(h0) -> degree-4 SH of dirs -> cin = [SH16, geo15, 0] -> colour net -> sigmoid.  Side outputs rounded as the
    kernel stores them: x_rows, h, cin in T; rgbs T-valued.  Returns float64 tensors."""
    B = dirs.shape[0]
    ms, mc = split_weights(ws, *SIGMA_NET), split_weights(wc, *COLOUR_NET)
    res = {k: torch.empty(B, n, dtype=F64, device=dirs.device) for k, n in (("x_rows", 32), ("h", 16), ("cin", 32), ("rgbs", 3))}
    for k, n in (("h_mag", 16), ("cin_mag", 32), ("rgbs_mag", 3)):
        res[k] = torch.empty(B, n, device=dirs.device)
    res["sigma"] = torch.empty(B, dtype=F64, device=dirs.device)
    for s in range(0, B, chunk):
        e = min(B, s + chunk)
        x = rnd(feats_lbc[:, s:e].to(F64).permute(1, 0, 2).reshape(e - s, 32), dtype)  # row n: level l channel c at 2 l + c
        mh, mo = [], []
        h, _ = mlp_forward(x, ms, 0, 6, dtype, mh)
        sh = rnd(sh4(dirs[s:e]), dtype)
        cin = torch.cat([sh, h[:, 1:], torch.zeros_like(h[:, :1])], dim=1)
        hc, _ = mlp_forward(cin, mc, 0, 6, dtype, mo)
        res["x_rows"][s:e], res["h"][s:e], res["cin"][s:e] = x, h, cin
        res["h_mag"][s:e] = mh[-1]
        res["cin_mag"][s:e] = torch.cat([torch.ones_like(sh), mh[-1][:, 1:], torch.zeros_like(h[:, :1])], dim=1)  # SH: O(1) polynomials
        res["rgbs_mag"][s:e] = 0.25 * mo[-1][:, :3]  # sigmoid: slope <= 1/4
        res["sigma"][s:e] = torch.exp(h[:, 0])
        res["rgbs"][s:e] = rnd(torch.sigmoid(hc[:, :3]), dtype)
    return res


def field_backward(grad_sigma, grad_rgbs, rgbs, h, cin, x_rows, ws, wc, dtype, hidden_s=None, hidden_c=None, chunk=CHUNK):
    """The backward of field_forward from the saved side outputs (float64, T-valued).  The colour net's output gradient is the framework's
    sigmoid backward on 16-bit tensors, (g (1 - y)) y with every operation rounded to T; the sigma net's is [grad_sigma exp(clamp(h0, -15,
    15)) (trunc_exp), grad_cin[:, 16:31]].  Returns grad_cin and grad_x (T-valued; grad_x of the bf16 field also rounded to fp16, the hash
    table's type) and per network the weight gradient and its sum of |terms|.  hidden_s / hidden_c: the networks' activations as the kernels
    compute them (see mlp_reference)."""
    B = rgbs.shape[0]
    ms, mc = split_weights(ws, *SIGMA_NET), split_weights(wc, *COLOUR_NET)
    dev = rgbs.device
    res = {"grad_cin": torch.empty(B, 32, dtype=F64, device=dev), "grad_x": torch.empty(B, 32, dtype=F64, device=dev),
           "grad_cin_mag": torch.empty(B, 32, device=dev), "grad_x_mag": torch.empty(B, 32, device=dev)}
    for k, spec in (("s", SIGMA_NET), ("c", COLOUR_NET)):
        res["gw_" + k] = torch.zeros(n_params(*spec), dtype=F64, device=dev)
        res["terms_" + k] = torch.zeros(2, n_params(*spec), dtype=F64, device=dev)
    for s in range(0, B, chunk):
        e = min(B, s + chunk)
        y = rgbs[s:e].to(F64)
        u = rnd(rnd(grad_rgbs[s:e].to(F64), dtype) * rnd(1.0 - y, dtype), dtype)
        g_hc = torch.zeros(e - s, 16, dtype=F64, device=dev)
        g_hc[:, :3] = rnd(u * y, dtype)
        c_in = cin[s:e].to(F64)
        _, ys = mlp_forward(c_in, mc, 0, 6, dtype)
        if hidden_c is not None:
            ys = [y[s:e].to(F64) for y in hidden_c]
        d, gw, terms, _, dmag = mlp_backward(g_hc, c_in, mc, ys, 0, dtype)
        gcin = rnd(d, dtype)
        res["grad_cin"][s:e], res["grad_cin_mag"][s:e] = gcin, dmag
        res["gw_c"] += torch.cat([m.reshape(-1) for m in gw])
        res["terms_c"] += torch.cat([m.reshape(2, -1) for m in terms], dim=1)
        h0 = h[s:e, 0].to(F64)
        col0 = rnd(grad_sigma[s:e].to(F64) * torch.exp(h0.clamp(-15.0, 15.0)), dtype)
        g_h = torch.cat([col0[:, None], gcin[:, 16:31]], dim=1)
        xs = x_rows[s:e].to(F64)
        _, ys = mlp_forward(xs, ms, 0, 6, dtype)
        if hidden_s is not None:
            ys = [y[s:e].to(F64) for y in hidden_s]
        d, gw, terms, _, dmag = mlp_backward(g_h, xs, ms, ys, 0, dtype)
        gx = rnd(d, dtype)
        res["grad_x_mag"][s:e] = dmag
        res["grad_x"][s:e] = gx if dtype == torch.float16 else rnd(gx, torch.float16)
        res["gw_s"] += torch.cat([m.reshape(-1) for m in gw])
        res["terms_s"] += torch.cat([m.reshape(2, -1) for m in terms], dim=1)
    return res
