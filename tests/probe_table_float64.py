"""TEST INFRASTRUCTURE: the per-probe visibility fit in float64 on given points (tests/test_probe_table_cpu.py, tests/test_gpu_probe_table.py).

  basis9     the nine order-2 bases, with the polynomials and signs the fit evaluates (sh_light_model.py:22-30's constants), float64
  fit        fit_product_of_SHs' loop on points [rounds, batch, 3]: gt_c = (Y . sh1_c)(Y . lobe), pred_c = Y . sh_c, the gradient
             2 / batch Y^T (pred - gt) ADDED to the running gradient (the reference never clears it; zero_grad=True clears it, to show
             that the tests tell the two apart), torch's single-tensor Adam.  tests/test_probe_table_cpu.py holds it to the reference's own
             float64 run on the same points.
  tolerance  what a fp32 implementation on the same points is held to: 8 x the reference's own fp32-against-float64 gap on such a stream
             (g_replay at 40 x 96, g_full at 800 x 1024; both from the fixture) + 1e-6.  The margin of 8: the device sums a round's terms as a
             tree, the framework vectorised, and the gap was seen on a few probes only.
"""
import numpy as np

C0, C1 = 0.28209479177387814, 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)


def basis9(p):
    """[N, 3] -> [N, 9] float64."""
    p = np.asarray(p, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([np.full_like(x, C0), -C1 * y, C1 * z, -C1 * x, C2[0] * x * y, C2[1] * y * z, C2[2] * (2.0 * z * z - x * x - y * y), C2[3] * x * z,
                     C2[4] * (x * x - y * y)], axis=-1)


def fit(env_shs, lobe, points, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, zero_grad=False):
    """env_shs [>= 9, 3], lobe [9], points [rounds, batch, 3] -> [9, 3] float64."""
    sh1 = np.asarray(env_shs, np.float64)[:9]
    lobe = np.asarray(lobe, np.float64)
    sh, g_run, m, v = sh1.copy(), np.zeros((9, 3)), np.zeros((9, 3)), np.zeros((9, 3))
    for t, pts in enumerate(np.asarray(points), start=1):
        Y = basis9(pts)
        gt = (Y @ sh1) * (Y @ lobe)[:, None]
        g = (2.0 / Y.shape[0]) * (Y.T @ (Y @ sh - gt))
        g_run = g if zero_grad else g_run + g
        m = m + (g_run - m) * (1 - beta1)
        v = v * beta2 + (1 - beta2) * g_run * g_run
        denom = np.sqrt(v) / (1 - beta2 ** t) ** 0.5 + eps
        sh = sh + (-(lr / (1 - beta1 ** t))) * m / denom
    return sh


def tolerance(gap):
    return 8.0 * float(gap) + 1e-6
