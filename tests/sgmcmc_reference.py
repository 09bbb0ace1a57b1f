"""Float64 numpy restatement of blm_sgmcmc_update (include/bayeslm.h, csrc/sgmcmc.hip) and of the cyclical schedule
(bayeslms_amd/sgmcmc.py): the inputs are the fp32 arrays and the fp32 scalars the kernel gets, every operation on them runs in
float64, nothing is rounded to fp32 on the way.  ``update`` returns, beside the new p (and v), the bound the kernel is held to:
derived from the rounded fp32 operations behind each output and evaluated per element from the float64 magnitudes of the terms,
with a factor 2 over the derivation, as tests/swag_reference.py derives its own.  u = 2^-24, the relative error of one rounded fp32
operation; sqrt and the division are correctly rounded (u each).  Nothing here was tuned on the kernel's output.

The derivation, e_x the absolute error of x before the factor 2:
  c    sqrt(sq) (u), times grad_scale (u), plus 1e-6 (u, and the constant's own rounding: below u), clip / that (u), the minimum,
       times grad_scale (u): at most 6 u |c| with the constant's.  blm_clip_sgd_multi may contract sqrt(sq) * gs + 1e-6 into one
       fma, which removes a rounding: the same bound covers it.
  d    = (c g) + (wd p):  e_d = 7 u |c g| + u |wd p| + u |d|            (c's 6 u and the product's own; wd is handed in as fp32)
  sgld   t = lr d:  e_t = lr e_d + u |t|;   q = p - t:  e_q = e_t + u |q|;   n = sigma xi:  e_n = u |n| + sigma e_xi
         p' = q + n:  e_p = e_q + e_n + u |p'|
  psgld  a = alpha v (u |a|);  m = ((1 - alpha) d) d, 1 - alpha rounded once:  e_m = oma (3 u d^2 + 2 |d| e_d) + tiny
         v' = a + m:  e_v = u |a| + e_m + u |v'|
         s = sqrt(v'):  |sqrt(x + e) - sqrt(x)| <= e / sqrt(x), so e_s = e_v / s + u s    (v' = 0 only where d = 0 and v = 0: exact)
         D = damping + s:  e_D = e_s + u D;   G = 1 / D:  e_G = e_D / D^2 + u G
         k = lr G:  e_k = lr e_G + u k;   t = k d:  e_t = |d| e_k + k e_d + u |t|;   q = p - t:  e_q = e_t + u |q|
         r = sqrt(G):  e_r = e_G / r + u r;   w = sigma r:  e_w = sigma e_r + u w;   n = w xi:  e_n = |xi| e_w + u |n| + w e_xi
         p' = q + n:  e_p = e_q + e_n + u |p'|
tiny = 2^-149: a product of two small numbers may land among the subnormals, where the spacing is absolute.

e_xi is the distance of the noise the reference was handed from the noise the kernel generated.  Handed the kernel's own stream
read back through blm_philox_normal it is 0; handed oracle.philox.normal (numpy's logarithm and cosine instead of the device's)
it is XI_ORACLE = 3e-5, the distance tests/test_gpu_kernels.py::test_philox_stream_matches_numpy_oracle holds blm_philox_normal
to that numpy stream to."""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
XI_ORACLE = 3e-5


def f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def f32(x):
    """a scalar as the C ABI takes it: rounded to float32 once"""
    return float(np.float32(x))


def clip_coefficient(sq, clip, grad_scale):
    """c = min(1, clip / (sqrt(sq) grad_scale + 1e-6)) grad_scale from the fp32 scalars -> (c, e_c)"""
    sq, clip, gs = f32(sq), f32(clip), f32(grad_scale)
    c = min(1.0, clip / (math.sqrt(sq) * gs + f32(1e-6))) * gs
    return c, 6 * U * abs(c)


def update(p, g, sq, clip, lr, grad_scale, weight_decay, sigma, xi=None, v=None, alpha=0.99, damping=1e-5, e_xi=0.0):
    """-> (p', v' or None, bound of p', bound of v' or None).  ``xi``: the noise (None with sigma = 0)."""
    p, g = f64(p), f64(g)
    lr, wd, sigma, alpha, damping = f32(lr), f32(weight_decay), f32(sigma), f32(alpha), f32(damping)
    c, e_c = clip_coefficient(sq, clip, grad_scale)
    xi = np.zeros_like(p) if xi is None or sigma == 0.0 else f64(xi)
    if sigma == 0.0:
        e_xi = 0.0
    cg, wp = c * g, wd * p
    d = cg + wp
    e_d = (e_c / max(abs(c), 1e-300) + U) * np.abs(cg) + U * np.abs(wp) + U * np.abs(d)
    if v is None:
        t = lr * d
        q = p - t
        n = sigma * xi
        out = q + n
        e_p = lr * e_d + U * np.abs(t) + U * np.abs(q) + U * np.abs(n) + sigma * e_xi + U * np.abs(out)
        return out, None, 2 * e_p, None
    v = f64(v)
    oma = f32(1.0 - alpha)  # the launcher's 1.0f - alpha
    a = alpha * v
    m = oma * d * d
    e_m = oma * (3 * U * d * d + 2 * np.abs(d) * e_d) + TINY
    vn = a + m
    e_v = U * np.abs(a) + e_m + U * np.abs(vn)
    s = np.sqrt(vn)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_s = np.where(vn > 0, e_v / s, 0.0) + U * s
    D = damping + s
    G = 1.0 / D
    e_G = (e_s + U * D) / (D * D) + U * G
    k = lr * G
    e_k = lr * e_G + U * k
    t = k * d
    e_t = np.abs(d) * e_k + k * e_d + U * np.abs(t)
    q = p - t
    r = np.sqrt(G)
    e_r = e_G / r + U * r
    w = sigma * r
    e_w = sigma * e_r + U * w
    n = w * xi
    e_n = np.abs(xi) * e_w + U * np.abs(n) + w * e_xi
    out = q + n
    e_p = e_t + U * np.abs(q) + e_n + U * np.abs(out)
    return out, vn, 2 * e_p, 2 * e_v


# ------------------------------------------------------------------ host side
def sampler_coefficients(lr, temperature, prior_precision, n_tokens):
    """-> (weight_decay, sigma): tau / N and float32(sqrt(2 lr T / N)) formed in double"""
    return prior_precision / n_tokens, f32(math.sqrt(2.0 * lr * temperature / n_tokens))


def cyclical(k, total_steps, cycles, lr0, explore=0.8):
    """Zhang et al. 2020, eq. 1 -> (rate, sampling) of step k (1-based); cycles = 0: (lr0, True)"""
    if cycles == 0:
        return lr0, True
    L = -(-total_steps // cycles)
    r = ((k - 1) % L) / L
    return lr0 / 2.0 * (math.cos(math.pi * r) + 1.0), r >= explore
