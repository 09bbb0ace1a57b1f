"""Float64 restatement of the weight-update kernels (csrc/elementwise.hip, csrc/search.hip), with running error bounds.

One plain numpy function per operation.  The inputs are the float32 arrays the kernel sees, cast up; the hyper-parameters are
rounded to float32 first (the C ABI takes ``float``) and everything after that is float64.  Every output comes with a
MAGNITUDE: the same expression with each term replaced by its absolute value.  A float32 evaluation of the expression with K
roundings on its longest path is within ``K * U * magnitude`` of the exact value (U = 2^-24, the unit roundoff), element by
element, so the GPU tests (tests/test_gpu_update_kernels.py) bound the error per element and never by a global maximum.
The constants K below are counted from the kernel source, not measured; each carries its count.  A fused multiply-add only
removes a rounding, so the counts hold with and without contraction.

tests/test_update_reference_cpu.py checks these functions against torch in float64.
"""
import numpy as np

U = 2.0 ** -24  # unit roundoff of float32 (round to nearest)

# ---------------------------------------------------------------------------------------------------------------- constants
# blm_sqnorm_multi: every term g*g is >= 0, so the bound is relative to the sum and K is the longest chain of roundings one
# term goes through.  sqnorm_multi_kernel: one product (1), then per vector round of a lane 4 additions (3 inside the quad and
# the `a +=`), plus at most one scalar-tail element (1), the wave butterfly (6), the four waves of the block (4); sum_kernel:
# ceil(partials / 1024) additions per lane, its butterfly (6), its sixteen waves (16), and the final `out[0] +=` (1).
#   n == 1 (1024 blocks): 3,200,003 floats are 800,000 quads over 262,144 lanes = 4 rounds: 1 + 16 + 1 + 6 + 4 + 1 + 6 + 16 + 1 = 52
#   n == 1, misaligned g (scalar loop): 13 rounds of one addition: 1 + 13 + 6 + 4 + 1 + 6 + 16 + 1 = 48
#   n == 40 (64 blocks each): 200,003 floats are 50,000 quads over 16,384 lanes = 4 rounds, 2560 partials = 3 per lane:
#       1 + 16 + 1 + 6 + 4 + 3 + 6 + 16 + 1 = 54;  scalar: 13 rounds: 1 + 13 + 6 + 4 + 3 + 6 + 16 + 1 = 50
K_SQNORM = 64

# c = fminf(1, clip / (sqrtf(sq) * gs + 1e-6f)) * gs, clipped: half of sq's relative error (32), sqrtf (2: not required to be
# correctly rounded), * gs (1), + 1e-6f (1), the division (2, likewise), * gs (1) = 39.  The c*g term of the new momentum adds
# its product and the two additions behind it (3), the new parameter lr * buf and the subtraction (2): 44 at most.
K_C = 48
# Every other term: mom*buf goes through its product and the outer addition (2) and, in the parameter, lr * buf and the
# subtraction (4).  wd*p goes through its product and two additions (3), 5 in the parameter; p itself through the subtraction
# only (1).  Summed, 5 lr wd |p| + |p| <= 4 (lr wd |p| + |p|) whenever lr * wd <= 3, so 4 on "the others" holds for the sum.
K_TERM = 4
# Unclipped, fminf returns 1.0f and c IS gs (1.0f * gs is exact), so c*g is an ordinary term: product and outer addition in
# the momentum (2; 3 in the weight-decay entry), lr * buf and the subtraction behind them (4; 5 in the weight-decay entry
# without contraction, 4 with the fused multiply-adds hipcc emits for `mom * m + t` and `p - lr * mv`).
K_UNCLIPPED = 4

# blm_adam_step, the update term lr * (m / bc1) / (sqrtf(v / bc2) + eps): bc1 and bc2 rounded to float (1 + 1/2), m / bc1 (2),
# v / bc2 and sqrtf (2 + 2, halved by the root or not: 3), + eps (1), lr * (1), the division (2), the subtraction (1): 13.
K_ADAM = 16
# new m = b1*m + (1-b1)*gv: products (1 each) and the addition (1), the longest path 2; 1 - b1 is exact in float32 for
# 1/2 <= b1 <= 1.  new v = b2*v + ((1-b2)*gv)*gv: two products and the addition: 3.  All terms of v are >= 0.
K_ADAM_M = 4
K_ADAM_V = 4
K_ADAM_GV = 2  # gv = g + wd*p: the product and the addition; exact (gv is g) without weight decay

K_AXPY = 2  # y + a*x: the product and the addition


def colsum_k(M, deterministic=False):
    """Roundings on the longest path of one column sum of blm_colsum / blm_colsum2: the rows one lane adds (grid.y row chunks of
    ceil(M / gy) rows, eight row lanes per chunk), the shared-memory combine of the eight lanes and the scale (8), and one
    atomic addition per row chunk (gy).  gy = min(64, ceil(M / 256)); 1 in deterministic mode."""
    gy = 1 if deterministic else max(1, min(64, (M + 255) // 256))
    rows_per = (M + gy - 1) // gy
    return (rows_per + 7) // 8 + 8 + gy


def f32(x):
    """A hyper-parameter as the C ABI receives it: rounded to float32, then exact in float64."""
    return float(np.float32(x))


def _f64(a):
    a = np.asarray(a)
    assert a.dtype in (np.float32, np.float64), a.dtype
    return a.astype(np.float64)


# --------------------------------------------------------------------------------------------------------------- operations
def sqnorm(grads):
    """sum_i |g_i|^2 over a list of arrays.  Every term is non-negative: the magnitude is the value itself."""
    s = float(sum(float(np.sum(_f64(g) ** 2)) for g in grads))
    return s, s


def clip_sgd(params, grads, bufs, clip, lr, mom, first, grad_scale=1.0, weight_decay=0.0):
    """Global-norm clip + SGD momentum as stated in include/bayeslm.h:
        norm = sqrt(sum |g|^2) * gs;  c = min(1, clip / (norm + 1e-6)) * gs
        buf = (first ? 0 : mom * buf) + c*g + wd*p;  p -= lr * buf
    ``bufs`` is not read when ``first``.  -> dict with
        sq, c, clipped         the squared norm (before gs), the factor on g, and whether the clip is active
        p, buf                 lists of the new parameters / momentum buffers (float64)
        p_mag, buf_mag         their magnitudes
        p_err, buf_err         the per-element float32 error bounds (K_C on the c*g term when clipped, K_TERM on the others;
                               K_UNCLIPPED throughout when not)"""
    clip, lr, mom, gs, wd = f32(clip), f32(lr), f32(mom), f32(grad_scale), f32(weight_decay)
    sq, _ = sqnorm(grads)
    norm = np.sqrt(sq) * gs
    ratio = clip / (norm + f32(1e-6))
    clipped = bool(ratio < 1.0)
    c = min(1.0, ratio) * gs
    k_cg = K_C if clipped else K_UNCLIPPED
    k_t = K_TERM if clipped else K_UNCLIPPED
    out = dict(sq=sq, c=c, clipped=clipped, ratio=ratio, p=[], buf=[], p_mag=[], buf_mag=[], p_err=[], buf_err=[])
    for p, g, b in zip(params, grads, bufs):
        p, g = _f64(p), _f64(g)
        old = np.zeros_like(p) if first else mom * _f64(b)
        cg, wp = c * g, wd * p
        buf = old + cg + wp
        out["buf"].append(buf)
        out["buf_mag"].append(np.abs(old) + np.abs(cg) + np.abs(wp))
        out["buf_err"].append(U * (k_cg * np.abs(cg) + k_t * (np.abs(old) + np.abs(wp))))
        out["p"].append(p - lr * buf)
        out["p_mag"].append(np.abs(p) + lr * out["buf_mag"][-1])
        out["p_err"].append(U * (k_cg * lr * np.abs(cg) + k_t * (lr * (np.abs(old) + np.abs(wp)) + np.abs(p))))
    return out


def adam(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
    """torch.optim.Adam(weight_decay) for one tensor, ``step`` counting from 1:
        gv = g + wd*p;  m = b1*m + (1-b1)*gv;  v = b2*v + (1-b2)*gv^2
        p -= lr * (m / bc1) / (sqrt(v / bc2) + eps),   bc_i = 1 - b_i^step
    -> dict with p, m, v (float64), their magnitudes p_mag, m_mag, v_mag, and the float32 error bounds p_err, m_err, v_err.
    p_err is K_ADAM on the update term plus one rounding on p, plus the momentum's own absolute bound and the second moment's
    interval carried through 1 / bc1 / (sqrt(v / bc2) + eps)."""
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    bc1, bc2 = 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)
    gv = g + wd * p
    gv_mag = np.abs(g) + np.abs(wd * p)
    gv_err = K_ADAM_GV * U * gv_mag if wd != 0.0 else np.zeros_like(gv)
    m1 = b1 * m + (1.0 - b1) * gv
    m_mag = np.abs(b1 * m) + (1.0 - b1) * gv_mag
    m_err = K_ADAM_M * U * m_mag + (1.0 - b1) * gv_err
    v1 = b2 * v + (1.0 - b2) * gv * gv
    v_mag = np.abs(b2 * v) + (1.0 - b2) * gv_mag ** 2
    # the interval of the float32 second moment: gv anywhere within its bound, then K_ADAM_V relative roundings
    v_hi = (b2 * v + (1.0 - b2) * (np.abs(gv) + gv_err) ** 2) * (1.0 + K_ADAM_V * U)
    v_lo = (b2 * v + (1.0 - b2) * np.maximum(np.abs(gv) - gv_err, 0.0) ** 2) * (1.0 - K_ADAM_V * U)
    v_err = np.maximum(v_hi - v1, v1 - v_lo)

    def den(x):
        return np.sqrt(x / bc2) + eps
    upd = lr * (m1 / bc1) / den(v1)
    am = np.abs(m1)
    # the update with m anywhere in [m - m_err, m + m_err] and v in [v_lo, v_hi], against the exact one
    carried = (lr / bc1) * np.maximum((am + m_err) / den(v_lo) - am / den(v1), am / den(v1) - np.maximum(am - m_err, 0.0) / den(v_hi))
    upd_mag = (lr / bc1) * (am + m_err) / den(v_lo)
    return dict(p=p - upd, m=m1, v=v1, p_mag=np.abs(p) + np.abs(upd), m_mag=m_mag, v_mag=v_mag, upd=upd,
                p_err=K_ADAM * U * upd_mag + U * np.abs(p) + carried, m_err=m_err, v_err=v_err)


def rows_gather_add(dst, slot, src, n_src):
    """dst[v,:] += src[slot[v],:] for the rows with 0 <= slot[v] < n_src; the other rows stay.  -> (out, magnitude, touched),
    ``touched`` the boolean row mask.  One addition per element: the float32 result is the float32 numpy sum, bit for bit."""
    dst, src, slot = _f64(dst), _f64(src), np.asarray(slot, dtype=np.int64)
    touched = (slot >= 0) & (slot < int(n_src))
    out, mag = dst.copy(), np.abs(dst)
    rows = np.nonzero(touched)[0]
    out[rows] = dst[rows] + src[slot[rows]]
    mag[rows] = np.abs(dst[rows]) + np.abs(src[slot[rows]])
    return out, mag, touched


def init_multi(n, src=None, src2=None):
    """dst[0..n) = (src or 0) + (src2 or 0) for one item of blm_init_multi.  -> (out, magnitude).  One addition per element."""
    a = np.zeros(n) if src is None else _f64(src).reshape(-1)
    b = np.zeros(n) if src2 is None else _f64(src2).reshape(-1)
    assert a.shape == (n,) and b.shape == (n,)
    return a + b, np.abs(a) + np.abs(b)


def axpy(x, y, a):
    """y + a*x.  -> (out, magnitude)."""
    x, y, a = _f64(x), _f64(y), f32(a)
    return y + a * x, np.abs(y) + np.abs(a * x)


def colsum(x, out0=None):
    """(out0 or 0) + sum over the rows of x (M, N).  -> (out, magnitude)."""
    x = _f64(x)
    base = np.zeros(x.shape[1]) if out0 is None else _f64(out0)
    return base + x.sum(0), np.abs(base) + np.abs(x).sum(0)
