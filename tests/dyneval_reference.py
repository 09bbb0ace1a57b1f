"""Float64 numpy restatement of the dynamic-evaluation kernels (include/bayeslm.h, csrc/dyneval.hip): the inputs are the fp32
arrays the kernels get, every operation on them runs in float64, nothing is rounded to fp32 on the way."""
import numpy as np


def f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def accum(ms, g):
    """ms + g^2"""
    return f64(ms) + f64(g) ** 2


def rms(ms, count):
    """-> (rms, rbar, live): rms = sqrt(ms / count); rbar its mean over the LIVE entries ms > 0, live their number"""
    ms = f64(ms)
    r = np.sqrt(ms / float(count))
    live = ms > 0
    n = int(live.sum())
    return r, (float(r[live].sum() / n) if n else 0.0), n


def update_terms(p, g, p0, lr, decay, r=None, rbar=None, eps=0.01):
    """-> (step, d (p0 - p)): the two terms of  p - step + d (p0 - p).  ``r`` None: the sgd rule, step = lr g, d = min(1, decay);
    else the rms rule, step = lr g / (r + eps rbar) (0 where g = 0), d = min(1, decay r / rbar).  lr, decay, eps and rbar are
    taken as the fp32 values the kernel is handed."""
    p, g, p0 = f64(p), f64(g), f64(p0)
    lr, decay, eps = (float(np.float32(v)) for v in (lr, decay, eps))
    if r is None:
        step, d = lr * g, np.full_like(p, min(1.0, decay))
    else:
        r, rbar = f64(r), float(np.float32(rbar))
        den = r + eps * rbar
        with np.errstate(divide="ignore", invalid="ignore"):
            step = np.where(g == 0.0, 0.0, lr * g / den)
        d = np.minimum(1.0, decay * r / rbar)
    return step, d * (p0 - p)


def update(p, g, p0, lr, decay, r=None, rbar=None, eps=0.01):
    step, pull = update_terms(p, g, p0, lr, decay, r, rbar, eps)
    return f64(p) - step + pull


def update_bound(p, g, p0, lr, decay, r=None, rbar=None, eps=0.01):
    """The kernel is at most about eight rounded fp32 operations on the terms: |out - ref| <= 16 * 2^-24 * (|p| + |step| +
    |d (p0 - p)|) per element"""
    step, pull = update_terms(p, g, p0, lr, decay, r, rbar, eps)
    return 16.0 * 2.0 ** -24 * (np.abs(f64(p)) + np.abs(step) + np.abs(pull))
