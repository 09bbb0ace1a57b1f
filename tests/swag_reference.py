"""Float64 numpy restatement of the SWAG kernels (include/bayeslm.h, csrc/swag.hip): the inputs are the fp32 arrays the kernels
get, every operation on them runs in float64, nothing is rounded to fp32 on the way.  Each function that a kernel is held to
comes with its bound, derived from the rounded fp32 operations behind that output and evaluated per element from the float64
magnitudes of the terms, with a factor 2 over the derivation.  u = 2^-24, the relative error of one rounded fp32 operation."""
import math

import numpy as np

U = 2.0 ** -24


def f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------ collect
def collect(theta, mean, m2, count):
    """-> (mean', m2', deviation) of iterate number ``count``; at 0 mean and m2 are not looked at"""
    th = f64(theta)
    if count == 0:
        return th.copy(), np.zeros_like(th), np.zeros_like(th)
    mean, m2 = f64(mean), f64(m2)
    d = th - mean
    mn = mean + d / (count + 1.0)
    dev = th - mn
    return mn, m2 + d * dev, dev


def collect_bound(theta, mean, m2, count):
    """d = th - mean (u |d|); d * inv with inv rounded once (3 u |d inv| with d's own error); mean' = mean + d inv (u |mean'|):
         e_mean = u (|mean'| + 3 |d inv|)
       dev = th - mean':  e_dev = e_mean + u |dev|
       m2' = m2 + d * dev:  e_m2 = u |m2'| + 2 u |d dev| + |d| e_dev
    -> (2 e_mean, 2 e_m2, 2 e_dev); exact at count 0"""
    th = f64(theta)
    if count == 0:
        z = np.zeros_like(th)
        return z, z, z
    mn, q, dev = collect(theta, mean, m2, count)
    d = th - f64(mean)
    e_mean = U * (np.abs(mn) + 3 * np.abs(d / (count + 1.0)))
    e_dev = e_mean + U * np.abs(dev)
    e_m2 = U * np.abs(q) + 2 * U * np.abs(d * dev) + np.abs(d) * e_dev
    return 2 * e_mean, 2 * e_m2, 2 * e_dev


# ------------------------------------------------------------------ sample
def coefficients(scale, k_live, diag=False):
    if diag or k_live < 2:
        return math.sqrt(scale), 0.0, 0
    return math.sqrt(scale / 2.0), math.sqrt(scale / (2.0 * (k_live - 1))), k_live


def sample_terms(mean, m2, n, a, b, floor, z1, dev=None, z2=None):
    """-> (mean, a sqrt(max(m2 / n, floor)) z1, b sum_k dev[k] z2[k], b sum_k |dev[k] z2[k]|, rows) for ONE sample; z1 (P,) and
    z2 (k,) are the fp32 normals the kernel used, floor the fp32 value it was handed"""
    mean, m2, z1 = f64(mean), f64(m2), f64(z1)
    var = np.maximum(m2 / float(n), float(np.float32(floor)))
    t1 = a * np.sqrt(var) * z1
    k = 0 if z2 is None else len(z2)
    t2, t2abs = np.zeros_like(mean), np.zeros_like(mean)
    for i in range(k):
        term = f64(dev[i]) * float(np.float32(z2[i]))
        t2 += term
        t2abs += np.abs(term)
    return mean, t1, b * t2, abs(b) * t2abs, k


def sample(mean, m2, n, a, b, floor, z1, dev=None, z2=None):
    m, t1, t2, _, _ = sample_terms(mean, m2, n, a, b, floor, z1, dev, z2)
    return m + t1 + t2


def sample_bound(mean, m2, n, a, b, floor, z1, dev=None, z2=None):
    """var = m2 * inv_n (inv_n rounded, the product rounded: 2 u), sqrt (u + half of var's), a rounded and multiplied (2 u): the
    diagonal factor carries 4 u;  base = fma(sd, z1, mean): 4 u |T1| + u |base|;  low: K fmas, each u of a partial sum that
    never exceeds sum_k |D z|: K u T2abs, then b (rounded) in the last fma: (K + 1) u T2abs + u |out|.  With |base| <= |mean| +
    |T1| and |out| <= |mean| + |T1| + T2abs:  e = u (2 |mean| + 6 |T1| + (K + 2) T2abs);  -> 2 e"""
    m, t1, _, t2abs, k = sample_terms(mean, m2, n, a, b, floor, z1, dev, z2)
    return 2 * U * (2 * np.abs(m) + 6 * np.abs(t1) + (k + 2) * t2abs)


# ------------------------------------------------------------------ log-mean-exp over the samples
def _row_parts(z):
    """float64 row-wise: max, d = z - max, p = softmax, log L, lse"""
    z = f64(z)
    M = z.max(1, keepdims=True)
    with np.errstate(invalid="ignore"):
        d = z - M
    e = np.exp(d)
    L = e.sum(1, keepdims=True)
    return M, d, e / L, np.log(L), M + np.log(L)


def logp_entropy(z):
    """-> (logp (R, V), H (R,)) of the rows of logits z; a column at -inf has p log p = 0"""
    M, d, p, logl, lse = _row_parts(z)
    with np.errstate(invalid="ignore"):
        pd = np.where(p > 0, p * d, 0.0)
    return f64(z) - lse, (logl - pd.sum(1, keepdims=True))[:, 0]


def logp_errors(z):
    """The error of one sample's fp32 log-softmax and entropy -> (e_logp (R, V), e_H (R,), e_lse (R,)), before the factor 2.
    Column j with d_j = z_j - max enters the sum as exp(d_j): the product d_j log2(e) and the constant are rounded (2 u |d_j| on
    the result), the hardware exponential is within an ulp (2 u), and in the two-sweep form the lane's running sum is rescaled at
    most once per trip, each rescale a rounded product and another exponential whose exponents add up to at most |d_j|:
        delta_j = u (2 + 3 trips + 2 |d_j|),  trips = ceil(V / 4096) + 1
    The V terms are added in a tree of depth at most 4 ceil(V / 4096) + 14 (a lane's own, six butterfly steps, sixteen waves):
        eps_L = sum_j p_j delta_j + depth u                       relative error of L
    log L by the hardware logarithm times ln 2 (2 u (1 + |log L|)), lse = max + log L rounded (u |lse|):
        e_lse = eps_L + 2 u (1 + |log L|) + u |lse|;   e_logp = e_lse + u |logp|
    H = log L - (sum_j exp(d_j) d_j) / L: the numerator's terms carry delta_j + u each and the tree's depth, the quotient eps_L + u:
        e_H = eps_L + 2 u (1 + |log L|) + sum_j p_j |d_j| (delta_j + (2 + depth) u) + (sum_j p_j |d_j|) (eps_L + u) + u |H|"""
    M, d, p, logl, lse = _row_parts(z)
    V = d.shape[1]
    trips, depth = -(-V // 4096) + 1, 4 * -(-V // 4096) + 14
    with np.errstate(invalid="ignore"):
        ad = np.where(p > 0, np.abs(d), 0.0)
    delta = U * (2 + 3 * trips + 2 * ad)
    eps_L = (p * delta).sum(1, keepdims=True) + depth * U
    e_lse = eps_L + 2 * U * (1 + np.abs(logl)) + U * np.abs(lse)
    logp, H = logp_entropy(z)
    with np.errstate(invalid="ignore"):
        e_logp = e_lse + U * np.where(np.isfinite(logp), np.abs(logp), 0.0)
    pad = (p * ad).sum(1, keepdims=True)
    e_H = (eps_L + 2 * U * (1 + np.abs(logl)) + (p * ad * (delta + (2 + depth) * U)).sum(1, keepdims=True) + pad * (eps_L + U))[:, 0] \
        + U * np.abs(H)
    return e_logp, e_H, e_lse[:, 0]


def average(zs, targets=None):
    """zs: S arrays (R, V) of logits -> dict(acc = log mean_s p_s, hsum = sum_s H_s, nll_s (S, R): -logp_s at the target, 0 for a
    target outside [0, V)) with the bounds b_acc, b_hsum, b_nll_s.

    The fold acc' = max(acc, lp) + log1p(exp(-|acc - lp|)) is logaddexp, which moves by at most max(e_acc, e_lp) when its
    arguments move by e_acc and e_lp; its own rounded steps, with t = exp(-|acc - lp|) <= 1: the difference (u |diff|, times the
    slope t / (1 + t) <= t), the exponential (u (2 + 2 |diff|) t), log1p (2 u log 2) and the sum (u |acc'|).  The last sample
    subtracts log S, rounded once (u log S), by one more rounded operation (u |acc|).  hsum adds u |hsum| per sample after the
    first."""
    S = len(zs)
    R, V = np.asarray(zs[0]).shape
    acc = e_acc = hsum = e_hsum = None
    nll_s, b_nll = np.zeros((S, R)), np.zeros((S, R))
    for s, z in enumerate(zs):
        lp, H = logp_entropy(z)
        e_lp, e_H, e_lse = logp_errors(z)
        if targets is not None:
            for r, t in enumerate(np.asarray(targets).reshape(-1)):
                if 0 <= t < V:
                    nll_s[s, r] = -lp[r, t]
                    b_nll[s, r] = 2 * (e_lse[r] + U * abs(lp[r, t]))
        if s == 0:
            acc, e_acc, hsum, e_hsum = lp, e_lp, H, e_H
        else:
            with np.errstate(invalid="ignore"):
                diff = np.where(np.isfinite(acc) | np.isfinite(lp), np.abs(acc - lp), 0.0)
            diff = np.where(np.isfinite(diff), diff, 0.0)  # one side at -inf: t = 0, the other side passes through
            t = np.where(np.isfinite(acc) & np.isfinite(lp), np.exp(-diff), 0.0)
            new = np.logaddexp(acc, lp)
            fin = np.where(np.isfinite(new), np.abs(new), 0.0)
            e_acc = np.maximum(e_acc, e_lp) + U * (diff * t + (2 + 2 * diff) * t + 2 * math.log(2.0) + fin)
            acc = new
            hsum = hsum + H
            e_hsum = e_hsum + e_H + U * np.abs(hsum)
    acc = acc - math.log(S)
    e_acc = e_acc + U * math.log(S) + U * np.where(np.isfinite(acc), np.abs(acc), 0.0)
    return {"acc": acc, "hsum": hsum, "nll_s": nll_s, "b_acc": 2 * e_acc, "b_hsum": 2 * e_hsum, "b_nll_s": b_nll}


def entropy_of_logp(logp):
    """H of rows that are already log-probabilities (float64)"""
    lp = np.asarray(logp, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return -np.where(np.isfinite(lp), np.exp(lp) * lp, 0.0).sum(1)
