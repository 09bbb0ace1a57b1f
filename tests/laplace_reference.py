"""Float64 numpy restatement of the last-layer Laplace formulas (include/bayeslm.h, csrc/laplace.hip, bayeslms_amd/laplace.py):
the inputs are the fp32 arrays the kernels get (the noise eps read back through ops.philox_normal), every operation on them
runs in float64.  Each output a kernel is held to comes with its bound, derived from the rounded fp32 operations behind it and
evaluated per element from the float64 magnitudes, with a factor 2 over the derivation (as tests/swag_reference.py does).

u = 2^-24, the relative error of one rounded fp32 operation.  The building blocks, each used below where it is named:
  exp   __expf(d) is v_exp_f32(d log2 e): the product is rounded (and log2 e itself), 2 u |d| on the exponent, and the instruction
        is good to 1 ulp = 2 u:  relative (2 |d| + 2) u.  A result below 2^-126 may be flushed: TINY absolute.
  log   logf is good to 1 ulp: 2 u |log x|.
  sum   n rounded additions of non-negative terms in any order: n u times the sum; n is the longest chain of additions a value
        passes through, adds(V): 4 ceil(V / 1024) in a lane of a 256-lane workgroup, 6 butterfly steps, up to 16 waves.
  online softmax: a term exp(x - m_k) summed under the running maximum m_k is later scaled by exp(m_k - M) in r <= rescales(V)
        steps (one per quad a lane reads, 6 + 4 merges), each a rounded exp and a rounded product: together with its own exp and
        the rounded difference that is relative (3 |x - M| + 2 + 3 r) u per term, since |x - m_k| + (M - m_k) = M - x."""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -120
PI8 = float(np.float32(0.39269908169872414))


def f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def adds(V):
    return 4 * math.ceil(V / 1024.0) + 6 + 16


def rescales(V):
    return math.ceil(V / 1024.0) + 10


# ------------------------------------------------------------------ softmax pieces of rows x (..., V) with input error ex
def softmax_parts(x, ex=0.0):
    """-> dict of float64 pieces of the rows ``x`` (..., V) whose entries carry the absolute error ``ex`` (scalar or array):
    M, d = x - M, t = exp(d), l = sum t, lse, and the bounds (without the factor 2) rel_l of l (relative) and e_lse of lse.
    The inputs' own error moves lse by at most max ex (a weighted mean of ex)."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[-1]
    ex = np.broadcast_to(np.asarray(ex, dtype=np.float64), x.shape)
    M = x.max(-1, keepdims=True)
    d = np.where(np.isneginf(x), -np.inf, x - M)
    t = np.exp(d)
    l = t.sum(-1, keepdims=True)
    ad = np.where(np.isfinite(d), np.abs(d), 0.0)
    e_l = (t * U * (3 * ad + 2 + 3 * rescales(V))).sum(-1, keepdims=True) + U * adds(V) * l + V * TINY
    rel_l = e_l / l
    lse = M + np.log(l)
    exm = ex.max(-1, keepdims=True)
    e_lse = rel_l + 2 * U * np.abs(np.log(l)) + U * np.abs(lse) + exm
    return dict(M=M, d=d, ad=ad, t=t, l=l, lse=lse, rel_l=rel_l, e_lse=e_lse, ex=ex, exm=exm, V=V)


# ------------------------------------------------------------------ curvature
def curvature(logits, ex=0.0):
    """a = p (1 - p), p = softmax(logits) row by row -> (a, bound).  d = x - lse is rounded (u |d|) and carries lse's and x's
    errors; p = exp(d): relative rp = (3 |d| + 2) u + ex + e_lse; a = fma(-p, p, p) is one rounding of the exact p - p^2:
    e_a = |1 - 2 p| p rp + (p rp)^2 + u a."""
    x = f64(logits) if np.asarray(logits).dtype != np.float64 else np.asarray(logits)
    s = softmax_parts(x, ex)
    dl = np.where(np.isneginf(x), -np.inf, x - s["lse"])
    p = np.exp(dl)
    adl = np.where(np.isfinite(dl), np.abs(dl), 0.0)
    rp = (3 * adl + 2) * U + s["ex"] + s["e_lse"]
    a = p * (1.0 - p)
    e = np.abs(1.0 - 2.0 * p) * p * rp + (p * rp) ** 2 + U * a + TINY
    return a, 2 * e


def fisher(a, e_a, h):
    """F_W = sum_t a_t h_t^2, F_b = sum_t a_t from curvature rows ``a`` (N, V) with bound ``e_a`` and decoder inputs ``h`` (N, K)
    -> (F_W, F_b, bound_W, bound_b).  h^2 is rounded once (u); the products of the matrix instruction are exact and their
    N-term sums rounded at most N + 4 times whatever the order or the number of K slices: (N + 5) u of sum_t a h^2."""
    h2 = f64(h) ** 2
    N = h2.shape[0]
    fw, fb = a.T @ h2, a.sum(0)
    bw = e_a.T @ h2 + (N + 5) * U * fw * 2
    bb = e_a.sum(0) + (N + 5) * U * fb * 2
    return fw, fb, bw, bb


def variance(h, f_w, f_b, tau):
    """var[r, v] = sum_k h[r, k]^2 / (F_W[v, k] + tau) + 1 / (F_b[v] + tau) in float64; tau = inf: 0"""
    h2 = f64(h) ** 2
    if math.isinf(tau):
        return np.zeros((h2.shape[0], np.asarray(f_w).shape[0]))
    return h2 @ (1.0 / (f64(f_w) + tau)).T + 1.0 / (f64(f_b) + tau)[None, :]


# ------------------------------------------------------------------ closed-form links
def link_y(z, var, link):
    """y and its bound e_y (without the factor 2).  probit: t = fma(pi/8, var, 1) (the constant rounded: u on its term, the fma
    u), v_rsq_f32 1 ulp = 2 u and half of t's, the product u: 4 u |y|.  expexp: one fma: u |y|."""
    z, var = f64(z), f64(var)
    if link == "probit":
        y = z / np.sqrt(1.0 + PI8 * var)
        return y, 4 * U * np.abs(y)
    if link == "expexp":
        y = z + 0.5 * var
        return y, U * np.abs(y)
    raise ValueError(link)


def softmax64(y):
    m = y.max(-1, keepdims=True)
    e = np.exp(y - m)
    return e / e.sum(-1, keepdims=True)


def row_stats(y, ey, tgt, var=None):
    """blm_row_stats' figures of rows ``y`` (R, V) whose entries carry the error ``ey``, and vbar = sum p var -> dict of (value,
    bound) pairs.  With s = softmax_parts(y), p = t / l, T = sum t d, H = log l - T / l:
      nll   (M - y_t) rounded, log l (2 u |log l| + rel_l), their sum rounded; the inputs move it by ey_t + max ey
      conf  1 / l: rel_l + u; the inputs by conf (ey_M + max ey)
      T     a term t d: its exp and scalings (3 |d| + 2 + 3 r) u, the product and d's rounding 2 u; every rescale also rounds
            t + d s and the product with f, 3 u each of a partial sum below sum t |d|: r times, twice:
            e_T = u sum t |d| (3 |d| + 4 + 9 r + adds)
      H     2 u |log l| + rel_l + e_T / l + |T / l| (rel_l + u) + u |H|; the inputs by max ey sum p |log p + H|
      vbar  w = sum t var: e_w = u sum t var (3 |d| + 3 + 3 r + adds); e_w / l + vbar (rel_l + u); inputs: max ey sum p |var - vbar|"""
    s = softmax_parts(y, ey)
    R, V = y.shape
    p = s["t"] / s["l"]
    rel_l, exm, l = s["rel_l"][:, 0], s["exm"][:, 0], s["l"][:, 0]
    logl = np.log(l)
    tgt = np.asarray(tgt)
    ok = (tgt >= 0) & (tgt < V)
    tc = np.where(ok, tgt, 0)
    rows = np.arange(R)
    yt = y[rows, tc]
    nll = s["lse"][:, 0] - yt
    e_nll = U * np.abs(s["M"][:, 0] - yt) + 2 * U * np.abs(logl) + rel_l + U * np.abs(nll) + s["ex"][rows, tc] + exm
    conf = 1.0 / l
    e_conf = conf * (rel_l + 2 * U + 2 * exm)
    r, ad = rescales(V), s["ad"]
    T = (s["t"] * np.where(np.isfinite(s["d"]), s["d"], 0.0)).sum(-1)
    e_T = U * (s["t"] * ad * (3 * ad + 4 + 9 * r + adds(V))).sum(-1)
    H = logl - T / l
    logp = np.where(p > 0, np.log(np.where(p > 0, p, 1.0)), 0.0)
    e_H = (2 * U * np.abs(logl) + rel_l + e_T / l + np.abs(T / l) * (rel_l + U) + U * np.abs(H)
           + exm * (p * np.abs(logp + H[:, None])).sum(-1))
    out = {"nll": (np.where(ok, nll, np.nan), 2 * e_nll), "conf": (conf, 2 * e_conf), "entropy": (H, 2 * e_H)}
    if var is not None:
        v = f64(var)
        vbar = (p * v).sum(-1)
        e_w = U * (s["t"] * v * (3 * ad + 3 + 3 * r + adds(V))).sum(-1)
        e_v = e_w / l + vbar * (rel_l + U) + exm * (p * np.abs(v - vbar[:, None])).sum(-1)
        out["vbar"] = (vbar, 2 * e_v + TINY)
    return out


def decided(y, ey, tgt):
    """pred, rank in float64 and the rows on which each is decided: the margin between the values that decide it exceeds
    4 x the value bound, 2 ey, of either of the two values -> (pred, rank, pred_ok, rank_ok)"""
    R, V = y.shape
    ey = np.broadcast_to(np.asarray(ey, dtype=np.float64), y.shape)
    rows, cols = np.arange(R), np.arange(V)[None, :]

    def clear_of(ref):
        slack = np.abs(y - y[rows, ref][:, None]) - 8 * np.maximum(ey, ey[rows, ref][:, None])
        slack[rows, ref] = np.inf
        return slack.min(-1) > 0

    pred = y.argmax(-1)
    pred_ok = clear_of(pred)
    tgt = np.asarray(tgt)
    ok = (tgt >= 0) & (tgt < V)
    tc = np.where(ok, tgt, 0)
    yt = y[rows, tc][:, None]
    rank = ((y > yt) | ((y == yt) & (cols < tc[:, None]))).sum(-1)
    return pred, np.where(ok, rank, -1), pred_ok, clear_of(tc) & ok


def closed_form(z, var, tgt, link):
    """The reference of blm_laplace_row_stats -> (dict of (value, bound), y, e_y)"""
    y, ey = link_y(z, var, link)
    return row_stats(y, ey, tgt, var), y, ey


# ------------------------------------------------------------------ Monte-Carlo link
def noise_rows(philox_normal, seed, stream, S, row0, R, V):
    """eps (S, R, V): element ((row0 + r) Vq + v) of the stream (seed, stream, step = s), read back through ``philox_normal``
    (n, seed, stream, step) -> fp32 array of the first n elements"""
    Vq = (V + 3) // 4 * 4
    out = np.empty((S, R, V), np.float64)
    for s in range(S):
        flat = f64(philox_normal((row0 + R) * Vq, seed, stream, s))
        out[s] = flat[row0 * Vq:].reshape(R, Vq)[:, :V]
    return out


def mc_rows(z, var, tgt, eps):
    """The reference of blm_laplace_mc_rows from the fp32 z, var (R, V) and the noise eps (S, R, V) -> dict of (value, bound).
      x_s   sd = sqrt(var) (1 ulp: 2 u), x = fma(sd, eps, z): ex = 2 u |sd eps| + u |x|
      lse_s softmax_parts(x_s, ex): e_lse;  nll_s = lse_s - x_s[t]: e_lse + ex_t + u |nll_s|
      p_s   d = x - lse rounded, exp: relative rp = (3 |d| + 2) u + ex + e_lse
      pbar  S rounded additions and the product with the rounded 1 / S: e_pb = (sum_s p_s rp_s) / S + (S + 2) u pbar
      bma   -log pbar_t: e_pb_t / pbar_t + 2 u |log pbar_t|
      conf  max pbar: max e_pb
      h     a term -pb log pb: (|log pb| + 1) e_pb + 3 u |pb log pb|; the sum adds(V) u sum |pb log pb|
      mi    a term p_s (d - lp), lp = log pb: p_s rp |d - lp| + p_s (e_d + e_lp) + 2 u |term| with e_d = u |d| + ex + e_lse and
            e_lp = e_pb / pb + 2 u |lp|; a lane adds 4 S ceil(V / 1024) of them in turn: (that + 26) u sum |term|; then 1 / S."""
    z, var = f64(z), f64(var)
    S, R, V = eps.shape
    sd = np.sqrt(var)
    x = z[None] + sd[None] * eps
    ex = 2 * U * np.abs(sd[None] * eps) + U * np.abs(x)
    sp = softmax_parts(x, ex)
    lse, e_lse = sp["lse"], sp["e_lse"]  # (S, R, 1)
    d = x - lse
    p = np.exp(d)
    e_d = U * np.abs(d) + ex + e_lse
    rp = (2 * np.abs(d) + 2) * U + e_d
    pb = p.sum(0) / S
    e_pb = (p * rp).sum(0) / S + (S + 2) * U * pb + TINY
    tgt = np.asarray(tgt)
    ok = (tgt >= 0) & (tgt < V)
    tc = np.where(ok, tgt, 0)
    rows = np.arange(R)
    xt = x[:, rows, tc]
    nll_s = lse[:, :, 0] - xt
    e_nll_s = e_lse[:, :, 0] + ex[:, rows, tc] + U * np.abs(nll_s)
    pt = pb[rows, tc]
    bma = -np.log(pt)
    e_bma = e_pb[rows, tc] / pt + 2 * U * np.abs(bma)
    conf, e_conf = pb.max(-1), e_pb.max(-1)
    lp = np.log(pb)
    plp = np.abs(pb * lp)
    h = -(pb * lp).sum(-1)
    e_h = ((np.abs(lp) + 1) * e_pb + 3 * U * plp).sum(-1) + adds(V) * U * plp.sum(-1)
    e_lp = e_pb / pb + 2 * U * np.abs(lp)
    term = p * (d - lp[None])
    e_term = p * rp * np.abs(d - lp[None]) + p * (e_d + e_lp[None]) + 2 * U * np.abs(term)
    chain = 4 * S * math.ceil(V / 1024.0) + 26
    mi = term.sum((0, 2)) / S
    e_mi = (e_term.sum((0, 2)) + chain * U * np.abs(term).sum((0, 2))) / S + 2 * U * np.abs(mi) + TINY
    nan = np.where(ok, 0.0, np.nan)
    return {"bma_nll": (bma + nan, 2 * e_bma), "nll_s": ((nll_s + nan[None]).T, 2 * e_nll_s.T), "h_pred": (h, 2 * e_h),
            "mi": (mi, 2 * e_mi), "conf": (conf, 2 * e_conf), "pbar": (pb, 2 * e_pb)}


def mc_decided(pb, e_pb, tgt):
    """pred and rank under pbar and the rows on which each is decided (margin > 4 x the value bound)"""
    return decided(pb, e_pb / 2, tgt)
