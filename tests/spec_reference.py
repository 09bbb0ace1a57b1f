"""A numpy float64 model of blm_spec_accept, written from the definitions of include/bayeslm.h (not from the kernel), with the
Philox words of oracle/philox.py.  Beside the decisions it returns the margins by which each was taken, so that a float32
evaluation can be held to exact agreement wherever float32 can decide the question at all.

The noise is DEFINED as blm_sample_rows' (the bonus row must equal blm_sample_rows bit for bit), and that uniform is a float32
number: float(w >> 8) + 0.5f is rounded to 24 bits, to the nearest even integer from w >> 8 = 2^23 on.  The model takes u as that
float32 value and does everything behind it in float64.  Taken in exact arithmetic instead, a u near 1 -- the largest Gumbel
values, which are the ones that win -- moves by half a unit in the last place, g = -log(-log u) with it by 0.5 / ((1 - u) 2^24),
several 1e-3 at u = 1 - 6e-6, and the model would describe another noise than the one the definitions name."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.philox import philox4x32_10  # noqa: E402


def uniforms(cols, rows, seed, stream, step):
    """The blm_sample_rows uniform ((w >> 8) + 0.5) * 2^-24 of the first Philox word at counter (col, row, stream, step), key
    seed -- the float32 number blm_sample_rows holds, as float64; cols and rows broadcast against each other."""
    cols, rows = np.broadcast_arrays(np.asarray(cols, np.uint64), np.asarray(rows, np.uint64))
    shape = cols.shape
    c0 = (cols.reshape(-1) & 0xFFFFFFFF).astype(np.uint32)
    c1 = (rows.reshape(-1) & 0xFFFFFFFF).astype(np.uint32)
    n = c0.shape[0]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(c0, c1, np.full(n, int(stream) & 0xFFFFFFFF, np.uint32), np.full(n, int(step) & 0xFFFFFFFF, np.uint32),
                      np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))[0]
    u = ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)  # float32, as blm_sample_rows forms it
    return u.astype(np.float64).reshape(shape)


def gumbel(cols, rows, seed, stream, step):
    """g = -log(-log u), float64"""
    with np.errstate(divide="ignore"):  # the float32 u reaches 1 at w >> 8 = 2^24 - 1: g = +inf there, as in the kernels
        return -np.log(-np.log(uniforms(cols, rows, seed, stream, step)))


def _argmax_lowest(key):
    """lowest index holding the maximum of a 1-D array (no NaN in it)"""
    return int(np.argmax(key))  # numpy returns the first occurrence


def _log_softmax(z):
    """log softmax of a 1-D float64 array from max-shifted values; a -inf entry has mass 0"""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = z - np.max(z)
        return d - np.log(np.sum(np.exp(d)))


def _margin2(key):
    """distance between the best and the second best entry of key (inf when there is only one finite entry)"""
    if key.shape[0] < 2:
        return np.inf
    top = np.partition(key, -2)[-2:]
    return float(top[1] - top[0]) if np.isfinite(top[0]) else np.inf


def spec_accept(P, Q, x, temperature, seed, stream, step):
    """P (G + 1, N, V), Q (G, N, V) or None at temperature 0, x (G, N) -> dict of
      accept (G, N) uint8, cand (G + 1, N) int64, n_acc (N,) int32, token (N,) int64      the definitions, in float64
      accept_margin (G, N)    |log u - min(0, log p(x) - log q(x))| (inf where the rule does not depend on a rounding)
      cand_margin (G + 1, N)  winning key minus the runner-up
      cand_cancel (G + 1, N)  |log p - log q| at the winning column of a residual draw (inf elsewhere): small where
                              p - q cancels and float32 cannot tell whether the column has rho > 0 at all"""
    P = np.asarray(P, np.float64)
    G, N, V = P.shape[0] - 1, P.shape[1], P.shape[2]
    x = np.asarray(x, np.int64)
    accept = np.zeros((G, N), np.uint8)
    cand = np.zeros((G + 1, N), np.int64)
    am = np.full((G, N), np.inf)
    cm = np.full((G + 1, N), np.inf)
    cc = np.full((G + 1, N), np.inf)
    tau = float(np.float32(temperature))
    cols = np.arange(V)
    if tau == 0.0:
        for t in range(G + 1):
            for n in range(N):
                row = P[t, n]
                if np.isnan(row).any():
                    cand[t, n] = -1
                    continue
                cand[t, n] = _argmax_lowest(row)
                if t < G:
                    accept[t, n] = 1 if x[t, n] == cand[t, n] else 0
    else:
        Q = np.asarray(Q, np.float64)
        beta = float(np.float32(1.0) / np.float32(tau))  # beta = float32(1 / tau)
        for t in range(G + 1):
            for n in range(N):
                r = t * N + n
                p_row = P[t, n]
                bad = np.isnan(p_row).any() or (t < G and np.isnan(Q[t, n]).any())
                if bad:
                    cand[t, n] = -1
                    continue
                g = gumbel(cols, r, seed, stream, step)
                with np.errstate(invalid="ignore", divide="ignore"):
                    plain = beta * p_row + g
                if t == G:
                    cand[t, n] = _argmax_lowest(plain)
                    cm[t, n] = _margin2(plain)
                    continue
                lp, lq = _log_softmax(beta * p_row), _log_softmax(beta * Q[t, n])
                xi = int(x[t, n])
                if 0 <= xi < V and lq[xi] > -np.inf:
                    lu = np.log(uniforms(0xFFFFFFFF, r, seed, stream, step))
                    bound = min(0.0, lp[xi] - lq[xi])
                    accept[t, n] = 1 if lu < bound else 0
                    am[t, n] = abs(lu - bound)
                p, q = np.exp(lp), np.exp(lq)
                rho = np.maximum(p - q, 0.0)
                live = rho > 0.0
                if live.any():
                    with np.errstate(divide="ignore"):
                        key = np.where(live, np.log(np.where(live, rho, 1.0)) + g, -np.inf)
                    cand[t, n] = _argmax_lowest(key)
                    cm[t, n] = _margin2(key)
                    with np.errstate(invalid="ignore"):
                        cc[t, n] = abs(lp[cand[t, n]] - lq[cand[t, n]])
                else:
                    cand[t, n] = _argmax_lowest(plain)
                    cm[t, n] = _margin2(plain)
    n_acc, token = finish(accept, cand)
    return dict(accept=accept, cand=cand, n_acc=n_acc, token=token, accept_margin=am, cand_margin=cm, cand_cancel=cc)


def finish(accept, cand):
    """n_acc[n] = the smallest t with accept[t, n] = 0, or G; token[n] = cand[n_acc[n], n]"""
    accept, cand = np.asarray(accept), np.asarray(cand)
    G, N = accept.shape
    n_acc = np.full(N, G, np.int32)
    for n in range(N):
        rej = np.nonzero(accept[:, n] == 0)[0]
        if rej.shape[0]:
            n_acc[n] = rej[0]
    return n_acc, cand[n_acc, np.arange(N)].astype(np.int64)


def sample_rows(X, temperature, seed, stream, step):
    """blm_sample_rows in float64 on the (R, V) matrix X: argmax_v X_v / temperature + g_v at counter (v, row, stream, step)"""
    X = np.asarray(X, np.float64)
    R, V = X.shape
    beta = float(np.float32(1.0) / np.float32(temperature))
    out = np.zeros(R, np.int64)
    for r in range(R):
        out[r] = _argmax_lowest(beta * X[r] + gumbel(np.arange(V), r, seed, stream, step))
    return out
