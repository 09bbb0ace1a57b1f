"""Float64 torch reference of the continuous neural cache (include/bayeslm.h, blm_cache_scores; engine.evaluate_cache): a dense
masked score matrix, as the definitions are written.  CPU or GPU, wherever the inputs live."""
import math

import torch


def key_ranges(hi, window, Nk, lo=None):
    """[start, end) per query, clamped as the kernel clamps: start = max(lo, hi - window, 0), end = min(hi, Nk)."""
    hi = hi.to(torch.int64)
    lo = torch.zeros_like(hi) if lo is None else lo.to(torch.int64)
    start = torch.maximum(torch.maximum(lo, hi - int(window)), torch.zeros_like(hi))
    end = torch.minimum(hi, torch.full_like(hi, int(Nk)))
    return start, end


def cache_scores(q, k, labels, targets, hi, thetas, window, lo=None):
    """-> (lse, match), both (J, M) float64; -inf over an empty set."""
    q64, k64 = q.double(), k.double()
    s = q64 @ k64.t()  # (M, Nk)
    start, end = key_ranges(hi, window, k.shape[0], lo)
    idx = torch.arange(k.shape[0], device=q.device)[None, :]
    in_range = (idx >= start[:, None]) & (idx < end[:, None])
    same = in_range & (labels.reshape(1, -1) == targets.reshape(-1, 1))
    ninf = torch.full_like(s, -math.inf)
    lse, match = [], []
    for t in thetas:
        z = float(t) * s
        lse.append(torch.logsumexp(torch.where(in_range, z, ninf), 1))
        match.append(torch.logsumexp(torch.where(same, z, ninf), 1))
    return torch.stack(lse), torch.stack(match)


def text_scores(h, y, thetas, window):
    """The evaluation's case: q = k = the text's rows, the cache of row t holds rows max(0, t - window) .. t - 1."""
    n = h.shape[0]
    return cache_scores(h, h, y, y, torch.arange(n, device=h.device), thetas, window)


def cache_mix(nll_model, lse, match, lam):
    """NLL of (1 - lam) p_model + lam exp(match - lse) in float64; p_model where the cache is empty (lse = -inf)."""
    nll = nll_model.double()
    lse, match = lse.double(), match.double()
    p_cache = torch.where(torch.isneginf(match), torch.zeros_like(match), torch.exp(match - lse))
    p = (1.0 - lam) * torch.exp(-nll) + lam * p_cache
    return torch.where(torch.isneginf(lse), nll, -torch.log(p))


def cache_distribution(h, y, V, t, theta, window):
    """p_cache(w) of row t for every word w in [0, V) -> (V,) float64 (zeros if the cache is empty)."""
    out = torch.zeros(V, dtype=torch.float64)
    a = max(0, t - window)
    if a >= t:
        return out
    w = torch.softmax(theta * (h[a:t].double() @ h[t].double()), 0)
    out.index_add_(0, y[a:t], w)
    return out
