"""Plain Python / numpy restatement of the n-best WER kernels (include/bayeslm.h, csrc/nbest.hip): tuple-valued dynamic
programming with `min` over (cost, ins) for the alignment, float64 totals and risks evaluated as the header writes them."""
import itertools

import numpy as np

EDIT_MAX_LEN = 1023


def align(a, b):
    """-> (cost, sub, ins, del) of hypothesis a against reference b: the minimum cost, and among the minimum-cost alignments the
    one with the fewest insertions (a word of a left unmatched)."""
    la, lb = len(a), len(b)
    prev = [(j, 0) for j in range(lb + 1)]  # no word of a yet: j deletions
    for i in range(1, la + 1):
        cur = [(i, i)]  # i insertions
        x = a[i - 1]
        for j in range(1, lb + 1):
            dc, di = prev[j - 1]
            uc, ui = prev[j]
            lc, li = cur[j - 1]
            cur.append(min((dc + (x != b[j - 1]), di), (uc + 1, ui + 1), (lc + 1, li)))
        prev = cur
    cost, ins = prev[lb]
    dele = ins - (la - lb)
    return cost, cost - ins - dele, ins, dele


def brute_force(a, b):
    """The same four numbers by enumerating EVERY alignment (monotone sets of matched position pairs): small inputs only."""
    la, lb = len(a), len(b)
    best = None
    for k in range(min(la, lb) + 1):
        for ia in itertools.combinations(range(la), k):
            for ib in itertools.combinations(range(lb), k):
                sub = sum(a[i] != b[j] for i, j in zip(ia, ib))
                ins, dele = la - k, lb - k
                cand = (sub + ins + dele, ins, sub, dele)
                if best is None or cand < best:
                    best = cand
    return best[0], best[2], best[1], best[3]


def edit_distance(tok, off, a, b):
    """-> cost (P,), sid (P, 3) int32 over flat sequences; a bad pair (index out of range, a reversed offset range or one that
    leaves tok, a length over the limit) gets -1 everywhere."""
    tok, off = np.asarray(tok), np.asarray(off, dtype=np.int64)
    n_seq = len(off) - 1
    cost = np.full(len(a), -1, np.int32)
    sid = np.full((len(a), 3), -1, np.int32)

    def seq(q):
        if not 0 <= q < n_seq:
            return None
        lo, hi = int(off[q]), int(off[q + 1])
        if lo < 0 or hi < lo or hi > len(tok) or hi - lo > EDIT_MAX_LEN:
            return None
        return tok[lo:hi].tolist()
    for p, (ia, ib) in enumerate(zip(np.asarray(a).tolist(), np.asarray(b).tolist())):
        sa, sb = seq(ia), seq(ib)
        if sa is None or sb is None:
            continue
        r = align(sa, sb)
        cost[p], sid[p] = r[0], r[1:]
    return cost, sid


def pairwise(tok, off, uoff):
    """-> (dist, doff): the dense symmetric N x N int32 block of every group, flat, and the U block offsets"""
    uoff = np.asarray(uoff, dtype=np.int64)
    blocks, doff, at = [], [], 0
    tok = np.asarray(tok)
    for u in range(len(uoff) - 1):
        lo, hi = int(uoff[u]), int(uoff[u + 1])
        n = hi - lo
        d = np.zeros((n, n), np.int32)
        seqs = [tok[int(off[q]):int(off[q + 1])].tolist() for q in range(lo, hi)]
        for i in range(n):
            for j in range(i + 1, n):
                d[i, j] = d[j, i] = align(seqs[i], seqs[j])[0]
        doff.append(at)
        at += n * n
        blocks.append(d.reshape(-1))
    return (np.concatenate(blocks) if blocks else np.zeros(0, np.int32)), np.asarray(doff, np.int64)


def _arr(x, H):
    return np.zeros(H, np.float64) if x is None else np.asarray(x, dtype=np.float64)


def totals(ac, g, lm, nn, ln, point, H=None):
    """T = ac + L * (((g + w * nn) + (1 - w) * lm) + p * len) in float64, operation by operation"""
    H = H if H is not None else max(len(x) for x in (ac, g, lm, nn, ln) if x is not None)
    ac, g, lm, nn, ln = (_arr(x, H) for x in (ac, g, lm, nn, ln))
    L, w, p = (np.float64(v) for v in point[:3])
    with np.errstate(all="ignore"):
        return ac + L * (((g + w * nn) + (np.float64(1.0) - w) * lm) + p * ln)


def _argmin_finite(t):
    best, bi = np.inf, -1
    for i, v in enumerate(t):
        if np.isfinite(v) and v < best:
            best, bi = v, i
    return bi


def select(ac, g, lm, nn, ln, uoff, grid, H=None):
    """-> pick (G, U) int32: per grid point and group the argmin of T, lowest index on ties; a non-finite T never wins, a group
    without a finite T picks 0, an empty group -1"""
    uoff = np.asarray(uoff, dtype=np.int64)
    U = len(uoff) - 1
    H = int(uoff[-1]) if H is None else H
    pick = np.full((len(grid), U), -1, np.int32)
    for k, point in enumerate(grid):
        t = totals(ac, g, lm, nn, ln, point, H)
        for u in range(U):
            lo, hi = int(uoff[u]), int(uoff[u + 1])
            if hi > lo:
                pick[k, u] = max(_argmin_finite(t[lo:hi]), 0)
    return pick


def posterior(t, L, s):
    """P_i = exp(-(s (T_i - min T) / L)) / sum; a non-finite T has P = 0, without a finite T the posterior is uniform"""
    t = np.asarray(t, np.float64)
    fin = np.isfinite(t)
    if not fin.any():
        return np.full(len(t), 1.0 / len(t))
    tmin = t[fin].min()
    with np.errstate(all="ignore"):
        e = np.where(fin, np.exp(-((np.float64(s) * (t - tmin)) / np.float64(L))), 0.0)
    return e / e.sum()


def mbr(ac, g, lm, nn, ln, uoff, dist, doff, grid, H=None):
    """-> (risk (G, H) float64, pick (G, U) int32): R_i = sum_j P_j d(i, j) with j ascending; the pick is the argmin of R, lowest
    index on ties, -1 for an empty group"""
    uoff = np.asarray(uoff, dtype=np.int64)
    U = len(uoff) - 1
    H = int(uoff[-1]) if H is None else H
    risk = np.zeros((len(grid), H), np.float64)
    pick = np.full((len(grid), U), -1, np.int32)
    for k, point in enumerate(grid):
        t = totals(ac, g, lm, nn, ln, point, H)
        for u in range(U):
            lo, hi = int(uoff[u]), int(uoff[u + 1])
            n = hi - lo
            if n <= 0:
                continue
            P = posterior(t[lo:hi], point[0], point[3])
            d = np.asarray(dist[int(doff[u]):int(doff[u]) + n * n], np.float64).reshape(n, n)
            r = np.zeros(n, np.float64)
            for j in range(n):  # j ascending, one product and one sum per term
                r = r + P[j] * d[:, j]
            risk[k, lo:hi] = r
            pick[k, u] = int(np.argmin(r))  # the first of equal minima
    return risk, pick


def rates(err, sub, ins, dele, ref_words, utt_wrong, utts):
    return {"err": int(err), "sub": int(sub), "ins": int(ins), "del": int(dele),
            "wer": 100.0 * err / ref_words if ref_words else 0.0, "ser": 100.0 * utt_wrong / utts if utts else 0.0}


class Backend:
    """The four ops of bayeslms_amd.ops that nbest_wer.evaluate calls, answered by this module on host tensors: what the tests
    hand to evaluate(backend=...) to check its host code without a GPU, and to compare the GPU's report against."""

    @staticmethod
    def _np(t):
        return None if t is None else t.detach().cpu().numpy()

    def edit_distance(self, tok, off, a, b, breakdown=False):
        import torch
        cost, sid = edit_distance(self._np(tok), self._np(off), self._np(a), self._np(b))
        cost, sid = torch.from_numpy(cost).to(a.device), torch.from_numpy(sid).to(a.device)
        return (cost, sid) if breakdown else cost

    def pairwise_edit_distance(self, tok, off, uoff):
        import torch
        dist, doff = pairwise(self._np(tok), self._np(off), self._np(uoff))
        return torch.from_numpy(dist).to(uoff.device), torch.from_numpy(doff).to(uoff.device)

    def nbest_select(self, ac, g, lm, nn, length, uoff, grid):
        import torch
        H = int(uoff[-1])
        return torch.from_numpy(select(*(self._np(t) for t in (ac, g, lm, nn, length)), self._np(uoff), list(grid), H)).to(uoff.device)

    def nbest_mbr(self, ac, g, lm, nn, length, uoff, dist, doff, grid, want_risk=True):
        import torch
        H = int(uoff[-1])
        risk, pick = mbr(*(self._np(t) for t in (ac, g, lm, nn, length)), self._np(uoff), self._np(dist), self._np(doff), list(grid), H)
        return torch.from_numpy(risk).to(uoff.device), torch.from_numpy(pick).to(uoff.device)
