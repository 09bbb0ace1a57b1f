"""The prefix trie of a packed n-best batch (compute_scores_batched(share_prefixes=True)).

Under a causal Transformer, or an LSTM whose columns start from their utterance's carried state, a token's activations and its
next-word distribution depend on its prefix only: the hypotheses of one utterance share long prefixes, and every distinct prefix
needs computing once.  A node is a distinct (utterance, input-id prefix); an edge is a distinct (node, target) pair -- the
decoder's log-sum-exp runs once per node, the target's logit once per edge.

Pure numpy and vectorised over the batch (no Python loop per token or per hypothesis; one loop over depths):
  1. the columns are lexsorted by (utterance, input ids) with padding first, so a hypothesis that is a prefix of another sorts
     before it;
  2. each sorted row shares lcp[r] leading ids with the previous one (0 across utterances) and introduces the nodes at depths
     lcp[r] .. len[r] - 1, numbered in row order -- which is DFS preorder;
  3. the node of (row, depth) below lcp[r] is the one of the last row that introduced that depth (a forward maximum.accumulate);
     a node's subtree ends where the next row with lcp <= its depth starts (a reverse minimum.accumulate per depth);
  4. edges are np.unique over (node, target) keys.
"""
from typing import NamedTuple

import numpy as np


class PrefixTrie(NamedTuple):
    sel: np.ndarray       # (M,) int64 flat padded index t * N + n of one hypothesis that reaches the node; t = its depth
    end: np.ndarray       # (M,) int32 preorder index one past the node's subtree
    lo: np.ndarray        # (M,) int32 first node of the node's utterance
    edge_node: np.ndarray  # (E,) int64 node of each distinct (node, target) pair, ascending
    edge_tgt: np.ndarray   # (E,) int64 its target id
    tok_edge: np.ndarray   # (R,) int64 edge of each real token, n-major (hypothesis by hypothesis), as the padded path orders them


def build_trie(data, lens, tgt, utt):
    """``data`` (Tm, N) input ids (anything past a column's length is ignored), ``lens`` (N,) tokens per column (>= 1), ``tgt``
    (R,) target ids of the real tokens n-major (R = sum(lens)), ``utt`` (N,) utterance of each column; an utterance's columns
    need not be adjacent.  -> PrefixTrie; each utterance's nodes are contiguous and in preorder."""
    data = np.asarray(data, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    tgt = np.asarray(tgt, dtype=np.int64)
    utt = np.asarray(utt, dtype=np.int64)
    Tm, N = data.shape
    if lens.shape != (N,) or utt.shape != (N,):
        raise ValueError("build_trie: lens and utt need one entry per column of data")
    if N == 0:
        raise ValueError("build_trie: an empty batch")
    if lens.min() < 1 or lens.max() > Tm:
        raise ValueError("build_trie: every column holds 1..Tm tokens")
    R = int(lens.sum())
    if tgt.shape != (R,):
        raise ValueError("build_trie: %d targets for %d tokens" % (tgt.shape[0], R))
    pos = np.arange(Tm, dtype=np.int64)
    real = pos[None, :] < lens[:, None]                       # (N, Tm)
    key = np.where(real, data.T, -1)                          # padding sorts before every id
    perm = np.lexsort(tuple(key[:, t] for t in range(Tm - 1, -1, -1)) + (utt,))
    S, Ls, Us = key[perm], lens[perm], utt[perm]
    # longest common prefix with the previous sorted row, 0 across utterances
    lcp = np.zeros(N, dtype=np.int64)
    if N > 1:
        eq = (S[1:] == S[:-1]) & (pos[None, :] < np.minimum(Ls[1:], Ls[:-1])[:, None])
        lcp[1:] = np.where(Us[1:] == Us[:-1], np.cumprod(eq, axis=1).sum(axis=1), 0)
    cnt = Ls - lcp                                            # nodes row r introduces (0: a duplicate hypothesis)
    off = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(cnt, out=off[1:])
    M = int(off[-1])
    # node of (sorted row, depth): introduced by the last row <= r with lcp <= depth
    intro = (pos[None, :] >= lcp[:, None]) & (pos[None, :] < Ls[:, None])
    own = np.maximum.accumulate(np.where(intro, np.arange(N, dtype=np.int64)[:, None], -1), axis=0)
    node_of = off[own] + pos[None, :] - lcp[own]              # valid where pos < Ls
    # per node: owner row and depth
    nrow = np.repeat(np.arange(N, dtype=np.int64), cnt)
    ndep = np.arange(M, dtype=np.int64) - off[nrow] + lcp[nrow]
    sel = ndep * N + perm[nrow]
    # end: the first node of the first later row with lcp <= depth (every row of a later utterance has lcp 0)
    nxt = np.empty((Tm, N), dtype=np.int64)
    idx = np.arange(N, dtype=np.int64)
    for t in range(Tm):
        cand = np.where(lcp <= t, idx, N)
        cand = np.minimum.accumulate(cand[::-1])[::-1]        # smallest r' >= r with lcp[r'] <= t
        nxt[t, :-1] = cand[1:]
        nxt[t, -1] = N
    end = off[nxt[ndep, nrow]]
    first = np.ones(N, dtype=bool)
    first[1:] = Us[1:] != Us[:-1]
    urow = np.maximum.accumulate(np.where(first, idx, 0))     # first sorted row of each row's utterance
    lo = off[urow[nrow]]
    # tokens (n-major) -> nodes -> edges
    inv = np.empty(N, dtype=np.int64)
    inv[perm] = idx
    starts = np.zeros(N, dtype=np.int64)
    np.cumsum(lens[:-1], out=starts[1:])
    tok_n = np.repeat(idx, lens)
    tok_t = np.arange(R, dtype=np.int64) - starts[tok_n]
    tok_node = node_of[inv[tok_n], tok_t]
    if tgt.size and (tgt.min() < 0 or tgt.max() >= (1 << 31)):
        raise ValueError("build_trie: target ids must be in [0, 2^31)")
    ekey, tok_edge = np.unique((tok_node << 31) | tgt, return_inverse=True)
    return PrefixTrie(sel, end.astype(np.int32), lo.astype(np.int32), ekey >> 31, ekey & ((1 << 31) - 1),
                      tok_edge.reshape(-1).astype(np.int64))
