"""numpy reference models shared by tests/test_beam_cpu.py (which tests them on hand-written cases) and tests/test_gpu_beam.py
(which holds the kernels to them): the row order of blm_topk_rows, blm_beam_select in float32, the allowed set of
blm_sample_rows_filtered in float64, and a beam-search driver over IncrementalLM's older public API."""
import numpy as np


def row_order(x):
    """Indices of the 1-D array x in the library's total order: value descending, then index ascending; NaN after -inf
    (np.lexsort sorts NaN last; -0 == +0)."""
    x = np.asarray(x)
    return np.lexsort((np.arange(x.shape[0]), -x))


def topk_rows(x, k):
    """(R, V) -> (vals (R, k), ids (R, k) int64), values copied"""
    ids = np.stack([row_order(r)[:k] for r in x]).astype(np.int64)
    return np.take_along_axis(x, ids, 1), ids


def beam_select(cand_vals, cand_ids, score, finished, B, eos):
    """blm_beam_select in float32: -> (score, finished, parent, token) after the step"""
    cand_vals = np.asarray(cand_vals, dtype=np.float32)
    score = np.asarray(score, dtype=np.float32)
    n, k = cand_vals.shape
    so, fo = np.empty(n, np.float32), np.empty(n, np.uint8)
    po, to = np.empty(n, np.int64), np.empty(n, np.int64)
    for g0 in range(0, n, B):
        flat, sc = [], []
        for b in range(B):
            if finished[g0 + b]:
                flat.append(b * k)
                sc.append(score[g0 + b])
            else:
                with np.errstate(invalid="ignore"):
                    s = (score[g0 + b] + cand_vals[g0 + b]).astype(np.float32)  # one IEEE fp32 add each
                flat += [b * k + j for j in range(k)]
                sc += list(s)
        flat, sc = np.asarray(flat), np.asarray(sc, dtype=np.float32)
        best = np.lexsort((flat, -sc))[:B]
        for slot, c in enumerate(best):
            b, j = divmod(int(flat[c]), k)
            fin = bool(finished[g0 + b])
            tok = eos if fin else int(cand_ids[g0 + b, j])
            so[g0 + slot], fo[g0 + slot] = sc[c], 1 if (fin or tok == eos) else 0
            po[g0 + slot], to[g0 + slot] = g0 + b, tok
    return so, fo, po, to


def allowed_set(x, temperature, top_k, top_p):
    """float64: boolean mask of the entries of the 1-D row x a filtered draw may return, and the q-mass of the allowed prefix
    before and after its last entry (None, None when top_p does not bind) for the caller's margin check."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    order = row_order(x)
    z = x[order] / temperature
    q = np.exp(z - np.nanmax(z))
    q = np.where(np.isnan(q), 0.0, q)
    cum = np.cumsum(q / q.sum())
    n_p, before, after = V, None, None
    if top_p < 1.0:
        n_p = int(np.searchsorted(cum, top_p, side="left")) + 1  # shortest prefix whose mass reaches top_p
        n_p = min(n_p, V)
        before, after = (cum[n_p - 2] if n_p > 1 else 0.0), cum[n_p - 1]
    n = min(n_p, top_k if top_k > 0 else V)
    mask = np.zeros(V, dtype=bool)
    mask[order[:n]] = True
    return mask, before, after


def beam_search_old_api(lm, prompts, B, W, eos, select_rows):
    """Beam search over the API IncrementalLM had before the device-resident search: step, full rows copied to the host,
    selection on the host, host-index reorder.  select_rows(lp (n, V) device tensor) -> host (vals (n, B), ids (n, B)).
    -> (parents (W, n), tokens (W, n), final fp32 scores (n,))"""
    import torch
    G = len(prompts)
    n = G * B
    lens = [len(p) for p in prompts]
    ids = torch.zeros(max(lens), G, dtype=torch.int64)
    for g, p in enumerate(prompts):
        ids[:lens[g], g] = torch.tensor(p)
    st = lm.start(G)
    lp = lm.step(st, ids, n_new=lens)
    fork = np.repeat(np.arange(G), B)
    st = lm.reorder(st, fork)
    lp = lp.index_select(0, torch.as_tensor(fork).to(lp.device))
    score = np.full(n, -np.inf, dtype=np.float32)
    score[::B] = 0.0
    finished = np.zeros(n, dtype=np.uint8)
    P, T = [], []
    for w in range(W):
        vals, cand = select_rows(lp)
        score, finished, parent, token = beam_select(vals, cand, score, finished, B, eos)
        P.append(parent)
        T.append(token)
        if w + 1 == W:
            break
        st = lm.reorder(st, parent)
        lp = lm.step(st, torch.as_tensor(token))
    return np.stack(P), np.stack(T), score


def backtrace(P, T, slot, eos):
    toks = []
    for w in range(P.shape[0] - 1, -1, -1):
        toks.append(int(T[w, slot]))
        slot = int(P[w, slot])
    toks.reverse()
    return toks[:toks.index(eos) + 1] if eos in toks else toks
