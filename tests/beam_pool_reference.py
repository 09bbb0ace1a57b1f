"""numpy float32 model of blm_beam_select_pool and of the search loop around it, written from the semantics in
include/bayeslm.h (not from the kernel): candidates, order, walk, flush, pool, stopping.  tests/test_beam_pool_cpu.py tests it on
hand-written cases, tests/test_gpu_beam_pool.py holds the kernel and IncrementalLM.beam_search_pool to it bit for bit."""
import numpy as np

from beam_reference import topk_rows

F = np.float32


def precedes(a, b):
    """norm a comes strictly before norm b: greater, NaN last (NaN ties with NaN, -0 with +0)"""
    if a != a:
        return False
    return b != b or a > b


def inv_norm(length, a):
    """float32(1 / length ** a), formed in float64 and rounded once"""
    return F(1.0 / float(length) ** float(a))


def new_pool(G, P):
    return dict(norm=np.zeros((G, P), F), raw=np.zeros((G, P), F), len=np.zeros((G, P), np.int32), step=np.zeros((G, P), np.int32),
                parent=np.zeros((G, P), np.int64), finished=np.zeros((G, P), np.uint8), count=np.zeros(G, np.int32),
                inserted=np.zeros(G, np.int64))


FIELDS = ("norm", "raw", "len", "step", "parent", "finished")


def offer(pool, g, entry):
    """one entry (norm, raw, len, step, parent, finished) offered to group g's pool"""
    P = pool["norm"].shape[1]
    c = int(pool["count"][g])
    pool["inserted"][g] += 1
    if c == P:
        if not precedes(entry[0], pool["norm"][g, P - 1]):
            return
        c -= 1  # the last entry leaves
    at = c
    for i in range(c):
        if precedes(entry[0], pool["norm"][g, i]):  # later in insertion order than every entry held: behind its ties
            at = i
            break
    for name, v in zip(FIELDS, entry):
        pool[name][g, at + 1:c + 1] = pool[name][g, at:c].copy()
        pool[name][g, at] = v
    pool["count"][g] = c + 1


def select_pool(cand_vals, cand_ids, score, live, B, eos, step, length, min_len, inv, inv_max, flush, pool):
    """one call of blm_beam_select_pool; the pool (new_pool) is updated in place
    -> (score_out, live_out, parent, token, done (G,), all_done)"""
    cand_vals, score = np.asarray(cand_vals, F), np.asarray(score, F)
    inv, inv_max = F(inv), F(inv_max)
    n, k = cand_vals.shape
    G = n // B
    so, lo = np.full(n, -np.inf, F), np.zeros(n, np.uint8)
    po, to = np.arange(n, dtype=np.int64), np.full(n, eos, np.int64)
    done = np.zeros(G, np.uint8)
    for g in range(G):
        g0 = g * B
        cands = []
        for b in range(B):
            if not live[g0 + b]:
                continue
            with np.errstate(invalid="ignore"):
                s = (score[g0 + b] + cand_vals[g0 + b]).astype(F)  # one fp32 add each
            for j in range(k):
                tok = int(cand_ids[g0 + b, j])
                if not s[j] > -np.inf or (tok == eos and length < min_len):
                    continue
                cands.append((s[j], b * k + j, b, tok))
        cands.sort(key=lambda c: (-float(c[0]), c[1]))
        beams = []
        for rank, (s, _, b, tok) in enumerate(cands[:min(2 * B, B * k)]):
            if tok == eos:
                if rank < B:
                    offer(pool, g, (s * inv, s, length, step, g0 + b, 1))
            elif len(beams) < B:
                beams.append((s, b, tok))
        if flush:
            for slot, (s, b, tok) in enumerate(beams):
                offer(pool, g, (s * inv, s, length, step, g0 + slot, 0))
        P = pool["norm"].shape[1]
        d = not beams or bool(flush) or (pool["count"][g] == P and precedes(pool["norm"][g, P - 1], beams[0][0] * inv_max))
        done[g] = d
        for slot, (s, b, tok) in enumerate(beams):
            po[g0 + slot], to[g0 + slot] = g0 + b, tok
            if not d:
                so[g0 + slot], lo[g0 + slot] = s, 1
    return so, lo, po, to, done, np.uint8(done.all())


def search(first_rows, advance, G, B, W, eos, P, a=0.0, min_len=0, stop=True):
    """The loop of IncrementalLM.beam_search_pool over any next-word model.  first_rows (G * B, V) float32: the rows after the
    prompts, every group's row repeated for its B beams; advance(parent, token) -> the next (G * B, V) rows.
    -> (pool, parents (w, G * B), tokens (w, G * B)), w the words run (stop: the loop ends once every group is done)"""
    n = G * B
    V = first_rows.shape[1]
    pool = new_pool(G, P)
    score, live = np.zeros(n, F), np.zeros(n, np.uint8)
    live[::B] = 1
    rows, PA, TK = first_rows, [], []
    inv_max = inv_norm(W, a) if stop else F(0.0)
    for w in range(W):
        vals, ids = topk_rows(rows, min(2 * B, V))
        score, live, parent, token, done, all_done = select_pool(vals, ids, score, live, B, eos, w, w + 1, min_len,
                                                                 inv_norm(w + 1, a), inv_max, w + 1 == W, pool)
        PA.append(parent)
        TK.append(token)
        if w + 1 == W or (stop and all_done):
            break
        rows = advance(parent, token)
    return pool, np.stack(PA), np.stack(TK)


def hypotheses(pool, PA, TK, eos):
    """-> per group, the pool's entries best first as (tokens, raw, norm, length, finished)"""
    out = []
    for g in range(pool["count"].shape[0]):
        hyps = []
        for e in range(int(pool["count"][g])):
            fin, cur, w = bool(pool["finished"][g, e]), int(pool["parent"][g, e]), int(pool["step"][g, e])
            toks = [eos] if fin else []
            for ww in range(w - 1 if fin else w, -1, -1):
                toks.append(int(TK[ww, cur]))
                cur = int(PA[ww, cur])
            toks.reverse()
            hyps.append((toks, F(pool["raw"][g, e]), F(pool["norm"][g, e]), int(pool["len"][g, e]), fin))
        out.append(hyps)
    return out


def search_lm(lm, prompts, B, W, eos, P, a=0.0, min_len=0, stop=True):
    """search() driven by IncrementalLM's public step / reorder on the host: full rows copied to the host every word, the
    selection in numpy, a host-index reorder.  Every launch has the shape beam_search_pool's has."""
    import torch
    G = len(prompts)
    lens = [len(p) for p in prompts]
    ids = torch.zeros(max(lens), G, dtype=torch.int64)
    for g, p in enumerate(prompts):
        ids[:lens[g], g] = torch.tensor(p)
    st = [lm.start(G)]
    lp = lm.step(st[0], ids, n_new=lens)
    fork = np.repeat(np.arange(G), B)
    st[0] = lm.reorder(st[0], fork)
    first = lp.index_select(0, torch.as_tensor(fork).to(lp.device)).cpu().numpy()

    def advance(parent, token):
        st[0] = lm.reorder(st[0], parent)
        return lm.step(st[0], torch.as_tensor(token)).cpu().numpy()
    pool, PA, TK = search(first, advance, G, B, W, eos, P, a, min_len, stop)
    return hypotheses(pool, PA, TK, eos)
