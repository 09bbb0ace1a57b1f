"""What n-best rescoring over prefix tries buys (compute_scores_batched(share_prefixes=True), --share-prefixes 1).

For each leg and n-best shape: hypotheses/s with the flag off and on, alternated in one process after a warm-up (median, min and
max over --reps runs each), the worst score difference on against off, the trie's share of rows (nodes / tokens, edges / tokens)
and the host milliseconds of the trie builds of one run.

  legs    cfg2       configs[2]-shaped Bayesian Transformer (--T_bayes_pos FFN, d 512, 8 heads, 6 layers), mean weights
          cfg4       configs[4] GP Transformer (--T_gauss_pos 3), mean weights
          cfg4_mc8   the same with 8 Monte-Carlo weight samples
          cfg1       configs[1] Bayesian LSTM (--L_bayes_pos 3, 1024 units, 2 layers), mean weights
          interp     the cfg2 Transformer interpolated with a second (non-Bayesian) one, alpha 0.8
  shapes  a  bench.synthetic_nbest 20-best (base sentence + up to three substitutions anywhere)
          b  late divergence: the 20 hypotheses differ only in the last third of their words
          c  no sharing: every hypothesis differs at its first word (the overhead case)
All at 33,000 words.  --legs / --shapes pick a subset (comma-separated); --out also writes the report to a file.
"""
import argparse
import random
import statistics
import sys
import time
from collections import OrderedDict

sys.path.insert(0, ".")

VW = 33000


def shape_nbest(shape, n_utt, n_hyp, seed=7):
    from bench import synthetic_nbest
    if shape == "a":
        nb, vocab, _ = synthetic_nbest(n_utt, n_hyp, VW, seed)
        return nb, vocab
    rnd = random.Random(seed)
    words = ["w%d" % i for i in range(VW - 2)]
    vocab = {w: i + 2 for i, w in enumerate(words)}
    vocab["<s>"], vocab["<unk>"] = 0, 1
    nb = OrderedDict()
    for u in range(n_utt):
        ln = max(3, min(60, 1 + int(rnd.expovariate(1 / 7.0)) + 3))
        base = [rnd.choice(words) for _ in range(ln)]
        hyps = []
        for _ in range(n_hyp):
            h = list(base)
            if shape == "b":  # substitutions in the last third only
                lo = ln - max(1, ln // 3)
                for _ in range(rnd.randint(1, 3)):
                    h[rnd.randrange(lo, ln)] = rnd.choice(words)
            else:  # "c": a different first word for every hypothesis
                h[0] = rnd.choice(words)
                for _ in range(rnd.randint(0, 3)):
                    h[rnd.randrange(ln)] = rnd.choice(words)
            hyps.append(" ".join(h))
        nb["utt%04d" % u] = hyps
    return nb, vocab


def build_leg(leg, dev):
    import torch
    from bayeslms_amd import model as M
    torch.manual_seed(1111)
    if leg in ("cfg2", "interp"):
        m1, mt = M.BayesTransformerModel(VW, 512, 8, 4096, 6, 0.5, True, "FFN"), "Transformer"
    elif leg in ("cfg4", "cfg4_mc8"):
        m1, mt = M.GaussTransformerModel(VW, 512, 8, 4096, 6, 0.5, True, 3), "Transformer"
    elif leg == "cfg1":
        m1, mt = M.BayesRNNModel("LSTM", VW, 1024, 1024, 2, 0.5, True, 3), "LSTM"
    else:
        raise SystemExit("unknown leg %s" % leg)
    m2 = M.BayesTransformerModel(VW, 512, 8, 4096, 6, 0.5, True, "none").to(dev) if leg == "interp" else None
    return m1.to(dev), m2, mt, (8 if leg == "cfg4_mc8" else 0)


def trie_stats(nbest, vocab):
    import numpy as np
    from bayeslms_amd.compute_sentence_scores import get_input_and_target
    from bayeslms_amd.prefix_trie import build_trie
    cols, utt = [], []
    for u, hyps in enumerate(nbest.values()):
        for h in hyps:
            cols.append(get_input_and_target(h, vocab))
            utt.append(u)
    lens = np.array([len(x) for x, _ in cols])
    data = np.zeros((lens.max(), len(cols)), dtype=np.int64)
    for n, (x, _) in enumerate(cols):
        data[: len(x), n] = x
    tr = build_trie(data, lens, np.concatenate([np.asarray(t) for _, t in cols]), np.asarray(utt))
    R = float(lens.sum())
    return tr.sel.shape[0] / R, tr.edge_node.shape[0] / R


def run_leg(leg, shape, reps, n_utt, n_hyp, log):
    import torch
    from bayeslms_amd import compute_sentence_scores as css
    dev = torch.device("cuda:0")
    nbest, vocab = shape_nbest(shape, n_utt, n_hyp)
    m1, m2, mt, S = build_leg(leg, dev)
    total = sum(len(h) for h in nbest.values())
    host = []
    real_build = css.build_trie

    def timed_build(*a):
        t0 = time.perf_counter()
        out = real_build(*a)
        host.append(time.perf_counter() - t0)
        return out

    def run(share):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = css.compute_scores_batched(nbest, m1, vocab, mt, dev, model_2=m2, alpha=0.8 if m2 is not None else 0.0, mc_samples=S,
                                         share_prefixes=share)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    run(False)
    run(True)  # warm-up: code objects, plans, allocator
    t = {False: [], True: []}
    for _ in range(reps):
        for share in (False, True):
            t[share].append(run(share)[0])
    css.build_trie = timed_build
    try:
        _, on = run(True)
    finally:
        css.build_trie = real_build
    _, off = run(False)
    worst = max(abs(a - b) / max(1.0, abs(b)) for k in off for (_, a), (_, b) in zip(on[k], off[k]))
    nodes, edges = trie_stats(nbest, vocab)
    med = {s: statistics.median(t[s]) for s in t}
    log("%-9s shape %s  %d hyps  nodes/tokens %.3f  edges/tokens %.3f  trie build %.1f ms host per run (%d batches)"
        % (leg, shape, total, nodes, edges, sum(host) * 1e3, len(host)))
    for s in (False, True):
        d = t[s]
        log("    share %-3s  median %.3f s (min %.3f, max %.3f, %d runs)  %8.0f hypotheses/s"
            % ("on" if s else "off", med[s], min(d), max(d), len(d), total / med[s]))
    log("    on / off speed-up %.3f (medians; min-max range %.3f .. %.3f)  worst score difference %.2e relative"
        % (med[False] / med[True], min(t[False]) / max(t[True]), max(t[False]) / min(t[True]), worst))
    del m1, m2
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", type=str, default="cfg2,cfg4,cfg4_mc8,cfg1,interp")
    ap.add_argument("--shapes", type=str, default="a,b,c")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--utts", type=int, default=1000)
    ap.add_argument("--hyps", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    log("prefix_share_probe: %s, %d utterances x %d-best, %d alternated runs per setting after warm-up"
        % (torch.cuda.get_device_name(0), a.utts, a.hyps, a.reps))
    for leg in a.legs.split(","):
        for shape in a.shapes.split(","):
            run_leg(leg, shape, a.reps, a.utts if leg != "cfg4_mc8" else max(1, a.utts // 4), a.hyps, log)
            if a.out:
                with open(a.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
