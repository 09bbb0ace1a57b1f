#!/usr/bin/env python3
"""The device-resident beam search (IncrementalLM.beam_search) against the same search over the older public API, and the
search with a finished-hypothesis pool (IncrementalLM.beam_search_pool) beside them, and the selection kernels on their own.

    python tools/beam_probe.py [--out profiles/r07_beam_probe.txt] [--quick]

1. words/s of IncrementalLM._beam_trace (step -> blm_topk_rows -> blm_beam_select -> reorder_device, no host read inside the
   loop) against step -> torch.topk -> .cpu() -> numpy selection -> host-index reorder, for the configs[2] Transformer and the
   configs[1] LSTM, vocabulary 33,000, a 128-word prompt, G x B in 1x4, 1x8, 1x16, 8x8, 1x64; eos is a word id the random
   model has no reason to prefer, so both sides generate all WORDS words.  The pooled search (step -> blm_topk_rows(k = 2 B) ->
   blm_beam_select_pool -> reorder_device, a pool of B) is the third side at every point.  The sides alternate inside one
   process; each figure is the median of REPS timed searches after one warm-up search, and the spread (max - min) / median is
   printed.
2. blm_topk_rows against torch.topk on the same (R, 33,000) rows, R 8 / 64 / 512, k 8 / 64, with R x V x 4 bytes over the
   kernel's time beside the 8 TB/s HBM figure (rows this small may be served from L2 or the Infinity Cache, not HBM).
3. blm_sample_rows_filtered (top_k 50; top_p 0.9; both) against blm_sample_rows on the same rows.

Times are host clocks around work that ends in a device synchronise (1) and HIP events around back-to-back launches (2, 3)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import beam_reference as REF  # noqa: E402  (the old-API driver of the equality test)
from bayeslms_amd import _lib as L  # noqa: E402
from bayeslms_amd import ops  # noqa: E402
from bayeslms_amd.incremental import IncrementalLM  # noqa: E402
from decode_probe import V, _events, build  # noqa: E402

CTX, WORDS, REPS = 128, 32, 3


def search_rates(kind, m, G, B, dev, say):
    lm = IncrementalLM(m, max_streams=G * B, max_len=CTX + WORDS)
    rng = np.random.default_rng(G * 1000 + B)
    prompts = [[int(t) for t in rng.integers(1, V, size=CTX)] for _ in range(G)]
    eos = 0

    def topk_host(lp):
        v, i = torch.topk(lp, B, dim=1)
        return v.cpu().numpy(), i.cpu().numpy()

    def new():
        return lm._beam_trace(prompts, B, WORDS, eos, sync_every=16)

    def old():
        return REF.beam_search_old_api(lm, prompts, B, WORDS, eos, topk_host)

    def pooled():  # step -> blm_topk_rows(k = 2 B) -> blm_beam_select_pool -> reorder_device, a pool of B per prompt
        return lm.beam_search_pool(prompts, B, WORDS, eos, pool=B, sync_every=16)
    with torch.no_grad():
        a, b = new(), old()  # warm-up of every shape, and the two searches side by side
        same = bool(np.array_equal(a[1], b[1]))
        pooled()
        t = {"new": [], "old": [], "pool": []}
        for _ in range(REPS):
            for name, fn in (("new", new), ("old", old), ("pool", pooled)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[name].append(time.perf_counter() - t0)
    mn, mo = statistics.median(t["new"]), statistics.median(t["old"])
    sn, so = (max(t["new"]) - min(t["new"])) / mn, (max(t["old"]) - min(t["old"])) / mo
    say("%-4s G x B = %d x %-2d  device search %8.1f words/s (%7.2f ms/word, spread %4.1f %%) | old API %8.1f words/s (%7.2f ms/word, "
        "spread %4.1f %%) | device / old %.2fx  same tokens: %s"
        % (kind, G, B, WORDS / mn, mn / WORDS * 1e3, 100 * sn, WORDS / mo, mo / WORDS * 1e3, 100 * so, mo / mn, same))
    mp = statistics.median(t["pool"])
    sp = (max(t["pool"]) - min(t["pool"])) / mp
    say("%-4s G x B = %d x %-2d  pooled search %8.1f words/s (%7.2f ms/word, spread %4.1f %%) | pooled / device %.2fx the time per word | "
        "old API / pooled %.2fx" % (kind, G, B, WORDS / mp, mp / WORDS * 1e3, 100 * sp, mp / mn, mo / mp))
    if mp > mo * (1.0 + max(sp, so)):
        say("#    the pooled search is SLOWER than the old-API search here, beyond the spread")
    return mo / mn, max(sn, so)


def topk_alone(dev, say):
    for R in (8, 64, 512):
        x = torch.log_softmax(torch.randn(R, V, device=dev) * 3, -1)
        for k in (8, 64):
            def ours():
                for _ in range(20):
                    ops.topk_rows(x, k)

            def theirs():
                for _ in range(20):
                    torch.topk(x, k, dim=1)
            ours(), theirs()
            to, tt = _events(ours, 5)[0] / 20, _events(theirs, 5)[0] / 20
            nbytes = R * V * 4
            say("topk R=%-3d k=%-2d: blm_topk_rows %7.1f us (%5.2f TB/s of R x V x 4 = %.1f MB; HBM 8 TB/s, rows may come from "
                "L2) | torch.topk %7.1f us | torch / ours %.2fx" % (R, k, to * 1e3, nbytes / (to * 1e-3) / 1e12, nbytes / 1e6, tt * 1e3, tt / to))


def sampling_alone(dev, say):
    for R in (8, 64):
        x = torch.log_softmax(torch.randn(R, V, device=dev) * 3, -1)

        def run(**kw):
            def f():
                for i in range(20):
                    ops.sample_rows(x, 1.0, 1, 0, i, **kw)
            f()
            return _events(f, 5)[0] / 20 * 1e3
        base = run()
        say("sample R=%-2d: blm_sample_rows %6.1f us | filtered top_k 50: %6.1f us  top_p 0.9: %6.1f us  top_k 50 + top_p 0.9: %6.1f us"
            % (R, base, run(top_k=50), run(top_p=0.9), run(top_k=50, top_p=0.9)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r07_beam_probe.txt")
    ap.add_argument("--quick", action="store_true", help="the Transformer at 1x8 and the kernels only")
    ap.add_argument("--searches-only", action="store_true", help="part 1 only (the three searches)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L.require_gfx950()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/beam_probe.py: V %d, prompt %d words, %d generated words per search, median of %d, both sides alternated" % (V, CTX, WORDS, REPS))
    say("# 1. beam search: device-resident against the older public API, and the search with a finished-hypothesis pool of B beside "
        "them (host clock around a search that ends in a synchronise)")
    slower = []
    for kind in (("tlm",) if args.quick else ("tlm", "lstm")):
        m = build(kind, dev)
        for G, B in (((1, 8),) if args.quick else ((1, 4), (1, 8), (1, 16), (8, 8), (1, 64))):
            ratio, spread = search_rates(kind, m, G, B, dev, say)
            if ratio < 1.0 - spread:
                slower.append("%s %dx%d (%.2fx, spread %.1f %%)" % (kind, G, B, ratio, 100 * spread))
        del m
        torch.cuda.empty_cache()
    say("# device search slower than the old-API search beyond the spread at: %s" % (", ".join(slower) or "no measured point"))
    if args.searches_only:
        if args.out:
            _write(args.out, lines)
        return
    say("# 2. blm_topk_rows against torch.topk (HIP events, 20 calls per timing, median of 5)")
    topk_alone(dev, say)
    say("# 3. blm_sample_rows_filtered against blm_sample_rows (HIP events, 20 calls per timing, median of 5)")
    sampling_alone(dev, say)
    if args.out:
        _write(args.out, lines)


def _write(path, lines):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
