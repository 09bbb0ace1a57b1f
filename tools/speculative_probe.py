#!/usr/bin/env python3
"""Speculative sampling (bayeslms_amd/speculative.py) beside plain generation from the model average, and blm_spec_accept on its
own.

    python tools/speculative_probe.py [--out profiles/r15_speculative_probe.txt] [--quick] [--model-path trained.pt --kind tlm|lstm]

1. words/s of SpeculativeLM.generate (target: IncrementalLM(mc_samples=8), draft: the same model at its mean weights) beside plain
   generation with mc_samples 8 -- step + blm_sample_rows per word, what bayeslms_amd.generate runs -- in the same process, for
   the configs[2] Transformer and the configs[1] LSTM, vocabulary 33,000, a 128-word prompt, gamma 2 / 4 / 8 at 1 and 16 streams.
   The sides alternate; each figure is the median of REPS timed runs after one warm-up run, with the spread (max - min) / median.
   THE ACCEPTANCE RATE IS PRINTED NEXT TO EVERY RATE: freshly initialised weights say little about trained ones (their model
   average and their mean-weight model may agree far more, or far less, than a trained model's do), and the speed of the loop
   is a function of that rate.  --model-path loads a trained checkpoint of the chosen kind instead.
   By operation count a round costs gamma draft steps + S passes over gamma + 1 rows, against (accepted + 1) x S single-row passes.
2. blm_spec_accept against blm_sample_rows on the same (gamma + 1) x N target rows (HIP events around back-to-back launches):
   the verification reads two rows per position and draws two keys per column where the plain draw reads one and draws one.

Times in 1 are host clocks around runs that end in a device synchronise."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayeslms_amd import _lib as L  # noqa: E402
from bayeslms_amd import ops  # noqa: E402
from bayeslms_amd.incremental import IncrementalLM  # noqa: E402
from bayeslms_amd.speculative import STREAM_PLAIN, SpeculativeLM  # noqa: E402
from decode_probe import V, _events, build  # noqa: E402

CTX, WORDS, REPS, S = 128, 32, 3, 8


def plain_generate(lm, ctx, words, n, seed):
    """bayeslms_amd.generate.generate's loop: one step and one draw per word"""
    st = lm.start(n)
    ids = torch.tensor(ctx, dtype=torch.int64, device=lm.device).view(-1, 1).expand(-1, n).contiguous()
    out = torch.empty(words, n, dtype=torch.int64, device=lm.device)
    for i in range(words):
        nxt = ops.sample_rows(lm.step(st, ids), 1.0, seed, STREAM_PLAIN, i)
        out[i] = nxt
        ids = nxt.view(1, n)
    return out.cpu()


def loop_rates(kind, m, n, gamma, say):
    g = torch.Generator().manual_seed(n * 100 + gamma)
    ctx = [int(t) for t in torch.randint(1, V, (CTX,), generator=g)]
    target = IncrementalLM(m, max_streams=n, max_len=CTX + WORDS + gamma, mc_samples=S)
    spec = SpeculativeLM(target, None, gamma)
    stats = []

    def fast():
        stats.append(spec.generate(ctx, WORDS, n, 1.0, 7)[1])

    def plain():
        plain_generate(target, ctx, WORDS, n, 7)
    with torch.no_grad():
        fast(), plain()  # warm-up of every shape
        t = {"spec": [], "plain": []}
        for _ in range(REPS):
            for name, fn in (("spec", fast), ("plain", plain)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[name].append(time.perf_counter() - t0)
    ms, mp = statistics.median(t["spec"]), statistics.median(t["plain"])
    ss, sp = (max(t["spec"]) - min(t["spec"])) / ms, (max(t["plain"]) - min(t["plain"])) / mp
    st = stats[-1]
    say("%-4s streams %-2d gamma %d  speculative %8.1f words/s per stream (%7.2f ms/word, spread %4.1f %%) | plain mc_samples %d %8.1f "
        "words/s (%7.2f ms/word, spread %4.1f %%) | plain / speculative %.2fx the time | ACCEPTANCE RATE %.3f, %.2f words per target "
        "chunk, %d rounds" % (kind, n, gamma, WORDS / ms, ms / WORDS * 1e3, 100 * ss, S, WORDS / mp, mp / WORDS * 1e3, 100 * sp, mp / ms,
                              st.acceptance_rate, st.words_per_chunk(gamma), st.rounds))
    return mp / ms, max(ss, sp)


def kernel_alone(dev, say):
    for gamma, n in ((2, 1), (4, 1), (8, 1), (2, 16), (4, 16), (8, 16)):
        P = torch.log_softmax(torch.randn(gamma + 1, n, V, device=dev) * 3, -1)
        Q = torch.log_softmax(P[:gamma] + torch.randn(gamma, n, V, device=dev), -1)
        x = ops.sample_rows(Q.view(-1, V), 1.0, 1, 1, 0).view(gamma, n)

        def verify():
            for i in range(20):
                ops.spec_accept(P, Q, x, 1.0, 1, 2, i)

        def draw():
            for i in range(20):
                ops.sample_rows(P.view(-1, V), 1.0, 1, 2, i)
        verify(), draw()
        tv, td = _events(verify, 5)[0] / 20, _events(draw, 5)[0] / 20
        say("gamma %d streams %-2d (%3d rows of %d): blm_spec_accept %6.1f us (both launches) | blm_sample_rows on the target rows %6.1f us | "
            "ratio %.2f" % (gamma, n, (gamma + 1) * n, V, tv * 1e3, td * 1e3, tv / td))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r15_speculative_probe.txt")
    ap.add_argument("--quick", action="store_true", help="the Transformer at gamma 4 and the kernel only")
    ap.add_argument("--model-path", default="", help="a trained checkpoint (state dict) of the --kind model instead of fresh weights")
    ap.add_argument("--kind", default="", choices=("", "tlm", "lstm"), help="with --model-path: which of the two models it holds")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L.require_gfx950()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("# tools/speculative_probe.py: V %d, prompt %d words, %d generated words per stream, target mc_samples %d, draft = its own mean "
        "weights, median of %d, sides alternated" % (V, CTX, WORDS, S, REPS))
    say("# weights: %s" % (("the checkpoint %s" % os.path.basename(args.model_path)) if args.model_path else
                           "freshly initialised -- their acceptance rate says little about a trained model's"))
    say("# 1. SpeculativeLM.generate beside plain generation from the same model average (host clock around runs that end in a synchronise)")
    slower = []
    kinds = (args.kind,) if args.model_path else (("tlm",) if args.quick else ("tlm", "lstm"))
    for kind in kinds:
        m = build(kind, dev)
        if args.model_path:
            m.load_state_dict(torch.load(args.model_path, map_location=dev))
        for n in (1, 16):
            for gamma in ((4,) if args.quick else (2, 4, 8)):
                ratio, spread = loop_rates(kind, m, n, gamma, say)
                if ratio < 1.0 - spread:
                    slower.append("%s %d streams gamma %d (%.2fx, spread %.1f %%)" % (kind, n, gamma, ratio, 100 * spread))
        del m
        torch.cuda.empty_cache()
    say("# the speculative loop is slower than plain generation beyond the spread at: %s" % (", ".join(slower) or "no measured point"))
    say("# 2. blm_spec_accept against blm_sample_rows on the same target rows (HIP events, 20 calls per timing, median of 5)")
    kernel_alone(dev, say)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
