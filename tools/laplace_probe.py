#!/usr/bin/env python3
"""What the last-layer Laplace posterior costs: its three kernels and two products beside their neighbours, and
engine.fit_laplace / engine.evaluate_laplace beside engine.evaluate_report.

A. On 2048 decoder rows of the configs[2] shape (K = 512) and of the configs[1] shape (K = 1024), V = 33,000: kernel time by
   device events around the call, median of 9 rounds after one warm-up round, every leg in every round.  Every (2048, V) matrix
   exists three times and the rounds rotate through the sets (3 x 270 MB per operand: no launch finds its rows in the 256 MB
   Infinity Cache).  Legs: blm_laplace_curvature in place; the accumulate product (TN, ACCUMULATE, colsum_a) into F; the
   variance product ops.linear(h^2, S_w, s_b); blm_laplace_row_stats with either link beside blm_row_stats on the same rows;
   blm_laplace_mc_rows at S = 2 / 8 / 32.  GB/s = matrices moved x bytes / time where the kernel is bound by them.
B. tokens/s of engine.fit_laplace and of engine.evaluate_laplace (probit, expexp, mc with 8 samples) beside
   engine.evaluate_report on one synthetic text at the shapes' own (seq_len, columns): each after one warm-up call, median of
   3, a device synchronise inside the timed window.

The weights are freshly initialised unless ``--model-path`` loads trained ones (the configs[2] Transformer): the runs time
the code and say NOTHING about the calibration or perplexity a trained model gains.

usage: laplace_probe.py [--out PATH] [--model-path PATH] [rows|engine ...]
       (default: both; PATH defaults to profiles/r20_laplace_probe.txt)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from bayeslms_amd import engine, laplace, model as M, ops  # noqa: E402
from bayeslms_amd.data import batchify, synthetic_corpus  # noqa: E402

dev = torch.device("cuda:0")
out_file = None
model_path = None
SEED = 1111


def say(*a):
    print(*a, flush=True)
    if out_file is not None:
        print(*a, file=out_file, flush=True)


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def rotation(legs, rounds=10):
    times = {k: [] for k, _, _ in legs}
    for rnd in range(rounds):
        for k, _, fn in legs:
            us = event_us(lambda: fn(rnd))
            if rnd:
                times[k].append(us)
    return times


def rows_legs():
    R, V = 2048, bench.V
    for name, K in (("configs[2] decoder", bench.D_MODEL), ("configs[1] decoder", 1024)):
        gen = torch.Generator(device=dev).manual_seed(9)
        with torch.no_grad():
            sets = [dict(z=torch.randn(R, V, device=dev, generator=gen) * 3, var=torch.rand(R, V, device=dev, generator=gen),
                         a=torch.rand(R, V, device=dev, generator=gen) * 1e-3, h=torch.randn(R, K, device=dev, generator=gen))
                    for _ in range(3)]
            for s in sets:
                s["h2"] = ops._lrt_prepare(s["h"], 0)
            tg = torch.randint(0, V, (R,), device=dev, generator=gen)
            post = laplace.LaplacePosterior(V, K, dev)
            s_w, s_b = torch.rand(V, K, device=dev, generator=gen), torch.rand(V, device=dev, generator=gen)
            mb = R * V * 4 / 1e6
            legs = [("blm_laplace_curvature in place", 2, lambda r: ops.laplace_curvature(sets[r % 3]["z"], out=sets[r % 3]["z"])),
                    ("accumulate product TN + colsum_a", None, lambda r: post.accumulate(sets[r % 3]["a"], sets[r % 3]["h2"])),
                    ("variance product ops.linear", None, lambda r: ops.linear(sets[r % 3]["h2"], s_w, s_b)),
                    ("logits product ops.linear", None, lambda r: ops.linear(sets[r % 3]["h"], s_w, s_b)),
                    ("blm_row_stats", 1, lambda r: ops.row_stats(sets[r % 3]["var"], tg)),
                    ("blm_laplace_row_stats probit", 2, lambda r: ops.laplace_row_stats(sets[r % 3]["var"], sets[(r + 1) % 3]["var"], tg, "probit")),
                    ("blm_laplace_row_stats expexp", 2, lambda r: ops.laplace_row_stats(sets[r % 3]["var"], sets[(r + 1) % 3]["var"], tg, "expexp"))]
            legs += [("blm_laplace_mc_rows S = %d" % S, None,
                      lambda r, S=S: ops.laplace_mc_rows(sets[r % 3]["var"], sets[(r + 1) % 3]["var"], S, SEED, tg, 0)) for S in (2, 8, 32)]
            say("# A. %s: %d x %d rows (%.1f MB per matrix), K = %d, three sets in rotation; us per call, median of 9 rounds"
                % (name, R, V, mb, K))
            times = rotation(legs)
            for k, streams, _ in legs:
                us = statistics.median(times[k])
                rate = "" if streams is None else "  %d matrices  %7.1f GB/s" % (streams, streams * R * V * 4 / (us * 1e-6) / 1e9)
                say("  %-36s %10.1f us%s  (min %.1f max %.1f us)" % (k, us, rate, min(times[k]), max(times[k])))
            del sets, post, s_w


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), r


def engine_legs():
    say("# B. fit_laplace and evaluate_laplace beside evaluate_report, tokens/s, median of 3 calls.  %s"
        % ("weights of %s (Transformer)" % model_path if model_path else
           "FRESHLY INITIALISED weights: these runs time the code and say nothing about the calibration a trained model gains"))
    for which in ("transformer", "lstm"):
        torch.manual_seed(SEED)
        if which == "transformer":
            m, seq, cols = M.TransformerModel(bench.V, bench.D_MODEL, bench.NHEAD, bench.D_FF, bench.NLAYERS, 0.2, "gelu", True), 128, 20
            if model_path:
                from bayeslms_amd.compute_sentence_scores import load_partial
                load_partial(m, model_path)
        else:
            m, seq, cols = M.RNNModel("LSTM", bench.V, 1024, 1024, 2, 0.2, True), 35, 20
        m = m.to(dev).eval()
        src = batchify(synthetic_corpus(bench.V, cols * (12 * seq + 1), seed=2222), cols, dev)
        n = (src.size(0) - 1) * cols
        t_rep, rep = timed(lambda: engine.evaluate_report(m, src, seq))
        t_fit, post = timed(lambda: engine.fit_laplace(m, src, seq))
        say("%s of the %s shape, 12 windows of %d x %d, %d tokens, V %d:" % (which, "configs[2]" if which == "transformer" else "configs[1]",
                                                                           cols, seq, n, bench.V))
        say("  evaluate_report, mean weights        %9.0f tokens/s (%.1f ms), loss %.4f" % (n / t_rep, 1e3 * t_rep, rep.loss))
        say("  fit_laplace                          %9.0f tokens/s (%.1f ms): %.2f x evaluate_report's time" % (n / t_fit, 1e3 * t_fit, t_fit / t_rep))
        for link, S in (("probit", 0), ("expexp", 0), ("mc", 8)):
            t, r = timed(lambda: engine.evaluate_laplace(m, src, seq, post, 100.0, link=link, samples=S))
            say("  evaluate_laplace %-6s%s   %9.0f tokens/s (%.1f ms): %.2f x evaluate_report's time, loss %.4f"
                % (link, " S = %d" % S if S else "      ", n / t, 1e3 * t, t / t_rep, r.loss))
        t, fit = timed(lambda: engine.fit_laplace_prior(m, src, seq, post, [1.0, 10.0, 100.0, 1000.0]), reps=1)
        say("  fit_laplace_prior, 4 + 1 candidates, probit: %.1f ms (%.2f x evaluate_report's time); tau %g, loss %.4f -> %.4f"
            % (1e3 * t, t / t_rep, fit.tau, fit.loss_base, fit.loss))
        del m, post


if __name__ == "__main__":
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "r20_laplace_probe.txt")
    for flag in ("--out", "--model-path"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                path = args[i + 1]
            else:
                model_path = args[i + 1]
            del args[i:i + 2]
    with open(path, "w") as out_file:
        for w in (args or ["rows", "engine"]):
            {"rows": rows_legs, "engine": engine_legs}[w]()
