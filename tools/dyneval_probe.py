#!/usr/bin/env python3
"""What dynamic evaluation costs: the fused per-window update beside the same update composed from torch calls and beside the
training step's clip + SGD kernel, and engine.evaluate_dynamic beside engine.evaluate_report.

A. The flat buffers (engine.FlatBuffers) of the configs[2] Transformer (6 x d 512, ff 4096, Bayesian FFN) and the configs[1]
   LSTM (2 x 1024, Bayesian gate), V 33,000, freshly initialised: every leg on the SAME buffers in one rotation (leg after leg,
   round after round), kernel time by device events around the call, median of 9 rounds after one warm-up round; the gradient
   buffer is refilled before every timed call, outside the timed window (an update with zero_grad clears it).  Achieved bytes/s =
   streams x n x 4 bytes over that time, with the streams the algorithm needs: blm_dyneval_update reads p, g, p0 (and rms) and
   writes p (and g): 4 / 5 (sgd) and 5 / 6 (rms) without / with zero_grad; blm_dyneval_accum 3; blm_clip_sgd_multi reads p, g, m
   and writes p, m: 5; ops.clip_sgd adds the read of g by blm_sqnorm_multi: 6.  The torch composition is given the streams of
   the fused update it replaces, so its figure is the useful rate, not the traffic it causes.
B. tokens/s of evaluate_dynamic (sgd rule at lr 0.002, and the rms rule at lr 2e-5 with statistics from 4 windows; under the rms
   rule every live weight moves by about lr per window whatever its gradient, so it wants the far smaller rate) beside
   evaluate_report on the same synthetic text at (seq_len, columns) = (128, 20), (35, 10) and (5, 1): each after one warm-up
   call, median of 3, a device synchronise inside the timed window.

The weights are freshly initialised unless ``--model-path`` loads trained ones into both legs' models: the runs time the code
and say NOTHING about the perplexity dynamic evaluation gains on a trained model.

usage: dyneval_probe.py [--out PATH] [--model-path PATH] [kernel|engine ...]
       (default: both; PATH defaults to profiles/r17_dyneval_probe.txt)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from bayeslms_amd import _lib as L, engine, model as M, ops  # noqa: E402
from bayeslms_amd.data import batchify, synthetic_corpus  # noqa: E402

dev = torch.device("cuda:0")
LR, LR_RMS, DECAY, EPS = 0.002, 2e-5, 0.02, 0.01
out_file = None
model_path = None


def say(*a):
    print(*a, flush=True)
    if out_file is not None:
        print(*a, file=out_file, flush=True)


def models():
    torch.manual_seed(1111)
    legs = (("configs[2] Transformer", lambda: M.BayesTransformerModel(bench.V, bench.D_MODEL, bench.NHEAD, bench.D_FF, bench.NLAYERS,
                                                                        bench.DROPOUT, True, "FFN")),
            ("configs[1] LSTM", lambda: M.BayesRNNModel("LSTM", bench.V, 1024, 1024, 2, 0.5, True, 3)))
    for name, make in legs:
        m = make()
        if model_path:
            from bayeslms_amd.compute_sentence_scores import load_partial
            load_partial(m, model_path)
        yield name, m.to(dev).eval()


def kernel_legs():
    c = L.calls()
    say("# A. per-window update on the flat buffers; us per call by device events, median of 9 rounds, every leg in every round; "
        "GB/s = streams x n x 4 / time")
    for name, m in models():
        flat = engine.FlatBuffers(m)
        n = flat.total
        p, g, mom = flat.flat_param, flat.flat_grad, flat.flat_mom
        gen = torch.Generator(device=dev).manual_seed(7)
        g_src = torch.randn(n, device=dev, generator=gen) * 1e-3
        p0 = p.clone()
        p.add_(torch.randn(n, device=dev, generator=gen) * 1e-3)
        ms = g_src * g_src
        ms[torch.rand(n, device=dev, generator=gen) < 0.3] = 0.0  # log sigma, padding, rows the statistics never saw
        rms, mean = ops.dyneval_rms(ms, 1)
        rbar = float(mean[0])
        table = ops.PtrTable([p], [g], [mom])
        table.sq.fill_(1.0)
        st = L.stream()

        def torch_sgd():
            t = p0 - p
            p.add_(g, alpha=-LR).add_(t, alpha=min(1.0, DECAY))
            g.zero_()

        def torch_rms():
            step = g * LR / (rms + EPS * rbar)
            d = torch.clamp(rms * (DECAY / rbar), max=1.0)
            t = (p0 - p) * d
            p.sub_(step).add_(t)
            g.zero_()

        legs = [("blm_dyneval_update sgd, zero_grad", 5, lambda: ops.dyneval_update(p, g, p0, LR, DECAY)),
                ("blm_dyneval_update sgd", 4, lambda: ops.dyneval_update(p, g, p0, LR, DECAY, zero_grad=False)),
                ("blm_dyneval_update rms, zero_grad", 6, lambda: ops.dyneval_update(p, g, p0, LR, DECAY, rms, mean, EPS)),
                ("blm_dyneval_update rms", 5, lambda: ops.dyneval_update(p, g, p0, LR, DECAY, rms, mean, EPS, zero_grad=False)),
                ("blm_dyneval_accum", 3, lambda: ops.dyneval_accum(ms, g)),
                ("torch calls, sgd + zero", 5, torch_sgd),
                ("torch calls, rms + zero", 6, torch_rms),
                ("blm_clip_sgd_multi alone", 5, lambda: c.blm_clip_sgd_multi(L.ptr(table.params), L.ptr(table.grads), L.ptr(table.bufs),
                                                                              L.ptr(table.sizes), 1, L.ptr(table.sq), 1.0, LR, 0.9, 0, 1.0, st)),
                ("ops.clip_sgd (norm + update)", 6, lambda: ops.clip_sgd(table, 1.0, LR, 0.9, False))]
        times = {k: [] for k, _, _ in legs}
        for rnd in range(10):
            for k, _, fn in legs:
                g.copy_(g_src)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        say("%s: n = %d floats (%.1f MB per buffer)" % (name, n, n * 4 / 1e6))
        rate = {}
        for k, streams, _ in legs:
            us = statistics.median(times[k])
            rate[k] = streams * n * 4 / (us * 1e-6) / 1e9
            say("  %-34s %9.1f us  %d streams  %7.1f GB/s  (min %.1f max %.1f us)" % (k, us, streams, rate[k], min(times[k]), max(times[k])))
        ref = rate["blm_clip_sgd_multi alone"]
        say("  bytes/s of the update over blm_clip_sgd_multi's: sgd+zero %.3f, rms+zero %.3f (expected >= 0.9); the update over the "
            "torch calls, time: sgd %.2f x, rms %.2f x"
            % (rate["blm_dyneval_update sgd, zero_grad"] / ref, rate["blm_dyneval_update rms, zero_grad"] / ref,
               statistics.median(times["torch calls, sgd + zero"]) / statistics.median(times["blm_dyneval_update sgd, zero_grad"]),
               statistics.median(times["torch calls, rms + zero"]) / statistics.median(times["blm_dyneval_update rms, zero_grad"])))
        assert bool(torch.isfinite(p).all())
        del flat, table, p, g, mom, p0, ms, rms, g_src, m


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
    say("# B. evaluate_dynamic beside evaluate_report, tokens/s, median of 3 calls.  %s"
        % ("weights of %s" % model_path if model_path else
           "FRESHLY INITIALISED weights: these runs time the code and say nothing about the perplexity gained on a trained model"))
    for name, m in models():
        for seq, cols, windows in ((128, 20, 12), (35, 10, 24), (5, 1, 48)):
            src = batchify(synthetic_corpus(bench.V, cols * (windows * seq + 1), seed=2222), cols, dev)
            train = batchify(synthetic_corpus(bench.V, cols * (4 * seq + 1), seed=3333), cols, dev)
            n = (src.size(0) - 1) * cols
            t_stats, stats = timed(lambda: engine.dyneval_stats(m, train, seq, 4), 1)
            with torch.no_grad():
                t_rep, rep = timed(lambda: engine.evaluate_report(m, src, seq))
            t_sgd, sgd = timed(lambda: engine.evaluate_dynamic(m, src, seq, LR, DECAY))
            t_rms, rms = timed(lambda: engine.evaluate_dynamic(m, src, seq, LR_RMS, DECAY, stats=stats, eps=EPS))
            say("%s seq_len %3d x %2d columns, %d windows, %d tokens: evaluate_report %9.0f tokens/s (%.1f ms); evaluate_dynamic sgd "
                "%9.0f (%.1f ms, %.2f x the time), rms %9.0f (%.1f ms, %.2f x); dyneval_stats of 4 windows %.1f ms; loss %.4f -> sgd "
                "%.4f, rms %.4f" % (name, seq, cols, windows, n, n / t_rep, 1e3 * t_rep, n / t_sgd, 1e3 * t_sgd, t_sgd / t_rep,
                                     n / t_rms, 1e3 * t_rms, t_rms / t_rep, 1e3 * t_stats, rep.loss, sgd.loss, rms.loss))
        del m


if __name__ == "__main__":
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "r17_dyneval_probe.txt")
    for flag in ("--out", "--model-path"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                path = args[i + 1]
            else:
                model_path = args[i + 1]
            del args[i:i + 2]
    with open(path, "w") as out_file:
        for w in (args or ["kernel", "engine"]):
            {"kernel": kernel_legs, "engine": engine_legs}[w]()
