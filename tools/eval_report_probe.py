#!/usr/bin/env python3
"""engine.evaluate_report beside engine.evaluate, and blm_row_stats beside blm_log_softmax_rows.

A. The configs[2] Bayesian Transformer (6 x d 512, ff 4096, seq_len 128) and the configs[1] Bayesian LSTM (2 x 1024, seq_len 35)
   on bench._eval_leg's text (12 windows of 20 columns, V 33,000): tokens/s of evaluate (mean weights, fused NLL, nothing of
   width V stored), evaluate_report at S = 0, at S = 8, and at S = 8 with calibration=False.  Each after one warm-up call,
   median of 3, a device synchronise inside the timed window.
B. 2048 x 33,000 rows of logits: blm_row_stats (one read) beside blm_log_softmax_rows (three reads of the row, one write; the
   second and third read come from cache): kernel time by device events over 30 launches of the C entry points on pre-allocated
   outputs, three input buffers in turn so that no launch finds its rows in the Infinity Cache, median of 5, and the bytes each
   must move over that time.

usage: eval_report_probe.py [tlm|lstm|kernel ...]   (default: all three)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from bayeslms_amd import engine, model as M, ops  # noqa: E402
from bayeslms_amd.data import batchify, synthetic_corpus  # noqa: E402

dev = torch.device("cuda:0")


def say(*a):
    print(*a, flush=True)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), r


def model_legs(which):
    torch.manual_seed(1111)
    if which == "tlm":
        m, seq = M.BayesTransformerModel(bench.V, bench.D_MODEL, bench.NHEAD, bench.D_FF, bench.NLAYERS, bench.DROPOUT, True, "FFN"), 128
    else:
        m, seq = M.BayesRNNModel("LSTM", bench.V, 1024, 1024, 2, 0.2, True, 3), 35
    m = m.to(dev).eval()
    src = batchify(synthetic_corpus(bench.V, 20 * (12 * seq + 1), seed=2222), 20, dev)
    n = (src.size(0) - 1) * 20
    say("# A. %s: %d tokens (12 windows of 20 x %d), V %d; tokens/s, median of 3" % (which, n, seq, bench.V))
    legs = (("evaluate", lambda: engine.evaluate(m, src, seq)),
            ("evaluate_report S=0", lambda: engine.evaluate_report(m, src, seq)),
            ("evaluate_report S=8", lambda: engine.evaluate_report(m, src, seq, mc_samples=8)),
            ("evaluate_report S=8 calibration=False", lambda: engine.evaluate_report(m, src, seq, mc_samples=8, calibration=False)))
    for name, fn in legs:
        el, r = timed(fn, 3)
        say("%s %-40s %10.0f tokens/s  %8.2f ms  loss %.4f" % (which, name, n / el, 1e3 * el, r if isinstance(r, float) else r.loss))


def kernel_legs():
    """Kernel time, not call time: the C entry points on pre-allocated outputs, device events around 30 launches, and three
    input buffers taken in turn (810 MB: a launch never finds its rows in the 256 MiB Infinity Cache); median of 5."""
    from bayeslms_amd import _lib as L
    R, V, NB, N = 2048, 33000, 3, 30
    g = torch.Generator(device=dev).manual_seed(1)
    xs = [3.0 * torch.randn(R, V, device=dev, generator=g) for _ in range(NB)]
    outs = [torch.empty(R, V, device=dev) for _ in range(NB)]
    tgt = torch.randint(0, V, (R,), device=dev, generator=g)
    f = [torch.empty(R, device=dev) for _ in range(3)]
    i32 = [torch.empty(R, device=dev, dtype=torch.int32) for _ in range(2)]
    c, st = L.calls(), L.stream()
    say("# B. %d x %d rows of logits (%.0f MB), %d buffers in turn; us per launch by device events over %d launches, median of 5"
        % (R, V, R * V * 4 / 1e6, NB, N))
    legs = (("blm_row_stats", lambda k: c.blm_row_stats(xs[k].data_ptr(), V, tgt.data_ptr(), R, V, f[0].data_ptr(), f[1].data_ptr(),
                                                        f[2].data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(), st), 1),
            ("blm_row_stats (no targets)", lambda k: c.blm_row_stats(xs[k].data_ptr(), V, None, R, V, None, f[1].data_ptr(),
                                                                     f[2].data_ptr(), i32[0].data_ptr(), None, st), 1),
            ("blm_log_softmax_rows", lambda k: c.blm_log_softmax_rows(xs[k].data_ptr(), V, outs[k].data_ptr(), V, R, V, st), 2))
    for name, fn, passes in legs:
        for k in range(NB):
            fn(k)
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for j in range(N):
                fn(j % NB)
            e1.record()
            torch.cuda.synchronize()
            times.append(1e3 * e0.elapsed_time(e1) / N)
        us = statistics.median(times)
        nbytes = passes * R * V * 4
        say("%-28s %8.1f us  %6.2f TB/s of the %d MB it must move" % (name, us, nbytes / us / 1e6, nbytes // 10 ** 6))


if __name__ == "__main__":
    for w in (sys.argv[1:] or ["tlm", "lstm", "kernel"]):
        with torch.no_grad():
            kernel_legs() if w == "kernel" else model_legs(w)
