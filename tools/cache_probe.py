#!/usr/bin/env python3
"""blm_cache_scores on a text-sized band, and engine.evaluate_cache / fit_cache beside one engine.evaluate_report.

A. n = 245,000 synthetic rows (wikitext-2's test and validation texts are that long) drawn as N(0, 1) * 2 / K^(1/4), K 512 and
   1024, windows N 500 and 2000, J 1 and 8 thetas, labels over 33,000 words, q = k = the rows and hi[t] = t as the evaluation
   launches it: kernel time by device events around the C entry point on pre-allocated outputs, median of 5 after a warm-up
   launch; achieved TFLOP/s = 2 n N K over that time (the multiply-adds of the band alone, not those of the tile edges the
   kernel also computes) against the 157.3 TFLOP/s fp32 MFMA peak; eight thetas in one launch against eight launches of one.
B. max |got - want| / max(1, |want|) of lse and match against the float64 dense reference, per shape of tests/test_gpu_cache.py
   (the figures behind that test's bound).
C. The configs[2] Transformer (6 x d 512, ff 4096, seq_len 128) and the configs[1] LSTM (2 x 1024, seq_len 35) on bench._eval_leg's
   text shape, V 33,000: one evaluate_report, one evaluate_cache (window 2000) and a three-pass fit_cache, each after one warm-up
   call, median of 3, a device synchronise inside the timed window.  ``--model-path`` loads trained weights into the model of
   that leg (the flags of the evaluate command's defaults do not apply: the shapes above are fixed); without it the weights
   are freshly initialised, and the losses printed then say NOTHING about what a cache gains on a trained model -- only the times
   mean something.

usage: cache_probe.py [--out PATH] [--model-path PATH] [kernel|error|engine ...]
       (default: all three; PATH defaults to profiles/r16_cache_probe.txt)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import bench  # noqa: E402
from bayeslms_amd import engine, model as M, ops  # noqa: E402
from bayeslms_amd.data import batchify, synthetic_corpus  # noqa: E402

dev = torch.device("cuda:0")
PEAK_TF = 157.3
EIGHT = [0.0, 0.05, 0.1, 0.2, 0.35, 0.5, 0.75, 1.0]
out_file = None
model_path = None


def say(*a):
    print(*a, flush=True)
    if out_file is not None:
        print(*a, file=out_file, flush=True)


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


def kernel_legs():
    from bayeslms_amd import _lib as L
    n = 245000
    c, st = L.calls(), L.stream()
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.randint(0, 33000, (n,), device=dev, generator=g)
    hi = torch.arange(n, device=dev, dtype=torch.int32)
    lse, match = torch.empty(8, n, device=dev), torch.empty(8, n, device=dev)
    say("# A. blm_cache_scores, n = %d rows, q = k, hi[t] = t; ms per launch by device events, median of 5; TFLOP/s = 2 n N K / time, "
        "of the %.1f fp32 MFMA peak" % (n, PEAK_TF))
    for K in (512, 1024):
        h = torch.randn(n, K, device=dev, generator=g) * (2.0 / K ** 0.25)
        for N in (500, 2000):
            ms_of = {}
            for J in (1, 8):
                th = ops.cache_thetas(EIGHT[:J] if J == 8 else [0.5])

                def launch():
                    c.blm_cache_scores(h.data_ptr(), K, h.data_ptr(), K, y.data_ptr(), y.data_ptr(), None, hi.data_ptr(), N, n, n, K,
                                       L.C.byref(th), lse.data_ptr(), match.data_ptr(), None, st)
                launch()
                torch.cuda.synchronize()
                times = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    launch()
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1))
                ms = ms_of[J] = statistics.median(times)
                tf = 2.0 * n * N * K / (ms * 1e-3) / 1e12
                say("K %4d N %4d J %d  %9.3f ms  %6.1f TFLOP/s  %5.1f %% of peak  (min %.3f max %.3f ms)"
                    % (K, N, J, ms, tf, 100 * tf / PEAK_TF, min(times), max(times)))
            say("K %4d N %4d  eight thetas in one launch: %.3f ms against %.3f ms of eight J = 1 launches (%.2f of it)"
                % (K, N, ms_of[8], 8 * ms_of[1], ms_of[8] / (8 * ms_of[1])))
        del h


def error_legs():
    import cache_reference as R
    import test_gpu_cache as T
    say("# B. max |got - want| / max(1, |want|) against the float64 dense reference, the eight thetas of tests/test_gpu_cache.py "
        "(bound there: %g); entries at -inf agree exactly or the leg fails" % T.BOUND)
    for case in T.CASES:
        n, K, window, vocab = case
        h, y, hi, lse, match = T._case(case, dev)
        got = ops.cache_scores(h, h, y, y, hi, T._thetas(K), window)
        s = (h.double() @ h.double().t())
        errs = []
        for name, g, w in (("lse", got.lse, lse), ("match", got.match, match)):
            gi, wi = torch.isneginf(g), torch.isneginf(w)
            if not torch.equal(gi, wi):
                raise SystemExit("%s %s: -inf patterns differ" % (case, name))
            e = ((g.double() - w).abs() / w.abs().clamp(min=1.0))[~gi]
            errs.append(float(e.max()) if e.numel() else 0.0)
        say("n %4d K %4d N %4d V %7d  lse %.3g  match %.3g  (raw score std %.2f, theta <= %g)"
            % (n, K, window, vocab, errs[0], errs[1], float(s.std()), T._thetas(K)[-1]))


def engine_legs():
    torch.manual_seed(1111)
    legs = (("configs[2] Transformer", lambda: M.BayesTransformerModel(bench.V, bench.D_MODEL, bench.NHEAD, bench.D_FF, bench.NLAYERS,
                                                                        bench.DROPOUT, True, "FFN"), 128, 20, 12),
            ("configs[1] LSTM", lambda: M.BayesRNNModel("LSTM", bench.V, 1024, 1024, 2, 0.5, True, 3), 35, 20, 44))
    say("# C. evaluate_cache (window 2000) and fit_cache (3 passes) beside one evaluate_report; ms per call, median of 3.  %s"
        % ("weights of %s" % model_path if model_path else
           "FRESHLY INITIALISED weights: the losses say nothing about the gain on a trained model"))
    for name, make, seq, cols, windows in legs:
        m = make()
        if model_path:
            from bayeslms_amd.compute_sentence_scores import load_partial
            load_partial(m, model_path)
        m = m.to(dev).eval()
        src = batchify(synthetic_corpus(bench.V, cols * (windows * seq + 1), seed=2222), cols, dev)
        n = (src.size(0) - 1) * cols
        say("%s: %d tokens (%d windows of %d x %d), V %d" % (name, n, windows, cols, seq, bench.V))
        theta = 0.01 if "Transformer" in name else 0.3
        base = None
        for leg, fn in (("evaluate_report", lambda: engine.evaluate_report(m, src, seq)),
                        ("evaluate_cache", lambda: engine.evaluate_cache(m, src, seq, 2000, theta, 0.1)),
                        ("fit_cache, passes 3", lambda: engine.fit_cache(m, src, seq, 2000))):
            el, r = timed(fn, 3)
            base = base or el
            extra = ""
            if isinstance(r, engine.CacheFit):
                extra = "  theta %.4g lambda %.4f loss %.4f -> %.4f at_bound %s" % (r.theta, r.lam, r.loss_before, r.loss_after, r.at_bound)
            elif isinstance(r, engine.CacheReport):
                extra = "  loss %.4f -> %.4f hit %.4f" % (r.base_loss, r.loss, r.cache_hit_rate)
            say("  %-22s %9.2f ms  %5.2f evaluate_report calls%s" % (leg, 1e3 * el, el / base, extra))
        del m


if __name__ == "__main__":
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "r16_cache_probe.txt")
    for flag in ("--out", "--model-path"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                path = args[i + 1]
            else:
                model_path = args[i + 1]
            del args[i:i + 2]
    with open(path, "w") as out_file, torch.no_grad():
        for w in (args or ["kernel", "error", "engine"]):
            {"kernel": kernel_legs, "error": error_legs, "engine": engine_legs}[w]()
