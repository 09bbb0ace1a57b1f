#!/usr/bin/env python3
"""Incremental decoding (bayeslms_amd/incremental.py) against recomputing the next-word distribution with the full forward.

    python tools/decode_probe.py [--out profiles/r06_decode_probe.txt] [--quick]
    python tools/decode_probe.py --mc-samples [--out profiles/r06_decode_mc_probe.txt]

1. decode steps/s and tokens/s of IncrementalLM.step (one word per stream per step) for the configs[2] Transformer (Bayesian FFN,
   6 x 512, 8 heads, d_ff 4096) and the configs[1] LSTM (Bayesian pos 3, 2 x 1024), vocabulary 33,000, at 1 / 8 / 64 streams and
   contexts 16 / 128 / 512 / 1024 (the context is filled by one prompt chunk, then STEPS single-word steps are timed; the context
   grows by STEPS during them);
2. the time of today's alternative: the full forward over the (context, streams) prefix, whose last row is the same distribution;
3. blm_attn_decode on its own at 64 streams x 1024 cached tokens, 8 heads of 64: K/V bytes read per launch over its time.

--mc-samples measures Monte-Carlo weight samples on the same path instead (IncrementalLM(mc_samples=S)):
A. steps/s of both models at S 2 / 4 / 8, 1 / 8 / 64 streams, context 128, beside S x the mean-weight step of the same run (what
   S passes one after the other would cost if nothing were shared) and the host time per step;
B. blm_linear_mc_logprobs alone (ops.linear_mc_logprobs: both decoder products and the fold) at N x Sp rows, V 33,000, K 512 and
   1024, against the composed path it replaces: ops.linear over the S x N rows, ops.log_softmax_rows, torch.logsumexp over S.

Times are HIP events around back-to-back launches on the current stream (median of REPS repetitions); the host time of a step
is reported next to its GPU time, so a step bound by launches or Python shows as host ms >= GPU ms."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayeslms_amd import _lib as L  # noqa: E402
from bayeslms_amd import model as M  # noqa: E402
from bayeslms_amd.incremental import IncrementalLM  # noqa: E402

V = 33000
STEPS, REPS = 16, 3


def _events(fn, reps):
    """median GPU ms and host ms of fn()"""
    gpu, host = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        gpu.append(a.elapsed_time(b))
        host.append((t1 - t0) * 1e3)
    return statistics.median(gpu), statistics.median(host)


def build(kind, dev):
    torch.manual_seed(0)
    if kind == "tlm":
        m = M.BayesTransformerModel(V, 512, 8, 4096, 6, 0.1, True, "FFN")
    else:
        m = M.BayesRNNModel("LSTM", V, 1024, 1024, 2, 0.5, True, 3)
    return m.to(dev).eval()


def decode_vs_recompute(kind, m, n, ctx, dev, say):
    lm = IncrementalLM(m, max_streams=64, max_len=ctx + STEPS + 1)
    ids = torch.randint(0, V, (ctx + STEPS, n), device=dev)
    with torch.no_grad():
        dec = []
        for _ in range(REPS):
            st = lm.start(n)
            lm.step(st, ids[:ctx])
            dec.append(_events(lambda: [lm.step(st, ids[ctx + t]) for t in range(STEPS)], 1))
        g_ms = statistics.median(d[0] for d in dec) / STEPS
        h_ms = statistics.median(d[1] for d in dec) / STEPS
        if kind == "tlm":
            rec = _events(lambda: m(ids[:ctx]), REPS)[0]
        else:
            rec = _events(lambda: m(ids[:ctx], m.init_hidden(n)), REPS)[0]
    say("%-4s n=%-3d ctx=%-5d step %8.3f ms (host %7.3f ms)  %9.1f steps/s %10.0f tok/s | recompute %9.3f ms  speedup %7.1fx"
        % (kind, n, ctx, g_ms, h_ms, 1e3 / g_ms, n * 1e3 / g_ms, rec, rec / g_ms))
    return g_ms, rec


def mc_decode(kind, m, n, ctx, dev, say):
    """A: one word per stream per step at S samples, beside S x the mean-weight step measured in the same process"""
    ids = torch.randint(0, V, (ctx + STEPS, n), device=dev)

    def timed(lm):
        runs = []
        for _ in range(REPS):
            st = lm.start(n)
            lm.step(st, ids[:ctx])
            runs.append(_events(lambda: [lm.step(st, ids[ctx + t]) for t in range(STEPS)], 1))
        return statistics.median(r[0] for r in runs) / STEPS, statistics.median(r[1] for r in runs) / STEPS
    with torch.no_grad():
        g0, h0 = timed(IncrementalLM(m, max_streams=64, max_len=ctx + STEPS + 1))
        say("%-4s n=%-3d ctx=%-4d mean weights     step %8.3f ms (host %7.3f ms) %9.1f steps/s" % (kind, n, ctx, g0, h0, 1e3 / g0))
        for S in (2, 4, 8):
            g, h = timed(IncrementalLM(m, max_streams=64, max_len=ctx + STEPS + 1, mc_samples=S))
            say("%-4s n=%-3d ctx=%-4d mc_samples=%-2d     step %8.3f ms (host %7.3f ms) %9.1f steps/s | S x mean-weight step %8.3f ms"
                "  ratio %.2f" % (kind, n, ctx, S, g, h, 1e3 / g, S * g0, g / (S * g0)))


def mc_kernel(dev, say):
    """B: the fused launch against the composed path built from ops.linear / ops.log_softmax_rows / torch.logsumexp"""
    from bayeslms_amd import ops
    from bayeslms_amd.incremental import _MC_FUSED_MAX_ROWS_K
    verdict = []
    for K in (512, 1024):
        w = torch.randn(V, K, device=dev) * (4.0 / K ** 0.5)
        b = torch.randn(V, device=dev)
        dec = ops.McDecoder(w, b)
        for n in (1, 8, 64):
            for S in (2, 4, 8):
                x = torch.randn(S, n, K, device=dev)

                def fused():
                    for _ in range(10):
                        ops.linear_mc_logprobs(x, w, b, dec=dec, stats=False)

                def fused_stats():
                    for _ in range(10):
                        ops.linear_mc_logprobs(x, w, b, dec=dec, stats=True)

                def composed():
                    for _ in range(10):
                        lp = ops.log_softmax_rows(ops.linear(x.reshape(S * n, K), w, b), V)
                        torch.logsumexp(lp.view(S, n, V), 0).sub_(math.log(S))
                with torch.no_grad():
                    a = ops.linear_mc_logprobs(x, w, b, dec=dec, stats=False).logp
                    lp = ops.log_softmax_rows(ops.linear(x.reshape(S * n, K), w, b), V)
                    c = torch.logsumexp(lp.view(S, n, V), 0) - math.log(S)
                    err = float((a - c).abs().max())
                    for f in (fused, fused_stats, composed):
                        f()
                    tf, tfs, tc = (_events(f, 5) for f in (fused, fused_stats, composed))
                say("K=%-4d n=%-3d S=%d (%4d rows): fused %7.1f us (host %7.1f)  with h_pred / mi %7.1f us | composed %7.1f us (host %7.1f)"
                    "  composed / fused %.2f   max |fused - composed| %.1e"
                    % (K, n, S, n * (1 << (S - 1).bit_length()), tf[0] * 100, tf[1] * 100, tfs[0] * 100, tc[0] * 100, tc[1] * 100,
                       tc[0] / tf[0], err))
                if n == 64 and S == 8:
                    verdict.append("K %d: composed / fused %.2f -> IncrementalLM runs the %s path there" % (
                        K, tc[0] / tf[0], "fused" if n * S * K <= _MC_FUSED_MAX_ROWS_K else "composed"))
    say("# 64 streams x S 8 (512 rows): " + "; ".join(verdict) + " (incremental._MC_FUSED_MAX_ROWS_K = %d rows x K: the fused launch "
        "runs the decoder product twice, the composed path once plus S x rows x V floats through memory; with return_uncertainty "
        "the fused launch always runs)" % _MC_FUSED_MAX_ROWS_K)


def attn_bandwidth(dev, say, n=64, ctx=1024, nhead=8, hd=64):
    lib = L.lib()
    kv = torch.randn(2, n, nhead, ctx, hd, device=dev)
    q = torch.randn(1, n, 3 * nhead * hd, device=dev)
    past = torch.full((n,), ctx - 1, dtype=torch.int32, device=dev)
    out = torch.empty(1, n, nhead * hd, device=dev)
    nws = lib.blm_attn_decode_ws_floats(1, n, nhead, ctx, hd)
    ws = torch.empty(nws, device=dev)

    def once():
        for _ in range(20):
            L.check(lib.blm_attn_decode(q.data_ptr(), 3 * nhead * hd, kv.data_ptr(), past.data_ptr(), None, out.data_ptr(), ws.data_ptr(),
                                        nws, 1, n, n, nhead, ctx, hd, ctx, L.stream()), "blm_attn_decode")
    once()
    ms = _events(once, 5)[0] / 20
    kv_bytes = 2 * n * nhead * ctx * hd * 4
    say("blm_attn_decode n=%d ctx=%d nhead=%d hd=%d: %.1f us per call (split-K + combine), K/V %.1f MB -> %.2f TB/s"
        % (n, ctx, nhead, hd, ms * 1e3, kv_bytes / 1e6, kv_bytes / (ms * 1e-3) / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r06_decode_probe.txt")
    ap.add_argument("--quick", action="store_true", help="64 streams x 1024 context of the Transformer only (profiling runs)")
    ap.add_argument("--mc-samples", action="store_true",
                    help="Monte-Carlo weight samples: sections A and B of the docstring (default --out profiles/r06_decode_mc_probe.txt)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L.require_gfx950()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if args.mc_samples:
        out = args.out if args.out != ap.get_default("out") else "profiles/r06_decode_mc_probe.txt"
        say("# tools/decode_probe.py --mc-samples: V %d, %d timed steps, median of %d" % (V, STEPS, REPS))
        say("# A. IncrementalLM(mc_samples=S).step, one word per stream, context 128 (GPU ms per step, HIP events)")
        for kind in ("tlm", "lstm"):
            m = build(kind, dev)
            for n in (1, 8, 64):
                mc_decode(kind, m, n, 128, dev, say)
            del m
            torch.cuda.empty_cache()
        say("# B. blm_linear_mc_logprobs (pass 1 + pass 2, logp only) against ops.linear + ops.log_softmax_rows + torch.logsumexp, "
            "10 calls per timing, median of 5")
        mc_kernel(dev, say)
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    say("# tools/decode_probe.py: IncrementalLM.step vs full-forward recompute, V %d, %d timed steps, median of %d" % (V, STEPS, REPS))
    attn_bandwidth(dev, say)
    for kind in (("tlm",) if args.quick else ("tlm", "lstm")):
        m = build(kind, dev)
        for n in ((64,) if args.quick else (1, 8, 64)):
            for ctx in ((1024,) if args.quick else (16, 128, 512, 1024)):
                decode_vs_recompute(kind, m, n, ctx, dev, say)
        del m
        torch.cuda.empty_cache()
    if not args.quick and args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
