#!/usr/bin/env python3
"""Incremental decoding (bayeslms_amd/incremental.py) against recomputing the next-word distribution with the full forward.

    python tools/decode_probe.py [--out profiles/r06_decode_probe.txt] [--quick]

1. decode steps/s and tokens/s of IncrementalLM.step (one word per stream per step) for the configs[2] Transformer (Bayesian FFN,
   6 x 512, 8 heads, d_ff 4096) and the configs[1] LSTM (Bayesian pos 3, 2 x 1024), vocabulary 33,000, at 1 / 8 / 64 streams and
   contexts 16 / 128 / 512 / 1024 (the context is filled by one prompt chunk, then STEPS single-word steps are timed; the context
   grows by STEPS during them);
2. the time of today's alternative: the full forward over the (context, streams) prefix, whose last row is the same distribution;
3. blm_attn_decode on its own at 64 streams x 1024 cached tokens, 8 heads of 64: K/V bytes read per launch over its time.

Times are HIP events around back-to-back launches on the current stream (median of REPS repetitions); the host time of a step
is reported next to its GPU time, so a step bound by launches or Python shows as host ms >= GPU ms."""
import argparse
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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    L.require_gfx950()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
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
