#!/usr/bin/env python3
"""blm_row_stats_temps beside blm_row_stats, and engine.fit_temperature beside one engine.evaluate_report.

A. 2048 x 33,000 rows of logits: blm_row_stats (one temperature) beside blm_row_stats_temps with 1, 2, 4 and 8 inverse
   temperatures, every output requested: kernel time by device events over 30 launches of the C entry points on pre-allocated
   outputs, three input buffers in turn so that no launch finds its rows in the Infinity Cache, median of 5, the bytes each must
   move over that time, and the time per temperature.  J = 8 in one launch against eight J = 1 launches says whether the fit
   should hand the kernel eight temperatures at once.
B. The configs[2] Bayesian Transformer (6 x d 512, ff 4096, seq_len 128) on bench._eval_leg's text (12 windows of 20 columns,
   V 33,000), at mean weights and with S = 8: one evaluate_report, one evaluate_temperatures walk of eight temperatures, and
   fit_temperature (three search walks of eight temperatures and the walk that fills before / after).  Each after one warm-up
   call, median of 3, a device synchronise inside the timed window.

usage: temperature_probe.py [--out PATH] [kernel|fit ...]   (default: both; PATH defaults to profiles/r13_temperature_probe.txt)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from bayeslms_amd import engine, model as M, ops  # noqa: E402
from bayeslms_amd.data import batchify, synthetic_corpus  # noqa: E402

dev = torch.device("cuda:0")
EIGHT = [1 / 8, 1 / 4, 1 / 2, 1.0, 1.7, 3.0, 5.0, 8.0]
out_file = None


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
    R, V, NB, N = 2048, 33000, 3, 30
    g = torch.Generator(device=dev).manual_seed(1)
    xs = [3.0 * torch.randn(R, V, device=dev, generator=g) for _ in range(NB)]
    tgt = torch.randint(0, V, (R,), device=dev, generator=g)
    f = [torch.empty(8, R, device=dev) for _ in range(4)]
    i32 = [torch.empty(R, device=dev, dtype=torch.int32) for _ in range(2)]
    c, st = L.calls(), L.stream()
    say("# A. %d x %d rows of logits (%.0f MB), %d buffers in turn; us per launch by device events over %d launches, median of 5"
        % (R, V, R * V * 4 / 1e6, NB, N))

    def temps_leg(J):
        t = ops.row_temps(EIGHT[:J])
        return lambda k: c.blm_row_stats_temps(xs[k].data_ptr(), V, tgt.data_ptr(), R, V, L.C.byref(t), f[0].data_ptr(), f[1].data_ptr(),
                                               f[2].data_ptr(), f[3].data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(), st)
    legs = [("blm_row_stats", 1, lambda k: c.blm_row_stats(xs[k].data_ptr(), V, tgt.data_ptr(), R, V, f[0].data_ptr(), f[1].data_ptr(),
                                                           f[2].data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(), st))]
    legs += [("blm_row_stats_temps J = %d" % J, J, temps_leg(J)) for J in (1, 2, 4, 8)]
    us_of = {}
    for name, J, fn in legs:
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
        us = us_of[name] = statistics.median(times)
        nbytes = R * V * 4
        say("%-28s %8.1f us  %6.2f TB/s of the %d MB it must move  %8.1f us per temperature" % (name, us, nbytes / us / 1e6, nbytes // 10 ** 6, us / J))
    one, eight = us_of["blm_row_stats_temps J = 1"], us_of["blm_row_stats_temps J = 8"]
    say("eight temperatures in one launch: %.1f us against %.1f us of eight J = 1 launches (%.2f of it)" % (eight, 8 * one, eight / (8 * one)))


def fit_legs():
    torch.manual_seed(1111)
    m, seq = M.BayesTransformerModel(bench.V, bench.D_MODEL, bench.NHEAD, bench.D_FF, bench.NLAYERS, bench.DROPOUT, True, "FFN"), 128
    m = m.to(dev).eval()
    src = batchify(synthetic_corpus(bench.V, 20 * (12 * seq + 1), seed=2222), 20, dev)
    n = (src.size(0) - 1) * 20
    say("# B. configs[2] Transformer: %d tokens (12 windows of 20 x %d), V %d; ms per call, median of 3" % (n, seq, bench.V))
    for S in (0, 8):
        legs = (("evaluate_report", lambda: engine.evaluate_report(m, src, seq, mc_samples=S)),
                ("evaluate_temperatures, 8 betas", lambda: engine.evaluate_temperatures(m, src, seq, EIGHT, mc_samples=S)),
                ("fit_temperature, passes 3", lambda: engine.fit_temperature(m, src, seq, mc_samples=S)))
        base = None
        for name, fn in legs:
            el, r = timed(fn, 3)
            base = base or el
            extra = ""
            if isinstance(r, engine.TemperatureFit):
                extra = "  beta %.4f at_bound %s, %d search walks + 1" % (r.beta, r.at_bound, r.passes)
            say("S = %d %-32s %9.2f ms  %5.2f evaluate_report calls%s" % (S, name, 1e3 * el, el / base, extra))


if __name__ == "__main__":
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "r13_temperature_probe.txt")
    if "--out" in args:
        i = args.index("--out")
        path = args[i + 1]
        del args[i:i + 2]
    with open(path, "w") as out_file, torch.no_grad():
        for w in (args or ["kernel", "fit"]):
            kernel_legs() if w == "kernel" else fit_legs()
