#!/usr/bin/env python3
"""Local reparameterisation (NoiseState.local_reparam) against the weight-sampling estimator, two measurements:

1. the headline configuration's training step (bench.py's model and step: 6 layers, d_model 512, d_ff 4096, V 33000, T 128,
   B 64) with the flag off and on -- one process, one model, the sides alternated, three rounds of `--steps` steps each
   after a warm-up of both; median of the three per side with the spread (min .. max);
2. the variance of the weight-mean gradient dmu under each estimator at M 256, K 32, N 16 over 200 seeds (fixed x, mu,
   lgstd and target, loss = |y - target|^2 / (2 M); per-element variance over the seeds, averaged over the elements) and the ratio.

    python tools/lrt_probe.py [--steps 10]            -> profiles/r09_lrt_probe.txt
"""
import argparse
import statistics
import sys
import time

sys.path.insert(0, ".")
import torch  # noqa: E402

import bench  # noqa: E402
from bayeslms_amd import engine, model as M, ops  # noqa: E402
from bayeslms_amd.data import batchify, get_batch, synthetic_corpus  # noqa: E402


def step_times(dev, steps, warm=4, rounds=3):
    T, B, V = bench.T, bench.B_PER_GPU, bench.V
    torch.manual_seed(1111)
    m = M.BayesTransformerModel(V, bench.D_MODEL, bench.NHEAD, bench.D_FF, bench.NLAYERS, bench.DROPOUT, True, "FFN").to(dev)
    kl = lambda mm: mm.transformerlayers[0].linear2.kl_divergence()  # noqa: E731
    kl.fusable = True
    n_steps = 2 * (warm + rounds * steps)
    train = batchify(synthetic_corpus(V, B * (n_steps * T + 1) + 17, seed=1111), B, dev)
    tr = engine.Trainer(m, lr=bench.LR, clip=bench.CLIP, kl_scale=float(T) / train.size(0), seed=1111)
    pos = [0]

    def run(flag, n):
        m.set_local_reparam(flag)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            data, tgt = get_batch(train, pos[0], T)
            pos[0] += T
            loss = tr.step(data, tgt, kl_fn=kl)[0]
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, float(loss)
    for flag in (False, True):
        run(flag, warm)
    ms = {False: [], True: []}
    for _ in range(rounds):
        for flag in (False, True):
            t, loss = run(flag, steps)
            ms[flag].append(t)
    for flag in (False, True):
        v = ms[flag]
        print("training step, headline shape (T %d, B %d), local_reparam %-3s: median %.3f ms  (min %.3f .. max %.3f, %d rounds of %d steps)"
              % (T, B, "on" if flag else "off", statistics.median(v), min(v), max(v), rounds, steps), flush=True)
    print("on / off (medians): %.4f   last loss %.4f" % (statistics.median(ms[True]) / statistics.median(ms[False]), loss), flush=True)


def gradient_variance(dev, M_=256, K=32, N=16, seeds=200):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M_, K, generator=g).to(dev)
    mu0 = (0.3 * torch.randn(N, K, generator=g)).to(dev)
    lg0 = (-1.0 + 0.3 * torch.randn(N, K, generator=g)).to(dev)
    tgt = torch.randn(M_, N, generator=g).to(dev)
    grads = {"weight sample": [], "local reparam": []}
    for s in range(seeds):
        for name in grads:
            mu, lg = mu0.clone().requires_grad_(True), lg0.clone().requires_grad_(True)
            if name == "weight sample":
                y = ops.bayes_linear(x, mu, lg, ops.NoiseSpec(None, 1000 + s, 1, 0))
            else:
                y = ops.bayes_linear_lrt(x, mu, lg, ops.LrtNoise(None, 1000 + s, 1, 0))
            (0.5 * ((y - tgt) ** 2).sum() / M_).backward()
            grads[name].append(torch.cat([mu.grad.reshape(-1), lg.grad.reshape(-1)]).double())
    out = {}
    for name, gs in grads.items():
        var = torch.stack(gs).var(0, unbiased=True)
        out[name] = (float(var[:N * K].mean()), float(var[N * K:].mean()))
        print("gradient variance over %d seeds, M %d K %d N %d, %-13s: dmu %.6e   dlgstd %.6e" % (seeds, M_, K, N, name, *out[name]), flush=True)
    a, b = out["weight sample"], out["local reparam"]
    print("variance ratio weight sample / local reparam: dmu %.2f   dlgstd %.2f" % (a[0] / b[0], a[1] / b[1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gradient_variance(dev)
    if not a.skip_step:
        step_times(dev, a.steps)


if __name__ == "__main__":
    main()
