#!/usr/bin/env python3
"""What SG-MCMC sampling costs: the update kernel beside its neighbours, the training step with and without a sampler, and
engine.evaluate_samples beside engine.evaluate_swag.

A. blm_sgmcmc_update in its four forms ({sgld, psgld} x {noise, none}) on the flat buffer of the configs[2] Transformer without
   variational sites (48.4 M floats), beside blm_clip_sgd_multi on the same buffers and a one-sample blm_swag_sample at K = 0,
   which does the same noise work per 16 bytes (one Philox block, two Box-Muller pairs) over the same three streams as sgld with
   noise, in the SAME rotation (leg after leg, round after round): kernel time by device events around the call, median of 9
   rounds after one warm-up round; every leg calls its C entry directly, so the window holds the same host work for each.
   Every operand exists twice and the rounds alternate between the two sets (2 x 194 MB per
   stream against a 256 MB Infinity Cache).  Achieved bytes/s = streams x n x 4 bytes over that time, with the streams the
   algorithm needs: sgld reads p, g and writes p: 3; psgld reads p, g, v and writes p, v: 5; blm_clip_sgd_multi 5; the sample
   reads mean, m2 and writes one row: 3.  The number to judge the noise forms by is their bytes/s over the sample kernel's.
B. ms per step of engine.Trainer on the configs[2] shape (batch 64, seq_len 128) without a sampler, with sgld and with psgld at
   temperature 1: one trainer, the three legs alternating in three rounds of 6 steps each after 3 warm-up steps, a device
   synchronise inside each timed window; median over the rounds.
C. tokens/s of engine.evaluate_samples on 8 weight vectors beside engine.evaluate_swag with 8 samples of a posterior over the
   same model, on one synthetic text at (seq_len, columns) = (35, 10): alternating, median of 3 after one warm-up call each.

The weights are freshly initialised and the gradients synthetic: the runs time the code and say NOTHING about the perplexity or
calibration a sampled model gains.

usage: sgmcmc_probe.py [--out PATH] [kernel|step|engine ...]      (default: all three; PATH defaults to
       profiles/r23_sgmcmc_probe.txt)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from bayeslms_amd import _lib as L, engine, model as M, ops, sgmcmc, swag  # noqa: E402
from bayeslms_amd.data import batchify, get_batch, synthetic_corpus  # noqa: E402

dev = torch.device("cuda:0")
out_file = None
SEED = 1111


def say(*a):
    print(*a, flush=True)
    if out_file is not None:
        print(*a, file=out_file, flush=True)


def plain_model():
    torch.manual_seed(SEED)
    return M.TransformerModel(bench.V, bench.D_MODEL, bench.NHEAD, bench.D_FF, bench.NLAYERS, 0.2, "gelu", True).to(dev)


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def kernel_legs():
    c = L.calls()
    n = swag.flat_layout(plain_model())[2]
    gen = torch.Generator(device=dev).manual_seed(7)
    rand = lambda scale=1.0: torch.randn(n, device=dev, generator=gen) * scale  # noqa: E731
    sets = [dict(p=rand(), g=rand(1e-3), v=rand(1e-3).abs_(), mom=rand(1e-3), mean=rand(), m2=rand().abs_(), out=torch.empty(1, n, device=dev))
            for _ in range(2)]
    for s in sets:
        s["table"] = ops.PtrTable([s["p"]], [s["g"]], [s["mom"]])
        s["table"].sq.fill_(1.0)
    st = L.stream()

    # every leg calls its C entry directly with operands prepared here, so the event window holds the same host work for all
    import ctypes as C
    draws = [ops.swag_draw([r], SEED, 0.7, 0.0, 0.25, 1e-30) for r in range(10)]
    rngs = [L.rng(SEED, L.STREAM_SGMCMC, r) for r in range(10)]

    def update(rnd, rule, sigma):
        s = sets[rnd & 1]
        c.blm_sgmcmc_update(L.ptr(s["p"]), L.ptr(s["g"]), L.ptr(s["v"]) if rule == "psgld" else None, L.ptr(s["table"].sq), n, 1.0, 0.002,
                            1.0, 1e-6, sigma, 0.99, 1e-5, C.byref(rngs[rnd]), st)

    def clip(rnd):
        t = sets[rnd & 1]["table"]
        c.blm_clip_sgd_multi(L.ptr(t.params), L.ptr(t.grads), L.ptr(t.bufs), L.ptr(t.sizes), 1, L.ptr(t.sq), 1.0, 0.002, 0.9, 0, 1.0, st)

    def sample(rnd):
        s = sets[rnd & 1]
        c.blm_swag_sample(L.ptr(s["out"]), n, L.ptr(s["mean"]), L.ptr(s["m2"]), None, 0, 0, None, n, C.byref(draws[rnd]), st)

    legs = [("blm_sgmcmc_update sgld, noise", 3, lambda r: update(r, "sgld", 1e-3)),
            ("blm_sgmcmc_update sgld, none", 3, lambda r: update(r, "sgld", 0.0)),
            ("blm_sgmcmc_update psgld, noise", 5, lambda r: update(r, "psgld", 1e-3)),
            ("blm_sgmcmc_update psgld, none", 5, lambda r: update(r, "psgld", 0.0)),
            ("blm_clip_sgd_multi", 5, clip),
            ("blm_swag_sample K = 0, J = 1", 3, sample)]
    say("# A. the flat buffer of the configs[2] Transformer: n = %d floats (%.1f MB per buffer); us per call by device events, median "
        "of 9 rounds, every leg in every round, operands alternating between two sets; GB/s = streams x n x 4 / time" % (n, n * 4 / 1e6))
    times = {k: [] for k, _, _ in legs}
    for rnd in range(10):
        for k, _, fn in legs:
            us = event_us(lambda: fn(rnd))
            if rnd:
                times[k].append(us)
    rate = {}
    for k, streams, _ in legs:
        med = statistics.median(times[k])
        rate[k] = streams * n * 4 / (med * 1e-6) / 1e9
        say("  %-34s %9.1f us  %d streams  %7.1f GB/s  (min %.1f max %.1f us)" % (k, med, streams, rate[k], min(times[k]), max(times[k])))
    ref = rate["blm_swag_sample K = 0, J = 1"]
    say("  bytes/s over the one-sample blm_swag_sample's: sgld with noise %.3f, psgld with noise %.3f; sgld without %.3f, psgld "
        "without %.3f, blm_clip_sgd_multi %.3f" % tuple(rate[k] / ref for k, _, _ in legs[:5]))


def step_legs():
    seq, cols, warm, per, rounds = bench.T, bench.B_PER_GPU, 3, 6, 3
    m = plain_model()
    stream = synthetic_corpus(bench.V, cols * ((warm + 3 * per * rounds) * seq + 1) + 17, seed=SEED)
    train = batchify(stream, cols, dev)
    tr = engine.Trainer(m, lr=bench.LR, clip=bench.CLIP, seed=SEED)
    n_tokens = (train.size(0) - 1) * cols
    samplers = {"no sampler (clip + SGD)": None,
                "sgld, temperature 1": sgmcmc.Sampler("sgld", 0.01, n_tokens, seed=SEED),
                "psgld, temperature 1": sgmcmc.Sampler("psgld", 1e-4, n_tokens, seed=SEED)}
    i = 0

    def steps(k):
        nonlocal i
        for _ in range(k):
            data, tgt = get_batch(train, i * seq, seq)
            tr.step(data, tgt)
            i += 1

    steps(warm)
    times = {k: [] for k in samplers}
    for _ in range(rounds):
        for k, s in samplers.items():
            tr.set_sampler(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(per)
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0) / per)
    say("# B. engine.Trainer on the configs[2] shape without variational sites, batch %d x seq_len %d, %d floats of weights: ms per "
        "step, median of %d rounds of %d steps, the legs alternating (freshly initialised weights, synthetic text)"
        % (cols, seq, tr.flat.total, rounds, per))
    base = statistics.median(times["no sampler (clip + SGD)"])
    for k in samplers:
        med = statistics.median(times[k])
        say("  %-28s %8.3f ms per step  (%+.3f ms, %.4f x; rounds %s)" % (k, med, med - base, med / base, " ".join("%.3f" % t for t in times[k])))


def timed_alternating(fns, reps=3):
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    res = {}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            res[k] = fn()
            torch.cuda.synchronize()
            out[k].append(time.perf_counter() - t0)
    return {k: statistics.median(v) for k, v in out.items()}, res


def engine_legs():
    S, seq, cols, windows = 8, 35, 10, 24
    m = plain_model().eval()
    total = swag.flat_layout(m)[2]
    vec = sgmcmc.flat_of(m).to(dev)
    post = swag.SwagPosterior(total, 20, dev, swag.manifest_of(m))
    gen = torch.Generator(device=dev).manual_seed(3)
    for _ in range(4):
        post.collect(vec * (1 + 0.01 * torch.randn(total, device=dev, generator=gen)))
    mat = post.draw(S, SEED)  # eight vectors on the device: what evaluate_swag draws for itself
    bank = sgmcmc.SampleBank(total, swag.manifest_of(m), S)
    for s in range(S):
        bank.add(mat[s], {"kind": "sgld"})
    src = batchify(synthetic_corpus(bench.V, cols * (windows * seq + 1), seed=2222), cols, dev)
    n = (src.size(0) - 1) * cols
    t, r = timed_alternating({"swag": lambda: engine.evaluate_swag(m, src, seq, post, S, seed=SEED),
                              "matrix": lambda: engine.evaluate_samples(m, src, seq, mat),
                              "bank": lambda: engine.evaluate_samples(m, src, seq, bank)})
    say("# C. %d weight vectors over %d floats, seq_len %d x %d columns, %d windows, %d tokens; tokens/s, median of 3 calls, the legs "
        "alternating.  FRESHLY INITIALISED weights and vectors drawn around them: these runs time the code and say nothing about the "
        "perplexity or calibration a sampled model gains" % (S, total, seq, cols, windows, n))
    say("  evaluate_swag, %d samples (draws them)              %9.0f tokens/s (%.1f ms)" % (S, n / t["swag"], 1e3 * t["swag"]))
    say("  evaluate_samples, (%d, P) matrix on the device      %9.0f tokens/s (%.1f ms), %.3f x evaluate_swag's time"
        % (S, n / t["matrix"], 1e3 * t["matrix"], t["matrix"] / t["swag"]))
    say("  evaluate_samples, SampleBank on the host (%.2f GB)  %9.0f tokens/s (%.1f ms), %.3f x evaluate_swag's time"
        % (4e-9 * S * total, n / t["bank"], 1e3 * t["bank"], t["bank"] / t["swag"]))
    say("  loss: swag %.4f, matrix %.4f (the same draws: %s), bank %.4f" % (r["swag"].loss, r["matrix"].loss,
                                                                           "equal" if r["swag"].loss == r["matrix"].loss else "DIFFERENT", r["bank"].loss))


if __name__ == "__main__":
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "r23_sgmcmc_probe.txt")
    if "--out" in args:
        i = args.index("--out")
        path = args[i + 1]
        del args[i:i + 2]
    with open(path, "w") as out_file:
        for w in (args or ["kernel", "step", "engine"]):
            {"kernel": kernel_legs, "step": step_legs, "engine": engine_legs}[w]()
