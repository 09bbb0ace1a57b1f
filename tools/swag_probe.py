#!/usr/bin/env python3
"""What SWAG costs: the three kernels beside their neighbours, and engine.evaluate_swag beside the reports it stands next to.

A. blm_swag_collect and blm_swag_sample on the flat buffer of the configs[2] Transformer (the shape without variational sites: 48.4 M floats) at K = 0 / 20 and
   J = 1 / 8, beside blm_dyneval_update (sgd rule, zero_grad) and blm_clip_sgd_multi in the SAME rotation (leg after leg, round
   after round): kernel time by device events around the call, median of 9 rounds after one warm-up round.  Every small operand
   (theta, mean, m2, p, g, p0, momentum) exists twice and the rounds alternate between the two sets, and the K deviation rows
   (4 GB at K = 20) and the J output rows are far larger than the 256 MB Infinity Cache, so no launch finds its input there.
   Achieved bytes/s = streams x n x 4 bytes over that time, with the streams the algorithm needs: collect reads theta, mean, m2
   and writes mean, m2 (and the deviation row): 5 / 6; sample reads mean, m2 and K rows and writes J rows: 2 + K + J; the
   update 5; blm_clip_sgd_multi 5.  Eight J = 1 launches are timed as one leg beside the one J = 8 launch.
B. blm_logp_avg_accum on 2048 x 33,000 logits (s = 0: one read, one write; s = 1 of 2: two reads, one write) beside
   blm_log_softmax_rows (one read, one write) and blm_row_stats (one read) on the same rows; three sets of matrices in rotation.
C. tokens/s of engine.evaluate_swag with 8 samples beside 8 x engine.evaluate_report at mean weights (the same TransformerModel)
   and beside engine.evaluate_report(mc_samples=8) on a Bayesian model of the same shape, on one synthetic text at
   (seq_len, columns) = (35, 10): each after one warm-up call, median of 3, a device synchronise inside the timed window.

The weights are freshly initialised unless ``--model-path`` loads trained ones, and the posterior is four perturbed copies of
them: the runs time the code and say NOTHING about the perplexity or calibration a trained model gains.

usage: swag_probe.py [--out PATH] [--model-path PATH] [kernel|rows|engine ...]
       (default: all three; PATH defaults to profiles/r19_swag_probe.txt)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from bayeslms_amd import _lib as L, engine, model as M, ops, swag  # noqa: E402
from bayeslms_amd.data import batchify, synthetic_corpus  # noqa: E402

dev = torch.device("cuda:0")
out_file = None
model_path = None
SEED = 1111


def say(*a):
    print(*a, flush=True)
    if out_file is not None:
        print(*a, file=out_file, flush=True)


def plain_model():
    torch.manual_seed(SEED)
    m = M.TransformerModel(bench.V, bench.D_MODEL, bench.NHEAD, bench.D_FF, bench.NLAYERS, 0.2, "gelu", True)
    if model_path:
        from bayeslms_amd.compute_sentence_scores import load_partial
        load_partial(m, model_path)
    return m.to(dev).eval()


def event_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def rotation(legs, rounds=10):
    """legs: (name, streams or None, fn(round)) -> {name: [us per round after the first]}"""
    times = {k: [] for k, _, _ in legs}
    for rnd in range(rounds):
        for k, _, fn in legs:
            us = event_us(lambda: fn(rnd))
            if rnd:
                times[k].append(us)
    return times


def kernel_legs():
    c = L.calls()
    n = swag.flat_layout(plain_model())[2]
    K, J = 20, 8
    gen = torch.Generator(device=dev).manual_seed(7)
    rand = lambda scale=1.0: torch.randn(n, device=dev, generator=gen) * scale  # noqa: E731
    sets = [dict(theta=rand(), mean=rand(), m2=rand().abs_(), p=rand(), g=rand(1e-3), p0=rand(), mom=rand(1e-3)) for _ in range(2)]
    for s in sets:
        s["table"] = ops.PtrTable([s["p"]], [s["g"]], [s["mom"]])
        s["table"].sq.fill_(1.0)
    devs = torch.randn(K, n, device=dev, generator=gen) * 0.1
    out = torch.empty(J, n, device=dev)
    a, b, _ = swag.coefficients(0.5, K)
    ad, _, _ = swag.coefficients(0.5, 0)
    z2 = ops.swag_z2(list(range(J)), SEED, K, dev)
    st = L.stream()

    def sample(rnd, k, ids):
        s = sets[rnd & 1]
        ops.swag_sample(out[:len(ids)], s["mean"], s["m2"], ids, SEED, a if k else ad, b if k else 0.0, 0.25, 1e-30,
                        dev=devs if k else None, k_live=k, z2=z2[:len(ids)] if k else None)

    def eight_singles(rnd, k):
        for j in range(J):
            s = sets[rnd & 1]
            ops.swag_sample(out[j:j + 1], s["mean"], s["m2"], [j], SEED, a if k else ad, b if k else 0.0, 0.25, 1e-30,
                            dev=devs if k else None, k_live=k, z2=z2[j:j + 1] if k else None)

    def clip(rnd):
        t = sets[rnd & 1]["table"]
        c.blm_clip_sgd_multi(L.ptr(t.params), L.ptr(t.grads), L.ptr(t.bufs), L.ptr(t.sizes), 1, L.ptr(t.sq), 1.0, 0.002, 0.9, 0, 1.0, st)

    legs = [("blm_swag_collect K = 0", 5, lambda r: ops.swag_collect(sets[r & 1]["theta"], sets[r & 1]["mean"], sets[r & 1]["m2"], 3)),
            ("blm_swag_collect K > 0", 6, lambda r: ops.swag_collect(sets[r & 1]["theta"], sets[r & 1]["mean"], sets[r & 1]["m2"], 3, devs[r % K])),
            ("blm_swag_sample K = 0, J = 1", 3, lambda r: sample(r, 0, [0])),
            ("blm_swag_sample K = 0, J = 8", 2 + J, lambda r: sample(r, 0, list(range(J)))),
            ("blm_swag_sample K = 20, J = 1", 2 + K + 1, lambda r: sample(r, K, [0])),
            ("blm_swag_sample K = 20, J = 8", 2 + K + J, lambda r: sample(r, K, list(range(J)))),
            ("8 launches K = 0, J = 1", 8 * 3, lambda r: eight_singles(r, 0)),
            ("8 launches K = 20, J = 1", 8 * (2 + K + 1), lambda r: eight_singles(r, K)),
            ("blm_dyneval_update sgd, zero_grad", 5, lambda r: ops.dyneval_update(sets[r & 1]["p"], sets[r & 1]["g"], sets[r & 1]["p0"], 0.002, 0.02)),
            ("blm_clip_sgd_multi alone", 5, clip)]
    say("# A. the flat buffer of the configs[2] Transformer: n = %d floats (%.1f MB per buffer); us per call by device events, median "
        "of 9 rounds, every leg in every round, small operands alternating between two sets; GB/s = streams x n x 4 / time" % (n, n * 4 / 1e6))
    times = rotation(legs)
    med, rate = {}, {}
    for k, streams, _ in legs:
        med[k] = statistics.median(times[k])
        rate[k] = streams * n * 4 / (med[k] * 1e-6) / 1e9
        say("  %-34s %9.1f us  %3d streams  %7.1f GB/s  (min %.1f max %.1f us)" % (k, med[k], streams, rate[k], min(times[k]), max(times[k])))
    say("  bytes/s of blm_swag_sample K = 20, J = 8 over blm_dyneval_update's: %.3f; collect K > 0 over it: "
        "%.3f" % (rate["blm_swag_sample K = 20, J = 8"] / rate["blm_dyneval_update sgd, zero_grad"],
                                         rate["blm_swag_collect K > 0"] / rate["blm_dyneval_update sgd, zero_grad"]))
    for k in (0, K):
        one, eight = med["blm_swag_sample K = %d, J = 8" % k], med["8 launches K = %d, J = 1" % k]
        say("  K = %2d: one J = 8 launch %.1f us, eight J = 1 launches %.1f us: %.2f of their time (bytes: %.2f)"
            % (k, one, eight, one / eight, (2 + k + J) / (8.0 * (2 + k + 1))))


def rows_legs():
    R, V = 2048, bench.V
    gen = torch.Generator(device=dev).manual_seed(9)
    sets = [dict(z=torch.randn(R, V, device=dev, generator=gen) * 3, acc=torch.empty(R, V, device=dev), out=torch.empty(R, V, device=dev))
            for _ in range(3)]
    tg = torch.randint(0, V, (R,), device=dev, generator=gen)
    hsum, nll_s = torch.empty(R, device=dev), torch.empty(2, R, device=dev)
    for s in sets:
        ops.logp_avg_accum(s["z"], s["acc"], 0, 2, tg, hsum, nll_s)
    legs = [("blm_logp_avg_accum s = 0", 2, lambda r: ops.logp_avg_accum(sets[r % 3]["z"], sets[r % 3]["out"], 0, 2, tg, hsum, nll_s)),
            ("blm_logp_avg_accum s = 1 of 2", 3, lambda r: ops.logp_avg_accum(sets[r % 3]["z"], sets[r % 3]["acc"], 1, 2, tg, hsum, nll_s)),
            ("blm_log_softmax_rows", 2, lambda r: ops.log_softmax_rows(sets[r % 3]["z"], out=sets[r % 3]["out"])),
            ("blm_row_stats", 1, lambda r: ops.row_stats(sets[r % 3]["z"], tg))]
    say("# B. %d x %d rows (%.1f MB per matrix), three sets in rotation; us per call, median of 9 rounds; GB/s = matrices moved x "
        "bytes / time" % (R, V, R * V * 4 / 1e6))
    times = rotation(legs)
    for k, streams, _ in legs:
        us = statistics.median(times[k])
        say("  %-34s %9.1f us  %d matrices  %7.1f GB/s  (min %.1f max %.1f us)"
            % (k, us, streams, streams * R * V * 4 / (us * 1e-6) / 1e9, min(times[k]), max(times[k])))


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
    S, seq, cols, windows = 8, 35, 10, 24
    say("# C. evaluate_swag with %d samples beside its neighbours, tokens/s, median of 3 calls.  %s"
        % (S, "weights of %s" % model_path if model_path else
           "FRESHLY INITIALISED weights and a posterior of four perturbed copies: these runs time the code and say nothing about the "
           "perplexity or calibration a trained model gains"))
    m = plain_model()
    post = swag.SwagPosterior(swag.flat_layout(m)[2], 20, dev, swag.manifest_of(m))
    params, offsets, total = swag.flat_layout(m)
    vec = torch.zeros(total, device=dev)
    for p, o in zip(params, offsets):
        vec[o:o + p.numel()] = p.detach().reshape(-1)
    gen = torch.Generator(device=dev).manual_seed(3)
    for _ in range(4):
        post.collect(vec * (1 + 0.01 * torch.randn(total, device=dev, generator=gen)))
    src = batchify(synthetic_corpus(bench.V, cols * (windows * seq + 1), seed=2222), cols, dev)
    n = (src.size(0) - 1) * cols
    t_draw, _ = timed(lambda: post.draw(S, SEED))
    t_swag, rs = timed(lambda: engine.evaluate_swag(m, src, seq, post, S, seed=SEED))
    with torch.no_grad():
        t_rep, rep = timed(lambda: engine.evaluate_report(m, src, seq))
    torch.manual_seed(SEED)
    mb = M.BayesTransformerModel(bench.V, bench.D_MODEL, bench.NHEAD, bench.D_FF, bench.NLAYERS, 0.2, True, "FFN").to(dev).eval()
    with torch.no_grad():
        t_mc, mc = timed(lambda: engine.evaluate_report(mb, src, seq, mc_samples=S, seed=SEED))
    say("configs[2] shape, seq_len %d x %d columns, %d windows, %d tokens, posterior n %d rank %d over %d floats:" % (
        seq, cols, windows, n, post.n, post.rank, post.total))
    say("  evaluate_swag, %d samples          %9.0f tokens/s (%.1f ms; drawing the %d samples alone: %.1f ms)" % (S, n / t_swag, 1e3 * t_swag, S, 1e3 * t_draw))
    say("  evaluate_report, mean weights     %9.0f tokens/s (%.1f ms); %d of them: %.1f ms, evaluate_swag is %.2f x that"
        % (n / t_rep, 1e3 * t_rep, S, 1e3 * S * t_rep, t_swag / (S * t_rep)))
    say("  evaluate_report(mc_samples=%d), Bayesian FFN of the same shape %9.0f tokens/s (%.1f ms), evaluate_swag is %.2f x that"
        % (S, n / t_mc, 1e3 * t_mc, t_swag / t_mc))
    say("  loss: mean weights %.4f, swag %.4f (mi %.4f), Bayesian mc %.4f (mi %.4f)" % (rep.loss, rs.loss, rs.mean_mi, mc.loss, mc.mean_mi))


if __name__ == "__main__":
    args = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "r19_swag_probe.txt")
    for flag in ("--out", "--model-path"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                path = args[i + 1]
            else:
                model_path = args[i + 1]
            del args[i:i + 2]
    with open(path, "w") as out_file:
        for w in (args or ["kernel", "rows", "engine"]):
            {"kernel": kernel_legs, "rows": rows_legs, "engine": engine_legs}[w]()
