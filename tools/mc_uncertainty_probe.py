"""Cost of the token-level Monte-Carlo uncertainty (ops.linear_mc_stats, compute_scores_batched(uncertainty=True)).

  --kernel        the headline decoder shape, 2048 tokens x S = 8 samples x 33,000 words x K = 512, called --iters times (run it
                  under `rocprofv3 --kernel-trace --stats` for kernel times: both passes are gemm_f32_kernel launches over the
                  same 16,384 rows, pass 1 followed by ce_part_finish_kernel, pass 2 by mc_stats_finish_kernel)
  --samples S     samples per token of --kernel / --split-trace (default 8); the rows per pass are 2048 x S rounded up to a power
                  of two
  --split-trace CSV   per-pass summary of a rocprofv3 kernel_trace.csv of a --kernel run: mean time of pass 1 (the CE_PART
                  launch blm_linear_nll does) and pass 2 (the MC_PART launch), each as a fraction of the fp32 MFMA peak
  --e2e           BASELINE configs[4]'s GP Transformer (--T_gauss_pos 3, 33,000 words, d 512, 6 layers) rescoring a synthetic
                  AMI-shaped n-best list with 8 Monte-Carlo samples, uncertainty off and on, alternated in one process
"""
import argparse
import csv
import random
import statistics
import sys
import time
from collections import OrderedDict

sys.path.insert(0, ".")

PEAK_F32_MFMA = 157.3e12  # MI355X fp32 matrix peak, FLOP/s (v_mfma_f32_32x32x2_f32)
M_TOK, V, K = 2048, 33000, 512


def kernel(iters, S):
    import torch
    from bayeslms_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M_TOK, K, device=dev, generator=g) + 0.5 * torch.randn(S, M_TOK, K, device=dev, generator=g)
    w = torch.randn(V, K, device=dev, generator=g) * (4.0 / K ** 0.5)
    b = torch.randn(V, device=dev, generator=g)
    tgt = torch.randint(0, V, (M_TOK,), device=dev, generator=g)
    with torch.no_grad():
        for _ in range(3):
            ops.linear_mc_stats(x, w, b, tgt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            st = ops.linear_mc_stats(x, w, b, tgt)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / iters
    flops = 2.0 * M_TOK * (1 << (S - 1).bit_length()) * V * K
    print("linear_mc_stats %d tokens x S %d x V %d x K %d: %.3f ms per call (host clock, both passes + packing + folds); "
          "one pass at the fp32 MFMA peak: %.3f ms" % (M_TOK, S, V, K, dt * 1e3, flops / PEAK_F32_MFMA * 1e3))
    print("mean h_pred %.4f  mean mi %.5f  mean bma_nll %.4f" % (float(st.h_pred.mean()), float(st.mi.mean()), float(st.bma_nll.mean())))


def split_trace(path, S):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    p1, p2 = [], []
    for i, r in enumerate(rows):
        if "gemm_f32_kernel" not in r["Kernel_Name"] or i + 1 >= len(rows):
            continue
        nxt = rows[i + 1]["Kernel_Name"]
        dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
        if "ce_part_finish_kernel" in nxt:
            p1.append(dur)
        elif "mc_stats_finish_kernel" in nxt:
            p2.append(dur)
    flops = 2.0 * M_TOK * (1 << (S - 1).bit_length()) * V * K
    for name, d in (("pass 1 (CE_PART, blm_linear_nll's launch)", p1), ("pass 2 (MC_PART)", p2)):
        m = statistics.mean(d)
        print("%-42s %3d launches  mean %8.1f us  min %8.1f  max %8.1f  -> %.3f of the fp32 MFMA peak"
              % (name, len(d), m * 1e6, min(d) * 1e6, max(d) * 1e6, flops / m / PEAK_F32_MFMA))
    print("pass 2 / pass 1 = %.3f" % (statistics.mean(p2) / statistics.mean(p1)))


def e2e(reps, n_utt, n_hyp):
    import torch
    from bayeslms_amd import compute_sentence_scores as css, model as M
    dev = torch.device("cuda:0")
    Vw = 33000
    rnd = random.Random(7)
    words = ["w%d" % i for i in range(Vw - 2)]
    vocab = {w: i + 2 for i, w in enumerate(words)}
    vocab["<s>"], vocab["<unk>"] = 0, 1
    nbest = OrderedDict()
    for u in range(n_utt):
        base = [rnd.choice(words) for _ in range(rnd.randint(6, 30))]
        hyps = []
        for _ in range(n_hyp):
            h = list(base)
            for _ in range(rnd.randint(0, 3)):
                h[rnd.randrange(len(h))] = rnd.choice(words)
            hyps.append(" ".join(h))
        nbest["utt%03d" % u] = hyps
    total = n_utt * n_hyp
    torch.manual_seed(1111)
    m = M.GaussTransformerModel(Vw, 512, 8, 4096, 6, 0.2, True, 3).to(dev)

    def run(unc):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = css.compute_scores_batched(nbest, m, vocab, "Transformer", dev, mc_samples=8, uncertainty=unc)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    run(False)
    run(True)  # warm-up: code objects, plan, allocator
    t = {False: [], True: []}
    for _ in range(reps):
        for unc in (False, True):
            t[unc].append(run(unc)[0])
    _, (sc, unc) = run(True)
    _, base = run(False)
    worst = max(abs(a - b) / max(1.0, abs(b)) for k in base for (_, a), (_, b) in zip(sc[k], base[k]))
    for unc in (False, True):
        d = t[unc]
        print("uncertainty %-3s  %d hypotheses, 8 MC samples: median %.3f s (min %.3f, max %.3f, %d runs)  %.0f hypotheses/s"
              % ("on" if unc else "off", total, statistics.median(d), min(d), max(d), len(d), total / statistics.median(d)))
    print("on / off = %.3f (medians); worst score difference on vs off %.2e relative" %
          (statistics.median(t[True]) / statistics.median(t[False]), worst))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--split-trace", type=str, default="")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--utts", type=int, default=40)
    ap.add_argument("--hyps", type=int, default=100)
    a = ap.parse_args()
    if a.split_trace:
        split_trace(a.split_trace, a.samples)
    if a.kernel:
        kernel(a.iters, a.samples)
    if a.e2e:
        e2e(a.reps, a.utts, a.hyps)


if __name__ == "__main__":
    main()
