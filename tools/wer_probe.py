#!/usr/bin/env python3
"""What the n-best WER kernels cost (csrc/nbest.hip), by device events, on synthetic lists.

    python tools/wer_probe.py [--quick]

  1. blm_edit_distance on all pairs i < j of 20- / 100- / 1000-best lists with hypotheses around 10 and around 60 words:
     pairs/s and DP cell updates/s (len(a) * len(b) per pair) under the default split between the two forms and with every
     pair forced through the wavefront form (option "edit_lane_max" 0).
  2. the same two forms on pairs of EQUAL length 2 ... 32 (where both are legal): where the lane-per-pair form stops winning.
  3. blm_nbest_select (64 grid points) and blm_nbest_mbr (one grid point) on the lists of 1., microseconds per call.
  4. the pairs of 1. (a sample of them) through the test reference (tests/nbest_reference.py, plain Python) on the host.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bayeslms_amd import ops  # noqa: E402
import nbest_reference as R  # noqa: E402

DEV = "cuda"


def timed(fn, reps):
    """median device microseconds of fn() over reps calls, after two warm-up calls"""
    for _ in range(2):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def lists(rng, utts, nbest, mean_len, vocab=2000):
    """each list: variations of one sentence (a word in eight replaced, dropped or doubled), as n-best lists are"""
    seqs, sizes = [], []
    for _ in range(utts):
        n = max(1, int(rng.normal(mean_len, mean_len / 4)))
        base = rng.integers(0, vocab, n)
        for _ in range(nbest):
            s = []
            for w in base:
                r = rng.random()
                if r < 0.04:
                    continue
                s.append(int(rng.integers(0, vocab)) if r < 0.08 else int(w))
                if r > 0.96:
                    s.append(int(rng.integers(0, vocab)))
            seqs.append(s)
        sizes.append(nbest)
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    tok = np.concatenate([np.asarray(s, np.int32) for s in seqs])
    uoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return tok, off, uoff


def all_pairs(uoff):
    a, b = [], []
    for lo, hi in zip(uoff[:-1], uoff[1:]):
        i, j = np.triu_indices(hi - lo, 1)
        a.append(i + lo)
        b.append(j + lo)
    return np.concatenate(a).astype(np.int32), np.concatenate(b).astype(np.int32)


def edit_forms(tok, off, a, b, reps):
    t = [torch.from_numpy(x).to(DEV) for x in (tok, off, a, b)]
    ln = np.diff(off)
    cells = float((ln[a].astype(np.float64) * ln[b]).sum())
    short = float((np.minimum(ln[a], ln[b]) <= 32).mean())
    out = {}
    for name, lane_max in (("default", 32), ("wavefront", 0)):
        ops.set_option("edit_lane_max", lane_max)
        try:
            out[name] = timed(lambda: ops.edit_distance(*t, breakdown=True), reps)
        finally:
            ops.set_option("edit_lane_max", 32)
    return len(a), cells, short, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, no 1000-best lists")
    args = ap.parse_args()
    reps = 5 if args.quick else 15
    rng = np.random.default_rng(7)
    print("device: %s" % torch.cuda.get_device_name(0))
    print("\n1. blm_edit_distance, all pairs i < j of every list (sub / ins / del written); median [min, max] of %d calls" % reps)
    print("%-26s %10s %7s | %-34s | %-34s" % ("lists", "pairs", "<=32", "default split", "all through the wavefront form"))
    shapes = [(400, 20, 10), (400, 20, 60), (64, 100, 10), (64, 100, 60)] + ([] if args.quick else [(4, 1000, 10), (4, 1000, 60)])
    kept = {}
    for utts, nbest, ml in shapes:
        tok, off, uoff = lists(rng, utts, nbest, ml)
        a, b = all_pairs(uoff)
        P, cells, short, res = edit_forms(tok, off, a, b, reps)
        kept[(utts, nbest, ml)] = (tok, off, uoff, a, b)
        cols = ["%8.1f us %7.1f Mpairs/s %6.2f Gcells/s" % (r[0], P / r[0], cells / r[0] / 1e3) for r in (res["default"], res["wavefront"])]
        print("%4d x %4d-best, ~%2d words %10d %6.0f%% | %s | %s" % (utts, nbest, ml, P, 100 * short, cols[0], cols[1]))
        print("%52s [%.1f, %.1f] us %22s [%.1f, %.1f] us" % ("", res["default"][1], res["default"][2], "", res["wavefront"][1], res["wavefront"][2]))

    print("\n2. both forms on 262144 pairs of EQUAL length (three-word alphabet)")
    print("%6s | %-44s | %-44s | %s" % ("length", "lane-per-pair", "wavefront", "lane / wavefront"))
    for n in (2, 4, 8, 9, 12, 16, 17, 24, 32):
        S = 4096
        tok = rng.integers(0, 3, S * n).astype(np.int32)
        off = (np.arange(S + 1) * n).astype(np.int64)
        a, b = rng.integers(0, S, 262144).astype(np.int32), rng.integers(0, S, 262144).astype(np.int32)
        P, cells, _, res = edit_forms(tok, off, a, b, reps)
        cols = ["%8.1f us %7.1f Mpairs/s %6.2f Gcells/s" % (r[0], P / r[0], cells / r[0] / 1e3) for r in (res["default"], res["wavefront"])]
        print("%6d | %s | %s | %.2f" % (n, cols[0], cols[1], res["default"][0] / res["wavefront"][0]))

    print("\n3. selection on the lists of 1.: blm_nbest_select at 64 grid points, blm_nbest_mbr at one (risk written),")
    print("   and the distance blocks it reads (ops.pairwise_edit_distance: index building in torch + blm_edit_distance + the fill)")
    for key, (tok, off, uoff, a, b) in kept.items():
        H = int(uoff[-1])
        c = [torch.from_numpy(rng.normal(50, 10, H)).to(DEV) for _ in range(4)] + [torch.from_numpy(np.diff(off).astype(np.float64)).to(DEV)]
        u = torch.from_numpy(uoff).to(DEV)
        grid = [(7.0 + k % 11, (k // 11) / 6.0, 0.0, 1.0) for k in range(64)]
        sel = timed(lambda: ops.nbest_select(*c, u, grid), reps)
        t, o = torch.from_numpy(tok).to(DEV), torch.from_numpy(off).to(DEV)
        blocks = timed(lambda: ops.pairwise_edit_distance(t, o, u), max(3, reps // 3))
        dist, doff = ops.pairwise_edit_distance(t, o, u)
        mbr = timed(lambda: ops.nbest_mbr(*c, u, dist, doff, grid[:1]), reps)
        print("%4d x %4d-best, ~%2d words: select %8.1f us [%.1f, %.1f]   mbr %8.1f us [%.1f, %.1f] (%.2f G terms/s)   blocks %9.1f us"
              % (key + sel + mbr + (float(dist.numel()) / mbr[0] / 1e3, blocks[0])))

    print("\n4. the test reference on the host (tests/nbest_reference.py, plain Python, one core): a sample of the pairs of 1.")
    for key in ((400, 20, 10), (400, 20, 60)):
        tok, off, uoff, a, b = kept[key]
        k = 2000 if key[2] == 10 else 200
        ln = np.diff(off)
        t0 = time.perf_counter()
        R.edit_distance(tok, off, a[:k], b[:k])
        dt = time.perf_counter() - t0
        cells = float((ln[a[:k]].astype(np.float64) * ln[b[:k]]).sum())
        print("~%2d words: %d pairs in %.2f s = %.1f kpairs/s, %.2f Mcells/s" % (key[2], k, dt, k / dt / 1e3, cells / dt / 1e6))


if __name__ == "__main__":
    main()
