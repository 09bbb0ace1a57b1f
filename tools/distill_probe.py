#!/usr/bin/env python3
"""What distillation costs: blm_ce_soft_fwd_bwd beside blm_ce_fwd_bwd, and a distilled training step beside a plain one.

A. kernel: 8192 x 33,000 logits (and 8192 x 33,278 in rows padded to 33,280), gradient written in place, the hard-label kernel
   and the soft one on the SAME buffers in the same run: kernel time by device events over 30 launches of the C entry points,
   three logit buffers (and three teacher buffers) in turn so that no launch finds its rows in the Infinity Cache, median of 5,
   and the bytes each must move over that time (hard: read + write the logits; soft: the teacher's rows as well).
B. step: the configs[2] Bayesian Transformer (6 x d 512, ff 4096, 64 x 128 tokens, V 33,000) trained plain, then against a
   teacher of the same architecture at mean weights (S = 0) and under S = 2 and 8 Monte-Carlo samples: ms per step (teacher
   pass + student step), median of 10 after 3 warm-up steps, a device synchronise inside each timed step.

--top-k K adds the sparse path beside both:
A. blm_ce_soft_topk_fwd_bwd against the K best entries of the same teacher rows, as a third leg on the same logit buffers in the
   same rotation (it must move the logits twice and 2 K values per row), and ops.topk_rows on the 8192 x V teacher alone: what
   extracting the targets on the fly costs per batch.
B. the step with the targets extracted ON THE FLY (teacher pass + top-k + student step; mean weights and S = 8) and from a
   complete CACHE on disk (distill.TeacherCache.load + student step, no teacher): the second is what every epoch after the
   first, and every later run against the same teacher, pays.

--temperature T adds the tempered kernels (include/bayeslm.h, blm_ce_soft_temp_fwd_bwd) beside the untempered ones:
A. blm_ce_soft_temp_fwd_bwd at beta = 1 / T, soft_scale = T^2 -- and with --top-k blm_ce_soft_topk_temp_fwd_bwd -- as further legs on
   the same buffers, in the same rotation, in the same run; each is reported as a ratio to its untempered kernel, whose
   source the temperature did not touch.
B. the step against the mean-weight teacher's dense rows at temperature T and, with --top-k, from the complete cache at T.

usage: distill_probe.py [--top-k K] [--temperature T] [kernel|step ...]   (default: both)"""
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from bayeslms_amd import distill, engine, model as M, ops  # noqa: E402
from bayeslms_amd.data import synthetic_corpus  # noqa: E402

dev = torch.device("cuda:0")


def say(*a):
    print(*a, flush=True)


def kernel_legs(V, top_k=0, temperature=1.0):
    from bayeslms_amd import _lib as L
    L.require_gfx950()
    R, NB, N = 8192, 3, 30
    ld = (V + 3) // 4 * 4
    g = torch.Generator(device=dev).manual_seed(1)
    zs = [3.0 * torch.randn(R, ld, device=dev, generator=g) for _ in range(NB)]
    qs = [torch.log_softmax(3.0 * torch.randn(R, ld, device=dev, generator=g)[:, :V], 1) for _ in range(NB)]
    qs = [torch.nn.functional.pad(q, (0, ld - V)) for q in qs]
    tgt = torch.randint(0, V, (R,), device=dev, generator=g)
    f = [torch.empty(R, device=dev) for _ in range(5)]
    total = torch.zeros(1, device=dev)
    c, st = L.calls(), L.stream()
    say("# A. %d x %d logits, row stride %d (%.0f MB), gradient in place, %d buffers in turn; us per launch by device events over %d "
        "launches, median of 5" % (R, V, ld, R * V * 4 / 1e6, NB, N))
    legs = (("blm_ce_fwd_bwd", 2, lambda k: c.blm_ce_fwd_bwd(zs[k].data_ptr(), ld, tgt.data_ptr(), f[0].data_ptr(), None, total.data_ptr(),
                                                             zs[k].data_ptr(), 1.0 / R, R, V, st)),
            ("blm_ce_soft_fwd_bwd", 3, lambda k: c.blm_ce_soft_fwd_bwd(zs[k].data_ptr(), ld, qs[k].data_ptr(), ld, tgt.data_ptr(), 0.5,
                                                                       f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), f[3].data_ptr(),
                                                                       None, total.data_ptr(), zs[k].data_ptr(), 1.0 / R, R, V, st)))
    if top_k:
        best = [torch.topk(q[:, :V], top_k, dim=1) for q in qs]
        ks = [(b.indices.to(torch.int32).contiguous(), b.values.contiguous()) for b in best]
        legs += (("blm_ce_soft_topk_fwd_bwd", 2, lambda k: c.blm_ce_soft_topk_fwd_bwd(
            zs[k].data_ptr(), ld, ks[k][0].data_ptr(), ks[k][1].data_ptr(), top_k, top_k, tgt.data_ptr(), 0.5, f[0].data_ptr(),
            f[1].data_ptr(), f[2].data_ptr(), f[3].data_ptr(), None, total.data_ptr(), zs[k].data_ptr(), 1.0 / R, R, V, st)),
                 ("ops.topk_rows k = %d" % top_k, 1, lambda k: ops.topk_rows(qs[k][:, :V], top_k)))
    if temperature != 1.0:
        beta, scale = 1.0 / temperature, temperature * temperature
        legs += (("blm_ce_soft_temp_fwd_bwd", 3, lambda k: c.blm_ce_soft_temp_fwd_bwd(
            zs[k].data_ptr(), ld, qs[k].data_ptr(), ld, tgt.data_ptr(), 0.5, beta, scale, f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(),
            f[3].data_ptr(), None, total.data_ptr(), zs[k].data_ptr(), 1.0 / R, R, V, st)),)
        if top_k:
            legs += (("blm_ce_soft_topk_temp_fwd_bwd", 2, lambda k: c.blm_ce_soft_topk_temp_fwd_bwd(
                zs[k].data_ptr(), ld, ks[k][0].data_ptr(), ks[k][1].data_ptr(), top_k, top_k, tgt.data_ptr(), 0.5, beta, scale,
                f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), f[3].data_ptr(), None, total.data_ptr(), zs[k].data_ptr(), 1.0 / R, R,
                V, st)),)
    us = {}
    for name, passes, fn in legs:
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
        us[name] = statistics.median(times)
        nbytes = passes * R * V * 4 + (2 * top_k * R * 4 if "soft_topk" in name else 0)
        say("%-29s V %5d %8.1f us  %5.2f TB/s of the %d MB it must move" % (name, V, us[name], nbytes / us[name] / 1e6, nbytes // 10 ** 6))
    say("soft / hard at V %d: %.2f x  (3 matrices against 2: 1.5 by bytes)" % (V, us["blm_ce_soft_fwd_bwd"] / us["blm_ce_fwd_bwd"]))
    if top_k:
        t = us["blm_ce_soft_topk_fwd_bwd"]
        say("top-%d / hard at V %d: %.2f x  (%.3f by bytes);  top-%d / dense soft: %.2f x%s" % (
            top_k, V, t / us["blm_ce_fwd_bwd"], (2 * V + 2 * top_k) / (2.0 * V), top_k, t / us["blm_ce_soft_fwd_bwd"],
            "" if t <= us["blm_ce_soft_fwd_bwd"] else "  SLOWER THAN THE DENSE KERNEL: the gather or the correction step is wrong, no result"))
    if temperature != 1.0:
        say("tempered / untempered dense soft at V %d, T = %g: %.2f x  (the same 3 matrices; 6 exponentials per element against 4)"
            % (V, temperature, us["blm_ce_soft_temp_fwd_bwd"] / us["blm_ce_soft_fwd_bwd"]))
        if top_k:
            say("tempered / untempered top-%d at V %d, T = %g: %.2f x  (the same 2 matrices; 4 exponentials per element against 2)"
                % (top_k, V, temperature, us["blm_ce_soft_topk_temp_fwd_bwd"] / us["blm_ce_soft_topk_fwd_bwd"]))


def step_legs(top_k=0, temperature=1.0):
    T, B, V = 128, 64, bench.V

    def build():
        return M.BayesTransformerModel(V, bench.D_MODEL, bench.NHEAD, bench.D_FF, bench.NLAYERS, bench.DROPOUT, True, "FFN").to(dev)

    torch.manual_seed(1111)
    teacher_model = build().requires_grad_(False)
    stream = synthetic_corpus(V, B * (14 * T + 1), seed=2222).to(dev)
    src = stream[:B * (14 * T + 1) // B * B].view(B, -1).t().contiguous()
    kl_fn = lambda m: m.transformerlayers[0].linear2.kl_divergence()  # noqa: E731
    kl_fn.fusable = True
    say("# B. configs[2] Bayesian Transformer, %d x %d tokens per step, V %d; ms per step (teacher pass + student step), median of 10 "
        "after 3 warm-up steps" % (B, T, V))
    base = None
    cache = None
    if top_k:  # the cache of this walk, filled once from the mean-weight teacher: what a later epoch or run finds on disk
        path = os.path.join(tempfile.mkdtemp(), "teacher.cache")
        cache = distill.TeacherCache(path, distill.TeacherCache.describe(V, top_k, False, T, src.size(0), B, "probe", "probe", {}, 0, 1111))
        filler = distill.Teacher(teacher_model)
        for k in range(14):
            sparse, kept = filler.topk(src[k * T:(k + 1) * T], top_k)
            cache.store(k * T * B, sparse)
        cache.finish()
        say("# top-%d targets: mean kept teacher mass %.3f (an untrained teacher's: no statement about a trained one); cache of %d rows, %.1f MB, %.2f MB per "
            "batch" % (top_k, float(kept.mean()), cache.n, os.path.getsize(path) / 1e6, T * B * top_k * 8 / 1e6))
    legs = [(None, "plain"), (0, "dense"), (2, "dense"), (8, "dense")]
    if top_k:
        legs += [(0, "topk"), (8, "topk"), (0, "cache")]
    legs = [leg + (1.0,) for leg in legs]
    if temperature != 1.0:
        legs += [(0, "dense", temperature)] + ([(0, "cache", temperature)] if top_k else [])
    for S, how, temp in legs:
        torch.manual_seed(7)
        student = build()
        tr = engine.Trainer(student, lr=0.1, clip=1.0, kl_scale=T / float(src.size(0)), seed=1111)
        teacher = None if S is None else distill.Teacher(teacher_model, mc_samples=S)
        times = []
        for k in range(13):
            data, tgt = src[k * T:(k + 1) * T], src[k * T + 1:(k + 1) * T + 1].reshape(-1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if teacher is None:
                tr.step(data, tgt, None, kl_fn)
            elif how == "cache":
                tr.step(data, tgt, None, kl_fn, soft=(cache.load(k * T * B, T * B, dev), 0.5, temp))
            elif how == "topk":
                tr.step(data, tgt, None, kl_fn, soft=(teacher.topk(data, top_k)[0], 0.5, temp))
            else:
                logq, _ = teacher.logprobs(data)
                tr.step(data, tgt, None, kl_fn, soft=(logq, 0.5, temp))
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        ms = statistics.median(times[3:])
        base = base or ms
        name = ("plain" if S is None else "top-%d from the cache, no teacher" % top_k if how == "cache" else
                "teacher S = %d%s" % (S, ", top-%d on the fly" % top_k if how == "topk" else ""))
        name += "" if temp == 1.0 else ", T = %g" % temp
        say("%-43s %8.2f ms per step  %5.2f x plain" % (name, ms, ms / base))
        del student, tr, teacher


if __name__ == "__main__":
    argv, top_k, temperature = sys.argv[1:], 0, 1.0
    if "--temperature" in argv:
        i = argv.index("--temperature")
        temperature = float(argv[i + 1])
        del argv[i:i + 2]
    if "--top-k" in argv:
        i = argv.index("--top-k")
        top_k = int(argv[i + 1])
        del argv[i:i + 2]
    for w in (argv or ["kernel", "step"]):
        if w == "kernel":
            with torch.no_grad():
                kernel_legs(33000, top_k, temperature)
                kernel_legs(33278, top_k, temperature)
        else:
            step_legs(top_k, temperature)
