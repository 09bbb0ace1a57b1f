#!/usr/bin/env python3
"""What distillation costs: blm_ce_soft_fwd_bwd beside blm_ce_fwd_bwd, and a distilled training step beside a plain one.

A. kernel: 8192 x 33,000 logits (and 8192 x 33,278 in rows padded to 33,280), gradient written in place, the hard-label kernel
   and the soft one on the SAME buffers in the same run: kernel time by device events over 30 launches of the C entry points,
   three logit buffers (and three teacher buffers) in turn so that no launch finds its rows in the Infinity Cache, median of 5,
   and the bytes each must move over that time (hard: read + write the logits; soft: the teacher's rows as well).
B. step: the configs[2] Bayesian Transformer (6 x d 512, ff 4096, 64 x 128 tokens, V 33,000) trained plain, then against a
   teacher of the same architecture at mean weights (S = 0) and under S = 2 and 8 Monte-Carlo samples: ms per step (teacher
   pass + student step), median of 10 after 3 warm-up steps, a device synchronise inside each timed step.

usage: distill_probe.py [kernel|step ...]   (default: both)"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from bayeslms_amd import distill, engine, model as M  # noqa: E402
from bayeslms_amd.data import synthetic_corpus  # noqa: E402

dev = torch.device("cuda:0")


def say(*a):
    print(*a, flush=True)


def kernel_legs(V):
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
        nbytes = passes * R * V * 4
        say("%-22s V %5d %8.1f us  %5.2f TB/s of the %d MB it must move" % (name, V, us[name], nbytes / us[name] / 1e6, nbytes // 10 ** 6))
    say("soft / hard at V %d: %.2f x  (3 matrices against 2: 1.5 by bytes)" % (V, us["blm_ce_soft_fwd_bwd"] / us["blm_ce_fwd_bwd"]))


def step_legs():
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
    for S in (None, 0, 2, 8):
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
            else:
                logq, _ = teacher.logprobs(data)
                tr.step(data, tgt, None, kl_fn, soft=(logq, 0.5))
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        ms = statistics.median(times[3:])
        base = base or ms
        say("%-28s %8.2f ms per step  %5.2f x plain" % ("plain" if S is None else "teacher S = %d" % S, ms, ms / base))
        del student, tr, teacher


if __name__ == "__main__":
    for w in (sys.argv[1:] or ["kernel", "step"]):
        if w == "kernel":
            with torch.no_grad():
                kernel_legs(33000)
                kernel_legs(33278)
        else:
            step_legs()
