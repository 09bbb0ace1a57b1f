"""Training engine: flat parameter / gradient / momentum buffers, fused clip+SGD, and the
data-parallel gradient exchange (one process per GPU, RCCL over xGMI).

The reference trains in one process on one GPU (train.py:306-438).  New here: the step is
data-parallel over global-batch columns; all gradients live in ONE flat fp32
buffer that the wgrad kernels accumulate into in place, cut into buckets that are all-reduced on a
side stream as soon as backward has produced them (reverse parameter order), overlapping the
remaining backward GEMMs; then one fused global-norm clip + SGD-momentum kernel pass over the
three flat buffers (train.py:419-420,466 semantics, averaged over ranks).
"""
import contextlib
import dataclasses
import datetime
import gc
import itertools
import math
import os
import sys
import time
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from . import ops


RCCL_CHANNELS_DEFAULT = 16


def pin_rccl_channels(n=None):
    """Call BEFORE dist.init_process_group("nccl").  Pins RCCL's channel count (one 256-thread workgroup per channel and
    collective, each holding a CU's registers beside the backward GEMMs) with NCCL_MIN_NCHANNELS / NCCL_MAX_NCHANNELS unless
    the user has set them: ``n`` or BLM_RCCL_CHANNELS or 16.  Why 16 (profiles/r04_comm_occupancy_rehearsal.txt): the
    cfg3 gradient is 202 MB per 20 ms step -- 18 GB/s of bus bandwidth would hide it under backward -- and in the one-GPU
    rehearsal a 16-workgroup stand-in at 150-300 GB/s costs the step 1.1 ms (5 %), 8 workgroups cannot stream a bucket
    fast enough (2.3 ms, most of it exposed) and 32 cost 0.7-1.9 ms.  0 leaves RCCL's own choice.
    -> the settings in force (recorded in bench.py's ``comm``)."""
    n = int(os.environ.get("BLM_RCCL_CHANNELS", RCCL_CHANNELS_DEFAULT if n is None else n))
    if n > 0:
        os.environ.setdefault("NCCL_MIN_NCHANNELS", str(n))
        os.environ.setdefault("NCCL_MAX_NCHANNELS", str(n))
    return {k: os.environ.get(k) for k in ("NCCL_MIN_NCHANNELS", "NCCL_MAX_NCHANNELS")}


DIST_TIMEOUT_S = 180.0
_T0 = time.time()
_STAGE = {"last": "process start"}


def heartbeat(stage, rank=None):
    """One line on stderr per stage of a multi-rank run (``[blm rank R +S.Ss] stage``) and the stage remembered for
    ``last_stage()``: a run that stops -- a rendezvous nobody joins, a collective one rank never enters -- says where.
    bench.py's launcher parent parses these lines; they never go to stdout (the one JSON line lives there)."""
    if rank is None:
        rank = int(os.environ.get("RANK", "0"))
    _STAGE["last"] = stage
    sys.stderr.write("[blm rank %d +%.1fs] %s\n" % (rank, time.time() - _T0, stage))
    sys.stderr.flush()


def last_stage():
    return _STAGE["last"]


def dist_timeout_s(timeout_s=None):
    return float(os.environ.get("BLM_DIST_TIMEOUT_S", DIST_TIMEOUT_S if timeout_s is None else timeout_s))


def init_distributed(backend, device=None, timeout_s=None, **kw):
    """dist.init_process_group with a BOUNDED rendezvous and collective timeout (``timeout_s`` or BLM_DIST_TIMEOUT_S or
    180 s, not torch's 10 / 30 minutes: a rank that never arrives ends the job inside the timeout -- the store raises, and the
    RCCL watchdog aborts the process when a collective outlives it), RCCL's channel count pinned first
    (pin_rccl_channels), and two heartbeats: ``rendezvous ok`` when the group exists, ``first all-reduce ok`` after an
    8-byte all-reduce whose result is checked (the first real contact of the ranks' communicators -- on RCCL the ring /
    tree set-up over xGMI happens here).  -> the RCCL channel settings in force (None for another backend).
    The reference has no counterpart: one process, one device (train.py:136)."""
    timeout = datetime.timedelta(seconds=dist_timeout_s(timeout_s))
    rccl_env = None
    if backend == "nccl":
        rccl_env = pin_rccl_channels()  # before RCCL reads its environment
        if os.environ.get("NCCL_MAX_NCHANNELS"):
            sys.stderr.write("[blm] RCCL channels pinned: %s (BLM_RCCL_CHANNELS=0 leaves RCCL's own choice)\n" % (rccl_env,))
        dist.init_process_group("nccl", device_id=device, timeout=timeout, **kw)  # nccl == RCCL on ROCm
    else:
        dist.init_process_group(backend, timeout=timeout, **kw)
    world, rank = dist.get_world_size(), dist.get_rank()
    heartbeat("rendezvous ok (world %d, backend %s, timeout %.0f s)" % (world, backend, timeout.total_seconds()), rank)
    on_dev = backend == "nccl"
    t = torch.ones(1, dtype=torch.float64, device=device if on_dev else "cpu")
    dist.all_reduce(t)
    if float(t.item()) != float(world):
        raise RuntimeError("first all-reduce returned %r on rank %d, world %d" % (float(t.item()), rank, world))
    heartbeat("first all-reduce ok", rank)
    return rccl_env


def allreduce_busbw(nbytes, reps=5, device=None, group=None):
    """Stand-alone all-reduce of ``nbytes`` (fp32 sum), ``reps`` timed repetitions after one warm-up, nothing else on the
    device: what the links give the gradient exchange when it does not share the chip with backward.
    busbw = 2 (N-1)/N x bytes / time (the ring's per-link traffic, RCCL-tests' convention).  Collective: every rank calls."""
    world = dist.get_world_size(group)
    n = max(1, int(nbytes) // 4)
    cuda = device is not None and torch.device(device).type == "cuda" and dist.get_backend(group) == "nccl"  # gloo: host tensors
    x = torch.zeros(n, dtype=torch.float32, device=device if cuda else "cpu")
    dist.all_reduce(x, group=group)
    if cuda:
        torch.cuda.synchronize()
    gc_was_on = gc.isenabled()
    gc.disable()  # a full collection of the interpreter's heap takes tens of ms: it must not land between the two clock reads
    try:
        dist.barrier(group)
        t0 = time.perf_counter()
        for _ in range(reps):
            dist.all_reduce(x, group=group)
        if cuda:
            torch.cuda.synchronize()
        el = (time.perf_counter() - t0) / reps
    finally:
        if gc_was_on:
            gc.enable()
    t = torch.tensor([el], dtype=torch.float64, device=device if cuda else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    el = float(t.item())
    alg = n * 4 / el / 1e9
    return {"mb": round(n * 4 / 1e6, 2), "reps": reps, "ms": round(1e3 * el, 4), "algbw_gbps": round(alg, 2),
            "busbw_gbps": round(alg * 2.0 * (world - 1) / max(world, 1), 2)}


def rccl_version():
    try:
        v = torch.cuda.nccl.version()
        return ".".join(str(x) for x in v) if isinstance(v, (tuple, list)) else str(v)
    except Exception:  # noqa: BLE001
        return None


def rccl_channels():
    """The channel count RCCL was pinned to (0: unknown / RCCL's own choice -- the planner then keeps the whole chip)."""
    try:
        return max(0, int(os.environ.get("NCCL_MAX_NCHANNELS", "0")))
    except ValueError:
        return 0


class FlatBuffers:
    """Re-homes every distinct parameter of ``model`` into one contiguous buffer and gives each a
    ``.grad`` view into a second one.  Tied tensors (decoder.weight is encoder.weight) appear once."""

    def __init__(self, model):
        self.params = [p for p in model.parameters() if p.requires_grad]
        dev, dt = self.params[0].device, self.params[0].dtype
        sizes = [p.numel() for p in self.params]
        # 16-byte aligned slots so every tensor keeps the vectorised kernel paths
        self.offsets, off = [], 0
        for n in sizes:
            self.offsets.append(off)
            off += (n + 3) // 4 * 4
        self.total = off
        self.flat_param = torch.zeros(off, device=dev, dtype=dt)
        self.flat_grad = torch.zeros(off, device=dev, dtype=dt)
        self.flat_mom = torch.zeros(off, device=dev, dtype=dt)
        for p, o, n in zip(self.params, self.offsets, sizes):
            view = self.flat_param[o:o + n].view_as(p)
            view.copy_(p.data)
            p.data = view
            p.grad = self.flat_grad[o:o + n].view_as(p)

    def zero_grad(self):
        self.flat_grad.zero_()


class _HostStagedReduce:
    """Handle of one all-reduce on a host-staged transport (gloo with device gradients): the transport reduced a host copy;
    wait() waits for it and writes the sums back on the communication stream with a blocking copy."""

    def __init__(self, work, host, view, stream):
        self.work, self.host, self.view, self.stream = work, host, view, stream

    def wait(self):
        self.work.wait()
        with torch.cuda.stream(self.stream):
            self.view.copy_(self.host)  # pageable source: returns when the bytes are on the device


class GradReducer:
    """Bucketed asynchronous all-reduce of a flat gradient buffer.

    ``mark_ready(param)`` is called once per gradient contribution: by the backward kernels' launchers
    (ops._notify, for gradients the wgrad kernels accumulate in place) and by a post-accumulate-grad hook on
    every parameter (``hook_autograd``, for gradients autograd's AccumulateGrad adds: LSTM weights, GP
    coefficients, VNN noise rows, ...).  A parameter with several contributions is ready after the last one;
    how many there are is counted in the first step (calibration: everything is reduced at ``finish()``).
    When every parameter of a bucket is ready the bucket is all-reduced (sum) on ``comm_stream`` behind an
    event recorded on the compute stream.  Safety rules (a stale or racing all-reduce makes ranks diverge
    silently, so none of these is inferred):
      * a parameter that was never marked in the calibration step holds its bucket back until ``finish()``;
      * a contribution that arrives after its bucket was launched raises (the write pattern changed:
        rebuild the Trainer or pass ``overlap=False``);
      * ``overlap=False`` reduces every bucket at ``finish()``.
    Works on any device / backend (the gloo tests drive it with CPU tensors); on the GPU the backend is
    "nccl" = RCCL.
    """

    def __init__(self, flat, bucket_bytes=32 << 20, group=None, expected=None, overlap=True, comm_cus=0, collective=None,
                 comm_plan=None, comm_gbps=None):
        self.flat = flat
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.cuda = flat.flat_grad.is_cuda
        self.comm_stream = torch.cuda.Stream() if self.cuda else None
        self.overlap = overlap
        # CU contention: RCCL runs one channel workgroup per channel (gfx950: 256 threads, ~280 registers per
        # lane, 19.7 KB LDS -- a CU that hosts one cannot also host an eight-wave GEMM workgroup, and a launch that is
        # exactly one round of 256 one-per-CU workgroups spills a second round: 1.74x, tools/comm_occupancy_rehearsal.py).
        # comm_plan "window" (default when comm_cus > 0): every bucket opens / extends the planner's comm window by its
        # expected time on the links (bytes / comm_gbps); the GEMMs enqueued behind it take the plans measured beside a
        # resident channel stand-in (csrc/gemm_plans_comm.inc) until their modelled time has used the window up.
        # "narrow": the planner counts on 256 - comm_cus CUs from the first bucket of a step until finish() (measured:
        # loses 1.5-10 % in situ -- buckets are in flight for a tenth of backward; kept for A/B).  "off": nothing.
        self.comm_cus = int(comm_cus) if self.cuda else 0
        comm_plan = comm_plan or os.environ.get("BLM_COMM_PLAN", "window")
        if comm_plan not in ("window", "narrow", "off"):
            raise ValueError("comm_plan / BLM_COMM_PLAN must be window, narrow or off, not %r" % (comm_plan,))
        self.comm_plan = comm_plan if self.comm_cus > 0 else "off"
        self.comm_gbps = float(os.environ.get("BLM_COMM_GBPS", "100") if comm_gbps is None else comm_gbps)
        self._narrowed = False
        # rehearsal (tools/comm_occupancy_rehearsal.py): fn(view, comm_stream) stands in for dist.all_reduce, world 1
        self.collective = collective
        self.late = None  # LateRows, set by the Trainer
        self.no_dense = set()  # buckets whose only tensor gets ALL of its gradient through LateRows (untied encoder)
        self.measure = False  # record (backward end, communication end) event pairs on the compute stream
        self.exposed_events = []
        # diagnostics, one step at a time (bench.py's comm block): every collective of the step bracketed on the communication
        # stream -> bucket_report().  The bracket makes the communication stream wait for each collective in turn, so it is
        # never on inside a timed region
        self.measure_buckets = False
        self.bucket_events, self.bucket_marks = [], []
        # BLM_DP_CHECK=1 (diagnosis, off by default): in front of every collective of the gradient exchange the ranks compare
        # (sequence number, element count) through a small all-gather; a disagreement raises with every rank's pair instead of
        # ending in a transport error (gloo) or a hang until the collective timeout (RCCL)
        # collectives ordered on the device's streams (RCCL) or staged through the host with a copy back on the transport's own stream (gloo)
        self.stream_ordered = not (dist.is_initialized() and dist.get_backend(group) != "nccl")
        self.check = os.environ.get("BLM_DP_CHECK", "0") == "1"
        self.seq = 0
        # buckets = contiguous runs of parameters, built from the END of the buffer (backward order).  Two refinements
        # for what is exposed at the end of backward:
        #  * a tensor of a bucket's size or more travels ALONE (the tied encoder / decoder weight, 67.6 MB at cfg3: with
        #    LateRows its dense half is complete after the FIRST backward kernel -- sharing a bucket with the first
        #    layer's parameters would hold it, and 100+ MB of all-reduce, until the last one);
        #  * the parameters that become ready last (the lowest offsets) go in quarter-size buckets: the final all-reduce,
        #    which nothing can hide, moves 8 MB instead of 32.
        per = max(1, bucket_bytes // 4)
        n = len(flat.params)
        sizes = [(flat.offsets[i + 1] if i + 1 < n else flat.total) - flat.offsets[i] for i in range(n)]
        first_small = next((i for i in range(n) if sizes[i] < per), n)  # first parameter behind the leading big tensor(s)
        tail_end = flat.offsets[first_small] + 2 * per if first_small < n else 0  # offsets below this: quarter-size buckets
        self.buckets = []  # (start, end, [param indices])
        idxs, end = [], flat.total
        for i in range(n - 1, -1, -1):
            if sizes[i] >= per and idxs:  # close the run behind a big tensor first
                self.buckets.append((flat.offsets[i + 1], end, list(idxs)))
                idxs, end = [], flat.offsets[i + 1]
            idxs.append(i)
            limit = per // 4 if (flat.offsets[i] < tail_end and sizes[i] < per) else per
            if end - flat.offsets[i] >= max(1, limit) or i == 0:
                self.buckets.append((flat.offsets[i], end, list(idxs)))
                idxs, end = [], flat.offsets[i]
        self.bucket_of = {}
        for b, (_, _, ids) in enumerate(self.buckets):
            for i in ids:
                self.bucket_of[id(flat.params[i])] = b
        self.expected = {id(p): 0 for p in flat.params}
        self.calibrating = expected is None
        for p, n in (expected or {}).items():
            self.expected[id(p)] = n
        self._hooks = []
        self.reset()

    def hook_autograd(self):
        """Every leaf parameter reports the gradients autograd accumulates into it (AccumulateGrad does not run for
        the ``None`` our in-place wgrad Functions return, so nothing is counted twice)."""
        if self._hooks:
            return
        for p in self.flat.params:
            self._hooks.append(p.register_post_accumulate_grad_hook(self.mark_ready))

    def unhook(self):
        for h in self._hooks:
            h.remove()
        self._hooks = []

    def reset(self):
        self.seen = {k: 0 for k in self.expected}
        # a never-marked parameter keeps its bucket for finish(): "never written" is not "ready"
        self.pending = [len(ids) for _, _, ids in self.buckets]
        self.launched = [False] * len(self.buckets)
        self.handles = []
        self.last_reduced_elems = getattr(self, "reduced_elems", 0)  # elements the finished step exchanged
        self.reduced_elems = 0

    def mark_ready(self, param):
        k = id(param)
        if k not in self.seen:
            return
        self.seen[k] += 1
        if self.calibrating or not self.overlap:
            return
        b = self.bucket_of[k]
        if self.launched[b]:
            raise ops.BayesLMError(
                "GradReducer: a gradient of a %s parameter was written after its bucket had been all-reduced (the "
                "set of backward kernels changed since the calibration step); build the Trainer with overlap=False "
                "for models whose graph changes between steps" % (tuple(param.shape),))
        if self.seen[k] != self.expected[k]:
            return
        self.pending[b] -= 1
        if self.pending[b] == 0:
            self._launch(b)

    def _launch(self, b):
        if self.launched[b]:
            return
        self.launched[b] = True
        if self.world == 1 and self.collective is None:
            return
        if b in self.no_dense and self.late is not None and self.late.used:
            return  # nothing dense was written: the compact exchange carries the whole gradient of this tensor
        s, e, _ = self.buckets[b]
        self._all_reduce(self.flat.flat_grad[s:e])

    def _check_agreement(self, view, what):
        self.seq += 1
        if os.environ.get("BLM_DP_TRACE"):  # diagnosis: this rank's sequence of collectives, one line each, no synchronisation added
            import threading
            with open("%s.rank%d" % (os.environ["BLM_DP_TRACE"], dist.get_rank() if dist.is_initialized() else 0), "a") as f:
                f.write("%d %s %d thread=%s\n" % (self.seq, what, view.numel(), threading.current_thread().name))
        if not self.check or self.world <= 1 or self.collective is not None:
            return
        on_dev = self.cuda and dist.get_backend(self.group) == "nccl"
        mine = torch.tensor([self.seq, view.numel()], dtype=torch.int64, device=view.device if on_dev else "cpu")
        every = [torch.empty_like(mine) for _ in range(self.world)]
        dist.all_gather(every, mine, group=self.group)
        pairs = [tuple(int(x) for x in e.tolist()) for e in every]
        if any(p != pairs[0] for p in pairs):
            raise ops.BayesLMError("GradReducer (BLM_DP_CHECK): the ranks disagree on collective %s: (sequence number, elements) "
                                   "per rank = %s" % (what, pairs))

    def _all_reduce(self, view, what="bucket"):
        self._check_agreement(view, what)
        self.reduced_elems += view.numel()
        if self.cuda:
            ev = torch.cuda.Event(enable_timing=self.measure_buckets)
            ev.record(torch.cuda.current_stream())
            self.comm_stream.wait_event(ev)
            if self.comm_plan == "window":
                ops.gemm_comm_window(view.numel() * view.element_size() / (self.comm_gbps * 1e3))
                self._narrowed = True
            elif self.comm_plan == "narrow" and not self._narrowed:
                ops.set_gemm_cus(max(8, ops.get_gemm_cus() - self.comm_cus))
                self._narrowed = True
            if self.collective is not None:
                self.collective(view, self.comm_stream)
                return
            if not self.stream_ordered:  # gloo on device tensors: staged through the host HERE (see LateRows.begin), same handles and order
                with torch.cuda.stream(self.comm_stream):
                    t0 = time.perf_counter()
                    host = view.to("cpu")  # waits for the communication stream, which waits for `ev`
                    h = _HostStagedReduce(dist.all_reduce(host, op=dist.ReduceOp.SUM, group=self.group, async_op=True), host, view,
                                          self.comm_stream)
                if self.measure_buckets:
                    h.wait()
                    self.bucket_marks.append((view.numel() * view.element_size(), t0, time.perf_counter()))
                else:
                    self.handles.append(h)
                return
            with torch.cuda.stream(self.comm_stream):
                if self.measure_buckets:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(self.comm_stream)
                    h = dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=True)
                    h.wait()  # the communication stream (not the host, on RCCL) waits for this collective
                    e1.record(self.comm_stream)
                    self.bucket_events.append((view.numel() * view.element_size(), ev, e0, e1))
                    return
                self.handles.append(dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        else:
            if self.measure_buckets:
                t0 = time.perf_counter()
                dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group)
                self.bucket_marks.append((view.numel() * view.element_size(), t0, time.perf_counter()))
                return
            self.handles.append(dist.all_reduce(view, op=dist.ReduceOp.SUM, group=self.group, async_op=True))

    def finish(self):
        """Launch whatever was not triggered (parameters without gradient this step), wait for all
        buckets and make the compute stream wait for the communication stream."""
        if self.calibrating:
            self.expected = dict(self.seen)
            self.calibrating = False
            if self.late is not None and self.late.used:
                # an UNTIED encoder weight under LateRows has no dense contribution at all (the tied one has the
                # decoder's): when it travels alone, its bucket would be all-reduced as zeros, fully exposed
                k = id(self.late.weight)
                b = self.bucket_of.get(k)
                if b is not None and self.expected[k] == 0 and len(self.buckets[b][2]) == 1:
                    self.no_dense.add(b)
        ev0 = None
        if (self.measure or self.measure_buckets) and self.cuda:
            ev0 = torch.cuda.Event(enable_timing=True)
            ev0.record(torch.cuda.current_stream())
            self.bwd_end_event = ev0
        self.bwd_end_mark = time.perf_counter()
        for b in range(len(self.buckets)):
            self._launch(b)
        for h in self.handles:
            h.wait()
        if self.cuda and (self.world > 1 or self.collective is not None):
            torch.cuda.current_stream().wait_stream(self.comm_stream)
        if self._narrowed:  # whatever is enqueued from here on starts after the last bucket has landed
            if self.comm_plan == "window":
                ops.gemm_comm_window(0)
            else:
                ops.set_gemm_cus(0)
            self._narrowed = False
        if ev0 is not None and self.measure:
            ev1 = torch.cuda.Event(enable_timing=True)
            ev1.record(torch.cuda.current_stream())
            self.exposed_events.append((ev0, ev1))
        if self.late is not None:
            self.late.apply()
        self.reset()

    def bucket_report(self):
        """After ONE step taken with ``measure_buckets`` raised: one entry per collective of that step, in launch order --
        its size, launch -> done on the communication stream (ms), and where it sat relative to the end of backward
        (``ready_before_bwd_end_ms``: how long before the last backward kernel the bucket's gradients were complete;
        ``done_after_bwd_end_ms`` > 0: that much of it was exposed).  Synchronises; clears the record."""
        out = []
        if self.cuda and self.stream_ordered:
            torch.cuda.synchronize()
            end = getattr(self, "bwd_end_event", None)
            for nbytes, ready, e0, e1 in self.bucket_events:
                r = {"mb": round(nbytes / 1e6, 2), "ms": round(e0.elapsed_time(e1), 4)}
                if end is not None:
                    r["ready_before_bwd_end_ms"] = round(ready.elapsed_time(end), 4)
                    r["done_after_bwd_end_ms"] = round(end.elapsed_time(e1), 4)
                out.append(r)
        else:
            for nbytes, t0, t1 in self.bucket_marks:
                out.append({"mb": round(nbytes / 1e6, 4), "ms": round(1e3 * (t1 - t0), 4),
                            "ready_before_bwd_end_ms": round(1e3 * (self.bwd_end_mark - t0), 4),
                            "done_after_bwd_end_ms": round(1e3 * (t1 - self.bwd_end_mark), 4)})
        self.bucket_events, self.bucket_marks = [], []
        return out

    def comm_exposed_ms(self):
        """Average time per step the compute stream sat between the last backward kernel and the end of the
        gradient exchange (what the overlap did not hide).  Synchronises."""
        if not self.exposed_events:
            return None
        torch.cuda.synchronize()
        v = [a.elapsed_time(b) for a, b in self.exposed_events]
        return sum(v) / len(v)


class LateRows:
    """The embedding half of the (usually tied) encoder gradient, exchanged as a compact matrix.

    The tied encoder/decoder weight (model.py:1240; V x d = 67.6 MB at cfg3) gets its gradient from the FIRST
    backward kernel (decoder wgrad) and from the LAST one (embedding scatter), so as one tensor its all-reduce
    starts when backward is over and is fully exposed.  Here the decoder contribution is reduced with the
    other buckets while backward runs, and the embedding contribution -- at most T*B distinct rows per rank --
    goes to a compact (U, d) matrix, U = number of distinct token ids of the GLOBAL batch this step, which is
    all-reduced at the end of backward and added into the flat gradient (blm_rows_gather_add).  The row
    numbering is agreed at the START of the step, off the critical path: ids are all-gathered on the
    communication stream, presence bitmap -> prefix sum -> slot per vocabulary row (fixed-size tensor ops, no
    host synchronisation); only U travels to the host (pinned copy + event, read when backward reaches the
    embedding).  The sums are the same as the dense exchange's (order of float additions aside).
    """

    def __init__(self, reducer, weight):
        self.red = reducer
        self.weight = weight
        V, D = weight.shape
        self.V, self.D = V, D
        dev = weight.device
        self.cuda = weight.is_cuda
        self.gworld = dist.get_world_size(reducer.group)
        # persistent buffers (allocated on the compute stream's pool, used on both streams under events)
        self.buf = torch.zeros(V * D, device=dev, dtype=weight.dtype)
        self.mark = torch.zeros(V, device=dev, dtype=torch.int64)
        self.csum = torch.zeros(V, device=dev, dtype=torch.int64)
        self.slot_of_vocab = torch.full((V,), -1, device=dev, dtype=torch.int64)
        self.slots = self.allids = None
        self.count_host = torch.zeros(1, dtype=torch.int64, pin_memory=self.cuda)
        self.event = torch.cuda.Event() if self.cuda else None
        self.ids = None
        self.U = 0
        self.used = False

    def begin(self, ids):
        """Step start: agree on the compact row numbering of this step's global batch."""
        red = self.red
        self.ids, self.used, self.U = ids, False, 0
        n = ids.numel()
        if self.slots is None or self.slots.numel() != n:
            self.slots = torch.empty(n, device=ids.device, dtype=torch.int64)
            self.allids = torch.empty(self.gworld * n, device=ids.device, dtype=torch.int64)
        if self.cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            red.comm_stream.wait_event(ev)
            ctx = torch.cuda.stream(red.comm_stream)
        else:
            ctx = contextlib.nullcontext()
        with ctx:
            mine = ids.reshape(-1).clamp(0, self.V - 1)
            red._check_agreement(mine, "all-gather of the step's token ids")
            if self.cuda and not red.stream_ordered:
                # a host-staged transport (gloo: the one-GPU rehearsals) is handed HOST tensors.  c10d's own staging of device
                # tensors copies the result back on a stream of its own, and with 4 ranks sharing a GPU the numbering below read
                # `allids` while that copy was still landing in 1 of ~30 steps -- the ranks then disagreed on U and the compact
                # all-reduce died with a size mismatch (round 5: 4-8 of 16 `bench.py --gpus 4 --backend gloo` runs; 0 of 16 since).
                # Neither wait() on an explicit work object nor a device-wide synchronisation behind it closed the window.
                host = torch.empty(self.allids.numel(), dtype=torch.int64)
                dist.all_gather_into_tensor(host, mine.cpu(), group=red.group)
                self.allids.copy_(host)
            else:  # RCCL: ordered on this stream by construction
                dist.all_gather_into_tensor(self.allids, mine, group=red.group)
            self.mark.zero_()
            self.mark.index_fill_(0, self.allids, 1)
            torch.cumsum(self.mark, 0, out=self.csum)
            self.slot_of_vocab.copy_(self.csum).sub_(1)
            self.slot_of_vocab.masked_fill_(self.mark == 0, -1)
            torch.index_select(self.slot_of_vocab, 0, mine, out=self.slots)
            self.count_host.copy_(self.csum[-1:], non_blocking=True)
            if self.cuda:
                self.event.record(red.comm_stream)

    def sink(self, weight, ids):
        """ops.set_embed_grad_sink callback (runs inside backward, at the embedding's node)."""
        if weight is not self.weight or self.ids is None or self.used or ids.data_ptr() != self.ids.data_ptr() \
                or ids.shape != self.ids.shape:
            return None
        self.used = True
        if self.cuda:
            self.event.synchronize()  # the host needs U; the GPU passed this point at the start of the step
            torch.cuda.current_stream().wait_event(self.event)
        self.U = int(self.count_host.item())
        view = self.buf[: self.U * self.D]
        view.zero_()
        return view, self.slots.view(ids.shape), self.U, self._done

    def _done(self):
        self.red._all_reduce(self.buf[: self.U * self.D], "compact embedding rows (U = %d)" % self.U)

    def apply(self):
        """After the exchange: flat gradient rows += compact rows."""
        if not self.used or self.U == 0:
            self.ids = None
            return
        g = self.weight.grad
        src = self.buf[: self.U * self.D].view(self.U, self.D)
        if self.cuda:
            ops.rows_gather_add(g, self.slot_of_vocab, src, self.U)
        else:
            rows = torch.nonzero(self.slot_of_vocab >= 0).reshape(-1)
            g.index_add_(0, rows, src[self.slot_of_vocab[rows]])
        self.ids = None


class Trainer:
    """One optimisation step = forward + CE + KL*seq_len/len(train_data) + backward + (all-reduce)
    + clip + SGD, as train.py:315-420 does, for any of the model families."""

    def __init__(self, model, lr, clip, momentum=0.9, kl_scale=0.0, seed=1111, rank=0, world=1, global_batch=None,
                 bucket_bytes=32 << 20, fused_kl=True, weight_decay=0.0, overlap=True, late_rows=True, comm_cus=None,
                 collective=None, comm_plan=None, comm_gbps=None):
        self.model = model
        self.lr, self.clip, self.momentum = lr, clip, momentum
        self.weight_decay = weight_decay  # torch.optim.SGD(weight_decay=...) of train_search_bayes.py:391-392
        self.kl_scale = kl_scale
        self.rank, self.world = rank, world
        self.flat = FlatBuffers(model)
        if comm_cus is None:  # RCCL: one channel workgroup per channel (pin_rccl_channels); gloo moves bytes on the host
            comm_cus = rccl_channels() if (world > 1 and dist.is_initialized() and dist.get_backend() == "nccl") else 0
        self.reducer = GradReducer(self.flat, bucket_bytes, overlap=overlap, comm_cus=comm_cus if overlap else 0,
                                   collective=collective, comm_plan=comm_plan, comm_gbps=comm_gbps)
        hooked = world > 1 or collective is not None
        ops.set_grad_ready_hook(self.reducer.mark_ready if hooked else None)
        ops.set_embed_grad_sink(None)
        if hooked:
            self.reducer.hook_autograd()
            enc = getattr(getattr(model, "encoder", None), "weight", None)
            if late_rows and enc is not None and any(enc is p for p in self.flat.params) and dist.is_initialized():
                self.reducer.late = LateRows(self.reducer, enc)
                ops.set_embed_grad_sink(self.reducer.late.sink)
        self.table = ops.PtrTable([self.flat.flat_param], [self.flat.flat_grad], [self.flat.flat_mom])
        self.step_no = 0
        self.first = True
        model.set_seed(seed)
        self.fused_kl = fused_kl
        self.kl_layers = self._find_kl_layers()
        self.last_soft = None  # SoftStats of device scalars: the last distillation step's mean nll, soft loss and KL (step(soft=...))
        self.sampler = None  # sgmcmc.Sampler: its update takes the place of clip + SGD (set_sampler)

    def set_sampler(self, sampler):
        """SG-MCMC: from the next step on ``sampler.update(self)`` (sgmcmc.Sampler: blm_sqnorm_multi + blm_sgmcmc_update, noise of
        step = step_no) takes the place of ops.clip_sgd; None: clip + SGD again, its momentum buffer starting from zero.  Single
        process only."""
        if sampler is not None and self.world > 1:
            raise ops.BayesLMError("Trainer.set_sampler: world size %d: data-parallel sampling is not built" % self.world)
        if sampler is not None:
            sampler.begin(self)
        self.sampler = sampler
        self.first = True

    def _find_kl_layers(self):
        from .model import BayesLinear
        return [m for m in self.model.modules() if isinstance(m, BayesLinear)]

    def reset_optimizer(self, lr):
        """train.py:503-505: LR halving re-creates SGD, i.e. the momentum buffers start from zero."""
        self.lr = lr
        self.first = True

    def step(self, data, targets, hidden=None, kl_fn=None, philox_step=None, soft=None):
        """-> (loss tensor, kl tensor, new hidden).  ``kl_fn(model)`` returns the KL term train.py
        would add for this configuration (train.py:335-399), or None.  ``philox_step`` overrides the
        noise / dropout stream index (default: the optimisation step count).  ``soft`` = (teacher_logp, weight): distillation --
        ops.cross_entropy_soft against the teacher's (T * B, V) log-probabilities takes the place of the hard-label cross entropy
        (weight 0 is that loss), everything else is the same step; the step's mean hard NLL, soft loss and KL(teacher || student)
        stay on the device as ``self.last_soft``.  ``soft`` = (ops.SparseTargets, weight): the same against the teacher's K best
        entries per token (ops.cross_entropy_soft_topk).  ``soft`` = (targets, weight, temperature): the soft term at that softmax
        temperature T, times T ** 2 (the ops' ``temperature`` keyword); ``last_soft`` then holds the soft loss and the KL at
        temperature, without that factor.  Single process only."""
        if soft is not None and self.world > 1:
            raise ops.BayesLMError("Trainer.step: soft targets with world = %d: data-parallel distillation is not built (the teacher's "
                                   "rows would have to follow each rank's batch columns); train the student in one process" % self.world)
        m = self.model
        m.train()
        m.set_step(self.step_no if philox_step is None else philox_step)
        B = data.shape[1]
        m.set_columns(self.rank * B, self.world * B)
        self.flat.zero_grad()
        if self.reducer.late is not None:
            self.reducer.late.begin(data)
        fused = self.fused_kl and kl_fn is not None and len(self.kl_layers) > 0 and getattr(kl_fn, "fusable", False)
        for lyr in self.kl_layers:
            lyr.fused_kl_lambda = self.kl_scale if fused else 0.0
        if hidden is None:
            out = m(data)
        else:
            out, hidden = m(data, hidden)
        V = out.shape[-1]
        if soft is None:
            mle, _ = ops.cross_entropy(out.view(-1, V), targets, unit_grad=True)
        else:
            soft_loss = ops.cross_entropy_soft_topk if isinstance(soft[0], ops.SparseTargets) else ops.cross_entropy_soft
            mle, parts = soft_loss(out.view(-1, V), targets, soft[0], soft[1], unit_grad=True, temperature=soft[2] if len(soft) > 2 else 1.0)
            self.last_soft = ops.SoftStats(parts.nll.mean(), parts.soft.mean(), parts.kl.mean())  # no host synchronisation
        kl = None
        if kl_fn is not None:
            kl = kl_fn(m) * self.kl_scale
        if kl is None or fused:
            loss = mle + kl.detach() if kl is not None else mle
            mle.backward()
        else:
            loss = mle + kl
            loss.backward()
        self.reducer.finish()
        if self.sampler is None:
            ops.clip_sgd(self.table, self.clip, self.lr, self.momentum, self.first, 1.0 / self.world, self.weight_decay)
        else:
            self.sampler.update(self)
        self.first = False
        self.step_no += 1
        return loss.detach(), (kl.detach() if kl is not None else None), hidden


def evaluate(model, source, seq_len, eval_batch_size=None, rank=0, world=1, group=None):
    """Eval-mode loss per token exactly as train.py:441-458 sums it.  Data parallel (``world`` > 1): the columns of the
    evaluation batch are independent streams (batchify, train.py:167-179; an LSTM's carried state is per column), so rank r
    evaluates columns [r C / W, (r + 1) C / W) and the token-weighted sums meet in one 8-byte all-reduce -- the reference's
    single process walks the whole stream, and with W ranks doing that each the validation pass would be the part of an epoch
    that does not scale (it is ~1 % of a one-GPU epoch of the AMI recipe, ~10 % of an 8-GPU one).  Every rank returns the
    same value up to the all-reduce (callers that branch on it take rank 0's: train.ValidationSchedule)."""
    from .model import CarriedState, inference_decoder
    model.eval()
    cols = source.shape[1]
    lo, hi = (rank * cols) // world, ((rank + 1) * cols) // world
    mine = source if world == 1 else source[:, lo:hi].contiguous()
    total = torch.zeros((), device=source.device, dtype=torch.float64)
    # the decoder returns the per-token NLL itself when it can (ops.linear_nll: the (T*B, V) logits are never stored);
    # BLM_EVAL_FUSED_NLL=0 keeps decoder + cross-entropy kernel
    dec = inference_decoder(model)
    fused = (os.environ.get("BLM_EVAL_FUSED_NLL", "1") != "0" and dec is not None
             and ops.linear_nll_supported(dec.weight, dec.bias))
    # The windows come in groups (_eval_windows).  total = sum over windows of len * mean is unchanged up to the order of the
    # additions: the windows of a group are equally sized, so sum_k len * mean_k = G len * mean of all.
    with torch.no_grad(), (dec.inference() if fused else contextlib.nullcontext()):
        if hi > lo:  # else more ranks than columns: nothing of this stream is mine
            state = CarriedState(model, hi - lo)
            for data, targets, starts, n in _eval_windows(mine, seq_len, state.hidden is not None):
                if fused:
                    dec.set_nll_targets(targets)
                out = state(data)
                loss = out.mean() if fused else ops.cross_entropy(out.view(-1, out.shape[-1]), targets)[0]
                total += (len(starts) * n) * loss.double()
    if world > 1:  # sum_r (columns of r) * (its per-window means, summed) / all columns = the whole batch's per-window means, summed
        total = total * float(hi - lo) / float(cols)
        on_dev = dist.get_backend(group) == "nccl"
        t = total.reshape(1) if on_dev else total.reshape(1).cpu()
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        total = t[0]
    return float(total.item()) / (len(source) - 1)


def perplexity(loss):
    return math.exp(loss)


# ----------------------------------------------------------------------------
# evaluation report: model-average perplexity and calibration
# ----------------------------------------------------------------------------
# Hidden rows per decoder launch of evaluate_report: the chunk's logits (mean weights) or log pbar (Monte-Carlo) are the only
# (rows, V) matrix alive at a time -- 270 MB at V 33,000.  The value is unmeasured (tools/eval_report_probe.py times the call,
# not this constant).
_REPORT_ROWS = 2048


@dataclasses.dataclass
class EvalReport:
    """What evaluate_report returns; ``as_dict()`` is what the command lines write as JSON.  Fields that a run does not produce
    are None: the calibration block without a stored distribution (Monte-Carlo with calibration=False), the Monte-Carlo block
    at mean weights."""
    tokens: int                       # tokens that entered the figures
    skipped: int                      # tokens whose target is outside [0, V): left out of everything, as the cross entropy leaves them out
    loss: float                       # mean NLL, nats; under Monte-Carlo of the per-token model average pbar
    ppl: float
    mc_samples: int = 0
    accuracy: Optional[float] = None       # share of tokens whose target is the prediction (rank 0)
    top5_accuracy: Optional[float] = None  # ... is among the five best (rank < 5)
    mean_conf: Optional[float] = None      # mean largest probability
    mean_entropy: Optional[float] = None   # mean entropy of the distribution the token was scored with, nats
    ece: Optional[float] = None            # expected calibration error over `bins`
    bins: Optional[list] = None            # [count, mean_conf, accuracy] per equal-width confidence bin (zeros in an empty bin)
    sample_loss: Optional[list] = None     # (S) each weight sample's own mean NLL
    sample_loss_mean: Optional[float] = None
    mean_h_pred: Optional[float] = None    # mean predictive entropy H[pbar]
    mean_mi: Optional[float] = None        # mean mutual information between the word and the weights
    per_token: Optional[dict] = None       # keep_tokens: float / int arrays in text order, skipped tokens included (NaN / -1)
    swag: Optional[dict] = None            # SWAG (SwagPosterior.describe with scale, diag, samples, seed, path); None: the model's own weights
    samples: Optional[dict] = None         # a bank of weight vectors (SampleBank.describe: SG-MCMC samples or an ensemble); None: none
    laplace: Optional[dict] = None         # last-layer Laplace (LaplacePosterior.describe with prior, link, samples, seed); None: none
    cache: Optional[dict] = None           # neural cache (CacheReport.as_dict, with the fit's block after fit_cache); None: no cache
    dyneval: Optional[dict] = None         # dynamic evaluation (DynEvalReport.as_dict beside the static loss, with the fit's block); None: none
    temperature: Optional[dict] = None     # temperature scaling (temperature_block); None: the distribution as the model gives it

    def as_dict(self):
        d = dataclasses.asdict(self)
        del d["per_token"]
        for k in ("temperature", "cache", "dyneval", "swag", "laplace", "samples"):  # a run without one writes what it wrote before there was one
            if d[k] is None:
                del d[k]
        return d


def report_from_tokens(nll, conf=None, entropy=None, rank=None, valid=None, bins=15, nll_s=None, h_pred=None, mi=None):
    """The figures of an EvalReport from per-token arrays (host code; numpy or anything numpy converts): every sum in float64.
    ``valid`` (bool per token, default all): the tokens that count; the others are ``skipped``.  ``rank`` is blm_row_stats':
    entries ahead of the target.  Calibration needs ``conf`` and ``rank``: B = ``bins`` equal-width confidence bins, a token
    falls into bin min(B - 1, floor(conf B)) (conf = 1 into the last one), ece = sum_b n_b / N |accuracy_b - mean_conf_b|.
    ``nll_s`` (tokens, S), ``h_pred`` and ``mi`` make the Monte-Carlo block."""
    nll = np.asarray(nll, dtype=np.float64).reshape(-1)
    ok = np.ones(nll.shape[0], dtype=bool) if valid is None else np.asarray(valid, dtype=bool).reshape(-1)
    n = int(ok.sum())
    B = int(bins)
    if B < 1:
        raise ops.BayesLMError("report_from_tokens: bins must be positive, got %d" % B)

    def mean(a):
        return float(np.asarray(a, dtype=np.float64).reshape(-1)[ok].sum() / n) if n else float("nan")

    loss = mean(nll)
    rep = EvalReport(tokens=n, skipped=int(ok.shape[0] - n), loss=loss, ppl=math.exp(min(loss, 700.0)) if loss == loss else loss)
    if conf is not None:
        rep.mean_conf = mean(conf)
    if entropy is not None:
        rep.mean_entropy = mean(entropy)
    if rank is not None:
        r = np.asarray(rank).reshape(-1)[ok]
        rep.accuracy = float((r == 0).sum() / n) if n else float("nan")
        rep.top5_accuracy = float(((r >= 0) & (r < 5)).sum() / n) if n else float("nan")
    if conf is not None and rank is not None:
        c = np.asarray(conf, dtype=np.float64).reshape(-1)[ok]
        hit = (np.asarray(rank).reshape(-1)[ok] == 0).astype(np.float64)
        idx = np.clip(np.floor(np.nan_to_num(c) * B), 0, B - 1).astype(np.int64)
        cnt = np.bincount(idx, minlength=B)
        csum, hsum = np.bincount(idx, weights=c, minlength=B), np.bincount(idx, weights=hit, minlength=B)
        safe = np.maximum(cnt, 1)
        mconf, acc = csum / safe, hsum / safe
        rep.ece = float((cnt / n * np.abs(acc - mconf)).sum()) if n else float("nan")
        rep.bins = [[int(cnt[b]), float(mconf[b]), float(acc[b])] for b in range(B)]
    if nll_s is not None:
        s = np.asarray(nll_s, dtype=np.float64)
        s = s.reshape(nll.shape[0], -1)[ok]
        rep.mc_samples = int(s.shape[1])
        rep.sample_loss = [float(v) for v in (s.sum(0) / n)] if n else [float("nan")] * s.shape[1]
        rep.sample_loss_mean = float(np.mean(rep.sample_loss))
    if h_pred is not None:
        rep.mean_h_pred = mean(h_pred)
    if mi is not None:
        rep.mean_mi = mean(mi)
    return rep


def _eval_windows(source, seq_len, recurrent, group=True, limit=None, who="evaluate"):
    """The batches every evaluation walk forms from the batchified stream ``source``, in order -> (data, flat targets, starts,
    rows): ``data`` lays the windows that begin at the rows ``starts`` side by side, ``rows`` rows each (_window_positions
    places the targets in the text; ``len(starts) * rows`` is the batch's weight in a sum of per-window means).

    A model without carried state (the Transformers) sees every window on its own: G full windows are evaluated as ONE batch of
    G x columns independent columns (same positions, same causal mask per column) -- the reference's eval batch of 10-20 columns
    gives the matrix cores 1280-2560 rows per product, G of them ~16384 (headline model, 12 windows of 20 x 128: 1.085 M tokens/s
    window by window, 1.178 M in threes, 1.197 M in sixes, tools/eval_windows_probe.py).  The ragged last window goes alone.
    A recurrent model carries its state from window to window, so G consecutive windows ARE one window of G seq_len steps: the
    same recurrence step for step, with the input / decoder products over G times the rows (the LSTM language models' evaluation
    batch gives them 700 rows per window; the time loop is issued step by step, three windows of 700 rows pay, more do not) and
    the layer wavefront over a longer stretch (configs[1]'s model, 12 windows of 20 x 35: 668 k tokens/s window by window, 765 k
    in threes; no better and host-bound beyond).  BLM_EVAL_WINDOWS=G overrides G; 1 walks the windows one by one as
    train.py:441-458 does.

    ``group`` False is dynamic evaluation's plan: one window of ``seq_len`` rows at a time whatever the model and the
    environment say, the first ``limit`` of them (None: all), refusing under the name ``who`` a stream without a target."""
    from .data import get_batch
    if not group:
        if int(seq_len) < 1:
            raise ops.BayesLMError("%s: seq_len = %r" % (who, seq_len))
        if source.dim() != 2 or source.shape[0] < 2:
            raise ops.BayesLMError("%s: the stream holds %s rows: two are the least that give a target" % (who, tuple(source.shape)))
        seq_len = int(seq_len)
    nrows, cols = source.shape
    n_full = max(0, (nrows - 1) // seq_len)  # windows of exactly seq_len rows
    n_win = 1
    if group:
        budget = 2400 if recurrent else 16384
        n_win = int(os.environ.get("BLM_EVAL_WINDOWS", "0")) or max(1, min(max(n_full, 1), budget // max(1, seq_len * cols)))
    stride = seq_len * (n_win if recurrent else 1)

    def plan():
        i, left = 0, n_full
        while not recurrent and n_win > 1 and left > 1:
            g = min(n_win, left)
            starts = range(i, i + g * seq_len, seq_len)
            data = torch.cat([source[k:k + seq_len] for k in starts], 1)
            targets = torch.cat([source[k + 1:k + 1 + seq_len] for k in starts], 1).reshape(-1)
            yield data, targets, starts, seq_len
            i, left = i + g * seq_len, left - g
        for i in range(i, nrows - 1, stride):
            data, targets = get_batch(source, i, stride)
            yield data, targets, (i,), len(data)

    return itertools.islice(plan(), limit)


def _window_positions(shape, starts, rows):
    """Text position of every target of one batch of _eval_windows over a stream of ``shape`` = (nrows, columns), flat in the
    targets' order: column c of the batchified stream holds the tokens c * nrows .. (c + 1) * nrows - 1 of the text, so target
    r of the window that begins at row ``start`` is token start + 1 + r + c * nrows in column c."""
    nrows, cols = shape
    col0 = np.arange(cols, dtype=np.int64) * nrows
    return np.concatenate([np.arange(start + 1, start + 1 + rows, dtype=np.int64)[:, None] + col0[None, :] for start in starts],
                          1).reshape(-1)


def temperature_block(beta, fitted_on=None, at_bound=False, before=None, after=None, curve=None):
    """EvalReport.temperature: the scaling a report was made with -- T, beta = 1 / T as the kernel got it (float32), and, after a
    fit, the text it was fitted on, whether it ended at a bound of the search, the FIT text's loss and ECE at T = 1 and at T, and
    the curve of fit_temperature."""
    beta = float(beta)
    return {"temperature": 1.0 / beta, "beta": beta, "fitted_on": fitted_on, "at_bound": bool(at_bound),
            "loss_before": None if before is None else before.loss, "loss_after": None if after is None else after.loss,
            "ece_before": None if before is None else before.ece, "ece_after": None if after is None else after.ece,
            "curve": curve}


def _report_walk(who, model, source, seq_len, mc_samples, seed, calibration, betas, rows_out=None, chunks=None):
    """The walk evaluate_report, evaluate_temperatures and the neural cache share -> (host arrays in walk order, the (starts,
    rows) of every batch for _text_order, V, S).
    ``rows_out`` (mean weights only): a callable that is handed every window's decoder-input rows (rows, K), in the order of the
    targets, before the next window runs (the neural cache keeps them on the device).
    ``chunks`` (mean weights only): a callable (rows, targets) that takes the place of the row reduction for every window (the
    Laplace walks form their own products from the rows); the host arrays are then None.
    ``betas`` None: blm_row_stats reduces each chunk and the float arrays are (tokens,).  A list of J float32 inverse
    temperatures: blm_row_stats_temps reduces it, and nll, conf, entropy and dnll are (J, tokens), those of the tempered
    distributions; nll_s, h_pred and mi stay the untempered (tokens, ...) quantities of ops.linear_mc_logprobs."""
    from . import incremental
    from .model import CarriedState, inference_decoder, mc_sampling
    S = int(mc_samples)
    model.eval()
    if dist.is_initialized() and dist.get_world_size() > 1:
        raise ops.BayesLMError("%s runs in a single process (world size %d): sharding the report over ranks is not "
                               "built; call it on one rank" % (who, dist.get_world_size()))
    if S < 0 or S == 1 or S > 64:
        raise ops.BayesLMError("%s: mc_samples must be 0 (mean weights) or 2..64, got %d: one sample is neither the "
                               "mean-weight model nor an average, and blm_linear_mc_logprobs / blm_linear_mc_stats take at most 64 "
                               "samples per launch" % (who, S))
    if betas is not None and S and not calibration:
        raise ops.BayesLMError("%s: a temperature with mc_samples = %d and calibration=False: that path stores no row of width V, "
                               "so there is nothing to temper" % (who, S))
    dec = inference_decoder(model)
    if dec is None:
        raise ops.BayesLMError("%s: %s has no decoder that hands back its input rows" % (who, type(model).__name__))
    recurrent = hasattr(model, "init_hidden")
    if S and recurrent:
        cell = incremental._redraws_per_time_step(model)
        if cell:
            raise ops.BayesLMError("%s: mc_samples on %s: %s draws fresh noise at every time step of a call, so a "
                                   "sample is not one model over a stream" % (who, type(model).__name__, cell))
    V = dec.weight.shape[0]
    keep = {k: [] for k in ("tgt", "nll", "conf", "entropy", "dnll", "pred", "rank", "nll_s", "h_pred", "mi")}
    placed = []

    def row_stats(x, t):
        return ops.row_stats(x, t, V) if betas is None else ops.row_stats_temps(x, betas, t, V)

    def reduce_rows(x, targets):
        """x: (rows, K) at mean weights, (S, rows, K) under Monte-Carlo"""
        for a in range(0, targets.numel(), _REPORT_ROWS):
            t = targets[a:a + _REPORT_ROWS]
            if S == 0:
                st = row_stats(ops.linear(x[a:a + _REPORT_ROWS], dec.weight, dec.bias), t)
            elif calibration:
                mc = ops.linear_mc_logprobs(x[:, a:a + _REPORT_ROWS], dec.weight, dec.bias, tgt=t, dec=mc_dec, stats=True)
                st = row_stats(mc.logp, t)
            else:
                mc, st = ops.linear_mc_stats(x[:, a:a + _REPORT_ROWS], dec.weight, dec.bias, t, dec=mc_dec), None
            if S:
                keep["nll"].append(mc.bma_nll if betas is None else st.nll)
                keep["nll_s"].append(mc.nll_s)
                keep["h_pred"].append(mc.h_pred)
                keep["mi"].append(mc.mi)
            else:
                keep["nll"].append(st.nll)
            if st is not None:
                keep["conf"].append(st.conf)
                keep["entropy"].append(st.entropy)
                keep["pred"].append(st.pred)
                keep["rank"].append(st.rank)
                if betas is not None:
                    keep["dnll"].append(st.dnll)

    with torch.no_grad(), dec.inference(input_rows=True), (mc_sampling(model, seed, S) if S else contextlib.nullcontext()):
        mc_dec = ops.McDecoder(dec.weight, dec.bias) if S else None  # the vocabulary padded once for the run
        state = CarriedState(model, source.shape[1], max(S, 1))
        for data, targets, starts, n in _eval_windows(source, seq_len, recurrent):
            if S == 0:
                x = state(data)
                x = x.reshape(-1, x.shape[-1])
                if chunks is None:
                    reduce_rows(x, targets)
                else:
                    chunks(x, targets)
                if rows_out is not None:
                    rows_out(x)
            else:
                xs = []
                for s in range(S):
                    model.set_step(s)
                    x = state(data, s)
                    xs.append(x.reshape(-1, x.shape[-1]))
                reduce_rows(torch.stack(xs), targets)
            keep["tgt"].append(targets)
            placed.append((starts, n))
    if chunks is not None:
        return None, placed, V, S
    empty = ("nll",) if betas is None else ("nll", "conf", "entropy", "dnll", "pred", "rank")
    return _tokens_to_host(keep, None if betas is None else len(betas), empty), placed, V, S


_TEMPERED = ("nll", "conf", "entropy", "dnll")  # the fields that are (J, tokens) under J inverse temperatures


def _tokens_to_host(keep, temps=None, empty=("nll",), samples=0):
    """The per-window device arrays a walk kept, by field -> one host array per field, in walk order.  The float32 fields come
    in ONE copy, stacked as rows, ``pred`` and ``rank`` in another.  ``temps`` J: the walk reduced its chunks for J inverse
    temperatures, the _TEMPERED fields are (J, tokens) and take J rows each.  A text without a token gives the fields ``empty``
    (and ``tgt``) as typed arrays of no token, ``nll_s`` with ``samples`` columns."""
    n_tok = sum(t.numel() for t in keep["tgt"])
    if not n_tok:
        host = {k: np.zeros((temps, 0) if temps is not None and k in _TEMPERED else 0, np.float32) for k in empty}
        host.update({k: np.zeros(0, np.int32) for k in ("pred", "rank") if k in empty}, tgt=np.zeros(0, np.int64))
        if "nll_s" in empty:
            host["nll_s"] = np.zeros((0, samples), np.float32)
        return host
    fl = [k for k in ("nll", "conf", "entropy", "dnll", "h_pred", "mi") if keep.get(k)]
    rows = [torch.cat(keep[k], -1).reshape(-1, n_tok) for k in fl]
    packed, at, host = torch.cat(rows).cpu().numpy(), 0, {}
    for k, r in zip(fl, rows):
        host[k] = packed[at:at + r.shape[0]] if (temps is not None and k in _TEMPERED) else packed[at]
        at += r.shape[0]
    host["tgt"] = torch.cat(keep["tgt"]).cpu().numpy()
    if keep.get("rank"):
        host["pred"], host["rank"] = torch.stack([torch.cat(keep["pred"]), torch.cat(keep["rank"])]).cpu().numpy()
    if keep.get("nll_s"):
        host["nll_s"] = torch.cat(keep["nll_s"]).cpu().numpy()
    return host


def _text_order(shape, placed):
    """The permutation that puts a walk's tokens in text order; ``placed``: the (starts, rows) of its batches, in order"""
    if not placed:
        return np.zeros(0, np.int64)
    return np.argsort(np.concatenate([_window_positions(shape, starts, n) for starts, n in placed]), kind="stable")


def _betas_of(who, temperature):
    """``temperature`` T as a report takes it -> None at exactly 1.0 (the untempered kernels run), else [float32(1 / T)]"""
    if _float32_beta(who, temperature, "temperature") and float(temperature) != 1.0:
        return [_float32_beta(who, 1.0 / float(temperature), "1 / temperature")]
    return None


def _report_of(host, V, S, bins, betas=None, row=0, order=None):
    """EvalReport from the host arrays of a walk (_tokens_to_host).  ``betas``: the walk's inverse temperatures, of which the
    report is that of ``betas[row]``, row ``row`` of the (J, tokens) fields; ``order`` (_text_order) asks for ``per_token``."""
    if betas is not None:
        host = {k: (v[row] if k in _TEMPERED else v) for k, v in host.items()}
    valid = (host["tgt"] >= 0) & (host["tgt"] < V)
    rep = report_from_tokens(host["nll"], host.get("conf"), host.get("entropy"), host.get("rank"), valid, bins,
                             host.get("nll_s"), host.get("h_pred"), host.get("mi"))
    rep.mc_samples = S
    if betas is not None:
        rep.temperature = temperature_block(betas[row])
    if order is not None:
        rep.per_token = {k: v[order] for k, v in host.items()}
    return rep


def _float32_beta(who, value, name):
    """``value`` as the float32 inverse temperature the kernel is given; refuses what is not positive and finite."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    with np.errstate(over="ignore"):  # a value past float32 becomes inf and is refused below
        b = float(np.float32(v)) if math.isfinite(v) else v
    if not (math.isfinite(v) and v > 0.0 and math.isfinite(b) and b > 0.0):
        raise ops.BayesLMError("%s: %s = %r is not a positive finite number (in float32)" % (who, name, value))
    return b


def evaluate_report(model, source, seq_len, eval_batch_size=None, mc_samples=0, seed=1111, bins=15, calibration=True,
                    keep_tokens=False, temperature=1.0):
    """Held-out loss / perplexity, accuracy and calibration of ``model`` over the batchified stream ``source``, at mean weights
    (``mc_samples`` 0) or under the average of S = ``mc_samples`` >= 2 Monte-Carlo weight samples -> EvalReport.

    The walk is engine.evaluate's (same windows, same grouping: _eval_windows) with the decoder handing back its input rows;
    those go through the decoder in chunks of _REPORT_ROWS rows and blm_row_stats reduces each chunk's (rows, V) matrix to
    per-token NLL, confidence, entropy, prediction and rank in one read.  The per-token float32 arrays stay on the device
    until the walk is over, come to the host in one copy, and every sum is formed there in float64 (report_from_tokens).

    mc_samples = S: S passes per batch in the n-best scorer's sampling state (model.mc_sampling(model, seed, S), sample s
    selected with set_step(s)): sample s is ONE model for the whole text, and a recurrent model carries S (h, c) sets from window
    to window.  The model average is taken PER TOKEN, pbar(w | history) = mean_s p_s(w | history) -- a normalised distribution
    over word sequences, whose NLL is ``loss`` -- not the scorer's sentence-level -log mean_s exp(-NLL_s(sentence)).  One launch
    per chunk keeps log pbar with nll_s, bma_nll, h_pred and mi (ops.linear_mc_logprobs), and blm_row_stats reads log pbar.
    ``calibration`` False under Monte-Carlo: ops.linear_mc_stats instead -- nothing of width V is stored, and the report has no
    accuracy / confidence / calibration block (at mean weights the chunk's logits exist either way and the flag changes nothing).

    ``temperature`` T: exactly 1.0 launches what is described above.  Any other positive finite T sends each chunk through
    blm_row_stats_temps with beta = float32(1 / T) instead, and loss, ppl, mean_conf, mean_entropy, ece and bins are those of the
    tempered distribution p_beta ~ exp(beta x) -- for a model average pbar^beta / Z, one parameter on top of the average; under
    Monte-Carlo ``loss`` is then the kernel's tempered NLL of log pbar, not bma_nll.  accuracy and top5_accuracy do not depend on
    T; sample_loss*, mean_h_pred and mean_mi stay the UNTEMPERED quantities of ops.linear_mc_logprobs.  The report's
    ``temperature`` block (temperature_block) names T and beta.

    Refused: mc_samples 1; a model without variational sites or with local reparameterisation (mc_sampling's refusals); cells that
    redraw noise at every time step of a call (as IncrementalLM refuses them); a temperature that is not positive and finite, and
    one other than 1.0 with mc_samples > 0 and calibration=False, where no row of width V exists.  ``eval_batch_size`` is accepted
    for symmetry with the reference's evaluate and unused, like there.  Single process only.  The model is left in eval mode with
    the caller's noise (seed, step, auto_step)."""
    betas = _betas_of("evaluate_report", temperature)
    host, placed, V, S = _report_walk("evaluate_report", model, source, seq_len, mc_samples, seed, calibration, betas)
    order = _text_order(source.shape, placed) if keep_tokens else None
    return _report_of(host, V, S, bins, betas, order=order)


def evaluate_temperatures(model, source, seq_len, betas, mc_samples=0, seed=1111, bins=15):
    """evaluate_report at the 1..8 inverse temperatures ``betas`` (beta = 1 / T, each rounded to float32) from ONE walk of the
    text -> (one EvalReport per beta, the mean d nll / d beta per beta).  blm_row_stats_temps reduces each chunk's (rows, V)
    matrix for every beta in the same single read; windows, chunks, the single host copy and the float64 sums are
    evaluate_report's, and so are its refusals and what stays untempered under Monte-Carlo.  The report of beta is what
    evaluate_report(temperature=1 / beta) returns (at beta = 1 too: here that entry goes through the same kernel as the others).
    The summed NLL is convex in beta, so the second result changes sign at most once: TemperatureSearch rests on that."""
    try:
        betas = list(betas)
    except TypeError:
        raise ops.BayesLMError("evaluate_temperatures: betas must be 1..8 positive finite numbers, got %r" % (betas,))
    if not 1 <= len(betas) <= 8:
        raise ops.BayesLMError("evaluate_temperatures: %d inverse temperatures, one walk takes 1..8" % len(betas))
    bs = [_float32_beta("evaluate_temperatures", b, "betas[%d]" % j) for j, b in enumerate(betas)]
    host, _, V, S = _report_walk("evaluate_temperatures", model, source, seq_len, mc_samples, seed, True, bs)
    valid = (host["tgt"] >= 0) & (host["tgt"] < V)
    n = int(valid.sum())
    reps, dloss = [], []
    for j in range(len(bs)):
        reps.append(_report_of(host, V, S, bins, bs, j))
        dloss.append(float(host["dnll"][j].astype(np.float64)[valid].sum() / n) if n else float("nan"))
    return reps, dloss


class TemperatureSearch:
    """Host-side search for the inverse temperature that minimises a held-out NLL, from its value and slope on grids of
    ``points`` betas (one walk of the text each: evaluate_temperatures).  The NLL is convex in beta, so its slope changes sign
    at most once, from - to +; the search keeps the bracket [a, b] with slope(a) < 0 < slope(b).

        grid()     the next betas (float32 values): geometric over [1/8, 8] (cut to [lo, hi]) the first time, then geometric
                   over the bracket, ends included -- each pass divides the bracket's log-width by points - 1.  While the
                   slope has one sign on everything seen, the grid spans from the last end to the bound on that side.
        update()   takes the betas, their mean NLL and mean slope; a non-finite one raises, naming beta.
        result()   beta: the root of the secant through the bracket's two slopes; the bound with ``at_bound`` set once the
                   slope at lo is still > 0 or at hi still < 0; before that the seen beta whose slope is nearest 0.
        bracket    (a, b): what is known to hold the minimiser within [lo, hi]; nested from one update to the next."""

    def __init__(self, lo=1.0 / 16, hi=16.0, points=8):
        self.lo, self.hi, self.points = float(np.float32(lo)), float(np.float32(hi)), int(points)  # betas are float32 values
        if not (0.0 < self.lo < self.hi < math.inf):
            raise ops.BayesLMError("TemperatureSearch: need 0 < lo < hi < inf, got lo = %r, hi = %r" % (lo, hi))
        if not 2 <= self.points <= 8:
            raise ops.BayesLMError("TemperatureSearch: points = %r outside 2..8, what one walk evaluates" % (points,))
        self.seen = {}  # beta -> (loss, dloss)
        self.at_bound = False

    def _ends(self):
        """(a, b): the greatest seen beta with slope < 0 and the least with slope > 0 (None: none yet)"""
        neg = [b for b, (_, d) in self.seen.items() if d < 0]
        pos = [b for b, (_, d) in self.seen.items() if d >= 0]
        return (max(neg) if neg else None), (min(pos) if pos else None)

    @property
    def bracket(self):
        a, b = self._ends()
        return (self.lo if a is None else a), (self.hi if b is None else b)

    @property
    def done(self):
        """nothing left to learn: at a bound, or a slope of exactly 0 was seen"""
        a, b = self._ends()
        return self.at_bound or (b is not None and self.seen[b][1] == 0)

    def grid(self):
        a, b = self.bracket if self.seen else (max(self.lo, 0.125), min(self.hi, 8.0))
        g = np.exp(np.linspace(math.log(a), math.log(b), self.points))
        g[0], g[-1] = a, b
        return sorted({min(self.hi, max(self.lo, float(np.float32(v)))) for v in g})

    def update(self, betas, loss, dloss):
        for b, l, d in zip(betas, loss, dloss):
            b, l, d = float(b), float(l), float(d)
            if not (math.isfinite(l) and math.isfinite(d)):
                raise ops.BayesLMError("TemperatureSearch: loss %r with slope %r at beta = %r is not finite (a target the model "
                                       "gives probability 0, or a NaN in its output)" % (l, d, b))
            self.seen[b] = (l, d)
        a, b = self._ends()
        lo_seen, hi_seen = min(self.seen), max(self.seen)
        self.at_bound = (a is None and lo_seen <= self.lo) or (b is None and hi_seen >= self.hi)

    def result(self):
        if not self.seen:
            raise ops.BayesLMError("TemperatureSearch.result: nothing evaluated yet")
        a, b = self._ends()
        if a is not None and b is not None:
            da, db = self.seen[a][1], self.seen[b][1]
            return a - da * (b - a) / (db - da)
        return b if a is None else a  # one sign throughout: the end on the minimiser's side (the bound once at_bound)


@dataclasses.dataclass
class TemperatureFit:
    """What fit_temperature returns."""
    temperature: float   # 1 / beta
    beta: float          # the fitted inverse temperature, a float32 value: what evaluate_report(temperature=...) hands the kernel
    at_bound: bool       # the NLL still fell at the search's lo or hi: beta is that bound, not a minimiser
    passes: int          # search walks run (the walk that fills before / after not counted)
    curve: list          # [beta, loss, dloss, ece] of every beta evaluated, in the order evaluated
    before: EvalReport   # the fit text at beta = 1
    after: EvalReport    # the fit text at beta


def fit_temperature(model, source, seq_len, mc_samples=0, seed=1111, bins=15, passes=3, lo=1.0 / 16, hi=16.0, points=8):
    """Temperature scaling (Guo et al. 2017): the one scalar T = 1 / beta that minimises the NLL of ``model`` on the held-out
    stream ``source``, at mean weights or under the average of ``mc_samples`` weight samples (where it tempers the AVERAGE:
    pbar^beta / Z) -> TemperatureFit.  ``passes`` walks of the text evaluate ``points`` betas each (evaluate_temperatures: one
    read of every chunk for all of them) and narrow TemperatureSearch's bracket -- three passes of eight leave a ratio of
    64^(1/343) = 1.012 between its ends, and the secant through the two slopes places beta inside it; the search stops early at a
    bound.  A last walk over [1, beta] fills ``before`` and ``after``.  Refuses what evaluate_report refuses, and passes < 1."""
    if int(passes) < 1:
        raise ops.BayesLMError("fit_temperature: passes = %r, at least one search walk is needed" % (passes,))
    search = TemperatureSearch(lo, hi, points)
    curve, done = [], 0
    for _ in range(int(passes)):
        betas = search.grid()
        reps, dloss = evaluate_temperatures(model, source, seq_len, betas, mc_samples, seed, bins)
        search.update(betas, [r.loss for r in reps], dloss)
        curve += [[b, r.loss, d, r.ece] for b, r, d in zip(betas, reps, dloss)]
        done += 1
        if search.done:
            break
    beta = float(np.float32(search.result()))
    (before, after), dloss = evaluate_temperatures(model, source, seq_len, [1.0, beta], mc_samples, seed, bins)
    curve += [[b, r.loss, d, r.ece] for b, r, d in zip((1.0, beta), (before, after), dloss)]
    return TemperatureFit(1.0 / beta, beta, search.at_bound, done, curve, before, after)


# ----------------------------------------------------------------------------
# continuous neural cache: a pointer over the recent decoder-input rows of the evaluated text
# ----------------------------------------------------------------------------
_CACHE_ROWS_BYTES = 8 << 30  # the decoder-input rows of a text stay on the device: texts beyond this are refused


@dataclasses.dataclass
class CacheReport:
    """What evaluate_cache returns; ``as_dict()`` is the ``cache`` block the evaluate command writes."""
    tokens: int              # tokens that entered the figures
    skipped: int             # tokens whose target is outside [0, V): left out, as evaluate_report leaves them out
    loss: float              # mean NLL with the cache, nats
    ppl: float
    base_loss: float         # mean NLL of the model alone: evaluate_report(...).loss
    base_ppl: float
    window: int
    theta: float             # as the kernel got it (float32)
    lam: float
    cache_hit_rate: float    # share of tokens whose target is the label of a key in their window (a finite ``match``)
    mean_cache_prob: float   # mean p_cache(target)
    per_token: Optional[dict] = None  # keep_tokens: arrays in text order (tgt, nll_model, nll, lse, match), skipped tokens included

    def as_dict(self):
        d = dataclasses.asdict(self)
        del d["per_token"]
        return d


def _cache_args(who, mc_samples, temperature, window):
    """The refusals of the neural cache that need no model: all before any launch."""
    if int(mc_samples) != 0:
        raise ops.BayesLMError("%s: mc_samples = %r: a cache under Monte-Carlo weight samples is not built (whose rows would the "
                               "keys be?); run it at mean weights" % (who, mc_samples))
    if float(temperature) != 1.0:
        raise ops.BayesLMError("%s: temperature = %r: the cache mixes with the model's distribution as it is; a tempered one is "
                               "not built" % (who, temperature))
    if dist.is_initialized() and dist.get_world_size() > 1:
        raise ops.BayesLMError("%s runs in a single process (world size %d): more than one rank is not built, the cache reads "
                               "the text as one stream" % (who, dist.get_world_size()))
    if int(window) < 1:
        raise ops.BayesLMError("%s: window = %r, the cache needs at least one key" % (who, window))
    return int(window)


def _cache_walk(who, model, source, seq_len):
    """One walk of the text at mean weights (_report_walk: evaluate_report's windows and chunks) that keeps every decoder-input
    row on the device -> dict: rows (n_tok, K) and tgt / nll (n_tok,) on the device IN TEXT ORDER, hi = arange(n_tok) int32,
    the host's nll / valid in walk order (what evaluate_report sums), V."""
    from .model import inference_decoder
    dec = inference_decoder(model)
    if dec is None:
        raise ops.BayesLMError("%s: %s has no decoder that hands back its input rows" % (who, type(model).__name__))
    K = dec.weight.shape[1]
    n_tok = max(0, source.shape[0] - 1) * source.shape[1]
    if n_tok * K * 4 > _CACHE_ROWS_BYTES:
        raise ops.BayesLMError("%s: the %d decoder-input rows of width %d take %.2f GiB on the device, beyond the %d GiB this keeps "
                               "(streaming a longer text through the cache is not built)"
                               % (who, n_tok, K, n_tok * K * 4 / 2.0 ** 30, _CACHE_ROWS_BYTES >> 30))
    dev = source.device
    rows = torch.empty(n_tok, K, device=dev, dtype=torch.float32)
    at = [0]

    def keep_rows(x):
        rows[at[0]:at[0] + x.shape[0]] = x
        at[0] += x.shape[0]

    host, placed, V, _ = _report_walk(who, model, source, seq_len, 0, 0, True, None, rows_out=keep_rows)
    if at[0] != n_tok or len(host["tgt"]) != n_tok:
        raise ops.BayesLMError("%s: the walk handed back %d rows for %d targets (%d expected)" % (who, at[0], len(host["tgt"]), n_tok))
    order = _text_order(source.shape, placed)
    valid = (host["tgt"] >= 0) & (host["tgt"] < V)
    text_rows = rows.index_select(0, torch.from_numpy(order).to(dev))  # text order: one gather by position
    del rows
    return {"rows": text_rows, "tgt": torch.from_numpy(host["tgt"][order]).to(dev),
            "nll": torch.from_numpy(np.ascontiguousarray(host["nll"][order])).to(dev),
            "valid": torch.from_numpy(valid[order]).to(dev), "hi": torch.arange(n_tok, device=dev, dtype=torch.int32),
            "host_nll": host["nll"], "host_valid": valid, "order": order, "V": V, "n_tok": n_tok}


def _cache_scores(walk, thetas, window):
    """blm_cache_scores over the stored rows: q = k = the text's rows, hi[t] = t -> CacheScores, both (J, n_tok)"""
    with torch.no_grad():
        return ops.cache_scores(walk["rows"], walk["rows"], walk["tgt"], walk["tgt"], walk["hi"], thetas, window)


def evaluate_cache(model, source, seq_len, window, theta, lam, keep_tokens=False, mc_samples=0, temperature=1.0):
    """evaluate_report's held-out loss with the continuous neural cache (Grave, Joulin, Usunier 2017) mixed in -> CacheReport.

    Row t of the text has the decoder input h_t and the target y_t.  The cache of row t holds the ``window`` rows before it,
    C_t = { i : max(0, t - window) <= i < t } (the target of row t is known only after it), p_cache(y_t) =
    sum_{i in C_t, y_i = y_t} exp(theta h_t.h_i) / sum_{i in C_t} exp(theta h_t.h_i), and the token is scored with
    p = (1 - lam) p_model + lam p_cache; the first token (an empty cache) with p_model.  Text order is the order of the text
    positions: the stream is one text, the columns of ``source`` consecutive pieces of it, so a column's cache reaches back
    into the column before.

    The walk is evaluate_report's at mean weights (_report_walk) with the decoder-input rows kept on the device (n_tok x K x 4
    bytes; more than 8 GiB is refused), put in text order by one gather; blm_cache_scores reduces the banded h h^T to the two
    log-sums per token without storing a score, and ops.cache_mix mixes.  ``base_loss`` is evaluate_report's loss of the same
    arguments, bit for bit.  A token whose target is outside [0, V) is skipped as there; it still stands in the window as a key.

    Refused, before any launch: mc_samples other than 0, a temperature other than 1, more than one rank, window < 1, theta
    that is negative or not finite, lam outside [0, 1), a model whose decoder cannot hand back its input rows."""
    who = "evaluate_cache"
    window = _cache_args(who, mc_samples, temperature, window)
    th = ops.cache_thetas([theta], who)
    lam = float(lam)
    if not 0.0 <= lam < 1.0:
        raise ops.BayesLMError("%s: lam = %r outside [0, 1)" % (who, lam))
    walk = _cache_walk(who, model, source, seq_len)
    sc = _cache_scores(walk, [theta], window)
    lse, match = sc.lse[0], sc.match[0]
    nll = ops.cache_mix(walk["nll"], lse, match, lam)
    inv = np.argsort(walk["order"], kind="stable")  # text order -> walk order: the sums run as evaluate_report's do
    base = report_from_tokens(walk["host_nll"], valid=walk["host_valid"])
    dev_cols = torch.stack([nll, lse, match]).cpu().numpy()
    with_cache = report_from_tokens(dev_cols[0][inv], valid=walk["host_valid"])
    ok = walk["host_valid"][walk["order"]]
    n = int(ok.sum())
    with np.errstate(invalid="ignore"):
        p_cache = np.where(np.isneginf(dev_cols[2]), 0.0, np.exp(dev_cols[2].astype(np.float64) - dev_cols[1].astype(np.float64)))
    rep = CacheReport(tokens=base.tokens, skipped=base.skipped, loss=with_cache.loss, ppl=with_cache.ppl, base_loss=base.loss,
                      base_ppl=base.ppl, window=window, theta=float(th.theta[0]), lam=lam,
                      cache_hit_rate=float(np.isfinite(dev_cols[2])[ok].sum() / n) if n else float("nan"),
                      mean_cache_prob=float(p_cache[ok].sum() / n) if n else float("nan"))
    if keep_tokens:
        rep.per_token = {"tgt": walk["tgt"].cpu().numpy(),
                         "nll_model": walk["host_nll"][walk["order"]], "nll": dev_cols[0], "lse": dev_cols[1], "match": dev_cols[2]}
    return rep


class CacheSearch:
    """Host-side search for the theta of the neural cache that minimises a held-out loss, from the loss on log-spaced grids of
    ``points`` thetas (one launch of blm_cache_scores each: eight thetas share the dot products).

    Domain [lo, hi] = [1e-4, 16] by default.  theta multiplies a raw dot product h.h', whose size is about K for
    post-LayerNorm Transformer rows (|h|^2 = K = 512..1024: useful thetas of 1e-3..1e-1) and at most the hidden width, usually
    a few tens, for raw LSTM states in (-1, 1)^K (Grave et al. report 0.1..1 there): [1e-4, 16] holds both with a decade to
    spare on each side.  Three passes of eight points leave a ratio of (1.6e5)^(4/343) = 1.15 between neighbours.

        grid()     the next thetas (float32 values): geometric over the bracket, ends included.
        update()   takes the thetas and their losses (a non-finite loss raises, naming theta); the bracket becomes the best
                   theta seen and its two neighbours among everything seen (the domain's end where there is none).
        result()   the best theta seen; ``at_bound`` is set while that is an end of the domain: the loss may still fall beyond.

    The loss need not be unimodal in theta; the search then ends in the basin of its best grid point."""

    def __init__(self, lo=1e-4, hi=16.0, points=8):
        self.lo, self.hi, self.points = float(np.float32(lo)), float(np.float32(hi)), int(points)
        if not (0.0 < self.lo < self.hi < math.inf):
            raise ops.BayesLMError("CacheSearch: need 0 < lo < hi < inf, got lo = %r, hi = %r" % (lo, hi))
        if not 3 <= self.points <= 8:
            raise ops.BayesLMError("CacheSearch: points = %r outside 3..8, what one launch evaluates" % (points,))
        self.seen = {}  # theta -> loss
        self.at_bound = False

    @property
    def best(self):
        return min(self.seen, key=lambda t: (self.seen[t], t))

    @property
    def bracket(self):
        if not self.seen:
            return self.lo, self.hi
        ts, b = sorted(self.seen), self.best
        i = ts.index(b)
        return (ts[i - 1] if i > 0 else self.lo), (ts[i + 1] if i + 1 < len(ts) else self.hi)

    def grid(self):
        a, b = self.bracket
        g = np.exp(np.linspace(math.log(a), math.log(b), self.points))
        g[0], g[-1] = a, b
        return sorted({min(self.hi, max(self.lo, float(np.float32(v)))) for v in g})

    def update(self, thetas, loss):
        for t, l in zip(thetas, loss):
            t, l = float(t), float(l)
            if not math.isfinite(l):
                raise ops.BayesLMError("CacheSearch: loss %r at theta = %r is not finite" % (l, t))
            self.seen[t] = l
        self.at_bound = self.best <= self.lo or self.best >= self.hi

    def result(self):
        if not self.seen:
            raise ops.BayesLMError("CacheSearch.result: nothing evaluated yet")
        return self.best


def cache_best_lambda(nll_model, lse, match, valid=None, lam_max=0.95, iters=50):
    """For each row of the (J, n) arrays ``lse`` / ``match`` (or (n,) ones): the lam in [0, lam_max] that minimises the mean NLL
    of (1 - lam) p_model + lam p_cache over the ``valid`` tokens -> (lam (J,), loss (J,)) float64 tensors on the arrays' device.
    With r = p_cache / p_model per token the loss is -mean log p_model - mean log(1 + lam (r - 1)), convex in lam; its slope
    -mean (r - 1) / (1 + lam (r - 1)) changes sign at most once, and ``iters`` bisections on that sign place lam (every
    bracket moves in one tensor operation: no host round trip inside the loop).  Tokens with an empty cache (lse = -inf) keep
    p_model and do not enter the slope.  Everything in float64."""
    lam_max = float(lam_max)
    if not 0.0 < lam_max < 1.0:
        raise ops.BayesLMError("cache_best_lambda: lam_max = %r outside (0, 1)" % lam_max)
    nll = nll_model.double().reshape(1, -1)
    lse2, match2 = lse.double().reshape(-1, nll.shape[1]), match.double().reshape(-1, nll.shape[1])
    ok = torch.ones_like(nll, dtype=torch.bool) if valid is None else valid.reshape(1, -1).bool()
    n = ok.sum().clamp(min=1).double()
    live = ok & ~torch.isneginf(lse2)  # tokens the cache can move
    log_r = torch.where(torch.isneginf(match2), match2, match2 - lse2) + nll  # log (p_cache / p_model)
    d = torch.where(live, torch.exp(log_r) - 1.0, torch.zeros_like(log_r))   # r - 1 >= -1; 0: no contribution

    def slope_sum(lam):  # sum (r - 1) / (1 + lam (r - 1)) = -n d loss / d lam
        return (d / (1.0 + lam.reshape(-1, 1) * d)).sum(1)

    J = d.shape[0]
    a, b = torch.zeros(J, dtype=torch.float64, device=d.device), torch.full((J,), lam_max, dtype=torch.float64, device=d.device)
    falls_at_0, falls_at_max = slope_sum(a) > 0, slope_sum(b) >= 0
    for _ in range(int(iters)):
        mid = 0.5 * (a + b)
        falls = slope_sum(mid) > 0
        a, b = torch.where(falls, mid, a), torch.where(falls, b, mid)
    lam = torch.where(falls_at_max, torch.full_like(a, lam_max), torch.where(falls_at_0, 0.5 * (a + b), torch.zeros_like(a)))
    base = torch.where(ok, nll, torch.zeros_like(nll)).sum() / n
    loss = base - torch.log1p(lam.reshape(-1, 1) * d).sum(1) / n
    return lam, loss


@dataclasses.dataclass
class CacheFit:
    """What fit_cache returns."""
    theta: float        # a float32 value: what evaluate_cache hands the kernel
    lam: float
    at_bound: bool      # theta is an end of the search's domain, or lam its upper bound: the loss may still fall beyond
    loss_before: float  # the fit text without the cache
    loss_after: float   # ... with it at (theta, lam); <= loss_before, since lam = 0 is always a candidate
    curve: list         # [theta, best lam, loss] of every theta evaluated, in the order evaluated


def fit_cache(model, source, seq_len, window, passes=3, lo=1e-4, hi=16.0, points=8, lam_max=0.95, mc_samples=0, temperature=1.0):
    """The theta and lam of the neural cache that minimise the loss of ``model`` on the held-out stream ``source`` at the given
    ``window`` -> CacheFit.  The model walks the text ONCE (evaluate_cache's walk: the rows stay on the device); each of the
    ``passes`` search passes relaunches only blm_cache_scores on the stored rows with CacheSearch's ``points`` <= 8 thetas in one
    launch, and for every theta cache_best_lambda finds its best lam in [0, lam_max] on the device in float64.  lam = 0, the
    model alone, is always a candidate: loss_after <= loss_before.  Refuses what evaluate_cache refuses, and passes < 1."""
    who = "fit_cache"
    window = _cache_args(who, mc_samples, temperature, window)
    if int(passes) < 1:
        raise ops.BayesLMError("fit_cache: passes = %r, at least one search pass is needed" % (passes,))
    search = CacheSearch(lo, hi, points)
    walk = _cache_walk(who, model, source, seq_len)
    n = walk["valid"].sum().clamp(min=1).double()
    loss_before = float(walk["nll"].double()[walk["valid"]].sum() / n)
    curve, lam_of = [], {}
    for _ in range(int(passes)):
        thetas = search.grid()
        sc = _cache_scores(walk, thetas, window)
        lam, loss = cache_best_lambda(walk["nll"], sc.lse, sc.match, walk["valid"], lam_max)
        lam, loss = lam.cpu().tolist(), loss.cpu().tolist()
        search.update(thetas, loss)
        for t, la, l in zip(thetas, lam, loss):
            lam_of[t] = la
            curve.append([t, la, l])
    theta = float(np.float32(search.result()))
    lam, loss_after = lam_of[search.result()], search.seen[search.result()]
    if not loss_after < loss_before:  # the cache does not help on this text: the model alone
        lam, loss_after = 0.0, loss_before
    return CacheFit(theta, float(lam), bool(search.at_bound or lam >= lam_max), loss_before, float(loss_after), curve)


# ----------------------------------------------------------------------------
# dynamic evaluation (Krause, Kahembwe, Murray, Renals 2018): the weights adapt to the text while it is scored
# ----------------------------------------------------------------------------
# The model families whose eval-mode forward back-propagates through the engine's ops into every mean weight (each tried once
# on the GPU, tests/test_gpu_dyneval.py); any other class is refused by name.
_DYNEVAL_FAMILIES = ("TransformerModel", "BayesTransformerModel", "RNNModel", "BayesRNNModel", "GaussTransformerModel",
                     "VTransformerModel", "GaussRNNModel", "VariationalRNNModel")


@dataclasses.dataclass
class DynEvalStats:
    """What dyneval_stats returns: the gradient statistics of the rms rule, in the layout of FlatBuffers(model)."""
    rms: torch.Tensor   # (FlatBuffers.total,) float32 on the device: sqrt of the mean of g^2 over the windows; 0 in padding and log sigma
    mean: torch.Tensor  # (2,) float32 on the device: rbar, the mean of rms over the live entries (rms > 0), and their number
    live: int           # the number of live entries
    windows: int        # windows that entered the statistics


@dataclasses.dataclass
class DynEvalReport:
    """What evaluate_dynamic returns; ``as_dict()`` is the core of the ``dyneval`` block the evaluate command writes."""
    tokens: int      # tokens that entered the figures (targets inside [0, V))
    loss: float      # mean NLL, nats, every window scored BEFORE its update
    ppl: float
    lr: float
    decay: float
    eps: float
    rule: str        # "sgd" | "rms"
    windows: int
    updates: int     # windows - 1: none follows the last window
    per_token: Optional[dict] = None  # keep_tokens: tgt and nll in text order

    def as_dict(self):
        d = dataclasses.asdict(self)
        del d["per_token"]
        return d


@dataclasses.dataclass
class DynEvalFit:
    """What fit_dyneval returns."""
    lr: float
    decay: float
    loss: float         # the least loss of the curve; <= loss_static, since (0, 0) is always a candidate
    loss_static: float  # the fit text at lr = decay = 0: the walk without adaptation
    curve: list         # [lr, decay, loss] of every candidate, in the order evaluated


def _dyneval_rate(who, name, v):
    try:
        v = float(v)
    except (TypeError, ValueError):
        v = float("nan")
    if not (math.isfinite(v) and v >= 0.0):
        raise ops.BayesLMError("%s: %s = %r is not a finite number >= 0" % (who, name, v))
    return v


def _dyneval_rates(who, lr, decay, eps):
    return tuple(_dyneval_rate(who, k, v) for k, v in (("lr", lr), ("decay", decay), ("eps", eps)))


def _dyneval_check_stats(who, flat, stats):
    if stats is not None and (not isinstance(stats, DynEvalStats) or stats.rms.numel() != flat.total):
        raise ops.BayesLMError("%s: stats must be the DynEvalStats of this model (%d flat entries), got %s" % (
            who, flat.total, "%d entries" % stats.rms.numel() if isinstance(stats, DynEvalStats) else type(stats).__name__))


def _dyneval_args(who, mc_samples=0, temperature=1.0, cache_window=None):
    """The refusals of dynamic evaluation that need no model: all before any launch."""
    if int(mc_samples) != 0:
        raise ops.BayesLMError("%s: mc_samples = %r: dynamic evaluation under Monte-Carlo weight samples is not built (the update "
                               "moves the mean weights, which sample would it follow?); run it at mean weights" % (who, mc_samples))
    if float(temperature) != 1.0:
        raise ops.BayesLMError("%s: temperature = %r: the gradient step is taken on the model's own NLL; a tempered one is not "
                               "built" % (who, temperature))
    if cache_window is not None:
        raise ops.BayesLMError("%s: cache_window = %r: the neural cache together with dynamic evaluation is not built (its keys "
                               "would come from weights that move)" % (who, cache_window))
    if dist.is_initialized() and dist.get_world_size() > 1:
        raise ops.BayesLMError("%s runs in a single process (world size %d): more than one rank is not built, every column "
                               "shares one set of adapting weights" % (who, dist.get_world_size()))


@contextlib.contextmanager
def _dyneval_session(who, model):
    """The model re-homed into a FlatBuffers for one walk -> (flat, theta*: a copy of the flat weights).  On the way out, return
    or exception alike, every parameter gets back its ORIGINAL storage (never written: the trained values bit for bit) and its
    .grad, every module its training flag, and ops its gradient hook and embedding sink."""
    name = type(model).__name__
    if name not in _DYNEVAL_FAMILIES:
        raise ops.BayesLMError("%s: %s: the eval-mode forward of this family is not known to back-propagate through the engine's "
                               "ops (supported: %s)" % (who, name, ", ".join(_DYNEVAL_FAMILIES)))
    with _rehomed(who, model, "dynamic evaluation runs at mean weights") as flat:
        yield flat, flat.flat_param.clone()


@contextlib.contextmanager
def _rehomed(who, model, what):
    """The model re-homed into a FlatBuffers (no momentum buffer) for one walk that overwrites its weights in place -> flat.  On
    the way out, return or exception alike, every parameter gets back its ORIGINAL storage (never written: the trained values bit
    for bit) and its .grad, every module its training flag, and ops its gradient hook and embedding sink."""
    name = type(model).__name__
    state = getattr(model, "noise_state", None)
    if state is not None and state.source == "torch":
        raise ops.BayesLMError("%s: noise source 'torch' is a parity mode of training runs; %s "
                               "with the engine's own kernels (set_noise_source('philox'))" % (who, what))
    params = [p for p in model.parameters() if p.requires_grad]
    if not params:
        raise ops.BayesLMError("%s: %s has no trainable parameter" % (who, name))
    saved = [(p, p.data, p.grad) for p in params]
    flags = [(m, m.training) for m in model.modules()]
    hook, sink = ops._GRAD_HOOK, ops._EMBED_SINK
    try:
        ops.set_grad_ready_hook(None)
        ops.set_embed_grad_sink(None)
        model.eval()
        flat = FlatBuffers(model)
        flat.flat_mom = None  # no momentum in these walks
        yield flat
    finally:
        for p, data, grad in saved:
            p.data = data
            p.grad = grad
        for m, t in flags:
            m.training = t
        ops.set_grad_ready_hook(hook)
        ops.set_embed_grad_sink(sink)


def _dyneval_walk(who, model, flat, windows, cols, after_backward):
    """Steps 1 and 2 of every window: eval-mode forward in grad mode, the per-token NLL, the gradient of the window's mean NLL
    into flat.flat_grad (which must be zero on entry to every window: ``after_backward(k, nll, last)`` sees to it) -> the
    per-token NLLs, one device array per window."""
    from .model import CarriedState
    state = CarriedState(model, cols)
    nlls = []
    with torch.enable_grad():
        for k, (data, targets, _, _) in enumerate(windows):
            out = state(data)
            if not out.requires_grad:
                raise ops.BayesLMError("%s: the eval-mode forward of %s gave logits without a gradient path" % (who, type(model).__name__))
            loss, nll = ops.cross_entropy(out.view(-1, out.shape[-1]), targets, unit_grad=True)
            loss.backward()
            nlls.append(nll)
            after_backward(k, nll, k == len(windows) - 1)
    return nlls


def dyneval_stats(model, source, seq_len, windows):
    """The gradient statistics of the rms rule from the first ``windows`` windows of ``source`` (the training text), walked as
    evaluate_dynamic walks its text but with NO update: MS = the mean over those windows of g^2, rms = sqrt(MS), and rbar, the
    mean of rms over the live entries MS > 0 (blm_dyneval_accum per window, blm_dyneval_rms once) -> DynEvalStats.  A text with
    fewer windows gives them all (``windows`` of the result says how many).  Leaves the model as it found it."""
    who = "dyneval_stats"
    _dyneval_args(who)
    if int(windows) < 1:
        raise ops.BayesLMError("%s: windows = %r, the statistics need at least one" % (who, windows))
    with _dyneval_session(who, model) as (flat, _):
        wins = list(_eval_windows(source, seq_len, False, group=False, limit=int(windows), who=who))
        ms =torch.zeros_like(flat.flat_grad)

        def accumulate(k, nll, last):
            ops.dyneval_accum(ms, flat.flat_grad)
            flat.zero_grad()

        _dyneval_walk(who, model, flat, wins, source.shape[1], accumulate)
        rms, mean = ops.dyneval_rms(ms, len(wins))
        return DynEvalStats(rms, mean, int(mean[1].item()), len(wins))


def _dyneval_run(who, model, flat, theta0, source, wins, lr, decay, stats, eps, keep_tokens, on_window):
    """One adapted walk from theta* inside a session -> DynEvalReport"""
    with torch.no_grad():
        flat.flat_param.copy_(theta0)
    flat.zero_grad()
    rms, mean = (None, None) if stats is None else (stats.rms, stats.mean)

    def update(k, nll, last):
        if on_window is not None:
            on_window(k, nll)
        if not last:
            ops.dyneval_update(flat.flat_param, flat.flat_grad, theta0, lr, decay, rms, mean, eps, zero_grad=True)

    nlls = _dyneval_walk(who, model, flat, wins, source.shape[1], update)
    V = model.decoder.weight.shape[0]  # targets outside [0, V) are skipped, as evaluate_report skips them
    tgt = torch.cat([w[1] for w in wins]).cpu().numpy()
    nll = torch.cat(nlls).cpu().numpy()
    valid = (tgt >= 0) & (tgt < V)
    base = report_from_tokens(nll, valid=valid)
    rep = DynEvalReport(tokens=base.tokens, loss=base.loss, ppl=base.ppl, lr=lr, decay=decay, eps=eps,
                        rule="sgd" if stats is None else "rms", windows=len(wins), updates=max(0, len(wins) - 1))
    if keep_tokens:
        order = _text_order(source.shape, [w[2:] for w in wins])
        rep.per_token = {"tgt": tgt[order], "nll": nll[order]}
    return rep


def evaluate_dynamic(model, source, seq_len, lr, decay, stats=None, eps=0.01, keep_tokens=False, on_window=None, mc_samples=0,
                     temperature=1.0, cache_window=None):
    """Held-out loss of ``model`` over the batchified stream ``source`` under dynamic evaluation -> DynEvalReport.

    The text is walked in windows of ``seq_len`` rows, ONE at a time (no grouping as in evaluate: a window must not see weights
    adapted on its own future); all columns share one set of weights.  Window k is scored in eval mode (mean weights, no dropout,
    no noise) under the weights theta_k -- that NLL is what the report sums -- then the gradient g of its mean NLL (no KL, no
    clip) moves the weights by one fused pass over the flat buffers (ops.dyneval_update, blm_dyneval_update):
        sgd rule (``stats`` None):  theta <- theta - lr g                    + min(1, decay)          (theta* - theta)
        rms rule (dyneval_stats):   theta <- theta - lr g / (r + eps rbar)   + min(1, decay r / rbar) (theta* - theta)
    and clears g in the same pass.  No update follows the last window.  An LSTM's state is carried and detached between windows,
    a Transformer's windows are independent.  ``on_window(k, nll)`` is called after window k's backward, before its update.
    The walk synchronises with the host only at its end (and wherever ``on_window`` does).

    The model is left as it was found, on return and on an exception: every parameter in its original storage with its values
    bit for bit, every .grad, the training flags, ops' gradient hook and embedding sink.

    Refused: mc_samples other than 0, a temperature other than 1, a cache window, more than one rank, noise source 'torch', a
    model family outside _DYNEVAL_FAMILIES, lr / decay / eps negative or not finite, stats of another model."""
    who = "evaluate_dynamic"
    _dyneval_args(who, mc_samples, temperature, cache_window)
    lr, decay, eps = _dyneval_rates(who, lr, decay, eps)
    with _dyneval_session(who, model) as (flat, theta0):
        _dyneval_check_stats(who, flat, stats)
        wins = list(_eval_windows(source, seq_len, False, group=False, who=who))
        return _dyneval_run(who, model, flat, theta0, source, wins, lr, decay, stats, eps, keep_tokens, on_window)


def fit_dyneval(model, source, seq_len, lrs, decays, stats=None, eps=0.01, max_windows=None, mc_samples=0, temperature=1.0,
                cache_window=None):
    """The (lr, decay) of the grid ``lrs`` x ``decays`` that minimises evaluate_dynamic's loss on the held-out stream ``source``
    (its first ``max_windows`` windows, default all) -> DynEvalFit.  A plain grid: every candidate starts from the trained
    weights and is one evaluate_dynamic walk, bit for bit.  (0, 0), the walk without adaptation, is always a candidate and comes
    first, so the fitted loss never exceeds ``loss_static``; among equal losses the earlier candidate wins."""
    who = "fit_dyneval"
    _dyneval_args(who, mc_samples, temperature, cache_window)
    if max_windows is not None and int(max_windows) < 1:
        raise ops.BayesLMError("%s: max_windows = %r" % (who, max_windows))
    eps = _dyneval_rate(who, "eps", eps)
    cands = [(0.0, 0.0)]
    for a in lrs:
        for b in decays:
            c = (_dyneval_rate(who, "lr", a), _dyneval_rate(who, "decay", b))
            if c not in cands:
                cands.append(c)
    with _dyneval_session(who, model) as (flat, theta0):
        _dyneval_check_stats(who, flat, stats)
        if max_windows is not None:
            source = source[:int(max_windows) * int(seq_len) + 1]
        wins = list(_eval_windows(source, seq_len, False, group=False, who=who))
        curve = [[a, b, _dyneval_run(who, model, flat, theta0, source, wins, a, b, stats, eps, False, None).loss] for a, b in cands]
    best = min(curve, key=lambda c: c[2])
    return DynEvalFit(lr=best[0], decay=best[1], loss=best[2], loss_static=curve[0][2], curve=curve)


# ----------------------------------------------------------------------------
# SWAG: the model average over samples of a Gaussian fitted to the SGD iterates (bayeslms_amd/swag.py)
# ----------------------------------------------------------------------------
def evaluate_swag(model, source, seq_len, posterior, samples, seed=1111, scale=0.5, diag=False, bins=15, temperature=1.0,
                  keep_tokens=False):
    """evaluate_report's figures under the average of S = ``samples`` weight samples of the SWAG ``posterior``
    (swag.SwagPosterior) -> EvalReport with the Monte-Carlo block (mc_samples = S, sample_loss, mean_h_pred, mean_mi) and a
    ``per_token["nll_s"]`` of (tokens, S) under ``keep_tokens``.  Any model family, variational or not: every sample is a full
    set of weights, decoder included, which is what blm_linear_mc_logprobs (one decoder for all samples) cannot serve.

    The model is re-homed into a FlatBuffers for the walk (every parameter gets back its original storage, .grad and training
    flag, by return or by exception) and the S samples are drawn once (SwagPosterior.draw: sample s is a function of
    (posterior, seed, s, scale, diag) alone; S x P floats, refused beyond its byte budget).  The walk is evaluate_report's
    (_eval_windows), one batch at a time: for every s the flat buffer is overwritten with sample s, the eval-mode forward
    runs (a recurrent model carries S hidden sets), the decoder's logits are formed in chunks of _REPORT_ROWS rows and
    blm_logp_avg_accum folds them into the window's (rows, V) running log-average, with each sample's NLL and entropy; after the
    last sample blm_row_stats (blm_row_stats_temps with one beta under a ``temperature`` other than 1: pbar^(1/T) / Z, as
    under mc_samples) reduces log pbar.  mi = H[pbar] - mean_s H[p_s], both untempered.

    Refused: samples outside 2..64, a world size above 1, noise source 'torch', a posterior made for another model."""
    who = "evaluate_swag"
    S = int(samples)
    if not 2 <= S <= 64:
        raise ops.BayesLMError("%s: samples must lie in 2..64, got %d (the SWA mean alone is evaluate_report of "
                               "SwagPosterior.mean_state_dict)" % (who, S))

    def draws(flat):
        posterior.check(flat)
        return posterior.draw(S, seed, scale, diag)

    return _samples_walk(who, model, source, seq_len, S, draws, posterior.check, "a SWAG sample replaces every weight and runs",
                         bins, temperature, keep_tokens)


def _samples_walk(who, model, source, seq_len, S, draws_of, check, what, bins, temperature, keep_tokens):
    """The walk evaluate_swag and evaluate_samples share: ``draws_of(flat)`` -> the (S, P) device matrix of weight vectors in the
    layout of ``flat`` (the model re-homed), called once inside the re-homing; ``check(model)`` refuses another model first."""
    from .model import CarriedState, inference_decoder
    if dist.is_initialized() and dist.get_world_size() > 1:
        raise ops.BayesLMError("%s runs in a single process (world size %d)" % (who, dist.get_world_size()))
    betas = _betas_of(who, temperature)
    dec = inference_decoder(model)
    if dec is None:
        raise ops.BayesLMError("%s: %s has no decoder that hands back its input rows" % (who, type(model).__name__))
    check(model)
    V = dec.weight.shape[0]
    keep = {k: [] for k in ("tgt", "nll", "conf", "entropy", "pred", "rank", "nll_s", "h_pred", "mi")}
    placed = []
    with _rehomed(who, model, what) as flat:
        draws = draws_of(flat)
        dev = flat.flat_param.device
        with torch.no_grad(), dec.inference(input_rows=True):
            state = CarriedState(model, source.shape[1], S)
            for data, targets, starts, n in _eval_windows(source, seq_len, state.hidden is not None):
                R = targets.numel()
                chunks = [(a, min(R, a + _REPORT_ROWS)) for a in range(0, R, _REPORT_ROWS)]
                acc = torch.empty(R, V, device=dev, dtype=torch.float32)
                hsum = torch.empty(R, device=dev, dtype=torch.float32)
                nll_s = [torch.empty(S, b - a, device=dev, dtype=torch.float32) for a, b in chunks]
                for s in range(S):
                    flat.flat_param.copy_(draws[s])
                    x = state(data, s)
                    x = x.reshape(-1, x.shape[-1])
                    for c, (a, b) in enumerate(chunks):
                        ops.logp_avg_accum(ops.linear(x[a:b], dec.weight, dec.bias), acc[a:b], s, S, targets[a:b], hsum[a:b], nll_s[c])
                for a, b in chunks:
                    st = ops.row_stats(acc[a:b], targets[a:b], V)
                    h_pred = st.entropy
                    if betas is not None:  # the tempered fields as (1, rows), as _report_walk keeps them
                        st = ops.row_stats_temps(acc[a:b], betas, targets[a:b], V)
                    for k, v in (("nll", st.nll), ("conf", st.conf), ("entropy", st.entropy), ("pred", st.pred), ("rank", st.rank),
                                 ("h_pred", h_pred), ("mi", h_pred - hsum[a:b] / S)):
                        keep[k].append(v)
                keep["nll_s"].append(torch.cat(nll_s, 1).t())
                keep["tgt"].append(targets)
                placed.append((starts, n))
    host = _tokens_to_host(keep, None if betas is None else 1, ("nll", "conf", "entropy", "h_pred", "mi", "pred", "rank", "nll_s"), S)
    return _report_of(host, V, S, bins, betas, order=_text_order(source.shape, placed) if keep_tokens else None)


def evaluate_samples(model, source, seq_len, samples, bins=15, temperature=1.0, keep_tokens=False):
    """evaluate_report's figures under the average of S given weight vectors: ``samples`` is a sgmcmc.SampleBank (SG-MCMC
    samples, or the members of a deep ensemble: SampleBank.from_checkpoints) or an (S, P) float32 matrix in the layout of
    FlatBuffers, S = 2..64 -> EvalReport with the Monte-Carlo block and ``per_token["nll_s"]`` under ``keep_tokens``, as
    evaluate_swag, whose walk this is: evaluate_swag is "draw, then this".  The matrix is moved to the device once and refused
    beyond swag.DRAW_BYTES.  The model is left as found, by return or by exception.

    Refused: S outside 2..64, a matrix of another width or type, a bank made for another model (swag.PosteriorMismatch), a world
    size above 1, noise source 'torch'."""
    from . import sgmcmc as _sgmcmc, swag as _swag
    who = "evaluate_samples"
    bank = samples if isinstance(samples, _sgmcmc.SampleBank) else None
    mat = None if bank is not None else samples
    if bank is None and (not torch.is_tensor(mat) or mat.dim() != 2 or mat.dtype != torch.float32):
        raise ops.BayesLMError("%s: samples must be a SampleBank or an (S, P) float32 matrix" % who)
    S, P = (len(bank), bank.total) if bank is not None else (int(mat.shape[0]), int(mat.shape[1]))
    if not 2 <= S <= 64:
        raise ops.BayesLMError("%s: samples must hold 2..64 weight vectors, got %d" % (who, S))
    if 4 * S * P > _swag.DRAW_BYTES:
        raise ops.BayesLMError("%s: %d vectors of %d floats are %d bytes (%.2f GiB), beyond the budget of %d bytes: evaluate fewer"
                               % (who, S, P, 4 * S * P, 4 * S * P / 2.0 ** 30, _swag.DRAW_BYTES))

    def check(m):
        if bank is not None:
            bank.check(m)
        total = m.total if hasattr(m, "flat_param") else _swag.flat_layout(m)[2]
        if total != P:
            raise _swag.PosteriorMismatch("total", P, total, "weight vectors", "matrix")

    def draws(flat):
        check(flat)
        dev = flat.flat_param.device
        return bank.to_device(dev) if bank is not None else mat.to(dev).contiguous()

    return _samples_walk(who, model, source, seq_len, S, draws, check, "a weight sample replaces every weight and runs", bins,
                         temperature, keep_tokens)


# ----------------------------------------------------------------------------
# Last-layer Laplace posterior for the decoder (bayeslms_amd/laplace.py; include/bayeslm.h)
# ----------------------------------------------------------------------------
LAPLACE_LINKS = ("probit", "expexp", "mc")
LAPLACE_GRID_MAX = 8  # finite prior precisions one walk of fit_laplace_prior takes


@dataclasses.dataclass
class LaplacePriorFit:
    """What fit_laplace_prior returns: the prior precision with the lowest mean NLL on the fit text."""
    tau: float          # the winner; inf: no finite candidate beat the model itself
    loss: float         # its mean NLL on the fit text
    loss_base: float    # the model's own (tau = inf, through the same kernels)
    curve: list         # [tau, loss] per candidate, tau = inf first
    link: str
    samples: int

    def as_dict(self):
        return dataclasses.asdict(self)


def _laplace_args(who, link, samples, taus):
    """The argument checks that need no device -> (link, S, [tau, ...])"""
    from . import laplace
    if link not in LAPLACE_LINKS:
        raise ops.BayesLMError("%s: link %r is none of %s" % (who, link, ", ".join(LAPLACE_LINKS)))
    try:
        S = int(samples)
    except (TypeError, ValueError):
        raise ops.BayesLMError("%s: samples = %r" % (who, samples))
    if S != 0 and not 2 <= S <= ops.L.LAPLACE_SAMPLES_MAX:
        raise ops.BayesLMError("%s: samples must be 0 or lie in 2..%d, got %d: one sample is no average, and blm_laplace_mc_rows "
                               "takes at most %d" % (who, ops.L.LAPLACE_SAMPLES_MAX, S, ops.L.LAPLACE_SAMPLES_MAX))
    if link == "mc" and S == 0:
        raise ops.BayesLMError("%s: the mc link needs samples in 2..%d" % (who, ops.L.LAPLACE_SAMPLES_MAX))
    if link != "mc" and S != 0:
        raise ops.BayesLMError("%s: samples = %d with the closed-form link %r, which draws none: samples go with link 'mc'"
                               % (who, S, link))
    return link, S, [laplace.prior_precision(t, who) for t in taus]


def _laplace_decoder(who, model, posterior=None):
    from .model import inference_decoder
    if dist.is_initialized() and dist.get_world_size() > 1:
        raise ops.BayesLMError("%s runs in a single process (world size %d)" % (who, dist.get_world_size()))
    dec = inference_decoder(model)
    if dec is None:
        raise ops.BayesLMError("%s: %s has no decoder that hands back its input rows" % (who, type(model).__name__))
    if posterior is not None:
        posterior.check(model)
    return dec


@contextlib.contextmanager
def _training_flags_kept(model):
    """The walk puts the model into eval mode; every module gets its own training flag back, by return or by exception."""
    flags = [(m, m.training) for m in model.modules()]
    try:
        yield
    finally:
        for m, f in flags:
            m.training = f


def fit_laplace(model, source, seq_len, max_windows=None):
    """The last-layer Laplace posterior of ``model``'s decoder from the batchified stream ``source`` (the training text) ->
    laplace.LaplacePosterior.  The walk is evaluate_report's (same windows, chunks of _REPORT_ROWS rows, eval mode, mean
    weights, one process) over the first ``max_windows`` windows of ``seq_len`` rows (None: all).  Per chunk: the logits by
    ops.linear, blm_laplace_curvature in place, the squared rows by blm_lrt_prepare, then ONE TN product that accumulates F_W
    and, through colsum_a, F_b.  No label enters: every row counts.  F is checked once at the end for values that are not finite.
    The model is left as found (training flags, decoder scope), also when the walk raises."""
    from . import laplace
    who = "fit_laplace"
    dec = _laplace_decoder(who, model)
    if max_windows is not None:
        if int(max_windows) < 1:
            raise ops.BayesLMError("%s: max_windows = %r" % (who, max_windows))
        source = source[:int(max_windows) * int(seq_len) + 1]
    V, K = dec.weight.shape
    post = laplace.LaplacePosterior(V, K, dec.weight.device, laplace.manifest_of(dec))

    def chunks(x, targets):
        for a in range(0, x.shape[0], _REPORT_ROWS):
            h = x[a:a + _REPORT_ROWS].contiguous()
            logits = ops.linear(h, dec.weight, dec.bias)
            ops.laplace_curvature(logits, out=logits)
            post.accumulate(logits, ops._lrt_prepare(h, 0))

    with _training_flags_kept(model):
        _report_walk(who, model, source, seq_len, 0, 0, True, None, chunks=chunks)
    if post.n_tokens < 1:
        raise ops.BayesLMError("%s: the text gave no row" % who)
    post.check_finite()
    return post


def _laplace_walk(who, model, source, seq_len, posterior, taus, link, S, seed):
    """ONE walk for every prior precision of ``taus`` -> (one host dict per tau, placed, V).  Per chunk one logits product and
    one square pass, then per tau one variance product ops.linear(h^2, 1 / (F_W + tau), 1 / (F_b + tau)) and one row launch."""
    dec = _laplace_decoder(who, model, posterior)
    inv = [posterior.inverse(t) for t in taus]
    mc = link == "mc"
    fields = ("tgt", "nll", "conf", "entropy", "pred", "rank", "nll_s", "h_pred", "mi")
    keeps = [{k: [] for k in fields} for _ in taus]
    vbars = [[] for _ in taus]
    row0 = [0]

    def chunks(x, targets):
        for a in range(0, x.shape[0], _REPORT_ROWS):
            h = x[a:a + _REPORT_ROWS].contiguous()
            t = targets[a:a + _REPORT_ROWS]
            logits = ops.linear(h, dec.weight, dec.bias)
            h2 = ops._lrt_prepare(h, 0)
            for keep, vb, (s_w, s_b) in zip(keeps, vbars, inv):
                var = ops.linear(h2, s_w, s_b)
                if mc:
                    st = ops.laplace_mc_rows(logits, var, S, seed, t, row0[0] + a)
                    for k, v in (("nll", st.bma_nll), ("conf", st.conf), ("entropy", st.h_pred), ("pred", st.pred), ("rank", st.rank),
                                 ("nll_s", st.nll_s), ("h_pred", st.h_pred), ("mi", st.mi)):
                        keep[k].append(v)
                else:
                    st = ops.laplace_row_stats(logits, var, t, link)
                    for k, v in (("nll", st.nll), ("conf", st.conf), ("entropy", st.entropy), ("pred", st.pred), ("rank", st.rank)):
                        keep[k].append(v)
                    vb.append(st.vbar)
        row0[0] += x.shape[0]
        for keep in keeps:
            keep["tgt"].append(targets)

    with _training_flags_kept(model):
        _, placed, V, _ = _report_walk(who, model, source, seq_len, 0, 0, True, None, chunks=chunks)
    empty = ("nll", "conf", "entropy", "pred", "rank") + (("h_pred", "mi", "nll_s") if mc else ())
    hosts = []
    for keep, vb in zip(keeps, vbars):
        host = _tokens_to_host(keep, None, empty, S)
        if vb:
            host["vbar"] = torch.cat(vb).cpu().numpy()
        hosts.append(host)
    return hosts, placed, V


def evaluate_laplace(model, source, seq_len, posterior, prior_precision, link="probit", samples=0, seed=1111, bins=15,
                     keep_tokens=False):
    """evaluate_report's figures under the last-layer Laplace predictive of ``posterior`` (laplace.LaplacePosterior) with the
    prior precision tau = ``prior_precision`` in (0, inf] -> EvalReport with a ``laplace`` block.  The walk is evaluate_report's;
    per chunk the logits, the logit variance by one more decoder-sized product, then blm_laplace_row_stats (``link`` 'probit' or
    'expexp') or blm_laplace_mc_rows (``link`` 'mc' with ``samples`` in 2..32, noise keyed by ``seed``).  Under 'mc' the report
    carries sample_loss, mean_h_pred and mean_mi as the Monte-Carlo report does; the closed forms have no mutual information.
    tau = inf is the model itself.  Refused before any launch: more than one rank, a model whose decoder cannot hand back its
    rows, a posterior made for another decoder, tau <= 0 or NaN, samples outside 0 or 2..32, samples with a closed-form link,
    'mc' without samples.  The model is left as found, also when the walk raises."""
    who = "evaluate_laplace"
    link, S, (tau,) = _laplace_args(who, link, samples, [prior_precision])
    (host,), placed, V = _laplace_walk(who, model, source, seq_len, posterior, [tau], link, S, seed)
    vbar = host.pop("vbar", None)
    rep = _report_of(host, V, S, bins, order=_text_order(source.shape, placed) if keep_tokens else None)
    rep.laplace = dict(posterior.describe(), prior_precision=tau, link=link, samples=S, seed=int(seed) if S else None)
    if vbar is not None:
        ok = (host["tgt"] >= 0) & (host["tgt"] < V)
        rep.laplace["mean_vbar"] = float(vbar.astype(np.float64)[ok].mean()) if ok.any() else float("nan")
    return rep


def fit_laplace_prior(model, source, seq_len, posterior, taus, link="probit", samples=0, seed=1111):
    """The prior precision among ``taus`` (1..8 finite values) with the lowest mean NLL on the held-out stream ``source`` ->
    LaplacePriorFit, from ONE walk of the text: per chunk one logits product, then per candidate one variance product and one
    row launch.  tau = inf, the model itself, is always a candidate, evaluated through the same kernels and placed first, so
    that it wins a tie: the fitted loss never exceeds the model's own.  Refusals: evaluate_laplace's, and a tau that is not
    finite."""
    from . import laplace
    who = "fit_laplace_prior"
    try:
        taus = list(taus)
    except TypeError:
        raise ops.BayesLMError("%s: taus must be 1..%d positive finite numbers, got %r" % (who, LAPLACE_GRID_MAX, taus))
    if not 1 <= len(taus) <= LAPLACE_GRID_MAX:
        raise ops.BayesLMError("%s: %d prior precisions, one walk takes 1..%d" % (who, len(taus), LAPLACE_GRID_MAX))
    link, S, taus = _laplace_args(who, link, samples, taus)
    if any(math.isinf(t) for t in taus):
        raise ops.BayesLMError("%s: tau = inf is always a candidate; the grid takes finite values" % who)
    cands = [float("inf")] + taus
    hosts, _, V = _laplace_walk(who, model, source, seq_len, posterior, cands, link, S, seed)
    losses = []
    for host in hosts:
        ok = (host["tgt"] >= 0) & (host["tgt"] < V)
        losses.append(float(host["nll"].astype(np.float64)[ok].sum() / ok.sum()) if ok.any() else float("nan"))
    best = laplace.select_prior(cands, losses)
    return LaplacePriorFit(tau=cands[best], loss=losses[best], loss_base=losses[0], curve=[[t, v] for t, v in zip(cands, losses)],
                           link=link, samples=S)
