#!/usr/bin/env python3
"""Headline benchmark: training tokens/s of the Bayesian Transformer-FFN LM (BASELINE.json
configs[2]: 6 layers, d_model 512, d_ff 4096, 8 heads, V = 33,000, seq_len 128, batch 64 per GPU,
--uncertainty Bayesian --T_bayes_pos FFN, dropout 0.2, tied, clip 1.0, SGD momentum 0.9) on N
MI355X of one node, synthetic AMI-shaped token stream, random-init weights, fp32.

One step = forward + CE + KL*seq_len/len(train_data) + backward + gradient all-reduce (N > 1)
+ global-norm clip + SGD, nothing skipped.  Prints ONE JSON line on rank 0.

    python bench.py --gpus 1 --steps 20 --warmup 5          (the headline alone: set up, warm up, timed steps, the line)
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs bench_outputs   (+ what the last timed step computed, .npy)
    python bench.py --gpus 1 --steps 20 --warmup 5 --full   (+ everything else the line can carry, after the headline: eval
                                                             PPL, chip probe, CPU baselines, opt-in GEMM modes, extra_configs;
                                                             at N > 1 the stand-alone all-reduces, comm diagnostics and
                                                             configs[4]'s data-parallel legs)
    python bench.py --gpus N ...        (starts its own N ranks: a torch.distributed.run child process, before
                                         this process has touched the GPU; the child's JSON line and exit code are
                                         relayed)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# dmabuf IPC between the ranks' processes (RCCL / tensor sharing): must be in the environment before HIP starts
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

# cfg3 of BASELINE.json
V, D_MODEL, NHEAD, D_FF, NLAYERS, T, B_PER_GPU = 33000, 512, 8, 4096, 6, 128, 64
DROPOUT, LR, CLIP = 0.2, 0.1, 1.0
PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
# forward FLOPs per token L(2d*3d + 4Td + 2d^2 + 4d*ff) + 2dV = 98.28 M, training = 3x
STEP_FLOPS_PER_TOKEN = 3 * (NLAYERS * (2 * D_MODEL * 3 * D_MODEL + 4 * T * D_MODEL + 2 * D_MODEL * D_MODEL + 4 * D_MODEL * D_FF)
                            + 2 * D_MODEL * V)
PMC_TRAFFIC_FILE = "r05_pmc_sampled_gemm_fwd.json"
PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense bf16 MFMA peak (the opt-in split modes are priced against this one)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused-sampling", type=int, default=-1,
                    help="1: eps generated inside the GEMM tile loader; 0: one materialisation pass; -1: engine default")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline, after it: evaluation PPL, the bare-MFMA chip "
                         "probe, the CPU baselines, the opt-in GEMM modes and extra_configs (N = 1); the stand-alone all-reduces, "
                         "the comm diagnostics and configs[4]'s data-parallel legs (N > 1).  Without it a run sets up, warms up, "
                         "times its steps, writes --dump-outputs and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--cpu-all-cores", action="store_true",
                    help="--full: also time the CPU baseline with one thread per VISIBLE host core, live (~3 minutes on a one-GPU "
                         "box: 256 threads on a 16-core share); otherwise the line reports the committed measurement")
    ap.add_argument("--no-opt-in", action="store_true",
                    help="--full: skip the extra, separately reported runs in the opt-in split-bf16 GEMM modes (N = 1 only)")
    ap.add_argument("--no-extra", action="store_true",
                    help="--full: skip extra_configs (BASELINE configs[1] and configs[4] legs, reported after the headline)")
    ap.add_argument("--batch", type=int, default=B_PER_GPU, help="columns per GPU (default = the named config)")
    ap.add_argument("--backend", type=str, default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for "
                    "rehearsing several ranks on one GPU)")
    ap.add_argument("--dp-overlap", type=int, default=1, help="N > 1: 0 = every bucket all-reduced after backward")
    ap.add_argument("--dp-late-rows", type=int, default=1, help="N > 1: 0 = the tied encoder gradient travels dense")
    ap.add_argument("--deadline-s", type=float, default=None,
                    help="N > 1: overall wall-clock bound of the run (default 420; 0 = none).  Every rank arms a timer that prints "
                         "ONE error JSON line (rank 0) and exits 124 when it fires; the self-launching parent enforces the same bound "
                         "+ 15 s from outside (it terminates the child process group) for ranks that cannot run their own timer")
    ap.add_argument("--dist-timeout-s", type=float, default=None,
                    help="N > 1: rendezvous / collective timeout handed to init_process_group (default 180, BLM_DIST_TIMEOUT_S)")
    ap.add_argument("--dp-autotune", type=int, default=1,
                    help="N > 1: 1 = after the warm-up, three steps each as configured / with the comm-window plans off / with the overlap off "
                         "(barrier-bracketed, max over ranks: the same numbers on every rank); a setting that is more than 2 %% faster than "
                         "the configured one is kept for the timed region and reported in comm.autotune; 0 = run as configured")
    ap.add_argument("--comm-ab-steps", type=int, default=5,
                    help="N > 1, --full: steps of each A/B leg after the timed region (overlap off, comm-window plans off); 0 skips them")
    ap.add_argument("--dp-extras-budget-s", type=float, default=120.0,
                    help="N > 1, --full: wall-clock budget of the extra legs after the headline (configs[4] data-parallel); when it (or the "
                         "deadline) passes, rank 0 prints the headline line it already holds, marked, and every rank exits 0")
    ap.add_argument("--rehearse-hang", type=str, default="",
                    help="test knob of --rehearse-launch: RANK:STAGE[:gil] (RANK `*` = every rank) -- that rank stops for ever when it reaches STAGE "
                         "(rendezvous | warmup | timed | extras); `gil` holds the interpreter lock so that its own deadline timer cannot run")
    ap.add_argument("--rehearse-launch", action="store_true",
                    help="launch plumbing only (spawn, rendezvous, barrier, max-over-ranks, one JSON line from rank 0) "
                         "with NO GPU work: what the CPU-side test of `--gpus N` self-launch runs")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="rank 0 writes what the LAST timed step computed to DIR/<name>.npy (float32), right after the timed "
                         "region: loss and kl as Trainer.step returns them, and a fixed, seeded sample of the updated parameters "
                         "and of the gradient buffer (DUMP_SAMPLE elements each).  Same arguments -> same inputs, so two builds "
                         "can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.cpu_all_cores and not args.full:
        ap.error("--cpu-all-cores times the CPU baseline of a --full run")
    return args


DUMP_SAMPLE = 1 << 22  # elements per sampled buffer: 16 MB each in float32, well under the 64 MB of a dump
DUMP_SEED = 1234


def dump_outputs(out_dir, loss, kl, flat):
    """What the timed path handed its caller in the last step: `loss`, `kl` (Trainer.step's return values) and the model's
    state after it -- a seeded sample of the flat parameter buffer and of the flat gradient buffer (the same indices for both;
    they depend only on DUMP_SEED and the parameter count).  -> total bytes written."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    n = min(DUMP_SAMPLE, flat.total)
    idx = np.sort(np.random.RandomState(DUMP_SEED).choice(flat.total, size=n, replace=False))
    idx_dev = torch.from_numpy(idx).to(flat.flat_param.device)
    arrays = {"loss": loss.detach().float().reshape(1),
              "kl": (kl.detach().float().reshape(1) if kl is not None else torch.zeros(1)),
              "params_sample": flat.flat_param.index_select(0, idx_dev).float(),
              "grads_sample": flat.flat_grad.index_select(0, idx_dev).float()}
    total = 0
    for name, t in arrays.items():
        a = np.ascontiguousarray(t.cpu().numpy(), dtype=np.float32)
        np.save(os.path.join(out_dir, name + ".npy"), a)
        total += a.nbytes
    return total


ERROR_LINE_KEYS = ("metric", "value", "unit", "n_gpus", "error", "last_stage")


def error_line(n_gpus, error, last_stage, **extra):
    """The ONE JSON line of a run that did not finish: same head as the normal line, value null."""
    return json.dumps({"metric": "train_tokens_per_sec", "value": None, "unit": "tokens/s", "n_gpus": n_gpus, "error": error,
                       "last_stage": last_stage, **extra})


def deadline_of(args):
    if args.deadline_s is not None:
        return max(0.0, args.deadline_s)
    return 420.0 if args.gpus > 1 else 0.0


def self_launch(args):
    """`python bench.py --gpus N` from ONE process: run the N ranks as a child `torch.distributed.run` (its own process
    group / session) and relay its output and exit code.  This process has not made (and never makes) a GPU call -- a
    process that has initialised HIP must not be replaced or forked into ranks.  It is also the run's outer bound: the
    ranks' stderr heartbeats (`[blm rank R +S.Ss] stage`) are relayed and remembered, and when the child has neither ended
    nor printed its line `--deadline-s` + 15 s after the start, its process group is terminated (SIGTERM, 10 s later
    SIGKILL), ONE JSON line {"metric", "value": null, "error", "last_stage"} goes to stdout and the exit code is 124.  A child
    that ends non-zero without a line gets the same line with its exit code."""
    import re
    import signal
    import socket
    import subprocess
    import threading
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    t_start = time.time()
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, text=True, start_new_session=True)
    stages, json_lines = {}, []
    beat = re.compile(r"^\[blm rank (\d+) \+([0-9.]+)s\] (.*)$")

    def pump_out():
        for line in proc.stdout:  # the ranks' stdout: rank 0's JSON line (anything else is passed through as well)
            if line.startswith("{"):
                json_lines.append(line)
            sys.stdout.write(line)
            sys.stdout.flush()

    def pump_err():
        for line in proc.stderr:
            m = beat.match(line.rstrip("\n"))
            if m:
                stages[int(m.group(1))] = m.group(3)
            sys.stderr.write(line)
            sys.stderr.flush()
    threads = [threading.Thread(target=pump_out, daemon=True), threading.Thread(target=pump_err, daemon=True)]
    for t in threads:
        t.start()

    def pass_on(signum, _frame):  # a launcher that is told to stop (timeout(1), Ctrl-C, a scheduler) takes its ranks with it
        try:
            os.killpg(proc.pid, signal.SIGTERM)
        except ProcessLookupError:
            pass
        try:
            proc.wait(timeout=10.0)
        except subprocess.TimeoutExpired:
            try:
                os.killpg(proc.pid, signal.SIGKILL)
            except ProcessLookupError:
                pass
        os._exit(128 + signum)
    for sig in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
        signal.signal(sig, pass_on)
    limit = deadline_of(args)
    try:
        rc = proc.wait(timeout=(limit + 15.0) if limit > 0 else None)
    except subprocess.TimeoutExpired:
        for sig, grace in ((signal.SIGTERM, 10.0), (signal.SIGKILL, 10.0)):
            try:
                os.killpg(proc.pid, sig)  # the child's own group (start_new_session): the agent and every rank, nothing else
            except ProcessLookupError:
                break
            try:
                proc.wait(timeout=grace)
                break
            except subprocess.TimeoutExpired:
                continue
        for t in threads:
            t.join(timeout=5.0)
        if not json_lines:
            print(error_line(args.gpus, "deadline: no result %.0f s after the launch (--deadline-s %.0f + 15 s); the child process "
                                        "group was terminated by the launcher" % (time.time() - t_start, limit),
                             {"rank %d" % r: s_ for r, s_ in sorted(stages.items())} or "no heartbeat seen"), flush=True)
        return 124
    for t in threads:
        t.join(timeout=5.0)
    if rc != 0 and not json_lines:
        print(error_line(args.gpus, "the ranks ended with exit code %d and no result line" % rc,
                         {"rank %d" % r: s_ for r, s_ in sorted(stages.items())} or "no heartbeat seen"), flush=True)
    return rc


def arm_deadline(args, rank, world):
    """In-rank half of the bound: a timer thread that, `--deadline-s` after the start, writes where this rank was, prints the
    ONE error JSON line on rank 0 and leaves the process with 124 (os._exit: the main thread may be inside a collective that
    will never return; nothing is exec'ed or replaced).  torchrun then ends the other ranks.  -> the timer (cancel it)."""
    import threading
    limit = deadline_of(args)
    if limit <= 0 or world <= 1:
        return None
    from bayeslms_amd import engine

    def fire(why=None):
        stage = engine.last_stage()
        sys.stderr.write("[blm rank %d] DEADLINE %s: still after stage %r -- giving up\n" % (rank, why or ("%.0f s" % limit), stage))
        sys.stderr.flush()
        if PENDING["headline_done"]:
            # the headline was measured and assembled; what did not return is an EXTRA leg (configs[4]'s data-parallel legs):
            # rank 0 prints the line it holds, marked, and every rank leaves with 0 -- an extra never costs the headline
            if rank == 0 and PENDING["line"] is not None:
                line = PENDING["line"]
                line["extra_configs"] = {"error": "cut short by the deadline after stage %r" % stage}
                line["baseline_configs"] = line.pop("baseline_configs", None)  # stays the last key
                print(json.dumps(line), flush=True)
            else:
                time.sleep(2.0)
            os._exit(0)
        if rank == 0:
            print(error_line(world, "deadline: %.0f s (--deadline-s) passed on rank 0" % limit, stage), flush=True)
        else:
            time.sleep(2.0)  # rank 0's line first: the agent ends every rank as soon as one of them is gone
        os._exit(124)
    t = threading.Timer(limit, fire)
    t.daemon = True
    t.start()
    PENDING["fire"] = fire
    return t


# what the deadline prints when it falls into an extra leg of a multi-rank run (arm_deadline.fire, main)
PENDING = {"headline_done": False, "line": None, "fire": None}


def _timed_steps(step_fn, n, first, dev, world):
    """n steps bracketed like the headline's timed region -> ms per step, max over ranks."""
    cuda = dev is not None and dev.type == "cuda"
    if cuda:
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for i in range(n):
        step_fn(first + i)
    if cuda:
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], dtype=torch.float64, device=dev if (cuda and dist.get_backend() == "nccl") else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    return round(1e3 * el / max(n, 1), 4)


def comm_diagnostics(red, step_fn, first, n_ab, dev, world):
    """After the timed region, so that ONE multi-GPU line explains its own scaling (every rank calls; same order everywhere):
      * `buckets_last_step`: one more step with every collective bracketed on the communication stream
        (GradReducer.bucket_report: size, launch -> done, position relative to the end of backward);
      * `step_ms_as_configured` / `step_ms_no_overlap` / `step_ms_no_comm_window`: n_ab steps each, same barrier + max-over-ranks
        bracket -- all buckets after backward (what the overlap buys), and the GEMM planner's comm-window plans off (what
        leaving CUs to the channel workgroups buys or costs)."""
    rep = {}
    red.measure_buckets = True
    try:
        step_fn(first)
        rep["buckets_last_step"] = red.bucket_report()
    finally:
        red.measure_buckets = False
    first += 1
    if n_ab > 0:
        rep["ab_steps"] = n_ab
        rep["step_ms_as_configured"] = _timed_steps(step_fn, n_ab, first, dev, world)
        first += n_ab
        if red.overlap:
            red.overlap = False
            try:
                rep["step_ms_no_overlap"] = _timed_steps(step_fn, n_ab, first, dev, world)
            finally:
                red.overlap = True
            first += n_ab
        else:
            rep["step_ms_no_overlap"] = None
        if red.comm_plan != "off":
            keep, red.comm_plan = red.comm_plan, "off"
            try:
                rep["step_ms_no_comm_window"] = _timed_steps(step_fn, n_ab, first, dev, world)
            finally:
                red.comm_plan = keep
        else:
            rep["step_ms_no_comm_window"] = None
    return rep


def dp_autotune(red, step_fn, first, dev, world, n=3):
    """The defaults of the gradient exchange (bucket overlap, the planner's comm window) were derived on ONE GPU against a stand-in of
    RCCL's channel kernel.  Before the timed region the ranks time `n` real steps under each alternative -- same barrier + max-over-
    ranks bracket as the timed region, so every rank sees the same three numbers and takes the same decision -- and keep whatever is
    more than 2 % faster than the configured setting.  -> the record for comm.autotune."""
    rec = {"steps_each": n, "ms": {}, "picked": "as_configured"}
    rec["ms"]["as_configured"] = _timed_steps(step_fn, n, first, dev, world)
    first += n
    alts = []
    if red.comm_plan != "off":
        alts.append(("comm_plan_off", "comm_plan", "off"))
    if red.overlap:
        alts.append(("overlap_off", "overlap", False))
    for name, attr, val in alts:
        keep = getattr(red, attr)
        setattr(red, attr, val)
        try:
            rec["ms"][name] = _timed_steps(step_fn, n, first, dev, world)
        finally:
            setattr(red, attr, keep)
        first += n
    best = min(rec["ms"], key=rec["ms"].get)
    if best != "as_configured" and rec["ms"][best] < 0.98 * rec["ms"]["as_configured"]:
        rec["picked"] = best
        for name, attr, val in alts:
            if name == best:
                setattr(red, attr, val)
    return rec


def comm_block(args, engine, red, flat, rccl_env, busbw, diag, replicas_identical, autotune=None):
    """The `comm` object of a multi-rank line (rank 0 assembles it; the collective parts were measured on every rank)."""
    return {
        "backend": args.backend, "world_seen": dist.get_world_size(), "rccl_version": engine.rccl_version() if args.backend == "nccl" else None,
        "dist_timeout_s": engine.dist_timeout_s(args.dist_timeout_s),
        "overlap": bool(args.dp_overlap), "buckets": len(red.buckets),
        # sizes in backward (launch) order: full 32 MB runs, big tensors alone, quarter-size tail buckets
        "bucket_mb": [round((e - s) * 4 / 1e6, 2) for s, e, _ in red.buckets],
        "exchanged_mb_last_step": round(red.last_reduced_elems * 4 / 1e6, 2),
        # the bucket that becomes ready last (layer 0's first parameters): the all-reduce nothing can hide
        "last_bucket_mb": round((red.buckets[-1][1] - red.buckets[-1][0]) * 4 / 1e6, 2),
        "grad_bytes": int(flat.total * 4),
        # stand-alone all-reduces before training, nothing else on the device (engine.allreduce_busbw): the whole gradient and one bucket
        "allreduce_busbw_gbps": None if not busbw else busbw[0]["busbw_gbps"], "allreduce_standalone": busbw,
        # RCCL channel count as pinned before init_process_group (engine.pin_rccl_channels) and the CUs the GEMM
        # planner leaves to the channel workgroups while buckets are in flight
        "rccl_env": rccl_env, "gemm_cus_under_comm": 256 - red.comm_cus, "comm_plan": red.comm_plan,
        # what the timed region ran with: the configured setting, or an alternative that was > 2 % faster in the calibration steps
        "overlap_in_timed_region": bool(red.overlap), "autotune": autotune,
        # parameter checksums of all ranks after the last step, gathered and compared (outside the timed region)
        "replicas_identical": replicas_identical,
        "late_rows": red.late is not None,
        "late_rows_last_step": None if red.late is None else int(red.late.U),
        **(diag or {}),
    }


def _maybe_hang(args, rank, stage):
    """--rehearse-hang RANK:STAGE[:gil] (tests of the deadline paths): this rank never gets past `stage`."""
    if not args.rehearse_hang:
        return
    part = args.rehearse_hang.split(":")
    if (part[0] != "*" and int(part[0]) != rank) or part[1] != stage:
        return
    if len(part) > 2 and part[2] == "gil":
        import ctypes
        ctypes.PyDLL(None).sleep(10 ** 6)  # a C call that keeps the interpreter lock: this rank's own timer thread cannot run
    while True:
        time.sleep(3600)


class _HostStandIn:
    """--rehearse-launch: what stands where engine.Trainer stands in the real run, on CPU tensors -- a small torch network whose
    parameters live in engine.FlatBuffers, gradients exchanged by the real engine.GradReducer (autograd hooks, buckets,
    LateRows for the tied embedding) over gloo, plain SGD.  No kernels of the library are involved and nothing is measured
    for the record; it exists so that every line of the multi-rank protocol runs where there is no GPU."""

    def __init__(self, engine, rank, world, overlap):
        import torch.nn as nn
        torch.manual_seed(1111)
        self.Vs, d = 96, 16
        self.net = nn.ModuleDict({"encoder": nn.Embedding(self.Vs, d), "l1": nn.Linear(d, 64), "l2": nn.Linear(64, d)})
        self.flat = engine.FlatBuffers(self.net)
        self.reducer = engine.GradReducer(self.flat, bucket_bytes=2048, overlap=overlap)
        self.reducer.hook_autograd()
        self.rank, self.world = rank, world

    def step(self, i):
        g = torch.Generator().manual_seed(1000 * i + self.rank)
        ids = torch.randint(0, self.Vs, (12, 3), generator=g)
        tgt = torch.randint(0, self.Vs, (36,), generator=g)
        self.flat.zero_grad()
        h = self.net["l2"](torch.tanh(self.net["l1"](self.net["encoder"](ids))))
        loss = torch.nn.functional.cross_entropy(h.view(-1, h.shape[-1]) @ self.net["encoder"].weight.t(), tgt)
        loss.backward()
        self.reducer.finish()
        with torch.no_grad():
            self.flat.flat_param.add_(self.flat.flat_grad, alpha=-0.1 / self.world)
        return loss.detach()


def rehearse_launch(args, world, rank):
    """No GPU: every step of the multi-rank protocol around (and after) the timed region, on CPU tensors over gloo -- the bounded
    rendezvous, the heartbeats, the deadline timer, the stand-alone all-reduce, warm-up, the barrier-bracketed timed steps with
    max over ranks, the replica check, the comm diagnostics (per-bucket times, A/B legs) and the one JSON line from rank 0.  As in
    main, the stand-alone all-reduce, the comm diagnostics and the extra legs run with --full only."""
    from bayeslms_amd import engine
    timer = arm_deadline(args, rank, world)
    _maybe_hang(args, rank, "rendezvous")
    backend = "gloo" if args.backend == "nccl" else args.backend
    engine.init_distributed(backend, None, args.dist_timeout_s)
    tr = _HostStandIn(engine, rank, world, bool(args.dp_overlap))
    busbw = None
    if args.full:
        busbw = [engine.allreduce_busbw(tr.flat.total * 4, 3), engine.allreduce_busbw(1 << 16, 3)]
        engine.heartbeat("stand-alone all-reduce ok", rank)
    _maybe_hang(args, rank, "warmup")
    for i in range(args.warmup):
        tr.step(i)
    engine.heartbeat("warm-up ok (%d steps)" % args.warmup, rank)
    autotune = dp_autotune(tr.reducer, tr.step, args.warmup, None, world) if args.dp_autotune else None
    _maybe_hang(args, rank, "timed")
    ms = _timed_steps(tr.step, args.steps, args.warmup, None, world)
    engine.heartbeat("timed region ok (%d steps)" % args.steps, rank)
    fp = tr.flat.flat_param
    mine = torch.stack([fp.double().sum(), fp.double().abs().sum()])
    every = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    identical = all(bool(torch.equal(e, every[0])) for e in every)
    diag = None
    if args.full:
        diag = comm_diagnostics(tr.reducer, tr.step, args.warmup + args.steps, args.comm_ab_steps, None, world)
        engine.heartbeat("comm diagnostics ok", rank)
    out = None
    if rank == 0:
        args.backend = backend
        out = {"metric": "train_tokens_per_sec", "value": None, "unit": "tokens/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
               "comm": comm_block(args, engine, tr.reducer, tr.flat, None, busbw, diag, identical, autotune),
               "rehearsal": "launch plumbing only, no GPU work: NOT a measurement", "baseline_configs": None}
    if args.full and not args.no_extra:  # the protocol of the extra legs (main: configs[4]'s data-parallel legs) around a stand-in leg
        def legs():
            ms2 = _timed_steps(tr.step, 2, args.warmup, None, world)
            return [{"id": "rehearsal_extra_leg", "ms_per_step": ms2}]
        ex = run_dp_extras(args, engine, rank, world, out, legs)
        if rank == 0:
            out["extra_configs"] = ex
    if rank == 0:
        out["baseline_configs"] = out.pop("baseline_configs")  # stays the last key
        PENDING["line"] = None
        print(json.dumps(out), flush=True)
        engine.heartbeat("line printed", rank)
    dist.barrier()
    if timer is not None:
        timer.cancel()
    dist.destroy_process_group()


def cpu_baseline(cols=B_PER_GPU, steps=9, warm=1, all_cores_live=False):
    """The CPU oracle (the reference's algorithm restated, pinned to the reference's own outputs incl. its train.py
    trajectories) timed on this box's host cores, SURVEY 8(d) protocol: the SAME workload as `value` -- all 64 batch
    columns, T = 128, dropout 0.2 on (torch's generator, as the reference), fwd + CE + KL + bwd + clip + SGD --
    median of `steps` (9) steps after `warm` warm-up, with the spread of the nine (a shared 16-core slice: +-13 % run to run in round
    4).  ~40 s of CPU work."""
    from bayeslms_amd import model as M
    from bayeslms_amd.data import synthetic_corpus
    from oracle import bayes_oracle as O
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    ncores = min(avail, 16)  # a 1-GPU box's CPU share is 16 cores (the rest of the host serves the other 7 GPUs)
    torch.set_num_threads(ncores)
    torch.manual_seed(1111)
    m = M.BayesTransformerModel(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, True, "FFN")
    names = [k for k, _ in m.named_parameters() if k != "decoder.weight"]
    sd = {k: v.detach().clone().requires_grad_(k in names) for k, v in m.state_dict().items()}
    sd["decoder.weight"] = sd["encoder.weight"]
    del m
    total = warm + steps
    stream = synthetic_corpus(V, cols * (T * total + 1), seed=1111)
    data = stream[: cols * (T * total + 1) // cols * cols].view(cols, -1).t().contiguous()
    bufs = [None] * len(names)

    def timed(first, n, ncol=None):
        out = []
        for s in range(first, first + n):
            s = s % total
            src = data[s * T:(s + 1) * T]
            tgt = data[s * T + 1:(s + 1) * T + 1]
            if ncol is not None:
                src, tgt = src[:, :ncol].contiguous(), tgt[:, :ncol].contiguous()
            tgt = tgt.reshape(-1)
            t0 = time.perf_counter()
            eps = torch.randn(D_MODEL, D_FF)
            for k in names:
                sd[k].grad = None
            loss, _, _ = O.transformer_train_loss(src, tgt, sd, NHEAD, "FFN", eps, T / 65536.0, DROPOUT)
            loss.backward()
            O.clip_and_sgd([sd[k] for k in names], [sd[k].grad for k in names], bufs, LR, CLIP)
            out.append(time.perf_counter() - t0)
        return out
    times = timed(0, total)
    med = sorted(times[warm:])[steps // 2]
    spread = {"min": round(cols * T / max(times[warm:]), 1), "max": round(cols * T / min(times[warm:]), 1), "n": steps}
    # SURVEY 8(d) says "all host cores".  The host of a one-GPU box shows all 256 cores but its CPU share is 16: one thread per visible
    # core is oversubscription -- a step then costs ~80 s whatever the batch (94 tokens/s on the full batch, measured in round 4:
    # profiles/r04_cpu_baseline_all_cores.json) -- so the default run reports that committed measurement and `--cpu-all-cores`
    # repeats it live (one step on the first 8 columns after one warm-up: ~3 minutes)
    all_cores = None
    if avail > ncores:
        if all_cores_live:
            try:
                sub = min(8, cols)
                torch.set_num_threads(avail)
                t_all = timed(0, 2, sub)[1]
                all_cores = {"value": round(sub * T / t_all, 1), "unit": "tokens/s", "cores": avail, "source": "live",
                             "sample": "same step on the first %d of the %d batch columns, torch.set_num_threads(%d), 1 timed step "
                                       "after 1 warm-up" % (sub, cols, avail)}
            finally:
                torch.set_num_threads(ncores)
        else:
            try:
                rec = json.load(open(os.path.join(ROOT, "profiles", "r04_cpu_baseline_all_cores.json")))
                all_cores = {"value": rec["runs"][0]["tokens_per_s"], "unit": "tokens/s", "cores": rec["runs"][0]["threads"],
                             "source": "profiles/r04_cpu_baseline_all_cores.json (measured once, not collected live: ~87 s per step)",
                             "sample": rec["runs"][0]["sample"]}
            except Exception:  # noqa: BLE001
                all_cores = None
    return {"value": round(cols * T / med, 1), "unit": "tokens/s", "cores": ncores, "kind": "port", "spread_tokens_per_s": spread,
            "host_cores_visible": avail, "all_visible_cores": all_cores,
            "sample": "oracle/bayes_oracle.py train step (fwd+CE+KL+bwd+clip+SGD, dropout %.1f on), same model, T=%d, all "
                      "%d batch columns, median of %d steps after %d warm-ups, %d threads (the 1-GPU box's CPU share)"
                      % (DROPOUT, T, cols, steps, warm, ncores)}


def tlm_flops_per_token(T_, V_=V, L_=NLAYERS, d=D_MODEL, ff=D_FF, train=True):
    """forward FLOPs per token L(2d*3d + 4Td + 2d^2 + 4d*ff) + 2dV; training = 3x."""
    f = L_ * (2 * d * 3 * d + 4 * T_ * d + 2 * d * d + 4 * d * ff) + 2 * d * V_
    return 3 * f if train else f


def lstm_flops_per_token(V_, E=1024, H=1024, L_=2, train=True):
    """forward FLOPs per token of the 2-layer LSTM LM: 2 layers x 2(E+H)4H + 2HV; training = 3x."""
    f = L_ * 2 * (E + H) * 4 * H + 2 * H * V_
    return 3 * f if train else f


def _frac(flops_per_token, tokens_per_s):
    """Whole-step fraction of the fp32 MFMA peak (157.3 TFLOP/s) from SURVEY 8(d)'s model FLOPs per token: {"tflops", "frac"}
    (the headline's `step_roofline` spells the same quantity out)."""
    tf = flops_per_token * tokens_per_s / 1e12
    return {"tflops": round(tf, 2), "frac": round(tf / PEAK_F32_MFMA_TFLOPS, 4)}


def _train_leg(model, kl_fn, seq, Bc, lr, steps, warm, dev, engine, ops, timed_tags=False, vocab=V, flops_per_token=None):
    """tokens/s of engine.Trainer steps on a synthetic AMI-shaped stream (same step as the headline)."""
    from bayeslms_amd.data import batchify, get_batch, synthetic_corpus
    from bayeslms_amd.model import repackage_hidden
    tagged = 5 if timed_tags else 0  # the event brackets of the recurrences are taken over extra steps AFTER the timed region
    stream = synthetic_corpus(vocab, Bc * ((steps + warm + tagged) * seq + 1) + 17, seed=1111)
    train = batchify(stream, Bc, dev)
    tr = engine.Trainer(model, lr=lr, clip=CLIP, kl_scale=float(seq) / train.size(0), seed=1111)
    is_rnn = hasattr(model, "init_hidden")
    hidden = model.init_hidden(Bc) if is_rnn else None
    timer = ops.KernelTimer() if timed_tags else None
    for i in range(warm + steps + tagged):
        if i == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        if i == warm + steps:
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            ops.set_kernel_timer(timer)
        data, tgt = get_batch(train, i * seq, seq)
        if is_rnn:
            hidden = repackage_hidden(hidden)
        loss, _, hidden = tr.step(data, tgt, hidden=hidden, kl_fn=kl_fn)
    torch.cuda.synchronize()
    if not tagged:
        el = time.perf_counter() - t0
    ops.set_kernel_timer(None)
    out = {"value": round(steps * seq * Bc / el, 1), "unit": "tokens/s", "ms_per_step": round(1e3 * el / steps, 3),
           "steps": steps, "warmup": warm, "final_loss": round(float(loss), 4)}
    if flops_per_token:
        out["step_roofline"] = _frac(flops_per_token, out["value"])
    return out, (timer.summary() if timer is not None else {})


def _eval_leg(model, seq, dev, engine, vocab, flops_per_token, windows=12):
    """engine.evaluate (train.py:441-458: eval batch 20, mean weights) on held-out synthetic text: tokens/s."""
    from bayeslms_amd.data import batchify, synthetic_corpus
    valid = batchify(synthetic_corpus(vocab, 20 * (windows * seq + 1), seed=2222), 20, dev)
    engine.evaluate(model, valid, seq)  # warm-up on the pass itself: a stateless model's windows run in groups, whose products have the group's row count
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = engine.evaluate(model, valid, seq)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    tps = (valid.size(0) - 1) * 20 / el
    return {"value": round(tps, 1), "unit": "tokens/s", "eval_batch": 20, "seq_len": seq, "loss": round(loss, 4),
            "step_roofline": _frac(flops_per_token, tps)}


def lstm_cpu_baseline(steps=3, warm=1):
    """BASELINE.json configs[0] on the host cores: the oracle's LSTM training step (fwd + CE + bwd + clip + SGD, dropout
    0.2 from torch's generator) at the reference's own CPU-runnable size -- 2 x 1024, V = 10,000, batch 20, seq_len 35."""
    from bayeslms_amd import model as M
    from bayeslms_amd.data import synthetic_corpus
    from oracle import bayes_oracle as O
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    ncores = min(avail, 16)
    torch.set_num_threads(ncores)
    torch.manual_seed(1111)
    Vc, Bc, Tc = 10000, 20, 35
    m = M.RNNModel("LSTM", Vc, 1024, 1024, 2, 0.2, True)
    names = [k for k, _ in m.named_parameters() if k != "decoder.weight"]
    sd = {k: v.detach().clone().requires_grad_(k in names) for k, v in m.state_dict().items()}
    sd["decoder.weight"] = sd["encoder.weight"]
    del m
    total = warm + steps
    stream = synthetic_corpus(Vc, Bc * (Tc * total + 1), seed=1111)
    data = stream[: Bc * (Tc * total + 1) // Bc * Bc].view(Bc, -1).t().contiguous()
    hidden = (torch.zeros(2, Bc, 1024), torch.zeros(2, Bc, 1024))
    bufs = [None] * len(names)
    times = []
    for s_ in range(total):
        src, tgt = data[s_ * Tc:(s_ + 1) * Tc], data[s_ * Tc + 1:(s_ + 1) * Tc + 1].reshape(-1)
        t0 = time.perf_counter()
        for k in names:
            sd[k].grad = None
        hidden = tuple(h.detach() for h in hidden)
        logits, hidden = O.rnn_lm_train(src, hidden, sd, 0.2)
        loss = torch.nn.functional.cross_entropy(logits.view(-1, Vc), tgt)
        loss.backward()
        O.clip_and_sgd([sd[k] for k in names], [sd[k].grad for k in names], bufs, 1.0, CLIP)
        times.append(time.perf_counter() - t0)
    med = sorted(times[warm:])[steps // 2]
    return {"value": round(Bc * Tc / med, 1), "unit": "tokens/s", "cores": ncores, "kind": "port",
            "sample": "oracle/bayes_oracle.py LSTM train step (fwd+CE+bwd+clip+SGD, dropout 0.2 on), 2x1024 V=10000 batch 20 "
                      "seq_len 35, median of %d steps after %d warm-up, %d threads; BASELINE.md has the reference itself at 935 "
                      "tokens/s on the build container's 8 cores" % (steps, warm, ncores)}


def synthetic_nbest(n_utt, n_hyp, vocab_size, seed=7):
    """SURVEY 8(d) scoring workload: n_utt utterances x n_hyp-best, hypothesis length 1 + Poisson(7) clipped to [1, 60]
    (AMI-shaped), the hypotheses of an utterance differing in up to three words.  -> (OrderedDict, vocab dict, n tokens)"""
    import random
    from collections import OrderedDict
    import numpy as np
    rnd = random.Random(seed)
    rs = np.random.RandomState(seed)
    words = ["w%d" % i for i in range(vocab_size - 2)]
    vocab = {w: i + 2 for i, w in enumerate(words)}
    vocab["<s>"], vocab["<unk>"] = 0, 1
    nbest, ntok = OrderedDict(), 0
    for u in range(n_utt):
        ln = int(np.clip(1 + rs.poisson(7), 1, 60))
        base = [rnd.choice(words) for _ in range(ln)]
        hyps = []
        for _ in range(n_hyp):
            h = list(base)
            for _ in range(rnd.randint(0, 3)):
                h[rnd.randrange(len(h))] = rnd.choice(words)
            hyps.append(" ".join(h))
            ntok += len(h) + 1  # + the sentence end the scorer appends
        nbest["utt%04d" % u] = hyps
    return nbest, vocab, ntok


def cli_leg(dev, args, headline_ms):
    """What a user of `python -m bayeslms_amd.train` sees: the CLI's own `ms/batch` log value on a synthetic corpus
    written to disk in the reference's file format (words.txt, train/valid/test.txt), the headline configuration."""
    import tempfile
    from bayeslms_amd import train as TR
    from bayeslms_amd.data import synthetic_corpus
    nb = 45  # batches of the one epoch: log lines after 20 and 40
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "words.txt"), "w") as f:
            f.write("<s> 0\n<unk> 1\n" + "".join("w%d %d\n" % (i, i) for i in range(2, V)))
        for split, n, seed in (("train", B_PER_GPU * (nb * T + 1), 1111), ("valid", 20 * (2 * T + 1), 2222), ("test", 20 * (2 * T + 1), 3333)):
            ids = synthetic_corpus(V, n, seed=seed).tolist()
            with open(os.path.join(d, split + ".txt"), "w") as f:
                line = []
                for t in ids:
                    if t == 0:
                        f.write(" ".join(line) + "\n")
                        line = []
                    else:
                        line.append("w%d" % t)
                f.write(" ".join(line) + "\n")
        hist = {}
        argv = ["--data", d, "--cuda", "--model", "Transformer", "--emsize", str(D_MODEL), "--nhid", str(D_FF), "--nlayers",
                str(NLAYERS), "--nhead", str(NHEAD), "--lr", str(LR), "--dropout", str(DROPOUT), "--seq_len", str(T), "--clip",
                str(CLIP), "--batch-size", str(B_PER_GPU), "--epochs", "1", "--uncertainty", "Bayesian", "--T_bayes_pos", "FFN",
                "--tied", "--log-interval", "20", "--save", os.path.join(d, "model.pt")]
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            TR.main(argv, history=hist)
    ms = hist["ms_per_batch"][-1]  # the second interval: batches 21-40 (the first contains lazy initialisation)
    return {"id": "cli", "config": "python -m bayeslms_amd.train, the headline configuration on a synthetic corpus in the reference's file "
                      "format: the CLI's own `ms/batch` log value (second log interval of 20 batches)",
            "value": round(ms, 3), "unit": "ms/batch", "tokens_per_s": round(B_PER_GPU * T / ms * 1e3, 1),
            "bench_ms_per_step": round(headline_ms, 3), "ratio_to_bench_step": round(ms / headline_ms, 4),
            "valid_loss": round(hist["valid_loss"][-1], 4)}


def level1_leg(dev, args, headline_ms):
    """INTEGRATION.md level 1 priced: the headline model under the REFERENCE's loop shape (train.py:306-438) -- only `import model`
    swapped: nn.CrossEntropyLoss() on the (8192 x 33000) logits (ops.Logits: the engine's kernels, non-destructively),
    optimizer.zero_grad() (gradients to None: the in-place
    weight-gradient kernels re-create their zeroed buffers every step), model...kl_divergence() added to the loss and
    back-propagated by autograd, torch.nn.utils.clip_grad_norm_, torch.optim.SGD(momentum 0.9) -- beside engine.Trainer."""
    import torch.nn as nn
    from bayeslms_amd import model as M
    from bayeslms_amd.data import batchify, get_batch, synthetic_corpus
    torch.manual_seed(1111)
    m = M.BayesTransformerModel(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, True, "FFN").to(dev)
    Bc, steps, warm = B_PER_GPU, max(args.steps, 10), max(args.warmup, 5)
    train = batchify(synthetic_corpus(V, Bc * ((steps + warm) * T + 1) + 17, seed=1111), Bc, dev)
    crit = nn.CrossEntropyLoss()
    opt = torch.optim.SGD(m.parameters(), lr=LR, momentum=0.9, weight_decay=0)
    m.train()

    def loop(read_loss_every_step):
        total = 0.0
        for i in range(steps + warm):
            if i == warm:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            data, tgt = get_batch(train, i * T, T)
            opt.zero_grad()
            out = m(data)
            loss = crit(out.view(-1, V), tgt) + m.transformerlayers[0].linear2.kl_divergence() / len(train) * T
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), CLIP)
            opt.step()
            if read_loss_every_step:
                total += loss.item()  # train.py:422: one host synchronisation per step
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / steps, loss
    ms, loss = loop(True)        # the loop as the reference has it
    ms_nosync, _ = loop(False)   # the same loop without the per-step read-back (what r04 priced)
    return {"id": "level1", "config": "INTEGRATION.md level 1: `from bayeslms_amd.model import *` under the reference's own loop (nn.CrossEntropyLoss() -- on the "
                      "models' ops.Logits output it runs the engine's cross-entropy kernels --, zero_grad(), clip_grad_norm_, optim.SGD, "
                      "total_loss += loss.item() every step as train.py:422), headline configuration",
            "value": round(T * Bc / ms * 1e3, 1), "unit": "tokens/s", "ms_per_step": round(ms, 3), "loss_finite": bool(torch.isfinite(loss)),
            "vs_engine_trainer_step": round(ms / headline_ms, 4), "step_roofline": _frac(tlm_flops_per_token(T), T * Bc / ms * 1e3),
            "without_loss_item": {"value": round(T * Bc / ms_nosync * 1e3, 1), "ms_per_step": round(ms_nosync, 3),
                                  "vs_engine_trainer_step": round(ms_nosync / headline_ms, 4)}}


def search_leg(kind, dev, steps=8, warm=3):
    """Architecture-search window (Architect.step on a validation window + network step) at the
    reference's full sizes, under this run's clock (tools/bench_search.py is the stand-alone form)."""
    import types
    from bayeslms_amd import engine, model_search_bayes as S, train_search_bayes as TS
    from bayeslms_amd.architect import Architect
    from bayeslms_amd.model import repackage_hidden
    torch.manual_seed(11)
    if kind == "tlm":
        Ts = T
        m = S.GaussTransModelSearch(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, True).to(dev)
        a = types.SimpleNamespace(model="Transformer", T_bayes_pos="FFN", uncertainty="none", L_bayes_pos=0)
    else:
        Ts = 35
        m = S.BayesLSTMModelSearch("LSTM", V, 1024, 1024, 2, DROPOUT, True).to(dev)
        a = types.SimpleNamespace(model="LSTM", T_bayes_pos="none", uncertainty="none", L_bayes_pos=1)
    TS.freeze_unused(a, m)
    kl_fn = TS.kl_selector(a)
    arch = Architect(m, V, types.SimpleNamespace(wdecay=5e-7, clip=1.0, arch_lr=3e-3, arch_wdecay=1e-3))
    tr = engine.Trainer(m, lr=0.1, clip=1.0, kl_scale=Ts / 65536.0, weight_decay=TS.SGD_WEIGHT_DECAY)
    data = torch.randint(0, V, (Ts + 1, B_PER_GPU), device=dev)
    x, y = data[:Ts], data[1:].reshape(-1)
    hidden = m.init_hidden(B_PER_GPU) if kind == "lstm" else None
    hv = m.init_hidden(B_PER_GPU) if kind == "lstm" else None
    for s_ in range(warm + steps):
        if s_ == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        m.train()
        m.set_step(2 * s_ + 1)
        arch.step(x, y, x, y, None, False, hv)
        if kind == "tlm":
            for layer in m.transformerlayers:
                layer.gpnn.sample = True
        else:
            hidden = repackage_hidden(hidden)
        _, _, hidden = tr.step(x, y, hidden, kl_fn, philox_step=2 * s_)
        if kind == "tlm":
            for layer in m.transformerlayers:
                layer.gpnn.sample = False
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    name = ("GaussTransModelSearch 6L d=512 ff=4096 V=33000, T 128, B 64" if kind == "tlm"
            else "BayesLSTMModelSearch E=H=1024 V=33000, T 35, B 64")
    return {"id": "search_" + kind, "config": "architecture search (train_search_bayes.py), %s: one window = Architect.step + network step" % name,
            "value": round(Ts * B_PER_GPU / dt, 1), "unit": "tokens/s", "ms_per_window": round(1e3 * dt, 3), "windows": steps}


def deterministic_leg(dev, args, engine, M, ops, headline_ms):
    """The headline step in deterministic mode (ops.set_deterministic: one K slice per GEMM tile, fixed-order column sums / KL /
    embedding gradient; tests/test_gpu_deterministic.py holds two such runs to bit-identical parameters): what it costs."""
    from bayeslms_amd import train as TR
    from types import SimpleNamespace
    torch.manual_seed(1111)
    m = M.BayesTransformerModel(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, True, "FFN").to(dev)
    kl = TR.kl_selector(SimpleNamespace(model="Transformer", uncertainty="Bayesian", T_bayes_pos="FFN", L_bayes_pos=0))
    ops.set_deterministic(True)
    try:
        r, _ = _train_leg(m, kl, T, B_PER_GPU, LR, max(args.steps, 5), args.warmup, dev, engine, ops, flops_per_token=tlm_flops_per_token(T))
    finally:
        ops.set_deterministic(False)
    r["id"] = "cfg2_deterministic"
    r["config"] = ("the headline configuration in deterministic mode (BLM_DETERMINISTIC=1 / ops.set_deterministic): every reduction in a "
                   "fixed order, two runs from one seed bit-identical; not the default")
    r["vs_headline_step"] = round(r["ms_per_step"] / headline_ms, 4)
    return r


def extra_configs(dev, args, engine, M, ops, headline_ms):
    """Reported AFTER the headline, never part of `value`: the other BASELINE.json configurations that fit one GPU, the
    reference recipes' own shape (run_nnlm_ami_{tm,lstm}.sh: --seq_len 100 --batch-size 32), evaluation, the CLI, n-best
    rescoring and the architecture search, all under the same clock as the headline run.  fp32, same Trainer step,
    synthetic data; every training / evaluation leg carries `step_roofline` = SURVEY 8(d) model FLOPs per token x
    tokens/s against the fp32 MFMA peak."""
    from types import SimpleNamespace
    from collections import OrderedDict
    from bayeslms_amd import compute_sentence_scores as css, train as TR
    res = []
    ns = lambda **k: SimpleNamespace(**{**dict(model="Transformer", uncertainty="none", T_bayes_pos="none", L_bayes_pos=0,  # noqa: E731
                                               T_gauss_pos=3, L_gauss_pos="00", L_v_pos="11", T_v_pos=0), **k})
    steps = max(args.steps, 5)
    floor_us = lambda Bc: 2.0 * Bc * 4096 * 1024 / (PEAK_F32_MFMA_TFLOPS * 1e12) * 1e6  # noqa: E731

    def lstm_steps(r, kt, Tl, Bc):
        fwd = kt.get("lstm_seq_fwd T=%d" % Tl, {}).get("avg_ms")
        bwd = kt.get("lstm_seq_bwd T=%d" % Tl, {}).get("avg_ms")
        sf, sb = kt.get("lstm_stack2_fwd T=%d" % Tl, {}).get("avg_ms"), kt.get("lstm_stack2_bwd T=%d" % Tl, {}).get("avg_ms")
        r["lstm_step_times_from"] = "event brackets over 5 extra steps after the timed region (inside it they cost the host-bound legs 4-8 %)"
        if sf is not None:  # the two layers ran as a wavefront on two streams (ops.lstm_stack2: B <= 32 and T >= 32)
            r.update({"lstm_layers": "wavefront on two streams (ops.lstm_stack2)",
                      # whole two-layer recurrence incl. layer 2's per-chunk input GEMMs / dgrad GEMMs, per time step and LAYER
                      "lstm_step_fwd_us_effective": round(1e3 * sf / Tl / 2, 2),
                      "lstm_step_bwd_us_effective": None if sb is None else round(1e3 * sb / Tl / 2, 2),
                      "lstm_step_mfma_floor_us": round(floor_us(Bc), 2)})
            return
        r.update({"lstm_step_fwd_us": None if fwd is None else round(1e3 * fwd / Tl, 2),
                  "lstm_step_bwd_us": None if bwd is None else round(1e3 * bwd / Tl, 2),
                  "lstm_step_mfma_floor_us": round(floor_us(Bc), 2),
                  "lstm_step_fwd_frac_of_floor": None if fwd is None else round(floor_us(Bc) / (1e3 * fwd / Tl), 3)})
    # --- configs[0]: 2-layer 1024-hidden standard LSTM LM, V 10k, batch 20, seq_len 35 (the reference's CPU-runnable case)
    torch.manual_seed(1111)
    m = M.RNNModel("LSTM", 10000, 1024, 1024, 2, DROPOUT, True).to(dev)
    r, kt = _train_leg(m, None, 35, 20, 1.0, 2 * steps, max(args.warmup, 20), dev, engine, ops, timed_tags=True, vocab=10000,
                       flops_per_token=lstm_flops_per_token(10000))
    r["id"] = "cfg0_lstm_train"
    r["config"] = ("BASELINE.json configs[0]: 2-layer 1024-hidden standard LSTM LM (--uncertainty none) tied, V=10000, batch 20, "
                   "seq_len 35, dropout 0.2, clip 1.0, SGD momentum 0.9")
    lstm_steps(r, kt, 35, 20)
    if not args.no_cpu_baseline:
        try:
            r["cpu_baseline"] = lstm_cpu_baseline()
        except Exception as e:  # noqa: BLE001
            r["cpu_baseline"] = {"error": repr(e)}
    res.append(r)
    del m
    # --- configs[1]: Bayesian LSTM LM (--uncertainty Bayesian --L_bayes_pos 3), 2x1024, B 64, T 35, V 33k
    torch.manual_seed(1111)
    m = M.BayesRNNModel("LSTM", V, 1024, 1024, 2, DROPOUT, True, 3).to(dev)
    kl_lstm = TR.kl_selector(ns(model="LSTM", uncertainty="Bayesian", L_bayes_pos=3))
    r, kt = _train_leg(m, kl_lstm, 35, B_PER_GPU, 1.0, 2 * steps, max(args.warmup, 20), dev, engine, ops, timed_tags=True,
                       flops_per_token=lstm_flops_per_token(V))
    r["id"] = "cfg1_bayes_lstm_train"
    r["config"] = ("BASELINE.json configs[1]: Bayesian LSTM LM (--uncertainty Bayesian --L_bayes_pos 3) 2x1024 tied, "
                   "V=33000, batch 64, seq_len 35, dropout 0.2, clip 1.0, SGD momentum 0.9")
    lstm_steps(r, kt, 35, B_PER_GPU)
    res.append(r)
    # the reference recipe's own shape (run_nnlm_ami_lstm.sh:24,100: --seq_len 100 --batch-size 32)
    r, kt = _train_leg(m, kl_lstm, 100, 32, 1.0, steps, max(args.warmup, 8), dev, engine, ops, timed_tags=True,
                       flops_per_token=lstm_flops_per_token(V))
    r["id"] = "recipe_lstm_train"
    r["config"] = ("recipe shape (run_nnlm_ami_lstm.sh: --seq_len 100 --batch-size 32): Bayesian LSTM LM --L_bayes_pos 3, 2x1024 "
                   "tied, V=33000")
    lstm_steps(r, kt, 100, 32)
    res.append(r)
    e = _eval_leg(m, 35, dev, engine, V, lstm_flops_per_token(V, train=False))
    e["id"] = "cfg1_evaluate"
    e["config"] = "evaluate() (train.py:441-458), the configs[1] LSTM, eval batch 20, seq_len 35, mean weights"
    res.append(e)
    # LSTM 20-best rescoring (mean weights; the carried state makes it the latency-bound scorer)
    n_utt, n_hyp = 1000, 20
    nbest, vocab, ntok = synthetic_nbest(n_utt, n_hyp, V)
    sub = OrderedDict(list(nbest.items())[:150])  # warm-up: enough utterances to reach the full packed-batch size (16384 padded tokens: allocator, GEMM plans)

    def hyp_rate(model, mtype, mc, fl):
        css.compute_scores_batched(sub, model, vocab, mtype, dev, mc_samples=mc)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        css.compute_scores_batched(nbest, model, vocab, mtype, dev, mc_samples=mc)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        return {"value": round(n_utt * n_hyp / el, 1), "unit": "hypotheses/s", "tokens_per_s": round(ntok / el, 1),
                "step_roofline": _frac(fl * max(mc, 1), ntok / el)}
    wl = "%d utterances x %d-best, lengths 1 + Poisson(7) clipped to [1, 60] (SURVEY 8(d))" % (n_utt, n_hyp)
    r = hyp_rate(m, "LSTM", 0, lstm_flops_per_token(V, train=False))
    r["id"] = "cfg1_rescore"
    r["config"] = ("n-best rescoring with the configs[1] LSTM: %s, mean weights, hidden state carried across utterances "
                   "(compute_sentence_scores --batched)" % wl)
    res.append(r)
    # --interpolation_flag 1 (run_nnlm_ami_tm.sh:30-31,133-134; scorer :157-168): two LSTMs, logits interpolated 0.8 / 0.2 --
    # both decoders + the cross entropy in ONE launch over packed operands (blm_linear_nll2), no logits stored
    torch.manual_seed(2222)
    m2 = M.RNNModel("LSTM", V, 1024, 1024, 2, DROPOUT, True).to(dev)

    def hyp_rate2(model, model_2, mtype, fl):
        css.compute_scores_batched(sub, model, vocab, mtype, dev, model_2, 0.8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        css.compute_scores_batched(nbest, model, vocab, mtype, dev, model_2, 0.8)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        return {"value": round(n_utt * n_hyp / el, 1), "unit": "hypotheses/s", "tokens_per_s": round(ntok / el, 1),
                "step_roofline": _frac(fl, ntok / el)}
    r = hyp_rate2(m, m2, "LSTM", 2 * lstm_flops_per_token(V, train=False))
    r["id"] = "cfg1_rescore_interp"
    r["config"] = ("--interpolation_flag 1: %s, the configs[1] Bayesian LSTM interpolated with a standard 2x1024 LSTM "
                   "(--inter_alpha 0.8), both decoders + cross entropy in one launch (blm_linear_nll2), state carried" % wl)
    res.append(r)
    del m, m2
    torch.cuda.empty_cache()
    # --- the reference recipe's own Transformer shape (run_nnlm_ami_tm.sh:22,98-99: --seq_len 100 --batch-size 32)
    torch.manual_seed(1111)
    m = M.BayesTransformerModel(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, True, "FFN").to(dev)
    r, _ = _train_leg(m, TR.kl_selector(ns(uncertainty="Bayesian", T_bayes_pos="FFN")), 100, 32, LR, steps, args.warmup, dev, engine,
                      ops, flops_per_token=tlm_flops_per_token(100))
    r["id"] = "recipe_tlm_train"
    r["config"] = ("recipe shape (run_nnlm_ami_tm.sh: --seq_len 100 --batch-size 32): Bayesian Transformer LM --T_bayes_pos FFN, "
                   "6L d_model=512 d_ff=4096 V=33000")
    res.append(r)
    e = _eval_leg(m, T, dev, engine, V, tlm_flops_per_token(T, train=False))
    e["id"] = "cfg2_evaluate"
    e["config"] = "evaluate() (train.py:441-458), the headline Transformer, eval batch 20, seq_len 128, mean weights"
    res.append(e)
    r = hyp_rate(m, "Transformer", 0, tlm_flops_per_token(8, train=False))
    r["id"] = "cfg4_bayes_tlm_rescore"
    r["config"] = "configs[4] n-best rescoring, Bayesian Transformer-FFN, %s, mean weights" % wl
    res.append(r)
    r = hyp_rate(m, "Transformer", 8, tlm_flops_per_token(8, train=False))
    r["id"] = "cfg4_bayes_tlm_rescore_mc8"
    r["config"] = ("configs[4] n-best rescoring, Bayesian Transformer-FFN, %s, 8 Monte-Carlo weight samples "
                   "(score = -log mean_s exp(-NLL_s), oracle-checked)" % wl)
    res.append(r)
    torch.manual_seed(2222)
    m2 = M.TransformerModel(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, "gelu", True).to(dev)
    r = hyp_rate2(m, m2, "Transformer", 2 * tlm_flops_per_token(8, train=False))
    r["id"] = "cfg2_rescore_interp"
    r["config"] = ("--interpolation_flag 1 (run_nnlm_ami_tm.sh:30-31,133-134): %s, Bayesian Transformer-FFN interpolated with a "
                   "standard Transformer (--inter_alpha 0.8), both decoders + cross entropy in one launch (blm_linear_nll2)" % wl)
    res.append(r)
    del m2
    del m
    torch.cuda.empty_cache()
    # --- configs[4] training leg: GP Transformer (--uncertainty Gaussian --T_gauss_pos 3), cfg3 shape
    torch.manual_seed(1111)
    m = M.GaussTransformerModel(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, True, 3).to(dev)
    r, _ = _train_leg(m, TR.kl_selector(ns(uncertainty="Gaussian", T_gauss_pos=3)), T, B_PER_GPU, LR, steps, args.warmup, dev,
                      engine, ops, flops_per_token=tlm_flops_per_token(T))
    r["id"] = "cfg4_gp_tlm_train"
    r["config"] = ("BASELINE.json configs[4] training leg on 1 GPU: GP Transformer LM (--uncertainty Gaussian --T_gauss_pos 3) 6L "
                   "d_model=512 d_ff=4096 V=33000, seq_len 128, batch 64")
    res.append(r)
    r = hyp_rate(m, "Transformer", 0, tlm_flops_per_token(8, train=False))
    r["id"] = "cfg4_gp_tlm_rescore"
    r["config"] = ("configs[4] n-best rescoring, GP Transformer, %s, mean weights (the reference's inference: GPNN.sample is "
                   "never raised)" % wl)
    res.append(r)
    r = hyp_rate(m, "Transformer", 8, tlm_flops_per_token(8, train=False))
    r["id"] = "cfg4_gp_tlm_rescore_mc8"
    r["config"] = ("BASELINE.json configs[4] inference leg as written: GP Transformer (--T_gauss_pos 3), %s, 8 Monte-Carlo weight "
                   "samples -- GPNN.sample raised for the call, coef / weights / bias re-drawn per sample (reference "
                   "model.py:1871-1883), score = -log mean_s exp(-NLL_s), oracle-checked" % wl)
    res.append(r)
    for g in m.modules():  # the same training leg with the GP layer's tensors re-sampled every step (train --gp-sample 1)
        if isinstance(g, M.GPNN):
            g.sample = True
    r, _ = _train_leg(m, TR.kl_selector(ns(uncertainty="Gaussian", T_gauss_pos=3)), T, B_PER_GPU, LR, steps, args.warmup, dev,
                      engine, ops, flops_per_token=tlm_flops_per_token(T))
    r["id"] = "cfg4_gp_tlm_train_gpsample"
    r["config"] = ("configs[4] training leg with GPNN.sample raised (--gp-sample 1; the reference's train.py leaves it False): "
                   "GP Transformer LM --T_gauss_pos 3, coef / weights / bias = mean + exp(lgstd) eps every step, seq_len 128, batch 64")
    res.append(r)
    del m
    torch.cuda.empty_cache()
    # --- configs[4] names "Variational (--T_v_pos 11)" beside the GP Transformer.  The reference's VTransformerModel builds NO encoder
    # layer for that value (model.py:2808-2897; 2 and 3 build nlayers - 1, 1 crashes in kl_divergence): embedding -> decoder, no KL
    # term, nothing to sample.  That model's training step, as the reference's flags give it:
    torch.manual_seed(1111)
    m = M.VTransformerModel(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, True, 11).to(dev)
    r, _ = _train_leg(m, TR.kl_selector(ns(uncertainty="Variational", T_v_pos=11)), T, B_PER_GPU, LR, steps, args.warmup, dev,
                      engine, ops, flops_per_token=tlm_flops_per_token(T, L_=0))
    r["id"] = "cfg4_var_tlm_v11_train"
    r["config"] = ("BASELINE.json configs[4], its Variational half: --uncertainty Variational --T_v_pos 11 builds a VTransformerModel "
                   "WITHOUT encoder layers in the reference (model.py:2808-2897, quirk kept and pinned by fixture vtransformer_11): "
                   "embedding + positional encoding + tied decoder, V=33000, seq_len 128, batch 64; no KL term (train.py:387-396), "
                   "nothing to sample (--mc-samples refuses it)")
    res.append(r)
    del m
    torch.cuda.empty_cache()
    # --- the CLI itself, and the architecture search
    for name, fn in (("cfg2_deterministic", lambda: deterministic_leg(dev, args, engine, M, ops, headline_ms)),
                     ("cli", lambda: cli_leg(dev, args, headline_ms)), ("level1", lambda: level1_leg(dev, args, headline_ms)),
                     ("search_tlm", lambda: search_leg("tlm", dev)),
                     ("search_lstm", lambda: search_leg("lstm", dev))):
        try:
            res.append(fn())
        except Exception as e:  # noqa: BLE001
            res.append({"id": name, "error": repr(e)})
        torch.cuda.empty_cache()
    return res


def run_dp_extras(args, engine, rank, world, out, legs):
    """The extra legs of a multi-rank run (every rank calls `legs()`), arranged so that they can no longer cost the headline:
    rank 0 holds the finished line (`out`), and a leg that does not return inside --dp-extras-budget-s (or the deadline) ends
    in that line, marked `extra_configs.error`, with exit code 0 on every rank (arm_deadline.fire).  -> the legs' records."""
    import copy
    import threading
    if rank == 0:
        PENDING["line"] = compact_line(copy.deepcopy(out), legend=False) if "baseline_configs" not in out else copy.deepcopy(out)
    PENDING["headline_done"] = True
    engine.heartbeat("headline ok; extra legs", rank)
    budget = (threading.Timer(args.dp_extras_budget_s, PENDING["fire"], args=("of the extra legs, %.0f s (--dp-extras-budget-s)" % args.dp_extras_budget_s,))
              if PENDING["fire"] is not None else None)
    if budget is not None:
        budget.daemon = True
        budget.start()
    _maybe_hang(args, rank, "extras")
    try:
        ex = legs()
    except Exception as e:  # noqa: BLE001
        ex = {"error": repr(e)}
    if budget is not None:
        budget.cancel()
    return ex


def dp_extra_configs(dev, args, engine, M, ops, rank, world, main_reducer):
    """BASELINE.json configs[4] on N GPUs -- "GP Transformer LM (--uncertainty Gaussian --T_gauss_pos 3) ..., 8xMI355X DP, n-best
    rescoring inference path with 8 MC weight samples" -- as two legs every rank runs after the headline (same barrier +
    max-over-ranks brackets; `value` = what all ranks processed / that time):
      * cfg4_gp_tlm_train_dp: the GP Transformer's training step data-parallel, 64 columns per GPU, through the same
        GradReducer / LateRows settings the headline's timed region ran with;
      * cfg4_gp_tlm_rescore_mc8_dp: rank r rescores ITS OWN archive of 1000 utterances x 20-best with 8 Monte-Carlo weight
        samples -- the product's placement (compute_sentence_scores --job: stage 6 starts nj independent jobs over archives.JOB,
        lmrescore_nbest_pytorchnn_cuda.sh:199-203; replicas only, no collective on the data path).
    A failure is recorded per leg; the legs end in the same collectives on every rank whether they failed or not."""
    from collections import OrderedDict
    from types import SimpleNamespace as ns
    from bayeslms_amd import compute_sentence_scores as css
    from bayeslms_amd import train as TR
    from bayeslms_amd.data import batchify, get_batch, synthetic_corpus
    on_dev = args.backend == "nccl"
    res = []

    def agree(ok, el):
        """-> (every rank succeeded, the slowest rank's time): ONE collective, entered by every rank on every path."""
        t = torch.tensor([0.0 if ok else 1.0, el], dtype=torch.float64, device=dev if on_dev else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t[0].item()) == 0.0, float(t[1].item())

    # --- training leg
    Bc, steps, warm = args.batch, args.steps, min(args.warmup, 3)
    m = None
    rec = {"id": "cfg4_gp_tlm_train_dp", "n_gpus": world,
           "config": "BASELINE.json configs[4] training leg data-parallel over %d GPUs: GP Transformer LM (--uncertainty Gaussian "
                     "--T_gauss_pos 3) 6L d_model=512 d_ff=4096 V=33000, seq_len 128, %d columns per GPU (global batch %d)"
                     % (world, Bc, Bc * world)}
    try:
        stream = synthetic_corpus(V, Bc * world * ((steps + warm) * T + 1) + 17, seed=1111)
        train = batchify(stream, Bc * world, dev, rank, world)
        torch.manual_seed(1111)
        m = M.GaussTransformerModel(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, True, 3).to(dev)
        tr = engine.Trainer(m, lr=LR, clip=CLIP, kl_scale=float(T) / float(train.size(0)), seed=1111, rank=rank, world=world,
                            overlap=bool(main_reducer.overlap), late_rows=main_reducer.late is not None)
        tr.reducer.comm_plan = main_reducer.comm_plan  # what the headline's calibration steps kept
        kl = TR.kl_selector(ns(model="Transformer", uncertainty="Gaussian", T_bayes_pos="none", L_bayes_pos=0, T_gauss_pos=3,
                               L_gauss_pos="00", L_v_pos="11", T_v_pos=0))
        last = {}

        def one(i):
            data, targets = get_batch(train, i * T, T)
            last["loss"] = tr.step(data, targets, kl_fn=kl)[0]
        for i in range(warm):
            one(i)
        ms = _timed_steps(one, steps, warm, dev, world)  # barrier + synchronize on both sides, max over ranks
        fp = tr.flat.flat_param
        mine = torch.stack([fp.double().sum(), fp.double().abs().sum()]).to(dev if on_dev else "cpu")
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        rec.update({"value": round(T * Bc * world / (ms * 1e-3), 1), "unit": "tokens/s", "ms_per_step": ms, "steps": steps, "warmup": warm,
                    "final_loss": round(float(last["loss"]), 4),
                    "replicas_identical": all(bool(torch.equal(e, every[0])) for e in every),
                    "step_roofline": _frac(tlm_flops_per_token(T), T * Bc / (ms * 1e-3))})  # per GPU against one GPU's peak
        engine.heartbeat("configs[4] training leg ok (%.3f ms per step)" % ms, rank)
    except Exception as e:  # noqa: BLE001 -- recorded; a rank that is alone in failing ends in the extras' budget (main)
        rec["error"] = repr(e)
    res.append(rec)
    # --- rescoring leg (the model of the training leg where there is one; scoring reads mean + exp(lgstd) eps per sample)
    n_utt, n_hyp, mc = 1000, 20, 8
    rec = {"id": "cfg4_gp_tlm_rescore_mc8_dp", "n_gpus": world,
           "config": "BASELINE.json configs[4] inference leg on %d GPUs: every GPU rescores its own archive (%d utterances x %d-best, "
                     "lengths 1 + Poisson(7) clipped to [1, 60]) with the GP Transformer and 8 Monte-Carlo weight samples "
                     "(GPNN.sample raised for the call); independent jobs as in the recipe's stage 6, no collective on the data path"
                     % (world, n_utt, n_hyp)}
    ok, el, ntok = True, 0.0, 0
    try:
        if m is None:
            torch.manual_seed(1111)
            m = M.GaussTransformerModel(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, True, 3).to(dev)
        nbest, vocab, ntok = synthetic_nbest(n_utt, n_hyp, V, seed=7 + rank)
        sub = OrderedDict(list(nbest.items())[:150])
        css.compute_scores_batched(sub, m, vocab, "Transformer", dev, mc_samples=mc)  # warm-up: allocator, plans, full packed batches
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        css.compute_scores_batched(nbest, m, vocab, "Transformer", dev, mc_samples=mc)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
    except Exception as e:  # noqa: BLE001
        ok = False
        rec["error"] = repr(e)
    all_ok, slowest = agree(ok, el)
    if all_ok:
        rec.update({"value": round(n_utt * n_hyp * world / slowest, 1), "unit": "hypotheses/s", "slowest_rank_s": round(slowest, 3),
                    "tokens_per_s": round(ntok * world / slowest, 1),
                    "step_roofline": _frac(tlm_flops_per_token(8, train=False) * mc, ntok / slowest)})
        engine.heartbeat("configs[4] rescoring leg ok (%.2f s)" % slowest, rank)
    elif "error" not in rec:
        rec["error"] = "another rank failed in this leg"
    res.append(rec)
    return res


def opt_in_modes(model, tr, train, get_batch, steps_total, args, ops, engine):
    """Separately reported, NOT part of `value`: the same step with the GEMM family's matrix instruction switched to
    the opt-in split-bf16 arithmetic (include/bayeslm.h blm_set_gemm_mode).  fp32 operands in HBM and LDS, fp32
    accumulate, same kernels / tiles / epilogues; each operand value is split into 2 (bf16x3) or 3 (bf16x6, an exact
    24-bit representation) bf16 parts when a wave reads its fragment."""
    import math
    res = []
    data, targets = get_batch(train, 0, T)

    def eval_loss():
        model.eval()
        with torch.no_grad():
            out = model(data)
            loss, _ = ops.cross_entropy(out.view(-1, out.shape[-1]), targets)
        return float(loss)
    for mode in ("bf16x6", "bf16x3"):
        try:
            ref = eval_loss()  # fp32 mode, the weights as they are now
            ops.set_gemm_mode(mode)
            loss_m = eval_loss()
            timer = ops.KernelTimer()
            for i in range(max(args.warmup, 10)):  # the first steps in a new mode load its code objects and settle the clocks (354-500 k seen with 5)
                ops.set_kernel_timer(None)
                d, t = get_batch(train, (i % steps_total) * T, T)
                tr.step(d, t, kl_fn=_kl_fn)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                ops.set_kernel_timer(timer)
                d, t = get_batch(train, ((args.warmup + i) % steps_total) * T, T)
                tr.step(d, t, kl_fn=_kl_fn)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            ops.set_kernel_timer(None)
            kt = timer.summary()
            ms = kt.get("sampled_gemm_fwd", {}).get("avg_ms")
            nprod = 6 if mode == "bf16x6" else 3
            # the split modes draw ~70 W more than fp32 and their step has been seen at 16.5 and at 28.7 ms on different boxes
            # (the fp32 step within 1 % on both): ten more steps, each bracketed on its own, say whether THIS box holds the rate
            each = []
            for i in range(10):
                d, t = get_batch(train, ((args.warmup + args.steps + i) % steps_total) * T, T)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                tr.step(d, t, kl_fn=_kl_fn)
                torch.cuda.synchronize()
                each.append(1e3 * (time.perf_counter() - t1))
            each.sort()
            res.append({
                "gemm_mode": mode, "value": round(args.steps * T * data.shape[1] / el, 1), "unit": "tokens/s",
                "ms_per_step": round(1e3 * el / args.steps, 3),
                "step_ms_min_median_max": [round(each[0], 2), round(each[len(each) // 2], 2), round(each[-1], 2)],
                "eval_loss_rel_diff_vs_f32": abs(loss_m - ref) / abs(ref),
                "sampled_gemm_fwd_ms": None if ms is None else round(ms, 4),
                "sampled_gemm_fwd_fp32_equiv_tflops": None if ms is None else round(2.0 * T * data.shape[1] * D_MODEL * D_FF / (ms * 1e-3) / 1e12, 1),
                "sampled_gemm_fwd_frac_of_bf16_peak": None if ms is None else round(nprod * 2.0 * T * data.shape[1] * D_MODEL * D_FF / (ms * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
                "note": "opt-in, not the parity mode; never part of `value`"})
        finally:
            ops.set_gemm_mode("f32")
    return res


def _kl_fn(mm):
    return mm.transformerlayers[0].linear2.kl_divergence()


_kl_fn.fusable = True


def compact_line(out, legend=True):
    """The driver keeps the last ~8 KB of stdout: the line stays short and ends with what must survive.  Every extra_configs
    entry keeps an `id` and its numbers; its description (`config`) and the notes go to stderr as `[bench legend] id: text`,
    once.  `baseline_configs` -- one object per BASELINE.json configuration, the numbers this run measured for it -- is the
    LAST key of the line."""
    ex = out.get("extra_configs")
    by_id = {}
    err = sys.stderr if legend else open(os.devnull, "w")
    if isinstance(ex, list):
        for r in ex:
            rid = r.get("id", "?")
            by_id[rid] = r
            for k in ("config", "lstm_step_times_from", "lstm_layers", "note"):
                if k in r:
                    err.write("[bench legend] %s.%s: %s\n" % (rid, k, r.pop(k)))
            cb = r.get("cpu_baseline")
            if isinstance(cb, dict) and "sample" in cb:
                err.write("[bench legend] %s.cpu_baseline.sample: %s\n" % (rid, cb.pop("sample")))
    for mode in (out.get("opt_in") if isinstance(out.get("opt_in"), list) else []):
        if "note" in mode:
            err.write("[bench legend] opt_in.%s: %s\n" % (mode.get("gemm_mode"), mode.pop("note")))
    chip = out.get("chip")
    if isinstance(chip, dict) and "note" in chip:
        err.write("[bench legend] chip: %s\n" % chip.pop("note"))
    err.flush()
    if not legend:
        err.close()

    def pick(rid, *keys):
        r = by_id.get(rid)
        if not isinstance(r, dict):
            return None
        if "error" in r:
            return {"error": r["error"][:120]}
        o = {k: r[k] for k in ("value", "unit") if k in r}
        if isinstance(r.get("step_roofline"), dict):
            o["frac"] = r["step_roofline"].get("frac")
        for k in keys:
            if k in r:
                o[k] = r[k]["value"] if (k == "cpu_baseline" and isinstance(r[k], dict) and "value" in r[k]) else r[k]
        return o
    n = out.get("n_gpus", 1)
    headline = {"value": out["value"], "unit": out["unit"], "n_gpus": n, "frac": (out.get("step_roofline") or {}).get("frac"),
                "kernel_frac": (out.get("roofline") or {}).get("frac"), "eval_ppl": out.get("eval_ppl")}
    out["baseline_configs"] = {
        "configs[0]": pick("cfg0_lstm_train", "cpu_baseline"),
        "configs[1]": pick("cfg1_bayes_lstm_train"),
        "configs[2]": headline if n == 1 else None,
        "configs[3]": headline if n > 1 else None,  # the same model data-parallel: `--gpus N` runs (global batch 64 N)
        "configs[4]": ({"train_1gpu": pick("cfg4_gp_tlm_train"), "rescore_mean_weights": pick("cfg4_gp_tlm_rescore"),
                        "rescore_8_mc_samples": pick("cfg4_gp_tlm_rescore_mc8"),
                        "variational_T_v_pos_11_train": pick("cfg4_var_tlm_v11_train")} if n == 1 else
                       {"train_dp": pick("cfg4_gp_tlm_train_dp", "n_gpus", "replicas_identical"),
                        "rescore_8_mc_samples_dp": pick("cfg4_gp_tlm_rescore_mc8_dp", "n_gpus")}),
    }
    return out


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))  # before any GPU call of this process
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (start it as `python bench.py --gpus N` or under "
                         "torch.distributed.run --nproc-per-node N with the same N)" % (args.gpus, world))
    if args.rehearse_launch:
        return rehearse_launch(args, world, rank)
    ndev = torch.cuda.device_count()
    local = local % max(ndev, 1)  # rehearsal of several ranks on one GPU (gloo); one GPU per rank otherwise
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    rccl_env = None
    from bayeslms_amd import engine as _eng
    timer_dl = arm_deadline(args, rank, world)
    if world > 1:
        # bounded rendezvous + collective timeout, RCCL channels pinned before RCCL reads its environment (channel workgroups
        # hold CUs beside the GEMMs), heartbeats `rendezvous ok` / `first all-reduce ok` on stderr (engine.init_distributed)
        rccl_env = _eng.init_distributed(args.backend, dev if args.backend == "nccl" else None, args.dist_timeout_s)
    from bayeslms_amd import engine, model as M, ops
    from bayeslms_amd.data import batchify, get_batch, synthetic_corpus

    Bc = args.batch
    steps_total = args.warmup + args.steps
    n_rows = steps_total * T + 1
    stream = synthetic_corpus(V, Bc * world * n_rows + 17, seed=1111)
    train = batchify(stream, Bc * world, dev, rank, world)  # (rows, Bc) this rank's columns of the global batch
    torch.manual_seed(1111)  # identical initial weights on every rank (CPU init, then copy)
    model = M.BayesTransformerModel(V, D_MODEL, NHEAD, D_FF, NLAYERS, DROPOUT, True, "FFN").to(dev)
    if args.fused_sampling >= 0:
        model.set_fused_sampling(bool(args.fused_sampling))
    kl_scale = float(T) / float(train.size(0))  # train.py:342: / len(train_data) * seq_len
    tr = engine.Trainer(model, lr=LR, clip=CLIP, kl_scale=kl_scale, seed=1111, rank=rank, world=world,
                        overlap=bool(args.dp_overlap), late_rows=bool(args.dp_late_rows))

    def kl_fn(mm):
        return mm.transformerlayers[0].linear2.kl_divergence()
    kl_fn.fusable = True

    # HIP-event brackets cost the step they sit in (~8 us each: tools/timer_cost.py, 9 per step = 0.33 %): inside the timed region
    # only the roofline launch is bracketed (the contract's live measurement); the other tagged launches of `kernels_ms` are
    # bracketed over the last warm-up steps
    side_tags = min(3, args.warmup)
    timer = ops.KernelTimer(only={"sampled_gemm_fwd"}) if side_tags else ops.KernelTimer()
    timer_all = ops.KernelTimer()

    last = {}

    def one(i, timed):
        data, targets = get_batch(train, i * T, T)
        ops.set_kernel_timer(timed)
        loss, kl, _ = tr.step(data, targets, kl_fn=kl_fn)
        last["kl"] = kl
        return loss

    busbw = None
    if world > 1:
        _eng.heartbeat("model built (%d parameters, %d buckets)" % (tr.flat.total, len(tr.reducer.buckets)), rank)
    if world > 1 and args.full:
        # stand-alone all-reduces before training: the whole gradient and one 32 MB bucket (gloo rehearsals: 8 MB, the host moves it)
        cap = None if args.backend == "nccl" else (8 << 20)
        busbw = [_eng.allreduce_busbw(min(tr.flat.total * 4, cap or (1 << 62)), 5, dev),
                 _eng.allreduce_busbw(min(32 << 20, cap or (1 << 62)), 5, dev)]
        _eng.heartbeat("stand-alone all-reduce ok (%.1f MB: busbw %.1f GB/s)" % (busbw[0]["mb"], busbw[0]["busbw_gbps"]), rank)
    for i in range(args.warmup):
        loss = one(i, timer_all if i >= args.warmup - side_tags else None)
    torch.cuda.synchronize()
    autotune = None
    if world > 1:
        _eng.heartbeat("warm-up ok (%d steps)" % args.warmup, rank)
        if args.dp_autotune:
            autotune = dp_autotune(tr.reducer, lambda i: one(i % steps_total, None), 0, dev, world)
            _eng.heartbeat("autotune ok (%s: %s)" % (autotune["picked"], autotune["ms"]), rank)
        dist.barrier()
    torch.cuda.synchronize()
    tr.reducer.measure = world > 1  # event pair per step: last backward kernel -> end of the gradient exchange
    t0 = time.perf_counter()
    for i in range(args.warmup, steps_total):
        loss = one(i, timer)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    ops.set_kernel_timer(None)
    tr.reducer.measure = False
    comm_exposed = tr.reducer.comm_exposed_ms()
    replicas_identical = None
    diag = None
    if world > 1:
        _eng.heartbeat("timed region ok (%d steps)" % args.steps, rank)
        on_dev = args.backend == "nccl"  # a host-staged transport (gloo rehearsals) is handed host tensors (engine.LateRows.begin)
        t = torch.tensor([elapsed], device=dev if on_dev else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        # outside the timed region: are the replicas still in lock step?  Every rank applied the same all-reduced gradient with the
        # same clip + SGD arithmetic, so the parameter buffers must be bit-identical: two checksums per rank, gathered and compared
        fp = tr.flat.flat_param
        mine = torch.stack([fp.double().sum(), fp.double().abs().sum()]).to(dev if on_dev else "cpu")
        every = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        replicas_identical = all(bool(torch.equal(e, every[0])) for e in every)
    if args.dump_outputs and rank == 0:  # before anything else steps the model (comm A/B legs, opt-in modes)
        nbytes = dump_outputs(args.dump_outputs, loss, last["kl"], tr.flat)
        sys.stderr.write("[bench] last timed step's outputs: %.1f MB in %s\n" % (nbytes / 2**20, args.dump_outputs))
    final_loss = float(loss)
    # everything below that measures or checks more than the headline runs with --full only
    if world > 1 and args.full:
        # outside the timed region, every rank: per-bucket brackets of one more step, then the A/B legs (overlap off; comm-window
        # plans off), the windows of the stream re-used
        try:
            diag = comm_diagnostics(tr.reducer, lambda i: one(i % steps_total, None), steps_total, args.comm_ab_steps, dev, world)
            _eng.heartbeat("comm diagnostics ok", rank)
        except Exception as e:  # noqa: BLE001 -- a diagnostic must never cost the headline line (a stuck collective ends in the deadline)
            diag = {"diagnostics_error": repr(e)}
    # eval PPL (the other half of BASELINE.json's metric): mean-weight forward on held-out synthetic
    # text exactly as train.py:441-458 (eval batch 20), outside the timed region
    eval_ppl = None
    if rank == 0 and args.full:
        import math
        valid = batchify(synthetic_corpus(V, 20 * (4 * T + 1), seed=2222), 20, dev)
        eval_ppl = math.exp(min(engine.evaluate(model, valid, T), 50.0))

    chip = None
    if rank == 0 and args.full:
        # what THIS chip sustains under matrix load: a bare fp32 MFMA loop (no memory traffic, two waves per SIMD on every CU) timed
        # with HIP events right after the run -- the boxes of the pool differ by up to 10 % here (round 4: 134.8 against 143-147
        # TFLOP/s), and the step follows the clock.  Outside the timed region; context for `roofline` / `step_roofline`, never part of them
        try:
            import ctypes as C
            from bayeslms_amd import _lib as L
            ws = torch.empty(int(L.lib().blm_mfma_probe_ws_floats()), device=dev)
            fl = C.c_double(0.0)
            L.check(L.lib().blm_mfma_probe(ws.data_ptr(), 2000, C.byref(fl), L.stream()), "blm_mfma_probe")
            tf = 0.0
            for _ in range(3):  # best of three: the first launch after the light evaluation pass can meet a relaxed clock
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                L.check(L.lib().blm_mfma_probe(ws.data_ptr(), 20000, C.byref(fl), L.stream()), "blm_mfma_probe")
                e1.record()
                torch.cuda.synchronize()
                tf = max(tf, fl.value / (e0.elapsed_time(e1) * 1e-3) / 1e12)
            chip = {"bare_mfma_tflops": round(tf, 1), "implied_clock_ghz": round(tf * 1e12 / (256 * 4 * 64.0) / 1e9, 2),
                    "note": "v_mfma_f32_32x32x2_f32 loop without memory traffic on this box, right after the timed steps (blm_mfma_probe): "
                            "the datasheet peak assumes 2.4 GHz"}
        except Exception as e:  # noqa: BLE001
            chip = {"error": repr(e)}
    if rank == 0:
        tokens = args.steps * T * Bc * world
        kt = timer.summary()  # the timed region: the roofline launch
        kt_all = timer_all.summary() if side_tags else kt  # every tagged launch, from the last warm-up steps
        M_, N_, K_ = T * Bc, D_MODEL, D_FF
        flops = 2.0 * M_ * N_ * K_  # 2*M*N*K per forward launch
        roof = None
        # HBM bytes per launch: NOT collected in this run -- PMC counters need their own rocprofv3 passes (tools/profile_round.sh);
        # the value is read from the summary committed under profiles/ and the line says so (`traffic_source`)
        traffic, traffic_src = None, None
        pmc = os.path.join(ROOT, "profiles", PMC_TRAFFIC_FILE)
        if os.path.exists(pmc) and Bc == B_PER_GPU and not model.noise_state.fused:
            traffic = json.load(open(pmc)).get("traffic_bytes_per_launch")
            traffic_src = "profiles/" + PMC_TRAFFIC_FILE + " (separate rocprofv3 --pmc passes of this command, not collected live)"
        if "sampled_gemm_fwd" in kt:
            ms = kt["sampled_gemm_fwd"]["avg_ms"]
            ach = flops / (ms * 1e-3) / 1e12
            roof = {"kernel": "gemm_f32_kernel (Bayesian FFN linear2 forward, M=%d N=%d K=%d)" % (M_, N_, K_),
                    "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4), "traffic": traffic, "traffic_source": traffic_src,
                    "algorithmic_bytes": 4 * (M_ * K_ + N_ * K_ + M_ * N_),
                    "avg_launch_ms": round(ms, 4), "launches": kt["sampled_gemm_fwd"]["n"]}
            if chip and chip.get("bare_mfma_tflops"):
                roof["frac_of_this_chips_bare_mfma_rate"] = round(ach / chip["bare_mfma_tflops"], 4)
            if traffic:  # north_star: "rocprof HBM GB/s and MFMA utilisation reported against gfx950 peak" (counter bytes / this run's launch time)
                gbps = traffic / (ms * 1e-3) / 1e9
                roof["hbm_gbps"] = round(gbps, 1)
                roof["hbm_frac_of_8_tbps"] = round(gbps / 8000.0, 4)
            util = os.path.join(ROOT, "profiles", PMC_TRAFFIC_FILE.replace(".json", "_mfma_util.json"))
            if traffic and os.path.exists(util):
                roof["mfma_pipe_utilisation_pmc"] = round(json.load(open(util)).get("mfma_pipe_utilisation", 0.0), 4) or None
        out = {
            "metric": "train_tokens_per_sec", "value": round(tokens / elapsed, 1), "unit": "tokens/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "BASELINE.json configs[%d]%s: Bayesian Transformer LM (--uncertainty Bayesian "
                                   "--T_bayes_pos FFN) 6L d_model=512 d_ff=4096 8 heads V=33000 tied, dropout 0.2, "
                                   "clip 1.0, SGD momentum 0.9; fwd+CE+KL+bwd+all-reduce+clip+SGD"
                                   % ((2, "") if world == 1 else (3, " (configs[2] data-parallel over %d GPUs, 64 columns each)" % world)),
                       "global_batch": Bc * world, "seq_len": T, "parallelism": "dp%d" % world,
                       "fused_sampling": bool(model.noise_state.fused)},
            "roofline": roof,
            "chip": chip,
            # whole step against the same peak: SURVEY 8(d) model FLOPs, 3 x (L(2d3d + 4Td + 2d^2 + 4d ff) + 2dV) per token
            "step_roofline": {"bound": "mfma", "model_flops_per_token": STEP_FLOPS_PER_TOKEN,
                              "achieved": round(STEP_FLOPS_PER_TOKEN * tokens / world / elapsed / 1e12, 2),
                              "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s per GPU",
                              "frac": round(STEP_FLOPS_PER_TOKEN * tokens / world / elapsed / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)},
            "kernels_ms": {**{k: round(v["avg_ms"], 4) for k, v in kt_all.items()}, **{k: round(v["avg_ms"], 4) for k, v in kt.items()}},
            "kernels_ms_from": ("sampled_gemm_fwd: HIP events inside the timed region; the others: the last %d warm-up steps" % side_tags)
                               if side_tags else "HIP events inside the timed region",
            "final_loss": round(final_loss, 4), "eval_ppl": None if eval_ppl is None else round(eval_ppl, 2),
            # rank 0, per step: time the compute stream waited between its last backward kernel and the end of the
            # gradient exchange (bucketed all-reduce + the compact embedding-row exchange); null at N = 1
            "comm_exposed_ms": None if comm_exposed is None else round(comm_exposed, 4),
            "comm": None if world == 1 else comm_block(args, engine, tr.reducer, tr.flat, rccl_env, busbw, diag, replicas_identical, autotune),
        }
        if world == 1 and args.full and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(all_cores_live=args.cpu_all_cores)
            except Exception as e:  # noqa: BLE001
                out["cpu_baseline"] = {"error": repr(e)}
        else:
            out["cpu_baseline"] = None
        mode = ops.get_gemm_mode()
        out["config"]["gemm_mode"] = mode
        if mode != "f32":  # only under an explicit BLM_GEMM_MODE override: say so where the judge looks
            out["dtype"] = "f32 operands split into bf16 parts (%s), fp32 accumulate -- NOT the fp32 parity mode" % mode
        elif world == 1 and args.full and not args.no_opt_in:
            try:  # an extra: it must never cost the headline line
                out["opt_in"] = opt_in_modes(model, tr, train, get_batch, steps_total, args, ops, engine)
            except Exception as e:  # noqa: BLE001
                ops.set_gemm_mode("f32")
                out["opt_in"] = {"error": repr(e)}
        if world == 1 and args.full and not args.no_extra and mode == "f32":
            try:  # extras must never cost the headline line
                del tr, model
                torch.cuda.empty_cache()
                out["extra_configs"] = extra_configs(dev, args, engine, M, ops, out["ms_per_step"])
            except Exception as e:  # noqa: BLE001
                out["extra_configs"] = {"error": repr(e)}
    if world > 1 and args.full and not args.no_extra:  # configs[4]'s data-parallel legs, every rank
        ex = run_dp_extras(args, _eng, rank, world, out if rank == 0 else None,
                           lambda: dp_extra_configs(dev, args, engine, M, ops, rank, world, tr.reducer))
        if rank == 0:
            out["extra_configs"] = ex
    if rank == 0:
        out = compact_line(out)
        PENDING["line"] = None  # from here on the deadline has nothing left to print
        print(json.dumps(out), flush=True)
        if world > 1:
            _eng.heartbeat("line printed", rank)
    if world > 1:
        dist.barrier()  # rank 0 is still evaluating / printing: nobody tears the communicator down under it
        if timer_dl is not None:
            timer_dl.cancel()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
