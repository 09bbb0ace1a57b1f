"""Data-parallel correctness on the GPU box: two ranks (sharing the one GPU, gloo transport) that
each own half of the global batch columns must reproduce the single-process run of the whole global
batch: same eps (no rank in the Philox key), dropout masks keyed by global column, gradients
averaged by the bucketed all-reduce, identical clip+SGD."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


FAMILIES = ["tlm_ffn", "rnn_none", "rnn_bayes3", "rnn_gauss33", "rnn_var11", "tlm_gauss3"]


def _build(dev, family="tlm_ffn"):
    """-> (model, kl_fn or None, is_rnn).  The LSTM families get their weight gradients from autograd's
    AccumulateGrad (ops._LSTMLayer / _LSTMRecurrentGP return them) -- the ADVICE r1 case: readiness of those
    must come from the post-accumulate hooks, never from a missing notification."""
    from bayeslms_amd import model as M
    torch.manual_seed(5)
    V = 150
    if family == "tlm_ffn":
        return M.BayesTransformerModel(V, 32, 4, 64, 2, 0.2, True, "FFN").to(dev), _kl, False
    if family == "tlm_gauss3":
        m = M.GaussTransformerModel(V, 32, 4, 64, 2, 0.2, True, 3).to(dev)
        return m, (lambda mm: mm.transformerlayers[0].gpnn.kl_divergence()), False
    if family == "rnn_none":
        return M.RNNModel("LSTM", V, 32, 32, 2, 0.2, True).to(dev), None, True
    if family == "rnn_bayes3":
        return M.BayesRNNModel("LSTM", V, 32, 32, 2, 0.2, True, 3).to(dev), (lambda mm: mm.rnn.kl_divergence()), True
    if family == "rnn_gauss33":
        m = M.GaussRNNModel("LSTM", V, 32, 32, 2, 0.2, True, "33").to(dev)
        return m, (lambda mm: mm.rnn.rnn[0].gpnn.kl_divergence()), True
    if family == "rnn_var11":
        m = M.VariationalRNNModel("LSTM", V, 32, 32, 2, 0.2, True, "11").to(dev)
        return m, (lambda mm: sum(mm.rnn.rnn[c].vnn.kl_divergence() for c in (0, 1))), True
    raise ValueError(family)


def _kl(model):
    return model.transformerlayers[0].linear2.kl_divergence()


_kl.fusable = True


def _run(rank, world, port, ret, family="tlm_ffn", T=12):
    import torch.distributed as dist
    from bayeslms_amd import data as D, engine, ops
    from bayeslms_amd.model import repackage_hidden
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    stream = torch.randint(0, 150, (8 * (4 * T + 13),), generator=torch.Generator().manual_seed(1))
    train = D.batchify(stream, 8, dev, rank, world)
    m, kl_fn, is_rnn = _build(dev, family)
    if is_rnn and T >= 32:
        ops.set_lstm_wavefront(True)  # these models are 32 units wide: the measured rule (H >= 640) would keep their layers on one stream
    stack2 = []
    real_stack2 = ops.lstm_stack2
    ops.lstm_stack2 = lambda *a, **k: (stack2.append(1), real_stack2(*a, **k))[1]
    tr = engine.Trainer(m, lr=0.2, clip=0.5, kl_scale=0.01, seed=1111, rank=rank, world=world, bucket_bytes=8192)
    if world > 1:
        assert tr.reducer.late is not None and len(tr.reducer.buckets) > 2
    losses = []
    hidden = m.init_hidden(train.shape[1]) if is_rnn else None
    for i in range(4):
        data, tgt = D.get_batch(train, i * T, T)
        loss, kl, hidden = tr.step(data, tgt, hidden=hidden, kl_fn=kl_fn)
        if hidden is not None:
            hidden = repackage_hidden(hidden)
        losses.append(float(loss))
    if world > 1:
        # after calibration every parameter that receives a gradient is counted, whichever way it arrives
        silent = [tuple(p.shape) for p in tr.flat.params if tr.reducer.expected[id(p)] == 0 and p.grad.abs().sum() > 0]
        assert not silent, silent
        assert tr.reducer.late.U > 0
    ret[(world, rank)] = (losses, tr.flat.flat_param.detach().cpu().clone())
    ret[("stack2", world, rank)] = len(stack2)
    if world > 1:
        dist.destroy_process_group()


@pytest.mark.parametrize("family", FAMILIES)
def test_two_ranks_equal_one_rank_on_the_global_batch(family):
    with mp.Manager() as mgr:
        ret = mgr.dict()
        _spawn(1, ret, family)
        _spawn(2, ret, family)
        l1, p1 = ret[(1, 0)]
        l2a, p2a = ret[(2, 0)]
        l2b, p2b = ret[(2, 1)]
    assert torch.equal(p2a, p2b)  # ranks stay in lock step
    # mean loss over the global batch = mean of the two half-batch means
    for a, b, c in zip(l1, l2a, l2b):
        assert abs(a - 0.5 * (b + c)) < 2e-4 * abs(a)
    err = float((p1 - p2a).abs().max() / p1.abs().max())
    assert err < 1e-4, err


@pytest.mark.parametrize("family", ["tlm_ffn", "rnn_bayes3"])
def test_four_ranks_equal_one_rank_on_the_global_batch(family):
    """Two columns per rank: four ranks (sharing this box's GPU) reproduce the single-process run of the same global batch and
    stay bit-identical among themselves (tools/dp4_probe.py walks all six families this way)."""
    with mp.Manager() as mgr:
        ret = mgr.dict()
        _spawn(1, ret, family)
        _spawn(4, ret, family)
        l1, p1 = ret[(1, 0)]
        ps = [ret[(4, r)][1] for r in range(4)]
        ls = [ret[(4, r)][0] for r in range(4)]
    assert all(torch.equal(ps[0], p) for p in ps[1:])
    for i, a in enumerate(l1):
        assert abs(a - sum(l[i] for l in ls) / 4.0) < 2e-4 * abs(a)
    assert float((p1 - ps[0]).abs().max() / p1.abs().max()) < 1e-4


def _spawn(world, ret, family="tlm_ffn", T=12):
    port = _free_port()
    mp.spawn(_run, args=(world, port, ret, family, T), nprocs=world, join=True)


@pytest.mark.parametrize("family,T", [("rnn_none", 36), ("rnn_bayes3", 36), ("rnn_none", 72)])
def test_two_ranks_equal_one_rank_with_the_layer_wavefront(family, T):
    """What a data-parallel LSTM run at the recipes' shape executes: <= 32 columns per rank and T >= 32 put
    the two layers on the two-stream wavefront (ops.lstm_stack2) while the reducer's hooks, its communication stream and
    the bucket overlap (8 KB buckets) are active -- two ranks == one rank on the global batch, replicas bit-identical.
    T 72: nine chunks, i.e. the per-chunk GEMMs on their third stream (the recipes' T 100 takes that form)."""
    with mp.Manager() as mgr:
        ret = mgr.dict()
        _spawn(1, ret, family, T)
        _spawn(2, ret, family, T)
        l1, p1 = ret[(1, 0)]
        l2a, p2a = ret[(2, 0)]
        l2b, p2b = ret[(2, 1)]
        assert ret[("stack2", 1, 0)] == 4 and ret[("stack2", 2, 0)] == 4 and ret[("stack2", 2, 1)] == 4  # every step took it
    assert torch.equal(p2a, p2b)
    for a, b, c in zip(l1, l2a, l2b):
        assert abs(a - 0.5 * (b + c)) < 2e-4 * abs(a)
    err = float((p1 - p2a).abs().max() / p1.abs().max())
    assert err < 1e-4, err


def _run_eval(rank, world, port, ret, family):
    import torch.distributed as dist
    from bayeslms_amd import data as D, engine
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    m, _, _ = _build(dev, family)
    stream = torch.randint(0, 150, (4 * 83 + 3,), generator=torch.Generator().manual_seed(9))
    valid = D.batchify(stream, 4, dev)  # 4 columns: an uneven split over 3 ranks, and more ranks than columns at 5
    ret[(world, rank)] = engine.evaluate(m, valid, 12, rank=rank, world=world)
    if world > 1:
        dist.destroy_process_group()


@pytest.mark.parametrize("family", ["tlm_ffn", "rnn_bayes3"])
def test_sharded_evaluation_equals_the_single_process_pass(family):
    """engine.evaluate(rank, world): rank r evaluates its share of the evaluation batch's columns (independent streams; the
    LSTM's carried state is per column) and one 8-byte all-reduce joins the token-weighted sums -- the loss train.py:441-458
    computes, on every rank, for 2, 3 and (more ranks than columns) 5 ranks.  (The GPU box allows 6 processes on the card at
    once and the test runner itself is one of them: 5 ranks at most.)"""
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_run_eval, args=(1, _free_port(), ret, family), nprocs=1, join=True)
        one = ret[(1, 0)]
        for world in (2, 3, 5):
            mp.spawn(_run_eval, args=(world, _free_port(), ret, family), nprocs=world, join=True)
            vals = [ret[(world, r)] for r in range(world)]
            assert all(v == vals[0] for v in vals), vals
            assert abs(vals[0] - one) <= 2e-6 * abs(one), (world, vals[0], one)


def _rccl_one_rank(port, ret):
    """RCCL itself (backend "nccl"), one rank: process-group init with device_id as bench.py does it,
    the reducer's side-stream async all-reduce pattern, barrier, and a Trainer step in 'world 2'
    arithmetic (the collective over a 1-rank group is the identity, so the result must equal the
    plain run with gradients halved by grad_scale)."""
    import torch.distributed as dist
    from bayeslms_amd import _lib, data as D, engine
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    for k in ("NCCL_MIN_NCHANNELS", "NCCL_MAX_NCHANNELS"):
        os.environ.pop(k, None)
    # as bench.py / train.py do it: channels pinned before RCCL reads its environment, bounded timeout, checked first all-reduce
    pinned = engine.init_distributed("nccl", dev, 120, init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        bw = engine.allreduce_busbw(8 << 20, 3, dev)  # the stand-alone all-reduce of bench.py's comm block, on RCCL
        assert bw["mb"] == 8.39 and bw["ms"] > 0 and bw["busbw_gbps"] == 0.0 and engine.rccl_version()  # (N-1)/N = 0 at one rank
        x = torch.arange(1024, device=dev, dtype=torch.float32)
        side = torch.cuda.Stream()
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        side.wait_event(ev)
        with torch.cuda.stream(side):
            h = dist.all_reduce(x[128:512], op=dist.ReduceOp.SUM, async_op=True)
        h.wait()
        torch.cuda.current_stream().wait_stream(side)
        dist.barrier()
        ok_identity = bool(torch.equal(x.cpu(), torch.arange(1024, dtype=torch.float32)))
        stream = torch.randint(0, 150, (8 * 61,), generator=torch.Generator().manual_seed(1))
        train = D.batchify(stream, 8, dev)
        m, _, _ = _build(dev)
        tr = engine.Trainer(m, lr=0.2, clip=0.5, kl_scale=0.01, seed=1111, rank=0, world=2, bucket_bytes=8192)
        tr.reducer.world = 2  # grad-ready hooks on, bucketed collectives issued over RCCL (1-rank group: identity)
        # the pinned channel count reaches the reducer: the GEMM planner's comm window opens with the buckets and is closed
        # again when the step is over
        comm_ok = (pinned["NCCL_MAX_NCHANNELS"] == str(engine.RCCL_CHANNELS_DEFAULT) and tr.reducer.comm_cus == engine.RCCL_CHANNELS_DEFAULT
                   and tr.reducer.comm_plan == "window")
        losses = []
        for i in range(3):
            data, tgt = D.get_batch(train, i * 12, 12)
            loss, _, _ = tr.step(data, tgt, kl_fn=_kl)
            losses.append(float(loss))
            comm_ok = comm_ok and float(_lib.lib().blm_gemm_plan_comm_window_left()) == 0.0
        # per-bucket brackets on the communication stream around RCCL's own asynchronous work objects (bench.py's comm block)
        tr.reducer.measure_buckets = True
        data, tgt = D.get_batch(train, 36, 12)
        loss, _, _ = tr.step(data, tgt, kl_fn=_kl)
        rep = tr.reducer.bucket_report()
        tr.reducer.measure_buckets = False
        comm_ok = comm_ok and len(rep) >= len(tr.reducer.buckets) and all(r["ms"] > 0 and "done_after_bwd_end_ms" in r for r in rep)
        losses.append(float(loss))
        ret["rccl"] = (ok_identity and comm_ok, losses, bool(torch.isfinite(tr.flat.flat_param).all()))
    finally:
        dist.destroy_process_group()


def test_rccl_backend_single_rank_smoke():
    import torch.distributed as dist
    if not dist.is_nccl_available():
        pytest.skip("no RCCL in this torch build")
    with mp.Manager() as mgr:
        ret = mgr.dict()
        p = mp.get_context("spawn").Process(target=_rccl_one_rank, args=(_free_port(), ret))
        p.start()
        p.join(300)
        assert p.exitcode == 0
        ok, losses, finite = ret["rccl"]
        assert ok and finite and all(v == v for v in losses) and losses[-1] < losses[0] + 1.0


def test_bench_gpus2_self_launch_rehearsal_on_one_device():
    """`python bench.py --gpus 2` from one process: two ranks share this box's single GPU (gloo transport; RCCL
    refuses two ranks on one device), the real trainer step incl. the bucketed exchange and the compact
    embedding-row exchange, one JSON line with n_gpus 2 and comm_exposed_ms."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "2",
                        "--warmup", "2", "--batch", "8", "--no-cpu-baseline", "--no-opt-in", "--full"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 16 and out["value"] > 0
    assert out["comm_exposed_ms"] is not None and out["comm"]["late_rows"] and out["comm"]["late_rows_last_step"] > 0
    assert out["comm"]["replicas_identical"] is True  # parameter checksums of both ranks, gathered after the last step
    c = out["comm"]  # the line explains its own scaling
    assert c["world_seen"] == 2 and c["allreduce_busbw_gbps"] > 0 and c["dist_timeout_s"] == 180.0
    assert len(c["buckets_last_step"]) >= c["buckets"] and all(b["ms"] > 0 for b in c["buckets_last_step"])
    assert c["ab_steps"] == 5 and c["step_ms_as_configured"] > 0 and "step_ms_no_overlap" in c and "step_ms_no_comm_window" in c
    assert c["autotune"]["picked"] in c["autotune"]["ms"] and c["overlap_in_timed_region"] == (c["autotune"]["picked"] != "overlap_off")
    for stage in ("rendezvous ok", "first all-reduce ok", "model built", "stand-alone all-reduce ok", "warm-up ok", "timed region ok",
                  "comm diagnostics ok", "headline ok; extra legs", "configs[4] training leg ok", "configs[4] rescoring leg ok", "line printed"):
        assert stage in r.stderr, stage
    # BASELINE.json configs[4] on N GPUs (after the headline, every rank): the GP Transformer's training step data-parallel and
    # every rank rescoring its own archive with 8 Monte-Carlo weight samples
    ex = {e["id"]: e for e in out["extra_configs"]}
    tr, sc = ex["cfg4_gp_tlm_train_dp"], ex["cfg4_gp_tlm_rescore_mc8_dp"]
    assert "error" not in tr and tr["n_gpus"] == 2 and tr["value"] > 0 and tr["replicas_identical"] is True and tr["final_loss"] == tr["final_loss"]
    assert abs(tr["value"] - 128 * 8 * 2 / (tr["ms_per_step"] * 1e-3)) < 1.0  # all ranks' tokens / the slowest rank's time
    assert "error" not in sc and sc["unit"] == "hypotheses/s" and abs(sc["value"] - 2 * 1000 * 20 / sc["slowest_rank_s"]) < 0.05 * sc["value"]
    assert list(out)[-1] == "baseline_configs"
    b4 = out["baseline_configs"]["configs[4]"]
    assert b4["train_dp"]["value"] == tr["value"] and b4["rescore_8_mc_samples_dp"]["value"] == sc["value"]
    assert out["baseline_configs"]["configs[3]"]["value"] == out["value"] and out["baseline_configs"]["configs[2]"] is None


def test_bench_four_ranks_on_one_device_agree_on_the_compact_rows():
    """Round 5: `bench.py --gpus 4 --backend gloo` (4 ranks + launcher + torchrun agent share this box's GPU) used to die in 4-8 of
    16 runs -- the ranks disagreed on U, the number of distinct token ids of the global batch, because c10d's own staging of device
    tensors for gloo let engine.LateRows read the gathered ids while the copy back was still landing.  The rehearsal transport is
    now handed host tensors (engine.LateRows.begin, engine._HostStagedReduce).  Two runs back to back: both finish, replicas
    identical, U = the count computed here on the host from the same synthetic stream."""
    import json
    import subprocess
    import sys
    from bayeslms_amd.data import batchify, get_batch, synthetic_corpus
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    steps, warm, Bc, W, T, V = 3, 2, 16, 4, 128, 33000
    full = batchify(synthetic_corpus(V, Bc * W * ((steps + warm) * T + 1) + 17, seed=1111), Bc * W)
    # the last training step of the run is the first A/B leg's last step: the windows of the stream are re-used modulo steps + warm
    want = {int(torch.unique(get_batch(full, i * T, T)[0]).numel()) for i in range(steps + warm)}
    for _ in range(2):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(W), "--backend", "gloo", "--steps", str(steps),
                            "--warmup", str(warm), "--batch", str(Bc), "--no-cpu-baseline", "--no-opt-in", "--no-extra", "--comm-ab-steps", "1",
                            "--deadline-s", "240", "--full"], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        c = out["comm"]
        assert out["n_gpus"] == 4 and c["world_seen"] == 4 and c["replicas_identical"] is True and c["late_rows_last_step"] in want, c
