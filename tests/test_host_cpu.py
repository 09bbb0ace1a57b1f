"""CPU: host-side logic -- data layout vs the reference's own outputs, state_dict contract,
data-parallel column sharding and the gradient reducer under gloo (world_size 2)."""
import os
import time
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_corpus_and_batchify_match_reference():
    from bayeslms_amd import data
    g, _, _ = load_golden("data_layout")
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "words.txt"), "w") as f:
        f.write("".join("%s %d\n" % (w, i) for i, w in enumerate(g["words"])))
    for s in ("train", "valid", "test"):
        with open(os.path.join(d, s + ".txt"), "w") as f:
            f.write(str(g[s + "_txt"]))
    c = data.Corpus(d)
    assert len(c.dictionary) == len(g["words"])
    for s in ("train", "valid", "test"):
        assert torch.equal(getattr(c, s), g[s + "_ids"])
    b = data.batchify(c.train, int(g["bsz"]))
    assert torch.equal(b, g["batchified"])
    x, y = data.get_batch(b, int(g["get_batch_i"]), int(g["seq_len"]))
    assert torch.equal(x, g["get_batch_data"]) and torch.equal(y, g["get_batch_target"])
    # ragged tail: last window is shorter, and an empty line still yields '<s>'
    x, y = data.get_batch(b, b.size(0) - 3, 5)
    assert x.size(0) == 2 and y.numel() == 2 * b.size(1)


def test_dp_column_sharding_is_a_partition_of_the_global_batch():
    from bayeslms_amd import data
    stream = torch.arange(1000)
    full = data.batchify(stream, 8)
    parts = [data.batchify(stream, 8, rank=r, world=4) for r in range(4)]
    assert torch.equal(torch.cat(parts, 1), full)
    with pytest.raises(ValueError):
        data.batchify(stream, 6, rank=0, world=4)


def test_synthetic_corpus_shape():
    from bayeslms_amd.data import synthetic_corpus
    s = synthetic_corpus(1000, 20000, seed=1111)
    assert s.dtype == torch.int64 and s.numel() == 20000 and int(s.min()) == 0 and int(s.max()) < 1000
    assert torch.equal(s, synthetic_corpus(1000, 20000, seed=1111))
    lens = np.diff(np.flatnonzero(s.numpy() == 0))
    assert 6 < lens.mean() < 11 and lens.max() <= 61


STATE_DICT_CASES = [
    ("bayes_tlm_FFN", lambda M, V, d, ff, h: M.BayesTransformerModel(V, d, h, ff, 2, 0.2, True, "FFN")),
    ("bayes_tlm_MHA", lambda M, V, d, ff, h: M.BayesTransformerModel(V, d, h, ff, 2, 0.2, True, "MHA")),
    ("bayes_tlm_EMB", lambda M, V, d, ff, h: M.BayesTransformerModel(V, d, h, ff, 2, 0.2, True, "EMB")),
    ("bayes_tlm_none", lambda M, V, d, ff, h: M.BayesTransformerModel(V, d, h, ff, 2, 0.2, True, "none")),
    ("transformer_baseline", lambda M, V, d, ff, h: M.TransformerModel(V, d, h, ff, 2, 0.2, "gelu", True)),
]


@pytest.mark.parametrize("name,build", STATE_DICT_CASES)
def test_transformer_state_dict_contract(name, build):
    """Same keys and shapes as the reference's state_dict."""
    from bayeslms_amd import model as M
    g, sd, _ = load_golden(name)
    V, d = sd["encoder.weight"].shape
    ff = [v for k, v in sd.items() if k.endswith("0.linear1.weight")][0].shape[0]
    m = build(M, V, d, ff, int(g["nhead"]))
    own = m.state_dict()
    assert set(own) == set(sd)
    for k, v in sd.items():
        if not k.endswith("pos_encoder.pe"):
            assert tuple(own[k].shape) == tuple(v.shape), k
    assert own["pos_encoder.pe"].shape == (5000, 1, d)
    assert torch.allclose(own["pos_encoder.pe"][:64], sd["pos_encoder.pe"], atol=1e-6)
    if name != "transformer_baseline":
        assert m.decoder.weight is m.encoder.weight  # tied


@pytest.mark.parametrize("pos", [0, 1, 3])
def test_lstm_state_dict_contract(pos):
    from bayeslms_amd import model as M
    _, sd, _ = load_golden("bayes_rnn_pos%d" % pos)
    V, H = sd["encoder.weight"].shape
    m = M.BayesRNNModel("LSTM", V, H, H, 2, 0.0, True, pos)
    own = m.state_dict()
    assert set(own) == set(sd)
    for k, v in sd.items():
        assert tuple(own[k].shape) == tuple(v.shape), k
    _, sd, _ = load_golden("rnn_baseline")
    own = M.RNNModel("LSTM", V, H, H, 2, 0.2, True).state_dict()
    assert set(own) == set(sd)


def test_option_semantics_and_errors():
    from bayeslms_amd import model as M, BayesLMError
    # any other bayes_pos string builds zero layers, like the reference (model.py:1193-1214)
    assert len(M.BayesTransformerModel(20, 8, 2, 16, 3, 0.1, True, "bogus").transformerlayers) == 0
    m = M.BayesTransformerModel(20, 8, 2, 16, 3, 0.5, True, "FFN")
    assert m.transformerlayers[0].p == 0.2 and m.transformerlayers[1].p == 0.5  # hard-coded 0.2 on layer 0
    assert isinstance(m.transformerlayers[0].linear2, M.BayesLinear)
    assert not isinstance(m.transformerlayers[1].linear2, M.BayesLinear)  # only layer 0 is Bayesian
    with pytest.raises(ValueError):
        M.BayesRNNModel("LSTM", 20, 8, 16, 2, 0.1, True, 1)  # tied needs nhid == emsize
    with pytest.raises(ValueError):
        M.RNNModel("GRU", 20, 8, 8, 2)
    with pytest.raises(BayesLMError):
        m(torch.zeros(3, 2, dtype=torch.long))  # CPU tensors: the product path refuses, no fallback


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _reducer_worker(rank, world, port, ret):
    import torch.distributed as dist
    from bayeslms_amd import engine
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(50, 70), torch.nn.Linear(70, 30), torch.nn.Linear(30, 9))
    flat = engine.FlatBuffers(net)
    red = engine.GradReducer(flat, bucket_bytes=4096)
    assert len(red.buckets) > 1
    params = flat.params
    results = []
    for step in range(3):
        flat.zero_grad()
        # "backward": gradients appear in reverse parameter order; param 0 gets two contributions
        for i in range(len(params) - 1, -1, -1):
            params[i].grad.add_(float(rank + 1) * (i + 1 + step))
            red.mark_ready(params[i])
            if i == 0:
                params[i].grad.add_(0.5)
                red.mark_ready(params[i])
        red.finish()
        results.append(flat.flat_grad.clone())
    for step, r in enumerate(results):
        for i, p in enumerate(params):
            want = sum(float(k + 1) * (i + 1 + step) for k in range(world)) + (0.5 * world if i == 0 else 0.0)
            o = flat.offsets[i]
            assert torch.allclose(r[o:o + p.numel()], torch.full((p.numel(),), want)), (rank, step, i)
    # after calibration the reducer knows param 0 needs two notifications
    assert red.expected[id(params[0])] == 2 and red.expected[id(params[1])] == 1
    ret[rank] = True
    dist.destroy_process_group()


def _dp_check_worker(rank, world, port, ret):
    import torch.distributed as dist
    from bayeslms_amd import engine, BayesLMError
    os.environ["BLM_DP_CHECK"] = "1"
    os.environ["BLM_DP_TRACE"] = ret["trace"]
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    net = torch.nn.Sequential(torch.nn.Linear(8, 8))
    red = engine.GradReducer(engine.FlatBuffers(net), bucket_bytes=1 << 20)
    assert red.check
    buf = torch.zeros(64)
    red._all_reduce(buf[:16], "agreeing")          # same size everywhere: goes through
    for h in red.handles:
        h.wait()
    red.handles = []
    try:
        red._all_reduce(buf[: 16 + 8 * rank], "compact embedding rows (U = %d)" % (2 + rank))   # what a disagreement on U looks like
        ret[rank] = "no error"
    except BayesLMError as e:
        ret[rank] = str(e)
    dist.destroy_process_group()


def test_dp_check_names_the_collective_the_ranks_disagree_on():
    """BLM_DP_CHECK=1: a collective whose element count differs between the ranks raises on EVERY rank with each rank's
    (sequence number, elements) pair, before anything is handed to the transport."""
    port = _free_port()
    with mp.Manager() as mgr, tempfile.TemporaryDirectory() as d:
        ret = mgr.dict()
        ret["trace"] = os.path.join(d, "dp")
        mp.spawn(_dp_check_worker, args=(2, port, ret), nprocs=2, join=True)
        for r in (0, 1):
            assert "disagree" in ret[r] and "[(2, 16), (2, 24)]" in ret[r] and "compact embedding rows" in ret[r], ret[r]
            lines = open("%s.rank%d" % (ret["trace"], r)).read().splitlines()  # BLM_DP_TRACE: this rank's sequence of collectives
            assert len(lines) == 2 and lines[0].startswith("1 agreeing 16 ") and lines[1].startswith("2 compact embedding rows (U = %d) %d " % (2 + r, 16 + 8 * r))


@pytest.mark.parametrize("world", [2, 3, 8])  # 8: the world size of BASELINE configs[3], never run on hardware here
def test_grad_reducer_gloo_world2(world):
    port = _free_port()
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_reducer_worker, args=(world, port, ret), nprocs=world, join=True)
        assert all(ret.get(r) for r in range(world))


def _late_rows_worker(rank, world, port, ret):
    """Tied encoder gradient in two parts (engine.LateRows) over gloo with CPU tensors: the decoder contribution
    goes through the bucketed all-reduce, the embedding rows through the compact exchange; the sum must equal the
    dense all-reduce of both."""
    import torch.distributed as dist
    from bayeslms_amd import engine
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    V, D, T, B = 40, 6, 5, 3
    torch.manual_seed(0)
    net = torch.nn.ModuleDict({"encoder": torch.nn.Embedding(V, D), "other": torch.nn.Linear(D, 7)})
    flat = engine.FlatBuffers(net)
    red = engine.GradReducer(flat, bucket_bytes=256)
    enc = net["encoder"].weight
    red.late = engine.LateRows(red, enc)
    for step in range(3):
        g = torch.Generator().manual_seed(100 * step + rank)
        ids = torch.randint(0, V, (T, B), generator=g)
        dy = torch.randn(T, B, D, generator=g)
        dec = torch.randn(V, D, generator=g)
        flat.zero_grad()
        red.late.begin(ids)
        # backward order: other (last layer), decoder contribution into the tied weight, ..., embedding rows last
        for p in net["other"].parameters():
            p.grad.add_(1.0 + rank)
            red.mark_ready(p)
        enc.grad.add_(dec)
        red.mark_ready(enc)
        sink = red.late.sink(enc, ids)
        assert sink is not None
        buf, slots, U, done = sink
        assert slots.shape == ids.shape and int(slots.min()) >= 0 and int(slots.max()) < U <= min(V, world * T * B)
        buf.view(U, D).index_add_(0, slots.reshape(-1), dy.reshape(-1, D))
        done()
        assert red.late.sink(enc, ids) is None  # a second embedding lookup of the same step takes the dense path
        red.finish()
        # dense reference: every rank's (decoder + scattered rows), summed over ranks
        want = torch.zeros(V, D)
        for r in range(world):
            g = torch.Generator().manual_seed(100 * step + r)
            ids_r = torch.randint(0, V, (T, B), generator=g)
            dy_r = torch.randn(T, B, D, generator=g)
            dec_r = torch.randn(V, D, generator=g)
            want += dec_r
            want.index_add_(0, ids_r.reshape(-1), dy_r.reshape(-1, D))
        assert torch.allclose(enc.grad, want, atol=1e-5), (rank, step, float((enc.grad - want).abs().max()))
        for p in net["other"].parameters():
            assert torch.allclose(p.grad, torch.full_like(p.grad, sum(1.0 + r for r in range(world))))
    assert red.expected[id(enc)] == 1  # the embedding half no longer counts as a writer of the flat slot
    ret[rank] = True
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4, 8])
def test_late_rows_gloo_world2(world):
    port = _free_port()
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_late_rows_worker, args=(world, port, ret), nprocs=world, join=True)
        assert all(ret.get(r) for r in range(world))


def test_grad_reducer_never_infers_readiness():
    """a parameter nobody marked in the calibration step holds its bucket until finish(); a write that
    arrives after its bucket went out raises instead of racing the all-reduce."""
    from bayeslms_amd import engine, BayesLMError
    net = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 8))
    flat = engine.FlatBuffers(net)
    red = engine.GradReducer(flat, bucket_bytes=1 << 20)  # one bucket
    p = flat.params
    for q in p[1:]:  # calibration: p[0] is never written
        red.mark_ready(q)
    red.finish()
    assert red.expected[id(p[0])] == 0
    for q in p[1:]:
        red.mark_ready(q)
    assert not any(red.launched)  # the silent parameter keeps the bucket back
    red.mark_ready(p[0])          # ... and if it does get a gradient later, the bucket still waits for finish()
    assert not any(red.launched)
    red.finish()
    # two buckets: a late second write into an already reduced bucket is an error, not a race
    red = engine.GradReducer(flat, bucket_bytes=64)
    assert len(red.buckets) > 1
    for q in reversed(p):
        red.mark_ready(q)
    red.finish()
    for i in red.buckets[0][2]:   # first bucket in backward order = the tail of the buffer
        red.mark_ready(p[i])
    assert red.launched[0] and red.bucket_of[id(p[-1])] == 0
    with pytest.raises(BayesLMError):
        red.mark_ready(p[-1])
    red.reset()
    # hook_autograd: AccumulateGrad reports through the post-accumulate hook
    red.hook_autograd()
    x = torch.randn(4, 8)
    net(x).sum().backward()
    assert all(red.seen[id(q)] == 1 for q in p)
    red.unhook()


def _bench(argv, env_extra=None, timeout=300):
    import subprocess
    import sys
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=timeout,
                       env=env, cwd="/tmp")
    return r, time.time() - t0


def test_bench_under_the_drivers_own_launch_command_with_eight_ranks():
    """The driver does not use `bench.py`'s own launcher: it runs `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1 --master-port P bench.py --gpus N --steps K --warmup W`.  That command, verbatim, with N = 8 -- the
    world size of BASELINE configs[3], which has never met hardware here -- as a rehearsal on the host (gloo, --rehearse-launch: every
    stage of the multi-rank run, no GPU work): ONE JSON line from rank 0, all eight ranks through every heartbeat, replicas equal.
    Both as the plain run (the headline alone) and with --full (+ the stand-alone all-reduce, comm diagnostics, extra legs)."""
    import json
    import subprocess
    import sys
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    for full in (False, True):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1",
               "--backend", "gloo", "--rehearse-launch"] + (["--full"] if full else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd="/tmp")
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-3000:]
        out = json.loads(lines[0])
        assert out["n_gpus"] == 8 and out["steps"] == 2 and out["warmup"] == 1 and out["value"] is None and "NOT a measurement" in out["rehearsal"]
        c = out["comm"]
        assert c["world_seen"] == 8 and c["replicas_identical"] is True and c["autotune"]["picked"] in c["autotune"]["ms"]
        assert list(out)[-1] == "baseline_configs"
        if full:
            assert out["extra_configs"][0]["id"] == "rehearsal_extra_leg"  # the post-headline legs ran too
            assert len(c["allreduce_standalone"]) == 2 and c["ab_steps"] == 5
        else:
            assert "extra_configs" not in out and c["allreduce_standalone"] is None and "buckets_last_step" not in c
        err = r.stderr.splitlines()
        for rank in range(8):
            for stage in ("rendezvous ok (world 8, backend gloo, timeout 180 s)", "first all-reduce ok", "timed region ok (2 steps)"):
                assert any(ln.startswith("[blm rank %d +" % rank) and ln.endswith("] " + stage) for ln in err), (rank, stage, full)
            for stage in ("stand-alone all-reduce ok", "comm diagnostics ok", "headline ok; extra legs"):
                assert any(ln.startswith("[blm rank %d +" % rank) and ln.endswith("] " + stage) for ln in err) == full, (rank, stage, full)


def test_bench_self_launches_its_ranks_from_one_process():
    """VERDICT r1 / ADVICE: `python bench.py --gpus N` must start its own ranks (a torch.distributed.run child, before
    any GPU call) instead of exiting.  CPU side: the launch plumbing only (--rehearse-launch: no GPU work).
    VERDICT r4 #1: the rehearsal walks every stage of the real multi-rank run (bounded rendezvous, heartbeats, stand-alone
    all-reduce, timed region, replica check, per-bucket brackets, A/B legs) and fills every field of the `comm` block."""
    import json
    r, _ = _bench(["--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--rehearse-launch", "--dp-autotune", "0", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["value"] is None
    c = out["comm"]
    assert c["world_seen"] == 2 and c["backend"] == "gloo" and c["dist_timeout_s"] == 180.0 and c["replicas_identical"] is True
    assert "rccl_version" in c and c["allreduce_busbw_gbps"] > 0 and len(c["allreduce_standalone"]) == 2
    assert c["allreduce_standalone"][0]["mb"] == round(c["grad_bytes"] / 1e6, 2)
    b = c["buckets_last_step"]  # one entry per collective of one step, launch order = backward order
    assert len(b) == c["buckets"] >= 3 and all(x["ms"] > 0 and "ready_before_bwd_end_ms" in x and "done_after_bwd_end_ms" in x for x in b)
    assert abs(sum(x["mb"] for x in b) - c["grad_bytes"] / 1e6) < 1e-3
    assert c["ab_steps"] == 5 and c["step_ms_as_configured"] > 0 and c["step_ms_no_overlap"] > 0
    assert "step_ms_no_comm_window" in c  # null here: host tensors have no CUs to plan around (comm_plan "off")
    for stage in ("rendezvous ok (world 2, backend gloo, timeout 180 s)", "first all-reduce ok", "stand-alone all-reduce ok",
                  "warm-up ok (1 steps)", "timed region ok (2 steps)", "comm diagnostics ok"):
        for rank in (0, 1):
            assert any(ln.startswith("[blm rank %d +" % rank) and ln.endswith("] " + stage) for ln in r.stderr.splitlines()), (rank, stage)
    assert "[blm rank 0 +" in r.stderr and "line printed" in r.stderr
    # --dp-overlap 0: the A/B leg is reported as null, not re-measured under another name
    r, _ = _bench(["--gpus", "2", "--backend", "gloo", "--steps", "1", "--warmup", "1", "--rehearse-launch", "--dp-overlap", "0",
                   "--comm-ab-steps", "2", "--dist-timeout-s", "60", "--full"])
    c = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])["comm"]
    assert c["step_ms_no_overlap"] is None and c["ab_steps"] == 2 and c["dist_timeout_s"] == 60.0 and c["overlap"] is False
    # the calibration in front of the timed region (default on): the configured setting and its alternatives timed on every rank with
    # the same max-over-ranks numbers; what was picked is what the timed region ran with
    a = c["autotune"]
    assert a["steps_each"] == 3 and set(a["ms"]) == {"as_configured"} and a["picked"] == "as_configured"  # overlap already off, no comm window on the host
    assert c["overlap_in_timed_region"] is False
    r, _ = _bench(["--gpus", "2", "--backend", "gloo", "--steps", "1", "--warmup", "1", "--rehearse-launch", "--comm-ab-steps", "0", "--full"])
    c = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])["comm"]
    a = c["autotune"]
    assert set(a["ms"]) == {"as_configured", "overlap_off"} and a["picked"] in a["ms"]
    assert c["overlap_in_timed_region"] == (a["picked"] != "overlap_off")
    assert a["picked"] == "as_configured" or a["ms"][a["picked"]] < 0.98 * a["ms"]["as_configured"]
    # a WORLD_SIZE / --gpus mismatch is an error, not a silently different run
    r, _ = _bench(["--gpus", "2"], {"WORLD_SIZE": "3"})
    assert r.returncode != 0 and "WORLD_SIZE=3" in (r.stderr + r.stdout)


@pytest.mark.parametrize("hang,who_reports", [("1:warmup", "rank"), ("0:timed:gil", "launcher_rc"), ("*:rendezvous:gil", "launcher_kill")])
def test_bench_multi_rank_run_cannot_hang_silently(hang, who_reports):
    """a stuck rank ends the run INSIDE the deadline with a non-zero exit code and exactly one JSON line
    {"metric", "value": null, "error", "last_stage"}.  Three ways to be stuck:
      * a rank that stops in Python: every rank's own deadline timer fires, rank 0 prints the line, exit 124;
      * rank 0 stuck in a call that holds the interpreter lock (its timer cannot run): another rank's timer ends the job, the
        launcher parent sees a non-zero child without a line and prints it, with every rank's last heartbeat;
      * every rank stuck that way before the rendezvous: the launcher parent terminates the child's process group at
        deadline + 15 s and prints the line."""
    import json
    r, took = _bench(["--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--rehearse-launch", "--deadline-s", "4",
                      "--rehearse-hang", hang, "--full"], timeout=120)
    assert r.returncode != 0 and took < 60.0, (r.returncode, took)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["value"] is None and out["metric"] == "train_tokens_per_sec" and out["n_gpus"] == 2 and out["error"]
    if who_reports == "rank":
        # rank 0's own line (the other ranks leave two seconds after their timers fire); should the agent still be quicker, the
        # launcher's line with every rank's last heartbeat says the same
        assert out["last_stage"] in ("stand-alone all-reduce ok", {"rank 0": "stand-alone all-reduce ok", "rank 1": "stand-alone all-reduce ok"})
        assert "DEADLINE 4 s" in r.stderr
    elif who_reports == "launcher_rc":
        assert out["last_stage"] == {"rank 0": "warm-up ok (1 steps)", "rank 1": "warm-up ok (1 steps)"}
        assert "no result line" in out["error"]
    else:
        assert r.returncode == 124 and out["last_stage"] == "no heartbeat seen" and "terminated by the launcher" in out["error"]
        assert 15.0 <= took


@pytest.mark.parametrize("hang", ["", "1:extras", "*:extras"])
def test_bench_extra_legs_of_a_multi_rank_run_cannot_cost_the_headline(hang):
    """At N > 1 the line also carries configs[4]'s data-parallel legs, run by every rank AFTER the headline was measured and
    assembled.  Rank 0 holds the finished line while they run: legs that return are added (`extra_configs`, and
    `baseline_configs` stays the last key); a leg that does not return inside --dp-extras-budget-s ends in THAT line, marked, with
    exit code 0 on every rank -- still exactly one JSON line, with the headline's fields and its `comm` block intact."""
    import json
    argv = ["--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--rehearse-launch", "--dp-autotune", "0",
            "--comm-ab-steps", "0", "--dp-extras-budget-s", "4", "--full"]
    r, took = _bench(argv + (["--rehearse-hang", hang] if hang else []), timeout=120)
    assert r.returncode == 0 and took < 60.0, (r.returncode, took, r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ms_per_step"] > 0 and out["comm"]["replicas_identical"] is True
    assert list(out)[-1] == "baseline_configs"
    assert "headline ok; extra legs" in r.stderr
    if not hang:
        assert out["extra_configs"] == [{"id": "rehearsal_extra_leg", "ms_per_step": out["extra_configs"][0]["ms_per_step"]}]
        assert "line printed" in r.stderr and "DEADLINE" not in r.stderr
    else:
        assert "cut short by the deadline after stage 'headline ok; extra legs'" in out["extra_configs"]["error"]
        assert "DEADLINE" in r.stderr
    # --no-extra: the legs are skipped altogether
    if not hang:
        r, _ = _bench(argv + ["--no-extra"])
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert r.returncode == 0 and "extra_configs" not in out and "headline ok; extra legs" not in r.stderr



def test_bench_dump_outputs_writes_a_fixed_float32_sample(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR`: loss, kl and the same seeded sample of the parameter and gradient buffers, float32,
    under 64 MB, identical from call to call; `--steps` below 1 is refused before any work."""
    import importlib
    import types
    monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)  # bench.py sets it on import; undone after the test
    bench = importlib.import_module("bench")
    n = bench.DUMP_SAMPLE + 12345
    flat = types.SimpleNamespace(total=n, flat_param=torch.arange(n, dtype=torch.float32),
                                 flat_grad=-torch.arange(n, dtype=torch.float32))
    nbytes = bench.dump_outputs(str(tmp_path / "a"), torch.tensor(5.5), torch.tensor(0.25), flat)
    bench.dump_outputs(str(tmp_path / "b"), torch.tensor(5.5), None, flat)
    assert nbytes <= 64 << 20
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in ("loss", "kl", "params_sample", "grads_sample")}
    assert all(v.dtype == np.float32 for v in got.values()) and sum(v.nbytes for v in got.values()) == nbytes
    assert got["loss"].tolist() == [5.5] and got["kl"].tolist() == [0.25]
    p = got["params_sample"]
    assert p.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(p) > 0) and np.array_equal(got["grads_sample"], -p)
    assert np.array_equal(np.load(str(tmp_path / "b" / "params_sample.npy")), p)
    assert np.load(str(tmp_path / "b" / "kl.npy")).tolist() == [0.0]
    r, _ = _bench(["--steps", "0"], timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr


def test_init_distributed_is_bounded_and_checks_its_first_all_reduce(monkeypatch):
    """engine.init_distributed hands init_process_group a timeout (BLM_DIST_TIMEOUT_S / argument / 180 s) instead of torch's
    10-30 minutes: a rank whose peers never come raises inside it."""
    from bayeslms_amd import engine
    monkeypatch.delenv("BLM_DIST_TIMEOUT_S", raising=False)
    assert engine.dist_timeout_s() == 180.0 and engine.dist_timeout_s(25) == 25.0
    monkeypatch.setenv("BLM_DIST_TIMEOUT_S", "3")
    assert engine.dist_timeout_s(25) == 3.0
    rc, out, err = _py("import os, time\n"
                       "os.environ.update(RANK='0', WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT='%d')\n"
                       "from bayeslms_amd import engine\n"
                       "t0 = time.time()\n"
                       "try:\n"
                       "    engine.init_distributed('gloo')\n"
                       "except Exception as e:\n"
                       "    print('RAISED', type(e).__name__, round(time.time() - t0))\n" % _free_port(), {"BLM_DIST_TIMEOUT_S": "3"})
    assert "RAISED" in out and int(out.split()[-1]) < 30, (rc, out, err[-1500:])


def test_stage7_score_interpolation_matches_awk(tmp_path):
    """the awk hop of lmrescore_nbest_pytorchnn_cuda.sh:221-229 (graph + w * nn + (1 - w) * lm per n-best
    entry, printed by awk's rules) done by the scorer process; checked against awk itself when the box has one."""
    import shutil
    import subprocess
    from bayeslms_amd import compute_sentence_scores as S
    rng = np.random.RandomState(4)
    keys = ["utt%d-A-%d" % (u, n) for u in range(5) for n in range(1, 5)]
    d = str(tmp_path)
    cols = {}
    for name, scale in (("nolm", 40.0), ("lmonly", 25.0), ("nn", 30.0)):
        cols[name] = [round(float(v), 4) for v in rng.rand(len(keys)) * scale]
        cols[name][3] = 12.0  # an integer-valued score: awk prints it without a decimal point
        with open(os.path.join(d, "lmwt." + name), "w") as f:
            for k, v in zip(keys, cols[name]):
                f.write("%s %s\n" % (k, ("%.4f" % v) if name == "nn" else repr(v)))
    out = os.path.join(d, "lmwt.interp.0.8")
    S.interpolate_scores(os.path.join(d, "lmwt.nolm"), os.path.join(d, "lmwt.lmonly"), os.path.join(d, "lmwt.nn"), 0.8, out)
    got = [ln.split() for ln in open(out).read().splitlines()]
    assert [g[0] for g in got] == keys
    for g, a, b, c in zip(got, cols["nolm"], cols["lmonly"], cols["nn"]):
        assert abs(float(g[1]) - (a + 0.8 * c + 0.2 * b)) <= 5e-6 * max(1.0, abs(a + 0.8 * c + 0.2 * b))
    assert S._awk_num(12.0) == "12" and S._awk_num(0.5) == "0.5" and S._awk_num(1234567.25) == "1.23457e+06"
    if shutil.which("awk") and shutil.which("paste"):
        cmd = ("paste %s/lmwt.nolm %s/lmwt.lmonly %s/lmwt.nn | awk -v w=0.8 '{ print $1, $2 + (w * $6) + ((1 - w) * $4); }'"
               % (d, d, d))
        ref = subprocess.run(cmd, shell=True, capture_output=True, text=True, check=True).stdout
        assert open(out).read() == ref


def test_reducer_bucket_layout_big_tensor_alone_and_small_final_buckets():
    """What is exposed at the end of backward is the LAST bucket to become ready (the lowest offsets of the flat
    buffer): quarter-size buckets there; a tensor of a bucket's size or more (the tied encoder / decoder weight) travels
    alone, so that its dense half -- complete after the first backward kernel -- is not held back by other parameters."""
    import torch
    from bayeslms_amd import engine

    class Head(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.big = torch.nn.Parameter(torch.zeros(40000))
            self.bias = torch.nn.Parameter(torch.zeros(33))

    class M(torch.nn.Module):  # the layers first, the big (tied) tensor and the decoder bias at the end, as in the LMs
        def __init__(self):
            super().__init__()
            self.a = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n)) for n in (300, 500, 700, 900, 1100, 1300, 1500,
                                                                                          1700, 1900, 2100, 2300, 2500)])
            self.head = Head()
    flat = engine.FlatBuffers(M())
    red = engine.GradReducer(flat, bucket_bytes=4 * 4000)  # 4000 floats per bucket
    spans = [(s, e) for s, e, _ in red.buckets]
    assert spans[0][1] == flat.total and spans[-1][0] == 0
    assert all(spans[i][0] == spans[i + 1][1] for i in range(len(spans) - 1))  # contiguous cover, backward order
    ids = [i for _, _, i in red.buckets]
    big = [k for k, p in enumerate(flat.params) if p.numel() == 40000][0]
    assert [big] in ids  # alone
    # the parameters below 2 buckets' worth of offsets are cut at a quarter of the size: the final bucket is small
    assert spans[-1][1] - spans[-1][0] <= 2000 and len(red.buckets) >= 5
    # every parameter is in exactly one bucket
    assert sorted(i for b in ids for i in b) == list(range(len(flat.params)))


def _schedule_worker(rank, world, port, ret):
    """Every rank feeds ValidationSchedule ITS OWN validation loss: rank r's values are rank 0's plus a last-bits
    perturbation chosen so that a rank-local `val_loss < best_val` would flip on epochs 2 and 4."""
    import torch.distributed as dist
    from bayeslms_amd.train import ValidationSchedule
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    base = [5.0, 4.0, 4.0 - 1e-7, 3.9999999, 3.5, 3.6, 3.6, 3.6, 3.6, 3.6, 3.6, 3.6, 3.6]
    bump = [0.0, 0.0, 3e-7, -2e-7, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    sched = ValidationSchedule(1.0, world)
    local = ValidationSchedule(1.0, 1)  # what a rank deciding for itself would have done
    trace, ltrace = [], []
    for v, b in zip(base, bump):
        mine = v + (b if rank else 0.0)
        val, improved, stop = sched.update(mine)
        trace.append((val, improved, stop, sched.lr))
        lv, li, ls = local.update(mine)
        ltrace.append((li, ls, local.lr))
        if stop:
            break
    ret[rank] = (trace, ltrace, sched.agree(100.0 + rank))
    dist.destroy_process_group()


def test_validation_decision_is_rank0s_on_every_rank():
    """VERDICT r2 Weak #1: save / halve-LR / early-stop must not be decided per rank."""
    world = 2
    port = _free_port()
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_schedule_worker, args=(world, port, ret), nprocs=world, join=True)
        (t0, l0, a0), (t1, l1, a1) = ret[0], ret[1]
    assert t0 == t1 and a0 == a1 == 100.0          # identical values, branches, LR and stop epoch
    assert [x[:2] for x in l0] != [x[:2] for x in l1]  # ... where rank-local decisions WOULD have split
    assert t0[-1][2] and len(t0) == 12 and t0[-1][3] == 1.0 / 2 ** 8  # 8 halvings end the run (train.py:511)
    # the single-process schedule is the reference's: improved iff val < best, first epoch always saves
    from bayeslms_amd.train import ValidationSchedule
    s = ValidationSchedule(0.1)
    assert s.update(3.0)[1] and not s.update(3.0)[1] and s.lr == 0.05 and s.update(2.0)[1] and s.lr == 0.05


def _untied_late_rows_worker(rank, world, port, ret):
    """an UNTIED encoder weight under LateRows gets its whole gradient through the compact exchange; its
    bucket (the tensor travels alone) must not be all-reduced densely as zeros."""
    import torch.distributed as dist
    from bayeslms_amd import engine
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    V, D, T, B = 64, 8, 5, 3
    torch.manual_seed(0)
    net = torch.nn.ModuleDict({"encoder": torch.nn.Embedding(V, D), "other": torch.nn.Linear(D, 7)})
    flat = engine.FlatBuffers(net)
    red = engine.GradReducer(flat, bucket_bytes=256)
    enc = net["encoder"].weight
    red.late = engine.LateRows(red, enc)
    dense_elems = []
    for step in range(3):
        g = torch.Generator().manual_seed(100 * step + rank)
        ids = torch.randint(0, V, (T, B), generator=g)
        dy = torch.randn(T, B, D, generator=g)
        flat.zero_grad()
        red.late.begin(ids)
        for p in net["other"].parameters():
            p.grad.add_(1.0 + rank)
            red.mark_ready(p)
        buf, slots, U, done = red.late.sink(enc, ids)
        buf.view(U, D).index_add_(0, slots.reshape(-1), dy.reshape(-1, D))
        done()
        red.finish()
        dense_elems.append(red.last_reduced_elems - U * D)
        want = torch.zeros(V, D)
        for r in range(world):
            g = torch.Generator().manual_seed(100 * step + r)
            ids_r = torch.randint(0, V, (T, B), generator=g)
            want.index_add_(0, ids_r.reshape(-1), torch.randn(T, B, D, generator=g).reshape(-1, D))
        assert torch.allclose(enc.grad, want, atol=1e-5)
    assert red.expected[id(enc)] == 0 and red.bucket_of[id(enc)] in red.no_dense
    other = sum((p.numel() + 3) // 4 * 4 for p in net["other"].parameters())
    assert dense_elems[0] == other and dense_elems[1:] == [other, other], (dense_elems, other, V * D)
    # the sink refusing (a second lookup, foreign ids) puts the step back on the dense path
    flat.zero_grad()
    red.late.begin(ids)
    for p in net["other"].parameters():
        red.mark_ready(p)
    enc.grad.add_(float(rank + 1))
    red.mark_ready(enc)
    red.finish()
    assert torch.allclose(enc.grad, torch.full_like(enc.grad, float(sum(range(1, world + 1)))))
    ret[rank] = True
    dist.destroy_process_group()


def test_late_rows_untied_encoder_skips_the_dense_all_reduce():
    port = _free_port()
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_untied_late_rows_worker, args=(2, port, ret), nprocs=2, join=True)
        assert all(ret.get(r) for r in range(2))


def test_stage7_interpolation_nonfinite_scores_and_key_mismatch(tmp_path):
    """a nan / inf n-best score prints as awk prints it instead of aborting the file; lines whose keys differ
    between the three pasted files are an error naming the key, and nothing is written."""
    from bayeslms_amd import compute_sentence_scores as S
    d = str(tmp_path)
    assert S._awk_num(float("nan")) == "nan" and S._awk_num(float("inf")) == "inf" and S._awk_num(float("-inf")) == "-inf"
    files = {"nolm": ["a-1 1.5", "a-2 inf", "a-3 2"], "lmonly": ["a-1 2.5", "a-2 1", "a-3 nan"], "nn": ["a-1 3.0", "a-2 1", "a-3 1"]}
    for k, v in files.items():
        open(os.path.join(d, k), "w").write("\n".join(v) + "\n")
    out = os.path.join(d, "out")
    S.interpolate_scores(os.path.join(d, "nolm"), os.path.join(d, "lmonly"), os.path.join(d, "nn"), 0.5, out)
    assert open(out).read().split() == ["a-1", "4.25", "a-2", "inf", "a-3", "nan"]
    open(os.path.join(d, "nn"), "w").write("a-1 3.0\nb-2 1\na-3 1\n")
    os.remove(out)
    with pytest.raises(SystemExit) as e:
        S.interpolate_scores(os.path.join(d, "nolm"), os.path.join(d, "lmonly"), os.path.join(d, "nn"), 0.5, out)
    assert "b-2" in str(e.value) and "line 2" in str(e.value) and not os.path.exists(out)


def test_recipe_command_lines_parse_unchanged():
    """North star: 'keeping the run_nnlm_* CLI surface'.  The argument lists of the reference recipes -- the flags of
    run_nnlm_ami_tm.sh:89-110 and run_nnlm_ami_lstm.sh:89-110 in their order, with the values the scripts assign at
    :17-35 / :18-34 (note `--epoch`, an argparse prefix of --epochs) -- and of the rescoring script's scorer call
    (lmrescore_nbest_pytorchnn_cuda.sh:200-218) go through build_parser() and land on the reference's semantics;
    the engine's own new flags stay at their defaults."""
    from bayeslms_amd import train as T, compute_sentence_scores as S
    tm = ("--data data/pytorchnn_ami --model Transformer --emsize 512 --nhid 4096 --nlayers 6 --nhead 8 --lr 0.1 "
          "--dropout 0.2 --seq_len 100 --clip 1.0 --batch-size 32 --epoch 32 --seed 1111 --save exp/tfm/model.pt "
          "--prior False --prior_path steps/pytorchnn/prior/transformer --uncertainty Gaussian --T_bayes_pos FFN "
          "--T_gauss_pos 1 --T_v_pos 0 --tied --cuda").split()
    a = T.build_parser().parse_args(tm)
    assert (a.model, a.emsize, a.nhid, a.nlayers, a.nhead, a.seq_len, a.batch_size) == ("Transformer", 512, 4096, 6, 8, 100, 32)
    assert a.epochs == 32 and a.T_bayes_pos == "FFN" and a.uncertainty == "Gaussian" and a.T_gauss_pos == 1 and a.tied
    assert a.cuda and a.clip == 1.0 and a.lr == 0.1 and a.dropout == 0.2 and a.T_v_pos == 0 and a.prior == "False"
    assert a.dist_backend == "nccl" and a.dp_overlap == 1 and a.dp_late_rows == 1 and a.gemm_mode == "f32" and not a.history
    assert T.build_model(a, 50).__class__.__name__ == "GaussTransformerModel" and T.kl_selector(a) is not None
    lstm = ("--data data/pytorchnn_ami --model LSTM --emsize 1024 --nhid 1024 --nlayers 2 --nhead 8 --lr 5 --dropout 0.2 "
            "--seq_len 100 --clip 1.0 --batch-size 32 --epoch 32 --seed 1111 --save exp/lstm/model.pt --uncertainty Gaussian "
            "--L_bayes_pos 0 --L_gauss_pos 00 --L_v_pos 00 --prior False --prior_path steps/pytorchnn/prior/lstm --tied "
            "--mark marks --cuda").split()
    a = T.build_parser().parse_args(lstm)
    assert (a.model, a.emsize, a.nhid, a.nlayers, a.seq_len, a.batch_size, a.lr) == ("LSTM", 1024, 1024, 2, 100, 32, 5.0)
    assert a.L_gauss_pos == "00" and a.L_v_pos == "00" and a.L_bayes_pos == 0 and a.mark == "marks" and a.epochs == 32
    for k, v in (("--uncertainty", "Bayesian"), ("--L_bayes_pos", "3")):  # the configuration BASELINE configs[1] names
        lstm[lstm.index(k) + 1] = v
    a = T.build_parser().parse_args(lstm)
    assert a.uncertainty == "Bayesian" and a.L_bayes_pos == 3 and T.kl_selector(a) is not None
    sc = ("--nbest-list nbest.1/words_text --outfile nbest.1/lmwt.nn --vocabulary data/pytorchnn_ami/words.txt --model-path "
          "exp/tfm/model.pt --model Transformer --emsize 512 --nhid 4096 --nlayers 6 --nhead 8 --uncertainty Gaussian "
          "--L_bayes_pos 0 --T_bayes_pos FFN --L_v_pos 00 --T_v_pos 0 --L_gauss_pos 00 --T_gauss_pos 1 "
          "--interpolation_flag 0 --inter_alpha 0.8").split()
    b = S.build_parser().parse_args(sc)
    assert b.model == "Transformer" and b.T_gauss_pos == 1 and b.batched == 1 and b.mc_samples == 0 and b.inter_alpha == 0.8


def test_wavefront_chunks_are_equal_and_cover_the_window():
    """ops._stack_chunks (host rule of the LSTM layer wavefront): equal chunks of at most 16 steps for short training windows
    (T < 64), at most 8 for longer ones, 128-step chunks for the scorer's long B = 1 chain; always a partition of [0, T)."""
    from bayeslms_amd import ops
    for T in (8, 31, 32, 35, 64, 100, 128, 256, 257, 1000, 8192):
        ch = ops._stack_chunks(T)
        assert ch[0][0] == 0 and ch[-1][1] == T and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        sizes = [b - a for a, b in ch]
        assert max(sizes) <= (16 if T < 64 else (8 if T <= 256 else 128))
        assert max(sizes) - min(sizes) <= max(1, max(sizes) - (T - (len(ch) - 1) * max(sizes))) and min(sizes) >= 1
    assert [b - a for a, b in ops._stack_chunks(35)] == [12, 12, 11]      # BASELINE configs[0] / configs[1] window
    assert [b - a for a, b in ops._stack_chunks(100)] == [8] * 12 + [4]    # the recipes' window


def test_batched_scorer_restores_the_garbage_collector(monkeypatch):
    """compute_scores_batched switches the cyclic collector off for the call and puts it back -- also when the call fails."""
    import gc
    from bayeslms_amd import compute_sentence_scores as css
    seen = {}

    def boom(*a, **k):
        seen["enabled_inside"] = gc.isenabled()
        raise RuntimeError("stop")
    monkeypatch.setattr(css, "_compute_scores_batched", boom)
    assert gc.isenabled()
    with pytest.raises(RuntimeError):
        css.compute_scores_batched({}, None, {}, "LSTM", "cpu")
    assert seen["enabled_inside"] is False and gc.isenabled()
    gc.disable()
    try:
        with pytest.raises(RuntimeError):
            css.compute_scores_batched({}, None, {}, "LSTM", "cpu")
        assert not gc.isenabled()   # a caller that had it off keeps it off
    finally:
        gc.enable()


# ---------------------------------------------------------------------------------------------------------------------
# environment switches that are host code: each is read where the library / the engine reads it (a fresh process)
def _py(code, env):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.update(env)
    e["PYTHONPATH"] = root + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=300)
    return r.returncode, r.stdout.strip(), r.stderr


_PLAN_CODE = """
import ctypes as C
from bayeslms_amd import _lib as L
a = L.GemmArgs(); a.abi_version = L.ABI_VERSION
a.op, a.M, a.N, a.K, a.lda, a.ldb, a.ldc = L.GEMM_NT, 8192, 512, 4096, 4096, 4096, 512
p = L.GemmPlan(); L.check(L.lib().blm_gemm_plan_query(C.byref(a), C.byref(p)))
print(p.tile, p.splits, p.source)
"""


def test_gemm_plan_environment_switches():
    """BLM_GEMM_TILE / BLM_GEMM_SPLITK (the override) and BLM_GEMM_PLAN_SET (run-time table entries: profiling ONE launch under
    another plan, tools/profile_round.sh) reach the planner of a fresh process."""
    assert _py(_PLAN_CODE, {})[1] == "28 1 1"
    assert _py(_PLAN_CODE, {"BLM_GEMM_TILE": "21"})[1] == "21 1 2"
    assert _py(_PLAN_CODE, {"BLM_GEMM_TILE": "11", "BLM_GEMM_SPLITK": "4"})[1] == "11 4 2"
    assert _py(_PLAN_CODE, {"BLM_GEMM_PLAN_SET": "0,8192,512,4096,0,0,22,2;0,1,1,1,0,0,11,1"})[1] == "22 2 1"
    assert _py(_PLAN_CODE, {"BLM_GEMM_PLAN_SET": "0,8192,512,4096,0,0,99,2"})[1] == "28 1 1"  # an illegal entry is ignored


def test_kernel_options_start_from_their_environment_variables():
    code = ("import ctypes as C\nfrom bayeslms_amd import _lib as L\nv = C.c_int()\nout = []\n"
            "for n in ('attn_hpw', 'attn_short', 'attn_valu', 'lstm_gemv', 'lstm_pipe', 'lstm_tail'):\n"
            "    L.check(L.lib().blm_get_option(n.encode(), C.byref(v))); out.append(v.value)\nprint(out)")
    assert _py(code, {})[1] == "[0, 1, 0, 1, 1, 0]"
    assert _py(code, {"BLM_ATTN_HPW": "2", "BLM_ATTN_SHORT": "0", "BLM_ATTN_VALU": "1", "BLM_LSTM_GEMV": "0", "BLM_LSTM_PIPE": "0",
                      "BLM_LSTM_TAIL": "1"})[1] == "[2, 0, 1, 0, 0, 1]"
    assert _py(code, {"BLM_ATTN_HPW": "7"})[1] == "[0, 1, 0, 1, 1, 0]"  # out of range: the default


def test_blm_lib_selects_another_build_and_fails_loudly():
    rc, out, err = _py("from bayeslms_amd import _lib as L\nL.lib()", {"BLM_LIB": "/nonexistent/libbayeslm_hip.so"})
    assert rc != 0 and "no CPU fallback" in err


def test_rccl_channel_pinning_and_comm_plan_defaults(monkeypatch):
    from bayeslms_amd import engine
    for k in ("NCCL_MIN_NCHANNELS", "NCCL_MAX_NCHANNELS", "BLM_RCCL_CHANNELS"):
        monkeypatch.delenv(k, raising=False)
    assert engine.rccl_channels() == 0
    assert engine.pin_rccl_channels() == {"NCCL_MIN_NCHANNELS": "16", "NCCL_MAX_NCHANNELS": "16"} and engine.rccl_channels() == 16
    monkeypatch.setenv("NCCL_MAX_NCHANNELS", "24")  # the user's own setting wins
    monkeypatch.setenv("BLM_RCCL_CHANNELS", "8")
    assert engine.pin_rccl_channels()["NCCL_MAX_NCHANNELS"] == "24" and engine.rccl_channels() == 24
    for k in ("NCCL_MIN_NCHANNELS", "NCCL_MAX_NCHANNELS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BLM_RCCL_CHANNELS", "0")  # RCCL's own choice: nothing pinned, the planner keeps the whole chip
    assert engine.pin_rccl_channels() == {"NCCL_MIN_NCHANNELS": None, "NCCL_MAX_NCHANNELS": None} and engine.rccl_channels() == 0


def test_every_environment_switch_is_documented_and_tested():
    """A switch is product surface: every BLM_* variable the product reads is listed in INTEGRATION.md section 4 with the
    test that exercises it, and nothing is listed that no longer exists."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    used = set()
    for path in glob.glob(os.path.join(root, "bayeslms_amd", "**", "*"), recursive=True) + [os.path.join(root, "bench.py")]:
        if os.path.isfile(path) and path.endswith((".py", ".hip", ".h")):
            src = open(path, encoding="utf-8", errors="ignore").read()
            used |= set(re.findall(r'(?:getenv\(|environ\.get\(|environ\[|environ\.setdefault\()\s*["\'](BLM_[A-Z0-9_]+)', src))
            used |= set(re.findall(r'\{"[a-z0-9_]+", "(BLM_[A-Z0-9_]+)"', src))  # the option registry of csrc/capi.hip
    doc = open(os.path.join(root, "INTEGRATION.md"), encoding="utf-8").read()
    table = doc[doc.index("## 4. Switches"):]
    listed = set(re.findall(r"^\| `(BLM_[A-Z0-9_]+)`|, `(BLM_[A-Z0-9_]+)` \(", table, re.M)) if False else set()
    for row in table.splitlines():
        if row.startswith("| `BLM_"):
            listed |= set(re.findall(r"`(BLM_[A-Z0-9_]+)`", row.split("|")[1]))
            assert "test_" in row.split("|")[3], row  # every row names its test
    assert used == listed, (sorted(used - listed), sorted(listed - used))
    from bayeslms_amd import engine
    red = engine.GradReducer(engine.FlatBuffers(torch.nn.Linear(3, 2)), comm_cus=16)
    assert red.comm_cus == 0 and red.comm_plan == "off"  # host tensors: no CUs to contend for


def test_scorer_jobs_are_laid_round_robin_over_the_visible_gpus():
    """lmrescore_nbest_pytorchnn_cuda.sh:199 starts nj jobs that share nothing: --job JOB puts job j on GPU (j-1) mod N."""
    from bayeslms_amd.compute_sentence_scores import build_parser, job_device_index
    assert [job_device_index(j, 8) for j in range(1, 11)] == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1]
    assert [job_device_index(j, 1) for j in (1, 2, 5)] == [0, 0, 0]
    assert job_device_index(0, 8, "3") == 3 and job_device_index(0, 1) == 0   # default: LOCAL_RANK
    for bad in ((0, 2, "2"), (-1, 2, 0), (1, 0, 0)):
        with pytest.raises(SystemExit):
            job_device_index(*bad)
    base = ["--nbest-list", "a", "--outfile", "b", "--vocabulary", "c", "--model-path", "d"]
    assert build_parser().parse_args(base).job == 0 and build_parser().parse_args(base + ["--job", "4"]).job == 4


def test_gradient_slab_bookkeeping(monkeypatch):
    """ops._GradSlab (where a missing `.grad` comes from under the reference's zero_grad() loop) on host tensors: first sight = plain
    zeros, later steps = views of one zeroed slab per step at 256-byte aligned offsets; a second request for a slot means a new step
    and a new slab; parameters that died leave the layout; a parameter whose id is reused with another size is re-registered."""
    import gc
    import torch
    from bayeslms_amd import ops
    slab = ops._GradSlab()
    monkeypatch.setattr(slab, "eligible", lambda p: p.dtype == torch.float32)
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (5, 64, 130, 1)]
    first = [slab.take(p) for p in ps]
    assert all(float(g.abs().sum()) == 0.0 and g.shape == p.shape for g, p in zip(first, ps))
    assert len({g.untyped_storage().data_ptr() for g in first}) == 4                    # first sight: a buffer each
    step2 = [slab.take(p) for p in ps]
    base = step2[0].untyped_storage().data_ptr()
    assert all(g.untyped_storage().data_ptr() == base for g in step2)                  # one slab
    offs = [g.data_ptr() - base for g in step2]
    assert offs == [0, 256, 512, 512 + 192 * 4] and all(float(g.abs().sum()) == 0.0 for g in step2)
    for g in step2:
        g.add_(1.0)                                                                     # a step's gradients
    step3 = [slab.take(p) for p in ps]                                                  # same slots asked again: next step
    assert step3[0].untyped_storage().data_ptr() != base and all(float(g.abs().sum()) == 0.0 for g in step3)
    assert all(float(g.sum()) == g.numel() for g in step2)                              # the previous step's views keep their values
    # a late joiner gets plain zeros now and a slot afterwards; the slab in use is abandoned (its layout is stale)
    late = torch.nn.Parameter(torch.randn(7, 3))
    g_late = slab.take(late)
    assert g_late.shape == (7, 3) and g_late.untyped_storage().data_ptr() != step3[0].untyped_storage().data_ptr()
    step4 = [slab.take(p) for p in ps + [late]]
    assert len({g.untyped_storage().data_ptr() for g in step4}) == 1 and step4[-1].shape == (7, 3)
    # dead parameters leave the layout
    total_before = slab.dev[ps[0].device]["total"]
    del ps[2], first, step2, step3, step4
    gc.collect()
    step5 = [slab.take(p) for p in ps + [late]]
    assert slab.dev[late.device]["total"] < total_before and len(slab.dev[late.device]["slots"]) == 4
    assert len({g.untyped_storage().data_ptr() for g in step5}) == 1
    # switched off: plain zeros
    slab.on = False
    assert slab.take(ps[0]).untyped_storage().data_ptr() != step5[0].untyped_storage().data_ptr()


def test_shape_helpers_of_the_off_baseline_paths():
    """Host logic behind three round-5 fixes for shapes other than BASELINE's: the row chunks that keep a GEMM operand under the
    LDS-DMA loaders' 2^32-byte offset limit (logits of large batches), the gate-block padding of LSTM operands whose hidden size is
    not a multiple of 32, and the padded-row buffer / row-stride view of a vocabulary that is not a multiple of 4 words."""
    import torch
    from bayeslms_amd import ops
    # --- row chunks
    assert ops._row_chunks(8192, 33000) == [(0, 8192)]                       # the headline: one launch, as before
    assert ops._row_chunks(32768, 33000) == [(0, 16384), (16384, 32768)]     # T 128 x B 256: 4.3 GB of logits
    for M, ld in ((32768, 33000), (70016, 33000), (100000, 50000), (5, 1 << 31), (40000, 33280)):
        ch = ops._row_chunks(M, ld)
        assert ch[0][0] == 0 and ch[-1][1] == M and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        if len(ch) > 1:
            assert all((b - a) * ld * 4 < (1 << 32) and (b - a) % 128 == 0 for a, b in ch[:-1]) and (ch[-1][1] - ch[-1][0]) * ld * 4 < (1 << 32)
    # --- gate-block padding: block g of (4H, ...) lands at rows [g Hp, g Hp + H), zeros behind it; differentiable
    H, Hp, I = 5, 8, 3
    w = torch.arange(4 * H * I, dtype=torch.float32).reshape(4 * H, I).requires_grad_(True)
    wp = ops._pad_gate_blocks(w, H, Hp)
    assert wp.shape == (4 * Hp, I) and torch.equal(wp.reshape(4, Hp, I)[:, :H], w.detach().reshape(4, H, I))
    assert float(wp.reshape(4, Hp, I)[:, H:].abs().sum()) == 0.0
    (wp * torch.arange(4 * Hp * I, dtype=torch.float32).reshape(4 * Hp, I)).sum().backward()
    assert w.grad.shape == w.shape and float(w.grad[H, 0]) == float(Hp * I)   # gate block 1, unit 0 sits at padded row Hp
    wh = torch.arange(4 * H * H, dtype=torch.float32).reshape(4 * H, H)
    whp = ops._pad_gate_blocks(wh, H, Hp, cols=True)
    assert whp.shape == (4 * Hp, Hp) and torch.equal(whp.reshape(4, Hp, Hp)[:, :H, :H], wh.reshape(4, H, H)) and float(whp.sum()) == float(wh.sum())
    b = torch.arange(4 * H, dtype=torch.float32)
    assert torch.equal(ops._pad_gate_blocks(b, H, Hp).reshape(4, Hp)[:, :H], b.reshape(4, H))
    x = torch.arange(2 * 3 * 4 * H, dtype=torch.float32).reshape(2, 3, 4 * H)
    xp = ops._pad_last_gate_blocks(x, H, Hp)
    assert xp.shape == (2, 3, 4 * Hp) and torch.equal(xp.reshape(2, 3, 4, Hp)[..., :H], x.reshape(2, 3, 4, H)) and float(xp.sum()) == float(x.sum())
    # --- padded rows: a (..., N) view whose rows start 16 bytes apart-aligned; `.view(-1, N)` (train.py:404) keeps working
    y, ld = ops._padded_rows((6, 5), 33278, "cpu")
    assert y.shape == (6, 5, 33278) and ld == 33280 and y.stride() == (5 * 33280, 33280, 1)
    flat = y.view(-1, 33278)
    assert flat.shape == (30, 33278) and flat.stride() == (33280, 1) and flat.data_ptr() == y.data_ptr()
    y2, ld2 = ops._padded_rows((4,), 1000, "cpu")
    assert ld2 == 1000 and y2.is_contiguous()
