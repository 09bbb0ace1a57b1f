"""GPU: engine.evaluate_report -- mean-weight loss against engine.evaluate, the Monte-Carlo report against a float64 reference
formed from S ordinary forwards with materialised logits, refusals, the state the model is left in, and the two command lines.

Small models built here (V 1000, d 64, 2 layers, 2 heads, ff 128; LSTM H 64) over a synthetic text of 3,000 tokens: 10 columns
and seq_len 16 give the Transformers one batch of 18 grouped windows and a ragged last window of 11 rows; the LSTM runs on 40
columns, where engine.evaluate groups three windows, carries its state into a second batch and ends on a ragged window."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from bayeslms_amd import BayesLMError

pytestmark = pytest.mark.gpu

V, SEQ, S = 1000, 16, 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def text():
    from bayeslms_amd import data as D
    return D.synthetic_corpus(V, 3000, seed=7)


def _model(kind, dev, lgstd=None):
    from bayeslms_amd import model as M
    torch.manual_seed(11)
    if kind == "tlm_plain":
        m = M.TransformerModel(V, 64, 2, 128, 2, 0.2, "gelu", True)
    elif kind == "tlm_ffn":
        m = M.BayesTransformerModel(V, 64, 2, 128, 2, 0.2, True, "FFN")
    elif kind == "tlm_gauss":
        m = M.GaussTransformerModel(V, 64, 2, 128, 2, 0.2, True, 3)
    elif kind == "lstm_bayes3":
        m = M.BayesRNNModel("LSTM", V, 64, 64, 2, 0.2, True, 3)
    else:
        m = M.VariationalRNNModel("LSTM", V, 64, 64, 2, 0.2, True, "11")
    if kind.startswith("lstm"):
        # the LSTMs' initialisation (weights in +-0.1) leaves the next-word distribution almost flat (mean confidence 1.07e-3 over
        # 1000 words, 7.5 % of the tokens with a top-two gap under 1e-4): the tied embedding / decoder is widened so that ties
        # are as rare as in a trained model
        with torch.no_grad():
            m.encoder.weight.mul_(10.0)
    # every log sigma raised by 1.5, as the Monte-Carlo tests of the scorer and of IncrementalLM raise theirs: at initialisation
    # the mutual information is 2e-4 .. 4e-3 nats per token, where the ~4e-8 absolute error of a float32 mi is 1e-5 .. 2e-4 of
    # the mean and the 2e-5 relative bar on mean_mi would measure that rounding, not the report
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "lgstd" in k:
                p.add_(1.5) if lgstd is None else p.fill_(lgstd)
    return m.to(dev).eval()


def _source(text, kind, dev):
    from bayeslms_amd import data as D
    return D.batchify(text, 40 if kind.startswith("lstm") else 10, dev)


def _rel(name, got, want, rel=2e-5):
    print("%s: got %.9g want %.9g" % (name, got, want))
    assert abs(got - want) <= rel * abs(want), (name, got, want)


# ------------------------------------------------------------------------------------------------------------ mean weights
@pytest.mark.parametrize("kind", ["tlm_plain", "tlm_ffn", "lstm_bayes3"])
def test_mean_weight_loss_is_engine_evaluate(dev, text, kind):
    from bayeslms_amd import engine
    m, src = _model(kind, dev), _source(text, kind, dev)
    want = engine.evaluate(m, src, SEQ)
    rep = engine.evaluate_report(m, src, SEQ, keep_tokens=True)
    print("%s: evaluate %.9f report %.9f" % (kind, want, rep.loss))
    assert abs(rep.loss - want) <= 2e-6
    n = (src.shape[0] - 1) * src.shape[1]
    assert (rep.tokens, rep.skipped, rep.mc_samples) == (n, 0, 0) and rep.ppl == math.exp(rep.loss)
    assert rep.sample_loss is None and rep.mean_mi is None and len(rep.bins) == 15 and sum(b[0] for b in rep.bins) == n
    assert 0.0 <= rep.accuracy <= rep.top5_accuracy <= 1.0 and 0.0 <= rep.ece <= 1.0
    # per-token arrays come back in text order: column c of the batchified stream is a contiguous stretch of the text
    assert rep.per_token["tgt"].tolist() == src[1:].t().reshape(-1).tolist()
    assert not m.training
    # the two walks hand the model the same batches in the same order (the loss, a sum, would not notice another grouping)
    seen = []
    hook = m.register_forward_pre_hook(lambda mod, args: seen.append(args[0].clone()))
    try:
        engine.evaluate(m, src, SEQ)
        n_eval = len(seen)
        engine.evaluate_report(m, src, SEQ)
    finally:
        hook.remove()
    assert n_eval >= 2 and len(seen) == 2 * n_eval
    assert all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(seen[:n_eval], seen[n_eval:]))


# ------------------------------------------------------------------------------------------------------------ Monte-Carlo
def _reference(m, src, seed):
    """S ordinary forwards under model.mc_sampling, window by window, logits materialised -> float64 per-token arrays in text
    order: bma_nll, conf, h_pred, mi, nll_s (tokens, S), pred, rank, the top-two gap of log pbar, the smallest distance of
    another word's log pbar from the target's, and the words clearly ahead of the target (rank_lo: by more than 1e-4) and not
    clearly behind it (rank_hi: within 1e-4 or ahead)."""
    from bayeslms_amd import model as M
    from bayeslms_amd.data import get_batch
    rows, cols = src.shape
    recurrent = hasattr(m, "init_hidden")
    out = {k: [] for k in ("nll", "conf", "h", "mi", "nll_s", "pred", "rank", "gap", "tgap", "rank_lo", "rank_hi")}
    idx = torch.arange(V, device=src.device).view(1, V)
    with torch.no_grad(), M.mc_sampling(m, seed, S):
        hidden = [m.init_hidden(cols) for _ in range(S)] if recurrent else None
        for i in range(0, rows - 1, SEQ):
            data, tgt = get_batch(src, i, SEQ)
            lp = []
            for s in range(S):
                m.set_step(s)
                if recurrent:
                    y, h = m(data, hidden[s])
                    hidden[s] = M.repackage_hidden(h)
                else:
                    y = m(data)
                lp.append(torch.log_softmax(y.reshape(-1, V).double(), -1))
            lp = torch.stack(lp)
            lpbar = torch.logsumexp(lp, 0) - math.log(S)
            tv = lpbar.gather(1, tgt.view(-1, 1))
            top2 = lpbar.topk(2, -1).values
            others = (lpbar - tv).abs()
            others.scatter_(1, tgt.view(-1, 1), float("inf"))
            vals = {"nll": -tv.squeeze(1), "conf": top2[:, 0].exp(), "h": -(lpbar.exp() * lpbar).sum(-1),
                    "mi": (lp.exp() * (lp - lpbar)).sum(-1).mean(0), "nll_s": -lp.gather(2, tgt.view(1, -1, 1).expand(S, -1, 1)).squeeze(2).t(),
                    "pred": lpbar.argmax(-1), "rank": (lpbar > tv).sum(-1) + ((lpbar == tv) & (idx < tgt.view(-1, 1))).sum(-1),
                    "gap": top2[:, 0] - top2[:, 1], "tgap": others.min(-1).values,
                    "rank_lo": (lpbar > tv + 1e-4).sum(-1), "rank_hi": (lpbar >= tv - 1e-4).sum(-1) - 1}
            for k, v in vals.items():
                out[k].append(v.reshape(len(data), cols, -1))
    return {k: torch.cat(v).transpose(0, 1).reshape((rows - 1) * cols, -1).squeeze(-1).cpu().numpy() for k, v in out.items()}


def _within(name, got, want, rel=2e-5):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    worst = float((np.abs(got - want) / np.maximum(np.abs(want), 1.0)).max())
    print("%s: max |got - want| over the bound's scale %.3e (bound %.1e)" % (name, worst, rel))
    assert worst <= rel, (name, worst)


@pytest.mark.parametrize("kind", ["tlm_ffn", "tlm_gauss", "lstm_bayes3"])
def test_mc_report_equals_float64_of_s_forwards(dev, text, kind):
    """Per token within the bounds of test_gpu_mc_uncertainty._check; loss, sample_loss and the means 2e-5 relative: this pins
    the sample indexing, the S carried states and the grouping.

    pred, accuracy and ece are compared on the tokens whose reference top-two gap of log pbar is >= 1e-4 (a different GEMM plan
    may flip a nearer tie); at most 1 % of the tokens may be left out.  rank counts comparisons against the TARGET's value, so
    the top-two gap says nothing about it: it is held equal where no other word's log pbar lies within 1e-4 of the target's, and
    EVERYWHERE it must lie between the counts of words clearly ahead (> target + 1e-4) and not clearly behind
    (>= target - 1e-4) in the reference.  The share of targets with such a neighbour is capped at 20 %: V words whose log pbar has
    standard deviation sigma put at most V * 0.4 / sigma words per nat around a target, 2e-4 nats wide that is 0.08 / sigma
    neighbours expected at V = 1000, and sigma is 0.4 or more for these models (measured: 10.8 % and 11.7 % for the Transformers
    before their sigmas were raised; fp32 rounding flipped 1, 0 and 5 of ~2990 ranks).  top-5 accuracy may differ by the tokens
    whose interval [rank_lo, rank_hi] straddles 5, and by no more."""
    from bayeslms_amd import engine
    m, src = _model(kind, dev), _source(text, kind, dev)
    want = _reference(m, src, 1111)
    rep = engine.evaluate_report(m, src, SEQ, mc_samples=S, keep_tokens=True)
    t = rep.per_token
    n = (src.shape[0] - 1) * src.shape[1]
    assert (rep.tokens, rep.skipped, rep.mc_samples) == (n, 0, S) and t["nll_s"].shape == (n, S)
    _within("bma_nll", t["nll"], want["nll"])
    _within("nll_s", t["nll_s"], want["nll_s"])
    _within("conf", t["conf"], want["conf"])
    _within("entropy of log pbar", t["entropy"], want["h"])
    _within("h_pred", t["h_pred"], want["h"])
    d_mi = np.abs(t["mi"].astype(np.float64) - want["mi"])
    print("mi: max |got - want| %.3e, min %.3e, mean %.3e" % (d_mi.max(), t["mi"].min(), want["mi"].mean()))
    assert (d_mi <= 1e-5 + 1e-4 * want["mi"]).all()
    _rel("loss", rep.loss, want["nll"].mean())
    for s in range(S):
        _rel("sample_loss[%d]" % s, rep.sample_loss[s], want["nll_s"][:, s].mean())
    _rel("sample_loss_mean", rep.sample_loss_mean, want["nll_s"].mean())
    _rel("mean_conf", rep.mean_conf, want["conf"].mean())
    _rel("mean_entropy", rep.mean_entropy, want["h"].mean())
    _rel("mean_h_pred", rep.mean_h_pred, want["h"].mean())
    _rel("mean_mi", rep.mean_mi, want["mi"].mean())
    # the host arithmetic on its own: float64 means of the per-token float32 arrays the report kept
    for name, got, arr in (("loss", rep.loss, t["nll"]), ("mean_mi", rep.mean_mi, t["mi"]), ("mean_h_pred", rep.mean_h_pred, t["h_pred"]),
                           ("mean_conf", rep.mean_conf, t["conf"]), ("mean_entropy", rep.mean_entropy, t["entropy"])):
        assert abs(got - arr.astype(np.float64).mean()) <= 1e-12 * abs(got), name
    assert rep.loss <= rep.sample_loss_mean + 1e-6  # Jensen
    assert rep.mean_mi >= -1e-6
    assert len(set(rep.sample_loss)) == S  # S different models: a repeated sample index would repeat a value
    # ties
    keep = want["gap"] >= 1e-4
    print("%s: %.3f %% of the tokens have a top-two gap under 1e-4 (cap 1 %%), %.3f %% under 1e-3; raw mismatches pred %d rank %d of %d"
          % (kind, 100 * (1 - keep.mean()), 100 * (want["gap"] < 1e-3).mean(), int((t["pred"] != want["pred"]).sum()),
             int((t["rank"] != want["rank"]).sum()), n))
    assert 1 - keep.mean() <= 0.01
    assert (t["pred"][keep] == want["pred"][keep]).all()
    clear = keep & (want["tgap"] >= 1e-4)
    print("%.2f %% of the targets have another word within 1e-4 (cap 20 %%)" % (100 * (want["tgap"] < 1e-4).mean()))
    assert (want["tgap"] < 1e-4).mean() <= 0.20
    assert (t["rank"][clear] == want["rank"][clear]).all()
    assert ((want["rank_lo"] <= t["rank"]) & (t["rank"] <= want["rank_hi"])).all()
    assert ((t["rank"] == 0) == (want["rank"] == 0))[keep].all()
    got_k = engine.report_from_tokens(t["nll"][keep], t["conf"][keep], t["entropy"][keep], t["rank"][keep], bins=15)
    ref_k = engine.report_from_tokens(want["nll"][keep], want["conf"][keep], want["h"][keep], want["rank"][keep], bins=15)
    assert got_k.accuracy == ref_k.accuracy
    print("ece: got %.6g want %.6g; accuracy %.4f" % (got_k.ece, ref_k.ece, got_k.accuracy))
    assert abs(got_k.ece - ref_k.ece) <= 2e-5
    straddle = ((want["rank_lo"] < 5) & (want["rank_hi"] >= 5))[keep]
    print("top-5: got %.6f want %.6f, %d tokens straddle rank 5" % (got_k.top5_accuracy, ref_k.top5_accuracy, int(straddle.sum())))
    assert abs(got_k.top5_accuracy - ref_k.top5_accuracy) <= straddle.sum() / keep.sum() + 1e-12
    # calibration=False: the same figures without the (rows, V) matrix
    lean = engine.evaluate_report(m, src, SEQ, mc_samples=S, calibration=False)
    assert lean.accuracy is None and lean.ece is None and lean.bins is None and lean.mean_conf is None
    for name, g, w in [("loss", lean.loss, rep.loss), ("mean_h_pred", lean.mean_h_pred, rep.mean_h_pred)] + [
            ("sample_loss[%d]" % s, lean.sample_loss[s], rep.sample_loss[s]) for s in range(S)]:
        assert abs(g - w) <= 2e-5 * max(1.0, abs(w)), (name, g, w)
    assert abs(lean.mean_mi - rep.mean_mi) <= 1e-5 + 1e-4 * rep.mean_mi


def test_identical_samples_and_state(dev, text):
    """log sigma -40: S identical samples -- no mutual information, and the average is the single sample, which is the mean-weight
    model.  The model comes back in eval mode with the caller's (seed, step, auto_step)."""
    from bayeslms_amd import engine
    m, src = _model("tlm_ffn", dev, lgstd=-40.0), _source(text, "tlm_ffn", dev)
    ns = m.noise_state
    ns.seed, ns.step, ns.auto_step = 5, 9, True
    rep = engine.evaluate_report(m, src, SEQ, mc_samples=S, seed=77)
    assert not m.training and (ns.seed, ns.step, ns.auto_step) == (5, 9, True) and not ns.dropout_off
    print("mean_mi %.3e loss %.9f sample_loss %s" % (rep.mean_mi, rep.loss, rep.sample_loss))
    assert abs(rep.mean_mi) <= 1e-6
    for v in rep.sample_loss:  # two means of per-token float32 values that agree to rounding: the 2e-5 relative bar of `loss`
        assert abs(rep.loss - v) <= 2e-5 * v
    assert abs(rep.loss - engine.evaluate(m, src, SEQ)) <= 2e-5 * rep.loss
    assert (ns.seed, ns.step, ns.auto_step) == (5, 9, True)


def test_refusals_name_the_cause_and_leave_the_model_in_eval_mode(dev, text):
    from bayeslms_amd import engine
    src = _source(text, "tlm", dev)
    cases = [("lstm_variational", 4, "time step", _source(text, "lstm", dev)), ("tlm_plain", 2, "no variational tensor", src),
             ("tlm_ffn", 1, "mc_samples", src), ("tlm_ffn", 65, "mc_samples", src)]
    for kind, s, msg, source in cases:
        m = _model(kind, dev)
        ns = m.noise_state
        ns.seed, ns.step, ns.auto_step = 3, 4, True
        with pytest.raises(BayesLMError, match=msg):
            engine.evaluate_report(m, source, SEQ, mc_samples=s)
        assert not m.training and (ns.seed, ns.step, ns.auto_step) == (3, 4, True) and not ns.dropout_off, kind
        assert not m.decoder._scope and not m.decoder.return_input
    m = _model("tlm_ffn", dev)
    m.set_local_reparam(True)
    with pytest.raises(BayesLMError, match="local_reparam"):
        engine.evaluate_report(m, src, SEQ, mc_samples=4)
    assert not m.training and not m.decoder._scope
    assert engine.evaluate_report(m, src, SEQ).tokens == (src.shape[0] - 1) * src.shape[1]  # mean weights: nothing is sampled, nothing refused


def test_two_runs_give_equal_json(dev, text):
    """Bit-equal reports need bit-equal forwards, which the library promises in deterministic mode (an under-filled GEMM
    otherwise sums its K slices with float atomics); blm_row_stats and the host sums are fixed-order in every mode.  In the
    default mode what does hold is asserted: the same tokens, and losses within 2e-6, the bar for reordered float32 sums that
    test_evaluate_batches_the_windows_of_a_stateless_model uses."""
    from bayeslms_amd import engine, ops
    m, src = _model("tlm_ffn", dev), _source(text, "tlm_ffn", dev)
    for s in (0, S):
        a, b = (engine.evaluate_report(m, src, SEQ, mc_samples=s).as_dict() for _ in range(2))
        print("default mode, S = %d: equal JSON %s, |loss difference| %.3e" % (s, json.dumps(a) == json.dumps(b), abs(a["loss"] - b["loss"])))
        assert (a["tokens"], a["skipped"], a["mc_samples"]) == (b["tokens"], b["skipped"], b["mc_samples"])
        assert sum(x[0] for x in a["bins"]) == sum(x[0] for x in b["bins"]) == a["tokens"]
        assert abs(a["loss"] - b["loss"]) <= 2e-6 and abs(a["ece"] - b["ece"]) <= 2e-5 and abs(a["accuracy"] - b["accuracy"]) <= 0.01
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        for s in (0, S):
            a, b = (json.dumps(engine.evaluate_report(m, src, SEQ, mc_samples=s).as_dict()) for _ in range(2))
            assert a == b and json.loads(a)["tokens"] > 0
    finally:
        ops.set_deterministic(was)


# ------------------------------------------------------------------------------------------------------------ command lines
def _write_text(path, ids, words):
    """ids with 0 = <s> closing a sentence -> one sentence per line"""
    lines, cur = [], []
    for i in ids:
        if i == 0:
            lines.append(" ".join(cur))
            cur = []
        else:
            cur.append(words[i])
    if cur:
        lines.append(" ".join(cur))
    path.write_text("\n".join(lines) + "\n")
    return sum(len(ln.split()) + 1 for ln in lines)  # Corpus.tokenize closes every line with <s>


def test_evaluate_cli(dev, text, tmp_path, capsys):
    from bayeslms_amd import evaluate as E
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(2, V)]
    m = _model("tlm_ffn", dev)
    torch.save({k: v.detach().cpu() for k, v in m.state_dict().items()}, str(tmp_path / "model.pt"))
    (tmp_path / "words.txt").write_text("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    n_text = _write_text(tmp_path / "test.txt", text.tolist(), words)
    common = ["--model-path", str(tmp_path / "model.pt"), "--vocabulary", str(tmp_path / "words.txt"), "--data", str(tmp_path / "test.txt"),
              "--model", "Transformer", "--emsize", "64", "--nhid", "128", "--nlayers", "2", "--nhead", "2", "--uncertainty", "Bayesian",
              "--T_bayes_pos", "FFN", "--seq-len", "16"]
    for extra, fields in ((["--batch-size", "1", "--mc-samples", "4", "--mc-seed", "3"], 7), (["--batch-size", "1"], 5)):
        rp, tp = tmp_path / "report.json", tmp_path / "tokens.txt"
        E.main(common + extra + ["--write-report", str(rp), "--write-tokens", str(tp)])
        line = capsys.readouterr().out.strip().splitlines()
        assert len(line) == 1 and line[0].startswith("| evaluate | tokens ")
        rep = json.loads(rp.read_text())
        assert rep["tokens"] + rep["skipped"] == n_text - 1  # one column: every word but the first is predicted
        assert rep["mc_samples"] == (4 if fields == 7 else 0) and len(rep["bins"]) == 15
        assert ("loss %.4f" % rep["loss"]) in line[0]
        rows = tp.read_text().splitlines()
        assert len(rows) == rep["tokens"] and all(len(r.split()) == fields for r in rows)
        assert [r.split()[0] for r in rows[:50]] == [words[i] for i in E.D.Corpus.tokenize(_Vocab(words), str(tmp_path / "test.txt"))[1:51].tolist()]
        assert abs(np.mean([float(r.split()[1]) for r in rows]) - rep["loss"]) <= 1e-5 * rep["loss"]  # %.6g per token
    E.main(common + ["--write-report", str(rp)])  # the default 10 columns: the layout of train.py's test pass
    rep = json.loads(rp.read_text())
    assert rep["tokens"] == (n_text // 10 - 1) * 10 and rep["skipped"] == 0


class _Vocab:
    """What Corpus.tokenize reads of a Corpus: the dictionary."""

    def __init__(self, words):
        from bayeslms_amd import data as D
        self.dictionary = D.Dictionary()
        self.dictionary.idx2word = list(words)
        self.dictionary.word2idx = {w: i for i, w in enumerate(words)}


def test_train_cli_writes_the_test_report(dev, tmp_path, capsys):
    """--test-report after the final test pass: the JSON's loss is the test loss train.py printed, to the printed digits; with
    --test-mc-samples the same file holds the Monte-Carlo block."""
    from bayeslms_amd import data as D, train as T
    nv = 60
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(2, nv)]
    (tmp_path / "words.txt").write_text("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    for name, n, seed in (("train", 1500, 1), ("valid", 700, 2), ("test", 900, 3)):
        _write_text(tmp_path / (name + ".txt"), D.synthetic_corpus(nv, n, seed=seed).tolist(), words)
    common = ["--data", str(tmp_path), "--model", "Transformer", "--emsize", "32", "--nhid", "64", "--nlayers", "2", "--nhead", "2",
              "--uncertainty", "Bayesian", "--T_bayes_pos", "FFN", "--tied", "--cuda", "--batch-size", "8", "--seq_len", "16",
              "--save", str(tmp_path / "model.pt"), "--log-interval", "1000"]
    rp = tmp_path / "report.json"
    T.main(common + ["--epochs", "1", "--test-report", str(rp)])
    printed = re.search(r"End of training \| test loss\s+([0-9.]+) \|", capsys.readouterr().out).group(1)
    rep = json.loads(rp.read_text())
    print("printed %s, report %.9f" % (printed, rep["loss"]))
    assert "%.2f" % rep["loss"] == printed and rep["mc_samples"] == 0 and rep["sample_loss"] is None
    T.main(common + ["--epochs", "0", "--test-report", str(rp), "--test-mc-samples", "4"])  # the saved model, reloaded
    mc = json.loads(rp.read_text())
    assert mc["mc_samples"] == 4 and len(mc["sample_loss"]) == 4 and mc["tokens"] == rep["tokens"]
    assert mc["loss"] <= mc["sample_loss_mean"] + 1e-6 and mc["mean_mi"] >= -1e-6
    assert abs(mc["loss"] - rep["loss"]) < 0.5  # the same model, sampled around its mean
    os.remove(str(rp))
    T.main(common + ["--epochs", "0"])  # no flag: nothing new runs
    assert not rp.exists()
