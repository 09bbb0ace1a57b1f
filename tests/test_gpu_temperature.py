"""GPU: temperature scaling in the engine and on the command line -- engine.evaluate_temperatures and
evaluate_report(temperature=...) against float64 of materialised logits (of log pbar under Monte-Carlo), engine.fit_temperature
against the float64 minimiser over the same logits, and python -m bayeslms_amd.evaluate with the two flags.

The tiny models, the synthetic text and the layouts are those of tests/test_gpu_eval_report.py."""
import json
import math

import numpy as np
import pytest
import torch

from bayeslms_amd import BayesLMError
from test_gpu_eval_report import SEQ, S, V, _Vocab, _model, _source, _write_text  # noqa: F401  (helpers, no tests)

pytestmark = pytest.mark.gpu

BETAS = [0.5, 1.0, 2.0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def text():
    from bayeslms_amd import data as D
    return D.synthetic_corpus(V, 3000, seed=7)


@pytest.fixture
def deterministic():
    """Bit-equal forwards from one walk to the next (see test_gpu_eval_report.test_two_runs_give_equal_json)."""
    from bayeslms_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(was)


def _rows64(m, src, mc):
    """Window by window, logits materialised -> (tokens, V) float64 rows (logits at mean weights, log pbar of ``mc`` forwards
    under model.mc_sampling otherwise) and the targets.  Token order is the walk's, which no mean depends on."""
    from bayeslms_amd import model as M
    from bayeslms_amd.data import get_batch
    rows, cols = src.shape
    recurrent = hasattr(m, "init_hidden")
    xs, ts = [], []

    def walk(n):
        hidden = [m.init_hidden(cols) for _ in range(n)] if recurrent else None
        for i in range(0, rows - 1, SEQ):
            data, tgt = get_batch(src, i, SEQ)
            lp = []
            for s in range(n):
                if mc:
                    m.set_step(s)
                if recurrent:
                    y, h = m(data, hidden[s])
                    hidden[s] = M.repackage_hidden(h)
                else:
                    y = m(data)
                lp.append(y.reshape(-1, V).double())
            if mc:
                lp = torch.stack([torch.log_softmax(v, -1) for v in lp])
                xs.append(torch.logsumexp(lp, 0) - math.log(mc))
            else:
                xs.append(lp[0])
            ts.append(tgt)

    with torch.no_grad():
        if mc:
            with M.mc_sampling(m, 1111, mc):
                walk(mc)
        else:
            walk(1)
    return torch.cat(xs), torch.cat(ts)


def _figures64(x, t, beta):
    """per token, float64, under p ~ exp(beta x): nll, conf, entropy, slope of the nll in beta, hit"""
    z = beta * x
    lse = torch.logsumexp(z, -1)
    p = torch.softmax(z, -1)
    xt = x.gather(1, t.view(-1, 1)).squeeze(1)
    top2 = x.topk(2, -1).values
    return {"nll": lse - beta * xt, "conf": (z.max(-1).values - lse).exp(), "entropy": lse - (p * z).sum(-1),
            "dnll": (p * x).sum(-1) - xt, "hit": (x.max(-1).values == xt), "gap": top2[:, 0] - top2[:, 1]}


def _rel(name, got, want, rel=2e-5):
    print("%s: got %.9g want %.9g" % (name, got, want))
    assert abs(got - want) <= rel * abs(want), (name, got, want)


@pytest.mark.parametrize("kind,mc", [("tlm_plain", 0), ("tlm_ffn", S), ("lstm_bayes3", 0)])
def test_evaluate_temperatures_equals_float64_of_the_logits(dev, text, deterministic, kind, mc):
    """loss, mean_conf, mean_entropy and the mean slope 2e-5 relative.  ece and bins depend on which bin a confidence falls
    into and on whether the target is the prediction; a token whose float64 top-two gap is under 1e-4 or whose float64
    confidence lies within 1e-5 of a bin edge may land either way in float32, and one token that changes bin or outcome moves
    the ece by at most 2 / n and two bin counts by one each.  With k such tokens (capped at 1 %): |ece - want| <= 2e-5 + 2 k / n
    and sum |count - want| <= 2 k."""
    from bayeslms_amd import engine
    m, src = _model(kind, dev), _source(text, kind, dev)
    n = (src.shape[0] - 1) * src.shape[1]
    reps, dloss = engine.evaluate_temperatures(m, src, SEQ, BETAS, mc_samples=mc)
    plain = engine.evaluate_report(m, src, SEQ, mc_samples=mc)
    x, t = _rows64(m, src, mc)
    assert x.shape == (n, V) and len(reps) == len(dloss) == 3
    for b, rep, dl in zip(BETAS, reps, dloss):
        w = _figures64(x, t, b)
        name = "%s beta %g" % (kind, b)
        assert (rep.tokens, rep.skipped, rep.mc_samples) == (n, 0, mc) and rep.ppl == math.exp(rep.loss)
        _rel(name + " loss", rep.loss, float(w["nll"].mean()))
        _rel(name + " mean_conf", rep.mean_conf, float(w["conf"].mean()))
        _rel(name + " mean_entropy", rep.mean_entropy, float(w["entropy"].mean()))
        want_d = float(w["dnll"].mean())
        print("%s dloss: got %.9g want %.9g" % (name, dl, want_d))
        assert abs(dl - want_d) <= 2e-5 * max(1.0, abs(want_d))
        # what does not depend on the temperature
        assert (rep.accuracy, rep.top5_accuracy) == (plain.accuracy, plain.top5_accuracy)
        assert (rep.sample_loss, rep.mean_h_pred, rep.mean_mi) == (plain.sample_loss, plain.mean_h_pred, plain.mean_mi)
        assert rep.temperature["beta"] == b and rep.temperature["temperature"] == 1 / b and rep.temperature["fitted_on"] is None
        # calibration
        conf, hit = w["conf"].cpu().numpy(), w["hit"].cpu().numpy()
        edge = np.abs(conf * 15 - np.round(conf * 15)) <= 15 * 1e-5
        k = int((edge | (w["gap"].cpu().numpy() < 1e-4)).sum())
        want = engine.report_from_tokens(w["nll"].cpu().numpy(), conf, w["entropy"].cpu().numpy(), np.where(hit, 0, 1), bins=15)
        print("%s: ece got %.6g want %.6g, %d of %d tokens near a bin edge or a tie" % (name, rep.ece, want.ece, k, n))
        assert k <= 0.01 * n and len(rep.bins) == 15
        assert abs(rep.ece - want.ece) <= 2e-5 + 2.0 * k / n
        assert sum(abs(g[0] - r[0]) for g, r in zip(rep.bins, want.bins)) <= 2 * k and sum(g[0] for g in rep.bins) == n
        if k == 0:
            for g, r in zip(rep.bins, want.bins):
                assert g[0] == r[0] and abs(g[1] - r[1]) <= 2e-5 and abs(g[2] - r[2]) <= 1e-12
    # a sharper distribution is more confident and has less entropy; the slope rises with beta (the NLL is convex)
    assert reps[0].mean_conf < reps[1].mean_conf < reps[2].mean_conf and reps[0].mean_entropy > reps[1].mean_entropy > reps[2].mean_entropy
    assert dloss[0] < dloss[1] < dloss[2]
    # beta = 1 is the untempered report, within the kernel's bar
    for f in ("loss", "mean_conf", "mean_entropy"):
        _rel("%s beta 1 %s against evaluate_report" % (kind, f), getattr(reps[1], f), getattr(plain, f))
    # evaluate_report(temperature=2) is the beta = 0.5 entry, field for field
    two = engine.evaluate_report(m, src, SEQ, mc_samples=mc, temperature=2.0)
    assert two.as_dict() == reps[0].as_dict() and two.temperature["beta"] == 0.5


def test_temperature_one_launches_what_it_launched(dev, text, deterministic, monkeypatch):
    from bayeslms_amd import engine, ops
    m, src = _model("tlm_ffn", dev), _source(text, "tlm_ffn", dev)

    def never(*a, **k):
        raise AssertionError("ops.row_stats_temps called at temperature 1")
    with monkeypatch.context() as mp:
        mp.setattr(ops, "row_stats_temps", never)
        for s in (0, S):
            one = engine.evaluate_report(m, src, SEQ, mc_samples=s, temperature=1.0, keep_tokens=True)
            ref = engine.evaluate_report(m, src, SEQ, mc_samples=s, keep_tokens=True)
            assert one.as_dict() == ref.as_dict() and "temperature" not in one.as_dict()
            assert sorted(one.per_token) == sorted(ref.per_token) and "dnll" not in one.per_token
        with pytest.raises(AssertionError, match="row_stats_temps called"):
            engine.evaluate_report(m, src, SEQ, temperature=1.5)
    # the tempered per-token figures are the report's
    rep = engine.evaluate_report(m, src, SEQ, mc_samples=S, temperature=1.5, keep_tokens=True)
    t = rep.per_token
    assert t["nll"].shape == t["conf"].shape == t["mi"].shape == (rep.tokens,) and t["nll_s"].shape == (rep.tokens, S)
    assert abs(rep.loss - t["nll"].astype(np.float64).mean()) <= 1e-12 * rep.loss
    assert t["tgt"].tolist() == src[1:].t().reshape(-1).tolist()


def test_refusals(dev, text):
    from bayeslms_amd import engine
    m, src = _model("tlm_ffn", dev), _source(text, "tlm_ffn", dev)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60, "x"):
        with pytest.raises(BayesLMError, match="temperature"):
            engine.evaluate_report(m, src, SEQ, temperature=bad)
    with pytest.raises(BayesLMError, match="calibration=False"):
        engine.evaluate_report(m, src, SEQ, mc_samples=S, calibration=False, temperature=2.0)
    assert engine.evaluate_report(m, src, SEQ, mc_samples=S, calibration=False, temperature=1.0).ece is None
    for bad, msg in (([], "0 inverse"), ([1.0] * 9, "9 inverse"), ([1.0, 0.0], r"betas\[1\]"), ([float("nan")], r"betas\[0\]"), (3, "3")):
        with pytest.raises(BayesLMError, match=msg):
            engine.evaluate_temperatures(m, src, SEQ, bad)
    with pytest.raises(BayesLMError, match="mc_samples"):
        engine.evaluate_temperatures(m, src, SEQ, [1.0], mc_samples=1)
    with pytest.raises(BayesLMError, match="mc_samples"):
        engine.fit_temperature(m, src, SEQ, mc_samples=65)
    with pytest.raises(BayesLMError, match="passes"):
        engine.fit_temperature(m, src, SEQ, passes=0)
    with pytest.raises(BayesLMError, match="no variational tensor"):
        engine.fit_temperature(_model("tlm_plain", dev), src, SEQ, mc_samples=2)
    assert not m.training and not m.decoder._scope and not m.decoder.return_input


def _sampled_text(m, dev, n, temperature, seed):
    """n tokens the model itself generates at a sampling temperature: one stream through IncrementalLM.step"""
    from bayeslms_amd.incremental import IncrementalLM
    lm = IncrementalLM(m, max_streams=1, max_len=n + 1)
    st = lm.start(1)
    g = torch.Generator(device=dev).manual_seed(seed)
    ids = [0]
    for _ in range(n - 1):
        logp = lm.step(st, torch.tensor([ids[-1]], device=dev))
        ids.append(int(torch.multinomial(torch.softmax(logp.double() / temperature, -1), 1, generator=g)))
    return torch.tensor(ids, dtype=torch.int64)


def test_fit_finds_the_float64_minimiser(dev, text, deterministic):
    """A text the model generated at sampling temperature 2 is best explained near beta = 0.5: an interior optimum (a random
    model on unrelated text has beta* -> 0 and would test the bound alone).  beta within 1e-3 relative of the float64 minimiser
    over the same walk's logits: three passes of eight leave a bracket of ratio 1.0122, the secant lands well inside."""
    from bayeslms_amd import data as D, engine
    m = _model("lstm_bayes3", dev)
    src = D.batchify(_sampled_text(m, dev, 600, 2.0, seed=5), 1, dev)
    fit = engine.fit_temperature(m, src, SEQ)
    x, t = _rows64(m, src, 0)
    xt = x.gather(1, t.view(-1, 1)).squeeze(1)

    def slope(b):
        return float(((torch.softmax(b * x, -1) * x).sum(-1) - xt).mean())
    lo, hi = 1e-3, 1e3
    assert slope(lo) < 0 < slope(hi)
    for _ in range(100):
        mid = math.sqrt(lo * hi)
        lo, hi = (mid, hi) if slope(mid) < 0 else (lo, mid)
    star = math.sqrt(lo * hi)
    print("beta* %.9f fitted %.9f (relative %.3e), passes %d, loss %.6f -> %.6f, ece %.4f -> %.4f"
          % (star, fit.beta, fit.beta / star - 1, fit.passes, fit.before.loss, fit.after.loss, fit.before.ece, fit.after.ece))
    assert 0.3 < star < 0.8
    assert abs(fit.beta / star - 1) <= 1e-3
    assert not fit.at_bound and fit.passes == 3 and fit.temperature == 1.0 / fit.beta and fit.beta == float(np.float32(fit.beta))
    assert fit.after.loss <= fit.before.loss
    assert len(fit.curve) == 3 * 8 + 2 and all(len(c) == 4 for c in fit.curve)
    assert fit.curve[-2][0] == 1.0 and fit.curve[-1][:2] == [fit.beta, fit.after.loss] and fit.curve[-2][1] == fit.before.loss
    assert all(fit.after.loss <= c[1] + 1e-6 for c in fit.curve)  # no evaluated beta does better (1e-6: float32 per-token NLLs)
    # before is the untempered report (through the other kernel: floats within the bar, counts equal)
    ref = engine.evaluate_report(m, src, SEQ)
    for f in ("loss", "mean_conf", "mean_entropy"):
        _rel("before." + f, getattr(fit.before, f), getattr(ref, f))
    assert (fit.before.tokens, fit.before.accuracy, fit.before.top5_accuracy) == (ref.tokens, ref.accuracy, ref.top5_accuracy)
    assert abs(fit.before.ece - ref.ece) <= 2e-5 + 2.0 / ref.tokens  # at most a token on a bin edge
    # after is evaluate_report at the fitted temperature, field for field
    assert engine.evaluate_report(m, src, SEQ, temperature=fit.temperature).as_dict() == fit.after.as_dict()
    # the same model knows nothing of the synthetic text: the loss falls all the way to the bound
    flat = engine.fit_temperature(m, _source(text, "lstm_bayes3", dev), SEQ)
    print("synthetic text: beta %.6f at_bound %s passes %d" % (flat.beta, flat.at_bound, flat.passes))
    assert flat.at_bound and flat.beta == 1.0 / 16 and flat.passes <= 3 and flat.after.loss <= flat.before.loss


def test_evaluate_cli_with_a_temperature(dev, text, tmp_path, capsys, deterministic):
    from bayeslms_amd import data as D, engine, evaluate as E
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(2, V)]
    m = _model("tlm_ffn", dev)
    torch.save({k: v.detach().cpu() for k, v in m.state_dict().items()}, str(tmp_path / "model.pt"))
    (tmp_path / "words.txt").write_text("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    _write_text(tmp_path / "test.txt", text.tolist(), words)
    _write_text(tmp_path / "valid.txt", D.synthetic_corpus(V, 1500, seed=8).tolist(), words)
    common = ["--model-path", str(tmp_path / "model.pt"), "--vocabulary", str(tmp_path / "words.txt"), "--data", str(tmp_path / "test.txt"),
              "--model", "Transformer", "--emsize", "64", "--nhid", "128", "--nlayers", "2", "--nhead", "2", "--uncertainty", "Bayesian",
              "--T_bayes_pos", "FFN", "--seq-len", "16"]
    rp, tp = tmp_path / "report.json", tmp_path / "tokens.txt"
    tok = E.D.Corpus.tokenize(_Vocab(words), str(tmp_path / "test.txt"))
    src = D.batchify(tok, 10, dev)

    def run(extra):
        E.main(common + extra + ["--write-report", str(rp)])
        out = capsys.readouterr()
        line = out.out.strip().splitlines()
        assert len(line) == 1 and line[0].startswith("| evaluate | tokens ")
        return json.loads(rp.read_text()), line[0], out.err

    block = ["at_bound", "beta", "curve", "ece_after", "ece_before", "fitted_on", "loss_after", "loss_before", "temperature"]
    # no flag: the JSON and the line of before
    rep, line, err = run([])
    assert "temperature" not in rep and "temperature" not in line and err == ""
    assert rep == json.loads(json.dumps(engine.evaluate_report(m, src, SEQ).as_dict()))
    # --temperature
    rep, line, err = run(["--temperature", "1.5"])
    want = engine.evaluate_report(m, src, SEQ, temperature=1.5)
    assert rep == json.loads(json.dumps(want.as_dict())) and sorted(rep["temperature"]) == block
    assert rep["temperature"]["temperature"] == 1.0 / float(np.float32(1 / 1.5)) and rep["temperature"]["fitted_on"] is None
    assert line.endswith("| temperature 1.5000") and ("loss %.4f" % rep["loss"]) in line and err == ""
    # --fit-temperature-on, with Monte-Carlo samples and the per-token file
    extra = ["--fit-temperature-on", str(tmp_path / "valid.txt"), "--mc-samples", "4", "--write-tokens", str(tp)]
    rep, line, err = run(extra)
    t = rep["temperature"]
    assert sorted(t) == block and t["fitted_on"] == str(tmp_path / "valid.txt") and t["temperature"] == 1.0 / t["beta"]
    assert len(t["curve"]) >= 8 + 2 and t["loss_after"] <= t["loss_before"]
    assert ("warning" in err) == t["at_bound"]
    assert "| temperature %.4f | fit loss %.4f -> %.4f | ece %.4f -> %.4f" % (
        t["temperature"], t["loss_before"], t["loss_after"], t["ece_before"], t["ece_after"]) in line
    want = engine.evaluate_report(m, src, SEQ, mc_samples=4, temperature=t["temperature"]).as_dict()
    assert {k: v for k, v in rep.items() if k != "temperature"} == {k: v for k, v in json.loads(json.dumps(want)).items() if k != "temperature"}
    assert want["temperature"]["beta"] == t["beta"]
    rows = tp.read_text().splitlines()  # the tempered nll: its mean is the report's loss
    assert len(rows) == rep["tokens"] and all(len(r.split()) == 7 for r in rows)
    assert abs(np.mean([float(r.split()[1]) for r in rows]) - rep["loss"]) <= 1e-5 * rep["loss"]
    again, _, _ = run(extra)
    assert again == rep
