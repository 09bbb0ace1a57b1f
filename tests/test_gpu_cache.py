"""GPU: the continuous neural cache -- blm_cache_scores (ops.cache_scores) against the float64 dense reference of
tests/cache_reference.py, then engine.evaluate_cache / fit_cache and the evaluate command on small models.

Kernel inputs: rows drawn as N(0, 1) * 2 / K^(1/4), so a raw score q.k has a standard deviation of about 4 whatever K is (the
regime of _inputs in tests/test_gpu_mc_uncertainty.py); theta <= 1 for K >= 512, <= 2 below.  Finite outputs must lie within
2e-5 * max(1, |want|) of the reference -- the project's bound for log-sums over fp32 logits -- and the two must agree exactly on
which entries are -inf.

Measured on the MI355X (max |got - want| / max(1, |want|) over lse and match, all eight thetas): see
profiles/r16_cache_probe.txt."""
import json
import math

import numpy as np
import pytest
import torch

import cache_reference as R

pytestmark = pytest.mark.gpu

BOUND = 2e-5
# (n, K, window, label vocabulary)
CASES = [(127, 64, 50, 8), (128, 64, 50, 8), (129, 64, 50, 8),   # tile edges
         (300, 33, 17, 8),                                       # guarded K
         (70, 20, 500, 5),                                       # window longer than the text
         (200, 64, 1, 4),                                        # window of 1
         (1500, 512, 500, 50), (1500, 1024, 1000, 200),          # long K
         (400, 130, 64, 10 ** 6)]                                # almost no matches: -inf must agree exactly
THETAS_LONG_K = [0.0, 0.05, 0.1, 0.2, 0.35, 0.5, 0.75, 1.0]
THETAS_SHORT_K = [0.0, 0.1, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0]
V, H = 97, 96


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def deterministic():
    """Bit-equal forwards from one walk of a text to the next."""
    from bayeslms_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(was)


def _thetas(K):
    return [float(np.float32(t)) for t in (THETAS_LONG_K if K >= 512 else THETAS_SHORT_K)]


def _rows(n, K, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, K, generator=g) * (2.0 / K ** 0.25)).to(dev)


_CASE = {}


def _case(case, dev):
    """inputs and the float64 reference at the case's eight thetas: made once, shared, never written"""
    if case not in _CASE:
        n, K, window, vocab = case
        h = _rows(n, K, 100 + CASES.index(case), dev)
        g = torch.Generator().manual_seed(7)
        y = torch.randint(0, vocab, (n,), generator=g).to(dev)
        hi = torch.arange(n, device=dev, dtype=torch.int32)
        lse, match = R.cache_scores(h, h, y, y, hi, _thetas(K), window)
        _CASE[case] = (h, y, hi, lse, match)
    return _CASE[case]


def _compare(name, got, want, bound=BOUND):
    """every entry is compared: the same -inf pattern, finite ones within the bound -> the largest scaled error"""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert not torch.isnan(got).any(), name
    ginf, winf = torch.isneginf(got), torch.isneginf(want)
    assert torch.equal(ginf, winf), "%s: -inf at %d entries, the reference at %d" % (name, int(ginf.sum()), int(winf.sum()))
    assert torch.isfinite(got[~ginf]).all(), name
    if bool(ginf.all()):
        return 0.0
    err = float(((got - want).abs() / want.abs().clamp(min=1.0))[~ginf].max())
    print("%s: max scaled error %.3g, %d of %d entries -inf" % (name, err, int(ginf.sum()), got.numel()))
    assert err <= bound, (name, err)
    return err


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("J", [1, 2, 8])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_K%d_N%d_V%d" % c)
def test_kernel_equals_float64_reference(dev, case, J):
    from bayeslms_amd import ops
    n, K, window, _ = case
    h, y, hi, lse, match = _case(case, dev)
    pick = {1: [4], 2: [0, 7], 8: list(range(8))}[J]  # theta = 0 is in the lists of two and eight
    thetas = [_thetas(K)[j] for j in pick]
    got = ops.cache_scores(h, h, y, y, hi, thetas, window)
    assert got.lse.shape == got.match.shape == (J, n) and got.lse.dtype == torch.float32
    _compare("lse %s J %d" % (case, J), got.lse, lse[pick])
    _compare("match %s J %d" % (case, J), got.match, match[pick])
    assert bool(torch.isneginf(got.lse[:, 0]).all()) and bool(torch.isfinite(got.lse[:, 1:]).all())  # only the first cache is empty
    if 0 in pick:  # theta = 0: the size of the window, exactly that of the reference up to the bound
        size = torch.minimum(torch.arange(n, device=dev), torch.tensor(window, device=dev)).double()
        assert float((got.lse[0, 1:].double().exp() - size[1:]).abs().max()) <= 2e-5 * window


def test_separate_queries_and_keys_share_one_range(dev):
    """the scorer's case: other queries than keys, one range for all of them; operands that are views of wider, offset buffers
    (row stride > K, base 4 bytes past a 16-byte boundary: the guarded loads)"""
    from bayeslms_amd import ops
    M, Nk, K = 200, 333, 48
    qbuf, kbuf = _rows(M, K + 5, 1, dev), _rows(Nk, K + 3, 2, dev)
    q, k = qbuf[:, 1:1 + K], kbuf[:, 1:1 + K]
    g = torch.Generator().manual_seed(3)
    labels, targets = torch.randint(0, 6, (Nk,), generator=g).to(dev), torch.randint(0, 6, (M,), generator=g).to(dev)
    thetas = _thetas(K)[:4]
    # the last one: hi past the keys with a short window starts at 995, beyond the 333 keys -- an empty range by the definition
    for lo_v, hi_v, window in ((20, 300, 1000), (20, 300, 100), (0, 333, 333), (0, 340, 12), (0, 1000, 5)):
        lo = torch.full((M,), lo_v, dtype=torch.int32, device=dev)
        hi = torch.full((M,), hi_v, dtype=torch.int32, device=dev)
        got = ops.cache_scores(q, k, labels, targets, hi, thetas, window, lo=lo)
        want = R.cache_scores(q, k, labels, targets, hi, thetas, window, lo=lo)
        _compare("shared range lse %s" % ((lo_v, hi_v, window),), got.lse, want[0])
        _compare("shared range match %s" % ((lo_v, hi_v, window),), got.match, want[1])
        assert bool(torch.isneginf(got.lse).all() if hi_v == 1000 else torch.isfinite(got.lse).all())
        same = ops.cache_scores(q.contiguous(), k.contiguous(), labels, targets, hi, thetas, window, lo=lo)
        assert torch.equal(same.lse, got.lse) and torch.equal(same.match, got.match)  # the layout changes no bit


def test_ranges_are_clamped_whatever_lo_and_hi_hold(dev):
    """non-monotone, empty, reversed and out-of-range lo / hi: -inf where the clamped range is empty, the reference elsewhere"""
    from bayeslms_amd import ops
    M, Nk, K, window = 300, 260, 40, 90
    q, k = _rows(M, K, 4, dev), _rows(Nk, K, 5, dev)
    g = torch.Generator().manual_seed(6)
    labels, targets = torch.randint(0, 5, (Nk,), generator=g).to(dev), torch.randint(0, 5, (M,), generator=g).to(dev)
    lo = torch.randint(-50, Nk + 50, (M,), generator=g, dtype=torch.int32)
    hi = torch.randint(-50, Nk + 200, (M,), generator=g, dtype=torch.int32)
    big, small = 2 ** 31 - 1, -2 ** 31
    lo[:10] = torch.tensor([small, small, big, 0, 100, 5, -1, big, small, 255], dtype=torch.int32)
    hi[:10] = torch.tensor([small, big, big, 0, 100, 4, small, small, Nk + 10, big], dtype=torch.int32)
    lo, hi = lo.to(dev), hi.to(dev)
    thetas = [0.0, 0.5]
    got = ops.cache_scores(q, k, labels, targets, hi, thetas, window, lo=lo)
    want = R.cache_scores(q, k, labels, targets, hi, thetas, window, lo=lo)
    _compare("clamped lse", got.lse, want[0])
    _compare("clamped match", got.match, want[1])
    start, end = R.key_ranges(hi, window, Nk, lo)
    empty = start >= end
    assert 20 <= int(empty.sum()) <= M - 20  # both kinds are there
    assert bool(torch.isneginf(got.lse[:, empty]).all()) and bool(torch.isneginf(got.match[:, empty]).all())
    assert bool(torch.isfinite(got.lse[:, ~empty]).all())
    # [min, min), [max - window, Nk), [max, Nk), ... are empty; [Nk + 10 - window, Nk) is not; [max - window, Nk) with lo below Nk is
    assert bool(empty[:8].all()) and not bool(empty[8]) and bool(empty[9])
    assert (int(start[8]), int(end[8])) == (Nk + 10 - window, Nk)
    # lo = None is lo = 0
    none = ops.cache_scores(q, k, labels, targets, hi, thetas, window)
    zero = ops.cache_scores(q, k, labels, targets, hi, thetas, window, lo=torch.zeros_like(hi))
    assert torch.equal(none.lse, zero.lse) and torch.equal(none.match, zero.match)
    want = R.cache_scores(q, k, labels, targets, hi, thetas, window)
    _compare("lo None lse", none.lse, want[0])
    _compare("lo None match", none.match, want[1])
    # no keys at all
    got = ops.cache_scores(q, k[:0], labels[:0], targets, hi, thetas, window)
    assert bool(torch.isneginf(got.lse).all()) and bool(torch.isneginf(got.match).all())


def test_eight_thetas_in_one_launch_equal_eight_launches(dev):
    from bayeslms_amd import ops
    for case in (CASES[2], CASES[6]):
        n, K, window, _ = case
        h, y, hi, _, _ = _case(case, dev)
        thetas = _thetas(K)
        all8 = ops.cache_scores(h, h, y, y, hi, thetas, window)
        for j, t in enumerate(thetas):
            one = ops.cache_scores(h, h, y, y, hi, [t], window)
            _compare("one launch lse theta %g" % t, all8.lse[j:j + 1], one.lse)
            _compare("one launch match theta %g" % t, all8.match[j:j + 1], one.match)


def test_two_runs_give_the_same_bits(dev):
    from bayeslms_amd import ops
    n, K, window, _ = CASES[6]
    h, y, hi, _, _ = _case(CASES[6], dev)
    was = ops.is_deterministic()
    try:
        for mode in (False, True):
            ops.set_deterministic(mode)
            a = ops.cache_scores(h, h, y, y, hi, _thetas(K), window)
            b = ops.cache_scores(h, h, y, y, hi, _thetas(K), window)
            assert torch.equal(a.lse, b.lse) and torch.equal(a.match, b.match), mode
            if mode:
                assert torch.equal(a.lse, first.lse) and torch.equal(a.match, first.match)  # the mode changes nothing here
            first = a
    finally:
        ops.set_deterministic(was)


def test_cache_distribution_is_normalised_on_the_device(dev):
    """eight labels, the target looped over all eight: sum_w exp(match_w - lse) = 1 wherever the cache is not empty"""
    from bayeslms_amd import ops
    n, K, window, vocab = CASES[2]
    h, y, hi, _, _ = _case(CASES[2], dev)
    thetas = _thetas(K)
    total = torch.zeros(len(thetas), n, dtype=torch.float64, device=dev)
    for w in range(vocab):
        got = ops.cache_scores(h, h, y, torch.full_like(y, w), hi, thetas, window)
        total += torch.where(torch.isneginf(got.match), torch.zeros_like(total), (got.match.double() - got.lse.double()).exp())
    print("normalisation: max |sum - 1| = %.3g" % float((total[:, 1:] - 1).abs().max()))
    assert bool((total[:, 0] == 0).all()) and float((total[:, 1:] - 1).abs().max()) <= 1e-5


def test_chunked_queries_give_the_same_bits(dev, monkeypatch):
    """the chunking over queries (operands past the 32-bit offset limit) with the chunk size brought down to the test's"""
    from bayeslms_amd import ops
    n, K, window, _ = CASES[3]
    h, y, hi, _, _ = _case(CASES[3], dev)
    whole = ops.cache_scores(h, h, y, y, hi, [0.0, 0.5, 1.0], window)
    monkeypatch.setattr(ops, "_row_chunks", lambda M, ld: [(0, 128), (128, 256), (256, M)])
    parts = ops.cache_scores(h, h, y, y, hi, [0.0, 0.5, 1.0], window)
    assert torch.equal(whole.lse, parts.lse) and torch.equal(whole.match, parts.match)


def test_ops_refusals(dev):
    from bayeslms_amd import ops
    h, y, hi, _, _ = _case(CASES[0], dev)
    with pytest.raises(ops.BayesLMError, match="inference-only"):
        ops.cache_scores(h.clone().requires_grad_(), h, y, y, hi, [0.1], 5)
    with pytest.raises(ops.BayesLMError, match="window"):
        ops.cache_scores(h, h, y, y, hi, [0.1], 0)
    with pytest.raises(ops.BayesLMError, match="thetas"):
        ops.cache_scores(h, h, y, y, hi, [-0.1], 5)
    with pytest.raises(ops.BayesLMError):
        ops.cache_scores(h, h[:, :32], y, y, hi, [0.1], 5)
    with pytest.raises(ops.BayesLMError):
        ops.cache_scores(h, h, y[:5], y, hi, [0.1], 5)
    with pytest.raises(ops.BayesLMError):
        ops.cache_scores(h, h, y, y, hi.long(), [0.1], 5)


# ------------------------------------------------------------------------------------------------------------ end to end
def _model(kind, dev):
    from bayeslms_amd import model as M
    torch.manual_seed(5)
    m = M.TransformerModel(V, 128, 2, 256, 2, 0.5, "gelu", True) if kind == "tlm" else M.RNNModel("LSTM", V, H, H, 2, 0.5, True)
    return m.to(dev).eval()


def _text(n=2000, seed=3):
    from bayeslms_amd import data as D
    return D.synthetic_corpus(V, n, seed=seed)


def _source(text, kind, seq_len, dev):
    from bayeslms_amd import data as D
    return D.batchify(text, {("tlm", 35): 4, ("tlm", 20): 7, ("lstm", 35): 6, ("lstm", 20): 3}[(kind, seq_len)], dev)


@pytest.mark.parametrize("kind,seq_len", [("tlm", 35), ("tlm", 20), ("lstm", 35), ("lstm", 20)])
def test_evaluate_cache_equals_the_reference_on_the_walks_rows(dev, deterministic, kind, seq_len):
    from bayeslms_amd import engine, ops
    from bayeslms_amd.model import inference_decoder
    m, src = _model(kind, dev), _source(_text(), kind, seq_len, dev)
    n = (src.shape[0] - 1) * src.shape[1]
    window, theta, lam = 150, (0.02 if kind == "tlm" else 2.0), 0.2
    plain = engine.evaluate_report(m, src, seq_len, keep_tokens=True)
    rep = engine.evaluate_cache(m, src, seq_len, window, theta, lam, keep_tokens=True)
    assert rep.base_loss == plain.loss and rep.base_ppl == plain.ppl and (rep.tokens, rep.skipped) == (n, 0)
    assert (rep.window, rep.theta, rep.lam) == (window, float(np.float32(theta)), lam) and rep.ppl == math.exp(rep.loss)
    t = rep.per_token
    assert t["tgt"].tolist() == src[1:].t().reshape(-1).tolist()  # text order: a column is a contiguous stretch of the text
    assert np.array_equal(t["nll_model"], plain.per_token["nll"])
    # the rows of the same walk, in text order: they are the decoder's inputs of these targets ...
    walk = engine._cache_walk("test", m, src, seq_len)
    dec = inference_decoder(m)
    logits = walk["rows"].double() @ dec.weight.double().t()
    logp = torch.log_softmax(logits if dec.bias is None else logits + dec.bias.double(), -1)
    nll64 = -logp.gather(1, walk["tgt"].view(-1, 1)).squeeze(1).detach()
    assert float((nll64 - torch.from_numpy(t["nll_model"]).to(dev).double()).abs().max()) <= 2e-5 * float(nll64.max())
    # ... and the reference applied to them gives the per-token figures
    lse, match = R.text_scores(walk["rows"], walk["tgt"], [rep.theta], window)
    _compare("%s lse" % kind, torch.from_numpy(t["lse"]).to(dev), lse[0])
    _compare("%s match" % kind, torch.from_numpy(t["match"]).to(dev), match[0])
    want = R.cache_mix(torch.from_numpy(t["nll_model"]).to(dev), lse[0], match[0], lam)
    _compare("%s nll" % kind, torch.from_numpy(t["nll"]).to(dev), want)
    assert abs(rep.loss - float(want.mean())) <= BOUND * rep.loss
    hits = torch.isfinite(match[0])
    assert rep.cache_hit_rate == int(hits.sum()) / n and 0.0 < rep.cache_hit_rate < 1.0
    assert abs(rep.mean_cache_prob - float(torch.where(hits, (match[0] - lse[0]).exp(), torch.zeros_like(lse[0])).mean())) <= BOUND
    assert t["nll"][0] == t["nll_model"][0] and np.isneginf(t["lse"][0])  # the first token has an empty cache
    # lambda = 0 is the model alone, bit for bit
    zero = engine.evaluate_cache(m, src, seq_len, window, theta, 0.0, keep_tokens=True)
    assert np.array_equal(zero.per_token["nll"], plain.per_token["nll"]) and zero.loss == zero.base_loss == plain.loss
    assert not m.training


@pytest.mark.parametrize("kind", ["tlm", "lstm"])
def test_result_does_not_depend_on_the_grouping_of_windows(dev, deterministic, monkeypatch, kind):
    from bayeslms_amd import engine
    m, src = _model(kind, dev), _source(_text(), kind, 20, dev)
    args = (m, src, 20, 100, (0.02 if kind == "tlm" else 2.0), 0.3)
    default = engine.evaluate_cache(*args, keep_tokens=True)
    monkeypatch.setenv("BLM_EVAL_WINDOWS", "1")
    single = engine.evaluate_cache(*args, keep_tokens=True)
    for f in ("nll", "lse", "match"):
        _compare("%s windows 1 against default: %s" % (kind, f), torch.from_numpy(single.per_token[f]), torch.from_numpy(default.per_token[f]))
    assert abs(single.loss - default.loss) <= BOUND * default.loss and single.tokens == default.tokens


def test_fit_cache_finds_the_repeats_of_a_repeating_text(dev, deterministic):
    from bayeslms_amd import data as D, engine
    m = _model("lstm", dev)
    block = torch.from_numpy(np.random.RandomState(2).permutation(np.arange(2, 42)))
    text = block.repeat(50)  # 2000 tokens: a 40-word block, again and again
    src = D.batchify(text, 2, dev)
    fit = engine.fit_cache(m, src, 35, 100)
    print("repeating text: theta %.6g lambda %.4f loss %.4f -> %.4f at_bound %s" % (fit.theta, fit.lam, fit.loss_before, fit.loss_after, fit.at_bound))
    assert fit.lam > 0 and fit.loss_after < fit.loss_before and len(fit.curve) >= 8
    assert fit.theta == float(np.float32(fit.theta)) and all(fit.loss_after <= c[2] + 1e-12 for c in fit.curve)
    # evaluate_cache at the fitted pair gives the fit's loss (float32 mix on the device against the fit's float64)
    rep = engine.evaluate_cache(m, src, 35, 100, fit.theta, fit.lam)
    assert abs(rep.loss - fit.loss_after) <= BOUND * fit.loss_after and abs(rep.base_loss - fit.loss_before) <= 1e-9 * fit.loss_before
    assert rep.loss < rep.base_loss


@pytest.mark.parametrize("kind", ["tlm", "lstm"])
def test_fit_cache_never_does_worse_than_the_model(dev, deterministic, kind):
    from bayeslms_amd import engine
    m, src = _model(kind, dev), _source(_text(seed=4), kind, 35, dev)
    walks = []
    hook = m.register_forward_pre_hook(lambda mod, args: walks.append(1))
    try:
        fit = engine.fit_cache(m, src, 35, 60, passes=2)
    finally:
        hook.remove()
    one_walk = len(list(engine._eval_windows(src, 35, hasattr(m, "init_hidden"))))
    print("%s synthetic text: theta %.6g lambda %.4f loss %.6f -> %.6f" % (kind, fit.theta, fit.lam, fit.loss_before, fit.loss_after))
    assert len(walks) == one_walk  # the model walked the text once, whatever the number of passes
    assert fit.loss_after <= fit.loss_before and 0.0 <= fit.lam <= 0.95 and 8 <= len(fit.curve) <= 16
    assert abs(fit.loss_before - engine.evaluate_report(m, src, 35).loss) <= 1e-9 * fit.loss_before


def test_engine_refuses_a_model_without_rows(dev):
    from bayeslms_amd import engine, ops

    class NoDecoder(torch.nn.Module):
        pass
    with pytest.raises(ops.BayesLMError, match="no decoder that hands back its input rows"):
        engine.evaluate_cache(NoDecoder(), torch.zeros(10, 2, dtype=torch.int64, device=dev), 5, 10, 0.1, 0.1)


def test_evaluate_cli_with_and_without_the_cache(dev, tmp_path, capsys, deterministic):
    from bayeslms_amd import data as D, engine, evaluate as E
    from test_gpu_eval_report import _Vocab, _write_text
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(2, V)]
    m = _model("tlm", dev)
    torch.save({k: v.detach().cpu() for k, v in m.state_dict().items()}, str(tmp_path / "model.pt"))
    (tmp_path / "words.txt").write_text("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    _write_text(tmp_path / "test.txt", _text().tolist(), words)
    _write_text(tmp_path / "valid.txt", _text(1200, seed=8).tolist(), words)
    common = ["--model-path", str(tmp_path / "model.pt"), "--vocabulary", str(tmp_path / "words.txt"), "--data", str(tmp_path / "test.txt"),
              "--model", "Transformer", "--emsize", "128", "--nhid", "256", "--nlayers", "2", "--nhead", "2", "--seq-len", "20",
              "--batch-size", "5"]
    rp = tmp_path / "report.json"
    src = D.batchify(E.D.Corpus.tokenize(_Vocab(words), str(tmp_path / "test.txt")), 5, dev)
    val = D.batchify(E.D.Corpus.tokenize(_Vocab(words), str(tmp_path / "valid.txt")), 5, dev)

    def run(extra):
        E.main(common + extra + ["--write-report", str(rp)])
        out = capsys.readouterr()
        line = out.out.strip().splitlines()
        assert len(line) == 1
        return json.loads(rp.read_text()), line[0], out.err

    # no flag: no cache key, and the line of before the cache existed, character for character
    plain = engine.evaluate_report(m, src, 20)
    rep, line, err = run([])
    assert "cache" not in rep and rep == json.loads(json.dumps(plain.as_dict())) and err == ""
    assert line == "| evaluate | tokens %d | skipped %d | loss %.4f | ppl %.2f | accuracy %.4f | top5 %.4f | ece %.4f" % (
        plain.tokens, plain.skipped, plain.loss, plain.ppl, plain.accuracy, plain.top5_accuracy, plain.ece)
    # given values
    rep, line2, err = run(["--cache-window", "80", "--cache-theta", "0.02", "--cache-lambda", "0.1"])
    want = engine.evaluate_cache(m, src, 20, 80, 0.02, 0.1)
    c = rep["cache"]
    assert c == json.loads(json.dumps(want.as_dict())) and {k: v for k, v in rep.items() if k != "cache"} == json.loads(json.dumps(plain.as_dict()))
    assert line2 == line + " | cache window 80 theta %.6g lambda 0.1000 | loss %.4f -> %.4f | ppl %.2f -> %.2f | hit %.4f" % (
        c["theta"], c["base_loss"], c["loss"], c["base_ppl"], c["ppl"], c["cache_hit_rate"])
    assert c["base_loss"] == rep["loss"] and err == ""
    # fitted on another text
    rep, line3, err = run(["--cache-window", "80", "--fit-cache-on", str(tmp_path / "valid.txt"), "--cache-fit-passes", "2"])
    c = rep["cache"]
    fit = engine.fit_cache(m, val, 20, 80, passes=2)
    assert (c["theta"], c["lam"], c["at_bound"], c["fit_loss_before"], c["fit_loss_after"]) == (fit.theta, fit.lam, fit.at_bound, fit.loss_before, fit.loss_after)
    assert c["fitted_on"] == str(tmp_path / "valid.txt") and c["curve"] == json.loads(json.dumps(fit.curve)) and c["fit_loss_after"] <= c["fit_loss_before"]
    assert ("warning" in err) == c["at_bound"] and "| cache window 80 theta" in line3 and line3.startswith(line)
