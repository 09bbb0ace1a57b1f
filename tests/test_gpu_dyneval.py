"""GPU: dynamic evaluation -- blm_dyneval_accum / _rms / _update (ops.dyneval_*) against the float64 reference of
tests/dyneval_reference.py, then engine.evaluate_dynamic / dyneval_stats / fit_dyneval on tiny models.

Kernel bound, derived: an output is at most about eight rounded fp32 operations on its terms, so
|out - ref| <= 16 * 2^-24 * (|p| + |step| + |d (p0 - p)|) per element; ms and rms are held the same way against their own
terms (|ms| + g^2, and |rms|).  rbar comes from double partial sums of fp32 values: within 2^-22 relative; the live count exact.

The walk is pinned bit for bit against a loop written here from the same pieces (forward, ops.cross_entropy, backward,
ops.dyneval_update on an engine.FlatBuffers of a copy of the model), under ops.set_deterministic().  The static walk's per-token
NLL is held to float64 from the model's own logits at 1e-5 of the largest value: the forward tolerance of the "cross_entropy"
case of tests/test_gpu_operand_layouts.py (Case.tol[0], its `rel`)."""
import copy

import numpy as np
import pytest
import torch

import dyneval_reference as R

pytestmark = pytest.mark.gpu

ULP16 = 16.0 * 2.0 ** -24
GRID, BLOCK = 2048, 256  # csrc/dyneval.hip: DYN_GRID x DYN_TPB lanes, one float4 each per trip
SIZES = [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1025, 2 * GRID * BLOCK * 4 + 3]  # the last: every lane loops twice, a tail remains
LR, DECAY, EPS, COUNT = 0.3, 0.5, 0.01, 3
V, W, SEQ, COLS, ROWS = 48, 32, 4, 2, 23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def deterministic():
    from bayeslms_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(was)


# ------------------------------------------------------------------ kernels
_INPUT = {}


def _inputs(n):
    """fp32 host arrays, made once per size and never written: magnitudes from 1e-6 to 1e3, zeros in g and ms, a stretch with
    p == p0 (part of it without a gradient), entries whose decay * r / rbar exceeds 1"""
    if n not in _INPUT:
        rng = np.random.default_rng(1000 + n % 9973)
        mag = lambda: 10.0 ** rng.uniform(-6, 3, n)  # noqa: E731
        p = (rng.standard_normal(n) * mag()).astype(np.float32)
        g = (rng.standard_normal(n) * mag()).astype(np.float32)
        p0 = (p * (1 + 0.05 * rng.standard_normal(n))).astype(np.float32)
        ms = (rng.random(n) * mag() ** 2).astype(np.float32)
        g[rng.random(n) < 0.2] = 0.0
        ms[rng.random(n) < 0.2] = 0.0
        a, b = n // 3, n // 3 + max(1, n // 5)
        p0[a:b] = p[a:b]
        g[a:(a + b + 1) // 2] = 0.0
        ms[0] = max(ms[0], np.float32(1e-3))  # at least one live entry
        _INPUT[n] = tuple(np.ascontiguousarray(x) for x in (p, g, p0, ms))
    return _INPUT[n]


def _dev(dev, *arrays, offset=0):
    """device copies; ``offset`` > 0: views that start that many floats into a 16-byte aligned allocation (the scalar path)"""
    out = []
    for a in arrays:
        t = torch.empty(a.shape[0] + offset, device=dev, dtype=torch.float32)
        t[offset:].copy_(torch.from_numpy(a))
        out.append(t[offset:])
    return out


def _within(name, got, want, bound):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), name
    err = np.abs(got - want)
    worst = int(np.argmax(err - bound))
    assert (err <= bound).all(), (name, worst, got[worst], want[worst], err[worst], bound[worst])


@pytest.mark.parametrize("n", SIZES)
def test_accum_and_rms_match_float64(dev, n):
    from bayeslms_amd import ops
    p, g, p0, ms = _inputs(n)
    d_ms, d_g = _dev(dev, ms, g)
    assert ops.dyneval_accum(d_ms, d_g) is d_ms
    _within("accum", d_ms, R.accum(ms, g), ULP16 * (np.abs(R.f64(ms)) + R.f64(g) ** 2))
    assert torch.equal(d_g.cpu(), torch.from_numpy(g))
    (d_ms,) = _dev(dev, ms)
    rms, mean = ops.dyneval_rms(d_ms, COUNT)
    r, rbar, live = R.rms(ms, COUNT)
    _within("rms", rms, r, ULP16 * np.abs(r))
    assert torch.equal(rms == 0, d_ms == 0) and torch.equal(d_ms.cpu(), torch.from_numpy(ms))
    got_rbar, got_live = (float(v) for v in mean.cpu())
    assert got_live == live and live >= 1  # exact (n < 2^24)
    assert abs(got_rbar - rbar) <= 2.0 ** -22 * rbar, (got_rbar, rbar)
    rms2, mean2 = ops.dyneval_rms(d_ms, COUNT)
    assert torch.equal(rms, rms2) and torch.equal(mean, mean2)  # fixed-order sums: the same bits


# offset 1: arrays that start one float into an aligned allocation take the scalar path for their whole length
@pytest.mark.parametrize("rule", ["sgd", "rms"])
@pytest.mark.parametrize("n,offset", [(n, 0) for n in SIZES] + [(5, 1), (1025, 1)])
def test_update_matches_float64(dev, n, rule, offset):
    from bayeslms_amd import ops
    p, g, p0, ms = _inputs(n)
    kw, ref_kw = {}, {}
    if rule == "rms":
        (d_ms,) = _dev(dev, ms)
        rms, mean = ops.dyneval_rms(d_ms, COUNT)
        if offset:
            (rms,) = _dev(dev, rms.cpu().numpy(), offset=offset)
        kw = dict(rms=rms, mean=mean, eps=EPS)
        ref_kw = dict(r=rms.cpu().numpy(), rbar=float(mean[0]), eps=EPS)
        if n >= 255:
            assert (DECAY * ref_kw["r"].astype(np.float64) / ref_kw["rbar"] > 1).any()  # the clip of the pull is exercised
    want = R.update(p, g, p0, LR, DECAY, **ref_kw)
    bound = R.update_bound(p, g, p0, LR, DECAY, **ref_kw)
    still = (g == 0) & (p == p0)
    assert still.any() or n < 3
    runs = []
    for zero_grad in (True, False, True):
        d_p, d_g, d_p0 = _dev(dev, p, g, p0, offset=offset)
        assert (d_p.data_ptr() % 16 == 0) == (offset == 0)
        assert ops.dyneval_update(d_p, d_g, d_p0, LR, DECAY, zero_grad=zero_grad, **kw) is d_p
        _within("update %s zero_grad=%s" % (rule, zero_grad), d_p, want, bound)
        got = d_p.cpu()
        assert torch.equal(got[torch.from_numpy(still)], torch.from_numpy(p[still]))  # bit-identical where nothing acts
        if zero_grad:
            assert not d_g.any()
        else:
            assert torch.equal(d_g.cpu(), torch.from_numpy(g))
        assert torch.equal(d_p0.cpu(), torch.from_numpy(p0))
        runs.append(got)
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])  # run to run, and whatever zero_grad is


def test_zero_rates_leave_the_weights_and_rms_without_live_entries_raises(dev):
    from bayeslms_amd import ops
    p, g, p0, ms = _inputs(1023)
    d_p, d_g, d_p0 = _dev(dev, p, g, p0)
    ops.dyneval_update(d_p, d_g, d_p0, 0.0, 0.0, zero_grad=False)
    assert torch.equal(d_p.cpu(), torch.from_numpy(p))
    with pytest.raises(ops.BayesLMError, match="no live entry"):
        ops.dyneval_rms(torch.zeros(1000, device=dev), 2)
    with pytest.raises(ops.BayesLMError, match="g has 5 elements"):
        ops.dyneval_update(d_p, d_g[:5], d_p0, 0.1, 0.1)
    with pytest.raises(ops.BayesLMError, match="p0 must be contiguous"):
        ops.dyneval_update(d_p[:500], d_g[:500], d_p0[::2][:500], 0.1, 0.1)
    with pytest.raises(ops.BayesLMError, match="lr"):
        ops.dyneval_update(d_p, d_g, d_p0, -0.1, 0.1)
    with pytest.raises(ops.BayesLMError, match="ms must be"):
        ops.dyneval_accum(d_p.double(), d_g)


# ------------------------------------------------------------------ the walk
def _models(dev):
    from bayeslms_amd import model as M
    torch.manual_seed(5)
    # a Bayesian feed-forward, so log sigma slots exist; Bayes2LSTM is two layers by construction
    return {"transformer": M.BayesTransformerModel(V, W, 2, W, 1, 0.0, True, "FFN").to(dev),
            "lstm": M.BayesRNNModel("LSTM", V, W, W, 2, 0.0, True, 1).to(dev)}


@pytest.fixture(scope="module")
def models(dev):
    return _models(dev)


@pytest.fixture(scope="module")
def text(dev):
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, V, (ROWS, COLS), generator=g).to(dev)  # 2 x 23 tokens: five full windows of 4 rows and one of 2


def _forward(m, data, hidden):
    from bayeslms_amd.model import repackage_hidden
    if hidden is None:
        return m(data), None
    out, hidden = m(data, hidden)
    return out, repackage_hidden(hidden)


def _loop(model, source, lr=None, decay=None, stats=None, eps=EPS, windows=None):
    """The walk restated from its pieces on a COPY of the model -> (per-token NLL in walk order, the gradient of every window).
    ``lr`` None: no update (the statistics walk), the gradient cleared by hand."""
    from bayeslms_amd import engine, ops
    from bayeslms_amd.data import get_batch
    m = copy.deepcopy(model).eval()
    flat = engine.FlatBuffers(m)
    theta0 = flat.flat_param.clone()
    hidden = m.init_hidden(source.shape[1]) if hasattr(m, "init_hidden") else None
    starts = list(range(0, source.shape[0] - 1, SEQ))[:windows]
    nlls, grads = [], []
    for i in starts:
        data, targets = get_batch(source, i, SEQ)
        out, hidden = _forward(m, data, hidden)
        loss, nll = ops.cross_entropy(out.view(-1, V), targets, unit_grad=True)
        loss.backward()
        nlls.append(nll.clone())
        grads.append(flat.flat_grad.clone())
        if lr is None:
            flat.zero_grad()
        elif i != starts[-1]:
            ops.dyneval_update(flat.flat_param, flat.flat_grad, theta0, lr, decay, None if stats is None else stats.rms,
                               None if stats is None else stats.mean, eps, zero_grad=True)
    return torch.cat(nlls), grads, flat


def _text_order(walk_nll):
    """walk order is (row, column) row-major over the target rows; text order is column by column"""
    return walk_nll.reshape(-1, COLS).t().reshape(-1)


@pytest.mark.parametrize("kind", ["transformer", "lstm"])
def test_static_walk_matches_float64_from_the_models_own_logits(dev, models, text, kind, deterministic):
    from bayeslms_amd import engine
    from bayeslms_amd.data import get_batch
    m = models[kind]
    rep = engine.evaluate_dynamic(m, text, SEQ, 0.0, 0.0, keep_tokens=True)
    assert (rep.tokens, rep.windows, rep.updates, rep.rule) == ((ROWS - 1) * COLS, 6, 5, "sgd")
    want = []
    hidden = m.init_hidden(COLS) if hasattr(m, "init_hidden") else None
    m.eval()
    with torch.no_grad():
        for i in range(0, ROWS - 1, SEQ):
            data, targets = get_batch(text, i, SEQ)
            out, hidden = _forward(m, data, hidden)
            want.append(torch.nn.functional.cross_entropy(out.reshape(-1, V).double(), targets, reduction="none"))
    want = _text_order(torch.cat(want)).cpu().numpy()
    got = rep.per_token["nll"].astype(np.float64)
    assert np.abs(got - want).max() / np.abs(want).max() < 1e-5
    assert abs(rep.loss - want.mean()) <= 1e-5 * want.mean() and rep.ppl == pytest.approx(np.exp(rep.loss))
    assert np.array_equal(rep.per_token["tgt"], text[1:].t().reshape(-1).cpu().numpy())


@pytest.mark.parametrize("rule", ["sgd", "rms"])
@pytest.mark.parametrize("kind", ["transformer", "lstm"])
def test_adapted_walk_equals_a_loop_of_the_same_pieces_bit_for_bit(dev, models, text, kind, rule, deterministic):
    from bayeslms_amd import engine
    m = models[kind]
    stats = engine.dyneval_stats(m, text.flip(0).contiguous(), SEQ, 3) if rule == "rms" else None
    lr, decay = (0.5, 0.02) if rule == "sgd" else (0.02, 0.02)
    rep = engine.evaluate_dynamic(m, text, SEQ, lr, decay, stats=stats, keep_tokens=True)
    want, grads, _ = _loop(m, text, lr, decay, stats)
    got = torch.from_numpy(rep.per_token["nll"])
    assert torch.equal(got, _text_order(want).cpu())  # score before update, the carried state, zero_grad, no update after the last
    assert rep.rule == rule and rep.updates == 5
    static = torch.from_numpy(engine.evaluate_dynamic(m, text, SEQ, 0.0, 0.0, keep_tokens=True).per_token["nll"])
    first = SEQ  # per column, the first window's tokens come before any update
    assert torch.equal(got.reshape(COLS, -1)[:, :first], static.reshape(COLS, -1)[:, :first])
    assert not torch.equal(got.reshape(COLS, -1)[:, first:2 * first], static.reshape(COLS, -1)[:, first:2 * first])  # the weights moved


@pytest.mark.parametrize("kind", ["transformer", "lstm"])
def test_no_token_sees_weights_adapted_on_its_future(dev, models, text, kind, deterministic):
    from bayeslms_amd import engine
    m = models[kind]
    other = text.clone()
    other[ROWS - 2:] = (other[ROWS - 2:] + 7) % V  # the last window's targets and its second input row
    a = engine.evaluate_dynamic(m, text, SEQ, 0.5, 0.02, keep_tokens=True).per_token["nll"].reshape(COLS, -1)
    b = engine.evaluate_dynamic(m, other, SEQ, 0.5, 0.02, keep_tokens=True).per_token["nll"].reshape(COLS, -1)
    assert np.array_equal(a[:, :ROWS - 3], b[:, :ROWS - 3]) and not np.array_equal(a[:, ROWS - 3:], b[:, ROWS - 3:])


def _snapshot(m):
    from bayeslms_amd import ops
    return ({k: v.clone() for k, v in m.state_dict().items()}, [(p.data_ptr(), p.grad) for p in m.parameters()],
            [mod.training for mod in m.modules()], ops._GRAD_HOOK, ops._EMBED_SINK)


def _assert_restored(m, snap):
    from bayeslms_amd import ops
    sd, ptrs, flags, hook, sink = snap
    now = m.state_dict()
    assert list(now) == list(sd) and all(torch.equal(now[k], sd[k]) for k in sd)
    for p, (ptr, grad) in zip(m.parameters(), ptrs):
        assert p.data_ptr() == ptr and p.grad is grad
    assert [mod.training for mod in m.modules()] == flags
    assert ops._GRAD_HOOK is hook and ops._EMBED_SINK is sink


@pytest.mark.parametrize("kind", ["transformer", "lstm"])
def test_the_model_is_left_as_it_was_found(dev, models, text, kind, deterministic):
    from bayeslms_amd import engine, ops
    m = copy.deepcopy(models[kind])
    m.train()
    first = next(m.parameters())
    first.grad = torch.full_like(first, 0.25)
    hook, sink = (lambda p: None), (lambda w, ids: None)
    ops.set_grad_ready_hook(hook)
    ops.set_embed_grad_sink(sink)
    try:
        snap = _snapshot(m)
        engine.evaluate_dynamic(m, text, SEQ, 0.5, 0.02)
        _assert_restored(m, snap)
        stats = engine.dyneval_stats(m, text, SEQ, 2)
        _assert_restored(m, snap)
        engine.fit_dyneval(m, text, SEQ, [0.1], [0.01], stats=stats, max_windows=3)
        _assert_restored(m, snap)

        class Stop(Exception):
            pass

        def on_window(k, nll):
            if k == 2:
                raise Stop()

        with pytest.raises(Stop):
            engine.evaluate_dynamic(m, text, SEQ, 0.5, 0.02, on_window=on_window)
        _assert_restored(m, snap)
        assert torch.equal(first.grad, torch.full_like(first, 0.25))
    finally:
        ops.set_grad_ready_hook(None)
        ops.set_embed_grad_sink(None)


@pytest.mark.parametrize("kind", ["transformer", "lstm"])
def test_stats_match_the_reference_fed_with_the_windows_gradients(dev, models, text, kind, deterministic):
    """The same bound as the kernels': three fp32 additions of squares, a division and a root are inside the eight operations."""
    from bayeslms_amd import engine
    m = models[kind]
    stats = engine.dyneval_stats(m, text, SEQ, 3)
    _, grads, flat = _loop(m, text, windows=3)
    assert stats.windows == 3 and len(grads) == 3 and stats.rms.numel() == flat.total
    ms = sum(R.f64(g.cpu().numpy()) ** 2 for g in grads)
    r = np.sqrt(ms / 3.0)
    live = ms > 0
    _within("stats rms", stats.rms, r, ULP16 * np.abs(r))
    assert stats.live == int(live.sum()) == int(stats.mean[1]) and 0 < stats.live < flat.total
    rbar = r[live].sum() / live.sum()
    assert abs(float(stats.mean[0]) - rbar) <= ULP16 * rbar
    names = [k for k, p in m.named_parameters() if p.requires_grad]  # the order of FlatBuffers' slots
    assert len(names) == len(flat.params) and any("lgstd" in k for k in names)
    for k, o, p in zip(names, flat.offsets, flat.params):
        if "lgstd" in k:
            assert not stats.rms[o:o + p.numel()].any(), k  # log sigma gets no gradient in eval mode: not live
    assert engine.dyneval_stats(m, text, SEQ, 100).windows == 6  # a shorter text gives what it has


def test_fit_is_a_grid_of_plain_walks(dev, models, text, deterministic):
    from bayeslms_amd import engine
    m = models["transformer"]
    fit = engine.fit_dyneval(m, text, SEQ, [0.1, 0.5], [0.0, 0.02])
    assert [c[:2] for c in fit.curve] == [[0.0, 0.0], [0.1, 0.0], [0.1, 0.02], [0.5, 0.0], [0.5, 0.02]]
    for lr, decay, loss in fit.curve:
        assert loss == engine.evaluate_dynamic(m, text, SEQ, lr, decay).loss, (lr, decay)
    assert fit.curve[0][2] == fit.loss_static and fit.loss == min(c[2] for c in fit.curve) <= fit.loss_static
    assert [fit.lr, fit.decay, fit.loss] in fit.curve
    short = engine.fit_dyneval(m, text, SEQ, [0.5], [0.02], max_windows=2)
    assert short.curve[1][2] == engine.evaluate_dynamic(m, text[:2 * SEQ + 1], SEQ, 0.5, 0.02).loss


FAMILIES = {
    "TransformerModel": lambda M: M.TransformerModel(V, W, 2, W, 1, 0.0, "gelu", True),
    "BayesTransformerModel-MHA": lambda M: M.BayesTransformerModel(V, W, 2, W, 1, 0.0, True, "MHA"),
    "BayesTransformerModel-EMB": lambda M: M.BayesTransformerModel(V, W, 2, W, 1, 0.0, True, "EMB"),
    "RNNModel": lambda M: M.RNNModel("LSTM", V, W, W, 2, 0.0, True),
    "GaussTransformerModel": lambda M: M.GaussTransformerModel(V, W, 2, W, 1, 0.0, True, 3),
    "VTransformerModel": lambda M: M.VTransformerModel(V, W, 2, W, 1, 0.0, True, 0),
    "GaussRNNModel": lambda M: M.GaussRNNModel("LSTM", V, W, W, 2, 0.0, False, "00"),
    "VariationalRNNModel": lambda M: M.VariationalRNNModel("LSTM", V, W, W, 2, 0.0, True, "11"),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_supported_family_adapts(dev, text, family, deterministic):
    """The eval-mode forward of each family back-propagates through the engine's ops: the walk equals the loop of its pieces, the
    weights move after the first window, and the model is left alone."""
    from bayeslms_amd import engine, model as M
    torch.manual_seed(3)
    m = FAMILIES[family](M).to(dev)
    assert type(m).__name__ in engine._DYNEVAL_FAMILIES
    want, grads, _ = _loop(m, text, 0.5, 0.02)  # first: a grad-mode forward parks its last state on a VLSTMCell, which deepcopy refuses
    snap = _snapshot(m)
    rep = engine.evaluate_dynamic(m, text, SEQ, 0.5, 0.02, keep_tokens=True)
    _assert_restored(m, snap)
    assert np.isfinite(rep.loss) and torch.equal(torch.from_numpy(rep.per_token["nll"]), _text_order(want).cpu())
    assert all(bool(g.any()) and bool(torch.isfinite(g).all()) for g in grads)
    static = engine.evaluate_dynamic(m, text, SEQ, 0.0, 0.0).loss
    assert rep.loss != static


def test_refused_combinations_raise_the_named_error(dev, models, text):
    from bayeslms_amd import engine, ops
    m = models["transformer"]
    for kw, word in ((dict(mc_samples=4), "mc_samples"), (dict(temperature=0.5), "temperature"), (dict(cache_window=50), "cache")):
        with pytest.raises(ops.BayesLMError, match=word):
            engine.evaluate_dynamic(m, text, SEQ, 0.1, 0.1, **kw)
    stats = engine.dyneval_stats(models["lstm"], text, SEQ, 2)
    with pytest.raises(ops.BayesLMError, match="stats must be the DynEvalStats of this model"):
        engine.evaluate_dynamic(m, text, SEQ, 0.1, 0.1, stats=stats)
    with pytest.raises(ops.BayesLMError, match="stats must be"):
        engine.evaluate_dynamic(m, text, SEQ, 0.1, 0.1, stats=(stats.rms, stats.mean))
    with pytest.raises(ops.BayesLMError, match="Linear"):
        engine.evaluate_dynamic(torch.nn.Linear(3, 3).to(dev), text, SEQ, 0.1, 0.1)
    with pytest.raises(ops.BayesLMError, match="two are the least"):
        engine.evaluate_dynamic(m, text[:1], SEQ, 0.1, 0.1)
    m2 = copy.deepcopy(m)
    m2.set_noise_source("torch")
    with pytest.raises(ops.BayesLMError, match="noise source 'torch'"):
        engine.evaluate_dynamic(m2, text, SEQ, 0.1, 0.1)


def test_command_line_reports_the_block(dev, tmp_path, capsys):
    import json
    from bayeslms_amd import evaluate as E, model as M
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(2, V)]
    (tmp_path / "words.txt").write_text("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    rng = np.random.default_rng(0)
    for name in ("test.txt", "valid.txt", "train.txt"):
        (tmp_path / name).write_text("".join(" ".join(words[j] for j in rng.integers(2, V, 6)) + "\n" for _ in range(12)))
    torch.manual_seed(2)
    m = M.RNNModel("LSTM", V, W, W, 2, 0.5, True)
    torch.save(m.state_dict(), tmp_path / "m.pt")
    base = ["--model-path", str(tmp_path / "m.pt"), "--vocabulary", str(tmp_path / "words.txt"), "--data", str(tmp_path / "test.txt"),
            "--emsize", str(W), "--nhid", str(W), "--seq-len", "5", "--batch-size", "2"]
    plain = E.main(base)
    line0 = capsys.readouterr().out.strip()
    rep = E.main(base + ["--dyneval-lr", "0.3", "--dyneval-decay", "0.01", "--write-report", str(tmp_path / "r.json")])
    line1 = capsys.readouterr().out.strip()
    d = json.loads((tmp_path / "r.json").read_text())["dyneval"]
    assert line1.startswith(line0 + " | dyneval rule sgd lr 0.3 decay 0.01 | loss ") and rep.loss == plain.loss
    assert d["rule"] == "sgd" and d["base_loss"] == plain.loss and d["loss"] != plain.loss and "per_token" not in d
    rep = E.main(base + ["--fit-dyneval-on", str(tmp_path / "valid.txt"), "--dyneval-lr-grid", "0.1,0.3", "--dyneval-decay-grid", "0.01",
                         "--dyneval-stats-on", str(tmp_path / "train.txt"), "--dyneval-stats-windows", "3", "--dyneval-fit-windows", "4"])
    d = rep.dyneval
    assert d["rule"] == "rms" and d["fitted_on"].endswith("valid.txt") and len(d["curve"]) == 3
    assert d["fit_loss_after"] <= d["fit_loss_before"] and [d["lr"], d["decay"]] in [c[:2] for c in d["curve"]]
    assert " | dyneval rule rms lr " in capsys.readouterr().out
