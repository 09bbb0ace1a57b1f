"""GPU: Monte-Carlo weight samples in incremental scoring and generation.

blm_linear_mc_logprobs / ops.linear_mc_logprobs against float64 of the materialised logits (every element of the M x V result);
IncrementalLM(mc_samples=S) fed token by token, in chunks and ragged against the float64 model average of full forwards in the
scorer's sampling state; the n-best scorer's per-token uncertainty reproduced stream by stream; beams; the mean-weight default
untouched; the generate CLI's --mc-samples / --write-uncertainty."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bayeslms_amd import BayesLMError
from conftest import ROOT
from test_gpu_mc_uncertainty import _inputs, _scorer_model, _want

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _ops():
    from bayeslms_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------------------------ kernel
def _want_logp(x, w, b, chunk=256):
    """float64 log pbar (M, V) over the materialised logits of x (S, M, K)."""
    S, M, _ = x.shape
    V = w.shape[0]
    wd = w.double()
    bd = b.double() if b is not None else torch.zeros(V, dtype=torch.float64, device=w.device)
    out = []
    for a in range(0, M, chunk):
        lp = torch.log_softmax(x[:, a:a + chunk].double() @ wd.t() + bd, -1)
        out.append(torch.logsumexp(lp, 0) - math.log(S))
    return torch.cat(out)


def _within(name, got, want, rel=2e-5):
    """element-wise |got - want| <= rel * max(1, |want|), over every element; the worst excess is printed before it is judged"""
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    diff = (got - want).abs()
    worst = float((diff / want.abs().clamp(min=1.0)).max())
    print("%s: max |got - want| %.3e, max over the bound's scale %.3e (bound %.1e)" % (name, float(diff.max()), worst, rel))
    assert bool((diff <= rel * want.abs().clamp(min=1.0)).all()), (name, worst)


def _check_all(got, want, want_logp):
    wn, wb, wh, wm = want
    _within("logp", got.logp, want_logp)
    _within("nll_s", got.nll_s, wn)
    _within("bma_nll", got.bma_nll, wb)
    _within("h_pred", got.h_pred, wh)
    mi = got.mi.double()
    print("mi: max |got - want| %.3e, min %.3e" % (float((mi - wm).abs().max()), float(mi.min())))
    assert bool(((mi - wm).abs() <= 1e-5 + 1e-4 * wm).all()), float((mi - wm).abs().max())
    assert float(mi.min()) >= -1e-6


SHAPES = [(2048, 8, 33000, 512), (700, 4, 33278, 1024), (77, 3, 1000, 60), (129, 16, 260, 33), (5, 1, 52, 18), (2, 64, 8, 4),
          (33, 5, 1001, 64),  # the seven of test_mc_stats_equal_float64_of_the_materialised_logits, then the decode shapes
          (1, 8, 33000, 512), (64, 8, 33000, 512), (3, 5, 33000, 512), (1, 8, 33278, 512), (64, 8, 33278, 512), (3, 5, 33278, 512)]


@pytest.mark.parametrize("M,S,V,K", SHAPES)
def test_mc_logprobs_equal_float64_of_the_materialised_logits(dev, M, S, V, K):
    """Every plan tile where it is legal (the guarded kernel for K % 4 != 0): ALL M x V elements of log pbar, the per-sample and
    model-average NLL and the predictive entropy within 2e-5 max(1, |want|) of log_softmax / log-mean-exp of the fp64 logits,
    the mutual information within 1e-5 + 1e-4 want and >= -1e-6; V % 4 != 0 runs on the padded decoder copy and padded rows."""
    from bayeslms_amd import _lib as L
    ops = _ops()
    x, w, b, tgt = _inputs(dev, M, S, V, K)
    want, want_logp = _want(x, w, b, tgt), _want_logp(x, w, b)
    tiles = (0,) if (K % 4 or V < 64) else (0, 11, 12, 21, 22, 28)
    for tile in tiles:
        L.check(L.lib().blm_gemm_plan_override(tile, 0), "override")
        try:
            with torch.no_grad():
                got = ops.linear_mc_logprobs(x, w, b, tgt)
        finally:
            L.check(L.lib().blm_gemm_plan_override(0, 0), "override")
        assert got.logp.shape == (M, V) and got.nll_s.shape == (M, S) and got.mi.shape == (M,)
        print("tile", tile)
        _check_all(got, want, want_logp)
    with torch.no_grad():  # no bias, no targets, no statistics: the distribution alone
        got = ops.linear_mc_logprobs(x, w, None, S=S, stats=False)
    assert got.h_pred is None and got.mi is None and got.nll_s is None and got.bma_nll is None
    _within("logp (no bias)", got.logp, _want_logp(x, w, None))
    with torch.no_grad():  # targets select the same values the matrix holds
        got = ops.linear_mc_logprobs(x, w, b, tgt)
    _within("bma_nll vs -logp[target]", got.bma_nll, -got.logp.gather(1, tgt.view(-1, 1)).squeeze(1))


def test_one_sample_is_the_log_softmax(dev):
    ops = _ops()
    for M, V, K in ((300, 4096, 256), (17, 1001, 64)):
        x, w, b, _ = _inputs(dev, M, 1, V, K)
        with torch.no_grad():
            got = ops.linear_mc_logprobs(x, w, b)
            ref = ops.log_softmax_rows(ops.linear(x[0], w, b), V)
        _within("S = 1", got.logp, ref)
        assert float(got.mi.abs().max()) == 0.0


def test_identical_samples(dev):
    ops = _ops()
    M, S, V, K = 300, 8, 5000, 128
    x, w, b, _ = _inputs(dev, M, S, V, K)
    x1 = x[:1].contiguous()
    with torch.no_grad():
        got = ops.linear_mc_logprobs(x1.expand(S, -1, -1).contiguous(), w, b)
        one = ops.linear_mc_logprobs(x1, w, b)
    assert float(got.mi.abs().max()) == 0.0  # exactly: u = 0, W = S, L = 0
    _within("identical samples", got.logp, one.logp)


def test_rows_are_distributions_large_logits_and_padding(dev):
    ops = _ops()
    from bayeslms_amd import _lib as L
    x, w, b, tgt = _inputs(dev, 200, 6, 3001, 64)
    with torch.no_grad():
        got = ops.linear_mc_logprobs(x, w, b, tgt)
        big = ops.linear_mc_logprobs(16.0 * x, w, 16.0 * b, tgt)  # logits of magnitude ~80
    assert float((got.logp.double().exp().sum(-1) - 1.0).abs().max()) <= 1e-4
    z = (16.0 * x[0]) @ w.t() + 16.0 * b
    assert float(z.abs().max()) >= 80.0
    for t in big:
        assert bool(torch.isfinite(t).all())
    assert float((big.logp.double().exp().sum(-1) - 1.0).abs().max()) <= 1e-4
    assert float(big.mi.min()) >= -1e-6
    # the C entry point on a pre-filled (M, ldo) buffer with ldo > ceil4(V): columns >= V keep their contents
    M, S, V, K = 70, 3, 1001, 32
    x, w, b, _ = _inputs(dev, M, S, V, K)
    dec = ops.McDecoder(w, b)
    ldo = 1012
    buf = torch.full((M, ldo), 7.5, device=dev)
    xt = torch.zeros(M, 4, K, device=dev)
    xt[:, :S] = x.transpose(0, 1)
    ws = torch.empty(int(L.lib().blm_linear_mc_logprobs_ws_floats(M, S, V)), device=dev)
    L.check(L.lib().blm_linear_mc_logprobs(xt.data_ptr(), K, dec.wp.data_ptr(), K, dec.bp.data_ptr(), None, S, buf.data_ptr(), ldo,
                                           None, None, None, None, ws.data_ptr(), M, V, K, L.stream()), "blm_linear_mc_logprobs")
    assert bool((buf[:, V:] == 7.5).all())
    _within("padded buffer", buf[:, :V], _want_logp(x, w, b))
    with torch.no_grad():
        got = ops.linear_mc_logprobs(x, w, b)
    assert got.logp.stride(0) == 1004 and torch.equal(got.logp, buf[:, :V])


def test_out_of_range_target_is_nan_for_that_token_only(dev):
    ops = _ops()
    M, S, V = 64, 4, 1001
    x, w, b, tgt = _inputs(dev, M, S, V, 32)
    tgt[5], tgt[9], tgt[11] = V, -1, 1003
    with torch.no_grad():
        got = ops.linear_mc_logprobs(x, w, b, tgt)
    bad = torch.zeros(M, dtype=torch.bool, device=dev)
    bad[[5, 9, 11]] = True
    assert bool(torch.isnan(got.bma_nll[bad]).all()) and bool(torch.isnan(got.nll_s[bad]).all())
    assert bool(torch.isfinite(got.bma_nll[~bad]).all()) and bool(torch.isfinite(got.nll_s[~bad]).all())
    assert bool(torch.isfinite(got.logp).all()) and bool(torch.isfinite(got.h_pred).all()) and bool(torch.isfinite(got.mi).all())


def test_bit_identical_run_to_run_and_inference_only(dev):
    ops = _ops()
    x, w, b, tgt = _inputs(dev, 513, 8, 7000, 256)
    with torch.no_grad():
        a = ops.linear_mc_logprobs(x, w, b, tgt)
        c = ops.linear_mc_logprobs(x, w, b, tgt)
        st = ops.linear_mc_stats(x, w, b, tgt)
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    # the shared epilogue: the statistics are bit for bit those of blm_linear_mc_stats
    assert torch.equal(a.h_pred, st.h_pred) and torch.equal(a.mi, st.mi) and torch.equal(a.bma_nll, st.bma_nll)
    with pytest.raises(Exception, match="inference-only"):
        ops.linear_mc_logprobs(x.clone().requires_grad_(True), w, b, tgt)


# ------------------------------------------------------------------------------------------------------------ IncrementalLM
def _model(kind, dev):
    """-> (eval-mode model on the GPU, 'Transformer' | 'LSTM', vocabulary size)"""
    from bayeslms_amd import model as M
    if kind == "lstm_gauss33":  # as test_mc_sample_scoring_gp_and_variational_families builds its GP-LSTM
        _, _, vocab, _ = _scorer_model("tlm_ffn")
        torch.manual_seed(31)
        m = M.GaussRNNModel("LSTM", len(vocab), 12, 12, 2, 0.5, True, "33")
        with torch.no_grad():
            for k, p in m.named_parameters():
                if "lgstd" in k:
                    p.add_(1.0)
        return m.to(dev).eval(), "LSTM", len(vocab)
    m, mtype, vocab, _ = _scorer_model(kind)
    return m.to(dev).eval(), mtype, len(vocab)


class _sampling:
    """The scorer's sampling state, as test_scorer_uncertainty enters it."""

    def __init__(self, m, seed):
        self.m, self.seed = m, seed

    def __enter__(self):
        from bayeslms_amd.model import variational_sites
        m = self.m
        self.raised = [s for s in variational_sites(m) if getattr(s, "sample", True) is False]
        for s in self.raised:
            s.sample = True
        m.train()
        m.noise_state.dropout_off = True
        m.set_seed(self.seed)

    def __exit__(self, *exc):
        self.m.noise_state.dropout_off = False
        self.m.eval()
        for s in self.raised:
            s.sample = False
        return False


def _reference(m, mtype, src, S, seed, tgt=None):
    """float64 from full forwards over the histories src (T, B), model.set_step(s) per sample:
    -> log pbar (T, B, V), h_pred, mi (T, B), and with tgt (T, B): bma_nll (T, B), nll_s (T, B, S)"""
    lps = []
    with _sampling(m, seed), torch.no_grad():
        for s in range(S):
            m.set_step(s)
            logits = m(src) if mtype == "Transformer" else m(src, m.init_hidden(src.shape[1]))[0]
            lps.append(torch.log_softmax(logits.double().view(src.shape[0], src.shape[1], -1), -1))
    lp = torch.stack(lps)
    lpbar = torch.logsumexp(lp, 0) - math.log(S)
    h = -(lpbar.exp() * lpbar).sum(-1)
    mi = (lp.exp() * (lp - lpbar)).sum(-1).mean(0)
    if tgt is None:
        return lpbar, h, mi
    bma = -lpbar.gather(2, tgt.unsqueeze(2)).squeeze(2)
    nll_s = -lp.gather(3, tgt.view(1, *tgt.shape, 1).expand(S, -1, -1, 1)).squeeze(3).permute(1, 2, 0)
    return lpbar, h, mi, bma, nll_s


def _near(name, got, want, tol=1e-4):
    _within(name, got, want, tol)


@pytest.mark.parametrize("kind", ["tlm_ffn", "lstm_bayes3", "tlm_gauss3", "lstm_gauss33"])
def test_incremental_mc_against_the_full_forward(dev, kind):
    """S = 4, seed 4242: histories fed token by token, in chunks and ragged (a stream with n_new 0 among them); log pbar at the
    last position and at all positions, bma_nll of targets, h_pred, mi and nll_s within 1e-4 max(1, |want|) of the float64
    reference; the NaN slots are exactly the ones n_new leaves without a row; the model comes back in eval mode."""
    from bayeslms_amd.incremental import IncrementalLM
    m, mtype, V = _model(kind, dev)
    S, seed, T, B = 4, 4242, 9, 3
    g = torch.Generator().manual_seed(7)
    src = torch.randint(0, V, (T, B), generator=g).to(dev)
    tgt = torch.randint(0, V, (T, B), generator=g).to(dev)
    lpbar, h, mi, bma, nll_s = _reference(m, mtype, src, S, seed, tgt)
    assert float(mi.sum()) > 1e-6  # the samples do differ
    lm = IncrementalLM(m, max_streams=4, max_len=T, mc_samples=S, seed=seed)
    # token by token
    st = lm.start(B)
    for t in range(T):
        lp, unc = lm.step(st, src[t], return_uncertainty=True)
        assert lp.shape == (B, V) and unc.h_pred.shape == (B,) and unc.mi.shape == (B,) and unc.nll_s is None
        _near("step %d logp" % t, lp, lpbar[t])
        _near("step %d h_pred" % t, unc.h_pred, h[t])
        _near("step %d mi" % t, unc.mi, mi[t])
        assert not m.training and m.noise_state.dropout_off is False
    assert st.lengths == [T] * B
    # chunks: all positions, then targets
    st = lm.start(B)
    lp = lm.step(st, src[:4], all_positions=True)
    _near("chunk logp", lp, lpbar[:4])
    nll, unc = lm.step(st, src[4:], all_positions=True, targets=tgt[4:], return_uncertainty=True)
    assert nll.shape == (T - 4, B) and unc.nll_s.shape == (T - 4, B, S)
    _near("chunk bma_nll", nll, bma[4:])
    _near("chunk nll_s", unc.nll_s, nll_s[4:])
    _near("chunk h_pred", unc.h_pred, h[4:])
    _near("chunk mi", unc.mi, mi[4:])
    # ragged, one stream taking no row at first
    st = lm.start(B)
    k = [5, 0, 7]
    lp, unc = lm.step(st, src[:7], n_new=k, all_positions=True, return_uncertainty=True)
    empty = sum(7 - x for x in k)
    assert int(torch.isnan(lp).sum()) == empty * V and int(torch.isnan(unc.h_pred).sum()) == int(torch.isnan(unc.mi).sum()) == empty
    for n in range(B):
        if k[n]:
            _near("ragged logp %d" % n, lp[:k[n], n], lpbar[:k[n], n])
            _near("ragged h_pred %d" % n, unc.h_pred[:k[n], n], h[:k[n], n])
            _near("ragged mi %d" % n, unc.mi[:k[n], n], mi[:k[n], n])
    one = torch.zeros(3, B, dtype=torch.int64, device=dev)
    one[0, 0] = src[5, 0]
    last, unc = lm.step(st, one, n_new=[1, 0, 0], return_uncertainty=True)  # (n, V): streams 1 and 2 take no row
    assert int(torch.isnan(last).sum()) == 2 * V and int(torch.isnan(unc.mi).sum()) == 2
    _near("ragged single logp", last[0], lpbar[5, 0])
    rest = torch.zeros(T, B, dtype=torch.int64, device=dev)
    kk = [T - 6, T, T - 7]
    for n, a in enumerate((6, 0, 7)):
        rest[:T - a, n] = src[a:, n]
    tl = tgt[T - 1]
    nll, unc = lm.step(st, rest, n_new=kk, targets=tl, return_uncertainty=True)
    assert st.lengths == [T] * B
    _near("ragged bma_nll", nll, bma[T - 1])
    _near("ragged nll_s", unc.nll_s, nll_s[T - 1])
    _near("ragged mi", unc.mi, mi[T - 1])
    assert m.training is False and m.noise_state.dropout_off is False


def test_many_rows_of_a_wide_model(dev):
    """64 streams x 8 samples x d_model 1024 is past the measured crossover (incremental._MC_FUSED_MAX_ROWS_K): the distribution
    alone is composed from the logits, with return_uncertainty it comes from the fused launch; both against the float64
    reference (1e-4 max(1, |want|)) and against each other (2e-5: two fp32 paths)."""
    from bayeslms_amd import incremental, model as M
    torch.manual_seed(13)
    V, d, S, B, T = 1001, 1024, 8, 64, 3
    m = M.BayesTransformerModel(V, d, 8, 256, 1, 0.1, True, "FFN")
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "lgstd" in k:
                p.add_(1.0)
    m = m.to(dev).eval()
    assert B * S * d > incremental._MC_FUSED_MAX_ROWS_K
    src = torch.randint(0, V, (T, B), device=dev)
    lpbar, h, mi = _reference(m, "Transformer", src, S, 5)
    lm = incremental.IncrementalLM(m, max_streams=B, max_len=T, mc_samples=S, seed=5)
    a = lm.step(lm.start(B), src)
    b, unc = lm.step(lm.start(B), src, return_uncertainty=True)
    _near("composed", a, lpbar[-1])
    _near("fused", b, lpbar[-1])
    _within("composed vs fused", a, b)
    _near("h_pred", unc.h_pred, h[-1])
    _near("mi", unc.mi, mi[-1])


def test_models_without_one_sample_per_stream_are_refused(dev):
    from bayeslms_amd import model as M
    from bayeslms_amd.incremental import IncrementalLM
    plain = M.TransformerModel(50, 16, 2, 32, 1, 0.1, "gelu", True).to(dev).eval()
    with pytest.raises(BayesLMError, match="has no variational tensor to sample"):
        IncrementalLM(plain, mc_samples=4)
    var = M.VariationalRNNModel("LSTM", 50, 12, 12, 2, 0.5, True, "11").to(dev).eval()
    with pytest.raises(BayesLMError, match="every time step"):
        IncrementalLM(var, mc_samples=4)
    lm = IncrementalLM(var)  # mean weights: as before
    assert lm.step(lm.start(1), torch.zeros(1, dtype=torch.int64, device=dev)).shape == (1, 50)
    with pytest.raises(BayesLMError, match="return_uncertainty needs mc_samples >= 2"):
        lm.step(lm.start(1), torch.zeros(1, dtype=torch.int64, device=dev), return_uncertainty=True)


def test_same_numbers_as_the_scorer(dev):
    """Per-token bma_nll, h_pred and mi of compute_scores_batched(mc_samples=8, uncertainty=True) against feeding each utterance's
    hypotheses through IncrementalLM(mc_samples=8) as ragged streams with their targets: 1e-4 relative, floor 1."""
    from bayeslms_amd import compute_sentence_scores as S
    from bayeslms_amd.incremental import IncrementalLM
    m, mtype, vocab, nbest = _scorer_model("tlm_ffn")
    m = m.to(dev).eval()
    seed, NS = 4242, 8
    _, unc = S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=NS, seed=seed, uncertainty=True)
    H = max(len(h) for h in nbest.values())
    lm = IncrementalLM(m, max_streams=H, max_len=64, mc_samples=NS, seed=seed)
    tokens = 0
    for key, hv in unc.items():
        xs, ts = zip(*(S.get_input_and_target(hyp, vocab) for hyp, _ in hv))
        L = max(len(x) for x in xs)
        ids = torch.zeros(L, len(xs), dtype=torch.int64)
        tg = torch.zeros(L, len(xs), dtype=torch.int64)
        for j, (x, t) in enumerate(zip(xs, ts)):
            ids[:len(x), j] = torch.tensor(x)
            tg[:len(t), j] = torch.tensor(t)
        nll, rec = lm.step(lm.start(len(xs)), ids, n_new=[len(x) for x in xs], all_positions=True, targets=tg, return_uncertainty=True)
        nll, hp, mi = nll.cpu().numpy(), rec.h_pred.cpu().numpy(), rec.mi.cpu().numpy()
        for j, (_, u) in enumerate(hv):
            n = len(xs[j])
            assert len(u.bma_nll) == n
            for name, a, b in (("bma_nll", nll[:n, j], u.bma_nll), ("h_pred", hp[:n, j], u.h_pred), ("mi", mi[:n, j], u.mi)):
                assert np.all(np.abs(a - b) <= 1e-4 * np.maximum(1.0, np.abs(b))), (key, j, name, a, b)
            assert np.all(np.isnan(nll[n:, j]))
            tokens += n
    assert tokens >= 20


@pytest.mark.parametrize("kind", ["transformer", "lstm"])
def test_beams_prune_fork_continue(dev, kind):
    """reorder with repeats and drops, then continue: every surviving stream equals a fresh stream fed its whole history, sample
    by sample (nll_s column s of a stream still comes from cache slice s -- the columns differ visibly from one another, so a
    slice paired with another sample's weights would show); the consumed state raises."""
    from bayeslms_amd import model as M
    from bayeslms_amd.incremental import IncrementalLM
    torch.manual_seed(9)
    if kind == "transformer":
        V = 97
        m = M.BayesTransformerModel(V, 64, 4, 128, 2, 0.1, True, "MHA")
    else:
        V = 120
        m = M.BayesRNNModel("LSTM", V, 64, 64, 2, 0.2, True, 3)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "lgstd" in k:
                p.add_(1.5)
    m = m.to(dev).eval()
    S = 4
    rng = np.random.default_rng(0)
    N = 5
    hist = torch.randint(0, V, (6, N), device=dev)
    lm = IncrementalLM(m, max_streams=8, max_len=32, mc_samples=S, seed=77)
    st = lm.start(N)
    lens = [6, 3, 5, 6, 1]
    lm.step(st, hist, n_new=lens)
    hs = [hist[:lens[n], n] for n in range(N)]
    for _ in range(3):
        idx = rng.integers(0, st.n, size=int(rng.integers(2, 9)))  # forks (repeats) and prunes
        st = lm.reorder(st, torch.tensor(idx))
        hs = [hs[i] for i in idx]
        assert st.lengths == [len(h) for h in hs]
        nxt = torch.randint(0, V, (st.n,), device=dev)
        lp = lm.step(st, nxt)
        hs = [torch.cat([h, nxt[j:j + 1]]) for j, h in enumerate(hs)]
    fresh = lm.start(len(hs))
    L = max(len(h) for h in hs)
    pad = torch.zeros(L, len(hs), dtype=torch.int64, device=dev)
    for j, h in enumerate(hs):
        pad[:len(h), j] = h
    ref = lm.step(fresh, pad, n_new=[len(h) for h in hs])
    _near("after reorder", lp, ref)
    tg, tg2 = torch.randint(0, V, (st.n,), device=dev), torch.randint(0, V, (st.n,), device=dev)
    nll_a, ua = lm.step(st, tg, targets=tg2, return_uncertainty=True)
    nll_b, ub = lm.step(fresh, tg, targets=tg2, return_uncertainty=True)
    _near("bma_nll", nll_a, nll_b)
    for s in range(S):
        _near("nll_s column %d" % s, ua.nll_s[:, s], ub.nll_s[:, s])
        for s2 in range(s):  # far beyond the tolerance: a swapped pair of slices would not pass the line above
            assert float((ub.nll_s[:, s] - ub.nll_s[:, s2]).abs().max()) > 1e-2
    old = st
    st = lm.reorder(st, [0])
    with pytest.raises(BayesLMError, match="consumed"):
        lm.step(old, tg[:1])


def test_default_path_is_untouched(dev):
    from bayeslms_amd.incremental import IncrementalLM
    for kind in ("tlm_ffn", "lstm_bayes3"):
        m, mtype, V = _model(kind, dev)
        src = torch.randint(0, V, (6, 3), device=dev)
        outs = []
        for kw in ({}, {}, {"mc_samples": 0}, {"mc_samples": 0, "seed": 5}):
            lm = IncrementalLM(m, max_streams=4, max_len=16, **kw)
            st = lm.start(3)
            a = lm.step(st, src[:4], n_new=[4, 2, 3], all_positions=True)
            st = lm.reorder(st, [2, 0, 0])
            outs.append((a, lm.step(st, src[4]), lm.step(st, src[5], targets=src[0])))
        for o in outs[1:]:
            for u, v in zip(outs[0], o):
                assert torch.equal(torch.nan_to_num(u, nan=-1.0), torch.nan_to_num(v, nan=-1.0))
                assert torch.equal(torch.isnan(u), torch.isnan(v))


# ---------------------------------------------------------------------------------------------------------------------- CLI
def _run_cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "bayeslms_amd.generate"] + args, capture_output=True, text=True, timeout=600, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_generate_cli_mc_samples(dev, tmp_path):
    """--mc-samples 4 --write-uncertainty: as many "word h_pred mi" triples as words, the words those of --outf; the same seeds
    give the same text and file; h_pred + 1e-6 >= mi >= -1e-6 (the expected entropy is not negative)."""
    from bayeslms_amd import model as M
    torch.manual_seed(21)
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(38)]
    m = M.BayesTransformerModel(len(words), 32, 2, 64, 2, 0.5, True, "FFN")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k in sd:
        if "lgstd" in k:
            sd[k] += 1.0
    path, voc = str(tmp_path / "model.pt"), tmp_path / "words.txt"
    torch.save(sd, path)
    voc.write_text("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    common = ["--model-path", path, "--vocabulary", str(voc), "--model", "Transformer", "--emsize", "32", "--nhid", "64", "--nlayers", "2",
              "--nhead", "2", "--uncertainty", "Bayesian", "--T_bayes_pos", "FFN", "--words", "7", "--streams", "3", "--seed", "5",
              "--mc-samples", "4", "--mc-seed", "99", "--prompt", "w3 w7"]
    files = []
    for tag in ("a", "b"):
        o, u = tmp_path / ("g%s.txt" % tag), tmp_path / ("u%s.txt" % tag)
        _run_cli(common + ["--outf", str(o), "--write-uncertainty", str(u)])
        files.append((o.read_text(), u.read_text()))
    assert files[0] == files[1]
    text, unc = (f.splitlines() for f in files[0])
    assert len(text) == len(unc) == 3
    for tl, ul in zip(text, unc):
        f = ul.split(" ")
        assert len(tl.split()) == 7 and len(f) == 3 * 7
        assert f[0::3] == tl.split()
        for hp, mi in zip(f[1::3], f[2::3]):
            hp, mi = float(hp), float(mi)
            assert math.isfinite(hp) and hp + 1e-6 >= mi >= -1e-6
    o = tmp_path / "greedy.txt"
    _run_cli(common + ["--temperature", "0", "--outf", str(o)])  # greedy on the model average, no uncertainty file
    assert all(len(line.split()) == 7 for line in o.read_text().splitlines())
