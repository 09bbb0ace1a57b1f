"""GPU: token-level predictive uncertainty from Monte-Carlo weight samples (blm_linear_mc_stats, ops.linear_mc_stats, the
scorer's uncertainty=True and --write-uncertainty) against float64 torch computations of the materialised logits."""
import collections
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _ops():
    from bayeslms_amd import ops
    return ops


def _want(x, w, b, tgt, chunk=256):
    """float64 reference over the materialised logits: x (S, M, K) -> (nll_s (M, S), bma_nll, h_pred, mi)."""
    S, M, _ = x.shape
    V = w.shape[0]
    wd = w.double()
    bd = b.double() if b is not None else torch.zeros(V, dtype=torch.float64, device=w.device)
    out = [[], [], [], []]
    for a in range(0, M, chunk):
        xs = x[:, a:a + chunk].double()
        t = tgt[a:a + chunk]
        lp = torch.log_softmax(xs @ wd.t() + bd, -1)                       # (S, m, V)
        lpbar = torch.logsumexp(lp, 0) - math.log(S)                        # (m, V)
        ok = (t >= 0) & (t < V)
        tc = t.clamp(0, V - 1)
        nll_s = -lp.gather(2, tc.view(1, -1, 1).expand(S, -1, 1)).squeeze(2).t()
        bma = -lpbar.gather(1, tc.view(-1, 1)).squeeze(1)
        nll_s[~ok] = float("nan")
        bma[~ok] = float("nan")
        out[0].append(nll_s)
        out[1].append(bma)
        out[2].append(-(lpbar.exp() * lpbar).sum(-1))
        out[3].append((lp.exp() * (lp - lpbar)).sum(-1).mean(0))
    return [torch.cat(o) for o in out]


def _inputs(dev, M, S, V, K, spread=0.5, seed=0):
    g = torch.Generator(device=dev).manual_seed(M + S + V + K + seed)
    base = torch.randn(M, K, device=dev, generator=g)
    x = base + spread * torch.randn(S, M, K, device=dev, generator=g)  # S related samples of each token's decoder input
    w = torch.randn(V, K, device=dev, generator=g) * (4.0 / K ** 0.5)
    b = torch.randn(V, device=dev, generator=g)
    tgt = torch.randint(0, V, (M,), device=dev, generator=g)
    tgt[0], tgt[-1] = V - 1, 0
    return x, w, b, tgt


def _check(got, want):
    nll_s, bma, h, mi = (t.double() for t in got)
    wn, wb, wh, wm = want
    for name, g, w in (("nll_s", nll_s, wn), ("bma_nll", bma, wb), ("h_pred", h, wh)):  # element-wise: 2e-5 max(1, |want|)
        err = (g - w).abs() - 2e-5 * w.abs().clamp(min=1.0)
        assert float(err.max()) <= 0.0, (name, float((g - w).abs().max()))
    assert bool(((mi - wm).abs() <= 1e-5 + 1e-4 * wm).all()), float((mi - wm).abs().max())
    assert float(mi.min()) >= -1e-6


@pytest.mark.parametrize("M,S,V,K", [(2048, 8, 33000, 512), (700, 4, 33278, 1024), (77, 3, 1000, 60), (129, 16, 260, 33),
                                     (5, 1, 52, 18), (2, 64, 8, 4), (33, 5, 1001, 64)])
def test_mc_stats_equal_float64_of_the_materialised_logits(dev, M, S, V, K):
    """Every plan tile where it is legal (the guarded kernel for K % 4 != 0): per-sample NLL, model-average NLL, predictive
    entropy and mutual information against log_softmax of the fp64 logits; V % 4 != 0 runs on the padded decoder copy."""
    from bayeslms_amd import _lib as L
    ops = _ops()
    x, w, b, tgt = _inputs(dev, M, S, V, K)
    want = _want(x, w, b, tgt)
    tiles = (0,) if (K % 4 or V < 64) else (0, 11, 12, 21, 22, 28)
    for tile in tiles:
        L.check(L.lib().blm_gemm_plan_override(tile, 0), "override")
        try:
            with torch.no_grad():
                got = ops.linear_mc_stats(x, w, b, tgt)
        finally:
            L.check(L.lib().blm_gemm_plan_override(0, 0), "override")
        assert got.nll_s.shape == (M, S) and got.mi.shape == (M,)
        _check(got, want)
    with torch.no_grad():  # no bias
        _check(ops.linear_mc_stats(x, w, None, tgt, S=S), _want(x, w, None, tgt))


def test_decoders_in_turn_are_never_mixed_up(dev):
    """Two same-shape decoders over an odd vocabulary (each call pads its own copy), one of them changed in place through .data
    between calls, and a run-scoped McDecoder: every result is that of the weights the call was given."""
    ops = _ops()
    M, S, V, K = 96, 4, 1001, 64
    x, w1, b1, tgt = _inputs(dev, M, S, V, K)
    _, w2, b2, _ = _inputs(dev, M, S, V, K, seed=1)
    with torch.no_grad():
        for w, b in ((w1, b1), (w2, b2), (w1, b1)):
            _check(ops.linear_mc_stats(x, w, b, tgt), _want(x, w, b, tgt))
        w1.data.mul_(0.5)
        b1.data.add_(1.0)
        _check(ops.linear_mc_stats(x, w1, b1, tgt), _want(x, w1, b1, tgt))
        dec = ops.McDecoder(w2, b2)
        _check(ops.linear_mc_stats(x, w2, b2, tgt, dec=dec), _want(x, w2, b2, tgt))
        with pytest.raises(ValueError, match="another decoder"):
            ops.linear_mc_stats(x, w1, b1, tgt, dec=dec)


def test_identical_samples_carry_no_mutual_information(dev):
    ops = _ops()
    M, S, V, K = 300, 8, 5000, 128
    x, w, b, tgt = _inputs(dev, M, S, V, K)
    x = x[:1].expand(S, -1, -1).contiguous()
    with torch.no_grad():
        got = ops.linear_mc_stats(x, w, b, tgt)
    assert float(got.mi.max()) <= 1e-6
    lp = torch.log_softmax(x[0].double() @ w.double().t() + b.double(), -1)
    h1 = -(lp.exp() * lp).sum(-1)
    assert float((got.h_pred.double() - h1).abs().max()) < 2e-5 * max(1.0, float(h1.max()))


def test_one_sample_is_linear_nll(dev):
    ops = _ops()
    M, V, K = 1000, 4096, 256
    x, w, b, tgt = _inputs(dev, M, 1, V, K)
    with torch.no_grad():
        got = ops.linear_mc_stats(x, w, b, tgt)
        ref = ops.linear_nll(x[0], w, b, tgt)
    tol = 1e-6 * max(1.0, float(ref.abs().max()))
    assert float((got.nll_s[:, 0] - ref).abs().max()) <= tol
    assert float((got.bma_nll - ref).abs().max()) <= tol


def test_large_logits_stay_finite(dev):
    ops = _ops()
    x, w, b, tgt = _inputs(dev, 200, 6, 3000, 64)
    with torch.no_grad():
        got = ops.linear_mc_stats(50.0 * x, w, 50.0 * b, tgt)
    for t in got:
        assert bool(torch.isfinite(t).all())
    assert float(got.mi.min()) >= -1e-6


def test_out_of_range_target_is_nan_for_that_token_only(dev):
    ops = _ops()
    M, S, V = 64, 4, 1001
    x, w, b, tgt = _inputs(dev, M, S, V, 32)
    tgt[5], tgt[9], tgt[11] = V, -1, 1003  # 1003 < the padded vocabulary 1004: still outside [0, V)
    with torch.no_grad():
        got = ops.linear_mc_stats(x, w, b, tgt)
    bad = torch.zeros(M, dtype=torch.bool, device=dev)
    bad[[5, 9, 11]] = True
    assert bool(torch.isnan(got.bma_nll[bad]).all()) and bool(torch.isnan(got.nll_s[bad]).all())
    assert bool(torch.isfinite(got.bma_nll[~bad]).all()) and bool(torch.isfinite(got.nll_s[~bad]).all())
    assert bool(torch.isfinite(got.h_pred).all()) and bool(torch.isfinite(got.mi).all())


def test_bit_identical_run_to_run_and_inference_only(dev):
    ops = _ops()
    x, w, b, tgt = _inputs(dev, 513, 8, 7000, 256)
    with torch.no_grad():
        a = ops.linear_mc_stats(x, w, b, tgt)
        c = ops.linear_mc_stats(x, w, b, tgt)
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    with pytest.raises(Exception, match="inference-only"):
        ops.linear_mc_stats(x.clone().requires_grad_(True), w, b, tgt)


# ---- scorer ------------------------------------------------------------------------------------------------------------
def _nbest(g):
    vocab = {w: i for i, w in enumerate(g["words"])}
    nbest = collections.OrderedDict()
    for line in str(g["nbest_txt"]).splitlines():
        parts = line.strip().split(' ', 1)
        key, hyp = (parts[0], parts[1]) if len(parts) == 2 else (line.strip(), ' ')
        nbest.setdefault(key.rsplit('-', 1)[0], []).append(hyp)
    return vocab, nbest


def _scorer_model(kind):
    from bayeslms_amd import model as M
    if kind == "tlm_gauss3":  # BASELINE configs[4]'s family, built as test_mc_sample_scoring_gp_and_variational_families does
        g, _, _ = load_golden("scorer_tlm_ffn")
        vocab, nbest = _nbest(g)
        torch.manual_seed(31)
        m = M.GaussTransformerModel(len(vocab), 16, 4, 32, 2, 0.5, True, 3)
        with torch.no_grad():
            for k, p in m.named_parameters():
                if "lgstd" in k:
                    p.add_(1.0)
        return m, "Transformer", vocab, nbest
    g, sd, _ = load_golden("scorer_" + kind)
    vocab, nbest = _nbest(g)
    V = len(vocab)
    if kind == "tlm_ffn":
        m, mtype = M.BayesTransformerModel(V, 16, 4, 32, 2, 0.5, True, "FFN"), "Transformer"
    else:
        m, mtype = M.BayesRNNModel("LSTM", V, 12, 12, 2, 0.5, True, 3), "LSTM"
    own = m.state_dict()
    own.update({k: v for k, v in sd.items() if k in own and tuple(v.shape) == tuple(own[k].shape)})
    m.load_state_dict(own)
    return m, mtype, vocab, nbest


def _flat(unc):
    return [(k, n, u) for k, hv in unc.items() for n, (_, u) in enumerate(hv, 1)]


@pytest.mark.parametrize("kind", ["tlm_ffn", "lstm_bayes3", "tlm_gauss3"])
def test_scorer_uncertainty(dev, kind):
    """uncertainty=True leaves the scores as they are (1e-5 relative), does not depend on the batch packing, and -- for the
    Transformers -- each hypothesis' per-token h_pred / mi equal a float64 computation from that hypothesis alone (B = 1, no
    packing, the decoder's logits materialised, model.set_step(s) per sample)."""
    from bayeslms_amd import compute_sentence_scores as S
    from bayeslms_amd.model import variational_sites
    m, mtype, vocab, nbest = _scorer_model(kind)
    m = m.to(dev)
    seed, NS = 4242, 8
    base = S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=NS, seed=seed)
    runs = {}
    for bt in (8192, 16):
        sc, unc = S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=NS, seed=seed, batch_tokens=bt, uncertainty=True)
        assert list(sc) == list(base) == list(unc)
        for key in base:
            assert [h for h, _ in sc[key]] == [h for h, _ in base[key]] == [h for h, _ in unc[key]]
            for (_, a), (_, b) in zip(sc[key], base[key]):
                assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (bt, key, a, b)
        runs[bt] = unc
    hyps = 0
    for (k1, n1, u), (k2, n2, v) in zip(_flat(runs[8192]), _flat(runs[16])):
        assert (k1, n1) == (k2, n2)
        assert len(u.mi) == len(v.mi) >= 1
        for f in ("bma_nll", "h_pred", "mi"):
            a, b = getattr(u, f), getattr(v, f)
            assert np.all(np.abs(a - b) <= 1e-5 + 1e-5 * np.abs(b)), (f, k1, n1, a, b)
        assert abs(u.sent_logp_std - v.sent_logp_std) <= 1e-5 * max(1.0, v.sent_logp_std)
        assert np.all(np.isfinite(u.h_pred)) and np.all(u.mi >= -1e-6)
        hyps += 1
    assert hyps == sum(len(h) for h in base.values())
    assert any(float(np.sum(u.mi)) > 1e-6 for _, _, u in _flat(runs[8192]))  # the samples disagree somewhere
    if mtype != "Transformer":
        return
    # float64 from each hypothesis alone, in the scorer's sampling state (training mode, dropout off, sample flags raised)
    raised = [s for s in variational_sites(m) if getattr(s, "sample", True) is False]
    for s in raised:
        s.sample = True
    m.train()
    m.noise_state.dropout_off = True
    m.set_seed(seed)
    try:
        with torch.no_grad():
            for key, hv in runs[8192].items():
                for hyp, u in hv:
                    x, t = S.get_input_and_target(hyp, vocab)
                    data = torch.as_tensor(x, dtype=torch.int64, device=dev).view(-1, 1)
                    lps = []
                    for smp in range(NS):
                        m.set_step(smp)
                        lps.append(torch.log_softmax(m(data).reshape(len(x), -1).double(), -1))
                    lp = torch.stack(lps)
                    lpbar = torch.logsumexp(lp, 0) - math.log(NS)
                    h = (-(lpbar.exp() * lpbar).sum(-1)).cpu().numpy()
                    mi = (lp.exp() * (lp - lpbar)).sum(-1).mean(0).cpu().numpy()
                    bma = (-lpbar.gather(1, torch.as_tensor(t, device=dev).view(-1, 1)).squeeze(1)).cpu().numpy()
                    assert np.all(np.abs(u.h_pred - h) <= 1e-4 * np.maximum(1.0, np.abs(h))), (key, hyp)
                    assert np.all(np.abs(u.mi - mi) <= 1e-4 * np.maximum(1.0, np.abs(mi))), (key, hyp)
                    assert np.all(np.abs(u.bma_nll - bma) <= 1e-4 * np.maximum(1.0, np.abs(bma))), (key, hyp)
    finally:
        m.noise_state.dropout_off = False
        m.eval()
        for s in raised:
            s.sample = False


def test_scorer_uncertainty_refuses_two_models(dev):
    from bayeslms_amd import compute_sentence_scores as S
    from bayeslms_amd._lib import BayesLMError
    m, mtype, vocab, nbest = _scorer_model("tlm_ffn")
    m = m.to(dev)
    with pytest.raises(BayesLMError, match="one model"):
        S.compute_scores_batched(nbest, m, vocab, mtype, dev, model_2=m, alpha=0.5, mc_samples=4, uncertainty=True)
    with pytest.raises(BayesLMError, match="mc-samples >= 2"):
        S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=1, uncertainty=True)


def test_cli_write_uncertainty_end_to_end(dev, tmp_path):
    """--mc-samples 8 --write-uncertainty on a scorer fixture model: one line per hypothesis in the score file's order, every value
    finite, sum_mi >= 0; the score file equals the one written without the flag (1e-5 relative, or one unit of its %.4f)."""
    from bayeslms_amd import compute_sentence_scores as S
    from oracle import bayes_oracle as O
    g, sd, _ = load_golden("scorer_tlm_ffn")
    d = str(tmp_path)
    with open(os.path.join(d, "words.txt"), "w") as f:
        f.write("".join("%s %d\n" % (w, i) for i, w in enumerate(g["words"])))
    with open(os.path.join(d, "nbest.txt"), "w") as f:
        f.write(str(g["nbest_txt"]))
    full = dict(sd)
    full["pos_encoder.pe"] = O.positional_table(5000, full["encoder.weight"].shape[1])
    torch.save(full, os.path.join(d, "model.pt"))
    argv = ["--nbest-list", os.path.join(d, "nbest.txt"), "--vocabulary", os.path.join(d, "words.txt"),
            "--model-path", os.path.join(d, "model.pt"), "--mc-samples", "8"] + [str(a) for a in g["argv"]]
    S.main(argv + ["--outfile", os.path.join(d, "plain.txt")])
    S.main(argv + ["--outfile", os.path.join(d, "with.txt"), "--write-uncertainty", os.path.join(d, "unc.txt")])
    plain = [ln.split() for ln in open(os.path.join(d, "plain.txt")).read().splitlines()]
    withu = [ln.split() for ln in open(os.path.join(d, "with.txt")).read().splitlines()]
    unc = [ln.split() for ln in open(os.path.join(d, "unc.txt")).read().splitlines()]
    assert len(plain) == len(withu) == len(unc) == len(str(g["nbest_txt"]).splitlines())
    assert [a[0] for a in unc] == [a[0] for a in withu] == [a[0] for a in plain]
    for a, b in zip(withu, plain):
        assert abs(float(a[1]) - float(b[1])) <= max(1e-5 * abs(float(b[1])), 1.0001e-4), (a, b)
    for row, sc in zip(unc, withu):
        assert len(row) == 7 and row[1] == sc[1]
        vals = [float(v) for v in row[1:]]
        assert all(math.isfinite(v) for v in vals)
        assert vals[4] >= 0.0 and int(row[6]) >= 1
