"""GPU: n-best rescoring over prefix tries -- blm_attn_fwd_tree against a float64 masked softmax, blm_linear_nll_edges (one model and
interpolated) against float64 log_softmax, compute_scores_batched(share_prefixes=True) against the padded path, and the scorer CLI
with --share-prefixes 1 against the reference's score files."""
import math
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _trie_of(utts, rng_seed=0):
    """utts: [[hypothesis id lists]] -> (end, lo) int32 numpy arrays of their prefix tries (bayeslms_amd.prefix_trie)."""
    from bayeslms_amd.prefix_trie import build_trie
    cols, utt = [], []
    for u, hyps in enumerate(utts):
        for h in hyps:
            cols.append([0] + list(h))
            utt.append(u)
    lens = np.array([len(x) for x in cols])
    data = np.zeros((lens.max(), len(cols)), dtype=np.int64)
    for n, x in enumerate(cols):
        data[: len(x), n] = x
    tr = build_trie(data, lens, np.zeros(int(lens.sum()), dtype=np.int64), np.asarray(utt))
    return tr.end, tr.lo


def _random_utts(rng, n_utt, n_hyp, base_len, vocab=30, share=0.7):
    utts = []
    for _ in range(n_utt):
        base = list(rng.integers(1, vocab, size=base_len))
        hyps = []
        for _ in range(int(rng.integers(1, n_hyp + 1))):
            cut = int(rng.integers(0, base_len + 1)) if rng.random() > share else int(rng.integers(base_len // 2, base_len + 1))
            hyps.append(base[:cut] + list(rng.integers(1, vocab, size=int(rng.integers(0, 4)))))
        utts.append(hyps)
    return utts


def _tree_ref(q, k, v, end, lo, nhead):
    """float64 masked softmax: row i attends row j iff lo[i] <= j <= i and end[j] > i."""
    R, d = q.shape
    hd = d // nhead
    i = torch.arange(R).view(-1, 1)
    j = torch.arange(R).view(1, -1)
    e = torch.as_tensor(end, dtype=torch.int64).view(1, -1)
    lw = torch.as_tensor(lo, dtype=torch.int64).view(-1, 1)
    ok = ((j >= lw) & (j <= i) & (e > i)).to(q.device)
    qd, kd, vd = (t.double().view(R, nhead, hd).transpose(0, 1) for t in (q, k, v))
    s = qd @ kd.transpose(1, 2) / math.sqrt(hd)
    s = s.masked_fill(~ok, float("-inf"))
    return (torch.softmax(s, -1) @ vd).transpose(0, 1).reshape(R, d)


def _tree_attn(q, k, v, ld, end, lo, nhead, hd):
    from bayeslms_amd import _lib as L
    R = end.shape[0]
    out = torch.empty(R, nhead * hd, device=q.device, dtype=torch.float32)
    e = torch.as_tensor(end, dtype=torch.int32).to(q.device)
    lw = torch.as_tensor(lo, dtype=torch.int32).to(q.device)
    L.check(L.lib().blm_attn_fwd_tree(q.data_ptr(), k.data_ptr(), v.data_ptr(), ld, out.data_ptr(), e.data_ptr(), lw.data_ptr(), R, nhead,
                                      hd, None), "blm_attn_fwd_tree")
    torch.cuda.synchronize()
    return out


def _layouts():
    """(name, utts) covering R in {1, 31, 128, 129, 1000+}, utterances across 128-row blocks, one utterance over 1000 nodes."""
    rng = np.random.default_rng(11)
    out = [("one_node", [[[]]])]
    out.append(("r31", [[list(range(1, 31))]]))  # one chain of 31 nodes
    u = _random_utts(rng, 40, 6, 8)
    out.append(("many_utts", u))
    big = [[list(rng.integers(1, 400, size=int(rng.integers(5, 25)))) for _ in range(80)]]
    out.append(("one_big_utt", big))
    out.append(("mixed", _random_utts(rng, 7, 20, 14, share=0.9) + big + _random_utts(rng, 5, 3, 4)))
    return out


def _exact_rows(R_target):
    """a layout of exactly R_target nodes: one chain per utterance of 10 tokens (+ the rest)."""
    utts, left = [], R_target
    while left > 0:
        n = min(left, 11)
        utts.append([list(range(1, n))])
        left -= n
    return utts


@pytest.mark.parametrize("hd", [64, 32, 100, 128])
@pytest.mark.parametrize("layout", [n for n, _ in _layouts()] + ["r128", "r129"])
@pytest.mark.parametrize("fused", [True, False])
def test_tree_attention_equals_float64_masked_softmax(dev, hd, layout, fused):
    utts = {"r128": _exact_rows(128), "r129": _exact_rows(129)}.get(layout) or dict(_layouts())[layout]
    end, lo = _trie_of(utts)
    R = end.shape[0]
    if layout in ("r128", "r129"):
        assert R == int(layout[1:])
    nhead = 2 if hd != 32 else 4
    d = nhead * hd
    g = torch.Generator(device=dev).manual_seed(R + hd)
    if fused:
        qkv = torch.randn(R, 3 * d, device=dev, generator=g)
        q, k, v, ld = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], 3 * d
    else:
        q, k, v = (torch.randn(R, d, device=dev, generator=g) for _ in range(3))
        ld = d
    got = _tree_attn(q, k, v, ld, end, lo, nhead, hd)
    want = _tree_ref(q, k, v, end, lo, nhead)
    assert torch.isfinite(got).all()
    assert float((got.double() - want).abs().max()) < 2e-5 * max(1.0, float(want.abs().max())), (layout, hd)


@pytest.mark.parametrize("hd", [64, 32])
def test_tree_attention_on_chain_tries_equals_causal_attention(dev, hd):
    """One hypothesis per utterance: the tree mask is the causal mask of each chain -- blm_attn_fwd on the causal layout."""
    from bayeslms_amd import _lib as L
    T, B, nhead = 37, 6, 2
    d = nhead * hd
    g = torch.Generator(device=dev).manual_seed(hd)
    qkv = torch.randn(T, B, 3 * d, device=dev, generator=g)
    causal = torch.empty(T, B, d, device=dev)
    L.check(L.lib().blm_attn_fwd(qkv.data_ptr(), qkv[..., d:].data_ptr(), qkv[..., 2 * d:].data_ptr(), 3 * d, causal.data_ptr(), None,
                                 T, B, nhead, hd, 0.0, None, 0, B, None), "blm_attn_fwd")
    rows = qkv.transpose(0, 1).reshape(T * B, 3 * d).contiguous()  # column-major chains: utterance b = rows b*T .. b*T + T-1
    end = np.repeat((np.arange(B) + 1) * T, T).astype(np.int32)
    lo = np.repeat(np.arange(B) * T, T).astype(np.int32)
    got = _tree_attn(rows, rows[:, d:], rows[:, 2 * d:], 3 * d, end, lo, nhead, hd)
    want = causal.transpose(0, 1).reshape(T * B, d)
    assert float((got - want).abs().max()) < 1e-5 * max(1.0, float(want.abs().max()))


def test_tree_attention_valu_form_at_head_dim_64_and_determinism(dev):
    """Option "attn_valu" routes head_dim 64 to the vector-ALU tree kernel: both forms agree; deterministic mode repeats bit for bit."""
    from bayeslms_amd import _lib as L, ops
    end, lo = _trie_of(dict(_layouts())["mixed"])
    R, nhead, hd = end.shape[0], 4, 64
    g = torch.Generator(device=dev).manual_seed(5)
    qkv = torch.randn(R, 3 * nhead * hd, device=dev, generator=g)
    d = nhead * hd
    a = _tree_attn(qkv, qkv[:, d:], qkv[:, 2 * d:], 3 * d, end, lo, nhead, hd)
    L.check(L.lib().blm_set_option(b"attn_valu", 1), "attn_valu")
    try:
        b = _tree_attn(qkv, qkv[:, d:], qkv[:, 2 * d:], 3 * d, end, lo, nhead, hd)
    finally:
        L.check(L.lib().blm_set_option(b"attn_valu", 0), "attn_valu")
    assert float((a - b).abs().max()) < 2e-5 * max(1.0, float(a.abs().max()))
    ops.set_deterministic(True)
    try:
        c = _tree_attn(qkv, qkv[:, d:], qkv[:, 2 * d:], 3 * d, end, lo, nhead, hd)
        assert torch.equal(a, c)
    finally:
        ops.set_deterministic(False)


# ---------------------------------------------------------------------------------------------------------------- edge NLL
def _edge_case(dev, M, V, K, per_node, seed=0):
    g = torch.Generator(device=dev).manual_seed(M + V + K + seed)
    x = torch.randn(M, K, device=dev, generator=g)
    w = torch.randn(V, K, device=dev, generator=g) * (4.0 / K ** 0.5)
    b = torch.randn(V, device=dev, generator=g)
    rng = np.random.default_rng(M + V)
    pairs = set()
    for n in range(M):
        for t in rng.integers(0, V, size=int(rng.integers(1, per_node + 1))):
            pairs.add((n, int(t)))
    pairs.add((0, V - 1))
    pairs.add((M - 1, 0))
    en, et = (torch.tensor(c, dtype=torch.int64, device=dev) for c in zip(*sorted(pairs)))
    return x, w, b, en, et


def _edge_want(x, w, b, en, et):
    lp = torch.log_softmax(x.double() @ w.double().t() + (b.double() if b is not None else 0), 1)
    return -lp[en, et]


@pytest.mark.parametrize("M,V,K,per_node", [(300, 33000, 512, 3), (100, 33278, 256, 4), (77, 97, 64, 6), (9, 8, 12, 3),
                                           (1, 8, 4, 8), (513, 1000, 36, 2)])
@pytest.mark.parametrize("with_bias", [True, False])
def test_linear_nll_edges_equals_log_softmax(dev, M, V, K, per_node, with_bias):
    from bayeslms_amd import _lib as L, ops
    x, w, b, en, et = _edge_case(dev, M, V, K, per_node)
    b = b if with_bias else None
    want = _edge_want(x, w, b, en, et)
    dec = ops.McDecoder(w, b)  # pads an odd vocabulary once
    tiles = (0,) if (K % 4 or V < 64) else (0, 11, 12, 21, 22, 28)
    for tile in tiles:
        L.check(L.lib().blm_gemm_plan_override(tile, 0), "override")
        try:
            with torch.no_grad():
                got = ops.linear_nll_edges(x, dec, en, et)
        finally:
            L.check(L.lib().blm_gemm_plan_override(0, 0), "override")
        assert float(((got.double() - want).abs() / want.abs().clamp(min=1.0)).max()) < 2e-5, tile
    with pytest.raises(Exception, match="inference-only"):
        ops.linear_nll_edges(x.clone().requires_grad_(True), dec, en, et)


def test_linear_nll_edges_out_of_range_edges_give_nan_and_determinism(dev):
    from bayeslms_amd import ops
    x, w, b, en, et = _edge_case(dev, 50, 1000, 64, 3)
    dec = ops.McDecoder(w, b)
    en2, et2 = en.clone(), et.clone()
    en2[1], et2[2] = 50, 1000
    with torch.no_grad():
        got = ops.linear_nll_edges(x, dec, en2, et2)
    assert torch.isnan(got[1]) and torch.isnan(got[2]) and torch.isfinite(got[3:]).all()
    ops.set_deterministic(True)
    try:
        with torch.no_grad():
            a, c = ops.linear_nll_edges(x, dec, en, et), ops.linear_nll_edges(x, dec, en, et)
        assert torch.equal(a, c)
    finally:
        ops.set_deterministic(False)


@pytest.mark.parametrize("M,V,K1,K2,alpha", [(300, 33000, 512, 256, 0.8), (77, 33278, 64, 32, 0.3), (20, 97, 16, 12, 0.5), (5, 8, 4, 8, 1.0)])
def test_linear_nll_interp_edges_equals_log_softmax(dev, M, V, K1, K2, alpha):
    from bayeslms_amd import ops
    x1, w1, b1, en, et = _edge_case(dev, M, V, K1, 3)
    x2, w2, b2, _, _ = _edge_case(dev, M, V, K2, 3, seed=1)
    logits = alpha * (x1.double() @ w1.double().t() + b1.double()) + (1 - alpha) * (x2.double() @ w2.double().t() + b2.double())
    want = -torch.log_softmax(logits, 1)[en, et]
    dec = ops.InterpDecoder(w1, b1, w2, b2, alpha)
    with torch.no_grad():
        for _ in range(2):  # packs the weights, then reuses them
            got = ops.linear_nll_interp_edges(x1, x2, dec, en, et)
            assert float(((got.double() - want).abs() / want.abs().clamp(min=1.0)).max()) < 2e-5
    assert dec.packed


# ---------------------------------------------------------------------------------------------------------------- scorer
def _shared_nbest(V, n_utt=9, seed=5):
    """heavily prefix-shared n-best lists: a base sentence, hypotheses diverging late, duplicates, prefixes, an empty one."""
    rnd = random.Random(seed)
    words = ["w%d" % i for i in range(2, V)]
    nbest = OrderedDict()
    for u in range(n_utt):
        base = [rnd.choice(words) for _ in range(rnd.randint(1, 16))]
        hyps = []
        for _ in range(rnd.randint(1, 12)):
            h = list(base)
            r = rnd.random()
            if r < 0.5:
                h = h[: rnd.randint(len(h) // 2, len(h))] + [rnd.choice(words) for _ in range(rnd.randint(0, 3))]
            elif r < 0.6:
                h = h[: rnd.randint(0, len(h))]
            hyps.append(" ".join(h) if h else " ")
        if u % 3 == 0:
            hyps.append(hyps[0])
        nbest["utt%d" % u] = hyps
    return nbest


def _tf_models(M, V, kind):
    return {"plain": lambda: M.TransformerModel(V, 128, 2, 256, 2, 0.5, "gelu", True),
            "bayes_ffn": lambda: M.BayesTransformerModel(V, 128, 2, 256, 2, 0.5, True, "FFN"),
            "bayes_mha": lambda: M.BayesTransformerModel(V, 128, 2, 256, 2, 0.5, True, "MHA"),
            "bayes_emb": lambda: M.BayesTransformerModel(V, 128, 2, 256, 2, 0.5, True, "EMB"),
            "gauss3": lambda: M.GaussTransformerModel(V, 128, 2, 256, 2, 0.5, True, 3),
            "head100": lambda: M.TransformerModel(V, 200, 2, 256, 2, 0.5, "gelu", True)}[kind]()


def _rnn_models(M, V, kind):
    H = 96
    return {"plain": lambda: M.RNNModel("LSTM", V, H, H, 2, 0.5, True),
            "bayes3": lambda: M.BayesRNNModel("LSTM", V, H, H, 2, 0.5, True, 3),
            "gauss33": lambda: M.GaussRNNModel("LSTM", V, H, H, 2, 0.5, False, "33"),
            "variational11": lambda: M.VariationalRNNModel("LSTM", V, H, H, 2, 0.5, True, "11")}[kind]()


def _compare(dev, nbest, m1, model_type, V, m2=None, mc=0, bts=(150, 16384)):
    from bayeslms_amd import compute_sentence_scores as S
    vocab = {"<s>": 0, "<unk>": 1}
    vocab.update({"w%d" % i: i for i in range(2, V)})
    for bt in bts:
        out = []
        for share in (False, True):
            sc = S.compute_scores_batched(nbest, m1, vocab, model_type, dev, model_2=m2, alpha=0.3 if m2 is not None else 0.0,
                                          mc_samples=mc, seed=9, batch_tokens=bt, share_prefixes=share)
            assert list(sc) == list(nbest)
            out.append([s for key in nbest for _, s in sc[key]])
        a, b = np.asarray(out[1]), np.asarray(out[0])
        assert a.shape == b.shape and len(a) == sum(len(h) for h in nbest.values())
        np.testing.assert_allclose(a, b, rtol=2e-5, atol=1e-5, err_msg="batch_tokens %d" % bt)


# Monte-Carlo samples for the models that have variational tensors (plain / head100 have none)
@pytest.mark.parametrize("kind,mode", [(k, m) for k in ("plain", "bayes_ffn", "bayes_mha", "bayes_emb", "gauss3", "head100")
                                       for m in ("mean", "mc", "interp") if not (m == "mc" and k in ("plain", "head100"))])
def test_scorer_share_prefixes_equals_padded_transformer(dev, kind, mode):
    from bayeslms_amd import model as M
    V = 97
    torch.manual_seed(3)
    m1 = _tf_models(M, V, kind).to(dev)
    m2 = _tf_models(M, V, "plain" if kind != "head100" else "head100").to(dev) if mode == "interp" else None
    _compare(dev, _shared_nbest(V), m1, "Transformer", V, m2=m2, mc=4 if mode == "mc" else 0)


@pytest.mark.parametrize("kind,mode", [(k, m) for k in ("plain", "bayes3", "gauss33", "variational11") for m in ("mean", "mc", "interp")
                                       if not (m == "mc" and k == "plain")])
def test_scorer_share_prefixes_equals_padded_lstm(dev, kind, mode):
    from bayeslms_amd import model as M
    V = 97
    torch.manual_seed(4)
    m1 = _rnn_models(M, V, kind).to(dev)
    m2 = _rnn_models(M, V, "plain").to(dev) if mode == "interp" else None
    _compare(dev, _shared_nbest(V, seed=6), m1, "LSTM", V, m2=m2, mc=4 if mode == "mc" else 0, bts=(60, 8192))


def test_scorer_share_prefixes_odd_vocabulary_and_long_utterance(dev):
    """33,278 words (padded decoder), one utterance of 150 hypotheses (a trie over several 128-row blocks)."""
    from bayeslms_amd import model as M
    V = 33278
    torch.manual_seed(5)
    m1 = M.BayesTransformerModel(V, 128, 2, 256, 2, 0.5, True, "FFN").to(dev)
    rnd = random.Random(8)
    nb = _shared_nbest(V, n_utt=3)
    base = ["w%d" % rnd.randint(2, V - 1) for _ in range(20)]
    nb["long"] = [" ".join(base[: rnd.randint(5, 20)] + ["w%d" % rnd.randint(2, V - 1) for _ in range(rnd.randint(0, 4))]) for _ in range(150)]
    _compare(dev, nb, m1, "Transformer", V, bts=(16384,))


def test_scorer_share_prefixes_refusals_and_determinism(dev):
    from bayeslms_amd import compute_sentence_scores as S, model as M, ops
    from bayeslms_amd._lib import BayesLMError
    V = 97
    vocab = {"<s>": 0, "<unk>": 1}
    vocab.update({"w%d" % i: i for i in range(2, V)})
    nb = _shared_nbest(V)
    torch.manual_seed(3)
    vt = M.VTransformerModel(V, 128, 2, 256, 2, 0.5, True, 1).to(dev)
    with pytest.raises(BayesLMError, match="VTransformerModel"):
        S.compute_scores_batched(nb, vt, vocab, "Transformer", dev, share_prefixes=True)
    m = M.BayesTransformerModel(V, 128, 2, 256, 2, 0.5, True, "FFN").to(dev)
    with pytest.raises(BayesLMError, match="share_prefixes"):
        S.compute_scores_batched(nb, m, vocab, "Transformer", dev, mc_samples=4, uncertainty=True, share_prefixes=True)
    ops.set_deterministic(True)
    try:
        a = S.compute_scores_batched(nb, m, vocab, "Transformer", dev, mc_samples=3, share_prefixes=True)
        b = S.compute_scores_batched(nb, m, vocab, "Transformer", dev, mc_samples=3, share_prefixes=True)
        assert a == b
    finally:
        ops.set_deterministic(False)


# ---------------------------------------------------------------------------------------------------------------- CLI vs golden
def _write_corpus(g, d):
    with open(os.path.join(d, "words.txt"), "w") as f:
        f.write("".join("%s %d\n" % (w, i) for i, w in enumerate(g["words"])))
    for s in ("train", "valid", "test"):
        if s + "_txt" in g:
            with open(os.path.join(d, s + ".txt"), "w") as f:
                f.write(str(g[s + "_txt"]))


@pytest.mark.parametrize("tag", ["tlm_ffn", "lstm_bayes3", "tlm_gauss3"])
def test_scorer_cli_share_prefixes_matches_reference_output(dev, tag, tmp_path):
    from bayeslms_amd import compute_sentence_scores as S
    g, sd, _ = load_golden("scorer_" + tag)
    d = str(tmp_path)
    _write_corpus(g, d)
    with open(os.path.join(d, "nbest.txt"), "w") as f:
        f.write(str(g["nbest_txt"]))
    full = dict(sd)
    if "pos_encoder.pe" in full:
        from oracle import bayes_oracle as O
        full["pos_encoder.pe"] = O.positional_table(5000, full["encoder.weight"].shape[1])
    torch.save(full, os.path.join(d, "model.pt"))
    argv = ["--nbest-list", os.path.join(d, "nbest.txt"), "--outfile", os.path.join(d, "out.txt"), "--vocabulary",
            os.path.join(d, "words.txt"), "--model-path", os.path.join(d, "model.pt")] + [str(a) for a in g["argv"]]
    want = [ln.split() for ln in str(g["scores_txt"]).splitlines()]
    S.main(argv + ["--share-prefixes", "1"])
    got = [ln.split() for ln in open(os.path.join(d, "out.txt")).read().splitlines()]
    assert [a[0] for a in got] == [b[0] for b in want]
    for a, b in zip(got, want):
        assert abs(float(a[1]) - float(b[1])) <= 1e-3 * max(1.0, abs(float(b[1]))), (a, b)


@pytest.mark.parametrize("name,ctor", [
    ("scorer_cfg1_from_seed", lambda M, V: M.BayesRNNModel("LSTM", V, 1024, 1024, 2, 0.5, True, 3)),
    ("scorer_cfg2_from_seed", lambda M, V: M.BayesTransformerModel(V, 512, 8, 4096, 6, 0.5, True, "FFN")),
    ("scorer_cfg4_from_seed", lambda M, V: M.GaussTransformerModel(V, 512, 8, 4096, 6, 0.5, True, 3)),
])
def test_scorer_cli_share_prefixes_at_full_size_matches_the_reference_scorer(dev, name, ctor, tmp_path):
    from bayeslms_amd import compute_sentence_scores as S, model as M
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    V, d = int(g["words_n"]), str(tmp_path)
    with open(os.path.join(d, "words.txt"), "w") as f:
        for i, w in enumerate(["<s>", "<unk>"] + ["w%d" % i for i in range(V - 2)]):
            f.write("%s %d\n" % (w, i))
    with open(os.path.join(d, "nbest.txt"), "w") as f:
        f.write(str(g["nbest_txt"]))
    torch.manual_seed(int(g["seed"]))
    torch.save(ctor(M, V).state_dict(), os.path.join(d, "model.pt"))
    argv = ["--nbest-list", os.path.join(d, "nbest.txt"), "--outfile", os.path.join(d, "out.txt"), "--vocabulary",
            os.path.join(d, "words.txt"), "--model-path", os.path.join(d, "model.pt")] + [str(a) for a in g["argv"]]
    want = [ln.split() for ln in str(g["scores_txt"]).splitlines()]
    S.main(argv + ["--share-prefixes", "1"])
    got = [ln.split() for ln in open(os.path.join(d, "out.txt")).read().splitlines()]
    assert [a[0] for a in got] == [b[0] for b in want]
    for a, b in zip(got, want):
        assert abs(float(a[1]) - float(b[1])) / max(1.0, abs(float(b[1]))) <= 1e-3, (a, b)
