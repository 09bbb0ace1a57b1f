"""GPU parity of whole models through the reference's class surface against the golden vectors
the reference produced (tests/golden/*.npz): logits, per-token NLL, loss, KL and every parameter
gradient, with eps injected and dropout 0 (SURVEY.md 8(d) parity gates, 1e-3 relative bar)."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-4  # well inside the 1e-3 bar of BASELINE.json


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def grad_close(a, b, rtol=5e-4, atol=1e-7):
    """Gradients that are analytically zero (a key-projection bias under softmax) are ~1e-10 noise
    on both sides: compare with an absolute floor."""
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max()) <= rtol * float(b.abs().max()) + atol


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def zero_dropout(m):
    for mod in m.modules():
        if hasattr(mod, "p"):
            mod.p = 0.0
        if isinstance(getattr(mod, "dropout", None), float):
            mod.dropout = 0.0


def load_sd(model, sd):
    """Checkpoint interchange: the golden state_dict (reference key names) loads strictly, except
    that the fixture keeps only the first 64 rows of the deterministic positional table."""
    own = model.state_dict()
    assert set(own.keys()) == set(sd.keys()), set(own.keys()) ^ set(sd.keys())
    for k, v in sd.items():
        if k.endswith("pos_encoder.pe"):
            assert rel(own[k][: v.shape[0]], v) < 1e-6
            continue
        assert tuple(own[k].shape) == tuple(v.shape), k
        own[k].copy_(v)


@pytest.mark.parametrize("pos", ["FFN", "MHA", "EMB", "none"])
@pytest.mark.parametrize("fused", [False, True])
def test_bayes_transformer_golden(dev, pos, fused):
    from bayeslms_amd import model as M, ops
    g, sd, grad = load_golden("bayes_tlm_" + pos)
    V, d = sd["encoder.weight"].shape
    ff = sd["transformerlayers.0.linear1.weight"].shape[0]
    nl = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("transformerlayers."))
    nhead = int(g["nhead"])
    m = M.BayesTransformerModel(V, d, nhead, ff, nl, 0.2, True, pos).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    zero_dropout(m)
    m.set_fused_sampling(fused)
    src, tgt = g["src"].to(dev), g["tgt"].to(dev)
    # eval: mean weights
    m.eval()
    with torch.no_grad():
        logits = m(src)
        assert rel(logits, g["logits_eval"]) < TOL
        _, nll = ops.cross_entropy(logits.view(-1, V), tgt)
        assert rel(nll, g["nll_eval"]) < TOL
    # train: eps injected
    m.train()
    if pos == "FFN":
        m.transformerlayers[0].linear2.eps_override = g["eps"].to(dev)
        klf = m.transformerlayers[0].linear2.kl_divergence
    elif pos == "MHA":
        m.transformerlayers[0].self_attn.o_net.eps_override = g["eps"].to(dev)
        klf = m.transformerlayers[0].self_attn.o_net.kl_divergence
    elif pos == "EMB":
        m.embed_eps_override = g["eps"].to(dev)
        klf = m.embed_kl_divergence
    else:
        klf = None
    logits = m(src)
    assert rel(logits, g["logits_train"]) < TOL
    mle, _ = ops.cross_entropy(logits.view(-1, V), tgt)
    assert abs(float(mle) - float(g["mle"])) < TOL * abs(float(g["mle"]))
    loss = mle
    if klf is not None:
        kl = klf()
        assert abs(float(kl) - float(g["kl"])) < TOL * abs(float(g["kl"]))
        loss = mle + kl * float(g["kl_scale"])
    assert abs(float(loss) - float(g["loss"])) < TOL * abs(float(g["loss"]))
    loss.backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight":
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, grad[k]), k


def test_transformer_baseline_golden(dev):
    from bayeslms_amd import model as M
    g, sd, _ = load_golden("transformer_baseline")
    V, d = sd["encoder.weight"].shape
    ff = sd["transformerlayers.layers.0.linear1.weight"].shape[0]
    m = M.TransformerModel(V, d, int(g["nhead"]), ff, 2, 0.2, "gelu", True).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    m.eval()
    with torch.no_grad():
        assert rel(m(g["src"].to(dev)), g["logits_eval"]) < TOL


@pytest.mark.parametrize("pos", [0, 1, 2, 3, 4, 5])
def test_bayes_lstm_golden(dev, pos):
    from bayeslms_amd import model as M, ops
    g, sd, grad = load_golden("bayes_rnn_pos%d" % pos)
    V, H = sd["encoder.weight"].shape
    m = M.BayesRNNModel("LSTM", V, H, H, 2, 0.0, True, pos).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    x1, x2, tgt = g["x1"].to(dev), g["x2"].to(dev), g["tgt"].to(dev)
    B = x1.shape[1]
    m.eval()
    with torch.no_grad():
        hid = m.init_hidden(B)
        l1, hid = m(x1, hid)
        l2, hid = m(x2, hid)
        assert rel(l1, g["logits_eval_0"]) < TOL and rel(l2, g["logits_eval_1"]) < TOL
        assert rel(hid[0], g["h_eval"]) < TOL and rel(hid[1], g["c_eval"]) < TOL
    m.train()
    hid = m.init_hidden(B)
    for w, x in enumerate((x1, x2)):
        if 1 <= pos <= 4:
            m.rnn.eps_override = [g["eps_%d_%d" % (w, j)].to(dev) for j in range(8)]
        hid = M.repackage_hidden(hid)
        logits, hid = m(x, hid)
        assert rel(logits, g["logits_train_%d" % w]) < TOL
    assert rel(hid[0], g["h_train"]) < TOL
    mle, _ = ops.cross_entropy(logits.view(-1, V), tgt)
    assert abs(float(mle) - float(g["mle"])) < TOL * abs(float(g["mle"]))
    loss = mle
    if 1 <= pos <= 5:  # train.py:337; position 5 never samples but has the (layer-mixing) KL of model.py:746-755
        kl = m.rnn.kl_divergence()
        assert abs(float(kl) - float(g["kl"])) < TOL * abs(float(g["kl"]))
        loss = mle + kl * float(g["kl_scale"])
    loss.backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or k not in grad:
            continue  # position 5: tensors the reference's KL never touches have no gradient on either side
        assert p.grad is not None, k
        assert grad_close(p.grad, grad[k]), k


def test_rnn_baseline_golden(dev):
    from bayeslms_amd import model as M
    g, sd, _ = load_golden("rnn_baseline")
    V, H = sd["encoder.weight"].shape
    m = M.RNNModel("LSTM", V, H, H, 2, 0.2, True).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    m.eval()
    with torch.no_grad():
        hid = m.init_hidden(g["x1"].shape[1])
        l1, hid = m(g["x1"].to(dev), hid)
        l2, hid = m(g["x2"].to(dev), hid)
    assert rel(l1, g["logits_eval_0"]) < TOL and rel(l2, g["logits_eval_1"]) < TOL
    assert rel(hid[1], g["c_eval"]) < TOL


def test_trainer_step_matches_oracle_step(dev):
    """Flat buffers + fused KL epilogue + fused clip/SGD: two optimisation steps of the engine vs
    the oracle's restatement of train.py:315-420 (dropout 0, eps = the Philox stream)."""
    import numpy as np
    from bayeslms_amd import model as M, engine
    from oracle import bayes_oracle as O, philox as P
    torch.manual_seed(3)
    V, d, h, ff, nl, T, B = 120, 32, 4, 64, 2, 12, 4
    m = M.BayesTransformerModel(V, d, h, ff, nl, 0.0, True, "FFN")
    zero_dropout(m)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(dev)
    kl_scale = T / 500.0
    tr = engine.Trainer(m, lr=0.5, clip=0.25, kl_scale=kl_scale, seed=1111)
    lin2 = m.transformerlayers[0].linear2

    def kl_fn(model):
        return model.transformerlayers[0].linear2.kl_divergence()
    kl_fn.fusable = True

    # oracle side
    names = [k for k, _ in m.named_parameters() if k != "decoder.weight"]
    ref = {k: v.clone().requires_grad_(k in names) for k, v in sd0.items()}
    ref["decoder.weight"] = ref["encoder.weight"]
    bufs = [None] * len(names)
    gen = torch.Generator().manual_seed(9)
    for step in range(2):
        src = torch.randint(0, V, (T, B), generator=gen)
        tgt = torch.randint(0, V, (T * B,), generator=gen)
        loss, kl, _ = tr.step(src.to(dev), tgt.to(dev), kl_fn=kl_fn)
        eps = torch.from_numpy(P.normal(d * ff, 1111, P.STREAM_WEIGHT + lin2._site_base, step)).view(d, ff)
        for k in names:
            ref[k].grad = None
        rl, _, rkl = O.transformer_train_loss(src, tgt, ref, h, "FFN", eps, kl_scale)
        rl.backward()
        assert abs(float(loss) - float(rl)) < 2e-4 * abs(float(rl)), (step, float(loss), float(rl))
        assert abs(float(kl) - float(rkl)) < 2e-4 * abs(float(rkl))
        O.clip_and_sgd([ref[k] for k in names], [ref[k].grad for k in names], bufs, 0.5, 0.25)
        cur = dict(m.named_parameters())
        for k in names:
            assert rel(cur[k].data, ref[k].data) < 1e-3, (step, k)


@pytest.mark.parametrize("gp", [0, 1, 2, 3])
def test_gauss_transformer_golden(dev, gp):
    """GaussTransformerModel (GPNN activation mixture in the GEMM epilogue) vs the reference."""
    from bayeslms_amd import model as M, ops
    g, sd, grad = load_golden("gauss_tlm_%d" % gp)
    V, d = sd["encoder.weight"].shape
    ff = sd["transformerlayers.0.linear1.weight"].shape[0]
    m = M.GaussTransformerModel(V, d, int(g["nhead"]), ff, 2, 0.0, True, gp).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    src, tgt = g["src"].to(dev), g["tgt"].to(dev)
    m.eval()
    with torch.no_grad():
        assert rel(m(src), g["logits_eval"]) < TOL
    m.train()
    logits = m(src)
    assert rel(logits, g["logits_train"]) < TOL
    mle, _ = ops.cross_entropy(logits.view(-1, V), tgt)
    loss = mle
    if 1 <= gp <= 3:
        kl = m.transformerlayers[0].gpnn.kl_divergence()
        assert abs(float(kl) - float(g["kl"])) < TOL * abs(float(g["kl"])) + 1e-7
        loss = mle + kl * float(g["kl_scale"])
    loss.backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or k not in grad:
            continue  # linear1 of the GP layer is unused (reference model.py:2257,2283): no gradient either side
        assert p.grad is not None, k
        assert grad_close(p.grad, grad[k]), k


def _gp_eps(g, prefix, dev):
    return {k[len(prefix):]: v.to(dev) for k, v in g.items() if k.startswith(prefix) and k[len(prefix):] in ("coef", "weights", "bias")}


@pytest.mark.parametrize("gp", [1, 2, 3])
def test_gauss_transformer_sample_branch_golden(dev, gp):
    """GPNN.sample raised (reference model.py:1863-1884, redrawn per forward at :2280-2281): the reference's own eps
    buffers injected; logits, KL, every gradient incl. the reparameterisation gradients of the lgstd tensors."""
    from bayeslms_amd import model as M, ops
    g, sd, grad = load_golden("gauss_tlm_%d_sample" % gp)
    V, d = sd["encoder.weight"].shape
    ff = sd["transformerlayers.0.linear1.weight"].shape[0]
    m = M.GaussTransformerModel(V, d, int(g["nhead"]), ff, 2, 0.0, True, gp).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    src, tgt = g["src"].to(dev), g["tgt"].to(dev)
    gpnn = m.transformerlayers[0].gpnn
    gpnn.sample = True
    gpnn.eps_override = _gp_eps(g, "eps_", dev)
    m.eval()
    with torch.no_grad():  # eval mode never samples, flag or not
        assert rel(m(src), g["logits_eval"]) < TOL
    m.train()
    logits = m(src)
    assert rel(logits, g["logits_train"]) < TOL
    mle, _ = ops.cross_entropy(logits.view(-1, V), tgt)
    kl = gpnn.kl_divergence()
    assert abs(float(kl) - float(g["kl"])) < TOL * abs(float(g["kl"])) + 1e-7
    (mle + kl * float(g["kl_scale"])).backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or k not in grad:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, grad[k]), k
    # Philox mode: same (seed, step) -> same draw; another step -> another; sample off -> the mean forward
    gpnn.eps_override = None
    m.set_seed(3)
    m.set_step(5)
    with torch.no_grad():
        a, b = m(src), m(src)
        m.set_step(6)
        c = m(src)
        gpnn.sample = False
        e = m(src)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert rel(e, g["logits_eval"]) < TOL and rel(a, g["logits_eval"]) > 1e-4


def test_gauss_transformer_gpnn2_golden(dev):
    """--T_gauss_pos 4 (GPNN2 random-feature layer) vs the reference: eval logits, train logits with the
    recovered frequency draw injected, and every gradient."""
    from bayeslms_amd import model as M, ops
    g, sd, grad = load_golden("gauss_tlm_4")
    V, d = sd["encoder.weight"].shape
    ff = sd["transformerlayers.0.linear1.weight"].shape[0]
    m = M.GaussTransformerModel(V, d, int(g["nhead"]), ff, 2, 0.0, True, 4).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    src, tgt = g["src"].to(dev), g["tgt"].to(dev)
    m.eval()
    with torch.no_grad():
        assert rel(m(src), g["logits_eval"]) < TOL
    m.train()
    m.transformerlayers[0].gpnn.eps_override = g["eps"].to(dev)
    logits = m(src)
    assert rel(logits, g["logits_train"]) < TOL
    mle, _ = ops.cross_entropy(logits.view(-1, V), tgt)
    mle.backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or k not in grad:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, grad[k]), k
    # Philox mode: a different draw per step, same draw for the same step
    m.transformerlayers[0].gpnn.eps_override = None
    m.set_seed(7)
    m.set_step(1)
    a = m(src).detach().clone()
    b = m(src).detach().clone()
    m.set_step(2)
    c = m(src).detach().clone()
    assert torch.equal(a, b) and not torch.equal(a, c)


def _write_corpus(g, d):
    import os
    with open(os.path.join(d, "words.txt"), "w") as f:
        f.write("".join("%s %d\n" % (w, i) for i, w in enumerate(g["words"])))
    for s in ("train", "valid", "test"):
        if s + "_txt" in g:
            with open(os.path.join(d, s + ".txt"), "w") as f:
                f.write(str(g[s + "_txt"]))


@pytest.mark.parametrize("tag", ["tlm_ffn", "lstm_bayes3"])
def test_evaluate_reference_checkpoint(dev, tag, tmp_path):
    """model.pt written by the reference's train.py -> loaded by name -> engine.evaluate gives the
    reference's valid/test loss (PPL parity gate)."""
    from bayeslms_amd import data as D, engine, model as M
    g, sd, _ = load_golden("train_ckpt_" + tag)
    _write_corpus(g, str(tmp_path))
    c = D.Corpus(str(tmp_path))
    V = len(c.dictionary)
    if tag == "tlm_ffn":
        m = M.BayesTransformerModel(V, 16, 4, 32, 2, 0.0, True, "FFN")
    else:
        m = M.BayesRNNModel("LSTM", V, 12, 12, 2, 0.0, True, 3)
    own = m.state_dict()
    own.update({k: v for k, v in sd.items() if k in own})
    m.load_state_dict(own)
    m = m.to(dev)
    for split in ("valid", "test"):
        src = D.batchify(getattr(c, split), 20, dev)
        got = engine.evaluate(m, src, 7)
        assert abs(got - float(g[split + "_loss"])) < 1e-4 * float(g[split + "_loss"]), (split, got)


@pytest.mark.parametrize("tag", ["tlm_ffn", "lstm_bayes3", "tlm_gauss3", "lstm_gauss33", "lstm_var11"])
def test_scorer_cli_matches_reference_output(dev, tag, tmp_path):
    """Same n-best file, vocabulary and model.pt as the reference scorer run -> same score file."""
    import os
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
    for batched in ("1", "0"):  # padded per-utterance batch (default) and the reference's one-launch-per-hypothesis loop
        S.main(argv + ["--batched", batched])
        got = [ln.split() for ln in open(os.path.join(d, "out.txt")).read().splitlines()]
        assert [a[0] for a in got] == [b[0] for b in want]
        for a, b in zip(got, want):
            assert abs(float(a[1]) - float(b[1])) <= 1e-3 * max(1.0, abs(float(b[1]))), (batched, a, b)
    # Monte-Carlo weight sampling through the CLI (oracle comparison: test_mc_sample_scoring_matches_oracle)
    S.main(argv + ["--mc-samples", "4"])
    mc = [float(ln.split()[1]) for ln in open(os.path.join(d, "out.txt")).read().splitlines()]
    assert len(mc) == len(want) and all(v == v and v >= 0 for v in mc)


@pytest.mark.parametrize("name,ctor", [
    ("scorer_cfg1_from_seed", lambda M, V: M.BayesRNNModel("LSTM", V, 1024, 1024, 2, 0.5, True, 3)),
    ("scorer_cfg2_from_seed", lambda M, V: M.BayesTransformerModel(V, 512, 8, 4096, 6, 0.5, True, "FFN")),
    ("scorer_cfg4_from_seed", lambda M, V: M.GaussTransformerModel(V, 512, 8, 4096, 6, 0.5, True, 3)),
])
def test_scorer_cli_at_full_size_matches_the_reference_scorer(dev, name, ctor, tmp_path):
    """BASELINE.json configs[1] / [2] / [4] at their REAL sizes (33,000 words) through the rescoring path: the reference scorer's
    main() scored 8 utterances x 5-best (out-of-vocabulary words and an empty hypothesis among them) with the model its
    constructor gives under torch.manual_seed(1111) -- the fixture keeps the n-best text and the score file, no parameters.  Our
    constructor under the same seed gives the same model (tests/test_init_state_cpu.py); its state_dict goes to model.pt and the
    scorer CLI -- padded per-utterance batches (fused decoder + NLL, packed rows) and the per-hypothesis loop -- must write the
    reference's scores: every one within 1e-3 relative (north_star's bar for n-best rescoring scores)."""
    import os
    import numpy as np
    from conftest import GOLDEN
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
    assert len(want) == 40
    worst = 0.0
    for batched in ("1", "0"):
        S.main(argv + ["--batched", batched])
        got = [ln.split() for ln in open(os.path.join(d, "out.txt")).read().splitlines()]
        assert [a[0] for a in got] == [b[0] for b in want]
        for a, b in zip(got, want):
            err = abs(float(a[1]) - float(b[1])) / max(1.0, abs(float(b[1])))
            worst = max(worst, err)
            assert err <= 1e-3, (batched, a, b)
    assert worst <= 1e-4, worst  # in fact an order of magnitude inside the bar (the file prints four decimals)


@pytest.mark.parametrize("tag", ["tlm_ffn", "lstm_bayes3"])
def test_mc_sample_scoring_matches_oracle(dev, tag):
    """BASELINE.json configs[4]: n-best scoring with S Monte-Carlo weight samples.  Not in the reference (it scores
    with mean weights, :225); SURVEY 8(e) defines it.  Against the CPU oracle: sample s draws eps from Philox step s
    of each variational tensor's stream, score = -log mean_s exp(-NLL_s); S = 8 to 1e-3.  With sigma -> 0 and S = 1
    the scores are the reference scorer's own file.  The result must not depend on how utterances are batched."""
    import collections
    from bayeslms_amd import compute_sentence_scores as S, model as M
    from oracle import bayes_oracle as O
    g, sd, _ = load_golden("scorer_" + tag)
    vocab = {w: i for i, w in enumerate(g["words"])}
    V = len(vocab)
    nbest = collections.OrderedDict()
    for line in str(g["nbest_txt"]).splitlines():
        parts = line.strip().split(' ', 1)
        key, hyp = (parts[0], parts[1]) if len(parts) == 2 else (line.strip(), ' ')
        nbest.setdefault(key.rsplit('-', 1)[0], []).append(hyp)
    if tag == "tlm_ffn":
        m = M.BayesTransformerModel(V, 16, 4, 32, 2, 0.5, True, "FFN")
        fam, mtype = "tlm_ffn", "Transformer"
        ids = [m.transformerlayers[0].linear2._site_base]
    else:
        m = M.BayesRNNModel("LSTM", V, 12, 12, 2, 0.5, True, 3)
        fam, mtype = "lstm_bayes", "LSTM"
        ids = [m.rnn._site_base + k for k in range(8)]
    own = m.state_dict()
    own.update({k: v for k, v in sd.items() if k in own and tuple(v.shape) == tuple(own[k].shape)})
    m.load_state_dict(own)
    m = m.to(dev)
    osd = {k: v.clone() for k, v in sd.items()}
    if fam == "tlm_ffn":
        osd["pos_encoder.pe"] = O.positional_table(5000, 16)
    seed, NS = 4242, 8
    want = O.mc_scores(nbest, vocab, osd, fam, NS, seed, ids, get_input_and_target=S.get_input_and_target)
    for batch_tokens in (8192, 16):  # everything in one packed batch / (almost) one utterance per batch
        got = S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=NS, seed=seed, batch_tokens=batch_tokens)
        flat = [("%s-%d" % (k, n), v) for k, hv in got.items() for n, (_, v) in enumerate(hv, 1)]
        assert [k for k, _ in flat] == [k for k, _ in want]
        for (k, a), (_, b) in zip(flat, want):
            assert abs(a - b) <= 1e-3 * max(1.0, abs(b)), (batch_tokens, k, a, b)
    # the samples matter: S = 8 differs from the mean-weight scores of the reference file
    ref = [float(ln.split()[1]) for ln in str(g["scores_txt"]).splitlines()]
    assert any(abs(a - b) > 1e-4 for (_, a), b in zip(flat, ref))
    # sigma -> 0, S = 1: exactly the mean-weight model = the reference scorer's file
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "lgstd" in k:
                p.fill_(-50.0)
    got = S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=1, seed=seed)
    flat = [v for hv in got.values() for _, v in hv]
    for a, b in zip(flat, ref):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b))


def _scorer_nbest(g):
    import collections
    vocab = {w: i for i, w in enumerate(g["words"])}
    nbest = collections.OrderedDict()
    for line in str(g["nbest_txt"]).splitlines():
        parts = line.strip().split(' ', 1)
        key, hyp = (parts[0], parts[1]) if len(parts) == 2 else (line.strip(), ' ')
        nbest.setdefault(key.rsplit('-', 1)[0], []).append(hyp)
    return vocab, nbest


@pytest.mark.parametrize("fam,pos", [("tlm_gauss", 3), ("tlm_gauss", 1), ("tlm_gauss", 2), ("tlm_gauss", 4),
                                     ("lstm_gauss", "33"), ("lstm_gauss", "31"), ("lstm_gauss", "6360"), ("lstm_gauss", "530"),
                                     ("lstm_var", "11"), ("lstm_var", "01")])
def test_mc_sample_scoring_gp_and_variational_families(dev, fam, pos):
    """BASELINE.json configs[4] literally: GP Transformer (--T_gauss_pos 3) / GP-LSTM / Variational LSTM n-best scoring
    with 8 Monte-Carlo samples.  The scorer raises GPNN.sample for the call (the reference never does, model.py:1799), sample
    s draws coef / weights / bias (GPNN2: the frequencies; VNN: the noise rows) from Philox step s; S = 8 against the
    CPU oracle to 1e-3, independent of the batch packing; S differs from the mean-weight scores; sigma -> 0 gives them back."""
    from bayeslms_amd import compute_sentence_scores as S, model as M
    from oracle import bayes_oracle as O
    g, _, _ = load_golden("scorer_tlm_ffn")
    vocab, nbest = _scorer_nbest(g)
    V = len(vocab)
    torch.manual_seed(31)
    if fam == "tlm_gauss":
        m = M.GaussTransformerModel(V, 16, 4, 32, 2, 0.5, True, pos)
        mtype, ids = "Transformer", [m.transformerlayers[0].gpnn._site_base]
    elif fam == "lstm_gauss":
        m = M.GaussRNNModel("LSTM", V, 12, 12, 2, 0.5, True, pos)
        mtype = "LSTM"
        ids = {c: cell.gpnn._site_base for c, cell in enumerate(m.rnn.rnn) if hasattr(cell, "gpnn")}
    else:
        m = M.VariationalRNNModel("LSTM", V, 12, 12, 2, 0.5, True, pos)
        mtype = "LSTM"
        ids = {c: cell.vnn._site_base for c, cell in enumerate(m.rnn.rnn) if cell.vnn_type == 1}
    with torch.no_grad():  # sigma large enough for the samples to matter at these tiny sizes
        for k, p in m.named_parameters():
            if "lgstd" in k:
                p.add_(1.0)
    m = m.to(dev)
    osd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    if mtype == "Transformer":
        osd["pos_encoder.pe"] = O.positional_table(5000, 16)
    seed, NS = 977, 8
    want = O.mc_scores(nbest, vocab, osd, fam, NS, seed, ids, pos=pos, get_input_and_target=S.get_input_and_target)
    for batch_tokens in (8192, 16):
        got = S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=NS, seed=seed, batch_tokens=batch_tokens)
        flat = [("%s-%d" % (k, n), v) for k, hv in got.items() for n, (_, v) in enumerate(hv, 1)]
        assert [k for k, _ in flat] == [k for k, _ in want]
        for (k, a), (_, b) in zip(flat, want):
            assert abs(a - b) <= 1e-3 * max(1.0, abs(b)), (batch_tokens, k, a, b)
    assert not m.training and all(not getattr(mod, "sample", False) for mod in m.modules() if isinstance(mod, M.GPNN))
    mean = S.compute_scores_batched(nbest, m, vocab, mtype, dev)
    mflat = [v for hv in mean.values() for _, v in hv]
    assert any(abs(a - b) > 1e-4 for (_, a), b in zip(flat, mflat))
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "lgstd" in k:
                p.fill_(-50.0)
    got = S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=2, seed=seed)
    for a, b in zip([v for hv in got.values() for _, v in hv], mflat):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b))


@pytest.mark.parametrize("tag", ["tlm_gauss3", "lstm_gauss33", "lstm_var11"])
def test_mc_scoring_with_vanishing_sigma_reproduces_the_reference_scorer_file(dev, tag):
    """The reference scorer's own files for its Gaussian / Variational branches (fixtures scorer_tlm_gauss3, scorer_lstm_gauss33,
    scorer_lstm_var11): with sigma -> 0 the Monte-Carlo scorer (sample flags raised, noise on) gives them back; with the
    checkpoint's own sigma the samples move the scores."""
    from bayeslms_amd import compute_sentence_scores as S, model as M
    g, sd, _ = load_golden("scorer_" + tag)
    vocab, nbest = _scorer_nbest(g)
    V = len(vocab)
    m, mtype = {"tlm_gauss3": lambda: (M.GaussTransformerModel(V, 16, 4, 32, 2, 0.5, True, 3), "Transformer"),
                "lstm_gauss33": lambda: (M.GaussRNNModel("LSTM", V, 12, 12, 2, 0.5, False, "33"), "LSTM"),
                "lstm_var11": lambda: (M.VariationalRNNModel("LSTM", V, 12, 12, 2, 0.5, True, "11"), "LSTM")}[tag]()
    own = m.state_dict()
    own.update({k: v for k, v in sd.items() if k in own and tuple(v.shape) == tuple(own[k].shape)})
    m.load_state_dict(own)
    m = m.to(dev)
    ref = [float(ln.split()[1]) for ln in str(g["scores_txt"]).splitlines()]
    mean = [v for hv in S.compute_scores_batched(nbest, m, vocab, mtype, dev).values() for _, v in hv]
    for a, b in zip(mean, ref):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b))
    mc = [v for hv in S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=4, seed=5).values() for _, v in hv]
    assert any(abs(a - b) > 1e-4 for a, b in zip(mc, ref))
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "lgstd" in k:
                p.fill_(-50.0)
    mc0 = [v for hv in S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=2, seed=5).values() for _, v in hv]
    for a, b in zip(mc0, ref):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b))


@pytest.mark.parametrize("kind", ["plain_tlm", "gauss0", "vt11", "plain_lstm", "var00", "bayes5"])
def test_mc_samples_refused_when_nothing_is_sampled(dev, kind):
    """--mc-samples S on a model without a variational tensor used to run S identical mean-weight passes:
    it raises now -- incl. BASELINE configs[4]'s literal `--T_v_pos 11` (zero layers, nothing to sample)."""
    from bayeslms_amd import compute_sentence_scores as S, model as M
    from bayeslms_amd._lib import BayesLMError
    g, _, _ = load_golden("scorer_tlm_ffn")
    vocab, nbest = _scorer_nbest(g)
    V = len(vocab)
    m, mtype = {
        "plain_tlm": lambda: (M.TransformerModel(V, 16, 4, 32, 2, 0.5, "gelu", True), "Transformer"),
        "gauss0": lambda: (M.GaussTransformerModel(V, 16, 4, 32, 2, 0.5, True, 0), "Transformer"),
        "vt11": lambda: (M.VTransformerModel(V, 16, 4, 32, 2, 0.5, True, 11), "Transformer"),
        "plain_lstm": lambda: (M.RNNModel("LSTM", V, 12, 12, 2, 0.5, True), "LSTM"),
        "var00": lambda: (M.VariationalRNNModel("LSTM", V, 12, 12, 2, 0.5, True, "00"), "LSTM"),
        "bayes5": lambda: (M.BayesRNNModel("LSTM", V, 12, 12, 2, 0.5, True, 5), "LSTM"),
    }[kind]()
    m = m.to(dev)
    with pytest.raises(BayesLMError, match="no variational tensor"):
        S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=8)
    assert S.compute_scores_batched(nbest, m, vocab, mtype, dev)  # mean-weight scoring is unaffected


@pytest.mark.parametrize("fam,uncertainty", [("tlm_gauss", False), ("lstm_bayes", False), ("tlm_gauss", True)])
def test_mc_scoring_leaves_the_noise_key_as_it_found_it(dev, fam, uncertainty):
    """compute_scores_batched(mc_samples=2) runs in model.mc_sampling: afterwards the model's (seed, step, auto_step) are the
    values from before the call -- the step counter is not taken over -- and it is in eval mode with dropout on again and
    the GPNN flags lowered.  A second call gives the same scores."""
    from bayeslms_amd import compute_sentence_scores as S, model as M
    g, _, _ = load_golden("scorer_tlm_ffn")
    vocab, nbest = _scorer_nbest(g)
    V = len(vocab)
    torch.manual_seed(7)
    if fam == "tlm_gauss":
        m, mtype = M.GaussTransformerModel(V, 16, 4, 32, 2, 0.5, True, 3), "Transformer"
    else:
        m, mtype = M.BayesRNNModel("LSTM", V, 12, 12, 2, 0.5, True, 3), "LSTM"
    m = m.to(dev)
    m.set_seed(31337)
    m.noise_state.step = 9
    ns = m.noise_state
    before = (ns.seed, ns.step, ns.auto_step)
    assert before == (31337, 9, True)
    first = S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=2, seed=5, uncertainty=uncertainty)
    assert (ns.seed, ns.step, ns.auto_step) == before
    assert not m.training and ns.dropout_off is False
    assert all(not getattr(mod, "sample", False) for mod in m.modules() if isinstance(mod, M.GPNN))
    assert m.decoder.rows is None and m.decoder.nll_targets is None and m.decoder.return_input is False
    again = S.compute_scores_batched(nbest, m, vocab, mtype, dev, mc_samples=2, seed=5, uncertainty=uncertainty)
    assert (first[0] if uncertainty else first) == (again[0] if uncertainty else again)
    assert (ns.seed, ns.step, ns.auto_step) == before


@pytest.mark.parametrize("tag", ["tlm_ffn_interp", "lstm_bayes3_interp", "tlm_gauss3_interp", "lstm_gauss33_interp"])
def test_scorer_cli_interpolation_matches_reference(dev, tag, tmp_path, monkeypatch):
    """--interpolation_flag 1: two models; the batched scorer takes both decoders in ONE launch over packed operands
    (blm_linear_nll2, no logits stored), the per-hypothesis loop mixes the materialised logits inside the CE kernel
    (blm_ce_interp_fwd); scores of the reference's compute_scores on the same two checkpoints."""
    import os
    from bayeslms_amd import compute_sentence_scores as S
    from oracle import bayes_oracle as O
    g, sd, _ = load_golden("scorer_" + tag)
    d = str(tmp_path)
    _write_corpus(g, d)
    with open(os.path.join(d, "nbest.txt"), "w") as f:
        f.write(str(g["nbest_txt"]))
    for name, full in (("model.pt", dict(sd)), ("model2.pt", dict(g["sd2"]))):
        if "pos_encoder.pe" in full:
            full["pos_encoder.pe"] = O.positional_table(5000, full["encoder.weight"].shape[1])
        torch.save(full, os.path.join(d, name))
    argv = ["--nbest-list", os.path.join(d, "nbest.txt"), "--outfile", os.path.join(d, "out.txt"), "--vocabulary",
            os.path.join(d, "words.txt"), "--model-path", os.path.join(d, "model.pt"), "--inter_path",
            os.path.join(d, "model2.pt")] + [str(a) for a in g["argv"]]
    want = [ln.split() for ln in str(g["scores_txt"]).splitlines()]
    from bayeslms_amd import ops
    calls = {"fused": 0, "materialised": 0}
    real_f, real_m = ops.linear_nll_interp, ops.cross_entropy_interp
    monkeypatch.setattr(ops, "linear_nll_interp", lambda *a, **k: (calls.__setitem__("fused", calls["fused"] + 1), real_f(*a, **k))[1])
    monkeypatch.setattr(ops, "cross_entropy_interp", lambda *a, **k: (calls.__setitem__("materialised", calls["materialised"] + 1), real_m(*a, **k))[1])
    for batched in ("1", "0"):
        S.main(argv + ["--batched", batched])
        got = [ln.split() for ln in open(os.path.join(d, "out.txt")).read().splitlines()]
        assert [a[0] for a in got] == [b[0] for b in want]
        for a, b in zip(got, want):
            assert abs(float(a[1]) - float(b[1])) <= 1e-3 * max(1.0, abs(float(b[1]))), (batched, a, b)
        if batched == "1":  # the batched scorer: ONE decoder + cross-entropy launch per batch, no logits of either model
            assert calls["fused"] > 0 and calls["materialised"] == 0, calls
    assert calls["materialised"] > 0  # --batched 0 = the reference's per-hypothesis loop keeps the two-matrix kernel


@pytest.mark.parametrize("margs", [
    ["--model", "Transformer", "--emsize", "16", "--nhid", "32", "--nlayers", "2", "--nhead", "4", "--uncertainty",
     "Bayesian", "--T_bayes_pos", "FFN"],
    ["--model", "LSTM", "--emsize", "12", "--nhid", "12", "--nlayers", "2", "--uncertainty", "Bayesian", "--L_bayes_pos", "3"],
    ["--model", "Transformer", "--emsize", "16", "--nhid", "32", "--nlayers", "2", "--nhead", "4", "--uncertainty",
     "Gaussian", "--T_gauss_pos", "3"],
])
def test_train_cli_end_to_end(dev, margs, tmp_path, capsys):
    """The train.py-compatible CLI: 2 epochs on a tiny corpus, loss goes down, the checkpoint it
    saves reloads and evaluates (by the CPU oracle for the Bayesian families) to the loss it printed."""
    import os
    import re
    from bayeslms_amd import train as T
    # a learnable toy language: every sentence walks w[i], w[i+1], w[i+2], ... (mod vocabulary)
    import numpy as np
    rng = np.random.RandomState(0)
    words = ["<s>", "<unk>"] + ["w%03d" % i for i in range(2, 30)]

    def text(n):
        lines = []
        for _ in range(n):
            a, ln = rng.randint(2, 30), rng.randint(3, 9)
            lines.append(" ".join(words[2 + (a - 2 + k) % 28] for k in range(ln)))
        return "\n".join(lines) + "\n"
    g = {"words": words, "train_txt": text(600), "valid_txt": text(60), "test_txt": text(60)}
    d = str(tmp_path)
    _write_corpus(g, d)
    save = os.path.join(d, "model.pt")
    lr = "0.5" if margs[1] == "LSTM" else "0.1"  # the recipes' learning rates per family (run_nnlm_ami_*.sh)
    T.main(["--data", d, "--epochs", "2", "--batch-size", "4", "--seq_len", "7", "--dropout", "0.1", "--lr", lr,
            "--clip", "1.0", "--tied", "--cuda", "--save", save, "--log-interval", "10"] + margs)
    out = capsys.readouterr().out
    vals = [float(x) for x in re.findall(r"valid loss\s+([0-9.]+)", out)]
    test_loss = float(re.search(r"test loss\s+([0-9.]+)", out).group(1))
    assert len(vals) == 2 and vals[1] < vals[0] and vals[1] < 2.9  # ln(30) = 3.40 is the uniform baseline
    assert "| epoch   1 |" in out and "ms/batch" in out and "kl_loss" in out
    sd = torch.load(save, map_location="cpu")
    if "Gaussian" in margs:
        return
    from oracle import bayes_oracle as O
    from bayeslms_amd import data as D
    from test_oracle_golden import oracle_eval_loss
    c = D.Corpus(d)
    ref = oracle_eval_loss(sd, c.test, margs[1] == "LSTM", 4, 3)
    assert abs(ref - test_loss) < 0.006


GAUSS_RNN = ["33", "31", "13", "23", "43", "330", "6360", "3333", "53", "73", "00"]


@pytest.mark.parametrize("gp", GAUSS_RNN)
def test_gauss_rnn_golden(dev, gp):
    """GaussRNNModel / GPLSTM / GPLSTMCell (gate types 1-7, both layer arrangements) vs the reference."""
    from bayeslms_amd import model as M, ops
    g, sd, grad = load_golden("gauss_rnn_" + gp)
    V, H = sd["encoder.weight"].shape
    m = M.GaussRNNModel("LSTM", V, H, H, 2, 0.0, True, gp).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    x1, x2, tgt = g["x1"].to(dev), g["x2"].to(dev), g["tgt"].to(dev)
    B = x1.shape[1]
    m.eval()
    with torch.no_grad():
        hid = m.init_hidden(B)
        e1, hid = m(x1, hid)
        e2, hid = m(x2, hid)
    assert rel(e1, g["logits_eval_0"]) < TOL and rel(e2, g["logits_eval_1"]) < TOL
    assert rel(hid[0], g["h_eval"]) < TOL and rel(hid[1], g["c_eval"]) < TOL
    m.train()
    hid = m.init_hidden(B)
    l1, hid = m(x1, hid)
    l2, hid = m(x2, M.repackage_hidden(hid))
    assert rel(l1, g["logits_train_0"]) < TOL and rel(l2, g["logits_train_1"]) < TOL
    mle, _ = ops.cross_entropy(l2.view(-1, V), tgt)
    loss = mle
    if int(gp[0]) > 0 and 0 < int(gp[1]) <= 3:
        cells = [0] if len(gp) < 3 else ([1] if len(gp) == 3 else [0, 1])
        kl = sum(m.rnn.rnn[c].gpnn.kl_divergence() for c in cells)
        assert abs(float(kl) - float(g["kl"])) < TOL * abs(float(g["kl"])) + 1e-7
        loss = mle + kl * float(g["kl_scale"])
    loss.backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or k not in grad:
            continue  # bias_hh is never used by the GP cells (reference quirk): no gradient on either side
        assert p.grad is not None, k
        assert grad_close(p.grad, grad[k]), k


@pytest.mark.parametrize("gp", ["33", "31", "32", "13", "23", "43", "53", "63", "73", "330", "3333"])
def test_gauss_rnn_sample_branch_golden(dev, gp):
    """GP-LSTM cells with GPNN.sample raised vs the reference: one draw per cell and window (model.py:1721-1723), the
    reference's own eps buffers injected; both windows' logits, KL, every gradient."""
    from bayeslms_amd import model as M, ops
    g, sd, grad = load_golden("gauss_rnn_%s_sample" % gp)
    V, H = sd["encoder.weight"].shape
    m = M.GaussRNNModel("LSTM", V, H, H, 2, 0.0, True, gp).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    x1, x2, tgt = g["x1"].to(dev), g["x2"].to(dev), g["tgt"].to(dev)
    B = x1.shape[1]
    cells = [int(c) for c in g["cells"]]
    for c in cells:
        m.rnn.rnn[c].gpnn.sample = True
    m.eval()
    with torch.no_grad():
        hid = m.init_hidden(B)
        e1, hid = m(x1, hid)
        e2, hid = m(x2, hid)
    assert rel(e1, g["logits_eval_0"]) < TOL and rel(e2, g["logits_eval_1"]) < TOL
    m.train()
    hid = m.init_hidden(B)
    outs = []
    for w, x in enumerate((x1, x2)):
        for c in cells:
            m.rnn.rnn[c].gpnn.eps_override = _gp_eps(g, "eps_%d_%d_" % (w, c), dev)
        logits, hid = m(x, M.repackage_hidden(hid))
        outs.append(logits.detach().clone())
    assert rel(outs[0], g["logits_train_0"]) < TOL and rel(outs[1], g["logits_train_1"]) < TOL
    mle, _ = ops.cross_entropy(logits.view(-1, V), tgt)
    kl = sum(m.rnn.rnn[c].gpnn.kl_divergence() for c in cells)
    assert abs(float(kl) - float(g["kl"])) < TOL * abs(float(g["kl"])) + 1e-7
    (mle + kl * float(g["kl_scale"])).backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or k not in grad:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, grad[k]), k


@pytest.mark.parametrize("gp", ["33", "13", "23", "43", "330", "3343", "31", "32", "63", "6360", "73", "53", "52", "5363"])
def test_gauss_rnn_sample_branch_fused_steps_match_oracle(dev, gp):
    """H = 64 (the fused step kernels) with GPNN.sample raised: injected eps per cell and window, logits of both windows,
    KL and every gradient against the CPU oracle (pinned to the reference by the *_sample fixtures); then Philox mode."""
    from bayeslms_amd import model as M, ops
    from oracle import bayes_oracle as O
    torch.manual_seed(13)
    V, H, T, B = 30, 64, 5, 4
    m = M.GaussRNNModel("LSTM", V, H, H, 2, 0.0, True, gp).to(dev)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "coef_mean" in k:
                p.uniform_(-1.0, 1.0)
            elif "weights" in k or "weight_hh" in k:
                p.mul_(3.0)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    gen = torch.Generator().manual_seed(5)
    x1, x2 = torch.randint(0, V, (T, B), generator=gen), torch.randint(0, V, (T, B), generator=gen)
    tgt = torch.randint(0, V, (T * B,), generator=gen)
    cells = [0] if len(gp) < 3 else ([1] if len(gp) == 3 else [0, 1])
    eps = []
    for w in (0, 1):
        eps.append({c: {n: torch.randn(getattr(m.rnn.rnn[c].gpnn, n + "_mean").shape, generator=gen)
                        for n in ("coef", "weights", "bias") if hasattr(m.rnn.rnn[c].gpnn, n + "_lgstd")} for c in cells})
    for c in cells:
        m.rnn.rnn[c].gpnn.sample = True
    m.train()
    hid = m.init_hidden(B)
    keep = []
    for w, x in enumerate((x1, x2)):
        for c in cells:
            m.rnn.rnn[c].gpnn.eps_override = {n: e.to(dev) for n, e in eps[w][c].items()}
        logits, hid = m(x.to(dev), M.repackage_hidden(hid))
        keep.append(logits.detach().clone())
    mle, _ = ops.cross_entropy(logits.view(-1, V), tgt.to(dev))
    kl = sum(m.rnn.rnn[c].gpnn.kl_divergence() for c in cells)
    (mle + 0.2 * kl).backward()
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    leaf["decoder.weight"] = leaf["encoder.weight"]
    zeros = (torch.zeros(2, B, H), torch.zeros(2, B, H))
    r1, hr = O.gauss_rnn_lm(x1, zeros, leaf, gp, eps[0])
    r2, hr = O.gauss_rnn_lm(x2, tuple(h.detach() for h in hr), leaf, gp, eps[1])
    assert rel(keep[0], r1) < TOL and rel(keep[1], r2) < TOL
    klr = O.kl_gauss_rnn(leaf, gp)
    (O.cross_entropy_mean(r2.view(-1, V), tgt) + 0.2 * klr).backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or leaf[k].grad is None:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, leaf[k].grad), k
    for c in cells:
        m.rnn.rnn[c].gpnn.eps_override = None
    m.set_seed(3)
    m.set_step(5)
    with torch.no_grad():
        a, _ = m(x1.to(dev), m.init_hidden(B))
        b, _ = m(x1.to(dev), m.init_hidden(B))
        m.set_step(6)
        c2, _ = m(x1.to(dev), m.init_hidden(B))
    assert torch.equal(a, b) and not torch.equal(a, c2)


def test_gp_lstm_cell_state_gpnn_needs_square_input(dev):
    """Gate type 5 feeds the H-wide cell state to a GPNN built on input_size inputs (model.py:1694,1760): with
    emsize != nhid the reference raises a shape error; so does this engine, on the fused and the step-wise path."""
    from bayeslms_amd import model as M
    from bayeslms_amd._lib import BayesLMError
    cell = M.GPLSTMCell(64, 128, gate_type=5, gpnn_type=3).to(dev)
    M.bind_state(cell, M.NoiseState())
    with pytest.raises(BayesLMError):
        cell(torch.randn(3, 2, 64, device=dev))


@pytest.mark.parametrize("gp", ["34", "14", "64", "74", "54", "340", "3464"])
def test_gauss_rnn_gpnn2_golden(dev, gp):
    """Type digit 4: GPNN2 inside the GP-LSTM cells vs the reference (eval, train with the replayed
    per-time-step frequency draws, every gradient; no KL for this type, train.py:367)."""
    from bayeslms_amd import model as M, ops
    g, sd, grad = load_golden("gauss_rnn_" + gp)
    V, H = sd["encoder.weight"].shape
    m = M.GaussRNNModel("LSTM", V, H, H, 2, 0.0, True, gp).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    x1, x2, tgt = g["x1"].to(dev), g["x2"].to(dev), g["tgt"].to(dev)
    T, B = x1.shape
    m.eval()
    with torch.no_grad():
        hid = m.init_hidden(B)
        e1, hid = m(x1, hid)
        e2, hid = m(x2, hid)
    assert rel(e1, g["logits_eval_0"]) < TOL and rel(e2, g["logits_eval_1"]) < TOL
    assert rel(hid[0], g["h_eval"]) < TOL and rel(hid[1], g["c_eval"]) < TOL
    m.train()
    hid = m.init_hidden(B)
    outs = []
    for w, x in enumerate((x1, x2)):
        for c in g["cells"]:
            m.rnn.rnn[int(c)].gpnn.eps_override = [g["eps_%d_%d_%d" % (w, int(c), t)].to(dev) for t in range(T)]
        logits, hid = m(x, M.repackage_hidden(hid))
        outs.append(logits.detach().clone())
    assert rel(outs[0], g["logits_train_0"]) < TOL and rel(outs[1], g["logits_train_1"]) < TOL
    mle, _ = ops.cross_entropy(logits.view(-1, V), tgt)
    assert abs(float(mle) - float(g["mle"])) < TOL * abs(float(g["mle"]))
    mle.backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or k not in grad:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, grad[k]), k
    # Philox mode: the time steps of one forward draw different frequencies; same step -> same result
    for c in g["cells"]:
        m.rnn.rnn[int(c)].gpnn.eps_override = None
    m.set_seed(3)
    m.set_step(5)
    with torch.no_grad():
        a, _ = m(x1, m.init_hidden(B))
        b, _ = m(x1, m.init_hidden(B))
        m.set_step(6)
        c2, _ = m(x1, m.init_hidden(B))
    assert torch.equal(a, b) and not torch.equal(a, c2)


@pytest.mark.parametrize("gp", ["33", "13", "23", "43", "330", "3343", "31", "63", "6360", "73", "730", "6373", "53", "51", "530",
                                "5353", "5363"])
def test_gauss_rnn_fused_steps_match_oracle(dev, gp):
    """H = 64: GP cells with a GPNN on one gate (types 1-4) take the fused step kernels (GPNN rows inside
    the recurrent weight, mixture as the gate activation, its derivative and the coefficient gradient
    in the backward step); gate type 5 (GPNN on the cell state, model.py:1759-1760) runs its second recurrent product
    as one skinny launch in front of every step and the mixture / its derivative inside the step kernels.  Two windows with the carried hidden state; logits, KL, every gradient
    against the CPU oracle (which the golden tests pin to the reference)."""
    from bayeslms_amd import model as M, ops
    from oracle import bayes_oracle as O
    torch.manual_seed(11)
    V, H, T, B = 30, 64, 5, 4
    m = M.GaussRNNModel("LSTM", V, H, H, 2, 0.0, True, gp).to(dev)
    with torch.no_grad():  # livelier than the init: larger recurrent weights and mixed-sign coefficients
        for k, p in m.named_parameters():
            if "coef_mean" in k:
                p.uniform_(-1.0, 1.0)
            elif "weights" in k or "weight_hh" in k:
                p.mul_(3.0)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    x1, x2 = torch.randint(0, V, (T, B), generator=g), torch.randint(0, V, (T, B), generator=g)
    tgt = torch.randint(0, V, (T * B,), generator=g)
    m.train()
    hid = m.init_hidden(B)
    l1, hid = m(x1.to(dev), hid)
    keep1 = l1.detach().clone()
    l2, hid = m(x2.to(dev), M.repackage_hidden(hid))
    keep2 = l2.detach().clone()
    mle, _ = ops.cross_entropy(l2.view(-1, V), tgt.to(dev))
    cells = [0] if len(gp) < 3 else ([1] if len(gp) == 3 else [0, 1])
    kl = sum(m.rnn.rnn[c].gpnn.kl_divergence() for c in cells) if (int(gp[0]) > 0 and 0 < int(gp[1]) <= 3) else None
    (mle + (0.2 * kl if kl is not None else 0.0)).backward()
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    leaf["decoder.weight"] = leaf["encoder.weight"]
    zeros = (torch.zeros(2, B, H), torch.zeros(2, B, H))
    r1, hr = O.gauss_rnn_lm(x1, zeros, leaf, gp)
    r2, hr = O.gauss_rnn_lm(x2, tuple(h.detach() for h in hr), leaf, gp)
    assert rel(keep1, r1) < TOL and rel(keep2, r2) < TOL
    loss = O.cross_entropy_mean(r2.view(-1, V), tgt)
    if kl is not None:
        klr = O.kl_gauss_rnn(leaf, gp)
        assert abs(float(kl) - float(klr)) < TOL * abs(float(klr)) + 1e-7
        loss = loss + 0.2 * klr
    loss.backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or leaf[k].grad is None:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, leaf[k].grad), k


@pytest.mark.parametrize("gp", ["34", "14", "24", "44", "340", "3434", "3464", "54", "64", "540", "6454", "74", "740", "7434"])
def test_gauss_rnn_gpnn2_fused_steps_match_oracle(dev, gp):
    """H = 64: GP cells with a GPNN2 that draws fresh frequencies at every time step (type digit 4) -- on a gate's
    pre-activation (gate types 1-4, model.py:1763-1770), on the cell state (5) or as the hidden projection (6) -- run from one
    autograd node with 4-6 skinny launches per step (ops._LSTMRecurrentGPNN2); the input projection (7) is batched over the
    window (ops._GPNN2Steps) in front of the plain fused recurrence.  Injected
    per-step eps, two windows with the carried state; logits and every gradient against the CPU oracle (which the
    gauss_rnn_{34,14,...} fixtures pin to the reference); then Philox mode: same step -> same result, fused == step-wise."""
    from bayeslms_amd import model as M, ops
    from oracle import bayes_oracle as O
    torch.manual_seed(13)
    V, H, T, B = 30, 64, 5, 4
    m = M.GaussRNNModel("LSTM", V, H, H, 2, 0.0, True, gp).to(dev)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "weights" in k or "frequency_mean" in k:
                p.mul_(3.0)
    cells = [0] if len(gp) < 3 else ([1] if len(gp) == 3 else [c for c in (0, 1) if gp[2 * c + 1] == "4"])
    fused = [c for c in cells if 1 <= m.rnn.rnn[c].gate_type <= 7]
    assert fused and all(ops.lstm_recurrent_gpnn2_supported(H, m.rnn.rnn[c].gpnn.n_MC_terms) for c in fused)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(6)
    x1, x2 = torch.randint(0, V, (T, B), generator=g), torch.randint(0, V, (T, B), generator=g)
    tgt = torch.randint(0, V, (T * B,), generator=g)
    nmc = m.rnn.rnn[cells[0]].gpnn.n_MC_terms
    eps = [{c: [torch.randn(m.rnn.rnn[c].gpnn.input_dim, nmc, generator=g) for _ in range(T)] for c in cells} for _ in range(2)]
    m.train()
    hid = m.init_hidden(B)
    outs = []
    for w, x in enumerate((x1, x2)):
        for c in cells:
            m.rnn.rnn[c].gpnn.eps_override = [e.to(dev) for e in eps[w][c]]
        logits, hid = m(x.to(dev), M.repackage_hidden(hid))
        outs.append(logits.detach().clone())
    mle, _ = ops.cross_entropy(logits.view(-1, V), tgt.to(dev))
    mle.backward()
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    leaf["decoder.weight"] = leaf["encoder.weight"]
    zeros = (torch.zeros(2, B, H), torch.zeros(2, B, H))
    r1, hr = O.gauss_rnn_lm(x1, zeros, leaf, gp, eps[0])
    r2, hr = O.gauss_rnn_lm(x2, tuple(h.detach() for h in hr), leaf, gp, eps[1])
    assert rel(outs[0], r1) < TOL and rel(outs[1], r2) < TOL
    O.cross_entropy_mean(r2.view(-1, V), tgt).backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or leaf[k].grad is None:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, leaf[k].grad), k
    # Philox mode: the fused layer draws the noise the step-wise layer draws (same counters per call)
    for c in cells:
        m.rnn.rnn[c].gpnn.eps_override = None
    m.set_seed(3)
    m.set_step(5)
    with torch.no_grad():
        a, _ = m(x1.to(dev), m.init_hidden(B))
        b, _ = m(x1.to(dev), m.init_hidden(B))
        orig = ops.lstm_recurrent_gpnn2_supported
        ops.lstm_recurrent_gpnn2_supported = lambda *a_: False  # the step-wise loop of the same cells
        try:
            c2, _ = m(x1.to(dev), m.init_hidden(B))
        finally:
            ops.lstm_recurrent_gpnn2_supported = orig
        assert rel(a, c2) < 1e-5
        m.set_step(6)
        d, _ = m(x1.to(dev), m.init_hidden(B))
    assert torch.equal(a, b) and not torch.equal(a, d)


def test_gpnn2_cells_with_frozen_means_and_mixed_noise_lists(dev):
    """(i) a GPNN2 cell whose frequency_mean is frozen while frequency_lgstd still wants a gradient, run with mean
    frequencies (eval-mode graph): nothing flows to the frequencies and backward must not ask the library for two NULL outputs;
    (ii) a per-call eps_override list with holes is refused with a message instead of failing inside the tensor guard."""
    from bayeslms_amd import model as M, ops
    from bayeslms_amd._lib import BayesLMError
    torch.manual_seed(2)
    V, H, T, B = 30, 64, 4, 3
    for gp in ("34", "74"):
        m = M.GaussRNNModel("LSTM", V, H, H, 2, 0.0, True, gp).to(dev)
        gpnn = m.rnn.rnn[0].gpnn
        gpnn.frequency_mean.requires_grad_(False)
        x = torch.randint(0, V, (T, B), device=dev)
        tgt = torch.randint(0, V, (T * B,), device=dev)
        m.eval()  # mean frequencies, autograd on
        logits, _ = m(x, m.init_hidden(B))
        ops.cross_entropy(logits.view(-1, V), tgt)[0].backward()
        assert gpnn.frequency_lgstd.grad is None or float(gpnn.frequency_lgstd.grad.abs().max()) == 0.0
        assert m.rnn.rnn[0].weights_hh.grad is not None and gpnn.coef.weight.grad is not None
        m.train()
        gpnn.eps_override = [torch.randn(gpnn.input_dim, gpnn.n_MC_terms, device=dev) if t != 2 else None for t in range(T)]
        with pytest.raises(BayesLMError, match="EVERY step"):
            m(x, m.init_hidden(B))


@pytest.mark.parametrize("vp", ["00", "01", "10", "11"])
def test_variational_rnn_golden(dev, vp):
    from bayeslms_amd import model as M, ops
    g, sd, grad = load_golden("variational_rnn_" + vp)
    V, H = sd["encoder.weight"].shape
    m = M.VariationalRNNModel("LSTM", V, H, H, 2, 0.0, True, vp).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    x1, tgt = g["x1"].to(dev), g["tgt"].to(dev)
    B = x1.shape[1]
    m.eval()
    with torch.no_grad():
        e1, hid = m(x1, m.init_hidden(B))
    assert rel(e1, g["logits_eval_0"]) < TOL and rel(hid[0], g["h_eval"]) < TOL
    m.train()
    for c in (0, 1):
        if "eps_%d" % c in g:
            m.rnn.rnn[c].eps_override = g["eps_%d" % c].to(dev)
    l1, hid = m(x1, m.init_hidden(B))
    assert rel(l1, g["logits_train_0"]) < TOL
    mle, _ = ops.cross_entropy(l1.view(-1, V), tgt)
    loss = mle
    if "1" in vp:
        kl = sum(m.rnn.rnn[c].vnn.kl_divergence() for c in (0, 1) if vp[c] == "1")
        assert abs(float(kl) - float(g["kl"])) < TOL * abs(float(g["kl"]))
        loss = mle + kl * float(g["kl_scale"])
    loss.backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or k not in grad:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, grad[k]), k


@pytest.mark.parametrize("vp", ["11", "01", "10"])
def test_variational_rnn_fused_steps_match_oracle(dev, vp):
    """H = 64 takes the fused one-launch-per-step kernels (noise row added inside the forward step,
    its gradient from the per-step dh written by the backward step): logits, KL and every gradient
    against the CPU oracle with the same injected eps, over two windows with the hidden state carried."""
    from bayeslms_amd import model as M, ops
    from oracle import bayes_oracle as O
    torch.manual_seed(3)
    V, H, T, B = 40, 64, 6, 5
    m = M.VariationalRNNModel("LSTM", V, H, H, 2, 0.0, True, vp).to(dev)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    x = torch.randint(0, V, (T, B), generator=g)
    tgt = torch.randint(0, V, (T * B,), generator=g)
    eps = {c: torch.randn(T, H, generator=g) * 0.1 for c in (0, 1) if vp[c] == "1"}
    m.train()
    for c, e in eps.items():
        m.rnn.rnn[c].eps_override = e.to(dev)
    hid = m.init_hidden(B)
    l1, hid = m(x.to(dev), hid)
    logits = l1.detach().clone()  # ops.cross_entropy consumes the logits buffer (gradient written in place)
    mle, _ = ops.cross_entropy(l1.view(-1, V), tgt.to(dev))
    kl = sum(m.rnn.rnn[c].vnn.kl_divergence() for c in (0, 1) if vp[c] == "1")
    (mle + 0.3 * kl).backward()
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    leaf["decoder.weight"] = leaf["encoder.weight"]
    zeros = (torch.zeros(2, B, H), torch.zeros(2, B, H))
    lr, _, klr = O.variational_rnn_lm(x, zeros, leaf, vp, eps)
    (O.cross_entropy_mean(lr.view(-1, V), tgt) + 0.3 * klr).backward()
    assert rel(logits, lr) < TOL
    assert abs(float(kl) - float(klr)) < TOL * max(1e-6, abs(float(klr)))
    for k, p in m.named_parameters():
        if k == "decoder.weight" or leaf[k].grad is None:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, leaf[k].grad), k


@pytest.mark.parametrize("v_pos", [0, 1, 2, 3])
def test_vtransformer_golden(dev, v_pos):
    from bayeslms_amd import model as M
    g, sd, _ = load_golden("vtransformer_%d" % v_pos)
    V, d = sd["encoder.weight"].shape
    m = M.VTransformerModel(V, d, int(g["nhead"]), 32, 4, 0.0, True, v_pos).to(dev)
    with torch.no_grad():
        load_sd(m, sd)
    m.eval()
    with torch.no_grad():
        assert rel(m(g["src"].to(dev)), g["logits_eval"]) < TOL
    if v_pos in (1, 3):  # the reference's train-mode crash at T == 100 is reproduced
        m.train()
        with pytest.raises(AttributeError):
            m(torch.zeros(100, 1, dtype=torch.long, device=dev))


def test_vtransformer_11_golden(dev):
    """`--uncertainty Variational --T_v_pos 11`, the literal flags of BASELINE configs[4]: zero encoder layers
    (model.py:2822-2843).  Eval logits, train-mode loss and every gradient against the reference's fixture."""
    from bayeslms_amd import model as M, ops
    g, sd, grad = load_golden("vtransformer_11")
    V, d = sd["encoder.weight"].shape
    m = M.VTransformerModel(V, d, int(g["nhead"]), 32, 4, 0.0, True, 11).to(dev)
    assert len(m.transformerlayers) == 0
    with torch.no_grad():
        load_sd(m, sd)
    m.eval()
    with torch.no_grad():
        assert rel(m(g["src"].to(dev)), g["logits_eval"]) < TOL
    m.train()
    lt = m(g["src"].to(dev))
    assert rel(lt, g["logits_train"]) < TOL
    mle, _ = ops.cross_entropy(lt.view(-1, V), g["tgt"].to(dev))
    assert abs(float(mle) - float(g["mle"])) < TOL * abs(float(g["mle"]))
    mle.backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or k not in grad:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, grad[k]), k


def test_full_size_cfg3_model_against_oracle(dev):
    """BASELINE.json configs[2] at its real dimensions (6L, d 512, ff 4096, 8 heads, V 33000, T 128;
    2 batch columns so the CPU oracle finishes in seconds): eval NLL and one train-mode loss +
    gradients with eps = the Philox stream, GPU engine vs CPU oracle."""
    from bayeslms_amd import model as M, ops
    from oracle import bayes_oracle as O, philox as P
    V, d, h, ff, nl, T, B = 33000, 512, 8, 4096, 6, 128, 2
    torch.manual_seed(1111)
    m = M.BayesTransformerModel(V, d, h, ff, nl, 0.0, True, "FFN")
    zero_dropout(m)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = m.to(dev)
    gen = torch.Generator().manual_seed(5)
    src = torch.randint(0, V, (T, B), generator=gen)
    tgt = torch.randint(0, V, (T * B,), generator=gen)
    torch.set_num_threads(16)
    m.eval()
    with torch.no_grad():
        logits = m(src.to(dev))
        _, nll = ops.cross_entropy(logits.view(-1, V), tgt.to(dev))
        ref_logits = O.transformer_lm(src, sd, h, None)
        ref_nll = O.token_nll(ref_logits, tgt)
    assert rel(nll, ref_nll) < 1e-4
    # train mode: eps of layer-0 linear2 from the Philox stream (seed 1111, this module's stream id, step 3)
    m.train()
    m.set_seed(1111)
    m.set_step(3)
    lin2 = m.transformerlayers[0].linear2
    logits = m(src.to(dev))
    loss, _ = ops.cross_entropy(logits.view(-1, V), tgt.to(dev))
    loss.backward()
    eps = torch.from_numpy(P.normal(d * ff, 1111, P.STREAM_WEIGHT + lin2._site_base, 3)).view(d, ff)
    leaf = {k: v.clone().requires_grad_(k.endswith(("weight_mean", "weight_lgstd", "linear1.weight"))) for k, v in sd.items()}
    leaf["decoder.weight"] = leaf["encoder.weight"]
    rl = O.cross_entropy_mean(O.transformer_lm(src, leaf, h, eps), tgt)
    rl.backward()
    assert abs(float(loss) - float(rl)) < 1e-4 * abs(float(rl))
    cur = dict(m.named_parameters())
    for k in ("transformerlayers.0.linear2.weight_mean", "transformerlayers.0.linear2.weight_lgstd",
              "transformerlayers.3.linear1.weight"):
        assert grad_close(cur[k].grad, leaf[k].grad, rtol=1e-3, atol=1e-9), k


# ------------------------------------------------------------------ BASELINE.json sizes
def test_cfg3_full_size_matches_oracle_on_a_column_subset(dev):
    """BASELINE configs[2] at its real size (6L d512 ff4096 h8 V33000, T128 B64 -> M = 8192 rows through
    the production tiles): batch columns are independent, so the logits of the first 4 columns must
    equal the CPU oracle run on those columns alone; eval mode and train mode with the sampled weight
    (eps injected, dropout off).  Also: same (seed, step) -> bit-identical logits, next step -> not."""
    from bayeslms_amd import model as M
    from oracle import bayes_oracle as O
    torch.manual_seed(1111)
    V, T, B, C = 33000, 128, 64, 4
    m = M.BayesTransformerModel(V, 512, 8, 4096, 6, 0.2, True, "FFN").to(dev)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    src = torch.randint(0, V, (T, B), generator=g)
    m.eval()
    with torch.no_grad():
        e = m(src.to(dev))[:, :C].cpu()
        ref = O.transformer_lm(src[:, :C], sd, 8, None)
    assert rel(e, ref) < 1e-4
    eps = torch.randn(512, 4096, generator=g)
    m.train()
    m.noise_state.dropout_off = True
    m.transformerlayers[0].linear2.eps_override = eps.to(dev)
    with torch.no_grad():
        t = m(src.to(dev))[:, :C].cpu()
        ref_t = O.transformer_lm(src[:, :C], sd, 8, eps)
    assert rel(t, ref_t) < 1e-4
    assert rel(t, ref) > 1e-4  # the noise is really in
    m.transformerlayers[0].linear2.eps_override = None
    m.noise_state.dropout_off = False
    m.set_seed(5)
    m.set_step(3)
    with torch.no_grad():
        a = m(src.to(dev))
        b = m(src.to(dev))
        m.set_step(4)
        c = m(src.to(dev))
    assert torch.equal(a, b) and not torch.equal(a, c)


def test_cfg5_gp_transformer_full_size_sampled_matches_oracle_on_a_column_subset(dev):
    """BASELINE configs[4]'s model at its real size (GP Transformer --T_gauss_pos 3: 6L d512 ff4096 h8 V33000, T128 B64) with
    GPNN.sample raised: the sampled coef / weights / bias (eps injected, dropout off) through the production tiles -- the GP-mixture
    epilogue at M = 8192 -- against the CPU oracle on the first 3 columns; and the mean-weight forward."""
    from bayeslms_amd import model as M
    from oracle import bayes_oracle as O
    torch.manual_seed(1111)
    V, T, B, C = 33000, 128, 64, 3
    m = M.GaussTransformerModel(V, 512, 8, 4096, 6, 0.2, True, 3).to(dev)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(19)
    src = torch.randint(0, V, (T, B), generator=g)
    gp = m.transformerlayers[0].gpnn
    eps = {"coef": torch.randn(4, 4096, generator=g), "weights": torch.randn(4096, 512, generator=g), "bias": torch.randn(4096, generator=g)}
    m.eval()
    with torch.no_grad():
        e = m(src.to(dev))[:, :C].cpu()
        ref = O.transformer_lm(src[:, :C], sd, 8, None)
    assert rel(e, ref) < 1e-4
    m.train()
    m.noise_state.dropout_off = True
    gp.sample = True
    gp.eps_override = {k: v.to(dev) for k, v in eps.items()}
    with torch.no_grad():
        t = m(src.to(dev))[:, :C].cpu()
        ref_t = O.transformer_lm(src[:, :C], sd, 8, eps)
    assert rel(t, ref_t) < 1e-4
    assert rel(t, ref) > 1e-4  # the draw is really in


def test_cfg2_full_size_matches_oracle_on_a_column_subset(dev):
    """BASELINE configs[1] at its real size (2x1024 LSTM, V33000, T35 B64): fused step kernels and the
    decoder GEMMs at M = 2240; first 3 columns against the CPU oracle, eval mode, with a carried state."""
    from bayeslms_amd import model as M
    from oracle import bayes_oracle as O
    torch.manual_seed(1111)
    V, H, T, B, C = 33000, 1024, 35, 64, 3
    m = M.BayesRNNModel("LSTM", V, H, H, 2, 0.2, True, 3).to(dev)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(10)
    x1, x2 = torch.randint(0, V, (T, B), generator=g), torch.randint(0, V, (T, B), generator=g)
    m.eval()
    with torch.no_grad():
        hid = m.init_hidden(B)
        l1, hid = m(x1.to(dev), hid)
        l2, hid = m(x2.to(dev), hid)
        z = (torch.zeros(2, C, H), torch.zeros(2, C, H))
        r1, hr = O.bayes_rnn_lm(x1[:, :C], z, sd, 3, None)
        r2, hr = O.bayes_rnn_lm(x2[:, :C], hr, sd, 3, None)
    assert rel(l1[:, :C], r1) < 1e-4 and rel(l2[:, :C], r2) < 1e-4
    assert rel(hid[0][:, :C], hr[0]) < 1e-4 and rel(hid[1][:, :C], hr[1]) < 1e-4


def test_cfg1_full_size_matches_oracle(dev):
    """BASELINE configs[0] at its real size (RNNModel 2x1024, V 10000, T 35, B 20): at this shape the product runs the two
    layers as a wavefront on two streams (ops.lstm_stack2: B <= 32 and T >= 32), which at production width was only ever
    compared with the sequential path.  Against the CPU oracle: eval logits + carried state over two windows on the first 3
    columns, and -- dropout off -- the training loss and EVERY parameter gradient of the full 20-column batch."""
    from bayeslms_amd import model as M, ops
    from oracle import bayes_oracle as O
    torch.manual_seed(1111)
    V, H, T, B, C = 10000, 1024, 35, 20, 3
    m = M.RNNModel("LSTM", V, H, H, 2, 0.0, True).to(dev)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(12)
    x1, x2 = torch.randint(0, V, (T, B), generator=g), torch.randint(0, V, (T, B), generator=g)
    tgt = torch.randint(0, V, (T * B,), generator=g)
    calls = []
    real = ops.lstm_stack2
    ops.lstm_stack2 = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        m.eval()
        with torch.no_grad():
            hid = m.init_hidden(B)
            l1, hid = m(x1.to(dev), hid)
            l2, hid = m(x2.to(dev), hid)
            z = (torch.zeros(2, C, H), torch.zeros(2, C, H))
            r1, hr = O.rnn_lm(x1[:, :C], z, sd)
            r2, hr = O.rnn_lm(x2[:, :C], hr, sd)
        assert len(calls) == 2, "the wavefront path must be the one under test at this shape"
        assert rel(l1[:, :C], r1) < 1e-4 and rel(l2[:, :C], r2) < 1e-4
        assert rel(hid[0][:, :C], hr[0]) < 1e-4 and rel(hid[1][:, :C], hr[1]) < 1e-4
        m.train()
        h0 = tuple(h.detach() for h in hid)
        logits, _ = m(x2.to(dev), h0)
        assert len(calls) == 3
        loss, _ = ops.cross_entropy(logits.view(-1, V), tgt.to(dev))
        loss.backward()
    finally:
        ops.lstm_stack2 = real
    leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    leaf["decoder.weight"] = leaf["encoder.weight"]
    rl, _ = O.rnn_lm(x2, tuple(h.cpu() for h in h0), leaf)
    rloss = O.cross_entropy_mean(rl.view(-1, V), tgt)
    assert abs(float(loss) - float(rloss)) < 1e-4 * abs(float(rloss))
    rloss.backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight":
            continue
        assert grad_close(p.grad, leaf[k].grad), k


def test_cfg3_full_model_backward_matches_oracle(dev):
    """The cfg3 model at its real width/depth/vocabulary (B = 8 columns, T = 128 keep the CPU side at a few
    seconds): train-mode loss with the sampled FFN weight (eps injected, dropout off) plus the KL term,
    and every parameter gradient against the oracle's autograd -- the decoder GEMMs at K = 33000 /
    N = 33000, the Bayesian wgrad epilogue at 512 x 4096, attention backward at T = 128."""
    from bayeslms_amd import model as M, ops
    from oracle import bayes_oracle as O
    torch.manual_seed(1111)
    V, T, B = 33000, 128, 8
    m = M.BayesTransformerModel(V, 512, 8, 4096, 6, 0.2, True, "FFN").to(dev)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(19)
    src = torch.randint(0, V, (T, B), generator=g)
    tgt = torch.randint(0, V, (T * B,), generator=g)
    eps = torch.randn(512, 4096, generator=g)
    kl_scale = 0.01
    m.train()
    m.noise_state.dropout_off = True
    m.transformerlayers[0].linear2.eps_override = eps.to(dev)
    logits = m(src.to(dev))
    mle, _ = ops.cross_entropy(logits.view(-1, V), tgt.to(dev))
    kl = m.transformerlayers[0].linear2.kl_divergence()
    (mle + kl * kl_scale).backward()
    leaf = {k: v.clone().requires_grad_(v.dtype.is_floating_point and k != "pos_encoder.pe") for k, v in sd.items()}
    leaf["decoder.weight"] = leaf["encoder.weight"]
    loss_r, mle_r, kl_r = O.transformer_train_loss(src, tgt, leaf, 8, "FFN", eps, kl_scale)
    loss_r.backward()
    assert abs(float(mle) - float(mle_r)) < 1e-4 * float(mle_r)
    assert abs(float(kl) * kl_scale - float(kl_r)) < 1e-4 * abs(float(kl_r)) + 1e-9
    checked = 0
    for k, p in m.named_parameters():
        if k == "decoder.weight" or leaf[k].grad is None:
            continue
        assert p.grad is not None, k
        assert grad_close(p.grad, leaf[k].grad), k
        checked += 1
    assert checked > 70


def test_transformer_longer_than_128_tokens(dev):
    """Windows / hypotheses longer than 128 tokens take the chunked attention kernels: logits, loss and every
    gradient of a Bayesian Transformer at T = 200 against the CPU oracle (the reference accepts any length up to
    its 5000-row positional table, model.py:97-103)."""
    from bayeslms_amd import model as M, ops
    from oracle import bayes_oracle as O
    torch.manual_seed(21)
    V, d, nhead, ff, L, T, B = 60, 128, 2, 64, 2, 200, 2
    m = M.BayesTransformerModel(V, d, nhead, ff, L, 0.0, True, "FFN").to(dev)
    zero_dropout(m)  # layer 0 is built with a hard-coded 0.2 (model.py:1202)
    src, tgt = torch.randint(0, V, (T, B)), torch.randint(0, V, (T * B,))
    eps = torch.randn(d, ff)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    m.eval()
    with torch.no_grad():
        assert rel(m(src.to(dev)), O.transformer_lm(src, sd, nhead, None)) < TOL
    m.train()
    m.transformerlayers[0].linear2.eps_override = eps.to(dev)
    logits = m(src.to(dev))
    leaf = {k: (v.clone().requires_grad_(True) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    leaf["decoder.weight"] = leaf["encoder.weight"]
    want = O.transformer_lm(src, leaf, nhead, eps)
    assert rel(logits, want) < TOL
    mle, _ = ops.cross_entropy(logits.clone().view(-1, V), tgt.to(dev))
    mle.backward()
    O.cross_entropy_mean(want.view(-1, V), tgt).backward()
    for k, p in m.named_parameters():
        if k == "decoder.weight" or leaf[k].grad is None:
            continue
        assert grad_close(p.grad, leaf[k].grad), k


@pytest.mark.parametrize("margs", [
    # train.py's own defaults for the sizes (emsize 200, nhid 200, nlayers 2, nhead 2 -> head_dim 100; untied)
    ["--model", "Transformer", "--uncertainty", "Bayesian", "--T_bayes_pos", "FFN"],
    ["--model", "LSTM", "--uncertainty", "Bayesian", "--L_bayes_pos", "3"],
    # windows longer than 128 tokens
    ["--model", "Transformer", "--emsize", "128", "--nhid", "64", "--nhead", "2", "--seq_len", "150", "--tied",
     "--uncertainty", "Bayesian", "--T_bayes_pos", "MHA"],
])
def test_train_cli_reference_default_shapes(dev, margs, tmp_path, capsys):
    """Shapes outside the tuned kernels (odd head size, hidden size not a multiple of 32, windows > 128 tokens)
    train through the same CLI: one epoch, finite and decreasing loss."""
    import re
    import numpy as np
    from bayeslms_amd import train as T
    rng = np.random.RandomState(1)
    words = ["<s>", "<unk>"] + ["w%03d" % i for i in range(2, 30)]

    def text(n):
        lines = []
        for _ in range(n):
            a, ln = rng.randint(2, 30), rng.randint(3, 9)
            lines.append(" ".join(words[2 + (a - 2 + k) % 28] for k in range(ln)))
        return "\n".join(lines) + "\n"
    d = str(tmp_path)
    _write_corpus({"words": words, "train_txt": text(900), "valid_txt": text(200), "test_txt": text(200)}, d)
    base = ["--data", d, "--epochs", "2", "--batch-size", "4", "--dropout", "0.1", "--lr", "0.5" if "LSTM" in margs else "0.1",
            "--clip", "1.0", "--cuda", "--save", d + "/m.pt", "--log-interval", "50"]
    if "--seq_len" not in margs:
        base += ["--seq_len", "7"]
    T.main(base + margs)
    out = capsys.readouterr().out
    vals = [float(x) for x in re.findall(r"valid loss\s+([0-9.]+)", out)]
    assert len(vals) == 2 and vals[1] < vals[0] and vals[1] < 3.4 and np.isfinite(vals).all(), out[-500:]


@pytest.mark.parametrize("family", ["gauss53", "gauss33", "gauss6360", "variational11", "bayes3", "plain"])
def test_lstm_scorer_batched_equals_reference_loop(dev, family):
    """LSTM n-best scoring: the carry chain walked as one long sequence (states tapped at the utterance boundaries,
    or utterance by utterance for the step-wise cells) + cross-utterance batches with per-column initial state must
    give the scores of the reference's one-hypothesis-at-a-time loop (hidden carried from the first hypothesis)."""
    import random
    from collections import OrderedDict
    from bayeslms_amd import compute_sentence_scores as S, model as M
    torch.manual_seed(31)
    V, H = 60, 32
    words = ["w%d" % i for i in range(V - 2)]
    vocab = {w: i + 2 for i, w in enumerate(words)}
    vocab["<s>"], vocab["<unk>"] = 0, 1
    if family.startswith("gauss"):
        m = M.GaussRNNModel("LSTM", V, H, H, 2, 0.0, True, family[5:])
    elif family == "variational11":
        m = M.VariationalRNNModel("LSTM", V, H, H, 2, 0.0, True, "11")
    elif family == "bayes3":
        m = M.BayesRNNModel("LSTM", V, H, H, 2, 0.0, True, 3)
    else:
        m = M.RNNModel("LSTM", V, H, H, 2, 0.0, True)
    m = m.to(dev)
    rnd = random.Random(3)
    nbest = OrderedDict()
    for u in range(7):
        base = [rnd.choice(words) for _ in range(rnd.randint(1, 9))]
        hyps = []
        for _ in range(rnd.randint(1, 5)):
            h = list(base)
            if rnd.random() < 0.7:
                h = h + [rnd.choice(words) for _ in range(rnd.randint(0, 3))]
            hyps.append(" ".join(h))
        nbest["utt%d" % u] = hyps
    want = S.compute_scores(nbest, m, vocab, "LSTM", dev)
    for bt in (8192, 40):  # everything in one batch / a few utterances per batch
        got = S.compute_scores_batched(nbest, m, vocab, "LSTM", dev, batch_tokens=bt)
        assert list(got) == list(want)
        for k in want:
            for (h1, a), (h2, b) in zip(got[k], want[k]):
                assert h1 == h2 and abs(a - b) <= 1e-4 * max(1.0, abs(b)), (family, bt, k, a, b)


@pytest.mark.parametrize("kind", ["bayes_ffn", "bayes_mha", "gauss3", "plain", "interp", "mc"])
def test_scorer_packed_tokens_equal_padded_layout(dev, kind, monkeypatch):
    """ops.packed_tokens (the Transformer stacks keep only the real tokens' rows; attention alone sees the padded batch)
    against the padded layout: same scores for every hypothesis -- head_dim 64 (matrix-core attention), ragged
    hypotheses, two interpolated models, Monte-Carlo weight samples."""
    from collections import OrderedDict
    import numpy as np
    from bayeslms_amd import compute_sentence_scores as S, model as M
    V = 97
    torch.manual_seed(3)
    mk = {"bayes_ffn": lambda: M.BayesTransformerModel(V, 128, 2, 256, 2, 0.5, True, "FFN"),
          "bayes_mha": lambda: M.BayesTransformerModel(V, 128, 2, 256, 2, 0.5, True, "MHA"),
          "gauss3": lambda: M.GaussTransformerModel(V, 128, 2, 256, 2, 0.5, True, 3),
          "plain": lambda: M.TransformerModel(V, 128, 2, 256, 2, 0.5, "gelu", True)}
    m1 = mk["bayes_ffn" if kind in ("interp", "mc") else kind]().to(dev)
    m2 = mk["plain"]().to(dev) if kind == "interp" else None
    vocab = {"<s>": 0, "<unk>": 1}
    vocab.update({"w%d" % i: i for i in range(2, V)})
    rnd = np.random.RandomState(5)
    nbest = OrderedDict()
    for u in range(7):
        nbest["utt%d" % u] = [" ".join("w%d" % rnd.randint(2, V) for _ in range(rnd.randint(1, 14))) for _ in range(rnd.randint(1, 6))]
    out = []
    for packed in (True, False):
        monkeypatch.setattr(S, "_PACKED", packed)
        sc = S.compute_scores_batched(nbest, m1, vocab, "Transformer", dev, model_2=m2, alpha=0.3 if m2 is not None else 0.0,
                                      mc_samples=3 if kind == "mc" else 0, seed=9, batch_tokens=150)
        out.append([s for key in nbest for _, s in sc[key]])
    a, b = np.asarray(out[0]), np.asarray(out[1])
    assert a.shape == b.shape and len(a) == sum(len(h) for h in nbest.values())
    np.testing.assert_allclose(a, b, rtol=2e-5, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("gauss_pos", ["13", "23", "33", "43", "63", "73", "6360"])
def test_gp_lstm_pads_a_hidden_size_that_is_not_a_multiple_of_32(gauss_pos, monkeypatch):
    """A GP-LSTM whose hidden size is not a multiple of 32 used to leave the fused step kernels for the step-wise loop (650 units:
    71 k tokens/s against 305 k at 672).  ops.lstm_recurrent_gp zero-pads it -- weights, pre-activations AND mixture coefficients, so a
    padded unit's GP gate is 0, its cell and output stay 0 -- for every place the GPNN can sit (gate types 1-4, 6, 7; two cells).  The
    padded fused path against the unpadded step-wise loop (itself pinned by the gauss_rnn fixtures): logits, carried state, every gradient."""
    from bayeslms_amd import model as M, ops
    dev = torch.device("cuda:0")
    V, H, T, B = 90, 72, 6, 5
    g = torch.Generator().manual_seed(31)
    x = torch.randint(0, V, (T, B), generator=g).to(dev)
    go = torch.randn(T, B, V, generator=g).to(dev)
    res = {}
    for padded in (True, False):
        monkeypatch.setattr(ops, "_PAD_HIDDEN_FROM", 64 if padded else 1 << 30)
        torch.manual_seed(17)
        m = M.GaussRNNModel("LSTM", V, H, H, 2, 0.0, True, gauss_pos).to(dev)
        calls = []
        real = ops._LSTMRecurrentGP.apply
        monkeypatch.setattr(ops._LSTMRecurrentGP, "apply", staticmethod(lambda *a: (calls.append(tuple(a[3].shape)), real(*a))[1]))
        m.train()
        out, hid = m(x, m.init_hidden(B))
        (out.as_subclass(torch.Tensor) * go).sum().backward()
        res[padded] = (out.detach().as_subclass(torch.Tensor).clone(), [h.detach().clone() for h in hid],
                       {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, calls)
        monkeypatch.setattr(ops._LSTMRecurrentGP, "apply", real)
    assert res[True][3] and all(s == (4 * 96, 96) for s in res[True][3]) and not res[False][3]   # 72 -> 96 on the fused kernels / the loop
    assert rel(res[True][0], res[False][0]) < 1e-5
    for a, b in zip(res[True][1], res[False][1]):
        assert a.shape == b.shape and rel(a, b) < 1e-5
    assert set(res[True][2]) == set(res[False][2])
    for k in res[True][2]:
        a, b = res[True][2][k], res[False][2][k]
        assert a.shape == b.shape and float((a - b).abs().max()) <= 5e-5 * float(b.abs().max()) + 1e-8, k
