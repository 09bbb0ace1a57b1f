"""GPU: incremental next-word scoring with a key/value cache (bayeslms_amd/incremental.py, csrc/decode.hip).

The kernels against float64 references; IncrementalLM against the reference's own eval logits of every Transformer fixture (fed
token by token, in chunks and as ragged chunks), against the engine's full forward at long contexts and head sizes 100 / 128, the
LSTM families, the reference scorer's score files rescored by forking hypotheses from a shared <s> stream, beam prune / fork,
and the generate CLI against argmax generation by full recompute."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from bayeslms_amd import BayesLMError
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-4


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lib():
    from bayeslms_amd import _lib as L
    L.require_gfx950()
    return L, L.lib()


# ----------------------------------------------------------------------------------------------------------------- kernels
def _attn_ref(q, kv, past, n_new, nhead, hd):
    """float64: row (t, n) attends cache positions [0, past[n] + t] of kv (2, n_cap, nhead, max_len, hd)."""
    Tq, N = q.shape[0], q.shape[1]
    out = torch.zeros(Tq, N, nhead * hd, dtype=torch.float64)
    qd, kd = q.double().cpu(), kv.double().cpu()
    for n in range(N):
        for h in range(nhead):
            rows = n_new[n]
            Q = qd[:rows, n, h * hd:(h + 1) * hd] / np.sqrt(hd)
            Lk = past[n] + rows
            K, Vv = kd[0, n, h, :Lk], kd[1, n, h, :Lk]
            s = Q @ K.t()
            mask = torch.arange(Lk)[None, :] > (past[n] + torch.arange(rows))[:, None]
            s[mask] = -float("inf")
            out[:rows, n, h * hd:(h + 1) * hd] = torch.softmax(s, -1) @ Vv
    return out


def _decode(L, lib, q, ld, kv, past_d, nnew_d, Tq, N, n_cap, nhead, max_len, hd, ctx_max):
    out = torch.full((Tq, N, nhead * hd), 7.0, device=q.device)
    nws = lib.blm_attn_decode_ws_floats(Tq, N, nhead, ctx_max, hd)
    ws = torch.empty(nws, device=q.device)
    L.check(lib.blm_attn_decode(q.data_ptr(), ld, kv.data_ptr(), past_d.data_ptr(), L.ptr(nnew_d), out.data_ptr(), ws.data_ptr(), nws,
                                Tq, N, n_cap, nhead, max_len, hd, ctx_max, L.stream()), "blm_attn_decode")
    return out


@pytest.mark.parametrize("hd", [8, 25, 32, 64, 100, 128])
@pytest.mark.parametrize("Tq", [1, 2, 7, 33])
def test_attn_decode_against_float64(dev, hd, Tq):
    L, lib = _lib()
    g = torch.Generator().manual_seed(hd * 100 + Tq)
    nhead, max_len = 2, 5040
    past = [0, 1, 63, 64, 65, 1000, 4999]
    N, n_cap = len(past), len(past) + 1
    n_new = [Tq, max(1, Tq - 1), Tq, max(1, Tq // 2), Tq, 1, Tq]
    kv = torch.randn(2, n_cap, nhead, max_len, hd, generator=g).to(dev)
    ld = 3 * nhead * hd + 4  # the fused [q|k|v] projection, with a padded row
    q = torch.randn(Tq, N, ld, generator=g).to(dev)
    past_d = torch.tensor(past, dtype=torch.int32, device=dev)
    nnew_d = torch.tensor(n_new, dtype=torch.int32, device=dev)
    ctx_max = max(p + k for p, k in zip(past, n_new))
    out = _decode(L, lib, q, ld, kv, past_d, nnew_d, Tq, N, n_cap, nhead, max_len, hd, ctx_max)
    ref = _attn_ref(q, kv, past, n_new, nhead, hd)
    assert float((out.double().cpu() - ref).abs().max()) <= 2e-5
    for n in range(N):  # padding rows are zeros
        assert torch.all(out[n_new[n]:, n] == 0)
    again = _decode(L, lib, q, ld, kv, past_d, nnew_d, Tq, N, n_cap, nhead, max_len, hd, ctx_max)
    assert torch.equal(out, again)
    full = _decode(L, lib, q, ld, kv, past_d, None, Tq, N, n_cap, nhead, max_len, hd, max(past) + Tq)
    assert float((full.double().cpu() - _attn_ref(q, kv, past, [Tq] * N, nhead, hd)).abs().max()) <= 2e-5


def test_attn_decode_equals_full_attention(dev):
    """The whole sequence fed at once through blm_attn_decode equals blm_attn_fwd on it."""
    from bayeslms_amd import ops
    L, lib = _lib()
    T, B, nhead, hd = 70, 3, 4, 16
    d = nhead * hd
    qkv = torch.randn(T, B, 3 * d, device=dev)
    with torch.no_grad():
        ref = ops.attention(qkv, nhead)
    kv = torch.zeros(2, B, nhead, T, hd, device=dev)
    past = torch.zeros(B, dtype=torch.int32, device=dev)
    L.check(lib.blm_kv_append(qkv[..., d:].data_ptr(), qkv[..., 2 * d:].data_ptr(), 3 * d, kv.data_ptr(), past.data_ptr(), None, T, B, B,
                              nhead, T, hd, L.stream()), "blm_kv_append")
    out = _decode(L, lib, qkv, 3 * d, kv, past, None, T, B, B, nhead, T, hd, T)
    assert rel(out, ref) < 2e-6


def test_kv_append_and_gather_bitwise(dev):
    L, lib = _lib()
    Tq, N, n_cap, nhead, max_len, hd = 5, 4, 6, 3, 40, 12
    d = nhead * hd
    kv = torch.randn(2, n_cap, nhead, max_len, hd, device=dev)
    before = kv.clone()
    proj = torch.randn(Tq, N, 3 * d, device=dev)
    past = [0, 7, 33, 39]
    n_new = [5, 2, 5, 1]
    # device operands are held in names: a temporary's block goes back to the allocator before the foreign call is made
    past_d, nnew_d = torch.tensor(past, dtype=torch.int32, device=dev), torch.tensor(n_new, dtype=torch.int32, device=dev)
    L.check(lib.blm_kv_append(proj[..., d:].data_ptr(), proj[..., 2 * d:].data_ptr(), 3 * d, kv.data_ptr(), past_d.data_ptr(),
                              nnew_d.data_ptr(), Tq, N, n_cap, nhead, max_len, hd, L.stream()), "blm_kv_append")
    exp = before.clone()
    for n in range(N):
        for t in range(n_new[n]):
            exp[0, n, :, past[n] + t] = proj[t, n, d:2 * d].view(nhead, hd)
            exp[1, n, :, past[n] + t] = proj[t, n, 2 * d:].view(nhead, hd)
    assert torch.equal(kv, exp)

    # gather: 2 layers (outer 4), repeated idx, fewer streams out than in, only live prefixes copied
    outer = 4
    src = torch.randn(outer, n_cap, nhead, max_len, hd, device=dev)
    dst = torch.full_like(src, -3.0)
    lens = torch.tensor([3, 40, 0, 17, 9], dtype=torch.int32, device=dev)
    len_out = torch.full((n_cap,), -1, dtype=torch.int32, device=dev)
    idx = [3, 1, 3]
    idx_d = torch.tensor(idx, device=dev)
    L.check(lib.blm_kv_gather(src.data_ptr(), dst.data_ptr(), idx_d.data_ptr(), lens.data_ptr(), len_out.data_ptr(),
                              len(idx), 5, n_cap, outer, nhead, max_len, hd, L.stream()), "blm_kv_gather")
    exp = torch.full_like(src, -3.0)
    for j, i in enumerate(idx):
        ln = int(lens[i])
        exp[:, j, :, :ln] = src[:, i, :, :ln]
    assert torch.equal(dst, exp)
    assert len_out[:3].tolist() == [17, 40, 17] and len_out[3:].tolist() == [-1] * (n_cap - 3)
    # LSTM (h, c) rows: whole panels, no lengths
    H = 10
    hs = torch.randn(2, 2, n_cap, H, device=dev)
    hd2 = torch.zeros_like(hs)
    idx2 = torch.tensor([2, 2, 0], device=dev)
    L.check(lib.blm_kv_gather(hs.data_ptr(), hd2.data_ptr(), idx2.data_ptr(), None, None, 3, 4, n_cap,
                              4, 1, 1, H, L.stream()), "blm_kv_gather")
    assert torch.equal(hd2[:, :, :3], hs[:, :, [2, 2, 0]]) and torch.all(hd2[:, :, 3:] == 0)
    # overlapping source and destination are refused on the host
    assert lib.blm_kv_gather(src.data_ptr(), src.data_ptr() + 64, idx_d.data_ptr(), None, None, 3, 5, n_cap, outer,
                             nhead, max_len, hd, L.stream()) == L.ERR_INVALID


def test_embed_at(dev):
    from bayeslms_amd import ops
    V, D, T, N = 30, 24, 3, 4
    w = torch.randn(V, D, device=dev)
    pe = torch.randn(50, D, device=dev)
    ids = torch.randint(0, V, (T, N), device=dev)
    pos0 = torch.tensor([0, 5, 46, 11], dtype=torch.int32, device=dev)
    scale = 4.899
    out = ops.embed_at(ids, w, pe, scale, pos0)
    pos = pos0.long()[None, :] + torch.arange(T, device=dev)[:, None]
    assert torch.allclose(out, w[ids] * scale + pe[pos], rtol=0, atol=1e-6)
    x = torch.randn(T, N, D, device=dev)
    out2 = ops.embed_at(None, None, pe, 1.0, pos0, x=x)
    assert torch.allclose(out2, x + pe[pos], rtol=0, atol=1e-6)


def test_log_softmax_rows_padded_stride(dev):
    from bayeslms_amd import ops
    R, V, Vp = 9, 1001, 1004
    buf = torch.randn(R, Vp, device=dev) * 5
    x = buf[:, :V]
    ref = torch.log_softmax(x.double(), -1)
    out = ops.log_softmax_rows(x)
    assert float((out.double() - ref).abs().max()) < 2e-5
    ops.log_softmax_rows(x, out=x)  # in place
    assert float((x.double() - ref).abs().max()) < 2e-5


def test_sample_rows(dev):
    from bayeslms_amd import ops
    x = torch.randn(64, 500, device=dev)
    x[3, 10] = x[3, 400] = 50.0  # a tie: the lowest index wins
    g = ops.sample_rows(x, 0.0)
    assert torch.equal(g, x.argmax(1)) and int(g[3]) == 10
    a, b = ops.sample_rows(x, 1.0, 7, 0, 3), ops.sample_rows(x, 1.0, 7, 0, 3)
    c = ops.sample_rows(x, 1.0, 7, 0, 4)
    assert torch.equal(a, b) and not torch.equal(a, c)
    R, V = 1 << 16, 16
    logits = torch.randn(V) * 1.5
    p = torch.softmax(logits.double(), 0)
    ids = ops.sample_rows(logits.to(dev).expand(R, V).contiguous(), 1.0, 11, 2, 0)
    cnt = torch.bincount(ids.cpu(), minlength=V).double()
    se = torch.sqrt(R * p * (1 - p))
    assert torch.all((cnt - R * p).abs() <= 4 * se), (cnt, R * p)


# ------------------------------------------------------------------------------------------------------ reference fixtures
def _load(model, sd):
    own = model.state_dict()
    for k, v in sd.items():
        if k.endswith("pos_encoder.pe"):
            continue
        own[k].copy_(v)


def _fixture_model(name, dev):
    from bayeslms_amd import model as M
    g, sd, _ = load_golden(name)
    V, d = sd["encoder.weight"].shape
    nhead = int(g["nhead"])
    if name == "transformer_baseline":
        ff = sd["transformerlayers.layers.0.linear1.weight"].shape[0]
        m = M.TransformerModel(V, d, nhead, ff, 2, 0.2, "gelu", True)
    elif name.startswith("bayes_tlm_"):
        ff = sd["transformerlayers.0.linear1.weight"].shape[0]
        nl = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("transformerlayers."))
        m = M.BayesTransformerModel(V, d, nhead, ff, nl, 0.2, True, name[len("bayes_tlm_"):])
    elif name.startswith("gauss_tlm_"):
        ff = sd["transformerlayers.0.linear1.weight"].shape[0]
        m = M.GaussTransformerModel(V, d, nhead, ff, 2, 0.0, True, int(name[-1]))
    else:
        m = M.VTransformerModel(V, d, nhead, 32, 4, 0.0, True, int(name.split("_")[1]))
    m = m.to(dev)
    with torch.no_grad():
        _load(m, sd)
    m.eval()
    return m, g


FIXTURES = ["transformer_baseline"] + ["bayes_tlm_" + p for p in ("none", "EMB", "FFN", "MHA")] + \
           ["gauss_tlm_%d" % i for i in range(5)] + ["vtransformer_%d" % i for i in (0, 1, 2, 3, 11)]


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_logits_token_chunked_and_ragged(dev, name):
    from bayeslms_amd.incremental import IncrementalLM
    m, g = _fixture_model(name, dev)
    src = g["src"].to(dev)
    T, B = src.shape
    ref = torch.log_softmax(g["logits_eval"].double(), -1)
    lm = IncrementalLM(m, max_streams=B, max_len=64)
    st = lm.start(B)
    for t in range(T):  # token by token
        assert rel(lm.step(st, src[t]), ref[t]) < TOL, t
    assert st.lengths == [T] * B
    st = lm.start(B)
    t0 = 0
    for c in (2, 1, 3):  # chunks
        lp = lm.step(st, src[t0:t0 + c], all_positions=True)
        assert rel(lp, ref[t0:t0 + c]) < TOL, t0
        t0 += c
    st = lm.start(B)  # ragged: stream n takes k1[n] rows, then the rest
    k1 = [T - 1, T // 2, 1][:B] + [2] * max(0, B - 3)
    lp = lm.step(st, src, n_new=k1, all_positions=True)
    for n in range(B):
        assert rel(lp[:k1[n], n], ref[:k1[n], n]) < TOL, n
        assert torch.isnan(lp[k1[n]:, n]).all()
    k2 = [T - k for k in k1]
    rest = torch.zeros(max(k2), B, dtype=torch.int64, device=dev)
    for n in range(B):
        rest[:k2[n], n] = src[k1[n]:, n]
    last = lm.step(st, rest, n_new=k2)
    assert rel(last, ref[T - 1]) < TOL
    assert st.lengths == [T] * B


@pytest.mark.parametrize("name", ["bayes_tlm_FFN", "gauss_tlm_3"])
def test_fixture_targets_nll_after_chunks(dev, name):
    """targets=: the NLL of the word after a multi-row chunk, and of every position of a chunk, against the reference's logits."""
    from bayeslms_amd.incremental import IncrementalLM
    m, g = _fixture_model(name, dev)
    src = g["src"].to(dev)
    T, B = src.shape
    ref = torch.log_softmax(g["logits_eval"].double(), -1)
    tg = g["tgt"].view(T, B)
    lm = IncrementalLM(m, max_streams=B, max_len=64)
    st = lm.start(B)
    nll = lm.step(st, src[:4], targets=tg[3].to(dev))
    assert rel(nll, -ref[3].gather(1, tg[3].unsqueeze(1)).squeeze(1)) < TOL
    nll = lm.step(st, src[4:], all_positions=True, targets=tg[4:].to(dev))
    assert rel(nll, -ref[4:].gather(2, tg[4:].unsqueeze(2)).squeeze(2)) < TOL


def _full_logprobs(m, ids):
    with torch.no_grad():
        return torch.log_softmax(m(ids).double(), -1)


@pytest.mark.parametrize("shape", ["cfg2", "cfg4", "hd100", "hd128"])
def test_long_context_against_full_forward(dev, shape):
    """Context 1024: the full forward takes the long-sequence attention kernels; the incremental path a 1000-token prompt in pieces,
    then single tokens and a chunk."""
    from bayeslms_amd import model as M
    from bayeslms_amd.incremental import IncrementalLM
    torch.manual_seed(5)
    V = 2000
    if shape == "cfg2":
        m = M.BayesTransformerModel(V, 512, 8, 4096, 6, 0.1, True, "FFN")
    elif shape == "cfg4":
        m = M.GaussTransformerModel(V, 512, 8, 2048, 6, 0.1, True, 3)
    elif shape == "hd100":
        m = M.TransformerModel(V, 200, 2, 200, 2, 0.1, "gelu", True)
    else:
        m = M.BayesTransformerModel(V, 256, 2, 512, 2, 0.1, True, "MHA")
    m = m.to(dev).eval()
    T, B = 1024, 2
    src = torch.randint(0, V, (T, B), device=dev)
    ref = _full_logprobs(m, src)
    lm = IncrementalLM(m, max_streams=4, max_len=T)
    st = lm.start(B)
    lp = lm.step(st, src[:1000], all_positions=True)
    assert rel(lp[[0, 1, 255, 256, 999]], ref[[0, 1, 255, 256, 999]]) < TOL
    for t in range(1000, 1010):
        assert rel(lm.step(st, src[t]), ref[t]) < TOL, t
    lp = lm.step(st, src[1010:], all_positions=True)
    assert rel(lp, ref[1010:]) < TOL


def _lstm(kind, dev):
    from bayeslms_amd import model as M
    torch.manual_seed(3)
    V, H = 120, 64
    if kind == "none":
        m = M.RNNModel("LSTM", V, H, H, 2, 0.2, True)
    elif kind == "bayes3":
        m = M.BayesRNNModel("LSTM", V, H, H, 2, 0.2, True, 3)
    elif kind == "gauss33":
        m = M.GaussRNNModel("LSTM", V, H, H, 2, 0.2, False, "33")
    else:
        m = M.VariationalRNNModel("LSTM", V, H, H, 2, 0.2, True, "11")
    return m.to(dev).eval(), V


@pytest.mark.parametrize("kind", ["none", "bayes3", "gauss33", "var11"])
def test_lstm_families_against_full_forward(dev, kind):
    from bayeslms_amd.incremental import IncrementalLM
    m, V = _lstm(kind, dev)
    T, B = 9, 3
    src = torch.randint(0, V, (T, B), device=dev)
    with torch.no_grad():
        logits, _ = m(src, m.init_hidden(B))
    ref = torch.log_softmax(logits.double(), -1)
    lm = IncrementalLM(m, max_streams=4, max_len=T)
    st = lm.start(B)
    assert rel(lm.step(st, src[:4], all_positions=True), ref[:4]) < TOL
    for t in range(4, T):
        assert rel(lm.step(st, src[t]), ref[t]) < TOL
    st = lm.start(B)
    k = [5, 2, 7]
    lp = lm.step(st, src[:7], n_new=k, all_positions=True)
    for n in range(B):
        assert rel(lp[:k[n], n], ref[:k[n], n]) < TOL
    rest = torch.zeros(T - 2, B, dtype=torch.int64, device=dev)
    for n in range(B):
        rest[:T - k[n], n] = src[k[n]:, n]
    assert rel(lm.step(st, rest, n_new=[T - x for x in k]), ref[T - 1]) < TOL


@pytest.mark.parametrize("kind", ["transformer", "lstm"])
def test_beams_prune_fork_continue(dev, kind):
    """Random prune / fork, then continue: equal to fresh streams fed the forked histories; targets= NLL equals the gathered
    log-probs."""
    from bayeslms_amd import model as M
    from bayeslms_amd.incremental import IncrementalLM
    torch.manual_seed(9)
    if kind == "transformer":
        V = 97
        m = M.BayesTransformerModel(V, 64, 4, 128, 2, 0.1, True, "MHA").to(dev).eval()
    else:
        m, V = _lstm("bayes3", dev)
    rng = np.random.default_rng(0)
    N = 5
    hist = torch.randint(0, V, (6, N), device=dev)
    lm = IncrementalLM(m, max_streams=8, max_len=32)
    st = lm.start(N)
    lm.step(st, hist, n_new=[6, 3, 5, 6, 1])
    lens = [6, 3, 5, 6, 1]
    hs = [hist[:lens[n], n] for n in range(N)]
    for _ in range(3):
        idx = rng.integers(0, st.n, size=int(rng.integers(2, 9)))  # forks (repeats) and prunes
        st = lm.reorder(st, torch.tensor(idx))
        hs = [hs[i] for i in idx]
        assert st.lengths == [len(h) for h in hs]
        nxt = torch.randint(0, V, (st.n,), device=dev)
        lp = lm.step(st, nxt)
        hs = [torch.cat([h, nxt[j:j + 1]]) for j, h in enumerate(hs)]
    # fresh streams fed the forked histories in one ragged chunk
    fresh = lm.start(len(hs))
    L = max(len(h) for h in hs)
    pad = torch.zeros(L, len(hs), dtype=torch.int64, device=dev)
    for j, h in enumerate(hs):
        pad[:len(h), j] = h
    ref = lm.step(fresh, pad, n_new=[len(h) for h in hs])
    assert rel(lp, ref) < 1e-5
    # targets=: the NLL of given next words equals the negative of the gathered log-probs (fresh holds the same histories)
    tg, tg2 = torch.randint(0, V, (st.n,), device=dev), torch.randint(0, V, (st.n,), device=dev)
    lp2 = lm.step(st, tg)
    nll = lm.step(fresh, tg, targets=tg2)
    assert rel(nll, -lp2.gather(1, tg2.unsqueeze(1)).squeeze(1)) < 1e-5
    old = st
    st = lm.reorder(st, [0])
    with pytest.raises(BayesLMError):
        lm.step(old, tg[:1])  # consumed by reorder


# ------------------------------------------------------------------------------------------------------- scorer fixtures
def _scorer_model(name, tmp_path, dev):
    """The scorer fixture's model as the reference scorer builds it: its flags (compute_sentence_scores.build_models) and its
    model.pt (the fixture's state_dict, or -- the configs[1] / [2] / [4] fixtures -- the constructor under the fixture's seed)."""
    from bayeslms_amd import compute_sentence_scores as S
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    words = list(g["words"]) if "words" in g.files else ["<s>", "<unk>"] + ["w%d" % i for i in range(int(g["words_n"]) - 2)]
    args = S.build_parser().parse_args(["--nbest-list", "-", "--outfile", "-", "--vocabulary", "-", "--model-path", "-"] +
                                       [str(a) for a in g["argv"]])
    assert args.interpolation_flag == 0
    if "seed" in g.files:
        torch.manual_seed(int(g["seed"]))
        m, _ = S.build_models(args, len(words))
    else:
        m, _ = S.build_models(args, len(words))
        path = str(tmp_path / "model.pt")
        torch.save({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}, path)
        S.load_partial(m, path)  # by name and shape, as the scorer loads it (the fixture's short positional table is skipped)
    nbest = {}
    for line in str(g["nbest_txt"]).splitlines():
        parts = line.strip().split(" ", 1)
        key, hyp = (parts[0], parts[1]) if len(parts) == 2 else (line.strip(), " ")
        nbest.setdefault(key.rsplit("-", 1)[0], []).append(hyp)
    want = [(ln.split()[0], float(ln.split()[1])) for ln in str(g["scores_txt"]).splitlines()]
    return m.to(dev).eval(), {w: i for i, w in enumerate(words)}, nbest, want, args.model


@pytest.mark.parametrize("name", ["scorer_tlm_ffn", "scorer_tlm_gauss3", "scorer_lstm_bayes3", "scorer_lstm_gauss33",
                                  "scorer_lstm_var11", "scorer_cfg1_from_seed", "scorer_cfg2_from_seed", "scorer_cfg4_from_seed"])
def test_scorer_fixtures_rescored_incrementally(dev, name, tmp_path):
    """The reference scorer's score files, rescored through IncrementalLM: per utterance, one stream takes <s>, reorder() forks
    it into one stream per hypothesis, and a ragged chunk feeds each hypothesis' words (an empty hypothesis takes none) with its
    next words as targets; score = NLL of hyp + <s>.  LSTMs carry the state as the reference does (compute_scores): every
    hypothesis of an utterance starts from the state left by the FIRST hypothesis of the previous one; Transformers start each
    utterance from an empty stream.  Every score within 1e-4 relative."""
    from bayeslms_amd import compute_sentence_scores as S
    from bayeslms_amd.incremental import IncrementalLM
    m, vocab, nbest, want, mtype = _scorer_model(name, tmp_path, dev)
    H = max(len(h) for h in nbest.values())
    # a carried LSTM stream grows over the whole file (its state does not depend on max_len); a Transformer's over one utterance
    lm = IncrementalLM(m, max_streams=H, max_len=64 if mtype == "Transformer" else 4096)
    st = lm.start(1)
    got = []
    for key, hyps in nbest.items():
        if mtype == "Transformer":
            st = lm.start(1)
        lp0 = lm.step(st, torch.tensor([vocab["<s>"]]))  # (1, V): the first word after <s>
        st = lm.reorder(st, [0] * len(hyps))
        xs, ts = zip(*(S.get_input_and_target(h, vocab) for h in hyps))
        score = [-float(lp0[0, t[0]]) for t in ts]
        L = max(len(x) for x in xs) - 1  # words after <s>
        if L > 0:
            ids = torch.zeros(L, len(hyps), dtype=torch.int64)
            tgt = torch.zeros(L, len(hyps), dtype=torch.int64)
            for j, (x, t) in enumerate(zip(xs, ts)):
                ids[:len(x) - 1, j] = torch.tensor(x[1:])
                tgt[:len(t) - 1, j] = torch.tensor(t[1:])
            nll = lm.step(st, ids, n_new=[len(x) - 1 for x in xs], all_positions=True, targets=tgt).cpu()
            for j, x in enumerate(xs):
                score[j] += float(nll[:len(x) - 1, j].double().sum())
        got += [("%s-%d" % (key, j + 1), s) for j, s in enumerate(score)]
        st = lm.reorder(st, [0])  # LSTMs: the first hypothesis' state goes on to the next utterance
    assert [k for k, _ in got] == [k for k, _ in want]
    worst = max(abs(a - b) / max(1.0, abs(b)) for (_, a), (_, b) in zip(got, want))
    assert worst <= 1e-4, worst


# ---------------------------------------------------------------------------------------------------------------------- CLI
def _cli_model(tmp_path, dev):
    from bayeslms_amd import model as M
    torch.manual_seed(21)
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(38)]
    V = len(words)
    m = M.TransformerModel(V, 32, 2, 64, 2, 0.2, "gelu", True)
    path = tmp_path / "model.pt"
    with open(path, "wb") as f:
        torch.save({k: v.detach().cpu() for k, v in m.state_dict().items()}, f)
    voc = tmp_path / "words.txt"
    voc.write_text("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    return m.to(dev).eval(), words, str(path), str(voc)


def _run_cli(args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "bayeslms_amd.generate"] + args, capture_output=True, text=True, timeout=600, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def test_generate_cli(dev, tmp_path):
    m, words, path, voc = _cli_model(tmp_path, dev)
    common = ["--model-path", path, "--vocabulary", voc, "--model", "Transformer", "--emsize", "32", "--nhid", "64", "--nlayers", "2",
              "--nhead", "2"]
    out = tmp_path / "g.txt"
    _run_cli(common + ["--words", "12", "--temperature", "0", "--prompt", "w3 nosuchword w7", "--outf", str(out)])
    got = out.read_text().split("\n")[0].split()
    assert len(got) == 12
    w2i = {w: i for i, w in enumerate(words)}
    ctx = [w2i["<s>"], w2i["w3"], w2i["<unk>"], w2i["w7"]]
    for w in got:  # argmax generation by full recompute at every step
        with torch.no_grad():
            lg = m(torch.tensor(ctx, device=dev).view(-1, 1))[-1, 0].double()
        top = torch.topk(lg, 2)
        if w != words[int(top.indices[0])]:
            assert float(top.values[0] - top.values[1]) < 1e-5
        ctx.append(w2i[w])
    o1, o2 = tmp_path / "s1.txt", tmp_path / "s2.txt"
    for o in (o1, o2):
        _run_cli(common + ["--words", "7", "--temperature", "1.0", "--seed", "5", "--streams", "3", "--outf", str(o)])
    assert o1.read_text() == o2.read_text()
    lines = o1.read_text().splitlines()
    assert len(lines) == 3 and all(len(line.split()) == 7 for line in lines)
