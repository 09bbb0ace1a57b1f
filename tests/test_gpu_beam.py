"""GPU: the k best next words, beam search and top-k / nucleus sampling on the incremental path (csrc/beam.hip,
bayeslms_amd/incremental.py beam_search, generate.py).

blm_topk_rows and blm_beam_select are held EXACTLY (values bitwise, ids) to the numpy models of tests/beam_reference.py;
IncrementalLM.beam_search to a driver over step / host selection / host-index reorder, to greedy generation, to the brute-force
enumeration of all continuations and to rescoring from scratch; filtered sampling to the unfiltered draw, the float64 allowed
set and the renormalised frequencies."""
import itertools

import numpy as np
import pytest
import torch

import beam_reference as REF
from conftest import ROOT
from test_gpu_incremental import TOL, _cli_model, _fixture_model, _lstm, _run_cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _L():
    from bayeslms_amd import _lib as L
    L.require_gfx950()
    return L, L.lib()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ blm_topk_rows
def _rows(R, V, seed):
    """rows of random normals, rows quantised to 16 levels, all-equal, -inf runs, all-NaN, descending, ascending -- in turn"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((R, V)).astype(np.float32)
    for r in range(R):
        kind = r % 8
        if kind == 1:
            x[r] = np.round(x[r] * 4).clip(-8, 7) / 4
        elif kind == 2:
            x[r] = -3.25
        elif kind == 3:
            a = int(rng.integers(0, V))
            x[r, a:a + max(1, V // 3)] = -np.inf
            x[r, ::5] = -np.inf
        elif kind == 4:
            x[r] = np.nan
        elif kind == 5:
            x[r] = -np.arange(V, dtype=np.float32) * 0.5
        elif kind == 6:
            x[r] = np.arange(V, dtype=np.float32) * 0.5
        elif kind == 7:
            x[r, rng.integers(0, V, size=max(1, V // 7))] = np.nan
            x[r, rng.integers(0, V, size=max(1, V // 9))] = 0.0
            x[r, rng.integers(0, V, size=max(1, V // 9))] = -0.0
    return x


@pytest.mark.parametrize("V", [1, 7, 50, 4096, 33000, 33278])
@pytest.mark.parametrize("R", [1, 8, 64, 513])
def test_topk_rows_equals_lexsort_exactly(dev, V, R):
    L, lib = _L()
    ldx = V + 5
    host = _rows(R, V, 100 * V + R)
    x = torch.full((R, ldx), float("inf"), device=dev)  # the padding would win if it were read
    x[:, :V] = torch.from_numpy(host).to(dev)
    order = np.stack([REF.row_order(r)[:L.TOPK_MAX] for r in host])
    for k in sorted({1, 2, 8, 63, 64, L.TOPK_MAX}):
        if k > V:
            continue
        out = []
        for _ in range(2):
            vals = torch.full((R, k), 7.0, device=dev)
            ids = torch.full((R, k), -1, dtype=torch.int64, device=dev)
            L.check(lib.blm_topk_rows(x.data_ptr(), ldx, R, V, k, vals.data_ptr(), ids.data_ptr(), L.stream()), "blm_topk_rows")
            out.append((vals.cpu().numpy(), ids.cpu().numpy()))
        want_ids = order[:, :k]
        assert np.array_equal(out[0][1], want_ids), (V, R, k)
        assert np.array_equal(_bits(out[0][0]), _bits(np.take_along_axis(host, want_ids, 1))), (V, R, k)
        assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(_bits(out[0][0]), _bits(out[1][0]))
    if V >= 8:  # the wrapper, on a contiguous matrix
        from bayeslms_amd import ops
        v, i = ops.topk_rows(torch.from_numpy(host).to(dev), 8)
        assert np.array_equal(i.cpu().numpy(), order[:, :8]) and v.dtype == torch.float32 and i.dtype == torch.int64


# ---------------------------------------------------------------------------------------------------------- blm_beam_select
@pytest.mark.parametrize("G", [1, 3, 16])
@pytest.mark.parametrize("B", [1, 4, 8, 64])
def test_beam_select_equals_the_float32_model_bit_for_bit(dev, G, B):
    from bayeslms_amd import ops
    rng = np.random.default_rng(G * 100 + B)
    n = G * B
    for k, trial in itertools.product(sorted({1, B, 2 * B + 1}), range(3)):
        cv = np.round(rng.standard_normal((n, k)) * 3).astype(np.float32) / 2 - 4  # coarse: many tied sums
        if trial == 2:
            cv = -np.abs(rng.standard_normal((n, k))).astype(np.float32) * 5
        ci = rng.integers(0, 12, size=(n, k)).astype(np.int64)
        score = (np.round(rng.standard_normal(n) * 2) / 2).astype(np.float32)
        finished = (rng.random(n) < 0.3).astype(np.uint8)
        if trial == 1:  # the start state of a search
            score[:] = -np.inf
            score[::B] = 0.0
            finished[:] = 0
        want = REF.beam_select(cv, ci, score, finished, B, eos=3)
        got = ops.beam_select(torch.from_numpy(cv).to(dev), torch.from_numpy(ci).to(dev), torch.from_numpy(score).to(dev),
                              torch.from_numpy(finished).to(dev), B, 3)
        got = [t.cpu().numpy() for t in got]
        assert np.array_equal(_bits(got[0]), _bits(want[0])), (G, B, k, trial)
        for a, b in zip(got[1:], want[1:]):
            assert np.array_equal(a, b), (G, B, k, trial)
        assert ((got[2] // B) == (np.arange(n) // B)).all()  # parents stay inside the group


# ------------------------------------------------------------------------------------------------------------ the search
def _model(name, dev):
    if name.startswith("lstm_"):
        return _lstm(name[5:], dev)[0]
    return _fixture_model(name, dev)[0]


MODELS = ["transformer_baseline", "bayes_tlm_FFN", "gauss_tlm_3", "lstm_bayes3"]


def _prompts(V, rng, G):
    return [[0] + [int(t) for t in rng.integers(1, V, size=int(rng.integers(0, 4)))] for _ in range(G)]


def _host_rows(B):
    def select(lp):
        return REF.topk_rows(lp.cpu().numpy(), B)
    return select


@pytest.mark.parametrize("name,mc", [(n, 0) for n in MODELS] + [("bayes_tlm_FFN", 4), ("lstm_bayes3", 4)])
def test_device_reorder_equals_host_reorder(dev, name, mc):
    """both model kinds, with and without mc_samples: the next step's log-probs bit-equal"""
    from bayeslms_amd.incremental import IncrementalLM
    lm = IncrementalLM(_model(name, dev), max_streams=8, max_len=16, mc_samples=mc)
    V = lm.vocab
    rng = np.random.default_rng(4)
    ids = torch.from_numpy(rng.integers(0, V, size=(3, 6))).to(dev)
    idx = np.array([1, 0, 0, 2, 5, 3])  # forks and a prune; every stream has length 3, so the promise holds
    nxt = torch.from_numpy(rng.integers(0, V, size=6)).to(dev)
    outs = []
    for device_index in (False, True):
        st = lm.start(6)
        lm.step(st, ids)
        st = lm.reorder_device(st, torch.from_numpy(idx).to(dev)) if device_index else lm.reorder(st, idx)
        assert st.lengths == [3] * 6
        outs.append(lm.step(st, nxt).cpu().numpy())
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize("name", MODELS)
def test_beam_search_equals_the_host_driver_bit_for_bit(dev, name):
    """tokens, parents and fp32 scores against step + full rows on the host + the numpy selection model + host-index reorder:
    both sides run the same launches on the same state"""
    from bayeslms_amd.incremental import IncrementalLM
    m = _model(name, dev)
    rng = np.random.default_rng(11)
    for G, B, W in ((1, 4, 6), (3, 5, 5)):
        lm = IncrementalLM(m, max_streams=G * B, max_len=4 + W)
        prompts = _prompts(lm.vocab, rng, G)
        P, T, s = lm._beam_trace(prompts, B, W, 0, sync_every=0)
        Pw, Tw, sw = REF.beam_search_old_api(lm, prompts, B, W, 0, _host_rows(B))
        assert np.array_equal(P, Pw) and np.array_equal(T, Tw) and np.array_equal(_bits(s), _bits(sw)), (name, G, B)


def _greedy(lm, prompt, W):
    from bayeslms_amd import ops
    st = lm.start(1)
    ids = torch.tensor(prompt, dtype=torch.int64).view(-1, 1)
    out = []
    for i in range(W):
        nxt = ops.sample_rows(lm.step(st, ids), 0.0)
        out.append(int(nxt))
        ids = nxt.view(1, 1)
    return out


def _rescore(lm, prompt, toks):
    """log-probability of toks after prompt, from scratch: one chunk with all_positions and targets"""
    st = lm.start(1)
    seq = list(prompt) + list(toks)
    ids = torch.tensor(seq[:-1], dtype=torch.int64).view(-1, 1)
    tg = torch.tensor(seq[1:], dtype=torch.int64).view(-1, 1)
    nll = lm.step(st, ids, all_positions=True, targets=tg).double().cpu().numpy()[:, 0]
    return -float(nll[len(prompt) - 1:].sum())


@pytest.mark.parametrize("name,mc", [(n, 0) for n in MODELS] + [("bayes_tlm_FFN", 4)])
def test_beam_search_against_greedy_brute_force_and_rescoring(dev, name, mc):
    from bayeslms_amd.incremental import IncrementalLM
    m = _model(name, dev)
    V = m.decoder.weight.shape[0]
    lm = IncrementalLM(m, max_streams=max(V, 12), max_len=16, mc_samples=mc)
    prompt = [0, 5, 9]
    # beam 1 is greedy generation (cut at the first eos)
    W = 8
    h = lm.beam_search([prompt], 1, W, 0)[0][0]
    g = _greedy(lm, prompt, W)
    g = g[:g.index(0) + 1] if 0 in g else g
    assert h.tokens == g and h.length == len(g)
    # beam = V, two words: the exact top V of all one- and two-word continuations (a one-word hypothesis ends in eos)
    st = lm.start(1)
    lp1 = lm.step(st, torch.tensor(prompt).view(-1, 1)).double().cpu().numpy()[0]
    st = lm.reorder(st, [0] * V)
    lp2 = lm.step(st, torch.arange(V)).double().cpu().numpy()
    brute = {(0,): lp1[0]}
    for a in range(1, V):
        for b in range(V):
            brute[(a, b)] = lp1[a] + lp2[a, b]
    want = sorted(brute.items(), key=lambda kv: -kv[1])[:V]
    got = lm.beam_search([prompt], V, 2, 0, length_penalty=0.0)[0]
    assert len(got) == V
    for r, (hyp, (toks, sc)) in enumerate(zip(got, want)):
        assert abs(hyp.score - sc) <= TOL * max(1.0, abs(sc)), (r, hyp, toks, sc)
        near = (r > 0 and abs(want[r - 1][1] - sc) <= TOL) or (r + 1 < V and abs(want[r + 1][1] - sc) <= TOL)
        if not near:
            assert tuple(hyp.tokens) == toks, (r, hyp, toks)
    # every score equals the hypothesis rescored from scratch; ragged prompts in one call equal one by one; sync_every
    prompts = [[0], [0, 3, 7, 2], [0, 11]]
    B, W = 4, 6
    many = lm.beam_search(prompts, B, W, 0, length_penalty=0.7)
    for p, hyps in zip(prompts, many):
        one = lm.beam_search([p], B, W, 0, length_penalty=0.7)[0]
        assert [(h.tokens, h.length) for h in hyps] == [(h.tokens, h.length) for h in one]
        assert all(abs(a.score - b.score) <= TOL * max(1.0, abs(b.score)) for a, b in zip(hyps, one))
        for h in hyps:
            ref = _rescore(lm, p, h.tokens)
            assert abs(h.score - ref) <= TOL * max(1.0, abs(ref)), (h, ref)
        keys = [h.score / h.length ** 0.7 for h in hyps]
        assert keys == sorted(keys, reverse=True)
    for se in (0, 1, 16):
        again = lm.beam_search(prompts, B, W, 0, length_penalty=0.7, sync_every=se)
        assert again == many, se
    lp = lm.step(lm.start(1), torch.tensor(prompt).view(-1, 1))
    vals, ids = lm.step_topk(lm.start(1), torch.tensor(prompt).view(-1, 1), 5)
    wv, wi = REF.topk_rows(lp.cpu().numpy(), 5)
    assert np.array_equal(ids.cpu().numpy(), wi) and np.array_equal(_bits(vals.cpu().numpy()), _bits(wv))


# --------------------------------------------------------------------------------------------------------- filtered sampling
def test_filtered_sampling(dev):
    from bayeslms_amd import ops
    rng = np.random.default_rng(2)
    x = torch.randn(64, 500, device=dev)
    x[3, 10] = x[3, 400] = 50.0
    a = ops.sample_rows(x, 0.8, 7, 1, 3)
    L, lib = _L()
    out = torch.empty(64, dtype=torch.int64, device=dev)
    r = L.rng(7, 1, 3)
    import ctypes as C
    L.check(lib.blm_sample_rows_filtered(x.data_ptr(), 500, 64, 500, 0.8, 0, 1.0, C.byref(r), out.data_ptr(), L.stream()), "filtered")
    assert torch.equal(out, a)  # top_k = 0, top_p = 1: the unfiltered draw, id for id
    assert torch.equal(ops.sample_rows(x, 0.8, 7, 1, 3, top_k=1), ops.sample_rows(x, 0.0))
    assert torch.equal(ops.sample_rows(x, 0.8, 7, 1, 3, top_p=1e-6), ops.sample_rows(x, 0.0))
    assert torch.equal(ops.sample_rows(x, 0.0, top_k=3, top_p=0.5), ops.sample_rows(x, 0.0))
    # no draw outside the float64 allowed set, on rows whose cut has a margin of 1e-3 in q-mass on either side
    V = 33000
    # Zipf-like rows (exponent 1.5 .. 2.55, ranks permuted, a little jitter): peaked enough that the word at a nucleus cut
    # carries more than 2e-3 of the mass, without which no cut could have the margin
    host = np.stack([-(1.5 + 0.15 * (r % 8)) * np.log1p(rng.permutation(V)) + 0.01 * rng.standard_normal(V) for r in range(24)])
    host = host.astype(np.float32)
    host[5, ::3] = host[5, 1]  # a row with many ties (only the cases it has a margin in use it)
    xs = torch.from_numpy(host).to(dev)
    for temperature, top_k, top_p in ((1.0, 0, 0.9), (0.7, 50, 1.0), (1.3, 2000, 0.8), (1.0, 3, 0.5), (1.0, 0, 0.6), (1.0, 5000, 1.0)):
        masks, rows = [], []
        for rr in range(host.shape[0]):
            mk, before, after = REF.allowed_set(host[rr], temperature, top_k, top_p)
            if before is None or (top_p - before >= 1e-3 and after - top_p >= 1e-3):
                masks.append(mk)
                rows.append(rr)
        assert len(rows) >= 8, (temperature, top_k, top_p, len(rows))
        sel = xs[rows].contiguous()
        for step in range(6):
            ids = ops.sample_rows(sel, temperature, 5, 0, step, top_k=top_k, top_p=top_p).cpu().numpy()
            inside = [bool(masks[j][ids[j]]) for j in range(len(rows))]
            assert all(inside), (temperature, top_k, top_p, step)
            base = ops.sample_rows(sel, temperature, 5, 0, step).cpu().numpy()  # the same noise: unchanged when already inside
            assert all(ids[j] == base[j] for j in range(len(rows)) if masks[j][base[j]])
    # frequencies: R = 2^16 rows of one 16-word distribution, every count within 4 standard errors of R x renormalised p
    R, V = 1 << 16, 16
    torch.manual_seed(0)
    logits = torch.randn(V) * 1.5
    p = torch.softmax(logits.double(), 0).numpy()
    xr = logits.to(dev).expand(R, V).contiguous()
    for kw in (dict(top_k=5), dict(top_p=0.8)):
        mask, before, after = REF.allowed_set(logits.double().numpy(), 1.0, kw.get("top_k", 0), kw.get("top_p", 1.0))
        if before is not None:
            assert 0.8 - before >= 1e-3 and after - 0.8 >= 1e-3
        q = np.where(mask, p, 0.0)
        q /= q.sum()
        ids = ops.sample_rows(xr, 1.0, 11, 2, 0, **kw)
        cnt = np.bincount(ids.cpu().numpy(), minlength=V).astype(np.float64)
        se = np.sqrt(R * q * (1 - q))
        print(kw, "max |count - R q| / se:", float(np.max(np.abs(cnt - R * q) / np.maximum(se, 1e-30) * (q > 0))))
        assert (cnt[~mask] == 0).all() and np.all(np.abs(cnt - R * q) <= 4 * se), (kw, cnt, R * q)


# ----------------------------------------------------------------------------------------------------------------------- CLI
def test_generate_cli_beam_and_top_k(dev, tmp_path):
    from bayeslms_amd import generate as Gn
    m, words, path, voc = _cli_model(tmp_path, dev)
    common = ["--model-path", path, "--vocabulary", voc, "--model", "Transformer", "--emsize", "32", "--nhid", "64", "--nlayers", "2",
              "--nhead", "2", "--prompt", "w3 w7"]
    vocab = {w: i for i, w in enumerate(words)}
    out, sc = tmp_path / "b.txt", tmp_path / "b.scores"
    _run_cli(common + ["--words", "9", "--beam", "4", "--nbest", "4", "--length-penalty", "0.5", "--outf", str(out),
                       "--write-scores", str(sc)])
    hyps = Gn.beam_generate(m, vocab, 9, 4, 4, "w3 w7", 0.5)
    assert out.read_text() == "".join(" ".join(words[i] for i in h.tokens) + "\n" for h in hyps)
    assert sc.read_text() == "".join("%d %.6f %d\n" % (r + 1, h.score, h.length) for r, h in enumerate(hyps))
    g, k = tmp_path / "g.txt", tmp_path / "k.txt"
    _run_cli(common + ["--words", "9", "--temperature", "0", "--outf", str(g)])
    _run_cli(common + ["--words", "9", "--top-k", "1", "--seed", "3", "--outf", str(k)])
    assert g.read_text() == k.read_text() and len(g.read_text().split()) == 9
