"""GPU: beam search with a pool of finished hypotheses (csrc/beam.hip blm_beam_select_pool, IncrementalLM.beam_search_pool,
generate --finished-pool).

The kernel is held bit for bit -- every output and the whole pool -- to the numpy model of tests/beam_pool_reference.py over
chained steps; beam_search_pool to the same model driven by lm.step on the host, to the search with stopping disabled, to the
brute-force enumeration of all finished sentences and to rescoring from scratch."""
import itertools

import numpy as np
import pytest
import torch

import beam_pool_reference as REF
from test_gpu_incremental import TOL, _cli_model, _run_cli

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    if np.asarray(want).dtype == np.float32:
        assert np.array_equal(_bits(got), _bits(want)), (what, got, want)
    else:
        assert np.array_equal(got, want), (what, got, want)


# ------------------------------------------------------------------------------------------------------- blm_beam_select_pool
def _candidates(rng, n, k, V, eos, step):
    """coarse non-positive values (many tied sums), ids distinct within a row, eos in most rows, -inf runs, an all-NaN row"""
    cv = -(np.round(np.abs(rng.standard_normal((n, k))) * 4) / 4).astype(F)
    ci = np.stack([rng.permutation(V)[:k] for _ in range(n)]).astype(np.int64)
    for r in range(n):
        if eos not in ci[r] and rng.random() < 0.7:
            at = int(rng.integers(0, k))
            ci[r, at] = eos  # the id it replaces is gone from the row: still distinct
            if rng.random() < 0.4:  # the sentence end is the row's best word
                cv[r] = np.minimum(cv[r], F(-0.25))
                cv[r, at] = 0.0
        if k >= 8 and rng.random() < 0.3:
            cv[r, rng.integers(0, k, size=max(1, k // 3))] = -np.inf
    if step == 4 and n > 1:
        cv[n - 1] = np.nan  # a stream that took no token
    if step == 2:
        cv[0, :] = cv[0, 0]  # a whole row of one value: the flat index decides
    return cv, ci


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("B", [1, 2, 5, 128])
def test_kernel_equals_the_float32_model_bit_for_bit_over_chained_steps(dev, G, B):
    """B = 1 and B = BLM_TOPK_MAX / 2, pools smaller and larger than the beam, a pool that overflows, min_len above the first
    two steps, dead slots, a group that is done beside one that runs on, and a flush step at the end"""
    from bayeslms_amd import ops
    V, eos, a, min_len = 300, 7, 0.6, 3
    n = G * B
    steps = 6 if B == 128 else 12 if B == 1 else 8
    seen_mixed = seen_replaced = seen_dead = False
    for k, P in itertools.product(sorted({min(2 * B, V), 256}), sorted({1, B, 7, 256})):
        rng = np.random.default_rng(1000 * G + 10 * B + k + P)
        pool_d, pool_h = ops.BeamPool(G, P, dev), REF.new_pool(G, P)
        score = np.zeros(n, F)
        live = np.zeros(n, np.uint8)
        live[::B] = 1
        for w in range(steps):
            cv, ci = _candidates(rng, n, k, V, eos, w)
            if G == 3 and w >= 3:
                cv[B:2 * B] -= 40.0  # group 1 falls behind: its bound drops below a full pool's last norm
            if w == steps - 3:
                cv[:B, 1:] = -np.inf  # one candidate per beam of group 0: with an eos among them, fewer than B new beams
            inv, inv_max, flush = REF.inv_norm(w + 1, a), REF.inv_norm(steps, a), w + 1 == steps
            want = REF.select_pool(cv, ci, score, live, B, eos, w, w + 1, min_len, inv, inv_max, flush, pool_h)
            got = ops.beam_select_pool(torch.from_numpy(cv).to(dev), torch.from_numpy(ci).to(dev), torch.from_numpy(score).to(dev),
                                       torch.from_numpy(live).to(dev), B, V, eos, w, w + 1, min_len, float(inv), float(inv_max), flush,
                                       pool_d)
            got = [t.cpu().numpy() for t in got]
            for name, x, y in zip(("score", "live", "parent", "token", "done"), got, want):
                _same(x, y, (G, B, k, P, w, name))
            assert int(got[5][0]) == int(want[5]), (G, B, k, P, w, "all_done")
            h = pool_d.host()
            for name in REF.FIELDS + ("count", "inserted"):
                _same(h[name], pool_h[name], (G, B, k, P, w, name))
            assert ((got[2] // B) == (np.arange(n) // B)).all()  # parents stay inside the group
            seen_mixed |= bool(0 < want[4].sum() < G and not flush)
            seen_replaced |= bool((pool_h["inserted"] > P).any())
            seen_dead |= bool((want[1].reshape(G, B).sum(1) < B).any() and not flush)
            score, live = want[0], want[1]
        assert want[4].all() and want[5] == 1 and not want[1].any()  # after the flush everything is done and dead
    assert seen_replaced and (seen_mixed or G == 1) and (seen_dead or B == 1)


# ------------------------------------------------------------------------------------------------------------------ the search
def _tiny(kind, dev, V=50):
    """2-layer Bayesian models over V words whose sentence end (word 0) is likely enough that hypotheses finish"""
    from bayeslms_amd import model as M
    torch.manual_seed(5)
    if kind == "transformer":
        m = M.BayesTransformerModel(V, 32, 2, 64, 2, 0.2, True, "FFN")
    else:
        m = M.BayesRNNModel("LSTM", V, 32, 32, 2, 0.2, True, 3)
    with torch.no_grad():
        # a fresh model's logits are 32 products of a unit-size state and weights in (-0.1, 0.1): a spread near 0.33, so the
        # best of the other 49 words sits near 0.75 and the sentence end at 1.5 is the best word of most steps
        m.decoder.bias[0] += 1.5
    return m.to(dev).eval()


def _rescore(lm, prompt, toks):
    """log-probability of toks after prompt, from scratch: one chunk with all_positions and targets"""
    st = lm.start(1)
    seq = list(prompt) + list(toks)
    ids = torch.tensor(seq[:-1], dtype=torch.int64).view(-1, 1)
    tg = torch.tensor(seq[1:], dtype=torch.int64).view(-1, 1)
    nll = lm.step(st, ids, all_positions=True, targets=tg).double().cpu().numpy()[:, 0]
    return -float(nll[len(prompt) - 1:].sum())


def _plain(hyps):
    return [[(h.tokens, _bits(h.score).item(), _bits(h.norm_score).item(), h.length, h.finished) for h in one] for one in hyps]


@pytest.mark.parametrize("kind,mc", [("transformer", 0), ("transformer", 2), ("lstm", 0), ("lstm", 2)])
def test_beam_search_pool_equals_the_numpy_loop_and_does_not_depend_on_when_it_stops(dev, kind, mc):
    from bayeslms_amd.incremental import IncrementalLM
    m = _tiny(kind, dev)
    prompts = [[0], [0, 3, 7, 2], [0, 11]]
    G, B, P, W, a, min_words = len(prompts), 3, 5, 7, 0.8, 2
    lm = IncrementalLM(m, max_streams=G * B, max_len=4 + W, mc_samples=mc)
    got = lm.beam_search_pool(prompts, B, W, 0, pool=P, length_penalty=a, min_words=min_words)
    want = REF.search_lm(lm, prompts, B, W, 0, P, a, min_words)
    assert _plain(got) == [[(t, _bits(r).item(), _bits(nm).item(), ln, f) for t, r, nm, ln, f in one] for one in want]
    for se in (0, 1, 16):
        assert _plain(lm.beam_search_pool(prompts, B, W, 0, pool=P, length_penalty=a, min_words=min_words, sync_every=se)) == _plain(got), se
    assert _plain(lm.beam_search_pool(prompts, B, W, 0, pool=P, length_penalty=a, min_words=min_words, _stop=False)) == _plain(got)
    assert any(h.finished for one in got for h in one)
    for p, one in zip(prompts, got):
        assert 1 <= len(one) <= P
        keys = [h.norm_score for h in one]
        assert keys == sorted(keys, reverse=True)
        for h in one:
            assert h.length == len(h.tokens) and (h.tokens[-1] == 0) == h.finished and 0 not in h.tokens[:-1]
            assert not h.finished or h.length >= min_words
            assert _bits(h.norm_score) == _bits(F(h.score) * REF.inv_norm(h.length, a))
            ref = _rescore(lm, p, h.tokens)  # the raw score is the hypothesis rescored from scratch
            assert abs(h.score - ref) <= TOL * max(1.0, abs(ref)), (h, ref)
    # the default pool is the beam
    assert all(len(one) <= B for one in lm.beam_search_pool(prompts, B, W, 0))


def test_a_wide_beam_finds_every_finished_sentence(dev):
    """V = 4, 4 words, 128 beams: nothing is pruned, so the pool holds all 1 + 3 + 9 + 27 finished sentences ranked by
    normalised score, and the 81 that are still alive after 4 words"""
    from bayeslms_amd import model as M
    from bayeslms_amd.incremental import IncrementalLM
    torch.manual_seed(9)
    V, W, a = 4, 4, 0.5
    m = M.TransformerModel(V, 32, 2, 64, 2, 0.2, "gelu", True)
    with torch.no_grad():
        m.encoder.weight.mul_(8.0)
    lm = IncrementalLM(m.to(dev).eval(), max_streams=128, max_len=2 + W)
    prompt = [0, 2]
    got = lm.beam_search_pool([prompt], 128, W, 0, pool=256, length_penalty=a)[0]
    fin = [h for h in got if h.finished]
    assert len(fin) == 40 and len(got) == 121
    brute = []
    for n in range(W):
        for body in itertools.product(range(1, V), repeat=n):
            toks = list(body) + [0]
            sc = _rescore(lm, prompt, toks)
            brute.append((toks, sc, sc / len(toks) ** a))
    brute.sort(key=lambda e: -e[2])
    assert sorted(map(tuple, (h.tokens for h in fin))) == sorted(tuple(t) for t, _, _ in brute)
    for r, (h, (toks, sc, nm)) in enumerate(zip(fin, brute)):
        assert abs(h.score - sc) <= TOL * max(1.0, abs(sc)) and abs(h.norm_score - nm) <= TOL * max(1.0, abs(nm)), (r, h, toks, sc, nm)
        near = (r > 0 and abs(brute[r - 1][2] - nm) <= TOL) or (r + 1 < len(brute) and abs(brute[r + 1][2] - nm) <= TOL)
        if not near:
            assert h.tokens == toks, (r, h, toks)


# ----------------------------------------------------------------------------------------------------------------------- CLI
def test_generate_cli_finished_pool(dev, tmp_path):
    from bayeslms_amd import generate as Gn
    m, words, path, voc = _cli_model(tmp_path, dev)
    with torch.no_grad():  # the sentence end likely enough that hypotheses finish; saved again for the command line
        m.decoder.bias[0] += 1.5
    with open(path, "wb") as f:
        torch.save({k: v.detach().cpu() for k, v in m.state_dict().items()}, f)
    common = ["--model-path", path, "--vocabulary", voc, "--model", "Transformer", "--emsize", "32", "--nhid", "64", "--nlayers", "2",
              "--nhead", "2", "--prompt", "w3 w7", "--words", "9"]
    vocab = {w: i for i, w in enumerate(words)}
    out, sc = tmp_path / "p.txt", tmp_path / "p.scores"
    _run_cli(common + ["--beam", "3", "--finished-pool", "8", "--nbest", "8", "--min-words", "2", "--length-penalty", "0.5", "--outf",
                       str(out), "--write-scores", str(sc)])
    hyps = Gn.pool_generate(m, vocab, 9, 3, 8, 8, "w3 w7", 0.5, 2)
    assert len(hyps) == 8 and len(out.read_text().splitlines()) == 8
    assert out.read_text() == "".join(" ".join(words[i] for i in h.tokens) + "\n" for h in hyps)
    assert sc.read_text() == "".join("%d %.6f %.6f %d%s\n" % (r + 1, h.score, h.norm_score, h.length, "" if h.finished else " unfinished")
                                     for r, h in enumerate(hyps))
    assert all(h.length >= 2 for h in hyps if h.finished)
    # without the new flags the command writes what it wrote before
    old, olds = tmp_path / "b.txt", tmp_path / "b.scores"
    _run_cli(common + ["--beam", "4", "--nbest", "4", "--length-penalty", "0.5", "--outf", str(old), "--write-scores", str(olds)])
    hyps = Gn.beam_generate(m, vocab, 9, 4, 4, "w3 w7", 0.5)
    assert old.read_text() == "".join(" ".join(words[i] for i in h.tokens) + "\n" for h in hyps)
    assert olds.read_text() == "".join("%d %.6f %d\n" % (r + 1, h.score, h.length) for r, h in enumerate(hyps))
