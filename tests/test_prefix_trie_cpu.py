"""CPU: the prefix trie of a packed n-best batch (bayeslms_amd/prefix_trie.py) against a naive dict trie, the scorer's
--share-prefixes flag and its refusals, and the new C entry points' bindings and argument checks (no GPU)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from bayeslms_amd.prefix_trie import build_trie

HEADER = os.path.join(ROOT, "include", "bayeslm.h")
LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")
FAKE = 4096  # a non-NULL address that is never dereferenced: validation returns first


def _batch(rng, n_utt, vocab=6):
    """Random n-best lists in the scorer's layout: input ids '<s> hyp' (id 0 = <s>), targets 'hyp <s>'.  Small vocabularies
    and derived hypotheses give duplicates, prefix hypotheses, empty hypotheses and one-hypothesis utterances."""
    cols, utt = [], []
    for u in range(n_utt):
        kind = rng.integers(4)
        base = list(rng.integers(1, vocab, size=rng.integers(0, 9)))
        hyps = [base]
        n = 1 if kind == 0 else int(rng.integers(2, 40 if kind == 3 else 12))
        for _ in range(n - 1):
            h = list(hyps[int(rng.integers(len(hyps)))] if rng.random() < 0.5 else base)
            op = rng.integers(5)
            if op == 0 and h:
                h = h[: rng.integers(0, len(h))]             # a prefix (possibly empty)
            elif op == 1:
                h = h + list(rng.integers(1, vocab, size=rng.integers(1, 5)))
            elif op == 2 and h:
                i = rng.integers(len(h))
                h[i] = int(rng.integers(1, vocab))
            elif op == 3:
                h = []
            hyps.append(h)                                  # op 4: a duplicate
        rng.shuffle(hyps)
        for h in hyps:
            cols.append(([0] + [int(w) for w in h], [int(w) for w in h] + [0]))
            utt.append(u)
    order = rng.permutation(len(cols)) if rng.random() < 0.3 else np.arange(len(cols))  # columns of an utterance need not be adjacent
    cols = [cols[i] for i in order]
    utt = np.asarray(utt)[order]
    lens = np.array([len(x) for x, _ in cols])
    Tm, N = int(lens.max()), len(cols)
    data = np.full((Tm, N), 7777, dtype=np.int64)  # garbage in the padding: it must be ignored
    for n, (x, _) in enumerate(cols):
        data[: len(x), n] = x
    tgt = np.concatenate([t for _, t in cols])
    return data, lens, tgt, utt, cols


def _naive(cols, utt):
    """dict trie per utterance: node key (utt, prefix tuple); edges (node key, target)."""
    nodes, edges = set(), set()
    for (x, t), u in zip(cols, utt):
        for i in range(len(x)):
            nodes.add((int(u), tuple(x[: i + 1])))
            edges.add(((int(u), tuple(x[: i + 1])), t[i]))
    return nodes, edges


def _check(data, lens, tgt, utt, cols):
    tr = build_trie(data, lens, tgt, utt)
    N = data.shape[1]
    M = tr.sel.shape[0]
    nodes, edges = _naive(cols, utt)
    # node identity: the (utterance, prefix) its sel row reaches
    key = []
    for i in range(M):
        t, n = divmod(int(tr.sel[i]), N)
        assert t < lens[n]
        key.append((int(utt[n]), tuple(int(v) for v in data[: t + 1, n])))
    assert len(set(key)) == M and set(key) == nodes
    # depth = position: sel's t equals the prefix length - 1 (checked through the key's length above); preorder: a node's
    # parent precedes it, each utterance is contiguous, lo is its first node, end closes exactly the node's subtree
    index = {k: i for i, k in enumerate(key)}
    for i, (u, pre) in enumerate(key):
        if len(pre) > 1:
            assert index[(u, pre[:-1])] < i
        sub = [j for j, (u2, p2) in enumerate(key) if u2 == u and p2[: len(pre)] == pre]
        assert sub == list(range(i, int(tr.end[i]))), (i, sub, tr.end[i])
        ut = [j for j, (u2, _) in enumerate(key) if u2 == u]
        assert ut == list(range(ut[0], ut[-1] + 1)) and tr.lo[i] == ut[0]
    assert tr.end.dtype == np.int32 and tr.lo.dtype == np.int32
    # edges: unique, complete, sorted by node
    ek = [(key[int(a)], int(b)) for a, b in zip(tr.edge_node, tr.edge_tgt)]
    assert len(set(ek)) == len(ek) and set(ek) == edges
    assert np.all(np.diff(tr.edge_node) >= 0)
    # tok_edge reproduces every hypothesis' target sequence, from the right node
    o = 0
    for n, (x, t) in enumerate(cols):
        for i in range(len(x)):
            e = int(tr.tok_edge[o + i])
            assert tr.edge_tgt[e] == t[i] and key[int(tr.edge_node[e])] == (int(utt[n]), tuple(x[: i + 1]))
        o += len(x)
    assert o == tr.tok_edge.shape[0]
    return tr


@pytest.mark.parametrize("seed", range(300))
def test_trie_matches_a_naive_dict_trie(seed):
    rng = np.random.default_rng(seed)
    _check(*_batch(rng, int(rng.integers(1, 7))))


def test_trie_over_128_nodes_in_one_utterance():
    rng = np.random.default_rng(12345)
    cols = []
    for _ in range(60):
        h = list(rng.integers(1, 50, size=rng.integers(3, 12)))
        cols.append(([0] + h, h + [0]))
    utt = np.zeros(len(cols), dtype=np.int64)
    lens = np.array([len(x) for x, _ in cols])
    data = np.zeros((lens.max(), len(cols)), dtype=np.int64)
    for n, (x, _) in enumerate(cols):
        data[: len(x), n] = x
    tr = _check(data, lens, np.concatenate([t for _, t in cols]), utt, cols)
    assert tr.sel.shape[0] > 128


def test_special_cases():
    # empty hypothesis ' ' (input '<s>', target '<s>'), a one-hypothesis utterance, duplicates and a prefix hypothesis
    cols = [([0], [0]), ([0, 3, 4], [3, 4, 0]), ([0, 3], [3, 0]), ([0, 3, 4], [3, 4, 0]), ([0, 5], [5, 0])]
    utt = np.array([0, 1, 1, 1, 2])
    lens = np.array([len(x) for x, _ in cols])
    data = np.zeros((3, 5), dtype=np.int64)
    for n, (x, _) in enumerate(cols):
        data[: len(x), n] = x
    tr = _check(data, lens, np.concatenate([t for _, t in cols]), utt, cols)
    assert tr.sel.shape[0] == 1 + 3 + 2            # root | root, 3, 3 4 | root, 5
    assert tr.edge_node.shape[0] == 1 + 4 + 2      # <s> | 3, (3: 4 and <s>), (3 4: <s>) | 5, <s>
    # the duplicates score the same edges
    assert list(tr.tok_edge[1:4]) == list(tr.tok_edge[6:9])


def test_chain_trie_is_the_identity_layout():
    """One hypothesis per utterance: a node per token, in the hypotheses' order."""
    cols = [([0, 1, 2], [1, 2, 0]), ([0, 2], [2, 0]), ([0, 1, 1, 1], [1, 1, 1, 0])]
    lens = np.array([3, 2, 4])
    data = np.zeros((4, 3), dtype=np.int64)
    for n, (x, _) in enumerate(cols):
        data[: len(x), n] = x
    tr = _check(data, lens, np.concatenate([t for _, t in cols]), np.arange(3), cols)
    assert list(tr.end) == [3, 3, 3, 5, 5, 9, 9, 9, 9]
    assert list(tr.lo) == [0, 0, 0, 3, 3, 5, 5, 5, 5]
    assert list(tr.tok_edge) == list(range(9))


def test_trie_refuses_bad_input():
    with pytest.raises(ValueError):
        build_trie(np.zeros((2, 2)), np.array([1, 0]), np.zeros(1), np.zeros(2))
    with pytest.raises(ValueError):
        build_trie(np.zeros((2, 2)), np.array([1, 2]), np.zeros(2), np.zeros(2))


def test_trie_build_is_vectorised():
    """20-best lists of 1000 utterances (the bench's rescoring workload) in a fraction of a naive trie's time."""
    import time
    from bench import synthetic_nbest
    from bayeslms_amd.compute_sentence_scores import get_input_and_target
    nbest, vocab, _ = synthetic_nbest(1000, 20, 33000)
    cols, utt = [], []
    for u, hyps in enumerate(nbest.values()):
        for h in hyps:
            cols.append(get_input_and_target(h, vocab))
            utt.append(u)
    lens = np.array([len(x) for x, _ in cols])
    data = np.zeros((lens.max(), len(cols)), dtype=np.int64)
    for n, (x, _) in enumerate(cols):
        data[: len(x), n] = x
    tgt = np.concatenate([t for _, t in cols])
    t0 = time.perf_counter()
    tr = build_trie(data, lens, tgt, np.asarray(utt))
    dt = time.perf_counter() - t0
    assert 0.4 < tr.sel.shape[0] / lens.sum() < 0.6  # the issue's count on this workload: 0.51
    assert dt < 0.5, dt


# ---------------------------------------------------------------------------------------------------------------- scorer CLI
def test_cli_default_is_off():
    from bayeslms_amd.compute_sentence_scores import build_parser
    a = build_parser().parse_args(["--nbest-list", "a", "--outfile", "b", "--vocabulary", "c", "--model-path", "d"])
    assert a.share_prefixes == 0
    a = build_parser().parse_args(["--nbest-list", "a", "--outfile", "b", "--vocabulary", "c", "--model-path", "d",
                                   "--share-prefixes", "1"])
    assert a.share_prefixes == 1


def _cli(*extra):
    argv = [sys.executable, "-m", "bayeslms_amd.compute_sentence_scores", "--nbest-list", "missing_nbest", "--outfile", "missing_out",
            "--vocabulary", "missing_vocab", "--model-path", "missing_model", "--share-prefixes", "1"] + list(extra)
    return subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("extra,msg", [(("--batched", "0"), "--share-prefixes 1 needs --batched 1"),
                                       (("--mc-samples", "4", "--write-uncertainty", "u.txt"),
                                        "--share-prefixes 1 does not take --write-uncertainty"),
                                       (("--share-prefixes", "2"), "invalid choice")])
def test_cli_refuses_combinations(extra, msg):
    """Refused before the input paths are checked, any model is loaded or a device is looked for."""
    r = _cli(*extra)
    assert r.returncode != 0
    assert msg in r.stderr, r.stderr


def test_scorer_refuses_uncertainty_with_shared_prefixes():
    from bayeslms_amd._lib import BayesLMError
    from bayeslms_amd.compute_sentence_scores import compute_scores_batched
    with pytest.raises(BayesLMError, match="share_prefixes"):
        compute_scores_batched({}, object(), {}, "Transformer", "cpu", mc_samples=4, uncertainty=True, share_prefixes=True)


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from bayeslms_amd import _lib
    return _lib.lib()


def test_header_declares_and_bindings_bind_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    from bayeslms_amd import _lib
    for name, nargs in (("blm_attn_fwd_tree", 11), ("blm_linear_nll_edges_ws_floats", 2), ("blm_linear_nll_edges", 15),
                        ("blm_linear_nll2_edges_ws_floats", 4), ("blm_linear_nll2_edges", 23)):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name


def _tree(lib, q=FAKE, end=FAKE, lo=FAKE, ld=256, R=100, nhead=4, hd=64):
    return lib.blm_attn_fwd_tree(q, FAKE, FAKE, ld, FAKE, end, lo, R, nhead, hd, None)


@pytest.mark.parametrize("kw,msg", [({"q": None}, b"bad arguments"), ({"end": None}, b"bad arguments"), ({"lo": None}, b"bad arguments"),
                                    ({"R": -1}, b"bad arguments"), ({"nhead": 0}, b"bad arguments"), ({"ld": 128}, b"ld_qkv too small"),
                                    ({"R": 1 << 30, "ld": 1 << 14, "nhead": 256}, b"extents")])
def test_tree_attention_argument_errors(lib, kw, msg):
    assert _tree(lib, **kw) != 0
    assert msg in lib.blm_last_error()


def test_tree_attention_head_size_limit(lib):
    from bayeslms_amd import _lib
    assert _tree(lib, hd=136, ld=136 * 4) == _lib.ERR_UNSUPPORTED
    assert b"head_dim" in lib.blm_last_error()
    assert _tree(lib, R=0) == 0


def _edges(lib, x=FAKE, en=FAKE, nll=FAKE, ws=FAKE, M=16, E=20, N=1000, nv=1000, K=64, ldx=64):
    return lib.blm_linear_nll_edges(x, ldx, FAKE, K, None, en, FAKE, nll, ws, M, E, N, nv, K, None)


@pytest.mark.parametrize("kw,msg", [({"x": None}, b"bad arguments"), ({"en": None}, b"bad arguments"), ({"N": 0}, b"bad shape"),
                                    ({"nv": 1001}, b"bad shape"), ({"E": -1}, b"bad shape"), ({"ldx": 32}, b"bad arguments"),
                                    ({"N": 1002, "nv": 1002}, b"N % 4 == 0"), ({"ws": FAKE + 4}, b"aligned"),
                                    ({"M": 1 << 30, "ldx": 1 << 12, "K": 64}, b"extents")])
def test_edge_nll_argument_errors(lib, kw, msg):
    assert _edges(lib, **kw) != 0
    assert msg in lib.blm_last_error()


def test_edge_nll_workspace_size(lib):
    f = lib.blm_linear_nll_edges_ws_floats
    assert f(100, 1000) == lib.blm_linear_nll_ws_floats(100, 1000) + 4 + 4 * 100
    assert f(0, 8) == 4
    for bad in ((1 << 30, 33000), (-1, 1000), (10, -4)):
        assert f(*bad) == 0, bad
    g = lib.blm_linear_nll2_edges_ws_floats
    assert g(100, 1001, 64, 32) == 100 * 96 + f(100, 1004)
    assert g(-1, 1000, 64, 64) == 0


def _edges2(lib, x1=FAKE, ldx1=64, K1=64, ldw2=32, wcat=FAKE, M=16, E=20, N=1001):
    return lib.blm_linear_nll2_edges(x1, ldx1, FAKE, 64, None, K1, FAKE, 32, FAKE, ldw2, None, 32, ctypes.c_float(0.5), FAKE, FAKE,
                                     FAKE, wcat, 1, FAKE, M, E, N, None)


@pytest.mark.parametrize("kw,msg", [({"x1": None}, b"bad arguments"), ({"wcat": None}, b"bad arguments"), ({"ldw2": 16}, b"bad arguments"),
                                    ({"N": 0}, b"bad shape"), ({"E": -2}, b"bad shape"), ({"K1": 62, "ldx1": 62}, b"multiples of 4")])
def test_interpolated_edge_nll_argument_errors(lib, kw, msg):
    assert _edges2(lib, **kw) != 0
    assert msg in lib.blm_last_error()
