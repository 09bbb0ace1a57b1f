"""CPU: speculative sampling without a device.  The float64 model of tests/spec_reference.py (what tests/test_gpu_speculative.py
holds the kernel to) on hand-written cases; blm_spec_accept declared, exported, bound, and refusing bad arguments on the host before
any launch; the generate CLI's refusals, which fire before a device is needed; and SpeculativeLM's host bookkeeping on a stub
IncrementalLM: uneven streams, the two-word draft feed after a full accept, the cut at ``words``, an LSTM on either side."""
import copy
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import spec_reference as R
from conftest import ROOT

LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")
NEG = -np.inf


# ------------------------------------------------------------------------------------------------------- the reference model
def _rand(G, N, V, seed=0, sigma=0.7):
    g = np.random.default_rng(seed)
    P = 2.5 * g.standard_normal((G + 1, N, V))
    return P, P[:G] + sigma * g.standard_normal((G, N, V)), g


def test_reference_p_equal_q_accepts_everything_and_draws_plainly():
    P, _, g = _rand(3, 6, 19)
    x = g.integers(0, 19, (3, 6))
    r = R.spec_accept(P, P[:3].copy(), x, 0.8, 5, 2, 1)
    assert r["accept"].all() and (r["n_acc"] == 3).all()
    # no column has rho > 0: every candidate is the plain draw from p at that row index, the bonus row included
    assert np.array_equal(r["cand"].reshape(-1), R.sample_rows(P.reshape(-1, 19), 0.8, 5, 2, 1))
    assert np.array_equal(r["token"], r["cand"][3])


def test_reference_point_mass_draft_on_a_word_the_target_excludes():
    G, N, V, w = 2, 40, 9, 4
    P, _, g = _rand(G, N, V, 1)
    P[:, :, w] = NEG                      # p(w) = 0
    Q = np.full((G, N, V), NEG)
    Q[:, :, w] = 0.3                      # q = a point mass on w
    x = np.full((G, N), w)
    r = R.spec_accept(P, Q, x, 1.0, 5, 2, 1)
    assert not r["accept"].any() and (r["n_acc"] == 0).all()
    assert (r["cand"] != w).all() and np.array_equal(r["token"], r["cand"][0])
    # and with q(x) = 0 or x outside [0, V) the draft is rejected whatever p says
    x2 = np.full((G, N), 0)
    x2[1] = V
    assert not R.spec_accept(P, Q, x2, 1.0, 5, 2, 1)["accept"].any()


def test_reference_accept_rule_and_residual_on_a_two_word_vocabulary():
    """V = 2, p = (0.8, 0.2), q = (0.5, 0.5): x = 0 is always accepted (p >= q), x = 1 with probability 0.4, and the residual
    max(p - q, 0) is a point mass on word 0."""
    N = 400
    P = np.log(np.tile(np.array([0.8, 0.2]), (2, N, 1)))
    Q = np.log(np.tile(np.array([0.5, 0.5]), (1, N, 1)))
    r0 = R.spec_accept(P, Q, np.zeros((1, N), np.int64), 1.0, 9, 2, 0)
    assert r0["accept"].all()
    r1 = R.spec_accept(P, Q, np.ones((1, N), np.int64), 1.0, 9, 2, 0)
    u = R.uniforms(0xFFFFFFFF, np.arange(N), 9, 2, 0)
    assert np.array_equal(r1["accept"][0], (u < 0.4).astype(np.uint8))
    assert abs(r1["accept"].mean() - 0.4) < 4 * np.sqrt(0.24 / N)
    assert (r1["cand"][0] == 0).all()
    assert np.array_equal(r1["token"], np.where(r1["accept"][0] == 1, r1["cand"][1], 0))


def test_reference_emits_the_target_distribution():
    V, N = 5, 6000
    g = np.random.default_rng(3)
    lp, lq = 1.2 * g.standard_normal(V), 0.8 * g.standard_normal(V)
    p, q = np.exp(R._log_softmax(lp)), np.exp(R._log_softmax(lq))
    x = R.sample_rows(np.tile(lq, (N, 1)), 1.0, 7, 1, 0)[None, :]
    r = R.spec_accept(np.tile(lp, (2, N, 1)), np.tile(lq, (1, N, 1)), x, 1.0, 7, 2, 0)
    out = np.where(r["accept"][0] == 1, x[0], r["token"])
    cnt = np.bincount(out, minlength=V)
    assert (np.abs(cnt - N * p) <= 4 * np.sqrt(N * p * (1 - p))).all(), (cnt, N * p)
    a = np.minimum(p, q).sum()
    assert abs(r["accept"].mean() - a) <= 4 * np.sqrt(a * (1 - a) / N)


def test_reference_greedy_rules():
    P, _, g = _rand(2, 5, 12, 2)
    P[0, 0, 3] = P[0, 0, 9] = 40.0  # a tie: the lowest index
    best = P.argmax(-1)
    assert best[0, 0] == 3
    x = best[:2].copy()
    x[1, 2] = (x[1, 2] + 1) % 12
    x[0, 4] = (x[0, 4] + 5) % 12
    r = R.spec_accept(P, None, x, 0.0, 0, 0, 0)
    assert np.array_equal(r["cand"], best)
    assert np.array_equal(r["accept"], (x == best[:2]).astype(np.uint8))
    assert r["n_acc"].tolist() == [2, 2, 1, 2, 0]
    assert r["token"].tolist() == [best[2, 0], best[2, 1], best[1, 2], best[2, 3], best[0, 4]]


def test_reference_nan_row_spoils_only_itself():
    P, Q, g = _rand(2, 4, 10, 4)
    x = g.integers(0, 10, (2, 4))
    clean = R.spec_accept(P, Q, x, 1.0, 5, 2, 1)
    P[1, 2, 7] = np.nan
    Q[0, 3, 0] = np.nan
    P[2, 0, 1] = np.nan
    r = R.spec_accept(P, Q, x, 1.0, 5, 2, 1)
    for t in range(3):
        for n in range(4):
            if (t, n) in {(1, 2), (0, 3), (2, 0)}:
                assert r["cand"][t, n] == -1 and (t == 2 or r["accept"][t, n] == 0)
            else:
                assert r["cand"][t, n] == clean["cand"][t, n] and (t == 2 or r["accept"][t, n] == clean["accept"][t, n])
    assert r["token"][3] == -1 and r["n_acc"][3] == 0


# ------------------------------------------------------------------------------------------------------- the entry point
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from bayeslms_amd import _lib as L
    return L, L.lib()


def test_entry_point_is_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "bayeslm.h")).read()
    declared = set(re.findall(r"\b(blm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L, _ = lib
    assert "blm_spec_accept" in declared and "blm_spec_accept" in exported and "blm_spec_accept" in L.SIGNATURES
    assert "#define BLM_ABI_VERSION 1u" in hdr
    assert "speculative.hip" in open(os.path.join(ROOT, "bayeslms_amd", "csrc", "Makefile")).read()


def test_entry_point_refuses_on_the_host(lib):
    import ctypes as C
    L, l = lib
    r = L.rng(1, 2, 3)
    B = 0x100000  # never dereferenced: every call below fails its checks before a launch
    good = dict(p=B, ldp=16, q=B + 0x10000, ldq=16, d=B + 0x20000, G=2, N=4, V=16, tau=1.0, rng=C.byref(r), a=B + 0x30000, c=B + 0x40000,
                n=B + 0x50000, t=B + 0x60000)

    def call(**kw):
        a = dict(good, **kw)
        return l.blm_spec_accept(a["p"], a["ldp"], a["q"], a["ldq"], a["d"], a["G"], a["N"], a["V"], a["tau"], a["rng"], a["a"], a["c"],
                                 a["n"], a["t"], None)
    cases = [dict(p=None), dict(q=None), dict(d=None), dict(a=None), dict(c=None), dict(n=None), dict(t=None), dict(rng=None),
             dict(G=0), dict(G=-1), dict(N=0), dict(V=0), dict(V=-5), dict(ldp=15), dict(ldq=15),
             dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(tau=1e-45),
             dict(G=2 ** 31 - 1), dict(N=2 ** 31 - 1), dict(ldp=2 ** 40), dict(G=70000, N=70000, ldp=2 ** 20, ldq=2 ** 20),
             dict(a=B), dict(c=B + 64), dict(n=B + 0x10000 + 8), dict(t=B + 0x20000), dict(c=B + 3 * 4 * 16 * 4 - 8),
             dict(q=None, tau=0.0, p=None)]
    for kw in cases:
        assert call(**kw) == L.ERR_INVALID, kw
        assert b"blm_spec_accept" in l.blm_last_error(), kw


# ------------------------------------------------------------------------------------------------------- the command line
@pytest.mark.parametrize("argv,needle", [
    (["--speculate", "4", "--mc-samples", "4", "--beam", "3"], "--beam"),
    (["--speculate", "4", "--mc-samples", "4", "--top-k", "10"], "--top-k"),
    (["--speculate", "4", "--mc-samples", "4", "--top-p", "0.9"], "--top-p"),
    (["--speculate", "4", "--mc-samples", "4", "--write-uncertainty", "u.txt"], "--write-uncertainty"),
    (["--draft-model-path", "student.pt"], "--draft-model-path needs --speculate"),
    (["--draft-args", "--model Transformer"], "--draft-args needs --speculate"),
    (["--speculate", "4"], "--mc-samples"),
    (["--speculate", "4", "--mc-samples", "1"], "--mc-samples"),
    (["--speculate", "17", "--mc-samples", "4"], "1..16"),
    (["--speculate", "-1", "--mc-samples", "4"], "1..16"),
    (["--speculate", "4", "--mc-samples", "4", "--draft-args", "--model LSTM"], "--draft-args needs --draft-model-path"),
])
def test_cli_refuses_before_any_file_or_device(argv, needle):
    from bayeslms_amd import generate
    with pytest.raises(SystemExit) as e:
        generate.main(["--model-path", "/no/such/model.pt", "--vocabulary", "/no/such/words.txt"] + argv)
    assert needle in str(e.value) and "MI355X" not in str(e.value), e.value


def test_cli_draft_args_shape_the_draft_alone():
    from bayeslms_amd import generate
    p = generate.build_parser()
    args = p.parse_args(["--model-path", "m.pt", "--vocabulary", "w.txt", "--model", "Transformer", "--emsize", "64", "--nhid", "128",
                         "--speculate", "4", "--draft-model-path", "s.pt", "--draft-args", "--model LSTM --emsize 32 --nlayers 1"])
    shape = generate.check_speculate_args(args)
    assert (shape.model, shape.emsize, shape.nlayers, shape.nhid) == ("LSTM", 32, 1, 1024) and shape.interpolation_flag == 0
    assert (args.model, args.emsize) == ("Transformer", 64)
    args = p.parse_args(["--model-path", "m.pt", "--vocabulary", "w.txt", "--model", "Transformer", "--emsize", "64", "--speculate", "2",
                         "--draft-model-path", "s.pt"])
    shape = generate.check_speculate_args(args)  # the default: the target's own
    assert (shape.model, shape.emsize) == ("Transformer", 64)
    assert generate.check_speculate_args(p.parse_args(["--model-path", "m.pt", "--vocabulary", "w.txt"])) is None


# ------------------------------------------------------------------------------------------------------- the driver's bookkeeping
V = 23


def _next(hist):
    """the target's word after a history (greedy): a function of all of it"""
    return (3 * hist[-1] + len(hist) + sum(hist) % 5) % V


class _Hist:
    """what a stub state holds in place of device memory: every stream's tokens"""

    def __init__(self, n):
        self.h = [[] for _ in range(n)]

    def clone(self):
        return copy.deepcopy(self)

    def copy_(self, other):
        self.h = copy.deepcopy(other.h)


class _StubState:
    def __init__(self, lm, n):
        self._lm, self.n, self._buf, self.lengths = lm, n, _Hist(n), [0] * n

    def _live(self, lm):
        assert lm is self._lm
        return self._buf


class _StubLM:
    """IncrementalLM's surface over token lists: step returns rows peaked on a next word that is a function of the stream's whole
    history -- ``wrong(j, hist)`` says where this model disagrees with the target's word."""
    mc_samples, device, model = 0, torch.device("cpu"), None

    def __init__(self, kind, max_streams, max_len, wrong=None, mc_samples=0):
        self.kind, self.max_streams, self.max_len, self.vocab, self.wrong, self.mc_samples = kind, max_streams, max_len, V, wrong, mc_samples
        self.calls = []  # (ids (Tq, N) as a list of rows, n_new as a list)

    def start(self, n):
        assert 1 <= n <= self.max_streams
        return _StubState(self, n)

    def _row(self, j, hist):
        w = _next(hist)
        if self.wrong is not None and self.wrong(j, hist):
            w = (w + 1) % V
        row = torch.full((V,), -8.0)
        row[w] = 0.0
        return row

    def step(self, st, ids, n_new=None, all_positions=False):
        ids = ids.view(1, -1) if ids.dim() == 1 else ids
        Tq, N = ids.shape
        k = [Tq] * N if n_new is None else [int(v) for v in n_new]
        assert N == st.n and max(k) >= 1 and all(0 <= v <= Tq for v in k)
        self.calls.append((ids.tolist(), list(k)))
        out = torch.full((Tq, N, V), float("nan"))
        for j in range(N):
            for t in range(k[j]):
                assert 0 <= int(ids[t, j]) < V
                st._buf.h[j].append(int(ids[t, j]))
                out[t, j] = self._row(j, st._buf.h[j])
            assert len(st._buf.h[j]) <= self.max_len, "a stream holds more than max_len"
        st.lengths = [len(h) for h in st._buf.h]
        if all_positions:
            return out
        return torch.stack([out[k[j] - 1, j] if k[j] else out[0, j] for j in range(N)])

    def truncate(self, st, lengths):
        from bayeslms_amd import BayesLMError
        if self.kind != "transformer":
            raise BayesLMError("no truncate on an LSTM")
        assert all(0 <= int(a) <= b for a, b in zip(lengths, st.lengths))
        st._buf.h = [h[:int(a)] for h, a in zip(st._buf.h, lengths)]
        st.lengths = [int(a) for a in lengths]


def _spec(target, draft, gamma, truth, L0, W):
    """SpeculativeLM with the two device ops replaced by their references; the verification also checks, for every stream that
    still wants words, what both sides have consumed at that moment: the target s + x_0 .. x_{G-1}, the draft one word fewer."""
    from bayeslms_amd.speculative import SpeculativeLM

    class Spec(SpeculativeLM):
        verified = 0

        def _sample(self, rows, temperature, seed, step):
            assert temperature == 0.0
            return torch.nan_to_num(rows, nan=-1e30).argmax(-1)

        def _verify(self, logp, logq, drafted, temperature, seed, step):
            G, N = drafted.shape
            assert logq is None and tuple(logp.shape) == (G + 1, N, V)
            th, dh = self.tst_seen._buf.h, self.dst_seen._buf.h
            for j in range(N):
                ls = len(th[j]) - G  # len(s)
                if ls >= L0 + W:
                    continue  # a frozen stream: whatever it runs is taken back
                xs = drafted[:, j].tolist()
                assert th[j] == truth[:ls] + xs, (j, th[j], truth[:ls], xs)
                assert dh[j] == truth[:ls] + xs[:G - 1], (j, dh[j])
            type(self).verified += 1
            r = R.spec_accept(logp.double().numpy(), None, drafted.numpy(), 0.0, seed, 2, step)
            return SimpleNamespace(n_acc=torch.from_numpy(r["n_acc"]), token=torch.from_numpy(r["token"]))

    s = Spec(target, draft, gamma)
    t_start, d_start = target.start, draft.start

    def keep_t(n):
        s.tst_seen = t_start(n)
        return s.tst_seen

    def keep_d(n):
        s.dst_seen = d_start(n)
        return s.dst_seen
    target.start, draft.start = keep_t, keep_d
    return s


def _truth(ctx, W, extra):
    seq = list(ctx)
    for _ in range(W + extra):
        seq.append(_next(seq))
    return seq


@pytest.mark.parametrize("kinds", [("transformer", "transformer"), ("lstm", "transformer"), ("transformer", "lstm"), ("lstm", "lstm")])
@pytest.mark.parametrize("gamma", [1, 2, 4])
def test_driver_bookkeeping_on_stub_models(kinds, gamma):
    N, W, ctx = 5, 17, [1, 7, 2]
    L0 = len(ctx)
    truth = _truth(ctx, W, gamma + 2)
    # stream j's draft is wrong wherever (len(history) + j) % (j + 2) == 0; the last stream's draft is always right
    wrong = lambda j, hist: j != N - 1 and (len(hist) + j) % (j + 2) == 0  # noqa: E731
    target = _StubLM(kinds[0], N, L0 + W + gamma)
    draft = _StubLM(kinds[1], N, L0 + W + gamma, wrong)
    spec = _spec(target, draft, gamma, truth, L0, W)
    out, stats = spec.generate(ctx, W, N, 0.0, 5)
    assert out == [truth[L0:L0 + W]] * N                      # greedy: the target's own continuation, cut at `words`
    assert stats.rounds == type(spec).verified and stats.rounds < W   # somebody skipped ahead
    assert 0 < stats.accepted < stats.drafted and stats.drafted % gamma == 0
    assert stats.accepted + stats.drafted // gamma >= N * W   # every stream-round emits n_acc + 1 words
    assert stats.target_chunks == stats.rounds if kinds[0] == "transformer" else stats.target_chunks >= stats.rounds
    # uneven streams: the always-right stream finished in ceil(W / (gamma + 1)) rounds, the others took more
    assert stats.rounds > -(-W // (gamma + 1))
    # after a full accept the draft is fed two words in one ragged step: x_{G-1}, then the bonus word
    two = [(ids, k) for ids, k in draft.calls if len(ids) == 2 and 2 in k]
    assert two, "no two-word draft feed"
    ids, k = two[0]
    j = k.index(2)
    at = [i for i in range(len(truth) - 1) if truth[i] == ids[0][j] and truth[i + 1] == ids[1][j]]
    assert at, "the two words are not consecutive words of the sequence"
    assert all(v in (0, 1, 2) for _, kk in two for v in kk)


def test_driver_refusals():
    from bayeslms_amd import BayesLMError
    from bayeslms_amd.speculative import SpeculativeLM
    t = _StubLM("transformer", 4, 40)
    for g in (0, 17):
        with pytest.raises(BayesLMError, match="gamma"):
            SpeculativeLM(t, _StubLM("transformer", 4, 40), g)
    with pytest.raises(BayesLMError, match="mc_samples >= 2"):
        SpeculativeLM(t, None, 4)
    with pytest.raises(BayesLMError, match="cheap"):
        SpeculativeLM(t, _StubLM("transformer", 4, 40, mc_samples=2), 4)
    other = _StubLM("transformer", 4, 40)
    other.vocab = V + 1
    with pytest.raises(BayesLMError, match="vocabulary"):
        SpeculativeLM(t, other, 4)
    s = SpeculativeLM(t, _StubLM("transformer", 4, 40), 4)
    with pytest.raises(BayesLMError, match="max_len"):
        s.generate([1, 2], 35, 2, 0.0, 1)  # 2 + 35 + 4 > 40
    with pytest.raises(BayesLMError, match="streams"):
        s.generate([1, 2], 5, 5, 0.0, 1)
    assert s.generate([1, 2], 0, 2, 0.0, 1)[0] == [[], []]
    from bayeslms_amd import speculative as SP
    assert (SP.STREAM_PLAIN, SP.STREAM_DRAFT, SP.STREAM_VERIFY) == (0, 1, 2)
