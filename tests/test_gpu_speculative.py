"""GPU: speculative sampling (csrc/speculative.hip, ops.spec_accept, IncrementalLM.truncate, bayeslms_amd/speculative.py).

The kernel against the float64 model of tests/spec_reference.py.  A float32 evaluation of the definitions can legitimately differ
from the float64 one in two places, and only there:
  * the accept margin |log u - min(0, log p(x) - log q(x))| lies below 1e-4;
  * the winning key lies within 1e-3 of the runner-up, or the winner (of either side) is a column where p_v - q_v cancels.
    "Cancels" is |log p_v - log q_v| < 1e-2: a float32 log p - log q carries an absolute error of about 1e-5 (one rounding of
    beta P at |beta P| < 64 is 4e-6, the log-sum and the subtraction add the rest), rho_v / p_v = 1 - exp(log q_v - log p_v) is
    about |log p_v - log q_v|, so below 1e-2 the relative error of rho_v, and with it the error of the key log rho_v + g_v,
    passes 1e-3.
A case may leave out at most max(1, 0.5 %) of its rows on these grounds; every other row agrees exactly.  n_acc and token follow
from the kernel's own flags and candidates with no exception."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import spec_reference as R
from bayeslms_amd import BayesLMError
from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED, DRAFT_STREAM, VERIFY_STREAM = 20231, 1, 2
# (V, row stride or None for contiguous rows, G, N) -- the forms: V 16 and 1001 / 1004 (a V % 4 tail) and 4100 the 3-quad register
# form, 33,278 / 33,280 the 9-quad one at the top of its range, 40,000 the sweep
CASES = [(16, None, 4, 512), (1001, 1004, 4, 512), (4100, None, 4, 64), (33278, 33280, 3, 64), (40000, None, 3, 64)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rows(T, N, V, ld, gen, dev, base=None, sigma=None):
    """(T, N, V) float32 on the device, as a view of rows padded to ld (NaN in the padding: it must never be read)"""
    x = 2.5 * torch.randn(T, N, V, generator=gen) if base is None else base + sigma * torch.randn(T, N, V, generator=gen)
    if ld is None:
        return x, x.to(dev)
    buf = torch.full((T, N, ld), float("nan"))
    buf[..., :V] = x
    return x, buf.to(dev)[..., :V]


def _inputs(V, ld, G, N, tau, sigma, dev, seed=0):
    from bayeslms_amd import ops
    gen = torch.Generator().manual_seed(1000 * V + int(10 * sigma) + seed)
    P, Pd = _rows(G + 1, N, V, ld, gen, dev)
    Q, Qd = _rows(G, N, V, ld, gen, dev, P[:G], sigma)
    x = ops.sample_rows(Qd.reshape(G * N, V), tau, SEED, DRAFT_STREAM, 3).view(G, N)  # drawn from q, under another stream id
    return P, Pd, Q, Qd, x


def _cancel(P, Q, tau, t, n, col):
    """|log p - log q| at column col of row (t, n), float64"""
    beta = float(np.float32(1.0) / np.float32(tau))
    lp, lq = R._log_softmax(beta * P[t, n].double().numpy()), R._log_softmax(beta * Q[t, n].double().numpy())
    with np.errstate(invalid="ignore"):
        return abs(lp[col] - lq[col])


def _compare(out, ref, P, Q, tau, G, N):
    """-> the rows left out, after asserting that each is one float32 may decide otherwise and that they are few"""
    acc, cand = out.accept.cpu().numpy(), out.cand.cpu().numpy()
    left = set()
    for t, n in zip(*np.nonzero(acc != ref["accept"])):
        assert ref["accept_margin"][t, n] < 1e-4, ("accept", t, n, ref["accept_margin"][t, n])
        left.add((t, n))
    for t, n in zip(*np.nonzero(cand != ref["cand"])):
        near = ref["cand_margin"][t, n] < 1e-3
        if not near and t < G and cand[t, n] >= 0:
            near = min(_cancel(P, Q, tau, t, n, ref["cand"][t, n]), _cancel(P, Q, tau, t, n, cand[t, n])) < 1e-2
        assert near, ("cand", t, n, cand[t, n], ref["cand"][t, n], ref["cand_margin"][t, n])
        left.add((t, n))
    rows = (G + 1) * N
    print("rows left out: %d of %d (accept flips %d, candidates %d)" % (len(left), rows, int((acc != ref["accept"]).sum()),
                                                                     int((cand != ref["cand"]).sum())))
    assert len(left) <= max(1, int(0.005 * rows)), (len(left), rows)
    n_acc, token = R.finish(acc, cand)  # from the kernel's own flags and candidates, no exception
    assert np.array_equal(out.n_acc.cpu().numpy(), n_acc) and np.array_equal(out.token.cpu().numpy(), token)
    return left


@pytest.mark.parametrize("sigma", [0.3, 1.0])
@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("V,ld,G,N", CASES)
def test_kernel_against_float64(dev, V, ld, G, N, tau, sigma):
    from bayeslms_amd import ops
    P, Pd, Q, Qd, x = _inputs(V, ld, G, N, tau, sigma, dev)
    out = ops.spec_accept(Pd, Qd, x, tau, SEED, VERIFY_STREAM, 5)
    ref = R.spec_accept(P.numpy(), Q.numpy(), x.cpu().numpy(), tau, SEED, VERIFY_STREAM, 5)
    assert out.accept.shape == (G, N) and out.cand.shape == (G + 1, N) and out.n_acc.dtype == torch.int32
    _compare(out, ref, P, Q, tau, G, N)
    assert 0 < int(out.accept.sum()) < G * N  # the inputs exercise both outcomes
    again = ops.spec_accept(Pd, Qd, x, tau, SEED, VERIFY_STREAM, 5)  # repeat runs: the same bits
    assert all(torch.equal(a, b) for a, b in zip(out, again))


@pytest.mark.parametrize("V,ld,G,N", CASES)
def test_bonus_row_is_sample_rows_bit_for_bit(dev, V, ld, G, N):
    from bayeslms_amd import ops
    for tau in (0.5, 1.0, 2.0):
        P, Pd, Q, Qd, x = _inputs(V, ld, G, N, tau, 1.0, dev)
        out = ops.spec_accept(Pd, Qd, x, tau, SEED, VERIFY_STREAM, 9)
        plain = ops.sample_rows(Pd.reshape((G + 1) * N, V), tau, SEED, VERIFY_STREAM, 9)  # row index t * N + n
        assert torch.equal(out.cand[G], plain[G * N:]), tau


def test_all_rho_zero_falls_back_to_the_plain_draw(dev):
    """q = p bit for bit: no column has rho > 0, every draft is accepted, and every candidate is the plain draw from p."""
    from bayeslms_amd import ops
    for V, G, N in ((16, 2, 64), (4100, 2, 16), (40000, 1, 8)):
        gen = torch.Generator().manual_seed(V)
        P = (2.5 * torch.randn(G + 1, N, V, generator=gen)).to(dev)
        Q = P[:G].clone()
        x = ops.sample_rows(Q.view(G * N, V), 1.0, SEED, DRAFT_STREAM, 0).view(G, N)
        out = ops.spec_accept(P, Q, x, 1.0, SEED, VERIFY_STREAM, 1)
        assert bool(out.accept.all()) and bool((out.n_acc == G).all())
        assert torch.equal(out.cand.view(-1), ops.sample_rows(P.view(-1, V), 1.0, SEED, VERIFY_STREAM, 1))
        assert torch.equal(out.token, out.cand[G])


@pytest.mark.parametrize("V,ld,G,N", CASES)
def test_greedy_is_exact(dev, V, ld, G, N):
    from bayeslms_amd import ops
    gen = torch.Generator().manual_seed(V + 7)
    P, Pd = _rows(G + 1, N, V, ld, gen, dev)
    hi = float(P.max()) + 1.0
    for t, n, a, b in ((0, 0, 3, V - 1), (G, N - 1, 0, V // 2), (1, 1, V // 3, V // 3 + 1)):  # planted ties: the lowest index wins
        P[t, n, a] = P[t, n, b] = hi
        Pd[t, n, a] = Pd[t, n, b] = hi
    best = P.argmax(-1)
    assert int(best[0, 0]) == 3 and int(best[G, N - 1]) == 0
    x = best[:G].clone()
    x[:, ::3] = (x[:, ::3] + 1) % V  # every third stream drafts another word
    x[0, 1] = V - 1 if int(best[0, 1]) != V - 1 else 0
    out = ops.spec_accept(Pd, None, x.to(dev), 0.0)
    assert torch.equal(out.cand.cpu(), best)
    assert torch.equal(out.accept.cpu(), (x == best[:G]).to(torch.uint8))
    n_acc, token = R.finish(out.accept.cpu().numpy(), out.cand.cpu().numpy())
    assert np.array_equal(out.n_acc.cpu().numpy(), n_acc) and np.array_equal(out.token.cpu().numpy(), token)
    ref = R.spec_accept(P.numpy(), None, x.numpy(), 0.0, 0, 0, 0)
    assert np.array_equal(ref["cand"], best.numpy()) and np.array_equal(ref["n_acc"], n_acc)


@pytest.mark.parametrize("V,ld,off", [(4100, 4104, 8), (1001, 1003, 1), (33280, 33284, 4)])
def test_strided_and_offset_views_give_the_bits_of_contiguous_copies(dev, V, ld, off):
    """Aligned padded rows of a V that is a multiple of 4 (the same register form on both sides: 3 quads, 9 quads) and odd strides
    from an odd offset (the sweep on both sides: a contiguous row of 1001 floats is no multiple of 4 either).  The forms round their
    sums differently, so bits are compared within a form."""
    from bayeslms_amd import ops
    G, N = 2, 24
    gen = torch.Generator().manual_seed(V + off)
    flat_p = torch.full((off + (G + 1) * N * ld,), float("nan"), device=dev)
    flat_q = torch.full((off + G * N * ld,), float("nan"), device=dev)
    Pv = flat_p[off:].view(G + 1, N, ld)[..., :V]
    Qv = flat_q[off:].view(G, N, ld)[..., :V]
    Pv.copy_(2.5 * torch.randn(G + 1, N, V, generator=gen))
    Qv.copy_(Pv[:G] + 0.5 * torch.randn(G, N, V, generator=gen).to(dev))
    assert not Pv.is_contiguous() and Pv.data_ptr() == flat_p.data_ptr() + 4 * off
    x = ops.sample_rows(Qv.reshape(G * N, V), 1.0, SEED, DRAFT_STREAM, 0).view(G, N)
    a = ops.spec_accept(Pv, Qv, x, 1.0, SEED, VERIFY_STREAM, 2)
    b = ops.spec_accept(Pv.contiguous(), Qv.contiguous(), x, 1.0, SEED, VERIFY_STREAM, 2)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert bool(torch.isnan(flat_p[:off]).all()) and bool(torch.isnan(flat_p[off:].view(G + 1, N, ld)[..., V:]).all())  # inputs untouched


def test_repeat_runs_and_the_deterministic_option_give_the_same_bits(dev):
    from bayeslms_amd import _lib as L
    from bayeslms_amd import ops
    P, Pd, Q, Qd, x = _inputs(4100, None, 4, 64, 1.0, 1.0, dev)
    a = ops.spec_accept(Pd, Qd, x, 1.0, SEED, VERIFY_STREAM, 5)
    L.check(L.lib().blm_set_option(b"deterministic", 1))
    try:
        b = ops.spec_accept(Pd, Qd, x, 1.0, SEED, VERIFY_STREAM, 5)
    finally:
        L.check(L.lib().blm_set_option(b"deterministic", 0))
    assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("V", [16, 4100, 33278, 40000])
def test_nan_row_spoils_only_itself(dev, V):
    from bayeslms_amd import ops
    G, N = 3, 8
    P, Pd, Q, Qd, x = _inputs(V, None, G, N, 1.0, 1.0, dev)
    clean = ops.spec_accept(Pd, Qd, x, 1.0, SEED, VERIFY_STREAM, 5)
    Pd, Qd = Pd.clone(), Qd.clone()
    Pd[1, 2, V - 1] = float("nan")   # a target row
    Qd[0, 5, 0] = float("nan")       # a draft row
    Pd[G, 7, V // 2] = float("nan")  # a bonus row
    out = ops.spec_accept(Pd, Qd, x, 1.0, SEED, VERIFY_STREAM, 5)
    spoiled = {(1, 2), (0, 5), (G, 7)}
    for t in range(G + 1):
        for n in range(N):
            if (t, n) in spoiled:
                assert int(out.cand[t, n]) == -1 and (t == G or int(out.accept[t, n]) == 0)
            else:
                assert int(out.cand[t, n]) == int(clean.cand[t, n]) and (t == G or int(out.accept[t, n]) == int(clean.accept[t, n]))
    n_acc, token = R.finish(out.accept.cpu().numpy(), out.cand.cpu().numpy())
    assert np.array_equal(out.n_acc.cpu().numpy(), n_acc) and np.array_equal(out.token.cpu().numpy(), token)
    g = ops.spec_accept(Pd, None, x, 0.0)  # greedy: the same rule on P's rows
    assert int(g.cand[1, 2]) == -1 and int(g.accept[1, 2]) == 0 and int(g.cand[G, 7]) == -1 and int(g.cand[0, 5]) >= 0


def _emitted_counts(dev, verify_stream, verify_step):
    """V 16, fixed p and q of different shape, G 1, 2^16 streams -> (counts of the emitted word, N p, accepted share, sum min)"""
    from bayeslms_amd import ops
    V, N = 16, 1 << 16
    gen = torch.Generator().manual_seed(4)
    lp, lq = torch.randn(V, generator=gen) * 1.5, torch.randn(V, generator=gen) * 0.7
    p, q = torch.softmax(lp.double(), 0), torch.softmax(lq.double(), 0)
    P = lp.to(dev).expand(2, N, V).contiguous()
    Q = lq.to(dev).expand(1, N, V).contiguous()
    x = ops.sample_rows(Q.view(N, V), 1.0, SEED, DRAFT_STREAM, 7).view(1, N)
    out = ops.spec_accept(P, Q, x, 1.0, SEED, verify_stream, verify_step)
    emitted = torch.where(out.accept[0].bool(), x[0], out.token)
    cnt = torch.bincount(emitted.cpu(), minlength=V).double()
    return cnt, N * p, float(out.accept.double().mean()), float(torch.minimum(p, q).sum()), N, p


def test_emitted_words_are_distributed_as_the_target(dev):
    cnt, want, share, overlap, N, p = _emitted_counts(dev, VERIFY_STREAM, 0)
    se = torch.sqrt(N * p * (1 - p))
    assert torch.all((cnt - want).abs() <= 4 * se), (cnt, want)
    assert abs(share - overlap) <= 4 * np.sqrt(overlap * (1 - overlap) / N), (share, overlap)


def test_independence_rule_is_visible(dev):
    """The verify call keyed by the draft's own stream id and step reuses the draft's noise in the residual draw: the same
    count test must FAIL, which shows that it can see a wrong draw."""
    cnt, want, share, overlap, N, p = _emitted_counts(dev, DRAFT_STREAM, 7)
    se = torch.sqrt(N * p * (1 - p))
    assert not torch.all((cnt - want).abs() <= 4 * se), (cnt, want)


def test_refusals(dev):
    from bayeslms_amd import _lib as L
    from bayeslms_amd import ops
    P, Q = torch.randn(3, 4, 16, device=dev), torch.randn(2, 4, 16, device=dev)
    x = torch.zeros(2, 4, dtype=torch.int64, device=dev)
    for bad in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature=1e-45)):
        with pytest.raises(BayesLMError):
            ops.spec_accept(P, Q, x, **bad)
    with pytest.raises(BayesLMError):
        ops.spec_accept(P, None, x, 1.0)
    with pytest.raises(BayesLMError):
        ops.spec_accept(P, Q[:1], x, 1.0)
    with pytest.raises(BayesLMError):
        ops.spec_accept(P, Q, x[:1], 1.0)
    lib, r = L.lib(), L.rng(1, 2, 3)
    import ctypes as C
    acc = torch.zeros(8, dtype=torch.uint8, device=dev)
    cand = torch.zeros(12, dtype=torch.int64, device=dev)
    na = torch.zeros(4, dtype=torch.int32, device=dev)
    tok = torch.zeros(4, dtype=torch.int64, device=dev)

    def call(p=P, ldp=16, q=Q, ldq=16, d=x, G=2, N=4, V=16, tau=1.0, a=acc, c=cand, n=na, t=tok):
        return lib.blm_spec_accept(L.ptr(p), ldp, L.ptr(q), ldq, L.ptr(d), G, N, V, tau, C.byref(r), L.ptr(a), L.ptr(c), L.ptr(n), L.ptr(t),
                                   L.stream())
    assert call() == L.OK
    for kw in (dict(p=None), dict(q=None), dict(d=None), dict(a=None), dict(c=None), dict(n=None), dict(t=None), dict(G=0), dict(N=0),
               dict(V=0), dict(ldp=15), dict(ldq=15), dict(tau=-0.5), dict(tau=float("inf")), dict(tau=1e-45),
               dict(c=P.view(torch.int64)), dict(t=x), dict(a=Q.view(torch.uint8))):
        assert call(**kw) == L.ERR_INVALID, kw
        assert b"blm_spec_accept" in lib.blm_last_error()
    assert call(q=None, tau=0.0) == L.OK


# ------------------------------------------------------------------------------------------------------- IncrementalLM.truncate
@pytest.mark.parametrize("name,S", [("transformer_baseline", 0), ("bayes_tlm_FFN", 0), ("bayes_tlm_FFN", 2), ("gauss_tlm_3", 2)])
def test_truncate_equals_a_fresh_state_fed_the_kept_prefix(dev, name, S):
    from bayeslms_amd.incremental import IncrementalLM
    from test_gpu_incremental import TOL, _fixture_model, rel
    m, _ = _fixture_model(name, dev)
    V, B = m.decoder.weight.shape[0], 3
    gen = torch.Generator().manual_seed(11)
    ids = torch.randint(0, V, (12, B), generator=gen).to(dev)
    other = torch.randint(0, V, (3, B), generator=gen).to(dev)
    keep = [9, 4, 0]
    lm = IncrementalLM(m, max_streams=B, max_len=64, mc_samples=S)
    st = lm.start(B)
    lm.step(st, ids)
    with pytest.raises(BayesLMError):
        lm.truncate(st, [13, 0, 0])
    with pytest.raises(BayesLMError):
        lm.truncate(st, [1, -1, 0])
    assert st.lengths == [12] * B
    lm.truncate(st, keep)
    assert st.lengths == keep
    assert st._buf.past[:max(S, 1) * B].cpu().tolist() == keep * max(S, 1)  # every sample slot moved
    lp = lm.step(st, other, all_positions=True)
    fresh = lm.start(B)
    lm.step(fresh, ids, n_new=keep)
    want = lm.step(fresh, other, all_positions=True)
    assert st.lengths == fresh.lengths == [k + 3 for k in keep]
    assert rel(lp, want) < TOL
    lm.truncate(st, st.lengths)  # nothing to take back: allowed
    assert rel(lm.step(st, other[0]), lm.step(fresh, other[0])) < TOL


def test_truncate_refuses_an_lstm(dev):
    from bayeslms_amd import model as M
    from bayeslms_amd.incremental import IncrementalLM
    m = M.RNNModel("LSTM", 60, 64, 64, 2, 0.0, True).to(dev).eval()
    lm = IncrementalLM(m, max_streams=2, max_len=16)
    st = lm.start(2)
    lm.step(st, torch.zeros(3, 2, dtype=torch.int64, device=dev))
    with pytest.raises(BayesLMError, match="LSTM"):
        lm.truncate(st, [1, 1])
    assert st.lengths == [3, 3]


# ------------------------------------------------------------------------------------------------------- the driver
VOC = 500


def _model(kind, seed, dev, bayes=False):
    """a small random 2-layer model over VOC words, weights untied.  The decoder is then scaled so that the log-probabilities
    behind a two-word context spread with a standard deviation of 2: far from uniform (between near-uniform distributions every
    draft is accepted and the tests below see nothing), and not a point mass either."""
    from bayeslms_amd import model as M
    from bayeslms_amd.incremental import IncrementalLM
    torch.manual_seed(seed)
    if kind == "transformer":
        m = M.BayesTransformerModel(VOC, 64, 2, 128, 2, 0.0, False, "FFN") if bayes else M.TransformerModel(VOC, 64, 2, 128, 2, 0.0, "gelu", False)
    else:
        m = M.BayesRNNModel("LSTM", VOC, 64, 64, 2, 0.0, False, 3) if bayes else M.RNNModel("LSTM", VOC, 64, 64, 2, 0.0, False)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "lgstd" in k:
                p += 1.0  # weight samples that differ visibly from the mean
    m = m.to(dev).eval()
    lm = IncrementalLM(m, max_streams=1, max_len=4)
    spread = float(lm.step(lm.start(1), torch.tensor([[3], [17]], dtype=torch.int64, device=dev)).std())
    with torch.no_grad():
        m.decoder.weight *= 2.0 / spread
    return m


def _plain_greedy(lm, ctx, W, N):
    """plain greedy generation -> (words (W, N), gap between the two best log-probabilities of each (W, N))"""
    from bayeslms_amd import ops
    st = lm.start(N)
    ids = torch.tensor(ctx, dtype=torch.int64, device=lm.device).view(-1, 1).expand(-1, N).contiguous()
    out, gaps = [], []
    for _ in range(W):
        lp = lm.step(st, ids)
        top = lp.topk(2, dim=-1).values
        gaps.append((top[:, 0] - top[:, 1]).cpu())
        ids = ops.sample_rows(lp, 0.0).view(1, N)
        out.append(ids[0].cpu())
    return torch.stack(out), torch.stack(gaps)


@pytest.mark.parametrize("kinds", [("transformer", "lstm"), ("lstm", "transformer"), ("transformer", "transformer")])
def test_greedy_speculation_equals_plain_greedy_generation(dev, kinds):
    """temperature 0 with an unrelated draft: word for word the plain greedy output; a difference is admitted only at a word
    where the plain run's two best log-probabilities lie within 1e-4 of each other (the chunk and the single step round differently)."""
    from bayeslms_amd.incremental import IncrementalLM
    from bayeslms_amd.speculative import SpeculativeLM
    N, W, ctx = 3, 24, [3, 17, 250, 4]
    target = IncrementalLM(_model(kinds[0], 1, dev), max_streams=N, max_len=len(ctx) + W + 4)
    draft = IncrementalLM(_model(kinds[1], 2, dev), max_streams=N, max_len=len(ctx) + W + 4)
    want, gaps = _plain_greedy(target, ctx, W, N)
    out, stats = SpeculativeLM(target, draft, 4).generate(ctx, W, N, 0.0, 5)
    assert all(len(o) == W for o in out) and stats.target_chunks >= stats.rounds >= -(-W // 5)
    for j in range(N):
        for i in range(W):
            if out[j][i] != int(want[i, j]):
                assert float(gaps[i, j]) < 1e-4, (j, i, out[j][i], int(want[i, j]), float(gaps[i, j]))
                break  # the two runs continue from different words


@pytest.mark.parametrize("kind", ["transformer", "lstm"])
def test_own_mean_weights_as_draft_are_accepted(dev, kind):
    """Draft = the target's own model, both at mean weights: p and q differ by rounding only, at least 0.99 of the drafts pass."""
    from bayeslms_amd.incremental import IncrementalLM
    from bayeslms_amd.speculative import SpeculativeLM
    N, W, ctx = 8, 30, [3, 17]
    m = _model(kind, 3, dev)
    target = IncrementalLM(m, max_streams=N, max_len=len(ctx) + W + 4)
    draft = IncrementalLM(m, max_streams=N, max_len=len(ctx) + W + 4)
    out, stats = SpeculativeLM(target, draft, 4).generate(ctx, W, N, 1.0, 7)
    assert all(len(o) == W and all(0 <= w < VOC for w in o) for o in out)
    assert stats.accepted >= 0.99 * stats.drafted, stats
    assert len({tuple(o) for o in out}) > 1  # the streams draw their own words


@pytest.mark.parametrize("kind", ["transformer", "lstm"])
def test_model_average_target_with_its_own_mean_weight_draft(dev, kind):
    """mc_samples = 4, draft = None: the run completes and SpecStats adds up; the FIRST generated word over 64 streams x 64 seeds
    is distributed as exp(log pbar) of lm.step: counts within 4 standard errors, over the words expected at least 5 times."""
    from bayeslms_amd.incremental import IncrementalLM
    from bayeslms_amd.speculative import SpeculativeLM
    N, ctx, G = 64, [3, 17, 99], 3
    m = _model(kind, 4, dev, bayes=True)
    target = IncrementalLM(m, max_streams=N, max_len=len(ctx) + 12 + G, mc_samples=4, seed=31)
    spec = SpeculativeLM(target, None, G)
    assert spec.draft.mc_samples == 0 and spec.draft.model is m
    out, stats = spec.generate(ctx, 12, 5, 1.0, 3)
    assert len(out) == 5 and all(len(o) == 12 and all(0 <= w < VOC for w in o) for o in out)
    assert stats.rounds >= 3 and stats.drafted % G == 0 and 0 <= stats.accepted <= stats.drafted
    assert 5 * 12 <= stats.accepted + stats.drafted // G <= 5 * 12 + 5 * G  # every stream-round emits n_acc + 1 words; the cut drops <= G each
    assert not m.training
    st = target.start(1)
    p = target.step(st, torch.tensor(ctx, dtype=torch.int64, device=dev).view(-1, 1))[0].double().exp().cpu()
    assert abs(float(p.sum()) - 1.0) < 1e-4
    first = []
    for seed in range(64):
        o, _ = spec.generate(ctx, 1, N, 1.0, 1000 + seed)
        first += [w[0] for w in o]
    n = len(first)
    assert n == 4096
    cnt = torch.bincount(torch.tensor(first), minlength=VOC).double()
    often = n * p >= 5
    se = torch.sqrt(n * p * (1 - p))
    print("words expected >= 5 times: %d; largest deviation %.2f standard errors"
          % (int(often.sum()), float(((cnt - n * p).abs() / se)[often].max())))
    assert int(often.sum()) >= 10
    assert torch.all(((cnt - n * p).abs() <= 4 * se)[often]), ((cnt - n * p).abs() / se)[often].max()


def test_cli_speculates_end_to_end(dev, tmp_path):
    from bayeslms_amd import model as M
    torch.manual_seed(21)
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(38)]
    m = M.BayesTransformerModel(len(words), 32, 2, 64, 2, 0.5, True, "FFN")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    path, voc = str(tmp_path / "model.pt"), tmp_path / "words.txt"
    torch.save(sd, path)
    voc.write_text("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    o = tmp_path / "out.txt"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "bayeslms_amd.generate", "--model-path", path, "--vocabulary", str(voc), "--model",
                        "Transformer", "--emsize", "32", "--nhid", "64", "--nlayers", "2", "--nhead", "2", "--uncertainty", "Bayesian",
                        "--T_bayes_pos", "FFN", "--words", "7", "--streams", "3", "--seed", "5", "--speculate", "4", "--mc-samples", "2",
                        "--prompt", "w3 w7", "--outf", str(o)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = o.read_text().splitlines()
    assert len(lines) == 3 and all(len(line.split()) == 7 and all(w in words for w in line.split()) for line in lines)
    stats = [line for line in r.stderr.splitlines() if line.startswith("speculative sampling:")]
    assert len(stats) == 1 and "acceptance rate" in stats[0] and "words per target chunk" in stats[0]
