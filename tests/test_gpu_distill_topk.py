"""GPU: distillation from top-k teacher targets -- blm_ce_soft_topk_fwd_bwd against float64 of the same float32 operands in every
kernel form (register rows NV = 3 / 9 / 16, the two-sweep form, aligned and not), in place and bit for bit, and against the
dense blm_ce_soft_fwd_bwd on the scattered teacher; ops.cross_entropy_soft_topk against float64 autograd; distill.Teacher.topk
against torch.topk of the teacher's rows; engine.Trainer.step(soft=(SparseTargets, weight)); the train command line with
--distill-top-k and --distill-cache.  Helpers, models and bars are those of tests/test_gpu_distill.py: the arithmetic is the same."""
import copy
import functools
import math
import os
import re

import pytest
import torch

import test_gpu_distill as D0
from test_gpu_distill import GS, rel, strided, within

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def kl_close(got, want, what):
    """test_gpu_distill.kl_close, |got - want| <= 1e-5 + 1e-4 want, with |want| in the bar: the K entries of a teacher hold a
    mass Q < 1, so sum_j q_j (logq_j - log p_j) is no divergence and may be negative, where the bar as written would ask for
    less than nothing.  For want >= 0 it is the same bar."""
    got, want = got.detach().double().cpu(), want.double().cpu()
    over = ((got - want).abs() - (1e-5 + 1e-4 * want.abs())).max()
    assert float(over) <= 0.0, (what, float(over), float((got - want).abs().max()))


def scatter_dense(ids, logq, V):
    """The sparse rows as a dense float32 teacher: -inf wherever no live id points (the identity the header states)."""
    M, K = ids.shape
    dense = torch.full((M, V), -math.inf)
    for m in range(M):
        live = (ids[m] >= 0) & (ids[m] < V)
        dense[m, ids[m, live].long()] = logq[m, live]
    return dense


@functools.lru_cache(maxsize=8)
def operands(M, V, K):
    """Logits randn * 3 and, per row, K slots cut from the float64 softmax of an independent randn * 3 (its best entries, so
    Q < 1 unless every column is live), in shuffled order.  The rows are built to hit the places the kernel can go wrong:
      row 0  live ids include 0, V - 1 and the first column of the V % 4 tail; the target is among them; one entry is -inf
      row 1  the target is outside [0, V); half of the slots are empty (-1, V, V + 5, 2^31 - 1), their logq is NaN
      row 2  the target is NOT among the live ids; one entry is -inf
      row 3  the target is V - 1, a live id (in the V % 4 tail where there is one)
      row 4  half of the slots live, empty ones (-1) between them; the target is the last live slot
    With K > V the slots beyond V are empty (-1).  -> z (M, V), ids (M, K) int32, logq (M, K), tgt (M,), dense (M, V)"""
    g = torch.Generator().manual_seed(100000 * K + 1000 * M + V)
    z = torch.randn(M, V, generator=g) * 3
    teacher = torch.log_softmax(torch.randn(M, V, generator=g).double() * 3, 1).float()
    ids = torch.full((M, K), -1, dtype=torch.int32)
    logq = torch.full((M, K), math.nan)
    tgt = torch.randint(0, V, (M,), generator=g)
    for m in range(M):
        n = min(K, V) if m != 4 else (min(K, V) + 1) // 2  # row 4 leaves every other slot or so empty
        best = torch.topk(teacher[m], n).indices.tolist()
        forced = []
        if m == 0:
            forced = list(dict.fromkeys([0, V - 1, V // 4 * 4 if V % 4 else V - 2 if V > 1 else 0]))[:n]
        elif m == 3:
            forced = [V - 1]
        cols = forced + [c for c in best if c not in forced][:n - len(forced)]
        cols = [cols[i] for i in torch.randperm(n, generator=g).tolist()]
        slots = torch.randperm(K, generator=g)[:n].sort().values.tolist() if m == 4 else list(range(n))
        for s, c in zip(slots, cols):
            ids[m, s], logq[m, s] = c, teacher[m, c]
        if m == 0:
            tgt[m] = cols[0]
            if n > 1:
                logq[m, slots[1]] = -math.inf
        elif m == 1:
            tgt[m] = V if M == 2 else -100
            for i, s in enumerate(slots[::2]):
                ids[m, s], logq[m, s] = (-1, V, V + 5, 2 ** 31 - 1)[i % 4], math.nan
        elif m == 2:
            tgt[m] = next(c for c in range(V - 1, -1, -1) if c not in cols) if n < V else cols[0]
            logq[m, slots[0]] = -math.inf
        elif m == 3:
            tgt[m] = V - 1
        elif m == 4:
            tgt[m] = cols[-1]
    return z, ids, logq, tgt, scatter_dense(ids, logq, V)


def sparse_bufs(ids, logq, ldk, dev):
    """(M, ldk) device buffers whose padding columns hold an id that looks live and a NaN: neither may be read"""
    M, K = ids.shape
    ibuf = torch.full((M, ldk), 3, dtype=torch.int32, device=dev)
    qbuf = torch.full((M, ldk), math.nan, device=dev)
    ibuf[:, :K], qbuf[:, :K] = ids.to(dev), logq.to(dev)
    return ibuf, qbuf


def run_kernel(dev, zbuf, ld, ibuf, qbuf, ldk, K, tgt, lam, M, V, in_place, sum0=0.0):
    from bayeslms_amd import _lib as L
    L.require_gfx950()
    out = {k: torch.full((M,), float("nan"), device=dev) for k in ("loss", "nll", "soft", "kl", "lse")}
    loss_sum = torch.full((1,), sum0, device=dev)  # the kernel adds to it
    dbuf = zbuf if in_place else torch.full_like(zbuf, 5.0)
    L.calls().blm_ce_soft_topk_fwd_bwd(L.ptr(zbuf), ld, L.ptr(ibuf), L.ptr(qbuf), ldk, K, L.ptr(tgt), float(lam), L.ptr(out["loss"]),
                                       L.ptr(out["nll"]), L.ptr(out["soft"]), L.ptr(out["kl"]), L.ptr(out["lse"]), L.ptr(loss_sum),
                                       L.ptr(dbuf), GS, M, V, L.stream())
    out["loss_sum"], out["dbuf"] = loss_sum, dbuf
    return out


# both sides of 4096 x 3, 4096 x 9 and 4096 x 16 (the register-row forms), small and odd sizes, the two-sweep form above 65536
VS = [7, 40, 67, 1001, 12288, 12292, 33000, 33278, 36864, 36868, 65536, 65540, 70000]


@pytest.mark.parametrize("pad", [False, True], ids=["ld=V", "ld=V_up_to_4"])
@pytest.mark.parametrize("K", [1, 4, 32, 256])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("M", [2, 5])
def test_kernel_against_float64(dev, M, V, K, pad):
    z, ids, logq, tgt, dense = operands(M, V, K)
    ld = (V + 3) // 4 * 4 if pad else V
    ldk = K + 3  # rows of ids / logq that start at no particular alignment
    ibuf, qbuf = sparse_bufs(ids, logq, ldk, dev)
    for lam in (0.0, 0.3, 1.0):
        want = D0.reference(z, dense, tgt, lam, GS)
        zbuf, _ = strided(z, ld, dev)
        got = run_kernel(dev, zbuf, ld, ibuf, qbuf, ldk, K, tgt.to(dev), lam, M, V, in_place=False)
        for k in ("nll", "soft", "loss", "lse"):
            within(got[k], want[k], (k, lam))
        kl_close(got["kl"], want["kl"], ("kl", lam))
        assert rel(got["dbuf"][:, :V], want["grad"]) < 1e-5, lam
        s = float(want["loss"].sum())
        assert abs(float(got["loss_sum"]) - s) <= 1e-5 * abs(s), lam
        assert bool((got["dbuf"][:, V:] == 5.0).all()) and bool((zbuf[:, V:] == 7.0).all())  # padding columns are nobody's
        assert torch.equal(zbuf[:, :V].cpu(), z)  # a separate gradient buffer leaves the logits alone


@pytest.mark.parametrize("V,pad", [(67, True), (67, False), (12288, False), (33278, True), (70000, False)])
def test_in_place_and_bit_identical(dev, V, pad):
    from bayeslms_amd import ops
    M, K = 5, 32
    z, ids, logq, tgt, _ = operands(M, V, K)
    ld = (V + 3) // 4 * 4 if pad else V
    ibuf, qbuf = sparse_bufs(ids, logq, K + 3, dev)
    runs = []
    for det in (False, False, True, True):
        ops.set_deterministic(det)
        try:
            for in_place in (False, True):
                zbuf, _ = strided(z, ld, dev)
                got = run_kernel(dev, zbuf, ld, ibuf, qbuf, K + 3, K, tgt.to(dev), 0.3, M, V, in_place, sum0=2.0)
                assert abs(float(got["loss_sum"]) - 2.0 - float(got["loss"].double().sum())) <= 1e-4  # += : the 2 stays in
                runs.append(torch.cat([got["dbuf"][:, :V].reshape(-1)] + [got[k] for k in ("loss", "nll", "soft", "kl", "lse", "loss_sum")]))
                if in_place:
                    assert bool((zbuf[:, V:] == 7.0).all())
        finally:
            ops.set_deterministic(False)
    for r in runs[1:]:
        assert torch.equal(r, runs[0])  # in place or not, run after run, deterministic mode or not: the same bits


@pytest.mark.parametrize("V", [67, 33000, 33278])
def test_sparse_equals_dense(dev, V):
    """blm_ce_soft_fwd_bwd on the scattered float32 teacher, -inf elsewhere, computes the same thing: the bars of the float64
    comparison, two-sided."""
    M, K = 5, 32
    z, ids, logq, tgt, dense = operands(M, V, K)
    ld = (V + 3) // 4 * 4
    ibuf, qbuf = sparse_bufs(ids, logq, K + 3, dev)
    for lam in (0.0, 0.3, 1.0):
        zbuf, _ = strided(z, ld, dev)
        sp = run_kernel(dev, zbuf, ld, ibuf, qbuf, K + 3, K, tgt.to(dev), lam, M, V, in_place=False)
        zbuf, _ = strided(z, ld, dev)
        lbuf, _ = strided(dense, ld, dev, fill=0.0)
        de = D0.run_kernel(dev, zbuf, ld, lbuf, ld, tgt.to(dev), lam, M, V, in_place=False)
        for a, b in ((sp, de), (de, sp)):
            for k in ("nll", "soft", "loss", "lse"):
                within(a[k], b[k], (k, lam))
            kl_close(a["kl"], b["kl"], ("kl", lam))
            assert rel(a["dbuf"][:, :V], b["dbuf"][:, :V]) < 1e-5, lam
            assert abs(float(a["loss_sum"]) - float(b["loss_sum"])) <= 1e-5 * abs(float(b["loss_sum"])), lam


# ------------------------------------------------------------------------------------------- ops.cross_entropy_soft_topk
def teacher_topk(M, V, K, g, scale=3.0):
    """The K best entries of a random teacher -> (ids (M, K) int32, logq (M, K), the dense float32 rows with -inf elsewhere)"""
    l = torch.log_softmax(torch.randn(M, V, generator=g).double() * scale, 1).float()
    vals, idx = torch.topk(l, K, dim=1)
    ids = idx.to(torch.int32)
    return ids, vals, scatter_dense(ids, vals, V)


@pytest.mark.parametrize("M,V", [(5, 40), (6, 1001), (3, 33278)])
def test_cross_entropy_soft_topk_against_float64_autograd(dev, M, V):
    from bayeslms_amd import ops
    g = torch.Generator().manual_seed(V)
    z = torch.randn(M, V, generator=g) * 3
    ids, logq, dense = teacher_topk(M, V, 8, g)
    tgt = torch.randint(0, V, (M,), generator=g)
    tgt[0] = int(ids[0, 3])  # a target that is also a teacher entry
    lam = 0.3
    zr = z.double().requires_grad_(True)
    ref = D0.soft_loss64(zr, tgt, dense, lam)
    (ref * 1.7).backward()
    want = D0.reference(z, dense, tgt, lam, 1.0)
    sparse = ops.SparseTargets(ids.to(dev), logq.to(dev))
    for unit in (False, True):
        zd = z.to(dev).requires_grad_(True)
        y = zd * 1.0
        before = y._version
        loss, parts = ops.cross_entropy_soft_topk(y, tgt.to(dev), sparse, lam, unit_grad=unit)
        assert isinstance(parts, ops.SoftStats)
        assert (y._version > before) == unit  # unit_grad consumes the logits and says so; otherwise they stay
        assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
        for k in ("nll", "soft"):
            within(getattr(parts, k), want[k], k)
        kl_close(parts.kl, want["kl"], "kl")
        (loss * (1.0 if unit else 1.7)).backward()
        assert rel(zd.grad, zr.grad / (1.7 if unit else 1.0)) < 1e-5, unit
        if not unit:
            assert torch.equal(y.detach().cpu(), z)  # its own gradient buffer: the logits stay
    with torch.no_grad():
        loss, parts = ops.cross_entropy_soft_topk(z.to(dev), tgt.to(dev), sparse, lam)
        assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)) and parts.kl.shape == (M,)


@pytest.mark.parametrize("V", [67, 1001])
def test_linear_then_cross_entropy_soft_topk(dev, V):
    """The decoder's padded odd-vocabulary rows go into the loss as they are, and its backward takes the gradient as it comes."""
    from bayeslms_amd import ops
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(V)
    T, B, D, lam = 6, 5, 32, 0.5
    x = torch.randn(T, B, D, generator=g) * 0.5
    w = torch.randn(V, D, generator=g) * 0.1
    b = torch.randn(V, generator=g) * 0.1
    tgt = torch.randint(0, V, (T * B,), generator=g)
    ids, logq, dense = teacher_topk(T * B, V, 16, g, scale=2.0)
    leaves = [a.double().requires_grad_(True) for a in (x, w, b)]
    ref = D0.soft_loss64(F.linear(*leaves).view(-1, V), tgt, dense, lam)
    ref.backward()
    sparse = ops.SparseTargets(ids.to(dev), logq.to(dev))
    for unit in (True, False):
        xs, ws, bs = [a.to(dev).requires_grad_(True) for a in (x, w, b)]
        y = ops.linear(xs, ws, bs)
        assert y.stride(-2) == (V + 3) // 4 * 4
        loss, _ = ops.cross_entropy_soft_topk(y.view(-1, V), tgt.to(dev), sparse, lam, unit_grad=unit)
        assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
        loss.backward()
        for got, want in zip((xs, ws, bs), leaves):
            assert rel(got.grad, want.grad) < 5e-4, unit


def test_cross_entropy_soft_topk_refusals(dev):
    from bayeslms_amd import ops
    M, V, K = 4, 40, 8
    g = torch.Generator().manual_seed(1)
    z = torch.randn(M, V, generator=g)
    tgt = torch.randint(0, V, (M,), generator=g)
    ids, logq, _ = teacher_topk(M, V, K, g)
    zd, td, sp = z.to(dev), tgt.to(dev), ops.SparseTargets(ids.to(dev), logq.to(dev))
    zg = zd.clone().requires_grad_(True)
    loss, _ = ops.cross_entropy_soft_topk(zg * 1.0, td, sp, 0.5)
    loss.backward(retain_graph=True)
    with pytest.raises(ops.BayesLMError, match="backward ran already"):
        loss.backward()
    y = zg * 1.0
    other = (y * y).sum()  # another consumer of the logits, from before the loss
    ops.cross_entropy_soft_topk(y, td, sp, 0.5, unit_grad=True)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):  # consumed: the version was bumped
        other.backward()
    with pytest.raises(ops.BayesLMError, match="GPU"):
        ops.cross_entropy_soft_topk(z, tgt, ops.SparseTargets(ids, logq), 0.5)
    with pytest.raises(ops.BayesLMError, match="GPU"):
        ops.cross_entropy_soft_topk(zd, td, ops.SparseTargets(ids, logq), 0.5)
    with pytest.raises(ops.BayesLMError, match="int32"):
        ops.cross_entropy_soft_topk(zd, td, ops.SparseTargets(sp.ids.long(), sp.logq), 0.5)
    with pytest.raises(ops.BayesLMError, match="float32"):
        ops.cross_entropy_soft_topk(zd, td, ops.SparseTargets(sp.ids, sp.logq.double()), 0.5)
    with pytest.raises(ops.BayesLMError, match="requires grad"):
        ops.cross_entropy_soft_topk(zd, td, ops.SparseTargets(sp.ids, sp.logq.clone().requires_grad_(True)), 0.5)
    with pytest.raises(ops.BayesLMError, match="SparseTargets"):
        ops.cross_entropy_soft_topk(zd, td, sp.logq, 0.5)
    for bad in (ops.SparseTargets(sp.ids[:M - 1], sp.logq[:M - 1]), ops.SparseTargets(sp.ids, sp.logq[:, :K - 1]),
                ops.SparseTargets(sp.ids.reshape(-1), sp.logq.reshape(-1))):
        with pytest.raises(ops.BayesLMError, match=r"\(M, K\)"):
            ops.cross_entropy_soft_topk(zd, td, bad, 0.5)
    for k in (0, 257):
        with pytest.raises(ops.BayesLMError, match="BLM_TOPK_MAX"):
            ops.cross_entropy_soft_topk(zd, td, ops.SparseTargets(torch.zeros(M, k, dtype=torch.int32, device=dev),
                                                                  torch.zeros(M, k, device=dev)), 0.5)
    with pytest.raises(ops.BayesLMError, match="targets for"):
        ops.cross_entropy_soft_topk(zd, td[:M - 1], sp, 0.5)
    for bad in (-0.1, 1.1, float("nan"), "0.5", None):
        with pytest.raises(ops.BayesLMError, match=r"\[0, 1\]"):
            ops.cross_entropy_soft_topk(zd, td, sp, bad)


# -------------------------------------------------------------------------------------------------------- Teacher.topk
@pytest.mark.parametrize("S", [0, 3], ids=["mean_weights", "S=3"])
@pytest.mark.parametrize("kind", ["tlm_ffn", "lstm_bayes3"])
def test_teacher_topk(dev, kind, S):
    from bayeslms_amd import distill, ops
    k = 8
    m = D0.teacher_model(kind, dev)
    m.train(S == 0)  # found in training mode at mean weights, in eval mode under Monte-Carlo, as the teacher tests there
    m.set_seed(5)
    m.set_step(9)
    found = D0.noise_triple(m)
    t = distill.Teacher(m, mc_samples=S, seed=77)
    rows = []
    dense_rows = t.logprobs
    t.logprobs = lambda data: rows.append(dense_rows(data)) or rows[-1]  # the very rows topk cut its entries from
    for renorm in (False, True):
        t.reset(D0.TB)
        for d in D0.batches(dev, 2):
            sp, kept = t.topk(d, k, renorm=renorm)
            assert m.training == (S == 0) and D0.noise_triple(m) == found  # left as found
            lp = rows[-1][0]
            assert lp.shape == (D0.TT * D0.TB, D0.TV)
            vals, idx = torch.topk(lp, k, dim=1)
            assert isinstance(sp, ops.SparseTargets) and sp.ids.dtype == torch.int32 and sp.logq.dtype == torch.float32
            assert sp.ids.shape == sp.logq.shape == (D0.TT * D0.TB, k) and kept.shape == (D0.TT * D0.TB,)
            assert torch.equal(sp.ids.long(), idx)
            within(kept, vals.double().exp().sum(1), "kept")
            assert bool((kept < 1.0 + 2e-5).all())
            if renorm:
                within(torch.logsumexp(sp.logq.double(), 1), torch.zeros(lp.shape[0], dtype=torch.float64), "renormalised")
                within(sp.logq, vals.double() - vals.double().exp().sum(1).log()[:, None], "renormalised values")
            else:
                assert torch.equal(sp.logq, vals)  # copied, not recomputed
    assert len(rows) == 4
    for bad in (0, D0.TV + 1, 257):
        with pytest.raises(ops.BayesLMError, match="Teacher.topk: k"):
            t.topk(D0.batches(dev, 1)[0], bad)
    assert len(rows) == 4  # refused before the teacher ran


# ------------------------------------------------------------------------------------------------------------- Trainer
def all_columns(logq, g):
    """Dense (M, V) rows as SparseTargets with K = V: every column, in an order of its own per row"""
    M, V = logq.shape
    ids = torch.stack([torch.randperm(V, generator=g) for _ in range(M)])
    return ids.to(torch.int32), logq.gather(1, ids)


@pytest.mark.parametrize("kind", ["tlm", "lstm"])
def test_trainer_sparse_steps_are_the_dense_steps(dev, kind):
    from bayeslms_amd import ops
    bs = D0.train_batches(dev, 3)
    g = torch.Generator().manual_seed(2)
    logq = [torch.log_softmax(torch.randn(D0.ST * D0.SB, D0.SV, generator=g) * 2, 1) for _ in bs]
    sparse = [ops.SparseTargets(*(t.to(dev) for t in all_columns(l, g))) for l in logq]
    a, kl_fn = D0.student(kind, dev)
    b = copy.deepcopy(a)
    _, dense = D0.run_steps(a, kl_fn, bs, [l.to(dev) for l in logq] + [0.5])
    tr, got = D0.run_steps(b, kl_fn, bs, sparse + [0.5])
    for x, y in zip(got, dense):
        assert abs(x - y) <= 1e-5 * abs(y), (got, dense)
    for (k, p), (_, r) in zip(b.named_parameters(), a.named_parameters()):
        assert rel(p, r) < 1e-3, k
    assert tr.last_soft.nll.is_cuda and tr.last_soft.soft.dim() == 0 and math.isfinite(float(tr.last_soft.kl))


@pytest.mark.parametrize("kind", ["tlm", "lstm"])
def test_trainer_weight_zero_is_the_plain_step(dev, kind):
    from bayeslms_amd import ops
    bs = D0.train_batches(dev, 3)
    g = torch.Generator().manual_seed(2)
    sparse = []
    for _ in bs:
        ids, logq, _ = teacher_topk(D0.ST * D0.SB, D0.SV, 8, g, scale=2.0)  # K < V
        sparse.append(ops.SparseTargets(ids.to(dev), logq.to(dev)))
    a, kl_fn = D0.student(kind, dev)
    b = copy.deepcopy(a)
    _, plain = D0.run_steps(a, kl_fn, bs, None)
    tr, soft = D0.run_steps(b, kl_fn, bs, sparse + [0.0])
    for x, y in zip(soft, plain):
        assert abs(x - y) <= 1e-5 * abs(y), (soft, plain)
    for (k, p), (_, r) in zip(b.named_parameters(), a.named_parameters()):
        assert rel(p, r) < 1e-3, k
    tr.world = 2
    data, tgt = bs[0]
    with pytest.raises(ops.BayesLMError, match="data-parallel distillation"):
        tr.step(data, tgt, None, kl_fn, soft=(sparse[0], 0.5))


# --------------------------------------------------------------------------------------------------------- command line
DISTILLED = D0.TODAY + r" \| soft +[\d.]+ \| kd_kl +-?[\d.]+"


def test_cli_cache_end_to_end(dev, tmp_path, capsys, monkeypatch):
    from bayeslms_amd import distill, engine, ops, train as T
    d = str(tmp_path)
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(38)]
    with open(os.path.join(d, "words.txt"), "w") as f:
        f.write("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    g = torch.Generator().manual_seed(4)
    for split, n in (("train", 40), ("valid", 30), ("test", 30)):
        with open(os.path.join(d, split + ".txt"), "w") as f:
            for _ in range(n):
                f.write(" ".join(words[2 + int(i)] for i in torch.randint(0, 38, (7,), generator=g) ** 2 // 38) + "\n")
    shape = ["--emsize", "32", "--nhid", "32", "--nlayers", "1", "--nhead", "2", "--model", "Transformer", "--tied"]
    run = ["--data", d, "--cuda", "--seq_len", "8", "--batch-size", "4", "--log-interval", "3", "--deterministic", "1"]
    bayes = ["--uncertainty", "Bayesian", "--T_bayes_pos", "FFN"]
    teacher_pt, cache = os.path.join(d, "teacher.pt"), os.path.join(d, "teacher.cache")
    calls, handed = [], []
    dense_rows, step = distill.Teacher.logprobs, engine.Trainer.step

    def counted(self, data):
        calls.append(data.shape)
        return dense_rows(self, data)

    def watched(self, data, targets, hidden=None, kl_fn=None, philox_step=None, soft=None):
        if soft is not None:
            assert isinstance(soft[0], ops.SparseTargets)
            handed.append((soft[0].ids.clone(), soft[0].logq.clone()))
        return step(self, data, targets, hidden, kl_fn, philox_step, soft)

    def student_run(name, k="8", teacher=teacher_pt, hist=None):
        T.main(shape + run + ["--epochs", "2", "--save", os.path.join(d, name), "--distill-from", teacher, "--distill-weight", "0.5",
                              "--distill-mc-samples", "2", "--distill-teacher-args", " ".join(shape + bayes), "--distill-top-k", k,
                              "--distill-cache", cache], history=hist)

    try:
        T.main(shape + bayes + run + ["--epochs", "1", "--save", teacher_pt])
        capsys.readouterr()
        monkeypatch.setattr(distill.Teacher, "logprobs", counted)
        monkeypatch.setattr(engine.Trainer, "step", watched)
        first = {}
        student_run("student1.pt", hist=first)
        out = capsys.readouterr().out
        lines = [ln for ln in out.splitlines() if ln.startswith("| epoch")]
        assert len(lines) >= 4 and all(re.fullmatch(DISTILLED, ln) for ln in lines), lines
        assert "top-8 teacher targets" in out and "first epoch computes them" in out
        assert len(handed) % 2 == 0 and len(handed) >= 8
        per_epoch = len(handed) // 2
        assert len(calls) == per_epoch  # the teacher ran for the batches of one epoch, and never again
        with open(cache, "rb") as f:
            head = f.read(distill.TeacherCache.HEADER_BYTES)
        assert b'"complete": true' in head and b'"k": 8' in head
        for (i1, q1), (i2, q2) in zip(handed[:per_epoch], handed[per_epoch:]):  # epoch 2 read what epoch 1 stored
            assert torch.equal(i1, i2) and torch.equal(q1, q2)
        first_handed, handed[:], calls[:] = handed[:per_epoch], [], []

        second = {}
        student_run("student2.pt", hist=second)
        out = capsys.readouterr().out
        assert "top-8 teacher targets" in out and "loaded from the complete cache" in out
        assert calls == [] and len(handed) == 2 * per_epoch  # no teacher forward at all
        for (i1, q1), (i2, q2) in zip(first_handed, handed[:per_epoch]):
            assert torch.equal(i1, i2) and torch.equal(q1, q2)
        assert len(first["interval_loss"]) >= 4 and second["interval_loss"] == first["interval_loss"]  # fixed-order reductions: exactly
        assert second["interval_soft"] == first["interval_soft"] and second["interval_kd_kl"] == first["interval_kd_kl"]

        with pytest.raises(SystemExit, match="field 'k' differs"):  # a cache written for another K
            student_run("student3.pt", k="4")
        other_pt = os.path.join(d, "teacher2.pt")
        sd = torch.load(teacher_pt, map_location="cpu")
        sd["decoder.bias"] = sd["decoder.bias"] + 0.5
        torch.save(sd, other_pt)
        with pytest.raises(SystemExit, match="field 'teacher_sha256' differs"):  # ... for another teacher
            student_run("student3.pt", teacher=other_pt)
        assert calls == []
        with open(cache, "rb") as f:
            assert f.read(distill.TeacherCache.HEADER_BYTES) == head  # a refused file is left as it was
        capsys.readouterr()

        plain = {}
        T.main(shape + run + ["--epochs", "1", "--save", os.path.join(d, "plain.pt")], history=plain)
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("| epoch")]
        assert len(lines) >= 2 and all(re.fullmatch(D0.TODAY, ln) for ln in lines), lines  # flags off: today's lines
        assert "interval_soft" not in plain and handed[2 * per_epoch:] == []
    finally:
        ops.set_deterministic(False)
