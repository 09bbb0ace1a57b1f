"""GPU: distillation of a teacher's next-word distribution -- blm_ce_soft_fwd_bwd against float64 of the same float32 operands
in every kernel form (register rows NV = 3 / 9, the two-sweep form, aligned and not), ops.cross_entropy_soft against float64
autograd, distill.Teacher against passes run by hand, engine.Trainer.step(soft=...) and the train command line."""
import copy
import functools
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

GS = 0.25  # grad_scale of the kernel-level tests


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def within(got, want, what):
    """|got - want| <= 2e-5 max(1, |want|), the bar of tests/test_gpu_row_stats.py and test_gpu_mc_uncertainty.py"""
    got, want = got.detach().double().cpu(), want.double().cpu()
    err = ((got - want).abs() / want.abs().clamp(min=1.0)).max()
    assert float(err) <= 2e-5, (what, float(err))


def kl_close(got, want, what):
    """|got - want| <= 1e-5 + 1e-4 want, two-sided: the bar the mutual information of blm_linear_mc_stats is held to"""
    got, want = got.detach().double().cpu(), want.double().cpu()
    over = ((got - want).abs() - (1e-5 + 1e-4 * want)).max()
    assert float(over) <= 0.0, (what, float(over), float((got - want).abs().max()))


def reference(z32, l32, tgt, lam, gs):
    """The definitions of include/bayeslm.h in float64, on the float32 operands."""
    z, l = z32.double(), l32.double()
    V = z.shape[1]
    q = l.exp()
    pos = q > 0
    Q = q.sum(1)
    lse = torch.logsumexp(z, 1)
    p = (z - lse[:, None]).exp()
    valid = (tgt >= 0) & (tgt < V)
    t = tgt.clamp(0, V - 1)
    nll = torch.where(valid, lse - z.gather(1, t[:, None])[:, 0], torch.zeros_like(lse))
    zero = torch.zeros_like(z)
    soft = Q * lse - torch.where(pos, q * z, zero).sum(1)
    kl = torch.where(pos, q * (l.masked_fill(~pos, 0.0) - z + lse[:, None]), zero).sum(1)
    onehot = torch.zeros_like(z).scatter_(1, t[:, None], 1.0) * valid[:, None]
    grad = ((1 - lam) * (valid[:, None] * p - onehot) + lam * (Q[:, None] * p - q)) * gs
    return dict(nll=nll, soft=soft, kl=kl, loss=(1 - lam) * nll + lam * soft, grad=grad, lse=lse)


@functools.lru_cache(maxsize=None)
def operands(M, V):
    """Logits randn * 3; teacher = float64 log-softmax of an independent randn * 3, cast to float32; row 0 has three -inf
    columns (Q < 1), row 1 a target outside [0, V)."""
    g = torch.Generator().manual_seed(1000 * M + V)
    z = torch.randn(M, V, generator=g) * 3
    l = torch.log_softmax(torch.randn(M, V, generator=g).double() * 3, 1).float()
    l[0, torch.randperm(V, generator=g)[:3]] = -math.inf
    tgt = torch.randint(0, V, (M,), generator=g)
    tgt[1] = V if M == 2 else -100
    return z, l, tgt


def strided(t, ld, dev, fill=7.0):
    """(M, V) on the device as a view of an (M, ld) buffer whose padding holds ``fill``"""
    M, V = t.shape
    buf = torch.full((M, ld), fill, device=dev, dtype=torch.float32)
    buf[:, :V] = t.to(dev)
    return buf, buf[:, :V]


def run_kernel(dev, zbuf, ld, lbuf, ldq, tgt, lam, M, V, in_place, sum0=0.0):
    from bayeslms_amd import _lib as L
    L.require_gfx950()
    out = {k: torch.full((M,), float("nan"), device=dev) for k in ("loss", "nll", "soft", "kl", "lse")}
    loss_sum = torch.full((1,), sum0, device=dev)  # the kernel adds to it
    dbuf = zbuf if in_place else torch.full_like(zbuf, 5.0)
    L.calls().blm_ce_soft_fwd_bwd(L.ptr(zbuf), ld, L.ptr(lbuf), ldq, L.ptr(tgt), float(lam), L.ptr(out["loss"]), L.ptr(out["nll"]),
                                  L.ptr(out["soft"]), L.ptr(out["kl"]), L.ptr(out["lse"]), L.ptr(loss_sum), L.ptr(dbuf), GS, M, V,
                                  L.stream())
    out["loss_sum"], out["dbuf"] = loss_sum, dbuf
    return out


VS = [7, 40, 67, 1001, 12284, 12288, 12292, 33000, 33278, 36864, 36868, 50000, 70000]  # both sides of 4096 x 3 and 4096 x 9


@pytest.mark.parametrize("pad", [False, True], ids=["ld=V", "ld=V_up_to_4"])
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("M", [2, 5])
def test_kernel_against_float64(dev, M, V, pad):
    z, l, tgt = operands(M, V)
    ld = (V + 3) // 4 * 4 if pad else V
    ldq = ld + 4  # another stride than the logits'; aligned rows stay aligned
    for lam in (0.0, 0.3, 1.0):
        want = reference(z, l, tgt, lam, GS)
        zbuf, _ = strided(z, ld, dev)
        lbuf, _ = strided(l, ldq, dev, fill=0.0)
        got = run_kernel(dev, zbuf, ld, lbuf, ldq, tgt.to(dev), lam, M, V, in_place=False)
        for k in ("nll", "soft", "loss", "lse"):
            within(got[k], want[k], (k, lam))
        kl_close(got["kl"], want["kl"], ("kl", lam))
        assert rel(got["dbuf"][:, :V], want["grad"]) < 1e-5, lam
        s = float(want["loss"].sum())
        assert abs(float(got["loss_sum"]) - s) <= 1e-5 * abs(s), lam
        assert bool((got["dbuf"][:, V:] == 5.0).all()) and bool((zbuf[:, V:] == 7.0).all())  # padding columns are nobody's
        assert torch.equal(zbuf[:, :V].cpu(), z)  # a separate gradient buffer leaves the logits alone


@pytest.mark.parametrize("V", [67, 33000, 33278])
@pytest.mark.parametrize("eps", [0.0, 1e-3, 3e-2])
def test_small_kl(dev, V, eps):
    """The student almost on the teacher: kl is summed term by term and stays within its bar where soft - H[q] would cancel."""
    M = 4
    g = torch.Generator().manual_seed(V)
    z = torch.randn(M, V, generator=g) * 3
    l = torch.log_softmax(z.double() + eps * torch.randn(M, V, generator=g).double(), 1).float()
    tgt = torch.randint(0, V, (M,), generator=g)
    ld = (V + 3) // 4 * 4
    for lam in (0.3, 1.0):
        want = reference(z, l, tgt, lam, GS)
        zbuf, _ = strided(z, ld, dev)
        lbuf, _ = strided(l, ld, dev, fill=0.0)
        got = run_kernel(dev, zbuf, ld, lbuf, ld, tgt.to(dev), lam, M, V, in_place=False)
        kl_close(got["kl"], want["kl"], ("kl", lam))
        if eps == 0.0 and lam == 1.0:
            assert float(got["dbuf"][:, :V].abs().max()) <= 2e-5 * GS


@pytest.mark.parametrize("V,pad", [(67, True), (67, False), (12288, False), (33278, True), (50000, False)])
def test_in_place_and_bit_identical(dev, V, pad):
    from bayeslms_amd import ops
    M = 5
    z, l, tgt = operands(M, V)
    ld = (V + 3) // 4 * 4 if pad else V
    runs = []
    for det in (False, False, True, True):
        ops.set_deterministic(det)
        try:
            for in_place in (False, True):
                zbuf, _ = strided(z, ld, dev)
                lbuf, _ = strided(l, ld, dev, fill=0.0)
                got = run_kernel(dev, zbuf, ld, lbuf, ld, tgt.to(dev), 0.3, M, V, in_place, sum0=2.0)
                assert abs(float(got["loss_sum"]) - 2.0 - float(got["loss"].double().sum())) <= 1e-4  # += : the 2 stays in
                runs.append(torch.cat([got["dbuf"][:, :V].reshape(-1)] + [got[k] for k in ("loss", "nll", "soft", "kl", "lse", "loss_sum")]))
                if in_place:
                    assert bool((zbuf[:, V:] == 7.0).all())
        finally:
            ops.set_deterministic(False)
    for r in runs[1:]:
        assert torch.equal(r, runs[0])  # in place or not, run after run, deterministic mode or not: the same bits


# ------------------------------------------------------------------------------------------------ ops.cross_entropy_soft
def soft_loss64(logits, tgt, l32, lam):
    """mean_m (1 - lam) nll + lam soft in float64, differentiable in ``logits``"""
    lse = torch.logsumexp(logits, 1)
    q = l32.double().exp()
    nll = lse - logits.gather(1, tgt[:, None])[:, 0]
    soft = q.sum(1) * lse - (q * logits).sum(1)
    return ((1 - lam) * nll + lam * soft).mean()


@pytest.mark.parametrize("M,V", [(5, 40), (6, 1001), (3, 33278)])
def test_cross_entropy_soft_against_float64_autograd(dev, M, V):
    from bayeslms_amd import ops
    g = torch.Generator().manual_seed(V)
    z = torch.randn(M, V, generator=g) * 3
    l = torch.log_softmax(torch.randn(M, V, generator=g).double() * 3, 1).float()
    tgt = torch.randint(0, V, (M,), generator=g)
    lam = 0.3
    zr = z.double().requires_grad_(True)
    ref = soft_loss64(zr, tgt, l, lam)
    (ref * 1.7).backward()
    want = reference(z, l, tgt, lam, 1.0)
    for unit in (False, True):
        zd = z.to(dev).requires_grad_(True)
        y = zd * 1.0
        loss, parts = ops.cross_entropy_soft(y, tgt.to(dev), l.to(dev), lam, unit_grad=unit)
        assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
        for k in ("nll", "soft"):
            within(getattr(parts, k), want[k], k)
        kl_close(parts.kl, want["kl"], "kl")
        (loss * (1.0 if unit else 1.7)).backward()
        assert rel(zd.grad, zr.grad / (1.7 if unit else 1.0)) < 1e-5, unit
        if not unit:
            assert torch.equal(y.detach().cpu(), z)  # its own gradient buffer: the logits stay
    with torch.no_grad():
        loss, parts = ops.cross_entropy_soft(z.to(dev), tgt.to(dev), l.to(dev), lam)
        assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref)) and parts.kl.shape == (M,)


@pytest.mark.parametrize("V", [67, 1001])
def test_linear_then_cross_entropy_soft(dev, V):
    """The decoder's padded odd-vocabulary rows go into the loss as they are, and its backward takes the gradient as it comes."""
    from bayeslms_amd import ops
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(V)
    T, B, K, lam = 6, 5, 32, 0.5
    x = torch.randn(T, B, K, generator=g) * 0.5
    w = torch.randn(V, K, generator=g) * 0.1
    b = torch.randn(V, generator=g) * 0.1
    tgt = torch.randint(0, V, (T * B,), generator=g)
    l = torch.log_softmax(torch.randn(T * B, V, generator=g).double() * 2, 1).float()
    leaves = [a.double().requires_grad_(True) for a in (x, w, b)]
    ref = soft_loss64(F.linear(*leaves).view(-1, V), tgt, l, lam)
    ref.backward()
    lbuf, lview = strided(l, (V + 3) // 4 * 4 + 4, dev, fill=0.0)
    for unit in (True, False):
        xs, ws, bs = [a.to(dev).requires_grad_(True) for a in (x, w, b)]
        y = ops.linear(xs, ws, bs)
        assert y.stride(-2) == (V + 3) // 4 * 4
        loss, _ = ops.cross_entropy_soft(y.view(-1, V), tgt.to(dev), lview, lam, unit_grad=unit)
        assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
        loss.backward()
        for got, want in zip((xs, ws, bs), leaves):
            assert rel(got.grad, want.grad) < 5e-4, unit


def test_cross_entropy_soft_refusals(dev):
    from bayeslms_amd import ops
    M, V = 4, 40
    z, l, tgt = operands(5, V)
    z, l, tgt = z[:M], l[:M], tgt[:M].clamp(0, V - 1)
    zd = z.to(dev).requires_grad_(True)
    loss, _ = ops.cross_entropy_soft(zd * 1.0, tgt.to(dev), l.to(dev), 0.5)
    loss.backward(retain_graph=True)
    with pytest.raises(ops.BayesLMError, match="backward ran already"):  # as cross_entropy's second backward
        loss.backward()
    y = zd * 1.0
    other = (y * y).sum()  # another consumer of the logits, from before the loss
    ops.cross_entropy_soft(y, tgt.to(dev), l.to(dev), 0.5, unit_grad=True)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):  # consumed: the version was bumped
        other.backward()
    with pytest.raises(ops.BayesLMError, match="GPU"):
        ops.cross_entropy_soft(z, tgt, l, 0.5)
    with pytest.raises(ops.BayesLMError, match="GPU"):
        ops.cross_entropy_soft(z.to(dev), tgt.to(dev), l, 0.5)
    with pytest.raises(ops.BayesLMError, match="requires grad"):
        ops.cross_entropy_soft(z.to(dev), tgt.to(dev), l.to(dev).requires_grad_(True), 0.5)
    with pytest.raises(ops.BayesLMError, match=r"\(M, V\)"):
        ops.cross_entropy_soft(z.to(dev), tgt.to(dev), l.to(dev)[:, :V - 1], 0.5)
    with pytest.raises(ops.BayesLMError, match="float32"):
        ops.cross_entropy_soft(z.to(dev), tgt.to(dev), l.to(dev).double(), 0.5)
    for bad in (-0.1, 1.1, float("nan"), "0.5", None):
        with pytest.raises(ops.BayesLMError, match=r"\[0, 1\]"):
            ops.cross_entropy_soft(z.to(dev), tgt.to(dev), l.to(dev), bad)


# ------------------------------------------------------------------------------------------------------------- Teacher
TV, TD, TT, TB = 97, 128, 6, 3


def teacher_model(kind, dev):
    from bayeslms_amd import model as M
    torch.manual_seed(5)
    if kind == "tlm_ffn":
        m = M.BayesTransformerModel(TV, TD, 2, 256, 2, 0.2, True, "FFN")
    elif kind == "tlm_plain":
        m = M.TransformerModel(TV, TD, 2, 256, 2, 0.2, "gelu", True)
    elif kind == "lstm_var":
        m = M.VariationalRNNModel("LSTM", TV, TD, TD, 2, 0.2, True, "11")
    else:
        m = M.BayesRNNModel("LSTM", TV, TD, TD, 2, 0.2, True, 3)
    with torch.no_grad():
        if kind.startswith("lstm"):
            m.encoder.weight.mul_(4.0)  # the LSTMs' +-0.1 initialisation leaves the distribution almost flat
        for k, p in m.named_parameters():
            if "lgstd" in k:
                p.add_(1.5)  # weight noise that moves the distribution, as the other Monte-Carlo tests raise it
    return m.to(dev)


def batches(dev, n):
    g = torch.Generator().manual_seed(3)
    return [torch.randint(0, TV, (TT, TB), generator=g).to(dev) for _ in range(n)]


def noise_triple(m):
    ns = m.noise_state
    return ns.seed, ns.step, ns.auto_step


@pytest.mark.parametrize("kind", ["tlm_ffn", "lstm_bayes3"])
def test_teacher_at_mean_weights(dev, kind):
    from bayeslms_amd import distill
    m = teacher_model(kind, dev).train()
    found = noise_triple(m)
    t = distill.Teacher(m)
    d1, d2 = batches(dev, 2)
    t.reset(TB)
    (lp1, h1), (lp2, h2) = t.logprobs(d1), t.logprobs(d2)
    assert h1 is None and lp1.shape == (TT * TB, TV) and lp1.dtype == torch.float32 and not lp1.requires_grad
    assert m.training and noise_triple(m) == found  # left as found
    m.eval()
    with torch.no_grad():
        if kind == "tlm_ffn":
            want = [torch.log_softmax(m(d).double(), -1).view(-1, TV) for d in (d1, d2)]
        else:  # two consecutive windows are one forward over their concatenation
            y, _ = m(torch.cat([d1, d2]), m.init_hidden(TB))
            want = list(torch.log_softmax(y.double(), -1).view(2, TT * TB, TV))
    within(lp1, want[0], "window 1")
    within(lp2, want[1], "window 2")
    t.logprobs(d1)
    assert not m.training  # ... also when that was eval mode


@pytest.mark.parametrize("kind", ["tlm_ffn", "lstm_bayes3"])
def test_teacher_monte_carlo(dev, kind):
    from bayeslms_amd import distill, model as M
    S, seed = 3, 77
    m = teacher_model(kind, dev).eval()
    m.set_seed(5)
    m.set_step(9)
    found = noise_triple(m)
    t = distill.Teacher(m, mc_samples=S, seed=seed)
    data = batches(dev, 2)
    t.reset(TB)
    got = [t.logprobs(d) for d in data]
    assert not m.training and noise_triple(m) == found
    recurrent = kind.startswith("lstm")
    with torch.no_grad(), M.mc_sampling(m, seed, S):
        hidden = [m.init_hidden(TB) for _ in range(S)] if recurrent else None
        for d, (logq, h_q) in zip(data, got):
            lps = []
            for s in range(S):
                m.set_step(s)
                if recurrent:
                    y, h = m(d, hidden[s])
                    hidden[s] = M.repackage_hidden(h)
                else:
                    y = m(d)
                lps.append(torch.log_softmax(y.double(), -1).view(-1, TV))
            want = torch.logsumexp(torch.stack(lps), 0) - math.log(S)
            assert logq.shape == (TT * TB, TV) and h_q.shape == (TT * TB,)
            within(logq, want, "log pbar")
            within(h_q, -(want.exp() * want).sum(1), "H[pbar]")
    assert noise_triple(m) == found


def test_teacher_refusals(dev):
    from bayeslms_amd import distill, ops
    ffn = teacher_model("tlm_ffn", dev)
    for S in (1, 65, -2):
        with pytest.raises(ops.BayesLMError, match="mc_samples must be 0"):
            distill.Teacher(ffn, mc_samples=S)
    with pytest.raises(ops.BayesLMError, match="no variational tensor"):
        distill.Teacher(teacher_model("tlm_plain", dev), mc_samples=2)
    ffn.set_local_reparam(True)
    with pytest.raises(ops.BayesLMError, match="local_reparam"):
        distill.Teacher(ffn, mc_samples=2)
    ffn.set_local_reparam(False)
    with pytest.raises(ops.BayesLMError, match="fresh noise at every time step"):
        distill.Teacher(teacher_model("lstm_var", dev), mc_samples=2)
    with pytest.raises(ops.BayesLMError, match="no decoder"):
        distill.Teacher(torch.nn.Linear(4, 4))
    with pytest.raises(ops.BayesLMError, match="reset"):
        distill.Teacher(teacher_model("lstm_bayes3", dev)).logprobs(batches(dev, 1)[0])


# ------------------------------------------------------------------------------------------------------------- Trainer
SV, SD, ST, SB = 67, 32, 8, 4


def student(kind, dev, dropout=0.2):
    from bayeslms_amd import model as M
    torch.manual_seed(21)
    if kind == "tlm":
        m, kl_fn = M.BayesTransformerModel(SV, SD, 2, 64, 2, dropout, True, "FFN"), lambda m: m.transformerlayers[0].linear2.kl_divergence()
        kl_fn.fusable = True
    elif kind == "lstm":
        m, kl_fn = M.BayesRNNModel("LSTM", SV, SD, SD, 2, dropout, True, 3), lambda m: m.rnn.kl_divergence()
        kl_fn.fusable = False
    elif kind == "tlm_plain":
        m, kl_fn = M.TransformerModel(SV, SD, 2, 64, 2, dropout, "gelu", True), None
    else:
        m, kl_fn = M.RNNModel("LSTM", SV, SD, SD, 2, dropout, True), None
    return m.to(dev), kl_fn


def train_batches(dev, n):
    g = torch.Generator().manual_seed(8)
    out = []
    for _ in range(n):
        seq = torch.randint(0, SV, (ST + 1, SB), generator=g).to(dev)
        out.append((seq[:-1].contiguous(), seq[1:].reshape(-1).contiguous()))
    return out


def run_steps(m, kl_fn, bs, soft):
    from bayeslms_amd import engine, model as M
    tr = engine.Trainer(m, lr=0.5, clip=1.0, kl_scale=1e-3, seed=1111)
    hidden = m.init_hidden(SB) if hasattr(m, "init_hidden") else None
    losses = []
    for k, (data, tgt) in enumerate(bs):
        if hidden is not None:
            hidden = M.repackage_hidden(hidden)
        loss, _, hidden = tr.step(data, tgt, hidden, kl_fn, soft=None if soft is None else (soft[k], soft[-1]))
        losses.append(float(loss))
    return tr, losses


@pytest.mark.parametrize("kind", ["tlm", "lstm"])
def test_trainer_weight_zero_is_the_plain_step(dev, kind):
    bs = train_batches(dev, 3)
    g = torch.Generator().manual_seed(2)
    logq = [torch.log_softmax(torch.randn(ST * SB, SV, generator=g) * 2, 1).to(dev) for _ in bs]
    a, kl_fn = student(kind, dev)
    b = copy.deepcopy(a)
    _, plain = run_steps(a, kl_fn, bs, None)
    tr, soft = run_steps(b, kl_fn, bs, logq + [0.0])
    for x, y in zip(soft, plain):
        assert abs(x - y) <= 1e-5 * abs(y), (soft, plain)
    for (k, p), (_, r) in zip(b.named_parameters(), a.named_parameters()):
        assert rel(p, r) < 1e-3, k
    assert tr.last_soft.nll.is_cuda and tr.last_soft.soft.dim() == 0 and math.isfinite(float(tr.last_soft.kl))


@pytest.mark.parametrize("kind", ["tlm_plain", "lstm_plain"])
def test_trainer_student_equal_to_its_teacher_has_no_kl(dev, kind):
    from bayeslms_amd import distill
    t, _ = student(kind, dev, dropout=0.0)
    s = copy.deepcopy(t)
    teacher = distill.Teacher(t.requires_grad_(False))
    teacher.reset(SB)
    (data, tgt), = train_batches(dev, 1)
    logq, _ = teacher.logprobs(data)
    tr, _ = run_steps(s, None, [(data, tgt)], [logq, 0.5])
    assert 0.0 <= float(tr.last_soft.kl) + 1e-5 and float(tr.last_soft.kl) <= 1e-5
    assert abs(float(tr.last_soft.soft) - float(-(logq.double().exp() * logq.double()).sum(1).mean())) <= 1e-4  # = H[q] then


@pytest.mark.parametrize("kind", ["tlm", "lstm"])
def test_trainer_fits_a_fixed_batch(dev, kind):
    from bayeslms_amd import distill, engine, model as M
    teacher = distill.Teacher(teacher_for_students(kind, dev), mc_samples=2)
    (data, tgt), = train_batches(dev, 1)
    m, kl_fn = student(kind, dev)
    tr = engine.Trainer(m, lr=0.2, clip=1.0, kl_scale=1e-3, seed=1111)
    softs, losses = [], []
    for _ in range(30):
        teacher.reset(SB)
        logq, _ = teacher.logprobs(data)
        hidden = m.init_hidden(SB) if hasattr(m, "init_hidden") else None
        loss, _, _ = tr.step(data, tgt, hidden, kl_fn, soft=(logq, 1.0))
        losses.append(float(loss))
        softs.append(float(tr.last_soft.soft))
    assert all(math.isfinite(v) for v in losses + softs), (losses, softs)
    assert softs[-1] < softs[0], softs
    tr.world = 2
    from bayeslms_amd import ops
    with pytest.raises(ops.BayesLMError, match="data-parallel distillation"):
        tr.step(data, tgt, None, kl_fn, soft=(logq, 1.0))


def teacher_for_students(kind, dev):
    from bayeslms_amd import model as M
    torch.manual_seed(99)
    m = (M.BayesTransformerModel(SV, SD, 2, 64, 2, 0.2, True, "FFN") if kind == "tlm" else M.BayesRNNModel("LSTM", SV, SD, SD, 2, 0.2, True, 3))
    with torch.no_grad():
        m.encoder.weight.mul_(4.0)  # a teacher with an opinion: far from uniform
    return m.to(dev).requires_grad_(False)


# --------------------------------------------------------------------------------------------------------- command line
TODAY = (r"\| epoch +\d+ \| +\d+/ +\d+ batches \| lr [\d.]+ \| ms/batch +[\d.]+ \| loss +[\d.]+ \| kl_loss +[-\d.e+]+ \| ppl +[\d.]+")


def test_cli_end_to_end(dev, tmp_path, capsys):
    from bayeslms_amd import train as T
    d = str(tmp_path)
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(38)]
    with open(os.path.join(d, "words.txt"), "w") as f:
        f.write("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    g = torch.Generator().manual_seed(4)
    for split, n in (("train", 90), ("valid", 30), ("test", 30)):
        with open(os.path.join(d, split + ".txt"), "w") as f:
            for _ in range(n):
                f.write(" ".join(words[2 + int(i)] for i in torch.randint(0, 38, (7,), generator=g) ** 2 // 38) + "\n")
    shape = ["--emsize", "32", "--nhid", "32", "--nlayers", "1", "--nhead", "2", "--model", "Transformer", "--tied"]
    run = ["--data", d, "--cuda", "--epochs", "1", "--seq_len", "8", "--batch-size", "4", "--log-interval", "5"]
    bayes = ["--uncertainty", "Bayesian", "--T_bayes_pos", "FFN"]
    teacher_pt, student_pt = os.path.join(d, "teacher.pt"), os.path.join(d, "student.pt")
    T.main(shape + bayes + run + ["--save", teacher_pt])
    assert os.path.exists(teacher_pt)
    capsys.readouterr()
    hist = {}
    T.main(shape + run + ["--save", student_pt, "--distill-from", teacher_pt, "--distill-weight", "0.5", "--distill-mc-samples", "2",
                          "--distill-teacher-args", " ".join(shape + bayes)], history=hist)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("| epoch")]
    assert len(lines) >= 2 and all(re.fullmatch(TODAY + r" \| soft +[\d.]+ \| kd_kl +-?[\d.]+", ln) for ln in lines), lines
    assert len(hist["interval_soft"]) == len(hist["interval_kd_kl"]) == len(hist["interval_loss"]) == len(lines)
    assert all(math.isfinite(v) and v > 0 for v in hist["interval_soft"]) and math.isfinite(hist["test_loss"])
    plain = {}
    T.main(shape + run + ["--save", os.path.join(d, "plain.pt")], history=plain)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("| epoch")]
    assert len(lines) >= 2 and all(re.fullmatch(TODAY, ln) for ln in lines), lines  # flags off: today's lines
    assert "interval_soft" not in plain
    with pytest.raises(SystemExit, match="does not fit the teacher"):  # the default teacher shape is the student's own: not Bayesian
        T.main(shape + run + ["--save", student_pt, "--distill-from", teacher_pt])
