"""GPU: the distillation temperature -- blm_ce_soft_temp_fwd_bwd and blm_ce_soft_topk_temp_fwd_bwd against float64 of the same
float32 operands in every kernel form (register rows NV = 3 / 9 / 16, the sweeping forms, aligned and not), their properties
(temperature 1 is the untempered kernel on a normalised teacher, a constant on a teacher row changes nothing, top-k is dense on
the scattered teacher, the same bits in place and run after run), the ``temperature`` keyword of the ops against float64
autograd, engine.Trainer.step(soft=(targets, weight, temperature)) and the train command line with --distill-temperature.
The reference is written from the text of include/bayeslm.h; the bars are those of tests/test_gpu_distill.py."""
import copy
import functools
import math
import os
import re

import pytest
import torch

import test_gpu_distill as D0
import test_gpu_distill_topk as D1
from test_gpu_distill import GS, kl_close, rel, strided, within

pytestmark = pytest.mark.gpu

M = 6
BETAS = [0.25, 0.5, 1.0, 2.0, 4.0]
LAMBDAS = [0.0, 0.3, 1.0]
# both sides of every form boundary: 4096 x 3 and 4096 x 9 (dense and top-k), 4096 x 16 (top-k); odd sizes take the unaligned form
VS = [7, 67, 1001, 12288, 12292, 33278, 36864, 36868, 70000]
VS_TOPK = VS + [65536, 65540]
KS = [1, 32, 256]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def reference(z32, l32, tgt, lam, beta, c, gs):
    """The definitions of include/bayeslm.h (blm_ce_soft_temp_fwd_bwd) in float64, on the float32 operands."""
    z, l = z32.double(), l32.double()
    V = z.shape[1]
    zero = torch.zeros_like(z)
    live = l > -math.inf
    has_q = live.any(1)
    ml = torch.where(has_q, l.max(1).values, torch.zeros_like(l[:, 0]))
    shifted = beta * (l.masked_fill(~live, 0.0) - ml[:, None])  # beta (l_v - ml) where live
    e = torch.where(live, shifted.exp(), zero)
    Z = e.sum(1)
    qt = e / Z.clamp(min=1e-300)[:, None]
    m = z.max(1).values
    a = z - m[:, None]
    logl = a.exp().sum(1).log()
    lse = m + logl
    p = (a - logl[:, None]).exp()
    logs = (beta * a).exp().sum(1).log()
    lse_b = beta * m + logs
    pt = (beta * a - logs[:, None]).exp()
    valid = (tgt >= 0) & (tgt < V)
    t = tgt.clamp(0, V - 1)
    nll = torch.where(valid, lse - z.gather(1, t[:, None])[:, 0], torch.zeros_like(lse))
    soft = torch.where(has_q, lse_b - beta * torch.where(live, qt * z, zero).sum(1), torch.zeros_like(lse))
    logZ = Z.clamp(min=1e-300).log()
    kl = torch.where(live, qt * ((shifted - logZ[:, None]) - (beta * a - logs[:, None])), zero).sum(1)
    onehot = torch.zeros_like(z).scatter_(1, t[:, None], 1.0) * valid[:, None]
    grad = ((1 - lam) * (valid[:, None] * p - onehot) + lam * c * beta * has_q[:, None] * (pt - qt)) * gs
    return dict(nll=nll, soft=soft, kl=kl, loss=(1 - lam) * nll + lam * c * soft, grad=grad, lse=lse)


@functools.lru_cache(maxsize=None)
def operands(V):
    """Logits randn * 3; teacher = float64 log-softmax of an independent randn * 3, cast to float32.  Row 0 has three -inf
    teacher columns, row 1 a target outside [0, V), row 2 an all -inf teacher (has_q = 0), row 3 its logits shifted by +80
    (beta z passes 320), row 4 its teacher row shifted by -30 (exp(beta l) underflows without the max shift)."""
    g = torch.Generator().manual_seed(7000 + V)
    z = torch.randn(M, V, generator=g) * 3
    l = torch.log_softmax(torch.randn(M, V, generator=g).double() * 3, 1).float()
    l[0, torch.randperm(V, generator=g)[:3]] = -math.inf
    tgt = torch.randint(0, V, (M,), generator=g)
    tgt[1] = -100
    l[2] = -math.inf
    z[3] += 80.0
    l[4] -= 30.0
    return z, l, tgt


@functools.lru_cache(maxsize=None)
def wanted(V, beta):
    """reference() once per (V, beta), shared: lambda and c enter the loss and the gradient linearly"""
    z, l, tgt = operands(V)
    hard = reference(z, l, tgt, 0.0, beta, 1.0, GS)
    soft = reference(z, l, tgt, 1.0, beta, 1.0, GS)
    return hard, soft


def mixed(hard, soft, lam, c):
    out = dict(hard)
    out["loss"] = (1 - lam) * hard["nll"] + lam * c * hard["soft"]
    out["grad"] = (1 - lam) * hard["grad"] + lam * c * soft["grad"]
    return out


def check(got, want, V, what):
    """The bars of tests/test_gpu_distill.py."""
    for k in ("nll", "soft", "loss", "lse"):
        within(got[k], want[k], (k,) + what)
    kl_close(got["kl"], want["kl"], ("kl",) + what)
    assert rel(got["dbuf"][:, :V], want["grad"]) < 1e-5, what
    s = float(want["loss"].sum())
    assert abs(float(got["loss_sum"]) - s) <= 1e-5 * abs(s), what


def run_dense(dev, zbuf, ld, lbuf, ldq, tgt, lam, beta, c, rows, V, in_place, sum0=0.0):
    from bayeslms_amd import _lib as L
    L.require_gfx950()
    out = {k: torch.full((rows,), float("nan"), device=dev) for k in ("loss", "nll", "soft", "kl", "lse")}
    loss_sum = torch.full((1,), sum0, device=dev)  # the kernel adds to it
    dbuf = zbuf if in_place else torch.full_like(zbuf, 5.0)
    L.calls().blm_ce_soft_temp_fwd_bwd(L.ptr(zbuf), ld, L.ptr(lbuf), ldq, L.ptr(tgt), float(lam), float(beta), float(c), L.ptr(out["loss"]),
                                       L.ptr(out["nll"]), L.ptr(out["soft"]), L.ptr(out["kl"]), L.ptr(out["lse"]), L.ptr(loss_sum),
                                       L.ptr(dbuf), GS, rows, V, L.stream())
    out["loss_sum"], out["dbuf"] = loss_sum, dbuf
    return out


def run_topk(dev, zbuf, ld, ibuf, qbuf, ldk, K, tgt, lam, beta, c, rows, V, in_place, sum0=0.0):
    from bayeslms_amd import _lib as L
    L.require_gfx950()
    out = {k: torch.full((rows,), float("nan"), device=dev) for k in ("loss", "nll", "soft", "kl", "lse")}
    loss_sum = torch.full((1,), sum0, device=dev)
    dbuf = zbuf if in_place else torch.full_like(zbuf, 5.0)
    L.calls().blm_ce_soft_topk_temp_fwd_bwd(L.ptr(zbuf), ld, L.ptr(ibuf), L.ptr(qbuf), ldk, K, L.ptr(tgt), float(lam), float(beta), float(c),
                                            L.ptr(out["loss"]), L.ptr(out["nll"]), L.ptr(out["soft"]), L.ptr(out["kl"]), L.ptr(out["lse"]),
                                            L.ptr(loss_sum), L.ptr(dbuf), GS, rows, V, L.stream())
    out["loss_sum"], out["dbuf"] = loss_sum, dbuf
    return out


# ------------------------------------------------------------------------------------------------ kernels against float64
@pytest.mark.parametrize("pad", [False, True], ids=["ld=V", "ld=V_up_to_4"])
@pytest.mark.parametrize("V", VS)
def test_dense_kernel_against_float64(dev, V, pad):
    z, l, tgt = operands(V)
    ld = (V + 3) // 4 * 4 if pad else V
    ldq = ld + 4  # another stride than the logits'; aligned rows stay aligned
    lbuf, _ = strided(l, ldq, dev, fill=0.0)
    td = tgt.to(dev)
    for beta in BETAS:
        hard, soft = wanted(V, beta)
        for lam in LAMBDAS:
            for c in sorted({1.0, 1.0 / beta ** 2}):
                zbuf, _ = strided(z, ld, dev)
                got = run_dense(dev, zbuf, ld, lbuf, ldq, td, lam, beta, c, M, V, in_place=False)
                check(got, mixed(hard, soft, lam, c), V, (beta, lam, c))
                assert bool((got["dbuf"][:, V:] == 5.0).all()) and bool((zbuf[:, V:] == 7.0).all())  # padding columns are nobody's
                assert torch.equal(zbuf[:, :V].cpu(), z)  # a separate gradient buffer leaves the logits alone
                if lam == 1.0:  # row 2 has no live teacher entry: no soft term and no soft gradient (and, at lambda = 1, no gradient)
                    assert float(got["soft"][2]) == 0.0 and float(got["kl"][2]) == 0.0 and float(got["dbuf"][2, :V].abs().max()) == 0.0
                assert bool((got["kl"] >= -1e-5).all())


@functools.lru_cache(maxsize=None)
def sparse_operands(V, K):
    """The K best entries of operands(V)'s teacher rows, in shuffled order; with K > V the slots behind V are empty (-1).  With
    K >= 3 every row has one empty slot (id -1, its logq NaN: never read) and one -inf entry; with K = 1 row 0's only slot is
    empty and row 5's is -inf (both rows then have no live entry, as row 2 has none at any K).
    -> z, ids (M, K) int32, logq (M, K), tgt, the same teacher as dense (M, V) rows: -inf wherever no live id points"""
    z, l, tgt = operands(V)
    g = torch.Generator().manual_seed(9000 + 300 * V + K)
    n = min(K, V)
    ids = torch.full((M, K), -1, dtype=torch.int32)
    logq = torch.full((M, K), math.nan)
    for r in range(M):
        cols = torch.topk(l[r], n).indices[torch.randperm(n, generator=g)]
        ids[r, :n], logq[r, :n] = cols.to(torch.int32), l[r, cols]
        if n >= 3:
            ids[r, r % n], logq[r, r % n] = -1, math.nan
            logq[r, (r + 1) % n] = -math.inf
    if n < 3:
        ids[0, 0], logq[0, 0] = -1, math.nan
        logq[5, 0] = -math.inf
    return z, ids, logq, tgt, D1.scatter_dense(ids, logq, V)


@functools.lru_cache(maxsize=None)
def wanted_topk(V, K, beta):
    """as wanted(), against the scattered teacher"""
    z, _, _, tgt, scattered = sparse_operands(V, K)
    return reference(z, scattered, tgt, 0.0, beta, 1.0, GS), reference(z, scattered, tgt, 1.0, beta, 1.0, GS)


@pytest.mark.parametrize("pad", [False, True], ids=["ld=V", "ld=V_up_to_4"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("V", VS_TOPK)
def test_topk_kernel_against_float64(dev, V, K, pad):
    z, ids, logq, tgt, scattered = sparse_operands(V, K)
    ld = (V + 3) // 4 * 4 if pad else V
    ldk = K + 3  # rows of ids / logq that start at no particular alignment
    ibuf, qbuf = D1.sparse_bufs(ids, logq, ldk, dev)
    td = tgt.to(dev)
    for beta in BETAS:
        hard, soft = wanted_topk(V, K, beta)
        for lam in LAMBDAS:
            for c in sorted({1.0, 1.0 / beta ** 2}):
                zbuf, _ = strided(z, ld, dev)
                got = run_topk(dev, zbuf, ld, ibuf, qbuf, ldk, K, td, lam, beta, c, M, V, in_place=False)
                check(got, mixed(hard, soft, lam, c), V, (beta, lam, c))
                assert bool((got["dbuf"][:, V:] == 5.0).all()) and bool((zbuf[:, V:] == 7.0).all())
                assert torch.equal(zbuf[:, :V].cpu(), z)


# ------------------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("V", [67, 12288, 33278, 70000])
def test_beta_one_is_the_untempered_dense_kernel_where_the_teacher_sums_to_one(dev, V):
    g = torch.Generator().manual_seed(V)
    z = torch.randn(M, V, generator=g) * 3
    l = torch.log_softmax(torch.randn(M, V, generator=g).double() * 3, 1).float()  # Q = 1 in every row
    tgt = torch.randint(0, V, (M,), generator=g)
    ld = (V + 3) // 4 * 4
    lbuf, _ = strided(l, ld, dev, fill=0.0)
    for lam in LAMBDAS:
        old = D0.run_kernel(dev, strided(z, ld, dev)[0], ld, lbuf, ld, tgt.to(dev), lam, M, V, in_place=False)
        got = run_dense(dev, strided(z, ld, dev)[0], ld, lbuf, ld, tgt.to(dev), lam, 1.0, 1.0, M, V, in_place=False)
        want = {k: old[k].cpu() for k in ("nll", "soft", "kl", "loss", "lse")}
        want["grad"] = old["dbuf"][:, :V].cpu()
        check(got, want, V, (lam,))


@pytest.mark.parametrize("V,K", [(67, 32), (12292, 256), (36868, 32), (70000, 256)])
def test_beta_one_is_the_untempered_topk_kernel_where_the_entries_sum_to_one(dev, V, K):
    g = torch.Generator().manual_seed(V + K)
    z = torch.randn(M, V, generator=g) * 3
    ids = torch.stack([torch.randperm(V, generator=g)[:K] for _ in range(M)]).to(torch.int32)
    logq = torch.log_softmax(torch.randn(M, K, generator=g).double() * 3, 1).float()  # a teacher with all its mass on K words
    tgt = torch.randint(0, V, (M,), generator=g)
    tgt[0] = int(ids[0, 0])
    ld = (V + 3) // 4 * 4
    ibuf, qbuf = D1.sparse_bufs(ids, logq, K, dev)
    for lam in LAMBDAS:
        old = D1.run_kernel(dev, strided(z, ld, dev)[0], ld, ibuf, qbuf, K, K, tgt.to(dev), lam, M, V, in_place=False)
        got = run_topk(dev, strided(z, ld, dev)[0], ld, ibuf, qbuf, K, K, tgt.to(dev), lam, 1.0, 1.0, M, V, in_place=False)
        want = {k: old[k].cpu() for k in ("nll", "soft", "kl", "loss", "lse")}
        want["grad"] = old["dbuf"][:, :V].cpu()
        check(got, want, V, (lam,))


SHIFT = torch.tensor([-3.5, 2.25, 0.0, 11.0, -7.0, 0.625])  # a constant per teacher row


@pytest.mark.parametrize("V", [67, 12288, 36864, 70000])
def test_a_constant_on_a_teacher_row_changes_nothing(dev, V):
    """Renorm-independence: the reference is that of the UNSHIFTED teacher."""
    z, l, tgt = operands(V)
    ld = (V + 3) // 4 * 4
    lbuf, _ = strided(l + SHIFT[:, None], ld, dev, fill=0.0)
    for beta in (0.25, 2.0):
        hard, soft = wanted(V, beta)
        got = run_dense(dev, strided(z, ld, dev)[0], ld, lbuf, ld, tgt.to(dev), 0.3, beta, 1.0 / beta ** 2, M, V, in_place=False)
        check(got, mixed(hard, soft, 0.3, 1.0 / beta ** 2), V, (beta,))
    K = 32
    z, ids, logq, tgt, scattered = sparse_operands(V, K)
    ibuf, qbuf = D1.sparse_bufs(ids, logq + SHIFT[:, None], K, dev)
    for beta in (0.25, 2.0):
        want = reference(z, scattered, tgt, 0.3, beta, 1.0 / beta ** 2, GS)
        got = run_topk(dev, strided(z, ld, dev)[0], ld, ibuf, qbuf, K, K, tgt.to(dev), 0.3, beta, 1.0 / beta ** 2, M, V, in_place=False)
        check(got, want, V, (beta,))


@pytest.mark.parametrize("V,K", [(67, 32), (12288, 256), (36868, 32), (65540, 256)])
def test_topk_is_dense_on_the_scattered_teacher(dev, V, K):
    z, ids, logq, tgt, scattered = sparse_operands(V, K)
    ld = (V + 3) // 4 * 4
    ibuf, qbuf = D1.sparse_bufs(ids, logq, K + 1, dev)
    lbuf, _ = strided(scattered, ld, dev, fill=0.0)
    for beta in (0.5, 4.0):
        dense = run_dense(dev, strided(z, ld, dev)[0], ld, lbuf, ld, tgt.to(dev), 0.3, beta, 1.0 / beta ** 2, M, V, in_place=False)
        got = run_topk(dev, strided(z, ld, dev)[0], ld, ibuf, qbuf, K + 1, K, tgt.to(dev), 0.3, beta, 1.0 / beta ** 2, M, V, in_place=False)
        want = {k: dense[k].cpu() for k in ("nll", "soft", "kl", "loss", "lse")}
        want["grad"] = dense["dbuf"][:, :V].cpu()
        check(got, want, V, (beta,))


@pytest.mark.parametrize("V,pad", [(67, True), (67, False), (12288, False), (33278, True), (36868, True), (70000, False)])
def test_in_place_and_bit_identical(dev, V, pad):
    from bayeslms_amd import ops
    z, l, tgt = operands(V)
    _, ids, logq, _, _ = sparse_operands(V, 32)
    ld = (V + 3) // 4 * 4 if pad else V
    lbuf, _ = strided(l, ld, dev, fill=0.0)
    ibuf, qbuf = D1.sparse_bufs(ids, logq, 32, dev)
    runs = {"dense": [], "topk": []}
    for det in (False, False, True, True):
        ops.set_deterministic(det)
        try:
            for in_place in (False, True):
                for form in ("dense", "topk"):
                    zbuf, _ = strided(z, ld, dev)
                    if form == "dense":
                        got = run_dense(dev, zbuf, ld, lbuf, ld, tgt.to(dev), 0.3, 0.5, 4.0, M, V, in_place, sum0=2.0)
                    else:
                        got = run_topk(dev, zbuf, ld, ibuf, qbuf, 32, 32, tgt.to(dev), 0.3, 0.5, 4.0, M, V, in_place, sum0=2.0)
                    assert abs(float(got["loss_sum"]) - 2.0 - float(got["loss"].double().sum())) <= 1e-3  # += : the 2 stays in
                    runs[form].append(torch.cat([got["dbuf"][:, :V].reshape(-1)] + [got[k] for k in ("loss", "nll", "soft", "kl", "lse", "loss_sum")]))
                    if in_place:
                        assert bool((zbuf[:, V:] == 7.0).all())
        finally:
            ops.set_deterministic(False)
    for form in runs:
        for r in runs[form][1:]:
            assert torch.equal(r, runs[form][0]), form  # in place or not, run after run, deterministic mode or not: the same bits


# -------------------------------------------------------------------------------------------------------------------- ops
def soft_loss64(logits, tgt, l32, lam, T):
    """mean_m (1 - lam) nll + lam T^2 soft(T) in float64, differentiable in ``logits``: soft = cross entropy of softmax(z / T)
    under the teacher raised to 1 / T and renormalised"""
    nll = torch.logsumexp(logits, 1) - logits.gather(1, tgt[:, None])[:, 0]
    qt = torch.softmax(l32.double() / T, 1)
    soft = -(qt * torch.log_softmax(logits / T, 1)).sum(1)
    return ((1 - lam) * nll + lam * T * T * soft).mean()


@pytest.mark.parametrize("rows,V", [(5, 40), (6, 1001), (3, 33278)])
def test_cross_entropy_soft_temperature_against_float64_autograd(dev, rows, V):
    from bayeslms_amd import ops
    g = torch.Generator().manual_seed(V)
    z = torch.randn(rows, V, generator=g) * 3
    l = torch.log_softmax(torch.randn(rows, V, generator=g).double() * 3, 1).float()
    tgt = torch.randint(0, V, (rows,), generator=g)
    lam, T = 0.3, 2.0
    zr = z.double().requires_grad_(True)
    ref = soft_loss64(zr, tgt, l, lam, T)
    (ref * 1.7).backward()
    want = reference(z, l, tgt, lam, 1.0 / T, T * T, 1.0)
    for unit in (False, True):
        zd = z.to(dev).requires_grad_(True)
        y = zd * 1.0
        loss, parts = ops.cross_entropy_soft(y, tgt.to(dev), l.to(dev), lam, unit_grad=unit, temperature=T)
        assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
        for k in ("nll", "soft"):
            within(getattr(parts, k), want[k], k)  # soft: at temperature, without the factor T^2
        kl_close(parts.kl, want["kl"], "kl")
        (loss * (1.0 if unit else 1.7)).backward()
        assert rel(zd.grad, zr.grad / (1.7 if unit else 1.0)) < 1e-5, unit
        if not unit:
            assert torch.equal(y.detach().cpu(), z)  # its own gradient buffer: the logits stay
    with torch.no_grad():
        loss, parts = ops.cross_entropy_soft(z.to(dev), tgt.to(dev), l.to(dev), lam, temperature=T, soft_scale=1.0)
        plain = reference(z, l, tgt, lam, 1.0 / T, 1.0, 1.0)
        assert abs(float(loss) - float(plain["loss"].mean())) <= 1e-5 * abs(float(plain["loss"].mean()))


@pytest.mark.parametrize("rows,V,K", [(5, 40, 8), (6, 1001, 32), (3, 33278, 256)])
def test_cross_entropy_soft_topk_temperature_against_float64_autograd(dev, rows, V, K):
    from bayeslms_amd import ops
    g = torch.Generator().manual_seed(V + K)
    z = torch.randn(rows, V, generator=g) * 3
    teacher = torch.log_softmax(torch.randn(rows, V, generator=g).double() * 3, 1).float()
    vals, idx = torch.topk(teacher, K, dim=1)
    scattered = D1.scatter_dense(idx.to(torch.int32), vals, V)
    tgt = torch.randint(0, V, (rows,), generator=g)
    lam, T = 0.3, 2.0
    zr = z.double().requires_grad_(True)
    ref = soft_loss64(zr, tgt, scattered, lam, T)  # softmax over a row that is -inf outside the K entries: renormalised over them
    (ref * 1.7).backward()
    want = reference(z, scattered, tgt, lam, 1.0 / T, T * T, 1.0)
    sp = ops.SparseTargets(idx.to(torch.int32).to(dev), vals.to(dev))
    for unit in (False, True):
        zd = z.to(dev).requires_grad_(True)
        y = zd * 1.0
        loss, parts = ops.cross_entropy_soft_topk(y, tgt.to(dev), sp, lam, unit_grad=unit, temperature=T)
        assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
        for k in ("nll", "soft"):
            within(getattr(parts, k), want[k], k)
        kl_close(parts.kl, want["kl"], "kl")
        (loss * (1.0 if unit else 1.7)).backward()
        assert rel(zd.grad, zr.grad / (1.7 if unit else 1.0)) < 1e-5, unit


@pytest.mark.parametrize("V", [67, 1001])
def test_linear_then_cross_entropy_soft_temperature(dev, V):
    """The decoder's padded odd-vocabulary rows go into the tempered loss as they are; the consumed buffer's version is bumped."""
    from bayeslms_amd import ops
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(V)
    T_, B, K, lam, T = 6, 5, 32, 0.5, 2.0
    x = torch.randn(T_, B, K, generator=g) * 0.5
    w = torch.randn(V, K, generator=g) * 0.1
    b = torch.randn(V, generator=g) * 0.1
    tgt = torch.randint(0, V, (T_ * B,), generator=g)
    l = torch.log_softmax(torch.randn(T_ * B, V, generator=g).double() * 2, 1).float()
    leaves = [a.double().requires_grad_(True) for a in (x, w, b)]
    ref = soft_loss64(F.linear(*leaves).view(-1, V), tgt, l, lam, T)
    ref.backward()
    lbuf, lview = strided(l, (V + 3) // 4 * 4 + 4, dev, fill=0.0)
    for unit in (True, False):
        xs, ws, bs = [a.to(dev).requires_grad_(True) for a in (x, w, b)]
        y = ops.linear(xs, ws, bs)
        assert y.stride(-2) == (V + 3) // 4 * 4
        loss, _ = ops.cross_entropy_soft(y.view(-1, V), tgt.to(dev), lview, lam, unit_grad=unit, temperature=T)
        assert abs(float(loss.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
        loss.backward()
        for got, want in zip((xs, ws, bs), leaves):
            assert rel(got.grad, want.grad) < 5e-4, unit
    z = torch.randn(4, V, generator=g).to(dev).requires_grad_(True)
    yz = z * 1.0
    other = (yz * yz).sum()  # another consumer of the logits, from before the loss
    ops.cross_entropy_soft(yz, tgt[:4].to(dev), l[:4].to(dev), lam, unit_grad=True, temperature=T)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):  # consumed: the version was bumped
        other.backward()


@pytest.mark.parametrize("V", [40, 33278])
def test_temperature_one_is_the_old_entry_point_bit_for_bit(dev, V):
    from bayeslms_amd import _lib as L, ops
    rows, lam = 5, 0.3
    g = torch.Generator().manual_seed(V)
    z = torch.randn(rows, V, generator=g) * 3
    l = torch.log_softmax(torch.randn(rows, V, generator=g).double() * 3, 1).float()
    tgt = torch.randint(0, V, (rows,), generator=g).to(dev)
    vals, idx = torch.topk(l, 8, dim=1)
    sp = ops.SparseTargets(idx.to(torch.int32).to(dev), vals.to(dev))
    dev_l = l.to(dev)

    def direct(form):
        """the old entry point as the op calls it in the trainer's case: in place, at scale 1 / rows"""
        zb = z.to(dev)
        o = {k: torch.empty(rows, device=dev) for k in ("loss", "nll", "soft", "kl")}
        total = torch.zeros((), device=dev)
        tail = (float(lam), L.ptr(o["loss"]), L.ptr(o["nll"]), L.ptr(o["soft"]), L.ptr(o["kl"]), None, L.ptr(total), L.ptr(zb), 1.0 / rows,
                rows, V, L.stream())
        if form == "dense":
            L.calls().blm_ce_soft_fwd_bwd(L.ptr(zb), V, L.ptr(dev_l), V, L.ptr(tgt), *tail)
        else:
            L.calls().blm_ce_soft_topk_fwd_bwd(L.ptr(zb), V, L.ptr(sp.ids), L.ptr(sp.logq), 8, 8, L.ptr(tgt), *tail)
        return total / rows, o, zb

    for form in ("dense", "topk"):
        want_loss, want, want_grad = direct(form)
        for kw in (dict(), dict(temperature=1.0), dict(temperature=1, soft_scale=1.0), dict(temperature=1.0, soft_scale=None)):
            zd = z.to(dev).requires_grad_(True)
            y = zd * 1.0
            if form == "dense":
                loss, parts = ops.cross_entropy_soft(y, tgt, dev_l, lam, unit_grad=True, **kw)
            else:
                loss, parts = ops.cross_entropy_soft_topk(y, tgt, sp, lam, unit_grad=True, **kw)
            assert torch.equal(loss.detach(), want_loss)
            assert torch.equal(parts.nll, want["nll"]) and torch.equal(parts.soft, want["soft"]) and torch.equal(parts.kl, want["kl"])
            loss.backward()
            assert torch.equal(zd.grad, want_grad), (form, kw)  # the consumed buffer, handed back untouched


def test_temperature_one_calls_the_old_entry_points_with_the_old_arguments(dev, monkeypatch):
    """Temperature 1 launches exactly what it launched before the keyword: the same entry point, the same argument values --
    so the same bits."""
    from bayeslms_amd import _lib as L, ops
    rows, V = 4, 40
    z, l, tgt = D0.operands(5, V)
    z, l, tgt = z[:rows], l[:rows], tgt[:rows].clamp(0, V - 1)
    vals, idx = torch.topk(l, 8, dim=1)
    sp = ops.SparseTargets(idx.to(torch.int32).to(dev), vals.to(dev))
    real = L.calls()
    called = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if "ce_soft" not in name:
                return fn
            return lambda *a: called.append((name, len(a))) or fn(*a)

    monkeypatch.setattr(ops, "calls", lambda: Spy())
    outs = []
    for kw in (dict(), dict(temperature=1.0), dict(temperature=1.0, soft_scale=1.0), dict(temperature=2.0), dict(temperature=1.0, soft_scale=4.0)):
        with torch.no_grad():
            a, pa = ops.cross_entropy_soft(z.to(dev), tgt.to(dev), l.to(dev), 0.5, **kw)
            b, pb = ops.cross_entropy_soft_topk(z.to(dev), tgt.to(dev), sp, 0.5, **kw)
        outs.append((a, pa, b, pb))
    assert called == [("blm_ce_soft_fwd_bwd", 17), ("blm_ce_soft_topk_fwd_bwd", 19)] * 3 + \
        [("blm_ce_soft_temp_fwd_bwd", 19), ("blm_ce_soft_topk_temp_fwd_bwd", 21)] * 2
    for a, pa, b, pb in outs[1:3]:  # bit-identical to the call without the keyword
        assert torch.equal(a, outs[0][0]) and torch.equal(b, outs[0][2])
        for x, y in zip(pa + pb, outs[0][1] + outs[0][3]):
            assert torch.equal(x, y)
    assert not torch.equal(outs[3][0], outs[0][0]) and not torch.equal(outs[4][0], outs[0][0])


# ------------------------------------------------------------------------------------------------------------- Trainer
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "topk"])
@pytest.mark.parametrize("kind", ["tlm_plain", "lstm_plain"])
def test_trainer_step_at_a_temperature_is_the_step_made_by_hand(dev, kind, sparse):
    from bayeslms_amd import engine, ops
    (data, tgt), = D0.train_batches(dev, 1)
    g = torch.Generator().manual_seed(2)
    logq = torch.log_softmax(torch.randn(D0.ST * D0.SB, D0.SV, generator=g) * 2, 1)
    if sparse:
        vals, idx = torch.topk(logq, 8, dim=1)
        targets = ops.SparseTargets(idx.to(torch.int32).to(dev), vals.to(dev))
    else:
        targets = logq.to(dev)
    a, _ = D0.student(kind, dev)
    b = copy.deepcopy(a)
    tr = engine.Trainer(a, lr=0.5, clip=1.0, kl_scale=1e-3, seed=1111)
    hidden = a.init_hidden(D0.SB) if hasattr(a, "init_hidden") else None
    loss, _, _ = tr.step(data, tgt, hidden, None, soft=(targets, 0.5, 2.0))
    # by hand: the same step with the loss formed through the op (Trainer.step's own sequence, kl_fn = None)
    hand = engine.Trainer(b, lr=0.5, clip=1.0, kl_scale=1e-3, seed=1111)
    b.train()
    b.set_step(0)
    b.set_columns(0, D0.SB)
    hand.flat.zero_grad()
    out = b(data) if hidden is None else b(data, b.init_hidden(D0.SB))[0]
    soft_loss = ops.cross_entropy_soft_topk if sparse else ops.cross_entropy_soft
    mle, parts = soft_loss(out.view(-1, D0.SV), tgt, targets, 0.5, unit_grad=True, temperature=2.0)
    mle.backward()
    hand.reducer.finish()
    ops.clip_sgd(hand.table, hand.clip, hand.lr, hand.momentum, True, 1.0, hand.weight_decay)
    assert abs(float(loss) - float(mle.detach())) <= 1e-5 * abs(float(mle.detach()))
    for got, want in zip(tr.last_soft, (parts.nll.mean(), parts.soft.mean(), parts.kl.mean())):
        assert got.is_cuda and got.dim() == 0 and abs(float(got) - float(want)) <= 1e-5 * max(1.0, abs(float(want)))
    assert rel(tr.flat.flat_param, hand.flat.flat_param) < 1e-3
    for (k, p), (_, r) in zip(a.named_parameters(), b.named_parameters()):
        assert rel(p, r) < 1e-3, k
    # ... and it is another step than the one at temperature 1
    c, _ = D0.student(kind, dev)
    tr1 = engine.Trainer(c, lr=0.5, clip=1.0, kl_scale=1e-3, seed=1111)
    tr1.step(data, tgt, c.init_hidden(D0.SB) if hidden is not None else None, None, soft=(targets, 0.5))
    assert abs(float(tr1.last_soft.soft) - float(tr.last_soft.soft)) > 1e-3


# --------------------------------------------------------------------------------------------------------- command line
def test_cli_temperature_and_one_cache_for_every_temperature(dev, tmp_path, capsys, monkeypatch):
    from bayeslms_amd import distill, ops, train as T
    d = str(tmp_path)
    words = ["<s>", "<unk>", "a", "b", "c"]  # a five-word corpus
    with open(os.path.join(d, "words.txt"), "w") as f:
        f.write("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    g = torch.Generator().manual_seed(4)
    for split, n in (("train", 40), ("valid", 12), ("test", 12)):
        with open(os.path.join(d, split + ".txt"), "w") as f:
            for _ in range(n):
                f.write(" ".join(words[2 + int(i)] for i in torch.randint(0, 3, (7,), generator=g)) + "\n")
    shape = ["--emsize", "32", "--nhid", "32", "--nlayers", "1", "--nhead", "2", "--model", "Transformer", "--tied"]
    run = ["--data", d, "--cuda", "--epochs", "1", "--seq_len", "8", "--batch-size", "4", "--log-interval", "3", "--deterministic", "1"]
    teacher_pt, cache = os.path.join(d, "teacher.pt"), os.path.join(d, "teacher.cache")
    torch.manual_seed(31)
    teacher = T.build_model(T.build_parser().parse_args(shape), len(words))  # a tiny teacher checkpoint, untrained but with an opinion
    with torch.no_grad():
        teacher.encoder.weight.mul_(4.0)
    torch.save(teacher.state_dict(), teacher_pt)
    calls = []
    dense_rows = distill.Teacher.logprobs
    monkeypatch.setattr(distill.Teacher, "logprobs", lambda self, data: calls.append(data.shape) or dense_rows(self, data))

    def student_run(name, temperature, hist):
        T.main(shape + run + ["--save", os.path.join(d, name), "--distill-from", teacher_pt, "--distill-weight", "0.5", "--distill-top-k", "3",
                              "--distill-top-k-renorm", "1", "--distill-cache", cache, "--distill-temperature", temperature], history=hist)
        return capsys.readouterr().out

    try:
        first, second = {}, {}
        out = student_run("student2.pt", "2", first)
        start = [ln for ln in out.splitlines() if ln.startswith("distilling from")]
        assert len(start) == 1 and "temperature 2" in start[0], out
        assert "first epoch computes them" in out and len(calls) > 0
        lines = [ln for ln in out.splitlines() if ln.startswith("| epoch")]
        assert len(lines) >= 2 and all(re.fullmatch(D1.DISTILLED, ln) for ln in lines), lines
        with open(cache, "rb") as f:
            head = f.read(distill.TeacherCache.HEADER_BYTES)
        assert b'"complete": true' in head and b"temperature" not in head  # the cache knows no temperature
        calls[:] = []
        out = student_run("student4.pt", "4", second)
        start = [ln for ln in out.splitlines() if ln.startswith("distilling from")]
        assert len(start) == 1 and "temperature 4" in start[0], out
        assert "loaded from the complete cache" in out and "the teacher does not run" in out and calls == []
        with open(cache, "rb") as f:
            assert f.read(distill.TeacherCache.HEADER_BYTES) == head
        soft2 = [ln.split("| soft")[1] for ln in lines]
        soft4 = [ln.split("| soft")[1] for ln in out.splitlines() if ln.startswith("| epoch")]
        assert len(soft4) == len(soft2) and soft4 != soft2, (soft2, soft4)  # other printed figures
        assert len(first["interval_soft"]) == len(second["interval_soft"]) >= 2
        assert all(math.isfinite(v) and v > 0 for v in first["interval_soft"] + second["interval_soft"])
        assert all(abs(x - y) > 1e-3 for x, y in zip(first["interval_soft"], second["interval_soft"]))
        plain = student_run("student1.pt", "1", {})  # temperature 1: the start-up line of a run without the flag
        start = [ln for ln in plain.splitlines() if ln.startswith("distilling from")]
        assert len(start) == 1 and start[0].endswith("mean weights"), plain  # (the path before it may hold any word)
    finally:
        ops.set_deterministic(False)
