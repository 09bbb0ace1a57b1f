"""GPU: SWAG -- blm_swag_collect / blm_swag_sample / blm_logp_avg_accum (ops.swag_collect, ops.swag_sample, ops.logp_avg_accum)
against the float64 reference of tests/swag_reference.py, then swag.SwagPosterior, engine.evaluate_swag and the two command lines
on tiny models.

Kernel bounds: derived in tests/swag_reference.py from the rounded fp32 operations behind each output, evaluated per element
from the float64 magnitudes of the terms, with a factor 2.  The sample kernel's noise is read back from blm_philox_normal on
the device (the stream itself is pinned bit for bit by the first sample test), so the bound covers arithmetic only.

Through the layers every comparison runs under ops.set_deterministic(): the decoder's logits of two runs on the same weight
bits are then the same bits, and what differs between engine.evaluate_swag and engine.evaluate_report is one fp32 log-softmax
kernel against another.  Either is within e1 = u (28 + 3 D + 4 log V + max|z|) of float64 per token, from swag_reference's
logp_errors with |d_j| <= D = 2 max|z|, trips = 2, depth = 18 (eps_L = u (26 + 2 D)), log L <= log V, |lse| <= max|z| + log V and
|logp| <= D + log V; a fold of the
log-average adds at most u (4 + |acc|) (its rounded steps at t = 1), the final subtraction u (log S + |acc|)."""
import copy
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import swag_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GRID, BLOCK = 2048, 256  # csrc/swag.hip: SWAG_GRID x SWAG_TPB lanes, one float4 each per trip
BIG = BLOCK * 4 * GRID + 5  # beyond the grid cap: lanes loop, a tail remains
SIZES = [1, 3, 4, 5, 1027, BIG]
SEED = 1111
V, W, SEQ, COLS, ROWS = 50, 32, 5, 3, 41


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def deterministic():
    from bayeslms_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(was)


def _up(a, dev, offset=0):
    """the fp32 host array on the device, its base ``offset`` floats past a 16-byte boundary"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 4, device=dev, dtype=torch.float32)
    t = buf[offset:offset + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 * offset
    return t


def _within(got, ref, bound, what):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d of %d beyond the bound, worst |err| %.3e at bound %.3e" % (
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(np.asarray(bound)[bad].max()))


# ------------------------------------------------------------------ collect
_COLLECT = {}


def _collect_inputs(n):
    if n not in _COLLECT:
        rng = np.random.default_rng(2000 + n % 9973)
        mag = 10.0 ** rng.uniform(-4, 2, n)
        mean = (rng.standard_normal(n) * mag).astype(np.float32)
        theta = (mean * (1 + 0.1 * rng.standard_normal(n))).astype(np.float32)
        far = rng.random(n) < 0.1  # a few far from their mean
        theta[far] = (rng.standard_normal(n) * mag).astype(np.float32)[far]
        m2 = (rng.random(n) * (0.1 * mag) ** 2).astype(np.float32)
        _COLLECT[n] = (theta, mean, m2)
    return _COLLECT[n]


@pytest.mark.parametrize("with_dev", [True, False])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_collect_matches_float64(dev, n, offset, with_dev):
    from bayeslms_amd import ops
    theta, mean, m2 = _collect_inputs(n)
    for count in (0, 1, 7):
        t = _up(theta, dev, offset)
        fill = np.full(n, np.nan, np.float32)
        m, q = _up(fill if count == 0 else mean, dev, offset), _up(fill if count == 0 else m2, dev, offset)
        d = _up(fill, dev, offset) if with_dev else None
        ops.swag_collect(t, m, q, count, d)
        rm, rq, rd = R.collect(theta, mean, m2, count)
        bm, bq, bd = R.collect_bound(theta, mean, m2, count)
        if count == 0:  # exactly theta, 0, 0, whatever was there
            assert torch.equal(m, t) and not q.any() and (d is None or not d.any())
        _within(m, rm, bm, "mean n=%d count=%d" % (n, count))
        _within(q, rq, bq, "m2 n=%d count=%d" % (n, count))
        if with_dev:
            _within(d, rd, bd, "dev n=%d count=%d" % (n, count))
        assert torch.equal(t, torch.from_numpy(theta).to(dev))  # theta is read only


def test_posterior_ring_wraps_and_five_iterates_give_numpys_moments(dev):
    from bayeslms_amd import swag
    n = 1027
    rng = np.random.default_rng(7)
    thetas = (rng.standard_normal((5, n)) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
    post = swag.SwagPosterior(n, 2, dev)
    mean64, m264 = np.zeros(n), np.zeros(n)
    e_mean, e_m2 = np.zeros(n), np.zeros(n)
    rows = {}
    for i, th in enumerate(thetas):
        prev_mean, prev_m2 = post.mean.cpu().numpy(), post.m2.cpu().numpy()
        assert post.collect(torch.from_numpy(th).to(dev)) == i + 1
        # each step against the reference fed with the kernel's own previous outputs
        rm, rq, rd = R.collect(th, prev_mean, prev_m2, i)
        bm, bq, bd = R.collect_bound(th, prev_mean, prev_m2, i)
        _within(post.mean, rm, bm, "mean, step %d" % i)
        _within(post.m2, rq, bq, "m2, step %d" % i)
        _within(post.dev[i % 2], rd, bd, "deviation row %d, step %d" % (i % 2, i))
        rows[i % 2] = post.dev[i % 2].clone()
        if i:
            assert torch.equal(post.dev[(i + 1) % 2], rows[(i + 1) % 2])  # the other row is untouched
        # and the float64 chain, whose end is numpy's mean and population variance; the kernel's distance from it: a step's own
        # bound, the mean's earlier error carried with weight n / (n + 1) <= 1, and into m2 through d and dev: 2 |d| e_mean
        d64 = R.f64(th) - mean64
        mean64 = mean64 + d64 / (i + 1.0)
        m264 = m264 + d64 * (R.f64(th) - mean64)
        e_m2 = e_m2 + bq + 2 * np.abs(d64) * e_mean
        e_mean = e_mean + bm
    assert post.n == 5 and post.k_live == 2
    t64 = thetas.astype(np.float64)
    np.testing.assert_allclose(mean64, t64.mean(0), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(m264 / 5, t64.var(0), rtol=1e-9, atol=1e-300)
    _within(post.mean, t64.mean(0), e_mean, "mean after five iterates")
    _within(post.m2, 5 * t64.var(0), e_m2, "m2 after five iterates")


# ------------------------------------------------------------------ sample
def _philox(dev, n, stream, step, seed=SEED):
    from bayeslms_amd import _lib as L
    import ctypes as C
    out = torch.empty(n, device=dev, dtype=torch.float32)
    r = L.rng(seed, stream, step)
    L.calls().blm_philox_normal(L.ptr(out), n, C.byref(r), L.stream())
    return out


_SAMPLE = {}


def _sample_inputs(n, K):
    """mean, m2 (zeros and values below the floor among them), K deviation rows: fp32 host arrays, made once, never written"""
    if (n, K) not in _SAMPLE:
        rng = np.random.default_rng(3000 + n % 9973 + K)
        mag = 10.0 ** rng.uniform(-3, 1, n)
        mean = (rng.standard_normal(n) * mag).astype(np.float32)
        m2 = (rng.random(n) * (0.2 * mag) ** 2 * 6).astype(np.float32)
        m2[rng.random(n) < 0.15] = 0.0
        m2[rng.random(n) < 0.15] *= np.float32(1e-9)
        dev_rows = (rng.standard_normal((K, n)) * 0.2 * mag).astype(np.float32)
        _SAMPLE[(n, K)] = (mean, m2, dev_rows)
    return _SAMPLE[(n, K)]


def _check_samples(dev, n, k_live, ids, offset=0, pad=0, diag=False, n_iter=6, floor=1e-6, scale=0.5):
    from bayeslms_amd import _lib as L, ops
    mean, m2, rows = _sample_inputs(n, max(k_live, 1))
    a, b, k = R.coefficients(scale, k_live, diag)
    m, q = _up(mean, dev, offset), _up(m2, dev, offset)
    d = None
    if k:
        buf = torch.empty(k * (n + pad) + 4, device=dev, dtype=torch.float32)
        d = buf[offset:offset + k * (n + pad)].view(k, n + pad)[:, :n]
        d.copy_(torch.from_numpy(rows[:k]))
    obuf = torch.full((len(ids) * (n + pad) + 4,), float("nan"), device=dev, dtype=torch.float32)
    out = obuf[offset:offset + len(ids) * (n + pad)].view(len(ids), n + pad)[:, :n]
    ops.swag_sample(out, m, q, ids, SEED, a, b, 1.0 / n_iter, floor, dev=d, k_live=k)
    for j, i in enumerate(ids):
        z1 = _philox(dev, n, L.STREAM_SWAG, i).cpu().numpy()
        z2 = _philox(dev, k, L.STREAM_SWAG + 1, i).cpu().numpy() if k else None
        args = (mean, m2, n_iter, a, b, floor, z1, rows[:k] if k else None, z2)
        _within(out[j], R.sample(*args), R.sample_bound(*args), "sample id %d, n=%d k=%d J=%d" % (i, n, k, len(ids)))
    if pad:  # nothing is written between the rows
        full = obuf[offset:offset + len(ids) * (n + pad)].view(len(ids), n + pad)
        assert torch.isnan(full[:, n:]).all()
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sample_stream_is_blm_philox_normals(dev, n):
    """mean 0, m2 = n = 4 iterates, a = 1, b = 0: var = 4 * 0.25 = 1 exactly, out = fma(1, z, 0) = z"""
    from bayeslms_amd import _lib as L, ops
    for offset, ids in ((0, [0]), (0, [3, 9, 4]), (1, [7] if n == BIG else [2, 11])):
        mean, m2 = _up(np.zeros(n), dev, offset), _up(np.full(n, 4.0), dev, offset)
        out = _up(np.full((len(ids), n), np.nan), dev, offset)
        ops.swag_sample(out, mean, m2, ids, SEED, 1.0, 0.0, 0.25, 0.0)
        for j, i in enumerate(ids):
            assert torch.equal(out[j], _philox(dev, n, L.STREAM_SWAG, i)), (n, offset, i)


@pytest.mark.parametrize("n", SIZES)
def test_sample_matches_float64_at_every_size(dev, n):
    _check_samples(dev, n, 2, [0, 1, 2])


@pytest.mark.parametrize("k_live", [0, 1, 2, 20, 32])
def test_sample_matches_float64_at_every_rank(dev, k_live):
    out = _check_samples(dev, 1027, k_live, [4, 5])
    if k_live == 1:  # one deviation row is the diagonal form: the same bits as none
        assert torch.equal(out, _check_samples(dev, 1027, 0, [4, 5]))


@pytest.mark.parametrize("J", [1, 2, 3, 8])
def test_sample_matches_float64_at_every_count(dev, J):
    _check_samples(dev, 1027, 5, list(range(10, 10 + J)))
    _check_samples(dev, 1027, 5, list(range(J)), diag=True)


@pytest.mark.parametrize("offset,pad", [(0, 4), (0, 3), (1, 0), (3, 1)])
def test_sample_honours_strides_and_unaligned_bases(dev, offset, pad):
    a = _check_samples(dev, 1027, 6, [1, 2, 3], offset=offset, pad=pad)
    assert torch.equal(a, _check_samples(dev, 1027, 6, [1, 2, 3]))  # the scalar path gives the 16-byte path's bits


def test_sample_is_a_function_of_its_id_alone(dev):
    from bayeslms_amd import swag
    n, K = 1027, 6
    mean, m2, rows = _sample_inputs(n, K)
    post = swag.SwagPosterior(n, K, dev)
    post.mean.copy_(torch.from_numpy(mean)); post.m2.copy_(torch.from_numpy(m2)); post.dev.copy_(torch.from_numpy(rows)); post.n = 9
    alone = post.draw(1, SEED, first=5)[0]
    first_of_8 = post.draw(8, SEED, first=5)[0]
    last_of_8 = post.draw(8, SEED, first=0)[5]
    slot7 = post.draw(8, SEED, first=0)
    nine = post.draw(9, SEED)  # two launches
    assert torch.equal(alone, first_of_8) and torch.equal(alone, last_of_8) and torch.equal(alone, post.draw(1, SEED, first=5)[0])
    assert torch.equal(nine[:8], slot7) and torch.equal(nine[8], post.draw(1, SEED, first=8)[0]) and torch.equal(nine[5], alone)
    assert torch.equal(post.draw(8, SEED, first=1)[6], slot7[7])  # slot 7 against slot 6
    from bayeslms_amd import ops
    a, b, k = swag.coefficients(0.5, post.k_live)
    last = torch.empty(8, n, device=dev)
    ops.swag_sample(last, post.mean, post.m2, [10, 11, 12, 13, 14, 15, 16, 5], SEED, a, b, 1.0 / post.n, 1e-30, dev=post.dev, k_live=k)
    assert torch.equal(last[7], alone) and torch.equal(last[0], post.draw(1, SEED, first=10)[0])  # id 5 as slot 7 of a list of 8
    assert not torch.equal(alone, post.draw(1, SEED + 1, first=5)[0]) and not torch.equal(nine[4], nine[5])
    assert torch.equal(post.draw(3, SEED, scale=0.0), post.mean.expand(3, n))  # scale 0: the mean, bit for bit


# ------------------------------------------------------------------ logp_avg_accum
def _logits(rng, rows, V_, centre=0.0, spread=3.0):
    return (centre + spread * rng.standard_normal((rows, V_))).astype(np.float32)


def _run_avg(dev, zs, targets, ld=None, offset=0, ld_acc=None):
    from bayeslms_amd import ops
    S, (rows, V_) = len(zs), zs[0].shape
    ld, ld_acc = ld or V_, ld_acc or V_
    abuf = torch.full((rows * ld_acc + 4,), float("nan"), device=dev)
    acc = abuf[offset:offset + rows * ld_acc].view(rows, ld_acc)[:, :V_]
    hsum = torch.full((rows,), float("nan"), device=dev)
    nll_s = torch.full((S, rows), float("nan"), device=dev)
    tg = torch.as_tensor(targets, dtype=torch.int64, device=dev)
    for s, z in enumerate(zs):
        zbuf = torch.zeros(rows * ld + 4, device=dev)
        zt = zbuf[offset:offset + rows * ld].view(rows, ld)[:, :V_]
        zt.copy_(torch.from_numpy(z))
        ops.logp_avg_accum(zt, acc, s, S, tg, hsum, nll_s)
        assert torch.equal(zt.cpu(), torch.from_numpy(z))
    return acc, hsum, nll_s


def _check_avg(dev, zs, targets, **layout):
    acc, hsum, nll_s = _run_avg(dev, zs, targets, **layout)
    ref = R.average(zs, targets)
    got = acc.cpu().numpy().astype(np.float64)
    inf = np.isneginf(ref["acc"])
    assert not np.isnan(got).any() and (np.isneginf(got) == inf).all()
    _within(np.where(inf, 0.0, got), np.where(inf, 0.0, ref["acc"]), ref["b_acc"], "acc")
    _within(hsum, ref["hsum"], ref["b_hsum"], "hsum")
    _within(nll_s, ref["nll_s"], ref["b_nll_s"], "nll_s")
    return acc, hsum, nll_s, ref


@pytest.mark.parametrize("rows,S", [(1, 2), (5, 3)])
@pytest.mark.parametrize("V_", [1, 3, 4, 1000, 33000, 36868])
def test_logp_avg_matches_float64(dev, V_, rows, S):
    rng = np.random.default_rng(V_ + rows)
    zs = [_logits(rng, rows, V_) for _ in range(S)]
    _check_avg(dev, zs, rng.integers(0, V_, rows))


@pytest.mark.parametrize("V_,layout", [(1000, dict(ld=1004)), (1000, dict(ld=1001, ld_acc=1003)), (1000, dict(offset=1)),
                                       (33000, dict(ld=33004, ld_acc=33000)), (33000, dict(ld=33001)), (33000, dict(offset=3)),
                                       (36868, dict(offset=2, ld=36869))])
def test_logp_avg_honours_strides_and_unaligned_bases(dev, V_, layout):
    rng = np.random.default_rng(V_)
    zs = [_logits(rng, 5, V_) for _ in range(2)]
    tg = rng.integers(0, V_, 5)
    acc, hsum, nll_s, _ = _check_avg(dev, zs, tg, **layout)
    plain = _run_avg(dev, zs, tg)
    if V_ <= 36864:  # against the register form on the plain layout: the same sums in another order, so bounds, not bits
        ref = R.average(zs, tg)
        _within(acc, plain[0].cpu().numpy().astype(np.float64), 2 * ref["b_acc"], "acc, two forms")


@pytest.mark.parametrize("layout", [dict(), dict(offset=1), dict(ld=1), dict(ld_acc=3)], ids=["aligned", "offset", "ld", "ld_acc"])
@pytest.mark.parametrize("V_", [1000, 36868])
def test_logp_avg_columns_at_minus_infinity(dev, V_, layout):
    """Columns at -inf in every sample stay -inf in acc and nothing is NaN, in the register form (V 1000, aligned), in the 16-byte
    sweep (V 36868 aligned: columns 4..7 are one lane's whole first float4) and in the scalar sweep (any other layout, where lane
    t meets column t first, so the first value a lane sees is -inf while its running max is still -inf)."""
    rng = np.random.default_rng(5 + V_)
    rows = 5
    layout = {k: (v if k == "offset" else V_ + v) for k, v in layout.items()}  # a stride that is no multiple of 4
    zs = [_logits(rng, rows, V_) for _ in range(3)]
    for z in zs:
        z[:, 4:8] = -np.inf
        z[:, 700] = -np.inf
    zs[1][:, 11] = -np.inf  # in one sample only: the average stays finite
    tg = rng.integers(20, 600, rows)  # finite columns
    tg[0], tg[1] = -100, V_  # outside [0, V): nll_s = 0 there, blm_ce_fwd_bwd's rule
    acc, hsum, nll_s, _ = _check_avg(dev, zs, tg, **layout)
    assert torch.isneginf(acc[:, 4:8]).all() and torch.isneginf(acc[:, 700]).all() and torch.isfinite(acc[:, 11]).all()
    assert not nll_s[:, :2].any() and torch.isfinite(nll_s).all() and torch.isfinite(hsum).all()


@pytest.mark.parametrize("V_", [1000, 36868])
def test_logp_avg_edge_values(dev, V_):
    rng = np.random.default_rng(5 + V_)
    rows = 5
    # logits near 80 and near -80
    for centre in (80.0, -80.0):
        _check_avg(dev, [_logits(rng, rows, V_, centre, 2.0) for _ in range(2)], rng.integers(0, V_, rows))
    # S identical rows: acc = logp, hsum = S H, mi = 0, within the bound
    z = _logits(rng, rows, V_)
    acc, hsum, _, ref = _check_avg(dev, [z, z, z], rng.integers(0, V_, rows))
    logp, H = R.logp_entropy(z)
    _within(acc, logp, ref["b_acc"], "acc of identical samples")
    mi = R.entropy_of_logp(acc.cpu().numpy()) - hsum.cpu().numpy().astype(np.float64) / 3
    assert (np.abs(mi) <= ref["b_hsum"] / 3 + (np.exp(logp) * (1 + np.abs(logp)) * ref["b_acc"]).sum(1)).all()


def test_ops_refuse_what_the_kernels_cannot_take(dev):
    from bayeslms_amd import ops
    f = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    with pytest.raises(ops.BayesLMError, match="sample 2 of 2"):
        ops.logp_avg_accum(f(2, 8), f(2, 8), 2, 2)
    with pytest.raises(ops.BayesLMError, match="go together"):
        ops.logp_avg_accum(f(2, 8), f(2, 8), 0, 2, targets=torch.zeros(2, dtype=torch.int64, device=dev))
    with pytest.raises(ops.BayesLMError, match="k_live = 33"):
        ops.swag_sample(f(1, 8), f(8), f(8), [0], 1, 1.0, 0.0, 1.0, 0.0, dev=f(40, 8), k_live=33)
    with pytest.raises(ops.BayesLMError, match="9 sample ids"):
        ops.swag_sample(f(9, 8), f(8), f(8), list(range(9)), 1, 1.0, 0.0, 1.0, 0.0)
    with pytest.raises(ops.BayesLMError, match="inv_n"):
        ops.swag_sample(f(1, 8), f(8), f(8), [0], 1, 1.0, 0.0, 0.0, 0.0)
    with pytest.raises(ops.BayesLMError, match="has 7 elements"):
        ops.swag_collect(f(8), f(7), f(8), 0)


# ------------------------------------------------------------------ through the layers
def _families(dev):
    from bayeslms_amd import model as M
    torch.manual_seed(3)
    return {"lstm": M.RNNModel("LSTM", V, W, W, 2, 0.0, True).to(dev).eval(),
            "transformer": M.TransformerModel(V, W, 2, W, 2, 0.0, "gelu", True).to(dev).eval(),
            "bayes": M.BayesTransformerModel(V, W, 2, W, 2, 0.0, True, "FFN").to(dev).eval()}


@pytest.fixture(scope="module")
def families(dev):
    return _families(dev)


@pytest.fixture(scope="module")
def text(dev):
    g = torch.Generator().manual_seed(12)
    return torch.randint(0, V, (ROWS, COLS), generator=g).to(dev)  # 3 x 41 tokens: eight windows of 5 rows


def _flat_of(model):
    from bayeslms_amd import swag
    params, offsets, total = swag.flat_layout(model)
    vec = torch.zeros(total, device=params[0].device)
    for p, o in zip(params, offsets):
        vec[o:o + p.numel()] = p.detach().reshape(-1)
    return vec


_POST = {}


def _posterior(model, kind):
    """four iterates around the model's weights, rank 3"""
    from bayeslms_amd import swag
    if kind not in _POST:
        base = _flat_of(model)
        post = swag.SwagPosterior(base.numel(), 3, base.device, swag.manifest_of(model))
        g = torch.Generator(device="cpu").manual_seed(21)
        for _ in range(4):
            post.collect(base * (1 + 0.05 * torch.randn(base.numel(), generator=g).to(base.device)))
        _POST[kind] = post
    return _POST[kind]


def _zmax(model, text):
    with torch.no_grad():
        if hasattr(model, "init_hidden"):
            out, _ = model(text[:-1], model.init_hidden(text.shape[1]))
        else:
            out = torch.cat([model(text[i:i + SEQ]) for i in range(0, text.shape[0] - 1, SEQ)])
    return float(out.abs().max())


def _e1(zmax):
    return U * (28 + 3 * 2 * zmax + 4 * math.log(V) + zmax)


def _eH(zmax):
    """swag_reference.logp_errors' e_H with |d_j| <= D = 2 max|z|, delta_j <= u (8 + 2 D), depth 18, eps_L <= u (26 + 2 D) and
    log L, H <= log V: u (28 + 3 log V + 57 D + 4 D^2)"""
    D = 2 * zmax
    return U * (28 + 3 * math.log(V) + 57 * D + 4 * D * D)


@pytest.mark.parametrize("kind", ["lstm", "transformer", "bayes"])
def test_scale_zero_is_the_report_of_the_swa_mean(dev, families, text, kind, deterministic):
    from bayeslms_amd import engine
    m = families[kind]
    post = _posterior(m, kind)
    S = 3
    rep = engine.evaluate_swag(m, text, SEQ, post, S, scale=0.0, keep_tokens=True)
    mean_model = copy.deepcopy(m)
    mean_model.load_state_dict(post.mean_state_dict(m))
    plain = engine.evaluate_report(mean_model, text, SEQ, keep_tokens=True)
    nll = plain.per_token["nll"].astype(np.float64)
    # S equal samples: two log-softmax kernels (2 e1), S - 1 folds and the subtraction on values of size |nll| + log S
    bound = 2 * (2 * _e1(_zmax(mean_model, text)) + U * ((S - 1) * (4 + nll + math.log(S)) + 2 * math.log(S) + nll))
    print("scale 0 %s: worst |diff| %.3e, least bound %.3e" % (kind, np.abs(rep.per_token["nll"] - nll).max(), bound.min()))
    _within(rep.per_token["nll"], nll, bound, "per-token NLL at scale 0")
    assert rep.tokens == plain.tokens and rep.mc_samples == S and np.array_equal(rep.per_token["rank"], plain.per_token["rank"])
    for s in range(S):
        _within(rep.per_token["nll_s"][:, s], nll, 2 * 2 * _e1(_zmax(mean_model, text)) + 2 * U * nll, "nll_s at scale 0")
    # mi = H[pbar] - hsum / S is 0 for equal samples.  Each entropy is within e_H of float64 (_eH; blm_row_stats' by the same
    # derivation), the sum of S of them and its division add 2 u H, and H[pbar] moves by at most sum_v p_v |log p_v + H| e_acc
    # <= 2 log V e_acc when the row it is formed from is off by e_acc = e1 + the folds' and the subtraction's rounded steps
    zmax, logV = _zmax(mean_model, text), math.log(V)
    lp = 2 * zmax + logV + math.log(S)
    e_acc = _e1(zmax) + U * ((S - 1) * (4 + lp) + 2 * math.log(S) + lp)
    mi_bound = 2 * (2 * _eH(zmax) + 2 * U * logV + 2 * logV * e_acc)
    print("scale 0 %s: worst |mi| %.3e, bound %.3e" % (kind, np.abs(rep.per_token["mi"]).max(), mi_bound))
    assert np.abs(rep.per_token["mi"]).max() <= mi_bound and abs(rep.mean_mi) <= mi_bound


@pytest.mark.parametrize("kind", ["lstm", "transformer", "bayes"])
def test_every_sample_is_a_fresh_model_with_the_drawn_weights(dev, families, text, kind, deterministic):
    """The stale-cache test: nothing derived from the weights may survive the in-place overwrite between samples."""
    from bayeslms_amd import engine
    m = families[kind]
    post = _posterior(m, kind)
    S = 3
    rep = engine.evaluate_swag(m, text, SEQ, post, S, seed=77, scale=0.5, keep_tokens=True)
    draws = post.draw(S, 77, 0.5)
    fresh = []
    for s in range(S):
        ms = _families(dev)[kind]  # built anew, then filled through the manifest
        post.load_flat(ms, draws[s])
        r = engine.evaluate_report(ms, text, SEQ, keep_tokens=True)
        fresh.append(r.per_token["nll"].astype(np.float64))
        e1 = _e1(_zmax(ms, text))
        print("fresh %s sample %d: worst |diff| %.3e, bound %.3e" % (kind, s, np.abs(rep.per_token["nll_s"][:, s] - fresh[s]).max(), 4 * e1))
        _within(rep.per_token["nll_s"][:, s], fresh[s], 2 * (2 * e1 + U * fresh[s]), "nll_s[%d] against a fresh model" % s)
        assert abs(rep.sample_loss[s] - r.loss) <= 4 * e1 + 2 * U * r.loss
    assert max(abs(a - b).max() for a in fresh for b in fresh if a is not b) > 1e-3  # the samples are different models
    f = np.stack(fresh)
    avg = -(np.logaddexp.reduce(-f, 0) - math.log(S))
    bound = 2 * (2 * e1 + U * ((S - 1) * (4 + f.max(0) + math.log(S)) + 2 * math.log(S) + avg))
    _within(rep.per_token["nll"], avg, bound, "NLL of the average against -log mean_s exp(-nll_s)")
    assert abs(rep.loss - avg.mean()) <= bound.max() and rep.mean_mi > 0 and rep.mean_h_pred > 0
    assert sorted(k for k, v in rep.as_dict().items() if v is None) == []  # every field of the --mc-samples report is there


def _snapshot(m):
    from bayeslms_amd import ops
    return ({k: v.clone() for k, v in m.state_dict().items()}, [(p.data_ptr(), p.grad) for p in m.parameters()],
            [mod.training for mod in m.modules()], ops._GRAD_HOOK, ops._EMBED_SINK)


def _assert_restored(m, snap):
    from bayeslms_amd import ops
    sd, ptrs, flags, hook, sink = snap
    now = m.state_dict()
    assert list(now) == list(sd) and all(torch.equal(now[k], sd[k]) for k in sd)
    for p, (ptr, grad) in zip(m.parameters(), ptrs):
        assert p.data_ptr() == ptr and p.grad is grad
    assert [mod.training for mod in m.modules()] == flags
    assert ops._GRAD_HOOK is hook and ops._EMBED_SINK is sink


@pytest.mark.parametrize("kind", ["lstm", "transformer"])
def test_the_model_is_left_as_it_was_found(dev, families, text, kind, deterministic, monkeypatch):
    from bayeslms_amd import engine, ops
    m = copy.deepcopy(families[kind])
    post = _posterior(families[kind], kind)
    before = engine.evaluate_report(m, text, SEQ, keep_tokens=True).per_token["nll"]
    m.train()
    first = next(m.parameters())
    first.grad = torch.full_like(first, 0.25)
    snap = _snapshot(m)
    engine.evaluate_swag(m, text, SEQ, post, 2)
    _assert_restored(m, snap)

    class Stop(Exception):
        pass

    real, calls = ops.logp_avg_accum, []

    def failing(*a, **k):
        calls.append(1)
        if len(calls) == 2:  # mid-way: the second sample of the first window
            raise Stop()
        return real(*a, **k)

    monkeypatch.setattr(ops, "logp_avg_accum", failing)
    with pytest.raises(Stop):
        engine.evaluate_swag(m, text, SEQ, post, 2)
    monkeypatch.undo()
    _assert_restored(m, snap)
    assert torch.equal(first.grad, torch.full_like(first, 0.25))
    assert np.array_equal(engine.evaluate_report(m, text, SEQ, keep_tokens=True).per_token["nll"], before)


def test_one_seed_one_result_and_the_refusals(dev, families, text, deterministic):
    from bayeslms_amd import engine, ops, swag
    m = families["transformer"]
    post = _posterior(m, "transformer")
    a = engine.evaluate_swag(m, text, SEQ, post, 3, seed=5, keep_tokens=True)
    b = engine.evaluate_swag(m, text, SEQ, post, 3, seed=5, keep_tokens=True)
    c = engine.evaluate_swag(m, text, SEQ, post, 3, seed=6, keep_tokens=True)
    for k in ("nll", "nll_s", "h_pred", "mi", "conf", "entropy", "rank"):
        assert np.array_equal(a.per_token[k], b.per_token[k]), k
    assert not np.array_equal(a.per_token["nll"], c.per_token["nll"])
    t = engine.evaluate_swag(m, text, SEQ, post, 3, seed=5, temperature=2.0, keep_tokens=True)
    assert t.temperature["temperature"] == 2.0 and t.loss != a.loss and np.array_equal(t.per_token["h_pred"], a.per_token["h_pred"])
    assert np.array_equal(t.per_token["nll_s"], a.per_token["nll_s"]) and t.mean_entropy > a.mean_entropy
    d = engine.evaluate_swag(m, text, SEQ, post, 3, seed=5, diag=True)
    assert d.loss != a.loss
    for S in (0, 1, 65):
        with pytest.raises(ops.BayesLMError, match="samples must lie in 2..64"):
            engine.evaluate_swag(m, text, SEQ, post, S)
    with pytest.raises(swag.PosteriorMismatch, match="'total'"):
        engine.evaluate_swag(families["lstm"], text, SEQ, post, 2)
    m2 = copy.deepcopy(m)
    m2.set_noise_source("torch")
    with pytest.raises(ops.BayesLMError, match="noise source 'torch'"):
        engine.evaluate_swag(m2, text, SEQ, post, 2)
    with pytest.raises(ops.BayesLMError, match=r"GiB\), beyond the budget"):
        post.draw(3, 1, budget=1000)


# ------------------------------------------------------------------ the command lines
def _corpus(tmp_path):
    d = str(tmp_path)
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(38)]
    with open(os.path.join(d, "words.txt"), "w") as f:
        f.write("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    g = torch.Generator().manual_seed(4)
    for split, n in (("train", 60), ("valid", 20), ("test", 20)):
        with open(os.path.join(d, split + ".txt"), "w") as f:
            for _ in range(n):
                f.write(" ".join(words[2 + int(i)] for i in torch.randint(0, 38, (7,), generator=g) ** 2 // 38) + "\n")
    return d


SHAPE = ["--emsize", "32", "--nhid", "32", "--nlayers", "2", "--model", "LSTM", "--tied"]


def test_train_collects_and_evaluate_reads_the_posterior(dev, tmp_path, capsys, deterministic, monkeypatch):
    from bayeslms_amd import engine, evaluate as E, swag, train as T
    d = _corpus(tmp_path)
    run = ["--data", d, "--cuda", "--epochs", "3", "--seq_len", "8", "--batch-size", "4", "--log-interval", "5", "--seed", "3",
           "--deterministic", "1"]  # two runs from one seed: the same bits
    pt, sw = os.path.join(d, "model.pt"), os.path.join(d, "swag.pt")
    # the weights at every epoch's end, taken from the model itself where the loop hands it to the validation pass (right after
    # the epoch's last step, before any checkpoint is reloaded): nothing of the collector is involved
    seen, real_evaluate = [], engine.evaluate

    def watching(model, *a, **k):
        seen.append(_flat_of(model).cpu().numpy().copy())
        return real_evaluate(model, *a, **k)

    monkeypatch.setattr(engine, "evaluate", watching)
    T.main(SHAPE + run + ["--save", pt, "--swag-save", sw, "--swag-start", "2", "--swag-every", "0", "--swag-rank", "2"])
    monkeypatch.undo()
    assert len(seen) == 4  # three validation passes and the test pass
    out = capsys.readouterr().out
    marks = [ln for ln in out.splitlines() if ln.startswith("| swag n ")]
    assert [int(ln.split()[3]) for ln in marks] == [1, 2]
    post = swag.SwagPosterior.load(sw, dev)
    assert post.n == 2 and post.rank == 2 and post.k_live == 2
    steps = int(re.search(r"step (\d+)", marks[0]).group(1)) // 2  # optimisation steps per epoch: the first mark ends epoch 2
    # the same two iterates, collected by step count in a second run: epoch 2's and epoch 3's last steps
    sw2 = os.path.join(d, "swag2.pt")
    T.main(SHAPE + run + ["--save", os.path.join(d, "m2.pt"), "--swag-save", sw2, "--swag-start", "2", "--swag-every", str(steps),
                          "--swag-rank", "2"])
    marks2 = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("| swag n ")]
    post2 = swag.SwagPosterior.load(sw2, dev)
    assert len(marks2) == 2 and post2.n == 2 and torch.equal(post.mean, post2.mean) and torch.equal(post.m2, post2.m2)
    # the posterior against the float64 moments of the epoch-2 and epoch-3 weights seen above
    t1, t2 = seen[1], seen[2]
    assert np.abs(t1 - t2).max() > 0 and post.total == t1.size
    t64 = np.stack([t1, t2]).astype(np.float64)
    bm, bq, bd = R.collect_bound(t2, t1, np.zeros_like(t1), 1)  # the first iterate is stored exactly: mean = t1, m2 = 0
    _within(post.mean, t64.mean(0), bm, "mean against the two epoch-end weights")
    _within(post.m2, 2 * t64.var(0), bq, "m2 against their population variance")
    _within(post.dev[1], t64[1] - t64.mean(0), bd, "the latest deviation")
    assert not post.dev[0].any()  # the first iterate's deviation from itself
    # --swag-lr pins the logged rate from --swag-start on
    T.main(SHAPE + run + ["--save", os.path.join(d, "m3.pt"), "--swag-save", os.path.join(d, "swag3.pt"), "--swag-start", "2",
                          "--swag-lr", "0.125"])
    lrs = {(int(m.group(1)), m.group(2)) for m in re.finditer(r"\| epoch +(\d+) \|.*?\| lr ([\d.]+)", capsys.readouterr().out)}
    assert {lr for e, lr in lrs if e >= 2} == {"0.125"} and {lr for e, lr in lrs if e == 1} == {"0.100"}
    # without the flags: the same log and the same model.pt from two runs, one of them from another working directory
    outs = []
    for i, cwd in enumerate((os.getcwd(), d)):
        here = os.getcwd()
        os.chdir(cwd)
        try:
            T.main(SHAPE + run + ["--save", os.path.join(d, "plain.pt")])
        finally:
            os.chdir(here)
        log = capsys.readouterr().out
        outs.append((re.sub(r"ms/batch +[\d.]+|time: +[\d.]+s", "", log), open(os.path.join(d, "plain.pt"), "rb").read()))
        assert "swag" not in log
    assert outs[0] == outs[1]

    # ---- the evaluate command line
    base = ["--model-path", pt, "--vocabulary", os.path.join(d, "words.txt"), "--data", os.path.join(d, "test.txt"),
            "--emsize", "32", "--nhid", "32", "--seq-len", "5", "--batch-size", "2"]
    plain = E.main(base)
    line0 = capsys.readouterr().out.strip()
    assert "swag" not in line0 and "swag" not in plain.as_dict()
    rj = os.path.join(d, "r.json")
    rep = E.main(base + ["--swag", sw, "--swag-samples", "3", "--write-report", rj, "--write-tokens", os.path.join(d, "tok.txt")])
    line = capsys.readouterr().out.strip()
    assert re.search(r" \| mc samples 3 \| sample loss [\d.]+ \| h_pred [\d.]+ \| mi [\d.]+ \| swag n 2 rank 2 scale 0.5 samples 3$", line), line
    block = json.load(open(rj))["swag"]
    assert block == {"n": 2, "rank": 2, "k_live": 2, "total": post.total, "scale": 0.5, "diag": False, "samples": 3, "seed": 1111,
                     "path": sw} and rep.mc_samples == 3
    assert len(open(os.path.join(d, "tok.txt")).readline().split()) == 7  # word nll conf entropy rank h_pred mi
    t = E.main(base + ["--swag", sw, "--swag-samples", "2", "--swag-scale", "0.25", "--swag-diag", "1", "--temperature", "2"])
    assert t.swag["scale"] == 0.25 and t.swag["diag"] is True and t.temperature["temperature"] == 2.0
    assert capsys.readouterr().out.strip().endswith("| temperature 2.0000 | swag n 2 rank 2 scale 0.25 samples 2")
    # --swag-samples 0: the SWA mean through the ordinary report
    swa = E.main(base + ["--swag", sw, "--swag-samples", "0"])
    assert capsys.readouterr().out.strip().endswith("| swag n 2 rank 2 scale 0 samples 0") and swa.mc_samples == 0
    mean_pt = os.path.join(d, "mean.pt")
    from bayeslms_amd import model as M
    torch.manual_seed(0)
    shell = M.RNNModel("LSTM", 40, 32, 32, 2, 0.5, True).to(dev)
    torch.save(post.mean_state_dict(shell), mean_pt)
    direct = E.main(["--model-path", mean_pt] + base[2:])
    assert direct.loss == swa.loss and direct.ece == swa.ece and swa.loss != plain.loss
    other = swag.SwagPosterior(8, 0)
    other.mean.zero_(); other.m2.zero_(); other.n = 1
    other.save(os.path.join(d, "other.pt"))
    with pytest.raises(SystemExit, match="field 'total' differs: the posterior has 8"):
        E.main(base + ["--swag", os.path.join(d, "other.pt"), "--swag-samples", "2"])
