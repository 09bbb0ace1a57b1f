"""GPU: SG-MCMC -- blm_sgmcmc_update (ops.sgmcmc_update) against the float64 reference of tests/sgmcmc_reference.py, then
sgmcmc.Sampler under engine.Trainer, engine.evaluate_samples and the two command lines on tiny models.

Kernel bounds: derived in tests/sgmcmc_reference.py from the rounded fp32 operations behind each output, evaluated per element
from the float64 magnitudes of the terms, with a factor 2.  The kernel's noise is pinned bit for bit to blm_philox_normal by the
first test; the float64 comparisons take their noise from oracle.philox.normal, whose distance from the device's stream
(XI_ORACLE, the figure tests/test_gpu_kernels.py holds the two to) enters the bound through the noise's coefficient.

Through the layers every comparison runs under ops.set_deterministic(): two models with the same weight bits then give the same
gradient bits, so a step of the sampler and a step of clip + SGD from the same weights differ by the two update kernels alone,
and each is within the kernel's bound of float64.  A difference made in one step moves the next step's gradients by an amount
no rounding analysis of the update bounds, so the three steps are compared ONE BY ONE: before each step the sampler's trainer
is handed the plain trainer's weights.  The evaluation bounds are those tests/test_gpu_swag.py documents (e1, e_H)."""
import copy
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import sgmcmc_reference as R
from oracle import philox as P

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GRID, BLOCK = 2048, 256  # csrc/sgmcmc.hip: SGM_GRID x SGM_TPB lanes, one float4 each per trip
BIG = BLOCK * 4 * GRID + 5  # beyond the grid cap: lanes loop, a tail remains
SIZES = [1, 3, 4, 5, 1027, BIG]
SEED, STEP = 2 ** 40 + 1111, 7
STREAM = 0x60000000  # BLM_STREAM_SGMCMC
V, W, SEQ, COLS, ROWS = 50, 32, 5, 3, 41
FORMS = [("sgld", 0.0), ("sgld", 0.01), ("psgld", 0.0), ("psgld", 0.01)]  # {sgld, psgld} x {no noise, noise}


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
    print("%s: worst |err| %.3e, worst err / bound %.3f" % (what, float(err.max()), float((err / np.maximum(bound, 1e-300)).max())))
    assert not bad.any(), "%s: %d of %d beyond the bound, worst |err| %.3e at bound %.3e" % (
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(np.asarray(bound)[bad].max()))


_INPUTS, _NOISE = {}, {}


def _inputs(n):
    """p, g, v over six decades, a tenth of the entries with g = 0 and v = 0 (an embedding row the batch did not touch)"""
    if n not in _INPUTS:
        rng = np.random.default_rng(3000 + n % 9973)
        p = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-5, 1, n)).astype(np.float32)
        v = ((rng.standard_normal(n) * 10.0 ** rng.uniform(-5, 1, n)) ** 2).astype(np.float32)
        still = rng.random(n) < 0.1
        g[still] = 0.0
        v[still] = 0.0
        if n >= 3:
            g[0], v[0], p[0] = 0.0, 0.0, 0.0  # moves by the noise alone
        sq = float(np.float32((g.astype(np.float64) ** 2).sum()))
        _INPUTS[n] = (p, g, v, sq)
    return _INPUTS[n]


def _oracle_noise(n, step=STEP):
    if (n, step) not in _NOISE:
        _NOISE[(n, step)] = P.normal(n, SEED, STREAM, step)
    return _NOISE[(n, step)]


def _sq(dev, sq):
    return torch.full((1,), sq, device=dev, dtype=torch.float32)


def _run(dev, n, offset, rule, sigma, clip, gs=0.5, wd=1e-3, lr=0.05, step=STEP, alpha=0.9, damping=1e-5):
    from bayeslms_amd import ops
    p, g, v, sq = _inputs(n)
    pd, gd = _up(p, dev, offset), _up(g, dev, offset)
    vd = _up(v, dev, offset) if rule == "psgld" else None
    out = ops.sgmcmc_update(pd, gd, _sq(dev, sq), clip, lr, sigma, SEED, step, v=vd, grad_scale=gs, weight_decay=wd, alpha=alpha,
                            damping=damping)
    assert out is pd and torch.equal(gd, torch.from_numpy(g).to(dev))  # in place on p; g is read only
    return pd, vd


# ------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_noise_is_the_philox_normal_stream_bit_for_bit(dev, n, offset):
    """p = 0, g = 0, no weight decay, sigma = 1: what is left is xi itself, element i of the array handed in on either path"""
    from bayeslms_amd import ops, _lib as L
    assert L.STREAM_SGMCMC == STREAM
    z = np.zeros(n, np.float32)
    p = _up(z, dev, offset)
    ops.sgmcmc_update(p, _up(z, dev, offset), _sq(dev, 0.0), 0.25, 0.1, 1.0, SEED, STEP)
    want = ops.philox_normal(n, SEED, STREAM, STEP)
    assert torch.equal(p, want), int((p != want).sum())
    assert p.abs().max() > 0 or n == 1


@pytest.mark.parametrize("rule,sigma", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_aligned_and_scalar_paths_give_the_same_bits(dev, n, rule, sigma):
    a, va = _run(dev, n, 0, rule, sigma, clip=0.25)
    b, vb = _run(dev, n, 1, rule, sigma, clip=0.25)
    assert torch.equal(a, b), int((a != b).sum())
    if rule == "psgld":
        assert torch.equal(va, vb), int((va != vb).sum())


@pytest.mark.parametrize("rule", ["sgld", "psgld"])
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_both_rules_match_float64(dev, n, offset, rule):
    p, g, v, sq = _inputs(n)
    norm = math.sqrt(sq) * 0.5
    # the clip active (a tenth of the scaled norm) and inactive (ten times it; a lone zero gradient has norm 0: any clip is inactive)
    for clip in (0.1 * norm if norm > 0 else 0.25, 10.0 * norm if norm > 0 else 0.25):
        for sigma in (0.0, 0.01):
            pd, vd = _run(dev, n, offset, rule, sigma, clip)
            c = R.clip_coefficient(sq, clip, 0.5)[0]
            if norm > 0:
                assert (c < 0.5) == (clip < norm + R.f32(1e-6))
            rp, rv, bp, bv = R.update(p, g, sq, clip, 0.05, 0.5, 1e-3, sigma, _oracle_noise(n), v if rule == "psgld" else None,
                                      alpha=0.9, damping=1e-5, e_xi=R.XI_ORACLE)
            _within(pd, rp, bp, "%s p n=%d offset=%d clip=%.3g sigma=%g" % (rule, n, offset, clip, sigma))
            if rule == "psgld":
                _within(vd, rv, bv, "%s v n=%d offset=%d clip=%.3g" % (rule, n, offset, clip))
                assert (vd >= 0).all()
    if n >= 3 and rule == "psgld":  # the entry with p = g = v = 0: G = 1 / damping, p' = sigma sqrt(G) xi
        want = R.f32(0.01) * math.sqrt(1.0 / R.f32(1e-5)) * float(_oracle_noise(n)[0])
        assert rp[0] == pytest.approx(want, rel=1e-12) and rv[0] == 0.0 and float(vd[0]) == 0.0 and float(pd[0]) != 0.0


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_without_noise_and_decay_sgld_is_clip_sgd_at_momentum_zero(dev, n, offset):
    """Not bit for bit: blm_clip_sgd_multi may contract.  Each of the two is within e of float64, so they are within the bound 2 e
    of each other."""
    from bayeslms_amd import ops
    p, g, _, _ = _inputs(n)
    for clip, gs in ((0.25, 1.0), (1e6, 0.5)):
        p1, p2, gd = _up(p, dev, offset), _up(p, dev, offset), _up(g, dev, offset)
        mom = torch.zeros_like(p2)
        table = ops.PtrTable([p2], [gd], [mom])
        sq = ops.clip_sgd(table, clip, 0.05, 0.0, True, gs)
        ops.sgmcmc_update(p1, gd, sq, clip, 0.05, 0.0, grad_scale=gs)
        rp, _, bp, _ = R.update(p, g, float(sq), clip, 0.05, gs, 0.0, 0.0)
        _within(p1, rp, bp, "sgld against float64 n=%d clip=%g" % (n, clip))
        _within(p2, rp, bp, "clip_sgd against float64 n=%d clip=%g" % (n, clip))
        _within(p1, p2.double().cpu().numpy(), bp, "sgld against clip_sgd n=%d clip=%g" % (n, clip))
        assert n < 3 or not torch.equal(p1, torch.from_numpy(p).to(dev))


@pytest.mark.parametrize("rule", ["sgld", "psgld"])
def test_two_runs_give_the_same_bits_and_another_step_other_noise(dev, rule):
    n = 1027
    a, va = _run(dev, n, 0, rule, 0.01, 0.25)
    b, vb = _run(dev, n, 0, rule, 0.01, 0.25)
    c, vc = _run(dev, n, 0, rule, 0.01, 0.25, step=STEP + 1)
    assert torch.equal(a, b) and not torch.equal(a, c)
    if rule == "psgld":
        assert torch.equal(va, vb) and torch.equal(va, vc)  # the second moment sees no noise
    diff = (c.double() - a.double()).cpu().numpy()
    xi0, xi1 = _oracle_noise(n).astype(np.float64), _oracle_noise(n, STEP + 1).astype(np.float64)
    assert np.corrcoef(diff, xi1 - xi0)[0, 1] > 0.5  # what changed is the noise


def test_ops_refuse_what_the_kernel_cannot_take(dev):
    from bayeslms_amd import ops
    p, g, sq = torch.zeros(8, device=dev), torch.zeros(8, device=dev), torch.zeros(1, device=dev)
    with pytest.raises(ops.BayesLMError, match="g has 7 elements"):
        ops.sgmcmc_update(p, g[:7], sq, 0.25, 0.1, 0.0)
    with pytest.raises(ops.BayesLMError, match="must be contiguous"):
        ops.sgmcmc_update(p[::2], g[::2], sq, 0.25, 0.1, 0.0)
    with pytest.raises(ops.BayesLMError, match="sq must hold 1 float"):
        ops.sgmcmc_update(p, g, torch.zeros(2, device=dev), 0.25, 0.1, 0.0)
    with pytest.raises(ops.BayesLMError, match="lr = -0.1"):
        ops.sgmcmc_update(p, g, sq, 0.25, -0.1, 0.0)
    with pytest.raises(ops.BayesLMError, match="sigma = inf"):
        ops.sgmcmc_update(p, g, sq, 0.25, 0.1, math.inf)
    with pytest.raises(ops.BayesLMError, match="clip = 0.0"):
        ops.sgmcmc_update(p, g, sq, 0.0, 0.1, 0.0)
    with pytest.raises(ops.BayesLMError, match="alpha = 1.0"):
        ops.sgmcmc_update(p, g, sq, 0.25, 0.1, 0.0, v=torch.zeros(8, device=dev), alpha=1.0)
    with pytest.raises(ops.BayesLMError, match="must live on the GPU"):
        ops.sgmcmc_update(p.cpu(), g, sq, 0.25, 0.1, 0.0)


# ------------------------------------------------------------------ through the layers
def _families(dev):
    from bayeslms_amd import model as M
    torch.manual_seed(3)
    return {"lstm": M.RNNModel("LSTM", V, W, W, 2, 0.0, True).to(dev).eval(),
            "transformer": M.TransformerModel(V, W, 2, W, 2, 0.0, "gelu", True).to(dev).eval()}


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


def _trainer(model, sampler=None, lr=0.5):
    from bayeslms_amd import engine
    t = engine.Trainer(copy.deepcopy(model), lr=lr, clip=0.25, momentum=0.0, seed=SEED)
    if sampler is not None:
        t.set_sampler(sampler)
    return t


def _step(trainer, text, k, hidden):
    from bayeslms_amd.model import repackage_hidden
    data, targets = text[k * SEQ:(k + 1) * SEQ], text[k * SEQ + 1:(k + 1) * SEQ + 1].reshape(-1)
    if hasattr(trainer.model, "init_hidden"):
        hidden = trainer.model.init_hidden(COLS) if hidden is None else repackage_hidden(hidden)
    return trainer.step(data, targets, hidden)[2]


N_TOKENS = (ROWS - 1) * COLS


@pytest.mark.parametrize("kind", ["lstm", "transformer"])
def test_three_steps_at_zero_temperature_are_three_plain_steps(dev, families, text, kind, deterministic):
    from bayeslms_amd import sgmcmc
    lr = 0.5
    plain = _trainer(families[kind], lr=lr)
    samp = _trainer(families[kind], sgmcmc.Sampler("sgld", lr, N_TOKENS, temperature=0.0, prior_precision=0.0, seed=SEED), lr=lr)
    assert samp.sampler.weight_decay == 0.0 and samp.sampler.plan(1)[1] == 0.0
    ha = hb = None
    for k in range(3):
        samp.flat.flat_param.copy_(plain.flat.flat_param)  # one step at a time (the module docstring)
        before = plain.flat.flat_param.cpu().numpy().copy()
        ha, hb = _step(plain, text, k, ha), _step(samp, text, k, hb)
        assert torch.equal(plain.flat.flat_grad, samp.flat.flat_grad) and torch.equal(plain.table.sq, samp.table.sq)
        assert plain.step_no == samp.step_no == k + 1 and samp.sampler.k == k + 1
        rp, _, bp, _ = R.update(before, plain.flat.flat_grad.cpu().numpy(), float(plain.table.sq), 0.25, lr, 1.0, 0.0, 0.0)
        _within(samp.flat.flat_param, rp, bp, "%s step %d: the sampler against float64" % (kind, k))
        _within(plain.flat.flat_param, rp, bp, "%s step %d: clip + SGD against float64" % (kind, k))
        _within(samp.flat.flat_param, plain.flat.flat_param.double().cpu().numpy(), bp, "%s step %d: the sampler against clip + SGD" % (kind, k))
        assert np.abs(rp - before).max() > 1e-4  # the step moved the weights
    assert not samp.flat.flat_mom.any()  # sgld keeps no second moment, and momentum is not used while sampling


@pytest.mark.parametrize("kind", ["lstm", "transformer"])
def test_the_noise_of_a_step_is_sigma_xi_of_the_trainers_step_number(dev, families, text, kind, deterministic):
    from bayeslms_amd import ops, sgmcmc
    lr = 0.5
    cold = _trainer(families[kind], sgmcmc.Sampler("sgld", lr, N_TOKENS, temperature=0.0, prior_precision=0.0, seed=SEED))
    warm = _trainer(families[kind], sgmcmc.Sampler("sgld", lr, N_TOKENS, temperature=0.0, prior_precision=0.0, seed=SEED))
    ha, hb = _step(cold, text, 0, None), _step(warm, text, 0, None)
    assert torch.equal(cold.flat.flat_param, warm.flat.flat_param)
    warm.set_sampler(sgmcmc.Sampler("sgld", lr, N_TOKENS, temperature=1.0, prior_precision=0.0, seed=SEED))
    assert warm.step_no == 1
    _step(cold, text, 1, ha), _step(warm, text, 1, hb)
    sigma = warm.sampler.last_sigma
    assert sigma == R.sampler_coefficients(lr, 1.0, 0.0, N_TOKENS)[1] and sigma > 0 and cold.sampler.last_sigma == 0.0
    xi = ops.philox_normal(warm.flat.total, SEED, STREAM, 1).double().cpu().numpy()
    p0, p1 = cold.flat.flat_param.double().cpu().numpy(), warm.flat.flat_param.double().cpu().numpy()
    # p1 = fl(p0 + fl(sigma xi)): the product and the sum, one rounding each
    _within(p1 - p0, sigma * xi, 2 * U * (np.abs(sigma * xi) + np.abs(p1)), "%s: the noise of step 1" % kind)
    other = ops.philox_normal(warm.flat.total, SEED, STREAM, 0).double().cpu().numpy()
    assert np.abs((p1 - p0) - sigma * other).max() > 0.1 * sigma


@pytest.mark.parametrize("rule", ["sgld", "psgld"])
def test_one_seed_one_trajectory(dev, families, text, rule, deterministic):
    from bayeslms_amd import ops, sgmcmc
    runs = []
    for seed in (SEED, SEED, SEED + 1):
        t = _trainer(families["lstm"], sgmcmc.Sampler(rule, 1e-3 if rule == "psgld" else 0.5, N_TOKENS, seed=seed))
        h = None
        for k in range(3):
            h = _step(t, text, k, h)
        runs.append((t.flat.flat_param.clone(), t.flat.flat_mom.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0], runs[2][0])
    assert runs[0][1].any() == (rule == "psgld") and torch.isfinite(runs[0][0]).all()
    # what a sampler cannot take
    from bayeslms_amd import engine, model as M
    torch.manual_seed(0)
    bayes = M.BayesTransformerModel(V, W, 2, W, 2, 0.0, True, "FFN").to(dev)
    with pytest.raises(ops.BayesLMError, match="linear2.weight_lgstd is a variational site"):
        engine.Trainer(bayes, lr=0.5, clip=0.25, seed=SEED).set_sampler(sgmcmc.Sampler("sgld", 0.5, N_TOKENS))
    t = _trainer(families["lstm"])
    t.world = 2
    with pytest.raises(ops.BayesLMError, match="world size 2"):
        t.set_sampler(sgmcmc.Sampler("sgld", 0.5, N_TOKENS))


# ------------------------------------------------------------------ evaluation under a bank
def _zmax(model, text):
    with torch.no_grad():
        if hasattr(model, "init_hidden"):
            out, _ = model(text[:-1], model.init_hidden(text.shape[1]))
        else:
            out = torch.cat([model(text[i:i + SEQ]) for i in range(0, text.shape[0] - 1, SEQ)])
    return float(out.abs().max())


def _e1(zmax):
    """tests/test_gpu_swag.py: one fp32 log-softmax kernel against float64, per token"""
    return U * (28 + 3 * 2 * zmax + 4 * math.log(V) + zmax)


def _eH(zmax):
    """tests/test_gpu_swag.py: one fp32 entropy against float64"""
    D = 2 * zmax
    return U * (28 + 3 * math.log(V) + 57 * D + 4 * D * D)


@pytest.mark.parametrize("kind", ["lstm", "transformer"])
def test_copies_of_the_models_weights_give_its_own_report(dev, families, text, kind, deterministic):
    from bayeslms_amd import engine
    m = families[kind]
    S = 3
    rep = engine.evaluate_samples(m, text, SEQ, _flat_of(m).repeat(S, 1).cpu(), keep_tokens=True)  # a host matrix: moved once
    plain = engine.evaluate_report(m, text, SEQ, keep_tokens=True)
    nll = plain.per_token["nll"].astype(np.float64)
    zmax, logV = _zmax(m, text), math.log(V)
    # S equal samples: two log-softmax kernels (2 e1), S - 1 folds and the subtraction on values of size |nll| + log S
    bound = 2 * (2 * _e1(zmax) + U * ((S - 1) * (4 + nll + math.log(S)) + 2 * math.log(S) + nll))
    _within(rep.per_token["nll"], nll, bound, "%s: per-token NLL under S copies" % kind)
    assert rep.tokens == plain.tokens and rep.mc_samples == S and np.array_equal(rep.per_token["rank"], plain.per_token["rank"])
    for s in range(S):
        _within(rep.per_token["nll_s"][:, s], nll, 2 * 2 * _e1(zmax) + 2 * U * nll, "%s: nll_s under S copies" % kind)
    lp = 2 * zmax + logV + math.log(S)
    e_acc = _e1(zmax) + U * ((S - 1) * (4 + lp) + 2 * math.log(S) + lp)
    mi_bound = 2 * (2 * _eH(zmax) + 2 * U * logV + 2 * logV * e_acc)
    print("%s: worst |mi| %.3e, bound %.3e" % (kind, np.abs(rep.per_token["mi"]).max(), mi_bound))
    assert np.abs(rep.per_token["mi"]).max() <= mi_bound and abs(rep.mean_mi) <= mi_bound
    assert rep.samples is None and rep.swag is None  # the blocks are the caller's to fill


@pytest.mark.parametrize("kind", ["lstm", "transformer"])
def test_two_vectors_are_two_models_and_the_average_is_theirs(dev, families, text, kind, deterministic):
    from bayeslms_amd import engine, sgmcmc, swag
    m = families[kind]
    others = [_families(dev)[kind] for _ in range(2)]
    g = torch.Generator().manual_seed(31)
    for o in others:
        with torch.no_grad():
            for p in o.parameters():
                p.mul_(1 + 0.1 * torch.randn(p.shape, generator=g).to(dev))
    bank = sgmcmc.SampleBank(swag.flat_layout(m)[2], swag.manifest_of(m), 2)
    for o in others:
        bank.add(_flat_of(o), {"kind": "checkpoint"})
    before = _flat_of(m).clone()
    assert torch.equal(bank.to_device(dev), bank.matrix().to(dev)) and torch.equal(bank.to_device(dev, 1), bank.matrix(1).to(dev))
    rep = engine.evaluate_samples(m, text, SEQ, bank, keep_tokens=True)
    assert torch.equal(_flat_of(m), before)
    fresh = []
    for s, o in enumerate(others):
        r = engine.evaluate_report(o, text, SEQ, keep_tokens=True)
        fresh.append(r.per_token["nll"].astype(np.float64))
        e1 = _e1(_zmax(o, text))
        _within(rep.per_token["nll_s"][:, s], fresh[s], 2 * (2 * e1 + U * fresh[s]), "%s: nll_s[%d] against the model with vector %d" % (kind, s, s))
        assert abs(rep.sample_loss[s] - r.loss) <= 4 * e1 + 2 * U * r.loss
    assert np.abs(fresh[0] - fresh[1]).max() > 1e-3
    f, S = np.stack(fresh), 2
    avg = -(np.logaddexp.reduce(-f, 0) - math.log(S))
    bound = 2 * (2 * e1 + U * ((S - 1) * (4 + f.max(0) + math.log(S)) + 2 * math.log(S) + avg))
    _within(rep.per_token["nll"], avg, bound, "%s: NLL of the average against -log mean_s exp(-nll_s)" % kind)
    assert abs(rep.loss - avg.mean()) <= bound.max() and rep.mean_mi > 0 and rep.mean_h_pred > 0


def _posterior(model):
    from bayeslms_amd import swag
    base = _flat_of(model)
    post = swag.SwagPosterior(base.numel(), 3, base.device, swag.manifest_of(model))
    g = torch.Generator(device="cpu").manual_seed(21)
    for _ in range(4):
        post.collect(base * (1 + 0.05 * torch.randn(base.numel(), generator=g).to(base.device)))
    return post


@pytest.mark.parametrize("kind", ["lstm", "transformer"])
def test_evaluate_swag_is_draw_then_evaluate_samples(dev, families, text, kind, deterministic):
    from bayeslms_amd import engine
    m = families[kind]
    post = _posterior(m)
    for kw in (dict(), dict(temperature=2.0)):
        a = engine.evaluate_swag(m, text, SEQ, post, 3, seed=5, scale=0.5, keep_tokens=True, **kw)
        b = engine.evaluate_samples(m, text, SEQ, post.draw(3, 5, 0.5), keep_tokens=True, **kw)
        for k in ("nll", "nll_s", "h_pred", "mi", "conf", "entropy", "rank", "pred", "tgt"):
            assert np.array_equal(a.per_token[k], b.per_token[k]), k
        assert a.as_dict() == b.as_dict()


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


def test_the_model_is_left_as_found_and_the_refusals(dev, families, text, deterministic, monkeypatch):
    from bayeslms_amd import engine, ops, swag
    m = copy.deepcopy(families["lstm"])
    mat = torch.stack([_flat_of(m) * 1.01, _flat_of(m) * 0.99])
    before = engine.evaluate_report(m, text, SEQ, keep_tokens=True).per_token["nll"]
    m.train()
    first = next(m.parameters())
    first.grad = torch.full_like(first, 0.25)
    snap = _snapshot(m)
    engine.evaluate_samples(m, text, SEQ, mat)
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
        engine.evaluate_samples(m, text, SEQ, mat)
    monkeypatch.undo()
    _assert_restored(m, snap)
    assert torch.equal(first.grad, torch.full_like(first, 0.25))
    assert np.array_equal(engine.evaluate_report(m, text, SEQ, keep_tokens=True).per_token["nll"], before)
    snap = _snapshot(m)  # the report left the model in eval mode; a refusal leaves it as it is now
    for rows in (1, 65):
        with pytest.raises(ops.BayesLMError, match="2..64 weight vectors, got %d" % rows):
            engine.evaluate_samples(m, text, SEQ, mat[:1].repeat(rows, 1))
    with pytest.raises(ops.BayesLMError, match=r"\(S, P\) float32 matrix"):
        engine.evaluate_samples(m, text, SEQ, mat.double())
    with pytest.raises(swag.PosteriorMismatch, match="'total'"):
        engine.evaluate_samples(families["transformer"], text, SEQ, mat)
    monkeypatch.setattr(swag, "DRAW_BYTES", 1000)
    with pytest.raises(ops.BayesLMError, match="beyond the budget of 1000 bytes"):
        engine.evaluate_samples(m, text, SEQ, mat)
    _assert_restored(m, snap)


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
REPORT_KEYS = ["accuracy", "bins", "ece", "loss", "mc_samples", "mean_conf", "mean_entropy", "mean_h_pred", "mean_mi", "ppl",
               "sample_loss", "sample_loss_mean", "skipped", "tokens", "top5_accuracy"]  # what a plain run wrote before this flag


def _untimed(log):
    return re.sub(r"ms/batch +[\d.]+|time: +[\d.]+s", "", log)


def test_train_fills_a_bank_and_evaluate_reads_it(dev, tmp_path, capsys, deterministic):
    from bayeslms_amd import evaluate as E, sgmcmc, train as T
    d = _corpus(tmp_path)
    run = ["--data", d, "--cuda", "--epochs", "2", "--seq_len", "8", "--batch-size", "4", "--log-interval", "5", "--seed", "3",
           "--deterministic", "1"]
    pt, plain_pt, bank_pt = os.path.join(d, "model.pt"), os.path.join(d, "plain.pt"), os.path.join(d, "bank.pt")
    T.main(SHAPE + run + ["--save", plain_pt])
    plain_log = capsys.readouterr().out
    assert "sgmcmc" not in plain_log
    T.main(SHAPE + run + ["--save", pt, "--sgmcmc-save", bank_pt, "--sgmcmc-lr", "0.05", "--sgmcmc-start", "2", "--sgmcmc-every", "2",
                          "--sgmcmc-keep", "4"])
    log = capsys.readouterr().out

    def epoch1(text_):
        return [ln for ln in _untimed(text_).splitlines() if re.match(r"\| (end of )?epoch +1 \|", ln)]

    assert epoch1(log) == epoch1(plain_log) and len(epoch1(log)) >= 3  # the burn-in is the run without the flags
    # the configuration printed is the unflagged run's, but for --save
    conf = lambda t: [ln for ln in t.split("Args:")[0].splitlines() if not ln.startswith("save ")]  # noqa: E731
    assert conf(log) == conf(plain_log)
    marks = [ln for ln in log.splitlines() if ln.startswith("| sgmcmc n ")]
    steps = 15  # 60 lines of 8 tokens in 4 columns: 120 rows, windows of 8
    assert [int(ln.split()[3]) for ln in marks] == [1, 2, 3, 4, 4, 4, 4]
    assert [int(re.search(r"step (\d+)", ln).group(1)) for ln in marks] == [steps + 2 * i for i in range(1, 8)]
    n_tokens = 119 * 4
    sigma = R.sampler_coefficients(0.05, 1.0, 1.0, n_tokens)[1]
    assert all(re.search(r"\| epoch +2 \| step \d+ \| lr 0.05 \| sigma %s \|$" % re.escape("%.6g" % sigma), ln) for ln in marks), marks[0]
    assert {m.group(1) for m in re.finditer(r"\| epoch +2 \|.*?\| lr ([\d.]+) \| ms", log)} == {"0.050"}
    assert "sgmcmc: wrote %s (4 samples of 7 seen, sgld)" % bank_pt in log
    bank = sgmcmc.SampleBank.load(bank_pt)
    assert len(bank) == 4 and bank.seen == 7 and bank.capacity == 4 and bank.kind() == "sgld"
    assert [e["step"] for e in bank.meta] == [steps + 2 * i for i in range(4, 8)] and {e["epoch"] for e in bank.meta} == {2}
    assert bank.sampler["n_tokens"] == n_tokens and bank.sampler["lr"] == 0.05 and bank.sampler["temperature"] == 1.0
    mat = bank.matrix()
    assert torch.isfinite(mat).all() and not torch.equal(mat[0], mat[1])
    pad = torch.ones(bank.total, dtype=torch.bool)
    for o, shape in zip(bank.manifest["offsets"], bank.manifest["shapes"]):
        pad[o:o + int(np.prod(shape))] = False
    assert pad.sum() == 0 or not mat[:, pad].any()

    # under a cyclical schedule the epoch lines print the rate the sampler applied, which moves; the collections fall in the
    # sampling share of the cycle
    T.main(SHAPE + run[:3] + ["--epochs", "1"] + run[5:] + ["--save", os.path.join(d, "c.pt"), "--sgmcmc-save", os.path.join(d, "c_bank.pt"),
                              "--sgmcmc-lr", "0.05", "--sgmcmc-cycles", "1", "--sgmcmc-explore", "0.5", "--sgmcmc-every", "1"])
    clog = capsys.readouterr().out
    rates = [float(m.group(1)) for m in re.finditer(r"\| epoch +1 \|.*?\| lr ([\d.]+) \| ms", clog)]
    assert len(rates) == 2 and rates == [round(R.cyclical(k, steps, 1, 0.05, 0.5)[0], 3) for k in (6, 11)] and rates[0] > rates[1]
    cmarks = [int(re.search(r"step (\d+)", ln).group(1)) for ln in clog.splitlines() if ln.startswith("| sgmcmc n ")]
    assert cmarks == [k for k in range(1, steps + 1) if R.cyclical(k, steps, 1, 0.05, 0.5)[1]] == list(range(9, 16))

    # ---- the evaluate command line
    base = ["--model-path", pt, "--vocabulary", os.path.join(d, "words.txt"), "--data", os.path.join(d, "test.txt"),
            "--emsize", "32", "--nhid", "32", "--seq-len", "5", "--batch-size", "2"]
    rj = os.path.join(d, "r.json")
    plain = E.main(base + ["--write-report", rj])
    line0 = capsys.readouterr().out.strip()
    assert "samples kind" not in line0 and sorted(json.load(open(rj))) == REPORT_KEYS and sorted(plain.as_dict()) == REPORT_KEYS
    rep = E.main(base + ["--sample-bank", bank_pt, "--write-report", rj, "--write-tokens", os.path.join(d, "tok.txt")])
    line = capsys.readouterr().out.strip()
    assert re.search(r" \| mc samples 4 \| sample loss [\d.]+ \| h_pred [\d.]+ \| mi [\d.]+ \| samples kind sgld n 4$", line), line
    block = json.load(open(rj))["samples"]
    assert block == dict(bank.describe(), path=bank_pt) and block["n"] == 4 and block["seen"] == 7 and rep.mc_samples == 4
    assert sorted(json.load(open(rj))) == sorted(REPORT_KEYS + ["samples"])
    assert len(open(os.path.join(d, "tok.txt")).readline().split()) == 7  # word nll conf entropy rank h_pred mi
    two = E.main(base + ["--sample-bank", bank_pt, "--bank-samples", "2", "--temperature", "2"])
    assert capsys.readouterr().out.strip().endswith("| temperature 2.0000 | samples kind sgld n 2")
    assert two.mc_samples == 2 and two.samples["meta"] == bank.describe()["meta"][2:] and two.temperature["temperature"] == 2.0
    # an ensemble of the checkpoint and a second member (the same weights, every one a hundredth larger)
    b_pt = os.path.join(d, "b.pt")
    torch.save({k: v * 1.01 if v.dtype.is_floating_point else v for k, v in torch.load(pt, map_location="cpu").items()}, b_pt)
    ens = E.main(base + ["--ensemble", "%s,%s" % (pt, b_pt), "--write-report", rj])
    assert capsys.readouterr().out.strip().endswith("| samples kind checkpoint n 2")
    block = json.load(open(rj))["samples"]
    assert block["kind"] == "checkpoint" and block["n"] == 2 and block["path"] == "%s,%s" % (pt, b_pt) and block["sampler"] is None
    # the members in the order given: each one's own loss lies nearer the plain report of its checkpoint than of the other
    other = E.main(["--model-path", b_pt] + base[2:])
    capsys.readouterr()
    assert ens.mc_samples == 2 and other.loss != plain.loss
    assert abs(ens.sample_loss[0] - plain.loss) < abs(ens.sample_loss[0] - other.loss)
    assert abs(ens.sample_loss[1] - other.loss) < abs(ens.sample_loss[1] - plain.loss)
    after = E.main(base)  # --model-path was a member: the model kept its weights
    capsys.readouterr()
    assert after.loss == plain.loss
    with pytest.raises(SystemExit, match="--bank-samples 5|5 of 4 vectors"):
        E.main(base + ["--sample-bank", bank_pt, "--bank-samples", "5"])
    with pytest.raises(SystemExit, match="--sample-bank .*not a sample bank"):
        E.main(base + ["--sample-bank", pt])
