"""GPU: local reparameterisation of the Bayesian linear layers (ops.bayes_linear_lrt, NoiseState.local_reparam) --
y = x mu^T + sqrt(x^2 (sigma^2)^T) * zeta with zeta ~ N(0,1) per (row, column), against the formulas in float64 on the CPU.
Bars: the project's for kernels against the oracle, 1e-4 relative on y and 5e-4 on gradients (of the largest reference value)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(70, 36, 52), (128, 128, 64), (1, 4, 4), (33, 7, 5)]  # (M, N, K); the last takes the scalar loops
SEED, SITE, STEP = 1111, 48, 7


def _dev():
    return torch.device("cuda:0")


def _inputs(M, N, K, seed=0):
    g = torch.Generator().manual_seed(seed + 31 * M + N)
    x = torch.randn(M, K, generator=g)
    mu = 0.3 * torch.randn(N, K, generator=g)
    lg = -1.0 + 0.3 * torch.randn(N, K, generator=g)
    zeta = torch.randn(M, N, generator=g)
    dy = torch.randn(M, N, generator=g)
    return x, mu, lg, zeta, dy


def _ref64(x, mu, lg, zeta, dy, kl_lambda=0.0):
    """float64 autograd of the expression (+ kl_lambda * mean(mu^2 - 2 lg + exp(2 lg)) / 2) -> y, dx, dmu, dlg."""
    x, mu, lg = (t.double().clone().requires_grad_(True) for t in (x, mu, lg))
    y = x @ mu.t() + torch.sqrt((x * x) @ torch.exp(2 * lg).t()) * zeta.double()
    loss = (y * dy.double()).sum() + kl_lambda * (mu * mu - 2 * lg + torch.exp(2 * lg)).mean() / 2
    loss.backward()
    return y.detach(), x.grad, mu.grad, lg.grad


def _run(x, mu, lg, noise, dy, kl_lambda=0.0):
    from bayeslms_amd import ops
    dev = _dev()
    x, mu, lg = (t.to(dev).requires_grad_(True) for t in (x, mu, lg))
    y = ops.bayes_linear_lrt(x, mu, lg, noise, kl_lambda)
    y.backward(dy.to(dev))
    torch.cuda.synchronize()
    return y.detach().cpu(), x.grad.cpu(), mu.grad.cpu(), lg.grad.cpu()


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("kl_lambda", [0.0, 0.37])
def test_forward_and_backward_against_float64(M, N, K, kl_lambda):
    """Tests 1 and 2 of the feature: zeta handed in; y, dx, dmu, dlgstd against float64 autograd of the same expression, the KL
    term's gradient included when kl_lambda is set."""
    from bayeslms_amd import ops
    x, mu, lg, zeta, dy = _inputs(M, N, K)
    got = _run(x, mu, lg, ops.LrtNoise(eps=zeta.to(_dev())), dy, kl_lambda)
    want = _ref64(x, mu, lg, zeta, dy, kl_lambda)
    errs = [_rel(g, w) for g, w in zip(got, want)]
    print("rel err y dx dmu dlg:", errs)
    assert errs[0] <= 1e-4 and max(errs[1:]) <= 5e-4, errs


def test_kl_gradient_equals_what_the_weight_sampling_path_adds():
    """With dy = 0 the data terms vanish and what is left in dmu / dlgstd is the KL gradient alone: the closed form
    kl_lambda * mu / n and kl_lambda * (exp(2 lgstd) - 1) / n, from this path and from the weight-sampling path's epilogue."""
    from bayeslms_amd import ops
    dev = _dev()
    M, N, K = 70, 36, 52
    x, mu, lg, zeta, _ = _inputs(M, N, K)
    lam = 0.37
    eps = torch.randn(N, K, generator=torch.Generator().manual_seed(9)).to(dev)
    want = (lam * mu.double() / (N * K), lam * (torch.exp(2 * lg.double()) - 1) / (N * K))
    for fn in (lambda x_, m_, l_: ops.bayes_linear_lrt(x_, m_, l_, ops.LrtNoise(eps=zeta.to(dev)), lam),
               lambda x_, m_, l_: ops.bayes_linear(x_, m_, l_, ops.NoiseSpec(eps=eps), lam)):
        m_, l_ = mu.to(dev).requires_grad_(True), lg.to(dev).requires_grad_(True)
        fn(x.to(dev), m_, l_).backward(torch.zeros(M, N, device=dev))
        errs = [_rel(m_.grad.cpu(), want[0]), _rel(l_.grad.cpu(), want[1])]
        print("KL gradient rel err:", errs)
        assert max(errs) <= 5e-4, errs


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_philox_path_is_bit_identical_to_the_handed_in_path(M, N, K):
    """zeta drawn with blm_philox_normal on STREAM_LRT + site for (seed, step) and handed in == the kernels' own draw, forward and
    (regenerated) backward; the next step draws something else."""
    from bayeslms_amd import ops, _lib as L
    x, mu, lg, _, dy = _inputs(M, N, K)
    zeta = ops.philox_normal(M * N, SEED, L.STREAM_LRT + SITE, STEP).view(M, N)
    a = _run(x, mu, lg, ops.LrtNoise(eps=zeta), dy, 0.1)
    b = _run(x, mu, lg, ops.LrtNoise(None, SEED, SITE, STEP), dy, 0.1)
    for u, v in zip(a, b):
        assert torch.equal(u, v), float((u - v).abs().max())
    c = _run(x, mu, lg, ops.LrtNoise(None, SEED, SITE, STEP + 1), dy, 0.1)
    assert not torch.equal(a[0], c[0])


def test_degenerate_variance_gives_the_mean_and_finite_gradients():
    from bayeslms_amd import ops
    dev = _dev()
    M, N, K = 70, 36, 52
    x, mu, lg, zeta, dy = _inputs(M, N, K)
    x[5] = 0.0
    lg[11] = float("-inf")
    y, dx, dmu, dlg = _run(x, mu, lg, ops.LrtNoise(eps=zeta.to(dev)), dy)
    m = ops.linear(x.to(dev), mu.to(dev)).cpu()
    assert torch.equal(y[5], m[5]) and torch.equal(y[:, 11], m[:, 11])
    assert not torch.equal(y[6], m[6])
    assert all(bool(torch.isfinite(t).all()) for t in (dx, dmu, dlg))
    assert float(dlg[11].abs().max()) == 0.0 and float((dx[5].double() - (dy[5].double() @ mu.double())).abs().max()) < 1e-4
    # no variance anywhere: the layer IS the mean product
    y0 = _run(x, mu, torch.full_like(lg, float("-inf")), ops.LrtNoise(None, SEED, SITE, STEP), dy)
    assert torch.equal(y0[0], m) and all(bool(torch.isfinite(t).all()) for t in y0)


def test_rows_are_independent_and_columns_follow_the_global_batch():
    from bayeslms_amd import ops
    dev = _dev()
    T, B, K, N = 3, 16, 32, 8
    g = torch.Generator().manual_seed(4)
    x = torch.randn(T, B, K, generator=g)
    x[1, 3] = x[1, 2]
    mu, lg = 0.3 * torch.randn(N, K, generator=g), -1.0 + 0.3 * torch.randn(N, K, generator=g)
    full = ops.bayes_linear_lrt(x.to(dev), mu.to(dev), lg.to(dev), ops.LrtNoise(None, SEED, SITE, STEP)).cpu()
    assert not torch.equal(full[1, 3], full[1, 2])  # identical rows, noise of their own
    w = ops.bayes_linear(x.to(dev), mu.to(dev), lg.to(dev), ops.NoiseSpec(None, SEED, SITE, STEP)).cpu()
    assert torch.equal(w[1, 3], w[1, 2])  # the weight-sampling estimator shares one draw over the batch
    part = ops.bayes_linear_lrt(x[:, 8:].contiguous().to(dev), mu.to(dev), lg.to(dev),
                                ops.LrtNoise(None, SEED, SITE, STEP, col_offset=8, global_cols=16)).cpu()
    assert torch.equal(part, full[:, 8:])
    # and so do the gradients (zeta regenerated with the same key)
    dy = torch.randn(T, B, N, generator=g)
    grads = []
    for xs, ds, nz in ((x, dy, ops.LrtNoise(None, SEED, SITE, STEP)),
                       (x[:, 8:].contiguous(), dy[:, 8:].contiguous(), ops.LrtNoise(None, SEED, SITE, STEP, 8, 16))):
        xd = xs.to(dev).requires_grad_(True)
        ops.bayes_linear_lrt(xd, mu.to(dev), lg.to(dev), nz).backward(ds.to(dev))
        grads.append(xd.grad.cpu())
    assert torch.equal(grads[1], grads[0][:, 8:])


MOM = dict(M=4096, K=32, N=8, seed=2024, site=5, step=3)


def _moment_bounds(zeta, mean, var):
    """6 standard errors: of the sample mean, sqrt(var / M); of the sample variance of a normal, var * sqrt(2 / (M - 1))."""
    M = zeta.shape[0]
    y = mean + np.sqrt(var) * zeta
    return (np.abs(y.mean(0) - mean) <= 6 * np.sqrt(var / M)).all() and (np.abs(y.var(0, ddof=1) - var) <= 6 * var * np.sqrt(2.0 / (M - 1))).all()


def test_moments_of_identical_rows():
    from oracle import philox as P
    from bayeslms_amd import ops, _lib as L
    M, K, N = MOM["M"], MOM["K"], MOM["N"]
    g = torch.Generator().manual_seed(6)
    x1, mu, lg = torch.randn(K, generator=g), 0.3 * torch.randn(N, K, generator=g), -1.0 + 0.3 * torch.randn(N, K, generator=g)
    mean = (mu.double() @ x1.double()).numpy()
    var = (torch.exp(2 * lg.double()) @ (x1.double() ** 2)).numpy()
    # the condition first, in float64 on the CPU with the same zeta stream: the chosen seed passes it
    zeta = P.normal(M * N, MOM["seed"], L.STREAM_LRT + MOM["site"], MOM["step"]).astype(np.float64).reshape(M, N)
    assert _moment_bounds(zeta, mean, var)
    dev = _dev()
    y = ops.bayes_linear_lrt(x1.expand(M, K).contiguous().to(dev), mu.to(dev), lg.to(dev),
                             ops.LrtNoise(None, MOM["seed"], MOM["site"], MOM["step"])).double().cpu().numpy()
    se_m, se_v = np.sqrt(var / M), var * np.sqrt(2.0 / (M - 1))
    print("mean dev / se:", np.abs(y.mean(0) - mean) / se_m, "var dev / se:", np.abs(y.var(0, ddof=1) - var) / se_v)
    assert (np.abs(y.mean(0) - mean) <= 6 * se_m).all() and (np.abs(y.var(0, ddof=1) - var) <= 6 * se_v).all()


# ---------------------------------------------------------------------------------------------------------------- model level
V, D_, FF, T_, B_ = 101, 64, 128, 16, 4


@pytest.fixture()
def det():
    from bayeslms_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(was)


def _model(dropout=0.2):
    from bayeslms_amd import model as Mo
    torch.manual_seed(5)
    return Mo.BayesTransformerModel(V, D_, 4, FF, 2, dropout, True, "FFN").to(_dev())


def _one_step(m):
    from bayeslms_amd import ops
    g = torch.Generator().manual_seed(2)
    src, tgt = torch.randint(0, V, (T_, B_), generator=g).to(_dev()), torch.randint(0, V, (T_ * B_,), generator=g).to(_dev())
    m.train()
    m.set_step(3)
    loss, _ = ops.cross_entropy(m(src).view(-1, V), tgt)
    loss.backward()
    torch.cuda.synchronize()
    return [loss.detach().cpu()] + [p.grad.cpu().clone() for p in m.parameters()]


def test_flag_off_is_bit_identical_to_a_model_that_never_had_it(det):
    """Deterministic mode, so that two runs of ONE path are bit-identical and a difference can only come from the flag."""
    a, b = _model(), _model()
    a.set_local_reparam(True)
    on = _one_step(a)
    a.zero_grad()
    a.set_local_reparam(False)
    assert "local_reparam" in vars(a.noise_state) and "local_reparam" not in vars(b.noise_state)
    off, never = _one_step(a), _one_step(b)
    for u, v in zip(off, never):
        assert torch.equal(u, v)
    assert not all(torch.equal(u, v) for u, v in zip(on, never))  # and the flag does change the step


def _train20(seed=1111):
    from bayeslms_amd import data as D, engine
    m = _model()
    m.set_local_reparam(True)
    kl = lambda mm: mm.transformerlayers[0].linear2.kl_divergence()  # noqa: E731
    kl.fusable = True
    stream = torch.randint(0, V, (B_ * (20 * T_ + 1) + 5,), generator=torch.Generator().manual_seed(1))
    train = D.batchify(stream, B_, _dev())
    tr = engine.Trainer(m, lr=0.5, clip=0.5, kl_scale=float(T_) / train.size(0), seed=seed, bucket_bytes=1 << 20)
    losses = []
    for i in range(20):
        data, tgt = D.get_batch(train, 0, T_)  # one batch, seen 20 times with fresh noise: the loss has to fall
        losses.append(tr.step(data, tgt, kl_fn=kl)[0])
    return [float(v) for v in torch.stack(losses).cpu()], tr.flat.flat_param.detach().cpu().clone()


def test_flagged_model_trains_and_is_deterministic_run_to_run(det):
    l1, p1 = _train20()
    l2, p2 = _train20()
    print("losses:", l1)
    assert all(np.isfinite(l1)) and sum(l1[-5:]) / 5 < sum(l1[:5]) / 5
    assert l1 == l2 and torch.equal(p1, p2)


def _refused_models():
    from bayeslms_amd import model as Mo
    return [("MHA", lambda: Mo.BayesTransformerModel(V, D_, 4, FF, 2, 0.2, True, "MHA")),
            ("EMB", lambda: Mo.BayesTransformerModel(V, D_, 4, FF, 2, 0.2, False, "EMB")),
            ("LSTM", lambda: Mo.BayesRNNModel("LSTM", V, 64, 64, 2, 0.2, True, 3)),
            ("GP", lambda: Mo.GaussTransformerModel(V, D_, 4, FF, 2, 0.2, True, 3)),
            ("GP", lambda: Mo.GaussRNNModel("LSTM", V, 64, 64, 2, 0.2, True, "33")),
            ("Variational", lambda: Mo.VariationalRNNModel("LSTM", V, 64, 64, 2, 0.2, True, "11"))]


@pytest.mark.parametrize("i", range(6))
def test_sites_without_the_path_refuse_the_flag(i):
    from bayeslms_amd import BayesLMError
    site, make = _refused_models()[i]
    torch.manual_seed(5)
    m = make().to(_dev())
    m.set_local_reparam(True)
    m.train()
    src = torch.randint(0, V, (T_, B_), device=_dev())
    with pytest.raises(BayesLMError, match=r"local_reparam.*\b%s\b" % site):
        m(src, m.init_hidden(B_)) if hasattr(m, "init_hidden") else m(src)


def test_monte_carlo_sampling_refuses_a_flagged_model():
    from bayeslms_amd import BayesLMError, model as Mo
    from bayeslms_amd.incremental import IncrementalLM
    m = _model().eval()
    m.set_local_reparam(True)
    with pytest.raises(BayesLMError, match="local_reparam"):
        with Mo.mc_sampling(m, 1, 2):
            pass
    with pytest.raises(BayesLMError, match="local_reparam"):
        IncrementalLM(m, mc_samples=2)
    m.set_local_reparam(False)
    with Mo.mc_sampling(m, 1, 2):
        pass
