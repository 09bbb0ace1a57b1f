"""CPU: the last-layer Laplace posterior without a device -- the float64 reference (tests/laplace_reference.py) against autograd
and in its limits, laplace.LaplacePosterior's file format and refusals, the prior selection, and every refusal of evaluate.py and
of the engine's argument checks that needs no GPU."""
import math

import numpy as np
import pytest
import torch

import laplace_reference as R


# ------------------------------------------------------------------ the reference itself
def test_reference_curvature_is_the_diagonal_of_the_autograd_hessian():
    """For V = 5, K = 3 in float64: the diagonal of the Hessian of sum_t logsumexp(W h_t + b) in (W, b) is (F_W, F_b)."""
    V, K, N = 5, 3, 4
    g = torch.Generator().manual_seed(5)
    W = torch.randn(V, K, generator=g, dtype=torch.float64)
    b = torch.randn(V, generator=g, dtype=torch.float64)
    h = torch.randn(N, K, generator=g, dtype=torch.float64)

    def f(W, b):
        return torch.logsumexp(h @ W.t() + b, -1).sum()

    (hww, _), (_, hbb) = torch.autograd.functional.hessian(f, (W, b))
    diag_w = hww.reshape(V * K, V * K).diagonal().reshape(V, K).numpy()
    diag_b = hbb.diagonal().numpy()
    a, _ = R.curvature((h @ W.t() + b).numpy())
    h32 = h.numpy()
    fw, fb = a.T @ h32 ** 2, a.sum(0)  # the formulas of fisher() on the float64 rows themselves
    np.testing.assert_allclose(fw, diag_w, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(fb, diag_b, rtol=1e-12, atol=1e-15)
    # and fisher() itself, from the rows rounded to fp32 as it takes them
    fw32, fb32, bw, bb = R.fisher(a, np.zeros_like(a), h32.astype(np.float32))
    assert np.all(np.abs(fw32 - fw) <= 4 * 2.0 ** -24 * np.abs(fw) + bw) and np.allclose(fb32, fb)


def _example(seed=3, rows=4, V=7):
    rng = np.random.default_rng(seed)
    z = (2 * rng.standard_normal((rows, V))).astype(np.float32)
    var = rng.uniform(0.1, 3.0, (rows, V)).astype(np.float32)
    tgt = rng.integers(0, V, rows)
    return z, var, tgt


def test_zero_variance_makes_every_link_the_softmax():
    z, _, tgt = _example()
    zero = np.zeros_like(z)
    p = R.softmax64(R.f64(z))
    for link in ("probit", "expexp"):
        y, ey = R.link_y(z, zero, link)
        assert np.array_equal(y, R.f64(z))
        st = R.row_stats(y, ey, tgt, zero)
        np.testing.assert_allclose(st["nll"][0], -np.log(p[np.arange(len(tgt)), tgt]), rtol=1e-12)
        assert np.all(st["vbar"][0] == 0)
    eps = np.random.default_rng(1).standard_normal((5,) + z.shape)
    mc = R.mc_rows(z, zero, tgt, eps)
    np.testing.assert_allclose(mc["pbar"][0], p, rtol=1e-12)
    np.testing.assert_allclose(mc["bma_nll"][0], -np.log(p[np.arange(len(tgt)), tgt]), rtol=1e-12)
    assert np.all(np.abs(mc["mi"][0]) <= 1e-15) and np.all(mc["mi"][1] > 0)


def test_expexp_is_shift_invariant_and_probit_is_not():
    z, var, tgt = _example()
    z = (np.round(z * 256) / 256).astype(np.float32)  # multiples of 2^-8 below 16: z + 4 is exact in fp32
    c = np.float32(4.0)
    pe = R.softmax64(R.link_y(z, var, "expexp")[0])
    pe_c = R.softmax64(R.link_y(z + c, var, "expexp")[0])
    np.testing.assert_allclose(pe_c, pe, rtol=1e-12)
    pp = R.softmax64(R.link_y(z, var, "probit")[0])
    pp_c = R.softmax64(R.link_y(z + c, var, "probit")[0])
    assert np.abs(pp_c - pp).max() > 1e-2
    # the Monte-Carlo estimate is invariant too
    eps = np.random.default_rng(2).standard_normal((4,) + z.shape)
    np.testing.assert_allclose(R.mc_rows(z + c, var, tgt, eps)["pbar"][0], R.mc_rows(z, var, tgt, eps)["pbar"][0], rtol=1e-10)


def test_reference_decides_pred_and_rank_by_margin():
    y = np.array([[0.0, 1.0, 1.0 + 1e-9, -1.0]])
    pred, rank, pok, rok = R.decided(y, 1e-8, np.array([0]))
    assert pred[0] == 2 and rank[0] == 2 and not pok[0] and rok[0]
    pred, rank, pok, rok = R.decided(y, 1e-12, np.array([7]))
    assert pok[0] and rank[0] == -1 and not rok[0]


# ------------------------------------------------------------------ LaplacePosterior
class _Model(torch.nn.Module):
    """the least model LaplacePosterior.check takes: one whose decoder is the package's vocabulary projection"""

    def __init__(self, V=6, K=3, seed=0):
        super().__init__()
        from bayeslms_amd import model as M
        self.decoder = M._ProjHolder(K, V)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.decoder.weight.copy_(torch.randn(V, K, generator=g))
            self.decoder.bias.copy_(torch.randn(V, generator=g))


def _Dec(V=6, K=3, seed=0):
    return _Model(V, K, seed)


def _posterior(model):
    from bayeslms_amd import laplace
    dec = model.decoder
    V, K = dec.weight.shape
    post = laplace.LaplacePosterior(V, K, manifest=laplace.manifest_of(dec))
    post.f_w.copy_(torch.rand(V, K))
    post.f_b.copy_(torch.rand(V))
    post._fw[V:] = float("nan")  # the pad rows of the buffers are nobody's: nothing below may look at them
    post._fb[V:] = float("nan")
    post.check_finite()
    post.n_tokens = 17
    return post


def test_posterior_round_trip_inverse_and_describe(tmp_path):
    from bayeslms_amd import laplace
    dec = _Dec()
    post = _posterior(dec)
    path = str(tmp_path / "laplace.pt")
    post.save(path)
    back = laplace.LaplacePosterior.load(path)
    assert torch.equal(back.f_w, post.f_w) and torch.equal(back.f_b, post.f_b) and back.n_tokens == 17
    assert back.manifest == post.manifest and back.f_w.shape == (6, 3) and back._fw.shape == (8, 3)
    back.check(dec)
    s_w, s_b = back.inverse(2.0)
    assert torch.allclose(s_w, 1 / (post.f_w + 2.0)) and torch.allclose(s_b, 1 / (post.f_b + 2.0))
    z_w, z_b = back.inverse(float("inf"))
    assert z_w.shape == (6, 3) and not z_w.any() and not z_b.any()
    for bad in (0.0, -1.0, float("nan"), "x"):
        with pytest.raises(laplace.BayesLMError, match="prior precision"):
            back.inverse(bad)
    d = back.describe()
    assert d["tokens"] == 17 and d["shape"] == [6, 3] and d["fingerprint"] == post.manifest["fingerprint"][:16]
    empty = laplace.LaplacePosterior(6, 3)
    with pytest.raises(laplace.BayesLMError, match="no row accumulated"):
        empty.save(path)


def test_posterior_of_another_decoder_is_refused_by_field(tmp_path):
    from bayeslms_amd import laplace, swag
    dec = _Dec()
    post = _posterior(dec)
    moved = _Dec()
    with torch.no_grad():
        moved.decoder.weight[2, 1] += 1e-3
    with pytest.raises(swag.PosteriorMismatch, match="field 'fingerprint' differs") as e:
        post.check(moved)
    assert e.value.field == "fingerprint" and isinstance(e.value, laplace.LaplaceMismatch)
    biased = _Dec()
    with torch.no_grad():
        biased.decoder.bias[0] += 1.0
    with pytest.raises(laplace.LaplaceMismatch, match="fingerprint"):
        post.check(biased)
    with pytest.raises(laplace.LaplaceMismatch, match=r"field 'shape' differs: the posterior has \[6, 3\], this model has \[6, 4\]"):
        post.check(_Dec(6, 4))
    with pytest.raises(laplace.BayesLMError, match="has no decoder that hands back its input rows"):
        post.check(moved.decoder)  # a model, not its decoder
    # the fingerprint does not depend on the step it is summed in, and every word counts
    dec = _Dec(40, 9, seed=2).decoder
    whole = laplace.fingerprint(dec.weight, dec.bias)
    was = laplace._FP_CHUNK
    try:
        laplace._FP_CHUNK = 7
        assert laplace.fingerprint(dec.weight, dec.bias) == whole
        w2 = dec.weight.detach().clone()
        w2[39, 8] = -w2[39, 8]
        assert laplace.fingerprint(w2, dec.bias) != whole
        w3 = dec.weight.detach().clone()
        w3[[0, 1]] = w3[[1, 0]]  # the same words in another order: the plain sum alone would not see it
        assert laplace.fingerprint(w3, dec.bias) != whole
    finally:
        laplace._FP_CHUNK = was
    path = str(tmp_path / "other.pt")
    st = post.state()
    st["format"] = "bayeslms_amd.swag/1"
    torch.save(st, path)
    with pytest.raises(laplace.BayesLMError, match=r"not a Laplace posterior of this package \(format 'bayeslms_amd.laplace/1' expected"):
        laplace.LaplacePosterior.load(path)
    st = post.state()
    st["f_b"] = st["f_b"][:-1]
    torch.save(st, path)
    with pytest.raises(laplace.BayesLMError, match="f_b is"):
        laplace.LaplacePosterior.load(path)
    st = post.state()
    del st["n_tokens"]
    torch.save(st, path)
    with pytest.raises(laplace.BayesLMError, match="field 'n_tokens' is missing"):
        laplace.LaplacePosterior.load(path)


# ------------------------------------------------------------------ selection
def test_prior_selection_ties_and_the_infinite_candidate():
    from bayeslms_amd import laplace
    inf = float("inf")
    assert laplace.select_prior([inf, 1.0, 10.0], [2.0, 1.5, 1.7]) == 1
    assert laplace.select_prior([inf, 1.0, 10.0], [2.0, 2.0, 2.0]) == 0      # a tie goes to the model itself
    assert laplace.select_prior([inf, 1.0, 10.0], [2.0, 1.5, 1.5]) == 1      # and among finite ones to the first
    assert laplace.select_prior([inf, 1.0], [2.0, float("nan")]) == 0        # a NaN never wins
    assert laplace.select_prior([inf, 1.0], [float("nan"), 3.0]) == 1
    with pytest.raises(laplace.BayesLMError, match="every candidate"):
        laplace.select_prior([inf], [float("nan")])
    with pytest.raises(laplace.BayesLMError, match="candidates"):
        laplace.select_prior([inf, 1.0], [1.0])


# ------------------------------------------------------------------ the engine's argument checks
def test_engine_refuses_before_it_touches_the_model():
    from bayeslms_amd import engine, ops
    model = source = posterior = object()  # never looked at: the arguments are refused first
    for kw, message in ((dict(link="logit"), "link 'logit' is none of"),
                        (dict(link="mc"), "the mc link needs samples"),
                        (dict(link="mc", samples=1), "samples must be 0 or lie in 2..32"),
                        (dict(link="mc", samples=33), "samples must be 0 or lie in 2..32"),
                        (dict(link="probit", samples=4), "samples = 4 with the closed-form link 'probit'"),
                        (dict(link="expexp", samples=2), "closed-form link 'expexp'")):
        with pytest.raises(ops.BayesLMError, match=message):
            engine.evaluate_laplace(model, source, 5, posterior, 1.0, **kw)
        with pytest.raises(ops.BayesLMError, match=message):
            engine.fit_laplace_prior(model, source, 5, posterior, [1.0], **kw)
    for tau in (0.0, -2.0, float("nan"), None):
        with pytest.raises(ops.BayesLMError, match="prior precision"):
            engine.evaluate_laplace(model, source, 5, posterior, tau)
        with pytest.raises(ops.BayesLMError, match="prior precision"):
            engine.fit_laplace_prior(model, source, 5, posterior, [1.0, tau])
    with pytest.raises(ops.BayesLMError, match="9 prior precisions, one walk takes 1..8"):
        engine.fit_laplace_prior(model, source, 5, posterior, [float(i + 1) for i in range(9)])
    with pytest.raises(ops.BayesLMError, match="0 prior precisions"):
        engine.fit_laplace_prior(model, source, 5, posterior, [])
    with pytest.raises(ops.BayesLMError, match="tau = inf is always a candidate"):
        engine.fit_laplace_prior(model, source, 5, posterior, [1.0, float("inf")])
    with pytest.raises(ops.BayesLMError, match="taus must be"):
        engine.fit_laplace_prior(model, source, 5, posterior, 3.0)


def test_engine_refuses_a_model_without_an_inference_decoder_and_another_decoder():
    from bayeslms_amd import engine, laplace, model as M, ops
    with pytest.raises(ops.BayesLMError, match="has no decoder that hands back its input rows"):
        engine.fit_laplace(torch.nn.Linear(3, 3), None, 5)
    m = M.RNNModel("LSTM", 20, 8, 8, 2, 0.0, True)
    post = _posterior(_Dec(20, 8))
    with pytest.raises(laplace.LaplaceMismatch, match="fingerprint"):
        engine.evaluate_laplace(m, None, 5, post, 1.0)
    with pytest.raises(ops.BayesLMError, match="max_windows = 0"):
        engine.fit_laplace(m, None, 5, max_windows=0)
    assert m.training  # nothing ran: the model is as found


def test_ops_refuse_before_any_launch():
    from bayeslms_amd import ops
    x = torch.zeros(2, 5)
    with pytest.raises(ops.BayesLMError, match="must live on the GPU"):
        ops.laplace_curvature(x)
    with pytest.raises(ops.BayesLMError, match="neither 'probit' nor 'expexp'"):
        ops.laplace_row_stats(x, x, link="mc")
    with pytest.raises(ops.BayesLMError, match="samples = 33 outside 1..32"):
        ops.laplace_mc_rows(x, x, 33, 1)
    with pytest.raises(ops.BayesLMError, match="row0 = -1"):
        ops.laplace_mc_rows(x, x, 2, 1, row0=-1)
    with pytest.raises(ops.BayesLMError, match="row-major"):
        ops.laplace_row_stats(x.t(), x.t())


def test_the_c_entry_points_refuse_bad_arguments_without_a_device():
    import ctypes as C
    from bayeslms_amd import _lib as L
    lib = L.lib()
    p = 0x10000
    r = L.rng(1, L.STREAM_LAPLACE, 0)
    assert L.STREAM_LAPLACE == 0x50000000 and L.LAPLACE_SAMPLES_MAX == 32
    assert lib.blm_laplace_curvature(None, 8, p, 8, 1, 8, None) == L.ERR_INVALID
    assert lib.blm_laplace_curvature(p, 7, p + 4096, 8, 1, 8, None) == L.ERR_INVALID       # ld < V
    assert lib.blm_laplace_curvature(p, 8, p, 12, 2, 8, None) == L.ERR_INVALID             # in place with another stride
    assert lib.blm_laplace_curvature(p, 8, p + 16, 8, 2, 8, None) == L.ERR_INVALID and b"overlap" in lib.blm_last_error()
    assert lib.blm_laplace_curvature(p, 8, p, 8, 0, 8, None) == L.OK                       # zero rows: nothing launched
    assert lib.blm_laplace_row_stats(p, 8, p, 8, None, 1, 8, 2, None, p, p, p, None, p, None) == L.ERR_INVALID and b"link 2" in lib.blm_last_error()
    assert lib.blm_laplace_row_stats(p, 8, p, 8, None, 1, 8, 0, p, p, p, p, None, p, None) == L.ERR_INVALID  # nll without targets
    assert lib.blm_laplace_row_stats(p, 8, p, 8, None, 0, 8, 0, None, p, p, p, None, p, None) == L.OK
    for S in (0, 33, -1):
        assert lib.blm_laplace_mc_rows(p, 8, p, 8, None, 1, 8, S, C.byref(r), 0, None, None, p, p, p, p, None, None) == L.ERR_INVALID
    assert lib.blm_laplace_mc_rows(p, 8, p, 8, None, 1, 8, 2, None, 0, None, None, p, p, p, p, None, None) == L.ERR_INVALID
    assert lib.blm_laplace_mc_rows(p, 8, p, 8, None, 1, 8, 2, C.byref(r), -1, None, None, p, p, p, p, None, None) == L.ERR_INVALID
    assert lib.blm_laplace_mc_rows(p, 8, p, 8, None, 1, 8, 2, C.byref(r), 0, p, None, p, p, p, p, None, None) == L.ERR_INVALID  # bma without tgt
    assert lib.blm_laplace_mc_rows(p, 8, p, 8, None, 0, 8, 2, C.byref(r), 0, None, None, p, p, p, p, None, None) == L.OK


# ------------------------------------------------------------------ the command line
BASE = ["--model-path", "m.pt", "--vocabulary", "w.txt", "--data", "t.txt"]
LP = ["--laplace", "l.pt", "--laplace-prior-precision", "10"]


@pytest.mark.parametrize("flags,message", [
    (["--laplace-samples", "4"], "--laplace-samples needs --laplace or --laplace-fit-on"),
    (["--laplace-prior-precision", "1"], "--laplace-prior-precision needs --laplace"),
    (["--laplace-save", "x.pt"], "--laplace-save needs --laplace"),
    (["--laplace-link", "probit"], "--laplace-link needs --laplace"),
    (["--laplace-prior-grid", "1,2"], "--laplace-prior-grid needs --laplace"),
    (["--laplace", "l.pt"], "a Laplace posterior needs its prior"),
    (["--laplace", "l.pt", "--laplace-fit-on", "tr.txt", "--laplace-prior-precision", "1"], "exclude each other: load a posterior or fit one"),
    (["--laplace", "l.pt", "--laplace-prior-precision", "1", "--laplace-save", "x.pt"], "need --laplace-fit-on"),
    (["--laplace-fit-on", "tr.txt", "--laplace-prior-precision", "1", "--laplace-fit-windows", "0"], "at least 1"),
    (["--laplace", "l.pt", "--laplace-prior-precision", "0"], r"must lie in \(0, inf\]"),
    (["--laplace", "l.pt", "--laplace-prior-precision", "nan"], r"must lie in \(0, inf\]"),
    (["--laplace", "l.pt", "--fit-laplace-prior-on", "v.txt"], "go together"),
    (["--laplace", "l.pt", "--laplace-prior-grid", "1,2"], "go together"),
    (["--laplace", "l.pt", "--fit-laplace-prior-on", "v.txt", "--laplace-prior-grid", "1,2", "--laplace-prior-precision", "3"],
     "give tau or the text to pick it on"),
    (["--laplace", "l.pt", "--fit-laplace-prior-on", "v.txt", "--laplace-prior-grid", "1,x"], "numbers separated by commas"),
    (["--laplace", "l.pt", "--fit-laplace-prior-on", "v.txt", "--laplace-prior-grid", "1,inf"], "each positive and finite"),
    (["--laplace", "l.pt", "--fit-laplace-prior-on", "v.txt", "--laplace-prior-grid", "1,2,3,4,5,6,7,8,9"], "needs 1..8 values"),
    (LP + ["--laplace-link", "mc"], "needs --laplace-samples in 2..32"),
    (LP + ["--laplace-link", "mc", "--laplace-samples", "1"], "needs --laplace-samples in 2..32"),
    (LP + ["--laplace-link", "mc", "--laplace-samples", "33"], "needs --laplace-samples in 2..32"),
    (LP + ["--laplace-samples", "4"], "the closed-form links draw no sample"),
    (LP + ["--mc-samples", "4"], "Laplace with --mc-samples: the posterior stands at the mean weights"),
    (LP + ["--swag", "s.pt", "--swag-samples", "2"], "Laplace with --swag: two posteriors"),
    (LP + ["--cache-window", "50", "--cache-theta", "0.3", "--cache-lambda", "0.1"], "Laplace with --cache-window: the cache mixes"),
    (LP + ["--dyneval-lr", "0.1", "--dyneval-decay", "0.01"], "Laplace with dynamic evaluation: the curvature was fitted"),
    (LP + ["--fit-dyneval-on", "v.txt", "--dyneval-lr-grid", "1", "--dyneval-decay-grid", "1"], "Laplace with dynamic evaluation"),
    (LP + ["--fit-temperature-on", "v.txt"], "Laplace with --fit-temperature-on: a temperature on top"),
    (LP + ["--temperature", "1.5"], "Laplace with --temperature 1.5: a temperature on top"),
])
def test_evaluate_refuses_before_anything_is_loaded(flags, message):
    from bayeslms_amd import evaluate as E
    with pytest.raises(SystemExit, match=message):
        E.check_args(E.build_parser().parse_args(BASE + flags))


def test_evaluate_accepts_the_flags_and_the_report_block_is_optional():
    from bayeslms_amd import engine, evaluate as E
    E.check_args(E.build_parser().parse_args(BASE + LP))
    E.check_args(E.build_parser().parse_args(BASE + LP + ["--temperature", "1"]))
    E.check_args(E.build_parser().parse_args(BASE + ["--laplace", "l.pt", "--laplace-prior-precision", "inf", "--laplace-link", "expexp"]))
    E.check_args(E.build_parser().parse_args(BASE + LP + ["--laplace-link", "mc", "--laplace-samples", "8", "--mc-seed", "3"]))
    E.check_args(E.build_parser().parse_args(BASE + ["--laplace-fit-on", "tr.txt", "--laplace-fit-windows", "10", "--laplace-save", "l.pt",
                                                     "--fit-laplace-prior-on", "v.txt", "--laplace-prior-grid", "0.1,1,10"]))
    rep = engine.report_from_tokens([1.0, 2.0], [0.5, 0.6], [1.0, 1.1], [0, 3])
    assert "laplace" not in rep.as_dict()
    line = E.summary_line(rep)
    assert "laplace" not in line
    rep.laplace = {"tokens": 5, "prior_precision": 10.0, "link": "mc", "samples": 4, "shape": [3, 2]}
    assert rep.as_dict()["laplace"]["link"] == "mc"
    assert E.summary_line(rep) == line + " | laplace tokens 5 prior 10 link mc samples 4"
    rep.laplace.update(link="probit", samples=0, prior_precision=math.inf, fitted_on="v.txt", fit_loss_before=2.0, fit_loss_after=1.5,
                       curve=[[math.inf, 2.0], [1.0, 1.5]])
    assert E.summary_line(rep) == line + " | laplace tokens 5 prior inf link probit | fit loss 2.0000 -> 1.5000"
    # what --write-report writes is strict JSON: no Infinity token
    import json
    block = E.laplace_block_json(rep.laplace)
    text = json.dumps(block, allow_nan=False)
    assert json.loads(text)["prior_precision"] == "inf" and json.loads(text)["curve"] == [["inf", 2.0], [1.0, 1.5]]
    assert rep.laplace["prior_precision"] == math.inf  # the report itself keeps the number
