"""CPU: the neural cache's host side -- the float64 reference's own properties, CacheSearch, the lambda bisection, every
refusal of blm_cache_scores through ctypes (all before any launch) and the evaluate command's flag refusals."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import cache_reference as R


@pytest.fixture(scope="module")
def L():
    from bayeslms_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _tiny(n=23, K=5, V=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, K, generator=g, dtype=torch.float64), torch.randint(0, V, (n,), generator=g)


# ------------------------------------------------------------------ the reference's own properties
@pytest.mark.parametrize("window", [1, 3, 50])
@pytest.mark.parametrize("theta", [0.0, 0.7])
def test_reference_cache_distribution_sums_to_one(window, theta):
    V = 4
    h, y = _tiny(V=V)
    for t in range(h.shape[0]):
        total = 0.0
        for w in range(V):  # the target looped over every word: exp(match - lse) is p_cache(w)
            tgt = y.clone()
            tgt[t] = w
            lse, match = R.cache_scores(h, h, y, tgt, torch.arange(h.shape[0]), [theta], window)
            total += 0.0 if match[0, t] == -math.inf else math.exp(float(match[0, t] - lse[0, t]))
        dist = R.cache_distribution(h, y, V, t, theta, window)
        if t == 0:
            assert total == 0.0 and float(dist.sum()) == 0.0  # an empty cache
        else:
            assert abs(total - 1.0) <= 1e-12 and abs(float(dist.sum()) - 1.0) <= 1e-12


def test_reference_theta_zero_counts_matches():
    h, y = _tiny(n=40, V=3)
    window = 7
    lse, match = R.text_scores(h, y, [0.0], window)
    for t in range(40):
        a = max(0, t - window)
        size, hits = t - a, int((y[a:t] == y[t]).sum())
        assert (lse[0, t] == -math.inf) if size == 0 else abs(float(lse[0, t]) - math.log(size)) <= 1e-12
        assert (match[0, t] == -math.inf) if hits == 0 else abs(math.exp(float(match[0, t] - lse[0, t])) - hits / size) <= 1e-12


def test_reference_mixed_distribution_sums_to_one():
    V, window, theta, lam = 4, 6, 0.5, 0.3
    h, y = _tiny(V=V, seed=3)
    g = torch.Generator().manual_seed(9)
    logp = torch.log_softmax(torch.randn(h.shape[0], V, generator=g, dtype=torch.float64), -1)
    for t in (0, 1, 5, 22):
        total = 0.0
        for w in range(V):
            tgt = y.clone()
            tgt[t] = w
            lse, match = R.cache_scores(h, h, y, tgt, torch.arange(h.shape[0]), [theta], window)
            total += math.exp(-float(R.cache_mix(-logp[:, w], lse[0], match[0], lam)[t]))
        assert abs(total - 1.0) <= 1e-12


def test_ops_cache_mix_is_the_reference_and_lambda_zero_is_the_model():
    from bayeslms_amd import ops
    h, y = _tiny(n=60, V=3, seed=5)
    lse, match = R.text_scores(h, y, [0.4], 9)
    nll = torch.rand(60, dtype=torch.float64) * 5
    assert ops.cache_mix(nll, lse[0], match[0], 0.0) is nll
    for lam in (1e-3, 0.25, 0.9):
        got, want = ops.cache_mix(nll, lse[0], match[0], lam), R.cache_mix(nll, lse[0], match[0], lam)
        assert torch.isfinite(got).all() and float((got - want).abs().max()) <= 1e-12
        assert got[0] == nll[0]  # the empty cache
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ops.BayesLMError):
            ops.cache_mix(nll, lse[0], match[0], bad)


# ------------------------------------------------------------------ CacheSearch
def test_cache_search_finds_the_minimum_of_a_known_curve():
    from bayeslms_amd import engine
    for t_star in (3e-3, 0.08, 1.7):
        s = engine.CacheSearch()
        for _ in range(3):
            g = s.grid()
            assert 3 <= len(g) <= 8 and g == sorted(g) and all(float(np.float32(v)) == v for v in g)
            s.update(g, [(math.log(t) - math.log(t_star)) ** 2 + 2.0 for t in g])
        a, b = s.bracket
        assert a <= t_star <= b and not s.at_bound
        assert abs(math.log(s.result() / t_star)) <= math.log(1.6e5) * (2.0 / 7) ** 2 / 7 + 1e-6  # one step of the last grid


def test_cache_search_reports_a_bound_and_refuses_bad_domains():
    from bayeslms_amd import engine, ops
    up, down = engine.CacheSearch(), engine.CacheSearch()
    for _ in range(2):
        g = up.grid()
        up.update(g, [-t for t in g])   # still falling at hi
        g = down.grid()
        down.update(g, [t for t in g])  # still falling towards lo
    assert up.at_bound and up.result() == up.hi == 16.0
    assert down.at_bound and down.result() == down.lo == float(np.float32(1e-4))
    for lo, hi, points in ((0.0, 1.0, 8), (-1.0, 1.0, 8), (2.0, 1.0, 8), (1.0, 1.0, 8), (1e-3, math.inf, 8), (1e-3, 1.0, 2), (1e-3, 1.0, 9)):
        with pytest.raises(ops.BayesLMError):
            engine.CacheSearch(lo, hi, points)
    with pytest.raises(ops.BayesLMError):
        engine.CacheSearch().result()
    with pytest.raises(ops.BayesLMError):
        engine.CacheSearch().update([0.1], [float("nan")])


# ------------------------------------------------------------------ lambda
def test_best_lambda_against_a_brute_force_grid():
    from bayeslms_amd import engine
    h, y = _tiny(n=400, K=6, V=5, seed=11)
    h[200:] = h[:200] + 0.05 * h[200:]  # the second half repeats the first: the cache helps
    y[200:] = y[:200]
    thetas = [0.0, 0.5, 2.0]
    lse, match = R.text_scores(h, y, thetas, 250)
    nll = torch.rand(400, dtype=torch.float64) * 3 + 0.5
    valid = torch.ones(400, dtype=torch.bool)
    valid[17] = False
    nll[17] = float("nan")  # a skipped token
    lam, loss = engine.cache_best_lambda(nll, lse, match, valid, lam_max=0.95)
    grid = np.linspace(0.0, 0.95, 1901)
    for j in range(3):
        brute = [float(R.cache_mix(nll, lse[j], match[j], float(l))[valid].mean()) for l in grid]
        k = int(np.argmin(brute))
        assert abs(float(lam[j]) - grid[k]) <= grid[1] and float(loss[j]) <= brute[k] + 1e-12
        assert abs(float(loss[j]) - float(R.cache_mix(nll, lse[j], match[j], float(lam[j]))[valid].mean())) <= 1e-12
    assert float(lam.max()) > 0.0
    # a cache that never matches: lambda 0 and the model's loss; one that is always right: the upper bound
    never = torch.full_like(match, -math.inf)
    lam, loss = engine.cache_best_lambda(nll, lse, never, valid)
    assert lam.tolist() == [0.0] * 3 and float((loss - nll[valid].mean()).abs().max()) <= 1e-12
    lam, _ = engine.cache_best_lambda(nll, lse, lse.clone(), valid, lam_max=0.9)
    assert lam.tolist() == [0.9] * 3


# ------------------------------------------------------------------ the C ABI's refusals
def _args(L, **over):
    """A call blm_cache_scores accepts up to the launch (M = 0: BLM_OK, nothing launched), with ``over`` applied."""
    th = L.CacheThetas()
    th.abi_version, th.count = L.ABI_VERSION, 2
    th.theta[0], th.theta[1] = 0.0, 0.5
    a = dict(q=0x1000, ldq=8, k=0x2000, ldk=8, label=0x3000, tgt=0x4000, lo=None, hi=0x5000, window=4, M=0, Nk=16, K=8, thetas=th,
             lse=0x6000, match=0x7000, ws=None, stream=None)
    a.update(over)
    return a


def _call(L, a):
    return L.lib().blm_cache_scores(a["q"], a["ldq"], a["k"], a["ldk"], a["label"], a["tgt"], a["lo"], a["hi"], a["window"], a["M"],
                                    a["Nk"], a["K"], C.byref(a["thetas"]) if a["thetas"] is not None else None, a["lse"], a["match"],
                                    a["ws"], a["stream"])


def test_cabi_declares_binds_and_exports_the_entry(L):
    res, args = L.SIGNATURES["blm_cache_scores"]
    assert res is C.c_int and len(args) == 17 and args[12] is C.POINTER(L.CacheThetas)
    assert "blm_cache_scores" not in L.VALUE_RETURNING and L.calls().blm_cache_scores.errcheck is not None
    assert C.sizeof(L.CacheThetas) == 8 + 4 * L.CACHE_THETAS_MAX and L.CACHE_THETAS_MAX == 8


def test_cabi_refusals_reach_no_launch(L):
    # the pointers are made-up device addresses: a call that got as far as a launch would not return these statuses, and the
    # accepted call below has M = 0, which by contract launches nothing
    assert _call(L, _args(L)) == L.OK
    assert _call(L, _args(L, lo=0x8000, ws=0x9000)) == L.OK
    bad = []
    for name in ("q", "k", "label", "tgt", "hi", "thetas", "lse", "match"):
        bad.append((name + " NULL", _args(L, **{name: None}), L.ERR_INVALID))
    for name, v in (("M", -1), ("Nk", -1), ("K", 0), ("K", -3), ("window", 0), ("window", -5), ("ldq", 7), ("ldk", 7)):
        bad.append(("%s = %d" % (name, v), _args(L, **{name: v}), L.ERR_INVALID))
    for count in (0, -1, 9):
        a = _args(L)
        a["thetas"].count = count
        bad.append(("count %d" % count, a, L.ERR_INVALID))
    for theta in (-1e-3, float("nan"), float("inf")):
        a = _args(L)
        a["thetas"].theta[1] = theta
        bad.append(("theta %r" % theta, a, L.ERR_INVALID))
    # extents whose byte offsets overflow
    bad.append(("huge ldq", _args(L, M=2 ** 30, ldq=2 ** 40), L.ERR_INVALID))
    bad.append(("huge ldk", _args(L, Nk=2 ** 30, ldk=2 ** 40), L.ERR_INVALID))
    bad.append(("M beyond 2^30", _args(L, M=2 ** 31 - 1), L.ERR_INVALID))
    a = _args(L)
    a["thetas"].abi_version = L.ABI_VERSION + 1
    bad.append(("abi", a, L.ERR_ABI))
    for what, a, status in bad:
        a["M"] = a["M"] or 64  # work to launch, were the call accepted
        assert _call(L, a) == status, what
        assert b"blm_cache_scores" in L.lib().blm_last_error(), what
    # a theta beyond the count is not read
    a = _args(L)
    a["thetas"].theta[5] = float("nan")
    assert _call(L, a) == L.OK
    with pytest.raises(L.BayesLMError) as e:
        L.calls().blm_cache_scores(None, 8, None, 8, None, None, None, None, 4, 8, 8, 8, None, None, None, None, None)
    assert e.value.status == L.ERR_INVALID


def test_ops_cache_thetas_rounds_once_and_refuses():
    from bayeslms_amd import ops
    t = ops.cache_thetas([0, 0.1, 3])
    assert t.count == 3 and t.theta[1] == float(np.float32(0.1)) and t.theta[0] == 0.0
    for bad in ([], [0.1] * 9, [-0.5], [float("nan")], [float("inf")], [1e39], ["x"], None):
        with pytest.raises(ops.BayesLMError):
            ops.cache_thetas(bad)


# ------------------------------------------------------------------ engine and command line: refused before anything is touched
def test_engine_refusals_come_before_the_model_is_used():
    from bayeslms_amd import engine, ops

    class Untouchable:  # any use of the model or the text raises AttributeError, not BayesLMError
        pass

    for kw, word in ((dict(mc_samples=4), "mc_samples"), (dict(temperature=2.0), "temperature"), (dict(window=0), "window")):
        args = dict(window=10)
        args.update(kw)
        window = args.pop("window")
        with pytest.raises(ops.BayesLMError, match=word):
            engine.evaluate_cache(Untouchable(), Untouchable(), 35, window, 0.1, 0.1, **args)
        with pytest.raises(ops.BayesLMError, match=word):
            engine.fit_cache(Untouchable(), Untouchable(), 35, window, **args)
    with pytest.raises(ops.BayesLMError, match="theta"):
        engine.evaluate_cache(Untouchable(), Untouchable(), 35, 10, -1.0, 0.1)
    with pytest.raises(ops.BayesLMError, match="lam"):
        engine.evaluate_cache(Untouchable(), Untouchable(), 35, 10, 0.1, 1.0)
    with pytest.raises(ops.BayesLMError, match="passes"):
        engine.fit_cache(Untouchable(), Untouchable(), 35, 10, passes=0)


def test_engine_refuses_a_text_beyond_the_row_budget_by_size():
    from bayeslms_amd import engine, model as M, ops
    m = M.RNNModel("LSTM", 50, 1024, 1024, 2, 0.5, True)  # K = 1024: 2^21 + 1 rows pass 8 GiB

    class Source:  # only its shape is read before the refusal
        shape = (2 ** 21 + 2, 1)
    with pytest.raises(ops.BayesLMError, match=r"8\.00 GiB.*beyond the 8 GiB"):
        engine.evaluate_cache(m, Source(), 35, 100, 0.1, 0.1)


def test_cache_report_dict_and_eval_report_without_a_cache():
    from bayeslms_amd import engine
    rep = engine.report_from_tokens([1.0, 2.0])
    assert "cache" not in rep.as_dict() and "temperature" not in rep.as_dict()
    rep.cache = {"window": 5}
    assert rep.as_dict()["cache"] == {"window": 5}
    c = engine.CacheReport(2, 0, 1.0, math.e, 1.5, math.exp(1.5), 5, 0.25, 0.1, 0.5, 0.2, per_token={"nll": np.zeros(2)})
    assert sorted(c.as_dict()) == ["base_loss", "base_ppl", "cache_hit_rate", "lam", "loss", "mean_cache_prob", "ppl", "skipped", "theta",
                                   "tokens", "window"]


@pytest.mark.parametrize("flags,word", [
    (["--cache-theta", "0.1", "--cache-lambda", "0.1"], "need --cache-window"),
    (["--fit-cache-on", "valid.txt"], "need --cache-window"),
    (["--cache-window", "0", "--cache-theta", "0.1", "--cache-lambda", "0.1"], "at least 1"),
    (["--cache-window", "100", "--cache-theta", "0.1", "--cache-lambda", "0.1", "--mc-samples", "4"], "--mc-samples"),
    (["--cache-window", "100", "--cache-theta", "0.1", "--cache-lambda", "0.1", "--temperature", "2"], "--temperature"),
    (["--cache-window", "100", "--cache-theta", "0.1", "--cache-lambda", "0.1", "--fit-temperature-on", "v.txt"], "--fit-temperature-on"),
    (["--cache-window", "100", "--cache-theta", "0.1"], "--cache-theta together with --cache-lambda"),
    (["--cache-window", "100", "--cache-lambda", "0.1"], "--cache-theta together with --cache-lambda"),
    (["--cache-window", "100"], "or --fit-cache-on"),
    (["--cache-window", "100", "--fit-cache-on", "v.txt", "--cache-theta", "0.1", "--cache-lambda", "0.1"], "exclude each other"),
    (["--cache-window", "100", "--fit-cache-on", "v.txt", "--cache-lambda", "0.1"], "exclude each other"),
    (["--cache-window", "100", "--cache-theta", "-1", "--cache-lambda", "0.1"], "--cache-theta must be"),
    (["--cache-window", "100", "--cache-theta", "0.1", "--cache-lambda", "1"], "--cache-lambda must lie"),
    (["--cache-window", "100", "--fit-cache-on", "v.txt", "--cache-fit-passes", "0"], "--cache-fit-passes"),
])
def test_cli_refuses_conflicting_flags_before_any_file_is_opened(flags, word, tmp_path):
    from bayeslms_amd import evaluate as E
    missing = str(tmp_path / "does_not_exist")  # opening any of them would raise FileNotFoundError, not SystemExit
    with pytest.raises(SystemExit) as e:
        E.main(["--model-path", missing, "--vocabulary", missing, "--data", missing] + flags)
    assert word in str(e.value)
