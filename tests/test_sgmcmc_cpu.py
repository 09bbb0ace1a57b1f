"""CPU: the host side of SG-MCMC sampling, sample banks and ensembles (bayeslms_amd/sgmcmc.py), the refusals of the two command
lines, raised before a device is touched, and the argument checks of blm_sgmcmc_update, which come before any launch."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import sgmcmc_reference as R

V, W = 50, 32


def _lstm(seed=3):
    from bayeslms_amd import model as M
    torch.manual_seed(seed)
    return M.RNNModel("LSTM", V, W, W, 2, 0.0, True)


def _transformer(seed=3):
    from bayeslms_amd import model as M
    torch.manual_seed(seed)
    return M.TransformerModel(V, W, 2, W, 2, 0.0, "gelu", True)


# ------------------------------------------------------------------ schedule and scaling
def test_cyclical_schedule_at_cycle_ends_and_the_explore_boundary():
    from bayeslms_amd import sgmcmc
    from bayeslms_amd._lib import BayesLMError
    K, M, lr0 = 100, 4, 0.5
    s = sgmcmc.CyclicalSchedule(K, M, lr0, 0.8)
    assert s.length == 25
    for k in (1, 26, 51, 76):  # each cycle starts at the full rate, exploring
        assert s.r(k) == 0.0 and s.rate(k) == lr0 and not s.sampling(k)
    for k in (25, 50, 75, 100):  # and ends one step short of zero, sampling
        assert s.r(k) == 24 / 25 and s.sampling(k)
        assert s.rate(k) == pytest.approx(lr0 / 2 * (math.cos(math.pi * 24 / 25) + 1), rel=1e-15) and 0 < s.rate(k) < 0.01 * lr0
    assert not s.sampling(20) and s.sampling(21)  # r = 19/25 < 0.8 <= 20/25
    assert [s.sampling(k) for k in range(1, 26)].count(True) == 5
    for k in range(1, K + 1):
        rate, sampling = R.cyclical(k, K, M, lr0, 0.8)
        assert s.rate(k) == pytest.approx(rate, rel=1e-15) and s.sampling(k) == sampling
    # K no multiple of M: L = ceil(K / M), the last cycle is cut short
    odd = sgmcmc.CyclicalSchedule(10, 3, 1.0, 0.5)
    assert odd.length == 4 and [odd.sampling(k) for k in range(1, 11)] == [False, False, True, True] * 2 + [False, False]
    assert odd.rate(3) == pytest.approx(0.5, rel=1e-15)
    # no cycles: a constant rate with noise throughout
    flat = sgmcmc.CyclicalSchedule(7, 0, 0.25)
    assert all(flat.rate(k) == 0.25 and flat.sampling(k) for k in range(1, 8))
    for bad in (dict(total_steps=0, cycles=0, lr0=1.0), dict(total_steps=5, cycles=6, lr0=1.0), dict(total_steps=5, cycles=1, lr0=0.0),
                dict(total_steps=5, cycles=1, lr0=1.0, explore=1.0)):
        with pytest.raises(BayesLMError, match="CyclicalSchedule"):
            sgmcmc.CyclicalSchedule(**bad)
    with pytest.raises(BayesLMError, match="count from 1"):
        s.rate(0)


def test_sigma_and_weight_decay_from_the_rate_temperature_prior_and_tokens():
    from bayeslms_amd import sgmcmc
    from bayeslms_amd._lib import BayesLMError
    lr, T, tau, N = 0.37, 0.5, 3.0, 123457
    s = sgmcmc.Sampler("sgld", lr, N, T, tau)
    wd, sigma = R.sampler_coefficients(lr, T, tau, N)
    assert s.weight_decay == wd == tau / N
    assert s.sigma(lr) == sigma == float(np.float32(math.sqrt(2 * lr * T / N)))
    assert s.plan(1) == (lr, sigma, True)
    # eps = 2 lr / N is the Langevin step on U = N mean NLL + tau / 2 |theta|^2: noise variance eps T, drift eps / 2 grad U
    eps = 2 * lr / N
    assert sigma ** 2 == pytest.approx(eps * T, rel=2e-7) and eps / 2 * tau == pytest.approx(lr * wd, rel=1e-15)
    assert sgmcmc.Sampler("sgld", lr, N, 0.0, 0.0).plan(1) == (lr, 0.0, True)  # T = 0, tau = 0: plain SGD at momentum 0
    cyc = sgmcmc.Sampler("psgld", lr, N, T, tau, schedule=sgmcmc.CyclicalSchedule(10, 2, 0.2, 0.6))
    assert cyc.plan(1) == (0.2, 0.0, False)  # exploring: no noise
    rate = R.cyclical(4, 10, 2, 0.2, 0.6)[0]
    assert cyc.plan(4) == (pytest.approx(rate, rel=1e-15), R.sampler_coefficients(cyc.plan(4)[0], T, tau, N)[1], True)
    assert cyc.settings()["schedule"] == {"total_steps": 10, "cycles": 2, "lr0": 0.2, "explore": 0.6} and cyc.settings()["rule"] == "psgld"
    for bad in (dict(rule="sghmc", lr=1.0, n_tokens=1), dict(rule="sgld", lr=0.0, n_tokens=1), dict(rule="sgld", lr=1.0, n_tokens=0),
                dict(rule="sgld", lr=1.0, n_tokens=1, temperature=-1.0), dict(rule="sgld", lr=1.0, n_tokens=1, prior_precision=math.inf),
                dict(rule="psgld", lr=1.0, n_tokens=1, alpha=1.0), dict(rule="psgld", lr=1.0, n_tokens=1, damping=0.0)):
        with pytest.raises(BayesLMError, match="Sampler"):
            sgmcmc.Sampler(**bad)


# ------------------------------------------------------------------ the bank
def _bank(model, capacity=3, vectors=0, seed=0):
    from bayeslms_amd import sgmcmc, swag
    bank = sgmcmc.SampleBank(swag.flat_layout(model)[2], swag.manifest_of(model), capacity, {"rule": "sgld"})
    g = torch.Generator().manual_seed(seed)
    added = []
    for i in range(vectors):
        vec = torch.randn(bank.total, generator=g)
        bank.add(vec, {"kind": "sgld", "epoch": 1 + i // 2, "step": 10 * i, "rate": 0.5 / (i + 1)})
        added.append(vec)
    return bank, added


def _padding_mask(model):
    from bayeslms_amd import swag
    params, offsets, total = swag.flat_layout(model)
    pad = torch.ones(total, dtype=torch.bool)
    for p, o in zip(params, offsets):
        pad[o:o + p.numel()] = False
    return pad


def test_bank_round_trip_ring_and_zeroed_padding(tmp_path):
    from bayeslms_amd import sgmcmc
    from bayeslms_amd._lib import BayesLMError
    m = _lstm()
    # tensors whose length is no multiple of 4 leave padding floats in the layout: the decoder's bias (50 -> 52) and this one (7 -> 8)
    m.register_parameter("odd_tail", torch.nn.Parameter(torch.zeros(7)))
    pad = _padding_mask(m)
    assert pad.sum() == 3 and pad[7] and pad[-2:].all()  # a module's own parameters come first
    bank, added = _bank(m, capacity=3, vectors=5)
    # the ring once full: the latest three, oldest first, and the count of all ever seen
    assert len(bank) == 3 and bank.seen == 5
    mat = bank.matrix()
    assert mat.shape == (3, bank.total) and mat.dtype == torch.float32 and not mat.is_cuda
    for row, vec in zip(mat, added[2:]):
        assert torch.equal(row[~pad], vec[~pad]) and not row[pad].any() and vec[pad].any()
    assert [e["step"] for e in bank.meta] == [20, 30, 40] and bank.kind() == "sgld"
    assert torch.equal(bank.matrix(2), mat[1:]) and torch.equal(bank.latest(2).matrix(), mat[1:]) and bank.latest(2).seen == 5
    added[4].zero_()  # add() copied: the bank does not see the caller's later writes
    assert bank.matrix()[2].any()
    # save / load
    path = os.path.join(str(tmp_path), "bank.pt")
    bank.save(path)
    raw = torch.load(path, map_location="cpu")
    assert raw["format"] == sgmcmc.FORMAT == "bayeslms_amd.samples/1"
    assert sorted(raw) == ["capacity", "format", "manifest", "meta", "sampler", "seen", "total", "vectors"]
    assert isinstance(raw["vectors"], list) and len(raw["vectors"]) == 3  # the rows themselves, never a stacked copy
    back = sgmcmc.SampleBank.load(path)
    assert torch.equal(back.matrix(), mat) and back.meta == bank.meta and back.seen == 5 and back.capacity == 3
    assert back.manifest == bank.manifest and back.sampler == {"rule": "sgld"} and back.describe() == bank.describe()
    d = back.describe()
    assert (d["kind"], d["n"], d["seen"], d["capacity"], d["total"]) == ("sgld", 3, 5, 3, bank.total)
    assert d["meta"][0] == {"kind": "sgld", "epoch": 2, "step": 20, "rate": 0.5 / 3}
    back.add(torch.zeros(bank.total))  # a loaded bank goes on as a ring
    assert len(back) == 3 and back.seen == 6 and back.meta[-1] == {"kind": None, "epoch": None, "step": None, "rate": None}
    assert back.kind() == "mixed"
    # refusals
    torch.save({"format": "bayeslms_amd.swag/1"}, path)
    with pytest.raises(BayesLMError, match="not a sample bank"):
        sgmcmc.SampleBank.load(path)
    with pytest.raises(BayesLMError, match="nothing to write"):
        _bank(m)[0].save(path)
    for cap in (1, 65):
        with pytest.raises(BayesLMError, match="capacity"):
            sgmcmc.SampleBank(8, None, cap)
    with pytest.raises(BayesLMError, match="float32 vector of %d floats" % bank.total):
        bank.add(torch.zeros(bank.total + 1))
    with pytest.raises(BayesLMError, match="float32 vector"):
        bank.add(torch.zeros(bank.total, dtype=torch.float64))
    with pytest.raises(BayesLMError, match="4 of 3 vectors"):
        bank.matrix(4)


def test_bank_refuses_another_model_by_field():
    from bayeslms_amd import swag
    m = _lstm()
    bank, _ = _bank(m, vectors=2)
    bank.check(m)
    bank.check(_lstm(seed=9))  # other values, the same layout
    with pytest.raises(swag.PosteriorMismatch, match="sample bank: field 'total' differs: the bank has %d" % bank.total) as e:
        bank.check(_transformer())
    assert e.value.field == "total"
    from bayeslms_amd import model as M
    torch.manual_seed(0)
    untied = M.RNNModel("LSTM", V, W, W, 2, 0.0, False)
    with pytest.raises(swag.PosteriorMismatch):
        bank.check(untied)
    # the same total, another split: named by the first field that differs
    other = dict(bank.manifest, shapes=[list(s) for s in bank.manifest["shapes"]])
    other["shapes"][0] = [other["shapes"][0][1], other["shapes"][0][0]]
    swapped = type(bank)(bank.total, other, 3)
    with pytest.raises(swag.PosteriorMismatch, match=r"shapes\[0\]"):
        swapped.check(m)


def test_from_checkpoints_on_two_tiny_models_and_its_refusals(tmp_path):
    from bayeslms_amd import sgmcmc, swag
    from bayeslms_amd._lib import BayesLMError
    d = str(tmp_path)
    members = [_lstm(seed=s) for s in (11, 12)]
    paths = []
    for i, mem in enumerate(members):
        paths.append(os.path.join(d, "m%d.pt" % i))
        torch.save({k: v.detach().cpu() for k, v in mem.state_dict().items()}, paths[-1])
    m = _lstm(seed=5)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    bank = sgmcmc.SampleBank.from_checkpoints(m, paths)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())  # the model keeps the weights it had
    assert len(bank) == 2 and bank.seen == 2 and bank.kind() == "checkpoint" and bank.manifest == swag.manifest_of(m)
    assert bank.describe()["meta"] == [{"kind": "checkpoint", "epoch": None, "step": None, "rate": None}] * 2
    for row, mem in zip(bank.matrix(), members):
        assert torch.equal(row, sgmcmc.flat_of(mem))
        params, offsets, _ = swag.flat_layout(mem)
        assert torch.equal(row[offsets[1]:offsets[1] + params[1].numel()].view_as(params[1]), params[1].detach())
    assert not torch.equal(bank.matrix()[0], bank.matrix()[1])
    bank.check(m)
    # refusals: fewer than two, a missing key, a foreign key, another shape -- each named, the model untouched
    with pytest.raises(BayesLMError, match="1 checkpoints: an ensemble has 2..64"):
        sgmcmc.SampleBank.from_checkpoints(m, paths[:1])
    sd = torch.load(paths[1], map_location="cpu")
    key = [k for k in sd if k.endswith("weight_hh_l0")][0]
    torch.save({k: v for k, v in sd.items() if k != key}, os.path.join(d, "missing.pt"))
    with pytest.raises(BayesLMError, match="key %r of the model is missing" % key):
        sgmcmc.SampleBank.from_checkpoints(m, [paths[0], os.path.join(d, "missing.pt")])
    torch.save(dict(sd, stranger=torch.zeros(1)), os.path.join(d, "extra.pt"))
    with pytest.raises(BayesLMError, match="key 'stranger' of the checkpoint is not in the model"):
        sgmcmc.SampleBank.from_checkpoints(m, [paths[0], os.path.join(d, "extra.pt")])
    torch.save(dict(sd, **{key: torch.zeros(3, 3)}), os.path.join(d, "shape.pt"))
    with pytest.raises(BayesLMError, match=r"key %r has shape \(3, 3\)" % key):
        sgmcmc.SampleBank.from_checkpoints(m, [paths[0], os.path.join(d, "shape.pt")])
    torch.save(_transformer().state_dict(), os.path.join(d, "tlm.pt"))
    with pytest.raises(BayesLMError, match="is missing from the checkpoint"):
        sgmcmc.SampleBank.from_checkpoints(m, [paths[0], os.path.join(d, "tlm.pt")])
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())


def test_variational_sites_are_named():
    from bayeslms_amd import model as M, sgmcmc
    assert sgmcmc.variational_site(_lstm()) is None and sgmcmc.variational_site(_transformer()) is None
    torch.manual_seed(0)
    bayes = M.BayesTransformerModel(V, W, 2, W, 2, 0.0, True, "FFN")
    assert sgmcmc.variational_site(bayes) == "transformerlayers.0.linear2.weight_lgstd"


# ------------------------------------------------------------------ the command lines
TRAIN = ["--data", "/nonexistent", "--cuda", "--epochs", "3"]
SG = ["--sgmcmc-save", "bank.pt", "--sgmcmc-lr", "0.1"]


@pytest.mark.parametrize("flags,message", [
    (["--sgmcmc-lr", "0.1"], "--sgmcmc-lr needs --sgmcmc-save"),
    (["--sgmcmc-rule", "psgld"], "--sgmcmc-rule needs --sgmcmc-save"),
    (["--sgmcmc-start", "2"], "--sgmcmc-start needs --sgmcmc-save"),
    (["--sgmcmc-temperature", "1"], "--sgmcmc-temperature needs --sgmcmc-save"),
    (["--sgmcmc-prior-precision", "1"], "--sgmcmc-prior-precision needs --sgmcmc-save"),
    (["--sgmcmc-every", "0"], "--sgmcmc-every needs --sgmcmc-save"),
    (["--sgmcmc-keep", "16"], "--sgmcmc-keep needs --sgmcmc-save"),
    (["--sgmcmc-cycles", "0"], "--sgmcmc-cycles needs --sgmcmc-save"),
    (["--sgmcmc-explore", "0.8"], "--sgmcmc-explore needs --sgmcmc-save"),
    (["--sgmcmc-seed", "1"], "--sgmcmc-seed needs --sgmcmc-save"),
    (["--sgmcmc-save", "bank.pt"], "--sgmcmc-save needs --sgmcmc-lr"),
    (["--sgmcmc-save", "bank.pt", "--sgmcmc-lr", "0"], "--sgmcmc-lr must be positive and finite"),
    (SG + ["--swag-save", "swag.pt"], "--sgmcmc-save with --swag-save"),
    (SG + ["--distill-from", "teacher.pt"], "--sgmcmc-save with --distill-from"),
    (SG + ["--noise-source", "torch"], "--sgmcmc-save with --noise-source torch"),
    (SG + ["--model", "Transformer", "--uncertainty", "Bayesian", "--T_bayes_pos", "FFN"],
     "--sgmcmc-save with --uncertainty Bayesian --T_bayes_pos FFN"),
    (SG + ["--uncertainty", "Variational"], "--sgmcmc-save with --uncertainty Variational --L_v_pos 11"),
    (SG + ["--uncertainty", "Gaussian", "--L_gauss_pos", "33"], "--sgmcmc-save with --uncertainty Gaussian --L_gauss_pos 33"),
    (SG + ["--sgmcmc-start", "4"], "--sgmcmc-start 4 lies beyond --epochs 3"),
    (SG + ["--sgmcmc-start", "0"], "--sgmcmc-start is a 1-based epoch"),
    (SG + ["--sgmcmc-temperature", "-1"], "--sgmcmc-temperature must be finite and >= 0"),
    (SG + ["--sgmcmc-prior-precision", "-1"], "--sgmcmc-prior-precision must be finite and >= 0"),
    (SG + ["--sgmcmc-every", "-1"], "--sgmcmc-every must be 0"),
    (SG + ["--sgmcmc-keep", "1"], "--sgmcmc-keep must lie in 2..64"),
    (SG + ["--sgmcmc-keep", "65"], "--sgmcmc-keep must lie in 2..64"),
    (SG + ["--sgmcmc-cycles", "-1"], "--sgmcmc-cycles must be >= 0"),
    (SG + ["--sgmcmc-explore", "0.5"], "--sgmcmc-explore needs --sgmcmc-cycles"),
    (SG + ["--sgmcmc-cycles", "2", "--sgmcmc-explore", "1"], r"--sgmcmc-explore must lie in \[0, 1\)"),
])
def test_train_refuses_before_anything_is_loaded(flags, message, monkeypatch):
    from bayeslms_amd import train as T
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("BLM_NOISE_SOURCE", raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was asked for"))
    with pytest.raises(SystemExit, match=message):
        T.main(TRAIN + flags)


def test_train_refuses_torchrun(monkeypatch):
    from bayeslms_amd import train as T
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was asked for"))
    with pytest.raises(SystemExit, match=r"--sgmcmc-save runs in a single process.*world size 2"):
        T.main(TRAIN + SG)


def test_train_without_the_flags_keeps_its_configuration():
    from bayeslms_amd import train as T
    args = T.build_parser().parse_args(TRAIN)
    before = set(vars(args))
    assert {f for f in before if f.startswith("sgmcmc")} == set(T.SGMCMC_FLAGS)
    assert T.take_swag_args(args, 1) is None and T.take_sgmcmc_args(args, 1, False) is None
    assert not [f for f in vars(args) if f.startswith(("sgmcmc", "swag"))]
    args = T.build_parser().parse_args(TRAIN + SG + ["--sgmcmc-rule", "psgld", "--sgmcmc-start", "2", "--sgmcmc-cycles", "3"])
    T.take_swag_args(args, 1)
    w = T.take_sgmcmc_args(args, 1, False)
    assert not [f for f in vars(args) if f.startswith("sgmcmc")]
    assert vars(w) == dict(save="bank.pt", lr=0.1, rule="psgld", start=2, temperature=1.0, prior_precision=1.0, every=0, keep=16, cycles=3,
                           explore=0.8, seed=1111)


EVAL = ["--model-path", "/nonexistent/model.pt", "--vocabulary", "/nonexistent/words.txt", "--data", "/nonexistent/test.txt"]
LAPLACE = ["--laplace-prior-precision", "1"]


@pytest.mark.parametrize("source", [["--sample-bank", "bank.pt"], ["--ensemble", "a.pt,b.pt"]], ids=["bank", "ensemble"])
@pytest.mark.parametrize("flags,message", [
    (["--mc-samples", "4"], "with --mc-samples"),
    (["--swag", "swag.pt", "--swag-samples", "2"], "with --swag"),
    (["--laplace", "lap.pt"] + LAPLACE, "with the Laplace flags"),
    (["--laplace-fit-on", "train.txt"] + LAPLACE, "with the Laplace flags"),
    (["--cache-window", "100", "--cache-theta", "1", "--cache-lambda", "0.1"], "with --cache-window"),
    (["--dyneval-lr", "0.1", "--dyneval-decay", "0.1"], "with dynamic evaluation"),
    (["--fit-dyneval-on", "valid.txt", "--dyneval-lr-grid", "0.1", "--dyneval-decay-grid", "0.1"], "with dynamic evaluation"),
    (["--fit-temperature-on", "valid.txt"], "with --fit-temperature-on"),
])
def test_evaluate_refuses_before_anything_is_loaded(source, flags, message, monkeypatch):
    from bayeslms_amd import evaluate as E
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was asked for"))
    with pytest.raises(SystemExit, match=source[0] + " " + message):
        E.main(EVAL + source + flags)


@pytest.mark.parametrize("flags,message", [
    (["--bank-samples", "4"], "--bank-samples needs --sample-bank"),
    (["--sample-bank", "bank.pt", "--ensemble", "a.pt,b.pt"], "--sample-bank and --ensemble exclude each other"),
    (["--ensemble", "a.pt,b.pt", "--bank-samples", "2"], "--bank-samples needs --sample-bank"),
    (["--ensemble", "a.pt"], r"--ensemble takes 2..64 checkpoints separated by commas \(got 1\)"),
    (["--ensemble", ",".join("m%d.pt" % i for i in range(65))], r"--ensemble takes 2..64 checkpoints separated by commas \(got 65\)"),
    (["--sample-bank", "bank.pt", "--bank-samples", "1"], "--bank-samples must lie in 2..64"),
    (["--sample-bank", "bank.pt", "--bank-samples", "65"], "--bank-samples must lie in 2..64"),
])
def test_evaluate_refuses_malformed_bank_flags(flags, message, monkeypatch):
    from bayeslms_amd import evaluate as E
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was asked for"))
    with pytest.raises(SystemExit, match=message):
        E.main(EVAL + flags)


def test_evaluate_accepts_temperature_beside_a_bank():
    from bayeslms_amd import evaluate as E
    E.check_args(E.build_parser().parse_args(EVAL + ["--sample-bank", "bank.pt", "--bank-samples", "8", "--temperature", "2"]))
    E.check_args(E.build_parser().parse_args(EVAL + ["--ensemble", "a.pt, b.pt ,c.pt", "--temperature", "0.5"]))
    assert E.ensemble_paths("a.pt, b.pt ,c.pt,") == ["a.pt", "b.pt", "c.pt"]


def test_report_drops_an_absent_samples_block():
    from bayeslms_amd import engine
    rep = engine.EvalReport(tokens=1, skipped=0, loss=1.0, ppl=math.e)
    assert rep.samples is None and "samples" not in rep.as_dict()
    rep.samples = {"kind": "sgld", "n": 2}
    assert rep.as_dict()["samples"] == {"kind": "sgld", "n": 2}


# ------------------------------------------------------------------ the entry point's argument checks
def test_entry_point_refuses_bad_arguments_before_any_launch():
    from bayeslms_amd import _lib as L
    lib = L.lib()
    f = ctypes.c_float
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rng = L.rng(1, L.STREAM_SGMCMC, 0)
    assert L.STREAM_SGMCMC == 0x60000000

    def call(p_=p, g=p, v=None, sq=p, n=4, clip=0.25, lr=0.1, gs=1.0, wd=0.0, sigma=0.0, alpha=0.99, damping=1e-5, r=ctypes.byref(rng)):
        return lib.blm_sgmcmc_update(p_, g, v, sq, n, f(clip), f(lr), f(gs), f(wd), f(sigma), f(alpha), f(damping), r, None)

    assert call(p_=None) == L.ERR_INVALID and b"blm_sgmcmc_update" in lib.blm_last_error()
    inf, nan = math.inf, math.nan
    for bad in (dict(g=None), dict(sq=None), dict(n=-1), dict(n=(1 << 40) + 1), dict(clip=0.0), dict(clip=-1.0), dict(clip=nan),
                dict(lr=-0.1), dict(lr=inf), dict(lr=nan), dict(sigma=-1.0), dict(sigma=inf), dict(wd=-1.0), dict(wd=nan),
                dict(v=p, alpha=1.0), dict(v=p, alpha=-0.1), dict(v=p, alpha=nan), dict(v=p, damping=0.0), dict(v=p, damping=nan),
                dict(sigma=1.0, r=None)):
        assert call(**bad) == L.ERR_INVALID, bad
        assert b"blm_sgmcmc_update" in lib.blm_last_error(), bad
    # n = 0 is a successful no-op, with or without v and rng; alpha and damping are not looked at without v
    assert call(n=0) == L.OK and call(n=0, v=p) == L.OK and call(n=0, r=None) == L.OK and call(n=0, alpha=7.0, damping=-1.0) == L.OK
