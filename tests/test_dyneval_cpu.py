"""CPU: dynamic evaluation's host side -- the float64 reference's own properties, the three entry points in the header, the
library and the binding, their refusals through ctypes (all before any launch), the engine's and the evaluate command's
refusals, and the report's ``dyneval`` block and summary line."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import dyneval_reference as R
from conftest import ROOT

NAMES = ("blm_dyneval_accum", "blm_dyneval_rms", "blm_dyneval_update")


@pytest.fixture(scope="module")
def L():
    from bayeslms_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _arrays(n=97, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    p0 = (p + 0.1 * rng.standard_normal(n)).astype(np.float32)
    ms = (rng.random(n) * 10.0 ** rng.integers(-6, 3, n)).astype(np.float32)
    return p, g, p0, ms


# ------------------------------------------------------------------ the reference's own properties
def test_reference_zero_rates_are_the_identity():
    p, g, p0, ms = _arrays()
    r, rbar, _ = R.rms(ms, 3)
    assert np.array_equal(R.update(p, g, p0, 0.0, 0.0), R.f64(p))
    assert np.array_equal(R.update(p, g, p0, 0.0, 0.0, r, rbar, 0.01), R.f64(p))


def test_reference_entry_without_gradient_at_the_trained_value_does_not_move():
    p, g, p0, ms = _arrays()
    g[10:20], p0[10:20] = 0.0, p[10:20]
    ms[10:15] = 0.0  # also where the statistics never saw it: 0 / (0 + eps rbar), and with eps = 0 no 0 / 0
    r, rbar, _ = R.rms(ms, 3)
    for eps in (0.01, 0.0):
        for out in (R.update(p, g, p0, 0.3, 0.2), R.update(p, g, p0, 0.3, 0.2, r, rbar, eps)):
            assert np.array_equal(out[10:20], R.f64(p)[10:20]) and np.isfinite(out[10:20]).all()
            assert not np.array_equal(out, R.f64(p))  # the others moved


def test_reference_pull_is_clipped_to_one():
    p, g, p0, ms = _arrays()
    g[:] = 0.0
    ms[:5] = 1e6  # r / rbar far above 1 / decay
    r, rbar, _ = R.rms(ms, 1)
    assert (0.5 * r[:5] / rbar > 1.0).all() and (0.5 * r[5:] / rbar < 1.0).any()
    out = R.update(p, g, p0, 0.1, 0.5, r, rbar)
    np.testing.assert_allclose(out[:5], R.f64(p0)[:5], rtol=0, atol=1e-15)  # d = 1: exactly back at the trained value
    out = R.update(p, g, p0, 0.1, 7.0)  # sgd: min(1, lambda)
    np.testing.assert_allclose(out, R.f64(p0), rtol=0, atol=1e-15)


def test_reference_mean_is_over_live_entries_only():
    ms = np.array([4.0, 0.0, 16.0, 0.0, 0.0, 36.0], np.float32)
    r, rbar, live = R.rms(ms, 4)
    assert live == 3 and rbar == (1.0 + 2.0 + 3.0) / 3.0 and np.array_equal(r, [1.0, 0.0, 2.0, 0.0, 0.0, 3.0])
    assert R.rms(np.zeros(4, np.float32), 2)[1:] == (0.0, 0)
    assert np.array_equal(R.accum(ms, np.array([1, 2, 3, 0, 0, 0], np.float32)), [5.0, 4.0, 25.0, 0.0, 0.0, 36.0])


# ------------------------------------------------------------------ header, library, binding
def test_cabi_declares_binds_and_exports_the_entries(L):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bayeslm.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name  # an `int` status in the header
        assert name in exported, name
        res, args = L.SIGNATURES[name]
        assert res is C.c_int and name not in L.VALUE_RETURNING and getattr(L.calls(), name).errcheck is not None, name
    assert [len(L.SIGNATURES[n][1]) for n in NAMES] == [4, 7, 11]
    assert L.SIGNATURES["blm_dyneval_update"][1][5] is C.c_int64 and L.SIGNATURES["blm_dyneval_accum"][1][2] is C.c_int64
    assert re.search(r"#define\s+BLM_DYNEVAL_RMS_WS_FLOATS\s+%d\b" % L.DYNEVAL_RMS_WS_FLOATS, src)


def test_cabi_refusals_reach_no_launch(L):
    # made-up device addresses, 16-byte aligned: an accepted call here has n = 0, which by contract launches nothing
    lib = L.lib()
    A, B, D, E, M, W = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    assert lib.blm_dyneval_accum(A, B, 0, None) == L.OK
    assert lib.blm_dyneval_update(A, B, D, None, None, 0, 0.1, 0.2, 0.01, 1, None) == L.OK
    assert lib.blm_dyneval_update(A, B, D, E, M, 0, 0.0, 0.0, 0.0, 0, None) == L.OK
    assert lib.blm_dyneval_update(A + 4, B + 8, D + 12, E + 4, M + 4, 0, 0.1, 0.2, 0.01, 1, None) == L.OK  # any float alignment
    bad = [("accum", (None, B, 8, None)), ("accum", (A, None, 8, None)), ("accum", (A, B, -1, None)), ("accum", (A, B, 2 ** 41, None)),
           ("rms", (None, 8, 1, B, M, W, None)), ("rms", (A, 8, 1, None, M, W, None)), ("rms", (A, 8, 1, B, None, W, None)),
           ("rms", (A, 8, 1, B, M, None, None)), ("rms", (A, -1, 1, B, M, W, None)), ("rms", (A, 8, 0, B, M, W, None)),
           ("rms", (A, 8, -2, B, M, W, None)), ("rms", (A, 8, 1, B, M, W + 4, None)), ("rms", (A, 2 ** 41, 1, B, M, W, None))]
    ok = dict(p=A, g=B, p0=D, rms=E, mean=M, n=8, lr=0.1, decay=0.2, eps=0.01)
    for over in (dict(p=None), dict(g=None), dict(p0=None), dict(rms=None), dict(mean=None), dict(n=-1), dict(n=2 ** 41),
                 dict(lr=-0.1), dict(lr=float("nan")), dict(lr=float("inf")), dict(decay=-1.0), dict(decay=float("nan")),
                 dict(decay=float("inf")), dict(eps=-1e-3), dict(eps=float("nan")), dict(eps=float("inf"))):
        a = dict(ok, **over)
        bad.append(("update", (a["p"], a["g"], a["p0"], a["rms"], a["mean"], a["n"], a["lr"], a["decay"], a["eps"], 1, None)))
    for which, args in bad:
        name = "blm_dyneval_" + which
        assert getattr(lib, name)(*args) == L.ERR_INVALID, (name, args)
        assert name.encode() in lib.blm_last_error(), (name, args)
    with pytest.raises(L.BayesLMError) as e:
        L.calls().blm_dyneval_update(None, None, None, None, None, 8, 0.1, 0.1, 0.1, 1, None)
    assert e.value.status == L.ERR_INVALID


def test_ops_refusals_name_the_argument():
    import torch
    from bayeslms_amd import ops
    x = torch.zeros(8)
    for call, word in ((lambda: ops.dyneval_accum(x, x), "ms"), (lambda: ops.dyneval_rms(x, 1), "ms"),
                       (lambda: ops.dyneval_update(x, x, x, 0.1, 0.1), "p must live on the GPU"),
                       (lambda: ops.dyneval_update(x, x, x, 0.1, 0.1, rms=x), "rms and mean go together"),
                       (lambda: ops.dyneval_update(x, x, x, 0.1, 0.1, mean=x), "rms and mean go together"),
                       (lambda: ops.dyneval_accum(None, x), "ms must be a tensor")):
        with pytest.raises(ops.BayesLMError, match=word):
            call()


# ------------------------------------------------------------------ engine and command line: refused before anything is touched
def test_engine_refusals_come_before_the_model_is_used():
    from bayeslms_amd import engine, ops

    class Untouchable:  # any use of the model or the text raises AttributeError, not BayesLMError
        pass

    m, s = Untouchable(), Untouchable()
    for kw, word in ((dict(mc_samples=4), "mc_samples"), (dict(temperature=2.0), "temperature"), (dict(cache_window=100), "cache")):
        with pytest.raises(ops.BayesLMError, match=word):
            engine.evaluate_dynamic(m, s, 35, 0.1, 0.1, **kw)
        with pytest.raises(ops.BayesLMError, match=word):
            engine.fit_dyneval(m, s, 35, [0.1], [0.1], **kw)
    for kw, word in ((dict(lr=-1.0), "lr"), (dict(decay=float("nan")), "decay"), (dict(eps=float("inf")), "eps")):
        a = dict(lr=0.1, decay=0.1, eps=0.01)
        a.update(kw)
        with pytest.raises(ops.BayesLMError, match=word):
            engine.evaluate_dynamic(m, s, 35, a["lr"], a["decay"], eps=a["eps"])
    with pytest.raises(ops.BayesLMError, match="lr"):
        engine.fit_dyneval(m, s, 35, [0.1, -2.0], [0.1])
    with pytest.raises(ops.BayesLMError, match="max_windows"):
        engine.fit_dyneval(m, s, 35, [0.1], [0.1], max_windows=0)
    with pytest.raises(ops.BayesLMError, match="windows"):
        engine.dyneval_stats(m, s, 35, 0)
    with pytest.raises(ops.BayesLMError, match="Untouchable"):  # a family that is not supported is refused by name
        engine.evaluate_dynamic(m, s, 35, 0.1, 0.1)


def test_engine_refuses_the_torch_noise_source_and_restores_the_model():
    import torch
    from bayeslms_amd import engine, model as M, ops
    m = M.RNNModel("LSTM", 20, 8, 8, 1, 0.0, True)
    m.set_noise_source("torch")
    m.train()
    before = [(p.data_ptr(), p.grad) for p in m.parameters()]
    sink = lambda w, ids: None  # noqa: E731
    ops.set_embed_grad_sink(sink)
    try:
        with pytest.raises(ops.BayesLMError, match="noise source 'torch'"):
            engine.evaluate_dynamic(m, torch.zeros(9, 2, dtype=torch.int64), 4, 0.1, 0.1)
        m.set_noise_source("philox")
        with pytest.raises(ops.BayesLMError, match="GPU"):  # host tensors: the walk fails inside the session, at its first kernel
            engine.evaluate_dynamic(m, torch.zeros(9, 2, dtype=torch.int64), 4, 0.1, 0.1)
        assert ops._EMBED_SINK is sink and ops._GRAD_HOOK is None
    finally:
        ops.set_embed_grad_sink(None)
    assert m.training and [(p.data_ptr(), p.grad) for p in m.parameters()] == before


@pytest.mark.parametrize("flags,word", [
    (["--dyneval-lr", "0.1"], "go together"),
    (["--dyneval-decay", "0.1"], "go together"),
    (["--dyneval-stats-on", "t.txt"], "need --dyneval-lr"),
    (["--dyneval-lr-grid", "0.1"], "need --dyneval-lr"),
    (["--dyneval-fit-windows", "3"], "need --dyneval-lr"),
    (["--fit-dyneval-on", "v.txt", "--dyneval-lr", "0.1", "--dyneval-decay", "0.1"], "exclude each other"),
    (["--fit-dyneval-on", "v.txt", "--dyneval-lr-grid", "0.1", "--dyneval-decay-grid", "0.1", "--dyneval-decay", "0.1"], "exclude each other"),
    (["--fit-dyneval-on", "v.txt"], "needs --dyneval-lr-grid and --dyneval-decay-grid"),
    (["--fit-dyneval-on", "v.txt", "--dyneval-lr-grid", "0.1"], "needs --dyneval-lr-grid and --dyneval-decay-grid"),
    (["--dyneval-lr", "0.1", "--dyneval-decay", "0.1", "--dyneval-lr-grid", "0.1"], "need --fit-dyneval-on"),
    (["--dyneval-lr", "0.1", "--dyneval-decay", "0.1", "--dyneval-fit-windows", "2"], "need --fit-dyneval-on"),
    (["--dyneval-lr", "0.1", "--dyneval-decay", "0.1", "--mc-samples", "4"], "--mc-samples"),
    (["--dyneval-lr", "0.1", "--dyneval-decay", "0.1", "--temperature", "2"], "--temperature"),
    (["--dyneval-lr", "0.1", "--dyneval-decay", "0.1", "--fit-temperature-on", "v.txt"], "--fit-temperature-on"),
    (["--dyneval-lr", "0.1", "--dyneval-decay", "0.1", "--cache-window", "100", "--cache-theta", "0.1", "--cache-lambda", "0.1"],
     "--cache-window"),
    (["--dyneval-lr", "-0.1", "--dyneval-decay", "0.1"], "--dyneval-lr must be"),
    (["--dyneval-lr", "nan", "--dyneval-decay", "0.1"], "--dyneval-lr must be"),
    (["--dyneval-lr", "0.1", "--dyneval-decay", "inf"], "--dyneval-decay must be"),
    (["--dyneval-lr", "0.1", "--dyneval-decay", "0.1", "--dyneval-epsilon", "-1"], "--dyneval-epsilon must be"),
    (["--dyneval-lr", "0.1", "--dyneval-decay", "0.1", "--dyneval-stats-on", "t.txt", "--dyneval-stats-windows", "0"],
     "--dyneval-stats-windows"),
    (["--fit-dyneval-on", "v.txt", "--dyneval-lr-grid", "0.1,-1", "--dyneval-decay-grid", "0.1"], "--dyneval-lr-grid"),
    (["--fit-dyneval-on", "v.txt", "--dyneval-lr-grid", "0.1", "--dyneval-decay-grid", "x"], "--dyneval-decay-grid"),
    (["--fit-dyneval-on", "v.txt", "--dyneval-lr-grid", "0.1", "--dyneval-decay-grid", "0.1", "--dyneval-fit-windows", "0"],
     "--dyneval-fit-windows"),
    (["--fit-dyneval-on", "v.txt", "--dyneval-lr-grid", "0.1", "--dyneval-decay-grid", "0.1", "--mc-samples", "4"], "--mc-samples"),
])
def test_cli_refuses_conflicting_flags_before_any_file_is_opened(flags, word, tmp_path):
    from bayeslms_amd import evaluate as E
    missing = str(tmp_path / "does_not_exist")  # opening any of them would raise FileNotFoundError, not SystemExit
    with pytest.raises(SystemExit) as e:
        E.main(["--model-path", missing, "--vocabulary", missing, "--data", missing] + flags)
    assert word in str(e.value)
    args = E.build_parser().parse_args(["--model-path", missing, "--vocabulary", missing, "--data", missing] + flags)
    with pytest.raises(SystemExit):
        E.check_dyneval_args(args)  # the refusal is check_dyneval_args' own


def test_cli_accepts_the_documented_combinations_and_says_epsilon_is_unmeasured():
    from bayeslms_amd import evaluate as E
    base = ["--model-path", "m", "--vocabulary", "v", "--data", "d"]
    for flags in ([], ["--dyneval-lr", "0.1", "--dyneval-decay", "0"], ["--dyneval-lr", "0", "--dyneval-decay", "0.1", "--dyneval-stats-on", "t"],
                  ["--fit-dyneval-on", "v", "--dyneval-lr-grid", "0.1,1", "--dyneval-decay-grid", "0,0.01", "--dyneval-fit-windows", "5",
                   "--dyneval-stats-on", "t", "--dyneval-stats-windows", "7", "--dyneval-epsilon", "0.1"]):
        args = E.build_parser().parse_args(base + flags)
        E.check_args(args)
    assert args.dyneval_epsilon == 0.1 and E.build_parser().parse_args(base).dyneval_epsilon == 0.01
    assert "nobody has measured" in re.sub(r"\s+", " ", E.build_parser().format_help())
    assert E.dyneval_grid("0.1, 1,", "--x") == [0.1, 1.0]


# ------------------------------------------------------------------ the report's block and the summary line
def _static():
    from bayeslms_amd import engine
    rep = engine.report_from_tokens([1.0, 2.0], conf=[0.5, 0.25], entropy=[1.0, 1.0], rank=[0, 3])
    return rep


def test_summary_line_and_json_without_the_block_are_what_they_were():
    from bayeslms_amd import evaluate as E
    rep = _static()
    assert E.summary_line(rep) == ("| evaluate | tokens 2 | skipped 0 | loss 1.5000 | ppl %.2f | accuracy 0.5000 | top5 1.0000 | ece %.4f"
                                   % (math.exp(1.5), rep.ece))
    assert "dyneval" not in rep.as_dict() and "cache" not in rep.as_dict() and "temperature" not in rep.as_dict()
    import dataclasses
    names = [f.name for f in dataclasses.fields(rep)]
    assert names[-1] == "temperature" and names.index("dyneval") == len(names) - 2


def test_dyneval_block_and_summary_line_from_a_hand_made_report():
    from bayeslms_amd import engine, evaluate as E
    rep = _static()
    plain = E.summary_line(rep)
    dyn = engine.DynEvalReport(tokens=2, loss=1.25, ppl=math.exp(1.25), lr=0.002, decay=0.02, eps=0.01, rule="rms", windows=6, updates=5,
                               per_token={"nll": np.zeros(2)})
    assert sorted(dyn.as_dict()) == ["decay", "eps", "loss", "lr", "ppl", "rule", "tokens", "updates", "windows"]
    rep.dyneval = E.dyneval_block(dyn, rep)
    assert sorted(rep.dyneval) == ["base_loss", "base_ppl", "decay", "eps", "loss", "lr", "ppl", "rule", "tokens", "updates", "windows"]
    assert rep.dyneval["base_loss"] == 1.5 and rep.as_dict()["dyneval"] == rep.dyneval
    assert E.summary_line(rep) == plain + " | dyneval rule rms lr 0.002 decay 0.02 | loss 1.5000 -> 1.2500 | ppl %.2f -> %.2f" % (
        math.exp(1.5), math.exp(1.25))
    fit = engine.DynEvalFit(lr=0.002, decay=0.02, loss=1.2, loss_static=1.4, curve=[[0.0, 0.0, 1.4], [0.002, 0.02, 1.2]])
    block = E.dyneval_block(dyn, rep, fit, "valid.txt")
    assert {k: block[k] for k in ("fitted_on", "fit_loss_before", "fit_loss_after", "curve")} == {
        "fitted_on": "valid.txt", "fit_loss_before": 1.4, "fit_loss_after": 1.2, "curve": fit.curve}
    import json
    json.dumps(block)
