"""CPU: blm_row_stats is declared, exported, bound and refuses bad arguments on the host; the report arithmetic
(engine.report_from_tokens: binning, ECE, top-5, skipped tokens) against hand-computed cases; the window plan every evaluation
walk shares (engine._eval_windows) and the state carrier (model.CarriedState); the evaluate command line's arguments; train.py refuses --test-report under more than one rank."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from bayeslms_amd import _lib as L
    return L, L.lib()


def test_header_declares_and_library_exports_row_stats(lib):
    import ctypes as C
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bayeslm.h")).read(), flags=re.S)
    assert "blm_row_stats" in set(re.findall(r"\b(blm_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    assert "blm_row_stats" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    L, _ = lib
    res, args = L.SIGNATURES["blm_row_stats"]
    assert res is C.c_int and len(args) == 11 and args[1] is C.c_int64 and args[3] is C.c_int and args[4] is C.c_int
    assert "blm_row_stats" not in L.VALUE_RETURNING  # a status: the checked view raises on failure
    assert L.calls().blm_row_stats.errcheck is not None


def test_row_stats_refuses_bad_arguments_before_any_launch(lib):
    L, l = lib
    P = 0x10000  # never dereferenced
    bad = [
        l.blm_row_stats(None, 10, P, 4, 10, P, P, P, P, P, None),       # NULL x
        l.blm_row_stats(P, 10, P, -1, 10, P, P, P, P, P, None),         # negative rows
        l.blm_row_stats(P, 10, P, 4, 0, P, P, P, P, P, None),           # no columns
        l.blm_row_stats(P, 10, P, 4, -3, P, P, P, P, P, None),
        l.blm_row_stats(P, 9, P, 4, 10, P, P, P, P, P, None),           # ldx < V
        l.blm_row_stats(P, 10, None, 4, 10, P, P, P, P, None, None),    # nll without targets
        l.blm_row_stats(P, 10, None, 4, 10, None, P, P, P, P, None),    # rank without targets
        l.blm_row_stats(P, 2 ** 40, P, 2 ** 30, 10, P, P, P, P, P, None),  # extents
        l.blm_row_stats(P, 2 ** 20, P, 2 ** 30, 10, P, P, P, P, P, None),
    ]
    assert bad == [L.ERR_INVALID] * len(bad), bad
    assert b"blm_row_stats" in l.blm_last_error()
    assert l.blm_row_stats(P, 10, None, 4, 10, None, P, P, P, P, None) == L.ERR_INVALID and b"targets" in l.blm_last_error()
    assert l.blm_row_stats(P, 10, P, 0, 10, P, P, P, P, P, None) == L.OK  # no rows: nothing to do, nothing launched
    with pytest.raises(L.BayesLMError, match="blm_row_stats"):
        L.calls().blm_row_stats(None, 10, P, 4, 10, P, P, P, P, P, None)


# ----------------------------------------------------------------------------------------------- report arithmetic
def _report(*a, **k):
    from bayeslms_amd import engine
    return engine.report_from_tokens(*a, **k)


def test_all_tokens_in_one_bin():
    # four tokens of confidence 0.30 .. 0.33 (bin 4 of 15: [4/15, 5/15)), one of them right
    conf = [0.30, 0.31, 0.32, 0.33]
    r = _report([1.0, 2.0, 3.0, 4.0], conf, [0.5, 0.5, 1.0, 2.0], [0, 1, 7, 4], bins=15)
    assert (r.tokens, r.skipped) == (4, 0)
    assert r.loss == 2.5 and r.ppl == math.exp(2.5)
    assert r.accuracy == 0.25 and r.top5_accuracy == 0.75  # ranks 0, 1 and 4 are inside the five best, rank 7 is not
    assert r.mean_conf == pytest.approx(0.315, abs=1e-15) and r.mean_entropy == 1.0
    assert [b[0] for b in r.bins] == [0] * 4 + [4] + [0] * 10 and len(r.bins) == 15
    assert r.bins[4][1] == pytest.approx(0.315, abs=1e-15) and r.bins[4][2] == 0.25
    assert r.ece == pytest.approx(abs(0.25 - 0.315), abs=1e-15)
    assert r.sample_loss is None and r.mean_mi is None and r.mc_samples == 0


def test_confidence_one_lands_in_the_last_bin_and_edges_go_up():
    # B = 4: 0.25 and 0.5 sit on bin edges and belong to the bin they open; 1.0 would open bin 4 and is put into bin 3
    conf = [1.0, 0.25, 0.5, 0.0, 0.999]
    rank = [0, 0, 1, 2, 0]
    r = _report([0.0] * 5, conf, [0.0] * 5, rank, bins=4)
    assert [b[0] for b in r.bins] == [1, 1, 1, 2]
    assert r.bins[3][1] == pytest.approx(0.9995) and r.bins[3][2] == 1.0
    assert r.bins[0][1:] == [0.0, 0.0] and r.bins[1][1:] == [0.25, 1.0] and r.bins[2][1:] == [0.5, 0.0]
    want = (1 * abs(0.0 - 0.0) + 1 * abs(1.0 - 0.25) + 1 * abs(0.0 - 0.5) + 2 * abs(1.0 - 0.9995)) / 5
    assert r.ece == pytest.approx(want, abs=1e-15)
    assert r.accuracy == 0.6 and r.top5_accuracy == 1.0
    one = _report([0.0], [1.0], [0.0], [0], bins=1)
    assert one.bins == [[1, 1.0, 1.0]] and one.ece == 0.0


def test_skipped_tokens_enter_nothing():
    nan = float("nan")
    nll = [2.0, nan, 4.0, nan]
    valid = [True, False, True, False]
    r = _report(nll, [0.9, nan, 0.1, 0.7], [1.0, nan, 3.0, 5.0], [0, -1, 9, -1], valid, bins=2,
                nll_s=[[1.0, 3.0], [nan, nan], [5.0, 3.0], [nan, nan]], h_pred=[1.0, nan, 2.0, 7.0], mi=[0.5, nan, 0.25, 7.0])
    assert (r.tokens, r.skipped) == (2, 2)
    assert r.loss == 3.0 and r.mean_conf == 0.5 and r.mean_entropy == 2.0
    assert r.accuracy == 0.5 and r.top5_accuracy == 0.5
    assert r.bins == [[1, 0.1, 0.0], [1, 0.9, 1.0]]
    assert r.ece == pytest.approx(0.5 * 0.1 + 0.5 * 0.1, abs=1e-15)
    assert r.mc_samples == 2 and r.sample_loss == [3.0, 3.0] and r.sample_loss_mean == 3.0
    assert r.mean_h_pred == 1.5 and r.mean_mi == 0.375
    d = r.as_dict()
    assert "per_token" not in d and d["tokens"] == 2 and d["bins"] == r.bins


def test_sums_are_float64():
    # float32(0.1) summed 2^20 times in float32 drifts by ~1e-3 relative; float32(0.7) * 10 is 6.99999988 in float64: bin 6
    n = 1 << 20
    nll = np.full(n, np.float32(0.1))
    r = _report(nll, np.full(n, np.float32(0.7)), nll, np.zeros(n, np.int32), bins=10)
    assert r.loss == pytest.approx(float(np.float32(0.1)), rel=1e-14)
    assert r.bins[6][0] == n and r.ece == pytest.approx(1.0 - float(np.float32(0.7)), rel=1e-12)


def test_no_tokens_and_bad_bins():
    from bayeslms_amd import BayesLMError
    r = _report([], [], [], [], bins=3)
    assert r.tokens == 0 and r.skipped == 0 and math.isnan(r.loss)
    with pytest.raises(BayesLMError, match="bins"):
        _report([1.0], [0.5], [0.1], [0], bins=0)


def _plan_source():
    import torch
    cols, rows = 3, 47
    return torch.arange(rows * cols).view(cols, rows).t().contiguous()  # the value IS the text position


def _plan(src, recurrent, **kw):
    """engine._eval_windows as a list, each batch with the text positions of its targets"""
    from bayeslms_amd import engine
    return [(d, t, engine._window_positions(src.shape, starts, n), len(starts) * n)
            for d, t, starts, n in engine._eval_windows(src, 5, recurrent, **kw)]


def test_windows_follow_engine_evaluate(monkeypatch):
    """_eval_windows: a stateless model gets the full windows side by side and the ragged one alone, a recurrent one
    consecutive windows as one; every target once, with its text position."""
    monkeypatch.delenv("BLM_EVAL_WINDOWS", raising=False)
    src = _plan_source()
    for recurrent, shapes in ((False, [(5, 27), (1, 3)]), (True, [(45, 3), (1, 3)])):
        got = _plan(src, recurrent)
        assert [tuple(d.shape) for d, _, _, _ in got] == shapes
        for d, t, p, _ in got:
            assert t.tolist() == p.tolist() and (d.reshape(-1) + 1).tolist() == t.tolist()
        assert sorted(np.concatenate([p for _, _, p, _ in got]).tolist()) == sorted(src[1:].reshape(-1).tolist())


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a, b)


_NINE = [(5, 3)] * 9 + [(1, 3)]
_PLAN_CASES = [  # BLM_EVAL_WINDOWS, recurrent, the batches' shapes over all 3 columns (the slice [:, 1:3]: 2 / 3 of the columns)
    (None, False, [(5, 27), (1, 3)]), (None, True, [(45, 3), (1, 3)]),
    ("1", False, _NINE), ("1", True, _NINE),
    ("4", False, [(5, 12), (5, 12), (5, 3), (1, 3)]), ("4", True, [(20, 3), (20, 3), (6, 3)]),
]


@pytest.mark.parametrize("windows,recurrent,shapes", _PLAN_CASES)
def test_window_plan(monkeypatch, windows, recurrent, shapes):
    if windows is None:
        monkeypatch.delenv("BLM_EVAL_WINDOWS", raising=False)
    else:
        monkeypatch.setenv("BLM_EVAL_WINDOWS", windows)
    src = _plan_source()
    got = _plan(src, recurrent)
    assert [tuple(d.shape) for d, _, _, _ in got] == shapes
    for d, t, p, _ in got:
        assert t.tolist() == p.tolist() and (d.reshape(-1) + 1).tolist() == t.tolist()
    assert sorted(np.concatenate([p for _, _, p, _ in got]).tolist()) == sorted(src[1:].reshape(-1).tolist())
    assert sum(w for _, _, _, w in got) == 46  # windows x rows: what evaluate weights each batch's mean loss by
    # a rank's column slice: positions there are relative to the slice, so shapes and targets only
    mine = src[:, 1:3].contiguous()
    got = _plan(mine, recurrent)
    assert [tuple(d.shape) for d, _, _, _ in got] == [(r, c * 2 // 3) for r, c in shapes]
    for d, t, _, _ in got:
        assert (d.reshape(-1) + 1).tolist() == t.tolist()
    assert sorted(np.concatenate([t.numpy() for _, t, _, _ in got]).tolist()) == sorted(mine[1:].reshape(-1).tolist())
    assert sum(w for _, _, _, w in got) == 46


@pytest.mark.parametrize("windows", [None, "4"])
@pytest.mark.parametrize("recurrent", [False, True])
def test_window_plan_ungrouped(monkeypatch, windows, recurrent):
    """group=False, dynamic evaluation's plan: one window at a time whatever the model and BLM_EVAL_WINDOWS say"""
    from bayeslms_amd import BayesLMError, engine
    if windows is None:
        monkeypatch.delenv("BLM_EVAL_WINDOWS", raising=False)
    else:
        monkeypatch.setenv("BLM_EVAL_WINDOWS", windows)
    src = _plan_source()
    got = _plan(src, recurrent, group=False)
    assert [tuple(d.shape) for d, _, _, _ in got] == _NINE
    for d, t, p, _ in got:
        assert t.tolist() == p.tolist() and (d.reshape(-1) + 1).tolist() == t.tolist()
    assert sorted(np.concatenate([p for _, _, p, _ in got]).tolist()) == sorted(src[1:].reshape(-1).tolist())
    first = _plan(src, recurrent, group=False, limit=3)
    assert len(first) == 3 and all(_same(a[0], b[0]) and _same(a[1], b[1]) for a, b in zip(first, got))
    with pytest.raises(BayesLMError, match=r"fit_dyneval: seq_len = 0"):
        engine._eval_windows(src, 0, recurrent, group=False, who="fit_dyneval")
    with pytest.raises(BayesLMError, match=r"dyneval_stats: the stream holds \(1, 3\) rows: two are the least that give a target"):
        engine._eval_windows(src[:1], 5, recurrent, group=False, who="dyneval_stats")


def test_carried_state():
    """model.CarriedState: ``copies`` detached hidden sets for a module with init_hidden, nothing for one without"""
    import torch
    from bayeslms_amd.model import CarriedState

    class Counts(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(()))

        def init_hidden(self, columns):
            return (torch.zeros(columns), torch.zeros(2, columns))

        def forward(self, data, hidden):
            h, c = hidden
            return data * self.w, (h + len(data) * self.w, c + len(data) * self.w)

    class Stateless(torch.nn.Module):
        def forward(self, *args):
            assert len(args) == 1
            return args[0] + 1

    state = CarriedState(Counts(), 4, copies=3)
    out = state(torch.ones(2, 4), 1)
    assert out.requires_grad and out.shape == (2, 4)
    state(torch.ones(3, 4), 1)
    state(torch.ones(7, 4), 0)
    assert [float(h[0]) for h, _ in state.hidden] == [7.0, 5.0, 0.0]
    assert [tuple(c.shape) for _, c in state.hidden] == [(2, 4)] * 3 and float(state.hidden[1][1][1, 3]) == 5.0
    assert not any(t.requires_grad for hc in state.hidden for t in hc)
    free = CarriedState(Stateless(), 4, copies=3)
    assert free.hidden is None and free(torch.zeros(2, 4), 2).tolist() == [[1.0] * 4] * 2 and free.hidden is None


# ----------------------------------------------------------------------------------------------- command lines
def test_evaluate_cli_arguments():
    from bayeslms_amd import evaluate as E
    from bayeslms_amd import generate as G
    p = E.build_parser()
    a = p.parse_args(["--model-path", "m.pt", "--vocabulary", "w.txt", "--data", "t.txt"])
    assert (a.seq_len, a.batch_size, a.mc_samples, a.mc_seed, a.bins, a.write_report, a.write_tokens) == (35, 10, 0, 1111, 15, "", "")
    E.check_args(a)
    # the scorer's model flags, with generate.py's defaults
    g = G.build_parser().parse_args(["--model-path", "m.pt", "--vocabulary", "w.txt"])
    for k in ("model", "emsize", "nhid", "nlayers", "nhead", "uncertainty", "T_bayes_pos", "L_bayes_pos", "L_gauss_pos", "T_gauss_pos",
              "L_v_pos", "T_v_pos"):
        assert getattr(a, k) == getattr(g, k), k
    a = p.parse_args(["--model-path", "m.pt", "--vocabulary", "w.txt", "--data", "t.txt", "--seq-len", "16", "--batch-size", "1",
                      "--mc-samples", "8", "--mc-seed", "7", "--bins", "20", "--write-report", "r.json", "--write-tokens", "t.out",
                      "--model", "Transformer", "--uncertainty", "Bayesian", "--T_bayes_pos", "FFN"])
    assert (a.seq_len, a.batch_size, a.mc_samples, a.mc_seed, a.bins, a.write_report, a.write_tokens) == (16, 1, 8, 7, 20, "r.json", "t.out")
    E.check_args(a)
    for flag in ("--model-path", "--vocabulary", "--data"):
        rest = [x for f in ("--model-path", "--vocabulary", "--data") if f != flag for x in (f, "x")]
        with pytest.raises(SystemExit):
            p.parse_args(rest)
    for bad in (["--mc-samples", "1"], ["--mc-samples", "-2"], ["--mc-samples", "65"], ["--bins", "0"], ["--seq-len", "0"],
                ["--batch-size", "0"]):
        with pytest.raises(SystemExit, match=bad[0]):
            E.main(["--model-path", "m.pt", "--vocabulary", "w.txt", "--data", "t.txt"] + bad)  # before a file or a device is looked at


def test_train_refuses_test_report_under_several_ranks(monkeypatch):
    from bayeslms_amd import train as T
    a = T.build_parser().parse_args([])
    assert a.test_report == "" and a.test_mc_samples == 0  # no flag: nothing new runs
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit, match="single process"):
        T.main(["--test-report", "r.json"])  # at argument parsing: before the process group, the data or a device
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit, match="--test-report"):
        T.main(["--test-mc-samples", "4"])
    with pytest.raises(SystemExit, match="2..64"):
        T.main(["--test-report", "r.json", "--test-mc-samples", "1"])
