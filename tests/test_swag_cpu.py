"""CPU: the host side of SWAG (bayeslms_amd/swag.py and the two command lines' refusals); the kernels are tested on the GPU
(tests/test_gpu_swag.py)."""
import math

import numpy as np
import pytest
import torch

import swag_reference as R


def _tiny():
    from bayeslms_amd import model as M
    torch.manual_seed(1)
    return M.RNNModel("LSTM", 20, 8, 8, 2, 0.0, True)


def _filled(model, rank=2, n=3):
    from bayeslms_amd import swag
    man = swag.manifest_of(model)
    post = swag.SwagPosterior(man["total"], rank, None, man)
    g = torch.Generator().manual_seed(2)
    post.mean.copy_(torch.randn(post.total, generator=g))
    post.m2.copy_(torch.rand(post.total, generator=g))
    post.dev.copy_(torch.randn(rank, post.total, generator=g))
    post.n = n
    return post


def test_coefficients_of_the_two_forms():
    from bayeslms_amd import swag
    c = 0.5
    assert swag.coefficients(c, 0) == (math.sqrt(c), 0.0, 0) and swag.coefficients(c, 1) == (math.sqrt(c), 0.0, 0)
    assert swag.coefficients(c, 2) == (math.sqrt(c / 2), math.sqrt(c / 2), 2)
    a, b, k = swag.coefficients(c, 20)
    assert (a, k) == (0.5, 20) and b == math.sqrt(c / 38)
    assert swag.coefficients(c, 20, diag=True) == (math.sqrt(c), 0.0, 0)
    assert swag.coefficients(0.0, 20) == (0.0, 0.0, 20)
    for k_live in (0, 1, 2, 20):
        for diag in (False, True):
            assert swag.coefficients(c, k_live, diag) == R.coefficients(c, k_live, diag)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(swag.BayesLMError, match="scale"):
            swag.coefficients(bad, 3)


def test_manifest_follows_the_flat_layout():
    from bayeslms_amd import swag
    m = _tiny()
    man = swag.manifest_of(m)
    params = [p for p in m.parameters() if p.requires_grad]
    assert man["names"][0] == "encoder.weight" and "decoder.weight" not in man["names"]  # tied: once, under its first name
    assert man["shapes"] == [list(p.shape) for p in params] and man["offsets"][0] == 0
    assert all(o % 4 == 0 for o in man["offsets"]) and man["total"] % 4 == 0
    assert man["total"] >= sum(p.numel() for p in params)


def test_posterior_round_trip_and_the_mean_as_a_state_dict(tmp_path):
    from bayeslms_amd import swag
    m = _tiny()
    post = _filled(m)
    path = str(tmp_path / "swag.pt")
    post.save(path)
    back = swag.SwagPosterior.load(path)
    assert (back.total, back.rank, back.n, back.k_live) == (post.total, 2, 3, 2) and back.manifest == post.manifest
    assert torch.equal(back.mean, post.mean) and torch.equal(back.m2, post.m2) and torch.equal(back.dev, post.dev)
    back.check(m)
    assert back.describe() == {"n": 3, "rank": 2, "k_live": 2, "total": post.total}
    sd = back.mean_state_dict(m)
    assert list(sd) == list(m.state_dict()) and sd["decoder.weight"].data_ptr() != sd["encoder.weight"].data_ptr()
    assert torch.equal(sd["decoder.weight"], sd["encoder.weight"])
    off = dict(zip(post.manifest["names"], post.manifest["offsets"]))
    for name, p in m.named_parameters():
        assert torch.equal(sd[name].reshape(-1), post.mean[off[name]:off[name] + p.numel()]), name
    other = _tiny()
    other.load_state_dict(sd)
    post.load_flat(m, post.mean)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), other.state_dict().values()))
    torch.save({"format": "something else"}, str(tmp_path / "x.pt"))
    with pytest.raises(swag.BayesLMError, match="not a SWAG posterior"):
        swag.SwagPosterior.load(str(tmp_path / "x.pt"))
    with pytest.raises(swag.BayesLMError, match="no iterate collected"):
        swag.SwagPosterior(8, 0).save(str(tmp_path / "y.pt"))
    with pytest.raises(swag.BayesLMError, match="rank = 33"):
        swag.SwagPosterior(8, 33)


def test_a_posterior_of_another_model_is_refused_by_field():
    from bayeslms_amd import model as M, swag
    m = _tiny()
    post = _filled(m)
    torch.manual_seed(1)
    wider = M.RNNModel("LSTM", 20, 12, 12, 2, 0.0, True)
    with pytest.raises(swag.PosteriorMismatch, match="field 'total' differs") as e:
        post.check(wider)
    assert e.value.field == "total" and e.value.found == post.total
    untied = M.RNNModel("LSTM", 20, 8, 8, 2, 0.0, False)
    with pytest.raises(swag.PosteriorMismatch, match="total|len\\(names\\)"):
        post.check(untied)
    # the same length, another split: the first differing entry is named
    twin = _filled(m)
    twin.manifest = dict(post.manifest, names=list(post.manifest["names"]))
    twin.manifest["names"][2] = "rnn.other"
    with pytest.raises(swag.PosteriorMismatch, match=r"field 'names\[2\]' differs: the posterior has 'rnn.other'"):
        twin.check(m)
    twin.manifest = dict(post.manifest, shapes=[list(s) for s in post.manifest["shapes"]])
    twin.manifest["shapes"][1] = [1, 2]
    with pytest.raises(swag.PosteriorMismatch, match=r"field 'shapes\[1\]' differs"):
        twin.check(m)


def test_draw_is_refused_beyond_its_byte_budget():
    from bayeslms_amd import swag
    post = _filled(_tiny())
    need = 4 * 5 * post.total
    with pytest.raises(swag.BayesLMError, match=r"5 samples of %d floats are %d bytes \(.* GiB\), beyond the budget of %d bytes"
                       % (post.total, need, need - 1)):
        post.draw(5, 1, budget=need - 1)
    assert swag.DRAW_BYTES == 8 << 30
    with pytest.raises(swag.BayesLMError):  # within the budget it goes to the kernel, and there is no CPU path
        post.draw(5, 1, budget=need)
    with pytest.raises(swag.BayesLMError, match="samples = 0"):
        post.draw(0, 1)


def test_collector_schedule():
    from bayeslms_amd import swag

    class Flat:
        total = 8
        flat_param = torch.zeros(8)

    class Trainer:
        flat, world, model = Flat(), 1, None

    seen = []
    c = swag.SwagCollector(Trainer(), 0, start_epoch=2, every=0, manifest={"total": 8})
    c._collect = lambda: seen.append("c") or len(seen)
    assert [c.after_step(1), c.epoch_end(1), c.after_step(2), c.epoch_end(2), c.epoch_end(3)] == [None, None, None, 1, 2]
    seen.clear()
    c = swag.SwagCollector(Trainer(), 0, start_epoch=2, every=3, manifest={"total": 8})
    c._collect = lambda: seen.append("c") or len(seen)
    got = [c.after_step(1) for _ in range(4)] + [c.after_step(2) for _ in range(7)] + [c.epoch_end(2)]
    assert got == [None] * 4 + [None, None, 1, None, None, 2, None] + [None]
    t = Trainer()
    t.world = 2
    with pytest.raises(swag.BayesLMError, match="data-parallel collection is not built"):
        swag.SwagCollector(t, 0)
    with pytest.raises(swag.BayesLMError, match="start_epoch"):
        swag.SwagCollector(Trainer(), 0, start_epoch=0, manifest={"total": 8})


@pytest.mark.parametrize("flags,message", [
    (["--swag-start", "2"], "--swag-start needs --swag-save"),
    (["--swag-every", "5"], "--swag-every needs --swag-save"),
    (["--swag-rank", "3"], "--swag-rank needs --swag-save"),
    (["--swag-lr", "0.1"], "--swag-lr needs --swag-save"),
    (["--swag-save", "s.pt", "--swag-rank", "33"], "--swag-rank must lie in 0..32"),
    (["--swag-save", "s.pt", "--swag-start", "0"], "--swag-start is a 1-based epoch"),
    (["--swag-save", "s.pt", "--swag-every", "-1"], "--swag-every must be 0"),
    (["--swag-save", "s.pt", "--swag-lr", "0"], "--swag-lr must be positive and finite"),
    (["--swag-save", "s.pt", "--swag-start", "9", "--epochs", "3"], "--swag-start 9 lies beyond --epochs 3"),
])
def test_train_refuses_before_anything_is_loaded(flags, message):
    from bayeslms_amd import train as T
    with pytest.raises(SystemExit, match=message):
        T.main(["--data", "/nonexistent", "--cuda"] + flags)


def test_train_refuses_swag_under_torchrun_and_keeps_its_configuration_print(monkeypatch):
    from bayeslms_amd import train as T
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--swag-save runs in a single process"):
        T.main(["--data", "/nonexistent", "--cuda", "--swag-save", "s.pt"])
    args = T.build_parser().parse_args(["--data", "x"])
    assert T.take_swag_args(args, 1) is None and not any(k.startswith("swag") for k in vars(args))  # what the log prints
    args = T.build_parser().parse_args(["--data", "x", "--swag-save", "s.pt", "--epochs", "3"])
    w = T.take_swag_args(args, 1)
    assert (w.save, w.start, w.every, w.rank, w.lr) == ("s.pt", 1, 0, 20, None)


BASE = ["--model-path", "m.pt", "--vocabulary", "w.txt", "--data", "t.txt"]


@pytest.mark.parametrize("flags,message", [
    (["--swag-samples", "3"], "--swag-samples needs --swag"),
    (["--swag-scale", "0.5"], "--swag-scale needs --swag"),
    (["--swag-diag", "1"], "--swag-diag needs --swag"),
    (["--swag", "s.pt"], "--swag needs --swag-samples"),
    (["--swag", "s.pt", "--swag-samples", "1"], "--swag-samples must be 0 .* or lie in 2..64"),
    (["--swag", "s.pt", "--swag-samples", "65"], "--swag-samples must be 0 .* or lie in 2..64"),
    (["--swag", "s.pt", "--swag-samples", "0", "--swag-scale", "1"], "--swag-samples 0 draws none"),
    (["--swag", "s.pt", "--swag-samples", "2", "--swag-scale", "-1"], "--swag-scale must be finite and >= 0"),
    (["--swag", "s.pt", "--swag-samples", "2", "--mc-samples", "4"], "--swag with --mc-samples"),
    (["--swag", "s.pt", "--swag-samples", "2", "--fit-temperature-on", "v.txt"], "--swag with --fit-temperature-on"),
    (["--swag", "s.pt", "--swag-samples", "2", "--cache-window", "10", "--cache-theta", "1", "--cache-lambda", "0.1"],
     "--swag with --cache-window"),
    (["--swag", "s.pt", "--swag-samples", "2", "--dyneval-lr", "0.1", "--dyneval-decay", "0.1"], "--swag with dynamic evaluation"),
    (["--swag", "s.pt", "--swag-samples", "2", "--fit-dyneval-on", "v.txt", "--dyneval-lr-grid", "1", "--dyneval-decay-grid", "1"],
     "--swag with dynamic evaluation"),
])
def test_evaluate_refuses_before_anything_is_loaded(flags, message):
    from bayeslms_amd import evaluate as E
    with pytest.raises(SystemExit, match=message):
        E.check_args(E.build_parser().parse_args(BASE + flags))


def test_evaluate_accepts_the_flags_and_the_report_block_is_optional():
    from bayeslms_amd import engine, evaluate as E
    E.check_args(E.build_parser().parse_args(BASE + ["--swag", "s.pt", "--swag-samples", "8", "--temperature", "1.5"]))
    E.check_args(E.build_parser().parse_args(BASE + ["--swag", "s.pt", "--swag-samples", "0"]))
    rep = engine.report_from_tokens(np.array([1.0, 2.0]), np.array([0.5, 0.6]), np.array([1.0, 1.0]), np.array([0, 3]))
    plain = E.summary_line(rep)
    assert "swag" not in rep.as_dict() and "swag" not in plain
    rep.swag = {"n": 4, "rank": 2, "k_live": 2, "total": 10, "scale": 0.5, "diag": False, "samples": 8, "seed": 1111, "path": "s.pt"}
    assert rep.as_dict()["swag"] == rep.swag and E.summary_line(rep) == plain + " | swag n 4 rank 2 scale 0.5 samples 8"


def test_stream_class_and_struct_match_the_header():
    import os
    import re
    from bayeslms_amd import _lib as L
    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "bayeslm.h")).read()
    assert int(re.search(r"#define BLM_STREAM_SWAG\s+(0x[0-9a-fA-F]+)u", h).group(1), 16) == L.STREAM_SWAG == 0x40000000
    for name, v in (("RANK", L.SWAG_RANK_MAX), ("DRAWS", L.SWAG_DRAWS_MAX), ("SAMPLES", L.SWAG_SAMPLES_MAX)):
        assert int(re.search(r"#define BLM_SWAG_%s_MAX (\d+)" % name, h).group(1)) == v


def test_struct_layout_of_blm_swag_draw(tmp_path):
    """sizeof / offsetof of blm_swag_draw as gcc sees the header == the ctypes mirror (the mechanism of test_cabi_cpu.py)"""
    import ctypes
    import os
    import subprocess
    from bayeslms_amd import _lib as L
    from conftest import ROOT
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bayeslm.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(blm_swag_draw), offsetof(blm_swag_draw, a),'
                   ' offsetof(blm_swag_draw, inv_n), offsetof(blm_swag_draw, var_floor), offsetof(blm_swag_draw, sample_id),'
                   ' offsetof(blm_swag_draw, rng)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    D = L.SwagDraw
    assert got == [ctypes.sizeof(D), D.a.offset, D.inv_n.offset, D.var_floor.offset, D.sample_id.offset, D.rng.offset]
