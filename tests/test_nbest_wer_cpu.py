"""CPU: the host side of the n-best WER evaluation (bayeslms_amd/nbest_wer.py, python -m bayeslms_amd.wer) and its plain-Python
reference (tests/nbest_reference.py).  The GPU kernels are tested in tests/test_gpu_nbest_wer.py."""
import itertools
import json
import os
import re

import numpy as np
import pytest
import torch

import nbest_reference as R
from conftest import ROOT

from bayeslms_amd import nbest_wer as W  # noqa: E402
from bayeslms_amd import wer as CLI  # noqa: E402


# ---- the reference itself ----
def test_reference_alignment_equals_brute_force_enumeration():
    """every pair of sequences of length <= 6 over a 3-word alphabet would be 1093^2 pairs: all pairs up to length 3, and one in
    11 of a 1-in-35 lattice of the longer ones -- cost and the fewest-insertions breakdown against the enumeration of every alignment"""
    seqs = [list(s) for n in range(7) for s in itertools.product(range(3), repeat=n)]
    short = [s for s in seqs if len(s) <= 3]
    for a in short:
        for b in short:
            assert R.align(a, b) == R.brute_force(a, b), (a, b)
    k = 0
    for a in seqs[::7]:
        for b in seqs[::5]:
            k += 1
            if k % 11 == 0 and len(a) + len(b) > 6:
                assert R.align(a, b) == R.brute_force(a, b), (a, b)


def test_reference_tie_rule_and_symmetry():
    assert R.align([1, 2], [2, 1]) == (2, 2, 0, 0)  # two substitutions, not an insertion and a deletion
    assert R.align([], []) == (0, 0, 0, 0) and R.align([5], []) == (1, 0, 1, 0) and R.align([], [5, 6]) == (2, 0, 0, 2)
    rng = np.random.default_rng(0)
    for _ in range(200):
        a, b = (rng.integers(0, 2, rng.integers(0, 9)).tolist() for _ in range(2))
        c, s, i, d = R.align(a, b)
        assert R.align(b, a) == (c, s, d, i) and i - d == len(a) - len(b)


def test_reference_bad_pairs_and_blocks():
    tok, off = [1, 2, 3, 4], [0, 2, 4, 3]  # the third sequence is reversed
    cost, sid = R.edit_distance(tok, off, [0, 0, 2, 3, -1], [1, 0, 0, 0, 0])
    assert cost.tolist() == [2, 0, -1, -1, -1] and sid[0].tolist() == [2, 0, 0] and sid[2].tolist() == [-1, -1, -1]
    dist, doff = R.pairwise([1, 2, 1, 3, 1], [0, 2, 4, 5], [0, 3, 3])
    assert doff.tolist() == [0, 9] and dist.reshape(3, 3).tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]]


# ---- a hand-worked example ----
NBEST = {"u1": ["a b c", "a x c d", "a b"], "u2": ["p q", "q"], "u3": ["m", " ", "m n o"]}
REFS = {"u1": ["a", "b", "c"], "u2": ["q"], "u3": ["m", "n"], "u4": ["z", "z"]}
#            err (sub, ins, del) of every hypothesis against its reference:
#   u1: a b c -> 0;  a x c d -> 2 (1, 1, 0);  a b -> 1 (0, 0, 1)
#   u2: p q -> 1 (0, 1, 0);  q -> 0
#   u3: m -> 1 (0, 0, 1);  (empty) -> 2 (0, 0, 2);  m n o -> 1 (0, 1, 0)
NN = {"u1-1": 9.0, "u1-2": 2.0, "u1-3": 5.0, "u2-1": 3.0, "u2-2": 4.0, "u3-1": 6.0, "u3-2": 1.0, "u3-3": 6.0}
AC = {k: 0.0 for k in NN}
AC["u2-1"] = 10.0


def _evaluate(**kw):
    args = dict(nbest=NBEST, refs=REFS, costs={"ac": AC, "g": None, "lm": None, "nn": [("nn", NN)]},
                grid=W.make_grid([1.0, 4.0], [1.0], [0.0]), device="cpu", backend=R.Backend())
    args.update(kw)
    return W.evaluate(**args)


def test_hand_worked_example():
    rep = _evaluate()
    d = rep.to_dict()
    assert d["utterances"] == 3 and d["ref_words"] == 6  # u4 has no list: skipped in mode "present"
    assert d["first"] == {"err": 2, "sub": 0, "ins": 1, "del": 1, "wer": 100.0 * 2 / 6, "ser": 100.0 * 2 / 3}
    assert d["oracle"] == {"err": 1, "sub": 0, "ins": 0, "del": 1, "wer": 100.0 / 6, "ser": 100.0 / 3}  # u3: the first of its two 1s
    # L = 1: totals ac + nn -> u1 picks 2 (2 errors), u2 picks 2 (4 < 13: 0 errors), u3 picks 2 (empty: 2 deletions)
    # L = 4: ac + 4 nn -> the same order inside u1 and u3; u2: 22 against 16 -> still 2
    g0, g1 = d["systems"][0]["grid"]
    assert g0 == {"lmwt": 1.0, "nnweight": 1.0, "wip": 0.0, "err": 4, "sub": 1, "ins": 1, "del": 2, "wer": 100.0 * 4 / 6,
                  "ser": 100.0 * 2 / 3}
    assert {k: g1[k] for k in W.FIELDS} == {k: g0[k] for k in W.FIELDS}
    assert d["systems"][0]["best"] == g0  # the first in grid order on a tie
    assert rep.picks["nn"] == [1, 1, 1] and rep.picks["first"] == [0, 0, 0] and rep.picks["oracle"] == [0, 1, 0]
    assert "mbr" not in d


def test_insertion_penalty_and_nnweight_move_the_picks():
    # w = 0 takes the old LM's cost instead of the neural one; p charges every word of the hypothesis
    lm = {k: 0.0 for k in NN}
    lm["u1-1"] = -0.5
    rep = _evaluate(costs={"ac": None, "g": None, "lm": lm, "nn": [("nn", NN)]}, grid=[(1.0, 0.0, 0.0), (1.0, 0.0, 1.0)])
    assert rep.picks["nn"] == [0, 0, 0]  # (w = 0, p = 0): lm alone, ties to the first
    g1 = rep.systems[0]["grid"][1]       # p = 1: u1 -0.5 + 3 against 0 + 2 -> 'a b'; u2 -> 'q'; u3 -> the empty hypothesis
    assert (g1["err"], g1["sub"], g1["ins"], g1["del"]) == (3, 0, 0, 3)


def test_modes():
    rep = _evaluate(mode="all")
    d = rep.to_dict()
    assert d["utterances"] == 4 and d["ref_words"] == 8
    assert d["first"] == {"err": 4, "sub": 0, "ins": 1, "del": 3, "wer": 50.0, "ser": 75.0}
    assert rep.utts == ["u1", "u2", "u3", "u4"] and rep.picks["nn"][-1] == -1
    with pytest.raises(SystemExit, match="u4"):
        _evaluate(mode="strict")
    with pytest.raises(Exception, match="mode"):
        _evaluate(mode="some")


def test_ignore_words():
    rep = _evaluate(ignore_words={"x", "d", "p"})
    # u1's second hypothesis becomes `a c` (one deletion), u2's first `q` (correct)
    assert rep.to_dict()["first"]["err"] == 1 and rep.systems[0]["grid"][0]["err"] == 1 + 0 + 2


def test_mbr_block_and_batching():
    rep = _evaluate(mbr=True, budget_bytes=40)  # blocks of 36, 16 and 36 bytes: three batches of one utterance
    one = _evaluate(mbr=True)
    assert rep.to_dict()["mbr"] == one.to_dict()["mbr"] and rep.picks["nn/mbr"] == one.picks["nn/mbr"]
    m = one.to_dict()["mbr"][0]
    assert set(m) == {"name", "lmwt", "nnweight", "wip", "posterior_scale", "mean_risk"} | set(W.FIELDS)
    assert (m["lmwt"], m["nnweight"], m["wip"]) == (1.0, 1.0, 0.0) and m["mean_risk"] >= 0.0
    explicit = _evaluate(mbr=True, mbr_point=(2.0, 1.0, 0.0))
    assert explicit.to_dict()["mbr"][0]["lmwt"] == 2.0 and explicit.to_dict()["mbr"][0]["posterior_scale"] == 1.0


def test_batches_under_a_byte_budget():
    assert W.batches([3, 2, 3], 40) == [(0, 1), (1, 2), (2, 3)]
    assert W.batches([3, 2, 3], 52) == [(0, 2), (2, 3)]
    assert W.batches([3, 2, 3], 1 << 30) == [(0, 3)]
    assert W.batches([100, 1, 1], 8) == [(0, 1), (1, 3)]  # a list beyond the budget is a batch of its own
    assert W.batches([], 8) == []
    for budget in (4, 16, 36, 100):
        b = W.batches([1, 2, 3, 1, 1, 2], budget)
        assert [x for lo, hi in b for x in range(lo, hi)] == list(range(6))
        assert all(sum(4 * n * n for n in [1, 2, 3, 1, 1, 2][lo:hi]) <= budget or hi - lo == 1 for lo, hi in b)


def test_grid_parsers():
    assert W.parse_values("7:17") == [float(v) for v in range(7, 18)]
    assert W.parse_values("0:1:0.1") == [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]
    assert W.parse_values("0,0.5,1") == [0.0, 0.5, 1.0] and W.parse_values("12") == [12.0] and W.parse_values("3:3") == [3.0]
    for bad in ("a", "1:2:0", "5:1", "1:2:3:4", ""):
        with pytest.raises(SystemExit):
            W.parse_values(bad)
    g = W.make_grid([7, 8], [0.0, 0.5], [0.0], 2.0)
    assert g == [(7.0, 0.0, 0.0, 2.0), (7.0, 0.5, 0.0, 2.0), (8.0, 0.0, 0.0, 2.0), (8.0, 0.5, 0.0, 2.0)]


def test_archives_and_key_mismatches(tmp_path):
    p = tmp_path / "lmwt.nn"
    p.write_text("u1-1 9\nu1-2 2.5\n\nu1-3 -1e1\n")
    assert W.read_archive(str(p)) == {"u1-1": 9.0, "u1-2": 2.5, "u1-3": -10.0}
    p.write_text("u1-1 9\nu1-1 2\n")
    with pytest.raises(SystemExit, match="u1-1 twice"):
        W.read_archive(str(p))
    p.write_text("u1-1 9 3\n")
    with pytest.raises(SystemExit, match="line 1"):
        W.read_archive(str(p))
    p.write_text("u1-1 x\n")
    with pytest.raises(SystemExit, match="not a number"):
        W.read_archive(str(p))
    t = tmp_path / "text"
    t.write_text("u1 a b c\nu2\n\nu3 m\n")
    assert W.read_text(str(t)) == {"u1": ["a", "b", "c"], "u2": [], "u3": ["m"]}
    assert W.match_archive(NBEST, ["u2", "u1"], NN, "nn") == [3.0, 4.0, 9.0, 2.0, 5.0]  # other utterances' values are not asked for
    short = dict(NN)
    del short["u3-2"]
    with pytest.raises(SystemExit, match="no value for u3-2"):
        W.match_archive(NBEST, ["u1", "u2", "u3"], short, "lmwt.nn")
    with pytest.raises(SystemExit, match="lmwt.nn holds u2-3"):
        W.match_archive(NBEST, ["u1", "u2", "u3"], dict(NN, **{"u2-3": 1.0}), "lmwt.nn")
    with pytest.raises(SystemExit, match="no value for u3-2"):
        _evaluate(costs={"ac": None, "g": None, "lm": None, "nn": [("nn", short)]})


def test_json_layout_and_writers(tmp_path):
    rep = _evaluate(mbr=True, costs={"ac": AC, "g": None, "lm": None, "nn": [("mean", NN), ("mc8", dict(NN, **{"u1-1": 0.0}))]})
    W.write_report(str(tmp_path / "r.json"), rep)
    d = json.load(open(tmp_path / "r.json"))
    assert list(d) == ["utterances", "ref_words", "first", "oracle", "systems", "mbr"]
    assert [s["name"] for s in d["systems"]] == ["mean", "mc8"] and [m["name"] for m in d["mbr"]] == ["mean", "mc8"]
    for blk in [d["first"], d["oracle"]] + [s["best"] for s in d["systems"]] + [p for s in d["systems"] for p in s["grid"]] + d["mbr"]:
        assert set(W.FIELDS) <= set(blk)
    assert d["systems"][1]["best"]["err"] == 2  # the second file prefers u1's correct hypothesis
    best = W.best_transcripts(NBEST, rep, name="mc8")
    assert best == [("u1", "a b c"), ("u2", "q"), ("u3", "")]
    W.write_best(str(tmp_path / "best.txt"), best)
    assert open(tmp_path / "best.txt").read() == "u1 a b c\nu2 q\nu3\n"
    assert W.read_text(str(tmp_path / "best.txt")) == {"u1": ["a", "b", "c"], "u2": ["q"], "u3": []}  # round trip
    W.write_utt(str(tmp_path / "utt.txt"), rep)
    lines = open(tmp_path / "utt.txt").read().splitlines()
    assert len(lines) == 3 and lines[0].split()[:7] == ["u1", "3", "3", "0", "0", "2", "2"] and len(lines[0].split()) == 10
    table = rep.table()
    assert "3 utterances, 6 reference words" in table and "mc8 mbr" in table and "oracle" in table


def test_command_line_parses_its_options():
    a = CLI.build_parser().parse_args(["--words-text", "w", "--ref-text", "t", "--nn", "x/lmwt.nn", "--nn", "y/lmwt.nn", "--mbr", "1",
                                       "--mode", "all", "--wip", "0,0.5,1", "--posterior-scale", "0.5"])
    assert a.nn == ["x/lmwt.nn", "y/lmwt.nn"] and a.mbr == 1 and a.lmwt == "7:17" and a.nnweight == "0:1:0.1" and a.mode == "all"
    with pytest.raises(SystemExit):
        CLI.build_parser().parse_args(["--words-text", "w", "--ref-text", "t", "--mode", "none"])


def test_product_ops_refuse_host_tensors():
    from bayeslms_amd import ops, BayesLMError
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(BayesLMError):
        ops.edit_distance(z, torch.zeros(2, dtype=torch.int64), z[:1], z[:1])
    with pytest.raises(BayesLMError):
        ops.pairwise_edit_distance(z, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(BayesLMError):
        ops.nbest_select(torch.zeros(2, dtype=torch.float64), None, None, None, None, torch.zeros(2, dtype=torch.int64), [(1, 0, 0)])
    with pytest.raises(BayesLMError):
        ops.nbest_mbr(torch.zeros(2, dtype=torch.float64), None, None, None, None, torch.zeros(2, dtype=torch.int64), z,
                      torch.zeros(1, dtype=torch.int64), [(1, 0, 0)])
    for bad in ([], [(0.0, 0, 0)], [(float("inf"), 0, 0)], [(1.0, 0, 0, -1.0)], [(1.0, 0)]):
        with pytest.raises(BayesLMError):
            ops.nbest_grids(bad)
    chunks = ops.nbest_grids([(1.0 + k, 0.5, 0.25) for k in range(65)])
    assert [(k0, s.G) for k0, s in chunks] == [(0, 64), (64, 1)] and chunks[1][1].lmwt[0] == 65.0 and chunks[0][1].pscale[3] == 1.0


# ---- the three entries, once in every layer ----
def test_header_binding_and_ops_name_the_three_entries_once():
    from bayeslms_amd import _lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bayeslm.h")).read(), flags=re.S)
    ops_src = open(os.path.join(ROOT, "bayeslms_amd", "ops.py")).read()
    for name in ("blm_edit_distance", "blm_nbest_select", "blm_nbest_mbr"):
        assert len(re.findall(r"\b%s\s*\(" % name, header)) == 1, name
        assert name in L.SIGNATURES and name not in L.VALUE_RETURNING
        assert len(re.findall(r"calls\(\)\.%s\(" % name, ops_src)) == 1, name
    assert L.EDIT_MAX_LEN == 1023 and L.NBEST_GRID_MAX == 64 == len(L.NbestGrid().lmwt)
    assert "#define BLM_EDIT_MAX_LEN 1023" in header and "#define BLM_NBEST_GRID_MAX 64" in header


def test_entries_validate_before_any_launch():
    import ctypes as C
    from bayeslms_amd import _lib as L
    lib = L.lib()
    buf = (C.c_int64 * 8)()
    p = C.addressof(buf)
    g = L.NbestGrid()
    g.abi_version, g.G = L.ABI_VERSION, 1
    g.lmwt[0], g.pscale[0] = 1.0, 1.0
    assert lib.blm_edit_distance(p, 4, p, 1, p, p, 0, p, None, None) == L.OK          # P == 0
    assert lib.blm_edit_distance(p, 4, None, 1, p, p, 1, p, None, None) == L.ERR_INVALID
    assert lib.blm_edit_distance(p, -1, p, 1, p, p, 1, p, None, None) == L.ERR_INVALID
    assert lib.blm_edit_distance(None, 4, p, 1, p, p, 1, p, None, None) == L.ERR_INVALID
    assert lib.blm_edit_distance(p, 4, p, 1, p, p, 2 ** 31 - 1, p, None, None) == L.ERR_INVALID
    assert lib.blm_nbest_select(None, None, None, None, None, p, 0, C.byref(g), p, None) == L.OK  # U == 0
    assert lib.blm_nbest_select(None, None, None, None, None, p, -1, C.byref(g), p, None) == L.ERR_INVALID
    assert lib.blm_nbest_select(None, None, None, None, None, p, 1, None, p, None) == L.ERR_INVALID
    assert lib.blm_nbest_mbr(None, None, None, None, None, p, 0, 0, p, p, C.byref(g), None, p, None) == L.OK
    assert lib.blm_nbest_mbr(None, None, None, None, None, p, 1, 1, None, p, C.byref(g), None, p, None) == L.ERR_INVALID
    for field_, value in (("G", 0), ("G", 65), ("lmwt", 0.0), ("lmwt", float("inf")), ("lmwt", float("nan")), ("pscale", -0.5),
                          ("pscale", float("nan"))):
        h = L.NbestGrid()
        C.memmove(C.byref(h), C.byref(g), C.sizeof(g))
        if field_ == "G":
            h.G = value
        else:
            getattr(h, field_)[0] = value
        assert lib.blm_nbest_select(None, None, None, None, None, p, 1, C.byref(h), p, None) == L.ERR_INVALID, (field_, value)
        assert lib.blm_nbest_mbr(None, None, None, None, None, p, 1, 1, p, p, C.byref(h), None, p, None) == L.ERR_INVALID
        assert lib.blm_last_error()
    g.abi_version = L.ABI_VERSION + 1
    assert lib.blm_nbest_select(None, None, None, None, None, p, 1, C.byref(g), p, None) == L.ERR_ABI


def test_grid_struct_layout_matches_the_c_compiler(tmp_path):
    import ctypes as C
    import subprocess
    from bayeslms_amd import _lib as L
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bayeslm.h"\nint main(){printf("%zu %zu %zu %zu\\n", '
                   'sizeof(blm_nbest_grid), offsetof(blm_nbest_grid, lmwt), offsetof(blm_nbest_grid, wip), '
                   'offsetof(blm_nbest_grid, pscale));return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "sz")], text=True).split()]
    G = L.NbestGrid
    assert got == [C.sizeof(G), G.lmwt.offset, G.wip.offset, G.pscale.offset]
