"""CPU: blm_beam_select_pool (csrc/beam.hip) is declared, exported and bound, and refuses bad arguments on the host before any
launch; the generate CLI refuses the pool's flags without --finished-pool before it looks for a device; the numpy model that
tests/test_gpu_beam_pool.py holds the kernel to (tests/beam_pool_reference.py) is right on hand-written cases, and its early
stop returns the pool of the search run to the end."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import beam_pool_reference as REF
from conftest import ROOT

LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")
F = np.float32
inf = np.inf


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from bayeslms_amd import _lib as L
    return L, L.lib()


def test_header_declares_library_exports_and_binding_covers_the_entry_point(lib):
    hdr = open(os.path.join(ROOT, "include", "bayeslm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(blm_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L, _ = lib
    assert "blm_beam_select_pool" in declared and "blm_beam_select_pool" in exported and "blm_beam_select_pool" in L.SIGNATURES
    assert "typedef struct blm_beam_pool" in hdr and "#define BLM_ABI_VERSION 1u" in hdr  # a new symbol: no new ABI version
    # the ctypes mirror of blm_beam_pool: two 32-bit words, then eight pointers
    assert C.sizeof(L.BeamPoolArgs) == 8 + 8 * C.sizeof(C.c_void_p) and L.BeamPoolArgs.norm.offset == 8


def _call(L, l, **kw):
    """a call that passes every check (and would launch) unless ``kw`` breaks it; the addresses are never dereferenced"""
    A = 0x10000
    a = dict(cand_vals=A, cand_ids=A, score=A, live=A, G=2, B=4, k=8, V=50, eos=0, step=0, len=1, min_len=0, inv_norm=1.0,
             inv_norm_max=0.5, flush=0, P=8, pool_null=None, pool_abi=L.ABI_VERSION, score_out=A + 64, live_out=A + 128, parent=A,
             token=A, done_out=A, all_done=A, pool=True)
    a.update(kw)
    pa = L.BeamPoolArgs(a["pool_abi"], a["P"], *[None if n == a["pool_null"] else (A + 4 if n == a.get("pool_odd") else A)
                                                for n in ("norm", "raw", "len", "step", "parent", "finished", "count", "inserted")])
    return l.blm_beam_select_pool(a["cand_vals"], a["cand_ids"], a["score"], a["live"], a["G"], a["B"], a["k"], a["V"], a["eos"], a["step"],
                                  a["len"], a["min_len"], a["inv_norm"], a["inv_norm_max"], a["flush"], C.byref(pa) if a["pool"] else None,
                                  a["score_out"], a["live_out"], a["parent"], a["token"], a["done_out"], a["all_done"], None)


def test_host_side_refusals(lib):
    L, l = lib
    A = 0x10000
    bad = [dict(k=7),                       # k < min(2 B, V) = 8
           dict(V=5, k=4),                  # k < V < 2 B
           dict(B=129, k=256, V=1000),      # 2 B > BLM_TOPK_MAX
           dict(P=0), dict(P=257), dict(P=-1),
           dict(score_out=None), dict(live_out=None), dict(parent=None), dict(token=None), dict(done_out=None), dict(all_done=None),
           dict(cand_vals=None), dict(cand_ids=None), dict(score=None), dict(live=None), dict(pool=False),
           dict(pool_null="norm"), dict(pool_null="parent"), dict(pool_null="count"), dict(pool_null="inserted"),
           dict(score_out=A), dict(live_out=A),  # the state after the step aliases the state before it
           dict(G=-1), dict(B=0), dict(k=0), dict(V=0), dict(G=2 ** 30 + 1), dict(len=0), dict(step=-1), dict(min_len=-1),
           dict(inv_norm=-1.0), dict(inv_norm=float("nan")), dict(inv_norm=float("inf")), dict(inv_norm_max=2.0),
           dict(inv_norm_max=float("nan")),
           dict(cand_vals=A + 2), dict(cand_ids=A + 4), dict(parent=A + 4), dict(token=A + 4), dict(score_out=A + 66),
           dict(pool_odd="parent"), dict(pool_odd="inserted")]
    got = [_call(L, l, **kw) for kw in bad]
    assert got == [L.ERR_INVALID] * len(bad), [(kw, rc) for kw, rc in zip(bad, got) if rc != L.ERR_INVALID]
    assert _call(L, l, k=7) == L.ERR_INVALID and b"min(2 B, V)" in l.blm_last_error()
    assert _call(L, l, B=129, k=256, V=1000) == L.ERR_INVALID and b"BLM_TOPK_MAX" in l.blm_last_error()
    assert _call(L, l, pool_abi=L.ABI_VERSION + 1) == L.ERR_ABI
    assert _call(L, l, G=0) == L.OK                 # no groups: nothing to do
    assert _call(L, l, V=5, k=5, G=0) == L.OK       # k = V < 2 B is the whole row
    with pytest.raises(L.BayesLMError, match="blm_beam_select_pool"):  # the checked view raises
        L.calls().blm_beam_select_pool(*([None] * 4), 1, 1, 2, 2, 0, 0, 1, 0, 1.0, 1.0, 0, None, *([None] * 7))


@pytest.mark.parametrize("flags,word", [(["--beam", "4", "--min-words", "2"], "--finished-pool"),
                                        (["--beam", "2", "--nbest", "3"], "--nbest"),
                                        (["--min-words", "2"], "--beam"), (["--finished-pool", "4"], "--beam"),
                                        (["--beam", "2", "--finished-pool", "4", "--nbest", "5"], "--nbest"),
                                        (["--beam", "2", "--finished-pool", "300"], "--finished-pool"),
                                        (["--beam", "2", "--finished-pool", "4", "--length-penalty", "-1"], "--length-penalty")])
def test_generate_refuses_the_flags_before_it_looks_for_a_device(flags, word):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "bayeslms_amd.generate", "--model-path", "/nonexistent/m.pt", "--vocabulary",
                        "/nonexistent/w.txt"] + flags, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and word in r.stderr and "MI355X" not in r.stderr and "nonexistent" not in r.stderr, r.stderr[-500:]


def test_beam_search_pool_checks_its_arguments_before_any_launch():
    from bayeslms_amd import BayesLMError
    from bayeslms_amd.incremental import IncrementalLM

    class Fake(IncrementalLM):  # the argument checks need no model
        def __init__(self):
            self.vocab, self.max_streams, self.max_len, self.mc_samples = 40, 8, 16, 0
    lm = Fake()
    ok = dict(prompts=[[0]], beam=2, max_words=3, eos=0)
    for kw in (dict(prompts=[]), dict(prompts=[[]]), dict(beam=0), dict(beam=129), dict(pool=0), dict(pool=257), dict(max_words=0),
               dict(min_words=-1), dict(sync_every=-1), dict(length_penalty=-0.5), dict(length_penalty=float("nan")),
               dict(prompts=[[0]] * 5), dict(prompts=[[0] * 14]), dict(eos=40)):
        with pytest.raises(BayesLMError, match="beam_search_pool"):
            lm.beam_search_pool(**dict(ok, **kw))


# ------------------------------------------------------------------------------------------------------- the numpy model
CV = np.array([[-0.1, -0.5, -1.0, -3.0], [-0.05, -0.2, -2.0, -4.0]], F)
CI = np.array([[5, 9, 6, 7], [9, 1, 2, 3]], np.int64)


def _step(pool, min_len=0, flush=0, score=(0.0, -1.0), live=(1, 1)):
    """2 beams, k = 4, eos 9, length 2 under a = 1: the sums are -0.1 (5), -0.5 (eos), -1.0 (6), -1.05 (eos), -1.2 (1), ..."""
    return REF.select_pool(CV, CI, np.array(score, F), np.array(live, np.uint8), 2, 9, 1, 2, min_len, REF.inv_norm(2, 1.0),
                           REF.inv_norm(4, 1.0), flush, pool)


def test_model_pools_an_eos_of_rank_below_B_and_drops_one_beyond():
    pool = REF.new_pool(1, 3)
    s, l, p, t, done, all_done = _step(pool)
    # rank 1 (eos of beam 0) is pooled; rank 3 (eos of beam 1, -1.05) is inside the walk but beyond rank B: dropped
    assert pool["count"].tolist() == [1] and pool["inserted"].tolist() == [1]
    assert (pool["norm"][0, 0], pool["raw"][0, 0]) == (F(-0.25), F(-0.5))
    assert (pool["len"][0, 0], pool["step"][0, 0], pool["parent"][0, 0], pool["finished"][0, 0]) == (2, 1, 0, 1)
    assert s.tolist() == [F(-0.1), F(-1.0)] and l.tolist() == [1, 1] and p.tolist() == [0, 0] and t.tolist() == [5, 6]
    assert done.tolist() == [0] and all_done == 0
    # a dead beam offers nothing: beam 1 alone -> its eos is rank 0
    pool = REF.new_pool(1, 3)
    s, l, p, t, _, _ = _step(pool, live=(0, 1))
    assert pool["raw"][0, 0] == F(-1.0) + F(-0.05) and pool["parent"][0, 0] == 1 and t.tolist() == [1, 2] and p.tolist() == [1, 1]


def test_model_min_len_suppresses_an_eos_and_flush_pools_the_live_beams():
    pool = REF.new_pool(1, 3)
    s, l, p, t, done, _ = _step(pool, min_len=3)
    assert pool["count"].tolist() == [0] and t.tolist() == [5, 6] and s.tolist() == [F(-0.1), F(-1.0)]
    s, l, p, t, done, all_done = _step(pool, min_len=3, flush=1)
    assert pool["count"].tolist() == [2] and pool["finished"][0, :2].tolist() == [0, 0] and pool["parent"][0, :2].tolist() == [0, 1]
    assert pool["norm"][0, :2].tolist() == [F(-0.05), F(-0.5)] and pool["len"][0, :2].tolist() == [2, 2]
    assert l.tolist() == [0, 0] and s.tolist() == [-inf, -inf] and t.tolist() == [5, 6] and done.tolist() == [1] and all_done == 1


def test_model_pool_replaces_only_on_strict_precedence_and_ties_keep_insertion_order():
    pool = REF.new_pool(1, 2)
    for i, norm in enumerate((-1.0, -1.0)):
        REF.offer(pool, 0, (F(norm), F(norm), 1, 0, i, 1))
    assert pool["parent"][0].tolist() == [0, 1]  # a tie: the earlier entry stays in front
    REF.offer(pool, 0, (F(-1.0), F(-1.0), 1, 0, 2, 1))  # full, ties with the last: not inserted
    assert pool["parent"][0].tolist() == [0, 1] and pool["inserted"].tolist() == [3] and pool["count"].tolist() == [2]
    REF.offer(pool, 0, (F(-0.5), F(-0.5), 1, 0, 3, 1))
    assert pool["parent"][0].tolist() == [3, 0] and pool["norm"][0].tolist() == [-0.5, -1.0]
    REF.offer(pool, 0, (F(-0.5), F(-0.5), 1, 0, 4, 1))  # precedes the last, ties with the first: behind it
    assert pool["parent"][0].tolist() == [3, 4]
    REF.offer(pool, 0, (F(np.nan), F(np.nan), 1, 0, 5, 1))  # NaN precedes nothing
    assert pool["parent"][0].tolist() == [3, 4] and pool["inserted"].tolist() == [6]


def test_model_gives_dead_slots_with_fewer_than_B_candidates():
    pool = REF.new_pool(2, 2)
    cv = np.array([[-0.1, -inf]] * 3 + [[np.nan, np.nan]] * 3, F)
    ci = np.array([[1, 0]] * 6, np.int64)
    s, l, p, t, done, all_done = REF.select_pool(cv, ci, np.zeros(6, F), np.array([1, 0, 0, 1, 1, 1], np.uint8), 3, 0, 0, 1, 0, 1.0, 1.0, 0,
                                                 pool)
    assert s.tolist() == [F(-0.1), -inf, -inf, -inf, -inf, -inf] and l.tolist() == [1, 0, 0, 0, 0, 0]
    assert p.tolist() == [0, 1, 2, 3, 4, 5] and t.tolist() == [1, 0, 0, 0, 0, 0]
    assert done.tolist() == [0, 1] and all_done == 0 and pool["count"].tolist() == [0, 0]  # all-NaN rows: no beam is left


def test_model_stopping_bound_and_the_tie_that_does_not_stop():
    def run(best):
        pool = REF.new_pool(1, 1)
        REF.offer(pool, 0, (F(-1.0), F(-2.0), 2, 0, 0, 1))
        cv, ci = np.array([[best, -9.0]], F), np.array([[3, 4]], np.int64)
        return REF.select_pool(cv, ci, np.zeros(1, F), np.ones(1, np.uint8), 1, 0, 1, 2, 0, 0.5, 0.5, 0, pool), pool
    (s, l, p, t, done, _), pool = run(-2.0)  # bound -2 * 0.5 = -1 ties with the pool's last norm: the group goes on
    assert done.tolist() == [0] and l.tolist() == [1] and s.tolist() == [-2.0]
    (s, l, p, t, done, all_done), pool = run(-2.5)  # bound -1.25 is strictly below it: nothing alive can enter the pool
    assert done.tolist() == [1] and all_done == 1 and l.tolist() == [0] and s.tolist() == [-inf] and t.tolist() == [3]
    (s, l, p, t, done, _), pool = run(-1.0)  # the bound is above it
    assert done.tolist() == [0]
    # a pool that is not full never stops a group
    pool = REF.new_pool(1, 2)
    REF.offer(pool, 0, (F(-0.1), F(-0.2), 2, 0, 0, 1))
    out = REF.select_pool(np.array([[-50.0, -60.0]], F), np.array([[3, 4]], np.int64), np.zeros(1, F), np.ones(1, np.uint8), 1, 0, 1, 2, 0,
                          0.5, 0.5, 0, pool)
    assert out[4].tolist() == [0]


def _markov(V, seed, eos_boost):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((V, V)) * 1.5
    x[:, 0] += eos_boost
    x = x - np.log(np.exp(x).sum(1, keepdims=True))
    return x.astype(F)


@pytest.mark.parametrize("a", [0.0, 0.7, 1.5])
def test_model_early_stop_returns_the_pool_of_the_search_run_to_the_end(a):
    stopped = 0
    for seed, (G, B, P, W, min_len) in enumerate([(1, 1, 1, 12, 0), (2, 2, 3, 12, 0), (3, 4, 2, 10, 3), (2, 3, 8, 12, 0), (1, 4, 4, 8, 2),
                                                  (2, 2, 1, 16, 0)]):
        table = _markov(7, 10 * seed + int(a * 10), 1.0)
        starts = np.random.default_rng(seed).integers(1, 7, size=G)
        first = np.repeat(table[starts], B, axis=0)
        res = []
        for stop in (True, False):
            pool, PA, TK = REF.search(first, lambda parent, token: table[token], G, B, W, 0, P, a, min_len, stop)
            res.append((REF.hypotheses(pool, PA, TK, 0), pool["count"].tolist(), PA.shape[0]))
        assert res[0][0] == res[1][0] and res[0][1] == res[1][1], (seed, a)
        assert res[1][2] == W
        stopped += res[0][2] < W
        for hyps in res[0][0]:
            for toks, raw, norm, length, fin in hyps:
                assert length == len(toks) >= (min_len if fin else 0) and (toks[-1] == 0) == fin and 0 not in toks[:-1]
                assert norm == raw * REF.inv_norm(length, a)
    # the bound r / W ** a weakens as a grows: under a = 1.5 these walks run to the end, under 0 and 0.7 most of them stop early
    assert stopped >= (2 if a < 1.0 else 0)
