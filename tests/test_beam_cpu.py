"""CPU: the search entry points (csrc/beam.hip: blm_topk_rows, blm_beam_select, blm_sample_rows_filtered) are declared, exported
and bound, and refuse bad arguments on the host before any launch; the generate CLI refuses conflicting flags before it looks
for a device; the numpy reference models that tests/test_gpu_beam.py holds the kernels to are right on hand-written cases."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import beam_reference as REF
from conftest import ROOT

NEW = ("blm_topk_rows", "blm_beam_select", "blm_sample_rows_filtered")
LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from bayeslms_amd import _lib as L
    return L, L.lib()


def test_header_declares_library_exports_and_binding_covers_the_entry_points(lib):
    hdr = open(os.path.join(ROOT, "include", "bayeslm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(blm_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    L, _ = lib
    for name in NEW:
        assert name in declared and name in exported and name in L.SIGNATURES, name
    topk_max = int(re.search(r"#define BLM_TOPK_MAX (\d+)", hdr).group(1))
    assert topk_max >= 64 and topk_max == L.TOPK_MAX
    assert "#define BLM_ABI_VERSION 1u" in hdr


def test_host_side_refusals(lib):
    L, l = lib
    P = 0x10000  # never dereferenced: every call below fails its checks before a launch
    K = L.TOPK_MAX
    bad = [
        l.blm_topk_rows(None, 10, 4, 10, 2, P, P, None), l.blm_topk_rows(P, 10, 4, 10, 2, None, P, None),
        l.blm_topk_rows(P, 10, 4, 10, 2, P, None, None), l.blm_topk_rows(P, 10, -1, 10, 2, P, P, None),
        l.blm_topk_rows(P, 10, 4, -10, 2, P, P, None), l.blm_topk_rows(P, 9, 4, 10, 2, P, P, None),
        l.blm_topk_rows(P, 10, 4, 10, 0, P, P, None), l.blm_topk_rows(P, 10, 4, 10, 11, P, P, None),
        l.blm_topk_rows(P, 1000, 4, 1000, K + 1, P, P, None), l.blm_topk_rows(P, 2 ** 40, 2 ** 30, 10, 2, P, P, None),
        l.blm_beam_select(None, P, P, P, 1, 4, 4, 0, P + 64, P + 128, P, P, None),
        l.blm_beam_select(P, P, P, P, 1, 4, 4, 0, P + 64, P + 128, None, P, None),
        l.blm_beam_select(P, P, P, P, -1, 4, 4, 0, P + 64, P + 128, P, P, None),
        l.blm_beam_select(P, P, P, P, 1, 0, 4, 0, P + 64, P + 128, P, P, None),
        l.blm_beam_select(P, P, P, P, 1, 4, 0, 0, P + 64, P + 128, P, P, None),
        l.blm_beam_select(P, P, P, P, 1, K + 1, K + 1, 0, P + 64, P + 128, P, P, None),
        l.blm_beam_select(P, P, P, P, 1, 4, 4, 0, P, P + 128, P, P, None),  # score_out aliases score
        l.blm_sample_rows_filtered(None, 10, 4, 10, 1.0, 0, 1.0, None, P, None),
        l.blm_sample_rows_filtered(P, 10, -4, 10, 1.0, 0, 1.0, None, P, None),
        l.blm_sample_rows_filtered(P, 10, 4, 10, -1.0, 0, 1.0, None, P, None),
        l.blm_sample_rows_filtered(P, 10, 4, 10, 1.0, -1, 1.0, None, P, None),
        l.blm_sample_rows_filtered(P, 10, 4, 10, 1.0, 0, 0.0, None, P, None),
        l.blm_sample_rows_filtered(P, 10, 4, 10, 1.0, 0, 1.5, None, P, None),
        l.blm_sample_rows_filtered(P, 10, 4, 10, 1.0, 0, float("nan"), None, P, None),
        l.blm_sample_rows_filtered(P, 10, 4, 10, 1.0, 3, 0.5, None, P, None),  # sampling needs rng
    ]
    assert bad == [L.ERR_INVALID] * len(bad), bad
    assert l.blm_topk_rows(P, 1000, 4, 1000, K + 1, P, P, None) == L.ERR_INVALID and b"BLM_TOPK_MAX" in l.blm_last_error()
    assert l.blm_topk_rows(P, 10, 0, 10, 2, P, P, None) == L.OK  # no rows: nothing to do


@pytest.mark.parametrize("flags,word", [(["--beam", "4", "--streams", "2"], "--streams"), (["--beam", "4", "--temperature", "0.5"], "--temperature"),
                                        (["--beam", "4", "--top-k", "3"], "--top-k"), (["--beam", "4", "--top-p", "0.5"], "--top-p"),
                                        (["--beam", "4", "--mc-samples", "2", "--write-uncertainty", "u.txt"], "--write-uncertainty"),
                                        (["--beam", "2", "--nbest", "3"], "--nbest"), (["--nbest", "2"], "--beam"),
                                        (["--top-p", "1.5"], "--top-p"), (["--top-k", "-1"], "--top-k")])
def test_generate_refuses_conflicting_flags_before_it_looks_for_a_device(flags, word):
    """the paths do not exist and no GPU is asked for: the message is about the flags"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "bayeslms_amd.generate", "--model-path", "/nonexistent/m.pt", "--vocabulary",
                        "/nonexistent/w.txt"] + flags, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and word in r.stderr and "MI355X" not in r.stderr and "nonexistent" not in r.stderr, r.stderr[-500:]


def test_beam_search_and_step_topk_check_their_arguments_before_any_launch():
    import torch
    from bayeslms_amd import BayesLMError
    from bayeslms_amd.incremental import IncrementalLM

    class Fake(IncrementalLM):  # the argument checks need no model
        def __init__(self):
            self.vocab, self.max_streams, self.max_len, self.mc_samples = 40, 8, 16, 0
    lm = Fake()
    for kw in (dict(prompts=[], beam=2, max_words=3, eos=0), dict(prompts=[[]], beam=2, max_words=3, eos=0),
               dict(prompts=[[0]], beam=41, max_words=3, eos=0), dict(prompts=[[0]], beam=0, max_words=3, eos=0),
               dict(prompts=[[0]] * 3, beam=4, max_words=3, eos=0), dict(prompts=[[0] * 10], beam=2, max_words=7, eos=0),
               dict(prompts=[[0]], beam=2, max_words=0, eos=0), dict(prompts=[[0]], beam=2, max_words=3, eos=40)):
        with pytest.raises(BayesLMError):
            lm.beam_search(**kw)
    lm.vocab = 1000
    with pytest.raises(BayesLMError, match="BLM_TOPK_MAX"):
        lm.beam_search([[0]], 257, 3, 0)
    with pytest.raises(BayesLMError):
        lm.step_topk(None, torch.zeros(1, dtype=torch.int64), 0)
    with pytest.raises(BayesLMError):
        lm.step_topk(None, torch.zeros(1, dtype=torch.int64), 257)


# --------------------------------------------------------------------------------------------------- the reference models
def test_reference_row_order_on_ties_infinities_and_nan():
    inf, nan = np.inf, np.nan
    x = np.array([1.0, nan, -inf, 3.0, 1.0, inf, -0.0, 0.0, 3.0, -inf, nan], dtype=np.float32)
    assert list(REF.row_order(x)) == [5, 3, 8, 0, 4, 6, 7, 2, 9, 1, 10]
    vals, ids = REF.topk_rows(np.stack([x, x[::-1]]), 4)
    assert ids.tolist() == [[5, 3, 8, 0], [5, 2, 7, 6]] and vals[0].tolist() == [inf, 3.0, 3.0, 1.0]
    assert list(REF.row_order(np.full(5, nan, np.float32))) == [0, 1, 2, 3, 4]
    assert list(REF.row_order(np.full(4, 2.5, np.float32))) == [0, 1, 2, 3]


def test_reference_beam_select_on_hand_written_cases():
    inf = np.inf
    # one group of 3 beams, k = 3; beam 1 is finished; beam 2 has not started (-inf)
    cv = np.array([[-1.0, -2.0, -3.0], [-0.5, -0.6, -0.7], [-0.1, -0.2, -0.3]], np.float32)
    ci = np.array([[7, 8, 9], [4, 5, 6], [1, 2, 3]], np.int64)
    s, f, p, t = REF.beam_select(cv, ci, np.array([-1.0, -2.5, -inf], np.float32), np.array([0, 1, 0], np.uint8), 3, eos=9)
    # candidates: (0,0) -2 tok 7; (0,1) -3 tok 8; (0,2) -4 tok 9; beam 1 itself -2.5 tok eos; beam 2: -inf x 3
    assert s.tolist() == [-2.0, -2.5, -3.0] and p.tolist() == [0, 1, 0] and t.tolist() == [7, 9, 8] and f.tolist() == [0, 1, 0]
    # ties resolve to the lowest flat candidate index; a token equal to eos finishes the beam; two groups, parents stay global
    cv = np.array([[-1.0, -1.0], [-1.0, -1.0]] * 2, np.float32)
    ci = np.array([[3, 5], [5, 2]] * 2, np.int64)
    s, f, p, t = REF.beam_select(cv, ci, np.zeros(4, np.float32), np.zeros(4, np.uint8), 2, eos=5)
    assert p.tolist() == [0, 0, 2, 2] and t.tolist() == [3, 5, 3, 5] and f.tolist() == [0, 1, 0, 1] and s.tolist() == [-1.0] * 4
    # the start state: only beam 0 is live, so the first step does not pick B copies of one word; NaN scores come last
    cv = np.array([[-0.1, -0.2], [-0.1, -0.2]], np.float32)
    s, f, p, t = REF.beam_select(cv, np.array([[1, 2], [1, 2]]), np.array([0.0, -inf], np.float32), np.zeros(2, np.uint8), 2, eos=0)
    assert p.tolist() == [0, 0] and t.tolist() == [1, 2]
    s, f, p, t = REF.beam_select(cv, np.array([[1, 2], [1, 2]]), np.array([np.nan, -5.0], np.float32), np.zeros(2, np.uint8), 2, eos=0)
    assert p.tolist() == [1, 1] and s.tolist() == [np.float32(-5.0) + np.float32(-0.1), np.float32(-5.0) + np.float32(-0.2)]
    # every beam finished: each keeps itself, ordered by score
    s, f, p, t = REF.beam_select(cv, np.array([[1, 2], [1, 2]]), np.array([-3.0, -1.0], np.float32), np.ones(2, np.uint8), 2, eos=0)
    assert p.tolist() == [1, 0] and t.tolist() == [0, 0] and s.tolist() == [-1.0, -3.0] and f.tolist() == [1, 1]


def test_reference_allowed_set():
    p = np.array([0.1, 0.4, 0.05, 0.25, 0.2])
    x = np.log(p)
    m, before, after = REF.allowed_set(x, 1.0, 0, 0.7)
    assert m.tolist() == [False, True, False, True, True] and abs(before - 0.65) < 1e-12 and abs(after - 0.85) < 1e-12
    assert REF.allowed_set(x, 1.0, 2, 1.0)[0].tolist() == [False, True, False, True, False]
    assert REF.allowed_set(x, 1.0, 2, 0.3)[0].tolist() == [False, True, False, False, False]  # at least one entry
    assert REF.allowed_set(x, 1.0, 0, 1.0)[0].all()
    # ties: the lower index is inside first; -inf and NaN entries carry no mass and come last
    x = np.array([0.0, 0.0, -np.inf, np.nan, 0.0])
    assert REF.allowed_set(x, 1.0, 2, 1.0)[0].tolist() == [True, True, False, False, False]
    assert REF.allowed_set(x, 1.0, 0, 0.5)[0].tolist() == [True, True, False, False, False]
    # temperature sharpens q: at 0.5 the same top_p needs fewer words
    x = np.log(np.array([0.5, 0.3, 0.2]))
    assert REF.allowed_set(x, 1.0, 0, 0.6)[0].sum() == 2 and REF.allowed_set(x, 0.5, 0, 0.6)[0].sum() == 1
