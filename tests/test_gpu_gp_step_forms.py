"""GPU: the GP and GPNN2 epilogues of the fused LSTM step kernels (csrc/lstm_step.hip) in EVERY kernel form the host can
pick, against the float64 reference of tests/gp_recurrence_reference.py (pinned to the oracle by
tests/test_gp_recurrence_reference_cpu.py).  The host picks a form from H and B alone:

  forward  (blm_lstm_step_fwd_gp): nchunk = (H/8 + 31)/32; odd -> <1,4>; 2 -> <2,4,false>; even >= 4 -> software
           pipelined, whole chunks when H % 256 == 0, else the K-tail form; one workgroup row per 32 batch rows
  backward and the skinny products (launch_step_bwd): nchunk = (G/16 + 31)/32 with G = 4H in the recurrence (G = H or
           GP = 192 in the GPNN2 products); odd -> <1>; 2 -> <2>; even >= 4 -> pipelined, whole chunks when G % 512 == 0;
           one workgroup row per 16 batch rows

    H   | forward form (nchunk)            | backward form (nchunk, G = 4H)
   -----+----------------------------------+--------------------------------
     64 | 1                                | 1
    192 | 1                                | 2 (<2>)
    320 | 2 (<2,4,false>, K tail)          | 3
    448 | 2                                | 4, pipelined with tail
    512 | 2, whole chunks                  | 4, pipelined whole chunks
    576 | 3                                | 5
    832 | 4, pipelined with tail           | 7
   1024 | 4, pipelined whole chunks        | 8, pipelined whole chunks
   extra, ovr <= 4 (ovr 5 needs H % 64 == 0):
     96 | 1                                | 1
    160 | 1                                | 2
    288 | 2 (tail 4)                       | 3
    416 | 2                                | 4, pipelined with tail
    800 | 4, pipelined with tail           | 7

(`test_the_table_is_the_dispatch` recomputes the nchunk columns with the host's arithmetic.)  B = 33 is one full 32-row
forward tile plus a 1-row tile, and two full 16-row backward tiles plus a 1-row tile.  "lstm_pipe" = 0 turns the pipelined
forms at H = 1024 into the plain ring forms <2,4> / <2>, "lstm_tail" = 1 into the general pipelined form on whole chunks.

Every mixture coefficient row is non-zero here, the GELU row included, and the GPNN2 cases run ``acts`` 15 next to the
models' 7.  Magnitudes are ordinary (tests/gp_recurrence_reference.py make_*_case); the subject is shapes and forms.

Bounds: 1e-5 for y / hT / cT, 5e-5 for gradients, relative to the reference tensor's largest magnitude -- what
test_lstm_layer_fused_step_matches_oracle asks of the same kernels in plain mode.  The float32 torch composition of the
reference differs from float64 by at most 3.7e-6 on these inputs, so the reference leaves a factor of 3 to 13.  The
gradient of xw, and in mode 4 of coef4 / rbias, is also held to the bound per gate block: the four gates' gradients differ
by an order of magnitude and a wrong block must not hide under another's maximum.  profiles/gp_step_forms_rel.txt holds
the measured worst case per (op, mode, output)."""
import functools
import os

import pytest
import torch

import gp_recurrence_reference as R

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = 1e-5, 5e-5
T = 3
MAIN_H = (64, 192, 320, 448, 512, 576, 832, 1024)
EXTRA_H = (96, 160, 288, 416, 800)
WORST = {}  # (op, mode, output) -> largest rel seen in this session


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def option():
    """set(name, value) for the duration of a test; every option goes back to what it was."""
    from bayeslms_amd import ops
    saved = {}

    def setter(name, value):
        saved.setdefault(name, ops.get_option(name))
        ops.set_option(name, value)
    yield setter
    for k, v in saved.items():
        ops.set_option(k, v)


@pytest.fixture(scope="module", autouse=True)
def _rel_table():
    """GP_STEP_FORMS_REL_OUT=<file>: the worst rel per (op, mode, output) of this session goes there (profiles/gp_step_forms_rel.txt)."""
    yield
    path = os.environ.get("GP_STEP_FORMS_REL_OUT")
    if path and WORST:
        with open(path, "w") as f:
            f.write("# op  mode  output  worst_rel  (bound %.0e outputs, %.0e gradients)\n" % (OUT_TOL, GRAD_TOL))
            for (op, mode, name), v in sorted(WORST.items()):
                f.write("%-22s %-10s %-12s %.3e\n" % (op, mode, name, v))


def _blocks(name, got, want, nblock):
    """(label, got, want) of the whole tensor and of each of ``nblock`` blocks of its last dimension."""
    out = [(name, got, want)]
    if nblock > 1:
        for g, (a, b) in enumerate(zip(got.chunk(nblock, -1), want.chunk(nblock, -1))):
            out.append(("%s[g%d]" % (name, g), a, b))
    return out


def _compare(op, mode, got, ref, blocked=()):
    """Every entry of ``ref`` (outputs y / hT / cT / out, gradients d*) against ``got`` under the bounds; all figures are
    printed and recorded before anything is asserted."""
    bad = []
    for k, want in ref.items():
        have = got.get(k)
        if want is None:
            assert have is None, k
            continue
        assert have is not None and have.shape == want.shape, k
        for label, a, b in _blocks(k, have, want, 4 if k in blocked else 1):
            r = rel(a, b)
            tol = GRAD_TOL if k.startswith("d") else OUT_TOL
            WORST[(op, mode, label)] = max(WORST.get((op, mode, label), 0.0), r)
            print("rel %s mode=%s %s %.3e" % (op, mode, label, r))
            if not r < tol:
                bad.append("%s %.3e >= %.0e" % (label, r, tol))
    assert not bad, "; ".join(bad)


def _vacuous_guard(got, wrong):
    """the kernel's results are far (100x the bound) from a reference with a deliberate mistake: the comparison can fail."""
    for k, w in wrong.items():
        if w is not None:
            assert rel(got[k], w) > 100 * (GRAD_TOL if k.startswith("d") else OUT_TOL), k


def _to_dev(case, names, dev):
    return {k: (None if case[k] is None else case[k].float().to(dev).requires_grad_(True)) for k in names}


def _results(outs, names, ups, leaves, dev):
    loss = sum((o * u.float().to(dev)).sum() for o, u in zip(outs, ups))
    loss.backward()
    torch.cuda.synchronize()
    res = {k: o.detach() for k, o in zip(names, outs)}
    res.update({"d" + k: v.grad for k, v in leaves.items() if v is not None})
    return res


# ------------------------------------------------------------------ ops.lstm_recurrent_gp
def _gp_ref_new(H, B, ovr):
    case = R.make_gp_case(T, B, H, ovr, R.gp_seed(H, B, ovr))
    return case, R.eval_gp(case)


_gp_ref_shared = functools.lru_cache(maxsize=None)(_gp_ref_new)


def _gp_ref(H, B, ovr):
    """the float64 reference of a case, computed once for the cases that the optional-form tests run again"""
    return (_gp_ref_shared if (B == 33 and H in (512, 1024)) else _gp_ref_new)(H, B, ovr)


def _run_gp(dev, H, B, ovr):
    from bayeslms_amd import ops
    case, ref = _gp_ref(H, B, ovr)
    a = _to_dev(case, R.GP_INPUTS, dev)
    outs = ops.lstm_recurrent_gp(a["xw"], a["h0"], a["c0"], a["w_rec"], a["coef4"], ovr, a["rbias"], a["w_cell"])
    got = _results(outs, ("y", "hT", "cT"), (case["gy"], case["gh"], case["gc"]), a, dev)
    return case, ref, got


GP_BLOCKED = {4: ("dxw", "dcoef4", "drbias")}


def _check_gp(dev, H, B, ovr, tag):
    case, ref, got = _run_gp(dev, H, B, ovr)
    _compare("lstm_recurrent_gp" + tag, "ovr%d" % ovr, got, ref, GP_BLOCKED.get(ovr, ("dxw",)))
    return case, got


GP_FORMS = [(H, ovr) for H in MAIN_H for ovr in (-1, 0, 1, 2, 3, 4, 5)] + [(H, ovr) for H in EXTRA_H for ovr in (-1, 0, 1, 2, 3, 4)]


def test_the_table_is_the_dispatch():
    """the nchunk columns of the module docstring by the host's own arithmetic (blm_lstm_step_fwd_gp, launch_step_bwd), and:
    every form reachable with default options is hit by every ovr (ovr 5 on the main rows alone)."""
    fwd = {H: (H // 8 + 31) // 32 for H in MAIN_H + EXTRA_H}
    bwd = {H: (4 * H // 16 + 31) // 32 for H in MAIN_H + EXTRA_H}
    assert [fwd[H] for H in MAIN_H] == [1, 1, 2, 2, 2, 3, 4, 4] and [fwd[H] for H in EXTRA_H] == [1, 1, 2, 2, 4]
    assert [bwd[H] for H in MAIN_H] == [1, 2, 3, 4, 4, 5, 7, 8] and [bwd[H] for H in EXTRA_H] == [1, 2, 3, 4, 7]

    def form(n, whole):
        return "odd" if n % 2 else ("two" if n == 2 else ("pipe-whole" if whole else "pipe-tail"))
    for hs in (MAIN_H, MAIN_H + EXTRA_H):
        assert {form(fwd[H], H % 256 == 0) for H in hs} == {"odd", "two", "pipe-whole", "pipe-tail"}
        assert {form(bwd[H], 4 * H % 512 == 0) for H in hs} == {"odd", "two", "pipe-whole", "pipe-tail"}
    assert all(H % 64 == 0 for H in MAIN_H)
    # the GPNN2 feature product contracts over H: one chunk up to 512, two from 576
    assert [(H // 16 + 31) // 32 for H in GPNN2_H] == [1, 1, 1, 1, 1, 2, 2]


@pytest.mark.parametrize("H,ovr", GP_FORMS)
def test_gp_recurrence_in_every_kernel_form(dev, H, ovr):
    """(a) B = 33: a full and a one-row forward tile, two full and a one-row backward tile, in each form of the table."""
    case, got = _check_gp(dev, H, 33, ovr, "")
    if (ovr, H) == (2, 320):
        _vacuous_guard(got, R.eval_gp(case, coef4=case["coef4"][[1, 0, 2, 3]]))  # tanh and sigmoid rows swapped
    if (ovr, H) == (4, 512):
        _vacuous_guard(got, R.eval_gp(case, rbias=case["rbias"].roll(H)))  # rbias off by one gate block


@pytest.mark.parametrize("B", [1, 15, 16, 17, 32, 50, 64])
@pytest.mark.parametrize("ovr", [-1, 0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("H", [64, 320])
def test_gp_recurrence_at_the_batch_tile_edges(dev, H, ovr, B):
    """(b) the edges of the 32-row forward and the 16-row backward tiling; B = 1 with a GP mode has no tiny-batch kernel to
    take (blm_lstm_step_fwd_gp keeps ovr >= 0 on the matrix-core kernel) and must agree like any other batch."""
    _check_gp(dev, H, B, ovr, "")


@pytest.mark.parametrize("H", [512, 1024])
@pytest.mark.parametrize("ovr", [-1, 0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("name,value", [("lstm_pipe", 0), ("lstm_tail", 1)])
def test_gp_recurrence_in_the_optional_forms(dev, option, name, value, ovr, H):
    """(c) "lstm_pipe" 0: the un-pipelined ring forms <2,4> (H = 1024 forward) / <2> (both H backward) where the default
    pipelines; "lstm_tail" 1: the general pipelined form on whole chunks (H = 1024 forward, both H backward).  Against
    float64, not against the default form."""
    option(name, value)
    _check_gp(dev, H, 33, ovr, " %s=%d" % (name, value))


# ------------------------------------------------------------------ ops.lstm_recurrent_gpnn2
GPNN2_H = (64, 192, 320, 448, 512, 576, 1024)
GPNN2_MODES = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (2, 0)]


def _gpnn2_ref(H, B, M, mode, gate, acts, with_eps):
    case = R.make_gpnn2_case(T, B, H, M, mode, gate, acts, R.gpnn2_seed(H, B, M, mode, gate, acts))
    return case, R.eval_gpnn2(case, use_eps=with_eps)


def _check_gpnn2(dev, H, B, M, mode, gate, acts, with_eps=True):
    from bayeslms_amd import ops
    case, ref = _gpnn2_ref(H, B, M, mode, gate, acts, with_eps)
    a = _to_dev(case, R.GPNN2_INPUTS, dev)
    noises = [ops.NoiseSpec(eps=e.float().to(dev)) for e in case["eps"]] if with_eps else None
    outs = ops.lstm_recurrent_gpnn2(a["xw"], a["h0"], a["c0"], a["w_hh"], a["coef_w"], a["coef_b"], a["fmean"], a["flgstd"],
                                    noises, gate, acts, mode)
    got = _results(outs, ("y", "hT", "cT"), (case["gy"], case["gh"], case["gc"]), a, dev)
    _compare("lstm_recurrent_gpnn2", "m%dg%d" % (mode, gate) if mode == 0 else "m%d" % mode, got, ref, ("dxw",))
    return case, got


@pytest.mark.parametrize("acts", [7, 15])
@pytest.mark.parametrize("mode,gate", GPNN2_MODES)
@pytest.mark.parametrize("H", GPNN2_H)
def test_gpnn2_recurrence_in_every_kernel_form(dev, H, mode, gate, acts):
    """(d) M = 150, B = 33, fresh injected frequencies at every step: the feature product (contraction H) runs one chunk up
    to H = 512 and two from 576, the 4H products follow the backward column of the table, the GP = 192 products one chunk."""
    case, got = _check_gpnn2(dev, H, 33, 150, mode, gate, acts)
    if (mode, gate, H, acts) == (0, 0, 576, 15):
        _vacuous_guard(got, R.eval_gpnn2(case, acts=7))  # the GELU bit dropped


@pytest.mark.parametrize("B", [1, 15, 16, 17])
@pytest.mark.parametrize("mode,gate", GPNN2_MODES)
@pytest.mark.parametrize("H", [64, 576])
def test_gpnn2_recurrence_at_the_batch_tile_edges(dev, H, mode, gate, B):
    _check_gpnn2(dev, H, B, 150, mode, gate, 15)


@pytest.mark.parametrize("M,mode,gate", [(37, 0, 2), (159, 2, 0)])
def test_gpnn2_recurrence_pads_the_feature_columns(dev, M, mode, gate):
    """the zero rows / columns between M, MP = 160 and GP = 192: M far below MP, and M + 1 (the bias column) == MP"""
    _check_gpnn2(dev, 192, 33, M, mode, gate, 15)


@pytest.mark.parametrize("acts,mode,gate", [(0, 0, 3), (8, 1, 0)])
def test_gpnn2_recurrence_with_no_activation_and_gelu_alone(dev, acts, mode, gate):
    _check_gpnn2(dev, 192, 33, 150, mode, gate, acts)


def test_gpnn2_recurrence_with_mean_frequencies(dev):
    """``noises`` None: F_t = fmean at every step, no gradient for flgstd"""
    _check_gpnn2(dev, 192, 33, 150, 0, 1, 15, with_eps=False)


# ------------------------------------------------------------------ ops.gpnn2_steps
def _steps_ref(Tn, B, E, NO, acts):
    case = R.make_steps_case(Tn, B, E, NO, 150, acts, 1000 * E + 10 * B + NO + acts + Tn)
    return case, R.eval_steps(case)


@pytest.mark.parametrize("acts", [7, 15])
@pytest.mark.parametrize("Tn,B", [(1, 1), (1, 17), (3, 33)])
@pytest.mark.parametrize("NO", [128, 256])
@pytest.mark.parametrize("E", [64, 192, 576])
def test_gpnn2_steps_match_float64(dev, E, NO, Tn, B, acts):
    """(e) the batched GPNN2 of a whole window: per-step feature products (contraction E), batched coefficient product"""
    from bayeslms_amd import ops
    case, ref = _steps_ref(Tn, B, E, NO, acts)
    a = _to_dev(case, R.STEPS_INPUTS, dev)
    noises = [ops.NoiseSpec(eps=e.float().to(dev)) for e in case["eps"]]
    out = ops.gpnn2_steps(a["x"], a["coef_w"], a["coef_b"], a["fmean"], a["flgstd"], noises, acts)
    got = _results((out,), ("out",), (case["gout"],), a, dev)
    _compare("gpnn2_steps", "acts%d" % acts, got, ref)


# ------------------------------------------------------------------ refusals: host checks, no launch
def test_gp_steps_refuse_bad_modes_and_missing_operands(dev):
    from bayeslms_amd import _lib
    from bayeslms_amd._lib import ptr, stream, ERR_INVALID
    lib = _lib.lib()
    B, H = 4, 64
    SENT = 7.5
    full = lambda *s: torch.full(s, SENT, device=dev)  # noqa: E731
    xw, w, hp, cp = full(B, 4 * H), full(4 * H, H), full(B, H), full(B, H)
    h, c, ga, z = full(B, H), full(B, H), full(B, 4 * H), full(B, 4 * H)
    coef, rb = full(4, 4 * H), full(4 * H)

    def fwd(ovr, coef4, rbias, z_out):
        return lib.blm_lstm_step_fwd_gp(ptr(xw), ptr(w), ptr(hp), ptr(cp), ptr(h), ptr(c), ptr(ga), None, ovr, coef4, rbias, z_out,
                                        B, H, stream())
    assert fwd(6, ptr(coef), ptr(rb), ptr(z)) == ERR_INVALID
    for ovr in (0, 3, 4, 5):
        assert fwd(ovr, None, ptr(rb), ptr(z)) == ERR_INVALID
    assert fwd(4, ptr(coef), None, ptr(z)) == ERR_INVALID
    assert fwd(5, ptr(coef), None, ptr(z)) == ERR_INVALID
    assert fwd(5, ptr(coef), ptr(rb), None) == ERR_INVALID

    w_t, dy, dcn = full(H, 4 * H), full(B, H), full(B, H)
    dgo, dcp, dh, dact, dz = full(B, 4 * H), full(B, H), full(B, H), full(B, H), full(B, 4 * H)

    def bwd(ovr, coef4, z_prev, dact_out, dz_out):
        return lib.blm_lstm_step_bwd_gp(ptr(xw), ptr(w_t), ptr(dy), ptr(dcn), ptr(cp), ptr(c), ptr(ga), ptr(dgo), ptr(dcp), ptr(dh),
                                        ovr, coef4, z_prev, dact_out, dz_out, B, H, stream())
    assert bwd(6, ptr(coef), ptr(z), ptr(dact), ptr(dz)) == ERR_INVALID
    for ovr in (0, 3, 4, 5):
        assert bwd(ovr, None, ptr(z), ptr(dact), ptr(dz)) == ERR_INVALID
        assert bwd(ovr, ptr(coef), None, ptr(dact), ptr(dz)) == ERR_INVALID
    assert bwd(4, ptr(coef), ptr(z), ptr(dact), None) == ERR_INVALID
    assert bwd(5, ptr(coef), ptr(z), ptr(dact), None) == ERR_INVALID
    assert bwd(5, ptr(coef), ptr(z), None, ptr(dz)) == ERR_INVALID

    # the skinny product with the GPNN2 activation sum: M inside the output width, act_mode 1 or 2, acts a 4-bit set
    MP, GP = 160, 192
    src, FT, out, feat = full(B, H), full(MP, H), full(B, GP), full(B, MP)

    def dh_act(M, act_mode, acts):
        return lib.blm_lstm_step_dh_act(ptr(src), ptr(FT), ptr(out), GP, B, MP, H, act_mode, ptr(feat), MP, M, 0.1, acts, stream())
    assert dh_act(MP, 1, 7) == ERR_INVALID and dh_act(MP + 5, 2, 7) == ERR_INVALID
    assert dh_act(150, 0, 7) == ERR_INVALID and dh_act(150, 3, 7) == ERR_INVALID
    assert dh_act(150, 1, 16) == ERR_INVALID and dh_act(150, 2, 16) == ERR_INVALID

    torch.cuda.synchronize()
    for t in (h, c, ga, z, dgo, dcp, dh, dact, dz, out, feat):  # nothing ran: no output was touched
        assert bool((t == SENT).all())


def test_gp_ops_refuse_bad_shapes(dev):
    from bayeslms_amd import ops
    case = R.make_gp_case(2, 3, 64, 5, 1)
    a = {k: (None if case[k] is None else case[k].float().to(dev)) for k in R.GP_INPUTS}
    for bad in (a["w_cell"][:, :32].contiguous(), a["w_cell"][:32].contiguous(), torch.zeros(64, 65, device=dev)):
        with pytest.raises(ops.BayesLMError):
            ops.lstm_recurrent_gp(a["xw"], a["h0"], a["c0"], a["w_rec"], a["coef4"], 5, a["rbias"], bad)
    for H, M in ((96, 150), (64, 160)):
        case = R.make_gpnn2_case(2, 3, H, M, 0, 1, 7, 2)
        a = {k: case[k].float().to(dev) for k in R.GPNN2_INPUTS}
        noises = [ops.NoiseSpec(eps=e.float().to(dev)) for e in case["eps"]]
        with pytest.raises(ops.BayesLMError):
            ops.lstm_recurrent_gpnn2(a["xw"], a["h0"], a["c0"], a["w_hh"], a["coef_w"], a["coef_b"], a["fmean"], a["flgstd"],
                                     noises, 1, 7, 0)
