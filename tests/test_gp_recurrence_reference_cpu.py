"""CPU: tests/gp_recurrence_reference.py (the float64 reference of the GP / GPNN2 step-kernel tests) computes what
oracle.bayes_oracle.gp_lstm_cell computes, once the operands are assembled the way model.GPLSTMCell assembles them for
ops.lstm_recurrent_gp / lstm_recurrent_gpnn2 / gpnn2_steps.  Both sides are float64 torch: they differ by summation order
only, so outputs and every gradient agree to 1e-12.  The deliberately wrong references of the GPU file are shown here to be
visible on its inputs."""
import math

import pytest
import torch

import gp_recurrence_reference as R
from oracle import bayes_oracle as O

SLOT = {"tanh": 0, "sigmoid": 1, "relu": 2, "gelu": 3}  # model.GPNN._SLOT
TOL = 1e-12


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _leaf(t):
    return t.double().requires_grad_(True)


def _cell_sd(gate_type, E, H, two, g, M=150):
    """float64 state dict of one GPLSTMCell with random values (every bias too: the doubled bias_ih must show)."""
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    s = 1.0 / math.sqrt(H)
    sd = {"weights_ih": n(4 * H, E) * s, "bias_ih": n(4 * H) * 0.3, "weights_hh": n(4 * H, H) * s}
    if two:
        NO = H if gate_type <= 5 else 4 * H
        NI = E if gate_type == 7 else H
        sd.update({"gpnn.frequency_mean": n(NI, M) / math.sqrt(NI), "gpnn.frequency_lgstd": -3.0 + 0.3 * n(NI, M),
                   "gpnn.coef.weight": 0.4 * n(NO, M), "gpnn.coef.bias": 0.3 * n(NO)})
    else:
        nact = len(O._gp_acts(gate_type))
        NI, NO = (H + E, H) if gate_type <= 4 else ((E, H) if gate_type == 5 else (E, 4 * H))
        for name, shape, scale in (("weights", (NO, NI), 1.0 / math.sqrt(NI)), ("bias", (NO,), 0.3), ("coef", (nact, NO), 0.7)):
            sd["gpnn.%s_mean" % name] = n(*shape) * scale
            sd["gpnn.%s_lgstd" % name] = -2.0 + 0.3 * n(*shape)
    return {k: _leaf(v) for k, v in sd.items()}


def _coef4(coef, acts):
    """model.GPNN.coef4: the rows of ``coef`` in the kernels' slot order, unused slots zero."""
    rows = [torch.zeros_like(coef[0])] * 4
    for i, a in enumerate(acts):
        rows[SLOT[a]] = coef[i]
    return torch.stack(rows)


def _compare(got, want, leaves, ups):
    for a, b, name in zip(got, want, ("y", "hT", "cT")):
        assert a.shape == b.shape and rel(a, b) < TOL, name
    loss = lambda outs: sum((o * u).sum() for o, u in zip(outs, ups))  # noqa: E731
    names = sorted(leaves)
    ga = torch.autograd.grad(loss(got), [leaves[k] for k in names], allow_unused=True)
    gb = torch.autograd.grad(loss(want), [leaves[k] for k in names], allow_unused=True)
    n_grads = 0
    for k, a, b in zip(names, ga, gb):
        assert (a is None) == (b is None), k
        if b is not None:
            assert rel(a, b) < TOL, k
            n_grads += 1
    return n_grads


def _inputs(T, B, E, H, g):
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    io = {"x": _leaf(n(T, B, E)), "h0": _leaf(0.5 * n(B, H)), "c0": _leaf(0.5 * n(B, H))}
    return io, (n(T, B, H), n(B, H), n(B, H))


@pytest.mark.parametrize("gate_type", [1, 2, 3, 4, 5, 6, 7])
def test_ref_gp_matches_oracle_cell_with_sampled_gpnn(gate_type):
    """GPNN type 3 (Bayesian coefficients, weights and bias, one draw per forward), E = H = 12."""
    T, B, E, H = 4, 3, 12, 12
    g = torch.Generator().manual_seed(100 + gate_type)
    sd = _cell_sd(gate_type, E, H, False, g)
    io, ups = _inputs(T, B, E, H, g)
    eps = {k: torch.randn(sd["gpnn.%s_mean" % k].shape, generator=g, dtype=torch.float64) for k in ("weights", "bias", "coef")}
    want = O.gp_lstm_cell(io["x"], io["h0"], io["c0"], sd, "", gate_type, eps)
    # operands as in model.GPLSTMCell.forward
    Wg, bg, cf = (sd["gpnn.%s_mean" % k] + torch.exp(sd["gpnn.%s_lgstd" % k]) * eps[k] for k in ("weights", "bias", "coef"))
    c4 = _coef4(cf, O._gp_acts(gate_type))
    x, h0, c0 = io["x"], io["h0"], io["c0"]
    w_ih, b_ih, w_hh = sd["weights_ih"], sd["bias_ih"], sd["weights_hh"]
    lin = torch.nn.functional.linear
    if gate_type <= 4:
        k = gate_type - 1
        xw_std = lin(x, w_ih, 2.0 * b_ih)
        xw = torch.cat([xw_std[..., :k * H], lin(x, Wg[:, :E], bg), xw_std[..., (k + 1) * H:]], -1)
        w_rec = torch.cat([w_hh[:k * H], Wg[:, E:], w_hh[(k + 1) * H:]], 0)
        got = R.ref_gp(xw, h0, c0, w_rec, c4, k)
    elif gate_type == 5:
        got = R.ref_gp(lin(x, w_ih, 2.0 * b_ih), h0, c0, w_hh, c4, 5, bg, Wg)
    elif gate_type == 6:
        got = R.ref_gp(lin(x, w_ih, b_ih), h0, c0, Wg, c4, 4, bg)
    else:
        got = R.ref_gp(R.mix(lin(x, Wg, bg), c4) + b_ih, h0, c0, w_hh)
    assert _compare(got, want, {**sd, **io}, ups) >= 9


@pytest.mark.parametrize("gate_type", [1, 2, 3, 4, 5, 6, 7])
def test_ref_gpnn2_matches_oracle_cell_with_injected_eps(gate_type):
    """GPNN2 type 4 with fresh frequencies at every step, H = 64, M = 150, acts = 7 as the models always pass; gate type 7
    goes through ref_gpnn2_steps and the plain recurrence, as the model does."""
    T, B, E, H, M = 3, 3, 64, 64, 150
    g = torch.Generator().manual_seed(200 + gate_type)
    sd = _cell_sd(gate_type, E, H, True, g, M)
    io, ups = _inputs(T, B, E, H, g)
    eps = [torch.randn(sd["gpnn.frequency_mean"].shape, generator=g, dtype=torch.float64) for _ in range(T)]
    want = O.gp_lstm_cell(io["x"], io["h0"], io["c0"], sd, "", gate_type, eps)
    x, h0, c0 = io["x"], io["h0"], io["c0"]
    w_ih, b_ih, w_hh = sd["weights_ih"], sd["bias_ih"], sd["weights_hh"]
    cw, cb, fm, fl = (sd["gpnn." + k] for k in ("coef.weight", "coef.bias", "frequency_mean", "frequency_lgstd"))
    lin = torch.nn.functional.linear
    acts = sum(1 << SLOT[a] for a in ("sigmoid", "relu", "tanh"))
    assert acts == 7
    if gate_type <= 6:
        xw = lin(x, w_ih, b_ih if gate_type == 6 else 2.0 * b_ih)
        mode, gate = (0, gate_type - 1) if gate_type <= 4 else ((1, 0) if gate_type == 5 else (2, 0))
        got = R.ref_gpnn2(xw, h0, c0, None if gate_type == 6 else w_hh, cw, cb, fm, fl, eps, gate, acts, mode)
    else:
        got = R.ref_gp(R.ref_gpnn2_steps(x, cw, cb + b_ih, fm, fl, eps, acts), h0, c0, w_hh)
    assert _compare(got, want, {**sd, **io}, ups) >= 9


def test_ref_gpnn2_mean_frequencies_match_oracle_eval():
    T, B, E, H, M = 3, 2, 64, 64, 150
    g = torch.Generator().manual_seed(77)
    sd = _cell_sd(2, E, H, True, g, M)
    io, ups = _inputs(T, B, E, H, g)
    want = O.gp_lstm_cell(io["x"], io["h0"], io["c0"], sd, "", 2, None)
    xw = torch.nn.functional.linear(io["x"], sd["weights_ih"], 2.0 * sd["bias_ih"])
    got = R.ref_gpnn2(xw, io["h0"], io["c0"], sd["weights_hh"], sd["gpnn.coef.weight"], sd["gpnn.coef.bias"],
                      sd["gpnn.frequency_mean"], sd["gpnn.frequency_lgstd"], None, 1, 7, 0)
    _compare(got, want, {**sd, **io}, ups)


def test_gelu_erf_is_torch_gelu():
    z = torch.linspace(-9, 9, 2001, dtype=torch.float64)
    assert rel(R.gelu_erf(z), torch.nn.functional.gelu(z)) < TOL
    assert rel(R.actsum(z, 8), z + torch.nn.functional.gelu(z)) < TOL
    coef = torch.tensor([[0.0], [0.0], [0.0], [1.0]], dtype=torch.float64)
    assert rel(R.mix(z[:, None], coef), torch.nn.functional.gelu(z)[:, None]) < TOL


@pytest.mark.parametrize("ovr", [0, 1, 2, 3, 4, 5])
def test_gelu_row_changes_the_result(ovr):
    """The models keep the GELU row zero; the cases of the GPU file do not, and that row reaches every output."""
    case = R.make_gp_case(3, 4, 64, ovr, 5)
    full = R.eval_gp(case)
    c0 = case["coef4"].clone()
    c0[3] = 0
    none = R.eval_gp(case, coef4=c0)
    for k in ("y", "hT", "cT", "dxw", "dh0", "dw_rec"):
        assert rel(none[k], full[k]) > 1e-2, k
    assert float(full["dcoef4"][3].abs().max()) > 1e-2


def test_gpnn2_gelu_bit_changes_the_result():
    case = R.make_gpnn2_case(3, 4, 64, 150, 0, 1, 15, 6)
    full, none = R.eval_gpnn2(case), R.eval_gpnn2(case, acts=7)
    for k in ("y", "hT", "cT", "dxw", "dfmean", "dcoef_w"):
        assert rel(none[k], full[k]) > 1e-2, k


# The deliberately wrong references of tests/test_gpu_gp_step_forms.py, on its own cases: each one moves every output by more
# than 100x the output bound (1e-5) and every gradient by more than 100x the gradient bound (5e-5).
def _visible(wrong, right):
    for k, v in right.items():
        if v is not None:
            assert rel(wrong[k], v) > 100 * (5e-5 if k.startswith("d") else 1e-5), k


def test_swapped_coef_rows_are_visible():
    case = R.make_gp_case(3, 33, 320, 2, R.gp_seed(320, 33, 2))
    _visible(R.eval_gp(case, coef4=case["coef4"][[1, 0, 2, 3]]), R.eval_gp(case))


def test_rolled_rbias_is_visible():
    case = R.make_gp_case(3, 33, 512, 4, R.gp_seed(512, 33, 4))
    _visible(R.eval_gp(case, rbias=case["rbias"].roll(512)), R.eval_gp(case))


def test_wrong_acts_are_visible():
    case = R.make_gpnn2_case(3, 33, 576, 150, 0, 0, 15, R.gpnn2_seed(576, 33, 150, 0, 0, 15))
    _visible(R.eval_gpnn2(case, acts=7), R.eval_gpnn2(case))
