"""Plain torch references of the GP-LSTM and GPNN2-LSTM recurrences behind ``ops.lstm_recurrent_gp``,
``ops.lstm_recurrent_gpnn2`` and ``ops.gpnn2_steps``: dtype-agnostic (the tests run them in float64), no GPU, autograd
gives every gradient.  Operand conventions are the ops' own (ops._LSTMRecurrentGP / _LSTMRecurrentGPNN2 / _GPNN2Steps):
the mixture's slot order is tanh, sigmoid, relu, gelu; ``acts`` bits 1, 2, 4, 8 are the same four in the same order.

tests/test_gp_recurrence_reference_cpu.py pins these functions to oracle.bayes_oracle.gp_lstm_cell, which the golden
fixtures pin to the original project."""
import math

import torch

GP_INPUTS = ("xw", "h0", "c0", "w_rec", "coef4", "rbias", "w_cell")
GPNN2_INPUTS = ("xw", "h0", "c0", "w_hh", "coef_w", "coef_b", "fmean", "flgstd")
STEPS_INPUTS = ("x", "coef_w", "coef_b", "fmean", "flgstd")


def gelu_erf(z):
    return z * 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))


def mix(z, coef):
    """sum of the four activations of z weighted by the rows of ``coef`` (4, N), N the last dimension of z."""
    return torch.tanh(z) * coef[0] + torch.sigmoid(z) * coef[1] + torch.relu(z) * coef[2] + gelu_erf(z) * coef[3]


def actsum(z, acts):
    out = z
    if acts & 1:
        out = out + torch.tanh(z)
    if acts & 2:
        out = out + torch.sigmoid(z)
    if acts & 4:
        out = out + torch.relu(z)
    if acts & 8:
        out = out + gelu_erf(z)
    return out


def _cell(s, c, H, gate=-1, gate_act=None):
    a = [torch.sigmoid(s[:, :H]), torch.sigmoid(s[:, H:2 * H]), torch.tanh(s[:, 2 * H:3 * H]), torch.sigmoid(s[:, 3 * H:])]
    if gate >= 0:
        a[gate] = gate_act
    i, f, g, o = a
    c = f * c + i * g
    return o * torch.tanh(c), c


def ref_gp(xw, h0, c0, w_rec, coef4=None, ovr=-1, rbias=None, w_cell=None):
    """-> (y (T,B,H), hT, cT).  ``ovr`` -1 plain; 0..3 the mixture (coef4 (4,H)) is that gate's activation; 4 the hidden
    projection plus ``rbias`` goes through the mixture (coef4 (4,4H)); 5 the cell state enters every step as
    mix(c w_cell^T + rbias)."""
    T = xw.shape[0]
    H = xw.shape[-1] // 4
    h, c = h0, c0
    ys = []
    for t in range(T):
        hw = h @ w_rec.t()
        if ovr == 4:
            hw = mix(hw + rbias, coef4)
        s = xw[t] + hw
        gate_act = mix(s[:, ovr * H:(ovr + 1) * H], coef4) if 0 <= ovr < 4 else None
        if ovr == 5:
            c = mix(c @ w_cell.t() + rbias, coef4)
        h, c = _cell(s, c, H, ovr if 0 <= ovr < 4 else -1, gate_act)
        ys.append(h)
    return torch.stack(ys), h, c


def _gpnn2(x, coef_w, coef_b, fmean, flgstd, eps, acts):
    F = fmean if eps is None else fmean + eps * torch.exp(flgstd)
    M = fmean.shape[1]
    return torch.nn.functional.linear(actsum(x @ F, acts) / math.sqrt(M), coef_w, coef_b)


def ref_gpnn2(xw, h0, c0, w_hh, coef_w, coef_b, fmean, flgstd, eps_list, gate, acts, mode):
    """-> (y, hT, cT).  mode 0: gate ``gate`` is GPNN2_t of its own pre-activation; 1: c = GPNN2_t(c) before the update;
    2: the hidden projection of all four gates is GPNN2_t(h) (coef_w (4H,M), w_hh unused).  ``eps_list`` None: mean
    frequencies at every step."""
    T = xw.shape[0]
    H = xw.shape[-1] // 4
    h, c = h0, c0
    ys = []
    for t in range(T):
        e = None if eps_list is None else eps_list[t]
        gp = lambda v: _gpnn2(v, coef_w, coef_b, fmean, flgstd, e, acts)  # noqa: E731
        s = xw[t] + (gp(h) if mode == 2 else h @ w_hh.t())
        gate_act = gp(s[:, gate * H:(gate + 1) * H]) if mode == 0 else None
        if mode == 1:
            c = gp(c)
        h, c = _cell(s, c, H, gate if mode == 0 else -1, gate_act)
        ys.append(h)
    return torch.stack(ys), h, c


def ref_gpnn2_steps(x, coef_w, coef_b, fmean, flgstd, eps_list, acts):
    """(T,B,E) -> (T,B,NO): GPNN2_t(x[t])."""
    return torch.stack([_gpnn2(x[t], coef_w, coef_b, fmean, flgstd, None if eps_list is None else eps_list[t], acts)
                        for t in range(x.shape[0])])


# ---------------------------------------------------------------------------- cases
def _draws(seed):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1  # noqa: E731
    return n, u


def make_gp_case(T, B, H, ovr, seed):
    """float64 operands of ref_gp / ops.lstm_recurrent_gp plus upstream gradients gy, gh, gc; absent operands are None."""
    n, u = _draws(seed)
    k = 3.0 / math.sqrt(H)
    C = 4 * H if ovr == 4 else H
    case = {"ovr": ovr, "xw": n(T, B, 4 * H), "h0": 0.5 * n(B, H), "c0": 0.5 * n(B, H), "w_rec": u(4 * H, H) * k,
            "coef4": u(4, C) if ovr >= 0 else None, "rbias": 0.3 * n(C) if ovr >= 4 else None,
            "w_cell": u(H, H) * k if ovr == 5 else None}
    case.update(gy=n(T, B, H), gh=n(B, H), gc=n(B, H))
    return case


def make_gpnn2_case(T, B, H, M, mode, gate, acts, seed):
    """float64 operands of ref_gpnn2 / ops.lstm_recurrent_gpnn2 (``eps``: list of T (H,M) draws) plus gy, gh, gc."""
    n, u = _draws(seed)
    NO = 4 * H if mode == 2 else H
    case = {"mode": mode, "gate": gate, "acts": acts, "xw": n(T, B, 4 * H), "h0": 0.5 * n(B, H), "c0": 0.5 * n(B, H),
            "w_hh": u(4 * H, H) * (3.0 / math.sqrt(H)) if mode != 2 else None,
            "coef_w": 0.4 * u(NO, M), "coef_b": 0.3 * n(NO), "fmean": n(H, M) / math.sqrt(H), "flgstd": u(H, M) * 0.5 - 3.0,
            "eps": [n(H, M) for _ in range(T)]}
    case.update(gy=n(T, B, H), gh=n(B, H), gc=n(B, H))
    return case


def make_steps_case(T, B, E, NO, M, acts, seed):
    """float64 operands of ref_gpnn2_steps / ops.gpnn2_steps plus the upstream gradient ``gout``."""
    n, u = _draws(seed)
    return {"acts": acts, "x": n(T, B, E), "coef_w": 0.4 * u(NO, M), "coef_b": 0.3 * n(NO), "fmean": n(E, M) / math.sqrt(E),
            "flgstd": u(E, M) * 0.5 - 3.0, "eps": [n(E, M) for _ in range(T)], "gout": n(T, B, NO)}


def gp_seed(H, B, ovr):
    """the seed of the (H, B, ovr) case: the GPU file and the CPU check of its wrong references draw the same operands."""
    return 1000 * H + 10 * B + ovr + 1


def gpnn2_seed(H, B, M, mode, gate, acts):
    return 1000 * H + 10 * B + M + 7 * mode + 3 * gate + 100 * acts


# ---------------------------------------------------------------------------- outputs and gradients of a case
def _leaves(case, names, dtype):
    return {k: (None if case[k] is None else case[k].to(dtype).clone().requires_grad_(True)) for k in names}


def _collect(outs, out_names, ups, leaves):
    loss = sum((o * u.to(o.dtype)).sum() for o, u in zip(outs, ups))
    loss.backward()
    res = {k: o.detach() for k, o in zip(out_names, outs)}
    res.update({"d" + k: v.grad for k, v in leaves.items() if v is not None})
    return res


def eval_gp(case, dtype=torch.float64, **replace):
    """{y, hT, cT, dxw, dh0, ...} of ref_gp on ``case``; ``replace`` swaps operands (the deliberately wrong references)."""
    lv = _leaves(dict(case, **replace), GP_INPUTS, dtype)
    outs = ref_gp(lv["xw"], lv["h0"], lv["c0"], lv["w_rec"], lv["coef4"], case["ovr"], lv["rbias"], lv["w_cell"])
    return _collect(outs, ("y", "hT", "cT"), (case["gy"], case["gh"], case["gc"]), lv)


def eval_gpnn2(case, dtype=torch.float64, acts=None, use_eps=True):
    lv = _leaves(case, GPNN2_INPUTS, dtype)
    eps = [e.to(dtype) for e in case["eps"]] if use_eps else None
    outs = ref_gpnn2(lv["xw"], lv["h0"], lv["c0"], lv["w_hh"], lv["coef_w"], lv["coef_b"], lv["fmean"], lv["flgstd"], eps,
                     case["gate"], case["acts"] if acts is None else acts, case["mode"])
    return _collect(outs, ("y", "hT", "cT"), (case["gy"], case["gh"], case["gc"]), lv)


def eval_steps(case, dtype=torch.float64):
    lv = _leaves(case, STEPS_INPUTS, dtype)
    out = ref_gpnn2_steps(lv["x"], lv["coef_w"], lv["coef_b"], lv["fmean"], lv["flgstd"], [e.to(dtype) for e in case["eps"]],
                          case["acts"])
    return _collect((out,), ("out",), (case["gout"],), lv)
