"""CPU: tests/attention_reference.py -- the float64 reference of tests/test_gpu_attention_forms.py -- against the oracle, and the
conditioning of every case of that suite's table: the float32 evaluation of the reference itself stays within CAP times its own
error on ordinary inputs, so a bound of the GPU suite never has to be cut off at the cap."""
import math

import pytest
import torch

import attention_reference as A
from oracle import bayes_oracle as O


def _max_abs(a, b):
    return float((a.double() - b.double()).abs().max())


@pytest.mark.parametrize("T,B,nhead,hd", [(1, 2, 2, 64), (33, 2, 2, 64), (97, 3, 1, 64), (129, 2, 2, 100), (40, 2, 2, 4)])
def test_reference_equals_the_oracle_and_its_autograd(T, B, nhead, hd):
    q, k, v, go = A.make_case("ordinary", T, B, nhead, hd, 5)
    out, lse, dq, dk, dv = A.reference(q, k, v, go, nhead)
    assert out.dtype == torch.float64 and lse.shape == (B * nhead, T)
    leaves = [t.double().requires_grad_(True) for t in (q, k, v)]
    want = O.attention_core(*leaves, nhead, O.causal_mask(T).double())
    want.backward(go.double())
    for got, ref in zip((out, dq, dk, dv), (want.detach(), *[t.grad for t in leaves])):
        assert _max_abs(got, ref) <= 1e-12 * max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("family", A.FAMILIES)
def test_lse_is_the_logsumexp_of_the_masked_scores(family):
    T, B, nhead, hd = 70, 2, 2, 64
    q, k, v, go = A.make_case(family, T, B, nhead, hd, 11)
    lse = A.reference(q, k, v, go, nhead)[1]
    for b in range(B):
        for h in range(nhead):
            sl = slice(h * hd, (h + 1) * hd)
            s = q[:, b, sl].double() @ k[:, b, sl].double().t() / math.sqrt(hd)
            for t in (0, 1, 31, 32, T - 1):
                assert abs(float(torch.logsumexp(s[t, :t + 1], 0)) - float(lse[b * nhead + h, t])) <= 1e-12 * max(1.0, abs(float(lse[b * nhead + h, t])))


def test_keep_form_equals_the_composition_of_the_dropout_test():
    """the composition of test_attention_dropout_uses_philox_mask (tests/test_gpu_kernels.py), in float64, on a column window"""
    T, B, nhead, hd = 50, 2, 2, 64
    c, mask, off, G = A.drop_case("ordinary", T, B, nhead, hd, True)
    assert (off, G) == (1, B + 2) and mask.shape == (G * nhead, T, T)
    keep = mask[off * nhead:(off + B) * nhead].double()
    vals = keep.unique().tolist()
    assert 0.6 < float((keep > 0).double().mean()) < 0.8 and len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] - 1 / 0.7) < 1e-6
    q, k, v, go = c.inputs
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    qh = (qr * hd ** -0.5).contiguous().view(T, B * nhead, hd).transpose(0, 1)
    kh = kr.contiguous().view(T, B * nhead, hd).transpose(0, 1)
    vh = vr.contiguous().view(T, B * nhead, hd).transpose(0, 1)
    pr = torch.softmax(torch.bmm(qh, kh.transpose(1, 2)) + O.causal_mask(T).double(), -1) * keep
    ref = torch.bmm(pr, vh).transpose(0, 1).contiguous().view(T, B, nhead * hd)
    ref.backward(go.double())
    for name, want in zip(("out", "dq", "dk", "dv"), (ref.detach(), qr.grad, kr.grad, vr.grad)):
        assert _max_abs(c.ref[name], want) <= 1e-12 * max(1.0, float(want.abs().max())), name


def test_families_are_what_the_table_says():
    T, B, nhead, hd = 97, 2, 2, 64
    base = A.make_case("ordinary", T, B, nhead, hd, 3)
    again = A.make_case("ordinary", T, B, nhead, hd, 3)
    assert all(torch.equal(a, b) for a, b in zip(base, again))
    pk = A.make_case("peaked", T, B, nhead, hd, 3)
    assert torch.allclose(pk[0], base[0] * math.sqrt(6.0)) and torch.allclose(pk[1], base[1] * math.sqrt(6.0)) and torch.equal(pk[2], base[2])
    for family, first, last in (("rising", 0.0, 32.0), ("falling", 0.0, -32.0), ("shifted", 24.0, 24.0)):
        q, k, v, go = A.make_case(family, T, B, nhead, hd, 3)
        assert bool((q[..., 0::hd] == 8.0).all()) and bool((k[0][..., 0::hd] == first).all()) and bool((k[-1][..., 0::hd] == last).all())
        other = torch.ones(nhead * hd, dtype=torch.bool)
        other[0::hd] = False
        assert torch.equal(q[..., other], base[0][..., other]) and torch.equal(k[..., other], base[1][..., other])
        assert torch.equal(v, base[2]) and torch.equal(go, base[3])
    for family in A.FAMILIES:  # the scalings keep the largest |score| at about 45, lse up to about 40
        c = A.case(family, 385, 2, 2, 64)
        assert float(c.ref["lse"].abs().max()) < 50.0, family
    assert A.make_case("rising", 1, 2, 2, 64, 3)[1][..., 0].abs().max() == 0  # max(T - 1, 1)


def test_the_case_table_covers_what_it_promises():
    ts = A.family_ts(A.ALL_T)
    assert ts["ordinary"] == ts["rising"] == A.ALL_T and ts["peaked"] == ts["falling"] == ts["shifted"] == (1, 127, 128)
    assert A.family_ts(A.LONG_T)["peaked"] == (129, 385) and A.family_ts(A.SHORT_T)["shifted"] == (1, 31, 32)
    assert len(A.pair_cases()) == 399 and len(A.keep_cases()) == 12 and len(A.rows_cases()) == 25 and len(A.tree_cases()) == 24
    assert len(A.decode_cases()) == 76 and len(A.drop_cases()) == 72 and len(A.ALIGN_CASES) == 16


def test_every_case_of_the_table_is_conditioned_within_the_cap():
    """multiplier e32 / U <= CAP for every tensor and block of every case the GPU suite runs: without and with dropout, the
    decode rows included.  If a BLAS difference moves a case over the cap, lower that family's scale; the cap stays."""
    U = A.unit()
    assert 1e-7 < U < 5e-6, U  # float32's own error on ordinary inputs: a handful of ulps
    worst, allow = {}, {}

    def take(what, c, family):
        m = c.multiplier() / U
        worst[family] = max(worst.get(family, 0.0), m)
        assert set(c.extra) == ({"dq"} if family in A.FEATURE0 else set())
        allow[family] = max(allow.get(family, 0.0), max(c.extra.get("dq", [0.0])))
        assert m <= A.CAP, (what, c.key, m)
    for s in A.table_shapes():
        take("plain", A.case(*s), s[0])
    for hd, f, past, Tq in A.decode_cases():
        take("decode", A.decode_case(f, past, Tq, 2, 2, hd), f)
    for key, f, T in A.keep_cases():
        take(key, A.drop_case(f, T, 2, 2, A.KEEP_FORMS[key][0], True, "torch")[0], f)
    for key, f, T, win in A.drop_cases():
        take(key, A.drop_case(f, T, 2, 2, A.DROP_FORMS[key][0], win)[0], f)
    for T, hpw, p, f in A.ALIGN_CASES:
        if p > 0:
            take("align", A.drop_case(f, T, 2, 2, 64, False)[0], f)
    print("U %.3e; worst multiplier per family: %s" % (U, ", ".join("%s %.2f" % kv for kv in sorted(worst.items()))))
    assert worst["ordinary"] <= 2.0  # dropout masks on ordinary inputs stay at the unit
    print("largest recomputation allowance of dq per family: %s" % ", ".join("%s %.2e" % kv for kv in sorted(allow.items())))
    assert allow["ordinary"] == allow["peaked"] == 0.0  # their bounds are the plain ones
