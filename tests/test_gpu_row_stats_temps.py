"""GPU: blm_row_stats_temps / ops.row_stats_temps against float64 of the same float32 rows, at every inverse temperature of the
list.  nll, conf, entropy and dnll within 2e-5 max(1, |want|), the bar tests/test_gpu_row_stats.py holds the same quantities
to (a float32 emulation of the lane-wise accumulation stays below 1.8e-6 of that scale up to V 33,278 and beta 1/8 .. 8); pred
and rank are comparisons of the given floats and must be EQUAL."""
import math

import pytest
import torch

from bayeslms_amd import BayesLMError

pytestmark = pytest.mark.gpu

FIELDS = ("nll", "conf", "entropy", "dnll")
EIGHT = [1 / 8, 1 / 4, 1 / 2, 1.0, 1.7, 3.0, 5.0, 8.0]
BETAS = [[1.0], [0.5, 1.0, 2.0], [0.7, 1.0, 1.3, 2.0, 4.0], EIGHT]  # the third: a count with no kernel form of its own


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _ops():
    from bayeslms_amd import ops
    return ops


def _f32(b):
    return float(torch.tensor(b, dtype=torch.float32))  # the inverse temperature the kernel is given


def _nll64(xd, tv, beta):
    return torch.logsumexp(beta * xd, -1) - beta * tv


def _want(x, beta, tgt=None):
    """float64 of the float32 rows x (R, V) under p ~ exp(beta x) -> nll, conf, entropy, dnll, pred, rank."""
    xd = x.double()
    R, V = xd.shape
    beta = _f32(beta)
    idx = torch.arange(V, device=x.device).view(1, V)
    mx = xd.max(-1, keepdim=True).values
    z = beta * xd
    lse = torch.logsumexp(z, -1)
    p = torch.softmax(z, -1)
    zero = torch.zeros_like(xd)
    entropy = lse - torch.where(p > 0, p * z, zero).sum(-1)
    mean_x = torch.where(p > 0, p * xd, zero).sum(-1)
    conf = (beta * mx.squeeze(1) - lse).exp()
    pred = torch.where(xd == mx, idx, torch.full_like(idx, V)).min(-1).values
    if tgt is None:
        return None, conf, entropy, None, pred, None
    ok = (tgt >= 0) & (tgt < V)
    tc = tgt.clamp(0, V - 1).view(R, 1)
    tv = xd.gather(1, tc)
    nll = lse - beta * tv.squeeze(1)
    dnll = mean_x - tv.squeeze(1)
    rank = (xd > tv).sum(-1) + ((xd == tv) & (idx < tc)).sum(-1)
    nll[~ok] = float("nan")
    dnll[~ok] = float("nan")
    rank[~ok] = -1
    return nll, conf, entropy, dnll, pred, rank


def _check(name, got, j, want, rows=None):
    """temperature slot j of ``got`` against ``want``; rows: the rows to compare (default all)"""
    sel = slice(None) if rows is None else rows
    for field, w in zip(FIELDS, want[:4]):
        g = getattr(got, field)
        if w is None:
            assert g is None
            continue
        g, w = g[j].double()[sel], w[sel]
        fin = torch.isfinite(w)
        assert torch.equal(torch.isfinite(g), fin), (name, field)
        assert torch.equal(g[~fin].nan_to_num(nan=-7.0), w[~fin].nan_to_num(nan=-7.0)), (name, field)  # inf stays inf, NaN stays NaN
        diff = (g[fin] - w[fin]).abs()
        worst = float((diff / w[fin].abs().clamp(min=1.0)).max()) if diff.numel() else 0.0
        print("%s %s: max |got - want| over the bound's scale %.3e (bound 2e-5)" % (name, field, worst))
        assert worst <= 2e-5, (name, field, worst)
    assert got.pred.dtype == torch.int32 and torch.equal(got.pred.long()[sel], want[4][sel]), (name, "pred")
    if want[5] is None:
        assert got.rank is None
    else:
        assert got.rank.dtype == torch.int32 and torch.equal(got.rank.long()[sel], want[5][sel]), (name, "rank")


def _layouts(x):
    """The four layouts of tests/test_gpu_row_stats.py: ldx = V, rows padded to 4 floats with NaN / 3e38 in the padding, a view of
    padded rows, and padded rows whose base is 4 bytes off a 16-byte boundary."""
    R, V = x.shape
    ld = (V + 3) // 4 * 4
    yield "ldx=V", x.clone(), V
    pad = torch.full((R, ld), float("nan"), device=x.device)
    pad[:, V:] = 3e38
    pad[:, :V] = x
    yield "padded", pad, V
    yield "view of padded rows", pad[:, :V], None
    buf = torch.full((R * ld + 4,), 3e38, device=x.device)
    off = buf[1:1 + R * ld].view(R, ld)
    off[:, :V] = x
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    yield "offset", off, V


SHAPES = [(1, 1), (3, 5), (7, 63), (4, 65), (9, 257), (6, 1001), (130, 4096), (4, 33278)]


@pytest.mark.parametrize("R,V", SHAPES)
def test_every_temperature_equals_float64_of_the_rows(dev, R, V):
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(1000 * R + V)
    logits = 3.0 * torch.randn(R, V, device=dev, generator=g)
    tgt = torch.randint(0, V, (R,), device=dev, generator=g)
    tgt[0], tgt[-1] = V - 1, 0
    for kind, x in (("logits", logits), ("log-probs", torch.log_softmax(logits.double(), -1).float())):
        want = {b: _want(x, b, tgt) for bs in BETAS for b in bs}  # once per temperature, shared by lists and layouts
        tv = x.double().gather(1, tgt.view(R, 1)).squeeze(1)
        for b in EIGHT:  # the reference's slope against a central difference of its own float64 nll
            h = 1e-5 * _f32(b)
            fd = (_nll64(x.double(), tv, _f32(b) + h) - _nll64(x.double(), tv, _f32(b) - h)) / (2 * h)
            assert float(((fd - want[b][3]).abs() / want[b][3].abs().clamp(min=1.0)).max()) <= 1e-6
        for name, mat, v in _layouts(x):
            for bs in BETAS:
                got = ops.row_stats_temps(mat, bs, tgt, v)
                assert all(getattr(got, f).shape == (len(bs), R) for f in FIELDS) and got.pred.shape == got.rank.shape == (R,)
                for j, b in enumerate(bs):
                    _check("%s %s beta %g of %d" % (kind, name, b, len(bs)), got, j, want[b])
                    if name == "ldx=V" and len(bs) == 8:  # dnll against the central difference of the float64 nll itself
                        h = 1e-5 * _f32(b)
                        fd = (_nll64(x.double(), tv, _f32(b) + h) - _nll64(x.double(), tv, _f32(b) - h)) / (2 * h)
                        worst = float(((got.dnll[j].double() - fd).abs() / fd.abs().clamp(min=1.0)).max())
                        print("%s beta %g: dnll against the central difference %.3e" % (kind, b, worst))
                        assert worst <= 2e-5


def test_beta_one_is_row_stats(dev):
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(3)
    for R, V in ((9, 257), (6, 1001), (130, 4096)):
        x = 3.0 * torch.randn(R, V, device=dev, generator=g)
        tgt = torch.randint(0, V, (R,), device=dev, generator=g)
        one, ref = ops.row_stats_temps(x, [0.5, 1.0, 2.0], tgt), ops.row_stats(x, tgt)
        assert torch.equal(one.pred, ref.pred) and torch.equal(one.rank, ref.rank)
        for f in ("nll", "conf", "entropy"):
            a, b = getattr(one, f)[1].double(), getattr(ref, f).double()
            assert float(((a - b).abs() / b.abs().clamp(min=1.0)).max()) <= 2e-5, f


def _klass(t):
    """finite 0, +inf 1, -inf 2, NaN 3 per element"""
    t = t.double()
    return torch.isposinf(t) * 1 + torch.isneginf(t) * 2 + torch.isnan(t) * 3


def test_special_rows_are_answered_as_row_stats_answers_them(dev):
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(7)
    R, V = 10, 515
    x = torch.randn(R, V, device=dev, generator=g)
    tgt = torch.randint(0, V, (R,), device=dev, generator=g)
    x[1, 100] = float("nan")            # a NaN in the row
    x[2, V - 1] = float("nan")          # ... in the scalar tail
    tgt[3], tgt[4] = -1, V              # targets out of range
    x[5, :] = float("-inf")             # one finite value among -inf, the target at -inf
    x[5, 77], tgt[5] = 2.5, 5
    x[6, :] = float("-inf")             # ... and the target on the finite value
    x[6, 300], tgt[6] = -1e4, 300
    x[7, int(tgt[7])] = float("-inf")   # a -inf target in an ordinary row
    x[8] = torch.randint(0, 3, (V,), device=dev, generator=g).float()  # ties
    x[9] = 0.37                         # all equal
    ref = ops.row_stats(x, tgt)
    for bs in BETAS:
        got = ops.row_stats_temps(x, bs, tgt)
        assert torch.equal(got.pred, ref.pred) and torch.equal(got.rank, ref.rank)
        for j, b in enumerate(bs):
            for f in ("nll", "conf", "entropy"):
                assert torch.equal(_klass(getattr(got, f)[j]), _klass(getattr(ref, f))), (b, f)
            assert torch.equal(_klass(got.dnll[j]), _klass(ref.nll)), b  # the slope is finite, +inf or NaN where the NLL is
            _check("special beta %g" % b, got, j, _want(x, b, tgt), rows=[0, 3, 4, 5, 6, 7, 8, 9])
        assert got.nll[:, 5].tolist() == [float("inf")] * len(bs) == got.dnll[:, 5].tolist() == got.nll[:, 7].tolist()
        assert got.nll[:, 6].tolist() == [0.0] * len(bs) and got.conf[:, 6].tolist() == [1.0] * len(bs)
    none, ref = ops.row_stats_temps(x, EIGHT), ops.row_stats(x)
    assert none.nll is None and none.dnll is None and none.rank is None and torch.equal(none.pred, ref.pred)
    for j in range(8):
        for f in ("conf", "entropy"):
            assert torch.equal(_klass(getattr(none, f)[j]), _klass(getattr(ref, f))), (j, f)
    with_t = ops.row_stats_temps(x, EIGHT, tgt)
    assert torch.equal(none.conf.nan_to_num(nan=-7.0), with_t.conf.nan_to_num(nan=-7.0))
    empty = ops.row_stats_temps(torch.empty(0, 130, device=dev), [1.0, 2.0], torch.empty(0, dtype=torch.int64, device=dev))
    assert all(getattr(empty, f).shape == (2, 0) for f in FIELDS) and empty.pred.shape == (0,)


def test_a_temperature_gives_the_same_bits_alone_in_a_list_and_elsewhere_in_it(dev):
    """Every kernel form (1, 2, 4 and 8 slots, 16-byte loads and the scalar loop) runs the same operations per slot."""
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(9)
    for R, V in ((130, 4096), (40, 1001), (4, 33278)):
        x = 3.0 * torch.randn(R, V, device=dev, generator=g)
        tgt = torch.randint(0, V, (R,), device=dev, generator=g)
        for b in (1.7, 1 / 8, 8.0):
            alone = ops.row_stats_temps(x, [b], tgt)
            others = [v for v in EIGHT if v != b]
            lists = [(EIGHT, EIGHT.index(b)), (EIGHT[::-1], 7 - EIGHT.index(b)), ([b] + others, 0), ([3.0, b], 1), ([b, 0.3], 0),
                     ([0.9, 2.2, b], 2), ([0.9, b, 2.2, 4.0], 1), ([0.9, 2.2, 4.0, 0.2, b], 4), (others[:6] + [b], 6)]
            for bs, j in lists:
                got = ops.row_stats_temps(x, bs, tgt)
                for f in FIELDS:
                    assert torch.equal(getattr(got, f)[j], getattr(alone, f)[0]), (V, b, bs, f)
                assert torch.equal(got.pred, alone.pred) and torch.equal(got.rank, alone.rank)


def test_two_runs_are_bit_identical(dev):
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(9)
    x = 3.0 * torch.randn(300, 33278, device=dev, generator=g)
    tgt = torch.randint(0, 33278, (300,), device=dev, generator=g)
    a = ops.row_stats_temps(x, EIGHT, tgt)
    assert all(torch.equal(u, v) for u, v in zip(a, ops.row_stats_temps(x, EIGHT, tgt)))
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        b, c = ops.row_stats_temps(x, EIGHT, tgt), ops.row_stats_temps(x, EIGHT, tgt)
    finally:
        ops.set_deterministic(was)
    assert all(torch.equal(u, v) for u, v in zip(b, c)) and all(torch.equal(u, v) for u, v in zip(a, b))


def test_surplus_slots_and_neighbouring_memory_stay_unwritten(dev):
    """Five temperatures run the eight-slot form: rows 5.. of a (8, R) buffer handed in as the outputs keep their fill."""
    from bayeslms_amd import _lib as L
    ops = _ops()
    R, V = 33, 257
    x = torch.randn(R, V, device=dev)
    tgt = torch.randint(0, V, (R,), device=dev)
    bufs = [torch.full((8, R), -77.0, device=dev) for _ in range(4)]
    temps = ops.row_temps(BETAS[2])
    L.calls().blm_row_stats_temps(x.data_ptr(), V, tgt.data_ptr(), R, V, L.C.byref(temps), *[b.data_ptr() for b in bufs], None, None,
                                  L.stream())
    torch.cuda.synchronize()
    want = ops.row_stats_temps(x, BETAS[2], tgt)
    for b, f in zip(bufs, FIELDS):
        assert torch.equal(b[:5], getattr(want, f)) and bool((b[5:] == -77.0).all()), f


def test_bad_arguments_raise(dev):
    ops = _ops()
    x = torch.randn(4, 10, device=dev)
    tgt = torch.zeros(4, dtype=torch.int64, device=dev)
    with pytest.raises(BayesLMError, match="GPU"):
        ops.row_stats_temps(x.cpu(), [1.0], tgt)
    with pytest.raises(BayesLMError, match="float32"):
        ops.row_stats_temps(x.double(), [1.0], tgt)
    with pytest.raises(BayesLMError, match="row-major"):
        ops.row_stats_temps(x[0], [1.0], tgt[:1])
    with pytest.raises(BayesLMError, match="targets"):
        ops.row_stats_temps(x, [1.0], tgt[:3])
    with pytest.raises(BayesLMError, match="int64"):
        ops.row_stats_temps(x, [1.0], tgt.int())
    with pytest.raises(BayesLMError, match="V = 11"):
        ops.row_stats_temps(x, [1.0], tgt, V=11)
    with pytest.raises(BayesLMError, match="V = 0"):
        ops.row_stats_temps(x, [1.0], tgt, V=0)
    for bad, msg in (([], "0 inverse"), ([1.0] * 9, "9 inverse"), ([1.0, 0.0], r"betas\[1\] = 0.0"), ([-1.0], r"betas\[0\] = -1.0"),
                     ([float("nan")], "nan"), ([float("inf")], "inf")):
        with pytest.raises(BayesLMError, match=msg):
            ops.row_stats_temps(x, bad, tgt)
    assert math.isfinite(float(ops.row_stats_temps(x, [1.0], tgt).nll.sum()))
