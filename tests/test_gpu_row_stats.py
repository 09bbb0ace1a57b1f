"""GPU: blm_row_stats / ops.row_stats against float64 of the same float32 rows.  nll, entropy and conf within
2e-5 max(1, |want|) (the bound tests/test_gpu_mc_uncertainty.py::_check holds the same quantities to); pred and rank are
comparisons of the given floats and must be EQUAL."""
import math

import pytest
import torch

from bayeslms_amd import BayesLMError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _ops():
    from bayeslms_amd import ops
    return ops


def _want(x, tgt=None):
    """float64 of the float32 rows x (R, V) -> nll, conf, entropy, pred, rank (nll / rank None without targets)."""
    xd = x.double()
    R, V = xd.shape
    idx = torch.arange(V, device=x.device).view(1, V)
    mx = xd.max(-1, keepdim=True).values
    lse = torch.logsumexp(xd, -1)
    p = torch.softmax(xd, -1)
    entropy = lse - torch.where(p > 0, p * xd, torch.zeros_like(xd)).sum(-1)
    conf = (mx.squeeze(1) - lse).exp()
    pred = torch.where(xd == mx, idx, torch.full_like(idx, V)).min(-1).values
    if tgt is None:
        return None, conf, entropy, pred, None
    ok = (tgt >= 0) & (tgt < V)
    tc = tgt.clamp(0, V - 1).view(R, 1)
    tv = xd.gather(1, tc)
    nll = lse - tv.squeeze(1)
    rank = (xd > tv).sum(-1) + ((xd == tv) & (idx < tc)).sum(-1)
    nll[~ok] = float("nan")
    rank[~ok] = -1
    return nll, conf, entropy, pred, rank


def _check(name, got, want, rows=None):
    """rows: the rows to compare (default all)"""
    sel = slice(None) if rows is None else rows
    for field, g, w in zip(("nll", "conf", "entropy"), (got.nll, got.conf, got.entropy), want[:3]):
        if w is None:
            assert g is None
            continue
        g, w = g.double()[sel], w[sel]
        fin = torch.isfinite(w)
        assert torch.equal(torch.isfinite(g), fin), (name, field)
        assert torch.equal(g[~fin].nan_to_num(nan=-7.0), w[~fin].nan_to_num(nan=-7.0)), (name, field)  # inf stays inf, NaN stays NaN
        diff = (g[fin] - w[fin]).abs()
        worst = float((diff / w[fin].abs().clamp(min=1.0)).max()) if diff.numel() else 0.0
        print("%s %s: max |got - want| over the bound's scale %.3e (bound 2e-5)" % (name, field, worst))
        assert worst <= 2e-5, (name, field, worst)
    assert got.pred.dtype == torch.int32 and torch.equal(got.pred.long()[sel], want[3][sel]), (name, "pred")
    if want[4] is None:
        assert got.rank is None
    else:
        assert got.rank.dtype == torch.int32 and torch.equal(got.rank.long()[sel], want[4][sel]), (name, "rank")


def _layouts(x):
    """x (R, V) -> (name, matrix to pass, V): the rows as they are (ldx = V: 16-byte loads when V % 4 == 0, else the scalar
    loop), rows padded to 4 floats with garbage in the padding, and padded rows that start 4 bytes off a 16-byte boundary."""
    R, V = x.shape
    ld = (V + 3) // 4 * 4
    yield "ldx=V", x.clone(), V
    pad = torch.full((R, ld), float("nan"), device=x.device)
    pad[:, V:] = 3e38
    pad[:, :V] = x
    yield "padded", pad, V
    yield "view of padded rows", pad[:, :V], None  # not contiguous when V % 4 != 0: read in place through its row stride
    buf = torch.full((R * ld + 4,), 3e38, device=x.device)
    off = buf[1:1 + R * ld].view(R, ld)
    off[:, :V] = x
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    yield "offset", off, V


SHAPES = [(1, 1), (3, 5), (7, 63), (5, 64), (4, 65), (9, 255), (9, 257), (6, 1001), (130, 4096), (4, 33278)]


@pytest.mark.parametrize("R,V", SHAPES)
def test_row_stats_equal_float64_of_the_rows(dev, R, V):
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(1000 * R + V)
    logits = 3.0 * torch.randn(R, V, device=dev, generator=g)
    tgt = torch.randint(0, V, (R,), device=dev, generator=g)
    tgt[0], tgt[-1] = V - 1, 0
    for kind, x in (("logits", logits), ("log-probs", torch.log_softmax(logits.double(), -1).float())):
        want = _want(x, tgt)
        for name, mat, v in _layouts(x):
            got = ops.row_stats(mat, tgt, v)
            if name.startswith("view") and V % 4 and R > 1:
                assert not mat.is_contiguous() and mat.stride(0) == (V + 3) // 4 * 4
            assert all(t.shape == (R,) for t in got)
            _check("%s %s" % (kind, name), got, want)


def test_all_values_equal(dev):
    ops = _ops()
    for V in (1, 5, 64, 257, 1001):
        x = torch.full((3, V), 0.37, device=dev)
        tgt = torch.tensor([0, V // 2, V - 1], device=dev)
        got = ops.row_stats(x, tgt)
        assert got.pred.tolist() == [0, 0, 0] and got.rank.tolist() == tgt.tolist()
        for g, w in ((got.conf, 1.0 / V), (got.entropy, math.log(V)), (got.nll, math.log(V))):
            assert float((g.double() - w).abs().max()) <= 2e-5 * max(1.0, abs(w)), (V, w)


def test_one_finite_value_among_minus_infinity(dev):
    ops = _ops()
    V = 300
    x = torch.full((4, V), float("-inf"), device=dev)
    x[:, 77] = 2.5
    x[3, 77], x[3, 299] = float("-inf"), -1e4  # the finite value in the scalar tail's neighbourhood, and a large one
    tgt = torch.tensor([77, 5, 299, 299], device=dev)
    got = ops.row_stats(x, tgt)
    assert got.conf.tolist() == [1.0] * 4 and got.entropy.tolist() == [0.0] * 4
    assert got.nll.tolist() == [0.0, float("inf"), float("inf"), 0.0]
    assert got.pred.tolist() == [77, 77, 77, 299]
    assert got.rank.tolist() == [0, 1 + 5, 1 + 298, 0]  # behind the finite value and the -inf columns at lower indices
    _check("one finite", got, _want(x, tgt))


def test_values_near_1e4_stay_finite(dev):
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(5)
    for V in (257, 4096):
        x = (torch.rand(6, V, device=dev, generator=g) * 2 - 1) * 1e4
        x[1] = 1e4 - torch.rand(V, device=dev, generator=g)   # a crowded top
        x[2] = -1e4 + torch.rand(V, device=dev, generator=g)
        tgt = torch.randint(0, V, (6,), device=dev, generator=g)
        got = ops.row_stats(x, tgt)
        assert all(bool(torch.isfinite(t).all()) for t in (got.nll, got.conf, got.entropy))
        _check("near 1e4", got, _want(x, tgt))


def test_duplicated_maxima_and_ties(dev):
    ops = _ops()
    V = 1001
    x = torch.zeros(3, V, device=dev)
    x[:, [9, 300, 700, 1000]] = 4.0
    tgt = torch.tensor([700, 9, 1000], device=dev)
    got = ops.row_stats(x, tgt)
    assert got.pred.tolist() == [9, 9, 9] and got.rank.tolist() == [2, 0, 3]
    g = torch.Generator(device=dev).manual_seed(6)
    for V in (63, 256, 1001, 4100):  # a handful of distinct values: every comparison is a tie somewhere
        x = torch.randint(0, 5, (16, V), device=dev, generator=g).float()
        tgt = torch.randint(0, V, (16,), device=dev, generator=g)
        for name, mat, v in _layouts(x):
            _check("ties %s" % name, ops.row_stats(mat, tgt, v), _want(x, tgt))


def test_bad_targets_and_nan_rows_touch_their_row_only(dev):
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(7)
    R, V = 6, 515
    x = torch.randn(R, V, device=dev, generator=g)
    tgt = torch.randint(0, V, (R,), device=dev, generator=g)
    bad = tgt.clone()
    bad[1], bad[4] = -1, V
    got = ops.row_stats(x, bad)
    want = _want(x, bad)
    assert torch.isnan(got.nll[[1, 4]]).all() and got.rank[[1, 4]].tolist() == [-1, -1]
    _check("bad targets", got, want)  # the other rows, and conf / entropy / pred of rows 1 and 4, are what they were
    assert torch.equal(got.conf, ops.row_stats(x, tgt).conf)
    for col in (0, 100, V - 1):  # first float4, the middle, the scalar tail
        y = x.clone()
        y[2, col] = float("nan")
        got = ops.row_stats(y, tgt)
        assert all(math.isnan(float(t[2])) for t in (got.nll, got.conf, got.entropy))
        assert int(got.pred[2]) == -1 and int(got.rank[2]) == -1
        _check("NaN row", got, _want(x, tgt), rows=[0, 1, 3, 4, 5])


def test_without_targets_and_without_rows(dev):
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(8)
    x = torch.randn(5, 130, device=dev, generator=g)
    got = ops.row_stats(x)
    assert got.nll is None and got.rank is None
    _check("tgt=None", got, _want(x))
    empty = ops.row_stats(torch.empty(0, 130, device=dev), torch.empty(0, dtype=torch.int64, device=dev))
    assert all(t.shape == (0,) for t in empty)
    assert all(t.shape == (0,) for t in ops.row_stats(torch.empty(0, 130, device=dev))[1:4])


def test_two_runs_are_bit_identical(dev):
    ops = _ops()
    g = torch.Generator(device=dev).manual_seed(9)
    x = 3.0 * torch.randn(300, 33278, device=dev, generator=g)
    tgt = torch.randint(0, 33278, (300,), device=dev, generator=g)
    a = ops.row_stats(x, tgt)
    assert all(torch.equal(u, v) for u, v in zip(a, ops.row_stats(x, tgt)))
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        b, c = ops.row_stats(x, tgt), ops.row_stats(x, tgt)
    finally:
        ops.set_deterministic(was)
    assert all(torch.equal(u, v) for u, v in zip(b, c)) and all(torch.equal(u, v) for u, v in zip(a, b))


def test_bad_arguments_raise(dev):
    ops = _ops()
    x = torch.randn(4, 10, device=dev)
    tgt = torch.zeros(4, dtype=torch.int64, device=dev)
    with pytest.raises(BayesLMError, match="GPU"):
        ops.row_stats(x.cpu(), tgt)
    with pytest.raises(BayesLMError, match="float32"):
        ops.row_stats(x.double(), tgt)
    with pytest.raises(BayesLMError, match="row-major"):
        ops.row_stats(x[0], tgt[:1])
    with pytest.raises(BayesLMError, match="targets"):
        ops.row_stats(x, tgt[:3])
    with pytest.raises(BayesLMError, match="int64"):
        ops.row_stats(x, tgt.int())
    with pytest.raises(BayesLMError, match="V = 11"):
        ops.row_stats(x, tgt, V=11)
    with pytest.raises(BayesLMError, match="V = 0"):
        ops.row_stats(x, tgt, V=0)
