"""GPU: the operand rules that the row wrappers of bayeslms_amd.ops share (ops._rows_in_place, ops._row_targets), pinned across
every wrapper that takes them: what each refuses and with which words, the layouts each reads or writes where they lie, and
the order in which the 256-thread row kernels fold their lanes.  R = 3 rows of V = 11 columns at row stride 12 unless stated.
References and bars are those of each entry point's own test file, imported from there."""
import numpy as np
import pytest
import torch

import beam_reference
import cache_reference
import laplace_reference
import swag_reference
import test_gpu_cache as TC
import test_gpu_laplace as TL
import test_gpu_row_stats as TR
import test_gpu_row_stats_temps as TT
import test_gpu_swag as TS

pytestmark = pytest.mark.gpu

R, V, LD = 3, 11, 12
BETAS = [0.5, 1.0, 2.0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _i64(dev, *v):
    return torch.tensor(v, dtype=torch.int64, device=dev)


# name -> (matrix arguments, call(ops, mats, V, targets), used in place, takes V, takes one target per row)
def _cache(o, m, V, t):
    dev, n = m["q"].device, m["q"].shape[0]
    return o.cache_scores(m["q"], m["k"], _i64(dev, *range(m["k"].shape[0])) % 2, _i64(dev, *range(n)) % 2,
                          torch.arange(1, n + 1, device=dev, dtype=torch.int32), [0.5], 4)


def _swag(o, m, V, t):
    vec = torch.ones(m["out"].shape[-1], device=m["out"].device)
    return o.swag_sample(m["out"], vec, vec, list(range(R)), 1, 1.0, 0.5, 0.5, 1e-6, dev=m["dev"], k_live=2)


def _avg(o, m, V, t):
    nll_s = None if t is None else torch.empty(2, m["logits"].shape[0], device=m["logits"].device)
    return o.logp_avg_accum(m["logits"], m["acc"], 0, 2, t, None, nll_s, V)


WRAPPERS = {
    "row_stats": (("x",), lambda o, m, V, t: o.row_stats(m["x"], t, V), False, True, True),
    "row_stats_temps": (("x",), lambda o, m, V, t: o.row_stats_temps(m["x"], BETAS, t, V), False, True, True),
    "cache_scores": (("q", "k"), _cache, False, False, False),
    "topk_rows": (("x",), lambda o, m, V, t: o.topk_rows(m["x"], 2), False, False, False),
    "swag_sample": (("out", "dev"), _swag, True, False, False),
    "logp_avg_accum": (("logits", "acc"), _avg, True, True, True),
    "laplace_curvature": (("logits", "out"), lambda o, m, V, t: o.laplace_curvature(m["logits"], m["out"], V), True, True, False),
    "laplace_row_stats": (("z", "var"), lambda o, m, V, t: o.laplace_row_stats(m["z"], m["var"], t, "probit", V), True, True, True),
    "laplace_mc_rows": (("z", "var"), lambda o, m, V, t: o.laplace_mc_rows(m["z"], m["var"], 2, 1, t, 0, V), True, True, True),
}
EACH = [(w, a) for w, spec in WRAPPERS.items() for a in spec[0]]
# what the parent says of an operand that is no matrix
NOT_2D = {"row_stats": "row-major", "row_stats_temps": "row-major", "topk_rows": "row-major", "cache_scores": "must be a .*matrix",
          "swag_sample": "matrix with unit inner stride"}
# and of rows that overlap: the wrapper, or for logp_avg_accum the library
OVERLAP = {"logp_avg_accum": "bad shape"}


def _good(dev, name):
    g = torch.Generator().manual_seed(5)
    return {a: torch.rand(R, LD, generator=g).to(dev) for a in WRAPPERS[name][0]}


def _refused(name, fragment, mats, V=None, targets=None):
    from bayeslms_amd import ops
    with pytest.raises(ops.BayesLMError, match=fragment):
        WRAPPERS[name][1](ops, mats, V, targets)


@pytest.mark.parametrize("name,arg", EACH)
def test_refuses_a_host_tensor_float64_and_what_is_no_matrix(dev, name, arg):
    tgt = _i64(dev, 0, 1, 2) if WRAPPERS[name][4] else None
    good = _good(dev, name)
    _refused(name, "GPU", dict(good, **{arg: good[arg].cpu()}), targets=tgt)
    _refused(name, "float32", dict(good, **{arg: good[arg].double()}), targets=tgt)
    _refused(name, NOT_2D.get(name, "row-major"), dict(good, **{arg: good[arg][0]}), targets=tgt)


@pytest.mark.parametrize("name", [w for w, s in WRAPPERS.items() if s[3]])
def test_refuses_v_outside_the_columns(dev, name):
    tgt = _i64(dev, 0, 1, 2) if WRAPPERS[name][4] else None
    _refused(name, "V = 0", _good(dev, name), 0, tgt)
    _refused(name, "V = %d" % (LD + 1), _good(dev, name), LD + 1, tgt)


@pytest.mark.parametrize("name", [w for w, s in WRAPPERS.items() if s[4]])
def test_refuses_targets_of_another_count_or_type(dev, name):
    _refused(name, "targets", _good(dev, name), V, _i64(dev, 0, 1))
    _refused(name, "int64", _good(dev, name), V, torch.zeros(R, device=dev))


@pytest.mark.parametrize("name,arg", [(w, a) for w, a in EACH if WRAPPERS[w][2]])
def test_in_place_wrappers_refuse_rows_that_overlap(dev, name, arg):
    good = {a: t[:, :V] for a, t in _good(dev, name).items()}
    lapped = torch.zeros(8 * (R - 1) + V, device=dev).as_strided((R, V), (8, 1))
    tgt = _i64(dev, 0, 1, 2) if WRAPPERS[name][4] else None
    _refused(name, OVERLAP.get(name, "overlap"), dict(good, **{arg: lapped}), V if WRAPPERS[name][3] else None, tgt)


# ------------------------------------------------------------------ accepted layouts
LAYOUTS = ["contiguous", "padded view", "offset view", "single row"]


def _place(host, dev, layout):
    """the host matrix (3, 12) -> the device matrix of that layout: all of it; its first 11 columns as a view of rows 12 apart,
    on a 16-byte boundary and one float past one; its row 1 alone, cut from rows 40 apart"""
    host = np.ascontiguousarray(host, dtype=np.float32)
    if layout == "contiguous":
        return torch.from_numpy(host).to(dev)
    if layout == "single row":
        wide = torch.full((R, 40), 3e38, device=dev)
        wide[:, :V] = torch.from_numpy(host[:, :V]).to(dev)
        t = wide[1:2, :V]
        assert t.stride(0) == 40
        return t
    off = int(layout == "offset view")
    buf = torch.full((R * LD + 4,), 3e38, device=dev)
    t = buf[off:off + R * LD].view(R, LD)[:, :V]
    t.copy_(torch.from_numpy(host[:, :V]).to(dev))
    assert t.data_ptr() % 16 == 4 * off and not t.is_contiguous()
    return t


@pytest.fixture
def seen(monkeypatch):
    """the addresses that ops hands to the library during the test"""
    from bayeslms_amd import ops
    out, real = [], ops.ptr

    def ptr(t):
        out.append(real(t))
        return out[-1]
    monkeypatch.setattr(ops, "ptr", ptr)
    return out


def _host(seed, cols=LD, spread=3.0):
    return (spread * np.random.default_rng(seed).standard_normal((R, cols))).astype(np.float32)


def _rows_of(t):
    return t.cpu().numpy().astype(np.float32)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_row_stats_and_temps_read_the_layout_in_place(dev, seen, layout):
    from bayeslms_amd import ops
    x = _place(_host(1), dev, layout)
    tgt = _i64(dev, 3, 0, 10)[:x.shape[0]]
    dense = x.clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = ops.row_stats(x, tgt)
    grown = torch.cuda.memory_allocated() - before
    assert x.data_ptr() in seen
    assert grown == sum(-(-t.numel() * t.element_size() // 512) * 512 for t in got), "row_stats allocated beside its outputs"
    TR._check("row_stats %s" % layout, got, TR._want(dense, tgt))
    del seen[:]
    gott = ops.row_stats_temps(x, BETAS, tgt)
    assert x.data_ptr() in seen
    for j, b in enumerate(BETAS):
        TT._check("row_stats_temps %s" % layout, gott, j, TT._want(dense, b, tgt))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_laplace_wrappers_use_the_layout_in_place(dev, seen, layout):
    from bayeslms_amd import ops
    zh, vh = _host(2), np.abs(_host(3, spread=0.5))
    z, var = _place(zh, dev, layout), _place(vh, dev, layout)
    zh, vh = _rows_of(z), _rows_of(var)
    th = np.array([3, 0, 10])[:z.shape[0]]
    tgt = torch.from_numpy(th).to(dev)
    for link in ("probit", "expexp"):
        del seen[:]
        got = ops.laplace_row_stats(z, var, tgt, link)
        assert z.data_ptr() in seen and var.data_ptr() in seen
        st, y, ey = laplace_reference.closed_form(zh, vh, th, link)
        for k in ("nll", "conf", "entropy", "vbar"):
            TL._within(getattr(got, k), st[k][0], st[k][1], "%s %s %s" % (layout, link, k))
        pred, rank, pok, rok = laplace_reference.decided(y, ey, th)
        assert np.array_equal(got.pred.cpu().numpy()[pok], pred[pok]) and np.array_equal(got.rank.cpu().numpy()[rok], rank[rok])
    del seen[:]
    ops.laplace_mc_rows(z, var, 2, 1, tgt)
    assert z.data_ptr() in seen and var.data_ptr() in seen
    del seen[:]
    a_ref, bound = laplace_reference.curvature(zh)
    out = ops.laplace_curvature(z, out=_place(np.zeros_like(_host(0)), dev, layout))
    assert z.data_ptr() in seen and out.data_ptr() in seen
    TL._within(out, a_ref, bound, "%s curvature" % layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_logp_avg_accum_uses_the_layout_in_place(dev, seen, layout):
    from bayeslms_amd import ops
    zs = [_place(_host(10 + s), dev, layout) for s in range(2)]
    acc = _place(np.zeros_like(_host(0)), dev, layout)
    rows = acc.shape[0]
    th = np.array([3, 0, 10])[:rows]
    hsum, nll_s = torch.empty(rows, device=dev), torch.empty(2, rows, device=dev)
    for s, z in enumerate(zs):
        assert ops.logp_avg_accum(z, acc, s, 2, torch.from_numpy(th).to(dev), hsum, nll_s) is acc
        assert z.data_ptr() in seen and acc.data_ptr() in seen
    ref = swag_reference.average([_rows_of(z) for z in zs], th)
    TS._within(acc, ref["acc"], ref["b_acc"], "%s acc" % layout)
    TS._within(hsum, ref["hsum"], ref["b_hsum"], "%s hsum" % layout)
    TS._within(nll_s, ref["nll_s"], ref["b_nll_s"], "%s nll_s" % layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_cache_scores_and_topk_rows_read_the_layout_in_place(dev, seen, layout):
    from bayeslms_amd import ops
    q = _place(_host(20, spread=0.7), dev, layout)
    k = _place(_host(21, spread=0.7), dev, "padded view" if layout == "single row" else layout)
    n = q.shape[0]
    labels, targets = _i64(dev, 0, 1, 0), _i64(dev, 0, 0, 1)[:n]
    hi = torch.arange(1, n + 1, device=dev, dtype=torch.int32)
    thetas = [float(np.float32(t)) for t in (0.0, 0.5, 2.0)]
    got = ops.cache_scores(q, k, labels, targets, hi, thetas, 2)
    assert q.data_ptr() in seen and k.data_ptr() in seen
    lse, match = cache_reference.cache_scores(q.clone(), k.clone(), labels, targets, hi, thetas, 2)
    TC._compare("%s lse" % layout, got.lse, lse)
    TC._compare("%s match" % layout, got.match, match)
    del seen[:]
    vals, ids = ops.topk_rows(q, 4)
    assert q.data_ptr() in seen
    wv, wi = beam_reference.topk_rows(_rows_of(q), 4)
    assert np.array_equal(vals.cpu().numpy(), wv) and np.array_equal(ids.cpu().numpy(), wi)


@pytest.mark.parametrize("offset,pad,ids", [(0, 0, [0, 1, 2]), (0, 1, [0, 1, 2]), (1, 1, [0, 1, 2]), (0, 29, [1])],
                         ids=LAYOUTS)
def test_swag_sample_writes_the_layout_in_place(dev, offset, pad, ids):
    TS._check_samples(dev, V + (pad == 0), 2, ids, offset=offset, pad=pad)


# ------------------------------------------------------------------ fold order
@pytest.mark.parametrize("Vv", [257, 1024, 1027])
def test_a_tie_between_the_first_and_the_last_wave_goes_to_the_lower_index(dev, Vv):
    """The maximum stands at column 0 (wave 0's first) and at the last column that thread 255 reads (wave 3's last: 255, 1023,
    1023, in the scalar walk and in the float4 walk alike); two more columns equal the target's value, one below and one above
    its index.  A merge in another order, or a lane that is dropped, moves pred or rank."""
    from bayeslms_amd import ops
    x = torch.linspace(-4.0, -1.0, Vv, device=dev).repeat(2, 1)
    last = max(c for c in range(Vv) if c % 256 == 255)
    x[:, 0] = x[:, last] = 5.0
    t = Vv // 2
    x[:, 7] = x[:, Vv - 3] = x[:, t]
    tgt = _i64(dev, t, last)
    above = int((x[0] > x[0, t]).sum())
    want_pred, want_rank = [0, 0], [above + 1, 1]  # row 0: the tie at column 7 is ahead; row 1: column 0 is ahead of the last
    var = torch.zeros_like(x)
    results = [ops.row_stats(x, tgt), ops.row_stats_temps(x, BETAS, tgt), ops.laplace_row_stats(x, var, tgt, "probit"),
               ops.laplace_row_stats(x, var, tgt, "expexp")]
    ld = (Vv + 7) // 4 * 4
    for off in (0, 1):  # rows 16-byte aligned and a multiple of 4 apart: the float4 walk; one float past that: the scalar walk
        xo = torch.zeros(2 * ld + 4, device=dev)[off:off + 2 * ld].view(2, ld)[:, :Vv]
        vo = torch.zeros(2 * ld + 4, device=dev)[off:off + 2 * ld].view(2, ld)[:, :Vv]
        xo.copy_(x)
        results += [ops.row_stats(xo, tgt), ops.row_stats_temps(xo, BETAS, tgt), ops.laplace_row_stats(xo, vo, tgt, "probit"),
                    ops.laplace_row_stats(xo, vo, tgt, "expexp")]
    for got in results:
        assert got.pred.tolist() == want_pred and got.rank.tolist() == want_rank, (type(got).__name__, got.pred, got.rank)
