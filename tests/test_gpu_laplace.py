"""GPU: the last-layer Laplace posterior -- blm_laplace_curvature / blm_laplace_row_stats / blm_laplace_mc_rows
(ops.laplace_curvature, ops.laplace_row_stats, ops.laplace_mc_rows) against the float64 reference of tests/laplace_reference.py,
then laplace.LaplacePosterior, engine.fit_laplace / evaluate_laplace / fit_laplace_prior and the evaluate command line on tiny
models.

Bounds: derived in tests/laplace_reference.py from the rounded fp32 operations behind each output, evaluated per element from
the float64 magnitudes, with a factor 2.  The Monte-Carlo kernel's noise is read back through ops.philox_normal, so its bound
covers arithmetic only.  pred and rank are asserted exactly on the rows the reference decides by margin (more than 4 x the
value bound between the values that decide them); the inputs' seed is the first of a fixed list for which at most 1 row in 20
is left undecided -- a property of the float64 reference alone -- and that cap is asserted.

Through the layers the decoder's logits in float64 carry the product's error: K exact products summed in fp32, (K + 3) u of
sum |h w| + |b|."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import laplace_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEED = 1111
STREAM = 0x50000000
# (rows, V): one row of one column (a one-row view's row stride means nothing: ops takes max(stride, V)), one column, a tail, more
# than one trip of a lane, a tail past 4096
VS = [(1, 1), (3, 1), (3, 37), (5, 1000), (2, 4099)]
LAYOUTS = ["aligned", "wide", "offset"]
V, W, SEQ, COLS, ROWS = 50, 32, 5, 3, 41
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def deterministic():
    from bayeslms_amd import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(was)


def _place(a, dev, layout, fill=7.0):
    """the fp32 host matrix (R, V) on the device -> (view (R, V), its whole buffer (R, ld)).  aligned: rows Vq = V rounded up to 4
    apart on a 16-byte boundary (the 16-byte path); wide: Vq + 8 apart; offset: V apart, the base one float past a boundary."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    Rr, Vv = a.shape
    Vq = (Vv + 3) // 4 * 4
    ld = {"aligned": Vq, "wide": Vq + 8, "offset": Vv}[layout]
    off = 1 if layout == "offset" else 0
    buf = torch.full((Rr * ld + 4,), fill, device=dev, dtype=torch.float32)
    whole = buf[off:off + Rr * ld].view(Rr, ld)
    view = whole[:, :Vv]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 * off
    return view, whole


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _within(got, ref, bound, what):
    got = _np(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref, bound = np.broadcast_to(ref, got.shape), np.broadcast_to(bound, got.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d of %d beyond the bound, worst |err| %.3e at bound %.3e" % (
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(bound[bad].max()))


# ------------------------------------------------------------------ curvature
CURV = VS + [(2, 4096 * 3 + 4), (2, 4096 * 9 + 4)]  # and just past each switch of the kernel's form: registers x3, x9, two sweeps


def _curv_logits(rows, Vv):
    rng = np.random.default_rng(100 + Vv)
    x = (3 * rng.standard_normal((rows, Vv))).astype(np.float32)
    if Vv > 1:
        x[0, Vv // 2] = -np.inf  # a column at -inf
        others = np.log(np.exp(R.f64(x[-1, 1:])).sum())
        x[-1, 0] = np.float32(others + 13.8)  # a dominant column: 1 - p about 1e-6
    return x


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rows,Vv", CURV)
def test_curvature_matches_float64(dev, rows, Vv, layout, in_place):
    from bayeslms_amd import ops
    x = _curv_logits(rows, Vv)
    a_ref, bound = R.curvature(x)
    xv, xw = _place(x, dev, layout)
    if in_place:
        out, whole = ops.laplace_curvature(xv, out=xv), xw
        assert out.data_ptr() == xv.data_ptr()
    else:
        out, whole = _place(np.zeros_like(x), dev, layout, fill=9.0)
        assert ops.laplace_curvature(xv, out=out) is out
        assert torch.equal(xv.cpu(), torch.from_numpy(x))  # the input is left alone
    _within(out, a_ref, bound, "a = p (1 - p)")
    if Vv > 1:
        got = out.cpu().numpy()
        # the dominant column: x - lse is formed in fp32 beside |lse| about 20, whose spacing (1.9e-6) exceeds 1 - p; the bound
        # above carries that, so a may come out as 0 there
        assert got[0, Vv // 2] == 0.0 and 0 <= got[-1, 0] < 4e-6
    Vq = (Vv + 3) // 4 * 4
    if whole.shape[1] >= Vq:
        assert not whole[:, Vv:Vq].any(), "pad columns V .. Vq - 1 are written 0"
        assert torch.all(whole[:, Vq:] == (7.0 if in_place else 9.0)), "nothing past Vq is touched"
    # two runs: the same bits
    again = _place(x, dev, layout)[0]
    again = ops.laplace_curvature(again, out=again if in_place else _place(np.zeros_like(x), dev, layout)[0])
    assert torch.equal(again, out)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_curvature_nan_row_and_refusals(dev, layout):
    from bayeslms_amd import ops
    x = _curv_logits(3, 37)
    x[1, 5] = np.nan
    out = ops.laplace_curvature(_place(x, dev, layout)[0]).cpu().numpy()
    assert np.isnan(out[1]).all() and np.isfinite(out[0]).all() and np.isfinite(out[2]).all()
    xv, whole = _place(x, dev, layout)
    assert ops.laplace_curvature(xv[:0]).shape == (0, 37)
    with pytest.raises(ops.BayesLMError, match="overlap"):
        ops.laplace_curvature(whole[:2, :20], out=whole[1:3, :20])
    with pytest.raises(ops.BayesLMError, match="logits has 3 rows, out 2"):
        ops.laplace_curvature(xv, out=torch.empty(2, 37, device=dev))


@pytest.mark.parametrize("stride0", [0, 1, 5])
def test_one_row_views_take_any_row_stride(dev, stride0):
    """A (1, V) view says nothing with its row stride -- 0 after an expand, 1 or 5 out of a slice, all below V = 37: every op takes
    max(stride, V), and gives the bits of the contiguous row."""
    from bayeslms_amd import laplace, ops
    Vv, K = 37, 8
    rng = np.random.default_rng(3)
    z = (3 * rng.standard_normal((1, Vv))).astype(np.float32)
    var = rng.uniform(0, 2, (1, Vv)).astype(np.float32)
    tt = torch.tensor([5], device=dev)
    zc, vc = torch.from_numpy(z).to(dev), torch.from_numpy(var).to(dev)
    zv, vv = (t.clone().as_strided((1, Vv), (stride0, 1)) for t in (zc, vc))
    assert zv.stride(0) == stride0
    a_ref, bound = R.curvature(z)
    a = ops.laplace_curvature(zv)
    _within(a, a_ref, bound, "one row")
    assert torch.equal(a, ops.laplace_curvature(zc))
    for link in ("probit", "expexp"):
        one, two = ops.laplace_row_stats(zv, vv, tt, link), ops.laplace_row_stats(zc, vc, tt, link)
        assert all(torch.equal(x, y) for x, y in zip(one, two))
        st, _, _ = R.closed_form(z, var, [5], link)
        _within(one.nll, st["nll"][0], st["nll"][1], "one row nll")
    one, two = ops.laplace_mc_rows(zv, vv, 3, SEED, tt, 4), ops.laplace_mc_rows(zc, vc, 3, SEED, tt, 4)
    assert all(torch.equal(x, y) for x, y in zip(one, two))
    # in place, and into the posterior's sums: F of one row is a^T h^2, a single product per entry
    av = ops.laplace_curvature(zv, out=zv)
    assert av.data_ptr() == zv.data_ptr() and torch.equal(av, a)
    h = rng.standard_normal((1, K)).astype(np.float32)
    post = laplace.LaplacePosterior(Vv, K, dev)
    assert post.accumulate(av, ops._lrt_prepare(torch.from_numpy(h).to(dev), 0)) == 1
    fw, fb, bw, bb = R.fisher(_np(a), np.zeros((1, Vv)), h)
    _within(post.f_w, fw, bw, "F_W of one row")
    _within(post.f_b, fb, bb, "F_b of one row")
    post.check_finite()


# ------------------------------------------------------------------ closed-form links
def _link_inputs(rows, Vv, link, seeds=range(40, 48)):
    """z, var, targets for which the reference decides pred and rank on at least 19 rows in 20"""
    for seed in seeds:
        rng = np.random.default_rng(seed * 7919 + Vv)
        z = (3 * rng.standard_normal((rows, Vv))).astype(np.float32)
        var = rng.uniform(0.0, 2.0, (rows, Vv)).astype(np.float32)
        var[:, ::5] = 0.0
        tgt = rng.integers(0, Vv, rows)
        st, y, ey = R.closed_form(z, var, tgt, link)
        pred, rank, pok, rok = R.decided(y, ey, tgt)
        if 20 * int((~pok).sum() + (~rok).sum()) <= 2 * rows:
            return z, var, tgt, st, (pred, rank, pok, rok)
    raise AssertionError("no seed decides 19 rows in 20")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("link", ["probit", "expexp"])
@pytest.mark.parametrize("rows,Vv", VS)
def test_row_stats_matches_float64(dev, rows, Vv, link, layout):
    from bayeslms_amd import ops
    z, var, tgt, st, (pred, rank, pok, rok) = _link_inputs(rows, Vv, link)
    zt, vt = _place(z, dev, layout)[0], _place(var, dev, layout)[0]
    got = ops.laplace_row_stats(zt, vt, torch.from_numpy(tgt).to(dev), link)
    for k in ("nll", "conf", "entropy", "vbar"):
        _within(getattr(got, k), st[k][0], st[k][1], "%s %s" % (link, k))
    assert 20 * int((~pok).sum()) <= rows and 20 * int((~rok).sum()) <= rows
    assert np.array_equal(got.pred.cpu().numpy()[pok], pred[pok]) and np.array_equal(got.rank.cpu().numpy()[rok], rank[rok])
    assert got.pred.dtype == torch.int32 and got.rank.dtype == torch.int32
    # without targets: the same bits in what remains
    bare = ops.laplace_row_stats(zt, vt, None, link)
    assert bare.nll is None and bare.rank is None
    for k in ("conf", "entropy", "vbar", "pred"):
        assert torch.equal(getattr(bare, k), getattr(got, k))
    # var = 0: blm_row_stats' figures within the two bounds
    zero = torch.zeros_like(vt)
    flat, plain = ops.laplace_row_stats(zt, zero, torch.from_numpy(tgt).to(dev), link), ops.row_stats(zt, torch.from_numpy(tgt).to(dev))
    s0 = R.row_stats(R.f64(z), 0.0, tgt, np.zeros_like(z))
    for k in ("nll", "conf", "entropy"):
        _within(getattr(flat, k), s0[k][0], s0[k][1], "var = 0 %s" % k)
        _within(getattr(plain, k), _np(getattr(flat, k)), 2 * s0[k][1], "row_stats beside var = 0 %s" % k)
    assert not flat.vbar.any()


@pytest.mark.parametrize("link", ["probit", "expexp"])
def test_row_stats_bad_rows_targets_and_null_outputs(dev, link):
    from bayeslms_amd import _lib as L, ops
    z, var, tgt, st, _ = _link_inputs(5, 37, link)
    var = var.copy()
    z = z.copy()
    var[1, 3] = -1e-3
    var[2, 30] = np.nan
    z[3, 36] = np.nan
    tgt = tgt.copy()
    tgt[0], tgt[4] = -1, 37
    zt, vt, tt = torch.from_numpy(z).to(dev), torch.from_numpy(var).to(dev), torch.from_numpy(tgt).to(dev)
    got = ops.laplace_row_stats(zt, vt, tt, link)
    nll, conf, ent, vbar = (getattr(got, k).cpu().numpy() for k in ("nll", "conf", "entropy", "vbar"))
    pred, rank = got.pred.cpu().numpy(), got.rank.cpu().numpy()
    for r in (1, 2, 3):  # negative var, NaN var, NaN z: blm_row_stats' answer to a NaN row
        assert np.isnan([nll[r], conf[r], ent[r], vbar[r]]).all() and pred[r] == -1 and rank[r] == -1
    for r in (0, 4):  # a target outside [0, V): that row's nll and rank only
        assert np.isnan(nll[r]) and rank[r] == -1 and np.isfinite([conf[r], ent[r], vbar[r]]).all() and pred[r] >= 0
    # NULL outputs through the C entry: only conf asked for
    only = torch.empty(5, device=dev)
    L.calls().blm_laplace_row_stats(zt.data_ptr(), 37, vt.data_ptr(), 37, None, 5, 37, L.LAPLACE_LINKS[link], None, only.data_ptr(),
                                    None, None, None, None, L.stream())
    assert torch.equal(only[[0, 4]], got.conf[[0, 4]])
    empty = ops.laplace_row_stats(zt[:0], vt[:0], tt[:0], link)
    assert empty.nll.shape == (0,) and empty.vbar.shape == (0,)
    with pytest.raises(ops.BayesLMError, match="z has 5 rows, var 4"):
        ops.laplace_row_stats(zt, vt[:4], tt, link)
    with pytest.raises(ops.BayesLMError, match="3 targets for 5 rows"):
        ops.laplace_row_stats(zt, vt, tt[:3], link)


# ------------------------------------------------------------------ Monte-Carlo link
def _noise(ops, S, row0, rows, Vv, seed=SEED):
    return R.noise_rows(lambda n, sd, st, s: ops.philox_normal(n, sd, st, s).cpu().numpy(), seed, STREAM, S, row0, rows, Vv)


def _mc_inputs(ops, rows, Vv, S, row0, seeds=range(60, 68)):
    eps = _noise(ops, S, row0, rows, Vv)
    for seed in seeds:
        rng = np.random.default_rng(seed * 104729 + Vv)
        z = (3 * rng.standard_normal((rows, Vv))).astype(np.float32)
        var = rng.uniform(0.0, 2.0, (rows, Vv)).astype(np.float32)
        var[:, ::5] = 0.0
        tgt = rng.integers(0, Vv, rows)
        ref = R.mc_rows(z, var, tgt, eps)
        dec = R.mc_decided(ref["pbar"][0], ref["pbar"][1], tgt)
        if 20 * int((~dec[2]).sum() + (~dec[3]).sum()) <= 2 * rows:
            return z, var, tgt, ref, dec
    raise AssertionError("no seed decides 19 rows in 20")


@pytest.mark.parametrize("layout", ["aligned", "offset"])
@pytest.mark.parametrize("S", [1, 2, 5, 32])
@pytest.mark.parametrize("rows,Vv", VS)
def test_mc_rows_matches_float64(dev, rows, Vv, S, layout):
    from bayeslms_amd import ops
    row0 = 3
    z, var, tgt, ref, (pred, rank, pok, rok) = _mc_inputs(ops, rows, Vv, S, row0)
    zt, vt = _place(z, dev, layout)[0], _place(var, dev, layout)[0]
    got = ops.laplace_mc_rows(zt, vt, S, SEED, torch.from_numpy(tgt).to(dev), row0)
    for k in ("bma_nll", "nll_s", "h_pred", "mi", "conf"):
        _within(getattr(got, k), ref[k][0], ref[k][1], "mc S=%d %s" % (S, k))
    assert np.all(_np(got.mi) >= -ref["mi"][1])
    assert 20 * int((~pok).sum()) <= rows and 20 * int((~rok).sum()) <= rows
    assert np.array_equal(got.pred.cpu().numpy()[pok], pred[pok]) and np.array_equal(got.rank.cpu().numpy()[rok], rank[rok])
    assert got.nll_s.shape == (rows, S)
    # var = 0: no mutual information, and the softmax NLL
    zero = torch.zeros_like(vt)
    flat = ops.laplace_mc_rows(zt, zero, S, SEED, torch.from_numpy(tgt).to(dev), row0)
    r0 = R.mc_rows(z, np.zeros_like(z), tgt, _noise(ops, S, row0, rows, Vv))
    _within(flat.mi, 0.0, r0["mi"][1], "var = 0 mi")
    plain = ops.row_stats(zt, torch.from_numpy(tgt).to(dev))
    s0 = R.row_stats(R.f64(z), 0.0, tgt)
    _within(flat.bma_nll, r0["bma_nll"][0], r0["bma_nll"][1], "var = 0 bma_nll")
    _within(plain.nll, _np(flat.bma_nll), r0["bma_nll"][1] + s0["nll"][1], "row_stats beside var = 0 bma_nll")


@pytest.mark.parametrize("layout", ["aligned", "offset"])
@pytest.mark.parametrize("rows,Vv", [(5, 37), (5, 1000), (3, 4099)])
def test_mc_rows_invariance_bit_for_bit(dev, rows, Vv, layout):
    from bayeslms_amd import ops
    rng = np.random.default_rng(5 + Vv)
    z = (3 * rng.standard_normal((rows, Vv))).astype(np.float32)
    var = rng.uniform(0.0, 2.0, (rows, Vv)).astype(np.float32)
    tt = torch.from_numpy(rng.integers(0, Vv, rows)).to(dev)
    zt, vt = _place(z, dev, layout)[0], _place(var, dev, layout)[0]
    S, row0 = 5, 11
    one = ops.laplace_mc_rows(zt, vt, S, SEED, tt, row0)
    two = ops.laplace_mc_rows(zt, vt, S, SEED, tt, row0)
    head = ops.laplace_mc_rows(zt[:2], vt[:2], S, SEED, tt[:2], row0)
    tail = ops.laplace_mc_rows(zt[2:], vt[2:], S, SEED, tt[2:], row0 + 2)
    for k in one._fields:
        a = getattr(one, k)
        assert torch.equal(a, getattr(two, k)), "two runs: %s" % k
        assert torch.equal(a, torch.cat([getattr(head, k), getattr(tail, k)])), "rows split into two launches: %s" % k
    assert not torch.equal(one.bma_nll, ops.laplace_mc_rows(zt, vt, S, SEED, tt, row0 + 1).bma_nll)  # row0 keys the noise
    small, big = ops.laplace_mc_rows(zt, vt, 2, SEED, tt, row0), ops.laplace_mc_rows(zt, vt, 32, SEED, tt, row0)
    assert torch.equal(small.nll_s, big.nll_s[:, :2]) and torch.equal(small.nll_s, one.nll_s[:, :2])


def test_mc_rows_bad_rows_targets_and_null_outputs(dev):
    import ctypes as C
    from bayeslms_amd import _lib as L, ops
    rng = np.random.default_rng(9)
    z = rng.standard_normal((5, 37)).astype(np.float32)
    var = rng.uniform(0, 1, (5, 37)).astype(np.float32)
    var[1, 3], var[2, 30], z[3, 36] = -1e-3, np.nan, np.nan
    tgt = np.array([-1, 2, 3, 4, 37])
    zt, vt, tt = torch.from_numpy(z).to(dev), torch.from_numpy(var).to(dev), torch.from_numpy(tgt).to(dev)
    got = ops.laplace_mc_rows(zt, vt, 3, SEED, tt)
    f = {k: getattr(got, k).cpu().numpy() for k in got._fields}
    for r in (1, 2, 3):
        assert np.isnan([f["bma_nll"][r], f["h_pred"][r], f["mi"][r], f["conf"][r]]).all() and np.isnan(f["nll_s"][r]).all()
        assert f["pred"][r] == -1 and f["rank"][r] == -1
    for r in (0, 4):
        assert np.isnan(f["bma_nll"][r]) and np.isnan(f["nll_s"][r]).all() and f["rank"][r] == -1
        assert np.isfinite([f["h_pred"][r], f["mi"][r], f["conf"][r]]).all() and f["pred"][r] >= 0
    bare = ops.laplace_mc_rows(zt, vt, 3, SEED)
    assert bare.bma_nll is None and bare.nll_s is None and bare.rank is None and torch.equal(bare.h_pred[[0, 4]], got.h_pred[[0, 4]])
    only = torch.empty(5, device=dev)
    r = L.rng(SEED, L.STREAM_LAPLACE, 99)  # the step is not read
    L.calls().blm_laplace_mc_rows(zt.data_ptr(), 37, vt.data_ptr(), 37, None, 5, 37, 3, C.byref(r), 0, None, None, None, only.data_ptr(),
                                  None, None, None, L.stream())
    assert torch.equal(only[[0, 4]], got.mi[[0, 4]])
    assert ops.laplace_mc_rows(zt[:0], vt[:0], 3, SEED, tt[:0]).nll_s.shape == (0, 3)


# ------------------------------------------------------------------ through the engine
def _families(dev):
    from bayeslms_amd import model as M
    torch.manual_seed(7)
    return {"lstm": M.RNNModel("LSTM", V, W, W, 2, 0.0, True).to(dev).eval(),
            "transformer": M.TransformerModel(V, W, 2, W, 2, 0.0, "gelu", True).to(dev).eval()}


@pytest.fixture(scope="module")
def families(dev):
    return _families(dev)


@pytest.fixture(scope="module")
def text(dev):
    g = torch.Generator().manual_seed(12)
    return torch.randint(0, V, (ROWS, COLS), generator=g).to(dev)  # 3 x 41 tokens: eight windows of 5 rows


def _walk_rows(model, source):
    """the decoder-input rows, targets and plain per-token NLL of evaluate_report's walk, in walk order"""
    from bayeslms_amd import engine
    rows = []
    host, _, _, _ = engine._report_walk("test", model, source, SEQ, 0, 0, True, None, rows_out=lambda x: rows.append(x.clone()))
    return torch.cat(rows), host


def _logits64(model, h):
    """the decoder's logits in float64 from the fp32 rows, and the product's bound (K + 3) u (sum |h w| + |b|)"""
    Wt, b = _np(model.decoder.weight), _np(model.decoder.bias)
    h = _np(h)
    return h @ Wt.T + b, (h.shape[1] + 3) * U * (np.abs(h) @ np.abs(Wt).T + np.abs(b))


@pytest.mark.parametrize("family", ["lstm", "transformer"])
def test_fit_laplace_matches_the_reference_and_its_chunked_self(dev, families, text, family, monkeypatch):
    from bayeslms_amd import engine, laplace, ops
    model = families[family]
    post = engine.fit_laplace(model, text, SEQ)
    h, _ = _walk_rows(model, text)
    assert post.n_tokens == (ROWS - 1) * COLS == h.shape[0]
    z, ez = _logits64(model, h)
    a, ea = R.curvature(z, ez)
    fw, fb, bw, bb = R.fisher(a, ea, h.cpu().numpy())
    _within(post.f_w, fw, bw, "F_W")
    _within(post.f_b, fb, bb, "F_b")
    assert post.f_w.shape == (V, W) and post.manifest == laplace.manifest_of(model.decoder)
    monkeypatch.setattr(engine, "_REPORT_ROWS", 16)
    small = engine.fit_laplace(model, text, SEQ)
    assert small.n_tokens == post.n_tokens
    _within(small.f_w, _np(post.f_w), 2 * bw, "F_W in chunks of 16 rows")
    _within(small.f_b, _np(post.f_b), 2 * bb, "F_b in chunks of 16 rows")
    monkeypatch.undo()
    # chunks of 7 rows: the batch of 120 rows ends in a chunk of ONE row
    seen, real = [], ops.laplace_curvature
    monkeypatch.setattr(engine, "_REPORT_ROWS", 7)
    monkeypatch.setattr(ops, "laplace_curvature", lambda x, **k: (seen.append(x.shape[0]), real(x, **k))[1])
    odd = engine.fit_laplace(model, text, SEQ)
    monkeypatch.undo()
    assert 1 in seen and sum(seen) == post.n_tokens == odd.n_tokens
    _within(odd.f_w, _np(post.f_w), 2 * bw, "F_W in chunks of 7 rows")
    _within(odd.f_b, _np(post.f_b), 2 * bb, "F_b in chunks of 7 rows")
    few = engine.fit_laplace(model, text, SEQ, max_windows=3)
    assert few.n_tokens == 3 * SEQ * COLS and bool((few.f_b <= post.f_b * (1 + 1e-5)).all())


@pytest.mark.parametrize("family", ["lstm", "transformer"])
def test_evaluate_laplace_at_a_vanishing_variance_is_evaluate_report(dev, families, text, family, deterministic):
    from bayeslms_amd import engine, ops
    model = families[family]
    post = engine.fit_laplace(model, text, SEQ)
    base = engine.evaluate_report(model, text, SEQ)
    h, host = _walk_rows(model, text)
    logits = ops.linear(h, model.decoder.weight.detach(), model.decoder.bias.detach())
    ok = (host["tgt"] >= 0) & (host["tgt"] < V)
    assert base.skipped == 0 and ok.all()
    plain = R.row_stats(R.f64(logits.cpu().numpy()), 0.0, host["tgt"])
    for tau in (1e30, float("inf")):
        var = ops.linear(ops._lrt_prepare(h, 0), *post.inverse(tau))
        assert float(var.max()) <= 1e-25
        for link in ("probit", "expexp"):
            rep = engine.evaluate_laplace(model, text, SEQ, post, tau, link=link)
            st, _, _ = R.closed_form(logits.cpu().numpy(), var.cpu().numpy(), host["tgt"], link)
            bound = float(st["nll"][1][ok].mean() + plain["nll"][1][ok].mean())
            assert abs(rep.loss - base.loss) <= bound, (tau, link, rep.loss, base.loss, bound)
            assert rep.tokens == base.tokens and rep.skipped == 0 and rep.accuracy == base.accuracy and rep.mean_mi is None
            assert rep.laplace["prior_precision"] == tau and rep.laplace["link"] == link and rep.laplace["tokens"] == post.n_tokens
            assert rep.laplace["mean_vbar"] <= 1e-25 and "laplace" in rep.as_dict() and "laplace" not in base.as_dict()
        mc = engine.evaluate_laplace(model, text, SEQ, post, tau, link="mc", samples=3, seed=5)
        eps = R.noise_rows(lambda n, sd, stq, s: ops.philox_normal(n, sd, stq, s).cpu().numpy(), 5, STREAM, 3, 0, h.shape[0], V)
        ref = R.mc_rows(logits.cpu().numpy(), var.cpu().numpy(), host["tgt"], eps)
        assert abs(mc.loss - base.loss) <= float(ref["bma_nll"][1].mean() + plain["nll"][1].mean())
        assert abs(mc.mean_mi) <= float(ref["mi"][1].mean()) and mc.mc_samples == 3 and len(mc.sample_loss) == 3


@pytest.mark.parametrize("family", ["lstm", "transformer"])
def test_evaluate_laplace_matches_the_reference_and_does_not_depend_on_the_chunks(dev, families, text, family, deterministic, monkeypatch):
    from bayeslms_amd import engine, ops
    model = families[family]
    post = engine.fit_laplace(model, text, SEQ)
    h, host = _walk_rows(model, text)
    ok = (host["tgt"] >= 0) & (host["tgt"] < V)
    logits = ops.linear(h, model.decoder.weight.detach(), model.decoder.bias.detach()).cpu().numpy()
    var = ops.linear(ops._lrt_prepare(h, 0), *post.inverse(2.0)).cpu().numpy()
    assert var.min() > 0
    reps = {}
    for link in ("probit", "expexp"):
        rep = reps[link] = engine.evaluate_laplace(model, text, SEQ, post, 2.0, link=link, keep_tokens=True)
        st, _, _ = R.closed_form(logits, var, host["tgt"], link)
        assert abs(rep.loss - st["nll"][0][ok].mean()) <= st["nll"][1][ok].mean()
        assert abs(rep.mean_entropy - st["entropy"][0][ok].mean()) <= st["entropy"][1][ok].mean()
        assert abs(rep.laplace["mean_vbar"] - st["vbar"][0][ok].mean()) <= st["vbar"][1][ok].mean()
        assert rep.per_token["nll"].shape == ((ROWS - 1) * COLS,)
    mc = engine.evaluate_laplace(model, text, SEQ, post, 2.0, link="mc", samples=4, seed=9, keep_tokens=True)
    eps = R.noise_rows(lambda n, sd, stq, s: ops.philox_normal(n, sd, stq, s).cpu().numpy(), 9, STREAM, 4, 0, h.shape[0], V)
    ref = R.mc_rows(logits, var, host["tgt"], eps)
    assert abs(mc.loss - ref["bma_nll"][0][ok].mean()) <= ref["bma_nll"][1][ok].mean()
    assert abs(mc.mean_mi - ref["mi"][0][ok].mean()) <= ref["mi"][1][ok].mean() and mc.mean_mi > 0
    assert abs(mc.mean_h_pred - ref["h_pred"][0][ok].mean()) <= ref["h_pred"][1][ok].mean()
    for chunk in (16, 7):  # 7: the batch of 120 rows ends in a chunk of one row
        monkeypatch.setattr(engine, "_REPORT_ROWS", chunk)
        again = engine.evaluate_laplace(model, text, SEQ, post, 2.0, link="mc", samples=4, seed=9, keep_tokens=True)
        for k in ("nll", "mi", "h_pred", "nll_s", "rank"):  # the chunking moves no bit: row0 keys the noise by the global row
            assert np.array_equal(again.per_token[k], mc.per_token[k], equal_nan=True), k
        assert again.loss == mc.loss
        for link in ("probit", "expexp"):  # one workgroup per row: a row's figures do not know its chunk
            part = engine.evaluate_laplace(model, text, SEQ, post, 2.0, link=link, keep_tokens=True)
            assert np.array_equal(part.per_token["nll"], reps[link].per_token["nll"]) and part.loss == reps[link].loss


def test_fit_laplace_prior_never_exceeds_the_model(dev, families, text, deterministic):
    from bayeslms_amd import engine
    model = families["transformer"]
    post = engine.fit_laplace(model, text, SEQ)
    for kw in (dict(link="probit"), dict(link="expexp"), dict(link="mc", samples=2)):
        fit = engine.fit_laplace_prior(model, text, SEQ, post, [0.5, 5.0, 500.0], **kw)
        assert fit.loss <= fit.loss_base and len(fit.curve) == 4 and fit.curve[0][0] == float("inf") and fit.curve[0][1] == fit.loss_base
        assert fit.tau in (float("inf"), 0.5, 5.0, 500.0) and fit.loss == min(c[1] for c in fit.curve)
        one = engine.evaluate_laplace(model, text, SEQ, post, fit.tau, **kw)
        assert one.loss == fit.loss  # the candidate alone: the same kernels on the same rows


def test_a_walk_that_raises_leaves_the_model_as_found(dev, families, text, monkeypatch):
    from bayeslms_amd import engine, ops
    model = families["lstm"]
    post = engine.fit_laplace(model, text, SEQ)
    model.train()
    model.decoder.eval()
    flags = [m.training for m in model.modules()]
    hooks = (ops._GRAD_HOOK, ops._EMBED_SINK, ops._STATE_TAP, ops._TIMER)
    calls = [0]
    real = ops.laplace_row_stats

    def failing(*a, **k):
        calls[0] += 1
        if calls[0] == 2:
            raise RuntimeError("thrown by the test")
        return real(*a, **k)

    monkeypatch.setattr(ops, "laplace_row_stats", failing)
    monkeypatch.setattr(engine, "_REPORT_ROWS", 16)
    try:
        for run in (lambda: engine.evaluate_laplace(model, text, SEQ, post, 1.0),
                    lambda: engine.fit_laplace_prior(model, text, SEQ, post, [1.0])):
            calls[0] = 0
            with pytest.raises(RuntimeError, match="thrown by the test"):
                run()
            assert [m.training for m in model.modules()] == flags
            dec = model.decoder
            assert not dec._scope and dec.return_input is False and dec.rows is None and dec.nll_targets is None
            assert (ops._GRAD_HOOK, ops._EMBED_SINK, ops._STATE_TAP, ops._TIMER) == hooks
        monkeypatch.setattr(ops, "laplace_curvature", failing)
        calls[0] = 1
        with pytest.raises(RuntimeError, match="thrown by the test"):
            engine.fit_laplace(model, text, SEQ)
        assert [m.training for m in model.modules()] == flags and not model.decoder._scope
        monkeypatch.undo()
        rep = engine.evaluate_laplace(model, text, SEQ, post, 1.0)  # and a walk that returns leaves it as found too
        assert [m.training for m in model.modules()] == flags and rep.tokens == (ROWS - 1) * COLS
    finally:
        model.eval()


# ------------------------------------------------------------------ the command line
def _corpus(tmp_path):
    d = str(tmp_path)
    words = ["<s>", "<unk>"] + ["w%d" % i for i in range(38)]
    with open(os.path.join(d, "words.txt"), "w") as f:
        f.write("".join("%s %d\n" % (w, i) for i, w in enumerate(words)))
    g = torch.Generator().manual_seed(4)
    for split, n in (("train", 40), ("valid", 12), ("test", 12)):
        with open(os.path.join(d, split + ".txt"), "w") as f:
            for _ in range(n):
                f.write(" ".join(words[2 + int(i)] for i in torch.randint(0, 38, (7,), generator=g) ** 2 // 38) + "\n")
    return d


def _evaluate(argv):
    env = dict(os.environ, BLM_DETERMINISTIC="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "bayeslms_amd.evaluate"] + argv, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.strip()


def test_evaluate_command_line_in_child_processes(dev, tmp_path, deterministic):
    from bayeslms_amd import evaluate as E, laplace, model as M
    d = _corpus(tmp_path)
    torch.manual_seed(3)
    model = M.RNNModel("LSTM", 40, 32, 32, 2, 0.0, True)
    pt, lp = os.path.join(d, "model.pt"), os.path.join(d, "laplace.pt")
    torch.save(model.state_dict(), pt)
    rj = [os.path.join(d, "r%d.json" % i) for i in range(3)]
    base = ["--model-path", pt, "--vocabulary", os.path.join(d, "words.txt"), "--data", os.path.join(d, "test.txt"),
            "--emsize", "32", "--nhid", "32", "--seq-len", "5", "--batch-size", "2"]
    plain = "| evaluate | tokens \\d+ | skipped 0 | loss [\\d.]+ | ppl [\\d.]+ | accuracy [\\d.]+ | top5 [\\d.]+ | ece [\\d.]+"
    # fit, save, pick the prior on the validation text, evaluate
    line = _evaluate(base + ["--laplace-fit-on", os.path.join(d, "train.txt"), "--laplace-fit-windows", "20", "--laplace-save", lp,
                             "--fit-laplace-prior-on", os.path.join(d, "valid.txt"), "--laplace-prior-grid", "1,100", "--write-report", rj[0]])
    assert re.fullmatch(plain.replace("|", "\\|") + r" \| laplace tokens 200 prior (inf|1|100) link probit \| fit loss [\d.]+ -> [\d.]+", line), line
    block = json.load(open(rj[0]))["laplace"]
    assert block["tokens"] == 200 and block["shape"] == [40, 32] and block["link"] == "probit" and block["samples"] == 0
    assert block["path"] == lp and block["fitted_on"].endswith("valid.txt") and block["fit_loss_after"] <= block["fit_loss_before"]
    assert len(block["curve"]) == 3 and block["prior_precision"] in ("inf", 1.0, 100.0) and block["curve"][0][0] == "inf"
    json.loads(open(rj[0]).read(), parse_constant=lambda name: pytest.fail("the report holds the token %s: not JSON" % name))
    post = laplace.LaplacePosterior.load(lp)
    assert post.n_tokens == 200 and post.manifest["fingerprint"].startswith(block["fingerprint"])
    # load it, Monte-Carlo link
    line = _evaluate(base + ["--laplace", lp, "--laplace-prior-precision", "10", "--laplace-link", "mc", "--laplace-samples", "4",
                             "--mc-seed", "3", "--write-report", rj[1], "--write-tokens", os.path.join(d, "tok.txt")])
    assert re.fullmatch(plain.replace("|", "\\|") + r" \| mc samples 4 \| sample loss [\d.]+ \| h_pred [\d.]+ \| mi [\d.]+"
                        r" \| laplace tokens 200 prior 10 link mc samples 4", line), line
    rep = json.load(open(rj[1]))
    assert rep["mc_samples"] == 4 and len(rep["sample_loss"]) == 4 and rep["mean_mi"] > 0
    assert rep["laplace"]["seed"] == 3 and rep["laplace"]["path"] == lp and rep["laplace"]["prior_precision"] == 10.0
    assert len(open(os.path.join(d, "tok.txt")).readline().split()) == 7
    # without the flags: the line and the report in the format they always had
    line = _evaluate(base + ["--write-report", rj[2]])
    assert re.fullmatch(plain.replace("|", "\\|"), line), line
    text = open(rj[2]).read()
    here = E.main(base)
    assert line == E.summary_line(here) == "| evaluate | tokens %d | skipped %d | loss %.4f | ppl %.2f | accuracy %.4f | top5 %.4f | ece %.4f" % (
        here.tokens, here.skipped, here.loss, here.ppl, here.accuracy, here.top5_accuracy, here.ece)
    assert list(json.loads(text)) == ["tokens", "skipped", "loss", "ppl", "mc_samples", "accuracy", "top5_accuracy", "mean_conf",
                                      "mean_entropy", "ece", "bins", "sample_loss", "sample_loss_mean", "mean_h_pred", "mean_mi"]
    assert text == json.dumps(here.as_dict())
    # a posterior of another checkpoint is refused by field
    torch.manual_seed(4)
    torch.save(M.RNNModel("LSTM", 40, 32, 32, 2, 0.0, True).state_dict(), os.path.join(d, "other.pt"))
    with pytest.raises(SystemExit, match="field 'fingerprint' differs"):
        E.main(["--model-path", os.path.join(d, "other.pt")] + base[2:] + ["--laplace", lp, "--laplace-prior-precision", "1"])
