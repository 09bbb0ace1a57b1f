"""GPU: the kernels that write the parameters -- blm_sqnorm_multi + sum_kernel, blm_clip_sgd_multi(_wd), blm_adam_step,
blm_rows_gather_add, blm_init_multi, blm_axpy, blm_colsum / blm_colsum2 -- against the float64 reference of
tests/update_reference.py, at the sizes the trainer uses: the n == 1 grids of a flat parameter buffer past the first round of
every grid-stride loop, the scalar paths behind a pointer at a storage offset of 1-3 floats, tails of 1-3 elements, the
unclipped step, grad_scale != 1, `first` over a buffer of NaN, Adam at a late step and on zero gradients.

Every error is bounded PER ELEMENT by K * 2^-24 * magnitude, K the number of roundings on the longest path through the kernel
(counted from the source in update_reference.py, next to each constant), never by a global maximum.  Every in-place operand
lives in a slab between guard floats that must come back bit-identical, and read-only operands must be unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import update_reference as R

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = np.float32(-77777.75)
U = R.U


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Slab:
    """Tensors carved out of one device buffer, each starting ``off`` floats past a 16-byte boundary (``offs``: one value or one
    per tensor), with at least GUARD sentinel floats before and after each.  Everything that is not a tensor is guard."""

    def __init__(self, dev, sizes, offs=0):
        offs = [offs] * len(sizes) if isinstance(offs, int) else list(offs)
        pos, self.spans = 0, []
        for n, off in zip(sizes, offs):
            start = (pos + GUARD + 3) // 4 * 4 + off
            self.spans.append((start, int(n)))
            pos = start + int(n) + GUARD
        self.host = np.full(pos + GUARD, SENTINEL, np.float32)
        self.guard = np.ones(self.host.size, bool)
        for s, n in self.spans:
            self.guard[s:s + n] = False
        self.dev, self.t = dev, None

    def fill(self, arrays):
        for (s, n), a in zip(self.spans, arrays):
            self.host[s:s + n] = np.asarray(a, np.float32).reshape(-1)
        return self

    def upload(self):
        self.t = torch.from_numpy(self.host).to(self.dev)
        assert self.t.data_ptr() % 16 == 0
        self.views = [self.t[s:s + n] for s, n in self.spans]
        for v, (s, n) in zip(self.views, self.spans):
            assert n == 0 or v.data_ptr() == self.t.data_ptr() + 4 * s
        return self

    def download(self):
        """-> the tensors as the device holds them now, after checking that every guard float is bit-identical."""
        now = self.t.cpu().numpy()
        bad = np.nonzero(bits(now)[self.guard] != bits(SENTINEL.reshape(1))[0])[0]
        assert bad.size == 0, "guard floats overwritten at slab positions %s" % np.nonzero(self.guard)[0][bad][:8]
        return [now[s:s + n].copy() for s, n in self.spans]

    def unchanged(self):
        """A read-only operand: the whole slab is bit-identical to what was uploaded."""
        assert np.array_equal(bits(self.t.cpu().numpy()), bits(self.host))


def within(got, ref, err, what):
    """|got - ref| <= err element by element (NaN fails); reports the worst element against its bound."""
    got, ref, err = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(err, np.float64)
    assert got.shape == ref.shape == err.shape, what
    d = np.abs(got - ref)
    ok = d <= err
    if not ok.all():
        i = int(np.argmax(np.where(ok, 0.0, np.where(np.isnan(d), np.inf, d / (err + 1e-300)))))
        raise AssertionError("%s: element %d of %d: got %r, reference %r, |diff| %.3e > bound %.3e (%d outside)"
                             % (what, i, got.size, got.reshape(-1)[i], ref.reshape(-1)[i], d.reshape(-1)[i],
                                err.reshape(-1)[i], int((~ok).sum())))


# ------------------------------------------------------------------------------------------------- norm + clip + SGD momentum
LR, MOM = 0.25, 0.9
GS = (1.0, 0.5, 1.0 / 3.0)
WD = (0.0, 1e-2)
ALIGNED, G_OFF1, M_OFF3, P_OFF2 = (0, 0, 0), (0, 1, 0), (0, 0, 3), (2, 0, 0)  # storage offsets of p, g, m in floats

# n == 1: the form engine.Trainer runs (one flat buffer): 1024 workgroups for the norm, 2048 for the update.  One round of the
# norm's vector loop is 1,048,576 floats, one of the update's 2,097,152; the scalar loops go round every 262,144 / 524,288.
N1_SIZES = (1, 3, 4, 5, 1023, 1048576, 1048576 + 5, 2097152, 2097152 + 3 * 1024 + 3, 3200003)


def _n1_cases():
    cases = []
    for i, n in enumerate(N1_SIZES):  # every size: aligned and clipped, then misaligned and unclipped
        cases.append((n, ALIGNED, True, GS[i % 3], WD[i % 2]))
        cases.append((n, G_OFF1 if i % 2 == 0 else M_OFF3, False, GS[(i + 1) % 3], WD[(i + 1) % 2]))
    cases += [  # the other two pairings at the sizes where the loops turn, and p alone misaligned
        (5, ALIGNED, False, 1.0, 0.0), (5, G_OFF1, True, 0.5, 1e-2), (1023, M_OFF3, True, 1.0 / 3.0, 0.0),
        (1048576 + 5, G_OFF1, True, 1.0, 1e-2), (2097152, ALIGNED, False, 1.0 / 3.0, 1e-2),
        (2097152 + 3 * 1024 + 3, M_OFF3, True, 0.5, 0.0), (3200003, ALIGNED, False, 1.0, 0.0), (4, P_OFF2, True, 1.0, 0.0)]
    return cases


def _id(case):
    n, offs, clipped, gs, wd = case
    return "%s-p%dg%dm%d-%s-gs%.2f-wd%g" % (n if isinstance(n, int) else "n%d" % len(n), offs[0], offs[1], offs[2],
                                            "clipped" if clipped else "unclipped", gs, wd)


def _run_clip_sgd(dev, sizes, offs, clipped, gs, wd, steps, seed):
    """``steps`` consecutive steps through ops.PtrTable / ops.clip_sgd, the first with first=True over momentum buffers of NaN.
    Each step is compared with the reference applied to the float32 state the kernel started that step from."""
    from bayeslms_amd import ops
    from bayeslms_amd._lib import calls, ptr, stream
    rng = np.random.default_rng(seed)
    P, G, M = Slab(dev, sizes, offs[0]), Slab(dev, sizes, offs[1]), Slab(dev, sizes, offs[2])
    g_host = [rng.standard_normal(n, dtype=np.float32) * np.float32(3.0) for n in sizes]
    P.fill([rng.standard_normal(n, dtype=np.float32) for n in sizes]).upload()
    G.fill(g_host).upload()
    M.fill([np.full(n, np.nan, np.float32) for n in sizes]).upload()  # garbage: `first` must not read it
    table = ops.PtrTable(P.views, G.views, M.views)
    assert table.n == len(sizes) and table.ws.numel() == (1024 if len(sizes) == 1 else 64 * len(sizes))
    sq_ref, _ = R.sqnorm(g_host)
    # far below / far above the norm of the scaled gradient: no doubt about which branch fminf takes
    clip = np.sqrt(sq_ref) * R.f32(gs) * (0.01 if clipped else 100.0)
    p0, m0 = P.download(), M.download()
    sq_bits = []
    for step in range(steps):
        first = step == 0
        sq = ops.clip_sgd(table, clip, LR, MOM, first, gs, wd)
        sq_gpu = float(sq.item())
        p1, m1 = P.download(), M.download()  # guards checked here
        G.unchanged()
        ref = R.clip_sgd(p0, g_host, m0, clip, LR, MOM, first, gs, wd)
        assert ref["clipped"] == clipped
        # K_SQNORM roundings on the longest chain of additions, all terms >= 0: relative to the sum
        assert abs(sq_gpu - ref["sq"]) <= R.K_SQNORM * U * ref["sq"], (sq_gpu, ref["sq"])
        sq_bits.append(int(bits(np.float32(sq_gpu).reshape(1))[0]))
        for i, n in enumerate(sizes):
            what = "step %d tensor %d (%d floats)" % (step, i, n)
            assert np.isfinite(p1[i]).all() and np.isfinite(m1[i]).all(), what
            # K_C on the c*g term and K_TERM on the others when the clip is active, K_UNCLIPPED throughout when not
            within(m1[i], ref["buf"][i], ref["buf_err"][i], what + " momentum")
            within(p1[i], ref["p"][i], ref["p_err"][i], what + " parameter")
            if not clipped:
                # plain momentum SGD with c == grad_scale exactly, K_UNCLIPPED = 4 roundings on every term
                p64, g64 = p0[i].astype(np.float64), g_host[i].astype(np.float64)
                old = 0.0 * p64 if first else R.f32(MOM) * m0[i].astype(np.float64)
                buf = old + R.f32(gs) * g64 + R.f32(wd) * p64
                buf_mag = np.abs(old) + np.abs(R.f32(gs) * g64) + np.abs(R.f32(wd) * p64)
                within(m1[i], buf, 4 * U * buf_mag, what + " momentum, plain SGD")
                within(p1[i], p64 - R.f32(LR) * buf, 4 * U * (np.abs(p64) + R.f32(LR) * buf_mag), what + " parameter, plain SGD")
        p0, m0 = p1, m1
    # the header promises a fixed order of additions: the same gradients give the same bits, here and in a run of its own
    table.sq.zero_()
    calls().blm_sqnorm_multi(ptr(table.grads), ptr(table.sizes), table.n, ptr(table.sq), ptr(table.ws), stream())
    sq_bits.append(int(bits(table.sq.cpu().numpy())[0]))
    assert len(set(sq_bits)) == 1, sq_bits


@pytest.mark.parametrize("case", _n1_cases(), ids=_id)
def test_clip_sgd_one_flat_buffer(dev, case):
    n, offs, clipped, gs, wd = case
    _run_clip_sgd(dev, [n], offs, clipped, gs, wd, steps=3 if n <= 1023 else 2, seed=n % 1000 + 7 * offs[1] + offs[2])


# n == 40: 64 workgroups per tensor (one round of the vector loop is 65,536 floats), 2560 partials: sum_kernel goes round
# more than once.  The empty tensor must change nothing.
N40_SIZES = ([1, 2, 3, 7, 64, 1000, 4096, 65536, 65536 + 7, 200003] * 4)[:39]
N40_SIZES.insert(17, 0)


@pytest.mark.parametrize("case", [(N40_SIZES, ALIGNED, True, 1.0 / 3.0, 0.0), (N40_SIZES, G_OFF1, False, 0.5, 1e-2),
                                  (N40_SIZES, M_OFF3, True, 1.0, 1e-2), (N40_SIZES, ALIGNED, False, 1.0, 0.0)], ids=_id)
def test_clip_sgd_forty_tensors(dev, case):
    sizes, offs, clipped, gs, wd = case
    assert len(sizes) == 40 and sizes.count(0) == 1
    _run_clip_sgd(dev, sizes, offs, clipped, gs, wd, steps=3, seed=40 + offs[1] + offs[2])


# ----------------------------------------------------------------------------------------------------------------------- Adam
ADAM = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8)


@pytest.mark.parametrize("n,wd,late,offs", [
    (16, 0.0, False, (0, 0, 0, 0)), (16, 1e-3, True, (0, 0, 0, 0)), (524288, 1e-3, False, (0, 0, 0, 0)),
    (524288, 0.0, True, (0, 0, 0, 1)), (524289, 0.0, False, (1, 0, 0, 0)), (524289, 1e-3, True, (0, 0, 1, 0)),
    (1300001, 0.0, False, (0, 1, 0, 0)), (1300001, 1e-3, True, (0, 0, 0, 0))])
def test_adam_step(dev, n, wd, late, offs):
    """blm_adam_step: steps 1-3 from zero state, or step 10000 from random m and v >= 0 (bc1 rounds to 1).  One round of the
    grid-stride loop is 2048 * 256 = 524,288 floats.  A tenth of the gradient is exactly zero; with m = v = 0 and no weight
    decay the update there is lr * 0 / (0 + eps) = 0 and p must come back bit-identical."""
    from bayeslms_amd import ops
    rng = np.random.default_rng(n + late)
    g = rng.standard_normal(n, dtype=np.float32)
    zero = np.arange(n) % 10 == 3
    g[zero] = 0.0
    if late:
        m0 = rng.standard_normal(n, dtype=np.float32) * np.float32(0.1)
        v0 = rng.random(n, dtype=np.float32) * np.float32(0.5)
    else:
        m0, v0 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    P, G, M, V = (Slab(dev, [n], o) for o in offs)
    P.fill([rng.standard_normal(n, dtype=np.float32)]).upload()
    G.fill([g]).upload()
    M.fill([m0]).upload()
    V.fill([v0]).upload()
    p0 = P.download()[0]
    for step in ([10000] if late else [1, 2, 3]):
        ops.adam_step(P.views[0], G.views[0], M.views[0], V.views[0], step, ADAM["lr"], ADAM["betas"], ADAM["eps"], wd)
        p1, m1, v1 = P.download()[0], M.download()[0], V.download()[0]
        G.unchanged()
        ref = R.adam(p0, g, m0, v0, step, ADAM["lr"], ADAM["betas"][0], ADAM["betas"][1], ADAM["eps"], wd)
        what = "step %d" % step
        # K_ADAM_M / K_ADAM_V roundings (+ K_ADAM_GV on g + wd*p); K_ADAM = 16 on the update term, one rounding on p, and the
        # moments' own bounds carried through 1 / bc1 / (sqrt(v / bc2) + eps): update_reference.adam
        within(m1, ref["m"], ref["m_err"], what + " m")
        within(v1, ref["v"], ref["v_err"], what + " v")
        within(p1, ref["p"], ref["p_err"], what + " p")
        assert (v1 >= 0).all()
        if wd == 0.0 and not late:
            assert np.array_equal(bits(p1[zero]), bits(p0[zero])) and not m1[zero].any() and not v1[zero].any()
            assert (p1[~zero] != p0[~zero]).mean() > 0.99
        p0, m0, v0 = p1, m1, v1


# ------------------------------------------------------------------------------------------------------------ rows_gather_add
@pytest.mark.parametrize("V,D,dst_off,src_off", [(1, 1, 0, 0), (5, 4, 0, 0), (7, 260, 0, 0), (33, 256, 0, 0), (33, 256, 1, 0),
                                                 (1001, 1024, 0, 0), (6, 130, 0, 0), (5, 4, 0, 3)])
def test_rows_gather_add(dev, V, D, dst_off, src_off):
    """dst[v,:] += src[slot[v],:] where 0 <= slot[v] < n_src: one addition per element, so the float32 numpy sum bit for bit;
    rows whose slot is -1 or >= n_src are bit-identical to before.  The vector path needs D % 4 == 0 and both bases aligned."""
    from bayeslms_amd import ops
    rng = np.random.default_rng(V * 7 + D)
    n_src = max(1, V // 3)
    rows_src = n_src + 3  # rows behind n_src exist in memory and must not be gathered
    slot = rng.choice(np.array([-1, -1, n_src, n_src + 2, 1 << 40] + list(range(n_src)) * 2, dtype=np.int64), size=V)
    if V == 1:
        slot[0] = 0
    else:
        slot[0], slot[1], slot[-1] = n_src - 1, n_src - 1, n_src  # a repeat, and the first index out of range
    dst0, src = rng.standard_normal((V, D), dtype=np.float32), rng.standard_normal((rows_src, D), dtype=np.float32)
    Dst, Src = Slab(dev, [V * D], dst_off).fill([dst0]).upload(), Slab(dev, [rows_src * D], src_off).fill([src]).upload()
    ops.rows_gather_add(Dst.views[0].view(V, D), torch.from_numpy(slot).to(dev), Src.views[0].view(rows_src, D), n_src)
    got = Dst.download()[0].reshape(V, D)
    Src.unchanged()
    ref, mag, touched = R.rows_gather_add(dst0, slot, src, n_src)
    want = dst0.copy()
    want[touched] = dst0[touched] + src[slot[touched]]  # float32 + float32, rounded once
    assert np.array_equal(want.astype(np.float64), ref.astype(np.float32).astype(np.float64))
    assert np.array_equal(bits(got[~touched]), bits(dst0[~touched]))
    assert np.array_equal(bits(got), bits(want))
    assert V == 1 or (touched.any() and not touched.all())


# ---------------------------------------------------------------------------------------------------------------- init_multi
BIG = 1048576 + 4  # one round of init_multi's vector loop is 1024 * 256 * 4 floats


def _init_items(dev, count, seed):
    """``count`` items over the sizes 0, 1, 5, 4096 and (once) BIG, cycling through the source combinations: both, src only,
    src2 only, neither (a zero fill), dst is src2 (in place).  Item 3, of 4096 floats, starts one float past a 16-byte boundary:
    the scalar path although n % 4 == 0.  -> (slab, items, expected float32 results, (device tensor, host copy) per source)."""
    rng = np.random.default_rng(seed)
    sizes = [(0, 1, 5, 4096)[i % 4] for i in range(count)]
    sizes[count // 2] = BIG
    if count > 1:
        sizes[-1] = 4096  # the vector path with a short tail of lanes, next to the long item in the same launch
    offs = [1 if i == 3 else 0 for i in range(count)]
    slab = Slab(dev, sizes, offs)
    before = [rng.standard_normal(n, dtype=np.float32) for n in sizes]
    slab.fill(before).upload()
    items, wants, sources = [], [], []
    for i, n in enumerate(sizes):
        a, b = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        combo = (i + count) % 5
        if combo == 0:
            item, pair = (slab.views[i], ta, tb), (a, b)
        elif combo == 1:
            item, pair = (slab.views[i], ta, None), (a, None)
        elif combo == 2:
            item, pair = (slab.views[i], None, tb), (None, b)
        elif combo == 3:
            item, pair = (slab.views[i], None, None), (None, None)
        else:
            item, pair = (slab.views[i], ta, slab.views[i]), (a, before[i])  # grad = db + grad, in place
        items.append(item)
        sources += [(t, h) for t, h in ((ta, a), (tb, b))]
        ref, _ = R.init_multi(n, *pair)
        want = (np.zeros(n, np.float32) if pair[0] is None else pair[0]) + (np.zeros(n, np.float32) if pair[1] is None else pair[1])
        assert np.array_equal(ref.astype(np.float32), want)  # one addition per element: the float32 sum is the rounded float64 one
        wants.append(want)
    return slab, items, wants, sources


def _check_init(slab, wants, sources):
    got = slab.download()
    for i, (g, w) in enumerate(zip(got, wants)):
        assert np.array_equal(bits(g), bits(w)), "item %d of %d floats" % (i, w.size)
    for t, h in sources:
        assert np.array_equal(bits(t.cpu().numpy()), bits(h))


@pytest.mark.parametrize("count", [1, 8, 9, 17])
def test_init_multi_through_ops(dev, count):
    """ops._init_multi chunks the items by eight: 9 items are two launches, 17 are three."""
    from bayeslms_amd import ops
    slab, items, wants, sources = _init_items(dev, count, count)
    ops._init_multi(items)
    _check_init(slab, wants, sources)


@pytest.mark.parametrize("count", [1, 8])
def test_init_multi_through_the_abi(dev, count):
    from bayeslms_amd._lib import calls, ptr, stream
    slab, items, wants, sources = _init_items(dev, count, 100 + count)
    d, a, b, n = (C.c_void_p * 8)(), (C.c_void_p * 8)(), (C.c_void_p * 8)(), (C.c_int64 * 8)()
    for i, (dst, s1, s2) in enumerate(items):
        d[i], a[i], b[i], n[i] = ptr(dst), ptr(s1), ptr(s2), dst.numel()
    calls().blm_init_multi(count, d, a, b, n, stream())
    _check_init(slab, wants, sources)
    # src / src2 NULL altogether: a zero fill of every item
    calls().blm_init_multi(count, d, None, None, n, stream())
    _check_init(slab, [np.zeros_like(w) for w in wants], sources)


def test_init_multi_refuses_nine_items(dev):
    from bayeslms_amd._lib import BayesLMError, calls, stream
    slab = Slab(dev, [4] * 9).fill([np.ones(4, np.float32)] * 9).upload()
    d, n = (C.c_void_p * 9)(), (C.c_int64 * 9)()
    for i in range(9):
        d[i], n[i] = slab.views[i].data_ptr(), 4
    with pytest.raises(BayesLMError, match="blm_init_multi: bad arguments \\(at most 8 vectors\\)") as e:
        calls().blm_init_multi(9, d, None, None, n, stream())
    assert e.value.status != 0
    assert all(np.array_equal(t, np.ones(4, np.float32)) for t in slab.download())  # refused before anything was written


# ---------------------------------------------------------------------------------------------------------------------- axpy
@pytest.mark.parametrize("n,x_off,y_off", [(1, 0, 0), (524288, 0, 0), (524289, 0, 1), (1300001, 1, 0)])
@pytest.mark.parametrize("a", [1.0, -0.5, 0.0])
def test_axpy(dev, n, x_off, y_off, a):
    """y += a*x straight through the ABI; one round of the grid-stride loop is 2048 * 256 = 524,288 floats.  K_AXPY = 2: the
    product and the addition."""
    from bayeslms_amd import _lib as L
    rng = np.random.default_rng(n)
    x, y0 = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    X, Y = Slab(dev, [n], x_off).fill([x]).upload(), Slab(dev, [n], y_off).fill([y0]).upload()
    L.check(L.lib().blm_axpy(L.ptr(X.views[0]), L.ptr(Y.views[0]), n, a, L.stream()), "blm_axpy")
    got = Y.download()[0]
    X.unchanged()
    ref, mag = R.axpy(x, y0, a)
    within(got, ref, R.K_AXPY * U * mag, "axpy a=%g" % a)
    if a == 0.0:
        assert np.array_equal(got, y0)


# ---------------------------------------------------------------------------------------------------------- colsum / colsum2
COLSUM_SHAPES = [(1, 1, 1, 0), (7, 3, 3, 0), (8, 4, 4, 0), (300, 70, 70, 0), (300, 70, 72, 0), (300, 70, 72, 1), (257, 131, 131, 0),
                 (20000, 129, 132, 0)]  # (M, N, ld, storage offset of x); 20000 rows are 64 row chunks


def _colsum(dev, M, N, ld, x_off, accumulate, two, seed, same_start=False):
    """One call of blm_colsum (``two`` False) or blm_colsum2 over fresh operands -> the output vector(s) and the reference.
    The vectors hold non-zero values beforehand (different ones unless ``same_start``)."""
    from bayeslms_amd._lib import calls, ptr, stream
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, ld), dtype=np.float32)
    o0 = [rng.standard_normal(N, dtype=np.float32), rng.standard_normal(N, dtype=np.float32)]
    if same_start:
        o0[1] = o0[0].copy()
    X = Slab(dev, [M * ld], x_off).fill([x]).upload()
    O = Slab(dev, [N, N]).fill(o0).upload()
    if two:
        calls().blm_colsum2(ptr(X.views[0]), ld, ptr(O.views[0]), ptr(O.views[1]), M, N, accumulate, stream())
    else:
        calls().blm_colsum(ptr(X.views[0]), ld, ptr(O.views[0]), M, N, accumulate, stream())
    got = O.download()
    X.unchanged()
    refs = [R.colsum(x[:, :N], o0[k] if accumulate else None) for k in range(2)]
    if not two:
        assert np.array_equal(bits(got[1]), bits(o0[1]))
    return got, refs


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("M,N,ld,x_off", COLSUM_SHAPES)
def test_colsum(dev, M, N, ld, x_off, accumulate):
    """out (+)= column sums, alone and with a second vector from the same pass.  K = rows added per lane + 8 + row chunks
    (update_reference.colsum_k), per column against sum |x| (+ |out| when accumulating onto a non-zero vector).  Written, not
    accumulated, the two vectors of blm_colsum2 are ONE sum: bit-identical to each other at any number of row chunks.  (The
    64 chunks of the 20000-row case showed them apart in the last bits while each took the float atomics in its own order.)
    The vector of a blm_colsum call of its own is another run of the atomics and only shares the bound."""
    k = R.colsum_k(M)
    one = _colsum(dev, M, N, ld, x_off, accumulate, False, M + N)[0][0]
    got, refs = _colsum(dev, M, N, ld, x_off, accumulate, True, M + N)
    for j, name in ((0, "out"), (1, "out2")):
        within(got[j], refs[j][0], k * U * refs[j][1], "colsum2 %s" % name)
    within(one, refs[0][0], k * U * refs[0][1], "colsum out")
    if not accumulate:  # with accumulate the two vectors start from different values
        assert np.array_equal(bits(got[0]), bits(got[1]))
        if M <= 512:  # at most two row chunks onto zero: 0 + a + b == 0 + b + a, whichever atomic lands first
            assert np.array_equal(bits(one), bits(got[0]))


@pytest.mark.parametrize("M,N,ld,x_off", [(300, 70, 72, 1), (257, 131, 131, 0), (20000, 129, 132, 0)])
def test_colsum_deterministic_option(dev, option, M, N, ld, x_off):
    """"deterministic" 1: one row chunk, one writer per sum -- two runs are bit-identical, and so are out and out2, also when
    they accumulate from the same non-zero values; all under the bound of the longer chain (M / 8 rows per lane).  The option
    goes back to what it was."""
    option("deterministic", 1)
    k = R.colsum_k(M, deterministic=True)
    runs = [_colsum(dev, M, N, ld, x_off, acc, True, 9, same_start=True) for acc in (0, 0, 1, 1)]
    for (got, refs) in runs:
        for j in range(2):
            within(got[j], refs[j][0], k * U * refs[j][1], "deterministic colsum2")
        assert np.array_equal(bits(got[0]), bits(got[1]))
    for a, b in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert np.array_equal(bits(a[0][0]), bits(b[0][0])) and np.array_equal(bits(a[0][1]), bits(b[0][1]))
    assert not np.array_equal(bits(runs[0][0][0]), bits(runs[2][0][0]))  # the accumulating runs did start from non-zero values
