"""CPU: the float64 reference of the weight-update kernels (tests/update_reference.py) against torch in float64 --
clip_grad_norm_ + torch.optim.SGD(momentum, weight_decay), torch.optim.Adam(weight_decay), index_add_ -- to 1e-12 of each
element's magnitude, and every magnitude >= |output|.  The GPU tests (tests/test_gpu_update_kernels.py) hold the kernels to
this reference; this file holds the reference to torch without a GPU."""
import numpy as np
import pytest
import torch

import update_reference as R

TOL = 1e-12  # float64 restatements of the same arithmetic agree to a few 2^-53; a wrong formula is off by far more


def _close(got, want, mag):
    got, want, mag = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(mag, np.float64)
    assert got.shape == want.shape
    assert np.all(np.abs(got - want) <= TOL * mag + 1e-300), float(np.max(np.abs(got - want) / (mag + 1e-300)))


def _dominates(mag, out):
    assert np.all(np.asarray(mag) >= np.abs(np.asarray(out)) * (1 - 1e-15))


SIZES = (1, 5, 64, 1000)


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("gs", [1.0, 1.0 / 3.0])
def test_clip_sgd_is_clip_grad_norm_plus_torch_sgd(clipped, wd, gs):
    """Three steps over four tensors, then a re-started optimiser (``first`` again over the old buffers, which must not be
    read).  grad_scale: torch sees the already scaled gradients gs * g."""
    rng = np.random.default_rng(11)
    lr, mom = 0.1, 0.9
    gs32, lr32, mom32, wd32 = R.f32(gs), R.f32(lr), R.f32(mom), R.f32(wd)
    ps = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    tp = [torch.nn.Parameter(torch.from_numpy(p.astype(np.float64))) for p in ps]
    p_np = [p.astype(np.float64) for p in ps]
    bufs = [np.full(n, np.nan) for n in SIZES]  # garbage: not read at a first step
    opt = None
    for step in range(5):
        first = step in (0, 3)
        if first:
            opt = torch.optim.SGD(tp, lr=lr32, momentum=mom32, weight_decay=wd32)
            bufs = [np.full(n, np.nan) for n in SIZES]
        gr = [(rng.standard_normal(n) * 3).astype(np.float32) for n in SIZES]
        norm = np.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in gr)) * gs32
        clip = norm * (0.05 if clipped else 20.0)
        clip32 = R.f32(clip)
        out = R.clip_sgd(p_np, gr, bufs, clip, lr, mom, first, gs, wd)
        assert out["clipped"] == clipped
        if not clipped:
            assert out["c"] == gs32  # exactly grad_scale
        sq, sq_mag = R.sqnorm(gr)
        assert out["sq"] == sq and sq_mag == sq
        for t, g in zip(tp, gr):
            t.grad = torch.from_numpy(g.astype(np.float64)) * gs32
        total = torch.nn.utils.clip_grad_norm_(tp, clip32)  # coefficient clamp(clip / (total + 1e-6), max=1)
        assert abs(float(total) - norm) <= TOL * norm
        opt.step()
        for i, t in enumerate(tp):
            # torch's 1e-6 is a double, the kernel's 1e-6f a float: |1e-6 - 1e-6f| / norm < 1e-13 for these norms (> 10)
            _close(out["p"][i], t.detach().numpy(), out["p_mag"][i])
            _close(out["buf"][i], opt.state[t]["momentum_buffer"].numpy(), out["buf_mag"][i])
            _dominates(out["p_mag"][i], out["p"][i])
            _dominates(out["buf_mag"][i], out["buf"][i])
            assert np.all(out["p_err"][i] >= 0) and np.all(out["buf_err"][i] >= 0)
            k = R.K_C if clipped else R.K_UNCLIPPED
            assert np.all(out["p_err"][i] <= k * R.U * out["p_mag"][i] * (1 + 1e-12))
            assert np.all(out["buf_err"][i] <= k * R.U * out["buf_mag"][i] * (1 + 1e-12))
        p_np, bufs = out["p"], out["buf"]


def test_clip_sgd_empty_tensor_and_hyperparameters_rounded_to_float32():
    out = R.clip_sgd([np.zeros(0, np.float32), np.ones(3, np.float32)], [np.zeros(0, np.float32), np.ones(3, np.float32)],
                     [np.zeros(0, np.float32), np.zeros(3, np.float32)], 100.0, 0.1, 0.9, False, 1.0 / 3.0, 0.0)
    assert out["p"][0].shape == (0,) and out["sq"] == 3.0 and not out["clipped"]
    third = float(np.float32(1.0 / 3.0))
    assert out["c"] == third and third != 1.0 / 3.0
    assert np.array_equal(out["buf"][1], np.full(3, third))
    assert np.array_equal(out["p"][1], 1.0 - float(np.float32(0.1)) * np.full(3, third))


def _torch_adam(p, m, v, steps_done, lr, b1, b2, eps, wd):
    t = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([t], lr=R.f32(lr), betas=(R.f32(b1), R.f32(b2)), eps=R.f32(eps), weight_decay=R.f32(wd))
    if steps_done:
        opt.state[t] = {"step": torch.tensor(float(steps_done)), "exp_avg": torch.from_numpy(m.astype(np.float64)),
                        "exp_avg_sq": torch.from_numpy(v.astype(np.float64))}
    return t, opt


def _check_adam(out, t, opt):
    st = opt.state[t]
    _close(out["p"], t.detach().numpy(), out["p_mag"])
    _close(out["m"], st["exp_avg"].numpy(), out["m_mag"])
    _close(out["v"], st["exp_avg_sq"].numpy(), out["v_mag"])
    for k in "pmv":
        _dominates(out[k + "_mag"], out[k])
        assert np.all(out[k + "_err"] >= 0) and np.all(np.isfinite(out[k + "_err"]))


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_adam_is_torch_adam_steps_1_to_5(wd):
    rng = np.random.default_rng(5)
    n, lr, b1, b2, eps = 257, 3e-3, 0.9, 0.999, 1e-8
    p = rng.standard_normal(n).astype(np.float32)
    t, opt = _torch_adam(p, None, None, 0, lr, b1, b2, eps, wd)
    p_np, m, v = p.astype(np.float64), np.zeros(n), np.zeros(n)
    for step in range(1, 6):
        g = rng.standard_normal(n).astype(np.float32)
        g[::10] = 0.0
        out = R.adam(p_np, g, m, v, step, lr, b1, b2, eps, wd)
        t.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        _check_adam(out, t, opt)
        if wd == 0.0 and step == 1:
            assert np.array_equal(out["p"][::10], p_np[::10]) and np.all(out["p_err"][::10] == R.U * np.abs(p_np[::10]))
        p_np, m, v = out["p"], out["m"], out["v"]


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_adam_is_torch_adam_at_step_10000(wd):
    rng = np.random.default_rng(6)
    n, lr, b1, b2, eps = 300, 3e-3, 0.9, 0.999, 1e-8
    p, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    m, v = (rng.standard_normal(n) * 0.1).astype(np.float32), (rng.random(n) * 0.5).astype(np.float32)
    t, opt = _torch_adam(p, m, v, 9999, lr, b1, b2, eps, wd)
    t.grad = torch.from_numpy(g.astype(np.float64))
    opt.step()
    _check_adam(R.adam(p, g, m, v, 10000, lr, b1, b2, eps, wd), t, opt)


@pytest.mark.parametrize("V,D", [(1, 1), (7, 5), (40, 12)])
def test_rows_gather_add_is_index_add(V, D):
    rng = np.random.default_rng(V)
    n_src = max(1, V // 2)
    dst, src = rng.standard_normal((V, D)).astype(np.float32), rng.standard_normal((n_src + 2, D)).astype(np.float32)
    slot = rng.integers(-1, n_src + 2, size=V)
    out, mag, touched = R.rows_gather_add(dst, slot, src, n_src)
    want = torch.from_numpy(dst.astype(np.float64))
    rows = torch.from_numpy(np.nonzero((slot >= 0) & (slot < n_src))[0])
    want.index_add_(0, rows, torch.from_numpy(src.astype(np.float64))[torch.from_numpy(slot)[rows]])
    _close(out, want.numpy(), mag)
    _dominates(mag, out)
    assert np.array_equal(out[~touched], dst[~touched].astype(np.float64))
    assert np.array_equal(touched, (slot >= 0) & (slot < n_src))


def test_init_multi_axpy_colsum_and_sqnorm():
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal(9).astype(np.float32), rng.standard_normal(9).astype(np.float32)
    for s1, s2 in ((a, b), (a, None), (None, b), (None, None)):
        out, mag = R.init_multi(9, s1, s2)
        want = (0 if s1 is None else torch.from_numpy(s1).double()) + (0 if s2 is None else torch.from_numpy(s2).double()) + torch.zeros(9).double()
        _close(out, want.numpy(), mag + 1e-30)
        _dominates(mag, out)
    assert R.init_multi(0)[0].shape == (0,)
    for coef in (1.0, -0.5, 0.0, 1.0 / 3.0):
        out, mag = R.axpy(a, b, coef)
        _close(out, torch.add(torch.from_numpy(b).double(), torch.from_numpy(a).double(), alpha=R.f32(coef)).numpy(), mag)
        _dominates(mag, out)
    x, o = rng.standard_normal((33, 9)).astype(np.float32), rng.standard_normal(9).astype(np.float32)
    out, mag = R.colsum(x)
    _close(out, torch.from_numpy(x).double().sum(0).numpy(), mag)
    _dominates(mag, out)
    out, mag = R.colsum(x, o)
    _close(out, (torch.from_numpy(o).double() + torch.from_numpy(x).double().sum(0)).numpy(), mag)
    _dominates(mag, out)
    sq, sq_mag = R.sqnorm([a, b, np.zeros(0, np.float32)])
    want = float(torch.from_numpy(a).double().pow(2).sum() + torch.from_numpy(b).double().pow(2).sum())
    assert abs(sq - want) <= TOL * want and sq_mag >= sq


def test_colsum_k_counts_rows_per_lane_combine_and_chunks():
    """(rows added per lane) + 8 + gy with gy = min(64, ceil(M / 256)), 1 in deterministic mode."""
    assert R.colsum_k(1) == 1 + 8 + 1
    assert R.colsum_k(300) == 19 + 8 + 2          # two chunks of 150 rows, eight lanes each
    assert R.colsum_k(20000) == 40 + 8 + 64       # 64 chunks of 313 rows
    assert R.colsum_k(20000, deterministic=True) == 2500 + 8 + 1
