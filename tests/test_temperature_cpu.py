"""CPU: temperature scaling below the GPU -- the header, the export and the binding of blm_row_stats_temps, its refusals (all
made before any launch, so they are observable without a GPU), engine.TemperatureSearch against a float64 objective in numpy,
the report's JSON and the command line's flags."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "bayeslm.h")


@pytest.fixture(scope="module")
def L():
    from bayeslms_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_the_entry_the_struct_and_the_limit():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+BLM_ROW_TEMPS_MAX\s+8\b", src)
    assert re.search(r"typedef struct blm_row_temps \{\s*uint32_t abi_version;\s*int32_t count;\s*float beta\[BLM_ROW_TEMPS_MAX\];\s*\} "
                     r"blm_row_temps;", src)
    m = re.search(r"\bint blm_row_stats_temps\(([^)]*)\)", src)
    assert m and len(m.group(1).split(",")) == 13 and "const blm_row_temps* temps" in m.group(1)
    assert re.search(r"#define\s+BLM_ABI_VERSION\s+1u\b", src)


def test_library_exports_and_binding_binds_it(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    assert any(line.split()[-1] == "blm_row_stats_temps" and " T " in line for line in out.splitlines())
    res, args = L.SIGNATURES["blm_row_stats_temps"]
    assert res is C.c_int and len(args) == 13 and args[5] is C.POINTER(L.RowTemps)
    assert "blm_row_stats_temps" not in L.VALUE_RETURNING
    assert L.ABI_VERSION == 1 and L.lib().blm_abi_version() == 1 and L.ROW_TEMPS_MAX == 8
    assert C.sizeof(L.RowTemps) == 8 + 4 * 8 and L.RowTemps.beta.offset == 8


def _temps(L, betas, abi=None):
    t = L.RowTemps()
    t.abi_version, t.count = (L.ABI_VERSION if abi is None else abi), len(betas)
    for j, b in enumerate(betas[:8]):
        t.beta[j] = b
    return t


def test_refusals_come_before_any_launch(L):
    lib = L.lib()
    x = (C.c_float * 64)()  # never read: every call below is refused, or has no rows
    tg = (C.c_int64 * 8)()
    out = (C.c_float * 64)()
    xp, tp, op = C.addressof(x), C.addressof(tg), C.addressof(out)
    good = _temps(L, [0.5, 1.0, 2.0])

    def call(x=xp, ldx=8, tgt=tp, R=4, V=8, temps=good, nll=op, conf=op, entropy=op, dnll=op, pred=None, rank=None):
        return lib.blm_row_stats_temps(x, ldx, tgt, R, V, None if temps is None else C.byref(temps), nll, conf, entropy, dnll, pred,
                                       rank, None)

    def count(n):
        t = _temps(L, [1.0] * 8)
        t.count = n
        return t

    cases = [("null x", dict(x=None), L.ERR_INVALID, b"null"),
             ("null temps", dict(temps=None), L.ERR_INVALID, b"null"),
             ("abi", dict(temps=_temps(L, [1.0], abi=L.ABI_VERSION + 1)), L.ERR_ABI, b"abi_version"),
             ("count 0", dict(temps=count(0)), L.ERR_INVALID, b"count 0"),
             ("count 9", dict(temps=count(9)), L.ERR_INVALID, b"count 9"),
             ("count -1", dict(temps=count(-1)), L.ERR_INVALID, b"count -1"),
             ("beta 0", dict(temps=_temps(L, [1.0, 0.0])), L.ERR_INVALID, b"beta[1]"),
             ("beta < 0", dict(temps=_temps(L, [-1.0])), L.ERR_INVALID, b"beta[0]"),
             ("beta inf", dict(temps=_temps(L, [1.0, 2.0, float("inf")])), L.ERR_INVALID, b"beta[2]"),
             ("beta nan", dict(temps=_temps(L, [float("nan")])), L.ERR_INVALID, b"beta[0]"),
             ("R < 0", dict(R=-1), L.ERR_INVALID, b"shape"),
             ("V = 0", dict(V=0), L.ERR_INVALID, b"shape"),
             ("ldx < V", dict(ldx=7), L.ERR_INVALID, b"shape"),
             ("nll without tgt", dict(tgt=None, dnll=None), L.ERR_INVALID, b"need targets"),
             ("dnll without tgt", dict(tgt=None, nll=None), L.ERR_INVALID, b"need targets"),
             ("rank without tgt", dict(tgt=None, nll=None, dnll=None, rank=op), L.ERR_INVALID, b"need targets"),
             ("extents", dict(R=2 ** 31 - 1, ldx=2 ** 40), L.ERR_INVALID, b"extents")]
    for name, kw, status, msg in cases:
        rc = call(**kw)
        assert rc == status, (name, rc)
        text = lib.blm_last_error()
        assert text.startswith(b"blm_row_stats_temps: ") and msg in text, (name, text)
    assert call(R=0) == L.OK
    assert call(R=0, tgt=None, nll=None, dnll=None) == L.OK
    with pytest.raises(L.BayesLMError, match=r"blm_row_stats_temps failed \(status -1\): blm_row_stats_temps: count 9"):
        L.calls().blm_row_stats_temps(xp, 8, tp, 4, 8, C.byref(count(9)), op, op, op, op, None, None, None)


def test_op_refuses_bad_temperature_lists_without_a_device():
    from bayeslms_amd import BayesLMError, ops
    for bad, msg in (([], "0 inverse"), ([1.0] * 9, "9 inverse"), ([1.0, 0.0], r"betas\[1\] = 0.0"), ([-2.0], r"betas\[0\] = -2.0"),
                     ([float("nan")], r"betas\[0\] = nan"), ([1.0, float("inf")], r"betas\[1\] = inf"), ([1e-60], r"betas\[0\] = 1e-60"),
                     ([1e60], r"betas\[0\] = 1e\+60"), (2.0, "2.0"), (["x"], "x")):
        with pytest.raises(BayesLMError, match=msg):
            ops.row_stats_temps(None, bad)
    t = ops.row_temps([0.5, 1, 2])
    assert (t.abi_version, t.count, list(t.beta)) == (1, 3, [0.5, 1.0, 2.0, 0, 0, 0, 0, 0])


# ------------------------------------------------------------------------------------------------------------ the search
class _Objective:
    """Mean NLL and its slope in beta, float64: 2000 rows x 50 columns of logits ``scale`` * base with targets drawn from
    softmax(base) -- the minimiser sits near 1 / scale."""

    def __init__(self, scale, seed=0):
        rng = np.random.default_rng(seed)
        base = 2.0 * rng.standard_normal((2000, 50))
        p = np.exp(base - base.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        self.t = (p.cumsum(1) < rng.random((2000, 1))).sum(1).clip(0, 49)
        self.x = scale * base
        self.calls = 0

    def __call__(self, beta):
        self.calls += 1
        z = beta * self.x
        z = z - z.max(1, keepdims=True)
        e = np.exp(z)
        s = e.sum(1)
        xt = self.x[np.arange(len(self.t)), self.t]
        loss = (np.log(s) - z[np.arange(len(self.t)), self.t]).mean()
        return float(loss), float(((e * self.x).sum(1) / s - xt).mean())

    def minimiser(self):
        lo, hi = 1e-4, 1e4
        assert self(lo)[1] < 0 < self(hi)[1]
        for _ in range(200):
            mid = math.sqrt(lo * hi)
            lo, hi = (mid, hi) if self(mid)[1] < 0 else (lo, mid)
        return math.sqrt(lo * hi)


def _run(search, f, passes):
    brackets = []
    for _ in range(passes):
        g = search.grid()
        assert 1 <= len(g) <= search.points and g == sorted(g) and all(b == float(np.float32(b)) for b in g)
        vals = [f(b) for b in g]
        search.update(g, [v[0] for v in vals], [v[1] for v in vals])
        brackets.append(search.bracket)
        if search.done:
            break
    return brackets


@pytest.mark.parametrize("scale", [2.5, 1.0, 0.6])
def test_search_finds_the_float64_minimiser_in_three_passes(scale):
    """1e-3: three passes of eight points leave a bracket of ratio 64^(1/343) = 1.0122, so an end or the midpoint would be off
    by up to 6e-3; the secant through the two slopes is what gets below 1e-3."""
    from bayeslms_amd import engine
    f = _Objective(scale)
    star = f.minimiser()
    s = engine.TemperatureSearch()
    assert (s.lo, s.hi, s.points) == (1.0 / 16, 16.0, 8) and s.bracket == (1.0 / 16, 16.0)
    first = s.grid()
    assert len(first) == 8 and first[0] == 0.125 and first[-1] == 8.0
    assert np.allclose(np.diff(np.log(first)), math.log(64) / 7, rtol=1e-6)  # geometric
    br = _run(s, f, 3)
    got = s.result()
    print("scale %g: beta* %.9f, fitted %.9f, relative %.3e, brackets %s" % (scale, star, got, got / star - 1, br))
    assert abs(got / star - 1) <= 1e-3 and not s.at_bound and len(br) == 3
    prev = (s.lo, s.hi)
    for a, b in br:
        assert a <= star <= b and prev[0] <= a and b <= prev[1]
        prev = (a, b)
    assert br[-1][1] / br[-1][0] <= 64 ** (1 / 343) * (1 + 1e-6)
    assert br[-1][0] <= got <= br[-1][1]


def test_search_ends_at_a_bound_the_minimiser_lies_beyond():
    from bayeslms_amd import engine
    for scale, kw, want in ((40.0, {}, 1.0 / 16), (1.0 / 40, {}, 16.0), (2.5, dict(lo=0.5, hi=2.0), 0.5), (0.6, dict(lo=0.25, hi=1.5), 1.5)):
        f = _Objective(scale)
        s = engine.TemperatureSearch(**kw)
        br = _run(s, f, 3)
        print("scale %g: beta* %.6f ends at %.6f after %d passes" % (scale, f.minimiser(), s.result(), len(br)))
        assert s.at_bound and s.done and s.result() == want and len(br) <= 2
        assert all(s.lo <= b <= s.hi for b in s.seen)
    f = _Objective(1.0)  # an interior minimiser is no bound
    s = engine.TemperatureSearch(lo=0.5, hi=2.0)
    _run(s, f, 3)
    assert not s.at_bound and abs(s.result() / f.minimiser() - 1) <= 1e-3


def test_search_refuses_a_non_finite_loss_naming_beta():
    from bayeslms_amd import BayesLMError, engine
    s = engine.TemperatureSearch()
    g = s.grid()
    loss, dl = [3.0] * 8, list(np.linspace(-1, 1, 8))
    loss[3] = float("nan")
    with pytest.raises(BayesLMError, match=re.escape("beta = %r" % g[3])):
        s.update(g, loss, dl)
    loss[3], dl[5] = 3.0, float("inf")
    with pytest.raises(BayesLMError, match=re.escape("beta = %r" % g[5])):
        s.update(g, loss, dl)
    with pytest.raises(BayesLMError, match="lo"):
        engine.TemperatureSearch(lo=2.0, hi=1.0)
    with pytest.raises(BayesLMError, match="points"):
        engine.TemperatureSearch(points=9)
    with pytest.raises(BayesLMError, match="nothing evaluated"):
        engine.TemperatureSearch().result()


# ------------------------------------------------------------------------------------------------------------ report and flags
def test_report_json_has_no_temperature_key_without_a_temperature():
    from bayeslms_amd import engine
    rep = engine.report_from_tokens([1.0, 2.0], [0.5, 0.25], [1.0, 1.5], [0, 3], bins=4)
    assert rep.temperature is None and "temperature" not in rep.as_dict()
    assert list(rep.as_dict())[-1] == "mean_mi" and [f.name for f in engine.dataclasses.fields(rep)][-1] == "temperature"
    rep.temperature = engine.temperature_block(0.5)
    d = rep.as_dict()["temperature"]
    assert sorted(d) == ["at_bound", "beta", "curve", "ece_after", "ece_before", "fitted_on", "loss_after", "loss_before", "temperature"]
    assert (d["temperature"], d["beta"], d["fitted_on"], d["at_bound"]) == (2.0, 0.5, None, False)


NEEDED = ["--model-path", "/nonexistent/model.pt", "--vocabulary", "/nonexistent/words.txt", "--data", "/nonexistent/test.txt"]


def test_parser_defaults_and_refusals_before_any_file_is_opened():
    from bayeslms_amd import evaluate as E
    args = E.build_parser().parse_args(NEEDED)
    assert args.temperature is None and args.fit_temperature_on == "" and args.fit_passes == 3
    E.check_args(args)
    for extra, flag in ((["--temperature", "0"], "--temperature"), (["--temperature", "-2"], "--temperature"),
                        (["--temperature", "nan"], "--temperature"), (["--temperature", "inf"], "--temperature"),
                        (["--temperature", "2", "--fit-temperature-on", "/nonexistent/valid.txt"], "--fit-temperature-on"),
                        (["--fit-temperature-on", "/nonexistent/valid.txt", "--fit-passes", "0"], "--fit-passes"),
                        (["--fit-passes", "7"], "--fit-passes")):
        with pytest.raises(SystemExit) as e:
            E.main(NEEDED + extra)  # the files do not exist: a refusal that came later would be another error
        assert flag in str(e.value), (extra, e.value)
    E.check_args(E.build_parser().parse_args(NEEDED + ["--temperature", "1.5"]))
    E.check_args(E.build_parser().parse_args(NEEDED + ["--fit-temperature-on", "v.txt", "--fit-passes", "6"]))


def test_summary_line_gains_the_temperature_only_with_one():
    from bayeslms_amd import engine, evaluate as E
    rep = engine.report_from_tokens([1.0, 2.0], [0.5, 0.25], [1.0, 1.5], [0, 3], bins=4)
    plain = E.summary_line(rep)
    assert "temperature" not in plain
    rep.temperature = engine.temperature_block(0.5)
    assert E.summary_line(rep) == plain + " | temperature 2.0000"
    rep.temperature = engine.temperature_block(0.5, "valid.txt", False, rep, rep, [])
    assert E.summary_line(rep) == plain + " | temperature 2.0000 | fit loss 1.5000 -> 1.5000 | ece %.4f -> %.4f" % (rep.ece, rep.ece)
