"""CPU: blm_ce_soft_temp_fwd_bwd and blm_ce_soft_topk_temp_fwd_bwd are declared, exported, bound and refuse bad arguments on the
host, before any launch -- everything their untempered siblings refuse, and a bad beta or soft_scale, each by the value; the
``temperature`` / ``soft_scale`` keywords of the ops refuse what is no temperature; --distill-temperature of bayeslms_amd.train
defaults to 1 and every refusal exits with its message before a device is looked for."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")
HOST_LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip_asan.so")
DENSE, TOPK = "blm_ce_soft_temp_fwd_bwd", "blm_ce_soft_topk_temp_fwd_bwd"
PARAMS = {
    DENSE: ["const float* logits", "int64_t ld", "const float* logq", "int64_t ldq", "const int64_t* tgt", "float lambda", "float beta",
            "float soft_scale", "float* loss", "float* nll", "float* soft", "float* kl", "float* lse", "float* loss_sum",
            "float* dlogits", "float grad_scale", "int M", "int V", "void* stream"],
    TOPK: ["const float* logits", "int64_t ld", "const int32_t* ids", "const float* logq", "int64_t ldk", "int K", "const int64_t* tgt",
           "float lambda", "float beta", "float soft_scale", "float* loss", "float* nll", "float* soft", "float* kl", "float* lse",
           "float* loss_sum", "float* dlogits", "float grad_scale", "int M", "int V", "void* stream"],
}
CTYPES = {"const float*": C.c_void_p, "float*": C.c_void_p, "const int64_t*": C.c_void_p, "const int32_t*": C.c_void_p,
          "void*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from bayeslms_amd import _lib as L
    return L, L.lib()


@pytest.mark.parametrize("name", [DENSE, TOPK])
def test_header_declares_library_exports_binding_has_it(lib, name):
    text = open(os.path.join(ROOT, "include", "bayeslm.h")).read()
    assert re.search(r"^#define BLM_ABI_VERSION 1u\b", text, flags=re.M)  # additive symbols: the ABI version stays
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert proto, "not declared"
    params = [" ".join(p.split()) for p in proto.group(1).split(",")]
    assert params == PARAMS[name]
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    assert name in {line.split()[-1] for line in out.splitlines() if " T " in line}
    L, l = lib
    res, args = L.SIGNATURES[name]
    assert res is C.c_int and list(args) == [CTYPES[p.rsplit(" ", 1)[0]] for p in params]  # the declared count, the declared types
    assert name not in L.VALUE_RETURNING and getattr(L.calls(), name).errcheck is not None  # in the checked view
    assert L.ABI_VERSION == 1 and l.blm_abi_version() == 1
    old = name.replace("_temp", "")  # the untempered sibling is declared as it was: beta and soft_scale are the only difference
    assert [p for p in params if p not in ("float beta", "float soft_scale")] == \
        [" ".join(p.split()) for p in re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % old, src).group(1).split(",")]


def test_header_states_the_definitions():
    text = " ".join(open(os.path.join(ROOT, "include", "bayeslm.h")).read().replace("*", " ").split())
    for words in ("beta = 1/T > 0", "c = soft_scale >= 0", "has_q = any live", "ml = max over live l_v",
                  "This is the teacher (or model average) raised to beta and renormalised over its live entries: pbar^beta / Z",
                  "Both p and p~ are formed from the max-shifted logits, never as exp(beta z - lse_beta)",
                  "This is the cross entropy of p~ under q~, unscaled", "It is summed term by term and is >= 0 up to rounding",
                  "loss[m] = (1 - lambda) nll + lambda c soft",
                  "The tempered target is always normalised (sum q~ = 1)", "differ by the factor Q otherwise",
                  "A constant added to a row's logq cancels in q~", "serves every temperature"):
        assert words in text, words


# ------------------------------------------------------------------------------------------- refusals, on the host-only build
# addresses that are never dereferenced: logits, ids, logq, targets, per-row outputs, a separate gradient buffer far from all of them
Z, I, Q, T, O, D = 0x100000, 0x700000, 0x900000, 0x10000, 0x20000, 0x1100000
M, V, K = 4, 10, 3
NAN, INF = float("nan"), float("inf")


def dense(l, logits=Z, ld=V, logq=Q, ldq=V, tgt=T, lam=0.5, beta=0.5, c=4.0, loss=O, dlogits=D, m=M, v=V):
    return getattr(l, DENSE)(logits, ld, logq, ldq, tgt, lam, beta, c, loss, O + 64, O + 128, O + 192, None, None, dlogits, 0.25, m, v, None)


def topk(l, logits=Z, ld=V, ids=I, logq=Q, ldk=K, k=K, tgt=T, lam=0.5, beta=0.5, c=4.0, loss=O, dlogits=D, m=M, v=V):
    return getattr(l, TOPK)(logits, ld, ids, logq, ldk, k, tgt, lam, beta, c, loss, O + 64, O + 128, O + 192, None, None, dlogits, 0.25,
                            m, v, None)


TEMPER = [
    (dict(beta=0.0), b"beta = 0"), (dict(beta=-2.0), b"beta = -2"), (dict(beta=NAN), b"beta = nan"), (dict(beta=INF), b"beta = inf"),
    (dict(beta=-INF), b"beta = -inf"), (dict(c=-0.5), b"soft_scale = -0.5"), (dict(c=NAN), b"soft_scale = nan"),
    (dict(c=INF), b"soft_scale = inf"), (dict(c=-INF), b"soft_scale = -inf"),
]
DENSE_BAD = [  # tests/test_distill_cpu.py's list for blm_ce_soft_fwd_bwd
    (dict(logits=None), b"required"), (dict(logq=None), b"required"), (dict(tgt=None), b"required"), (dict(loss=None), b"required"),
    (dict(ld=V - 1), b"ld = 9"), (dict(ldq=V - 1), b"ldq = 9"), (dict(ld=2 ** 40), b"ld = "),
    (dict(m=-1), b"M = -1"), (dict(v=0), b"V = 0"), (dict(v=-3, ld=0, ldq=0), b"V = -3"),
    (dict(lam=-0.01), b"lambda = -0.01"), (dict(lam=1.5), b"lambda = 1.5"), (dict(lam=NAN), b"lambda = nan"),
    (dict(dlogits=Q), b"overlaps logq"), (dict(dlogits=Q + 4 * (M * V - 1)), b"overlaps logq"),
    (dict(dlogits=Q - 4 * (M * V - 1)), b"overlaps logq"),
    (dict(dlogits=Z + 4), b"in place"), (dict(dlogits=Z - 4 * (M * V - 1)), b"in place"), (dict(dlogits=Z + 4 * V), b"in place"),
]
TOPK_BAD = [  # tests/test_distill_topk_cpu.py's list for blm_ce_soft_topk_fwd_bwd
    (dict(logits=None), b"logits is NULL"), (dict(ids=None), b"ids is NULL"), (dict(logq=None), b"logq is NULL"),
    (dict(tgt=None), b"tgt is NULL"), (dict(loss=None), b"loss is NULL"),
    (dict(m=-1), b"M = -1"), (dict(v=0), b"V = 0"), (dict(v=-3, ld=0), b"V = -3"),
    (dict(k=0), b"K = 0"), (dict(k=-2), b"K = -2"), (dict(k=257, ldk=257), b"K = 257"), (dict(k=2 ** 31 - 1, ldk=2 ** 31), b"K = 2147483647"),
    (dict(ld=V - 1), b"ld = 9"), (dict(ldk=K - 1), b"ldk = 2"), (dict(ld=2 ** 40), b"ld = "), (dict(ldk=2 ** 40), b"ldk = "),
    (dict(ld=-5), b"ld = -5"), (dict(ldk=-5), b"ldk = -5"), (dict(m=2 ** 31 - 1, ld=2 ** 30), b"ld = "),
    (dict(lam=-0.01), b"lambda = -0.01"), (dict(lam=1.5), b"lambda = 1.5"), (dict(lam=NAN), b"lambda = nan"),
    (dict(dlogits=I), b"overlaps ids"), (dict(dlogits=I + 4 * (M * K - 1)), b"overlaps ids"),
    (dict(dlogits=I - 4 * (M * V - 1)), b"overlaps ids"),
    (dict(dlogits=Q), b"overlaps logq"), (dict(dlogits=Q + 4 * (M * K - 1)), b"overlaps logq"),
    (dict(dlogits=Q - 4 * (M * V - 1)), b"overlaps logq"),
    (dict(dlogits=Z + 4), b"in place"), (dict(dlogits=Z - 4 * (M * V - 1)), b"in place"), (dict(dlogits=Z + 4 * V), b"in place"),
]
REFUSALS = [(DENSE, kw, msg) for kw, msg in DENSE_BAD + TEMPER] + [(TOPK, kw, msg) for kw, msg in TOPK_BAD + TEMPER]

# The host-only build (csrc/Makefile, `asan`: AddressSanitizer + UndefinedBehaviorSanitizer on the launchers and argument checks, no
# device code, so a check that let a call through would show as a launch error, not a refusal).  A stand-alone C program,
# compiled with the same sanitizers and linked against that build, makes every call of the list and prints what it was told.
class Recorder:
    """Stands in for the library: keeps the arguments of the one call made through it"""
    def __init__(self, name):
        self.name, self.args = name, None

    def __getattr__(self, name):
        assert name == self.name
        return lambda *a: setattr(self, "args", list(a)) or 0


def c_call(name, kw):
    rec = Recorder(name)
    (dense if name == DENSE else topk)(rec, **kw)
    words = []
    for decl, a in zip(PARAMS[name], rec.args):
        ctype = decl.rsplit(" ", 1)[0]
        if ctype.endswith("*"):
            words.append("(%s)%s" % (ctype, "0" if a is None else hex(a)))
        elif ctype == "float":
            words.append("NAN" if a != a else ("-" if a < 0 else "") + "INFINITY" if math.isinf(a) else "%rf" % float(a))
        else:
            words.append("(%s)%dLL" % (ctype, a))
    return "  said(%s(%s));\n" % (name, ", ".join(words))


def test_refusals_on_the_host_only_build(lib, tmp_path):
    L, _ = lib
    clang = os.path.join(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "..", "lib", "llvm", "bin", "clang")
    if not os.path.exists(clang):
        pytest.skip("no clang beside hipcc in this image")
    if not os.path.exists(HOST_LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "bayeslms_amd", "csrc"), "-j", "8", "asan"])
    src, exe = str(tmp_path / "refusals.c"), str(tmp_path / "refusals")
    with open(src, "w") as f:
        f.write('#include <math.h>\n#include <stdio.h>\n#include "bayeslm.h"\n'
                'static void said(int status) { printf("%d|%s\\n", status, blm_last_error()); }\n'
                "int main(void) {\n" + "".join(c_call(name, kw) for name, kw, _ in REFUSALS) + "  return 0;\n}\n")
    runtime = os.path.dirname(subprocess.check_output([clang, "-print-file-name=libclang_rt.asan-x86_64.so"], text=True).strip())
    libdir = os.path.dirname(HOST_LIB)
    subprocess.check_call([clang, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-shared-libsan", "-g",
                           "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-L" + libdir, "-l:" + os.path.basename(HOST_LIB),
                           "-Wl,-rpath,%s,-rpath,%s,-rpath-link,/opt/rocm/lib" % (libdir, runtime)])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    answers = [ln.split("|", 1) for ln in r.stdout.splitlines()]
    assert len(answers) == len(REFUSALS)
    for (name, kw, msg), (status, err) in zip(REFUSALS, answers):
        assert int(status) == L.ERR_INVALID, (name, kw, status, err)
        assert name in err and msg.decode() in err, (name, kw, err)


@pytest.mark.parametrize("name,kw,msg", REFUSALS)
def test_refuses_bad_arguments_before_any_launch(lib, name, kw, msg):
    L, l = lib
    assert (dense if name == DENSE else topk)(l, **kw) == L.ERR_INVALID
    err = l.blm_last_error()
    assert name.encode() in err and msg in err, err
    if name == TOPK:
        assert DENSE.encode() not in err  # each entry point answers under its own name


def test_no_rows_is_a_no_op_and_the_checked_view_raises(lib):
    L, l = lib
    for call in (dense, topk):
        assert call(l, m=0) == L.OK                    # nothing to do, nothing launched
        assert call(l, m=0, dlogits=Z) == L.OK
        assert call(l, m=0, lam=2.0) == L.ERR_INVALID   # the arguments are still checked
        assert call(l, m=0, beta=0.0) == L.ERR_INVALID
        assert call(l, m=0, c=-1.0) == L.ERR_INVALID
        assert call(l, m=0, c=0.0) == L.OK              # a soft term switched off is no error
    with pytest.raises(L.BayesLMError, match=DENSE):
        getattr(L.calls(), DENSE)(Z, V, Q, V, T, 0.5, -1.0, 1.0, O, None, None, None, None, None, None, 1.0, M, V, None)
    with pytest.raises(L.BayesLMError, match=TOPK):
        getattr(L.calls(), TOPK)(Z, V, I, Q, K, K, T, 0.5, 1.0, NAN, O, None, None, None, None, None, None, 1.0, M, V, None)


# ------------------------------------------------------------------------------------------------------------------ ops
BAD_T = [0, 0.0, -1.0, -0.0, NAN, INF, -INF, True, False, "2", None, 1e-39, 1e-300, 1e46, 1e300]
#        ... and temperatures whose 1 / T is no positive finite float32: it overflows (1e-39, 1e-300) or is zero (1e46, 1e300)


@pytest.mark.parametrize("bad", BAD_T, ids=[repr(b) for b in BAD_T])
def test_ops_refuse_what_is_no_temperature(bad):
    """Refused by the value alone, before a tensor or a device is looked at."""
    from bayeslms_amd import ops
    z, t, l = torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 5)
    sp = ops.SparseTargets(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3))
    with pytest.raises(ops.BayesLMError, match="cross_entropy_soft: temperature"):
        ops.cross_entropy_soft(z, t, l, 0.5, temperature=bad)
    with pytest.raises(ops.BayesLMError, match="cross_entropy_soft_topk: temperature"):
        ops.cross_entropy_soft_topk(z, t, sp, 0.5, temperature=bad)


@pytest.mark.parametrize("bad", [-1.0, NAN, INF, True, "1"], ids=repr)
def test_ops_refuse_what_is_no_soft_scale(bad):
    from bayeslms_amd import ops
    z, t, l = torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 5)
    sp = ops.SparseTargets(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3))
    with pytest.raises(ops.BayesLMError, match="cross_entropy_soft: soft_scale"):
        ops.cross_entropy_soft(z, t, l, 0.5, temperature=2.0, soft_scale=bad)
    with pytest.raises(ops.BayesLMError, match="cross_entropy_soft_topk: soft_scale"):
        ops.cross_entropy_soft_topk(z, t, sp, 0.5, temperature=2.0, soft_scale=bad)


def test_ops_pick_the_entry_point_by_the_temperature():
    """T = 1 with the factor left alone or 1 is the untempered call; anything else carries beta = float32(1 / T) and c = T^2."""
    from bayeslms_amd import ops
    assert ops._temper("x", 1.0, None) is None and ops._temper("x", 1, 1.0) is None and ops._temper("x", 1.0, 1) is None
    assert ops._temper("x", 2.0, None) == (0.5, 4.0) and ops._temper("x", 4, None) == (0.25, 16.0)
    assert ops._temper("x", 1.0, 2.0) == (1.0, 2.0) and ops._temper("x", 1.0, 0.0) == (1.0, 0.0)
    beta, c = ops._temper("x", 3.0, 1.0)
    assert c == 1.0 and beta == float(torch.tensor(1.0 / 3.0, dtype=torch.float32)) and beta != 1.0 / 3.0  # a float32 value
    with pytest.raises(ops.BayesLMError, match="soft_scale"):
        ops._temper("x", 1e30, None)  # T^2 is no float32


# ----------------------------------------------------------------------------------------------------------- command line
def test_parser_default_is_one_and_the_check_returns_what_it_returned():
    from bayeslms_amd import train
    a = train.build_parser().parse_args([])
    assert a.distill_temperature == 1.0
    assert train.check_distill_args(a, 1) is None
    argv = ["--distill-from", "t.pt", "--emsize", "32", "--tied", "--distill-top-k", "8"]
    b, c = train.build_parser().parse_args(argv), train.build_parser().parse_args(argv + ["--distill-temperature", "1"])
    assert b.distill_temperature == 1.0
    shape, same = train.check_distill_args(b, 1), train.check_distill_args(c, 1)  # T = 1 with unrenormalised top-k: today's run
    assert vars(shape) == vars(same) == {f: getattr(b, f) for f in train.TEACHER_FLAGS}
    d = train.build_parser().parse_args(argv + ["--distill-top-k-renorm", "1", "--distill-temperature", "2.5"])
    assert vars(train.check_distill_args(d, 1)) == vars(shape) and d.distill_temperature == 2.5
    e = train.build_parser().parse_args(argv[:5] + ["--distill-temperature", "0.0625"])  # dense, at the lower bound
    assert vars(train.check_distill_args(e, 1)) == vars(shape)
    assert (train.DISTILL_T_LO, train.DISTILL_T_HI) == (1.0 / 16, 16.0)
    from bayeslms_amd import engine
    s = engine.TemperatureSearch()
    assert (s.lo, s.hi) == (train.DISTILL_T_LO, train.DISTILL_T_HI)  # the bounds that search already uses


FROM = ("--distill-from", "missing_teacher.pt")
CLI_BAD = [
    (("--distill-temperature", "2"), "--distill-temperature needs --distill-from"),
    (("--distill-temperature", "nan"), "--distill-temperature needs --distill-from"),
    (FROM + ("--distill-temperature", "nan"), "--distill-temperature must be a finite number"),
    (FROM + ("--distill-temperature", "inf"), "--distill-temperature must be a finite number"),
    (FROM + ("--distill-temperature=-inf",), "--distill-temperature must be a finite number"),
    (FROM + ("--distill-temperature", "0"), "--distill-temperature must lie in [1/16, 16]"),
    (FROM + ("--distill-temperature=-2",), "--distill-temperature must lie in [1/16, 16]"),
    (FROM + ("--distill-temperature", "0.06"), "--distill-temperature must lie in [1/16, 16]"),
    (FROM + ("--distill-temperature", "16.5"), "--distill-temperature must lie in [1/16, 16]"),
    (FROM + ("--distill-temperature", "2", "--distill-top-k", "8"), "needs --distill-top-k-renorm 1"),
    (FROM + ("--distill-temperature", "0.5", "--distill-top-k", "8", "--distill-top-k-renorm", "0"), "needs --distill-top-k-renorm 1"),
]


@pytest.mark.parametrize("extra,msg", CLI_BAD)
def test_check_distill_args_refuses(extra, msg):
    from bayeslms_amd import train
    with pytest.raises(SystemExit) as e:
        train.check_distill_args(train.build_parser().parse_args(list(extra)), 1)
    assert msg in str(e.value), e.value


# a child in which asking for a device is an error: the refusal has to come first
NO_DEVICE = ("import sys, torch\n"
             "def no(*a, **k):\n"
             "    raise RuntimeError('a device was asked for')\n"
             "torch.device = torch.cuda.is_available = torch.cuda.device_count = torch.cuda.set_device = torch.cuda.init = no\n"
             "from bayeslms_amd import train\n"
             "train.main(sys.argv[1:])\n")


@pytest.mark.parametrize("extra,msg", CLI_BAD)
def test_cli_refuses(extra, msg):
    """Refused before the input paths are looked at (neither the corpus nor the teacher exists) and before any device is."""
    argv = [sys.executable, "-c", NO_DEVICE, "--data", "missing_corpus", "--cuda", "--save", "missing_model.pt"] + list(extra)
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    r = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode != 0
    assert msg in r.stderr and "a device was asked for" not in r.stderr, r.stderr
    assert math.isfinite(r.returncode)
