"""CPU: blm_ce_soft_fwd_bwd is declared, exported, bound and refuses bad arguments on the host, before any launch; the
--distill-* flags of bayeslms_amd.train default to off and every refusal exits with its message before a device is looked
for."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")
NAME = "blm_ce_soft_fwd_bwd"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from bayeslms_amd import _lib as L
    return L, L.lib()


def test_header_declares_library_exports_binding_has_it(lib):
    text = open(os.path.join(ROOT, "include", "bayeslm.h")).read()
    assert re.search(r"^#define BLM_ABI_VERSION 1u\b", text, flags=re.M)  # an additive symbol: the ABI version stays
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert NAME in set(re.findall(r"\b(blm_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    assert NAME in {line.split()[-1] for line in out.splitlines() if " T " in line}
    L, l = lib
    res, args = L.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 17 and args[1] is C.c_int64 and args[3] is C.c_int64 and args[5] is C.c_float
    assert args[13] is C.c_float and args[14] is C.c_int and args[15] is C.c_int
    assert NAME not in L.VALUE_RETURNING and L.calls().blm_ce_soft_fwd_bwd.errcheck is not None
    assert L.ABI_VERSION == 1 and l.blm_abi_version() == 1


# addresses that are never dereferenced: logits, logq, targets, per-row outputs, a separate gradient buffer far from both matrices
Z, Q, T, O, D = 0x100000, 0x900000, 0x10000, 0x20000, 0x1100000
M, V = 4, 10


def call(l, logits=Z, ld=V, logq=Q, ldq=V, tgt=T, lam=0.5, loss=O, nll=O + 64, soft=O + 128, kl=O + 192, lse=None, loss_sum=None,
         dlogits=D, m=M, v=V):
    return l.blm_ce_soft_fwd_bwd(logits, ld, logq, ldq, tgt, lam, loss, nll, soft, kl, lse, loss_sum, dlogits, 0.25, m, v, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(logits=None), b"required"), (dict(logq=None), b"required"), (dict(tgt=None), b"required"), (dict(loss=None), b"required"),
    (dict(ld=V - 1), b"ld"), (dict(ldq=V - 1), b"ldq"), (dict(ld=2 ** 40), b"ld"),
    (dict(m=-1), b"M = -1"), (dict(v=0), b"V = 0"), (dict(v=-3, ld=0, ldq=0), b"V = -3"),
    (dict(lam=-0.01), b"lambda"), (dict(lam=1.5), b"lambda"), (dict(lam=float("nan")), b"lambda"),
    (dict(dlogits=Q), b"overlaps logq"), (dict(dlogits=Q + 4 * (M * V - 1)), b"overlaps logq"),
    (dict(dlogits=Q - 4 * (M * V - 1)), b"overlaps logq"),
    (dict(dlogits=Z + 4), b"in place"), (dict(dlogits=Z - 4 * (M * V - 1)), b"in place"), (dict(dlogits=Z + 4 * V), b"in place"),
])
def test_refuses_bad_arguments_before_any_launch(lib, kw, msg):
    L, l = lib
    assert call(l, **kw) == L.ERR_INVALID
    err = l.blm_last_error()
    assert NAME.encode() in err and msg in err, err


def test_no_rows_is_a_no_op_and_the_checked_view_raises(lib):
    L, l = lib
    assert call(l, m=0) == L.OK                   # nothing to do, nothing launched
    assert call(l, m=0, dlogits=Z) == L.OK
    assert call(l, m=0, lam=2.0) == L.ERR_INVALID  # the arguments are still checked
    with pytest.raises(L.BayesLMError, match=NAME):
        L.calls().blm_ce_soft_fwd_bwd(None, V, Q, V, T, 0.5, O, None, None, None, None, None, None, 1.0, M, V, None)


# ----------------------------------------------------------------------------------------------- command line
def test_parser_defaults_are_off():
    from bayeslms_amd import train
    a = train.build_parser().parse_args([])
    assert a.distill_from == "" and a.distill_weight is None and a.distill_mc_samples == 0
    assert a.distill_mc_seed == 1111 and a.distill_teacher_args is None
    assert train.check_distill_args(a, 1) is None
    b = train.build_parser().parse_args(["--distill-from", "t.pt", "--emsize", "32", "--tied", "--distill-teacher-args",
                                         "--model Transformer --emsize 64 --uncertainty Bayesian --T_bayes_pos FFN --lr 7"])
    shape = train.check_distill_args(b, 1)
    assert b.distill_weight == 0.5  # the default, once distillation is on
    assert (shape.model, shape.emsize, shape.uncertainty, shape.T_bayes_pos, shape.tied) == ("Transformer", 64, "Bayesian", "FFN", False)
    assert not hasattr(shape, "lr")  # only the model-shaping flags are read
    c = train.build_parser().parse_args(["--distill-from", "t.pt", "--emsize", "32", "--tied"])
    own = train.check_distill_args(c, 1)
    assert (own.emsize, own.tied, own.model) == (32, True, "LSTM")  # default: the student's own flags


def _cli(*extra, env=None):
    argv = [sys.executable, "-m", "bayeslms_amd.train", "--data", "missing_corpus", "--cuda", "--save", "missing_model.pt"] + list(extra)
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=300, env=e)


@pytest.mark.parametrize("extra,env,msg", [
    (("--distill-weight", "0.3"), None, "--distill-weight needs --distill-from"),
    (("--distill-mc-samples", "4"), None, "--distill-mc-samples needs --distill-from"),
    (("--distill-teacher-args", "--emsize 64"), None, "--distill-teacher-args needs --distill-from"),
    (("--distill-from", "missing_teacher.pt", "--distill-weight", "1.5"), None, "--distill-weight must lie in [0, 1]"),
    (("--distill-from", "missing_teacher.pt", "--distill-weight", "-0.1"), None, "--distill-weight must lie in [0, 1]"),
    (("--distill-from", "missing_teacher.pt", "--distill-mc-samples", "1"), None, "--distill-mc-samples must be 0"),
    (("--distill-from", "missing_teacher.pt", "--distill-mc-samples", "65"), None, "--distill-mc-samples must be 0"),
    (("--distill-from", "missing_teacher.pt"), {"WORLD_SIZE": "2"}, "single process"),
    (("--distill-from", "missing_teacher.pt", "--noise-source", "torch"), None, "--noise-source torch"),
])
def test_cli_refuses(extra, env, msg):
    """Refused before the input paths are looked at (neither the corpus nor the teacher exists) and before any device is."""
    r = _cli(*extra, env=env)
    assert r.returncode != 0
    assert msg in r.stderr, r.stderr


def test_cli_refuses_a_teacher_over_another_vocabulary(tmp_path):
    """The one refusal that has to read its inputs -- words.txt and the teacher's state_dict, on the host -- still comes before
    the device is looked for (this test runs without one)."""
    import torch
    data = tmp_path / "corpus"
    data.mkdir()
    (data / "words.txt").write_text("".join("%s %d\n" % (w, i) for i, w in enumerate(["<s>", "<unk>", "a", "b", "c"])))
    teacher = tmp_path / "teacher.pt"
    torch.save({"encoder.weight": torch.zeros(7, 4), "decoder.weight": torch.zeros(7, 4), "decoder.bias": torch.zeros(7)}, str(teacher))
    r = _cli("--distill-from", str(teacher), "--data", str(data))
    assert r.returncode != 0
    assert "the teacher's vocabulary has 7 words" in r.stderr and "has 5" in r.stderr, r.stderr
