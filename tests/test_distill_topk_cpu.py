"""CPU: blm_ce_soft_topk_fwd_bwd is declared, exported, bound and refuses bad arguments on the host, before any launch;
distill.TeacherCache round-trips rows bit for bit, refuses a file written for anything else and rebuilds an unfinished one;
the --distill-top-k / --distill-cache flags of bayeslms_amd.train are refused before a device is looked for."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")
NAME = "blm_ce_soft_topk_fwd_bwd"


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
    proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, src)
    assert proto, "not declared"
    params = [" ".join(p.split()) for p in proto.group(1).split(",")]
    assert params == ["const float* logits", "int64_t ld", "const int32_t* ids", "const float* logq", "int64_t ldk", "int K",
                      "const int64_t* tgt", "float lambda", "float* loss", "float* nll", "float* soft", "float* kl", "float* lse",
                      "float* loss_sum", "float* dlogits", "float grad_scale", "int M", "int V", "void* stream"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    assert NAME in {line.split()[-1] for line in out.splitlines() if " T " in line}
    L, l = lib
    res, args = L.SIGNATURES[NAME]
    want = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_float] + [C.c_void_p] * 7 + \
           [C.c_float, C.c_int, C.c_int, C.c_void_p]
    assert res is C.c_int and list(args) == want
    assert NAME not in L.VALUE_RETURNING and getattr(L.calls(), NAME).errcheck is not None  # in the checked view
    assert L.ABI_VERSION == 1 and l.blm_abi_version() == 1
    assert L.TOPK_MAX == int(re.search(r"^#define BLM_TOPK_MAX (\d+)", text, flags=re.M).group(1))


# addresses that are never dereferenced: logits, ids, logq, targets, per-row outputs, a separate gradient buffer far from all of them
Z, I, Q, T, O, D = 0x100000, 0x700000, 0x900000, 0x10000, 0x20000, 0x1100000
M, V, K = 4, 10, 3


def call(l, logits=Z, ld=V, ids=I, logq=Q, ldk=K, k=K, tgt=T, lam=0.5, loss=O, nll=O + 64, soft=O + 128, kl=O + 192, lse=None,
         loss_sum=None, dlogits=D, m=M, v=V):
    return getattr(l, NAME)(logits, ld, ids, logq, ldk, k, tgt, lam, loss, nll, soft, kl, lse, loss_sum, dlogits, 0.25, m, v, None)


@pytest.mark.parametrize("kw,msg", [
    (dict(logits=None), b"logits is NULL"), (dict(ids=None), b"ids is NULL"), (dict(logq=None), b"logq is NULL"),
    (dict(tgt=None), b"tgt is NULL"), (dict(loss=None), b"loss is NULL"),
    (dict(m=-1), b"M = -1"), (dict(v=0), b"V = 0"), (dict(v=-3, ld=0), b"V = -3"),
    (dict(k=0), b"K = 0"), (dict(k=-2), b"K = -2"), (dict(k=257, ldk=257), b"K = 257"), (dict(k=2 ** 31 - 1, ldk=2 ** 31), b"K = 2147483647"),
    (dict(ld=V - 1), b"ld = 9"), (dict(ldk=K - 1), b"ldk = 2"), (dict(ld=2 ** 40), b"ld = "), (dict(ldk=2 ** 40), b"ldk = "),
    (dict(ld=-5), b"ld = -5"), (dict(ldk=-5), b"ldk = -5"), (dict(m=2 ** 31 - 1, ld=2 ** 30), b"ld = "),
    (dict(lam=-0.01), b"lambda"), (dict(lam=1.5), b"lambda"), (dict(lam=float("nan")), b"lambda"),
    (dict(dlogits=I), b"overlaps ids"), (dict(dlogits=I + 4 * (M * K - 1)), b"overlaps ids"),
    (dict(dlogits=I - 4 * (M * V - 1)), b"overlaps ids"),
    (dict(dlogits=Q), b"overlaps logq"), (dict(dlogits=Q + 4 * (M * K - 1)), b"overlaps logq"),
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
    assert call(l, m=0, k=0) == L.ERR_INVALID
    with pytest.raises(L.BayesLMError, match=NAME):
        getattr(L.calls(), NAME)(None, V, I, Q, K, K, T, 0.5, O, None, None, None, None, None, None, 1.0, M, V, None)


# ------------------------------------------------------------------------------------------------------- TeacherCache
ROWS, COLS, SEQ, CK = 12, 3, 4, 5  # 11 x 3 = 33 cached rows in windows of 4, 4 and a ragged 3 time steps


def fields(**over):
    from bayeslms_amd.distill import TeacherCache
    f = dict(vocab=40, k=CK, renorm=False, seq_len=SEQ, rows=ROWS, columns=COLS, data_sha256="d" * 64, teacher_sha256="t" * 64,
             teacher_flags={"model": "Transformer", "emsize": 32, "tied": True}, mc_samples=2, mc_seed=1111)
    f.update(over)
    return TeacherCache.describe(**f)


def rows_of_the_walk():
    g = torch.Generator().manual_seed(11)
    n = (ROWS - 1) * COLS
    ids = torch.randint(-1, 40, (n, CK), generator=g, dtype=torch.int32)
    logq = torch.randn(n, CK, generator=g)
    logq[1, 2], logq[5, 0] = -float("inf"), -0.0  # bit for bit: the sign of a zero and an infinity come back
    return ids, logq


def windows():
    return [(i * COLS, min(SEQ, ROWS - 1 - i) * COLS) for i in range(0, ROWS - 1, SEQ)]


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_cache_round_trips_bit_for_bit(tmp_path):
    from bayeslms_amd import ops
    from bayeslms_amd.distill import TeacherCache
    path = str(tmp_path / "teacher.cache")
    ids, logq = rows_of_the_walk()
    c = TeacherCache(path, fields())
    assert not c.complete and c.n == 33
    assert [w for w in windows()] == [(0, 12), (12, 12), (24, 9)]  # the last window is ragged
    for off, n in reversed(windows()):  # stored out of order
        c.store(off, ops.SparseTargets(ids[off:off + n], logq[off:off + n]))
    assert not json.loads(open(path, "rb").read(TeacherCache.HEADER_BYTES))["complete"]
    c.finish()
    assert c.complete and json.loads(open(path, "rb").read(TeacherCache.HEADER_BYTES))["complete"]
    assert os.path.getsize(path) == TeacherCache.HEADER_BYTES + 33 * CK * 8
    for reader in (c, TeacherCache(path, fields())):
        assert reader.complete
        for off, n in windows():
            got = reader.load(off, n, "cpu")
            assert isinstance(got, ops.SparseTargets) and got.ids.dtype == torch.int32 and got.logq.dtype == torch.float32
            assert got.ids.shape == got.logq.shape == (n, CK)
            assert torch.equal(got.ids, ids[off:off + n]) and same_bits(got.logq, logq[off:off + n])
    with pytest.raises(ValueError, match="complete"):
        c.store(0, ops.SparseTargets(ids[:12], logq[:12]))
    for off, n in ((-1, 4), (30, 4), (0, 0)):
        with pytest.raises(IndexError):
            c.load(off, n, "cpu")


@pytest.mark.parametrize("field,over", [
    ("vocab", dict(vocab=41)), ("k", dict(k=CK + 1)), ("renorm", dict(renorm=True)), ("seq_len", dict(seq_len=SEQ + 1)),
    ("rows", dict(rows=ROWS + 1)), ("columns", dict(columns=COLS + 1)), ("data_sha256", dict(data_sha256="e" * 64)),
    ("teacher_sha256", dict(teacher_sha256="u" * 64)),
    ("teacher_flags", dict(teacher_flags={"model": "Transformer", "emsize": 64, "tied": True})),
    ("mc_samples", dict(mc_samples=0)), ("mc_seed", dict(mc_seed=7)),
])
def test_cache_refuses_a_header_that_differs_in_one_field(tmp_path, field, over):
    from bayeslms_amd import ops
    from bayeslms_amd.distill import CacheMismatch, TeacherCache
    path = str(tmp_path / "teacher.cache")
    ids, logq = rows_of_the_walk()
    c = TeacherCache(path, fields())
    c.store(0, ops.SparseTargets(ids, logq))
    c.finish()
    before = open(path, "rb").read()
    with pytest.raises(CacheMismatch) as e:
        TeacherCache(path, fields(**over))
    assert e.value.field == field
    text = str(e.value)
    assert repr(field) in text and repr(fields()[field]) in text and repr(fields(**over)[field]) in text, text
    assert open(path, "rb").read() == before  # a refused file is left as it was


def test_cache_refuses_another_format_version(tmp_path, monkeypatch):
    from bayeslms_amd.distill import CacheMismatch, TeacherCache
    path = str(tmp_path / "teacher.cache")
    TeacherCache(path, fields())
    monkeypatch.setattr(TeacherCache, "VERSION", TeacherCache.VERSION + 1)
    with pytest.raises(CacheMismatch, match="'version'"):
        TeacherCache(path, fields())


def test_cache_without_complete_is_rebuilt(tmp_path):
    from bayeslms_amd import ops
    from bayeslms_amd.distill import TeacherCache
    path = str(tmp_path / "teacher.cache")
    ids, logq = rows_of_the_walk()
    c = TeacherCache(path, fields())
    c.store(0, ops.SparseTargets(ids[:12], logq[:12]))  # an interrupted first epoch: never finished
    c.ids.flush()
    del c
    c = TeacherCache(path, fields())
    assert not c.complete
    assert not c.ids[:].any() and not c.logq[:].any()  # from the start: nothing of the partial file is kept
    c.store(0, ops.SparseTargets(ids, logq))
    c.finish()
    got = TeacherCache(path, fields()).load(0, 33, "cpu")
    assert torch.equal(got.ids, ids) and same_bits(got.logq, logq)
    with open(path, "r+b") as f:  # a complete header on a truncated file is no complete cache either
        f.truncate(TeacherCache.HEADER_BYTES + 100)
    assert not TeacherCache(path, fields()).complete


# ----------------------------------------------------------------------------------------------- command line
def test_parser_defaults_are_off():
    from bayeslms_amd import train
    a = train.build_parser().parse_args([])
    assert a.distill_top_k == 0 and a.distill_top_k_renorm == 0 and a.distill_cache == ""
    assert train.check_distill_args(a, 1) is None
    b = train.build_parser().parse_args(["--distill-from", "t.pt", "--distill-top-k", "32", "--distill-top-k-renorm", "1",
                                         "--distill-cache", "c.bin"])
    assert train.check_distill_args(b, 1) is not None
    assert (b.distill_top_k, b.distill_top_k_renorm, b.distill_cache) == (32, 1, "c.bin")


def _cli(*extra):
    argv = [sys.executable, "-m", "bayeslms_amd.train", "--data", "missing_corpus", "--cuda", "--save", "missing_model.pt"] + list(extra)
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    return subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=300, env=e)


@pytest.mark.parametrize("extra,msg", [
    (("--distill-top-k", "8"), "--distill-top-k needs --distill-from"),
    (("--distill-top-k-renorm", "1"), "--distill-top-k-renorm needs --distill-from"),
    (("--distill-cache", "c.bin"), "--distill-cache needs --distill-from"),
    (("--distill-from", "missing_teacher.pt", "--distill-cache", "c.bin"), "--distill-cache needs --distill-top-k"),
    (("--distill-from", "missing_teacher.pt", "--distill-top-k-renorm", "1"), "--distill-top-k-renorm needs --distill-top-k"),
    (("--distill-from", "missing_teacher.pt", "--distill-top-k", "257"), "--distill-top-k must lie in 1..256"),
    (("--distill-from", "missing_teacher.pt", "--distill-top-k", "-1"), "--distill-top-k must lie in 1..256"),
])
def test_cli_refuses(extra, msg):
    """Refused before the input paths are looked at (neither the corpus nor the teacher exists) and before any device is."""
    r = _cli(*extra)
    assert r.returncode != 0
    assert msg in r.stderr, r.stderr


def test_cli_refuses_more_targets_than_words(tmp_path):
    """Needs words.txt and the teacher's state_dict, on the host; still before the device is looked for."""
    data = tmp_path / "corpus"
    data.mkdir()
    (data / "words.txt").write_text("".join("%s %d\n" % (w, i) for i, w in enumerate(["<s>", "<unk>", "a", "b", "c"])))
    teacher = tmp_path / "teacher.pt"
    torch.save({"encoder.weight": torch.zeros(5, 4), "decoder.weight": torch.zeros(5, 4), "decoder.bias": torch.zeros(5)}, str(teacher))
    r = _cli("--distill-from", str(teacher), "--data", str(data), "--distill-top-k", "6")
    assert r.returncode != 0
    assert "--distill-top-k 6: the vocabulary" in r.stderr and "has 5 words" in r.stderr, r.stderr
