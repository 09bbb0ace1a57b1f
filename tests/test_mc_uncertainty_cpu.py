"""CPU: the Monte-Carlo uncertainty entry points -- header, bindings, argument checks before any HIP call, the CLI's refusals
before any model load or device check, and the uncertainty file's format (no compute)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "bayeslm.h")
LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")
FAKE = 4096  # a non-NULL address that is never dereferenced: validation returns first


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from bayeslms_amd import _lib
    return _lib.lib()


def test_header_declares_and_bindings_bind_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int64_t\s+blm_linear_mc_stats_ws_floats\s*\(\s*int M,\s*int S,\s*int V\s*\)", src)
    assert re.search(r"int\s+blm_linear_mc_stats\s*\(", src)
    assert "BLM_EPI_MC_PART" in src
    from bayeslms_amd import _lib
    assert "blm_linear_mc_stats" in _lib.SIGNATURES and "blm_linear_mc_stats_ws_floats" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["blm_linear_mc_stats"][1]) == 16


def _call(lib, S=8, V=1000, K=64, M=16, ldx=64, ldw=64, mi=FAKE):
    return lib.blm_linear_mc_stats(FAKE, ldx, FAKE, ldw, None, FAKE, S, None, FAKE, FAKE, mi, FAKE, M, V, K, None)


@pytest.mark.parametrize("kw,msg", [({"S": 0}, b"S must be in 1..64"), ({"S": 65}, b"S must be in 1..64"), ({"V": 0}, b"bad shape"),
                                    ({"ldx": 32}, b"leading dimension"), ({"mi": None}, b"null output"),
                                    ({"M": 1 << 29, "ldx": 1 << 12, "K": 64}, b"extents")])
def test_argument_errors_fail_before_any_hip_call(lib, kw, msg):
    assert _call(lib, **kw) != 0
    assert msg in lib.blm_last_error()


def test_blm_gemm_refuses_the_internal_epilogue(lib):
    import ctypes
    from bayeslms_amd import _lib
    a = _lib.GemmArgs()
    a.abi_version = _lib.ABI_VERSION
    a.op, a.M, a.N, a.K, a.lda, a.ldb, a.ldc = 0, 64, 64, 64, 64, 64, 64
    a.A = a.B = a.C = FAKE
    a.epilogue = 8
    assert lib.blm_gemm(ctypes.byref(a), None) != 0
    assert b"internal to blm_linear_mc_stats" in lib.blm_last_error()


def test_workspace_size(lib):
    f = lib.blm_linear_mc_stats_ws_floats
    # Sp = 8 rows per token: blm_linear_nll's workspace over M * 8 rows of the padded vocabulary, plus nll and lse per row
    assert f(100, 5, 1001) == lib.blm_linear_nll_ws_floats(800, 1004) + 2 * 800
    assert f(3, 1, 8) == lib.blm_linear_nll_ws_floats(3, 8) + 6
    for bad in ((1 << 30, 64, 33000), (-1, 8, 1000), (10, 0, 1000), (10, 65, 1000), (10, 8, 0), (1 << 25, 64, 1 << 20)):
        assert f(*bad) == 0, bad


def _cli(*extra):
    argv = [sys.executable, "-m", "bayeslms_amd.compute_sentence_scores", "--nbest-list", "missing_nbest", "--outfile", "missing_out",
            "--vocabulary", "missing_vocab", "--model-path", "missing_model", "--write-uncertainty", "unc.txt"] + list(extra)
    return subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("extra", [(), ("--mc-samples", "1"), ("--mc-samples", "8", "--interpolation_flag", "1")])
def test_cli_refuses_write_uncertainty_without_samples(extra):
    """Refused before the input paths are checked, any model is loaded or a device is looked for."""
    r = _cli(*extra)
    assert r.returncode != 0
    assert "--write-uncertainty needs --mc-samples >= 2 and --interpolation_flag 0" in r.stderr, r.stderr


def test_uncertainty_file_format(tmp_path):
    from collections import OrderedDict
    from bayeslms_amd.compute_sentence_scores import HypUncertainty, write_scores, write_uncertainty
    scores, unc = OrderedDict(), OrderedDict()
    scores["utt_b"] = [("a b", 12.345678), ("a c", 7.0)]
    scores["utt_a"] = [("x", 0.123456789)]
    f32 = lambda *v: np.asarray(v, dtype=np.float32)  # noqa: E731
    unc["utt_b"] = [("a b", HypUncertainty(f32(1.5, 2.25), f32(3.0, 4.0), f32(0.125, 1e-7), 0.0123456789)),
                    ("a c", HypUncertainty(f32(7.0), f32(2.0), f32(0.0), 0.0))]
    unc["utt_a"] = [("x", HypUncertainty(f32(0.1, 0.2, 0.3), f32(1.0, 1.0, 1.0), f32(0.01, 0.02, 0.03), 123456.789))]
    write_scores(scores, str(tmp_path / "s.txt"))
    write_uncertainty(scores, unc, str(tmp_path / "u.txt"))
    s = [ln.split() for ln in open(tmp_path / "s.txt").read().splitlines()]
    u = open(tmp_path / "u.txt").read().splitlines()
    assert [ln.split()[0] for ln in u] == [a[0] for a in s] == ["utt_b-1", "utt_b-2", "utt_a-1"]
    assert all(len(ln.split()) == 7 for ln in u)
    assert [ln.split()[1] for ln in u] == [a[1] for a in s]
    assert u[0] == "utt_b-1 12.3457 0.0123457 3.75 7 0.125 2"
    assert u[1] == "utt_b-2 7.0000 0 7 2 0 1"
    assert u[2].split()[2] == "123457" and u[2].split()[-1] == "3"
    assert u[2].split()[3:6] == ["%.6g" % float(np.sum(f32(0.1, 0.2, 0.3), dtype=np.float64)), "3",
                                 "%.6g" % float(np.sum(f32(0.01, 0.02, 0.03), dtype=np.float64))]
