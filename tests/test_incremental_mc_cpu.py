"""CPU: the model average's next-word distribution (blm_linear_mc_logprobs) is declared, exported and bound, sizes its workspace and
refuses bad arguments on the host before any HIP call; IncrementalLM and the generate CLI refuse bad Monte-Carlo arguments before
any GPU use."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

NEW = ("blm_linear_mc_logprobs", "blm_linear_mc_logprobs_ws_floats")
LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")
FAKE = 0x10000  # never dereferenced: every call below fails its checks before a launch


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from bayeslms_amd import _lib
    return _lib.lib()


def test_header_library_and_binding_agree(lib):
    from bayeslms_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bayeslm.h")).read(), flags=re.S)
    assert re.search(r"int64_t\s+blm_linear_mc_logprobs_ws_floats\s*\(\s*int M,\s*int S,\s*int V\s*\)", src)
    assert re.search(r"int\s+blm_linear_mc_logprobs\s*\(", src)
    assert re.search(r"BLM_EPI_MC_LOGP\s*=\s*9\b", src)
    assert re.search(r"#define\s+BLM_ABI_VERSION\s+1u?\b", src)  # additive: the ABI version stays
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in exported and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["blm_linear_mc_logprobs"][1]) == 18


def test_workspace_size(lib):
    f = lib.blm_linear_mc_logprobs_ws_floats
    sizes = [f(m, 5, 1001) for m in (1, 2, 64, 100, 2048)]
    assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes))  # positive, strictly growing with M
    for m, s in zip((1, 2, 64, 100, 2048), sizes):  # blm_linear_mc_stats' workspace, and room for M zero targets behind it
        assert s >= lib.blm_linear_mc_stats_ws_floats(m, 5, 1001) + 2 * m
    for bad in ((1 << 30, 64, 33000), (-1, 8, 1000), (10, 0, 1000), (10, 65, 1000), (10, 8, 0), (1 << 25, 64, 1 << 20)):
        assert f(*bad) == 0, bad


def _call(lib, S=8, V=1000, K=64, M=16, ldx=64, ldw=64, logp=FAKE, ldo=1000, tgt=None, bma=None, nll_s=None):
    return lib.blm_linear_mc_logprobs(FAKE, ldx, FAKE, ldw, None, tgt, S, logp, ldo, nll_s, bma, FAKE, FAKE, FAKE, M, V, K, None)


@pytest.mark.parametrize("kw,status,msg", [
    ({"logp": None}, "ERR_INVALID", b"null output"),
    ({"S": 0}, "ERR_INVALID", b"S must be in 1..64"),
    ({"S": 65}, "ERR_INVALID", b"S must be in 1..64"),
    ({"ldo": 996}, "ERR_UNSUPPORTED", b"ldo < V"),
    ({"ldo": 1002}, "ERR_UNSUPPORTED", b"ldo % 4 == 0"),
    ({"logp": FAKE + 4}, "ERR_UNSUPPORTED", b"16-byte aligned logp"),
    ({"V": 0}, "ERR_INVALID", b"bad shape"),
    ({"M": -1}, "ERR_INVALID", b"bad shape"),
    ({"ldx": 32}, "ERR_INVALID", b"leading dimension"),
    ({"tgt": FAKE}, "ERR_INVALID", b"bma_nll goes with tgt"),
    ({"bma": FAKE}, "ERR_INVALID", b"bma_nll goes with tgt"),
    ({"nll_s": FAKE}, "ERR_INVALID", b"bma_nll goes with tgt"),
    ({"M": 1 << 29, "ldx": 1 << 12, "K": 64}, "ERR_INVALID", b"extents"),
])
def test_argument_errors_fail_before_any_hip_call(lib, kw, status, msg):
    from bayeslms_amd import _lib
    assert _call(lib, **kw) == getattr(_lib, status)
    assert msg in lib.blm_last_error(), lib.blm_last_error()


def test_no_tokens_is_a_no_op(lib):
    from bayeslms_amd import _lib
    assert _call(lib, M=0) == _lib.OK


def test_blm_gemm_refuses_the_internal_epilogue(lib):
    from bayeslms_amd import _lib
    a = _lib.GemmArgs()
    a.abi_version = _lib.ABI_VERSION
    a.op, a.M, a.N, a.K, a.lda, a.ldb, a.ldc = 0, 64, 64, 64, 64, 64, 64
    a.A = a.B = a.C = FAKE
    a.epilogue = 9
    assert lib.blm_gemm(ctypes.byref(a), None) == _lib.ERR_INVALID
    assert b"internal to blm_linear_mc_logprobs" in lib.blm_last_error()


def test_incremental_lm_refuses_bad_sample_counts():
    """Decided before anything of the model is read, so before any GPU use."""
    from bayeslms_amd import BayesLMError
    from bayeslms_amd import model as M
    from bayeslms_amd.incremental import IncrementalLM
    m = M.BayesTransformerModel(20, 16, 2, 32, 1, 0.1, True, "FFN").eval()
    for bad in (-1, 65):
        with pytest.raises(BayesLMError, match="mc_samples must lie in 0..64"):
            IncrementalLM(m, mc_samples=bad)
    with pytest.raises(BayesLMError, match="GPU"):  # accepted values go on to the ordinary checks (a CPU model here)
        IncrementalLM(m, mc_samples=4, seed=7)


def _cli(*extra):
    argv = [sys.executable, "-m", "bayeslms_amd.generate", "--model-path", "missing_model", "--vocabulary", "missing_vocab",
            "--write-uncertainty", "unc.txt"] + list(extra)
    return subprocess.run(argv, cwd=ROOT, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("extra", [(), ("--mc-samples", "1"), ("--mc-samples", "0", "--mc-seed", "3")])
def test_generate_cli_refuses_write_uncertainty_without_samples(extra):
    """Refused before the input paths are checked, any model is loaded or a device is looked for."""
    r = _cli(*extra)
    assert r.returncode != 0
    assert "--write-uncertainty needs --mc-samples >= 2" in r.stderr, r.stderr


def test_generate_help_states_the_uncertainty_format():
    from bayeslms_amd.generate import build_parser
    text = " ".join(build_parser().format_help().split())
    assert '"word h_pred mi"' in text and "one line per stream" in text


def test_uncertainty_file_format(tmp_path):
    import numpy as np
    from bayeslms_amd.generate import write_uncertainty
    h = np.asarray([[1.5, 2.25], [7.0, 0.123456789]], dtype=np.float32)
    mi = np.asarray([[0.125, 1e-7], [0.0, 3.0]], dtype=np.float32)
    write_uncertainty([["a", "b"], ["c", "d"]], h, mi, str(tmp_path / "u.txt"))
    assert open(tmp_path / "u.txt").read() == "a 1.5 0.125 b 2.25 1e-07\nc 7 0 d 0.123457 3\n"
