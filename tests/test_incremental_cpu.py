"""CPU: the incremental-decoding entry points (csrc/decode.hip) are declared and exported, size their workspace, refuse bad
arguments on the host before any launch; IncrementalLM validates its model and arguments before touching a GPU."""
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT

NEW = ("blm_attn_decode", "blm_attn_decode_ws_floats", "blm_kv_append", "blm_kv_gather", "blm_embed_at", "blm_log_softmax_rows",
       "blm_sample_rows")
LIB = os.path.join(ROOT, "bayeslms_amd", "libbayeslm_hip.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from bayeslms_amd import _lib as L
    return L, L.lib()


def test_header_declares_and_library_exports_the_decode_entry_points(lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bayeslm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(blm_[a-z0-9_]+)\s*\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NEW:
        assert name in declared and name in exported, name
    L, _ = lib
    assert all(name in L.SIGNATURES for name in NEW)


def test_attn_decode_workspace_sizes(lib):
    _, l = lib
    # Tq * N * nhead * ceil(ctx_max / 64) * (head_dim + 2)
    assert l.blm_attn_decode_ws_floats(1, 64, 8, 1024, 64) == 64 * 8 * 16 * 66
    assert l.blm_attn_decode_ws_floats(7, 3, 2, 65, 100) == 7 * 3 * 2 * 2 * 102
    assert l.blm_attn_decode_ws_floats(1, 1, 1, 1, 128) == 130
    assert l.blm_attn_decode_ws_floats(1, 1, 1, 64, 129) == 0  # head size out of range
    assert l.blm_attn_decode_ws_floats(-1, 1, 1, 64, 64) == 0
    assert l.blm_attn_decode_ws_floats(1, 1, 0, 64, 64) == 0


def test_host_side_refusals(lib):
    L, l = lib
    P = 0x10000  # never dereferenced: every call below fails its checks before a launch
    # negative sizes
    assert l.blm_attn_decode(P, 64, P, P, None, P, P, 1 << 20, -1, 1, 1, 1, 16, 64, 16, None) == L.ERR_INVALID
    assert l.blm_kv_append(P, P, 64, P, P, None, 1, -2, 4, 1, 16, 64, None) == L.ERR_INVALID
    assert l.blm_embed_at(P, P, 10, 1.0, None, None, 0, None, P, -1, 1, 8, None) == L.ERR_INVALID
    assert l.blm_log_softmax_rows(P, 10, P, 10, -1, 10, None) == L.ERR_INVALID
    assert l.blm_sample_rows(P, 10, 4, 10, -1.0, None, P, None) == L.ERR_INVALID
    # head_dim > 128
    assert l.blm_attn_decode(P, 2 * 129, P, P, None, P, P, 1 << 20, 1, 1, 1, 2, 16, 129, 16, None) == L.ERR_UNSUPPORTED
    assert b"head_dim" in l.blm_last_error()
    # ctx_max past max_len, stream capacity below the stream count, too small a workspace
    assert l.blm_attn_decode(P, 64, P, P, None, P, P, 1 << 20, 1, 1, 1, 1, 16, 64, 17, None) == L.ERR_INVALID
    assert l.blm_attn_decode(P, 64, P, P, None, P, P, 1 << 20, 1, 4, 2, 1, 16, 64, 16, None) == L.ERR_INVALID
    assert l.blm_attn_decode(P, 64, P, P, None, P, P, 10, 1, 1, 1, 1, 16, 64, 16, None) == L.ERR_INVALID
    # overlapping gather ranges: state bytes = outer * n_cap * nhead * max_len * head_dim * 4
    n = 2 * 4 * 2 * 8 * 16 * 4
    assert l.blm_kv_gather(P, P + n - 16, P, None, None, 2, 4, 4, 2, 2, 8, 16, None) == L.ERR_INVALID
    assert b"overlap" in l.blm_last_error()
    assert l.blm_kv_gather(P + n - 16, P, P, None, None, 2, 4, 4, 2, 2, 8, 16, None) == L.ERR_INVALID
    assert l.blm_kv_gather(P, P, P, None, None, 2, 4, 4, 2, 2, 8, 16, None) == L.ERR_INVALID
    # log-softmax: x and out overlapping other than exactly in place (same pointer, same stride)
    assert l.blm_log_softmax_rows(P, 12, P + 16, 12, 4, 10, None) == L.ERR_INVALID
    assert l.blm_log_softmax_rows(P, 12, P, 16, 4, 10, None) == L.ERR_INVALID
    # more output streams than the capacity
    assert l.blm_kv_gather(P, P + 4 * n, P, None, None, 5, 4, 4, 2, 2, 8, 16, None) == L.ERR_INVALID


def _tiny_transformer():
    from bayeslms_amd import model as M
    return M.TransformerModel(20, 16, 2, 32, 1, 0.1, "gelu", True)


def test_incremental_lm_argument_validation():
    from bayeslms_amd import BayesLMError
    from bayeslms_amd import model as M
    from bayeslms_amd import model_search_bayes as S
    from bayeslms_amd.incremental import IncrementalLM
    m = _tiny_transformer()
    with pytest.raises(BayesLMError, match="training mode"):
        IncrementalLM(m)  # nn.Module starts in training mode
    m.eval()
    with pytest.raises(BayesLMError, match="positional table"):
        IncrementalLM(m, max_len=5001)
    with pytest.raises(BayesLMError, match="GPU"):
        IncrementalLM(m)  # a CPU model
    with pytest.raises(BayesLMError, match="not one of"):
        IncrementalLM(torch.nn.Linear(3, 3).eval())
    supernets = [c for c in vars(S).values() if isinstance(c, type) and c.__name__.endswith("Search") and issubclass(c, torch.nn.Module)]
    assert supernets
    for cls in supernets:
        fake = cls.__new__(cls)  # the refusal is decided by the class, before anything of the instance is read
        with pytest.raises(BayesLMError, match="super-net"):
            IncrementalLM(fake)
    lstm = M.RNNModel("LSTM", 20, 16, 16, 2, 0.1, True).eval()
    with pytest.raises(BayesLMError, match="GPU"):
        IncrementalLM(lstm)
