"""CPU: the host side of local reparameterisation -- the training switch, the new entry points' prototypes, the stream class
and the refusals that need no device."""
import pytest


def test_parser_default_is_off():
    from bayeslms_amd import train as T
    base = ["--data", "x", "--model", "Transformer"]
    assert T.build_parser().parse_args(base).local_reparam == 0
    assert T.build_parser().parse_args(base + ["--local-reparam", "1"]).local_reparam == 1


def test_torch_noise_source_is_refused_before_any_device_is_touched(monkeypatch):
    import torch
    from bayeslms_amd import train as T

    def touched(*a, **k):
        raise AssertionError("a device call was made before the refusal")
    for name in ("is_available", "set_device", "device_count"):
        monkeypatch.setattr(torch.cuda, name, touched)
    with pytest.raises(SystemExit, match="local-reparam"):
        T.main(["--data", "/nonexistent", "--cuda", "--local-reparam", "1", "--noise-source", "torch"])
    monkeypatch.setenv("BLM_NOISE_SOURCE", "torch")  # the same source selected from outside
    with pytest.raises(SystemExit, match="local-reparam"):
        T.main(["--data", "/nonexistent", "--cuda", "--local-reparam", "1"])


def test_new_entry_points_are_exported_with_prototypes_and_return_statuses():
    import ctypes as C
    from bayeslms_amd import _lib as L
    names = ("blm_lrt_prepare", "blm_lrt_combine", "blm_lrt_bwd_factor", "blm_lrt_mul")
    lib = L.lib()  # resolves every name of SIGNATURES: a missing export raises here
    for n in names:
        assert n in L.SIGNATURES and L.SIGNATURES[n][0] is C.c_int and n not in L.VALUE_RETURNING
    r = L.rng(1, L.STREAM_LRT, 0)
    # NULL operands, negative and huge extents, a column window outside the global batch: a status and a message, no launch
    bad = [lib.blm_lrt_prepare(None, None, 4, 0, None), lib.blm_lrt_prepare(16, 16, -1, 0, None), lib.blm_lrt_prepare(16, 32, 4, 2, None),
           lib.blm_lrt_prepare(16, 32, 2 ** 41, 0, None),
           lib.blm_lrt_combine(None, None, None, None, 1, 1, 1, 0, 0, None), lib.blm_lrt_combine(16, 32, None, None, 1, 1, 4, 0, 0, None),
           lib.blm_lrt_combine(16, 16, None, C.byref(r), 1, 1, 4, 0, 0, None), lib.blm_lrt_combine(16, 32, None, C.byref(r), -1, 1, 4, 0, 0, None),
           lib.blm_lrt_combine(16, 32, None, C.byref(r), 2 ** 30, 2 ** 30, 4, 0, 0, None),
           lib.blm_lrt_combine(16, 32, None, C.byref(r), 2, 8, 4, 8, 8, None),
           lib.blm_lrt_bwd_factor(16, 32, None, None, C.byref(r), 1, 1, 4, 0, 0, None),
           lib.blm_lrt_bwd_factor(16, 32, 48, None, C.byref(r), 2, 8, 4, -1, 16, None),
           lib.blm_lrt_mul(None, 16, 16, 4, 1.0, 0, None), lib.blm_lrt_mul(16, 16, 16, -4, 1.0, 0, None)]
    assert bad == [L.ERR_INVALID] * len(bad), bad
    assert b"blm_lrt_mul" in lib.blm_last_error()
    # nothing to do is not an error
    assert lib.blm_lrt_prepare(16, 32, 0, 0, None) == L.OK and lib.blm_lrt_combine(16, 32, None, C.byref(r), 0, 4, 4, 0, 0, None) == L.OK


def test_stream_class_is_disjoint_from_the_existing_ones():
    from bayeslms_amd import _lib as L
    classes = [L.STREAM_WEIGHT, L.STREAM_DROPOUT, L.STREAM_LRT]
    assert len({c >> 28 for c in classes}) == 3 and all(c & 0x0FFFFFFF == 0 for c in classes)
    top_id = (1 << 28) - 1  # the largest tensor / site id model.bind_state hands out stays inside its class
    assert len({(c + i) & 0xFFFFFFFF for c in classes for i in (0, top_id)}) == 6
    import re
    import os
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "bayeslm.h")).read()
    assert int(re.search(r"#define BLM_STREAM_LRT\s+(0x[0-9a-fA-F]+)u", hdr).group(1), 16) == L.STREAM_LRT


def test_refusals_name_the_site_without_a_device():
    import torch
    from bayeslms_amd import BayesLMError, model as M
    torch.manual_seed(0)
    ok = M.BayesTransformerModel(50, 16, 2, 32, 2, 0.2, True, "FFN")
    assert M._local_reparam_refusals(ok) == []
    for site, m in (("MHA", M.BayesTransformerModel(50, 16, 2, 32, 2, 0.2, True, "MHA")),
                    ("EMB", M.BayesTransformerModel(50, 16, 2, 32, 2, 0.2, False, "EMB")),
                    ("LSTM", M.BayesRNNModel("LSTM", 50, 16, 16, 2, 0.2, True, 3))):
        m.set_local_reparam(True)
        with pytest.raises(BayesLMError, match=r"local_reparam.*\b%s\b" % site):  # the pre-forward check: no kernel is reached
            m(torch.zeros(4, 2, dtype=torch.long))
    ok.set_local_reparam(True)
    with pytest.raises(BayesLMError, match="local_reparam"):
        with M.mc_sampling(ok, 1, 2):
            pass
    lin = M.BayesLinear(8, 4)
    lin._st().local_reparam = True
    lin._st().source = "torch"
    with pytest.raises(BayesLMError, match="torch"):
        lin(torch.zeros(2, 8))
