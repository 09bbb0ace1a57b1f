"""CPU: the binding's two views of one library -- _lib.lib() returns statuses, _lib.calls() raises on them (host-only calls:
argument validation happens before any HIP call, so a failure is observable without a GPU)."""
import ast
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import ROOT

# the entries whose declaration in include/bayeslm.h returns a value, not a blm_status
VALUE_RETURNING = {
    "blm_abi_version", "blm_last_error", "blm_get_gemm_mode", "blm_gemm_plan_get_cus", "blm_gemm_plan_comm_window_left",
    "blm_mfma_probe_ws_floats", "blm_ln_bwd_ws_floats", "blm_attn_bwd_ws_floats", "blm_attn_decode_ws_floats",
    "blm_linear_nll_ws_floats", "blm_linear_mc_stats_ws_floats", "blm_linear_mc_logprobs_ws_floats",
    "blm_linear_nll2_wcat_floats", "blm_linear_nll2_ws_floats", "blm_linear_nll_edges_ws_floats",
    "blm_linear_nll2_edges_ws_floats", "blm_sqnorm_ws_floats", "blm_mix2_partials", "blm_lstm_search_cell_partials",
    "blm_lstm_search_step_partials"}


@pytest.fixture(scope="module")
def L():
    from bayeslms_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _bad_calls(L):
    """(entry, arguments the library rejects, status): nothing here reaches the HIP runtime."""
    buf = (C.c_float * 16)()
    g = L.GemmArgs()
    g.abi_version = L.ABI_VERSION + 1
    attn_bwd_ws = (None,) * 3 + (0,) + (None,) * 6 + (0, 0, 0, 0, 0, 0.0, None, 0, 0, None, 0, None)
    return [("blm_transpose", (None, None, 4, 4, None), L.ERR_INVALID),
            ("blm_transpose", (C.addressof(buf), C.addressof(buf), -4, 4, None), L.ERR_INVALID),
            ("blm_gemm", (C.byref(g), None), L.ERR_ABI),
            ("blm_gemm", (None, None), L.ERR_INVALID),
            ("blm_attn_bwd_ws", attn_bwd_ws, L.ERR_INVALID)], (buf, g)


def test_checked_view_raises_what_check_raises_and_raw_view_returns(L):
    cases, keep = _bad_calls(L)
    assert L.lib()._handle == L.calls()._handle  # one library: options, planner state and the error message are shared
    for name, args, status in cases:
        rc = getattr(L.lib(), name)(*args)  # the raw view returns the status, it does not raise
        assert rc == status, (name, rc)
        with pytest.raises(L.BayesLMError) as want:
            L.check(getattr(L.lib(), name)(*args), name)
        with pytest.raises(L.BayesLMError) as got:
            getattr(L.calls(), name)(*args)
        assert str(got.value) == str(want.value) and str(got.value).startswith("%s failed (status %d): " % (name, status))
        assert got.value.status == status
    assert L.calls().blm_gemm_plan_clear(0) == L.OK  # a call that succeeds returns its status


def test_every_entry_is_classified_from_the_header(L):
    assert L.VALUE_RETURNING == VALUE_RETURNING and VALUE_RETURNING <= set(L.SIGNATURES)
    for name in L.SIGNATURES:
        assert (getattr(L.calls(), name).errcheck is not None) == (name not in VALUE_RETURNING), name
        assert getattr(L.lib(), name).errcheck is None, name
    # every status-returning entry is an `int` in the header, and the two `int` getters are the only ints that are values
    for name, (res, _) in L.SIGNATURES.items():
        if name not in VALUE_RETURNING:
            assert res is C.c_int, name
    assert sorted(n for n in VALUE_RETURNING if L.SIGNATURES[n][0] is C.c_int) == ["blm_gemm_plan_get_cus", "blm_get_gemm_mode"]


def test_value_returning_getters_are_not_checked(L):
    calls = L.calls()
    assert calls.blm_get_gemm_mode() == 0
    calls.blm_set_gemm_mode(1)
    try:
        assert calls.blm_get_gemm_mode() == 1 and L.lib().blm_get_gemm_mode() == 1  # a non-zero VALUE: returned, not raised
    finally:
        calls.blm_set_gemm_mode(0)
    assert calls.blm_gemm_plan_get_cus() > 0
    assert calls.blm_attn_bwd_ws_floats(16, 4, 4, 16) >= 0


def _roctx_library():
    for so in ("librocprofiler-sdk-roctx.so", "libroctx64.so"):
        try:
            C.CDLL(so)
            return so
        except OSError:
            pass
    return None


def test_roctx_ranges_wrap_the_checked_view():
    """BLM_ROCTX=1: a failing call through the checked view still raises with the entry's name, the raw view still returns, and
    every call of either view is exactly one range (the message of a failure is fetched outside the ranges)."""
    if _roctx_library() is None:
        pytest.skip("no roctx library on this machine")
    code = ("from bayeslms_amd import _lib as L\n"
            "calls, lib = L.calls(), L.lib()\n"
            "n0 = L.ROCTX_RANGES[0]\n"
            "try:\n"
            "    calls.blm_transpose(None, None, 4, 4, None)\n"
            "    raise SystemExit('did not raise')\n"
            "except L.BayesLMError as e:\n"
            "    assert str(e).startswith('blm_transpose failed (status -1): blm_transpose'), str(e)\n"
            "assert L.ROCTX_RANGES[0] == n0 + 1, L.ROCTX_RANGES\n"
            "assert lib.blm_transpose(None, None, 4, 4, None) == L.ERR_INVALID\n"
            "assert calls.blm_get_gemm_mode() == 0 and calls.blm_gemm_plan_clear(0) == 0\n"
            "assert L.ROCTX_RANGES[0] == n0 + 4, L.ROCTX_RANGES\n"
            "print('RANGES OK')\n")
    env = dict(os.environ, BLM_ROCTX="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "RANGES OK" in r.stdout, (r.stdout, r.stderr[-2000:])


def test_ops_names_no_entry_point_twice():
    """ops.py goes through the checked view alone: no call of check(), and no blm_* string handed to a call as its label."""
    tree = ast.parse(open(os.path.join(ROOT, "bayeslms_amd", "ops.py")).read())
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call)]
    assert len(calls) > 1000
    bad = [n.lineno for n in calls if isinstance(n.func, ast.Name) and n.func.id == "check"]
    bad += [n.lineno for n in calls if len(n.args) >= 2 and isinstance(n.args[1], ast.Constant)
            and isinstance(n.args[1].value, str) and n.args[1].value.startswith("blm_")]
    assert not bad, bad
    names = {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)}
    assert "check" not in names and "lib" not in names  # neither imported nor used: the raw view is not what ops calls
