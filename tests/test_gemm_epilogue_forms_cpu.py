"""CPU: every launch of tests/test_gpu_gemm_epilogue_forms.py runs the tile its table claims.  The planner is host code, so
blm_gemm_plan_query answers without a GPU; the launches are those of tests/gemm_epilogue_forms_table.py (all_launches), which
the GPU file also checks each of its own launches against.

What the query cannot show -- which epilogue body and which keep / eps form a launch takes -- is read from the code
(csrc/gemm_f32_mfma.h launch_cfg, gemm_f32_kernel, epilogue, epilogue_rows; csrc/gemm_api.hip blm_gemm) and stated in the
docstring of the GPU file; `test_the_bodies_follow_the_leading_dimension` only pins the arithmetic that table rests on."""
import ctypes as C

import pytest

import gemm_epilogue_forms_table as T
from bayeslms_amd import _lib as L


@pytest.fixture(autouse=True)
def _clean():
    lib = L.lib()
    lib.blm_gemm_plan_override(0, 0)
    yield
    lib.blm_gemm_plan_override(0, 0)


def plan(a):
    out = L.GemmPlan()
    L.check(L.lib().blm_gemm_plan_query(C.byref(a), C.byref(out)), "blm_gemm_plan_query")
    return out


def test_the_fast_rule_is_the_table():
    for (M, N, K), row in T.FAST_TABLE.items():
        assert tuple(T.is_fast(op, M, N, K) for op in (T.NT, T.NN, T.TN)) == row, (M, N, K)
    assert sorted(T.FAST_TABLE) == sorted(T.SHAPES)
    # the legalisations, written out: guarded -> 11 whatever is forced, 28 -> 22 on a K tail, 28 kept on whole K tiles
    assert [T.tile_run(T.NT, 200, 136, 98, t) for t in T.TILES] == [11] * 5
    assert [T.tile_run(T.NN, 200, 134, 96, t) for t in T.TILES] == [11] * 5
    assert [T.tile_run(T.TN, 200, 136, 98, t) for t in T.TILES] == [11, 12, 21, 22, 22]
    assert [T.tile_run(T.NT, 200, 134, 100, t) for t in T.TILES] == [11, 12, 21, 22, 22]
    assert [T.tile_run(T.NN, 200, 136, 96, t) for t in T.TILES] == [11, 12, 21, 22, 28]
    assert [T.tile_run(T.TN, 128, 128, 64, t) for t in T.TILES] == [11, 12, 21, 22, 28]


def test_every_launch_of_the_gpu_table_runs_the_claimed_tile():
    lib = L.lib()
    launches = T.all_launches()
    assert set(launches) == T.LAUNCH_SET and len(launches) >= 400
    seen = set()
    for l in launches:
        L.check(lib.blm_gemm_plan_override(l.forced, l.splits), "override")
        p = plan(T.plan_args(l))
        want = T.tile_run(l.op, l.M, l.N, l.K, l.forced)
        assert p.tile == want and p.source == 2, (l, p.tile, want)
        # slices only where the epilogue is linear in the product and C can take atomics, never with fused sampling
        lin = l.epi == L.EPI_NONE and (l.acc or l.ldc == l.N)
        if l.splits and not l.samp and (lin or (l.epi == L.EPI_BAYES_WGRAD and l.acc)):
            assert abs(p.splits) == abs(l.splits) and l.K // abs(p.splits) >= 32, (l, p.splits)
        else:
            assert p.splits == 1, (l, p.splits)
        # a misaligned operand is the other way into the guarded kernel
        assert plan(T.plan_args(l, base=(1 << 20) + 4)).tile == 11
        seen.add((l.epi, want, T.is_fast(l.op, l.M, l.N, l.K)))
    # the coverage claim: every activation epilogue at all five tiles and in the guarded kernel; the Bayesian wgrad too
    for epi in (L.EPI_BIAS_GELU, L.EPI_MUL_DGELU, L.EPI_GP_MIX, L.EPI_MUL_DGP_MIX, L.EPI_BAYES_WGRAD):
        assert {t for e, t, fast in seen if e == epi and fast} == set(T.TILES), epi
        assert (epi, 11, False) in seen, epi


def test_the_bodies_follow_the_leading_dimension():
    """launch_cfg: the row-wise body needs N % 4 == 0 and ldc % 4 == 0 (and aligned C / aux / bias / C2, no atomics); blm_gemm:
    drop_quad = N % 4 == 0.  Both bodies exist at every N % 4 == 0 shape of the table, the scalar keep form at N = 134 alone."""
    for M, N, K in T.SHAPES:
        for body in T.bodies(N):
            ld = T.ldc_of(N, body)
            rows = N % 4 == 0 and ld % 4 == 0
            assert rows == (body == "rows") and (N % 4 == 0) == (body != "register-scalar") and ld > N
    assert {b for _, N, _ in T.SHAPES for b in T.bodies(N)} == {"rows", "register-quad", "register-scalar"}
    for body in ("rows", "register-quad", "register-scalar"):
        for tile in T.TILES:  # each body at each tile the host can run: forced, fast, K whole where the tile is 28
            assert any(t == tile and b == body and T.tile_run(T.NT, M, N, K, t) == tile for t, M, N, K, b in T.ACT_MAIN), (body, tile)
