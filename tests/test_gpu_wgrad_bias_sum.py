"""GPU: the bias gradient out of the weight-gradient product (blm_gemm TN with colsum_a) against float64, on the cases the
colsum_a rows of tests/test_gpu_gemm_epilogue_forms.py leave out.  The LDS-DMA kernels sum A's columns from the operand
fragments their waves hold for the MFMAs (csrc/gemm_f32_mfma.h compute_dma): the wave columns of a row group share the four
fragment groups of a K tile, every lane half holds four of a group's eight k rows, and the partials meet once after the K loop.

  K    32 one tile (the steady loop never runs) | 64, 160 an even and an odd tile count through the two-tile trip | 164 a K tail
  M    64 exactly one row tile | 132 a fast launch whose last row block is four live rows at BM 128 and at BM 64: the M guard
       of the reduction after the K loop | 130 not a multiple of 4: the launch is not fast, tile 11 with the sums in a pass
       of their own
  N    136: two columns of workgroups at every tile width, only one of them may add
  tile 11 / 12 / 21 / 22 / 28 forced (28 runs 22 where K is not whole tiles), plans (store | accumulate) x (no slices | 3 slices)

Row k of A carries the scale 1 + k % 7, so a dropped or doubled k row, fragment group or lane half moves a sum by a multiple
of a whole row's magnitude.  colsum_a starts non-zero, alpha = 0.5.  The bound and its measure are those of the epilogue-forms
file (rel: largest difference over the reference's largest magnitude; OUT_TOL), imported, not restated.

Bitwise: in deterministic mode two launches of a tile form give equal C and colsum_a, and C does not depend on whether
colsum_a is asked for."""
import ctypes
import functools

import pytest
import torch

import gemm_epilogue_forms_table as T
from gemm_epilogue_forms_table import TN
from test_gpu_gemm_epilogue_forms import OUT_TOL, rel

pytestmark = pytest.mark.gpu

N = 136
ALPHA = 0.5
KS = (32, 64, 160, 164)
MS = (64, 130, 132)
PLANS = ((False, 0), (True, 0), (False, 3), (True, 3))  # (accumulate, forced K slices)


def ops_mod():
    from bayeslms_amd import ops
    return ops


def lib_mod():
    from bayeslms_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _override_off():
    yield
    lib_mod().lib().blm_gemm_plan_override(0, 0)


@functools.lru_cache(maxsize=None)
def problem(M, K):
    """A[K, M] with a different scale on every k row, B[K, N], C0, the start of colsum_a, and the float64 results"""
    g = torch.Generator().manual_seed(7919 * M + K)
    scale = (1 + torch.arange(K) % 7).float().unsqueeze(1)
    A = scale * torch.randn(K, M, generator=g)
    B = torch.randn(K, N, generator=g) * K ** -0.5
    C0 = torch.randn(M, N, generator=g)
    v0 = torch.randn(M, generator=g)
    return {"A": A, "B": B, "C0": C0, "v0": v0, "prod": ALPHA * (A.double().t() @ B.double()),
            "sums": v0.double() + ALPHA * A.double().sum(0)}


def launch(A, B, C, M, K, tile, splits, acc, colsum):
    """force (tile, splits), assert the tile the host will run, launch, take the override off again"""
    ops, L = ops_mod(), lib_mod()
    a = T.plan_args(T.Launch(TN, M, N, K, L.EPI_NONE, N, acc, False, tile, splits))
    out = L.GemmPlan()
    L.check(L.lib().blm_gemm_plan_override(tile, splits), "override")
    try:
        L.check(L.lib().blm_gemm_plan_query(ctypes.byref(a), ctypes.byref(out)), "query")
        assert out.tile == T.tile_run(TN, M, N, K, tile), (M, K, tile, out.tile)
        ops.gemm(TN, A, B, C, M, N, K, M, N, N, alpha=ALPHA, accumulate=acc, colsum_a=colsum)
    finally:
        L.check(L.lib().blm_gemm_plan_override(0, 0), "override")
    return out.tile


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("tile", T.TILES)
def test_colsum_a_against_float64(dev, tile, M, K):
    p = problem(M, K)
    A, B = p["A"].to(dev), p["B"].to(dev)
    bad = []
    for acc, splits in PLANS:
        C = p["C0"].to(dev).clone()
        db = p["v0"].to(dev).clone()
        ran = launch(A, B, C, M, K, tile, splits, acc, db)
        rc = rel(C, p["prod"] + (p["C0"].double() if acc else 0))
        rs = rel(db, p["sums"])
        tag = "tile=%d->%d M=%d K=%d %s splits%d" % (tile, ran, M, K, "acc" if acc else "store", splits)
        print("rel %s C %.3e colsum %.3e" % (tag, rc, rs))
        if not rc < OUT_TOL:
            bad.append("%s C %.3e" % (tag, rc))
        if not rs < OUT_TOL:
            bad.append("%s colsum %.3e" % (tag, rs))
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("tile", T.TILES)
def test_bitwise_repeatable_and_c_independent_of_the_sums(dev, tile):
    """deterministic mode, every K of the table at M = 64 (the LDS-DMA kernels): launch twice with colsum_a, once without"""
    ops = ops_mod()
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        for K in KS:
            p = problem(64, K)
            A, B = p["A"].to(dev), p["B"].to(dev)
            got = []
            for _ in range(2):
                C = p["C0"].to(dev).clone()
                db = p["v0"].to(dev).clone()
                launch(A, B, C, 64, K, tile, 0, True, db)
                got.append((C, db))
            Cn = p["C0"].to(dev).clone()
            launch(A, B, Cn, 64, K, tile, 0, True, None)
            assert torch.equal(got[0][0], got[1][0]), "C differs between two launches, tile %d K %d" % (tile, K)
            assert torch.equal(got[0][1], got[1][1]), "colsum_a differs between two launches, tile %d K %d" % (tile, K)
            assert torch.equal(got[0][0], Cn), "C depends on colsum_a, tile %d K %d" % (tile, K)
            assert rel(got[0][1], p["sums"]) < OUT_TOL
    finally:
        ops.set_deterministic(was)
