"""The launch table shared by tests/test_gpu_gemm_epilogue_forms.py (which runs every launch on the GPU against float64) and
tests/test_gemm_epilogue_forms_cpu.py (which asks the host's planner, without a GPU, for the tile of every launch).

Every operand of these launches is 16-byte aligned with a leading dimension equal to its contiguous extent, so whether a
launch is "fast" (LDS-DMA or register loaders) or takes the guarded loaders depends on the shape alone (blm_gemm, plan_key):
the contiguous extents of A and B must be multiples of 4 -- K and K for NT, K and N for NN, M and N for TN.

  (M, N, K)        | NT            | NN            | TN
  -----------------+---------------+---------------+---------------
  (200, 136,  96)  | fast, 28 ok   | fast, 28 ok   | fast, 28 ok
  (200, 136, 100)  | fast, 28->22  | fast, 28->22  | fast, 28->22
  (200, 136,  98)  | guarded -> 11 | guarded -> 11 | fast, 28->22
  (200, 134,  96)  | fast, 28 ok   | guarded -> 11 | guarded -> 11
  (200, 134, 100)  | fast, 28->22  | guarded -> 11 | guarded -> 11
  (200, 134,  98)  | guarded -> 11 | guarded -> 11 | guarded -> 11
  (128, 128,  64)  | fast, 28 ok   | fast, 28 ok   | fast, 28 ok

`tile_run` below is that table as arithmetic; FAST_TABLE is the same table written out, and the CPU test holds the two and
blm_gemm_plan_query against one another."""
from collections import namedtuple

from bayeslms_amd import _lib as L

NT, NN, TN = L.GEMM_NT, L.GEMM_NN, L.GEMM_TN
OP_NAME = {NT: "NT", NN: "NN", TN: "TN"}
TILES = (11, 12, 21, 22, 28)
SHAPES = [(200, N, K) for N in (136, 134) for K in (96, 100, 98)] + [(128, 128, 64)]

# (M, N, K) -> which of NT, NN, TN are fast; written out by hand from the rule in the docstring
FAST_TABLE = {
    (200, 136, 96): (True, True, True),
    (200, 136, 100): (True, True, True),
    (200, 136, 98): (False, False, True),
    (200, 134, 96): (True, False, False),
    (200, 134, 100): (True, False, False),
    (200, 134, 98): (False, False, False),
    (128, 128, 64): (True, True, True),
}


def is_fast(op, M, N, K):
    ac, bc = (M if op == TN else K), (K if op == NT else N)
    return ac % 4 == 0 and bc % 4 == 0 and ac >= 4 and bc >= 4


def tile_run(op, M, N, K, forced):
    """the tile blm_gemm_plan_query answers under blm_gemm_plan_override(forced, *): 11 for a launch that is not fast, 22 for
    the eight-wave tile on a K that is not whole K tiles, else the forced one"""
    if not is_fast(op, M, N, K):
        return 11
    if forced == 28 and K % 32 != 0:
        return 22
    return forced


def bodies(N):
    return ("rows", "register-quad") if N % 4 == 0 else ("register-scalar",)


def ldc_of(N, body):
    """rows: everything aligned; register-quad: rows that start on 8-byte boundaries only; register-scalar: N % 4 != 0"""
    return N + {"rows": 4, "register-quad": 2, "register-scalar": 3}[body]


def drop_b(M):
    """M = rows x drop_B: 40 x 5, and 32 x 4 for the shape with nothing partial"""
    return 5 if M % 5 == 0 else 4


Launch = namedtuple("Launch", "op M N K epi ldc acc samp forced splits")

# ------------------------------------------------------------------ the parameter lists of the GPU tests
ACT_MAIN = [(tile, M, N, K, body) for tile in TILES for (M, N, K) in SHAPES for body in bodies(N)]
# the two layouts production does not use for an epilogue, tile 22 only: (forward op, backward op)
ACT_OTHER = [(22, fwd, bwd, M, N, K, body) for fwd, bwd in ((NN, NT), (TN, TN))
             for (M, N, K) in ((200, 136, 100), (200, 134, 100)) for body in bodies(N)]
ACT_ACC = [(tile, M, N, K, body) for tile in (11, 28) for (M, N, K) in ((200, 136, 96), (200, 136, 100), (200, 134, 96))
           for body in bodies(N)]
WGRAD = [(tile, 200, N, K, eps) for tile in TILES for N in (136, 134) for K in (96, 100) for eps in ("injected", "philox")]
WGRAD_PLANS = ((False, 0), (True, 0), (True, 3), (True, -2))  # (accumulate, forced splits)
VARB = [(tile, op, 200, 136, K, eps) for tile in TILES for op, K in ((NT, 96), (NT, 100), (NN, 96), (NN, 100), (NN, 98))
        for eps in ("injected", "philox")]
COLSUM = [(tile, 200, N, K) for tile in TILES for N, K in ((136, 96), (136, 100), (134, 96))]
COLSUM_PLANS = ((False, 0), (True, 0), (True, 3), (True, -2), (False, 3))


def all_launches():
    """every blm_gemm launch of the GPU file, as the planner sees it"""
    out = []

    def pair(tile, fwd, bwd, M, N, K, body, acc):
        ld = ldc_of(N, body)
        for epi_f, epi_b in ((L.EPI_BIAS_GELU, L.EPI_MUL_DGELU), (L.EPI_GP_MIX, L.EPI_MUL_DGP_MIX)):
            out.append(Launch(fwd, M, N, K, epi_f, ld, acc, False, tile, 0))
            out.append(Launch(bwd, M, N, K, epi_b, ld, acc, False, tile, 0))
    for tile, M, N, K, body in ACT_MAIN:
        pair(tile, NT, NN, M, N, K, body, False)
    for tile, fwd, bwd, M, N, K, body in ACT_OTHER:
        pair(tile, fwd, bwd, M, N, K, body, False)
    for tile, M, N, K, body in ACT_ACC:
        pair(tile, NT, NN, M, N, K, body, True)
    for tile, M, N, K, _ in WGRAD:
        for acc, splits in WGRAD_PLANS:
            out.append(Launch(TN, M, N, K, L.EPI_BAYES_WGRAD, N + 4, acc, False, tile, splits))
    for tile, op, M, N, K, _ in VARB:
        out.append(Launch(op, M, N, K, L.EPI_NONE, N + 4, False, True, tile, 0))
        if op == NN:
            for body in bodies(N):
                out.append(Launch(op, M, N, K, L.EPI_MUL_DGELU, ldc_of(N, body), False, True, tile, 0))
    for tile, M, N, K in COLSUM:
        for acc, splits in COLSUM_PLANS:
            out.append(Launch(TN, M, N, K, L.EPI_NONE, N, acc, False, tile, splits))
    return out


LAUNCH_SET = frozenset(all_launches())


def plan_args(l, base=1 << 20):
    """blm_gemm_args of a launch for blm_gemm_plan_query: the pointers are only inspected for alignment"""
    a = L.GemmArgs()
    a.abi_version = L.ABI_VERSION
    a.op, a.M, a.N, a.K = l.op, l.M, l.N, l.K
    a.A, a.B, a.C = base, base, base
    a.lda = l.M if l.op == TN else l.K
    a.ldb = l.K if l.op == NT else l.N
    a.ldc = l.ldc
    a.alpha = 1.0
    a.epilogue = l.epi
    a.flags = L.GEMM_ACCUMULATE if l.acc else 0
    if l.samp:
        a.var_b.lgstd = base
    return a
