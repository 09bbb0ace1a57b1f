"""GPU: the epilogues of the fp32 MFMA GEMM (csrc/gemm_f32_mfma.h) and the dropout fused into them, in EVERY form the host
can instantiate, against float64 torch on the same values with the Philox oracle's mask (oracle/philox.py keep_mask) and
normals (normal).  Kernel level, through ops.gemm, with the tile forced by blm_gemm_plan_override and the tile the host will
run asserted through blm_gemm_plan_query; then the three feed-forward ops with dropout on against float64 autograd.

Which loader, epilogue body and keep / eps form a launch reaches is READ FROM THE CODE (launch_op, launch_cfg, gemm_f32_kernel,
epilogue, epilogue_rows, blm_gemm); only the tile can be queried (tests/test_gemm_epilogue_forms_cpu.py does, without a GPU):

  tile      forced 11 / 12 / 21 / 22 / 28; a launch that is not fast runs 11 (guarded loaders), tile 28 on K % 32 != 0 runs 22.
            With var_b the planner still answers 28, launch_op has no eight-wave form with fused sampling and runs 22: nothing
            to assert through the API, the result is compared all the same.
  loader    fast and no var_b: LDS-DMA; var_b: register loaders (SAMP); not fast: guarded, tile 11 only.  "Fast" per
            (layout, shape) is the table of tests/gemm_epilogue_forms_table.py.
  body      "rows" (epilogue_rows, 16-byte rows through LDS): C, aux, bias, C2 aligned, N % 4 == 0, ldc % 4 == 0, no atomics --
            here ldc = N + 4.  Otherwise the register walk (epilogue): "register-quad" ldc = N + 2 (aux has C's ld),
            "register-scalar" N = 134, ldc = N + 3.  BAYES_WGRAD always walks the registers.
  keep      rows -> keep4 (one Philox block per lane); register-quad -> gemm_keep_quad (blocks exchanged inside a quad by
            DPP); register-scalar -> gemm_keep.  gemm_keep_pair sits behind INTERLEAVE = false and is dead.
  eps       BAYES_WGRAD: injected; Philox at N % 4 == 0 -> gemm_eps_quad; Philox at N = 134 -> scalar (and guarded).

  test                                   | layouts        | tiles      | loader              | body        | keep / eps
  ---------------------------------------+----------------+------------+---------------------+-------------+----------------------
  bias_gelu_and_mul_dgelu (ACT_MAIN)     | NT then NN     | all five   | DMA; guarded at     | rows, quad  | keep4, gemm_keep_quad
    and gp_mix_and_mul_dgp_mix           |                |            | K = 98 / NN N = 134 | scalar      | gemm_keep
  ..._on_the_other_layouts (ACT_OTHER)   | NN/NT, TN/TN   | 22         | DMA; guarded N=134  | all three   | all three
  ..._accumulate_and_alpha (ACT_ACC)     | NT then NN     | 11, 28     | DMA; guarded NN 134 | all three   | all three
  bayes_wgrad (WGRAD)                    | TN             | all five   | DMA; guarded N=134  | register    | injected, eps_quad,
                                         |                |            |                     |             | scalar; slices 3, -2
  var_b (VARB)                           | NT, NN         | all five   | register (SAMP);    | rows, quad  | injected / Philox eps
                                         |                | (28 -> 22) | guarded NN K = 98   |             | in the loader
  colsum_a (COLSUM)                      | TN             | all five   | DMA; N = 134 guarded| rows / reg. | slices 3, -2
                                         |                |            | (blm_colsum route)  | (atomics)   |
  ffn / ffn_gp / ffn_lrt                 | all            | own + five | all three           | rows; 134:  | keep4; gemm_keep;
                                         |                |            |                     | scalar      | injected eps

Shapes (the smallest with whole and partial tiles at every tile size): M = 200 = 40 rows x drop_B 5 = 128 + 72 = 3 x 64 + 8, so
both passes of the WTM = 2 row body run and the second is partly filled; N = 136 = a whole 128-column tile and a tile of two
quads; N = 134 the scalar keep form; K = 96 whole K tiles (tile 28 eligible), 100 a K tail, 98 the NT guarded loaders;
(128, 128, 64) nothing partial.  Weights carry K ** -0.5, so pre-activations stay within about +-4: ordinary magnitudes.

Bounds, relative to the reference's largest magnitude: 1e-5 for C and aux, 2e-5 for the products with a derivative factor
(test_gemm_epilogues, tests/test_gpu_operand_layouts.py) -- the same two bounds where eps is the device's Philox normal and the
reference's is the numpy one (oracle/philox.py normal): C2 of BAYES_WGRAD 2e-5, C of var_b 1e-5 (2e-5 with MUL_DGELU).  With dropout on and accumulate off the mask must match EXACTLY: the zero
pattern of C (BIAS_GELU, GP_MIX), of BIAS_GELU's aux and of MUL_DGP_MIX's C2 is the dropped set, after the precondition that
no kept element of the float64 reference is zero.  The padding columns of C, aux and C2 hold a sentinel and must come back
bit-identical.  GEMM_EPI_FORMS_REL_OUT=<file> writes the worst rel per (epilogue, tile, body, output) of the session
(profiles/gemm_epilogue_forms_rel.txt)."""
import ctypes
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

import gemm_epilogue_forms_table as T
from gemm_epilogue_forms_table import NT, NN, TN

pytestmark = pytest.mark.gpu

from oracle import bayes_oracle as O  # noqa: E402
from oracle import philox as P  # noqa: E402

OUT_TOL, DER_TOL = 1e-5, 2e-5
SENT = -777.25
P_DROP, SEED, SITE, STEP = 0.3, 1234, 5, 7
WINDOWS = {"full": (0, 0), "window": (2, 9)}  # (col_offset, global_cols); 0 = drop_B
ACTS = ("tanh", "sigmoid", "relu", "gelu")
WORST = {}  # (epilogue, tile, body, output) -> largest rel seen in this session


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
def _override_off_and_rel_table():
    """the plan override is off again when the module is done, whatever happened; the rel table is written then"""
    yield
    lib_mod().lib().blm_gemm_plan_override(0, 0)
    path = os.environ.get("GEMM_EPI_FORMS_REL_OUT")
    if path and WORST:
        with open(path, "w") as f:
            f.write("# epilogue  tile  body  output  worst_rel\n")
            for (epi, tile, body, name), v in sorted(WORST.items(), key=str):
                f.write("%-28s %-4s %-16s %-10s %.3e\n" % (epi, tile, body, name, v))


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


class Checks:
    """figures are printed and recorded first, asserted together at the end of a test"""

    def __init__(self, epi, tile, body, detail=""):
        self.key, self.detail, self.bad = (epi, str(tile), body), detail, []

    def close(self, name, got, want, tol):
        r = rel(got, want)
        k = self.key + (name,)
        WORST[k] = max(WORST.get(k, 0.0), r)
        print("rel %s tile=%s %s [%s] %s %.3e" % (self.key + (self.detail, name, r)))
        if not r < tol:
            self.bad.append("%s [%s] %s %.3e >= %.0e" % (self.key[0], self.detail, name, r, tol))

    def true(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        assert not self.bad, "; ".join(self.bad)


# ------------------------------------------------------------------ references (float64, CPU, computed once per shape)
def gelu_d(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-z * z / 2) / math.sqrt(2 * math.pi)


def gp_d(z, coef):
    s = torch.sigmoid(z)
    return coef[0] * (1 - torch.tanh(z) ** 2) + coef[1] * s * (1 - s) + coef[2] * (z > 0).double() + coef[3] * gelu_d(z)


@functools.lru_cache(maxsize=None)
def problem(op, M, N, K):
    """operands of one product C[M, N] in the layout of ``op`` (B carries K ** -0.5) and the float64 product"""
    g = torch.Generator().manual_seed(100003 * op + 1009 * M + 31 * N + K)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if op == NT:
        A, B = rn(M, K), rn(N, K) * K ** -0.5
        prod = A.double() @ B.double().t()
    elif op == NN:
        A, B = rn(M, K), rn(K, N) * K ** -0.5
        prod = A.double() @ B.double()
    else:
        A, B = rn(K, M), rn(K, N) * K ** -0.5
        prod = A.double().t() @ B.double()
    bias = rn(N) * 0.5
    coef = (torch.rand(4, N, generator=g) + 0.25) * torch.where(torch.rand(4, N, generator=g) < 0.5, -1.0, 1.0)
    return {"A": A, "B": B, "prod": prod, "bias": bias, "coef": coef, "C0": rn(M, N)}


@functools.lru_cache(maxsize=None)
def keep_mask(M, N, mode):
    """bool (M, N): the kept elements of a (rows, drop_B, N) activation, columns [off, off + B) of G global ones"""
    if mode == "off":
        return torch.ones(M, N, dtype=torch.bool)
    B = T.drop_b(M)
    off, G = WINDOWS[mode]
    G = G or B
    rows = M // B
    m = P.keep_mask(rows * G * N, P_DROP, SEED, P.STREAM_DROPOUT + SITE, STEP).reshape(rows, G, N)[:, off:off + B]
    return torch.from_numpy(m.copy()).reshape(M, N)


def keep_factor(M, N, mode):
    return keep_mask(M, N, mode).double() / ((1 - P_DROP) if mode != "off" else 1.0)


def drop_of(mode):
    ops = ops_mod()
    if mode == "off":
        return ops.NO_DROP
    off, G = WINDOWS[mode]
    return ops.Drop(P_DROP, SEED, SITE, STEP, off, G)


# ------------------------------------------------------------------ launches
def padded(dev, rows, cols, ld, values=None):
    """-> (storage (rows, ld) filled with the sentinel, its (rows, cols) view holding ``values``)"""
    st = torch.full((rows, ld), SENT, device=dev)
    v = st[:, :cols]
    if values is not None:
        v.copy_(values)
    assert st.data_ptr() % 16 == 0
    return st, v


def padding_intact(st, cols):
    return bool((st[:, cols:] == SENT).all())


def launch(op, A, B, Cv, M, N, K, ldc, tile, splits=0, **kw):
    """force (tile, splits), assert the tile the host will run, launch, and take the override off again"""
    ops, L = ops_mod(), lib_mod()
    l = T.Launch(op, M, N, K, kw.get("epilogue", L.EPI_NONE), ldc, bool(kw.get("accumulate")), kw.get("var_b") is not None, tile, splits)
    assert l in T.LAUNCH_SET, l  # the CPU test walks the same launches
    a = T.plan_args(l)
    a.A, a.B, a.C = A.data_ptr(), B.data_ptr(), Cv.data_ptr()
    assert (a.lda, a.ldb) == (A.stride(0), B.stride(0))
    if l.samp:
        a.var_b = kw["var_b"]
    out = L.GemmPlan()
    L.check(L.lib().blm_gemm_plan_override(tile, splits), "override")
    try:
        L.check(L.lib().blm_gemm_plan_query(ctypes.byref(a), ctypes.byref(out)), "query")
        assert out.tile == T.tile_run(op, M, N, K, tile) and out.source == 2, (l, out.tile)
        ops.gemm(op, A, B, Cv, M, N, K, A.stride(0), B.stride(0), ldc, **kw)
    finally:
        L.check(L.lib().blm_gemm_plan_override(0, 0), "override")
    return out.tile


def _act_pair(dev, kind, tile, fwd, bwd, M, N, K, body, mode, acc=False, alpha=1.0):
    """forward epilogue (BIAS_GELU or GP_MIX, aux written) in layout ``fwd``, then the backward epilogue (MUL_DGELU or
    MUL_DGP_MIX with C2 given and without) in layout ``bwd`` reading that aux, with the same Drop and drop_B"""
    L = lib_mod()
    gp = kind == "gp"
    ld = T.ldc_of(N, body)
    pf, pb = problem(fwd, M, N, K), problem(bwd, M, N, K)
    keep, kf = keep_mask(M, N, mode), keep_factor(M, N, mode)
    drop, B = drop_of(mode), T.drop_b(M)
    z = alpha * pf["prod"] + pf["bias"].double()
    coef = pf["coef"].double()
    act = O.gp_mixture(z, coef, ACTS) if gp else F.gelu(z)
    dact = gp_d(z, coef) if gp else gelu_d(z)
    C0 = pf["C0"].double() if acc else 0.0
    epi_f, epi_b = (L.EPI_GP_MIX, L.EPI_MUL_DGP_MIX) if gp else (L.EPI_BIAS_GELU, L.EPI_MUL_DGELU)
    name_f, name_b = ("GP_MIX", "MUL_DGP_MIX") if gp else ("BIAS_GELU", "MUL_DGELU")
    tag = "drop-" + mode + (" acc" if acc else "")
    to = lambda t: t.to(dev)  # noqa: E731

    # ---- forward
    Cst, Cv = padded(dev, M, N, ld, pf["C0"] if acc else None)
    Xst, Xv = padded(dev, M, N, ld)
    ran = launch(fwd, to(pf["A"]), to(pf["B"]), Cv, M, N, K, ld, tile, alpha=alpha, accumulate=acc, epilogue=epi_f,
                 bias=to(pf["bias"]), aux=Xv, coef=to(pf["coef"]) if gp else None, drop=drop, drop_B=B)
    ck = Checks("%s %s" % (T.OP_NAME[fwd], name_f), ran, body, tag)
    ck.close("C", Cv, act * kf + C0, OUT_TOL)
    ck.close("aux", Xv, z if gp else dact * kf, OUT_TOL)
    ck.true(padding_intact(Cst, N) and padding_intact(Xst, N), "forward wrote the padding columns")
    if mode != "off":
        assert bool((act[keep] != 0).all()) and (gp or bool((dact[keep] != 0).all()))  # precondition on the reference
        if not acc:
            ck.true(torch.equal(Cv.cpu() == 0, ~keep), "%s: zero pattern of C is not the dropped set" % name_f)
        if not gp:
            ck.true(torch.equal(Xv.cpu() == 0, ~keep), "BIAS_GELU: zero pattern of aux is not the dropped set")
    ck.done()

    # ---- backward: reads the aux the forward left
    gprod = alpha * pb["prod"]
    for with_c2 in ((True, False) if gp else (False,)):
        Dst, Dv = padded(dev, M, N, ld, pb["C0"] if acc else None)
        C2st, C2v = padded(dev, M, N, ld) if with_c2 else (None, None)
        kw = dict(coef=to(pf["coef"]), C2=C2v, drop=drop, drop_B=B) if gp else {}
        ran = launch(bwd, to(pb["A"]), to(pb["B"]), Dv, M, N, K, ld, tile, alpha=alpha, accumulate=acc, epilogue=epi_b, aux=Xv, **kw)
        ck = Checks("%s %s" % (T.OP_NAME[bwd], name_b), ran, body, tag)
        D0 = pb["C0"].double() if acc else 0.0
        ck.close("C", Dv, gprod * kf * dact + D0, DER_TOL)
        ck.true(padding_intact(Dst, N) and padding_intact(Xst, N), "backward wrote the padding columns")
        if with_c2:
            ck.close("C2", C2v, gprod * kf, OUT_TOL)  # written, never accumulated
            ck.true(padding_intact(C2st, N), "backward wrote the padding columns of C2")
            if mode != "off":
                assert bool((gprod[keep] != 0).all())
                ck.true(torch.equal(C2v.cpu() == 0, ~keep), "MUL_DGP_MIX: zero pattern of C2 is not the mask of the forward")
        ck.done()


@pytest.mark.parametrize("tile,M,N,K,body", T.ACT_MAIN)
def test_bias_gelu_and_mul_dgelu(dev, tile, M, N, K, body):
    for mode in ("off", "full", "window"):
        _act_pair(dev, "gelu", tile, NT, NN, M, N, K, body, mode)


@pytest.mark.parametrize("tile,M,N,K,body", T.ACT_MAIN)
def test_gp_mix_and_mul_dgp_mix(dev, tile, M, N, K, body):
    """all four coefficient rows non-zero; C2 and C of the NN backward carry the mask the NT forward drew"""
    for mode in ("off", "full", "window"):
        _act_pair(dev, "gp", tile, NT, NN, M, N, K, body, mode)


@pytest.mark.parametrize("kind", ["gelu", "gp"])
@pytest.mark.parametrize("tile,fwd,bwd,M,N,K,body", T.ACT_OTHER)
def test_activation_epilogues_on_the_other_layouts(dev, kind, tile, fwd, bwd, M, N, K, body):
    """each of the four on the two layouts production does not launch it with"""
    for mode in ("off", "window"):
        _act_pair(dev, kind, tile, fwd, bwd, M, N, K, body, mode)


@pytest.mark.parametrize("kind", ["gelu", "gp"])
@pytest.mark.parametrize("tile,M,N,K,body", T.ACT_ACC)
def test_activation_epilogues_accumulate_and_alpha(dev, kind, tile, M, N, K, body):
    """accumulate onto random C with alpha = 0.75: alpha scales the product before the bias, aux and C2 are still written"""
    for mode in ("off", "full"):
        _act_pair(dev, kind, tile, NT, NN, M, N, K, body, mode, acc=True, alpha=0.75)


# ------------------------------------------------------------------ BAYES_WGRAD
def _eps(dev, rows, cols, kind, tid):
    """-> (float64 reference eps, NoiseSpec)"""
    ops = ops_mod()
    if kind == "injected":
        e = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols + tid))
        return e.double(), ops.NoiseSpec(eps=e.to(dev))
    e = torch.from_numpy(P.normal(rows * cols, SEED, P.STREAM_WEIGHT + tid, STEP)).view(rows, cols)
    return e.double(), ops.NoiseSpec(None, SEED, tid, STEP)


@pytest.mark.parametrize("tile,M,N,K,eps_kind", T.WGRAD)
def test_bayes_wgrad(dev, tile, M, N, K, eps_kind):
    """include/bayeslm.h: dW = alpha acc; C (+)= dW + kl_lambda mu / n_kl on the noisy rows; C2[r] (+)= dW eps exp(lgstd) +
    kl_lambda (exp(2 lgstd) - 1) / n_kl.  Full and partial row window, accumulate off and on, and on with forced slices 3
    and -2: the KL terms are added once."""
    ops, L = ops_mod(), lib_mod()
    p = problem(TN, M, N, K)
    g = torch.Generator().manual_seed(M + N + K)
    mu = torch.randn(M, N, generator=g) * 0.3
    lam, inv_n, alpha, ld = 0.37, 1.0 / 777.0, 0.75, N + 4
    form = "injected" if eps_kind == "injected" else ("eps_quad" if N % 4 == 0 else "scalar")
    for row_lo, srows in ((0, M), (8, M - 24)):
        lg = torch.rand(srows, N, generator=g) - 3.0
        e64, noise = _eps(dev, srows, N, eps_kind, 11)
        dW = alpha * p["prod"]
        sig = torch.exp(lg.double())
        want_c = dW.clone()
        want_c[row_lo:row_lo + srows] += lam * inv_n * mu.double()[row_lo:row_lo + srows]
        want_c2 = dW[row_lo:row_lo + srows] * e64 * sig + lam * inv_n * (sig * sig - 1)
        must, mv = padded(dev, M, N, ld, mu)
        lgd = lg.to(dev)
        for acc, splits in T.WGRAD_PLANS:
            C0, C20 = p["C0"], torch.randn(srows, N, generator=torch.Generator().manual_seed(5))
            Cst, Cv = padded(dev, M, N, ld, C0 if acc else None)
            C2 = C20.to(dev) if acc else torch.full((srows, N), SENT, device=dev)
            ran = launch(TN, p["A"].to(dev), p["B"].to(dev), Cv, M, N, K, ld, tile, splits, alpha=alpha, accumulate=acc,
                         epilogue=L.EPI_BAYES_WGRAD, C2=C2, wg_mu=mv, var_c=ops._variational(lgd, noise, row_lo, srows),
                         kl_lambda=lam, kl_inv_n=inv_n)
            ck = Checks("TN BAYES_WGRAD " + form, ran, "register", "window%d%s%s" % (row_lo, " acc" if acc else "", " splits%d" % splits if splits else ""))
            ck.close("C", Cv, want_c + (C0.double() if acc else 0), OUT_TOL)
            ck.close("C2", C2, want_c2 + (C20.double() if acc else 0), DER_TOL)
            ck.true(padding_intact(Cst, N) and padding_intact(must, N), "wrote the padding columns")
            ck.done()


# ------------------------------------------------------------------ var_b: W = mu + exp(lgstd) eps formed in the tile loader
@pytest.mark.parametrize("tile,op,M,N,K,eps_kind", T.VARB)
def test_var_b(dev, tile, op, M, N, K, eps_kind):
    """fused sampling of B (register loaders; NN at K = 98 the guarded ones): plain on NT and NN, and NN with MUL_DGELU as
    _FFN.backward launches it, in both bodies; full row window and row_lo = 8, srows = wrows - 24"""
    ops, L = ops_mod(), lib_mod()
    p = problem(op, M, N, K)
    wrows, wcols = (N, K) if op == NT else (K, N)
    g = torch.Generator().manual_seed(M + N + K + op)
    for row_lo, srows in ((0, wrows), (8, wrows - 24)):
        lg = torch.rand(srows, wcols, generator=g) - 3.0
        e64, noise = _eps(dev, srows, wcols, eps_kind, 12)
        W = p["B"].double().clone()
        W[row_lo:row_lo + srows] += torch.exp(lg.double()) * e64
        prod = p["A"].double() @ (W.t() if op == NT else W)
        lgd = lg.to(dev)
        A, B = p["A"].to(dev), p["B"].to(dev)
        tag = "%s window%d" % (eps_kind, row_lo)
        Cst, Cv = padded(dev, M, N, N + 4)
        ran = launch(op, A, B, Cv, M, N, K, N + 4, tile, var_b=ops._variational(lgd, noise, row_lo, srows))
        ck = Checks("%s var_b %s NONE" % (T.OP_NAME[op], eps_kind), ran, "rows", tag)
        ck.close("C", Cv, prod, OUT_TOL)
        ck.true(padding_intact(Cst, N), "wrote the padding columns")
        ck.done()
        if op == NN:
            aux64 = gelu_d(problem(NT, M, N, K)["prod"]) * keep_factor(M, N, "full")
            for body in T.bodies(N):
                ld = T.ldc_of(N, body)
                Xst, Xv = padded(dev, M, N, ld, aux64.float())
                Cst, Cv = padded(dev, M, N, ld)
                ran = launch(op, A, B, Cv, M, N, K, ld, tile, epilogue=L.EPI_MUL_DGELU, aux=Xv,
                             var_b=ops._variational(lgd, noise, row_lo, srows))
                ck = Checks("NN var_b %s MUL_DGELU" % eps_kind, ran, body, tag)
                ck.close("C", Cv, prod * aux64.float().double(), DER_TOL)
                ck.true(padding_intact(Cst, N) and padding_intact(Xst, N), "wrote the padding columns")
                ck.done()


# ------------------------------------------------------------------ colsum_a: the bias gradient out of the wgrad product
@pytest.mark.parametrize("tile,M,N,K", T.COLSUM)
def test_colsum_a(dev, tile, M, N, K):
    """colsum_a[m] += alpha * sum_k A[k, m] onto a non-zero vector, M no multiple of any tile; with forced K slices the sums
    are added once, not per slice.  N = 134 is not fast: blm_gemm takes the sums in a pass of their own."""
    p = problem(TN, M, N, K)
    alpha = 0.5
    A, B = p["A"].to(dev), p["B"].to(dev)
    v0 = torch.randn(M, generator=torch.Generator().manual_seed(K))
    for acc, splits in T.COLSUM_PLANS:
        C = p["C0"].to(dev).clone()
        db = v0.to(dev).clone()
        ran = launch(TN, A, B, C, M, N, K, N, tile, splits, alpha=alpha, accumulate=acc, colsum_a=db)
        body = "register" if splits or N % 4 else "rows"  # K slices meet through atomics: the register walk
        ck = Checks("TN NONE colsum_a", ran, body, "%s%s" % ("acc" if acc else "store", " splits%d" % splits if splits else ""))
        ck.close("C", C, alpha * p["prod"] + (p["C0"].double() if acc else 0), OUT_TOL)
        ck.close("colsum", db, v0.double() + alpha * p["A"].double().sum(0), OUT_TOL)
        ck.done()


# ------------------------------------------------------------------ the feed-forward ops with dropout, against float64 autograd
FFN_SHAPES = [(40, 5, 72, 136), (40, 5, 66, 134)]
FFN_TILES = (0, 11, 12, 21, 22, 28)  # 0: the planner's own


@functools.lru_cache(maxsize=None)
def ffn_inputs(kind, T_, B, D, Fd):
    g = torch.Generator().manual_seed(7 * D + Fd + len(kind))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = {"x": rn(T_, B, D), "w1": rn(Fd, D) * D ** -0.5, "b1": rn(Fd) * 0.5, "go": rn(T_, B, D)}
    if kind == "gp":
        t["coef"] = (torch.rand(4, Fd, generator=g) + 0.25) * torch.where(torch.rand(4, Fd, generator=g) < 0.5, -1.0, 1.0)
    t["w2"] = rn(D, Fd) * Fd ** -0.5
    if kind in ("plain", "gp"):
        t["b2"] = rn(D) * 0.5
    else:
        t["lgstd2"] = torch.rand(D, Fd, generator=g) - 3.0
        t["eps"] = rn(T_ * B, D) if kind == "lrt" else rn(D, Fd)
    return t


def ffn_reference(kind, t, mode, lam):
    """float64 autograd: (y, {name: grad}) for the upstream gradient t["go"]"""
    T_, B, D = t["x"].shape
    Fd = t["w1"].shape[0]
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in t.items() if k not in ("go", "eps")}
    z = leaves["x"] @ leaves["w1"].t() + leaves["b1"]
    h = O.gp_mixture(z, leaves["coef"], ACTS) if kind == "gp" else F.gelu(z)
    h = h * keep_factor(T_ * B, Fd, mode).view(T_, B, Fd)
    if kind in ("plain", "gp"):
        y = h @ leaves["w2"].t() + leaves["b2"]
        loss = (y * t["go"].double()).sum()
    else:
        mu, lg = leaves["w2"], leaves["lgstd2"]
        if kind == "lrt":
            y = h @ mu.t() + torch.sqrt((h * h) @ torch.exp(2 * lg).t()) * t["eps"].double().view(T_, B, D)
        else:
            y = h @ (mu + torch.exp(lg) * t["eps"].double()).t()
        loss = (y * t["go"].double()).sum() + lam * O.kl_mean_form(mu, lg)
    loss.backward()
    return y.detach(), {k: v.grad for k, v in leaves.items()}


def ffn_run(dev, kind, t, mode, lam, fused):
    ops = ops_mod()
    a = {k: v.to(dev).requires_grad_(True) for k, v in t.items() if k not in ("go", "eps")}
    drop = drop_of(mode)
    if kind == "plain":
        y = ops.ffn(a["x"], a["w1"], a["b1"], a["w2"], a["b2"], drop=drop)
    elif kind == "gp":
        y = ops.ffn_gp(a["x"], a["w1"], a["b1"], a["coef"], a["w2"], a["b2"], drop=drop)
    elif kind == "lrt":
        y = ops.ffn_lrt(a["x"], a["w1"], a["b1"], a["w2"], a["lgstd2"], ops.LrtNoise(eps=t["eps"].to(dev)), kl_lambda=lam, drop=drop)
    else:
        y = ops.ffn(a["x"], a["w1"], a["b1"], a["w2"], None, a["lgstd2"], ops.NoiseSpec(eps=t["eps"].to(dev)), lam, fused, drop)
    y.backward(t["go"].to(dev))
    torch.cuda.synchronize()
    return y.detach(), {k: v.grad for k, v in a.items()}


FFN_KINDS = [("plain", 0.0, False), ("bayes", 0.0, False), ("bayes", 0.37, False), ("bayes", 0.0, True), ("bayes", 0.37, True),
             ("gp", 0.0, False), ("lrt", 0.0, False), ("lrt", 0.37, False)]


# fused sampling reads float4s of the weight: ops.ffn(fused=True) at F = 134 is refused (below), not run
FFN_PARAMS = [(shape + kind + (tile,)) for shape in FFN_SHAPES for kind in FFN_KINDS for tile in FFN_TILES
              if not (kind[2] and shape[3] % 4)]


def test_ffn_fused_sampling_of_an_odd_width_is_refused(dev):
    t = ffn_inputs("bayes", 40, 5, 66, 134)
    with pytest.raises(lib_mod().BayesLMError):
        ffn_run(dev, "bayes", t, "full", 0.0, True)


@pytest.mark.parametrize("T_,B,D,Fd,kind,lam,fused,tile", FFN_PARAMS)
def test_ffn_ops_with_dropout(dev, T_, B, D, Fd, kind, lam, fused, tile):
    """ops.ffn (plain; Bayesian second linear with injected eps, materialised and fused, with and without the KL term),
    ops.ffn_gp and ops.ffn_lrt with Drop(0.3), with and without a column window: the output and every gradient.
    (40, 5, 66, 134) is guarded and scalar throughout."""
    L = lib_mod()
    t = ffn_inputs(kind, T_, B, D, Fd)
    for mode in ("full", "window"):
        L.check(L.lib().blm_gemm_plan_override(tile, 0), "override")
        try:
            y, grads = ffn_run(dev, kind, t, mode, lam, fused)
        finally:
            L.check(L.lib().blm_gemm_plan_override(0, 0), "override")
        want_y, want = ffn_reference(kind, t, mode, lam)
        name = "ffn_%s%s%s" % (kind, " fused" if fused else "", " kl" if lam else "")
        ck = Checks(name, tile or "own", "F%d" % Fd, "drop-" + mode)
        ck.close("y", y, want_y, OUT_TOL)
        assert set(grads) == set(want)
        for k in sorted(want):
            ck.true(grads[k] is not None, "no gradient reached " + k)
            if grads[k] is not None:
                ck.close("d" + k, grads[k], want[k], DER_TOL)
        ck.done()
