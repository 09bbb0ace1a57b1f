"""GPU: causal attention (csrc/attention_mfma.hip, csrc/attention.hip, blm_attn_decode of csrc/decode.hip) in EVERY kernel form the
host can pick, on five input families, against the float64 reference of tests/attention_reference.py (pinned to the oracle by
tests/test_attention_reference_cpu.py).  The host picks a form from T, head_dim, B * nhead, the options "attn_hpw" / "attn_short" /
"attn_valu", the workspace pointer and the kind of dropout mask (`test_the_table_is_the_dispatch` recomputes both kernel columns
with the host's rules and holds blm_attn_bwd_ws_floats, the one selection a caller can observe, to them):

  key             | hd  | T        | B,nhead | options      | ws  | forward kernel           | backward kernels
  ----------------+-----+----------+---------+--------------+-----+--------------------------+---------------------------------
  mfma1           | 64  | 33..128  | 2,2     | attn_hpw=1   | yes | attn_fwd_mfma_kernel<1>  | attn_bwd_dkv_mfma_kernel<1,true>
  mfma2           | 64  | 33..128  | 2,2     | attn_hpw=2   | yes | attn_fwd_mfma_kernel<2>  | attn_bwd_dkv_mfma_kernel<2,true>
  mfma1_nows      | 64  | 33..128  | 2,2     | attn_hpw=1   | no  | attn_fwd_mfma_kernel<1>  | attn_bwd_dq_mfma_kernel<1> + attn_bwd_dkv_mfma_kernel<1>
  mfma2_nows      | 64  | 33..128  | 2,2     | attn_hpw=2   | no  | attn_fwd_mfma_kernel<2>  | attn_bwd_dq_mfma_kernel<2> + attn_bwd_dkv_mfma_kernel<2>
  odd_hpw2        | 64  | 33..128  | 3,1     | attn_hpw=2   | yes | attn_fwd_mfma_kernel<1>  | attn_bwd_dkv_mfma_kernel<1,true>
  short           | 64  | 1..32    | 2,2     |              | yes | attn_fwd_short_kernel    | attn_bwd_dkv_mfma_kernel<1,true>
  short_hpw2      | 64  | 1..32    | 2,2     | attn_hpw=2   | yes | attn_fwd_short_kernel    | attn_bwd_dkv_mfma_kernel<2,true>
  short_nows      | 64  | 1..32    | 2,2     |              | no  | attn_fwd_short_kernel    | attn_bwd_dq_mfma_kernel<1> + attn_bwd_dkv_mfma_kernel<1>
  short_hpw2_nows | 64  | 1..32    | 2,2     | attn_hpw=2   | no  | attn_fwd_short_kernel    | attn_bwd_dq_mfma_kernel<2> + attn_bwd_dkv_mfma_kernel<2>
  short_off       | 64  | 1..32    | 2,2     | attn_short=0 | yes | attn_fwd_mfma_kernel<1>  | attn_bwd_dkv_mfma_kernel<1,true>
  long            | 64  | 129..385 | 2,2     |              | yes | attn_fwd_long_kernel     | attn_bwd_dq_long_kernel + attn_bwd_dkv_long_kernel
  valu4           | 4   | 1..128   | 2,2     |              | yes | attn_fwd_kernel<4>       | attn_bwd_kernel<4>
  valu8           | 8   | 1..128   | 2,2     |              | yes | attn_fwd_kernel<8>       | attn_bwd_kernel<8>
  valu16          | 16  | 1..128   | 2,2     |              | yes | attn_fwd_kernel<16>      | attn_bwd_kernel<16>
  valu32          | 32  | 1..128   | 2,2     |              | yes | attn_fwd_kernel<32>      | attn_bwd_kernel<32>
  valu64          | 64  | 1..128   | 2,2     | attn_valu=1  | yes | attn_fwd_kernel<64>      | attn_bwd_kernel<64>
  wide128         | 128 | 1..128   | 2,2     |              | yes | attn_fwd_wide_kernel<true>  | attn_bwd_wide_kernel<true>
  wide100         | 100 | 1..128   | 2,2     |              | yes | attn_fwd_wide_kernel<false> | attn_bwd_wide_kernel<false>
  wide65          | 65  | 1..128   | 2,2     |              | yes | attn_fwd_wide_kernel<false> | attn_bwd_wide_kernel<false>
  generic100      | 100 | 129      | 2,2     |              | yes | attn_fwd_generic_kernel  | attn_bwd_dq_generic_kernel + attn_bwd_dkv_generic_kernel
  generic130      | 130 | 40       | 2,2     |              | yes | attn_fwd_generic_kernel  | attn_bwd_dq_generic_kernel + attn_bwd_dkv_generic_kernel
  generic64       | 64  | 160      | 2,2     | attn_valu=1  | yes | attn_fwd_generic_kernel  | attn_bwd_dq_generic_kernel + attn_bwd_dkv_generic_kernel

("ws yes": the workspace pointer is offered; only the T <= 128 matrix-core backward takes it.)  Beside the table:

  keep64 / keep100, *_generic   blm_attn_fwd_keep + blm_attn_bwd_keep, the mask torch's dropout drew (p 0.3) for a column window:
                                the tiled vector-ALU kernels at T 97, 128 and the one-wave-per-query ones at T 160 / 129
  rows                          blm_attn_fwd_rows: attn_fwd_short_kernel through a rowmap, identity and ragged (shuffled rows)
  tree64 / tree32               blm_attn_fwd_tree on a chain trie lo = 0, end = R (the causal mask), R = 97, 129, 257:
                                attn_fwd_tree_kernel (hd 64) and attn_fwd_tree_generic_kernel (hd 32)
  decode64 / decode100          blm_attn_decode (split-K part + combine kernels): past 0, 63, 64, 65, 200, Tq 1 and 7; the family
                                lies along the cache position
  drop_*                        the Philox dropout stream (p 0.3) through ops.attention on the packed projection: both matrix-core
                                forms with and without workspace, short (T 32) and long (T 160), attn_*_kernel<32>, the wide form at
                                hd 100 and the generic ones (T 160) -- each with col_offset 0 and as the window col_offset 1 of B + 2
                                global columns, whose reference takes heads [nhead, (1 + B) nhead) of the mask drawn for B + 2
  ws_offset                     blm_attn_bwd_ws with the workspace one float past a 16-byte boundary: the scalar path of the
                                one-launch backward, equal to the aligned call and within the float64 bounds

Forward and backward of a key run in one test: the forms with a workspace go through ops.attention_qkv (out, gradients) and take lse
from blm_attn_fwd itself, whose out must equal the op's bit for bit; the forms without one call blm_attn_fwd / blm_attn_bwd_ws (NULL).
The backward always reads the out and lse its own forward produced.

Shapes: B = nhead = 2 (B = 3, nhead = 1 where an odd head count matters).  T in {1, 31, 32} / {33, 64, 97, 127, 128} / {129, 160, 257,
385}: a single row, partial tiles, every tile border, T % 4 != 0, one key past a chunk, a partial second chunk, a chunk border + 1
and three chunks + 1.  `ordinary` and `rising` run at every T of a form, `peaked`, `falling` and `shifted` at its smallest, its
largest and one T % 4 != 0.  That is 399 forward + backward cases, 12 keep, 25 rows, 24 tree, 76 decode, 72 dropout-stream and 16
workspace-alignment cases: 624, each a few milliseconds of GPU time; every float64 reference is computed once per (family, T, B,
nhead, hd) and shared (attention_reference.case).

Figures and bounds (attention_reference): max|got - ref| / max|ref| per tensor -- out, lse, dq, dk, dv, never concatenated -- and per
32-row block of out / dq (query rows) and dk / dv (key rows) against the block's own maximum; bound = base * max(1, e32 / U), the
factor capped at 16, base 1e-5 for out and lse and 2e-5 for gradients, e32 the figure of the plain float32 evaluation of the same
case on the CPU and U the largest e32 on ordinary inputs.  dq of `rising`, `falling` and `shifted` has one more, additive term for what recomputing the scores
in the backward costs where a key feature is large (attention_reference.recompute_allowance derives it; without it
attn_bwd_kernel<8> on `shifted` at T 128 gave 2.83e-5 against 2.26e-5 in rows 96:, the one miss of 624 cases).  Every figure is printed and recorded before anything is asserted;
ATTENTION_FORMS_REL_OUT=<file> writes the record (profiles/attention_forms_rel.txt)."""
import ctypes as C
import os

import pytest
import torch

import attention_reference as A

pytestmark = pytest.mark.gpu

RECORD = {}  # (key, kernel, family, tensor) -> [worst rel, worst block rel, e32 and bound of the worst figure, largest rel / bound]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def option():
    """set(name, value) for the duration of a test; every option goes back to what it was."""
    from bayeslms_amd import ops
    saved = {}

    def setter(name, value):
        saved.setdefault(name, ops.get_option(name))
        ops.set_option(name, value)
    yield setter
    for k, v in saved.items():
        ops.set_option(k, v)


@pytest.fixture(scope="module")
def unit():
    """U: float32's own error on the ordinary family over every shape of the table (CPU, once)"""
    return A.unit()


@pytest.fixture(scope="module", autouse=True)
def _rel_table():
    yield
    path = os.environ.get("ATTENTION_FORMS_REL_OUT")
    if path and RECORD:
        with open(path, "w") as f:
            f.write("# key  kernel  family  tensor  worst_rel  worst_block_rel  e32  bound  worst_rel/bound   (rel = max|got - f64| / max|f64|, whole\n"
                    "# tensor and 32-row block; e32 and bound belong to the largest of the two figures: e32 the float32 evaluation's figure there,\n"
                    "# bound = base * min(16, max(1, e32 / U)) [+ the recomputation allowance of dq], base %.0e out / lse, %.0e gradients; last column:\n"
                    "# the largest figure / bound over every tensor and block of the line's cases)\n" % (A.OUT_TOL, A.GRAD_TOL))
            for (key, kern, fam, name), (w, wb, e, b, r) in sorted(RECORD.items()):
                f.write("%-22s %-78s %-9s %-4s %.3e %.3e %.3e %.3e %.2f\n" % (key, kern.replace(" ", ""), fam, name, w, wb, e, b, r))


def _lib():
    from bayeslms_amd import _lib as L
    L.require_gfx950()
    return L, L.lib()


def _set(option, opts):
    for k, v in opts.items():
        option(k, v)


def _compare(key, kern, family, got, c, unit, names):
    """tensors ``names`` of ``got`` against the case's float64 reference: whole and per block, each under its own bound"""
    bad = []
    for name in names:
        ref, e32 = c.ref[name], c.e32[name]
        base = A.GRAD_TOL if name.startswith("d") else A.OUT_TOL
        assert bool(torch.isfinite(got[name]).all()), name
        figs = A.figures(got[name], ref, c.floor)
        bnds = A.bounds(e32, base, unit, c.extra.get(name))
        worst = max(range(len(figs)), key=lambda i: figs[i])
        rec = RECORD.setdefault((key, kern, family, name.replace("_tail", "")), [0.0, 0.0, 0.0, base, 0.0])
        rec[0], rec[1] = max(rec[0], figs[0]), max(rec[1], max(figs[1:], default=figs[0]))
        if figs[worst] >= max(rec[0], rec[1]) or rec[2] == 0.0:
            rec[2], rec[3] = e32[worst], bnds[worst]
        rec[4] = max(rec[4], max(f / b for f, b in zip(figs, bnds)))
        print("rel %s %s %s T=%d %s whole %.3e (bound %.3e) worst block %.3e" % (key, kern, family, c.key[1], name, figs[0], bnds[0],
                                                                                 max(figs[1:], default=figs[0])))
        for i, (fg, bd) in enumerate(zip(figs, bnds)):
            if not fg < bd:
                bad.append("%s%s %.3e >= %.3e (e32 %.3e)" % (name, "" if i == 0 else "[rows %d:]" % (32 * (i - 1)), fg, bd, e32[i]))
    assert not bad, "%s %s %s: %s" % (key, family, c.key, "; ".join(bad))


def _drop_args(drop):
    """(p, rng or NULL, col_offset, global_cols) of a C call from an ops.Drop or None"""
    if drop is None:
        return 0.0, None, 0, 0
    r = drop.rng()
    return float(drop.p), C.byref(r), int(drop.col_offset), int(drop.global_cols)


def _c_fwd(q, k, v, ld, T, B, nhead, hd, drop=None):
    """blm_attn_fwd -> out (T, B, d), lse (B * nhead, T)"""
    L, lib = _lib()
    out = torch.full((T, B, nhead * hd), 7.5, device=q.device)
    lse = torch.full((B * nhead, T), 7.5, device=q.device)
    p, r, off, G = _drop_args(drop)
    L.check(lib.blm_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), ld, out.data_ptr(), lse.data_ptr(), T, B, nhead, hd, p, r, off,
                             G or B, L.stream()), "blm_attn_fwd")
    return out, lse


def _c_bwd(q, k, v, ld, out, go, lse, T, B, nhead, hd, ws_ptr=None, nws=0, drop=None):
    """blm_attn_bwd_ws with the workspace at ``ws_ptr`` (None: NULL, the two-recomputation forms) -> dq, dk, dv"""
    L, lib = _lib()
    d = nhead * hd
    dq, dk, dv = (torch.full((T, B, d), 7.5, device=q.device) for _ in range(3))
    p, r, off, G = _drop_args(drop)
    L.check(lib.blm_attn_bwd_ws(q.data_ptr(), k.data_ptr(), v.data_ptr(), ld, out.data_ptr(), go.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                dk.data_ptr(), dv.data_ptr(), d, T, B, nhead, hd, p, r, off, G or B, ws_ptr, nws, L.stream()),
            "blm_attn_bwd_ws")
    return dq, dk, dv


# ------------------------------------------------------------------ the table
def _doc_table():
    rows = {}
    for line in __doc__.splitlines():
        cells = [c.strip() for c in line.split("|")]
        if len(cells) == 8 and cells[0] in A.FORMS:
            rows[cells[0]] = cells
    return rows


ALL_KERNELS = {"attn_fwd_mfma_kernel<1>", "attn_fwd_mfma_kernel<2>", "attn_fwd_short_kernel", "attn_fwd_long_kernel",
               "attn_fwd_kernel<4>", "attn_fwd_kernel<8>", "attn_fwd_kernel<16>", "attn_fwd_kernel<32>", "attn_fwd_kernel<64>",
               "attn_fwd_wide_kernel<true>", "attn_fwd_wide_kernel<false>", "attn_fwd_generic_kernel",
               "attn_bwd_dkv_mfma_kernel<1,true>", "attn_bwd_dkv_mfma_kernel<2,true>", "attn_bwd_dq_mfma_kernel<1>",
               "attn_bwd_dkv_mfma_kernel<1>", "attn_bwd_dq_mfma_kernel<2>", "attn_bwd_dkv_mfma_kernel<2>", "attn_bwd_dq_long_kernel",
               "attn_bwd_dkv_long_kernel", "attn_bwd_kernel<4>", "attn_bwd_kernel<8>", "attn_bwd_kernel<16>", "attn_bwd_kernel<32>",
               "attn_bwd_kernel<64>", "attn_bwd_wide_kernel<true>", "attn_bwd_wide_kernel<false>", "attn_bwd_dq_generic_kernel",
               "attn_bwd_dkv_generic_kernel"}


def test_the_table_is_the_dispatch(dev, option):
    """Both kernel columns of the docstring table by the host's rules (attention_reference.fwd_kernel / bwd_kernel: T > 128,
    T <= 32 && attn_short, heads / 2 >= 256 or attn_hpw, own_kernel, tiled_ok, use_mfma, blm_attn_bwd_ws_floats > 0) for every case,
    and blm_attn_bwd_ws_floats itself -- the one selection the library lets a caller observe -- for every backward case."""
    L, lib = _lib()
    doc = _doc_table()
    assert set(doc) == set(A.FORMS)
    seen = set()
    for key, (hd, Ts, (B, nhead), opts, ws) in A.FORMS.items():
        cells = doc[key]
        assert int(cells[1]) == hd and cells[2] == ("%d..%d" % (min(Ts), max(Ts)) if len(Ts) > 1 else str(Ts[0])), key
        assert cells[3] == "%d,%d" % (B, nhead) and cells[4] == ",".join("%s=%d" % kv for kv in opts.items()) and cells[5] == ("yes" if ws else "no"), key
        _set(option, {"attn_hpw": 0, "attn_short": 1, "attn_valu": 0})
        _set(option, opts)
        for T in Ts:
            assert A.fwd_kernel(T, B, nhead, hd, opts) == cells[6], (key, T)
            assert A.bwd_kernel(T, B, nhead, hd, opts, ws) == cells[7], (key, T)
            want = A.ws_floats(T, B, nhead, hd, opts)
            assert int(lib.blm_attn_bwd_ws_floats(T, B, nhead, hd)) == want, (key, T)
            assert want == (B * nhead * T * T if (hd == 64 and T <= 128 and not opts.get("attn_valu")) else 0)
            assert (",true>" in cells[7]) == (ws and want > 0), (key, T)
        seen |= {cells[6]} | set(cells[7].split(" + "))
    assert seen == ALL_KERNELS
    # the default picks two heads per workgroup from 512 heads on, whatever the table forces
    assert A.fwd_kernel(128, 64, 8, 64, {}) == "attn_fwd_mfma_kernel<2>" and A.fwd_kernel(128, 32, 8, 64, {}) == "attn_fwd_mfma_kernel<1>"
    assert A.bwd_kernel(128, 65, 8, 64, {}, True) == "attn_bwd_dkv_mfma_kernel<2,true>" and A.bwd_kernel(128, 65, 7, 64, {}, True).endswith("<1,true>")
    # the dropout-stream and keep cases reach these kernels
    drop = set()
    for key, (hd, Ts, opts, ws) in A.DROP_FORMS.items():
        for T in Ts:
            drop |= {A.fwd_kernel(T, 2, 2, hd, opts)} | set(A.bwd_kernel(T, 2, 2, hd, opts, ws).split(" + "))
    assert drop == {k for k in ALL_KERNELS if "_kernel<4>" not in k and "_kernel<8>" not in k and "_kernel<16>" not in k
                    and "_kernel<64>" not in k and "wide_kernel<true>" not in k}
    keep = set()
    for key, (hd, Ts) in A.KEEP_FORMS.items():
        for T in Ts:
            keep |= {A.fwd_kernel(T, 2, 2, hd, {}, keep=True)} | set(A.bwd_kernel(T, 2, 2, hd, {}, True, keep=True).split(" + "))
    assert keep == {"attn_fwd_kernel<64>", "attn_bwd_kernel<64>", "attn_fwd_wide_kernel<false>", "attn_bwd_wide_kernel<false>",
                    "attn_fwd_generic_kernel", "attn_bwd_dq_generic_kernel", "attn_bwd_dkv_generic_kernel"}


# ------------------------------------------------------------------ forward + backward, no dropout
@pytest.mark.parametrize("key,family,T", A.pair_cases())
def test_attention_in_every_kernel_form(dev, option, unit, key, family, T):
    from bayeslms_amd import ops
    hd, _, (B, nhead), opts, ws = A.FORMS[key]
    _set(option, opts)
    c = A.case(family, T, B, nhead, hd)
    q, k, v, go = (t.to(dev) for t in c.inputs)
    d = nhead * hd
    out, lse = _c_fwd(q, k, v, d, T, B, nhead, hd)
    if ws:  # through the op: it offers the workspace blm_attn_bwd_ws_floats asks for
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        out_op = ops.attention_qkv(*leaves, nhead)
        out_op.backward(go)
        assert torch.equal(out_op.detach(), out)
        dq, dk, dv = (t.grad for t in leaves)
    else:
        dq, dk, dv = _c_bwd(q, k, v, d, out, go, lse, T, B, nhead, hd)
    torch.cuda.synchronize()
    got = {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    fk, bk = A.fwd_kernel(T, B, nhead, hd, opts), A.bwd_kernel(T, B, nhead, hd, opts, ws)
    errors = []
    for kern, names in ((fk, ("out", "lse")), (bk, ("dq", "dk", "dv"))):
        try:
            _compare(key, kern, family, got, c, unit, names)
        except AssertionError as e:  # every figure of the case is printed and recorded before the case fails
            errors.append(str(e))
    assert not errors, "\n".join(errors)
    if (key, family, T) in (("mfma1", "rising", 97), ("long", "rising", 257), ("valu32", "rising", 97)):
        _vacuous_guard(c, got)


def _vacuous_guard(c, got):
    """the comparison can fail: lse without its log-sum term, and a dq that missed the scale, are far outside the bounds"""
    T, B, d = c.inputs[0].shape
    nhead = c.key[3]
    hd = d // nhead
    q, k = (t.double().view(T, B * nhead, hd).transpose(0, 1) for t in c.inputs[:2])
    s = (torch.bmm(q, k.transpose(1, 2)) * hd ** -0.5).masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    assert A.figures(s.max(-1).values, c.ref["lse"])[0] > 100 * A.CAP * A.OUT_TOL
    assert A.figures(got["lse"], s.max(-1).values)[0] > 100 * A.CAP * A.OUT_TOL
    assert A.figures(got["dq"] * hd ** 0.5, c.ref["dq"])[0] > 100 * A.CAP * A.GRAD_TOL


# ------------------------------------------------------------------ the dropout mask handed over
@pytest.mark.parametrize("key,family,T", A.keep_cases())
def test_attention_with_a_keep_mask_in_every_kernel_form(dev, unit, key, family, T):
    L, lib = _lib()
    hd = A.KEEP_FORMS[key][0]
    B, nhead = 2, 2
    d = nhead * hd
    c, mask, off, G = A.drop_case(family, T, B, nhead, hd, True, "torch")
    q, k, v, go = (t.to(dev) for t in c.inputs)
    keep = mask.to(dev)
    out, lse = torch.full((T, B, d), 7.5, device=dev), torch.full((B * nhead, T), 7.5, device=dev)
    dq, dk, dv = (torch.full((T, B, d), 7.5, device=dev) for _ in range(3))
    L.check(lib.blm_attn_fwd_keep(q.data_ptr(), k.data_ptr(), v.data_ptr(), d, out.data_ptr(), lse.data_ptr(), T, B, nhead, hd,
                                  keep.data_ptr(), off, G, L.stream()), "blm_attn_fwd_keep")
    L.check(lib.blm_attn_bwd_keep(q.data_ptr(), k.data_ptr(), v.data_ptr(), d, out.data_ptr(), go.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                  dk.data_ptr(), dv.data_ptr(), d, T, B, nhead, hd, keep.data_ptr(), off, G, L.stream()), "blm_attn_bwd_keep")
    torch.cuda.synchronize()
    got = {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    kern = A.fwd_kernel(T, B, nhead, hd, {}, keep=True) + " / " + A.bwd_kernel(T, B, nhead, hd, {}, True, keep=True)
    _compare(key, kern, family, got, c, unit, A.NAMES)


# ------------------------------------------------------------------ packed rows, tries, the key / value cache
@pytest.mark.parametrize("family,T,ragged", A.rows_cases())
def test_attention_on_packed_rows(dev, unit, family, T, ragged):
    """blm_attn_fwd_rows: the real tokens of a padded (T, B) batch as shuffled packed rows; a column's missing tail keys lie behind
    every real query, where the reference's causal mask has them"""
    L, lib = _lib()
    B, nhead, hd = 2, 2, 64
    d = nhead * hd
    c = A.case(family, T, B, nhead, hd)
    lens = [T, max(1, T - 7)] if ragged else [T, T]
    sel = torch.tensor([t * B + n for n in range(B) for t in range(lens[n])], dtype=torch.int64)
    sel = sel[torch.randperm(sel.numel(), generator=torch.Generator().manual_seed(T))]
    R = sel.numel()
    rowmap = torch.full((T * B,), -1, dtype=torch.int32)
    rowmap[sel] = torch.arange(R, dtype=torch.int32)
    q, k, v = (t.reshape(T * B, d)[sel].contiguous().to(dev) for t in c.inputs[:3])
    out = torch.full((R, d), 7.5, device=dev)
    L.check(lib.blm_attn_fwd_rows(q.data_ptr(), k.data_ptr(), v.data_ptr(), d, out.data_ptr(), rowmap.to(dev).data_ptr(), T, B, nhead, hd,
                                  L.stream()), "blm_attn_fwd_rows")
    torch.cuda.synchronize()
    full = c.ref["out"].clone().reshape(T * B, d)  # the padding positions have no row: they take the reference's value
    full[sel] = out.double().cpu()
    _compare("rows_ragged" if ragged else "rows", "attn_fwd_short_kernel", family, {"out": full.view(T, B, d)}, c, unit, ("out",))


@pytest.mark.parametrize("hd,family,R", A.tree_cases())
def test_tree_attention_on_a_chain(dev, unit, hd, family, R):
    L, lib = _lib()
    nhead = 2
    d = nhead * hd
    c = A.case(family, R, 1, nhead, hd)
    q, k, v = (t.reshape(R, d).to(dev) for t in c.inputs[:3])
    end = torch.full((R,), R, dtype=torch.int32, device=dev)
    lo = torch.zeros(R, dtype=torch.int32, device=dev)
    out = torch.full((R, d), 7.5, device=dev)
    L.check(lib.blm_attn_fwd_tree(q.data_ptr(), k.data_ptr(), v.data_ptr(), d, out.data_ptr(), end.data_ptr(), lo.data_ptr(), R, nhead, hd,
                                  L.stream()), "blm_attn_fwd_tree")
    torch.cuda.synchronize()
    kern = "attn_fwd_tree_kernel" if hd == 64 else "attn_fwd_tree_generic_kernel"
    _compare("tree%d" % hd, kern, family, {"out": out.view(R, 1, d)}, c, unit, ("out",))


@pytest.mark.parametrize("hd,family,past,Tq", A.decode_cases())
def test_attention_over_the_cache(dev, unit, hd, family, past, Tq):
    """blm_attn_decode: Tq new rows of N = 2 streams after ``past`` cached tokens, split over 64-key chunks and combined"""
    L, lib = _lib()
    N, nhead = 2, 2
    d = nhead * hd
    Lk = past + Tq
    c = A.decode_case(family, past, Tq, N, nhead, hd)
    q, k, v, _ = c.inputs
    n_cap, max_len = N + 1, Lk + 5
    kv = torch.full((2, n_cap, nhead, max_len, hd), 7.5)
    kv[0, :N, :, :Lk] = k.view(Lk, N, nhead, hd).permute(1, 2, 0, 3)
    kv[1, :N, :, :Lk] = v.view(Lk, N, nhead, hd).permute(1, 2, 0, 3)
    kv = kv.to(dev)
    qn = q[past:].contiguous().to(dev)
    past_d = torch.full((n_cap,), past, dtype=torch.int32, device=dev)
    out = torch.full((Tq, N, d), 7.5, device=dev)
    nws = int(lib.blm_attn_decode_ws_floats(Tq, N, nhead, Lk, hd))
    ws = torch.empty(max(nws, 1), device=dev)
    L.check(lib.blm_attn_decode(qn.data_ptr(), d, kv.data_ptr(), past_d.data_ptr(), None, out.data_ptr(), ws.data_ptr(), nws, Tq, N, n_cap,
                                nhead, max_len, hd, Lk, L.stream()), "blm_attn_decode")
    torch.cuda.synchronize()
    _compare("decode%d" % hd, "blm_attn_decode", family, {"out_tail": out}, c, unit, ("out_tail",))


# ------------------------------------------------------------------ dropout on the Philox stream
@pytest.mark.parametrize("key,family,T,window", A.drop_cases())
def test_attention_dropout_stream_in_every_kernel_form(dev, option, unit, monkeypatch, key, family, T, window):
    from bayeslms_amd import ops
    hd, _, opts, ws = A.DROP_FORMS[key]
    B, nhead = 2, 2
    d = nhead * hd
    _set(option, opts)
    monkeypatch.setattr(ops, "_ATTN_WS", ws)
    c, _, off, G = A.drop_case(family, T, B, nhead, hd, window)
    seed, site, step = A.DROP_KEY
    drop = ops.Drop(A.DROP_P, seed, site, step, off, G)
    q, k, v, go = c.inputs
    qkv = torch.cat([q, k, v], -1).to(dev).requires_grad_(True)
    out = ops.attention(qkv, nhead, drop)
    out.backward(go.to(dev))
    with torch.no_grad():
        out_c, lse = _c_fwd(qkv, qkv[..., d:], qkv[..., 2 * d:], 3 * d, T, B, nhead, hd, drop)
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), out_c)
    dq, dk, dv = qkv.grad.split(d, -1)
    got = {"out": out.detach(), "lse": lse, "dq": dq, "dk": dk, "dv": dv}
    kern = A.fwd_kernel(T, B, nhead, hd, opts) + " / " + A.bwd_kernel(T, B, nhead, hd, opts, ws)
    _compare(key + ("_window" if window else ""), kern, family, got, c, unit, A.NAMES)
    if window and T > 1:  # the mask of columns [0, B) is another mask: the window is not vacuous
        other = A.drop_case(family, T, B, nhead, hd, False)[0]
        assert A.figures(got["out"], other.ref["out"])[0] > 100 * A.CAP * A.OUT_TOL
        assert A.figures(got["dq"], other.ref["dq"])[0] > 100 * A.CAP * A.GRAD_TOL


# ------------------------------------------------------------------ the workspace off its 16-byte alignment
@pytest.mark.parametrize("T,hpw,p,family", A.ALIGN_CASES)
def test_attention_backward_with_an_unaligned_workspace(dev, option, unit, T, hpw, p, family):
    """blm_attn_bwd_ws with the workspace one float into a buffer one float larger: the scalar dS path of the one-launch backward
    equals the aligned call (rel < 2e-6, the bar of test_attention_backward_workspace_path_equals_recomputation) and meets the
    float64 bounds"""
    from bayeslms_amd import ops
    L, lib = _lib()
    B, nhead, hd = 2, 2, 64
    d = nhead * hd
    option("attn_hpw", hpw)
    if p > 0:
        c = A.drop_case(family, T, B, nhead, hd, False)[0]
        drop = ops.Drop(p, *A.DROP_KEY, 0, B)
    else:
        c, drop = A.case(family, T, B, nhead, hd), None
    q, k, v, go = (t.to(dev) for t in c.inputs)
    out, lse = _c_fwd(q, k, v, d, T, B, nhead, hd, drop)
    nws = int(lib.blm_attn_bwd_ws_floats(T, B, nhead, hd))
    assert nws == B * nhead * T * T
    buf = torch.empty(nws + 1, device=dev)
    assert buf.data_ptr() % 16 == 0
    res = {}
    for name, shift in (("aligned", 0), ("offset", 4)):
        res[name] = _c_bwd(q, k, v, d, out, go, lse, T, B, nhead, hd, buf.data_ptr() + shift, nws, drop)
    torch.cuda.synchronize()
    for name, a, b in zip(("dq", "dk", "dv"), res["offset"], res["aligned"]):
        r = A.figures(a, b)[0]
        print("rel ws_offset against aligned hpw=%d p=%.1f %s T=%d %s %.3e" % (hpw, p, family, T, name, r))
        assert r < 2e-6, name
    kern = A.bwd_kernel(T, B, nhead, hd, {"attn_hpw": hpw}, True)
    for name in ("aligned", "offset"):
        got = dict(zip(("dq", "dk", "dv"), res[name]))
        _compare("ws_" + name + ("_drop" if p > 0 else ""), kern, family, got, c, unit, ("dq", "dk", "dv"))
