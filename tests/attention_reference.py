"""Float64 reference of the causal attention core (model.py:889-920), the input families that drive the attention kernels out
of their easy regime, the case table of tests/test_gpu_attention_forms.py and the bounds of that suite.  Plain torch on the CPU:
tests/test_attention_reference_cpu.py pins this file to the oracle and checks the conditioning of every case of the table.

What is compared is always ``max|got - ref| / max|ref|`` against ``reference(..., dtype=float64)``, per tensor (out, lse, dq, dk,
dv; never concatenated) and per 32-row block of the first dimension (query rows of out / dq, key rows of dk / dv), each block
against its own maximum.  The bound of a tensor or block is ``base * max(1, e32 / U)``, the factor capped at ``CAP``:

  base  1e-5 for out and lse, 2e-5 for the gradients (test_attention_matches_oracle's bounds)
  e32   the same figure for ``reference(..., dtype=float32)`` -- a plain float32 evaluation -- on that tensor or block
  U     the largest e32 of the ``ordinary`` family over every shape of the table, whole tensors and blocks (``unit()``)

so a structured family, whose scores of 40 are rounded to 4e-6 before they are exponentiated, gets the room that any float32
evaluation needs and no more; the factor comes from the reference alone.  CAP is a condition on the inputs, not a tolerance.
dq of the families with a large key feature has a second, additive term (``recompute_allowance``, with its derivation);
`ordinary` and `peaked` do not, and no bound exceeds CAP * base."""
import functools
import math

import torch

FAMILIES = ("ordinary", "peaked", "rising", "falling", "shifted")
FEATURE0 = ("rising", "falling", "shifted")  # feature 0 of q and k carries the structure
OUT_TOL, GRAD_TOL, CAP = 1e-5, 2e-5, 16.0
BLOCK = 32


# ------------------------------------------------------------------------------------------------------------ the reference
def reference(q, k, v, go, nhead, keep=None, dtype=torch.float64):
    """q, k, v, go (T, B, nhead * hd) -> out (T, B, d), lse (B * nhead, T), dq, dk, dv, all in ``dtype``: causal attention with
    scale hd ** -0.5 on q, head index b * nhead + head, ``keep`` (B * nhead, T, T) multiplying the probabilities (the dropout
    factors, 0 or 1 / (1 - p)); the gradients are those of sum(out * go)."""
    T, B, d = q.shape
    hd = d // nhead
    qr, kr, vr = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    qh = (qr * (float(hd) ** -0.5)).contiguous().view(T, B * nhead, hd).transpose(0, 1)
    kh = kr.contiguous().view(T, B * nhead, hd).transpose(0, 1)
    vh = vr.contiguous().view(T, B * nhead, hd).transpose(0, 1)
    s = torch.bmm(qh, kh.transpose(1, 2))
    future = torch.ones(T, T, dtype=torch.bool).triu(1)
    s = s.masked_fill(future, float("-inf"))
    lse = torch.logsumexp(s, -1)
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep.to(dtype)
    out = torch.bmm(p, vh).transpose(0, 1).contiguous().view(T, B, d)
    out.backward(go.to(dtype))
    return out.detach(), lse.detach(), qr.grad, kr.grad, vr.grad


NAMES = ("out", "lse", "dq", "dk", "dv")


# ------------------------------------------------------------------------------------------------------------ input families
def make_case(family, T, B, nhead, hd, seed):
    """float32 q, k, v, go (T, B, nhead * hd).  ``ordinary``: all randn.  ``peaked``: q and k times sqrt(6), scores about
    6 N(0,1).  ``rising`` / ``falling``: feature 0 of every head is q = sqrt(hd) and k[t] = +-32 t / max(T - 1, 1), so the score
    carries +-32 t / (T - 1) along the keys.  ``shifted``: feature 0 is q = sqrt(hd) and k = 24, every score carries +24.  The
    largest |score| stays at about 45: beyond that float32 itself loses the digits and the test would be one of conditioning."""
    assert family in FAMILIES, family
    g = torch.Generator().manual_seed(int(seed))
    d = nhead * hd
    q, k, v, go = (torch.randn(T, B, d, generator=g) for _ in range(4))
    if family == "peaked":
        q, k = q * math.sqrt(6.0), k * math.sqrt(6.0)
    elif family != "ordinary":
        q[..., 0::hd] = math.sqrt(hd)
        if family == "shifted":
            k[..., 0::hd] = 24.0
        else:
            ramp = 32.0 * torch.arange(T, dtype=torch.float32) / max(T - 1, 1)
            k[..., 0::hd] = (ramp if family == "rising" else -ramp).view(T, 1, 1)
    return q, k, v, go


def seed_of(family, T, B, nhead, hd):
    """The draw is part of a case's conditioning: the last block of T = 97, 129, 257 or 385 is ONE row, its dk is one dS scalar
    times q, and where dP - delta of that scalar happens to cancel, float32 keeps 20 to 40 U of the block and not 10 U (seen in
    half of eight offsets tried here, each time in one or two of the table's blocks).  This offset leaves every block below
    12 U; test_every_case_of_the_table_is_conditioned_within_the_cap holds the draws to the cap."""
    return 47514 + 100003 * FAMILIES.index(family) + 1009 * T + 101 * hd + 7 * B + nhead


# ------------------------------------------------------------------------------------------------------------ the figures
def figures(got, ref, floor=0.0):
    """[whole, block 0, block 1, ...] of max|got - ref| / max|ref| over ``BLOCK``-row blocks of dimension 0 (``blocked`` tensors;
    an lse gives [whole]).  A reference block that is exactly zero (dq and dk at T = 1) has no scale of its own: ``floor``, the
    largest gradient entry of the case, stands in for it."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)

    def one(a, b):
        m = float(b.abs().max())
        return float((a - b).abs().max()) / (m if m > 0.0 else (floor if floor > 0.0 else 1e-30))
    out = [one(got, ref)]
    if ref.dim() == 3:
        out += [one(got[i:i + BLOCK], ref[i:i + BLOCK]) for i in range(0, ref.shape[0], BLOCK)]
    return out


def bounds(e32, base, unit, extra=None):
    """base * max(1, e32 / U) with the factor capped at CAP, plus ``extra`` (recompute_allowance, dq alone); never above CAP * base"""
    extra = extra or [0.0] * len(e32)
    return [min(CAP * base, base * min(CAP, max(1.0, e / unit)) + x) for e, x in zip(e32, extra)]


def recompute_allowance(inputs, nhead, ref_dq, keep=None):
    """What a backward that RECOMPUTES the scores may add to dq beyond a self-consistent float32 evaluation; [whole, blocks...].

    Every backward form reads delta = rowsum(dO * O) from the forward's output and recomputes p~_j = exp(s~_j - lse) from scores
    of its own.  Its dS~_j = p~_j (keep_j dP_j - delta) then sums to sum_j p_j theta_j (keep_j dP_j - delta) over a row, theta_j
    being the difference between the two float32 evaluations of score j, and no longer to zero as the exact dS does (softmax
    is shift invariant) and as torch's float32 softmax backward does by construction -- so e32 does not see it.  Two float32
    evaluations of a dot product agree only to the rounding of its partial sums (the order of the terms, fused or separate
    multiply-add: vector-ALU, matrix-core, forward and backward kernels are free to differ), about |s| 2^-23 where |s| is 24 to 45.
    To first order  |d dq_if| <= scale * sum_j |dS_ij| theta_ij |k_jf|, which a key feature that is large and equal along the
    keys (feature 0 of `shifted`, `rising`, `falling`: 24 to 32 where dq itself nearly cancels) multiplies by that size.
    theta_ij is taken as twice (two evaluations) the error of the float32 evaluation of score ij on the CPU against float64:
    like e32 it comes from the reference alone.  Only the feature-0 families take the term (Case.extra): there it is 1e-5 to
    6e-4 (the bound stops at CAP * base = 3.2e-4), where the kernels were measured at up to 2.8e-5 (attn_bwd_kernel<8>,
    `shifted`, T 128, rows 96: against 2.26e-5 without the term; a float32 torch emulation of such a backward on
    the CPU gives 2.8e-5 on that case too, and 1.9e-6 once its delta is made self-consistent)."""
    q, k, v, go = inputs
    T, B, d = q.shape
    hd = d // nhead
    scale = float(hd) ** -0.5
    future = torch.ones(T, T, dtype=torch.bool).triu(1)

    def heads(t, dtype):
        return t.to(dtype).view(T, B * nhead, hd).transpose(0, 1)
    s32 = torch.bmm(heads(q, torch.float32) * scale, heads(k, torch.float32).transpose(1, 2)).double()
    s64 = torch.bmm(heads(q, torch.float64) * scale, heads(k, torch.float64).transpose(1, 2))
    theta = 2.0 * (s32 - s64).abs().masked_fill(future, 0.0)
    p = torch.softmax(s64.masked_fill(future, float("-inf")), -1)
    dp = torch.bmm(heads(go, torch.float64), heads(v, torch.float64).transpose(1, 2))
    if keep is not None:
        dp = dp * keep.double()
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    a = (torch.bmm(ds.abs() * theta, heads(k, torch.float64).abs()) * scale).transpose(0, 1).reshape(T, B, d)
    whole = float(ref_dq.abs().max()) or 1e-30
    out = [float(a.max()) / whole]
    for i in range(0, T, BLOCK):
        m = float(ref_dq[i:i + BLOCK].abs().max())
        out.append(float(a[i:i + BLOCK].max()) / (m if m > 0.0 else whole))
    return out


class Case:
    """One evaluated case: ``ref`` (float64) and ``e32`` (the float32 evaluation's figures) per tensor; rows ``lo:`` of the
    query-side tensors are what a decode call computes."""

    def __init__(self, family, T, B, nhead, hd, keep=None, lo=None):
        self.key = (family, T, B, nhead, hd)
        self.inputs = make_case(family, T, B, nhead, hd, seed_of(family, T, B, nhead, hd))
        r64 = reference(*self.inputs, nhead, keep, torch.float64)
        r32 = reference(*self.inputs, nhead, keep, torch.float32)
        self.ref = dict(zip(NAMES, r64))
        self.floor = max(float(self.ref[n].abs().max()) for n in ("dq", "dk", "dv"))
        self.e32 = {n: figures(b, a, self.floor) for n, a, b in zip(NAMES, r64, r32)}
        # the families with a large key feature alone: `ordinary` and `peaked` keep the plain bounds
        self.extra = {"dq": recompute_allowance(self.inputs, nhead, self.ref["dq"], keep)} if family in FEATURE0 else {}
        if lo is not None:  # the rows a decode call computes: the last T - lo queries
            self.ref["out_tail"] = self.ref["out"][lo:]
            self.e32["out_tail"] = figures(r32[0][lo:], r64[0][lo:])

    def multiplier(self):
        return max(max(v) for v in self.e32.values())  # divided by unit() by the caller


@functools.lru_cache(maxsize=None)
def case(family, T, B, nhead, hd):
    """the reference of a case without dropout, computed once for all forms that share it"""
    return Case(family, T, B, nhead, hd)


# ------------------------------------------------------------------------------------------------------------ the case table
SHORT_T, MID_T, LONG_T = (1, 31, 32), (33, 64, 97, 127, 128), (129, 160, 257, 385)
ALL_T = SHORT_T + MID_T
TREE_R = (97, 129, 257)
DECODE_PAST, DECODE_TQ = (0, 63, 64, 65, 200), (1, 7)

# key -> (hd, Ts, (B, nhead), options, workspace offered to the backward); the kernels of each key are in the docstring
# table of tests/test_gpu_attention_forms.py, which test_the_table_is_the_dispatch holds against the host's rules
FORMS = {
    "mfma1":           (64, MID_T, (2, 2), {"attn_hpw": 1}, True),
    "mfma2":           (64, MID_T, (2, 2), {"attn_hpw": 2}, True),
    "mfma1_nows":      (64, MID_T, (2, 2), {"attn_hpw": 1}, False),
    "mfma2_nows":      (64, MID_T, (2, 2), {"attn_hpw": 2}, False),
    "odd_hpw2":        (64, MID_T, (3, 1), {"attn_hpw": 2}, True),
    "short":           (64, SHORT_T, (2, 2), {}, True),
    "short_hpw2":      (64, SHORT_T, (2, 2), {"attn_hpw": 2}, True),
    "short_nows":      (64, SHORT_T, (2, 2), {}, False),
    "short_hpw2_nows": (64, SHORT_T, (2, 2), {"attn_hpw": 2}, False),
    "short_off":       (64, SHORT_T, (2, 2), {"attn_short": 0}, True),
    "long":            (64, LONG_T, (2, 2), {}, True),
    "valu4":           (4, ALL_T, (2, 2), {}, True),
    "valu8":           (8, ALL_T, (2, 2), {}, True),
    "valu16":          (16, ALL_T, (2, 2), {}, True),
    "valu32":          (32, ALL_T, (2, 2), {}, True),
    "valu64":          (64, ALL_T, (2, 2), {"attn_valu": 1}, True),
    "wide128":         (128, ALL_T, (2, 2), {}, True),
    "wide100":         (100, ALL_T, (2, 2), {}, True),
    "wide65":          (65, ALL_T, (2, 2), {}, True),
    "generic100":      (100, (129,), (2, 2), {}, True),
    "generic130":      (130, (40,), (2, 2), {}, True),
    "generic64":       (64, (160,), (2, 2), {"attn_valu": 1}, True),
}
KEEP_FORMS = {  # blm_attn_fwd_keep / blm_attn_bwd_keep: always the vector-ALU kernels
    "keep64":         (64, (97, 128)),
    "keep64_generic": (64, (160,)),
    "keep100":        (100, (97, 128)),
    "keep100_generic": (100, (129,)),
}
DROP_FORMS = {  # the Philox stream through ops.attention: key -> (hd, Ts, options, workspace)
    "drop_mfma1":      (64, (32, 97, 128, 160), {"attn_hpw": 1}, True),
    "drop_mfma2":      (64, (97, 128), {"attn_hpw": 2}, True),
    "drop_mfma1_nows": (64, (97, 128), {"attn_hpw": 1}, False),
    "drop_mfma2_nows": (64, (97, 128), {"attn_hpw": 2}, False),
    "drop_valu32":     (32, (32, 97, 128, 160), {}, True),
    "drop_wide100":    (100, (32, 97, 128, 160), {}, True),
}
DROP_P = 0.3
DROP_KEY = (4321, 9, 3)  # seed, site, step of the Philox dropout stream


def family_ts(Ts):
    """{family: Ts}: ordinary and rising at every T of a form; the others at its smallest, its largest and one T % 4 != 0."""
    odd = [t for t in Ts if t % 4]
    few = sorted({min(Ts), max(Ts)} | set(odd[-1:]))
    return {f: (tuple(Ts) if f in ("ordinary", "rising") else tuple(few)) for f in FAMILIES}


def pair_cases():
    """(key, family, T) of every forward + backward case without dropout"""
    return [(key, f, T) for key, spec in FORMS.items() for f, ts in family_ts(spec[1]).items() for T in ts]


def keep_cases():
    return [(key, f, T) for key, (hd, Ts) in KEEP_FORMS.items() for f in ("ordinary", "rising") for T in Ts]


def rows_cases():
    """(family, T, ragged): identity rowmap at every short T, the ragged one where a column can be shorter"""
    return [(f, T, rg) for f, ts in family_ts(SHORT_T).items() for T in ts for rg in (False, True) if not (rg and T == 1)]


def tree_cases():
    return [(hd, f, R) for hd in (64, 32) for f, rs in family_ts(TREE_R).items() for R in rs]


def decode_cases():
    pasts = family_ts(DECODE_PAST)  # ordinary and rising at every past length; the others at 0, 200 and 65
    return [(hd, f, past, Tq) for hd in (64, 100) for f in FAMILIES for past in pasts[f] for Tq in DECODE_TQ]


def drop_cases():
    return [(key, f, T, win) for key, spec in DROP_FORMS.items() for f in ("ordinary", "rising") for T in spec[1] for win in (False, True)]


ALIGN_CASES = [(T, hpw, p, f) for T in (128, 64) for hpw in (1, 2) for p in (0.0, DROP_P) for f in ("ordinary", "rising")]


def table_shapes():
    """every (family, T, B, nhead, hd) without dropout that the GPU suite evaluates"""
    out = set()
    for key, f, T in pair_cases():
        hd, _, (B, nhead) = FORMS[key][:3]
        out.add((f, T, B, nhead, hd))
    for f, T, _ in rows_cases():
        out.add((f, T, 2, 2, 64))
    for hd, f, R in tree_cases():
        out.add((f, R, 1, 2, hd))
    for hd, f, past, Tq in decode_cases():
        out.add((f, past + Tq, 2, 2, hd))
    for T, _, p, f in ALIGN_CASES:
        out.add((f, T, 2, 2, 64))
    return sorted(out)


@functools.lru_cache(maxsize=None)
def unit():
    """U: the largest float32-evaluation figure of the ``ordinary`` family over every shape of the table, tensors and blocks"""
    return max(case(*s).multiplier() for s in table_shapes() if s[0] == "ordinary")


# ------------------------------------------------------------------------------------------------------------ dropout masks
@functools.lru_cache(maxsize=None)
def philox_keep(G, nhead, T):
    """(G * nhead, T, T) factors 0 or 1 / (1 - p) of the Philox dropout stream DROP_KEY drawn for G global batch columns"""
    from oracle import philox as P
    seed, site, step = DROP_KEY
    m = P.keep_mask(G * nhead * T * T, DROP_P, seed, P.STREAM_DROPOUT + site, step)
    return torch.from_numpy(m).view(G * nhead, T, T).float() / (1 - DROP_P)


@functools.lru_cache(maxsize=None)
def torch_keep(G, nhead, T):
    """the same factors as torch's CPU dropout draws them (NoiseState.source "torch")"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(G * 1000 + T)
        return torch.dropout(torch.ones(G * nhead, T, T), DROP_P, True)


@functools.lru_cache(maxsize=None)
def decode_case(family, past, Tq, B, nhead, hd):
    """``Tq`` new tokens after ``past`` cached ones: the family lies along the cache position, the queries are its last Tq rows"""
    return Case(family, past + Tq, B, nhead, hd, lo=past)


@functools.lru_cache(maxsize=None)
def drop_case(family, T, B, nhead, hd, window, source="philox"):
    """a case under dropout p = DROP_P: the rank holds columns [off, off + B) of G global ones -> (Case, whole mask, off, G)"""
    G, off = (B + 2, 1) if window else (B, 0)
    mask = (philox_keep if source == "philox" else torch_keep)(G, nhead, T)
    return Case(family, T, B, nhead, hd, keep=mask[off * nhead:(off + B) * nhead]), mask, off, G


# ------------------------------------------------------------------------------------------------------------ the host's rules
def _hpw(heads, opt):
    v = opt.get("attn_hpw", 0)
    return v if v in (1, 2) else (2 if heads // 2 >= 256 else 1)


def ws_floats(T, B, nhead, hd, opt):
    """blm_attn_bwd_ws_floats by the host's rule: the T <= 128 matrix-core backward alone has a use for a workspace"""
    use_mfma = hd == 64 and not opt.get("attn_valu", 0)
    n = B * nhead * T * T
    return n if (T > 0 and B > 0 and nhead > 0 and use_mfma and T <= 128 and n < (1 << 30)) else 0


def _valu(T, hd, what):
    tiled_ok = T <= 128 and hd <= 128
    own_kernel = hd in (4, 8, 16, 32, 64)
    if not tiled_ok:
        return "attn_fwd_generic_kernel" if what == "fwd" else "attn_bwd_dq_generic_kernel + attn_bwd_dkv_generic_kernel"
    if not own_kernel:
        return "attn_%s_wide_kernel<%s>" % (what, "true" if hd == 128 else "false")
    return "attn_%s_kernel<%d>" % (what, hd)


def fwd_kernel(T, B, nhead, hd, opt, keep=False):
    """the forward kernel blm_attn_fwd (blm_attn_fwd_keep: ``keep``) launches, by the host's rules"""
    use_mfma = hd == 64 and not opt.get("attn_valu", 0) and not keep
    if not use_mfma:
        return _valu(T, hd, "fwd")
    if T > 128:
        return "attn_fwd_long_kernel"
    if T <= 32 and opt.get("attn_short", 1):
        return "attn_fwd_short_kernel"
    heads = B * nhead
    return "attn_fwd_mfma_kernel<%d>" % (2 if heads % 2 == 0 and _hpw(heads, opt) == 2 else 1)


def bwd_kernel(T, B, nhead, hd, opt, ws, keep=False):
    """the backward kernels blm_attn_bwd_ws launches with (``ws``) or without a workspace pointer"""
    use_mfma = hd == 64 and not opt.get("attn_valu", 0) and not keep
    if not use_mfma:
        return _valu(T, hd, "bwd")
    if T > 128:
        return "attn_bwd_dq_long_kernel + attn_bwd_dkv_long_kernel"
    heads = B * nhead
    n = 2 if heads % 2 == 0 and _hpw(heads, opt) == 2 else 1
    if ws and ws_floats(T, B, nhead, hd, opt) > 0:
        return "attn_bwd_dkv_mfma_kernel<%d,true>" % n
    return "attn_bwd_dq_mfma_kernel<%d> + attn_bwd_dkv_mfma_kernel<%d>" % (n, n)
