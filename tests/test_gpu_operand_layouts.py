"""The public ops on operands of every layout a caller can hand them, against float64 CPU references.

The models only ever produce fresh, contiguous, 16-byte aligned fp32 tensors and leaf parameters, and the other GPU tests
mostly use that layout too.  Here every op of the table is run with each tensor argument (weights included) as a strided
view, as a contiguous view at a 1-3 float storage offset and as float64; with upstream gradients that are narrow views out
of torch.cat (with a live sibling), expanded, transposed or the sum of two consumers; with weights passed as non-leaf
tensors, strided leaves, leaves that already hold a (possibly strided) .grad and weights shared by two calls.  Each result
must match the float64 reference within the bounds of the aligned case, or the op must raise BayesLMError before any
launch -- never a different number.  Forward inputs and sibling gradients must come out bitwise unchanged (the documented
consumption of the logits by ops.cross_entropy aside), and a second backward over a retained graph adds the gradient again
or raises.  The feed-forward ops (ffn, ffn_bayes, ffn_gp, ffn_lrt, dropout on) accumulate some weight gradients straight into
.grad (Case.in_place): for those weights a strided tensor, a non-leaf or a strided .grad must raise BayesLMError before any
launch, and the tests assert that it does.

Every strided or offset operand is a view into a storage at least (offset + numel) floats long, on the GPU; no operand is
host-resident, half-width or expanded (stride 0) in a forward call."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import bayes_oracle as O  # noqa: E402
from oracle import philox as P  # noqa: E402

DEV = torch.device("cuda:0")


def ops_mod():
    from bayeslms_amd import ops
    return ops


def BayesLMError():
    from bayeslms_amd._lib import BayesLMError as E
    return E


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def keep(shape, p, seed, site, step):
    n = 1
    for s in shape:
        n *= s
    return torch.from_numpy(P.keep_mask(n, p, seed, P.STREAM_DROPOUT + site, step)).view(*shape).double() / (1 - p)


def eps_of(shape, seed, tid, step):
    n = 1
    for s in shape:
        n *= s
    return torch.from_numpy(P.normal(n, seed, P.STREAM_WEIGHT + tid, step)).view(*shape).double()


# ------------------------------------------------------------------ operand layouts (GPU copies of a CPU fp32 tensor)
def aligned(t):
    return t.to(DEV)


def strided(t):
    """Same values, non-contiguous: a column slice of a wider matrix (1-D: every other element)."""
    if t.dim() == 1:
        v = torch.zeros(2 * t.numel() + 1, device=DEV)[: 2 * t.numel()][::2]
    else:
        v = torch.zeros(*t.shape[:-1], t.shape[-1] + 3, device=DEV)[..., : t.shape[-1]]
    v.copy_(t)
    assert not v.is_contiguous()
    return v


def offset(k):
    def f(t):
        v = torch.zeros(t.numel() + k + 4, device=DEV)[k:k + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 * k
        return v
    f.__name__ = "offset%d" % k
    return f


def as_f64(t):
    return t.double().to(DEV)


LAYOUTS = {"strided": strided, "offset1": offset(1), "offset2": offset(2), "offset3": offset(3), "f64": as_f64}


# ------------------------------------------------------------------ the table
class Case:
    """``make(g)`` -> dict of CPU tensors (float32 operands, int64 indices); ``diff``: the names that get gradients;
    ``weights``: the weight-like names; ``fwd(ops, t)`` the GPU call; ``ref(t)`` the same operation in float64 on the CPU;
    ``unit``: the op ignores the upstream gradient's value (cross_entropy unit_grad: it must be exactly 1);
    ``consumes``: inputs the op documents as overwritten; ``in_place``: weights whose gradient the op can only accumulate
    straight into .grad (ops._weight(in_place=True)): anything but the caller's contiguous leaf with a contiguous .grad
    must raise BayesLMError before any launch."""

    def __init__(self, name, make, diff, fwd, ref, weights=(), tol=(1e-5, 2e-5), unit=False, consumes=(), scalar=False, in_place=()):
        self.name, self.make, self.diff, self.fwd, self.ref = name, make, tuple(diff), fwd, ref
        self.weights, self.tol, self.unit, self.consumes, self.scalar = tuple(weights), tol, unit, tuple(consumes), scalar
        self.in_place = tuple(in_place)

    def shapes(self):
        return {k: tuple(v.shape) for k, v in self.make(torch.Generator().manual_seed(0)).items()}


def _lin_make(M, N, K):
    def make(g):
        return {"x": torch.randn(M, 3, K, generator=g), "w": torch.randn(N, K, generator=g) * 0.2, "b": torch.randn(N, generator=g)}
    return make


def _bl(noise, fused):
    def make(g):
        return {"x": torch.randn(4, 3, 64, generator=g), "mu": torch.randn(48, 64, generator=g) * 0.1,
                "lgstd": torch.rand(48, 64, generator=g) - 3.0}

    def fwd(ops, t):
        return ops.bayes_linear(t["x"], t["mu"], t["lgstd"], ops.NoiseSpec(None, 1111, 5, 42) if noise else None, 0.0, fused)

    def ref(t):
        W = t["mu"] + torch.exp(t["lgstd"]) * eps_of((48, 64), 1111, 5, 42) if noise else t["mu"]
        return F.linear(t["x"], W)
    return make, fwd, ref


def _attn_ref(q, k, v, nhead):
    T, B, d = q.shape
    hd = d // nhead
    sh = lambda a: a.reshape(T, B * nhead, hd).transpose(0, 1)  # noqa: E731
    s = torch.bmm(sh(q), sh(k).transpose(1, 2)) / hd ** 0.5
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    return torch.bmm(torch.softmax(s, -1), sh(v)).transpose(0, 1).reshape(T, B, d)


def _attn(nhead, hd, packed):
    d = nhead * hd

    def make(g):
        if packed:
            return {"qkv": torch.randn(20, 2, 3 * d, generator=g)}
        return {n: torch.randn(20, 2, d, generator=g) for n in ("q", "k", "v")}

    def fwd(ops, t):
        return ops.attention(t["qkv"], nhead) if packed else ops.attention_qkv(t["q"], t["k"], t["v"], nhead)

    def ref(t):
        if packed:
            return _attn_ref(*t["qkv"].chunk(3, -1), nhead)
        return _attn_ref(t["q"], t["k"], t["v"], nhead)
    return make, fwd, ref, (("qkv",) if packed else ("q", "k", "v"))


def _ln(p, T=6, B=5, D=64):
    def make(g):
        return {"x": torch.randn(T, B, D, generator=g), "y": torch.randn(T, B, D, generator=g),
                "gamma": torch.randn(D, generator=g), "beta": torch.randn(D, generator=g)}

    def fwd(ops, t):
        return ops.add_dropout_ln(t["x"], t["y"], t["gamma"], t["beta"], 1e-5, ops.Drop(p, 5, 1, 2, 0, B) if p else ops.NO_DROP)

    def ref(t):
        y = t["y"] * keep((T, B, D), p, 5, 1, 2) if p else t["y"]
        return F.layer_norm(t["x"] + y, (D,), t["gamma"], t["beta"], 1e-5)
    return make, fwd, ref


def _embed(p, T=7, B=3, V=50, D=64):
    def make(g):
        return {"ids": torch.randint(0, V, (T, B), generator=g), "weight": torch.randn(V, D, generator=g),
                "pe": torch.randn(16, D, generator=g)}

    def fwd(ops, t):
        return ops.embed(t["ids"], t["weight"], t["pe"], 2.0, ops.Drop(p, 9, 3, 1, 0, B) if p else ops.NO_DROP)

    def ref(t):
        out = t["weight"][t["ids"]] * 2.0 + t["pe"][:T, None]
        return out * keep((T, B, D), p, 9, 3, 1) if p else out
    return make, fwd, ref


def _ce(mode, M=12, V=70):
    def make(g):
        return {"logits": torch.randn(M, V, generator=g) * 2, "tgt": torch.randint(0, V, (M,), generator=g)}

    def fwd(ops, t):
        if mode == "torch":
            return F.cross_entropy(ops.as_logits(t["logits"]), t["tgt"])
        return ops.cross_entropy(t["logits"], t["tgt"], unit_grad=(mode == "unit"))[0]

    def ref(t):
        return F.cross_entropy(t["logits"], t["tgt"])
    return make, fwd, ref


def _mk(**shapes):
    def make(g):
        return {k: (torch.randn(*s, generator=g) if not callable(s) else s(g)) for k, s in shapes.items()}
    return make


CASES = [
    Case("linear_n96", _lin_make(5, 96, 64), ("x", "w", "b"), lambda ops, t: ops.linear(t["x"], t["w"], t["b"]),
         lambda t: F.linear(t["x"], t["w"], t["b"]), weights=("w", "b")),
    Case("linear_n67", _lin_make(5, 67, 32), ("x", "w", "b"), lambda ops, t: ops.linear(t["x"], t["w"], t["b"]),
         lambda t: F.linear(t["x"], t["w"], t["b"]), weights=("w", "b")),
    Case("bayes_linear_mean", *_bl(False, False)[:1], ("x", "mu"), *_bl(False, False)[1:], weights=("mu", "lgstd")),
    Case("bayes_linear_noise", *_bl(True, False)[:1], ("x", "mu", "lgstd"), *_bl(True, False)[1:], weights=("mu", "lgstd"),
         tol=(2e-4, 5e-4)),
    Case("bayes_linear_fused", *_bl(True, True)[:1], ("x", "mu", "lgstd"), *_bl(True, True)[1:], weights=("mu", "lgstd"),
         tol=(2e-4, 5e-4)),
]
for _nh, _hd in ((2, 64), (1, 100)):
    for _packed in (True, False):
        _m, _f, _r, _d = _attn(_nh, _hd, _packed)
        CASES.append(Case("attention%s_hd%d" % ("" if _packed else "_qkv", _hd), _m, _d, _f, _r))
for _p in (0.0, 0.25):
    CASES.append(Case("add_dropout_ln_p%g" % _p, _ln(_p)[0], ("x", "y", "gamma", "beta"), *_ln(_p)[1:], weights=("gamma", "beta")))
    CASES.append(Case("embed_p%g" % _p, _embed(_p)[0], ("weight",), *_embed(_p)[1:], weights=("weight", "pe")))
CASES += [
    Case("add_pe", _mk(x=(7, 3, 64), pe=(16, 64)), ("x",),
         lambda ops, t: ops.add_pe(t["x"], t["pe"], ops.Drop(0.3, 4, 6, 2, 0, 3)),
         lambda t: (t["x"] + t["pe"][:7, None]) * keep((7, 3, 64), 0.3, 4, 6, 2), weights=("pe",)),
    Case("dropout", _mk(x=(6, 3, 64)), ("x",), lambda ops, t: ops.dropout(t["x"], ops.Drop(0.3, 8, 2, 5, 0, 3)),
         lambda t: t["x"] * keep((6, 3, 64), 0.3, 8, 2, 5)),
    Case("cross_entropy", _ce("plain")[0], ("logits",), *_ce("plain")[1:], consumes=("logits",), scalar=True),
    Case("cross_entropy_unit", _ce("unit")[0], ("logits",), *_ce("unit")[1:], unit=True, consumes=("logits",), scalar=True),
    Case("cross_entropy_as_logits", _ce("torch")[0], ("logits",), *_ce("torch")[1:], scalar=True),
    Case("kl_mean", _mk(mu=(20, 8), lgstd=lambda g: torch.rand(20, 8, generator=g) - 2.0), ("mu", "lgstd"),
         lambda ops, t: ops.kl_mean(t["mu"], t["lgstd"]),
         lambda t: (t["mu"] ** 2 - 2 * t["lgstd"] + torch.exp(2 * t["lgstd"])).mean() / 2, weights=("mu", "lgstd"), scalar=True),
    Case("sampled", _mk(mu=(12, 16), lgstd=lambda g: torch.rand(12, 16, generator=g) - 2.0), ("mu", "lgstd"),
         lambda ops, t: ops.sampled(t["mu"], t["lgstd"], ops.NoiseSpec(None, 3, 5, 2)),
         lambda t: t["mu"] + torch.exp(t["lgstd"]) * eps_of((12, 16), 3, 5, 2), weights=("mu", "lgstd")),
    Case("gp_mix", _mk(z=(5, 3, 32), coef4=(4, 32)), ("z", "coef4"), lambda ops, t: ops.gp_mix(t["z"], t["coef4"]),
         lambda t: O.gp_mixture(t["z"], t["coef4"], ("tanh", "sigmoid", "relu", "gelu")), weights=("coef4",)),
    Case("add_rowvec", _mk(h=(6, 32), v=(32,)), ("h", "v"), lambda ops, t: ops.add_rowvec(t["h"], t["v"]),
         lambda t: t["h"] + t["v"], weights=("v",)),
    Case("mix2", _mk(a=(5, 3, 32), b=(5, 3, 32), probs=lambda g: torch.rand(2, generator=g)), ("a", "b", "probs"),
         lambda ops, t: ops.mix2(t["a"], t["b"], t["probs"], ops.Drop(0.2, 6, 7, 3, 0, 3)),
         lambda t: (t["probs"][0] * t["a"] + t["probs"][1] * t["b"]) * keep((5, 3, 32), 0.2, 6, 7, 3), weights=("probs",)),
]


# the feed-forward ops with dropout on (a column window: 5 of 9 global columns from 2): the GELU and GP-mixture epilogues of the
# first product, its backward epilogue, and the second linear plain, Bayesian (injected eps) and under local reparameterisation
def _ffn(kind, T=6, B=5, D=32, Fd=40):
    site = {"plain": 4, "bayes": 5, "gp": 6, "lrt": 7}[kind]
    noise = torch.randn(T * B * D if kind == "lrt" else D * Fd, generator=torch.Generator().manual_seed(40 + site))

    def make(g):
        rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        t = {"x": rn(T, B, D), "w1": rn(Fd, D) * D ** -0.5, "b1": rn(Fd) * 0.5}
        if kind == "gp":
            t["coef"] = torch.rand(4, Fd, generator=g) + 0.25
        t["w2"] = rn(D, Fd) * Fd ** -0.5
        if kind in ("plain", "gp"):
            t["b2"] = rn(D) * 0.5
        else:
            t["lgstd2"] = torch.rand(D, Fd, generator=g) - 3.0
        return t

    def fwd(ops, t):
        drop = ops.Drop(0.3, 21, site, 3, 2, 9)
        if kind == "plain":
            return ops.ffn(t["x"], t["w1"], t["b1"], t["w2"], t["b2"], drop=drop)
        if kind == "gp":
            return ops.ffn_gp(t["x"], t["w1"], t["b1"], t["coef"], t["w2"], t["b2"], drop=drop)
        if kind == "lrt":
            return ops.ffn_lrt(t["x"], t["w1"], t["b1"], t["w2"], t["lgstd2"], ops.LrtNoise(eps=noise.view(T * B, D).to(DEV)), drop=drop)
        return ops.ffn(t["x"], t["w1"], t["b1"], t["w2"], None, t["lgstd2"], ops.NoiseSpec(eps=noise.view(D, Fd).to(DEV)), drop=drop)

    def ref(t):
        z = F.linear(t["x"], t["w1"], t["b1"])
        h = O.gp_mixture(z, t["coef"], ("tanh", "sigmoid", "relu", "gelu")) if kind == "gp" else F.gelu(z)
        h = h * keep((T, 9, Fd), 0.3, 21, site, 3)[:, 2:2 + B]
        if kind in ("plain", "gp"):
            return F.linear(h, t["w2"], t["b2"])
        if kind == "lrt":
            return F.linear(h, t["w2"]) + torch.sqrt(F.linear(h * h, torch.exp(2 * t["lgstd2"]))) * noise.double().view(T, B, D)
        return F.linear(h, t["w2"] + torch.exp(t["lgstd2"]) * noise.double().view(D, Fd))
    names = list(make(torch.Generator().manual_seed(0)))
    in_place = {"plain": ("w1", "b1", "w2", "b2"), "bayes": ("w1", "b1", "w2", "lgstd2"), "gp": ("w2", "b2"), "lrt": ("w1", "b1")}[kind]
    return Case({"plain": "ffn", "bayes": "ffn_bayes", "gp": "ffn_gp", "lrt": "ffn_lrt"}[kind], make, names, fwd, ref,
                weights=names[1:], in_place=in_place)


CASES += [_ffn("plain"), _ffn("bayes"), _ffn("gp"), _ffn("lrt")]
BY_NAME = {c.name: c for c in CASES}


def _inputs(case, seed):
    g = torch.Generator().manual_seed(seed)
    return case.make(g)


def _reference(case, cpu, go):
    """float64 reference: (output, {name: grad}) for the upstream gradient ``go`` (CPU)."""
    t = {k: (v.double().requires_grad_(k in case.diff) if v.is_floating_point() else v) for k, v in cpu.items()}
    out = case.ref(t)
    out.backward(go.double())
    return out.detach(), {k: t[k].grad for k in case.diff}


def _gpu_leaves(case, cpu, layouts):
    t = {}
    for k, v in cpu.items():
        if not v.is_floating_point():
            t[k] = v.to(DEV)
            continue
        g = layouts.get(k, aligned)(v)
        if k in case.diff:
            g.requires_grad_(True)
        t[k] = g
    return t


def _check_grads(case, t, ref_grads, scale=1.0, base=None):
    tol = case.tol[1]
    for k in case.diff:
        want = ref_grads[k] * scale + (base[k] if base is not None and k in base else 0)
        got = t[k].grad
        assert got is not None, "%s: no gradient reached %s" % (case.name, k)
        assert got.shape == t[k].shape
        assert rel(got, want) < tol, (case.name, k, rel(got, want))


def _go_for(case, out, g):
    return torch.ones(()) if case.unit else torch.randn(out.shape, generator=g)


# ------------------------------------------------------------------ A. operand layouts
A_PARAMS = [(c.name, arg, lay) for c in CASES for arg, v in c.make(torch.Generator().manual_seed(0)).items()
            if v.is_floating_point() for lay in LAYOUTS]


@pytest.mark.parametrize("name,arg,layout", A_PARAMS)
def test_operand_layout(name, arg, layout):
    """Every tensor argument as a strided view, an offset view or float64: the aligned case's result, or BayesLMError."""
    ops, case = ops_mod(), BY_NAME[name]
    cpu = _inputs(case, 1)
    t = _gpu_leaves(case, cpu, {arg: LAYOUTS[layout]})
    before = {k: v.detach().clone() for k, v in t.items()}
    if layout == "strided" and arg in case.in_place:  # a gradient that can only go straight into .grad: refused, nothing launched
        with pytest.raises(BayesLMError()):
            case.fwd(ops, t)
        for k, v in before.items():  # nothing was launched: no input was written
            assert torch.equal(t[k].detach(), v), "%s: input %s changed by a refused call" % (name, k)
        return
    try:
        out = case.fwd(ops, t)
    except BayesLMError():
        if layout != "f64":  # every op takes fp32 views of any layout
            raise
        return
    go = _go_for(case, out, torch.Generator().manual_seed(2))
    ref, ref_grads = _reference(case, cpu, go)
    assert rel(out, ref) < case.tol[0], (rel(out, ref))
    out.backward(go.to(DEV))
    _check_grads(case, t, ref_grads)
    for k, v in before.items():  # D: inputs are not written (the consumed logits aside)
        if k not in case.consumes:
            assert torch.equal(t[k].detach(), v), "%s: input %s changed" % (name, k)
    # an operand the op copies gives bit for bit what the aligned operand gives
    if layout == "strided":
        t0 = _gpu_leaves(case, cpu, {})
        out0 = case.fwd(ops, t0)
        assert torch.equal(out0.detach(), out.detach())


# ------------------------------------------------------------------ B. upstream-gradient layouts
B_MODES = ("cat", "expand", "transpose", "two")
B_PARAMS = [(c.name, m) for c in CASES if not c.unit for m in B_MODES if not (c.scalar and m in ("cat", "transpose"))]


@pytest.mark.parametrize("name,mode", B_PARAMS)
def test_upstream_gradient_layout(name, mode):
    ops, case = ops_mod(), BY_NAME[name]
    cpu = _inputs(case, 3)
    g = torch.Generator().manual_seed(4)
    t = _gpu_leaves(case, cpu, {})
    probe = case.fwd(ops, _gpu_leaves(case, cpu, {})).detach()  # the output's shape
    scalar = probe.dim() == 0
    assert scalar == case.scalar
    z = None
    if mode == "cat":
        N = probe.shape[-1]
        c = (N + 3) // 4 * 4 - N if (name.startswith("linear") and N % 4) else 1 + N % 3  # odd-N linear: exactly Np - N
        z = torch.randn(*probe.shape[:-1], c, generator=g).to(DEV).requires_grad_(True)  # produced before the op
    before = {k: v.detach().clone() for k, v in t.items()}
    out = case.fwd(ops, t)
    if mode == "cat":
        G = torch.randn(*out.shape[:-1], out.shape[-1] + z.shape[-1], generator=g)
        (torch.cat([out, z], -1) * G.to(DEV)).sum().backward()
        go = G[..., :out.shape[-1]]
        assert torch.equal(z.grad.cpu(), G[..., out.shape[-1]:]), "%s: the sibling's gradient was changed" % name
    elif mode == "expand":
        if scalar:
            (out * torch.full((4,), 0.5, device=DEV)).sum().backward()
            go = torch.tensor(2.0)
        else:
            out.sum().backward()
            go = torch.ones(out.shape)
    elif mode == "transpose":
        Gt = torch.randn(out.transpose(0, -1).shape, generator=g)
        (out.transpose(0, -1) * Gt.to(DEV)).sum().backward()
        go = Gt.transpose(0, -1)
    else:
        G1, G2 = torch.randn(out.shape, generator=g), torch.randn(out.shape, generator=g)
        ((out * G1.to(DEV)).sum() + (out * G2.to(DEV)).sum()).backward()
        go = G1 + G2
    ref, ref_grads = _reference(case, cpu, go)
    _check_grads(case, t, ref_grads)
    for k, v in before.items():
        if k not in case.consumes:
            assert torch.equal(t[k].detach(), v), "%s: input %s changed" % (name, k)


# ------------------------------------------------------------------ C. gradient routing of weights
C_MODES = ("nonleaf", "strided_leaf", "shared", "held_grad", "strided_grad")
C_PARAMS = [(c.name, w, m) for c in CASES for w in c.weights if w in c.diff for m in C_MODES
            if not (m == "strided_grad" and len(c.shapes()[w]) < 2)]  # every .grad layout of a 1-D weight is contiguous


@pytest.mark.parametrize("name,wname,mode", C_PARAMS)
def test_weight_gradient_routing(name, wname, mode):
    """The caller's leaf gets the reference gradient whatever tensor reaches the op, or the op raises at forward."""
    ops, case = ops_mod(), BY_NAME[name]
    cpu = _inputs(case, 5)
    go = None
    t = _gpu_leaves(case, cpu, {wname: strided} if mode == "strided_leaf" else {})
    leaf = t[wname]
    base = None
    if mode == "held_grad":
        leaf.grad = torch.full(leaf.shape, 0.5, device=DEV)
        base = {wname: torch.full(leaf.shape, 0.5, dtype=torch.float64)}
    if mode == "strided_grad":
        vals = torch.randn(leaf.shape, generator=torch.Generator().manual_seed(6))
        leaf.grad = vals.t().contiguous().to(DEV).t()
        assert not leaf.grad.is_contiguous()
        base = {wname: vals.double()}
    call = dict(t)
    if mode == "nonleaf":
        call[wname] = leaf * 1.0
    if wname in case.in_place and mode in ("nonleaf", "strided_leaf", "strided_grad"):
        before = {k: v.detach().clone() for k, v in call.items()}
        held = None if leaf.grad is None else leaf.grad.clone()
        with pytest.raises(BayesLMError()):
            case.fwd(ops, call)
        for k, v in before.items():  # nothing was launched: no input and no held gradient was written
            assert torch.equal(call[k].detach(), v), "%s: input %s changed by a refused call" % (name, k)
        assert held is None or torch.equal(leaf.grad, held)
        return
    out = case.fwd(ops, call)
    g = torch.Generator().manual_seed(7)
    go = _go_for(case, out, g)
    if mode == "shared":
        out2 = case.fwd(ops, call)
        go2 = _go_for(case, out2, g)
        ((out * go.to(DEV)).sum() + (out2 * go2.to(DEV)).sum()).backward()
        go = go + go2
    else:
        out.backward(go.to(DEV))
    ref, ref_grads = _reference(case, cpu, go)
    _check_grads(case, t, ref_grads, base=base)


# ------------------------------------------------------------------ D. a retained graph differentiated twice
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_backward_twice_adds_or_raises(name):
    ops, case = ops_mod(), BY_NAME[name]
    cpu = _inputs(case, 8)
    t = _gpu_leaves(case, cpu, {})
    out = case.fwd(ops, t)
    go = _go_for(case, out, torch.Generator().manual_seed(9))
    out.backward(go.to(DEV), retain_graph=True)
    try:
        out.backward(go.to(DEV))
    except RuntimeError:  # BayesLMError is one; autograd's "freed buffers" is the other legitimate refusal
        return
    ref, ref_grads = _reference(case, cpu, go)
    _check_grads(case, t, ref_grads, scale=2.0)


# ------------------------------------------------------------------ the odd-vocabulary decoder: padded buffers it owns
def test_linear_padded_backward_still_taken_for_its_own_logits():
    """The padding-aware backward of an odd N is kept for the buffers the engine hands out: the decoder's own output and
    the gradient of the `Logits` loss; both give the reference gradients."""
    ops = ops_mod()
    case = BY_NAME["linear_n67"]
    cpu = _inputs(case, 10)
    tgt = torch.randint(0, 67, (15,), generator=torch.Generator().manual_seed(11))
    for keep_path in (False, True):
        t = _gpu_leaves(case, cpu, {})
        y = ops.linear(t["x"], t["w"], t["b"])
        assert ops._owns_padded(y)
        if keep_path:
            loss = F.cross_entropy(ops.as_logits(y).view(-1, 67), tgt.to(DEV))
        else:
            loss = ops.cross_entropy(y.view(-1, 67), tgt.to(DEV), unit_grad=True)[0]
        loss.backward()
        tr = {k: (v.double().requires_grad_(k in case.diff)) for k, v in cpu.items()}
        F.cross_entropy(F.linear(tr["x"], tr["w"], tr["b"]).view(-1, 67), tgt).backward()
        for k in case.diff:
            assert rel(t[k].grad, tr[k].grad) < 2e-5, (keep_path, k)


# ------------------------------------------------------------------ LayerNorm kernels: every width class, dropout, many rows
@pytest.mark.parametrize("T,B,D,p", [(6, 5, 2048, 0.0), (6, 5, 2048, 0.2),      # VPT = 8 register kernel
                                      (1024, 8, 512, 0.2),                       # the headline: 8192 rows, grid-stride rows
                                      (130, 8, 1100, 0.0), (130, 8, 1100, 0.2),  # generic width, M > 1024
                                      (30, 1, 768, 0.2), (7, 3, 100, 0.2)])
def test_add_dropout_ln_backward_elementwise(T, B, D, p):
    """Forward and every gradient against float64 with the Philox mask, accumulated onto .grad that already holds values."""
    ops = ops_mod()
    make, fwd, ref = _ln(p, T, B, D)
    case = Case("ln", make, ("x", "y", "gamma", "beta"), fwd, ref)
    cpu = _inputs(case, D + T)
    t = _gpu_leaves(case, cpu, {})
    t["gamma"].grad = torch.full((D,), 0.25, device=DEV)
    t["beta"].grad = torch.full((D,), -0.5, device=DEV)
    out = case.fwd(ops, t)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(12))
    r, ref_grads = _reference(case, cpu, go)
    assert rel(out, r) < 1e-5
    out.backward(go.to(DEV))
    base = {"gamma": torch.full((D,), 0.25, dtype=torch.float64), "beta": torch.full((D,), -0.5, dtype=torch.float64)}
    _check_grads(case, t, ref_grads, base=base)
