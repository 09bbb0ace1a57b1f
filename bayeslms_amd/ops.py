"""Operators of the hot path as torch.autograd.Functions over the C ABI.

Each Function launches hand-written gfx950 kernels from libbayeslm_hip.so on
torch's current HIP stream with raw device pointers.  PyTorch is used for
device memory and the autograd tape only.  Parameter gradients are accumulated
straight into ``param.grad`` by the wgrad kernels (BLM_GEMM_ACCUMULATE), so the
flat gradient buffer the data-parallel all-reduce works on is filled in place;
the Functions return ``None`` for parameters.

There is no CPU path: every entry point raises on non-GPU tensors.

What each op accepts: floating operands are fp32 on this process's GPU, anything else raises
BayesLMError; strided operands are copied, offset ones are read in place through the kernels' scalar loops; a weight that
is not a contiguous leaf with a contiguous (or no) .grad -- a non-leaf, a strided leaf -- gets its gradient back through
autograd (`_weight`, `_wgrad_target`), except where an op can only accumulate in place, which then raises at forward.
"""
import ctypes as C
import math
import os
import threading
import weakref
from dataclasses import dataclass
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

from . import _lib as L
from ._lib import BayesLMError, calls, dev_tensor, ptr, stream

__all__ = ["Drop", "NoiseSpec", "LrtNoise", "ResidualLink", "linear", "bayes_linear", "bayes_linear_lrt", "ffn", "ffn_lrt", "ffn_gp", "attention", "attention_qkv", "add_dropout_ln",
           "embed", "add_pe", "dropout", "cross_entropy", "cross_entropy_soft", "SoftStats", "cross_entropy_soft_topk", "SparseTargets", "kl_mean", "philox_normal", "sample_weight", "sampled", "lstm_layer", "lstm_stack2", "lstm_stack2_ok", "set_lstm_wavefront", "lstm_cell", "gp_mix", "add_rowvec",
           "clip_sgd", "gemm", "PtrTable", "set_grad_ready_hook", "set_embed_grad_sink", "rows_gather_add", "KernelTimer", "set_kernel_timer"]


# ----------------------------------------------------------------------------
# small descriptors
# ----------------------------------------------------------------------------
@dataclass
class Drop:
    """A dropout site: probability + Philox key + the global column window of
    this rank (masks are keyed by global column)."""
    p: float = 0.0
    seed: int = 0
    site: int = 0
    step: int = 0
    col_offset: int = 0
    global_cols: int = 0
    keep: torch.Tensor = None  # attention only (parity mode): the dropout factors of the probabilities themselves, (global_cols * nhead, T, T)

    @property
    def on(self):
        return self.p > 0.0

    def rng(self):
        return L.rng(self.seed, L.STREAM_DROPOUT + self.site, self.step)


NO_DROP = Drop()


@dataclass
class NoiseSpec:
    """Where eps of a variational tensor comes from: an injected tensor
    (parity tests) or the Philox stream (seed, tensor id, step)."""
    eps: torch.Tensor = None
    seed: int = 0
    tensor_id: int = 0
    step: int = 0

    def rng(self):
        return L.rng(self.seed, L.STREAM_WEIGHT + self.tensor_id, self.step)


def _variational(lgstd, noise, row_lo, srows):
    v = L.Variational()
    v.lgstd = ptr(lgstd)
    if noise is not None and noise.eps is not None:
        e = noise.eps
        # an injected eps is read by the kernels with lgstd's extent on trust: a wrong shape would read past it
        if not (torch.is_tensor(e) and e.is_cuda and e.dtype == torch.float32 and e.is_contiguous() and e.numel() == lgstd.numel()):
            raise BayesLMError("injected eps must be a contiguous fp32 GPU tensor with lgstd's %d elements, got %s"
                               % (lgstd.numel(), (tuple(e.shape), e.dtype, e.device) if torch.is_tensor(e) else type(e)))
    v.eps = ptr(noise.eps) if (noise is not None and noise.eps is not None) else None
    v.row_lo = int(row_lo)
    v.srows = int(srows)
    v.rng = noise.rng() if noise is not None else L.rng(0, 0, 0)
    return v


class _GradSlab:
    """Where ``param.grad`` comes from when it is None -- the state ``zero_grad()`` (set_to_none, torch's default and what the
    reference's loop leaves behind, train.py:401) puts every parameter in at the start of every step.  A zeros_like per
    parameter is one fill launch each: 78 launches of ~5 us per step of the headline model under the reference's own loop
    (INTEGRATION level 1; 1.9 % of the step, rocprofv3 of tools/level1_probe.py).  Instead: the parameters seen in one step
    get a 256-byte aligned slot each, and from the next step on the first request of a step allocates ONE zeroed slab for
    all of them (one fill) and every request is a view into it.  A parameter asking again for a slot the current slab has
    already handed out means a new step has begun: new slab.  Dead parameters (weak references) leave the layout when a
    slab is built.  The data-parallel trainer never comes here: its gradients are views of engine.FlatBuffers."""

    def __init__(self):
        self.lock = threading.Lock()
        self.on = True
        self.dev = {}

    @staticmethod
    def eligible(param):
        return param.is_cuda and param.dtype == torch.float32

    def take(self, param):
        if not (self.on and self.eligible(param)):
            return torch.zeros_like(param, memory_format=torch.contiguous_format)
        key = id(param)
        with self.lock:
            st = self.dev.setdefault(param.device, {"slots": {}, "total": 0, "buf": None, "claimed": set()})
            slot = st["slots"].get(key)
            if slot is not None and (slot[0]() is not param or slot[2] != param.numel()):
                slot = None  # the id belongs to another tensor now
            if slot is None:  # first sight: plain zeros now, a slot from the next step on
                n = param.numel()
                st["slots"][key] = (weakref.ref(param), st["total"], n)
                st["total"] += (n + 63) // 64 * 64
                st["buf"] = None  # the slab in use does not know the new layout
                return torch.zeros_like(param, memory_format=torch.contiguous_format)
            if st["buf"] is None or key in st["claimed"]:
                off = 0
                live = {}
                for k, (ref, _, n) in st["slots"].items():
                    if ref() is not None:
                        live[k] = (ref, off, n)
                        off += (n + 63) // 64 * 64
                st["slots"], st["total"] = live, off
                st["buf"] = torch.zeros(off, device=param.device, dtype=torch.float32)
                st["claimed"] = set()
                slot = live[key]
            st["claimed"].add(key)
            return st["buf"][slot[1]:slot[1] + slot[2]].view(param.shape)


_GRAD_SLAB = _GradSlab()


def set_grad_slab(on):
    """False: every missing ``param.grad`` is its own zeros_like again (tests compare the two)."""
    _GRAD_SLAB.on = bool(on)
    with _GRAD_SLAB.lock:
        _GRAD_SLAB.dev.clear()


def _grad_buf(param):
    """param.grad (zeroed when it does not exist yet: a view of the step's gradient slab): wgrad kernels accumulate into it."""
    if param.grad is None:
        param.grad = _GRAD_SLAB.take(param)
    return param.grad


_GRAD_HOOK = None


def set_grad_ready_hook(fn):
    """fn(param) is called after a backward kernel that writes param.grad has been enqueued (the
    data-parallel reducer uses it to start bucket all-reduces while backward is still running)."""
    global _GRAD_HOOK
    _GRAD_HOOK = fn


_EMBED_SINK = None


def set_embed_grad_sink(fn):
    """Data-parallel training only.  ``fn(weight, ids)`` is asked by the embedding backward where its rows go: None =
    scatter into weight.grad as usual; or (buffer, slot_ids, n_rows, done) = scatter dy rows into the compact
    (n_rows, D) ``buffer`` at row ``slot_ids[t,b]`` and call ``done()`` once the kernel is enqueued (engine.LateRows:
    the embedding half of the tied encoder/decoder gradient is exchanged as the rows this step touched)."""
    global _EMBED_SINK
    _EMBED_SINK = fn


def rows_gather_add(dst, slot, src, n_src):
    """dst[v,:] += src[slot[v],:] where 0 <= slot[v] < n_src."""
    L.require_gfx950()
    V, D = dst.shape
    calls().blm_rows_gather_add(ptr(dst), ptr(dev_tensor(slot, "slot", torch.int64)), ptr(src), V, D, int(n_src), stream())


def _notify(*params):
    if _GRAD_HOOK is not None:
        for p in params:
            if p is not None and p.is_leaf and p.requires_grad:
                _GRAD_HOOK(p)


_VP8, _I64x8 = C.c_void_p * 8, C.c_int64 * 8


def _init_multi(items):
    """``items``: (dst, src | None, src2 | None) triples of equally sized vectors -- dst = (src or 0) + (src2 or 0) -- set by
    one launch per eight (blm_init_multi): the initial states into row 0 of the state histories, b_ih + b_hh, zeroed gradient
    carries of a recurrent layer.  dst must be contiguous fp32 views on the GPU; sources of another layout / type are converted."""
    L.require_gfx950()
    for k in range(0, len(items), 8):
        part = items[k:k + 8]
        d, a, b, n = _VP8(), _VP8(), _VP8(), _I64x8()
        keep = []
        for i, (dst, s1, s2) in enumerate(part):
            if not (dst.is_cuda and dst.dtype == torch.float32 and dst.is_contiguous()):
                raise BayesLMError("_init_multi: destinations are contiguous fp32 GPU tensors")
            d[i], n[i] = dst.data_ptr(), dst.numel()
            for arr, src in ((a, s1), (b, s2)):
                if src is None:
                    arr[i] = None
                    continue
                src = _f32(src, "src")
                if src.numel() != dst.numel():
                    raise BayesLMError("_init_multi: %d elements into %d" % (src.numel(), dst.numel()))
                keep.append(src)
                arr[i] = src.data_ptr()
        calls().blm_init_multi(len(part), d, a, b, n, stream())


def _grad_in_place(w):
    """May a backward kernel accumulate w's gradient straight into ``w.grad``?  Only when w is the caller's own contiguous
    leaf and its .grad is absent or a contiguous fp32 GPU tensor.  A non-leaf (``p * 1.0``, a parametrization, the
    contiguous copy `_weight` made of a strided parameter) would keep a .grad nobody reads, and a strided .grad would be
    written as if it were contiguous."""
    if not (w.is_leaf and w.is_contiguous()):
        return False
    g = w.grad
    return g is None or (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous())


def _wgrad_target(w, zero=False):
    """-> (buffer, accumulate, value_to_return): a weight that `_grad_in_place` allows accumulates into .grad and autograd
    gets None; any other (a sampled tensor, a non-leaf, a copy) gets a fresh gradient tensor that goes back through
    autograd.  ``zero``: the kernel only accumulates, so the fresh tensor starts at 0."""
    if _grad_in_place(w):
        return _grad_buf(w), True, None
    buf = (torch.zeros if zero else torch.empty)(w.shape, device=w.device, dtype=torch.float32)
    return buf, False, buf


def _f32(t, name):
    return dev_tensor(t, name, torch.float32)


def _weight(t, name, in_place=False):
    """The operand guard of a weight-like argument (weights, LayerNorm parameters, positional tables), applied BEFORE the
    autograd Function sees it: an fp32 tensor on this process's GPU (BayesLMError otherwise: no float64, no host tensor); a
    non-contiguous one is replaced by its contiguous copy, which autograd links back to the caller's tensor, so the
    Function's `_wgrad_target` hands the gradient back through autograd.  ``in_place``: the Function can only accumulate
    into .grad -- a tensor that requires grad and that `_grad_in_place` refuses raises here, before any launch."""
    if t is None:
        return None
    if not torch.is_tensor(t):
        raise BayesLMError("%s must be a tensor, got %s" % (name, type(t).__name__))
    if in_place and t.requires_grad and torch.is_grad_enabled() and not _grad_in_place(t):
        raise BayesLMError("%s: this op accumulates its gradient straight into .grad, so it takes a contiguous leaf tensor "
                           "(whose .grad, if any, is contiguous fp32) only; got a %s" % (
                               name, "non-leaf tensor" if not t.is_leaf else "strided tensor or .grad"))
    return _f32(t, name)


def _rows_in_place(who, name, t, V=None, copy=False, overlap=False):
    """The operand check of the row kernels that take a row stride: ``t`` as a 2-D float32 device matrix with unit inner stride
    whose first V columns (default: all) are used -> (tensor, R, V, row stride as the kernel takes it).  A view of padded rows
    is read where it lies, after the device checks of the product path on its first row.  ``copy`` (a read-only operand):
    anything else goes through `_f32`, which copies a non-contiguous tensor; without it (an operand used in place) anything else
    is refused, and so are rows that overlap (row stride < V) unless ``overlap`` leaves that to the library."""
    label = "%s: %s" % (who, name)
    ok = torch.is_tensor(t) and t.dim() == 2 and t.stride(-1) == 1
    if ok and (not copy or t.stride(0) >= t.shape[1]):
        dev_tensor(t[:1], label)  # the view itself is what the kernel reads
    elif copy and torch.is_tensor(t):
        t = _f32(t, label)
        ok = t.dim() == 2 and t.stride(-1) == 1
    if not ok:
        raise BayesLMError("%s must be a row-major (R, V) matrix with unit inner stride" % label)
    R, V, given = t.shape[0], int(V if V is not None else t.shape[1]), V is not None
    if given and not 1 <= V <= t.shape[1]:  # a matrix without columns is the library's to refuse, or to accept
        raise BayesLMError("%s: V = %d outside [1, %d], the columns of %s" % (who, V, t.shape[1], name))
    ld = t.stride(0) if R > 1 else max(t.stride(0), V)  # a single row has no stride to honour: torch may report any
    if ld < V and not copy and not overlap:
        raise BayesLMError("%s: the rows of %s overlap (row stride %d < %d)" % (who, name, ld, V))
    return t, R, V, ld


def _rows_pair(who, na, a, nb, b, V, overlap=False):
    """Two operands of `_rows_in_place`, both used in place, with one row count -> (R, V, row stride of a, of b)"""
    _, R, V, lda = _rows_in_place(who, na, a, V, overlap=overlap)
    _, Rb, _, ldb = _rows_in_place(who, nb, b, V, overlap=overlap)
    if Rb != R:
        raise BayesLMError("%s: %s has %d rows, %s %d" % (who, na, R, nb, Rb))
    return R, V, lda, ldb


def _row_targets(who, targets, R):
    """(R,) int64 device targets, one per row, or None"""
    if targets is None:
        return None
    tgt = dev_tensor(targets.reshape(-1), "%s: targets" % who, torch.int64)
    if tgt.numel() != R:
        raise BayesLMError("%s: %d targets for %d rows" % (who, tgt.numel(), R))
    return tgt


def _slots(what, struct, field, arg, values, bound, strict, noun, entry):
    """The ABI struct of the 1..bound values ``entry`` takes per launch (``noun``s: inverse temperatures, thetas): finite
    float32 numbers > 0 (``strict``) or >= 0, each rounded to float32 once."""
    above = (lambda v: v > 0.0) if strict else (lambda v: v >= 0.0)
    kind = "finite float32 number %s 0" % (">" if strict else ">=")
    try:
        vs = [float(v) for v in values]
    except (TypeError, ValueError):
        raise BayesLMError("%s: %s must be 1..%d %ss, each a %s, got %r" % (what, arg, bound, noun, kind, values))
    if not 1 <= len(vs) <= bound:
        raise BayesLMError("%s: %d %ss, %s takes 1..%d per launch" % (what, len(vs), noun, entry, bound))
    t = struct()
    t.abi_version, t.count = L.ABI_VERSION, len(vs)
    slot = getattr(t, field)
    for j, v in enumerate(vs):
        slot[j] = v if math.isfinite(v) else 0.0  # ctypes rounds to float32 (an overflow to inf, an underflow to 0 is caught below)
        if not (math.isfinite(v) and above(v) and above(slot[j]) and slot[j] < math.inf):
            raise BayesLMError("%s: %s[%d] = %r is not a %s" % (what, arg, j, v, kind))
    return t


def _rows2d(t, N, name):
    """-> ((M, N) view of ``t``, its row stride).  The logits of a vocabulary that is not a multiple of 4 words (wikitext-2: 33278)
    live in a buffer whose rows are padded to one (below): the kernels take the row stride, so such a tensor is used as it is; any
    other layout is made contiguous first, as `_f32` does."""
    if t.dim() >= 2 and t.shape[-1] == N and not t.is_contiguous() and t.stride(-1) == 1 and t.is_cuda and t.dtype == torch.float32:
        try:
            v = t.view(-1, N)  # fails if the leading dimensions are not uniformly strided
        except RuntimeError:
            v = None
        if v is not None and v.stride(0) >= N and v.stride(0) % 4 == 0 and v.data_ptr() % 16 == 0:
            dev_tensor(v[:1], name, torch.float32)  # the device checks of the product path
            return v, v.stride(0)
    c = _f32(t, name)
    return c.reshape(-1, N), N


def _row_chunks(M, ld):
    """Row ranges of an (M, ld) fp32 operand that each stay under 2^32 bytes.  The LDS-DMA loaders of the GEMM kernels address an
    operand with 32-bit byte offsets (include/bayeslm.h: larger operands take the guarded loaders, at roughly half the rate); the
    logits' gradient of a 256 x 128 token batch over 33,000 words is 4.3 GB, and the 288 GB of an MI355X invite such batches
    (tools/batch_size_probe.py: 410 k tokens/s at B 128, 353 k at B 256).  The decoder's backward products run chunk by chunk instead."""
    lim = ((1 << 32) - 1) // (4 * max(int(ld), 1))
    if M <= lim or lim < 256:
        return [(0, M)]
    n = -(-M // lim)
    step = (-(-M // n) + 127) // 128 * 128
    while step > lim:
        n += 1
        step = (-(-M // n) + 127) // 128 * 128
    return [(r, min(M, r + step)) for r in range(0, M, step)]


_OWN_PADDED = weakref.WeakValueDictionary()  # storage address -> the storage object of a padded buffer handed out by this module


def _padded_rows(lead_shape, N, device):
    """An (..., N) fp32 tensor whose rows start 16 bytes aligned: a view of a buffer with the row stride rounded up to 4 floats.
    The storage is registered as this module's own: only such storage may have its padding columns written (_Linear)."""
    M = 1
    for d in lead_shape:
        M *= int(d)
    Np = (N + 3) // 4 * 4
    full = torch.empty(M, Np, device=device, dtype=torch.float32)
    st = full.untyped_storage()  # torch keeps one Python object per live storage: the weak value dies with the storage
    _OWN_PADDED[st.data_ptr()] = st
    return full[:, :N].view(*lead_shape, N), Np


def _owns_padded(t):
    """Is ``t`` a view into a buffer `_padded_rows` allocated?  Any other tensor with the same strides (a narrow view out of
    torch.cat's backward, say) may hold live data in what looks like padding.  The identity test (not the address alone)
    keeps a new allocation at a freed buffer's address out."""
    st = t.untyped_storage()
    return _OWN_PADDED.get(st.data_ptr()) is st


class _P:
    """Row addresses of a contiguous tensor: ``_P(t)[i]`` == ``t[i].data_ptr()`` without building a view per time step
    (six views per LSTM step cost more host time than the 12 us kernel they feed)."""
    __slots__ = ("b", "s")

    def __init__(self, t):
        self.b = t.data_ptr()
        self.s = t.stride(0) * t.element_size()

    def __getitem__(self, i):
        return self.b + i * self.s


class ResidualLink:
    """Joins the two backward paths of a post-LN residual block  out = LN(x + drop(f(x)))  (model.py:1041-1045).
    Autograd would add the residual path's gradient (from the LayerNorm backward) and the branch's input gradient
    (the last dgrad GEMM of f) with a separate elementwise pass over (T,B,d) -- 12 launches per cfg3 step.  The
    same ``link`` object is handed to the first op of the branch (``linear`` / ``ffn`` / ``ffn_gp`` ``link=``) and to
    ``add_dropout_ln(..., link=)``.  The branch op ARMS the link in its forward with the identity of its input; the
    LayerNorm (whose forward runs after the branch, whose backward runs before it) uses the link only when exactly ONE
    op armed it for the very tensor it adds as the residual.  Then its backward parks dx here and returns NO gradient
    for x; the branch's dgrad GEMM accumulates into the parked buffer (stream order: every earlier use is enqueued)
    and returns THAT as its input gradient.  Autograd therefore sees one producer for the pair, so any further
    consumer of x (a hook, a tap on the layer input, a layer variant that reuses it) is summed in correctly whatever
    order the nodes run in; when the link is not armed, or armed twice, or for another tensor, both ops fall back to
    returning their own gradients.  Explicit per-block objects, no global matching."""
    __slots__ = ("dx", "armed", "key")

    def __init__(self):
        self.dx = None
        self.armed = 0
        self.key = None

    @staticmethod
    def _key(x):
        return (x.data_ptr(), tuple(x.shape), x.is_contiguous())

    def arm(self, x):
        """Branch op, forward: 'my backward will run and will fold its input gradient into a parked buffer for x'."""
        self.armed += 1
        self.key = self._key(x)

    def joins(self, x):
        """LayerNorm, forward: is exactly one branch op waiting for this residual's gradient?"""
        return self.armed == 1 and self.key == self._key(x)

    def take(self, like):
        """The parked residual gradient if it fits ``like`` (the branch then returns it, completed, as its dx)."""
        d, self.dx = self.dx, None
        if d is not None and d.shape == like.shape and d.is_contiguous():
            return d
        return None


# ----------------------------------------------------------------------------
# per-kernel timing with HIP events on the launch stream (bench.py's live roofline numbers)
# ----------------------------------------------------------------------------
class KernelTimer:
    def __init__(self, all_gemms=False, only=None):
        self.records = []
        self.all_gemms = all_gemms  # also bracket untagged GEMMs, keyed by layout/shape/epilogue
        self.only = None if only is None else frozenset(only)  # bracket these tags only (a bracket costs the step ~8 us)

    def bracket(self, tag):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.records.append((tag, a, b))
        return a, b

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for tag, a, b in self.records:
            agg.setdefault(tag, []).append(a.elapsed_time(b))
        return {k: {"avg_ms": sum(v) / len(v), "n": len(v)} for k, v in agg.items()}


_TIMER = None


def set_kernel_timer(t):
    global _TIMER
    _TIMER = t


_NO_EVENT = SimpleNamespace(record=lambda: None)


def _timer_start(fmt, T):
    """Opens and starts a _TIMER bracket tagged ``fmt % T``; .record() on what it returns ends it (no timer: the shared no-op)."""
    if _TIMER is None:
        return _NO_EVENT
    ev0, ev1 = _TIMER.bracket(fmt % T)
    ev0.record()
    return ev1


# ----------------------------------------------------------------------------
# raw GEMM
# ----------------------------------------------------------------------------
def set_gemm_mode(mode):
    """"f32" (default, the parity mode), "bf16x3" or "bf16x6": OPT-IN split-bf16 arithmetic of the GEMM family's matrix
    instruction (include/bayeslm.h blm_set_gemm_mode): lower precision than the reference's fp32 (4.5e-6 against
    3.6e-7 max relative error per GEMM at K = 4096), about twice the GEMM rate.  Process-wide."""
    code = {"f32": 0, "bf16x3": 1, "bf16x6": 2}[mode]
    calls().blm_set_gemm_mode(code)


def set_option(name, value):
    """Kernel-selection options of the library (include/bayeslm.h blm_set_option): "attn_hpw", "attn_short", "attn_valu",
    "lstm_gemv", "lstm_pipe", "lstm_tail", "lstm_mb2", "edit_lane_max", "deterministic" (see set_deterministic).  Each of the others picks between two BUILT and parity-tested forms of a kernel; the defaults are
    the measured winners (INTEGRATION.md lists them with their tests and BLM_* environment variables)."""
    calls().blm_set_option(name.encode(), int(value))


def get_option(name):
    v = C.c_int(0)
    calls().blm_get_option(name.encode(), C.byref(v))
    return int(v.value)


def set_deterministic(on=True):
    """Deterministic mode (blm_set_option("deterministic", 1) / BLM_DETERMINISTIC=1): every reduction of the library
    in a fixed order -- one K slice per GEMM tile (no float atomics into C), bias / GP-coefficient column sums in one row chunk,
    KL sums through block partials added by one block, the embedding gradient by one wave per vocabulary row in position order
    -- and, on this side, the two-layer LSTM stack on one stream (no layer wavefront).  Two runs from one seed then give
    bit-identical losses and parameters (tests/test_gpu_deterministic.py), also two data-parallel runs of the same world
    size; a run at another world size sums the batch columns in another order and is equal to rounding only.  Costs a few
    per cent of the step (bench.py extra_configs `deterministic`).  Process-wide."""
    set_option("deterministic", 1 if on else 0)


def is_deterministic():
    return get_option("deterministic") == 1


def set_gemm_cus(n):
    """Compute units the GEMM planner may count on (0: the whole chip).  engine.GradReducer narrows it while gradient buckets
    are in flight: the collective's channel workgroups hold CUs beside the backward GEMMs (include/bayeslm.h
    blm_gemm_plan_set_cus).  Host-side state of the planner: it affects launches enqueued AFTER the call."""
    calls().blm_gemm_plan_set_cus(int(n))


def get_gemm_cus():
    return int(calls().blm_gemm_plan_get_cus())


def gemm_comm_window(us):
    """A gradient bucket expected to spend ``us`` microseconds on the links has been launched (0: the exchange is over): the
    GEMMs planned while the window is open run beside the collective's channel workgroups and take the plans measured
    there (include/bayeslm.h blm_gemm_plan_comm_window)."""
    calls().blm_gemm_plan_comm_window(float(us))


def get_gemm_mode():
    return ("f32", "bf16x3", "bf16x6")[int(calls().blm_get_gemm_mode())]


def gemm(op, A, B, Cout, M, N, K, lda, ldb, ldc, *, alpha=1.0, accumulate=False, epilogue=L.EPI_NONE, bias=None,
         aux=None, coef=None, var_b=None, C2=None, wg_mu=None, var_c=None, kl_lambda=0.0, kl_inv_n=0.0,
         drop=None, drop_B=0, tag=None, colsum_a=None):
    if _TIMER is not None and (tag is not None or _TIMER.all_gemms) and (_TIMER.only is None or tag in _TIMER.only):
        if _TIMER.all_gemms:
            tag = f"{('NT', 'NN', 'TN')[op]} {M}x{N}x{K} epi{epilogue}{' acc' if accumulate else ''} [{tag or '-'}]"
        ev0, ev1 = _TIMER.bracket(tag)
        ev0.record()
        _gemm(op, A, B, Cout, M, N, K, lda, ldb, ldc, alpha, accumulate, epilogue, bias, aux, coef, var_b, C2, wg_mu,
              var_c, kl_lambda, kl_inv_n, drop, drop_B, colsum_a)
        ev1.record()
        return
    _gemm(op, A, B, Cout, M, N, K, lda, ldb, ldc, alpha, accumulate, epilogue, bias, aux, coef, var_b, C2, wg_mu,
          var_c, kl_lambda, kl_inv_n, drop, drop_B, colsum_a)


def _gemm(op, A, B, Cout, M, N, K, lda, ldb, ldc, alpha, accumulate, epilogue, bias, aux, coef, var_b, C2, wg_mu,
          var_c, kl_lambda, kl_inv_n, drop, drop_B, colsum_a=None):
    L.require_gfx950()
    a = L.GemmArgs()
    a.abi_version = L.ABI_VERSION
    a.op = op
    a.M, a.N, a.K = int(M), int(N), int(K)
    a.A, a.lda = ptr(A), int(lda)
    a.B, a.ldb = ptr(B), int(ldb)
    a.C, a.ldc = ptr(Cout), int(ldc)
    a.alpha = float(alpha)
    a.flags = L.GEMM_ACCUMULATE if accumulate else 0
    a.epilogue = epilogue
    a.bias, a.aux, a.coef = ptr(bias), ptr(aux), ptr(coef)
    if var_b is not None:
        a.var_b = var_b
    a.C2, a.wg_mu = ptr(C2), ptr(wg_mu)
    if var_c is not None:
        a.var_c = var_c
    a.kl_lambda, a.kl_inv_n = float(kl_lambda), float(kl_inv_n)
    if drop is not None and drop.on:
        a.drop_p = float(drop.p)
        a.drop_rng = drop.rng()
        a.drop_B = int(drop_B)
        a.drop_col_offset = int(drop.col_offset)
        a.drop_global_cols = int(drop.global_cols or drop_B)
    a.colsum_a = ptr(colsum_a)
    calls().blm_gemm(C.byref(a), stream())


def _colsum_into(dy2, M, N, out, accumulate=True, ld=None):
    calls().blm_colsum(ptr(dy2), N if ld is None else int(ld), ptr(out), M, N, 1 if accumulate else 0, stream())


# ----------------------------------------------------------------------------
# Linear:  y = x W^T + b      (model.py:876,921,975-977,1306 F.linear call sites)
# ----------------------------------------------------------------------------
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, link=None):
        x = _f32(x, "x")
        N, K = w.shape
        M = x.numel() // K
        if N % 4 and N >= 64:
            # an output width that is not a multiple of 4 (a vocabulary of 33278 words): rows of N floats are not 16-byte aligned,
            # which took this product's epilogue, the cross entropy and BOTH backward products (the logits' gradient is their
            # A operand) off their vector paths -- the headline step 19.9 -> 26.4 ms (tools/shape_cliff_probe.py).  The rows are
            # padded to a multiple of 4 floats instead; what the caller sees is the (..., N) view of that buffer.
            # The product itself runs on a copy of the weight with Np - N zero rows behind it (and a zero-padded bias): every extent
            # a multiple of 4, the padding columns of the output exactly 0.
            y, ldy = _padded_rows(x.shape[:-1], N, x.device)
            pad = torch.nn.functional.pad
            w_p = pad(w.detach(), (0, 0, 0, ldy - N))
            b_p = pad(b.detach(), (0, ldy - N)) if b is not None else None
            gemm(L.GEMM_NT, x, w_p, y, M, ldy, K, K, K, ldy, epilogue=L.EPI_BIAS if b is not None else L.EPI_NONE, bias=b_p)
            ctx.w_p = w_p if (ctx.needs_input_grad[0]) else None
        else:
            y, ldy = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32), N
            gemm(L.GEMM_NT, x, w, y, M, N, K, K, K, ldy, epilogue=L.EPI_BIAS if b is not None else L.EPI_NONE, bias=b)
            ctx.w_p = None
        ctx.save_for_backward(x)
        ctx.w, ctx.b, ctx.link = w, b, link
        if link is not None and ctx.needs_input_grad[0]:
            link.arm(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        w, b = ctx.w, ctx.b
        N, K = w.shape
        M = x.numel() // K
        dy, ldy = _rows2d(dy, N, "dy")  # the padded rows of an odd vocabulary's logits come back as they went out
        Np = (N + 3) // 4 * 4
        # the padded path writes zeros into dy's padding columns: only for storage this module handed out (its own y, the
        # gradient buffer of _CrossEntropy(keep=True)), never for a strided gradient whose "padding" is a sibling's data
        if (N % 4 and N >= 64 and ldy == Np and ctx.link is None and _owns_padded(dy)
                and (dy.storage_offset() + (M - 1) * Np + Np) * 4 <= dy.untyped_storage().nbytes()):
            return _Linear._backward_padded(ctx, x, w, b, dy, M, N, Np, K)
        dx = None
        if ctx.needs_input_grad[0]:
            parked = ctx.link.take(x) if ctx.link is not None else None
            if parked is not None and parked.data_ptr() == dy.data_ptr():
                # this op feeds the LayerNorm directly and no dropout sits between them: the LayerNorm backward hands ONE
                # buffer out as dx and dy, and a GEMM cannot accumulate into its own A operand
                dx = torch.empty_like(x)
                gemm(L.GEMM_NN, dy, w, dx, M, K, N, ldy, K, K)
                dx.add_(parked)
            elif parked is not None:  # residual block: add into the LayerNorm backward's dx (ResidualLink)
                gemm(L.GEMM_NN, dy, w, parked, M, K, N, ldy, K, K, accumulate=True)
                dx = parked
            else:
                dx = torch.empty_like(x)
                dx2 = dx.view(-1, K)
                for r0, r1 in _row_chunks(M, ldy):  # one chunk unless dy is 4 GB or more
                    gemm(L.GEMM_NN, dy[r0:r1], w, dx2[r0:r1], r1 - r0, K, N, ldy, K, K)
        dw = db = None
        fuse_b = w.requires_grad and b is not None and b.requires_grad and _grad_in_place(b)
        if w.requires_grad:
            buf, acc, dw = _wgrad_target(w)
            x2 = x.view(-1, K)
            for r0, r1 in _row_chunks(M, ldy):
                gemm(L.GEMM_TN, dy[r0:r1], x2[r0:r1], buf, N, K, r1 - r0, ldy, K, K, accumulate=acc or r0 > 0,
                     colsum_a=_grad_buf(b) if fuse_b else None)
        if b is not None and b.requires_grad and not fuse_b:
            buf, acc, db = _wgrad_target(b)
            _colsum_into(dy, M, N, buf, accumulate=acc, ld=ldy)
        _notify(w, b)
        return dx, dw, db, None

    @staticmethod
    def _backward_padded(ctx, x, w, b, dy, M, N, Np, K):
        """Backward over the padded layout of an output whose width is not a multiple of 4: dy is the (M, N) window of an
        (M, Np) buffer.  Both products take the whole buffer -- the gradient of the logits is their A operand, and its contiguous
        extent has to be a multiple of 4 for the vector / LDS-DMA loaders -- with the padding columns zeroed (the forward left
        zeros there and the cross entropy writes only real columns, but the buffer may be anybody's) against the zero-row padded
        weight; the weight gradient's padding rows are dropped when it is added to ``w.grad``."""
        full = dy.as_strided((M, Np), (Np, 1))
        full[:, N:].zero_()
        dx = None
        if ctx.needs_input_grad[0]:
            w_p = ctx.w_p if ctx.w_p is not None else torch.nn.functional.pad(w.detach(), (0, 0, 0, Np - N))
            dx = torch.empty_like(x)
            dx2 = dx.view(-1, K)
            for r0, r1 in _row_chunks(M, Np):
                gemm(L.GEMM_NN, full[r0:r1], w_p, dx2[r0:r1], r1 - r0, K, Np, Np, K, K)
        dw = db = None
        want_b = b is not None and b.requires_grad
        if w.requires_grad:
            dw_p = torch.empty(Np, K, device=x.device, dtype=torch.float32)
            db_p = torch.zeros(Np, device=x.device, dtype=torch.float32) if want_b else None
            x2 = x.view(-1, K)
            for r0, r1 in _row_chunks(M, Np):
                gemm(L.GEMM_TN, full[r0:r1], x2[r0:r1], dw_p, Np, K, r1 - r0, Np, K, K, accumulate=r0 > 0, colsum_a=db_p)
            if _grad_in_place(w):
                _grad_buf(w).add_(dw_p[:N])
            else:
                dw = dw_p[:N]
            if want_b:
                if _grad_in_place(b):
                    _grad_buf(b).add_(db_p[:N])
                else:
                    db = db_p[:N]
        elif want_b:
            buf, acc, db = _wgrad_target(b)
            _colsum_into(full, M, N, buf, accumulate=acc, ld=Np)
        _notify(w, b)
        return dx, dw, db, None


def linear(x, w, b=None, link=None):
    w, b = _weight(w, "weight"), _weight(b, "bias")
    if w.dim() != 2 or x.shape[-1] != w.shape[1] or (b is not None and b.numel() != w.shape[0]):
        # the kernels take M = numel / K on trust: a mismatch would read past a buffer instead of raising like F.linear
        raise BayesLMError("linear: input (..., %d) against weight %s%s" % (x.shape[-1], tuple(w.shape),
                                                                            "" if b is None else " and bias %s" % (tuple(b.shape),)))
    return _Linear.apply(x, w, b, link)


# ----------------------------------------------------------------------------
# BayesLinear:  y = x (mu + exp(lgstd) eps)^T   (model.py:1083-1129)
# ----------------------------------------------------------------------------
def sample_weight(mu, lgstd, noise, row_lo=0, srows=None, out=None, kl_out=None, kl_weight=1.0):
    """W = mu (+ noise on rows [row_lo,row_lo+srows)); optional fused KL accumulation into kl_out."""
    L.require_gfx950()
    mu = _f32(mu, "mu")
    rows = mu.shape[0]
    cols = mu.numel() // rows
    if srows is None:
        srows = rows
    v = _variational(lgstd, noise, row_lo, srows)
    if out is None and (noise is not None or kl_out is None):
        out = torch.empty_like(mu)
    calls().blm_sample_weight(ptr(mu), rows, cols, C.byref(v), ptr(out), ptr(kl_out), float(kl_weight), stream())
    return out


class _SampleWeight(torch.autograd.Function):
    """Differentiable materialisation, used where the sampled tensor feeds something other than one
    GEMM (the LSTM stack, bias vectors, the EMB projection)."""

    @staticmethod
    def forward(ctx, mu, lgstd, noise, row_lo):
        W = sample_weight(mu, lgstd, noise, row_lo, lgstd.shape[0])
        ctx.meta = (mu, lgstd, noise, row_lo)
        return W

    @staticmethod
    def backward(ctx, dW):
        mu, lgstd, noise, row_lo = ctx.meta
        dW = _f32(dW, "dW")
        rows = mu.shape[0]
        cols = mu.numel() // rows
        v = _variational(lgstd, noise, row_lo, lgstd.shape[0])
        gmu, _, dmu = _wgrad_target(mu, zero=True) if mu.requires_grad else (None, False, None)
        glg, _, dlg = _wgrad_target(lgstd, zero=True) if lgstd.requires_grad else (None, False, None)
        calls().blm_sample_weight_bwd(ptr(dW), rows, cols, C.byref(v), ptr(gmu), ptr(glg), stream())
        _notify(mu, lgstd)
        return dmu, dlg, None, None


def sampled(mu, lgstd, noise, row_lo=0):
    """W = mu with noise on rows [row_lo, row_lo + lgstd.shape[0]); differentiable w.r.t. mu, lgstd."""
    mu, lgstd = _weight(mu, "mu"), _weight(lgstd, "lgstd")
    if lgstd.dim() < 1 or mu.dim() < 1 or lgstd.shape[1:] != mu.shape[1:] or not 0 <= row_lo <= mu.shape[0] - lgstd.shape[0]:
        raise BayesLMError("sampled: lgstd %s does not fit rows [%d, ...) of mu %s" % (tuple(lgstd.shape), row_lo, tuple(mu.shape)))
    return _SampleWeight.apply(mu, lgstd, noise, row_lo)


class _VarGroup(torch.autograd.Function):
    """Every variational tensor of a module in ONE launch per direction (blm_variational_group_fwd / _bwd): the
    samples W_i, the module's KL term as a by-product of the same pass, and in backward dmu / dlgstd of all items with
    the KL gradient folded in.  ``specs``: (mu, lgstd, noise, row_lo, kl_weight, kl_minus) per item; ``params`` repeats
    the mu / lgstd tensors so that autograd sees them."""

    @staticmethod
    def forward(ctx, specs, *params):
        L.require_gfx950()
        n = len(specs)
        items = (L.VarItem * n)()
        outs = []
        any_kl = any(sp[4] != 0.0 for sp in specs)
        kl = torch.empty((), device=specs[0][0].device, dtype=torch.float32) if any_kl else None
        for it, (mu, lg, noise, row_lo, klw, klm) in zip(items, specs):
            mu, lg = _f32(mu, "mu"), _f32(lg, "lgstd")
            W = torch.empty_like(mu)
            it.mu, it.rows = ptr(mu), mu.shape[0]
            it.cols = mu.numel() // mu.shape[0]
            it.v = _variational(lg, noise, row_lo, lg.shape[0])
            it.w_out, it.kl_weight, it.kl_minus = ptr(W), float(klw), float(klm)
            outs.append(W)
        calls().blm_variational_group_fwd(items, n, ptr(kl), stream())
        ctx.specs = specs
        if kl is None:
            kl = torch.zeros((), device=specs[0][0].device, dtype=torch.float32)
            ctx.mark_non_differentiable(kl)
        return (*outs, kl)

    @staticmethod
    def backward(ctx, *grads):
        specs = ctx.specs
        n = len(specs)
        items = (L.VarItem * n)()
        keep, touched = [], []
        for it, (mu, lg, noise, row_lo, klw, klm), dW in zip(items, specs, grads[:n]):
            if dW is not None:
                dW = _f32(dW, "dW")
                keep.append(dW)
            it.mu, it.rows = ptr(mu), mu.shape[0]
            it.cols = mu.numel() // mu.shape[0]
            it.v = _variational(lg, noise, row_lo, lg.shape[0])
            it.kl_weight, it.kl_minus = float(klw), float(klm)
            it.dw = ptr(dW)
            it.dmu = ptr(_grad_buf(mu)) if mu.requires_grad else None
            it.dlgstd = ptr(_grad_buf(lg)) if lg.requires_grad else None
            touched += [mu, lg]
        g = grads[n]
        if g is not None:
            g = _f32(g.reshape(1), "g")
        calls().blm_variational_group_bwd(items, n, ptr(g), stream())
        _notify(*touched)
        return (None,) * (1 + 2 * n)


def variational_group(specs):
    """specs: [(mu, lgstd, noise, row_lo, kl_weight, kl_minus)] -> ([W_i], kl).  W_i = mu_i with noise on the rows
    [row_lo, row_lo + lgstd.shape[0]); kl = sum_i kl_weight_i * mean_i(mu_s^2 - 2 lgstd + exp(2 lgstd) - kl_minus) / 2
    over the noisy rows (0 when no item carries a weight).  One launch forward, one backward."""
    if len(specs) > L.VAR_GROUP_MAX or any(sp[0].numel() >= 2 ** 31 or sp[2] is None for sp in specs):
        raise BayesLMError("variational_group: at most %d sampled tensors of < 2^31 elements" % L.VAR_GROUP_MAX)
    specs = [(_weight(sp[0], "mu", in_place=True), _weight(sp[1], "lgstd", in_place=True)) + tuple(sp[2:]) for sp in specs]
    flat = []
    for sp in specs:
        flat += [sp[0], sp[1]]
    out = _VarGroup.apply(specs, *flat)
    return list(out[:-1]), out[-1]


class _BayesLinear(torch.autograd.Function):
    """``fused=True``: eps is generated inside the GEMM tile loader (no W in HBM) in forward and
    dgrad; ``fused=False``: one materialisation pass writes W, then plain GEMMs.  The wgrad GEMM's
    epilogue turns dW into (dmu, dlgstd) with eps regenerated from the counter and adds the KL
    gradient scaled by kl_lambda."""

    @staticmethod
    def forward(ctx, x, mu, lgstd, noise, kl_lambda, fused):
        x = _f32(x, "x")
        N, K = mu.shape
        M = x.numel() // K
        y = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
        W = None
        if noise is None:
            gemm(L.GEMM_NT, x, mu, y, M, N, K, K, K, N)
        elif fused:
            gemm(L.GEMM_NT, x, mu, y, M, N, K, K, K, N, var_b=_variational(lgstd, noise, 0, N))
        else:
            W = sample_weight(mu, lgstd, noise)
            gemm(L.GEMM_NT, x, W, y, M, N, K, K, K, N)
        ctx.save_for_backward(x, W)
        ctx.mu, ctx.lgstd, ctx.noise, ctx.kl_lambda, ctx.fused = mu, lgstd, noise, kl_lambda, fused
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        mu, lgstd, noise = ctx.mu, ctx.lgstd, ctx.noise
        dy = _f32(dy, "dy")
        N, K = mu.shape
        M = x.numel() // K
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            if noise is None:
                gemm(L.GEMM_NN, dy, mu, dx, M, K, N, N, K, K)
            elif ctx.fused:
                gemm(L.GEMM_NN, dy, mu, dx, M, K, N, N, K, K, var_b=_variational(lgstd, noise, 0, N))
            else:
                gemm(L.GEMM_NN, dy, W, dx, M, K, N, N, K, K)
        dmu = dlg = None
        if mu.requires_grad:
            gmu, _, dmu = _wgrad_target(mu, zero=True)
            if noise is None:  # eval-mode graph: only the mean gets a gradient
                gemm(L.GEMM_TN, dy, x, gmu, N, K, M, N, K, K, accumulate=True)
            else:
                glg, _, dlg = _wgrad_target(lgstd, zero=True) if lgstd.requires_grad else (
                    torch.zeros(lgstd.shape, device=lgstd.device, dtype=torch.float32), False, None)
                gemm(L.GEMM_TN, dy, x, gmu, N, K, M, N, K, K, accumulate=True,
                     epilogue=L.EPI_BAYES_WGRAD, C2=glg, wg_mu=mu,
                     var_c=_variational(lgstd, noise, 0, N), kl_lambda=ctx.kl_lambda, kl_inv_n=1.0 / (N * K))
                _notify(lgstd)
            _notify(mu)
        return dx, dmu, dlg, None, None, None


def bayes_linear(x, mu, lgstd, noise=None, kl_lambda=0.0, fused=False):
    mu, lgstd = _weight(mu, "mu"), _weight(lgstd, "lgstd")
    if x.shape[-1] != mu.shape[-1] or mu.dim() != 2 or lgstd.shape != mu.shape:
        raise BayesLMError("bayes_linear: input (..., %d) against mu %s and lgstd %s" % (x.shape[-1], tuple(mu.shape), tuple(lgstd.shape)))
    if fused and (mu.shape[1] % 4 or (mu.data_ptr() | lgstd.data_ptr()) % 16
                  or (noise is not None and noise.eps is not None and noise.eps.data_ptr() % 16)):
        fused = False  # the in-loader sampling reads float4s: misaligned operands take the materialising kernels, same numbers
    return _BayesLinear.apply(x, mu, lgstd, noise, kl_lambda, fused)


# ----------------------------------------------------------------------------
# BayesLinear under local reparameterisation (opt-in, no reference counterpart):
#   y = x mu^T + sqrt(x^2 (sigma^2)^T) * zeta,  zeta ~ N(0,1) per (row, column)
# ----------------------------------------------------------------------------
@dataclass
class LrtNoise:
    """Where zeta of `bayes_linear_lrt` comes from: an injected (M, N) tensor (parity tests) or the Philox stream
    (seed, STREAM_LRT + site, step), keyed by the global batch column like a dropout mask (Drop)."""
    eps: torch.Tensor = None
    seed: int = 0
    site: int = 0
    step: int = 0
    col_offset: int = 0
    global_cols: int = 0

    def rng(self):
        return L.rng(self.seed, L.STREAM_LRT + self.site, self.step)


_ONES = {}


def _one(device):
    """A device scalar 1.0: the upstream gradient blm_kl_mean_bwd reads when the KL term is folded into a layer's backward."""
    t = _ONES.get(device)
    if t is None:
        t = _ONES[device] = torch.ones(1, device=device, dtype=torch.float32)
    return t


def _lrt_prepare(src, mode):
    dst = torch.empty_like(src)
    calls().blm_lrt_prepare(ptr(src), ptr(dst), src.numel(), mode, stream())
    return dst


def _lrt_mul(out, a, b, scale=1.0, accumulate=False):
    calls().blm_lrt_mul(ptr(out), ptr(a), ptr(b), out.numel(), float(scale), 1 if accumulate else 0, stream())


class _BayesLinearLRT(torch.autograd.Function):
    """m = x mu^T and v = x^2 (sigma^2)^T are two products of the GEMM family; one combine pass turns them into
    y = m + sqrt(v) * zeta in place with zeta generated in registers and keeps s = sqrt(v).  Backward regenerates zeta in the
    pass that forms q = dy zeta / (2 s) (0 where s == 0), then dmu += dy^T x, dlgstd += 2 sigma^2 * (q^T x^2) and
    dx = dy mu + 2 x * (q sigma^2).  sigma^2 = exp(2 lgstd) is formed once in forward and kept (N x K, a weight's size);
    x^2 is formed again in backward instead of being kept: a second M x K activation held from forward to backward would
    cost more than the one streaming pass that rebuilds it.  No sampled W exists at any point.  The KL gradient, scaled by
    kl_lambda, is blm_kl_mean_bwd's: what BLM_EPI_BAYES_WGRAD adds on the weight-sampling path."""

    @staticmethod
    def forward(ctx, x, mu, lgstd, noise, kl_lambda):
        L.require_gfx950()
        x = _f32(x, "x")
        N, K = mu.shape
        M = x.numel() // K
        B = x.shape[-2] if x.dim() >= 2 else 1
        sig2 = _lrt_prepare(lgstd.detach(), 1)
        x2 = _lrt_prepare(x, 0)
        y = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
        s = torch.empty(M, N, device=x.device, dtype=torch.float32)
        gemm(L.GEMM_NT, x, mu, y, M, N, K, K, K, N, tag="lrt_mean_fwd")
        gemm(L.GEMM_NT, x2, sig2, s, M, N, K, K, K, N, tag="lrt_var_fwd")
        ctx.key = (M // B if B else 0, B, N, int(noise.col_offset), int(noise.global_cols))
        calls().blm_lrt_combine(ptr(y), ptr(s), ptr(noise.eps), C.byref(noise.rng()), *ctx.key, stream())
        ctx.save_for_backward(x, s, sig2)
        ctx.mu, ctx.lgstd, ctx.noise, ctx.kl_lambda = mu, lgstd, noise, kl_lambda
        return y

    @staticmethod
    def backward(ctx, dy):
        x, s, sig2 = ctx.saved_tensors
        mu, lgstd, noise, kl_lambda = ctx.mu, ctx.lgstd, ctx.noise, ctx.kl_lambda
        dy = _f32(dy, "dy")
        N, K = mu.shape
        M = x.numel() // K
        q = torch.empty_like(s)
        calls().blm_lrt_bwd_factor(ptr(dy), ptr(s), ptr(q), ptr(noise.eps), C.byref(noise.rng()), *ctx.key, stream())
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            gemm(L.GEMM_NN, q, sig2, dx, M, K, N, N, K, K, tag="lrt_var_dgrad")
            _lrt_mul(dx, dx, x, 2.0)
            gemm(L.GEMM_NN, dy, mu, dx, M, K, N, N, K, K, accumulate=True, tag="lrt_mean_dgrad")
        dmu = dlg = gmu = glg = None
        if mu.requires_grad:
            gmu, _, dmu = _wgrad_target(mu, zero=True)
            gemm(L.GEMM_TN, dy, x, gmu, N, K, M, N, K, K, accumulate=True, tag="lrt_mean_wgrad")
        if lgstd.requires_grad:
            glg, _, dlg = _wgrad_target(lgstd, zero=True)
            t = torch.empty_like(sig2)
            gemm(L.GEMM_TN, q, _lrt_prepare(x, 0), t, N, K, M, N, K, K, tag="lrt_var_wgrad")
            _lrt_mul(glg, t, sig2, 2.0, accumulate=True)
        if kl_lambda != 0.0 and (gmu is not None or glg is not None):
            # the kernel writes both gradients; a tensor that does not require one gets a scratch buffer
            calls().blm_kl_mean_bwd(ptr(mu), K, ptr(lgstd), N, K, ptr(_one(x.device)), float(kl_lambda),
                                    ptr(gmu if gmu is not None else torch.zeros_like(mu)), K,
                                    ptr(glg if glg is not None else torch.zeros_like(lgstd)), stream())
        _notify(mu, lgstd)
        return dx, dmu, dlg, None, None


def bayes_linear_lrt(x, mu, lgstd, noise, kl_lambda=0.0):
    """BayesLinear under local reparameterisation.  ``noise``: an `LrtNoise` (never None: eval mode is `bayes_linear`);
    x is seen as (..., B, K), and zeta's Philox stream is keyed by the global batch column col_offset + b."""
    mu, lgstd = _weight(mu, "mu"), _weight(lgstd, "lgstd")
    if x.shape[-1] != mu.shape[-1] or mu.dim() != 2 or lgstd.shape != mu.shape:
        raise BayesLMError("bayes_linear_lrt: input (..., %d) against mu %s and lgstd %s" % (x.shape[-1], tuple(mu.shape), tuple(lgstd.shape)))
    if not isinstance(noise, LrtNoise):
        raise BayesLMError("bayes_linear_lrt: noise must be an ops.LrtNoise, got %s (mean weights: bayes_linear)" % type(noise).__name__)
    M, N = x.numel() // max(mu.shape[1], 1), mu.shape[0]
    B = x.shape[-2] if x.dim() >= 2 else 1
    e = noise.eps
    if e is not None and not (torch.is_tensor(e) and e.is_cuda and e.dtype == torch.float32 and e.is_contiguous() and e.numel() == M * N):
        # an injected zeta is read by the kernels with y's extent on trust: a wrong shape would read past it
        raise BayesLMError("bayes_linear_lrt: injected zeta must be a contiguous fp32 GPU tensor with the output's %d x %d elements, got %s"
                           % (M, N, (tuple(e.shape), e.dtype, e.device) if torch.is_tensor(e) else type(e)))
    if noise.col_offset < 0 or (noise.global_cols and noise.col_offset + B > noise.global_cols) or (not noise.global_cols and noise.col_offset):
        raise BayesLMError("bayes_linear_lrt: batch columns [%d, %d) do not fit a global batch of %d columns"
                           % (noise.col_offset, noise.col_offset + B, noise.global_cols or B))
    return _BayesLinearLRT.apply(x, mu, lgstd, noise, kl_lambda)


# ----------------------------------------------------------------------------
# FFN:  y = lin2(drop(gelu(x W1^T + b1)))        (model.py:1043, 1169)
# lin2 is nn.Linear (w2, b2) or BayesLinear (mu2, lgstd2, no bias).
# ----------------------------------------------------------------------------
class _FFN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, lgstd2, noise, kl_lambda, fused, drop, link=None):
        ctx.link = link
        x = _f32(x, "x")
        if link is not None and ctx.needs_input_grad[0]:
            link.arm(x)
        F_, D = w1.shape  # (ff, d)
        N2 = w2.shape[0]
        M = x.numel() // D
        B = x.shape[-2] if x.dim() >= 2 else 1
        need_bwd = any(ctx.needs_input_grad)  # forward itself runs with grad mode off
        z = torch.empty(M, F_, device=x.device, dtype=torch.float32) if need_bwd else None
        h = torch.empty(M, F_, device=x.device, dtype=torch.float32)
        gemm(L.GEMM_NT, x, w1, h, M, F_, D, D, D, F_, epilogue=L.EPI_BIAS_GELU, bias=b1, aux=z, drop=drop, drop_B=B,
             tag="ffn_linear1_fwd")
        y = torch.empty(*x.shape[:-1], N2, device=x.device, dtype=torch.float32)
        W = None
        bayes = lgstd2 is not None
        if bayes and noise is not None:
            if fused:
                gemm(L.GEMM_NT, h, w2, y, M, N2, F_, F_, F_, N2, var_b=_variational(lgstd2, noise, 0, N2),
                     tag="sampled_gemm_fwd")
            else:
                W = sample_weight(w2, lgstd2, noise)
                gemm(L.GEMM_NT, h, W, y, M, N2, F_, F_, F_, N2, tag="sampled_gemm_fwd")
        else:
            gemm(L.GEMM_NT, h, w2, y, M, N2, F_, F_, F_, N2,
                 epilogue=L.EPI_BIAS if b2 is not None else L.EPI_NONE, bias=b2)
        ctx.save_for_backward(x, z, h, W)
        ctx.p = (w1, b1, w2, b2, lgstd2, noise, kl_lambda, fused, drop, B)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, z, h, W = ctx.saved_tensors
        w1, b1, w2, b2, lgstd2, noise, kl_lambda, fused, drop, B = ctx.p
        dy = _f32(dy, "dy")
        F_, D = w1.shape
        N2 = w2.shape[0]
        M = x.numel() // D
        bayes = lgstd2 is not None and noise is not None
        # dz = (dy W2) * [gelu'(z) * keep]: the bracket was written by the forward epilogue (aux)
        dz = torch.empty(M, F_, device=x.device, dtype=torch.float32)
        if bayes and fused:
            gemm(L.GEMM_NN, dy, w2, dz, M, F_, N2, N2, F_, F_, epilogue=L.EPI_MUL_DGELU, aux=z,
                 var_b=_variational(lgstd2, noise, 0, N2), tag="sampled_gemm_dgrad")
        else:
            gemm(L.GEMM_NN, dy, W if bayes else w2, dz, M, F_, N2, N2, F_, F_, epilogue=L.EPI_MUL_DGELU, aux=z,
                 tag="sampled_gemm_dgrad" if bayes else None)
        # linear2 weight gradients
        if w2.requires_grad:
            if bayes:
                gemm(L.GEMM_TN, dy, h, _grad_buf(w2), N2, F_, M, N2, F_, F_, accumulate=True,
                     epilogue=L.EPI_BAYES_WGRAD, C2=_grad_buf(lgstd2), wg_mu=w2,
                     var_c=_variational(lgstd2, noise, 0, N2), kl_lambda=kl_lambda, kl_inv_n=1.0 / (N2 * F_),
                     tag="sampled_gemm_wgrad")
            else:
                gemm(L.GEMM_TN, dy, h, _grad_buf(w2), N2, F_, M, N2, F_, F_, accumulate=True,
                     colsum_a=_grad_buf(b2) if (b2 is not None and b2.requires_grad) else None)
        elif b2 is not None and b2.requires_grad:
            _colsum_into(dy, M, N2, _grad_buf(b2))
        _notify(w2, b2, lgstd2 if bayes else None)
        return (_ffn_linear1_backward(ctx, x, dz, w1, b1),) + (None,) * 10


def _ffn_linear1_backward(ctx, x, dz, w1, b1):
    """The first linear's half of a feed-forward backward, given dz (M, ff): w1 / b1 gradients in place, dx returned."""
    F_, D = w1.shape
    M = x.numel() // D
    # linear1 (bias gradient = column sums of dz, taken inside the wgrad GEMM)
    if w1.requires_grad:
        gemm(L.GEMM_TN, dz, x, _grad_buf(w1), F_, D, M, F_, D, D, accumulate=True,
             colsum_a=_grad_buf(b1) if b1.requires_grad else None)
    elif b1.requires_grad:
        _colsum_into(dz, M, F_, _grad_buf(b1))
    _notify(w1, b1)
    dx = None
    if ctx.needs_input_grad[0]:
        parked = ctx.link.take(x) if ctx.link is not None else None
        if parked is not None:
            gemm(L.GEMM_NN, dz, w1, parked, M, D, F_, F_, D, D, accumulate=True)
            dx = parked
        else:
            dx = torch.empty_like(x)
            gemm(L.GEMM_NN, dz, w1, dx, M, D, F_, F_, D, D)
    return dx


def ffn(x, w1, b1, w2, b2=None, lgstd2=None, noise=None, kl_lambda=0.0, fused=False, drop=NO_DROP, link=None):
    w1, b1, w2, b2, lgstd2 = (_weight(t, n, in_place=True) for t, n in ((w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2"), (lgstd2, "lgstd2")))
    return _FFN.apply(x, w1, b1, w2, b2, lgstd2, noise, kl_lambda, fused, drop, link)


class _FFNLinear1(torch.autograd.Function):
    """h = drop(gelu(x W1^T + b1)) on its own: the first product of `_FFN` with the same bias + GELU + dropout epilogue, for a
    feed-forward whose second linear cannot be part of the one fused function (`ffn_lrt`).  Backward multiplies the incoming
    dh by the factor the epilogue left (GELU' and keep mask) in one elementwise pass where `_FFN` has it in a GEMM epilogue."""

    @staticmethod
    def forward(ctx, x, w1, b1, drop, link):
        ctx.link = link
        x = _f32(x, "x")
        if link is not None and ctx.needs_input_grad[0]:
            link.arm(x)
        F_, D = w1.shape
        M = x.numel() // D
        B = x.shape[-2] if x.dim() >= 2 else 1
        z = torch.empty(M, F_, device=x.device, dtype=torch.float32) if any(ctx.needs_input_grad) else None
        h = torch.empty(*x.shape[:-1], F_, device=x.device, dtype=torch.float32)
        gemm(L.GEMM_NT, x, w1, h, M, F_, D, D, D, F_, epilogue=L.EPI_BIAS_GELU, bias=b1, aux=z, drop=drop, drop_B=B,
             tag="ffn_linear1_fwd")
        ctx.save_for_backward(x, z)
        ctx.p = (w1, b1)
        return h

    @staticmethod
    def backward(ctx, dh):
        x, z = ctx.saved_tensors
        w1, b1 = ctx.p
        dh = _f32(dh, "dh")
        dz = torch.empty_like(z)
        _lrt_mul(dz, dh, z)
        return _ffn_linear1_backward(ctx, x, dz, w1, b1), None, None, None, None


def ffn_lrt(x, w1, b1, mu2, lgstd2, noise, kl_lambda=0.0, drop=NO_DROP, link=None):
    """`ffn` with a Bayesian second linear under local reparameterisation: `_FFNLinear1`, then `bayes_linear_lrt`."""
    w1, b1 = _weight(w1, "w1", in_place=True), _weight(b1, "b1", in_place=True)
    return bayes_linear_lrt(_FFNLinear1.apply(x, w1, b1, drop, link), mu2, lgstd2, noise, kl_lambda)


class _FFNGP(torch.autograd.Function):
    """y = lin2(drop(sum_i act_i(x Wg^T + bg) coef[i]))   GaussTransformerEncoderLayer FFN
    (model.py:2283): GPNN replaces GELU(linear1(x)); acts = tanh, sigmoid, relu, gelu (model.py:2263)."""

    @staticmethod
    def forward(ctx, x, wg, bg, coef, w2, b2, drop, link=None):
        ctx.link = link
        x = _f32(x, "x")
        if link is not None and ctx.needs_input_grad[0]:
            link.arm(x)
        F_, D = wg.shape
        N2 = w2.shape[0]
        M = x.numel() // D
        B = x.shape[-2]
        z = torch.empty(M, F_, device=x.device, dtype=torch.float32) if any(ctx.needs_input_grad) else None
        h = torch.empty(M, F_, device=x.device, dtype=torch.float32)
        gemm(L.GEMM_NT, x, wg, h, M, F_, D, D, D, F_, epilogue=L.EPI_GP_MIX, bias=bg, aux=z, coef=coef, drop=drop, drop_B=B)
        y = torch.empty(*x.shape[:-1], N2, device=x.device, dtype=torch.float32)
        gemm(L.GEMM_NT, h, w2, y, M, N2, F_, F_, F_, N2, epilogue=L.EPI_BIAS, bias=b2)
        ctx.save_for_backward(x, z, h)
        ctx.p = (wg, bg, coef, w2, b2, drop, B)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, z, h = ctx.saved_tensors
        wg, bg, coef, w2, b2, drop, B = ctx.p
        dy = _f32(dy, "dy")
        F_, D = wg.shape
        N2 = w2.shape[0]
        M = x.numel() // D
        dz = torch.empty(M, F_, device=x.device, dtype=torch.float32)
        dhk = torch.empty(M, F_, device=x.device, dtype=torch.float32) if coef.requires_grad else None
        gemm(L.GEMM_NN, dy, w2, dz, M, F_, N2, N2, F_, F_, epilogue=L.EPI_MUL_DGP_MIX, aux=z, coef=coef, C2=dhk,
             drop=drop, drop_B=B)
        # wg / bg / coef are the leaf mean tensors, or -- GPNN.sample raised -- sampled (non-leaf) ones whose gradients go
        # back to the sampling node (ops.variational_group: d mean, d lgstd = dW eps sigma in one launch)
        dwg = dbg = dcoef = None
        if coef.requires_grad:
            buf, acc, dcoef = _wgrad_target(coef)
            if not acc:
                buf.zero_()
            calls().blm_gp_coef_grad(ptr(dhk), ptr(z), ptr(buf), M, F_, stream())
        if w2.requires_grad:
            gemm(L.GEMM_TN, dy, h, _grad_buf(w2), N2, F_, M, N2, F_, F_, accumulate=True)
        if b2.requires_grad:
            _colsum_into(dy, M, N2, _grad_buf(b2))
        if wg.requires_grad:
            buf, acc, dwg = _wgrad_target(wg)
            gemm(L.GEMM_TN, dz, x, buf, F_, D, M, F_, D, D, accumulate=acc)
        if bg.requires_grad:
            buf, acc, dbg = _wgrad_target(bg)
            _colsum_into(dz, M, F_, buf, accumulate=acc)
        _notify(coef, w2, b2, wg, bg)
        dx = None
        if ctx.needs_input_grad[0]:
            parked = ctx.link.take(x) if ctx.link is not None else None
            if parked is not None:
                gemm(L.GEMM_NN, dz, wg, parked, M, D, F_, F_, D, D, accumulate=True)
                dx = parked
            else:
                dx = torch.empty_like(x)
                gemm(L.GEMM_NN, dz, wg, dx, M, D, F_, F_, D, D)
        return dx, dwg, dbg, dcoef, None, None, None, None


def ffn_gp(x, wg, bg, coef, w2, b2, drop=NO_DROP, link=None):
    wg, bg, coef = _weight(wg, "wg"), _weight(bg, "bg"), _weight(coef, "coef")  # gradients through _wgrad_target
    w2, b2 = _weight(w2, "w2", in_place=True), _weight(b2, "b2", in_place=True)
    return _FFNGP.apply(x, wg, bg, coef, w2, b2, drop, link)


# ----------------------------------------------------------------------------
# causal self-attention core on packed or separate q/k/v   (model.py:889-920)
# ----------------------------------------------------------------------------
class _Attention(torch.autograd.Function):
    """Packed: qkv (T,B,3d) = [q|k|v] from one qkv_net GEMM (model.py:876); separate: three (T,B,d)
    tensors (BayesMultiheadAttention, model.py:975-977).  One input / one gradient tensor in the
    packed case, so autograd never splits or re-concatenates the 3d-wide activation."""

    @staticmethod
    def forward(ctx, a, k, v, nhead, drop):
        a = _f32(a, "qkv")
        packed = k is None
        if packed:
            T, B, d3 = a.shape
            d = d3 // 3
            q, kk, vv, ld = a, a[..., d:], a[..., 2 * d:], d3
        else:
            T, B, d = a.shape
            q, kk, vv, ld = a, _f32(k, "k"), _f32(v, "v"), d
        hd = d // nhead
        out = torch.empty(T, B, d, device=a.device, dtype=torch.float32)
        lse = torch.empty(B * nhead, T, device=a.device, dtype=torch.float32)
        L.require_gfx950()
        r = drop.rng() if drop.on else None
        if drop.keep is not None:  # the mask itself (torch's CPU dropout drew it): the vector-ALU kernels read it
            keep = _f32(drop.keep, "keep")
            if keep.numel() != (drop.global_cols or B) * nhead * T * T or not keep.is_contiguous():
                raise BayesLMError("attention: keep mask must be (global_cols * nhead, T, T) contiguous")
            calls().blm_attn_fwd_keep(q.data_ptr(), kk.data_ptr(), vv.data_ptr(), ld, ptr(out), ptr(lse), T, B, nhead, hd,
                                      ptr(keep), drop.col_offset, drop.global_cols or B, stream())
        else:
            calls().blm_attn_fwd(q.data_ptr(), kk.data_ptr(), vv.data_ptr(), ld, ptr(out), ptr(lse), T, B, nhead, hd,
                                 float(drop.p), C.byref(r) if r is not None else None, drop.col_offset,
                                 drop.global_cols or B, stream())
        ctx.save_for_backward(q, kk if not packed else None, vv if not packed else None, out, lse)
        ctx.meta = (nhead, drop, packed, d)
        return out

    @staticmethod
    def backward(ctx, dout):
        a, k, v, out, lse = ctx.saved_tensors
        nhead, drop, packed, d = ctx.meta
        T, B = a.shape[0], a.shape[1]
        dout = _f32(dout, "dout")
        if packed:
            q, kk, vv, ld = a, a[..., d:], a[..., 2 * d:], 3 * d
            dqkv = torch.empty(T, B, 3 * d, device=a.device, dtype=torch.float32)
            dq, dk, dv, ldd = dqkv, dqkv[..., d:], dqkv[..., 2 * d:], 3 * d
        else:
            q, kk, vv, ld = a, k, v, d
            dq, dk, dv = (torch.empty(T, B, d, device=a.device, dtype=torch.float32) for _ in range(3))
            ldd = d
        if drop.keep is not None:
            calls().blm_attn_bwd_keep(q.data_ptr(), kk.data_ptr(), vv.data_ptr(), ld, ptr(out), ptr(dout), ptr(lse),
                                      dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ldd, T, B, nhead, d // nhead,
                                      ptr(drop.keep), drop.col_offset, drop.global_cols or B, stream())
            return (dqkv, None, None, None, None) if packed else (dq, dk, dv, None, None)
        r = drop.rng() if drop.on else None
        # scratch for dS (B*nhead, T, T): the dK/dV kernel leaves it there, dQ = dS K needs no second recomputation
        nws = int(calls().blm_attn_bwd_ws_floats(T, B, nhead, d // nhead)) if _ATTN_WS else 0
        ws = torch.empty(nws, device=a.device, dtype=torch.float32) if nws > 0 else None
        calls().blm_attn_bwd_ws(q.data_ptr(), kk.data_ptr(), vv.data_ptr(), ld, ptr(out), ptr(dout), ptr(lse),
                                dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ldd, T, B, nhead, d // nhead,
                                float(drop.p), C.byref(r) if r is not None else None, drop.col_offset,
                                drop.global_cols or B, ptr(ws), nws, stream())
        if packed:
            return dqkv, None, None, None, None
        return dq, dk, dv, None, None


_ATTN_WS = os.environ.get("BLM_ATTN_WS", "1") != "0"  # 0: the two-recomputation backward (A/B measurements)


def attention(qkv, nhead, drop=NO_DROP):
    """Causal self-attention core on packed (T,B,3d) projections."""
    return _Attention.apply(qkv, None, None, nhead, drop)


def attention_qkv(q, k, v, nhead, drop=NO_DROP):
    """Same, on three separate (T,B,d) projections."""
    return _Attention.apply(q, k, v, nhead, drop)


# ----------------------------------------------------------------------------
# out = LayerNorm(x + drop(y))      (model.py:1041-1042, 1044-1045)
# ----------------------------------------------------------------------------
class _AddDropLN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, gamma, beta, eps, drop, link=None):
        x, y = _f32(x, "x"), _f32(y, "y")
        ctx.link = link if (link is not None and link.joins(x)) else None
        D = x.shape[-1]
        B = x.shape[-2]
        rows = x.numel() // (B * D)
        out = torch.empty_like(x)
        s = torch.empty_like(x)
        mean = torch.empty(rows * B, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        L.require_gfx950()
        r = drop.rng() if drop.on else None
        calls().blm_add_dropout_ln_fwd(ptr(x), ptr(y), ptr(gamma), ptr(beta), ptr(out), ptr(s), ptr(mean), ptr(rstd),
                                       rows, B, D, float(eps), float(drop.p), C.byref(r) if r is not None else None,
                                       drop.col_offset, drop.global_cols or B, stream())
        ctx.save_for_backward(s, mean, rstd)
        ctx.meta = (gamma, beta, drop, rows, B, D)
        return out

    @staticmethod
    def backward(ctx, dout):
        s, mean, rstd = ctx.saved_tensors
        gamma, beta, drop, rows, B, D = ctx.meta
        dout = _f32(dout, "dout")
        dx = torch.empty_like(s)
        dy = torch.empty_like(s) if drop.on else None
        ws = torch.empty(int(calls().blm_ln_bwd_ws_floats(rows * B, D)), device=s.device, dtype=torch.float32)
        r = drop.rng() if drop.on else None
        # frozen LayerNorm parameters (architect step): their sums land in a scratch row instead of .grad; a parameter that is not
        # the caller's contiguous leaf gets its sums back through autograd (the kernel accumulates: zeroed buffers)
        dgamma, _, rgamma = _wgrad_target(gamma, zero=True) if gamma.requires_grad else (torch.zeros_like(gamma), False, None)
        dbeta, _, rbeta = _wgrad_target(beta, zero=True) if beta.requires_grad else (torch.zeros_like(beta), False, None)
        calls().blm_add_dropout_ln_bwd(ptr(dout), ptr(s), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dy),
                                       ptr(dgamma), ptr(dbeta), ptr(ws), rows, B, D,
                                       float(drop.p), C.byref(r) if r is not None else None, drop.col_offset,
                                       drop.global_cols or B, stream())
        _notify(gamma, beta)
        dres = dx
        if ctx.link is not None and ctx.needs_input_grad[0]:
            ctx.link.dx = dx  # the branch's first op completes this buffer and returns it as ITS dx (ResidualLink)
            dres = None
        return dres, (dy if dy is not None else dx), rgamma, rbeta, None, None, None


def add_dropout_ln(x, y, gamma, beta, eps=1e-5, drop=NO_DROP, link=None):
    gamma, beta = _weight(gamma, "gamma"), _weight(beta, "beta")
    if gamma.numel() != x.shape[-1] or beta.numel() != x.shape[-1] or x.shape != y.shape:
        raise BayesLMError("add_dropout_ln: x %s, y %s, gamma %s, beta %s" % (tuple(x.shape), tuple(y.shape), tuple(gamma.shape),
                                                                             tuple(beta.shape)))
    return _AddDropLN.apply(x, y, gamma, beta, eps, drop, link)


# ----------------------------------------------------------------------------
# embedding (+ sqrt(d) scale + positional table + dropout)   (model.py:1284,116-117,218)
# ----------------------------------------------------------------------------
class _Embed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, weight, pe, scale, drop):
        ids = dev_tensor(ids, "ids", torch.int64)
        T, B = ids.shape
        V, D = weight.shape
        if pe is not None and pe.shape[0] < T:
            raise BayesLMError("sequence length %d exceeds the positional table (%d)" % (T, pe.shape[0]))
        out = torch.empty(T, B, D, device=weight.device, dtype=torch.float32)
        L.require_gfx950()
        r = drop.rng() if drop.on else None
        calls().blm_embed_fwd(ptr(ids), ptr(weight), ptr(pe), ptr(out), T, B, D, V, float(scale), float(drop.p),
                              C.byref(r) if r is not None else None, drop.col_offset, drop.global_cols or B,
                              stream())
        ctx.save_for_backward(ids)
        ctx.meta = (weight, scale, drop)
        return out

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        weight, scale, drop = ctx.meta
        if weight.requires_grad:
            dy = _f32(dy, "dy")
            T, B = ids.shape
            V, D = weight.shape
            r = drop.rng() if drop.on else None
            sink = _EMBED_SINK(weight, ids) if (_EMBED_SINK is not None and _grad_in_place(weight)) else None
            if sink is not None:
                buf, slots, nrows, done = sink
                calls().blm_embed_bwd(ptr(slots), ptr(dy), ptr(buf), T, B, D, int(nrows), float(scale),
                                      float(drop.p), C.byref(r) if r is not None else None, drop.col_offset,
                                      drop.global_cols or B, stream())
                done()
                return None, None, None, None, None
            gw, _, dw = _wgrad_target(weight, zero=True)
            calls().blm_embed_bwd(ptr(ids), ptr(dy), ptr(gw), T, B, D, V, float(scale),
                                  float(drop.p), C.byref(r) if r is not None else None, drop.col_offset,
                                  drop.global_cols or B, stream())
            _notify(weight)
            return None, dw, None, None, None
        return None, None, None, None, None


def _pe_table(pe, D):
    """The positional table guard: (max_len, D) fp32 on the GPU, and fixed -- its gradient is not computed, so a table that
    requires grad is refused rather than silently left without one."""
    if pe is None:
        return None
    if pe.requires_grad and torch.is_grad_enabled():
        raise BayesLMError("the positional table is a fixed buffer here: a pe that requires grad gets no gradient (detach it)")
    pe = _weight(pe, "pe")
    if pe.dim() != 2 or pe.shape[1] != D:
        raise BayesLMError("positional table must be (max_len, %d), got %s" % (D, tuple(pe.shape)))
    return pe


def embed(ids, weight, pe=None, scale=1.0, drop=NO_DROP):
    weight = _weight(weight, "weight")
    if weight.dim() != 2:
        raise BayesLMError("embed: weight must be (V, D), got %s" % (tuple(weight.shape),))
    pe = _pe_table(pe, weight.shape[1])
    return _Embed.apply(ids, weight, pe, scale, drop)


class _AddPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pe, drop):
        x = _f32(x, "x")
        T, B, D = x.shape
        if pe.shape[0] < T:
            raise BayesLMError("sequence length %d exceeds the positional table (%d)" % (T, pe.shape[0]))
        out = torch.empty_like(x)
        L.require_gfx950()
        r = drop.rng() if drop.on else None
        calls().blm_add_pe_dropout(ptr(x), ptr(pe), ptr(out), T, B, D, float(drop.p),
                                   C.byref(r) if r is not None else None, drop.col_offset, drop.global_cols or B,
                                   stream())
        ctx.drop = drop
        return out

    @staticmethod
    def backward(ctx, dy):
        dy = _f32(dy, "dy")
        return (_dropout_apply(dy, ctx.drop) if ctx.drop.on else dy), None, None


def add_pe(x, pe, drop=NO_DROP):
    """drop(x + pe[:T]) with pe a (max_len, D) table (model.py:116-117)."""
    pe = _pe_table(pe, x.shape[-1])
    return _AddPE.apply(x, pe, drop)


# ----------------------------------------------------------------------------
# dropout on a (rows, B, D) activation  (model.py:220 etc.)
# ----------------------------------------------------------------------------
class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, drop):
        x = _f32(x, "x")
        ctx.drop = drop
        return _dropout_apply(x, drop)

    @staticmethod
    def backward(ctx, dy):
        return _dropout_apply(_f32(dy, "dy"), ctx.drop), None


def _dropout_apply(x, drop, row0=0, out=None):
    """``row0``: x is the block of rows [row0, row0 + rows) of a longer (T, B, D) tensor and gets THAT block's mask."""
    D = x.shape[-1]
    B = x.shape[-2] if x.dim() >= 2 else 1
    if x.numel() == 0:
        raise BayesLMError("dropout: empty tensor %s" % (tuple(x.shape),))
    rows = x.numel() // (B * D)
    y = torch.empty_like(x) if out is None else out
    L.require_gfx950()
    r = drop.rng()
    calls().blm_dropout_rows(ptr(x), ptr(y), rows, int(row0), B, D, float(drop.p), C.byref(r), drop.col_offset, drop.global_cols or B, stream())
    return y


def dropout(x, drop):
    if not drop.on:
        return x
    return _Dropout.apply(x, drop)


# ----------------------------------------------------------------------------
# cross entropy (mean over M tokens) on materialised logits  (train.py:233,332)
# ----------------------------------------------------------------------------
class _CrossEntropy(torch.autograd.Function):
    """unit_grad=True (the trainer's case, loss = CE + KL with coefficient 1, train.py:412): the
    forward pass over the logits also overwrites them in place with d(mean NLL)/d(logits), and
    backward returns that buffer untouched.  unit_grad=False: forward keeps lse, backward runs the
    gradient kernel with the real upstream scalar.  Either way the logits buffer is consumed -- unless
    ``keep`` (the `Logits` short cut of an unchanged torch loop): the logits stay the caller's, are saved through
    autograd (an in-place edit between the loss and backward() raises, as torch's own loss would), the gradient gets
    its own buffer, and the mean is torch's: over the rows whose target is not ignore_index (-100), which get neither
    loss nor gradient (the kernels give any row without a target in [0, V) a zero NLL and a zero gradient row)."""

    @staticmethod
    def forward(ctx, logits, targets, unit_grad, keep=False):
        V = logits.shape[-1]
        whole = logits                      # what autograd gets back as the gradient in the fused form: the caller's tensor ...
        logits, ld = _rows2d(logits, V, "logits")  # rows padded to 4 floats (odd vocabulary, ops._Linear) are taken as they are
        if whole.data_ptr() != logits.data_ptr():
            whole = logits.view(whole.shape)  # ... or the contiguous copy that had to be made of it, in its shape
        targets = dev_tensor(targets, "targets", torch.int64)
        M = logits.numel() // V
        if targets.numel() != M:
            raise BayesLMError("cross_entropy: %d targets for %d rows" % (targets.numel(), M))
        if M == 0:
            raise BayesLMError("cross_entropy: no rows (the mean over zero tokens is undefined; torch returns nan here)")
        nll = torch.empty(M, device=logits.device, dtype=torch.float32)
        loss = torch.zeros((), device=logits.device, dtype=torch.float32)
        grad_mode = ctx.needs_input_grad[0]  # forward itself runs with grad mode off
        fuse = grad_mode and unit_grad and not keep
        lse = torch.empty(M, device=logits.device, dtype=torch.float32) if (grad_mode and not fuse) else None
        L.require_gfx950()
        calls().blm_ce_fwd_bwd(ptr(logits), ld, ptr(targets), ptr(nll), ptr(lse), ptr(loss), ptr(logits) if fuse else None, 1.0 / M, M, V, stream())
        if fuse:  # the buffer now holds the gradient: any other autograd consumer of the logits must fail, not read it
            torch.autograd.graph.increment_version(whole)
        inv_count = None
        if keep:  # torch's mean: over the targets that are not ignore_index (device-side count, no host synchronisation)
            inv_count = 1.0 / (targets != -100).sum().clamp_(min=1).to(torch.float32)
            ctx.save_for_backward(whole)  # version-checked at backward
            ctx.meta = (None, targets, lse, fuse, M, V, keep, inv_count, ld)
        else:
            ctx.meta = (whole, targets, lse, fuse, M, V, keep, None, ld)
        ctx.mark_non_differentiable(nll)
        ctx.set_materialize_grads(False)  # no zero fill for the per-token NLL's (non-existent) gradient
        return (loss * inv_count if keep else loss / M), nll

    @staticmethod
    def backward(ctx, g, _g_nll):
        logits, targets, lse, fuse, M, V, keep, inv_count, ld = ctx.meta
        if g is None:
            return None, None, None, None
        if fuse:
            return logits, None, None, None
        if not keep:  # the gradient is written over the logits: a second backward would read the first one's gradient
            if getattr(ctx, "spent", False):
                raise BayesLMError("cross_entropy: backward ran already and overwrote the logits with their gradient; a second "
                                   "backward over a retained graph needs keep=True (ops.as_logits + F.cross_entropy)")
            ctx.spent = True
        g = _f32(g.reshape(1), "g")
        if keep:
            (logits,) = ctx.saved_tensors
            g = g * (inv_count * M)  # the kernel scales by 1 / M
        # keep: the caller's logits stay what they are (a user loop may still read them after backward): the gradient gets its own
        # buffer, rows strided as the logits' (one stride serves both in the kernel)
        if not keep:
            out = logits
        elif ld == V:
            out = torch.empty_like(logits)
        elif ld == (V + 3) // 4 * 4:  # registered as this module's: ops._Linear may run its padded backward on it
            out = _padded_rows(logits.shape[:-1], V, logits.device)[0]
        else:
            out = torch.empty(M, ld, device=logits.device, dtype=torch.float32)[:, :V].view(logits.shape)
        calls().blm_ce_bwd(ptr(logits), ld, ptr(targets), ptr(lse), ptr(g), 1.0 / M, ptr(out), M, V, stream())
        if not keep:
            torch.autograd.graph.increment_version(logits)
        return out, None, None, None


def cross_entropy(logits, targets, unit_grad=False):
    """-> (mean NLL, per-token NLL).  In grad mode the logits buffer is CONSUMED: it is overwritten with the gradient
    (its version counter is bumped, so another autograd use of the same tensor raises instead of reading gradients;
    read anything else you need from the logits BEFORE calling this).  ``unit_grad=True`` is the trainers' contract
    only: the loss enters the objective with coefficient exactly 1 (train.py:412) and the upstream gradient is not
    looked at.  The mean is over ALL M rows (the trainers' targets are corpus words, train.py:299-304); a row whose target
    is outside [0, V) contributes no loss and no gradient but still counts in M -- torch's ``ignore_index`` mean (over the
    other rows only) is what ``F.cross_entropy`` on the models' `Logits` gives."""
    if type(logits) is not torch.Tensor:
        logits = logits.as_subclass(torch.Tensor)  # model outputs are `Logits` in grad mode (below); the op wants the plain tensor
    return _CrossEntropy.apply(logits, targets, unit_grad)


# ----------------------------------------------------------------------------
# distillation: cross entropy against a teacher's dense distribution, mixed with the hard-label one  (blm_ce_soft_fwd_bwd)
# ----------------------------------------------------------------------------
class SoftStats(NamedTuple):
    """The per-token parts of ops.cross_entropy_soft (include/bayeslm.h, blm_ce_soft_fwd_bwd)."""
    nll: torch.Tensor   # (M,) hard-label NLL; 0 where the target is outside [0, V)
    soft: torch.Tensor  # (M,) cross entropy of the student under the teacher's distribution q
    kl: torch.Tensor    # (M,) KL(q || student), summed term by term


class _CrossEntropySoft(torch.autograd.Function):
    """As _CrossEntropy, for loss = mean_m (1 - weight) nll[m] + weight soft[m].  unit_grad=True (the trainer's case): the forward
    pass over the logits overwrites them in place with the gradient at scale 1 / M, and backward returns that buffer untouched.
    unit_grad=False: the same kernel writes the gradient into a buffer of its own in forward, and backward multiplies it by the
    upstream scalar."""

    @staticmethod
    def forward(ctx, logits, targets, teacher_logp, weight, unit_grad, temper=None):
        V = logits.shape[-1]
        whole = logits
        logits, ld = _rows2d(logits, V, "logits")  # rows padded to 4 floats (odd vocabulary, ops._Linear) are taken as they are
        if whole.data_ptr() != logits.data_ptr():
            whole = logits.view(whole.shape)
        targets = dev_tensor(targets, "targets", torch.int64)
        M = logits.numel() // V
        if targets.numel() != M:
            raise BayesLMError("cross_entropy_soft: %d targets for %d rows" % (targets.numel(), M))
        if M == 0:
            raise BayesLMError("cross_entropy_soft: no rows (the mean over zero tokens is undefined; torch returns nan here)")
        if teacher_logp.dim() != 2 or tuple(teacher_logp.shape) != (M, V):
            raise BayesLMError("cross_entropy_soft: teacher_logp %s against %d rows of %d logits: an (M, V) matrix over the same "
                               "vocabulary expected" % (tuple(teacher_logp.shape), M, V))
        logq, ldq = _rows2d(teacher_logp, V, "teacher_logp")  # linear_mc_logprobs' padded rows likewise
        dev = logits.device
        rows, nll, soft, kl = (torch.empty(M, device=dev, dtype=torch.float32) for _ in range(4))
        loss = torch.zeros((), device=dev, dtype=torch.float32)
        grad_mode = ctx.needs_input_grad[0]  # forward itself runs with grad mode off
        fuse = grad_mode and unit_grad
        grad = None
        if fuse:
            grad = logits
        elif grad_mode:  # rows strided as the logits' (one stride serves both in the kernel)
            if ld == V:
                grad = torch.empty_like(logits)
            elif ld == (V + 3) // 4 * 4:  # registered as this module's: ops._Linear may run its padded backward on it
                grad = _padded_rows((M,), V, dev)[0]
            else:
                grad = torch.empty(M, ld, device=dev, dtype=torch.float32)[:, :V]
        L.require_gfx950()
        if temper is None:
            calls().blm_ce_soft_fwd_bwd(ptr(logits), ld, ptr(logq), ldq, ptr(targets), float(weight), ptr(rows), ptr(nll), ptr(soft), ptr(kl),
                                        None, ptr(loss), ptr(grad), 1.0 / M, M, V, stream())
        else:  # (beta, soft_scale): the soft term at a temperature
            calls().blm_ce_soft_temp_fwd_bwd(ptr(logits), ld, ptr(logq), ldq, ptr(targets), float(weight), temper[0], temper[1], ptr(rows),
                                             ptr(nll), ptr(soft), ptr(kl), None, ptr(loss), ptr(grad), 1.0 / M, M, V, stream())
        if fuse:  # the buffer now holds the gradient: any other autograd consumer of the logits must fail, not read it
            torch.autograd.graph.increment_version(whole)
        ctx.meta = (whole if fuse else grad.view(whole.shape) if grad is not None else None, fuse)
        ctx.mark_non_differentiable(nll, soft, kl)
        ctx.set_materialize_grads(False)
        return loss / M, nll, soft, kl

    @staticmethod
    def backward(ctx, g, _g_nll, _g_soft, _g_kl):
        grad, fuse = ctx.meta
        if g is None:
            return None, None, None, None, None, None
        if fuse:
            return grad, None, None, None, None, None
        if getattr(ctx, "spent", False):  # the buffer was scaled by the first backward's upstream gradient
            raise BayesLMError("cross_entropy_soft: backward ran already and scaled the gradient buffer by its upstream gradient; a "
                               "second backward over a retained graph needs a second forward")
        ctx.spent = True
        grad.mul_(_f32(g.reshape(()), "g"))
        return grad, None, None, None, None, None


def _temper(name, temperature, soft_scale):
    """The ``temperature`` / ``soft_scale`` keywords of the distillation losses -> None (temperature 1 and factor 1: the untempered
    entry point, as before the keywords existed) or (beta, c) = (float32(1 / T), soft_scale or T * T) for the tempered one."""
    T = temperature
    if isinstance(T, bool) or not isinstance(T, (int, float)) or not math.isfinite(T) or not T > 0:
        raise BayesLMError("%s: temperature must be a finite float > 0, got %r" % (name, T))
    beta = float(torch.tensor(1.0 / float(T), dtype=torch.float32))
    if not (math.isfinite(beta) and beta > 0.0):
        raise BayesLMError("%s: temperature %r: 1 / temperature = %r is no finite float32 > 0" % (name, T, beta))
    c = soft_scale
    if c is not None and (isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) or c < 0):
        raise BayesLMError("%s: soft_scale must be None (temperature ** 2) or a finite float >= 0, got %r" % (name, c))
    if float(T) == 1.0 and (c is None or float(c) == 1.0):
        return None
    c = float(T) * float(T) if c is None else float(c)
    if not math.isfinite(float(torch.tensor(c, dtype=torch.float32))):
        raise BayesLMError("%s: soft_scale = %r (temperature %r) is no finite float32" % (name, c, T))
    return beta, c


def cross_entropy_soft(logits, targets, teacher_logp, weight, unit_grad=False, temperature=1.0, soft_scale=None):
    """Distillation loss -> (mean over the M rows of (1 - weight) nll + weight soft, SoftStats(nll, soft, kl)): ``soft`` is the
    cross entropy of softmax(logits) under the teacher's distribution exp(teacher_logp), ``nll`` the hard-label one against
    ``targets``, ``kl`` = KL(teacher || student) per row; definitions in include/bayeslm.h, blm_ce_soft_fwd_bwd -- one pass
    over both matrices, the gradient included.  ``teacher_logp``: (M, V) fp32 log-probabilities on the GPU, no gradient (the
    padded rows of ops.linear_mc_logprobs are read in place; -inf entries are zeros of the teacher).  ``weight``: a float in
    [0, 1]; 0 is ops.cross_entropy's loss.  As there, in grad mode with ``unit_grad=True`` (the trainers' contract: the loss
    enters the objective with coefficient exactly 1) the logits buffer is CONSUMED: it is overwritten with the gradient and
    its version counter is bumped; with ``unit_grad=False`` the logits stay and the gradient has its own buffer.
    ``temperature`` T (a finite float > 0) puts the soft term at a softmax temperature (include/bayeslm.h,
    blm_ce_soft_temp_fwd_bwd): softmax(logits / T) against the teacher raised to 1 / T and renormalised, times ``soft_scale``
    (None: T ** 2, Hinton's scaling); the hard term stays at temperature 1, and ``soft`` / ``kl`` of the result are the quantities
    at temperature, without that factor.  T = 1 with ``soft_scale`` None or 1 is the untempered call, bit for bit."""
    if type(logits) is not torch.Tensor:
        logits = logits.as_subclass(torch.Tensor)  # model outputs are `Logits` in grad mode (below); the op wants the plain tensor
    if not torch.is_tensor(teacher_logp):
        raise BayesLMError("cross_entropy_soft: teacher_logp must be a tensor, got %s" % type(teacher_logp).__name__)
    if teacher_logp.requires_grad:
        raise BayesLMError("cross_entropy_soft: teacher_logp requires grad; the teacher is a constant of the loss (detach it: "
                           "no gradient is formed for it)")
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0.0 <= float(weight) <= 1.0:
        raise BayesLMError("cross_entropy_soft: weight must be a float in [0, 1], got %r" % (weight,))
    temper = _temper("cross_entropy_soft", temperature, soft_scale)
    loss, nll, soft, kl = _CrossEntropySoft.apply(logits, targets, teacher_logp, float(weight), unit_grad, temper)
    return loss, SoftStats(nll, soft, kl)


# ----------------------------------------------------------------------------
# distillation from top-k teacher targets: the same loss against K (id, log-probability) pairs per token  (blm_ce_soft_topk_fwd_bwd)
# ----------------------------------------------------------------------------
class SparseTargets(NamedTuple):
    """A teacher's K best next words per token (distill.Teacher.topk, distill.TeacherCache.load): what
    ops.cross_entropy_soft_topk is trained against.  An id outside [0, V) (-1 by convention) marks an empty slot."""
    ids: torch.Tensor   # (M, K) int32, the live ids of a row distinct
    logq: torch.Tensor  # (M, K) float32 log-probabilities; -inf: a zero of the teacher


class _CrossEntropySoftTopk(torch.autograd.Function):
    """_CrossEntropySoft with the teacher's dense rows replaced by SparseTargets: the same buffers, the same two gradient forms."""

    @staticmethod
    def forward(ctx, logits, targets, ids, logq, weight, unit_grad, temper=None):
        V = logits.shape[-1]
        whole = logits
        logits, ld = _rows2d(logits, V, "logits")  # rows padded to 4 floats (odd vocabulary, ops._Linear) are taken as they are
        if whole.data_ptr() != logits.data_ptr():
            whole = logits.view(whole.shape)
        targets = dev_tensor(targets, "targets", torch.int64)
        M = logits.numel() // V
        if targets.numel() != M:
            raise BayesLMError("cross_entropy_soft_topk: %d targets for %d rows" % (targets.numel(), M))
        if M == 0:
            raise BayesLMError("cross_entropy_soft_topk: no rows (the mean over zero tokens is undefined; torch returns nan here)")
        if ids.dim() != 2 or ids.shape[0] != M or tuple(logq.shape) != tuple(ids.shape):
            raise BayesLMError("cross_entropy_soft_topk: sparse ids %s, logq %s against %d rows of logits: two (M, K) matrices expected"
                               % (tuple(ids.shape), tuple(logq.shape), M))
        K = ids.shape[1]
        if not 1 <= K <= L.TOPK_MAX:
            raise BayesLMError("cross_entropy_soft_topk: K = %d targets per row outside [1, BLM_TOPK_MAX = %d]" % (K, L.TOPK_MAX))
        ids, logq = dev_tensor(ids, "sparse.ids", torch.int32), dev_tensor(logq, "sparse.logq", torch.float32)
        dev = logits.device
        rows, nll, soft, kl = (torch.empty(M, device=dev, dtype=torch.float32) for _ in range(4))
        loss = torch.zeros((), device=dev, dtype=torch.float32)
        grad_mode = ctx.needs_input_grad[0]  # forward itself runs with grad mode off
        fuse = grad_mode and unit_grad
        grad = None
        if fuse:
            grad = logits
        elif grad_mode:  # rows strided as the logits' (one stride serves both in the kernel)
            if ld == V:
                grad = torch.empty_like(logits)
            elif ld == (V + 3) // 4 * 4:  # registered as this module's: ops._Linear may run its padded backward on it
                grad = _padded_rows((M,), V, dev)[0]
            else:
                grad = torch.empty(M, ld, device=dev, dtype=torch.float32)[:, :V]
        L.require_gfx950()
        if temper is None:
            calls().blm_ce_soft_topk_fwd_bwd(ptr(logits), ld, ptr(ids), ptr(logq), K, K, ptr(targets), float(weight), ptr(rows), ptr(nll),
                                             ptr(soft), ptr(kl), None, ptr(loss), ptr(grad), 1.0 / M, M, V, stream())
        else:  # (beta, soft_scale): the soft term at a temperature
            calls().blm_ce_soft_topk_temp_fwd_bwd(ptr(logits), ld, ptr(ids), ptr(logq), K, K, ptr(targets), float(weight), temper[0],
                                                  temper[1], ptr(rows), ptr(nll), ptr(soft), ptr(kl), None, ptr(loss), ptr(grad), 1.0 / M,
                                                  M, V, stream())
        if fuse:  # the buffer now holds the gradient: any other autograd consumer of the logits must fail, not read it
            torch.autograd.graph.increment_version(whole)
        ctx.meta = (whole if fuse else grad.view(whole.shape) if grad is not None else None, fuse)
        ctx.mark_non_differentiable(nll, soft, kl)
        ctx.set_materialize_grads(False)
        return loss / M, nll, soft, kl

    @staticmethod
    def backward(ctx, g, _g_nll, _g_soft, _g_kl):
        grad, fuse = ctx.meta
        if g is None:
            return None, None, None, None, None, None, None
        if fuse:
            return grad, None, None, None, None, None, None
        if getattr(ctx, "spent", False):  # the buffer was scaled by the first backward's upstream gradient
            raise BayesLMError("cross_entropy_soft_topk: backward ran already and scaled the gradient buffer by its upstream gradient; "
                               "a second backward over a retained graph needs a second forward")
        ctx.spent = True
        grad.mul_(_f32(g.reshape(()), "g"))
        return grad, None, None, None, None, None, None


def cross_entropy_soft_topk(logits, targets, sparse, weight, unit_grad=False, temperature=1.0, soft_scale=None):
    """ops.cross_entropy_soft against the K best entries of the teacher per token instead of its dense rows -> (loss,
    SoftStats(nll, soft, kl)); definitions in include/bayeslm.h, blm_ce_soft_topk_fwd_bwd.  ``sparse``: SparseTargets(ids (M, K)
    int32, logq (M, K) float32) on the GPU, no gradient, 1 <= K <= BLM_TOPK_MAX, the live ids of a row distinct (ops.topk_rows'
    are); an id outside [0, V) is an empty slot.  The teacher's mass Q = sum_j exp(logq_j) of a row is carried as it is: with
    Q < 1 (top-k of a normalised teacher) the soft term weighs Q, and the tail of the teacher is dropped.  ``weight``,
    ``unit_grad`` and what happens to the logits buffer: as ops.cross_entropy_soft.  ``temperature``, ``soft_scale``: as there
    (blm_ce_soft_topk_temp_fwd_bwd); the tempered target is the K entries raised to 1 / T and renormalised over the live ones, so
    a constant on a row's logq -- renormalised targets or not -- changes nothing, and Q is not carried."""
    if type(logits) is not torch.Tensor:
        logits = logits.as_subclass(torch.Tensor)  # model outputs are `Logits` in grad mode (below); the op wants the plain tensor
    if not (isinstance(sparse, tuple) and len(sparse) == 2 and torch.is_tensor(sparse[0]) and torch.is_tensor(sparse[1])):
        raise BayesLMError("cross_entropy_soft_topk: sparse must be SparseTargets(ids, logq), got %s" % type(sparse).__name__)
    ids, logq = sparse
    if ids.dtype != torch.int32:
        raise BayesLMError("cross_entropy_soft_topk: sparse.ids must be int32, got %s" % ids.dtype)
    if logq.requires_grad:
        raise BayesLMError("cross_entropy_soft_topk: sparse.logq requires grad; the teacher is a constant of the loss (detach it: "
                           "no gradient is formed for it)")
    if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not 0.0 <= float(weight) <= 1.0:
        raise BayesLMError("cross_entropy_soft_topk: weight must be a float in [0, 1], got %r" % (weight,))
    temper = _temper("cross_entropy_soft_topk", temperature, soft_scale)
    loss, nll, soft, kl = _CrossEntropySoftTopk.apply(logits, targets, ids, logq, float(weight), unit_grad, temper)
    return loss, SoftStats(nll, soft, kl)


class Logits(torch.Tensor):
    """What a language model's decoder returns in grad mode: a plain fp32 tensor to every consumer, except that
    ``torch.nn.functional.cross_entropy`` on it (the reference loop's ``criterion(output.view(-1, ntokens), targets)``,
    train.py:332 with ``nn.CrossEntropyLoss()``) runs the engine's one-pass cross-entropy kernels instead of torch's
    log-softmax + NLL chain over the (M, V) logits -- an unchanged reference training script gets them by importing the shim
    (INTEGRATION.md level 1).  Non-destructive here: the logits keep their values, the gradient gets its own buffer.  Only the
    default loss takes the short cut (mean reduction, no class weights, no label smoothing, ignore_index at its default -100, which is
    honoured as torch honours it: such rows get no loss and no gradient, the mean is over the others); anything else falls through to
    torch.  ``view`` / ``reshape`` / ``contiguous`` /
    ``flatten`` keep the type (so the reshaped logits still reach the loss as ``Logits``); every other operation returns plain
    tensors."""

    _KEEP = None  # filled below: the shape-only ops that preserve the type

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func is torch.nn.functional.cross_entropy:
            inp = args[0] if len(args) > 0 else kwargs.get("input")
            tgt = args[1] if len(args) > 1 else kwargs.get("target")
            plain = (kwargs.get("weight") is None and kwargs.get("reduction", "mean") == "mean" and kwargs.get("label_smoothing", 0.0) == 0.0
                     and kwargs.get("ignore_index", -100) == -100 and kwargs.get("size_average") is None and kwargs.get("reduce") is None
                     and len(args) <= 2 and torch.is_tensor(inp) and torch.is_tensor(tgt) and inp.dim() == 2 and tgt.dim() == 1
                     and inp.is_cuda and inp.dtype == torch.float32 and tgt.dtype == torch.int64 and tgt.numel() == inp.shape[0])
            if plain:
                with torch._C.DisableTorchFunctionSubclass():
                    return _CrossEntropy.apply(inp.as_subclass(torch.Tensor), tgt, False, True)[0]
        if func in cls._KEEP:
            return super().__torch_function__(func, types, args, kwargs)
        with torch._C.DisableTorchFunctionSubclass():
            return func(*args, **kwargs)


Logits._KEEP = frozenset([torch.Tensor.view, torch.Tensor.reshape, torch.Tensor.contiguous, torch.Tensor.flatten, torch.flatten,
                          torch.reshape, torch.Tensor.view_as, torch.Tensor.reshape_as])


def as_logits(t):
    """Decoder output of a language model in grad mode (see Logits)."""
    return t.as_subclass(Logits) if (torch.is_grad_enabled() and type(t) is torch.Tensor) else t


def cross_entropy_interp(logits_a, logits_b, alpha, targets):
    """Scoring with two models: per-token NLL of the interpolated LOGITS alpha*a + (1-alpha)*b
    (compute_sentence_scores_bayes_jianwei.py:157-168) without storing the mixture.  Forward only.
    -> (mean NLL, per-token NLL)"""
    a, b = _f32(logits_a, "logits_a"), _f32(logits_b, "logits_b")
    if a.shape != b.shape or a.dim() != 2:
        raise ValueError("cross_entropy_interp: logits must be two (M, V) matrices of the same shape")
    L.require_gfx950()
    M, V = a.shape
    tgt = targets.contiguous()
    nll = torch.empty(M, device=a.device, dtype=torch.float32)
    calls().blm_ce_interp_fwd(ptr(a), ptr(b), V, float(alpha), ptr(tgt), ptr(nll), M, V, stream())
    return nll.mean(), nll


def _inference_only(name, *tensors):
    """The guard of the fused decoder family: forward-only launches, refused where autograd would expect a backward."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise BayesLMError("%s is an inference-only path (no backward): call it under torch.no_grad()" % name)


def _unit_rows(x, name):
    """(..., K) fp32 -> its 2-D rows (M, K) with unit inner stride (a copy only when the inner stride is not 1)."""
    x2 = _f32(x, name).reshape(-1, x.shape[-1])
    return x2 if x2.stride(-1) == 1 else x2.contiguous()


def linear_nll_supported(weight, bias):
    """Decoders blm_linear_nll takes: fp32 on the GPU, row-major, vocabulary a multiple of 4, 16-byte aligned bias."""
    return (weight.is_cuda and weight.dtype == torch.float32 and weight.dim() == 2 and weight.is_contiguous()
            and weight.shape[0] % 4 == 0 and (bias is None or (bias.is_contiguous() and bias.data_ptr() % 16 == 0)))


def linear_nll(x, weight, bias, targets):
    """Inference only: per-row NLL of the decoder ``x @ weight.T + bias`` against ``targets`` without materialising the (M, V)
    logits (blm_linear_nll: softmax partials per column tile in the GEMM epilogue + a folding kernel).  What
    decoder -> log_softmax -> gather computes in train.py:452-455 / compute_sentence_scores...py:157-170.  -> (M,) NLL"""
    _inference_only("linear_nll", x, weight)
    x2 = _unit_rows(x, "x")
    M, K = x2.shape
    V = weight.shape[0]
    if weight.shape[1] != K or targets.numel() != M:
        raise ValueError("linear_nll: x (M, K), weight (V, K) and M targets expected")
    L.require_gfx950()
    tgt = targets.reshape(-1).contiguous()
    nll = torch.empty(M, device=x2.device, dtype=torch.float32)
    ws = torch.empty(int(calls().blm_linear_nll_ws_floats(M, V)), device=x2.device, dtype=torch.float32)
    calls().blm_linear_nll(ptr(x2), x2.stride(0), ptr(weight), weight.stride(0), ptr(bias), ptr(tgt), ptr(nll), None, ptr(ws), M, V, K, stream())
    return nll


class McStats(NamedTuple):
    """Per-token uncertainty of S Monte-Carlo weight samples (include/bayeslm.h, blm_linear_mc_stats)."""
    nll_s: torch.Tensor    # (M, S) NLL of the target under each sample
    bma_nll: torch.Tensor  # (M,) NLL of the target under the sample-averaged distribution pbar
    h_pred: torch.Tensor   # (M,) predictive entropy H[pbar]
    mi: torch.Tensor       # (M,) mutual information between prediction and weights, mean_s KL(p_s || pbar); H[pbar] - mi = E_s H[p_s]


def _mc_pad(weight, bias):
    """(weight, bias) as blm_linear_mc_stats takes them: Np = V rounded up to 4 rows, contiguous, 16-byte aligned -- the tensors
    themselves when they are, else a copy onto zero padding rows."""
    V, K = weight.shape
    if V % 4 == 0 and weight.is_contiguous() and weight.data_ptr() % 16 == 0 and (
            bias is None or (bias.is_contiguous() and bias.data_ptr() % 16 == 0)):
        return weight, bias
    Np = (V + 3) // 4 * 4
    wp = torch.zeros(Np, K, device=weight.device, dtype=torch.float32)
    wp[:V] = weight
    bp = None
    if bias is not None:
        bp = torch.zeros(Np, device=weight.device, dtype=torch.float32)
        bp[:V] = bias
    return wp, bp


class McDecoder:
    """The padded decoder of a run of linear_mc_stats calls over FIXED weights (one scoring run), built once and passed as ``dec``
    to each call, as InterpDecoder is for the two-model launch.  It holds the source tensors and the caller scopes it to the run:
    a copy made here is not refreshed when the weights change, so it must not outlive the run."""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias
        self.wp, self.bp = _mc_pad(_f32(weight, "weight"), None if bias is None else _f32(bias, "bias"))


def _mc_operands(name, x, weight, bias, S, dec, n_targets):
    """The checks linear_mc_stats and linear_mc_logprobs share -> (x fp32, S, M, K, V, padded weight, padded bias, Sp, chunks):
    Sp the samples rounded up to a power of two, chunks the token ranges whose M * Sp * K * 4 bytes stay under the LDS-DMA
    loaders' 2^32.  ``n_targets``: the number of targets, or None without targets."""
    _inference_only(name, x, weight, bias)
    if dec is not None and (dec.weight is not weight or dec.bias is not bias):
        raise ValueError("%s: dec was built for another decoder" % name)
    x = _f32(x, "x")
    if x.dim() != 3:
        raise ValueError("%s: x must be (S, M, K)" % name)
    S_, M, K = x.shape
    if S is not None and int(S) != S_:
        raise ValueError("%s: S = %d but x holds %d samples" % (name, S, S_))
    S = S_
    if not 1 <= S <= 64:
        raise BayesLMError("%s: 1..64 samples, got %d" % (name, S))
    weight = _f32(weight, "weight")
    if weight.dim() != 2 or weight.shape[1] != K or (n_targets is not None and n_targets != M) or (
            bias is not None and bias.numel() != weight.shape[0]):
        raise ValueError("%s: x (S, M, K), weight (V, K), bias (V,) and M targets expected" % name)
    if bias is not None:
        bias = _f32(bias, "bias")
    L.require_gfx950()
    wp, bp = (dec.wp, dec.bp) if dec is not None else _mc_pad(weight, bias)
    Sp = 1 << (S - 1).bit_length()
    return x, S, M, K, weight.shape[0], wp, bp, Sp, _row_chunks(M, Sp * K)


def _mc_token_major(x, a, b, Sp):
    """Rows [a, b) of the sample-major (S, M, K) operand as the kernels take them: token-major (b - a, Sp, K), zeros in the
    padding samples."""
    S, _, K = x.shape
    if S == Sp:
        return x[:, a:b].transpose(0, 1).contiguous()
    xt = torch.zeros(b - a, Sp, K, device=x.device, dtype=torch.float32)
    xt[:, :S] = x[:, a:b].transpose(0, 1)
    return xt


def linear_mc_stats(x, weight, bias, targets, S=None, dec=None):
    """Inference only: token-level predictive uncertainty of S Monte-Carlo weight samples without materialising any of the
    S x M x V logits (blm_linear_mc_stats: two decoder products whose epilogues keep per-tile partials, and a folding kernel).
    ``x``: (S, M, K), sample-major as the S forward passes produce it; ``weight`` (V, K), ``bias`` (V,) or None, ``targets`` (M,).
    ``dec``: McDecoder(weight, bias) of the run, reused instead of padding the vocabulary (V % 4 != 0) again per call.
    -> McStats(nll_s (M, S), bma_nll, h_pred, mi (M,)); definitions in include/bayeslm.h."""
    x, S, M, K, V, wp, bp, Sp, chunks = _mc_operands("linear_mc_stats", x, weight, bias, S, dec, targets.numel())
    tgt = dev_tensor(targets.reshape(-1), "targets", torch.int64)
    dev = x.device
    nll_s = torch.empty(M, S, device=dev, dtype=torch.float32)
    bma, h, mi = (torch.empty(M, device=dev, dtype=torch.float32) for _ in range(3))
    if M == 0:
        return McStats(nll_s, bma, h, mi)
    ws = torch.empty(int(calls().blm_linear_mc_stats_ws_floats(max(b - a for a, b in chunks), S, V)), device=dev, dtype=torch.float32)
    for a, b in chunks:
        xt = _mc_token_major(x, a, b, Sp)
        calls().blm_linear_mc_stats(ptr(xt), K, ptr(wp), K, ptr(bp), ptr(tgt[a:b]), S, ptr(nll_s[a:b]), ptr(bma[a:b]),
                                    ptr(h[a:b]), ptr(mi[a:b]), ptr(ws), b - a, V, K, stream())
    return McStats(nll_s, bma, h, mi)


class McLogProbs(NamedTuple):
    """The model average's next-word distribution over S Monte-Carlo weight samples (include/bayeslm.h, blm_linear_mc_logprobs);
    the statistics are those of McStats, None where they were not asked for."""
    logp: torch.Tensor               # (M, V) log pbar: a view of rows padded to 4 floats
    h_pred: Optional[torch.Tensor]   # (M,) with stats
    mi: Optional[torch.Tensor]       # (M,) with stats
    nll_s: Optional[torch.Tensor]    # (M, S) with targets
    bma_nll: Optional[torch.Tensor]  # (M,) with targets: -logp[m, targets[m]]


def linear_mc_logprobs(x, weight, bias, tgt=None, S=None, dec=None, stats=True):
    """Inference only: log of the sample-averaged next-word distribution, log pbar = log mean_s softmax(x[s] @ weight.T + bias),
    for every token -- the (M, V) matrix a caller samples from or ranks -- without materialising the S x M x V logits
    (blm_linear_mc_logprobs: linear_mc_stats' two decoder products, the second one also storing log pbar from its epilogue).
    ``x``: (S, M, K) as linear_mc_stats takes it; ``dec``: the run's McDecoder; ``stats``: also h_pred and mi; ``tgt`` (M,): also
    nll_s and bma_nll.  -> McLogProbs; S = 1 gives the log-softmax."""
    x, S, M, K, V, wp, bp, Sp, chunks = _mc_operands("linear_mc_logprobs", x, weight, bias, S, dec, None if tgt is None else tgt.numel())
    dev = x.device
    logp, Np = _padded_rows((M,), V, dev)
    h, mi = ((torch.empty(M, device=dev, dtype=torch.float32) for _ in range(2)) if stats else (None, None))
    nll_s = bma = None
    if tgt is not None:
        tgt = dev_tensor(tgt.reshape(-1), "targets", torch.int64)
        nll_s = torch.empty(M, S, device=dev, dtype=torch.float32)
        bma = torch.empty(M, device=dev, dtype=torch.float32)
    if M == 0:
        return McLogProbs(logp, h, mi, nll_s, bma)
    ws = torch.empty(int(calls().blm_linear_mc_logprobs_ws_floats(max(b - a for a, b in chunks), S, V)), device=dev, dtype=torch.float32)
    for a, b in chunks:
        o_tgt, o_nll, o_bma, o_h, o_mi = (None if t is None else ptr(t[a:b]) for t in (tgt, nll_s, bma, h, mi))
        xt = _mc_token_major(x, a, b, Sp)
        calls().blm_linear_mc_logprobs(ptr(xt), K, ptr(wp), K, ptr(bp), o_tgt, S, ptr(logp[a:b]), Np, o_nll, o_bma, o_h, o_mi,
                                       ptr(ws), b - a, V, K, stream())
    return McLogProbs(logp, h, mi, nll_s, bma)


class InterpDecoder:
    """The packed operands of a two-model scoring run (blm_linear_nll2): [W1 | W2] and alpha b1 + (1 - alpha) b2 are
    built by the first call and kept for the following ones (same weights, same alpha: one scoring run)."""

    def __init__(self, w1, b1, w2, b2, alpha):
        self.w1, self.b1, self.w2, self.b2, self.alpha = _f32(w1, "w1"), b1, _f32(w2, "w2"), b2, float(alpha)
        if self.w1.shape[0] != self.w2.shape[0]:
            raise BayesLMError("interpolated decoders need one vocabulary: %d and %d rows" % (self.w1.shape[0], self.w2.shape[0]))
        V, K1, K2 = self.w1.shape[0], self.w1.shape[1], self.w2.shape[1]
        self.wcat = torch.empty(int(calls().blm_linear_nll2_wcat_floats(V, K1, K2)), device=self.w1.device, dtype=torch.float32)
        self.packed = False


def linear_nll_interp_supported(w1, b1, w2, b2):
    """fp32 row-major decoders over ONE vocabulary (any size: the packed copy is padded) with feature counts that are multiples of 4."""
    ok = lambda w, b: (w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and w.shape[1] % 4 == 0  # noqa: E731
                       and w.data_ptr() % 16 == 0 and (b is None or (b.is_contiguous() and b.numel() == w.shape[0])))
    return ok(w1, b1) and ok(w2, b2) and w1.shape[0] == w2.shape[0]


def _interp_operands(name, x1, x2, dec, counts_ok, counted):
    """The operand prelude of the two-model launches -> (rows of x1, rows of x2, M, K1, K2, V), checked against the InterpDecoder
    ``dec``.  ``counts_ok(M)``: the caller's own count check, ``counted`` its wording in the one shape error."""
    _inference_only(name, x1, x2)
    a, b = _unit_rows(x1, "x1"), _unit_rows(x2, "x2")
    M, K1 = a.shape
    K2 = b.shape[1]
    if b.shape[0] != M or dec.w1.shape[1] != K1 or dec.w2.shape[1] != K2 or not counts_ok(M):
        raise ValueError("%s: x1 (M, K1), x2 (M, K2), decoders (V, K1) / (V, K2) and %s expected" % (name, counted))
    L.require_gfx950()
    return a, b, M, K1, K2, dec.w1.shape[0]


def _edge_operands(edge_node, edge_tgt, device):
    """The (node, target) pairs of a prefix-trie launch as int64 device vectors, and the (E,) NLL buffer it fills."""
    en = dev_tensor(edge_node.reshape(-1), "edge_node", torch.int64)
    et = dev_tensor(edge_tgt.reshape(-1), "edge_tgt", torch.int64)
    return en, et, torch.empty(en.numel(), device=device, dtype=torch.float32)


def linear_nll_interp(x1, x2, dec, targets):
    """Inference only: per-row NLL of the INTERPOLATED logits alpha (x1 W1^T + b1) + (1 - alpha) (x2 W2^T + b2)
    (compute_sentence_scores_bayes_jianwei.py:157-168) from ONE decoder + cross-entropy launch over the packed operands
    [alpha x1 | (1 - alpha) x2] . [W1 | W2]^T: neither model's (M, V) logits are stored.  ``dec``: InterpDecoder.  -> (M,) NLL"""
    a, b, M, K1, K2, V = _interp_operands("linear_nll_interp", x1, x2, dec, lambda M: targets.numel() == M, "M targets")
    tgt = dev_tensor(targets.reshape(-1), "targets", torch.int64)
    nll = torch.empty(M, device=a.device, dtype=torch.float32)
    if M == 0:
        return nll
    ws = torch.empty(int(calls().blm_linear_nll2_ws_floats(M, V, K1, K2)), device=a.device, dtype=torch.float32)
    calls().blm_linear_nll2(ptr(a), a.stride(0), ptr(dec.w1), dec.w1.stride(0), ptr(dec.b1), K1,
                            ptr(b), b.stride(0), ptr(dec.w2), dec.w2.stride(0), ptr(dec.b2), K2, dec.alpha,
                            ptr(tgt), ptr(nll), None, ptr(dec.wcat), 0 if dec.packed else 1, ptr(ws), M, V, stream())
    dec.packed = True
    return nll


# ----------------------------------------------------------------------------
# KL term  mean(mu^2 - 2 lg + exp(2 lg) [-1]) / 2  over a row window of mu
# ----------------------------------------------------------------------------
class _KLMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, lgstd, row_lo, minus_one, count_override):
        mu = _f32(mu, "mu")
        lgstd = _f32(lgstd, "lgstd")
        rows = lgstd.shape[0]
        cols = lgstd.numel() // rows
        ld = mu.numel() // mu.shape[0]
        out = torch.zeros((), device=mu.device, dtype=torch.float32)
        n = rows * cols
        w = float(n) / float(count_override) if count_override else 1.0
        L.require_gfx950()
        calls().blm_kl_mean_fwd(mu.data_ptr() + 4 * row_lo * ld, ld, ptr(lgstd), rows, cols, int(minus_one), w, ptr(out), stream())
        ctx.meta = (mu, lgstd, row_lo, rows, cols, ld, w)
        return out

    @staticmethod
    def backward(ctx, g):
        mu, lgstd, row_lo, rows, cols, ld, w = ctx.meta
        g = _f32(g.reshape(1), "g")
        # the kernel writes both gradients; a tensor that does not require one gets a scratch buffer
        gm, _, dmu = _wgrad_target(mu, zero=True) if mu.requires_grad else (torch.zeros_like(mu), False, None)
        gl, _, dlg = _wgrad_target(lgstd, zero=True) if lgstd.requires_grad else (torch.zeros_like(lgstd), False, None)
        calls().blm_kl_mean_bwd(mu.data_ptr() + 4 * row_lo * ld, ld, ptr(lgstd), rows, cols, ptr(g), w,
                                gm.data_ptr() + 4 * row_lo * ld, ld, ptr(gl), stream())
        _notify(mu, lgstd)
        return dmu, dlg, None, None, None


def kl_mean(mu, lgstd, row_lo=0, minus_one=False, count=None):
    """KL of the rows [row_lo, row_lo+lgstd.shape[0]) of mu against lgstd.  ``count`` replaces the
    element count of the mean (Bayes2LSTM concatenates hh and ih before taking it, model.py:737-740)."""
    mu, lgstd = _weight(mu, "mu"), _weight(lgstd, "lgstd")
    if (mu.dim() < 1 or lgstd.dim() < 1 or mu.numel() // max(mu.shape[0], 1) != lgstd.numel() // max(lgstd.shape[0], 1)
            or not 0 <= row_lo <= mu.shape[0] - lgstd.shape[0]):
        raise BayesLMError("kl_mean: lgstd %s does not fit rows [%d, ...) of mu %s" % (tuple(lgstd.shape), row_lo, tuple(mu.shape)))
    return _KLMean.apply(mu, lgstd, row_lo, minus_one, count)


def philox_normal(n, seed, stream_id, step, device="cuda"):
    out = torch.empty(n, device=device, dtype=torch.float32)
    L.require_gfx950()
    r = L.rng(seed, stream_id, step)
    calls().blm_philox_normal(ptr(out), n, C.byref(r), stream())
    return out


# ----------------------------------------------------------------------------
# 2-layer LSTM stack as _VF.lstm computes it (model.py:812), explicit cell
# ----------------------------------------------------------------------------
_STATE_TAP = None
_PACK = threading.local()  # per thread: two scorers on two threads never see each other's layout


def _split_qkv(q, k, v, contiguous=False):
    """The attention operands of the packed-row layouts -> (q, k, v, d, row stride): the fused (R, 1, 3d) projection in ``q``
    (k = v = None) is addressed in place, separate (R, 1, d) tensors as they are or -- ``contiguous`` -- as contiguous copies."""
    if k is None:
        qkv = _f32(q, "qkv")
        d = qkv.shape[-1] // 3
        return qkv, qkv[..., d:], qkv[..., 2 * d:], d, 3 * d
    qq, kk, vv = _f32(q, "q"), _f32(k, "k"), _f32(v, "v")
    if contiguous:
        qq, kk, vv = qq.contiguous(), kk.contiguous(), vv.contiguous()
    return qq, kk, vv, qq.shape[-1], qq.shape[-1]


class packed_tokens:
    """Inference helper (the n-best scorer): inside the context the Transformer stacks keep their activations as a
    compact (R, 1, d) matrix of the REAL tokens of a padded (T, N) batch of hypotheses -- every token-wise operation
    (projections, feed-forward, layer norms, decoder) then runs on R rows instead of T * N (padding is 40-50 % of a
    batch of AMI-shaped hypotheses); only the attention core sees the padded layout (scatter before, gather after; the
    padding rows hold zeros and, the attention being causal and column-wise, never reach a real token).
    ``sel`` (R,) int64: flat indices t * N + n of the real tokens, in the order the caller wants the rows.
    The layout is thread-local and does not nest.  (The scorer also holds the model's decoder in a ``_ProjHolder.inference``
    scope, which refuses a second entry: a model object serves one scoring call at a time.)"""

    def __init__(self, sel, T, N):
        self.sel, self.T, self.N = sel, int(T), int(N)
        self._rowmap = None
        self._rows_ok = True  # the packed-row attention kernel takes this batch (decided by the library at the first call)

    def __enter__(self):
        if torch.is_grad_enabled():
            raise BayesLMError("ops.packed_tokens is an inference-only layout")
        if getattr(_PACK, "cur", None) is not None:
            raise BayesLMError("ops.packed_tokens does not nest")
        _PACK.cur = self
        return self

    def __exit__(self, *exc):
        _PACK.cur = None
        return False

    def pack(self, x):
        """(T, N, W) -> (R, 1, W)"""
        return x.reshape(self.T * self.N, x.shape[-1]).index_select(0, self.sel).unsqueeze(1)

    def unpack(self, xc):
        """(R, 1, W) -> (T, N, W), zeros in the padding"""
        out = xc.new_zeros(self.T * self.N, xc.shape[-1])
        out.index_copy_(0, self.sel, xc.reshape(-1, xc.shape[-1]))
        return out.view(self.T, self.N, -1)

    def rowmap(self):
        """(T * N,) int32: the packed row of the token at padded position t * N + n, -1 for padding (built once per batch)."""
        if self._rowmap is None:
            m = torch.full((self.T * self.N,), -1, device=self.sel.device, dtype=torch.int32)
            m[self.sel] = torch.arange(self.sel.numel(), device=self.sel.device, dtype=torch.int32)
            self._rowmap = m
        return self._rowmap

    def attention(self, q, k, v, nhead):
        """The attention core of a packed batch: q / k / v (R, 1, d) (or q = the fused (R, 1, 3d) projection, k = v = None) ->
        (R, 1, d).  Short batches (T <= 32, head_dim 64: what n-best hypotheses are) run on the packed rows themselves
        (blm_attn_fwd_rows: the kernel finds a token's row through rowmap); anything else is scattered into the padded layout,
        run through the ordinary kernels and gathered back -- a zero fill, an index_copy and a gather per layer."""
        if self._rows_ok:
            qq, kk, vv, d, ld = _split_qkv(q, k, v)
            R = qq.numel() // qq.shape[-1]
            out = torch.empty(R, 1, d, device=qq.device, dtype=torch.float32)
            L.require_gfx950()
            try:
                calls().blm_attn_fwd_rows(qq.data_ptr(), kk.data_ptr(), vv.data_ptr(), ld, ptr(out), ptr(self.rowmap()), self.T, self.N,
                                          nhead, d // nhead, stream())
                return out
            except BayesLMError as e:
                if e.status != L.ERR_UNSUPPORTED:
                    raise
            self._rows_ok = False
        if k is None:
            return self.pack(attention(self.unpack(q), nhead))
        return self.pack(attention_qkv(self.unpack(q), self.unpack(k), self.unpack(v), nhead))



class tree_tokens(packed_tokens):
    """Inference helper (the n-best scorer with shared prefixes): ``packed_tokens`` whose rows are the M nodes of the batch's prefix
    tries (bayeslms_amd/prefix_trie.py) instead of every real token -- ``sel`` (M,) int64 gives one padded position t * N + n per
    node, t being its depth, so the embedding and positional encoding are packed as for a real token; every token-wise operation
    runs on M rows.  The attention core is blm_attn_fwd_tree over the nodes: a node attends itself and its ancestors, ``end`` and
    ``lo`` (M,) int32 device tensors (one past the node's subtree, first node of its utterance).  The model must declare
    ``supports_packed``."""

    def __init__(self, sel, T, N, end, lo, model=None):
        if model is not None and not getattr(model, "supports_packed", False):
            raise BayesLMError("ops.tree_tokens: %s does not keep its activations token-wise outside the attention core "
                               "(no supports_packed): it cannot score over a prefix trie" % type(model).__name__)
        super().__init__(sel, T, N)
        if end.dtype != torch.int32 or lo.dtype != torch.int32 or end.numel() != sel.numel() or lo.numel() != sel.numel():
            raise ValueError("ops.tree_tokens: end and lo must be (M,) int32, one entry per node")
        self.end, self.lo = end.contiguous(), lo.contiguous()

    def attention(self, q, k, v, nhead):
        """q / k / v (M, 1, d) (or q = the fused (M, 1, 3d) projection, k = v = None) -> (M, 1, d) over the trie mask."""
        qq, kk, vv, d, ld = _split_qkv(q, k, v, contiguous=True)
        R = qq.numel() // qq.shape[-1]
        out = torch.empty(R, 1, d, device=qq.device, dtype=torch.float32)
        L.require_gfx950()
        calls().blm_attn_fwd_tree(qq.data_ptr(), kk.data_ptr(), vv.data_ptr(), ld, ptr(out), ptr(self.end), ptr(self.lo), R, nhead,
                                  d // nhead, stream())
        return out


def linear_nll_edges(x, dec, edge_node, edge_tgt):
    """Inference only: per-edge NLL over a prefix trie, nll[e] = logsumexp(x[node] W^T + b) - (x[node] . W[tgt] + b[tgt]) for the
    E (node, target) edges, no logit stored (blm_linear_nll_edges).  ``x`` (M, K) node rows; ``dec``: McDecoder(weight, bias) of the
    scoring run (the vocabulary padded to a multiple of 4 once); ``edge_node`` / ``edge_tgt`` (E,) int64.  -> (E,) NLL"""
    _inference_only("linear_nll_edges", x)
    x2 = _unit_rows(x, "x")
    M, K = x2.shape
    V, Np = dec.weight.shape[0], dec.wp.shape[0]
    if dec.wp.shape[1] != K or edge_node.numel() != edge_tgt.numel():
        raise ValueError("linear_nll_edges: x (M, K), a (V, K) decoder and E (node, target) pairs expected")
    L.require_gfx950()
    en, et, nll = _edge_operands(edge_node, edge_tgt, x2.device)
    E = en.numel()
    if E == 0:
        return nll
    ws = torch.empty(int(calls().blm_linear_nll_edges_ws_floats(M, Np)), device=x2.device, dtype=torch.float32)
    calls().blm_linear_nll_edges(ptr(x2), x2.stride(0), ptr(dec.wp), dec.wp.stride(0), ptr(dec.bp), ptr(en), ptr(et), ptr(nll), ptr(ws),
                                 M, E, Np, V, K, stream())
    return nll


def linear_nll_interp_edges(x1, x2, dec, edge_node, edge_tgt):
    """Inference only: linear_nll_edges over two models' INTERPOLATED logits alpha (x1 W1^T + b1) + (1 - alpha) (x2 W2^T + b2)
    (the mixing of linear_nll_interp; ``dec``: the run's InterpDecoder).  -> (E,) NLL"""
    a, b, M, K1, K2, V = _interp_operands("linear_nll_interp_edges", x1, x2, dec, lambda M: edge_node.numel() == edge_tgt.numel(),
                                          "E (node, target) pairs")
    en, et, nll = _edge_operands(edge_node, edge_tgt, a.device)
    E = en.numel()
    if E == 0:
        return nll
    ws = torch.empty(int(calls().blm_linear_nll2_edges_ws_floats(M, V, K1, K2)), device=a.device, dtype=torch.float32)
    calls().blm_linear_nll2_edges(ptr(a), a.stride(0), ptr(dec.w1), dec.w1.stride(0), ptr(dec.b1), K1,
                                  ptr(b), b.stride(0), ptr(dec.w2), dec.w2.stride(0), ptr(dec.b2), K2, dec.alpha,
                                  ptr(en), ptr(et), ptr(nll), ptr(dec.wcat), 0 if dec.packed else 1, ptr(ws), M, E, V, stream())
    dec.packed = True
    return nll


def packing():
    return getattr(_PACK, "cur", None)


# ----------------------------------------------------------------------------
# incremental decoding: key/value cache, embedding at per-stream positions, log-softmax and sampling of decoder rows
# (csrc/decode.hip; the public API is bayeslms_amd/incremental.py)
# ----------------------------------------------------------------------------
class KVCache:
    """The device side of an incremental state: ``kv`` (layers, 2, n_cap, nhead, max_len, head_dim) fp32 -- the layout of
    blm_attn_decode -- and ``past`` (n_cap,) int32, the tokens each stream holds (the first N entries are live)."""

    def __init__(self, layers, n_cap, nhead, max_len, head_dim, device):
        self.layers, self.n_cap, self.nhead, self.max_len, self.head_dim = layers, n_cap, nhead, max_len, head_dim
        self.kv = torch.empty(layers, 2, n_cap, nhead, max_len, head_dim, device=device, dtype=torch.float32)
        self.past = torch.zeros(n_cap, device=device, dtype=torch.int32)


class cached_tokens:
    """Inference helper (bayeslms_amd/incremental.py): inside the context a Transformer forward over ``ids`` (Tq, N) is the
    continuation of N streams whose earlier tokens are in ``cache`` (a KVCache).  Layers are numbered by the order in which they
    call ``attention``; each appends its K / V rows at the streams' current lengths (blm_kv_append) and attends the cache
    (blm_attn_decode).  ``PositionalEncoding`` reads ``positions`` (the streams' start offsets) and embeds there (blm_embed_at).
    ``n_new`` ((N,) int32 device tensor, or None): a ragged chunk -- rows t >= n_new[n] are padding; ``sel`` ((R,) int64, the
    flat indices t * N + n of the real rows, ascending) then drops them after the embedding, so no token-wise op runs on padding;
    the attention core scatters into and gathers from the padded layout.  ``ctx_max``: the host-known largest stream length
    after this chunk.  The cache's lengths are not advanced here: the caller owns them."""

    def __init__(self, cache, Tq, N, ctx_max, n_new=None, sel=None):
        self.cache, self.T, self.N, self.ctx_max = cache, int(Tq), int(N), int(ctx_max)
        self.n_new, self.sel = n_new, sel
        self.positions = cache.past
        self.layer = 0

    def __enter__(self):
        if torch.is_grad_enabled():
            raise BayesLMError("ops.cached_tokens is an inference-only layout")
        if getattr(_PACK, "cur", None) is not None:
            raise BayesLMError("ops.cached_tokens does not nest")
        _PACK.cur = self
        return self

    def __exit__(self, *exc):
        _PACK.cur = None
        return False

    def pack(self, x):
        """(Tq, N, W) -> (R, 1, W) real rows of a ragged chunk; a full chunk keeps its (Tq, N, W) shape"""
        if self.sel is None:
            return x
        return x.reshape(self.T * self.N, x.shape[-1]).index_select(0, self.sel).unsqueeze(1)

    def unpack(self, xc):
        if self.sel is None:
            return xc
        out = xc.new_zeros(self.T * self.N, xc.shape[-1])
        out.index_copy_(0, self.sel, xc.reshape(-1, xc.shape[-1]))
        return out.view(self.T, self.N, -1)

    def attention(self, q, k, v, nhead):
        """q / k / v (packed rows, or q = the fused [q|k|v] projection and k = v = None) -> attention output, same row layout."""
        c = self.cache
        if self.layer >= c.layers:
            raise BayesLMError("cached_tokens: the model called attention %d times, the cache holds %d layers" % (self.layer + 1, c.layers))
        if k is None:
            qkv = _f32(self.unpack(q), "qkv").contiguous()
            d = qkv.shape[-1] // 3
            qq, kk, vv, ld = qkv, qkv[..., d:], qkv[..., 2 * d:], 3 * d
        else:
            qq, kk, vv = (_f32(self.unpack(t), n).contiguous() for t, n in ((q, "q"), (k, "k"), (v, "v")))
            d = ld = qq.shape[-1]
        if nhead != c.nhead or d != nhead * c.head_dim:
            raise BayesLMError("cached_tokens: layer %d has %d heads of %d, the cache %d of %d" % (self.layer, nhead, d // nhead, c.nhead,
                                                                                                  c.head_dim))
        kv = c.kv[self.layer]
        self.layer += 1
        L.require_gfx950()
        T, N, hd = self.T, self.N, c.head_dim
        calls().blm_kv_append(kk.data_ptr(), vv.data_ptr(), ld, ptr(kv), ptr(c.past), ptr(self.n_new), T, N, c.n_cap, nhead, c.max_len, hd, stream())
        nws = int(calls().blm_attn_decode_ws_floats(T, N, nhead, self.ctx_max, hd))
        ws = torch.empty(max(nws, 1), device=qq.device, dtype=torch.float32)
        out = torch.empty(T, N, d, device=qq.device, dtype=torch.float32)
        calls().blm_attn_decode(qq.data_ptr(), ld, ptr(kv), ptr(c.past), ptr(self.n_new), ptr(out), ptr(ws), nws, T, N, c.n_cap,
                                nhead, c.max_len, hd, self.ctx_max, stream())
        return self.pack(out)


def embed_at(ids, weight, pe, scale, pos0, x=None):
    """Inference only: out[t, n] = (ids ? weight[ids[t, n]] * scale : x[t, n]) + pe[pos0[n] + t] (blm_embed_at) -- the embedding
    and positional encoding of PositionalEncoding.embed / .forward at per-stream offsets ``pos0`` ((N,) int32 device)."""
    pe = _pe_table(pe, weight.shape[1] if weight is not None else x.shape[-1])
    if ids is not None:
        weight = _weight(weight, "weight")
        ids = dev_tensor(ids, "ids", torch.int64)
        T, N = ids.shape
        D, V = weight.shape[1], weight.shape[0]
    else:
        x = _f32(x, "x").contiguous()
        T, N, D = x.shape
        V = 0
    if pos0 is None or pos0.dtype != torch.int32 or pos0.numel() < N:
        raise BayesLMError("embed_at: pos0 must be (N,) int32")
    out = torch.empty(T, N, D, device=pe.device, dtype=torch.float32)
    L.require_gfx950()
    calls().blm_embed_at(ptr(ids), ptr(weight) if ids is not None else None, V, float(scale), ptr(x), ptr(pe), pe.shape[0],
                         ptr(pos0), ptr(out), T, N, D, stream())
    return out


def log_softmax_rows(x, V=None, out=None):
    """Row-wise log-softmax of the first V columns of the (R, >= V) matrix x (row stride honoured: padded logit rows) ->
    (R, V), or in place into ``out`` (blm_log_softmax_rows)."""
    x = _f32(x, "x")
    if x.dim() != 2 or x.stride(-1) != 1:
        raise BayesLMError("log_softmax_rows: a row-major (R, V) matrix expected")
    R, V = x.shape[0], int(V if V is not None else x.shape[1])
    out = torch.empty(R, V, device=x.device, dtype=torch.float32) if out is None else out
    L.require_gfx950()
    calls().blm_log_softmax_rows(ptr(x), x.stride(0), ptr(out), out.stride(0), R, V, stream())
    return out


class RowStats(NamedTuple):
    """What an evaluation keeps of each row of logits or log-probabilities (include/bayeslm.h, blm_row_stats)."""
    nll: Optional[torch.Tensor]   # (R,) float32 logsumexp - x[target]; NaN where the target is outside [0, V); None without targets
    conf: torch.Tensor            # (R,) float32 the largest probability of the row
    entropy: torch.Tensor         # (R,) float32 entropy of the row's distribution, nats
    pred: torch.Tensor            # (R,) int32 the lowest index that holds the maximum
    rank: Optional[torch.Tensor]  # (R,) int32 entries ahead of the target (0: it is the prediction; -1: no target); None without targets


def row_stats(x, targets=None, V=None):
    """NLL of the target, confidence, entropy, prediction and rank of the target for every row of the (R, >= V) matrix x of
    logits or log-probabilities -- the row is normalised by the kernel -- from one read of x (blm_row_stats; row stride honoured:
    padded rows, and a (R, V) view of padded rows, are read in place).  ``targets`` (R,) int64 or None.  A row that holds a NaN
    is NaN / -1 throughout.  Bit-identical run to run.  -> RowStats"""
    return _row_stats("row_stats", x, targets, V)


def _row_stats(who, x, targets, V, temps=None):
    """row_stats, and with ``temps`` (a blm_row_temps struct) row_stats_temps, whose float figures are (J, R)"""
    x, R, V, ld = _rows_in_place(who, "x", x, V, copy=True)
    tgt = _row_targets(who, targets, R)
    figure = lambda: torch.empty(*(() if temps is None else (temps.count,)), R, device=x.device, dtype=torch.float32)  # noqa: E731
    index = lambda: torch.empty(R, device=x.device, dtype=torch.int32)  # noqa: E731
    conf, entropy, pred = figure(), figure(), index()
    nll, rank = (None, None) if tgt is None else (figure(), index())
    if temps is None:
        out = RowStats(nll, conf, entropy, pred, rank)
    else:
        out = RowStatsTemps(nll, conf, entropy, None if tgt is None else figure(), pred, rank)
    if R == 0:
        return out
    L.require_gfx950()
    if temps is None:
        calls().blm_row_stats(ptr(x), ld, ptr(tgt), R, V, ptr(nll), ptr(conf), ptr(entropy), ptr(pred), ptr(rank), stream())
    else:
        calls().blm_row_stats_temps(ptr(x), ld, ptr(tgt), R, V, C.byref(temps), ptr(nll), ptr(conf), ptr(entropy), ptr(out.dnll),
                                    ptr(pred), ptr(rank), stream())
    return out


class RowStatsTemps(NamedTuple):
    """RowStats at J inverse temperatures (include/bayeslm.h, blm_row_stats_temps): the float fields are (J, R), row j the
    figures of the tempered distribution p ~ exp(betas[j] x)."""
    nll: Optional[torch.Tensor]   # (J, R) float32; None without targets
    conf: torch.Tensor            # (J, R) float32
    entropy: torch.Tensor         # (J, R) float32
    dnll: Optional[torch.Tensor]  # (J, R) float32 d nll / d beta = E_beta[x] - x[target]; None without targets
    pred: torch.Tensor            # (R,) int32, the same at every temperature
    rank: Optional[torch.Tensor]  # (R,) int32, likewise; None without targets


def row_temps(betas, what="row_stats_temps"):
    """The blm_row_temps struct of 1..8 positive finite inverse temperatures, each rounded to float32 once."""
    return _slots(what, L.RowTemps, "beta", "betas", betas, L.ROW_TEMPS_MAX, True, "inverse temperature", "blm_row_stats_temps")


def row_stats_temps(x, betas, targets=None, V=None):
    """ops.row_stats at the J = len(betas) <= 8 inverse temperatures ``betas`` (beta = 1 / T > 0) from ONE read of x
    (blm_row_stats_temps): per temperature the NLL of the target, the confidence, the entropy and d nll / d beta of the tempered
    distribution p ~ exp(beta x); prediction and rank do not depend on beta.  Argument rules of row_stats (row stride honoured).
    Temperature j's figures are bit-identical whatever else is in the list.  -> RowStatsTemps"""
    return _row_stats("row_stats_temps", x, targets, V, row_temps(betas))


class CacheScores(NamedTuple):
    """The two log-sums of the neural cache per theta and query (include/bayeslm.h, blm_cache_scores)."""
    lse: torch.Tensor    # (J, M) float32 log sum over the query's key range of exp(theta q.k); -inf over an empty range
    match: torch.Tensor  # (J, M) float32 the same sum over the keys whose label is the query's target; -inf without one


def cache_thetas(thetas, what="cache_scores"):
    """The blm_cache_thetas struct of 1..8 finite thetas >= 0, each rounded to float32 once."""
    return _slots(what, L.CacheThetas, "theta", "thetas", thetas, L.CACHE_THETAS_MAX, False, "theta", "blm_cache_scores")


def cache_scores(q, k, labels, targets, hi, thetas, window, lo=None):
    """Inference only: the neural cache's two log-sums for the M rows of ``q`` (M, K) over the Nk rows of ``k`` (Nk, K) at the
    J = len(thetas) <= 8 values ``thetas`` from the same dot products (blm_cache_scores: fp32 matrix cores, no score stored).
    Query m reads keys [max(lo[m], hi[m] - window, 0), min(hi[m], Nk)): ``hi`` (M,) and ``lo`` (M,) or None (= 0) are int32
    device arrays that the kernel clamps; ``labels`` (Nk,) and ``targets`` (M,) are int64.  Chunked over queries where q passes
    the 32-bit offset limit.  Bit-identical run to run.  -> CacheScores(lse, match), both (J, M)"""
    _inference_only("cache_scores", q, k)
    th = cache_thetas(thetas)
    J, window = th.count, int(window)
    if window < 1:
        raise BayesLMError("cache_scores: window = %d, at least one key is needed" % window)
    (q, M, K, ldq), (k, Nk, _, ldk) = (_rows_in_place("cache_scores", n, t, copy=True) for n, t in (("q", q), ("k", k)))
    if K < 1 or k.shape[1] != K:
        raise BayesLMError("cache_scores: q is (%d, %d) and k is (%d, %d): one width K >= 1 expected" % (M, K, Nk, k.shape[1]))
    labels = dev_tensor(labels.reshape(-1), "labels", torch.int64)
    targets = dev_tensor(targets.reshape(-1), "targets", torch.int64)
    hi = dev_tensor(hi.reshape(-1), "hi", torch.int32)
    lo = None if lo is None else dev_tensor(lo.reshape(-1), "lo", torch.int32)
    if labels.numel() != Nk or targets.numel() != M or hi.numel() != M or (lo is not None and lo.numel() != M):
        raise BayesLMError("cache_scores: %d labels for %d keys, %d targets, %d hi%s for %d queries"
                           % (labels.numel(), Nk, targets.numel(), hi.numel(), "" if lo is None else ", %d lo" % lo.numel(), M))
    lse, match = (torch.empty(J, M, device=q.device, dtype=torch.float32) for _ in range(2))
    if M == 0 or Nk == 0:  # nothing to launch: no query, or no key for any of them
        return CacheScores(lse.fill_(-math.inf), match.fill_(-math.inf))
    L.require_gfx950()
    chunks = _row_chunks(M, ldq)
    for r0, r1 in chunks:
        one = len(chunks) == 1
        ls, mt = (lse, match) if one else (torch.empty(J, r1 - r0, device=q.device, dtype=torch.float32) for _ in range(2))
        calls().blm_cache_scores(ptr(q[r0:r1]), ldq, ptr(k), ldk, ptr(labels), ptr(targets[r0:r1]),
                                 None if lo is None else ptr(lo[r0:r1]), ptr(hi[r0:r1]), window, r1 - r0, Nk, K, C.byref(th), ptr(ls),
                                 ptr(mt), None, stream())
        if not one:
            lse[:, r0:r1], match[:, r0:r1] = ls, mt
    return CacheScores(lse, match)


def cache_mix(nll_model, lse, match, lam):
    """The NLL of p = (1 - lam) p_model + lam p_cache with p_cache = exp(match - lse):
    -logaddexp(log(1 - lam) - nll_model, log(lam) + match - lse), elementwise over arrays of one shape (torch, not a kernel: a
    few passes over (tokens,) arrays).  Where lse = -inf (an empty cache) p = p_model and nll_model is returned; lam = 0
    returns nll_model bit for bit.  0 <= lam < 1."""
    lam = float(lam)
    if not 0.0 <= lam < 1.0:
        raise BayesLMError("cache_mix: lam = %r outside [0, 1)" % lam)
    if lam == 0.0:
        return nll_model
    log_cache = torch.where(torch.isneginf(match), match, match - lse)  # -inf - -inf never formed
    mixed = -torch.logaddexp(math.log1p(-lam) - nll_model, math.log(lam) + log_cache)
    return torch.where(torch.isneginf(lse), nll_model, mixed)


def _dyneval_flat(who, **arrays):
    """The flat operands of the dynamic-evaluation kernels: float32, contiguous, on this process's GPU, of one length (they
    are updated in place or read at the same index, so a copy of a strided one would be the wrong tensor) -> that length"""
    n = None
    for name, t in arrays.items():
        if not torch.is_tensor(t):
            raise BayesLMError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
        if dev_tensor(t, "%s: %s" % (who, name)) is not t:
            raise BayesLMError("%s: %s must be contiguous (it is used in place)" % (who, name))
        if n is None:
            n, first = t.numel(), name
        elif t.numel() != n:
            raise BayesLMError("%s: %s has %d elements, %s has %d" % (who, name, t.numel(), first, n))
    return n


def _dyneval_rate(who, name, v):
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0 and float(torch.tensor(v, dtype=torch.float32)) < math.inf):
        raise BayesLMError("%s: %s = %r is not a finite float32 number >= 0" % (who, name, v))
    return v


def dyneval_accum(ms, g):
    """ms += g * g over two flat float32 arrays of one length (blm_dyneval_accum): one window's share of the gradient
    statistics of dynamic evaluation.  In place; -> ms"""
    n = _dyneval_flat("dyneval_accum", ms=ms, g=g)
    L.require_gfx950()
    calls().blm_dyneval_accum(ptr(ms), ptr(g), n, stream())
    return ms


def dyneval_rms(ms, count):
    """-> (rms, mean): rms = sqrt(ms / count) and the DEVICE pair mean = [rbar, live] -- rbar the mean of rms over the live
    entries (ms > 0), live their number (blm_dyneval_rms: double partial sums in a fixed order, the same bits in every run).
    Raises when no entry is live (rbar = 0: the rms rule would divide by it); that check reads the pair back once."""
    n = _dyneval_flat("dyneval_rms", ms=ms)
    count = int(count)
    if count < 1:
        raise BayesLMError("dyneval_rms: count = %d, the statistics need at least one window" % count)
    L.require_gfx950()
    rms, mean = torch.empty_like(ms), torch.empty(2, device=ms.device, dtype=torch.float32)
    ws = torch.empty(L.DYNEVAL_RMS_WS_FLOATS, device=ms.device, dtype=torch.float32)
    calls().blm_dyneval_rms(ptr(ms), n, count, ptr(rms), ptr(mean), ptr(ws), stream())
    if not float(mean[1]) > 0.0:
        raise BayesLMError("dyneval_rms: no live entry among %d (every mean square is zero): rbar = 0 and the rms rule is undefined"
                           % n)
    return rms, mean


def dyneval_update(p, g, p0, lr, decay, rms=None, mean=None, eps=0.01, zero_grad=True):
    """The per-window update of dynamic evaluation over flat float32 arrays of one length, in place on ``p``
    (blm_dyneval_update, one pass): p <- p - step + d (p0 - p) with step = lr g, d = min(1, decay) (sgd rule: ``rms`` and
    ``mean`` None) or step = lr g / (rms + eps rbar), d = min(1, decay rms / rbar) (rms rule: both from dyneval_rms; rbar is read
    on the device).  ``zero_grad``: g = 0 in the same pass.  -> p"""
    if (rms is None) != (mean is None):
        raise BayesLMError("dyneval_update: rms and mean go together (both from dyneval_rms for the rms rule, neither for sgd)")
    arrays = dict(p=p, g=g, p0=p0) if rms is None else dict(p=p, g=g, p0=p0, rms=rms)
    n = _dyneval_flat("dyneval_update", **arrays)
    if mean is not None and (_dyneval_flat("dyneval_update", mean=mean) != 2):
        raise BayesLMError("dyneval_update: mean must hold 2 floats (rbar, live), got %d" % mean.numel())
    lr, decay, eps = (_dyneval_rate("dyneval_update", k, v) for k, v in (("lr", lr), ("decay", decay), ("eps", eps)))
    L.require_gfx950()
    calls().blm_dyneval_update(ptr(p), ptr(g), ptr(p0), ptr(rms), ptr(mean), n, lr, decay, eps, 1 if zero_grad else 0, stream())
    return p


def _swag_rows(who, name, t, n):
    """A (rows, n) float32 device matrix used in place (a row of it may start at any float) -> its row stride as the kernel
    takes it"""
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != n:
        raise BayesLMError("%s: %s must be a (rows, %d) matrix with unit inner stride" % (who, name, n))
    return _rows_in_place(who, name, t)[3]


def swag_collect(theta, mean, m2, count, dev_row=None):
    """One iterate into a SWAG posterior, in place over flat float32 arrays of one length (blm_swag_collect, one pass):
    Welford's update of ``mean`` and ``m2`` by ``theta`` as iterate number ``count`` (0: mean = theta, m2 = 0, and neither is read)
    and the deviation theta - mean' into ``dev_row`` (None: a diagonal posterior keeps none)."""
    arrays = dict(theta=theta, mean=mean, m2=m2) if dev_row is None else dict(theta=theta, mean=mean, m2=m2, dev_row=dev_row)
    n = _dyneval_flat("swag_collect", **arrays)
    count = int(count)
    if not 0 <= count < 1 << 24:
        raise BayesLMError("swag_collect: count = %d outside 0..2^24-1" % count)
    L.require_gfx950()
    calls().blm_swag_collect(ptr(theta), ptr(mean), ptr(m2), ptr(dev_row), n, count, stream())


def swag_draw(sample_ids, seed, a, b, inv_n, floor):
    """The blm_swag_draw struct of 1..8 sample ids; a, b, inv_n and floor are rounded to float32 once, here."""
    ids = [int(i) for i in sample_ids]
    if not 1 <= len(ids) <= L.SWAG_DRAWS_MAX or any(not 0 <= i < 1 << 32 for i in ids):
        raise BayesLMError("swag_sample: %d sample ids (%r): blm_swag_sample takes 1..%d per launch, each in 0..2^32-1"
                           % (len(ids), ids[:9], L.SWAG_DRAWS_MAX))
    d = L.SwagDraw()
    d.abi_version, d.count = L.ABI_VERSION, len(ids)
    for name, v, positive in (("a", a, False), ("b", b, False), ("inv_n", inv_n, True), ("var_floor", floor, False)):
        v = float(v)
        setattr(d, name, v if math.isfinite(v) else 0.0)  # ctypes rounds to float32
        got = getattr(d, name)
        if not (math.isfinite(v) and v >= 0.0 and got < math.inf and (got > 0.0 or not positive)):
            raise BayesLMError("swag_sample: %s = %r is not a finite float32 number %s 0" % (name, v, ">" if positive else ">="))
    for j, i in enumerate(ids):
        d.sample_id[j] = i
    d.rng = L.rng(seed, L.STREAM_SWAG, 0)
    return d


def swag_z2(sample_ids, seed, k_live, device):
    """(len(sample_ids), k_live) device array: row j the first k_live normals of the Philox stream (seed, STREAM_SWAG + 1,
    step = sample_ids[j]), as blm_philox_normal writes them."""
    z2 = torch.empty(len(sample_ids), k_live, device=device, dtype=torch.float32)
    for j, i in enumerate(sample_ids):
        r = L.rng(seed, L.STREAM_SWAG + 1, int(i))
        calls().blm_philox_normal(ptr(z2[j]), k_live, C.byref(r), stream())
    return z2


def swag_sample(out, mean, m2, sample_ids, seed, a, b, inv_n, floor, dev=None, k_live=0, z2=None):
    """Weight samples of a SWAG posterior into the rows of ``out`` (len(sample_ids) <= 8, P), all from one read of ``mean``,
    ``m2`` (P,) and the first ``k_live`` rows of ``dev`` (K, P) (blm_swag_sample):
    out[j] = mean + a sqrt(max(m2 inv_n, floor)) z1_j + b sum_k dev[k] z2[j, k], z1_j the Philox normals of (seed, STREAM_SWAG,
    step = sample_ids[j]).  ``z2`` (len(sample_ids), k_live): default swag_z2's.  Row j is a function of its own id alone: the
    same bits alone, in a longer list and at another slot.  -> out"""
    n = _dyneval_flat("swag_sample", mean=mean, m2=m2)
    ids = [int(i) for i in sample_ids]
    draw = swag_draw(ids, seed, a, b, inv_n, floor)
    ld_out = _swag_rows("swag_sample", "out", out, n)
    if out.shape[0] != len(ids):
        raise BayesLMError("swag_sample: %d rows of out for %d sample ids" % (out.shape[0], len(ids)))
    k_live, ld_dev = int(k_live), 0
    if not 0 <= k_live <= L.SWAG_RANK_MAX:
        raise BayesLMError("swag_sample: k_live = %d outside 0..%d" % (k_live, L.SWAG_RANK_MAX))
    L.require_gfx950()
    if k_live:
        if dev is None:
            raise BayesLMError("swag_sample: k_live = %d without deviation rows" % k_live)
        ld_dev = _swag_rows("swag_sample", "dev", dev, n)
        if dev.shape[0] < k_live:
            raise BayesLMError("swag_sample: k_live = %d of %d deviation rows" % (k_live, dev.shape[0]))
        z2 = swag_z2(ids, seed, k_live, mean.device) if z2 is None else dev_tensor(z2, "swag_sample: z2")
        if tuple(z2.shape) != (len(ids), k_live):
            raise BayesLMError("swag_sample: z2 is %s, (%d, %d) expected" % (tuple(z2.shape), len(ids), k_live))
    else:
        dev = z2 = None
    calls().blm_swag_sample(ptr(out), ld_out, ptr(mean), ptr(m2), ptr(dev), ld_dev, k_live, ptr(z2), n, C.byref(draw), stream())
    return out


def logp_avg_accum(logits, acc, s, S, targets=None, hsum=None, nll_s=None, V=None):
    """Sample ``s`` of ``S`` into the running model average of a chunk of rows (blm_logp_avg_accum): with logp = log-softmax of
    the first V columns of ``logits`` (R, >= V), ``acc`` (R, >= V) becomes logp at s = 0 (it is not read) and
    logaddexp(acc, logp) after, less log S at s = S - 1: log mean_s p_s once every sample is in.  ``hsum`` (R,) gathers the
    samples' entropies the same way; ``nll_s`` (S, R) gets row s = -logp[r, targets[r]] (0 for a target outside [0, V)).
    Row strides are honoured; both matrices are used in place.  The same bits in every run."""
    R, V, ld, lda = _rows_pair("logp_avg_accum", "logits", logits, "acc", acc, V, overlap=True)  # the library refuses overlap
    s, S = int(s), int(S)
    if not (1 <= S <= L.SWAG_SAMPLES_MAX and 0 <= s < S):
        raise BayesLMError("logp_avg_accum: sample %d of %d (1..%d samples)" % (s, S, L.SWAG_SAMPLES_MAX))
    if (targets is None) != (nll_s is None):
        raise BayesLMError("logp_avg_accum: targets and nll_s go together")
    tgt = _row_targets("logp_avg_accum", targets, R)
    if tgt is not None and (dev_tensor(nll_s, "logp_avg_accum: nll_s") is not nll_s or tuple(nll_s.shape) != (S, R)):
        raise BayesLMError("logp_avg_accum: nll_s must be a contiguous (%d, %d) matrix beside %d targets" % (S, R, R))
    if hsum is not None and (dev_tensor(hsum, "logp_avg_accum: hsum") is not hsum or hsum.numel() != R):
        raise BayesLMError("logp_avg_accum: hsum must be a contiguous array of %d" % R)
    if R == 0:
        return acc
    L.require_gfx950()
    calls().blm_logp_avg_accum(ptr(logits), ld, ptr(acc), lda, ptr(tgt), R, V, s, S, ptr(hsum), ptr(nll_s), stream())
    return acc


# ----------------------------------------------------------------------------
# last-layer Laplace posterior: the three row kernels of csrc/laplace.hip (definitions: include/bayeslm.h)
# ----------------------------------------------------------------------------
def laplace_curvature(logits, out=None, V=None):
    """a = p (1 - p), p = softmax of the first V columns of each row of ``logits`` (R, >= V) (blm_laplace_curvature): the diagonal
    Gauss-Newton factor of the decoder's Laplace posterior.  ``out`` None: a new (R, V) matrix; ``out`` the same tensor as
    ``logits``: in place; any other overlap is refused.  Row strides are honoured; where a row of ``out`` has room for them,
    the columns V .. Vq - 1 (V rounded up to 4) are written 0.  -> out"""
    who = "laplace_curvature"
    _, R, V, ld = _rows_in_place(who, "logits", logits, V)
    if out is None:
        out = torch.empty(R, V, device=logits.device, dtype=torch.float32)
    _, Ro, _, lda = _rows_in_place(who, "out", out, V)
    if Ro != R:
        raise BayesLMError("%s: logits has %d rows, out %d" % (who, R, Ro))
    if R == 0:
        return out
    L.require_gfx950()
    calls().blm_laplace_curvature(ptr(logits), ld, ptr(out), lda, R, V, stream())
    return out


class LaplaceRowStats(NamedTuple):
    """RowStats of the closed-form Laplace predictive (include/bayeslm.h, blm_laplace_row_stats), and the variance figure."""
    nll: Optional[torch.Tensor]   # (R,) float32; None without targets
    conf: torch.Tensor            # (R,) float32
    entropy: torch.Tensor         # (R,) float32
    pred: torch.Tensor            # (R,) int32
    rank: Optional[torch.Tensor]  # (R,) int32; None without targets
    vbar: torch.Tensor            # (R,) float32 sum_v ptilde_v var_v


def laplace_row_stats(z, var, targets=None, link="probit", V=None):
    """ops.row_stats of y = link(z, var) for every row of the logit means ``z`` and variances ``var`` (R, >= V), y formed in
    registers from one read of each (blm_laplace_row_stats).  ``link``: 'probit', y = z / sqrt(1 + pi / 8 var), or 'expexp',
    y = z + var / 2.  A row with a NaN or a var that is negative or not finite is NaN / -1 throughout.  -> LaplaceRowStats"""
    who = "laplace_row_stats"
    if link not in L.LAPLACE_LINKS:
        raise BayesLMError("%s: link %r is neither 'probit' nor 'expexp' (the 'mc' link is laplace_mc_rows)" % (who, link))
    R, V, ldz, ldv = _rows_pair(who, "z", z, "var", var, V)
    dev = z.device
    conf, entropy, vbar = (torch.empty(R, device=dev, dtype=torch.float32) for _ in range(3))
    pred = torch.empty(R, device=dev, dtype=torch.int32)
    tgt = _row_targets(who, targets, R)
    nll = rank = None
    if tgt is not None:
        nll = torch.empty(R, device=dev, dtype=torch.float32)
        rank = torch.empty(R, device=dev, dtype=torch.int32)
    if R:
        L.require_gfx950()
        calls().blm_laplace_row_stats(ptr(z), ldz, ptr(var), ldv, ptr(tgt), R, V, L.LAPLACE_LINKS[link], ptr(nll), ptr(conf),
                                      ptr(entropy), ptr(pred), ptr(rank), ptr(vbar), stream())
    return LaplaceRowStats(nll, conf, entropy, pred, rank, vbar)


class LaplaceMcRows(NamedTuple):
    """The Monte-Carlo Laplace predictive per row (include/bayeslm.h, blm_laplace_mc_rows)."""
    bma_nll: Optional[torch.Tensor]  # (R,) float32 -log pbar[target]; None without targets
    nll_s: Optional[torch.Tensor]    # (R, S) float32, a view of the kernel's (S, R); None without targets
    h_pred: torch.Tensor             # (R,) float32 entropy of pbar
    mi: torch.Tensor                 # (R,) float32 mean_s KL(p_s || pbar)
    conf: torch.Tensor               # (R,) float32 max pbar
    pred: torch.Tensor               # (R,) int32
    rank: Optional[torch.Tensor]     # (R,) int32; None without targets


def laplace_mc_rows(z, var, samples, seed, targets=None, row0=0, V=None):
    """The model average over S = ``samples`` (1..32) logit samples z + sqrt(var) eps for every row of ``z`` and ``var``
    (R, >= V) (blm_laplace_mc_rows); eps of row r, column v and sample s is element ((row0 + r) Vq + v) of the Philox normal
    stream (seed, STREAM_LAPLACE, step = s), Vq = V rounded up to 4, made in registers.  ``row0``: the global index of the first
    row, so that a text gives the same figures however it is chunked.  -> LaplaceMcRows"""
    who = "laplace_mc_rows"
    S, row0 = int(samples), int(row0)
    if not 1 <= S <= L.LAPLACE_SAMPLES_MAX:
        raise BayesLMError("%s: samples = %d outside 1..%d" % (who, S, L.LAPLACE_SAMPLES_MAX))
    if not 0 <= row0 <= 1 << 40:
        raise BayesLMError("%s: row0 = %d outside 0..2^40" % (who, row0))
    R, V, ldz, ldv = _rows_pair(who, "z", z, "var", var, V)
    dev = z.device
    h_pred, mi, conf = (torch.empty(R, device=dev, dtype=torch.float32) for _ in range(3))
    pred = torch.empty(R, device=dev, dtype=torch.int32)
    tgt = _row_targets(who, targets, R)
    bma = nll_s = rank = None
    if tgt is not None:
        bma = torch.empty(R, device=dev, dtype=torch.float32)
        nll_s = torch.empty(S, R, device=dev, dtype=torch.float32)
        rank = torch.empty(R, device=dev, dtype=torch.int32)
    if R:
        L.require_gfx950()
        r = L.rng(seed, L.STREAM_LAPLACE, 0)
        calls().blm_laplace_mc_rows(ptr(z), ldz, ptr(var), ldv, ptr(tgt), R, V, S, C.byref(r), row0, ptr(bma), ptr(nll_s), ptr(h_pred),
                                    ptr(mi), ptr(conf), ptr(pred), ptr(rank), stream())
    return LaplaceMcRows(bma, None if nll_s is None else nll_s.t(), h_pred, mi, conf, pred, rank)


def sample_rows(x, temperature=0.0, seed=0, stream_id=0, step=0, top_k=0, top_p=1.0):
    """One id per row of the (R, V) matrix x (blm_sample_rows): argmax at temperature 0, else Gumbel-max over x / temperature
    with Philox noise keyed by (seed, stream_id, step) and the (row, column) counter.  -> (R,) int64
    ``top_k`` > 0 and / or ``top_p`` < 1 restrict the draw to the top_k best entries and to the shortest prefix of the order
    (value descending, index ascending) whose softmax(x / temperature) mass reaches top_p (blm_sample_rows_filtered: the same
    noise, so the draw is unchanged whenever it falls inside the allowed set)."""
    x = _f32(x, "x")
    if x.dim() != 2 or x.stride(-1) != 1:
        raise BayesLMError("sample_rows: a row-major (R, V) matrix expected")
    top_k, top_p = int(top_k), float(top_p)
    if top_k < 0 or not 0.0 < top_p <= 1.0:
        raise BayesLMError("sample_rows: top_k >= 0 (0: no limit) and top_p in (0, 1] expected, got %d and %g" % (top_k, top_p))
    out = torch.empty(x.shape[0], device=x.device, dtype=torch.int64)
    r = L.rng(seed, stream_id, step)
    L.require_gfx950()
    if top_k == 0 and top_p == 1.0:
        calls().blm_sample_rows(ptr(x), x.stride(0), x.shape[0], x.shape[1], float(temperature), C.byref(r), ptr(out), stream())
    else:
        calls().blm_sample_rows_filtered(ptr(x), x.stride(0), x.shape[0], x.shape[1], float(temperature), top_k, top_p,
                                         C.byref(r), ptr(out), stream())
    return out


class SpecAccept(NamedTuple):
    """What one verification of G drafted words per stream decides (include/bayeslm.h, blm_spec_accept)."""
    n_acc: torch.Tensor   # (N,) int32: the drafted words kept, the smallest t with accept[t, n] = 0 (G: all of them)
    token: torch.Tensor   # (N,) int64: the word emitted behind them, cand[n_acc[n], n]
    accept: torch.Tensor  # (G, N) uint8: every position's own flag, whether or not an earlier one rejected
    cand: torch.Tensor    # (G + 1, N) int64: every position's own candidate; -1 in a row that holds a NaN


def _spec_rows(t, name, V):
    """(T, N, V) float32 rows for blm_spec_accept -> (tensor, row stride): a view whose rows lie at one stride >= V (padded
    vocabulary rows, a column slice) is read in place, anything else through its contiguous copy."""
    if t.dim() != 3 or t.shape[2] != V:
        raise BayesLMError("spec_accept: %s must be (T, N, V = %d), got %s" % (name, V, tuple(t.shape)))
    T, N = t.shape[0], t.shape[1]
    ld = t.stride(1) if N > 1 else (t.stride(0) if T > 1 else V)
    if t.dtype == torch.float32 and t.stride(2) == 1 and ld >= V and (T == 1 or t.stride(0) == N * ld) and not t.is_contiguous():
        dev_tensor(t[:1, :1], name)  # the device checks of the product path; the view itself is what the kernel reads
        return t, ld
    return _f32(t, name), V


def spec_accept(logp, logq, draft, temperature=1.0, seed=0, stream_id=0, step=0):
    """The accept / reject / residual-draw step of speculative sampling (blm_spec_accept; definitions: include/bayeslm.h): the
    target's rows ``logp`` (G + 1, N, V) and the draft's rows ``logq`` (G, N, V) -- logits or log-probabilities, the kernel
    normalises -- against the drafted ids ``draft`` (G, N) int64.  temperature 0 is greedy and takes logq = None.  The Philox
    noise is keyed by (seed, stream_id, step), which MUST differ from the (stream_id, step) under which the drafted ids were drawn:
    otherwise the residual draw reuses the draft's noise and the emitted words are no longer distributed as the target.
    -> SpecAccept(n_acc, token, accept, cand)"""
    tau = float(temperature)
    t32 = C.c_float(tau).value if math.isfinite(tau) else tau  # what the entry point receives
    if not (tau >= 0.0 and math.isfinite(t32)):
        raise BayesLMError("spec_accept: temperature = %r: a finite value >= 0 expected" % (temperature,))
    if tau > 0.0 and (t32 == 0.0 or not math.isfinite(C.c_float(1.0 / t32).value)):
        raise BayesLMError("spec_accept: 1 / temperature (%r) is no finite float32" % (temperature,))
    tau = t32
    if not torch.is_tensor(logp) or logp.dim() != 3 or logp.shape[0] < 2 or logp.shape[1] < 1 or logp.shape[2] < 1:
        raise BayesLMError("spec_accept: logp must be (G + 1, N, V) with G >= 1, N >= 1 and V >= 1")
    G, N, V = logp.shape[0] - 1, logp.shape[1], logp.shape[2]
    if logq is None and tau > 0.0:
        raise BayesLMError("spec_accept: logq may be None at temperature 0 only")
    logp, ldp = _spec_rows(logp, "logp", V)
    ldq = V
    if logq is not None:
        if not torch.is_tensor(logq) or tuple(logq.shape) != (G, N, V):
            raise BayesLMError("spec_accept: logq must be (G, N, V) = (%d, %d, %d)" % (G, N, V))
        logq, ldq = _spec_rows(logq, "logq", V)
    if not torch.is_tensor(draft) or tuple(draft.shape) != (G, N):
        raise BayesLMError("spec_accept: draft must be (G, N) = (%d, %d) int64" % (G, N))
    draft = dev_tensor(draft, "draft", torch.int64)
    dev = logp.device
    accept = torch.empty(G, N, device=dev, dtype=torch.uint8)
    cand = torch.empty(G + 1, N, device=dev, dtype=torch.int64)
    n_acc = torch.empty(N, device=dev, dtype=torch.int32)
    token = torch.empty(N, device=dev, dtype=torch.int64)
    r = L.rng(seed, stream_id, step)
    L.require_gfx950()
    calls().blm_spec_accept(ptr(logp), ldp, ptr(logq), ldq, ptr(draft), G, N, V, tau, C.byref(r), ptr(accept), ptr(cand), ptr(n_acc),
                            ptr(token), stream())
    return SpecAccept(n_acc, token, accept, cand)


def topk_rows(x, k):
    """The k best entries of every row of the (R, V) matrix x, best first (blm_topk_rows): value descending, then index
    ascending, NaN below -inf; values are copied bit for bit.  1 <= k <= min(V, _lib.TOPK_MAX).
    -> (vals (R, k) float32, ids (R, k) int64)"""
    x, R, V, ld = _rows_in_place("topk_rows", "x", x, copy=True)  # padded odd-vocabulary rows are read in place
    k = int(k)
    vals = torch.empty(R, k, device=x.device, dtype=torch.float32)
    ids = torch.empty(R, k, device=x.device, dtype=torch.int64)
    L.require_gfx950()
    calls().blm_topk_rows(ptr(x), ld, R, V, k, ptr(vals), ptr(ids), stream())
    return vals, ids


def beam_select(cand_vals, cand_ids, score, finished, beams, eos):
    """One beam-search step over groups of ``beams`` streams (blm_beam_select): cand_vals / cand_ids (G * beams, k) from
    topk_rows, score (G * beams,) float32 and finished (G * beams,) uint8 before the step.
    -> (score, finished, parent (global stream index), token) after it, each (G * beams,)"""
    cand_vals = dev_tensor(cand_vals, "cand_vals")
    cand_ids = dev_tensor(cand_ids, "cand_ids", torch.int64)
    score = dev_tensor(score, "score")
    finished = dev_tensor(finished, "finished", torch.uint8)
    n, B = score.numel(), int(beams)
    if cand_vals.dim() != 2 or cand_vals.shape != cand_ids.shape or cand_vals.shape[0] != n or finished.numel() != n or \
            B < 1 or n % B:
        raise BayesLMError("beam_select: (G * beams, k) candidates and (G * beams,) score / finished expected")
    score_out, fin_out = torch.empty_like(score), torch.empty_like(finished)
    parent = torch.empty(n, device=score.device, dtype=torch.int64)
    token = torch.empty(n, device=score.device, dtype=torch.int64)
    L.require_gfx950()
    calls().blm_beam_select(ptr(cand_vals), ptr(cand_ids), ptr(score), ptr(finished), n // B, B, cand_vals.shape[1], int(eos),
                            ptr(score_out), ptr(fin_out), ptr(parent), ptr(token), stream())
    return score_out, fin_out, parent, token


class BeamPool:
    """The finished-hypothesis pool of beam_select_pool (blm_beam_pool, include/bayeslm.h): ``slots`` entries for each of
    ``groups`` searches, every array a view of ONE device allocation.  Slots [0, count[g]) of group g are its entries best first
    (norm descending, then insertion order); the rest is never read.  A new pool is empty."""
    FIELDS = (("parent", torch.int64, True), ("inserted", torch.int64, False), ("norm", torch.float32, True),
              ("raw", torch.float32, True), ("len", torch.int32, True), ("step", torch.int32, True), ("count", torch.int32, False),
              ("finished", torch.uint8, True))  # widest elements first: every view is aligned to its element

    def __init__(self, groups, slots, device):
        self.groups, self.slots = int(groups), int(slots)
        if self.groups < 1 or not 1 <= self.slots <= L.TOPK_MAX:
            raise BayesLMError("BeamPool: groups >= 1 and 1 <= slots <= BLM_TOPK_MAX = %d expected, got %d and %d"
                               % (L.TOPK_MAX, self.groups, self.slots))
        sizes = [(self.groups * (self.slots if per_slot else 1)) * torch.empty(0, dtype=dt).element_size()
                 for _, dt, per_slot in self.FIELDS]
        self.buf = torch.zeros(sum(sizes), dtype=torch.uint8, device=device)
        at = 0
        for (name, dt, per_slot), nbytes in zip(self.FIELDS, sizes):
            v = self.buf[at:at + nbytes].view(dt)
            setattr(self, name, v.view(self.groups, self.slots) if per_slot else v)
            at += nbytes
        self.args = L.BeamPoolArgs(L.ABI_VERSION, self.slots, *(ptr(getattr(self, n)) for n in
                                                              ("norm", "raw", "len", "step", "parent", "finished", "count", "inserted")))

    def host(self):
        """-> dict of host arrays, one copy of the allocation (synchronises)"""
        flat = self.buf.cpu().numpy()
        out, at = {}, 0
        for name, dt, per_slot in self.FIELDS:
            n = self.groups * (self.slots if per_slot else 1)
            npdt = {torch.int64: "int64", torch.float32: "float32", torch.int32: "int32", torch.uint8: "uint8"}[dt]
            a = flat[at:at + n * torch.empty(0, dtype=dt).element_size()].view(npdt)
            out[name] = a.reshape(self.groups, self.slots) if per_slot else a
            at += a.nbytes
        return out


def beam_inv_norm(length, length_penalty):
    """float32(1 / length ** a) as beam_select_pool takes it: formed in float64 and rounded once, returned as a Python float"""
    import numpy as np
    return float(np.float32(1.0 / float(length) ** float(length_penalty)))


def beam_select_pool(cand_vals, cand_ids, score, live, beams, vocab, eos, step, length, min_len, inv_norm, inv_norm_max, flush, pool):
    """One beam-search step with a finished-hypothesis pool over groups of ``beams`` streams (blm_beam_select_pool, which has the
    semantics): cand_vals / cand_ids (G * beams, k >= min(2 * beams, vocab)) from topk_rows, score (G * beams,) float32 and
    live (G * beams,) uint8 before the step; ``length`` the length of a hypothesis that ends at this step, inv_norm /
    inv_norm_max from beam_inv_norm; ``pool`` a BeamPool of G groups, updated in place.
    -> (score, live, parent (global stream index), token, done (G,) uint8, all_done (1,) uint8) after it"""
    cand_vals = dev_tensor(cand_vals, "cand_vals")
    cand_ids = dev_tensor(cand_ids, "cand_ids", torch.int64)
    score = dev_tensor(score, "score")
    live = dev_tensor(live, "live", torch.uint8)
    n, B = score.numel(), int(beams)
    if cand_vals.dim() != 2 or cand_vals.shape != cand_ids.shape or cand_vals.shape[0] != n or live.numel() != n or B < 1 or n % B:
        raise BayesLMError("beam_select_pool: (G * beams, k) candidates and (G * beams,) score / live expected")
    if not isinstance(pool, BeamPool) or pool.groups != n // B or pool.buf.device != score.device:
        raise BayesLMError("beam_select_pool: a BeamPool of %d groups on the candidates' device expected" % (n // B))
    score_out, live_out = torch.empty_like(score), torch.empty_like(live)
    parent = torch.empty(n, device=score.device, dtype=torch.int64)
    token = torch.empty(n, device=score.device, dtype=torch.int64)
    done = torch.empty(n // B + 1, device=score.device, dtype=torch.uint8)  # the groups' flags, then the one for all of them
    L.require_gfx950()
    calls().blm_beam_select_pool(ptr(cand_vals), ptr(cand_ids), ptr(score), ptr(live), n // B, B, cand_vals.shape[1], int(vocab),
                                 int(eos), int(step), int(length), int(min_len), float(inv_norm), float(inv_norm_max), int(bool(flush)),
                                 C.byref(pool.args), ptr(score_out), ptr(live_out), ptr(parent), ptr(token), ptr(done),
                                 ptr(done) + n // B, stream())
    return score_out, live_out, parent, token, done[:n // B], done[n // B:]


def kv_gather(src, dst, idx, n_src, outer, nhead, max_len, head_dim, len_src=None, len_dst=None):
    """Beam prune / fork of a state laid out [outer][n_cap][nhead][max_len][head_dim] (blm_kv_gather, one launch): stream j of
    ``dst`` continues stream idx[j] of ``src``; with lengths, only each panel's live prefix is copied and len_dst[j] = len_src[idx[j]]."""
    n_cap = src.numel() // (outer * nhead * max_len * head_dim)
    if dst.numel() != src.numel() or n_cap * outer * nhead * max_len * head_dim != src.numel():
        raise BayesLMError("kv_gather: source and destination must be two states of the same shape")
    idx = dev_tensor(idx, "idx", torch.int64)
    L.require_gfx950()
    calls().blm_kv_gather(ptr(src), ptr(dst), ptr(idx), ptr(len_src), ptr(len_dst), idx.numel(), int(n_src), n_cap, outer, nhead,
                          max_len, head_dim, stream())
    return dst


class state_tap:
    """Inference helper: inside the context every fused LSTM layer forward also records its (h, c) AFTER the time
    steps ``idx`` (int64 device tensor) -- the scorer walks the carry chain of a whole n-best file as one long B = 1
    sequence and reads the states at the utterance boundaries (compute_sentence_scores.py).  ``layers`` holds one
    (h (n,B,H), c (n,B,H)) pair per layer call, in call order; step-wise cells do not report (the caller checks)."""

    def __init__(self, idx):
        self.idx = idx + 1  # row t+1 of the (T+1,B,H) state buffers = state after step t
        self.layers = []

    def __enter__(self):
        global _STATE_TAP
        _STATE_TAP = self
        return self

    def __exit__(self, *exc):
        global _STATE_TAP
        _STATE_TAP = None
        return False


def _bias_pair_grads(b_refs, dbs, needs):
    """b_ih and b_hh of an LSTM layer receive the same gradient ``db`` (one per layer in ``dbs``; ``b_refs`` the (b_ih, b_hh)
    parameters layer by layer).  Leaf biases take it in place -- ONE launch for all of them (blm_init_multi: grad = grad + db) --
    and autograd gets None; anything else gets db itself.  -> the values to return, in b_refs' order."""
    items, out, told = [], [], []
    for i, b in enumerate(b_refs):
        db = dbs[i // 2]
        if not needs[i]:
            out.append(None)
        elif b.is_leaf and b.is_contiguous() and b.dtype == torch.float32:
            g = _grad_buf(b)
            items.append((g, g, db))
            told.append(b)
            out.append(None)
        else:
            out.append(db)
    # a cell that passes ONE parameter as both biases (VLSTMCell / GPLSTMCell add bias_ih twice, model.py:2519, :1750-1752) gets
    # db twice: the two updates of one buffer must not share a launch
    while items:
        seen, now, later = set(), [], []
        for it in items:
            (later if it[0].data_ptr() in seen else now).append(it)
            seen.add(it[0].data_ptr())
        _init_multi(now)
        items = later
    _notify(*told)
    return out


def _new(dev, *shape):
    """Uninitialised fp32 scratch on ``dev``: every element is written by a kernel before it is read."""
    return torch.empty(*shape, device=dev, dtype=torch.float32)


class _LSTMLayer(torch.autograd.Function):
    """One layer over T steps.  Input GEMM batched over T (M = T*B), recurrent GEMM + fused cell per
    step.  Weights arrive already sampled (W = mu + noise on the gate rows)."""

    @staticmethod
    def forward(ctx, x, h0, c0, w_ih, w_hh, b_ih, b_hh, noise_rows=None):
        x = _f32(x, "x")
        T, B, E = x.shape
        if noise_rows is not None:  # (T, H): row t is added to every batch row of h_t (VLSTMCell)
            noise_rows = _f32(noise_rows, "noise_rows")
        H = w_hh.shape[1]
        G = 4 * H
        dev = x.device
        bias = _new(dev, G)
        hs = _new(dev, T + 1, B, H)
        cs = _new(dev, T + 1, B, H)
        _init_multi([(bias, b_ih, b_hh), (hs[0], h0, None), (cs[0], c0, None)])  # one launch: b_ih + b_hh, the initial state
        xw = _new(dev, T, B, G)
        gemm(L.GEMM_NT, x, w_ih, xw, T * B, G, E, E, E, G, epilogue=L.EPI_BIAS, bias=bias)
        ga = _new(dev, T, B, G)
        st = stream()
        # one launch per step (recurrent product + cell, blm_lstm_step_fwd) when the shape allows it,
        # else skinny GEMM + cell kernel
        fused_step = H % 32 == 0 and w_hh.data_ptr() % 16 == 0 and hs.data_ptr() % 16 == 0 and w_hh.is_contiguous()
        if fused_step and not torch.is_grad_enabled() and B >= _UNFUSED_STEP_B:
            # wide inference batches (the scorer packs hundreds of hypotheses per step): the fused step kernel re-reads W_hh
            # once per 32 batch rows and runs at 0.57 of the matrix peak there; the tiled GEMM + cell kernel pair is faster
            # from B ~ 200 on (n-best rescoring 64.5 k -> 70-72 k hypotheses/s)
            fused_step = False
        if fused_step:  # the whole layer from one call: T launches issued by the library
            ev = _timer_start("lstm_seq_fwd T=%d", T)
            calls().blm_lstm_seq_fwd(ptr(xw), ptr(w_hh), ptr(hs), ptr(cs), ptr(ga), ptr(noise_rows), T, B, H, st)
            ev.record()
        else:
            hw = _new(dev, B, G)
            for t in range(T):
                gemm(L.GEMM_NT, hs[t], w_hh, hw, B, G, H, H, H, G)
                calls().blm_lstm_cell_fwd(ptr(xw[t]), ptr(hw), ptr(cs[t]), ptr(hs[t + 1]), ptr(cs[t + 1]), ptr(ga[t]), B, H, st)
                if noise_rows is not None:
                    calls().blm_add_rowvec(ptr(hs[t + 1]), ptr(noise_rows[t]), B, H, st)
        if _STATE_TAP is not None:
            _STATE_TAP.layers.append((hs.index_select(0, _STATE_TAP.idx), cs.index_select(0, _STATE_TAP.idx)))
        ctx.save_for_backward(x, hs, cs, ga, w_ih, w_hh)
        ctx.w_refs = (w_ih, w_hh)  # the parameter objects themselves (their .grad is the accumulation target)
        ctx.b_refs = (b_ih, b_hh)
        ctx.has_noise = noise_rows is not None
        ctx.set_materialize_grads(False)  # the final states usually feed nothing: their gradients arrive as None, not as zero fills
        return hs[1:], hs[T], cs[T]

    @staticmethod
    def backward(ctx, dy, dhT, dcT):
        x, hs, cs, ga, w_ih, w_hh = ctx.saved_tensors
        T, B, E = x.shape
        H = w_hh.shape[1]
        G = 4 * H
        dev = x.device
        dy = torch.zeros(T, B, H, device=dev, dtype=torch.float32) if dy is None else _f32(dy, "dy")
        dgates = _new(dev, T, B, G)
        st = stream()
        dh = _new(dev, B, H)
        dcs = _new(dev, 2, B, H)  # ping-pong dc buffers
        db = _new(dev, G)
        _init_multi([(dh, dhT, None), (dcs[0], dcT, None), (db, None, None)])  # one launch: incoming state gradients (or zeros), db = 0
        fused_step = (H % 32 == 0 and w_hh.is_contiguous() and w_hh.data_ptr() % 16 == 0 and dgates.data_ptr() % 16 == 0)
        noise = getattr(ctx, "has_noise", False)
        # dhr[t] = gradient reaching h_t from step t+1 (dhr[T-1] = dhT); kept for every step only when the
        # additive noise rows need their gradient (column sums of dhr + dy)
        dhr = torch.zeros(T, B, H, device=dev, dtype=torch.float32) if (noise or not fused_step) else None
        if dhr is not None:
            dhr[T - 1].copy_(dh)
        if fused_step:
            # one launch per step: dh_{t-1} = dgates_t . W_hh on the matrix cores with the cell backward
            # of step t-1 fused behind it (blm_lstm_step_bwd); W_hh is transposed once per layer
            w_t = _new(dev, H, G)
            calls().blm_transpose(ptr(w_hh), ptr(w_t), G, H, st)
            ev = _timer_start("lstm_seq_bwd T=%d", T)
            # the whole chain from one call (step T-1: the plain cell backward; every earlier step one fused launch)
            calls().blm_lstm_seq_bwd(ptr(dh), ptr(dy), ptr(cs), ptr(ga), ptr(w_t), ptr(dgates), ptr(dcs), 0,
                                     ptr(dhr) if noise else None, T, T, 0, B, H, st)
            k = T & 1
            dh = _new(dev, B, H)
            calls().blm_lstm_step_bwd(ptr(dgates[0]), ptr(w_t), None, None, None, None, None, None, None, ptr(dh), B, H, st)
            ev.record()
            dc = dcs[k]
        else:
            # recurrent dh of every step accumulates (split-K atomics) into one pre-zeroed buffer: a
            # single memset per layer instead of one in front of every skinny GEMM
            dh0 = torch.zeros(B, H, device=dev, dtype=torch.float32)
            for t in range(T - 1, -1, -1):
                k = (T - 1 - t) & 1
                calls().blm_lstm_cell_bwd2(ptr(dhr[t]), ptr(dy[t]), ptr(dcs[k]), ptr(cs[t]), ptr(cs[t + 1]), ptr(ga[t]),
                                           ptr(dgates[t]), ptr(dcs[k ^ 1]), B, H, st)
                gemm(L.GEMM_NN, dgates[t], w_hh, dhr[t - 1] if t > 0 else dh0, B, H, G, G, H, H, accumulate=True)
            dh = dh0
            dc = dcs[T & 1]
        d_noise = None
        if noise:  # noise row t was added to every batch row of h_t: its gradient is the column sum of dh_t
            d_noise = _new(dev, T, H)
            tot = dhr + dy
            for t in range(T):
                _colsum_into(tot[t], B, H, d_noise[t], accumulate=False)
        dx = torch.empty_like(x)
        gemm(L.GEMM_NN, dgates, w_ih, dx, T * B, E, G, G, E, E)
        # leaf weights (nn.LSTM-style parameters) accumulate straight into .grad like every other wgrad of the engine -- returned
        # to autograd they cost an AccumulateGrad add over 16.8 MB each at H = 1024 (~10 us per weight and step); sampled
        # (non-leaf) weights of Bayes2LSTM get a fresh gradient tensor for their sampling node
        w_ih_p, w_hh_p = ctx.w_refs
        dw_ih = dw_hh = None
        if ctx.needs_input_grad[3]:
            buf_ih, acc_ih, dw_ih = _wgrad_target(w_ih_p)
            # the bias gradient = column sums of dgates, taken from the A tiles this weight-gradient GEMM stages anyway
            gemm(L.GEMM_TN, dgates, x, buf_ih, G, E, T * B, G, E, E, accumulate=acc_ih, colsum_a=db)
        else:
            _colsum_into(dgates, T * B, G, db, accumulate=False)
        if ctx.needs_input_grad[4]:
            buf_hh, acc_hh, dw_hh = _wgrad_target(w_hh_p)
            gemm(L.GEMM_TN, dgates, hs, buf_hh, G, H, T * B, G, H, H, accumulate=acc_hh)  # hs[0:T] = h_{t-1}
        _notify(w_ih_p, w_hh_p)
        db_ih, db_hh = _bias_pair_grads(ctx.b_refs, [db], ctx.needs_input_grad[5:7])
        return dx, dh, dc, dw_ih, dw_hh, db_ih, db_hh, d_noise


def _pad_gate_blocks(t, H, Hp, cols=False):
    """(4H, ...) -> (4Hp, ...): gate block g = rows [g H, (g + 1) H) moves to [g Hp, g Hp + H), zeros behind it (``cols``: the last
    dimension H -> Hp as well).  Differentiable (F.pad): its backward is the slice that drops the padding's gradient."""
    t4 = t.reshape(4, H, *t.shape[1:])
    pad = [0, Hp - H] if t4.dim() == 2 else ([0, Hp - H if cols else 0] + [0, 0] * (t4.dim() - 3) + [0, Hp - H])
    return torch.nn.functional.pad(t4, pad).reshape(4 * Hp, *([Hp] if cols else t.shape[1:]))


_PAD_HIDDEN_FROM = 64  # smaller layers stay on the GEMM + cell composition (padding 8 units to 32 would quadruple them)


def lstm_layer(x, h0, c0, w_ih, w_hh, b_ih, b_hh, noise_rows=None):
    """One LSTM layer over T steps.  ``noise_rows`` (T, H), optional: row t is added to every batch row
    of h_t after the cell and carried into step t+1 (VLSTMCell, reference model.py:2523-2527).

    A hidden size that is not a multiple of 32 (the classic word-language-model sizes: 200, 650, 1500 -- train.py's own default is
    200) does not fit the fused step kernels' tiles and used to fall back to one skinny GEMM + one cell kernel per step: 1.4-1.9 x
    the step time of the next multiple of 32 (tools/lstm_hidden_size_probe.py).  It is zero-padded to that multiple instead: padded
    units have zero weights and a zero bias, so their gates are (1/2, 1/2, 0, 1/2), their cell and output stay exactly 0, and they
    feed nothing back (their columns of W_hh are zero) -- the real units compute what they computed before.  The padding and the
    slices that undo it are torch ops: autograd routes the gradients back to the unpadded parameters."""
    H = w_hh.shape[1]
    B = x.shape[1] if x.dim() == 3 else 0
    if (H % 32 and H >= _PAD_HIDDEN_FROM and x.dim() == 3 and w_hh.dim() == 2 and w_hh.shape[0] == 4 * H
            and (torch.is_grad_enabled() or B < _UNFUSED_STEP_B)):
        Hp = (H + 31) // 32 * 32
        pad = torch.nn.functional.pad
        y, hT, cT = _LSTMLayer.apply(x, pad(h0, (0, Hp - H)), pad(c0, (0, Hp - H)), _pad_gate_blocks(w_ih, H, Hp),
                                     _pad_gate_blocks(w_hh, H, Hp, cols=True), _pad_gate_blocks(b_ih, H, Hp),
                                     _pad_gate_blocks(b_hh, H, Hp), None if noise_rows is None else pad(noise_rows, (0, Hp - H)))
        return y[..., :H], hT[..., :H], cT[..., :H]
    return _LSTMLayer.apply(x, h0, c0, w_ih, w_hh, b_ih, b_hh, noise_rows)


_SIDE_STREAMS = {}


def _side_stream(i=0):
    """Side stream i of the layer wavefront (0: the other layer's recurrence, 1: the per-chunk GEMMs between the layers)."""
    st_ = _SIDE_STREAMS.get(i)
    if st_ is None:
        st_ = _SIDE_STREAMS[i] = torch.cuda.Stream()
    return st_


# no-grad forwards at B >= 256 (the scorer's packed batches) take the tiled GEMM + cell kernel: the fused step kernel re-reads
# W_hh once per 32 batch rows (measured: n-best rescoring 64.5 k -> 70-72 k hypotheses/s with the threshold at ~200-256)
_UNFUSED_STEP_B = 256


def _stack_chunks(T):
    """Time chunks of the layer wavefront: layer 2 runs one chunk behind layer 1.  Small enough that the lag is a
    small part of T, large enough that the host's per-chunk work (two library calls, one GEMM, two events) stays cheap."""
    # T 35 (BASELINE configs[0]: a 2.2 ms step of which the host needs 1.6-1.9 ms to issue): 3 x 12; smaller chunks win 2 % when the
    # host keeps up and lose 10-25 % when it does not (round 4, tools/wf_probe.py).  T 100 (the LSTM recipe: 10 ms step, 5 ms of
    # host): 13 chunks of 8 beat 7 of 15 by 1.2-1.5 % now that the per-chunk GEMMs run on a stream of their own (9.80-9.86 against
    # 9.94-10.02 ms, four runs each).  A B = 1 chain of thousands of steps (the scorer's carry chain) runs best on 128-step
    # chunks (62 k -> 66 k hypotheses/s).
    cmax = 16 if T < 64 else (8 if T <= 256 else 128)
    n = (T + cmax - 1) // cmax
    c = (T + n - 1) // n
    return [(t0, min(T, t0 + c)) for t0 in range(0, T, c)]


class _LSTMStack2(torch.autograd.Function):
    """Two stacked LSTM layers as a WAVEFRONT on two streams (what _VF.lstm / nn.LSTM(num_layers=2) compute,
    model.py:812, :35).  A fused step kernel occupies the chip for ~11 us but is bound by its launch -> load -> MFMA ->
    store latency chain, and two of them fit a CU (70 KB LDS, <= 256 VGPRs each): the steps of layer 2 over time chunk c
    run on a side stream WHILE layer 1 walks chunk c + 1 on the main stream (a step PAIR takes 15.4 us forward /
    17.4 us backward against 21.7 / 26.5 us back to back; tools/lstm_step_bench.py).  Per chunk: layer 1's steps, event,
    [inter-layer dropout of that chunk, RNNModel only] and layer 2's input GEMM over the chunk's rows on a THIRD stream (so
    that layer 2's recurrence only ever waits for the first of these GEMMs), layer 2's steps.  Layer 1's next chunk is
    issued before the host turns to layer 2's previous one.  Backward mirrors it (layer 2's chain leads on the side stream,
    the dgrad GEMM of the chunk on the stream between, layer 1 follows a chunk behind); both chains are issued by the library
    (blm_lstm_seq_fwd / blm_lstm_seq_bwd: ~3.3 us of host time per launch against ~5 us of device time per launch when
    two recurrences are in flight); the weight-gradient GEMMs stay batched over all T at the end.  Same kernels and the same
    arithmetic per step as two ops.lstm_layer calls: the forward is bit-identical to them; the backward is equal up to
    summation order (the per-chunk dgrad GEMMs accumulate into a pre-zeroed dy1, with K slices through float atomics where the
    planner picks them -- 1e-6 run to run; deterministic mode, ops.set_deterministic, takes the one-stream path instead)."""

    @staticmethod
    def forward(ctx, x, h0a, c0a, h0b, c0b, w_ih1, w_hh1, b_ih1, b_hh1, w_ih2, w_hh2, b_ih2, b_hh2, drop):
        x = _f32(x, "x")
        T, B, E = x.shape
        H = w_hh1.shape[1]
        G = 4 * H
        dev = x.device
        st = stream
        lib_ = calls()
        bias1, bias2 = _new(dev, G), _new(dev, G)
        hs1, cs1, ga1 = _new(dev, T + 1, B, H), _new(dev, T + 1, B, H), _new(dev, T, B, G)
        hs2, cs2, ga2 = _new(dev, T + 1, B, H), _new(dev, T + 1, B, H), _new(dev, T, B, G)
        # one launch: both layers' b_ih + b_hh and the four initial states into row 0 of the state histories
        _init_multi([(bias1, b_ih1, b_hh1), (bias2, b_ih2, b_hh2), (hs1[0], h0a, None), (cs1[0], c0a, None), (hs2[0], h0b, None),
                     (cs2[0], c0b, None)])
        xw1 = _new(dev, T, B, G)
        gemm(L.GEMM_NT, x, w_ih1, xw1, T * B, G, E, E, E, G, epilogue=L.EPI_BIAS, bias=bias1)
        xw2 = _new(dev, T, B, G)
        x2 = _new(dev, T, B, H) if drop.on else None  # layer 2's input = drop(h1) (nn.LSTM's inter-layer dropout)
        main, side = torch.cuda.current_stream(), _side_stream()
        tev = _timer_start("lstm_stack2_fwd T=%d", T)
        bh, bg = B * H * 4, B * G * 4  # bytes per time row
        p_xw1, p_xw2 = xw1.data_ptr(), xw2.data_ptr()
        p = {k: v.data_ptr() for k, v in (("hs1", hs1), ("cs1", cs1), ("ga1", ga1), ("hs2", hs2), ("cs2", cs2), ("ga2", ga2))}
        chunks = _stack_chunks(T)
        if B <= 4:
            # tiny batches (the scorer's carry chain): layer 1 over chunk c and layer 2 over chunk c - 1 from ONE stream, a step
            # of each per launch (blm_lstm_seq_pair_fwd) -- no second stream, no events, half the launches
            prev = None
            for cur in chunks + [None]:
                if prev is not None:
                    a0, a1 = prev
                    inp = hs1[a0 + 1:a1 + 1]
                    if drop.on:
                        inp = _dropout_apply(inp, drop, row0=a0, out=x2[a0:a1])
                    gemm(L.GEMM_NT, inp, w_ih2, xw2[a0:a1], (a1 - a0) * B, G, H, H, H, G, epilogue=L.EPI_BIAS, bias=bias2)
                t0, t1 = cur if cur is not None else (0, 0)
                a0, a1 = prev if prev is not None else (0, 0)
                lib_.blm_lstm_seq_pair_fwd(p_xw1 + t0 * bg, ptr(w_hh1), p["hs1"] + t0 * bh, p["cs1"] + t0 * bh, p["ga1"] + t0 * bg, t1 - t0,
                                           p_xw2 + a0 * bg, ptr(w_hh2), p["hs2"] + a0 * bh, p["cs2"] + a0 * bh, p["ga2"] + a0 * bg, a1 - a0,
                                           B, H, st())
                prev = cur
            chunks = []
        else:
            # many chunks (T >= 64): the per-chunk GEMMs get a stream of their own; few (T 35: three chunks, a step the host can
            # barely issue in time): they stay in front of layer 2's steps on the side stream, two events per chunk fewer
            three = len(chunks) > 4
            between = _side_stream(1) if three else side
            side.wait_stream(main)
            if three:
                between.wait_stream(main)

        def layer1(t0, t1):
            lib_.blm_lstm_seq_fwd(p_xw1 + t0 * bg, ptr(w_hh1), p["hs1"] + t0 * bh, p["cs1"] + t0 * bh, p["ga1"] + t0 * bg, None, t1 - t0, B, H, st())
            ev = torch.cuda.Event()
            ev.record(main)
            return ev

        def layer2(t0, t1, ev):
            n = t1 - t0
            # layer 2's input rows of this chunk on a stream of their own: layer 2's recurrence (one chunk behind) never waits
            # for a GEMM except in front of its first chunk
            with torch.cuda.stream(between):
                between.wait_event(ev)
                inp = hs1[t0 + 1:t1 + 1]
                if drop.on:
                    inp = _dropout_apply(inp, drop, row0=t0, out=x2[t0:t1])
                gemm(L.GEMM_NT, inp, w_ih2, xw2[t0:t1], n * B, G, H, H, H, G, epilogue=L.EPI_BIAS, bias=bias2)
                if three:
                    ev2 = torch.cuda.Event()
                    ev2.record(between)
            with torch.cuda.stream(side):
                if three:
                    side.wait_event(ev2)
                lib_.blm_lstm_seq_fwd(p_xw2 + t0 * bg, ptr(w_hh2), p["hs2"] + t0 * bh, p["cs2"] + t0 * bh, p["ga2"] + t0 * bg, None, n, B, H, st())
        # issue order with three streams: layer 1's NEXT chunk goes to its stream before the host turns to layer 2's previous one,
        # so the leading recurrence never waits for the host
        pend = None
        for (t0, t1) in chunks:
            ev = layer1(t0, t1)
            if not three:
                layer2(t0, t1, ev)
                continue
            if pend is not None:
                layer2(*pend)
            pend = (t0, t1, ev)
        if pend is not None:
            layer2(*pend)
        if chunks:
            main.wait_stream(side)
        tev.record()
        if _STATE_TAP is not None:
            _STATE_TAP.layers.append((hs1.index_select(0, _STATE_TAP.idx), cs1.index_select(0, _STATE_TAP.idx)))
            _STATE_TAP.layers.append((hs2.index_select(0, _STATE_TAP.idx), cs2.index_select(0, _STATE_TAP.idx)))
        ctx.save_for_backward(x, hs1, cs1, ga1, hs2, cs2, ga2, x2, w_ih1, w_hh1, w_ih2, w_hh2)
        ctx.w_refs = (w_ih1, w_hh1, w_ih2, w_hh2)
        ctx.b_refs = (b_ih1, b_hh1, b_ih2, b_hh2)
        ctx.drop = drop
        ctx.set_materialize_grads(False)  # the final states usually feed nothing: their gradients arrive as None, not as zero fills
        return hs2[1:], hs1[T], cs1[T], hs2[T], cs2[T]

    @staticmethod
    def backward(ctx, dy, dh1T, dc1T, dh2T, dc2T):
        x, hs1, cs1, ga1, hs2, cs2, ga2, x2, w_ih1, w_hh1, w_ih2, w_hh2 = ctx.saved_tensors
        drop = ctx.drop
        T, B, E = x.shape
        H = w_hh1.shape[1]
        G = 4 * H
        dev = x.device
        lib_ = calls()
        st = stream
        dy = torch.zeros(T, B, H, device=dev, dtype=torch.float32) if dy is None else _f32(dy, "dy")

        def state(w_hh):
            w_t = _new(dev, H, G)
            lib_.blm_transpose(ptr(w_hh), ptr(w_t), G, H, st())
            return {"dh": _new(dev, B, H), "dcs": _new(dev, 2, B, H), "k": 0, "w_t": w_t, "dg": _new(dev, T, B, G)}
        s1, s2 = state(w_hh1), state(w_hh2)
        dy1 = _new(dev, T, B, H)  # gradient reaching layer 1's outputs = layer 2's input gradient
        db1, db2 = _new(dev, G), _new(dev, G)
        # one launch: the incoming state gradients (or zeros) of both layers, zeroed bias gradients, and dy1 = 0 -- its chunks are
        # written by K-sliced products that would each need a memset of their own otherwise
        _init_multi([(s1["dh"], dh1T, None), (s1["dcs"][0], dc1T, None), (s2["dh"], dh2T, None), (s2["dcs"][0], dc2T, None),
                     (db1, None, None), (db2, None, None), (dy1, None, None)])
        bh, bg = B * H * 4, B * G * 4

        def chain(s, dyp, cs, ga, t_hi, t_lo):
            """dgates[t] for t = t_hi-1 .. t_lo (descending) of one layer from one call: the first launch of the whole chain is the
            plain cell backward of step T-1, every other one the fused step (dh_t = dgates[t+1] . W_hh, then the cell of step t)."""
            lib_.blm_lstm_seq_bwd(ptr(s["dh"]), dyp, ptr(cs), ptr(ga), ptr(s["w_t"]), ptr(s["dg"]), ptr(s["dcs"]), s["k"], None,
                                  T, t_hi, t_lo, B, H, st())
            s["k"] ^= (t_hi - t_lo) & 1
        main, side, between = torch.cuda.current_stream(), _side_stream(), _side_stream(1)
        dh01, dh02 = _new(dev, B, H), _new(dev, B, H)  # allocated on the main stream's pool, like everything else both streams touch
        tev = _timer_start("lstm_stack2_bwd T=%d", T)
        chunks = _stack_chunks(T)
        three = len(chunks) > 4  # as in forward
        if not three:
            between = main
        side.wait_stream(main)
        if three:
            between.wait_stream(main)
        for (t0, t1) in reversed(chunks):
            with torch.cuda.stream(side):
                chain(s2, dy.data_ptr(), cs2, ga2, t1, t0)
                ev = torch.cuda.Event()
                ev.record(side)
            n = t1 - t0
            # layer 1's incoming gradient rows of this chunk: on the stream between the layers when there are many chunks (layer 1's
            # chain, one chunk behind, then only ever waits for the first of these GEMMs), else in front of layer 1's steps
            with torch.cuda.stream(between):
                between.wait_event(ev)
                gemm(L.GEMM_NN, s2["dg"][t0:t1], w_ih2, dy1[t0:t1], n * B, H, G, G, H, H, accumulate=True)  # into the zeroed rows
                if drop.on:
                    _dropout_apply(dy1[t0:t1], drop, row0=t0, out=dy1[t0:t1])
                if three:
                    ev2 = torch.cuda.Event()
                    ev2.record(between)
            if three:
                main.wait_event(ev2)
            chain(s1, dy1.data_ptr(), cs1, ga1, t1, t0)
        # gradient w.r.t. the initial states: dh_{-1} = dgates[0] . W_hh
        for s, strm, d in ((s2, side, dh02), (s1, main, dh01)):
            with torch.cuda.stream(strm):
                lib_.blm_lstm_step_bwd(ptr(s["dg"][0]), ptr(s["w_t"]), None, None, None, None, None, None, None, ptr(d), B, H, st())
        main.wait_stream(side)
        tev.record()
        dc02, dc01 = s2["dcs"][s2["k"]], s1["dcs"][s1["k"]]
        dg1, dg2 = s1["dg"], s2["dg"]
        inp2 = x2 if drop.on else hs1[1:]
        dx = torch.empty_like(x)
        gemm(L.GEMM_NN, dg1, w_ih1, dx, T * B, E, G, G, E, E)
        # leaf weights accumulate straight into .grad (see _LSTMLayer.backward); sampled ones get fresh tensors
        outs = []
        summed = [False, False]  # the bias gradient = column sums of dgates: taken from the A tiles a weight-gradient GEMM stages anyway
        for j, (w_p, A, Bm, kdim) in enumerate(((ctx.w_refs[0], dg1, x, E), (ctx.w_refs[1], dg1, hs1, H), (ctx.w_refs[2], dg2, inp2, H),
                                                (ctx.w_refs[3], dg2, hs2, H))):
            if not w_p.requires_grad:
                outs.append(None)
                continue
            buf, acc, ret = _wgrad_target(w_p)
            cs_a = None
            if not summed[j // 2]:
                cs_a, summed[j // 2] = (db1, db2)[j // 2], True
            gemm(L.GEMM_TN, A, Bm, buf, G, kdim, T * B, G, kdim, kdim, accumulate=acc, colsum_a=cs_a)  # hs[0:T] = h_{t-1}
            outs.append(ret)
        _notify(*ctx.w_refs)
        dw_ih1, dw_hh1, dw_ih2, dw_hh2 = outs
        for done, dgl, dbl in ((summed[0], dg1, db1), (summed[1], dg2, db2)):
            if not done:
                _colsum_into(dgl, T * B, G, dbl, accumulate=True)
        db_ih1, db_hh1, db_ih2, db_hh2 = _bias_pair_grads(ctx.b_refs, [db1, db2], [ctx.needs_input_grad[i] for i in (7, 8, 11, 12)])
        return dx, dh01, dc01, dh02, dc02, dw_ih1, dw_hh1, db_ih1, db_hh1, dw_ih2, dw_hh2, db_ih2, db_hh2, None


def lstm_stack2_ok(x, w_hh1, w_hh2, w_ih2):
    """Shapes the layer wavefront takes: fused step kernels (H % 32 == 0, aligned, contiguous) and equal hidden sizes --
    and, unless it was switched on or off explicitly, the shapes it PAYS for (see below)."""
    T, B, _ = x.shape
    H = w_hh1.shape[1]
    if _STACK2_ON is None:
        # deterministic mode keeps the stack on one stream unless the wavefront is forced on (set_lstm_wavefront(True)): with one K
        # slice per tile its per-chunk products are bit-identical to the sequential layers', which is what makes the forced form
        # a bitwise race check of the stream schedule (tests/test_gpu_deterministic.py)
        on = B <= 32 and T >= 32 and H >= 640 and not is_deterministic()
    else:
        on = _STACK2_ON
    return (on and T >= 8 and H % 32 == 0 and w_hh2.shape[1] == H and w_ih2.shape[1] == H and w_hh1.is_contiguous() and w_hh2.is_contiguous()
            and w_hh1.data_ptr() % 16 == 0 and w_hh2.data_ptr() % 16 == 0 and (B * H) % 4 == 0)


# When does the wavefront pay?  A fused step kernel launches ceil(B / 32) * H / 8 workgroups (forward) -- at B <= 32 and
# H = 1024 that is 128, HALF the chip -- and is bound by its launch -> load -> MFMA -> store latency chain, so two of them
# side by side cost what one does.  Measured (tools/run_workload.py, same box, off / on):
#   recipe shape (run_nnlm_ami_lstm.sh: T 100, B 32): 11.07 -> 9.96 ms per training step (289 k -> 321 k tokens/s);
#   cfg2 (T 35, B 64: the kernels fill the chip, layer 2's per-chunk input GEMM of M = 320 rows and the one-chunk lag give the
#   overlap back): 6.65 -> 6.74 ms;  cfg1 (T 35, B 20): 2.31 -> 2.21 ms with three chunks of 12 steps (2.30 with 5-step
#   chunks, 2.31 with 16 + 16 + 3), evaluate() at T 35 / B 20 1.14 -> 1.07 ms.
#   smaller layers (round 5, tools/lstm_hidden_size_probe.py, T 35, B 20, off / on): H 128: 528 / 421 k tokens/s, 256: 500 / 447 k,
#   512: 465 / 441 k, 768: 362 / 361 k, 672: 349 / 386 k, 1536: 197 / 201 k -- the step kernels of a small layer are a few dozen
#   workgroups and the step is host-bound: the second stream's events cost more than the overlap returns.
# Rule: on for B <= 32, T >= 32 and H >= 640; BLM_LSTM_WAVEFRONT=0|1 / set_lstm_wavefront(True | False) force it, None = rule.
_env_wf = os.environ.get("BLM_LSTM_WAVEFRONT")
_STACK2_ON = None if _env_wf is None else _env_wf == "1"


def set_lstm_wavefront(on):
    """True / False: two-layer LSTM stacks always / never run as a wavefront on two streams (ops.lstm_stack2); None: by the
    measured rule above."""
    global _STACK2_ON
    _STACK2_ON = None if on is None else bool(on)


def lstm_stack2(x, h0, c0, layer1, layer2, drop=NO_DROP):
    """Two stacked LSTM layers; ``h0`` / ``c0`` are (2, B, H), ``layer*`` = (w_ih, w_hh, b_ih, b_hh), ``drop`` the
    inter-layer dropout (nn.LSTM's; NO_DROP for _VF.lstm(dropout=0.)).  -> (y (T,B,H), (h1T, h2T), (c1T, c2T))"""
    y, h1, c1, h2, c2 = _LSTMStack2.apply(x, h0[0], c0[0], h0[1], c0[1], *layer1, *layer2, drop)
    return y, (h1, h2), (c1, c2)


class _LSTMRecurrentGP(torch.autograd.Function):
    """Recurrent part of a GP-LSTM layer on the fused step kernels.  ``xw`` (T,B,4H) holds the input-side
    pre-activations of all steps (biases inside), ``w_rec`` (4H,H) the recurrent rows.  ``ovr``:
      0..3  GPNN on that gate (GPLSTMCell gate types 1-4, reference model.py:1754-1771): block ``ovr`` of
            xw / w_rec is the GPNN's input / hidden part, ``coef4`` (4,H) its mixture coefficients;
      4     gate type 6 (model.py:1744-1752): the whole hidden projection h w_rec^T + rbias goes through
            the mixture (``coef4`` (4,4H)) before it is added to xw;
      -1    plain recurrence on a given xw (gate type 7: xw is the GPNN of the inputs)."""

    @staticmethod
    def forward(ctx, xw, h0, c0, w_rec, coef4, ovr, rbias, w_cell=None):
        xw, w_rec = _f32(xw, "xw"), _f32(w_rec, "w_rec")
        ovr = int(ovr)
        coef4 = _f32(coef4, "coef4") if ovr >= 0 else None
        rbias = _f32(rbias, "rbias") if ovr >= 4 else None
        w_cell = _f32(w_cell, "w_cell") if ovr == 5 else None
        T, B, G = xw.shape
        H = G // 4
        if tuple(w_rec.shape) != (G, H) or (ovr == 5 and tuple(w_cell.shape) != (H, H)):
            # the step kernels take these as (4H, H) / (H, H) operands on trust
            raise BayesLMError("lstm_recurrent_gp: w_rec %s / w_cell %s do not fit xw (T, B, %d)"
                               % (tuple(w_rec.shape), None if w_cell is None else tuple(w_cell.shape), G))
        dev = xw.device
        L.require_gfx950()
        hs = _new(dev, T + 1, B, H)
        cs = _new(dev, T + 1, B, H)
        hs[0].copy_(h0)
        cs[0].copy_(c0)
        ga = _new(dev, T, B, G)
        zs = _new(dev, T, B, G if ovr == 4 else H) if ovr >= 0 else None
        st = stream()
        xw_p, hs_p, cs_p, ga_p = _P(xw), _P(hs), _P(cs), _P(ga)
        zs_p = None if zs is None else _P(zs)
        w_p, co_p, rb_p = ptr(w_rec), ptr(coef4), ptr(rbias)
        step_fwd = calls().blm_lstm_step_fwd_gp
        step_dh = calls().blm_lstm_step_dh
        wc_p = ptr(w_cell)
        for t in range(T):
            if ovr == 5:  # z_t = c_{t-1} Wg^T: the second recurrent product of the step, one skinny launch in front of it
                step_dh(cs_p[t], wc_p, zs_p[t], B, H, H, st)
            step_fwd(xw_p[t], w_p, hs_p[t], cs_p[t], hs_p[t + 1], cs_p[t + 1], ga_p[t], None, ovr, co_p, rb_p,
                     None if zs_p is None else zs_p[t], B, H, st)
        if _STATE_TAP is not None:
            _STATE_TAP.layers.append((hs.index_select(0, _STATE_TAP.idx), cs.index_select(0, _STATE_TAP.idx)))
        ctx.save_for_backward(hs, cs, ga, w_rec, *([zs, coef4] if ovr >= 0 else []), *([w_cell] if ovr == 5 else []))
        ctx.ovr = ovr
        return hs[1:], hs[T], cs[T]

    @staticmethod
    def backward(ctx, dy, dhT, dcT):
        ovr = ctx.ovr
        w_cell = None
        if ovr == 5:
            hs, cs, ga, w_rec, zs, coef4, w_cell = ctx.saved_tensors
        elif ovr >= 0:
            hs, cs, ga, w_rec, zs, coef4 = ctx.saved_tensors
        else:
            hs, cs, ga, w_rec = ctx.saved_tensors
            zs = coef4 = None
        T, B, G = ga.shape
        H = G // 4
        dev = ga.device
        dy = _f32(dy, "dy")
        st = stream()
        dgates = _new(dev, T, B, G)
        dact = _new(dev, T, B, H) if (0 <= ovr < 4 or ovr == 5) else None
        # A operands of the next products: ovr 4 -- d z of the hidden projection (B,4H); ovr 5 -- d z of the cell-state GPNN (B,H)
        dzs = _new(dev, T, B, G if ovr == 4 else H) if ovr >= 4 else None
        dh = torch.zeros(B, H, device=dev, dtype=torch.float32) if dhT is None else _f32(dhT, "dhT").clone()
        dcs = torch.zeros(2, B, H, device=dev, dtype=torch.float32)
        if dcT is not None:
            dcs[0].copy_(dcT)
        w_t = _new(dev, H, G)
        calls().blm_transpose(ptr(w_rec), ptr(w_t), G, H, st)
        # last step: plain cell backward (the GP gate as an external activation), then the mixture's derivative
        if 0 <= ovr < 4:
            calls().blm_axpy(ptr(dy[T - 1]), ptr(dh), B * H, 1.0, st)
            calls().blm_lstm_cell_ovr_bwd(ptr(dh), ptr(dcs[0]), ptr(cs[T - 1]), ptr(cs[T]), ptr(ga[T - 1]), ovr,
                                          ptr(dgates[T - 1]), ptr(dact[T - 1]), ptr(dcs[1]), B, H, st)
            dz = _new(dev, B, H)
            calls().blm_gp_mix_bwd(ptr(dact[T - 1]), ptr(zs[T - 1]), ptr(coef4), ptr(dz), B, H, st)
            dgates[T - 1][:, ovr * H:(ovr + 1) * H].copy_(dz)
        else:
            c_in = cs[T - 1]
            if ovr == 5:  # the last step's cell saw the mixture of z_{T-1}
                c_in = _new(dev, B, H)
                calls().blm_gp_mix_fwd(ptr(zs[T - 1]), ptr(coef4), ptr(c_in), B, H, st)
            calls().blm_lstm_cell_bwd2(ptr(dh), ptr(dy[T - 1]), ptr(dcs[0]), ptr(c_in), ptr(cs[T]), ptr(ga[T - 1]),
                                       ptr(dgates[T - 1]), ptr(dcs[1]), B, H, st)
            if ovr == 5:
                w_cell_t = _new(dev, H, H)
                calls().blm_transpose(ptr(w_cell), ptr(w_cell_t), H, H, st)
                dact[T - 1].copy_(dcs[1])
                calls().blm_gp_mix_bwd(ptr(dcs[1]), ptr(zs[T - 1]), ptr(coef4), ptr(dzs[T - 1]), B, H, st)
                calls().blm_lstm_step_dh(ptr(dzs[T - 1]), ptr(w_cell_t), ptr(dcs[1]), B, H, H, st)
            if ovr == 4:
                calls().blm_gp_mix_bwd(ptr(dgates[T - 1]), ptr(zs[T - 1]), ptr(coef4), ptr(dzs[T - 1]), B, G, st)
        A = dzs if ovr == 4 else dgates
        k = 1
        A_p, dy_p, cs_p, ga_p, dg_p, dcs_p = _P(A), _P(dy), _P(cs), _P(ga), _P(dgates), _P(dcs)
        zs_p = None if zs is None else _P(zs)
        da_p = None if dact is None else _P(dact)
        dzs_p = None if dzs is None else _P(dzs)
        wt_p, co_p = ptr(w_t), ptr(coef4)
        step_bwd = calls().blm_lstm_step_bwd_gp
        wct_p = ptr(w_cell_t) if ovr == 5 else None
        step_dh = calls().blm_lstm_step_dh
        for t in range(T - 1, 0, -1):
            step_bwd(A_p[t], wt_p, dy_p[t - 1], dcs_p[k], cs_p[t - 1], cs_p[t], ga_p[t - 1], dg_p[t - 1], dcs_p[k ^ 1], None,
                     ovr, co_p, None if zs_p is None else zs_p[t - 1], None if da_p is None else da_p[t - 1],
                     None if dzs_p is None else dzs_p[t - 1], B, H, st)
            if ovr == 5:  # raw cell-state gradient of the earlier step: d z . Wg
                step_dh(dzs_p[t - 1], wct_p, dcs_p[k ^ 1], B, H, H, st)
            k ^= 1
        dh0 = _new(dev, B, H)
        calls().blm_lstm_step_bwd(ptr(A[0]), ptr(w_t), None, None, None, None, None, None, None, ptr(dh0), B, H, st)
        dw = torch.empty_like(w_rec)
        gemm(L.GEMM_TN, A, hs, dw, G, H, T * B, G, H, H)  # hs[0:T] = h_{t-1}
        dcoef = drb = dwc = None
        if 0 <= ovr < 4 or ovr == 5:
            dcoef = torch.zeros_like(coef4)
            calls().blm_gp_coef_grad(ptr(dact), ptr(zs), ptr(dcoef), T * B, H, st)
        if ovr == 5:  # the cell-state GPNN's affine map, batched over all steps: dWg = dz^T c_{t-1}, db = column sums of dz
            dwc = torch.empty_like(w_cell)
            gemm(L.GEMM_TN, dzs, cs, dwc, H, H, T * B, H, H, H)  # cs[0:T] = c_{t-1}
            drb = _new(dev, H)
            _colsum_into(dzs, T * B, H, drb, accumulate=False)
        elif ovr == 4:
            dcoef = torch.zeros_like(coef4)
            calls().blm_gp_coef_grad(ptr(dgates), ptr(zs), ptr(dcoef), T * B, G, st)
            drb = _new(dev, G)
            _colsum_into(dzs, T * B, G, drb, accumulate=False)
        return dgates, dh0, dcs[k], dw, dcoef, None, drb, dwc


class _LSTMRecurrentGPNN2(torch.autograd.Function):
    """GP-LSTM layer whose cell holds a GPNN2 that draws FRESH frequencies at every time step (GPLSTMCell with type digit 4,
    model.py:1698-1702, 1744-1771; GPNN2 :2061-2076), from ONE autograd node.  GPNN2_t(x) = (actsum(x F_t) | 1) [W | b]^T,
    F_t = mean + eps_t * exp(lgstd).  ``mode``:
      0  gate types 1-4: gate ``g``'s activation is GPNN2_t of its pre-activation  xw_t[:, g] + (h_{t-1} W_hh^T)[:, g]
      1  gate type 5:    the cell state enters the update as GPNN2_t(c_{t-1})
      2  gate type 6:    the hidden projection of all four gates is GPNN2_t(h_{t-1})  (w_hh unused)
    Per step 4-6 skinny launches (products on blm_lstm_step_dh: fixed summation order, no split-K atomics, no memset)
    instead of ~10 launches plus ten autograd nodes; the time loops run in C (blm_lstm_gpnn2_seq_fwd / _bwd).  The T
    frequency matrices are sampled in one launch (blm_gpnn2_sample_steps) with the Philox counters the step-wise path
    uses, so both paths see the same noise; the weight gradients are batched over all steps after the loop, the per-step
    frequency gradients x_t^T d f_t become d mean / d lgstd in one launch (blm_gpnn2_freq_grad, eps_t regenerated)."""

    MP, GP = 160, 192  # feature columns padded to the products' tile rules (output % 16, contraction % 64); 150 MC terms

    @staticmethod
    def _noise(noises, dev):
        """-> (eps_all (T,H,M) or None, rng of call 0 or None): injected tensors are stacked, Philox specs must be the
        consecutive steps GPNN2.step_noises hands out."""
        if noises is None:
            return None, None
        if any(n.eps is not None for n in noises):
            if any(n.eps is None for n in noises):  # a per-call eps_override list with holes
                raise BayesLMError("lstm_recurrent_gpnn2: the per-step noise is either injected for EVERY step or drawn from Philox for every step")
            return torch.stack([_f32(n.eps, "eps") for n in noises]).contiguous(), None
        for t, n in enumerate(noises):
            if n.eps is not None or n.seed != noises[0].seed or n.tensor_id != noises[0].tensor_id or n.step != ((noises[0].step + t) & 0xFFFFFFFF):
                raise BayesLMError("lstm_recurrent_gpnn2: the per-step noise must be one Philox stream at consecutive steps")
        return None, noises[0].rng()

    @staticmethod
    def _desc(mode, g, acts, T, B, H, M, nF, **bufs):
        q = L.Gpnn2Seq()
        q.abi_version, q.mode, q.gate, q.acts = L.ABI_VERSION, mode, g, acts
        q.T, q.B, q.H, q.M, q.MP, q.GP, q.nF = T, B, H, M, _LSTMRecurrentGPNN2.MP, _LSTMRecurrentGPNN2.GP, nF
        for k, v in bufs.items():
            setattr(q, k, ptr(v))
        return q

    @staticmethod
    def forward(ctx, xw, h0, c0, w_hh, coef_w, coef_b, fmean, flgstd, noises, g, acts, mode):
        xw = _f32(xw, "xw")
        w_hh = _f32(w_hh, "w_hh") if mode != 2 else None
        T, B, G4 = xw.shape
        H = G4 // 4
        M = fmean.shape[1]
        MP, GP = _LSTMRecurrentGPNN2.MP, _LSTMRecurrentGPNN2.GP
        NO = G4 if mode == 2 else H  # outputs of the GPNN2
        if M >= MP or H % 64 != 0 or fmean.shape[0] != H or coef_w.shape != (NO, M):
            raise BayesLMError("lstm_recurrent_gpnn2: needs n_MC_terms < %d, H %% 64 == 0, a GPNN2(H, %d)" % (MP, NO))
        dev = xw.device
        L.require_gfx950()
        lib_, st = calls(), stream()
        nF = T if noises is not None else 1
        # F_t^T with zero rows m >= M (the w_t operand of the feature product) and F_t padded along m (the w_t operand of
        # d x = d f . F_t^T), all T of them in ONE launch, with the noise of calls 0..T-1 of the step-wise path
        FT, Fp = _new(dev, nF, MP, H), _new(dev, nF, H, GP)
        eps_all, rng0 = _LSTMRecurrentGPNN2._noise(noises, dev)
        if noises is None:
            eps_all = torch.zeros(1, H, M, device=dev, dtype=torch.float32)  # mean frequencies at every step
        lib_.blm_gpnn2_sample_steps(ptr(_f32(fmean, "frequency_mean")), ptr(_f32(flgstd, "frequency_lgstd")), ptr(eps_all),
                                    C.byref(rng0) if rng0 is not None else None, nF, H, M, MP, GP, ptr(FT), ptr(Fp), st)
        cwp = torch.zeros(NO, GP, device=dev, dtype=torch.float32)  # [coef.weight | coef.bias | 0]
        cwp[:, :M].copy_(coef_w)
        cwp[:, M].copy_(coef_b)
        hs, cs = _new(dev, T + 1, B, H), _new(dev, T + 1, B, H)
        hs[0].copy_(h0)
        cs[0].copy_(c0)
        ga = _new(dev, T, B, G4)
        z4 = _new(dev, T, B, G4) if mode == 0 else None
        pre = _new(dev, T, B, H) if mode == 0 else None
        feat, gout = _new(dev, T, B, MP), _new(dev, T, B, NO)
        sact = torch.zeros(T, B, GP, device=dev, dtype=torch.float32)  # the feature product writes columns < MP; the padding stays 0
        q = _LSTMRecurrentGPNN2._desc(mode, g, acts, T, B, H, M, nF, xw=xw, w_hh=w_hh, FT=FT, Fp=Fp, cwp=cwp, hs=hs, cs=cs, ga=ga, z4=z4,
                                      pre=pre, feat=feat, sact=sact, gout=gout)
        lib_.blm_lstm_gpnn2_seq_fwd(C.byref(q), st)
        if _STATE_TAP is not None:
            _STATE_TAP.layers.append((hs.index_select(0, _STATE_TAP.idx), cs.index_select(0, _STATE_TAP.idx)))
        ctx.save_for_backward(hs, cs, ga, feat, sact, Fp, cwp, *([w_hh] if mode != 2 else []), *([pre] if mode == 0 else []),
                              *([gout] if mode == 1 else []))
        ctx.meta = (mode, g, acts, M, fmean, flgstd, noises, coef_w.requires_grad, coef_b.requires_grad)
        return hs[1:], hs[T], cs[T]

    @staticmethod
    def backward(ctx, dy, dhT, dcT):
        mode, g, acts, M, fmean, flgstd, noises, need_cw, need_cb = ctx.meta
        hs, cs, ga, feat, sact, Fp, cwp = ctx.saved_tensors[:7]
        rest = list(ctx.saved_tensors[7:])
        w_hh = rest.pop(0) if mode != 2 else None
        pre = rest.pop(0) if mode == 0 else None
        gout = rest.pop(0) if mode == 1 else None
        T, B, G4 = ga.shape
        H = G4 // 4
        MP, GP = _LSTMRecurrentGPNN2.MP, _LSTMRecurrentGPNN2.GP
        NO = cwp.shape[0]
        dev = ga.device
        dy = _f32(dy, "dy")
        lib_, st = calls(), stream()
        nF = Fp.shape[0]
        w_t = None
        if mode != 2:
            w_t = _new(dev, H, G4)
            lib_.blm_transpose(ptr(w_hh), ptr(w_t), G4, H, st)
        cwt = _new(dev, GP, NO)
        lib_.blm_transpose(ptr(cwp), ptr(cwt), NO, GP, st)
        dgates, df = _new(dev, T, B, G4), _new(dev, T, B, GP)
        da = _new(dev, T, B, H) if mode != 2 else None
        dh = torch.zeros(B, H, device=dev, dtype=torch.float32) if dhT is None else _f32(dhT, "dhT").clone()
        dcs = torch.zeros(2, B, H, device=dev, dtype=torch.float32)
        if dcT is not None:
            dcs[0].copy_(dcT)
        q = _LSTMRecurrentGPNN2._desc(mode, g, acts, T, B, H, M, nF, w_hh_t=w_t, Fp=Fp, cwt=cwt, cs=cs, ga=ga, feat=feat, gout=gout, dy=dy,
                                      dh=dh, dcs2=dcs, dgates=dgates, da=da, df=df)
        lib_.blm_lstm_gpnn2_seq_bwd(C.byref(q), st)
        k = T & 1
        dw = None
        if mode != 2:
            dw = torch.empty_like(w_hh)
            gemm(L.GEMM_TN, dgates, hs, dw, G4, H, T * B, G4, H, H)  # hs[0:T] = h_{t-1}
        dcw = dcb = None
        if need_cw or need_cb:
            dout = dgates if mode == 2 else da  # the gradient of the GPNN2's output, all steps
            dcwp = _new(dev, NO, GP)
            gemm(L.GEMM_TN, dout, sact, dcwp, NO, GP, T * B, NO, GP, GP)  # column M of s is the constant 1: its row is d coef.bias
            dcw = dcwp[:, :M].contiguous() if need_cw else None
            dcb = dcwp[:, M].contiguous() if need_cb else None
        # (mean frequencies -- eval mode or a deterministic GPNN2 -- give the lgstd no gradient: with the mean frozen there is nothing to do)
        if fmean.requires_grad or (flgstd.requires_grad and noises is not None):
            # d F_t = x_t^T d f_t (contraction over the B rows of ONE step: the frequencies differ per step); d mean is their
            # sum, d lgstd their eps_t-weighted sum times sigma -- one launch, eps_t regenerated from the Philox counters
            x_in = pre if mode == 0 else (cs if mode == 1 else hs)  # rows 0..T-1: the GPNN2's inputs
            eps_all, rng0 = _LSTMRecurrentGPNN2._noise(noises, dev)
            Tn, Bn = T, B
            if noises is None:  # mean frequencies (deterministic GPNN2): d mean only, one contraction over all T*B rows
                eps_all = torch.zeros(1, H, M, device=dev, dtype=torch.float32)
                Tn, Bn = 1, T * B
            lib_.blm_gpnn2_freq_grad(ptr(x_in), ptr(df), ptr(eps_all), C.byref(rng0) if rng0 is not None else None,
                                     ptr(flgstd), ptr(_grad_buf(fmean)) if fmean.requires_grad else None,
                                     ptr(_grad_buf(flgstd)) if (flgstd.requires_grad and noises is not None) else None,
                                     Tn, Bn, H, M, GP, st)
            _notify(fmean, flgstd)
        return dgates, dh, dcs[k], dw, dcw, dcb, None, None, None, None, None, None


class _GPNN2Steps(torch.autograd.Function):
    """out[t] = GPNN2_t(x[t]) for all T steps of a window -- a GPNN2 that is called once per time step and draws fresh
    frequencies at every call, on inputs that do not depend on the recurrence (GPLSTMCell gate type 7 with type digit 4:
    the input projection, model.py:1747-1748).  Only the feature product is per step (T skinny launches, independent of
    each other); the activation sum, the coefficient product and every gradient are batched over the T*B rows."""

    @staticmethod
    def forward(ctx, x, coef_w, coef_b, fmean, flgstd, noises, acts):
        x = _f32(x, "x")
        T, B, E = x.shape
        NO, M = coef_w.shape
        MP, GP = _LSTMRecurrentGPNN2.MP, _LSTMRecurrentGPNN2.GP
        if M >= MP or E % 64 != 0 or fmean.shape != (E, M):
            raise BayesLMError("gpnn2_steps: needs n_MC_terms < %d, input width %% 64 == 0" % MP)
        dev = x.device
        L.require_gfx950()
        lib_, st = calls(), stream()
        nF = T if noises is not None else 1
        FT, Fp = _new(dev, nF, MP, E), _new(dev, nF, E, GP)
        eps_all, rng0 = _LSTMRecurrentGPNN2._noise(noises, dev)
        if noises is None:
            eps_all = torch.zeros(1, E, M, device=dev, dtype=torch.float32)
        lib_.blm_gpnn2_sample_steps(ptr(_f32(fmean, "frequency_mean")), ptr(_f32(flgstd, "frequency_lgstd")), ptr(eps_all),
                                    C.byref(rng0) if rng0 is not None else None, nF, E, M, MP, GP, ptr(FT), ptr(Fp), st)
        cwp = torch.zeros(NO, GP, device=dev, dtype=torch.float32)
        cwp[:, :M].copy_(coef_w)
        cwp[:, M].copy_(coef_b)
        feat, sact = _new(dev, T, B, MP), _new(dev, T, B, GP)
        x_p, f_p, FT_p = _P(x), _P(feat), _P(FT)
        for t in range(T):
            lib_.blm_lstm_step_dh(x_p[t], FT_p[t if nF > 1 else 0], f_p[t], B, MP, E, st)
        lib_.blm_gpnn2_actsum_fwd(ptr(feat), ptr(sact), T * B, M, MP, GP, 1.0 / math.sqrt(M), acts, st)
        out = _new(dev, T, B, NO)
        gemm(L.GEMM_NT, sact, cwp, out, T * B, NO, GP, GP, GP, NO)
        ctx.save_for_backward(x, feat, sact, Fp, cwp)
        ctx.meta = (acts, M, fmean, flgstd, noises, coef_w.requires_grad, coef_b.requires_grad)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, feat, sact, Fp, cwp = ctx.saved_tensors
        acts, M, fmean, flgstd, noises, need_cw, need_cb = ctx.meta
        T, B, E = x.shape
        NO = cwp.shape[0]
        MP, GP = _LSTMRecurrentGPNN2.MP, _LSTMRecurrentGPNN2.GP
        dev = x.device
        dout = _f32(dout, "dout")
        lib_, st = calls(), stream()
        nF = Fp.shape[0]
        ds = _new(dev, T, B, GP)
        gemm(L.GEMM_NN, dout, cwp, ds, T * B, GP, NO, NO, GP, GP)
        df = _new(dev, T, B, GP)
        lib_.blm_gpnn2_actsum_bwd(ptr(ds), ptr(feat), ptr(df), T * B, M, MP, GP, 1.0 / math.sqrt(M), acts, st)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _new(dev, T, B, E)
            df_p, dx_p, Fp_p = _P(df), _P(dx), _P(Fp)
            for t in range(T):
                lib_.blm_lstm_step_dh(df_p[t], Fp_p[t if nF > 1 else 0], dx_p[t], B, E, GP, st)
        dcw = dcb = None
        if need_cw or need_cb:
            dcwp = _new(dev, NO, GP)
            gemm(L.GEMM_TN, dout, sact, dcwp, NO, GP, T * B, NO, GP, GP)
            dcw = dcwp[:, :M].contiguous() if need_cw else None
            dcb = dcwp[:, M].contiguous() if need_cb else None
        if fmean.requires_grad or (flgstd.requires_grad and noises is not None):
            eps_all, rng0 = _LSTMRecurrentGPNN2._noise(noises, dev)
            Tn, Bn = T, B
            if noises is None:
                eps_all = torch.zeros(1, E, M, device=dev, dtype=torch.float32)
                Tn, Bn = 1, T * B
            lib_.blm_gpnn2_freq_grad(ptr(x), ptr(df), ptr(eps_all), C.byref(rng0) if rng0 is not None else None, ptr(flgstd),
                                     ptr(_grad_buf(fmean)) if fmean.requires_grad else None,
                                     ptr(_grad_buf(flgstd)) if (flgstd.requires_grad and noises is not None) else None,
                                     Tn, Bn, E, M, GP, st)
            _notify(fmean, flgstd)
        return dx, dcw, dcb, None, None, None, None


def gpnn2_steps(x, coef_w, coef_b, fmean, flgstd, noises, acts):
    """(T,B,E) -> (T,B,NO): GPNN2_t(x[t]) with the noise of calls 0..T-1 (``noises`` as for lstm_recurrent_gpnn2)."""
    fmean, flgstd = _weight(fmean, "fmean", in_place=True), _weight(flgstd, "flgstd", in_place=True)
    return _GPNN2Steps.apply(x, coef_w, coef_b, fmean, flgstd, noises, int(acts))


def lstm_recurrent_gpnn2_supported(H, n_mc):
    return H % 64 == 0 and n_mc < _LSTMRecurrentGPNN2.MP


def lstm_recurrent_gpnn2(xw, h0, c0, w_hh, coef_w, coef_b, fmean, flgstd, noises, gate, acts, mode=0):
    """-> (y (T,B,H), hT, cT).  ``noises``: list of T NoiseSpec (training) or None (mean frequencies); ``acts``: bit set of the
    GPNN2's activations in the mixture's slot order (1 tanh, 2 sigmoid, 4 relu, 8 gelu); ``mode``: see _LSTMRecurrentGPNN2."""
    fmean, flgstd = _weight(fmean, "fmean", in_place=True), _weight(flgstd, "flgstd", in_place=True)
    return _LSTMRecurrentGPNN2.apply(xw, h0, c0, w_hh, coef_w, coef_b, fmean, flgstd, noises, int(gate), int(acts), int(mode))


def lstm_recurrent_gp_supported(H, w_rec):
    return H % 32 == 0 or H >= _PAD_HIDDEN_FROM  # other sizes from 64 up are zero-padded to the next multiple of 32 (below)


def _pad_last_gate_blocks(t, H, Hp):
    """(..., 4H) -> (..., 4Hp), gate block g of the last dimension moved to [g Hp, g Hp + H)."""
    return torch.nn.functional.pad(t.reshape(*t.shape[:-1], 4, H), (0, Hp - H)).reshape(*t.shape[:-1], 4 * Hp)


def lstm_recurrent_gp(xw, h0, c0, w_rec, coef4=None, ovr=-1, rbias=None, w_cell=None):
    """The GP-LSTM recurrence on the fused step kernels (_LSTMRecurrentGP).  A hidden size that is not a multiple of 32 is
    zero-padded as in ``lstm_layer`` (650: 71 k -> the padded rate, tools/lstm_family_hidden_size_probe.py): with zero recurrent
    rows / columns, zero pre-activations and ZERO mixture coefficients a padded unit's GP gate is 0 and its other gates 1/2, so its
    cell and output stay exactly 0 whichever gate the GPNN sits on; pad and slice are torch ops (autograd undoes them)."""
    G = xw.shape[-1]
    H = G // 4
    if H % 32 and H >= _PAD_HIDDEN_FROM and G == 4 * H and tuple(w_rec.shape) == (G, H):
        Hp = (H + 31) // 32 * 32
        pad = torch.nn.functional.pad
        ovr = int(ovr)
        c4 = coef4
        if coef4 is not None and ovr >= 0:
            c4 = _pad_last_gate_blocks(coef4, H, Hp) if coef4.shape[-1] == 4 * H else pad(coef4, (0, Hp - H))
        rb = _pad_last_gate_blocks(rbias, H, Hp) if (rbias is not None and ovr >= 4) else rbias
        wc = pad(w_cell, (0, Hp - H, 0, Hp - H)) if (w_cell is not None and ovr == 5) else w_cell
        y, hT, cT = _LSTMRecurrentGP.apply(_pad_last_gate_blocks(xw, H, Hp), pad(h0, (0, Hp - H)), pad(c0, (0, Hp - H)),
                                           _pad_gate_blocks(w_rec, H, Hp, cols=True), c4, ovr, rb, wc)
        return y[..., :H], hT[..., :H], cT[..., :H]
    return _LSTMRecurrentGP.apply(xw, h0, c0, w_rec, coef4, ovr, rbias, w_cell)


# ----------------------------------------------------------------------------
# Step-wise cells for the GP / Variational LSTMs (the reference runs them as Python time loops,
# model.py:1734-1777, 2503-2531; so does this host code, one fused cell kernel per step)
# ----------------------------------------------------------------------------
class _LSTMCellStep(torch.autograd.Function):
    """(xw, hw, c_prev[, gate_ovr]) -> (h, c).  gates = xw + hw (biases inside), order i,f,g,o; gate
    ``gate_idx`` may take an externally computed activation (GPNN output)."""

    @staticmethod
    def forward(ctx, xw, hw, c_prev, gate_ovr, gate_idx):
        xw, hw, c_prev = _f32(xw, "xw"), _f32(hw, "hw"), _f32(c_prev, "c_prev")
        B, G = xw.shape
        H = G // 4
        h = _new(xw.device, B, H)
        c = torch.empty_like(h)
        ga = _new(xw.device, B, G)
        L.require_gfx950()
        if gate_ovr is None:
            calls().blm_lstm_cell_fwd(ptr(xw), ptr(hw), ptr(c_prev), ptr(h), ptr(c), ptr(ga), B, H, stream())
        else:
            gate_ovr = _f32(gate_ovr, "gate_ovr")
            calls().blm_lstm_cell_ovr_fwd(ptr(xw), ptr(hw), ptr(c_prev), ptr(gate_ovr), int(gate_idx), ptr(h), ptr(c), ptr(ga), B, H, stream())
        ctx.save_for_backward(c_prev, c, ga)
        ctx.meta = (gate_ovr is not None, int(gate_idx), B, H)
        return h, c

    @staticmethod
    def backward(ctx, dh, dc):
        c_prev, c, ga = ctx.saved_tensors
        has_ovr, gidx, B, H = ctx.meta
        dev = c.device
        dh = torch.zeros(B, H, device=dev) if dh is None else _f32(dh, "dh")
        dc = None if dc is None else _f32(dc, "dc")
        dgates = _new(dev, B, 4 * H)
        dc_prev = _new(dev, B, H)
        d_ovr = None
        if has_ovr:
            d_ovr = _new(dev, B, H)
            calls().blm_lstm_cell_ovr_bwd(ptr(dh), ptr(dc), ptr(c_prev), ptr(c), ptr(ga), gidx, ptr(dgates), ptr(d_ovr), ptr(dc_prev), B, H, stream())
        else:
            calls().blm_lstm_cell_bwd(ptr(dh), ptr(dc), ptr(c_prev), ptr(c), ptr(ga), ptr(dgates), ptr(dc_prev), B, H, stream())
        return dgates, dgates, dc_prev, d_ovr, None


def lstm_cell(xw, hw, c_prev, gate_ovr=None, gate_idx=-1):
    return _LSTMCellStep.apply(xw, hw, c_prev, gate_ovr, gate_idx)


class _GPMix(torch.autograd.Function):
    """out = sum_i act_i(z) * coef4[i]  with the fixed slot order tanh, sigmoid, relu, gelu."""

    @staticmethod
    def forward(ctx, z, coef4):
        z, coef4 = _f32(z, "z"), _f32(coef4, "coef4")
        N = z.shape[-1]
        M = z.numel() // N
        out = torch.empty_like(z)
        L.require_gfx950()
        calls().blm_gp_mix_fwd(ptr(z), ptr(coef4), ptr(out), M, N, stream())
        ctx.save_for_backward(z, coef4)
        return out

    @staticmethod
    def backward(ctx, dout):
        z, coef4 = ctx.saved_tensors
        dout = _f32(dout, "dout")
        N = z.shape[-1]
        M = z.numel() // N
        dz = torch.empty_like(z)
        calls().blm_gp_mix_bwd(ptr(dout), ptr(z), ptr(coef4), ptr(dz), M, N, stream())
        dcoef = torch.zeros_like(coef4)
        calls().blm_gp_coef_grad(ptr(dout), ptr(z), ptr(dcoef), M, N, stream())
        return dz, dcoef


def gp_mix(z, coef4):
    return _GPMix.apply(z, coef4)


class _AddRowVec(torch.autograd.Function):
    """h (B,H) + v (H,) broadcast over rows (VNN noise on the hidden state, model.py:2571-2577)."""

    @staticmethod
    def forward(ctx, h, v):
        out = _f32(h, "h").clone()
        v = _f32(v, "v")
        B, H = out.shape
        L.require_gfx950()
        calls().blm_add_rowvec(ptr(out), ptr(v), B, H, stream())
        return out

    @staticmethod
    def backward(ctx, g):
        g = _f32(g, "g")
        B, H = g.shape
        dv = _new(g.device, H)
        _colsum_into(g, B, H, dv, accumulate=False)
        return g, dv


def add_rowvec(h, v):
    return _AddRowVec.apply(h, v)


# ----------------------------------------------------------------------------
# optimiser:  clip_grad_norm_ + SGD(momentum)   (train.py:419-420,466)
# ----------------------------------------------------------------------------
class PtrTable:
    """Device arrays of pointers/sizes for the multi-tensor kernels (built once per tensor list)."""

    def __init__(self, params, grads, bufs):
        dev = params[0].device
        self.n = len(params)
        self.params = torch.tensor([p.data_ptr() for p in params], dtype=torch.int64, device=dev)
        self.grads = torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64, device=dev)
        self.bufs = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device=dev)
        self.sizes = torch.tensor([p.numel() for p in params], dtype=torch.int64, device=dev)
        self.sq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.ws = torch.zeros(int(calls().blm_sqnorm_ws_floats(self.n)), dtype=torch.float32, device=dev)
        self._keep = (params, grads, bufs)


def clip_sgd(table, clip, lr, momentum, first, grad_scale=1.0, weight_decay=0.0):
    """-> device scalar holding the squared global gradient norm (before grad_scale).  ``weight_decay``:
    torch.optim.SGD's L2 term, added after the clip (train_search_bayes.py:391-392)."""
    L.require_gfx950()
    table.sq.zero_()
    st = stream()
    calls().blm_sqnorm_multi(ptr(table.grads), ptr(table.sizes), table.n, ptr(table.sq), ptr(table.ws), st)
    if weight_decay:
        calls().blm_clip_sgd_multi_wd(ptr(table.params), ptr(table.grads), ptr(table.bufs), ptr(table.sizes), table.n,
                                      ptr(table.sq), float(clip), float(lr), float(momentum), 1 if first else 0,
                                      float(grad_scale), float(weight_decay), st)
    else:
        calls().blm_clip_sgd_multi(ptr(table.params), ptr(table.grads), ptr(table.bufs), ptr(table.sizes), table.n,
                                   ptr(table.sq), float(clip), float(lr), float(momentum), 1 if first else 0,
                                   float(grad_scale), st)
    return table.sq


def sqnorm(table):
    """-> table.sq, the device scalar holding the squared global gradient norm (blm_sqnorm_multi, as clip_sgd runs it)"""
    L.require_gfx950()
    table.sq.zero_()
    calls().blm_sqnorm_multi(ptr(table.grads), ptr(table.sizes), table.n, ptr(table.sq), ptr(table.ws), stream())
    return table.sq


def sgmcmc_update(p, g, sq, clip, lr, sigma, seed=0, step=0, v=None, grad_scale=1.0, weight_decay=0.0, alpha=0.99, damping=1e-5,
                  stream_id=None):
    """One SG-MCMC update over flat float32 arrays of one length, in place on ``p`` (and ``v``) (blm_sgmcmc_update, one pass):
    with c = min(1, clip / (sqrt(sq) grad_scale + 1e-6)) grad_scale and d = c g + weight_decay p,
      sgld  (``v`` None):  p <- p - lr d + sigma xi
      psgld:               v <- alpha v + (1 - alpha) d d,  G = 1 / (damping + sqrt(v)),  p <- p - lr G d + sigma sqrt(G) xi
    xi[i] element i of the Philox normal stream (seed, stream_id = STREAM_SGMCMC, step), i the index into the arrays handed in.
    ``sq``: the device scalar sqnorm / clip_sgd leave.  sigma = 0 runs the form without the generator.  The defaults of alpha and
    damping are RMSprop's customary ones and are unmeasured here.  -> p"""
    arrays = dict(p=p, g=g) if v is None else dict(p=p, g=g, v=v)
    n = _dyneval_flat("sgmcmc_update", **arrays)
    if _dyneval_flat("sgmcmc_update", sq=sq) != 1:
        raise BayesLMError("sgmcmc_update: sq must hold 1 float (the squared gradient norm), got %d" % sq.numel())
    lr, sigma, weight_decay = (_dyneval_rate("sgmcmc_update", k, x) for k, x in (("lr", lr), ("sigma", sigma),
                                                                                 ("weight_decay", weight_decay)))
    clip, alpha, damping = float(clip), float(alpha), float(damping)
    if not clip > 0.0:
        raise BayesLMError("sgmcmc_update: clip = %r must be > 0" % clip)
    if v is not None and not (0.0 <= alpha < 1.0 and damping > 0.0):
        raise BayesLMError("sgmcmc_update: alpha = %r must lie in [0, 1) and damping = %r be > 0" % (alpha, damping))
    L.require_gfx950()
    r = L.rng(seed, L.STREAM_SGMCMC if stream_id is None else stream_id, int(step))
    calls().blm_sgmcmc_update(ptr(p), ptr(g), ptr(v), ptr(sq), n, clip, lr, float(grad_scale), weight_decay, sigma, alpha, damping,
                              C.byref(r), stream())
    return p


def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """In-place torch.optim.Adam update of one tensor (architect.py:33); ``step`` counts from 1."""
    L.require_gfx950()
    calls().blm_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), float(lr), float(betas[0]), float(betas[1]),
                          float(eps), float(weight_decay), int(step), stream())


# ----------------------------------------------------------------------------
# architecture search (model_search_bayes.py): branch mixes with gradients for the mixing weights
# ----------------------------------------------------------------------------
def _reduce_partials(partial, k):
    """(n, k) per-block partial sums -> (k,) on the device."""
    out = _new(partial.device, k)
    _colsum_into(partial, partial.numel() // k, k, out, accumulate=False)
    return out


def _drop_args(drop, B):
    if drop is not None and drop.on:
        return float(drop.p), C.byref(drop.rng()), int(drop.col_offset), int(drop.global_cols or B)
    return 0.0, None, 0, 0


class _Mix2(torch.autograd.Function):
    """out = (p[0] a + p[1] b) * keep over (rows, B, N) activations, probs (2,) on the device
    (BayesTransSearchEncoderLayer, model_search_bayes.py:77-78)."""

    @staticmethod
    def forward(ctx, a, b, probs, drop):
        a, b, probs = _f32(a, "a"), _f32(b, "b"), _f32(probs, "probs")
        N, B = a.shape[-1], a.shape[-2]
        rows = a.numel() // (B * N)
        out = torch.empty_like(a)
        dp, drng, dco, dgc = _drop_args(drop, B)
        L.require_gfx950()
        calls().blm_mix2_fwd(ptr(a), ptr(b), ptr(probs), ptr(out), rows, B, N, dp, drng, dco, dgc, stream())
        ctx.save_for_backward(a, b, probs)
        ctx.meta = (drop, rows, B, N)
        return out

    @staticmethod
    def backward(ctx, dout):
        a, b, probs = ctx.saved_tensors
        drop, rows, B, N = ctx.meta
        dout = _f32(dout, "dout")
        da = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        db = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        partial = _new(a.device, int(calls().blm_mix2_partials(rows, B, N)))
        dp, drng, dco, dgc = _drop_args(drop, B)
        calls().blm_mix2_bwd(ptr(dout), ptr(a), ptr(b), ptr(probs), None, ptr(da), ptr(db), ptr(partial), rows, B, N, dp, drng, dco, dgc, stream())
        dprobs = _reduce_partials(partial, 2) if ctx.needs_input_grad[2] else None
        return da, db, dprobs, None


def mix2(a, b, probs, drop=NO_DROP):
    return _Mix2.apply(a, b, probs, drop)


class _SearchFFN(torch.autograd.Function):
    """y = lin2(drop(p[0] * GELU(x W1^T + b1) + p[1] * sum_i act_i(x Wg^T + bg) coef[i]))
    GaussTransSearchEncoderLayer FFN (model_search_bayes.py:234-236).  ``probs`` (2,) lives on the device and
    gets its gradient; wg/bg/coef may be leaf parameters or sampled (non-leaf) tensors.  The weight-gradient
    GEMMs are skipped for tensors that do not require grad (the architect step differentiates w.r.t. the
    architecture logits only, architect.py:66-75)."""

    @staticmethod
    def forward(ctx, x, w1, b1, wg, bg, coef, probs, w2, b2, drop):
        x, probs = _f32(x, "x"), _f32(probs, "probs")
        F_, D = w1.shape
        N2 = w2.shape[0]
        M = x.numel() // D
        B = x.shape[-2]
        rows = M // B
        dev = x.device
        need_bwd = any(ctx.needs_input_grad)
        a1 = _new(dev, M, F_) if need_bwd else None
        zg = _new(dev, M, F_) if need_bwd else None
        h1 = _new(dev, M, F_)
        hg = _new(dev, M, F_)
        gemm(L.GEMM_NT, x, w1, h1, M, F_, D, D, D, F_, epilogue=L.EPI_BIAS_GELU, bias=b1, aux=a1)
        gemm(L.GEMM_NT, x, wg, hg, M, F_, D, D, D, F_, epilogue=L.EPI_GP_MIX, bias=bg, aux=zg, coef=coef)
        s = _new(dev, M, F_)
        dp, drng, dco, dgc = _drop_args(drop, B)
        calls().blm_mix2_fwd(ptr(h1), ptr(hg), ptr(probs), ptr(s), rows, B, F_, dp, drng, dco, dgc, stream())
        y = _new(dev, *x.shape[:-1], N2)
        gemm(L.GEMM_NT, s, w2, y, M, N2, F_, F_, F_, N2, epilogue=L.EPI_BIAS, bias=b2)
        ctx.save_for_backward(x, a1, h1, zg, hg, s, probs)
        ctx.p = (w1, b1, wg, bg, coef, w2, b2, drop, B)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, a1, h1, zg, hg, s, probs = ctx.saved_tensors
        w1, b1, wg, bg, coef, w2, b2, drop, B = ctx.p
        dy = _f32(dy, "dy")
        F_, D = w1.shape
        N2 = w2.shape[0]
        M = x.numel() // D
        rows = M // B
        dev = x.device
        st = stream()
        ds = _new(dev, M, F_)
        gemm(L.GEMM_NN, dy, w2, ds, M, F_, N2, N2, F_, F_)
        partial = _new(dev, int(calls().blm_mix2_partials(rows, B, F_)))
        dz1 = _new(dev, M, F_)
        dzg = _new(dev, M, F_)
        dp, drng, dco, dgc = _drop_args(drop, B)
        # one pass: dz1 = p0 g GELU'(z1), dzg = p1 g mixture'(zg), the two mixing-weight partials, and -- only when
        # the coefficients want their gradient -- dhg = p1 g for blm_gp_coef_grad
        dhg = _new(dev, M, F_) if coef.requires_grad else None
        calls().blm_mix2_gp_bwd(ptr(ds), ptr(h1), ptr(hg), ptr(probs), ptr(a1), ptr(zg), ptr(coef), ptr(dz1), ptr(dzg),
                                ptr(dhg), ptr(partial), rows, B, F_, dp, drng, dco, dgc, st)
        dprobs = _reduce_partials(partial, 2) if ctx.needs_input_grad[6] else None
        dcoef = None
        if coef.requires_grad:
            buf, _, dcoef = _wgrad_target(coef)
            if dcoef is not None:
                buf.zero_()
            calls().blm_gp_coef_grad(ptr(dhg), ptr(zg), ptr(buf), M, F_, st)
            del dhg
        if w2.requires_grad:
            gemm(L.GEMM_TN, dy, s, _grad_buf(w2), N2, F_, M, N2, F_, F_, accumulate=True,
                 colsum_a=_grad_buf(b2) if b2.requires_grad else None)
        elif b2.requires_grad:
            _colsum_into(dy, M, N2, _grad_buf(b2))
        if w1.requires_grad:
            gemm(L.GEMM_TN, dz1, x, _grad_buf(w1), F_, D, M, F_, D, D, accumulate=True,
                 colsum_a=_grad_buf(b1) if b1.requires_grad else None)
        elif b1.requires_grad:
            _colsum_into(dz1, M, F_, _grad_buf(b1))
        dwg = dbg = None
        if wg.requires_grad:
            buf, acc, dwg = _wgrad_target(wg)
            gemm(L.GEMM_TN, dzg, x, buf, F_, D, M, F_, D, D, accumulate=acc)
        if bg.requires_grad:
            buf, acc, dbg = _wgrad_target(bg)
            _colsum_into(dzg, M, F_, buf, accumulate=acc)
        _notify(w2, b2, w1, b1, wg, bg, coef)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            gemm(L.GEMM_NN, dz1, w1, dx, M, D, F_, F_, D, D)
            gemm(L.GEMM_NN, dzg, wg, dx, M, D, F_, F_, D, D, accumulate=True)
        return dx, None, None, dwg, dbg, dcoef, dprobs, None, None, None


def search_ffn(x, w1, b1, wg, bg, coef, probs, w2, b2, drop=NO_DROP):
    wg, bg, coef = _weight(wg, "wg"), _weight(bg, "bg"), _weight(coef, "coef")  # gradients through _wgrad_target
    w1, b1, w2, b2 = (_weight(t, n, in_place=True) for t, n in ((w1, "w1"), (b1, "b1"), (w2, "w2"), (b2, "b2")))
    return _SearchFFN.apply(x, w1, b1, wg, bg, coef, probs, w2, b2, drop)


class _LSTMSearchLayer(torch.autograd.Function):
    """One BayesLSTMSearchCell over a window (model_search_bayes.py:661-710).  w8_ih (8H,I), w8_hh (8H,H),
    bias8 (8H): the standard gate block [i f g o] stacked on the four `Bayes` gate maps; probs (4,2) on the
    device.  Per step: one (B,8H) recurrent GEMM + the pointwise search cell; the input products of all
    steps, both weight gradients and dx are single GEMMs over the whole window."""

    @staticmethod
    def forward(ctx, x, h0, c0, w8_ih, w8_hh, bias8, probs):
        x, h0, c0, probs = _f32(x, "x"), _f32(h0, "h0"), _f32(c0, "c0"), _f32(probs, "probs")
        w8_ih, w8_hh, bias8 = _f32(w8_ih, "w8_ih"), _f32(w8_hh, "w8_hh"), _f32(bias8, "bias8")
        T, B, I = x.shape
        H = h0.shape[-1]
        dev = x.device
        st = stream()
        need_bwd = any(ctx.needs_input_grad)
        xw = _new(dev, T, B, 8 * H)
        gemm(L.GEMM_NT, x, w8_ih, xw, T * B, 8 * H, I, I, I, 8 * H, epilogue=L.EPI_BIAS, bias=bias8)
        hs = _new(dev, T + 1, B, H)
        cs = _new(dev, T + 1, B, H)
        hs[0].copy_(h0)
        cs[0].copy_(c0)
        acts = _new(dev, T, B, 8 * H) if need_bwd else None
        if H % 32 == 0:  # one launch per step: recurrent product over the stacked weight + the search cell
            xw_p, hs_p, cs_p, w_p, pr_p = _P(xw), _P(hs), _P(cs), ptr(w8_hh), ptr(probs)
            ac_p = _P(acts) if need_bwd else None
            step_fwd = calls().blm_lstm_search_step_fwd
            for t in range(T):
                step_fwd(xw_p[t], w_p, hs_p[t], cs_p[t], pr_p, hs_p[t + 1], cs_p[t + 1], ac_p[t] if need_bwd else None, B, H, st)
        else:
            hw = _new(dev, B, 8 * H)
            for t in range(T):
                gemm(L.GEMM_NT, hs[t], w8_hh, hw, B, 8 * H, H, H, H, 8 * H)
                calls().blm_lstm_search_cell_fwd(ptr(xw[t]), ptr(hw), ptr(cs[t]), ptr(probs), ptr(hs[t + 1]),
                                                 ptr(cs[t + 1]), ptr(acts[t]) if need_bwd else None, B, H, st)
        ctx.save_for_backward(x, hs, cs, acts, w8_ih, w8_hh, probs)
        ctx.dims = (T, B, I, H)
        return hs[1:], hs[T], cs[T]

    @staticmethod
    def backward(ctx, dy, dhT, dcT):
        x, hs, cs, acts, w8_ih, w8_hh, probs = ctx.saved_tensors
        T, B, I, H = ctx.dims
        dev = x.device
        st = stream()
        dy = _f32(dy.contiguous(), "dy")
        npart = int(calls().blm_lstm_search_cell_partials(B, H))
        part = _new(dev, T, npart)
        dz = _new(dev, T, B, 8 * H)
        dcb = [_new(dev, B, H) for _ in range(2)]
        dhr = [_new(dev, B, H) for _ in range(2)]
        dh_rec = _f32(dhT.contiguous(), "dhT") if dhT is not None else None
        dc = _f32(dcT.contiguous(), "dcT") if dcT is not None else None
        # H % 16 == 0: one launch per step -- the skinny recurrent dgrad dh = dz8 . W8 on the LSTM step kernel (fixed
        # summation order, no split-K memset + atomics) against the weight transposed once per window, with the
        # search cell's backward of the previous step fused behind it; otherwise cell kernel + blm_gemm per step
        fused = H % 16 == 0
        part2 = None
        if fused:
            w_t = _new(dev, H, 8 * H)
            calls().blm_transpose(ptr(w8_hh), ptr(w_t), 8 * H, H, st)
            part = _new(dev, 1, npart)
            calls().blm_lstm_search_cell_bwd(ptr(dy[T - 1]), ptr(dh_rec), ptr(dc), ptr(cs[T - 1]), ptr(cs[T]),
                                             ptr(acts[T - 1]), ptr(probs), ptr(dz[T - 1]), ptr(dcb[0]), ptr(part[0]), B, H, st)
            nstep = int(calls().blm_lstm_search_step_partials(B, H))
            part2 = _new(dev, max(T - 1, 1), nstep)
            k = 0
            dz_p, dy_p, cs_p, ac_p, p2_p = _P(dz), _P(dy), _P(cs), _P(acts), _P(part2)
            dcb_p, wt_p, pr_p = (ptr(dcb[0]), ptr(dcb[1])), ptr(w_t), ptr(probs)
            step_bwd = calls().blm_lstm_search_step_bwd
            for t in range(T - 1, 0, -1):
                step_bwd(dz_p[t], wt_p, dy_p[t - 1], dcb_p[k], cs_p[t - 1], cs_p[t], ac_p[t - 1], pr_p, dz_p[t - 1],
                         dcb_p[k ^ 1], p2_p[t - 1], B, H, st)
                k ^= 1
            calls().blm_lstm_step_dh(ptr(dz[0]), ptr(w_t), ptr(dhr[0]), B, H, 8 * H, st)
            dh_rec, dc = dhr[0], dcb[k]
            if T == 1:
                part2 = None
        else:
            for t in range(T - 1, -1, -1):
                k = t & 1
                calls().blm_lstm_search_cell_bwd(ptr(dy[t]), ptr(dh_rec), ptr(dc), ptr(cs[t]), ptr(cs[t + 1]), ptr(acts[t]),
                                                 ptr(probs), ptr(dz[t]), ptr(dcb[k]), ptr(part[t]), B, H, st)
                dc = dcb[k]
                gemm(L.GEMM_NN, dz[t], w8_hh, dhr[k], B, H, 8 * H, 8 * H, H, H)
                dh_rec = dhr[k]
        dprobs = None
        if ctx.needs_input_grad[6]:
            dprobs = _reduce_partials(part, 8)
            if part2 is not None:
                dprobs = dprobs + _reduce_partials(part2, 8)
            dprobs = dprobs.view(4, 2)
        dw_ih = dw_hh = db = dx = None
        M = T * B
        if ctx.needs_input_grad[4]:
            dw_hh = torch.empty_like(w8_hh)
            gemm(L.GEMM_TN, dz, hs, dw_hh, 8 * H, H, M, 8 * H, H, H)
        if ctx.needs_input_grad[3]:
            dw_ih = torch.empty_like(w8_ih)
            db = _new(dev, 8 * H) if ctx.needs_input_grad[5] else None
            if db is not None:
                db.zero_()
            gemm(L.GEMM_TN, dz, x, dw_ih, 8 * H, I, M, 8 * H, I, I, colsum_a=db)
        elif ctx.needs_input_grad[5]:
            db = _new(dev, 8 * H)
            _colsum_into(dz, M, 8 * H, db, accumulate=False)
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            gemm(L.GEMM_NN, dz, w8_ih, dx, M, I, 8 * H, 8 * H, I, I)
        return dx, dh_rec, dc, dw_ih, dw_hh, db, dprobs


def lstm_search_layer(x, h0, c0, w8_ih, w8_hh, bias8, probs):
    return _LSTMSearchLayer.apply(x, h0, c0, w8_ih, w8_hh, bias8, probs)


# ----------------------------------------------------------------------------
# word error rate of n-best lists: alignment in bulk, selection over a weight grid, minimum Bayes risk (csrc/nbest.hip)
# ----------------------------------------------------------------------------
def _i32(t, name):
    return dev_tensor(t, name, torch.int32)


def _i64(t, name):
    return dev_tensor(t, name, torch.int64)


def _f64_or_none(t, name, H=None):
    if t is None:
        return None
    t = dev_tensor(t, name, torch.float64).reshape(-1)
    if H is not None and t.numel() != H:
        raise BayesLMError("%s holds %d values for %d hypotheses" % (name, t.numel(), H))
    return t


def nbest_grids(points, what="nbest_select"):
    """The blm_nbest_grid structs of a list of grid points (L, w, p) or (L, w, p, s) (s = 1 where it is left out), 64 points
    to a struct: L finite and > 0, s finite and >= 0 (include/bayeslm.h).  -> [(first point, struct), ...]"""
    pts = []
    for k, pt in enumerate(points):
        try:
            pt = tuple(float(v) for v in pt)
        except (TypeError, ValueError):
            pt = ()
        if len(pt) == 3:
            pt = pt + (1.0,)
        if len(pt) != 4:
            raise BayesLMError("%s: grid point %d must be (lmwt, nnweight, wip[, posterior scale]), got %r" % (what, k, points[k]))
        if not (math.isfinite(pt[0]) and pt[0] > 0.0):
            raise BayesLMError("%s: grid point %d: lmwt = %r is not a positive finite LM weight" % (what, k, pt[0]))
        if not (math.isfinite(pt[3]) and pt[3] >= 0.0):
            raise BayesLMError("%s: grid point %d: posterior scale = %r is not a finite number >= 0" % (what, k, pt[3]))
        pts.append(pt)
    if not pts:
        raise BayesLMError("%s: an empty grid" % what)
    out = []
    for k0 in range(0, len(pts), L.NBEST_GRID_MAX):
        chunk = pts[k0:k0 + L.NBEST_GRID_MAX]
        s = L.NbestGrid()
        s.abi_version, s.G = L.ABI_VERSION, len(chunk)
        for k, (lw, w, p, ps) in enumerate(chunk):
            s.lmwt[k], s.nnweight[k], s.wip[k], s.pscale[k] = lw, w, p, ps
        out.append((k0, s))
    return out


def edit_distance(tok, off, a, b, breakdown=False):
    """Word-level alignment of P pairs of sequences (blm_edit_distance): ``tok`` int32 word ids, flat; ``off`` (n_seq + 1,) int64
    offsets; ``a`` / ``b`` (P,) int32 sequence indices, a the hypothesis and b the reference.  -> cost (P,) int32, the minimum
    number of substitutions + insertions + deletions; with ``breakdown`` also sid (P, 3) int32 = sub / ins / del of the
    minimum-cost alignment with the fewest insertions.  A bad pair (an index outside the sequences, a reversed offset range or one
    that leaves tok, more than 1023 words) gets -1 everywhere.  Integer and exact."""
    tok, off = _i32(tok, "tok").reshape(-1), _i64(off, "off").reshape(-1)
    a, b = _i32(a, "a").reshape(-1), _i32(b, "b").reshape(-1)
    if off.numel() < 1:
        raise BayesLMError("edit_distance: off must hold n_seq + 1 offsets")
    if a.numel() != b.numel():
        raise BayesLMError("edit_distance: %d indices in a, %d in b" % (a.numel(), b.numel()))
    P = a.numel()
    cost = torch.empty(P, device=a.device, dtype=torch.int32)
    sid = torch.empty(P, 3, device=a.device, dtype=torch.int32) if breakdown else None
    if P:
        L.require_gfx950()
        calls().blm_edit_distance(ptr(tok) if tok.numel() else None, tok.numel(), ptr(off), off.numel() - 1, ptr(a), ptr(b), P,
                                  ptr(cost), ptr(sid), stream())
    return (cost, sid) if breakdown else cost


def pairwise_edit_distance(tok, off, uoff):
    """The distance blocks blm_nbest_mbr reads: group u owns sequences uoff[u] .. uoff[u + 1] of (tok, off), N of them; every
    pair i < j of a group is aligned once (blm_edit_distance) and written to both halves of the group's dense N x N block.
    -> (dist (sum of N^2,) int32, doff (U,) int64 block offsets).  Index building and the fill are plain torch."""
    tok, off, uoff = _i32(tok, "tok").reshape(-1), _i64(off, "off").reshape(-1), _i64(uoff, "uoff").reshape(-1)
    if uoff.numel() < 1:
        raise BayesLMError("pairwise_edit_distance: uoff must hold U + 1 offsets")
    dev = uoff.device
    n = (uoff[1:] - uoff[:-1]).clamp_(min=0)
    sq = n * n
    ends = torch.cumsum(sq, 0)
    doff = ends - sq
    total = int(ends[-1]) if ends.numel() else 0
    dist = torch.zeros(total, device=dev, dtype=torch.int32)
    if total == 0:
        return dist, doff
    if total > 2 ** 30:
        raise BayesLMError("pairwise_edit_distance: %d block elements in one call, at most 2^30 (batch the utterances)" % total)
    grp = torch.repeat_interleave(torch.arange(n.numel(), device=dev), sq)
    local = torch.arange(total, device=dev) - doff[grp]
    ng = n[grp]
    i, j = torch.div(local, ng, rounding_mode="floor"), local % ng
    upper = i < j
    grp, i, j, ng = grp[upper], i[upper], j[upper], ng[upper]
    base = uoff[grp]
    cost = edit_distance(tok, off, (base + i).to(torch.int32), (base + j).to(torch.int32))
    dist[doff[grp] + i * ng + j] = cost
    dist[doff[grp] + j * ng + i] = cost
    return dist, doff


def _nbest_costs(what, ac, g, lm, nn, length, uoff):
    uoff = _i64(uoff, "uoff").reshape(-1)
    if uoff.numel() < 1:
        raise BayesLMError("%s: uoff must hold U + 1 offsets" % what)
    given = [t for t in (ac, g, lm, nn, length) if t is not None]
    H = given[0].numel() if given else None
    arrs = [_f64_or_none(t, n, H) for t, n in ((ac, "ac"), (g, "g"), (lm, "lm"), (nn, "nn"), (length, "length"))]
    return arrs, uoff, H


def nbest_select(ac, g, lm, nn, length, uoff, grid):
    """The best hypothesis of every group at every grid point (blm_nbest_select).  ac / g / lm / nn / length: (H,) float64
    COSTS per hypothesis, each may be None (zeros); group u owns uoff[u] .. uoff[u + 1]; ``grid``: points (L, w, p[, s]).
    T = ac + L (g + w nn + (1 - w) lm + p length); -> pick (G, U) int32, per point and group the index WITHIN the group of the
    least T, lowest index on ties (a non-finite T never wins; none finite: 0; an empty group: -1).  A grid of more than 64
    points takes one launch per 64."""
    arrs, uoff, _ = _nbest_costs("nbest_select", ac, g, lm, nn, length, uoff)
    chunks = nbest_grids(grid, "nbest_select")
    U = uoff.numel() - 1
    G = chunks[-1][0] + chunks[-1][1].G
    pick = torch.empty(G, U, device=uoff.device, dtype=torch.int32)
    if U:
        L.require_gfx950()
        for k0, s in chunks:
            calls().blm_nbest_select(*[ptr(t) for t in arrs], ptr(uoff), U, C.byref(s), ptr(pick[k0:k0 + s.G]), stream())
    return pick


def nbest_mbr(ac, g, lm, nn, length, uoff, dist, doff, grid, want_risk=True):
    """Minimum-Bayes-risk selection (blm_nbest_mbr): with T as in nbest_select, P_i = exp(-s (T_i - min T) / L) / sum over the
    group and R_i = sum_j P_j d(i, j) over the group's symmetric distance block (pairwise_edit_distance's ``dist`` / ``doff``).
    At least one cost array must be given (it fixes H).  -> (risk (G, H) float64 or None, pick (G, U) int32: the argmin of R,
    lowest index on ties, -1 for an empty group).  A grid of more than 64 points takes one launch per 64."""
    arrs, uoff, H = _nbest_costs("nbest_mbr", ac, g, lm, nn, length, uoff)
    if H is None:
        raise BayesLMError("nbest_mbr: at least one of ac, g, lm, nn, length must be given")
    dist, doff = _i32(dist, "dist").reshape(-1), _i64(doff, "doff").reshape(-1)
    U = uoff.numel() - 1
    if doff.numel() != U:
        raise BayesLMError("nbest_mbr: %d block offsets for %d groups" % (doff.numel(), U))
    chunks = nbest_grids(grid, "nbest_mbr")
    G = chunks[-1][0] + chunks[-1][1].G
    pick = torch.empty(G, U, device=uoff.device, dtype=torch.int32)
    risk = torch.zeros(G, H, device=uoff.device, dtype=torch.float64) if want_risk else None
    if U:
        L.require_gfx950()
        for k0, s in chunks:
            # every group empty: no block is read, and an empty tensor has no address to pass for the required pointer
            calls().blm_nbest_mbr(*[ptr(t) for t in arrs], ptr(uoff), U, H, ptr(dist) if dist.numel() else ptr(doff), ptr(doff),
                                  C.byref(s), ptr(risk[k0:k0 + s.G]) if want_risk else None, ptr(pick[k0:k0 + s.G]), stream())
    return risk, pick
