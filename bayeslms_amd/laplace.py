"""Last-layer Laplace approximation for the decoder (MacKay 1992; Kristiadi, Hein, Hennig 2020; Daxberger et al. 2021): a
Gaussian posterior over the vocabulary projection of a model that is already trained, from one pass over a text and no
retraining, for any checkpoint (``--uncertainty none`` and the rest alike, at their mean weights).

    posterior = engine.fit_laplace(model, train_stream, seq_len, max_windows=200)
    posterior.save("laplace.pt")
    ...
    posterior = LaplacePosterior.load("laplace.pt", device)
    fit = engine.fit_laplace_prior(model, valid_stream, seq_len, posterior, [1.0, 10.0, 100.0])
    report = engine.evaluate_laplace(model, test_stream, seq_len, posterior, fit.tau, link="probit")

What is kept is the diagonal of the generalised Gauss-Newton matrix of the decoder z = W h + b, summed over the N rows of the
fit text: F_W[v, k] = sum_t a_t[v] h_t[k]^2 and F_b[v] = sum_t a_t[v] with a_t = p_t (1 - p_t).  The prior N(0, 1/tau I) enters
only when the posterior is used: Lambda = F + tau, and a new row h has the logit variance sum_k h[k]^2 / Lambda_W[v, k] +
1 / Lambda_b[v], one more decoder-sized product (ops.linear of h^2 against ``inverse(tau)``).  The definitions, the three links
to a next-word distribution and the kernels: include/bayeslm.h, csrc/laplace.hip."""
import hashlib
import math

import torch

from . import _lib as L
from . import ops
from ._lib import BayesLMError
from .swag import PosteriorMismatch

FORMAT = "bayeslms_amd.laplace/1"


class LaplaceMismatch(PosteriorMismatch):
    """A Laplace posterior was made for another decoder; ``field`` names the manifest field that differs."""

    def __init__(self, field, found, wanted):
        self.field, self.found, self.wanted = field, found, wanted
        BayesLMError.__init__(self, "laplace posterior: field %r differs: the posterior has %r, this model has %r"
                              % (field, found, wanted))


_FP_CHUNK = 1 << 22  # words per step of fingerprint(): 3 x 32 MB of transient int64 at most, whatever the decoder's size


def fingerprint(weight, bias):
    """A fingerprint of the bytes of the decoder's weight and bias, formed where they live (no copy of a (V, K) matrix to the
    host): per tensor the float32 words read as integers, their sum and their sum weighted by 1 + (index mod 65521), both modulo
    2^64 (an exact integer sum: the order of the additions does not matter), hashed with the shapes.  One changed element
    changes the first sum.  The words go through in steps of _FP_CHUNK and the four sums reach the host in one copy."""
    sums = []
    for t in (weight, bias):
        words = t.detach().to(torch.float32).contiguous().view(torch.int32).reshape(-1)
        plain = torch.zeros((), device=words.device, dtype=torch.int64)
        weighted = torch.zeros((), device=words.device, dtype=torch.int64)
        for a in range(0, words.numel(), _FP_CHUNK):
            v = words[a:a + _FP_CHUNK].to(torch.int64)
            i = torch.arange(a, a + v.numel(), device=v.device, dtype=torch.int64)
            plain += v.sum()
            weighted += (v * (i % 65521 + 1)).sum()
        sums += [plain, weighted]
    sums = torch.stack(sums).tolist()
    return hashlib.sha256(repr((tuple(weight.shape), tuple(bias.shape), sums)).encode()).hexdigest()


def manifest_of(decoder):
    """What a posterior was made for: the decoder's shape and the fingerprint of its weight and bias bytes."""
    w, b = decoder.weight, decoder.bias
    return {"shape": [int(w.shape[0]), int(w.shape[1])], "fingerprint": fingerprint(w, b)}


def _decoder_of(model):
    from .model import inference_decoder
    dec = inference_decoder(model)
    if dec is None:
        raise BayesLMError("laplace: %s has no decoder that hands back its input rows" % type(model).__name__)
    return dec


def prior_precision(value, who="laplace"):
    """``value`` as a prior precision tau: a float in (0, inf]; refuses anything else."""
    try:
        tau = float(value)
    except (TypeError, ValueError):
        tau = float("nan")
    if not tau > 0.0:
        raise BayesLMError("%s: prior precision %r is not a number in (0, inf]" % (who, value))
    return tau


def select_prior(taus, losses):
    """The candidate with the lowest loss -> its index; the first of equal losses wins, and a loss that is NaN never does.
    (fit_laplace_prior puts tau = inf first: the model itself wins a tie.)"""
    if len(taus) != len(losses) or not taus:
        raise BayesLMError("select_prior: %d candidates, %d losses" % (len(taus), len(losses)))
    best = None
    for i, v in enumerate(losses):
        if v == v and (best is None or v < losses[best]):
            best = i
    if best is None:
        raise BayesLMError("select_prior: every candidate's loss is NaN")
    return best


class LaplacePosterior:
    """f_w (V, K), f_b (V): the Gauss-Newton diagonal summed over ``n_tokens`` rows; ``manifest``: manifest_of(decoder).
    The sums live in buffers of Vq = V rounded up to 4 rows, so that a vocabulary that is no multiple of 4 accumulates from the
    padded logit rows ops.linear hands out; f_w and f_b are the (V, ...) views of them."""

    def __init__(self, V, K, device=None, manifest=None):
        V, K = int(V), int(K)
        if V < 1 or K < 1:
            raise BayesLMError("LaplacePosterior: decoder shape (%d, %d)" % (V, K))
        if manifest is not None and list(manifest["shape"]) != [V, K]:
            raise BayesLMError("LaplacePosterior: the manifest describes a decoder of %s, not (%d, %d)" % (manifest["shape"], V, K))
        self.V, self.K, self.n_tokens, self.manifest = V, K, 0, manifest
        Vq = (V + 3) // 4 * 4
        self._fw = torch.zeros(Vq, K, device=device, dtype=torch.float32)
        self._fb = torch.zeros(Vq, device=device, dtype=torch.float32)

    @property
    def f_w(self):
        return self._fw[:self.V]

    @property
    def f_b(self):
        return self._fb[:self.V]

    def accumulate(self, curvature_rows, h2_rows):
        """F_W += a^T h2 and F_b += the column sums of a, in ONE TN product of the GEMM family (BLM_GEMM_ACCUMULATE, colsum_a).
        ``curvature_rows`` (rows, V): what ops.laplace_curvature wrote -- where its rows are Vq apart, their pad columns (zeros,
        by that kernel) ride along so that every extent is a multiple of 4; they land in the Vq - V pad rows of the buffers,
        which f_w, f_b, inverse, check_finite and save never look at, so rows from elsewhere with anything in their padding
        do no harm either.  ``h2_rows`` (rows, K) contiguous: the squared decoder inputs."""
        a, h2 = curvature_rows, h2_rows
        if a.dim() != 2 or h2.dim() != 2 or a.shape[1] != self.V or h2.shape[1] != self.K or a.shape[0] != h2.shape[0]:
            raise BayesLMError("LaplacePosterior.accumulate: curvature %s and h2 %s against a decoder of (%d, %d)"
                               % (tuple(a.shape), tuple(h2.shape), self.V, self.K))
        if a.stride(-1) != 1 or not h2.is_contiguous():
            raise BayesLMError("LaplacePosterior.accumulate: row-major curvature rows and contiguous h2 rows expected")
        rows = a.shape[0]
        if rows == 0:
            return self.n_tokens
        lda = a.stride(0) if rows > 1 else max(a.stride(0), self.V)
        M = self._fw.shape[0] if lda >= self._fw.shape[0] else self.V
        ops.gemm(L.GEMM_TN, a, h2, self._fw, M, self.K, rows, lda, self.K, self.K, accumulate=True, colsum_a=self._fb)
        self.n_tokens += rows
        return self.n_tokens

    def inverse(self, tau):
        """(S_w, s_b) = (1 / (F_W + tau), 1 / (F_b + tau)), the operands of the variance product; tau = inf: zeros."""
        tau = prior_precision(tau, "LaplacePosterior.inverse")
        if math.isinf(tau):
            return torch.zeros_like(self.f_w), torch.zeros_like(self.f_b)
        return 1.0 / (self.f_w + tau), 1.0 / (self.f_b + tau)

    def check_finite(self):
        if not (bool(torch.isfinite(self.f_w).all()) and bool(torch.isfinite(self.f_b).all())):
            raise BayesLMError("laplace posterior: the accumulated curvature holds a value that is not finite")

    def state(self):
        return {"format": FORMAT, "shape": [self.V, self.K], "n_tokens": self.n_tokens, "manifest": self.manifest,
                "f_w": self.f_w.detach().cpu().clone(), "f_b": self.f_b.detach().cpu().clone()}

    def save(self, path):
        if self.n_tokens < 1:
            raise BayesLMError("LaplacePosterior.save: no row accumulated yet: nothing to write to %s" % path)
        with open(path, "wb") as f:
            torch.save(self.state(), f)

    @classmethod
    def load(cls, path, device=None):
        d = torch.load(path, map_location="cpu")
        if not isinstance(d, dict) or d.get("format") != FORMAT:
            raise BayesLMError("%s is not a Laplace posterior of this package (format %r expected, found %r)"
                               % (path, FORMAT, d.get("format") if isinstance(d, dict) else type(d).__name__))
        for k in ("shape", "n_tokens", "manifest", "f_w", "f_b"):
            if k not in d:
                raise BayesLMError("%s: field %r is missing" % (path, k))
        V, K = (int(v) for v in d["shape"])
        for k, shape in (("f_w", (V, K)), ("f_b", (V,))):
            t = d[k]
            if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32:
                raise BayesLMError("%s: %s is %s %s, float32 %s expected"
                                   % (path, k, getattr(t, "dtype", type(t).__name__), tuple(getattr(t, "shape", ())), shape))
        if int(d["n_tokens"]) < 1:
            raise BayesLMError("%s: n_tokens = %d" % (path, int(d["n_tokens"])))
        self = cls(V, K, device, d["manifest"])
        self._fw[:V].copy_(d["f_w"])
        self._fb[:V].copy_(d["f_b"])
        self.n_tokens = int(d["n_tokens"])
        return self

    def check(self, model):
        """Refuses a posterior made for another decoder: LaplaceMismatch names ``shape`` or ``fingerprint``."""
        dec = _decoder_of(model)
        shape = [int(dec.weight.shape[0]), int(dec.weight.shape[1])]
        if shape != [self.V, self.K]:
            raise LaplaceMismatch("shape", [self.V, self.K], shape)
        if self.manifest is None:
            return
        if list(self.manifest["shape"]) != shape:
            raise LaplaceMismatch("shape", list(self.manifest["shape"]), shape)
        theirs = fingerprint(dec.weight, dec.bias)
        if self.manifest["fingerprint"] != theirs:
            raise LaplaceMismatch("fingerprint", self.manifest["fingerprint"], theirs)

    def describe(self):
        """The ``laplace`` block of a report"""
        return {"tokens": self.n_tokens, "shape": [self.V, self.K],
                "fingerprint": None if self.manifest is None else self.manifest["fingerprint"][:16]}
