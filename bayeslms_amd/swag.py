"""SWAG (Maddox, Garipov, Izmailov, Vetrov, Wilson, NeurIPS 2019): a Gaussian over ALL weights of a model, fitted to the SGD
iterates at no training cost, for models trained without any variational site (``--uncertainty none`` and the rest alike).

    posterior = SwagPosterior(trainer.flat.total, rank=20, manifest=manifest_of(model))
    posterior.collect(trainer.flat.flat_param)      # once per epoch, or every N steps (SwagCollector)
    posterior.save("swag.pt")
    ...
    posterior = SwagPosterior.load("swag.pt", device)
    engine.evaluate_swag(model, source, seq_len, posterior, samples=8)

The posterior lives in the layout of engine.FlatBuffers: one flat float32 array of P floats, tied tensors once, every tensor
at a 16-byte aligned offset.  It holds the running mean (stochastic weight averaging, Izmailov et al. 2018), the Welford sum of
squared deviations m2 (var = m2 / n), and a ring of the K most recent deviations theta - mean.  Sample j is

    theta_j = mean + a sqrt(max(var, floor)) z1_j + b sum_{k < K_live} D[k] z2[j][k]

with a = sqrt(c / 2), b = sqrt(c / (2 (K_live - 1))) for K_live = min(n, K) >= 2, and the diagonal form a = sqrt(c), b = 0
otherwise or on request; c is the scale (0.5: the value Maddox et al. ran with; nobody has measured it here).  The definitions
and the kernels: include/bayeslm.h, csrc/swag.hip."""
import math

import torch

from . import _lib as L
from . import ops
from ._lib import BayesLMError

FORMAT = "bayeslms_amd.swag/1"
DRAW_BYTES = 8 << 30  # draw(): samples beyond this many bytes are refused (the neural cache's budget)


def flat_layout(model):
    """The trainable parameters of ``model`` as engine.FlatBuffers lays them out -> (parameters, offsets, total)"""
    params = [p for p in model.parameters() if p.requires_grad]
    offsets, off = [], 0
    for p in params:
        offsets.append(off)
        off += (p.numel() + 3) // 4 * 4
    return params, offsets, off


def manifest_of(model):
    """What a posterior was made for: the name (the first one of a tied tensor), shape and offset of every trainable parameter
    in the flat layout, and its length."""
    params, offsets, total = flat_layout(model)
    names = {}
    for name, p in model.named_parameters(remove_duplicate=False):
        names.setdefault(id(p), name)
    return {"total": total, "names": [names[id(p)] for p in params], "shapes": [list(p.shape) for p in params],
            "offsets": list(offsets)}


def coefficients(scale, k_live, diag=False):
    """-> (a, b, rows used): the full form a = sqrt(c / 2), b = sqrt(c / (2 (k_live - 1))) over k_live >= 2 deviation rows, else
    (or with ``diag``) the diagonal form a = sqrt(c), b = 0 over none."""
    c, k = float(scale), int(k_live)
    if not (math.isfinite(c) and c >= 0.0):
        raise BayesLMError("swag: scale = %r is not a finite number >= 0" % scale)
    if k < 0:
        raise BayesLMError("swag: k_live = %d" % k)
    if diag or k < 2:
        return math.sqrt(c), 0.0, 0
    return math.sqrt(c / 2.0), math.sqrt(c / (2.0 * (k - 1))), k


class PosteriorMismatch(BayesLMError):
    """A posterior (or a bank of weight vectors: ``what`` / ``owner`` name it) was made for another model; ``field`` names the first
    manifest field that differs."""

    def __init__(self, field, found, wanted, what="swag posterior", owner="posterior"):
        self.field, self.found, self.wanted = field, found, wanted
        super().__init__("%s: field %r differs: the %s has %r, this model has %r" % (what, field, owner, found, wanted))


def check_manifest(total, manifest, model_or_flat, what="swag posterior", owner="posterior"):
    """Refuses what was made for another model (PosteriorMismatch names the first manifest field that differs).  A model is
    compared by names, shapes and offsets; an engine.FlatBuffers, which knows no names, by shapes and offsets."""
    if hasattr(model_or_flat, "flat_param"):
        flat = model_or_flat
        theirs = {"total": flat.total, "names": None, "shapes": [list(p.shape) for p in flat.params], "offsets": list(flat.offsets)}
    else:
        theirs = manifest_of(model_or_flat)
    if theirs["total"] != total:
        raise PosteriorMismatch("total", total, theirs["total"], what, owner)
    if manifest is None:
        return
    for field in ("names", "shapes", "offsets"):
        a, b = manifest[field], theirs[field]
        if b is None or a == b:
            continue
        if len(a) != len(b):
            raise PosteriorMismatch("len(%s)" % field, len(a), len(b), what, owner)
        i = next(i for i, (x, y) in enumerate(zip(a, b)) if x != y)
        raise PosteriorMismatch("%s[%d]" % (field, i), a[i], b[i], what, owner)


class SwagPosterior:
    """mean, m2 (P,), the (K, P) ring of deviations and n, the number of iterates collected.  ``manifest``: manifest_of(model)."""

    def __init__(self, total, rank, device=None, manifest=None):
        total, rank = int(total), int(rank)
        if total < 1:
            raise BayesLMError("SwagPosterior: total = %d" % total)
        if not 0 <= rank <= L.SWAG_RANK_MAX:
            raise BayesLMError("SwagPosterior: rank = %d outside 0..%d (0: diagonal only)" % (rank, L.SWAG_RANK_MAX))
        if manifest is not None and manifest["total"] != total:
            raise BayesLMError("SwagPosterior: the manifest describes %d floats, total = %d" % (manifest["total"], total))
        self.total, self.rank, self.n, self.manifest = total, rank, 0, manifest
        # the kernel writes all three at n = 0 without reading them: no fill
        self.mean = torch.empty(total, device=device, dtype=torch.float32)
        self.m2 = torch.empty(total, device=device, dtype=torch.float32)
        self.dev = torch.empty(rank, total, device=device, dtype=torch.float32)

    @property
    def k_live(self):
        return min(self.n, self.rank)

    def collect(self, flat_param):
        """One iterate (blm_swag_collect): the flat weights as they are now."""
        if flat_param.numel() != self.total:
            raise BayesLMError("SwagPosterior.collect: %d floats, the posterior holds %d" % (flat_param.numel(), self.total))
        ops.swag_collect(flat_param, self.mean, self.m2, self.n, self.dev[self.n % self.rank] if self.rank else None)
        self.n += 1
        return self.n

    def variance(self):
        """The population variance m2 / n (float32, a new tensor)"""
        if self.n < 1:
            raise BayesLMError("SwagPosterior: no iterate collected yet")
        return self.m2 / float(self.n)

    def state(self):
        return {"format": FORMAT, "total": self.total, "rank": self.rank, "n": self.n, "manifest": self.manifest,
                "mean": self.mean.detach().cpu(), "m2": self.m2.detach().cpu(), "dev": self.dev.detach().cpu()}

    def save(self, path):
        if self.n < 1:
            raise BayesLMError("SwagPosterior.save: no iterate collected yet: nothing to write to %s" % path)
        with open(path, "wb") as f:
            torch.save(self.state(), f)

    @classmethod
    def load(cls, path, device=None):
        d = torch.load(path, map_location="cpu")
        if not isinstance(d, dict) or d.get("format") != FORMAT:
            raise BayesLMError("%s is not a SWAG posterior of this package (format %r expected)" % (path, FORMAT))
        self = cls.__new__(cls)
        self.total, self.rank, self.n, self.manifest = int(d["total"]), int(d["rank"]), int(d["n"]), d["manifest"]
        shapes = {"mean": (self.total,), "m2": (self.total,), "dev": (self.rank, self.total)}
        for k, shape in shapes.items():
            t = d[k]
            if tuple(t.shape) != shape or t.dtype != torch.float32:
                raise BayesLMError("%s: %s is %s %s, float32 %s expected" % (path, k, t.dtype, tuple(t.shape), shape))
            setattr(self, k, t.to(device).contiguous())
        if self.n < 1 or not 0 <= self.rank <= L.SWAG_RANK_MAX:
            raise BayesLMError("%s: n = %d, rank = %d" % (path, self.n, self.rank))
        return self

    def check(self, model_or_flat):
        """Refuses a posterior made for another model (PosteriorMismatch names the first manifest field that differs).  A model is
        compared by names, shapes and offsets; an engine.FlatBuffers, which knows no names, by shapes and offsets."""
        check_manifest(self.total, self.manifest, model_or_flat)

    def _slices(self, model):
        self.check(model)
        params, offsets, _ = flat_layout(model)
        return [(p, o, p.numel()) for p, o in zip(params, offsets)]

    def load_flat(self, model, flat_vector):
        """Writes a (P,) vector in this posterior's layout -- a row of draw(), or the mean -- into the parameters of ``model``."""
        with torch.no_grad():
            for p, o, n in self._slices(model):
                p.copy_(flat_vector[o:o + n].view_as(p))
        return model

    def mean_state_dict(self, model):
        """The SWA weights as an ordinary state_dict of ``model`` (host tensors, what --save writes): every trainable parameter
        from the mean, everything else as the model holds it."""
        if self.n < 1:
            raise BayesLMError("SwagPosterior: no iterate collected yet")
        where = {id(p): (o, n) for p, o, n in self._slices(model)}
        named = {name: p for name, p in model.named_parameters(remove_duplicate=False)}
        sd = {}
        for k, v in model.state_dict().items():
            p = named.get(k)
            if p is not None and id(p) in where:
                o, n = where[id(p)]
                sd[k] = self.mean[o:o + n].view_as(p).detach().cpu().clone()
            else:
                sd[k] = v.detach().cpu()
        return sd

    def draw(self, samples, seed, scale=0.5, diag=False, floor=1e-30, first=0, budget=DRAW_BYTES):
        """Samples ``first`` .. ``first + samples - 1`` -> (samples, P), ceil(samples / 8) launches of blm_swag_sample.  Sample j is a
        function of (posterior, seed, j, scale, diag, floor) alone, whatever else is drawn beside it."""
        S = int(samples)
        if S < 1 or int(first) < 0:
            raise BayesLMError("SwagPosterior.draw: samples = %d, first = %d" % (S, int(first)))
        if self.n < 1:
            raise BayesLMError("SwagPosterior.draw: no iterate collected yet")
        nbytes = 4 * S * self.total
        if nbytes > budget:
            raise BayesLMError("SwagPosterior.draw: %d samples of %d floats are %d bytes (%.2f GiB), beyond the budget of %d bytes "
                               "(%.2f GiB): draw fewer at a time" % (S, self.total, nbytes, nbytes / 2.0 ** 30, budget, budget / 2.0 ** 30))
        a, b, k = coefficients(scale, self.k_live, diag)
        out = torch.empty(S, self.total, device=self.mean.device, dtype=torch.float32)
        for j0 in range(0, S, L.SWAG_DRAWS_MAX):
            ids = list(range(int(first) + j0, int(first) + min(S, j0 + L.SWAG_DRAWS_MAX)))
            ops.swag_sample(out[j0:j0 + len(ids)], self.mean, self.m2, ids, seed, a, b, 1.0 / self.n, floor, dev=self.dev, k_live=k)
        return out

    def describe(self):
        """The ``swag`` block of a report"""
        return {"n": self.n, "rank": self.rank, "k_live": self.k_live, "total": self.total}


class SwagCollector:
    """When the training loop collects: from epoch ``start_epoch`` (1-based) on, at each epoch's end (``every`` 0) or after every
    ``every`` optimisation steps counted from that epoch's first one.  ``trainer``: an engine.Trainer (its flat buffer is read)."""

    def __init__(self, trainer, rank, start_epoch=1, every=0, manifest=None):
        if int(start_epoch) < 1 or int(every) < 0:
            raise BayesLMError("SwagCollector: start_epoch = %r (1-based), every = %r (>= 0)" % (start_epoch, every))
        if getattr(trainer, "world", 1) > 1:
            raise BayesLMError("SwagCollector: world size %d: data-parallel collection is not built" % trainer.world)
        self.flat = trainer.flat
        if manifest is None:
            manifest = manifest_of(trainer.model)
        self.posterior = SwagPosterior(self.flat.total, rank, self.flat.flat_param.device, manifest)
        self.start_epoch, self.every, self.steps = int(start_epoch), int(every), 0

    def active(self, epoch):
        return epoch >= self.start_epoch

    def _collect(self):
        return self.posterior.collect(self.flat.flat_param)

    def after_step(self, epoch):
        """-> n after a collection, else None"""
        if not self.active(epoch) or not self.every:
            return None
        self.steps += 1
        return self._collect() if self.steps % self.every == 0 else None

    def epoch_end(self, epoch):
        """-> n after a collection, else None"""
        return self._collect() if self.active(epoch) and not self.every else None
