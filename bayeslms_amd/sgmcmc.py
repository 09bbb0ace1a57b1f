"""Stochastic-gradient MCMC over ALL weights of a model without variational sites, and banks of complete weight vectors: the
samples of such a chain, or the members of a deep ensemble (Lakshminarayanan, Pritzel, Blundell, NeurIPS 2017).

    sampler = Sampler("psgld", lr=1e-3, n_tokens=N)          # or "sgld"; schedule=CyclicalSchedule(...) for cyclical SG-MCMC
    trainer.set_sampler(sampler)                             # Trainer.step now ends in blm_sgmcmc_update, not in clip + SGD
    bank = SampleBank(trainer.flat.total, swag.manifest_of(model), capacity=16)
    bank.add(trainer.flat.flat_param, {"kind": "psgld", "epoch": e, "step": trainer.step_no, "rate": sampler.last_lr})
    bank.save("bank.pt")
    ...
    engine.evaluate_samples(model, source, seq_len, SampleBank.load("bank.pt"))
    engine.evaluate_samples(model, source, seq_len, SampleBank.from_checkpoints(model, ["a.pt", "b.pt", "c.pt"]))

The rules are stochastic-gradient Langevin dynamics (Welling and Teh, ICML 2011) and its RMSprop-preconditioned form (Li, Chen,
Carlson, Carin, AAAI 2016), which Gan, Li, Chen, Pu, Su and Carin (ACL 2017) ran on LSTM language models; the cyclical schedule is
Zhang, Li, Zhang, Chen, Wilson (ICLR 2020), eq. 1.  The update itself is one kernel over the flat buffer: include/bayeslm.h,
csrc/sgmcmc.hip.

Scaling.  The step's loss is the MEAN negative log-likelihood over its tokens.  With N the number of target tokens one epoch of
the training text walks, the potential is U = N * mean NLL + tau / 2 |theta|^2 (a Gaussian prior of precision tau), and a Langevin
step of size eps on U, theta <- theta - eps / 2 grad U + N(0, eps T), reads on the mean loss

    rate lr = eps N / 2,   weight_decay = tau / N,   sigma = sqrt(2 lr T / N)

(sigma formed in double and rounded to float32 once).  T is the temperature of the chain: 1 samples the posterior, 0 is plain
SGD with weight decay, and values below 1 are the "cold posteriors" many report to work better.

What biases the chain.  The gradient is clipped to the trainer's global norm before the step, as in every training run of this
package; a clipped step is not a Langevin step, so where the clip is active the stationary distribution is not the posterior.
The preconditioned rule drops the Gamma(theta) term, as Li et al.'s practical algorithm does.  No Metropolis correction, as in
all SG-MCMC.

Defaults.  prior_precision = 1, alpha = 0.99 and damping = 1e-5 are the customary values (Li et al. 2016 for the last two).
Nobody has measured them here, on any model."""
import math

import torch

from . import ops
from . import swag
from ._lib import BayesLMError

FORMAT = "bayeslms_amd.samples/1"
CAPACITY_MAX = 64  # BLM_SWAG_SAMPLES_MAX: the most weight vectors one evaluation averages
RULES = ("sgld", "psgld")


class CyclicalSchedule:
    """Zhang et al. 2020, eq. 1 (host only): K = ``total_steps`` sampling steps in M = ``cycles`` cycles of L = ceil(K / M) steps.
    At step k (1-based), r(k) = mod(k - 1, L) / L, the rate is lr0 / 2 (cos(pi r) + 1); while r < ``explore`` the step is an
    exploration step (no noise, nothing collected), from there on a sampling step (noise on, samples collected).
    ``cycles`` = 0: the constant rate lr0 with noise throughout."""

    def __init__(self, total_steps, cycles, lr0, explore=0.8):
        K, M, lr0, explore = int(total_steps), int(cycles), float(lr0), float(explore)
        if K < 1 or M < 0 or M > K:
            raise BayesLMError("CyclicalSchedule: total_steps = %d, cycles = %d (0 <= cycles <= total_steps, total_steps >= 1)" % (K, M))
        if not (math.isfinite(lr0) and lr0 > 0.0):
            raise BayesLMError("CyclicalSchedule: lr0 = %r is not a positive finite number" % lr0)
        if not 0.0 <= explore < 1.0:
            raise BayesLMError("CyclicalSchedule: explore = %r outside [0, 1)" % explore)
        self.total_steps, self.cycles, self.lr0, self.explore = K, M, lr0, explore
        self.length = -(-K // M) if M else 0

    def r(self, k):
        """Position of step k (1-based) inside its cycle, in [0, 1)"""
        if int(k) < 1:
            raise BayesLMError("CyclicalSchedule: step %d (steps count from 1)" % int(k))
        return ((int(k) - 1) % self.length) / float(self.length) if self.cycles else 0.0

    def rate(self, k):
        return self.lr0 * 0.5 * (math.cos(math.pi * self.r(k)) + 1.0) if self.cycles else self.lr0

    def sampling(self, k):
        return self.r(k) >= self.explore if self.cycles else True

    def settings(self):
        return {"total_steps": self.total_steps, "cycles": self.cycles, "lr0": self.lr0, "explore": self.explore}


class Sampler:
    """What Trainer.step runs in place of clip + SGD once Trainer.set_sampler has it.  ``lr`` is the rate on the MEAN loss (eps N / 2
    of the module docstring); with a ``schedule`` (CyclicalSchedule) the schedule's rate takes its place and its exploration
    steps run without noise.  ``prior_precision`` tau, ``alpha`` and ``damping`` default to customary values that are unmeasured
    here."""

    def __init__(self, rule, lr, n_tokens, temperature=1.0, prior_precision=1.0, alpha=0.99, damping=1e-5, seed=1111, schedule=None):
        if rule not in RULES:
            raise BayesLMError("Sampler: rule %r is not one of %s" % (rule, ", ".join(RULES)))
        lr, N, T, tau = float(lr), int(n_tokens), float(temperature), float(prior_precision)
        if not (math.isfinite(lr) and lr > 0.0):
            raise BayesLMError("Sampler: lr = %r is not a positive finite number" % lr)
        if N < 1:
            raise BayesLMError("Sampler: n_tokens = %d: the number of target tokens of one epoch, at least 1" % N)
        if not (math.isfinite(T) and T >= 0.0):
            raise BayesLMError("Sampler: temperature = %r is not a finite number >= 0" % T)
        if not (math.isfinite(tau) and tau >= 0.0):
            raise BayesLMError("Sampler: prior_precision = %r is not a finite number >= 0" % tau)
        if not (0.0 <= float(alpha) < 1.0 and float(damping) > 0.0 and math.isfinite(float(damping))):
            raise BayesLMError("Sampler: alpha = %r must lie in [0, 1) and damping = %r be positive and finite" % (alpha, damping))
        self.rule, self.lr, self.n_tokens, self.temperature, self.prior_precision = rule, lr, N, T, tau
        self.alpha, self.damping, self.seed, self.schedule = float(alpha), float(damping), int(seed), schedule
        self.k = 0                 # sampler steps taken
        self.last_lr = None        # the rate, sigma and kind (sampling or exploration) of the last step taken
        self.last_sigma = None
        self.last_sampling = False

    @property
    def weight_decay(self):
        """tau / N: the prior's share of the gradient of the mean loss"""
        return self.prior_precision / self.n_tokens

    def sigma(self, lr):
        """float32(sqrt(2 lr T / N)), formed in double"""
        return float(torch.tensor(math.sqrt(2.0 * float(lr) * self.temperature / self.n_tokens), dtype=torch.float64).float())

    def plan(self, k):
        """-> (rate, sigma, sampling) of sampler step k (1-based)"""
        if self.schedule is None:
            lr, sampling = self.lr, True
        else:
            lr, sampling = self.schedule.rate(k), self.schedule.sampling(k)
        return lr, (self.sigma(lr) if sampling else 0.0), sampling

    def begin(self, trainer):
        """Trainer.set_sampler calls this: refuses what cannot be sampled and zeroes the second moment (psgld keeps it in the
        trainer's momentum buffer; momentum itself is not used while sampling)."""
        if getattr(trainer, "world", 1) > 1:
            raise BayesLMError("Sampler: world size %d: data-parallel sampling is not built" % trainer.world)
        site = variational_site(trainer.model)
        if site is not None:
            raise BayesLMError("Sampler: %s is a variational site: the model already carries a posterior over these weights, and "
                               "two posteriors over the same weights are not built" % site)
        if trainer.weight_decay:
            raise BayesLMError("Sampler: the trainer's weight_decay = %r: under a sampler the prior (prior_precision / n_tokens) is "
                               "the weight decay" % trainer.weight_decay)
        if self.rule == "psgld":
            trainer.flat.flat_mom.zero_()
        self.k = 0

    def update(self, trainer):
        """blm_sqnorm_multi as ops.clip_sgd runs it, then blm_sgmcmc_update over the flat buffer, noise of step trainer.step_no"""
        self.k += 1
        lr, sigma, sampling = self.plan(self.k)
        flat = trainer.flat
        sq = ops.sqnorm(trainer.table)
        ops.sgmcmc_update(flat.flat_param, flat.flat_grad, sq, trainer.clip, lr, sigma, self.seed, trainer.step_no,
                          v=flat.flat_mom if self.rule == "psgld" else None, grad_scale=1.0 / trainer.world,
                          weight_decay=self.weight_decay, alpha=self.alpha, damping=self.damping)
        self.last_lr, self.last_sigma, self.last_sampling = lr, sigma, sampling

    def settings(self):
        """What a bank records of the chain that filled it"""
        return {"rule": self.rule, "lr": self.lr, "n_tokens": self.n_tokens, "temperature": self.temperature,
                "prior_precision": self.prior_precision, "alpha": self.alpha, "damping": self.damping, "seed": self.seed,
                "schedule": None if self.schedule is None else self.schedule.settings()}


def variational_site(model):
    """The name of the first parameter of ``model`` that is a log standard deviation of a variational site, or None"""
    for name, _ in model.named_parameters():
        if "lgstd" in name:
            return name
    return None


def flat_of(model):
    """The trainable parameters of ``model`` as one HOST vector in the flat layout (swag.flat_layout), padding floats zero"""
    params, offsets, total = swag.flat_layout(model)
    out = torch.zeros(total, dtype=torch.float32)
    for p, o in zip(params, offsets):
        out[o:o + p.numel()].copy_(p.detach().reshape(-1))
    return out


class SampleBank:
    """Up to ``capacity`` (2..64) complete weight vectors of ``total`` floats in the flat layout of engine.FlatBuffers
    (``manifest``: swag.manifest_of(model)), held on the HOST; once full, the latest ``capacity`` are kept.  Each vector carries a
    meta dict (kind, epoch, step, rate); ``sampler``: the settings of the chain that filled the bank (Sampler.settings), or None."""

    def __init__(self, total, manifest=None, capacity=16, sampler=None):
        total, capacity = int(total), int(capacity)
        if total < 1:
            raise BayesLMError("SampleBank: total = %d" % total)
        if not 2 <= capacity <= CAPACITY_MAX:
            raise BayesLMError("SampleBank: capacity = %d outside 2..%d" % (capacity, CAPACITY_MAX))
        if manifest is not None and manifest["total"] != total:
            raise BayesLMError("SampleBank: the manifest describes %d floats, total = %d" % (manifest["total"], total))
        self.total, self.manifest, self.capacity, self.sampler = total, manifest, capacity, sampler
        self.seen = 0     # vectors ever added
        self.rows = []    # the latest min(seen, capacity) vectors, oldest first
        self.meta = []

    def __len__(self):
        return len(self.rows)

    def _padding(self):
        """[(start, end)] of the floats that belong to no tensor"""
        m = self.manifest
        if m is None:
            return []
        ends = list(m["offsets"][1:]) + [m["total"]]
        gaps = []
        for o, shape, e in zip(m["offsets"], m["shapes"], ends):
            n = 1
            for d in shape:
                n *= int(d)
            if o + n < e:
                gaps.append((o + n, e))
        return gaps

    def add(self, flat_param, meta=None):
        """Copies one weight vector out (device or host) -> the number of vectors held.  The layout's padding floats are stored as
        zero: the update kernel writes noise there, and they belong to no tensor."""
        if not torch.is_tensor(flat_param) or flat_param.dim() != 1 or flat_param.numel() != self.total or flat_param.dtype != torch.float32:
            raise BayesLMError("SampleBank.add: a float32 vector of %d floats expected, got %s %s" % (
                self.total, getattr(flat_param, "dtype", type(flat_param).__name__), tuple(getattr(flat_param, "shape", ()))))
        row = flat_param.detach().to("cpu", copy=True).contiguous()
        for a, b in self._padding():
            row[a:b] = 0.0
        meta = dict(meta or {})
        entry = {k: meta.get(k) for k in ("kind", "epoch", "step", "rate")}
        self.rows.append(row)
        self.meta.append(entry)
        if len(self.rows) > self.capacity:
            del self.rows[0], self.meta[0]
        self.seen += 1
        return len(self.rows)

    def matrix(self, latest=None):
        """The latest ``latest`` vectors (default all) -> (S, total) float32 on the host, oldest first"""
        S = len(self.rows) if latest is None else int(latest)
        if not 1 <= S <= len(self.rows):
            raise BayesLMError("SampleBank: %d of %d vectors asked for" % (S, len(self.rows)))
        return torch.stack(self.rows[len(self.rows) - S:])

    def latest(self, count):
        """A bank of the latest ``count`` vectors (they are shared, not copied)"""
        S = int(count)
        if not 1 <= S <= len(self.rows):
            raise BayesLMError("SampleBank: %d of %d vectors asked for" % (S, len(self.rows)))
        b = SampleBank(self.total, self.manifest, self.capacity, self.sampler)
        b.seen, b.rows, b.meta = self.seen, self.rows[len(self.rows) - S:], self.meta[len(self.meta) - S:]
        return b

    def to_device(self, device, latest=None):
        """The latest ``latest`` vectors (default all) -> (S, total) float32 on ``device``, copied row by row: no second copy of
        the bank on the host"""
        S = len(self.rows) if latest is None else int(latest)
        if not 1 <= S <= len(self.rows):
            raise BayesLMError("SampleBank: %d of %d vectors asked for" % (S, len(self.rows)))
        out = torch.empty(S, self.total, device=device, dtype=torch.float32)
        for s, row in enumerate(self.rows[len(self.rows) - S:]):
            out[s].copy_(row)
        return out

    def state(self):
        """What save writes; ``vectors`` is the list of the rows themselves (no stacked copy: 64 vectors of a large model are GBs)"""
        return {"format": FORMAT, "total": self.total, "capacity": self.capacity, "seen": self.seen, "manifest": self.manifest,
                "meta": [dict(m) for m in self.meta], "sampler": self.sampler, "vectors": list(self.rows)}

    def save(self, path):
        if not self.rows:
            raise BayesLMError("SampleBank.save: no vector held: nothing to write to %s" % path)
        with open(path, "wb") as f:
            torch.save(self.state(), f)

    @classmethod
    def load(cls, path):
        d = torch.load(path, map_location="cpu")
        if not isinstance(d, dict) or d.get("format") != FORMAT:
            raise BayesLMError("%s is not a sample bank of this package (format %r expected)" % (path, FORMAT))
        self = cls(int(d["total"]), d["manifest"], int(d["capacity"]), d.get("sampler"))
        v, meta = d["vectors"], d["meta"]
        if not isinstance(v, (list, tuple)) or not 1 <= len(v) <= self.capacity or len(meta) != len(v) or not all(
                torch.is_tensor(r) and tuple(r.shape) == (self.total,) and r.dtype == torch.float32 for r in v):
            raise BayesLMError("%s: vectors must be 1..%d float32 tensors of %d floats, one meta entry each (%d entries)" % (
                path, self.capacity, self.total, len(meta)))
        self.rows, self.meta, self.seen = list(v), [dict(m) for m in meta], int(d["seen"])  # the loaded tensors themselves
        if self.seen < len(self.rows):
            raise BayesLMError("%s: seen = %d below the %d vectors held" % (path, self.seen, len(self.rows)))
        return self

    def check(self, model_or_flat):
        """Refuses a bank made for another model: swag.PosteriorMismatch names the first manifest field that differs"""
        swag.check_manifest(self.total, self.manifest, model_or_flat, "sample bank", "bank")

    def kind(self):
        kinds = sorted({str(m.get("kind")) for m in self.meta})
        return kinds[0] if len(kinds) == 1 else "mixed"

    def describe(self):
        """The ``samples`` block of a report"""
        return {"kind": self.kind(), "n": len(self.rows), "seen": self.seen, "capacity": self.capacity, "total": self.total,
                "meta": [dict(m) for m in self.meta], "sampler": self.sampler}

    @classmethod
    def from_checkpoints(cls, model, paths):
        """A deep ensemble as a bank: each ``model.pt`` of ``paths`` (2..64 state_dicts of this architecture) is loaded into
        ``model`` in turn and its flat vector copied out (kind "checkpoint").  The model is left with the weights it had.  A
        checkpoint whose keys or shapes differ from the model's is refused, naming the key."""
        paths = list(paths)
        if not 2 <= len(paths) <= CAPACITY_MAX:
            raise BayesLMError("SampleBank.from_checkpoints: %d checkpoints: an ensemble has 2..%d members" % (len(paths), CAPACITY_MAX))
        own = model.state_dict()
        kept = {k: v.detach().clone() for k, v in own.items()}
        bank = cls(swag.flat_layout(model)[2], swag.manifest_of(model), max(2, len(paths)))
        try:
            for path in paths:
                sd = torch.load(path, map_location="cpu")
                if not isinstance(sd, dict):
                    raise BayesLMError("%s is not a state_dict" % path)
                for k in own:
                    if k not in sd:
                        raise BayesLMError("%s: key %r of the model is missing from the checkpoint" % (path, k))
                for k, v in sd.items():
                    if k not in own:
                        raise BayesLMError("%s: key %r of the checkpoint is not in the model" % (path, k))
                    if not torch.is_tensor(v) or tuple(v.shape) != tuple(own[k].shape):
                        raise BayesLMError("%s: key %r has shape %s, the model's has %s" % (
                            path, k, tuple(getattr(v, "shape", ())), tuple(own[k].shape)))
                with torch.no_grad():
                    for k, v in sd.items():
                        own[k].copy_(v)
                bank.add(flat_of(model), {"kind": "checkpoint", "epoch": None, "step": None, "rate": None})
        finally:
            with torch.no_grad():
                for k, v in kept.items():
                    own[k].copy_(v)
        return bank


class SampleCollector:
    """When the training loop adds to the bank: swag.SwagCollector's surface (``active``, ``after_step``, ``epoch_end``).  From
    epoch ``start_epoch`` (1-based) on, at each epoch's end (``every`` 0) or after every ``every`` optimisation steps counted from
    that epoch's first one -- and only where the trainer's sampler says the step was a sampling step (a cyclical schedule's
    exploration steps add nothing)."""

    def __init__(self, trainer, bank, start_epoch=1, every=0):
        if int(start_epoch) < 1 or int(every) < 0:
            raise BayesLMError("SampleCollector: start_epoch = %r (1-based), every = %r (>= 0)" % (start_epoch, every))
        if getattr(trainer, "world", 1) > 1:
            raise BayesLMError("SampleCollector: world size %d: data-parallel collection is not built" % trainer.world)
        bank.check(trainer.flat)
        self.trainer, self.bank = trainer, bank
        self.start_epoch, self.every, self.steps = int(start_epoch), int(every), 0

    def active(self, epoch):
        return epoch >= self.start_epoch

    def _collect(self, epoch):
        s = self.trainer.sampler
        if s is None or not s.last_sampling:
            return None
        return self.bank.add(self.trainer.flat.flat_param, {"kind": s.rule, "epoch": int(epoch), "step": int(self.trainer.step_no),
                                                            "rate": s.last_lr})

    def after_step(self, epoch):
        """-> vectors held after a collection, else None"""
        if not self.active(epoch) or not self.every:
            return None
        self.steps += 1
        return self._collect(epoch) if self.steps % self.every == 0 else None

    def epoch_end(self, epoch):
        """-> vectors held after a collection, else None"""
        return self._collect(epoch) if self.active(epoch) and not self.every else None
