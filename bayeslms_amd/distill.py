"""Distillation of the Monte-Carlo model average into a mean-weight student ("Bayesian dark knowledge").

A ``Teacher`` wraps a frozen model and hands out, batch by batch, the (T * B, V) log-probabilities a student is trained
against with ``ops.cross_entropy_soft`` / ``engine.Trainer.step(soft=(logq, weight))``: the log-softmax of the teacher at
mean weights, or -- ``mc_samples`` = S >= 2 -- log pbar, the log of the average of S Monte-Carlo weight samples' next-word
distributions, formed by one ``ops.linear_mc_logprobs`` launch without storing the S x M x V logits.  Sample s means what it
means everywhere else (``model.mc_sampling(model, seed, S)``, ``model.set_step(s)``): ONE model for the whole stream, so a
recurrent teacher carries S (h, c) sets from batch to batch.

``Teacher.topk(data, k)`` hands out the k best entries of those rows as ``ops.SparseTargets`` for ``ops.cross_entropy_soft_topk``
/ ``Trainer.step(soft=(SparseTargets, weight))``, and a ``TeacherCache`` keeps them on disk: the trainer walks the same windows
in the same order in every epoch and the teacher is frozen, so its rows are computed once.  What top-k does to the objective:
without ``renorm`` the soft term of a row is weighted by the mass Q < 1 its k entries hold and the tail of the teacher is
dropped; with ``renorm`` the target is the renormalised head (Q = 1).

Neither the teacher nor the cache knows a softmax temperature: the losses take one (``temperature=`` of the two ops, a third
entry of ``soft``), raise the rows handed out here to 1 / T and renormalise them, and a constant on a row cancels there -- so
one cache file serves every temperature.

A student is judged as every model is, by hard-label loss: ``python -m bayeslms_amd.evaluate`` on the student at mean weights,
on the teacher at mean weights and on the teacher with ``--mc-samples S`` gives perplexity and calibration error of all three.
"""
import hashlib
import json
import os

import numpy as np
import torch

from . import incremental, ops
from ._lib import TOPK_MAX
from .model import CarriedState, inference_decoder, mc_sampling, require_variational_sites

__all__ = ["Teacher", "TeacherCache", "CacheMismatch", "sha256_file", "sha256_tensor"]


class Teacher:
    """``Teacher(model, mc_samples=0, seed=1111)``; ``reset(columns)`` at the start of every walk over a stream (an epoch),
    then ``logprobs(data) -> (logq, h_q)`` per batch: ``logq`` (T * B, V) float32 log-probabilities (rows possibly padded to 4
    floats: a view), ``h_q`` (T * B,) the predictive entropy H[pbar] under Monte-Carlo, None at mean weights.

    Refused here, as engine.evaluate_report refuses them: mc_samples 1 or above 64; Monte-Carlo sampling of a model without a
    variational site or flagged for local reparameterisation; recurrent cells that redraw noise at every time step of a call;
    a model whose decoder cannot hand back its input rows.  The teacher's parameters get no gradient; its mode and noise
    (seed, step, auto_step) are left as they were found after every call."""

    def __init__(self, model, mc_samples=0, seed=1111):
        S = int(mc_samples)
        if S < 0 or S == 1 or S > 64:
            raise ops.BayesLMError("Teacher: mc_samples must be 0 (mean weights) or 2..64, got %d: one sample is neither the "
                                   "mean-weight model nor an average, and blm_linear_mc_logprobs takes at most 64 samples per "
                                   "launch" % S)
        self.dec = inference_decoder(model)
        if self.dec is None:
            raise ops.BayesLMError("Teacher: %s has no decoder that hands back its input rows" % type(model).__name__)
        self.recurrent = hasattr(model, "init_hidden")
        if S:
            require_variational_sites(model, S)  # nothing to sample / local reparameterisation: raises, naming the cause
            cell = incremental._redraws_per_time_step(model) if self.recurrent else None
            if cell:
                raise ops.BayesLMError("Teacher: mc_samples on %s: %s draws fresh noise at every time step of a call, so a sample "
                                       "is not one model over a stream" % (type(model).__name__, cell))
        self.model, self.S, self.seed = model, S, int(seed)
        self.vocab = self.dec.weight.shape[0]
        self.state = None if self.recurrent else CarriedState(model, 0)  # a stateless teacher carries nothing: no reset needed
        self._mc_dec = None

    def reset(self, columns):
        """Start a walk over a stream of ``columns`` batch columns: a recurrent teacher's state -- one (h, c) set, or one per
        sample -- starts from zero."""
        self.state = CarriedState(self.model, columns, max(self.S, 1))

    def _forward(self, data, slot=0):
        """Decoder input rows (T * B, K) of one pass; ``slot``: the sample whose carried state is used."""
        if self.state is None:
            raise ops.BayesLMError("Teacher.logprobs: call reset(columns) before the first batch of a recurrent teacher")
        x = self.state(data, slot)
        return x.reshape(-1, x.shape[-1])

    def logprobs(self, data):
        m, dec, V = self.model, self.dec, self.vocab
        was_training = m.training
        try:
            with torch.no_grad(), dec.inference(input_rows=True):
                if self.S == 0:
                    m.eval()
                    logits = ops.linear(self._forward(data), dec.weight, dec.bias)
                    rows = logits
                    if not logits.is_contiguous():  # an odd vocabulary's padded rows (ops.linear): normalised where they are
                        rows = logits.as_strided((logits.shape[0], logits.stride(0)), (logits.stride(0), 1))
                    ops.log_softmax_rows(rows, V, out=rows)
                    return logits, None
                with mc_sampling(m, self.seed, self.S):
                    if self._mc_dec is None:  # the vocabulary padded once: the teacher is frozen
                        self._mc_dec = ops.McDecoder(dec.weight, dec.bias)
                    xs = []
                    for s in range(self.S):
                        m.set_step(s)
                        xs.append(self._forward(data, s))
                    mc = ops.linear_mc_logprobs(torch.stack(xs), dec.weight, dec.bias, dec=self._mc_dec, stats=True)
                return mc.logp, mc.h_pred
        finally:
            m.train(was_training)

    def topk(self, data, k, renorm=False):
        """-> (ops.SparseTargets(ids (M, k) int32, logq (M, k) float32), kept (M,)): the k best entries of every row of
        ``logprobs(data)``, best first (ops.topk_rows on the V live columns, padded rows read in place), the values copied bit
        for bit, and the teacher mass ``kept`` = sum_j exp(logq_j) they hold.  ``renorm``: logq -= log kept, so the k entries sum
        to one.  1 <= k <= min(V, BLM_TOPK_MAX)."""
        k = int(k)
        if not 1 <= k <= min(self.vocab, TOPK_MAX):
            raise ops.BayesLMError("Teacher.topk: k = %d outside [1, min(V = %d, BLM_TOPK_MAX = %d)]" % (k, self.vocab, TOPK_MAX))
        logq, _ = self.logprobs(data)
        vals, ids = ops.topk_rows(logq, k)
        kept = vals.exp().sum(1)
        if renorm:
            vals = vals - kept.log()[:, None]
        return ops.SparseTargets(ids.to(torch.int32), vals), kept


def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for block in iter(lambda: f.read(1 << 20), b""):
            h.update(block)
    return h.hexdigest()


def sha256_tensor(t):
    """SHA-256 of an integer tensor's values as little-endian int64, row-major (the batchified training ids)."""
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy().astype("<i8")).tobytes()).hexdigest()


class CacheMismatch(ValueError):
    """An existing TeacherCache file was written for something else; ``field`` names the first header field that differs."""

    def __init__(self, path, field, found, wanted):
        super().__init__("teacher cache %s: field %r differs: the file has %r, this run has %r" % (path, field, found, wanted))
        self.field, self.found, self.wanted = field, found, wanted


class TeacherCache:
    """A teacher's top-k targets of one training walk in one file, read and written through numpy memory maps only (no GPU
    needed): a JSON header in a fixed block of HEADER_BYTES, then (rows - 1) * columns x K int32 ids, then as many float32
    log-probabilities.  Row r of the file is token r of the flattened walk: the batch that starts at row i of the batchified
    (rows, columns) training tensor has offset i * columns, and the last window is ragged.

    ``TeacherCache(path, fields)``: ``fields`` is a dict with exactly the keys FIELDS (``TeacherCache.describe`` builds it).  A
    file at ``path`` whose header differs in any of them raises CacheMismatch naming the field and both values; a file without
    the ``complete`` flag (an interrupted first epoch) or no file is (re)built from the start: ``complete`` is False, ``store``
    fills rows in any order, ``finish()`` flushes the rows and only then writes the flag.  A complete file is opened read-only
    and ``load(offset, rows, device)`` returns ops.SparseTargets through one pinned host copy and one non-blocking device copy."""

    VERSION = 1
    HEADER_BYTES = 4096
    FIELDS = ("version", "vocab", "k", "renorm", "seq_len", "rows", "columns", "data_sha256", "teacher_sha256", "teacher_flags",
              "mc_samples", "mc_seed")

    @classmethod
    def describe(cls, vocab, k, renorm, seq_len, rows, columns, data_sha256, teacher_sha256, teacher_flags, mc_samples, mc_seed):
        return {"version": cls.VERSION, "vocab": int(vocab), "k": int(k), "renorm": bool(renorm), "seq_len": int(seq_len),
                "rows": int(rows), "columns": int(columns), "data_sha256": str(data_sha256), "teacher_sha256": str(teacher_sha256),
                "teacher_flags": {str(a): b for a, b in sorted(dict(teacher_flags).items())}, "mc_samples": int(mc_samples),
                "mc_seed": int(mc_seed)}

    def __init__(self, path, fields):
        if set(fields) != set(self.FIELDS):
            raise ValueError("TeacherCache: fields %s given, %s expected" % (sorted(fields), sorted(self.FIELDS)))
        fields = json.loads(json.dumps(fields))  # as a header read back from disk compares: lists for tuples, str keys
        self.path, self.fields = path, fields
        self.n, self.k = (fields["rows"] - 1) * fields["columns"], fields["k"]
        if self.n < 1 or not 1 <= self.k <= TOPK_MAX:
            raise ValueError("TeacherCache: %d rows of %d targets: at least one row and 1 <= k <= %d expected" % (self.n, self.k, TOPK_MAX))
        self.complete = False
        found = self._read_header()
        if found is not None:
            for f in self.FIELDS:
                if found.get(f) != fields[f]:
                    raise CacheMismatch(path, f, found.get(f), fields[f])
            self.complete = bool(found.get("complete")) and os.path.getsize(path) == self._size()
        if not self.complete:
            with open(path, "wb") as f:  # from the start: a partial file's rows are not trusted
                f.write(self._header(False))
                f.truncate(self._size())
        self._map("r" if self.complete else "r+")

    def _size(self):
        return self.HEADER_BYTES + 8 * self.n * self.k

    def _header(self, complete):
        blob = json.dumps(dict(self.fields, complete=bool(complete)), sort_keys=True).encode()
        if len(blob) >= self.HEADER_BYTES:
            raise ValueError("TeacherCache: a header of %d bytes does not fit its %d-byte block" % (len(blob), self.HEADER_BYTES))
        return blob + b"\n" + b" " * (self.HEADER_BYTES - len(blob) - 1)

    def _read_header(self):
        """The header of the file at ``path`` as a dict; None if there is no file or no readable header (then it is rebuilt)."""
        try:
            with open(self.path, "rb") as f:
                head = json.loads(f.read(self.HEADER_BYTES).decode())
        except (OSError, ValueError):
            return None
        return head if isinstance(head, dict) else None

    def _map(self, mode):
        self.ids = np.memmap(self.path, dtype="<i4", mode=mode, offset=self.HEADER_BYTES, shape=(self.n, self.k))
        self.logq = np.memmap(self.path, dtype="<f4", mode=mode, offset=self.HEADER_BYTES + 4 * self.n * self.k, shape=(self.n, self.k))

    def _check(self, offset, rows):
        if offset < 0 or rows < 1 or offset + rows > self.n:
            raise IndexError("TeacherCache: rows %d .. %d of %d" % (offset, offset + rows, self.n))

    def store(self, offset, sparse):
        """Rows offset .. offset + M of the walk; any order, any tensors (device or host) of shape (M, k)."""
        if self.complete:
            raise ValueError("TeacherCache.store: %s is complete and open read-only" % self.path)
        ids, logq = sparse
        M = ids.shape[0]
        self._check(offset, M)
        if tuple(ids.shape) != (M, self.k) or tuple(logq.shape) != (M, self.k) or ids.dtype != torch.int32 or logq.dtype != torch.float32:
            raise ValueError("TeacherCache.store: (%d, %d) int32 ids and float32 logq expected" % (M, self.k))
        self.ids[offset:offset + M] = ids.detach().cpu().numpy()
        self.logq[offset:offset + M] = logq.detach().cpu().numpy()

    def finish(self):
        """Every row is stored: flush them, then -- last -- write the header with ``complete`` set, and reopen read-only."""
        if self.complete:
            return
        self.ids.flush()
        self.logq.flush()
        head = np.memmap(self.path, dtype=np.uint8, mode="r+", offset=0, shape=(self.HEADER_BYTES,))
        head[:] = np.frombuffer(self._header(True), dtype=np.uint8)
        head.flush()
        del head
        self.complete = True
        self._map("r")

    def load(self, offset, rows, device):
        """-> ops.SparseTargets of rows offset .. offset + rows on ``device``: one pinned host buffer (ids and logq side by side),
        one non-blocking copy."""
        self._check(offset, rows)
        pin = torch.device(device).type == "cuda"
        host = torch.empty(2, rows, self.k, dtype=torch.int32, pin_memory=pin)
        buf = host.numpy()
        buf[0] = self.ids[offset:offset + rows]
        buf[1] = self.logq[offset:offset + rows].view("<i4")
        both = host.to(device, non_blocking=True)
        return ops.SparseTargets(both[0], both[1].view(torch.float32))
