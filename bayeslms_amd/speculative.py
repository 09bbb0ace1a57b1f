"""Speculative sampling on the incremental path (Leviathan et al. 2023; Chen et al. 2023): a cheap draft proposes ``gamma`` words
per stream, the target scores all gamma + 1 positions in ONE chunk, and an accept / reject rule (blm_spec_accept: definitions in
include/bayeslm.h) keeps a prefix and draws one more word.  The emitted words are distributed exactly as if every one had been
drawn from the target.

    spec = SpeculativeLM(IncrementalLM(model, max_streams=16, max_len=400, mc_samples=8), gamma=4)   # draft: the same network at
    tokens, stats = spec.generate(ctx, words=100, streams=16, temperature=1.0, seed=1111)            # its mean weights
    spec = SpeculativeLM(target, IncrementalLM(student, max_streams=16, max_len=400), gamma=4)       # a distilled student drafts

A Bayesian model carries its own draft: with ``draft=None`` (the target has mc_samples >= 2) a mean-weight IncrementalLM is built
over the same model.  The two are used strictly one after the other, and step leaves eval mode behind, as it always does.

One round, per stream with s = prompt + words so far (the target has consumed s[:-1]):
    gamma draft steps, each followed by ops.sample_rows at the temperature on the draft's row; the rows are kept in one
        preallocated (gamma, N, V) buffer
    one target step(all_positions=True) over [s[-1], x_0 ... x_{gamma-1}]: S passes over gamma + 1 rows instead of S per word
    one ops.spec_accept
    ONE device-to-host copy of (n_acc, token): the host mirrors of the lengths need them, and THIS IS THE LOOP'S ONE
        SYNCHRONISATION PER ROUND
    both states are taken back to what was kept.
The draft has consumed one word fewer than the target: it never sees x_{gamma-1}.  After a fully accepted round a stream therefore
feeds its draft two words (x_{gamma-1}, then the bonus word) through the ragged n_new of step; the other streams feed one.
Streams advance unevenly; a stream that has its ``words`` is frozen (it takes no part in the draft's first step, what it runs
afterwards is taken back in full) and the loop ends when every stream has them, the output cut there.  No stream ever holds more
than len(ctx) + words + gamma tokens, which is what max_len of both sides must allow (checked before any launch).

An LSTM on either side cannot take tokens back (IncrementalLM.truncate refuses): its (h, c) buffer, which is small, is copied
before the words that may be rejected, copied back after the decision, and the kept words are fed again in one ragged step
(skipped when nobody keeps any).  Correct by construction; its speed is unmeasured.

Philox stream ids, disjoint so that the verification never reuses the noise a drafted word was drawn with (the independence
rule of blm_spec_accept): plain generate keeps 0 (STREAM_PLAIN), draft draws use 1 (STREAM_DRAFT) with step = round * gamma + t, the
verify call uses 2 (STREAM_VERIFY) with step = round.

Not built: top-k / top-p filtering (the verification would need the FILTERED target as p) and return_uncertainty."""
from typing import NamedTuple

import numpy as np
import torch

from . import ops
from ._lib import BayesLMError
from .incremental import IncrementalLM, _upload

# the three Philox stream ids of generation: named here and nowhere else
STREAM_PLAIN, STREAM_DRAFT, STREAM_VERIFY = 0, 1, 2
GAMMA_MAX = 16


class SpecStats(NamedTuple):
    rounds: int         # draft / verify rounds
    drafted: int        # words proposed to streams that still wanted words (gamma per such stream and round)
    accepted: int       # of those, the ones kept; every such stream and round emits one more word behind them
    target_chunks: int  # target steps of the loop: one chunk per round, plus an LSTM target's re-feeds

    @property
    def acceptance_rate(self):
        return self.accepted / self.drafted if self.drafted else 0.0

    def words_per_chunk(self, gamma):
        """words emitted per stream and verification chunk, 1 + gamma * acceptance_rate (plain generation: 1)"""
        return 1.0 + gamma * self.acceptance_rate


class SpeculativeLM:
    """Speculative sampling over two IncrementalLMs (module docstring)."""

    def __init__(self, target, draft=None, gamma=4):
        self.gamma = int(gamma)
        if not 1 <= self.gamma <= GAMMA_MAX:
            raise BayesLMError("SpeculativeLM: gamma = %d outside 1..%d" % (self.gamma, GAMMA_MAX))
        if draft is None:
            if target.mc_samples < 2:
                raise BayesLMError("SpeculativeLM: draft=None drafts at the target's own mean weights, which needs a target with "
                                   "mc_samples >= 2 (got %d)" % target.mc_samples)
            draft = IncrementalLM(target.model, max_streams=target.max_streams, max_len=target.max_len)
        if draft.mc_samples:
            raise BayesLMError("SpeculativeLM: the draft has mc_samples = %d; it is meant to be cheap (mean weights)" % draft.mc_samples)
        if draft.vocab != target.vocab:
            raise BayesLMError("SpeculativeLM: the draft's vocabulary (%d words) is not the target's (%d)" % (draft.vocab, target.vocab))
        self.target, self.draft = target, draft
        self.device = target.device

    # ---------------------------------------------------------------- the device side, one method each
    def _put(self, a, dtype):
        """host array -> device tensor without a synchronisation"""
        if self.device.type == "cuda":
            return _upload(a, self.device, dtype)
        return torch.as_tensor(np.ascontiguousarray(a)).to(dtype)

    def _sample(self, rows, temperature, seed, step):
        return ops.sample_rows(rows, temperature, seed, STREAM_DRAFT, step)

    def _verify(self, logp, logq, drafted, temperature, seed, step):
        return ops.spec_accept(logp, logq, drafted, temperature, seed, STREAM_VERIFY, step)

    @staticmethod
    def _copy_state(lm, st):
        """an LSTM's (h, c) before words that may be rejected (None for a Transformer, which truncates)"""
        return None if lm.kind == "transformer" else (st._live(lm).clone(), list(st.lengths))

    @staticmethod
    def _take_back(lm, st, saved, base, keep, ids):
        """``st`` back to ``base`` tokens + the first keep[j] rows of ``ids`` (Tq, N), the words fed since -> steps run (0 / 1)"""
        if lm.kind == "transformer":
            lm.truncate(st, [b + int(k) for b, k in zip(base, keep)])
            return 0
        buf, lengths = saved
        st._live(lm).copy_(buf)
        st.lengths = list(lengths)
        if ids is None or int(keep.max()) == 0:
            return 0
        lm.step(st, ids, n_new=keep)
        return 1

    # ---------------------------------------------------------------- the loop
    def generate(self, ctx, words, streams=1, temperature=1.0, seed=1111):
        """``streams`` continuations of the word ids ``ctx`` (at least one: the sentence start), ``words`` new words each
        -> (list of ``streams`` lists of word ids, SpecStats).  temperature 0: greedy, the output of plain greedy generation."""
        G, N, W, tau = self.gamma, int(streams), int(words), float(temperature)
        ctx = [int(c) for c in ctx]
        L0 = len(ctx)
        tg, dr = self.target, self.draft
        if L0 < 1 or W < 0 or not tau >= 0.0:
            raise BayesLMError("SpeculativeLM.generate: a context of at least one word, words >= 0 and temperature >= 0 expected")
        if not 1 <= N <= min(tg.max_streams, dr.max_streams):
            raise BayesLMError("SpeculativeLM.generate: %d streams, max_streams is %d (target) and %d (draft)"
                               % (N, tg.max_streams, dr.max_streams))
        need = L0 + W + G  # gamma + 1 rows beyond the len(ctx) + words - 1 tokens a finished stream holds
        if min(tg.max_len, dr.max_len) < need:
            raise BayesLMError("SpeculativeLM.generate: %d context + %d new words + gamma = %d need max_len >= %d on both sides "
                               "(target %d, draft %d)" % (L0, W, G, need, tg.max_len, dr.max_len))
        if any(not 0 <= c < tg.vocab for c in ctx):
            raise BayesLMError("SpeculativeLM.generate: a context word lies outside the vocabulary")
        if W == 0:
            return [[] for _ in range(N)], SpecStats(0, 0, 0, 0)
        tst, dst = tg.start(N), dr.start(N)
        if L0 > 1:  # both sides consume all but the last word; the loop feeds that one
            head = self._put(np.repeat(np.asarray(ctx[:-1], np.int64)[:, None], N, 1), torch.int64)
            tg.step(tst, head)
            dr.step(dst, head)
        last_h = np.full(N, ctx[-1], np.int64)        # s[-1] of every stream
        emitted = np.zeros(N, np.int64)               # words each stream has
        pending = np.zeros(N, bool)                   # the draft still owes x_{gamma-1} of the round before
        qbuf = torch.empty(G, N, tg.vocab, device=self.device, dtype=torch.float32)
        xbuf = torch.zeros(G, N, device=self.device, dtype=torch.int64)
        greedy = tau == 0.0
        rounds = drafted = accepted = chunks = 0
        trace = []  # per round: (drafted ids on the device, n_acc, token, the streams that took part)
        while True:
            active = emitted < W
            if not active.any():
                break
            last_d = self._put(last_h, torch.int64)
            # ---- draft: the first step feeds s[-1] (behind x_{gamma-1} where the round before accepted everything)
            if pending.any():
                owed = torch.where(self._put(pending, torch.bool), xbuf[G - 1], last_d)
                ids0, n0 = torch.stack([owed, last_d]), np.where(pending, 2, 1) * active
            else:
                ids0, n0 = last_d.view(1, N), active.astype(np.int64)
            qbuf[0] = dr.step(dst, ids0, n_new=None if n0.min() == ids0.shape[0] else n0)
            d_saved, d_base = self._copy_state(dr, dst), list(dst.lengths)
            for t in range(G):
                if t:
                    qbuf[t] = dr.step(dst, xbuf[t - 1])
                xbuf[t] = self._sample(qbuf[t], tau, seed, rounds * G + t)
            # ---- target: one chunk over [s[-1], x_0 ... x_{gamma-1}]
            t_saved, t_base = self._copy_state(tg, tst), list(tst.lengths)
            chunk = torch.cat([last_d.view(1, N), xbuf])
            logp = tg.step(tst, chunk, all_positions=True)
            chunks += 1
            r = self._verify(logp, None if greedy else qbuf, xbuf, tau, seed, rounds)
            both = torch.stack([r.n_acc.to(torch.int64), r.token]).cpu().numpy()  # the round's one synchronisation
            n_acc, token = both[0], both[1]
            trace.append((xbuf.clone(), n_acc, token, active))
            # ---- the host side: what every stream keeps
            left = W - emitted                                      # words still wanted (<= 0: frozen)
            ending = active & (n_acc + 1 >= left)
            going = active & ~ending
            keep_t = np.where(going, n_acc + 1, np.where(ending, left, 0)).astype(np.int64)   # of [s[-1], x_0 ...]
            keep_d = np.where(going, np.minimum(n_acc, G - 1), 0).astype(np.int64)             # of [x_0 ... x_{gamma-2}]
            pending = going & (n_acc == G)
            emitted = emitted + np.where(active, n_acc + 1, 0)
            last_h = np.where(going, token, last_h)
            rounds += 1
            drafted += G * int(active.sum())
            accepted += int(n_acc[active].sum())
            if not (emitted < W).any():
                break
            chunks += self._take_back(tg, tst, t_saved, t_base, keep_t, chunk)
            self._take_back(dr, dst, d_saved, d_base, keep_d, xbuf[:G - 1] if G > 1 else None)
        out = [[] for _ in range(N)]
        if trace:
            xs = torch.stack([t[0] for t in trace]).cpu().numpy()  # one copy of every round's drafted ids
            for rd, (_, n_acc, token, active) in enumerate(trace):
                for j in np.nonzero(active)[0]:
                    out[j].extend(int(v) for v in xs[rd, :n_acc[j], j])
                    out[j].append(int(token[j]))
        return [o[:W] for o in out], SpecStats(rounds, drafted, accepted, chunks)
