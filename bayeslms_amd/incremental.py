"""Incremental next-word scoring and generation: the distribution of the word after each of N word histories without running
the histories through the model again.

    lm = IncrementalLM(model, max_streams=64, max_len=1024)   # model.eval(), on the GPU
    st = lm.start(n)                                           # n empty streams
    lp = lm.step(st, ids)                     # ids (Tq, n) or (n,) int64 -> (n, V) log-probs of the word after each stream
    lp = lm.step(st, ids, n_new=k)            # ragged chunk: stream j takes its first k[j] rows (prompts of different lengths;
                                              # 0: the stream takes no part and its row is NaN)
    lp = lm.step(st, ids, all_positions=True) # (Tq, n, V) (NaN on the padding rows of a ragged chunk)
    nll = lm.step(st, ids, targets=t)         # NLL of the given next words, no logits stored
    st = lm.reorder(st, idx)                  # beam prune / fork: new stream j continues old stream idx[j]; `st` is consumed
    st.lengths                                # host mirror of the per-stream lengths
    lm.truncate(st, lengths)                  # take tokens back out: stream j keeps its first lengths[j] (Transformer only; what
                                              # speculative sampling, bayeslms_amd/speculative.py, does with rejected drafts)
    vals, ids = lm.step_topk(st, ids, k=8)    # the 8 best next words of each stream, best first (blm_topk_rows)
    st = lm.reorder_device(st, idx)           # the same gather with a DEVICE index and no copy to the host (equal lengths promised)
    nbest = lm.beam_search([[bos, w1, w2]], beam=8, max_words=30, eos=bos)   # -> [[BeamHypothesis(tokens, score, length), ...]]
    nbest = lm.beam_search_pool([[bos, w1]], beam=8, max_words=30, eos=bos, pool=20, length_penalty=0.8)   # finished hypotheses
                                              # leave the beam for a pool ranked by score / length ** a -> [[PooledHypothesis, ...]]

    lm = IncrementalLM(model, max_streams=64, max_len=1024, mc_samples=8, seed=1111)   # the model average over 8 weight samples
    lp = lm.step(st, ids)                                   # log pbar, the distribution the n-best scorer's --mc-samples scores with
    lp, unc = lm.step(st, ids, return_uncertainty=True)     # + McUncertainty(h_pred, mi, nll_s) per returned row

Transformers (TransformerModel, BayesTransformerModel none / EMB / FFN / MHA, GaussTransformerModel, VTransformerModel) keep a
key/value cache: the model's own forward runs under ops.cached_tokens, where every attention core appends the chunk's K / V rows
and attends the cache (blm_kv_append + blm_attn_decode) and the positional encoding starts at each stream's length
(blm_embed_at).  The decoder product runs on the returned rows only.  The LSTM families carry (h, c) through their ordinary
fused step kernels.  reorder gathers either state in one launch (blm_kv_gather).

Every length is known on the host (each append is), so a step checks its arguments before any launch and needs no
host-device synchronisation of its own; the lengths the kernels read stay on the device.  Eval mode is deterministic in every
family (mean weights; no dropout), which is what makes a cached continuation equal to the full forward over the history.

mc_samples = S > 0 (default 0: everything above, unchanged): every stream is S streams, one per Monte-Carlo weight sample.  Sample s
is the model in the n-best scorer's sampling state (train(), dropout off, the GPNN sample flags raised, set_seed(seed),
set_step(s)): its weights are a pure function of (seed, s), so they are the SAME at every step of a stream and a cached
continuation still equals the full forward over the history.  step runs the S passes one after the other, each on its own slice
of the state, and one decoder launch over all S of them returns log pbar = log mean_s p_s (blm_linear_mc_logprobs; many rows
of a wide model compose it from the logits instead, _MC_FUSED_MAX_ROWS_K), or with targets their NLL under pbar
(blm_linear_mc_stats).  The sampling state is entered and left inside step: the model is in eval
mode whenever the caller holds it.  Not covered: two-model interpolation, the architecture-search super-nets, and under
mc_samples the LSTM cells that draw fresh noise at every time step of a CALL (the Variational LSTM's noise rows, the GP-LSTM's
random frequencies: such a sample is not one model over a stream).  Monte-Carlo perplexity of a held-out text is
engine.evaluate_report.
"""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import model as M
from . import ops
from ._lib import TOPK_MAX as L_TOPK_MAX
from ._lib import BayesLMError

_TRANSFORMERS = (M.TransformerModel, M.BayesTransformerModel, M.GaussTransformerModel, M.VTransformerModel)
_LSTMS = (M.RNNModel, M.BayesRNNModel, M.GaussRNNModel, M.VariationalRNNModel)
_ATTENTION = (M.MultiheadAttention, M.BayesMultiheadAttention, M._TorchMHAParams)
# a single step() runs at most this many query rows per stream through the attention at once (bounds the split-K workspace);
# longer chunks are fed in pieces
_MAX_CHUNK = 256
# mc_samples: the fused launch (blm_linear_mc_logprobs) runs the decoder product twice and stores no logit; composing ops.linear,
# ops.log_softmax_rows and torch.logsumexp runs it once and passes S x rows x V floats through memory.  Measured at V 33,000
# (tools/decode_probe.py --mc-samples, profiles/r06_decode_mc_probe.txt, composed / fused): 512 rows x K 512 1.11, 256 x 1024
# 1.00, 512 x 1024 0.84 -- the second product outweighs the saved traffic beyond rows x K = 2^18, so the distribution alone is
# composed from there on (with return_uncertainty the fused launch stays: h_pred and mi cost it 1 % and the composed path
# several more passes over the logits).
_MC_FUSED_MAX_ROWS_K = 1 << 18


def _host_ints(v, n, what):
    """A host-side integer vector of length n from an int, a sequence, a numpy array or a CPU tensor (a device tensor would
    need a synchronising copy: refused)."""
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            raise BayesLMError("%s must be known on the host (an int, a list or a CPU tensor), not a device tensor" % what)
        v = v.numpy()
    a = np.full(n, int(v), dtype=np.int64) if np.isscalar(v) else np.asarray(v, dtype=np.int64).reshape(-1)
    if a.shape[0] != n:
        raise BayesLMError("%s: %d entries for %d streams" % (what, a.shape[0], n))
    return a


def _upload(a, device, dtype):
    """Host array -> device tensor by an asynchronous copy from pinned memory (no host-device synchronisation)."""
    return _to_device(torch.as_tensor(np.ascontiguousarray(a)), device, dtype)


def _to_device(t, device, dtype):
    """A tensor on the device as ``dtype``; a host tensor goes through pinned memory, so the copy is asynchronous (from pageable
    memory it would wait for the copy to finish)."""
    if t.is_cuda:
        return t.to(device, dtype)
    return t.to(dtype).pin_memory().to(device, non_blocking=True)


class McUncertainty(NamedTuple):
    """Token-level uncertainty of a step with mc_samples (definitions: include/bayeslm.h, blm_linear_mc_stats), shaped like the
    step's main result -- (n,) or (Tq, n) -- and NaN where that is."""
    h_pred: torch.Tensor           # predictive entropy of the model average, H[pbar]
    mi: torch.Tensor               # mutual information between the next word and the weights, mean_s KL(p_s || pbar)
    nll_s: Optional[torch.Tensor]  # (..., S) NLL of the target under each sample; None without targets


class BeamHypothesis(NamedTuple):
    """One result of IncrementalLM.beam_search."""
    tokens: list   # generated word ids (prompt excluded), cut after the first eos
    score: float   # raw fp32 cumulative log-probability of `tokens`, the eos included
    length: int    # len(tokens)


class PooledHypothesis(NamedTuple):
    """One result of IncrementalLM.beam_search_pool."""
    tokens: list       # generated word ids (prompt excluded), the closing eos included when finished
    score: float       # raw fp32 cumulative log-probability of `tokens`
    norm_score: float  # fp32 score * float32(1 / length ** length_penalty): what the pool is ranked by
    length: int        # len(tokens)
    finished: bool     # ended by eos; False: still alive after max_words words


class _SampleCache:
    """Sample s of a KVCache that holds S x n streams sample-major (slot s * n + j): the same allocation entered at slot s * n.
    The K-to-V distance stays the whole cache's n_cap, so the decode kernels address it as they address the whole."""

    def __init__(self, full, first):
        self.layers, self.n_cap, self.nhead, self.max_len, self.head_dim = full.layers, full.n_cap, full.nhead, full.max_len, full.head_dim
        self.kv = full.kv[:, :, first:]
        self.past = full.past[first:]


def _redraws_per_time_step(model):
    """Name of the first LSTM cell of ``model`` whose training-mode noise is keyed by the time step inside ONE call (the
    Variational LSTM's noise rows, the GP-LSTM's random frequencies), or None: the other sites are keyed by (seed, step) alone."""
    for m in model.modules():
        if isinstance(m, M.VLSTMCell) and m.draws_noise():
            return type(m).__name__
        if isinstance(m, M.GPLSTMCell) and isinstance(getattr(m, "gpnn", None), M.GPNN2) and m.gpnn.draws_noise():
            return type(m).__name__
    return None


class IncrementalState:
    """N streams of one IncrementalLM.  ``lengths`` is the exact host mirror of the tokens each stream holds.  With mc_samples = S
    the state holds S x N streams sample-major: sample s of stream j lives in slot s * N + j."""

    def __init__(self, lm, n, buf):
        self._lm, self.n, self._buf = lm, int(n), buf
        self.lengths = [0] * self.n

    def _live(self, lm):
        if self._lm is not lm:
            raise BayesLMError("this state belongs to another IncrementalLM")
        if self._buf is None:
            raise BayesLMError("this state was consumed by reorder(); continue with the state it returned")
        return self._buf


class IncrementalLM:
    """Incremental scoring over an eval-mode language model on the GPU (see the module docstring)."""

    def __init__(self, model, max_streams=64, max_len=1024, mc_samples=0, seed=1111):
        """``mc_samples`` = S (0..64; 0: mean weights): score with the average of S Monte-Carlo weight samples keyed by ``seed``
        (module docstring).  The state is S times the mean-weight one -- per state buffer, of which reorder keeps two:
            Transformer  max(S, 1) * max_streams * layers * 2 * nhead * max_len * head_dim * 4 bytes
            LSTM         max(S, 1) * max_streams * layers * 2 * hidden * 4 bytes
        and a step runs S forward passes one after the other."""
        self.mc_samples = int(mc_samples)
        if not 0 <= self.mc_samples <= 64:
            raise BayesLMError("IncrementalLM: mc_samples must lie in 0..64 (0: mean weights), got %d" % self.mc_samples)
        self.seed = int(seed)
        name = type(model).__name__
        if type(model).__module__.endswith("model_search_bayes"):
            raise BayesLMError("IncrementalLM: %s is an architecture-search super-net; derive the searched model first" % name)
        if isinstance(model, _TRANSFORMERS):
            self.kind = "transformer"
        elif isinstance(model, _LSTMS):
            self.kind = "lstm"
        else:
            raise BayesLMError("IncrementalLM: %s is not one of the Transformer or LSTM language model families" % name)
        if model.training:
            raise BayesLMError("IncrementalLM: the model is in training mode (call model.eval(): incremental scoring uses mean "
                               "weights and no dropout)")
        self.max_streams, self.max_len = int(max_streams), int(max_len)
        if self.max_streams < 1 or self.max_len < 1:
            raise BayesLMError("IncrementalLM: max_streams and max_len must be positive")
        self.model = model
        self.vocab = model.decoder.weight.shape[0]
        if self.kind == "transformer":
            attn = [m for m in model.modules() if isinstance(m, _ATTENTION)]
            pe_rows = model.pos_encoder.pe.shape[0]
            if self.max_len > pe_rows:
                raise BayesLMError("IncrementalLM: max_len %d exceeds the positional table (%d rows)" % (self.max_len, pe_rows))
            self.layers = len(attn)
            self.nhead = attn[0].num_heads if attn else 1
            self.head_dim = model.ninp // self.nhead if attn else 1  # a stack without layers (VTransformerModel v_pos 11) caches nothing
            if self.head_dim > 128:
                raise BayesLMError("IncrementalLM: head size %d is not supported by the decode attention (<= 128)" % self.head_dim)
        else:
            self.layers, self.hidden = model.nlayers, model.nhid
        p = next(model.parameters())
        if not p.is_cuda:
            raise BayesLMError("IncrementalLM: the model must live on the GPU: bayeslms_amd has no CPU path")
        self.device = p.device
        self._spare = None
        self._mc_dec = None
        if self.mc_samples > 0:
            M.require_variational_sites(model, self.mc_samples)  # the scorer's refusal, before any launch
            cell = _redraws_per_time_step(model) if self.kind == "lstm" else None
            if cell:
                raise BayesLMError("IncrementalLM: mc_samples on %s: %s draws fresh noise at every time step of a call, so a "
                                   "sample is not one model over a stream" % (name, cell))
            # the decoder padded once (an odd vocabulary is copied onto zero rows): weights changed later need a new IncrementalLM
            self._mc_dec = ops.McDecoder(model.decoder.weight, model.decoder.bias)

    # ---------------------------------------------------------------- states
    def _new_buf(self):
        b, self._spare = self._spare, None
        if b is not None:
            return b
        cap = max(self.mc_samples, 1) * self.max_streams
        if self.kind == "transformer":
            return ops.KVCache(max(self.layers, 1), cap, self.nhead, self.max_len, self.head_dim, self.device)
        return torch.empty(2, self.layers, cap, self.hidden, device=self.device, dtype=torch.float32)

    def start(self, n):
        """n empty streams."""
        n = int(n)
        if not 1 <= n <= self.max_streams:
            raise BayesLMError("IncrementalLM.start: %d streams, max_streams is %d" % (n, self.max_streams))
        buf = self._new_buf()
        if self.kind == "transformer":
            buf.past.zero_()
        else:
            buf.zero_()  # init_hidden
        return IncrementalState(self, n, buf)

    def truncate(self, st, lengths):
        """Take tokens back out of ``st``: stream j keeps its first lengths[j] tokens (host-known, 0 <= lengths[j] <=
        st.lengths[j]).  Transformer: the device `past` of every sample slot (with mc_samples all S slices) and the host mirror
        are set back and nothing else moves -- the key/value rows beyond a length are overwritten by the next append.  LSTM:
        refused, because (h, c) of an earlier position no longer exists (bayeslms_amd/speculative.py keeps a copy instead)."""
        buf = st._live(self)
        if self.kind != "transformer":
            raise BayesLMError("IncrementalLM.truncate: an LSTM state cannot be taken back, (h, c) of an earlier position no "
                               "longer exists (copy the state before the step instead)")
        a = _host_ints(lengths, st.n, "lengths")
        if any(int(v) < 0 or int(v) > have for v, have in zip(a, st.lengths)):
            raise BayesLMError("IncrementalLM.truncate: lengths must lie in [0, st.lengths] = %s, got %s" % (st.lengths, a.tolist()))
        S = max(self.mc_samples, 1)
        with torch.no_grad():
            buf.past[:S * st.n].copy_(_upload(np.tile(a, S), self.device, torch.int32))  # sample-major: slot s * n + j
        st.lengths = [int(v) for v in a]

    def reorder(self, st, idx):
        """Beam prune / fork: new stream j continues stream idx[j] of ``st`` (idx (m,) int64: host, or one copy to the host;
        entries may repeat, m <= max_streams).  One gather launch of every layer's state; ``st`` is consumed."""
        st._live(self)
        if isinstance(idx, torch.Tensor) and idx.is_cuda:
            idx = idx.cpu()
        ih = np.asarray(idx.numpy() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64).reshape(-1)
        m = ih.shape[0]
        if not 1 <= m <= self.max_streams:
            raise BayesLMError("IncrementalLM.reorder: %d streams, max_streams is %d" % (m, self.max_streams))
        if ih.min() < 0 or ih.max() >= st.n:
            raise BayesLMError("IncrementalLM.reorder: idx out of range [0, %d)" % st.n)
        S = max(self.mc_samples, 1)
        # every sample's slice in the one launch: new slot s * m + j continues old slot s * n + idx[j]
        iall = ih if S == 1 else (np.arange(S, dtype=np.int64)[:, None] * st.n + ih[None, :]).reshape(-1)
        return self._gather(st, _upload(iall, self.device, torch.int64), m, [st.lengths[i] for i in ih])

    def reorder_device(self, st, idx):
        """reorder with a device index and no copy to the host: new stream j continues stream idx[j], idx an (st.n,) int64
        DEVICE tensor.  The caller promises what the host cannot check without a synchronise: every idx[j] lies in [0, st.n)
        (the gather copies nothing for an entry outside) and stream idx[j] holds as many tokens as stream j did, so
        ``lengths`` stays as it is, position by position (beam search: parents stay inside their group, whose beams have one
        length).  The device lengths follow the index exactly.  The same single gather launch; ``st`` is consumed."""
        st._live(self)
        if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 1):
            raise BayesLMError("IncrementalLM.reorder_device: idx must be a 1-D int64 tensor on the device (reorder takes a host index)")
        if idx.shape[0] != st.n:
            raise BayesLMError("IncrementalLM.reorder_device: %d entries for %d streams (the stream count is kept)" % (idx.shape[0], st.n))
        S = max(self.mc_samples, 1)
        with torch.no_grad():
            # every sample's slice in the one launch: new slot s * n + j continues old slot s * n + idx[j]
            iall = idx if S == 1 else (torch.arange(S, device=idx.device).view(S, 1) * st.n + idx.view(1, -1)).reshape(-1)
        return self._gather(st, iall, st.n, list(st.lengths))

    def _gather(self, st, iall, m, lengths):
        """The gather of reorder / reorder_device: every layer's state of ``st`` through the per-sample slot index ``iall`` (device)
        into the spare buffer -> the state of ``m`` streams; ``st`` is consumed and its buffer becomes the spare one."""
        src, dst = st._live(self), self._new_buf()
        n_src = max(self.mc_samples, 1) * st.n
        with torch.no_grad():
            if self.kind == "transformer":
                ops.kv_gather(src.kv, dst.kv, iall, n_src, 2 * src.layers, self.nhead, self.max_len, self.head_dim, src.past, dst.past)
            else:
                ops.kv_gather(src, dst, iall, n_src, 2 * self.layers, 1, 1, self.hidden)
        out = IncrementalState(self, m, dst)
        out.lengths = lengths
        st._buf = None
        self._spare = src
        return out

    # ---------------------------------------------------------------- search
    def step_topk(self, st, ids, k, n_new=None):
        """step, then the k best next words of every stream, best first (blm_topk_rows: value descending, lowest id on ties)
        -> (log-probs (n, k) float32, ids (n, k) int64).  With mc_samples: the top k of log pbar."""
        k = int(k)
        if not 1 <= k <= min(self.vocab, L_TOPK_MAX):
            raise BayesLMError("IncrementalLM.step_topk: k = %d outside [1, min(V = %d, %d)]" % (k, self.vocab, L_TOPK_MAX))
        return ops.topk_rows(self.step(st, ids, n_new=n_new), k)

    def beam_search(self, prompts, beam, max_words, eos, length_penalty=0.0, sync_every=16):
        """Beam search over G prompts at once -> list (per prompt) of ``beam`` BeamHypothesis, best first.

        ``prompts``: G non-empty lists of word ids (ragged allowed), G * beam <= max_streams and
        max(len(prompt)) + max_words <= max_len, both checked before any launch.  Per word: step -> blm_topk_rows(k = beam) ->
        blm_beam_select -> reorder_device; parents and tokens of every step stay on the device and are read once at the end.
        Selection inside the loop is by RAW cumulative log-probability only (exact top ``beam`` of all beam x V continuations,
        lowest candidate index on ties); ``length_penalty`` a enters only the final ranking, on the host in float64, by
        score / length ** a (ties by beam index).  A beam that produced ``eos`` is finished: it keeps its slot and score, is
        fed eos like any other stream (its rows are ignored), so every launch keeps its shape.  The host reads one "all
        finished" flag every ``sync_every`` words (0: never) and stops early when it is set; results do not depend on it.
        With mc_samples the search runs under log pbar, the model average."""
        P, T, score = self._beam_trace(prompts, beam, max_words, eos, sync_every)
        G, B = len(prompts), int(beam)
        out = []
        for g in range(G):
            hyps = []
            for b in range(B):
                cur, toks = g * B + b, []
                for w in range(P.shape[0] - 1, -1, -1):
                    toks.append(int(T[w, cur]))
                    cur = int(P[w, cur])
                toks.reverse()
                if eos in toks:
                    toks = toks[:toks.index(eos) + 1]
                hyps.append(BeamHypothesis(toks, float(score[g * B + b]), len(toks)))
            rank = sorted(range(B), key=lambda b: (-(float(np.float64(hyps[b].score) / np.float64(hyps[b].length) ** float(length_penalty))), b))
            out.append([hyps[b] for b in rank])
        return out

    def _beam_trace(self, prompts, beam, max_words, eos, sync_every=16):
        """The search loop of beam_search -> host arrays (parents (W, G * beam) int64, tokens (W, G * beam) int64, final scores
        (G * beam,) float32), W <= max_words the words generated before every beam was seen finished."""
        G, B, W, eos = len(prompts), int(beam), int(max_words), int(eos)
        if G < 1 or any(len(p) < 1 for p in prompts):
            raise BayesLMError("IncrementalLM.beam_search: at least one prompt, and at least one word (the sentence start) in each")
        if not 1 <= B <= min(self.vocab, L_TOPK_MAX):
            raise BayesLMError("IncrementalLM.beam_search: beam = %d outside [1, min(V = %d, BLM_TOPK_MAX = %d)]"
                               % (B, self.vocab, L_TOPK_MAX))
        if W < 1 or int(sync_every) < 0:
            raise BayesLMError("IncrementalLM.beam_search: max_words >= 1 and sync_every >= 0 expected")
        if G * B > self.max_streams:
            raise BayesLMError("IncrementalLM.beam_search: %d prompts x %d beams, max_streams is %d" % (G, B, self.max_streams))
        lens = [len(p) for p in prompts]
        if max(lens) + W > self.max_len:
            raise BayesLMError("IncrementalLM.beam_search: prompt of %d words + %d new words, max_len is %d" % (max(lens), W, self.max_len))
        if not 0 <= eos < self.vocab:
            raise BayesLMError("IncrementalLM.beam_search: eos %d outside the vocabulary" % eos)
        n = G * B
        ids = np.zeros((max(lens), G), dtype=np.int64)
        for g, p in enumerate(prompts):
            ids[:lens[g], g] = p
        with torch.no_grad():
            # every prompt through the model once, then forked into its group of beams
            st = self.start(G)
            lp = self.step(st, _upload(ids, self.device, torch.int64), n_new=lens)
            fork = np.repeat(np.arange(G, dtype=np.int64), B)
            st = self.reorder(st, fork)
            lp = lp.index_select(0, _upload(fork, self.device, torch.int64))
            s0 = np.full(n, -np.inf, dtype=np.float32)
            s0[::B] = 0.0  # one live beam per group, or the first step picks `beam` copies of one word
            score = _upload(s0, self.device, torch.float32)
            finished = torch.zeros(n, dtype=torch.uint8, device=self.device)
            parents, tokens = [], []
            for w in range(W):
                vals, cand = ops.topk_rows(lp, B)
                score, finished, parent, token = ops.beam_select(vals, cand, score, finished, B, eos)
                parents.append(parent)
                tokens.append(token)
                if w + 1 == W:
                    break
                if sync_every and (w + 1) % int(sync_every) == 0 and bool(finished.all()):  # the loop's only host read
                    break
                st = self.reorder_device(st, parent)
                lp = self.step(st, token)
            return torch.stack(parents).cpu().numpy(), torch.stack(tokens).cpu().numpy(), score.cpu().numpy()

    def beam_search_pool(self, prompts, beam, max_words, eos, pool=None, length_penalty=0.0, min_words=0, sync_every=16, _stop=True):
        """Beam search with a pool of finished hypotheses over G prompts at once -> list (per prompt) of up to ``pool`` (default
        ``beam``, at most BLM_TOPK_MAX) PooledHypothesis, best first by norm_score, then by the order in which they were pooled.

        A hypothesis that produces ``eos`` among the ``beam`` best candidates of its word leaves the beam for the pool, ranked
        there by norm_score = score / length ** ``length_penalty`` (a >= 0; one fp32 multiply by float32(1 / length ** a)), and
        the beam is refilled to ``beam`` live hypotheses at every word; an eos that would end a hypothesis of fewer than
        ``min_words`` words (the eos counted) is not considered.  The hypotheses still alive after ``max_words`` words are
        pooled unfinished.  A prompt's search stops once its pool is full and nothing alive can still enter it (include/bayeslm.h,
        blm_beam_select_pool, has the exact rules).  Per word: step -> blm_topk_rows(k = min(2 * beam, V)) ->
        blm_beam_select_pool -> reorder_device; the pool, the parents and the tokens of every step stay on the device and are read
        once at the end, where the hypotheses are traced back.  The host reads one "every prompt is done" flag every
        ``sync_every`` words (0: never); results do not depend on it.  ``prompts``, ``max_words`` and the capacity checks are
        beam_search's, all made before any launch.  With mc_samples the search runs under log pbar, the model average."""
        G, B, W, eos, a, M_ = len(prompts), int(beam), int(max_words), int(eos), float(length_penalty), int(min_words)
        P = B if pool is None else int(pool)
        if G < 1 or any(len(p) < 1 for p in prompts):
            raise BayesLMError("IncrementalLM.beam_search_pool: at least one prompt, and at least one word (the sentence start) in each")
        if not 1 <= B <= L_TOPK_MAX // 2:
            raise BayesLMError("IncrementalLM.beam_search_pool: beam = %d outside [1, BLM_TOPK_MAX / 2 = %d]" % (B, L_TOPK_MAX // 2))
        if not 1 <= P <= L_TOPK_MAX:
            raise BayesLMError("IncrementalLM.beam_search_pool: pool = %d outside [1, BLM_TOPK_MAX = %d]" % (P, L_TOPK_MAX))
        if W < 1 or int(sync_every) < 0 or M_ < 0:
            raise BayesLMError("IncrementalLM.beam_search_pool: max_words >= 1, min_words >= 0 and sync_every >= 0 expected")
        if not a >= 0.0 or math.isinf(a):
            raise BayesLMError("IncrementalLM.beam_search_pool: length_penalty %r: the stopping rule needs a finite a >= 0" % length_penalty)
        if G * B > self.max_streams:
            raise BayesLMError("IncrementalLM.beam_search_pool: %d prompts x %d beams, max_streams is %d" % (G, B, self.max_streams))
        lens = [len(p) for p in prompts]
        if max(lens) + W > self.max_len:
            raise BayesLMError("IncrementalLM.beam_search_pool: prompt of %d words + %d new words, max_len is %d"
                               % (max(lens), W, self.max_len))
        if not 0 <= eos < self.vocab:
            raise BayesLMError("IncrementalLM.beam_search_pool: eos %d outside the vocabulary" % eos)
        n, V = G * B, self.vocab
        k = min(2 * B, V)
        ids = np.zeros((max(lens), G), dtype=np.int64)
        for g, p in enumerate(prompts):
            ids[:lens[g], g] = p
        # a bound of 0 is never below a norm (log-probabilities are <= 0): nothing stops before the flush
        inv_max = ops.beam_inv_norm(W, a) if _stop else 0.0
        with torch.no_grad():
            st = self.start(G)
            lp = self.step(st, _upload(ids, self.device, torch.int64), n_new=lens)
            fork = np.repeat(np.arange(G, dtype=np.int64), B)
            st = self.reorder(st, fork)
            lp = lp.index_select(0, _upload(fork, self.device, torch.int64))
            l0 = np.zeros(n, dtype=np.uint8)
            l0[::B] = 1  # one live beam per group, or the first step picks `beam` copies of one word
            live = _upload(l0, self.device, torch.uint8)
            score = torch.zeros(n, dtype=torch.float32, device=self.device)
            fin = ops.BeamPool(G, P, self.device)
            parents, tokens = [], []
            for w in range(W):
                vals, cand = ops.topk_rows(lp, k)
                score, live, parent, token, _, all_done = ops.beam_select_pool(
                    vals, cand, score, live, B, V, eos, w, w + 1, M_, ops.beam_inv_norm(w + 1, a), inv_max, w + 1 == W, fin)
                parents.append(parent)
                tokens.append(token)
                if w + 1 == W:
                    break
                if sync_every and (w + 1) % int(sync_every) == 0 and bool(all_done.item()):  # the loop's only host read
                    break
                st = self.reorder_device(st, parent)
                lp = self.step(st, token)
            PA, TK, h = torch.stack(parents).cpu().numpy(), torch.stack(tokens).cpu().numpy(), fin.host()
        out = []
        for g in range(G):
            hyps = []
            for e in range(int(h["count"][g])):
                done, cur, w = bool(h["finished"][g, e]), int(h["parent"][g, e]), int(h["step"][g, e])
                toks = [eos] if done else []
                for ww in range(w - 1 if done else w, -1, -1):
                    toks.append(int(TK[ww, cur]))
                    cur = int(PA[ww, cur])
                toks.reverse()
                hyps.append(PooledHypothesis(toks, float(h["raw"][g, e]), float(h["norm"][g, e]), int(h["len"][g, e]), done))
            out.append(hyps)
        return out

    # ---------------------------------------------------------------- stepping
    def step(self, st, ids, n_new=None, all_positions=False, targets=None, return_uncertainty=False):
        """Feed ``ids`` (Tq, n) (or (n,): one word per stream) and return the log-probabilities of the next word: (n, V) after each
        stream's last new token, or (Tq, n, V) with all_positions.  ``n_new``: stream j takes only its first n_new[j] rows
        (0 <= n_new[j] <= Tq, host-known; a stream with 0 keeps its state and gets NaN rows).  ``targets``: (n,) next words (or (Tq, n) with all_positions) -> their NLL instead.
        With mc_samples the distribution is the model average pbar (log pbar; the targets' NLL under pbar), and
        ``return_uncertainty`` makes the result a pair (that, McUncertainty)."""
        buf = st._live(self)
        if return_uncertainty and self.mc_samples < 2:
            raise BayesLMError("IncrementalLM.step: return_uncertainty needs mc_samples >= 2 (got %d)" % self.mc_samples)
        if self.model.training:
            raise BayesLMError("IncrementalLM.step: the model is in training mode (call model.eval())")
        if ids.dim() == 1:
            ids = ids.unsqueeze(0)
        if ids.dim() != 2 or ids.shape[1] != st.n:
            raise BayesLMError("IncrementalLM.step: ids must be (Tq, %d) or (%d,)" % (st.n, st.n))
        Tq, N = ids.shape
        if Tq < 1:
            raise BayesLMError("IncrementalLM.step: empty chunk")
        k = _host_ints(Tq if n_new is None else n_new, N, "n_new")
        if k.min() < 0 or k.max() > Tq or k.max() < 1:
            raise BayesLMError("IncrementalLM.step: n_new must lie in [0, %d], and some stream must take a row" % Tq)
        after = [a + int(b) for a, b in zip(st.lengths, k)]
        if max(after) > self.max_len:
            raise BayesLMError("IncrementalLM.step: a stream would hold %d tokens, max_len is %d" % (max(after), self.max_len))
        if targets is not None and tuple(targets.shape) != ((Tq, N) if all_positions else (N,)):
            raise BayesLMError("IncrementalLM.step: targets must be %s" % (((Tq, N),) if all_positions else ((N,),)))
        ids = _to_device(ids, self.device, torch.int64)
        ragged = bool((k < Tq).any())
        with torch.no_grad():
            if self.mc_samples == 0:
                return self._decode(self._hidden_rows(st, buf, ids, k, ragged), Tq, N, k, all_positions, targets)
            # S passes, sample s on slots [s * n, (s + 1) * n) of the state; the host lengths move once
            before, passes = st.lengths, []
            with M.mc_sampling(self.model, self.seed, self.mc_samples):
                for s in range(self.mc_samples):
                    self.model.set_step(s)
                    st.lengths = before
                    if self.kind == "transformer":
                        part = _SampleCache(buf, s * N)
                    else:
                        part = buf[:, :, s * N:]
                    passes.append(self._hidden_rows(st, part, ids, k, ragged))
            return self._decode_mc(passes, Tq, N, k, all_positions, targets, return_uncertainty)

    def _hidden_rows(self, st, buf, ids, k, ragged):
        """One forward over the chunk on the state ``buf`` -> [(first row, rows per stream, (flat indices or None, hidden rows))]"""
        Tq = ids.shape[0]
        rows = []  # (Tq, N, d) hidden rows of the chunk, or packed real rows with their flat indices
        if self.kind == "transformer":
            for t0 in range(0, Tq, _MAX_CHUNK):
                kk = np.clip(k - t0, 0, min(_MAX_CHUNK, Tq - t0))
                if kk.max() == 0:  # only padding left in this piece
                    break
                rows.append((t0, kk, self._transformer_chunk(st, buf, ids[t0:t0 + _MAX_CHUNK], kk)))
        else:
            rows.append((0, k, self._lstm_chunk(st, buf, ids, k, ragged)))
        return rows

    def _transformer_chunk(self, st, cache, ids, k):
        """One piece of a chunk through the model under ops.cached_tokens -> (flat row indices t * N + n or None, hidden rows).
        k[n] may be 0 here (a stream whose rows ended in an earlier piece): it takes no part."""
        Tq, N = ids.shape
        ragged = bool((k < Tq).any())
        sel_h = None
        if ragged:
            t = np.arange(Tq)[:, None]
            sel_h = np.nonzero((t < k[None, :]).reshape(-1))[0]
        ctx_max = max(a + int(b) for a, b in zip(st.lengths, k))
        n_new = _upload(k, self.device, torch.int32) if ragged else None
        sel = _upload(sel_h, self.device, torch.int64) if ragged else None
        with ops.cached_tokens(cache, Tq, N, ctx_max, n_new, sel) as ctx, self.model.decoder.inference(input_rows=True):
            h = self.model(ids)
            if ctx.layer != self.layers:
                raise BayesLMError("IncrementalLM: %d attention layers ran, %d expected" % (ctx.layer, self.layers))
        # the lengths move on only after every layer has appended at the old ones
        if ragged:
            cache.past[:N] += n_new
        else:
            cache.past[:N] += Tq
        st.lengths = [a + int(b) for a, b in zip(st.lengths, k)]
        return sel_h, h.reshape(-1, h.shape[-1])

    def _lstm_chunk(self, st, hc, ids, k, ragged):
        """(h, c) carried through the model's own fused LSTM kernels: the rows every stream takes (min n_new) as one chunk, then a
        ragged tail step by step on the streams that still have rows (their states gathered, advanced and scattered back)."""
        Tq, N = ids.shape
        h, c = hc[0, :, :N], hc[1, :, :N]
        p = int(k.min())
        with self.model.decoder.inference(input_rows=True):
            if p > 0:
                y0, (h2, c2) = self.model(ids[:p], (h.contiguous(), c.contiguous()))
                h.copy_(h2)
                c.copy_(c2)
            if not ragged:
                out = (None, y0.reshape(-1, y0.shape[-1]))
            else:
                y = torch.full((Tq, N, self.hidden), float("nan"), device=self.device)
                if p > 0:
                    y[:p] = y0
                for t in range(p, Tq):
                    act = np.nonzero(k > t)[0]
                    if act.shape[0] == 0:
                        break
                    a = _upload(act, self.device, torch.int64)
                    ys, (h2, c2) = self.model(ids[t:t + 1].index_select(1, a), (h.index_select(1, a), c.index_select(1, a)))
                    h.index_copy_(1, a, h2)
                    c.index_copy_(1, a, c2)
                    y[t].index_copy_(0, a, ys.reshape(-1, ys.shape[-1]))
                out = (None, y.reshape(-1, self.hidden))
        st.lengths = [a + int(b) for a, b in zip(st.lengths, k)]
        return out

    def _returned(self, passes, Tq, N, k, all_positions):
        """The hidden rows a step returns, of every pass in ``passes`` (all over the same chunk) -> ([rows per pass], slots, slots
        that have a row, their device indices or None when every slot has one)."""
        # host map: (t, n) -> row of the concatenated hidden rows (-1: padding)
        rowof = np.full(Tq * N, -1, dtype=np.int64)
        base = 0
        for t0, kk, (sel_h, x) in passes[0]:
            tp = x.shape[0] // N if sel_h is None else None
            flat = np.arange(tp * N) if sel_h is None else sel_h
            rowof[t0 * N + flat] = base + np.arange(flat.shape[0])
            base += flat.shape[0]
        xcat = [ps[0][2][1] if len(ps) == 1 else torch.cat([x for _, _, (_, x) in ps], 0) for ps in passes]
        # slots: the returned rows -- (t, n) flat positions with all_positions, else streams; `want` the slots that have a row
        nslot = Tq * N if all_positions else N
        if all_positions:
            want = np.nonzero(rowof >= 0)[0]
            src = rowof[want]
        else:
            want = np.nonzero(k > 0)[0]
            src = rowof[(k[want] - 1) * N + want]
        every = want.shape[0] == nslot
        if np.array_equal(src, np.arange(src[0], src[0] + src.shape[0])):  # full chunks: a slice, no index upload
            xr = [x[int(src[0]):int(src[0]) + src.shape[0]] for x in xcat]
        else:
            sidx = _upload(src, self.device, torch.int64)
            xr = [x.index_select(0, sidx) for x in xcat]
        widx = None if every else _upload(want, self.device, torch.int64)
        return xr, nslot, every, widx

    def _decode(self, pieces, Tq, N, k, all_positions, targets):
        """Decoder product on the rows that are returned only, then the log-softmax (blm_log_softmax_rows) or the NLL of the
        targets without logits (blm_linear_nll).  Returned slots without a row (padding, streams with n_new 0) are NaN."""
        (xr,), nslot, every, widx = self._returned([pieces], Tq, N, k, all_positions)
        W, b = self.model.decoder.weight, self.model.decoder.bias
        V = self.vocab
        if targets is not None:
            tg = _to_device(targets, self.device, torch.int64).reshape(-1)
            if not every:
                tg = tg.index_select(0, widx)
            if ops.linear_nll_supported(W, b):
                r = ops.linear_nll(xr, W, b, tg)
            else:
                lp = ops.log_softmax_rows(ops.linear(xr, W, b), V)
                r = -lp.gather(1, tg.unsqueeze(1)).squeeze(1)
            if not every:
                r = torch.full((nslot,), float("nan"), device=self.device).index_copy_(0, widx, r)
            return r.view(Tq, N) if all_positions else r
        lp = ops.log_softmax_rows(ops.linear(xr, W, b), V)
        if not every:
            lp = torch.full((nslot, V), float("nan"), device=self.device).index_copy_(0, widx, lp)
        return lp.view(Tq, N, V) if all_positions else lp

    def _decode_mc(self, passes, Tq, N, k, all_positions, targets, uncertainty):
        """One decoder launch over the S passes' returned rows: log pbar (blm_linear_mc_logprobs), or with targets their NLL under
        pbar with no (rows, V) buffer (blm_linear_mc_stats); NaN in the slots without a row, in every array."""
        xr, nslot, every, widx = self._returned(passes, Tq, N, k, all_positions)
        W, b = self.model.decoder.weight, self.model.decoder.bias
        x = torch.stack(xr)
        S = self.mc_samples
        lead = (Tq, N) if all_positions else (N,)

        def slots(r):  # (rows, ...) -> the step's shape, NaN where no row is
            if r is None:
                return None
            if not every:
                r = torch.full((nslot,) + tuple(r.shape[1:]), float("nan"), device=self.device).index_copy_(0, widx, r)
            return r.view(*lead, *r.shape[1:])

        if targets is not None:
            tg = _to_device(targets, self.device, torch.int64).reshape(-1)
            if not every:
                tg = tg.index_select(0, widx)
            r = ops.linear_mc_stats(x, W, b, tg, dec=self._mc_dec)
            main, rec = slots(r.bma_nll), (r.h_pred, r.mi, r.nll_s)
        elif not uncertainty and (x.shape[1] << (S - 1).bit_length()) * x.shape[2] > _MC_FUSED_MAX_ROWS_K:
            lp = ops.log_softmax_rows(ops.linear(x.reshape(-1, x.shape[2]), W, b), self.vocab)
            main, rec = slots(torch.logsumexp(lp.view(S, -1, self.vocab), 0).sub_(math.log(S))), None
        else:
            r = ops.linear_mc_logprobs(x, W, b, dec=self._mc_dec, stats=uncertainty)
            main, rec = slots(r.logp), (r.h_pred, r.mi, None)
        if not uncertainty:
            return main
        return main, McUncertainty(*(slots(t) for t in rec))
