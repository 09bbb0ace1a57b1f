"""Text generation from a trained language model (the word_language_model example's generate.py, which the reference dropped),
on the incremental key/value-cache path (bayeslms_amd/incremental.py): each new word costs one decode step, not a forward over
the whole history.

    python -m bayeslms_amd.generate --model-path model.pt --vocabulary words.txt --model Transformer --emsize 512 --nhid 2048 \
        --nlayers 6 --nhead 8 --words 50 --temperature 1.0 --streams 4 --prompt "the meeting" --outf generated.txt

The model is built from the scorer's flags (compute_sentence_scores.build_models) and loaded as the scorer loads it.  Every stream
starts from the sentence boundary ``<s>`` followed by the prompt (OOV words map to ``<unk>``); ``--words`` new words are drawn per
stream (``--temperature 0``: greedy) and written space-separated, one stream per line.

``--mc-samples S`` draws every word from the average of S Monte-Carlo weight samples of a Bayesian / GP model (the distribution
the n-best scorer's ``--mc-samples`` scores with; ``--mc-seed`` keys the weights, ``--seed`` the sampling noise), and
``--write-uncertainty PATH`` then writes, per generated word, the predictive entropy of that average and the mutual information
between the word and the weights.

``--top-k K`` / ``--top-p P`` restrict every draw to the K most probable words and / or to the smallest set of most probable
words whose probability reaches P (blm_sample_rows_filtered; the same noise as the unrestricted draw).  ``--beam B`` searches
instead of sampling (IncrementalLM.beam_search; a hypothesis ends at the sentence boundary ``<s>``): the ``--nbest`` N (default 1)
best continuations of the prompt are written best first, one per line, ranked by score / length ** ``--length-penalty``, and
``--write-scores PATH`` writes one "rank score length" line per hypothesis.  With ``--mc-samples`` the search runs under the
model average.

``--finished-pool P`` (with ``--beam``; default 0: the search above, unchanged) searches with a pool of P finished hypotheses
beside the beam (IncrementalLM.beam_search_pool): a hypothesis that ends leaves the beam, which is refilled to B live ones at
every word, the pool is ranked by score / length ** ``--length-penalty`` (>= 0) INSIDE the loop, and the search stops once
nothing alive can enter it.  ``--nbest`` may then go up to P (fewer lines are written when fewer hypotheses were found),
``--min-words M`` refuses a hypothesis of fewer than M words (the closing ``<s>`` counted), and ``--write-scores`` writes
"rank score normalised-score length" with a trailing "unfinished" on a hypothesis that was still alive after ``--words`` words.

``--speculate G`` samples speculatively (bayeslms_amd/speculative.py): a cheap draft proposes G words per stream, the model scores
all G + 1 positions in one chunk and an accept / reject rule keeps a prefix and draws one more word; the words written are
distributed exactly as without the flag (not the same words: the noise is keyed differently).  The draft is the model itself at
its mean weights, which needs ``--mc-samples S`` >= 2 to be any cheaper than the target, or another checkpoint:
``--draft-model-path student.pt``, shaped by ``--draft-args "--model Transformer ..."`` (this command line's own flags; only the
model-shaping ones are read, the default is the target's own).  The run ends with one line on stderr: rounds, words per target
chunk, acceptance rate.  Not built with it: ``--beam``, ``--top-k`` / ``--top-p`` and ``--write-uncertainty``."""
import argparse
import shlex
import sys

import torch

from . import compute_sentence_scores as S
from . import ops
from .incremental import IncrementalLM


def build_parser():
    p = argparse.ArgumentParser(description="Generate text with a trained neural LM (MI355X engine, incremental decoding).")
    p.add_argument('--model-path', type=str, required=True)
    p.add_argument('--vocabulary', type=str, required=True, help='words.txt (word id per line)')
    p.add_argument('--model', type=str, default='LSTM')
    p.add_argument('--emsize', type=int, default=1024)
    p.add_argument('--nhid', type=int, default=1024)
    p.add_argument('--nlayers', type=int, default=2)
    p.add_argument('--nhead', type=int, default=8)
    p.add_argument('--uncertainty', type=str, default='none')
    p.add_argument('--T_bayes_pos', type=str, default='none')
    p.add_argument('--L_bayes_pos', type=int, default=0)
    p.add_argument('--L_gauss_pos', type=str, default='00')
    p.add_argument('--T_gauss_pos', type=int, default=3)
    p.add_argument('--L_v_pos', type=str, default='11')
    p.add_argument('--T_v_pos', type=int, default=0)
    p.add_argument('--words', type=int, default=100, help='words to generate per stream')
    p.add_argument('--temperature', type=float, default=None, help='default 1.0; 0: greedy (argmax, lowest id on ties)')
    p.add_argument('--top-k', type=int, default=None, metavar='K', help='sample among the K most probable words only (0: all)')
    p.add_argument('--top-p', type=float, default=None, metavar='P',
                   help='sample among the smallest set of most probable words whose probability reaches P, in (0, 1] (1: all)')
    p.add_argument('--beam', type=int, default=0, metavar='B',
                   help='B > 0: beam search with B beams instead of sampling; at most --words words per hypothesis, ended by <s>')
    p.add_argument('--nbest', type=int, default=1, metavar='N', help='with --beam: write the N best hypotheses (N <= B; with --finished-pool P: N <= P)')
    p.add_argument('--length-penalty', type=float, default=0.0, metavar='A',
                   help='with --beam: the final ranking is by score / length ** A (the search itself is by raw score)')
    p.add_argument('--write-scores', type=str, default='', metavar='PATH',
                   help='with --beam: one line "rank score length" per written hypothesis (rank from 1, score %%.6f: its '
                        'cumulative log-probability including the closing <s>, length in words including it)')
    p.add_argument('--finished-pool', type=int, default=0, metavar='P',
                   help='with --beam, P > 0: keep the P best finished hypotheses in a pool beside the beam, ranked by score / length '
                        '** A inside the search; --nbest may go up to P (0: finished hypotheses keep their beam slot)')
    p.add_argument('--min-words', type=int, default=0, metavar='M',
                   help='with --finished-pool: no hypothesis of fewer than M words, the closing <s> counted')
    p.add_argument('--seed', type=int, default=1111, help='key of the sampling noise: the same seed gives the same text')
    p.add_argument('--streams', type=int, default=1, help='independent samples, generated in one batch')
    p.add_argument('--prompt', type=str, default='', help='words every stream starts from (after <s>)')
    p.add_argument('--outf', type=str, default='generated.txt', help="output file ('-': stdout)")
    p.add_argument('--mc-samples', type=int, default=0,
                   help='S > 0: draw every word from the average of S Monte-Carlo weight samples (0: mean weights)')
    p.add_argument('--mc-seed', type=int, default=1111, help='key of the weight samples (the n-best scorer\'s default)')
    p.add_argument('--write-uncertainty', type=str, default='', metavar='PATH',
                   help='with --mc-samples >= 2: one line per stream, in the order of --outf, holding for each generated word '
                        'the three space-separated fields "word h_pred mi" (3 x --words fields per line, single spaces, no '
                        'header): the word as written to --outf, then %%.6g of the predictive entropy of the model average and of '
                        'the mutual information between the word and the weights (nats; the distribution the word was drawn from)')
    p.add_argument('--speculate', type=int, default=0, metavar='G',
                   help='G in 1..16: speculative sampling, G drafted words per round and stream (0: off)')
    p.add_argument('--draft-model-path', type=str, default='', metavar='PATH',
                   help='with --speculate: the checkpoint that drafts (default: the model itself at mean weights, which needs '
                        '--mc-samples >= 2)')
    p.add_argument('--draft-args', type=str, default=None, metavar='"..."',
                   help='with --draft-model-path: the flags that shape the DRAFT, as one string of this command line\'s own flags '
                        '(a checkpoint holds weights, not an architecture).  Only the model-shaping ones are read: %s.  Default: '
                        'the target\'s own' % ", ".join("--" + f for f in DRAFT_FLAGS))
    return p


# the flags build_models reads: what --draft-args may set for the draft
DRAFT_FLAGS = ("model", "emsize", "nhid", "nlayers", "nhead", "uncertainty", "T_bayes_pos", "L_bayes_pos", "L_gauss_pos", "T_gauss_pos",
               "L_v_pos", "T_v_pos")


def check_speculate_args(args):
    """The --speculate / --draft-* flags, refused before any file or device is looked at -> the draft's model-shaping flags (a
    namespace; None when the model drafts for itself or nothing is speculated)."""
    if not args.speculate:
        for flag, given in (("--draft-model-path", bool(args.draft_model_path)), ("--draft-args", args.draft_args is not None)):
            if given:
                raise SystemExit("%s needs --speculate" % flag)
        return None
    given = [f for f, v in (("--beam", args.beam), ("--top-k", args.top_k is not None), ("--top-p", args.top_p is not None),
                            ("--write-uncertainty", args.write_uncertainty)) if v]
    if given:
        raise SystemExit("--speculate is not built with %s (filtering would need the filtered target in the accept rule)" % ", ".join(given))
    if not 1 <= args.speculate <= 16:
        raise SystemExit("--speculate G: G in 1..16 expected (got %d)" % args.speculate)
    if not args.draft_model_path:
        if args.draft_args is not None:
            raise SystemExit("--draft-args needs --draft-model-path")
        if args.mc_samples < 2:
            raise SystemExit("--speculate without --draft-model-path drafts at the model's own mean weights, which needs --mc-samples "
                             ">= 2 (got --mc-samples %d)" % args.mc_samples)
        return None
    shape = argparse.Namespace(**{f: getattr(args, f) for f in DRAFT_FLAGS})
    if args.draft_args is not None:
        theirs = build_parser().parse_args(["--model-path", "-", "--vocabulary", "-"] + shlex.split(args.draft_args))
        shape = argparse.Namespace(**{f: getattr(theirs, f) for f in DRAFT_FLAGS})
    shape.interpolation_flag = 0
    return shape


def speculative_generate(model, vocab, words, gamma, streams=1, temperature=1.0, seed=1111, prompt="", mc_samples=0, mc_seed=1111,
                         draft_model=None):
    """generate() by speculative sampling -> (list of `streams` lists of generated word ids, SpecStats); ``draft_model`` None:
    the model's own mean weights draft (mc_samples >= 2)."""
    from .speculative import SpeculativeLM
    ctx = _context(vocab, prompt)
    max_len = len(ctx) + max(words, 1) + gamma
    target = IncrementalLM(model, max_streams=streams, max_len=max_len, mc_samples=mc_samples, seed=mc_seed)
    draft = None if draft_model is None else IncrementalLM(draft_model, max_streams=streams, max_len=max_len)
    return SpeculativeLM(target, draft, gamma).generate(ctx, words, streams, temperature, seed)


def _context(vocab, prompt):
    """<s> followed by the prompt's word ids (OOV -> <unk>)"""
    unk = vocab.get('<unk>')
    ctx = [vocab['<s>']]
    for w in prompt.split():
        if w not in vocab and unk is None:
            raise SystemExit("prompt word %r is not in the vocabulary, which has no <unk>" % w)
        ctx.append(vocab.get(w, unk))
    return ctx


def beam_generate(model, vocab, words, beam, nbest=1, prompt="", length_penalty=0.0, mc_samples=0, mc_seed=1111):
    """-> the ``nbest`` best BeamHypothesis of a ``beam``-wide search for at most ``words`` words after <s> + prompt, best first;
    a hypothesis ends at the sentence boundary <s>."""
    ctx = _context(vocab, prompt)
    lm = IncrementalLM(model, max_streams=beam, max_len=len(ctx) + words, mc_samples=mc_samples, seed=mc_seed)
    return lm.beam_search([ctx], beam, words, vocab['<s>'], length_penalty)[0][:nbest]


def pool_generate(model, vocab, words, beam, pool, nbest=1, prompt="", length_penalty=0.0, min_words=0, mc_samples=0, mc_seed=1111):
    """-> the (up to) ``nbest`` best PooledHypothesis of a ``beam``-wide search with a pool of ``pool`` finished hypotheses, for
    at most ``words`` words after <s> + prompt, best first by normalised score."""
    ctx = _context(vocab, prompt)
    lm = IncrementalLM(model, max_streams=beam, max_len=len(ctx) + words, mc_samples=mc_samples, seed=mc_seed)
    return lm.beam_search_pool([ctx], beam, words, vocab['<s>'], pool, length_penalty, min_words)[0][:nbest]


def generate(model, vocab, words, streams=1, temperature=1.0, seed=1111, prompt="", mc_samples=0, mc_seed=1111, uncertainty=False,
             top_k=0, top_p=1.0):
    """-> list of `streams` lists of generated word ids (prompt excluded); with ``uncertainty`` (mc_samples >= 2) the pair
    (that, (h_pred, mi)): two (streams, words) float arrays of the distributions the words were drawn from."""
    ctx = _context(vocab, prompt)
    lm = IncrementalLM(model, max_streams=streams, max_len=len(ctx) + max(words, 1), mc_samples=mc_samples, seed=mc_seed)
    st = lm.start(streams)
    dev = lm.device
    ids = torch.tensor(ctx, dtype=torch.int64).view(-1, 1).expand(-1, streams).contiguous().to(dev)
    out = torch.empty(max(words, 0), streams, dtype=torch.int64, device=dev)
    unc = torch.empty(2, max(words, 0), streams, dtype=torch.float32, device=dev)
    for i in range(words):
        if uncertainty:
            lp, u = lm.step(st, ids, return_uncertainty=True)
            unc[0, i], unc[1, i] = u.h_pred, u.mi
        else:
            lp = lm.step(st, ids)  # with mc_samples: log pbar, the model average
        nxt = ops.sample_rows(lp, temperature, seed, 0, i, top_k, top_p)  # shift-invariant: log-probs sample as the logits would
        out[i] = nxt
        ids = nxt.view(1, streams)
    if uncertainty:
        h, mi = unc.cpu().numpy()
        return out.t().cpu().tolist(), (h.T, mi.T)
    return out.t().cpu().tolist()


def write_uncertainty(rows, h_pred, mi, path):
    """--write-uncertainty: one line per stream, "word h_pred mi" per generated word (%.6g), single spaces, no header."""
    with open(path, 'w', encoding='utf-8') as f:
        for r, hs, ms in zip(rows, h_pred, mi):
            f.write(" ".join("%s %.6g %.6g" % (w, float(a), float(b)) for w, a, b in zip(r, hs, ms)) + "\n")


def main(argv=None):
    args = build_parser().parse_args(argv)
    draft_shape = check_speculate_args(args)  # before the input paths, the model or a device are looked at
    if args.beam:  # before the input paths, the model or a device are looked at
        given = [f for f, v in (("--temperature", args.temperature), ("--top-k", args.top_k), ("--top-p", args.top_p)) if v is not None]
        if given:
            raise SystemExit("--beam searches, it does not sample: %s cannot be given with it" % ", ".join(given))
        if args.streams != 1:
            raise SystemExit("--beam writes the hypotheses of ONE search: --streams %d cannot be given with it" % args.streams)
        if args.write_uncertainty:
            raise SystemExit("--write-uncertainty belongs to sampling; --beam has --write-scores")
        if args.finished_pool:
            if args.beam < 1 or args.words < 1 or not 1 <= args.nbest <= args.finished_pool:
                raise SystemExit("--beam >= 1, 1 <= --nbest <= --finished-pool and --words >= 1 expected")
            if not 1 <= args.finished_pool <= 256 or args.beam > 128:
                raise SystemExit("--finished-pool in [1, 256] and --beam <= 128 with it expected")
            if args.min_words < 0 or not 0.0 <= args.length_penalty < float("inf"):
                raise SystemExit("--min-words >= 0 and a finite --length-penalty >= 0 expected with --finished-pool")
        elif args.min_words:
            raise SystemExit("--min-words needs --finished-pool")
        elif args.beam < 0 or not 1 <= args.nbest <= args.beam or args.words < 1:
            raise SystemExit("--beam >= 1, 1 <= --nbest <= --beam and --words >= 1 expected")
    elif args.nbest != 1 or args.length_penalty != 0.0 or args.write_scores:
        raise SystemExit("--nbest, --length-penalty and --write-scores need --beam")
    elif args.finished_pool or args.min_words:
        raise SystemExit("--finished-pool and --min-words need --beam")
    args.temperature = 1.0 if args.temperature is None else args.temperature
    args.top_k = 0 if args.top_k is None else args.top_k
    args.top_p = 1.0 if args.top_p is None else args.top_p
    if args.top_k < 0 or not 0.0 < args.top_p <= 1.0:
        raise SystemExit("--top-k >= 0 and --top-p in (0, 1] expected")
    if args.words < 0 or args.streams < 1 or args.temperature < 0:
        raise SystemExit("--words >= 0, --streams >= 1 and --temperature >= 0 expected")
    if args.mc_samples < 0 or args.mc_samples > 64:
        raise SystemExit("--mc-samples must lie in 0..64 (got %d)" % args.mc_samples)
    if args.write_uncertainty and args.mc_samples < 2:  # before the input paths, the model or a device are looked at
        raise SystemExit("--write-uncertainty needs --mc-samples >= 2 (got --mc-samples %d)" % args.mc_samples)
    if not torch.cuda.is_available():
        raise SystemExit("bayeslms_amd generation needs an MI355X: there is no CPU path")
    vocab = S.read_vocab(args.vocabulary)
    if '<s>' not in vocab:
        raise SystemExit("the vocabulary has no <s>")
    args.interpolation_flag = 0
    model, _ = S.build_models(args, len(vocab))
    S.load_partial(model, args.model_path)
    model = model.to(torch.device("cuda", torch.cuda.current_device())).eval()
    inv = {i: w for w, i in vocab.items()}
    if args.beam and args.finished_pool:
        hyps = pool_generate(model, vocab, args.words, args.beam, args.finished_pool, args.nbest, args.prompt, args.length_penalty,
                             args.min_words, args.mc_samples, args.mc_seed)
        ids = [h.tokens for h in hyps]
        if args.write_scores:
            with open(args.write_scores, 'w', encoding='utf-8') as f:
                f.write("".join("%d %.6f %.6f %d%s\n" % (r + 1, h.score, h.norm_score, h.length, "" if h.finished else " unfinished")
                                for r, h in enumerate(hyps)))
    elif args.beam:
        hyps = beam_generate(model, vocab, args.words, args.beam, args.nbest, args.prompt, args.length_penalty, args.mc_samples,
                             args.mc_seed)
        ids = [h.tokens for h in hyps]
        if args.write_scores:
            with open(args.write_scores, 'w', encoding='utf-8') as f:
                f.write("".join("%d %.6f %d\n" % (r + 1, h.score, h.length) for r, h in enumerate(hyps)))
    elif args.speculate:
        draft_model = None
        if args.draft_model_path:
            draft_model, _ = S.build_models(draft_shape, len(vocab))
            S.load_partial(draft_model, args.draft_model_path)
            draft_model = draft_model.to(torch.device("cuda", torch.cuda.current_device())).eval()
        ids, stats = speculative_generate(model, vocab, args.words, args.speculate, args.streams, args.temperature, args.seed,
                                          args.prompt, args.mc_samples, args.mc_seed, draft_model)
        sys.stderr.write("speculative sampling: %d rounds, %d target chunks, %.3f words per target chunk and stream, acceptance rate "
                         "%.4f (%d of %d drafted words)\n" % (stats.rounds, stats.target_chunks, stats.words_per_chunk(args.speculate),
                                                              stats.acceptance_rate, stats.accepted, stats.drafted))
    else:
        ids = generate(model, vocab, args.words, args.streams, args.temperature, args.seed, args.prompt, args.mc_samples,
                       args.mc_seed, bool(args.write_uncertainty), args.top_k, args.top_p)
    if args.write_uncertainty:
        ids, (h_pred, mi) = ids
        write_uncertainty([[inv[i] for i in row] for row in ids], h_pred, mi, args.write_uncertainty)
    text = "".join(" ".join(inv[i] for i in row) + "\n" for row in ids)
    if args.outf == '-':
        sys.stdout.write(text)
    else:
        with open(args.outf, 'w', encoding='utf-8') as f:
            f.write(text)


if __name__ == '__main__':
    main()
