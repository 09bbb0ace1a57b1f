"""Held-out evaluation of a trained language model: loss / perplexity, accuracy and calibration, at mean weights or under the
average of Monte-Carlo weight samples (engine.evaluate_report; the reference evaluates at mean weights inside train.py only).

    python -m bayeslms_amd.evaluate --model-path model.pt --vocabulary words.txt --data test.txt --model Transformer \
        --emsize 512 --nhid 2048 --nlayers 6 --nhead 8 --uncertainty Bayesian --T_bayes_pos FFN --mc-samples 8 \
        --write-report report.json --write-tokens tokens.txt

The model is built from the scorer's flags (compute_sentence_scores.build_models) and loaded as the scorer loads it.  ``--data``
is tokenised as the training corpus is (``<s>`` closes every line, OOV words map to ``<unk>``) and laid out as train.py lays
out its test set: ``--batch-size`` columns of contiguous text walked in windows of ``--seq-len`` rows.  The layout drops the
len(text) % batch-size last tokens and predicts no word across a column's end, so (len(text) // batch-size - 1) * batch-size
words are scored; ``--batch-size 1`` scores all but the first.

One summary line goes to stdout.  ``--write-report PATH`` writes EvalReport.as_dict() as JSON: tokens, skipped, loss, ppl,
accuracy, top5_accuracy, mean_conf, mean_entropy, ece and the [count, mean_conf, accuracy] table of ``--bins`` equal-width
confidence bins; with ``--mc-samples S`` (>= 2) the loss is that of the per-token model average pbar = mean_s p_s, and
sample_loss (each sample's own), sample_loss_mean, mean_h_pred and mean_mi are added.  ``--write-tokens PATH`` writes one line
per scored word in text order, ``word nll conf entropy rank`` and under ``--mc-samples`` also ``h_pred mi`` (%.6g, nats; rank
0: the word was the prediction).

Temperature scaling.  ``--temperature T`` evaluates ``--data`` under the tempered distribution p^(1/T) / Z (for ``--mc-samples``
that of the model average): loss, ppl, mean_conf, mean_entropy, ece, the bins and what ``--write-tokens`` writes as nll, conf
and entropy are then the tempered figures; accuracy, rank and the Monte-Carlo block do not change.  ``--fit-temperature-on PATH``
fits T on that text first (tokenised and laid out like ``--data``; engine.fit_temperature, ``--fit-passes`` search walks) --
the validation text, never ``--data`` itself -- and then evaluates ``--data`` at the fitted T.  With either flag the summary
line and the report gain a ``temperature`` block; without them both are what they were."""
import argparse
import json
import math
import sys

import torch

from . import compute_sentence_scores as S
from . import data as D
from . import engine


def build_parser():
    p = argparse.ArgumentParser(description="Evaluate a trained neural LM on held-out text (MI355X engine): perplexity and calibration.")
    p.add_argument('--model-path', type=str, required=True)
    p.add_argument('--vocabulary', type=str, required=True, help='words.txt (word id per line)')
    p.add_argument('--data', type=str, required=True, help='held-out text, one sentence per line')
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
    p.add_argument('--seq-len', type=int, default=35, help='rows per window (train.py --seq_len)')
    p.add_argument('--batch-size', type=int, default=10, help='columns of contiguous text the stream is cut into')
    p.add_argument('--mc-samples', type=int, default=0,
                   help='S >= 2: score under the average of S Monte-Carlo weight samples (0: mean weights)')
    p.add_argument('--mc-seed', type=int, default=1111, help='key of the weight samples (the n-best scorer\'s default)')
    p.add_argument('--bins', type=int, default=15, help='equal-width confidence bins of the calibration table')
    p.add_argument('--write-report', type=str, default='', metavar='PATH', help='the report as JSON')
    p.add_argument('--write-tokens', type=str, default='', metavar='PATH',
                   help='one line per scored word in text order: "word nll conf entropy rank", with --mc-samples also "h_pred mi"')
    p.add_argument('--temperature', type=float, default=None, metavar='T',
                   help='evaluate under the tempered distribution p^(1/T) / Z (default: 1, the model as it is)')
    p.add_argument('--fit-temperature-on', type=str, default='', metavar='PATH',
                   help='fit T on this held-out text (the validation text), then evaluate --data at the fitted T')
    p.add_argument('--fit-passes', type=int, default=3, help='search walks of the fit text (1..6), eight temperatures each')
    return p


def check_args(args):
    """Refusals that need neither the input files, the model nor a device."""
    if args.temperature is not None and args.fit_temperature_on:
        raise SystemExit("--temperature and --fit-temperature-on exclude each other: give T or the text to fit it on")
    if args.temperature is not None and not (math.isfinite(args.temperature) and args.temperature > 0):
        raise SystemExit("--temperature must be positive and finite (got %r)" % args.temperature)
    if not 1 <= args.fit_passes <= 6:
        raise SystemExit("--fit-passes must lie in 1..6 (got %d)" % args.fit_passes)
    if args.mc_samples < 0 or args.mc_samples == 1 or args.mc_samples > 64:
        raise SystemExit("--mc-samples must be 0 (mean weights) or lie in 2..64, the most one decoder launch averages (got %d)" % args.mc_samples)
    if args.seq_len < 1 or args.batch_size < 1 or args.bins < 1:
        raise SystemExit("--seq-len, --batch-size and --bins must be positive")


def summary_line(rep):
    line = "| evaluate | tokens %d | skipped %d | loss %.4f | ppl %.2f | accuracy %.4f | top5 %.4f | ece %.4f" % (
        rep.tokens, rep.skipped, rep.loss, rep.ppl, rep.accuracy, rep.top5_accuracy, rep.ece)
    if rep.mc_samples:
        line += " | mc samples %d | sample loss %.4f | h_pred %.4f | mi %.4f" % (
            rep.mc_samples, rep.sample_loss_mean, rep.mean_h_pred, rep.mean_mi)
    t = rep.temperature
    if t:
        line += " | temperature %.4f" % t["temperature"]
        if t["fitted_on"]:
            line += " | fit loss %.4f -> %.4f | ece %.4f -> %.4f" % (t["loss_before"], t["loss_after"], t["ece_before"], t["ece_after"])
    return line


def write_tokens(rep, words, path):
    """--write-tokens: ``words[id]`` of every scored target and its figures, text order, skipped tokens left out."""
    t = rep.per_token
    cols = [t[k] for k in ("nll", "conf", "entropy")]
    extra = [t[k] for k in ("h_pred", "mi")] if rep.mc_samples else []
    V = len(words)
    with open(path, 'w', encoding='utf-8') as f:
        for i, w in enumerate(t["tgt"]):
            if 0 <= w < V:
                f.write("%s %s %d%s\n" % (words[w], " ".join("%.6g" % float(c[i]) for c in cols), int(t["rank"][i]),
                                          "".join(" %.6g" % float(c[i]) for c in extra)))


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_args(args)
    if not torch.cuda.is_available():
        raise SystemExit("bayeslms_amd evaluation needs an MI355X: there is no CPU path")
    corpus = D.Corpus.__new__(D.Corpus)  # the vocabulary and one text, tokenised as Corpus tokenises its three
    corpus.dictionary = D.Dictionary()
    corpus.dictionary.read_vocab(args.vocabulary)
    text = corpus.tokenize(args.data)
    if len(text) // args.batch_size < 2:
        raise SystemExit("--data holds %d tokens: fewer than two rows of --batch-size %d columns" % (len(text), args.batch_size))
    fit_text = None
    if args.fit_temperature_on:
        fit_text = corpus.tokenize(args.fit_temperature_on)
        if len(fit_text) // args.batch_size < 2:
            raise SystemExit("--fit-temperature-on holds %d tokens: fewer than two rows of --batch-size %d columns"
                             % (len(fit_text), args.batch_size))
    args.interpolation_flag = 0
    model, _ = S.build_models(args, len(corpus.dictionary))
    S.load_partial(model, args.model_path)
    device = torch.device("cuda", torch.cuda.current_device())
    model = model.to(device).eval()
    temperature, fit = (1.0 if args.temperature is None else args.temperature), None
    if args.fit_temperature_on:
        fit = engine.fit_temperature(model, D.batchify(fit_text, args.batch_size, device), args.seq_len, mc_samples=args.mc_samples,
                                     seed=args.mc_seed, bins=args.bins, passes=args.fit_passes)
        temperature = fit.temperature
        if fit.at_bound:
            print("warning: the fit on %s ended at the search's bound, temperature %.4f: the loss still falls there, so this is no "
                  "minimiser (a model that knows nothing of this text?)" % (args.fit_temperature_on, temperature), file=sys.stderr)
    rep = engine.evaluate_report(model, D.batchify(text, args.batch_size, device), args.seq_len, mc_samples=args.mc_samples,
                                 seed=args.mc_seed, bins=args.bins, keep_tokens=bool(args.write_tokens), temperature=temperature)
    if fit is not None:  # also when the fit gave exactly 1
        rep.temperature = engine.temperature_block(fit.beta, args.fit_temperature_on, fit.at_bound, fit.before, fit.after, fit.curve)
    print(summary_line(rep), flush=True)
    if args.write_report:
        with open(args.write_report, 'w') as f:
            json.dump(rep.as_dict(), f)
    if args.write_tokens:
        write_tokens(rep, corpus.dictionary.idx2word, args.write_tokens)
    return rep


if __name__ == '__main__':
    main()
