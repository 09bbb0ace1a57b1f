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
line and the report gain a ``temperature`` block; without them both are what they were.

Neural cache.  ``--cache-window N`` also scores ``--data`` with the continuous neural cache (engine.evaluate_cache: a pointer over
the N decoder-input rows before each word, mixed into the model's distribution with weight lambda): either at the given
``--cache-theta`` and ``--cache-lambda``, or at the pair that ``--fit-cache-on PATH`` finds on that text first (engine.fit_cache,
``--cache-fit-passes`` launches of eight thetas on one walk of it).  The summary line gains ``| cache window ... theta ... lambda
... | loss a -> b | ppl a -> b | hit ...`` and the report a ``cache`` block (CacheReport.as_dict, plus ``fitted_on``,
``at_bound``, ``fit_loss_before``, ``fit_loss_after`` and ``curve`` after a fit); every other figure stays the model's own.  The
cache runs at mean weights and at temperature 1: ``--mc-samples``, ``--temperature`` and ``--fit-temperature-on`` are refused with
it.  Without ``--cache-window`` the line and the report are what they were.

Dynamic evaluation.  ``--dyneval-lr ETA --dyneval-decay LAMBDA`` also scores ``--data`` with the weights adapting to it
(engine.evaluate_dynamic: the text window by window, one gradient step on each window after it was scored, pulled back towards the
trained weights), or ``--fit-dyneval-on PATH --dyneval-lr-grid a,b,c --dyneval-decay-grid a,b,c`` picks the pair on that text
first (engine.fit_dyneval, a plain grid over its first ``--dyneval-fit-windows`` windows).  ``--dyneval-stats-on PATH`` selects the
rms rule: the step of every weight is scaled by the root mean square of its gradient over the first ``--dyneval-stats-windows``
windows of that text (the training text).  The summary line gains ``| dyneval rule ... lr ... decay ... | loss a -> b | ppl a ->
b`` and the report a ``dyneval`` block (DynEvalReport.as_dict, ``base_loss`` / ``base_ppl`` of the static report, and
``fitted_on``, ``fit_loss_before``, ``fit_loss_after`` and ``curve`` after a fit); every other figure, ``--write-tokens`` included,
stays the static model's.  Refused with it: ``--mc-samples``, ``--temperature``, ``--fit-temperature-on``, ``--cache-window``.
Without these flags the line and the report are what they were.

SWAG.  ``--swag PATH --swag-samples S`` evaluates ``--data`` under the average of S (2..64) weight samples of the SWAG posterior
that ``python -m bayeslms_amd.train --swag-save PATH`` wrote (engine.evaluate_swag; ``--swag-scale`` c, default 0.5,
``--swag-diag 1`` for the diagonal form, ``--mc-seed`` keys the samples); any model family, ``--uncertainty none`` included.
``--swag-samples 0`` evaluates the SWA mean through the ordinary mean-weight report.  ``--temperature`` is honoured.  The summary
line gains ``| swag n ... rank ... scale ... samples ...`` and the report a ``swag`` block.  Refused beside ``--swag``:
``--mc-samples``, ``--fit-temperature-on``, ``--cache-window`` and the dyneval flags.  Without ``--swag`` the line and the report
are what they were.

Laplace.  ``--laplace PATH`` evaluates ``--data`` under the last-layer Laplace posterior of the decoder saved there
(engine.evaluate_laplace; bayeslms_amd/laplace.py), ``--laplace-fit-on train.txt [--laplace-fit-windows N] [--laplace-save PATH]``
fits one first (engine.fit_laplace: one pass over that text, no retraining, any checkpoint).  The prior precision is
``--laplace-prior-precision TAU`` in (0, inf], or the entry of ``--laplace-prior-grid a,b,c`` (1..8 finite values, and always
inf, the model itself) with the lowest loss on ``--fit-laplace-prior-on valid.txt`` (engine.fit_laplace_prior, one walk).
``--laplace-link probit|expexp|mc`` picks the link from logit mean and variance to a distribution (default probit; mc needs
``--laplace-samples`` 2..32, keyed by ``--mc-seed``, and adds the Monte-Carlo block).  The summary line gains ``| laplace tokens ...
prior ... link ... [samples ...]`` and, after a prior fit, ``| fit loss a -> b`` of the fit text; the report gains a ``laplace``
block, in which an infinite prior precision is written as the string ``"inf"`` (JSON has no number for it).  Refused beside
these flags: ``--mc-samples``, ``--swag``, ``--cache-window``, the dyneval flags, ``--fit-temperature-on`` and a ``--temperature``
other than 1.  Without them the line and the report are what they were.

Sample banks and ensembles.  ``--sample-bank PATH [--bank-samples S]`` evaluates ``--data`` under the average of the latest S
(default all) weight samples in the bank that ``python -m bayeslms_amd.train --sgmcmc-save PATH`` wrote, ``--ensemble
a.pt,b.pt,...`` under the average of 2..64 checkpoints of the ``--model-path`` architecture (a deep ensemble; ``--model-path`` may
be one of them) -- both through engine.evaluate_samples, the walk of evaluate_swag.  ``--temperature`` is honoured.  The summary
line gains ``| samples kind ... n ...`` and the report a ``samples`` block.  Refused beside either: ``--mc-samples``, ``--swag``,
the Laplace flags, ``--cache-window``, the dyneval flags and ``--fit-temperature-on``.  Without them the line and the report are
what they were."""
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
    p.add_argument('--cache-window', type=int, default=None, metavar='N',
                   help='also score --data with the neural cache over the N rows before each word')
    p.add_argument('--cache-theta', type=float, default=None, metavar='THETA', help='sharpness of the pointer (with --cache-lambda)')
    p.add_argument('--cache-lambda', type=float, default=None, metavar='LAMBDA', help='weight of the cache in the mix, in [0, 1)')
    p.add_argument('--fit-cache-on', type=str, default='', metavar='PATH',
                   help='fit theta and lambda on this held-out text (the validation text), then score --data with them')
    p.add_argument('--cache-fit-passes', type=int, default=3, help='search launches of the cache fit (1..6), eight thetas each')
    p.add_argument('--dyneval-lr', type=float, default=None, metavar='ETA',
                   help='also score --data under dynamic evaluation with this learning rate (with --dyneval-decay)')
    p.add_argument('--dyneval-decay', type=float, default=None, metavar='LAMBDA', help='pull of the weights back towards the trained ones')
    p.add_argument('--dyneval-epsilon', type=float, default=0.01, metavar='EPS',
                   help='rms rule: floor of the gradient scale, relative to the mean scale (default 0.01; nobody has measured '
                        'this default here)')
    p.add_argument('--dyneval-stats-on', type=str, default='', metavar='PATH',
                   help='the rms rule: gradient statistics from this text (the training text); without it the sgd rule')
    p.add_argument('--dyneval-stats-windows', type=int, default=100, metavar='W', help='windows of --dyneval-stats-on that are read')
    p.add_argument('--fit-dyneval-on', type=str, default='', metavar='PATH',
                   help='pick the learning rate and decay on this held-out text (the validation text) from the two grids')
    p.add_argument('--dyneval-lr-grid', type=str, default='', metavar='a,b,c')
    p.add_argument('--dyneval-decay-grid', type=str, default='', metavar='a,b,c')
    p.add_argument('--dyneval-fit-windows', type=int, default=None, metavar='N', help='windows of --fit-dyneval-on a candidate walks (default all)')
    p.add_argument('--swag', type=str, default='', metavar='PATH',
                   help='evaluate under the SWAG posterior that train --swag-save wrote (with --swag-samples)')
    p.add_argument('--swag-samples', type=int, default=None, metavar='S',
                   help='with --swag: 2..64 weight samples whose distributions are averaged; 0: the SWA mean alone')
    p.add_argument('--swag-scale', type=float, default=None, metavar='C',
                   help='with --swag: the scale of the sampled covariance (default 0.5, the value of Maddox et al. 2019; unmeasured here)')
    p.add_argument('--swag-diag', type=int, default=None, choices=[0, 1], help='with --swag: 1 = the diagonal form, no low-rank term')
    p.add_argument('--laplace', type=str, default='', metavar='PATH', help='evaluate under the last-layer Laplace posterior saved there')
    p.add_argument('--laplace-fit-on', type=str, default='', metavar='PATH',
                   help='fit the Laplace posterior of the decoder on this text (the training text), then evaluate --data under it')
    p.add_argument('--laplace-fit-windows', type=int, default=None, metavar='N', help='windows of --laplace-fit-on that are read (default all)')
    p.add_argument('--laplace-save', type=str, default='', metavar='PATH', help='write the fitted posterior there')
    p.add_argument('--laplace-prior-precision', type=float, default=None, metavar='TAU', help='precision of the prior N(0, 1/TAU), in (0, inf]')
    p.add_argument('--fit-laplace-prior-on', type=str, default='', metavar='PATH',
                   help='pick the prior precision on this held-out text (the validation text) from --laplace-prior-grid')
    p.add_argument('--laplace-prior-grid', type=str, default='', metavar='a,b,c', help='1..8 finite prior precisions')
    p.add_argument('--laplace-link', type=str, default=None, choices=['probit', 'expexp', 'mc'],
                   help='from logit mean and variance to a distribution (default probit)')
    p.add_argument('--laplace-samples', type=int, default=None, metavar='S', help='with --laplace-link mc: 2..32 logit samples (--mc-seed keys them)')
    p.add_argument('--sample-bank', type=str, default='', metavar='PATH',
                   help='evaluate under the average of the weight samples in the bank that train --sgmcmc-save wrote')
    p.add_argument('--bank-samples', type=int, default=None, metavar='S',
                   help='with --sample-bank: the latest S vectors of the bank, 2..64 (default: all it holds)')
    p.add_argument('--ensemble', type=str, default='', metavar='a.pt,b.pt,...',
                   help='evaluate under the average of 2..64 checkpoints of the --model-path architecture (a deep ensemble); '
                        '--model-path may be one of them')
    return p


def check_samples_args(args):
    """The refusals of --sample-bank / --ensemble: before any file or device is touched."""
    if not (args.sample_bank or args.ensemble):
        if args.bank_samples is not None:
            raise SystemExit("--bank-samples needs --sample-bank")
        return
    if args.sample_bank and args.ensemble:
        raise SystemExit("--sample-bank and --ensemble exclude each other: one set of weight vectors per run")
    what = "--sample-bank" if args.sample_bank else "--ensemble"
    if args.ensemble:
        if args.bank_samples is not None:
            raise SystemExit("--bank-samples needs --sample-bank (an ensemble is evaluated whole)")
        n = len(ensemble_paths(args.ensemble))
        if not 2 <= n <= 64:
            raise SystemExit("--ensemble takes 2..64 checkpoints separated by commas (got %d)" % n)
    elif args.bank_samples is not None and not 2 <= args.bank_samples <= 64:
        raise SystemExit("--bank-samples must lie in 2..64 (got %d)" % args.bank_samples)
    if args.mc_samples:
        raise SystemExit("%s with --mc-samples: the weight vectors are the Monte-Carlo samples of this run" % what)
    if args.swag:
        raise SystemExit("%s with --swag: one source of weight samples per run" % what)
    if args.laplace or args.laplace_fit_on:
        raise SystemExit("%s with the Laplace flags: the Laplace posterior stands at one set of weights" % what)
    if args.cache_window is not None:
        raise SystemExit("%s with --cache-window: the cache runs at the model's own mean weights" % what)
    if args.dyneval_lr is not None or args.dyneval_decay is not None or args.fit_dyneval_on:
        raise SystemExit("%s with dynamic evaluation: the two together are not built" % what)
    if args.fit_temperature_on:
        raise SystemExit("%s with --fit-temperature-on: fitting a temperature under a bank is not built (--temperature T is honoured)" % what)


def ensemble_paths(text):
    return [p.strip() for p in text.split(",") if p.strip()]


def laplace_grid(text):
    """"a,b,c" -> [a, b, c]: 1..8 positive finite numbers"""
    try:
        vals = [float(v) for v in text.split(",") if v.strip()]
    except ValueError:
        raise SystemExit("--laplace-prior-grid must be numbers separated by commas (got %r)" % text)
    if not 1 <= len(vals) <= engine.LAPLACE_GRID_MAX or not all(math.isfinite(v) and v > 0 for v in vals):
        raise SystemExit("--laplace-prior-grid needs 1..%d values, each positive and finite (got %r)" % (engine.LAPLACE_GRID_MAX, text))
    return vals


def check_laplace_args(args):
    """The Laplace flags' refusals: before any file or device is touched."""
    on = bool(args.laplace or args.laplace_fit_on)
    if not on:
        for flag, v in (("--laplace-fit-windows", args.laplace_fit_windows), ("--laplace-save", args.laplace_save or None),
                        ("--laplace-prior-precision", args.laplace_prior_precision),
                        ("--fit-laplace-prior-on", args.fit_laplace_prior_on or None),
                        ("--laplace-prior-grid", args.laplace_prior_grid or None), ("--laplace-link", args.laplace_link),
                        ("--laplace-samples", args.laplace_samples)):
            if v is not None:
                raise SystemExit("%s needs --laplace or --laplace-fit-on" % flag)
        return
    if args.laplace and args.laplace_fit_on:
        raise SystemExit("--laplace and --laplace-fit-on exclude each other: load a posterior or fit one")
    if not args.laplace_fit_on and (args.laplace_fit_windows is not None or args.laplace_save):
        raise SystemExit("--laplace-fit-windows and --laplace-save need --laplace-fit-on")
    if args.laplace_fit_windows is not None and args.laplace_fit_windows < 1:
        raise SystemExit("--laplace-fit-windows must be at least 1 (got %d)" % args.laplace_fit_windows)
    if bool(args.fit_laplace_prior_on) != bool(args.laplace_prior_grid):
        raise SystemExit("--fit-laplace-prior-on and --laplace-prior-grid go together")
    if args.fit_laplace_prior_on and args.laplace_prior_precision is not None:
        raise SystemExit("--fit-laplace-prior-on and --laplace-prior-precision exclude each other: give tau or the text to pick it on")
    if not args.fit_laplace_prior_on and args.laplace_prior_precision is None:
        raise SystemExit("a Laplace posterior needs its prior: --laplace-prior-precision TAU, or --fit-laplace-prior-on with --laplace-prior-grid")
    if args.laplace_prior_precision is not None and not args.laplace_prior_precision > 0:
        raise SystemExit("--laplace-prior-precision must lie in (0, inf] (got %r)" % args.laplace_prior_precision)
    if args.laplace_prior_grid:
        laplace_grid(args.laplace_prior_grid)
    link, S = args.laplace_link or "probit", args.laplace_samples or 0
    if link == "mc" and not 2 <= S <= 32:
        raise SystemExit("--laplace-link mc needs --laplace-samples in 2..32 (got %r)" % args.laplace_samples)
    if link != "mc" and args.laplace_samples is not None:
        raise SystemExit("--laplace-samples with --laplace-link %s: the closed-form links draw no sample" % link)
    if args.mc_samples:
        raise SystemExit("Laplace with --mc-samples: the posterior stands at the mean weights; its own samples are --laplace-samples")
    if args.swag:
        raise SystemExit("Laplace with --swag: two posteriors over the same decoder; the two together are not built")
    if args.cache_window is not None:
        raise SystemExit("Laplace with --cache-window: the cache mixes with the model's own distribution")
    if args.dyneval_lr is not None or args.dyneval_decay is not None or args.fit_dyneval_on:
        raise SystemExit("Laplace with dynamic evaluation: the curvature was fitted at the trained weights, which the update moves")
    if args.fit_temperature_on:
        raise SystemExit("Laplace with --fit-temperature-on: a temperature on top of the Laplace predictive is not built")
    if args.temperature is not None and args.temperature != 1.0:
        raise SystemExit("Laplace with --temperature %r: a temperature on top of the Laplace predictive is not built" % args.temperature)


def check_swag_args(args):
    """The SWAG flags' refusals: before any file or device is touched."""
    if not args.swag:
        for flag, v in (("--swag-samples", args.swag_samples), ("--swag-scale", args.swag_scale), ("--swag-diag", args.swag_diag)):
            if v is not None:
                raise SystemExit("%s needs --swag" % flag)
        return
    if args.swag_samples is None:
        raise SystemExit("--swag needs --swag-samples (2..64 samples, or 0 for the SWA mean)")
    S = args.swag_samples
    if S != 0 and not 2 <= S <= 64:
        raise SystemExit("--swag-samples must be 0 (the SWA mean) or lie in 2..64 (got %d)" % S)
    if S == 0 and (args.swag_scale is not None or args.swag_diag is not None):
        raise SystemExit("--swag-scale and --swag-diag shape the samples: --swag-samples 0 draws none")
    if args.swag_scale is not None and not (math.isfinite(args.swag_scale) and args.swag_scale >= 0):
        raise SystemExit("--swag-scale must be finite and >= 0 (got %r)" % args.swag_scale)
    if args.mc_samples:
        raise SystemExit("--swag with --mc-samples: the SWAG samples are the Monte-Carlo samples of this run (--swag-samples)")
    if args.fit_temperature_on:
        raise SystemExit("--swag with --fit-temperature-on: fitting a temperature under SWAG is not built (--temperature T is honoured)")
    if args.cache_window is not None:
        raise SystemExit("--swag with --cache-window: the cache runs at the model's own mean weights")
    if args.dyneval_lr is not None or args.dyneval_decay is not None or args.fit_dyneval_on:
        raise SystemExit("--swag with dynamic evaluation: the two together are not built")


def dyneval_grid(text, flag):
    """"a,b,c" -> [a, b, c]: finite numbers >= 0, at least one"""
    try:
        vals = [float(v) for v in text.split(",") if v.strip()]
    except ValueError:
        raise SystemExit("%s must be numbers separated by commas (got %r)" % (flag, text))
    if not vals or not all(math.isfinite(v) and v >= 0 for v in vals):
        raise SystemExit("%s needs at least one value, each finite and >= 0 (got %r)" % (flag, text))
    return vals


def check_dyneval_args(args):
    """The dynamic-evaluation flags' refusals: before any file or device is touched."""
    given = args.dyneval_lr is not None or args.dyneval_decay is not None
    fit = bool(args.fit_dyneval_on)
    if not given and not fit:
        if args.dyneval_stats_on or args.dyneval_lr_grid or args.dyneval_decay_grid or args.dyneval_fit_windows is not None:
            raise SystemExit("--dyneval-stats-on, --dyneval-lr-grid, --dyneval-decay-grid and --dyneval-fit-windows need "
                             "--dyneval-lr with --dyneval-decay, or --fit-dyneval-on")
        return
    if fit and given:
        raise SystemExit("--fit-dyneval-on and --dyneval-lr / --dyneval-decay exclude each other: give the values or the text to fit them on")
    if fit and not (args.dyneval_lr_grid and args.dyneval_decay_grid):
        raise SystemExit("--fit-dyneval-on needs --dyneval-lr-grid and --dyneval-decay-grid")
    if not fit and (args.dyneval_lr_grid or args.dyneval_decay_grid or args.dyneval_fit_windows is not None):
        raise SystemExit("--dyneval-lr-grid, --dyneval-decay-grid and --dyneval-fit-windows need --fit-dyneval-on")
    if not fit and (args.dyneval_lr is None or args.dyneval_decay is None):
        raise SystemExit("--dyneval-lr and --dyneval-decay go together")
    if args.mc_samples:
        raise SystemExit("dynamic evaluation with --mc-samples: the update moves the mean weights, it runs at mean weights")
    if args.temperature is not None or args.fit_temperature_on:
        raise SystemExit("dynamic evaluation with --temperature / --fit-temperature-on: the gradient step is taken on the untempered NLL")
    if args.cache_window is not None:
        raise SystemExit("dynamic evaluation with --cache-window: the two together are not built")
    for flag, v in (("--dyneval-lr", args.dyneval_lr), ("--dyneval-decay", args.dyneval_decay), ("--dyneval-epsilon", args.dyneval_epsilon)):
        if v is not None and not (math.isfinite(v) and v >= 0):
            raise SystemExit("%s must be finite and >= 0 (got %r)" % (flag, v))
    if fit:
        dyneval_grid(args.dyneval_lr_grid, "--dyneval-lr-grid")
        dyneval_grid(args.dyneval_decay_grid, "--dyneval-decay-grid")
    if args.dyneval_stats_windows < 1:
        raise SystemExit("--dyneval-stats-windows must be at least 1 (got %d)" % args.dyneval_stats_windows)
    if args.dyneval_fit_windows is not None and args.dyneval_fit_windows < 1:
        raise SystemExit("--dyneval-fit-windows must be at least 1 (got %d)" % args.dyneval_fit_windows)


def dyneval_block(rep, base, fit=None, fitted_on=None):
    """The ``dyneval`` block of the report: the DynEvalReport ``rep`` beside the static EvalReport ``base``, and the DynEvalFit"""
    d = rep.as_dict()
    d.update(base_loss=base.loss, base_ppl=base.ppl)
    if fit is not None:
        d.update(fitted_on=fitted_on, fit_loss_before=fit.loss_static, fit_loss_after=fit.loss, curve=fit.curve)
    return d


def check_cache_args(args):
    """The cache flags' refusals: before any file or device is touched."""
    given = args.cache_theta is not None or args.cache_lambda is not None
    if args.cache_window is None:
        if given or args.fit_cache_on:
            raise SystemExit("--cache-theta, --cache-lambda and --fit-cache-on need --cache-window")
        return
    if args.cache_window < 1:
        raise SystemExit("--cache-window must be at least 1 (got %d)" % args.cache_window)
    if args.mc_samples:
        raise SystemExit("--cache-window with --mc-samples: the cache runs at mean weights")
    if args.temperature is not None or args.fit_temperature_on:
        raise SystemExit("--cache-window with --temperature / --fit-temperature-on: the cache mixes with the untempered distribution")
    if args.fit_cache_on and given:
        raise SystemExit("--fit-cache-on and --cache-theta / --cache-lambda exclude each other: give the values or the text to fit them on")
    if not args.fit_cache_on and (args.cache_theta is None or args.cache_lambda is None):
        raise SystemExit("--cache-window needs --cache-theta together with --cache-lambda, or --fit-cache-on")
    if given and not (math.isfinite(args.cache_theta) and args.cache_theta >= 0):
        raise SystemExit("--cache-theta must be finite and >= 0 (got %r)" % args.cache_theta)
    if given and not 0 <= args.cache_lambda < 1:
        raise SystemExit("--cache-lambda must lie in [0, 1) (got %r)" % args.cache_lambda)
    if not 1 <= args.cache_fit_passes <= 6:
        raise SystemExit("--cache-fit-passes must lie in 1..6 (got %d)" % args.cache_fit_passes)


def check_args(args):
    """Refusals that need neither the input files, the model nor a device."""
    check_samples_args(args)
    check_cache_args(args)
    check_dyneval_args(args)
    check_swag_args(args)
    check_laplace_args(args)
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
    c = rep.cache
    if c:
        line += " | cache window %d theta %.6g lambda %.4f | loss %.4f -> %.4f | ppl %.2f -> %.2f | hit %.4f" % (
            c["window"], c["theta"], c["lam"], c["base_loss"], c["loss"], c["base_ppl"], c["ppl"], c["cache_hit_rate"])
    w = rep.swag
    if w:
        line += " | swag n %d rank %d scale %.6g samples %d" % (w["n"], w["rank"], w["scale"], w["samples"])
    b = rep.samples
    if b:
        line += " | samples kind %s n %d" % (b["kind"], b["n"])
    lp = rep.laplace
    if lp:
        line += " | laplace tokens %d prior %.6g link %s" % (lp["tokens"], lp["prior_precision"], lp["link"])
        if lp["samples"]:
            line += " samples %d" % lp["samples"]
        if lp.get("fitted_on"):
            line += " | fit loss %.4f -> %.4f" % (lp["fit_loss_before"], lp["fit_loss_after"])
    d = rep.dyneval
    if d:
        line += " | dyneval rule %s lr %.6g decay %.6g | loss %.4f -> %.4f | ppl %.2f -> %.2f" % (
            d["rule"], d["lr"], d["decay"], d["base_loss"], d["loss"], d["base_ppl"], d["ppl"])
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
    cache_fit_text = None
    if args.fit_cache_on:
        cache_fit_text = corpus.tokenize(args.fit_cache_on)
        if len(cache_fit_text) // args.batch_size < 2:
            raise SystemExit("--fit-cache-on holds %d tokens: fewer than two rows of --batch-size %d columns"
                             % (len(cache_fit_text), args.batch_size))
    dyn_texts = {}
    for flag, path in (("--dyneval-stats-on", args.dyneval_stats_on), ("--fit-dyneval-on", args.fit_dyneval_on)):
        if path:
            dyn_texts[flag] = corpus.tokenize(path)
            if len(dyn_texts[flag]) // args.batch_size < 2:
                raise SystemExit("%s holds %d tokens: fewer than two rows of --batch-size %d columns"
                                 % (flag, len(dyn_texts[flag]), args.batch_size))
    args.interpolation_flag = 0
    model, _ = S.build_models(args, len(corpus.dictionary))
    S.load_partial(model, args.model_path)
    device = torch.device("cuda", torch.cuda.current_device())
    model = model.to(device).eval()
    temperature, fit = (1.0 if args.temperature is None else args.temperature), None
    if args.swag:
        return swag_main(args, model, corpus, text, device, temperature)
    if args.sample_bank or args.ensemble:
        return samples_main(args, model, corpus, text, device, temperature)
    if args.laplace or args.laplace_fit_on:
        return laplace_main(args, model, corpus, text, device)
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
    if args.cache_window is not None:
        theta, lam, cfit = args.cache_theta, args.cache_lambda, None
        if args.fit_cache_on:
            cfit = engine.fit_cache(model, D.batchify(cache_fit_text, args.batch_size, device), args.seq_len, args.cache_window,
                                    passes=args.cache_fit_passes)
            theta, lam = cfit.theta, cfit.lam
            if cfit.at_bound:
                print("warning: the cache fit on %s ended at a bound of its search, theta %.6g lambda %.4f: the loss may still fall "
                      "beyond it" % (args.fit_cache_on, theta, lam), file=sys.stderr)
        rep.cache = engine.evaluate_cache(model, D.batchify(text, args.batch_size, device), args.seq_len, args.cache_window, theta,
                                          lam).as_dict()
        if cfit is not None:
            rep.cache.update(fitted_on=args.fit_cache_on, at_bound=cfit.at_bound, fit_loss_before=cfit.loss_before,
                             fit_loss_after=cfit.loss_after, curve=cfit.curve)
    if args.dyneval_lr is not None or args.fit_dyneval_on:
        lr, decay, stats, dfit = args.dyneval_lr, args.dyneval_decay, None, None
        if args.dyneval_stats_on:
            stats = engine.dyneval_stats(model, D.batchify(dyn_texts["--dyneval-stats-on"], args.batch_size, device), args.seq_len,
                                         args.dyneval_stats_windows)
        if args.fit_dyneval_on:
            dfit = engine.fit_dyneval(model, D.batchify(dyn_texts["--fit-dyneval-on"], args.batch_size, device), args.seq_len,
                                      dyneval_grid(args.dyneval_lr_grid, "--dyneval-lr-grid"),
                                      dyneval_grid(args.dyneval_decay_grid, "--dyneval-decay-grid"), stats=stats,
                                      eps=args.dyneval_epsilon, max_windows=args.dyneval_fit_windows)
            lr, decay = dfit.lr, dfit.decay
        dyn = engine.evaluate_dynamic(model, D.batchify(text, args.batch_size, device), args.seq_len, lr, decay, stats=stats,
                                      eps=args.dyneval_epsilon)
        rep.dyneval = dyneval_block(dyn, rep, dfit, args.fit_dyneval_on)
    print(summary_line(rep), flush=True)
    if args.write_report:
        with open(args.write_report, 'w') as f:
            json.dump(rep.as_dict(), f)
    if args.write_tokens:
        write_tokens(rep, corpus.dictionary.idx2word, args.write_tokens)
    return rep


def swag_main(args, model, corpus, text, device, temperature):
    """--swag: the report under the posterior's samples, or, --swag-samples 0, the mean-weight report of the SWA weights"""
    from . import swag
    from ._lib import BayesLMError
    try:
        posterior = swag.SwagPosterior.load(args.swag, device)
        posterior.check(model)
    except BayesLMError as e:
        raise SystemExit("--swag %s: %s" % (args.swag, e))
    source = D.batchify(text, args.batch_size, device)
    scale = 0.5 if args.swag_scale is None else args.swag_scale
    if args.swag_samples == 0:
        model.load_state_dict(posterior.mean_state_dict(model))
        rep = engine.evaluate_report(model, source, args.seq_len, bins=args.bins, keep_tokens=bool(args.write_tokens), temperature=temperature)
        scale = 0.0
    else:
        rep = engine.evaluate_swag(model, source, args.seq_len, posterior, args.swag_samples, seed=args.mc_seed, scale=scale,
                                   diag=bool(args.swag_diag), bins=args.bins, temperature=temperature, keep_tokens=bool(args.write_tokens))
    rep.swag = dict(posterior.describe(), scale=scale, diag=bool(args.swag_diag), samples=args.swag_samples, seed=args.mc_seed,
                    path=args.swag)
    print(summary_line(rep), flush=True)
    if args.write_report:
        with open(args.write_report, 'w') as f:
            json.dump(rep.as_dict(), f)
    if args.write_tokens:
        write_tokens(rep, corpus.dictionary.idx2word, args.write_tokens)
    return rep


def samples_main(args, model, corpus, text, device, temperature):
    """--sample-bank / --ensemble: the report under the average of the bank's weight vectors"""
    from . import sgmcmc
    from ._lib import BayesLMError
    flag, value = ("--sample-bank", args.sample_bank) if args.sample_bank else ("--ensemble", args.ensemble)
    try:
        if args.sample_bank:
            bank = sgmcmc.SampleBank.load(args.sample_bank)
            bank.check(model)
            if args.bank_samples is not None:
                bank = bank.latest(args.bank_samples)
        else:
            bank = sgmcmc.SampleBank.from_checkpoints(model, ensemble_paths(args.ensemble))
        rep = engine.evaluate_samples(model, D.batchify(text, args.batch_size, device), args.seq_len, bank, bins=args.bins,
                                      temperature=temperature, keep_tokens=bool(args.write_tokens))
    except BayesLMError as e:
        raise SystemExit("%s %s: %s" % (flag, value, e))
    rep.samples = dict(bank.describe(), path=value)
    print(summary_line(rep), flush=True)
    if args.write_report:
        with open(args.write_report, 'w') as f:
            json.dump(rep.as_dict(), f)
    if args.write_tokens:
        write_tokens(rep, corpus.dictionary.idx2word, args.write_tokens)
    return rep


def laplace_main(args, model, corpus, text, device):
    """--laplace / --laplace-fit-on: the report under the decoder's last-layer Laplace predictive"""
    from . import laplace
    from ._lib import BayesLMError

    def stream_of(flag, path):
        toks = corpus.tokenize(path)
        if len(toks) // args.batch_size < 2:
            raise SystemExit("%s holds %d tokens: fewer than two rows of --batch-size %d columns" % (flag, len(toks), args.batch_size))
        return D.batchify(toks, args.batch_size, device)

    link, S = args.laplace_link or "probit", args.laplace_samples or 0
    try:
        if args.laplace:
            posterior = laplace.LaplacePosterior.load(args.laplace, device)
            posterior.check(model)  # the walks check again: four small sums on the device each time
        else:
            posterior = engine.fit_laplace(model, stream_of("--laplace-fit-on", args.laplace_fit_on), args.seq_len, args.laplace_fit_windows)
            if args.laplace_save:
                posterior.save(args.laplace_save)
    except BayesLMError as e:
        raise SystemExit("%s %s: %s" % ("--laplace" if args.laplace else "--laplace-fit-on", args.laplace or args.laplace_fit_on, e))
    tau, pfit = args.laplace_prior_precision, None
    if args.fit_laplace_prior_on:
        pfit = engine.fit_laplace_prior(model, stream_of("--fit-laplace-prior-on", args.fit_laplace_prior_on), args.seq_len, posterior,
                                        laplace_grid(args.laplace_prior_grid), link=link, samples=S, seed=args.mc_seed)
        tau = pfit.tau
    rep = engine.evaluate_laplace(model, D.batchify(text, args.batch_size, device), args.seq_len, posterior, tau, link=link, samples=S,
                                  seed=args.mc_seed, bins=args.bins, keep_tokens=bool(args.write_tokens))
    rep.laplace["path"] = args.laplace or args.laplace_save or None
    if pfit is not None:
        rep.laplace.update(fitted_on=args.fit_laplace_prior_on, fit_loss_before=pfit.loss_base, fit_loss_after=pfit.loss, curve=pfit.curve)
    print(summary_line(rep), flush=True)
    if args.write_report:
        d = rep.as_dict()
        d["laplace"] = laplace_block_json(d["laplace"])
        with open(args.write_report, 'w') as f:
            json.dump(d, f)
    if args.write_tokens:
        write_tokens(rep, corpus.dictionary.idx2word, args.write_tokens)
    return rep


def laplace_block_json(block):
    """The ``laplace`` block as JSON takes it: an infinite prior precision (the block's own and the curve's) is the string "inf",
    since JSON has no token for it."""
    def tau(v):
        return "inf" if isinstance(v, float) and math.isinf(v) else v
    out = dict(block, prior_precision=tau(block["prior_precision"]))
    if out.get("curve"):
        out["curve"] = [[tau(t), v] for t, v in out["curve"]]
    return out


if __name__ == '__main__':
    main()
