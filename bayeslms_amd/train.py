#!/usr/bin/env python3
"""Train and evaluate a neural LM -- same command line as the reference's
steps/pytorchnn/train.py (argument names, types, defaults: train.py:28-103; log line formats
:426-430,476-478,544-545; best-checkpoint / LR-halving / early-stop loop :464-519), running on the
HIP engine.  New optional behaviour: launched under ``torchrun`` it trains data-parallel, each rank
owning a slice of the global batch columns (``--batch-size`` stays the GLOBAL batch).

    python -m bayeslms_amd.train --data DIR --model Transformer --emsize 512 --nhid 4096 --nlayers 6 \
        --nhead 8 --uncertainty Bayesian --T_bayes_pos FFN --tied --cuda --save model.pt
"""
import argparse
import math
import os
import random
import time

import torch
import torch.distributed as dist

from ._lib import TOPK_MAX


def build_parser():
    p = argparse.ArgumentParser(description="Train and evaluate a neural language model (MI355X engine).")
    p.add_argument('--data', type=str, default='./data/pytorchnn', help='location of the data corpus')
    p.add_argument('--model', type=str, default='LSTM', help='LSTM or Transformer')
    p.add_argument('--emsize', type=int, default=200)
    p.add_argument('--nhid', type=int, default=200)
    p.add_argument('--nlayers', type=int, default=2)
    p.add_argument('--nhead', type=int, default=2)
    p.add_argument('--uncertainty', type=str, default='none', help='[none | Bayesian | Gaussian | Variational]')
    p.add_argument('--T_bayes_pos', type=str, default='none', help='[none | FFN | MHA | EMB]')
    p.add_argument('--L_bayes_pos', type=int, default=0, help='0 none, 1 input, 2 forget, 3 cell, 4 output gate')
    p.add_argument('--L_gauss_pos', type=str, default='00')
    p.add_argument('--L_v_pos', type=str, default='11')
    p.add_argument('--T_gauss_pos', type=int, default=3)
    p.add_argument('--T_v_pos', type=int, default=0)
    p.add_argument('--mark', type=str, default='none')
    p.add_argument('--lr', type=float, default=0.1)
    p.add_argument('--batch-size', type=int, default=20, metavar='N')
    p.add_argument('--epochs', type=int, default=20)
    p.add_argument('--seq_len', type=int, default=35)
    p.add_argument('--clip', type=float, default=0.25)
    p.add_argument('--dropout', type=float, default=0.2)
    p.add_argument('--tied', action='store_true')
    p.add_argument('--optimizer', type=str, default='SGD')
    p.add_argument('--log-interval', type=int, default=200, metavar='N')
    p.add_argument('--cuda', action='store_true', help='required: the engine has no CPU path')
    p.add_argument('--save', type=str, default='model.pt')
    p.add_argument('--seed', type=int, default=1111)
    p.add_argument('--resume', type=str, default='')
    p.add_argument('--debug', action='store_true')
    p.add_argument('--work_dir', default='TFM', type=str)
    p.add_argument('--prior', default="False", type=str)
    p.add_argument('--prior_path', default='steps/pytorchnn/prior', type=str)
    p.add_argument('--prior2_path', default='steps/pytorchnn/prior/transformer2/', type=str)
    # new, optional
    p.add_argument('--fused-sampling', type=int, default=0, help='1: eps generated inside the GEMM tile loader')
    p.add_argument('--local-reparam', type=int, default=0, choices=[0, 1],
                   help='new, optional: 1 trains the Bayesian feed-forward (--uncertainty Bayesian --T_bayes_pos FFN) with the local '
                        'reparameterisation estimator: noise per row of the batch on the pre-activations instead of one sampled weight '
                        'per step (DESIGN.md section 4).  Every other variational site refuses it; so does --noise-source torch')
    p.add_argument('--gp-sample', type=int, default=0,
                   help='new, optional: 1 raises GPNN.sample (reference model.py:1799 leaves it False and train.py never sets '
                        'it): the GP coefficients / weights of --uncertainty Gaussian are re-sampled every training step')
    p.add_argument('--gemm-mode', type=str, default='f32', choices=['f32', 'bf16x6', 'bf16x3'],
                   help='new, optional: opt-in split-bf16 arithmetic of the GEMM family (DESIGN.md section 7); default fp32 MFMA')
    p.add_argument('--noise-source', type=str, default=None, choices=['philox', 'torch'],
                   help='new, optional: where the noise of a training run comes from (default: BLM_NOISE_SOURCE or philox).  philox: counter-based '
                        'streams keyed by (seed, tensor / site, step), generated inside the kernels.  torch: a parity mode -- every draw the '
                        'reference makes from torch\'s CPU generator (variational eps, GP draws, every dropout mask) is made by the same call in '
                        'the same order and uploaded, the blocks run unfused: a run from the same --seed follows the reference\'s CPU run, '
                        'noise and dropout on')
    p.add_argument('--deterministic', type=int, default=0,
                   help='new, optional: 1 = every reduction of the engine in a fixed order (ops.set_deterministic / BLM_DETERMINISTIC=1): '
                        'two runs from one seed give bit-identical losses and parameters, also under torchrun at the same world size; '
                        'costs about a quarter of the step')
    p.add_argument('--dist-backend', type=str, default='nccl',
                   help='new, optional (under torchrun): torch.distributed backend; nccl = RCCL over xGMI, one GPU per rank; '
                        'gloo lets several ranks rehearse on one GPU')
    p.add_argument('--dist-timeout-s', type=float, default=None,
                   help='new, optional (under torchrun): rendezvous and collective timeout in seconds (default 180, BLM_DIST_TIMEOUT_S): '
                        'a rank that never arrives, or a collective one rank never enters, ends the job instead of hanging it')
    p.add_argument('--dp-overlap', type=int, default=1,
                   help='new, optional: 1 = bucket all-reduces start while backward is still running, 0 = all after backward')
    p.add_argument('--dp-late-rows', type=int, default=1,
                   help='new, optional: 1 = the embedding half of the encoder gradient travels as the compact matrix of the '
                        'rows the global batch touched (engine.LateRows), 0 = dense')
    p.add_argument('--history', type=str, default='',
                   help='new, optional: rank 0 writes what the log lines print with two decimals (interval / valid / test '
                        'loss, LR-halving epochs, ms per batch) at full precision to this JSON file')
    p.add_argument('--test-report', type=str, default='', metavar='PATH',
                   help='new, optional: after the final test pass, write engine.evaluate_report of the test set (loss, perplexity, '
                        'accuracy, calibration; bayeslms_amd.evaluate\'s JSON) to this file.  Single process only')
    p.add_argument('--test-mc-samples', type=int, default=0, metavar='S',
                   help='new, optional (with --test-report): S >= 2 reports the test set under the average of S Monte-Carlo weight '
                        'samples keyed by --seed (0: mean weights)')
    p.add_argument('--distill-from', type=str, default='', metavar='PATH',
                   help='new, optional: train this model as the STUDENT of the frozen model saved at PATH (a state_dict, as --save writes '
                        'it): every batch the teacher\'s next-word distribution is a dense target of the loss (DESIGN.md section 7, '
                        'bayeslms_amd/distill.py).  Validation, checkpoints and the test pass stay hard-label.  Single process only')
    p.add_argument('--distill-weight', type=float, default=None, metavar='L',
                   help='new, optional (with --distill-from): loss = (1 - L) hard-label cross entropy + L cross entropy against the '
                        'teacher, L in [0, 1] (default 0.5)')
    p.add_argument('--distill-mc-samples', type=int, default=0, metavar='S',
                   help='new, optional (with --distill-from): S in 2..64 distils the average of S Monte-Carlo weight samples of the '
                        'teacher (0: the teacher at mean weights)')
    p.add_argument('--distill-mc-seed', type=int, default=1111, metavar='N',
                   help='new, optional (with --distill-from): the key of the teacher\'s weight samples')
    p.add_argument('--distill-teacher-args', type=str, default=None, metavar='"..."',
                   help='new, optional (with --distill-from): the flags that shape the TEACHER, as one string of this command line\'s '
                        'own flags (a checkpoint holds weights, not an architecture).  Only the model-shaping ones are read: %s.  '
                        'Default: the student\'s own' % ", ".join("--" + f for f in TEACHER_FLAGS))
    p.add_argument('--distill-top-k', type=int, default=0, metavar='K',
                   help='new, optional (with --distill-from): train against the K best entries of the teacher per token (1..%d, at '
                        'most the vocabulary) instead of its dense rows: the soft term of a token is weighted by the teacher mass '
                        'its K entries hold and the tail is dropped (0: dense)' % TOPK_MAX)
    p.add_argument('--distill-top-k-renorm', type=int, default=0, choices=[0, 1],
                   help='new, optional (with --distill-top-k): 1 = renormalise the K entries of every token to sum to one')
    p.add_argument('--distill-cache', type=str, default='', metavar='PATH',
                   help='new, optional (with --distill-top-k): keep the teacher\'s top-K targets of the training walk in this file.  '
                        'The first epoch computes and stores them, every later epoch -- and every later run against the same '
                        'teacher, corpus, K and batch shape -- loads them and runs no teacher; a file written for anything else is '
                        'refused')
    p.add_argument('--distill-temperature', type=float, default=1.0, metavar='T',
                   help='new, optional (with --distill-from): the softmax temperature of the soft term, T in [1/16, 16] (Hinton et al. '
                        '2015): the student\'s softmax(logits / T) is trained against the teacher raised to 1 / T and renormalised, '
                        'times T^2; the hard-label term stays at temperature 1.  With --distill-top-k the K entries are renormalised '
                        '(T other than 1 needs --distill-top-k-renorm 1), and one --distill-cache file serves every temperature')
    p.add_argument('--swag-save', type=str, default='', metavar='PATH',
                   help='new, optional: collect a SWAG posterior over all weights from the SGD iterates (bayeslms_amd/swag.py; Maddox et '
                        'al. 2019) and write it to PATH at the end of training; bayeslms_amd.evaluate --swag PATH reads it.  Single '
                        'process only')
    p.add_argument('--swag-start', type=int, default=None, metavar='E',
                   help='new, optional (with --swag-save): the first epoch, 1-based, that collects (default 1)')
    p.add_argument('--swag-every', type=int, default=None, metavar='N',
                   help='new, optional (with --swag-save): 0 = one iterate at each epoch\'s end (the default), else one every N '
                        'optimisation steps from epoch E on')
    p.add_argument('--swag-rank', type=int, default=None, metavar='K',
                   help='new, optional (with --swag-save): deviations kept for the low-rank term, 0..32 (default 20; 0: diagonal only)')
    p.add_argument('--swag-lr', type=float, default=None, metavar='LR',
                   help='new, optional (with --swag-save): from epoch E on the learning rate is this constant and the halving rule is '
                        'suspended (default: the schedule is untouched)')
    p.add_argument('--sgmcmc-save', type=str, default='', metavar='PATH',
                   help='new, optional: from epoch --sgmcmc-start on, replace clip + SGD by a stochastic-gradient MCMC update over all '
                        'weights (bayeslms_amd/sgmcmc.py; Welling and Teh 2011, Li et al. 2016), collect weight samples and write the '
                        'bank to PATH at the end of training; bayeslms_amd.evaluate --sample-bank PATH reads it.  Models without '
                        'variational sites, single process only')
    p.add_argument('--sgmcmc-lr', type=float, default=None, metavar='LR',
                   help='new, required with --sgmcmc-save: the rate of the sampler on the mean loss (eps N / 2 for a Langevin step eps '
                        'over N training tokens); no default can be right')
    p.add_argument('--sgmcmc-rule', type=str, default=None, choices=['sgld', 'psgld'],
                   help='new, optional (with --sgmcmc-save): sgld (the default), or psgld, preconditioned by an RMSprop second moment')
    p.add_argument('--sgmcmc-start', type=int, default=None, metavar='E',
                   help='new, optional (with --sgmcmc-save): the first epoch, 1-based, that samples (default 1); earlier epochs are '
                        'ordinary SGD, the burn-in.  From epoch E on the halving rule is suspended')
    p.add_argument('--sgmcmc-temperature', type=float, default=None, metavar='T',
                   help='new, optional (with --sgmcmc-save): temperature of the chain, >= 0 (default 1: the posterior)')
    p.add_argument('--sgmcmc-prior-precision', type=float, default=None, metavar='TAU',
                   help='new, optional (with --sgmcmc-save): precision of the Gaussian prior, >= 0 (default 1; unmeasured here)')
    p.add_argument('--sgmcmc-every', type=int, default=None, metavar='N',
                   help='new, optional (with --sgmcmc-save): 0 = one sample at each epoch\'s end (the default), else one every N '
                        'optimisation steps from epoch E on')
    p.add_argument('--sgmcmc-keep', type=int, default=None, metavar='K',
                   help='new, optional (with --sgmcmc-save): the bank keeps the latest K samples, 2..64 (default 16)')
    p.add_argument('--sgmcmc-cycles', type=int, default=None, metavar='M',
                   help='new, optional (with --sgmcmc-save): M > 0 = cyclical SG-MCMC (Zhang et al. 2020): the steps from epoch E on '
                        'in M cosine cycles starting at --sgmcmc-lr (default 0: a constant rate, noise throughout)')
    p.add_argument('--sgmcmc-explore', type=float, default=None, metavar='BETA',
                   help='new, optional (with --sgmcmc-cycles): the share of each cycle run without noise and without collecting, '
                        'in [0, 1) (default 0.8)')
    p.add_argument('--sgmcmc-seed', type=int, default=None, metavar='N',
                   help='new, optional (with --sgmcmc-save): the key of the chain\'s noise (default --seed)')
    return p


SGMCMC_FLAGS = ("sgmcmc_save", "sgmcmc_lr", "sgmcmc_rule", "sgmcmc_start", "sgmcmc_temperature", "sgmcmc_prior_precision",
                "sgmcmc_every", "sgmcmc_keep", "sgmcmc_cycles", "sgmcmc_explore", "sgmcmc_seed")


def variational_site_flag(args):
    """The flag that gives the model of ``args`` a variational site, as text, or None"""
    if args.uncertainty == 'none':
        return None
    if args.model == 'Transformer':
        pos = {'Bayesian': 'T_bayes_pos', 'Gaussian': 'T_gauss_pos', 'Variational': 'T_v_pos'}.get(args.uncertainty)
    else:
        pos = {'Bayesian': 'L_bayes_pos', 'Gaussian': 'L_gauss_pos', 'Variational': 'L_v_pos'}.get(args.uncertainty)
    return "--uncertainty %s" % args.uncertainty + ("" if pos is None else " --%s %s" % (pos, getattr(args, pos)))


def take_sgmcmc_args(args, world, swag_on):
    """The --sgmcmc-* flags, taken OUT of ``args`` (a run without them prints the configuration it printed before there were any)
    and refused before anything is loaded -> a namespace (save, lr, rule, start, temperature, prior_precision, every, keep, cycles,
    explore, seed), or None without --sgmcmc-save."""
    got = {f: getattr(args, f) for f in SGMCMC_FLAGS}
    for f in SGMCMC_FLAGS:
        delattr(args, f)
    if not got["sgmcmc_save"]:
        for f in SGMCMC_FLAGS[1:]:
            if got[f] is not None:
                raise SystemExit("--%s needs --sgmcmc-save" % f.replace("_", "-"))
        return None

    def of(name, default):
        return default if got[name] is None else got[name]

    w = argparse.Namespace(save=got["sgmcmc_save"], lr=got["sgmcmc_lr"], rule=of("sgmcmc_rule", "sgld"), start=of("sgmcmc_start", 1),
                           temperature=of("sgmcmc_temperature", 1.0), prior_precision=of("sgmcmc_prior_precision", 1.0),
                           every=of("sgmcmc_every", 0), keep=of("sgmcmc_keep", 16), cycles=of("sgmcmc_cycles", 0),
                           explore=of("sgmcmc_explore", 0.8), seed=of("sgmcmc_seed", args.seed))
    if w.lr is None:
        raise SystemExit("--sgmcmc-save needs --sgmcmc-lr: the rate of the sampler has no default that can be right")
    if not (math.isfinite(w.lr) and w.lr > 0):
        raise SystemExit("--sgmcmc-lr must be positive and finite (got %r)" % w.lr)
    if swag_on:
        raise SystemExit("--sgmcmc-save with --swag-save: SWAG fits the SGD iterates, and under a sampler there are none")
    if args.distill_from:
        raise SystemExit("--sgmcmc-save with --distill-from: sampling a student's weights is not built")
    if world > 1:
        raise SystemExit("--sgmcmc-save runs in a single process: data-parallel sampling is not built (world size %d)" % world)
    if (args.noise_source or os.environ.get("BLM_NOISE_SOURCE", "philox")) == "torch":
        raise SystemExit("--sgmcmc-save with --noise-source torch: the parity mode follows the reference's run, which has no sampler")
    site = variational_site_flag(args)
    if site is not None:
        raise SystemExit("--sgmcmc-save with %s: that site already carries a variational posterior, and two posteriors over the "
                         "same weights are not built; sample a model of --uncertainty none" % site)
    if w.start < 1:
        raise SystemExit("--sgmcmc-start is a 1-based epoch (got %d)" % w.start)
    if w.start > args.epochs:
        raise SystemExit("--sgmcmc-start %d lies beyond --epochs %d: nothing would be sampled" % (w.start, args.epochs))
    if not (math.isfinite(w.temperature) and w.temperature >= 0):
        raise SystemExit("--sgmcmc-temperature must be finite and >= 0 (got %r)" % w.temperature)
    if not (math.isfinite(w.prior_precision) and w.prior_precision >= 0):
        raise SystemExit("--sgmcmc-prior-precision must be finite and >= 0 (got %r)" % w.prior_precision)
    if w.every < 0:
        raise SystemExit("--sgmcmc-every must be 0 (each epoch's end) or a positive number of steps (got %d)" % w.every)
    if not 2 <= w.keep <= 64:
        raise SystemExit("--sgmcmc-keep must lie in 2..64 (got %d)" % w.keep)
    if w.cycles < 0:
        raise SystemExit("--sgmcmc-cycles must be >= 0 (got %d)" % w.cycles)
    if got["sgmcmc_explore"] is not None and not w.cycles:
        raise SystemExit("--sgmcmc-explore needs --sgmcmc-cycles")
    if not 0 <= w.explore < 1:
        raise SystemExit("--sgmcmc-explore must lie in [0, 1) (got %r)" % w.explore)
    return w


SWAG_FLAGS = ("swag_save", "swag_start", "swag_every", "swag_rank", "swag_lr")


def take_swag_args(args, world):
    """The --swag-* flags, taken OUT of ``args`` (a run without them prints the configuration it printed before there were any)
    and refused before anything is loaded -> a namespace (save, start, every, rank, lr), or None without --swag-save."""
    got = {f: getattr(args, f) for f in SWAG_FLAGS}
    for f in SWAG_FLAGS:
        delattr(args, f)
    if not got["swag_save"]:
        for f in SWAG_FLAGS[1:]:
            if got[f] is not None:
                raise SystemExit("--%s needs --swag-save" % f.replace("_", "-"))
        return None
    if world > 1:
        raise SystemExit("--swag-save runs in a single process: data-parallel collection is not built (world size %d)" % world)
    w = argparse.Namespace(save=got["swag_save"], start=1 if got["swag_start"] is None else got["swag_start"],
                           every=got["swag_every"] or 0, rank=20 if got["swag_rank"] is None else got["swag_rank"], lr=got["swag_lr"])
    if w.start < 1:
        raise SystemExit("--swag-start is a 1-based epoch (got %d)" % w.start)
    if w.every < 0:
        raise SystemExit("--swag-every must be 0 (each epoch's end) or a positive number of steps (got %d)" % w.every)
    if not 0 <= w.rank <= 32:
        raise SystemExit("--swag-rank must lie in 0..32 (got %d)" % w.rank)
    if w.lr is not None and not (math.isfinite(w.lr) and w.lr > 0):
        raise SystemExit("--swag-lr must be positive and finite (got %r)" % w.lr)
    if w.start > args.epochs:
        raise SystemExit("--swag-start %d lies beyond --epochs %d: nothing would be collected" % (w.start, args.epochs))
    return w


# the flags build_model reads: what --distill-teacher-args may set for the teacher
TEACHER_FLAGS = ("model", "emsize", "nhid", "nlayers", "nhead", "uncertainty", "T_bayes_pos", "L_bayes_pos", "L_gauss_pos", "L_v_pos",
                 "T_gauss_pos", "T_v_pos", "dropout", "tied")
DISTILL_T_LO, DISTILL_T_HI = 1.0 / 16, 16.0  # --distill-temperature: the default bounds of engine.TemperatureSearch


def check_distill_args(args, world):
    """The --distill-* flags, refused before anything is loaded -> the teacher's model-shaping flags (a namespace), or None."""
    if not args.distill_from:
        for flag, given in (("--distill-weight", args.distill_weight is not None), ("--distill-mc-samples", args.distill_mc_samples != 0),
                            ("--distill-teacher-args", args.distill_teacher_args is not None),
                            ("--distill-top-k", args.distill_top_k != 0), ("--distill-top-k-renorm", args.distill_top_k_renorm != 0),
                            ("--distill-cache", bool(args.distill_cache)), ("--distill-temperature", args.distill_temperature != 1.0)):
            if given:
                raise SystemExit("%s needs --distill-from" % flag)
        return None
    if args.distill_weight is None:
        args.distill_weight = 0.5
    if not 0.0 <= args.distill_weight <= 1.0:
        raise SystemExit("--distill-weight must lie in [0, 1] (got %r)" % args.distill_weight)
    S = args.distill_mc_samples
    if S < 0 or S == 1 or S > 64:
        raise SystemExit("--distill-mc-samples must be 0 (mean weights) or lie in 2..64, the most one decoder launch averages (got %d)" % S)
    if args.distill_top_k == 0:
        for flag, given in (("--distill-top-k-renorm", args.distill_top_k_renorm != 0), ("--distill-cache", bool(args.distill_cache))):
            if given:
                raise SystemExit("%s needs --distill-top-k" % flag)
    elif not 1 <= args.distill_top_k <= TOPK_MAX:
        raise SystemExit("--distill-top-k must lie in 1..%d, the most entries per token the sparse loss takes (got %d)"
                         % (TOPK_MAX, args.distill_top_k))
    T = args.distill_temperature
    if not math.isfinite(T):
        raise SystemExit("--distill-temperature must be a finite number (got %r)" % T)
    if not DISTILL_T_LO <= T <= DISTILL_T_HI:
        raise SystemExit("--distill-temperature must lie in [1/16, 16], the range the evaluation's temperature search covers (got %r)" % T)
    if T != 1.0 and args.distill_top_k and not args.distill_top_k_renorm:
        raise SystemExit("--distill-temperature %r with --distill-top-k needs --distill-top-k-renorm 1: the tempered target is the K "
                         "entries renormalised, and only then does T -> 1 meet the run without the flag" % T)
    if world > 1:
        raise SystemExit("--distill-from runs in a single process: data-parallel distillation is not built (world size %d)" % world)
    if (args.noise_source or os.environ.get("BLM_NOISE_SOURCE", "philox")) == "torch":
        raise SystemExit("--distill-from with --noise-source torch: the parity mode follows the reference's run, which has no teacher")
    shape = argparse.Namespace(**{f: getattr(args, f) for f in TEACHER_FLAGS})
    if args.distill_teacher_args is not None:
        import shlex
        theirs = build_parser().parse_args(shlex.split(args.distill_teacher_args))
        shape = argparse.Namespace(**{f: getattr(theirs, f) for f in TEACHER_FLAGS})
    return shape


def load_teacher_state(args):
    """The teacher's state_dict (on the host) once its vocabulary has been checked against the corpus's words.txt -- before any
    device is touched."""
    from .data import Dictionary
    words = Dictionary()
    words.read_vocab(os.path.join(args.data, "words.txt"))
    sd = torch.load(args.distill_from, map_location='cpu')
    rows = [v.shape[0] for k, v in sd.items() if k in ("decoder.weight", "decoder.bias")] if isinstance(sd, dict) else []
    if not rows:
        raise SystemExit("--distill-from %s: not a state_dict of one of this package's language models (no decoder.weight)" % args.distill_from)
    if rows[0] != len(words):
        raise SystemExit("--distill-from %s: the teacher's vocabulary has %d words, the corpus at %s has %d: a teacher's distribution "
                         "must be over the student's words" % (args.distill_from, rows[0], args.data, len(words)))
    if args.distill_top_k > len(words):
        raise SystemExit("--distill-top-k %d: the vocabulary at %s has %d words only" % (args.distill_top_k, args.data, len(words)))
    return sd


def check_report_args(args, world):
    """--test-report / --test-mc-samples, refused before anything is loaded."""
    if args.test_mc_samples and not args.test_report:
        raise SystemExit("--test-mc-samples needs --test-report")
    if args.test_mc_samples < 0 or args.test_mc_samples == 1 or args.test_mc_samples > 64:
        raise SystemExit("--test-mc-samples must be 0 (mean weights) or lie in 2..64, the most one decoder launch averages (got %d)" % args.test_mc_samples)
    if args.test_report and world > 1:
        raise SystemExit("--test-report runs in a single process: the report is not sharded over ranks (world size %d); "
                         "write it with bayeslms_amd.evaluate from the saved model" % world)


def build_model(args, ntokens):
    """Model dispatch of train.py:193-223.  With ``--uncertainty none`` the reference builds the model TWICE and trains the
    second one (``model_2`` first, train.py:196-199 / :211-214): the first construction is repeated here and dropped, so that
    the same ``--seed`` starts from the same weights (the constructors draw from torch's generator in the reference's order,
    tests/test_init_state_cpu.py)."""
    from . import model as M
    if args.model == 'Transformer':
        if args.uncertainty == 'none':
            M.TransformerModel(ntokens, args.emsize, args.nhead, args.nhid, args.nlayers, args.dropout, "gelu", args.tied)  # model_2
            return M.TransformerModel(ntokens, args.emsize, args.nhead, args.nhid, args.nlayers, args.dropout, "gelu", args.tied)
        if args.uncertainty == 'Bayesian':
            return M.BayesTransformerModel(ntokens, args.emsize, args.nhead, args.nhid, args.nlayers, args.dropout,
                                           args.tied, args.T_bayes_pos)
        if args.uncertainty == 'Gaussian':
            return M.GaussTransformerModel(ntokens, args.emsize, args.nhead, args.nhid, args.nlayers, args.dropout,
                                           args.tied, args.T_gauss_pos)
        if args.uncertainty == 'Variational':
            return M.VTransformerModel(ntokens, args.emsize, args.nhead, args.nhid, args.nlayers, args.dropout,
                                       args.tied, args.T_v_pos)
    else:
        if args.uncertainty == 'none':
            M.RNNModel(args.model, ntokens, args.emsize, args.nhid, args.nlayers, args.dropout, args.tied)  # model_2
            return M.RNNModel(args.model, ntokens, args.emsize, args.nhid, args.nlayers, args.dropout, args.tied)
        if args.uncertainty == 'Bayesian':
            return M.BayesRNNModel(args.model, ntokens, args.emsize, args.nhid, args.nlayers, args.dropout, args.tied,
                                   args.L_bayes_pos)
        if args.uncertainty == 'Gaussian':
            return M.GaussRNNModel(args.model, ntokens, args.emsize, args.nhid, args.nlayers, args.dropout, args.tied,
                                   args.L_gauss_pos)
        if args.uncertainty == 'Variational':
            return M.VariationalRNNModel(args.model, ntokens, args.emsize, args.nhid, args.nlayers, args.dropout,
                                         args.tied, args.L_v_pos)
    raise SystemExit("--model %s --uncertainty %s is not built by this engine yet" % (args.model, args.uncertainty))


def kl_selector(args):
    """Which module's KL train.py adds to the loss for this flag combination (train.py:335-399).
    Returns None or fn(model) -> KL tensor; ``fn.fusable`` marks KLs whose gradient the Bayesian
    wgrad epilogue can add itself."""
    fn = None
    if args.uncertainty == 'Bayesian':
        if args.model == 'LSTM' and 1 <= args.L_bayes_pos <= 5:  # train.py:337
            fn = lambda m: m.rnn.kl_divergence()  # noqa: E731
            fn.fusable = False
        elif args.model == 'Transformer':
            if args.T_bayes_pos == 'FFN':
                fn = lambda m: m.transformerlayers[0].linear2.kl_divergence()  # noqa: E731
                fn.fusable = True
            elif args.T_bayes_pos == 'MHA':
                fn = lambda m: m.transformerlayers[0].self_attn.o_net.kl_divergence()  # noqa: E731
                fn.fusable = True
            elif args.T_bayes_pos == 'EMB':
                fn = lambda m: m.embed_kl_divergence()  # noqa: E731
                fn.fusable = False
    elif args.uncertainty == 'Gaussian' and args.model == 'Transformer' and 1 <= args.T_gauss_pos <= 3:
        fn = lambda m: m.transformerlayers[0].gpnn.kl_divergence()  # noqa: E731
        fn.fusable = False
    elif args.uncertainty == 'Gaussian' and args.model == 'LSTM':
        g = args.L_gauss_pos
        if int(g[0]) > 0 and 0 < int(g[1]) <= 3:  # train.py:367-375
            cells = [0] if len(g) < 3 else ([1] if len(g) == 3 else [0, 1])
            fn = lambda m: sum(m.rnn.rnn[c].gpnn.kl_divergence() for c in cells)  # noqa: E731
            fn.fusable = False
    elif args.uncertainty == 'Variational' and args.model == 'LSTM':
        cells = [c for c in (0, 1) if int(args.L_v_pos[c]) == 1]  # train.py:379-382
        if cells:
            fn = lambda m: sum(m.rnn.rnn[c].vnn.kl_divergence() for c in cells)  # noqa: E731
            fn.fusable = False
    elif args.uncertainty == 'Variational' and args.model == 'Transformer' and int(args.T_v_pos) in (1, 2, 3):
        layers = {1: [0], 2: [1], 3: [0, 1]}[int(args.T_v_pos)]  # train.py:387-396 (raises like the reference)
        fn = lambda m: sum(m.transformerlayers[i].kl_divergence() for i in layers)  # noqa: E731
        fn.fusable = False
    return fn


def _print_coef_mean(args, model, say):
    """train.py:483-494 / :529-540: the per-epoch print of the GP activation-mixture coefficients, averaged
    over units (one value per basis activation)."""
    sd = model.state_dict()
    if args.model == 'Transformer' and args.uncertainty == 'Gaussian' and args.T_gauss_pos <= 3:
        say(sd['transformerlayers.0.gpnn.coef_mean'].mean(dim=1))
    elif args.model == 'LSTM' and args.uncertainty == 'Gaussian' and int(args.L_gauss_pos[1]) <= 3:
        g = args.L_gauss_pos
        cells = [0] if len(g) < 3 else ([1] if len(g) == 3 else [0, 1])
        for c in cells:
            say(sd['rnn.rnn.%d.gpnn.coef_mean' % c].mean(dim=1))


class ValidationSchedule:
    """The end-of-epoch decision of train.py:496-512 -- keep the checkpoint when the validation loss improved, else
    halve the learning rate (fresh SGD, reload the best checkpoint), stop after 8 halvings -- taken ONCE for the job.
    Every rank evaluates the same validation stream, but an under-filled evaluation GEMM sums its K slices with float
    atomics, so two ranks may see losses that differ in the last bits; a rank-local ``val_loss < best_val`` could then
    halve the LR on one rank only, or leave the ranks in different epochs with the next all-reduce hanging.  ``update``
    therefore replaces every rank's value by rank 0's (one 8-byte broadcast per epoch) before it is compared, logged
    or stored, so all ranks walk the same branch by construction."""

    def __init__(self, lr, world=1, device=None, group=None, patience=8):
        self.lr, self.world, self.device, self.group = lr, world, device, group
        self.best_val = None
        self.counter = 0
        self.patience = patience

    def agree(self, value):
        """rank 0's ``value`` on every rank (identity for a single process)."""
        if self.world <= 1:
            return float(value)
        on_dev = dist.get_backend(self.group) == "nccl"
        t = torch.tensor([float(value)], dtype=torch.float64, device=self.device if on_dev else "cpu")
        dist.broadcast(t, src=0, group=self.group)
        return float(t.item())

    def observe(self, val_loss):
        """-> (the job's validation loss, improved): the comparison alone, no halving (a held learning rate, --swag-lr)"""
        val_loss = self.agree(val_loss)
        improved = (not self.best_val) or val_loss < self.best_val  # train.py:497
        if improved:
            self.best_val = val_loss
        return val_loss, improved

    def update(self, val_loss):
        """-> (the job's validation loss, improved, stop).  ``improved`` False means: lr has been halved."""
        val_loss, improved = self.observe(val_loss)
        if not improved:
            self.lr /= 2.
            self.counter += 1
        return val_loss, improved, self.counter == self.patience


def main(argv=None, history=None):
    """``history`` (optional dict) receives what the log lines print with two decimals at full precision:
    interval_loss, valid_loss, halved_epochs, test_loss."""
    args = build_parser().parse_args(argv)
    if args.local_reparam and (args.noise_source or os.environ.get("BLM_NOISE_SOURCE", "philox")) == "torch":
        raise SystemExit("--local-reparam 1 --noise-source torch: the reference has no per-row draw to reproduce "
                         "(local reparameterisation takes the Philox streams only)")
    if history is None:
        history = {}
    history.update({"interval_loss": [], "valid_loss": [], "halved_epochs": [], "test_loss": None, "ms_per_batch": []})
    world = int(os.environ.get("WORLD_SIZE", "1"))
    swag_args = take_swag_args(args, world)
    sg_args = take_sgmcmc_args(args, world, swag_args is not None)
    check_report_args(args, world)
    teacher_shape = check_distill_args(args, world)
    teacher_sd = load_teacher_state(args) if teacher_shape is not None else None
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    is_main = rank == 0
    if world > 1:  # before the first torch.cuda call: the HSA runtime reads its environment when it is initialised
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    def say(*a):
        if is_main:
            print(*a, flush=True)

    random.seed(args.seed)
    torch.manual_seed(args.seed)
    if not args.cuda or not torch.cuda.is_available():
        raise SystemExit("bayeslms_amd.train needs --cuda and an MI355X: there is no CPU path")
    if args.dist_backend != "nccl":
        local = local % max(torch.cuda.device_count(), 1)  # rehearsal: several ranks share a GPU (RCCL refuses that)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        # bounded rendezvous / collective timeout (--dist-timeout-s, BLM_DIST_TIMEOUT_S, 180 s), RCCL's channel count pinned before
        # RCCL reads its environment, `rendezvous ok` / `first all-reduce ok` heartbeats on stderr (engine.init_distributed)
        from .engine import init_distributed
        rccl_env = init_distributed(args.dist_backend, device if args.dist_backend == "nccl" else None, args.dist_timeout_s)
        if rccl_env is not None:
            say("RCCL channels:", rccl_env)

    from . import data as D, engine, ops
    from .model import repackage_hidden
    if args.gemm_mode != 'f32':
        ops.set_gemm_mode(args.gemm_mode)
    if args.deterministic:
        ops.set_deterministic(True)

    say('Configurations')
    for k, v in vars(args).items():
        say(k, v)
    corpus = D.Corpus(args.data)
    say("train set:", len(corpus.train))
    say("valid set:", len(corpus.valid))
    say("test set:", len(corpus.test))
    say("num tokens:", len(corpus.dictionary))
    frac = {"base-0.5set": 2, "base-0.25set": 4, "base-0.1set": 10, "base-0.05set": 20}.get(args.mark, 1)  # train.py:151-165
    pruning_train = int(len(corpus.train) / frac)
    eval_batch_size = 20
    train_data = D.batchify(corpus.train[:pruning_train], args.batch_size, device, rank, world)
    val_data = D.batchify(corpus.valid, eval_batch_size, device)
    test_data = D.batchify(corpus.test, eval_batch_size, device)
    ntokens = len(corpus.dictionary)

    model = build_model(args, ntokens)
    if args.prior == "True":  # partial state-dict load, keys filtered by name (train.py:239-258)
        prior = torch.load(os.path.join(args.prior_path, 'model.pt'), map_location='cpu')
        own = model.state_dict()
        own.update({k: v for k, v in prior.items() if k in own})
        model.load_state_dict(own)
    model = model.to(device)
    model.set_fused_sampling(bool(args.fused_sampling))
    if args.noise_source is not None:
        model.set_noise_source(args.noise_source)
    model.set_local_reparam(bool(args.local_reparam))
    if args.gp_sample:
        from .model import GPNN
        gps = [m for m in model.modules() if isinstance(m, GPNN) and m.draws_noise()]
        if not gps:
            raise SystemExit("--gp-sample 1: this model has no GPNN with Bayesian coefficients or weights")
        for m in gps:
            m.sample = True
    total_params = sum(x.data.nelement() for x in model.parameters())
    say('Args: {}'.format(args))
    say('Model total parameters: {}'.format(total_params))
    say(str(model.transformerlayers if args.model == 'Transformer' else model.rnn))

    teacher, topk, cache = None, 0, None
    if teacher_shape is not None:
        from . import distill
        with torch.random.fork_rng(devices=[]):  # the constructors draw from torch's generator: the student's run does not see it
            teacher_model = build_model(teacher_shape, ntokens)
        try:
            teacher_model.load_state_dict(teacher_sd)
        except RuntimeError as e:
            raise SystemExit("--distill-from %s does not fit the teacher that --distill-teacher-args (default: this run's own flags) "
                             "describes: %s" % (args.distill_from, e))
        teacher_model = teacher_model.to(device).requires_grad_(False)
        try:
            teacher = distill.Teacher(teacher_model, args.distill_mc_samples, args.distill_mc_seed)
        except ops.BayesLMError as e:
            raise SystemExit("--distill-from %s: %s" % (args.distill_from, e))
        history.update({"interval_soft": [], "interval_kd_kl": []})
        topk = args.distill_top_k
        if args.distill_cache:
            fields = distill.TeacherCache.describe(ntokens, topk, args.distill_top_k_renorm, args.seq_len, train_data.size(0),
                                                   train_data.size(1), distill.sha256_tensor(train_data),
                                                   distill.sha256_file(args.distill_from), vars(teacher_shape),
                                                   args.distill_mc_samples, args.distill_mc_seed)
            try:
                cache = distill.TeacherCache(args.distill_cache, fields)
            except distill.CacheMismatch as e:
                raise SystemExit("--distill-cache: %s" % e)
        say("distilling from %s (%s), weight %g, %s%s" % (
            args.distill_from, type(teacher_model).__name__, args.distill_weight,
            "%d Monte-Carlo samples" % teacher.S if teacher.S else "mean weights",
            "" if args.distill_temperature == 1.0 else
            ", temperature %g (soft term times %g; soft and kd_kl below are at temperature)" % (args.distill_temperature,
                                                                                               args.distill_temperature ** 2)))
        if topk:
            say("top-%d teacher targets%s: %s" % (
                topk, " (renormalised)" if args.distill_top_k_renorm else "",
                "computed every batch, no cache" if cache is None else
                "loaded from the complete cache %s, the teacher does not run" % args.distill_cache if cache.complete else
                "the first epoch computes them and fills the cache %s, later epochs load them" % args.distill_cache))

    kl_fn = kl_selector(args)
    kl_scale = float(args.seq_len) / float(len(train_data))  # KL / len(train_data) * seq_len (train.py:338)
    trainer = engine.Trainer(model, lr=args.lr, clip=args.clip, momentum=0.9, kl_scale=kl_scale, seed=args.seed,
                             rank=rank, world=world, overlap=bool(args.dp_overlap), late_rows=bool(args.dp_late_rows))
    is_rnn = args.model != 'Transformer'
    collector = None
    if swag_args is not None:
        from . import swag
        collector = swag.SwagCollector(trainer, swag_args.rank, swag_args.start, swag_args.every)
        say("swag: collecting from epoch %d, %s, rank %d%s, into %s" % (
            swag_args.start, "every %d steps" % swag_args.every if swag_args.every else "at each epoch's end", swag_args.rank,
            "" if swag_args.lr is None else ", lr %g held from there" % swag_args.lr, swag_args.save))

    sampler = bank = None
    if sg_args is not None:
        from . import sgmcmc, swag as _swag
        steps_per_epoch = len(range(0, train_data.size(0) - 1, args.seq_len))
        n_tokens = (train_data.size(0) - 1) * train_data.size(1)  # the target tokens one epoch walks
        schedule = None
        try:
            if sg_args.cycles:
                schedule = sgmcmc.CyclicalSchedule((args.epochs - sg_args.start + 1) * steps_per_epoch, sg_args.cycles, sg_args.lr,
                                                   sg_args.explore)
            sampler = sgmcmc.Sampler(sg_args.rule, sg_args.lr, n_tokens, sg_args.temperature, sg_args.prior_precision,
                                     seed=sg_args.seed, schedule=schedule)
            bank = sgmcmc.SampleBank(trainer.flat.total, _swag.manifest_of(model), sg_args.keep, sampler.settings())
            collector = sgmcmc.SampleCollector(trainer, bank, sg_args.start, sg_args.every)
        except ops.BayesLMError as e:
            raise SystemExit("--sgmcmc-save: %s" % e)
        say("sgmcmc: %s from epoch %d, lr %g, temperature %g, prior precision %g over %d tokens (weight decay %g), %s, "
            "sampling %s, keeping %d, into %s" % (
                sg_args.rule, sg_args.start, sg_args.lr, sg_args.temperature, sg_args.prior_precision, n_tokens, sampler.weight_decay,
                "%d cycles, exploring %g of each" % (sg_args.cycles, sg_args.explore) if sg_args.cycles else "a constant rate",
                "every %d steps" % sg_args.every if sg_args.every else "at each epoch's end", sg_args.keep, sg_args.save))

    def swag_collected(epoch, n):
        if n is not None and bank is not None:
            say('| sgmcmc n {:d} | epoch {:3d} | step {:d} | lr {:.6g} | sigma {:.6g} |'.format(
                n, epoch, trainer.step_no, sampler.last_lr, sampler.last_sigma))
            return
        if n is not None:
            say('| swag n {:d} | epoch {:3d} | step {:d} | rank {:d} | k_live {:d} |'.format(
                n, epoch, trainer.step_no, collector.posterior.rank, collector.posterior.k_live))

    def train_epoch(epoch, lr):
        total_loss = 0.
        start = time.time()
        hidden = model.init_hidden(train_data.size(1)) if is_rnn else None
        total_soft = total_kd = 0.
        cached = teacher is not None and cache is not None and cache.complete  # this epoch's targets come from disk
        if teacher is not None and not cached:
            teacher.reset(train_data.size(1))
        for batch, i in enumerate(range(0, train_data.size(0) - 1, args.seq_len)):
            data, targets = D.get_batch(train_data, i, args.seq_len)
            if is_rnn:
                hidden = repackage_hidden(hidden)
            if teacher is None:
                loss, kl, hidden = trainer.step(data, targets, hidden, kl_fn)
            else:
                if cached:
                    logq = cache.load(i * train_data.size(1), data.numel(), device)
                elif topk:
                    logq, _ = teacher.topk(data, topk, bool(args.distill_top_k_renorm))
                    if cache is not None:
                        cache.store(i * train_data.size(1), logq)
                else:
                    logq, _ = teacher.logprobs(data)
                loss, kl, hidden = trainer.step(data, targets, hidden, kl_fn, soft=(logq, args.distill_weight, args.distill_temperature))
                total_soft, total_kd = total_soft + trainer.last_soft.soft, total_kd + trainer.last_soft.kl
            if collector is not None:
                swag_collected(epoch, collector.after_step(epoch))
            total_loss = total_loss + loss  # stays on the device: one host sync per log interval (train.py:422 syncs per step)
            if batch % args.log_interval == 0 and batch > 0:
                if world > 1:  # the mean over the GLOBAL batch, as the single-process log line prints it
                    total_loss = total_loss.detach().clone()
                    if args.dist_backend != "nccl":
                        total_loss = total_loss.cpu()  # a host-staged transport is handed host tensors (engine.LateRows.begin)
                    dist.all_reduce(total_loss)
                    total_loss = total_loss / world
                cur = float(total_loss) / args.log_interval
                history["interval_loss"].append(cur)
                elapsed = time.time() - start
                history["ms_per_batch"].append(elapsed * 1000 / args.log_interval)
                if trainer.sampler is not None and trainer.sampler.last_lr is not None:
                    lr = trainer.sampler.last_lr  # the rate the sampler applied to this step (a cyclical schedule moves it)
                line = ('| epoch {:3d} | {:5d}/{:5d} batches | lr {:02.3f} | ms/batch {:5.2f} | loss {:5.2f} | '
                        'kl_loss {:5.4} | ppl {:8.2f}'.format(epoch, batch, len(train_data) // args.seq_len, lr,
                                                              elapsed * 1000 / args.log_interval, cur,
                                                              float(kl) if kl is not None else 0., math.exp(min(cur, 80.0))))
                if teacher is not None:  # `loss` above is the mixed objective; these are its soft part and KL(teacher || student)
                    history["interval_soft"].append(float(total_soft) / args.log_interval)
                    history["interval_kd_kl"].append(float(total_kd) / args.log_interval)
                    line += ' | soft {:5.2f} | kd_kl {:5.4f}'.format(history["interval_soft"][-1], history["interval_kd_kl"][-1])
                    total_soft = total_kd = 0.
                say(line)
                total_loss = 0.
                start = time.time()
        if teacher is not None and cache is not None and not cache.complete:
            cache.finish()  # every window of the walk is stored: the file is marked complete, the next epoch reads it

    sched = ValidationSchedule(args.lr, world, device)
    say("Start training")
    try:
        for epoch in range(1, args.epochs + 1):
            t0 = time.time()
            sampling = sampler is not None and collector.active(epoch)
            if sampling and trainer.sampler is None:  # the burn-in is over: the sampler's update from this epoch on
                try:
                    trainer.set_sampler(sampler)
                except ops.BayesLMError as e:
                    raise SystemExit("--sgmcmc-save: %s" % e)
            held = sampling or (swag_args is not None and swag_args.lr is not None and collector.active(epoch))
            if held and not sampling:  # a constant rate from --swag-start on; the halving rule is suspended below
                trainer.lr = swag_args.lr
            train_epoch(epoch, (sg_args.lr if sampling else swag_args.lr) if held else sched.lr)
            if collector is not None:
                swag_collected(epoch, collector.epoch_end(epoch))
            if world > 1:
                engine.heartbeat("epoch %d trained" % epoch, rank)
            if held:
                (val_loss, improved), stop = sched.observe(engine.evaluate(model, val_data, args.seq_len, rank=rank, world=world)), False
            else:
                val_loss, improved, stop = sched.update(engine.evaluate(model, val_data, args.seq_len, rank=rank, world=world))
            say('-' * 89)
            say('| end of epoch {:3d} | time: {:5.2f}s | valid loss {:5.2f} | valid ppl {:8.2f}'.format(
                epoch, time.time() - t0, val_loss, math.exp(val_loss)))
            say('-' * 89)
            history["valid_loss"].append(val_loss)
            _print_coef_mean(args, model, say)
            if improved:
                if is_main:
                    with open(args.save, 'wb') as f:
                        torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, f)
            elif not held:  # train.py:503-508: halve LR, fresh SGD (momentum reset), reload best
                history["halved_epochs"].append(epoch)
                trainer.reset_optimizer(sched.lr)
                if world > 1:
                    dist.barrier()  # rank 0's checkpoint of an earlier epoch is on disk before anyone reads it
                with torch.no_grad():
                    sd = torch.load(args.save, map_location='cpu')
                    own = model.state_dict()
                    for k, v in sd.items():
                        own[k].copy_(v)
            if stop:
                break
    except KeyboardInterrupt:
        say('-' * 89)
        say('Exiting from training early')

    if bank is not None:
        if len(bank) < 1:
            say("sgmcmc: no sample was collected: %s is not written" % sg_args.save)
        else:
            bank.save(sg_args.save)
            say("sgmcmc: wrote %s (%d samples of %d seen, %s)" % (sg_args.save, len(bank), bank.seen, sg_args.rule))
    elif collector is not None:
        if collector.posterior.n < 1:
            say("swag: no iterate was collected: %s is not written" % swag_args.save)
        else:
            collector.posterior.save(swag_args.save)
            say("swag: wrote %s (n %d, rank %d)" % (swag_args.save, collector.posterior.n, collector.posterior.rank))
    if world > 1:
        dist.barrier()
    if os.path.exists(args.save):
        with torch.no_grad():
            sd = torch.load(args.save, map_location='cpu')
            own = model.state_dict()
            for k, v in sd.items():
                own[k].copy_(v)
    _print_coef_mean(args, model, say)
    test_loss = sched.agree(engine.evaluate(model, test_data, args.seq_len, rank=rank, world=world))
    history["test_loss"] = test_loss
    say('=' * 89)
    say('| End of training | test loss {:5.2f} | test ppl {:8.2f}'.format(test_loss, math.exp(test_loss)))
    say('=' * 89)
    if args.history and is_main:
        import json
        with open(args.history, 'w') as f:
            json.dump(history, f)
    if args.test_report:
        import json
        report = engine.evaluate_report(model, test_data, args.seq_len, mc_samples=args.test_mc_samples, seed=args.seed)
        with open(args.test_report, 'w') as f:
            json.dump(report.as_dict(), f)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return test_loss


if __name__ == "__main__":
    main()
