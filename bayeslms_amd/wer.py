"""python -m bayeslms_amd.wer: word error rate of a rescoring directory's n-best lists over a grid of LM weight, nnweight and
word insertion penalty, with the list's own order and its lower bound beside it and, on request, minimum-Bayes-risk selection
(bayeslms_amd/nbest_wer.py).

    python -m bayeslms_amd.wer --words-text DIR/words_text --ref-text data/dev/text --acwt DIR/acwt --nolm DIR/lmwt.nolm \\
        --lmonly DIR/lmwt.lmonly --nn DIR/lmwt.nn --nn DIR/lmwt.nn.mc8 --lmwt 7:17 --nnweight 0:1:0.1 --wip 0,0.5,1 \\
        --mbr 1 --write-report wer.json --write-best best.txt
"""
import argparse
import os

from . import nbest_wer as W
from .compute_sentence_scores import load_nbest


def build_parser():
    p = argparse.ArgumentParser(prog="python -m bayeslms_amd.wer", description=__doc__.split("\n\n")[0])
    p.add_argument("--words-text", required=True, help="the n-best lists: `uttid-n w1 w2 ...`")
    p.add_argument("--ref-text", required=True, help="Kaldi text of the references: `uttid w1 w2 ...`")
    p.add_argument("--acwt", help="acoustic costs, `key-n value`")
    p.add_argument("--nolm", help="graph costs (lmwt.nolm)")
    p.add_argument("--lmonly", help="the old LM's costs (lmwt.lmonly)")
    p.add_argument("--nn", action="append", default=[], help="neural costs as the scorer writes them (lmwt.nn); may be given "
                   "several times: alignments are computed once and every file is ranked on the same grid")
    p.add_argument("--lmwt", default="7:17", help="LM weights: a number, `a,b,c` or `lo:hi[:step]` (default 7:17)")
    p.add_argument("--nnweight", default="0:1:0.1", help="weights of the neural cost against the old LM's (default 0:1:0.1)")
    p.add_argument("--wip", default="0", help="word insertion penalties (default 0)")
    p.add_argument("--posterior-scale", type=float, default=1.0, help="scale of the costs in the MBR posterior (default 1)")
    p.add_argument("--mbr", type=int, default=0, choices=(0, 1), help="1: also minimum-Bayes-risk selection")
    p.add_argument("--mbr-point", help="`lmwt,nnweight,wip` for MBR; default: each --nn file's best grid point")
    p.add_argument("--mbr-budget-mb", type=float, default=1024.0, help="MBR distance blocks are built for batches of utterances "
                   "under this many MiB (default 1024)")
    p.add_argument("--ignore-words", help="a file of words dropped from hypotheses and references before alignment")
    p.add_argument("--mode", default="present", choices=W.MODES, help="references without a list: present skips them, all counts "
                   "them as deletions, strict refuses them (compute-wer's)")
    p.add_argument("--write-report", help="the whole report as JSON")
    p.add_argument("--write-best", help="transcripts of the first --nn file's best point (its MBR picks with --mbr 1), text format")
    p.add_argument("--write-utt", help="one line per utterance: utt ref_words hyps first_err low_err pick err [mbr_pick mbr_err mbr_risk]")
    p.add_argument("--device", default="cuda")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    nbest = load_nbest(args.words_text)
    refs = W.read_text(args.ref_text)
    costs = {k: W.read_archive(path) if path else None for k, path in (("ac", args.acwt), ("g", args.nolm), ("lm", args.lmonly))}
    names = []
    for path in args.nn:
        name = os.path.basename(path)
        names.append(name if name not in names else "%s#%d" % (name, len(names) + 1))
    costs["nn"] = [(name, W.read_archive(path)) for name, path in zip(names, args.nn)]
    grid = W.make_grid(W.parse_values(args.lmwt), W.parse_values(args.nnweight), W.parse_values(args.wip), args.posterior_scale)
    point = None
    if args.mbr_point:
        point = tuple(W.parse_values(args.mbr_point))
        if len(point) != 3:
            raise SystemExit("--mbr-point takes `lmwt,nnweight,wip`")
        point += (args.posterior_scale,)
    report = W.evaluate(nbest, refs, costs, grid, mode=args.mode,
                        ignore_words=W.read_words(args.ignore_words) if args.ignore_words else (), mbr=bool(args.mbr),
                        mbr_point=point, budget_bytes=int(args.mbr_budget_mb * (1 << 20)), device=args.device)
    print(report.table())
    if args.write_report:
        W.write_report(args.write_report, report)
    if args.write_best:
        W.write_best(args.write_best, W.best_transcripts(nbest, report, mbr=bool(args.mbr)))
    if args.write_utt:
        W.write_utt(args.write_utt, report)
    return report


if __name__ == "__main__":
    main()
