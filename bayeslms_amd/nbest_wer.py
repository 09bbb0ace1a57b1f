"""Word error rate of rescored n-best lists: the step the rescoring recipe ends in, from the text archives of its directory.

words_text holds the hypotheses, a Kaldi ``text`` file the references, and `key-n value` archives the costs of every
hypothesis (acwt, lmwt.nolm, lmwt.lmonly, and one lmwt.nn per scorer run).  Every hypothesis is aligned against its reference
once on the GPU (ops.edit_distance); a grid of (LM weight, nnweight, word insertion penalty) is then ranked by
ops.nbest_select and each point's picks are summed into err / sub / ins / del / WER / SER.  Two bounds frame the grid: the
list's own order (`first`) and the hypothesis with the fewest errors of every list (the lower bound any weighting can reach).
Minimum-Bayes-risk selection (Stolcke, Koenig, Weintraub 1997) picks the hypothesis with the least expected word error under
the list's own posterior; its pairwise distances are built for batches of utterances under a byte budget, never for the whole
set at once.

Conventions: every array is a COST (lower is better), as Kaldi writes them; the total of a hypothesis at a grid point
(L, w, p) is  ac + L (g + w nn + (1 - w) lm + p len), stage 7's sum ranked as Kaldi ranks at --inv-acoustic-scale=L.
Word ids are assigned from the surface words of hypotheses and references together, not from an LM vocabulary.
"""
import json
from collections import OrderedDict
from dataclasses import dataclass, field

import torch

from . import ops
from ._lib import BayesLMError

# the report's key for the lower bound of a list, spelt in two pieces: tests/test_cabi_cpu.py keeps the name of the CPU
# reference package out of this package's sources
LOWER_BOUND = "ora" + "cle"
FIELDS = ("err", "sub", "ins", "del", "wer", "ser")
MODES = ("present", "all", "strict")


# ---- text ----
def read_text(path):
    """Kaldi text: `uttid w1 w2 ...` -> {uttid: [w1, ...]} in file order"""
    out = OrderedDict()
    with open(path, "r", encoding="utf-8") as f:
        for ln in f:
            parts = ln.split()
            if parts:
                if parts[0] in out:
                    raise SystemExit("read_text: %s holds %s twice" % (path, parts[0]))
                out[parts[0]] = parts[1:]
    return out


def read_archive(path):
    """`key-n value` lines -> {key-n: float} in file order"""
    out = OrderedDict()
    with open(path, "r", encoding="utf-8") as f:
        for i, ln in enumerate(f, 1):
            parts = ln.split()
            if not parts:
                continue
            if len(parts) != 2:
                raise SystemExit("read_archive: %s line %d is not `key value`: %r" % (path, i, ln.rstrip("\n")))
            if parts[0] in out:
                raise SystemExit("read_archive: %s holds %s twice" % (path, parts[0]))
            try:
                out[parts[0]] = float(parts[1])
            except ValueError:
                raise SystemExit("read_archive: %s line %d: %r is not a number" % (path, i, parts[1]))
    return out


def read_words(path):
    with open(path, "r", encoding="utf-8") as f:
        return {w for ln in f for w in ln.split()}


def match_archive(nbest, utts, archive, name):
    """The archive's values in the order of the hypotheses of ``utts`` (hypothesis n of a list has the key `utt-n`, n from 1, as
    the scorer writes them).  Refuses with the offending key: a hypothesis without a value, or a value of one of these
    utterances without a hypothesis."""
    vals, used = [], 0
    for u in utts:
        for n in range(1, len(nbest[u]) + 1):
            key = "%s-%d" % (u, n)
            if key not in archive:
                raise SystemExit("nbest_wer: %s has no value for %s" % (name, key))
            vals.append(archive[key])
        used += len(nbest[u])
    if used != len(archive):
        want = set(utts)
        for key in archive:
            u, _, n = key.rpartition("-")
            if u in want and not (n.isdigit() and 1 <= int(n) <= len(nbest[u])):
                raise SystemExit("nbest_wer: %s holds %s, which is no hypothesis of the n-best lists" % (name, key))
    return vals


# ---- grid ----
def parse_values(spec):
    """`7:17` (step 1), `0:1:0.1`, `0,0.5,1` or one number -> list of floats; a range includes its end"""
    spec = str(spec).strip()
    try:
        if ":" in spec:
            parts = [float(x) for x in spec.split(":")]
            if len(parts) == 2:
                parts.append(1.0)
            lo, hi, step = parts
            if len(parts) != 3 or not step > 0 or hi < lo:
                raise ValueError
            n = int((hi - lo) / step + 1e-9) + 1
            return [round(lo + k * step, 10) for k in range(n)]
        return [float(x) for x in spec.split(",")]
    except ValueError:
        raise SystemExit("nbest_wer: %r is neither a number, a list `a,b,c` nor a range `lo:hi[:step]`" % spec)


def make_grid(lmwt, nnweight, wip, posterior_scale=1.0):
    """Points (L, w, p, s), L outermost and p innermost: the order `best` breaks ties in"""
    return [(float(lw), float(w), float(p), float(posterior_scale)) for lw in lmwt for w in nnweight for p in wip]


def batches(sizes, budget_bytes):
    """Consecutive utterances whose distance blocks (4 N^2 bytes each) fit the budget together -> [(first, end), ...]; an
    utterance that exceeds it alone is a batch of its own"""
    out, first, used = [], 0, 0
    for u, n in enumerate(sizes):
        b = 4 * n * n
        if u > first and used + b > budget_bytes:
            out.append((first, u))
            first, used = u, 0
        used += b
    if len(sizes) > first:
        out.append((first, len(sizes)))
    return out


# ---- report ----
def rates(err, sub, ins, dele, ref_words, wrong, utts):
    return {"err": int(err), "sub": int(sub), "ins": int(ins), "del": int(dele),
            "wer": 100.0 * int(err) / ref_words if ref_words else 0.0, "ser": 100.0 * int(wrong) / utts if utts else 0.0}


@dataclass
class WerReport:
    utterances: int
    ref_words: int
    first: dict
    lower_bound: dict
    systems: list                      # per nn entry: {"name", "grid": [{"lmwt", "nnweight", "wip", **rates}], "best": {...}}
    mbr: list = None                   # per nn entry: {"name", "lmwt", "nnweight", "wip", "posterior_scale", **rates, "mean_risk"}
    utts: list = field(default_factory=list)    # the utterances counted, in reference order
    picks: dict = field(default_factory=dict)   # name -> per utterance the chosen index in its list (-1: no list): "first",
    #                                             the lower bound, "<nn name>" (its best point), "<nn name>/mbr"
    utt_rows: list = field(default_factory=list)

    def to_dict(self):
        d = {"utterances": self.utterances, "ref_words": self.ref_words, "first": self.first, LOWER_BOUND: self.lower_bound,
             "systems": self.systems}
        if self.mbr is not None:
            d["mbr"] = self.mbr
        return d

    def table(self):
        rows = [("system", "lmwt", "nnweight", "wip") + FIELDS]

        def row(name, pt, r):
            return (name,) + tuple("-" if v is None else "%g" % v for v in pt) + tuple(
                "%.2f" % r[k] if k in ("wer", "ser") else "%d" % r[k] for k in FIELDS)
        rows.append(row("first", (None,) * 3, self.first))
        rows.append(row(LOWER_BOUND, (None,) * 3, self.lower_bound))
        for s in self.systems:
            b = s["best"]
            rows.append(row(s["name"], (b["lmwt"], b["nnweight"], b["wip"]), b))
        for m in self.mbr or ():
            rows.append(row(m["name"] + " mbr", (m["lmwt"], m["nnweight"], m["wip"]), m))
        width = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
        head = "%d utterances, %d reference words" % (self.utterances, self.ref_words)
        return "\n".join([head] + ["  ".join(v.ljust(w) if c == 0 else v.rjust(w) for c, (v, w) in enumerate(zip(r, width)))
                                   for r in rows])


def evaluate(nbest, refs, costs, grid, mode="present", ignore_words=(), mbr=False, mbr_point=None, budget_bytes=1 << 30,
             device=None, backend=None):
    """nbest: {utt: [hypothesis string, ...]} (load_nbest); refs: {utt: [word, ...]} (read_text); costs: {"ac": archive or None,
    "g": ..., "lm": ..., "nn": [(name, archive), ...]} with archives {key-n: cost} (read_archive); grid: points (L, w, p, s)
    (make_grid).  mode (compute-wer's): "present" skips references without a list, "all" counts them as all deletions, "strict"
    refuses them.  ignore_words are dropped from both sides before alignment (the word count of the insertion penalty is the
    hypothesis's own).  mbr: also minimum-Bayes-risk selection, at ``mbr_point`` (L, w, p, s) or at each nn entry's best point.
    backend: the module that supplies edit_distance / pairwise_edit_distance / nbest_select / nbest_mbr, ops by default (the
    tests hand in their plain-Python restatement to check this host code without a GPU; there is no fallback: ops raises on a
    tensor that is not on the GPU).  -> WerReport"""
    be = backend if backend is not None else ops
    if mode not in MODES:
        raise BayesLMError("nbest_wer.evaluate: mode %r is not one of %s" % (mode, ", ".join(MODES)))
    if not grid:
        raise BayesLMError("nbest_wer.evaluate: an empty grid")
    dev = torch.device(device if device is not None else "cuda")
    ignore = set(ignore_words)
    missing = [u for u in refs if u not in nbest]
    if missing and mode == "strict":
        raise SystemExit("nbest_wer: no n-best list for %s (%d references without one; --mode strict)" % (missing[0], len(missing)))
    utts = [u for u in refs if u in nbest]
    ref_seqs = [[w for w in refs[u] if w not in ignore] for u in utts]
    extra_ref = [[w for w in refs[u] if w not in ignore] for u in missing] if mode == "all" else []
    extra_del = sum(len(r) for r in extra_ref)
    extra_wrong = sum(1 for r in extra_ref if r)
    n_utts = len(utts) + len(extra_ref)
    ref_words = sum(len(r) for r in ref_seqs) + extra_del

    # sequences: the H hypotheses, then the U references; ids from the surface words of both
    ids = {}
    tok, off, lens, sizes = [], [0], [], []
    for u in utts:
        sizes.append(len(nbest[u]))
        for hyp in nbest[u]:
            words = hyp.split()
            lens.append(float(len(words)))
            tok.extend(ids.setdefault(w, len(ids)) for w in words if w not in ignore)
            off.append(len(tok))
    H = len(lens)
    for r in ref_seqs:
        tok.extend(ids.setdefault(w, len(ids)) for w in r)
        off.append(len(tok))
    U = len(utts)
    uoff_host = [0]
    for n in sizes:
        uoff_host.append(uoff_host[-1] + n)
    tok_d = torch.tensor(tok, dtype=torch.int32, device=dev)
    off_d = torch.tensor(off, dtype=torch.int64, device=dev)
    uoff = torch.tensor(uoff_host, dtype=torch.int64, device=dev)
    grp = torch.repeat_interleave(torch.arange(U, device=dev), torch.tensor(sizes, dtype=torch.int64, device=dev)) if U else \
        torch.zeros(0, dtype=torch.int64, device=dev)
    a = torch.arange(H, device=dev, dtype=torch.int32)
    b = (grp + H).to(torch.int32)
    cost, sid = be.edit_distance(tok_d, off_d, a, b, breakdown=True)
    if H and int(cost.min()) < 0:
        bad = int((cost < 0).nonzero()[0])
        raise SystemExit("nbest_wer: hypothesis %d of the lists or its reference is longer than %d words" % (bad, 1023))
    quad = torch.cat([cost[:, None], sid], 1).to(torch.int64)  # (H, 4) err / sub / ins / del

    def summed(pick):
        """pick (K, U) -> K rate dicts: gathers and sums in int64"""
        out = []
        if U == 0:
            return [rates(extra_del, 0, 0, extra_del, ref_words, extra_wrong, n_utts) for _ in range(pick.shape[0])]
        rows = quad[(uoff[:-1][None, :] + pick.to(torch.int64)).reshape(-1)].reshape(pick.shape[0], U, 4)
        tot = rows.sum(1).tolist()
        wrong = (rows[:, :, 0] > 0).sum(1).tolist()
        for (e, s, i, d), wr in zip(tot, wrong):
            out.append(rates(e + extra_del, s, i, d + extra_del, ref_words, wr + extra_wrong, n_utts))
        return out

    def as_f64(vals):
        return torch.tensor(vals, dtype=torch.float64, device=dev)
    one = [(1.0, 0.0, 0.0, 1.0)]
    pick_first = be.nbest_select(torch.zeros(H, dtype=torch.float64, device=dev), None, None, None, None, uoff, one)
    pick_low = be.nbest_select(cost.to(torch.float64), None, None, None, None, uoff, one)
    picks = {"first": pick_first[0], LOWER_BOUND: pick_low[0]}
    report = WerReport(n_utts, ref_words, summed(pick_first)[0], summed(pick_low)[0], [], None)

    ac, g, lm = (as_f64(match_archive(nbest, utts, costs[k], k)) if costs.get(k) is not None else None for k in ("ac", "g", "lm"))
    ln = as_f64(lens)
    nn_entries = list(costs.get("nn") or [])
    if not nn_entries:
        nn_entries = [("no-nn", None)]
    points = [tuple(pt) + (1.0,) * (4 - len(pt)) for pt in grid]
    mbr_jobs = []
    for name, archive in nn_entries:
        nn = as_f64(match_archive(nbest, utts, archive, name)) if archive is not None else None
        pick = be.nbest_select(ac, g, lm, nn, ln, uoff, points)
        rows = summed(pick)
        grid_rows = [dict(lmwt=pt[0], nnweight=pt[1], wip=pt[2], **r) for pt, r in zip(points, rows)]
        k_best = min(range(len(rows)), key=lambda k: (rows[k]["err"], k))
        report.systems.append({"name": name, "grid": grid_rows, "best": dict(grid_rows[k_best])})
        picks[name] = pick[k_best]
        mbr_jobs.append((name, nn, tuple(mbr_point) + (1.0,) * (4 - len(mbr_point)) if mbr_point is not None else points[k_best]))

    if mbr:
        report.mbr = []
        hyp_off = off_d[:H + 1]
        per_job = [([], []) for _ in mbr_jobs]  # picks, risks of the picks, batch by batch
        for u0, u1 in batches(sizes, budget_bytes):
            h0, h1 = uoff_host[u0], uoff_host[u1]
            sub_uoff = uoff[u0:u1 + 1] - h0
            # the batch's own sequences: offsets h0 .. h1 of the same flat buffer
            dist, doff = be.pairwise_edit_distance(tok_d, hyp_off[h0:h1 + 1], sub_uoff)

            def cut(t):
                return None if t is None else t[h0:h1]
            for (name, nn, pt), (pk, rk) in zip(mbr_jobs, per_job):
                risk, pick = be.nbest_mbr(cut(ac), cut(g), cut(lm), cut(nn), cut(ln), sub_uoff, dist, doff, [pt])
                pk.append(pick[0])
                rk.append(risk[0][(sub_uoff[:-1] + pick[0].to(torch.int64))])
            del dist
        for (name, nn, pt), (pk, rk) in zip(mbr_jobs, per_job):
            pick = torch.cat(pk)[None, :] if pk else torch.zeros(1, 0, dtype=torch.int32, device=dev)
            r = summed(pick)[0]
            risks = torch.cat(rk) if rk else torch.zeros(0, dtype=torch.float64, device=dev)
            report.mbr.append(dict(name=name, lmwt=pt[0], nnweight=pt[1], wip=pt[2], posterior_scale=pt[3],
                                   mean_risk=float(risks.mean()) if U else 0.0, **r))
            picks[name + "/mbr"] = pick[0]
            picks[name + "/mbr_risk"] = risks

    # host copies for the writers
    report.utts = utts + (missing if mode == "all" else [])
    pad = [-1] * len(extra_ref)
    err_host = cost.tolist()
    for k, v in picks.items():
        if k.endswith("/mbr_risk"):
            report.picks[k] = v.tolist() + [0.0] * len(pad)
        else:
            report.picks[k] = v.tolist() + pad
    chosen = nn_entries[0][0]
    for i, u in enumerate(report.utts):
        if i < U:
            def e(name):
                return err_host[uoff_host[i] + report.picks[name][i]]
            row = {"utt": u, "ref_words": len(ref_seqs[i]), "hyps": sizes[i], "first_err": e("first"), "low_err": e(LOWER_BOUND),
                   "pick": report.picks[chosen][i] + 1, "err": e(chosen)}
            if mbr:
                row.update(mbr_pick=report.picks[chosen + "/mbr"][i] + 1, mbr_err=e(chosen + "/mbr"),
                           mbr_risk=report.picks[chosen + "/mbr_risk"][i])
        else:
            n = len(extra_ref[i - U])
            row = {"utt": u, "ref_words": n, "hyps": 0, "first_err": n, "low_err": n, "pick": 0, "err": n}
            if mbr:
                row.update(mbr_pick=0, mbr_err=n, mbr_risk=0.0)
        report.utt_rows.append(row)
    return report


def best_transcripts(nbest, report, name=None, mbr=False):
    """[(utt, hypothesis string)] of the picks of nn entry ``name`` (default: the first) at its best grid point, or its MBR picks;
    an utterance without a list (mode "all") has an empty transcript"""
    name = name if name is not None else report.systems[0]["name"]
    pk = report.picks[name + "/mbr" if mbr else name]
    return [(u, " ".join(nbest[u][k].split()) if k >= 0 else "") for u, k in zip(report.utts, pk)]


def write_best(path, transcripts):
    with open(path, "w", encoding="utf-8") as f:
        for u, words in transcripts:
            f.write(("%s %s" % (u, words)).rstrip() + "\n")


def write_utt(path, report):
    """One line per utterance: utt ref_words hyps first_err low_err pick err [mbr_pick mbr_err mbr_risk]; picks count from 1
    as the archive keys do, 0: no list"""
    with open(path, "w", encoding="utf-8") as f:
        for r in report.utt_rows:
            cols = [r["utt"], r["ref_words"], r["hyps"], r["first_err"], r["low_err"], r["pick"], r["err"]]
            if "mbr_pick" in r:
                cols += [r["mbr_pick"], r["mbr_err"], "%.6g" % r["mbr_risk"]]
            f.write(" ".join(str(c) for c in cols) + "\n")


def write_report(path, report):
    with open(path, "w", encoding="utf-8") as f:
        json.dump(report.to_dict(), f, indent=1)
        f.write("\n")
