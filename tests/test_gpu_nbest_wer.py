"""GPU: the n-best WER kernels (csrc/nbest.hip: blm_edit_distance in both forms, blm_nbest_select, blm_nbest_mbr) and the
evaluation built on them, against tests/nbest_reference.py.  Integer results are compared with torch.equal."""
import os

import numpy as np
import pytest
import torch

import nbest_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from bayeslms_amd import ops
    return ops


def flat(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    tok = np.concatenate([np.asarray(s, np.int32) for s in seqs] + [np.zeros(0, np.int32)])
    return tok, off


def run(ops, tok, off, a, b, lane_max=None):
    t = (torch.from_numpy(np.asarray(tok, np.int32)).to(DEV), torch.from_numpy(np.asarray(off, np.int64)).to(DEV),
         torch.from_numpy(np.asarray(a, np.int32)).to(DEV), torch.from_numpy(np.asarray(b, np.int32)).to(DEV))
    if lane_max is None:
        return ops.edit_distance(*t, breakdown=True)
    ops.set_option("edit_lane_max", lane_max)
    try:
        return ops.edit_distance(*t, breakdown=True)
    finally:
        ops.set_option("edit_lane_max", 32)


def expect(tok, off, a, b):
    cost, sid = R.edit_distance(tok, off, a, b)
    return torch.from_numpy(cost).to(DEV), torch.from_numpy(sid).to(DEV)


def check(ops, tok, off, a, b, forms=(None, 0)):
    """the default split between the forms, and every pair with two non-empty sides through the wavefront form"""
    want = expect(tok, off, a, b)
    for lane_max in forms:
        cost, sid = run(ops, tok, off, a, b, lane_max)
        assert cost.dtype == torch.int32 and sid.dtype == torch.int32
        assert torch.equal(cost, want[0]), (lane_max, (cost != want[0]).nonzero()[:5].tolist())
        assert torch.equal(sid, want[1]), (lane_max, (sid != want[1]).any(1).nonzero()[:5].tolist())
    return want


# ---- edit distance ----
def test_edit_distance_small_cases(ops):
    seqs = [[], [7], [7, 8], [8, 7], [1, 2, 3, 4, 5], [9], [1, 2, 3, 9, 5, 6]]
    tok, off = flat(seqs)
    n = len(seqs)
    a, b = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)  # every pair, a sequence with itself among them
    cost, sid = check(ops, tok, off, a, b, forms=(None, 0, 1, 8))
    at = lambda i, j: (int(cost[i * n + j]),) + tuple(sid[i * n + j].tolist())
    assert at(0, 0) == (0, 0, 0, 0) and at(1, 0) == (1, 0, 1, 0) and at(0, 2) == (2, 0, 0, 2) and at(4, 4) == (0, 0, 0, 0)
    assert at(2, 3) == (2, 2, 0, 0)  # [x, y] against [y, x]: two substitutions, not an insertion and a deletion
    assert at(1, 5) == (1, 1, 0, 0) and at(4, 6) == (2, 1, 0, 1)


def test_edit_distance_empty_call(ops):
    tok, off = flat([[1, 2]])
    cost, sid = run(ops, tok, off, [], [])
    assert cost.shape == (0,) and sid.shape == (0, 3)
    cost = ops.edit_distance(torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV),
                             torch.tensor([0, 1], dtype=torch.int32, device=DEV), torch.tensor([1, 1], dtype=torch.int32, device=DEV))
    assert cost.tolist() == [0, 0]  # no words at all: two empty sequences


@pytest.fixture(scope="module")
def threshold_case():
    """the lengths at which the kernels change path (columns per instance 8 / 16 / 32, the lane-per-pair limit 32, columns per
    lane 1 / 2 / 4 / 16 of the wavefront form, the limit 1023) against each other and against 1, two-word alphabet"""
    rng = np.random.default_rng(5)
    lens = [1, 31, 32, 33, 63, 64, 65, 127, 129, 1023]
    seqs = [rng.integers(0, 2, n).tolist() for n in lens]
    tok, off = flat(seqs)
    n = len(lens)
    a, b = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    return tok, off, a, b, expect(tok, off, a, b)


@pytest.mark.parametrize("lane_max", [None, 0, 16])
def test_edit_distance_lengths_at_the_thresholds(ops, threshold_case, lane_max):
    tok, off, a, b, want = threshold_case
    cost, sid = run(ops, tok, off, a, b, lane_max)
    assert torch.equal(cost, want[0]) and torch.equal(sid, want[1])


def test_edit_distance_random_pairs_with_ties_everywhere_in_both_orientations(ops):
    rng = np.random.default_rng(11)
    seqs = [rng.integers(0, rng.integers(2, 4), rng.integers(0, 41)).tolist() for _ in range(160)]
    seqs += [rng.integers(0, 3, rng.integers(33, 80)).tolist() for _ in range(12)]
    tok, off = flat(seqs)
    P = 3000
    a, b = rng.integers(0, len(seqs), P), rng.integers(0, len(seqs), P)
    cost, sid = check(ops, tok, off, a, b, forms=(None, 0, 9))
    back = run(ops, tok, off, b, a)  # (b, a): the same cost and substitutions, insertions and deletions exchanged
    assert torch.equal(back[0], cost) and torch.equal(back[1], sid[:, [0, 2, 1]])
    assert torch.equal(sid.sum(1), cost)
    only = ops.edit_distance(*(torch.from_numpy(x).to(DEV) for x in (tok, off, a.astype(np.int32), b.astype(np.int32))))
    assert torch.equal(only, cost)  # without the breakdown


def test_edit_distance_negative_and_large_ids(ops):
    big = [-2 ** 31, 2 ** 31 - 1, -1, 0, 2 ** 30, -2 ** 30, 65536, 65537]
    rng = np.random.default_rng(2)
    seqs = [[big[k] for k in rng.integers(0, len(big), n)] for n in (0, 3, 9, 17, 33, 40, 70, 5)]
    tok, off = flat(seqs)
    n = len(seqs)
    check(ops, tok, off, np.repeat(np.arange(n), n), np.tile(np.arange(n), n))


def test_edit_distance_bad_pairs_get_minus_one_and_their_neighbours_are_right(ops):
    rng = np.random.default_rng(3)
    tok = rng.integers(0, 3, 1100).astype(np.int32)
    # sequences: 0 = [0, 5), 1 = [5, 3) reversed, 2 = [3, 8), 3 = [8, 1032) 1024 words, 4 = [1032, 1040), 5 = [1040, 1101) leaves tok,
    # 6 = [1101, 1050) reversed and outside, 7 = [1050, 1100), 8 = [1100, 1100) empty at the very end, 9 = [-2, 3) starts before tok
    off = np.array([0, 5, 3, 8, 1032, 1040, 1101, 1050, 1100, 1100], np.int64)
    off2 = np.array([-2, 3], np.int64)
    a = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 0, -1, 9, 1, 2 ** 31 - 1, -2 ** 31, 7, 4, 0], np.int32)
    b = np.array([2, 2, 1, 4, 3, 0, 0, 4, 7, 9, 0, 0, 0, 0, 0, 7, 2, 8], np.int32)
    cost, sid = check(ops, tok, off, a, b)
    assert cost.tolist()[:9] == [int(cost[0]), -1, -1, -1, -1, -1, -1, int(cost[7]), 50] and int(cost[0]) >= 0 and int(cost[7]) >= 0
    assert cost.tolist()[9:15] == [-1] * 6 and cost.tolist()[15] == 0 and int(cost[16]) >= 0 and cost.tolist()[17] == 5
    assert torch.equal(sid[cost < 0], torch.full((int((cost < 0).sum()), 3), -1, dtype=torch.int32, device=DEV))
    c2, s2 = check(ops, tok, off2, np.array([0], np.int32), np.array([0], np.int32))
    assert c2.tolist() == [-1]


def test_pairwise_blocks(ops):
    rng = np.random.default_rng(4)
    sizes = [1, 4, 0, 7, 2]
    seqs = [rng.integers(0, 3, rng.integers(0, 12)).tolist() for _ in range(sum(sizes))]
    tok, off = flat(seqs)
    uoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    dist, doff = ops.pairwise_edit_distance(*(torch.from_numpy(x).to(DEV) for x in (tok, off, uoff)))
    want = R.pairwise(tok, off, uoff)
    assert dist.dtype == torch.int32 and doff.dtype == torch.int64
    assert torch.equal(dist.cpu(), torch.from_numpy(want[0])) and torch.equal(doff.cpu(), torch.from_numpy(want[1]))


# ---- selection ----
SIZES = [1, 63, 64, 0, 65, 257, 1025, 2, 5]


def exact_costs(rng, H):
    """multiples of 2^-6 below 2^14: with w in eighths, p in quarters and an integer L <= 32 every product and sum of the total
    is exact in float64 whatever the order, so the picks must equal the reference's everywhere, ties included"""
    return [rng.integers(0, 2 ** 20, H).astype(np.float64) / 64.0 for _ in range(4)] + [rng.integers(0, 40, H).astype(np.float64)]


def exact_grid(rng, G):
    return [(float(rng.integers(1, 33)), float(rng.integers(-8, 17)) / 8.0, float(rng.integers(-8, 9)) / 4.0, 1.0) for _ in range(G)]


@pytest.fixture(scope="module")
def select_case():
    rng = np.random.default_rng(21)
    uoff = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    H = int(uoff[-1])
    arrs = exact_costs(rng, H)
    # ties: whole stretches of equal hypotheses, across the lanes of a wave, across waves and across a lane's own turns
    for lo, hi in ((1, 64), (70, 90), (200, 450), (460, 1480)):
        for x in arrs:
            x[lo:hi] = x[lo + (hi - lo) // 2]
    for x in arrs:
        x[1300] = x[600]
        x[-5:] = x[-5]
    arrs[0][300] -= 1.0 / 64  # one winner inside a stretch of ties
    grid = exact_grid(rng, 65) + [(1.0, 0.0, 0.0, 1.0), (32.0, 2.0, -2.0, 1.0)]
    return arrs, uoff, grid, {G: R.select(*arrs, uoff, grid[:G]) for G in (1, 64, 67)}


def dev64(x):
    return None if x is None else torch.from_numpy(np.asarray(x, np.float64)).to(DEV)


@pytest.mark.parametrize("G", [1, 64, 67])
def test_select_equals_the_reference_exactly(ops, select_case, G):
    arrs, uoff, grid, want = select_case
    pick = ops.nbest_select(*(dev64(x) for x in arrs), torch.from_numpy(uoff).to(DEV), grid[:G])
    assert pick.dtype == torch.int32 and pick.shape == (G, len(SIZES))
    assert torch.equal(pick.cpu(), torch.from_numpy(want[G]))
    assert (pick[:, 3] == -1).all()  # the empty group
    if G == 67:  # some picks are decided by a tie: the reference's lowest index among equal totals
        t = R.totals(*arrs, grid[0])
        assert any((t[lo:hi] == t[lo:hi].min()).sum() > 1 for lo, hi in zip(uoff[:-1], uoff[1:]) if hi > lo)


def test_select_missing_arrays_count_as_zeros(ops, select_case):
    arrs, uoff, grid, _ = select_case
    u = torch.from_numpy(uoff).to(DEV)
    for keep in ((0,), (3,), (1, 4), (2, 3)):
        sub = [x if k in keep else None for k, x in enumerate(arrs)]
        want = R.select(*sub, uoff, grid[:5], H=int(uoff[-1]))
        assert torch.equal(ops.nbest_select(*(dev64(x) for x in sub), u, grid[:5]).cpu(), torch.from_numpy(want))
    none = ops.nbest_select(None, None, None, None, None, u, grid[:2])  # every total is 0: the first of each list
    assert torch.equal(none.cpu(), torch.from_numpy(R.select(None, None, None, None, None, uoff, grid[:2])))


def test_select_non_finite_totals_never_win(ops):
    rng = np.random.default_rng(22)
    sizes = [4, 3, 0, 300, 1, 2]
    uoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    arrs = exact_costs(rng, int(uoff[-1]))
    arrs[0][0], arrs[1][1], arrs[3][2] = np.nan, np.inf, -np.inf   # group 0: only its last hypothesis is finite
    arrs[0][4:7] = [np.nan, np.inf, -np.inf]                      # group 1: none is finite -> 0
    arrs[2][7:307:3] = np.nan
    arrs[0][8:307:7] = -np.inf
    arrs[0][307] = np.inf                                          # a group of one non-finite hypothesis -> 0
    arrs[4][308] = np.nan
    grid = exact_grid(rng, 6) + [(2.0, 1.0, 0.0, 1.0)]             # w = 1: 0 * lm, which is NaN where lm is
    want = R.select(*arrs, uoff, grid)
    pick = ops.nbest_select(*(dev64(x) for x in arrs), torch.from_numpy(uoff).to(DEV), grid)
    assert torch.equal(pick.cpu(), torch.from_numpy(want))
    assert (pick[:, 0] == 3).all() and (pick[:, 1] == 0).all() and (pick[:, 2] == -1).all() and (pick[:, 4] == 0).all()
    assert (pick[:, 5] == 1).all()


# ---- minimum Bayes risk ----
def random_blocks(rng, sizes, hi=30):
    blocks, doff, at = [], [], 0
    for n in sizes:
        d = rng.integers(0, hi, (n, n)).astype(np.int32)
        d = np.triu(d, 1)
        d = d + d.T
        blocks.append(d.reshape(-1))
        doff.append(at)
        at += n * n
    return np.concatenate(blocks + [np.zeros(0, np.int32)]), np.asarray(doff, np.int64)


def bound(n):
    """a few ulp for each of the N terms of the two sums and the exponential, on both sides: 4 (N + 8) 2^-52, relative"""
    return 4.0 * (n + 8) * 2.0 ** -52


def mbr_on_gpu(ops, arrs, uoff, dist, doff, grid):
    risk, pick = ops.nbest_mbr(*(dev64(x) for x in arrs), torch.from_numpy(uoff).to(DEV), torch.from_numpy(dist).to(DEV),
                               torch.from_numpy(doff).to(DEV), grid)
    return risk.cpu().numpy(), pick.cpu().numpy()


def check_mbr(risk, pick, ref_risk, uoff):
    worst = 0.0
    for k in range(risk.shape[0]):
        for u, (lo, hi) in enumerate(zip(uoff[:-1], uoff[1:])):
            n = int(hi - lo)
            if n == 0:
                assert pick[k, u] == -1
                continue
            r, rr = risk[k, lo:hi], ref_risk[k, lo:hi]
            err = np.abs(r - rr) / np.where(rr > 0, rr, 1.0)
            worst = max(worst, float(err.max()) / bound(n))
            assert (np.abs(r - rr) <= bound(n) * np.abs(rr)).all(), (k, u, n, float(err.max()), bound(n))
            assert pick[k, u] == int(np.argmin(r)), (k, u)  # the lowest index among the least of the kernel's OWN risks
            assert rr[pick[k, u]] <= rr.min() * (1.0 + bound(n)), (k, u, rr[pick[k, u]], rr.min())
    print("largest risk error / bound: %.3f" % worst)


@pytest.fixture(scope="module")
def mbr_case():
    rng = np.random.default_rng(31)
    sizes = [1, 2, 63, 0, 64, 65, 257, 600]
    uoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    H = int(uoff[-1])
    arrs = [rng.normal(0, 30, H) + 100, rng.normal(0, 3, H), rng.normal(0, 4, H) + 20, rng.normal(0, 4, H) + 22,
            rng.integers(1, 30, H).astype(np.float64)]
    dist, doff = random_blocks(rng, sizes)
    grid = [(10.0, 0.5, 0.0, 1.0), (7.0, 0.8, 0.5, 0.3), (12.5, 1.0, -0.5, 4.0), (9.0, 0.0, 0.0, 0.0)]  # the last: s = 0
    return arrs, uoff, dist, doff, grid, R.mbr(*arrs, uoff, dist, doff, grid)


def test_mbr_risk_and_pick_against_the_reference(ops, mbr_case):
    arrs, uoff, dist, doff, grid, (ref_risk, ref_pick) = mbr_case
    risk, pick = mbr_on_gpu(ops, arrs, uoff, dist, doff, grid)
    check_mbr(risk, pick, ref_risk, uoff)
    # s = 0: the posterior is uniform, the risk of a hypothesis is the mean of its row
    lo, hi = int(uoff[6]), int(uoff[7])
    n = hi - lo
    mean = dist[int(doff[6]):int(doff[6]) + n * n].reshape(n, n).astype(np.float64).mean(1)
    np.testing.assert_allclose(risk[3, lo:hi], mean, rtol=bound(n), atol=0)
    again, pick2 = mbr_on_gpu(ops, arrs, uoff, dist, doff, grid)  # no atomics: the same bits in every run
    assert np.array_equal(again.view(np.int64), risk.view(np.int64)) and np.array_equal(pick2, pick)
    only_pick = ops.nbest_mbr(*(dev64(x) for x in arrs), torch.from_numpy(uoff).to(DEV), torch.from_numpy(dist).to(DEV),
                              torch.from_numpy(doff).to(DEV), grid, want_risk=False)
    assert only_pick[0] is None and np.array_equal(only_pick[1].cpu().numpy(), pick)


def test_mbr_list_longer_than_one_posterior_chunk_and_grid_chunking(ops):
    """N = 2100 > 2048: the posterior is formed chunk by chunk, once per 256 rows; 65 grid points take two launches"""
    rng = np.random.default_rng(32)
    sizes = [3, 2100]
    uoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    H = int(uoff[-1])
    arrs = [rng.normal(0, 20, H) + 100, None, rng.normal(0, 4, H), rng.normal(0, 4, H), None]
    dist, doff = random_blocks(rng, sizes)
    grid = [(10.0, 0.5, 0.0, 1.0), (8.0, 1.0, 0.0, 0.5)]
    risk, pick = mbr_on_gpu(ops, arrs, uoff, dist, doff, grid)
    check_mbr(risk, pick, R.mbr(*arrs, uoff, dist, doff, grid)[0], uoff)
    small = [a[:3] if a is not None else None for a in arrs]
    grid65 = [(5.0 + 0.25 * k, 0.5, 0.0, 1.0) for k in range(65)]
    r65, p65 = mbr_on_gpu(ops, small, uoff[:2], dist[:9], doff[:1], grid65)
    assert r65.shape == (65, 3) and p65.shape == (65, 1)
    check_mbr(r65, p65, R.mbr(*small, uoff[:2], dist[:9], doff[:1], grid65)[0], uoff[:2])


def test_mbr_exact_picks_where_the_reference_margins_are_wide(ops):
    """seed chosen on the CPU: in every group and at every grid point the reference's least risk is more than 1e-6 (relative)
    below its runner-up, asserted here on the reference itself; the kernel's picks must then be the reference's"""
    rng = np.random.default_rng(33)
    sizes = [2, 5, 17, 64, 130, 300]
    uoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    H = int(uoff[-1])
    arrs = [rng.normal(0, 30, H) + 100, rng.normal(0, 3, H), rng.normal(0, 4, H) + 20, rng.normal(0, 4, H) + 22,
            rng.integers(1, 30, H).astype(np.float64)]
    dist, doff = random_blocks(rng, sizes)
    grid = [(10.0, 0.5, 0.0, 1.0), (7.0, 0.8, 0.5, 0.3), (15.0, 0.2, 0.0, 2.0)]
    ref_risk, ref_pick = R.mbr(*arrs, uoff, dist, doff, grid)
    for k in range(len(grid)):
        for lo, hi in zip(uoff[:-1], uoff[1:]):
            r = np.sort(ref_risk[k, lo:hi])
            assert r[1] - r[0] > 1e-6 * r[0], (k, lo, r[:2])
    risk, pick = mbr_on_gpu(ops, arrs, uoff, dist, doff, grid)
    assert np.array_equal(pick, ref_pick)


def test_mbr_duplicate_hypotheses_have_identical_risk_bits_and_the_lower_index_wins(ops):
    rng = np.random.default_rng(34)
    n = 70
    uoff = np.array([0, n], np.int64)
    arrs = [rng.normal(0, 10, n) + 50 for _ in range(4)] + [rng.integers(1, 20, n).astype(np.float64)]
    dist, doff = random_blocks(rng, [n], hi=12)
    d = dist.reshape(n, n)
    d += 1  # no two different hypotheses at distance 0
    d[np.arange(n), np.arange(n)] = 0
    for lo, hi in ((5, 66), (20, 21)):  # hi is a copy of lo: the same costs, the same distances to everything, 0 between them
        for x in arrs:
            x[hi] = x[lo]
        d[hi, :] = d[lo, :]
        d[:, hi] = d[:, lo]
        d[hi, hi] = d[lo, hi] = d[hi, lo] = 0
    assert (d == d.T).all()
    arrs[0][5] = arrs[0][66] = arrs[0].min() - 400.0  # the pair the posterior sits on: the least risk
    grid = [(10.0, 0.5, 0.0, 1.0), (10.0, 0.5, 0.0, 0.0)]
    risk, pick = mbr_on_gpu(ops, arrs, uoff, dist, doff, grid)
    bits = risk.view(np.int64)
    assert (bits[:, 5] == bits[:, 66]).all() and (bits[:, 20] == bits[:, 21]).all()
    ref_risk, ref_pick = R.mbr(*arrs, uoff, dist, doff, grid)
    assert ref_pick[0, 0] == 5 and pick[0, 0] == 5
    check_mbr(risk, pick, ref_risk, uoff)


def test_mbr_non_finite_totals_have_no_weight(ops):
    rng = np.random.default_rng(35)
    sizes = [6, 4]
    uoff = np.array([0, 6, 10], np.int64)
    arrs = [rng.normal(0, 5, 10) + 30, None, None, rng.normal(0, 5, 10), None]
    arrs[0][1], arrs[3][2], arrs[0][4] = np.nan, np.inf, -np.inf
    arrs[0][6:] = np.nan  # the second group has no finite total: a uniform posterior
    dist, doff = random_blocks(rng, sizes)
    grid = [(10.0, 1.0, 0.0, 1.0)]
    risk, pick = mbr_on_gpu(ops, arrs, uoff, dist, doff, grid)
    check_mbr(risk, pick, R.mbr(*arrs, uoff, dist, doff, grid)[0], uoff)
    assert np.isfinite(risk).all()


# ---- end to end ----
@pytest.fixture(scope="module")
def lists():
    """the n-best text and the scores of a scorer fixture; the references are the first hypotheses with a few words edited"""
    from bayeslms_amd import nbest_wer as W
    z = np.load(os.path.join(GOLDEN, "scorer_tlm_ffn.npz"), allow_pickle=True)
    nbest, nn = {}, {}
    for ln in str(z["nbest_txt"]).splitlines():
        key, _, hyp = ln.strip().partition(" ")
        nbest.setdefault(key.rsplit("-", 1)[0], []).append(hyp if hyp else " ")
    for ln in str(z["scores_txt"]).splitlines():
        key, v = ln.split()
        nn[key] = float(v)
    refs = {}
    for k, (u, hyps) in enumerate(nbest.items()):
        words = hyps[0].split()
        if k % 2 == 0:
            words = words + ["w003"]      # a deletion for every hypothesis that lacks it
        if k % 3 == 1 and words:
            words[0] = "w028"             # a substitution
        refs[u] = words
    refs["utt9-A"] = ["w002", "w003"]     # a reference without a list
    ac = {key: 2.5 * len(nbest[key.rsplit("-", 1)[0]][int(key.rsplit("-", 1)[1]) - 1].split()) + 1.0 for key in nn}
    lm = {key: 0.5 * v + 3.0 for key, v in nn.items()}
    nn2 = {key: v + (0.75 if key.endswith("-1") else 0.0) for key, v in nn.items()}
    return W, nbest, refs, {"ac": ac, "g": None, "lm": lm, "nn": [("mean", nn), ("mc8", nn2)]}


@pytest.mark.parametrize("mode", ["present", "all"])
def test_evaluate_report_equals_the_reference_field_by_field(lists, mode):
    W, nbest, refs, costs = lists
    grid = W.make_grid([7.0, 10.0, 13.0], [0.0, 0.5, 1.0], [0.0, 0.5])
    kw = dict(mode=mode, ignore_words={"zzz"}, mbr=True, budget_bytes=80)
    got = W.evaluate(nbest, refs, costs, grid, device=DEV, **kw)
    want = W.evaluate(nbest, refs, costs, grid, device="cpu", backend=R.Backend(), **kw)
    g, w = got.to_dict(), want.to_dict()
    assert list(g) == list(w) and g["utterances"] == w["utterances"] == (5 if mode == "all" else 4)
    for k in ("ref_words", "first", "oracle", "systems"):
        assert g[k] == w[k], k
    assert g["oracle"]["err"] <= min(s["best"]["err"] for s in g["systems"]) <= g["first"]["err"] + 10
    for mg, mw in zip(g["mbr"], w["mbr"]):
        assert {k: v for k, v in mg.items() if k != "mean_risk"} == {k: v for k, v in mw.items() if k != "mean_risk"}
        assert abs(mg["mean_risk"] - mw["mean_risk"]) <= bound(3) * mw["mean_risk"]
    for k in want.picks:
        if not k.endswith("mbr_risk"):
            assert got.picks[k] == want.picks[k], k


def test_command_line_writes_a_report_and_transcripts_that_round_trip(lists, tmp_path, capsys):
    import json
    from bayeslms_amd import wer as CLI
    W, nbest, refs, costs = lists
    with open(tmp_path / "words_text", "w") as f:
        for u, hyps in nbest.items():
            for n, h in enumerate(hyps, 1):
                f.write(("%s-%d %s" % (u, n, h)).rstrip() + "\n")
    with open(tmp_path / "text", "w") as f:
        for u, words in refs.items():
            f.write(" ".join([u] + words) + "\n")
    for name, arch in (("acwt", costs["ac"]), ("lmwt.lmonly", costs["lm"]), ("lmwt.nn", costs["nn"][0][1]), ("lmwt.nn.mc8", costs["nn"][1][1])):
        with open(tmp_path / name, "w") as f:
            for key, v in arch.items():
                f.write("%s %r\n" % (key, v))
    (tmp_path / "ignore").write_text("zzz\n")
    p = lambda n: str(tmp_path / n)
    rep = CLI.main(["--words-text", p("words_text"), "--ref-text", p("text"), "--acwt", p("acwt"), "--lmonly", p("lmwt.lmonly"),
                    "--nn", p("lmwt.nn"), "--nn", p("lmwt.nn.mc8"), "--lmwt", "7:13:3", "--nnweight", "0:1:0.5", "--wip", "0,0.5",
                    "--mbr", "1", "--ignore-words", p("ignore"), "--write-report", p("r.json"), "--write-best", p("best.txt"),
                    "--write-utt", p("utt.txt")])
    named = dict(costs, nn=[("lmwt.nn", costs["nn"][0][1]), ("lmwt.nn.mc8", costs["nn"][1][1])])  # a file's base name is its name
    want = W.evaluate(nbest, refs, named, W.make_grid([7.0, 10.0, 13.0], [0.0, 0.5, 1.0], [0.0, 0.5]), ignore_words={"zzz"},
                      mbr=True, device="cpu", backend=R.Backend())
    d = json.load(open(p("r.json")))
    assert d["systems"] == json.loads(json.dumps(want.to_dict()["systems"])) and [s["name"] for s in d["systems"]] == ["lmwt.nn", "lmwt.nn.mc8"]
    best = W.read_text(p("best.txt"))  # the transcripts round-trip: the chosen hypotheses, word for word
    assert list(best) == rep.utts and best == {u: nbest[u][k].split() for u, k in zip(rep.utts, rep.picks["lmwt.nn/mbr"])}
    assert len(open(p("utt.txt")).read().splitlines()) == 4
    assert "4 utterances" in capsys.readouterr().out
