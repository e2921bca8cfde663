"""GPU: the gradient-boosted tree kernels (csrc/gbdt.hip), GBDT and LambdaMART against the numpy restatement tests/gbdt_ref.py, fed the same
fp32 inputs.  Everything a tree decides rests on integer sums, so the comparisons are exact: bins, fixed-point values, histograms, split
records, partitions, tree structures, fp32 leaf values, scores and predictions are compared bit for bit, and the float64 gain to 1e-12
relative.  The last section pins whole fits to an implementation from outside the project: scikit-learn's trees, read from
tests/golden/gbdt_sklearn.npz (tests/gbdt_sk.py; scikit-learn itself is not needed here).  Nothing here is compared with LightGBM: it is not
installed where this runs, and the quantile binning rule and the tie rules are this project's own."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gbdt_ref as R
import gbdt_sk as SK
from launch_form import launch_form

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def padded(bins):
    """[n, F] uint8 -> the device layout [n, round_up(F, 16)], pad columns 0."""
    n, nf = bins.shape
    out = np.zeros((n, (nf + 15) // 16 * 16), np.uint8)
    out[:, :nf] = bins
    return dev(out)


# ---------------------------------------------------------------- ptr_gbdt_bin
@pytest.mark.parametrize("nf,n,max_bin", [(1, 1, 2), (3, 63, 15), (3, 64, 16), (136, 65, 63), (700, 64, 255), (3, 1000, 256), (136, 1000, 255),
                                          (1, 65, 256), (700, 63, 16)])
def test_bin_is_exact(nf, n, max_bin):
    from ptranking_amd import functional as F
    rng = np.random.default_rng(nf * 1000 + n)
    base = rng.standard_normal((max(n, 300), nf)).astype(np.float32)
    base[:, 0] = np.float32(1.25)                                                    # a constant column (when it is the only one: one bin)
    if nf > 1:
        base[:, 1] = rng.integers(0, 5, base.shape[0])                               # few distinct values: lossless bins
    edges, nbins = R.bin_edges(base, max_bin)
    X = base[:n].copy()
    k = 0
    for f in range(nf):                                                              # values exactly on edges, below the first, above the last
        for v in list(edges[f, :nbins[f] - 1][:3]) + [np.float32(-1e30), np.float32(1e30)]:
            X[k % n, f] = v
            k += 1
    got = F.gbdt_bin(dev(X), dev(edges), dev(nbins)).cpu().numpy()
    assert got.shape == (n, (nf + 15) // 16 * 16) and not got[:, nf:].any()
    assert np.array_equal(got[:, :nf], R.bin_matrix(X, edges, nbins))


# ---------------------------------------------------------------- ptr_gbdt_quantize
def _quant_case(name):
    rng = np.random.default_rng(23)
    if name == "span":
        n = 5000
        g = (np.ldexp(1.0, rng.integers(-30, 21, n)) * rng.uniform(0.5, 1.0, n) * rng.choice([-1, 1], n)).astype(np.float32)
        g[7], g[9] = np.float32(2.0 ** 20), np.float32(2.0 ** -30)
        return g, (rng.random(n) * 3).astype(np.float32)
    if name == "zero":
        return np.zeros(100, np.float32), np.zeros(100, np.float32)
    if name == "single":
        return np.array([-0.0037], np.float32), np.array([0.21], np.float32)
    if name == "blocks":
        g = rng.standard_normal(70001).astype(np.float32)
        g[70000] = 9.5                                                               # the maximum sits in the last reduction block
        return g, rng.random(70001).astype(np.float32)
    if name == "halves":                                                             # x.5 after scaling: ties go to even
        return np.array([0.5, 1.5, 2.5, -3.5, 2.0 ** 29], np.float32) / np.float32(2.0 ** 29) * 3, np.ones(5, np.float32)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["span", "zero", "single", "blocks", "halves"])
def test_quantize_is_exact(name):
    from ptranking_amd import functional as F
    g, h = _quant_case(name)
    qg, qh, expo, flag = F.gbdt_quantize(dev(g), dev(h))
    rg, rh, rexpo, rflag = R.quantize(g, h)
    assert tuple(expo.tolist()) == rexpo and int(flag) == rflag == 0
    assert np.array_equal(qg.cpu().numpy(), rg) and np.array_equal(qh.cpu().numpy(), rh)
    if name != "zero":
        assert 2 ** 29 <= np.abs(rg.astype(np.int64)).max() < 2 ** 30


def test_quantize_flags_a_nan_and_clamps_nothing():
    from ptranking_amd import functional as F
    g, h = _quant_case("blocks")
    g[12345] = np.nan
    h[3] = np.inf
    qg, qh, expo, flag = F.gbdt_quantize(dev(g), dev(h))
    rg, rh, rexpo, rflag = R.quantize(g, h)
    assert int(flag) == rflag == 1 and tuple(expo.tolist()) == rexpo
    assert np.array_equal(qg.cpu().numpy(), rg) and np.array_equal(qh.cpu().numpy(), rh)
    F.gbdt_quantize(dev(np.ones(4, np.float32)), dev(np.ones(4, np.float32)), flag=flag)
    assert int(flag) == 1                                                            # sticky until the caller clears it


# ---------------------------------------------------------------- ptr_gbdt_histogram
N_ROWS = 70000


@functools.lru_cache(maxsize=None)
def hist_data(nf, max_bin, n=N_ROWS, extreme=False):
    rng = np.random.default_rng(nf * 7 + max_bin)
    bins = rng.integers(0, max_bin, (n, nf)).astype(np.uint8)
    bins[:, 0] = max_bin - 1                                                         # a constant feature: every lane on one bin
    if nf > 1:
        bins[:, 1] = np.arange(n) % max_bin                                          # a ramp: consecutive rows walk the bins
    if extreme:
        qg = np.where(rng.random(n) < 0.7, 2 ** 30 - 1, -(2 ** 30 - 1)).astype(np.int32)
        qh = np.full(n, 2 ** 30 - 1, np.int32)
    else:
        qg = rng.integers(-2 ** 30 + 1, 2 ** 30, n).astype(np.int32)
        qh = rng.integers(0, 2 ** 30, n).astype(np.int32)
    return bins, qg, qh, padded(bins), dev(qg), dev(qh)


def row_list(m, order, n=N_ROWS):
    rng = np.random.default_rng(m + 1)
    rows = (rng.permutation(n)[:m] if m <= n else rng.integers(0, n, m)).astype(np.int32)      # a list longer than the matrix repeats rows
    return np.sort(rows) if order == "sorted" else rows


def form_name(m, nf, max_bin):
    kind, tile, tiles, chunks, lds = launch_form("ptr_gbdt_histogram", m, nf, max_bin)[:5]
    assert tile == 16 and tiles == (nf + 15) // 16
    return {0: "none", 1: "direct", 2: "lds-1-chunk" if chunks == 1 else "lds-chunks"}[kind]


# (rows, order, F, max_bin): the row counts around the direct form's bound (256) and the block size, the feature counts around the tile of
# 16, every max_bin of the issue; n = 70 000 rows span several chunks of the LDS form
HIST_CASES = [(m, "random", 29, 16) for m in (0, 1, 2, 63, 64, 65, 255, 256, 257, 1000)] + \
             [(m, "sorted", 17, 255) for m in (1, 64, 256, 257, 1000)] + \
             [(1000, "random", nf, 16) for nf in (1, 3, 15, 16, 17, 27, 28, 32, 33)] + \
             [(300, "random", 136, 256), (300, "sorted", 700, 255), (200, "random", 700, 256), (4100, "random", 136, 255)] + \
             [(1000, "random", 17, mb) for mb in (2, 255, 256)] + \
             [(70000, "random", 3, 256), (70000, "sorted", 29, 255), (70000, "random", 17, 2), (70000, "random", 33, 16)]


@pytest.mark.parametrize("m,order,nf,max_bin", HIST_CASES)
def test_histogram_is_integer_exact(m, order, nf, max_bin):
    from ptranking_amd import functional as F
    bins, qg, qh, dbins, dqg, dqh = hist_data(nf, max_bin)
    rows = row_list(m, order)
    form_name(m, nf, max_bin)
    got = F.gbdt_histogram(dbins, dqg, dqh, dev(rows) if m else torch.zeros(0, dtype=torch.int32, device="cuda"), nf, max_bin)
    want = R.histogram(bins, qg, qh, rows, max_bin)
    assert np.array_equal(got.cpu().numpy(), want)
    if m:
        assert got[0, max_bin - 1, 2].item() == m and got[0, :max_bin - 1].abs().sum().item() == 0          # the constant feature


def test_histogram_cases_reach_every_form():
    forms = {form_name(m, nf, mb) for m, _, nf, mb in HIST_CASES}
    assert forms == {"none", "direct", "lds-1-chunk", "lds-chunks"}
    assert form_name(256, 29, 16) == "direct" and form_name(257, 29, 16) == "lds-1-chunk" and form_name(70000, 3, 256) == "lds-chunks"


def test_histogram_all_rows_without_a_list_and_extreme_gradients():
    """rows=None is the root's list 0 .. n - 1; every qg = +-(2^30 - 1) on 70 000 rows: the int64 sums are far beyond int32."""
    from ptranking_amd import functional as F
    bins, qg, qh, dbins, dqg, dqh = hist_data(3, 256, extreme=True)
    got = F.gbdt_histogram(dbins, dqg, dqh, None, 3, 256)
    want = R.histogram(bins, qg, qh, None, 256)
    assert np.array_equal(got.cpu().numpy(), want) and abs(int(want[0, 255, 0])) > 2 ** 40 and int(want[0, 255, 1]) == N_ROWS * (2 ** 30 - 1)
    part = F.gbdt_histogram(dbins, dqg, dqh, None, 3, 256, m=1000)
    assert np.array_equal(part.cpu().numpy(), R.histogram(bins, qg, qh, np.arange(1000), 256))


@pytest.mark.parametrize("m", [200, 5000])
def test_histogram_adds_splits_and_repeats(m):
    from ptranking_amd import functional as F
    bins, qg, qh, dbins, dqg, dqh = hist_data(29, 255)
    rows = row_list(m, "random")
    drows = dev(rows)
    once = F.gbdt_histogram(dbins, dqg, dqh, drows, 29, 255)
    assert torch.equal(once, F.gbdt_histogram(dbins, dqg, dqh, drows, 29, 255))                 # repeated launches: the same bits
    start = torch.randint(-2 ** 40, 2 ** 40, (29, 255, 3), device="cuda", dtype=torch.int64)
    acc = F.gbdt_histogram(dbins, dqg, dqh, drows, 29, 255, hist=start.clone())
    assert torch.equal(acc, start + once)                                                       # adds, does not overwrite
    halves = F.gbdt_histogram(dbins, dqg, dqh, drows[:m // 3].contiguous(), 29, 255)
    F.gbdt_histogram(dbins, dqg, dqh, drows[m // 3:].contiguous(), 29, 255, hist=halves)
    assert torch.equal(halves, once)                                                            # two parts (of either form) = one launch
    # ptr_gbdt_hist_sub: the sibling = parent - child, exactly; in place too
    child = F.gbdt_histogram(dbins, dqg, dqh, drows[:m // 3].contiguous(), 29, 255)
    sib = F.gbdt_hist_sub(once, child)
    assert np.array_equal(sib.cpu().numpy(), R.histogram(bins, qg, qh, rows[m // 3:], 255))
    parent = once.clone()
    F.gbdt_hist_sub(parent, child, out=parent)
    assert torch.equal(parent, sib)


# ---------------------------------------------------------------- ptr_gbdt_best_split
def leaf_hists(seed, leaves, nf, max_bin, rows_per_leaf, signed_hessians=False, twin=False):
    """Histograms of `leaves` random leaves, built from rows (so every feature of a leaf holds the same totals)."""
    rng = np.random.default_rng(seed)
    nbins = rng.integers(2, max_bin + 1, nf).astype(np.int32)
    nbins[0] = max_bin
    if nf > 2:
        nbins[2] = 1                                                                 # a constant feature: never split
    hists = np.zeros((leaves, nf, max_bin, 3), np.int64)
    for l in range(leaves):
        m = int(rng.integers(rows_per_leaf // 2, rows_per_leaf + 1))
        bins = (rng.integers(0, 1 << 30, (m, nf)) % nbins[None, :]).astype(np.uint8)
        if twin and nf > 1:
            bins[:, 1] = bins[:, 0]
            nbins[1] = nbins[0]
        qg = rng.integers(-2 ** 29, 2 ** 29, m).astype(np.int32)
        qh = rng.integers(-2 ** 27 if signed_hessians else 2 ** 20, 2 ** 29, m).astype(np.int32)
        R.histogram(bins, qg, qh, None, max_bin, hists[l])
    return hists, nbins


def check_splits(hists, nbins, expo, **kw):
    from ptranking_amd import functional as F
    rec = F.gbdt_best_split(dev(hists), dev(nbins), dev(np.array(expo, np.int32)), kw.get("l2", 0.0), kw.get("min_data", 1), kw.get("min_hess", 1e-3),
                            kw.get("min_gain", 0.0)).cpu().numpy()
    refs = [R.best_split(h, nbins, expo, kw.get("l2", 0.0), kw.get("min_data", 1), kw.get("min_hess", 1e-3), kw.get("min_gain", 0.0)) for h in hists]
    for l, s in enumerate(refs):
        want = R.record(s)
        assert np.array_equal(rec[l, 1:], want[1:]), (l, rec[l], want)
        got_gain = rec[l, :1].view(np.float64)[0]
        if s["gain"] > -np.inf:
            assert abs(got_gain - s["gain"]) <= 1e-12 * abs(s["gain"]), (l, got_gain, s["gain"])
        else:
            assert got_gain == -np.inf
    return refs


@pytest.mark.parametrize("leaves,nf,max_bin,rows", [(1, 1, 256, 400), (5, 136, 255, 300), (400, 136, 64, 60), (5, 700, 256, 200), (1, 700, 16, 50),
                                                    (400, 1, 2, 30)])
def test_best_split_matches_the_restatement(leaves, nf, max_bin, rows):
    expo = (12, 9)
    for seed in range(50):                                       # the screen: a condition on the inputs, decided by the restatement alone
        hists, nbins = leaf_hists(seed * 101 + leaves, leaves, nf, max_bin, rows)
        screen = [R.margin(R.best_split(h, nbins, expo, 0.5, 3, 1e-3, 0.0)) for h in hists]
        if min(screen) > 1e-9:
            break
    assert min(screen) > 1e-9
    refs = check_splits(hists, nbins, expo, l2=0.5, min_data=3)
    assert any(s["gain"] > -np.inf for s in refs)


def test_best_split_constraints_bind_one_at_a_time():
    expo = (12, 9)
    hists, nbins = leaf_hists(5, 5, 40, 64, 300)
    free = check_splits(hists, nbins, expo, min_data=1, min_hess=0.0)
    # min_data_in_leaf: one more than the free choice's smaller child
    for l, s in enumerate(free):
        need = min(s["left"][2], s["right"][2]) + 1
        bound = check_splits(hists[l:l + 1], nbins, expo, min_data=need, min_hess=0.0)[0]
        assert (bound["feature"], bound["bin"]) != (s["feature"], s["bin"]) and bound["gain"] <= s["gain"]
        if bound["gain"] > -np.inf:
            assert min(bound["left"][2], bound["right"][2]) >= need
        # min_gain_to_split: just above the best gain leaves nothing; just below keeps it
        assert check_splits(hists[l:l + 1], nbins, expo, min_hess=0.0, min_gain=s["gain"] * (1 + 1e-9))[0]["gain"] == -np.inf
        assert check_splits(hists[l:l + 1], nbins, expo, min_hess=0.0, min_gain=s["gain"] * (1 - 1e-9))[0]["gain"] == s["gain"]
        # min_sum_hessian_in_leaf: one unit above the free choice's smaller Hessian sum
        small_h = np.ldexp(float(min(s["left"][1], s["right"][1]) + 1), -expo[1])
        bound = check_splits(hists[l:l + 1], nbins, expo, min_hess=small_h)[0]
        assert (bound["feature"], bound["bin"]) != (s["feature"], s["bin"])
    # no valid split at all: -inf, feature and bin -1, zero sums
    none = check_splits(hists, nbins, expo, min_data=10 ** 6)
    assert all(s["gain"] == -np.inf and s["feature"] == -1 for s in none)


def test_best_split_hessian_floor_with_negative_hessian_sums():
    """hessian='reference' gives rank-signed Hessians: prefix sums can be negative or zero.  Such candidates never divide: they are invalid
    under the floor max(min_sum_hessian_in_leaf, 2^-40)."""
    expo = (12, 9)
    hists, nbins = leaf_hists(9, 5, 40, 64, 40, signed_hessians=True)
    pre = np.cumsum(hists, axis=2)
    assert (pre[..., 1] < 0).any() and ((pre[:, :, -1:, 1] - pre[..., 1]) < 0).any()
    refs = check_splits(hists, nbins, expo, min_hess=0.0, min_data=1)
    for s in refs:
        if s["gain"] > -np.inf:
            assert s["left"][1] > 0 and s["right"][1] > 0
    assert any(s["gain"] > -np.inf for s in refs)


def test_best_split_exact_ties_go_to_the_lower_feature_then_the_lower_bin():
    expo = (12, 9)
    hists, nbins = leaf_hists(13, 5, 8, 32, 200, twin=True)
    hists[:, 2:] = 0                                                                 # only the two identical columns can split
    hists[:, 2:, 0, :] = hists[:, :1].sum(axis=2)                                      # (their rows all sit in bin 0)
    refs = check_splits(hists, nbins, expo)
    assert all(s["feature"] == 0 for s in refs)
    # an empty bin repeats its left neighbour's prefix sums: two equal gains within one feature, the lower bin wins
    l = next(i for i, s in enumerate(refs) if s["bin"] <= 29)
    b = refs[l]["bin"]
    h = hists[l:l + 1, :1].copy()
    h[:, :, b + 2] += h[:, :, b + 1]
    h[:, :, b + 1] = 0
    tied, _, _ = R.gains(h[0], nbins[:1], expo, 0.0, 1, 1e-3, 0.0)
    assert tied[0, b] == tied[0, b + 1] == tied.max()
    assert check_splits(h, nbins[:1], expo)[0]["bin"] == b


# ---------------------------------------------------------------- ptr_gbdt_partition
# 256 * 1024 + 1025 entries are 258 workgroups: a thread of the scan over their counts owns two of them, and the last threads own none
@pytest.mark.parametrize("m", [0, 1, 64, 65, 1000, 1024, 1025, 70000, 256 * 1024 + 1025])
def test_partition_is_stable_and_exact(m):
    from ptranking_amd import functional as F
    bins, _, _, dbins, _, _ = hist_data(29, 16)
    rows = row_list(m, "random")
    for feature, b in ((5, 7), (1, 3), (0, 14), (0, 15), (7, 0)):                      # feature 0 is constant at bin 15: all right, all left
        out, lc = F.gbdt_partition(dbins, dev(rows) if m else torch.zeros(0, dtype=torch.int32, device="cuda"), feature, b, 29)
        want, cl = R.partition(bins, rows, feature, b)
        assert int(lc) == cl and np.array_equal(out.cpu().numpy(), want), (feature, b)
    if m:
        assert R.partition(bins, rows, 0, 14)[1] == 0 and R.partition(bins, rows, 0, 15)[1] == m


# ---------------------------------------------------------------- whole trees
def ranking_set(seed, queries, lo, hi, nf=20):
    """Planted linear + interaction relevance, an MSLR-like label mix."""
    rng = np.random.default_rng(seed)
    group = rng.integers(lo, hi + 1, queries)
    group[0], group[1] = lo, hi                                                      # both ends of the length range, always
    n = int(group.sum())
    X = rng.standard_normal((n, nf)).astype(np.float32)
    X[:, 3] = np.round(X[:, 3] * 2) / 2                                              # a feature of few distinct values
    w = np.random.default_rng(99).standard_normal(nf)
    s = X @ w / np.sqrt(nf) + 0.8 * X[:, 0] * X[:, 1] + 0.5 * rng.standard_normal(n)
    y = np.digitize(s, np.quantile(s, [0.52, 0.84, 0.97, 0.99])).astype(np.float32)
    return X, y, group


def drive_rounds(seed, queries, lo, hi, rounds, params, objective="lambdarank", hessian="sum"):
    """GBDT.update and the restatement under the SAME device gradients every round (the device's tree_pair_grad_hess at the device's current
    scores).  -> the smallest margin of any split search (the screen), and the comparisons to make."""
    import ptranking_amd as pa
    from ptranking_amd import tree as T
    X, y, group = ranking_set(seed, queries, lo, hi)
    lm = pa.LambdaMART(params, objective=objective, hessian=hessian)
    res = T._Resident(y, group, torch.device("cuda"))
    booster = pa.GBDT(params, X)
    p = booster.params
    edges, nbins = R.bin_edges(X, p["max_bin"])
    assert np.array_equal(edges, booster.edges) and np.array_equal(nbins, booster.nbins)
    bins = R.bin_matrix(X, edges, nbins)
    assert np.array_equal(booster.bins.cpu().numpy()[:, :X.shape[1]], bins)
    scores = np.zeros(X.shape[0], np.float32)
    worst, checks = np.inf, []
    for _ in range(rounds):
        g, h = lm.grad_hess(booster.scores, res)
        got = booster.update(g, h)
        qg, qh, expo, flag = R.quantize(g.cpu().numpy(), h.cpu().numpy())
        assert flag == 0
        want, leaf_rows, margin = R.grow_tree(bins, qg, qh, expo, edges, nbins, p["max_bin"], p["num_leaves"], p["learning_rate"], p["lambda_l2"],
                                              p["min_data_in_leaf"], p["min_sum_hessian_in_leaf"], p["min_gain_to_split"], p["max_depth"])
        worst = min(worst, margin)
        scores = R.add_leaf_values(scores, leaf_rows, want["value"])
        checks.append((got, want, booster.scores.cpu().numpy().copy(), scores.copy()))
    return worst, checks, booster, X


def assert_rounds_equal(checks):
    for got, want, dev_scores, ref_scores in checks:
        for k in ("feature", "left", "right"):
            assert np.array_equal(got[k], want[k]), k                                # the structure
        assert np.array_equal(got["threshold"].view(np.int32), want["threshold"].view(np.int32))
        assert np.array_equal(got["value"].view(np.int32), want["value"].view(np.int32))           # leaf values equal as fp32
        assert np.array_equal(dev_scores.view(np.int32), ref_scores.view(np.int32))                # training scores: bit-identical


def screened(run):
    """Redraws the seed until the restatement's own margins pass the screen, and asserts that they do."""
    for seed in range(20):
        worst, checks, booster, X = run(seed)
        if worst > 1e-9:
            break
    assert worst > 1e-9
    return checks, booster, X


TREE_PARAMS = {"num_leaves": 8, "learning_rate": 0.1, "min_data_in_leaf": 5, "max_bin": 63, "lambda_l2": 0.1}


@pytest.fixture(scope="module")
def five_rounds():
    return screened(lambda seed: drive_rounds(seed, 40, 5, 130, 5, TREE_PARAMS))


def test_whole_trees_match_the_restatement(five_rounds):
    checks, booster, X = five_rounds
    assert_rounds_equal(checks)
    assert all(c[0]["feature"].size == 7 for c in checks)                            # 8 leaves each: the data allow it


def test_deep_leafwise_growth_matches():
    """num_leaves 400 on about 3 000 documents, one round: many small leaves, leaves that cannot split any more, the direct histogram form."""
    params = dict(TREE_PARAMS, num_leaves=400, min_data_in_leaf=3, max_bin=255)
    checks, booster, X = screened(lambda seed: drive_rounds(seed, 45, 5, 130, 1, params))
    assert 2000 <= X.shape[0] <= 4200
    assert_rounds_equal(checks)
    assert checks[0][0]["feature"].size > 100


def test_max_depth_limits_the_tree():
    params = dict(TREE_PARAMS, num_leaves=64, max_depth=3)
    checks, booster, X = screened(lambda seed: drive_rounds(seed, 40, 5, 130, 2, params))
    assert_rounds_equal(checks)
    assert all(c[0]["feature"].size <= 7 for c in checks)


def test_reference_hessian_trees_match():
    """The rank-signed Hessian: negative sums meet the Hessian floor inside whole trees."""
    checks, booster, X = screened(lambda seed: drive_rounds(seed, 40, 5, 130, 2, TREE_PARAMS, hessian="reference"))
    assert_rounds_equal(checks)


# ---------------------------------------------------------------- ptr_gbdt_predict
def test_predict_equals_training_scores_and_the_tree_walk(five_rounds, tmp_path):
    import ptranking_amd as pa
    checks, booster, X = five_rounds
    assert torch.equal(booster.predict(X), booster.scores)                           # the training matrix: the resident scores, bit for bit
    assert torch.equal(booster.predict(X, num_iteration=2), torch.from_numpy(checks[1][2]).cuda())
    rng = np.random.default_rng(4)
    path = tmp_path / "model.npz"
    booster.save_model(path)
    loaded = pa.GBDT.load_model(path)
    for n in (1, 65, 5000):
        fresh = (rng.standard_normal((n, X.shape[1])) * 1.5).astype(np.float32)
        fresh[0, :] = booster.trees[0]["threshold"][0]                               # a value exactly on a threshold goes left
        got = booster.predict(fresh)
        assert np.array_equal(got.cpu().numpy().view(np.int32), R.predict(fresh, booster.trees).view(np.int32))
        assert torch.equal(loaded.predict(fresh), got)                               # a saved and reloaded model: the same bits
    part = booster.predict(X[:100], num_iteration=4, first_tree=2).cpu().numpy()
    assert np.array_equal(part.view(np.int32), R.predict(X[:100], booster.trees[2:4]).view(np.int32))
    assert torch.equal(pa.GBDT({"num_leaves": 2}).predict(X[:5]), torch.zeros(5, device="cuda"))        # no tree: zeros


def test_add_leaf_values_one_launch_for_all_leaves():
    from ptranking_amd import functional as F
    rng = np.random.default_rng(8)
    n = 5000
    rows = rng.permutation(n).astype(np.int32)
    cuts = np.sort(rng.choice(np.arange(1, n), 6, replace=False))
    offsets = np.concatenate([[0], cuts, [n]]).astype(np.int32)
    offsets[3] = offsets[2]                                                          # an empty leaf
    values = rng.standard_normal(7).astype(np.float32)
    start = rng.standard_normal(n).astype(np.float32)
    got = F.gbdt_add_leaf_values(dev(start), dev(rows), dev(offsets), dev(values)).cpu().numpy()
    want = start.copy()
    for l in range(7):
        seg = rows[offsets[l]:offsets[l + 1]]
        want[seg] = want[seg] + values[l]
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


# ---------------------------------------------------------------- LambdaMART
FIT_PARAMS = {"num_leaves": 16, "learning_rate": 0.1, "min_data_in_leaf": 10, "num_trees": 30, "max_bin": 63}


@pytest.fixture(scope="module")
def fit_sets():
    return ranking_set(31, 200, 10, 60), ranking_set(32, 60, 10, 60)


@pytest.mark.parametrize("objective", ["lambdarank", "ranknet", "listnet"])
def test_lambdamart_learns_to_rank(fit_sets, objective):
    import ptranking_amd as pa
    (X, y, group), (Xv, yv, gv) = fit_sets
    lm = pa.LambdaMART(FIT_PARAMS, objective=objective).fit(X, y, group, eval_set=(Xv, yv), eval_group=gv, eval_at=5)
    assert len(lm.booster.trees) == 30 and len(lm.evals_result) == 30 and lm.best_iteration is None
    yv_d, y_d = dev(yv), dev(y)
    valid = lambda s: pa.LambdaMART.ndcg_at(s, yv_d, gv, 5)
    train = lambda s: pa.LambdaMART.ndcg_at(s, y_d, group, 5)
    after, one_tree, constant = valid(lm.predict(Xv)), valid(lm.predict(Xv, num_iteration=1)), valid(torch.zeros(Xv.shape[0], device="cuda"))
    print(f"{objective}: valid nDCG@5 constant {constant:.4f}, one tree {one_tree:.4f}, 30 trees {after:.4f}")
    assert after > constant and after > one_tree
    assert after == lm.evals_result[-1]                                              # the running validation scores are predict()'s bits
    first, last = train(lm.predict(X, num_iteration=1)), train(lm.booster.scores)
    print(f"{objective}: train nDCG@5 round 1 {first:.4f}, round 30 {last:.4f}")
    assert last >= first
    assert torch.equal(lm.predict(X), lm.booster.scores)


def test_early_stopping_and_best_iteration(fit_sets):
    import ptranking_amd as pa
    (X, y, group), (Xv, yv, gv) = fit_sets
    params = dict(FIT_PARAMS, num_trees=200, learning_rate=0.5, num_leaves=31, min_data_in_leaf=3)
    lm = pa.LambdaMART(params).fit(X[:1500], y[:1500], _groups_upto(group, 1500), eval_set=(Xv, yv), eval_group=gv, early_stopping_rounds=3)
    ran = len(lm.evals_result)
    assert ran < 200 and len(lm.booster.trees) == ran
    assert lm.best_iteration == int(np.argmax(lm.evals_result)) + 1 == ran - 3 and lm.best_score == max(lm.evals_result)
    assert torch.equal(lm.predict(Xv), lm.predict(Xv, num_iteration=lm.best_iteration))
    assert not torch.equal(lm.predict(Xv), lm.predict(Xv, num_iteration=ran))
    assert pa.LambdaMART.ndcg_at(lm.predict(Xv), dev(yv), gv, 5) == lm.best_score


def _groups_upto(group, n):
    """The leading queries that together hold exactly the first rows of a set (the last one cut short)."""
    out, left = [], n
    for g in group:
        if left <= 0:
            break
        out.append(min(int(g), left))
        left -= out[-1]
    return np.array(out)


def test_two_identical_fits_give_bit_identical_models(fit_sets):
    import ptranking_amd as pa
    (X, y, group), _ = fit_sets
    params = dict(FIT_PARAMS, num_trees=5)
    a = pa.LambdaMART(params).fit(X, y, group).booster
    b = pa.LambdaMART(params).fit(X, y, group).booster
    fa, fb = a.flat(), b.flat()
    for k in fa:
        assert fa[k].tobytes() == fb[k].tobytes(), k
    assert torch.equal(a.scores, b.scores)


def test_a_nan_gradient_raises():
    import ptranking_amd as pa
    X, y, group = ranking_set(2, 10, 5, 20)
    booster = pa.GBDT({"num_leaves": 4, "min_data_in_leaf": 2}, X)
    g = torch.randn(X.shape[0], device="cuda")
    g[3] = float("nan")
    with pytest.raises(FloatingPointError):
        booster.update(g, torch.ones_like(g))
    assert len(booster.trees) == 0
    booster.update(torch.nan_to_num(g), torch.ones_like(g))                          # the flag was cleared: the next round runs
    assert len(booster.trees) == 1


def test_run_letor_on_the_committed_sample():
    import ptranking_amd as pa
    one, zero = os.path.join(GOLD, "letor_sample.txt"), os.path.join(GOLD, "letor_sample_zero.txt")
    lm = pa.LambdaMART({"num_leaves": 4, "min_data_in_leaf": 1, "num_trees": 5, "max_bin": 16})
    y_test, group_test, y_pred = lm.run_letor(one, one, one)
    assert y_test.shape == y_pred.shape and int(group_test.sum()) == y_test.size and y_pred.dtype == np.float32
    assert len(lm.evals_result) == 5 and np.isfinite(y_pred).all()
    y2, g2, p2 = pa.LambdaMART({"num_leaves": 4, "min_data_in_leaf": 1, "num_trees": 3, "max_bin": 16}).run_letor(zero, one_indexed=False)
    assert y2.shape == p2.shape and int(g2.sum()) == y2.size


def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_lambdamart_native.py"), "--queries", "120", "--rounds", "20"], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("round ")]
    assert len(lines) == 2 and "nDCG@5" in lines[0], out.stdout
    assert float(lines[-1].split("valid nDCG@5 ")[1].split()[0]) > float(out.stdout.split("constant scores: valid nDCG@5 ")[1].split()[0])


# ---------------------------------------------------------------- whole fits against scikit-learn (tests/golden/gbdt_sklearn.npz)
SK_NAMES = ("a", "b", "c", "d", "e", "f")


@pytest.fixture(scope="module")
def sk_fits(tmp_path_factory):
    """Every fixture case fitted once: GBDT on the case's X, the scores set to sklearn's baseline, per round g = (scores - y) * w and h = w in
    fp32 on the device, then update.  Records what the tests compare, and the shape of every histogram launch."""
    import ptranking_amd as pa
    from ptranking_amd import functional as Fn
    cases, out = SK.load()[0], {}
    assert tuple(sorted(cases)) == SK_NAMES
    real = Fn.gbdt_histogram
    for name, c in cases.items():
        launches = []

        def spy(bins, qg, qh, rows, nf, max_bin, **kw):
            launches.append((bins.shape[0] if rows is None else rows.numel(), nf, max_bin))
            return real(bins, qg, qh, rows, nf, max_bin, **kw)

        p = c["params"]
        booster = pa.GBDT(SK.booster_params(p), c["X"])
        base = np.float32(c["baseline"])
        booster.scores.fill_(float(base))
        y, w = dev(c["y"]), dev(np.ones_like(c["y"]) if c["w"] is None else c["w"])
        rounds = []
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(Fn, "gbdt_histogram", spy)
            for _ in range(p["rounds"]):
                tree = booster.update((booster.scores - y) * w, w)
                rounds.append((tree, booster.scores.cpu().numpy().copy()))
        fresh = booster.predict(c["fresh"])
        path = tmp_path_factory.mktemp("sk") / f"{name}.npz"
        booster.save_model(path)
        reloaded = pa.GBDT.load_model(path).predict(c["fresh"])
        out[name] = dict(case=c, booster=booster, rounds=rounds, fresh=(fresh + float(base)).cpu().numpy(), same_bits=torch.equal(fresh, reloaded),
                         launches=launches)
    return out


@pytest.mark.parametrize("name", SK_NAMES)
def test_whole_fits_match_sklearn(sk_fits, name):
    """Cases a - e: HistGradientBoostingRegressor; case f: one DecisionTreeRegressor, the exact greedy best-first tree (g = -y, h = 1 from
    zero scores).  Trees equal in canonical form; training scores after every round and the fresh predictions within
    C_GBDT_SK 2^-24 max(1, max |score|), the constant being twice what the numpy restatement needs against sklearn (test_gbdt_cpu.py)."""
    fit = sk_fits[name]
    c, p = fit["case"], fit["case"]["params"]
    edges, nbins = SK.midpoint_edges(c["codes"], p["max_bin"])
    assert np.array_equal(fit["booster"].edges, edges) and np.array_equal(fit["booster"].nbins, nbins)     # the midpoints the codes imply
    assert len(fit["rounds"]) == p["rounds"]
    for r, (tree, scores) in enumerate(fit["rounds"]):
        nodes, leaves = SK.canonical(tree, c["X"])
        miss = SK.tree_mismatch(nodes, leaves, c, r)
        assert miss is None, f"round {r}: {miss}"
        err = float(np.abs(scores.astype(np.float64) - c["staged"][r]).max())
        print(f"MEASURED gbdt vs sklearn, case {name} round {r}: training scores need C >= {err / SK.need_unit(c['staged'][r]):.2f}")
        assert err <= SK.gate(c["staged"][r]), r
    err = float(np.abs(fit["fresh"].astype(np.float64) - c["fresh_pred"]).max())
    print(f"MEASURED gbdt vs sklearn, case {name}: {c['fresh'].shape[0]} fresh rows need C >= {err / SK.need_unit(c['fresh_pred']):.2f}")
    assert err <= SK.gate(c["fresh_pred"])
    assert fit["same_bits"]                                                          # a saved and reloaded model predicts the same bits


@pytest.mark.parametrize("name", SK_NAMES)
def test_whole_fits_equal_the_restatement_bit_for_bit(sk_fits, name):
    """The same fits against gbdt_ref.py: should a case miss sklearn, this says whether the kernels or the shared rules are at fault."""
    fit = sk_fits[name]
    want, fresh, _ = SK.run_restatement(fit["case"])
    assert_rounds_equal([(tree, ref_tree, scores, ref_scores) for (tree, scores), (ref_tree, ref_scores) in zip(fit["rounds"], want)])
    assert np.array_equal(fit["fresh"].view(np.int32), fresh.view(np.int32))


def test_sklearn_cases_reach_both_histogram_forms_and_several_feature_tiles(sk_fits):
    """From the histogram launches the fits really made: the case list cannot silently shrink onto one path."""
    forms = {name: {form_name(*shape) for shape in fit["launches"]} for name, fit in sk_fits.items()}
    tiles = {name: (fit["case"]["X"].shape[1] + 15) // 16 for name, fit in sk_fits.items()}
    assert set().union(*forms.values()) == {"direct", "lds-1-chunk"}
    assert forms["a"] == {"direct", "lds-1-chunk"} and forms["e"] == {"direct", "lds-1-chunk"}
    assert (tiles["a"], tiles["b"], tiles["d"], tiles["e"]) == (1, 2, 3, 1)
    for name, fit in sk_fits.items():
        n, nf = fit["case"]["X"].shape
        root = fit["launches"][0]
        assert root == (n, nf, fit["case"]["params"]["max_bin"]) and form_name(*root) == "lds-1-chunk"
        assert launch_form("ptr_gbdt_histogram", *root)[2] == tiles[name]
    assert sk_fits["e"]["launches"][0][0] == 257                                     # one row over the direct form's bound


# ---------------------------------------------------------------- non-finite features at prediction time
def _one_tree_booster():
    import ptranking_amd as pa
    X, y, group = ranking_set(2, 10, 5, 20)
    booster = pa.GBDT({"num_leaves": 4, "min_data_in_leaf": 2}, X)
    booster.update(dev(y - y.mean()) * -1.0, torch.ones(X.shape[0], device="cuda"))
    return booster, X


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_predict_raises_on_a_non_finite_feature(bad):
    booster, X = _one_tree_booster()
    assert torch.isfinite(booster.predict(X)).all()
    for i, f in ((0, 0), (X.shape[0] - 1, X.shape[1] - 1), (X.shape[0] // 2, 3)):        # first, last and an inner element
        Xb = X.copy()
        Xb[i, f] = bad
        with pytest.raises(ValueError, match="NaN or an infinity"):
            booster.predict(Xb)
        with pytest.raises(ValueError, match="NaN or an infinity"):
            booster.predict(dev(Xb))
    Xb = X.copy()
    Xb[0, 0], Xb[1, 0] = np.inf, -np.inf                                                 # both infinities, and a NaN beside them
    Xb[2, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or an infinity"):
        booster.predict(Xb)
    big = np.full((4, X.shape[1]), np.finfo(np.float32).max, np.float32)                 # finite, however large: no false alarm
    big[1] = -big[1]
    assert torch.isfinite(booster.predict(big)).all()
    assert booster.predict(np.zeros((0, X.shape[1]), np.float32)).numel() == 0


def test_fit_raises_on_a_non_finite_validation_feature_before_the_first_round(fit_sets):
    import ptranking_amd as pa
    (X, y, group), (Xv, yv, gv) = fit_sets
    Xb = Xv.copy()
    Xb[17, 2] = np.nan
    lm = pa.LambdaMART(dict(FIT_PARAMS, num_trees=2))
    with pytest.raises(ValueError, match="NaN or an infinity"):
        lm.fit(X, y, group, eval_set=(Xb, yv), eval_group=gv)
    assert lm.evals_result == [] and len(lm.booster.trees) == 0
    with pytest.raises(ValueError, match="NaN or an infinity"):
        lm.fit(X, y, group, eval_set=(dev(Xb), yv), eval_group=gv)
    lm.fit(X, y, group, eval_set=(Xv, yv), eval_group=gv)
    with pytest.raises(ValueError, match="NaN or an infinity"):
        lm.predict(Xb)


def test_fit_checks_the_validation_matrix_once_and_no_round_checks_again(fit_sets, monkeypatch):
    """The check synchronises, so fit makes it once before the first round; the per-round predict of the checked matrix skips it."""
    import ptranking_amd as pa
    from ptranking_amd import gbdt
    (X, y, group), (Xv, yv, gv) = fit_sets
    seen, real = [], gbdt._require_finite

    def spy(Xd):
        seen.append(tuple(Xd.shape))
        return real(Xd)

    monkeypatch.setattr(gbdt, "_require_finite", spy)
    lm = pa.LambdaMART(dict(FIT_PARAMS, num_trees=4)).fit(X, y, group, eval_set=(Xv, yv), eval_group=gv)
    assert len(lm.evals_result) == 4 and seen == [Xv.shape]
    lm.predict(Xv)
    assert seen == [Xv.shape, Xv.shape]
    lm.booster.predict(Xv, check_finite=False)
    assert len(seen) == 2
