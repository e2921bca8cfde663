"""GPU: depth-wise growth (grow_policy='depthwise') and the four batched entry points of a level (csrc/gbdt.hip).  Everything is compared
with the numpy restatement (tests/gbdt_level_ref.py, tests/gbdt_ref.py) or with the single-leaf entry points on the same inputs, and
integers are compared exactly.  Where the leaf cap cannot bind, depth-wise and leaf-wise growth must give the same trees in canonical
form with bit-equal fp32 leaf values and training scores; whole fits are pinned to scikit-learn's depth-limited trees through
tests/golden/gbdt_sklearn_depth.npz (scikit-learn itself is not needed here)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gbdt_level_ref as LR
import gbdt_ref as R
import gbdt_sk as SK
from launch_form import launch_form
from test_gbdt_gpu import FIT_PARAMS, TREE_PARAMS, _groups_upto, dev, hist_data, leaf_hists, ranking_set

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (0, 1, 255, 256, 257, 2048, 2049, 5000)
SENTINEL = -7_777_777_777


# ---------------------------------------------------------------- ptr_gbdt_histogram_segments
def segment_table(K, nslots, seed):
    """K segments with gaps between them, lengths cycling through LENS from a seeded offset, slots permuted and non-consecutive."""
    rng = np.random.default_rng(seed)
    lens = np.array([LENS[(i + seed) % len(LENS)] for i in range(K)])
    if K >= len(LENS):
        lens = rng.permutation(lens)
    gaps = rng.integers(0, 40, K)
    starts = np.cumsum(gaps + np.concatenate([[0], lens[:-1]]))
    slots = rng.permutation(nslots)[:K]
    return np.stack([starts, lens, slots], axis=1).astype(np.int64), int(starts[-1] + lens[-1] + 17)


@pytest.mark.parametrize("K,nf,max_bin", [(1, 1, 2), (2, 16, 63), (7, 17, 255), (64, 33, 256), (7, 136, 255), (64, 17, 63), (2, 136, 256), (64, 1, 255)])
def test_batched_histogram_is_integer_exact(K, nf, max_bin):
    from ptranking_amd import functional as F
    bins, qg, qh, dbins, dqg, dqh = hist_data(nf, max_bin)
    nslots = 2 * K + 3
    segs, nrows = segment_table(K, nslots, K + nf)
    if K == 1:
        segs[0, 1] = 5000
        nrows = int(segs[0, 0]) + 5000 + 3
    rng = np.random.default_rng(K * 1000 + nf)
    rows = rng.integers(0, bins.shape[0], nrows).astype(np.int32)
    drows = dev(rows)
    start = torch.full((nslots, nf, max_bin, 3), SENTINEL, device="cuda", dtype=torch.int64)
    start[dev(segs[:, 2])] = torch.randint(-2 ** 40, 2 ** 40, (K, nf, max_bin, 3), device="cuda", dtype=torch.int64)     # accumulation into non-zero slots
    pool = F.gbdt_histogram_segments(dbins, dqg, dqh, drows, segs, nf, max_bin, start.clone())
    again = F.gbdt_histogram_segments(dbins, dqg, dqh, drows, segs, nf, max_bin, start.clone())
    assert torch.equal(pool, again)                                                      # a repeat: the same bits
    listed = np.zeros(nslots, bool)
    for s, m, slot in segs:
        listed[slot] = True
        seg_rows = drows[s:s + m].contiguous()
        want = F.gbdt_histogram(dbins, dqg, dqh, seg_rows, nf, max_bin) if m else torch.zeros_like(start[0])
        assert torch.equal(pool[slot] - start[slot], want), (s, m, slot)                 # what ptr_gbdt_histogram gives for that row list
        if m in (1, 257) or (m == 5000 and nf <= 17):
            assert np.array_equal(want.cpu().numpy(), R.histogram(bins, qg, qh, rows[s:s + m], max_bin))
    assert bool((pool[dev(np.nonzero(~listed)[0])] == SENTINEL).all())                   # unlisted slots keep the sentinel exactly
    kinds = {launch_form("ptr_gbdt_histogram_segments", m, nf, max_bin, 0)[0] for m in segs[:, 1]}
    if K >= 7:
        assert kinds == {0, 1, 2}                                                        # empty, direct and LDS segments in ONE call
    items, nd, nl = F.gbdt_segment_items(segs[:, 1], nf, max_bin)
    assert nd == int(((segs[:, 1] > 0) & (segs[:, 1] <= 256)).sum()) and (nl > 0) == (2 in kinds)
    assert launch_form("ptr_gbdt_histogram_segments", 257, nf, max_bin, 0)[7] == 2       # at most two launches however many segments


def test_batched_histogram_chunks_long_segments_and_skips_bad_entries():
    from ptranking_amd import functional as F
    nf, max_bin = 17, 255
    bins, qg, qh, dbins, dqg, dqh = hist_data(nf, max_bin)
    n = bins.shape[0]
    rows = np.random.default_rng(3).permutation(n).astype(np.int32)
    drows = dev(rows)
    good = np.array([[0, 30000, 2], [30010, 200, 0], [31000, 39000, 5]])
    chunk = launch_form("ptr_gbdt_histogram_segments", 1, nf, max_bin, 69000)[5]
    assert launch_form("ptr_gbdt_histogram_segments", 39000, nf, max_bin, 69000)[3] == -(-39000 // chunk) > 1      # several row chunks
    bad = np.array([[60000, 20000, 1], [-5, 100, 1], [0, -3, 1], [100, 100, 6], [100, 100, -1], [2 ** 31 - 10, 5, 1], [100, 300, 600]])
    table = np.concatenate([bad[:3], good[:1], bad[3:5], good[1:], bad[5:]])
    pool = F.gbdt_histogram_segments(dbins, dqg, dqh, drows, table, nf, max_bin, torch.zeros((6, nf, max_bin, 3), device="cuda", dtype=torch.int64))
    for s, m, slot in good:
        assert np.array_equal(pool[slot].cpu().numpy(), R.histogram(bins, qg, qh, rows[s:s + m], max_bin))
    assert not pool[[1, 3, 4]].any()                                                     # the entries out of range were skipped, not followed
    # a row index out of range inside a good segment is skipped too, as in ptr_gbdt_histogram
    rows2 = rows.copy()
    rows2[[5, 40000]] = [-1, n]
    pool2 = F.gbdt_histogram_segments(dbins, dqg, dqh, dev(rows2), good, nf, max_bin, torch.zeros((6, nf, max_bin, 3), device="cuda", dtype=torch.int64))
    keep = lambda s, m: np.array([r for r in rows2[s:s + m] if 0 <= r < n], np.int32)
    assert np.array_equal(pool2[2].cpu().numpy(), R.histogram(bins, qg, qh, keep(0, 30000), max_bin))
    assert np.array_equal(pool2[5].cpu().numpy(), R.histogram(bins, qg, qh, keep(31000, 39000), max_bin))
    empty = F.gbdt_histogram_segments(dbins, dqg, dqh, drows, np.zeros((0, 3)), nf, max_bin, torch.ones((2, nf, max_bin, 3), device="cuda", dtype=torch.int64))
    assert bool((empty == 1).all())                                                      # K == 0: a successful no-op


# ---------------------------------------------------------------- ptr_gbdt_hist_sub_segments
@pytest.mark.parametrize("nf,max_bin", [(1, 2), (17, 255), (136, 256)])
def test_batched_subtraction_is_exact_and_may_alias_the_parent(nf, max_bin):
    from ptranking_amd import functional as F
    start = torch.randint(-2 ** 50, 2 ** 50, (12, nf, max_bin, 3), device="cuda", dtype=torch.int64)
    trips = np.array([[0, 1, 0], [2, 3, 2], [4, 5, 6], [7, 8, 7], [9, 10, 11], [0, 12, 3], [-1, 1, 5], [1, 2, 12]])      # the last three: out of range
    pool = F.gbdt_hist_sub_segments(start.clone(), trips)
    want = start.clone()
    for p, c, o in trips[:5]:
        want[o] = start[p] - start[c]
    assert torch.equal(pool, want)
    assert torch.equal(F.gbdt_hist_sub_segments(start.clone(), np.zeros((0, 3))), start)
    assert launch_form("ptr_gbdt_hist_sub_segments", 5)[0] == 1


# ---------------------------------------------------------------- ptr_gbdt_best_split_slots
@pytest.mark.parametrize("K,nf", [(1, 1), (5, 1), (64, 1), (1, 136), (5, 136), (64, 136)])
def test_best_split_over_slots_equals_the_contiguous_batch_bit_for_bit(K, nf):
    from ptranking_amd import functional as F
    max_bin, expo = 64, (12, 9)
    hists, nbins = leaf_hists(K * 7 + nf, K, nf, max_bin, 300)
    nslots = 2 * K + 1
    slots = np.random.default_rng(K).permutation(nslots)[:K]
    pool = torch.randint(-2 ** 30, 2 ** 30, (nslots, nf, max_bin, 3), device="cuda", dtype=torch.int64)
    pool[dev(slots)] = dev(hists)
    dn, de = dev(nbins), dev(np.array(expo, np.int32))
    free = F.gbdt_best_split(dev(hists), dn, de, 0.0, 1, 0.0, 0.0).cpu().numpy()
    gains = free[:, 0].copy().view(np.float64)
    assert (gains > -np.inf).any()
    small = np.minimum(free[:, 5], free[:, 8])
    small_h = np.minimum(free[:, 4], free[:, 7])
    settings = {"free": (0.0, 1, 0.0, 0.0), "l2": (0.5, 3, 1e-3, 0.0), "min_data": (0.0, int(small[gains > -np.inf].max()) + 1, 0.0, 0.0),
                "min_hess": (0.0, 1, float(np.ldexp(float(small_h[gains > -np.inf].max() + 1), -expo[1])), 0.0),
                "min_gain": (0.0, 1, 0.0, float(gains.max()) * (1 + 1e-9))}
    for name, (l2, md, mh, mg) in settings.items():
        want = F.gbdt_best_split(dev(hists), dn, de, l2, md, mh, mg)                     # on the gathered, contiguous copy
        got = F.gbdt_best_split_slots(pool, slots, dn, de, l2, md, mh, mg)
        assert torch.equal(got, want), name                                              # the gain's bits included
        if name in ("min_data", "min_hess", "min_gain"):
            assert not np.array_equal(want.cpu().numpy(), free), name                    # the constraint binds on some slot
    ref = R.record(R.best_split(hists[0], nbins, expo, 0.5, 3, 1e-3, 0.0))
    got = F.gbdt_best_split_slots(pool, slots[:1], dn, de, 0.5, 3, 1e-3, 0.0).cpu().numpy()[0]
    assert np.array_equal(got[1:], ref[1:])
    mixed = F.gbdt_best_split_slots(pool, [int(slots[0]), nslots, -1], dn, de).cpu().numpy()      # slots outside the pool: no split, nothing read
    assert np.array_equal(mixed[0], F.gbdt_best_split(dev(hists[:1]), dn, de).cpu().numpy()[0])
    for r in mixed[1:]:
        assert r[:1].view(np.float64)[0] == -np.inf and r[1:].tolist() == [-1, -1, 0, 0, 0, 0, 0, 0]
    assert F.gbdt_best_split_slots(pool, [], dn, de).shape == (0, 9)


# ---------------------------------------------------------------- ptr_gbdt_partition_segments
def test_batched_partition_is_stable_and_exact():
    from ptranking_amd import functional as F
    nf = 29
    bins, _, _, dbins, _, _ = hist_data(nf, 16)
    n = bins.shape[0]
    rng = np.random.default_rng(12)
    lens = np.concatenate([[0, 1, 1023, 1024, 1025, 70000, 2048, 4097], rng.integers(0, 300, 292)])
    K = lens.size
    assert K == 300
    gaps = rng.integers(0, 9, K)
    gaps[0] = 5
    starts = np.cumsum(gaps + np.concatenate([[0], lens[:-1]]))
    nrows = int(starts[-1] + lens[-1] + 11)
    feats, cuts = rng.integers(1, nf, K), rng.integers(0, 15, K)
    feats[[6, 7, 20, 21]], cuts[[6, 20]], cuts[[7, 21]] = 0, 15, 14                      # feature 0 is constant at bin 15: all left, all right
    segs = np.stack([starts, lens, feats, cuts], axis=1)
    rows = rng.integers(0, n, nrows).astype(np.int32)
    drows = dev(rows)
    out, lc = F.gbdt_partition_segments(dbins, drows, segs, nf)
    got, got_lc = out.cpu().numpy(), lc.cpu().numpy()
    want, inside = rows.copy(), np.zeros(nrows, bool)
    for k, (s, m, f, b) in enumerate(segs):
        part, cl = R.partition(bins, rows[s:s + m], f, b)
        want[s:s + m], inside[s:s + m] = part, True
        assert got_lc[k] == cl, k
    assert np.array_equal(got, want)                                                     # order exact, every segment with its own (feature, bin)
    assert (~inside).sum() > 0 and np.array_equal(got[~inside], rows[~inside])           # outside the segments: copied verbatim
    assert got_lc[6] == lens[6] and got_lc[7] == 0 and got_lc[0] == 0
    for k in (1, 3, 4, 5, 8):                                                            # each segment = ptr_gbdt_partition on it
        s, m, f, b = segs[k]
        single, single_lc = F.gbdt_partition(dbins, drows[s:s + m].contiguous(), int(f), int(b), nf)
        assert torch.equal(out[s:s + m], single) and int(single_lc) == got_lc[k]
    assert launch_form("ptr_gbdt_partition_segments", 70000)[:2] == (3, 69)              # a fixed number of launches; 1024 rows a workgroup
    again, _ = F.gbdt_partition_segments(dbins, drows, segs, nf)
    assert torch.equal(again, out)


def test_batched_partition_skips_bad_entries_and_serves_one_or_no_segment():
    from ptranking_amd import functional as F
    nf = 29
    bins, _, _, dbins, _, _ = hist_data(nf, 16)
    rows = np.random.default_rng(2).integers(0, bins.shape[0], 5000).astype(np.int32)
    drows = dev(rows)
    segs = np.array([[0, 1500, 5, 7], [1500, 6000, 5, 7], [1600, 100, nf, 3], [1700, 100, -1, 3], [1800, 100, 4, 256], [-4, 100, 4, 3], [2000, 2500, 3, 9]])
    out, lc = F.gbdt_partition_segments(dbins, drows, segs, nf)
    want = rows.copy()
    for k in (0, 6):
        s, m, f, b = segs[k]
        want[s:s + m], cl = R.partition(bins, rows[s:s + m], f, b)
        assert int(lc[k]) == cl
    assert np.array_equal(out.cpu().numpy(), want) and lc[1:6].tolist() == [0] * 5       # the bad entries changed nothing
    none, none_lc = F.gbdt_partition_segments(dbins, drows, np.zeros((0, 4)), nf)
    assert torch.equal(none, drows) and none_lc.numel() == 0                             # K == 0: out is still a whole row list
    one, one_lc = F.gbdt_partition_segments(dbins, drows, [[0, 5000, 1, 3]], nf)
    single, single_lc = F.gbdt_partition(dbins, drows, 1, 3, nf)
    assert torch.equal(one, single) and int(one_lc) == int(single_lc)
    with pytest.raises(RuntimeError, match="out must not be rows"):
        F.gbdt_partition_segments(dbins, drows, [[0, 10, 1, 3]], nf, out=drows)


# ---------------------------------------------------------------- whole trees
def drive(policy, seed, queries, lo, hi, rounds, params, hessian="sum"):
    """GBDT.update under a growth policy, fed LambdaMART's device gradients at the booster's own scores -> per round (tree, scores, g, h)."""
    import ptranking_amd as pa
    from ptranking_amd import tree as T
    X, y, group = ranking_set(seed, queries, lo, hi)
    params = dict(params, grow_policy=policy)
    lm = pa.LambdaMART(params, hessian=hessian)
    res = T._Resident(y, group, torch.device("cuda"))
    booster = pa.GBDT(params, X)
    out = []
    for _ in range(rounds):
        g, h = lm.grad_hess(booster.scores, res)
        before = booster.host_reads
        tree = booster.update(g, h)
        out.append(dict(tree=tree, scores=booster.scores.cpu().numpy().copy(), g=g.cpu().numpy(), h=h.cpu().numpy(), reads=booster.host_reads - before))
    return out, booster, X


def node_shape(tree, X):
    """Per node of a tree: (its depth, its two children's row counts), walking the training rows; and the tree's depth."""
    k = tree["feature"].size
    at, depth, kids = {0: np.arange(X.shape[0])}, np.zeros(max(k, 1), np.int64), np.zeros((k, 2), np.int64)
    for i in range(k):
        rows = at.pop(i)
        go_left = X[rows, tree["feature"][i]] <= tree["threshold"][i]
        for sd, (child, part) in enumerate(((int(tree["left"][i]), rows[go_left]), (int(tree["right"][i]), rows[~go_left]))):
            kids[i, sd] = part.size
            if child >= 0:
                at[child], depth[child] = part, depth[i] + 1
    return depth[:k], kids, (int(depth[:k].max()) + 1 if k else 0)


def leafwise_reads(tree, X, p):
    """The host reads of one leaf-wise update, from its loop: the root's, then one after every split whose children are searched — the tree
    can still grow (split k leaves k + 2 leaves) and a child is splittable."""
    depth, kids, _ = node_shape(tree, X)
    ok = lambda count, d: count >= 2 * max(p["min_data_in_leaf"], 1) and (p["max_depth"] <= 0 or d < p["max_depth"])
    return 1 + sum(1 for k in range(depth.size) if k + 2 < p["num_leaves"] and (ok(kids[k, 0], depth[k] + 1) or ok(kids[k, 1], depth[k] + 1)))


def assert_policies_agree(lw, dw, X):
    for a, b in zip(lw, dw):
        na, la = SK.canonical(a["tree"], X)
        nb, lb = SK.canonical(b["tree"], X)
        assert np.array_equal(na, nb) and np.array_equal(la, lb)                         # the structure; the fp32 leaf values as float64: bit-equal
        assert np.array_equal(a["scores"].view(np.int32), b["scores"].view(np.int32))    # training scores: bit-identical


SHAPES = {"depth3": (dict(TREE_PARAMS, num_leaves=8, max_depth=3), 40, 5, 130, 5, "sum"),
          "depth6": (dict(TREE_PARAMS, num_leaves=64, max_depth=6, max_bin=255, min_data_in_leaf=3), 45, 5, 130, 2, "sum"),
          "signed": (dict(TREE_PARAMS, num_leaves=16, max_depth=4), 40, 5, 130, 2, "reference")}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_depthwise_equals_leafwise_on_the_device_where_the_cap_cannot_bind(shape, tmp_path):
    import ptranking_amd as pa
    params, queries, lo, hi, rounds, hessian = SHAPES[shape]
    assert params["num_leaves"] >= 2 ** params["max_depth"]
    lw, lw_booster, X = drive("leafwise", 0, queries, lo, hi, rounds, params, hessian)
    dw, booster, _ = drive("depthwise", 0, queries, lo, hi, rounds, params, hessian)
    assert_policies_agree(lw, dw, X)
    p = booster.params
    for a, b in zip(lw, dw):
        _, _, depth = node_shape(b["tree"], X)
        splits = a["tree"]["feature"].size
        print(f"{shape}: {splits} splits, depth {depth}: host reads leaf-wise {a['reads']}, depth-wise {b['reads']}")
        assert b["reads"] <= depth + 2                                                   # one read per level (and the root's)
        assert a["reads"] == leafwise_reads(a["tree"], X, p) <= splits + 1               # one read per searched split (and the root's)
        assert splits < 7 or b["reads"] < a["reads"]
    if shape == "depth6":
        assert 2000 <= X.shape[0] <= 4200 and max(r["tree"]["feature"].size for r in dw) > 31
    # against the restatement too, under the device's own gradients: node numbering and leaf indices as the policy defines them
    edges, nbins = R.bin_edges(X, p["max_bin"])
    bins = R.bin_matrix(X, edges, nbins)
    scores = np.zeros(X.shape[0], np.float32)
    for r in dw:
        qg, qh, expo, _ = R.quantize(r["g"], r["h"])
        want, leaf_rows, margin, _ = LR.grow_tree(bins, qg, qh, expo, edges, nbins, p["max_bin"], p["num_leaves"], p["learning_rate"], p["lambda_l2"],
                                                  p["min_data_in_leaf"], p["min_sum_hessian_in_leaf"], p["min_gain_to_split"], p["max_depth"])
        assert margin > 1e-9                                                             # the screen, decided by the restatement alone
        for k in ("feature", "left", "right"):
            assert np.array_equal(r["tree"][k], want[k]), k
        assert np.array_equal(r["tree"]["threshold"].view(np.int32), want["threshold"].view(np.int32))
        assert np.array_equal(r["tree"]["value"].view(np.int32), want["value"].view(np.int32))
        scores = R.add_leaf_values(scores, leaf_rows, want["value"])
        assert np.array_equal(r["scores"].view(np.int32), scores.view(np.int32))
    if shape == "signed":
        # the rank-signed Hessians of a query sum to zero, so one child of every candidate has a Hessian sum <= 0 and the floor of the split
        # scan refuses it: both policies keep the single leaf (LambdaMART's docstring says so), from the root's one read
        assert all(r["tree"]["feature"].size == 0 and r["reads"] == 1 for r in lw + dw)
        return
    # predict = the training scores = a reloaded model, bit for bit
    assert torch.equal(booster.predict(X), booster.scores)
    path = tmp_path / "model.npz"
    booster.save_model(path)
    loaded = pa.GBDT.load_model(path)
    assert loaded.params["grow_policy"] == "depthwise" and torch.equal(loaded.predict(X), booster.scores)


@pytest.mark.parametrize("num_leaves,max_depth", [(20, -1), (11, 5), (400, -1)])
def test_depthwise_follows_the_restatement_where_the_cap_binds(num_leaves, max_depth):
    params = dict(TREE_PARAMS, num_leaves=num_leaves, max_depth=max_depth, min_data_in_leaf=3, max_bin=255)
    dw, booster, X = drive("depthwise", 1, 45, 5, 130, 2, params)
    p = booster.params
    edges, nbins = R.bin_edges(X, p["max_bin"])
    bins = R.bin_matrix(X, edges, nbins)
    scores = np.zeros(X.shape[0], np.float32)
    for r in dw:
        qg, qh, expo, _ = R.quantize(r["g"], r["h"])
        want, leaf_rows, margin, levels = LR.grow_tree(bins, qg, qh, expo, edges, nbins, p["max_bin"], num_leaves, p["learning_rate"], p["lambda_l2"],
                                                       p["min_data_in_leaf"], p["min_sum_hessian_in_leaf"], p["min_gain_to_split"], max_depth)
        assert margin > 1e-9
        for k in ("feature", "left", "right"):
            assert np.array_equal(r["tree"][k], want[k]), k
        assert np.array_equal(r["tree"]["threshold"].view(np.int32), want["threshold"].view(np.int32))
        assert np.array_equal(r["tree"]["value"].view(np.int32), want["value"].view(np.int32))
        scores = R.add_leaf_values(scores, leaf_rows, want["value"])
        assert np.array_equal(r["scores"].view(np.int32), scores.view(np.int32))
        if num_leaves < 400:                                                             # (400 leaves: a deep tree of many small segments,
            assert r["tree"]["value"].size == num_leaves                                 # which the data need not fill) a full tree,
            assert len(levels[-1]["candidates"]) > len(levels[-1]["kept"])               # and the cap did bind at the last level
        else:
            assert r["tree"]["value"].size > 200 and len(levels) >= 8
        assert r["reads"] <= len(levels) + 1
    assert torch.equal(booster.predict(X), booster.scores)


# ---------------------------------------------------------------- whole fits against scikit-learn (tests/golden/gbdt_sklearn_depth.npz)
@pytest.fixture(scope="module")
def depth_fits(tmp_path_factory):
    """Every case of the depth fixture fitted once with grow_policy='depthwise', driven round by round as gbdt_sk's leaf-wise cases are."""
    import ptranking_amd as pa
    from ptranking_amd import functional as Fn
    cases, out = LR.load()[0], {}
    real = Fn.gbdt_histogram_segments
    for name, c in cases.items():
        counts = []

        def spy(bins, qg, qh, rows, segs, nf, max_bin, pool):
            counts.append(np.asarray(segs)[:, 1].tolist())
            return real(bins, qg, qh, rows, segs, nf, max_bin, pool)

        p = c["params"]
        booster = pa.GBDT(dict(SK.booster_params(p), grow_policy="depthwise"), c["X"])
        base = np.float32(c["baseline"])
        booster.scores.fill_(float(base))
        y, w = dev(c["y"]), dev(np.ones_like(c["y"]) if c["w"] is None else c["w"])
        rounds = []
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(Fn, "gbdt_histogram_segments", spy)
            for _ in range(p["rounds"]):
                tree = booster.update((booster.scores - y) * w, w)
                rounds.append((tree, booster.scores.cpu().numpy().copy()))
        fresh = booster.predict(c["fresh"])
        path = tmp_path_factory.mktemp("skd") / f"{name}.npz"
        booster.save_model(path)
        reloaded = pa.GBDT.load_model(path).predict(c["fresh"])
        out[name] = dict(case=c, booster=booster, rounds=rounds, fresh=(fresh + float(base)).cpu().numpy(), same_bits=torch.equal(fresh, reloaded),
                         counts=counts)
    return out


@pytest.mark.parametrize("name", ("g", "h", "i", "j"))
def test_depthwise_fits_match_sklearn_and_the_restatement(depth_fits, name):
    """HistGradientBoostingRegressor(max_leaf_nodes=None, max_depth=d): trees equal in canonical form, staged and fresh predictions within
    gbdt_sk's gate C_GBDT_SK 2^-24 max(1, max |score|), taken over unchanged; and everything bit-identical to the restatement."""
    fit = depth_fits[name]
    c, p = fit["case"], fit["case"]["params"]
    assert len(fit["rounds"]) == p["rounds"]
    for r, (tree, scores) in enumerate(fit["rounds"]):
        nodes, leaves = SK.canonical(tree, c["X"])
        miss = SK.tree_mismatch(nodes, leaves, c, r)
        assert miss is None, f"round {r}: {miss}"
        err = float(np.abs(scores.astype(np.float64) - c["staged"][r]).max())
        print(f"MEASURED depth-wise gbdt vs sklearn, case {name} round {r}: training scores need C >= {err / SK.need_unit(c['staged'][r]):.2f}")
        assert err <= SK.gate(c["staged"][r]), r
    err = float(np.abs(fit["fresh"].astype(np.float64) - c["fresh_pred"]).max())
    print(f"MEASURED depth-wise gbdt vs sklearn, case {name}: fresh rows need C >= {err / SK.need_unit(c['fresh_pred']):.2f}")
    assert err <= SK.gate(c["fresh_pred"]) and fit["same_bits"]
    want, fresh, _ = LR.run_restatement(c, "depthwise")
    for (tree, scores), (ref_tree, ref_scores) in zip(fit["rounds"], want):
        for k in ("feature", "left", "right"):
            assert np.array_equal(tree[k], ref_tree[k]), k
        assert np.array_equal(tree["threshold"].view(np.int32), ref_tree["threshold"].view(np.int32))
        assert np.array_equal(tree["value"].view(np.int32), ref_tree["value"].view(np.int32))
        assert np.array_equal(scores.view(np.int32), ref_scores.view(np.int32))
    assert np.array_equal(fit["fresh"].view(np.int32), fresh.view(np.int32))
    assert fit["booster"].host_reads <= p["rounds"] * (p["max_depth"] + 2)


def test_depth_cases_reach_both_forms_in_one_level(depth_fits):
    """From the batched histogram calls the fits really made."""
    mixed = [cnt for cnt in depth_fits["h"]["counts"] if min(cnt) <= 256 < max(cnt)]
    assert mixed                                                                         # case h: direct-form and LDS-form segments in one call
    tiles = {name: launch_form("ptr_gbdt_histogram_segments", 300, fit["case"]["X"].shape[1], fit["case"]["params"]["max_bin"], 0)[2] for name, fit in depth_fits.items()}
    assert tiles == {"g": 1, "h": 2, "i": 3, "j": 1}
    assert all(max(cnt) <= 256 for cnt in depth_fits["j"]["counts"]) and depth_fits["j"]["case"]["X"].shape[0] == 257


# ---------------------------------------------------------------- LambdaMART
@pytest.fixture(scope="module")
def fit_sets():
    return ranking_set(31, 200, 10, 60), ranking_set(32, 60, 10, 60)


def test_lambdamart_learns_to_rank_depthwise(fit_sets):
    import ptranking_amd as pa
    (X, y, group), (Xv, yv, gv) = fit_sets
    lm = pa.LambdaMART(dict(FIT_PARAMS, grow_policy="depthwise")).fit(X, y, group, eval_set=(Xv, yv), eval_group=gv, eval_at=5)
    assert len(lm.booster.trees) == 30 and lm.booster.params["grow_policy"] == "depthwise"
    yv_d, y_d = dev(yv), dev(y)
    valid = lambda s: pa.LambdaMART.ndcg_at(s, yv_d, gv, 5)
    train = lambda s: pa.LambdaMART.ndcg_at(s, y_d, group, 5)
    after, constant = valid(lm.predict(Xv)), valid(torch.zeros(Xv.shape[0], device="cuda"))
    first, last = train(lm.predict(X, num_iteration=1)), train(lm.booster.scores)
    print(f"depthwise lambdarank: valid nDCG@5 constant {constant:.4f}, 30 trees {after:.4f}; train round 1 {first:.4f}, round 30 {last:.4f}")
    assert after > constant and after == lm.evals_result[-1] and last > first
    assert torch.equal(lm.predict(X), lm.booster.scores)
    assert lm.booster.host_reads <= 30 * 6                                               # 16 leaves: four levels


def test_early_stopping_and_two_identical_fits_depthwise(fit_sets):
    import ptranking_amd as pa
    (X, y, group), (Xv, yv, gv) = fit_sets
    params = dict(FIT_PARAMS, num_trees=200, learning_rate=0.5, num_leaves=31, min_data_in_leaf=3, grow_policy="depthwise")
    lm = pa.LambdaMART(params).fit(X[:1500], y[:1500], _groups_upto(group, 1500), eval_set=(Xv, yv), eval_group=gv, early_stopping_rounds=3)
    ran = len(lm.evals_result)
    assert ran < 200 and lm.best_iteration == int(np.argmax(lm.evals_result)) + 1 == ran - 3
    assert torch.equal(lm.predict(Xv), lm.predict(Xv, num_iteration=lm.best_iteration))
    few = dict(FIT_PARAMS, num_trees=5, grow_policy="depthwise")
    a = pa.LambdaMART(few).fit(X, y, group).booster
    b = pa.LambdaMART(few).fit(X, y, group).booster
    fa, fb = a.flat(), b.flat()
    for k in fa:
        assert fa[k].tobytes() == fb[k].tobytes(), k
    assert torch.equal(a.scores, b.scores)


def test_the_example_runs_depthwise():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_lambdamart_native.py"), "--queries", "120", "--rounds", "20",
                          "--grow-policy", "depthwise"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("round ")]
    assert len(lines) == 2 and "nDCG@5" in lines[0], out.stdout
    assert float(lines[-1].split("valid nDCG@5 ")[1].split()[0]) > float(out.stdout.split("constant scores: valid nDCG@5 ")[1].split()[0])
