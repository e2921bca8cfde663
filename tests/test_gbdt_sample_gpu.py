"""GPU: row sampling of the native booster against the numpy restatement tests/gbdt_sample_ref.py, bit for bit: the bag mask by row and by
query, GOSS (the exact select, the mask, the weighted gradients), the stable partition under a mask, the walk of one tree over binned rows,
and whole fits under bagging, query bagging and GOSS with both growth policies.  The training scores stay predict(X) for every row."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gbdt_ref as R
import gbdt_sample_ref as S
from launch_form import launch_form

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


def ragged(n):
    """Documents per query that sum to n: ragged, with an empty and a one-document query wherever n allows them."""
    sizes, out, k = (1, 0, 7, 64, 3, 130, 2, 0, 29), [], 0
    while sum(out) < n:
        out.append(min(sizes[k % len(sizes)], n - sum(out)))
        k += 1
    return np.array(out + [0], np.int64)


# ---------------------------------------------------------------- ptr_gbdt_bag_mask
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025, 5000])
def test_bag_mask_equals_the_restatement(n):
    from ptranking_amd import functional as F
    group = ragged(n)
    qid = S.group_qid(group)
    assert qid.size == n and (n < 10 or ((group == 0).any() and (group == 1).any()))
    for fraction in (2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0):
        for seed, draw in ((3, 0), (3, 1), (2 ** 40 + 17, 2 ** 33 + 5)):
            got = F.gbdt_bag_mask(n, seed, draw, fraction, device="cuda").cpu().numpy()
            assert got.dtype == np.uint8 and np.array_equal(got, S.bag_mask(n, seed, draw, fraction)), (fraction, seed, draw)
            got_q = F.gbdt_bag_mask(n, seed, draw, fraction, qid=dev(qid)).cpu().numpy()
            assert np.array_equal(got_q, S.bag_mask(n, seed, draw, fraction, qid)), (fraction, seed, draw)
            if fraction == 1.0:
                assert got.all() and got_q.all()
    if n >= 257:
        a, b = (F.gbdt_bag_mask(n, 3, d, 0.5, device="cuda") for d in (0, 1))
        assert not torch.equal(a, b) and 0 < int(a.sum()) < n                            # two draws differ
        q = F.gbdt_bag_mask(n, 3, 0, 0.5, qid=dev(qid)).cpu().numpy()
        assert all(len(set(q[qid == k].tolist())) <= 1 for k in range(group.size))       # a query is in or out as a whole


# ---------------------------------------------------------------- ptr_gbdt_goss
def goss_family(name, n, rng):
    if name == "gauss":
        return rng.standard_normal(n).astype(np.float32), rng.random(n).astype(np.float32)
    if name == "ties":
        return np.full(n, -0.5, np.float32), np.ones(n, np.float32)
    if name == "zero":
        return np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    e1, e2 = rng.integers(-70, 51, n), rng.integers(-70, 51, n)                          # products 2^-140 .. 2^100: denormals among them
    return (np.ldexp(1.0, e1) * np.where(rng.random(n) < 0.5, -1, 1)).astype(np.float32), np.ldexp(1.0, e2).astype(np.float32)


def check_goss(g, h, top, other, seed, draw, aliased):
    from ptranking_amd import functional as F
    n = g.size
    gd, hd = dev(g), dev(h)
    g2, h2, mask, info = F.gbdt_goss(gd, hd, top, other, seed, draw, out=(gd, hd) if aliased else None)
    assert (g2.data_ptr() == gd.data_ptr()) == aliased
    wg, wh, wmask, winfo = S.goss(g, h, top, other, seed, draw)
    assert tuple(info.cpu().tolist()) == tuple(int(np.int32(np.uint32(v))) for v in winfo), (info.cpu().tolist(), winfo)
    assert np.array_equal(mask.cpu().numpy(), wmask)
    for got, want in ((g2, wg), (h2, wh)):
        nan = np.isnan(want)
        assert np.array_equal(bits(got)[~nan], bits(want)[~nan]) and np.isnan(got.cpu().numpy()[nan]).all()
    return wmask, winfo


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097, 70001])
def test_goss_equals_the_restatement(n):
    from ptranking_amd import functional as F
    rng = np.random.default_rng(n)
    for family in ("gauss", "ties", "zero", "exponents"):
        g, h = goss_family(family, n, rng)
        for top, other in ((0.2, 0.1), (0.5, 0.5), (1.0 / n, 0.9)):
            if top + other > 1.0:                                                        # 1 / n with n <= 2: outside the rates' range
                with pytest.raises(ValueError, match="sum to at most 1"):
                    F.gbdt_goss(dev(g), dev(h), top, other, 3, 0)
                continue
            for aliased in (False, True):
                wmask, (tau, ntop, nkeep) = check_goss(g, h, top, other, 3, n % 7, aliased)
            if family == "ties":
                assert ntop == n == nkeep                                                # ties at tau are all in
            if family == "gauss" and n >= 255:
                assert ntop == max(1, int(np.floor(n * top))) and (other == 0.5 or 0 < nkeep < n)
    if n == 70001:
        assert launch_form("ptr_gbdt_goss", n)[2] == 18                                  # several workgroups of the counting passes
    else:
        assert launch_form("ptr_gbdt_goss", n)[2] == (1 if n <= 4096 else 2)


def test_goss_with_a_nan_gradient():
    import ptranking_amd as pa
    rng = np.random.default_rng(5)
    n = 4097
    g, h = goss_family("gauss", n, rng)
    g[5], h[4000] = np.nan, np.nan
    for aliased in (False, True):
        wmask, (tau, ntop, nkeep) = check_goss(g, h, 0.2, 0.1, 3, 2, aliased)            # the mask is still the restatement's
    keys = np.abs(g * h)
    assert ntop == 819 and tau == np.sort(keys[~np.isnan(keys)])[::-1][818].view(np.uint32)
    # in the trainer: past the warm-up (one tree at learning_rate 1.0) the NaN raises, and the next round works
    X = rng.standard_normal((n, 4)).astype(np.float32)
    booster = pa.GBDT({"num_leaves": 4, "min_data_in_leaf": 2, "learning_rate": 1.0, "data_sample_strategy": "goss", "max_bin": 31}, X)
    good = dev(np.nan_to_num(g))
    booster.update(good, torch.ones_like(good))
    with pytest.raises(FloatingPointError):
        booster.update(dev(g), torch.ones_like(good))
    assert len(booster.trees) == 1
    booster.update(good, torch.ones_like(good))
    assert len(booster.trees) == 2 and torch.equal(booster.predict(X), booster.scores)


# ---------------------------------------------------------------- ptr_gbdt_partition_mask
# 256 * 1024 + 1025 entries are 258 workgroups: a thread of the scan over their counts owns two of them, and the last threads own none.
# That list is longer than the mask: it repeats rows, and the identity list runs past the mask's end.
@pytest.mark.parametrize("m", [0, 1, 255, 256, 257, 1024, 1025, 3 * 1024 + 17, 256 * 1024 + 1025])
def test_partition_mask_is_stable_and_exact(m):
    from ptranking_amd import functional as F
    rng = np.random.default_rng(m)
    n = 4000
    lists = {"identity": None, "subset": rng.permutation(n)[:m].astype(np.int32),
             "out of range": (rng.permutation(n + 600)[:m] - 300).astype(np.int32)}
    if m > n:
        lists.update({"subset": rng.integers(0, n, m).astype(np.int32), "out of range": rng.integers(-300, n + 300, m).astype(np.int32)})
    for kind, mask in (("zeros", np.zeros(n, np.uint8)), ("ones", np.ones(n, np.uint8)), ("random", (rng.random(n) < 0.4).astype(np.uint8) * 3)):
        for name, rows in lists.items():
            out, lc = F.gbdt_partition_mask(dev(mask), None if rows is None else dev(rows), m=m if rows is None else None)
            want, kept = S.partition_mask(mask, rows, m)
            assert out.numel() == m and int(lc) == kept and np.array_equal(out.cpu().numpy(), want), (kind, name)
            if name == "subset" or (name == "identity" and m <= n):                      # a list inside the mask
                assert kept == {"zeros": 0, "ones": m}.get(kind, kept)
    if m > 600:
        r = lists["out of range"]
        assert (r < 0).any() and (r >= n).any()


# ---------------------------------------------------------------- ptr_gbdt_add_tree_binned
@pytest.fixture(scope="module")
def fit_data():
    """Squared error on 3000 rows of 5 features, max_bin 31: the whole fits' data, its bins on the host and on the device."""
    rng = np.random.default_rng(7)
    n, nf, max_bin = 3000, 5, 31
    X = rng.standard_normal((n, nf)).astype(np.float32)
    X[:, 2] = np.round(X[:, 2] * 3)                                                      # a feature of few distinct values
    y = (X[:, 0] + (X[:, 1] > 0.3) * 1.5 - 0.4 * X[:, 2] + X[:, 3] * X[:, 4] + 0.2 * rng.standard_normal(n)).astype(np.float32)
    edges, nbins = R.bin_edges(X, max_bin)
    group = ragged(n)
    return dict(X=X, y=y, edges=edges, nbins=nbins, bins=R.bin_matrix(X, edges, nbins), group=group, qid=S.group_qid(group), max_bin=max_bin)


def test_add_tree_binned_equals_the_walk_and_predict(fit_data):
    from ptranking_amd import functional as F
    d = fit_data
    X, bins, n = d["X"], d["bins"], d["X"].shape[0]
    params = {"max_bin": d["max_bin"], "num_leaves": 8, "min_data_in_leaf": 10, "learning_rate": 0.5}
    tree, _, add, _ = S.grow(bins, -d["y"], np.ones(n, np.float32), d["edges"], d["nbins"], params, 0)
    sb = S.split_bins(tree, d["edges"], d["nbins"])
    assert tree["feature"].size == 7
    dbins = F.gbdt_bin(dev(X), dev(d["edges"]), dev(d["nbins"]))
    assert np.array_equal(dbins.cpu().numpy()[:, :5], bins)
    t = [dev(tree[k]) for k in ("feature",)] + [dev(sb)] + [dev(tree[k]) for k in ("left", "right", "value")]
    start = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    got = F.gbdt_add_tree_binned(dev(start), dbins, 5, None, *t)
    assert np.array_equal(bits(got), bits(start + add))                                  # the restatement's walk
    offs = dev(np.array([0, 7], np.int32))
    pred = F.gbdt_predict(dev(X), dev(tree["feature"]), dev(tree["threshold"]), dev(tree["left"]), dev(tree["right"]), dev(tree["value"]), offs)
    assert np.array_equal(bits(F.gbdt_add_tree_binned(torch.zeros(n, device="cuda"), dbins, 5, None, *t)), bits(pred))      # predict on the raw X
    rows = np.random.default_rng(2).permutation(n)[:1111].astype(np.int32)               # a row list: only its rows, once each
    want = start.copy()
    want[rows] = want[rows] + add[rows]
    assert np.array_equal(bits(F.gbdt_add_tree_binned(dev(start), dbins, 5, dev(rows), *t)), bits(want))
    assert np.array_equal(bits(F.gbdt_add_tree_binned(dev(start), dbins, 5, dev(rows[:0]), *t)), bits(start))               # m = 0
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    leaf = F.gbdt_add_tree_binned(dev(start), dbins, 5, None, none, none, none, none, dev(np.array([0.25], np.float32)))
    assert np.array_equal(bits(leaf), bits(start + np.float32(0.25)))                    # a single leaf
    bad_left = tree["left"].copy()
    bad_left[0] = 99                                                                     # a child index out of range: NaN for the rows that go there
    bad = F.gbdt_add_tree_binned(torch.zeros(n, device="cuda"), dbins, 5, None, t[0], t[1], dev(bad_left), t[3], t[4]).cpu().numpy()
    went = bins[:, tree["feature"][0]] <= sb[0]
    assert went.any() and np.isnan(bad[went]).all() and np.array_equal(bits(bad[~went]), bits(add[~went]))
    loop = F.gbdt_add_tree_binned(torch.zeros(n, device="cuda"), dbins, 5, None, t[0], t[1], dev(np.zeros(7, np.int32)), dev(np.zeros(7, np.int32)), t[4])
    assert torch.isnan(loop).all()                                                       # a cycle ends after nnodes steps


# ---------------------------------------------------------------- whole fits
BASE = {"max_bin": 31, "num_leaves": 8, "min_data_in_leaf": 10, "learning_rate": 0.1}
CASES = {"bag": {"bagging_fraction": 0.5, "bagging_freq": 1},
         "bag2": {"bagging_fraction": 0.5, "bagging_freq": 2},
         "query": {"bagging_fraction": 0.5, "bagging_freq": 1, "bagging_by_query": True},
         "goss": {"data_sample_strategy": "goss", "learning_rate": 0.5}}
ROUNDS = 6
SAMPLER_CALLS = ("gbdt_bag_mask", "gbdt_goss", "gbdt_partition_mask", "gbdt_add_tree_binned")


def run_fit(d, params, restate=True, rounds=ROUNDS):
    """GBDT.update under squared error for `rounds` rounds, and the restatement under the SAME device gradients every round.
    -> dict(booster, trees, masks (the device's, None for an unsampled tree), want = the restatement's (tree, mask, scores) per round,
    worst = its smallest split margin, calls = per round the sampler's wrappers update() went through)."""
    import ptranking_amd as pa
    from ptranking_amd import functional as F, gbdt as G
    X, y, n = d["X"], d["y"], d["X"].shape[0]
    calls, real = [], {k: getattr(F, k) for k in SAMPLER_CALLS}

    def spy(name):
        def wrapped(*a, **kw):
            calls.append((name, a[3].numel() if name == "gbdt_add_tree_binned" else None))      # the walk: how many rows it was handed
            return real[name](*a, **kw)
        return wrapped
    for k in SAMPLER_CALLS:
        setattr(F, k, spy(k))
    try:
        return _run_fit(pa, G, d, params, restate, rounds, calls)
    finally:
        for k in SAMPLER_CALLS:
            setattr(F, k, real[k])


def _run_fit(pa, G, d, params, restate, rounds, calls):
    X, y, n = d["X"], d["y"], d["X"].shape[0]
    booster = pa.GBDT(params).fit_bins(X, group=d["group"])
    p = booster.params
    assert np.array_equal(booster.bins.cpu().numpy()[:, :X.shape[1]], d["bins"])
    yd, ones = dev(y), torch.ones(n, device="cuda")
    ref_scores = np.zeros(n, np.float32)
    out = dict(booster=booster, trees=[], masks=[], want=[], worst=np.inf, calls=[])
    for t in range(rounds):
        g = booster.scores - yd
        gh = g.cpu().numpy()
        del calls[:]
        out["trees"].append(booster.update(g, ones))
        out["calls"].append(list(calls))
        active = G.sampling(p) and not (G.sampling(p) == "goss" and t < int(np.floor(1.0 / p["learning_rate"])))
        out["masks"].append(booster._mask.cpu().numpy().copy() if active else None)
        if restate:
            tree, mask, add, margin = S.grow(d["bins"], gh, np.ones(n, np.float32), d["edges"], d["nbins"], p, t, d["qid"])
            ref_scores = ref_scores + add
            out["want"].append((tree, mask, ref_scores.copy(), booster.scores.cpu().numpy().copy()))
            out["worst"] = min(out["worst"], margin)
    return out


@pytest.fixture(scope="module")
def fits(fit_data):
    return {(name, policy): run_fit(fit_data, dict(BASE, grow_policy=policy, **extra)) for name, extra in CASES.items() for policy in ("leafwise", "depthwise")}


@pytest.mark.parametrize("policy", ["leafwise", "depthwise"])
@pytest.mark.parametrize("name", list(CASES))
def test_sampled_fits_equal_the_restatement(fits, fit_data, name, policy):
    run = fits[(name, policy)]
    booster, n = run["booster"], fit_data["X"].shape[0]
    assert run["worst"] > 1e-9                                                           # the screen: no split of the restatement is a near tie
    sampled = 0
    for t, (got, (want, mask, ref_scores, dev_scores)) in enumerate(zip(run["trees"], run["want"])):
        for k in ("feature", "left", "right"):
            assert np.array_equal(got[k], want[k]), (t, k)                               # node for node
        assert np.array_equal(bits(got["threshold"]), bits(want["threshold"])) and np.array_equal(bits(got["value"]), bits(want["value"])), t
        assert np.array_equal(bits(dev_scores), bits(ref_scores)), t                     # every row, in the bag or not
        assert (mask is None) == (run["masks"][t] is None)
        names = [c[0] for c in run["calls"][t]]
        if mask is not None:
            assert np.array_equal(run["masks"][t], mask) and 0 < mask.sum() < n, t       # some rows are outside the bag: the walk ran
            assert run["calls"][t][-1] == ("gbdt_add_tree_binned", n - int(mask.sum())), t          # once, over exactly the rows outside the bag
            first = "gbdt_goss" if name == "goss" else "gbdt_bag_mask"
            drawn = name != "bag2" or t % 2 == 0                                          # bagging_freq 2: the odd trees reuse the mask
            assert names == ([first] if drawn else []) + ["gbdt_partition_mask", "gbdt_add_tree_binned"], (t, names)
            sampled += 1
        else:
            assert names == [], (t, names)                                                # GOSS's warm-up: exactly the unsampled calls
        assert got["feature"].size == 7
    assert sampled == (ROUNDS - 2 if name == "goss" else ROUNDS)
    assert torch.equal(booster.predict(fit_data["X"]), booster.scores)                   # scores stay predict(X), bit for bit
    m = run["masks"]
    if name == "bag2":
        assert np.array_equal(m[0], m[1]) and not np.array_equal(m[1], m[2]) and np.array_equal(m[2], m[3])
    if name == "bag":
        assert not np.array_equal(m[0], m[1])
    if name == "query":
        qid = fit_data["qid"]
        assert all(len(set(m[0][qid == k].tolist())) <= 1 for k in range(fit_data["group"].size))
    assert booster.host_reads > 0


@pytest.mark.parametrize("policy", ["leafwise", "depthwise"])
def test_goss_warm_up_trees_are_the_unsampled_fit(fits, fit_data, policy):
    plain = run_fit(fit_data, dict(BASE, grow_policy=policy, learning_rate=0.5), restate=False, rounds=3)
    goss = fits[("goss", policy)]
    same = lambda a, b: all(a[k].tobytes() == b[k].tobytes() for k in ("feature", "threshold", "left", "right", "value"))
    assert same(plain["trees"][0], goss["trees"][0]) and same(plain["trees"][1], goss["trees"][1])
    assert not same(plain["trees"][2], goss["trees"][2])
    assert goss["masks"][0] is None and goss["masks"][1] is None and goss["masks"][2] is not None


def test_two_fits_give_the_same_bits_and_another_seed_another_model(fits, fit_data):
    for name in ("bag", "goss"):
        params = dict(BASE, grow_policy="leafwise", **CASES[name])
        again = run_fit(fit_data, params, restate=False)
        fa, fb = fits[(name, "leafwise")]["booster"], again["booster"]
        for k, v in fa.flat().items():
            assert v.tobytes() == fb.flat()[k].tobytes(), (name, k)
        assert torch.equal(fa.scores, fb.scores) and fa.host_reads == fb.host_reads
        other = run_fit(fit_data, dict(params, bagging_seed=4), restate=False)["booster"]
        assert any(v.tobytes() != other.flat()[k].tobytes() for k, v in fa.flat().items()), name


def test_query_bagging_needs_the_groups(fit_data):
    import ptranking_amd as pa
    params = dict(BASE, **CASES["query"])
    with pytest.raises(ValueError, match="needs the queries"):
        pa.GBDT(params, fit_data["X"])
    with pytest.raises(ValueError, match="needs the queries"):
        pa.GBDT(params).fit_bins(fit_data["X"])
    with pytest.raises(ValueError, match="sum to"):
        pa.GBDT(params).fit_bins(fit_data["X"], group=[5, 5])


def test_inactive_sampling_is_the_fit_without_the_keys(fit_data, tmp_path):
    """Explicit defaults, and bagging_freq 5 with bagging_fraction 1.0: the trees, the scores and host_reads of a fit without the keys, and
    for the explicit defaults the saved model entry for entry."""
    from test_gbdt_sample_cpu import NEW_DEFAULTS
    for policy in ("leafwise", "depthwise"):
        base = dict(BASE, grow_policy=policy)
        plain = run_fit(fit_data, base, restate=False, rounds=3)["booster"]
        for extra in (NEW_DEFAULTS, {"bagging_freq": 5, "bagging_fraction": 1.0}):
            run = run_fit(fit_data, dict(base, **extra), restate=False, rounds=3)
            other = run["booster"]
            assert not hasattr(other, "_mask") and run["calls"] == [[], [], []]          # no sampler state, no sampler call
            for k, v in plain.flat().items():
                assert v.tobytes() == other.flat()[k].tobytes(), (policy, k)
            assert torch.equal(plain.scores, other.scores) and plain.host_reads == other.host_reads
            if extra is NEW_DEFAULTS:
                plain.save_model(tmp_path / "a.npz")
                other.save_model(tmp_path / "b.npz")
                with np.load(tmp_path / "a.npz") as a, np.load(tmp_path / "b.npz") as b:
                    assert sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() for k in a.files)


# ---------------------------------------------------------------- LambdaMART
@pytest.mark.parametrize("name", ["query", "goss"])
def test_lambdamart_learns_to_rank_under_sampling(name, tmp_path):
    import ptranking_amd as pa
    from test_gbdt_gpu import FIT_PARAMS, ranking_set
    (X, y, group), (Xv, yv, gv) = ranking_set(31, 200, 10, 60), ranking_set(32, 60, 10, 60)
    extra = {"query": {"bagging_fraction": 0.5, "bagging_freq": 1, "bagging_by_query": True}, "goss": {"data_sample_strategy": "goss"}}[name]
    lm = pa.LambdaMART(dict(FIT_PARAMS, **extra)).fit(X, y, group, eval_set=(Xv, yv), eval_group=gv, eval_at=5)
    assert len(lm.booster.trees) == 30 and len(lm.evals_result) == 30 and lm.best_iteration is None
    yv_d = dev(yv)
    valid = lambda s: pa.LambdaMART.ndcg_at(s, yv_d, gv, 5)
    after, one_tree, constant = valid(lm.predict(Xv)), valid(lm.predict(Xv, num_iteration=1)), valid(torch.zeros(Xv.shape[0], device="cuda"))
    print(f"{name}: valid nDCG@5 constant {constant:.4f}, one tree {one_tree:.4f}, 30 trees {after:.4f}")
    assert after > constant and after > one_tree
    assert after == lm.evals_result[-1]                                                  # the running validation scores are predict()'s bits
    y_d = dev(y)
    first, last = (pa.LambdaMART.ndcg_at(s, y_d, group, 5) for s in (lm.predict(X, num_iteration=1), lm.booster.scores))
    print(f"{name}: train nDCG@5 round 1 {first:.4f}, round 30 {last:.4f}")
    assert last >= first
    assert torch.equal(lm.predict(X), lm.booster.scores)                                 # out-of-bag rows included
    kept = int(lm.booster._mask.sum())
    assert 0 < kept < X.shape[0]
    path = tmp_path / "model.npz"
    lm.booster.save_model(path)
    back = pa.GBDT.load_model(path)
    assert back.params == lm.booster.params and torch.equal(back.predict(Xv), lm.predict(Xv)) and torch.equal(back.predict(X), lm.booster.scores)


@pytest.mark.parametrize("flags", [["--goss"], ["--by-query", "--bagging-fraction", "0.5", "--bagging-freq", "1"]])
def test_the_example_runs_with_sampling(flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_lambdamart_native.py"), "--queries", "120", "--rounds", "20"] + flags,
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("round ")]
    assert len(lines) == 2 and "nDCG@5" in lines[0], out.stdout
    assert "sampling: " in out.stdout and ("goss" if flags == ["--goss"] else "by query") in out.stdout
