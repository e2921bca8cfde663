"""GPU: missing feature values in the native booster (use_missing=True; the *_missing entry points of csrc/gbdt.hip) against the numpy
restatement tests/gbdt_missing_ref.py, bit for bit, and whole fits on data with NaNs against scikit-learn
(tests/golden/gbdt_sklearn_missing.npz) under the gate the restatement set (test_gbdt_missing_cpu.py)."""
import numpy as np
import pytest
import torch

import gbdt_missing_ref as MR
import gbdt_ref as R
import gbdt_sk as SK

pytestmark = pytest.mark.gpu
EXPO = (10, 10)
ONE = 1 << 10                                                            # a Hessian of 1.0 per row in fixed point


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


def device_records(hist, nbins, nan_bin, **kw):
    from ptranking_amd import functional as F
    hist = np.asarray(hist, np.int64)
    hist = hist[None] if hist.ndim == 3 else hist
    return F.gbdt_best_split(dev(hist), dev(nbins), dev(np.array(EXPO, np.int32)), kw.get("l2", 0.0), kw.get("min_data", 1), kw.get("min_hess", 1e-3),
                             kw.get("min_gain", 0.0), nan_bin=dev(nan_bin)).cpu().numpy()


def restated(hist, nbins, nan_bin, **kw):
    return MR.best_split(hist, nbins, nan_bin, EXPO, kw.get("l2", 0.0), kw.get("min_data", 1), kw.get("min_hess", 1e-3), kw.get("min_gain", 0.0))


# ---------------------------------------------------------------- the split scan on hand-made histograms
SCAN_SHAPES = [(4, 3), (16, 3), (16, 4), (16, 5), (255, 3), (255, 4), (255, 5), (255, 252), (256, 4), (256, 252), (256, 255)]
SCENARIOS = ("mc0", "nan_rest", "left", "tie")


def scan_case(max_bin, nan_bin, scenario, seed=0):
    """Histograms [3, max_bin, 3] summed from 800 synthetic rows, so that every feature holds the node's totals.  Feature 0 has no NaN bin,
    feature 1 has nan_bin value bins and its NaN bin right behind them (a lane boundary of the four-bins-per-lane scan at 3, 4, 5, 252 and
    255), feature 2 two value bins and a NaN bin.  The gradients follow feature 1 by scenario.  With 252 or 255 value bins most bins are empty
    in the node: equal gains over empty stretches are the rule."""
    rng = np.random.default_rng([max_bin, nan_bin, SCENARIOS.index(scenario), seed])
    n, nb1 = 800, nan_bin
    nbins = np.array([min(max_bin, 7), nb1, 2], np.int32)
    nanb = np.array([-1, nan_bin, 2], np.int32)
    b = np.stack([rng.integers(0, nbins[0], n), rng.integers(0, nb1, n), rng.integers(0, 2, n)], axis=1)
    miss1 = (rng.random(n) < 0.25) & (scenario != "mc0")
    b[miss1, 1] = nan_bin
    b[rng.random(n) < 0.2, 2] = 2
    low = b[:, 1] < (nb1 + 1) // 2
    qh = np.full(n, ONE, np.int64)
    if scenario == "nan_rest":
        qg = np.where(miss1, -40 * ONE, 3 * ONE) + rng.integers(-ONE // 8, ONE // 8, n)
    elif scenario == "tie":
        qg = np.where(low, -20 * ONE, 20 * ONE) + rng.integers(-ONE // 8, ONE // 8, n)
        qg[miss1], qh[miss1] = 0, 0                                      # missing rows that carry nothing: the two directions tie exactly
    else:
        qg = np.where(low | (miss1 & (scenario == "left")), -20 * ONE, 20 * ONE) + rng.integers(-ONE // 8, ONE // 8, n)
    hist = R.histogram(b.astype(np.uint8), qg.astype(np.int32), qh.astype(np.int32), None, max_bin)
    return hist, nbins, nanb, int(miss1.sum())


@pytest.mark.parametrize("max_bin,nan_bin", SCAN_SHAPES)
def test_split_scan_equals_the_restatement(max_bin, nan_bin):
    from ptranking_amd import functional as F
    pool, want = [], []
    for scenario in SCENARIOS:
        hist, nbins, nanb, mc = scan_case(max_bin, nan_bin, scenario)
        s = restated(hist, nbins, nanb, min_hess=0.0)
        assert s["feature"] == 1 and s["missing"] == mc, scenario
        if scenario == "mc0":                                            # no missing rows: the old scan's winner, and the majority child
            old = R.best_split(hist, nbins, EXPO, min_hess=0.0)
            assert mc == 0 and (s["gain"], s["bin"], s["left"]) == (old["gain"], old["bin"], old["left"])
            assert s["default_left"] == int(s["left"][2] > s["right"][2])
        if scenario == "nan_rest":                                       # every value left, the NaNs right
            assert mc > 0 and s["default_left"] == 0 and s["right"][2] == mc
        if scenario == "left":
            assert mc > 0 and s["default_left"] == 1 and s["bin"] < nan_bin - 1
        if scenario == "tie":                                            # an exact tie of the two directions keeps missing-right
            gain = MR.candidates(hist, nbins, nanb, EXPO, 0.0, 1, 0.0, 0.0)[0]
            assert mc > 0 and gain[1, s["bin"], 0] == gain[1, s["bin"], 1] == s["gain"] and s["default_left"] == 0
        got = device_records(hist, nbins, nanb, min_hess=0.0)
        assert np.array_equal(got[0], MR.record(s)), (scenario, got[0].tolist(), MR.record(s).tolist())
        pool.append(hist)
        want.append(got[0])
    # the slot-list form equals the contiguous form, out of order and with a slot outside the pool
    slots = [3, 0, 7, 2, 1, -1]
    got = F.gbdt_best_split_slots(dev(np.stack(pool)), slots, dev(nbins), dev(np.array(EXPO, np.int32)), 0.0, 1, 0.0, 0.0, nan_bin=dev(nanb)).cpu().numpy()
    none = MR.record(MR.best_split(np.zeros_like(pool[0]), nbins, nanb, EXPO))
    for k, slot in enumerate(slots):
        assert np.array_equal(got[k], want[slot] if 0 <= slot < 4 else none), slot
    # without a NaN bin anywhere the missing scan gives the old records but for field 2's direction
    hist, nbins, nanb, _ = scan_case(max_bin, nan_bin, "mc0")
    none_b = np.full(3, -1, np.int32)
    old = F.gbdt_best_split(dev(hist[None]), dev(nbins), dev(np.array(EXPO, np.int32)), 0.0, 1, 0.0, 0.0).cpu().numpy()[0]
    new = device_records(hist, nbins, none_b, min_hess=0.0)[0]
    assert new[2] % 256 == old[2] and new[2] // 256 == int(old[5] > old[8]) and np.array_equal(np.delete(new, 2), np.delete(old, 2))


@pytest.mark.parametrize("max_bin,nan_bin", [(16, 4), (256, 255)])
def test_split_scan_constraints_reject_each_side(max_bin, nan_bin):
    """min_data_in_leaf and the Hessian floor, each at the value that still admits the winner's smaller side and one above it."""
    seen = set()
    for scenario in ("nan_rest", "left"):
        hist, nbins, nanb, mc = scan_case(max_bin, nan_bin, scenario)
        free = restated(hist, nbins, nanb)
        small = min(free["left"][2], free["right"][2])                   # h = 1 per row: the Hessian sum of a side is its row count
        for kw in ({"min_data": small}, {"min_data": small + 1}, {"min_hess": float(small)}, {"min_hess": small + 0.5},
                   {"min_data": free["left"][2] + 1}, {"min_hess": free["left"][2] + 0.5}, {"min_data": 401}, {"min_gain": free["gain"] * 2}):
            s = restated(hist, nbins, nanb, **kw)
            got = device_records(hist, nbins, nanb, **kw)[0]
            assert np.array_equal(got, MR.record(s)), (scenario, kw, got.tolist(), MR.record(s).tolist())
            admits = (s["feature"], s["bin"], s["default_left"]) == (free["feature"], free["bin"], free["default_left"])
            assert admits == (list(kw.values())[0] in (small, float(small))), (scenario, kw)
            seen.add((scenario, s["feature"], s["bin"], s["default_left"]))
    assert len(seen) >= 5


# ---------------------------------------------------------------- binning
@pytest.mark.parametrize("nf", [1, 16, 17])
def test_binning_with_nan_bins(nf):
    from ptranking_amd import functional as F, gbdt
    rng = np.random.default_rng(nf)
    n = 300
    X = (rng.integers(0, 30, (n, nf)) / 4).astype(np.float32)
    X[:, 0] = rng.standard_normal(n).astype(np.float32)                  # more distinct values than bins
    clean = X.copy()
    for f in range(0, nf, 3):
        X[rng.random(n) < 0.25, f] = np.nan
    for mb in (8, 256):
        edges, nbins, nan_bin = gbdt.bin_edges(X, mb, use_missing=True)
        got = F.gbdt_bin(dev(X), dev(edges), dev(nbins), nan_bin=dev(nan_bin)).cpu().numpy()
        want = MR.bin_matrix(X, edges, nbins, nan_bin)
        assert got.shape == (n, (nf + 15) // 16 * 16) and np.array_equal(got[:, :nf], want) and not got[:, nf:].any()
        assert (got[:, :nf][np.isnan(X)] == np.broadcast_to(nan_bin, X.shape)[np.isnan(X)]).all() and (nan_bin[::3] == nbins[::3]).all()
        e0, n0 = gbdt.bin_edges(clean, mb)                               # no NaN: the bins of the entry point without nan_bin
        old = F.gbdt_bin(dev(clean), dev(e0), dev(n0))
        assert torch.equal(F.gbdt_bin(dev(clean), dev(e0), dev(n0), nan_bin=dev(np.full(nf, -1, np.int32))), old)


# ---------------------------------------------------------------- both partitions
# 256 * 1024 + 1025 entries are 258 workgroups: a thread of the scan over their counts owns two of them, and the last threads own none
@pytest.mark.parametrize("m", [1, 255, 256, 257, 1024, 1025, 4097, 256 * 1024 + 1025])
def test_partitions_with_a_bin_that_goes_left_as_well(m):
    from ptranking_amd import functional as F
    rng = np.random.default_rng(m)
    n = m + 700
    binsn = np.zeros((n, 16), np.uint8)
    binsn[:, :3] = rng.integers(0, 12, (n, 3))
    bins = dev(binsn)
    rows = rng.permutation(n).astype(np.int32)
    if m > 4097:
        rows[:m] = rng.integers(0, n, m)                                  # the long list repeats rows
    for also in (9, 11, 2, -1):
        out, lc = F.gbdt_partition(bins, dev(rows[:m]), 1, 3, 3, also_left=also)
        want, wl = MR.partition(binsn, rows[:m], 1, 3, also)
        assert np.array_equal(out.cpu().numpy(), want) and int(lc) == wl, also
    old, olc = F.gbdt_partition(bins, dev(rows[:m]), 1, 3, 3)
    assert torch.equal(out, old) and int(olc) == int(lc)                  # also_left = -1: the entry point without it
    # the segment form: K = 3, one also_left = -1, gaps between the segments
    segs = np.array([[0, m, 1, 3, 9], [m + 5, 257, 0, 6, -1], [m + 300, 391, 2, 0, 11]], np.int64)
    out, lcs = F.gbdt_partition_segments(bins, dev(rows), segs, 3, also_left=True)
    want = rows.copy()
    for k, (s, c, f, b, also) in enumerate(segs):
        want[s:s + c], wl = MR.partition(binsn, rows[s:s + c], f, b, also)
        assert int(lcs[k]) == wl, k
    assert np.array_equal(out.cpu().numpy(), want)
    old, olcs = F.gbdt_partition_segments(bins, dev(rows), np.concatenate([segs[:, :4]]), 3)
    out2, lcs2 = F.gbdt_partition_segments(bins, dev(rows), np.concatenate([segs[:, :4], np.full((3, 1), -1)], axis=1), 3, also_left=True)
    assert torch.equal(out2, old) and torch.equal(lcs2, olcs)
    bad = segs.copy()
    bad[0, 4] = 256                                                       # a table entry out of range: the segment is left as it was
    out3, lcs3 = F.gbdt_partition_segments(bins, dev(rows), bad, 3, also_left=True)
    assert np.array_equal(out3.cpu().numpy()[:m], rows[:m]) and int(lcs3[0]) == 0 and np.array_equal(out3.cpu().numpy()[m:], want[m:])
    with pytest.raises(RuntimeError, match="also_left"):
        F.gbdt_partition(bins, dev(rows[:m]), 1, 3, 3, also_left=256)


# ---------------------------------------------------------------- the binned walk and predict
def test_binned_walk_and_predict_on_a_tree_with_an_infinite_threshold():
    from ptranking_amd import functional as F, gbdt
    rng = np.random.default_rng(11)
    n = 1500
    X = (rng.integers(0, 9, (n, 3)) / 2).astype(np.float32)
    X[rng.random(n) < 0.3, 1] = np.nan
    X[rng.random(n) < 0.2, 2] = np.nan
    edges, nbins, nan_bin = gbdt.bin_edges(X, 16, use_missing=True)
    assert nan_bin.tolist() == [-1, 9, 9]
    # node 0: feature 2 at bin 3, NaNs left; node 1: feature 1, the NaNs against the rest (bin nbins - 1, threshold +inf); node 2: feature 0
    tree = {"feature": np.array([2, 1, 0], np.int32), "split_bin": np.array([3, 8, 4], np.int32), "left": np.array([1, ~0, ~2], np.int32),
            "right": np.array([2, ~1, ~3], np.int32), "value": np.array([-1.5, 0.25, 2.0, -0.75], np.float32), "default_left": np.array([1, 0, 1], np.uint8)}
    tree["threshold"] = edges[tree["feature"], tree["split_bin"]]
    assert np.isinf(tree["threshold"][1]) and np.isfinite(tree["threshold"][[0, 2]]).all()
    also = np.where(tree["default_left"] != 0, nan_bin[tree["feature"]], -1).astype(np.int32)
    assert also.tolist() == [9, -1, -1]
    binsn = MR.bin_matrix(X, edges, nbins, nan_bin)
    bins = F.gbdt_bin(dev(X), dev(edges), dev(nbins), nan_bin=dev(nan_bin))
    leaf = MR.walk_binned(binsn, tree, tree["split_bin"], also)
    want = MR.predict(X, [tree])
    assert np.array_equal(want, tree["value"][leaf]) and len(set(leaf.tolist())) == 4      # the binned walk is the raw walk; every leaf is reached
    rows = rng.permutation(n)[:1100].astype(np.int32)
    scores = torch.zeros(n, device="cuda")
    F.gbdt_add_tree_binned(scores, bins, 3, dev(rows), dev(tree["feature"]), dev(tree["split_bin"]), dev(tree["left"]), dev(tree["right"]),
                           dev(tree["value"]), also_left=dev(also))
    expect = np.zeros(n, np.float32)
    expect[rows] = want[rows]
    assert np.array_equal(bits(scores), bits(expect))
    offs = dev(np.array([0, 3, 6], np.int32))
    two = {k: dev(np.concatenate([tree[k], tree[k]])) for k in ("feature", "threshold", "left", "right", "value", "default_left")}
    got = F.gbdt_predict(dev(X), two["feature"], two["threshold"], two["left"], two["right"], two["value"], offs, default_left=two["default_left"])
    assert np.array_equal(bits(got), bits(MR.predict(X, [tree, tree])))
    # a malformed tree gives NaN and reads nothing out of range: a cycle, a child and a feature out of range
    for k, v in (("left", [0, ~0, ~2]), ("right", [2, 7, ~3]), ("feature", [2, 5, 0])):
        broken = {**{q: dev(tree[q]) for q in ("feature", "threshold", "left", "right", "value", "default_left")}, k: dev(np.array(v, np.int32))}
        out = F.gbdt_predict(dev(X), broken["feature"], broken["threshold"], broken["left"], broken["right"], broken["value"], dev(np.array([0, 3], np.int32)),
                             default_left=broken["default_left"]).cpu().numpy()
        assert np.isnan(out).any() and np.array_equal(out[~np.isnan(out)], want[~np.isnan(out)])


# ---------------------------------------------------------------- whole fits against scikit-learn
NAMES = ("p", "q", "r", "s", "t")


def fit_case(c, depthwise=False, extra=None, rounds=None, baseline=True):
    import ptranking_amd as pa
    p = c["params"]
    booster = pa.GBDT(dict(MR.booster_params(p, depthwise), **(extra or {})), c["X"])
    base = np.float32(c["baseline"] if baseline else 0.0)
    booster.scores.fill_(float(base))
    y, w = dev(c["y"]), dev(np.ones_like(c["y"]) if c["w"] is None else c["w"])
    out = []
    for _ in range(p["rounds"] if rounds is None else rounds):
        tree = booster.update((booster.scores - y) * w, w)
        out.append((tree, booster.scores.cpu().numpy().copy()))
    return booster, out


@pytest.fixture(scope="module")
def fits(tmp_path_factory):
    import ptranking_amd as pa
    cases, out = MR.load()[0], {}
    assert tuple(sorted(cases)) == NAMES
    for name, c in cases.items():
        for depthwise in ((False, True) if c["params"]["depthwise"] else (False,)):
            booster, rounds = fit_case(c, depthwise)
            fresh = booster.predict(c["fresh"])
            path = tmp_path_factory.mktemp("missing") / f"{name}.npz"
            booster.save_model(path)
            back = pa.GBDT.load_model(path)
            with np.load(path, allow_pickle=False) as z:
                fmt = int(z["format"])
            out[name, depthwise] = dict(case=c, booster=booster, rounds=rounds, fresh=(fresh + float(np.float32(c["baseline"]))).cpu().numpy(),
                                        reloaded=torch.equal(fresh, back.predict(c["fresh"])) and fmt == 2 and np.array_equal(back.nan_bin, booster.nan_bin))
    return out


@pytest.mark.parametrize("name,depthwise", [(n, False) for n in NAMES] + [("t", True)])
def test_whole_fits_with_nans_match_sklearn(fits, name, depthwise):
    """Trees equal to HistGradientBoostingRegressor's in canonical form (nodes, the missing rows under them, missing_go_to_left where it is
    decided, leaf row counts); training scores after every round and the compared fresh rows within C_GBDT_SK_MISSING 2^-24 max(1, max
    |score|).  Case t is fitted depth-wise as well (sklearn: max_leaf_nodes=None)."""
    fit = fits[name, depthwise]
    c, p = fit["case"], fit["case"]["params"]
    edges, nbins, nan_bin = MR.bin_edges(c["X"], p["max_bin"])
    b = fit["booster"]
    assert np.array_equal(b.edges, edges) and np.array_equal(b.nbins, nbins) and np.array_equal(b.nan_bin, nan_bin)
    assert np.array_equal(b.bins.cpu().numpy()[:, :c["X"].shape[1]], MR.bin_matrix(c["X"], edges, nbins, nan_bin))
    assert len(fit["rounds"]) == p["rounds"]
    for r, (tree, scores) in enumerate(fit["rounds"]):
        nodes, leaves = MR.canonical(tree, c["X"])
        miss = MR.tree_mismatch(nodes, leaves, c, r)
        assert miss is None, f"round {r}: {miss}"
        err = float(np.abs(scores.astype(np.float64) - c["staged"][r]).max())
        print(f"MEASURED gbdt missing vs sklearn, case {name} round {r}: training scores need C >= {err / SK.need_unit(c['staged'][r]):.2f}")
        assert err <= MR.gate(c["staged"][r]), r
    keep = c["fresh_compared"]
    err = float(np.abs(fit["fresh"].astype(np.float64) - c["fresh_pred"])[keep].max())
    print(f"MEASURED gbdt missing vs sklearn, case {name}: {int(keep.sum())} fresh rows need C >= {err / SK.need_unit(c['fresh_pred']):.2f}")
    assert err <= MR.gate(c["fresh_pred"])
    assert fit["reloaded"]                                               # format 2 saved and loaded: the same bits


@pytest.mark.parametrize("name", NAMES)
def test_whole_fits_equal_the_restatement_bit_for_bit(fits, name):
    fit = fits[name, False]
    want, fresh, _ = MR.run_restatement(fit["case"])
    for r, ((tree, scores), (ref, ref_scores)) in enumerate(zip(fit["rounds"], want)):
        for k in ("feature", "left", "right", "default_left"):
            assert np.array_equal(tree[k], ref[k]) and tree[k].dtype == ref[k].dtype, (r, k)
        assert np.array_equal(bits(tree["threshold"]), bits(ref["threshold"])) and np.array_equal(bits(tree["value"]), bits(ref["value"])), r
        assert np.array_equal(bits(scores), bits(ref_scores)), r
    assert np.array_equal(bits(fit["fresh"]), bits(fresh))


def test_leafwise_equals_depthwise_where_the_cap_cannot_bind(fits):
    lw, dw = fits["t", False], fits["t", True]
    X = lw["case"]["X"]
    for (a, sa), (b, sb) in zip(lw["rounds"], dw["rounds"]):
        for x, y in zip(MR.canonical(a, X), MR.canonical(b, X)):
            assert np.array_equal(x, y)                                  # fp32 thresholds and values as float64: equal bits
        assert np.array_equal(bits(sa), bits(sb))
    assert np.array_equal(bits(lw["fresh"]), bits(dw["fresh"]))
    assert dw["booster"].host_reads < lw["booster"].host_reads


def test_two_fits_give_the_same_bits(fits):
    for depthwise in (False, True):
        first = fits["t", depthwise]
        _, again = fit_case(first["case"], depthwise)
        for (a, sa), (b, sb) in zip(first["rounds"], again):
            assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a) and np.array_equal(bits(sa), bits(sb))


# ---------------------------------------------------------------- bagging and GOSS with NaNs
@pytest.mark.parametrize("depthwise", [False, True])
@pytest.mark.parametrize("extra", [{"bagging_fraction": 0.5, "bagging_freq": 1}, {"data_sample_strategy": "goss", "learning_rate": 0.5}], ids=["bagging", "goss"])
def test_sampled_fits_with_nans_keep_scores_equal_to_predict(fits, extra, depthwise, monkeypatch):
    """The rows outside the bag reach their leaf through the binned walk, NaN bins included: scores stay predict(X) bit for bit, and every
    device-to-host read inside update() is one host_reads counts."""
    c = fits["t", False]["case"]
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(1), real(self, *a, **k))[1])
    booster, rounds = fit_case(c, depthwise, extra, rounds=4, baseline=False)
    monkeypatch.undo()
    assert len(reads) == booster.host_reads + 4                           # fit_case reads the scores once per round itself
    if depthwise:                                                         # one read for the root, one per level that searched: what it was
        assert booster.host_reads <= 4 * (1 + c["params"]["max_depth"])
    assert np.array_equal(bits(booster.scores), bits(booster.predict(c["X"])))
    assert any(t["default_left"].any() for t, _ in rounds) and all("default_left" in t for t, _ in rounds)
    nodes = np.concatenate([MR.canonical(t, c["X"])[0] for t, _ in rounds])
    assert ((nodes[:, 4] > 0) & (nodes[:, 3] == 1)).any()                 # missing rows that went left, out of the bag too


# ---------------------------------------------------------------- other behaviour
@pytest.mark.parametrize("policy", ["leafwise", "depthwise"])
def test_data_without_a_nan_give_the_same_model_under_the_switch(policy):
    import ptranking_amd as pa
    c = SK.load()[0]["a"]
    p = dict(SK.booster_params(c["params"]), grow_policy=policy, max_depth=3 if policy == "depthwise" else -1)
    y = dev(c["y"])
    models = []
    for use in (False, True):
        b = pa.GBDT(dict(p, use_missing=use), c["X"])
        for _ in range(4):
            b.update(b.scores - y, torch.ones_like(y))
        models.append(b)
    off, on = models
    assert (on.nan_bin == -1).all() and torch.equal(off.bins, on.bins) and off.host_reads == on.host_reads
    assert np.array_equal(bits(off.scores), bits(on.scores)) and np.array_equal(bits(off.predict(c["fresh"])), bits(on.predict(c["fresh"])))
    for a, b in zip(off.trees, on.trees):
        assert "default_left" not in a and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
        at = {0: np.arange(c["X"].shape[0])}
        for i in range(a["feature"].size):                               # default_left is the child with more training rows
            rows = at.pop(i)
            left = c["X"][rows, a["feature"][i]] <= a["threshold"][i]
            assert b["default_left"][i] == int(left.sum() > (~left).sum()), i
            for child, part in ((a["left"][i], rows[left]), (a["right"][i], rows[~left])):
                if child >= 0:
                    at[int(child)] = part
    fresh = c["fresh"].copy()
    fresh[::3, 1] = np.nan
    assert np.array_equal(bits(on.predict(fresh)), bits(MR.predict(fresh, on.trees)))      # a NaN follows the majority child
    with pytest.raises(ValueError, match="missing values are not handled"):
        off.predict(fresh)
    fresh[0, 0] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        on.predict(fresh)


def test_lambdamart_fit_with_nans_in_x_and_in_the_eval_set():
    import ptranking_amd as pa
    rng = np.random.default_rng(3)
    group = rng.integers(5, 40, 60)
    n = int(group.sum())
    X = rng.standard_normal((n, 6)).astype(np.float32)
    y = np.clip(np.rint(X[:, 0] + 0.5 * X[:, 1] + 0.3 * rng.standard_normal(n) + 1), 0, 4).astype(np.float32)
    X[rng.random(n) < 0.3, 0] = np.nan
    X[rng.random(n) < 0.2, 3] = np.nan
    vg = rng.integers(5, 40, 20)
    nv = int(vg.sum())
    Xv = rng.standard_normal((nv, 6)).astype(np.float32)
    yv = np.clip(np.rint(Xv[:, 0] + 0.5 * Xv[:, 1] + 1), 0, 4).astype(np.float32)
    Xv[rng.random(nv) < 0.3, 0] = np.nan
    Xv[rng.random(nv) < 0.3, 5] = np.nan                                  # a feature that never had a NaN in training
    params = {"num_leaves": 8, "min_data_in_leaf": 5, "learning_rate": 0.2, "num_trees": 6, "max_bin": 63}
    with pytest.raises(ValueError, match="missing values are not handled"):
        pa.LambdaMART(params).fit(X, y, group)
    with pytest.raises(ValueError, match="missing values are not handled"):
        pa.LambdaMART(params).fit(np.nan_to_num(X), y, group, eval_set=(Xv, yv), eval_group=vg)
    m = pa.LambdaMART(dict(params, use_missing=True)).fit(X, y, group, eval_set=(Xv, yv), eval_group=vg, eval_at=5)
    assert len(m.evals_result) == 6 and all(0.0 < s <= 1.0 for s in m.evals_result)
    b = m.booster
    assert b.nan_bin.tolist() == [b.nbins[0], -1, -1, b.nbins[3], -1, -1] and any(t["default_left"].any() for t in b.trees)
    assert np.array_equal(bits(b.scores), bits(m.predict(X)))
    assert np.array_equal(bits(m.predict(Xv)), bits(MR.predict(Xv, b.trees)))
    Xv[0, 0] = -np.inf
    with pytest.raises(ValueError, match="infinity"):
        pa.LambdaMART(dict(params, use_missing=True)).fit(X, y, group, eval_set=(Xv, yv), eval_group=vg)
