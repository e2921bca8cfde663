"""GPU: categorical features in the native booster (categorical_feature; the *_cat entry points of csrc/gbdt.hip) against the numpy
restatement tests/gbdt_cat_ref.py, bit for bit, and whole fits against scikit-learn's HistGradientBoostingRegressor(categorical_features=...)
(tests/golden/gbdt_sklearn_cat.npz) under the gate the restatement set (test_gbdt_cat_cpu.py)."""
import zipfile

import numpy as np
import pytest
import torch

import gbdt_cat_ref as CR
import gbdt_missing_ref as MR
import gbdt_ref as R
import gbdt_sk as SK

pytestmark = pytest.mark.gpu
EXPO = (10, 10)
ONE = 1 << 10                                                            # a Hessian of 1.0 per row in fixed point
SMOOTH = 3.0                                                             # cat_smooth of the hand-made histograms: three rows of unit Hessian
MAX_BIN = 256
IS_CAT = np.array([1, 0, 1, 1, 0], np.uint8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


# ---------------------------------------------------------------- the split scan on hand-made histograms
def scan_leaf(u, kind, nan, seed):
    """One leaf's histograms [5, 256, 3] summed from synthetic rows, so that every feature holds the node's totals.  Feature 0 is
    categorical with exactly u used codes scattered over the 256 bins (3 or 4 rows each), a few codes of 1 or 2 rows (low support) and
    empty bins; feature 1 numeric (7 bins); feature 2 categorical (5 codes) with its NaN bin at 5 under nan = 'used' (many rows there) or
    'unused' (one row); feature 3 categorical (23 codes); feature 4 numeric (40 bins).  kind 'unit': Hessians of 1; 'weights': Hessians
    in [1/2, 2) so that TC / TH != 1; 'ties': gradients that depend on the code's parity alone, so that many keys are equal.
    -> (hist, nbins, nan_bin or None, the used codes of feature 0)."""
    rng = np.random.default_rng([u, ("unit", "weights", "ties").index(kind), (None, "used", "unused").index(nan), seed])
    perm = rng.permutation(256)
    used, low = perm[:u], perm[u:u + min(256 - u, 9)]
    col0 = np.concatenate([np.repeat(used, 3), used[:u // 2], np.repeat(low, 1), low[:3]]).astype(np.int64)
    if u == 0:
        col0 = np.repeat(perm[:20], 2).astype(np.int64)                  # no code reaches three rows
    elif col0.size < 40:
        col0 = np.concatenate([col0, np.repeat(used[:1], 40 - col0.size)])     # rows enough for the other features; the code was used already
    n = col0.size
    b = np.stack([col0, rng.integers(0, 7, n), rng.integers(0, 5, n), rng.integers(0, 23, n), rng.integers(0, 40, n)], axis=1)
    nbins = np.array([int(col0.max()) + 1, 7, 5, 23, 40], np.int32)
    nan_bin = None
    if nan is not None:
        nan_bin = np.array([-1, -1, 5, -1, 7 if nan == "used" else -1], np.int32)      # (feature 4's NaN bin lies inside its value bins: reads as none)
        miss = rng.random(n) < 0.3 if nan == "used" else np.arange(n) == n // 2
        b[miss, 2] = 5
    lift = rng.standard_normal(256) * 6 * ONE
    if kind == "ties":
        qg = np.where(col0 % 2 == 0, -5 * ONE, 5 * ONE) + np.where(b[:, 2] == 5, 3 * ONE, 0)
        qh = np.full(n, ONE, np.int64)
    else:
        qg = (lift[col0] + rng.integers(-ONE, ONE, n) + np.where(b[:, 2] == 5, -9 * ONE, 0) + (b[:, 3] % 3) * ONE).astype(np.int64)
        qh = rng.integers(ONE // 2, 2 * ONE, n) if kind == "weights" else np.full(n, ONE, np.int64)
    hist = R.histogram(b.astype(np.uint8), qg.astype(np.int32), qh.astype(np.int32), None, MAX_BIN)
    return hist, nbins, nan_bin, used


def device_search(hists, nbins, nan_bin, is_cat=IS_CAT, smooth=SMOOTH, **kw):
    from ptranking_amd import functional as F
    rec, sets = F.gbdt_best_split_cat(dev(np.stack(hists)), dev(nbins), dev(np.array(EXPO, np.int32)), dev(is_cat), smooth, kw.get("l2", 0.0),
                                      kw.get("min_data", 1), kw.get("min_hess", 1e-3), kw.get("min_gain", 0.0), nan_bin=None if nan_bin is None else dev(nan_bin))
    return rec.cpu().numpy(), sets.cpu().numpy()


def restated(hist, nbins, nan_bin, is_cat=IS_CAT, smooth=SMOOTH, **kw):
    s = CR.best_split(hist, nbins, nan_bin, is_cat, EXPO, kw.get("l2", 0.0), kw.get("min_data", 1), kw.get("min_hess", 1e-3), kw.get("min_gain", 0.0), smooth)
    return s, CR.record(s, nan_bin is not None)


@pytest.mark.parametrize("nan", [None, "used", "unused"])
@pytest.mark.parametrize("u", [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256])
def test_split_scan_equals_the_restatement(u, nan):
    """Records and left sets bit for bit: 3 leaves x 5 features in one call (15 wavefronts: no multiple of the 4 of a workgroup), numeric
    and categorical features mixed, low-support and empty bins, equal keys, the NaN bin used and unused."""
    from ptranking_amd import functional as F
    leaves = [scan_leaf(u, kind, nan, 0) for kind in ("unit", "weights", "ties")]
    nbins = np.max([lf[1] for lf in leaves], axis=0).astype(np.int32)   # one nbins per call: the widest leaf's (the bins behind a leaf's codes are empty)
    nan_bin = leaves[0][2]
    rec, sets = device_search([lf[0] for lf in leaves], nbins, nan_bin)
    for k, (hist, _, _, used) in enumerate(leaves):
        if k != 1:                                                       # unit Hessians: the used codes are the ones of three rows and more
            h0 = hist[0]
            assert int(((h0[:, 2] > 0) & (h0[:, 1] / ONE >= SMOOTH)).sum()) == u == used.size
        s, (want, want_set) = restated(hist, nbins, nan_bin)
        assert np.array_equal(rec[k], want), (k, rec[k].tolist(), want.tolist(), s)
        assert np.array_equal(sets[k], want_set), (k, sets[k].tolist(), want_set.tolist())
        # feature 0 alone: its own record, whichever feature wins the leaf
        only = np.array([1, 0, 0, 0, 0], np.uint8)
        one = np.zeros_like(hist)
        one[0] = hist[0]
        one[1:, 0] = hist[0].sum(axis=0)                                 # the other features: everything in bin 0, no candidate
        nb1 = np.array([nbins[0], 1, 1, 1, 1], np.int32)
        s0, (want, want_set) = restated(one, nb1, None, only)
        r0, t0 = device_search([one], nb1, None, only)
        assert np.array_equal(r0[0], want) and np.array_equal(t0[0], want_set), (k, r0[0].tolist(), want.tolist())
        if u <= 1:
            assert s0["feature"] == -1 and not t0.any()
        elif k == 0:
            assert s0["feature"] == 0 and s0["cat"] and 1 <= s0["bin"] <= (u + 1) // 2 and bin(s0["set"]).count("1") == s0["bin"]
    # the slot form equals the contiguous form, out of order and with a slot outside the pool
    slots = [2, 0, 5, 1, -1]
    got, got_sets = F.gbdt_best_split_slots_cat(dev(np.stack([lf[0] for lf in leaves])), slots, dev(nbins), dev(np.array(EXPO, np.int32)), dev(IS_CAT), SMOOTH,
                                                0.0, 1, 1e-3, 0.0, nan_bin=None if nan_bin is None else dev(nan_bin))
    got, got_sets = got.cpu().numpy(), got_sets.cpu().numpy()
    none = R.record(R.best_split(np.zeros((5, MAX_BIN, 3), np.int64), nbins, EXPO))
    for k, slot in enumerate(slots):
        assert np.array_equal(got[k], rec[slot] if 0 <= slot < 3 else none), slot
        assert np.array_equal(got_sets[k], sets[slot] if 0 <= slot < 3 else np.zeros(4, np.int64)), slot


def test_split_scan_nan_bin_is_one_more_category():
    hist, nbins, nan_bin, _ = scan_leaf(4, "unit", "used", 1)
    only = np.array([0, 0, 1, 0, 0], np.uint8)
    s, (want, want_set) = restated(hist, nbins, nan_bin, only)
    rec, sets = device_search([hist], nbins, nan_bin, only)
    assert np.array_equal(rec[0], want) and np.array_equal(sets[0], want_set)
    assert s["feature"] == 2 and s["cat"] and s["default_left"] == 1 and (s["set"] >> 5) & 1 and rec[0, 2] == s["bin"] + 256
    faulty = CR.best_split(hist, nbins, nan_bin, only, EXPO, 0.0, 1, 1e-3, 0.0, SMOOTH, fault="nan_ignored")
    assert faulty["set"] != s["set"]
    hist, nbins, nan_bin, _ = scan_leaf(4, "unit", "unused", 1)           # one missing row: below the support, it goes right
    s, (want, want_set) = restated(hist, nbins, nan_bin, only)
    rec, sets = device_search([hist], nbins, nan_bin, only)
    assert np.array_equal(rec[0], want) and np.array_equal(sets[0], want_set) and s["default_left"] == 0 and hist[2, 5, 2] == 1


@pytest.mark.parametrize("kw", [{"min_data": 40}, {"min_hess": 60.0}, {"min_gain": 1e9}, {"l2": 2.5}, {"smooth": 0.0}, {"smooth": 4.0}, {"smooth": 1e6}])
def test_split_scan_constraints_and_cat_smooth(kw):
    kw = dict(kw)
    smooth = kw.pop("smooth", SMOOTH)
    for kind in ("unit", "weights"):
        hist, nbins, _, _ = scan_leaf(64, kind, None, 2)
        s, (want, want_set) = restated(hist, nbins, None, smooth=smooth, **kw)
        rec, sets = device_search([hist], nbins, None, smooth=smooth, **kw)
        assert np.array_equal(rec[0], want) and np.array_equal(sets[0], want_set), (kind, rec[0].tolist(), want.tolist())


@pytest.mark.parametrize("nan", [None, "used"])
def test_numeric_features_give_the_bits_of_the_existing_entry_points(nan):
    from ptranking_amd import functional as F
    leaves = [scan_leaf(65, kind, nan, 3) for kind in ("unit", "weights", "ties")]
    nbins = np.max([lf[1] for lf in leaves], axis=0).astype(np.int32)
    nan_bin = leaves[0][2]
    hists = dev(np.stack([lf[0] for lf in leaves]))
    old = F.gbdt_best_split(hists, dev(nbins), dev(np.array(EXPO, np.int32)), 0.0, 1, 1e-3, 0.0, nan_bin=None if nan_bin is None else dev(nan_bin))
    rec, sets = device_search([lf[0] for lf in leaves], nbins, nan_bin, np.zeros(5, np.uint8))
    assert np.array_equal(rec, old.cpu().numpy()) and not sets.any()


# ---------------------------------------------------------------- the partitions
def random_set(rng):
    return rng.integers(0, 2 ** 63, 4).astype(np.int64) * np.array([1, -1, 1, -1], np.int64)


@pytest.mark.parametrize("m", [0, 1, 1023, 1024, 1025, 3000])
def test_partition_by_a_set(m):
    from ptranking_amd import functional as F
    rng = np.random.default_rng(m)
    n, nf = 3000, 5
    b = np.zeros((n, 16), np.uint8)
    b[:, :nf] = rng.integers(0, 256, (n, nf))
    b[::7, 1] = 9                                                        # feature 1's NaN bin
    rows = rng.permutation(n)[:m].astype(np.int32)
    st = random_set(rng)
    is_cat = np.array([0, 0, 1, 0, 1], np.uint8)
    nan_bin = np.array([-1, 9, -1, -1, -1], np.int32)
    inset = lambda v: np.array([(CR.set_bits(st) >> int(x)) & 1 for x in v], bool)
    for f, bin_, dl, nb in ((2, 0, 0, None), (4, 200, 1, nan_bin), (1, 100, 0, nan_bin), (1, 4, 1, nan_bin), (1, 4, 1, None)):
        v = b[rows, f]
        left = inset(v) if is_cat[f] else ((v <= bin_) | ((v == 9) & bool(dl) & (nb is not None)))
        out, lc = F.gbdt_partition_cat(dev(b), dev(rows), f, bin_, nf, dev(is_cat), st, default_left=dl, nan_bin=None if nb is None else dev(nb))
        assert int(lc.cpu()) == int(left.sum()), (f, m)
        assert np.array_equal(out.cpu().numpy(), np.concatenate([rows[left], rows[~left]])), (f, m)


@pytest.mark.parametrize("K", [1, 3])
def test_partition_segments_by_sets(K):
    from ptranking_amd import functional as F
    rng = np.random.default_rng(K)
    n, nf = 5000, 5
    b = np.zeros((n, 16), np.uint8)
    b[:, :nf] = rng.integers(0, 256, (n, nf))
    b[::5, 1] = 9
    is_cat = np.array([0, 0, 1, 0, 1], np.uint8)
    nan_bin = np.array([-1, 9, -1, -1, -1], np.int32)
    rows = rng.permutation(n).astype(np.int32)
    segs = [(0, 1500, 2, 0, 0), (1500, 1025, 1, 60, 1), (2600, 2000, 4, 0, 0)][:K]
    segs.append((4000, 2000, 2, 0, 0) if K == 1 else (4700, 100, 7, 0, 0))      # the bad one: it leaves the list / names no feature
    sets = np.stack([random_set(rng) for _ in segs])
    out, lc = F.gbdt_partition_segments_cat(dev(b), dev(rows), np.array(segs), sets, nf, dev(is_cat), nan_bin=dev(nan_bin))
    want, counts = rows.copy(), []
    for (s, c, f, bin_, dl), st in list(zip(segs, sets))[:K]:
        part = rows[s:s + c]
        v = b[part, f]
        left = np.array([(CR.set_bits(st) >> int(x)) & 1 for x in v], bool) if is_cat[f] else ((v <= bin_) | ((v == 9) & bool(dl)))
        want[s:s + c] = np.concatenate([part[left], part[~left]])
        counts.append(int(left.sum()))
    assert np.array_equal(out.cpu().numpy(), want)
    assert lc.cpu().numpy().tolist() == counts + [0]


# ---------------------------------------------------------------- the walks
def hand_forest():
    """Two trees over 4 features (0 and 2 categorical): tree 0 = cat(f0) -> [num(f1), cat(f2)], tree 1 = num(f3) -> [leaf, cat(f0)]."""
    s0 = sum(1 << c for c in (1, 4, 7, 13))
    s1 = sum(1 << c for c in (0, 2, 5)) | (1 << 6)                      # bit 6: feature 2's NaN bin
    s2 = sum(1 << c for c in (3, 200))
    t0 = {"feature": np.array([0, 1, 2], np.int32), "threshold": np.array([0, 1.25, 0], np.float32), "left": np.array([1, ~0, ~2], np.int32),
          "right": np.array([2, ~1, ~3], np.int32), "value": np.array([0.5, -1.25, 2.0, -3.5], np.float32), "default_left": np.array([0, 1, 1], np.uint8),
          "cat_index": np.array([0, -1, 1], np.int32), "cat_set": np.stack([CR.set_words(s0), CR.set_words(s1)]), "split_bin": np.array([0, 2, 0], np.int32)}
    t1 = {"feature": np.array([3, 0], np.int32), "threshold": np.array([2.5, 0], np.float32), "left": np.array([~0, ~1], np.int32),
          "right": np.array([1, ~2], np.int32), "value": np.array([0.125, 7.0, -0.75], np.float32), "default_left": np.array([0, 0], np.uint8),
          "cat_index": np.array([-1, 0], np.int32), "cat_set": np.stack([CR.set_words(s2)]), "split_bin": np.array([5, 0], np.int32)}
    return [t0, t1]


def flat_forest(trees):
    cat = lambda k, dt: np.concatenate([t[k] for t in trees]).astype(dt)
    base = np.cumsum([0] + [t["cat_set"].shape[0] for t in trees])
    return {"feature": cat("feature", np.int32), "threshold": cat("threshold", np.float32), "left": cat("left", np.int32), "right": cat("right", np.int32),
            "value": cat("value", np.float32), "default_left": cat("default_left", np.uint8),
            "tree_offsets": np.cumsum([0] + [t["feature"].size for t in trees]).astype(np.int32),
            "cat_index": np.concatenate([np.where(t["cat_index"] >= 0, t["cat_index"] + b, -1) for t, b in zip(trees, base)]).astype(np.int32),
            "cat_sets": np.concatenate([t["cat_set"] for t in trees]).astype(np.int64)}


def device_predict(fl, X, is_cat, default_left=True, **over):
    from ptranking_amd import functional as F
    a = {k: dev(over.get(k, v)) for k, v in fl.items()}
    return F.gbdt_predict_cat(dev(X), a["feature"], a["threshold"], a["left"], a["right"], a["value"], a["tree_offsets"], dev(is_cat), a["cat_index"],
                              a["cat_sets"], default_left=a["default_left"] if default_left else None).cpu().numpy()


def test_walks_on_a_hand_built_forest():
    from ptranking_amd import functional as F, gbdt
    rng = np.random.default_rng(5)
    trees = hand_forest()
    fl = flat_forest(trees)
    is_cat = np.array([1, 0, 1, 0], np.uint8)
    n = 700                                                              # three workgroups of the walk
    X = np.stack([rng.integers(0, 16, n), rng.integers(0, 5, n) * 0.5, rng.integers(0, 6, n), rng.integers(0, 8, n) * 0.5 + 0.25], axis=1).astype(np.float32)
    X[rng.random(n) < 0.2, 2] = np.nan
    X[:6, 0] = [200, 13, 7, 4, 1, 15]
    got = device_predict(fl, X, is_cat)
    assert np.array_equal(bits(got), bits(CR.predict(X, trees)))
    # the binned walk lands where the raw walk lands
    edges, nbins, nan_bin = gbdt.bin_edges(X, 256, True, categorical=(0, 2))
    assert nbins[0] == 201 and nan_bin[2] == 6 and nbins[2] == 6
    trees[0]["threshold"][1], trees[1]["threshold"][0] = edges[1, 2], edges[3, 5]
    fl = flat_forest(trees)
    got = device_predict(fl, X, is_cat)
    assert np.array_equal(bits(got), bits(CR.predict(X, trees)))
    b = F.gbdt_bin(dev(X), dev(edges), dev(nbins), nan_bin=dev(nan_bin))
    scores = torch.zeros(n, device="cuda")
    rows = dev(rng.permutation(n).astype(np.int32))
    for t in trees:
        F.gbdt_add_tree_binned_cat(scores, b, 4, rows, dev(t["feature"]), dev(t["split_bin"]), dev(t["left"]), dev(t["right"]), dev(t["value"]), dev(is_cat),
                                   dev(t["cat_index"]), dev(t["cat_set"]), default_left=dev(t["default_left"]), nan_bin=dev(nan_bin))
    assert np.array_equal(bits(scores), bits(got))
    # raw rows that are no codes: unseen codes, non-integers, values outside 0 .. 255, NaN with and without default_left
    odd = np.array([[200, 0.5, 3, 9.0], [201, 0.5, 3, 9.0], [255, 0.5, 2, 9.0], [256, 0.5, 2, 9.0], [4.5, 0.5, 2, 9.0], [-1, 0.5, 2, 9.0],
                    [1e9, 0.5, 2.000001, 9.0], [-0.0, 0.5, np.nan, 9.0], [np.nan, np.nan, np.nan, 9.0], [4, np.nan, 0, np.nan], [3, 0.5, 0, 9.0]], np.float32)
    got = device_predict(fl, odd, is_cat)
    assert np.array_equal(bits(got), bits(CR.predict(odd, trees)))
    assert got[0] == np.float32(-3.5) + np.float32(7.0) and got[10] == np.float32(2.0) + np.float32(7.0)      # the codes 200 and 3 are in s2 alone
    assert got[1] == np.float32(-3.5) + np.float32(-0.75)                 # code 201: in no set
    no_dl = [{k: v for k, v in t.items() if k != "default_left"} for t in trees]
    assert np.array_equal(bits(device_predict(fl, odd, is_cat, default_left=False)), bits(CR.predict(odd, no_dl)))      # a NaN then goes right everywhere
    # malformed trees give NaN and read nothing out of range: a set index past the sets, a node whose kind is not its feature's, a cycle
    ok = device_predict(fl, X, is_cat)
    for over in ({"cat_index": np.array([0, -1, 7, -1, 2], np.int32)}, {"cat_index": np.array([-1, -1, 1, -1, 2], np.int32)},
                 {"cat_index": np.array([0, 0, 1, -1, 2], np.int32)}, {"left": np.array([0, ~0, ~2, ~0, ~1], np.int32)},
                 {"feature": np.array([0, 1, 9, 3, 0], np.int32)}):
        bad = device_predict(fl, X, is_cat, **over)
        assert np.isnan(bad).any() and (np.isnan(bad) | (bad == ok)).all(), over


# ---------------------------------------------------------------- whole fits against scikit-learn
NAMES = ("a", "b", "c", "d", "e", "f")


def fit_case(c, extra=None, rounds=None, baseline=True, params=None):
    import ptranking_amd as pa
    p = c["params"]
    booster = pa.GBDT(dict(CR.booster_params(p) if params is None else params, **(extra or {})), c["X"])
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
    cases, out = CR.load()[0], {}
    assert tuple(sorted(cases)) == NAMES
    for name, c in cases.items():
        booster, rounds = fit_case(c)
        fresh = booster.predict(c["fresh"])
        path = tmp_path_factory.mktemp("cat") / f"{name}.npz"
        booster.save_model(path)
        back = pa.GBDT.load_model(path)
        with np.load(path, allow_pickle=False) as z:
            fmt = int(z["format"])
        staged = all(torch.equal(booster.predict(c["fresh"], num_iteration=k + 1, first_tree=k), back.predict(c["fresh"], num_iteration=k + 1, first_tree=k))
                     for k in range(len(rounds)))
        out[name] = dict(case=c, booster=booster, rounds=rounds, fresh=(fresh + float(np.float32(c["baseline"]))).cpu().numpy(),
                         reloaded=torch.equal(fresh, back.predict(c["fresh"])) and fmt == 3 and staged)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_whole_fits_match_sklearn(fits, name):
    """Trees equal to HistGradientBoostingRegressor's in canonical form (nodes, left code sets, missing_go_to_left where NaNs decide it,
    leaf row counts); training scores after every round and the fresh rows within C_GBDT_SK_CAT 2^-24 max(1, max |score|).  Case f is
    fitted depth-wise (sklearn: max_leaf_nodes=None)."""
    fit = fits[name]
    c, p, b = fit["case"], fit["case"]["params"], fit["booster"]
    edges, nbins, nan_bin, is_cat, binned = CR.setup(c)
    assert np.array_equal(b.edges, edges) and np.array_equal(b.nbins, nbins) and (nan_bin is None or np.array_equal(b.nan_bin, nan_bin))
    assert np.array_equal(b.bins.cpu().numpy()[:, :c["X"].shape[1]], binned)
    assert len(fit["rounds"]) == p["rounds"] and (b.params["grow_policy"] == "depthwise") == bool(p["depthwise"])
    for r, (tree, scores) in enumerate(fit["rounds"]):
        nodes, leaves = CR.canonical(tree, c["X"], nbins)
        miss = CR.tree_mismatch(nodes, leaves, c, r)
        assert miss is None, f"round {r}: {miss}"
        err = float(np.abs(scores.astype(np.float64) - c["staged"][r]).max())
        print(f"MEASURED gbdt categorical vs sklearn, case {name} round {r}: training scores need C >= {err / SK.need_unit(c['staged'][r]):.2f}")
        assert err <= CR.gate(c["staged"][r]), r
    err = float(np.abs(fit["fresh"].astype(np.float64) - c["fresh_pred"]).max())
    print(f"MEASURED gbdt categorical vs sklearn, case {name}: fresh rows need C >= {err / SK.need_unit(c['fresh_pred']):.2f}")
    assert err <= CR.gate(c["fresh_pred"])
    assert fit["reloaded"]                                               # format 3 saved and loaded: the same bits, tree by tree too


@pytest.mark.parametrize("name", NAMES)
def test_whole_fits_equal_the_restatement_bit_for_bit(fits, name):
    fit = fits[name]
    want, fresh, _ = CR.run_restatement(fit["case"])
    for r, ((tree, scores), (ref, ref_scores)) in enumerate(zip(fit["rounds"], want)):
        if not fit["case"]["params"]["depthwise"]:                      # depth-wise numbers its nodes by level: compared in canonical form above
            for k in ("feature", "left", "right", "cat_index", "cat_set") + (("default_left",) if "default_left" in ref else ()):
                assert np.array_equal(tree[k], ref[k]) and tree[k].dtype == ref[k].dtype, (r, k)
            assert np.array_equal(bits(tree["threshold"]), bits(ref["threshold"])) and np.array_equal(bits(tree["value"]), bits(ref["value"])), r
        assert np.array_equal(bits(scores), bits(ref_scores)), r
    assert np.array_equal(bits(fit["fresh"]), bits(fresh))


# ---------------------------------------------------------------- invariants
def test_leafwise_equals_depthwise_where_the_cap_cannot_bind(fits):
    dw = fits["f"]
    c = dw["case"]
    params = {k: v for k, v in CR.booster_params(c["params"]).items() if k != "grow_policy"}
    booster, lw = fit_case(c, params=params)
    nbins = dw["booster"].nbins
    for (a, sa), (b, sb) in zip(lw, dw["rounds"]):
        for x, y in zip(CR.canonical(a, c["X"], nbins), CR.canonical(b, c["X"], nbins)):
            assert np.array_equal(x, y)
        assert np.array_equal(bits(sa), bits(sb))
    assert dw["booster"].host_reads < booster.host_reads


def test_two_fits_give_the_same_bits(fits):
    for name in ("c", "f"):
        first = fits[name]
        _, again = fit_case(first["case"])
        for (a, sa), (b, sb) in zip(first["rounds"], again):
            assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a) and np.array_equal(bits(sa), bits(sb))


@pytest.mark.parametrize("policy", ["leafwise", "depthwise"])
def test_host_reads_equal_those_of_the_numeric_fit_of_the_same_shape(fits, policy):
    """The left set rides in the read that brings the records.  Columns of two codes make the twin: a set split {0} | {1} and the numeric
    split at 0.5 are one partition with the same integer sums, so both fits grow trees of one shape (a categorical node may have its
    children exchanged: the lower key goes left) with the same fp32 scores, and must cost the same reads.  min_data_in_leaf 20 keeps
    every code of a valid split above cat_smooth."""
    c = dict(fits["b"]["case"])
    ncat = c["params"]["ncat"]
    c["X"] = c["X"].copy()
    c["X"][:, :ncat] = c["X"][:, :ncat] % 2
    params = dict(CR.booster_params(c["params"]), grow_policy=policy, num_leaves=8)
    assert params["min_data_in_leaf"] == 20 and c["w"] is None
    cat_b, cat_r = fit_case(c, params=params, rounds=3)
    num_b, num_r = fit_case(c, params={k: v for k, v in params.items() if k not in ("categorical_feature", "cat_smooth")}, rounds=3)
    assert any((t["cat_index"] >= 0).any() for t, _ in cat_r)
    for (a, sa), (b, sb) in zip(cat_r, num_r):
        assert a["feature"].size == b["feature"].size and sorted(a["feature"].tolist()) == sorted(b["feature"].tolist())
        assert np.array_equal(bits(sa), bits(sb))
    assert cat_b.host_reads == num_b.host_reads > 3


@pytest.mark.parametrize("policy", ["leafwise", "depthwise"])
@pytest.mark.parametrize("extra", [{"bagging_fraction": 0.5, "bagging_freq": 1}, {"data_sample_strategy": "goss", "learning_rate": 0.5}], ids=["bagging", "goss"])
def test_sampled_fits_keep_scores_equal_to_predict(fits, extra, policy, monkeypatch):
    """The rows outside the bag walk the categorical tree on their bins: scores stay predict(X) bit for bit, and every device-to-host read
    inside update() is one host_reads counts."""
    c = fits["c"]["case"]
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(1), real(self, *a, **k))[1])
    booster, rounds = fit_case(c, dict(extra, grow_policy=policy), rounds=4, baseline=False)
    monkeypatch.undo()
    assert len(reads) == booster.host_reads + 4                           # fit_case reads the scores once per round itself
    assert np.array_equal(bits(booster.scores), bits(booster.predict(c["X"])))
    assert any((t["cat_index"] >= 0).any() for t, _ in rounds)


def test_an_empty_categorical_feature_changes_nothing(fits, tmp_path):
    import ptranking_amd as pa
    c = fits["b"]["case"]
    base = {k: v for k, v in CR.booster_params(c["params"]).items() if k not in ("categorical_feature", "cat_smooth")}
    files = []
    for k, prm in enumerate((base, dict(base, categorical_feature=[], cat_smooth=3.0), dict(base, categorical_feature=()))):
        booster, rounds = fit_case(c, params=prm, rounds=2)
        assert all("cat_index" not in t for t, _ in rounds)
        booster.save_model(tmp_path / f"{k}.npz")
        with zipfile.ZipFile(tmp_path / f"{k}.npz") as z:                 # every member's bytes (the archive's own headers carry the time of writing)
            files.append([(i.filename, z.read(i.filename)) for i in z.infolist()])
    assert files[0] == files[1] == files[2]
    with np.load(tmp_path / "1.npz", allow_pickle=False) as z:
        assert int(z["format"]) == 1 and "cat_smooth" not in str(z["params"]) and "categorical_feature" not in str(z["params"])
    assert pa.GBDT.load_model(tmp_path / "1.npz").params["categorical_feature"] == ()


def test_fit_bins_and_predict_reject_what_is_no_code():
    import ptranking_amd as pa
    X = np.array([[0, 1.5], [3, 2.5], [1, 0.5], [2, 0.25]], np.float32)
    with pytest.raises(ValueError, match="categorical_feature 2"):
        pa.GBDT({"categorical_feature": [2]}, X)
    for bad in (1.5, -1.0, 8.0):
        Y = X.copy()
        Y[1, 0] = bad
        with pytest.raises(ValueError, match="integer codes"):
            pa.GBDT({"categorical_feature": [0], "max_bin": 8}, Y)
    b = pa.GBDT({"categorical_feature": [0], "max_bin": 8, "min_data_in_leaf": 1, "cat_smooth": 0.0, "num_leaves": 4}, X)
    b.update(dev(np.array([1, -1, 1, -1], np.float32)), dev(np.ones(4, np.float32)))
    assert np.array_equal(bits(b.scores), bits(b.predict(X)))
    Y = X.copy()
    Y[0, 0] = 2.5
    with pytest.raises(ValueError, match="integer codes"):
        b.predict(Y)
    got = b.predict(Y, check_finite=False).cpu().numpy()                  # unchecked: what is no code is in no set
    Y[0, 0] = 7.0                                                         # a code the training data never held: legal, and in no set either
    assert np.array_equal(bits(got), bits(b.predict(Y)))


# ---------------------------------------------------------------- LambdaMART
def test_lambdamart_finds_a_planted_set():
    """40 queries of 20 documents; relevance planted on membership in a scattered set of 5 of 23 codes: after one round with two leaves the
    root splits on that column with exactly the planted set on one side — the left one, where the relevant documents' negative
    gradients sort first."""
    import ptranking_amd as pa
    rng = np.random.default_rng(11)
    q, d = 40, 20
    planted = (1, 4, 7, 13, 20)
    X = np.stack([rng.standard_normal(q * d), rng.integers(0, 23, q * d), rng.standard_normal(q * d)], axis=1).astype(np.float32)
    X[:23, 1] = np.arange(23)
    y = np.isin(X[:, 1], planted).astype(np.float32) * 2.0
    m = pa.LambdaMART({"categorical_feature": [1], "num_leaves": 2, "num_trees": 1, "min_data_in_leaf": 5, "learning_rate": 0.5})
    m.fit(X, y, np.full(q, d))
    (tree,) = m.booster.trees
    assert tree["feature"].tolist() == [1] and tree["cat_index"].tolist() == [0]
    assert CR.set_bits(tree["cat_set"][0]) == sum(1 << c for c in planted)
    s = m.predict(X).cpu().numpy()
    assert s[y > 0].min() > s[y == 0].max()
