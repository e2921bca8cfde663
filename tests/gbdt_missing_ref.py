"""Plain-numpy restatement of the missing-value rules of the gradient-boosted trees (use_missing=True of ptranking_amd/gbdt.py; the
*_missing entry points of ptranking_amd/csrc/gbdt.hip), on top of gbdt_ref.py, and the whole-fit comparison with scikit-learn's
HistGradientBoostingRegressor on data with NaNs (tests/golden/gbdt_sklearn_missing.npz, written by
tests/golden/make_golden_gbdt_sklearn_missing.py).  Test infrastructure, never imported by the package; it needs neither a GPU nor
scikit-learn.

The rules.  A NaN is a missing value.  A feature that holds one in the training matrix is binned, without its NaNs, under max_bin - 1, and
its NaNs get the bin behind its value bins (nan_bin[f] = nbins[f]); any other feature has nan_bin[f] = -1.  Per (leaf, feature) with
(MG, MH, MC) the histogram entry of the NaN bin (zero without one) the split scan evaluates
    1. b < nbins - 1, bins <= b left, the missing rows right;
    2. only when MC > 0: b = nbins - 1, every value left and the NaNs right (threshold +inf);
    3. only when MC > 0: b < nbins - 1 with the missing rows LEFT.
The highest gain wins, then the lowest feature, then missing-right before missing-left, then the lowest bin among missing-right candidates
and the HIGHEST bin among missing-left ones: sklearn scans the missing-left candidates from the top bin down and keeps the first of equal
gains, and bins that are empty in a node make such ties (bit-equal sums, bit-equal gains) an everyday event, not a coincidence.  With
MC == 0 the rows of the node do not decide the direction and default_left = (left count > right count).  A record's field 2 is bin + 256 * default_left.  A training row
goes left iff its bin <= the split bin, or default_left is set and its bin is the feature's NaN bin; a raw row goes left on
x <= threshold, a NaN along default_left.

`fault` arguments plant one wrong rule each: "always_right" (rule 3 left out), "no_nan_split" (rule 2 left out), "tie_left" (an exact tie
of the two directions taken as missing-left), "minority" (the majority rule inverted)."""
import os

import numpy as np

import gbdt_ref as R
import gbdt_sk as SK

FAULTS = ("always_right", "no_nan_split", "tie_left", "minority")
FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gbdt_sklearn_missing.npz")
PARAM_NAMES = SK.PARAM_NAMES + ("depthwise",)

# The gate, as gbdt_sk's: |got - sklearn| <= C_GBDT_SK_MISSING * 2^-24 * max(1, max |sklearn's scores of that round|).  Twice the worst need
# of the RESTATEMENT against sklearn over every round and every compared fresh row of the fixture (test_gbdt_missing_cpu.py re-measures it
# and prints it), rounded up to an integer; never taken from the kernels' output.
C_GBDT_SK_MISSING = 4
NEED_RECORDED = 1.93                      # case p, its training scores


# ---- binning
def bin_edges(X, max_bin):
    """-> (edges float32 [F, max_bin - 1] padded with +inf, nbins int32 [F], nan_bin int32 [F]).  gbdt_ref.bin_edges of the feature's
    non-NaN rows, under max_bin - 1 where the feature holds a NaN."""
    X = np.asarray(X, np.float32)
    nf = X.shape[1]
    edges = np.full((nf, max_bin - 1), np.inf, np.float32)
    nbins, nan_bin = np.ones(nf, np.int32), np.full(nf, -1, np.int32)
    for f in range(nf):
        col = X[:, f]
        miss = np.isnan(col)
        cap = max_bin - 1 if miss.any() else max_bin
        if (~miss).any() and cap >= 2:
            e, nb = R.bin_edges(col[~miss][:, None], cap)
            edges[f, :cap - 1], nbins[f] = e[0], nb[0]
        if miss.any():
            nan_bin[f] = nbins[f]
    return edges, nbins, nan_bin


def bin_matrix(X, edges, nbins, nan_bin):
    """bins [n, F] uint8: gbdt_ref.bin_matrix for the values; a NaN gets nan_bin[f] (0 where the feature has none, as the kernel)."""
    X = np.asarray(X, np.float32)
    out = R.bin_matrix(np.where(np.isnan(X), -np.inf, X), edges, nbins)
    for f in range(X.shape[1]):
        out[np.isnan(X[:, f]), f] = max(int(nan_bin[f]), 0)
    return out


# ---- the split scan
def candidates(hist, nbins, nan_bin, expo, l2, min_data, min_hess, min_gain, fault=None):
    """-> (gain float64 [F, max_bin, 2] of every candidate (feature, bin, missing-left), -inf where it is not one or not valid; the left
    sums int64 [F, max_bin, 2, 3]; the totals [3]; MC int64 [F])."""
    hist = np.asarray(hist, np.int64)
    nf, mb, _ = hist.shape
    nbins, nan_bin = np.asarray(nbins), np.asarray(nan_bin)
    has = (nan_bin >= nbins) & (nan_bin < mb)
    M = np.where(has[:, None], hist[np.arange(nf), np.where(has, nan_bin, 0)], 0)              # [F, 3]
    values = np.where((np.arange(mb)[None, :] < nbins[:, None])[:, :, None], hist, 0)
    pre = np.cumsum(values, axis=1)
    tot = pre[0, -1] + M[0]
    left = np.stack([pre, pre + M[:, None, :]], axis=2)                                         # [F, mb, 2, 3]
    b = np.arange(mb)[None, :]
    mc = M[:, 2][:, None]
    is_cand = np.zeros((nf, mb, 2), bool)
    is_cand[:, :, 0] = (b < nbins[:, None] - 1) | ((mc > 0) & (b == nbins[:, None] - 1) & (fault != "no_nan_split"))
    is_cand[:, :, 1] = (b < nbins[:, None] - 1) & (mc > 0) & (fault != "always_right")
    G, H = np.ldexp(np.float64(tot[0]), -expo[0]), np.ldexp(np.float64(tot[1]), -expo[1])
    GL, HL = np.ldexp(left[..., 0].astype(np.float64), -expo[0]), np.ldexp(left[..., 1].astype(np.float64), -expo[1])
    GR = np.ldexp((tot[0] - left[..., 0]).astype(np.float64), -expo[0])
    HR = np.ldexp((tot[1] - left[..., 1]).astype(np.float64), -expo[1])
    CL, CR = left[..., 2], tot[2] - left[..., 2]
    floor_h = max(min_hess, 2.0 ** -40)
    ok = is_cand & (CL >= min_data) & (CR >= min_data) & (HL >= floor_h) & (HR >= floor_h)
    with np.errstate(all="ignore"):
        gain = ((GL * GL) / (HL + l2) + (GR * GR) / (HR + l2)) - (G * G) / (H + l2)
    ok &= gain >= min_gain
    return np.where(ok, gain, -np.inf), left, tot, M[:, 2]


def best_split(hist, nbins, nan_bin, expo, l2=0.0, min_data=1, min_hess=1e-3, min_gain=0.0, fault=None):
    """-> dict(gain, feature, bin, default_left, missing (the node's MC of that feature), left, right, runner_up).  runner_up: the best gain
    among the candidates that give ANOTHER partition of the node's sums (other left sums, and not the winner's exchanged): the two
    directions of one bin where MC == 0 are one candidate."""
    gain, left, tot, mc = candidates(hist, nbins, nan_bin, expo, l2, min_data, min_hess, min_gain, fault)
    best = gain.max() if gain.size else -np.inf
    if not best > -np.inf:
        return {"gain": -np.inf, "feature": -1, "bin": -1, "default_left": 0, "missing": 0, "left": (0, 0, 0), "right": (0, 0, 0),
                "runner_up": -np.inf}
    fs, bs, ds = np.nonzero(gain == best)
    key = np.where(ds == 0, bs, 511 - bs)                                # missing-right ascending, then missing-left from the top bin down
    if fault == "tie_left":
        key = np.where(ds == 1, bs, 511 - bs)
    k = int(np.lexsort((key, fs))[0])                                    # the lowest feature, then the lowest key
    f, b, d = int(fs[k]), int(bs[k]), int(ds[k])
    lsum = left[f, b, d]
    if mc[f] > 0:
        default_left = d
    else:
        default_left = int(lsum[2] > tot[2] - lsum[2])
        if fault == "minority":
            default_left = int(lsum[2] < tot[2] - lsum[2])
    same = (left == lsum).all(axis=-1) | (left == (tot - lsum)).all(axis=-1)
    rest = np.where(same, -np.inf, gain)
    lt = tuple(int(v) for v in lsum)
    return {"gain": float(best), "feature": f, "bin": b, "default_left": default_left, "missing": int(mc[f]), "left": lt,
            "right": tuple(int(t) - v for t, v in zip(tot, lt)), "runner_up": float(rest.max())}


def record(split):
    """The 9 int64 of the device's record: field 2 = bin + 256 * default_left."""
    field = split["bin"] + 256 * split["default_left"] if split["feature"] >= 0 else -1
    return np.array([np.float64(split["gain"]).view(np.int64), split["feature"], field, *split["left"], *split["right"]], np.int64)


margin = R.margin


# ---- routing
def also_left(split, nan_bin):
    """The bin that goes left beside the bins <= split bin, or -1."""
    return int(nan_bin[split["feature"]]) if split["default_left"] and nan_bin[split["feature"]] >= 0 else -1


def partition(bins, rows, feature, b, also=-1):
    """-> (left rows in their order, then right rows in theirs; left count): left iff bin <= b or bin == also."""
    rows = np.asarray(rows, np.int32)
    v = bins[rows, feature].astype(np.int64)
    left = (v <= b) | (v == also)
    return np.concatenate([rows[left], rows[~left]]).astype(np.int32), int(left.sum())


def walk_binned(bins, tree, split_bin, also):
    """The leaf index of every binned row under one tree (split_bin and also by node)."""
    out = np.zeros(bins.shape[0], np.int64)
    for i in range(bins.shape[0]):
        node = 0 if tree["feature"].size else ~0
        while node >= 0:
            v = int(bins[i, tree["feature"][node]])
            node = tree["left"][node] if (v <= split_bin[node] or v == also[node]) else tree["right"][node]
        out[i] = ~node
    return out


def predict(X, trees):
    """fp32 sum of the leaf values in tree order; left on x <= threshold, a NaN along default_left."""
    X = np.asarray(X, np.float32)
    out = np.zeros(X.shape[0], np.float32)
    for i in range(X.shape[0]):
        s = np.float32(0.0)
        for t in trees:
            node = 0 if t["feature"].size else ~0
            while node >= 0:
                x = X[i, t["feature"][node]]
                go = bool(t["default_left"][node]) if np.isnan(x) else bool(x <= t["threshold"][node])
                node = t["left"][node] if go else t["right"][node]
            s = np.float32(s + t["value"][~node])
        out[i] = s
    return out


# ---- leaf-wise growth (gbdt_ref.grow_tree with the rules above)
def grow_tree(bins, qg, qh, expo, edges, nbins, nan_bin, max_bin, num_leaves, lr=0.1, l2=0.0, min_data=1, min_hess=1e-3, min_gain=0.0, max_depth=-1,
              fault=None):
    """-> (tree dict of feature / threshold / left / right / value / default_left / split_bin / missing (the node's missing rows in its
    feature), the leaves' row lists, the smallest margin of any search)."""
    n = bins.shape[0]
    none = {"gain": -np.inf, "runner_up": -np.inf}

    def splittable(count, depth):
        return count >= 2 * max(min_data, 1) and not (max_depth > 0 and depth >= max_depth)

    def search(hist):
        return best_split(hist, nbins, nan_bin, expo, l2, min_data, min_hess, min_gain, fault)

    all_rows = np.arange(n, dtype=np.int32)
    tot = (int(qg.astype(np.int64).sum()), int(qh.astype(np.int64).sum()))
    root_hist = R.histogram(bins, qg, qh, all_rows, max_bin)
    leaves = [{"rows": all_rows, "depth": 0, "parent": -1, "side": 0, "sums": tot, "hist": root_hist,
               "split": search(root_hist) if splittable(n, 0) else none}]
    worst = margin(leaves[0]["split"])
    feature, threshold, left, right, go_left, split_bin, missing = [], [], [], [], [], [], []
    while len(leaves) < num_leaves:
        li = max(range(len(leaves)), key=lambda i: (leaves[i]["split"]["gain"], -i))
        leaf = leaves[li]
        s = leaf["split"]
        if not s["gain"] > -np.inf:
            break
        out, cl = partition(bins, leaf["rows"], s["feature"], s["bin"], also_left(s, nan_bin))
        assert cl == s["left"][2] or fault is not None
        node = len(feature)
        feature.append(s["feature"]); threshold.append(edges[s["feature"], s["bin"]]); left.append(~li); right.append(~len(leaves))
        go_left.append(s["default_left"]); split_bin.append(s["bin"]); missing.append(s["missing"])
        if leaf["parent"] >= 0:
            (left if leaf["side"] == 0 else right)[leaf["parent"]] = node
        kids = [{"rows": rows, "depth": leaf["depth"] + 1, "parent": node, "side": side, "sums": sums[:2], "hist": None, "split": none}
                for side, rows, sums in ((0, out[:cl], s["left"]), (1, out[cl:], s["right"]))]
        can = [splittable(c["rows"].size, c["depth"]) for c in kids]
        if len(leaves) + 1 < num_leaves and any(can):
            small, large = (kids[0], kids[1]) if kids[0]["rows"].size <= kids[1]["rows"].size else (kids[1], kids[0])
            small["hist"] = R.histogram(bins, qg, qh, small["rows"], max_bin)
            large["hist"] = leaf["hist"] - small["hist"]
            for c, ok in zip(kids, can):
                if ok:
                    c["split"] = search(c["hist"])
                    worst = min(worst, margin(c["split"]))
        leaf["hist"] = None
        leaves[li] = kids[0]
        leaves.append(kids[1])
    value = np.array([R.leaf_value(c["sums"][0], c["sums"][1], expo, l2, lr) for c in leaves], np.float32)
    tree = {"feature": np.array(feature, np.int32), "threshold": np.array(threshold, np.float32), "left": np.array(left, np.int32),
            "right": np.array(right, np.int32), "value": value, "default_left": np.array(go_left, np.uint8),
            "split_bin": np.array(split_bin, np.int32), "missing": np.array(missing, np.int64)}
    return tree, [c["rows"] for c in leaves], worst


# ---- the fixture
def load(path=None):
    """{case: gbdt_sk.load's dict with NaNs in X and fresh, plus nan (bool [n, F]), fresh_nan, fresh_compared (bool [m]: the rows whose
    walk meets no undecided node with a NaN in its feature), nodes [K, 5] per round}, and the sklearn version."""
    out = {}
    with np.load(path or FILE, allow_pickle=False) as z:
        version = str(z["sklearn_version"])
        for name in sorted({k.split("/")[0] for k in z.files if "/" in k}):
            g = lambda k: z[f"{name}/{k}"]
            p = dict(zip(PARAM_NAMES, g("params").tolist()))
            for k in PARAM_NAMES:
                if k not in ("learning_rate", "lambda_l2"):
                    p[k] = int(p[k])
            nan, fresh_nan = g("nan").astype(bool), g("fresh_nan").astype(bool)
            X = np.where(nan, np.float32(np.nan), g("codes").astype(np.float32) / np.float32(8.0)).astype(np.float32)
            fresh = np.where(fresh_nan, np.float32(np.nan), g("fresh16").astype(np.float32) / np.float32(16.0)).astype(np.float32)
            offs = g("tree_offsets")
            nodes, leaves = g("nodes"), g("leaves")
            out[name] = dict(X=X, codes=g("codes"), nan=nan, y=g("y64").astype(np.float32) / np.float32(64.0),
                             w=g("w16").astype(np.float32) / np.float32(16.0) if f"{name}/w16" in z.files else None, params=p,
                             baseline=float(g("baseline")), staged=g("staged"), fresh=fresh, fresh_nan=fresh_nan,
                             fresh_pred=g("fresh_pred"), fresh_compared=g("fresh_compared").astype(bool),
                             nodes=[nodes[offs[r, 0]:offs[r + 1, 0]] for r in range(p["rounds"])],
                             leaves=[leaves[offs[r, 1]:offs[r + 1, 1]] for r in range(p["rounds"])])
    return out, version


def booster_params(p, depthwise=False):
    """The fixture's parameters under the booster's names."""
    out = dict(SK.booster_params(p), use_missing=True)
    if depthwise:
        out["grow_policy"] = "depthwise"
    return out


def sort_nodes(a):
    """Canonical nodes [K, 5] = (feature, threshold, rows, missing_go_to_left, missing rows) sorted by feature, threshold, rows, missing
    rows, and the direction last (it may be undecided)."""
    a = np.asarray(a, np.float64).reshape(-1, 5)
    return a[np.lexsort((a[:, 3], a[:, 4], a[:, 2], a[:, 1], a[:, 0]))] if a.shape[0] else a


def canonical_node(X, rows, f, threshold, go_left, feature_has_nan):
    """One canonical node (feature, fp32 threshold, rows, missing_go_to_left, missing rows) from the training rows under it and the
    node as its implementation wrote it -> (the node, bool [rows]: which of them go left).  Two kinds of node have several spellings
    for ONE partition of their rows, between which sklearn's choice is rounding noise (it scans the bins once upwards with the missing
    rows right and once downwards with them left, its float sums differ in the last bits, and the first strictly larger gain wins):
      - the NaNs against every value: "every value left, NaNs right" at any edge above the node's largest value, or mirrored, "NaNs left" at
        any edge below its smallest value.  Written here as (feature, +inf, rows, 0, missing rows);
      - a node without missing rows in a feature that has NaNs elsewhere: the upward scan keeps the lowest edge of an empty stretch, the
        downward one the highest.  Written here with the lowest such edge: the midpoint between the largest value that goes left and the
        feature's next distinct training value.  (Its direction is undecided too and is not compared.)"""
    x = X[rows, f]
    miss = np.isnan(x)
    mc = int(miss.sum())
    left = np.where(miss, bool(go_left), x <= threshold)
    if mc > 0 and (np.array_equal(left, miss) or np.array_equal(left, ~miss)):
        return (float(f), np.inf, float(rows.size), 0.0, float(mc)), left
    if mc == 0 and feature_has_nan[f] and left.any() and not left.all():
        col = X[:, f]
        lo = x[left].max()
        hi = col[col > lo].min()
        mid = np.float32((np.float64(lo) + np.float64(hi)) * 0.5)
        threshold = lo if mid >= hi else mid
    return (float(f), float(np.float32(threshold)), float(rows.size), float(bool(go_left)), float(mc)), left


def canonical(tree, X):
    """(nodes [K, 5], leaves [L, 2]) of one of this project's trees: the training rows X are walked through it on the raw features, left on
    x <= threshold, a NaN along default_left; every node through canonical_node."""
    X = np.asarray(X, np.float32)
    k = tree["feature"].size
    at = {0: np.arange(X.shape[0])}
    leaf_rows = np.zeros(tree["value"].size, np.int64)
    has_nan = np.isnan(X).any(axis=0)
    nodes = []
    if k == 0:
        leaf_rows[0] = X.shape[0]
    for i in range(k):
        rows = at.pop(i)
        node, go_left = canonical_node(X, rows, int(tree["feature"][i]), tree["threshold"][i], tree["default_left"][i], has_nan)
        nodes.append(node)
        for child, part in ((int(tree["left"][i]), rows[go_left]), (int(tree["right"][i]), rows[~go_left])):
            if child >= 0:
                assert child > i
                at[child] = part
            else:
                leaf_rows[~child] = part.size
    leaves = np.stack([tree["value"].astype(np.float64), leaf_rows.astype(np.float64)], axis=1)
    return sort_nodes(nodes), SK.sort_rows(leaves)


def gate(ref):
    return C_GBDT_SK_MISSING * SK.need_unit(ref)


def decided(nodes, feature_has_nan):
    """bool [K]: the node's direction is decided by the rules: it holds missing rows in its feature, or its feature has no training NaN."""
    return (nodes[:, 4] > 0) | ~np.asarray(feature_has_nan)[nodes[:, 0].astype(np.int64)]


def tree_mismatch(got_nodes, got_leaves, case, r):
    """None when a canonical tree equals round r of the fixture (nodes, their missing rows and the leaf row counts exactly, the direction
    where it is decided, leaf values within the gate of that round's scores), else a word on what differs."""
    nodes, leaves = case["nodes"][r], case["leaves"][r]
    if got_nodes.shape != nodes.shape or not np.array_equal(got_nodes[:, :3], nodes[:, :3]):
        return "internal nodes"
    if not np.array_equal(got_nodes[:, 4], nodes[:, 4]):
        return "missing rows under the nodes"
    d = decided(nodes, case["nan"].any(axis=0))
    if not np.array_equal(got_nodes[d, 3], nodes[d, 3]):
        return "missing_go_to_left"
    if got_leaves.shape != leaves.shape or not np.array_equal(got_leaves[:, 1], leaves[:, 1]):
        return "leaf row counts"
    if not (np.abs(got_leaves[:, 0] - leaves[:, 0]) <= gate(case["staged"][r])).all():
        return "leaf values"
    return None


def run_restatement(case, fault=None):
    """The restatement driven round by round from the fixture's baseline -> (per round (tree, training scores fp32), fresh predictions fp32
    with the baseline added, the smallest margin of any split search)."""
    p, X, y, w = case["params"], case["X"], case["y"], case["w"]
    edges, nbins, nan_bin = bin_edges(X, p["max_bin"])
    bins = bin_matrix(X, edges, nbins, nan_bin)
    base = np.float32(case["baseline"])
    scores = np.full(X.shape[0], base, np.float32)
    rounds, worst = [], np.inf
    for _ in range(p["rounds"]):
        g, h = SK.gradients(scores, y, w)
        qg, qh, expo, flag = R.quantize(g, h)
        assert flag == 0
        tree, leaf_rows, m = grow_tree(bins, qg, qh, expo, edges, nbins, nan_bin, p["max_bin"], p["num_leaves"], p["learning_rate"], p["lambda_l2"],
                                       p["min_data_in_leaf"], 1e-3, 0.0, p["max_depth"], fault=fault)
        worst = min(worst, m)
        scores = R.add_leaf_values(scores.copy(), leaf_rows, tree["value"])
        rounds.append((tree, scores))
    fresh = (predict(case["fresh"], [t for t, _ in rounds]) + base).astype(np.float32)
    return rounds, fresh, worst


def compare_restatement(case, fault=None):
    """-> (the first mismatch as a string or None, the worst need of the predictions, the worst need of the leaf values, the margin)."""
    rounds, fresh, worst = run_restatement(case, fault)
    need = leaf_need = 0.0
    bad = None
    for r, (tree, scores) in enumerate(rounds):
        nodes, leaves = canonical(tree, case["X"])
        miss = tree_mismatch(nodes, leaves, case, r)
        if miss is not None:
            return f"round {r}: {miss}", need, leaf_need, worst
        unit = SK.need_unit(case["staged"][r])
        leaf_need = max(leaf_need, float(np.abs(leaves[:, 0] - case["leaves"][r][:, 0]).max()) / unit)
        need = max(need, float(np.abs(scores.astype(np.float64) - case["staged"][r]).max()) / unit)
        if need > C_GBDT_SK_MISSING and bad is None:
            bad = f"round {r}: training scores need {need:.2f}"
    keep = case["fresh_compared"]
    n_fresh = float(np.abs(fresh.astype(np.float64) - case["fresh_pred"])[keep].max()) / SK.need_unit(case["fresh_pred"])
    need = max(need, n_fresh)
    if n_fresh > C_GBDT_SK_MISSING and bad is None:
        bad = f"fresh rows need {n_fresh:.2f}"
    return bad, need, leaf_need, worst
