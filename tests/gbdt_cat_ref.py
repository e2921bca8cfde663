"""Plain-numpy restatement of the categorical-feature rules of the gradient-boosted trees (categorical_feature of ptranking_amd/gbdt.py; the
*_cat entry points of ptranking_amd/csrc/gbdt.hip), on top of gbdt_ref.py and gbdt_missing_ref.py.  Test infrastructure, never imported by
the package; it needs neither a GPU nor scikit-learn.

The rule (include/ptranking_amd.h states it; scikit-learn's _find_best_bin_to_split_category wherever that is deterministic).  A
categorical column holds integer codes; code c is bin c and nbins[f] is the largest code plus 1.  For such a feature at a node with
totals (TG, TH, TC), the NaN bin included:
    1. the categories are the value bins 0 .. nbins[f] - 1 and, where nan_bin[f] >= 0, the NaN bin; G_c, H_c = ldexp(qsum, -e), exact;
    2. a category is USED iff it holds a row and H_c * (TC / TH) >= cat_smooth (float64, in that order), and its key is a number;
    3. its key is v_c = G_c / (H_c + cat_smooth);
    4. with u used categories, u <= 1 gives no split on the feature; else they are sorted ascending by v, equal keys by the lower bin;
    5. left to right the first i + 1 sorted categories go left, i = 0 .. (u + 1) // 2 - 1; right to left the last i + 1, i = 0 ..
       (u + 1) // 2 - 2; unused categories and empty bins always go right;
    6. validity and gain are the numeric scan's (gbdt_ref.gains): min_data, the Hessian floor, min_gain, the uncontracted float64 gain;
    7. ties: the highest gain, the lowest feature, left-to-right before right-to-left, then fewer categories on the left;
    8. a record's field 2 is the number of left categories + 256 * default_left, default_left being the NaN bin's bit in the left set.
Numeric features are searched by gbdt_missing_ref.candidates (which is gbdt_ref.gains where no feature has a NaN bin).

`fault` arguments plant one wrong rule each: "wrong_middle" (both scans stop one candidate early: u // 2 in place of (u + 1) // 2),
"unused_left" (the categories that hold rows but fail the support test go left with the set), "nan_ignored" (the NaN bin is no category),
"support_no_factor" (the support test without TC / TH)."""
import os

import numpy as np

import gbdt_missing_ref as MR
import gbdt_ref as R
import gbdt_sk as SK

FAULTS = ("wrong_middle", "unused_left", "nan_ignored", "support_no_factor")
FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gbdt_sklearn_cat.npz")
PARAM_NAMES = MR.PARAM_NAMES + ("ncat", "use_missing")
CAT_SMOOTH = 10.0                       # scikit-learn's MIN_CAT_SUPPORT

# The gate, as gbdt_sk's: |got - sklearn| <= C_GBDT_SK_CAT * 2^-24 * max(1, max |sklearn's scores of that round|).  Twice the worst need of
# the RESTATEMENT against sklearn over every round and every fresh row of the fixture (test_gbdt_cat_cpu.py re-measures it and prints it),
# rounded up to an integer; never taken from the kernels' output.
C_GBDT_SK_CAT = 4
NEED_RECORDED = 1.66                      # case b, its training scores


# ---- binning
def bin_edges(X, max_bin, categorical=(), use_missing=False):
    """-> (edges, nbins, nan_bin): gbdt_missing_ref.bin_edges (gbdt_ref's without NaNs) for the numeric columns; a categorical column gets
    the edges 0.5, 1.5, ... and nbins = the largest code + 1, its NaN bin (under use_missing, where it holds a NaN) behind them."""
    X = np.asarray(X, np.float32)
    assert use_missing or not np.isnan(X).any()
    edges, nbins, nan_bin = MR.bin_edges(X, max_bin)
    for f in categorical:
        col = X[:, f]
        miss = np.isnan(col)
        codes = col[~miss]
        assert (codes == np.floor(codes)).all() and (codes >= 0).all() and (codes <= max_bin - (2 if miss.any() else 1)).all()
        top = int(codes.max()) if codes.size else 0
        edges[f] = np.inf
        edges[f, :top] = np.arange(top, dtype=np.float32) + np.float32(0.5)
        nbins[f] = top + 1
        nan_bin[f] = nbins[f] if miss.any() else -1
    return edges, nbins, nan_bin


# ---- the split scan
def set_words(bits):
    """A left set (python int, bit b = bin b) as the device's 4 int64."""
    return np.array([(bits >> (64 * w)) & (2 ** 64 - 1) for w in range(4)], np.uint64).view(np.int64)


def set_bits(words):
    w = np.asarray(words, np.int64).view(np.uint64)
    return sum(int(w[k]) << (64 * k) for k in range(4))


def cat_candidates(hf, nb, mbin, tot, expo, l2, min_data, min_hess, min_gain, cat_smooth, fault=None):
    """The candidates of one categorical feature from its histogram hf [max_bin, 3] -> (list of (gain, key, left sums (3 ints), left set
    as a python int), the smallest relative gap of the screen: adjacent sort keys from each other, support values from cat_smooth)."""
    mb = hf.shape[0]
    cats = list(range(nb)) + ([mbin] if (nb <= mbin < mb and fault != "nan_ignored") else [])
    TG, TH, TC = (int(v) for v in tot)
    H = np.ldexp(np.float64(TH), -expo[1])
    with np.errstate(all="ignore"):
        factor = np.float64(1.0) if fault == "support_no_factor" else np.float64(TC) / H
        used, gap, low = [], np.inf, 0
        for c in cats:
            g, h, cnt = (int(v) for v in hf[c])
            Gc, Hc = np.ldexp(np.float64(g), -expo[0]), np.ldexp(np.float64(h), -expo[1])
            v = Gc / (Hc + np.float64(cat_smooth))
            if cnt > 0 and cat_smooth > 0 and factor != 1.0:            # with unit Hessians both sides of the test are exact integers: not screened
                gap = min(gap, abs(float(Hc * factor) - cat_smooth) / cat_smooth)
            if cnt > 0 and Hc * factor >= cat_smooth and v == v:
                used.append((float(v), c))
            elif cnt > 0 and fault == "unused_left":
                low |= 1 << c
    u = len(used)
    if u <= 1:
        return [], gap
    used.sort()                                                          # by the key, then the lower bin
    for (a, _), (b, _) in zip(used[:-1], used[1:]):
        gap = min(gap, abs(b - a) / max(abs(a), abs(b), 1e-300))
    mid = u // 2 if fault == "wrong_middle" else (u + 1) // 2
    G, Hn = np.ldexp(np.float64(TG), -expo[0]), H
    with np.errstate(all="ignore"):
        parent = (G * G) / (Hn + l2)
    floor_h = max(min_hess, 2.0 ** -40)
    out = []
    for rtl, count in ((0, mid), (1, mid - 1)):
        order = used[::-1] if rtl else used
        left, bits = np.zeros(3, np.int64), low
        for i in range(count):
            left = left + hf[order[i][1]]
            bits |= 1 << order[i][1]
            gl, hl, cl = (int(v) for v in left)
            if cl < min_data or TC - cl < min_data:
                continue
            GL, HL = np.ldexp(np.float64(gl), -expo[0]), np.ldexp(np.float64(hl), -expo[1])
            GR, HR = np.ldexp(np.float64(TG - gl), -expo[0]), np.ldexp(np.float64(TH - hl), -expo[1])
            if not HL >= floor_h or not HR >= floor_h:
                continue
            gain = ((GL * GL) / (HL + l2) + (GR * GR) / (HR + l2)) - parent
            if gain >= min_gain:
                out.append((float(gain), 256 * rtl + i, (gl, hl, cl), bits))
    return out, gap


def best_split(hist, nbins, nan_bin, is_cat, expo, l2=0.0, min_data=1, min_hess=1e-3, min_gain=0.0, cat_smooth=CAT_SMOOTH, fault=None):
    """-> dict(gain, feature, cat (bool), bin (numeric) or the number of left categories, default_left, set (python int), left, right,
    runner_up, gap).  nan_bin: None without missing values (a numeric record's field 2 is then the bin alone).  runner_up: the best gain
    among the candidates that give another partition of the node's sums; gap: the screen's smallest relative gap of a key or a support
    test over the categorical features."""
    hist = np.asarray(hist, np.int64)
    nf, mb, _ = hist.shape
    nbins, is_cat = np.asarray(nbins), np.asarray(is_cat, bool)
    nb_arr = np.full(nf, -1, np.int64) if nan_bin is None else np.asarray(nan_bin)
    gain, left, tot, mc = MR.candidates(hist, nbins, nb_arr, expo, l2, min_data, min_hess, min_gain)
    gain = np.where(is_cat[:, None, None], -np.inf, gain)
    cands = []                                                           # (gain, feature, key, left sums, cat, set)
    fs, bs, ds = np.nonzero(gain > -np.inf)
    for f, b, d in zip(fs.tolist(), bs.tolist(), ds.tolist()):
        cands.append((float(gain[f, b, d]), f, b if d == 0 else 511 - b, tuple(int(v) for v in left[f, b, d]), False, 0))
    gap = np.inf
    for f in np.nonzero(is_cat)[0].tolist():
        cc, g = cat_candidates(hist[f], int(min(max(nbins[f], 1), mb)), int(nb_arr[f]), tot, expo, l2, min_data, min_hess, min_gain, cat_smooth, fault)
        gap = min(gap, g)
        cands.extend((gn, f, key, lsum, True, bits) for gn, key, lsum, bits in cc)
    if not cands:
        return {"gain": -np.inf, "feature": -1, "cat": False, "bin": -1, "default_left": 0, "set": 0, "left": (0, 0, 0), "right": (0, 0, 0),
                "runner_up": -np.inf, "gap": gap}
    gn, f, key, lsum, cat, bits = min(cands, key=lambda c: (-c[0], c[1], c[2]))
    tt = tuple(int(v) for v in tot)
    comp = tuple(t - v for t, v in zip(tt, lsum))
    rest = [c[0] for c in cands if c[3] != lsum and c[3] != comp]
    if cat:
        mbin = int(nb_arr[f])
        default_left = int(mbin >= 0 and (bits >> mbin) & 1)
        b = (key & 255) + 1
    else:
        b = key if key < 256 else 511 - key
        default_left = 0
        if nan_bin is not None:
            default_left = int(key >= 256) if mc[f] > 0 else int(lsum[2] > tt[2] - lsum[2])
    return {"gain": gn, "feature": f, "cat": cat, "bin": b, "default_left": default_left, "set": bits, "left": lsum, "right": comp,
            "runner_up": max(rest) if rest else -np.inf, "gap": gap}


def record(split, missing):
    """(the 9 int64 of the device's record, the 4 int64 of its left set)."""
    field = -1 if split["feature"] < 0 else split["bin"] + (256 * split["default_left"] if (missing or split["cat"]) else 0)
    return (np.array([np.float64(split["gain"]).view(np.int64), split["feature"], field, *split["left"], *split["right"]], np.int64),
            set_words(split["set"] if split["cat"] else 0))


def margin(split):
    """The screen's figure of one search: the relative distance of the best gain from the runner-up, and the smallest key or support gap."""
    return min(R.margin(split), split["gap"])


# ---- routing
def goes_left(bins_col, split, nan_bin):
    """bool per binned value of the split feature."""
    v = bins_col.astype(np.int64)
    if split["cat"]:
        return np.array([(split["set"] >> int(b)) & 1 for b in v], bool)
    also = int(nan_bin[split["feature"]]) if (nan_bin is not None and split["default_left"]) else -1
    return (v <= split["bin"]) | (v == also)


def partition(bins, rows, split, nan_bin):
    rows = np.asarray(rows, np.int32)
    left = goes_left(bins[rows, split["feature"]], split, nan_bin)
    return np.concatenate([rows[left], rows[~left]]).astype(np.int32), int(left.sum())


def node_goes_left(x, tree, node):
    """One raw value at one node of a tree dict (cat_index / cat_set / default_left optional), as ptr_gbdt_predict_cat decides."""
    dl = bool(tree["default_left"][node]) if "default_left" in tree else False
    ci = int(tree["cat_index"][node]) if "cat_index" in tree else -1
    if ci >= 0:
        if np.isnan(x):
            return dl
        if not (0.0 <= x <= 255.0) or x != np.floor(x):
            return False
        return bool((set_bits(tree["cat_set"][ci]) >> int(x)) & 1)
    return dl if (np.isnan(x) and "default_left" in tree) else bool(x <= tree["threshold"][node])


def predict(X, trees):
    """fp32 sum of the leaf values in tree order."""
    X = np.asarray(X, np.float32)
    out = np.zeros(X.shape[0], np.float32)
    for i in range(X.shape[0]):
        s = np.float32(0.0)
        for t in trees:
            node = 0 if t["feature"].size else ~0
            while node >= 0:
                node = t["left"][node] if node_goes_left(X[i, t["feature"][node]], t, node) else t["right"][node]
            s = np.float32(s + t["value"][~node])
        out[i] = s
    return out


# ---- leaf-wise growth (gbdt_ref.grow_tree with the rules above)
def grow_tree(bins, qg, qh, expo, edges, nbins, nan_bin, is_cat, max_bin, num_leaves, lr=0.1, l2=0.0, min_data=1, min_hess=1e-3, min_gain=0.0,
              max_depth=-1, cat_smooth=CAT_SMOOTH, fault=None):
    """-> (tree dict of feature / threshold / left / right / value / cat_index / cat_set / split_bin (and default_left where nan_bin is not
    None), the leaves' row lists, the smallest margin of any search)."""
    n = bins.shape[0]
    none = {"gain": -np.inf, "runner_up": -np.inf, "gap": np.inf}

    def splittable(count, depth):
        return count >= 2 * max(min_data, 1) and not (max_depth > 0 and depth >= max_depth)

    def search(hist):
        return best_split(hist, nbins, nan_bin, is_cat, expo, l2, min_data, min_hess, min_gain, cat_smooth, fault)

    all_rows = np.arange(n, dtype=np.int32)
    tot = (int(qg.astype(np.int64).sum()), int(qh.astype(np.int64).sum()))
    root_hist = R.histogram(bins, qg, qh, all_rows, max_bin)
    leaves = [{"rows": all_rows, "depth": 0, "parent": -1, "side": 0, "sums": tot, "hist": root_hist,
               "split": search(root_hist) if splittable(n, 0) else none}]
    worst = margin(leaves[0]["split"])
    feature, threshold, left, right, go_left, split_bin, cat_index, cat_set = [], [], [], [], [], [], [], []
    while len(leaves) < num_leaves:
        li = max(range(len(leaves)), key=lambda i: (leaves[i]["split"]["gain"], -i))
        leaf = leaves[li]
        s = leaf["split"]
        if not s["gain"] > -np.inf:
            break
        out, cl = partition(bins, leaf["rows"], s, nan_bin)
        assert cl == s["left"][2] or fault is not None
        node = len(feature)
        feature.append(s["feature"]); left.append(~li); right.append(~len(leaves)); go_left.append(s["default_left"])
        threshold.append(np.float32(0.0) if s["cat"] else edges[s["feature"], s["bin"]])
        split_bin.append(0 if s["cat"] else s["bin"])
        cat_index.append(len(cat_set) if s["cat"] else -1)
        if s["cat"]:
            cat_set.append(set_words(s["set"]))
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
            "right": np.array(right, np.int32), "value": value, "cat_index": np.array(cat_index, np.int32),
            "cat_set": np.array(cat_set, np.int64).reshape(-1, 4), "split_bin": np.array(split_bin, np.int32)}
    if nan_bin is not None:
        tree["default_left"] = np.array(go_left, np.uint8)
    return tree, [c["rows"] for c in leaves], worst


# ---- the fixture
def load(path=None):
    """{case: dict(X fp32 [n, F] (the leading ncat columns hold codes, NaN where <c>/nan is set; the others codes / 8), y, w or None,
    params, baseline, nodes / leaves per round (canonical), staged, fresh fp32 [m, F], fresh_pred)}, and the sklearn version."""
    out = {}
    with np.load(path or FILE, allow_pickle=False) as z:
        version = str(z["sklearn_version"])
        for name in sorted({k.split("/")[0] for k in z.files if "/" in k}):
            g = lambda k: z[f"{name}/{k}"]
            p = dict(zip(PARAM_NAMES, g("params").tolist()))
            for k in PARAM_NAMES:
                if k not in ("learning_rate", "lambda_l2"):
                    p[k] = int(p[k])
            codes, nan = g("codes"), g("nan").astype(bool)
            X = codes.astype(np.float32) / np.float32(8.0)
            X[:, :p["ncat"]] = codes[:, :p["ncat"]]
            X[nan] = np.nan
            fresh = g("fresh16").astype(np.float32) / np.float32(16.0)
            fresh[g("fresh_nan").astype(bool)] = np.nan
            offs = g("tree_offsets")
            nodes, leaves = g("nodes"), g("leaves")
            out[name] = dict(X=X, nan=nan, y=g("y64").astype(np.float32) / np.float32(64.0),
                             w=g("w16").astype(np.float32) / np.float32(16.0) if f"{name}/w16" in z.files else None, params=p,
                             baseline=float(g("baseline")), staged=g("staged"), fresh=fresh, fresh_pred=g("fresh_pred"),
                             nodes=[nodes[offs[r, 0]:offs[r + 1, 0]] for r in range(p["rounds"])],
                             leaves=[leaves[offs[r, 1]:offs[r + 1, 1]] for r in range(p["rounds"])])
    return out, version


def booster_params(p):
    """The fixture's parameters under the booster's names."""
    out = dict(SK.booster_params(p), categorical_feature=list(range(p["ncat"])), cat_smooth=CAT_SMOOTH)
    if p["use_missing"]:
        out["use_missing"] = True
    if p["depthwise"]:
        out["grow_policy"] = "depthwise"
    return out


NODE_COLS = 13      # feature, categorical, fp32 threshold (0 at a categorical node), rows, missing_go_to_left, the left codes as 8 uint32


def node_row(f, cat, threshold, rows, go_left, bits):
    """One canonical node.  bits: the left CODES as a python int (the NaN bin's bit is not among them: go_left carries it)."""
    return [float(f), float(cat), 0.0 if cat else float(np.float32(threshold)), float(rows), float(bool(go_left))] + \
           [float((bits >> (32 * k)) & 0xffffffff) for k in range(8)]


def canonical(tree, X, nbins):
    """(nodes [K, NODE_COLS], leaves [L, 2]) of one of this project's trees: the training rows X are walked through it on the raw features."""
    X = np.asarray(X, np.float32)
    k = tree["feature"].size
    at = {0: np.arange(X.shape[0])}
    leaf_rows = np.zeros(tree["value"].size, np.int64)
    nodes = []
    if k == 0:
        leaf_rows[0] = X.shape[0]
    for i in range(k):
        rows = at.pop(i)
        f, ci = int(tree["feature"][i]), int(tree["cat_index"][i])
        go = np.array([node_goes_left(x, tree, i) for x in X[rows, f]], bool)
        bits = set_bits(tree["cat_set"][ci]) & ((1 << int(nbins[f])) - 1) if ci >= 0 else 0
        nodes.append(node_row(f, ci >= 0, tree["threshold"][i], rows.size, tree["default_left"][i] if "default_left" in tree else 0, bits))
        for child, part in ((int(tree["left"][i]), rows[go]), (int(tree["right"][i]), rows[~go])):
            if child >= 0:
                assert child > i
                at[child] = part
            else:
                leaf_rows[~child] = part.size
    leaves = np.stack([tree["value"].astype(np.float64), leaf_rows.astype(np.float64)], axis=1)
    return sort_nodes(nodes), SK.sort_rows(leaves)


def sort_nodes(a):
    """Canonical nodes sorted by every column but the direction, which comes last (it is compared only where it is decided)."""
    a = np.asarray(a, np.float64).reshape(-1, NODE_COLS)
    keys = [a[:, 4]] + [a[:, c] for c in range(NODE_COLS - 1, 4, -1)] + [a[:, 3], a[:, 2], a[:, 1], a[:, 0]]
    return a[np.lexsort(keys)] if a.shape[0] else a


def gate(ref):
    return C_GBDT_SK_CAT * SK.need_unit(ref)


def tree_mismatch(got_nodes, got_leaves, case, r):
    """None when a canonical tree equals round r of the fixture: the nodes' feature, kind, threshold, rows and left codes and the leaves' row
    counts exactly; missing_go_to_left at the categorical nodes of a feature that holds NaNs in training (elsewhere scikit-learn sends a
    NaN to the larger child, a rule for inputs the fixture does not hold); the leaf values within the gate of that round's scores."""
    nodes, leaves = case["nodes"][r], case["leaves"][r]
    cols = [0, 1, 2, 3] + list(range(5, NODE_COLS))
    if got_nodes.shape != nodes.shape or not np.array_equal(got_nodes[:, cols[:4]], nodes[:, cols[:4]]):
        return "internal nodes"
    if not np.array_equal(got_nodes[:, 5:], nodes[:, 5:]):
        return "left sets"
    d = (nodes[:, 1] > 0) & case["nan"].any(axis=0)[nodes[:, 0].astype(np.int64)]
    if not np.array_equal(got_nodes[d, 4], nodes[d, 4]):
        return "missing_go_to_left"
    if got_leaves.shape != leaves.shape or not np.array_equal(got_leaves[:, 1], leaves[:, 1]):
        return "leaf row counts"
    if not (np.abs(got_leaves[:, 0] - leaves[:, 0]) <= gate(case["staged"][r])).all():
        return "leaf values"
    return None


def setup(case):
    """(edges, nbins, nan_bin or None, is_cat, bins) of a case."""
    p, X = case["params"], case["X"]
    cats = tuple(range(p["ncat"]))
    edges, nbins, nan_bin = bin_edges(X, p["max_bin"], cats, bool(p["use_missing"]))
    bins = MR.bin_matrix(X, edges, nbins, nan_bin)
    is_cat = np.zeros(X.shape[1], bool)
    is_cat[list(cats)] = True
    return edges, nbins, (nan_bin if p["use_missing"] else None), is_cat, bins


def run_restatement(case, fault=None):
    """The restatement driven round by round from the fixture's baseline -> (per round (tree, training scores fp32), fresh predictions fp32
    with the baseline added, the smallest margin of any split search)."""
    p, X, y, w = case["params"], case["X"], case["y"], case["w"]
    edges, nbins, nan_bin, is_cat, bins = setup(case)
    base = np.float32(case["baseline"])
    scores = np.full(X.shape[0], base, np.float32)
    rounds, worst = [], np.inf
    for _ in range(p["rounds"]):
        g, h = SK.gradients(scores, y, w)
        qg, qh, expo, flag = R.quantize(g, h)
        assert flag == 0
        tree, leaf_rows, m = grow_tree(bins, qg, qh, expo, edges, nbins, nan_bin, is_cat, p["max_bin"], p["num_leaves"], p["learning_rate"], p["lambda_l2"],
                                       p["min_data_in_leaf"], 1e-3, 0.0, p["max_depth"], CAT_SMOOTH, fault=fault)
        worst = min(worst, m)
        scores = R.add_leaf_values(scores.copy(), leaf_rows, tree["value"])
        rounds.append((tree, scores))
    fresh = (predict(case["fresh"], [t for t, _ in rounds]) + base).astype(np.float32)
    return rounds, fresh, worst


def compare_restatement(case, fault=None):
    """-> (the first mismatch as a string or None, the worst need of the predictions, the worst need of the leaf values, the margin)."""
    rounds, fresh, worst = run_restatement(case, fault)
    nbins = setup(case)[1]
    need = leaf_need = 0.0
    bad = None
    for r, (tree, scores) in enumerate(rounds):
        nodes, leaves = canonical(tree, case["X"], nbins)
        miss = tree_mismatch(nodes, leaves, case, r)
        if miss is not None:
            return f"round {r}: {miss}", need, leaf_need, worst
        unit = SK.need_unit(case["staged"][r])
        leaf_need = max(leaf_need, float(np.abs(leaves[:, 0] - case["leaves"][r][:, 0]).max()) / unit)
        need = max(need, float(np.abs(scores.astype(np.float64) - case["staged"][r]).max()) / unit)
        if need > C_GBDT_SK_CAT and bad is None:
            bad = f"round {r}: training scores need {need:.2f}"
    n_fresh = float(np.abs(fresh.astype(np.float64) - case["fresh_pred"]).max()) / SK.need_unit(case["fresh_pred"])
    need = max(need, n_fresh)
    if n_fresh > C_GBDT_SK_CAT and bad is None:
        bad = f"fresh rows need {n_fresh:.2f}"
    return bad, need, leaf_need, worst
