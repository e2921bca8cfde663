"""Plain-numpy restatement of the monotone and interaction constraints of the gradient-boosted trees (monotone_constraints and
interaction_constraints of ptranking_amd/gbdt.py; the *_cst entry points of ptranking_amd/csrc/gbdt.hip), on top of gbdt_ref.py,
gbdt_missing_ref.py and gbdt_cat_ref.py.  Test infrastructure, never imported by the package; it needs neither a GPU nor scikit-learn.

The rules (include/ptranking_amd.h states them; scikit-learn's splitting.pyx / grower.py wherever those are deterministic).  Every node
keeps (lo, hi, v) in float64; root: lo = -inf, hi = +inf, v = -G / (H + l2).  Under active monotone constraints EVERY candidate of EVERY
search (numeric, the missing-value candidates, categorical sets, features of constraint 0, nodes of infinite bounds) takes the bounded gain:
    1. vL = min(max(-GL / (HL + l2), lo), hi), vR likewise;
    2. rejected if the feature's constraint is +1 and vL > vR, or -1 and vL < vR (a categorical feature has none);
    3. gain = ((G * v) - (GL * vL)) - (GR * vR), float64 in that order;
    4. validity (min_data, the Hessian floor), min_gain, ties and the record are those of the unconstrained scans.
A child takes its clamped vL / vR as v; with mid = (vL + vR) / 2 the bounds are [lo, hi] for both under constraint 0, left [lo, mid] and
right [mid, hi] under +1, left [mid, hi] and right [lo, mid] under -1.  A leaf stores float32(v * learning_rate).
Interaction constraints: the groups, plus one group of the features in none; root: all groups active, all features allowed; a child of a
split on f keeps the active groups that contain f and may split on their union only.  With interaction constraints alone the gain is the
unconstrained one, bit for bit.

`fault` arguments plant one wrong rule each: "no_clamp" (values are never clamped), "mid_unclamped" (mid from the unclamped values),
"swapped_neg" (under -1 the children get the bounds of +1), "inherit_all_groups" (a child keeps every group of its parent)."""
import os

import numpy as np

import gbdt_cat_ref as CR
import gbdt_missing_ref as MR
import gbdt_ref as R
import gbdt_sk as SK

FAULTS = ("no_clamp", "mid_unclamped", "swapped_neg", "inherit_all_groups")
FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gbdt_sklearn_cst.npz")
PARAM_NAMES = CR.PARAM_NAMES
CAT_SMOOTH = CR.CAT_SMOOTH

# The gate, as gbdt_sk's: |got - sklearn| <= C_GBDT_SK_CST * 2^-24 * max(1, max |sklearn's scores of that round|).  Twice the worst need of
# the RESTATEMENT against sklearn over every round and every fresh row of the fixture (test_gbdt_cst_cpu.py re-measures it and prints it),
# rounded up to an integer; never taken from the kernels' output.
C_GBDT_SK_CST = 4
NEED_RECORDED = 1.94                      # case d

NONE = {"gain": -np.inf, "feature": -1, "cat": False, "bin": -1, "default_left": 0, "set": 0, "left": (0, 0, 0), "right": (0, 0, 0),
        "runner_up": -np.inf, "gap": np.inf, "changed": False, "vl": 0.0, "vr": 0.0}


# ---- the bounded gain
def node_value(g_sum, h_sum, expo, l2):
    """-G / (H + l2) in float64 from the integer sums (0 where H + l2 is not positive)."""
    G, H = np.ldexp(np.float64(int(g_sum)), -int(expo[0])), np.ldexp(np.float64(int(h_sum)), -int(expo[1]))
    den = H + np.float64(l2)
    with np.errstate(all="ignore"):
        return -G / den if den > 0.0 else np.float64(0.0)


def child_values(lsum, tot, expo, l2, lo, hi, clamp=True):
    """(vL, vR, GL, GR): the children's values, clamped to [lo, hi] (min(max(x, lo), hi)) unless clamp is False."""
    eg, eh = int(expo[0]), int(expo[1])
    GL, HL = np.ldexp(np.float64(int(lsum[0])), -eg), np.ldexp(np.float64(int(lsum[1])), -eh)
    GR, HR = np.ldexp(np.float64(int(tot[0]) - int(lsum[0])), -eg), np.ldexp(np.float64(int(tot[1]) - int(lsum[1])), -eh)
    l2 = np.float64(l2)
    with np.errstate(all="ignore"):
        xl, xr = -GL / (HL + l2), -GR / (HR + l2)
    if clamp:
        xl, xr = np.minimum(np.maximum(xl, lo), hi), np.minimum(np.maximum(xr, lo), hi)
    return np.float64(xl), np.float64(xr), GL, GR


def bounded_gain(lsum, tot, expo, l2, cst, sign, fault=None):
    """-> (gain or None where the order test rejects the candidate, vL, vR, the gain without the order test)."""
    lo, hi, v = (np.float64(c) for c in cst)
    vl, vr, GL, GR = child_values(lsum, tot, expo, l2, lo, hi, clamp=fault != "no_clamp")
    G = np.ldexp(np.float64(int(tot[0])), -int(expo[0]))
    with np.errstate(all="ignore"):
        gain = ((G * v) - (GL * vl)) - (GR * vr)
    rejected = (sign > 0 and vl > vr) or (sign < 0 and vl < vr)
    return (None if rejected else float(gain)), float(vl), float(vr), float(gain)


def child_cst(cst, sign, vl, vr, lsum, tot, expo, l2, fault=None):
    """(lo, hi, v) of the left and the right child of a split whose clamped values are vl, vr."""
    lo, hi = np.float64(cst[0]), np.float64(cst[1])
    a, b = np.float64(vl), np.float64(vr)
    if fault == "mid_unclamped":
        a, b = child_values(lsum, tot, expo, l2, lo, hi, clamp=False)[:2]
    mid = (a + b) / np.float64(2.0)
    if fault == "swapped_neg" and sign < 0:
        sign = 1
    if sign > 0:
        return (lo, mid, np.float64(vl)), (mid, hi, np.float64(vr))
    if sign < 0:
        return (mid, hi, np.float64(vl)), (lo, mid, np.float64(vr))
    return (lo, hi, np.float64(vl)), (lo, hi, np.float64(vr))


# ---- groups
def all_groups(groups, nf):
    """The groups as sets, the features in no group as one more group."""
    groups = [frozenset(int(c) for c in g) for g in groups]
    rest = frozenset(range(nf)) - frozenset().union(*groups) if groups else frozenset()
    return groups + ([rest] if rest else [])


def allowed_mask(groups, active, nf):
    m = np.zeros(nf, bool)
    for g in active:
        m[list(groups[g])] = True
    return m


# ---- the split scan
def best_split(hist, nbins, nan_bin, is_cat, expo, l2=0.0, min_data=1, min_hess=1e-3, min_gain=0.0, cat_smooth=CAT_SMOOTH, mono=None, cst=None,
               allowed=None, fault=None):
    """gbdt_cat_ref.best_split under the constraints.  mono int [F] with cst = (lo, hi, v): the bounded gain on every candidate (cst None: the
    unconstrained gain); allowed bool [F] or None.  -> its dict plus vl, vr (the winner's clamped child values under cst), changed (the
    winner differs from the one the same search finds without the order test: a rejection decided), gap (also the smallest relative
    distance of an order test from equality, where the two values differ)."""
    hist = np.asarray(hist, np.int64)
    nf, mb, _ = hist.shape
    nbins, is_cat = np.asarray(nbins), np.asarray(is_cat, bool)
    nb_arr = np.full(nf, -1, np.int64) if nan_bin is None else np.asarray(nan_bin)
    bounded = cst is not None
    if bounded and (not (cst[0] <= cst[1]) or cst[2] != cst[2]):
        return dict(NONE)
    mg = -np.inf if bounded else min_gain                                # the bounded gain replaces the gain: validity alone is taken from below
    gain, left, tot, mc = MR.candidates(hist, nbins, nb_arr, expo, l2, min_data, min_hess, mg)
    gain = np.where(is_cat[:, None, None], -np.inf, gain)
    cands = []                                                           # (gain, feature, key, left sums, cat, set)
    fs, bs, ds = np.nonzero(gain > -np.inf)
    for f, b, d in zip(fs.tolist(), bs.tolist(), ds.tolist()):
        cands.append((float(gain[f, b, d]), f, b if d == 0 else 511 - b, tuple(int(v) for v in left[f, b, d]), False, 0))
    gap = np.inf
    for f in np.nonzero(is_cat)[0].tolist():
        cc, g = CR.cat_candidates(hist[f], int(min(max(nbins[f], 1), mb)), int(nb_arr[f]), tot, expo, l2, min_data, min_hess, mg, cat_smooth)
        if allowed is None or allowed[f]:
            gap = min(gap, g)
        cands.extend((gn, f, key, lsum, True, bits) for gn, key, lsum, bits in cc)
    if allowed is not None:
        cands = [c for c in cands if allowed[c[1]]]
    values, free = {}, []
    if bounded:
        kept = []
        for c in cands:
            sign = 0 if c[4] else int(mono[c[1]]) if mono is not None and -1 <= int(mono[c[1]]) <= 1 else 0
            gn, vl, vr, raw = bounded_gain(c[3], tot, expo, l2, cst, sign, fault)
            if sign != 0 and vl != vr:
                gap = min(gap, abs(vl - vr) / max(abs(vl), abs(vr), 1e-300))
            if raw >= min_gain:
                free.append((raw,) + c[1:])
            if gn is not None and gn >= min_gain:
                kept.append((gn,) + c[1:])
                values[c[1:4]] = (vl, vr)
        cands = kept
    if not cands:
        return dict(NONE, gap=gap)
    order = lambda c: (-c[0], c[1], c[2])
    gn, f, key, lsum, cat, bits = min(cands, key=order)
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
    vl, vr = values.get((f, key, lsum), (0.0, 0.0))
    return {"gain": gn, "feature": f, "cat": cat, "bin": b, "default_left": default_left, "set": bits, "left": lsum, "right": comp,
            "runner_up": max(rest) if rest else -np.inf, "gap": gap, "changed": bool(free) and min(free, key=order)[1:4] != (f, key, lsum),
            "vl": vl, "vr": vr}


record = CR.record
margin = CR.margin


# ---- leaf-wise growth (gbdt_cat_ref.grow_tree with the rules above)
def grow_tree(bins, qg, qh, expo, edges, nbins, nan_bin, is_cat, max_bin, num_leaves, lr=0.1, l2=0.0, min_data=1, min_hess=1e-3, min_gain=0.0,
              max_depth=-1, cat_smooth=CAT_SMOOTH, mono=None, groups=None, fault=None):
    """mono: int [F] or None (all zeros counts as None); groups: a list of feature groups or None.  -> (tree dict as gbdt_cat_ref.grow_tree's,
    the leaves' row lists, the smallest margin of any search, stats dict(changed: searches a rejection decided, clamped: leaves whose v is
    not -G / (H + l2), paths: the set of features on each leaf's path))."""
    n, nf = bins.shape[0], np.asarray(nbins).size
    none = dict(NONE)
    mono = None if mono is None or not np.any(mono) else np.asarray(mono, np.int64)
    groups = all_groups(groups, nf) if groups else None

    def splittable(count, depth):
        return count >= 2 * max(min_data, 1) and not (max_depth > 0 and depth >= max_depth)

    def search(hist, cst, active):
        return best_split(hist, nbins, nan_bin, is_cat, expo, l2, min_data, min_hess, min_gain, cat_smooth, mono, cst if mono is not None else None,
                          allowed_mask(groups, active, nf) if groups is not None else None, fault)

    all_rows = np.arange(n, dtype=np.int32)
    tot = (int(qg.astype(np.int64).sum()), int(qh.astype(np.int64).sum()))
    root_hist = R.histogram(bins, qg, qh, all_rows, max_bin)
    root_cst = (np.float64(-np.inf), np.float64(np.inf), node_value(tot[0], tot[1], expo, l2))
    root_active = tuple(range(len(groups))) if groups is not None else ()
    leaves = [{"rows": all_rows, "depth": 0, "parent": -1, "side": 0, "sums": tot, "hist": root_hist, "cst": root_cst, "active": root_active,
               "path": frozenset(), "split": search(root_hist, root_cst, root_active) if splittable(n, 0) else none}]
    worst = margin(leaves[0]["split"])
    changed = int(leaves[0]["split"]["changed"])
    feature, threshold, left, right, go_left, split_bin, cat_index, cat_set = [], [], [], [], [], [], [], []
    while len(leaves) < num_leaves:
        li = max(range(len(leaves)), key=lambda i: (leaves[i]["split"]["gain"], -i))
        leaf = leaves[li]
        s = leaf["split"]
        if not s["gain"] > -np.inf:
            break
        out, cl = CR.partition(bins, leaf["rows"], s, nan_bin)
        assert cl == s["left"][2]
        node = len(feature)
        f = s["feature"]
        feature.append(f); left.append(~li); right.append(~len(leaves)); go_left.append(s["default_left"])
        threshold.append(np.float32(0.0) if s["cat"] else edges[f, s["bin"]])
        split_bin.append(0 if s["cat"] else s["bin"])
        cat_index.append(len(cat_set) if s["cat"] else -1)
        if s["cat"]:
            cat_set.append(CR.set_words(s["set"]))
        if leaf["parent"] >= 0:
            (left if leaf["side"] == 0 else right)[leaf["parent"]] = node
        if mono is not None:
            node_tot = tuple(a + b for a, b in zip(s["left"], s["right"]))
            kid_cst = child_cst(leaf["cst"], 0 if s["cat"] else int(mono[f]), s["vl"], s["vr"], s["left"], node_tot, expo, l2, fault)
        else:
            kid_cst = (None, None)
        active = leaf["active"]
        if groups is not None and fault != "inherit_all_groups":
            active = tuple(g for g in active if f in groups[g])
        kids = [{"rows": rows, "depth": leaf["depth"] + 1, "parent": node, "side": side, "sums": sums[:2], "hist": None, "split": none,
                 "cst": kid_cst[side], "active": active, "path": leaf["path"] | {f}}
                for side, rows, sums in ((0, out[:cl], s["left"]), (1, out[cl:], s["right"]))]
        can = [splittable(c["rows"].size, c["depth"]) for c in kids]
        if len(leaves) + 1 < num_leaves and any(can):
            small, large = (kids[0], kids[1]) if kids[0]["rows"].size <= kids[1]["rows"].size else (kids[1], kids[0])
            small["hist"] = R.histogram(bins, qg, qh, small["rows"], max_bin)
            large["hist"] = leaf["hist"] - small["hist"]
            for c, ok in zip(kids, can):
                if ok:
                    c["split"] = search(c["hist"], c["cst"], c["active"])
                    worst = min(worst, margin(c["split"]))
                    changed += int(c["split"]["changed"])
        leaf["hist"] = None
        leaves[li] = kids[0]
        leaves.append(kids[1])
    clamped = 0
    if mono is not None and len(leaves) > 1:
        value = np.array([np.float32(c["cst"][2] * np.float64(lr)) for c in leaves], np.float32)
        clamped = sum(int(c["cst"][2] != node_value(c["sums"][0], c["sums"][1], expo, l2)) for c in leaves)
    else:
        value = np.array([R.leaf_value(c["sums"][0], c["sums"][1], expo, l2, lr) for c in leaves], np.float32)
    tree = {"feature": np.array(feature, np.int32), "threshold": np.array(threshold, np.float32), "left": np.array(left, np.int32),
            "right": np.array(right, np.int32), "value": value, "cat_index": np.array(cat_index, np.int32),
            "cat_set": np.array(cat_set, np.int64).reshape(-1, 4), "split_bin": np.array(split_bin, np.int32)}
    if nan_bin is not None:
        tree["default_left"] = np.array(go_left, np.uint8)
    return tree, [c["rows"] for c in leaves], worst, {"changed": changed, "clamped": clamped, "paths": [c["path"] for c in leaves]}


def tree_paths(tree):
    """The set of features on every root-to-leaf path of a tree dict (feature / left / right)."""
    out = []

    def walk(node, seen):
        if node < 0:
            out.append(seen)
            return
        seen = seen | {int(tree["feature"][node])}
        walk(int(tree["left"][node]), seen)
        walk(int(tree["right"][node]), seen)
    walk(0 if tree["feature"].size else ~0, frozenset())
    return out


def forbidden_pairs(paths, groups, nf):
    """The (a, b) on one path that share no group."""
    gs = all_groups(groups, nf)
    return sorted({(a, b) for p in paths for a in p for b in p if a < b and not any(a in g and b in g for g in gs)})


# ---- the fixture
def load(path=None):
    """gbdt_cat_ref.load's cases, each with mono int8 [F], groups (a list of lists, [] for none) and, where stored, sweep fp32 [S, F],
    sweep_feature [S], sweep_block [S], sweep_pred (scikit-learn under the constraints) and sweep_free (without) float64 [S]."""
    cases, version = CR.load(path or FILE)
    with np.load(path or FILE, allow_pickle=False) as z:
        for name, case in cases.items():
            case["mono"] = z[f"{name}/mono"].astype(np.int8)
            case["groups"] = [np.nonzero(row)[0].tolist() for row in z[f"{name}/groups"]]
            if f"{name}/sweep16" in z.files:
                sw = z[f"{name}/sweep16"].astype(np.float32) / np.float32(16.0)
                sw[z[f"{name}/sweep_nan"].astype(bool)] = np.nan
                case.update(sweep=sw, sweep_feature=z[f"{name}/sweep_feature"], sweep_block=z[f"{name}/sweep_block"],
                            sweep_pred=z[f"{name}/sweep_pred"], sweep_free=z[f"{name}/sweep_free"])
    return cases, version


def booster_params(case):
    """The fixture's parameters under the booster's names."""
    p = case["params"]
    out = dict(SK.booster_params(p))
    if p["ncat"]:
        out.update(categorical_feature=list(range(p["ncat"])), cat_smooth=CAT_SMOOTH)
    if p["use_missing"]:
        out["use_missing"] = True
    if p["depthwise"]:
        out["grow_policy"] = "depthwise"
    if np.any(case["mono"]):
        out["monotone_constraints"] = case["mono"].tolist()
    if case["groups"]:
        out["interaction_constraints"] = [list(g) for g in case["groups"]]
    return out


def canonical(tree, X, nbins):
    """gbdt_cat_ref.canonical; a tree of a booster without categorical features has no cat_index and gets one of -1."""
    if "cat_index" not in tree:
        tree = dict(tree, cat_index=np.full(tree["feature"].size, -1, np.int32), cat_set=np.zeros((0, 4), np.int64))
    return CR.canonical(tree, X, nbins)


def gate(ref):
    return C_GBDT_SK_CST * SK.need_unit(ref)


def tree_mismatch(got_nodes, got_leaves, case, r):
    """gbdt_cat_ref.tree_mismatch under this fixture's gate."""
    miss = CR.tree_mismatch(got_nodes, got_leaves, dict(case, staged=np.full_like(case["staged"], np.inf)), r)
    if miss is None and not (np.abs(got_leaves[:, 0] - case["leaves"][r][:, 0]) <= gate(case["staged"][r])).all():
        return "leaf values"
    return miss


def setup(case):
    return CR.setup(case)


def run_restatement(case, fault=None, mono="case", groups="case"):
    """The restatement driven round by round from the fixture's baseline -> (per round (tree, training scores fp32), fresh predictions fp32
    with the baseline added, the smallest margin of any split search, the per-round stats).  mono / groups: 'case' or an override (None:
    that constraint off)."""
    p, X, y, w = case["params"], case["X"], case["y"], case["w"]
    edges, nbins, nan_bin, is_cat, bins = setup(case)
    mono = case["mono"] if isinstance(mono, str) else mono
    groups = case["groups"] if isinstance(groups, str) else groups
    base = np.float32(case["baseline"])
    scores = np.full(X.shape[0], base, np.float32)
    rounds, worst, stats = [], np.inf, []
    for _ in range(p["rounds"]):
        g, h = SK.gradients(scores, y, w)
        qg, qh, expo, flag = R.quantize(g, h)
        assert flag == 0
        tree, leaf_rows, m, st = grow_tree(bins, qg, qh, expo, edges, nbins, nan_bin, is_cat, p["max_bin"], p["num_leaves"], p["learning_rate"],
                                           p["lambda_l2"], p["min_data_in_leaf"], 1e-3, 0.0, p["max_depth"], CAT_SMOOTH, mono, groups or None, fault)
        worst = min(worst, m)
        scores = R.add_leaf_values(scores.copy(), leaf_rows, tree["value"])
        rounds.append((tree, scores))
        stats.append(st)
    fresh = (CR.predict(case["fresh"], [t for t, _ in rounds]) + base).astype(np.float32)
    return rounds, fresh, worst, stats


def compare_restatement(case, fault=None):
    """-> (the first mismatch as a string or None, the worst need of the predictions, the worst need of the leaf values, the margin)."""
    rounds, fresh, worst, _ = run_restatement(case, fault)
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
        if need > C_GBDT_SK_CST and bad is None:
            bad = f"round {r}: training scores need {need:.2f}"
    n_fresh = float(np.abs(fresh.astype(np.float64) - case["fresh_pred"]).max()) / SK.need_unit(case["fresh_pred"])
    need = max(need, n_fresh)
    if n_fresh > C_GBDT_SK_CST and bad is None:
        bad = f"fresh rows need {n_fresh:.2f}"
    return bad, need, leaf_need, worst
