"""Plain-numpy restatement of DEPTH-WISE growth (grow_policy='depthwise' of ptranking_amd/gbdt.py), built from gbdt_ref's histogram,
best_split, partition and leaf_value; and the loader of the depth fixture (tests/golden/gbdt_sklearn_depth.npz, written by
tests/golden/make_golden_gbdt_sklearn_depth.py).  Test infrastructure, never imported by the package.

The policy: the leaves made at the previous level are the frontier; a leaf is a candidate when it is splittable and its search found a
split; with more candidates than the leaf budget the largest gains are kept (ties: the smaller start, that is row order) and the others
stay leaves for good; all kept candidates are split together, numbered in ascending start.  The left child inherits the parent's leaf index,
the right child is appended.  A sibling pair gets histograms only if the tree can still grow and a child is splittable: the child with
fewer rows (ties: the left) is summed from its rows, the other is parent minus child.

`fault` plants one wrong rule: "cap_smallest" keeps the smallest gains at the cap; "neighbour_split" partitions a segment with its
neighbour's (feature, bin); "larger_hist" exchanges the two children's histograms; "refused_frontier" keeps a leaf that was refused at the
cap in the next frontier."""
import os

import numpy as np

import gbdt_ref as R
import gbdt_sk as SK

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gbdt_sklearn_depth.npz")
FAULTS = ("cap_smallest", "neighbour_split", "larger_hist", "refused_frontier")


def grow_tree(bins, qg, qh, expo, edges, nbins, max_bin, num_leaves, lr=0.1, l2=0.0, min_data=1, min_hess=1e-3, min_gain=0.0, max_depth=-1,
              fault=None):
    """-> (tree dict of feature / threshold / left / right / value, the leaves' row lists by leaf index, the smallest margin of any search,
    levels: per level dict(candidates=[(gain, start)], kept=[(gain, start)], searched=number of children searched))."""
    n = bins.shape[0]
    none = {"gain": -np.inf, "runner_up": -np.inf}

    def splittable(count, depth):
        return count >= 2 * max(min_data, 1) and not (max_depth > 0 and depth >= max_depth)

    def search(hist):
        return R.best_split(hist, nbins, expo, l2, min_data, min_hess, min_gain)

    all_rows = np.arange(n, dtype=np.int32)
    root_hist = R.histogram(bins, qg, qh, all_rows, max_bin)
    root = {"leaf": 0, "start": 0, "rows": all_rows, "depth": 0, "parent": -1, "side": 0, "hist": root_hist,
            "sums": (int(qg.astype(np.int64).sum()), int(qh.astype(np.int64).sum())), "split": search(root_hist) if splittable(n, 0) else none}
    worst = R.margin(root["split"])
    leaves = [root]                                    # by leaf index
    frontier = [root]                                  # ascending start
    feature, threshold, left, right, levels = [], [], [], [], []
    while True:
        cands = [c for c in frontier if splittable(c["rows"].size, c["depth"]) and c["split"]["gain"] > -np.inf]
        budget = num_leaves - len(leaves)
        if not cands or budget <= 0:
            break
        kept, refused = cands, []
        if len(cands) > budget:
            sign = 1.0 if fault == "cap_smallest" else -1.0
            ranked = sorted(cands, key=lambda c: (sign * c["split"]["gain"], c["start"]))
            kept, refused = sorted(ranked[:budget], key=lambda c: c["start"]), ranked[budget:]
        levels.append({"candidates": [(c["split"]["gain"], c["start"]) for c in cands], "kept": [(c["split"]["gain"], c["start"]) for c in kept],
                       "searched": 0})
        made = []
        for i, c in enumerate(kept):
            s = c["split"]
            how = kept[(i + 1) % len(kept)]["split"] if fault == "neighbour_split" else s
            out, cl = R.partition(bins, c["rows"], how["feature"], how["bin"])
            assert cl == s["left"][2] or fault in ("neighbour_split", "larger_hist")
            node = len(feature)
            feature.append(s["feature"]); threshold.append(edges[s["feature"], s["bin"]]); left.append(~c["leaf"]); right.append(~len(leaves))
            if c["parent"] >= 0:
                (left if c["side"] == 0 else right)[c["parent"]] = node
            kids = [{"leaf": li, "start": st, "rows": rows, "depth": c["depth"] + 1, "parent": node, "side": sd, "hist": None, "sums": sums[:2],
                     "split": none}
                    for li, st, rows, sd, sums in ((c["leaf"], c["start"], out[:cl], 0, s["left"]), (len(leaves), c["start"] + cl, out[cl:], 1, s["right"]))]
            leaves[c["leaf"]] = kids[0]
            leaves.append(kids[1])
            made.append((c, kids))
        for c, kids in made:                            # after ALL of the level's splits: whether the tree can still grow is a fact of the level
            can = [splittable(k["rows"].size, k["depth"]) for k in kids]
            if len(leaves) < num_leaves and any(can):
                small, large = (kids[0], kids[1]) if kids[0]["rows"].size <= kids[1]["rows"].size else (kids[1], kids[0])
                small["hist"] = R.histogram(bins, qg, qh, small["rows"], max_bin)
                large["hist"] = c["hist"] - small["hist"]
                if fault == "larger_hist":
                    small["hist"], large["hist"] = large["hist"], small["hist"]
                for k, ok in zip(kids, can):
                    if ok:
                        k["split"] = search(k["hist"])
                        worst = min(worst, R.margin(k["split"]))
                        levels[-1]["searched"] += 1
            c["hist"] = None
        frontier = [k for _, kids in made for k in kids]
        if fault == "refused_frontier":
            frontier = sorted(frontier + refused, key=lambda c: c["start"])
    value = np.array([R.leaf_value(c["sums"][0], c["sums"][1], expo, l2, lr) for c in leaves], np.float32)
    tree = {"feature": np.array(feature, np.int32), "threshold": np.array(threshold, np.float32), "left": np.array(left, np.int32),
            "right": np.array(right, np.int32), "value": value}
    return tree, [c["rows"] for c in leaves], worst, levels


def load(path=None):
    """The depth fixture's cases, as gbdt_sk.load gives the leaf-wise ones."""
    return SK.load(path or FILE)


def run_restatement(case, policy="depthwise", fault=None):
    """gbdt_sk.run_restatement under a growth policy -> (per round (tree, training scores fp32), fresh predictions fp32 with the baseline
    added, the smallest margin of any split search)."""
    if policy == "leafwise":
        return SK.run_restatement(case, fault)
    p, X, y, w = case["params"], case["X"], case["y"], case["w"]
    edges, nbins = R.bin_edges(X, p["max_bin"])
    bins = R.bin_matrix(X, edges, nbins)
    base = np.float32(case["baseline"])
    scores = np.full(X.shape[0], base, np.float32)
    rounds, worst = [], np.inf
    for _ in range(p["rounds"]):
        g, h = SK.gradients(scores, y, w)
        qg, qh, expo, flag = R.quantize(g, h)
        assert flag == 0
        tree, leaf_rows, margin, _ = grow_tree(bins, qg, qh, expo, edges, nbins, p["max_bin"], p["num_leaves"], p["learning_rate"], p["lambda_l2"],
                                               p["min_data_in_leaf"], 1e-3, 0.0, p["max_depth"], fault=fault)
        worst = min(worst, margin)
        scores = R.add_leaf_values(scores.copy(), leaf_rows, tree["value"])
        rounds.append((tree, scores))
    fresh = (R.predict(case["fresh"], [t for t, _ in rounds]) + base).astype(np.float32)
    return rounds, fresh, worst


def compare_restatement(case, fault=None):
    """gbdt_sk.compare_restatement for the depth-wise restatement -> (the first mismatch or None, the worst need of the predictions, of the
    leaf values, the margin)."""
    rounds, fresh, worst = run_restatement(case, "depthwise", fault)
    need = leaf_need = 0.0
    bad = None
    for r, (tree, scores) in enumerate(rounds):
        nodes, leaves = SK.canonical(tree, case["X"])
        miss = SK.tree_mismatch(nodes, leaves, case, r)
        if miss is not None:
            return f"round {r}: {miss}", need, leaf_need, worst
        unit = SK.need_unit(case["staged"][r])
        leaf_need = max(leaf_need, float(np.abs(leaves[:, 0] - case["leaves"][r][:, 0]).max()) / unit)
        need = max(need, float(np.abs(scores.astype(np.float64) - case["staged"][r]).max()) / unit)
        if need > SK.C_GBDT_SK and bad is None:
            bad = f"round {r}: training scores need {need:.2f}"
    n_fresh = float(np.abs(fresh.astype(np.float64) - case["fresh_pred"]).max()) / SK.need_unit(case["fresh_pred"])
    need = max(need, n_fresh)
    if n_fresh > SK.C_GBDT_SK and bad is None:
        bad = f"fresh rows need {n_fresh:.2f}"
    return bad, need, leaf_need, worst


def same_trees(a, b, X):
    """Whether two runs (lists of (tree, scores)) agree: the trees in canonical form with bit-equal fp32 leaf values, and bit-equal scores."""
    if len(a) != len(b):
        return False
    for (ta, sa), (tb, sb) in zip(a, b):
        na, la = SK.canonical(ta, X)
        nb, lb = SK.canonical(tb, X)
        if na.shape != nb.shape or la.shape != lb.shape or not np.array_equal(na, nb) or not np.array_equal(la, lb):
            return False
        if not np.array_equal(np.asarray(sa, np.float32).view(np.int32), np.asarray(sb, np.float32).view(np.int32)):
            return False
    return True
