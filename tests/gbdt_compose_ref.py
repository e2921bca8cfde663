"""Plain-numpy restatement of GBDT.update (ptranking_amd/gbdt.py) under EVERY option at once: row sampling, quantized gradients with and
without renewed leaves, missing values, categorical splits, monotone and interaction constraints, DART's tree rate and linear leaves.  It
composes the restatements each option arrived with (gbdt_ref, gbdt_sample_ref, gbdt_quant_ref, gbdt_missing_ref, gbdt_cat_ref,
gbdt_cst_ref, gbdt_dart_ref, gbdt_linear_ref) by the rules include/ptranking_amd.h states; it copies no product code.  Test
infrastructure, never imported by the package; it needs no GPU.

Depth-wise growth has no second grower here: the composed cases keep num_leaves >= 2^max_depth, where the leaf cap cannot bind and a
depth-wise fit is the leaf-wise fit of the same max_depth up to the numbering of nodes and leaves; such trees are compared in canonical
form (canonical below: gbdt_cat_ref.canonical).

`fault` arguments plant one wrong composition each: "quant_ignores_bag" (the tree grows on the bag, the renewed leaf values are summed over
every row that walks to the leaf), "renew_plain_lr" (the renewed values use learning_rate where DART's tree rate applies),
"cat_row0_set" (a searched right child takes the left set found for its left sibling), "stale_default_left" (a node on a feature without a
NaN bin keeps the direction of the node before it), "groups_after_cat" (a categorical split does not narrow the active groups)."""
import numpy as np

import gbdt_cat_ref as CR
import gbdt_cst_ref as CS
import gbdt_dart_ref as D
import gbdt_linear_ref as L
import gbdt_quant_ref as Q
import gbdt_ref as R
import gbdt_sample_ref as S

FAULTS = ("quant_ignores_bag", "renew_plain_lr", "cat_row0_set", "stale_default_left", "groups_after_cat")
GROWER_FAULTS = ("cat_row0_set", "groups_after_cat")               # planted inside gbdt_cst_ref.grow_tree
TREE_KEYS = ("feature", "left", "right", "threshold", "value", "default_left", "cat_index", "cat_set")
DEFAULTS = {"learning_rate": 0.1, "lambda_l2": 0.0, "min_data_in_leaf": 20, "min_sum_hessian_in_leaf": 1e-3, "min_gain_to_split": 0.0, "max_depth": -1,
            "cat_smooth": 10.0, "linear_lambda": 0.0}


def option(p, key):
    return p.get(key, DEFAULTS[key])


def quantized(p):
    return bool(p.get("use_quantized_grad", False))


def renewed(p):
    return quantized(p) and bool(p.get("quant_train_renew_leaf", False))


# ---- the walks
def bin_goes_left(tree, node, b, nan_bin):
    """One binned value at one node: a categorical node sends the bins of its left set left (a NaN bin is one more category, its bit is
    default_left); a numeric node the bins <= its split bin and, under default_left, its feature's NaN bin."""
    ci = int(tree["cat_index"][node])
    if ci >= 0:
        return bool((CR.set_bits(tree["cat_set"][ci]) >> int(b)) & 1)
    f = int(tree["feature"][node])
    also = int(nan_bin[f]) if (nan_bin is not None and "default_left" in tree and tree["default_left"][node]) else -1
    return int(b) <= int(tree["split_bin"][node]) or int(b) == also


def leaf_of_bins(bins, tree, nan_bin):
    """The leaf of every binned row -> int64 [n]."""
    out = np.zeros(bins.shape[0], np.int64)
    for i in range(bins.shape[0]):
        node = 0 if tree["feature"].size else ~0
        while node >= 0:
            node = int(tree["left"][node] if bin_goes_left(tree, node, bins[i, tree["feature"][node]], nan_bin) else tree["right"][node])
        out[i] = ~node
    return out


def raw_goes_left(tree, node, x):
    """One raw value at one node: a NaN goes along default_left (right in a tree that keeps none); at a categorical node a code of the left
    set goes left and anything else (an unseen code, a value that is no code) right; at a numeric node x <= threshold goes left."""
    if np.isnan(x):
        return bool(tree["default_left"][node]) if "default_left" in tree else False
    ci = int(tree["cat_index"][node]) if "cat_index" in tree else -1
    if ci < 0:
        return bool(np.float32(x) <= np.float32(tree["threshold"][node]))
    if x != np.floor(x) or x < 0.0 or x > 255.0:
        return False
    return bool((CR.set_bits(tree["cat_set"][ci]) >> int(x)) & 1)


def leaf_of_rows(X, tree):
    X = np.asarray(X, np.float32)
    out = np.zeros(X.shape[0], np.int64)
    for i in range(X.shape[0]):
        node = 0 if tree["feature"].size else ~0
        while node >= 0:
            node = int(tree["left"][node] if raw_goes_left(tree, node, X[i, tree["feature"][node]]) else tree["right"][node])
        out[i] = ~node
    return out


def tree_outputs(X, tree):
    """One tree's output for every raw row, float32: value[leaf], or under linear leaves gbdt_linear_ref.leaf_output rounded once."""
    leaf = leaf_of_rows(X, tree)
    if "leaf_features" not in tree:
        return np.asarray(tree["value"], np.float32)[leaf]
    X = np.asarray(X, np.float32)
    return np.array([L.leaf_output(x, tree["value"][l], tree["leaf_features"][l], tree["leaf_coeff"][l], tree["leaf_const"][l]) for x, l in zip(X, leaf)],
                    np.float64).astype(np.float32)


def predict(X, trees):
    """Fresh rows (NaNs, category codes no left set holds, values on edges) -> the fp32 sum of the trees' outputs in tree order."""
    out = np.zeros(np.asarray(X).shape[0], np.float32)
    for t in trees:
        out = (out + tree_outputs(X, t)).astype(np.float32)
    return out


# ---- one tree
def grow(X, bins, g, h, edges, nbins, nan_bin, is_cat, params, t, qid=None, lr=None, fault=None):
    """Tree t (from 0) of GBDT.update -> (tree, mask or None, add: every row's leaf value by the binned walk (under linear_tree: its leaf
    output on the raw row), the smallest split margin, stats).  nan_bin: None without use_missing; is_cat: bool [F]; lr: the tree's rate
    where it is not learning_rate (DART's lr / (1 + k)).
    GOSS's warm-up counts floor(1 / learning_rate) trees with the PARAMETER learning_rate under DART too: GBDT._sample reads
    params['learning_rate'], not the tree rate, and gbdt_sample_ref.tree_mask is handed the same dict.
    stats: gbdt_cst_ref.grow_tree's (changed, clamped, paths) plus cat_nodes, default_left (the nodes' directions), oob (rows outside the
    bag), leaf_rows (row indices per leaf, the bag's alone) and, under linear_tree, linear: per leaf (A, b, P, status, pivot ratio)."""
    p = params
    rate = option(p, "learning_rate")
    lr = rate if lr is None else lr
    l2 = option(p, "lambda_l2")
    g2, h2, mask = S.tree_mask(p, t, np.asarray(g, np.float32), np.asarray(h, np.float32), qid)
    if quantized(p):
        qg, qh, expo, flag = Q.quantize_low(g2, h2, p.get("num_grad_quant_bins", 4), p.get("stochastic_rounding", True), p.get("quant_seed", 0), t)
    else:
        qg, qh, expo, flag = R.quantize(g2, h2)
    assert flag == 0
    n = bins.shape[0]
    bag = np.arange(n) if mask is None else np.nonzero(mask)[0]
    mono = np.asarray(p["monotone_constraints"], np.int64) if np.any(p.get("monotone_constraints", ())) else None
    groups = [list(gr) for gr in p.get("interaction_constraints", ())] or None
    tree, leaf_rows, margin, stats = CS.grow_tree(bins[bag], qg[bag], qh[bag], expo, edges, nbins, nan_bin, np.asarray(is_cat, bool), p["max_bin"],
                                                  p["num_leaves"], lr, l2, option(p, "min_data_in_leaf"), option(p, "min_sum_hessian_in_leaf"),
                                                  option(p, "min_gain_to_split"), option(p, "max_depth"), option(p, "cat_smooth"), mono, groups,
                                                  fault if fault in GROWER_FAULTS else None, exact_ties=True)
    leaf_rows = [bag[rows] for rows in leaf_rows]
    if fault == "stale_default_left" and nan_bin is not None:
        for k in range(1, tree["feature"].size):
            if nan_bin[tree["feature"][k]] < 0:
                tree["default_left"][k] = tree["default_left"][k - 1]
    leaf = leaf_of_bins(bins, tree, nan_bin)
    if fault not in GROWER_FAULTS:                                        # in the bag the walk gives each row the leaf the growth put it in
        for l, rows in enumerate(leaf_rows):
            assert (leaf[rows] == l).all()
        assert sum(rows.size for rows in leaf_rows) == bag.size
    if renewed(p):                                                        # the 30-bit pair over each leaf's bag rows, at the tree's rate
        g30, h30, e30, _ = R.quantize(g2, h2)
        over = [np.nonzero(leaf == l)[0] for l in range(len(leaf_rows))] if fault == "quant_ignores_bag" else leaf_rows
        at = rate if fault == "renew_plain_lr" else lr
        tree["value"] = np.array([R.leaf_value(int(g30[rows].astype(np.int64).sum()), int(h30[rows].astype(np.int64).sum()), e30, l2, at) for rows in over],
                                 np.float32)
    stats = dict(stats, cat_nodes=int((tree["cat_index"] >= 0).sum()), default_left=tree["default_left"].tolist() if "default_left" in tree else [],
                 oob=n - bag.size, leaf_rows=leaf_rows)
    if p.get("linear_tree", False):
        nl = tree["value"].size
        tree["leaf_features"], tree["leaf_coeff"], tree["leaf_const"] = np.full((nl, L.K), -1, np.int32), np.zeros((nl, L.K)), np.zeros(nl)
        stats["linear"] = []
        for l, P in enumerate(L.path_features(tree)):
            A, b, m_u = (np.asarray(a, np.float64) for a in L.moments(X, leaf_rows[l], P, g2, h2, np.longdouble)[:3])     # summed in extended precision,
            c, status, ratio = L.solve(A, b, len(P), int(m_u), option(p, "linear_lambda"))                                # rounded once (test_gbdt_linear_gpu.py)
            if status == 0:
                tree["leaf_features"][l, :len(P)], tree["leaf_coeff"][l, :len(P)], tree["leaf_const"][l] = P, c[:-1] * lr, c[-1] * lr
            stats["linear"].append((A, b, P, status, ratio))
        add = tree_outputs(X, tree)
    else:
        add = np.asarray(tree["value"], np.float32)[leaf]
    return tree, mask, add, margin, stats


# ---- whole fits
def squared_error(y):
    y = np.asarray(y, np.float32)
    return lambda r, scores: (scores - y).astype(np.float32)


def selection(case):
    """DART: gbdt_dart_ref.replay_selection of the case's rounds -> [(dropped, tree rate, factor)]; None under 'gbdt'."""
    p = case["params"]
    if case.get("boosting", "gbdt") != "dart":
        return None
    return D.replay_selection(case["rounds"], option(p, "learning_rate"), p.get("drop_rate", 0.1), p.get("max_drop", 50), p.get("skip_drop", 0.5),
                              p.get("uniform_drop", False), p.get("drop_seed", 4), p.get("xgboost_dart_mode", False))


def fit(case, gradients=None, fault=None, params=None):
    """case: dict(params, rounds, boosting, data: dict(X, y, bins, edges, nbins, nan_bin, is_cat, qid)).  Drives `rounds` rounds with unit
    Hessians; gradients(r, scores) -> the round's fp32 gradients at `scores` (the resident scores with the round's dropped trees
    subtracted).  The default takes squared error at the restatement's own scores; a GPU test hands the device's own gradients, so that
    a difference cannot compound.  -> (the trees with their final values, per round dict(tree: as born, mask, add, margin, stats, drop, lr,
    factor, at: the scores the gradients were taken at, scores: after the round))."""
    d, p = case["data"], dict(case["params"] if params is None else params)
    gradients = squared_error(d["y"]) if gradients is None else gradients
    n = d["bins"].shape[0]
    sel = selection(case)
    scores, trees, per_tree, out = np.zeros(n, np.float32), [], [], []
    ones = np.ones(n, np.float32)
    for r in range(case["rounds"]):
        drop, lr, factor = sel[r] if sel is not None else ([], None, 1.0)
        at = D.walk(scores, per_tree, drop, -1) if drop else scores
        g = np.asarray(gradients(r, at), np.float32)
        tree, mask, add, margin, stats = grow(d["X"], d["bins"], g, ones, d["edges"], d["nbins"], d["nan_bin"], d["is_cat"], p, r, d["qid"], lr, fault)
        scores = (at + add).astype(np.float32)
        born = {k: np.array(v) for k, v in tree.items()}
        trees.append(tree)
        per_tree.append(add)
        if drop:                                                          # the dropped trees come back rescaled: float32(float64(value) * factor)
            for k in drop:
                per_tree[k], trees[k]["value"] = D.scaled(per_tree[k], factor), D.scaled(trees[k]["value"], factor)
            scores = D.walk(scores, per_tree, drop, 1)
        out.append(dict(tree=born, mask=mask, add=add, margin=margin, stats=stats, drop=drop, lr=lr, factor=factor, at=at, scores=scores.copy()))
    return trees, out


# ---- comparisons
def with_cat(tree):
    return tree if "cat_index" in tree else dict(tree, cat_index=np.full(tree["feature"].size, -1, np.int32), cat_set=np.zeros((0, 4), np.int64))


def same_tree(got, want):
    """Bit for bit in test_gbdt_quant_gpu.same_tree's sense, over every array a tree of the booster keeps: feature, left, right, the bits of
    threshold and value, and where the booster keeps them default_left, cat_index and cat_set."""
    for k in TREE_KEYS:
        if k in got and not (k in want and np.asarray(got[k]).shape == np.asarray(want[k]).shape and np.asarray(got[k]).tobytes() == np.asarray(want[k], np.asarray(got[k]).dtype).tobytes()):
            return False
    return "default_left" in got or "default_left" not in want


def canonical(tree, X, nbins):
    """gbdt_cat_ref.canonical with the leaves' fp32 bits kept: (nodes sorted, leaves (value bits, rows) sorted)."""
    nodes, _ = CR.canonical(with_cat(tree), X, nbins)
    leaf = leaf_of_rows(X, tree)
    vb = np.asarray(tree["value"], np.float32).view(np.uint32).astype(np.int64)
    leaves = np.array(sorted((int(vb[l]), int((leaf == l).sum())) for l in range(vb.size)), np.int64).reshape(-1, 2)
    return nodes, leaves


def same_canonical(got, want, X, nbins):
    """Depth-wise against leaf-wise where the cap cannot bind: the same nodes (feature, kind, threshold bits, rows, direction, left codes)
    and the same leaves (value bits, rows), whatever their numbering."""
    a, b = canonical(got, X, nbins), canonical(want, X, nbins)
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def node_counts(tree, leaf_rows):
    """(rows per node, depth per node, rows per leaf, depth per leaf) from the leaves' row lists."""
    nn = tree["feature"].size
    count, depth = np.zeros(nn, np.int64), np.zeros(nn, np.int64)
    lcount, ldepth = np.array([r.size for r in leaf_rows], np.int64), np.zeros(len(leaf_rows), np.int64)

    def down(at, dep):
        if at < 0:
            ldepth[~at] = dep
            return lcount[~at]
        depth[at] = dep
        count[at] = down(int(tree["left"][at]), dep + 1) + down(int(tree["right"][at]), dep + 1)
        return count[at]
    if nn:
        down(0, 0)
    return count, depth, lcount, ldepth


def host_reads(tree, leaf_rows, params, dropped_before=False):
    """The device-to-host reads the docstrings of GBDT promise for one round, from the restated tree alone: the root read; leaf-wise one per
    split that is followed by a search (the cap not yet reached and a child that may split), depth-wise one per level whose children are
    searched; +1 under quant_train_renew_leaf; +1 under linear_tree; +1 where begin_round read a drop list (DART, any tree to drop)."""
    p = params
    count, depth, lcount, ldepth = node_counts(tree, leaf_rows)
    cap, md, floor = p["num_leaves"], option(p, "max_depth"), 2 * max(option(p, "min_data_in_leaf"), 1)
    kid = lambda c, dep: (count[c], dep) if c >= 0 else (lcount[~c], dep)
    can = lambda c, dep: bool(kid(c, dep)[0] >= floor and not (md > 0 and dep >= md))
    searched = [any(can(int(c), depth[k] + 1) for c in (tree["left"][k], tree["right"][k])) for k in range(tree["feature"].size)]
    reads = 1
    if p.get("grow_policy", "leafwise") == "depthwise":
        leaves = 1
        for dep in range(int(depth.max()) + 1 if depth.size else 0):
            level = np.nonzero(depth == dep)[0]
            leaves += level.size
            reads += int(leaves < cap and any(searched[k] for k in level))
    else:
        reads += sum(int(k + 2 < cap and searched[k]) for k in range(tree["feature"].size))
    return reads + int(renewed(p)) + int(bool(p.get("linear_tree", False))) + int(dropped_before)
