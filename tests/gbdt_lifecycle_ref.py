"""Numpy restatement of what carries a trained GBDT onto new data (include/ptranking_amd.h, the section 'A trained model on new data'):
the walk of raw fp32 rows to a LEAF INDEX with the missing and categorical rules of ptr_gbdt_predict / _missing / _cat, the per-leaf integer
sums of ptr_gbdt_leaf_sums, and the refit value rule of GBDT.refit in its stated order of operations.  Nothing here imports the package; the quantization is the restatement of tests/gbdt_ref.py.

A tree is a dict of numpy arrays as GBDT keeps one: feature, threshold, left, right [nodes] (a child c < 0 is the leaf ~c), value
[nodes + 1]; under use_missing default_left [nodes]; with categorical features cat_index [nodes] (-1: numeric) and cat_set [sets, 4] int64
(256 bits per set)."""
import numpy as np

import gbdt_ref as R


def in_set(cat_set, code):
    word = np.asarray(cat_set, np.int64).view(np.uint64)[code >> 6]
    return bool((int(word) >> (code & 63)) & 1)


def goes_left(tree, node, x, is_cat=None):
    """How one raw value decides at a node -> True (left), False (right) or None (a malformed node: its kind is not its feature's, or its
    set does not exist)."""
    f = int(tree["feature"][node])
    xv = np.float32(x[f])
    dl = bool(tree["default_left"][node]) if "default_left" in tree else False
    ci = int(tree["cat_index"][node]) if "cat_index" in tree else -1
    col_is_cat = bool(is_cat[f]) if is_cat is not None else False
    if "cat_index" in tree:
        if (ci >= 0) != col_is_cat or ci >= np.asarray(tree["cat_set"]).reshape(-1, 4).shape[0]:
            return None
    if ci >= 0:
        if np.isnan(xv):
            return dl                                                      # a NaN follows the node's direction
        if not 0.0 <= xv <= 255.0 or xv != np.floor(xv):
            return False                                                   # what is no code 0 .. 255 is in no set
        return in_set(np.asarray(tree["cat_set"]).reshape(-1, 4)[ci], int(xv))     # a code the training data never held is in no set: right
    if np.isnan(xv):
        return dl if "default_left" in tree else False                    # without directions a NaN fails x <= threshold: right
    return bool(xv <= np.float32(tree["threshold"][node]))


def leaf_of_row(tree, x, is_cat=None, nleaves=None):
    """The leaf index one row ends in; a tree of no node gives 0; -1 where the tree loses the row (a child or a feature out of range, a
    walk of more steps than nodes, a malformed categorical node) or where the index is >= nleaves."""
    nn = np.asarray(tree["feature"]).size
    nleaves = nn + 1 if nleaves is None else nleaves
    node, lost = (0 if nn else ~0), False
    for _ in range(nn):
        if node < 0 or node >= nn:
            break
        f = int(tree["feature"][node])
        if f < 0 or f >= len(x):
            break
        way = goes_left(tree, node, x, is_cat)
        if way is None:
            lost, way = True, False
        node = int(tree["left"][node]) if way else int(tree["right"][node])
    if lost or node >= 0 or ~node > nn or ~node >= nleaves:
        return -1
    return ~node


def leaf_index(tree, X, is_cat=None, nleaves=None):
    """leaf_of_row over a matrix -> int32 [n]."""
    X = np.asarray(X, np.float32)
    return np.array([leaf_of_row(tree, x, is_cat, nleaves) for x in X], np.int32).reshape(-1)


def leaf_index_numeric(tree, X, nleaves=None):
    """leaf_index for a tree of numeric nodes without directions, vectorised over the rows (the rows leave the loop as they land): what
    the large hand-built chains of the GPU test need.  test_gbdt_lifecycle_cpu.py pins it to leaf_index."""
    X = np.asarray(X, np.float32)
    feature, left, right = (np.asarray(tree[k]).astype(np.int64) for k in ("feature", "left", "right"))
    thr = np.asarray(tree["threshold"], np.float32)
    nn, n = feature.size, X.shape[0]
    nleaves = nn + 1 if nleaves is None else nleaves
    node = np.full(n, 0 if nn else ~0, np.int64)
    for _ in range(nn):
        live = np.nonzero((node >= 0) & (node < nn))[0]
        live = live[(feature[node[live]] >= 0) & (feature[node[live]] < X.shape[1])]
        if live.size == 0:
            break
        at = node[live]
        xv = X[live, feature[at]]
        node[live] = np.where(xv <= thr[at], left[at], right[at])          # a NaN compares false: right
    # a row still on a node, or on one whose feature is out of range, is lost
    ok = (node < 0) & (~node <= nn) & (~node < nleaves)
    return np.where(ok, ~node, -1).astype(np.int32)


def pred_leaf(trees, X, is_cat=None):
    """LightGBM's pred_leaf layout: int32 [n, trees]."""
    X = np.asarray(X, np.float32)
    return (np.stack([leaf_index(t, X, is_cat) for t in trees], axis=1) if trees else np.zeros((X.shape[0], 0))).astype(np.int32)


def leaf_sums(leaf, qg, qh, nleaves):
    """(sum qg, sum qh, count) per leaf over the rows with 0 <= leaf < nleaves -> int64 [nleaves, 3]."""
    sums = np.zeros((nleaves, 3), np.int64)
    leaf = np.asarray(leaf).astype(np.int64)
    keep = (leaf >= 0) & (leaf < nleaves)
    np.add.at(sums[:, 0], leaf[keep], np.asarray(qg, np.int64)[keep])
    np.add.at(sums[:, 1], leaf[keep], np.asarray(qh, np.int64)[keep])
    np.add.at(sums[:, 2], leaf[keep], 1)
    return sums


def new_value(g_sum, h_sum, expo, lambda_l2, learning_rate):
    """-G / (H + lambda_l2) * learning_rate in float64, G and H from the integer sums by ldexp, or None where H + lambda_l2 <= 0."""
    G = np.ldexp(np.float64(int(g_sum)), -int(expo[0]))
    H = np.ldexp(np.float64(int(h_sum)), -int(expo[1]))
    den = H + np.float64(lambda_l2)
    if not den > 0.0:
        return None
    return (-G / den) * np.float64(learning_rate)


def refit_value(old, g_sum, h_sum, count, expo, lambda_l2, learning_rate, decay_rate):
    """float32(decay_rate * float64(old) + (1 - decay_rate) * new); a leaf no row reaches, or one with H + lambda_l2 <= 0, keeps old."""
    old = np.float32(old)
    new = new_value(g_sum, h_sum, expo, lambda_l2, learning_rate) if int(count) > 0 else None
    if new is None:
        return old
    d = np.float64(decay_rate)
    return np.float32(d * np.float64(old) + (np.float64(1.0) - d) * new)


def refit(trees, X, grad_hess, lambda_l2, learning_rate, decay_rate, is_cat=None):
    """GBDT.refit on the host: per tree, in order, grad_hess at the running fp32 scores (from zero) -> quantize -> leaf sums -> the value
    rule -> scores += value[leaf] in fp32.  grad_hess(scores float32 [n]) -> (g, h) float32 [n].  -> (value arrays, scores float32 [n])."""
    X = np.asarray(X, np.float32)
    scores = np.zeros(X.shape[0], np.float32)
    values = []
    for t in trees:
        g, h = grad_hess(scores)
        qg, qh, expo, _ = R.quantize(g, h)                                 # ptr_gbdt_quantize, as tests/gbdt_ref.py restates it
        leaf = leaf_index(t, X, is_cat)
        nl = np.asarray(t["value"]).size
        s = leaf_sums(leaf, qg, qh, nl)
        v = np.array([refit_value(t["value"][l], s[l, 0], s[l, 1], s[l, 2], expo, lambda_l2, learning_rate, decay_rate) for l in range(nl)], np.float32)
        values.append(v)
        hit = leaf >= 0
        scores[hit] = (scores[hit] + v[leaf[hit]]).astype(np.float32)
    return values, scores


def sum_leaf_values(trees, leaves):
    """value[leaf] summed in tree order in fp32 from 0: what predict gives."""
    s = np.zeros(leaves.shape[0], np.float32)
    for k, t in enumerate(trees):
        s = (s + np.asarray(t["value"], np.float32)[leaves[:, k]]).astype(np.float32)
    return s


def chain_tree(nleaves, F=1, lo=0.0, step=1.0):
    """A hand-built chain of nleaves leaves on feature 0: node i sends x <= lo + i step to leaf i and the rest to node i + 1; the last node's
    right child is leaf nleaves - 1.  nleaves = 1 is the tree of no node."""
    nn = nleaves - 1
    t = {"feature": np.zeros(nn, np.int32), "threshold": (lo + step * np.arange(nn)).astype(np.float32),
         "left": ~np.arange(nn, dtype=np.int32), "right": np.arange(1, nn + 1, dtype=np.int32),
         "value": np.linspace(-1.0, 1.0, nleaves).astype(np.float32)}
    if nn:
        t["right"][nn - 1] = ~nn
    return t
