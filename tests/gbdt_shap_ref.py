"""Plain-numpy float64 restatements of the TreeSHAP contributions of the native booster (ptr_gbdt_shap of ptranking_amd/csrc/gbdt.hip;
include/ptranking_amd.h states the rule).  Test infrastructure, never imported by the package.  Two independent restatements:

  shap_exponential   the Shapley definition itself.  Over the M distinct features a tree uses,
                       phi_i = sum over S in M \\ {i} of |S|! (M - |S| - 1)! / M! [v(S + i) - v(S)],
                     v(S) the conditional expectation of the tree: follow x at the nodes whose feature is in S, take the cover-weighted mean
                     of both children at every other node.  2^M tree evaluations: M <= 12 or so.  It reads trees and leaf counts only.
  shap_polynomial    the per-leaf closed form over the SAME path tables the kernel reads (gbdt.shap_tables): the sum over subsets as the
                     Gauss-Legendre quadrature of prod_j (z_j (1 - t) + o_j t), in the kernel's own order of operations (float64,
                     nothing contracted), so that the kernel is expected to give its very bits.

A tree is a dict of feature / threshold / left / right / value, with default_left, cat_index and cat_set where the model has them (the
dicts of GBDT.trees).  "Goes left" restates the predicates of ptr_gbdt_predict / _missing / _cat on raw fp32 rows."""
import math

import numpy as np

# The gate: |got - oracle| <= C_SHAP x 2^-52 x sum over trees of max_l |v_l|, per element.  The need of shap_polynomial against
# shap_exponential on the trees of tests/test_gbdt_shap_cpu.py (M <= 8; numeric, NaN with default_left, categorical sets), in that unit, is
# NEED_POLYNOMIAL; C_SHAP = 2 x the need, rounded up to the next half, as C_METRIC was set (test_gbdt_shap_cpu.py measures both again).
NEED_POLYNOMIAL = 1.432  # measured: numeric 1.431, NaN with default_left 1.386, categorical sets 1.094
C_SHAP = 3.0             # = ceil_to_half(2 x 1.432)
UNIT = 2.0 ** -52


def constant_from_need(need):
    return math.ceil(2.0 * need * 2.0) / 2.0


def goes_left(tree, node, X):
    """bool [n]: which rows of X (float32 [n, F]) go left at a node."""
    f = int(tree["feature"][node])
    x = np.asarray(X, np.float32)[:, f]
    nan = np.isnan(x)
    dl = bool(tree["default_left"][node]) if "default_left" in tree else False
    if "cat_index" in tree and int(tree["cat_index"][node]) >= 0:
        words = np.asarray(tree["cat_set"][int(tree["cat_index"][node])]).astype(np.int64).view(np.uint64)
        code = np.where(nan, 0, x)
        ok = ~nan & (code >= 0) & (code <= 255) & (code == np.floor(code))
        c = np.where(ok, code, 0).astype(np.int64)
        bit = ((words[c >> 6] >> (c & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
        return np.where(nan, dl, ok & bit)
    with np.errstate(invalid="ignore"):
        return np.where(nan, dl, x <= np.float32(tree["threshold"][node]))


def leaf_of(tree, X):
    """int64 [n]: the leaf each row reaches."""
    n = np.asarray(X).shape[0]
    at = np.zeros(n, np.int64) if tree["feature"].size else np.full(n, ~0, np.int64)
    for _ in range(tree["feature"].size + 1):
        for node in np.unique(at[at >= 0]):
            rows = at == node
            gl = goes_left(tree, int(node), X)
            at[rows] = np.where(gl[rows], tree["left"][node], tree["right"][node])
    assert (at < 0).all()
    return ~at


def leaf_counts(tree, X):
    return np.bincount(leaf_of(tree, X), minlength=tree["feature"].size + 1).astype(np.int64)


def node_covers(tree, counts):
    """The rows below every node, from the leaf counts, by recursion over the children."""
    cover = np.zeros(tree["feature"].size, np.int64)

    def below(c):
        if c < 0:
            return int(counts[~c])
        cover[c] = below(int(tree["left"][c])) + below(int(tree["right"][c]))
        return int(cover[c])
    if tree["feature"].size:
        below(0)
    return cover


def shap_exponential(trees, counts, X, F):
    """float64 [n, F + 1] by the Shapley definition; counts: per tree the background's rows per leaf."""
    X = np.asarray(X, np.float32)
    n = X.shape[0]
    phi = np.zeros((n, F + 1))
    for tree, cnt in zip(trees, counts):
        nn = tree["feature"].size
        value = np.asarray(tree["value"], np.float32).astype(np.float64)
        cover = node_covers(tree, cnt)
        feats = sorted(set(int(f) for f in tree["feature"]))
        M = len(feats)
        go = [goes_left(tree, i, X) for i in range(nn)]
        size = lambda c: float(cnt[~c]) if c < 0 else float(cover[c])

        def expect(c, mask):
            if c < 0:
                return np.full(n, value[~c])
            lo, hi = int(tree["left"][c]), int(tree["right"][c])
            a, b = expect(lo, mask), expect(hi, mask)
            if mask >> feats.index(int(tree["feature"][c])) & 1:
                return np.where(go[c], a, b)
            return (size(lo) * a + size(hi) * b) / float(cover[c])
        v = [expect(0 if nn else ~0, mask) for mask in range(1 << M)]
        phi[:, F] += v[0]
        for i, f in enumerate(feats):
            acc = np.zeros(n)
            for mask in range(1 << M):
                if mask >> i & 1:
                    continue
                s = bin(mask).count("1")
                acc += math.factorial(s) * math.factorial(M - s - 1) / math.factorial(M) * (v[mask | 1 << i] - v[mask])
            phi[:, f] += acc
    return phi


def shap_polynomial(tables, trees, X, F, first_leaf=0, stop_leaf=None):
    """float64 [n, F + 1] from the path tables (gbdt.shap_tables) in the kernel's order of operations; the leaves first_leaf .. stop_leaf - 1."""
    X = np.asarray(X, np.float32)
    n = X.shape[0]
    offs = np.concatenate([[0], np.cumsum([t["feature"].size for t in trees])])
    owner = np.searchsorted(offs, np.arange(int(offs[-1])), side="right") - 1
    go = {}
    phi = np.zeros((n, F + 1))
    stop_leaf = tables["leaf_value"].size if stop_leaf is None else stop_leaf
    for l in range(first_leaf, stop_leaf):
        p0, p1 = int(tables["path_offsets"][l]), int(tables["path_offsets"][l + 1])
        e0, e1 = int(tables["elem_offsets"][l]), int(tables["elem_offsets"][l + 1])
        d = e1 - e0
        assert d <= 63
        o = np.ones((n, d), bool)
        for p in range(p0, p1):
            at = int(tables["path_node"][p])
            if at not in go:
                t = int(owner[at])
                go[at] = goes_left(trees[t], at - int(offs[t]), X)
            o[:, int(tables["path_elem"][p])] &= go[at] == bool(tables["path_dir"][p])
        z = tables["elem_z"][e0:e1].astype(np.float64)
        Q = (d + 1) >> 1
        off = Q * (Q - 1) // 2
        qt, qw = tables["quad_t"][off:off + Q].astype(np.float64), tables["quad_w"][off:off + Q].astype(np.float64)
        P = np.ones((n, Q))                                              # P[:, q] = prod_j (z_j (1 - t_q) + (o_j ? t_q : 0)), in element order
        pz = np.float64(1.0)
        for j in range(d):
            P = P * (z[j] * (1.0 - qt)[None, :] + np.where(o[:, j:j + 1], qt[None, :], 0.0))
            pz = pz * z[j]
        total = np.zeros((n, d))
        for q in range(Q):
            f = z[None, :] * (1.0 - qt[q]) + np.where(o, qt[q], 0.0)
            total = total + qw[q] * (P[:, q:q + 1] / f)
        v = np.float64(np.float32(tables["leaf_value"][l]))
        for e in range(d):
            f = int(tables["elem_feature"][e0 + e])
            phi[:, f] = phi[:, f] + (total[:, e] * (o[:, e].astype(np.float64) - z[e])) * v
        phi[:, F] = phi[:, F] + v * pz
    return phi


def bound(trees):
    """The unit of the gate: 2^-52 x the sum over the trees of the largest |leaf value|."""
    return UNIT * sum(float(np.abs(np.asarray(t["value"], np.float32).astype(np.float64)).max()) for t in trees)


def need(got, ref, trees):
    b = bound(trees)
    err = float(np.abs(np.asarray(got, np.float64) - ref).max()) if np.asarray(ref).size else 0.0
    return err / b if b > 0 else (0.0 if err == 0 else np.inf)


# ---- hand-built trees
def random_tree(rng, F, leaves, kind="numeric", cat_features=()):
    """A random binary tree of `leaves` leaves in the booster's layout (a split turns leaf l into a node whose left child keeps l, the right
    one takes the next leaf number).  kind: 'numeric', 'missing' (default_left per node) or 'cat' (set nodes on cat_features)."""
    feature, threshold, left, right, dl, ci, sets = [], [], [], [], [], [], []
    where = {0: (-1, 0)}                                                   # leaf -> (parent node, side)
    for k in range(leaves - 1):
        l = int(rng.integers(0, k + 1))
        node = len(feature)
        f = int(rng.integers(0, F))
        feature.append(f)
        left.append(~l)
        right.append(~(k + 1))
        dl.append(int(rng.integers(0, 2)))
        if kind == "cat" and f in cat_features:
            bits = int(rng.integers(1, 255))
            threshold.append(0.0)
            ci.append(len(sets))
            sets.append([bits, 0, 0, 0])
        else:
            threshold.append(float(rng.integers(-2, 3)) / 2 if f not in cat_features else float(rng.integers(0, 7)) + 0.5)
            ci.append(-1)
        par, side = where[l]
        if par >= 0:
            (left if side == 0 else right)[par] = node
        where[l], where[k + 1] = (node, 0), (node, 1)
    t = {"feature": np.array(feature, np.int32), "threshold": np.array(threshold, np.float32), "left": np.array(left, np.int32),
         "right": np.array(right, np.int32), "value": rng.standard_normal(leaves).astype(np.float32)}
    if kind in ("missing", "cat"):
        t["default_left"] = np.array(dl, np.uint8)
    if kind == "cat":
        t["cat_index"], t["cat_set"] = np.array(ci, np.int32), np.array(sets, np.int64).reshape(-1, 4)
    return t


def random_rows(rng, n, F, kind="numeric", cat_features=()):
    X = (rng.integers(-3, 4, (n, F)) / 2 + rng.integers(0, 2, (n, F)) / 4).astype(np.float32)
    for f in cat_features:
        X[:, f] = rng.integers(0, 8, n)
    if kind in ("missing", "cat"):
        X[rng.random((n, F)) < 0.15] = np.nan
    return X


def chain_tree(features, thresholds, values):
    """A chain: node i splits on features[i], its left child is leaf i, its right child node i + 1 (the last: leaf len(features))."""
    k = len(features)
    return {"feature": np.array(features, np.int32), "threshold": np.array(thresholds, np.float32),
            "left": np.array([~i for i in range(k)], np.int32), "right": np.array([i + 1 for i in range(k - 1)] + [~k], np.int32)[:k],
            "value": np.array(values, np.float32)}
