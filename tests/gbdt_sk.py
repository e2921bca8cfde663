"""The whole-fit comparison of the gradient-boosted trees with scikit-learn (tests/golden/gbdt_sklearn.npz, written by
tests/golden/make_golden_gbdt_sklearn.py): the fixture's loader, the canonical form of a tree, the restatement driven round by round, and
the gate.  Test infrastructure, never imported by the package; it needs neither a GPU nor scikit-learn.

A case is a regression fit under squared error: every round's inputs are g = (score - y) * w and h = w in fp32 (w = 1 without weights),
from the scores sklearn starts at (its baseline).  Cases a - e are HistGradientBoostingRegressor fits, case f is one
DecisionTreeRegressor (the exact greedy best-first tree: baseline 0, learning rate 1).

Node numbering differs between the implementations, so trees are compared in a canonical form:
    nodes   float64 [K, 3]  the internal nodes' (feature, fp32 threshold, training rows under the node), sorted
    leaves  float64 [L, 2]  the leaves' (value, training rows), sorted
The nodes and the leaves' row counts must be EQUAL; a leaf value cannot be (sklearn sums fp32 gradients in float64 and keeps float64
values, this project sums integers and keeps fp32 values), so the values, like the predictions, are held to the gate."""
import os

import numpy as np

import gbdt_ref as R

FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gbdt_sklearn.npz")
PARAM_NAMES = ("max_bin", "num_leaves", "min_data_in_leaf", "learning_rate", "lambda_l2", "rounds", "max_depth", "exact_tree", "seed")
MIN_MARGIN = 1e-5        # the condition on the inputs: sklearn's gains carry about 1e-7 of relative noise (fp32 gradient sums)
FAULTS = ("newest_leaf", "no_l2", "larger_hist")

# The gate: |got - sklearn| <= C_GBDT_SK * 2^-24 * max(1, max |sklearn's scores of that round|).  The constant is twice the worst need of
# the RESTATEMENT against sklearn over every round and every fresh row of the fixture (test_gbdt_cpu.py re-measures it and prints it:
# 2.06, case b after its sixth round), rounded up to an integer; it is never taken from the kernels' output.
C_GBDT_SK = 5
NEED_RECORDED = 2.06


def load(path=None):
    """{case: dict(X fp32 [n, F], y fp32 [n], w fp32 [n] or None, params dict, baseline float64, nodes / leaves per round (canonical),
    staged float64 [rounds, n], fresh fp32 [m, F], fresh_pred float64 [m])}, and the sklearn version."""
    out = {}
    with np.load(path or FILE, allow_pickle=False) as z:
        version = str(z["sklearn_version"])
        for name in sorted({k.split("/")[0] for k in z.files if "/" in k}):
            g = lambda k: z[f"{name}/{k}"]
            p = dict(zip(PARAM_NAMES, g("params").tolist()))
            for k in PARAM_NAMES:
                if k not in ("learning_rate", "lambda_l2"):
                    p[k] = int(p[k])
            X = (g("codes").astype(np.float32) / np.float32(8.0))
            offs = g("tree_offsets")
            nodes, leaves = g("nodes"), g("leaves")
            out[name] = dict(X=X, codes=g("codes"), y=g("y64").astype(np.float32) / np.float32(64.0),
                             w=g("w16").astype(np.float32) / np.float32(16.0) if f"{name}/w16" in z.files else None, params=p,
                             baseline=float(g("baseline")), staged=g("staged"), fresh=g("fresh16").astype(np.float32) / np.float32(16.0),
                             fresh_pred=g("fresh_pred"),
                             nodes=[nodes[offs[r, 0]:offs[r + 1, 0]] for r in range(p["rounds"])],
                             leaves=[leaves[offs[r, 1]:offs[r + 1, 1]] for r in range(p["rounds"])])
    return out, version


def booster_params(p):
    """The fixture's parameters under the booster's names."""
    return {"max_bin": p["max_bin"], "num_leaves": p["num_leaves"], "min_data_in_leaf": p["min_data_in_leaf"], "learning_rate": p["learning_rate"],
            "lambda_l2": p["lambda_l2"], "max_depth": p["max_depth"]}


def midpoint_edges(codes, max_bin):
    """The edges implied by the codes: every feature has at most max_bin distinct values, so an edge lies at the midpoint of every two
    neighbouring values, (c1 + c2) / 16, exact in fp32."""
    edges = np.full((codes.shape[1], max_bin - 1), np.inf, np.float32)
    nbins = np.ones(codes.shape[1], np.int32)
    for f in range(codes.shape[1]):
        v = np.unique(codes[:, f]).astype(np.int64)
        assert v.size <= max_bin
        edges[f, :v.size - 1] = (v[:-1] + v[1:]).astype(np.float32) / np.float32(16.0)
        nbins[f] = v.size
    return edges, nbins


def sort_rows(a):
    """The rows of a 2-d array in ascending order: by the first column, then the second, ..."""
    a = np.asarray(a, np.float64)
    return a[np.lexsort(a.T[::-1])] if a.shape[0] else a


def canonical(tree, X):
    """(nodes [K, 3], leaves [L, 2]) of one of this project's trees (dict of feature / threshold / left / right / value): the training rows X
    are walked through it, left on x <= threshold.  A child's node number is above its parent's (node k is the k-th split)."""
    X = np.asarray(X, np.float32)
    k = tree["feature"].size
    at = {0: np.arange(X.shape[0])}
    node_rows, leaf_rows = np.zeros(k, np.int64), np.zeros(tree["value"].size, np.int64)
    if k == 0:
        leaf_rows[0] = X.shape[0]
    for i in range(k):
        rows = at.pop(i)
        node_rows[i] = rows.size
        go_left = X[rows, tree["feature"][i]] <= tree["threshold"][i]
        for child, part in ((int(tree["left"][i]), rows[go_left]), (int(tree["right"][i]), rows[~go_left])):
            if child >= 0:
                assert child > i
                at[child] = part
            else:
                leaf_rows[~child] = part.size
    nodes = np.stack([tree["feature"].astype(np.float64), tree["threshold"].astype(np.float64), node_rows.astype(np.float64)], axis=1)
    leaves = np.stack([tree["value"].astype(np.float64), leaf_rows.astype(np.float64)], axis=1)
    return sort_rows(nodes.reshape(-1, 3)), sort_rows(leaves)


def gate(ref):
    """The largest admissible |got - ref| for an array of sklearn's scores."""
    return C_GBDT_SK * need_unit(ref)


def need_unit(ref):
    return 2.0 ** -24 * max(1.0, float(np.abs(ref).max()))


def tree_mismatch(got_nodes, got_leaves, case, r):
    """None when a canonical tree equals round r of the fixture (nodes and leaf row counts exactly, leaf values within the gate of that
    round's scores), else a word on what differs."""
    nodes, leaves = case["nodes"][r], case["leaves"][r]
    if got_nodes.shape != nodes.shape or not np.array_equal(got_nodes, nodes):
        return "internal nodes"
    if got_leaves.shape != leaves.shape or not np.array_equal(got_leaves[:, 1], leaves[:, 1]):
        return "leaf row counts"
    if not (np.abs(got_leaves[:, 0] - leaves[:, 0]) <= gate(case["staged"][r])).all():
        return "leaf values"
    return None


def gradients(scores, y, w):
    """The round's fp32 inputs under squared error: g = (score - y) * w, h = w."""
    w = np.ones_like(y) if w is None else w
    return ((scores - y) * w).astype(np.float32), w.astype(np.float32)


def run_restatement(case, fault=None):
    """gbdt_ref.py driven round by round from the fixture's baseline -> (per round (tree, training scores fp32), fresh predictions fp32
    with the baseline added, the smallest margin of any split search)."""
    p, X, y, w = case["params"], case["X"], case["y"], case["w"]
    edges, nbins = R.bin_edges(X, p["max_bin"])
    bins = R.bin_matrix(X, edges, nbins)
    base = np.float32(case["baseline"])
    scores = np.full(X.shape[0], base, np.float32)
    rounds, worst = [], np.inf
    for _ in range(p["rounds"]):
        g, h = gradients(scores, y, w)
        qg, qh, expo, flag = R.quantize(g, h)
        assert flag == 0
        tree, leaf_rows, margin = R.grow_tree(bins, qg, qh, expo, edges, nbins, p["max_bin"], p["num_leaves"], p["learning_rate"], p["lambda_l2"],
                                              p["min_data_in_leaf"], 1e-3, 0.0, p["max_depth"], fault=fault)
        worst = min(worst, margin)
        scores = R.add_leaf_values(scores.copy(), leaf_rows, tree["value"])
        rounds.append((tree, scores))
    fresh = (R.predict(case["fresh"], [t for t, _ in rounds]) + base).astype(np.float32)
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
        unit = need_unit(case["staged"][r])
        leaf_need = max(leaf_need, float(np.abs(leaves[:, 0] - case["leaves"][r][:, 0]).max()) / unit)
        need = max(need, float(np.abs(scores.astype(np.float64) - case["staged"][r]).max()) / unit)
        if need > C_GBDT_SK and bad is None:
            bad = f"round {r}: training scores need {need:.2f}"
    n_fresh = float(np.abs(fresh.astype(np.float64) - case["fresh_pred"]).max()) / need_unit(case["fresh_pred"])
    need = max(need, n_fresh)
    if n_fresh > C_GBDT_SK and bad is None:
        bad = f"fresh rows need {n_fresh:.2f}"
    return bad, need, leaf_need, worst
